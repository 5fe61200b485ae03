"""bench.py's N = 1 line carries what the driver and the judge read: the
headline metric with its roofline and ms_per_step in a plain run (which can
dump the last timed step's outputs); with --full also parity and the
corruption drill, and the sweep over every other BASELINE config and mode
(VERDICT r01 #2), each entry with its launch time, frac, parity against the
reference build and a drill.  Run at reduced sizes (--pages-per-gpu,
--sweep-scale) so it takes seconds."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWEEP_KEYS = ["config3_xxh3", "config3_xxh64", "config4_xxh3", "config5_xxh3", "config7_xxh3",
              "config2_xxh3_validate", "config2_xxh3_stamp"]


def test_bench_line_and_sweep():
    r = subprocess.run([sys.executable, "bench.py", "--full", "--steps", "5", "--warmup", "2", "--pages-per-gpu", "65536",
                        "--sweep-steps", "3", "--sweep-warmup", "1", "--sweep-scale", "16", "--no-cpu-baseline",
                        "--no-host-inclusive"],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["metric"] == "GiB/s device-resident batched page XXH3-64, 4 KiB pages, 1/2/4/8 MI355X"
    assert d["unit"] == "GiB/s" and d["n_gpus"] == 1 and d["value"] > 0 and d["higher_is_better"]
    assert d["scaling"] == "weak" and d["dtype"] == "u64"
    roof = d["roofline"]
    assert roof["bound"] == "hbm" and roof["unit"] == "GB/s" and roof["peak"] == 8000.0
    assert 0 < roof["frac"] < 1.0 and abs(roof["frac"] - roof["achieved"] / roof["peak"]) < 1e-3
    assert d["parity"]["mismatches"] == 0 and d["parity"]["pages"] > 0
    assert d["corruption_drill"]["pass"]
    assert d["stream_read_GBps"] > 0
    # the ceiling and the hash kernel under one protocol
    ceil = d["ceiling"]
    assert ceil["stream_read_GBps"] == d["stream_read_GBps"] and 0.5 < ceil["frac_of_ceiling"] < 1.5, ceil
    assert roof["frac_of_ceiling"] > 0
    # the driver's protocol at process start, before the settle
    assert d["cold"]["value"] > 0 and d["cold"]["steps"] == 5 and d["cold"]["warmup"] == 2 and d["cold"]["frac"] > 0
    assert "host_inclusive" not in d
    # untimed steps ran for the default 1.5 s before the warmup
    assert d["settle"]["ms"] == 1500.0 and d["settle"]["steps"] >= 8 and d["settle"]["steps"] % 8 == 0
    assert [e["key"] for e in d["sweep"]] == SWEEP_KEYS
    for e in d["sweep"]:
        assert e["avg_launch_ms"] > 0 and 0 < e["frac"] < 1.0, e
        assert e["parity"]["mismatches"] == 0 and e["parity"]["pages"] > 0, e
        assert e["corruption_drill"]["pass"], e
        assert e["steps"] == 3 and e["warmup"] == 1
    # config-2 entries ran on the headline's batch (resident, not re-allocated)
    assert [e["pages"] for e in d["sweep"] if e["config"] == 2] == [65536, 65536]


def _one_line(r):
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_config1_leg_on_the_real_file():
    """BASELINE configs[0]: the GPU CLI writes and stamps the 1 GiB file, the
    reference's own xxHash validates every page on one thread, the repo's C
    restatement re-digests them, and the CLI's --scan scrubs the file: all
    must agree (tools/page_checksum_tool.cpp:94-105, page.cpp:25-31)."""
    d = _one_line(subprocess.run([sys.executable, "bench.py", "--config", "1", "--cpu-seconds", "1"],
                                 cwd=ROOT, capture_output=True, text=True, timeout=300))
    assert "error" not in d, d
    one = d["cpu_baseline"]
    assert one["kind"] == "reference" and one["cores"] == 1 and one["value"] > 0
    assert one["pages_failed"] == 0
    assert d["cpu_port"]["pages_failed"] == 0 and d["cpu_port"]["value"] > 0
    assert d["cpu_ref_inmem"]["pages_failed"] == 0 and d["cpu_ref_inmem"]["cores"] == 1
    assert d["cli_scan"]["rc"] == 0, d["cli_scan"]
    # every usable core: pread loop and in-memory pages
    for k in ("cpu_all_cores", "cpu_ref_inmem_all_cores"):
        assert d[k]["pages_failed"] == 0 and d[k]["cores"] >= 1 and d[k]["value"] > 0, d[k]
    assert d["cpu_ref_inmem_all_cores"]["cores"] == d["cpu_all_cores"]["cores"]
    assert not os.listdir(os.path.join(ROOT, ".bench_tmp")), "config-1 file left behind"


def test_bench_line_survives_failing_config1():
    env = dict(os.environ, PCS_BENCH_FAIL_CONFIG1="1")
    d = _one_line(subprocess.run([sys.executable, "bench.py", "--full", "--steps", "5", "--warmup", "2", "--pages-per-gpu",
                                  "65536", "--no-sweep", "--host-inclusive"], cwd=ROOT, env=env,
                                 capture_output=True, text=True, timeout=300))
    assert "PCS_BENCH_FAIL_CONFIG1" in d["config1_error"]
    assert d["cpu_baseline"] is None
    assert d["roofline"]["frac"] > 0 and d["parity"]["mismatches"] == 0
    hi = d["host_inclusive"]
    assert hi["parity_mismatches"] == 0 and set(hi["legs"]) == {"direct_pinned", "gather_pageable",
                                                                "gather_scattered", "zero_copy_scattered"}
    for leg in hi["legs"].values():
        assert leg["GiBps"] > 0 and 0 < leg["frac_of_pcie"] < 1.5 and leg["parity_mismatches"] == 0, leg


def test_host_inclusive_runs_by_default():
    """the N=1 --full line carries the host-inclusive legs without being asked for them."""
    d = _one_line(subprocess.run([sys.executable, "bench.py", "--full", "--steps", "5", "--warmup", "2", "--pages-per-gpu",
                                  "65536", "--no-sweep", "--no-cpu-baseline", "--no-live-traffic"], cwd=ROOT,
                                 capture_output=True, text=True, timeout=300))
    assert d["host_inclusive"]["parity_mismatches"] == 0 and d["host_inclusive"]["pages"] == 65536


def test_bench_wall_budget_skips_optional_legs():
    d = _one_line(subprocess.run([sys.executable, "bench.py", "--full", "--steps", "5", "--warmup", "2", "--pages-per-gpu",
                                  "65536", "--sweep-scale", "16", "--wall-budget", "0"], cwd=ROOT,
                                 capture_output=True, text=True, timeout=300))
    assert "wall budget" in d["config1_skipped"]
    assert [e["key"] for e in d["sweep"]] == SWEEP_KEYS and all("skipped" in e for e in d["sweep"])
    assert d["roofline"]["frac"] > 0


def test_live_traffic_leg():
    """At the default headline workload, roofline.traffic comes from two
    rocprofv3 --pmc passes (FETCH_SIZE, WRITE_SIZE) over the headline kernel in
    this very run, corrected for gfx950; on this streaming kernel it equals
    the algorithmic bytes."""
    d = _one_line(subprocess.run([sys.executable, "bench.py", "--full", "--steps", "5", "--warmup", "2", "--no-sweep",
                                  "--no-cpu-baseline"], cwd=ROOT, capture_output=True, text=True, timeout=300))
    roof = d["roofline"]
    live = roof["traffic_live"]
    assert live and "error" not in live, live
    assert roof["traffic_source"].startswith("live:") and roof["traffic"] == live["traffic"]
    assert 0.98 < roof["traffic"] / roof["algorithmic_bytes_per_launch"] < 1.05, roof
    assert live["dispatches"]["FETCH_SIZE"] >= 3 and live["dispatches"]["WRITE_SIZE"] >= 3


FULL_ONLY = ("cold", "parity", "corruption_drill", "ceiling", "stream_read_GBps", "cpu_baseline", "host_inclusive",
             "sweep", "checks_all_ranks_pass")


def _u64(halves):
    assert halves.dtype == np.float64 and halves.ndim == 2 and halves.shape[1] == 2
    return halves[:, 0].astype(np.uint64) | (halves[:, 1].astype(np.uint64) << np.uint64(32))


def test_plain_run_is_the_headline_only_and_dumps_its_digests(tmp_path):
    """Without --full: W warmup and K timed steps, one line with the headline
    fields and ms_per_step, none of the legs that take runs of their own; and
    --dump-outputs writes the last timed step's digests (low and high 32 bits
    as exact float64 pairs), which are the oracle's digests of the generator's
    pages for this seed."""
    import oracle
    from workload import fill_pages

    n = 4097
    d = _one_line(subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1",
                                  "--pages-per-gpu", str(n), "--dump-outputs", str(tmp_path / "out")], cwd=ROOT,
                                 capture_output=True, text=True, timeout=120))
    assert d["metric"] == "GiB/s device-resident batched page XXH3-64, 4 KiB pages, 1/2/4/8 MI355X"
    assert d["unit"] == "GiB/s" and d["higher_is_better"] is True and d["dtype"] == "u64" and d["full"] is False
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0
    # value = bytes per step / the wall time of one step
    assert abs(d["value"] - n * 4096 / (d["ms_per_step"] / 1e3) / 2**30) <= 0.02 * d["value"]
    assert d["roofline"]["frac"] > 0 and d["roofline"]["avg_launch_ms"] > 0
    assert not [k for k in FULL_ONLY if k in d], d.keys()
    assert os.listdir(tmp_path / "out") == ["digests.npy"]
    got = _u64(np.load(tmp_path / "out" / "digests.npy"))
    assert np.array_equal(got, oracle.pages_digest(fill_pages(0x5EED0002, 0, n, 4096).reshape(-1), 4096))


def test_timed_outputs_of_every_mode(tmp_path, monkeypatch):
    """bench.timed_outputs: validate leaves verdicts and the first bad index,
    stamp the headers it wrote (fixed and mixed page sizes), all float32 or
    float64; bench.dump_outputs writes one .npy per array."""
    import bench
    import oracle

    w = bench.Workload(2, 0, 0, 1000, "cuda:0")
    w.step("stamp")
    hdr = bench.timed_outputs(w, "stamp")
    want = oracle.pages_digest(w.pages.cpu().numpy(), 4096)
    assert list(hdr) == ["headers"] and np.array_equal(_u64(hdr["headers"]), want)
    w.pages[3 * 4096 + 10] ^= 0xFF
    w.step("validate")
    out = bench.timed_outputs(w, "validate")
    assert out["ok"].dtype == np.float32 and out["ok"].shape == (1000,)
    assert out["ok"].sum() == 999 and out["ok"][3] == 0 and out["first_bad"].tolist() == [3.0]
    m = bench.Workload(3, 0, 0, 300, "cuda:0")
    m.step("stamp")
    got = _u64(bench.timed_outputs(m, "stamp")["headers"])
    assert np.array_equal(got, oracle.desc_digest(m.pages.cpu().numpy(), m.offs, m.lens))
    # an output larger than DUMP_MAX_ROWS: the same seeded, sorted sample of rows in every call
    monkeypatch.setattr(bench, "DUMP_MAX_ROWS", 256)
    a, b = bench.timed_outputs(w, "stamp"), bench.timed_outputs(m, "stamp")
    idx = a["sample_index"].astype(np.int64)
    assert len(np.unique(idx)) == 256 and (np.diff(idx) > 0).all() and idx.max() < 1000
    assert np.array_equal(_u64(a["headers"]), _u64(hdr["headers"])[idx])
    assert np.array_equal(_u64(b["headers"]), got[b["sample_index"].astype(np.int64)])
    w.step("digest")
    d = bench.timed_outputs(w, "digest")
    assert np.array_equal(d["sample_index"], a["sample_index"])
    assert np.array_equal(_u64(d["digests"]), w.out.cpu().numpy().view(np.uint64)[idx])
    bench.dump_outputs(str(tmp_path / "o"), out, rank=1)
    assert sorted(os.listdir(tmp_path / "o")) == ["first_bad_rank1.npy", "ok_rank1.npy"]
    assert np.array_equal(np.load(tmp_path / "o" / "ok_rank1.npy"), out["ok"])
