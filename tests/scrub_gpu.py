"""Helpers shared by the GPU scrub tests: uploads at a chosen base alignment,
garbage-filled outputs with sentinels past n and past n_listed, the checked
scrub call, and tuning that is restored on every exit path."""
import contextlib

import numpy as np
import torch

import eloqstore_amd as pcs

DEV = "cuda:0"
SENTINEL = 0x5A5A5A5A5A5A5A5A
PAD = 16  # output elements past n, which no call may write
CLS_FILL, TYPE_FILL = 0xEE, 0xDD


def to_dev(pg, offset=0):
    """The pages at byte `offset` of a fresh device buffer (allocations are
    256-byte aligned, so offset % 16 is the view's alignment)."""
    flat = torch.from_numpy(np.ascontiguousarray(pg).reshape(-1))
    buf = torch.empty(flat.numel() + 16, dtype=torch.uint8, device=DEV)
    view = buf[offset: offset + flat.numel()]
    view.copy_(flat)
    return view


def garbage(n, cap):
    """(cls, types, summary, list): cls and types PAD elements longer than n."""
    return (torch.full((n + PAD,), CLS_FILL, dtype=torch.uint8, device=DEV),
            torch.full((n + PAD,), TYPE_FILL, dtype=torch.uint8, device=DEV),
            torch.full((12,), 0x1234567, dtype=torch.int64, device=DEV),
            torch.from_numpy(np.full(max(cap, 1), SENTINEL, dtype=np.uint64).view(np.int64)).to(DEV))


def scrub_checked(dpages, P, n, want, cap=1024, reps=3, types=True):
    """reps calls into garbage-filled outputs, each compared with `want`
    (classes, types, summary, list as scrub_ref.classify returns them, at any
    cap >= this one).  Returns the n class bytes on the device."""
    wcls, wtypes, ws, wbad = want
    for _ in range(reps):
        cls, ty, summ, lst = garbage(n, cap)
        pcs.pages_scrub_async(dpages, P, n, cls, ty if types else False, summ, lst if cap else None, cap)
        torch.cuda.synchronize()
        got = pcs.summary_dict(summ.cpu().tolist())
        ws_cap = dict(ws, n_listed=min(ws["n_corrupt"], cap))
        assert got == ws_cap, (got, ws_cap)
        hcls, hty = cls.cpu().numpy(), ty.cpu().numpy()
        assert np.array_equal(hcls[:n], wcls), np.flatnonzero(hcls[:n] != wcls)[:8]
        assert (hcls[n:] == CLS_FILL).all()  # nothing is written past cls[n]
        if types:
            assert np.array_equal(hty[:n], wtypes), np.flatnonzero(hty[:n] != wtypes)[:8]
            assert (hty[n:] == TYPE_FILL).all()
        else:
            assert (hty == TYPE_FILL).all()  # a NULL type array leaves the caller's memory alone
        l = lst.cpu().numpy().view(np.uint64)
        k = got["n_listed"]
        assert np.array_equal(l[:k], wbad[:k])
        assert (l[k:] == SENTINEL).all()  # entries at n_listed and beyond are not written
    return cls[:n]


@contextlib.contextmanager
def tuning(values):
    """pcs_set_tuning for the block, every key restored on every exit path."""
    saved = {k: pcs.get_tuning(k) for k in values}
    try:
        for k, v in values.items():
            pcs.set_tuning(k, v)
        yield
    finally:
        for k, v in saved.items():
            pcs.set_tuning(k, v)
