"""Numpy model of pcs_stream_read_dev's per-page fold, shared by the GPU tests."""
import numpy as np


def stream_fold(buf: np.ndarray) -> np.ndarray:
    """What pcs_stream_read_dev computes per 4 KiB page: lane g of the page's
    group folds its 16 pieces (bytes 256c + 16g) with xor/add, the 16 lanes
    xor-reduced; a partial page reads only its whole 16 B pieces."""
    nbytes = buf.nbytes - buf.nbytes % 16
    npg = (nbytes + 4095) // 4096
    pad = np.zeros(npg * 4096, dtype=np.uint8)
    pad[:nbytes] = buf[:nbytes]
    w = pad.view(np.uint32).reshape(npg, 16, 16, 4)  # page, chunk c, lane g, word
    x = np.bitwise_xor.reduce(w[..., 0], axis=1).astype(np.uint64)
    y = w[..., 1].astype(np.uint64).sum(axis=1) & 0xFFFFFFFF
    z = np.bitwise_xor.reduce(w[..., 2], axis=1).astype(np.uint64)
    ww = w[..., 3].astype(np.uint64).sum(axis=1) & 0xFFFFFFFF
    r = ((x ^ z) << np.uint64(32)) | ((y + ww) & np.uint64(0xFFFFFFFF))
    return np.bitwise_xor.reduce(r, axis=1)
