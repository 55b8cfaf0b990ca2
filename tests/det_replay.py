"""NumPy replay of the deterministic hash-grid scatter's contract (include/mipsf.h, MIPSF_HG_DETERMINISTIC); no tests here.

Indices and weights come from the CPU oracle (oracle/tcnn_cpu.py: _cell_and_frac, _corner_tables, _grid_index).  Every
entry's contributions v = (double)w * (double)g are ordered by (sample, corner), cut into pieces of HG_DET_PIECE items, each
piece summed left to right in fp64 from +0, the piece sums added left to right in fp64 from +0, and the total rounded once
to fp32.  np.add.at applies its additions one after the other in index order: it is the sequential fp64 sum.

The oracle's _fma32 forms x * scale + 0.5 as an exact fp64 product plus an fp64 add, then rounds to fp32: a true fma (the
kernel's fmaf) whenever that add is exact.  It is not only when |scale * x| < 2^-6 with x != 0; ``det_backward`` checks the
TwoSum error of the add for every point and level, and ``move_tiny`` moves such points out of the way beforehand."""
import numpy as np
import torch

from oracle import tcnn_cpu

HG_DET_PIECE = 512


def _twosum_err(a: np.ndarray, b: float) -> np.ndarray:
    s = a + b
    bp = s - a
    ap = s - bp
    return (a - ap) + (b - bp)


def move_tiny(x: np.ndarray, meta) -> np.ndarray:
    """Points whose coordinate times some level's scale is below 2^-6 in magnitude (but not zero) are set to zero in that
    coordinate: the replay's fp64 emulation of the position fma is exact for every other point."""
    x = np.array(x, dtype=np.float32, copy=True)
    smin = min(meta.scales)
    tiny = (x != 0) & (np.abs(x.astype(np.float64) * smin) < 2.0 ** -6)
    x[tiny] = 0.0
    return x


def det_backward(x32: np.ndarray, dout: np.ndarray, meta, dparams_in: np.ndarray = None, zero: bool = True) -> np.ndarray:
    """x32 [M,3] fp32, dout [M, L, F] fp32 (per sample, level, feature) -> dparams [n_params] fp32 by the contract.
    zero: MIPSF_HG_DPARAMS_ZERO (dparams[e] = s); else dparams[e] = dparams_in[e] + s in fp32.  Entries without a
    contribution keep dparams_in (or +0 with `zero` and no dparams_in)."""
    M, L, F = dout.shape
    assert F == 2 and L == meta.n_levels
    x_t = torch.from_numpy(np.ascontiguousarray(x32, dtype=np.float32))
    keys, samples, corners, vals = [], [], [], []
    for level in range(L):
        off = meta.offsets[level]
        size = meta.offsets[level + 1] - off
        scale = meta.scales[level]
        prod = x32.astype(np.float64) * np.float64(np.float32(scale))
        err = _twosum_err(prod, 0.5)
        assert not np.any(err != 0), "a point's position fma is not exact in the fp64 emulation: move it (move_tiny)"
        cell, frac = tcnn_cpu._cell_and_frac(x_t, scale)
        cor, w = tcnn_cpu._corner_tables(cell, frac)
        idx = (tcnn_cpu._grid_index(cor, size, meta.resolutions[level]) + off).numpy()      # [M, 8]
        w = w.numpy()
        g = dout[:, level, :]
        live = ~((g[:, 0] == 0) & (g[:, 1] == 0))
        i = np.nonzero(live)[0]
        if i.size == 0:
            continue
        keys.append(idx[i].reshape(-1))
        samples.append(np.repeat(i, 8))
        corners.append(np.tile(np.arange(8), i.size))
        v = w[i].astype(np.float64)[:, :, None] * g[i].astype(np.float64)[:, None, :]       # [n, 8, 2], exact
        vals.append(v.reshape(-1, 2))
    n_entries = meta.offsets[L]
    out = np.zeros(n_entries * 2, dtype=np.float32) if dparams_in is None else np.array(dparams_in, dtype=np.float32, copy=True)
    out = out.reshape(n_entries, 2)
    if not keys:
        return out.reshape(-1)
    key = np.concatenate(keys).astype(np.int64)
    smp = np.concatenate(samples)
    cor = np.concatenate(corners)
    val = np.concatenate(vals)
    order = np.lexsort((cor, smp, key))               # by entry, then sample, then corner
    key, val = key[order], val[order]
    n = key.size
    head = np.ones(n, dtype=bool)
    head[1:] = key[1:] != key[:-1]
    start = np.maximum.accumulate(np.where(head, np.arange(n), 0))
    rank = np.arange(n) - start
    new_piece = head | (rank % HG_DET_PIECE == 0)
    piece = np.cumsum(new_piece) - 1                  # piece id in order
    psum = np.zeros((piece[-1] + 1, 2), dtype=np.float64)
    np.add.at(psum, piece, val)                       # each piece left to right from +0
    piece_key = key[new_piece]
    ent = np.cumsum(head[new_piece]) - 1              # entry ordinal of each piece
    tot = np.zeros((ent[-1] + 1, 2), dtype=np.float64)
    np.add.at(tot, ent, psum)                         # the piece sums left to right from +0
    ekeys = piece_key[head[new_piece]]
    s = tot.astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        out[ekeys] = s if zero else (out[ekeys] + s).astype(np.float32)
    return out.reshape(-1)
