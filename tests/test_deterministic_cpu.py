"""CPU: the deterministic hash-grid scatter's contract (include/mipsf.h, MIPSF_HG_DETERMINISTIC) as replayed by
tests/det_replay.py agrees with the oracle's scatter; its scratch size query and its constants agree between the library,
_lib.py and the header."""
import os
import re

import numpy as np
import pytest
import torch

from oracle import tcnn_cpu

from . import det_replay

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_defines():
    with open(os.path.join(ROOT, "include", "mipsf.h")) as f:
        text = f.read()
    return {m.group(1): m.group(2) for m in re.finditer(r"^#define (MIPSF_\w+) +(\S+)", text, re.M)}


def _case(seed, M, log2_size, spread=False):
    rng = np.random.default_rng(seed)
    meta = tcnn_cpu.make_grid_meta(n_levels=8, log2_hashmap_size=log2_size, base_resolution=4, per_level_scale=1.8)
    x = rng.uniform(0.0, 1.0, (M, 3)).astype(np.float32)
    x[: M // 8] = rng.uniform(-2.0, 3.0, (M // 8, 3)).astype(np.float32)            # outside the box
    k = M // 8
    x[k: 2 * k] = x[2 * k: 3 * k]                                                    # duplicates
    x = det_replay.move_tiny(x, meta)
    g = rng.standard_normal((M, meta.n_levels, 2)).astype(np.float32)
    if spread:
        g *= np.exp2(rng.uniform(-20, 20, g.shape)).astype(np.float32)
    g[M // 2:, 3:] = 0.0                                                             # dead pairs
    g[-M // 8:] = 0.0                                                                # a dead tail
    return meta, x, g


@pytest.mark.parametrize("seed,M,log2_size,spread", [(0, 300, 10, False), (1, 2000, 14, True), (2, 1500, 12, False)])
def test_replay_agrees_with_the_oracle_scatter(seed, M, log2_size, spread):
    meta, x, g = _case(seed, M, log2_size, spread)
    got = det_replay.det_backward(x, g, meta)
    ref, _ = tcnn_cpu.hashgrid_backward(torch.from_numpy(x), torch.zeros(meta.n_params), torch.from_numpy(g.reshape(M, -1)),
                                        meta, need_dx=False)
    ref = ref.numpy()
    scale = float(np.abs(ref).max())
    assert scale > 0
    assert float(np.abs(got - ref).max()) <= 1e-6 * scale
    assert np.array_equal(got == 0, ref == 0)


def test_replay_piece_rule_and_accumulate():
    """A coarse grid of one level: thousands of contributions per entry (several pieces); accumulation adds in fp32."""
    meta = tcnn_cpu.make_grid_meta(n_levels=1, log2_hashmap_size=10, base_resolution=2, per_level_scale=1.5)
    rng = np.random.default_rng(7)
    M = 3000
    x = det_replay.move_tiny(rng.uniform(0.0, 1.0, (M, 3)).astype(np.float32), meta)
    g = rng.standard_normal((M, 1, 2)).astype(np.float32)
    got = det_replay.det_backward(x, g, meta)
    ref, _ = tcnn_cpu.hashgrid_backward(torch.from_numpy(x), torch.zeros(meta.n_params), torch.from_numpy(g.reshape(M, -1)),
                                        meta, need_dx=False)
    assert float(np.abs(got - ref.numpy()).max()) <= 1e-6 * float(np.abs(ref.numpy()).max())
    base = rng.standard_normal(meta.n_params).astype(np.float32)
    acc = det_replay.det_backward(x, g, meta, dparams_in=base, zero=False)
    touched = got != 0
    assert np.array_equal(acc[touched], (base[touched] + got[touched]).astype(np.float32))
    assert np.array_equal(acc[~touched], base[~touched])


def test_det_scratch_size_is_sane():
    from mipsfusion_amd import _lib
    meta = _lib.make_grid_meta(n_levels=16, n_features=2, log2_hashmap_size=19, base_resolution=16, per_level_scale=1.38)
    M = 262144
    n = _lib.buffer_size(_lib.SIZE_HASHGRID_DET_SCRATCH, M, 0, 0, meta)
    n_dx = _lib.buffer_size(_lib.SIZE_HASHGRID_DET_SCRATCH, M, 1, 0, meta)
    items = 8 * 16 * M
    assert 4 * items <= n <= 5 * items                 # two key and two value arrays, counts, starts, piece sums
    assert n_dx - n == 16 * M * 3
    assert _lib.buffer_size(_lib.SIZE_HASHGRID_DET_SCRATCH, 0, 0, 0, meta) < 1 << 24
    assert _lib.buffer_size(_lib.SIZE_HASHGRID_DET_SCRATCH, 2 * M, 0, 0, meta) > n


def test_constants_agree_with_the_header():
    from mipsfusion_amd import _lib, ops
    d = _header_defines()
    assert int(d["MIPSF_ABI_VERSION"]) == 2 == _lib.lib().mipsf_abi_version()
    assert int(d["MIPSF_HG_DPARAMS_ZERO"].rstrip("u")) == _lib.HG_DPARAMS_ZERO == ops.HG_DPARAMS_ZERO
    assert int(d["MIPSF_HG_ROUTED"].rstrip("u")) == _lib.HG_ROUTED == ops.HG_ROUTED
    assert int(d["MIPSF_HG_DETERMINISTIC"].rstrip("u")) == _lib.HG_DETERMINISTIC == ops.HG_DETERMINISTIC
    assert int(d["MIPSF_HG_DET_PIECE"]) == _lib.HG_DET_PIECE == det_replay.HG_DET_PIECE
    assert int(d["MIPSF_SIZE_HASHGRID_DET_SCRATCH"]) == _lib.SIZE_HASHGRID_DET_SCRATCH
    assert d["MIPSF_HG_DET_MAX_ITEMS"] == "(1ull" and _lib.HG_DET_MAX_ITEMS == 1 << 31
    assert d["MIPSF_TILE_ORDER_MAX_M"] == "(1u" and _lib.TILE_ORDER_MAX_M == 1 << 27
    assert int(d["MIPSF_WGRAD_LEAN_DACT"].rstrip("u")) == _lib.WGRAD_LEAN_DACT
    assert int(d["MIPSF_WGRAD_DETERMINISTIC"].rstrip("u")) == _lib.WGRAD_DETERMINISTIC


def test_deterministic_attribute_follows_torch():
    from mipsfusion_amd import ops
    prev = torch.are_deterministic_algorithms_enabled()
    try:
        torch.use_deterministic_algorithms(True)
        assert ops.resolve_deterministic(None) is True
        assert ops.resolve_deterministic(False) is False
        torch.use_deterministic_algorithms(False)
        assert ops.resolve_deterministic(None) is False
        assert ops.resolve_deterministic(True) is True
    finally:
        torch.use_deterministic_algorithms(prev)
