"""GPU tests of the mesh evaluation (mipsfusion_amd/evaluate.py, csrc/eval.hip) against the float64 restatement of
tests/eval_cpu.py.  Both sides get the same fp32 words and evaluate the same integer and float64 expressions, so samples, faces,
areas, neighbours, squared distances and counts are compared for EQUALITY; only the two-stage sums carry a tolerance, the bound
n * 2^-53 (relative) that holds for any order of adding n non-negative terms.  tests/test_eval_cpu.py holds the restatement to
what is known without it and bounds the cost of the ring walk on the cases used here."""
import math

import numpy as np
import pytest
import torch

from mipsfusion_amd import _lib, evaluate as ev, mesh as mesh_mod, synth

from . import eval_cpu as E
from . import scene_mesh_cpu as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")
    return torch.device("cuda:0")


def _box_room():
    return synth.box_room_mesh(synth.config_reference_defaults()["mapping"]["bound"])


MESHES = {
    "box_room": _box_room,
    "square": lambda: E.mesh_square(0.25),
    "one_face": lambda: (np.array([[0.1, 0.2, 0.3], [1.3, 0.1, 0.7], [0.4, 1.5, -0.2]]), np.array([[0, 1, 2]])),
    "random_5000": E.mesh_random,
}


def _words(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------- 1. sampler
@pytest.mark.parametrize("name", sorted(MESHES))
def test_samples_equal_the_restatement(dev, name):
    v, f = MESHES[name]()
    v32 = np.asarray(v, np.float32)
    for seed in E.SAMPLE_SEEDS:
        for n in E.SAMPLE_NS:
            want_p, want_f, want_area = E.sample_surface(v32, f, n, seed)
            got_p, got_f, got_area = ev.sample_surface(v32, f, n, seed)
            assert got_p.dtype == torch.float32 and got_f.dtype == torch.int32 and got_p.device.type == "cuda"
            assert got_area == want_area, (name, n, seed)
            assert np.array_equal(got_f.cpu().numpy(), want_f), (name, n, seed)
            assert np.array_equal(_words(got_p.cpu().numpy()), _words(want_p)), (name, n, seed)


def _box_faces(m, first=None):
    v, f = E.tessellated_box((0, 0, 0), (3, 2, 1), m=m)
    return np.asarray(v, np.float32), f[:first]


# the prefix sum of the faces' areas (csrc/block_dev.h's device-wide scan, uint64, inclusive) around one tile of 1024 faces and
# on either side of 256 tiles: past them a thread of the one-block top scan owns two tile sums.  At m = 148 the restatement's
# 4096 samples land on 4096 distinct faces from index 66 to 262 838, so a wrong tile offset anywhere shows.
SCAN_EDGE_MESHES = {
    "1023_faces": lambda: _box_faces(10, 1023),
    "1024_faces": lambda: _box_faces(10, 1024),
    "1025_faces": lambda: _box_faces(10, 1025),
    "254_tiles": lambda: _box_faces(147),
    "257_tiles": lambda: _box_faces(148),
}


@pytest.mark.parametrize("name", sorted(SCAN_EDGE_MESHES))
def test_samples_equal_the_restatement_around_the_scan_tiles(dev, name):
    v32, f = SCAN_EDGE_MESHES[name]()
    assert f.shape[0] == {"1023_faces": 1023, "1024_faces": 1024, "1025_faces": 1025, "254_tiles": 259308, "257_tiles": 262848}[name]
    want_p, want_f, want_area = E.sample_surface(v32, f, 4096, 7)
    got_p, got_f, got_area = ev.sample_surface(v32, f, 4096, 7)
    assert got_area == want_area
    assert np.array_equal(got_f.cpu().numpy(), want_f)
    assert np.array_equal(_words(got_p.cpu().numpy()), _words(want_p))


def test_sampler_accepts_a_mesh_and_tensors(dev):
    v, f = _box_room()
    want = E.sample_surface(v.astype(np.float32), f, 1000, 3)
    m = mesh_mod.Mesh(v, f, None)
    for got in (ev.sample_surface(m, n=1000, seed=3), ev.sample_surface((v, f), n=1000, seed=3),
                ev.sample_surface(torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev), 1000, 3)):
        assert np.array_equal(_words(got[0].cpu().numpy()), _words(want[0])) and np.array_equal(got[1].cpu().numpy(), want[1])
        assert got[2] == want[2]


def test_sampler_refuses_what_has_no_area(dev):
    v = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [2.0, 0.0, 0.0], [0.0, 5000.0, 0.0], [5000.0, 0.0, 0.0]], device=dev)
    none = torch.zeros((0, 3), dtype=torch.int32, device=dev)
    with pytest.raises(RuntimeError, match="without faces"):               # refused on the host: nothing is launched
        ev.sample_enqueue(v, none, 16)
    with pytest.raises(ValueError, match="without faces"):
        ev.sample_surface(v, none, 16)
    flat = torch.tensor([[0, 1, 2], [0, 0, 1], [0, 1, 7], [-1, 1, 2]], dtype=torch.int32, device=dev)      # a line, a repeat, two bad indices
    big = torch.tensor([[0, 4, 3]], dtype=torch.int32, device=dev)                                        # 1.25e7 m^2 >= 2^23 m^2
    for faces, status, word in ((flat, _lib.EVAL_NO_AREA, "no area"), (big, _lib.EVAL_AREA_OVERFLOW, "2\\^23")):
        points = torch.full((16, 3), -7.0, device=dev)
        face_of = torch.full((16,), -7, dtype=torch.int32, device=dev)
        _, _, record = ev.sample_enqueue(v, faces, 16, 0, points, face_of)
        assert ev.read_sample_record(record).status == status
        assert bool((points == -7.0).all()) and bool((face_of == -7).all())      # the drawing kernel wrote nothing
        with pytest.raises(ValueError, match=word):
            ev.sample_surface(v, faces, 16)


def test_sampler_gives_the_same_bytes_twice(dev):
    v, f = E.mesh_random()
    vt, ft = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(torch.int32).to(dev)
    a, b = ev.sample_enqueue(vt, ft, 4097, 9), ev.sample_enqueue(vt, ft, 4097, 9)
    assert all(x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes() for x, y in zip(a, b))
    assert not torch.equal(a[0], ev.sample_enqueue(vt, ft, 4097, 10)[0])


# ------------------------------------------------------------------------------------------------------------- 2. nearest
@pytest.mark.parametrize("name", E.NEAREST_NAMES)
def test_nearest_equals_the_restatement(dev, name):
    src, tgt, kw, want_j, want_d2 = E.nearest_cases()[name]
    j, d2 = ev.nearest_distance(src, tgt, **kw)
    assert j.dtype == torch.int32 and d2.dtype == torch.float64 and j.shape == (len(src),)
    assert np.array_equal(j.cpu().numpy().astype(np.int64), want_j), name
    assert np.array_equal(d2.cpu().numpy(), want_d2), name


def test_nearest_does_not_depend_on_the_grid(dev):
    c = E.nearest_cases()
    src, tgt = c["room_1000"][:2]
    base = ev.nearest_distance(src, tgt)
    for kw in (c["one_cell"][2], c["fine"][2], {"max_cells": 1000}, {"min_edge": 0.5}):
        got = ev.nearest_distance(src, tgt, **kw)
        assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1]), kw


def test_nearest_of_points_without_a_position(dev):
    """a source coordinate that is NaN or infinite: -1 and inf for that point, nothing else disturbed, and the walk ends"""
    src, tgt, _, want_j, want_d2 = E.nearest_cases()["room_31"]
    bad = src.copy()
    bad[3, 1], bad[7, 0], bad[11, 2] = np.nan, np.inf, -np.inf
    j, d2 = ev.nearest_distance(bad, tgt)
    j, d2 = j.cpu().numpy(), d2.cpu().numpy()
    ok = np.ones(len(src), bool)
    ok[[3, 7, 11]] = False
    assert np.all(j[~ok] == -1) and np.all(np.isinf(d2[~ok]))
    assert np.array_equal(j[ok], want_j[ok]) and np.array_equal(d2[ok], want_d2[ok])
    empty = ev.nearest_distance(src[:0], tgt)
    assert empty[0].shape == (0,) and empty[1].shape == (0,)


# ------------------------------------------------------------------------------------------------------------- 3. statistics
def _sums_close(got, want, n):
    return abs(got - want) <= n * 2.0 ** -53 * abs(want)


@pytest.mark.parametrize("n", [0, 1, 1025, 100000])
def test_stats_equal_the_restatement(dev, n):
    g = np.random.default_rng(n)
    d2 = g.uniform(0.0, 0.02, n) ** 2 * g.choice([1.0, 1.0, 1.0, 400.0], n)
    if n > 2:
        d2[n // 2], d2[n // 3] = 0.05 * 0.05, 0.0                       # on the threshold: counted
    want = E.stats(d2, 0.05)
    got = ev.distance_stats(torch.from_numpy(d2).to(dev), 0.05)
    assert (got.within, got.finite) == (want["within"], want["finite"]) and got.finite == n
    assert got.max_d == want["max_d"]
    assert _sums_close(got.sum_d, want["sum_d"], n) and _sums_close(got.sum_d2, want["sum_d2"], n)


def test_stats_count_entries_that_are_not_finite_out(dev):
    """inf (an empty target) and NaN enter neither the sums, nor the maximum, nor `within`; `finite` counts the rest"""
    g = np.random.default_rng(1)
    d2 = g.uniform(0.0, 0.1, 5000) ** 2
    d2[::7], d2[3::101] = np.inf, np.nan
    want = E.stats(d2, 0.05)
    got = ev.distance_stats(torch.from_numpy(d2).to(dev), 0.05)
    assert want["finite"] == int(np.isfinite(d2).sum()) < 5000
    assert (got.within, got.finite, got.max_d) == (want["within"], want["finite"], want["max_d"])
    assert _sums_close(got.sum_d, want["sum_d"], 5000) and _sums_close(got.sum_d2, want["sum_d2"], 5000)
    all_inf = ev.distance_stats(torch.full((300,), float("inf"), dtype=torch.float64, device=dev), 0.05)
    assert all_inf == ev.DistanceStats(0.0, 0.0, 0.0, 0, 0)


# ------------------------------------------------------------------------------------------------------------- 4. end to end
def _check_metrics(got, want, n):
    print("device %s\nrestatement %s" % (got, {k: v for k, v in want.items() if not k.startswith("d2")}))
    for k in ("completion_ratio", "accuracy_ratio", "accuracy_max", "completion_max", "area_rec", "area_gt"):
        assert getattr(got, k) == want[k], k                              # counts, maxima and areas: equal
    for k in ("accuracy", "completion"):
        assert abs(getattr(got, k) - want[k]) <= n * 2.0 ** -53 * want[k], k
    assert abs(got.chamfer - want["chamfer"]) <= n * 2.0 ** -53 * want["chamfer"]
    assert got.n_samples == n


def test_metrics_of_the_shifted_box(dev):
    """2 cm along x; the ratios are exactly 1 at E.SHIFT_THRESHOLD (0.3: tests/test_eval_cpu.py says why it is not 0.05)"""
    rec, gt = E.shifted_box_pair()
    want = E.reconstruction_metrics(rec, gt, E.E2E_SAMPLES, E.SHIFT_THRESHOLD)
    got = ev.reconstruction_metrics(mesh_mod.Mesh(rec[0], rec[1], None), mesh_mod.Mesh(gt[0], gt[1], None), E.E2E_SAMPLES,
                                    E.SHIFT_THRESHOLD)
    _check_metrics(got, want, E.E2E_SAMPLES)
    assert got.accuracy >= 0 and got.completion_ratio == 1.0
    assert got.threshold == E.SHIFT_THRESHOLD


def test_metrics_of_the_marched_box(dev):
    """the device's marching cubes of the box room's analytic SDF on a 48^3 volume against the room's 12 triangles"""
    v, f = _box_room()
    lo, hi = v.min(0), v.max(0)
    pad = 0.25
    ticks = [torch.linspace(float(lo[d] - pad), float(hi[d] + pad), 48, dtype=torch.float64, device=dev) for d in range(3)]
    p = torch.stack(torch.meshgrid(*ticks, indexing="ij"), -1)
    tlo, thi = torch.from_numpy(lo).to(dev), torch.from_numpy(hi).to(dev)
    sdf = torch.minimum(p - tlo, thi - p).amin(-1).to(torch.float32).contiguous()           # positive inside the room
    mv, mf = mesh_mod.marching_cubes(sdf, 0.0, truncation=3.0)
    assert len(mf) > 1000
    step = np.array([(float(t[-1]) - float(t[0])) / 47.0 for t in ticks])
    world = np.array([float(t[0]) for t in ticks]) + mv * step
    want = E.reconstruction_metrics((world, mf), (v, f), E.E2E_SAMPLES, 0.05)
    got = ev.reconstruction_metrics(mesh_mod.Mesh(world, mf, None), mesh_mod.Mesh(v, f, None), E.E2E_SAMPLES, 0.05)
    _check_metrics(got, want, E.E2E_SAMPLES)
    assert abs(got.area_rec - got.area_gt) < 0.05 * got.area_gt             # the same room, its edges bevelled by the cubes


# ------------------------------------------------------------------------------------------------------------- 5. cull
def test_cull_keeps_the_faces_the_keyframes_saw(dev):
    c = E.cull_case()
    views = (c["kf_c2w"], c["kf_max_depth"], c["K"], c["W"], c["H"])
    v32 = c["vertices"].astype(np.float32)
    assert not S.ambiguous_points(v32, *views).any()                        # no vertex hangs on an fp32 rounding
    keep = S.point_mask(v32, *views)[c["faces"]].all(1)
    assert 0 < keep.sum() < len(keep)
    got = ev.cull_to_views(mesh_mod.Mesh(c["vertices"], c["faces"], None), *views)
    assert isinstance(got, mesh_mod.Mesh) and got.faces.dtype == np.int64
    assert np.array_equal(got.faces, c["faces"][keep]) and np.array_equal(got.vertices, c["vertices"])
    assert ev.sample_surface(got, n=500)[2] == E.sample_surface(v32, c["faces"][keep], 500)[2]
