"""The float64 restatement of the mesh evaluation (tests/eval_cpu.py) against things that are known without it, the ground-truth
meshes of mipsfusion_amd/synth.py, and the cost of the device's ring walk on the cases tests/test_gpu_eval.py runs."""
import math

import numpy as np
import pytest

from mipsfusion_amd import synth

from . import eval_cpu as E


def _barycentric(p, a, b, c):
    v0, v1, v2 = b - a, c - a, p - a
    d00, d01, d11, d20, d21 = v0 @ v0, v0 @ v1, v1 @ v1, v2 @ v0, v2 @ v1
    den = d00 * d11 - d01 * d01
    v, w = (d11 * d20 - d01 * d21) / den, (d00 * d21 - d01 * d20) / den
    return np.stack([1.0 - v - w, v, w], -1)


@pytest.mark.parametrize("name", ["triangle", "square"])
def test_samples_lie_in_their_faces(name):
    if name == "triangle":
        v, f = np.array([[0.1, 0.2, 0.3], [1.3, 0.1, 0.7], [0.4, 1.5, -0.2]]), np.array([[0, 1, 2]])
    else:
        v, f = E.mesh_square(0.25)
    v32 = v.astype(np.float32)
    pts, face_of, area = E.sample_surface(v32, f, 2000, seed=1)
    assert pts.dtype == np.float32 and face_of.dtype == np.int32 and pts.shape == (2000, 3)
    assert abs(area - E.mesh_area(v32.astype(np.float64), f)) <= len(f) * E.UNIT
    for k in range(len(f)):
        a, b, c = (v32[i].astype(np.float64) for i in f[k])
        p = pts[face_of == k].astype(np.float64)
        normal = np.cross(b - a, c - a)
        assert np.max(np.abs((p - a) @ normal) / np.linalg.norm(normal)) < 1e-6          # fp32 rounding of the point
        assert _barycentric(p, a, b, c).min() > -1e-6
    if name == "square":
        assert np.count_nonzero(face_of == 0) == 1000                                     # two faces of the same area


def test_face_counts_follow_the_areas():
    """Stratification: sample k's position lies in the k-th of n equal shares of the total.  A face owns one interval of the
    cumulative area; every share wholly inside it gives it exactly one sample, and at most 2 shares are cut by its two ends, each
    giving 0 or 1.  With e = n * area_f / total there are more than e - 2 and at most e whole shares, so |count - e| < 2 in exact
    arithmetic; the rounding of the position (relative 2^-51) can move a sample across an end only when it lies on it, which is
    the further 1 of the bound: |count - e| < 1 + 2."""
    v, f = E.mesh_random()
    units = np.array(E.face_units(v, f), np.float64)
    for n in (1000, 4096, 50000):
        _, face_of, _ = E.sample_surface(v, f, n, seed=7)
        counts = np.bincount(face_of, minlength=len(f))
        expect = n * units / units.sum()
        assert np.max(np.abs(counts - expect)) < 3.0
        assert counts[units == 0].sum() == 0


def test_degenerate_faces_are_never_chosen():
    v, f = E.mesh_random()
    units = np.array(E.face_units(v, f))
    bad = np.any((f < 0) | (f >= len(v)), axis=1)
    assert bad.sum() == 3 and np.all(units[bad] == 0)
    assert np.count_nonzero(units == 0) >= 28                   # 25 repeated vertices + 3 bad indices; collinear ones may keep a few units
    assert units.max() > 1e5 * np.median(units[units > 0])
    for seed in (0, 1):
        _, face_of, _ = E.sample_surface(v, f, 20000, seed)
        assert np.all(units[face_of] > 0) and not np.any(bad[face_of])
    with pytest.raises(E.SampleError):
        E.sample_surface(v, f[:0], 10)
    with pytest.raises(E.SampleError):
        E.sample_surface(v, np.array([[0, 0, 1], [-1, 2, 3]]), 10)
    with pytest.raises(E.SampleError):                           # 2^23 m^2 and more
        E.sample_surface(np.array([[0, 0, 0], [5000, 0, 0], [0, 5000, 0]], np.float32), np.array([[0, 1, 2]]), 10)


def test_uniforms_are_reproducible_and_uniform():
    k = np.arange(100000)
    u = E.uniforms(3, k, 1)
    assert u.min() >= 0.0 and u.max() < 1.0 and np.array_equal(u, E.uniforms(3, k, 1))
    assert abs(u.mean() - 0.5) < 0.01 and abs(np.corrcoef(u, E.uniforms(3, k, 2))[0, 1]) < 0.02
    assert not np.array_equal(u, E.uniforms(4, k, 1))
    assert int(E.hash_words(0, [0], 0)[0]) == 0                 # the hash of the zero word is zero: a fixed point worth knowing


def test_nearest_equals_brute_force_with_ties():
    g = np.random.default_rng(11)
    target = g.integers(0, 6, (300, 3)).astype(np.float32)      # lattice points, many of them repeated: exact ties
    source = np.concatenate([g.integers(0, 6, (250, 3)).astype(np.float32) + 0.5, g.uniform(-2, 8, (250, 3)).astype(np.float32)])
    j, d2 = E.nearest(source, target)
    jb, d2b = E.nearest_brute(source, target)
    assert np.array_equal(j, jb) and np.array_equal(d2, d2b)
    s64, t64 = source.astype(np.float64), target.astype(np.float64)
    ties = sum(np.count_nonzero(((s64[i] - t64) ** 2).sum(1) == d2b[i]) > 1 for i in range(len(source)))
    assert ties > 100
    src, tgt = E.tie_wall()
    jw, d2w = E.nearest(src, tgt)
    jwb, d2wb = E.nearest_brute(src, tgt)
    assert np.array_equal(jw, jwb) and np.array_equal(d2w, d2wb) and np.all(d2w == 2.0 * 2.0 ** -12)


def test_parallel_squares():
    delta = 0.1
    a, b = E.mesh_square(0.0), E.mesh_square(delta)
    m = E.reconstruction_metrics(a, b, 2000, threshold=0.09)
    # the nearest point of the other plane is at least delta away; fp32 z = 0.1 is 0.100000001
    assert m["accuracy"] >= delta and m["completion"] >= delta
    assert m["completion_ratio"] == 0 and m["accuracy_ratio"] == 0
    bound = math.sqrt(delta * delta + 2.0) * (1 + 1e-7)
    assert m["accuracy_max"] <= bound and m["completion_max"] <= bound
    assert np.all(np.sqrt(m["d2_acc"]) <= bound) and np.all(np.sqrt(m["d2_comp"]) <= bound)
    assert abs(m["chamfer"] - 0.5 * (m["accuracy"] + m["completion"])) < 1e-15


def test_box_room_mesh():
    import torch
    bound = synth.config_reference_defaults()["mapping"]["bound"]
    v, f = synth.box_room_mesh(bound)
    assert v.dtype == np.float64 and v.shape == (8, 3) and f.shape == (12, 3)
    b32 = torch.as_tensor(bound, dtype=torch.float32)
    lo, hi = (b32[:, 0] + 0.3).double().numpy(), (b32[:, 1] - 0.3).double().numpy()          # render_box_frame's lo, hi
    assert np.all((v == lo) | (v == hi))
    e = hi - lo
    closed = 2.0 * (e[0] * e[1] + e[1] * e[2] + e[2] * e[0])
    assert abs(E.mesh_area(v, f) - closed) <= 1e-12 * closed
    assert abs(E.sample_surface(v.astype(np.float32), f, 10)[2] - closed) <= 1e-12 * closed
    centre = 0.5 * (lo + hi)
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    assert np.all(((centre - v[f[:, 0]]) * n).sum(1) > 0)                                    # normals point into the room
    v2, _ = synth.box_room_mesh(bound, shrink=0.5)
    assert np.all((v2 == (b32[:, 0] + 0.5).double().numpy()) | (v2 == (b32[:, 1] - 0.5).double().numpy()))


def test_two_rooms_mesh():
    """Convention: the shared wall is there once per room (two coincident copies with opposite normals), each copy without the
    door, so the area is both boxes minus twice the door."""
    v, f = synth.two_rooms_mesh(synth.TWO_ROOMS)
    A, B, door = (np.asarray(synth.TWO_ROOMS[k], np.float32).astype(np.float64) for k in ("room_a", "room_b", "door"))

    def box_area(b):
        e = b[:, 1] - b[:, 0]
        return 2.0 * (e[0] * e[1] + e[1] * e[2] + e[2] * e[0])
    want = box_area(A) + box_area(B) - 2.0 * (door[0, 1] - door[0, 0]) * (door[1, 1] - door[1, 0])
    assert abs(E.mesh_area(v, f) - want) <= 1e-12 * want
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    mid = v[f].mean(1)
    z_wall = A[2, 1]
    in_a = (mid[:, 2] < z_wall) | ((mid[:, 2] == z_wall) & (n[:, 2] < 0))
    centre = np.where(in_a[:, None], A.mean(1), B.mean(1))
    assert np.all(((centre - v[f[:, 0]]) * n).sum(1) > 0)                                    # normals point into their room
    pts, face_of, _ = E.sample_surface(v.astype(np.float32), f, 50000, seed=2)
    p = pts.astype(np.float64)
    on_wall = np.abs(p[:, 2] - z_wall) < 1e-6
    assert on_wall.sum() > 1000
    m = 1e-5                                                                                 # fp32 rounding of a sample
    inside = on_wall & (p[:, 0] > door[0, 0] + m) & (p[:, 0] < door[0, 1] - m) & (p[:, 1] > door[1, 0] - 1.0) & (p[:, 1] < door[1, 1] - m)
    assert not inside.any()
    with pytest.raises(ValueError):
        synth.two_rooms_mesh({"room_a": synth.TWO_ROOMS["room_a"], "room_b": synth.TWO_ROOMS["room_b"], "door": [[0.55, 1.85], [1.0, 5.2]]})


def test_stats_restatement():
    d2 = np.array([0.0, 0.0025, 0.0025000001, 4.0, np.inf, np.nan, 1e-300])
    s = E.stats(d2, 0.05)
    assert s["finite"] == 5 and s["within"] == 3 and s["max_d"] == 2.0
    assert abs(s["sum_d"] - (0.05 + math.sqrt(0.0025000001) + 2.0 + 1e-150)) < 1e-15
    assert E.stats(np.zeros(0), 0.05) == {"sum_d": 0.0, "sum_d2": 0.0, "max_d": 0.0, "within": 0, "finite": 0}


def test_shifted_box_completion_ratio_is_one():
    """The end-to-end GPU case: the box room against itself shifted by 2 cm along x, 4096 samples.  At 5 cm the ratio is NOT 1 at
    this sample count: 4096 samples on 99 m^2 lie about 16 cm apart, cloud-to-cloud distances are of that size (mean 8 cm, largest
    27.2 cm) and the ratio at 5 cm is 0.26.  The smallest round threshold at which it is exactly 1 is 0.3 (E.SHIFT_THRESHOLD), which
    is what the GPU test uses for this pair; at 0.25 it is not."""
    m = E.reconstruction_metrics(*E.shifted_box_pair(), E.E2E_SAMPLES, threshold=E.SHIFT_THRESHOLD)
    print("shifted box: accuracy %.6f completion %.6f ratio %.6f max %.6f" % (m["accuracy"], m["completion"], m["completion_ratio"], m["completion_max"]))
    assert m["accuracy"] >= 0 and m["completion_ratio"] == 1.0 and m["accuracy_ratio"] == 1.0
    assert E.reconstruction_metrics(*E.shifted_box_pair(), E.E2E_SAMPLES, threshold=0.25)["completion_ratio"] < 1.0
    assert E.reconstruction_metrics(*E.shifted_box_pair(), E.E2E_SAMPLES, threshold=0.05)["completion_ratio"] < 0.5


# Largest number of cells one source point's walk visits over the cases of tests/test_gpu_eval.py, and the largest number over a
# whole case (measured here: see WALK_* below); a cell visit is two 4-byte loads plus 16 bytes and one float64 distance per point.
# Measured: 225 828 cells for one point (the fine grid, a source 1 m from the target: 40 rings of 4 cm), 14 788 384 cells over a
# case (1000 sources 10 m below the room: every one scans the whole grid of 15 808 cells and its 30 000 points, 3e7 distances).
WALK_MAX_CELLS_PER_POINT = 1 << 18
WALK_MAX_CELLS_PER_CASE = 2.0e7


def test_ring_walk_is_bounded_on_the_gpu_cases():
    worst = (0, 0, "")
    for name, (s, t, kw, _, d2) in E.nearest_cases().items():
        if len(t) == 0 or len(s) == 0:
            continue
        cells, rings = E.walk_cells(s, t, d2, kw.get("min_edge", 0.0), kw.get("max_cells", 1 << 21))
        print(f"{name:32s} sources {len(s):6d} cells/point max {cells.max():8d} total {cells.sum():10d} rings max {rings.max():4d}")
        assert cells.max() <= WALK_MAX_CELLS_PER_POINT and cells.sum() <= WALK_MAX_CELLS_PER_CASE
        worst = max(worst, (int(cells.sum()), int(cells.max()), name))
    print("worst case:", worst)
