"""No GPU: the restatement of the brick-by-brick marcher (tests/sparse_mesh_cpu.py) is held to the dense restatement.
The two paths round a vertex's running coordinate in different frames (block-local against window-relative), so they are not
bit-equal; what must hold is: the same V and F, a one-to-one vertex map within one fp32 rounding per frame, the same faces under the
map, and the same triangles per cell.  The map is only well defined while distinct welded vertices stay far apart, which is checked
and printed per case."""
import numpy as np
import pytest
from scipy.spatial import cKDTree

from . import mcubes_cpu as M
from . import sparse_cpu as S
from . import sparse_mesh_cpu as B
from . import tsdf_cpu as T

CLOSEST_DISTINCT = 1e-4       # voxels: ten weld cells; below it a weld cluster need not be a clique and the two welds may differ

# the issue's table: slots in use, T, V, F
EXPECTED = {"box/40x56/v0.15/t4": (48, 6421, 3407, 6421), "box/40x56/v0.10/t4": (129, 17194, 8963, 17176), S.VIRTUAL: (217, 17194, 8963, 17176),
            "two_rooms/v0.20": (45, 2896, 1775, 2896), "colour": (30, 1914, 1095, 1914), "bad_pixels": (20, 214, 156, 214)}


def ulp32(x):
    return float(np.spacing(np.float32(x)))


def oriented(faces):
    """faces as a sorted list of triples, each rotated to start at its smallest index (orientation kept)"""
    f = np.asarray(faces, np.int64)
    first = f.argmin(1)
    rot = np.stack([f[np.arange(len(f)), (first + s) % 3] for s in range(3)], 1)
    return rot[np.lexsort(rot.T[::-1])]


def against_dense(name, sp, m, lo, hi, min_weight=1.0):
    """conditions 2 to 5 for the mesh m of the volume sp against the dense restatement over the window lo .. hi; prints, then asserts"""
    _, want_f, want_v = S.extract_mesh(sp, lo, hi, min_weight)
    got_v = m["index"] - np.asarray(lo, np.float64)                          # window-relative, exact
    print(f"{name}: bricks {len(sp['slot_brick'])}, T {len(m['soup'])}, V {len(got_v)} (dense {len(want_v)}), F {len(m['faces'])} (dense {len(want_f)}), "
          f"weld rounds {m['rounds']}")
    assert len(got_v) == len(want_v) and len(m["faces"]) == len(want_f), name
    # 5. every cell emits in exactly one brick
    n = tuple(b - a for a, b in zip(lo, hi))
    _, dense_cells = M.soup(T.marching_volume(S.window_state(sp, lo, hi), min_weight), 0.0, 1.0)
    base = B.bases(sp)[m["tri_slot"]]
    c = m["cells"].astype(np.int64)
    ijk = base + 1 + np.stack([c // 128, (c // 16) % 8, c % 16], 1) - np.asarray(lo, np.int64)
    assert ((ijk >= 0) & (ijk < np.asarray(n))).all()
    assert np.array_equal(np.sort((ijk[:, 0] * n[1] + ijk[:, 1]) * n[2] + ijk[:, 2]), np.sort(dense_cells.astype(np.int64))), name
    if len(got_v) == 0:
        return
    # 4. the condition under which 2 and 3 may be asserted
    if len(got_v) > 1:
        closest = float(cKDTree(got_v).query(got_v, k=2)[0][:, 1].min())
        print(f"{name}: closest pair of distinct welded vertices {closest:.3e} voxels")
        assert closest >= CLOSEST_DISTINCT, name
    # 2. one to one, faces equal as oriented triples under the map
    dist, to_dense = cKDTree(want_v).query(got_v)
    assert np.array_equal(np.sort(to_dense), np.arange(len(want_v))), name
    assert np.array_equal(oriented(to_dense[m["faces"]]), oriented(want_f)), name
    # 3. one rounding in each frame
    S_max = float(want_v.max())
    bound = 0.5 * ulp32(S_max) + 0.5 * ulp32(17.5)
    worst = float(np.abs(got_v - want_v[to_dense]).max())
    print(f"{name}: nearest-neighbour distance {dist.max():.2e}, worst coordinate difference {worst:.3e} (bound {bound:.3e}, S {S_max:.1f})")
    assert worst <= bound, name


@pytest.mark.parametrize("name", B.CASES)
def test_the_brick_mesh_is_the_dense_mesh_of_the_tight_window(name):
    sp = S.case(name)["sp"]
    m = B.case_mesh(name)
    assert (len(sp["slot_brick"]), len(m["soup"]), len(m["index"]), len(m["faces"])) == EXPECTED[name], name
    assert m["offsets"][-1] == len(m["soup"]) and np.array_equal(np.diff(m["offsets"]), np.bincount(m["tri_slot"], minlength=len(sp["slot_brick"])))
    assert m["soup"].min() >= 0.5 and m["soup"].max() <= 17.5 and m["rounds"] <= 2
    against_dense(name, sp, m, *S.tight_window(sp))
    if name == "colour":                                         # read through the virtual grid or over the window: the same colour
        st = S.window_state(sp, *S.tight_window(sp))
        lo = np.asarray(S.tight_window(sp)[0], np.float64)
        assert np.abs(m["colors"] - T.sample_color(m["index"] - lo, st["weight"], st["color"])).max() == 0.0


def test_an_empty_volume_and_a_slab_too_thin_to_march_give_the_empty_mesh():
    sp = S.case("1x5x70")["sp"]
    m = B.mesh(sp)
    assert len(sp["slot_brick"]) > 0 and len(m["soup"]) == 0 and len(m["index"]) == 0 and len(m["faces"]) == 0 and m["offsets"][-1] == 0
    empty = B.hand_made((24, 24, 32), np.zeros((24, 24, 32)), np.zeros((24, 24, 32)), [])
    m = B.mesh(empty)
    assert m["soup"].shape == (0, 3, 3) and m["faces"].shape == (0, 3) and m["index"].shape == (0, 3)


@pytest.mark.parametrize("name", B.HAND_CASES)
def test_hand_made_states_on_3x3x2_bricks(name):
    sp, _ = B.hand_case(name)
    for min_weight in (1.0, 2.0):
        m = B.mesh(sp, min_weight)
        assert len(m["soup"]) > 100, name
        against_dense(f"{name}/w{min_weight:g}", sp, m, (0, 0, 0), sp["dims"], min_weight)
    m = B.mesh(sp)
    full, _ = B.hand_case("sphere")
    if name == "sphere":
        per_brick = np.diff(m["offsets"])
        assert (per_brick > 0).sum() >= 16                       # the sphere crosses the inner faces, edges and the corners
        M.check_manifold(m["index"], m["faces"], B.marching_volume(sp), 0.0, 1.0)
    if name == "sphere_hole":
        assert len(m["faces"]) < len(B.mesh(full)["faces"])
        # the rim: cells whose own voxel is allocated but which read the hole emit nothing, so no vertex lies inside the hole's brick
        inside = ((m["index"] > np.array([8.0, 8.0, 0.0])) & (m["index"] < np.array([15.0, 15.0, 15.0]))).all(1)
        assert not inside.any()
    if name == "through_faces":
        v = m["index"]
        assert v.min() == 0.5 and np.allclose(v.max(0), np.asarray(sp["dims"]) - 1.5)      # it leaves through the low and high faces
    if name == "plane_snap":
        assert len(m["faces"]) < len(m["soup"])                  # collapsed faces are dropped
        on_node = np.abs(m["index"] - np.floor(m["index"]) - 0.5).max(1) == 0.0
        assert on_node.sum() > 100                               # vertices snapped to dual nodes
    if name == "ragged":
        assert m["colors"] is not None and m["colors"].min() >= 0.0 and m["colors"].max() > 0.5


def test_the_loader_writes_the_state_it_was_given():
    sp, _ = B.hand_case("ragged")
    n = len(sp["slot_brick"])
    pool = B.pool_of(sp, sp["state"]["tsdf"], beyond=7.0)
    assert pool.shape == (n, 8, 8, 16)
    coords = B.brick_coords(sp)
    for s in (0, n // 2, n - 1):
        lo = coords[s] * B.BRICK
        hi = np.minimum(lo + B.BRICK, sp["dims"])
        ext = hi - lo
        assert np.array_equal(pool[s][:ext[0], :ext[1], :ext[2]], sp["state"]["tsdf"][lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]])
        rest = np.ones((8, 8, 16), bool)
        rest[:ext[0], :ext[1], :ext[2]] = False
        assert (pool[s][rest] == 7.0).all()
