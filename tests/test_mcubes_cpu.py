"""CPU: the mesh extractor's tables, its numpy restatement against the results recorded from the upstream extractor, the PLY
writer, the grid counts and the C ABI of the new entry points (no GPU)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from mipsfusion_amd import _lib, mesh

from . import mcubes_cpu as mc
from .conftest import ROOT, load_golden


def test_committed_tables_are_what_the_generator_writes():
    gen = mc.load_generator()
    assert open(gen.HEADER).read() == gen.render()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_mcubes_tables.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_every_case_has_the_recorded_crossings_and_vector_area():
    """(a) the same crossed edges, i.e. the same vertex set within 2e-5 (the upstream's weld reach), (b) the same vector area
    within 2e-4 (perimeter < 7, each vertex within 2e-5: < 1.4e-4).  The vector area depends on the boundary loops and their
    winding only, so it pins the cut of alternating faces and the orientation and leaves the fan free."""
    from scipy.spatial import cKDTree
    g = load_golden("mcubes_cases.npz")
    _, ntri, _ = mc.tables()
    for case in range(256):
        tris, _ = mc.soup(g["vol"][case], 0.0, 3.0)
        ref = g["tri"][g["tri_case"] == case].astype(np.float64)
        assert len(tris) == ntri[case]
        assert (len(tris) == 0) == (len(ref) == 0), case
        if len(ref) == 0:
            continue
        own_v, ref_v = np.unique(tris.reshape(-1, 3).astype(np.float64), axis=0), np.unique(ref.reshape(-1, 3), axis=0)
        assert len(own_v) == len(ref_v), case
        assert cKDTree(ref_v).query(own_v)[0].max() <= mc.MATCH_TOL and cKDTree(own_v).query(ref_v)[0].max() <= mc.MATCH_TOL, case
        assert np.abs(mc.vector_area(tris) - mc.vector_area(ref)).max() <= mc.AREA_TOL, case
    # no triangle of the tables lies inside a face of the cube
    gen = mc.load_generator()
    assert not [c for c in range(256) for t in gen.case_triangles(c) if gen._in_one_face(t)]


@pytest.mark.parametrize("name", ["sphere", "wavy", "noise", "plane_snap", "plane_snap2", "iso025", "trunc8"])
def test_restatement_against_the_recorded_meshes(name):
    g = load_golden("mcubes.npz")
    assert name in list(g["cases"])
    vol = g[name + "_vol"]
    iso, trunc = g[name + "_par"]
    v, f, cells = mc.marching_cubes(vol, iso, trunc, return_cells=True)
    mc.compare_with_reference(name, v, f, g)
    if name not in mc.SNAP_CASES:           # snapped faces lie IN cell faces, where the centroid does not tell the cell
        assert np.array_equal(mc.face_cells(v, f, vol.shape), cells)
    mc.check_manifold(v, f, vol, iso, trunc)
    mc.check_manifold(g[name + "_v"].astype(np.float64), g[name + "_f"].astype(np.int64), vol, iso, trunc)
    if name == "trunc8":        # the thresh = 10 rejections are live here
        code, cv = mc.classify(vol, iso, trunc)
        below = cv[1:-1, 1:-1, 1:-1].reshape(-1, 8) < np.float32(iso)       # every voxel is valid here, so these cells are too
        silenced = below.any(1) & ~below.all(1) & (code[1:-1, 1:-1, 1:-1].reshape(-1) == 0)
        assert np.abs(vol).max() < trunc and mc.thresh_rejects(cv[1:-1, 1:-1, 1:-1].reshape(-1, 8)[silenced]).sum() >= 3


def test_parallel_weld_equals_the_sequential_one_on_the_fixtures():
    g = load_golden("mcubes.npz")
    for name in ("sphere", "plane_snap2", "iso025"):
        tris, _ = mc.soup(g[name + "_vol"], *g[name + "_par"])
        gv, gf = mc.weld_greedy(tris)
        wv, wf = mc.weld(tris)
        assert np.array_equal(gv, wv) and np.array_equal(gf, wf)
    # a chain a - b - c (a and c not adjacent): connected components make one vertex of it, whatever the order
    chain = np.zeros((1, 3, 3), np.float32)
    chain[0, :, 0] = [1.00000, 1.000021, 1.000011]
    v, f = mc.weld(chain)
    assert len(v) == 1 and f.tolist() == [[0, 0, 0]]


def test_ply_round_trip(tmp_path):
    rng = np.random.default_rng(0)
    v = rng.standard_normal((50, 3))
    f = rng.integers(0, 50, (80, 3))
    col = rng.random((50, 3)).astype(np.float32)
    mesh.save_ply(str(tmp_path / "a" / "plain.ply"), v, f)
    v2, f2, c2 = mesh.load_ply(str(tmp_path / "a" / "plain.ply"))
    assert np.array_equal(v, v2) and np.array_equal(f, f2) and c2 is None and f2.dtype == np.int64
    mesh.save_ply(str(tmp_path / "col.ply"), v, f, col)
    v2, f2, c2 = mesh.load_ply(str(tmp_path / "col.ply"))
    assert np.array_equal(v, v2) and np.array_equal(f, f2) and np.array_equal(c2, mesh.colors_to_uint8(col))
    mesh.save_ply(str(tmp_path / "empty.ply"), np.zeros((0, 3)), np.zeros((0, 3), np.int64))
    assert [len(t) for t in mesh.load_ply(str(tmp_path / "empty.ply"))[:2]] == [0, 0]


def test_grid_counts_are_the_recorded_ones():
    for row in load_golden("mcubes.npz")["getvoxels"]:
        box, vs, res, counts, second = row[:6], row[6], int(row[7]), row[8:11], row[11:14]
        t = mesh.getVoxels(*box, voxel_size=vs if vs > 0 else None, resolution=res if res > 0 else None)
        assert [len(a) for a in t] == [int(c) for c in counts]
        assert [float(a[1]) for a in t] == list(second)
        assert all(a.dtype.is_floating_point and a.dim() == 1 for a in t)


def test_header_declares_and_library_exports_the_mesh_entry_points():
    header = open(os.path.join(ROOT, "include", "mipsf_mesh.h")).read()
    declared = set(re.findall(r"\b(mipsf_mcubes_[a-z0-9_]+)\s*\(", header))
    assert declared == {"mipsf_mcubes_count", "mipsf_mcubes_emit", "mipsf_mcubes_weld"} == set(_lib.MESH_SIGNATURES)
    handle = C.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(handle, name), name
    for macro, value in (("MIPSF_SIZE_MCUBES_OFFSET_WORDS", _lib.SIZE_MCUBES_OFFSET_WORDS), ("MIPSF_SIZE_MCUBES_WELD_SLOTS", _lib.SIZE_MCUBES_WELD_SLOTS),
                         ("MIPSF_SIZE_MCUBES_WELD_WORDS", _lib.SIZE_MCUBES_WELD_WORDS), ("MIPSF_MCUBES_BLOCK_CELLS", _lib.MCUBES_BLOCK_CELLS)):
        assert int(re.search(rf"#define {macro} (\d+)", header).group(1)) == value
    lib = _lib.lib()
    assert _lib.buffer_size(_lib.SIZE_MCUBES_OFFSET_WORDS, 32, 32, 32) == 32 ** 3 // 4096 + 1
    assert _lib.buffer_size(_lib.SIZE_MCUBES_OFFSET_WORDS, 3, 5, 7) == 2
    slots = _lib.buffer_size(_lib.SIZE_MCUBES_WELD_SLOTS, 1000)
    assert slots >= 6000 and slots & (slots - 1) == 0
    assert _lib.buffer_size(_lib.SIZE_MCUBES_WELD_WORDS, 1000) == 4 * slots + 9000 + 2
    with pytest.raises(RuntimeError, match="too large"):
        _lib.buffer_size(_lib.SIZE_MCUBES_OFFSET_WORDS, 2048, 2048, 2048)
    for cls, fn in ((_lib.McubesArgs, lib.mipsf_mcubes_count), (_lib.McubesArgs, lib.mipsf_mcubes_emit),
                    (_lib.McubesWeldArgs, lib.mipsf_mcubes_weld)):
        blk = cls.new()
        blk.struct_size -= 4
        assert fn(C.byref(blk), None) != 0 and b"struct_size" in lib.mipsf_last_error()
    blk = _lib.McubesArgs.new(X=4, Y=4, Z=4)
    assert lib.mipsf_mcubes_count(C.byref(blk), None) != 0 and b"null pointer" in lib.mipsf_last_error()


def test_the_package_exports_the_mesh_interface_and_refuses_cpu_tensors():
    import torch
    import mipsfusion_amd
    for name in ("marching_cubes", "extract_mesh", "extract_mesh2", "Mesh", "save_ply", "load_ply"):
        assert getattr(mipsfusion_amd, name) is getattr(mesh, name)
    with pytest.raises(RuntimeError, match="GPU only"):
        mesh.marching_cubes(torch.zeros(4, 4, 4), 0.0, 3.0)
