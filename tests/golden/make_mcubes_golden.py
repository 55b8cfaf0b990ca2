#!/usr/bin/env python3
"""Records the mesh-extraction fixtures mcubes.npz (split in parts), mcubes_cases.npz from the upstream extractor.

usage: make_mcubes_golden.py /path/to/upstream/MIPSFusion

The upstream ``external/NumpyMarchingCubes`` is copied to a temporary directory OUTSIDE this repository, built there
(Cython 3 / numpy 2 need ``-include limits`` and the two numpy-1 names below) and called on the volumes made here.  Only
inputs and recorded results are written; nothing built leaves the temporary directory.

mcubes.npz       <case>_vol fp32 [X,Y,Z], <case>_v fp32 [V,3] (the extractor's vertices ARE fp32 values widened: asserted),
                 <case>_f int32 [F,3], <case>_par = (isovalue, truncation); `cases` = the names; getVoxels records;
                 `ref_seconds_96`, `ref_faces_96`, `ref_cpu`, `ref_date`: the upstream extractor timed on a 96^3 volume.
mcubes_cases.npz vol fp32 [256,5,5,5]: one probe volume per sign pattern.  The outer shell is -inf, so the only valid cell is
                 (2,2,2); its eight dual values (means of 2x2x2 voxels) carry the wanted signs with distinct magnitudes
                 (minimum-norm solution of the 8 x 27 system, scaled so that every |voxel| < 3).  `signs` [256,8] bool
                 (True = below the isovalue, corner order 4*dx + 2*dy + dz), tri fp32 [n,3,3] the recorded triangles,
                 tri_case int32 [n] the pattern each belongs to.
"""
import ast
import datetime
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch
from scipy import ndimage
from scipy.spatial import cKDTree

HERE = os.path.dirname(os.path.abspath(__file__))
LIMIT = 1000 * 1000


def build_reference(upstream):
    tmp = tempfile.mkdtemp(prefix="mcubes_ref_")
    assert not os.path.abspath(tmp).startswith(os.path.dirname(os.path.dirname(HERE)))
    dst = os.path.join(tmp, "NumpyMarchingCubes")
    src = os.path.join(upstream, "external", "NumpyMarchingCubes")
    shutil.copytree(src, dst, ignore=shutil.ignore_patterns("build", "dist", "*.egg-info", "_mcubes.cpp", "*.so"))
    env = dict(os.environ, CFLAGS="-include limits -DPyArray_DOUBLE=NPY_DOUBLE -DPyArray_ULONG=NPY_ULONG")
    subprocess.run([sys.executable, "setup.py", "build_ext", "--inplace"], cwd=dst, env=env, check=True,
                   stdout=subprocess.DEVNULL)
    sys.path.insert(0, dst)
    import marching_cubes
    return marching_cubes.marching_cubes, tmp


def upstream_get_voxels(upstream):
    """the upstream getVoxels alone (its module imports libraries that are not installed)"""
    tree = ast.parse(open(os.path.join(upstream, "utils", "utils.py")).read())
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "getVoxels"]
    ns = {"torch": torch}
    exec(compile(ast.Module(body=fn, type_ignores=[]), "getVoxels", "exec"), ns)
    return ns["getVoxels"]


def volumes():
    # the two noise seeds are the first whose recorded mesh passes the closest-pair check of main()
    out = {}

    def grid(shape):
        return np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")

    x, y, z = grid((32, 32, 32))
    out["sphere"] = (np.sqrt((x - 14.3) ** 2 + (y - 16.9) ** 2 + (z - 15.2) ** 2) - 9.7, 0.0, 3.0)
    x, y, z = grid((48, 40, 33))
    out["wavy"] = (np.sqrt((x - 23.1) ** 2 + (y - 19.4) ** 2 + (z - 16.2) ** 2) - 11.3
                   + 1.7 * np.sin(0.45 * x) * np.sin(0.38 * y + 0.5) * np.sin(0.52 * z + 1.0), 0.0, 3.0)
    n = ndimage.gaussian_filter(np.random.default_rng(5).standard_normal((40, 40, 40)), 1.6)
    out["noise"] = (n * (4.0 / np.abs(n).max()), 0.0, 3.0)
    x, y, z = grid((24, 28, 20))
    v = x - 10.5
    v[:, 20:23, :] = -np.inf
    out["plane_snap"] = (v, 0.0, 3.0)
    x, y, z = grid((22, 26, 24))
    v = 0.5 * (x - 9.5) + 0.5 * (y - 11.5)
    v[:, :, 15:17] = -np.inf
    v[3:5, :, :] = 5.0
    out["plane_snap2"] = (v, 0.0, 3.0)
    x, y, z = grid((36, 30, 34))
    out["iso025"] = (0.8 * (np.sqrt((x - 17.2) ** 2 + (y - 14.6) ** 2 + (z - 16.3) ** 2) - 8.4)
                     + 0.6 * np.sin(0.7 * x + 0.3) * np.cos(0.6 * z), 0.25, 3.0)
    # blocks of +-5.5 under smooth noise, values up to 7: corners that share one voxel differ by more than 10, so the per-cell
    # rejections on thresh = 10 are live (smooth fields never reach them: a dual value averages eight voxels)
    rng = np.random.default_rng(6)
    n = ndimage.gaussian_filter(rng.standard_normal((30, 30, 30)), 1.1)
    blocks = np.kron(rng.choice([-5.5, 5.5], size=(11, 11, 11)), np.ones((3, 3, 3)))[:30, :30, :30]
    out["trunc8"] = (n * (1.5 / np.abs(n).max()) + blocks, 0.0, 8.0)
    return {k: (np.ascontiguousarray(v.astype(np.float32)), iso, tr) for k, (v, iso, tr) in out.items()}


def probe_volumes():
    rows = np.zeros((8, 27))
    for c in range(8):
        dx, dy, dz = (c >> 2) & 1, (c >> 1) & 1, c & 1
        for a in range(2):
            for b in range(2):
                for d in range(2):
                    rows[c, ((dx + a) * 3 + dy + b) * 3 + dz + d] = 0.125
    mags = np.array([np.sqrt(2) / 2, np.pi / 5, np.e / 4, np.sqrt(3) / 3, np.sqrt(5) / 4, np.log(2), 0.9 / np.sqrt(2), np.sqrt(7) / 5])
    vols = np.full((256, 5, 5, 5), -np.inf, np.float32)
    signs = np.zeros((256, 8), bool)
    for case in range(256):
        below = np.array([(case >> c) & 1 for c in range(8)], bool)
        want = np.where(below, -mags, mags)
        sol = np.linalg.lstsq(rows, want, rcond=None)[0]
        sol *= min(1.0, 2.5 / np.abs(sol).max())
        vols[case, 1:4, 1:4, 1:4] = sol.reshape(3, 3, 3).astype(np.float32)
        signs[case] = below
    return vols, signs


def save_split(stem, arrays):
    """one .npz when it fits a committed file, else .partN.npz pieces that tests/conftest.load_golden reads as one"""
    for old in [f for f in os.listdir(HERE) if f.startswith(stem + ".") and f.endswith(".npz")]:
        os.unlink(os.path.join(HERE, old))
    path = os.path.join(HERE, stem + ".npz")
    np.savez_compressed(path, **arrays)
    if os.path.getsize(path) < LIMIT:
        return [path]
    os.unlink(path)
    parts, cur = [], {}
    for k in arrays:
        trial = dict(cur, **{k: arrays[k]})
        p = os.path.join(HERE, f"{stem}.part{len(parts) + 1}.npz")
        np.savez_compressed(p, **trial)
        if os.path.getsize(p) >= LIMIT and cur:
            np.savez_compressed(p, **cur)
            parts.append(p)
            cur = {k: arrays[k]}
        else:
            cur = trial
    p = os.path.join(HERE, f"{stem}.part{len(parts) + 1}.npz")
    np.savez_compressed(p, **cur)
    assert os.path.getsize(p) < LIMIT, (p, "one array alone exceeds the limit")
    return parts + [p]


def main():
    upstream = sys.argv[1]
    mc, tmp = build_reference(upstream)
    try:
        out = {}
        names = []
        for name, (vol, iso, trunc) in volumes().items():
            v, f = mc(vol, iso, trunc)
            v32 = v.astype(np.float32)
            assert np.array_equal(v32.astype(np.float64), v), "vertices are not fp32 values"
            dmin = cKDTree(v).query(v, k=2)[0][:, 1].min() if len(v) > 1 else np.inf
            print(f"{name:12s} {vol.shape} iso {iso} trunc {trunc}: V/F = {len(v)}/{len(f)}, closest pair {dmin:.2e}")
            assert dmin >= 1e-4, "the weld would be ambiguous on this input: refusing to write"
            names.append(name)
            out[name + "_vol"], out[name + "_v"], out[name + "_f"] = vol, v32, f.astype(np.int32)
            out[name + "_par"] = np.array([iso, trunc], np.float64)
        out["cases"] = np.array(names)

        gv = upstream_get_voxels(upstream)
        boxes = np.array([[1.5, -1.25, 2.0, -0.5, 3.0, 0.1], [0.7, -0.7, 0.3, -0.3, 1.0, 0.0], [4.0, -3.97, 2.5, -2.5, 1.26, -1.26]])
        rec = []
        for bx in boxes:
            for vs, res in ((0.05, None), (0.031, None), (0.1, None), (None, 17), (None, 64)):
                t = gv(*bx, voxel_size=vs, resolution=res)
                rec.append(list(bx) + [vs or 0.0, res or 0] + [len(a) for a in t] + [float(a[1]) for a in t])
        out["getvoxels"] = np.array(rec, np.float64)   # x_max x_min y_max y_min z_max z_min voxel_size resolution | Nx Ny Nz | 2nd ticks

        x, y, z = np.meshgrid(*[np.arange(96.0)] * 3, indexing="ij")
        vol = (np.sqrt((x - 47.3) ** 2 + (y - 48.1) ** 2 + (z - 46.6) ** 2) - 30.2
               + 2.0 * np.sin(0.3 * x) * np.sin(0.27 * y) * np.sin(0.33 * z)).astype(np.float32)
        best = np.inf
        for _ in range(3):
            t0 = time.perf_counter()
            v, f = mc(vol, 0.0, 3.0)
            best = min(best, time.perf_counter() - t0)
        cpu = [l.split(":", 1)[1].strip() for l in open("/proc/cpuinfo") if l.startswith("model name")][:1]
        out["ref_seconds_96"], out["ref_faces_96"] = np.float64(best), np.int64(len(f))
        out["ref_cpu"], out["ref_date"] = np.array(cpu[0] if cpu else "unknown"), np.array(datetime.date.today().isoformat())
        print(f"upstream extractor, 96^3, one thread: {best:.3f} s, {len(f)} faces ({out['ref_cpu']})")
        print("wrote", save_split("mcubes", out))

        vols, signs = probe_volumes()
        tris, owner = [], []
        for case in range(256):
            v, f = mc(vols[case], 0.0, 3.0)
            t = v[f.astype(np.int64)].astype(np.float32) if len(f) else np.zeros((0, 3, 3), np.float32)
            assert (t >= 1.5).all() and (t <= 2.5).all()
            tris.append(t)
            owner += [case] * len(t)
        print("wrote", save_split("mcubes_cases", {"vol": vols, "signs": signs, "tri": np.concatenate(tris),
                                                   "tri_case": np.array(owner, np.int32)}))
    finally:
        sys.path.pop(0)
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
