"""The map as a mesh: marching cubes on the device volume and the reference's ``extract_mesh`` / ``extract_mesh2``.

``marching_cubes`` has the signature and return types of the reference's ``marching_cubes.marching_cubes``
(external/NumpyMarchingCubes) and its semantics (dual grid, truncation, snapping, weld on the 1e-5 grid, face clean-up:
DESIGN.md 4.12), computed by the kernels of ``csrc/mcubes.hip`` on a volume that never leaves the GPU.
``extract_mesh`` / ``extract_mesh2`` are ``utils/utils.py:47,124`` of the reference: dense grid -> SDF through
``inference.query_in_batches`` -> marching cubes -> rescale in float64 -> per-vertex colour -> PLY.  The reference returns a
``trimesh.Trimesh``; here a small ``Mesh`` named tuple is returned and the file is written by ``save_ply``.
"""
import ctypes as C
import os
from typing import Callable, NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from .inference import query_in_batches


class Mesh(NamedTuple):
    vertices: np.ndarray                     # float64 [V,3]
    faces: np.ndarray                        # int64 [F,3]
    vertex_colors: Optional[np.ndarray]      # float32 [V,3] in 0..1, or None

    def to_trimesh(self):
        import trimesh
        return trimesh.Trimesh(self.vertices, self.faces, process=False, vertex_colors=self.vertex_colors)


# ------------------------------------------------------------------------------------------------------ marching cubes
def _count(vol: torch.Tensor, isovalue: float, truncation: float):
    X, Y, Z = vol.shape
    n = X * Y * Z
    dev = vol.device
    cases = torch.empty(n, dtype=torch.uint8, device=dev)
    offsets = torch.empty(_lib.buffer_size(_lib.SIZE_MCUBES_OFFSET_WORDS, X, Y, Z), dtype=torch.int32, device=dev)
    a = _lib.McubesArgs.new(X=X, Y=Y, Z=Z, isovalue=isovalue, truncation=truncation, volume=_lib.dptr(vol),
                            cases=_lib.dptr(cases, torch.uint8), block_offsets=_lib.dptr(offsets, torch.int32))
    _lib.check(_lib.lib().mipsf_mcubes_count(C.byref(a), _lib.stream_ptr()), "mcubes_count")
    return a, cases, offsets


def triangle_soup(volume: torch.Tensor, isovalue: float, truncation: float):
    """-> soup fp32 [T,3,3] in cell order (i, j, k), k fastest, table order within a cell, and the cell id int32 [T]
    ((i*Y + j)*Z + k) of every triangle; both on the volume's device."""
    vol = _device_volume(volume)
    with torch.cuda.device(vol.device):
        a, cases, offsets = _count(vol, isovalue, truncation)
        T = int(offsets[-1])                        # the one read-back the soup's size needs
        soup = torch.empty((T, 3, 3), dtype=torch.float32, device=vol.device)
        cells = torch.empty((T,), dtype=torch.int32, device=vol.device)
        if T:
            a.soup, a.cell_ids, a.capacity_tris = _lib.dptr(soup), _lib.dptr(cells, torch.int32), T
            _lib.check(_lib.lib().mipsf_mcubes_emit(C.byref(a), _lib.stream_ptr()), "mcubes_emit")
    return soup, cells


def weld(soup: torch.Tensor, max_rounds: int = 2):
    """soup fp32 [T,3,3] -> vertices fp32 [V,3] (welded on the 1e-5 grid, numbered by first appearance), faces int32 [T,3]"""
    T = soup.shape[0]
    dev = soup.device
    if T == 0:
        return torch.zeros((0, 3), dtype=torch.float32, device=dev), torch.zeros((0, 3), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        scratch = torch.empty(_lib.buffer_size(_lib.SIZE_MCUBES_WELD_WORDS, T), dtype=torch.int32, device=dev)
        vertices = torch.empty((3 * T, 3), dtype=torch.float32, device=dev)
        faces = torch.empty((T, 3), dtype=torch.int32, device=dev)
        counts = torch.empty(4, dtype=torch.int32, device=dev)
        while True:
            a = _lib.McubesWeldArgs.new(T=T, soup=_lib.dptr(soup), scratch=_lib.dptr(scratch, torch.int32),
                                        vertices=_lib.dptr(vertices), faces=_lib.dptr(faces, torch.int32),
                                        counts=_lib.dptr(counts, torch.int32), max_rounds=max_rounds)
            _lib.check(_lib.lib().mipsf_mcubes_weld(C.byref(a), _lib.stream_ptr()), "mcubes_weld")
            V, moved, unplaced, _ = counts.tolist()
            if unplaced:
                raise RuntimeError(f"mcubes_weld: {unplaced} soup vertices with a negative or non-finite coordinate")
            if moved < max_rounds:
                break
            if max_rounds >= 64:
                raise RuntimeError("mcubes_weld: labels still moving after 64 rounds (a chain of more than 64 weld cells)")
            max_rounds = min(64, 4 * max_rounds)                # a chain of clusters longer than the rounds: go on
    return vertices[:V], faces


def filter_faces(faces: torch.Tensor, *per_face: torch.Tensor):
    """drop faces with a repeated index, then repeated faces (same three indices in any order; the first stays)"""
    ok = (faces[:, 0] != faces[:, 1]) & (faces[:, 1] != faces[:, 2]) & (faces[:, 0] != faces[:, 2])
    idx = torch.nonzero(ok)[:, 0]
    if idx.numel():
        key = torch.sort(faces[idx].to(torch.int64), 1)[0]
        _, inv = torch.unique(key, dim=0, return_inverse=True)
        first = torch.full((int(inv.max()) + 1,), idx.numel(), dtype=torch.int64, device=faces.device)
        first.scatter_reduce_(0, inv, torch.arange(idx.numel(), device=faces.device), "amin")
        idx = idx[torch.sort(first)[0]]
    return (faces[idx],) + tuple(p[idx] for p in per_face)


def _device_volume(volume) -> torch.Tensor:
    if isinstance(volume, np.ndarray):
        volume = torch.from_numpy(np.ascontiguousarray(volume, np.float32)).cuda()
    if volume.dim() != 3:
        raise RuntimeError("Only three-dimensional arrays are supported.")
    if not volume.is_cuda:
        raise RuntimeError("marching_cubes runs on the GPU only (no CPU fallback); pass a numpy volume to have it uploaded")
    return volume.to(torch.float32).contiguous()


def marching_cubes(volume, isovalue: float, truncation: float, return_device: bool = False, return_cells: bool = False):
    """-> (vertices float64 [V,3], faces int64 [F,3]) as numpy arrays; tensors on the GPU with ``return_device``;
    ``return_cells`` adds the cell id ((i*Y + j)*Z + k, int32 [F]) each face came from."""
    soup, cells = triangle_soup(volume, isovalue, truncation)
    vertices, faces = weld(soup)
    faces, cells = filter_faces(faces, cells)
    out = (vertices.to(torch.float64), faces.to(torch.int64)) + ((cells,) if return_cells else ())
    return out if return_device else tuple(t.cpu().numpy() for t in out)


# ------------------------------------------------------------------------------------------------------------ PLY
def save_ply(path: str, vertices, faces, vertex_colors=None) -> None:
    """binary little-endian PLY: float64 x y z (, uchar red green blue), faces as uchar count + int32 indices"""
    v = np.ascontiguousarray(vertices, "<f8")
    f = np.ascontiguousarray(faces).astype("<i4")
    head = ["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}", "property double x", "property double y",
            "property double z"]
    vt = [("xyz", "<f8", (3,))]
    if vertex_colors is not None:
        head += ["property uchar red", "property uchar green", "property uchar blue"]
        vt.append(("rgb", "u1", (3,)))
    head += [f"element face {len(f)}", "property list uchar int vertex_indices", "end_header"]
    rec = np.zeros(len(v), np.dtype(vt))
    rec["xyz"] = v
    if vertex_colors is not None:
        rec["rgb"] = colors_to_uint8(vertex_colors)
    frec = np.zeros(len(f), np.dtype([("n", "u1"), ("idx", "<i4", (3,))]))
    frec["n"], frec["idx"] = 3, f
    if os.path.dirname(path):
        os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "wb") as fh:
        fh.write(("\n".join(head) + "\n").encode("ascii"))
        fh.write(rec.tobytes())
        fh.write(frec.tobytes())


def colors_to_uint8(c) -> np.ndarray:
    c = np.asarray(c)
    if c.dtype == np.uint8:
        return c[:, :3]
    return np.clip(np.rint(c[:, :3].astype(np.float64) * 255.0), 0, 255).astype(np.uint8)


def load_ply(path: str):
    """reads what save_ply writes -> (vertices float64 [V,3], faces int64 [F,3], colours uint8 [V,3] or None)"""
    with open(path, "rb") as fh:
        lines = []
        while not lines or lines[-1] != "end_header":
            lines.append(fh.readline().decode("ascii").strip())
        if lines[:2] != ["ply", "format binary_little_endian 1.0"]:
            raise ValueError("not a binary little-endian PLY")
        nv = int([l for l in lines if l.startswith("element vertex")][0].split()[-1])
        nf = int([l for l in lines if l.startswith("element face")][0].split()[-1])
        colours = "property uchar red" in lines
        vt = [("xyz", "<f8", (3,))] + ([("rgb", "u1", (3,))] if colours else [])
        rec = np.frombuffer(fh.read(nv * np.dtype(vt).itemsize), np.dtype(vt))
        ft = np.dtype([("n", "u1"), ("idx", "<i4", (3,))])
        frec = np.frombuffer(fh.read(nf * ft.itemsize), ft)
        if len(rec) != nv or len(frec) != nf or (nf and (frec["n"] != 3).any()):
            raise ValueError("truncated PLY or a face that is not a triangle")
    return rec["xyz"].astype(np.float64), frec["idx"].astype(np.int64), (rec["rgb"].copy() if colours else None)


# ------------------------------------------------------------------------------------------------- the reference's API
def getVoxels(x_max, x_min, y_max, y_min, z_max, z_min, voxel_size=None, resolution=None):
    """utils/utils.py:12-34: the ticks of the dense grid (``round(extent / voxel_size + 0.0005)`` cells, or ``resolution`` ticks)"""
    x_max, x_min, y_max, y_min, z_max, z_min = (float(t) for t in (x_max, x_min, y_max, y_min, z_max, z_min))
    if voxel_size is not None:
        counts = [round((hi - lo) / voxel_size + 0.0005) + 1 for hi, lo in ((x_max, x_min), (y_max, y_min), (z_max, z_min))]
    else:
        counts = [resolution] * 3
    return tuple(torch.linspace(lo, hi, n) for (lo, hi), n in zip(((x_min, x_max), (y_min, y_max), (z_min, z_max)), counts))


def transform_points(pts: torch.Tensor, mat: torch.Tensor) -> torch.Tensor:
    """helper_functions/geometry_helper.py:76-82: R @ pts^T + t, transposed back"""
    return torch.transpose(mat[:3, :3] @ torch.transpose(pts, 0, 1) + mat[:3, 3:], 0, 1)


def _extract(query_fn: Callable, first_kf_c2w, config, bounding_box, marching_cube_bound, color_func, voxel_size, resolution,
             isolevel, mesh_savepath, rank, world, color_normalised, on_volume):
    if marching_cube_bound is None:
        marching_cube_bound = bounding_box
    x_min, y_min, z_min = marching_cube_bound[:, 0]
    x_max, y_max, z_max = marching_cube_bound[:, 1]
    tx, ty, tz = getVoxels(x_max, x_min, y_max, y_min, z_max, z_min, voxel_size, resolution)
    query_pts = torch.stack(torch.meshgrid(tx, ty, tz, indexing="ij"), -1).to(torch.float32)
    sh = query_pts.shape
    flat = query_pts.reshape([-1, 3]).to(bounding_box[:, 0])
    w2l = None
    if first_kf_c2w is not None:
        w2l = first_kf_c2w.inverse()
        flat = transform_points(flat.to(w2l), w2l)
    if config["grid"]["tcnn_encoding"]:
        flat = (flat - bounding_box[:, 0]) / (bounding_box[:, 1] - bounding_box[:, 0])
    raw = query_in_batches(lambda p: query_fn(p[:, None, :]), flat, 1024 * 64, rank, world)
    volume = raw.to(torch.float32).reshape(sh[0], sh[1], sh[2])
    if on_volume is not None:
        on_volume(volume)
    vertices, triangles = marching_cubes(volume, isolevel, truncation=3.0)

    # normalise, rescale and translate as the reference's numpy does (float64)
    vertices[:, :3] /= np.array([[tx.shape[0] - 1, ty.shape[0] - 1, tz.shape[0] - 1]])
    tx, ty, tz = (t.cpu().data.numpy() for t in (tx, ty, tz))
    scale = np.array([tx[-1] - tx[0], ty[-1] - ty[0], tz[-1] - tz[0]])
    offset = np.array([tx[0], ty[0], tz[0]])
    vertices[:, :3] = scale[np.newaxis, :] * vertices[:, :3] + offset
    vertices[:, :3] = vertices[:, :3] / config["data"]["sc_factor"] - config["data"]["translation"]

    color = None
    if color_func is not None:
        vert_flat = torch.from_numpy(vertices).to(bounding_box)
        if w2l is not None:
            # extract_mesh2 of the reference queries colour at UN-normalised local coordinates (utils.py:178-180: the
            # normalising line is commented out there); color_normalised does what was evidently meant
            vert_flat = transform_points(vert_flat.to(w2l), w2l)
            if color_normalised and config["grid"]["tcnn_encoding"]:
                vert_flat = (vert_flat - bounding_box[:, 0].to(vert_flat)) / (bounding_box[:, 1] - bounding_box[:, 0]).to(vert_flat)
        elif config["grid"]["tcnn_encoding"]:
            vert_flat = (vert_flat - bounding_box[:, 0]) / (bounding_box[:, 1] - bounding_box[:, 0])
        if vert_flat.shape[0]:
            raw = query_in_batches(lambda p: color_func(p[:, None, :]), vert_flat, 1024 * 64, rank, world)
            color = raw.cpu().data.numpy().astype(np.float32).reshape(vert_flat.shape[0], -1)
        else:
            color = np.zeros((0, 3), np.float32)
    mesh = Mesh(vertices, triangles, color)
    if mesh_savepath and rank == 0:
        save_ply(mesh_savepath, mesh.vertices, mesh.faces, mesh.vertex_colors)
    return mesh


@torch.no_grad()
def extract_mesh(query_fn, config, bounding_box, marching_cube_bound=None, color_func=None, voxel_size=None, resolution=None,
                 isolevel=0.0, scene_name="", mesh_savepath="", rank=0, world=1, on_volume=None):
    """utils/utils.py:47 of the reference.  ``rank, world`` shard the two grid queries (every rank gets the whole volume back and
    extracts the same mesh; rank 0 writes the file); ``on_volume(volume)`` sees the device volume before it is marched."""
    return _extract(query_fn, None, config, bounding_box, marching_cube_bound, color_func, voxel_size, resolution, isolevel,
                    mesh_savepath, rank, world, False, on_volume)


@torch.no_grad()
def extract_mesh2(query_fn, first_kf_c2w, config, bounding_box, marching_cube_bound=None, color_func=None, voxel_size=None,
                  resolution=None, isolevel=0.0, scene_name="", mesh_savepath="", rank=0, world=1, color_normalised=False,
                  on_volume=None):
    """utils/utils.py:124 of the reference: the grid is laid out in world coordinates and queried in the sub-map's local frame
    (``first_kf_c2w`` inverted).  Colour is queried at un-normalised local coordinates as the reference does, unless
    ``color_normalised``."""
    return _extract(query_fn, first_kf_c2w, config, bounding_box, marching_cube_bound, color_func, voxel_size, resolution,
                    isolevel, mesh_savepath, rank, world, color_normalised, on_volume)
