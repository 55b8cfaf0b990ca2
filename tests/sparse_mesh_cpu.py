"""numpy restatement of the sparse volume's mesh marched brick by brick (mipsfusion_amd/sparse_tsdf.py: extract_mesh_bricks,
csrc/sparse_mesh.hip, include/mipsf_sparse_mesh.h), following the header literally: per slot in use the padded block
of the marching volume (the brick plus one voxel on every side, -inf where there is no slot, the weight is low or the grid ends) goes
through tests/mcubes_cpu.py's `soup`; the soups are concatenated in slot order with BLOCK-LOCAL fp32 vertices; the weld is
mcubes_cpu's relation over the integer cells q = base * 100000 + weld_cells(local); a surviving vertex is base + local in float64;
the face filters are mcubes_cpu's and the colour is tsdf_cpu.sample_color over sparse_cpu.virtual_state.  The device's soup words,
tri_slot, offsets, vertex words, faces and colour words must EQUAL what this file gives when it is fed the device's slot order.  It
also holds the loader of hand-made states, for the restatement and for a SparseTSDFVolume.  It is a checker, not the product.
"""
import numpy as np

from . import mcubes_cpu as M
from . import sparse_cpu as S
from . import tsdf_cpu as T

BRICK = S.BRICK
BLOCK = tuple(int(b) + 2 for b in BRICK)
GRID = 100000                         # cells of the 1e-5 weld grid per voxel
MAX_SIDE = 21474                      # MIPSF_SPARSE_MESH_MAX_SIDE


def brick_coords(sp, bricks=None):
    """brick ids (the slots in use by default, in slot order) -> int64 [m,3]"""
    nb = sp["bricks"]
    b = np.asarray(sp["slot_brick"] if bricks is None else bricks, np.int64).reshape(-1)
    return np.stack([b // (nb[1] * nb[2]), (b // nb[2]) % nb[1], b % nb[2]], 1)


def bases(sp, bricks=None):
    return brick_coords(sp, bricks) * BRICK - 1


def marching_volume(sp, min_weight=1.0):
    """M over the state's window: tsdf where the brick has a slot and weight >= min_weight, -inf elsewhere"""
    st = sp["state"]
    on = S._voxel_mask(sp, sp["table"] >= 0) & (st["weight"] >= np.float32(min_weight))
    return np.where(on, st["tsdf"], np.float32(-np.inf)).astype(np.float32)


def block(sp, vol, base):
    """B = M[base .. base + (10,10,18)), -inf outside the state's window (outside the grid, or bricks the window does not hold: they
    have no slot, sparse_cpu.inside_window)"""
    out = np.full(BLOCK, -np.inf, np.float32)
    lo, hi = np.asarray(sp["lo"], np.int64), np.asarray(sp["hi"], np.int64)
    g0, g1 = np.maximum(base, lo), np.minimum(base + np.asarray(BLOCK), hi)
    if (g1 > g0).all():
        out[tuple(slice(a - b, c - b) for a, b, c in zip(g0, base, g1))] = vol[tuple(slice(a - l, c - l) for a, l, c in zip(g0, lo, g1))]
    return out


def brick_soup(sp, min_weight=1.0, bricks=None):
    """-> soup fp32 [T,3,3] block-local, tri_slot int32 [T], offsets int64 [m + 1], cell within the brick int32 [T], for the slots
    `bricks` (ids in slot order; the restatement's own by default)"""
    vol = marching_volume(sp, min_weight)
    tris, slots, cells, offsets = [np.zeros((0, 3, 3), np.float32)], [np.zeros(0, np.int32)], [np.zeros(0, np.int32)], [0]
    for s, base in enumerate(bases(sp, bricks)):
        t, c = M.soup(block(sp, vol, base), 0.0, 1.0)
        i, j, k = np.unravel_index(c.astype(np.int64), BLOCK)
        assert ((i >= 1) & (i <= BRICK[0]) & (j >= 1) & (j <= BRICK[1]) & (k >= 1) & (k <= BRICK[2])).all(), "a cell outside the brick emitted"
        tris.append(t), slots.append(np.full(len(t), s, np.int32)), cells.append((((i - 1) * BRICK[1] + (j - 1)) * BRICK[2] + (k - 1)).astype(np.int32))
        offsets.append(offsets[-1] + len(t))
    return np.concatenate(tris), np.concatenate(slots), np.asarray(offsets, np.int64), np.concatenate(cells)


def weld_cells(q):
    """integer cells int64 [n,3] -> (survivor bool [n], label of every vertex as a vertex number int64 [n]): mcubes_cpu.weld's
    relation and numbering, on cells that are given"""
    n = len(q)
    r = np.zeros_like(q)
    for ax in range(3):
        u = np.unique(q[:, ax])
        rank = np.concatenate([[0], np.cumsum(np.minimum(np.diff(u), 2))]) + 1
        r[:, ax] = rank[np.searchsorted(u, q[:, ax])]
    m = int(r.max()) + 3

    def key(c):
        return (c[:, 0] * m + c[:, 1]) * m + c[:, 2]

    keys, inv = np.unique(key(r), return_inverse=True)
    inv = inv.reshape(-1)
    label = np.full(len(keys), n, np.int64)
    np.minimum.at(label, inv, np.arange(n))
    rc = r[label]
    nb = []
    for a in (-1, 0, 1):
        for b in (-1, 0, 1):
            for c in (-1, 0, 1):
                k = key(rc + np.array([a, b, c]))
                pos = np.minimum(np.searchsorted(keys, k), len(keys) - 1)
                nb.append(np.where(keys[pos] == k, pos, -1))
    nb = np.stack(nb, 1)
    rounds = 0
    while True:
        new = np.minimum(label, np.where(nb >= 0, label[np.maximum(nb, 0)], n).min(1))
        if np.array_equal(new, label):
            break
        label, rounds = new, rounds + 1
    root = label[inv]
    keep = root == np.arange(n)
    return keep, (np.cumsum(keep) - 1)[root], rounds


def weld(tris, tri_slot, base):
    """soup [T,3,3] block-local, tri_slot [T], base int64 [m,3] of the slots -> vertices float64 [V,3] in index units, faces int32
    [T,3], rounds in which a label moved"""
    if len(tris) == 0:
        return np.zeros((0, 3), np.float64), np.zeros((0, 3), np.int32), 0
    flat = tris.reshape(-1, 3)
    b = np.repeat(base[tri_slot], 3, 0)
    keep, ids, rounds = weld_cells(b * GRID + M.weld_cells(flat))
    return b[keep].astype(np.float64) + flat[keep].astype(np.float64), ids.reshape(-1, 3).astype(np.int32), rounds


def mesh(sp, min_weight=1.0, bricks=None):
    """extract_mesh_bricks -> dict(soup, tri_slot, offsets, cells, index: vertices in index units, all_faces int32 [T,3], faces int64
    [F,3], face_tri: the triangle of a kept face, vertices: world, colors fp32 [V,3] or None, rounds)"""
    assert max(sp["dims"]) <= MAX_SIDE
    tris, tri_slot, offsets, cells = brick_soup(sp, min_weight, bricks)
    index, all_faces, rounds = weld(tris, tri_slot, bases(sp, bricks))
    faces, face_tri = M.filter_faces(all_faces, np.arange(len(all_faces)))
    vs = S.virtual_state(sp)
    colors = None if vs["color"] is None else T.sample_color(index, vs["weight"], vs["color"])
    return {"soup": tris, "tri_slot": tri_slot, "offsets": offsets, "cells": cells, "index": index, "all_faces": all_faces,
            "faces": faces.astype(np.int64), "face_tri": face_tri, "vertices": sp["origin"] + index * sp["voxel"], "colors": colors, "rounds": rounds}


# ------------------------------------------------------------------------------------------------------------ hand-made states
def hand_made(dims, tsdf, weight, bricks, color=None, origin=(0.0, 0.0, 0.0), voxel=0.05, capacity=None):
    """a restatement's volume whose state is the dense arrays given, under the mask of `bricks`: brick coordinates [m,3], which get the
    slots 0 .. m-1 in the order given"""
    sp = S.new_volume(origin, voxel, dims, 4 * voxel, len(bricks) if capacity is None else capacity, color is not None)
    nb = sp["bricks"]
    for b in bricks:
        b = (int(b[0]) * nb[1] + int(b[1])) * nb[2] + int(b[2])
        assert sp["table"][b] < 0 and len(sp["slot_brick"]) < sp["capacity"]
        sp["table"][b] = len(sp["slot_brick"])
        sp["slot_brick"].append(b)
    on = S._voxel_mask(sp, sp["table"] >= 0)
    st = sp["state"]
    st["tsdf"] = np.where(on, np.asarray(tsdf, np.float32), np.float32(0))
    st["weight"] = np.where(on, np.asarray(weight, np.float32), np.float32(0))
    if color is not None:
        st["color"] = np.where(on[..., None], np.asarray(color, np.float32), np.float32(0))
    return sp


def pool_of(sp, a, beyond=0.0):
    """a dense array over the whole grid -> the words of the slots in use [m,8,8,16(,3)]; `beyond`: the words past the grid's edge"""
    assert sp["lo"] == (0, 0, 0) and sp["hi"] == sp["dims"]
    nb, tail = sp["bricks"], a.shape[3:]
    full = np.full(tuple(int(n * b) for n, b in zip(nb, BRICK)) + tail, beyond, np.float32)
    full[:a.shape[0], :a.shape[1], :a.shape[2]] = a
    full = full.reshape((nb[0], int(BRICK[0]), nb[1], int(BRICK[1]), nb[2], int(BRICK[2])) + tail)
    full = np.moveaxis(full, (0, 2, 4), (0, 1, 2)).reshape((-1,) + tuple(int(b) for b in BRICK) + tail)
    return np.ascontiguousarray(full[np.asarray(sp["slot_brick"], np.int64)])


def to_device(sp, dev, beyond=(0.0, 0.0), guard_slots=0):
    """the restatement's volume written into a SparseTSDFVolume's table, slot_brick, count and pool tensors; `beyond`: the tsdf and
    weight written to the words of a slot past the grid's edge (the fusion leaves zeros there); `guard_slots`: capacity beyond
    sp's, left as the constructor made it"""
    import torch

    from mipsfusion_amd import sparse_tsdf
    st, n = sp["state"], len(sp["slot_brick"])
    vol = sparse_tsdf.SparseTSDFVolume(sp["origin"], sp["voxel"], sp["dims"], sp["trunc"], sp["capacity"] + guard_slots, color=st["color"] is not None,
                                       max_weight=sp["max_weight"], device=dev)
    vol.table.copy_(torch.from_numpy(S.table_of(sp)))
    vol.slot_brick[:n] = torch.tensor(sp["slot_brick"], dtype=torch.int32)
    vol.count.fill_(n)
    if n:
        vol.tsdf[:n] = torch.from_numpy(pool_of(sp, st["tsdf"], beyond[0]))
        vol.weight[:n] = torch.from_numpy(pool_of(sp, st["weight"], beyond[1]))
        if st["color"] is not None:
            vol.color[:n] = torch.from_numpy(pool_of(sp, st["color"]))
    return vol


# ------------------------------------------------------------------------------------------------------------ cases
CASES = ("box/40x56/v0.15/t4", "box/40x56/v0.10/t4", "two_rooms/v0.20", "colour", "bad_pixels", S.VIRTUAL)
HAND_DIMS, HAND_BRICKS = (24, 24, 32), [(x, y, z) for x in range(3) for y in range(3) for z in range(2)]
HAND_CASES = ("sphere", "sphere_hole", "through_faces", "plane_snap", "ragged")
_meshes, _hand = {}, {}


def case_mesh(name):
    """mesh(sparse_cpu.case(name)["sp"]), computed once"""
    if name not in _meshes:
        _meshes[name] = mesh(S.case(name)["sp"])
    return _meshes[name]


def hand_case(name):
    """name -> (volume, `beyond` for to_device): the hand-made states on 3 x 3 x 2 bricks, the smallest shape with an inner brick face,
    edge and corner on every axis.  Values are kept inside the truncation: |tsdf| < 1 wherever a cell should emit.
      sphere          a sphere of radius 9.3 about (11.6, 12.3, 15.7): it crosses every internal brick face, edge and corner
      sphere_hole     the same with the centre brick (1,1,0), which the sphere crosses, left out, and the slots numbered against the
                      brick order: the mesh has a hole whose rim cells emit nothing
      through_faces   a slanted plane that leaves through the low and high faces of a grid of 23 x 22 x 30 voxels on every axis (base
                      -1, and with `beyond` the words of a slot past the edge hold a surface that must not be read)
      plane_snap      tsdf = 0.125 ((i - 7.5) + (j - 7.5)): the dual values on the plane i + j = 15 are exactly 0, and the plane holds
                      the brick edge (7.5, 7.5, .) and the brick corner (7.5, 7.5, 15.5): vertices snap to dual nodes shared by up to
                      eight cells of several bricks, and collapsed faces are dropped
      ragged          the sphere on a grid of 21 x 19 x 29 voxels: no side a multiple of the brick, colour fused"""
    if name in _hand:
        return _hand[name]
    dims = {"ragged": (21, 19, 29), "through_faces": (23, 22, 30)}.get(name, HAND_DIMS)
    i, j, k = np.meshgrid(*(np.arange(d, dtype=np.float64) for d in dims), indexing="ij")
    bricks, beyond, color = list(HAND_BRICKS), (0.0, 0.0), None
    if name in ("sphere", "sphere_hole", "ragged"):
        r = 7.9 if name == "ragged" else 9.3
        c = (10.1, 9.2, 14.7) if name == "ragged" else (11.6, 12.3, 15.7)
        d = (np.sqrt((i - c[0]) ** 2 + (j - c[1]) ** 2 + (k - c[2]) ** 2) - r) / 4.0
        if name == "sphere_hole":
            bricks = [b for b in bricks if b != (1, 1, 0)][::-1]
        if name == "ragged":
            color = np.stack([i / dims[0], j / dims[1], k / dims[2]], -1)
            beyond = (0.0, 3.0)
    elif name == "through_faces":
        d = (0.61 * (i - 11.3) + 0.47 * (j - 12.1) - 0.38 * (k - 15.2)) / 4.0
        beyond = (0.0, 3.0)
    elif name == "plane_snap":
        d = 0.125 * ((i - 7.5) + (j - 7.5)) + 0.0 * k
    else:
        raise KeyError(name)
    tsdf = np.clip(d, -1.0, 1.0).astype(np.float32)
    weight = np.where(np.abs(d) < 1.0, 2.0, 0.0).astype(np.float32)
    weight[(i + 2 * j + 3 * k) % 97 == 0] = np.float32(1.0)                         # min_weight = 2 switches these off
    _hand[name] = (hand_made(dims, tsdf, weight, bricks, color), beyond)
    return _hand[name]
