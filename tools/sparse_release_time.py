"""Times the release, the archive and the restore of bricks of the brick-sparse volume (mipsfusion_amd/sparse_tsdf.py release_enqueue and
restore_enqueue) on one GPU beside the sparse fusion step of one view, on the scenes of tools/sparse_time.py: the
marched 128^3 box room seen from 256 views of 460 x 620 pixels, in a virtual grid of 256^3 voxels and in one of 1536^3, which no dense
volume holds.

    python tools/sparse_release_time.py [--reps 5] [--res 256] [--big 1536] [--views 256] [--out file.json]

Milliseconds between two events on the stream after one warm-up call, median of --reps; the state every timed call starts from
(table, slots and pool, all 256 views fused) is put back, untimed, before every repeat:
  release_empty          release_enqueue(empty=True): every slot's weights are read; the slots the band allocated and no view observed go
  release_quarter/half   release_enqueue(box): the box begins at a brick boundary along x so that about a quarter / a half of the bricks
                         lie outside, the ones in the FIRST slots, so that as many tail slots move; `released` and `moved` are the
                         record's
  release_half_tail      the half at the other end of x: the last slots, nothing moves
  release_all            release_enqueue of a box that holds no brick: every slot is zeroed, none moves
  .._archive             the same into a BrickArchive with room for every brick
  restore_half           restore_enqueue of the archive release_half_archive wrote, into the volume it left
  integrate_one_view     integrate_enqueue of the last view into the full volume: what a frame of the walk pays anyway
`bytes` is what the rule says a release must touch -- 8 KB read and 8 KB written per moved slot, 8 KB zeroed per released slot, 8 KB
read and written per archived slot, 4 KB of weights read per slot in use with EMPTY -- and `GB_per_s` is that over the time.  The shader
clock and package power sampled across the timed regions are printed beside the times (bench.BoardSampler), the date too."""
import argparse
import datetime
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import BoardSampler                                                # noqa: E402
from mipsfusion_amd import mesh_render as mr, sparse_tsdf, synth              # noqa: E402
from tools.raster_time import marched_room, timed, view_poses                # noqa: E402

SLOT = 4096                            # bytes of one array of a slot


def time_scene(origin, voxel, dims, capacity, depth, poses, K, reps, dev):
    vol = sparse_tsdf.SparseTSDFVolume(origin, voxel, dims, 4 * voxel, capacity, device=dev)
    _, alloc = vol.integrate_enqueue(depth, poses, K)
    in_use, dropped = int(alloc[3]), int(alloc[2])
    words = [vol.table, vol.slot_brick, vol.count, vol.tsdf, vol.weight]
    full = [t.clone() for t in words]

    def put(state=full):
        for t, s in zip(words, state):
            t.copy_(s)
    run = {"capacity_bricks": capacity, "bricks_of_the_grid": int(np.prod(vol.bricks)), "bricks_in_use": in_use, "bricks_dropped": dropped,
           "pool_bytes_in_use": in_use * 2 * SLOT}
    bx = np.sort(vol.allocated_bricks()[:, 0])
    far = 1.0e6
    rec = torch.empty(7, dtype=torch.int64, device=dev)
    arch = sparse_tsdf.BrickArchive.empty(in_use, False, False, dev)

    def box_for(fraction, tail=False):
        """About `fraction` of the bricks lie outside: those with bx below a threshold brick (the box begins half a voxel before its
        first voxel centre), which hold the FIRST slots -- slots are handed out in brick order, x slowest -- so that as many tail
        slots move into their holes; with `tail` those above it, the last slots, which leaves nothing to move"""
        if fraction >= 1.0:
            return torch.tensor([far, far, far, 2 * far, 2 * far, 2 * far], dtype=torch.float64, device=dev)
        if tail:
            edge = int(bx[int(round((1.0 - fraction) * (len(bx) - 1)))])
            return torch.tensor([-far, -far, -far, float(origin[0]) + voxel * (8 * edge + 0.5), far, far], dtype=torch.float64, device=dev)
        edge = int(bx[int(round(fraction * (len(bx) - 1)))])
        return torch.tensor([float(origin[0]) + voxel * (8 * edge - 0.5), -far, -far, far, far, far], dtype=torch.float64, device=dev)

    def note(name, ms, empty=False, archived=False):
        got = dict(zip(("candidates", "released", "released_outside", "released_empty", "deferred", "moved", "in_use"), rec.tolist()))
        moved, released = got["moved"], got["released"]
        touched = 2 * SLOT * (2 * moved + released) + (2 * 2 * SLOT * released if archived else 0) + (SLOT * in_use if empty else 0)
        run[name] = {"ms": ms, "released": released, "moved": moved, "bytes": touched, "GB_per_s": round(touched / ms / 1e6, 1) if ms > 0 else None}
    ms = timed(lambda: vol.release_enqueue(None, True, record=rec), reps, setup=put)
    note("release_empty", ms, empty=True)
    for name, fraction in (("quarter", 0.25), ("half", 0.5), ("all", 1.0)):
        box = box_for(fraction)
        ms = timed(lambda: vol.release_enqueue(box, record=rec), reps, setup=put)
        note(f"release_{name}", ms)
        ms = timed(lambda: vol.release_enqueue(box, record=rec, into=arch), reps, setup=put)
        note(f"release_{name}_archive", ms, archived=True)
        if name == "half":
            put()
            vol.release_enqueue(box, record=rec, into=arch)
            left = [t.clone() for t in words]
            back = torch.empty(7, dtype=torch.int64, device=dev)
            ms = timed(lambda: vol.restore_enqueue(arch, back), reps, setup=lambda: put(left))
            got = back.tolist()
            run["restore_half"] = {"ms": ms, "listed": got[0], "invalid": got[1], "restored": got[4], "bytes": 2 * 2 * SLOT * got[4],
                                   "GB_per_s": round(2 * 2 * SLOT * got[4] / ms / 1e6, 1)}
    tail = box_for(0.5, tail=True)
    ms = timed(lambda: vol.release_enqueue(tail, record=rec), reps, setup=put)
    note("release_half_tail", ms)
    put()
    n = depth.shape[0]
    frame_d, frame_p = depth[n - 1:].contiguous(), poses[n - 1:].contiguous()
    run["integrate_one_view_ms"] = timed(lambda: vol.integrate_enqueue(frame_d, frame_p, K), reps, setup=put)
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--big", type=int, default=1536)
    ap.add_argument("--views", type=int, default=256)
    ap.add_argument("--out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sparse_release_time.py needs a GPU")
    dev = torch.device("cuda:0")
    H, W, fx, fy, cx, cy = synth.intrinsics_after_crop(synth.config_reference_defaults())
    K = (fx, fy, cx, cy)
    marched, room = marched_room(dev, 128)
    lo, hi = room[0].min(0), room[0].max(0)
    centre = 0.5 * (lo + hi)
    poses = view_poses(args.views, centre).to(dev).contiguous()
    depth = torch.cat([mr.render_mesh_depth(marched, poses[k:k + 64], K, H, W)[0] for k in range(0, args.views, 64)])
    res = {"date": datetime.date.today().isoformat(), "image": [H, W], "views": args.views, "trunc_voxels": 4, "band": "trunc", "reps": args.reps, "runs": {}}
    with BoardSampler(dev.index or 0) as board:
        for name, side, capacity in (("256", args.res, 16384), ("1536", args.big, 262144)):
            voxel = float((hi - lo + 0.5).max() / (side - 1))
            origin = centre - 0.5 * voxel * (side - 1)
            run = {"dims": [side] * 3, "voxel_m": round(voxel, 5), "voxels": side ** 3}
            run.update(time_scene(origin, voxel, (side,) * 3, capacity, depth, poses, K, args.reps, dev))
            res["runs"][name] = run
            torch.cuda.empty_cache()
    res["board"] = board.summary()
    print(json.dumps(res, indent=1))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
