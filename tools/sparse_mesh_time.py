"""Times the sparse volume's mesh marched brick by brick (SparseTSDFVolume.extract_mesh_bricks) beside the windowed path
(to_dense and the dense marcher) on one GPU, on tools/sparse_time.py's scene: the marched 128^3 box room seen from 64 views of
460 x 620 pixels, fused at 256^3 and at 1536^3 voxels.

    python tools/sparse_mesh_time.py [--reps 5] [--res 256] [--big 1536] [--views 64] [--out file.json]

Three comparisons, each in the same run; "march" is the soup, the weld and the face filters with the mesh left on the device (what
mesh.marching_cubes(return_device=True) does), host wall time with a synchronise since both paths read counts back, median of --reps
after one warm-up:
  both          the --res^3 scene: bricks against to_dense() over the tight window + marching cubes
  window        the 512^3 corner window of the --big^3 scene, as a grid of its own with the same voxels (the same views fused, so
                its bricks are the window's): bricks against to_dense() + marching cubes of that window
  whole         the whole --big^3 scene in one call against a loop of windowed calls over 512^3 tiles of its tight box, not stitched
and the parts on their own: the count between two events on the stream, the count with the emit and the weld as host wall time.  The
whole scene is timed twice, with a pool of 131072 slots and with the largest pool: the count and the emit launch a workgroup per slot of
the pool.  The shader clock and package power sampled across the timed regions are printed beside the times (bench.BoardSampler), the
date too."""
import argparse
import datetime
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import BoardSampler                                                # noqa: E402
from mipsfusion_amd import _lib, mesh as mesh_mod, mesh_render as mr, sparse_tsdf, synth   # noqa: E402
from tools.raster_time import marched_room, timed, view_poses                # noqa: E402
from tools.tsdf_time import wall                                              # noqa: E402


def march_bricks(vol):
    soup, tri_slot, _ = vol.brick_soup_enqueue()
    v, f = vol.weld_bricks(soup, tri_slot)
    return v, mesh_mod.filter_faces(f)[0]


def march_window(vol, lo, hi):
    return mesh_mod.marching_cubes(vol.to_dense(lo, hi).volume(), 0.0, truncation=1.0, return_device=True)


def tiles(lo, hi, side=512):
    return [((x, y, z), (min(x + side, hi[0]), min(y + side, hi[1]), min(z + side, hi[2])))
            for x in range(lo[0], hi[0], side) for y in range(lo[1], hi[1], side) for z in range(lo[2], hi[2], side)]


def fused(origin, voxel, dims, capacity, depth, poses, K, dev):
    vol = sparse_tsdf.SparseTSDFVolume(origin, voxel, dims, 4 * voxel, capacity, device=dev)
    _, alloc = vol.integrate_enqueue(depth, poses, K)
    return vol, int(alloc[3]), int(alloc[2])


def time_bricks(vol, reps):
    run = {"capacity_bricks": vol.capacity, "bricks_march_ms": wall(lambda: march_bricks(vol), reps)}
    run["count_ms"] = timed(lambda: vol._mesh_args(1.0), reps)
    soup, tri_slot, _ = vol.brick_soup_enqueue()
    run["count_and_emit_ms"] = wall(lambda: vol.brick_soup_enqueue(), reps)
    run["weld_ms"] = wall(lambda: vol.weld_bricks(soup, tri_slot), reps)
    v, f = march_bricks(vol)
    run.update(triangles=int(soup.shape[0]), vertices=int(v.shape[0]), faces=int(f.shape[0]))
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--big", type=int, default=1536)
    ap.add_argument("--views", type=int, default=64)
    ap.add_argument("--out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sparse_mesh_time.py needs a GPU")
    dev = torch.device("cuda:0")
    H, W, fx, fy, cx, cy = synth.intrinsics_after_crop(synth.config_reference_defaults())
    K = (fx, fy, cx, cy)
    marched, room = marched_room(dev, 128)
    lo, hi = room[0].min(0), room[0].max(0)
    centre = 0.5 * (lo + hi)
    poses = view_poses(args.views, centre).to(dev).contiguous()
    depth, _ = mr.render_mesh_depth(marched, poses, K, H, W)
    res = {"date": datetime.date.today().isoformat(), "image": [H, W], "views": args.views, "reps": args.reps, "runs": {}}

    def grid(side):
        voxel = float((hi - lo + 0.5).max() / (side - 1))
        return centre - 0.5 * voxel * (side - 1), voxel

    with BoardSampler(dev.index or 0) as board:
        # ---- the scene both volumes take
        origin, voxel = grid(args.res)
        vol, in_use, dropped = fused(origin, voxel, (args.res,) * 3, 16384, depth, poses, K, dev)
        window = vol.tight_window()
        run = {"dims": [args.res] * 3, "bricks_in_use": in_use, "bricks_dropped": dropped, "window": [list(window[0]), list(window[1])]}
        run["bricks"] = time_bricks(vol, args.reps)
        run["windowed_march_ms"] = wall(lambda: march_window(vol, *window), args.reps)
        run["windowed_faces"] = int(march_window(vol, *window)[1].shape[0])
        res["runs"]["both"] = run
        del vol
        torch.cuda.empty_cache()
        # ---- the corner window of the large scene, as a grid of its own
        origin, voxel = grid(args.big)
        side = min(args.big, 512)
        vol, in_use, dropped = fused(origin, voxel, (side,) * 3, 65536, depth, poses, K, dev)
        run = {"dims": [side] * 3, "of": [args.big] * 3, "bricks_in_use": in_use, "bricks_dropped": dropped}
        run["bricks"] = time_bricks(vol, args.reps)
        run["windowed_march_ms"] = wall(lambda: march_window(vol, (0, 0, 0), (side,) * 3), args.reps)
        run["windowed_faces"] = int(march_window(vol, (0, 0, 0), (side,) * 3)[1].shape[0])
        res["runs"]["window"] = run
        del vol
        torch.cuda.empty_cache()
        # ---- the whole large scene
        run = {"dims": [args.big] * 3, "voxels": args.big ** 3}
        for capacity in (131072, _lib.SPARSE_MAX_CAPACITY):
            vol, in_use, dropped = fused(origin, voxel, (args.big,) * 3, capacity, depth, poses, K, dev)
            run.update(bricks_in_use=in_use, bricks_dropped=dropped)
            run[f"bricks_capacity_{capacity}"] = time_bricks(vol, args.reps)
            if capacity != _lib.SPARSE_MAX_CAPACITY:
                del vol
                torch.cuda.empty_cache()
        box = vol.tight_window()
        parts = tiles(*box)
        run["tight_box"], run["tiles"] = [list(box[0]), list(box[1])], len(parts)
        run["windowed_loop_ms"] = wall(lambda: [march_window(vol, a, b) for a, b in parts], min(args.reps, 3))
        run["windowed_loop_faces_unstitched"] = int(sum(march_window(vol, a, b)[1].shape[0] for a, b in parts))
        res["runs"]["whole"] = run
    res["board"] = board.summary()
    print(json.dumps(res, indent=1))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
