"""Generate the golden fixtures in this directory.  BUILD CONTAINER ONLY.

    python tests/golden/make_golden.py

Imports the reference's own Python from /root/reference (through oracle/ref_import.py,
which substitutes the absent tinycudann / pytorch3d and neutralises ``.cuda()``) and records
inputs + the reference's outputs as small ``.npz`` files.  The fixtures are data only.

Files written
  sampler.npz        sampling_helper.py:13-68 + mipsfusion.py:135-138 (depth image, seeds) -> indices
  losses.npz         helper_functions/utils.py:71-111 get_sdf_loss incl. edge cases
  decoder.npz        model/decoder.py:53-75 MLP_reg.forward + gradients
  scene_cfg1.npz     model/scene_rep.py:153-238 render_rays / forward (train, EMD 0.01 and 0, eval)
                     + gradients, BASELINE config 1 (256 rays x 16 samples, hash 2^10)
  scene_s75.npz      same with the reference's default S = 50 + 25 (> one wavefront), 64 rays
  scene_nd0.npz      same with training.n_samples_d = 0 (scene_rep.py:166-167: the depth-guided samples alone), 64 rays
  fresh_seed.npz     model/scene_rep.py forward (train) of a model the reference's constructor initialised, seed 123
  adam.npz           torch.optim.Adam with the two param groups of mipsfusion.py:580-584
  quaternion.npz     geometry_helper.py:11-17 qt_to_transform_matrix (+ grads) [pytorch3d unpinned]
  ba_trace.npz       loss-per-iteration trace of a 6-iteration local-BA-style loop (mipsfusion.py:293-342)
  ro.npz             RandomOptimizer.py:164-227 optimize (6 iterations, pose after each) + one get_fitness
  keyframe_rays.npz  model/keyframeSet.py:268-290, 386-455 ray samplers of the reference's KeyframeSet (seeded)
  ref_model_0.pth    a checkpoint as the reference writes it (Logger.py:33-34: torch.save(model.state_dict()))
  checkpoint_probe.npz  points + the reference model's query_color_sdf output for that checkpoint
  hashgrid.npz       ORACLE-generated (tinycudann absent => parity unpinned): hash-grid indices,
                     features and gradients at hash 2^10 and a sparse probe at hash 2^19
"""
import os
import random
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import ref_import, tcnn_cpu  # noqa: E402
from mipsfusion_amd import synth  # noqa: E402

ref = ref_import.load()


def seed_all(s=0):
    random.seed(s)
    np.random.seed(s)
    torch.manual_seed(s)


FILE_LIMIT = 1 << 20          # no committed file reaches 1 MiB


def save(name, **arrays):
    out = {}
    for k, v in arrays.items():
        if torch.is_tensor(v):
            v = v.detach().cpu().numpy()
        out[k] = np.asarray(v)
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **out)
    print(f"{name}: {os.path.getsize(path) / 1024:.0f} KiB, {len(out)} arrays")
    n = 1
    while os.path.exists(path) and os.path.getsize(path) >= FILE_LIMIT:
        # too large: <stem>.part1.npz, .part2.npz, ... (consecutive arrays of about equal size), which
        # tests/conftest.py::load_golden reads back as one fixture
        os.remove(path)
        n += 1
        keys, total = list(out), sum(v.nbytes for v in out.values())
        groups, acc = [[] for _ in range(n)], 0
        for k in keys:
            groups[min(n - 1, int(acc * n / max(total, 1)))].append(k)
            acc += out[k].nbytes
        parts = [os.path.join(HERE, f"{name[:-4]}.part{i + 1}.npz") for i in range(n)]
        for p, grp in zip(parts, groups):
            np.savez_compressed(p, **{k: out[k] for k in grp})
        if all(os.path.getsize(p) < FILE_LIMIT for p in parts):
            print(f"  in {n} parts: " + ", ".join(f"{os.path.getsize(p) / 1024:.0f} KiB" for p in parts))
            break
        for p in parts:
            os.remove(p)


class FixedRand:
    """Make ``torch.rand`` inside the reference return a recorded tensor (scene_rep.py:176)."""

    def __init__(self, noise):
        self.noise = noise

    def __enter__(self):
        self.orig = torch.rand
        torch.rand = lambda *a, **k: self.noise.clone()

    def __exit__(self, *exc):
        torch.rand = self.orig


# ------------------------------------------------------------------------- sampler
def gen_sampler():
    sh = ref.sampling_helper
    cfg = synth.config_plumbing()
    frame = synth.make_frame(cfg, seed=3)
    depth = frame["depth"]
    H, W = depth.shape
    out = {"depth": depth}
    rows, cols = sh.sample_pixels_uniformly(460, 620, 16, 24)
    out["uniform_460x620_16x24_rows"], out["uniform_460x620_16x24_cols"] = rows, cols
    rows, cols = sh.sample_pixels_uniformly(H, W, 4, 6)
    out["uniform_small_rows"], out["uniform_small_cols"] = rows, cols
    seed_all(11)
    out["random_seed11_n100"] = sh.sample_pixels_random(H, W, 100)
    seed_all(12)
    out["valid_random_seed12_n64"] = sh.sample_valid_pixels_random(depth, 64)
    seed_all(13)
    rows, cols = sh.sample_pixels_mix(H, W, 4, 6, depth, 120)
    out["mix_seed13_rows"], out["mix_seed13_cols"] = rows, cols
    out["mix_seed13_indices"] = sh.pixel_rc_to_indices(rows, cols, H, W)
    seed_all(14)
    out["select_samples_seed14_n50"] = torch.tensor(random.sample(range(H * W), 50))
    save("sampler.npz", **out)


# -------------------------------------------------------------------------- losses
def gen_losses():
    seed_all(1)
    N, S = 48, 16
    z = torch.sort(torch.rand(N, S) * 5, -1).values
    d = torch.rand(N, 1) * 4 + 0.3
    d[::7] = 0.0
    sdf = torch.tanh(torch.randn(N, S))
    prob = torch.softmax(torch.randn(N, S, 5), -1)
    out = dict(z_vals=z, target_d=d, sdf=sdf, prob=prob, truncation=0.1)
    for tag, w in (("emd", 0.01), ("noemd", 0.0)):
        s = sdf.clone().requires_grad_(True)
        p = prob.clone().requires_grad_(True)
        fs, sd = ref.utils.get_sdf_loss(z, d, s, p, 0.1, 5, w, "l2")
        (3.0 * fs + 7.0 * sd).backward()
        out[f"{tag}_fs"], out[f"{tag}_sdf"] = fs, sd
        out[f"{tag}_dsdf"] = s.grad
        out[f"{tag}_dprob"] = p.grad if p.grad is not None else torch.zeros_like(p)
    # edge: no sample in front nor in band (all depths invalid) -> 0/0 weights -> NaN
    d0 = torch.zeros(N, 1)
    fs, sd = ref.utils.get_sdf_loss(z, d0, sdf, prob, 0.1, 5, 0.01, "l2")
    out["nodepth_fs"], out["nodepth_sdf"] = fs, sd
    fm, sm, fw, sw = ref.utils.get_masks(z, d, 0.1)
    out["front_mask"], out["sdf_mask"], out["fs_weight"], out["sdf_weight"] = fm, sm, fw, sw
    save("losses.npz", **out)


# ------------------------------------------------------------------------- decoder
def gen_decoder():
    seed_all(2)
    dec = ref.decoder.MLP_reg({}, input_ch=32, input_ch_pos=48)
    M = 200
    embed = (torch.randn(M, 32) * 0.1).requires_grad_(True)
    x = torch.rand(M, 3).requires_grad_(True)
    pe = torch.randn(M, 48).clamp(-1, 1).requires_grad_(True)
    out = dec(embed, pe, x)
    gout = torch.randn(M, 10)
    out.backward(gout)
    arrays = dict(embed=embed, embed_pos=pe, x=x, out=out, gout=gout, d_embed=embed.grad, d_embed_pos=pe.grad,
                  d_x=x.grad)
    for k, v in dec.state_dict().items():
        arrays["w." + k] = v
    for k, v in dec.named_parameters():
        arrays["g." + k] = v.grad
    save("decoder.npz", **arrays)


# --------------------------------------------------------------------------- scene
def scene_case(cfg, n_rays, name, seed):
    seed_all(seed)
    bb = torch.from_numpy(np.array(cfg["mapping"]["bound"]))
    nf = torch.from_numpy(np.array(cfg["mapping"]["localMLP_max_len"]))
    model = ref.scene_rep.JointEncoding(cfg, bb, nf)
    # non-trivial grid values so that SDF sign changes occur along rays
    with torch.no_grad():
        model.embed_fn.params.copy_(torch.randn_like(model.embed_fn.params) * 0.3)
        model.decoder.sdf_linear[2].weight.mul_(6.0)
    frame = synth.make_frame(cfg, seed=seed)
    H, W = frame["depth"].shape
    idx = torch.tensor(random.sample(range(H * W), n_rays))
    c2w = frame["c2w"]
    rays_o, rays_d, tgt_rgb, tgt_d = synth.ray_batch(frame, idx, c2w)
    S = cfg["training"]["n_samples_d"] + cfg["training"]["n_range_d"]
    noise = torch.rand(n_rays, S)
    arrays = dict(rays_o=rays_o, rays_d=rays_d, target_rgb=tgt_rgb, target_d=tgt_d, noise=noise, pixel_idx=idx,
                  bound=bb, half_len=nf)
    for k, v in model.state_dict().items():
        arrays["w." + k] = v

    model.eval()
    with torch.no_grad(), FixedRand(noise):
        ev = model.forward(rays_o, rays_d, tgt_rgb, tgt_d)
    for k in ("rgb", "depth", "disp_map", "acc_map", "depth_var", "z_vals", "raw"):
        arrays["eval." + k] = ev[k]
    # eval without depth guidance (render_rays(target_d=None), Logger.py:205 style)
    noise_nd = torch.rand(n_rays, cfg["training"]["n_samples"])
    with torch.no_grad(), FixedRand(noise_nd):
        nd = model.render_rays(rays_o, rays_d, target_d=None)
    arrays["noise_nodepth"] = noise_nd
    for k in ("rgb", "depth", "z_vals", "raw"):
        arrays["nodepth." + k] = nd[k]

    model.train()
    tr = cfg["training"]
    for tag, w in (("emd", 0.01), ("noemd", 0.0)):
        model.zero_grad()
        ro = rays_o.clone().requires_grad_(True)
        rd = rays_d.clone().requires_grad_(True)
        with FixedRand(noise):
            ret = model.forward(ro, rd, tgt_rgb, tgt_d, EMD_w=w)
        loss = (tr["rgb_weight"] * ret["rgb_loss"] + tr["depth_weight"] * ret["depth_loss"]
                + tr["sdf_weight"] * ret["sdf_loss"] + tr["fs_weight"] * ret["fs_loss"])
        loss.backward()
        for k in ("rgb", "depth", "rgb_loss", "depth_loss", "sdf_loss", "fs_loss", "psnr"):
            arrays[f"{tag}.{k}"] = ret[k]
        arrays[f"{tag}.loss"] = loss
        arrays[f"{tag}.d_rays_o"], arrays[f"{tag}.d_rays_d"] = ro.grad, rd.grad
        for k, v in model.named_parameters():
            if v.numel():
                arrays[f"{tag}.g.{k}"] = v.grad
    save(name, **arrays)


def gen_fresh_seed():
    """The training forward of the reference's JointEncoding at a seed no other fixture uses (model initialised by the
    reference's constructor at torch seed 123, grid values N(0, 0.2^2), 64 random rays with three of zero depth): state dict,
    inputs and the returned rgb / depth / losses."""
    cfg = synth.config_plumbing()
    torch.manual_seed(123)
    bb = torch.from_numpy(np.array(cfg["mapping"]["bound"]))
    nf = torch.from_numpy(np.array(cfg["mapping"]["localMLP_max_len"]))
    model = ref.scene_rep.JointEncoding(cfg, bb, nf)
    with torch.no_grad():
        model.embed_fn.params.copy_(torch.randn_like(model.embed_fn.params) * 0.2)
    N, S = 64, 16
    ro = torch.rand(N, 3) * 0.2
    rd = torch.nn.functional.normalize(torch.randn(N, 3), dim=-1)
    rgb, d = torch.rand(N, 3), torch.rand(N, 1) * 1.5
    d[:3] = 0
    noise = torch.rand(N, S)
    arrays = dict(rays_o=ro, rays_d=rd, target_rgb=rgb, target_d=d, noise=noise, bound=bb, half_len=nf)
    for k, v in model.state_dict().items():
        arrays["w." + k] = v
    model.train()
    with FixedRand(noise):
        r = model.forward(ro, rd, rgb, d)
    for k in ("rgb", "depth", "rgb_loss", "depth_loss", "sdf_loss", "fs_loss"):
        arrays["train." + k] = r[k]
    save("fresh_seed.npz", **arrays)


def gen_scene_nd0():
    """training.n_samples_d = 0: the branch `z_vals = z_samples` of model/scene_rep.py:166-167 -- the depth-guided samples
    alone, no uniform list, no sort.  No shipped configuration sets it; the reference accepts it."""
    c = synth.config_plumbing()
    c["training"].update(n_samples_d=0, n_range_d=16, n_samples=16)
    scene_case(c, 64, "scene_nd0.npz", seed=10)


# ---------------------------------------------------------------------------- adam
def gen_adam():
    seed_all(4)
    n_grid, n_dec, steps = 4096, 600, 6
    pg = (torch.rand(n_grid) * 2 - 1) * 1e-4
    pd = torch.randn(n_dec) * 0.1
    grid = torch.nn.Parameter(pg.clone())
    dec = torch.nn.Parameter(pd.clone())
    opt = torch.optim.Adam([{"params": [dec], "weight_decay": 1e-6, "lr": 0.01},
                            {"params": [grid], "eps": 1e-15, "lr": 0.01}], betas=(0.9, 0.99))
    grads_g, grads_d, traj_g, traj_d = [], [], [], []
    for s in range(steps):
        gg = torch.randn(n_grid) * 1e-3
        gg[torch.rand(n_grid) < 0.7] = 0.0          # most grid entries untouched: dense semantics matter
        gd = torch.randn(n_dec) * 1e-2
        grid.grad, dec.grad = gg.clone(), gd.clone()
        opt.step()
        grads_g.append(gg), grads_d.append(gd)
        traj_g.append(grid.detach().clone()), traj_d.append(dec.detach().clone())
    st_g, st_d = opt.state[grid], opt.state[dec]
    save("adam.npz", grid0=pg, dec0=pd, grid_grads=torch.stack(grads_g), dec_grads=torch.stack(grads_d),
         grid_traj=torch.stack(traj_g), dec_traj=torch.stack(traj_d), grid_m=st_g["exp_avg"],
         grid_v=st_g["exp_avg_sq"], dec_m=st_d["exp_avg"], dec_v=st_d["exp_avg_sq"])


# ---------------------------------------------------------------------- quaternion
def gen_quaternion():
    seed_all(5)
    gh = ref.geometry_helper
    rot = torch.randn(9, 4)
    rot[0] = torch.tensor([1.0, 0.0, 0.0, 0.0])
    rot = rot.requires_grad_(True)
    trans = torch.randn(9, 3).requires_grad_(True)
    T = gh.qt_to_transform_matrix(rot, trans)
    g = torch.randn_like(T)
    T.backward(g)
    q_back = gh.matrix_to_quaternion(T[:, :3, :3].detach())
    save("quaternion.npz", rot=rot, trans=trans, T=T, gT=g, d_rot=rot.grad, d_trans=trans.grad, q_back=q_back)


# ------------------------------------------------------------------------ BA trace
def gen_ba_trace():
    """6 iterations of the mapping loop (mipsfusion.py:293-342) for ONE keyframe pose being
    optimised together with the map; records losses and final parameters."""
    seed_all(6)
    cfg = synth.config_plumbing()
    tr = cfg["training"]
    bb = torch.from_numpy(np.array(cfg["mapping"]["bound"]))
    nf = torch.from_numpy(np.array(cfg["mapping"]["localMLP_max_len"]))
    model = ref.scene_rep.JointEncoding(cfg, bb, nf)
    model.train()
    gh = ref.geometry_helper
    frame = synth.make_frame(cfg, seed=6)
    H, W = frame["depth"].shape
    opt = torch.optim.Adam([{"params": model.decoder.parameters(), "weight_decay": 1e-6, "lr": 0.01},
                            {"params": model.embed_fn.parameters(), "eps": 1e-15, "lr": 0.01}], betas=(0.9, 0.99))
    pose0 = frame["c2w"][None].clone()
    pose0[0, :3, 3] += 0.02
    cur_trans = torch.nn.Parameter(pose0[:, :3, 3].clone())
    cur_rot = torch.nn.Parameter(gh.matrix_to_quaternion(pose0[:, :3, :3]))
    pose_opt = torch.optim.Adam([{"params": cur_rot, "lr": 1e-3}, {"params": cur_trans, "lr": 1e-3}])
    w0 = {k: v.clone() for k, v in model.state_dict().items()}
    S = tr["n_samples_d"] + tr["n_range_d"]
    iters, n = 6, 128
    idxs, noises, losses = [], [], []
    poses_all = gh.qt_to_transform_matrix(cur_rot, cur_trans)
    opt.zero_grad(), pose_opt.zero_grad()
    for i in range(iters):
        idx = torch.tensor(random.sample(range(H * W), n))
        noise = torch.rand(n, S)
        r, c = torch.div(idx, W, rounding_mode="floor"), torch.remainder(idx, W)
        d_cam, t_rgb, t_d = frame["direction"][r, c], frame["rgb"][r, c], frame["depth"][r, c][:, None]
        which = torch.zeros(n, dtype=torch.int64)
        rays_d = torch.sum(d_cam[..., None, None, :] * poses_all[which, None, :3, :3], -1).reshape(-1, 3)
        rays_o = poses_all[which, :3, -1].reshape(-1, 3)
        with FixedRand(noise):
            ret = model.forward(rays_o, rays_d, t_rgb, t_d)
        loss = (tr["rgb_weight"] * ret["rgb_loss"] + tr["depth_weight"] * ret["depth_loss"]
                + tr["sdf_weight"] * ret["sdf_loss"] + tr["fs_weight"] * ret["fs_loss"])
        loss.backward(retain_graph=True)
        opt.step()
        opt.zero_grad()
        if (i + 1) % 2 == 0:                       # pose_accum_step = 2 (ScanNet setting)
            pose_opt.step()
            poses_all = gh.qt_to_transform_matrix(cur_rot, cur_trans)
            pose_opt.zero_grad()
        idxs.append(idx), noises.append(noise), losses.append(loss.detach())
    arrays = dict(pixel_idx=torch.stack(idxs), noise=torch.stack(noises), losses=torch.stack(losses),
                  pose0=pose0, rot_final=cur_rot, trans_final=cur_trans, frame_seed=6)
    for k, v in w0.items():
        arrays["w0." + k] = v
    for k, v in model.state_dict().items():
        if k.startswith("decoder"):
            arrays["w1." + k] = v
    arrays["w1.embed_fn.params"] = model.embed_fn.params
    save("ba_trace.npz", **arrays)


# ------------------------------------------------------------------------ hashgrid
def gen_hashgrid():
    seed_all(7)
    pls = float(2.0 ** (np.log2(256 / 16) / 15))
    out = {}
    for tag, log2_t, M in (("t10", 10, 384), ("t19", 19, 96)):
        meta = tcnn_cpu.make_grid_meta(16, 2, log2_t, 16, pls)
        x = torch.rand(M, 3)
        x[0] = torch.tensor([0.0, 0.0, 0.0])
        x[1] = torch.tensor([1.0, 1.0, 1.0])
        x[2] = torch.tensor([1.0, 0.0, 0.5])
        x[3] = torch.tensor([-0.05, 1.07, 0.5])     # outside the box: uint32 wrap of (int) casts
        x[4] = torch.tensor([0.5, 0.5, 0.5])
        g = torch.Generator().manual_seed(1000 + log2_t)
        params = (torch.rand(meta.n_params, generator=g) * 2 - 1) * 0.5
        dy = torch.randn(M, 32)
        y = tcnn_cpu.hashgrid_forward(x, params, meta)
        idx = tcnn_cpu.hashgrid_indices(x, meta)
        dparams, dx = tcnn_cpu.hashgrid_backward(x, params, dy, meta)
        out[f"{tag}.x"], out[f"{tag}.dy"], out[f"{tag}.y"] = x, dy, y
        out[f"{tag}.idx"] = idx.to(torch.int32)
        out[f"{tag}.dx"] = dx
        out[f"{tag}.param_seed"] = 1000 + log2_t
        out[f"{tag}.offsets"] = np.array(meta.offsets, dtype=np.int64)
        out[f"{tag}.scales"] = np.array(meta.scales, dtype=np.float32)
        out[f"{tag}.resolutions"] = np.array(meta.resolutions, dtype=np.int64)
        nz = torch.nonzero(dparams).squeeze(-1)
        out[f"{tag}.dparams_nz_idx"], out[f"{tag}.dparams_nz_val"] = nz.to(torch.int32), dparams[nz]
        if log2_t == 10:
            out[f"{tag}.params"] = params
    xf = torch.rand(64, 3)
    xf[0] = 0.0
    xf[1] = 1.0
    out["freq.x"] = xf
    out["freq.y8"] = tcnn_cpu.frequency_forward(xf, 8)
    gy = torch.randn(64, 48)
    out["freq.dy"] = gy
    out["freq.dx8"] = tcnn_cpu.frequency_backward(xf, gy, 8)
    save("hashgrid.npz", **out)


# ------------------------------------------------------------------- RandomOptimizer
def gen_ro():
    """RandomOptimizer.optimize (RandomOptimizer.py:164-227) on BASELINE config 1 with a small particle swarm.
    The reference's class is imported unmodified (pytorch3d.transforms -> oracle/p3d_cpu, see ref_import)."""
    import importlib
    import types
    RO = importlib.import_module("RandomOptimizer")
    seed_all(11)
    cfg = synth.config_plumbing()
    cfg["tracking"]["RO"] = dict(cfg["tracking"].get("RO", {}), particle_size=96, n_rows=4, n_cols=6,
                                 initial_scaling_factor=0.02, rescaling_factor=0.5)
    cfg["tracking"].setdefault("ignore_edge_W", 2)
    cfg["tracking"].setdefault("ignore_edge_H", 2)
    bb = torch.from_numpy(np.array(cfg["mapping"]["bound"]))
    nf = torch.from_numpy(np.array(cfg["mapping"]["localMLP_max_len"]))
    model = ref.scene_rep.JointEncoding(cfg, bb, nf)
    with torch.no_grad():
        model.embed_fn.params.copy_(torch.randn_like(model.embed_fn.params) * 0.3)
        model.decoder.sdf_linear[2].weight.mul_(6.0)
    model.eval()
    frame = synth.make_frame(cfg, seed=11)
    H, W, fx, fy, cx, cy = synth.intrinsics_after_crop(cfg)
    depth = frame["depth"].clone()
    dataset = types.SimpleNamespace(H=H, W=W, fx=fx, fy=fy, cx=cx, cy=cy, rays_d=frame["direction"])
    slam = types.SimpleNamespace(dataset=dataset, device=torch.device("cpu"))
    ro = RO.RandomOptimizer(cfg, slam)
    depth[ro.row_indices[3] + 1, ro.col_indices[3] + 1] = 0.0   # an invalid lattice pixel (valid_mask branch, offset 1)
    depth[ro.row_indices[7], ro.col_indices[7]] = 0.0
    c2w = frame["c2w"].clone()
    # start a little away from the true pose so that the swarm finds better particles
    init = c2w.clone()
    init[:3, 3] += torch.tensor([0.03, -0.02, 0.025])
    arrays = dict(pst=ro.pre_sampled_particle, rows=ro.row_indices, cols=ro.col_indices, depth=depth,
                  rays_dir=dataset.rays_d, init_pose=init, bound=bb, half_len=nf,
                  particle_size=96, n_rows=4, n_cols=6, c1=0.02, c2=0.5, trunc=cfg["training"]["trunc"])
    for k, v in model.state_dict().items():
        arrays["w." + k] = v
    for n_iter in range(0, 7):
        arrays[f"pose_after_{n_iter}"] = ro.optimize(model, depth, init.clone(), c2w, n_iter=n_iter)
    # one fitness evaluation in isolation (RandomOptimizer.py:113-131)
    pst7 = ro.pose_6D_to_7D(ro.pre_sampled_particle * 0.02)
    rot, trans = ro.get_abs_pose(init[:3, :3], init[:3, 3:], pst7)
    td = depth[ro.row_indices, ro.col_indices].unsqueeze(-1)
    rd = dataset.rays_d[ro.row_indices, ro.col_indices, :]
    with torch.no_grad():
        fit, mms = ro.get_fitness(model, rot, trans, c2w, td, rd)
    arrays.update(fit0=fit, mean_masked0=mms, pst7_0=pst7, abs_rot0=rot, abs_trans0=trans)
    save("ro.npz", **arrays)


# ------------------------------------------------------------------- keyframe ray sampling
def gen_keyframe_rays():
    """model/keyframeSet.py ray samplers (:268-290, :386-455) of the reference's own KeyframeSet: for a seeded
    python RNG and a random ray database, which rows come out (rays, kf_ids, kf_indices)."""
    import importlib
    KF = importlib.import_module("model.keyframeSet")
    cfg = {"sampling": {"kf_n_rays_h": 6, "kf_n_rays_w": 8},
           "mapping": {"localMLP_num": 2, "localMLP_max_len": [7.0, 7.0, 7.0], "overlapping": {"n_rays_h": 2, "n_rays_w": 2}}}
    num_kf = 7
    kfs = KF.KeyframeSet(cfg, 32, 32, num_kf, torch.device("cpu"))
    seed_all(21)
    kfs.rays = torch.randn(num_kf, kfs.num_rays_to_save, 7)
    kfs.frame_ids = torch.arange(num_kf, dtype=torch.float32) * 5
    arrays = dict(db=kfs.rays, num_rays_to_save=kfs.num_rays_to_save)
    cases = {"sub1": (torch.tensor(2), torch.tensor([2]), 40), "sub2": (torch.tensor(1), torch.tensor([1, 4]), 40),
             "sub5": (torch.tensor(0), torch.tensor([0, 2, 3, 5, 6]), 45)}
    for name, (first, rel, n) in cases.items():
        random.seed(100 + n)
        rays, kf_ids, kf_indices = kfs.sample_rays_in_submap(first, rel, n)
        arrays.update({f"{name}.first": first, f"{name}.related": rel, f"{name}.n": n, f"{name}.seed": 100 + n,
                       f"{name}.rays": rays, f"{name}.kf_ids": kf_ids, f"{name}.kf_indices": kf_indices})
    random.seed(7)
    rays, kf_ids, kf_indices = kfs.sample_rays_in_given_kf(torch.tensor([6, 1, 3]), 30)
    arrays.update({"given.rays": rays, "given.kf_ids": kf_ids, "given.kf_indices": kf_indices})
    random.seed(8)
    rays, kf_ids = kfs.sample_global_rays(25)
    arrays.update({"global.rays": rays, "global.kf_ids": kf_ids})
    random.seed(9)
    rays, kf_indices = kfs.sample_rays_from_given(torch.tensor([5, 0]), 20)
    arrays.update({"from_given.rays": rays, "from_given.kf_indices": kf_indices})
    save("keyframe_rays.npz", **arrays)


# ------------------------------------------------------------------- checkpoint format
def gen_checkpoint():
    """A checkpoint exactly as the reference writes it (Logger.py:33-34, 267-277: torch.save(model.state_dict())),
    from the reference's own JointEncoding at BASELINE config 1, plus the eval output it must reproduce."""
    seed_all(31)
    cfg = synth.config_plumbing()
    bb = torch.from_numpy(np.array(cfg["mapping"]["bound"]))
    nf = torch.from_numpy(np.array(cfg["mapping"]["localMLP_max_len"]))
    model = ref.scene_rep.JointEncoding(cfg, bb, nf)
    with torch.no_grad():
        model.embed_fn.params.copy_(torch.randn_like(model.embed_fn.params) * 0.3)
    torch.save(model.state_dict(), os.path.join(HERE, "ref_model_0.pth"))
    pts = torch.rand(64, 3)
    with torch.no_grad():
        out = model.query_color_sdf(pts)
    save("checkpoint_probe.npz", pts=pts, out=out, bound=bb, half_len=nf)
    print("ref_model_0.pth:", os.path.getsize(os.path.join(HERE, "ref_model_0.pth")) // 1024, "KiB")


# ------------------------------------------------------------------- two-submap sequence (BASELINE config 3)
def reference_backend():
    """tests/seq_harness.py Backend over the REFERENCE's own classes (CPU)."""
    import copy
    import importlib
    import types
    KF = importlib.import_module("model.keyframeSet")
    RO = importlib.import_module("RandomOptimizer")
    gh = ref.geometry_helper

    def make_model(cfg, bb, nf):
        return ref.scene_rep.JointEncoding(cfg, bb, nf)

    return types.SimpleNamespace(
        device=torch.device("cpu"), make_model=make_model, deepcopy=copy.deepcopy, Adam=torch.optim.Adam,
        sh=ref.sampling_helper, qt_to_transform_matrix=gh.qt_to_transform_matrix,
        matrix_to_quaternion=gh.matrix_to_quaternion,
        make_kfset=lambda cfg, H, W, n: KF.KeyframeSet(cfg, H, W, n, torch.device("cpu")),
        make_ro=lambda cfg, slam: RO.RandomOptimizer(cfg, slam),
        ro_optimize=lambda ro, model, depth, init, last, n: ro.optimize(model, depth, init, last, n_iter=n))


def gen_sequence():
    """tests/seq_harness.run_sequence over the reference's classes: index stream, loss trace, poses, both sub-maps'
    final weights (mipsfusion.py:661-735 loop with a switch to a new sub-map and a switch back)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import seq_harness
    out = seq_harness.run_sequence(reference_backend())
    arrays = dict(losses=out["losses"], est=out["est"], tags=np.array(out["tags"]),
                  idx_flat=torch.cat(out["idx"]), idx_len=np.array([t.numel() for t in out["idx"]]))
    keep = ("decoder.pts_linear.0.weight", "decoder.sdf_linear.2.weight", "decoder.rgb_linear.0.bias", "embed_fn.params")
    for sm, sd in out["models"].items():
        for k in keep:
            arrays[f"m{sm}.{k}"] = sd[k]
    for k in keep[:2]:
        arrays[f"copy.{k}"] = out["active_copy"][k]
    save("sequence.npz", **arrays)


if __name__ == "__main__":
    if len(sys.argv) > 1:                       # python make_golden.py gen_sequence  -> only that fixture
        for name in sys.argv[1:]:
            globals()[name]()
        sys.exit(0)
    gen_sequence()
    gen_sampler()
    gen_losses()
    gen_decoder()
    scene_case(synth.config_plumbing(), 256, "scene_cfg1.npz", seed=8)
    c75 = synth.config_plumbing()
    c75["training"].update(n_samples_d=50, n_range_d=25, n_samples=75)
    scene_case(c75, 64, "scene_s75.npz", seed=9)
    gen_scene_nd0()
    gen_fresh_seed()
    gen_adam()
    gen_quaternion()
    gen_ba_trace()
    gen_hashgrid()
    gen_ro()
    gen_keyframe_rays()
    gen_checkpoint()
