"""Golden PARAMETER GRADIENTS from the real reference's autograd.

Run in the build container only (needs /root/reference, see oracle/ref_harness.py):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_grads.py
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_grads.py --samples 128       # full_train_grads_s128
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_grads.py --samples 200       # full_train_grads_s200
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_grads.py --samples 128 w4    # full_train_grads_w4_s128

For each case the reference's Renderer.render runs in train mode (seed 233: jitter, then noise, from the CPU
generator), the reference's own loss module (utils/loss.py, L2 + occupancy mask term) is applied, and
loss.backward() fills the .grad of the 33 parameters - including the double-backward path through
d sigma/dx -> normal -> lighting.  Stored: the batch, the random draws, the forward outputs, the loss terms and,
per parameter, the full gradient (<= 20 000 elements) or a fixed-stride sample of 4096 elements, plus its L2 norm
and sum; the same from a float64 run of the reference (suffix _f64) as the noise floor.  Data only.
"""
from __future__ import annotations

import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(ROOT, "oracle"))
spec = importlib.util.spec_from_file_location("synth", os.path.join(ROOT, "dual-space-nerf_amd", "synth.py"))
synth = importlib.util.module_from_spec(spec)
spec.loader.exec_module(synth)
import ref_harness as rh  # noqa: E402

TH = (0.2, -0.1, 1.0)
FRAME = 5
FULL_LIMIT = 20000
SAMPLE = 4096


def sample_index(n):
    return (np.arange(SAMPLE, dtype=np.int64) * 2654435761 + 12345) % n


def grads_of(render, batch, seed, loss_fn, dtype):
    import torch
    render.train()
    torch.manual_seed(seed)
    b = {k: (v.clone() if hasattr(v, "clone") else v) for k, v in batch.items()}
    ret = render.render(b)["coarse"]
    fwd = {k: v.detach().numpy().copy() for k, v in ret.items()}
    terms = loss_fn(ret, b)                     # utils/loss.py: may edit acc_map in place, like the trainer's call
    loss = 0
    for k in terms:
        loss = loss + terms[k]                  # trainer.py:73-76
    render.net.zero_grad()
    loss.backward()
    out = {"loss": np.float64(loss.item())}
    for k in terms:
        out["loss:" + k] = np.float64(terms[k].item())
    for name, p in render.net.named_parameters():
        g = p.grad.detach().double().numpy().reshape(-1)
        out["norm:" + name] = np.float64(np.linalg.norm(g))
        out["sum:" + name] = np.float64(g.sum())
        sel = g if g.size <= FULL_LIMIT else g[sample_index(g.size)]
        out["grad:" + name] = sel.astype(np.float64 if dtype == "float64" else np.float32)
    return fwd, out


def case(name, canon, faces, xyz, poses, rays, sel, S, state, raw_noise_std, seed=233, config2=False, compact=False):
    """config2: BASELINE configs[2]'s own size (8192 rays x 64 samples).  float32 reference only (its float64 twin does not fit the
    build container's memory), and the fixture keeps what cannot be regenerated: the loss, the 33 norms / sums / sub-sampled
    gradients and the per-ray outputs - rays, body, draws and targets are functions of the seeds (tests/test_gpu_train.py rebuilds
    them the same way)."""
    import torch
    rh.install_shims()
    from utils.loss import make_loss            # the reference's loss module (torch only)

    R = len(sel)
    target = synth.hash_uniform(R * 3, 91).reshape(R, 3).astype(np.float32)
    occ = (synth.hash_uniform(R, 92) > 0.5).astype(np.float32)
    arrs = dict(canonical_vertex=canon, faces=faces.astype(np.int32), xyz=xyz, poses=poses, Th=np.asarray(TH, np.float32),
                frame=np.int64(FRAME), S=np.int64(S), ray_o=rays["ray_o"][sel], ray_d=rays["ray_d"][sel],
                near=rays["near"][sel], far=rays["far"][sel], target_rgb=target, occupancy=occ,
                raw_noise_std=np.float64(raw_noise_std), seed=np.int64(seed))
    torch.manual_seed(seed)                     # the draws the reference will make (pts_utils.py:12, nerf_net_utils.py:31)
    arrs["jitter"] = torch.rand(1, R, S).numpy()[0]
    arrs["noise"] = (torch.randn(R, S) * raw_noise_std).numpy()
    for dtype in (("float32",) if config2 else ("float32", "float64")):
        render = rh.build_reference(canon, faces, state, S, dtype=dtype)
        render.cfg.MODEL.raw_noise_std = raw_noise_std
        render.cfg.MODEL.LOSSwMask = True
        loss_fn = make_loss(render.cfg)
        tdt = getattr(torch, dtype)
        batch = rh.make_batch(rays, xyz, poses, TH, FRAME, dtype=dtype, sel=sel)
        batch["rgb"] = torch.from_numpy(target).to(tdt)[None]
        batch["occupancy"] = torch.from_numpy(occ).to(tdt)[None]
        fwd, out = grads_of(render, batch, seed, loss_fn, dtype)
        sfx = "" if dtype == "float32" else "_f64"
        for k, v in fwd.items():
            arrs["render:" + k + sfx] = v
        for k, v in out.items():
            arrs[k + sfx] = v
    path = os.path.join(HERE, name + ".npz")
    if config2:
        keep = ("S", "frame", "Th", "raw_noise_std", "seed", "render:color", "render:acc_map", "render:depth_map")
        arrs = {k: v for k, v in arrs.items() if k in keep or k.split(":")[0] in ("loss", "norm", "sum", "grad")}
        arrs["rays"] = np.int64(R)
        arrs["z_vals_sum"] = np.float64(fwd["z_vals"].astype(np.float64).sum())
        np.savez_compressed(path, **arrs)
        print(f"{name}: {os.path.getsize(path) / 1024:.0f} KiB; loss {arrs['loss']:.6f}")
        return
    if compact:
        # (the S > 64 cases: what cannot be regenerated - z_vals, the per-ray outputs, the loss terms, the norms / sums and the
        #  float32 run's stored gradients.  Of the float64 run's gradients only what the tests use is kept: per tensor, the relative
        #  L2 distance of the float32 run's stored elements from it ("spread:").  Body, rays, targets and draws are functions of the
        #  seeds: tests/test_gpu_train.py rebuilds them and checks the draws against the sums kept here)
        for k in [k for k in arrs if k.startswith("grad:") and not k.endswith("_f64")]:
            a, b = arrs[k].astype(np.float64), arrs[k + "_f64"].astype(np.float64)
            arrs["spread:" + k[5:]] = np.float64(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))
        arrs["jitter_sum"] = np.float64(arrs["jitter"].astype(np.float64).sum())
        arrs["noise_sum"] = np.float64(arrs["noise"].astype(np.float64).sum())
        keep = ("S", "frame", "Th", "raw_noise_std", "seed", "jitter_sum", "noise_sum", "render:z_vals", "render:color",
                "render:acc_map", "render:depth_map")
        arrs = {k: v for k, v in arrs.items() if k in keep or k.startswith(("loss", "norm:", "sum:", "spread:"))
                or (k.startswith("grad:") and not k.endswith("_f64"))}
        arrs["rays"] = np.int64(R)
    np.savez_compressed(path, **arrs)
    print(f"{name}: {os.path.getsize(path) / 1024:.0f} KiB; loss {arrs['loss']:.6f} (f64 {arrs['loss_f64']:.6f})")
    for k in ("nerf.stage1.0.weight", "nerf.stage2.4.weight", "lighting_mlp.lights_encoding.0.weight", "pose_mlp.0.weight",
              "nerf.embedding.weight", "nerf.density_net.0.weight"):
        print(f"   |grad {k}| = {arrs['norm:' + k]:.6e}  (f64 {arrs['norm:' + k + '_f64']:.6e})")


def main():
    import torch
    torch.set_num_threads(8)
    if "--config2" in sys.argv:                  # BASELINE configs[2] at its own size: 8192 rays x 64 samples of the 512 x 512 view
        tag = ([a for a in sys.argv[sys.argv.index("--config2") + 1:] if not a.startswith("-")] or ["default"])[0]
        if tag == "default":
            state = synth.make_state_dict()
        else:
            z = np.load(os.path.join(HERE, f"weights_{tag}.npz"))
            state = {k[2:]: z[k] for k in z.files if k.startswith("w:")}
        poses = synth.make_poses()
        canon, faces = synth.make_body()
        xyz = synth.pose_body(canon)
        rays = synth.make_rays(512, 512, xyz, fit_box=True)
        sel = np.linspace(0, 512 * 512 - 1, 8192).astype(np.int64)
        case("full_train_grads_8192" + ("" if tag == "default" else "_" + tag), canon, faces, xyz, poses, rays, sel, 64, state,
             raw_noise_std=1.0, config2=True)
        return
    if "--nonuniform" in sys.argv:               # the SMPL-like body (synth.make_body(nonuniform=True)): dense caps at head / hands / feet
        state = synth.make_state_dict()
        poses = synth.make_poses()
        canon, faces = synth.make_body(nonuniform=True)
        xyz = synth.pose_body(canon)
        rays = synth.make_rays(32, 32, xyz, fit_box=True)
        case("full_train_grads_nu", canon, faces, xyz, poses, rays, np.arange(0, 1024, 8), 64, state, raw_noise_std=1.0)
        return
    if "--other-weights" in sys.argv:            # the trained parameter sets: w2 (make_weights_w2.py, default) or `--other-weights w4`
        rest = [a for a in sys.argv[sys.argv.index("--other-weights") + 1:] if not a.startswith("-")]
        tag = rest[0] if rest else "w2"
        z = np.load(os.path.join(HERE, f"weights_{tag}.npz"))
        state = {k[2:]: z[k] for k in z.files if k.startswith("w:")}
        poses = synth.make_poses()
        canon_s, faces_s = synth.make_small_body()
        xyz_s = synth.pose_body(canon_s)
        rays_s = synth.make_rays(8, 8, xyz_s, cam_dist=2.2, focal_frac=2.0)
        case("small_train_grads_" + tag, canon_s, faces_s, xyz_s, poses, rays_s, np.arange(64), 16, state, raw_noise_std=1.0)
        canon, faces = synth.make_body()
        xyz = synth.pose_body(canon)
        rays = synth.make_rays(32, 32, xyz, fit_box=True)
        case("full_train_grads_" + tag, canon, faces, xyz, poses, rays, np.arange(0, 1024, 8), 64, state, raw_noise_std=1.0)
        return
    if "--samples" in sys.argv:                  # the full case at another S: `--samples 128` or `--samples 200 [w4]` (see below)
        rest = [a for a in sys.argv[sys.argv.index("--samples") + 1:] if not a.startswith("-")]
        S = int(rest[0])
        tag = rest[1] if len(rest) > 1 else "default"
        if tag == "default":
            state = synth.make_state_dict()
        else:
            z = np.load(os.path.join(HERE, f"weights_{tag}.npz"))
            state = {k[2:]: z[k] for k in z.files if k.startswith("w:")}
        poses = synth.make_poses()
        canon, faces = synth.make_body()
        xyz = synth.pose_body(canon)
        rays = synth.make_rays(32, 32, xyz, fit_box=True)
        # the same 128 rays as full_train_grads at every S: S = 128 is the training adjoint's two-chunk wave form
        # (65 <= S <= 128), S = 200 its one-thread-per-ray form (S > 128); both runs, float32 and float64, fit the container.
        # Stored compact (see case()): about 0.3 - 0.4 MB each
        case("full_train_grads" + ("" if tag == "default" else "_" + tag) + f"_s{S}", canon, faces, xyz, poses, rays,
             np.arange(0, 1024, 8), S, state, raw_noise_std=1.0, compact=True)
        return
    state = synth.make_state_dict()
    poses = synth.make_poses()
    canon_s, faces_s = synth.make_small_body()
    xyz_s = synth.pose_body(canon_s)
    rays_s = synth.make_rays(8, 8, xyz_s, cam_dist=2.2, focal_frac=2.0)
    case("small_train_grads", canon_s, faces_s, xyz_s, poses, rays_s, np.arange(64), 16, state, raw_noise_std=1.0)
    case("small_train_grads_nonoise", canon_s, faces_s, xyz_s, poses, rays_s, np.arange(64), 16, state, raw_noise_std=0.0)
    canon, faces = synth.make_body()
    xyz = synth.pose_body(canon)
    rays = synth.make_rays(32, 32, xyz, fit_box=True)
    sel = np.arange(0, 1024, 8)                 # 128 rays spread over the frame
    case("full_train_grads", canon, faces, xyz, poses, rays, sel, 64, state, raw_noise_std=1.0)


if __name__ == "__main__":
    main()
