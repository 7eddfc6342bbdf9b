#!/usr/bin/env python
"""Timing of the input gradients (informational, no threshold).

    python scripts/input_grad_timing.py [--reps 30] [--warmup 5] [--out FILE]

(a) hn_encode_bwd_input against hn_encode_fwd at 262,144 points, L = 16,
    T = 19 (the blender box, finest 512, a seeded uniform table, points drawn
    uniformly in the box): the two launches alternate call by call after a
    warm-up of each, every call between two HIP events on the launch stream.
(b) One pose-gradient step at 1,024 rays, 64 + 128: the pose an nn.Parameter,
    the field frozen, the rays of 1,024 pixels of a 400 x 400 blender camera
    from get_rays(pose), render(...), the MSE on rgb_map + rgb0 and
    backward(); events around the whole step, which ends before the
    synchronise that reads them.

Writes one JSON file: median, mean, standard deviation, min and max in ms per
arm."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MLP_KW = dict(num_layers=2, hidden_dim=64, geo_feat_dim=15, num_layers_color=3, hidden_dim_color=64,
              input_ch=32, input_ch_views=16)
BOX = (torch.tensor([-4.0, -4.0, -3.4]), torch.tensor([4.0, 4.0, 3.3]))


def stats(ms):
    a = np.asarray(ms, np.float64)
    return {"n": int(a.size), "median_ms": float(np.median(a)), "mean_ms": float(a.mean()), "std_ms": float(a.std()),
            "min_ms": float(a.min()), "max_ms": float(a.max())}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def encode_arms(hn, n, reps, warmup):
    L = hn._lib
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    emb = hn.HashEmbedder(BOX, log2_hashmap_size=19, finest_resolution=512).to(dev)
    with torch.no_grad():
        emb.table.uniform_(-0.5, 0.5)
    table = emb.table.detach()
    x = (BOX[0] + (BOX[1] - BOX[0]) * torch.rand(n, 3)).to(dev)
    dfeat = torch.randn(n, 32, device=dev)
    feat = torch.empty(n, 32, device=dev)
    keep = torch.empty(n, dtype=torch.uint8, device=dev)
    dx = torch.empty(n, 3, device=dev)
    g, lib, st = emb.grid(), L.lib(), L.stream(dev)
    fwd = lambda: L.check(lib.hn_encode_fwd(g, L.ptr(x), n, L.ptr(table), L.ptr(feat), L.ptr(keep), st), "encode_fwd")
    bwd = lambda: L.check(lib.hn_encode_bwd_input(g, L.ptr(x), n, L.ptr(table), L.ptr(dfeat), L.ptr(dx), st),
                          "encode_bwd_input")
    for _ in range(warmup):
        fwd()
        bwd()
    torch.cuda.synchronize()
    t = {"encode_fwd": [], "encode_bwd_input": []}
    for _ in range(reps):
        t["encode_fwd"].append(timed(fwd))
        t["encode_bwd_input"].append(timed(bwd))
    out = {k: stats(v) for k, v in t.items()}
    out["points"], out["levels"], out["log2_hashmap_size"] = n, 16, 19
    # bytes the algorithm needs: 8 rows of 8 B per (point, level) gathered, the point and the features / gradient rows
    out["gather_bytes"] = n * 16 * 8 * 8
    return out


def pose_step(hn, n_rays, reps, warmup):
    dev = torch.device("cuda:0")
    torch.manual_seed(1)
    emb = hn.HashEmbedder(BOX, log2_hashmap_size=19, finest_resolution=512).to(dev)
    with torch.no_grad():
        emb.table.uniform_(-0.5, 0.5)
    mc, mf = hn.NeRFSmall(**MLP_KW).to(dev), hn.NeRFSmall(**MLP_KW).to(dev)
    for m in (emb, mc, mf):
        m.requires_grad_(False)
    nq = hn.NetworkQuery(emb, hn.SHEncoder())
    _, K = hn.rays.blender_intrinsics(400, 400)
    pose = torch.nn.Parameter(hn.pose_spherical(30.0, -30.0, 4.0)[:3, :4].to(dev))
    sel = torch.randperm(400 * 400, device=dev)[:n_rays]
    target = torch.rand(n_rays, 3, device=dev)

    def step():
        pose.grad = None
        o, d = hn.get_rays(400, 400, K, pose)
        rays = (o.reshape(-1, 3)[sel], d.reshape(-1, 3)[sel])
        rgb, _, _, ex = hn.render(400, 400, K, rays=rays, use_viewdirs=True, ndc=False, near=2., far=6.,
                                  network_query_fn=nq, network_fn=mc, network_fine=mf, N_samples=64, N_importance=128,
                                  perturb=0., white_bkgd=True, raw_noise_std=0.)
        loss, _ = hn.training_loss(rgb, ex, target, 0.)
        loss.backward()
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    out = stats([timed(step) for _ in range(reps)])
    assert pose.grad is not None and bool(torch.isfinite(pose.grad).all()) and emb.table.grad is None
    out["rays"], out["samples"], out["log2_hashmap_size"] = n_rays, "64 + 128", 19
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14", "input_grad.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("input_grad_timing: needs the GPU (no fall-back)")
    import hn_loader
    hn = hn_loader.load()
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup,
           "encode": encode_arms(hn, 262144, a.reps, a.warmup), "pose_step": pose_step(hn, 1024, a.reps, a.warmup)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
