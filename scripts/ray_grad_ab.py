#!/usr/bin/env python
"""A/B of one pose-refinement step on a frozen field: the fused ray gradient
(render(..., ray_grad="fused"): the fused forward with its state kept, then
hn_render_bwd_rays) against the unfused composition of the standalone ops that
rays with grad take by default.  1,024 and 4,096 rays of a 400 x 400 blender
camera, 64 + 128 samples, T = 19 (the blender box, finest 512, a seeded uniform
table), white background, no raw noise, MSE on rgb_map + rgb0.

    python scripts/ray_grad_ab.py [--steps 200] [--warmup 20] [--rays 1024 4096] [--out FILE]
    python scripts/ray_grad_ab.py --trace-only [--steps 30]   # under rocprofv3 --kernel-trace --stats --output-format csv
    python scripts/ray_grad_ab.py --merge-kernel-stats DIR [--out FILE]

A step: get_rays(pose) on the device, the selected pixels' rays, render(...),
the loss, backward(); the pose is an nn.Parameter, the table and both nets have
requires_grad False.  Both arms live in one process and alternate step by step
after a warm-up of each; a step is timed with a host clock between two device
synchronises.  Reports mean, std and median per arm and whether the difference
exceeds twice the pooled std (the yardstick is the unfused arm of the same
run).  --trace-only runs the fused arm alone at each ray count, for a
rocprofv3 --kernel-trace --stats run; --merge-kernel-stats adds that run's rows
of the kernels hn_render_bwd_rays launches to the JSON.
"""
import argparse
import csv
import glob
import json
import math
import os
import re
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "r16", "ray_grad_ab.json")
T = 19
MLP_KW = dict(num_layers=2, hidden_dim=64, geo_feat_dim=15, num_layers_color=3, hidden_dim_color=64,
              input_ch=32, input_ch_views=16)
BOX = (torch.tensor([-4.0, -4.0, -3.4]), torch.tensor([4.0, 4.0, 3.3]))
KERNELS = ("render_bwd_rays_kernel", "render_bwd_rays_reduce_kernel", "render_comp_bwd_kernel", "render_fwd_kernel",
           "mlp_pack2_kernel")


def stats(ms):
    return dict(n=len(ms), mean_ms=round(statistics.fmean(ms), 4), std_ms=round(statistics.pstdev(ms), 4),
                min_ms=round(min(ms), 4), median_ms=round(statistics.median(ms), 4), max_ms=round(max(ms), 4))


def compare(a, b):
    """b against a: ratio of means, and whether the difference exceeds twice the pooled std."""
    pooled = math.sqrt((a["std_ms"] ** 2 + b["std_ms"] ** 2) / 2)
    diff = b["mean_ms"] - a["mean_ms"]
    return dict(ratio=round(b["mean_ms"] / a["mean_ms"], 4), diff_ms=round(diff, 4), pooled_std_ms=round(pooled, 4),
                counts=abs(diff) > 2 * pooled)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def field(hn, dev):
    torch.manual_seed(1)
    emb = hn.HashEmbedder(BOX, log2_hashmap_size=T, finest_resolution=512).to(dev)
    with torch.no_grad():
        emb.table.uniform_(-0.5, 0.5)
    mc, mf = hn.NeRFSmall(**MLP_KW).to(dev), hn.NeRFSmall(**MLP_KW).to(dev)
    for m in (emb, mc, mf):
        m.requires_grad_(False)
    return emb, mc, mf


def pose_step(hn, fld, n_rays, dev, ray_grad):
    """-> (step(), pose): one pose-gradient step of n_rays rays; ray_grad None (unfused) or "fused"."""
    emb, mc, mf = fld
    nq = hn.NetworkQuery(emb, hn.SHEncoder())
    _, K = hn.rays.blender_intrinsics(400, 400)
    pose = torch.nn.Parameter(hn.pose_spherical(30.0, -30.0, 4.0)[:3, :4].to(dev))
    g = torch.Generator(device=dev).manual_seed(2)
    sel = torch.randperm(400 * 400, device=dev, generator=g)[:n_rays]
    target = torch.rand(n_rays, 3, device=dev, generator=g)

    def step():
        pose.grad = None
        o, d = hn.get_rays(400, 400, K, pose)
        rays = (o.reshape(-1, 3)[sel], d.reshape(-1, 3)[sel])
        rgb, _, _, ex = hn.render(400, 400, K, rays=rays, use_viewdirs=True, ndc=False, near=2., far=6.,
                                  network_query_fn=nq, network_fn=mc, network_fine=mf, N_samples=64, N_importance=128,
                                  perturb=0., white_bkgd=True, raw_noise_std=0., ray_grad=ray_grad)
        loss, _ = hn.training_loss(rgb, ex, target, 0.)
        loss.backward()
    return step, pose


def merge_kernel_stats(d, out):
    res = json.load(open(out))
    rows = {}
    for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            for k in KERNELS:
                name = r.get("Name", "")
                if re.search(r"(?<![A-Za-z0-9_])" + k + r"(?![A-Za-z0-9_])", name) or f"{len(k)}{k}E" in name:
                    e = rows.setdefault(k, dict(calls=0, total_us=0.0, min_us=float("inf"), max_us=0.0))
                    e["calls"] += int(r["Calls"])
                    e["total_us"] += float(r["AverageNs"]) * int(r["Calls"]) / 1e3
                    e["min_us"] = min(e["min_us"], float(r["MinNs"]) / 1e3)
                    e["max_us"] = max(e["max_us"], float(r["MaxNs"]) / 1e3)
    if "render_bwd_rays_kernel" not in rows:
        raise SystemExit(f"ray_grad_ab.py: no render_bwd_rays_kernel row under {d}")
    for e in rows.values():
        e["average_us"] = round(e.pop("total_us") / e["calls"], 2)
        e["min_us"], e["max_us"] = round(e["min_us"], 2), round(e["max_us"], 2)
    res["kernel_trace"] = dict(
        how="rocprofv3 --kernel-trace --stats on --trace-only, a run of its own: the fused arm at each ray count, "
            "every step, warm-up included, the ray counts pooled (min: the smaller, max: the larger)", kernels=rows)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res["kernel_trace"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rays", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--merge-kernel-stats", metavar="DIR", default=None)
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    if args.merge_kernel_stats:
        return merge_kernel_stats(args.merge_kernel_stats, args.out)
    if not torch.cuda.is_available():
        raise SystemExit("ray_grad_ab.py: needs the GPU (no fall-back)")

    import hn_loader
    hn = hn_loader.load()
    from hashnerf_pytorch_amd import functional as HF
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    fld = field(hn, dev)
    if args.trace_only:
        for n in args.rays:
            step, pose = pose_step(hn, fld, n, dev, "fused")
            for _ in range(args.steps):
                step()
            torch.cuda.synchronize()
            HF.L.check_device_faults()
            assert bool(torch.isfinite(pose.grad).all())
        return
    sizes = {}
    for n in args.rays:
        (fused, pf), (unfused, pu) = pose_step(hn, fld, n, dev, "fused"), pose_step(hn, fld, n, dev, None)
        for _ in range(args.warmup):
            timed(unfused)
            timed(fused)
        a, b = [], []
        for _ in range(args.steps):
            b.append(timed(unfused))
            a.append(timed(fused))
        HF.L.check_device_faults()
        assert all(p.grad is None for p in (fld[0].table, *fld[1].weights(), *fld[2].weights()))
        assert bool(torch.isfinite(pf.grad).all()) and float(pf.grad.abs().max()) > 0
        rel = float((pf.grad - pu.grad).norm() / pu.grad.norm())
        sa, sb = stats(a), stats(b)
        c = compare(sb, sa)
        sizes[str(n)] = dict(fused=sa, unfused=sb, fused_vs_unfused=c,
                             faster=bool(sb["mean_ms"] - sa["mean_ms"] > 2 * c["pooled_std_ms"]),
                             pose_grad_rel_diff=rel)
    props = torch.cuda.get_device_properties(dev)
    res = {
        "what": "one pose-gradient step on a frozen field: render(..., ray_grad=\"fused\") against the unfused "
                "composition (the default for rays with grad)",
        "device": props.name, "torch": torch.__version__, "hip": torch.version.hip,
        "settings": {"N_samples": 64, "N_importance": 128, "log2_hashmap_size": T, "raw_noise_std": 0.0,
                     "near_far": [2., 6.], "camera": "400 x 400 blender, pose_spherical(30, -30, 4)",
                     "field": "blender box, finest 512, uniform table, untrained nets; requires_grad False",
                     "steps": args.steps, "warmup": args.warmup,
                     "alternation": "unfused then fused, step by step; one process; host clock between synchronises",
                     "bar": "faster = the difference exceeds twice the pooled std of the two arms"},
        "rays": sizes,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(sizes))


if __name__ == "__main__":
    main()
