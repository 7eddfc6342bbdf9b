#!/usr/bin/env python
"""A/B of the evaluation renderer at bench.py's config 2: render_path through
the chunked training forward (image_kernel=False, chunk 32768) against
render_path through the whole-image kernel (image_kernel=True), and the image
kernel's two design alternatives (hn_render_image_variant).

    python scripts/render_image_ab.py [--pretrain 1000] [--rounds 10] [--sizes 800 400] [--out FILE]

Trains --pretrain steps on the procedural chair, then renders the 8 held-out
test poses at each size.  render_path: both arms in this one process,
alternating, after a warm-up of each at that size, timed with a host clock
around a call that ends in a device synchronise (the call includes the copies
of the frames to the host, as a user's does).  The kernel's design points
(coarse-twin slot reuse against re-encoding, tiled against row-major ray
order): the 8 views in one launch into preallocated outputs, alternating the
variants launch by launch, HIP events around the launch alone.  Writes one JSON
file: mean, standard deviation and rays/s per arm, each arm's PSNR against the
scene's test images, whether a difference exceeds twice the pooled standard
deviation, and the kernel's line of the compiler's resource report.
"""
import argparse
import json
import math
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(ms, rays):
    m = statistics.fmean(ms)
    return dict(n=len(ms), mean_ms=round(m, 4), std_ms=round(statistics.pstdev(ms), 4), min_ms=round(min(ms), 4),
                median_ms=round(statistics.median(ms), 4), max_ms=round(max(ms), 4), rays_per_s=round(rays / (m * 1e-3)))


def compare(a, b):
    """b against a: the ratio of means, and whether the difference counts
    (it exceeds twice the pooled standard deviation of the two arms)."""
    pooled = math.sqrt((a["std_ms"] ** 2 + b["std_ms"] ** 2) / 2)
    diff = b["mean_ms"] - a["mean_ms"]
    return dict(ratio=round(b["mean_ms"] / a["mean_ms"], 4), diff_ms=round(diff, 4), pooled_std_ms=round(pooled, 4),
                counts=abs(diff) > 2 * pooled)


def resource_report(path):
    """render_image_kernel's lines of -Rpass-analysis=kernel-resource-usage:
    from `path` (the report's text) or from a device-only compile here."""
    if path:
        text = open(path).read()
    else:
        from importlib import util
        spec = util.spec_from_file_location("_hn_build", os.path.join(ROOT, "hashnerf-pytorch_amd", "build.py"))
        b = util.module_from_spec(spec)
        spec.loader.exec_module(b)
        with tempfile.TemporaryDirectory() as d:
            r = subprocess.run([b.HIPCC, *b.CFLAGS, "-Rpass-analysis=kernel-resource-usage", "--offload-device-only",
                                "-S", os.path.join(b.CSRC, "hn_render.hip"), "-o", os.path.join(d, "hn_render.s")],
                               capture_output=True, text=True, check=True)
        text = r.stderr
    out, on = {}, False
    for line in text.split("\n"):
        m = re.search(r"remark:\s+(.*?): (\S+) \[-Rpass-analysis", line)
        if not m:
            continue
        key, val = m.group(1).strip(), m.group(2).strip()
        if key == "Function Name":
            on = "render_image_kernel" in val
        elif on:
            out[key] = val
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pretrain", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=10, help="timed alternations per size (>= 5)")
    ap.add_argument("--sizes", type=int, nargs="+", default=[800, 400])
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--kernel-launches", type=int, default=10, help="timed launches per variant and size")
    ap.add_argument("--resource", default=None, help="text of the compiler's resource report (default: compile here)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10", "render_image_ab.json"))
    args = ap.parse_args()
    if args.rounds < 5:
        raise SystemExit("render_image_ab.py: at least 5 alternations")

    import bench
    import hn_loader
    hn = hn_loader.load()
    from hashnerf_pytorch_amd import functional as HF
    from hashnerf_pytorch_amd.rays import blender_intrinsics
    from hashnerf_pytorch_amd.train import SyntheticBlender, Trainer, default_args, render_procedural

    cfg2 = dict(bench.CONFIGS[2])
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    targs = default_args(N_rand=cfg2["N_rand"], log2_hashmap_size=cfg2["log2_hashmap_size"],
                         finest_res=cfg2["finest_res"], tv_loss_weight=cfg2["tv_loss_weight"],
                         tv_until=cfg2.get("tv_until", 1001), white_bkgd=cfg2.get("white_bkgd", True),
                         sparse_loss_weight=cfg2.get("sparse_loss_weight", 1e-10),
                         no_batching=cfg2.get("no_batching", True))
    data = SyntheticBlender(400, 400, 100, dev, seed=0, scene="procedural", n_test=args.views)
    if "bbox" in cfg2:
        data.bounding_box = tuple(torch.tensor(v) for v in cfg2["bbox"])
    tr = Trainer(targs, data, dev, seed=0)
    loss = None
    for _ in range(args.pretrain):
        loss, _ = tr.step()
    torch.cuda.synchronize()
    HF.L.check_device_faults()

    kw = dict(tr.kw_test, near=2., far=6.)
    poses = data.test_poses
    emb = kw["network_query_fn"].embed_fn
    rcfg = HF.make_render_cfg(emb.grid(), bool(kw.get("white_bkgd", False)), bool(kw.get("lindisp", False)), False)
    ws = kw["network_fn"].weights() + kw["network_fine"].weights()
    wsb = torch.empty(HF.L.lib().hn_render_image_workspace_bytes(rcfg), dtype=torch.uint8, device=dev)
    variants = {"shipped": 0, "reencode": HF.L.IMAGE_VARIANTS["reencode"], "row_major": HF.L.IMAGE_VARIANTS["row_major"]}

    def psnr(rgbs, gt):
        return [round(float(-10. * np.log10(np.mean(np.square(rgbs[i] - gt[i])))), 4) for i in range(len(gt))]

    sizes = {}
    for S in args.sizes:
        focal, K = blender_intrinsics(S, S)
        gt = data.test_images if S == data.H else torch.stack([render_procedural(S, S, K, c) for c in poses], 0)
        gt = gt.cpu().numpy()
        rays = len(poses) * S * S

        def path(image_kernel):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rgbs, _ = hn.render_path(poses, (S, S, focal), K, 32768, kw, image_kernel=image_kernel)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, rgbs

        arms = {False: [], True: []}
        frames = {}
        for ik in (False, True):                 # this size warm in both arms
            _, frames[ik] = path(ik)
        for _ in range(args.rounds):
            for ik in (False, True):
                arms[ik].append(path(ik)[0])
        a, b = stats(arms[False], rays), stats(arms[True], rays)

        # the kernel alone: the 8 views in one launch, the variants alternating
        out = (torch.empty((len(poses), S, S, 3), device=dev), torch.empty((len(poses), S, S), device=dev),
               torch.empty((len(poses), S, S), device=dev))
        pose34 = poses[:, :3, :4].contiguous()
        ev = {k: [] for k in variants}
        sums = {}
        for c in range(-2, args.kernel_launches):    # 2 untimed launches of every variant first
            for name, v in variants.items():
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                HF.render_image(rcfg, S, S, K, pose34, 2., 6., emb.table, ws, wsb=wsb, weights_packed=c > -2,
                                variant=v, out=out)
                e.record()
                if c >= 0:
                    ev[name].append((s, e))
                elif c == -1:
                    sums[name] = float(out[0].double().sum())
        torch.cuda.synchronize()
        kern = {k: stats([s.elapsed_time(e) for s, e in v], rays) for k, v in ev.items()}
        sizes[str(S)] = {
            "rays": rays,
            "render_path_chunked": a, "render_path_image_kernel": b,
            "image_kernel_vs_chunked": compare(a, b),
            "psnr_chunked": psnr(frames[False], gt), "psnr_image_kernel": psnr(frames[True], gt),
            "max_abs_rgb_diff_between_arms": float(np.abs(frames[False] - frames[True]).max()),
            "kernel": kern,
            "reencode_vs_shipped": compare(kern["shipped"], kern["reencode"]),
            "row_major_vs_shipped": compare(kern["shipped"], kern["row_major"]),
            "kernel_rgb_sums": sums,
        }

    props = torch.cuda.get_device_properties(dev)
    res = {
        "what": "evaluation renderer A/B: render_path chunked vs whole-image kernel (host clock, ends in a "
                "synchronise), and the kernel's design alternatives (HIP events around the launch)",
        "device": props.name, "torch": torch.__version__, "hip": torch.version.hip,
        "settings": {"config": 2, "workload": cfg2["workload"],
                     "dataset": f"SyntheticBlender(400, 400, 100), procedural, {args.views} test poses",
                     "pretrain_steps": args.pretrain, "loss_after_pretrain": None if loss is None else float(loss),
                     "chunk": 32768, "rounds": args.rounds, "kernel_launches": args.kernel_launches,
                     "alternation": "chunked then image kernel, round by round; variants launch by launch; one process",
                     "bar": "a difference counts if it exceeds twice the pooled std of the two arms"},
        "sizes": sizes,
        "render_image_kernel_resources": resource_report(args.resource),
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    keys = ("render_path_chunked", "render_path_image_kernel", "image_kernel_vs_chunked", "reencode_vs_shipped",
            "row_major_vs_shipped", "psnr_chunked", "psnr_image_kernel")
    print(json.dumps({S: {k: sizes[S][k] for k in keys} for S in sizes}))


if __name__ == "__main__":
    main()
