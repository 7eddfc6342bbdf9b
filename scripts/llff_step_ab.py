#!/usr/bin/env python
"""A/B of one training step of the LLFF configuration (dataset_type llff: NDC
rays, near 0, far 1, 64 + 64 samples, raw_noise_std 1, no precrop), T = 19, on
SyntheticLLFF(378, 504, 20), at N_rand 1024 (the LLFF configs' value) and 4096,
for both no_batching settings (the reference's default pool, and per-image
draws).

    python scripts/llff_step_ab.py [--steps 200] [--warmup 20] [--n-rand 1024 4096] [--out FILE]
    python scripts/llff_step_ab.py --trace-only ndc|world [--steps 60]   # under rocprofv3 --kernel-trace --stats
    python scripts/llff_step_ab.py --merge-kernel-stats ndc=DIR world=DIR [--out FILE]

* device:  Trainer.step() self-driven: the samplers hand out the final NDC rays
           (hn_ray_ndc), the uniforms come from the sampler's launch and, with
           per-image draws, the next batch from the backward's small launches.
* torch:   the route a caller had before the samplers knew NDC: the same draw
           as world rays, rays.get_ndc_rays on them (about fifteen small torch
           launches), a repacked [B, 11] batch, step(i, batch).

Both arms live in one process and alternate step by step after a warm-up of
each; a step is timed with a host clock between two device synchronises.
Reports mean +- std per arm and whether the difference exceeds twice the pooled
std.  --trace-only runs 'ndc' (the device arm with per-image draws: an NDC next
batch inside the backward) or 'world' (the same trainer drawing world rays: the
next-batch job as it was) alone, for a rocprofv3 --kernel-trace --stats run each;
--merge-kernel-stats adds their render_lists_kernel / ovf_place_kernel rows.
"""
import argparse
import csv
import glob
import json
import math
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "r15", "llff_step_ab.json")
T = 19
DATA = (378, 504, 20)
KERNELS = ("render_lists_kernel", "ovf_place_kernel")


def stats(ms):
    return dict(n=len(ms), mean_ms=round(statistics.fmean(ms), 4), std_ms=round(statistics.pstdev(ms), 4),
                min_ms=round(min(ms), 4), median_ms=round(statistics.median(ms), 4), max_ms=round(max(ms), 4))


def compare(a, b):
    """b against a: ratio of means, and whether the difference exceeds twice the pooled std."""
    pooled = math.sqrt((a["std_ms"] ** 2 + b["std_ms"] ** 2) / 2)
    diff = b["mean_ms"] - a["mean_ms"]
    return dict(ratio=round(b["mean_ms"] / a["mean_ms"], 4), diff_ms=round(diff, 4), pooled_std_ms=round(pooled, 4),
                counts=abs(diff) > 2 * pooled)


def trainer(data, n_rand, no_batching, dev, world_rays=False):
    from hashnerf_pytorch_amd.train import Trainer, default_args
    args = default_args(dataset_type="llff", N_importance=64, raw_noise_std=1., white_bkgd=False,
                        no_batching=no_batching, precrop_iters=0, N_rand=n_rand, log2_hashmap_size=T)
    tr = Trainer(args, data, dev, seed=0, mode="explicit")
    if world_rays:
        tr.ndc = None    # its samplers make the calls they made before they knew NDC
    return tr


def torch_route_step(hn, tr):
    """World rays from the sampler, render()'s NDC step by torch, a repacked batch."""
    d = tr.data
    i = tr.global_step + 1
    b = tr.draw_batch(i)
    r = b["rays"]
    o, dd = hn.get_ndc_rays(d.H, d.W, d.K[0][0], 1., r[:, 0:3], r[:, 3:6])
    b["rays"] = torch.cat([o, dd, r[:, 6:11]], -1)
    return tr.step(i, b)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def merge_kernel_stats(pairs, out):
    res = json.load(open(out))
    trace = {}
    for pair in pairs:
        arm, d = pair.split("=", 1)
        rows = {}
        for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for r in csv.DictReader(open(f)):
                for k in KERNELS:
                    if k in r.get("Name", ""):
                        rows[k] = dict(calls=int(r["Calls"]), average_us=round(float(r["AverageNs"]) / 1e3, 2),
                                       min_us=round(float(r["MinNs"]) / 1e3, 2),
                                       max_us=round(float(r["MaxNs"]) / 1e3, 2))
        if not rows:
            raise SystemExit(f"llff_step_ab.py: no {' / '.join(KERNELS)} row under {d}")
        trace[arm] = rows
    res["next_batch_kernel_trace"] = dict(
        how="rocprofv3 --kernel-trace --stats on --trace-only ndc / world, a run each (per-image draws, N_rand 1024, "
            "every step, warm-up included): the two launches that carry the next batch's job, with an NDC job and "
            "with a world-ray job", arms=trace)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res["next_batch_kernel_trace"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--n-rand", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--trace-only", choices=["ndc", "world"], default=None)
    ap.add_argument("--merge-kernel-stats", metavar="ARM=DIR", nargs="+", default=None)
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    if args.merge_kernel_stats:
        return merge_kernel_stats(args.merge_kernel_stats, args.out)

    import hn_loader
    hn = hn_loader.load()
    from hashnerf_pytorch_amd import functional as HF
    from hashnerf_pytorch_amd.train import SyntheticLLFF
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    data = SyntheticLLFF(*DATA, dev, seed=0)
    if args.trace_only:
        tr = trainer(data, 1024, True, dev, world_rays=args.trace_only == "world")
        for _ in range(args.steps):
            tr.step()
        torch.cuda.synchronize()
        HF.L.check_device_faults()
        assert tr._fuses_next_batch()
        return
    sizes = {}
    for n_rand in args.n_rand:
        for no_batching in (False, True):
            dev_tr = trainer(data, n_rand, no_batching, dev)
            torch_tr = trainer(data, n_rand, no_batching, dev, world_rays=True)
            step_a = dev_tr.step
            step_b = lambda: torch_route_step(hn, torch_tr)
            for _ in range(args.warmup):
                timed(step_a)
                timed(step_b)
            a, b = [], []
            for _ in range(args.steps):
                b.append(timed(step_b))
                a.append(timed(step_a))
            HF.L.check_device_faults()
            assert dev_tr._cfg.n_importance == 64 and dev_tr._binned
            assert dev_tr._fuses_next_batch() == no_batching
            sa, sb = stats(a), stats(b)
            c = compare(sb, sa)
            sizes[f"{n_rand}/{'per_image' if no_batching else 'pool'}"] = dict(
                device_sampler_ndc=sa, torch_ndc_route=sb, device_vs_torch=c,
                faster=bool(sb["mean_ms"] - sa["mean_ms"] > 2 * c["pooled_std_ms"]))
            del dev_tr, torch_tr
            torch.cuda.empty_cache()
    props = torch.cuda.get_device_properties(dev)
    res = {
        "what": "one training step of the LLFF configuration: NDC rays from the device samplers (Trainer.step() "
                "self-driven) against world rays + torch get_ndc_rays + repack + step(i, batch)",
        "device": props.name, "torch": torch.__version__, "hip": torch.version.hip,
        "settings": {"N_samples": 64, "N_importance": 64, "log2_hashmap_size": T, "raw_noise_std": 1.0,
                     "near_far": [0., 1.], "dataset": "SyntheticLLFF(378, 504, 20), uniform targets, untrained field",
                     "steps": args.steps, "warmup": args.warmup,
                     "alternation": "torch route then device, step by step; one process; host clock between "
                                    "synchronises",
                     "bar": "faster = the difference exceeds twice the pooled std of the two arms"},
        "n_rand/draw": sizes,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(sizes))


if __name__ == "__main__":
    main()
