#!/usr/bin/env python
"""A/B of one training step at 64 + 64 samples (N_samples = 64, N_importance =
64: the LLFF configurations' counts), T = 19, raw_noise_std = 1, at N_rand
1024 (the LLFF configs' value) and 4096.

    python scripts/ni64_ab.py [--steps 200] [--warmup 20] [--n-rand 1024 4096] [--out FILE]
    python scripts/ni64_ab.py --trace-only [--steps 30]          # under rocprofv3 --kernel-trace --stats
    python scripts/ni64_ab.py --merge-kernel-stats DIR [--out FILE]

* new:        the fused path, Trainer(mode="explicit") with all its fusions.
* reference:  what the library did for this configuration before it had the
              64 form -- the unfused composition through the module API
              (render + training_loss + backward + RAdam.step), forced here by
              a plain-lambda network_query_fn (Trainer(mode="autograd")).

Both arms live in this one process and alternate step by step after a warm-up
of each; a step is timed with a host clock between two device synchronises.
The scene is the procedural blender one (there is no LLFF loader): the rays
are not NDC rays, the sample counts, the noise and the table size are the LLFF
configurations'.  Reports mean +- std per arm and whether the difference
exceeds twice the pooled std.  --trace-only runs the fused arm alone, for a
separate rocprofv3 --kernel-trace --stats run, whose render_fwd_kernel rows
--merge-kernel-stats then adds to the JSON.
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
OUT = os.path.join(ROOT, "profiles", "r11", "ni64_ab.json")
T = 19


def stats(ms):
    return dict(n=len(ms), mean_ms=round(statistics.fmean(ms), 4), std_ms=round(statistics.pstdev(ms), 4),
                min_ms=round(min(ms), 4), median_ms=round(statistics.median(ms), 4), max_ms=round(max(ms), 4))


def compare(a, b):
    """b against a: ratio of means, and whether the difference exceeds twice the pooled std."""
    pooled = math.sqrt((a["std_ms"] ** 2 + b["std_ms"] ** 2) / 2)
    diff = b["mean_ms"] - a["mean_ms"]
    return dict(ratio=round(b["mean_ms"] / a["mean_ms"], 4), diff_ms=round(diff, 4), pooled_std_ms=round(pooled, 4),
                counts=abs(diff) > 2 * pooled)


def trainers(hn, n_rand, dev, fused_only=False):
    from hashnerf_pytorch_amd.train import SyntheticBlender, Trainer, default_args
    data = SyntheticBlender(400, 400, 100, dev, seed=0, scene="procedural")
    mk = lambda: default_args(N_rand=n_rand, N_importance=64, log2_hashmap_size=T, raw_noise_std=1.0,
                              sparse_loss_weight=1e-10, tv_loss_weight=1e-6)
    new = Trainer(mk(), data, dev, seed=0, mode="explicit")
    if fused_only:
        return new, None
    ref = Trainer(mk(), data, dev, seed=0, mode="autograd")
    emb, sh = ref.embed_fn, ref.kw_train["network_query_fn"].embeddirs_fn
    ref.kw_train["network_query_fn"] = lambda i, v, f: hn.run_network(i, v, f, emb, sh)   # not a NetworkQuery: unfused
    return new, ref


def timed(tr):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tr.step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def merge_kernel_stats(d, out):
    rows = {}
    for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if "render_fwd_kernel" in r.get("Name", ""):
                rows[r["Name"].split("(")[0].replace("void ", "")] = dict(
                    calls=int(r["Calls"]), average_us=round(float(r["AverageNs"]) / 1e3, 2),
                    min_us=round(float(r["MinNs"]) / 1e3, 2), max_us=round(float(r["MaxNs"]) / 1e3, 2))
    if not rows:
        raise SystemExit(f"ni64_ab.py: no render_fwd_kernel row under {d}")
    res = json.load(open(out))
    res["render_fwd_kernel_trace"] = dict(
        how="rocprofv3 --kernel-trace --stats on --trace-only (the fused arm alone, every step of every N_rand, "
            "warm-up included)", kernels=rows)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res["render_fwd_kernel_trace"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--n-rand", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--merge-kernel-stats", metavar="DIR", default=None)
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    if args.merge_kernel_stats:
        return merge_kernel_stats(args.merge_kernel_stats, args.out)

    import hn_loader
    hn = hn_loader.load()
    from hashnerf_pytorch_amd import functional as HF
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    sizes = {}
    for n_rand in args.n_rand:
        new, ref = trainers(hn, n_rand, dev, fused_only=args.trace_only)
        if args.trace_only:
            for _ in range(args.steps):
                new.step()
            torch.cuda.synchronize()
            HF.L.check_device_faults()
            continue
        for _ in range(args.warmup):
            timed(new)
            timed(ref)
        a, b = [], []
        for _ in range(args.steps):
            b.append(timed(ref))
            a.append(timed(new))
        HF.L.check_device_faults()
        assert new._cfg.n_importance == 64 and new._binned
        sa, sb = stats(a), stats(b)
        sizes[str(n_rand)] = dict(fused_explicit=sa, unfused_module_api=sb, fused_vs_unfused=compare(sb, sa),
                                  faster=bool(sb["mean_ms"] - sa["mean_ms"] > 2 * compare(sb, sa)["pooled_std_ms"]))
        del new, ref
        torch.cuda.empty_cache()
    if args.trace_only:
        return
    props = torch.cuda.get_device_properties(dev)
    res = {
        "what": "one training step at 64 + 64 samples: the fused path (Trainer explicit mode) against the unfused "
                "module-API composition the library ran for this configuration before the 64 form",
        "device": props.name, "torch": torch.__version__, "hip": torch.version.hip,
        "settings": {"N_samples": 64, "N_importance": 64, "log2_hashmap_size": T, "raw_noise_std": 1.0,
                     "dataset": "SyntheticBlender(400, 400, 100), procedural (blender rays, not NDC)",
                     "steps": args.steps, "warmup": args.warmup,
                     "alternation": "unfused then fused, step by step; one process; host clock between synchronises",
                     "bar": "faster = the difference exceeds twice the pooled std of the two arms"},
        "n_rand": sizes,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(sizes))


if __name__ == "__main__":
    main()
