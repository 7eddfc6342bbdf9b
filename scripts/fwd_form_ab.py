#!/usr/bin/env python
"""render_fwd_kernel's two forms (hn_render_fwd_form: ring, resident) on the
bench workload, which gives hn_render_fwd's dispatch rule.

    python scripts/fwd_form_ab.py --config 2 --n-rand 1024 2048 4096 8192 [--runs 2] [--out FILE]
    python scripts/fwd_form_ab.py --config 2 3 5 --arms parent auto --parent DIR --runs 4 --steps 200
    python scripts/fwd_form_ab.py --bench FORM -- <bench.py arguments>

Each (config, N_rand, arm) is a fresh `bench.py --full --no-cpu-baseline`
process (the trained regime: 1000 untimed steps first), the arms alternating:
a form of this tree (functional.FWD_FORM set: ring, resident, auto) or the
parent commit's own checkout and library.  The figures are bench.py's:
ms_per_step and the HIP-event launch times of --kernel-steps further steps.
--bench runs bench.py itself in this process under one form (e.g. under a
profiler).
"""
import argparse
import json
import math
import os
import runpy
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "r12", "fwd_form_ab.json")
FORMS = ("ring", "resident")


def bench_under(form, argv):
    import hn_loader
    hn_loader.load().functional.FWD_FORM = form
    sys.argv = [os.path.join(ROOT, "bench.py")] + argv
    runpy.run_path(sys.argv[0], run_name="__main__")


def stats(v):
    return dict(n=len(v), mean_ms=round(statistics.fmean(v), 5), std_ms=round(statistics.pstdev(v), 5), runs=v)


def compare(a, b):
    """b against a: whether the difference exceeds twice the pooled std."""
    pooled = math.sqrt((a["std_ms"] ** 2 + b["std_ms"] ** 2) / 2)
    diff = b["mean_ms"] - a["mean_ms"]
    return dict(ratio=round(b["mean_ms"] / a["mean_ms"], 4), diff_ms=round(diff, 5), pooled_std_ms=round(pooled, 5),
                counts=abs(diff) > 2 * pooled)


def run_arm(arm, parent, bench_args):
    """One fresh bench.py process: under a form of this tree, or ("parent") the
    plain bench.py of a checkout of the parent commit with its library built."""
    if arm == "parent":
        cmd, cwd = [sys.executable, os.path.join(parent, "bench.py")] + bench_args, parent
    else:
        cmd, cwd = [sys.executable, os.path.abspath(__file__), "--bench", arm, "--"] + bench_args, ROOT
    p = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=400)
    if p.returncode:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit(f"fwd_form_ab.py: bench.py failed in arm {arm} (exit {p.returncode})")
    return json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])


def main():
    if "--bench" in sys.argv[1:2]:
        return bench_under(sys.argv[2], sys.argv[4:] if sys.argv[3:4] == ["--"] else sys.argv[3:])
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, nargs="+", default=[2])
    ap.add_argument("--n-rand", type=int, nargs="+", default=[0], help="0: the config's own")
    ap.add_argument("--arms", nargs="+", default=list(FORMS), choices=FORMS + ("auto", "parent"),
                    help="the first arm is the one the others are compared against")
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit, built (the parent arm)")
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--kernel-steps", type=int, default=50)
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    if ("parent" in args.arms) != bool(args.parent):
        ap.error("the parent arm and --parent DIR go together")
    keys = ("ms_per_step", "render_fwd_ms", "render_bwd_ms")
    cases = {}
    for config in args.config:
        for n in args.n_rand:
            runs = {a: {k: [] for k in keys} for a in args.arms}
            for _ in range(args.runs):
                for arm in args.arms:
                    line = run_arm(arm, args.parent, ["--gpus", "1", "--config", str(config)] +
                                   (["--n-rand", str(n)] if n else []) +
                                   ["--steps", str(args.steps), "--warmup", "10", "--full", "--no-cpu-baseline",
                                    "--kernel-steps", str(args.kernel_steps)])
                    got = dict(line["kernels"], ms_per_step=line["ms_per_step"])
                    for k in keys:
                        runs[arm][k].append(got[k])
                    print(config, n, arm, *[got[k] for k in keys], flush=True)
            r = {a: {k: stats(v) for k, v in runs[a].items()} for a in args.arms}
            for a in args.arms[1:]:
                r[f"{a}_vs_{args.arms[0]}"] = {k: compare(r[args.arms[0]][k], r[a][k]) for k in keys}
            cases[f"config{config}" + (f"_n{n}" if n else "")] = r
    res = {"what": "bench.py --gpus 1 --full --no-cpu-baseline per case and arm, fresh processes, the arms "
                   "alternating; render_fwd_ms / render_bwd_ms: HIP events over --kernel-steps steps after the "
                   "timed region",
           "rule": "a difference counts only beyond twice the pooled std of the two arms (compare())",
           "arms": args.arms, "steps": args.steps, "kernel_steps": args.kernel_steps, "runs_per_arm": args.runs,
           "cases": cases}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({c: {k: v for k, v in r.items() if "_vs_" in k} for c, r in cases.items()}))


if __name__ == "__main__":
    main()
