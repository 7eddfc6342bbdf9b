#!/usr/bin/env python
"""A/B of the use_batching pool draw's two orders at bench.py's config 5:
the shuffle's order (hn_sample_pool) against Morton order of the rays'
mid-depth points (hn_sample_pool_ordered), on the same pool positions.

    python scripts/pool_order_ab.py [--pretrain 1000] [--batches 16] [--rounds 13] [--out FILE]

Trains --pretrain steps with pool_order=0, then, with the trained weights
untouched, draws a fixed list of batches in both orders and times the
inference forward (feat NULL) on them with HIP events around the launch alone,
alternating the two orders batch by batch in this one process after warming
both up; and times the sampler launch alone in both forms.  A sampler launch
is shorter than the host's own work between the two event records, so each
timed sampler call is queued behind a filler kernel that keeps the device busy
meanwhile; the same pair of events around nothing gives the floor to subtract.
Writes one JSON file with every setting and both sets of times (mean, standard
deviation, min, median, max in milliseconds).
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(ms):
    return dict(n=len(ms), mean_ms=round(statistics.fmean(ms), 5), std_ms=round(statistics.pstdev(ms), 5),
                min_ms=round(min(ms), 5), median_ms=round(statistics.median(ms), 5), max_ms=round(max(ms), 5))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pretrain", type=int, default=1000)
    ap.add_argument("--batches", type=int, default=16, help="pool batches in the fixed list (>= 16)")
    ap.add_argument("--rounds", type=int, default=13, help="timed passes over the list (batches x rounds >= 200)")
    ap.add_argument("--warmup", type=int, default=2, help="untimed passes over the list, both orders")
    ap.add_argument("--sampler-calls", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09", "pool_order_ab.json"))
    args = ap.parse_args()
    if args.batches < 16 or args.batches * args.rounds < 200:
        raise SystemExit("pool_order_ab.py: at least 16 batches and 200 timed forwards per order")

    import bench
    import hn_loader
    hn_loader.load()
    from hashnerf_pytorch_amd import functional as HF
    from hashnerf_pytorch_amd.render import _linspace_cached
    from hashnerf_pytorch_amd.train import SyntheticBlender, Trainer, _step_seed, default_args

    cfg5 = dict(bench.CONFIGS[5])
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    targs = default_args(N_rand=cfg5["N_rand"], log2_hashmap_size=cfg5["log2_hashmap_size"],
                         finest_res=cfg5["finest_res"], tv_loss_weight=cfg5["tv_loss_weight"],
                         white_bkgd=cfg5["white_bkgd"], sparse_loss_weight=cfg5["sparse_loss_weight"],
                         no_batching=cfg5["no_batching"])
    data = SyntheticBlender(400, 400, 100, dev, seed=0)
    data.bounding_box = tuple(torch.tensor(v) for v in cfg5["bbox"])
    tr = Trainer(targs, data, dev, seed=0, pool_order=0)
    loss = None
    for _ in range(args.pretrain):
        loss, _ = tr.step()
    torch.cuda.synchronize()
    HF.L.check_device_faults()

    # the fixed batches: positions [b B, (b + 1) B) of one epoch's shuffle, in both orders
    B = targs.N_rand
    g = tr.embed_fn.grid()
    box = (list(g.box_min), list(g.box_max))
    ids = tr._pool_ids
    seed = _step_seed(0, 0, -1)
    pool = (data.images, data.poses, ids, data.K, 2., 6., seed)
    batches = {0: [], 1: []}
    distinct = []
    for b in range(args.batches):
        r0, _ = HF.sample_pool(*pool, b * B, B)
        r1, _, k1 = HF.sample_pool(*pool, b * B, B, order=1, box=box, return_keys=True)
        batches[0].append(r0)
        batches[1].append(r1)
        distinct.append(int(torch.unique(k1).numel()))

    # the inference forward, as render_rays makes it without perturb
    kw = tr.kw_test
    rcfg = HF.make_render_cfg(g, bool(kw.get("white_bkgd", False)), bool(kw.get("lindisp", False)), False)
    t_vals = _linspace_cached(64, dev)
    u = torch.linspace(0., 1., 128, device=dev).expand(B, 128).contiguous()
    ws = kw["network_fn"].weights() + kw["network_fine"].weights()
    table = tr.embed_fn.table
    wsb = torch.empty(HF.L.lib().hn_render_workspace_bytes(rcfg, B), dtype=torch.uint8, device=dev)

    def forward(rays):
        with torch.no_grad():
            out, _ = HF.render_fwd(rcfg, rays, t_vals, None, u, None, None, table, ws, False, wsb=wsb)
        return out

    check = {}
    for o in (0, 1):       # both shapes warm, and the outputs' sums agree between the orders
        for _ in range(args.warmup):
            for r in batches[o]:
                out = forward(r)
        check[o] = float(forward(batches[o][0])["rgb"].double().sum())
    torch.cuda.synchronize()
    HF.TIMER.reset()
    HF.TIMER.names, HF.TIMER.every, HF.TIMER.enabled = {"render_fwd"}, 1, True
    order_of_call = []
    for _ in range(args.rounds):
        for b in range(args.batches):
            for o in (0, 1):
                forward(batches[o][b])
                order_of_call.append(o)
    torch.cuda.synchronize()
    HF.TIMER.enabled = False
    ev = HF.TIMER.events["render_fwd"]
    fwd = {o: [s.elapsed_time(e) for (s, e), oc in zip(ev, order_of_call) if oc == o] for o in (0, 1)}
    HF.TIMER.reset()

    # the sampler launch alone: draw order; ordered; ordered with the step's two uniform draws
    # in the launch; and the draw order's own pair of launches (hn_sample_pool + hn_uniform_philox)
    filler = torch.empty(1 << 28, dtype=torch.float32, device=dev)      # 1 GiB: its fill outlasts the host's calls
    uni = [(B, 64), (B, 128)]
    forms = {
        "floor_event_pair": lambda b: None,
        "order0": lambda b: HF.sample_pool(*pool, b * B, B),
        "order1": lambda b: HF.sample_pool(*pool, b * B, B, order=1, box=box),
        "order0_with_uniforms": lambda b: HF.sample_pool(*pool, b * B, B, uniforms=uni),
        "order1_with_uniforms": lambda b: HF.sample_pool(*pool, b * B, B, order=1, box=box, uniforms=uni),
    }
    samp = {k: [] for k in forms}
    for c in range(-8, args.sampler_calls):                               # 8 untimed calls of every form first
        for name, fn in forms.items():
            filler.zero_()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn(c % args.batches)
            e.record()
            if c >= 0:
                samp[name].append((s, e))
    torch.cuda.synchronize()
    samp = {k: [s.elapsed_time(e) for s, e in v] for k, v in samp.items()}

    props = torch.cuda.get_device_properties(dev)
    res = {
        "what": "pool batch order A/B: inference forward (feat NULL) and sampler launch, HIP events",
        "device": props.name, "torch": torch.__version__, "hip": torch.version.hip,
        "settings": {"config": 5, "workload": cfg5["workload"], "dataset": "SyntheticBlender(400, 400, 100), uniform",
                     "bbox": cfg5["bbox"], "N_rand": B, "log2_hashmap_size": cfg5["log2_hashmap_size"],
                     "finest_res": cfg5["finest_res"], "white_bkgd": cfg5["white_bkgd"],
                     "sparse_loss_weight": cfg5["sparse_loss_weight"], "tv_loss_weight": cfg5["tv_loss_weight"],
                     "no_batching": cfg5["no_batching"], "near": 2., "far": 6., "pretrain_steps": args.pretrain,
                     "pretrain_pool_order": 0, "loss_after_pretrain": None if loss is None else float(loss),
                     "batches": args.batches, "rounds": args.rounds, "warmup_passes": args.warmup,
                     "sampler_calls": args.sampler_calls, "pool_seed": seed,
                     "alternation": "order 0 then order 1 on each batch, batch by batch, one process"},
        "distinct_keys_per_batch": distinct,
        "rgb_sum_batch0": check,
        "forward": {"order0": stats(fwd[0]), "order1": stats(fwd[1]),
                    "order1_over_order0_mean": round(statistics.fmean(fwd[1]) / statistics.fmean(fwd[0]), 4)},
        "sampler": {k: stats(v) for k, v in samp.items()},
        "sampler_method": "each timed call queued behind a 1 GiB fill; floor_event_pair is the same pair of "
                          "events around no launch (subtract it)",
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({"forward": res["forward"], "sampler": res["sampler"]}))


if __name__ == "__main__":
    main()
