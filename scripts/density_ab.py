#!/usr/bin/env python
"""A/B of the density queries: density_grid (one density_kernel launch, the
lattice's points formed in the kernel) against the module composition a user
had to write before it -- HashEmbedder over a chunk of points, a dummy SH block
concatenated, NeRFSmall, column 3 kept -- chunked at 2^18 points.

    python scripts/density_ab.py [--pretrain 1000] [--rounds 20] [--variant LABEL=LIB ...] [--out FILE]

Field: the procedural chair at T = 19 after --pretrain steps of the bench's
trainer (N_rand 4096), its fine net.  Sizes: 128^3 and 256^3 with sigma; 512^3
with occupancy only (the composition there writes sigma and compares it to the
threshold).  Both arms live in this one process and
alternate call by call after a warm-up of each size; a call is timed with HIP
events on the stream it runs on.  The composition's points are made before the
clock starts (lattice_coords, on the device) and its buffers are allocated
once: only its launches are timed.  At every size the arms' outputs are
compared bit for bit.  A difference counts when it exceeds twice the pooled
standard deviation of the two arms.

--variant LABEL=LIB: other builds of the library (another workgroup shape or
tile order of density_kernel).  Each is timed in a process of its own
(HN_LIB_PATH) on the saved field, the shipped build among them, in
--variant-passes passes that alternate the builds process by process.
"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CHUNK = 1 << 18
MLP = dict(num_layers=2, hidden_dim=64, geo_feat_dim=15, num_layers_color=3, hidden_dim_color=64, input_ch=32,
           input_ch_views=16)


def stats(ms, points):
    m = statistics.fmean(ms)
    return dict(n=len(ms), mean_ms=round(m, 4), std_ms=round(statistics.pstdev(ms), 4), min_ms=round(min(ms), 4),
                median_ms=round(statistics.median(ms), 4), max_ms=round(max(ms), 4),
                points_per_s=round(points / (m * 1e-3)))


def compare(a, b):
    """b against a: the ratio of means, and whether the difference counts."""
    pooled = math.sqrt((a["std_ms"] ** 2 + b["std_ms"] ** 2) / 2)
    diff = b["mean_ms"] - a["mean_ms"]
    return dict(ratio=round(b["mean_ms"] / a["mean_ms"], 4), speedup=round(a["mean_ms"] / b["mean_ms"], 2),
                diff_ms=round(diff, 4), pooled_std_ms=round(pooled, 4), counts=abs(diff) > 2 * pooled)


def timed(fn):
    """fn()'s time on the current stream in ms (HIP events) and its result."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def kernel_arm(hn, net, nq, n, occ_only):
    if occ_only:
        return lambda: hn.density_grid(n, net, nq, threshold=0.0, want_sigma=False)
    return lambda: hn.density_grid(n, net, nq)


def composition_arm(hn, net, nq, n, occ_only):
    """The route through the module API, chunked: sigma [n^3] (and, occ_only,
    its comparison with the threshold: the bool array a user would keep)."""
    from hashnerf_pytorch_amd import functional as HF
    from hashnerf_pytorch_amd.render import cell_centre_lattice
    emb = nq.embed_fn
    dev = emb.table.device
    lo, step, dims = cell_centre_lattice(n, *emb.box())
    pts = HF.lattice_coords(lo, step, dims, device=dev).reshape(-1, 3)
    sh = torch.zeros((CHUNK, 16), device=dev)
    sigma = torch.empty((pts.shape[0],), device=dev)

    @torch.no_grad()
    def run():
        for i in range(0, pts.shape[0], CHUNK):
            p = pts[i:i + CHUNK]
            feat, _ = emb(p)
            sigma[i:i + p.shape[0]] = net(torch.cat([feat, sh[:p.shape[0]]], -1))[:, 3]
        return sigma > 0.0 if occ_only else sigma
    return run


def ab(hn, net, nq, n, occ_only, rounds):
    arms = {"composition": composition_arm(hn, net, nq, n, occ_only), "density_grid": kernel_arm(hn, net, nq, n, occ_only)}
    outs = {k: f() for k, f in arms.items()}          # this size warm in both arms
    torch.cuda.synchronize()
    if occ_only:
        same = torch.equal(hn.unpack_occupancy(outs["density_grid"], (n, n, n)).reshape(-1), outs["composition"])
    else:
        same = torch.equal(outs["density_grid"].reshape(-1).view(torch.int32), outs["composition"].view(torch.int32))
    live = float((outs["composition"] > 0.0).float().mean()) if not occ_only else float(outs["composition"].float().mean())
    del outs
    ms = {k: [] for k in arms}
    for _ in range(rounds):
        for k, f in arms.items():
            ms[k].append(timed(f)[0])
    a, b = stats(ms["composition"], n ** 3), stats(ms["density_grid"], n ** 3)
    return {"points": n ** 3, "output": "occupancy words only" if occ_only else "sigma", "composition": a,
            "density_grid": b, "density_grid_vs_composition": compare(a, b), "outputs_bitwise_equal": bool(same),
            "share_of_points_with_sigma_above_0": round(live, 4)}


def load_field(hn, path, dev):
    f = torch.load(path, map_location=dev)
    emb = hn.HashEmbedder((f["bmin"].cpu(), f["bmax"].cpu()), log2_hashmap_size=f["T"],
                          finest_resolution=f["finest"]).to(dev)
    net = hn.NeRFSmall(**MLP).to(dev)
    with torch.no_grad():
        emb.table.copy_(f["table"])
        for w, v in zip(net.weights(), f["ws"]):
            w.copy_(v)
    return net, hn.NetworkQuery(emb, hn.SHEncoder())


def child(args):
    """One build's density_grid times on the saved field (a process of its own)."""
    import hn_loader
    hn = hn_loader.load()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    net, nq = load_field(hn, args.field, dev)
    out = {}
    for n, occ_only in ((128, False), (256, False), (512, True)):
        f = kernel_arm(hn, net, nq, n, occ_only)
        f()
        torch.cuda.synchronize()
        out[str(n)] = [timed(f)[0] for _ in range(args.rounds)]
    print("CHILD_JSON " + json.dumps(out))


def variants(args, field_path):
    libs = [("shipped", None)] + [tuple(v.split("=", 1)) for v in args.variant]
    ms = {label: {} for label, _ in libs}
    for _ in range(args.variant_passes):
        for label, lib in libs:
            env = dict(os.environ)
            if lib is not None:
                env["HN_LIB_PATH"] = os.path.abspath(lib)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--field", field_path, "--rounds",
                                str(args.rounds)], env=env, capture_output=True, text=True, timeout=300, check=True)
            line = [l for l in r.stdout.splitlines() if l.startswith("CHILD_JSON ")][-1]
            for n, v in json.loads(line[len("CHILD_JSON "):]).items():
                ms[label].setdefault(n, []).extend(v)
    res = {label: {n: stats(v, int(n) ** 3) for n, v in by_n.items()} for label, by_n in ms.items()}
    for label in res:
        if label != "shipped":
            for n in res[label]:
                res[label][n]["vs_shipped"] = compare(res["shipped"][n], res[label][n])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pretrain", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=20, help="timed alternations per size (>= 20)")
    ap.add_argument("--variant", action="append", default=[], metavar="LABEL=LIB")
    ap.add_argument("--variant-passes", type=int, default=2)
    ap.add_argument("--variant-notes", default=None, help="JSON object label -> what the build changes")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--field", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22", "density_ab.json"))
    args = ap.parse_args()
    if args.child:
        return child(args)
    if args.rounds < 20:
        raise SystemExit("density_ab.py: at least 20 alternations")

    import hn_loader
    hn = hn_loader.load()
    from hashnerf_pytorch_amd import functional as HF
    from hashnerf_pytorch_amd.train import SyntheticBlender, Trainer, default_args

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    T = 19
    data = SyntheticBlender(400, 400, 100, dev, seed=0, scene="procedural")
    tr = Trainer(default_args(N_rand=4096, log2_hashmap_size=T), data, dev, seed=0)
    loss = None
    for _ in range(args.pretrain):
        loss, _ = tr.step()
    torch.cuda.synchronize()
    HF.L.check_device_faults()
    net, nq = tr.kw_test["network_fine"], tr.kw_test["network_query_fn"]
    emb = nq.embed_fn

    sizes = {}
    for n, occ_only in ((128, False), (256, False), (512, True)):
        sizes[f"{n}^3"] = ab(hn, net, nq, n, occ_only, args.rounds)
        print(n, json.dumps(sizes[f"{n}^3"]), flush=True)
    var = None
    if args.variant:
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "field.pt")
            bmin, bmax = emb.box()
            torch.save({"bmin": bmin, "bmax": bmax, "T": T, "finest": int(emb.finest_resolution),
                        "table": emb.table.detach(), "ws": [w.detach() for w in net.weights()]}, path)
            var = variants(args, path)
        print("variants", json.dumps(var), flush=True)

    props = torch.cuda.get_device_properties(dev)
    doc = {"what": "density queries A/B: density_grid (density_kernel) vs the module composition (HashEmbedder, dummy "
                   "SH block, NeRFSmall, column 3) chunked at 2^18 points; HIP events around each call",
           "device": props.name, "torch": torch.__version__, "hip": torch.version.hip,
           "settings": {"log2_hashmap_size": T, "field": f"procedural chair after {args.pretrain} steps of the bench's "
                        "trainer (N_rand 4096), fine net", "loss_after_pretrain": None if loss is None else float(loss),
                        "lattice": "cell centres of the embedder's bounding box", "chunk": CHUNK,
                        "rounds": args.rounds,
                        "alternation": "composition then density_grid, call by call; one process",
                        "composition_not_timed": "its points (lattice_coords on the device) and buffers are made "
                                                 "before the clock starts",
                        "bar": "a difference counts if it exceeds twice the pooled std of the two arms"},
           "sizes": sizes}
    if var is not None:
        doc["kernel_variants"] = {"how": f"density_grid alone, each build in processes of its own on the saved field, "
                                         f"{args.variant_passes} passes alternating the builds, {args.rounds} timed calls "
                                         "per size and process after a warm-up call",
                                  "notes": json.loads(args.variant_notes) if args.variant_notes else None,
                                  "times": var}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
