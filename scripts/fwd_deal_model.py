#!/usr/bin/env python
"""Cost model of the resident forward's deal of ray runs to CUs, on the CPU.

    python scripts/fwd_deal_model.py [--views 8] [--rays 4096] [--size 400] [--threshold 1e-2]

The resident form of render_fwd_kernel gives a CU 16 rays (4 runs of 4) and the
launch ends with the slowest CU.  A ray's cost is a fixed part (the gathers,
the sigma nets on its 8 tiles) plus the colour net on its tiles with density:
cost = 490 + 36.4 * live_tiles K cycles, and with the texture path
the kernel's bound a CU's time is about the sum of its rays' costs.  What the
launch loses to imbalance is then 1 - mean / max of the CUs' sums.

Per view: --rays distinct pixels of a --size^2 image of train.procedural_field
(the true field standing in for the trained one) in Morton order, as the
sampler hands them out; a tile of 32 samples is live where one of its
densities exceeds --threshold; a ray's key is whether its target differs from
the white background by more than 1/512 in some channel.  The maps of the new
rule are hn_render_fwd_deal's, the function the kernel calls (the library
must be built; no GPU is used).  Prints mean / max per dealing."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FIXED, PER_TILE = 490.0, 36.4


def morton(x, y):
    def spread(v):
        v = v.astype(np.uint64)
        out = np.zeros_like(v)
        for b in range(16):
            out |= ((v >> np.uint64(b)) & np.uint64(1)) << np.uint64(2 * b)
        return out
    return spread(x) | (spread(y) << np.uint64(1))


def sample_pdf(bins, w, n):
    """Inverse-CDF samples at n evenly spaced u (run_nerf_helpers.sample_pdf, det=True)."""
    w = w + 1e-5
    cdf = torch.cumsum(w / w.sum(-1, keepdim=True), -1)
    cdf = torch.cat([torch.zeros_like(cdf[:, :1]), cdf], -1)
    u = torch.linspace(0., 1., n).expand(cdf.shape[0], n).contiguous()
    inds = torch.searchsorted(cdf, u, right=True)
    below, above = (inds - 1).clamp(min=0), inds.clamp(max=cdf.shape[-1] - 1)
    c0, c1 = cdf.gather(1, below), cdf.gather(1, above)
    b0, b1 = bins.gather(1, below), bins.gather(1, above)
    den = torch.where(c1 - c0 < 1e-5, torch.ones_like(c0), c1 - c0)
    return b0 + (u - c0) / den * (b1 - b0)


@torch.no_grad()
def view_batch(hn, pose, size, n_rays, rng, threshold):
    """(live tiles [n_rays] 0..8, key bit [n_rays]) of one view's batch in Morton order."""
    from hashnerf_pytorch_amd import train as T
    _, K = hn.rays.blender_intrinsics(size, size)
    ro, rd = hn.get_rays(size, size, K, pose[:3, :4])
    pix = rng.choice(size * size, n_rays, replace=False)
    pix = pix[np.argsort(morton(pix % size, pix // size), kind="stable")]
    o, d = ro.reshape(-1, 3)[pix], rd.reshape(-1, 3)[pix]
    dn = d.norm(dim=-1, keepdim=True)

    def field(z):
        return T.procedural_field(o[:, None] + d[:, None] * z[..., None])

    def weights(sigma, z):
        dist = torch.cat([z[:, 1:] - z[:, :-1], torch.full_like(z[:, :1], 1e10)], -1) * dn
        alpha = 1. - torch.exp(-sigma * dist)
        trans = torch.cumprod(torch.cat([torch.ones_like(alpha[:, :1]), 1. - alpha + 1e-10], -1), -1)[:, :-1]
        return alpha * trans

    zc = torch.linspace(2., 6., 64).expand(n_rays, 64)
    sc, _ = field(zc)
    wc = weights(sc, zc)
    zi = sample_pdf(.5 * (zc[:, 1:] + zc[:, :-1]), wc[:, 1:-1], 128)
    zf = torch.sort(torch.cat([zc, zi], -1), -1).values
    sf, cf = field(zf)
    wf = weights(sf, zf)
    target = (wf[..., None] * cf).sum(1) + (1. - wf.sum(-1, keepdim=True))
    live = (torch.cat([sc, sf], -1).reshape(n_rays, 8, 32) > threshold).any(-1).sum(-1)
    key = ((target - 1.).abs() > 1. / 512).any(-1)
    return live.numpy(), key.numpy()


def band_map(nb):
    b, s = np.meshgrid(np.arange(nb), np.arange(4), indexing="ij")
    return 4 * ((b % 8) * (nb // 8 * 4) + s * (nb // 8) + b // 8)


def dealt(hn, n_rays, nb, keys):
    out = np.empty(4 * nb, np.int32)
    k = None if keys is None else np.ascontiguousarray(keys, np.uint8)
    st = hn._lib.lib().hn_render_fwd_deal(n_rays, nb, None if k is None else k.ctypes.data, out.ctypes.data)
    assert st == 0, st
    return out.reshape(nb, 4)


def balance(cost, first):
    """mean / max of the workgroups' cost sums; first [nb, 4]: their runs' first rays."""
    run_cost = cost.reshape(-1, 4).sum(1)
    per = run_cost[first // 4].sum(1)
    return per.mean() / per.max()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--size", type=int, default=400)
    ap.add_argument("--threshold", type=float, default=1e-2)
    args = ap.parse_args()
    import hn_loader
    hn = hn_loader.load()
    nb = (args.rays + 15) // 16
    assert args.rays == 16 * nb and nb % 32 == 0, "whole workgroups, whole segments per XCD"
    poses = hn.rays.blender_cameras(100)
    rng = np.random.default_rng(0)
    names = ("16 consecutive rays", "4 runs of 4, XCD band", "segments interleaved", "segments + keys", "key = live tiles")
    rows = []
    for v in range(args.views):
        live, key = view_batch(hn, poses[(v * len(poses)) // args.views], args.size, args.rays, rng, args.threshold)
        cost = FIXED + PER_TILE * live
        run_key = key.reshape(-1, 4).sum(1)
        # (an upper bound for any key: the runs sorted by their modelled cost itself, in 5 levels)
        rc = cost.reshape(-1, 4).sum(1)
        ideal = np.round(4 * (rc - rc.min()) / max(rc.max() - rc.min(), 1e-9))
        maps = (4 * np.arange(4 * nb).reshape(nb, 4), band_map(nb), dealt(hn, args.rays, nb, None),
                dealt(hn, args.rays, nb, run_key), dealt(hn, args.rays, nb, ideal))
        rows.append([balance(cost, m) for m in maps])
        agree = np.mean((live > 2) == key)   # (the 2 coarse tiles of a ray that grazes the object count as empty space)
        print(f"view {v}: rays with density {np.mean(live > 0):.2f}, key agrees with fine density {agree:.3f}, "
              f"cost/fixed mean {cost[live > 0].mean() / FIXED:.2f} max {cost.max() / FIXED:.2f} | " +
              "  ".join(f"{x:.3f}" for x in rows[-1]))
    rows = np.array(rows)
    print("\nmean / max of the CUs' modelled time (mean over the views; min .. max)")
    for i, n in enumerate(names):
        print(f"  {n:24s} {rows[:, i].mean():.3f}  ({rows[:, i].min():.3f} .. {rows[:, i].max():.3f})")


if __name__ == "__main__":
    main()
