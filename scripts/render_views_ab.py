#!/usr/bin/env python
"""A/B of the evaluation renderer at 64 + 64 samples (the LLFF configurations'
counts): render_path through the chunked training forward (image_kernel=False,
chunk 32768) against render_path through the whole-image kernel
(image_kernel=True, hn_render_views).

    python scripts/render_views_ab.py [--pretrain 1000] [--rounds 10] [--only a b] [--out FILE]

(a) world rays: the procedural chair after --pretrain steps of
    Trainer(mode="explicit") at N_importance = 64 (a trained field's
    sparsity), T = 19, the 8 held-out test poses at 400 x 400.
(b) NDC rays at fern's evaluation shape: 8 views of 504 x 378 from seeded
    near-identity forward-facing poses, near 0, far 1, the box
    bbox_for_llff's, T = 19, a seeded random table and random nets (there is
    no LLFF loader or data here).  This field's density is NOT a trained
    scene's, so the share of tiles whose colour net is skipped is not
    representative; the arms still do the same work on the same field.

Both arms live in this one process and alternate call by call after a warm-up
of each; a call is timed with a host clock and ends in a device synchronise (it
includes the copies of the frames to the host, as a user's does).  A difference
counts when it exceeds twice the pooled standard deviation of the two arms.
Writes one JSON file: mean, standard deviation and rays/s per arm, the PSNR of
arm against arm (and, for (a), of each arm against the scene's test images).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from render_image_ab import compare, stats   # noqa: E402


def llff_poses(n, seed):
    """Near-identity forward-facing poses (cameras looking down -z, as LLFF's recentred ones)."""
    g = np.random.Generator(np.random.PCG64(seed))
    poses = np.zeros((n, 3, 4), dtype=np.float32)
    for p in poses:
        a = g.normal(0., 0.08, 3)
        rx = np.array([[1, 0, 0], [0, np.cos(a[0]), -np.sin(a[0])], [0, np.sin(a[0]), np.cos(a[0])]])
        ry = np.array([[np.cos(a[1]), 0, np.sin(a[1])], [0, 1, 0], [-np.sin(a[1]), 0, np.cos(a[1])]])
        rz = np.array([[np.cos(a[2]), -np.sin(a[2]), 0], [np.sin(a[2]), np.cos(a[2]), 0], [0, 0, 1]])
        p[:, :3] = (rz @ ry @ rx).astype(np.float32)
        p[:, 3] = g.normal(0., 0.15, 3).astype(np.float32)
    return poses


def psnr(a, b):
    return [round(float(-10. * np.log10(max(np.mean(np.square(a[i] - b[i])), 1e-20))), 4) for i in range(len(a))]


def ab(hn, poses, H, W, focal, K, kw, rounds):
    """The two render_path arms on one field: statistics, frames of each arm."""
    from hashnerf_pytorch_amd.render import _views_ineligible
    assert _views_ineligible(kw) is None
    rays = len(poses) * H * W

    def path(image_kernel):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rgbs, _ = hn.render_path(poses, (H, W, focal), K, 32768, kw, image_kernel=image_kernel)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, rgbs

    arms, frames = {False: [], True: []}, {}
    for ik in (False, True):                 # this shape warm in both arms
        _, frames[ik] = path(ik)
    for _ in range(rounds):
        for ik in (False, True):
            arms[ik].append(path(ik)[0])
    a, b = stats(arms[False], rays), stats(arms[True], rays)
    res = {"rays": rays, "render_path_chunked": a, "render_path_image_kernel": b,
           "image_kernel_vs_chunked": compare(a, b),
           "psnr_image_kernel_against_chunked": psnr(frames[True], frames[False]),
           "max_abs_rgb_diff_between_arms": float(np.abs(frames[False] - frames[True]).max())}
    return res, frames


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pretrain", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=10, help="timed alternations per workload (>= 5)")
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--only", nargs="+", default=["a", "b"], choices=["a", "b"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13", "render_views_ab.json"))
    args = ap.parse_args()
    if args.rounds < 5:
        raise SystemExit("render_views_ab.py: at least 5 alternations")

    import hn_loader
    hn = hn_loader.load()
    from hashnerf_pytorch_amd import functional as HF
    from hashnerf_pytorch_amd.rays import blender_intrinsics
    from hashnerf_pytorch_amd.train import SyntheticBlender, Trainer, default_args

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    T = 19
    out = {}
    loss = None
    if "a" in args.only:
        data = SyntheticBlender(400, 400, 100, dev, seed=0, scene="procedural", n_test=args.views)
        tr = Trainer(default_args(N_rand=4096, N_importance=64, log2_hashmap_size=T), data, dev, seed=0,
                     mode="explicit")
        for _ in range(args.pretrain):
            loss, _ = tr.step()
        torch.cuda.synchronize()
        HF.L.check_device_faults()
        kw = dict(tr.kw_test, near=2., far=6.)
        focal, K = blender_intrinsics(400, 400)
        res, frames = ab(hn, data.test_poses, 400, 400, focal, K, kw, args.rounds)
        gt = data.test_images.cpu().numpy()
        res["psnr_chunked"], res["psnr_image_kernel"] = psnr(frames[False], gt), psnr(frames[True], gt)
        res["field"] = f"procedural chair after {args.pretrain} steps of Trainer(mode='explicit'), N_rand 4096"
        res["shape"] = f"{args.views} x 400 x 400, world rays, near 2, far 6"
        out["a_world_64"] = res
    if "b" in args.only:
        H, W, focal = 378, 504, 407.5
        torch.manual_seed(13)
        p = llff_poses(args.views, 13)
        box = hn.bbox_for_llff(p, (H, W, focal))
        emb = hn.HashEmbedder(box, log2_hashmap_size=T, finest_resolution=512).to(dev)
        with torch.no_grad():
            emb.table.uniform_(-0.5, 0.5)
        mlp = dict(num_layers=2, hidden_dim=64, geo_feat_dim=15, num_layers_color=3, hidden_dim_color=64,
                   input_ch=32, input_ch_views=16)
        mc, mf = hn.NeRFSmall(**mlp).to(dev), hn.NeRFSmall(**mlp).to(dev)
        kw = dict(network_query_fn=hn.NetworkQuery(emb, hn.SHEncoder()), perturb=0., N_importance=64,
                  network_fine=mf, N_samples=64, network_fn=mc, embed_fn=emb, use_viewdirs=True, white_bkgd=False,
                  raw_noise_std=0., ndc=True, lindisp=False, near=0., far=1.)
        K = np.array([[focal, 0, 0.5 * W], [0, focal, 0.5 * H], [0, 0, 1]])
        res, _ = ab(hn, torch.from_numpy(p).to(dev), H, W, focal, K, kw, args.rounds)
        res["field"] = ("seeded random table (uniform +-0.5) and random nets: NOT a trained scene's density, the "
                        "colour-skip share is not representative")
        res["shape"] = f"{args.views} x 378 x 504 (fern's evaluation shape), NDC rays, near 0, far 1"
        out["b_ndc_64_fern_shape"] = res
    HF.L.check_device_faults()

    props = torch.cuda.get_device_properties(dev)
    doc = {"what": "evaluation renderer A/B at 64 + 64 samples: render_path chunked vs whole-image kernel "
                   "(hn_render_views); host clock around a call that ends in a synchronise",
           "device": props.name, "torch": torch.__version__, "hip": torch.version.hip,
           "settings": {"N_samples": 64, "N_importance": 64, "log2_hashmap_size": T, "chunk": 32768,
                        "rounds": args.rounds, "pretrain_steps": args.pretrain,
                        "loss_after_pretrain": None if loss is None else float(loss),
                        "alternation": "chunked then image kernel, call by call; one process",
                        "bar": "a difference counts if it exceeds twice the pooled std of the two arms"},
           "workloads": out}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
