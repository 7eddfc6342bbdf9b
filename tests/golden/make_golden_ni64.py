"""Golden fixtures for N_importance = 64 (the LLFF configurations' sample
counts) and the LLFF bounding box, made by the REFERENCE's own Python on CPU.

Run in the survey container only (the reference must be present; see
``make_golden.py``, whose helpers -- the reference shim, the seeded tables and
nets, the scene -- this script imports and leaves as they are):

    python tests/golden/make_golden_ni64.py

``render_ni64_*``: ``make_golden.gen_render``'s recipe with N_importance = 64
and u of width 64; the keys are gen_render's.  The table gradient is ~2 MB of
dense fp32 values that barely compress, so its levels 8-15 go into a second
file ``<name>.tg_hi.npz`` (key ``table_grad_hi``) and the main file keeps
levels 0-7 under ``table_grad``: each committed file stays under 1 MiB.
``load_render_ni64`` puts the two back together.

``bbox_llff.npz``: bbox.get_bbox3d_for_llff over 5 seeded near-identity poses.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG   # noqa: E402

NI = 64


def load_render_ni64(name):
    """The fixture as one dict with gen_render's keys (table_grad [16, 2^T, 2])."""
    g = dict(np.load(os.path.join(HERE, name + ".npz")))
    hi = np.load(os.path.join(HERE, name + ".tg_hi.npz"))["table_grad_hi"]
    g["table_grad"] = np.concatenate([g["table_grad"], hi], 0)
    return g


def gen_render_ni64(ref, name, T=14, finest=512, B=64, white=True, perturb=1.0, seed=21, sparse_w=1e-3):
    H = W = 40
    cams, box, K, focal = MG.scene(ref, H, W)
    emb, tab = MG.make_embedder(ref, box, T, finest, seed)
    shenc = ref.sh.SHEncoder()
    mc, mf = MG.make_mlps(ref, seed)
    g = MG.rng(seed)
    pose = cams[5][:3, :4]
    ro, rd = ref.ray_util.get_rays(H, W, K, pose)
    sel = g.choice(H * W, size=B, replace=False)
    rays_o = ro.reshape(-1, 3)[sel]
    rays_d = rd.reshape(-1, 3)[sel]
    target = torch.from_numpy(g.random((B, 3), dtype=np.float32))
    nq = lambda inputs, viewdirs, fn: ref.rnh.run_network(inputs, viewdirs, fn, embed_fn=emb,
                                                          embeddirs_fn=shenc, netchunk=65536)
    kw = dict(network_query_fn=nq, perturb=perturb, N_importance=NI, network_fine=mf,
              N_samples=64, network_fn=mc, embed_fn=emb, use_viewdirs=True, white_bkgd=white,
              raw_noise_std=0., ndc=False, lindisp=False, near=2., far=6., pytest=True)
    rgb, depth, acc, extras = ref.rnh.render(H, W, K, chunk=32768, rays=torch.stack([rays_o, rays_d], 0),
                                              retraw=True, **kw)
    loss = torch.mean((rgb - target) ** 2) + torch.mean((extras["rgb0"] - target) ** 2)
    loss = loss + sparse_w * (extras["sparsity_loss"].sum() + extras["sparsity_loss0"].sum())
    loss.backward()
    # the pytest hooks (run_nerf_helpers.py:531-534, 279-287) use np.random.seed(0)
    np.random.seed(0)
    t_rand = np.random.rand(B, 64).astype(np.float32)
    if perturb > 0:
        np.random.seed(0)
        u = np.random.rand(B, NI).astype(np.float32)
    else:   # det=True under pytest: np.linspace cast to fp32 (:283-287)
        u = np.broadcast_to(np.linspace(0., 1., NI), (B, NI)).astype(np.float32)
    grad = np.stack([emb.embeddings[l].weight.grad.numpy() for l in range(16)], 0)
    arrays = dict(box_min=box[0].numpy(), box_max=box[1].numpy(), log2T=T, finest=finest,
                  table_seed=seed, white=white, perturb=perturb, sparse_w=sparse_w,
                  rays_o=rays_o.numpy(), rays_d=rays_d.numpy(), target=target.numpy(),
                  t_rand=t_rand, u=u, rgb=rgb.detach().numpy(), depth=depth.detach().numpy(),
                  acc=acc.detach().numpy(), loss=loss.detach().numpy(),
                  table_grad=grad[:8])
    for k in ("rgb0", "depth0", "acc0", "sparsity_loss", "sparsity_loss0", "z_std", "raw"):
        arrays[k] = extras[k].detach().numpy()
    for tag, m in (("c", mc), ("f", mf)):
        for k, v in m.named_parameters():
            arrays[f"w{tag}:{k}"] = v.detach().numpy()
            arrays[f"g{tag}:{k}"] = v.grad.numpy()
    MG.save(name, **arrays)
    MG.save(name + ".tg_hi", table_grad_hi=grad[8:])


def gen_bbox_llff(ref):
    """bbox.get_bbox3d_for_llff on 5 seeded near-identity poses (forward-facing
    cameras looking down -z, as LLFF's recentred poses are)."""
    g = MG.rng(41)
    H, W, focal = 47, 63, 52.5
    poses = np.zeros((5, 3, 4), dtype=np.float32)
    for p in poses:
        a = g.normal(0., 0.08, 3)
        rx = np.array([[1, 0, 0], [0, np.cos(a[0]), -np.sin(a[0])], [0, np.sin(a[0]), np.cos(a[0])]])
        ry = np.array([[np.cos(a[1]), 0, np.sin(a[1])], [0, 1, 0], [-np.sin(a[1]), 0, np.cos(a[1])]])
        rz = np.array([[np.cos(a[2]), -np.sin(a[2]), 0], [np.sin(a[2]), np.cos(a[2]), 0], [0, 0, 1]])
        p[:, :3] = (rz @ ry @ rx).astype(np.float32)
        p[:, 3] = g.normal(0., 0.15, 3).astype(np.float32)
    lo, hi = ref.bbox.get_bbox3d_for_llff(poses, (H, W, focal), near=0., far=1.)
    MG.save("bbox_llff", poses=poses, H=H, W=W, focal=focal, near=0., far=1.,
            box_min=lo.numpy(), box_max=hi.numpy())


def main():
    torch.set_num_threads(8)
    ref = MG.load_reference()
    gen_render_ni64(ref, "render_ni64_white_perturb", T=14, white=True, perturb=1.0, seed=21)
    gen_render_ni64(ref, "render_ni64_black_det", T=14, white=False, perturb=0.0, seed=22)
    gen_bbox_llff(ref)


if __name__ == "__main__":
    main()
