"""Golden fixture for the whole-image renderer on an LLFF configuration (NDC
rays, 64 + 64 samples, near 0, far 1), made by the REFERENCE's own Python on
CPU.

Run in the survey container only (the reference must be present; see
``make_golden.py``, whose helpers -- the reference shim, the seeded tables and
nets -- this script imports and leaves as they are):

    python tests/golden/make_golden_views.py

``render_views_llff.npz``: run_nerf_helpers.render(H, W, K, chunk=50, c2w=pose,
ndc=True, near=0., far=1., N_samples=64, N_importance=64, perturb=0.,
raw_noise_std=0., white_bkgd=False, use_viewdirs=True, pytest=True) over an
11 x 14 image, T = 12.  The pose is one of ``bbox_llff.npz``'s seeded
near-identity poses (make_golden_ni64.gen_bbox_llff), the box the reference's
bbox.get_bbox3d_for_llff over all of them at this image's (H, W, focal).  The
keys are ``render_image.npz``'s; the table comes from its seed.

Before anything is written the script asserts that the fixture exercises the
composite (some acc strictly between 0.05 and 0.95) and that the project's
oracle, on the same rays, passes the GPU test's comparison against the
reference's outputs (so no ray sits on an importance-sampling knife edge).
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
import make_golden as MG   # noqa: E402

H, W, FOCAL, T, FINEST, NI, POSE = 11, 14, 11.5, 12, 256, 64, 2
# the GPU test's comparison (test_gpu_render_image.test_fixture_image_vs_reference's arguments)
RTOL, ATOL, FRAC, LOOSE = 1e-4, 1e-5, 0.6, 2e-2


def mostly_close_frac(a, b):
    """gpu_support.mostly_close, returning the fraction of rows within (RTOL, ATOL)."""
    a2, b2 = a.reshape(a.shape[0], -1), b.reshape(b.shape[0], -1)
    ok = np.isclose(a2, b2, rtol=RTOL, atol=ATOL, equal_nan=True).all(-1)
    np.testing.assert_allclose(a2, b2, rtol=0, atol=LOOSE)
    assert ok.mean() >= FRAC, ok.mean()
    return float(ok.mean())


def oracle_views(g):
    """The project's oracle on the fixture's inputs: get_rays, the view
    directions, get_ndc_rays at near plane 1 (render()'s steps, in torch on the
    CPU), then oracle.render_rays.  Returns rgb [H W, 3] and acc [H W]."""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from oracle import hashnerf_oracle as O
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    h, w, K = int(g["H"]), int(g["W"]), g["K"]
    c2w = t(g["c2w"])
    i, j = torch.meshgrid(torch.linspace(0, w - 1, w), torch.linspace(0, h - 1, h), indexing="ij")
    i, j = i.t(), j.t()
    dirs = torch.stack([(i - K[0][2]) / K[0][0], -(j - K[1][2]) / K[1][1], -torch.ones_like(i)], -1)
    rd = torch.sum(dirs[..., None, :] * c2w[:3, :3], -1).reshape(-1, 3).float()
    ro = c2w[:3, -1].expand(rd.shape)
    vd = rd / torch.norm(rd, dim=-1, keepdim=True)
    focal = K[0][0]
    tt = -(1. + ro[..., 2]) / rd[..., 2]
    ro = ro + tt[..., None] * rd
    ox_oz, oy_oz = ro[..., 0] / ro[..., 2], ro[..., 1] / ro[..., 2]
    o2 = 1. + 2. * 1. / ro[..., 2]
    no = torch.stack([-1. / (w / (2. * focal)) * ox_oz, -1. / (h / (2. * focal)) * oy_oz, o2], -1)
    nd = torch.stack([-1. / (w / (2. * focal)) * (rd[..., 0] / rd[..., 2] - ox_oz),
                      -1. / (h / (2. * focal)) * (rd[..., 1] / rd[..., 2] - oy_oz), 1 - o2], -1)
    B = rd.shape[0]
    rb = torch.cat([no, nd, torch.zeros(B, 1), torch.ones(B, 1), vd], -1).float()
    g_ = np.random.Generator(np.random.PCG64(int(g["table_seed"])))
    tab = t((g_.random((16, 2 ** int(g["log2T"]), 2), dtype=np.float32) * 2 - 1) * 0.5)
    wc = {k: t(g["wc:" + k]) for k in O.MLP_KEYS}
    wf = {k: t(g["wf:" + k]) for k in O.MLP_KEYS}
    u = torch.tensor(np.broadcast_to(np.linspace(0., 1., NI), (B, NI)), dtype=torch.float32)
    with torch.no_grad():
        ret = O.render_rays(rb, wc, wf, tab, t(g["box_min"]), t(g["box_max"]),
                            O.level_resolutions(16, 16, int(g["finest"])), int(g["log2T"]), N_importance=NI, u=u,
                            white_bkgd=False)
    return ret["rgb_map"].numpy(), ret["acc_map"].numpy()


def gen_render_views_llff(ref, seed=23):
    poses = np.load(os.path.join(HERE, "bbox_llff.npz"))["poses"]
    box = ref.bbox.get_bbox3d_for_llff(poses, (H, W, FOCAL), near=0., far=1.)
    K = np.array([[FOCAL, 0, 0.5 * W], [0, FOCAL, 0.5 * H], [0, 0, 1]])
    emb, tab = MG.make_embedder(ref, box, T, FINEST, seed)
    shenc = ref.sh.SHEncoder()
    mc, mf = MG.make_mlps(ref, seed)
    nq = lambda inputs, viewdirs, fn: ref.rnh.run_network(inputs, viewdirs, fn, embed_fn=emb,
                                                          embeddirs_fn=shenc, netchunk=65536)
    kw = dict(network_query_fn=nq, perturb=0., N_importance=NI, network_fine=mf,
              N_samples=64, network_fn=mc, embed_fn=emb, use_viewdirs=True, white_bkgd=False,
              raw_noise_std=0., lindisp=False, pytest=True)
    pose = torch.from_numpy(poses[POSE][:3, :4])
    with torch.no_grad():
        rgb, depth, acc, extras = ref.rnh.render(H, W, K, chunk=50, c2w=pose, ndc=True, near=0., far=1., **kw)
    arrays = dict(box_min=box[0].numpy(), box_max=box[1].numpy(), log2T=T, finest=FINEST,
                  table_seed=seed, H=H, W=W, K=K, c2w=pose.numpy(), rgb=rgb.numpy(),
                  depth=depth.numpy(), acc=acc.numpy(), rgb0=extras["rgb0"].numpy())
    for tag, m in (("c", mc), ("f", mf)):
        for k, v in m.named_parameters():
            arrays[f"w{tag}:{k}"] = v.detach().numpy()
    a = arrays["acc"]
    mid = int(((a > 0.05) & (a < 0.95)).sum())
    print(f"seed {seed}: acc in [{a.min():.4f}, {a.max():.4f}], {mid} of {a.size} strictly between 0.05 and 0.95")
    assert mid > 0, "the fixture does not exercise the composite: move the seed"
    orgb, oacc = oracle_views(arrays)
    print("oracle against the reference: rgb fraction %.4f, acc fraction %.4f" % (
        mostly_close_frac(orgb, arrays["rgb"].reshape(-1, 3)), mostly_close_frac(oacc, arrays["acc"].reshape(-1))))
    MG.save("render_views_llff", **arrays)


def main():
    torch.set_num_threads(8)
    gen_render_views_llff(MG.load_reference())


if __name__ == "__main__":
    main()
