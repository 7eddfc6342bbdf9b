"""Inputs of the fused ray-gradient tests, made on the CPU so that the oracle
sees the device's exact values: the small scene (T = 14, finest 64,
pcg_table(7), two NeRFSmall nets from torch.manual_seed(5)) in a box of a given
half-width, ray batches of a 400 x 400 blender camera at distance 4, and the
forward-facing NDC camera of the pose test."""
import numpy as np
import torch

from conftest import pcg_table
from gpu_support import MLP_KW, SMALL_FINEST, SMALL_T

SPARSE_W = 1e-3
NDC_H, NDC_W, NDC_FOCAL = 11, 14, 12.0
NDC_K = np.array([[NDC_FOCAL, 0, 0.5 * NDC_W], [0, NDC_FOCAL, 0.5 * NDC_H], [0, 0, 1]])
# The translation was chosen on the CPU among six near (0.3, -0.2, 0.4): on this scene the fp32 oracle's own
# error against the float64 one on the c2w gradient ranged from 4e-5 to 1.3e-3 over them (a sample within
# rounding of a cell face); this one's is well under half of the 5e-4 bar.
NDC_POSE = torch.tensor([[0.98, 0.05, -0.19, 0.26], [-0.04, 0.99, 0.06, -0.26], [0.19, -0.05, 0.98, 0.39]])
NDC_TARGET_SEED = 42


def box(half):
    return torch.tensor([-half] * 3), torch.tensor([half] * 3)


def scene(hn, half=1.5, dead=False, dev="cpu"):
    """Embedder, the two nets and the NetworkQuery, built on the CPU (the same
    values on every machine) and moved to dev.  dead: sigma_net's density row
    all negative, its inputs being ReLU outputs: every raw sigma <= 0."""
    from types import SimpleNamespace
    emb = hn.HashEmbedder(box(half), log2_hashmap_size=SMALL_T, finest_resolution=SMALL_FINEST)
    with torch.no_grad():
        emb.table.copy_(torch.from_numpy(pcg_table(7, SMALL_T)))
    torch.manual_seed(5)
    mc, mf = hn.NeRFSmall(**MLP_KW), hn.NeRFSmall(**MLP_KW)
    if dead:
        with torch.no_grad():
            for m in (mc, mf):
                row = m.sigma_net[1].weight[0]
                row.copy_(-row.abs().clamp_min(1e-3))
    emb, mc, mf = emb.to(dev), mc.to(dev), mf.to(dev)
    return SimpleNamespace(emb=emb, mc=mc, mf=mf, nq=hn.NetworkQuery(emb, hn.SHEncoder()), half=half)


def ray_batch(hn, B, seed=43):
    """B rays [o | d | 2 6 | d / |d|] of a 400 x 400 blender camera on the sphere of radius 4."""
    _, K = hn.rays.blender_intrinsics(400, 400)
    o, d = hn.get_rays(400, 400, K, hn.pose_spherical(30.0, -30.0, 4.0)[:3, :4])
    sel = torch.randperm(400 * 400, generator=torch.Generator().manual_seed(seed))[:B]
    o, d = o.reshape(-1, 3)[sel], d.reshape(-1, 3)[sel]
    return torch.cat([o, d, torch.full((B, 1), 2.), torch.full((B, 1), 6.), d / d.norm(dim=-1, keepdim=True)],
                     -1).contiguous()


def render_kw(s, ni, white, **more):
    kw = dict(network_query_fn=s.nq, perturb=0., N_importance=ni, network_fine=s.mf, N_samples=64, network_fn=s.mc,
              white_bkgd=white, raw_noise_std=0.)
    kw.update(more)
    return kw


def oracle_weights(oracle, s, dt):
    return [{k: v.detach().cpu().to(dt) for k, v in zip(oracle.MLP_KEYS, m.weights())} for m in (s.mc, s.mf)]


def oracle_render(oracle, s, rb, ni, white, z_fine, dt):
    """oracle.render_rays of the scene on a [B, 11] batch of dtype dt."""
    w = oracle_weights(oracle, s, dt)
    B = rb.shape[0]
    lo, hi = (b.to(dt) for b in box(s.half))
    return oracle.render_rays(rb, w[0], w[1], s.emb.table.detach().cpu().to(dt), lo, hi,
                              oracle.level_resolutions(16, 16, SMALL_FINEST), SMALL_T, N_importance=ni,
                              u=torch.linspace(0., 1., ni).to(dt).expand(B, ni), white_bkgd=white,
                              z_fine=None if z_fine is None else z_fine.cpu().to(dt))


def oracle_batch_grad(oracle, s, rays, ni, white, target, z_fine, dt):
    """d training loss / d ray batch by the oracle's autograd, the fine pass on z_fine."""
    rb = rays.detach().cpu().to(dt).requires_grad_(True)
    ret = oracle_render(oracle, s, rb, ni, white, z_fine, dt)
    oracle.training_loss(ret, target.cpu().to(dt), SPARSE_W).backward()
    return rb.grad


def ndc_rays_of(hn, oracle, c2w):
    """render(H, W, K, c2w=c2w, ndc=True, use_viewdirs=True)'s rays -> (o, d, viewdirs), each [H W, 3]."""
    o, d = oracle.get_rays(NDC_H, NDC_W, NDC_K, c2w)
    vd = (d / torch.norm(d, dim=-1, keepdim=True)).reshape(-1, 3)
    o, d = hn.rays.get_ndc_rays(NDC_H, NDC_W, NDC_K[0][0], 1., o, d)
    return o.reshape(-1, 3), d.reshape(-1, 3), vd


def oracle_pose_grad(hn, oracle, s, pose, target, z_fine, dt):
    """d training loss / d c2w of the NDC image (64 + 64, black background) by the oracle's autograd."""
    c2w = pose.detach().cpu().to(dt).requires_grad_(True)
    o, d, vd = ndc_rays_of(hn, oracle, c2w)
    B = o.shape[0]
    rb = torch.cat([o, d, torch.zeros((B, 1), dtype=dt), torch.ones((B, 1), dtype=dt), vd], -1)
    ret = oracle_render(oracle, s, rb, 64, False, z_fine, dt)
    oracle.training_loss(ret, target.reshape(-1, 3).cpu().to(dt), SPARSE_W).backward()
    return c2w.grad, ret
