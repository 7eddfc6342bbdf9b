"""The ray gradient of render_rays as the fused kernels assemble it, in torch
float64 on the CPU: near, far and the sampling draws are constants and the
importance samples are detached, so no d z reaches the ray and per ray

    d o       = sum_k dx_k
    d d       = sum_k z_k dx_k + d|d| d / |d|        (0 where |d| = 0)
    d viewdir = J_sh(viewdir)^T sum_k dsh_k

over the 64 coarse points (coarse net, coarse z) and the fine points (fine net,
fine z).  dx_k is hn_encode_bwd_input's closed form on the point's feature
gradient, dsh_k the colour net's input gradient on its 16 SH columns, d|d| =
sum_k d delta_k dist_k of each pass (hn_composite_bwd_inputs).  The per-sample
gradients (d feature, d sh, d delta) come from autograd on detached leaves;
everything from there to the [B, 11] result is written out here, nothing of it
is autograd through the rays.  Columns 6:8 (near, far) are zeros."""
import torch

from test_input_grad_cpu import encode_dx_closed_form, sh_ddirs_closed_form


def _pass(oracle, w, tables, box_min, box_max, res, log2T, o, d, vd, z, noise, white):
    """One pass on detached leaves -> (outputs of raw2outputs, leaves).  The
    leaves: the points' features [B*S, 32], their SH columns [B*S, 16] and
    delta = dists * |d| [B, S]."""
    B, S = z.shape
    pts = (o[:, None, :] + d[:, None, :] * z[..., None]).reshape(-1, 3)
    feat, keep = oracle.hash_encode(pts, tables, box_min, box_max, res, log2T)
    assert bool(keep.all())
    feat = feat.detach().requires_grad_(True)
    sh = oracle.sh_encode(vd[:, None].expand(B, S, 3).reshape(-1, 3)).detach().requires_grad_(True)
    raw = oracle.nerf_small(torch.cat([feat, sh], -1), w).reshape(B, S, 4)
    # raw2outputs (run_nerf_helpers.py:590-611) with delta as a leaf
    dists = torch.cat([z[:, 1:] - z[:, :-1], torch.full((B, 1), 1e10, dtype=z.dtype)], -1)
    delta = (dists * torch.norm(d, dim=-1, keepdim=True)).detach().requires_grad_(True)
    sig = raw[..., 3] if noise is None else raw[..., 3] + noise
    alpha = 1. - torch.exp(-torch.relu(sig) * delta)
    trans = torch.cumprod(torch.cat([torch.ones((B, 1), dtype=z.dtype), 1. - alpha + 1e-10], -1), -1)[:, :-1]
    weights = alpha * trans
    rgb = torch.sum(weights[..., None] * torch.sigmoid(raw[..., :3]), -2)
    acc = torch.sum(weights, -1)
    depth = torch.sum(weights * z, -1) / acc
    if white:
        rgb = rgb + (1. - acc[..., None])
    out = dict(rgb=rgb, acc=acc, depth=depth, sparsity=oracle.entropy_of_weights(weights), weights=weights)
    return out, dict(pts=pts, feat=feat, sh=sh, delta=delta, dists=dists, z=z)


def ray_grad_model(oracle, rays, w_coarse, w_fine, tables, box_min, box_max, res, log2T, n_importance, u, white,
                   loss_of, noise_c=None, noise_f=None, z_fine=None):
    """d loss_of(ret) / d rays [B, 11] for ret = the keys of oracle.render_rays
    that a loss may read (rgb_map, depth_map, acc_map, sparsity_loss, rgb0,
    depth0, acc0, sparsity_loss0).  rays: float64, no grad."""
    rays = rays.detach()
    o, d, vd = rays[:, 0:3], rays[:, 3:6], rays[:, 8:11]
    near, far = rays[:, 6:7], rays[:, 7:8]
    t = oracle.linspace_tvals(64)                 # float32, and so is 1 - t: oracle.render_rays' own z_vals
    z_c = (near * (1. - t) + far * t).expand(rays.shape[0], 64)
    args = (tables, box_min, box_max, res, log2T, o, d, vd)
    out_c, lv_c = _pass(oracle, w_coarse, *args, z_c, noise_c, white)
    if z_fine is None:
        z_mid = .5 * (z_c[..., 1:] + z_c[..., :-1])
        z_s = oracle.sample_pdf(z_mid, out_c["weights"][..., 1:-1], u).detach()
        z_fine, _ = torch.sort(torch.cat([z_c, z_s], -1), -1)
    assert z_fine.shape[1] == 64 + n_importance
    out_f, lv_f = _pass(oracle, w_fine, *args, z_fine.detach(), noise_f, white)
    ret = {"rgb_map": out_f["rgb"], "depth_map": out_f["depth"], "acc_map": out_f["acc"],
           "sparsity_loss": out_f["sparsity"], "rgb0": out_c["rgb"], "depth0": out_c["depth"], "acc0": out_c["acc"],
           "sparsity_loss0": out_c["sparsity"]}
    leaves = [lv[k] for lv in (lv_c, lv_f) for k in ("feat", "sh", "delta")]
    grads = torch.autograd.grad(loss_of(ret), leaves, allow_unused=True)     # a loss may read one pass only
    grads = [torch.zeros_like(x) if g is None else g for g, x in zip(grads, leaves)]
    B = rays.shape[0]
    d_o, d_d, dsh = torch.zeros_like(o), torch.zeros_like(d), torch.zeros(B, 16, dtype=rays.dtype)
    dnorm = torch.norm(d, dim=-1)
    for lv, (dfeat, dsh_k, ddelta) in zip((lv_c, lv_f), (grads[0:3], grads[3:6])):
        S = lv["z"].shape[1]
        dx = encode_dx_closed_form(oracle, lv["pts"], tables, box_min, box_max, res, log2T, dfeat).reshape(B, S, 3)
        d_o = d_o + dx.sum(1)
        d_d = d_d + (lv["z"][..., None] * dx).sum(1)
        dn = (ddelta * lv["dists"]).sum(-1)                       # d loss / d |d| of this pass
        d_d = d_d + torch.where(dnorm > 0, dn / dnorm, torch.zeros_like(dn))[:, None] * d
        dsh = dsh + dsh_k.reshape(B, S, 16).sum(1)
    out = torch.zeros_like(rays)
    out[:, 0:3], out[:, 3:6] = d_o, d_d
    out[:, 8:11] = sh_ddirs_closed_form(oracle, vd, dsh)
    return out
