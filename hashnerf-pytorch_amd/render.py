"""Volume rendering API of run_nerf_helpers.py (render, render_rays,
raw2outputs, sample_pdf, run_network, batchify, render_path) on HIP kernels.

``render_rays`` dispatches to the fused forward/backward kernels
(``functional.RenderRaysFn``) whenever the configuration is the HashNeRF one
(NetworkQuery over a 16-level HashEmbedder + SH, two NeRFSmall nets, 64+128
or 64+64 samples with view directions) and the rays carry no grad; otherwise it
composes the standalone HIP ops exactly like the reference composes eager ops,
differentiable in the rays as well (``render(..., c2w=pose)`` with a pose that
requires grad).  ``ray_grad="fused"`` keeps rays with grad on the fused
kernels too: their backward then forms the ray gradient from the saved state
(``functional.render_bwd_rays``).  There is no CPU path.
"""
from __future__ import annotations

import functools
import time
from typing import Optional

import numpy as np
import torch

from . import _lib as L
from . import functional as HF
from .embedding import HashEmbedder, SHEncoder
from .functional import _linspace_cached    # (train and the tests import it from here)
from .models import NeRFSmall
from .rays import get_ndc_rays, get_rays

img2mse = lambda x, y: torch.mean((x - y) ** 2)                     # run_nerf_helpers.py:24
mse2psnr = lambda x: -10. * torch.log(x) / torch.log(torch.tensor([10.], device=x.device))
to8b = lambda x: (255 * np.clip(x, 0, 1)).astype(np.uint8)


def batchify(fn, chunk):
    """run_nerf_helpers.py:203-210."""
    if chunk is None:
        return fn
    return lambda inputs: torch.cat([fn(inputs[i:i + chunk]) for i in range(0, inputs.shape[0], chunk)], 0)


def run_network(inputs, viewdirs, fn, embed_fn, embeddirs_fn, netchunk=1024 * 64):
    """run_nerf_helpers.py:212-227."""
    inputs_flat = torch.reshape(inputs, [-1, inputs.shape[-1]])
    embedded, keep_mask = embed_fn(inputs_flat)
    if viewdirs is not None:
        input_dirs = viewdirs[:, None].expand(inputs.shape)
        embedded_dirs = embeddirs_fn(torch.reshape(input_dirs, [-1, input_dirs.shape[-1]]))
        embedded = torch.cat([embedded, embedded_dirs], -1)
    outputs_flat = batchify(fn, netchunk)(embedded)
    outputs_flat = torch.where(keep_mask[:, None] | (torch.arange(outputs_flat.shape[-1],
                               device=outputs_flat.device) != outputs_flat.shape[-1] - 1),
                               outputs_flat, torch.zeros_like(outputs_flat))
    return torch.reshape(outputs_flat, list(inputs.shape[:-1]) + [outputs_flat.shape[-1]])


class NetworkQuery:
    """The ``network_query_fn`` closure of create_nerf (run_nerf_helpers.py:122-125),
    as an object so render_rays can see the embedders and take the fused path."""

    def __init__(self, embed_fn, embeddirs_fn, netchunk=1024 * 64):
        self.embed_fn, self.embeddirs_fn, self.netchunk = embed_fn, embeddirs_fn, netchunk

    def __call__(self, inputs, viewdirs, network_fn):
        return run_network(inputs, viewdirs, network_fn, embed_fn=self.embed_fn,
                           embeddirs_fn=self.embeddirs_fn, netchunk=self.netchunk)


def raw2outputs(raw, z_vals, rays_d, raw_noise_std=0, white_bkgd=False, pytest=False):
    """run_nerf_helpers.py:577-628 -> rgb, disp, acc, weights, depth, sparsity(entropy)."""
    noise = None
    if raw_noise_std > 0.:
        if pytest:
            np.random.seed(0)
            noise = torch.tensor(np.random.rand(*list(raw[..., 3].shape)) * raw_noise_std,
                                 dtype=torch.float32, device=raw.device)
        else:
            noise = torch.randn(raw[..., 3].shape, device=raw.device) * raw_noise_std
    rgb, disp, acc, weights, depth, ent = HF.CompositeFn.apply(raw, z_vals, rays_d, noise, bool(white_bkgd))
    return rgb, disp, acc, weights, depth, ent


def sample_pdf(bins, weights, N_samples, det=False, pytest=False):
    """run_nerf_helpers.py:264-307 (u drawn on the bins' device)."""
    B = bins.shape[0]
    if det:
        u = torch.linspace(0., 1., steps=N_samples, device=bins.device).expand(B, N_samples)
    else:
        u = torch.rand(B, N_samples, device=bins.device)
    if pytest:
        np.random.seed(0)
        u = np.broadcast_to(np.linspace(0., 1., N_samples), (B, N_samples)) if det \
            else np.random.rand(B, N_samples)
        u = torch.tensor(np.ascontiguousarray(u), dtype=torch.float32, device=bins.device)
    return HF.sample_pdf(bins, weights, u)


def _draw(shape, dev, pytest, fn):
    if pytest:
        np.random.seed(0)
        return torch.tensor(np.random.rand(*shape), dtype=torch.float32, device=dev)
    return fn(shape, device=dev)


def _fusable(ray_batch, network_fn, network_query_fn, N_samples, N_importance, network_fine):
    if not isinstance(network_query_fn, NetworkQuery):
        return False
    e, ed = network_query_fn.embed_fn, network_query_fn.embeddirs_fn
    return (isinstance(e, HashEmbedder) and e.n_levels == 16 and isinstance(ed, SHEncoder)
            and ed.degree == 4 and isinstance(network_fn, NeRFSmall)
            and isinstance(network_fine, NeRFSmall) and N_samples == 64 and N_importance in (64, 128)
            and ray_batch.shape[-1] > 8)


def _fused_cfg(ray_batch, network_fn, network_query_fn, N_samples, N_importance, network_fine, white_bkgd, lindisp,
               perturb):
    """The one eligibility pass of render_rays -> (cfg, None) where the fused
    kernels cover the call, else (None, the reason)."""
    if not _fusable(ray_batch, network_fn, network_query_fn, N_samples, N_importance, network_fine):
        return None, ("not the fused HashNeRF configuration (16-level hash grid + SH, two NeRFSmall nets, 64 + 128 "
                      "or 64 + 64 samples, view directions)")
    cfg = HF.make_render_cfg(network_query_fn.embed_fn.grid(), white_bkgd, lindisp, perturb > 0.,
                             n_importance=N_importance)
    # 64 importance samples (the LLFF configurations): fused on the binned
    # backward schedule only; elsewhere the standalone ops, as before
    if N_importance != 128 and L.lib().hn_render_scatter_mode(cfg, ray_batch.shape[0]) != 2:
        return None, ("N_importance = 64 keeps a forward's state on the binned backward schedule only "
                      "(hn_render_scatter_mode != 2 for this table and box)")
    return cfg, None


def render_rays(ray_batch, network_fn, network_query_fn, N_samples, embed_fn=None, retraw=False,
                lindisp=False, perturb=0., N_importance=0, network_fine=None, white_bkgd=False,
                raw_noise_std=0., verbose=False, pytest=False, ray_grad=None):
    """run_nerf_helpers.py:464-574.  Same arguments, same returned dict.
    A ray_batch that requires grad (pose refinement: rays built from a pose
    with grad) takes the standalone-op composition, which is differentiable
    in the rays as the reference's eager ops are.
    ray_grad="fused" (opt-in; a render_kwargs dict may carry it through
    render()): such a batch takes the fused forward instead, its state kept,
    and the backward forms d ray_batch with functional.render_bwd_rays (near
    and far, columns 6:8, get zeros) -- and the table's and weights' gradients
    only where they require grad.  Where the fused forward cannot run (another
    configuration; N_importance = 64 off the binned schedule) that raises
    ValueError naming the reason.  Rays without grad are unaffected."""
    if ray_grad not in (None, "fused"):
        raise ValueError(f"hashnerf_amd.render_rays: ray_grad must be None or \"fused\", got {ray_grad!r}")
    L.require_device(ray_batch)
    B = ray_batch.shape[0]
    dev = ray_batch.device
    cfg = None
    rays_need_grad = ray_batch.requires_grad and torch.is_grad_enabled()
    fused_rays = rays_need_grad and ray_grad == "fused"
    if not rays_need_grad or fused_rays:
        cfg, why = _fused_cfg(ray_batch, network_fn, network_query_fn, N_samples, N_importance, network_fine,
                              white_bkgd, lindisp, perturb)
        if fused_rays and cfg is None:
            raise ValueError(f"hashnerf_amd.render_rays: ray_grad=\"fused\" not eligible: {why}")
    if cfg is not None:
        emb = network_query_fn.embed_fn
        t_vals = _linspace_cached(N_samples, dev)
        t_rand = _draw((B, N_samples), dev, pytest, torch.rand) if perturb > 0. else None
        if perturb == 0.:
            if pytest:
                u = torch.tensor(np.broadcast_to(np.linspace(0., 1., N_importance), (B, N_importance)),
                                 dtype=torch.float32, device=dev)
            else:
                u = torch.linspace(0., 1., N_importance, device=dev).expand(B, N_importance)
        else:
            u = _draw((B, N_importance), dev, pytest, torch.rand)
        noise_c = noise_f = None
        if raw_noise_std > 0.:
            rn = (lambda s, device: torch.randn(s, device=device))
            noise_c = _draw((B, N_samples), dev, pytest, rn) * raw_noise_std
            noise_f = _draw((B, N_samples + N_importance), dev, pytest, rn) * raw_noise_std
        (rgb, depth, acc, sp, rgb0, depth0, acc0, sp0, z_std, raw) = HF.render_rays_fused(
            cfg, ray_batch, t_vals, t_rand, u, noise_c, noise_f, emb.table, network_fn.weights(),
            network_fine.weights(), ray_grad=fused_rays)
        ret = {"rgb_map": rgb, "depth_map": depth, "acc_map": acc, "sparsity_loss": sp}
        if retraw:
            ret["raw"] = raw
        ret.update({"rgb0": rgb0, "depth0": depth0, "acc0": acc0, "sparsity_loss0": sp0, "z_std": z_std})
        return ret
    return _render_rays_unfused(ray_batch, network_fn, network_query_fn, N_samples, retraw, lindisp,
                                perturb, N_importance, network_fine, white_bkgd, raw_noise_std, pytest)


def _render_rays_unfused(ray_batch, network_fn, network_query_fn, N_samples, retraw, lindisp, perturb,
                         N_importance, network_fine, white_bkgd, raw_noise_std, pytest):
    """Composition of the standalone HIP ops, op-for-op like the reference."""
    B = ray_batch.shape[0]
    dev = ray_batch.device
    rays_o, rays_d = ray_batch[:, 0:3], ray_batch[:, 3:6]
    viewdirs = ray_batch[:, -3:] if ray_batch.shape[-1] > 8 else None
    bounds = torch.reshape(ray_batch[..., 6:8], [-1, 1, 2])
    near, far = bounds[..., 0], bounds[..., 1]
    t_vals = torch.linspace(0., 1., steps=N_samples).to(dev)
    z_vals = near * (1. - t_vals) + far * t_vals if not lindisp else \
        1. / (1. / near * (1. - t_vals) + 1. / far * t_vals)
    z_vals = z_vals.expand([B, N_samples])
    if perturb > 0.:
        mids = .5 * (z_vals[..., 1:] + z_vals[..., :-1])
        upper = torch.cat([mids, z_vals[..., -1:]], -1)
        lower = torch.cat([z_vals[..., :1], mids], -1)
        t_rand = _draw(tuple(z_vals.shape), dev, pytest, torch.rand)
        z_vals = lower + (upper - lower) * t_rand
    pts = rays_o[..., None, :] + rays_d[..., None, :] * z_vals[..., :, None]
    raw = network_query_fn(pts, viewdirs, network_fn)
    rgb_map, disp_map, acc_map, weights, depth_map, sp = raw2outputs(raw, z_vals, rays_d, raw_noise_std,
                                                                     white_bkgd, pytest=pytest)
    ret = {}
    if N_importance > 0:
        rgb0, depth0, acc0, sp0 = rgb_map, depth_map, acc_map, sp
        z_mid = .5 * (z_vals[..., 1:] + z_vals[..., :-1])
        z_samples = sample_pdf(z_mid, weights[..., 1:-1], N_importance, det=(perturb == 0.),
                               pytest=pytest).detach()
        z_vals, _ = torch.sort(torch.cat([z_vals, z_samples], -1), -1)
        pts = rays_o[..., None, :] + rays_d[..., None, :] * z_vals[..., :, None]
        run_fn = network_fn if network_fine is None else network_fine
        raw = network_query_fn(pts, viewdirs, run_fn)
        rgb_map, disp_map, acc_map, weights, depth_map, sp = raw2outputs(raw, z_vals, rays_d,
                                                                         raw_noise_std, white_bkgd,
                                                                         pytest=pytest)
    ret.update({"rgb_map": rgb_map, "depth_map": depth_map, "acc_map": acc_map, "sparsity_loss": sp})
    if retraw:
        ret["raw"] = raw
    if N_importance > 0:
        ret.update({"rgb0": rgb0, "depth0": depth0, "acc0": acc0, "sparsity_loss0": sp0,
                    "z_std": torch.std(z_samples, dim=-1, unbiased=False)})
    return ret


def render(H, W, K, chunk=1024 * 32, rays=None, c2w=None, ndc=True, near=0., far=1.,
           use_viewdirs=False, c2w_staticcam=None, **kwargs):
    """run_nerf_helpers.py:310-392 -> [rgb_map, depth_map, acc_map, extras]."""
    if c2w is not None:
        rays_o, rays_d = get_rays(H, W, K, c2w)
    else:
        rays_o, rays_d = rays
    if use_viewdirs:
        viewdirs = rays_d
        if c2w_staticcam is not None:
            rays_o, rays_d = get_rays(H, W, K, c2w_staticcam)
        viewdirs = viewdirs / torch.norm(viewdirs, dim=-1, keepdim=True)
        viewdirs = torch.reshape(viewdirs, [-1, 3]).float()
    sh = rays_d.shape
    if ndc:
        rays_o, rays_d = get_ndc_rays(H, W, K[0][0], 1., rays_o, rays_d)
    rays_o = torch.reshape(rays_o, [-1, 3]).float()
    rays_d = torch.reshape(rays_d, [-1, 3]).float()
    near, far = near * torch.ones_like(rays_d[..., :1]), far * torch.ones_like(rays_d[..., :1])
    rays_ = torch.cat([rays_o, rays_d, near, far], -1)
    if use_viewdirs:
        rays_ = torch.cat([rays_, viewdirs], -1)
    return render_ray_batch(rays_, sh[:-1], chunk, **kwargs)


def render_ray_batch(rays_, out_shape, chunk=1024 * 32, **kwargs):
    """The chunk loop + output assembly of render() (run_nerf_helpers.py:370-392)
    over an already built [N, 8 or 11] ray batch (e.g. from the device sampler).
    render()-level keywords of a render_kwargs dict (ndc, near, far,
    use_viewdirs, c2w_staticcam) are already baked into the batch."""
    for k in ("ndc", "near", "far", "use_viewdirs", "c2w_staticcam"):
        kwargs.pop(k, None)
    all_ret = {}
    for i in range(0, rays_.shape[0], chunk):
        ret = render_rays(rays_[i:i + chunk], **kwargs)
        for k in ret:
            all_ret.setdefault(k, []).append(ret[k])
    all_ret = {k: (v[0] if len(v) == 1 else torch.cat(v, 0)) for k, v in all_ret.items()}
    for k in all_ret:
        all_ret[k] = torch.reshape(all_ret[k], list(out_shape) + list(all_ret[k].shape[1:]))
    k_extract = ["rgb_map", "depth_map", "acc_map"]
    return [all_ret[k] for k in k_extract] + [{k: all_ret[k] for k in all_ret if k not in k_extract}]


def _image_ineligible(kw) -> Optional[str]:
    """Why render_image cannot render this render() configuration (None: it can)."""
    why = _views_ineligible(kw)
    if why is None and kw.get("N_importance", 0) != 128:
        why = "N_importance != 128"
    if why is None and kw.get("ndc", True):
        why = "ndc rays"
    return why


def _whole_image(name, ineligible, call, H, W, K, c2w, kw):
    """render_image and render_views: the render() configuration kw checked by
    ``ineligible``, then ``call`` (the functional module's) on its cfg, poses,
    table and weights."""
    why = ineligible(kw)
    if why is not None:
        raise ValueError(f"hashnerf_amd.{name}: not eligible: {why}")
    c2w = torch.as_tensor(c2w)
    L.require_device(c2w)
    single = c2w.dim() == 2
    poses = (c2w[None] if single else c2w)[:, :3, :4]
    emb = kw["network_query_fn"].embed_fn
    cfg = HF.make_render_cfg(emb.grid(), bool(kw.get("white_bkgd", False)), bool(kw.get("lindisp", False)), False,
                             n_importance=kw["N_importance"])
    out = call(cfg, H, W, K, poses, kw.get("near", 0.), kw.get("far", 1.), emb.table,
               kw["network_fn"].weights() + kw["network_fine"].weights())
    return tuple(t[0] for t in out) if single else out


@torch.no_grad()
def render_image(H, W, K, c2w, **render_kwargs):
    """render(H, W, K, c2w=c2w, **render_kwargs)'s rgb, depth and acc maps from
    the whole-image kernel (functional.render_image): rays, both passes and
    the composite in one launch, nothing else written.  c2w: one [3, 4] pose or
    [n, 3, 4] (or [.., 4, 4]) poses, all rendered in that launch; returns rgb
    [(n,) H, W, 3], depth and acc [(n,) H, W].  Raises ValueError, naming the
    reason, for a configuration the kernel does not cover: anything but the
    fused HashNeRF configuration, N_importance != 128, perturb, raw noise, ndc,
    no view directions, c2w_staticcam or retraw."""
    return _whole_image("render_image", _image_ineligible, HF.render_image, H, W, K, c2w, render_kwargs)


def _views_ineligible(kw) -> Optional[str]:
    """Why render_views cannot render this render() configuration (None: it
    can): everything the fused forward covers with perturb = 0 and no raw
    noise -- N_importance 64 or 128, ndc either way."""
    if not _fusable(np.empty((0, 11)), kw.get("network_fn"), kw.get("network_query_fn"), kw.get("N_samples"),
                    kw.get("N_importance", 0), kw.get("network_fine")):
        return ("not the fused HashNeRF configuration (16-level hash grid + SH, two NeRFSmall nets, 64 + 128 or "
                "64 + 64 samples)")
    for why, bad in (("perturb != 0", kw.get("perturb", 0.) != 0.),
                     ("raw_noise_std != 0", kw.get("raw_noise_std", 0.) != 0.),
                     ("no view directions (use_viewdirs=False)", not kw.get("use_viewdirs", False)),
                     ("c2w_staticcam", kw.get("c2w_staticcam") is not None),
                     ("retraw", bool(kw.get("retraw", False)))):
        if bad:
            return why
    return None


@torch.no_grad()
def render_views(H, W, K, c2w, **render_kwargs):
    """render_image for every configuration _views_ineligible accepts: the
    fused HashNeRF configuration with N_importance 64 or 128 and ndc either way
    (render()'s default ndc=True means NDC rays here too: the LLFF
    configurations' evaluation).  Same arguments, same returns, one launch
    (functional.render_views).  At 64 the inference forward runs for every
    table size: no binned backward is needed.  Raises ValueError, naming the
    reason, for perturb, raw noise, no view directions, c2w_staticcam, retraw
    or anything but the fused configuration."""
    call = functools.partial(HF.render_views, ndc=bool(render_kwargs.get("ndc", True)))
    return _whole_image("render_views", _views_ineligible, call, H, W, K, c2w, render_kwargs)


unpack_occupancy = HF.unpack_occupancy


def _density_field(who, network_fn, network_query_fn):
    """(grid, table, weights) of a field the density kernel covers -- _fusable's
    conditions on the embedder and the net -- else ValueError naming the reason."""
    why = None
    if not isinstance(network_query_fn, NetworkQuery):
        why = "network_query_fn is not a NetworkQuery"
    elif not isinstance(network_query_fn.embed_fn, HashEmbedder):
        why = "the embedder is not a HashEmbedder"
    elif network_query_fn.embed_fn.n_levels != 16:
        why = f"the hash grid has {network_query_fn.embed_fn.n_levels} levels, not 16"
    elif not isinstance(network_fn, NeRFSmall):
        why = "network_fn is not a NeRFSmall"
    if why is not None:
        raise ValueError(f"hashnerf_amd.{who}: not eligible: {why}")
    emb = network_query_fn.embed_fn
    return emb.grid(), emb.table, network_fn.weights()


def cell_centre_lattice(resolution, bmin, bmax):
    """density_grid's lattice over the box [bmin, bmax]: resolution = n or (nx,
    ny, nz) cells, one point at each cell's centre -- step = (bmax - bmin) / n
    and lo = bmin + 0.5 * step, in float32 on the host.  Returns (lo, step,
    dims): two CPU float32 tensors and (nx, ny, nz)."""
    dims = (int(resolution),) * 3 if isinstance(resolution, (int, np.integer)) else tuple(int(v) for v in resolution)
    if len(dims) != 3 or min(dims) <= 0:
        raise ValueError(f"hashnerf_amd.density_grid: resolution must be n or (nx, ny, nz), each >= 1, got "
                         f"{resolution!r}")
    bmin = torch.as_tensor(bmin).detach().to("cpu", torch.float32).reshape(3)
    bmax = torch.as_tensor(bmax).detach().to("cpu", torch.float32).reshape(3)
    step = (bmax - bmin) / torch.tensor(dims, dtype=torch.float32)
    return bmin + 0.5 * step, step, dims


@torch.no_grad()
def query_density(pts, network_fn, network_query_fn, threshold=None):
    """Raw sigma of the field at pts [..., 3] -> [...]: network_fn's column 3
    (before raw2outputs' ReLU) at each point, bitwise what network_fn(cat[
    embed_fn(pts), sh]) gives there, from the density kernel alone
    (functional.density_points): no colour net, nothing per point written but
    the answer.  With a threshold: (sigma, sigma > threshold as bool [...]).
    network_fn / network_query_fn: create_nerf's (a NeRFSmall over a NetworkQuery
    with a 16-level HashEmbedder; anything else raises ValueError)."""
    grid, table, ws = _density_field("query_density", network_fn, network_query_fn)
    pts = torch.as_tensor(pts)
    if pts.shape[-1] != 3:
        raise ValueError(f"hashnerf_amd.query_density: pts must be [..., 3], got {tuple(pts.shape)}")
    shape = pts.shape[:-1]
    out = HF.density_points(grid, table, ws, pts.reshape(-1, 3), threshold=threshold)
    if threshold is None:
        return out.reshape(shape)
    sigma, occ = out
    if sigma.numel() == 0:   # no points: no words to unpack
        return sigma.reshape(shape), torch.empty(shape, dtype=torch.bool, device=sigma.device)
    return sigma.reshape(shape), HF.unpack_occupancy(occ, (sigma.numel(), 1, 1)).reshape(shape)


@torch.no_grad()
def density_grid(resolution, network_fn, network_query_fn, bounds=None, threshold=None, want_sigma=True):
    """Raw sigma of the field on a regular lattice, for meshing or an
    occupancy grid: resolution = n or (nx, ny, nz) cells over bounds = (min,
    max) (default: the embedder's bounding box), one point at each cell's
    centre (cell_centre_lattice).  The kernel forms the points itself
    (functional.density_lattice).  Returns sigma [nz, ny, nx]; with a threshold
    (sigma, words), words = the packed int32 occupancy sigma > threshold
    (unpack_occupancy(words, dims) -> bool [nz, ny, nx]); with want_sigma=False
    only the words (1 bit per point written)."""
    grid, table, ws = _density_field("density_grid", network_fn, network_query_fn)
    bmin, bmax = network_query_fn.embed_fn.box() if bounds is None else bounds
    lo, step, dims = cell_centre_lattice(resolution, bmin, bmax)
    return HF.density_lattice(grid, table, ws, lo, step, dims, threshold=threshold, want_sigma=want_sigma)


_IMAGE_GROUP = 8    # views per render_views launch of render_path: bounds the output buffers


@torch.no_grad()
def render_path(render_poses, hwf, K, chunk, render_kwargs, gt_imgs=None, savedir=None,
                render_factor=0, image_kernel=False):
    """run_nerf_helpers.py:395-459 (evaluation): returns (rgbs, depths), depth
    normalised to [0, 1] between near and far.  With gt_imgs (and no
    render_factor) the per-image PSNRs are computed as the reference does and,
    when savedir is given, pickled to test_psnrs_avg{avg:0.2f}.pkl like
    :452-456.  The per-frame matplotlib figures (:435-449) are not written:
    plotting is outside the hot path.
    image_kernel=True renders the poses through render_views, _IMAGE_GROUP
    views per launch, where the configuration is eligible for it
    (_views_ineligible: the LLFF configurations too; the same maps, PSNRs and
    pickle); where it is not, this is the default path."""
    H, W, focal = hwf
    near, far = render_kwargs["near"], render_kwargs["far"]
    if render_factor != 0:
        H, W, focal = H // render_factor, W // render_factor, focal / render_factor
    rgbs, depths, psnrs = [], [], []
    use_image = image_kernel and _views_ineligible(render_kwargs) is None
    maps = None
    for i, c2w in enumerate(render_poses):
        if use_image:
            if i % _IMAGE_GROUP == 0:
                group = torch.stack([torch.as_tensor(p)[:3, :4] for p in render_poses[i:i + _IMAGE_GROUP]], 0)
                maps = render_views(H, W, K, group, **render_kwargs)
            rgb, depth = maps[0][i % _IMAGE_GROUP], maps[1][i % _IMAGE_GROUP]
        else:
            rgb, depth, acc, _ = render(H, W, K, chunk=chunk, c2w=c2w[:3, :4], **render_kwargs)
        rgbs.append(rgb.cpu().numpy())
        depths.append(((depth - near) / (far - near)).cpu().numpy())
        if gt_imgs is not None and render_factor == 0:
            gt = gt_imgs[i].cpu().numpy() if torch.is_tensor(gt_imgs[i]) else gt_imgs[i]
            psnrs.append(-10. * np.log10(np.mean(np.square(rgbs[-1] - gt))))
    if gt_imgs is not None and render_factor == 0 and savedir is not None and psnrs:
        import os
        import pickle
        avg = sum(psnrs) / len(psnrs)
        with open(os.path.join(savedir, "test_psnrs_avg{:0.2f}.pkl".format(avg)), "wb") as fp:
            pickle.dump(psnrs, fp)
    render_path.last_psnrs = psnrs
    return np.stack(rgbs, 0), np.stack(depths, 0)
