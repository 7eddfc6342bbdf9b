"""torch.autograd wrappers around the HIP C ABI (one Function per entry point).

PyTorch supplies device memory, the current HIP stream and autograd
plumbing; every byte of arithmetic on the hot path runs in the gfx950 HIP
library.  Gradient buffers are zero-initialised here and accumulated (+=) by
the kernels, mirroring the C ABI contract.
"""
from __future__ import annotations

import ctypes as C
import math
import os
import weakref
from typing import Optional, Sequence

import torch

from . import _lib as L


class KernelTimer:
    """Optional HIP-event timing of the fused launches (bench.py): events are
    recorded on the same stream the kernels are enqueued on.  ``names``
    limits the timed launches (None: all); each recorded event idles the
    device for ~5 us, so bench times only what its line reports from the
    timed steps.  ``every`` = k times only every k-th call of a name (the
    sampled launches' mean; the others carry no events)."""

    def __init__(self):
        self.events = {}
        self.enabled = False
        self.names = None
        self.every = 1
        self.calls = {}

    def begin(self, name):
        if not self.enabled or (self.names is not None and name not in self.names):
            return None
        c = self.calls.get(name, 0)
        self.calls[name] = c + 1
        if c % max(self.every, 1):
            return None
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    def end(self, name, start):
        if start is None:
            return
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        self.events.setdefault(name, []).append((start, e))

    def mean_ms(self, name):
        ev = self.events.get(name, [])
        return sum(s.elapsed_time(e) for s, e in ev) / max(len(ev), 1)

    def reset(self):
        self.events = {}
        self.calls = {}


TIMER = KernelTimer()

# Debug hook for parity tests: when True, the fused forward keeps its saved
# z-values / raw outputs of the last call in LAST (no effect on results).
DEBUG_KEEP = False
LAST = {}
# The form of render_fwd_kernel that render_fwd calls without a form= of their
# own run (_lib.FWD_FORMS: "auto", the library's rule; "ring"; "resident" --
# identical bits).  A/B measurements of a whole step set it.
FWD_FORM = "auto"
# When True, every render backward is followed by a check of the device fault
# word (hn_device_faults: a blocking read).  The tests turn it on; trainers
# check every Trainer.fault_check_every steps instead.
CHECK_FAULTS = os.environ.get("HN_CHECK_FAULTS", "0") == "1"


def _ws(nbytes: int, device) -> torch.Tensor:
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)


def _ws_size(wsb) -> int:
    return wsb.numel() * wsb.element_size()


def _caller_ws(who: str, wsb, nbytes: int, dev):
    """A call's workspace and its size in bytes: the caller's wsb (contiguous,
    on dev, >= nbytes), or without one a fresh buffer of nbytes."""
    if wsb is None:
        return _ws(nbytes, dev), nbytes
    if _ws_size(wsb) < nbytes or not wsb.is_contiguous() or wsb.device != dev:
        raise ValueError(f"hashnerf_amd.{who}: wsb must be a contiguous buffer of >= {nbytes} bytes on {dev}")
    return wsb, _ws_size(wsb)


_LINSPACE = {}


def _linspace_cached(n, dev):
    """torch.linspace(0, 1, n) made on the CPU as the reference does (:514),
    copied to the device once (a per-call pageable copy would stall the
    host on every training step)."""
    key = (n, str(dev))
    t = _LINSPACE.get(key)
    if t is None:
        t = _LINSPACE[key] = torch.linspace(0., 1., steps=n).to(dev)
    return t


# --------------------------------------------------------------------------
# hash encoding (embedding/hash_encoding.py:84-110)
# --------------------------------------------------------------------------
class HashEncodeFn(torch.autograd.Function):
    """Each gradient is launched only where it is needed: d table
    (hn_encode_bwd into a zeroed table-sized buffer) for a table that requires
    grad, d x (hn_encode_bwd_input) for points that do -- a frozen field under
    pose refinement pays for no table gradient."""

    @staticmethod
    def forward(ctx, x: torch.Tensor, table: torch.Tensor, grid: L.HnGrid):
        L.require_device(x, table)
        x, table = x.contiguous(), table.contiguous()
        n = x.shape[0]
        n_feat = grid.n_levels * grid.n_features
        feat = torch.empty((n, n_feat), dtype=torch.float32, device=x.device)
        keep = torch.empty((n,), dtype=torch.uint8, device=x.device)
        L.check(L.lib().hn_encode_fwd(grid, L.ptr(x), n, L.ptr(table), L.ptr(feat),
                                      L.ptr(keep), L.stream(x.device)), "encode_fwd")
        ctx.save_for_backward(x, table)
        ctx.grid = grid
        ctx.mark_non_differentiable(keep)
        return feat, keep.bool()

    @staticmethod
    def backward(ctx, dfeat, _dkeep):
        x, table = ctx.saved_tensors
        dfeat = dfeat.contiguous()
        dx = dtable = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            L.check(L.lib().hn_encode_bwd_input(ctx.grid, L.ptr(x), x.shape[0], L.ptr(table), L.ptr(dfeat),
                                                L.ptr(dx), L.stream(x.device)), "encode_bwd_input")
        if ctx.needs_input_grad[1]:
            dtable = torch.zeros_like(table)
            L.check(L.lib().hn_encode_bwd(ctx.grid, L.ptr(x), x.shape[0], L.ptr(dfeat), L.ptr(dtable),
                                          L.stream(x.device)), "encode_bwd")
        return dx, dtable, None


def hash_encode(x, table, grid):
    return HashEncodeFn.apply(x, table, grid)


class SHEncodeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, d: torch.Tensor):
        out = torch.empty((d.shape[0], 16), dtype=torch.float32, device=d.device)
        L.check(L.lib().hn_sh_fwd(L.ptr(d), d.shape[0], L.ptr(out), L.stream(d.device)), "sh_fwd")
        ctx.save_for_backward(d)
        return out

    @staticmethod
    def backward(ctx, dout):
        (d,) = ctx.saved_tensors
        dd = torch.empty_like(d)
        L.check(L.lib().hn_sh_bwd(L.ptr(d), L.ptr(dout.contiguous()), d.shape[0], L.ptr(dd),
                                  L.stream(d.device)), "sh_bwd")
        return dd


def sh_encode(dirs: torch.Tensor) -> torch.Tensor:
    """SHEncoder.forward, degree 4 (embedding/spherical_harmonic.py:65-103)."""
    L.require_device(dirs)
    out = SHEncodeFn.apply(dirs.reshape(-1, 3).contiguous())
    return out.reshape(*dirs.shape[:-1], 16)


# --------------------------------------------------------------------------
# NeRFSmall (models.py:151-174)
# --------------------------------------------------------------------------
class NeRFSmallFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w0, w1, w2, w3, w4):
        L.require_device(x, w0, w1, w2, w3, w4)
        x = x.contiguous()
        ws = [w.contiguous() for w in (w0, w1, w2, w3, w4)]
        n = x.shape[0]
        out = torch.empty((n, 4), dtype=torch.float32, device=x.device)
        nbytes = L.lib().hn_mlp_workspace_bytes()
        ws_buf = _ws(nbytes, x.device)
        L.check(L.lib().hn_mlp_fwd(L.make_mlp(ws), L.ptr(x), n, L.ptr(out), L.ptr(ws_buf), nbytes,
                                   L.stream(x.device)), "mlp_fwd")
        ctx.save_for_backward(x, *ws)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, *ws = ctx.saved_tensors
        dout = dout.contiguous()
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dws = [torch.zeros_like(w) for w in ws]
        nbytes = L.lib().hn_mlp_workspace_bytes()
        ws_buf = _ws(nbytes, x.device)
        L.check(L.lib().hn_mlp_bwd(L.make_mlp(ws), L.ptr(x), L.ptr(dout), x.shape[0], L.ptr(dx),
                                   L.make_mlp_grad(dws), L.ptr(ws_buf), nbytes, L.stream(x.device)),
                "mlp_bwd")
        return (dx, *dws)


# --------------------------------------------------------------------------
# raw2outputs (run_nerf_helpers.py:577-628) and sample_pdf (:264-307)
# --------------------------------------------------------------------------
class CompositeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, raw, z, rays_d, noise, white: bool):
        L.require_device(raw, z, rays_d, noise)
        raw, z, rays_d, noise = (L.contig(t) for t in (raw, z, rays_d, noise))
        B, S = z.shape
        dev = raw.device
        rgb = torch.empty((B, 3), device=dev)
        disp, acc, depth, ent = (torch.empty((B,), device=dev) for _ in range(4))
        weights = torch.empty((B, S), device=dev)
        L.check(L.lib().hn_composite_fwd(L.ptr(raw), L.ptr(z), L.ptr(rays_d), L.ptr(noise), B, S,
                                         int(white), L.ptr(rgb), L.ptr(disp), L.ptr(acc),
                                         L.ptr(weights), L.ptr(depth), L.ptr(ent), L.stream(dev)),
                "composite_fwd")
        ctx.save_for_backward(raw, z, rays_d, noise, depth)
        ctx.set_materialize_grads(False)   # unused outputs => NULL, not zeros (0*inf)
        ctx.white = white
        return rgb, disp, acc, weights, depth, ent

    @staticmethod
    def backward(ctx, g_rgb, g_disp, g_acc, g_weights, g_depth, g_ent):
        raw, z, rays_d, noise, depth = ctx.saved_tensors
        if g_disp is not None:
            # disp = 1 / max(1e-10, depth): fold into the depth gradient
            gd = torch.where(depth > 1e-10, -g_disp / (depth * depth), torch.zeros_like(depth))
            g_depth = gd if g_depth is None else g_depth + gd
        B, S = z.shape
        d_raw = torch.empty_like(raw)
        gs = [L.contig(g) for g in (g_rgb, g_acc, g_depth, g_ent, g_weights)]
        L.check(L.lib().hn_composite_bwd(L.ptr(raw), L.ptr(z), L.ptr(rays_d), L.ptr(noise), B, S,
                                         int(ctx.white), *(L.ptr(g) for g in gs), L.ptr(d_raw),
                                         L.stream(raw.device)), "composite_bwd")
        # z and rays_d (pose refinement; rays with grad): a launch of its own, d_raw as before
        d_z = torch.empty_like(z) if ctx.needs_input_grad[1] else None
        d_rays_d = torch.empty_like(rays_d) if ctx.needs_input_grad[2] else None
        if d_z is not None or d_rays_d is not None:
            L.check(L.lib().hn_composite_bwd_inputs(L.ptr(raw), L.ptr(z), L.ptr(rays_d), L.ptr(noise), B, S,
                                                    int(ctx.white), *(L.ptr(g) for g in gs), L.ptr(d_z),
                                                    L.ptr(d_rays_d), L.stream(raw.device)),
                    "composite_bwd_inputs")
        return d_raw, d_z, d_rays_d, None, None


def sample_pdf(bins: torch.Tensor, weights: torch.Tensor, u: torch.Tensor) -> torch.Tensor:
    L.require_device(bins, weights, u)
    bins, weights, u = bins.contiguous(), weights.detach().contiguous(), u.contiguous()
    B, nb = bins.shape
    ns = u.shape[-1]
    out = torch.empty((B, ns), device=bins.device)
    L.check(L.lib().hn_sample_pdf(L.ptr(bins), L.ptr(weights), L.ptr(u), B, nb, ns, L.ptr(out),
                                  L.stream(bins.device)), "sample_pdf")
    return out


# --------------------------------------------------------------------------
# fused render_rays (run_nerf_helpers.py:464-574)
# --------------------------------------------------------------------------
class RenderState:
    """Buffers one fused forward leaves for its backward (z values, raw
    outputs, coarse origin of each fine sample, hash features, the workspace
    holding the packed weights)."""
    __slots__ = ("cfg", "rays", "noise_c", "noise_f", "table", "ws", "z_c", "z_f", "raw_c", "raw_f",
                 "fine_src", "feat", "wsb", "nbytes", "bwd_args", "skip_dead", "prepass_done", "__weakref__")

    def __init__(self):
        self.cfg = self.rays = self.noise_c = self.noise_f = self.table = self.ws = None
        self.z_c = self.z_f = self.raw_c = self.raw_f = self.fine_src = self.feat = None
        self.wsb = self.nbytes = None
        self.bwd_args = None        # a render_bwd(owner_defer=True)'s arguments, for render_bwd_owner
        self.skip_dead = False      # the forward ran with skip_dead_color
        self.prepass_done = None    # the loss key of a render_fwd(loss=...) no backward has used yet


def _fine_counts(cfg):
    """(importance samples, fine samples per ray) of a render cfg: the widths
    of u and of z_fine / raw_f / fine_src / noise_f / g_raw_f."""
    ni = int(cfg.n_importance)
    return ni, int(cfg.n_samples) + ni


# workspace address -> the state of the last forward that ran the composite
# backward into it (render_fwd(loss=...)): one workspace holds one ray batch's
# d raw, so a later such forward on it invalidates the earlier state's
_PREPASS_ON_WS = {}


def _loss_key(loss):
    """What a render_bwd(prepass_done=True)'s loss must repeat of the one its
    forward took (RenderState.prepass_done)."""
    return L.contig(loss["target"]).data_ptr(), float(loss["world"]), float(loss["sparse_w"])


def _render_loss(loss, tensors, scalars):
    """An hn_render_loss with the named tensor and scalar fields of the dict
    filled in, and those tensors (contiguous: the struct points at them)."""
    la = L.HnRenderLoss()
    ts = [L.contig(loss[k]) for k in tensors]
    L.require_device(*ts)
    for k, t in zip(tensors, ts):
        setattr(la, k, t.data_ptr())
    for k in scalars:
        setattr(la, k, float(loss[k]))
    return la, ts


def render_fwd(cfg, rays, t_vals, t_rand, u, noise_c, noise_f, table, ws, keep_feat, wsb=None,
               weights_packed=False, skip_dead_color=False, loss=None, form=None):
    """hn_render_fwd (run_nerf_helpers.py:464-574, forward).  Returns the
    output dict and a RenderState (None when keep_feat is False).  wsb: the
    caller's workspace (uint8, >= workspace_bytes; default a fresh one);
    weights_packed: it already holds ws's packed copies (render_bwd with
    repack=True since the last change of ws).  skip_dead_color (ABI 14, the
    trainer): tiles whose 32 raw sigmas are all <= 0 skip the colour net --
    rgb, depth, acc, the entropies and every gradient unchanged, the raw rgb
    of those samples written as 0 -- and such fine tiles' features are not
    stored: the backward must then run with cfg.dense_bwd = 0 (render_bwd
    refuses dense_bwd = 1 on such a state).
    loss = dict(target [B, 3], world, sparse_w) (the trainer's step, binned
    scatter only): each ray's forward wave also runs the composite backward
    of the training loss on the raw / z it still holds, and leaves d raw and
    the work marks in the workspace; the state's one render_bwd then takes
    the same loss with prepass_done=True and launches no pre-pass (bitwise
    the same gradients; every output here is unchanged).
    form (hn_render_fwd_form; None = FWD_FORM): "auto", "ring" (4-ray
    workgroups, the weight fragments through per-wave LDS rings) or "resident"
    (16-ray workgroups, both sigma nets held in LDS) -- identical bits; auto
    takes the resident form where the batch fills the device (fwd_pick)."""
    form = L.fwd_form(FWD_FORM if form is None else form)   # refused on the host, before any launch
    L.require_device(rays, t_vals, t_rand, u, noise_c, noise_f, table, *ws)
    rays, t_vals, t_rand, u, noise_c, noise_f = (L.contig(t) for t in (rays, t_vals, t_rand, u,
                                                                      noise_c, noise_f))
    ws = [w.contiguous() for w in ws]
    B = rays.shape[0]
    dev = rays.device
    # the fine pass's tensors are sized by the cfg (64 + 128 samples, or 64 + 64)
    ni, nf = _fine_counts(cfg)
    for name, t, w in (("u", u, ni), ("noise_f", noise_f, nf)):
        if t is not None and (t.numel() != B * w or (t.dim() and t.shape[-1] != w)):
            raise ValueError(f"hashnerf_amd.render_fwd: {name} must be [{B}, {w}] for n_importance = {ni}, "
                             f"got {tuple(t.shape)}")
    if keep_feat and ni != 128 and L.lib().hn_render_scatter_mode(cfg, B) != 2:
        raise ValueError("hashnerf_amd.render_fwd: n_importance = 64 trains on the binned backward only "
                         "(hn_render_scatter_mode != 2 for this configuration)")
    e = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
    out = dict(rgb=e(B, 3), depth=e(B), acc=e(B), sparsity=e(B), rgb0=e(B, 3), depth0=e(B),
               acc0=e(B), sparsity0=e(B), z_std=e(B), z_coarse=e(B, 64), z_fine=e(B, nf),
               raw_c=e(B, 64, 4), raw_f=e(B, nf, 4))
    a = L.HnRenderFwdArgs()
    a.n_rays = B
    for k, t in (("rays", rays), ("t_vals", t_vals), ("t_rand", t_rand), ("u", u),
                 ("noise_c", noise_c), ("noise_f", noise_f), ("table", table)):
        setattr(a, k, None if t is None else t.data_ptr())
    a.coarse = L.make_mlp(ws[:5])
    a.fine = L.make_mlp(ws[5:])
    for k, t in out.items():
        setattr(a, k, t.data_ptr())
    fine_src = torch.empty((B, nf), dtype=torch.uint8, device=dev)
    a.fine_src = fine_src.data_ptr()
    # hash features of every evaluated point, kept for the backward only
    # when a gradient will be taken (inference skips the 32 KB/ray store)
    feat = torch.empty((B, L.RENDER_FEAT_PER_RAY) if keep_feat else (0,), dtype=torch.float32,
                       device=dev)
    a.feat = feat.data_ptr() if keep_feat else None
    wsb, nbytes = _caller_ws("render_fwd", wsb, L.lib().hn_render_workspace_bytes(cfg, B), dev)
    a.weights_packed = 1 if weights_packed else 0
    a.skip_dead_color = 1 if skip_dead_color else 0
    la = None
    if loss is not None:
        if not keep_feat:
            raise ValueError("hashnerf_amd.render_fwd: loss= is for a forward whose backward follows (keep_feat)")
        la, (target,) = _render_loss(loss, ("target",), ("world", "sparse_w"))
        if tuple(target.shape) != (B, 3):
            raise ValueError(f"hashnerf_amd.render_fwd: loss target must be [{B}, 3]")
        a.loss = C.pointer(la)
    t0 = TIMER.begin("render_fwd")
    L.check(L.lib().hn_render_fwd_form(cfg, a, form, L.ptr(wsb), nbytes, L.stream(dev)), "render_fwd")
    TIMER.end("render_fwd", t0)
    if DEBUG_KEEP:
        LAST.update({k: out[k] for k in ("z_coarse", "z_fine", "raw_c", "raw_f")})
    st = None
    if keep_feat:
        st = RenderState()
        st.cfg, st.rays, st.noise_c, st.noise_f, st.table, st.ws = cfg, rays, noise_c, noise_f, table, ws
        st.z_c, st.z_f, st.raw_c, st.raw_f = out["z_coarse"], out["z_fine"], out["raw_c"], out["raw_f"]
        st.fine_src, st.feat, st.wsb, st.nbytes = fine_src, feat, wsb, nbytes
        st.skip_dead = bool(skip_dead_color)
        if la is not None:
            st.prepass_done = _loss_key(loss)
            _PREPASS_ON_WS[wsb.data_ptr()] = weakref.ref(st)
    return out, st


# the upstream gradients a backward takes (hn_render_bwd_args' g_* fields)
_GRAD_NAMES = ("g_rgb", "g_depth", "g_acc", "g_sparsity", "g_rgb0", "g_depth0", "g_acc0", "g_sparsity0", "g_raw_f")


def _bwd_args(who, st: RenderState, grads: dict):
    """The hn_render_bwd_args of a saved state and its upstream gradients
    (missing = NULL) -- nets, g_*, rays, noise, table, z, raw, fine_src, feat
    -- and the list of the contiguous tensors it points at, which the caller
    keeps alive until its launch is queued."""
    g_raw_f = grads.get("g_raw_f")
    if g_raw_f is not None and g_raw_f.numel() != st.raw_f.numel():
        raise ValueError(f"hashnerf_amd.{who}: g_raw_f must be {tuple(st.raw_f.shape)} (the cfg's "
                         f"n_importance = {_fine_counts(st.cfg)[0]}), got {tuple(g_raw_f.shape)}")
    a = L.HnRenderBwdArgs()
    a.n_rays = st.rays.shape[0]
    a.coarse = L.make_mlp(st.ws[:5])
    a.fine = L.make_mlp(st.ws[5:])
    keep = []
    for k, t in [(n, grads.get(n)) for n in _GRAD_NAMES] + [
            ("rays", st.rays), ("noise_c", st.noise_c), ("noise_f", st.noise_f), ("table", st.table),
            ("z_coarse", st.z_c), ("z_fine", st.z_f), ("raw_c", st.raw_c), ("raw_f", st.raw_f)]:
        t = L.contig(t)
        keep.append(t)
        setattr(a, k, None if t is None else t.data_ptr())
    a.fine_src = st.fine_src.data_ptr()
    a.feat = st.feat.data_ptr()
    return a, keep


def render_bwd(st: RenderState, grads: dict, d_table, dws, overwrite: bool = False, table_step=None,
               overwrite_mlp: bool = False, tv=None, table_live=None, owner_defer: bool = False, loss=None,
               mlp_step=None, repack: bool = False, prepass_done: bool = False, next_batch=None):
    """hn_render_bwd: accumulates (+=) d loss / d table into d_table (or
    writes it, overwrite=True: d_table need not be zeroed) and the ten
    NeRFSmall weight gradients into dws (coarse 5, fine 5, +=; written with
    overwrite_mlp=True, dws need not be zeroed).  grads: any
    of g_rgb, g_depth, g_acc, g_sparsity, g_rgb0, g_depth0, g_acc0,
    g_sparsity0, g_raw_f (missing = 0).  table_step = (table, exp_avg,
    exp_avg_sq, coeffs) from RAdam.take_step: the binned owner pass applies
    that RAdam step to the table with this gradient (d_table may be None).
    tv = (min_vertex [L, 3] device int32, cubes, g_tv [L]) from tv_fwd and the
    loss backward: the TV term's table gradient (loss.py:11-43) joins this
    backward -- as records of the binned owner pass (so table_step stays
    fused), or added to d_table -- instead of a separate tv_bwd.
    table_live = (n_levels, int32 bitmap) from train.live_pair_mask, with
    table_step: the fused step skips the row pairs no gradient can reach
    (bitwise the same update, fewer optimizer-state bytes).
    owner_defer=True (binned scatter): the table gradient is not formed yet;
    render_bwd_owner(st, lo, hi) then writes bins [lo, hi) (render_bins
    gives their geometry), e.g. each range before its gradient exchange.
    loss (ABI 13, the trainer's step): dict(target [B, 3], out [4] device,
    rgb / rgb0 / sparsity / sparsity0 = the forward's outputs, tv [L] or
    None, world, sparse_w, tv_w) forms the training loss's upstream
    gradients in the backward itself (run_nerf.py:612-636 under
    train.dp_loss's rule; grads is not read) and writes out = loss, mse,
    mse0, entropy sum (loss_fwd's).
    mlp_step (binned scatter): the ten (p, exp_avg, exp_avg_sq, coeffs) of
    RAdam.take_step for st.ws's tensors, applied where each weight's final
    gradient is formed (the slab reduction; dws is still written); with
    repack=True the stepped weights' packed copies are then written into the
    workspace, for a next render_fwd(wsb=st.wsb, weights_packed=True).
    prepass_done=True (with loss): st's render_fwd ran with this loss, so d
    raw and the marks are in the workspace and no composite pre-pass is
    launched.  Refused here when st's forward did not (or another such
    forward has used the workspace since, or a backward has consumed it);
    the library checks the forward's stamp on the device as well (fault
    bit 128).
    next_batch = a NextBatch (functional.next_batch; binned scatter, no
    owner_defer): the next step's rays, targets and uniform draws are made by
    extra workgroups of this backward's lists and placement launches instead
    of the sampler's own two launches -- bitwise sample_rays' values, in
    next_batch.out once this call's launches have run."""
    B = st.rays.shape[0]
    dev = st.rays.device
    # (these refusals read rays, cfg, wsb, skip_dead and prepass_done only: a bare state gets them too)
    if prepass_done:
        if st.prepass_done is None:
            raise ValueError("hashnerf_amd.render_bwd: prepass_done needs a render_fwd(loss=...) of this state "
                             "that no backward has used yet")
        if loss is None:
            raise ValueError("hashnerf_amd.render_bwd: prepass_done needs the forward's loss")
        owner = _PREPASS_ON_WS.get(st.wsb.data_ptr())
        if owner is None or owner() is not st:
            raise ValueError("hashnerf_amd.render_bwd: prepass_done, but another render_fwd(loss=...) has used "
                             "this workspace since this state's")
        if st.prepass_done != _loss_key(loss):
            raise ValueError("hashnerf_amd.render_bwd: prepass_done, but the loss (target, world, sparse_w) "
                             "is not the one the forward took")
    if st.skip_dead:
        # only the binned dense_bwd = 0 backward runs lists of the tiles that were stored
        if st.cfg.dense_bwd:
            raise ValueError("hashnerf_amd.render_bwd: the forward ran with skip_dead_color (features of tiles "
                             "without density not stored); the backward needs cfg.dense_bwd = 0")
        if L.lib().hn_render_scatter_mode(st.cfg, B) != 2:
            raise ValueError("hashnerf_amd.render_bwd: the forward ran with skip_dead_color (features of tiles "
                             "without density not stored); the float-atomic backward this configuration runs "
                             "(hn_render_scatter_mode != 2) loads every tile")
    a, keep = _bwd_args("render_bwd", st, grads)
    if d_table is not None:
        if not d_table.is_contiguous():
            raise RuntimeError("hashnerf_amd.render_bwd: d_table must be contiguous")
        a.d_table = d_table.data_ptr()
        keep.append(d_table)
    a.weights_packed = 1               # same workspace and weights as the forward
    a.d_table_mode = (1 if overwrite else 0) | (2 if overwrite_mlp else 0)
    a.d_coarse = L.make_mlp_grad(dws[:5])
    a.d_fine = L.make_mlp_grad(dws[5:])
    step = None
    if table_step is not None:
        p, m, v, c = table_step
        L.require_device(p, m, v)
        step = _radam_fill(L.HnRadamTensor(), p, None, m, v, c)
        a.table_step = C.pointer(step)
        if table_live is not None:
            n_lv, words = table_live
            if not words.is_cuda or words.dtype != torch.int32 or not words.is_contiguous() or \
                    words.numel() < (n_lv << st.cfg.grid.log2_hashmap_size) // 64:
                raise ValueError("hashnerf_amd.render_bwd: table_live must be a contiguous device int32 "
                                 "bitmap of n_levels << (T - 6) words")
            keep.append(words)
            a.table_live = words.data_ptr()
            a.table_live_levels = n_lv
    if tv is not None:
        mv, cubes, g_tv = tv
        tva = _tv_args(st.table, mv, cubes, st.cfg.grid.log2_hashmap_size)
        keep.append(tva)
        a.tv = C.cast(C.pointer(tva), C.c_void_p)
        g_tv = g_tv.contiguous()
        keep.append(g_tv)
        a.g_tv = g_tv.data_ptr()
    a.owner_defer = 1 if owner_defer else 0
    if mlp_step is not None:
        if len(mlp_step) != 10:
            raise ValueError("hashnerf_amd.render_bwd: mlp_step needs the ten NeRFSmall tensors' steps")
        ms = (L.HnRadamTensor * 10)()
        for d, (p, m, v, c), w in zip(ms, mlp_step, st.ws):
            if p.data_ptr() != w.data_ptr():
                raise ValueError("hashnerf_amd.render_bwd: mlp_step must follow the render's weights in order")
            L.require_device(p, m, v)
            _radam_fill(d, p, None, m, v, c)
        a.mlp_step = ms
        a.repack = 1 if repack else 0
        keep.append(ms)
    if loss is not None:
        la, ts = _render_loss(loss, ("target", "rgb", "rgb0", "sparsity", "sparsity0"), ("world", "sparse_w", "tv_w"))
        ltv = L.contig(loss.get("tv"))
        L.require_device(ltv, loss["out"])
        la.tv, la.n_tv = (ltv.data_ptr(), ltv.numel()) if ltv is not None else (None, 0)
        la.out = loss["out"].data_ptr()
        a.loss = C.pointer(la)
        keep += ts + [ltv, la]
    if next_batch is not None:
        a.next_batch = C.pointer(next_batch.job)
        keep.append(next_batch)
    if prepass_done:
        a.prepass_done = 1
        st.prepass_done = None   # the backward clears the forward's stamp
    t0 = TIMER.begin("render_bwd")
    next_ndc = None if next_batch is None else next_batch.ndc
    L.check(L.lib().hn_render_bwd_ndc(st.cfg, a, L.ptr(st.wsb), st.nbytes, next_ndc, L.stream(dev)),
            _ndc_label("render_bwd", next_ndc))
    TIMER.end("render_bwd", t0)
    # the deferred owner pass reuses these arguments (and the buffers they point to)
    st.bwd_args = (a, keep, step) if owner_defer else None
    if CHECK_FAULTS and not owner_defer:
        L.check_device_faults()


def render_bins(cfg, n_rays: int):
    """(number of bins, log2 table entries per bin) of the binned scatter
    (hn_render_bins); (0, 0) for the float-atomic schedule."""
    shift = C.c_int32(0)
    n = L.lib().hn_render_bins(cfg, n_rays, C.byref(shift))
    return int(n), int(shift.value)


def fwd_pick(n_rays: int):
    """(form, compute units): the form render_fwd's "auto" runs for n_rays on
    the current device (hn_render_fwd_pick: "resident" where ceil(n_rays / 16)
    reaches the device's compute units, else "ring"), and the count that rule
    was stated against."""
    cus = C.c_int32(0)
    form = L.lib().hn_render_fwd_pick(int(n_rays), C.byref(cus))
    return {v: k for k, v in L.FWD_FORMS.items()}[int(form)], int(cus.value)


def render_bwd_owner(st: RenderState, bin_lo: int, bin_hi: int):
    """hn_render_bwd_owner: the owner pass of a render_bwd(owner_defer=True)
    over bins [bin_lo, bin_hi) -- their slices of d_table written (or
    stepped, with table_step)."""
    if st.bwd_args is None:
        raise RuntimeError("hashnerf_amd.render_bwd_owner: needs a render_bwd(owner_defer=True) first")
    a = st.bwd_args[0]
    L.check(L.lib().hn_render_bwd_owner(st.cfg, a, L.ptr(st.wsb), st.nbytes, bin_lo, bin_hi,
                                        L.stream(st.rays.device)), "render_bwd_owner")
    if CHECK_FAULTS:
        L.check_device_faults()


def zeros_like_all(ts):
    """Zeroed tensors shaped like ts, views of ONE flat buffer (one fill)."""
    n = sum(t.numel() for t in ts)
    flat = torch.zeros(n, dtype=torch.float32, device=ts[0].device)
    out, off = [], 0
    for t in ts:
        out.append(flat[off:off + t.numel()].view_as(t))
        off += t.numel()
    return out


def render_bwd_rays(st: RenderState, grads: dict) -> torch.Tensor:
    """hn_render_bwd_rays: d loss / d rays [B, 11] of the fused forward that left
    st, from its saved z values, raw outputs and ReLU masks -- columns 0:3 d o,
    3:6 d d, 8:11 d viewdir; 6:8 (near, far) are written as zeros: no gradient
    is formed for them.  grads as render_bwd's (missing = 0).  The importance
    samples are detached, as in the reference, so no gradient flows through
    z.  Runs on a scratch of its own: st's workspace is untouched, and
    render_bwd(st, ...) may run before or after; neither a table gradient nor
    an MLP-weight gradient is formed here.  Bitwise repeatable."""
    B = st.rays.shape[0]
    dev = st.rays.device
    a, keep = _bwd_args("render_bwd_rays", st, grads)
    L.require_device(*keep)
    d_rays = torch.empty((B, 11), dtype=torch.float32, device=dev)
    nbytes = L.lib().hn_render_bwd_rays_workspace_bytes(st.cfg, B)
    scratch = _ws(nbytes, dev)
    t0 = TIMER.begin("render_bwd_rays")
    L.check(L.lib().hn_render_bwd_rays(st.cfg, a, L.ptr(scratch), nbytes, L.ptr(d_rays), L.stream(dev)),
            "render_bwd_rays")
    TIMER.end("render_bwd_rays", t0)
    if CHECK_FAULTS:
        L.check_device_faults()
    return d_rays


class RenderRaysFn(torch.autograd.Function):
    """Inputs: rays [B,11], t_vals [64], t_rand [B,64]|None, u [B,cfg.n_importance],
    noise_c/noise_f |None, table, 5 coarse + 5 fine NeRFSmall weights.
    Outputs: rgb, depth, acc, sparsity, rgb0, depth0, acc0, sparsity0, z_std, raw.
    The backward launches only what needs_input_grad asks for: render_bwd (table
    and weight gradients) where a table or weight requires grad, render_bwd_rays
    where the rays do and the caller opted in (RenderRaysGradFn) -- a frozen field
    under pose refinement allocates no table gradient and launches no MLP-weight
    or scatter work."""

    @staticmethod
    def forward(ctx, cfg: L.HnRenderCfg, keep_feat: bool, rays, t_vals, t_rand, u, noise_c, noise_f,
                table, *ws):
        out, st = render_fwd(cfg, rays, t_vals, t_rand, u, noise_c, noise_f, table, ws, keep_feat)
        ctx.st = st
        ctx.ray_grad = False               # RenderRaysGradFn: the caller opted in to d rays
        ctx.set_materialize_grads(False)   # unused outputs => NULL, not zeros (0*inf)
        ctx.mark_non_differentiable(out["z_std"])
        return (out["rgb"], out["depth"], out["acc"], out["sparsity"], out["rgb0"], out["depth0"],
                out["acc0"], out["sparsity0"], out["z_std"], out["raw_f"])

    @staticmethod
    def backward(ctx, g_rgb, g_depth, g_acc, g_sp, g_rgb0, g_depth0, g_acc0, g_sp0, _g_zstd, g_raw):
        st = ctx.st
        if st is None:
            raise RuntimeError("hashnerf_amd.render_rays: forward ran without keeping features "
                               "(no input required grad)")
        grads = dict(g_rgb=g_rgb, g_depth=g_depth, g_acc=g_acc, g_sparsity=g_sp, g_rgb0=g_rgb0,
                     g_depth0=g_depth0, g_acc0=g_acc0, g_sparsity0=g_sp0, g_raw_f=g_raw)
        # inputs: cfg, keep_feat, rays, t_vals, t_rand, u, noise_c, noise_f, table, the ten weights
        need = ctx.needs_input_grad
        d_rays = render_bwd_rays(st, grads) if need[2] and ctx.ray_grad else None
        d_table, dws = None, [None] * len(st.ws)
        if any(need[8:]):
            d_table = torch.zeros_like(st.table)
            dws = zeros_like_all(st.ws)
            render_bwd(st, grads, d_table, dws)
        ctx.st = None
        return (None, None, d_rays, None, None, None, None, None, d_table, *dws)


class RenderRaysGradFn(RenderRaysFn):
    """RenderRaysFn whose backward also forms d rays (render_bwd_rays) where the
    rays require grad: render_rays_fused(..., ray_grad=True).  RenderRaysFn
    itself returns None for the rays and launches nothing for them, as before."""

    @staticmethod
    def forward(ctx, *args):
        out = RenderRaysFn.forward(ctx, *args)
        ctx.ray_grad = True
        return out


# --------------------------------------------------------------------------
# training-step driver (run_nerf.py:576-636)
# --------------------------------------------------------------------------
def _uniform_draws(shapes, dev):
    """torch.rand(shape, device=dev) for each shape, as hn_uniform_draw
    records: the default generator's seed, each draw's philox offset and
    torch's thread count for its size (ATen calc_execution_policy: 256-thread
    blocks, at most CUs x 2048 / 256 of them, 4 values per thread and call);
    the generator is advanced as the torch.rand calls would advance it.
    Returns (seed, ctypes array, output tensors)."""
    if len(shapes) > L.UNIFORM_MAX_DRAWS:
        raise ValueError(f"hashnerf_amd: at most {L.UNIFORM_MAX_DRAWS} uniform draws per launch")
    dev = torch.device(dev)
    torch.cuda.init()                          # default_generators is filled lazily
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    gen = torch.cuda.default_generators[idx]
    props = _DEV_PROPS.get(idx)
    if props is None:
        p = torch.cuda.get_device_properties(idx)
        props = _DEV_PROPS[idx] = (p.multi_processor_count,
                                   getattr(p, "max_threads_per_multi_processor", 2048))
    max_blocks = props[0] * (props[1] // 256)
    seed, off = gen.initial_seed(), gen.get_offset()
    arr = (L.HnUniformDraw * len(shapes))()
    outs = []
    for d, shape in zip(arr, shapes):
        t = torch.empty(shape, dtype=torch.float32, device=dev)
        n = t.numel()
        threads = 256 * min((n + 255) // 256, max_blocks)
        d.out, d.numel, d.threads, d.offset = t.data_ptr(), n, max(threads, 1), off
        if n:
            off += ((n - 1) // (threads * 4) + 1) * 4
        outs.append(t)
    gen.set_offset(off)
    return seed & ((1 << 64) - 1), arr, outs


_DEV_PROPS = {}


def torch_uniform(shapes, dev):
    """torch.rand(shape, device=dev) for every shape, bitwise, in one HIP
    launch (hn_uniform_philox); the default generator ends where the torch.rand
    calls would leave it."""
    seed, arr, outs = _uniform_draws(shapes, dev)
    L.check(L.lib().hn_uniform_philox(seed, arr, len(shapes), L.stream(torch.device(dev))), "uniform_philox")
    return outs


def ndc_scalars(H, W, focal):
    """get_ndc_rays' two Python scalars (ray_util.py:131-136) as float64:
    -1. / (W / (2. * focal)) and -1. / (H / (2. * focal)), focal = K[0][0] --
    what _render_views puts into hn_view_args.ndc_sx / ndc_sy."""
    focal = float(focal)
    return -1. / (W / (2. * focal)), -1. / (H / (2. * focal))


def _ray_ndc(who, ndc):
    """A sampler's ``ndc`` argument as an hn_ray_ndc: None (world rays: the
    call as it is without), or (H, W, focal) of render()'s
    get_ndc_rays(H, W, K[0][0], 1., ...).  Refused here, before any library
    call: anything but three numbers, a size below 1, a focal length that is
    not positive and finite."""
    if ndc is None:
        return None
    if isinstance(ndc, (str, bytes)) or not hasattr(ndc, "__len__") or len(ndc) != 3:
        raise ValueError(f"{who}: ndc must be None or (H, W, focal), got {ndc!r}")
    H, W, focal = (float(v) for v in ndc)
    if not (H >= 1 and W >= 1 and math.isfinite(H) and math.isfinite(W)):
        raise ValueError(f"{who}: ndc image size {ndc[0]!r} x {ndc[1]!r}")
    if not (focal > 0. and math.isfinite(focal)):
        raise ValueError(f"{who}: ndc focal length {ndc[2]!r} must be positive and finite")
    n = L.HnRayNdc()
    n.sx, n.sy = ndc_scalars(ndc[0], ndc[1], focal)
    return n


def _ndc_label(name, nd):
    """L.check's label of an entry point taking an hn_ray_ndc: the call's name
    without one (ndc == NULL is that call, bit for bit), else its _ndc name."""
    return name if nd is None else name + "_ndc"


def _ray_sampler(image, c2w, K, near, far, crop, seed):
    """The hn_ray_sampler of one image and window, and the contiguous image and
    [3, 4] pose it is used with."""
    L.require_device(image, c2w)
    image, c2w = image.contiguous(), c2w[:3, :4].contiguous()
    s = L.HnRaySampler()
    s.H, s.W = image.shape[0], image.shape[1]
    s.crop_y0, s.crop_x0, s.crop_h, s.crop_w = (int(v) for v in crop)
    s.fx, s.fy, s.cx, s.cy = float(K[0][0]), float(K[1][1]), float(K[0][2]), float(K[1][2])
    s.near, s.far = float(near), float(far)
    s.seed = int(seed) & ((1 << 64) - 1)
    return s, image, c2w


def _batch_out(n_rays, dev):
    """The [n, 11] rays and [n, 3] target a sampler fills."""
    return (torch.empty((n_rays, 11), dtype=torch.float32, device=dev),
            torch.empty((n_rays, 3), dtype=torch.float32, device=dev))


class NextBatch:
    """sample_rays(order=1, uniforms=...) as a job of render_bwd
    (hn_render_bwd_args.next_batch): ``job`` the hn_next_batch, ``out`` =
    (rays, target, *uniform tensors) that the backward's launches fill."""
    __slots__ = ("job", "out", "keep", "ndc")   # ndc: the job's hn_ray_ndc (hn_render_bwd_ndc), or None


def _morton_job(who, image, c2w, n_rays, K, near, far, crop, seed, uniforms, nd):
    """sample_rays(order=1)'s call as a NextBatch: the hn_ray_sampler, the
    outputs, the Morton sampler's scratch and the uniform draws (the default
    generator advanced as the torch.rand calls would advance it), nothing
    launched.  nd: _ray_ndc's result."""
    s, image, c2w = _ray_sampler(image, c2w, K, near, far, crop, seed)
    nb = L.lib().hn_sample_rays_morton_workspace_bytes(s)
    if nb == 0:
        raise ValueError(f"{who}: window {s.crop_h}x{s.crop_w} too large")
    dev = image.device
    rays, target = _batch_out(n_rays, dev)
    ws = _sampler_ws(dev, nb)
    useed, arr, outs = _uniform_draws(uniforms, dev) if uniforms else (0, None, [])
    j = L.HnNextBatch()
    j.sampler = C.pointer(s)
    j.image, j.c2w, j.n_rays = image.data_ptr(), c2w.data_ptr(), n_rays
    j.rays, j.target = rays.data_ptr(), target.data_ptr()
    j.workspace, j.ws_bytes = ws.data_ptr(), nb
    j.seed, j.n_draws = useed, len(outs)
    if arr is not None:
        j.draws = arr
    b = NextBatch()
    b.job, b.out, b.keep, b.ndc = j, (rays, target, *outs), (s, image, c2w, ws, arr), nd
    return b


def next_batch(image, c2w, n_rays, K, near, far, crop, seed, uniforms=None, ndc=None):
    """The host half of sample_rays(image, ..., order=1, uniforms=uniforms,
    ndc=ndc): the sampler's arguments, the output tensors and the default
    generator's philox offsets (advanced as the torch.rand calls would),
    without the launches.  render_bwd(next_batch=...) of the binned schedule
    runs the device half inside its own two small launches, bitwise the values
    sample_rays would return."""
    return _morton_job("next_batch", image, c2w, n_rays, K, near, far, crop, seed, uniforms,
                       _ray_ndc("next_batch", ndc))


def sample_rays(image, c2w, n_rays, K, near, far, crop, seed, order=1, uniforms=None, ndc=None):
    """N_rand distinct pixels of one image (device, no replacement) -> the
    [n, 11] ray batch render() builds and the [n, 3] target colours.
    image [H, W, 3], c2w [3, 4] (or [4, 4]) fp32 on the device; crop =
    (y0, x0, h, w) sampling window; K the 3x3 intrinsics (host numbers).
    order=1 (hn_sample_rays_morton) lists the same drawn set in Morton order
    of its pixels -- the batch order changes the loss and its gradient only
    by float summation order -- so the fused forward's XCD-contiguous ray
    groups are spatially coherent; order=0 (hn_sample_rays) keeps the draw
    order.  Both are deterministic for a given seed.  uniforms: shapes of
    torch.rand draws to make as well (torch_uniform; with order=1 in the
    sampler's first launch), returned after rays and target.  ndc = (H, W,
    focal): rays[:, 0:6] are render()'s NDC rays of the drawn pixels
    (get_ndc_rays(H, W, focal, 1., o, d) bit for bit, formed in the same
    launch); near, far, the view direction (the world ray's, normalised) and
    the target are those of the call without."""
    if order not in (0, 1):
        raise ValueError(f"sample_rays: order {order!r}")
    nd = _ray_ndc("sample_rays", ndc)
    if order == 1:
        b = _morton_job("sample_rays(order=1)", image, c2w, n_rays, K, near, far, crop, seed, uniforms, nd)
        j = b.job
        L.check(L.lib().hn_sample_batch_morton_ndc(j.sampler, j.image, j.c2w, j.n_rays, j.rays, j.target, j.workspace,
                                                   j.ws_bytes, j.seed, j.draws, j.n_draws, nd, L.stream(image.device)),
                _ndc_label("sample_batch_morton" if uniforms else "sample_rays_morton", nd))
        return b.out
    s, image, c2w = _ray_sampler(image, c2w, K, near, far, crop, seed)
    dev = image.device
    rays, target = _batch_out(n_rays, dev)
    L.check(L.lib().hn_sample_rays_ndc(s, L.ptr(image), L.ptr(c2w), n_rays, L.ptr(rays), L.ptr(target), nd,
                                       L.stream(dev)), _ndc_label("sample_rays", nd))
    if uniforms:
        return (rays, target, *torch_uniform(uniforms, dev))
    return rays, target


POOL_ORDER_MAX = L.POOL_ORDER_MAX


def sample_pool(images, poses, image_ids, K, near, far, seed, start, n_rays, order=0, box=None, uniforms=None,
                return_keys=False, ndc=None):
    """use_batching draw (run_nerf.py:505-521, 544-555): pool positions
    [start, start + n_rays) of the epoch whose shuffle key is `seed`, as the
    [n, 11] ray batch and [n, 3] targets (hn_sample_pool).  images [N, H, W, 3]
    and poses [N, 3|4, 4] on the device; image_ids the training image indices
    (device int32); K the 3x3 intrinsics (host numbers, used in float64).
    order=1 (hn_sample_pool_ordered; at most POOL_ORDER_MAX rays) lists the
    same rays, bitwise, in Morton order of their mid-depth points inside
    box = (min, max), the hash grid's box; positions with equal keys keep the
    shuffle's order.  uniforms: shapes of torch.rand draws to make as well
    (with order=1 in the same launch, else torch_uniform), returned after rays
    and target; return_keys (order=1) appends the rows' int32 keys.  ndc =
    (H, W, focal): the rays' NDC step as in sample_rays; order=1 then keys the
    NDC rays (mid-depth of `near`, `far`: 0.5 for an LLFF pool) in `box`, the
    NDC box."""
    if order not in (0, 1):
        raise ValueError(f"sample_pool: order {order!r}")
    nd = _ray_ndc("sample_pool", ndc)
    if order == 0 and return_keys:
        raise ValueError("sample_pool: return_keys needs order=1")
    if order == 1:
        if box is None:
            raise ValueError("sample_pool(order=1) needs box=(min, max), the hash grid's box")
        if n_rays > L.POOL_ORDER_MAX:
            raise ValueError(f"sample_pool(order=1): {n_rays} rays, at most {L.POOL_ORDER_MAX} per call")
    L.require_device(images, poses)
    images, poses = images.contiguous(), poses.contiguous()
    if image_ids.dtype != torch.int32 or not image_ids.is_cuda:
        raise TypeError("hashnerf_amd.sample_pool: image_ids must be a device int32 tensor")
    p = L.HnRayPool()
    p.n_images = int(image_ids.numel())
    p.H, p.W = int(images.shape[1]), int(images.shape[2])
    p.pose_stride = int(poses.shape[1] * poses.shape[2])
    p.fx, p.fy, p.cx, p.cy = float(K[0][0]), float(K[1][1]), float(K[0][2]), float(K[1][2])
    p.near, p.far = float(near), float(far)
    p.seed = int(seed) & ((1 << 64) - 1)
    dev = images.device
    rays, target = _batch_out(n_rays, dev)
    ids = image_ids.contiguous()
    if order == 1:
        bmin = (C.c_float * 3)(*(float(v) for v in box[0]))
        bmax = (C.c_float * 3)(*(float(v) for v in box[1]))
        keys = torch.empty((n_rays,), dtype=torch.int32, device=dev) if return_keys else None
        useed, arr, outs = _uniform_draws(uniforms, dev) if uniforms else (0, None, [])
        L.check(L.lib().hn_sample_pool_ordered_ndc(p, L.ptr(images), L.ptr(poses), L.ptr(ids), int(start),
                                                   int(n_rays), bmin, bmax, L.ptr(rays), L.ptr(target), L.ptr(keys),
                                                   useed, arr, len(outs), nd, L.stream(dev)),
                _ndc_label("sample_pool_ordered", nd))
        return (rays, target, *outs, keys) if return_keys else (rays, target, *outs)
    L.check(L.lib().hn_sample_pool_ndc(p, L.ptr(images), L.ptr(poses), L.ptr(ids), int(start), int(n_rays),
                                       L.ptr(rays), L.ptr(target), nd, L.stream(dev)), _ndc_label("sample_pool", nd))
    if uniforms:
        return (rays, target, *torch_uniform(uniforms, dev))
    return rays, target


BLENDER_MODES = {"rgba": 0, "white": 1, "rgb": 2}


def blender_images(rgba_u8, half_res=False, mode="rgba"):
    """hn_blender_images: uint8 RGBA [n, H, W, 4] on the device -> float32
    images as load/load_blender.py:63-86 (/ 255., half_res INTER_AREA) and,
    mode="white" / "rgb", run_nerf.py:259-262's composite / channel cut."""
    if not rgba_u8.is_cuda or rgba_u8.dtype != torch.uint8 or rgba_u8.dim() != 4 or rgba_u8.shape[-1] != 4:
        raise TypeError("hashnerf_amd.blender_images: expects a device uint8 tensor [n, H, W, 4]")
    n, H, W, _ = rgba_u8.shape
    Ho, Wo = (H // 2, W // 2) if half_res else (H, W)
    m = BLENDER_MODES[mode]
    out = torch.empty((n, Ho, Wo, 4 if m == 0 else 3), dtype=torch.float32, device=rgba_u8.device)
    L.check(L.lib().hn_blender_images(L.ptr(rgba_u8.contiguous()), n, H, W, int(bool(half_res)), m, L.ptr(out),
                                      L.stream(rgba_u8.device)), "blender_images")
    return out


_SAMPLER_WS = {}


def _sampler_ws(dev, nbytes):
    """Scratch of the Morton sampler (block counts), grown on demand: one per
    (device, stream), so a batch drawn ahead on a side stream
    (Trainer.prefetch) never shares it with a draw on the current stream
    (ADVICE r05)."""
    key = (dev, torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else 0)
    ws = _SAMPLER_WS.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        _SAMPLER_WS[key] = ws
    return ws


def loss_fwd(rgb, rgb0, target, sp, sp0, tv, world, sparse_w, tv_w):
    """hn_loss_fwd -> device [4] = loss, mse, mse0, sum of entropies."""
    L.require_device(rgb, target, sp)
    n = rgb.shape[0]
    out = torch.empty(4, dtype=torch.float32, device=rgb.device)
    L.check(L.lib().hn_loss_fwd(L.ptr(L.contig(rgb)), L.ptr(L.contig(rgb0)), L.ptr(L.contig(target)),
                                L.ptr(L.contig(sp)), L.ptr(L.contig(sp0)), n, L.ptr(L.contig(tv)),
                                0 if tv is None else tv.numel(), float(world), float(sparse_w),
                                float(tv_w), L.ptr(out), L.stream(rgb.device)), "loss_fwd")
    return out


def _loss_grads(rgb, has_rgb0, has_sp0, n_tv):
    """The tensors hn_loss_bwd / hn_loss_fwd_bwd write: (g_rgb, g_rgb0, g_sp,
    g_sp0, g_tv), None for a term the loss does not have."""
    e = lambda n: torch.empty(n, dtype=torch.float32, device=rgb.device)
    return (torch.empty_like(rgb), torch.empty_like(rgb) if has_rgb0 else None, e(rgb.shape[0]),
            e(rgb.shape[0]) if has_sp0 else None, e(n_tv) if n_tv else None)


def loss_bwd(rgb, rgb0, target, n_tv, world, sparse_w, tv_w, g_loss, has_sp0=True):
    """hn_loss_bwd -> (g_rgb, g_rgb0, g_sp, g_sp0, g_tv) for upstream g_loss (device scalar)."""
    n = rgb.shape[0]
    dev = rgb.device
    g_rgb, g_rgb0, g_sp, g_sp0, g_tv = _loss_grads(rgb, rgb0 is not None, has_sp0, n_tv)
    L.check(L.lib().hn_loss_bwd(L.ptr(L.contig(rgb)), L.ptr(L.contig(rgb0)), L.ptr(L.contig(target)), n,
                                n_tv, float(world), float(sparse_w), float(tv_w), L.ptr(g_loss.contiguous()),
                                L.ptr(g_rgb), L.ptr(g_rgb0), L.ptr(g_sp), L.ptr(g_sp0), L.ptr(g_tv),
                                L.stream(dev)), "loss_bwd")
    return g_rgb, g_rgb0, g_sp, g_sp0, g_tv


def loss_fwd_bwd(rgb, rgb0, target, sp, sp0, tv, world, sparse_w, tv_w, g_loss):
    """hn_loss_fwd_bwd: loss_fwd and loss_bwd in one launch -> (out [4],
    (g_rgb, g_rgb0, g_sp, g_sp0, g_tv)), bitwise the two calls' results."""
    L.require_device(rgb, target, sp)
    n = rgb.shape[0]
    dev = rgb.device
    n_tv = 0 if tv is None else tv.numel()
    out = torch.empty(4, dtype=torch.float32, device=dev)
    g_rgb, g_rgb0, g_sp, g_sp0, g_tv = _loss_grads(rgb, rgb0 is not None, sp0 is not None, n_tv)
    L.check(L.lib().hn_loss_fwd_bwd(L.ptr(L.contig(rgb)), L.ptr(L.contig(rgb0)), L.ptr(L.contig(target)),
                                    L.ptr(L.contig(sp)), L.ptr(L.contig(sp0)), n, L.ptr(L.contig(tv)), n_tv,
                                    float(world), float(sparse_w), float(tv_w), L.ptr(out),
                                    L.ptr(g_loss.contiguous()), L.ptr(g_rgb), L.ptr(g_rgb0), L.ptr(g_sp),
                                    L.ptr(g_sp0), L.ptr(g_tv), L.stream(dev)), "loss_fwd_bwd")
    return out, (g_rgb, g_rgb0, g_sp, g_sp0, g_tv)


class TrainLossFn(torch.autograd.Function):
    """loss = (mse(rgb) + mse(rgb0)) / world + sparse_w * (sum sp + sum sp0) +
    tv_w * sum tv (run_nerf.py:612-636 under train.dp_loss's DP rule).
    Returns (loss, mse, mse0); mse/mse0 carry no gradient."""

    @staticmethod
    def forward(ctx, rgb, rgb0, target, sp, sp0, tv, world, sparse_w, tv_w):
        out = loss_fwd(rgb, rgb0, target, sp, sp0, tv, world, sparse_w, tv_w)
        ctx.save_for_backward(rgb, rgb0 if rgb0 is not None else rgb, target)
        ctx.has = (rgb0 is not None, sp0 is not None)
        ctx.n_tv = 0 if tv is None else tv.numel()
        ctx.consts = (float(world), float(sparse_w), float(tv_w))
        mse, mse0 = out[1], out[2]
        ctx.mark_non_differentiable(mse, mse0)
        return out[0], mse, mse0

    @staticmethod
    def backward(ctx, g_loss, _g_mse, _g_mse0):
        rgb, rgb0, target = ctx.saved_tensors
        has0, has_sp0 = ctx.has
        g = g_loss if g_loss is not None else torch.ones((), device=rgb.device)
        g_rgb, g_rgb0, g_sp, g_sp0, g_tv = loss_bwd(rgb, rgb0 if has0 else None, target, ctx.n_tv,
                                                    *ctx.consts, g, has_sp0)
        return g_rgb, g_rgb0, None, g_sp, g_sp0, g_tv, None, None, None


def train_loss(rgb, rgb0, target, sp, sp0, tv=None, world=1, sparse_w=0.0, tv_w=0.0):
    return TrainLossFn.apply(rgb, rgb0, target, sp, sp0, tv, world, sparse_w, tv_w)


def _tv_args(table, mv, cubes, log2T):
    a = L.HnTvArgs()
    a.n_levels = table.shape[0]
    a.log2_hashmap_size = int(log2T)
    for l, c in enumerate(cubes):
        a.cube[l] = int(c)
    a.min_vertex = mv.data_ptr()
    a.table = table.data_ptr()
    return a


def tv_fwd(table, min_vertex, cubes, log2T):
    """hn_tv_fwd: per-level TV values [L]; returns (tv, device min vertices)."""
    L.require_device(table)
    mv = min_vertex.to(dtype=torch.int32).contiguous()
    if mv.device.type == "cpu":            # no host stall: pinned + async copy
        mv = mv.pin_memory().to(table.device, non_blocking=True)
    else:
        mv = mv.to(table.device)
    tv = torch.empty(table.shape[0], dtype=torch.float32, device=table.device)
    L.check(L.lib().hn_tv_fwd(_tv_args(table, mv, cubes, log2T), L.ptr(tv), L.stream(table.device)),
            "tv_fwd")
    return tv, mv


def tv_bwd(table, mv, cubes, log2T, g_tv, dtable):
    """hn_tv_bwd: dtable += sum_l g_tv[l] d tv_l / d table."""
    g = g_tv.contiguous()
    L.check(L.lib().hn_tv_bwd(_tv_args(table, mv, cubes, log2T), L.ptr(g), L.ptr(dtable),
                              L.stream(table.device)), "tv_bwd")


def tv_bwd_records(cfg, table, mv, cubes, g_tv, d_table, wsb=None):
    """hn_render_bwd with no rays and a TV term (ABI 14): d_table = sum_l
    g_tv[l] d tv_l / d table (every entry written) through the binned
    scatter's TV records and exact owner pass -- bitwise reproducible, where
    tv_bwd's float atomics are not.  For a data-parallel rank that drew no
    rays (train.Trainer._empty_rank_grads).  wsb: workspace of >=
    hn_render_workspace_bytes(cfg, 0) bytes (default a fresh one)."""
    L.require_device(table, g_tv, d_table)
    if mv.device != table.device or mv.dtype != torch.int32 or not mv.is_contiguous():
        raise ValueError("hashnerf_amd.tv_bwd_records: min vertices must be tv_fwd's contiguous device int32 tensor")
    if not d_table.is_contiguous() or d_table.shape != table.shape:
        raise ValueError("hashnerf_amd.tv_bwd_records: d_table must be a contiguous tensor shaped like the table")
    nbytes = L.lib().hn_render_workspace_bytes(cfg, 0)
    if wsb is None or _ws_size(wsb) < nbytes:   # (a workspace too small is replaced, not refused)
        wsb = _ws(nbytes, table.device)
    a = L.HnRenderBwdArgs()
    a.n_rays = 0
    tva = _tv_args(table, mv, cubes, cfg.grid.log2_hashmap_size)
    a.tv = C.cast(C.pointer(tva), C.c_void_p)
    g = g_tv.contiguous()
    a.g_tv = g.data_ptr()
    a.d_table = d_table.data_ptr()
    a.d_table_mode = 1
    L.check(L.lib().hn_render_bwd(cfg, a, L.ptr(wsb), _ws_size(wsb), L.stream(table.device)), "render_bwd (TV only)")
    if CHECK_FAULTS:
        L.check_device_faults()
    return wsb


class TVFn(torch.autograd.Function):
    """Per-level hash-table TV (loss.py:11-43) for all levels in one launch."""

    @staticmethod
    def forward(ctx, table, min_vertex, cubes, log2T):
        tv, mv = tv_fwd(table, min_vertex, cubes, log2T)
        ctx.save_for_backward(table, mv)
        ctx.cubes, ctx.log2T = list(cubes), int(log2T)
        return tv

    @staticmethod
    def backward(ctx, g_tv):
        table, mv = ctx.saved_tensors
        dtable = torch.zeros_like(table)
        tv_bwd(table, mv, ctx.cubes, ctx.log2T, g_tv, dtable)
        return dtable, None, None, None


def _radam_fill(d, p, g, m, v, c):
    """One HnRadamTensor: the tensors' pointers (g None: a fused step, which
    forms the gradient itself) and the nine coefficients of dict c."""
    d.p, d.g, d.m, d.v = p.data_ptr(), None if g is None else g.data_ptr(), m.data_ptr(), v.data_ptr()
    d.n = p.numel()
    for k in ("beta1", "beta2", "one_minus_beta1", "one_minus_beta2", "eps", "neg_wd_lr", "neg_step_lr",
              "mode", "has_wd"):
        setattr(d, k, c[k])
    return d


def _radam_array(tensors, name):
    arr = (L.HnRadamTensor * len(tensors))()
    for d, (p, g, m, v, c) in zip(arr, tensors):
        L.require_device(p, g, m, v)
        for t in (p, g, m, v):
            if not t.is_contiguous():
                raise RuntimeError(f"hashnerf_amd.{name}: tensors must be contiguous")
        _radam_fill(d, p, g, m, v, c)
    return arr


def radam_step(tensors):
    """tensors: list of (p, g, m, v, coeff dict); one HIP launch per 16 tensors."""
    for i in range(0, len(tensors), L.RADAM_MAX_TENSORS):
        chunk = tensors[i:i + L.RADAM_MAX_TENSORS]
        arr = _radam_array(chunk, "radam_step")
        L.check(L.lib().hn_radam_step(arr, len(chunk), L.stream(chunk[0][0].device)), "radam_step")


SCATTER_MODES = {"auto": 0, "atomic": 1, "binned": 2}


def make_render_cfg(grid: L.HnGrid, white_bkgd: bool, lindisp: bool, perturb: bool,
                    n_samples: int = 64, n_importance: int = 128, scatter: str = "auto",
                    dense_bwd: bool = False) -> L.HnRenderCfg:
    """hn_render_cfg.  scatter: the backward's table-gradient scatter --
    "binned" (records + exact per-bin owner pass), "atomic" (float atomics),
    "auto" (binned where the table allows it: T <= 22).  dense_bwd: compute
    the backward of every sample, also those whose d raw is exactly zero
    (relu(sigma) = 0), which the default skips (ABI 14; same results up to
    the sign of zero)."""
    c = L.HnRenderCfg()
    c.grid = grid
    c.n_samples, c.n_importance = n_samples, n_importance
    c.white_bkgd, c.lindisp, c.perturb = int(white_bkgd), int(lindisp), int(perturb)
    c.scatter = SCATTER_MODES[scatter]
    c.dense_bwd = int(bool(dense_bwd))
    return c


def _render_views(name, cfg, H, W, K, poses, near, far, table, ws, ndc, t_vals, u, wsb, weights_packed, return_rays,
                  variant, out):
    """The whole-image call behind render_views (name "render_views":
    hn_render_views, u of cfg.n_importance values) and render_image (name
    "render_image": hn_render_image(_variant), 64 + 128 and world rays)."""
    L.require_device(poses, table, t_vals, u, *ws)
    if torch.is_grad_enabled() and poses.requires_grad:
        raise ValueError(f"hashnerf_amd.{name}: the whole-image kernel has no gradient w.r.t. the poses; "
                         "render(H, W, K, c2w=pose) is differentiable in them (or detach the poses)")
    dev = poses.device
    views = name == "render_views"
    if poses.dim() != 3 or tuple(poses.shape[1:]) not in ((3, 4), (4, 4)):
        raise ValueError(f"hashnerf_amd.{name}: poses must be [n, 3, 4] or [n, 4, 4], got {tuple(poses.shape)}")
    poses = poses.contiguous()
    n = poses.shape[0]
    ni = int(cfg.n_importance) if views else 128
    if t_vals is None:
        t_vals = _linspace_cached(64, dev)
    if u is None:
        u = torch.linspace(0., 1., ni, device=dev)
    t_vals, u, table = t_vals.contiguous(), u.contiguous(), table.contiguous()
    if t_vals.numel() != 64 or u.numel() != ni:
        raise ValueError(f"hashnerf_amd.{name}: t_vals must hold 64 and u {ni} values")
    ws = [w.contiguous() for w in ws]
    H, W = int(H), int(W)
    if out is None:
        out = (torch.empty((n, H, W, 3), dtype=torch.float32, device=dev),
               torch.empty((n, H, W), dtype=torch.float32, device=dev),
               torch.empty((n, H, W), dtype=torch.float32, device=dev))
    rgb, depth, acc = out
    L.require_device(rgb, depth, acc)
    for t, shape in ((rgb, (n, H, W, 3)), (depth, (n, H, W)), (acc, (n, H, W))):
        if tuple(t.shape) != shape or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"hashnerf_amd.{name}: out tensors must be contiguous {shape} on {dev}")
    rays = torch.empty((n * H * W, 11), dtype=torch.float32, device=dev) if return_rays else None
    va = L.HnViewArgs()
    a = va.image
    a.n_views, a.H, a.W, a.pose_stride = n, H, W, poses.shape[1] * 4
    a.fx, a.fy, a.cx, a.cy = float(K[0][0]), float(K[1][1]), float(K[0][2]), float(K[1][2])
    a.near, a.far = float(near), float(far)
    for k, t in (("poses", poses), ("t_vals", t_vals), ("u", u), ("table", table), ("rgb", rgb), ("depth", depth),
                 ("acc", acc), ("rays", rays)):
        setattr(a, k, None if t is None else t.data_ptr())
    a.coarse = L.make_mlp(ws[:5])
    a.fine = L.make_mlp(ws[5:])
    a.weights_packed = 1 if weights_packed else 0
    lib = L.lib()
    need = lib.hn_render_views_workspace_bytes(cfg) if views else lib.hn_render_image_workspace_bytes(cfg)
    wsb, nbytes = _caller_ws(name, wsb, need, dev)
    t0 = TIMER.begin(name)
    if views:
        va.ndc, va.variant = int(bool(ndc)), int(variant)
        if ndc:
            va.ndc_sx, va.ndc_sy = ndc_scalars(H, W, K[0][0])   # float64 here, float32 in the struct
        L.check(lib.hn_render_views(cfg, va, L.ptr(wsb), nbytes, L.stream(dev)), name)
    elif variant:
        L.check(lib.hn_render_image_variant(cfg, a, int(variant), L.ptr(wsb), nbytes, L.stream(dev)),
                "render_image_variant")
    else:
        L.check(lib.hn_render_image(cfg, a, L.ptr(wsb), nbytes, L.stream(dev)), name)
    TIMER.end(name, t0)
    return (rgb, depth, acc, rays) if return_rays else (rgb, depth, acc)


def render_image(cfg, H, W, K, poses, near, far, table, ws, t_vals=None, u=None, wsb=None, weights_packed=False,
                 return_rays=False, variant=0, out=None):
    """hn_render_image (run_nerf_helpers.py:310-392 under :395-459): every
    pose of ``poses`` ([n, 3, 4] or [n, 4, 4] c2w on the device) rendered in
    one launch as render(H, W, K, c2w=pose, ndc=False, use_viewdirs=True) with
    perturb = 0 and raw_noise_std = 0 renders it.  Returns (rgb [n, H, W, 3],
    depth [n, H, W], acc [n, H, W]) and, with return_rays, the [n H W, 11] ray
    batch the kernel made, in pixel order.  cfg: make_render_cfg(..., perturb=
    False); ws: the coarse then the fine net's five weights; t_vals / u: by
    default the tensors render_rays uses (linspace(0, 1, 64) made on the CPU,
    linspace(0, 1, 128) on the device).  wsb: the caller's workspace (uint8, >=
    hn_render_image_workspace_bytes; its size does not depend on the images);
    weights_packed: it already holds ws's packed copies.  variant: the
    measured design alternatives (L.IMAGE_VARIANTS' bits; bitwise the same
    images).  out: (rgb, depth, acc) to write into instead of fresh tensors.
    64 + 128 samples and world rays only: render_views covers the rest."""
    return _render_views("render_image", cfg, H, W, K, poses, near, far, table, ws, False, t_vals, u, wsb,
                         weights_packed, return_rays, variant, out)


def render_views(cfg, H, W, K, poses, near, far, table, ws, ndc=False, t_vals=None, u=None, wsb=None,
                 weights_packed=False, return_rays=False, variant=0, out=None):
    """hn_render_views: render_image for every configuration the fused forward
    covers with perturb = 0 and no raw noise -- cfg.n_importance 128 or 64, and
    with ndc=True render()'s NDC rays (get_ndc_rays(H, W, K[0][0], 1., ...) on
    the device, bit for bit torch's; near, far and the view directions are the
    world ray's, as in render()).  Same arguments and returns as render_image;
    u defaults to linspace(0, 1, cfg.n_importance) on the device and must have
    that width; with return_rays the rays are the final (NDC) ones; wsb >=
    hn_render_views_workspace_bytes (the same for both counts)."""
    return _render_views("render_views", cfg, H, W, K, poses, near, far, table, ws, ndc, t_vals, u, wsb,
                         weights_packed, return_rays, variant, out)


# --------------------------------------------------------------------------
# density queries (hn_density_points / hn_density_lattice)
# --------------------------------------------------------------------------
def _f32x3(who, name, v):
    """Three numbers (or a 3-element tensor) as a CPU float32 tensor."""
    t = torch.as_tensor(v).detach().to("cpu", torch.float32).reshape(-1)
    if t.numel() != 3:
        raise ValueError(f"hashnerf_amd.{who}: {name} must hold 3 values, got {tuple(t.shape)}")
    return t


def _lattice_dims(who, dims):
    d = tuple(int(v) for v in dims)
    if len(d) != 3 or min(d) <= 0 or max(d) >= 1 << 31 or d[0] * d[1] * d[2] > L.DENSITY_MAX_POINTS:
        raise ValueError(f"hashnerf_amd.{who}: dims must be (nx, ny, nz), each >= 1 and at most "
                         f"{L.DENSITY_MAX_POINTS} points in all, got {dims!r}")
    return d


def lattice_coords(lo, step, dims, device=None):
    """The points of a density lattice, [nz, ny, nx, 3] float32: point (ix, iy,
    iz) has the coordinate lo[a] + float32(i_a) * step[a] on axis a, one float32
    multiply and one float32 add -- the host statement of the rule
    density_lattice's kernel follows, bit for bit."""
    nx, ny, nz = _lattice_dims("lattice_coords", dims)
    lo, step = _f32x3("lattice_coords", "lo", lo), _f32x3("lattice_coords", "step", step)
    ax = [lo[a] + torch.arange(n, dtype=torch.float32) * step[a] for a, n in enumerate((nx, ny, nz))]
    out = torch.empty((nz, ny, nx, 3), dtype=torch.float32)
    out[..., 0] = ax[0][None, None, :]
    out[..., 1] = ax[1][None, :, None]
    out[..., 2] = ax[2][:, None, None]
    return out if device is None else out.to(device)


def unpack_occupancy(words, dims):
    """Occupancy words (int32: bit q & 31 of word q >> 5 is point q = (iz * ny +
    iy) * nx + ix) -> bool [nz, ny, nx], on the words' device."""
    nx, ny, nz = _lattice_dims("unpack_occupancy", dims)
    n = nx * ny * nz
    words = words.reshape(-1)
    if words.dtype != torch.int32 or words.numel() != (n + 31) // 32:
        raise ValueError(f"hashnerf_amd.unpack_occupancy: {(n + 31) // 32} int32 words for dims {dims!r}, got "
                         f"{words.numel()} of {words.dtype}")
    bits = (words[:, None] >> torch.arange(32, dtype=torch.int32, device=words.device)) & 1
    return bits.reshape(-1)[:n].bool().reshape(nz, ny, nx)


def _density(who, grid, table, net_weights, n, threshold, want_sigma, out, call):
    """What density_points and density_lattice share: the outputs (fresh, or the
    caller's ``out`` = (sigma, occ)), the workspace and the call.  Returns
    (sigma or None, occ or None)."""
    if grid.n_levels != 16:
        raise ValueError(f"hashnerf_amd.{who}: the density kernel covers 16-level grids, got {grid.n_levels}")
    if threshold is None and not want_sigma:
        raise ValueError(f"hashnerf_amd.{who}: nothing asked for (want_sigma=False needs a threshold)")
    ws = [w.detach().contiguous() for w in net_weights]
    if [w.numel() for w in ws] != [2048, 1024, 1984, 4096, 192]:
        raise ValueError(f"hashnerf_amd.{who}: net_weights must be one NeRFSmall's five tensors "
                         "(NeRFSmall.weights())")
    table = table.detach().contiguous()
    L.require_device(table, *ws)
    dev = table.device
    if table.numel() != (16 << grid.log2_hashmap_size) * 2:
        raise ValueError(f"hashnerf_amd.{who}: table must be [16, 2^{grid.log2_hashmap_size}, 2]")
    sigma, occ = out if out is not None else (None, None)
    if out is None:
        sigma = torch.empty((n,), dtype=torch.float32, device=dev) if want_sigma else None
        occ = torch.empty(((n + 31) // 32,), dtype=torch.int32, device=dev) if threshold is not None else None
    for t, dt, m, name in ((sigma, torch.float32, n, "sigma"), (occ, torch.int32, (n + 31) // 32, "occ")):
        if t is not None and (t.dtype != dt or t.numel() != m or not t.is_contiguous() or t.device != dev):
            raise ValueError(f"hashnerf_amd.{who}: out's {name} must be contiguous {dt} of {m} elements on {dev}")
    if sigma is None and occ is None:
        raise ValueError(f"hashnerf_amd.{who}: out holds neither sigma nor occ")
    if occ is not None and threshold is None:
        raise ValueError(f"hashnerf_amd.{who}: an occ output needs a threshold")
    if n == 0:   # nothing to launch (an empty tensor's pointer is NULL: the library would refuse it)
        return sigma, occ
    nbytes = L.lib().hn_mlp_workspace_bytes()
    wsb = _ws(nbytes, dev)
    t0 = TIMER.begin(who)
    L.check(call(grid, L.make_mlp(ws), L.ptr(table), 0.0 if threshold is None else float(threshold), L.ptr(sigma),
                 L.ptr(occ), L.ptr(wsb), nbytes, L.stream(dev)), who)
    TIMER.end(who, t0)
    return sigma, occ


def _density_result(sigma, occ):
    return sigma if occ is None else occ if sigma is None else (sigma, occ)


@torch.no_grad()
def density_points(grid, table, net_weights, pts, threshold=None, want_sigma=True, out=None):
    """hn_density_points: raw sigma (NeRFSmall's column 3, before raw2outputs'
    ReLU) of the field (grid, table, one net's five weights) at pts [n, 3] --
    bitwise what NeRFSmall(cat[HashEmbedder(pts), sh])[:, 3] gives, from one
    kernel that writes nothing but the answers.  Returns sigma [n]; with a
    threshold (sigma, occ), occ = the int32 words of sigma > threshold (bit q &
    31 of word q >> 5; unpack_occupancy); with want_sigma=False only occ.
    out = (sigma or None, occ or None): tensors to write into.  No autograd:
    the outputs are detached."""
    pts = pts.detach().contiguous()
    L.require_device(pts)
    if pts.dim() != 2 or pts.shape[1] != 3:
        raise ValueError(f"hashnerf_amd.density_points: pts must be [n, 3], got {tuple(pts.shape)}")
    n = pts.shape[0]
    lib = L.lib()
    call = lambda g, w, t, thr, *rest: lib.hn_density_points(g, w, t, L.ptr(pts), n, thr, *rest)
    return _density_result(*_density("density_points", grid, table, net_weights, n, threshold, want_sigma, out, call))


@torch.no_grad()
def density_lattice(grid, table, net_weights, lo, step, dims, threshold=None, want_sigma=True, out=None):
    """hn_density_lattice: density_points on lattice_coords(lo, step, dims)
    without the points: the kernel forms each coordinate itself (bitwise
    lattice_coords').  dims = (nx, ny, nz); returns sigma [nz, ny, nx] and / or
    the occupancy words [(nx ny nz + 31) // 32] as density_points does (out's
    sigma: any contiguous tensor of nx ny nz elements)."""
    nx, ny, nz = _lattice_dims("density_lattice", dims)
    lo, step = _f32x3("density_lattice", "lo", lo), _f32x3("density_lattice", "step", step)
    lat = L.HnLattice()
    for a in range(3):
        lat.lo[a], lat.step[a], lat.dims[a] = float(lo[a]), float(step[a]), (nx, ny, nz)[a]
    lib = L.lib()
    call = lambda g, w, t, thr, *rest: lib.hn_density_lattice(g, w, t, lat, thr, *rest)
    sigma, occ = _density("density_lattice", grid, table, net_weights, nx * ny * nz, threshold, want_sigma, out, call)
    return _density_result(None if sigma is None else sigma.view(nz, ny, nx), occ)


def render_rays_fused(cfg, rays, t_vals, t_rand, u, noise_c, noise_f, table,
                      coarse_ws: Sequence[torch.Tensor], fine_ws: Sequence[torch.Tensor], ray_grad: bool = False):
    """ray_grad: the saved state is also kept for rays that require grad and the
    backward forms d rays (render_bwd_rays, RenderRaysGradFn); without it the
    state is kept only for a table or weight that requires grad and rays with
    grad get None and no extra launch, as before."""
    keep_feat = torch.is_grad_enabled() and (any(t.requires_grad for t in (table, *coarse_ws, *fine_ws))
                                             or (ray_grad and rays.requires_grad))
    return (RenderRaysGradFn if ray_grad else RenderRaysFn).apply(cfg, keep_feat, rays, t_vals, t_rand, u, noise_c, noise_f, table,
                              *coarse_ws, *fine_ws)
