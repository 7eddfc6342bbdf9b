"""What the GPU tests share: constants, comparisons, and the builders of their
scenes and forward states.  Every builder makes its draws in one fixed order
(the tests' tolerances were measured on exactly these inputs), and nothing here
imports the HIP package before a test asks for it: hf() resolves it on demand,
so collection works with no GPU and no built library."""
from types import SimpleNamespace

import numpy as np
import torch

from conftest import golden, pcg_table

DEV = "cuda"
MLP_KW = dict(num_layers=2, hidden_dim=64, geo_feat_dim=15, num_layers_color=3, hidden_dim_color=64,
              input_ch=32, input_ch_views=16)
BLENDER_BOX = (torch.tensor([-4.0, -4.0, -3.4]), torch.tensor([4.0, 4.0, 3.3]))
SMALL_BOX = (torch.tensor([-1.5, -1.5, -1.5]), torch.tensor([1.5, 1.5, 1.5]))
SMALL_T, SMALL_FINEST = 14, 64
OUT_KEYS = ("rgb", "depth", "acc", "sparsity", "rgb0", "depth0", "acc0", "sparsity0", "z_std", "z_coarse", "z_fine",
            "raw_c", "raw_f")


def hf():
    """hashnerf_pytorch_amd.functional (the `hn` fixture has loaded the package)."""
    from importlib import import_module
    return import_module("hashnerf_pytorch_amd.functional")


def step_coeffs():
    """The fused step's RAdam coefficients: the rectified form at lr 1e-2."""
    return {"beta1": 0.9, "beta2": 0.99, "one_minus_beta1": 1 - 0.9, "one_minus_beta2": 1 - 0.99, "eps": 1e-15,
            "neg_wd_lr": 0.0, "neg_step_lr": -1e-2, "mode": 2, "has_wd": 0}


# ---- comparisons ---------------------------------------------------------------
def _np(a):
    return a.detach().cpu().numpy() if torch.is_tensor(a) else a


def g2t(a, dev=DEV):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def close(a, b, rtol=1e-5, atol=1e-6, msg=""):
    np.testing.assert_allclose(_np(a), b, rtol=rtol, atol=atol, err_msg=msg)


def rel_err(a, b):
    """||a - b|| / ||b|| in float64."""
    a, b = np.asarray(_np(a), np.float64), np.asarray(_np(b), np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def rel_close(a, b, tol, msg):
    """||a - b|| <= tol * ||b|| (gradients: summation order of float atomics)."""
    err = rel_err(a, b)
    assert err <= tol, f"{msg}: relative error {err:.3e}"


def mostly_close(a, b, rtol, atol, frac, loose, msg):
    """Rows within (rtol, atol) make up at least frac; every entry within loose."""
    a = _np(a)
    a2, b2 = a.reshape(a.shape[0], -1), b.reshape(b.shape[0], -1)
    ok = np.isclose(a2, b2, rtol=rtol, atol=atol, equal_nan=True).all(-1)
    assert ok.mean() >= frac, f"{msg}: only {ok.mean():.3f} of rays within tolerance"
    np.testing.assert_allclose(a2, b2, rtol=0, atol=loose, err_msg=msg)


def bits_equal(a, b):
    """torch.equal on the bit patterns (a NaN depth of an empty ray compares equal to itself)."""
    if a.dtype == torch.float32:
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return a.shape == b.shape and torch.equal(a, b)


def done():
    """Synchronise and read the device fault word (raises if a kernel set a bit)."""
    torch.cuda.synchronize()
    hf().L.check_device_faults()


# ---- the workspace ---------------------------------------------------------------
def ws_offsets(n_rays):
    """Byte offsets into a render workspace of n_rays, down to the lists' counts:
    the leading regions of ws_layout (hn_render.hip), the one place a test may
    take them from.  packed: both nets [2][MLP_PACKED_FLOATS] | slab: dW slabs
    [256][4][MLP_PARAMS] | dfeat: coarse feature grads [n][2048] | draw: d raw
    [n][256][4] | marks: [n][4] u8 | lmeta: 8 count words."""
    L = hf().L
    o = SimpleNamespace(packed=0)
    o.slab = o.packed + 2 * L.MLP_PACKED_FLOATS * 4
    o.dfeat = o.slab + 256 * 4 * L.MLP_PARAMS * 4
    o.draw = o.dfeat + n_rays * 2048 * 4
    o.marks = o.draw + n_rays * 256 * 16
    o.lmeta = o.marks + n_rays * 4
    return o


def ws_stamp(wsb, n_rays):
    """The training forward's stamp: the 8-byte aligned word within count words 4-7."""
    at = ws_offsets(n_rays).lmeta + 16
    return wsb[at + -(wsb.data_ptr() + at) % 8:][:8]


# ---- fixtures and scenes ---------------------------------------------------------
def golden_ni64(name):
    """make_golden_ni64.load_render_ni64: the table gradient's levels 8-15 live
    in a second file (each committed file stays under 1 MiB)."""
    g = golden(name)
    g["table_grad"] = np.concatenate([g["table_grad"], golden(name + ".tg_hi")["table_grad_hi"]], 0)
    return g


def blender_nets(hn, T, seed, box=BLENDER_BOX, finest=512, sigma_sign=0, table_range=0.5):
    """torch.manual_seed(seed), then a uniform table and the two nets on the
    device.  sigma_sign: sigma = w . relu(h), so all weights of one sign fix the
    sign of every raw sigma."""
    torch.manual_seed(seed)
    emb = hn.HashEmbedder(box, log2_hashmap_size=T, finest_resolution=finest).to(DEV)
    with torch.no_grad():
        emb.table.uniform_(-table_range, table_range)
    mc, mf = hn.NeRFSmall(**MLP_KW).to(DEV), hn.NeRFSmall(**MLP_KW).to(DEV)
    if sigma_sign:
        with torch.no_grad():
            for m in (mc, mf):
                w = m.sigma_net[1].weight
                w[0] = sigma_sign * w[0].abs()
    return SimpleNamespace(emb=emb, mc=mc, mf=mf)


def blender_state(hn, B, T, seed, scatter="binned", ni=128, bin_cap=0, box=BLENDER_BOX, finest=512, sigma_sign=0,
                  det=False, dense=False, keep_feat=True, skip_dead=False):
    """blender_nets, B rays of a 400 x 400 blender camera, seeded draws, one
    training forward and the upstream gradients of an MSE + sparsity loss."""
    HF = hf()
    s = blender_nets(hn, T, seed, box, finest, sigma_sign)
    focal, K = hn.rays.blender_intrinsics(400, 400)
    ro, rd = hn.get_rays(400, 400, K, hn.pose_spherical(30.0 + seed, -30.0, 4.0)[:3, :4].to(DEV))
    sel = torch.randperm(400 * 400, device=DEV)[:B]
    ro, rd = ro.reshape(-1, 3)[sel], rd.reshape(-1, 3)[sel]
    vd = rd / torch.norm(rd, dim=-1, keepdim=True)
    s.rays = torch.cat([ro, rd, 2. * torch.ones_like(rd[:, :1]), 6. * torch.ones_like(rd[:, :1]), vd], -1)
    g = torch.Generator(device=DEV).manual_seed(seed + 1)   # the forward does not touch it
    s.t_rand = torch.rand((B, 64), device=DEV, generator=g)
    s.u = torch.rand((B, 128), device=DEV, generator=g)[:, :ni].contiguous()
    s.target = torch.rand((B, 3), device=DEV, generator=g)
    if det:
        s.t_rand, s.u = None, torch.linspace(0., 1., ni, device=DEV).expand(B, ni).contiguous()
    s.t_vals = torch.linspace(0., 1., 64, device=DEV)
    s.cfg = HF.make_render_cfg(s.emb.grid(), True, False, not det, n_importance=ni, scatter=scatter, dense_bwd=dense)
    s.cfg.bin_cap = bin_cap
    s.HF, s.ws = HF, list(s.mc.weights()) + list(s.mf.weights())
    s.out, s.st = HF.render_fwd(s.cfg, s.rays, s.t_vals, s.t_rand, s.u, None, None, s.emb.table.detach(), s.ws,
                                keep_feat, skip_dead_color=skip_dead)
    s.grads = dict(g_rgb=2. * (s.out["rgb"] - s.target) / (3 * B), g_rgb0=2. * (s.out["rgb0"] - s.target) / (3 * B),
                   g_sparsity=torch.full((B,), 1e-3, device=DEV), g_sparsity0=torch.full((B,), 1e-3, device=DEV))
    return s


def bwd(s, st=None, grads=None, overwrite=False, init=None, mlp_junk=False):
    """render_bwd of a blender_state into zeros (or init / NaN-filled MLP
    gradients), then done().  Returns (d_table, dws)."""
    d_table = torch.zeros_like(s.emb.table) if init is None else init.clone()
    dws = s.HF.zeros_like_all(s.ws)
    if mlp_junk:
        for d in dws:
            d.fill_(float("nan"))
    s.HF.render_bwd(st or s.st, s.grads if grads is None else grads, d_table, dws, overwrite=overwrite,
                    overwrite_mlp=mlp_junk)
    done()
    return d_table, dws


def scene_from_golden(hn, g):
    """Embedder and nets of a reference-made fixture."""
    emb = hn.HashEmbedder((g2t(g["box_min"], "cpu"), g2t(g["box_max"], "cpu")),
                          log2_hashmap_size=int(g["log2T"]), finest_resolution=int(g["finest"])).to(DEV)
    with torch.no_grad():
        emb.table.copy_(g2t(pcg_table(g["table_seed"], g["log2T"])))
    mc, mf = hn.NeRFSmall(**MLP_KW).to(DEV), hn.NeRFSmall(**MLP_KW).to(DEV)
    mc.load_state_dict({k[3:]: g2t(v) for k, v in g.items() if k.startswith("wc:")})
    mf.load_state_dict({k[3:]: g2t(v) for k, v in g.items() if k.startswith("wf:")})
    return SimpleNamespace(emb=emb, mc=mc, mf=mf)


_SMALL = {}


def small_scene(hn, key, B, gen_seed, draws, edit=None):
    """T = 14, finest 64, the +-1.5 box, pcg_table(7), nets from
    torch.manual_seed(5), B rays of a 100 x 100 blender camera; built once per
    key and left unchanged.  draws: (name, "rand" | "randn", width) in the order
    they are taken from the CPU generator seeded with gen_seed, after the rays'
    randperm; a name (field, k) lands in the dict s.field[k].  edit(emb, nets,
    ws) may rewrite the table and the weights in place."""
    if key in _SMALL:
        return _SMALL[key]
    g = torch.Generator().manual_seed(gen_seed)
    emb = hn.HashEmbedder(SMALL_BOX, log2_hashmap_size=SMALL_T, finest_resolution=SMALL_FINEST).to(DEV)
    with torch.no_grad():
        emb.table.copy_(torch.from_numpy(pcg_table(7, SMALL_T)).to(DEV))
    torch.manual_seed(5)
    nets = [hn.NeRFSmall(**MLP_KW).to(DEV), hn.NeRFSmall(**MLP_KW).to(DEV)]   # coarse and fine: different weights
    ws = [w.detach() for n in nets for w in n.weights()]
    if edit is not None:
        with torch.no_grad():
            edit(emb, nets, ws)
    _, K = hn.rays.blender_intrinsics(100, 100)
    c2w = hn.pose_spherical(30.0, -30.0, 4.0)
    ro, rd = hn.get_rays(100, 100, K, c2w[:3, :4].to(DEV))
    sel = torch.randperm(100 * 100, generator=g)[:B].to(DEV)
    o, d = ro.reshape(-1, 3)[sel], rd.reshape(-1, 3)[sel]
    rays = torch.cat([o, d, torch.full((B, 1), 2.0, device=DEV), torch.full((B, 1), 6.0, device=DEV),
                      d / d.norm(dim=-1, keepdim=True)], -1).contiguous()
    s = SimpleNamespace(emb=emb, table=emb.table.detach(), ws=ws, rays=rays,
                        t_vals=torch.linspace(0., 1., 64, device=DEV))
    for name, kind, width in draws:
        x = getattr(torch, kind)(B, width, generator=g).to(DEV)
        if isinstance(name, tuple):
            vars(s).setdefault(name[0], {})[name[1]] = x
        else:
            setattr(s, name, x)
    vars(s).setdefault("noise_c", None)    # a scene without raw noise
    vars(s).setdefault("noise_f", None)
    _SMALL[key] = s
    return s


def _one_sign_density(sign):
    def edit(emb, nets, ws):
        for n in nets:
            row = n.sigma_net[1].weight[0]
            row.copy_(row.abs().clamp_min(1e-3) * sign)
    return edit


def kind_scene(hn, B, kind, noise=False):
    """The small scene of the pre-pass and next-batch tests.  kind: "rand" (about
    half of the samples dead), "dead" / "live" (sigma_net's density row of one
    sign, its inputs being ReLU outputs: all raw sigma <= 0 / > 0)."""
    draws = [("target", "rand", 3), ("t_rand", "rand", 64), ("u", "rand", 128)]
    if noise:
        draws += [("noise_c", "randn", 64), ("noise_f", "randn", 192)]
    edit = None if kind == "rand" else _one_sign_density(-1.0 if kind == "dead" else 1.0)
    return small_scene(hn, ("kind", B, kind, noise), B, 100 + B, draws, edit)


def forward_kind(HF, s, cfg, fused, skip_dead, wsb=None):
    """The training forward of a kind_scene, plain or with the loss (fused)."""
    loss = dict(target=s.target, world=1, sparse_w=1e-3) if fused else None
    return HF.render_fwd(cfg, s.rays, s.t_vals, s.t_rand, s.u, s.noise_c, s.noise_f, s.table, s.ws, True, wsb=wsb,
                         skip_dead_color=skip_dead, loss=loss)


def loss_of(s, out, lo):
    """render_bwd's loss= for a forward's outputs; the loss value lands in lo."""
    return dict(target=s.target, rgb=out["rgb"], rgb0=out["rgb0"], sparsity=out["sparsity"],
                sparsity0=out["sparsity0"], tv=None, world=1, sparse_w=1e-3, tv_w=0.0, out=lo)


def backward_after_loss_forward(HF, s, out, st):
    """The binned backward after a loss-mode forward: [loss value, table
    gradient] + the ten NeRFSmall gradients."""
    lo = torch.empty(4, device=DEV)
    dws = HF.zeros_like_all(s.ws)
    d_table = torch.empty_like(s.table)
    HF.render_bwd(st, {}, d_table, dws, overwrite=True, overwrite_mlp=True, loss=loss_of(s, out, lo),
                  prepass_done=True)
    return [lo, d_table] + dws
