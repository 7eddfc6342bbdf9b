"""The training forward that also runs the composite backward
(hn_render_fwd_args.loss) and the backward that then launches no pre-pass
(hn_render_bwd_args.prepass_done).  The d raw values come from the same
function on the same floats, so everything is compared bitwise against the
plain forward + the pre-pass.

Shapes: T=14, finest 64, B in {1, 5, 37, 256}: a single ray, a partial last
forward workgroup (4 rays each), and exactly one lists workgroup of 256."""
import ctypes as C

import numpy as np
import pytest
import torch

from gpu_support import (SMALL_BOX, SMALL_FINEST as FINEST, SMALL_T as T, backward_after_loss_forward, bits_equal,
                         forward_kind as forward, kind_scene as scene, loss_of, step_coeffs)

DEV = torch.device("cuda:0")
BS = (1, 5, 37, 256)
KINDS = ("rand", "dead", "live")   # about half of the samples dead, all raw sigma <= 0, all > 0
FAULT_PREPASS = 128

def run_pair(hn, B, kind, white, dense, noise=False):
    """(separate, fused) results of one case: loss value, table gradient, the
    ten NeRFSmall gradients, and the table / m / v after a fused table step."""
    from hashnerf_pytorch_amd import functional as HF
    s = scene(hn, B, kind, noise)
    cfg = HF.make_render_cfg(s.emb.grid(), white, False, True, scatter="binned", dense_bwd=bool(dense))
    assert hn._lib.lib().hn_render_scatter_mode(cfg, B) == 2
    g = torch.Generator().manual_seed(9)
    m0 = (torch.rand(s.table.shape, generator=g) - 0.5).to(DEV) * 1e-3
    v0 = torch.rand(s.table.shape, generator=g).to(DEV) * 1e-6
    res = []
    for fused in (False, True):
        r = {}
        for stepped in (False, True):
            out, st = forward(HF, s, cfg, fused, skip_dead=not dense and not noise)
            lo = torch.empty(4, device=DEV)
            dws = HF.zeros_like_all(s.ws)
            d_table = None if stepped else torch.empty_like(s.table)
            p, m, v = s.table.clone(), m0.clone(), v0.clone()
            HF.render_bwd(st, {}, d_table, dws, overwrite=True, overwrite_mlp=True, loss=loss_of(s, out, lo),
                          table_step=(p, m, v, step_coeffs()) if stepped else None, prepass_done=fused)
            torch.cuda.synchronize()
            if stepped:
                r.update(p=p, m=m, v=v)
            else:
                r.update(lo=lo, d_table=d_table, dws=dws)
        res.append(r)
    return res


def assert_pair_equal(a, b):
    for k in ("lo", "d_table", "p", "m", "v"):
        assert bits_equal(a[k], b[k]), k
    for i, (x, y) in enumerate(zip(a["dws"], b["dws"])):
        assert bits_equal(x, y), f"NeRFSmall gradient {i}"


@pytest.mark.gpu
@pytest.mark.parametrize("dense", [0, 1])
@pytest.mark.parametrize("white", [True, False])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B", BS)
def test_fused_prepass_matches_separate_bitwise(hn, B, kind, white, dense):
    """render_fwd(loss) + render_bwd(prepass_done) against render_fwd() +
    render_bwd(loss): loss value, d_table, the ten NeRFSmall gradients and a
    fused table step's table / m / v, torch.equal, with the exact-zero
    skipping (and the forward's skip_dead_color) and with dense_bwd."""
    a, b = run_pair(hn, B, kind, white, dense)
    assert_pair_equal(a, b)
    if kind != "dead":
        assert torch.count_nonzero(a["d_table"]) > 0
    else:
        assert torch.count_nonzero(a["dws"][5]) == 0   # no density: the fine net has no gradient


@pytest.mark.gpu
@pytest.mark.parametrize("dense", [0, 1])
@pytest.mark.parametrize("B", BS)
def test_fused_prepass_with_raw_noise_bitwise(hn, B, dense):
    a, b = run_pair(hn, B, "rand", True, dense, noise=True)
    assert_pair_equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B", BS)
def test_loss_mode_forward_outputs_unchanged(hn, B, kind):
    """The loss-mode forward gives bitwise the plain forward's rgb, depth,
    acc, sparsity (both passes), z_std, raw, z, fine_src, features and masks."""
    from hashnerf_pytorch_amd import functional as HF
    s = scene(hn, B, kind)
    cfg = HF.make_render_cfg(s.emb.grid(), True, False, True, scatter="binned")
    (oa, sa), (ob, sb) = (forward(HF, s, cfg, fused, skip_dead=False) for fused in (False, True))
    torch.cuda.synchronize()
    assert set(oa) == set(ob) and len(oa) == 13
    for k in oa:
        assert bits_equal(oa[k], ob[k]), k
    assert bits_equal(sa.fine_src, sb.fine_src)
    assert bits_equal(sa.feat, sb.feat)
    # with skip_dead_color the tiles that are stored, and everything else, agree too
    (oa, sa), (ob, sb) = (forward(HF, s, cfg, fused, skip_dead=True) for fused in (False, True))
    for k in oa:
        assert bits_equal(oa[k], ob[k]), k
    assert bits_equal(sa.fine_src, sb.fine_src)


@pytest.mark.gpu
def test_trainer_fused_prepass_same_trajectory(hn):
    """8 Trainer.step()s at T=14, B=64 (TV term on: steps <= tv_until) with
    the fold on, with the pre-pass kept (fuse_prepass off) and with the
    separate loss kernel (fuse_loss off): table, NeRFSmall weights and every
    RAdam moment bitwise equal after step 8."""
    from hashnerf_pytorch_amd.train import SyntheticBlender, Trainer, default_args
    data = SyntheticBlender(64, 64, 4, DEV, seed=0)
    res = []
    for fuse_loss, fuse_prepass in ((False, False), (True, False), (True, True)):
        args = default_args(N_rand=64, log2_hashmap_size=T, finest_res=FINEST, tv_loss_weight=1e-4,
                            sparse_loss_weight=1e-3)
        assert args.tv_until >= 8
        tr = Trainer(args, data, DEV, seed=3)
        tr.fuse_loss, tr.fuse_prepass = fuse_loss, fuse_prepass
        torch.manual_seed(11)
        losses = [float(tr.step()[0]) for _ in range(8)]
        t = tr.embed_fn.table
        ws = tr.kw_train["network_fn"].weights() + tr.kw_train["network_fine"].weights()
        sts = [tr.optimizer.state[p] for p in [t] + ws]
        res.append((losses, [p.detach().clone() for p in [t] + ws], [x["exp_avg"].clone() for x in sts],
                    [x["exp_avg_sq"].clone() for x in sts], [int(x["step"]) for x in sts]))
    ref = res[2]
    assert ref[4] == [8] * 11
    assert res[1][0] == ref[0]                               # the same loss workgroup
    np.testing.assert_allclose(res[0][0], ref[0], rtol=1e-6)  # hn_loss_fwd_bwd: another thread count
    for other in res[:2]:
        assert other[4] == ref[4]
        for k in (1, 2, 3):
            for i, (x, y) in enumerate(zip(other[k], ref[k])):
                assert torch.equal(x, y), (k, i)


def _read_faults(hn):
    torch.cuda.synchronize()
    w = C.c_int32(-1)
    assert hn._lib.lib().hn_device_faults(C.byref(w), 1) == 0
    return w.value


def _forge(HF, st, s):
    """Make functional.render_bwd believe st's forward ran with the loss, so
    that the device-side stamp check is what refuses the call."""
    import weakref
    st.prepass_done = (s.target.data_ptr(), 1.0, 1e-3)
    HF._PREPASS_ON_WS[st.wsb.data_ptr()] = weakref.ref(st)


@pytest.mark.gpu
def test_prepass_done_guards(hn, monkeypatch):
    """prepass_done after a plain forward, after a loss-mode forward of
    another B, and twice after one forward: functional.render_bwd refuses each
    before any launch; forced past that check, the first kernel finds no valid
    stamp and sets fault bit 128 without faulting the device."""
    from hashnerf_pytorch_amd import functional as HF
    B = 37
    s, s5 = scene(hn, B, "rand"), scene(hn, 5, "rand")
    cfg = HF.make_render_cfg(s.emb.grid(), True, False, True, scatter="binned")
    nbytes = hn._lib.lib().hn_render_workspace_bytes(cfg, B)
    wsb = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)   # no stale stamp in recycled memory
    monkeypatch.setattr(HF, "CHECK_FAULTS", False)
    assert _read_faults(hn) == 0

    def backward(st, out):
        backward_after_loss_forward(HF, s, out, st)

    # 1. a plain forward
    out, st = forward(HF, s, cfg, False, True, wsb=wsb)
    with pytest.raises(ValueError, match="prepass_done"):
        backward(st, out)
    assert _read_faults(hn) == 0
    _forge(HF, st, s)
    backward(st, out)
    assert _read_faults(hn) == FAULT_PREPASS
    # 2. a loss-mode forward of another B on the workspace since
    out, st = forward(HF, s, cfg, True, True, wsb=wsb)
    backward(st, out)                                    # (consumes this forward's stamp)
    assert _read_faults(hn) == 0
    out, st = forward(HF, s, cfg, False, True, wsb=wsb)
    forward(HF, s5, cfg, True, True, wsb=wsb)
    with pytest.raises(ValueError, match="prepass_done"):
        backward(st, out)
    _forge(HF, st, s)
    backward(st, out)
    assert _read_faults(hn) == FAULT_PREPASS
    # 3. two backwards on one loss-mode forward
    out, st = forward(HF, s, cfg, True, True, wsb=wsb)
    backward(st, out)
    assert _read_faults(hn) == 0
    with pytest.raises(ValueError, match="prepass_done"):
        backward(st, out)
    _forge(HF, st, s)
    backward(st, out)
    assert _read_faults(hn) == FAULT_PREPASS
    # the workspace is good for the next step
    out, st = forward(HF, s, cfg, True, True, wsb=wsb)
    backward(st, out)
    assert _read_faults(hn) == 0


def test_prepass_abi_validation_without_gpu(hn):
    """The additive ABI 14 fields are validated before any launch."""
    L = hn._lib
    lib = L.lib()
    HF = hn.functional
    emb = hn.HashEmbedder(SMALL_BOX, log2_hashmap_size=T, finest_resolution=FINEST)
    cfg = HF.make_render_cfg(emb.grid(), True, False, False, scatter="binned")
    cfg_a = HF.make_render_cfg(emb.grid(), True, False, False, scatter="atomic")
    x = 16   # never dereferenced
    ws = lib.hn_render_workspace_bytes(cfg, 8)
    f = L.HnRenderFwdArgs()
    f.n_rays = 8
    for name, kind in L.HnRenderFwdArgs._fields_:
        if kind is L._P and name not in ("t_rand", "noise_c", "noise_f"):
            setattr(f, name, x)
    for m in (f.coarse, f.fine):
        for name, _ in L.HnMlp._fields_:
            setattr(m, name, x)
    f.weights_packed = 1
    la = L.HnRenderLoss()
    la.world, la.sparse_w = 1.0, 1e-3
    f.loss = C.pointer(la)
    assert lib.hn_render_fwd(cfg, f, C.c_void_p(x), ws, None) == 1       # loss without a target
    la.target = x
    la.world = 0.0
    assert lib.hn_render_fwd(cfg, f, C.c_void_p(x), ws, None) == 2       # world must be positive
    la.world = 1.0
    assert lib.hn_render_fwd(cfg_a, f, C.c_void_p(x), ws, None) == 2     # float-atomic schedule: pre-pass kept
    b = L.HnRenderBwdArgs()
    b.n_rays = 8
    for name, kind in L.HnRenderBwdArgs._fields_:
        if kind is L._P and name in ("rays", "table", "z_coarse", "z_fine", "raw_c", "raw_f", "fine_src", "feat",
                                     "d_table"):
            setattr(b, name, x)
    for m in (b.coarse, b.fine, b.d_coarse, b.d_fine):
        for name, _ in L.HnMlp._fields_:
            setattr(m, name, x)
    b.weights_packed, b.d_table_mode, b.prepass_done = 1, 3, 1
    assert lib.hn_render_bwd(cfg, b, C.c_void_p(x), ws, None) == 2       # prepass_done needs the loss
    lb = L.HnRenderLoss()
    for name in ("target", "rgb", "rgb0", "sparsity", "sparsity0", "out"):
        setattr(lb, name, x)
    lb.world = 1.0
    b.loss = C.pointer(lb)
    b.g_rgb = x
    assert lib.hn_render_bwd(cfg, b, C.c_void_p(x), ws, None) == 2       # ... and no explicit upstream gradients
    b.g_rgb = None
    assert lib.hn_render_bwd(cfg_a, b, C.c_void_p(x), ws, None) == 2     # float-atomic schedule: pre-pass kept


def test_render_bwd_refuses_prepass_done_without_loss_forward(hn):
    HF = hn.functional
    st = HF.RenderState()
    st.rays = torch.zeros((4, 11))
    st.prepass_done = None
    with pytest.raises(ValueError, match="prepass_done"):
        HF.render_bwd(st, {}, None, [], prepass_done=True)
