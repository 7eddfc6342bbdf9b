"""The two forms of render_fwd_kernel (hn_render_fwd_form): 1, 4-ray workgroups
with the weight fragments through per-wave LDS rings, and 2, 16-ray workgroups
that hold both nets' sigma layers resident in LDS.  The MFMA products and
their order are the same, so every output is compared bitwise.

Shapes: T=14, finest 64; B in {1, 5, 16, 17, 37, 256}: one ray (15 waves of
the resident workgroup only copy and leave after the barrier), a partial
workgroup, exactly one, one + one ray, two full + a partial one, 16 full."""
from types import SimpleNamespace

import pytest
import torch

from gpu_support import (MLP_KW, OUT_KEYS, SMALL_T as T, backward_after_loss_forward as backward, bits_equal,
                         small_scene, ws_offsets, ws_stamp)

DEV = torch.device("cuda:0")
BS = (1, 5, 16, 17, 37, 256)
# loss mode, importance samples, skip_dead_color, perturb + raw noise, white background: every factor at both
# levels, every pair of factors at three or four of its combinations
VARIANTS = (
    dict(loss=False, ni=128, skip=False, noise=False, white=True),
    dict(loss=True, ni=128, skip=True, noise=False, white=True),    # the trainer's step
    dict(loss=True, ni=64, skip=True, noise=False, white=False),
    dict(loss=False, ni=64, skip=False, noise=True, white=False),
    dict(loss=True, ni=128, skip=False, noise=True, white=False),
    dict(loss=False, ni=128, skip=True, noise=False, white=False),
    dict(loss=False, ni=64, skip=True, noise=False, white=True),
    dict(loss=True, ni=64, skip=False, noise=True, white=True),
)


def make_nets(hn, seed=5):
    torch.manual_seed(seed)
    nets = [hn.NeRFSmall(**MLP_KW).to(DEV), hn.NeRFSmall(**MLP_KW).to(DEV)]   # coarse and fine: different weights
    return [w.detach() for n in nets for w in n.weights()]


def scene(hn, B):
    """Rays, targets, draws (for both fine-pass shapes), table and the two nets,
    built once per B and left unchanged.  Half of the space has no density,
    so tiles with and without the colour net both occur."""
    def half_space_density(emb, nets, ws):
        assert not torch.equal(ws[0], ws[5])
        # density where x < 0 only: the coarsest level's first feature is +-0.5
        # by the vertex's side (its 17^3 vertices, the few that share a row
        # taking the later one's), and both nets' raw sigma is relu of it alone
        i = torch.arange(17)
        v = torch.stack(torch.meshgrid(i, i, i, indexing="ij"), -1).reshape(-1, 3)
        emb.table[0, hn.embedding.hash(v, T).to(DEV), 0] = torch.where(v[:, 0] < 8, 0.5, -0.5).to(DEV)
        for s0, s1 in ((ws[0], ws[1]), (ws[5], ws[6])):   # sigma_net.0 [64, 32], sigma_net.1 [16, 64]
            s0[0].zero_()
            s0[0, 0] = 1.0
            s1[0].zero_()
            s1[0, 0] = 1.0

    draws = [("target", "rand", 3), ("t_rand", "rand", 64), (("u", 128), "rand", 128), (("u", 64), "rand", 64),
             ("noise_c", "randn", 64), (("noise_f", 128), "randn", 192), (("noise_f", 64), "randn", 128)]
    return small_scene(hn, ("resident", B), B, 300 + B, draws, half_space_density)


def make_cfg(HF, s, v):
    return HF.make_render_cfg(s.emb.grid(), v["white"], False, v["noise"], n_importance=v["ni"], scatter="binned")


def forward(HF, s, v, form, rows=None, keep_feat=True, ws=None, wsb=None):
    """One render_fwd of the scene's rays (rows: a slice of them) in a form."""
    sl = slice(None) if rows is None else rows
    ni, noise = v["ni"], v["noise"]
    B = s.rays[sl].shape[0]
    loss = dict(target=s.target[sl], world=1, sparse_w=1e-3) if v["loss"] else None
    out, st = HF.render_fwd(make_cfg(HF, s, v), s.rays[sl], s.t_vals, s.t_rand[sl] if noise else None,
                            s.u[ni][sl], s.noise_c[sl] if noise else None,
                            s.noise_f[ni][sl] if noise else None, s.table, s.ws if ws is None else ws,
                            keep_feat, wsb=wsb, skip_dead_color=v["skip"], loss=loss, form=form)
    assert out["rgb"].shape == (B, 3)
    return out, st


def workspace_marks(HF, st, B, v):
    """What the loss-mode forward leaves in its workspace for the backward: d
    raw [B][64 + fine][4], the marks [B][4] u8 and the stamp."""
    at = ws_offsets(B)
    draw = st.wsb[at.draw:at.marks].view(torch.float32).view(B, 256, 4)[:, :64 + 64 + v["ni"]]
    marks = st.wsb[at.marks:at.lmeta]
    return draw.clone(), marks.clone(), ws_stamp(st.wsb, B).clone()


def stored_tiles(st, out, v):
    """The feature cache with the words no forward writes zeroed: [B][8 tiles]
    [1024] features, then [B][8][192] mask words; the fine pass has 6 or 4
    tiles, and under skip_dead_color (without raw noise) a fine tile is stored
    only if one of its 32 raw sigmas is positive."""
    B = st.feat.shape[0]
    n_fine = (64 + v["ni"]) // 32
    stored = torch.zeros(B, 8, dtype=torch.bool, device=DEV)
    stored[:, :2 + n_fine] = True
    if v["skip"] and not v["noise"]:
        stored[:, 2:2 + n_fine] = (out["raw_f"][..., 3].view(B, n_fine, 32) > 0).any(-1)
    feat = st.feat.view(torch.int32)
    f = torch.where(stored[..., None], feat[:, :8192].view(B, 8, 1024), 0)
    m = torch.where(stored[..., None], feat[:, 8192:].view(B, 8, 192), 0)
    return torch.cat([f.view(B, -1), m.view(B, -1)], 1), stored


@pytest.mark.gpu
@pytest.mark.parametrize("v", VARIANTS, ids=lambda v: "-".join(f"{k}{int(x)}" for k, x in v.items()))
@pytest.mark.parametrize("B", BS)
def test_resident_form_matches_ring_form_bitwise(hn, B, v):
    """Form 1 against form 2 on the same inputs: the 13 outputs, fine_src, the
    feature cache with its masks; under the loss mode also d raw, the marks and
    the stamp, and after each form the binned backward's loss value, table
    gradient and ten NeRFSmall gradients."""
    from hashnerf_pytorch_amd import functional as HF
    s = scene(hn, B)
    res = []
    for form in ("ring", "resident"):
        out, st = forward(HF, s, v, form)
        torch.cuda.synchronize()
        marks = grads = None
        if v["loss"]:
            marks = workspace_marks(HF, st, B, v)   # (the backward consumes the stamp)
            grads = backward(HF, s, out, st)
            torch.cuda.synchronize()
        res.append((out, st, marks, grads))
    (oa, sa, ma, ga), (ob, sb, mb, gb) = res
    assert set(oa) == set(OUT_KEYS) == set(ob)
    for k in OUT_KEYS:
        assert bits_equal(oa[k], ob[k]), k
    assert bits_equal(sa.fine_src, sb.fine_src), "fine_src"
    (fa, stored), (fb, _) = stored_tiles(sa, oa, v), stored_tiles(sb, ob, v)
    assert torch.equal(fa, fb), "feature cache and masks"
    assert torch.count_nonzero(fa[:, :8192]) > 0 and torch.count_nonzero(fa[:, 8192:]) > 0
    if B == 256:   # tiles of both kinds: the colour net skipped and run, in either pass
        for raw in (oa["raw_c"], oa["raw_f"]):
            live = (raw[..., 3].reshape(B, -1, 32) > 0).any(-1)
            assert 0 < int(live.sum()) < live.numel()
    if v["loss"]:
        for name, x, y in zip(("d raw", "marks", "stamp"), ma, mb):
            assert bits_equal(x, y), name
        assert torch.count_nonzero(ma[0]) > 0 and torch.count_nonzero(ma[2]) > 0
        names = ("loss", "d_table") + tuple(f"NeRFSmall gradient {j}" for j in range(10))
        for name, x, y in zip(names, ga, gb):
            assert bits_equal(x, y), name
        assert torch.count_nonzero(ga[1]) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("noise", [False, True])
def test_resident_form_ray_independent_of_batch_composition(hn, noise):
    """37 rays in one resident-form launch equal, ray by ray, the same rays
    launched as 16 + 16 + 5 and as single rays: a ray's result depends neither
    on its wave nor on its workgroup."""
    from hashnerf_pytorch_amd import functional as HF
    B = 37
    s = scene(hn, B)
    v = dict(loss=False, ni=128, skip=not noise, noise=noise, white=True)
    whole, _ = forward(HF, s, v, "resident", keep_feat=False)
    parts = [slice(0, 16), slice(16, 32), slice(32, 37)], [slice(i, i + 1) for i in range(B)]
    for split in parts:
        outs = [forward(HF, s, v, "resident", rows=rows, keep_feat=False)[0] for rows in split]
        torch.cuda.synchronize()
        for k in OUT_KEYS:
            assert bits_equal(torch.cat([o[k] for o in outs]), whole[k]), (k, len(split))
    # the stored tiles too (every tile is stored without skip_dead_color)
    v = dict(v, skip=False)
    _, st = forward(HF, s, v, "resident")
    sts = [forward(HF, s, v, "resident", rows=rows)[1] for rows in parts[0]]
    torch.cuda.synchronize()
    assert bits_equal(torch.cat([x.feat for x in sts]), st.feat)
    assert bits_equal(torch.cat([x.fine_src for x in sts]), st.fine_src)


@pytest.mark.gpu
def test_resident_form_sees_repacked_weights(hn):
    """The resident copies are made in every launch from the workspace's packed
    nets: form 2, the weights overwritten and packed again into the same
    workspace, form 2 again -- equal to form 1 on the new weights, and not to
    the first launch."""
    from hashnerf_pytorch_amd import functional as HF
    B = 37
    s = scene(hn, B)
    v = dict(loss=False, ni=128, skip=False, noise=False, white=True)
    ws = [w.clone() for w in s.ws]
    nbytes = hn._lib.lib().hn_render_workspace_bytes(make_cfg(HF, s, v), B)
    wsb = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    first, _ = forward(HF, s, v, "resident", ws=ws, wsb=wsb)
    first = {k: x.clone() for k, x in first.items()}
    new = make_nets(hn, seed=6)
    for w, x in zip(ws, new):
        w.copy_(x)
    second, st2 = forward(HF, s, v, "resident", ws=ws, wsb=wsb)
    ref, st1 = forward(HF, s, v, "ring", ws=new)
    torch.cuda.synchronize()
    for k in OUT_KEYS:
        assert bits_equal(second[k], ref[k]), k
    assert bits_equal(st2.feat, st1.feat)
    assert not bits_equal(first["raw_c"], second["raw_c"]) and not bits_equal(first["raw_f"], second["raw_f"])
    # the packed copies a backward's repack leaves (weights_packed): the same launch without a packing kernel
    third, _ = HF.render_fwd(make_cfg(HF, s, v), s.rays, s.t_vals, None, s.u[128], None, None, s.table, ws,
                             False, wsb=wsb, weights_packed=True, form="resident")
    torch.cuda.synchronize()
    for k in OUT_KEYS:
        assert bits_equal(third[k], ref[k]), k


@pytest.mark.gpu
def test_automatic_form_rule(hn):
    """hn_render_fwd picks the resident form where ceil(n_rays / 16) reaches the
    compute units the library reports (the device's), the ring form below."""
    from hashnerf_pytorch_amd import functional as HF
    _, cus = HF.fwd_pick(1)
    assert cus == torch.cuda.get_device_properties(DEV).multi_processor_count and cus > 0
    below = 16 * (cus - 1)            # cus - 1 workgroups of 16 rays
    assert HF.fwd_pick(below) == ("ring", cus)
    assert HF.fwd_pick(below + 1) == ("resident", cus)
    assert HF.fwd_pick(1)[0] == "ring" and HF.fwd_pick(16 * cus)[0] == "resident"
    # and the automatic launch at the threshold gives the forced forms' bits
    B = below + 1
    s = scene(hn, 256)
    idx = torch.arange(B, device=DEV) % 256
    big = SimpleNamespace(**dict(vars(s), rays=s.rays[idx], target=s.target[idx], t_rand=s.t_rand[idx],
                                 u={128: s.u[128][idx]}, noise_c=None, noise_f={128: None}))
    v = dict(loss=False, ni=128, skip=True, noise=False, white=True)
    outs = [forward(HF, big, v, form, keep_feat=False)[0] for form in ("auto", "ring", "resident")]
    torch.cuda.synchronize()
    for k in OUT_KEYS:
        assert bits_equal(outs[0][k], outs[1][k]) and bits_equal(outs[0][k], outs[2][k]), k
    # the first 256 rays again: a ray's result does not depend on the batch around it
    small = forward(HF, s, v, "ring", keep_feat=False)[0]
    for k in ("rgb", "raw_f", "z_fine"):
        assert bits_equal(outs[0][k][:256], small[k]), k
