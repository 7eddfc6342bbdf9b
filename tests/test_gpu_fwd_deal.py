"""The resident forward's deal of ray runs to workgroups (fwd_res_deal,
hn_render_fwd.h) leaves every result what it was: which wave computes a ray
changes nothing the ray writes.  Form 2 against form 1 (whose map is
untouched), bitwise, on the T=14 / finest-64 scene with density in half of the
space.

B = 1,024: 64 workgroups, two 64-ray segments per XCD, the smallest grid on
which segments interleave and keys reorder runs.  B = 1,000: 63 workgroups, the
earlier map (and a last workgroup with 8 rays).  The keys come from the
targets in the loss mode: all equal to the background colour (every key 0),
none equal to it (every key 4, and 2 or 0 at the end of B = 1,000), and the
first 300 rays background (keys 0 and 4 in every XCD's share, so the sort
moves runs)."""
from types import SimpleNamespace

import pytest
import torch

from gpu_support import OUT_KEYS, backward_after_loss_forward as backward, bits_equal
from test_gpu_fwd_resident import forward, scene, stored_tiles, workspace_marks

TARGETS = ("background", "none_background", "first_300_background")


def with_targets(s, kind, white):
    """The scene with its targets replaced (the scene itself is left unchanged)."""
    B = s.rays.shape[0]
    bg = 1.0 if white else 0.0
    t = 0.25 + 0.5 * s.target          # in [0.25, 0.75): no channel within 1/512 of 0 or 1
    if kind == "background":
        t = torch.full_like(t, bg)
    elif kind == "first_300_background":
        t = t.clone()
        t[:300] = bg
    else:
        assert kind == "none_background"
    assert t.shape == (B, 3)
    return SimpleNamespace(**dict(vars(s), target=t.contiguous()))


def compare_forms(HF, s, v, B):
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
    for k in OUT_KEYS:
        assert bits_equal(oa[k], ob[k]), k
    assert bits_equal(sa.fine_src, sb.fine_src), "fine_src"
    (fa, stored), (fb, _) = stored_tiles(sa, oa, v), stored_tiles(sb, ob, v)
    assert torch.equal(fa, fb), "feature cache and masks"
    assert torch.count_nonzero(fa[:, :8192]) > 0 and torch.count_nonzero(fa[:, 8192:]) > 0
    for raw in (oa["raw_c"], oa["raw_f"]):   # tiles of both kinds: the colour net skipped and run
        live = (raw[..., 3].reshape(B, -1, 32) > 0).any(-1)
        assert 0 < int(live.sum()) < live.numel()
    if v["loss"]:
        for name, x, y in zip(("d raw", "marks", "stamp"), ma, mb):
            assert bits_equal(x, y), name
        assert torch.count_nonzero(ma[0]) > 0 and torch.count_nonzero(ma[2]) > 0
        names = ("loss", "d_table") + tuple(f"NeRFSmall gradient {j}" for j in range(10))
        for name, x, y in zip(names, ga, gb):
            assert torch.equal(x, y), name
        assert torch.count_nonzero(ga[1]) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("targets", TARGETS)
@pytest.mark.parametrize("white", [True, False], ids=["white", "black"])
@pytest.mark.parametrize("B", [1024, 1000])
def test_dealt_forward_matches_ring_form_bitwise(hn, B, white, targets):
    """The trainer's forward (loss mode, skip_dead_color): the 13 outputs,
    fine_src, d raw, the marks, the stamp and the stored tiles, then the binned
    backward's loss value, table gradient and ten NeRFSmall gradients."""
    from hashnerf_pytorch_amd import functional as HF
    s = with_targets(scene(hn, B), targets, white)
    v = dict(loss=True, ni=128, skip=True, noise=False, white=white)
    compare_forms(HF, s, v, B)


@pytest.mark.gpu
def test_dealt_forward_without_loss(hn):
    """No targets: equal keys, so segments interleaved and the snake alone."""
    from hashnerf_pytorch_amd import functional as HF
    B = 1024
    v = dict(loss=False, ni=128, skip=True, noise=False, white=True)
    compare_forms(HF, scene(hn, B), v, B)
