"""hn_render_fwd_form's form argument is validated on the host, by the wrapper
and by the library, before any launch (no GPU needed)."""
import ctypes as C

import pytest
import torch

T, FINEST = 14, 64


def test_wrapper_refuses_an_invalid_form(hn):
    L, HF = hn._lib, hn.functional
    assert L.FWD_FORMS == {"auto": 0, "ring": 1, "resident": 2}
    for name, value in L.FWD_FORMS.items():
        assert L.fwd_form(name) == value == L.fwd_form(value)
    for bad in ("lds", "", 3, -1, 1.0, True, None):
        with pytest.raises(ValueError, match="form"):
            L.fwd_form(bad)
    # render_fwd checks it first: nothing else of the call is looked at
    with pytest.raises(ValueError, match="form"):
        HF.render_fwd(None, None, None, None, None, None, None, None, None, False, form=3)
    assert HF.FWD_FORM == "auto"


def test_wrapper_refuses_an_invalid_default_form(hn, monkeypatch):
    HF = hn.functional
    monkeypatch.setattr(HF, "FWD_FORM", "fastest")
    with pytest.raises(ValueError, match="form"):
        HF.render_fwd(None, None, None, None, None, None, None, None, None, False)


def test_library_refuses_an_invalid_form_before_any_launch(hn):
    L = hn._lib
    lib = L.lib()
    HF = hn.functional
    box = (torch.tensor([-1.5, -1.5, -1.5]), torch.tensor([1.5, 1.5, 1.5]))
    emb = hn.HashEmbedder(box, log2_hashmap_size=T, finest_resolution=FINEST)
    cfg = HF.make_render_cfg(emb.grid(), True, False, False, scatter="binned")
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
    for form in (3, -1, 255):
        assert lib.hn_render_fwd_form(cfg, f, form, C.c_void_p(x), ws, None) == 2          # HN_E_SHAPE
    # a valid form goes on to hn_render_fwd's own checks, with hn_render_fwd's answers
    f.rgb = None
    for form in (0, 1, 2):
        assert lib.hn_render_fwd_form(cfg, f, form, C.c_void_p(x), ws, None) == 1          # HN_E_NULL
    assert lib.hn_render_fwd(cfg, f, C.c_void_p(x), ws, None) == 1
    f.rgb = x
    for form in (0, 1, 2):
        assert lib.hn_render_fwd_form(cfg, f, form, C.c_void_p(x), ws - 1, None) == \
            lib.hn_render_fwd(cfg, f, C.c_void_p(x), ws - 1, None) != 0                     # workspace too small
    f.n_rays = 0
    assert lib.hn_render_fwd_form(cfg, f, 2, C.c_void_p(x), ws, None) == 0                 # no rays: no launch
    assert lib.hn_render_fwd_form(cfg, f, 3, C.c_void_p(x), ws, None) == 2
