"""hn_render_bwd_args.next_batch without a GPU: the ctypes mirror of
hn_next_batch against the header as gcc lays it out, the argument checks that
return before any launch, and the flags by which the Trainer decides whether a
self-driven step draws the next batch inside its backward."""
import ctypes as C
import os
import shutil
import subprocess
import types

import pytest
import torch

from conftest import ROOT

BOX = (torch.tensor([-1.5, -1.5, -1.5]), torch.tensor([1.5, 1.5, 1.5]))


def test_next_batch_struct_matches_compiled_header(hn, tmp_path):
    """Every field offset of hn_next_batch and of the hn_render_bwd_args that
    ends with it, as test_capi compiles the other structs."""
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    L = hn._lib
    structs = {"hn_next_batch": L.HnNextBatch, "hn_render_bwd_args": L.HnRenderBwdArgs}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "hashnerf_amd.h"', "int main(void) {"]
    for cname, cls in structs.items():
        lines.append(f'printf("{cname} sizeof %zu\\n", sizeof({cname}));')
        for f in cls._fields_:
            lines.append(f'printf("{cname} {f[0]} %zu\\n", offsetof({cname}, {f[0]}));')
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    got = {tuple(l.split()[:2]): int(l.split()[2]) for l in out if l.strip()}
    for cname, cls in structs.items():
        assert got[(cname, "sizeof")] == C.sizeof(cls), cname
        for f in cls._fields_:
            assert got[(cname, f[0])] == getattr(cls, f[0]).offset, (cname, f[0])
    assert L.HnRenderBwdArgs._fields_[-1][0] == "next_batch"          # appended: NULL in every older caller
    assert [f[0] for f in L.HnNextBatch._fields_] == ["sampler", "image", "c2w", "n_rays", "rays", "target",
                                                      "workspace", "ws_bytes", "seed", "draws", "n_draws"]


def test_next_batch_validation_without_gpu(hn):
    """A job is refused, with hn_sample_batch_morton's code for the same
    arguments, before anything is queued: no launch is reached on a machine
    without a device.  Where the launch has no lists and placement pair (no
    rays, deferred owner pass, float-atomic schedule) a job is HN_E_SHAPE."""
    L = hn._lib
    lib = L.lib()
    HF = hn.functional
    emb = hn.HashEmbedder(BOX, log2_hashmap_size=14, finest_resolution=64)
    cfg = HF.make_render_cfg(emb.grid(), True, False, True, scatter="binned")
    x = C.c_void_p(16)   # never dereferenced: validation happens before any launch
    B = 64
    ws = lib.hn_render_workspace_bytes(cfg, B)
    a = L.HnRenderBwdArgs()
    a.n_rays = B
    for k in ("rays", "table", "z_coarse", "z_fine", "raw_c", "raw_f", "fine_src", "feat", "d_table"):
        setattr(a, k, 16)
    for m in (a.coarse, a.fine, a.d_coarse, a.d_fine):
        for k in ("sigma0", "sigma1", "color0", "color1", "color2"):
            setattr(m, k, 16)
    a.weights_packed = 1
    s = L.HnRaySampler()
    s.H, s.W, s.crop_y0, s.crop_x0, s.crop_h, s.crop_w = 37, 29, 3, 5, 20, 13
    s.fx = s.fy = 30.0
    j = L.HnNextBatch()
    j.sampler = C.pointer(s)
    j.image = j.c2w = j.rays = j.target = j.workspace = 16
    j.ws_bytes = lib.hn_sample_rays_morton_workspace_bytes(s)
    a.next_batch = C.pointer(j)

    def both(want):
        alone = lib.hn_sample_batch_morton(j.sampler, j.image, j.c2w, j.n_rays, j.rays, j.target, j.workspace,
                                           j.ws_bytes, j.seed, j.draws, j.n_draws, None)
        assert alone == want
        assert lib.hn_render_bwd(cfg, a, x, ws, None) == want

    j.n_rays = 20 * 13 + 1
    both(2)                      # more rays than the window holds
    j.n_rays = -1
    both(2)
    j.n_rays, j.ws_bytes = 8, j.ws_bytes - 1
    both(3)                      # sampler workspace too small
    j.ws_bytes += 1
    j.target = None
    both(1)
    j.target = 16
    s.crop_w = 26                # window past the image
    both(2)
    s.crop_w = 13
    j.n_draws = 5
    both(2)                      # more than HN_UNIFORM_MAX_DRAWS
    j.n_draws = 1
    both(1)                      # no draws array
    d = (L.HnUniformDraw * 1)()
    d[0].numel, d[0].threads, d[0].offset = 8, 256, 2
    j.draws = d
    both(2)                      # offset not a multiple of 4
    j.n_draws, j.draws = 0, None
    j.sampler = None
    both(1)
    j.sampler = C.pointer(s)
    # no lists / placement pair to ride on
    a.owner_defer = 1
    assert lib.hn_render_bwd(cfg, a, x, ws, None) == 2
    a.owner_defer, a.n_rays = 0, 0
    assert lib.hn_render_bwd(cfg, a, x, ws, None) == 2
    a.n_rays = B
    cfg_a = HF.make_render_cfg(emb.grid(), True, False, True, scatter="atomic")
    assert lib.hn_render_scatter_mode(cfg_a, B) == 1
    assert lib.hn_render_bwd(cfg_a, a, x, lib.hn_render_workspace_bytes(cfg_a, B), None) == 2


def bare_trainer(hn, **over):
    """A Trainer with only the attributes its step plan reads (no device, no
    networks), at Trainer.__init__'s defaults."""
    from hashnerf_pytorch_amd.train import Trainer
    HF = hn.functional
    tr = Trainer.__new__(Trainer)
    tr.fuse_next_batch, tr.prefetch, tr.mode, tr.world = True, False, "explicit", 1
    tr.device, tr.use_batching, tr.ray_order, tr.fuse_table_step = torch.device("cuda", 0), False, 1, True
    tr.kw_train = dict(perturb=1.0)
    tr.skip_dead_rows = tr.dp_sharded = tr.fuse_mlp_step = tr.fuse_loss = tr.fuse_prepass = True
    tr._cfg = tr._xchg = None
    tr.dp_chunks, tr.dense_bwd = 1, False
    scatter = over.pop("scatter", "binned")
    emb = hn.HashEmbedder(BOX, log2_hashmap_size=14, finest_resolution=64)
    cfg = HF.make_render_cfg(emb.grid(), True, False, True, scatter=scatter)
    tr._binned = hn._lib.lib().hn_render_scatter_mode(cfg, 64) == 2      # as Trainer._fused_setup computes it
    for k, v in over.items():
        setattr(tr, k, v)
    return tr


def test_trainer_next_batch_flags(hn):
    """fuse_next_batch defaults to on and takes effect for one GPU, the
    binned schedule with the fused table step and the per-image Morton
    sampler; every other setting falls back to the sampler's own launches."""
    assert bare_trainer(hn)._fuses_next_batch() is True
    for over in (dict(world=2), dict(use_batching=True), dict(ray_order=0), dict(scatter="atomic"),
                 dict(fuse_table_step=False), dict(prefetch=True), dict(fuse_next_batch=False),
                 dict(mode="autograd"), dict(kw_train=dict(perturb=0.0)), dict(device=torch.device("cpu"))):
        assert bare_trainer(hn, **over)._fuses_next_batch() is False, over
    # the default of a constructed trainer, read off the class's initialiser
    import inspect
    from hashnerf_pytorch_amd.train import Trainer
    assert "self.fuse_next_batch = True" in inspect.getsource(Trainer.__init__)


def test_draw_batch_hands_out_or_refuses_pending(hn):
    """draw_batch(i) returns the batch drawn ahead for step i and raises for
    any other i while the mode holds (its random numbers are taken)."""
    tr = bare_trainer(hn)
    tr.global_step = 4
    tr.args = types.SimpleNamespace()
    tr.data = None
    batch = dict(rays=None)
    tr._nb = (5, batch)
    assert tr.draw_batch() is batch and tr._nb is None       # i = global_step + 1
    tr._nb = (5, batch)
    with pytest.raises(RuntimeError, match="step 5"):
        tr.draw_batch(7)
    assert tr._nb == (5, batch)                              # nothing discarded
    assert tr.draw_batch(5) is batch
