"""Digest of one fused forward + backward at the bench shape (4096 rays,
T=19, seeded inputs) with the library HN_LIB_PATH selects: sha256 of the
table gradient, the ten MLP gradients and the forward state, and of
hn_render_image's outputs on the image test's scene (3 views of 37 x 43, T =
14), so that variant libraries that must be bitwise equal can be compared
across processes.  Then the paths the fused step does not take: the stand-
alone composite kernels (37 rays, white background, raw noise), the 64 + 64
form's forward state and the ray gradients (B = 259, T = 14), and the input
gradients of the stand-alone NeRFSmall backward (96 points; its weight
gradients are LDS float atomics across waves, not repeatable).
  usage: HN_LIB_PATH=... python scripts/variant_digest.py [B] [T] [finest]"""
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hn_loader  # noqa: E402

hn = hn_loader.load()
from gpu_support import DEV, blender_state, bwd  # noqa: E402
from test_gpu_render_image import Scene  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
T = int(sys.argv[2]) if len(sys.argv) > 2 else 19
fin = int(sys.argv[3]) if len(sys.argv) > 3 else 512
s = blender_state(hn, B, T, 31, "binned", finest=fin)
HF, st = s.HF, s.st
h = lambda *ts: hashlib.sha256(b"".join(t.detach().contiguous().cpu().numpy().tobytes() for t in ts)).hexdigest()[:16]
f0 = h(st.z_f, st.raw_c, st.raw_f, st.feat)   # the forward state before the backward runs
tab, dws = bwd(s)
f1 = h(st.z_f, st.raw_c, st.raw_f, st.feat)
print(f"fwd {f0} table {h(tab)} mlp {h(*dws)}" + ("" if f1 == f0 else f" CHANGED-BY-BWD {f1}"))
if os.environ.get("HN_DIGEST_PARTS"):
    print("  parts z_f %s raw_c %s raw_f %s feat %s" % (h(st.z_f), h(st.raw_c), h(st.raw_f), h(st.feat)))
print("image " + h(*Scene(hn).image(HF, return_rays=True)))   # rgb, depth, acc, rays
gen = torch.Generator(device=DEV).manual_seed(5)
rnd = lambda *shape: torch.randn(shape, device=DEV, generator=gen)
for S in (64, 128, 192):
    raw, z, d = rnd(37, S, 4).requires_grad_(), torch.rand(37, S, device=DEV, generator=gen).sort(-1)[0], rnd(37, 3)
    out = HF.CompositeFn.apply(raw, z.requires_grad_(), d.requires_grad_(), rnd(37, S), True)
    torch.autograd.backward(out, [rnd(*o.shape) for o in out])   # hn_composite_bwd and hn_composite_bwd_inputs
    print(f"composite S={S} fwd {h(*out)} d_raw {h(raw.grad)} d_inputs {h(z.grad, d.grad)}")
for ni in (64, 128):
    s = blender_state(hn, 259, 14, 31, "binned", ni=ni)
    print(f"ni={ni} B=259 fwd {h(s.st.z_f, s.st.raw_c, s.st.raw_f, s.st.feat)} d_rays {h(HF.render_bwd_rays(s.st, s.grads))}")
x = rnd(96, 48).requires_grad_()
HF.NeRFSmallFn.apply(x, *(w.detach() for w in s.mc.weights())).backward(rnd(96, 4))
print(f"mlp_bwd d_x {h(x.grad)}")
