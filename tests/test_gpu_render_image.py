"""hn_render_image on the device (functional.render_image, render.render_image,
render_path(image_kernel=True)): against the reference's render of the
render_image fixture, bitwise against the training forward on the rays the
kernel itself made, the rays against get_rays, the empty field, repeatability,
and render_path's two paths."""
import numpy as np
import pytest
import torch

from conftest import golden, pcg_table
from gpu_support import MLP_KW, g2t, mostly_close, scene_from_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def fixture_scene(hn):
    """The reference's 12 x 14 render (168 rays: 42 ray groups, no multiple of 8)."""
    g = golden("render_image")
    sc = scene_from_golden(hn, g)
    emb, mc, mf = sc.emb, sc.mc, sc.mf
    kw = dict(network_query_fn=hn.NetworkQuery(emb, hn.SHEncoder()), perturb=0., N_importance=128,
              network_fine=mf, N_samples=64, network_fn=mc, embed_fn=emb, use_viewdirs=True,
              white_bkgd=True, raw_noise_std=0., ndc=False, lindisp=False, near=2., far=6., pytest=True)
    return g, kw


class Scene:
    """3 views of 37 x 43 pixels: 4,773 rays (odd sides, a count = 1 mod 4, more
    rays than the grid's 4,096 waves: every wave slot is reused and the last
    round is ragged), T = 14, finest 512, a random table and random nets."""
    V, H, W, T, NEAR, FAR = 3, 37, 43, 14, 2., 6.

    def __init__(self, hn):
        from hashnerf_pytorch_amd.train import SyntheticBlender
        torch.manual_seed(5)
        box = (torch.tensor([-1.5] * 3), torch.tensor([1.5] * 3))
        self.emb = hn.HashEmbedder(box, log2_hashmap_size=self.T, finest_resolution=512).to(DEV)
        with torch.no_grad():
            self.emb.table.copy_(g2t(pcg_table(41, self.T)))
        self.mc, self.mf = hn.NeRFSmall(**MLP_KW).to(DEV), hn.NeRFSmall(**MLP_KW).to(DEV)
        self.ws = [w.detach() for w in self.mc.weights() + self.mf.weights()]
        self.table = self.emb.table.detach()
        self.K = hn.rays.blender_intrinsics(self.H, self.W)[1]
        self.poses = SyntheticBlender(self.H, self.W, 7, DEV).poses[[0, 3, 5]].contiguous()   # [3, 4, 4]
        self.t_vals = torch.linspace(0., 1., 64).to(DEV)
        self.u = torch.linspace(0., 1., 128, device=DEV)

    def cfg(self, HF, white=True, lindisp=False):
        return HF.make_render_cfg(self.emb.grid(), white, lindisp, False)

    def image(self, HF, white=True, lindisp=False, poses=None, **kw):
        poses = self.poses if poses is None else poses
        return HF.render_image(self.cfg(HF, white, lindisp), self.H, self.W, self.K, poses, self.NEAR, self.FAR,
                               self.table, self.ws, **kw)

    def forward(self, HF, rays, white=True, lindisp=False, skip_dead_color=True, chunk=2048):
        """The training forward (inference mode) on a ray batch, in chunks."""
        outs = []
        with torch.no_grad():
            for i in range(0, rays.shape[0], chunk):
                r = rays[i:i + chunk]
                o, _ = HF.render_fwd(self.cfg(HF, white, lindisp), r, self.t_vals, None,
                                     self.u.expand(r.shape[0], 128), None, None, self.table, self.ws,
                                     keep_feat=False, skip_dead_color=skip_dead_color)
                outs.append(o)
        return {k: torch.cat([o[k] for o in outs], 0) for k in ("rgb", "depth", "acc")}


@pytest.fixture(scope="module")
def scene(hn):
    return Scene(hn)


@pytest.fixture(scope="module")
def scene_image(hn, scene):
    """The scene rendered once into NaN-filled outputs, with the kernel's rays."""
    from hashnerf_pytorch_amd import functional as HF
    V, H, W = scene.V, scene.H, scene.W
    out = tuple(torch.full(s, float("nan"), device=DEV) for s in ((V, H, W, 3), (V, H, W), (V, H, W)))
    rgb, depth, acc, rays = scene.image(HF, return_rays=True, out=out)
    torch.cuda.synchronize()
    return rgb, depth, acc, rays


def test_fixture_image_vs_reference(hn, fixture_scene):
    g, kw = fixture_scene
    H, W = int(g["H"]), int(g["W"])
    assert (H, W) == (12, 14)
    rgb, depth, acc = hn.render_image(H, W, g["K"], g2t(g["c2w"]), **kw)
    assert rgb.shape == (H, W, 3) and depth.shape == (H, W) and acc.shape == (H, W)
    mostly_close(rgb.reshape(-1, 3), g["rgb"].reshape(-1, 3), rtol=1e-4, atol=1e-5, frac=0.6, loose=2e-2, msg="rgb")
    mostly_close(acc.reshape(-1), g["acc"].reshape(-1), rtol=1e-4, atol=1e-5, frac=0.6, loose=2e-2, msg="acc")


def test_every_pixel_written(scene_image):
    for t in scene_image:
        assert not bool(torch.isnan(t).any())


@pytest.mark.parametrize("skip_dead_color", [True, False])
def test_bitwise_training_forward_on_the_kernels_rays(hn, scene, scene_image, skip_dead_color):
    """rgb, depth and acc are render_fwd's on the same rays, with the colour
    skip (what the kernel runs) and without it (what the header promises for
    that flag: no output changes)."""
    from hashnerf_pytorch_amd import functional as HF
    rgb, depth, acc, rays = scene_image
    ref = scene.forward(HF, rays, skip_dead_color=skip_dead_color)
    V, H, W = scene.V, scene.H, scene.W
    assert torch.equal(rgb, ref["rgb"].reshape(V, H, W, 3))
    assert torch.equal(depth, ref["depth"].reshape(V, H, W))
    assert torch.equal(acc, ref["acc"].reshape(V, H, W))


def test_bitwise_training_forward_black_lindisp(hn, scene):
    from hashnerf_pytorch_amd import functional as HF
    rgb, depth, acc, rays = scene.image(HF, white=False, lindisp=True, return_rays=True)
    ref = scene.forward(HF, rays, white=False, lindisp=True)
    V, H, W = scene.V, scene.H, scene.W
    assert torch.equal(rgb, ref["rgb"].reshape(V, H, W, 3))
    assert torch.equal(depth, ref["depth"].reshape(V, H, W))
    assert torch.equal(acc, ref["acc"].reshape(V, H, W))


def test_rays_and_pixel_placement(hn, scene, scene_image):
    """rays[v, j, i] is get_rays' ray of pixel (row j, column i) of view v
    (rtol 1e-6, the device sampler's tolerance: the same fp32 expressions,
    torch's 3-term sum order is not specified)."""
    from hashnerf_pytorch_amd import functional as HF
    V, H, W = scene.V, scene.H, scene.W
    rays = scene_image[3].reshape(V, H, W, 11)
    for v in range(V):
        c2w = scene.poses[v, :3, :4]
        ro, rd = hn.get_rays(H, W, scene.K, c2w)
        torch.testing.assert_close(rays[v, ..., 3:6], rd, rtol=1e-6, atol=1e-6)
        torch.testing.assert_close(rays[v, ..., 0:3], ro.expand(H, W, 3), rtol=0, atol=0)
        vd = rd / torch.norm(rd, dim=-1, keepdim=True)
        torch.testing.assert_close(rays[v, ..., 8:11], vd, rtol=1e-6, atol=1e-6)
    assert torch.equal(rays[..., 6], torch.full((V, H, W), scene.NEAR, device=DEV))
    assert torch.equal(rays[..., 7], torch.full((V, H, W), scene.FAR, device=DEV))
    # [n, 3, 4] poses (stride 12) give the same rays and the same images as [n, 4, 4] (stride 16)
    out12 = scene.image(HF, poses=scene.poses[:, :3, :4].contiguous(), return_rays=True)
    for a, b in zip(out12, scene_image):
        assert torch.equal(a, b)


def test_design_alternatives_render_the_same_images(hn, scene, scene_image):
    """hn_render_image_variant: re-encoding every fine sample, and the
    row-major ray order, change no bit of any output."""
    from hashnerf_pytorch_amd import functional as HF
    bits = hn._lib.IMAGE_VARIANTS
    for variant in (bits["reencode"], bits["row_major"], bits["reencode"] | bits["row_major"]):
        out = scene.image(HF, return_rays=True, variant=variant)
        for a, b in zip(out, scene_image):
            assert torch.equal(a, b), variant


def test_empty_field(hn, scene):
    """An all-zero table: no sample has density, every tile skips its colours."""
    from hashnerf_pytorch_amd import functional as HF
    H, W = 9, 5
    cfg = scene.cfg(HF)
    zero = torch.zeros_like(scene.table)
    rgb, depth, acc, rays = HF.render_image(cfg, H, W, scene.K, scene.poses[:1], scene.NEAR, scene.FAR, zero,
                                            scene.ws, return_rays=True)
    assert torch.equal(rgb, torch.ones_like(rgb))
    assert torch.equal(acc, torch.zeros_like(acc))
    with torch.no_grad():
        ref, _ = HF.render_fwd(cfg, rays, scene.t_vals, None, scene.u.expand(H * W, 128), None, None, zero,
                               scene.ws, keep_feat=False)
    # (no weight anywhere: the reference's depth map is 0 / 0 here, so the bits are compared)
    assert torch.equal(depth.reshape(-1).view(torch.int32), ref["depth"].view(torch.int32))


def test_repeatable(hn, scene, scene_image):
    from hashnerf_pytorch_amd import functional as HF
    again = scene.image(HF)
    for a, b in zip(again, scene_image[:3]):
        assert torch.equal(a, b)


def test_render_path_image_kernel(hn, fixture_scene):
    g, kw = fixture_scene
    H, W = int(g["H"]), int(g["W"])
    c2w = g2t(g["c2w"])
    other = hn.pose_spherical(40., -35., 4.).to(DEV)[:3, :4]
    poses = torch.stack([c2w, other], 0)
    rgb, depth, acc = hn.render_image(H, W, g["K"], poses, **kw)
    assert rgb.shape == (2, H, W, 3)
    gt = list(rgb.cpu().numpy() * 0.5 + 0.1)
    rgbs, depths = hn.render_path(poses, (H, W, None), g["K"], 50, dict(kw), gt_imgs=gt, image_kernel=True)
    np.testing.assert_array_equal(rgbs, rgb.cpu().numpy())
    np.testing.assert_allclose(depths, ((depth - 2.) / 4.).cpu().numpy(), rtol=1e-6, atol=1e-7)
    psnrs = hn.render_path.last_psnrs
    assert len(psnrs) == 2 and np.all(np.isfinite(psnrs))
    np.testing.assert_allclose(psnrs, [-10. * np.log10(np.mean(np.square(rgbs[i] - gt[i]))) for i in range(2)])
    # the default path renders the same scene within the reference test's own tolerances
    rgbs0, _ = hn.render_path(poses, (H, W, None), g["K"], 50, dict(kw))
    np.testing.assert_allclose(rgbs, rgbs0, rtol=0, atol=2e-2)


def test_render_path_image_kernel_ineligible_is_the_default_path(hn, fixture_scene):
    g, kw = fixture_scene
    H, W = int(g["H"]), int(g["W"])
    poses = torch.stack([g2t(g["c2w"])] * 2, 0)
    kw = dict(kw, perturb=1., pytest=False)
    torch.manual_seed(11)
    a = hn.render_path(poses, (H, W, None), g["K"], 50, dict(kw), image_kernel=True)
    torch.manual_seed(11)
    b = hn.render_path(poses, (H, W, None), g["K"], 50, dict(kw), image_kernel=False)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


def test_render_image_refuses_ineligible(hn, fixture_scene):
    g, kw = fixture_scene
    c2w = g2t(g["c2w"])
    for bad, why in ((dict(ndc=True), "ndc"), (dict(perturb=1.), "perturb"), (dict(raw_noise_std=1.), "noise"),
                     (dict(use_viewdirs=False), "view directions"), (dict(retraw=True), "retraw"),
                     (dict(c2w_staticcam=c2w), "staticcam")):
        with pytest.raises(ValueError, match=why):
            hn.render_image(12, 14, g["K"], c2w, **dict(kw, **bad))
