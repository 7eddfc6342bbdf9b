"""hn_render_views on the device (functional.render_views, render.render_views,
render_path(image_kernel=True) on an LLFF configuration): the reference's NDC
64 + 64 render of the render_views_llff fixture, every (count, ndc) pair
bitwise against the training forward on the rays the kernel itself made, the
NDC rays bitwise against get_ndc_rays, the variants, the empty field,
repeatability, render_path's two paths, and the old names' refusals."""
import numpy as np
import pytest
import torch

from conftest import golden, pcg_table
from gpu_support import MLP_KW, bits_equal, done, g2t, mostly_close, scene_from_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAIRS = [(64, True), (64, False), (128, True), (128, False)]


@pytest.fixture(scope="module")
def fixture_scene(hn):
    """The reference's 11 x 14 NDC render at 64 + 64 (154 rays: 42 ray groups, a cut last row of blocks)."""
    g = golden("render_views_llff")
    sc = scene_from_golden(hn, g)
    emb, mc, mf = sc.emb, sc.mc, sc.mf
    kw = dict(network_query_fn=hn.NetworkQuery(emb, hn.SHEncoder()), perturb=0., N_importance=64,
              network_fine=mf, N_samples=64, network_fn=mc, embed_fn=emb, use_viewdirs=True,
              white_bkgd=False, raw_noise_std=0., ndc=True, lindisp=False, near=0., far=1., pytest=True)
    return g, kw


def llff_poses(n, seed):
    """Near-identity forward-facing poses (cameras looking down -z, as LLFF's
    recentred ones): d_z of every pixel's ray is close to -1, never 0."""
    g = np.random.Generator(np.random.PCG64(seed))
    poses = np.zeros((n, 3, 4), dtype=np.float32)
    for p in poses:
        a = g.normal(0., 0.08, 3)
        rx = np.array([[1, 0, 0], [0, np.cos(a[0]), -np.sin(a[0])], [0, np.sin(a[0]), np.cos(a[0])]])
        ry = np.array([[np.cos(a[1]), 0, np.sin(a[1])], [0, 1, 0], [-np.sin(a[1]), 0, np.cos(a[1])]])
        rz = np.array([[np.cos(a[2]), -np.sin(a[2]), 0], [np.sin(a[2]), np.cos(a[2]), 0], [0, 0, 1]])
        p[:, :3] = (rz @ ry @ rx).astype(np.float32)
        p[:, 3] = g.normal(0., 0.15, 3).astype(np.float32)
    return poses


class Scene:
    """test_gpu_render_image.Scene's shape -- 3 views of 37 x 43 pixels: 4,773
    rays (odd sides, more rays than the grid's 4,096 waves, a ragged last
    round), T = 14, finest 512, a pcg_table and random nets -- from
    forward-facing poses.  NDC: near 0, far 1, the box bbox_for_llff's; world
    rays: near 2, far 6 and a box around those segments."""
    V, H, W, T, FOCAL = 3, 37, 43, 14, 40.

    def __init__(self, hn, ndc):
        torch.manual_seed(5)
        self.ndc = ndc
        poses = llff_poses(self.V, 43)
        if ndc:
            self.near, self.far = 0., 1.
            box = hn.bbox_for_llff(poses, (self.H, self.W, self.FOCAL))
        else:
            self.near, self.far = 2., 6.
            box = (torch.tensor([-4.5, -4.5, -7.]), torch.tensor([4.5, 4.5, -1.]))
        self.emb = hn.HashEmbedder(box, log2_hashmap_size=self.T, finest_resolution=512).to(DEV)
        with torch.no_grad():
            self.emb.table.copy_(g2t(pcg_table(41, self.T)))
        self.mc, self.mf = hn.NeRFSmall(**MLP_KW).to(DEV), hn.NeRFSmall(**MLP_KW).to(DEV)
        self.ws = [w.detach() for w in self.mc.weights() + self.mf.weights()]
        self.table = self.emb.table.detach()
        self.K = np.array([[self.FOCAL, 0, 0.5 * self.W], [0, self.FOCAL, 0.5 * self.H], [0, 0, 1]])
        self.poses = g2t(poses)   # [3, 3, 4]
        self.t_vals = torch.linspace(0., 1., 64).to(DEV)

    def cfg(self, HF, ni, white=True, lindisp=False):
        return HF.make_render_cfg(self.emb.grid(), white, lindisp, False, n_importance=ni)

    def views(self, HF, ni, white=True, lindisp=False, poses=None, table=None, H=None, W=None, ndc=None, **kw):
        return HF.render_views(self.cfg(HF, ni, white, lindisp), H or self.H, W or self.W, self.K,
                               self.poses if poses is None else poses, self.near, self.far,
                               self.table if table is None else table, self.ws,
                               ndc=self.ndc if ndc is None else ndc, **kw)

    def forward(self, HF, ni, rays, white=True, lindisp=False, skip_dead_color=True, table=None, chunk=2048):
        """The training forward (inference mode) on a ray batch, in chunks."""
        u = torch.linspace(0., 1., ni, device=DEV)
        outs = []
        with torch.no_grad():
            for i in range(0, rays.shape[0], chunk):
                r = rays[i:i + chunk]
                o, _ = HF.render_fwd(self.cfg(HF, ni, white, lindisp), r, self.t_vals, None, u.expand(r.shape[0], ni),
                                     None, None, self.table if table is None else table, self.ws, keep_feat=False,
                                     skip_dead_color=skip_dead_color)
                outs.append(o)
        return {k: torch.cat([o[k] for o in outs], 0) for k in ("rgb", "depth", "acc")}


@pytest.fixture(scope="module")
def scenes(hn):
    return {True: Scene(hn, True), False: Scene(hn, False)}


@pytest.fixture(scope="module")
def rendered(hn, scenes):
    """Every (count, ndc) pair rendered once into NaN-filled outputs, with the kernel's rays."""
    from hashnerf_pytorch_amd import functional as HF
    out = {}
    for ni, ndc in PAIRS:
        sc = scenes[ndc]
        V, H, W = sc.V, sc.H, sc.W
        nan = tuple(torch.full(s, float("nan"), device=DEV) for s in ((V, H, W, 3), (V, H, W), (V, H, W)))
        out[(ni, ndc)] = sc.views(HF, ni, return_rays=True, out=nan)
    done()
    return out


def assert_images_are_the_forwards(sc, got, ref):
    V, H, W = sc.V, sc.H, sc.W
    rgb, depth, acc = got[:3]
    assert torch.equal(rgb, ref["rgb"].reshape(V, H, W, 3))
    assert torch.equal(depth, ref["depth"].reshape(V, H, W))
    assert torch.equal(acc, ref["acc"].reshape(V, H, W))


def test_fixture_views_vs_reference(hn, fixture_scene):
    """test_fixture_image_vs_reference's comparison, the fractions printed
    (measured on an MI355X: 0.987 of the 154 rays within (1e-4, 1e-5) for rgb
    and for acc, largest differences 2.9e-5 and 5.6e-5)."""
    g, kw = fixture_scene
    H, W = int(g["H"]), int(g["W"])
    assert (H, W) == (11, 14)
    rgb, depth, acc = hn.render_views(H, W, g["K"], g2t(g["c2w"]), **kw)
    assert rgb.shape == (H, W, 3) and depth.shape == (H, W) and acc.shape == (H, W)
    for name, a, b in (("rgb", rgb.reshape(-1, 3), g["rgb"].reshape(-1, 3)),
                       ("acc", acc.reshape(-1, 1), g["acc"].reshape(-1, 1))):
        a2 = a.cpu().numpy()
        frac = np.isclose(a2, b, rtol=1e-4, atol=1e-5).all(-1).mean()
        print(f"render_views_llff {name}: {frac:.4f} of {a.shape[0]} rays within (1e-4, 1e-5), "
              f"max |diff| {np.abs(a2 - b).max():.3e}")
        mostly_close(a, b, rtol=1e-4, atol=1e-5, frac=0.6, loose=2e-2, msg=name)
    acc_np = acc.cpu().numpy()
    assert ((acc_np > 0.05) & (acc_np < 0.95)).any()     # the composite is exercised
    done()


@pytest.mark.parametrize("skip_dead_color", [True, False])
@pytest.mark.parametrize("ni,ndc", [(64, True), (64, False), (128, True)])
def test_bitwise_training_forward_on_the_kernels_rays(hn, scenes, rendered, ni, ndc, skip_dead_color):
    """rgb, depth and acc are render_fwd's on the same rays under the same cfg,
    with the colour skip (what the kernel runs) and without it."""
    from hashnerf_pytorch_amd import functional as HF
    sc, got = scenes[ndc], rendered[(ni, ndc)]
    assert_images_are_the_forwards(sc, got, sc.forward(HF, ni, got[3], skip_dead_color=skip_dead_color))
    done()


def test_bitwise_training_forward_black_lindisp(hn, scenes):
    """(64, world): lindisp needs near > 0, which NDC's near = 0 is not."""
    from hashnerf_pytorch_amd import functional as HF
    sc = scenes[False]
    got = sc.views(HF, 64, white=False, lindisp=True, return_rays=True)
    assert_images_are_the_forwards(sc, got, sc.forward(HF, 64, got[3], white=False, lindisp=True))
    done()


def test_128_world_is_render_image(hn, scenes, rendered):
    from hashnerf_pytorch_amd import functional as HF
    sc = scenes[False]
    old = HF.render_image(sc.cfg(HF, 128), sc.H, sc.W, sc.K, sc.poses, sc.near, sc.far, sc.table, sc.ws,
                          return_rays=True)
    for a, b in zip(rendered[(128, False)], old):
        assert torch.equal(a, b)
    done()


@pytest.mark.parametrize("ni,ndc", PAIRS)
def test_every_pixel_written(rendered, ni, ndc):
    for t in rendered[(ni, ndc)]:
        assert not bool(torch.isnan(t).any())
    done()


def test_ndc_rays_are_get_ndc_rays_bitwise(hn, scenes):
    """The kernel's NDC step against torch's on the kernel's own world rays:
    one correctly rounded float32 operation after the other in the same order
    on both sides, so every bit agrees; near, far and the view directions are
    the world ray's."""
    from hashnerf_pytorch_amd import functional as HF
    sc = scenes[True]
    V, H, W = sc.V, sc.H, sc.W
    world = sc.views(HF, 64, ndc=False, return_rays=True)[3]
    ndc = sc.views(HF, 64, ndc=True, return_rays=True)[3]
    assert torch.equal(world[:, 6:11], ndc[:, 6:11])
    o, d = hn.get_ndc_rays(H, W, float(sc.K[0][0]), 1., world[:, 0:3], world[:, 3:6])
    assert torch.equal(ndc[:, 0:3], o)
    assert torch.equal(ndc[:, 3:6], d)
    assert bool(torch.isfinite(ndc).all())
    # the world rays against get_rays (the existing test's tolerance: torch's 3-term sum order is not specified)
    rays = world.reshape(V, H, W, 11)
    for v in range(V):
        ro, rd = hn.get_rays(H, W, sc.K, sc.poses[v])
        torch.testing.assert_close(rays[v, ..., 3:6], rd, rtol=1e-6, atol=1e-6)
        torch.testing.assert_close(rays[v, ..., 0:3], ro.expand(H, W, 3), rtol=0, atol=0)
        vd = rd / torch.norm(rd, dim=-1, keepdim=True)
        torch.testing.assert_close(rays[v, ..., 8:11], vd, rtol=1e-6, atol=1e-6)
    assert torch.equal(ndc[:, 6], torch.zeros(V * H * W, device=DEV))
    assert torch.equal(ndc[:, 7], torch.ones(V * H * W, device=DEV))
    done()


def test_variants_render_the_same_images(hn, scenes, rendered):
    """At (64, ndc): re-encoding every fine sample, the row-major ray order and
    both change no bit of any output."""
    from hashnerf_pytorch_amd import functional as HF
    bits = hn._lib.IMAGE_VARIANTS
    for variant in (bits["reencode"], bits["row_major"], bits["reencode"] | bits["row_major"]):
        out = scenes[True].views(HF, 64, return_rays=True, variant=variant)
        for a, b in zip(out, rendered[(64, True)]):
            assert torch.equal(a, b), variant
    done()


def test_empty_field(hn, scenes):
    """(64, ndc), black background, an all-zero table: no sample has density."""
    from hashnerf_pytorch_amd import functional as HF
    sc = scenes[True]
    H, W = 9, 5
    zero = torch.zeros_like(sc.table)
    rgb, depth, acc, rays = sc.views(HF, 64, white=False, poses=sc.poses[:1], table=zero, H=H, W=W, return_rays=True)
    assert torch.equal(rgb, torch.zeros_like(rgb))
    assert torch.equal(acc, torch.zeros_like(acc))
    ref = sc.forward(HF, 64, rays, white=False, table=zero)
    # (no weight anywhere: the reference's depth map is 0 / 0 here, so the bits are compared)
    assert bits_equal(depth.reshape(-1), ref["depth"])
    done()


def test_repeatable(hn, scenes, rendered):
    from hashnerf_pytorch_amd import functional as HF
    again = scenes[True].views(HF, 64)
    for a, b in zip(again, rendered[(64, True)][:3]):
        assert torch.equal(a, b)
    done()


def test_u_width_follows_the_cfg(hn, scenes):
    from hashnerf_pytorch_amd import functional as HF
    with pytest.raises(ValueError, match="u 64 values"):
        scenes[True].views(HF, 64, u=torch.linspace(0., 1., 128, device=DEV))
    done()


def test_render_path_image_kernel_llff(hn, fixture_scene):
    g, kw = fixture_scene
    H, W = int(g["H"]), int(g["W"])
    poses = g2t(llff_poses(2, 47))
    poses[0] = g2t(g["c2w"])
    rgb, depth, acc = hn.render_views(H, W, g["K"], poses, **kw)
    assert rgb.shape == (2, H, W, 3)
    gt = list(rgb.cpu().numpy() * 0.5 + 0.1)
    rgbs, depths = hn.render_path(poses, (H, W, None), g["K"], 50, dict(kw), gt_imgs=gt, image_kernel=True)
    np.testing.assert_array_equal(rgbs, rgb.cpu().numpy())
    np.testing.assert_array_equal(depths, ((depth - 0.) / (1. - 0.)).cpu().numpy())
    psnrs = hn.render_path.last_psnrs
    assert len(psnrs) == 2 and np.all(np.isfinite(psnrs))
    np.testing.assert_allclose(psnrs, [-10. * np.log10(np.mean(np.square(rgbs[i] - gt[i]))) for i in range(2)])
    # the default path renders the same poses within the existing test's tolerance
    rgbs0, _ = hn.render_path(poses, (H, W, None), g["K"], 50, dict(kw))
    np.testing.assert_allclose(rgbs, rgbs0, rtol=0, atol=2e-2)
    done()


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
    done()


def test_old_names_keep_refusing(hn, fixture_scene):
    g, kw = fixture_scene
    c2w = g2t(g["c2w"])
    with pytest.raises(ValueError, match="N_importance"):
        hn.render_image(11, 14, g["K"], c2w, **dict(kw, ndc=False))
    with pytest.raises(ValueError, match="ndc"):
        hn.render_image(11, 14, g["K"], c2w, **dict(kw, N_importance=128))
    done()
