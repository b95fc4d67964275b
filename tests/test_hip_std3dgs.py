"""GSX_SEM_STD_3DGS on the GPU (through gsx_render_forward) against the C restatement of the
published 3DGS forward pass (oracle/raster_cpu.c:orc_render_std3dgs; PARITY UNPINNED, see there).

Bar: the counts (visible Gaussians, tile instances) are equal -- stage 1 shares the float32
operation order -- and pixels agree to 1e-4 except where the rule set itself is discontinuous.  It
has three discontinuities, and either side's rounding (v_exp_f32 against libm expf, exp2 of a
prescaled exponent against exp, T - T alpha against T (1 - alpha)) can put a pair on the other side
of each: a Gaussian whose alpha is within rounding of 1/255 is skipped by one side and composited by
the other (up to 0.99/255 of its colour times T); a pixel whose T (1 - alpha) is within rounding of
1e-4 stops on one side and takes that Gaussian and those behind it on the other (up to T of colour,
0.01 after one clamped alpha); an exponent within rounding of 0 (a pixel on the mean of a
degenerate conic) is skipped or used.  Such pixels must be rare (<= 1e-5 of the frame + 2) and the
excursion bounded by 0.006 -- and every one of them must be EXPLAINED: the float64 restatement
(tests/rule_set_restatement.py) must find a decision within float32's reach of its threshold at
that pixel, and both frames must lie within 12 E_REF of one of the colours the flips lead to.
tests/test_hip_rule_sets.py holds every pixel of the small cases to that restatement.
"""
import numpy as np
import pytest
import torch

from test_hip_parity import _need_gpu, _oracle_cam, _scene_from_arrays

pytestmark = pytest.mark.gpu


def _std_oracle(scene, sc, tile=16, background=(0.0, 0.0, 0.0), window=None):
    from oracle import c_oracle

    cam = _oracle_cam(scene)
    return c_oracle.render_std3dgs(sc["points"], scene.gaussians.colors.cpu().numpy(), sc["scales"],
                                   sc["quaternions"], sc["opacity"], cam, tile=tile, background=background,
                                   window=window)


def _check(img_hw3, ref, what=""):
    d = np.abs(img_hw3.astype(np.float64) - ref.astype(np.float64)).max(axis=-1)
    bad = int((d > 1e-4).sum())
    assert bad <= 2 + int(1e-5 * d.size), (what, bad, float(d.max()))
    assert d.max() < 0.006, (what, float(d.max()))
    return float(d.max()), bad


def _explained(img_hw3, ref, rows, colors, tile, background, what=""):
    """Every pixel beyond 1e-4 is an ambiguous pixel of the float64 walk, and kernel and port each match one of its
    alternatives.  The walk runs only when there is such a pixel."""
    import rule_set_restatement as rsr
    from test_rule_sets_host import BOUND

    if not (np.abs(img_hw3.astype(np.float64) - ref.astype(np.float64)) > 1e-4).any():
        return
    h, w = ref.shape[:2]
    wk = rsr.walk(rsr.STD_3DGS, rsr.records_std3dgs(rows, colors, w, h, tile), w, h, background)
    bad = rsr.explain_excursions(wk, img_hw3, ref, 1e-4, BOUND["std_3dgs"])
    assert not bad, (what, bad[:8])


@pytest.mark.parametrize("n,w,h,tile,seed,behind", [(2000, 256, 256, 16, 0, 0.0), (3000, 200, 150, 16, 1, 0.2),
                                                     (1500, 130, 70, 8, 2, 0.1), (1000, 96, 80, 32, 3, 0.0),
                                                     (800, 64, 64, 2, 4, 0.0), (50000, 640, 360, 16, 5, 0.05)])
def test_std3dgs_matches_oracle(tmp_path, n, w, h, tile, seed, behind):
    _need_gpu()
    from intro_to_gaussian_splatting_amd.synthetic import make_scene

    sc = make_scene(n, w, h, seed=seed, behind_fraction=behind)
    scene = _scene_from_arrays(tmp_path, sc)
    bg = (0.25, 0.5, 0.75)
    ref, nvis, inst, rows = _std_oracle(scene, sc, tile=tile, background=bg)
    stats = {}
    img = scene.render_image_hip(1, tile_size=tile, layout="hw3", semantics="std_3dgs", background=bg, stats=stats,
                                 published_rects=True)
    assert tuple(img.shape) == (h, w, 3)
    assert stats["n_visible"] == nvis and stats["n_instances"] == inst
    _check(img.cpu().numpy(), ref, "hw3")
    if w * h <= 256 * 256:                                     # the float64 walk is numpy: not for the 640x360 frame
        _explained(img.cpu().numpy(), ref, rows, scene.gaussians.colors.cpu().numpy(), tile, bg, "hw3")
    # default binning (bounding box of the alpha >= 1/255 ellipse): shorter lists, the same frame bit for bit
    tight = {}
    img_t = scene.render_image_hip(1, tile_size=tile, layout="hw3", semantics="std_3dgs", background=bg, stats=tight)
    assert torch.equal(img_t, img)
    assert tight["n_visible"] == nvis and tight["n_instances"] <= inst
    if n >= 1000:
        assert tight["n_instances"] < inst
    img_wh3 = scene.render_image_hip(1, tile_size=tile, layout="wh3", semantics="std_3dgs", background=bg)
    assert torch.equal(img_wh3.permute(1, 0, 2), img)          # same kernel arithmetic, other store addressing


def test_std3dgs_tile_windows_assemble_to_the_frame(tmp_path):
    _need_gpu()
    from intro_to_gaussian_splatting_amd.synthetic import make_scene

    w, h = 200, 120
    sc = make_scene(4000, w, h, seed=7)
    scene = _scene_from_arrays(tmp_path, sc)
    full = scene.render_image_hip(1, layout="hw3", semantics="std_3dgs")
    ntx, nty = (w + 15) // 16, (h + 15) // 16
    acc = torch.zeros_like(full)
    total = 0
    for (x0, x1) in ((0, 5), (5, ntx)):
        for (y0, y1) in ((0, 3), (3, nty)):
            st = {}
            part = scene.render_image_hip(1, layout="hw3", semantics="std_3dgs", tile_window=(x0, x1, y0, y1), stats=st)
            total += st["n_instances"]
            ys, xs = slice(y0 * 16, min(y1 * 16, h)), slice(x0 * 16, min(x1 * 16, w))
            assert torch.equal(part[ys, xs], full[ys, xs])
            mask = torch.ones((h, w), dtype=torch.bool, device=part.device)
            mask[ys, xs] = False
            assert not part[mask].any()
            acc += part
    assert torch.equal(acc, full)
    st = {}
    scene.render_image_hip(1, layout="hw3", semantics="std_3dgs", stats=st)
    assert total == st["n_instances"]


def test_std3dgs_empty_scene_is_background(tmp_path):
    _need_gpu()
    from intro_to_gaussian_splatting_amd.synthetic import make_scene

    sc = make_scene(64, 48, 40, seed=1, behind_fraction=1.0)     # every Gaussian behind the camera
    scene = _scene_from_arrays(tmp_path, sc)
    st = {}
    img = scene.render_image_hip(1, layout="hw3", semantics="std_3dgs", background=(0.2, 0.4, 0.6), stats=st)
    ref, nvis, inst, _ = _std_oracle(scene, sc, background=(0.2, 0.4, 0.6))
    assert nvis == 0 and st["n_instances"] == inst == 0 and st["n_visible"] == 0
    np.testing.assert_allclose(img.cpu().numpy(), ref, atol=1e-6)


def test_std3dgs_known_answer_single_gaussian(tmp_path):
    """Same hand-derived numbers as tests/test_std3dgs_oracle.py::test_known_answers_single_gaussian."""
    _need_gpu()
    w = h = 32
    sc = dict(points=np.array([[0.0, 0.0, 4.0]], np.float32), colors_0_255=np.array([[256.0, 128.0, 64.0]], np.float32),
              scales=np.full((1, 3), 0.5, np.float32), quaternions=np.array([[1.0, 0, 0, 0]], np.float32),
              opacity=np.array([[0.0]], np.float32), qvec=np.array([1.0, 0, 0, 0]), tvec=np.zeros(3),
              fx=np.float64(16.0), fy=np.float64(16.0), cx=np.float64(16.0), cy=np.float64(16.0),
              width=np.int64(w), height=np.int64(h))
    scene = _scene_from_arrays(tmp_path, sc)
    bg = (0.0, 0.0, 1.0)
    st = {}
    img = scene.render_image_hip(1, layout="hw3", semantics="std_3dgs", background=bg, stats=st,
                                 published_rects=True).cpu().numpy()
    assert st["n_visible"] == 1 and st["n_instances"] == 4
    alpha = 0.5 * np.exp(-0.5 * (0.25 + 0.25) / 4.3)
    np.testing.assert_allclose(img[15, 15], np.array([1.0, 0.5, 0.25]) * alpha + (1 - alpha) * np.array(bg), atol=2e-6)
    np.testing.assert_array_equal(img[0, 0], np.array(bg, np.float32))


def test_std3dgs_rejected_on_the_stage2_entry():
    _need_gpu()
    from intro_to_gaussian_splatting_amd import _ffi, render_preprocessed

    z = lambda *s: torch.zeros(s, device="cuda:0")  # noqa: E731
    with pytest.raises(_ffi.GsxError, match="gsx_render_forward"):
        render_preprocessed(32, 32, 16, z(4, 2), z(4, 3), z(4, 2, 2), z(4), z(4), z(4), z(4), z(4, 1),
                            semantics="std_3dgs")


@pytest.mark.parametrize("semantics", ["std_3dgs", "ref_cpu"])
def test_tile16_kernels_equal_the_generic_kernels_bit_for_bit(tmp_path, semantics):
    """tile == 16 runs the 4-pixels-per-lane kernels; GSX_FLAG_GENERIC_KERNELS forces the
    one-pixel-per-lane family: same arithmetic per pixel, so the frames must be identical."""
    _need_gpu()
    from intro_to_gaussian_splatting_amd.synthetic import make_scene

    w, h = 300, 200                                       # std_3dgs: partial edge tiles on both axes
    sc = make_scene(20000, w, h, seed=9, behind_fraction=0.1)
    scene = _scene_from_arrays(tmp_path, sc)
    kw = dict(semantics=semantics, background=(0.3, 0.2, 0.1)) if semantics == "std_3dgs" else dict(semantics=semantics)
    for layout in ("wh3", "hw3"):
        fast = scene.render_image_hip(1, layout=layout, **kw)
        slow = scene.render_image_hip(1, layout=layout, generic_kernels=True, **kw)
        assert torch.equal(fast, slow), (semantics, layout)


@pytest.mark.parametrize("seed", range(8))
def test_std3dgs_randomized_sweep(tmp_path, seed):
    """Random frame sizes, tile sizes, populations, cull shares, poses and backgrounds."""
    _need_gpu()
    from intro_to_gaussian_splatting_amd.synthetic import make_scene

    rs = np.random.RandomState(1000 + seed)
    w, h = int(rs.randint(17, 260)), int(rs.randint(17, 200))
    tile = int(rs.choice([4, 8, 16, 16, 16, 32]))
    n = int(rs.randint(1, 6000))
    q = rs.normal(size=4)
    sc = make_scene(n, w, h, seed=seed, behind_fraction=float(rs.choice([0.0, 0.3])),
                    qvec=tuple(q / np.linalg.norm(q)), tvec=tuple(rs.normal(size=3)))
    scene = _scene_from_arrays(tmp_path, sc)
    bg = tuple(float(v) for v in rs.uniform(0, 1, 3))
    ref, nvis, inst, rows = _std_oracle(scene, sc, tile=tile, background=bg)
    st = {}
    img = scene.render_image_hip(1, tile_size=tile, layout="hw3", semantics="std_3dgs", background=bg, stats=st,
                                 published_rects=True)
    assert st["n_visible"] == nvis and st["n_instances"] == inst, (w, h, tile, n)
    _check(img.cpu().numpy(), ref, (w, h, tile, n))
    _explained(img.cpu().numpy(), ref, rows, scene.gaussians.colors.cpu().numpy(), tile, bg, (w, h, tile, n))
    st2 = {}
    img2 = scene.render_image_hip(1, tile_size=tile, layout="hw3", semantics="std_3dgs", background=bg, stats=st2)
    assert torch.equal(img2, img) and st2["n_instances"] <= inst, (w, h, tile, n)
