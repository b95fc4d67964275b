"""gsx_render_contribution, gsx_density_plan_contribution and the Python surface on top of them, on the GPU.

weight_sum is pinned bit for bit to grad_colors[:, 0] of the existing backward entry (gsx_render_backward /
gsx_render_backward_std) under dL/dframe = 1 -- an entry that is itself held to the reference -- on every case of
tests/test_contribution_host.py::CASES; weight_max and pixels are held to the float64 restatement
(tests/contribution_restatement.py), weight_max to the project's pixel tolerance 1e-4 (a blend weight is one term of the
coverage A, which tests/test_hip_depth.py holds to 1e-4), pixels exactly, on the Gaussians the restatement does not leave out
(none on these scenes: tests/test_contribution_host.py).

Measured on an MI355X (every case of CASES; weight_sum equal to the backward entry's bits on all of them, tight and published
rectangles; pixels equal on every row; no row left out):
  worst |weight_max - restatement|   1.46e-07  (dense_48x48_n1500 ref_cpu tile 16; big_96x80_n301 std_3dgs tile 8)   bound 1e-4
  per scene, ref_cpu / std_3dgs:     tiny 5.91e-08 / 1.19e-07, cull 1.17e-07 / 1.17e-07, tile12_dense 1.19e-07 / 9.41e-08,
                                     the same to the printed digit at tiles 8, 16 and 32 except cull ref_cpu tile 8 (9.25e-08)
  weight_sum against the restatement (not the pin; relative to the largest sum): at most 2.28e-07 (cull std_3dgs tile 16)
  Trainer, tiny_48x48_n600, prune after step 3 at threshold 0.05; H = per pixel, the blend weights the pruned rows held:
    ref_cpu   600 -> 255 rows (265 no view listed, 80 below the threshold); largest pixel change 0.0459 where H = 0.0474;
              H at most 0.0488 and zero on 1641 of 2304 pixels; largest change above the pixel's own bound H (hi - lo): 1.22e-08
              (slack 1e-5); threshold x pruned weight_sum 0.0615
    std_3dgs  600 -> 538 rows (1 no view listed, 61 below the threshold); largest pixel change 0.0266 where H = 0.0401;
              H at most 0.0547 and zero on 2074 of 2304 pixels; no pixel above its own bound; threshold x pruned weight_sum 0.182
"""
import ctypes

import numpy as np
import pytest
import torch

import contribution_restatement as cr
from test_contribution_host import CASES, restated, scene_dict
from test_hip_backward import DEV, _scene
from test_hip_density import Guarded, _apply, _same

pytestmark = pytest.mark.gpu

TOL = 1e-4
BG = (0.25, 0.5, 0.75)
I32_POISON = 0x5A5A5A5


def _bits(t):
    return t.contiguous().view(torch.int32)


def _np(t):
    return t.detach().cpu().numpy()


def _make(tmp_path, name, **kw):
    sc = scene_dict(name)
    return sc, _scene(tmp_path, sc, colors=sc["colors"], **kw)


def _forward(scene, semantics, tile, idx=1, published=False):
    st = {}
    kw = dict(semantics="std_3dgs", background=BG, published_rects=published) if semantics == "std_3dgs" else {}
    with torch.no_grad():
        frame = scene.render_image_hip(idx, tile_size=tile, stats=st, **kw)
    return frame, st


def _contribution(scene, semantics, tile, st, idx=1, out=None, published=False):
    return scene._render_contribution(idx, tile, semantics, st["n_instances"], st["n_visible"], out=out, published_rects=published)


def _colour_gradient(scene, semantics, tile, frame, st, published=False):
    """grad_colors[:, 0] of the colour-only backward entry under dL/dframe = 1."""
    outs = scene._render_backward(1, tile, "wh3", frame, torch.ones_like(frame), st["n_instances"], st["n_visible"],
                                  std=(BG, published) if semantics == "std_3dgs" else None)
    assert len(outs) == 2
    return outs[0][:, 0].contiguous()


def _poison_free_blocks(n):
    """Freed allocator blocks of the outputs' sizes that hold NaN / a pattern: torch.empty hands them out again."""
    junk = [torch.full((n,), float("nan"), device=DEV) for _ in range(4)] + \
           [torch.full((n,), I32_POISON, dtype=torch.int32, device=DEV) for _ in range(4)]
    junk[0].sum().item()
    del junk


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%s-t%d" % c)
def test_sum_is_the_backward_s_bits_and_max_and_pixels_match_the_restatement(tmp_path, case):
    name, semantics, tile = case
    sc, scene = _make(tmp_path, name)
    n = sc["points"].shape[0]
    frame, st = _forward(scene, semantics, tile)
    _poison_free_blocks(n)
    con = _contribution(scene, semantics, tile, st)
    for t, dtype in zip(con, (torch.float32, torch.float32, torch.int32, torch.int32)):
        assert t.shape == (n,) and t.dtype == dtype and t.device.type == "cuda"
    # 1. weight_sum: the existing backward entry's bits
    gc0 = _colour_gradient(scene, semantics, tile, frame, st)
    assert torch.equal(_bits(con.weight_sum), _bits(gc0)), (case, float((con.weight_sum - gc0).abs().max()))
    # the same call twice, and through the public method: the same bits
    for other in (_contribution(scene, semantics, tile, st), scene.render_contribution_hip(1, semantics=semantics, tile_size=tile)):
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(con, other))
    # 2. weight_max and pixels: the restatement
    ref = restated(name, semantics, tile)
    wmax, wsum, pixels, views = (_np(t) for t in con)
    assert np.isfinite(wmax).all() and np.isfinite(wsum).all()
    err, bad = cr.compare(wmax, pixels, ref)
    err_sum = float(np.abs(wsum - ref.weight_sum).max() / max(1.0, ref.weight_sum.max()))
    print("%s %s tile %d: |weight_max - restatement| %.3g (bound %.3g), weight_sum vs restatement %.3g of its largest, "
          "%d of %d listed rows left out, %d rows composited, largest weight_max %.3g, %d pairs"
          % (name, semantics, tile, err, TOL, err_sum, int(ref.excluded.sum()), int(ref.listed.sum()), int((pixels > 0).sum()),
             float(wmax.max()) if n else 0.0, st["n_instances"]))
    assert err <= TOL, (case, err)
    assert bad.size == 0, (case, bad[:10], pixels[bad[:10]], ref.pixels[bad[:10]])
    assert err_sum <= TOL
    # views: 0 or 1; whoever was composited was listed; an unlisted row reads +0 / 0
    assert set(np.unique(views)) <= {0, 1}
    assert (views[pixels > 0] == 1).all()
    dead = views == 0
    assert not _bits(con.weight_max)[torch.from_numpy(dead).to(DEV)].any() and not wsum[dead].any() and not pixels[dead].any()
    if semantics == "ref_cpu":
        assert np.array_equal(views == 1, ref.listed)
    # the invariants, in float32: max <= min(1, sum) and max >= sum / pixels to the rounding of a sum of `pixels` terms
    seen = pixels > 0
    assert (wmax <= np.minimum(1.0, wsum * (1 + 1e-6))).all()
    assert (wmax[seen].astype(np.float64) >= wsum[seen].astype(np.float64) / pixels[seen] * (1 - 1e-5)).all()
    if name.startswith("none"):
        assert not views.any() and st["n_instances"] == 0
    if name.startswith("big"):
        assert pixels[300] > 64 * 64            # more than 64 tiles of 64 pixels: the slot loop's second trip
    if semantics == "std_3dgs":
        # published rectangles: other lists and slots, the same composited pairs -- max and pixels exactly, the sum to rounding
        frame_p, st_p = _forward(scene, semantics, tile, published=True)
        con_p = _contribution(scene, semantics, tile, st_p, published=True)
        assert st_p["n_instances"] >= st["n_instances"]
        assert torch.equal(_bits(con_p.weight_max), _bits(con.weight_max)) and torch.equal(con_p.pixels, con.pixels)
        assert torch.equal(_bits(con_p.weight_sum), _bits(_colour_gradient(scene, semantics, tile, frame_p, st_p, published=True)))
        assert bool((con_p.views >= con.views).all())


# ---- accumulate
def _two_view_scene(tmp_path, name):
    from intro_to_gaussian_splatting_amd import GaussianScene, Gaussians
    from intro_to_gaussian_splatting_amd.synthetic import orbit_poses, write_colmap_text

    sc = scene_dict(name)
    pose = orbit_poses(3, step_deg=20.0, qvec=sc["qvec"], tvec=sc["tvec"])[2]
    write_colmap_text(str(tmp_path), sc, extra_poses=[pose])
    g = Gaussians.from_arrays(sc["points"], sc["colors_0_255"], sc["scales"], sc["quaternions"], sc["opacity"], device=DEV)
    g.colors = torch.from_numpy(np.ascontiguousarray(sc["colors"], np.float32)).to(DEV)
    scene = GaussianScene(str(tmp_path), g)
    assert sorted(scene.images) == [1, 2]
    return sc, scene


@pytest.mark.parametrize("semantics", ["ref_cpu", "std_3dgs"])
def test_two_views_merge_to_the_composition_of_the_single_views_in_either_order(tmp_path, semantics):
    sc, scene = _two_view_scene(tmp_path, "cull_96x80_n400")
    n = sc["points"].shape[0]
    a = scene.render_contribution_hip(1, semantics=semantics)
    b = scene.render_contribution_hip(2, semantics=semantics)
    assert not torch.equal(a.weight_max, b.weight_max) and int(a.views.sum()) > 50 and int(b.views.sum()) > 50
    only_a, only_b = (a.views == 1) & (b.views == 0), (a.views == 0) & (b.views == 1)
    assert bool(only_a.any()) or bool(only_b.any())          # the views do not list the same rows
    want = (torch.maximum(a.weight_max, b.weight_max), a.weight_sum + b.weight_sum, a.pixels + b.pixels, a.views + b.views)
    ab = scene.render_contribution_hip(2, semantics=semantics, out=scene.render_contribution_hip(1, semantics=semantics))
    ba = scene.render_contribution_hip(1, semantics=semantics, out=scene.render_contribution_hip(2, semantics=semantics))
    swept, swept_back = scene.contribution(semantics=semantics), scene.contribution([2, 1], semantics=semantics)
    for got in (ab, ba, swept, swept_back):
        for k, (x, y) in enumerate(zip(got, want)):
            assert torch.equal(_bits(x), _bits(y)), (semantics, k)
    assert int(swept.views.max()) == 2
    # rows neither view lists keep what was there with accumulate = 1 ...
    neither = (a.views == 0) & (b.views == 0)
    assert int(neither.sum()) >= 100                        # the culled rows
    from intro_to_gaussian_splatting_amd import Contribution

    prior = Contribution(torch.full((n,), 0.75, device=DEV), torch.full((n,), -3.25, device=DEV),
                         torch.full((n,), 11, dtype=torch.int32, device=DEV), torch.full((n,), 5, dtype=torch.int32, device=DEV))
    got = scene.render_contribution_hip(2, semantics=semantics, out=scene.render_contribution_hip(1, semantics=semantics, out=prior))
    assert got is prior
    assert bool((got.weight_max[neither] == 0.75).all()) and bool((got.weight_sum[neither] == -3.25).all())
    assert bool((got.pixels[neither] == 11).all()) and bool((got.views[neither] == 5).all())
    both = ~neither
    assert torch.equal(got.views[both], want[3][both] + 5) and torch.equal(got.pixels[both], want[2][both] + 11)
    assert torch.equal(got.weight_max[both], torch.clamp(want[0][both], min=0.75))
    # ... and a Contribution of another length is refused
    with pytest.raises(ValueError, match="weight_max"):
        scene.render_contribution_hip(1, out=Contribution(*(t[:-1].contiguous() for t in prior)))
    with pytest.raises(ValueError, match="ref_cuda"):
        scene.render_contribution_hip(1, semantics="ref_cuda")
    with pytest.raises(ValueError, match="tile_window"):
        scene.render_contribution_hip(1, tile_window=(0, 1, 0, 1))


# ---- the C ABI between guarded margins, at the exact workspace size
@pytest.mark.parametrize("semantics", ["ref_cpu", "std_3dgs"])
def test_outputs_and_workspace_stay_inside_their_buffers(tmp_path, semantics):
    from intro_to_gaussian_splatting_amd import _ffi
    from intro_to_gaussian_splatting_amd._device import _ptr, _stream_handle

    name, tile = "cull_96x80_n400", 8
    sc, scene = _make(tmp_path, name)
    n = sc["points"].shape[0]
    frame, st = _forward(scene, semantics, tile)
    want = _contribution(scene, semantics, tile, st)
    lib = _ffi.load()
    dev, _, tensors = scene._inputs(1)
    cam = scene.images[1].gsx_camera()
    params, _ = scene._frame_params(dev, n, "wh3", semantics)
    if semantics == "ref_cpu":
        params.flags |= _ffi.rows_flag(n, st["n_visible"])
    need = lib.gsx_contribution_workspace_bytes(n, cam.width, cam.height, tile, st["n_instances"])       # not one pair to spare
    assert need > 0
    whole = torch.full((need + 1024,), 0xA5, dtype=torch.uint8, device=DEV)
    lead = 256 + (-(whole.data_ptr() + 256)) % 256
    ws = whole[lead:lead + need]
    assert ws.data_ptr() % 256 == 0

    def call(outs, accumulate, views=True, nbytes=need):
        with torch.cuda.device(dev):
            rc = lib.gsx_render_contribution(ctypes.byref(cam), *[_ptr(t.detach()) for t in tensors], n, tile,
                                             *[ctypes.c_void_p(o.view.data_ptr()) for o in outs[:3]],
                                             ctypes.c_void_p(outs[3].view.data_ptr()) if views else None, accumulate,
                                             ctypes.byref(params), _ptr(ws), nbytes, _stream_handle(dev))
        torch.cuda.synchronize()
        return rc

    def fresh():
        return [Guarded(n), Guarded(n), Guarded(n, 0, torch.int32), Guarded(n, 0, torch.int32)]

    outs = fresh()
    assert call(outs, 0) == 0, lib.gsx_last_error()
    for o, ref in zip(outs, want):
        assert o.intact() and torch.equal(_bits(o.view), _bits(ref))
        assert not bool((o.view == o.fill).any())              # accumulate = 0 writes every row, the unlisted ones too
    assert bool((whole[:lead] == 0xA5).all()) and bool((whole[lead + need:] == 0xA5).all())
    # accumulate = 1 into prior values: a listed row is merged (max, +=, +=, views += 1), an unlisted row is not touched
    outs1 = fresh()
    priors = (-1.0, 1.0, 7, 3)
    for o, v in zip(outs1, priors):
        o.view.fill_(v)
    assert call(outs1, 1) == 0, lib.gsx_last_error()
    unlisted = want.views == 0
    assert int(unlisted.sum()) >= 100
    for o, v in zip(outs1, priors):
        assert o.intact() and bool((o.view[unlisted] == v).all())
    listed = ~unlisted
    assert torch.equal(_bits(outs1[0].view[listed]), _bits(want.weight_max[listed]))
    assert torch.equal(_bits(outs1[1].view[listed]), _bits(1.0 + want.weight_sum[listed]))
    assert torch.equal(outs1[2].view[listed], want.pixels[listed] + 7) and bool((outs1[3].view[listed] == 4).all())
    # views may be NULL
    outs2 = fresh()
    assert call(outs2, 0, views=False) == 0, lib.gsx_last_error()
    assert bool((outs2[3].whole == outs2[3].fill).all())
    assert all(torch.equal(_bits(o.view), _bits(ref)) for o, ref in zip(outs2[:3], want))
    # one pair short: refused with the counts' message, nothing outside the buffers touched
    short = lib.gsx_contribution_workspace_bytes(n, cam.width, cam.height, tile, max(st["n_instances"] // 2, 1))
    assert call(fresh(), 0, nbytes=short) == _ffi.GSX_ERR_WORKSPACE_TOO_SMALL
    assert bool((whole[:lead] == 0xA5).all()) and bool((whole[lead + need:] == 0xA5).all())


# ---- gsx_density_plan_contribution + gsx_density_apply
@pytest.mark.parametrize("n", [1, 257, 1024, 5000])
@pytest.mark.parametrize("with_views", [True, False])
def test_plan_and_apply_equal_a_mask_composed_in_torch(n, with_views):
    from intro_to_gaussian_splatting_amd import _ffi

    lib = _ffi.load()
    rs = np.random.RandomState(n + int(with_views))
    thr = np.float32(0.01)
    w = (rs.uniform(0.0, 0.03, n)).astype(np.float32)
    w[rs.uniform(size=n) < 0.1] = thr                           # exactly equal: kept
    w[rs.uniform(size=n) < 0.05] = np.nextafter(thr, np.float32(0))     # one ulp below: pruned
    w[rs.uniform(size=n) < 0.05] = np.nan                       # fails the comparison: kept
    w[rs.uniform(size=n) < 0.05] = 0.0
    views = rs.randint(0, 3, n).astype(np.int32)
    views[rs.uniform(size=n) < 0.2] = 0
    keep = ~(w < thr)
    if with_views:
        keep &= views != 0
    need = lib.gsx_density_workspace_bytes(n)
    ws = torch.full((need + 256,), 0xA5, dtype=torch.uint8, device=DEV)
    ws = ws[(-ws.data_ptr()) % 256:][:need]
    wd, vd = torch.from_numpy(w).to(DEV), torch.from_numpy(views).to(DEV)
    counts = (ctypes.c_int64 * 4)(-1, -1, -1, -1)
    rc = lib.gsx_density_plan_contribution(wd.data_ptr(), vd.data_ptr() if with_views else None, float(thr), n, ws.data_ptr(), need,
                                           counts, ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    assert rc == 0, lib.gsx_last_error()
    n_out = int(keep.sum())
    assert tuple(counts) == (n_out, n - n_out, 0, 0)
    if n >= 257:
        assert 0 < n_out < n and np.isnan(w[keep]).any() and (w[keep] == thr).any() and (w[~keep] == 0).any()
    spec = [(3, 0), (1, 0), (48, 0), (3, 1), (4, 1), (3, 2), (3, 3), (4, 4)]      # COPY, ZERO_NEW (moments), POINTS, SCALES, QUATS
    sources = [rs.normal(size=(n, width)).astype(np.float32) for width, _ in spec]
    sources[0][rs.uniform(size=(n, 3)) < 0.05] = -0.0
    noise = rs.normal(size=(n, 2, 3)).astype(np.float32)
    for lead in (0, 1):
        rc, dsts, rows = _apply(ws, n, n_out, spec, sources, noise, lead)
        assert rc == 0, lib.gsx_last_error()
        assert np.array_equal(rows.view.cpu().numpy(), np.nonzero(keep)[0].astype(np.int32)) and rows.intact()
        for (width, role), d, src in zip(spec, dsts, sources):
            assert _same(d.view.cpu().numpy().reshape(n_out, width), src[keep]), (n, width, role)       # survivors, in order, same bits
            assert d.intact()


# ---- the Python surface: DensityControl.prune_contribution and the Trainer's event
def _trainer(tmp_path, sub, semantics, **kw):
    from intro_to_gaussian_splatting_amd import Trainer

    (tmp_path / sub).mkdir()
    sc, scene = _make(tmp_path / sub, "tiny_48x48_n600")
    target = torch.rand((48, 48, 3), generator=torch.Generator(device="cpu").manual_seed(3)).to(DEV)
    extra = dict(semantics="std_3dgs", background=BG) if semantics == "std_3dgs" else {}
    return Trainer(scene, {1: target}, tile_size=16, densify_every=None, opacity_reset_every=None, sh_degree_every=None,
                   seed=1, **extra, **kw)


def _held_weight(scene, rows, semantics):
    """(W, H): per pixel the summed blend weight T alpha of the Gaussians `rows` (a bool mask) in view 1 -- the frame over
    colours (1, 0, 0) for those rows and 0 for the others, over a black background."""
    g = scene.gaussians
    stored = g.colors
    g.colors = torch.stack([rows.to(torch.float32), torch.zeros_like(stored[:, 0]), torch.zeros_like(stored[:, 0])], 1).contiguous()
    try:
        with torch.no_grad():
            kw = dict(semantics="std_3dgs", background=(0.0, 0.0, 0.0)) if semantics == "std_3dgs" else {}
            out = scene.render_image_hip(1, tile_size=16, **kw).clone()
    finally:
        g.colors = stored
    assert not out[..., 1:].any()
    return out[..., 0]


def _state(tr):
    g, opt = tr.gaussians, tr.opt
    out = {name: getattr(g, name).detach().clone() for name in ("points", "scales", "quaternions", "opacity", "colors")}
    for name in opt.names:
        out["m_" + name], out["v_" + name] = opt.exp_avg[name].clone(), opt.exp_avg_sq[name].clone()
    return out


@pytest.mark.parametrize("semantics", ["ref_cpu", "std_3dgs"])
def test_trainer_event_is_the_calls_written_out_by_hand(tmp_path, semantics):
    threshold = 0.05
    auto = _trainer(tmp_path, "auto", semantics, prune_contribution_at=(3,), prune_contribution=dict(threshold=threshold))
    hand = _trainer(tmp_path, "hand", semantics)
    assert auto.events_at(3) == ("prune_contribution",) and hand.events_at(3) == ()
    auto.fit(3)
    hand.fit(3)
    kw = dict(semantics="std_3dgs", background=BG) if semantics == "std_3dgs" else {}
    with torch.no_grad():
        before = hand.scene.render_image_hip(1, tile_size=16, **kw).clone()
    colours_before = hand.gaussians.colors.detach().clone()
    con = hand.scene.contribution(None, semantics=semantics, tile_size=16)
    n = len(hand.gaussians)
    with pytest.raises(ValueError, match="rows"):
        hand.density.prune_contribution(type(con)(*(t[:-1].contiguous() for t in con)))
    with pytest.raises(ValueError, match="threshold"):
        hand.density.prune_contribution(con, threshold=float("nan"))
    keep = ~(con.weight_max < threshold) & (con.views != 0)
    pruned = ~keep
    held = _held_weight(hand.scene, pruned, semantics)      # (W, H): per pixel, the blend weights of the rows about to go
    counts = hand.density.prune_contribution(con, threshold=threshold)
    assert counts == dict(n_out=int(keep.sum()), n_pruned=int(pruned.sum()), n_cloned=0, n_split=0)
    assert 0 < counts["n_out"] < n and len(hand.gaussians) == counts["n_out"] == len(auto.gaussians)       # the container shrinks
    assert int((pruned & (con.views != 0)).sum()) > 0 and int((con.views == 0).sum()) > 0                 # by weight, and unseen
    a, h = _state(auto), _state(hand)
    for key in h:
        assert torch.equal(_bits(a[key]), _bits(h[key])), key
    assert hand.density.grad_sum.shape[0] == counts["n_out"] and not hand.density.grad_sum.any() and not hand.density.seen.any()
    # the next frame: no pixel moves by more than the sum of the pruned weights it held.  Per pixel, with H that sum: taking
    # the pruned records out of the walk raises every other record's weight and the background's share, none of them falls,
    # and the weights of a pixel add up to one with the background's -- so the rises add up to H as well.  The pixel loses
    # sum_pruned w c and gains sum_rest dw c (+ dT_fin bg): each channel moves by at most H (hi - lo), lo and hi the smallest
    # and largest of the colours, the background and 0 (ref_cpu's background).  SLACK: float32 rounding of two frames of at
    # most a few hundred terms each, and ref_cpu's stop rule, which may let a pixel go on below T = 1e-6.
    with torch.no_grad():
        after = hand.scene.render_image_hip(1, tile_size=16, **kw)
    delta = (after - before).abs().amax(dim=2)
    bg = BG if semantics == "std_3dgs" else (0.0, 0.0, 0.0)
    lo, hi = min(0.0, float(colours_before.min()), min(bg)), max(0.0, float(colours_before.max()), max(bg))
    moved, slack = float(delta.max()), 1e-5
    excess = float((delta - held * (hi - lo)).max())
    literal = threshold * float(con.weight_sum[pruned].double().sum())
    print("%s: %d -> %d rows (%d unseen, %d below %.2g); largest pixel change %.3g where the pruned rows held %.3g; held weight "
          "at most %.3g, zero on %d of %d pixels; largest change minus the pixel's own bound %.3g (colour range %.3g); "
          "threshold x pruned weight_sum %.3g"
          % (semantics, n, counts["n_out"], int((con.views == 0).sum()), int((pruned & (con.views != 0)).sum()), threshold, moved,
             float(held.flatten()[delta.argmax()]), float(held.max()), int((held == 0).sum()), held.numel(), excess, hi - lo,
             literal))
    assert excess <= slack, (semantics, excess)
    assert 0 < float(held.max()) < 0.5 and int((held == 0).sum()) > 0       # a bound well under one, and pixels that may not move
    assert moved > 10 * slack                                                 # ... and the prune is seen
    assert moved <= literal, (semantics, moved, literal)                      # the one figure over the whole frame
    # and on: one more step each, the same bits
    auto.fit(1)
    hand.fit(1)
    a, h = _state(auto), _state(hand)
    for key in h:
        assert torch.equal(_bits(a[key]), _bits(h[key])), key
