"""Randomised parity fuzz on the GPU box: random frame sizes, tile sizes, populations, footprints,
off-axis spread, cull shares, poses, layouts and tile windows; HIP path vs the C restatements.
    python tools/fuzz.py [first_seed] [count] [big] [plain] [extreme] [guard] [family=trained|needle|tie|few|mixed]
ref_cpu: D and N_vis equal, max |dpixel| <= 1e-4.  std_3dgs: counts equal with the published
rectangles, frames of both binnings bit-identical, pixels within 1e-4 up to 1/255-threshold flips."""
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from intro_to_gaussian_splatting_amd import GaussianScene, Gaussians, _ffi  # noqa: E402
if os.environ.get("GSX_FUZZ_TEST_LIB"):      # libgsx_test.so, so that its knobs (GSX_LONG_SPLIT, GSX_DEPTH_SORT, ...) select what is fuzzed
    _ffi.use_test_library()
from intro_to_gaussian_splatting_amd.synthetic import make_scene, write_colmap_text  # noqa: E402
from oracle import c_oracle, cpu_ref  # noqa: E402
from tools.fuzz_scene import fuzz_scene  # noqa: E402

first = int(sys.argv[1]) if len(sys.argv) > 1 else 0
count = int(sys.argv[2]) if len(sys.argv) > 2 else 100
big = "big" in sys.argv[3:]     # larger frames (up to > 65 536 tiles) and populations
family = ([a.split("=", 1)[1] for a in sys.argv[3:] if a.startswith("family=")] or [""])[0]     # trained / needle / tie / few / mixed
extreme = "extreme" in sys.argv[3:]     # needles to 3000:1, pancakes, specks, saturated opacities, coincident centres
guard = "guard" in sys.argv[3:]         # every seed once more inside buffers with guarded margins, at the exact pair capacity and one below
GUARD_MARGIN = 1 << 16


def guarded_frames(scene, n, w, h, tile, layout, window, d, want, tag, nvis):
    """Workspace (exactly gsx_workspace_bytes for d pairs, then for d - 1: GSX_ERR_WORKSPACE_TOO_SMALL), hints buffer and frame as
    the middle of allocations whose margins hold a pattern: no kernel writes outside what it is given (there is no GPU
    address sanitizer on this pool; tests/test_hip_parity.py: test_kernels_stay_inside_the_buffers_they_are_given)."""
    lib = _ffi.load()

    def guarded(nbytes, fill=0):
        big = torch.full((GUARD_MARGIN + nbytes + GUARD_MARGIN,), 0xA5, dtype=torch.uint8, device="cuda:0")
        big[GUARD_MARGIN:GUARD_MARGIN + nbytes] = fill
        return big, big[GUARD_MARGIN:GUARD_MARGIN + nbytes]

    def intact(big, nbytes):
        return bool((big[:GUARD_MARGIN] == 0xA5).all().item()) and bool((big[GUARD_MARGIN + nbytes:] == 0xA5).all().item())

    hbytes = lib.gsx_hints_bytes(w, h, tile)
    # (a private call is not issued again when at most three Gaussians turn out visible: it is told, like a captured frame)
    rows = max(_ffi.visible_rows_flag(n, nvis, 0), 0)
    # (the library derives its capacity from the bytes it is given: the largest whose carve fits -- a little more than asked for)
    for cap in ([d, max(d // 2, 1)] if d > 1 else [max(d, 1)]):
        nbytes = lib.gsx_workspace_bytes(n, w, h, tile, cap)
        ws_big, ws = guarded(nbytes, 0x5A)
        hints_big, hints = guarded(hbytes)
        out_big, out_bytes = guarded(want.numel() * 4)
        out = out_bytes.view(torch.float32).view(want.shape)
        for rep in range(2):
            try:
                got = scene.render_image_hip(1, tile_size=tile, layout=layout, tile_window=window, out=out,
                                             _private=dict(cap=cap, workspace=ws, hints=[hints, rep > 0], rows_flag=rows))
                torch.cuda.synchronize()
                assert torch.equal(got, want), ("guarded frame", tag, cap, d, rep)       # (no error: the carve held all d pairs)
            except _ffi.GsxError as exc:
                torch.cuda.synchronize()
                assert cap < d and exc.code == _ffi.GSX_ERR_WORKSPACE_TOO_SMALL, ("guarded frame", tag, cap, d, str(exc))
            assert intact(ws_big, nbytes) and intact(hints_big, hbytes) and intact(out_big, want.numel() * 4), ("margins overwritten", tag, cap, rep)
if "plain" in sys.argv[3:]:     # the second frame of every view takes GSX_FLAG_PLAIN_FOOTPRINTS where the first found it safe
    from intro_to_gaussian_splatting_amd import gaussian_scene as _wrapper
    _wrapper._PLAIN_MIN_TILES = 1
worst_ref, worst_std, flips_total = 0.0, 0.0, 0
for seed in range(first, first + count):
    rs, sc, w, h, tile, n, needles = fuzz_scene(seed, big, extreme, family)
    if n == 0:
        sc = {k: (v[:0] if isinstance(v, np.ndarray) and v.ndim == 2 else v) for k, v in sc.items()}
    with tempfile.TemporaryDirectory() as tmp:
        write_colmap_text(tmp, sc)
        g = Gaussians.from_arrays(sc["points"], sc["colors_0_255"], sc["scales"], sc["quaternions"], sc["opacity"],
                                  device="cuda:0")
        scene = GaussianScene(tmp, g)
        ordered = GaussianScene(tmp, g.spatially_ordered())     # the same Gaussians, rows along a Morton curve (GsxParams.original_index)
    im = scene.images[1]
    c = im.gsx_camera()
    cam = cpu_ref.Camera(im.world2view.cpu().numpy(), im.full_proj_transform.cpu().numpy(), np.float32(c.tan_fovx),
                         np.float32(c.tan_fovy), np.float32(c.fx), np.float32(c.fy), c.width, c.height)
    colors = g.colors.cpu().numpy()
    layout = str(rs.choice(["wh3", "hw3"]))
    tag = (seed, w, h, tile, n, layout)
    # ---- reference CPU rules
    pre = c_oracle.preprocess(sc["points"], colors, sc["scales"], sc["quaternions"], sc["opacity"], cam)
    _, _, inst = c_oracle.render(pre, w, h, tile, window=(0, 0, 0, 0))     # (the count alone)
    if inst > 300_000_000:
        continue        # (needles on a big frame: more pairs than a 2^31-pair workspace is for; not what is fuzzed here)
    ref, _, inst = c_oracle.render(pre, w, h, tile)
    st = {}
    img = scene.render_image_hip(1, tile_size=tile, layout=layout, stats=st).cpu().numpy()
    if layout == "hw3":
        img = img.transpose(1, 0, 2)
    assert st["n_instances"] == inst and st["n_visible"] == len(pre.depths), ("ref counts", tag, st, inst)
    d = float(np.abs(img - ref).max()) if img.size else 0.0
    assert d <= 1e-4, ("ref pixels", tag, d)
    worst_ref = max(worst_ref, d)
    # the next frame of the view finds this one's hints (splitters, costs, schedule): same pixels
    again = scene.render_image_hip(1, tile_size=tile, layout=layout).cpu().numpy()
    assert np.array_equal(again.transpose(1, 0, 2) if layout == "hw3" else again, img), ("hinted frame differs", tag)
    if guard and img.size:
        guarded_frames(scene, n, w, h, tile, layout, None, inst, scene.render_image_hip(1, tile_size=tile, layout=layout).clone(), tag, len(pre.depths))
    # ---- spatially ordered rows, everything filed under the original index: the same frame bit for bit, equal depths included
    so = {}
    oimg = ordered.render_image_hip(1, tile_size=tile, layout=layout, stats=so).cpu().numpy()
    assert np.array_equal(oimg.transpose(1, 0, 2) if layout == "hw3" else oimg, img), ("spatially ordered frame differs", tag)
    assert so["n_instances"] == inst and so["n_visible"] == len(pre.depths), ("spatially ordered counts", tag, so)
    # ---- the compositing in parts along the leading axis (GsxParams.n_substrips: what a rank sends while it composites the next)
    if tile == 16 and min(w, h) >= 32:
        from intro_to_gaussian_splatting_amd import strips as _strips
        n_lead = _strips.tiles_along(w if layout == "wh3" else h, tile)
        parts = int(rs.randint(2, min(16, n_lead) + 1)) if n_lead >= 2 else 0
        if parts:
            evs = []
            got = scene.render_image_hip(1, tile_size=tile, layout=layout, substrips=_strips.substrip_bounds(0, n_lead, parts),
                                         substrip_events=evs).cpu().numpy()
            torch.cuda.synchronize()
            assert np.array_equal(got.transpose(1, 0, 2) if layout == "hw3" else got, img), ("substrips differ", tag, parts)
    # ---- a random tile window of the same frame (multi-GPU strips use these)
    from intro_to_gaussian_splatting_amd import strips
    ntx, nty = strips.tiles_along(w, tile), strips.tiles_along(h, tile)
    if ntx > 0 and nty > 0:
        x0, y0 = int(rs.randint(0, ntx)), int(rs.randint(0, nty))
        win = (x0, int(rs.randint(x0, ntx)) + 1, y0, int(rs.randint(y0, nty)) + 1)
        wref, _, winst = c_oracle.render(pre, w, h, tile, window=win)
        st = {}
        wimg = scene.render_image_hip(1, tile_size=tile, layout="wh3", tile_window=win, stats=st).cpu().numpy()
        inside = np.zeros((w, h), bool)
        inside[win[0] * tile:win[1] * tile, win[2] * tile:win[3] * tile] = True
        assert not wimg[~inside].any(), ("window outside", tag, win)
        assert float(np.abs(wimg - wref).max()) <= 1e-4, ("window pixels", tag, win)
        # the oracle counts instances over all tiles; inside the window the GPU count is the sum of its lists
        assert st["n_instances"] <= inst, ("window count", tag, win)
        if guard and wimg.size and st["n_instances"] > 0:
            guarded_frames(scene, n, w, h, tile, "wh3", win, int(st["n_instances"]),
                           scene.render_image_hip(1, tile_size=tile, layout="wh3", tile_window=win).clone(), tag, len(pre.depths))
        so = {}
        owimg = ordered.render_image_hip(1, tile_size=tile, layout="wh3", tile_window=win, stats=so).cpu().numpy()
        assert np.array_equal(owimg, wimg) and so["n_instances"] == st["n_instances"], ("spatially ordered window differs", tag, win)
    if needles:
        # the other rule sets are restatements nothing pins (their source kernels cannot run here); on ill-conditioned
        # footprints kernel and restatement are two float32 evaluations of the same formula, a few 1e-4 apart
        continue
    # ---- the reference's CUDA-kernel rules (every pixel tests every Gaussian on the CPU side: keep it small)
    if w * h * max(n, 1) <= 3e8:
        cref = c_oracle.render_cuda_semantics(pre, w, h)
        cimg = scene.render_image_hip(1, tile_size=tile, layout="hw3", semantics="ref_cuda").cpu().numpy()
        dc = np.abs(cimg.astype(np.float64) - cref).max(axis=-1) if cimg.size else np.zeros(1)
        # stop rule at T(1-alpha) < 1e-3: a pixel whose test sits within an ulp of the threshold may stop one
        # Gaussian earlier or later on one side, which moves it by T alpha colour = 1e-3 alpha / (1 - alpha) colour -- up to
        # 0.099 at the rule's own alpha <= 0.99 (seed 204401 of round 6's campaign: test = 0.00100000075, alpha 0.84, 3.9e-3;
        # tools/attic/refcuda_flip.py walks such a pixel); everything else agrees to 1e-4
        assert int((dc > 1e-4).sum()) <= 2 + 1e-5 * dc.size and dc.max() < 0.1, ("ref_cuda pixels", tag, float(dc.max()))
    # ---- the stage-2 entry point on stage-1 arrays that no projection would produce: NaN / infinite /
    #      inverted bounding boxes, asymmetric inverse covariances (render.cu:90-101 takes them as given)
    if len(pre.depths) > 0:
        import copy
        from intro_to_gaussian_splatting_amd import render_preprocessed
        m = len(pre.depths)
        bad = {k: np.array(getattr(pre, k), copy=True) for k in ("min_x", "max_x", "min_y", "max_y", "inverse_covariance_2d")}
        pick = lambda frac: rs.uniform(size=m) < frac  # noqa: E731
        bad["min_x"][pick(0.05)] = np.nan
        bad["max_y"][pick(0.05)] = np.nan
        bad["max_x"][pick(0.05)] = np.inf
        bad["min_y"][pick(0.05)] = -np.inf
        sw = pick(0.05)
        bad["min_x"][sw], bad["max_x"][sw] = bad["max_x"][sw].copy(), bad["min_x"][sw].copy()
        bad["min_x"][pick(0.03)] = 3.0e9
        bad["max_x"][pick(0.03)] = -3.0e9
        # asymmetric off-diagonals with (nearly) the same sum: the quadratic form stays positive definite.  (An
        # indefinite form can push alpha towards 1, where the reference's "return before accumulating" drops a
        # contribution of size T alpha c and rounding decides which side of the 1e-6 test a pixel falls on.)
        eps = rs.uniform(-0.1, 0.1, m).astype(np.float32)
        bad["inverse_covariance_2d"][:, 0, 1] *= (1 + eps)
        bad["inverse_covariance_2d"][:, 1, 0] *= (1 - eps)
        pre_bad = pre._replace(**bad)
        bref, _, binst = c_oracle.render(pre_bad, w, h, tile)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
        st = {}
        bimg = render_preprocessed(h, w, tile, t(pre_bad.points), t(pre_bad.colors), t(pre_bad.inverse_covariance_2d),
                                   t(pre_bad.min_x), t(pre_bad.max_x), t(pre_bad.min_y), t(pre_bad.max_y),
                                   t(pre_bad.sigmoid_opacity), stats=st).cpu().numpy()
        assert st["n_instances"] == binst, ("stage-2 counts", tag, st, binst)
        db = np.abs(bimg - bref)
        if not db.max() <= 1e-4:
            ix = np.unravel_index(np.nanargmax(db), db.shape)
            print("stage-2 mismatch", tag, "max", db.max(), "at", ix, "gpu", bimg[ix[0], ix[1]], "cpu", bref[ix[0], ix[1]],
                  "pixels off", int((db.max(axis=-1) > 1e-4).sum()), "nan gpu/cpu", int(np.isnan(bimg).sum()), int(np.isnan(bref).sum()))
        assert float(db.max()) <= 1e-4, ("stage-2 pixels", tag)
    # ---- published 3DGS rules
    bg = tuple(float(v) for v in rs.uniform(0, 1, 3))
    sref, nvis, sinst, _ = c_oracle.render_std3dgs(sc["points"], colors, sc["scales"], sc["quaternions"], sc["opacity"],
                                                   cam, tile=tile, background=bg)
    st = {}
    a = scene.render_image_hip(1, tile_size=tile, layout="hw3", semantics="std_3dgs", background=bg, stats=st,
                               published_rects=True)
    assert st["n_instances"] == sinst and st["n_visible"] == nvis, ("std counts", tag, st, sinst, nvis)
    st2 = {}
    b = scene.render_image_hip(1, tile_size=tile, layout="hw3", semantics="std_3dgs", background=bg, stats=st2)
    assert torch.equal(a, b) and st2["n_instances"] <= sinst, ("std tight", tag)
    dd = np.abs(a.cpu().numpy().astype(np.float64) - sref).max(axis=-1) if a.numel() else np.zeros(1)
    flips = int((dd > 1e-4).sum())
    assert flips <= 2 + 1e-5 * dd.size and dd.max() < 0.006, ("std pixels", tag, flips, float(dd.max()))
    flips_total += flips
    worst_std = max(worst_std, float(dd[dd <= 1e-4].max()) if (dd <= 1e-4).any() else 0.0)
print("fuzz seeds %d..%d ok: ref_cpu worst |dpixel| %.2e; std_3dgs worst %.2e (+ %d threshold flips in total)" % (
    first, first + count - 1, worst_ref, worst_std, flips_total))
