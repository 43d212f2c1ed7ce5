"""Transmission records (rt_set_transmission) on an MI355X: the glass kernels for frames and ray
batches against tests/glass_fixture.py (lights_fixture's trace with the passage step), with and
without lights and RT_FLAG_SHADOWS, and their composition with everything a frame can be
combined with.

Inputs: the hand-built scene G (two glass spheres, three opaque ones, three walls and a pane in
front of the camera) at shadow_fixture's camera A, 48x32 and 13x8 (partial tiles), depth 3; scene
S (8 spheres + 4 walls) at cameras A and B; scene L (64 spheres + 6 walls: the wave-cull
kernels) at camera B, depth 6; the 1,536 scaled rays of camera A on G.  test_glass_host.py
confirms their content on the CPU.
"""
import contextlib

import numpy as np
import pytest

import glass_fixture as gfx
import lights_fixture as lfx
import shadow_fixture as sfx
from conftest import has_gpu
from rtamd import capi

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")]

F64, F32, MIXED, PATH64 = (capi.RT_PREC_F64, capi.RT_PREC_F32, capi.RT_PREC_MIXED,
                           capi.RT_PREC_PATH64)
O32, O64 = capi.RT_OUT_RGB_F32, capi.RT_OUT_RGB_F64
SH = capi.RT_FLAG_SHADOWS
F64_TOL = 1e-12      # the project's F64 bar
PATH64_TOL = 2e-5    # fp32 colour against fp64 colour on the same paths
OUTLIER_CAP = 0.005  # pixels of a frame that may exceed F64_TOL at all
INT32_MAX = 2 ** 31 - 1
DEFAULTS = {capi.RT_OPT_WAVE_CULL_MIN_SPHERES: 24, capi.RT_OPT_CLUSTER_COS: 400,
            capi.RT_OPT_SUPERSAMPLE: 1, capi.RT_OPT_FRAME_BATCH: 1, capi.RT_OPT_TILE_BINS: 1,
            capi.RT_OPT_EYE_TABLES: 1, capi.RT_OPT_MIRROR_BINS: 1}


@pytest.fixture(scope="module")
def rend():
    r = capi.Renderer(0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def bare():
    """A ctx that never had records."""
    r = capi.Renderer(0)
    yield r
    r.close()


_scene_on = {}


def use_scene(rend, key):
    """Scene G, S or L on rend (rt_set_scene clears the records)."""
    if _scene_on.get(id(rend)) != key:
        rend.set_scene(gfx.scene(key)[0])
        _scene_on[id(rend)] = key


@contextlib.contextmanager
def glassy(rend, key, lights="NONE"):
    """rend with scene `key`, its records and the named light set; cleared afterwards."""
    use_scene(rend, key)
    rend.set_transmission(gfx.scene(key)[1])
    rend.set_lights(None if lights == "NONE" else lfx.SETS[lights])
    try:
        yield
    finally:
        rend.set_lights(None)
        rend.set_transmission(None)


@contextlib.contextmanager
def options(rend, **kv):
    opts = {getattr(capi, k): v for k, v in kv.items()}
    for k, v in opts.items():
        rend.set_option(k, v)
    try:
        yield
    finally:
        for k in opts:
            rend.set_option(k, DEFAULTS.get(k, 0))


def check_against_fixture(got, tr, H, W, what):
    """test_lights_gpu.check_against_fixture's rule: every pixel within F64_TOL of the fixture; one
    above it only on a geometric discontinuity (3x3 neighbourhood of differing hit-index
    sequences) or where fragile, and at most OUTLIER_CAP of the frame at all."""
    d = np.abs(got.reshape(H, W, 3) - tr.rgb.reshape(H, W, 3)).max(axis=-1)
    bad = d > F64_TOL
    allowed = sfx.discontinuity_mask(tr.hits, H, W) | tr.fragile.reshape(H, W)
    print(f"{what}: max|d| = {d.max():.3e}, above {F64_TOL:g}: {int(bad.sum())}/{bad.size}, "
          f"fragile {int(tr.fragile.sum())}")
    assert not (bad & ~allowed).any(), (what, np.argwhere(bad & ~allowed)[:4].tolist(), d.max())
    assert bad.mean() <= OUTLIER_CAP, (what, int(bad.sum()))


# ------------------------------------------------- 1. F64 frames against the fixture
@pytest.mark.parametrize("lights", ["NONE", "K4"])
@pytest.mark.parametrize("name", ["G", "G13", "SA", "SB", "L"])
def test_f64_frames_against_the_fixture(rend, name, lights):
    key = gfx.CASES[name][0]
    for flags in (0, SH):
        _, _, cam, depth, tr = gfx.case(name, lights, bool(flags))
        with glassy(rend, key, lights):
            img, _ = rend.render(cam, depth, F64, flags, O64)
        check_against_fixture(img, tr, cam.height, cam.width, f"{name} {lights} flags {flags}")
        opaque = gfx.case(name, lights, bool(flags), glass=False)[4]
        assert np.abs(img.reshape(-1, 3) - opaque.rgb).max() > 1e-3     # the records take part


# ------------------------------------------------- 2. other precisions, segment counts
@pytest.mark.parametrize("name,lights", [("G", "NONE"), ("G13", "K4"), ("SB", "NONE"), ("L", "K4")])
def test_mixed_path64_and_segments(rend, bare, name, lights):
    key = gfx.CASES[name][0]
    _, _, cam, depth, _ = gfx.case(name)
    use_scene(bare, key)
    _, st0 = bare.render(cam, depth, F64, 0, O64, count_segments=True)
    for flags in (0, SH):
        with glassy(rend, key, lights):
            f64, st = rend.render(cam, depth, F64, flags, O64, count_segments=True)
            mixed, stm = rend.render(cam, depth, MIXED, flags, O64, count_segments=True)
            p64, stp = rend.render(cam, depth, PATH64, flags, O64, count_segments=True)
        assert mixed.tobytes() == f64.tobytes()
        d = float(np.abs(p64 - f64).max())
        print(f"{name} {lights} flags {flags}: PATH64 vs F64 max|d| = {d:.3e}; segments {st.segments} "
              f"(opaque {st0.segments})")
        assert d <= PATH64_TOL
        assert st.segments == stm.segments == stp.segments > 0
        if key == "G":
            assert st.segments != st0.segments      # the paths themselves change


# ------------------------------------------------- 3. clearing restores the plain kernels
@pytest.mark.parametrize("how", ["n0", "zeros"])
def test_clearing_restores_the_plain_kernels(rend, bare, how):
    prims, trans = gfx.scene("G")
    _, _, cam, depth, _ = gfx.case("G")
    use_scene(rend, "G")
    use_scene(bare, "G")
    rend.set_transmission(trans)
    on = {(p, f): rend.render(cam, depth, p, f, O64)[0] for p in (F64, PATH64) for f in (0, SH)}
    if how == "n0":
        capi.check(rend.lib.rt_set_transmission(rend.ctx, None, 0), rend.ctx)
    else:
        rend.set_transmission([(0.0, 1.0 + (j % 3)) for j in range(len(prims))])
    for prec in (F64, PATH64):
        for flags in (0, SH):
            want, _ = bare.render(cam, depth, prec, flags, O64)
            got, _ = rend.render(cam, depth, prec, flags, O64)
            assert got.tobytes() == want.tobytes(), (prec, flags)
            assert on[(prec, flags)].tobytes() != want.tobytes(), (prec, flags)
    # everything the records exclude works again
    rend.render(cam, depth, F32, 0, O32)
    rend.render(cam, depth, F64, capi.RT_FLAG_SUN, O64)
    assert rend.tile_row_costs(cam, depth, PATH64, 0).shape == (capi.tile_rows_of(cam.height),)


def test_set_scene_clears_the_records(bare):
    prims, trans = gfx.scene("G")
    _, _, cam, depth, _ = gfx.case("G")
    use_scene(bare, "G")
    want, _ = bare.render(cam, depth, F64, 0, O64)
    with capi.Renderer(0) as r:
        arr, n = capi.transmission_array(trans)
        assert r.lib.rt_set_transmission(r.ctx, arr, n) == capi.RT_ERR_NO_SCENE
        capi.check(r.lib.rt_set_transmission(r.ctx, None, 0), r.ctx)    # n == 0 needs no scene
        r.set_scene(prims)
        r.set_transmission(trans)
        on, _ = r.render(cam, depth, F64, 0, O64)
        r.set_scene(prims)                         # the records belong to the old objects
        got, _ = r.render(cam, depth, F64, 0, O64)
        r.render(cam, depth, F32, 0, O32)
    assert got.tobytes() == want.tobytes() != on.tobytes()


# ------------------------------------------------- 4. scan variants
@pytest.mark.parametrize("prec,fmt", [(F64, O64), (PATH64, O32)])
@pytest.mark.parametrize("name", ["G", "L"])
def test_scan_variants_bitwise(rend, name, prec, fmt):
    """Tile bins, eye tables, mirror bins, the wave cull forced on and off, the cluster walk and
    the cone: the scan never changes a decision or a colour."""
    key = gfx.CASES[name][0]
    _, _, cam, depth, _ = gfx.case(name)
    variants = [dict(RT_OPT_TILE_BINS=0), dict(RT_OPT_EYE_TABLES=0), dict(RT_OPT_MIRROR_BINS=0),
                dict(RT_OPT_WAVE_CULL_MIN_SPHERES=0), dict(RT_OPT_WAVE_CULL_MIN_SPHERES=INT32_MAX)]
    variants += [dict(RT_OPT_WAVE_CULL_MIN_SPHERES=0, RT_OPT_CLUSTER_COS=cc) for cc in (-2000, 400, 2000)]
    with glassy(rend, key, "K4"):
        for flags in (0, SH):
            want, _ = rend.render(cam, depth, prec, flags, fmt)
            for kv in variants:
                with options(rend, **kv):
                    got, _ = rend.render(cam, depth, prec, flags, fmt)
                assert got.tobytes() == want.tobytes(), (name, kv, flags)


# ------------------------------------------------- 5. ray batches
@pytest.mark.parametrize("lights", ["NONE", "K4"])
def test_ray_batch_against_the_fixture(rend, bare, lights):
    cam = capi.camera_init(**sfx.CAM_A)
    use_scene(bare, "G")
    _, _, o, d, depth, _ = gfx.ray_case()
    rgb0, hits0, st0 = bare.trace_rays(o, d, depth, F64, 0, want_hits=True, count_segments=True)
    _, honly0, _ = bare.trace_rays(o, d, depth, F64, 0, want_rgb=False, want_hits=True)
    for flags in (0, SH):
        tr = gfx.ray_case(lights, bool(flags))[5]
        with glassy(rend, "G", lights):
            rgb, hits, st = rend.trace_rays(o, d, depth, F64, flags, want_hits=True, count_segments=True)
            p64, _, stp = rend.trace_rays(o, d, depth, PATH64, flags, count_segments=True)
            mixed, _, _ = rend.trace_rays(o, d, depth, MIXED, flags)
            with options(rend, RT_OPT_WAVE_CULL_MIN_SPHERES=0):  # the cull kernels: the same bytes
                culled = []
                for cc in (2000, -2000):
                    with options(rend, RT_OPT_CLUSTER_COS=cc):
                        culled.append(rend.trace_rays(o, d, depth, F64, flags)[0])
        check_against_fixture(rgb, tr, cam.height, cam.width, f"scaled rays of A on G, {lights}, flags {flags}")
        assert rgb.tobytes() != rgb0.tobytes()
        assert hits.tobytes() == hits0.tobytes() == honly0.tobytes()
        assert st.segments == stp.segments != st0.segments
        dp = float(np.abs(p64 - rgb).max())
        print(f"scaled rays {lights} flags {flags}: PATH64 vs F64 max|d| = {dp:.3e}")
        assert dp <= PATH64_TOL
        assert mixed.tobytes() == rgb.tobytes()
        for c in culled:
            assert c.tobytes() == rgb.tobytes()


@pytest.mark.parametrize("n", [1, 63, 65])
def test_ray_batch_tails_leave_sentinels(rend, n):
    import torch
    dev = torch.device("cuda", 0)
    _, _, o, d, depth, tr = gfx.ray_case()
    # the glass-bound rays first, so that a tail of one ray still passes through an object
    order = np.argsort(-tr.passes, kind="stable")
    o, d = o[order], d[order]
    assert tr.passes[order[0]] >= 1
    with glassy(rend, "G", "K4"):
        want, _, _ = rend.trace_rays(o[:n], d[:n], depth, F64, SH)
        do = torch.from_numpy(o[:n].copy()).to(dev)
        dd = torch.from_numpy(d[:n].copy()).to(dev)
        out = torch.full((n + 64, 3), -7.0, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        rend.trace_rays_device(do.data_ptr(), dd.data_ptr(), n, depth, out.data_ptr(), 0, F64, SH, O64)
        torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert got[:n].tobytes() == want.tobytes()
    assert (got[n:] == -7.0).all()


# ------------------------------------------------- 6. composition
def test_row_band_equals_the_full_frames_rows(rend):
    _, _, cam, depth, _ = gfx.case("G")
    with glassy(rend, "G", "K4"):
        for prec, fmt in ((F64, O64), (PATH64, O32)):
            full, _ = rend.render(cam, depth, prec, SH, fmt)
            band, _ = rend.render(cam, depth, prec, SH, fmt, row0=5, nrows=14)
            assert band.tobytes() == full[5:19].tobytes(), prec


def test_interleaved_parts_equal_the_frame(rend):
    import torch
    _, _, cam, depth, _ = gfx.case("G")
    buf = torch.full((cam.height, cam.width, 3), -1.0, dtype=torch.float64,
                     device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    with glassy(rend, "G"):
        want, _ = rend.render(cam, depth, F64, SH, O64)
        for part in range(2):
            rend.render_device_interleaved(cam, depth, 2, part, buf.data_ptr(), F64, SH, O64,
                                           out_frame_rows=True)
        torch.cuda.synchronize()
    assert buf.cpu().numpy().tobytes() == want.tobytes()


def tree_mean(frame, s):
    v = np.asarray(frame, np.float64)
    k = {1: 0, 2: 1, 4: 2, 8: 3}[s]
    for _ in range(k):
        v = v[:, 0::2] + v[:, 1::2]
    for _ in range(k):
        v = v[0::2] + v[1::2]
    return v * (1.0 / (s * s))


@pytest.mark.parametrize("name,lights", [("G13", "NONE"), ("L", "K4")])
def test_supersample_with_records(rend, name, lights):
    _, _, cam, depth, _ = gfx.case(name)
    with glassy(rend, gfx.CASES[name][0], lights):
        for prec in (F64, PATH64):
            big, _ = rend.render(capi.supersample_camera(cam, 2), depth, prec, SH, O64)
            with options(rend, RT_OPT_SUPERSAMPLE=2):
                got, _ = rend.render(cam, depth, prec, SH, O64)
            assert got.tobytes() == tree_mean(big, 2).tobytes(), (name, prec)


def test_frame_batch_launches_such_frames_singly(rend):
    import torch
    dev = torch.device("cuda", 0)
    _, _, cam, depth, _ = gfx.case("G")
    cams = [cam, capi.camera_init(**sfx.CAM_B)]
    outs = [torch.full((cam.height, cam.width, 3), -1.0, dtype=torch.float32, device=dev)
            for _ in range(6)]
    torch.cuda.synchronize()
    with glassy(rend, "G"):
        refs = [rend.render(c, depth, PATH64, 0, O32)[0] for c in cams]
        with options(rend, RT_OPT_FRAME_BATCH=4):
            rend.render_device_frames(cams, depth, [o.data_ptr() for o in outs], PATH64, 0, O32,
                                      nframes=6)
            torch.cuda.synchronize()
    for f, o in enumerate(outs):
        assert o.cpu().numpy().tobytes() == refs[f % 2].tobytes(), f


def test_multi_renderer_gathers_the_one_gpu_frame(rend):
    prims, trans = gfx.scene("G")
    _, _, cam, depth, _ = gfx.case("G")
    with glassy(rend, "G", "K4"):
        want, _ = rend.render(cam, depth, PATH64, SH, O32)
    use_scene(rend, "G")
    plain, _ = rend.render(cam, depth, PATH64, SH, O32)
    with capi.MultiRenderer([0, 0], transport=capi.RT_TRANSPORT_COPY) as m:
        m.set_scene(prims)
        m.set_lights(lfx.K4)
        m.set_transmission(trans)
        got, _ = m.render(cam, depth, PATH64, SH, O32)
        m.set_lights(None)
        m.set_transmission(None)
        back, _ = m.render(cam, depth, PATH64, SH, O32)
    assert got.tobytes() == want.tobytes()
    assert back.tobytes() == plain.tobytes() != want.tobytes()


def test_pixel_pairs_and_row_feedback_are_ignored(rend):
    _, _, cam, depth, _ = gfx.case("G")
    with glassy(rend, "G"):
        want, _ = rend.render(cam, depth, PATH64, 0, O32)
        with options(rend, RT_OPT_PIXEL_PAIRS=1):
            got, _ = rend.render(cam, depth, PATH64, 0, O32)
        assert got.tobytes() == want.tobytes()
        rend.set_option(capi.RT_OPT_ROW_FEEDBACK, 1)
        try:
            for _ in range(3):
                got, _ = rend.render(cam, depth, PATH64, 0, O32)
                assert got.tobytes() == want.tobytes()
        finally:
            rend.set_option(capi.RT_OPT_ROW_FEEDBACK, 32)


# ------------------------------------------------- 7. status codes, what ignores the records
def test_refusals_while_records_are_set(rend, bare):
    _, _, cam, depth, _ = gfx.case("G")
    use_scene(bare, "G")
    _, _, o, d, rdepth, _ = gfx.ray_case()
    aov0, _ = bare.render_aov(cam)
    ao0, _ = bare.render_ao(cam, ndirs=8, radius=2.0)
    mask0, cnt0, _ = bare.occluded(o, d, 1.5)
    _, honly0, _ = bare.trace_rays(o, d, rdepth, F64, 0, want_rgb=False, want_hits=True)
    boxes0 = capi.frame_boxes(gfx.scene("G")[0], cam)
    with glassy(rend, "G"):
        before, _ = rend.render(cam, depth, PATH64, 0, O32)
        for call in (lambda: rend.render(cam, depth, F32, 0, O32),
                     lambda: rend.render(cam, depth, F64, capi.RT_FLAG_SUN, O64),
                     lambda: rend.trace_rays(o, d, rdepth, F64, capi.RT_FLAG_SUN),
                     lambda: rend.tile_row_costs(cam, depth, PATH64, 0)):
            with pytest.raises(capi.RTError) as e:
                call()
            assert e.value.status == capi.RT_ERR_UNSUPPORTED
        after, _ = rend.render(cam, depth, PATH64, 0, O32)
        assert after.tobytes() == before.tobytes()
        # these ignore the records (a hits-only call with the sun bit too: nothing is shaded)
        aov, _ = rend.render_aov(cam)
        ao, _ = rend.render_ao(cam, ndirs=8, radius=2.0)
        mask, cnt, _ = rend.occluded(o, d, 1.5)
        _, honly, _ = rend.trace_rays(o, d, rdepth, F64, capi.RT_FLAG_SUN, want_rgb=False, want_hits=True)
        boxes = capi.frame_boxes(gfx.scene("G")[0], cam)
    for k in aov0:
        assert np.asarray(aov[k]).tobytes() == np.asarray(aov0[k]).tobytes(), k
    for k in ao0:
        assert np.asarray(ao[k]).tobytes() == np.asarray(ao0[k]).tobytes(), k
    assert mask.tobytes() == mask0.tobytes() and cnt == cnt0
    assert honly.tobytes() == honly0.tobytes()
    assert all(np.array_equal(a, b) for a, b in zip(boxes[:2], boxes0[:2])) and boxes[2] == boxes0[2]


def test_invalid_arguments_keep_the_previous_records(rend):
    prims, trans = gfx.scene("G")
    _, _, cam, depth, _ = gfx.case("G")
    nan, inf = float("nan"), float("inf")
    n = len(prims)

    def with0(rec):
        return capi.transmission_array([rec] + list(trans[1:]))[0]

    good, _ = capi.transmission_array(trans)
    with glassy(rend, "G"):
        want, _ = rend.render(cam, depth, F64, SH, O64)
        for arr, cnt in ((good, n - 1), (good, -1), (capi.transmission_array(list(trans) + [0])[0], n + 1),
                         (None, n), (with0((nan, 1.5)), n), (with0((.5, inf)), n), (with0((.5, nan)), n),
                         (with0((-.01, 1.5)), n), (with0((1.01, 1.5)), n), (with0((.5, .99)), n),
                         (with0((.5, 4.01)), n), (with0((0.0, 0.5)), n)):
            assert rend.lib.rt_set_transmission(rend.ctx, arr, cnt) == capi.RT_ERR_INVALID_ARG
            got, _ = rend.render(cam, depth, F64, SH, O64)
            assert got.tobytes() == want.tobytes(), cnt
        # the bounds themselves are accepted
        rend.set_transmission([(1.0, 4.0)] + list(trans[1:]))
        rend.set_transmission([(0.0, 1.0)] + list(trans[1:]))
    assert rend.lib.rt_set_transmission(None, good, n) == capi.RT_ERR_INVALID_ARG
