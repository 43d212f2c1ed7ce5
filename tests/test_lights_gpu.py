"""Scene lights (rt_set_lights) on an MI355X: the lights kernels for frames and ray batches
against tests/lights_fixture.py (oracle + occluded_fixture, level by level), with and without
RT_FLAG_SHADOWS, and their composition with everything a frame can be combined with.

Inputs are shadow_fixture's: scene S (8 spheres + 4 walls, the linear-scan kernels) at cameras
A and B, 48x32, depth 3; the 13-wide B frame (partial tiles); scene L (64 spheres + 6 walls, the
wave-cull kernels), camera B, depth 6; the 1,536 scaled rays of B.  The light sets are
lights_fixture's ONE, K2, K4, K8; test_lights_host.py confirms their content on the CPU.
"""
import contextlib
import ctypes as C

import numpy as np
import pytest

import lights_fixture as lfx
import shadow_fixture as sfx
from conftest import has_gpu
from rtamd import capi

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")]

F64, F32, MIXED, PATH64 = (capi.RT_PREC_F64, capi.RT_PREC_F32, capi.RT_PREC_MIXED,
                           capi.RT_PREC_PATH64)
O32, O64, O8, O8W = (capi.RT_OUT_RGB_F32, capi.RT_OUT_RGB_F64, capi.RT_OUT_RGBA8,
                     capi.RT_OUT_RGBA8_WRAP)
SH = capi.RT_FLAG_SHADOWS
F64_TOL = 1e-12      # the project's F64 bar
PATH64_TOL = 2e-5    # fp32 colour against fp64 colour on the same paths
OUTLIER_CAP = 0.005  # pixels of a frame that may exceed F64_TOL at all
DEFAULTS = {capi.RT_OPT_WAVE_CULL_MIN_SPHERES: 24, capi.RT_OPT_CLUSTER_COS: 400,
            capi.RT_OPT_SUPERSAMPLE: 1, capi.RT_OPT_FRAME_BATCH: 1}


@pytest.fixture(scope="module")
def rend():
    r = capi.Renderer(0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def bare():
    """A ctx that never had lights."""
    r = capi.Renderer(0)
    yield r
    r.close()


_scene_on = {}


def use_scene(rend, name):
    ns, nw = sfx.CASES[name][:2]
    if _scene_on.get(id(rend)) != (ns, nw):
        rend.set_scene(sfx.scene_prims(ns, nw))
        _scene_on[id(rend)] = (ns, nw)


@contextlib.contextmanager
def lit(rend, lights):
    """rend with the named light set, back to the reference's light afterwards."""
    rend.set_lights(lfx.SETS[lights])
    try:
        yield
    finally:
        rend.set_lights(None)


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
    """test_shadows_gpu's rule: every pixel within F64_TOL of the fixture; one above it only on
    a geometric discontinuity (3x3 neighbourhood of differing hit-index sequences) or where
    fragile, and at most OUTLIER_CAP of the frame at all."""
    d = np.abs(got.reshape(H, W, 3) - tr.rgb.reshape(H, W, 3)).max(axis=-1)
    bad = d > F64_TOL
    allowed = sfx.discontinuity_mask(tr.hits, H, W) | tr.fragile.reshape(H, W)
    print(f"{what}: max|d| = {d.max():.3e}, above {F64_TOL:g}: {int(bad.sum())}/{bad.size}, "
          f"fragile {int(tr.fragile.sum())}")
    assert not (bad & ~allowed).any(), (what, np.argwhere(bad & ~allowed)[:4].tolist(), d.max())
    assert bad.mean() <= OUTLIER_CAP, (what, int(bad.sum()))


# ------------------------------------------------- 1. F64 frames against the fixture
@pytest.mark.parametrize("name,lights", [("A", "K4"), ("B", "K4"), ("B13", "K4"), ("L", "K2"),
                                         ("A", "K8")])
def test_f64_frames_against_the_fixture(rend, name, lights):
    use_scene(rend, name)
    for flags in (0, SH):
        _, cam, depth, tr = lfx.case(name, lights, bool(flags))
        with lit(rend, lights):
            img, _ = rend.render(cam, depth, F64, flags, O64)
        check_against_fixture(img, tr, cam.height, cam.width, f"{name} {lights} flags {flags}")


# ------------------------------------------------- 2. the reference's light through the lights kernels
@pytest.mark.parametrize("name", ["B", "L"])
def test_one_white_light_gives_the_light_less_bytes(rend, bare, name):
    _, cam, depth, _ = sfx.case(name, False)
    use_scene(rend, name)
    use_scene(bare, name)
    _, o, d, rdepth, _ = sfx.ray_case(False)
    for flags in (0, SH):
        want, _ = bare.render(cam, depth, F64, flags, O64)
        rwant, _, _ = bare.trace_rays(o, d, rdepth, F64, flags)
        with lit(rend, "ONE"):
            got, _ = rend.render(cam, depth, F64, flags, O64)
            rgot, _, _ = rend.trace_rays(o, d, rdepth, F64, flags)
        assert got.tobytes() == want.tobytes(), (name, flags)
        assert rgot.tobytes() == rwant.tobytes(), (name, flags)


# ------------------------------------------------- 3. n == 0 restores the plain kernels
def test_no_lights_after_k4_is_a_fresh_ctx(rend, bare):
    _, cam, depth, _ = sfx.case("B", False)
    use_scene(rend, "B")
    use_scene(bare, "B")
    with lit(rend, "K4"):
        k4 = {(p, f): rend.render(cam, depth, p, f, O64)[0] for p in (F64, PATH64) for f in (0, SH)}
    capi.check(rend.lib.rt_set_lights(rend.ctx, None, 0), rend.ctx)
    for prec in (F64, PATH64):
        for flags in (0, SH):
            want, _ = bare.render(cam, depth, prec, flags, O64)
            got, _ = rend.render(cam, depth, prec, flags, O64)
            assert got.tobytes() == want.tobytes(), (prec, flags)
            assert k4[(prec, flags)].tobytes() != want.tobytes(), (prec, flags)


# ------------------------------------------------- 4. other precisions, segment counts
@pytest.mark.parametrize("name,lights", [("B", "K4"), ("B13", "K4"), ("L", "K2")])
def test_mixed_path64_and_segments(rend, bare, name, lights):
    _, cam, depth, _ = sfx.case(name, False)
    use_scene(rend, name)
    use_scene(bare, name)
    _, st0 = bare.render(cam, depth, F64, 0, O64, count_segments=True)
    for flags in (0, SH):
        with lit(rend, lights):
            f64, st = rend.render(cam, depth, F64, flags, O64, count_segments=True)
            mixed, stm = rend.render(cam, depth, MIXED, flags, O64, count_segments=True)
            p64, stp = rend.render(cam, depth, PATH64, flags, O64, count_segments=True)
        assert mixed.tobytes() == f64.tobytes()
        d = float(np.abs(p64 - f64).max())
        print(f"{name} {lights} flags {flags}: PATH64 vs F64 max|d| = {d:.3e}")
        assert d <= PATH64_TOL
        assert st.segments == st0.segments == stm.segments == stp.segments > 0


# ------------------------------------------------- 5. scan variants
@pytest.mark.parametrize("prec,fmt", [(F64, O64), (PATH64, O32)])
def test_scan_variants_bitwise(rend, prec, fmt):
    """Scene S forced through the cull kernels, scene L forced to the cluster walk and to the
    cone: the scan never changes a decision or a colour."""
    _, cam, depth, _ = sfx.case("B", False)
    use_scene(rend, "B")
    with lit(rend, "K4"):
        for flags in (0, SH):
            want, _ = rend.render(cam, depth, prec, flags, fmt)
            with options(rend, RT_OPT_WAVE_CULL_MIN_SPHERES=0):
                for cc in (400, 2000, -2000):
                    with options(rend, RT_OPT_CLUSTER_COS=cc):
                        got, _ = rend.render(cam, depth, prec, flags, fmt)
                    assert got.tobytes() == want.tobytes(), ("S through the cull kernels", cc, flags)
    _, cam, depth, _ = sfx.case("L", False)
    use_scene(rend, "L")
    with lit(rend, "K2"):
        for flags in (0, SH):
            want, _ = rend.render(cam, depth, prec, flags, fmt)
            for cc in (2000, -2000):
                with options(rend, RT_OPT_CLUSTER_COS=cc):
                    got, _ = rend.render(cam, depth, prec, flags, fmt)
                assert got.tobytes() == want.tobytes(), ("L", cc, flags)


# ------------------------------------------------- 6. depth 0, output formats
def q8(v):
    v = np.where(v > 0.0, v, 0.0)
    v = np.where(v < 1.0, v, 1.0)
    return (v * 255.0).astype(np.uint32).astype(np.uint8)


def q8_wrap(v):
    """RT_OUT_RGBA8_WRAP's: int32 truncation of v * 255, low byte (highlights above 1 wrap)."""
    t = v * 255.0
    ok = (t > -2147483649.0) & (t < 2147483648.0)
    i = np.where(ok, np.trunc(np.where(ok, t, 0.0)), -2147483648.0).astype(np.int64)
    return (i & 0xff).astype(np.uint8)


def test_depth_0_k8_all_formats(rend):
    use_scene(rend, "A")
    for flags in (0, SH):
        _, cam, _, tr = lfx.case("A", "K8", bool(flags), depth=0)
        with lit(rend, "K8"):
            f64, _ = rend.render(cam, 0, F64, flags, O64)
            f32, _ = rend.render(cam, 0, F64, flags, O32)
            b8 = {fmt: rend.render(cam, 0, F64, flags, fmt)[0] for fmt in (O8, O8W)}
        check_against_fixture(f64, tr, cam.height, cam.width, f"A K8 depth 0 flags {flags}")
        assert f64.max() > 1.0     # saturation and wrap are exercised
        assert f32.tobytes() == f64.astype(np.float32).tobytes()
        for fmt, conv in ((O8, q8), (O8W, q8_wrap)):
            got = b8[fmt]
            assert np.array_equal(got[..., :3], conv(f64)) and (got[..., 3] == 255).all(), fmt
        assert not np.array_equal(b8[O8], b8[O8W])


# ------------------------------------------------- 7. ray batches
def test_ray_batch_against_the_fixture(rend, bare):
    cam = capi.camera_init(**sfx.CAM_B)
    use_scene(rend, "B")
    use_scene(bare, "B")
    _, o, d, depth, _ = lfx.ray_case("K4", False)
    rgb0, hits0, st0 = bare.trace_rays(o, d, depth, F64, 0, want_hits=True, count_segments=True)
    _, honly0, _ = bare.trace_rays(o, d, depth, F64, 0, want_rgb=False, want_hits=True)
    mask0, cnt0, _ = bare.occluded(o, d, 1.5)
    for flags in (0, SH):
        tr = lfx.ray_case("K4", bool(flags))[4]
        with lit(rend, "K4"):
            rgb, hits, st = rend.trace_rays(o, d, depth, F64, flags, want_hits=True, count_segments=True)
            p64, _, _ = rend.trace_rays(o, d, depth, PATH64, flags)
            mixed, _, _ = rend.trace_rays(o, d, depth, MIXED, flags)
            # a hits-only call ignores the lights (with the sun bit too: nothing is shaded)
            _, honly, _ = rend.trace_rays(o, d, depth, F64, flags | capi.RT_FLAG_SUN, want_rgb=False,
                                          want_hits=True)
            mask, cnt, _ = rend.occluded(o, d, 1.5)
            with options(rend, RT_OPT_WAVE_CULL_MIN_SPHERES=0):  # the cull kernels: the same bytes
                culled = []
                for cc in (2000, -2000):
                    with options(rend, RT_OPT_CLUSTER_COS=cc):
                        culled.append(rend.trace_rays(o, d, depth, F64, flags)[0])
        check_against_fixture(rgb, tr, cam.height, cam.width, f"scaled rays of B, K4, flags {flags}")
        assert rgb.tobytes() != rgb0.tobytes()
        assert hits.tobytes() == hits0.tobytes() and st.segments == st0.segments
        dp = float(np.abs(p64 - rgb).max())
        print(f"scaled rays flags {flags}: PATH64 vs F64 max|d| = {dp:.3e}")
        assert dp <= PATH64_TOL
        assert mixed.tobytes() == rgb.tobytes()
        assert honly.tobytes() == honly0.tobytes()
        assert mask.tobytes() == mask0.tobytes() and cnt == cnt0
        for c in culled:
            assert c.tobytes() == rgb.tobytes()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_ray_batch_tails_leave_sentinels(rend, n):
    import torch
    dev = torch.device("cuda", 0)
    _, o, d, depth, _ = sfx.ray_case(False)
    use_scene(rend, "B")
    with lit(rend, "K4"):
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


# ------------------------------------------------- 8. composition
def test_row_band_equals_the_full_frames_rows(rend):
    _, cam, depth, _ = sfx.case("B", False)
    use_scene(rend, "B")
    with lit(rend, "K4"):
        for prec, fmt in ((F64, O64), (PATH64, O32)):
            full, _ = rend.render(cam, depth, prec, SH, fmt)
            band, _ = rend.render(cam, depth, prec, SH, fmt, row0=5, nrows=14)
            assert band.tobytes() == full[5:19].tobytes(), prec


def test_interleaved_parts_equal_the_frame(rend):
    import torch
    _, cam, depth, _ = sfx.case("B", False)
    use_scene(rend, "B")
    buf = torch.full((cam.height, cam.width, 3), -1.0, dtype=torch.float64,
                     device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    with lit(rend, "K4"):
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


@pytest.mark.parametrize("name,lights", [("B13", "K4"), ("L", "K2")])
def test_supersample_with_lights(rend, name, lights):
    _, cam, depth, _ = sfx.case(name, False)
    use_scene(rend, name)
    with lit(rend, lights):
        for prec in (F64, PATH64):
            big, _ = rend.render(capi.supersample_camera(cam, 2), depth, prec, SH, O64)
            with options(rend, RT_OPT_SUPERSAMPLE=2):
                got, _ = rend.render(cam, depth, prec, SH, O64)
            assert got.tobytes() == tree_mean(big, 2).tobytes(), (name, prec)


def test_frame_batch_launches_lit_frames_singly(rend):
    import torch
    dev = torch.device("cuda", 0)
    _, cam, depth, _ = sfx.case("B", False)
    cams = [cam, capi.camera_init(**sfx.CAM_A)]
    use_scene(rend, "B")
    outs = [torch.full((cam.height, cam.width, 3), -1.0, dtype=torch.float32, device=dev)
            for _ in range(6)]
    torch.cuda.synchronize()
    with lit(rend, "K4"):
        refs = [rend.render(c, depth, PATH64, 0, O32)[0] for c in cams]
        with options(rend, RT_OPT_FRAME_BATCH=4):
            rend.render_device_frames(cams, depth, [o.data_ptr() for o in outs], PATH64, 0, O32,
                                      nframes=6)
            torch.cuda.synchronize()
    for f, o in enumerate(outs):
        assert o.cpu().numpy().tobytes() == refs[f % 2].tobytes(), f


def test_multi_renderer_gathers_the_one_gpu_frame(rend):
    prims, cam, depth, _ = sfx.case("B", False)
    use_scene(rend, "B")
    with lit(rend, "K4"):
        want, _ = rend.render(cam, depth, PATH64, SH, O32)
    plain, _ = rend.render(cam, depth, PATH64, SH, O32)
    with capi.MultiRenderer([0, 0], transport=capi.RT_TRANSPORT_COPY) as m:
        m.set_scene(prims)
        m.set_lights(lfx.K4)
        got, _ = m.render(cam, depth, PATH64, SH, O32)
        m.set_lights(None)
        back, _ = m.render(cam, depth, PATH64, SH, O32)
    assert got.tobytes() == want.tobytes()
    assert back.tobytes() == plain.tobytes() != want.tobytes()


# ------------------------------------------------- 9. status codes
def test_refusals_while_lights_are_set(rend):
    _, cam, depth, _ = sfx.case("B", False)
    use_scene(rend, "B")
    _, o, d, rdepth, _ = sfx.ray_case(False)
    with lit(rend, "K2"):
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
    # without lights all of them work again
    rend.render(cam, depth, F32, 0, O32)
    rend.render(cam, depth, F64, capi.RT_FLAG_SUN, O64)
    assert rend.tile_row_costs(cam, depth, PATH64, 0).shape == (capi.tile_rows_of(cam.height),)


def test_invalid_arguments_keep_the_previous_lights(rend):
    _, cam, depth, _ = sfx.case("B", False)
    use_scene(rend, "B")
    nan, inf = float("nan"), float("inf")
    nine, _ = capi.light_array(lfx.K8 + lfx.ONE)
    one, _ = capi.light_array(lfx.ONE)
    badpos, _ = capi.light_array([((0, nan, 0), (1, 1, 1))])
    badcol, _ = capi.light_array([((0, 0, 0), (1, -inf, 1))])
    with lit(rend, "K2"):
        want, _ = rend.render(cam, depth, F64, SH, O64)
        for arr, n in ((nine, 9), (one, -1), (None, 1), (badpos, 1), (badcol, 1)):
            assert rend.lib.rt_set_lights(rend.ctx, arr, n) == capi.RT_ERR_INVALID_ARG
            got, _ = rend.render(cam, depth, F64, SH, O64)
            assert got.tobytes() == want.tobytes(), n
    assert rend.lib.rt_set_lights(None, one, 1) == capi.RT_ERR_INVALID_ARG


def test_pixel_pairs_are_ignored(rend):
    _, cam, depth, _ = sfx.case("B", False)
    use_scene(rend, "B")
    with lit(rend, "K4"):
        want, _ = rend.render(cam, depth, PATH64, 0, O32)
        with options(rend, RT_OPT_PIXEL_PAIRS=1):
            got, _ = rend.render(cam, depth, PATH64, 0, O32)
    assert got.tobytes() == want.tobytes()


def test_lights_before_and_across_set_scene(rend):
    _, cam, depth, _ = sfx.case("B", False)
    use_scene(rend, "B")
    with lit(rend, "K4"):
        want, _ = rend.render(cam, depth, F64, SH, O64)
    with capi.Renderer(0) as r:
        r.set_lights(lfx.K4)                     # valid before rt_set_scene
        r.set_scene(sfx.scene_prims(64, 6))
        r.set_scene(sfx.scene_prims(8, 4))       # the lights survive rt_set_scene
        got, _ = r.render(cam, depth, F64, SH, O64)
    assert got.tobytes() == want.tobytes()
