"""RT_FLAG_SHADOWS on an MI355X: the light ray fused into the trace kernels, for frames and
for ray batches, against tests/shadow_fixture.py (oracle + occluded_fixture, level by level).

Inputs are the smallest that take every path: scene S (8 spheres + 4 walls, the linear-scan
kernels) at cameras A (at the light) and B (off it), 48x32, depth 3; the 13-wide B frame
(partial tiles); scene L (64 spheres + 6 walls, the wave-cull kernels), camera B, depth 6.
test_shadows_host.py confirms on the CPU that each of them has shadowed hits with sphere and
wall blockers at levels 0 and above.
"""
import contextlib

import numpy as np
import pytest

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
DEFAULTS = {capi.RT_OPT_WAVE_CULL_MIN_SPHERES: 24, capi.RT_OPT_CLUSTER_COS: 400}


@pytest.fixture(scope="module")
def rend():
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
def options(rend, **kv):
    opts = {getattr(capi, k): v for k, v in kv.items()}
    for k, v in opts.items():
        rend.set_option(k, v)
    try:
        yield
    finally:
        for k in opts:
            rend.set_option(k, DEFAULTS.get(k, {capi.RT_OPT_SUPERSAMPLE: 1, capi.RT_OPT_FRAME_BATCH: 1}.get(k, 0)))


def check_against_fixture(got, tr, H, W, what):
    """Every pixel within F64_TOL of the fixture; one above it only on a geometric
    discontinuity (3x3 neighbourhood of differing hit-index sequences) or where fragile, and
    at most OUTLIER_CAP of the frame at all."""
    d = np.abs(got.reshape(H, W, 3) - tr.rgb.reshape(H, W, 3)).max(axis=-1)
    bad = d > F64_TOL
    allowed = sfx.discontinuity_mask(tr.hits, H, W) | tr.fragile.reshape(H, W)
    print(f"{what}: max|d| = {d.max():.3e}, above {F64_TOL:g}: {int(bad.sum())}/{bad.size}, "
          f"fragile {int(tr.fragile.sum())}")
    assert not (bad & ~allowed).any(), (what, np.argwhere(bad & ~allowed)[:4].tolist(), d.max())
    assert bad.mean() <= OUTLIER_CAP, (what, int(bad.sum()))


# ------------------------------------------------- 3. F64 frames against the fixture
@pytest.mark.parametrize("name", ["A", "B", "B13", "L"])
def test_f64_frames_against_the_fixture(rend, name):
    prims, cam, depth, on = sfx.case(name, True)
    _, _, _, off = sfx.case(name, False)
    use_scene(rend, name)
    H, W = cam.height, cam.width
    plain, _ = rend.render(cam, depth, F64, 0, O64)
    check_against_fixture(plain, off, H, W, f"{name} unshadowed (control)")
    img, _ = rend.render(cam, depth, F64, SH, O64)
    check_against_fixture(img, on, H, W, f"{name} shadowed")


# ------------------------------------------------- 4. other precisions and options
@pytest.mark.parametrize("name", ["B", "B13", "L"])
def test_mixed_path64_and_segments(rend, name):
    _, cam, depth, _ = sfx.case(name, True)
    use_scene(rend, name)
    f64, st = rend.render(cam, depth, F64, SH, O64, count_segments=True)
    _, st0 = rend.render(cam, depth, F64, 0, O64, count_segments=True)
    mixed, stm = rend.render(cam, depth, MIXED, SH, O64, count_segments=True)
    p64, stp = rend.render(cam, depth, PATH64, SH, O64, count_segments=True)
    assert mixed.tobytes() == f64.tobytes()
    d = float(np.abs(p64 - f64).max())
    print(f"{name}: PATH64 vs F64, both shadowed: max|d| = {d:.3e}")
    assert d <= PATH64_TOL
    assert st.segments == st0.segments == stm.segments == stp.segments > 0


@pytest.mark.parametrize("prec,fmt", [(F64, O64), (PATH64, O32)])
def test_scan_variants_bitwise(rend, prec, fmt):
    """Scene S forced through the cull kernels, scene L forced to the cluster walk and to the
    cone: the scan never changes a decision."""
    _, cam, depth, _ = sfx.case("B", True)
    use_scene(rend, "B")
    want, _ = rend.render(cam, depth, prec, SH, fmt)
    with options(rend, RT_OPT_WAVE_CULL_MIN_SPHERES=0):
        for cc in (400, 2000, -2000):
            with options(rend, RT_OPT_CLUSTER_COS=cc):
                got, _ = rend.render(cam, depth, prec, SH, fmt)
            assert got.tobytes() == want.tobytes(), ("S through the cull kernels", cc)
    _, cam, depth, _ = sfx.case("L", True)
    use_scene(rend, "L")
    want, _ = rend.render(cam, depth, prec, SH, fmt)
    for cc in (2000, -2000):
        with options(rend, RT_OPT_CLUSTER_COS=cc):
            got, _ = rend.render(cam, depth, prec, SH, fmt)
        assert got.tobytes() == want.tobytes(), ("L", cc)


# ------------------------------------------------- 5. depth 0, output formats
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


def test_depth_0_all_formats(rend):
    prims, cam, _, _ = sfx.case("A", True)
    import oracle as orc_mod
    tr = sfx.trace_frame(orc_mod.Oracle(), prims, cam, 0, True, want_fragile=False)
    use_scene(rend, "A")
    H, W = cam.height, cam.width
    f64, _ = rend.render(cam, 0, F64, SH, O64)
    check_against_fixture(f64, tr, H, W, "A depth 0 shadowed")
    plain, _ = rend.render(cam, 0, F64, 0, O64)
    assert f64.tobytes() != plain.tobytes()
    f32, _ = rend.render(cam, 0, F64, SH, O32)
    assert f32.tobytes() == f64.astype(np.float32).tobytes()
    for fmt, conv in ((O8, q8), (O8W, q8_wrap)):
        got, _ = rend.render(cam, 0, F64, SH, fmt)
        assert np.array_equal(got[..., :3], conv(f64)) and (got[..., 3] == 255).all(), fmt
    p32, _ = rend.render(cam, 0, PATH64, SH, O32)
    got, _ = rend.render(cam, 0, PATH64, SH, O8)
    assert np.array_equal(got[..., :3], q8(p32.astype(np.float64)))


# ------------------------------------------------- 6. ray batches
def test_ray_batch_against_the_fixture(rend):
    prims, o, d, depth, on = sfx.ray_case(True)
    cam = capi.camera_init(**sfx.CAM_B)
    use_scene(rend, "B")
    rgb, hits, st = rend.trace_rays(o, d, depth, F64, SH, want_hits=True, count_segments=True)
    check_against_fixture(rgb, on, cam.height, cam.width, "scaled rays of B, shadowed")
    rgb0, hits0, st0 = rend.trace_rays(o, d, depth, F64, 0, want_hits=True, count_segments=True)
    assert hits.tobytes() == hits0.tobytes() and st.segments == st0.segments
    assert rgb.tobytes() != rgb0.tobytes()
    p64, _, _ = rend.trace_rays(o, d, depth, PATH64, SH)
    assert float(np.abs(p64 - rgb).max()) <= PATH64_TOL
    mixed, _, _ = rend.trace_rays(o, d, depth, MIXED, SH)
    assert mixed.tobytes() == rgb.tobytes()
    # a hits-only call ignores the flag (with the sun bit too: nothing is shaded)
    _, h1, _ = rend.trace_rays(o, d, depth, F64, SH | capi.RT_FLAG_SUN, want_rgb=False, want_hits=True)
    assert h1.tobytes() == hits0.tobytes()
    # the cull kernels give the same bytes
    with options(rend, RT_OPT_WAVE_CULL_MIN_SPHERES=0):
        for cc in (2000, -2000):
            with options(rend, RT_OPT_CLUSTER_COS=cc):
                got, _, _ = rend.trace_rays(o, d, depth, F64, SH)
            assert got.tobytes() == rgb.tobytes(), cc


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_ray_batch_tails_leave_sentinels(rend, n):
    import torch
    dev = torch.device("cuda", 0)
    _, o, d, depth, _ = sfx.ray_case(True)
    use_scene(rend, "B")
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


# ------------------------------------------------- 7. composition
def test_row_band_equals_the_full_frames_rows(rend):
    _, cam, depth, _ = sfx.case("B", True)
    use_scene(rend, "B")
    for prec, fmt in ((F64, O64), (PATH64, O32)):
        full, _ = rend.render(cam, depth, prec, SH, fmt)
        band, _ = rend.render(cam, depth, prec, SH, fmt, row0=5, nrows=14)
        assert band.tobytes() == full[5:19].tobytes(), prec


def test_interleaved_parts_equal_the_frame(rend):
    import torch
    _, cam, depth, _ = sfx.case("B", True)
    use_scene(rend, "B")
    want, _ = rend.render(cam, depth, F64, SH, O64)
    buf = torch.full((cam.height, cam.width, 3), -1.0, dtype=torch.float64,
                     device=torch.device("cuda", 0))
    torch.cuda.synchronize()
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


@pytest.mark.parametrize("name", ["B13", "L"])
def test_supersample_with_shadows(rend, name):
    _, cam, depth, _ = sfx.case(name, True)
    use_scene(rend, name)
    for prec in (F64, PATH64):
        big, _ = rend.render(capi.supersample_camera(cam, 2), depth, prec, SH, O64)
        with options(rend, RT_OPT_SUPERSAMPLE=2):
            got, _ = rend.render(cam, depth, prec, SH, O64)
        assert got.tobytes() == tree_mean(big, 2).tobytes(), (name, prec)


def test_frame_batch_launches_shadowed_frames_singly(rend):
    import torch
    dev = torch.device("cuda", 0)
    _, cam, depth, _ = sfx.case("B", True)
    cams = [cam, capi.camera_init(**sfx.CAM_A)]
    use_scene(rend, "B")
    refs = [rend.render(c, depth, PATH64, SH, O32)[0] for c in cams]
    outs = [torch.full((cam.height, cam.width, 3), -1.0, dtype=torch.float32, device=dev)
            for _ in range(6)]
    torch.cuda.synchronize()
    with options(rend, RT_OPT_FRAME_BATCH=4):
        rend.render_device_frames(cams, depth, [o.data_ptr() for o in outs], PATH64, SH, O32,
                                  nframes=6)
        torch.cuda.synchronize()
    for f, o in enumerate(outs):
        assert o.cpu().numpy().tobytes() == refs[f % 2].tobytes(), f


def test_multi_renderer_gathers_the_one_gpu_frame(rend):
    prims, cam, depth, _ = sfx.case("B", True)
    use_scene(rend, "B")
    want, _ = rend.render(cam, depth, PATH64, SH, O32)
    with capi.MultiRenderer([0, 0], transport=capi.RT_TRANSPORT_COPY) as m:
        m.set_scene(prims)
        got, _ = m.render(cam, depth, PATH64, SH, O32)
    assert got.tobytes() == want.tobytes()


# ------------------------------------------------- 8. status codes and invariance
def test_refused_combinations_leave_the_ctx_usable(rend):
    _, cam, depth, _ = sfx.case("B", True)
    use_scene(rend, "B")
    before, _ = rend.render(cam, depth, PATH64, 0, O32)
    for call in (lambda: rend.render(cam, depth, F32, SH, O32),
                 lambda: rend.render(cam, depth, F64, SH | capi.RT_FLAG_SUN, O64),
                 lambda: rend.tile_row_costs(cam, depth, PATH64, SH)):
        with pytest.raises(capi.RTError) as e:
            call()
        assert e.value.status == capi.RT_ERR_UNSUPPORTED
    flagged, _ = rend.render(cam, depth, PATH64, SH, O32)
    after, _ = rend.render(cam, depth, PATH64, 0, O32)
    assert after.tobytes() == before.tobytes()
    assert flagged.tobytes() != before.tobytes()
    assert rend.tile_row_costs(cam, depth, PATH64, 0).shape == (capi.tile_rows_of(cam.height),)


def test_pixel_pairs_are_ignored(rend):
    _, cam, depth, _ = sfx.case("B", True)
    use_scene(rend, "B")
    want, _ = rend.render(cam, depth, PATH64, SH, O32)
    with options(rend, RT_OPT_PIXEL_PAIRS=1):
        got, _ = rend.render(cam, depth, PATH64, SH, O32)
    assert got.tobytes() == want.tobytes()
