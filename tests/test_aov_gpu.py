"""GPU: frame AOVs (rt_render_aov / rt_render_aov_device) against the expected layers of
tests/aov_fixture.py, on an MI355X (`pytest -m gpu`).  Every layer is defined operation by
operation, so every comparison of layers is bytewise.  Frames are 48 x 32, 32 x 24 or 13 x 8."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import aov_fixture as afx
import lights_fixture as lfx
import shadow_fixture as sfx
from conftest import has_gpu
from rtamd import capi

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")]

LAYERS = afx.LAYERS
INT32_MAX = 2**31 - 1
DEFAULTS = {capi.RT_OPT_WAVE_CULL_MIN_SPHERES: 24, capi.RT_OPT_TILE_BINS: 1,
            capi.RT_OPT_EYE_TABLES: 1, capi.RT_OPT_WALL_ORDER: 0, capi.RT_OPT_CLUSTER_COS: 400,
            capi.RT_OPT_SUPERSAMPLE: 1}
OPTION_SETS = {
    "tile_bins_off": {capi.RT_OPT_TILE_BINS: 0},
    "eye_tables_off": {capi.RT_OPT_EYE_TABLES: 0},
    "wall_order_on": {capi.RT_OPT_WALL_ORDER: 1},
    "wave_cull_all": {capi.RT_OPT_WAVE_CULL_MIN_SPHERES: 0},
    "wave_cull_never": {capi.RT_OPT_WAVE_CULL_MIN_SPHERES: INT32_MAX},
    "clusters_never": {capi.RT_OPT_CLUSTER_COS: -2000},
    "clusters_always": {capi.RT_OPT_CLUSTER_COS: 2000},
    # the cluster walk on the small scene too (it only exists behind the wave cull)
    "cull_all_clusters_always": {capi.RT_OPT_WAVE_CULL_MIN_SPHERES: 0, capi.RT_OPT_CLUSTER_COS: 2000},
    "cull_all_clusters_never": {capi.RT_OPT_WAVE_CULL_MIN_SPHERES: 0, capi.RT_OPT_CLUSTER_COS: -2000},
}
GUARD = 16       # sentinel elements behind every buffer
SENTINEL = 0xAB


@pytest.fixture(scope="module")
def rend():
    r = capi.Renderer(0)
    yield r
    r.close()


@contextlib.contextmanager
def options(rend, opts):
    try:
        for k, v in opts.items():
            rend.set_option(k, v)
        yield
    finally:
        for k in opts:
            rend.set_option(k, DEFAULTS[k])


def guarded(name, npx):
    """A buffer of npx pixels of layer `name` plus GUARD elements, every byte SENTINEL."""
    dt, tail = capi.AOV_LAYERS[name]
    buf = np.empty((npx + GUARD,) + tail, dt)
    buf.view(np.uint8)[...] = SENTINEL
    return buf


def untouched(buf, first=0):
    return bool((np.ascontiguousarray(buf[first:]).view(np.uint8) == SENTINEL).all())


def aov_guarded(rend, cam, layers, row0=0, nrows=None):
    """rt_render_aov into guarded buffers for every layer; only `layers` are passed.  Returns
    {layer: [nrows, W(, 3)]} of the requested ones after checking that nothing behind them, and
    nothing of the buffers not passed, was written."""
    nrows = cam.height - row0 if nrows is None else nrows
    npx = nrows * cam.width
    bufs = {name: guarded(name, npx) for name in LAYERS}
    arg = capi.rt_aov_buffers(**{name: bufs[name].ctypes.data for name in layers})
    st = capi.rt_stats()
    capi.check(rend.lib.rt_render_aov(rend.ctx, C.byref(cam), row0, nrows, C.byref(arg), C.byref(st)),
               rend.ctx)
    assert st.segments == npx and st.ms > 0
    out = {}
    for name in LAYERS:
        if name in layers:
            assert untouched(bufs[name], npx), name
            out[name] = bufs[name][:npx].reshape((nrows, cam.width) + bufs[name].shape[1:])
        else:
            assert untouched(bufs[name]), name
    return out


def assert_layers(got, exp, rows=slice(None), what=""):
    for name in got:
        assert afx.same_bytes(got[name], exp[name][rows]), (what, name)


# ---------------------------------------------------------------- 1. the layers
@pytest.mark.parametrize("name", ["A", "B", "B13", "L", "views"])
def test_layers_match_fixture(rend, name):
    prims, cam, exp = afx.case(name)
    rend.set_scene(prims)
    got, st = rend.render_aov(cam)
    assert set(got) == set(LAYERS) and st.segments == cam.width * cam.height
    assert got["hit"].dtype == capi.HIT_DTYPE and got["hit"].shape == (cam.height, cam.width)
    assert got["normal"].shape == (cam.height, cam.width, 3) and got["normal"].dtype == np.float32
    print("aov", name, "misses / spheres / walls", afx.counts(exp))
    assert_layers(got, exp, what=name)


def test_empty_scene_all_misses(rend):
    _, cam, _ = afx.case("B13")
    rend.set_scene([])
    got, _ = rend.render_aov(cam)
    assert (got["index"] == -1).all() and np.isposinf(got["depth"]).all()
    assert (got["hit"]["distance"] == afx.DBL_MAX).all() and (got["hit"]["index"] == -1).all()
    for k in ("normal", "albedo"):
        assert not got[k].view(np.uint32).any()
    assert not got["hit"]["normal"].view(np.uint64).any() and not got["hit"]["reserved"].any()


# ---------------------------------------------------------------- 2. the record is k_ray_hits'
@pytest.mark.parametrize("name", ["A", "L"])
def test_hit_equals_trace_rays_record(rend, name):
    prims, cam, _ = afx.case(name)
    rend.set_scene(prims)
    o, d = sfx.camera_rays(cam)
    _, hits, _ = rend.trace_rays(o, d, 0, want_rgb=False, want_hits=True)
    got, _ = rend.render_aov(cam, layers=("hit",))
    assert afx.same_bytes(got["hit"].reshape(-1), hits)


# ---------------------------------------------------------------- 3. layers alone, guards
@pytest.mark.parametrize("name", ["B13", "L"])
def test_each_layer_alone_and_guards(rend, name):
    prims, cam, exp = afx.case(name)
    rend.set_scene(prims)
    assert_layers(aov_guarded(rend, cam, LAYERS), exp, what="all")
    for layer in LAYERS:
        assert_layers(aov_guarded(rend, cam, (layer,)), exp, what=layer)
    assert_layers(aov_guarded(rend, cam, ("index", "depth")), exp, what="index+depth")


# ---------------------------------------------------------------- 4. bands
@pytest.mark.parametrize("name", ["A", "L"])
def test_bands_equal_frame_slices(rend, name):
    prims, cam, exp = afx.case(name)
    rend.set_scene(prims)
    for row0, nrows in ((3, 18), (17, 1), (0, 1), (cam.height - 1, 1)):
        got = aov_guarded(rend, cam, LAYERS, row0, nrows)
        assert_layers(got, exp, slice(row0, row0 + nrows), what=(row0, nrows))


def test_band_statuses_are_rt_renders(rend):
    prims, cam, _ = afx.case("A")
    rend.set_scene(prims)
    H, npx = cam.height, cam.width * cam.height
    idx = guarded("index", npx)
    arg = capi.rt_aov_buffers(index=idx.ctypes.data)
    img = np.empty((H + 1, cam.width, 3), np.float32)
    seen = set()
    for row0, nrows in ((-1, 4), (H - 2, 4), (0, H + 1), (H, 1), (0, -1), (-1, -1), (H, 0), (H + 1, 0),
                        (0, 0)):
        a = rend.lib.rt_render_aov(rend.ctx, C.byref(cam), row0, nrows, C.byref(arg), None)
        b = rend.lib.rt_render_aov_device(rend.ctx, C.byref(cam), row0, nrows, C.byref(arg), None)
        r = rend.lib.rt_render(rend.ctx, C.byref(cam), row0, nrows, 0, capi.RT_PREC_F64, 0,
                               capi.RT_OUT_RGB_F32, img.ctypes.data_as(C.c_void_p), 0, None)
        assert a == r and b == r, (row0, nrows, a, b, r)
        seen.add(r)
    assert untouched(idx)
    assert {capi.RT_OK, capi.RT_ERR_INVALID_ARG, capi.RT_ERR_OUT_OF_RANGE} <= seen


# ---------------------------------------------------------------- 5. option invariance
@pytest.mark.parametrize("name", ["A", "L"])
@pytest.mark.parametrize("optset", list(OPTION_SETS))
def test_option_invariance(rend, name, optset):
    prims, cam, exp = afx.case(name)
    rend.set_scene(prims)
    with options(rend, OPTION_SETS[optset]):
        got, _ = rend.render_aov(cam)
    assert_layers(got, exp, what=(name, optset))


# ---------------------------------------------------------------- 6. non-interference
def test_frames_and_feedback_undisturbed():
    """RT_OPT_ROW_FEEDBACK at its default: render, AOV, render gives two identical colour frames
    (segment counts included), and the AOV between them is a fresh ctx's."""
    prims, cam, exp = afx.case("A")
    with capi.Renderer(0) as r:
        r.set_scene(prims)
        a, sa = r.render(cam, 3, capi.RT_PREC_PATH64, 0, capi.RT_OUT_RGB_F32, count_segments=True)
        got, _ = r.render_aov(cam)
        b, sb = r.render(cam, 3, capi.RT_PREC_PATH64, 0, capi.RT_OUT_RGB_F32, count_segments=True)
        assert afx.same_bytes(a, b) and sa.segments == sb.segments
        # a band of the frame, then the AOV of another band, then the band again
        c, _ = r.render(cam, 3, capi.RT_PREC_F64, 0, capi.RT_OUT_RGB_F64, row0=8, nrows=16)
        band, _ = r.render_aov(cam, row0=3, nrows=18)
        e, _ = r.render(cam, 3, capi.RT_PREC_F64, 0, capi.RT_OUT_RGB_F64, row0=8, nrows=16)
        assert afx.same_bytes(c, e)
        assert_layers(band, exp, slice(3, 21), what="band")
    with capi.Renderer(0) as fresh:
        fresh.set_scene(prims)
        alone, _ = fresh.render_aov(cam)
    assert_layers(got, alone, what="fresh")
    assert_layers(got, exp, what="fixture")


def test_lights_and_supersample_ignored(rend):
    prims, cam, exp = afx.case("A")
    rend.set_scene(prims)
    try:
        rend.set_lights(lfx.K4)
        rend.set_option(capi.RT_OPT_SUPERSAMPLE, 2)
        got, st = rend.render_aov(cam)
    finally:
        rend.set_lights(None)
        rend.set_option(capi.RT_OPT_SUPERSAMPLE, 1)
    assert st.segments == cam.width * cam.height
    assert got["index"].shape == (cam.height, cam.width)
    assert_layers(got, exp, what="lights + S = 2")


def test_supersample_camera_gives_the_samples(rend, oracle):
    """The samples' AOVs: rt_supersample_camera's camera (26 x 16 for B13 at S = 2)."""
    prims, cam, _ = afx.case("B13")
    cam2 = capi.supersample_camera(cam, 2)
    assert (cam2.width, cam2.height) == (2 * cam.width, 2 * cam.height)
    rend.set_scene(prims)
    got, _ = rend.render_aov(cam2)
    assert_layers(got, afx.expected(oracle, prims, cam2), what="S = 2 camera")


# ---------------------------------------------------------------- 7. device variant, statuses
def test_device_variant_on_a_torch_stream(rend):
    import torch
    prims, cam, exp = afx.case("L")
    rend.set_scene(prims)
    host, _ = rend.render_aov(cam)
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(dev)
    npx = cam.width * cam.height
    nbytes = {name: (npx + GUARD) * np.dtype(dt).itemsize * int(np.prod(tail, dtype=np.int64))
              for name, (dt, tail) in capi.AOV_LAYERS.items()}
    bufs = {name: torch.full((nbytes[name],), SENTINEL, dtype=torch.uint8, device=dev) for name in LAYERS}
    torch.cuda.synchronize()
    rend.render_aov_device(cam, {name: bufs[name].data_ptr() for name in LAYERS}, stream=st.cuda_stream)
    st.synchronize()
    for name, (dt, tail) in capi.AOV_LAYERS.items():
        raw = bufs[name].cpu().numpy()
        used = nbytes[name] // (npx + GUARD) * npx
        assert (raw[used:] == SENTINEL).all(), name
        got = raw[:used].view(dt).reshape((cam.height, cam.width) + tail)
        assert afx.same_bytes(got, host[name]) and afx.same_bytes(got, exp[name]), name
    # a band of two layers on the same stream; the others stay as they are
    for b in bufs.values():
        b.fill_(SENTINEL)
    torch.cuda.synchronize()
    rend.render_aov_device(cam, {"depth": bufs["depth"].data_ptr(), "index": bufs["index"].data_ptr(),
                                 "hit": 0}, row0=5, nrows=9, stream=st.cuda_stream)
    st.synchronize()
    n9 = 9 * cam.width
    for name in LAYERS:
        raw = bufs[name].cpu().numpy()
        if name in ("depth", "index"):
            assert afx.same_bytes(raw[:4 * n9].view(capi.AOV_LAYERS[name][0]).reshape(9, cam.width),
                                  exp[name][5:14]), name
            assert (raw[4 * n9:] == SENTINEL).all(), name
        else:
            assert (raw == SENTINEL).all(), name


def test_status_codes(rend):
    prims, cam, _ = afx.case("B13")
    lib = rend.lib
    npx = cam.width * cam.height
    idx, dep = guarded("index", npx), guarded("depth", npx)
    ok = capi.rt_aov_buffers(index=idx.ctypes.data, depth=dep.ctypes.data)
    none = capi.rt_aov_buffers()
    bad = capi.rt_aov_buffers(index=idx.ctypes.data, reserved=dep.ctypes.data)
    with capi.Renderer(0) as fresh:
        assert lib.rt_render_aov(fresh.ctx, C.byref(cam), 0, 1, C.byref(ok), None) == capi.RT_ERR_NO_SCENE
        assert lib.rt_render_aov_device(fresh.ctx, C.byref(cam), 0, 1, C.byref(ok),
                                        None) == capi.RT_ERR_NO_SCENE
    rend.set_scene(prims)
    for fn, last in ((lib.rt_render_aov, None), (lib.rt_render_aov_device, None)):
        assert fn(rend.ctx, C.byref(cam), 0, 1, C.byref(none), last) == capi.RT_ERR_INVALID_ARG
        assert fn(rend.ctx, C.byref(cam), 0, 1, C.byref(bad), last) == capi.RT_ERR_INVALID_ARG
        assert fn(rend.ctx, C.byref(cam), 0, 1, None, last) == capi.RT_ERR_INVALID_ARG
        assert fn(rend.ctx, None, 0, 1, C.byref(ok), last) == capi.RT_ERR_INVALID_ARG
        assert fn(None, C.byref(cam), 0, 1, C.byref(ok), last) == capi.RT_ERR_INVALID_ARG
    st = capi.rt_stats(ms=-1.0, segments=77)
    assert lib.rt_render_aov(rend.ctx, C.byref(cam), 0, 0, C.byref(ok), C.byref(st)) == capi.RT_OK
    assert st.segments == 0 and st.ms == 0.0
    assert untouched(idx) and untouched(dep)
    with pytest.raises(ValueError):
        rend.render_aov_device(cam, {"colour": 8})


# ---------------------------------------------------------------- 8. the beauty frame agrees
def test_misses_are_the_sky_pixels_of_the_frame(rend, oracle):
    """A at depth 0, F64, RT_OUT_RGB_F64: the pixels with index == -1 are exactly the pixels
    whose colour is the oracle's out_color(d).

    "Is" means: bit for bit where the ray points below the horizon (the ground colour is a
    constant), and within the F64 frames' bound of 1e-12 per channel above it — there
    out_color takes normalize(d).z to the power 1/4, which the kernels form as sqrt(sqrt(z))
    and the reference with pow(): the two roundings may differ in the last bits (DESIGN.md,
    "exactness"), and nothing else in a miss pixel is approximate.  Every hit pixel must differ
    from out_color(d) by more than that bound."""
    prims, cam, _ = afx.case("A")
    rend.set_scene(prims)
    img, _ = rend.render(cam, 0, capi.RT_PREC_F64, 0, capi.RT_OUT_RGB_F64)
    got, _ = rend.render_aov(cam, layers=("index",))
    _, d = sfx.camera_rays(cam)
    sky = np.array([oracle.out_color(v) for v in d]).reshape(cam.height, cam.width, 3)
    delta = np.abs(img - sky).max(axis=-1)
    miss = got["index"] == -1
    below = (d[:, 2] < 0).reshape(miss.shape)
    print("beauty vs aov: misses", int(miss.sum()), "bitwise-equal miss pixels",
          int((img[miss] == sky[miss]).all(axis=-1).sum()), "max delta on misses",
          float(delta[miss].max()), "min delta on hits", float(delta[~miss].min()))
    assert np.array_equal(delta <= 1e-12, miss)
    g = miss & below
    assert g.any() and (miss & ~below).any()
    assert img[g].tobytes() == sky[g].tobytes()
