"""GPU: ambient occlusion frames (rt_render_ao / rt_render_ao_device) against the expected
layers of tests/ao_fixture.py, on an MI355X (`pytest -m gpu`).  count is an integer and ao one
cast of an exact quotient, so every comparison is bytewise: no tolerance, no excluded pixel.
Frames are 48 x 32, 32 x 24, 24 x 16 or 13 x 8."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import ao_fixture as aofx
import aov_fixture as afx
import lights_fixture as lfx
from conftest import has_gpu
from rtamd import capi, scenes

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")]

LAYERS = ("count", "ao")
INT32_MAX = 2**31 - 1
DEFAULTS = {capi.RT_OPT_WAVE_CULL_MIN_SPHERES: 24, capi.RT_OPT_TILE_BINS: 1,
            capi.RT_OPT_EYE_TABLES: 1, capi.RT_OPT_WALL_ORDER: 0, capi.RT_OPT_CLUSTER_COS: 400,
            capi.RT_OPT_SUPERSAMPLE: 1}
OPTION_SETS = {   # test_aov_gpu.py's nine
    "tile_bins_off": {capi.RT_OPT_TILE_BINS: 0},
    "eye_tables_off": {capi.RT_OPT_EYE_TABLES: 0},
    "wall_order_on": {capi.RT_OPT_WALL_ORDER: 1},
    "wave_cull_all": {capi.RT_OPT_WAVE_CULL_MIN_SPHERES: 0},
    "wave_cull_never": {capi.RT_OPT_WAVE_CULL_MIN_SPHERES: INT32_MAX},
    "clusters_never": {capi.RT_OPT_CLUSTER_COS: -2000},
    "clusters_always": {capi.RT_OPT_CLUSTER_COS: 2000},
    "cull_all_clusters_always": {capi.RT_OPT_WAVE_CULL_MIN_SPHERES: 0, capi.RT_OPT_CLUSTER_COS: 2000},
    "cull_all_clusters_never": {capi.RT_OPT_WAVE_CULL_MIN_SPHERES: 0, capi.RT_OPT_CLUSTER_COS: -2000},
}
GUARD = 16       # sentinel elements behind every buffer
SENTINEL = 0xAB
SHORT, FAR = aofx.RADII
_dp = C.POINTER(C.c_double)


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
    buf = np.empty(npx + GUARD, capi.AO_LAYERS[name])
    buf.view(np.uint8)[...] = SENTINEL
    return buf


def untouched(buf, first=0):
    return bool((np.ascontiguousarray(buf[first:]).view(np.uint8) == SENTINEL).all())


def params(dirs, radius, ndirs=None, reserved=0, reserved2=None):
    """(rt_ao_params, the array it points into)."""
    w = np.ascontiguousarray(dirs, np.float64).reshape(-1, 3)
    return capi.rt_ao_params(w.ctypes.data_as(_dp), len(w) if ndirs is None else ndirs, reserved,
                             float(radius), reserved2), w


def ao_guarded(rend, cam, dirs, radius, layers=LAYERS, row0=0, nrows=None):
    """rt_render_ao into guarded buffers for both layers; only `layers` are passed.  Returns the
    requested ones as [nrows, W] after checking that nothing behind them, and nothing of a buffer
    not passed, was written."""
    nrows = cam.height - row0 if nrows is None else nrows
    npx = nrows * cam.width
    bufs = {name: guarded(name, npx) for name in LAYERS}
    arg = capi.rt_ao_buffers(**{name: bufs[name].ctypes.data for name in layers})
    prm, keep = params(dirs, radius)
    st = capi.rt_stats()
    capi.check(rend.lib.rt_render_ao(rend.ctx, C.byref(cam), row0, nrows, C.byref(prm), C.byref(arg),
                                     C.byref(st)), rend.ctx)
    assert st.segments == npx and st.ms > 0
    out = {}
    for name in LAYERS:
        if name in layers:
            assert untouched(bufs[name], npx), name
            out[name] = bufs[name][:npx].reshape(nrows, cam.width)
        else:
            assert untouched(bufs[name]), name
    return out


def assert_layers(got, exp, rows=slice(None), what=""):
    for name in got:
        assert afx.same_bytes(got[name], exp[name][rows]), (what, name)


# ---------------------------------------------------------------- 1. the layers
@pytest.mark.parametrize("name,k", aofx.GPU_CASES)
def test_layers_match_fixture(rend, name, k):
    e = aofx.case(name, k)
    rend.set_scene(e.prims)
    idx = rend.render_aov(e.cam, layers=("index",))[0]["index"]
    assert np.array_equal(idx >= 0, e.hitmask)
    for radius in aofx.RADII:
        got, st = rend.render_ao(e.cam, ndirs=k, radius=radius)
        assert set(got) == set(LAYERS) and st.segments == e.cam.width * e.cam.height
        assert got["count"].dtype == np.uint8 and got["ao"].dtype == np.float32
        assert got["count"].shape == got["ao"].shape == (e.cam.height, e.cam.width)
        exp = e.layers(radius)
        assert_layers(got, exp, what=(name, radius))
        assert not got["count"][idx == -1].any()
        assert got["ao"][idx == -1].tobytes() == np.ones(int((idx == -1).sum()), np.float32).tobytes()
        assert afx.same_bytes(got["ao"], aofx.ao_of(got["count"], k))


def test_empty_scene_all_open(rend):
    _, cam, _ = afx.case("B13")
    rend.set_scene([])
    got = ao_guarded(rend, cam, capi.ao_directions(16), SHORT)
    assert not got["count"].any() and (got["ao"].view(np.uint32) == 0x3F800000).all()


# ---------------------------------------------------------------- 2. composition on the device
def test_count_is_the_sum_of_occlusion_queries(rend):
    """Case A, seeded directions with lengths in [0.25, 4]: count equals the sum over k of
    rt_occluded(sp, +-w_k, radius), with sp and the flips built in numpy from rt_render_aov's
    records — so the radius is a parameter along the probe, not a world distance."""
    prims, cam, _ = afx.case("A")
    dirs = aofx.random_dirs(16, seed=5)
    assert np.linalg.norm(dirs, axis=1).min() < 0.8 and np.linalg.norm(dirs, axis=1).max() > 2.0
    rend.set_scene(prims)
    hits = rend.render_aov(cam, layers=("hit",))[0]["hit"].reshape(-1)
    hm = hits["index"] >= 0
    o, d = afx.sfx.camera_rays(cam)
    P, n = aofx.surface(prims, hits[hm], o[hm], d[hm])
    sp, w, _, _ = aofx.probes(P, n, d[hm], dirs)
    e = aofx.build(prims, cam, dirs)
    for radius in aofx.RADII:
        total = np.zeros(int(hm.sum()), np.int64)
        for k in range(len(dirs)):
            mask, _, _ = rend.occluded(sp, w[:, k, :], radius)
            total += mask
        got = rend.render_ao(cam, dirs=dirs, radius=radius, layers=("count",))[0]["count"]
        assert np.array_equal(got.reshape(-1)[hm], total) and not got.reshape(-1)[~hm].any()
        assert afx.same_bytes(got, e.count(radius))
    # as a world distance the short radius would give another answer somewhere
    unit = dirs / np.linalg.norm(dirs, axis=1)[:, None]
    assert not np.array_equal(aofx.build(prims, cam, unit).count(SHORT), e.count(SHORT))


# ---------------------------------------------------------------- 3. flip and order rules
@pytest.mark.parametrize("name", ["A", "L", "views"])
def test_negated_and_permuted_directions(rend, name):
    e = aofx.case(name, 16)
    rend.set_scene(e.prims)
    ok = ~e.degenerate
    assert ok[e.hitmask].sum() > 100
    perm = np.random.default_rng(3).permutation(16)
    neg = aofx.build(e.prims, e.cam, -e.dirs)
    for radius in aofx.RADII:
        a = rend.render_ao(e.cam, dirs=e.dirs, radius=radius)[0]
        b = rend.render_ao(e.cam, dirs=-e.dirs, radius=radius)[0]
        c = rend.render_ao(e.cam, dirs=e.dirs[perm], radius=radius)[0]
        assert np.array_equal(a["count"][ok], b["count"][ok])
        assert a["ao"][ok].tobytes() == b["ao"][ok].tobytes()
        assert_layers(c, a, what="permutation")
        assert_layers(b, neg.layers(radius), what="negated")


def hand_scene():
    """An axis-aligned wall (normal (0, -1, 0)) seen from its front, and a sphere above it on the
    +z side only: an in-plane probe (0, 0, 1) has s == 0 exactly."""
    S = scenes
    return S.to_prims([S.Wall(S.Material((.5, .5, .5)), (7, 2, -3), (0, -1, 0), 6, 6),
                       S.Sphere(S.Material((1, 0, 0)), (3.5, 1.5, 2.5), 1.0)])


def test_zero_dot_is_not_flipped(rend):
    prims = hand_scene()
    cam = capi.camera_init(**scenes.camera_args(24, 16))
    rend.set_scene(prims)
    up, down = np.array([[0.0, 0.0, 1.0]]), np.array([[0.0, 0.0, -1.0]])
    eu, ed = aofx.build(prims, cam, up), aofx.build(prims, cam, down)
    wall = eu.aov["kind"] == 1
    assert wall.sum() > 100 and (eu.s[eu.aov["kind"][eu.hitmask] == 1] == 0).all()
    gu = rend.render_ao(cam, dirs=up, radius=np.inf, layers=("count",))[0]["count"]
    gd = rend.render_ao(cam, dirs=down, radius=np.inf, layers=("count",))[0]["count"]
    assert afx.same_bytes(gu, eu.count(np.inf)) and afx.same_bytes(gd, ed.count(np.inf))
    # the blocker lies on the +z side only: flipping either direction would swap the answers
    assert gu[wall].sum() > 10 and not gd[wall].any()


def cancelling_scene():
    """24 x 8 (three tiles): a small sphere that covers exactly the two centre pixels of the
    middle tile's row 3, and a large sphere on either side of it along y, seen only in the outer
    tiles.  With the one direction (0, 1, 0) the two hit lanes of the middle tile probe along +y
    and -y: their unit directions cancel exactly, and each probe has a blocker."""
    S = scenes
    cam = capi.camera_init(**scenes.camera_args(24, 8))
    _, d = afx.sfx.camera_rays(cam)
    d = d.reshape(8, 24, 3)
    p1 = d[3, 11] / np.linalg.norm(d[3, 11]) * 5.0
    p2 = d[3, 12] / np.linalg.norm(d[3, 12]) * 5.0
    ctr, sep = (p1 + p2) / 2, float(np.linalg.norm(p2 - p1))
    w = np.array([0.0, 1.0, 0.0])
    prims = S.to_prims([S.Sphere(S.Material((1, 0, 0)), ctr, 0.6 * sep),
                        S.Sphere(S.Material((0, 1, 0)), ctr + w * 8 * sep, 2 * sep),
                        S.Sphere(S.Material((0, 0, 1)), ctr - w * 8 * sep, 2 * sep)])
    return prims, cam, w[None, :]


@pytest.mark.parametrize("optset", ["wave_cull_all", "cull_all_clusters_never", "cull_all_clusters_always"])
def test_probes_that_cancel_in_the_wave_cone(rend, optset):
    """The cull kernel's cone over a wave whose only live probes are w and -w: the sum of their
    unit directions is exactly zero.  Both probes are blocked."""
    prims, cam, dirs = cancelling_scene()
    e = aofx.build(prims, cam, dirs)
    mid = np.zeros(e.hitmask.shape, bool)
    mid[:, 8:16] = True
    assert int((e.hitmask & mid).sum()) == 2 and (e.aov["index"][e.hitmask & mid] == 0).all()
    s_mid = e.s[:, 0][(e.aov["index"][e.hitmask] == 0)]
    assert len(s_mid) == 2 and s_mid[0] * s_mid[1] < 0
    assert (e.count(np.inf)[e.hitmask & mid] == 1).all()
    rend.set_scene(prims)
    with options(rend, OPTION_SETS[optset]):
        for radius in (np.inf, 12.0):
            got = rend.render_ao(cam, dirs=dirs, radius=radius)[0]
            assert_layers(got, e.layers(radius), what=(optset, radius))
    assert (e.count(12.0)[e.hitmask & mid] == 1).all()


def test_count_grows_with_the_radius(rend):
    e = aofx.case("A", 16)
    rend.set_scene(e.prims)
    prev = np.zeros(e.hitmask.shape, np.uint8)
    for radius in (0.1, 0.75, SHORT, 3.0, 10.0, FAR):
        got = rend.render_ao(e.cam, dirs=e.dirs, radius=radius, layers=("count",))[0]["count"]
        assert (got >= prev).all()
        assert afx.same_bytes(got, e.count(radius))
        prev = got
    assert prev.max() > 4


def test_one_direction_and_sixty_four(rend):
    e64 = aofx.case("B13", 64)
    rend.set_scene(e64.prims)
    kbest = int(e64.blocked(FAR).sum(axis=0).argmax())   # the direction with the most blockers
    one = e64.dirs[kbest:kbest + 1]
    e1 = aofx.build(e64.prims, e64.cam, one)
    for radius in aofx.RADII:
        got = ao_guarded(rend, e64.cam, one, radius)
        assert_layers(got, e1.layers(radius), what="K = 1")
        assert set(np.unique(got["ao"])) <= {0.0, 1.0}
        assert_layers(ao_guarded(rend, e64.cam, e64.dirs, radius), e64.layers(radius), what="K = 64")
    assert e1.count(FAR).any() and e64.count(FAR).max() > 16


# ---------------------------------------------------------------- 4. mirrored from the AOVs
@pytest.mark.parametrize("name,k", [("B13", 64), ("L", 16)])
def test_each_layer_alone_and_guards(rend, name, k):
    e = aofx.case(name, k)
    rend.set_scene(e.prims)
    exp = e.layers(SHORT)
    assert_layers(ao_guarded(rend, e.cam, e.dirs, SHORT), exp, what="both")
    for layer in LAYERS:
        assert_layers(ao_guarded(rend, e.cam, e.dirs, SHORT, (layer,)), exp, what=layer)


@pytest.mark.parametrize("name", ["A", "L"])
def test_bands_equal_frame_slices(rend, name):
    e = aofx.case(name, 16)
    rend.set_scene(e.prims)
    exp = e.layers(SHORT)
    for row0, nrows in ((3, 18), (17, 1), (0, 1), (e.cam.height - 1, 1)):
        got = ao_guarded(rend, e.cam, e.dirs, SHORT, LAYERS, row0, nrows)
        assert_layers(got, exp, slice(row0, row0 + nrows), what=(row0, nrows))


def test_band_statuses_are_rt_renders(rend):
    e = aofx.case("A", 16)
    cam = e.cam
    rend.set_scene(e.prims)
    H, npx = cam.height, cam.width * cam.height
    cnt = guarded("count", npx)
    arg = capi.rt_ao_buffers(count=cnt.ctypes.data)
    prm, keep = params(e.dirs, SHORT)
    img = np.empty((H + 1, cam.width, 3), np.float32)
    seen = set()
    for row0, nrows in ((-1, 4), (H - 2, 4), (0, H + 1), (H, 1), (0, -1), (-1, -1), (H, 0), (H + 1, 0),
                        (0, 0)):
        a = rend.lib.rt_render_ao(rend.ctx, C.byref(cam), row0, nrows, C.byref(prm), C.byref(arg), None)
        b = rend.lib.rt_render_ao_device(rend.ctx, C.byref(cam), row0, nrows, C.byref(prm), C.byref(arg),
                                         None)
        r = rend.lib.rt_render(rend.ctx, C.byref(cam), row0, nrows, 0, capi.RT_PREC_F64, 0,
                               capi.RT_OUT_RGB_F32, img.ctypes.data_as(C.c_void_p), 0, None)
        assert a == r and b == r, (row0, nrows, a, b, r)
        seen.add(r)
    assert untouched(cnt)
    assert {capi.RT_OK, capi.RT_ERR_INVALID_ARG, capi.RT_ERR_OUT_OF_RANGE} <= seen


@pytest.mark.parametrize("name", ["A", "L"])
@pytest.mark.parametrize("optset", list(OPTION_SETS))
def test_option_invariance(rend, name, optset):
    e = aofx.case(name, 16)
    rend.set_scene(e.prims)
    with options(rend, OPTION_SETS[optset]):
        near = rend.render_ao(e.cam, dirs=e.dirs, radius=SHORT)[0]
        far = rend.render_ao(e.cam, dirs=e.dirs, radius=FAR, layers=("count",))[0]
    assert_layers(near, e.layers(SHORT), what=(name, optset, SHORT))
    assert_layers(far, e.layers(FAR), what=(name, optset, FAR))


def test_frames_and_feedback_undisturbed():
    """RT_OPT_ROW_FEEDBACK at its default: render, AO, render gives two identical colour frames
    (segment counts included), and the AO between them is a fresh ctx's."""
    e = aofx.case("A", 16)
    prims, cam = e.prims, e.cam
    with capi.Renderer(0) as r:
        r.set_scene(prims)
        a, sa = r.render(cam, 3, capi.RT_PREC_PATH64, 0, capi.RT_OUT_RGB_F32, count_segments=True)
        got, _ = r.render_ao(cam, dirs=e.dirs, radius=SHORT)
        b, sb = r.render(cam, 3, capi.RT_PREC_PATH64, 0, capi.RT_OUT_RGB_F32, count_segments=True)
        assert afx.same_bytes(a, b) and sa.segments == sb.segments
        c, _ = r.render(cam, 3, capi.RT_PREC_F64, 0, capi.RT_OUT_RGB_F64, row0=8, nrows=16)
        band, _ = r.render_ao(cam, dirs=e.dirs, radius=SHORT, row0=3, nrows=18)
        f, _ = r.render(cam, 3, capi.RT_PREC_F64, 0, capi.RT_OUT_RGB_F64, row0=8, nrows=16)
        assert afx.same_bytes(c, f)
        assert_layers(band, e.layers(SHORT), slice(3, 21), what="band")
    with capi.Renderer(0) as fresh:
        fresh.set_scene(prims)
        alone, _ = fresh.render_ao(cam, dirs=e.dirs, radius=SHORT)
    assert_layers(got, alone, what="fresh")
    assert_layers(got, e.layers(SHORT), what="fixture")


def test_lights_and_supersample_ignored(rend):
    e = aofx.case("A", 16)
    rend.set_scene(e.prims)
    try:
        rend.set_lights(lfx.K4)
        rend.set_option(capi.RT_OPT_SUPERSAMPLE, 2)
        got, st = rend.render_ao(e.cam, dirs=e.dirs, radius=SHORT)
    finally:
        rend.set_lights(None)
        rend.set_option(capi.RT_OPT_SUPERSAMPLE, 1)
    assert st.segments == e.cam.width * e.cam.height
    assert got["count"].shape == (e.cam.height, e.cam.width)
    assert_layers(got, e.layers(SHORT), what="lights + S = 2")


# ---------------------------------------------------------------- 5. device variant
def test_device_variant_keeps_each_launch_its_directions(rend):
    """Two launches with different direction sets back to back on a non-default stream, no sync
    between them, the host arrays overwritten as soon as each call has returned."""
    import torch
    e = aofx.case("L", 16)
    cam = e.cam
    other = aofx.random_dirs(9, seed=11)
    e2 = aofx.build(e.prims, cam, other)
    rend.set_scene(e.prims)
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(dev)
    npx = cam.width * cam.height
    size = {"count": 1, "ao": 4}
    bufs = [{name: torch.full(((npx + GUARD) * size[name],), SENTINEL, dtype=torch.uint8, device=dev)
             for name in LAYERS} for _ in range(2)]
    torch.cuda.synchronize()
    for b, dirs, radius in ((bufs[0], e.dirs, SHORT), (bufs[1], other, FAR)):
        scratch = np.array(dirs, np.float64, copy=True)
        prm, keep = params(scratch, radius)
        arg = capi.rt_ao_buffers(count=b["count"].data_ptr(), ao=b["ao"].data_ptr())
        capi.check(rend.lib.rt_render_ao_device(rend.ctx, C.byref(cam), 0, cam.height, C.byref(prm),
                                                C.byref(arg), C.c_void_p(st.cuda_stream)), rend.ctx)
        scratch[...] = np.nan      # consumed: the launch already carries its directions
        prm.ndirs, prm.radius = 1, -1.0
    st.synchronize()
    for b, exp in ((bufs[0], e.layers(SHORT)), (bufs[1], e2.layers(FAR))):
        for name in LAYERS:
            raw = b[name].cpu().numpy()
            used = npx * size[name]
            assert (raw[used:] == SENTINEL).all(), name
            got = raw[:used].view(capi.AO_LAYERS[name]).reshape(cam.height, cam.width)
            assert afx.same_bytes(got, exp[name]), name
    # a band of one layer through the binding; the other buffer stays as it is
    for t in bufs[0].values():
        t.fill_(SENTINEL)
    torch.cuda.synchronize()
    rend.render_ao_device(cam, e.dirs, SHORT, {"count": bufs[0]["count"].data_ptr(), "ao": 0},
                          row0=5, nrows=9, stream=st.cuda_stream)
    st.synchronize()
    raw = bufs[0]["count"].cpu().numpy()
    n9 = 9 * cam.width
    assert afx.same_bytes(raw[:n9].reshape(9, cam.width), e.count(SHORT)[5:14])
    assert (raw[n9:] == SENTINEL).all() and (bufs[0]["ao"].cpu().numpy() == SENTINEL).all()
    with pytest.raises(ValueError):
        rend.render_ao_device(cam, e.dirs, SHORT, {"depth": 8})


# ---------------------------------------------------------------- 6. statuses
def test_status_codes(rend):
    _, cam, _ = afx.case("B13")
    prims = afx.case("B13")[0]
    lib = rend.lib
    npx = cam.width * cam.height
    cnt, ao = guarded("count", npx), guarded("ao", npx)
    ok = capi.rt_ao_buffers(count=cnt.ctypes.data, ao=ao.ctypes.data)
    none = capi.rt_ao_buffers()
    badbuf = capi.rt_ao_buffers(count=cnt.ctypes.data, reserved=ao.ctypes.data)
    dirs = capi.ao_directions(8)
    good, keep = params(dirs, 1.0)

    def both(ctx, cam_p, prm_p, buf_p):
        a = lib.rt_render_ao(ctx, cam_p, 0, 1, prm_p, buf_p, None)
        b = lib.rt_render_ao_device(ctx, cam_p, 0, 1, prm_p, buf_p, None)
        assert a == b, (a, b)
        return a

    with capi.Renderer(0) as fresh:
        assert both(fresh.ctx, C.byref(cam), C.byref(good), C.byref(ok)) == capi.RT_ERR_NO_SCENE
    rend.set_scene(prims)
    bad = capi.RT_ERR_INVALID_ARG
    assert both(rend.ctx, C.byref(cam), C.byref(good), C.byref(none)) == bad
    assert both(rend.ctx, C.byref(cam), C.byref(good), C.byref(badbuf)) == bad
    assert both(rend.ctx, C.byref(cam), C.byref(good), None) == bad
    assert both(rend.ctx, C.byref(cam), None, C.byref(ok)) == bad
    assert both(rend.ctx, None, C.byref(good), C.byref(ok)) == bad
    assert both(None, C.byref(cam), C.byref(good), C.byref(ok)) == bad
    keepalive = []
    variants = [params(dirs, 1.0, reserved=1), params(dirs, 1.0, reserved2=cnt.ctypes.data),
                params(dirs, 1.0, ndirs=0), params(dirs, 1.0, ndirs=-1),
                params(np.ones((65, 3)), 1.0), params(dirs, np.nan), params(dirs, 0.0),
                params(dirs, -1.0), params(dirs, -np.inf)]
    for comp, val in ((0, np.nan), (1, np.inf), (2, -np.inf)):
        w = dirs.copy()
        w[3, comp] = val
        variants.append(params(w, 1.0))
    w = dirs.copy()
    w[7] = (0.0, -0.0, 0.0)
    variants.append(params(w, 1.0))
    nulldirs = capi.rt_ao_params(None, 8, 0, 1.0, None)
    variants.append((nulldirs, None))
    for prm, arr in variants:
        keepalive.append(arr)
        assert both(rend.ctx, C.byref(cam), C.byref(prm), C.byref(ok)) == bad, (prm.ndirs, prm.radius)
    st = capi.rt_stats(ms=-1.0, segments=77)
    assert lib.rt_render_ao(rend.ctx, C.byref(cam), 0, 0, C.byref(good), C.byref(ok), C.byref(st)) == capi.RT_OK
    assert st.segments == 0 and st.ms == 0.0
    assert lib.rt_render_ao_device(rend.ctx, C.byref(cam), 0, 0, C.byref(good), C.byref(ok), None) == capi.RT_OK
    assert untouched(cnt) and untouched(ao)
    # +inf is a valid radius, 64 a valid count
    got = ao_guarded(rend, cam, np.ones((64, 3)), np.inf)
    assert got["count"].max() <= 64
