"""GPU: tilted walls, rolled and z-looking cameras and non-default materials against the
reference's own numbers (tests/golden/views.npz), on an MI355X (`pytest -m gpu`).

Every comparison is with the fixture, or with the oracle that test_views_host.py pins to it
bitwise; nothing here compares one kernel variant with another.  All fixture frames are at most
48 x 48.

Bounds
  F64     |delta| <= 1e-12 * max(1, max|ref|) per channel, every pixel: the project's F64 bound
          (the geometry is bit-exact, only pow's last bit differs), scaled because tilt_wild's
          extrapolating materials reach values of several units.
  MIXED   bytewise F64.
  PATH64  <= 1e-4 per channel (north_star) on the bounded scenes; how many pixels exceed
          PATH64_TOL = 2e-5 is reported, not gated (that bound was measured with default
          materials only).  tilt_wild (metallic 1.5, colour 2, exponent 1025, ...): the same
          ray paths, finite output, delta reported.
  F32     test_gpu_parity.py's check_f32 unchanged: >= 99.5% of pixels within 1e-4 at depth 4,
          every outlier on the oracle's discontinuity mask.
Measured values are in DESIGN.md ("views fixture").
"""
import contextlib
import json
import os

import numpy as np
import pytest

from conftest import has_gpu
from rtamd import capi
from test_gpu_parity import check_f32, check_f64, discontinuity_mask
from test_rays_gpu import orc_trace
from test_supersample_gpu import tree_mean
from views_fixture import Views, int_exp, same_bytes

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")]

F64_TOL = 1e-12
PATH64_BOUND = 1e-4
PATH64_TOL = 2e-5
F64, F32, MIXED, PATH64 = (capi.RT_PREC_F64, capi.RT_PREC_F32, capi.RT_PREC_MIXED,
                           capi.RT_PREC_PATH64)
O64 = capi.RT_OUT_RGB_F64
NTHREADS = min(16, len(os.sched_getaffinity(0)))
BOUNDED = ("tilt", "tilt_mat", "cloud")

DEFAULTS = {capi.RT_OPT_WAVE_CULL_MIN_SPHERES: 24, capi.RT_OPT_TILE_BINS: 1,
            capi.RT_OPT_MIRROR_BINS: 1, capi.RT_OPT_EYE_TABLES: 1, capi.RT_OPT_WALL_ORDER: 0,
            capi.RT_OPT_CLUSTER_COS: 400, capi.RT_OPT_PIXEL_PAIRS: 0, capi.RT_OPT_SUPERSAMPLE: 1}
OPTION_SETS = {
    "defaults": {},
    "tile_bins_off": {capi.RT_OPT_TILE_BINS: 0},
    "mirror_bins_off": {capi.RT_OPT_MIRROR_BINS: 0, capi.RT_OPT_TILE_BINS: 1},
    "eye_tables_off": {capi.RT_OPT_EYE_TABLES: 0},
    "wall_order_on": {capi.RT_OPT_WALL_ORDER: 1},
    # the small scenes on the cull kernels, wall cone included
    "wave_cull_all": {capi.RT_OPT_WAVE_CULL_MIN_SPHERES: 0},
    "clusters_always": {capi.RT_OPT_CLUSTER_COS: 2000, capi.RT_OPT_WAVE_CULL_MIN_SPHERES: 0},
    "clusters_never": {capi.RT_OPT_CLUSTER_COS: -2000, capi.RT_OPT_WAVE_CULL_MIN_SPHERES: 0},
}


@pytest.fixture(scope="module")
def views():
    return Views()


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


_scene_on = {}


def use_scene(rend, views, name):
    if _scene_on.get(id(rend)) != name:
        rend.set_scene(views.prims(name))
        _scene_on[id(rend)] = name


@pytest.fixture(scope="module")
def expected(views, oracle):
    """Per fixture frame: the oracle's segment count at the frame's depth and the scene index
    its primary segment hits (-1 = miss); computed once, read only."""
    out = {}
    for key, scene, view, depth in views.frames:
        cam = views.camera(view)
        _, _, segs = oracle.render(views.prims(scene), cam, depth, want64=False)
        _, _, _, sig0 = oracle.render(views.prims(scene), cam, 0, want64=False, want_sig=True)
        out[key] = dict(segs=segs, primary=sig0.astype(np.int64) - 1)
    return out


def report(tag, rep):
    print(tag, json.dumps(rep))
    out = os.environ.get("RT_PARITY_REPORT")
    if out:
        with open(out, "a") as fh:
            fh.write(json.dumps(rep) + "\n")


# ---------------------------------------------------------------- exercise guards
def test_fixture_reaches_tilted_walls_and_general_pow(views, expected):
    """What the tests below render is the ground they are for: in every scene the primary hit of
    more than 100 fixture pixels is a wall whose normal has a z component and the closest hit of
    more than 20 fixture rays is one (the reference's hit indices); tilt_wild selects the
    general-pow kernels, and more than 100 pixels and 20 rays hit a primitive whose exponent is
    not an integer in [0, 1024]."""
    for scene in views.scene_names:
        zw = views.z_walls(scene)
        px = sum(int(np.isin(expected[k]["primary"], zw).sum())
                 for k, s, _, _ in views.frames if s == scene)
        rays = int(np.isin(views.rays(scene)["hits"]["index"], zw).sum())
        assert px > 100 and rays > 20, (scene, px, rays)
    prims = views.prims("tilt_wild")
    assert not int_exp(prims)
    assert all(int_exp(views.prims(s)) for s in BOUNDED)
    odd = [j for j, p in enumerate(prims) if not int_exp([p])]
    px = sum(int(np.isin(expected[k]["primary"], odd).sum())
             for k, s, _, _ in views.frames if s == "tilt_wild")
    rays = int(np.isin(views.rays("tilt_wild")["hits"]["index"], odd).sum())
    assert px > 100 and rays > 20, (px, rays)


# ---------------------------------------------------------------- frames, F64 and MIXED
@pytest.mark.parametrize("optset", list(OPTION_SETS))
def test_frames_f64_and_mixed_match_reference(rend, views, expected, optset):
    with options(rend, OPTION_SETS[optset]):
        for key, scene, view, depth in views.frames:
            use_scene(rend, views, scene)
            cam, ref = views.camera(view), views.z[key]
            img, st = rend.render(cam, depth, F64, 0, O64, count_segments=True)
            assert img.shape == ref.shape
            d = float(np.abs(img - ref).max())
            assert d <= F64_TOL * max(1.0, float(np.abs(ref).max())), (optset, key, d)
            assert st.segments == expected[key]["segs"], (optset, key)
            mix, sm = rend.render(cam, depth, MIXED, 0, O64, count_segments=True)
            assert same_bytes(mix, img) and sm.segments == st.segments, (optset, key)


# ---------------------------------------------------------------- frames, PATH64
@pytest.mark.parametrize("pairs", [0, 1])
def test_frames_path64(rend, views, expected, pairs):
    worst = {}
    with options(rend, {capi.RT_OPT_PIXEL_PAIRS: pairs}):
        for key, scene, view, depth in views.frames:
            use_scene(rend, views, scene)
            ref = views.z[key]
            img, st = rend.render(views.camera(view), depth, PATH64, 0, O64, count_segments=True)
            assert st.segments == expected[key]["segs"], (pairs, key)
            assert np.isfinite(img[np.isfinite(ref)]).all(), (pairs, key)
            d = np.abs(img - ref).max(axis=-1)
            w = worst.setdefault(scene, {"pixels": 0, "max_abs_delta": 0.0, "above_2e-5": 0,
                                         "max_ref": 0.0})
            w["pixels"] += int(d.size)
            w["max_abs_delta"] = max(w["max_abs_delta"], float(d.max()))
            w["above_2e-5"] += int((d > PATH64_TOL).sum())
            w["max_ref"] = max(w["max_ref"], float(np.abs(ref).max()))
            if scene in BOUNDED:
                assert d.max() <= PATH64_BOUND, (pairs, key, float(d.max()))
    report("views_vs_oracle", {"what": "path64_frames", "pixel_pairs": pairs, "scenes": worst})


# ---------------------------------------------------------------- frames at 192 pixels wide
F32_DEPTH = 4
_wide = {}


def wide_oracle(views, oracle, scene, view):
    """The oracle's depth-4 render of a fixture view at 192 pixels wide -> (camera, frame,
    segments, signatures); computed once per (scene, view), read only."""
    if (scene, view) not in _wide:
        cam = views.camera(view, width=192)
        o64, _, segs, sig = oracle.render(views.prims(scene), cam, F32_DEPTH, nthreads=NTHREADS,
                                          want_sig=True)
        o64.setflags(write=False)
        _wide[(scene, view)] = (cam, o64, segs, sig)
    return _wide[(scene, view)]


@pytest.mark.parametrize("scene", ["tilt", "tilt_mat"])
def test_frames_f32_discontinuity_rule(rend, views, oracle, scene):
    """Every view of tilt re-rendered 192 pixels wide at depth 4, against the oracle rendered
    here: check_f32's rule as it stands (>= 99.5% of pixels within 1e-4, every outlier on the
    oracle's discontinuity mask).  No view had to be replaced; the measured shares are in
    DESIGN.md."""
    shares, failures = {}, []
    use_scene(rend, views, scene)
    for view in views.views_of("tilt"):
        cam, o64, _, sig = wide_oracle(views, oracle, scene, view)
        img, _ = rend.render(cam, F32_DEPTH, F32, 0, capi.RT_OUT_RGB_F32)
        bad = np.abs(img.astype(np.float64) - o64).max(axis=-1) > 1e-4
        shares[view] = {"size": [cam.width, cam.height], "within_1e-4": float(1.0 - bad.mean()),
                        "outliers_off_discontinuity": int((bad & ~discontinuity_mask(sig)).sum())}
        try:
            check_f32(img, o64, sig, F32_DEPTH, (scene, view))
        except AssertionError as e:     # every view is measured and reported before the verdict
            failures.append(str(e))
    report("views_vs_oracle", {"what": "f32_frames", "scene": scene, "views": shares})
    assert not failures, failures


@pytest.mark.parametrize("scene", ["tilt", "tilt_mat"])
def test_frames_f64_and_mixed_at_192_wide(rend, views, oracle, scene):
    """The same 192-wide renders in F64 and MIXED: some 200 000 rays per scene graze the tilted
    rectangles' edges far more closely than the 48-pixel fixture frames do, which is where a
    rounding slip of the exact bounds test or too tight a margin of MIXED's fp32 wall cull would
    show.  F64: every pixel within 1e-12 of the oracle, the same segment count.  MIXED: bytewise
    F64."""
    use_scene(rend, views, scene)
    for view in views.views_of("tilt"):
        cam, o64, segs, _ = wide_oracle(views, oracle, scene, view)
        img, st = rend.render(cam, F32_DEPTH, F64, 0, O64, count_segments=True)
        d = float(np.abs(img - o64).max())
        assert d <= F64_TOL * max(1.0, float(np.abs(o64).max())), (scene, view, d)
        assert st.segments == segs, (scene, view)
        mix, sm = rend.render(cam, F32_DEPTH, MIXED, 0, O64, count_segments=True)
        assert same_bytes(mix, img) and sm.segments == segs, (scene, view)


# ---------------------------------------------------------------- supersample
@pytest.mark.parametrize("view", ["rolled", "down"])
def test_supersample_s2(rend, views, oracle, view):
    """RT_OPT_SUPERSAMPLE 2 on tilt: bytewise tree_mean of the plain render of
    rt_supersample_camera(cam, 2) (the contract), and for F64 within 1e-12 of tree_mean of the
    oracle's frame, a pixel above it only with a sample on the oracle's discontinuity mask
    (test_supersample_gpu.py test_f64_against_the_oracle's rule)."""
    s, depth = 2, 5
    use_scene(rend, views, "tilt")
    cam = views.camera(view)
    vcam = capi.supersample_camera(cam, s)
    for prec in (F64, PATH64):
        plain, _ = rend.render(vcam, depth, prec, 0, O64)
        with options(rend, {capi.RT_OPT_SUPERSAMPLE: s}):
            got, _ = rend.render(cam, depth, prec, 0, O64)
        assert same_bytes(got, tree_mean(plain, s)), (view, prec)
        if prec == F64:
            o64, _, _, sig = oracle.render(views.prims("tilt"), vcam, depth, want_sig=True)
            mask = discontinuity_mask(sig).reshape(cam.height, s, cam.width, s).any(axis=(1, 3))
            check_f64(got, tree_mean(o64, s), mask, what=("S=2", view))


# ---------------------------------------------------------------- ray batches
@pytest.mark.parametrize("cull_min", [24, 0])
@pytest.mark.parametrize("scene", ["tilt", "tilt_mat", "tilt_wild", "cloud"])
def test_ray_batches_match_reference(rend, views, oracle, scene, cull_min):
    prims, r = views.prims(scene), views.rays(scene)
    o, d, depth, ref = r["o"], r["d"], r["depth"], r["rgb"]
    _, osegs = orc_trace(oracle, prims, o, d, depth)
    tol = F64_TOL * max(1.0, float(np.abs(ref).max()))
    use_scene(rend, views, scene)
    p64 = np.zeros(len(o))
    with options(rend, {capi.RT_OPT_WAVE_CULL_MIN_SPHERES: cull_min}):
        for dep in range(9):
            m = depth == dep
            a, _, st = rend.trace_rays(o[m], d[m], dep, F64, count_segments=True)
            dlt = float(np.abs(a - ref[m]).max())
            assert dlt <= tol, (scene, cull_min, dep, dlt)
            assert st.segments == int(osegs[m].sum()), (scene, cull_min, dep)
            b, _, _ = rend.trace_rays(o[m], d[m], dep, MIXED)
            assert same_bytes(a, b), (scene, cull_min, dep)
            p, _, sp = rend.trace_rays(o[m], d[m], dep, PATH64, count_segments=True)
            assert sp.segments == int(osegs[m].sum()), (scene, cull_min, dep)
            assert np.isfinite(p[np.isfinite(ref[m])]).all(), (scene, cull_min, dep)
            p64[m] = np.abs(p - ref[m]).max(axis=-1)
        for prec in (F64, PATH64):
            _, hits, st = rend.trace_rays(o, d, 3, prec, want_rgb=False, want_hits=True,
                                          count_segments=True)
            assert st.segments == len(o)
            assert np.array_equal(hits["index"], r["hits"]["index"]), (scene, cull_min, prec)
            assert same_bytes(hits, r["hits"]), (scene, cull_min, prec)
    report("views_vs_oracle", {"what": "path64_rays", "scene": scene, "cull_min": cull_min,
                               "rays": int(len(o)), "max_abs_delta": float(p64.max()),
                               "above_2e-5": int((p64 > PATH64_TOL).sum()),
                               "max_ref": float(np.abs(ref).max())})
    if scene in BOUNDED:
        assert p64.max() <= PATH64_BOUND, (scene, cull_min, float(p64.max()))
