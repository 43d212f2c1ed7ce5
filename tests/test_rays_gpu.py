"""GPU: ray-batch queries (rt_trace_rays / rt_trace_rays_device) against the reference's own
numbers (tests/golden/rays.npz, ray_hits.npz) and the oracle, on an MI355X (`pytest -m gpu`).

Bounds: F64 |delta| <= 1e-12 per channel (the project's F64 bound: the geometry is bit-exact,
only pow's last bit differs); MIXED bytewise F64; PATH64 <= 1e-4 per channel (north_star), how
many rays exceed PATH64_TOL = 2e-5 is reported, not gated (random origins inside spheres and
|d| of 0.3-2 have not been measured at that bound); hit records bitwise the reference's.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, has_gpu, scene_by_name
from rtamd import capi, scenes

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")]

F64_TOL = 1e-12
PATH64_BOUND = 1e-4
PATH64_TOL = 2e-5
F64, MIXED, PATH64 = capi.RT_PREC_F64, capi.RT_PREC_MIXED, capi.RT_PREC_PATH64
INT32_MAX = 2**31 - 1


@pytest.fixture(scope="module")
def rend():
    r = capi.Renderer(0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def golden_hits():
    return np.load(os.path.join(GOLDEN, "ray_hits.npz"))


def _d3(v):
    return (C.c_double * 3)(float(v[0]), float(v[1]), float(v[2]))


def orc_trace(oracle, prims, o, d, depth, flags=0):
    """oracle.trace over a batch -> (rgb [n, 3], segments of each ray [n])."""
    arr, n = oracle.prim_array(prims), len(prims)
    depth = np.broadcast_to(np.asarray(depth), (len(o),))
    rgb, segs = np.empty((len(o), 3)), np.empty(len(o), np.int64)
    out3, s = (C.c_double * 3)(), C.c_uint64()
    for k in range(len(o)):
        oracle.lib.orc_trace(arr, n, _d3(o[k]), _d3(d[k]), int(depth[k]), flags, out3, C.byref(s))
        rgb[k] = out3[:]
        segs[k] = s.value
    return rgb, segs


def orc_hits(oracle, prims, o, d):
    """oracle.find_closest_hit over a batch -> HIT_DTYPE records."""
    arr, n = oracle.prim_array(prims), len(prims)
    out = np.zeros(len(o), capi.HIT_DTYPE)
    dist, nrm = C.c_double(), (C.c_double * 3)()
    for k in range(len(o)):
        out["index"][k] = oracle.lib.orc_find_closest_hit(arr, n, _d3(o[k]), _d3(d[k]),
                                                          C.byref(dist), nrm)
        out["distance"][k] = dist.value
        out["normal"][k] = nrm[:]
    return out


def fixture_hits(golden_hits, name):
    rec = np.zeros(len(golden_hits[f"{name}__index"]), capi.HIT_DTYPE)
    rec["index"] = golden_hits[f"{name}__index"]
    rec["distance"] = golden_hits[f"{name}__dist"]
    rec["normal"] = golden_hits[f"{name}__normal"]
    return rec


def random_rays(n, seed):
    """The fixture's distribution (tests/golden/make_golden.py), seeded."""
    rng = np.random.default_rng(seed)
    o = rng.uniform([-2, -5, -2], [9, 5, 3], size=(n, 3))
    d = rng.normal(size=(n, 3)) * rng.choice([0.3, 1.0, 2.0], size=(n, 1))
    return o, d


def camera_rays(cam):
    """Pixel rays of a camera as a batch, row-major: pos - ((tl + dx*x) + dy*i), main.cpp:132-133."""
    pos, tl = np.array(cam.position[:]), np.array(cam.image_top_left[:])
    dx, dy = np.array(cam.pixel_delta_x[:]), np.array(cam.pixel_delta_y[:])
    i, x = np.meshgrid(np.arange(cam.height, dtype=np.float64),
                       np.arange(cam.width, dtype=np.float64), indexing="ij")
    pc = (tl + dx * x[..., None]) + dy * i[..., None]
    d = (pos - pc).reshape(-1, 3)
    return np.broadcast_to(pos, d.shape).copy(), d


def same_bytes(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def s8w4_d4(oracle, golden_rays):
    """The s8w4 fixture rays at depth 4 with the oracle's radiance, segments and hits (computed
    once, shared read-only)."""
    prims = scenes.to_prims(scene_by_name("s8w4"))
    o, d = golden_rays["s8w4__o"], golden_rays["s8w4__d"]
    rgb, segs = orc_trace(oracle, prims, o, d, 4)
    return dict(prims=prims, o=o, d=d, rgb=rgb, segs=segs, hits=orc_hits(oracle, prims, o, d))


# ---------------------------------------------------------------- 1. radiance vs the reference
@pytest.mark.parametrize("name", ["default", "s8w4", "s64w6"])
def test_radiance_matches_reference_rays(rend, oracle, golden_rays, name):
    prims = scenes.to_prims(scene_by_name(name))
    rend.set_scene(prims)
    o, d = golden_rays[f"{name}__o"], golden_rays[f"{name}__d"]
    depth, ref = golden_rays[f"{name}__depth"], golden_rays[f"{name}__rgb"]
    _, osegs = orc_trace(oracle, prims, o, d, depth)
    assert set(np.unique(depth)) == set(range(9))
    p64_delta = np.zeros(len(o))
    for dep in range(9):
        m = depth == dep
        a, _, st = rend.trace_rays(o[m], d[m], dep, F64, count_segments=True)
        assert a.shape == (int(m.sum()), 3) and a.dtype == np.float64
        assert np.abs(a - ref[m]).max() <= F64_TOL, (name, dep)
        assert st.segments == int(osegs[m].sum()), (name, dep)
        b, _, _ = rend.trace_rays(o[m], d[m], dep, MIXED)
        assert same_bytes(a, b), (name, dep)
        p, _, sp = rend.trace_rays(o[m], d[m], dep, PATH64, count_segments=True)
        assert sp.segments == int(osegs[m].sum()), (name, dep)
        p64_delta[m] = np.abs(p - ref[m]).max(axis=-1)
    rep = {"scene": name, "rays": int(len(o)), "max_abs_delta": float(p64_delta.max()),
           "above_2e-5": int((p64_delta > PATH64_TOL).sum()),
           "above_1e-4": int((p64_delta > PATH64_BOUND).sum())}
    print("path64_random_rays", rep)
    out = os.environ.get("RT_RAYS_REPORT")
    if out:
        with open(out, "a") as fh:
            fh.write(json.dumps(rep) + "\n")
    assert np.isfinite(p64_delta).all() and p64_delta.max() <= PATH64_BOUND, rep


# ---------------------------------------------------------------- 2. hits vs the reference
@pytest.mark.parametrize("name", ["default", "s8w4", "s64w6"])
def test_hits_match_reference_bitwise(rend, golden_rays, golden_hits, name):
    rend.set_scene(scenes.to_prims(scene_by_name(name)))
    o, d = golden_rays[f"{name}__o"], golden_rays[f"{name}__d"]
    exp = fixture_hits(golden_hits, name)
    for prec in (F64, PATH64):
        rgb, hits, st = rend.trace_rays(o, d, 3, prec, want_rgb=False, want_hits=True,
                                        count_segments=True)
        assert rgb is None and st.segments == len(o)   # one segment per ray, no bounce
        assert np.array_equal(hits["index"], exp["index"]), (name, prec)
        assert same_bytes(hits["distance"], exp["distance"]), (name, prec)
        assert same_bytes(hits["normal"], exp["normal"]), (name, prec)
        assert same_bytes(hits, exp), (name, prec)      # whole records, every miss included
        # radiance and hits in one call: the same hits, the radiance of a radiance-only call
        both, h2, _ = rend.trace_rays(o, d, 3, prec, want_hits=True)
        alone, _, _ = rend.trace_rays(o, d, 3, prec)
        assert same_bytes(h2, exp) and same_bytes(both, alone), (name, prec)


# ---------------------------------------------------------------- 3. large-scene paths
@pytest.mark.parametrize("name", ["s256w0", "s64w6"])
def test_large_scene_paths(oracle, name):
    """Random rays (incoherent: the per-lane cluster walk) and a 64x48 camera's pixel rays as a
    batch (coherent: the wave cone) on the wave-cull scenes; every cull option gives the
    same bytes."""
    depth = 6
    prims = scenes.to_prims(scene_by_name(name))
    cam = capi.camera_init(**scenes.camera_args(64, 48))
    frame, _, fsegs = oracle.render(prims, cam, depth)
    batches = {"random": random_rays(1000, 77), "camera": camera_rays(cam)}
    with capi.Renderer(0) as r:
        r.set_scene(prims)
        base = {}
        for kind, (o, d) in batches.items():
            rgb, hits, st = r.trace_rays(o, d, depth, F64, want_hits=True, count_segments=True)
            if kind == "camera":
                ergb, esegs = frame.reshape(-1, 3), fsegs
            else:
                ergb, s = orc_trace(oracle, prims, o, d, depth)
                esegs = int(s.sum())
            assert np.abs(rgb - ergb).max() <= F64_TOL, (name, kind)
            assert st.segments == esegs, (name, kind)
            eh = orc_hits(oracle, prims, o, d)
            assert np.array_equal(hits["index"], eh["index"]), (name, kind)
            assert same_bytes(hits, eh), (name, kind)
            base[kind] = (rgb, hits)
        settings = [(capi.RT_OPT_WAVE_CULL_MIN_SPHERES, 0), (capi.RT_OPT_WAVE_CULL_MIN_SPHERES, INT32_MAX),
                    (capi.RT_OPT_WAVE_CULL_MIN_SPHERES, 24), (capi.RT_OPT_CLUSTER_COS, -2000),
                    (capi.RT_OPT_CLUSTER_COS, 2000)]
        for opt, val in settings:
            r.set_option(opt, val)
            for kind, (o, d) in batches.items():
                rgb, hits, _ = r.trace_rays(o, d, depth, F64, want_hits=True)
                assert same_bytes(rgb, base[kind][0]), (name, kind, opt, val)
                assert same_bytes(hits, base[kind][1]), (name, kind, opt, val)


# ---------------------------------------------------------------- 4. ragged sizes and edges
def test_ragged_sizes_and_sentinels(rend, s8w4_d4):
    rend.set_scene(s8w4_d4["prims"])
    o = np.ascontiguousarray(s8w4_d4["o"][:129])
    d = np.ascontiguousarray(s8w4_d4["d"][:129])
    full_rgb, full_hits, _ = rend.trace_rays(o, d, 4, F64, want_hits=True)
    assert np.abs(full_rgb - s8w4_d4["rgb"][:129]).max() <= F64_TOL
    lib, dp = rend.lib, C.POINTER(C.c_double)
    for n in (1, 63, 64, 65, 129):
        rgb = np.full((n + 1, 3), -7.25)
        hits = np.zeros(n + 1, capi.HIT_DTYPE)
        hits["distance"], hits["index"], hits["reserved"] = -7.25, 1234567, 89
        st = capi.rt_stats()
        capi.check(lib.rt_trace_rays(rend.ctx, o.ctypes.data_as(dp), d.ctypes.data_as(dp), n, 4, F64,
                                     0, capi.RT_OUT_RGB_F64, rgb.ctypes.data_as(C.c_void_p),
                                     hits.ctypes.data_as(C.POINTER(capi.rt_hit)), 1, C.byref(st)),
                   rend.ctx)
        assert same_bytes(rgb[:n], full_rgb[:n]) and same_bytes(hits[:n], full_hits[:n]), n
        assert (rgb[n] == -7.25).all(), n                      # the record past the end survives
        assert hits[n]["distance"] == -7.25 and hits[n]["index"] == 1234567 and hits[n]["reserved"] == 89
        assert st.segments == int(s8w4_d4["segs"][:n].sum()), n
        # hits alone
        h1 = hits.copy()
        h1["distance"][:n] = 0
        capi.check(lib.rt_trace_rays(rend.ctx, o.ctypes.data_as(dp), d.ctypes.data_as(dp), n, 4, F64,
                                     0, capi.RT_OUT_RGB_F64, None,
                                     h1.ctypes.data_as(C.POINTER(capi.rt_hit)), 0, None), rend.ctx)
        assert same_bytes(h1, hits), n
    # n == 0: RT_OK, nothing written
    rgb = np.full((1, 3), -7.25)
    assert lib.rt_trace_rays(rend.ctx, o.ctypes.data_as(dp), d.ctypes.data_as(dp), 0, 4, F64, 0,
                             capi.RT_OUT_RGB_F64, rgb.ctypes.data_as(C.c_void_p), None, 1,
                             None) == capi.RT_OK
    assert (rgb == -7.25).all()
    e_rgb, e_hits, _ = rend.trace_rays(np.zeros((0, 3)), np.zeros((0, 3)), 4, F64, want_hits=True)
    assert e_rgb.shape == (0, 3) and e_hits.shape == (0,)


def test_depth_limits_and_empty_scene(rend, oracle, s8w4_d4):
    prims, o, d = s8w4_d4["prims"], s8w4_d4["o"][:129], s8w4_d4["d"][:129]
    rend.set_scene(prims)
    maxd = rend.lib.rt_max_depth()
    for depth in (0, maxd):
        ergb, esegs = orc_trace(oracle, prims, o, d, depth)
        for prec, tol in ((F64, F64_TOL), (PATH64, PATH64_BOUND)):
            rgb, _, st = rend.trace_rays(o, d, depth, prec, count_segments=True)
            assert np.abs(rgb - ergb).max() <= tol, (depth, prec)
            assert st.segments == int(esegs.sum()), (depth, prec)
    with pytest.raises(capi.RTError) as ei:
        rend.trace_rays(o, d, maxd + 1, F64)
    assert ei.value.status == capi.RT_ERR_UNSUPPORTED
    # an empty scene: the oracle's sky or ground colour and a miss record for every ray
    rend.set_scene([])
    ergb, esegs = orc_trace(oracle, [], o, d, 4)
    assert (esegs == 1).all() and (d[:, 2] < 0).any() and (d[:, 2] > 0).any()
    for prec, tol in ((F64, F64_TOL), (PATH64, PATH64_BOUND)):
        rgb, hits, st = rend.trace_rays(o, d, 4, prec, want_hits=True, count_segments=True)
        assert np.abs(rgb - ergb).max() <= tol
        assert st.segments == len(o)
        miss = np.zeros(len(o), capi.HIT_DTYPE)
        miss["distance"], miss["index"] = np.finfo(np.float64).max, -1
        assert same_bytes(hits, miss)
    rend.set_scene(prims)


# ---------------------------------------------------------------- 5. interleaved scene order
def test_interleaved_scene_and_coincident_spheres(oracle):
    M = scenes.Material
    sc = [scenes.Wall(M((.3, .3, .8), .4), (3, 4, -1), (0, -1, 0), 8, 4),
          scenes.Sphere(M((.9, .2, .2), .6), (4.0, 0.5, 0.2), .7),
          scenes.Wall(M((.5, .5, .5), .5), (10, -4, -1), (-1, 0, 0), 8, 4),
          scenes.Sphere(M((.2, .9, .2), .3), (5.5, -1.0, 0.0), .6),
          # two coincident spheres: find_closest_hit's strict < keeps the lower index
          scenes.Sphere(M((.1, .1, .9), .5), (3.0, -2.0, 0.5), .5),
          scenes.Sphere(M((.9, .9, .1), .2), (3.0, -2.0, 0.5), .5)]
    prims = scenes.to_prims(sc)
    o, d = random_rays(600, 5)
    # aimed rays: at both named spheres, the coincident pair and both walls
    targets = np.array([(4.0, 0.5, 0.2), (5.5, -1.0, 0.0), (3.0, -2.0, 0.5), (0.0, 4.0, 0.5),
                        (10.0, 0.0, 1.0)])
    ao = np.tile(np.array([(0.0, 0.0, 0.0), (1.0, -0.5, 0.3), (-1.0, 1.0, 0.0)]), (len(targets), 1))
    ad = (np.repeat(targets, 3, axis=0) - ao) * 0.7
    o, d = np.concatenate([o, ao]), np.concatenate([d, ad])
    eh = orc_hits(oracle, prims, o, d)
    ergb, _ = orc_trace(oracle, prims, o, d, 5)
    assert set(eh["index"]) >= {-1, 0, 1, 2, 3, 4} and 5 not in set(eh["index"])
    with capi.Renderer(0) as r:
        r.set_scene(prims)
        for cull_min in (24, 0):   # the linear scan, then the wave-cull kernels
            r.set_option(capi.RT_OPT_WAVE_CULL_MIN_SPHERES, cull_min)
            rgb, hits, _ = r.trace_rays(o, d, 5, F64, want_hits=True)
            assert np.array_equal(hits["index"], eh["index"]), cull_min   # SCENE indices
            assert same_bytes(hits, eh), cull_min
            assert np.abs(rgb - ergb).max() <= F64_TOL, cull_min


# ---------------------------------------------------------------- 6. formats and sun
def test_output_formats(rend, oracle, s8w4_d4):
    rend.set_scene(s8w4_d4["prims"])
    o, d, o64 = s8w4_d4["o"], s8w4_d4["d"], s8w4_d4["rgb"]
    f64, _, _ = rend.trace_rays(o, d, 4, F64)
    f32, _, _ = rend.trace_rays(o, d, 4, F64, out_format=capi.RT_OUT_RGB_F32)
    assert f32.dtype == np.float32 and f32.shape == (len(o), 3)
    assert same_bytes(f32, f64.astype(np.float32))       # the rounded F64
    ulp = np.abs(f32.view(np.int32).astype(np.int64) - o64.astype(np.float32).view(np.int32).astype(np.int64))
    assert ulp.max() <= 1 and (ulp == 0).mean() > 0.999
    img, _, _ = rend.trace_rays(o, d, 4, F64, out_format=capi.RT_OUT_RGBA8)
    assert img.dtype == np.uint8 and img.shape == (len(o), 4) and (img[:, 3] == 255).all()
    exp = np.floor(np.clip(o64, 0.0, 1.0) * 255.0).astype(np.uint8)   # main.cpp:345 truncation
    edge = np.abs(np.clip(o64, 0, 1) * 255.0 - np.round(np.clip(o64, 0, 1) * 255.0)) < 1e-9
    assert ((img[:, :3] == exp) | edge).all()
    wrap, _, _ = rend.trace_rays(o, d, 4, F64, out_format=capi.RT_OUT_RGBA8_WRAP)
    t = o64 * 255.0
    edge = np.abs(t - np.round(t)) < 1e-9
    assert (wrap[:, 3] == 255).all()
    assert ((wrap[:, :3] == oracle.surface_u8(o64)) | edge).all()


def test_sun_flag(rend, oracle, s8w4_d4):
    prims, o, d = s8w4_d4["prims"], s8w4_d4["o"], s8w4_d4["d"]
    rend.set_scene(prims)
    ergb, esegs = orc_trace(oracle, prims, o, d, 4, flags=capi.RT_FLAG_SUN)
    assert np.abs(ergb - s8w4_d4["rgb"]).max() > 1e-3     # the flag changes lit rays
    a, _, st = rend.trace_rays(o, d, 4, F64, flags=capi.RT_FLAG_SUN, count_segments=True)
    assert np.abs(a - ergb).max() <= F64_TOL and st.segments == int(esegs.sum())
    p, _, _ = rend.trace_rays(o, d, 4, PATH64, flags=capi.RT_FLAG_SUN)
    assert np.abs(p - ergb).max() <= PATH64_BOUND


# ---------------------------------------------------------------- 7. frames untouched
def test_frames_unchanged_by_ray_calls(rend, s8w4_d4):
    rend.set_scene(s8w4_d4["prims"])
    cam = capi.camera_init(**scenes.camera_args(96, 54))
    for prec in (PATH64, F64):
        a, sa = rend.render(cam, 4, prec, 0, capi.RT_OUT_RGB_F64, count_segments=True)
        rend.trace_rays(s8w4_d4["o"], s8w4_d4["d"], 4, prec, want_hits=True, count_segments=True)
        b, sb = rend.render(cam, 4, prec, 0, capi.RT_OUT_RGB_F64, count_segments=True)
        assert same_bytes(a, b) and sa.segments == sb.segments, prec


# ---------------------------------------------------------------- 8. device variant, errors
def test_device_variant_on_a_torch_stream(rend, golden_rays):
    import torch
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(dev)
    pa = scenes.to_prims(scene_by_name("s64w6"))
    pb = scenes.to_prims(scenes.synthetic_scene(64, 6, seed=99))
    # enough rays that the batch is still in flight when the scene is replaced
    o = np.tile(golden_rays["s64w6__o"], (64, 1))
    d = np.tile(golden_rays["s64w6__d"], (64, 1))
    n = len(o)
    rend.set_scene(pa)
    for prec in (F64, PATH64):
        rgb, hits, hst = rend.trace_rays(o, d, 8, prec, want_hits=True, count_segments=True)
        t_o, t_d = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
        t_rgb = torch.full((n, 3), -1.0, dtype=torch.float64, device=dev)
        t_hits = torch.zeros(n * 40, dtype=torch.uint8, device=dev)
        t_segs = torch.zeros(1, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        rend.trace_rays_device(t_o.data_ptr(), t_d.data_ptr(), n, 8, t_rgb.data_ptr(),
                               t_hits.data_ptr(), prec, d_segments=t_segs.data_ptr(),
                               stream=st.cuda_stream)
        rend.set_scene(pb)     # the batch above may still be running: it must not see scene B
        torch.cuda.synchronize()
        assert same_bytes(t_rgb.cpu().numpy(), rgb), prec
        assert same_bytes(t_hits.cpu().numpy().view(capi.HIT_DTYPE), hits), prec
        assert int(t_segs.item()) == hst.segments
        other, _, _ = rend.trace_rays(o[:400], d[:400], 8, prec)
        assert not same_bytes(other, rgb[:400])            # scene B is what later calls see
        rend.set_scene(pa)
    # hits only, on the ctx's own stream
    t_hits = torch.zeros(n * 40, dtype=torch.uint8, device=dev)
    rend.trace_rays_device(t_o.data_ptr(), t_d.data_ptr(), n, 0, 0, t_hits.data_ptr())
    rend.set_scene(pa)         # waits for the ctx's stream
    assert same_bytes(t_hits.cpu().numpy().view(capi.HIT_DTYPE), hits)


def test_argument_errors(rend, s8w4_d4):
    rend.set_scene(s8w4_d4["prims"])
    lib, dp = rend.lib, C.POINTER(C.c_double)
    o = np.ascontiguousarray(s8w4_d4["o"][:8])
    d = np.ascontiguousarray(s8w4_d4["d"][:8])
    rgb = np.zeros((8, 3))
    po, pd, pr = o.ctypes.data_as(dp), d.ctypes.data_as(dp), rgb.ctypes.data_as(C.c_void_p)
    fmt = capi.RT_OUT_RGB_F64

    def call(ctx, po, pd, n, prec, pr, ph=None, depth=4):
        return lib.rt_trace_rays(ctx, po, pd, n, depth, prec, 0, fmt, pr, ph, 0, None)

    assert call(rend.ctx, po, pd, 8, F64, pr) == capi.RT_OK
    assert call(rend.ctx, po, pd, 8, capi.RT_PREC_F32, pr) == capi.RT_ERR_UNSUPPORTED
    assert call(rend.ctx, None, pd, 8, F64, pr) == capi.RT_ERR_INVALID_ARG
    assert call(rend.ctx, po, None, 8, F64, pr) == capi.RT_ERR_INVALID_ARG
    assert call(rend.ctx, po, pd, 8, F64, None, None) == capi.RT_ERR_INVALID_ARG
    assert call(rend.ctx, po, pd, -1, F64, pr) == capi.RT_ERR_INVALID_ARG
    assert call(rend.ctx, po, pd, 2**31, F64, pr) == capi.RT_ERR_INVALID_ARG
    assert call(rend.ctx, po, pd, 8, 7, pr) == capi.RT_ERR_INVALID_ARG
    assert call(rend.ctx, po, pd, 8, F64, pr, depth=-1) == capi.RT_ERR_INVALID_ARG
    assert lib.rt_trace_rays(rend.ctx, po, pd, 8, 4, F64, 0, 99, pr, None, 0, None) == capi.RT_ERR_INVALID_ARG
    # the device variant checks the same way (nothing is launched for a rejected call)
    assert lib.rt_trace_rays_device(rend.ctx, None, None, 8, 4, F64, 0, fmt, C.c_void_p(8), None,
                                    None, None) == capi.RT_ERR_INVALID_ARG
    assert lib.rt_trace_rays_device(rend.ctx, C.c_void_p(8), C.c_void_p(8), 8, 4, F64, 0, fmt, None,
                                    None, None, None) == capi.RT_ERR_INVALID_ARG
    assert lib.rt_trace_rays_device(rend.ctx, C.c_void_p(8), C.c_void_p(8), 8, 4, capi.RT_PREC_F32, 0,
                                    fmt, C.c_void_p(8), None, None, None) == capi.RT_ERR_UNSUPPORTED
    with capi.Renderer(0) as r2:   # no scene yet
        assert call(r2.ctx, po, pd, 8, F64, pr) == capi.RT_ERR_NO_SCENE
        assert lib.rt_trace_rays_device(r2.ctx, C.c_void_p(8), C.c_void_p(8), 8, 4, F64, 0, fmt,
                                        C.c_void_p(8), None, None, None) == capi.RT_ERR_NO_SCENE
