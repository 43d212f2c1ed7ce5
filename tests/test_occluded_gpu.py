"""GPU: the occlusion query (rt_occluded / rt_occluded_device) against the expected masks of
tests/occluded_fixture.py, on an MI355X (`pytest -m gpu`).  The query is exact: every mask
comparison is equality."""
import ctypes as C

import numpy as np
import pytest

from conftest import GOLDEN, has_gpu, scene_by_name
from occluded_fixture import (drawn_limits, expected_occluded, expected_params, point_pairs)
from rtamd import capi, scenes

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")]

SCENES = ("default", "s8w4", "s64w6")
INT32_MAX = 2**31 - 1
DBL_MAX = np.finfo(np.float64).max
DEFAULT_CLUSTER_COS = 400   # RT_OPT_CLUSTER_COS's default in thousandths (include/rt_capi.h)


@pytest.fixture(scope="module")
def rend():
    r = capi.Renderer(0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def cases(oracle, golden_rays):
    """Per scene, computed once and shared read-only: prims, the golden rays with their
    parameter matrix T, the drawn finite limits, and the point-pair batch with its matrix."""
    out = {}
    for name in SCENES:
        prims = scenes.to_prims(scene_by_name(name))
        o = np.ascontiguousarray(golden_rays[f"{name}__o"])
        d = np.ascontiguousarray(golden_rays[f"{name}__d"])
        po, pd = point_pairs(300, 20261020)
        out[name] = dict(prims=prims, o=o, d=d, T=expected_params(oracle, prims, o, d),
                         lim=drawn_limits(len(o), 7), po=po, pd=pd,
                         PT=expected_params(oracle, prims, po, pd))
    return out


def between(mask, lo=0.05, hi=0.95):
    return lo <= float(np.mean(mask)) <= hi


# ---------------------------------------------------------------- 1. no limit
@pytest.mark.parametrize("name", SCENES)
def test_no_limit(rend, cases, name):
    c = cases[name]
    rend.set_scene(c["prims"])
    idx = np.load(f"{GOLDEN}/ray_hits.npz")[f"{name}__index"]
    mask, count, st = rend.occluded(c["o"], c["d"])
    assert mask.dtype == np.uint8 and mask.shape == (len(idx),)
    assert np.array_equal(mask, (idx >= 0).astype(np.uint8))
    assert count == int(mask.sum()) and st.segments == len(idx)
    _, hits, _ = rend.trace_rays(c["o"], c["d"], 0, want_rgb=False, want_hits=True)
    assert np.array_equal(mask, (hits["index"] >= 0).astype(np.uint8))
    none, count2, _ = rend.occluded(c["o"], c["d"], want_mask=False)
    assert none is None and count2 == count


# ---------------------------------------------------------------- 2. finite limits, point pairs
@pytest.mark.parametrize("name", SCENES)
def test_finite_limits(rend, cases, name):
    c = cases[name]
    rend.set_scene(c["prims"])
    exp = expected_occluded(c["T"], c["lim"])
    mask, count, _ = rend.occluded(c["o"], c["d"], c["lim"])
    print("finite limits", name, "occluded fraction", float(exp.mean()))
    assert np.array_equal(mask, exp) and count == int(exp.sum())
    if name != "default":
        assert between(exp)
        # the limits decide: the unlimited answer differs
        assert int(expected_occluded(c["T"], np.inf).sum()) > int(exp.sum())


@pytest.mark.parametrize("name", SCENES)
def test_point_pairs(rend, cases, name):
    c = cases[name]
    rend.set_scene(c["prims"])
    exp = expected_occluded(c["PT"], 1.0)
    mask, count, _ = rend.occluded(c["po"], c["pd"], 1.0)
    print("point pairs", name, "occluded fraction", float(exp.mean()))
    assert np.array_equal(mask, exp) and count == int(exp.sum())
    if name != "default":
        assert between(exp)


# ---------------------------------------------------------------- 3. the boundary
@pytest.mark.parametrize("name,min_s,min_w", [("s8w4", 10, 50), ("s64w6", 50, 50)])
def test_boundary(rend, cases, name, min_s, min_w):
    """T equal to the first blocker's parameter occludes; the next double towards 0 does not
    (unless another primitive ties); the next one up does."""
    c = cases[name]
    rend.set_scene(c["prims"])
    has = ~np.isnan(c["T"]).all(axis=1)
    o, d, T = c["o"][has], c["d"][has], c["T"][has]
    T0 = np.nanmin(T, axis=1)
    first = np.nanargmin(T, axis=1)
    kinds = np.array([p.kind for p in c["prims"]])[first]
    assert int((kinds == capi.RT_PRIM_SPHERE).sum()) >= min_s
    assert int((kinds == capi.RT_PRIM_WALL).sum()) >= min_w
    at, _, _ = rend.occluded(o, d, T0)
    assert at.all()
    below = np.nextafter(T0, 0.0)
    m, _, _ = rend.occluded(o, d, below)
    exp = expected_occluded(T, below)
    assert np.array_equal(m, exp)                      # 0 unless another primitive ties
    assert not exp.all()
    above, _, _ = rend.occluded(o, d, np.nextafter(T0, np.inf))
    assert above.all()


# ---------------------------------------------------------------- 4. special limits
@pytest.mark.parametrize("name", ["s8w4", "s64w6"])
def test_special_limits(rend, cases, name):
    c = cases[name]
    rend.set_scene(c["prims"])
    hit = ~np.isnan(c["T"]).all(axis=1)
    o, d = c["o"][hit], c["d"][hit]
    assert len(o) > 50 and np.nanmin(c["T"][hit]) > 1e-300
    for t, want in ((np.nan, 0), (0.0, 0), (-1.0, 0), (1e-300, 0), (DBL_MAX, 1), (np.inf, 1)):
        mask, count, _ = rend.occluded(o, d, t)
        assert (mask == want).all() and count == want * len(o), t


# ---------------------------------------------------------------- 5. batch edges
def test_batch_edges(rend, cases):
    import torch
    c = cases["s8w4"]
    rend.set_scene(c["prims"])
    full, _, _ = rend.occluded(c["o"], c["d"], c["lim"])
    dev = torch.device("cuda", 0)
    t_o, t_d = torch.from_numpy(c["o"]).to(dev), torch.from_numpy(c["d"]).to(dev)
    t_t = torch.from_numpy(c["lim"]).to(dev)
    for n in (1, 63, 64, 65, 129):
        mask, count, st = rend.occluded(c["o"][:n], c["d"][:n], c["lim"][:n])
        assert np.array_equal(mask, full[:n]) and count == int(full[:n].sum()), n
        assert st.segments == n
        t_out = torch.full((n + 64,), 0xAB, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        rend.occluded_device(t_o.data_ptr(), t_d.data_ptr(), t_t.data_ptr(), n, t_out.data_ptr())
        torch.cuda.synchronize()
        got = t_out.cpu().numpy()
        assert np.array_equal(got[:n], full[:n]), n
        assert (got[n:] == 0xAB).all(), n


# ---------------------------------------------------------------- 6. scan paths agree
def test_scan_paths_agree(rend, cases):
    settings = [("s64w6", mn, cc) for mn in (0, INT32_MAX) for cc in (-2000, 2000)]
    settings.append(("s8w4", 0, None))
    try:
        for name, min_spheres, clu_cos in settings:
            c = cases[name]
            rend.set_scene(c["prims"])
            rend.set_option(capi.RT_OPT_WAVE_CULL_MIN_SPHERES, min_spheres)
            if clu_cos is not None:
                rend.set_option(capi.RT_OPT_CLUSTER_COS, clu_cos)
            mask, _, _ = rend.occluded(c["o"], c["d"], c["lim"])
            assert np.array_equal(mask, expected_occluded(c["T"], c["lim"])), (name, min_spheres, clu_cos)
            mask, _, _ = rend.occluded(c["po"], c["pd"], 1.0)
            assert np.array_equal(mask, expected_occluded(c["PT"], 1.0)), (name, min_spheres, clu_cos)
            mask, _, _ = rend.occluded(c["o"], c["d"])
            assert np.array_equal(mask, expected_occluded(c["T"], np.inf)), (name, min_spheres, clu_cos)
    finally:
        rend.set_option(capi.RT_OPT_WAVE_CULL_MIN_SPHERES, 24)
        rend.set_option(capi.RT_OPT_CLUSTER_COS, DEFAULT_CLUSTER_COS)


# ---------------------------------------------------------------- 7. device form
def test_device_form_on_a_torch_stream(rend, cases):
    import torch
    c = cases["s64w6"]
    rend.set_scene(c["prims"])
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(dev)
    n, m = len(c["o"]), len(c["po"])
    exp_a = expected_occluded(c["T"], c["lim"])
    exp_b = expected_occluded(c["PT"], 1.0)
    t_o, t_d = torch.from_numpy(c["o"]).to(dev), torch.from_numpy(c["d"]).to(dev)
    t_t = torch.from_numpy(c["lim"]).to(dev)
    p_o, p_d = torch.from_numpy(c["po"]).to(dev), torch.from_numpy(c["pd"]).to(dev)
    p_t = torch.ones(m, dtype=torch.float64, device=dev)
    out_a = torch.full((n,), 0xAB, dtype=torch.uint8, device=dev)
    out_b = torch.full((m,), 0xAB, dtype=torch.uint8, device=dev)
    cnt = torch.zeros(1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    rend.occluded_device(t_o.data_ptr(), t_d.data_ptr(), t_t.data_ptr(), n, out_a.data_ptr(),
                         cnt.data_ptr(), st.cuda_stream)
    rend.occluded_device(p_o.data_ptr(), p_d.data_ptr(), p_t.data_ptr(), m, out_b.data_ptr(),
                         cnt.data_ptr(), st.cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(out_a.cpu().numpy(), exp_a) and np.array_equal(out_b.cpu().numpy(), exp_b)
    assert int(cnt.item()) == int(exp_a.sum()) + int(exp_b.sum())
    # the count alone, then the mask alone (no limits: d_tmax = 0)
    cnt.zero_()
    torch.cuda.synchronize()
    rend.occluded_device(t_o.data_ptr(), t_d.data_ptr(), t_t.data_ptr(), n, 0, cnt.data_ptr(),
                         st.cuda_stream)
    out_a.fill_(0xAB)
    torch.cuda.synchronize()
    rend.occluded_device(t_o.data_ptr(), t_d.data_ptr(), 0, n, out_a.data_ptr(), 0, st.cuda_stream)
    torch.cuda.synchronize()
    assert int(cnt.item()) == int(exp_a.sum())
    assert np.array_equal(out_a.cpu().numpy(), expected_occluded(c["T"], np.inf))


# ---------------------------------------------------------------- 8. status codes
def test_status_codes(rend, cases):
    c = cases["s8w4"]
    lib, dp = rend.lib, C.POINTER(C.c_double)
    o, d = c["o"][:8].copy(), c["d"][:8].copy()
    po, pd = o.ctypes.data_as(dp), d.ctypes.data_as(dp)
    out = np.full(8, 0xAB, np.uint8)
    pout = out.ctypes.data_as(C.POINTER(C.c_uint8))
    cnt = C.c_uint64(77)
    with capi.Renderer(0) as fresh:
        assert lib.rt_occluded(fresh.ctx, po, pd, None, 8, pout, None, None) == capi.RT_ERR_NO_SCENE
        assert lib.rt_occluded_device(fresh.ctx, C.c_void_p(8), C.c_void_p(8), None, 8, C.c_void_p(8),
                                      None, None) == capi.RT_ERR_NO_SCENE
    rend.set_scene(c["prims"])
    st = capi.rt_stats()
    assert lib.rt_occluded(rend.ctx, po, pd, None, 0, pout, C.byref(cnt), C.byref(st)) == capi.RT_OK
    assert (out == 0xAB).all() and cnt.value == 77 and st.segments == 0
    assert lib.rt_occluded_device(rend.ctx, None, None, None, 0, C.c_void_p(8), None, None) == capi.RT_OK
    assert lib.rt_occluded(rend.ctx, po, pd, None, -1, pout, None, None) == capi.RT_ERR_INVALID_ARG
    assert lib.rt_occluded(rend.ctx, po, pd, None, 2**31, pout, None, None) == capi.RT_ERR_INVALID_ARG
    assert lib.rt_occluded(rend.ctx, po, pd, None, 8, None, None, None) == capi.RT_ERR_INVALID_ARG
    assert lib.rt_occluded(rend.ctx, None, pd, None, 8, pout, None, None) == capi.RT_ERR_INVALID_ARG
    assert lib.rt_occluded(rend.ctx, po, None, None, 8, pout, None, None) == capi.RT_ERR_INVALID_ARG
    assert lib.rt_occluded_device(rend.ctx, C.c_void_p(8), C.c_void_p(8), None, -1, C.c_void_p(8),
                                  None, None) == capi.RT_ERR_INVALID_ARG
    assert lib.rt_occluded_device(rend.ctx, C.c_void_p(8), C.c_void_p(8), None, 8, None, None,
                                  None) == capi.RT_ERR_INVALID_ARG
    assert (out == 0xAB).all()
    # an empty scene: nothing blocks
    rend.set_scene([])
    mask, count, _ = rend.occluded(c["o"], c["d"])
    assert not mask.any() and count == 0
    rend.set_scene(c["prims"])


# ---------------------------------------------------------------- 9. frames undisturbed
def test_frames_unchanged_by_occlusion_calls(rend, cases):
    c = cases["s8w4"]
    rend.set_scene(c["prims"])
    cam = capi.camera_init(**scenes.camera_args(64, 48))
    a, sa = rend.render(cam, 4, capi.RT_PREC_PATH64, 0, capi.RT_OUT_RGB_F32, count_segments=True)
    rend.occluded(c["o"], c["d"], c["lim"])
    b, sb = rend.render(cam, 4, capi.RT_PREC_PATH64, 0, capi.RT_OUT_RGB_F32, count_segments=True)
    assert a.tobytes() == b.tobytes() and sa.segments == sb.segments
