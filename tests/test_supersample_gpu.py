"""RT_OPT_SUPERSAMPLE on an MI355X: S x S rays per pixel, resolved in the trace kernel.

The contract (include/rt_capi.h) is exact, so nearly everything here compares bytes: a render
at S equals `tree_mean` — the normative balanced pairwise tree, fp64, columns then rows, times
1 / S^2 — of the plain render of rt_supersample_camera(cam, S), followed by the output
format's conversion restated in numpy.  The S-times larger frame is always read back as
RGB_F64, which holds every precision's sample colours exactly (the fp32-colour precisions
widen without rounding).  Shapes are the smallest at which each edge can go wrong: partial
tiles in x and y cut mid-tile, one output pixel per wave (S = 8), more tile rows than one
(row order active), a band whose first sample row is not tile-aligned.
"""
import contextlib

import numpy as np
import pytest

from conftest import has_gpu
from rtamd import capi, scenes

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")]

F64, F32, MIXED, PATH64 = (capi.RT_PREC_F64, capi.RT_PREC_F32, capi.RT_PREC_MIXED,
                           capi.RT_PREC_PATH64)
O32, O64, O8, O8W = (capi.RT_OUT_RGB_F32, capi.RT_OUT_RGB_F64, capi.RT_OUT_RGBA8,
                     capi.RT_OUT_RGBA8_WRAP)

SCENES = {"s8w4": lambda: scenes.synthetic_scene(8, 4),
          "s64w6": lambda: scenes.synthetic_scene(64, 6)}


@pytest.fixture(scope="module")
def rend():
    r = capi.Renderer(0)
    yield r
    r.close()


@contextlib.contextmanager
def supersample(rend, s):
    rend.set_option(capi.RT_OPT_SUPERSAMPLE, s)
    try:
        yield
    finally:
        rend.set_option(capi.RT_OPT_SUPERSAMPLE, 1)


_scene_on = {}


def use_scene(rend, name):
    if _scene_on.get(id(rend)) != name:
        rend.set_scene(scenes.to_prims(SCENES[name]()))
        _scene_on[id(rend)] = name


def camera(w, h):
    return capi.camera_init(**scenes.camera_args(w, h))


def tree_mean(frame, s):
    """The normative summation: fp64, pairwise over columns, then rows, times 1 / S^2."""
    v = np.asarray(frame, np.float64)
    k = {1: 0, 2: 1, 4: 2, 8: 3}[s]
    for _ in range(k):
        v = v[:, 0::2] + v[:, 1::2]
    for _ in range(k):
        v = v[0::2] + v[1::2]
    return v * (1.0 / (s * s))


def q8(v):
    """RT_OUT_RGBA8's conversion (rt_scan_dev.h q8): clamp to [0, 1], NaN -> 0, truncate v*255."""
    v = np.where(v > 0.0, v, 0.0)
    v = np.where(v < 1.0, v, 1.0)
    return (v * 255.0).astype(np.uint32)


def q8_wrap(v):
    """RT_OUT_RGBA8_WRAP's: int32 truncation of v*255 (out of range -> 0x80000000), low byte."""
    t = v * 255.0
    ok = (t > -2147483649.0) & (t < 2147483648.0)
    i = np.where(ok, np.trunc(np.where(ok, t, 0.0)), -2147483648.0).astype(np.int64)
    return (i & 0xff).astype(np.uint32)


def convert(mean, fmt):
    """store_px on the fp64 mean."""
    if fmt == O64:
        return mean
    if fmt == O32:
        return mean.astype(np.float32)
    q = q8 if fmt == O8 else q8_wrap
    out = np.empty(mean.shape[:2] + (4,), np.uint8)
    out[..., :3] = q(mean).astype(np.uint8)
    out[..., 3] = 255
    return out


_virtual = {}


def virtual_frame(rend, scene, w, h, s, depth, prec, flags=0):
    """The plain (S = 1) render of the S-times larger frame, RGB_F64; computed once."""
    key = (scene, w, h, s, depth, prec, flags)
    if key not in _virtual:
        use_scene(rend, scene)
        img, st = rend.render(capi.supersample_camera(camera(w, h), s), depth, prec, flags, O64,
                              count_segments=True)
        img.setflags(write=False)
        _virtual[key] = (img, st.segments)
    return _virtual[key]


def check_bitwise(rend, scene, w, h, s, depth, prec, fmt, flags=0, ref_prec=None):
    want = convert(tree_mean(virtual_frame(rend, scene, w, h, s, depth,
                                           prec if ref_prec is None else ref_prec, flags)[0], s), fmt)
    use_scene(rend, scene)
    with supersample(rend, s):
        got, _ = rend.render(camera(w, h), depth, prec, flags, fmt)
    assert got.shape == want.shape and got.dtype == want.dtype
    diff = got.view(np.uint8) != want.view(np.uint8)
    assert not diff.any(), (scene, w, h, s, depth, prec, fmt, flags, int(diff.sum()),
                            np.argwhere(diff.reshape(h, w, -1).any(axis=-1))[:4].tolist())


COMBOS = [(F64, O64), (F64, O32), (PATH64, O32), (F32, O32),
          (F64, O8), (F64, O8W), (PATH64, O8), (PATH64, O8W)]


# ------------------------------------------------- 1. bitwise against the plain render
@pytest.mark.parametrize("w,h,s", [(13, 7, 2), (13, 7, 4), (13, 7, 8), (50, 30, 4)])
def test_linear_kernels_bitwise(rend, w, h, s):
    for prec, fmt in COMBOS:
        check_bitwise(rend, "s8w4", w, h, s, 4, prec, fmt)


@pytest.mark.parametrize("s", [2, 4])
def test_mixed_equals_f64(rend, s):
    use_scene(rend, "s8w4")
    with supersample(rend, s):
        a, _ = rend.render(camera(13, 7), 4, MIXED, 0, O64)
        b, _ = rend.render(camera(13, 7), 4, F64, 0, O64)
    assert a.tobytes() == b.tobytes()
    check_bitwise(rend, "s8w4", 13, 7, s, 4, MIXED, O64, ref_prec=F64)


@pytest.mark.parametrize("depth,flags", [(0, 0), (4, capi.RT_FLAG_SUN)])
def test_depth_0_and_sun_bitwise(rend, depth, flags):
    for s in (2, 4):
        for prec, fmt in ((F64, O64), (PATH64, O32), (F32, O32), (F64, O8W)):
            check_bitwise(rend, "s8w4", 13, 7, s, depth, prec, fmt, flags)


# ------------------------------------------------- 2. cull kernels
@pytest.mark.parametrize("prec,fmt", [(F64, O64), (PATH64, O32)])
def test_cull_kernels_bitwise(rend, prec, fmt):
    """64 spheres, depth 6: coherent primary waves (the cone) and scattered bounces (the
    cluster walk); the cull kernels' store recomputes its coordinates after the trace."""
    check_bitwise(rend, "s64w6", 48, 27, 4, 6, prec, fmt)


def test_cull_kernels_on_the_small_scene_bitwise(rend):
    """RT_OPT_WAVE_CULL_MIN_SPHERES = 0 sends the 8-sphere scene through the cull kernels."""
    # references first, by the linear kernels (the wave cull never changes output)
    for prec in (F64, PATH64, F32):
        virtual_frame(rend, "s8w4", 13, 7, 2, 4, prec)
    rend.set_option(capi.RT_OPT_WAVE_CULL_MIN_SPHERES, 0)
    try:
        for prec, fmt in COMBOS:
            check_bitwise(rend, "s8w4", 13, 7, 2, 4, prec, fmt)
    finally:
        rend.set_option(capi.RT_OPT_WAVE_CULL_MIN_SPHERES, 24)


# ------------------------------------------------- 3. bands
@pytest.mark.parametrize("s,r0,n", [(2, 3, 3), (4, 1, 6)])
def test_bands_equal_the_full_frames_rows(rend, s, r0, n):
    """Rows [3, 6) at S = 2 start at sample row 6, rows [1, 7) at S = 4 at sample row 4: the
    band's tiles cut the samples elsewhere than the full frame's, and every lane of an S x S
    square still forms the same sum."""
    use_scene(rend, "s8w4")
    cam = camera(13, 7)
    with supersample(rend, s):
        for prec, fmt in ((F64, O64), (PATH64, O32), (F32, O32), (F64, O8)):
            full, _ = rend.render(cam, 4, prec, 0, fmt)
            band, _ = rend.render(cam, 4, prec, 0, fmt, row0=r0, nrows=n)
            assert band.shape[0] == n
            assert band.tobytes() == full[r0:r0 + n].tobytes(), (s, prec, fmt)


# ------------------------------------------------- 4. segments
def test_segments_count_every_sample(rend):
    for scene, w, h, depth in (("s8w4", 13, 7, 4), ("s64w6", 48, 27, 6)):
        _, want = virtual_frame(rend, scene, w, h, 4, depth, F64)
        use_scene(rend, scene)
        with supersample(rend, 4):
            _, st = rend.render(camera(w, h), depth, F64, 0, O64, count_segments=True)
        assert want > 4 * 4 * w * h and st.segments == want


# ------------------------------------------------- 5. oracle
def discontinuity_mask(sig):
    """True where any pixel of the 3x3 neighbourhood has a different hit-path signature."""
    h, w = sig.shape
    pad = np.pad(sig, 1, mode="edge")
    m = np.zeros((h, w), bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            m |= pad[1 + dy:1 + dy + h, 1 + dx:1 + dx + w] != sig
    return m


def check_f64(img, ref64, mask=None, tol=1e-12, min_frac=1.0, what=""):
    d = np.abs(img - ref64).max(axis=-1)
    bad = d > tol
    frac_ok = 1.0 - bad.mean()
    assert frac_ok >= min_frac, (what, frac_ok, d.max())
    if bad.any():
        assert mask is not None, (what, int(bad.sum()), d.max())
        assert mask[bad].all(), (what, "outlier off a discontinuity")


def test_f64_against_the_oracle(rend, oracle):
    """F64, S = 2, 40x24, depth 4 against tree_mean of the oracle's render of the 80x48
    frame, <= 1e-12; a pixel may exceed it only if one of its samples lies on the oracle
    signature's discontinuity mask (test_gpu_parity.py check_f64's rule)."""
    s, w, h = 2, 40, 24
    sc = SCENES["s8w4"]()
    vcam = capi.supersample_camera(camera(w, h), s)
    o64, _, _, sig = oracle.render(scenes.to_prims(sc), vcam, 4, want_sig=True)
    mask = discontinuity_mask(sig).reshape(h, s, w, s).any(axis=(1, 3))
    use_scene(rend, "s8w4")
    with supersample(rend, s):
        img, _ = rend.render(camera(w, h), 4, F64, 0, O64)
    d = np.abs(img - tree_mean(o64, s)).max()
    print(f"supersample vs oracle: max|d| = {d:.3e}, pixels with a sample on a discontinuity "
          f"{int(mask.sum())}/{mask.size}")
    check_f64(img, tree_mean(o64, s), mask, what="S=2 40x24")


# ------------------------------------------------- 6. frame batches
def _frames_equal_single_renders(rend, scene, w, h, depth, prec, s):
    import torch
    dev = torch.device("cuda", 0)
    use_scene(rend, scene)
    ca = scenes.camera_args(w, h)
    cams = [capi.camera_init(**ca)]
    a = dict(ca)
    a["position"] = (ca["position"][0] + 0.3, ca["position"][1], ca["position"][2])
    cams.append(capi.camera_init(**a))
    with supersample(rend, s):
        refs = [rend.render(c, depth, prec, 0, O32)[0] for c in cams]
        outs = [torch.full((h, w, 3), -1.0, dtype=torch.float32, device=dev) for _ in range(6)]
        torch.cuda.synchronize()
        rend.set_option(capi.RT_OPT_FRAME_BATCH, 4)
        try:
            rend.render_device_frames(cams, depth, [o.data_ptr() for o in outs], prec, 0, O32,
                                      nframes=6)
            torch.cuda.synchronize()
        finally:
            rend.set_option(capi.RT_OPT_FRAME_BATCH, 1)
    for f, o in enumerate(outs):
        assert o.cpu().numpy().tobytes() == refs[f % 2].tobytes(), (scene, prec, s, f)


@pytest.mark.parametrize("prec", [F64, PATH64])
def test_frame_batch_of_supersampled_frames(rend, prec):
    _frames_equal_single_renders(rend, "s8w4", 26, 14, 4, prec, 2)


def test_frame_batch_of_wave_cull_frames(rend):
    """The header promises that wave-cull scenes launch one frame at a time under
    RT_OPT_FRAME_BATCH; the grouping sent them to the table kernels, which do not exist for
    the cull path ("launch k_trace_tab")."""
    _frames_equal_single_renders(rend, "s64w6", 48, 27, 4, PATH64, 1)


def test_frame_batch_with_pixel_pairs(rend):
    rend.set_option(capi.RT_OPT_PIXEL_PAIRS, 1)
    try:
        _frames_equal_single_renders(rend, "s8w4", 50, 30, 4, PATH64, 1)
    finally:
        rend.set_option(capi.RT_OPT_PIXEL_PAIRS, 0)


# ------------------------------------------------- 7. unaffected and refused paths
def test_option_values(rend):
    for bad in (0, 3, 5, 16, -2):
        with pytest.raises(capi.RTError) as e:
            rend.set_option(capi.RT_OPT_SUPERSAMPLE, bad)
        assert e.value.status == capi.RT_ERR_INVALID_ARG
    for ok in (2, 4, 8, 1):
        rend.set_option(capi.RT_OPT_SUPERSAMPLE, ok)


def test_ray_queries_ignore_the_option(rend):
    use_scene(rend, "s8w4")
    rng = np.random.default_rng(7)
    o = np.zeros((256, 3))
    d = np.column_stack([-np.ones(256), rng.uniform(-1, 1, 256), rng.uniform(-1, 1, 256)])
    want = rend.trace_rays(o, d, 4, F64, want_hits=True)
    with supersample(rend, 4):
        got = rend.trace_rays(o, d, 4, F64, want_hits=True)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()


def test_interleaved_parts_are_refused(rend):
    import torch
    use_scene(rend, "s8w4")
    cam = camera(26, 28)
    buf = torch.zeros((28, 26, 3), dtype=torch.float32, device=torch.device("cuda", 0))
    with supersample(rend, 2):
        with pytest.raises(capi.RTError) as e:
            rend.render_device_interleaved(cam, 4, 2, 0, buf.data_ptr(), PATH64)
        assert e.value.status == capi.RT_ERR_UNSUPPORTED
        # one part is the whole frame: a contiguous band, supported
        rend.render_device_interleaved(cam, 4, 1, 0, buf.data_ptr(), PATH64)
        torch.cuda.synchronize()
        want, _ = rend.render(cam, 4, PATH64, 0, O32)
    assert buf.cpu().numpy().tobytes() == want.tobytes()


def test_multi_renderer_refuses_the_option():
    with capi.MultiRenderer([0, 0], transport=capi.RT_TRANSPORT_COPY) as m:
        with pytest.raises(capi.RTError) as e:
            m.set_option(capi.RT_OPT_SUPERSAMPLE, 2)
        assert e.value.status == capi.RT_ERR_UNSUPPORTED
        m.set_option(capi.RT_OPT_SUPERSAMPLE, 1)
        with pytest.raises(capi.RTError) as e:
            m.set_option(capi.RT_OPT_SUPERSAMPLE, 3)
        assert e.value.status == capi.RT_ERR_INVALID_ARG


def test_back_to_1_reproduces_the_plain_frame(rend):
    use_scene(rend, "s8w4")
    cam = camera(50, 30)
    for prec, fmt in ((F64, O64), (PATH64, O32)):
        before, _ = rend.render(cam, 4, prec, 0, fmt)
        with supersample(rend, 4):
            mid, _ = rend.render(cam, 4, prec, 0, fmt)
        after, _ = rend.render(cam, 4, prec, 0, fmt)
        assert after.tobytes() == before.tobytes()
        assert mid.tobytes() != before.tobytes()


# ------------------------------------------------- 8. determinism
def test_deterministic(rend):
    use_scene(rend, "s8w4")
    cam = camera(13, 7)
    with supersample(rend, 8):
        a, _ = rend.render(cam, 4, F64, 0, O64)
        b, _ = rend.render(cam, 4, F64, 0, O64)
    assert a.tobytes() == b.tobytes()
