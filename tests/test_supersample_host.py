"""RT_OPT_SUPERSAMPLE's host half (no device): rt_supersample_camera against its normative
formula, the geometry it promises (the S x S sample centres of a pixel average to the pixel's
centre), argument checking, and the unchanged ABI version."""
import ctypes as C

import numpy as np
import pytest

from rtamd import capi, scenes


def default_cam(w=13, h=7):
    return capi.camera_init(**scenes.camera_args(w, h))


def moved_cam(w=40, h=24):
    """A camera moved after init(): the reference keeps the old image_top_left (main.cpp:154)."""
    cam = capi.camera_init(**scenes.camera_args(w, h))
    for k, d in enumerate((0.3, -0.2, 0.1)):
        cam.position[k] += d
    return cam


CAMS = {"default": default_cam, "moved": moved_cam}


def vec(a):
    return np.array(list(a), np.float64)


def formula(cam, s):
    """include/rt_capi.h, operation for operation, in numpy fp64."""
    S = np.float64(s)
    h = np.float64((s - 1) * 0.5)
    dxs = vec(cam.pixel_delta_x) / S
    dys = vec(cam.pixel_delta_y) / S
    tl = (vec(cam.image_top_left) - dxs * h) - dys * h
    return tl, dxs, dys


@pytest.mark.parametrize("name", sorted(CAMS))
@pytest.mark.parametrize("s", [2, 4, 8])
def test_matches_the_formula_bitwise(name, s):
    cam = CAMS[name]()
    v = capi.supersample_camera(cam, s)
    tl, dxs, dys = formula(cam, s)
    assert vec(v.image_top_left).tobytes() == tl.tobytes()
    assert vec(v.pixel_delta_x).tobytes() == dxs.tobytes()
    assert vec(v.pixel_delta_y).tobytes() == dys.tobytes()
    assert vec(v.position).tobytes() == vec(cam.position).tobytes()
    assert (v.width, v.height) == (cam.width * s, cam.height * s)


@pytest.mark.parametrize("name", sorted(CAMS))
def test_s1_is_a_byte_copy(name):
    cam = CAMS[name]()
    v = capi.supersample_camera(cam, 1)
    assert bytes(v) == bytes(cam)


@pytest.mark.parametrize("name", sorted(CAMS))
@pytest.mark.parametrize("s", [2, 4, 8])
def test_sample_centres_average_to_the_pixel_centre(name, s):
    """Pixel (j, i)'s centre is tl + dx*j + dy*i (main.cpp:132); its S*S samples are the
    virtual camera's pixels (j*S + a, i*S + b).  Their mean differs from the centre by at most
    4 ulp of the largest coordinate magnitude (log2(S*S) + 2 roundings at most)."""
    cam = CAMS[name]()
    v = capi.supersample_camera(cam, s)
    tl, dx, dy = vec(cam.image_top_left), vec(cam.pixel_delta_x), vec(cam.pixel_delta_y)
    vtl, vdx, vdy = vec(v.image_top_left), vec(v.pixel_delta_x), vec(v.pixel_delta_y)
    jj, ii = np.meshgrid(np.arange(cam.width), np.arange(cam.height))
    centre = tl + dx * jj[..., None] + dy * ii[..., None]                     # [H, W, 3]
    a = np.arange(s)
    x = (jj[..., None] * s + a)[:, :, None, :, None]                          # [H, W, 1, S, 1]
    y = (ii[..., None] * s + a)[:, :, :, None, None]                          # [H, W, S, 1, 1]
    samples = vtl + vdx * x + vdy * y                                         # [H, W, S, S, 3]
    mean = samples.mean(axis=(2, 3))
    mag = max(np.abs(centre).max(), np.abs(samples).max())
    assert np.abs(mean - centre).max() <= 4 * np.spacing(mag)


def test_bad_arguments():
    lib = capi.load()
    cam = default_cam()
    out = capi.rt_camera()
    for s in (0, 3, 16):
        assert lib.rt_supersample_camera(C.byref(cam), s, C.byref(out)) == capi.RT_ERR_INVALID_ARG
        with pytest.raises(capi.RTError):
            capi.supersample_camera(cam, s)
    assert lib.rt_supersample_camera(None, 2, C.byref(out)) == capi.RT_ERR_INVALID_ARG
    assert lib.rt_supersample_camera(C.byref(cam), 2, None) == capi.RT_ERR_INVALID_ARG
    wide = default_cam()
    wide.width = 2 ** 30
    assert lib.rt_supersample_camera(C.byref(wide), 2, C.byref(out)) == capi.RT_ERR_INVALID_ARG
    assert lib.rt_supersample_camera(C.byref(wide), 1, C.byref(out)) == capi.RT_OK
    tall = default_cam()
    tall.height = 2 ** 28
    assert lib.rt_supersample_camera(C.byref(tall), 8, C.byref(out)) == capi.RT_ERR_INVALID_ARG
    assert lib.rt_supersample_camera(C.byref(tall), 4, C.byref(out)) == capi.RT_OK


def test_set_option_value_3_is_invalid():
    """RT_ERR_INVALID_ARG for S = 3.  A context needs a device, so here the call has none (the
    status is the same); test_supersample_gpu.py repeats it on a live context, where values
    1, 2, 4 and 8 are accepted."""
    lib = capi.load()
    assert capi.RT_OPT_SUPERSAMPLE == 22
    assert lib.rt_set_option(None, capi.RT_OPT_SUPERSAMPLE, 3) == capi.RT_ERR_INVALID_ARG
    assert lib.rt_multi_set_option(None, capi.RT_OPT_SUPERSAMPLE, 3) == capi.RT_ERR_INVALID_ARG


def test_abi_version_is_unchanged():
    assert capi.load().rt_capi_version() == 2
