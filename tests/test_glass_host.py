"""CPU-side checks of transmission records (rt_set_transmission): the struct, the header and the
bindings, what the entry points refuse without a ctx, and the expected-result fixture
(tests/glass_fixture.py): its invariants on the frames the GPU tests use, and that with every
tau == 0 it is lights_fixture.trace bit for bit.

A ctx needs a device, so the refusals that must leave the previous records in force, the two ways
of clearing and rt_set_scene's clearing are checked where a ctx exists: test_glass_gpu.py
(test_invalid_arguments_keep_the_previous_records, test_clearing_restores_the_plain_kernels,
test_set_scene_clears_the_records)."""
import ctypes as C
import os

import numpy as np
import pytest

import glass_fixture as gfx
import lights_fixture as lfx
import shadow_fixture as sfx
from conftest import REPO
from rtamd import capi


def test_struct_header_and_bindings():
    assert C.sizeof(capi.rt_transmission) == 16
    assert capi.rt_transmission.transmission.offset == 0 and capi.rt_transmission.ior.offset == 8
    text = open(os.path.join(REPO, "include", "rt_capi.h")).read()
    assert "#define RT_CAPI_VERSION 2" in text          # additive: the version stays
    assert "int rt_set_transmission(rt_ctx* ctx, const rt_transmission* recs, int32_t n);" in text
    assert "int rt_multi_set_transmission(rt_multi* m, const rt_transmission* recs, int32_t n);" in text
    names = [s[0] for s in capi.SIGNATURES]
    assert "rt_set_transmission" in names and "rt_multi_set_transmission" in names
    assert callable(capi.Renderer.set_transmission) and callable(capi.MultiRenderer.set_transmission)
    arr, n = capi.transmission_array(gfx.TRANS_G)
    assert n == 9 and (arr[0].transmission, arr[0].ior) == (.9, 1.5)
    assert (arr[2].transmission, arr[2].ior) == (0.0, 1.0) and (arr[8].transmission, arr[8].ior) == (.6, 1.0)
    assert capi.transmission_array([]) == (None, 0) and capi.transmission_array(None) == (None, 0)


def test_library_exports_and_null_handles():
    lib = capi.load()
    arr, n = capi.transmission_array(gfx.TRANS_G)
    for args in ((arr, n), (None, 0)):
        assert lib.rt_set_transmission(None, *args) == capi.RT_ERR_INVALID_ARG
        assert lib.rt_multi_set_transmission(None, *args) == capi.RT_ERR_INVALID_ARG


def test_scene_g_coverage():
    """Measured with this fixture at CAM_A, 48x32, depth 3: 18.1% of the primary rays hit a glass
    sphere, 29.7% the pane, 7.0% of the rays pass two or more transmissive objects; 386 sphere
    and 456 pane passages; k2 >= 6.8e-4; | |d'| - 1 | <= 4.5e-16."""
    prims, trans, cam, depth, tr = gfx.case("G")
    sph, pane, multi = gfx.coverage(tr, prims, trans)
    print(f"G: glass sphere {100 * sph:.1f}%, pane {100 * pane:.1f}%, >= 2 passages {100 * multi:.1f}%; "
          f"{int(tr.sphere_pass.sum())} sphere and {int(tr.pane_pass.sum())} pane passages, "
          f"k2 min {tr.k2_min:.3e}, | |d'| - 1 | max {tr.dnorm_max:.3e}")
    assert sph >= .15 and pane >= .25 and multi >= .05
    assert (int(tr.sphere_pass.sum()), int(tr.pane_pass.sum())) == (386, 456)     # as measured
    assert tr.k2_min > 0                       # the exit clamp never acts on these frames
    assert tr.dnorm_max <= 7e-16
    assert (tr.passes == tr.sphere_pass + tr.pane_pass).all()


def test_scene_l_passages_and_change():
    """L at camera B, depth 6: 150 sphere and 496 pane passages; 28% of the pixels differ from
    the opaque frame by more than 1e-6 (as measured)."""
    _, _, _, _, tr = gfx.case("L")
    _, _, _, _, op = gfx.case("L", glass=False)
    frac = float((np.abs(tr.rgb - op.rgb).max(axis=-1) > 1e-6).mean())
    print(f"L: {int(tr.sphere_pass.sum())} sphere and {int(tr.pane_pass.sum())} pane passages, "
          f"{100 * frac:.1f}% of the pixels differ from the opaque frame")
    assert (int(tr.sphere_pass.sum()), int(tr.pane_pass.sum())) == (150, 496)
    assert .25 <= frac <= .31
    assert tr.k2_min > 0


@pytest.mark.parametrize("name", ("G13", "SA", "SB"))
def test_every_gpu_frame_has_passages(name):
    _, _, _, _, tr = gfx.case(name)
    print(f"{name}: {int(tr.sphere_pass.sum())} sphere and {int(tr.pane_pass.sum())} pane passages")
    assert tr.sphere_pass.sum() > 0 and tr.pane_pass.sum() > 0 and tr.k2_min > 0


def test_ray_case_reaches_glass_after_an_opaque_bounce():
    """The scaled rays of CAM_A on G: |d| in [0.25, 4], so pos (main.cpp:99) lies off the surface
    and differs from the true P; at least one ray enters a glass sphere after an opaque bounce."""
    _, _, o, d, _, tr = gfx.ray_case()
    ln = np.sqrt((d * d).sum(axis=-1))
    _, _, cam, _, _ = gfx.case("G")
    _, d0 = sfx.camera_rays(cam)
    f = ln / np.sqrt((d0 * d0).sum(axis=-1))
    assert f.min() >= .25 - 1e-12 and f.max() <= 4 + 1e-12 and f.min() < .3 and f.max() > 3.5
    print(f"scaled rays: {int(tr.after_bounce.sum())} enter a glass sphere after an opaque bounce")
    assert tr.after_bounce.sum() >= 1
    assert tr.sphere_pass.sum() > 0 and tr.pane_pass.sum() > 0


def test_fragile_rays_of_the_gpu_inputs():
    for tr in (gfx.case("G", "K4", True)[4], gfx.case("L", "K4", True)[4], gfx.ray_case("K4", True)[5]):
        print(f"fragile {int(tr.fragile.sum())}/{len(tr.fragile)}")
        assert tr.fragile.mean() <= 0.005


@pytest.mark.parametrize("name,lights,shadows", [("G", "NONE", False), ("G", "K4", True), ("SB", "K4", True),
                                                 ("L", "NONE", False)])
def test_all_opaque_is_lights_fixture_bit_for_bit(oracle, name, lights, shadows):
    prims, trans, cam, depth, tr = gfx.case(name, lights, shadows, glass=False)
    o, d = sfx.camera_rays(cam)
    want = lfx.trace(oracle, prims, o, d, depth, gfx.LIGHTS[lights], shadows)
    assert tr.rgb.tobytes() == want.rgb.tobytes()
    assert np.array_equal(tr.hits, want.hits) and np.array_equal(tr.shadow, want.shadow)
    assert np.array_equal(tr.fragile, want.fragile) and tr.passes.sum() == 0
    # explicit zero records are the same as none
    zero = gfx.trace(oracle, prims, o, d, depth, gfx.LIGHTS[lights], shadows, [(0.0, 2.0)] * len(prims))
    assert zero.rgb.tobytes() == want.rgb.tobytes()
    # and the records change the frame
    assert gfx.case(name, lights, shadows)[4].rgb.tobytes() != want.rgb.tobytes()


def test_no_lights_is_the_oracle_when_opaque(oracle):
    prims, _, cam, depth, tr = gfx.case("G", glass=False)
    ref, _, _ = oracle.render(prims, cam, depth)
    assert tr.rgb.reshape(ref.shape).tobytes() == ref.tobytes()
