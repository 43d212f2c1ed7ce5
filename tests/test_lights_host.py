"""CPU-side checks of scene lights (rt_set_lights): the constants and the header, the
expected-result fixture (tests/lights_fixture.py) pinned to the oracle and to shadow_fixture with
the reference's light, and the content of the frames the GPU tests use, computed from the
fixture alone (counts as first measured)."""
import ctypes as C
import os

import numpy as np
import pytest

import lights_fixture as lfx
import shadow_fixture as sfx
from conftest import REPO
from rtamd import capi


def test_constants_struct_and_header():
    assert capi.RT_MAX_LIGHTS == 8
    assert C.sizeof(capi.rt_light) == 48
    assert capi.rt_light.position.offset == 0 and capi.rt_light.color.offset == 24
    text = open(os.path.join(REPO, "include", "rt_capi.h")).read()
    assert "#define RT_MAX_LIGHTS 8" in text
    assert "#define RT_CAPI_VERSION 2" in text          # additive: the version stays
    assert "int rt_set_lights(rt_ctx* ctx, const rt_light* lights, int32_t n);" in text
    assert "int rt_multi_set_lights(rt_multi* m, const rt_light* lights, int32_t n);" in text
    names = [s[0] for s in capi.SIGNATURES]
    assert "rt_set_lights" in names and "rt_multi_set_lights" in names
    arr, n = capi.light_array(lfx.K2)
    assert n == 2 and tuple(arr[1].position) == (6.0, 1.5, 3.0) and tuple(arr[0].color) == (1.0, .8, .6)
    assert capi.light_array([]) == (None, 0) and capi.light_array(None) == (None, 0)


@pytest.mark.parametrize("name", ("A", "B"))
def test_one_white_light_at_the_origin_is_the_reference(oracle, name):
    """ONE reproduces Oracle.render bitwise, and shadow_fixture bitwise with shadows on."""
    prims, cam, depth, tr = lfx.case(name, "ONE", False)
    ref, _, _ = oracle.render(prims, cam, depth)
    assert tr.rgb.reshape(ref.shape).tobytes() == ref.tobytes()
    _, _, _, on = lfx.case(name, "ONE", True)
    _, _, _, want = sfx.case(name, True)
    assert on.rgb.tobytes() == want.rgb.tobytes()
    assert np.array_equal(on.shadow[:, :, 0], want.shadow)
    assert np.array_equal(on.fragile, want.fragile)


LEVEL0 = {("A", "K4"): ([46, 33, 102, 141], 599),
          ("B", "K4"): ([4, 33, 114, 18], 580),
          ("L", "K2"): ([259, 441], 607)}


@pytest.mark.parametrize("name,lights", sorted(LEVEL0))
def test_shadowed_hits_per_light_at_level_0(name, lights):
    _, _, _, on = lfx.case(name, lights, True)
    got = [int(on.shadow[:, 0, l].sum()) for l in range(on.shadow.shape[2])]
    hits = int((on.hits[:, 0] >= 0).sum())
    print(f"{name} {lights}: shadowed per light at level 0 {got} of {hits}")
    assert (got, hits) == LEVEL0[(name, lights)]


@pytest.mark.parametrize("name", ("A", "B", "L"))
@pytest.mark.parametrize("lights", ("K2", "K4", "K8"))
def test_every_light_shadows_deeper_hits_and_no_ray_is_fragile(name, lights):
    _, cam, _, on = lfx.case(name, lights, True)
    deeper = on.shadow[:, 1:, :].reshape(-1, on.shadow.shape[2]).sum(axis=0)
    print(f"{name} {lights}: shadowed hits at levels >= 1 per light {deeper.tolist()}, "
          f"fragile {int(on.fragile.sum())}/{len(on.fragile)}")
    assert (deeper >= 1).all()
    assert on.fragile.mean() <= 0.005
    assert int(on.fragile.sum()) == 0          # as measured


def test_fragile_rays_of_the_other_gpu_inputs():
    for tr in (lfx.case("B13", "K4", True)[3], lfx.ray_case("K2", True)[4], lfx.ray_case("K4", True)[4]):
        assert tr.fragile.mean() <= 0.005
        assert int(tr.fragile.sum()) == 0      # as measured


@pytest.mark.parametrize("name,lights,floor", [("A", "K4", .10), ("B", "K4", .10), ("B13", "K4", .10),
                                               ("L", "K2", .30)])
def test_shadows_change_the_lit_frames(name, lights, floor):
    """Measured: 15.8%, 12.7%, 12.5% (K4 on A, B, B13) and 33.6% (K2 on L)."""
    _, _, _, on = lfx.case(name, lights, True)
    _, _, _, off = lfx.case(name, lights, False)
    assert np.array_equal(on.hits, off.hits)   # ray paths are untouched
    frac = float((np.abs(on.rgb - off.rgb).max(axis=-1) > 1e-3).mean())
    print(f"{name} {lights}: {100 * frac:.1f}% of the pixels differ between shadows on and off")
    assert frac >= floor


@pytest.mark.parametrize("name", ("A", "B"))
def test_k2_differs_from_the_default_light(name):
    """About 38% of the pixels (measured), everything that is not sky or ground."""
    _, _, _, k2 = lfx.case(name, "K2", False)
    _, _, _, one = sfx.case(name, False)
    frac = float((np.abs(k2.rgb - one.rgb).max(axis=-1) > 1e-3).mean())
    print(f"{name}: {100 * frac:.1f}% of the pixels differ between K2 and the default light")
    assert 0.33 <= frac <= 0.43


def test_k8_on_a_exceeds_one():
    """K8 on A reaches 1.43 (the shadowed depth-3 frame, as measured; 1.45 unshadowed, 2.35 at
    depth 0): RGBA8's saturation and RGBA8_WRAP's wrap are exercised by the depth-0 frames of
    the GPU test."""
    for sh in (False, True):
        top = float(lfx.case("A", "K8", sh, depth=0)[3].rgb.max())
        print(f"A K8 depth 0, shadows {sh}: max = {top:.4f}")
        assert top > 1.0 + 1.0 / 255.0
    top = float(lfx.case("A", "K8", True)[3].rgb.max())
    print(f"A K8 depth 3, shadowed: max = {top:.4f}")
    assert abs(top - 1.43) < 0.005
