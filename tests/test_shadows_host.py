"""CPU-side checks of RT_FLAG_SHADOWS: the expected-result fixture (tests/shadow_fixture.py)
pinned to the oracle with the flag off, and the shadow content of the frames the GPU tests
use, computed from the fixture alone."""
import os

import numpy as np
import pytest

import shadow_fixture as sfx
from conftest import REPO
from rtamd import capi

FRAMES = ("A", "B", "L")


def test_flag_constant_and_header():
    assert capi.RT_FLAG_SHADOWS == 2
    text = open(os.path.join(REPO, "include", "rt_capi.h")).read()
    assert "RT_FLAG_SHADOWS = 1u << 1" in text


@pytest.mark.parametrize("name", ("A", "B"))
def test_fixture_without_shadows_equals_oracle_render(oracle, name):
    prims, cam, depth, tr = sfx.case(name, False)
    ref, _, _ = oracle.render(prims, cam, depth)
    err = float(np.abs(tr.rgb.reshape(ref.shape) - ref).max())
    print(f"fixture vs Oracle.render, camera {name}: max|d| = {err:.3e}")
    assert err <= 1e-14


def test_fixture_without_shadows_equals_oracle_trace(oracle):
    prims, o, d, depth, tr = sfx.ray_case(False)
    pick = np.linspace(0, len(o) - 1, 64).astype(int)
    err = 0.0
    for k in pick:
        rgb, _ = oracle.trace(prims, o[k], d[k], depth)
        err = max(err, float(np.abs(tr.rgb[k] - np.array(rgb)).max()))
    print(f"fixture vs Oracle.trace, 64 scaled rays: max|d| = {err:.3e}")
    assert err <= 1e-14


@pytest.mark.parametrize("name", FRAMES)
def test_frames_have_shadow_content(name):
    _, cam, _, off = sfx.case(name, False)
    _, _, _, on = sfx.case(name, True)
    npx = cam.width * cam.height
    differ = np.abs(on.rgb - off.rgb).max(axis=-1) > 1e-3
    sh = on.shadow.astype(bool)
    print(f"{name}: {differ.sum()}/{npx} pixels differ, per level shadowed/hits "
          f"{[(int(sh[:, k].sum()), int((on.hits[:, k] >= 0).sum())) for k in range(sh.shape[1])]}, "
          f"fragile {int(on.fragile.sum())}")
    assert np.array_equal(on.hits, off.hits)              # ray paths are untouched
    assert differ.mean() >= 0.05
    assert np.any(sh & ((on.blocker_kinds & 1) != 0))     # a sphere blocker
    assert np.any(sh & ((on.blocker_kinds & 2) != 0))     # a wall blocker
    assert sh[:, 1:].any()                                # a shadowed hit at a level >= 1
    assert on.fragile.mean() <= 0.005


def test_cameras_a_b_counts():
    """The shadow content of scene S as first measured (shadowed / hits per level)."""
    want = {"A": [(102, 599), (75, 208), (12, 77), (6, 17)],
            "B": [(114, 580), (102, 332), (24, 76), (9, 32)]}
    for name, rows in want.items():
        _, _, _, on = sfx.case(name, True)
        got = [(int(on.shadow[:, k].sum()), int((on.hits[:, k] >= 0).sum())) for k in range(4)]
        assert got == rows, (name, got)
        assert int(on.fragile.sum()) == 0
