"""CPU checks on tests/golden/views.npz — tilted walls (normal.z != 0, un-normalised raw
normals), rolled and z-looking cameras, non-default materials — recorded from the reference's
own compiled code (tests/golden/make_golden.py --only views):

  * the oracle equals the fixture bitwise (frames, single rays, hit records, Wall::intersect),
    the bar of test_oracle_golden.py, so the GPU tests may use it on this ground;
  * oracle.camera_init and capi.camera_init equal the reference's Camera::init bitwise;
  * the host pixel boxes (rt_frame_boxes) stay conservative under roll, z-looking cameras and
    tilted walls (test_bins_host.py's property, boxes_check.py);
  * the fixture is what it says and exercises what it is for (every condition here is on the
    fixture's inputs and the oracle's hit paths, none on the code under test).

No device is used."""
import os

import numpy as np
import pytest

from boxes_check import check_boxes, check_wall_boxes
from conftest import GOLDEN
from rtamd import capi, scenes
from views_fixture import Views, decode, int_exp


@pytest.fixture(scope="module")
def views():
    return Views()


@pytest.fixture(scope="module")
def paths(views, oracle):
    """{(scene, view): [H, W] lists of the scene index hit on each of the first three segments}
    from the oracle's depth-2 path signatures; computed once, read only."""
    out = {}
    for _, scene, view, _ in views.frames:
        if (scene, view) in out:
            continue
        cam = oracle.camera_init(**views.cam_args(view))
        _, _, _, sig = oracle.render(views.prims(scene), cam, 2, want64=False, want_sig=True)
        out[(scene, view)] = [[decode(s) for s in row] for row in sig]
    return out


def _same(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and (np.array_equal(a.view(np.uint64), b.view(np.uint64)) or
                                   np.array_equal(a, b))


def _v(p, name):
    return np.array(getattr(p, name)[:])


# ---------------------------------------------------------------- the fixture is what it says
def test_fixture_contents(views):
    assert os.path.getsize(os.path.join(GOLDEN, "views.npz")) < 400 * 1000
    assert views.scene_names == ["tilt", "tilt_mat", "tilt_wild", "cloud"]
    assert len(views.frames) >= 12
    for key, _, view, _ in views.frames:
        h, w, _ = views.z[key].shape
        assert w <= 48 and h <= 48 and h == int(views.z[f"{view}__height"]), key
    assert {d for _, s, _, d in views.frames if s == "tilt"} == {0, 5}
    assert set(views.views_of("tilt")) == {"rolled", "up", "down", "wide", "narrow", "inside"}
    for s in ("tilt_mat", "tilt_wild", "cloud"):
        assert len(views.views_of(s)) == 2, s
    # the stored records hold the Wall constructor's normalisation of the stored raw normals
    for s in views.scene_names:
        for p, raw in zip(views.prims(s), views.raw_normals(s)):
            if p.kind == capi.RT_PRIM_WALL:
                assert _same(p.normal[:], scenes.normalize3(raw)), s
    # tilt: 6 spheres, 3 table walls, >= 5 tilted walls, two facing each other, one near z
    prims, raw = views.prims("tilt"), views.raw_normals("tilt")
    assert sum(p.kind == capi.RT_PRIM_SPHERE for p in prims) == 6
    assert sum(p.kind == capi.RT_PRIM_WALL and p.normal[2] == 0.0 for p in prims) == 3
    tilted = views.tilted_walls("tilt")
    assert len(tilted) >= 5
    for j in tilted:
        assert abs(np.linalg.norm(raw[j]) - 1.0) > 0.05 and prims[j].length != prims[j].width, j
    facing = min(float(np.dot(_v(prims[a], "normal"), _v(prims[b], "normal")))
                 for a in tilted for b in tilted)
    assert facing < -0.8
    assert any(tuple(r) == (0.02, 0.01, -1.0) for r in raw)
    # views: a rolled off-origin camera, up along +z, down along -z at width 37, vfov 150 at
    # aspect 0.5, vfov 5, a camera inside a sphere (rays leave along position - lookat)
    a = {v: views.z[f"{v}__args"] for v in views.view_names}
    assert tuple(a["rolled"][6:9]) == (0.3, 0.2, -1.0) and np.abs(a["rolled"][0:3]).min() > 0
    assert tuple(a["up"][0:3] - a["up"][3:6]) == (0.0, 0.0, 1.0) and tuple(a["up"][6:9]) == (0, -1, 0)
    assert tuple(a["down"][0:3] - a["down"][3:6]) == (0.0, 0.0, -1.0)
    assert tuple(a["down"][6:9]) == (1, 0, 0) and a["down"][11] == 37
    assert a["wide"][9] == 150 and a["wide"][10] == 0.5 and a["narrow"][9] == 5
    assert any(p.kind == capi.RT_PRIM_SPHERE and
               np.linalg.norm(a["inside"][0:3] - _v(p, "position")) < 0.5 * p.radius for p in prims)
    widths = {int(a[v][11]) for v in views.view_names}
    assert any(w % 8 for w in widths) and any(w % 2 for w in widths)          # ragged
    # the same geometry under all three material sets
    for s in ("tilt_mat", "tilt_wild"):
        for p, q in zip(prims, views.prims(s)):
            assert (p.kind, p.position[:], p.normal[:], p.radius, p.length, p.width) == \
                   (q.kind, q.position[:], q.normal[:], q.radius, q.length, q.width)
    # cloud: synthetic_scene(64, 6) + 4 tilted walls, cameras inside the sphere cloud
    cp = views.prims("cloud")
    sph = np.array([p.position[:] for p in cp if p.kind == capi.RT_PRIM_SPHERE])
    assert len(sph) == 64 and len(cp) == 74 and len(views.tilted_walls("cloud")) == 4
    for v in views.views_of("cloud"):
        pos = a[v][0:3]
        assert (pos > sph.min(axis=0) + 1).all() and (pos < sph.max(axis=0) - 1).all(), v


def test_fixture_materials(views):
    get = lambda s, f: {getattr(p.mat, f) for p in views.prims(s)}  # noqa: E731
    for f, dflt in (("ambient", .1), ("diffuse", .9), ("specular", .4), ("specular_exponent", 50.0)):
        assert get("tilt", f) == {dflt} and get("cloud", f) == {dflt}
    assert get("tilt_mat", "ambient") == {0, .1, .3}
    assert get("tilt_mat", "diffuse") == {0, .5, .9}
    assert get("tilt_mat", "specular") == {0, .4, 1}
    assert get("tilt_mat", "specular_exponent") == {1, 2, 7, 50, 200}
    assert get("tilt_mat", "metallic") == {0, .25, .9, 1}
    cols = {c for p in views.prims("tilt_mat") for c in p.mat.color[:]}
    assert {0.0, 1.0} <= cols and min(cols) >= 0 and max(cols) <= 1
    for p in views.prims("tilt_mat"):
        assert p.mat.ambient + p.mat.diffuse + p.mat.specular <= 1.4 + 1e-12
    assert get("tilt_wild", "metallic") == {0, 1, 1.5, -0.25}
    assert get("tilt_wild", "specular_exponent") == {0, 1024, 1025, 0.5, 37.5}
    assert -0.1 in get("tilt_wild", "ambient") and 2.0 in get("tilt_wild", "specular")
    assert 2.0 in {c for p in views.prims("tilt_wild") for c in p.mat.color[:]}
    # which pow kernels each scene selects
    assert [int_exp(views.prims(s)) for s in views.scene_names] == [True, True, False, True]


# ---------------------------------------------------------------- oracle == reference, bitwise
def test_oracle_frames_bit_exact(views, oracle):
    for key, scene, view, depth in views.frames:
        cam = oracle.camera_init(**views.cam_args(view))
        o64, _, _ = oracle.render(views.prims(scene), cam, depth, nthreads=4)
        assert _same(o64, views.z[key]), key


def test_oracle_rays_and_hits_bit_exact(views, oracle):
    for scene in views.scene_names:
        prims, r = views.prims(scene), views.rays(scene)
        assert len(r["o"]) == 300 and set(np.unique(r["depth"])) == set(range(9))
        for k in range(len(r["o"])):
            got, _ = oracle.trace(prims, r["o"][k], r["d"][k], int(r["depth"][k]))
            assert _same(got, r["rgb"][k]), (scene, k)
            idx, dist, nrm = oracle.find_closest_hit(prims, r["o"][k], r["d"][k])
            h = r["hits"][k]
            assert idx == h["index"] and _same(dist, h["distance"]) and _same(nrm, h["normal"]), \
                (scene, k)


def test_wall_intersect_known_answers(views, oracle):
    z = views.z
    names = [str(n) for n in z["wallkat__name"]]
    assert len(names) >= 8
    by = {}
    for k, name in enumerate(names):
        w = scenes.to_prims([scenes.Wall(scenes.Material((1, 1, 1)), z["wallkat__position"][k],
                                         z["wallkat__raw_normal"][k], float(z["wallkat__length"][k]),
                                         float(z["wallkat__width"][k]))])[0]
        assert w.normal[2] != 0.0 and abs(np.linalg.norm(z["wallkat__raw_normal"][k]) - 1) > 1e-4
        dist, n, hit = oracle.wall_intersect(w, z["wallkat__o"][k], z["wallkat__d"][k])
        assert _same(dist, z["wallkat__dist"][k]), name
        assert _same(n, z["wallkat__normal"][k]), name
        assert hit == z["wallkat__hit"][k], name
        by[name] = (hit, dist, n, w)
    for w in ("w0", "w1"):
        for side in ("px0", "px1", "py0", "py1"):
            assert by[f"{w}_in_{side}"][0] == 1 and by[f"{w}_out_{side}"][0] == 0, (w, side)
        assert by[f"{w}_front"][0] == 1 and by[f"{w}_parallel"][0] == 0
        hit, _, n, prim = by[f"{w}_back_side"]
        assert hit == 1 and _same(n, prim.normal[:])        # the normal is not flipped
    assert by["near_z_from_above"][0] == 1 and by["near_z_from_below"][0] == 1
    assert by["near_z_outside"][0] == 0


# ---------------------------------------------------------------- cameras
def test_cameras_match_reference_bitwise(views, oracle):
    for v in views.view_names:
        ref, h = views.z[f"{v}__refcam"].reshape(4, 3), int(views.z[f"{v}__height"])
        for name, cam in (("oracle", oracle.camera_init(**views.cam_args(v))),
                          ("capi", capi.camera_init(**views.cam_args(v)))):
            assert cam.height == h and cam.width == int(views.z[f"{v}__args"][11]), (v, name)
            assert _same(cam.position[:], ref[0]), (v, name)
            assert _same(cam.image_top_left[:], ref[1]), (v, name)
            assert _same(cam.pixel_delta_x[:], ref[2]), (v, name)
            assert _same(cam.pixel_delta_y[:], ref[3]), (v, name)


# ---------------------------------------------------------------- the fixture exercises its ground
def test_fixture_is_meaningful(views, paths):
    """Conditions on the oracle's hit paths and the reference's hit records (ISSUE: adjust the
    view, never the condition): >= 10% of every view's pixels hit a primitive on the primary
    segment; every tilted wall of every scene is the hit primitive of >= 20 fixture pixels (any
    of the first three segments) or rays; >= 100 pixel paths bounce off one tilted wall onto
    another primitive; in every view of tilt some tilted wall is seen from behind."""
    bounce = 0
    for (scene, view), grid in paths.items():
        flat = [p for row in grid for p in row]
        assert np.mean([p[0] >= 0 for p in flat]) >= 0.10, (scene, view)
        tilted = set(views.z_walls(scene))
        bounce += sum(1 for p in flat if p[0] in tilted and len(p) > 1 and p[1] >= 0)
        if scene == "tilt":
            prims, pos = views.prims(scene), views.z[f"{view}__args"][0:3]
            behind = {j for j in tilted
                      if np.dot(_v(prims[j], "normal"), pos - _v(prims[j], "position")) < 0}
            assert sum(1 for p in flat if p[0] in behind) >= 20, (scene, view)
    assert bounce >= 100
    for scene in views.scene_names:
        hits = views.rays(scene)["hits"]["index"]
        for j in views.z_walls(scene):
            n = int((hits == j).sum())
            n += sum(1 for (s, _), grid in paths.items() if s == scene
                     for row in grid for p in row if j in p)
            assert n >= 20, (scene, j, n)


def test_general_pow_materials_are_reached(views, paths):
    """tilt_wild selects the general-pow kernels (int_exp false), and primitives whose exponent
    is not an integer in [0, 1024] are what fixture pixels and rays actually hit."""
    prims = views.prims("tilt_wild")
    assert not int_exp(prims)
    odd = {j for j, p in enumerate(prims) if not int_exp([p])}
    frac = {j for j in odd if prims[j].mat.specular_exponent != np.floor(prims[j].mat.specular_exponent)}
    px = sum(1 for (s, _), grid in paths.items() if s == "tilt_wild"
             for row in grid for p in row if p[0] in odd)
    pxf = sum(1 for (s, _), grid in paths.items() if s == "tilt_wild"
              for row in grid for p in row if p[0] in frac)
    rays = int(np.isin(views.rays("tilt_wild")["hits"]["index"], list(odd)).sum())
    assert px > 100 and pxf > 100 and rays > 20, (px, pxf, rays)


# ---------------------------------------------------------------- host pixel boxes
def test_boxes_conservative_on_fixture_views(views, oracle):
    """test_bins_host.py's property on every fixture view of tilt (17 primitives: primary boxes
    and the first mirror level; 11 walls leave no room for the second) and of cloud (past the
    linear scan's limit: the walls' boxes the wave-cull kernels use, boxes_check.py)."""
    total = [0, 0, 0]
    for view in views.views_of("tilt"):
        _, checked = check_boxes(oracle, views.prims("tilt"), views.camera(view))
        assert checked[0] > 0, view
        total = [a + b for a, b in zip(total, checked)]
    assert total[1] > 100, total
    for view in views.views_of("cloud"):
        assert check_wall_boxes(oracle, views.prims("cloud"), views.camera(view)) > 100, view


def test_mirror_levels_conservative_on_tilted_walls(views, oracle):
    """Both mirror levels under roll and along z: tilt's first two spheres with the two tilted
    walls that face each other, the overhead one and the near-z floor (6 primitives, 4 walls:
    two mirror levels fit)."""
    prims = views.prims("tilt")
    tilted = views.tilted_walls("tilt")
    near_z = [j for j in views.z_walls("tilt") if j not in tilted]
    sub = prims[:2] + [prims[j] for j in tilted[1:4] + near_z]
    total = [0, 0, 0]
    for view in views.views_of("tilt"):
        _, _, depth = capi.frame_boxes(sub, views.camera(view))
        assert depth >= 2
        _, checked = check_boxes(oracle, sub, views.camera(view))
        total = [a + b for a, b in zip(total, checked)]
    assert total[1] > 100 and total[2] > 100, total
