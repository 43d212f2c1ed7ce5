"""The property the tile bins' host half must have (rt_frame_boxes, rt_frame_args.cpp frame_boxes),
checked against the oracle: every pixel whose path hits primitive j on its primary segment
lies inside j's primary pixel box; every pixel whose primary ray hit wall w (and whose first
bounce off it hit j) lies inside j's box for the camera mirrored in w; likewise for two-wall
chains.  Shared by test_bins_host.py and test_views_host.py.  No device is used."""
import math

from rtamd import capi

B = 1000003  # rt_oracle.c path signature: sig = sig * B + (scene index + 1) per segment


def _slots(prims):
    """scene index -> material slot (spheres in order, then walls that can ever be hit)."""
    sph = [j for j, o in enumerate(prims) if o.kind == capi.RT_PRIM_SPHERE]
    wal = []
    for j, o in enumerate(prims):
        if o.kind != capi.RT_PRIM_WALL:
            continue
        n = tuple(o.normal)   # as the Wall constructor normalised it (scenes.to_prims)
        cz = (n[1], -n[0], 0.0)  # cross(n, z)
        if math.isnan(n[0]) or (cz[0] == 0.0 and cz[1] == 0.0):
            continue  # NaN basis: never hit, not uploaded
        wal.append(j)
    m = {j: s for s, j in enumerate(sph)}
    m.update({j: len(sph) + w for w, j in enumerate(wal)})
    return m, len(sph), len(wal)


def decode(sig):
    """path signature -> list of scene indices (-1 = miss) per segment (<= 3 segments)."""
    sig = int(sig)
    digits = []
    while True:
        digits.append(sig % B)
        sig //= B
        if sig == 0:
            break
    return [d - 1 for d in reversed(digits)]


def _inside(box, x, i):
    return box[0] <= x <= box[1] and box[2] <= i <= box[3]


def check_boxes(oracle, prims, cam, row0=0, nrows=None):
    """-> (primary boxes, [pixels checked at the primary level, mirror level 1, level 2])"""
    if nrows is None:
        nrows = cam.height - row0
    prim_boxes, mir, depth = capi.frame_boxes(prims, cam, row0, nrows)
    slot, nS, nW = _slots(prims)
    np_ = nS + nW
    assert len(prim_boxes) == np_
    _, _, _, sig = oracle.render(prims, cam, 2, row0=row0, nrows=nrows, want64=False,
                                 want_sig=True)
    lvl1 = mir[:nW * np_].reshape(nW, np_, 4) if depth >= 1 else None
    lvl2 = mir[nW * np_:nW * np_ + nW * nW * np_].reshape(nW, nW, np_, 4) if depth >= 2 else None
    checked = [0, 0, 0]
    for r in range(nrows):
        i = row0 + r
        for x in range(cam.width):
            path = decode(sig[r, x])
            if path[0] < 0:
                continue
            s0 = slot[path[0]]
            assert _inside(prim_boxes[s0], x, i), ("primary", x, i, s0, prim_boxes[s0])
            checked[0] += 1
            if len(path) < 2 or path[1] < 0 or s0 < nS or lvl1 is None:
                continue
            w1, s1 = s0 - nS, slot[path[1]]
            assert _inside(lvl1[w1, s1], x, i), ("bounce 1", x, i, w1, s1, lvl1[w1, s1])
            checked[1] += 1
            if len(path) < 3 or path[2] < 0 or s1 < nS or lvl2 is None:
                continue
            w2, s2 = s1 - nS, slot[path[2]]
            assert _inside(lvl2[w1, w2, s2], x, i), ("bounce 2", x, i, w1, w2, s2)
            checked[2] += 1
    return prim_boxes, checked


def check_wall_boxes(oracle, prims, cam):
    """Scenes past the linear scan's 64 primitives take the wave-cull kernels, which keep the
    cone for their spheres and give only their walls pixel boxes (frame_boxes, `cull_walls`).
    rt_frame_boxes reports no boxes for such a scene, but boxes_for computes a wall's box from
    that wall and the camera alone, so the boxes of the walls-only scene are the ones those
    kernels get: every pixel whose primary segment hits wall j in the WHOLE scene must lie
    inside them.  -> pixels checked"""
    walls = [j for j, o in enumerate(prims) if o.kind == capi.RT_PRIM_WALL]
    sub = [prims[j] for j in walls]
    boxes, _, _ = capi.frame_boxes(sub, cam)
    slot, nS, nW = _slots(sub)
    assert nS == 0 and len(boxes) == nW
    _, _, _, sig = oracle.render(prims, cam, 0, want64=False, want_sig=True)
    checked = 0
    for i in range(cam.height):
        for x in range(cam.width):
            j = decode(sig[i, x])[0]
            if j in walls:
                s = slot[walls.index(j)]
                assert _inside(boxes[s], x, i), ("primary", x, i, j, boxes[s])
                checked += 1
    return checked
