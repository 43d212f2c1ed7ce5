"""Expected ambient occlusion frames (rt_render_ao), shared by the test_ao_* files.

The expectation uses the oracle's exports and numpy only.  Pixel (i, j)'s record is
aov_fixture.closest_hits' (the oracle's find_closest_hit on shadow_fixture.camera_rays); from
it, in numpy fp64 with one IEEE operation per written operation and dot products summed left to
right:

  P    wall: o + d * distance;  sphere: o + d * projection (occluded_fixture.sphere_projection,
       scene.cpp:75's intersection_point)
  f    dot(d, n), n the record's un-normalised normal;  nf = -n where f > 0, else n
  sp   P + nf * .0001
  s_k  dot(w_k, nf);  w = -w_k where s_k < 0, else w_k (s_k == 0 is not flipped)

and probe k is occluded iff occluded_fixture's accepted parameters of (sp, w) hold one <= the
radius.  count = the occluded probes; ao = float32((K - count) / K); a miss has 0 and 1.
"""
import functools

import numpy as np

import aov_fixture as afx
import occluded_fixture as ofx
from rtamd import capi

# The radii of the GPU tests: a short world distance and no limit.  (At 0.75 only 3.2% of the hit
# pixels of cases A and views have 0 < count < K and views has no sphere blocker: the coverage
# condition of test_ao_host.py fails, so the short radius is 1.5.)
RADII = (1.5, np.inf)


def ao_of(count, k):
    """The ao layer of a count layer: one cast of the exact fp64 quotient."""
    return ((k - count.astype(np.float64)) / np.float64(k)).astype(np.float32)


def surface(prims, hits, o, d):
    """(P, n) for the hit rays: the true point each ray sees and the record's normal."""
    n = hits["normal"].copy()
    t = hits["distance"].copy()   # a wall's distance is its parameter (scene.cpp:10)
    for j, prim in enumerate(prims):
        if prim.kind == capi.RT_PRIM_WALL:
            continue
        m = hits["index"] == j
        if m.any():
            t[m] = ofx.sphere_projection(prim, o[m], d[m])[0]
    return o + d * t[:, None], n


def probes(P, n, d, dirs):
    """-> (sp [m, 3], w [m, K, 3], f [m], s [m, K]) of m hit rays and K directions."""
    f = ofx._dot(d, n)
    nf = np.where((f > 0)[:, None], -n, n)
    sp = P + nf * .0001
    s = (dirs[None, :, 0] * nf[:, None, 0] + dirs[None, :, 1] * nf[:, None, 1]) + dirs[None, :, 2] * nf[:, None, 2]
    w = np.where((s < 0)[:, :, None], -dirs[None, :, :], dirs[None, :, :])
    return sp, w, f, s


class Expected:
    """One (scene, camera, direction set): everything but the radius.

    aov       aov_fixture.expected's layers (index, kind, hit, ...), [H, W]
    hitmask   [H, W] bool, pixels with a primary hit; m = their number, in row-major order
    sp, w     [m, 3] and [m, K, 3]: probe origins and flipped directions
    f, s      [m] and [m, K]
    T         [m, K, nprims] accepted parameter of every probe against every primitive, else NaN
    degenerate  [H, W] bool: some s == 0 or f == 0 (the flips are decided by a zero's sign)
    """

    def __init__(self, orc, prims, cam, dirs):
        self.prims, self.cam = prims, cam
        self.dirs = np.ascontiguousarray(dirs, np.float64).reshape(-1, 3)
        self.K = len(self.dirs)
        H, W = cam.height, cam.width
        o, d = afx.sfx.camera_rays(cam)
        self.aov = afx.expected(orc, prims, cam)
        hits = self.aov["hit"].reshape(-1)
        hm = hits["index"] >= 0
        self.hitmask = hm.reshape(H, W)
        P, n = surface(prims, hits[hm], o[hm], d[hm])
        self.sp, self.w, self.f, self.s = probes(P, n, d[hm], self.dirs)
        m = int(hm.sum())
        spk = np.repeat(self.sp, self.K, axis=0)
        self.T = ofx.expected_params(orc, prims, spk, self.w.reshape(-1, 3)).reshape(m, self.K, len(prims))
        deg = np.zeros(H * W, bool)
        deg[hm] = (self.f == 0) | (self.s == 0).any(axis=1)
        self.degenerate = deg.reshape(H, W)
        self.is_wall = np.array([p.kind == capi.RT_PRIM_WALL for p in prims], bool)

    def blocked(self, radius):
        """[m, K] uint8: probe k of hit pixel q is occluded within radius."""
        return ofx.expected_occluded(self.T.reshape(-1, len(self.prims)), radius).reshape(-1, self.K)

    def count(self, radius):
        """The count layer, uint8 [H, W]."""
        c = np.zeros(self.hitmask.shape, np.uint8)
        c[self.hitmask] = self.blocked(radius).sum(axis=1).astype(np.uint8)
        return c

    def layers(self, radius):
        c = self.count(radius)
        return {"count": c, "ao": ao_of(c, self.K)}

    def coverage(self, radius):
        """What the case exercises at this radius: the histogram of count over the hit pixels,
        the fraction of them with 0 < count < K, pixels with a sphere / a wall among their
        blockers, and walls seen from behind (f > 0)."""
        with np.errstate(invalid="ignore"):
            blk = self.T <= np.float64(radius)                       # [m, K, nprims]
        c = self.count(radius)[self.hitmask]
        wall_hit = self.aov["kind"][self.hitmask] == 1
        return dict(hist=np.bincount(c, minlength=self.K + 1),
                    partial=float(((c > 0) & (c < self.K)).mean()) if len(c) else 0.0,
                    sphere_blockers=int(blk[:, :, ~self.is_wall].any(axis=(1, 2)).sum()),
                    wall_blockers=int(blk[:, :, self.is_wall].any(axis=(1, 2)).sum()),
                    behind=int((wall_hit & (self.f > 0)).sum()))


def build(prims, cam, dirs):
    import oracle as orc_mod
    return Expected(orc_mod.Oracle(), prims, cam, dirs)


@functools.lru_cache(maxsize=None)
def case(name, k=16):
    """-> Expected of a named case (aov_fixture.case's names) with the helper's k directions,
    computed once per process; read only."""
    prims, cam, _ = afx.case(name)
    return build(prims, cam, capi.ao_directions(k))


# (case, K) of the GPU tests' fixture comparisons; each at both RADII
GPU_CASES = (("A", 16), ("L", 16), ("views", 16), ("B13", 64))


def random_dirs(k, seed):
    """Seeded directions with lengths in [0.25, 4]."""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(k, 3))
    v /= np.linalg.norm(v, axis=1)[:, None]
    return v * rng.uniform(0.25, 4.0, size=k)[:, None]
