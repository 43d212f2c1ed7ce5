"""Reader of tests/golden/views.npz (tests/golden/make_golden.py --only views): tilted walls
(normal.z != 0, un-normalised raw normals), rolled and z-looking cameras, non-default
materials — inputs and the reference's own outputs.  Everything a test needs comes from the
file; nothing here rebuilds a scene or a view from generator code.

  scenes   <scene>__prims  rt_prim records as bytes, <scene>__raw  [n, 3] raw normals
  views    <view>__args    position, lookat, vup, vfov, aspect_ratio, image_width (12 doubles)
           <view>__refcam  the reference's Camera::init: position, image_top_left,
                           pixel_delta_x, pixel_delta_y (12 doubles); <view>__height
  frames   frame__<scene>__<view>__d<depth>  [H, W, 3] fp64, recursive_ray_tracing
  rays     <scene>__ray_{o,d,depth,rgb}, <scene>__ray_hit_{index,dist,normal}
  walls    wallkat__{name,position,raw_normal,length,width,o,d,dist,normal,hit}
"""
import ctypes as C
import os

import numpy as np

from boxes_check import decode  # noqa: F401  (depth <= 2 signature -> hit index per segment)
from conftest import GOLDEN
from rtamd import capi



class Views:
    def __init__(self):
        self.z = np.load(os.path.join(GOLDEN, "views.npz"))
        self.scene_names = [str(s) for s in self.z["scene_names"]]
        self.view_names = [str(v) for v in self.z["view_names"]]
        # (key, scene, view, depth) of every frame, in file order
        self.frames = []
        for key in self.z.files:
            if key.startswith("frame__"):
                _, scene, view, depth = key.split("__")
                self.frames.append((key, scene, view, int(depth[1:])))
        self._prims = {}

    def prims(self, scene):
        """The scene's rt_prim records (normals as the Wall constructor normalised them)."""
        if scene not in self._prims:
            raw = self.z[f"{scene}__prims"].tobytes()
            n = len(raw) // C.sizeof(capi.rt_prim)
            assert n * C.sizeof(capi.rt_prim) == len(raw)
            arr = (capi.rt_prim * n).from_buffer_copy(raw)
            self._prims[scene] = [arr[i] for i in range(n)]
        return self._prims[scene]

    def raw_normals(self, scene):
        return self.z[f"{scene}__raw"]

    def cam_args(self, view, width=None):
        """camera_init's keyword arguments; width rescales image_width (same aspect)."""
        a = self.z[f"{view}__args"]
        return dict(position=tuple(a[0:3]), lookat=tuple(a[3:6]), vup=tuple(a[6:9]),
                    vfov=float(a[9]), aspect_ratio=float(a[10]),
                    image_width=float(a[11] if width is None else width))

    def camera(self, view, width=None):
        return capi.camera_init(**self.cam_args(view, width))

    def views_of(self, scene):
        return sorted({v for _, s, v, _ in self.frames if s == scene})

    def tilted_walls(self, scene, lo=0.2, hi=0.95):
        """Scene indices of the walls with lo <= |normal.z| <= hi."""
        return [j for j, p in enumerate(self.prims(scene))
                if p.kind == capi.RT_PRIM_WALL and lo <= abs(p.normal[2]) <= hi]

    def z_walls(self, scene):
        """Scene indices of the walls with any z in their normal (the near-z wall included)."""
        return [j for j, p in enumerate(self.prims(scene))
                if p.kind == capi.RT_PRIM_WALL and p.normal[2] != 0.0]

    def rays(self, scene):
        g = lambda k: self.z[f"{scene}__ray_{k}"]  # noqa: E731
        hits = np.zeros(len(g("o")), capi.HIT_DTYPE)
        hits["index"], hits["distance"], hits["normal"] = g("hit_index"), g("hit_dist"), g("hit_normal")
        return dict(o=g("o"), d=g("d"), depth=g("depth").astype(np.int64), rgb=g("rgb"), hits=hits)


def int_exp(prims):
    """rt_scene_pack.cpp pack_scene: every specular exponent an integer in [0, 1024] selects the
    integer-pow kernels, anything else the general-pow ones."""
    return all(0.0 <= p.mat.specular_exponent <= 1024.0 and
               p.mat.specular_exponent == np.floor(p.mat.specular_exponent) for p in prims)


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
