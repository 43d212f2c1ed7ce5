"""ctypes binding of include/rt_capi.h (the C-ABI drop-in boundary).

This is the binding a Python host would add; bench.py and the GPU parity tests drive the
HIP path through it.  The library is loaded from the in-tree build
(ray-tracer-from-scratch_amd/lib/librt_amd.so); a missing library raises — there is no
CPU fallback on the product path.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_DIR = os.path.join(PKG_DIR, "lib")
# RT_AMD_LIB: another build of the same C-ABI (the host sanitizer build of `make asan`)
LIB_PATH = os.environ.get("RT_AMD_LIB") or os.path.join(LIB_DIR, "librt_amd.so")
HOST_LIB_PATH = os.path.join(LIB_DIR, "librt_host.so")

# ---- enums (rt_capi.h) ----------------------------------------------------
RT_OK = 0
RT_ERR_INVALID_ARG = 1
RT_ERR_NO_DEVICE = 2
RT_ERR_HIP = 3
RT_ERR_OUT_OF_MEMORY = 4
RT_ERR_NO_SCENE = 5
RT_ERR_UNSUPPORTED = 6
RT_ERR_OUT_OF_RANGE = 7
RT_ERR_COMM = 8

RT_TRANSPORT_RCCL = 0
RT_TRANSPORT_COPY = 1
RT_TRANSPORT_RCCL_LOOPBACK = 2
RT_TRANSPORT_THREADS = 3   # rehearsal: one handle per rank in one process (include/rt_capi.h)
RT_TRANSPORT_IPC = 4       # rehearsal: one process per rank, shared-memory mailbox + HIP IPC
RT_MULTI_ID_BYTES = 128
RT_MULTI_SLOTS = 4
RT_MULTI_BATCH_MAX = 16

RT_PRIM_SPHERE = 0
RT_PRIM_WALL = 1

RT_PREC_F64 = 0
RT_PREC_F32 = 1
RT_PREC_MIXED = 2
RT_PREC_PATH64 = 3
PRECISIONS = {"f64": RT_PREC_F64, "f32": RT_PREC_F32, "mixed": RT_PREC_MIXED,
              "path64": RT_PREC_PATH64}

RT_OUT_RGB_F32 = 0
RT_OUT_RGB_F64 = 1
RT_OUT_RGBA8 = 2
RT_OUT_RGBA8_WRAP = 3

RT_FLAG_SUN = 1
RT_FLAG_SHADOWS = 2          # hard shadows: a ray to the light at every hit (F64, MIXED, PATH64)

RT_OPT_WAVE_CULL_MIN_SPHERES = 1
RT_OPT_STATS_DEVICE_PTR = 2
RT_OPT_EYE_TABLES = 3
RT_OPT_TILE_BINS = 4
RT_OPT_ROW_ORDER = 5
RT_OPT_MIRROR_BINS = 6
RT_OPT_BOX_CACHE = 7
RT_OPT_ROW_FEEDBACK = 8
RT_OPT_PIXEL_PAIRS = 9
RT_OPT_ROW_FEEDBACK_WARM = 10
RT_OPT_WALL_ORDER = 11
RT_OPT_CLUSTER_COS = 12
RT_OPT_MULTI_LAYOUT = 13
RT_OPT_HOST_PIPELINE = 16
RT_OPT_MULTI_FRAMES = 17
RT_OPT_MULTI_FAULT = 18
RT_OPT_MULTI_BATCH = 19
RT_OPT_MULTI_TIMEOUT_MS = 20
RT_OPT_FRAME_BATCH = 21
RT_OPT_SUPERSAMPLE = 22      # S in {1, 2, 4, 8}: S x S rays per pixel, mean stored (changes output)
RT_OPT_ROW_FEEDBACK_EMA = 14
RT_OPT_ROW_FEEDBACK_ISOLATE = 15
RT_OPT_ROW_MIX = 23          # 0 heaviest first, 1 mixed for frames in flight on streams, 2 mixed always
ROW_PERM_MAX = 2048          # dispatch units of a row order (rt_set_row_order, rt_order_units)
RT_MAX_LIGHTS = 8            # scene lights of rt_set_lights


class rt_material(C.Structure):
    _fields_ = [
        ("color", C.c_double * 3),
        ("ambient", C.c_double),
        ("metallic", C.c_double),
        ("diffuse", C.c_double),
        ("specular", C.c_double),
        ("specular_exponent", C.c_double),
    ]


class rt_prim(C.Structure):
    _fields_ = [
        ("kind", C.c_int32),
        ("reserved", C.c_int32),
        ("mat", rt_material),
        ("position", C.c_double * 3),
        ("normal", C.c_double * 3),
        ("radius", C.c_double),
        ("length", C.c_double),
        ("width", C.c_double),
    ]


class rt_camera(C.Structure):
    _fields_ = [
        ("position", C.c_double * 3),
        ("image_top_left", C.c_double * 3),
        ("pixel_delta_x", C.c_double * 3),
        ("pixel_delta_y", C.c_double * 3),
        ("width", C.c_int32),
        ("height", C.c_int32),
    ]


class rt_light(C.Structure):
    """A coloured point light of rt_set_lights (48 bytes)."""
    _fields_ = [("position", C.c_double * 3), ("color", C.c_double * 3)]


def light_array(lights):
    """lights as a ctypes array of rt_light: rt_light records, or (position, color) pairs of
    three numbers each.  None or an empty list gives (None, 0): the reference's light."""
    recs = []
    for l in lights or []:
        if not isinstance(l, rt_light):
            pos, col = l
            l = rt_light((C.c_double * 3)(*pos), (C.c_double * 3)(*col))
        recs.append(l)
    if not recs:
        return None, 0
    return (rt_light * len(recs))(*recs), len(recs)


class rt_transmission(C.Structure):
    """A transmission record of rt_set_transmission (16 bytes), one per scene object."""
    _fields_ = [("transmission", C.c_double), ("ior", C.c_double)]


def transmission_array(recs):
    """recs as a ctypes array of rt_transmission: rt_transmission records, (tau, ior) pairs, or
    a plain 0 for an opaque object (ior 1).  None or an empty list gives (None, 0): no records."""
    out = []
    for r in recs or []:
        if not isinstance(r, rt_transmission):
            tau, ior = (r, 1.0) if isinstance(r, (int, float)) else r
            r = rt_transmission(tau, ior)
        out.append(r)
    if not out:
        return None, 0
    return (rt_transmission * len(out))(*out), len(out)


class rt_stats(C.Structure):
    _fields_ = [("ms", C.c_double), ("segments", C.c_uint64)]


class rt_hit(C.Structure):
    """find_closest_hit's Collision as plain data (40 bytes); a miss is
    {DBL_MAX, (0, 0, 0), -1, 0}."""
    _fields_ = [("distance", C.c_double), ("normal", C.c_double * 3), ("index", C.c_int32),
                ("reserved", C.c_int32)]


# the same 40-byte layout as a numpy structured dtype (arrays of rt_hit records)
HIT_DTYPE = np.dtype([("distance", np.float64), ("normal", np.float64, (3,)),
                      ("index", np.int32), ("reserved", np.int32)])


class rt_aov_buffers(C.Structure):
    """The layers of rt_render_aov* (48 bytes); a NULL layer is not written."""
    _fields_ = [("hit", C.c_void_p), ("index", C.c_void_p), ("depth", C.c_void_p),
                ("normal", C.c_void_p), ("albedo", C.c_void_p), ("reserved", C.c_void_p)]


# the layers of a frame's AOVs: name -> (dtype, trailing shape), in rt_aov_buffers' order
AOV_LAYERS = {"hit": (HIT_DTYPE, ()), "index": (np.int32, ()), "depth": (np.float32, ()),
              "normal": (np.float32, (3,)), "albedo": (np.float32, (3,))}


RT_AO_MAX_DIRS = 64


class rt_ao_params(C.Structure):
    """The probes of rt_render_ao* (32 bytes): ndirs directions in HOST memory and the limit."""
    _fields_ = [("dirs", C.POINTER(C.c_double)), ("ndirs", C.c_int32), ("reserved", C.c_int32),
                ("radius", C.c_double), ("reserved2", C.c_void_p)]


class rt_ao_buffers(C.Structure):
    """The layers of rt_render_ao* (24 bytes); a NULL layer is not written."""
    _fields_ = [("count", C.c_void_p), ("ao", C.c_void_p), ("reserved", C.c_void_p)]


# the layers of an ambient occlusion frame: name -> dtype, in rt_ao_buffers' order
AO_LAYERS = {"count": np.uint8, "ao": np.float32}


# Every entry point include/rt_capi.h declares: (name, restype, argtypes).
_dbl3 = C.POINTER(C.c_double)
SIGNATURES = [
    ("rt_ctx_create", C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    ("rt_ctx_destroy", C.c_int, [C.c_void_p]),
    ("rt_strerror", C.c_char_p, [C.c_int]),
    ("rt_last_hip_error", C.c_char_p, [C.c_void_p]),
    ("rt_capi_version", C.c_int, []),
    ("rt_set_scene", C.c_int, [C.c_void_p, C.POINTER(rt_prim), C.c_int32]),
    ("rt_set_lights", C.c_int, [C.c_void_p, C.POINTER(rt_light), C.c_int32]),
    ("rt_set_transmission", C.c_int, [C.c_void_p, C.POINTER(rt_transmission), C.c_int32]),
    ("rt_set_option", C.c_int, [C.c_void_p, C.c_int32, C.c_int64]),
    ("rt_render", C.c_int,
     [C.c_void_p, C.POINTER(rt_camera), C.c_int32, C.c_int32, C.c_int32, C.c_int32,
      C.c_uint32, C.c_int32, C.c_void_p, C.c_int32, C.POINTER(rt_stats)]),
    ("rt_render_device", C.c_int,
     [C.c_void_p, C.POINTER(rt_camera), C.c_int32, C.c_int32, C.c_int32, C.c_int32,
      C.c_uint32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("rt_render_device_frames", C.c_int,
     [C.c_void_p, C.POINTER(rt_camera), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
      C.c_uint32, C.c_int32, C.POINTER(C.c_void_p), C.c_int32, C.POINTER(C.c_void_p),
      C.c_int32, C.c_int32]),
    ("rt_camera_init", C.c_int,
     [_dbl3, _dbl3, _dbl3, C.c_double, C.c_double, C.c_double, C.POINTER(rt_camera)]),
    ("rt_out_bytes_per_pixel", C.c_int32, [C.c_int32]),
    ("rt_supersample_camera", C.c_int, [C.POINTER(rt_camera), C.c_int32, C.POINTER(rt_camera)]),
    ("rt_band_rows", C.c_int,
     [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    ("rt_max_depth", C.c_int32, []),
    ("rt_tile_rows", C.c_int32, []),
    ("rt_frame_boxes", C.c_int,
     [C.POINTER(rt_prim), C.c_int32, C.POINTER(rt_camera), C.c_int32, C.c_int32,
      C.POINTER(C.c_int16), C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    ("rt_selftest", C.c_int, [C.c_void_p, C.c_int32, C.c_uint64, C.c_uint64,
                              C.POINTER(C.c_uint64)]),
    ("rt_set_row_order", C.c_int, [C.c_void_p, C.POINTER(C.c_int16), C.c_int32]),
    ("rt_interleaved_rows", C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32)]),
    ("rt_render_device_interleaved", C.c_int,
     [C.c_void_p, C.POINTER(rt_camera), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_uint32,
      C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    # ray queries
    ("rt_trace_rays", C.c_int,
     [C.c_void_p, _dbl3, _dbl3, C.c_int64, C.c_int32, C.c_int32, C.c_uint32, C.c_int32,
      C.c_void_p, C.POINTER(rt_hit), C.c_int32, C.POINTER(rt_stats)]),
    ("rt_trace_rays_device", C.c_int,
     [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_uint32, C.c_int32,
      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("rt_occluded", C.c_int,
     [C.c_void_p, _dbl3, _dbl3, _dbl3, C.c_int64, C.POINTER(C.c_uint8), C.POINTER(C.c_uint64),
      C.POINTER(rt_stats)]),
    ("rt_occluded_device", C.c_int,
     [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
      C.c_void_p]),
    # frame AOVs
    ("rt_render_aov", C.c_int,
     [C.c_void_p, C.POINTER(rt_camera), C.c_int32, C.c_int32, C.POINTER(rt_aov_buffers),
      C.POINTER(rt_stats)]),
    ("rt_render_aov_device", C.c_int,
     [C.c_void_p, C.POINTER(rt_camera), C.c_int32, C.c_int32, C.POINTER(rt_aov_buffers),
      C.c_void_p]),
    # ambient occlusion
    ("rt_render_ao", C.c_int,
     [C.c_void_p, C.POINTER(rt_camera), C.c_int32, C.c_int32, C.POINTER(rt_ao_params),
      C.POINTER(rt_ao_buffers), C.POINTER(rt_stats)]),
    ("rt_render_ao_device", C.c_int,
     [C.c_void_p, C.POINTER(rt_camera), C.c_int32, C.c_int32, C.POINTER(rt_ao_params),
      C.POINTER(rt_ao_buffers), C.c_void_p]),
    ("rt_ao_directions", C.c_int, [C.c_int32, _dbl3]),
    # multi-GPU frame operator
    ("rt_multi_unique_id", C.c_int, [C.POINTER(C.c_uint8)]),
    ("rt_multi_create", C.c_int,
     [C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_uint8), C.c_int32,
      C.POINTER(C.c_void_p)]),
    ("rt_multi_destroy", C.c_int, [C.c_void_p]),
    ("rt_multi_last_error", C.c_char_p, [C.c_void_p]),
    ("rt_multi_set_scene", C.c_int, [C.c_void_p, C.POINTER(rt_prim), C.c_int32]),
    ("rt_multi_set_option", C.c_int, [C.c_void_p, C.c_int32, C.c_int64]),
    ("rt_multi_set_lights", C.c_int, [C.c_void_p, C.POINTER(rt_light), C.c_int32]),
    ("rt_multi_set_transmission", C.c_int, [C.c_void_p, C.POINTER(rt_transmission), C.c_int32]),
    ("rt_multi_render_device", C.c_int,
     [C.c_void_p, C.POINTER(rt_camera), C.c_int32, C.c_int32, C.c_uint32, C.c_int32, C.c_void_p,
      C.c_void_p]),
    ("rt_multi_render_device_frames", C.c_int,
     [C.c_void_p, C.POINTER(rt_camera), C.c_int32, C.c_int32, C.c_int32, C.c_uint32, C.c_int32,
      C.POINTER(C.c_void_p), C.c_int32, C.POINTER(C.c_void_p), C.c_int32, C.c_int32]),
    ("rt_multi_render", C.c_int,
     [C.c_void_p, C.POINTER(rt_camera), C.c_int32, C.c_int32, C.c_uint32, C.c_int32, C.c_void_p,
      C.POINTER(rt_stats)]),
    ("rt_multi_sync", C.c_int, [C.c_void_p]),
    ("rt_multi_set_row_weights", C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.c_int32]),
    ("rt_weighted_band_rows", C.c_int,
     [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_float), C.c_int32, C.POINTER(C.c_int32),
      C.POINTER(C.c_int32)]),
    ("rt_tile_row_costs", C.c_int,
     [C.c_void_p, C.POINTER(rt_camera), C.c_int32, C.c_int32, C.c_uint32, C.POINTER(C.c_float),
      C.c_int32]),
    ("rt_order_units", C.c_int,
     [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_int32, C.c_int32, C.POINTER(C.c_int16)]),
    ("rt_unit_costs", C.c_int,
     [C.c_void_p, C.POINTER(C.c_uint16), C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_uint32),
      C.POINTER(C.c_uint32)]),
]

_lib = None


class RTError(RuntimeError):
    def __init__(self, status: int, detail: str = ""):
        self.status = status
        msg = f"rt status {status}"
        if _lib is not None:
            msg += f" ({_lib.rt_strerror(status).decode()})"
        if detail:
            msg += f": {detail}"
        super().__init__(msg)


def load(path: str | None = None) -> C.CDLL:
    """Load librt_amd.so (raises if it was not built — the product has no fallback)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise FileNotFoundError(
            f"{p} not built: run `make -C ray-tracer-from-scratch_amd` (or __graft_entry__.build())")
    lib = C.CDLL(p)
    for name, res, args in SIGNATURES:
        if path is not None and not hasattr(lib, name):
            continue  # an older build loaded side by side (tools/ab.py)
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if path is None:
        _lib = lib
    return lib


def check(status: int, ctx=None) -> None:
    if status != RT_OK:
        detail = ""
        if ctx is not None and _lib is not None:
            detail = (_lib.rt_last_hip_error(ctx) or b"").decode()
        raise RTError(status, detail)


def _d3(v) -> C.Array:
    return (C.c_double * 3)(*[float(x) for x in v])


def camera_init(position, lookat, vup, vfov: float, aspect_ratio: float,
                image_width: float) -> rt_camera:
    """Camera::init (scene.cpp:80-106) via the C-ABI host restatement."""
    lib = load()
    cam = rt_camera()
    check(lib.rt_camera_init(_d3(position), _d3(lookat), _d3(vup), float(vfov),
                             float(aspect_ratio), float(image_width), C.byref(cam)))
    return cam


def supersample_camera(cam: rt_camera, s: int) -> rt_camera:
    """rt_supersample_camera (host only): the camera of RT_OPT_SUPERSAMPLE's S-times larger
    frame, whose pixel (j*S + a, i*S + b) is sub-sample (a, b) of cam's pixel (j, i)."""
    lib = load()
    out = rt_camera()
    check(lib.rt_supersample_camera(C.byref(cam), int(s), C.byref(out)))
    return out


def frame_boxes(prims, cam: rt_camera, row0: int = 0, nrows: int | None = None):
    """rt_frame_boxes (host only) -> (primary [nbox, 4], mirror [.., 4], mir_depth): int16
    {x0, x1, i0, i1} boxes; the mirror array holds the levels back to back (the caller
    knows nW: level L has nW**L sequences of nbox boxes).  See include/rt_capi.h."""
    import numpy as np
    lib = load()
    if nrows is None:
        nrows = cam.height - row0
    arr = (rt_prim * max(1, len(prims)))(*prims)
    nb, md = C.c_int32(), C.c_int32()
    cap = 64 * (1 + 8 + 64 + 512)
    out = np.zeros((cap, 4), np.int16)
    check(lib.rt_frame_boxes(arr, len(prims), C.byref(cam), row0, nrows,
                             out.ctypes.data_as(C.POINTER(C.c_int16)), cap, C.byref(nb),
                             C.byref(md)))
    n = nb.value
    return out[:n], out[n:], md.value


def order_units(unit_max, unit_sum, mode: int = 0):
    """rt_order_units (host only): the dispatch order the row feedback derives from per-unit
    maxima and sums (mode 0 heaviest first, 1 RT_OPT_ROW_MIX's mixed order) -> int16 array."""
    import numpy as np
    lib = load()
    mx = np.ascontiguousarray(unit_max, np.uint32)
    sm = np.ascontiguousarray(unit_sum, np.uint32)
    if mx.shape != sm.shape or mx.ndim != 1:
        raise ValueError("unit_max and unit_sum differ in shape")
    n = len(mx)
    perm = np.zeros(max(1, n), np.int16)
    check(lib.rt_order_units(mx.ctypes.data_as(C.POINTER(C.c_uint32)),
                             sm.ctypes.data_as(C.POINTER(C.c_uint32)), n, int(mode),
                             perm.ctypes.data_as(C.POINTER(C.c_int16))))
    return perm[:n]


def band_rows(height: int, nranks: int, rank: int) -> tuple[int, int]:
    lib = load()
    r0, nr = C.c_int32(), C.c_int32()
    check(lib.rt_band_rows(height, nranks, rank, C.byref(r0), C.byref(nr)))
    return r0.value, nr.value


def tile_rows_of(height: int) -> int:
    """Tile rows of a frame of `height` pixel rows (rt_tile_rows() rows each)."""
    th = load().rt_tile_rows()
    return (height + th - 1) // th


def weighted_band_rows(height: int, nranks: int, rank: int, weights) -> tuple[int, int]:
    """rt_weighted_band_rows: contiguous band of `rank` cut at tile rows so every band
    carries ~1/nranks of the per-tile-row weights."""
    lib = load()
    w = list(weights)
    arr = (C.c_float * max(1, len(w)))(*w)
    r0, nr = C.c_int32(), C.c_int32()
    check(lib.rt_weighted_band_rows(height, nranks, rank, arr, len(w), C.byref(r0), C.byref(nr)))
    return r0.value, nr.value


def interleaved_rows(height: int, nparts: int, part: int) -> int:
    """rt_interleaved_rows: pixel rows of interleaved part `part` (tile rows part, part +
    nparts, ... of 8 rows)."""
    lib = load()
    n = C.c_int32()
    check(lib.rt_interleaved_rows(height, nparts, part, C.byref(n)))
    return n.value


def interleaved_row_index(height: int, nparts: int, part: int):
    """Frame rows of interleaved part `part`, in the order the part stores them."""
    th = load().rt_tile_rows()
    rows = []
    for t in range(part, (height + th - 1) // th, nparts):
        rows.extend(range(th * t, min(th * t + th, height)))
    return rows


def out_dtype_shape(out_format: int, nrows: int, width: int):
    if out_format == RT_OUT_RGB_F32:
        return np.float32, (nrows, width, 3)
    if out_format == RT_OUT_RGB_F64:
        return np.float64, (nrows, width, 3)
    if out_format in (RT_OUT_RGBA8, RT_OUT_RGBA8_WRAP):
        return np.uint8, (nrows, width, 4)
    raise ValueError(out_format)


class Renderer:
    """One rt_ctx on one HIP device (the C-ABI's lifecycle, RAII-style)."""

    def __init__(self, device: int = 0):
        self.lib = load()
        h = C.c_void_p()
        check(self.lib.rt_ctx_create(int(device), C.byref(h)))
        self.ctx = h
        self.device = device
        self._prims = None

    def close(self):
        if self.ctx:
            self.lib.rt_ctx_destroy(self.ctx)
            self.ctx = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_scene(self, prims) -> None:
        arr = (rt_prim * len(prims))(*prims)
        self._prims = arr
        check(self.lib.rt_set_scene(self.ctx, arr, len(prims)), self.ctx)

    def set_lights(self, lights) -> None:
        """rt_set_lights: 1..RT_MAX_LIGHTS coloured point lights (rt_light records or
        (position, color) pairs) for every launch enqueued afterwards; None or [] restores the
        reference's white light at the origin."""
        arr, n = light_array(lights)
        check(self.lib.rt_set_lights(self.ctx, arr, n), self.ctx)

    def set_transmission(self, recs) -> None:
        """rt_set_transmission: one (tau, ior) pair (or rt_transmission, or 0 = opaque) per scene
        object, in set_scene's order, for every launch enqueued afterwards; None or [] clears
        the records, and so does a list whose every tau is 0."""
        arr, n = transmission_array(recs)
        check(self.lib.rt_set_transmission(self.ctx, arr, n), self.ctx)

    def set_option(self, option: int, value: int) -> None:
        check(self.lib.rt_set_option(self.ctx, option, value), self.ctx)

    def set_row_order(self, perm) -> None:
        """rt_set_row_order: explicit tile-row dispatch order (None or [] clears it)."""
        perm = list(perm or [])
        arr = (C.c_int16 * max(1, len(perm)))(*perm)
        check(self.lib.rt_set_row_order(self.ctx, arr if perm else None, len(perm)), self.ctx)

    def selftest(self, test: int, n: int, seed: int = 1) -> int:
        bad = C.c_uint64()
        check(self.lib.rt_selftest(self.ctx, test, n, seed, C.byref(bad)), self.ctx)
        return bad.value

    def render(self, cam: rt_camera, depth: int, precision: int = RT_PREC_F64, flags: int = 0,
               out_format: int = RT_OUT_RGB_F32, row0: int = 0, nrows: int | None = None,
               count_segments: bool = False):
        """Synchronous render into a host numpy array -> (image, stats)."""
        if nrows is None:
            nrows = cam.height - row0
        dt, shape = out_dtype_shape(out_format, nrows, cam.width)
        out = np.empty(shape, dtype=dt)
        st = rt_stats()
        check(self.lib.rt_render(self.ctx, C.byref(cam), row0, nrows, depth, precision, flags,
                                 out_format, out.ctypes.data_as(C.c_void_p),
                                 1 if count_segments else 0, C.byref(st)), self.ctx)
        return out, st

    def render_device(self, cam: rt_camera, depth: int, d_out: int, precision: int = RT_PREC_F64,
                      flags: int = 0, out_format: int = RT_OUT_RGB_F32, row0: int = 0,
                      nrows: int | None = None, d_segments: int = 0, stream: int = 0) -> None:
        """Asynchronous render into device memory `d_out` on `stream` (raw pointers)."""
        if nrows is None:
            nrows = cam.height - row0
        check(self.lib.rt_render_device(self.ctx, C.byref(cam), row0, nrows, depth, precision,
                                        flags, out_format, C.c_void_p(d_out),
                                        C.c_void_p(d_segments or None),
                                        C.c_void_p(stream or None)), self.ctx)

    def tile_row_costs(self, cam: rt_camera, depth: int, precision: int = RT_PREC_PATH64,
                       flags: int = 0):
        """rt_tile_row_costs: measured cost (sum of the waves' shader cycles / 32) of every
        tile row of one render of the whole frame (synchronous) -> numpy float32."""
        n = tile_rows_of(cam.height)
        out = np.zeros(max(1, n), np.float32)
        check(self.lib.rt_tile_row_costs(self.ctx, C.byref(cam), depth, precision, flags,
                                         out.ctypes.data_as(C.POINTER(C.c_float)), n), self.ctx)
        return out[:n]

    def unit_costs(self, cost, units_log2: int):
        """rt_unit_costs: the row feedback's reduction kernel on a [gy, gx] uint16 array of
        wave costs -> (unit_max, unit_sum), uint32 arrays of gy << units_log2 units."""
        c = np.ascontiguousarray(cost, np.uint16)
        gy, gx = c.shape
        nu = gy << units_log2
        mx, sm = np.zeros(nu, np.uint32), np.zeros(nu, np.uint32)
        check(self.lib.rt_unit_costs(self.ctx, c.ctypes.data_as(C.POINTER(C.c_uint16)), gy, gx,
                                     units_log2, mx.ctypes.data_as(C.POINTER(C.c_uint32)),
                                     sm.ctypes.data_as(C.POINTER(C.c_uint32))), self.ctx)
        return mx, sm

    def render_device_interleaved(self, cam: rt_camera, depth: int, nparts: int, part: int,
                                  d_out: int, precision: int = RT_PREC_F64, flags: int = 0,
                                  out_format: int = RT_OUT_RGB_F32, out_frame_rows: bool = False,
                                  d_segments: int = 0, stream: int = 0) -> None:
        """rt_render_device_interleaved: interleaved part `part` of `nparts` into device
        memory, back to back (default) or at its frame rows."""
        check(self.lib.rt_render_device_interleaved(
            self.ctx, C.byref(cam), nparts, part, depth, precision, flags, out_format,
            C.c_void_p(d_out), 1 if out_frame_rows else 0, C.c_void_p(d_segments or None),
            C.c_void_p(stream or None)), self.ctx)

    def render_device_frames(self, cams, depth: int, d_outs, precision: int = RT_PREC_F64,
                             flags: int = 0, out_format: int = RT_OUT_RGB_F32, row0: int = 0,
                             nrows: int | None = None, streams=(), nframes: int = 1) -> None:
        """rt_render_device_frames: frame f renders cams[f % len(cams)] into
        d_outs[f % len(d_outs)] on streams[f % len(streams)] (raw pointers), one call."""
        cams = list(cams)
        if nrows is None:
            nrows = cams[0].height - row0
        ca = (rt_camera * len(cams))(*cams)
        outs = (C.c_void_p * len(d_outs))(*[C.c_void_p(o) for o in d_outs])
        sts = (C.c_void_p * max(1, len(streams)))(*[C.c_void_p(x or None) for x in streams])
        check(self.lib.rt_render_device_frames(self.ctx, ca, len(cams), row0, nrows, depth,
                                               precision, flags, out_format, outs, len(d_outs),
                                               sts, len(streams), nframes), self.ctx)


    def trace_rays(self, origins, directions, depth: int, precision: int = RT_PREC_F64,
                   flags: int = 0, out_format: int = RT_OUT_RGB_F64, want_rgb: bool = True,
                   want_hits: bool = False, count_segments: bool = False):
        """rt_trace_rays: radiance and / or closest hits of a batch of rays ([n, 3] origins
        and un-normalised directions), synchronous -> (rgb or None, hits or None, stats).
        rgb is [n, 3] (or [n, 4] uint8), hits a HIT_DTYPE array.  want_rgb=False is the pure
        find_closest_hit query (one segment per ray, no shading)."""
        o = np.ascontiguousarray(origins, np.float64).reshape(-1, 3)
        d = np.ascontiguousarray(directions, np.float64).reshape(-1, 3)
        if o.shape != d.shape:
            raise ValueError("origins and directions differ in shape")
        n = o.shape[0]
        rgb = hits = None
        if want_rgb:
            dt, shape = out_dtype_shape(out_format, 1, n)
            rgb = np.empty(shape[1:], dtype=dt)
        if want_hits:
            hits = np.empty(n, HIT_DTYPE)
        st = rt_stats()
        check(self.lib.rt_trace_rays(
            self.ctx, o.ctypes.data_as(_dbl3), d.ctypes.data_as(_dbl3), n, depth, precision, flags,
            out_format, rgb.ctypes.data_as(C.c_void_p) if want_rgb else None,
            hits.ctypes.data_as(C.POINTER(rt_hit)) if want_hits else None,
            1 if count_segments else 0, C.byref(st)), self.ctx)
        return rgb, hits, st

    def trace_rays_device(self, d_origins: int, d_directions: int, n: int, depth: int,
                          d_out: int, d_hits: int = 0, precision: int = RT_PREC_F64,
                          flags: int = 0, out_format: int = RT_OUT_RGB_F64, d_segments: int = 0,
                          stream: int = 0) -> None:
        """rt_trace_rays_device: the same on raw device addresses, enqueued on `stream`
        without synchronising (d_out or d_hits may be 0, not both)."""
        check(self.lib.rt_trace_rays_device(
            self.ctx, C.c_void_p(d_origins or None), C.c_void_p(d_directions or None), n, depth,
            precision, flags, out_format, C.c_void_p(d_out or None), C.c_void_p(d_hits or None),
            C.c_void_p(d_segments or None), C.c_void_p(stream or None)), self.ctx)

    def occluded(self, origins, directions, tmax=None, want_mask: bool = True):
        """rt_occluded: is anything on the segment o .. o + d * tmax of each ray ([n, 3] origins
        and un-normalised directions; tmax a scalar, [n] or None = +inf), synchronous ->
        (mask uint8[n] or None, count of occluded rays, stats)."""
        o = np.ascontiguousarray(origins, np.float64).reshape(-1, 3)
        d = np.ascontiguousarray(directions, np.float64).reshape(-1, 3)
        if o.shape != d.shape:
            raise ValueError("origins and directions differ in shape")
        n = o.shape[0]
        t = None
        if tmax is not None:
            t = np.ascontiguousarray(np.broadcast_to(np.asarray(tmax, np.float64), (n,)))
        mask = np.empty(n, np.uint8) if want_mask else None
        count, st = C.c_uint64(), rt_stats()
        check(self.lib.rt_occluded(
            self.ctx, o.ctypes.data_as(_dbl3), d.ctypes.data_as(_dbl3),
            t.ctypes.data_as(_dbl3) if t is not None else None, n,
            mask.ctypes.data_as(C.POINTER(C.c_uint8)) if want_mask else None, C.byref(count),
            C.byref(st)), self.ctx)
        return mask, int(count.value), st

    def occluded_device(self, d_origins: int, d_directions: int, d_tmax: int, n: int, d_out: int,
                        d_count: int = 0, stream: int = 0) -> None:
        """rt_occluded_device: the same on raw device addresses, enqueued on `stream` without
        synchronising (d_tmax 0 = +inf; d_out or d_count may be 0, not both; *d_count +=)."""
        check(self.lib.rt_occluded_device(
            self.ctx, C.c_void_p(d_origins or None), C.c_void_p(d_directions or None),
            C.c_void_p(d_tmax or None), n, C.c_void_p(d_out or None), C.c_void_p(d_count or None),
            C.c_void_p(stream or None)), self.ctx)

    def render_aov(self, cam: rt_camera, layers=("hit", "index", "depth", "normal", "albedo"),
                   row0: int = 0, nrows: int | None = None):
        """rt_render_aov: the primary hits of rows [row0, row0 + nrows) of cam's frame as
        per-pixel layers, synchronous -> ({layer: array}, stats).  hit is a HIT_DTYPE array
        [nrows, width], index int32 and depth float32 [nrows, width], normal and albedo
        float32 [nrows, width, 3]."""
        if nrows is None:
            nrows = cam.height - row0
        out = {}
        for name in layers:
            dt, tail = AOV_LAYERS[name]
            out[name] = np.empty((nrows, cam.width) + tail, dt)
        bufs = rt_aov_buffers(**{k: v.ctypes.data for k, v in out.items()})
        st = rt_stats()
        check(self.lib.rt_render_aov(self.ctx, C.byref(cam), row0, nrows, C.byref(bufs),
                                     C.byref(st)), self.ctx)
        return out, st

    def render_aov_device(self, cam: rt_camera, d_layers: dict, row0: int = 0,
                          nrows: int | None = None, stream: int = 0) -> None:
        """rt_render_aov_device: the same into raw device addresses ({layer: address}; a layer
        left out or 0 is not written), enqueued on `stream` without synchronising."""
        if nrows is None:
            nrows = cam.height - row0
        unknown = set(d_layers) - set(AOV_LAYERS)
        if unknown:
            raise ValueError(f"unknown AOV layers {sorted(unknown)}")
        bufs = rt_aov_buffers(**{k: (v or None) for k, v in d_layers.items()})
        check(self.lib.rt_render_aov_device(self.ctx, C.byref(cam), row0, nrows, C.byref(bufs),
                                            C.c_void_p(stream or None)), self.ctx)

    @staticmethod
    def _ao_params(dirs, radius: float):
        """(rt_ao_params, the array it points into) for [k, 3] directions."""
        w = np.ascontiguousarray(dirs, np.float64).reshape(-1, 3)
        return rt_ao_params(w.ctypes.data_as(_dbl3), w.shape[0], 0, float(radius), None), w

    def render_ao(self, cam: rt_camera, dirs=None, ndirs: int = 16, radius: float = float("inf"),
                  layers=("count", "ao"), row0: int = 0, nrows: int | None = None):
        """rt_render_ao: ambient occlusion of rows [row0, row0 + nrows) of cam's frame,
        synchronous -> ({layer: array}, stats).  dirs: [k, 3] probe directions (not normalised;
        None = ao_directions(ndirs)); radius: the probes' parametric limit.  count is uint8
        [nrows, width] (occluded probes), ao float32 [nrows, width] (open fraction)."""
        if nrows is None:
            nrows = cam.height - row0
        if dirs is None:
            dirs = ao_directions(ndirs)
        prm, keep = self._ao_params(dirs, radius)
        out = {name: np.empty((nrows, cam.width), AO_LAYERS[name]) for name in layers}
        bufs = rt_ao_buffers(**{k: v.ctypes.data for k, v in out.items()})
        st = rt_stats()
        check(self.lib.rt_render_ao(self.ctx, C.byref(cam), row0, nrows, C.byref(prm),
                                    C.byref(bufs), C.byref(st)), self.ctx)
        return out, st

    def render_ao_device(self, cam: rt_camera, dirs, radius: float, d_layers: dict, row0: int = 0,
                         nrows: int | None = None, stream: int = 0) -> None:
        """rt_render_ao_device: the same into raw device addresses ({layer: address}; a layer
        left out or 0 is not written), enqueued on `stream` without synchronising.  dirs is
        host memory, consumed before the call returns."""
        if nrows is None:
            nrows = cam.height - row0
        unknown = set(d_layers) - set(AO_LAYERS)
        if unknown:
            raise ValueError(f"unknown AO layers {sorted(unknown)}")
        prm, keep = self._ao_params(dirs, radius)
        bufs = rt_ao_buffers(**{k: (v or None) for k, v in d_layers.items()})
        check(self.lib.rt_render_ao_device(self.ctx, C.byref(cam), row0, nrows, C.byref(prm),
                                           C.byref(bufs), C.c_void_p(stream or None)), self.ctx)


def ao_directions(n: int) -> np.ndarray:
    """rt_ao_directions: n unit vectors of a spherical Fibonacci set over the whole sphere,
    [n, 3] float64 (1 <= n <= RT_AO_MAX_DIRS)."""
    out = np.empty((max(int(n), 0), 3), np.float64)
    check(load().rt_ao_directions(int(n), out.ctypes.data_as(_dbl3)))
    return out


def multi_unique_id() -> bytes:
    """rt_multi_unique_id: a communicator id to share with every process (one-process-per-GPU
    model of rt_multi_create)."""
    lib = load()
    buf = (C.c_uint8 * RT_MULTI_ID_BYTES)()
    check(lib.rt_multi_unique_id(buf))
    return bytes(buf)


class MultiRenderer:
    """One rt_multi: ONE frame split into row bands over `nranks` GPUs and gathered into the
    frame buffer of rank 0 (include/rt_capi.h "multi-GPU frame operator").

    MultiRenderer([0, 1, 2, 3])                         one process drives 4 GPUs (RCCL)
    MultiRenderer([0, 0, 0], transport=RT_TRANSPORT_COPY)  3 ranks on one GPU, peer copies
    MultiRenderer([local], nranks=N, first_rank=rank, unique_id=id)   one process per GPU
    MultiRenderer([0], nranks=N, first_rank=r, unique_id=id, transport=RT_TRANSPORT_THREADS)
        rank r of N handles in this process, each driven from its own thread (rehearsal)
    """

    def __init__(self, devices, nranks: int | None = None, first_rank: int = 0,
                 unique_id: bytes | None = None, transport: int = RT_TRANSPORT_RCCL):
        self.lib = load()
        devs = list(devices)
        self.nranks = len(devs) if nranks is None else int(nranks)
        self.first_rank = int(first_rank)
        self.devices = devs
        arr = (C.c_int32 * len(devs))(*devs)
        uid = None
        if unique_id is not None:
            uid = (C.c_uint8 * RT_MULTI_ID_BYTES)(*unique_id)
        h = C.c_void_p()
        check(self.lib.rt_multi_create(arr, len(devs), self.nranks, self.first_rank, uid,
                                       int(transport), C.byref(h)))
        self.m = h

    def _check(self, st: int) -> None:
        if st != RT_OK:
            raise RTError(st, (self.lib.rt_multi_last_error(self.m) or b"").decode())

    @property
    def has_root(self) -> bool:
        return self.first_rank == 0

    def close(self):
        if getattr(self, "m", None):
            self.lib.rt_multi_destroy(self.m)
            self.m = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_scene(self, prims) -> None:
        arr = (rt_prim * max(1, len(prims)))(*prims)
        self._prims = arr
        self._check(self.lib.rt_multi_set_scene(self.m, arr, len(prims)))

    def set_lights(self, lights) -> None:
        """rt_multi_set_lights: Renderer.set_lights on every local rank."""
        arr, n = light_array(lights)
        self._check(self.lib.rt_multi_set_lights(self.m, arr, n))

    def set_transmission(self, recs) -> None:
        """rt_multi_set_transmission: Renderer.set_transmission on every local rank."""
        arr, n = transmission_array(recs)
        self._check(self.lib.rt_multi_set_transmission(self.m, arr, n))

    def set_option(self, option: int, value: int) -> None:
        self._check(self.lib.rt_multi_set_option(self.m, option, value))

    def render(self, cam: rt_camera, depth: int, precision: int = RT_PREC_PATH64, flags: int = 0,
               out_format: int = RT_OUT_RGB_F32):
        """Synchronous: (frame on the root's process else None, stats)."""
        st = rt_stats()
        out = None
        ptr = None
        if self.has_root:
            dt, shape = out_dtype_shape(out_format, cam.height, cam.width)
            out = np.empty(shape, dtype=dt)
            ptr = out.ctypes.data_as(C.c_void_p)
        self._check(self.lib.rt_multi_render(self.m, C.byref(cam), depth, precision, flags,
                                             out_format, ptr, C.byref(st)))
        return out, st

    def render_device(self, cam: rt_camera, depth: int, d_frame: int, precision: int = RT_PREC_PATH64,
                      flags: int = 0, out_format: int = RT_OUT_RGB_F32, stream: int = 0) -> None:
        self._check(self.lib.rt_multi_render_device(self.m, C.byref(cam), depth, precision, flags,
                                                    out_format, C.c_void_p(d_frame or None),
                                                    C.c_void_p(stream or None)))

    def render_device_frames(self, cams, depth: int, d_frames, precision: int = RT_PREC_PATH64,
                             flags: int = 0, out_format: int = RT_OUT_RGB_F32, streams=(),
                             nframes: int = 1) -> None:
        cams = list(cams)
        ca = (rt_camera * len(cams))(*cams)
        d_frames = list(d_frames)
        outs = (C.c_void_p * max(1, len(d_frames)))(*[C.c_void_p(o or None) for o in d_frames])
        sts = (C.c_void_p * max(1, len(streams)))(*[C.c_void_p(x or None) for x in streams])
        self._check(self.lib.rt_multi_render_device_frames(
            self.m, ca, len(cams), depth, precision, flags, out_format, outs, len(d_frames), sts,
            len(streams), nframes))

    def sync(self) -> None:
        self._check(self.lib.rt_multi_sync(self.m))

    def set_row_weights(self, weights) -> None:
        """rt_multi_set_row_weights: per-tile-row weights of RT_OPT_MULTI_LAYOUT = 2 (the
        same on every rank; None or [] clears them)."""
        w = [float(x) for x in (weights if weights is not None else [])]
        arr = (C.c_float * max(1, len(w)))(*w)
        self._check(self.lib.rt_multi_set_row_weights(self.m, arr, len(w)))
