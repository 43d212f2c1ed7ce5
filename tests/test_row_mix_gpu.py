"""RT_OPT_ROW_MIX on the GPU: the mixed dispatch order changes scheduling only, so every
frame under it is bitwise the feedback-off frame; and the row feedback's reduction kernel
(k_unit_max_sum, through rt_unit_costs) gives each dispatch unit's maximum and sum.

The scene is c2's (8 spheres + 4 walls) at depth 4, PATH64 and F32, with a cost snapshot on
every frame (RT_OPT_ROW_FEEDBACK 1) and two warm snapshots, so the measured order is in
force by the fourth of the eight frames.  Sizes: the smallest that reach each split of a
tile row into dispatch units - 64x24 (one unit per row), 136x40 (two, ragged right edge),
520x76 (eight, ragged right and bottom) - and the row band [8, 44) of the 520-wide frame."""
import numpy as np
import pytest

from conftest import has_gpu
from rtamd import capi, scenes

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")]

DEPTH = 4
SIZES = [(64, 24, 0, None), (136, 40, 0, None), (520, 76, 0, None), (520, 76, 8, 36)]
PRECS = [capi.RT_PREC_PATH64, capi.RT_PREC_F32]


@pytest.fixture(scope="module")
def rend():
    with capi.Renderer(0) as r:
        r.set_scene(scenes.to_prims(scenes.CONFIGS["c2"].scene()))
        yield r


@pytest.fixture(scope="module")
def plain(rend):
    """Feedback-off frames, rendered once per (size, band, precision)."""
    rend.set_option(capi.RT_OPT_ROW_FEEDBACK, 0)
    ref = {}
    for (w, h, r0, n) in SIZES:
        cam = capi.camera_init(**scenes.camera_args(w, h))
        for pc in PRECS:
            img, _ = rend.render(cam, DEPTH, pc, 0, capi.RT_OUT_RGB_F32, row0=r0, nrows=n)
            img.setflags(write=False)
            ref[(w, h, r0, n, pc)] = img
    rend.set_option(capi.RT_OPT_ROW_FEEDBACK, 32)
    return ref


def _defaults(rend):
    rend.set_option(capi.RT_OPT_ROW_MIX, 1)
    rend.set_option(capi.RT_OPT_ROW_FEEDBACK_WARM, 0)
    rend.set_option(capi.RT_OPT_ROW_FEEDBACK, 32)


@pytest.mark.parametrize("mix", [1, 2])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d_r%d" % s[:3])
def test_mixed_order_is_output_invariant(rend, plain, size, mix):
    """Eight frames one at a time (mix 2: every one of them in the mixed order once the
    snapshots have landed; mix 1: heaviest first, as these frames do not overlap)."""
    w, h, r0, n = size
    cam = capi.camera_init(**scenes.camera_args(w, h))
    try:
        for pc in PRECS:
            ref = plain[(w, h, r0, n, pc)]
            rend.set_option(capi.RT_OPT_ROW_MIX, mix)
            rend.set_option(capi.RT_OPT_ROW_FEEDBACK_WARM, 2)
            rend.set_option(capi.RT_OPT_ROW_FEEDBACK, 1)
            for f in range(8):
                img, _ = rend.render(cam, DEPTH, pc, 0, capi.RT_OUT_RGB_F32, row0=r0, nrows=n)
                assert np.array_equal(img.view(np.uint32), ref.view(np.uint32)), (size, pc, f)
    finally:
        _defaults(rend)


@pytest.mark.parametrize("mix", [1, 2])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d_r%d" % s[:3])
def test_mixed_order_is_output_invariant_in_flight(rend, plain, size, mix):
    """The same through rt_render_device_frames on two streams and two buffers (mix 1: the
    frames in flight take the mixed order)."""
    import torch
    dev = torch.device("cuda", 0)
    w, h, r0, n = size
    cam = capi.camera_init(**scenes.camera_args(w, h))
    rows = h - r0 if n is None else n
    sts = [torch.cuda.Stream(dev) for _ in range(2)]
    try:
        for pc in PRECS:
            ref = plain[(w, h, r0, n, pc)]
            rend.set_option(capi.RT_OPT_ROW_MIX, mix)
            rend.set_option(capi.RT_OPT_ROW_FEEDBACK_WARM, 2)
            rend.set_option(capi.RT_OPT_ROW_FEEDBACK, 1)
            outs = [torch.zeros((rows, w, 3), dtype=torch.float32, device=dev) for _ in range(2)]
            ptrs = [o.data_ptr() for o in outs]
            for nf in (6, 2):   # frames 1-6, then 7-8 with the order of the landed snapshots
                rend.render_device_frames([cam], DEPTH, ptrs, pc, row0=r0, nrows=n,
                                          streams=[s.cuda_stream for s in sts], nframes=nf)
                torch.cuda.synchronize()
                for o in outs:
                    assert np.array_equal(o.cpu().numpy().view(np.uint32), ref.view(np.uint32)), (size, pc, nf)
                    o.zero_()
    finally:
        _defaults(rend)


def test_row_mix_option_values(rend):
    try:
        for v in (0, 1, 2):
            rend.set_option(capi.RT_OPT_ROW_MIX, v)
        for v in (-1, 3):
            with pytest.raises(capi.RTError):
                rend.set_option(capi.RT_OPT_ROW_MIX, v)
    finally:
        _defaults(rend)


@pytest.mark.parametrize("per_unit", [1, 63, 64, 65])
def test_unit_reduction_kernel_matches_numpy(rend, per_unit):
    """k_unit_max_sum on caller costs: 1, 63, 64 and 65 waves per unit (below, at and past the
    wave's 64 lanes), every split (1, 2, 4, 8 units per row, the last unit ragged or empty),
    random and saturated costs."""
    rng = np.random.default_rng(per_unit)
    for ul in (0, 1, 2, 3):
        upr = 1 << ul
        for gx in sorted({per_unit * upr, max(1, per_unit * upr - (upr - 1))}):
            U = (gx + upr - 1) >> ul
            if U != per_unit:
                continue
            gy = 5
            cost = rng.integers(0, 65536, (gy, gx)).astype(np.uint16)
            cost[1, :] = 65535                      # a saturated row
            cost[3, rng.random(gx) < 0.5] = 65535
            mx, sm = rend.unit_costs(cost, ul)
            emx = np.zeros((gy, upr), np.uint32)
            esm = np.zeros((gy, upr), np.uint32)
            for q in range(upr):
                part = cost[:, q * U:min(gx, q * U + U)].astype(np.uint32)
                if part.shape[1]:
                    emx[:, q] = part.max(axis=1)
                    esm[:, q] = part.sum(axis=1)
            assert np.array_equal(mx, emx.ravel()), (per_unit, ul, gx)
            assert np.array_equal(sm, esm.ravel()), (per_unit, ul, gx)
