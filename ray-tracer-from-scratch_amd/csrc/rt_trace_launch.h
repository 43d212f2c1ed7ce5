/* rt_trace_launch.h — the table and pixel-pair kernels (k_trace_tab, k_trace_pair) and the
 * launcher chain from launch_trace_ns down to launch_one, for the plain unit (rt_trace.hip,
 * rt::kno) and the stamped unit (rt_trace_stamp.hip, rt::kst).  Not a header of its own:
 * included inside the unit's namespace, behind rt_scan_dev.h and rt_frame_dev.h. */

/* The table kernels and the resolving kernels (RT_OPT_SUPERSAMPLE) are launched by the plain
 * unit alone, so only it instantiates them: row feedback never samples such a frame. */
constexpr bool PLAIN_UNIT = !RT_STAMP;

/* A batch of frames of one band in ONE launch (rt_render_device_frames with
 * RT_OPT_FRAME_BATCH): frame blockIdx.z's kernel arguments come from a device table the host
 * filled (one KParams per frame, copied in behind the previous work on the stream), the
 * same code as k_trace otherwise.  The table is addressed in the constant address space
 * (it is read-only while the kernel runs), like the kernel-argument segment: its fields
 * load through the scalar path and the pointers in it are known global — through a plain
 * pointer the compiler could not prove the table unclobbered by the kernel's own stores and
 * turned every access into a per-lane flat load.  The linear-scan kernels only (the cull
 * kernels' frames take one launch each). */
typedef __attribute__((address_space(4))) const KParams ConstKParams;
template <int PREC, bool SUN, bool INT_EXP, int MAXD>
__global__ void __launch_bounds__(BLOCK)
__attribute__((amdgpu_waves_per_eu(waves_per_eu<PREC, SUN, INT_EXP, false, MAXD>(), 8)))
k_trace_tab(uint64_t tab_addr) {
    ConstKParams* tab = (ConstKParams*)tab_addr;
    trace_grid<PREC, SUN, INT_EXP, false, MAXD>(*(const KParams*)&tab[blockIdx.z]);
}

/* PATH64 linear scan, two pixels per lane (trace_pair_p64): tile pair bp of dispatch unit
 * u covers tile columns 2bp and 2bp + 1 of its tile row. */
#ifndef RT_WPE_PAIR
#define RT_WPE_PAIR 3
#endif
#if RT_WAVES_PER_BLOCK == 1 && !RT_AB_SLIM  // one-wave 8x8 tiles only (see launch_trace_ns)
template <bool SUN, int MAXD>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(RT_WPE_PAIR, 8)))
k_trace_pair(KParams p) {
    static_assert(BLOCK == 64 && TILE_W == 8 && TILE_H == 8, "one 8x8 tile pair per wave");
    const int u = tile_row(p, blockIdx.y, (int)gridDim.y);
    const int ul = p.row_units_log2;
    const int gx = (p.W + TILE_W - 1) / TILE_W;
    const int bx = 2 * (((u & ((1 << ul) - 1)) * (int)gridDim.x) + (int)blockIdx.x);
    const int trow = u >> ul;
    const int lane = threadIdx.x & 63;
    const int x = bx * TILE_W + (lane & 7);
    const int r = trow * TILE_H + (lane >> 3);
    const bool va = x < p.W && r < p.nrows, vb = x + 8 < p.W && r < p.nrows;
    const int i = p.row0 + r;
    int segs = 0;
    uint64_t t_tile = 0;
    f3 ca, cb;
    trace_pair_p64<SUN, MAXD>(p, x, i, va, vb, segs, t_tile, ca, cb);
    if (va) store_pixel(p, r, x, ca.x, ca.y, ca.z);
    if (vb) store_pixel(p, r, x + 8, cb.x, cb.y, cb.z);
    count_segments(p, segs);
    if (RT_STAMP && lane == 0) {
        // both tiles get the pair's cost (the host's row order reads per-tile costs)
        const uint64_t c = (__builtin_amdgcn_s_memtime() - t_tile) >> 5;
        const uint16_t c16 = (uint16_t)(c < 65535 ? c : 65535);
        if (bx < gx) p.tile_cost[(size_t)trow * gx + bx] = c16;
        if (bx + 1 < gx) p.tile_cost[(size_t)trow * gx + bx + 1] = c16;
    }
}
template <bool SUN>
static hipError_t launch_pair(const KParams& p, dim3 grid, hipStream_t st, hipEvent_t done) {
    auto go = [&](auto kern) {
        if (done)
            hipExtLaunchKernelGGL(kern, grid, dim3(64), 0, st, nullptr, done, 0, p);
        else
            hipLaunchKernelGGL(kern, grid, dim3(64), 0, st, p);
    };
    if (p.depth <= MAXD_SMALL)
        go(k_trace_pair<SUN, MAXD_SMALL>);
    else if (p.depth <= MAXD_MID)
        go(k_trace_pair<SUN, MAXD_MID>);
    else if (p.depth <= MAXD_REF)
        go(k_trace_pair<SUN, MAXD_REF>);
    else
        go(k_trace_pair<SUN, MAXD_LARGE>);
    return hipGetLastError();
}
#endif  // RT_WAVES_PER_BLOCK == 1 && !RT_AB_SLIM

template <int PREC, bool SUN, bool INT_EXP, bool CULL, int MAXD, bool SS>
static void launch_one(const KParams& p, dim3 grid, hipStream_t st, hipEvent_t done,
                       const KParams* tab) {
    if constexpr (PLAIN_UNIT && !CULL && !SS) {
        if (tab) {  // grid.z frames, their arguments in the device table
            hipExtLaunchKernelGGL((k_trace_tab<PREC, SUN, INT_EXP, MAXD>), grid, dim3(BLOCK), 0, st,
                                  nullptr, done, 0, (uint64_t)(uintptr_t)tab);
            return;
        }
    }
    if (done)
        hipExtLaunchKernelGGL((k_trace<PREC, SUN, INT_EXP, CULL, MAXD, SS>), grid, dim3(BLOCK), 0, st,
                              nullptr, done, 0, p);
    else
        hipLaunchKernelGGL((k_trace<PREC, SUN, INT_EXP, CULL, MAXD, SS>), grid, dim3(BLOCK), 0, st, p);
}
template <int PREC, bool SUN, bool INT_EXP, bool CULL, bool SS>
static hipError_t launch_depth(const KParams& p, dim3 grid, hipStream_t st, hipEvent_t done,
                               const KParams* tab) {
    if constexpr (RT_AB_SLIM && (PREC != PREC_PATH64 || SUN)) {
        return hipErrorInvalidValue;
    } else if constexpr (RT_AB_SLIM) {
        if (p.depth <= MAXD_SMALL)
            launch_one<PREC, SUN, INT_EXP, CULL, MAXD_SMALL, SS>(p, grid, st, done, tab);
        else if (p.depth <= MAXD_MID)
            launch_one<PREC, SUN, INT_EXP, CULL, MAXD_MID, SS>(p, grid, st, done, tab);
        else
            return hipErrorInvalidValue;
        return hipGetLastError();
    } else {
        if (p.depth <= MAXD_SMALL)
            launch_one<PREC, SUN, INT_EXP, CULL, MAXD_SMALL, SS>(p, grid, st, done, tab);
        else if (p.depth <= MAXD_MID)
            launch_one<PREC, SUN, INT_EXP, CULL, MAXD_MID, SS>(p, grid, st, done, tab);
        else if (p.depth <= MAXD_REF)
            launch_one<PREC, SUN, INT_EXP, CULL, MAXD_REF, SS>(p, grid, st, done, tab);
        else
            launch_one<PREC, SUN, INT_EXP, CULL, MAXD_LARGE, SS>(p, grid, st, done, tab);
        return hipGetLastError();
    }
}
template <int PREC, bool SUN, bool INT_EXP, bool SS>
static hipError_t launch_cull(const KParams& p, dim3 grid, hipStream_t st, hipEvent_t done,
                              const KParams* tab) {
    if (tab && p.wave_cull) return hipErrorNotSupported;  // no table kernels for the cull path
    return p.wave_cull ? launch_depth<PREC, SUN, INT_EXP, true, SS>(p, grid, st, done, tab)
                       : launch_depth<PREC, SUN, INT_EXP, false, SS>(p, grid, st, done, tab);
}
template <int PREC, bool SS = false>
static hipError_t launch_prec(const KParams& p, dim3 grid, hipStream_t st, hipEvent_t done,
                              const KParams* tab = nullptr) {
    if constexpr (PREC == PREC_F64 || PREC == PREC_MIXED) {
        if (p.flags & FLAG_SUN)
            return p.int_exp ? launch_cull<PREC, true, true, SS>(p, grid, st, done, tab)
                             : launch_cull<PREC, true, false, SS>(p, grid, st, done, tab);
        return p.int_exp ? launch_cull<PREC, false, true, SS>(p, grid, st, done, tab)
                         : launch_cull<PREC, false, false, SS>(p, grid, st, done, tab);
    } else {
        return (p.flags & FLAG_SUN) ? launch_cull<PREC, true, true, SS>(p, grid, st, done, tab)
                                    : launch_cull<PREC, false, true, SS>(p, grid, st, done, tab);
    }
}

int max_depth_ns() { return MAXD_LARGE; }

int launch_trace_ns(const KParams& p, int prec, void* stream, void* done_event,
                    const KParams* d_tab = nullptr, int nframes = 1) {
    if (p.W <= 0 || p.nrows <= 0) return (int)hipSuccess;
    const int ul = p.row_units_log2;
    const int units = ((p.nrows + TILE_H - 1) / TILE_H) << ul;
    const dim3 grid((((p.W + TILE_W - 1) / TILE_W) + (1 << ul) - 1) >> ul, units, d_tab ? nframes : 1);
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipEvent_t done = static_cast<hipEvent_t>(done_event);
    if (d_tab) {  // a batch of frames: the table kernels (linear scan, one pixel per lane)
        if (p.wave_cull || p.pairs || p.ss_log2) return (int)hipErrorNotSupported;
        switch (prec) {
            case PREC_F64: return (int)launch_prec<PREC_F64>(p, grid, st, done, d_tab);
            case PREC_F32: return (int)launch_prec<PREC_F32>(p, grid, st, done, d_tab);
            case PREC_MIXED: return (int)launch_prec<PREC_MIXED>(p, grid, st, done, d_tab);
            case PREC_PATH64: return (int)launch_prec<PREC_PATH64>(p, grid, st, done, d_tab);
            default: return (int)hipErrorInvalidValue;
        }
    }
    if (p.ss_log2) {
        // RT_OPT_SUPERSAMPLE: the resolving variants, one pixel (sample) per lane; contiguous
        // bands, k in 1..3.  MIXED's contract is output == F64: the F64 kernels serve it.
        if constexpr (!PLAIN_UNIT) {
            return (int)hipErrorNotSupported;
        } else {
            if (p.ss_log2 < 0 || p.ss_log2 > 3 || p.tstride > 1 || ((p.W | p.nrows) & ((1 << p.ss_log2) - 1)))
                return (int)hipErrorInvalidValue;
            switch (prec) {
                case PREC_F64:
                case PREC_MIXED: return (int)launch_prec<PREC_F64, true>(p, grid, st, done);
                case PREC_F32: return (int)launch_prec<PREC_F32, true>(p, grid, st, done);
                case PREC_PATH64: return (int)launch_prec<PREC_PATH64, true>(p, grid, st, done);
                default: return (int)hipErrorInvalidValue;
            }
        }
    }
    // two pixels per lane exist only in one-wave (8x8 tile) builds: the pair kernel is not
    // instantiated for RT_WAVES_PER_BLOCK > 1 (RT_OPT_PIXEL_PAIRS ignored)
#if RT_WAVES_PER_BLOCK == 1 && !RT_AB_SLIM
    if (p.pairs && prec == PREC_PATH64 && !p.wave_cull) {
        // 16x8 pixels per wave: half the tile columns per dispatch unit
        const int gxp = (((p.W + TILE_W - 1) / TILE_W) + 1) >> 1;
        const dim3 gp((gxp + (1 << ul) - 1) >> ul, units);
        return (int)((p.flags & FLAG_SUN) ? launch_pair<true>(p, gp, st, done)
                                          : launch_pair<false>(p, gp, st, done));
    }
#endif
    switch (prec) {
        case PREC_F64: return (int)launch_prec<PREC_F64>(p, grid, st, done);
        case PREC_F32: return (int)launch_prec<PREC_F32>(p, grid, st, done);
        case PREC_MIXED: return (int)launch_prec<PREC_MIXED>(p, grid, st, done);
        case PREC_PATH64: return (int)launch_prec<PREC_PATH64>(p, grid, st, done);
        default: return (int)hipErrorInvalidValue;
    }
}

