/* rt_trace.hip — the plain frame kernels (namespace rt::kno): the per-pixel trace/shade hot
 * path for gfx950 (CDNA4), one thread per pixel.  The device code is rt_scan_dev.h (math,
 * exact tests, scans, shading: its opening comment describes the precisions and the exact
 * rewrites) and rt_frame_dev.h (a frame's pixel paths, tiles and grid); the kernels and the
 * launcher chain are rt_trace_launch.h, shared with the stamped unit (rt_trace_stamp.hip).
 * This unit alone builds the self-test of the exact helpers and the row-feedback reduction,
 * and holds the public launchers of plain frames and frame batches. */
#include "rt_knobs.h"

namespace rt {
namespace kno {
#include "rt_scan_dev.h"
#include "rt_frame_dev.h"
#include "rt_trace_launch.h"

/* ------------------------------------------------------------------------ */
/* self-test of the exact helpers (rt_selftest)                              */
/* ------------------------------------------------------------------------ */
__device__ __forceinline__ uint64_t mix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
/* random doubles spanning the magnitudes the kernel divides: 2^-40 .. 2^40, both signs */
__device__ __forceinline__ double rnd_double(uint64_t bits) {
    const uint64_t mant = bits & 0xFFFFFFFFFFFFFull;
    const uint64_t ex = 1023 - 40 + ((bits >> 52) % 81);
    const uint64_t sign = (bits >> 63) << 63;
    return __longlong_as_double((long long)(sign | (ex << 52) | mant));
}

__global__ void k_selftest(int which, uint64_t n, uint64_t seed, unsigned long long* bad) {
    unsigned long long nbad = 0;
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n;
         i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t z0 = mix64(seed + 3 * i), z1 = mix64(seed + 3 * i + 1);
        if (which == 0) {
            const double a = rnd_double(z0), b = rnd_double(z1);
            const double q = div_r(a, b, rcp_refined(b));
            if (__double_as_longlong(q) != __double_as_longlong(a / b)) ++nbad;
            // the normalisation pattern: component / sqrt(sum of squares)
            const double c = rnd_double(mix64(seed + 3 * i + 2));
            const double l = sqrt(a * a + b * b + c * c);
            const double q2 = div_r(c, l, rcp_refined(l));
            if (__double_as_longlong(q2) != __double_as_longlong(c / l)) ++nbad;
        } else if (which == 2) {
            const double a = fabs(rnd_double(z0));
            if (__double_as_longlong(sqrt_e(a)) != __double_as_longlong(sqrt(a))) ++nbad;
            const double b = (double)(z1 >> 11) * (1.0 / 9007199254740992.0);  // [0,1)
            if (__double_as_longlong(sqrt_e(b)) != __double_as_longlong(sqrt(b))) ++nbad;
            // the scaled range: subnormals and tiny normals up to 2^-700, and 0 / inf
            const uint64_t z2 = mix64(seed + 3 * i + 2);
            const uint64_t ex = z2 % 324;  // biased exponent 0 (subnormal) .. 323
            const double c = __longlong_as_double((long long)((ex << 52) | (z1 & 0xFFFFFFFFFFFFFull)));
            if (__double_as_longlong(sqrt_e(c)) != __double_as_longlong(sqrt(c))) ++nbad;
            if (i == 0) {
                const double sp[3] = {0.0, -0.0, __builtin_inf()};
                for (int k = 0; k < 3; ++k)
                    if (__double_as_longlong(sqrt_e(sp[k])) != __double_as_longlong(sqrt(sp[k]))) ++nbad;
            }
        } else {
            const double x = (double)(z0 >> 11) * (1.0 / 9007199254740992.0);  // [0,1)
            const double e = (double)(1 + (z1 % 64));
            const double ref = pow(x, e), got = pow_int(x, (int)e);
            // squaring compounds rounding: x^64 carries up to ~63u
            const double tol = 128.0 * 2.220446049250313e-16 * fabs(ref) + 1e-300;
            if (fabs(got - ref) > tol) ++nbad;
        }
    }
    for (int off = 32; off > 0; off >>= 1) nbad += __shfl_xor(nbad, off, 64);
    if ((threadIdx.x & 63) == 0 && nbad) atomicAdd(bad, nbad);
}

int launch_selftest_ns(int which, uint64_t n, uint64_t seed, unsigned long long* d_bad,
                       void* stream) {
    hipLaunchKernelGGL(k_selftest, dim3(1024), dim3(256), 0, static_cast<hipStream_t>(stream),
                       which, n, seed, d_bad);
    return (int)hipGetLastError();
}

/* ------------------------------------------------------------------------ */
/* row feedback: per dispatch unit, the most expensive wave of a sampled frame and the sum */
/* ------------------------------------------------------------------------ */
/* One wave per tile row: unit (r << ul) + q covers waves [q*U, min(gx, q*U + U)) of row r
 * (gx waves per row, U = ceil(gx / 2^ul)), the same split as the kernel's dispatch units.
 * ustat holds the nu = gy << ul maxima, then the nu sums (a unit's work; gx <= 65535 waves
 * of 16-bit costs fit 32 bits).  The host then reads 2 nu words instead of every wave's
 * cost (rt_capi.cpp order_units). */
__global__ void __launch_bounds__(64) k_unit_max_sum(const uint16_t* __restrict__ cost, int gy, int gx,
                                                     int ul, uint32_t* __restrict__ ustat) {
    const int r = blockIdx.x;
    if (r >= gy) return;
    const int upr = 1 << ul, U = (gx + upr - 1) >> ul, nu = gy << ul;
    for (int q = 0; q < upr; q++) {
        const int x0 = q * U, x1 = min(gx, x0 + U);
        uint32_t m = 0, s = 0;
        for (int x = x0 + (int)threadIdx.x; x < x1; x += 64) {
            const uint32_t c = cost[(size_t)r * gx + x];
            m = max(m, c);
            s += c;
        }
        for (int off = 32; off > 0; off >>= 1) {
            m = max(m, (uint32_t)__shfl_xor((int)m, off, 64));
            s += (uint32_t)__shfl_xor((int)s, off, 64);
        }
        if (threadIdx.x == 0) {
            ustat[(r << ul) + q] = m;
            ustat[nu + (r << ul) + q] = s;
        }
    }
}

int launch_unit_max_sum_ns(const uint16_t* cost, int gy, int gx, int ul, uint32_t* ustat, void* stream) {
    if (gy <= 0 || gx <= 0) return (int)hipSuccess;
    hipLaunchKernelGGL(k_unit_max_sum, dim3(gy), dim3(64), 0, static_cast<hipStream_t>(stream), cost,
                       gy, gx, ul, ustat);
    return (int)hipGetLastError();
}

#if RT_DIAG
extern "C" int rt_diag_read(unsigned long long* out16) {
    const int e = (int)hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_diag), sizeof g_diag);
    unsigned long long z[16] = {0};
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_diag), z, sizeof z);
    return e;
}
#endif

}  // namespace kno

int launch_trace_stamped(const KParams& p, int prec, void* stream, void* done_event);  // rt_trace_stamp.hip
int launch_trace(const KParams& p, int prec, void* stream, void* done_event) {
    return p.tile_cost != nullptr ? launch_trace_stamped(p, prec, stream, done_event)
                                  : kno::launch_trace_ns(p, prec, stream, done_event);
}
int max_depth() { return kno::max_depth_ns(); }
int launch_trace_batch(const KParams* d_tab, const KParams& p0, int nframes, int prec, void* stream,
                       void* done_event) {
    if (nframes <= 0) return (int)hipSuccess;
    return kno::launch_trace_ns(p0, prec, stream, done_event, d_tab, nframes);
}
int launch_selftest(int which, uint64_t n, uint64_t seed, unsigned long long* d_bad,
                    void* stream) {
    return kno::launch_selftest_ns(which, n, seed, d_bad, stream);
}
int launch_unit_max_sum(const uint16_t* cost, int gy, int gx, int ul, uint32_t* ustat, void* stream) {
    return kno::launch_unit_max_sum_ns(cost, gy, gx, ul, ustat, stream);
}

}  // namespace rt
