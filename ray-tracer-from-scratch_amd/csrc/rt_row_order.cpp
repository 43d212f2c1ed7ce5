/*
 * rt_row_order.cpp — the row feedback's ordering policy (pure host: no HIP, no rt_ctx): from
 * the per-unit maxima and sums of a cost snapshot to the dispatch order of the next frames.
 * rt_feedback.cpp owns the device side (when to sample, the snapshot, the bands).
 */
#include <algorithm>

#include "rt_host.h"

#ifndef RT_ROW_UNITS_MAX_LOG2
#define RT_ROW_UNITS_MAX_LOG2 3
#endif
#ifndef RT_ROW_MIX_TAIL_PERMILLE
#define RT_ROW_MIX_TAIL_PERMILLE 20
#endif

namespace rth __attribute__((visibility("hidden"))) {

/* Dispatch units per tile row for the measured order (log2): rows split in up to 8 parts
 * while the units fit row_perm and keep >= 8 tiles each — the ordering gets finer where a
 * row holds both heavy and light tiles (replay of c2's measured wave times: whole rows
 * -15%, quarter rows -19% vs centre-out). */
int units_log2(int gy, int gx) {
    if (rt::BLOCK != 64) return 0;
    for (int k = RT_ROW_UNITS_MAX_LOG2; k > 0; k--)
        if ((gy << k) <= rt::ROW_PERM_MAX && ((gx + (1 << k) - 1) >> k) >= 8) return k;
    return 0;
}

/* RT_OPT_ROW_MIX: o.mix = o.perm (heaviest first) with the light units merged between the
 * heavy ones, so that waves of both kinds share the SIMDs for the whole frame instead of a
 * heavy phase (VALU-bound) followed by a light one (issue-bound, VALU half idle).
 *  - heavy = a unit whose work (the sum of its waves' costs, o.work) is above the mean, plus
 *    the first unit of o.perm whatever its work; the heavy units keep o.perm's order;
 *  - the lightest units (from the end of o.perm: at least one, then while they total
 *    <= RT_ROW_MIX_TAIL_PERMILLE / 1000 of the frame's work, about one fill of the chip at
 *    c2) are held back for the end, so the frame drains on short waves;
 *  - the other light units are drawn lightest first, each when the light work dispatched
 *    has fallen behind the heavy work's share (cl / TL < ch / TH, in exact integers).
 * No unit above the mean (all equal): o.mix = o.perm.  One pass, O(nu), no allocation once
 * the vectors have their size.
 * Measured alternatives at c2 PATH64, tile rows through rt_set_row_order, two frames in
 * flight, us/frame (profiles/r07/probes/row_mix_probe.jsonl): heaviest first 27.07; this
 * merge 25.37; the same with the light units drawn heaviest first 27.19; no held-back tail
 * (light heaviest first) 30.47; a tail of 50/1000 25.44. */
static void mix_units(UnitOrder& o, int nu) {
    const std::vector<int16_t>& s = o.perm;
    std::vector<int16_t>& out = o.mix;
    out.assign(s.begin(), s.end());
    uint64_t total = 0;
    for (int u = 0; u < nu; u++) total += o.work[u];
    std::vector<int16_t>& hv = o.heavy;
    std::vector<int16_t>& lt = o.light;
    hv.clear();
    lt.clear();
    bool above = false;
    for (int k = 0; k < nu; k++) {
        const bool h = (uint64_t)o.work[s[k]] * (uint64_t)nu > total;
        above |= h;
        (h || k == 0 ? hv : lt).push_back(s[k]);
    }
    if (!above || lt.empty()) return;
    // lt[m ..): the held-back tail
    size_t m = lt.size() - 1;
    uint64_t tail = o.work[lt[m]];
    while (m > 0 && (tail + o.work[lt[m - 1]]) * 1000u <= total * (uint64_t)RT_ROW_MIX_TAIL_PERMILLE)
        tail += o.work[lt[--m]];
    uint64_t th = 0, tl = 0;
    for (int16_t u : hv) th += o.work[u];
    for (size_t j = 0; j < m; j++) tl += o.work[lt[j]];
    typedef unsigned __int128 u128;
    uint64_t ch = 0, cl = 0;
    size_t i = 0, j = m, k = 0;  // the light units are drawn from lt[m - 1] down to lt[0]
    while (i < hv.size() || j > 0) {
        if (i < hv.size() && (j == 0 || (u128)cl * th >= (u128)ch * tl)) {
            ch += o.work[hv[i]];
            out[k++] = hv[i++];
        } else {
            cl += o.work[lt[--j]];
            out[k++] = lt[j];
        }
    }
    for (size_t t = m; t < lt.size(); t++) out[k++] = lt[t];
}

/* Dispatch units ordered by their most expensive wave (heaviest first; ties keep the lower
 * unit), from the per-unit maxima of a cost snapshot (k_unit_max_sum); the units' sums are
 * their work for the mixed order (mix_units).  Host work is O(nu):
 * the keys are 16-bit (wave costs saturate at 65535), sorted by a stable two-pass radix
 * sort — the comparison sort it replaces took ~100 us on the thread that enqueues frames,
 * long enough to starve the GPU once per snapshot. */
void order_units(const uint32_t* umax, const uint32_t* usum, int nu, UnitOrder& o, bool acc_valid,
                 int ema) {
    // smoothed over the band's snapshots (RT_OPT_ROW_FEEDBACK_EMA), else this snapshot's
    const float w = ema / 100.0f;
    const bool smooth = acc_valid && (int)o.acc.size() == nu && (int)o.work.size() == nu && ema > 0;
    if (!smooth) {
        o.acc.assign(nu, 0.0f);
        o.work.assign(nu, 0u);
    }
    o.key.resize(nu);
    for (int u = 0; u < nu; u++) {
        const float m = (float)std::min<uint32_t>(umax[u], 65535u);
        const float a = smooth ? w * o.acc[u] + (1.0f - w) * m : m;
        o.acc[u] = a;
        o.key[u] = (uint16_t)(65535u - (uint32_t)std::min(a + 0.5f, 65535.0f));  // descending
        o.work[u] = smooth ? (uint32_t)(w * (float)o.work[u] + (1.0f - w) * (float)usum[u] + 0.5f) : usum[u];
    }
    std::vector<int16_t>& perm = o.perm;
    std::vector<int16_t>& tmp = o.tmp;
    tmp.resize(nu);
    perm.resize(nu);
    for (int u = 0; u < nu; u++) perm[u] = (int16_t)u;
    for (int sh = 0; sh < 16; sh += 8) {
        unsigned cnt[257] = {0};
        for (int k = 0; k < nu; k++) cnt[((o.key[perm[k]] >> sh) & 255) + 1]++;
        for (int b = 0; b < 256; b++) cnt[b + 1] += cnt[b];
        for (int k = 0; k < nu; k++) tmp[cnt[(o.key[perm[k]] >> sh) & 255]++] = perm[k];
        perm.swap(tmp);
    }
    mix_units(o, nu);
}

}  // namespace rth
