/* rt_trace_stamp.hip — the trace kernels of rt_trace.hip built a second time (namespace
 * rt::kst) with each wave recording its cost (shader cycles) into KParams::tile_cost: the
 * frames whose costs the host samples for the tile-row dispatch order (rt_capi.cpp row
 * feedback) launch these, every other frame the plain kernels.  A unit of its own because a
 * wave-start s_memtime costs ~15% at c2 wherever it sits (tools/ab.py), so the plain kernels
 * have none. */
#define RT_STAMP 1
#include "rt_knobs.h"

namespace rt {
namespace kst {
#include "rt_scan_dev.h"
#include "rt_frame_dev.h"
#include "rt_trace_launch.h"
}  // namespace kst

int launch_trace_stamped(const KParams& p, int prec, void* stream, void* done_event) {
    return kst::launch_trace_ns(p, prec, stream, done_event);
}

}  // namespace rt
