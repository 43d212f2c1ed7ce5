/* rt_trace_shadow.hip — the frame kernels of rt_trace.hip built once more (namespace
 * rt::ksh) with the light ray of RT_FLAG_SHADOWS in every segment (rt_trace.hip
 * light_blocked, rt_anyhit.h): the frames rendered with the flag launch these
 * (launch_trace_shadow), every other frame the plain kernels, whose code does not move. */
#define RT_SHADOW 1
#include "rt_trace.hip"
