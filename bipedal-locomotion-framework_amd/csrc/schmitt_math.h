// schmitt_math.h -- one sample of one Schmitt trigger (Contacts::SchmittTriggerDetector), the step
// include/blf/blf_c.h section 13 writes out.  schmitt_trigger_kernel and legged_odometry_kernel
// (odometry.hip) both call it, so the fused kernel's contact states are the stand-alone call's bit
// for bit by construction.  fp64, one subtraction and one comparison per test, selects only.
#pragma once

#include "blf_internal.h"

namespace blf {

// The trigger parameters of a call, by value in the kernel arguments (they are host memory in the
// C ABI, validated there): row c = (on_threshold, off_threshold, switch_on_after, switch_off_after)
// of slot c; a call with shared parameters repeats its one row.
struct TrigParams {
    double p[BLF_ODOM_MAX_CONTACTS][4];
};

// Slot k's row in registers: selects over the rows (a lane-indexed read of a kernel argument would
// put the table in scratch)
__device__ __forceinline__ void trig_row(const TrigParams& tp, int k, double* prm)
{
#pragma unroll
    for (int i = 0; i < 4; ++i) prm[i] = tp.p[0][i];
#pragma unroll
    for (int c = 1; c < BLF_ODOM_MAX_CONTACTS; ++c)
#pragma unroll
        for (int i = 0; i < 4; ++i) prm[i] = k == c ? tp.p[c][i] : prm[i];
}

// state: bit 0 the contact state, bit 1 an edge is pending; edge / sw: edge_time, switch_time
__device__ __forceinline__ void schmitt_step(const double* prm, double t, double v, int32_t& state, double& edge,
                                             double& sw)
{
    const bool fin = __builtin_isfinite(v) && __builtin_isfinite(t);
    const bool on = (state & 1) != 0;
    const bool pend = (state & 2) != 0;
    const bool cross = on ? v <= prm[1] : v >= prm[0];
    const double after = on ? prm[3] : prm[2];
    const double e = cross && !pend ? t : edge;   // a new edge is stamped, a pending one keeps its time
    const bool fire = cross && (t - e) >= after;
    const int32_t s = fire ? (on ? 0 : 1) : ((on ? 1 : 0) | (cross ? 2 : 0));
    state = fin ? s : state;
    edge = fin ? e : edge;
    sw = fin && fire ? t : sw;
}

}  // namespace blf
