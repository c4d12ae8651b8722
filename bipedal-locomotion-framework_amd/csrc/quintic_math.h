// quintic_math.h — the quintic segment's fit and Horner evaluation (include/blf/blf_c.h section 4),
// shared by quintic_fit_kernel / quintic_eval_kernel (planners.hip) and the swing-foot kernel
// (swing_foot.hip): one set of expressions in one order, so the two paths agree bit for bit (and
// with the oracle's orc_quintic_fit / orc_quintic_eval).
#pragma once
#include <hip/hip_runtime.h>

namespace blf {

// c[0..5] of p(tau) = sum c_i tau^i over a segment of length T matching (p0, v0, a0) at tau = 0 and
// (p1, v1, a1) at tau = T.
__device__ __forceinline__ void quintic_fit_coeffs(double T, double p0, double v0, double a0,
                                                   double p1, double v1, double a1, double* c)
{
    const double T2 = T * T;
    const double T3 = T2 * T;
    const double T4 = T3 * T;
    const double T5 = T4 * T;
    const double c2 = 0.5 * a0;
    const double h = p1 - ((p0 + v0 * T) + c2 * T2);
    const double hv = v1 - (v0 + a0 * T);
    const double ha = a1 - a0;
    c[0] = p0;
    c[1] = v0;
    c[2] = c2;
    c[3] = ((10.0 * h - 4.0 * (hv * T)) + 0.5 * (ha * T2)) / T3;
    c[4] = ((-15.0 * h + 7.0 * (hv * T)) - ha * T2) / T4;
    c[5] = ((6.0 * h - 3.0 * (hv * T)) + 0.5 * (ha * T2)) / T5;
}

// position, velocity and acceleration of the segment at tau
__device__ __forceinline__ void quintic_horner(double tau, double c0, double c1, double c2,
                                               double c3, double c4, double c5, double& p,
                                               double& v, double& a)
{
    p = c0 + tau * (c1 + tau * (c2 + tau * (c3 + tau * (c4 + tau * c5))));
    v = c1 + tau * (2.0 * c2 + tau * (3.0 * c3 + tau * (4.0 * c4 + tau * (5.0 * c5))));
    a = 2.0 * c2 + tau * (6.0 * c3 + tau * (12.0 * c4 + tau * (20.0 * c5)));
}

}  // namespace blf
