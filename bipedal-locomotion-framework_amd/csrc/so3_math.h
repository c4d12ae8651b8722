// so3_math.h — SO(3) helpers of the swing-foot and SO3 planner kernels (swing_foot.hip), in the
// arithmetic order of include/blf/blf_c.h section 11 (tests/swing_foot_reference.py restates it).
// Matrices are 3x3 row-major; every sum is evaluated left to right (no FMA contraction).
#pragma once
#include <hip/hip_runtime.h>

namespace blf {

__device__ __forceinline__ bool so3_finite(double v) { return __builtin_isfinite(v); }

// Unit axis u and angle theta in [0, pi] of E = Rn * Rr^T, through E's quaternion (Shepperd's rule:
// the branch is the largest of tr E, E00, E11, E22, the first of equals), its sign flipped to
// w >= 0.  nv = |q_v| == 0: theta = 0 and u = 0 (the only special case; theta == 0 iff nv == 0).
// At exactly pi (w == 0) the sign of u is whichever the branch produces.
__device__ __forceinline__ void so3_log_rel(const double* Rn, const double* Rr, double* u,
                                            double& theta)
{
    double E[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            E[3 * i + j] = (Rn[3 * i] * Rr[3 * j] + Rn[3 * i + 1] * Rr[3 * j + 1]) +
                           Rn[3 * i + 2] * Rr[3 * j + 2];
    const double tr = (E[0] + E[4]) + E[8];
    double w, x, y, z;
    if (tr >= E[0] && tr >= E[4] && tr >= E[8]) {
        const double s = 2.0 * sqrt(1.0 + tr);
        w = 0.25 * s;
        x = (E[7] - E[5]) / s;
        y = (E[2] - E[6]) / s;
        z = (E[3] - E[1]) / s;
    } else if (E[0] >= E[4] && E[0] >= E[8]) {
        const double s = 2.0 * sqrt(((1.0 + E[0]) - E[4]) - E[8]);
        w = (E[7] - E[5]) / s;
        x = 0.25 * s;
        y = (E[1] + E[3]) / s;
        z = (E[2] + E[6]) / s;
    } else if (E[4] >= E[8]) {
        const double s = 2.0 * sqrt(((1.0 + E[4]) - E[0]) - E[8]);
        w = (E[2] - E[6]) / s;
        x = (E[1] + E[3]) / s;
        y = 0.25 * s;
        z = (E[5] + E[7]) / s;
    } else {
        const double s = 2.0 * sqrt(((1.0 + E[8]) - E[0]) - E[4]);
        w = (E[3] - E[1]) / s;
        x = (E[2] + E[6]) / s;
        y = (E[5] + E[7]) / s;
        z = 0.25 * s;
    }
    if (w < 0.0) {
        w = -w;
        x = -x;
        y = -y;
        z = -z;
    }
    const double nv = sqrt((x * x + y * y) + z * z);
    if (nv == 0.0) {
        theta = 0.0;
        u[0] = 0.0;
        u[1] = 0.0;
        u[2] = 0.0;
        return;
    }
    theta = 2.0 * atan2(nv, w);
    u[0] = x / nv;
    u[1] = y / nv;
    u[2] = z / nv;
}

// The minimum-jerk profile at tau = (t - t0) / T: s, ds/dt, d2s/dt2.
__device__ __forceinline__ void so3_min_jerk(double tau, double T, double& s, double& sd,
                                             double& sdd)
{
    s = ((tau * tau) * tau) * (10.0 + tau * (-15.0 + 6.0 * tau));
    sd = ((tau * tau) * (30.0 + tau * (-60.0 + 30.0 * tau))) / T;
    sdd = (tau * (60.0 + tau * (-180.0 + 120.0 * tau))) / (T * T);
}

// R = Exp(a u) * Rr with Exp(a u) = I + sin(a) [u]x + 2 sin^2(a / 2) [u]x^2 and
// [u]x^2 = u u^T - I for a unit u.
__device__ __forceinline__ void so3_exp_apply(double a, const double* u, const double* Rr,
                                              double* R)
{
    const double sa = sin(a);
    const double sh = sin(0.5 * a);
    const double cv = 2.0 * (sh * sh);
    double M[9];
    M[0] = 1.0 + cv * (u[0] * u[0] - 1.0);
    M[4] = 1.0 + cv * (u[1] * u[1] - 1.0);
    M[8] = 1.0 + cv * (u[2] * u[2] - 1.0);
    M[1] = sa * (-u[2]) + cv * (u[0] * u[1]);
    M[2] = sa * u[1] + cv * (u[0] * u[2]);
    M[3] = sa * u[2] + cv * (u[1] * u[0]);
    M[5] = sa * (-u[0]) + cv * (u[1] * u[2]);
    M[6] = sa * (-u[1]) + cv * (u[2] * u[0]);
    M[7] = sa * u[0] + cv * (u[2] * u[1]);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            R[3 * i + j] = (M[3 * i] * Rr[j] + M[3 * i + 1] * Rr[3 + j]) + M[3 * i + 2] * Rr[6 + j];
}

}  // namespace blf
