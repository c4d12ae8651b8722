// contact_math.h — device helpers shared by the kernels that evaluate the ContinuousContactModel
// wrench (contact_model.hip, fb_dynamics.hip: ContinuousContactModel.cpp:79-108) or its regressor
// (contact_model.hip, rls.hip: :223-254), expression order of oracle/blf_oracle_contact.c.
#pragma once

#include <hip/hip_runtime.h>

namespace blf {

struct V3 {
    double x, y, z;
};

__device__ __forceinline__ V3 cross(V3 a, V3 b)
{
    return V3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
__device__ __forceinline__ double at(const V3& a, int i) { return i == 0 ? a.x : (i == 1 ? a.y : a.z); }

// pr = {L, W, k, b}; tw = {v, w} (mixed); ps, ns = {p, R row-major}; out = {force, torque}
__device__ __forceinline__ void contact_wrench(const double* pr, const double* tw, const double* ps,
                                               const double* ns, double* out)
{
    const double L = pr[0], W = pr[1], k = pr[2], b = pr[3];
    const double area = L * W;
    const double LL = L * L, WW = W * W;
    const double* R = ps + 3;
    const double* R0 = ns + 3;
    const V3 w{tw[3], tw[4], tw[5]};
    const V3 e1{R[0], R[3], R[6]}, e2{R[1], R[4], R[7]};
    const V3 r01{R0[0], R0[3], R0[6]}, r02{R0[1], R0[4], R0[7]};
    const double aR = fabs(R[8]);
    const V3 t1 = cross(e1, r01), t2 = cross(e2, r02);
    const V3 u1 = cross(e1, cross(e1, w)), u2 = cross(e2, cross(e2, w));
    const double cf = aR * area;
    const double ct = aR * area / 12.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        out[i] = cf * (k * (ns[i] - ps[i]) - b * tw[i]);
        out[3 + i] = ct * (LL * (b * at(u1, i) + k * at(t1, i)) + WW * (b * at(u2, i) + k * at(t2, i)));
    }
}

// skew(e)^2 = e e^T - |e|^2 I, row-major
__device__ __forceinline__ void skew2(V3 e, double* S)
{
    const double n = (e.x * e.x + e.y * e.y) + e.z * e.z;
    const double ev[3] = {e.x, e.y, e.z};
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) S[3 * i + j] = i == j ? ev[i] * ev[j] - n : ev[i] * ev[j];
}

// The regressor (ContinuousContactModel.cpp:223-254), 6 x 2 row-major, wrench = o (k, b), from the
// terms contact_eval_kernel already holds: aR = |R22|, area = L W, LL = L L, WW = W W, the null
// and current positions p0v / p, the linear and angular velocity v / w, t_i = e_i x r0_i and
// S_i = skew(e_i)^2.  One expression order for every kernel that needs it (contact_model.hip,
// rls.hip), so their bits agree.
__device__ __forceinline__ void contact_regressor_terms(double aR, double area, double LL, double WW,
                                                        const double* p0v, const double* p,
                                                        const double* v, V3 w, V3 t1, V3 t2,
                                                        const double* S1, const double* S2, double* o)
{
    const double cf = aR * area;
    const double cv = -aR * area;
    const double ct = area / 12.0 * aR;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        o[2 * i] = cf * (p0v[i] - p[i]);
        o[2 * i + 1] = cv * v[i];
        o[2 * (3 + i)] = ct * (LL * at(t1, i) + WW * at(t2, i));
        const double M0 = LL * S1[3 * i] + WW * S2[3 * i];
        const double M1 = LL * S1[3 * i + 1] + WW * S2[3 * i + 1];
        const double M2 = LL * S1[3 * i + 2] + WW * S2[3 * i + 2];
        o[2 * (3 + i) + 1] = ct * ((M0 * w.x + M1 * w.y) + M2 * w.z);
    }
}

// The same from a contact's inputs: L, W; tw = {v, w} (mixed); ps, ns = {p, R row-major}.
__device__ __forceinline__ void contact_regressor(double L, double W, const double* tw,
                                                  const double* ps, const double* ns, double* o)
{
    const double* R = ps + 3;
    const double* R0 = ns + 3;
    const V3 e1{R[0], R[3], R[6]}, e2{R[1], R[4], R[7]};
    const V3 r01{R0[0], R0[3], R0[6]}, r02{R0[1], R0[4], R0[7]};
    double S1[9], S2[9];
    skew2(e1, S1);
    skew2(e2, S2);
    contact_regressor_terms(fabs(R[8]), L * W, L * L, W * W, ns, ps, tw, V3{tw[3], tw[4], tw[5]},
                            cross(e1, r01), cross(e2, r02), S1, S2, o);
}

}  // namespace blf
