// rls.hip — Estimators::RecursiveLeastSquare on the device (RecursiveLeastSquare.cpp:96-133), many
// independent filters in fp64 that stream their samples.
//
//  * rls_advance_kernel<N>: one lane per filter, 64 per workgroup (one wavefront).  The state x (N)
//    and the upper triangle of the covariance P (N (N + 1) / 2) stay in registers over all T steps
//    of a call; every step's [rows][m N] regressor slab and [rows][m] measurement slab arrive
//    through LDS as coalesced 16-B loads (slab.h, with its unaligned fallback) and each lane reads
//    its own row.  The reference's K = P H^T (lambda R + H P H^T)^-1 with a diagonal R is evaluated
//    as m sequential scalar updates (no m x m inverse), in the arithmetic order written in
//    include/blf/blf_c.h section 10.
//  * contact_rls_kernel: the same update with N = 2, m = 6 and the ContinuousContactModel
//    regressor (contact_math.h, the expression blf_contact_model_eval evaluates) formed in
//    registers from each step's twist / pose, so the regressor never goes to HBM.
// Built with -ffp-contract=off; tests/rls_reference.py restates the order in numpy.
#include "blf_internal.h"
#include "contact_math.h"
#include "slab.h"

namespace blf {
namespace {

constexpr int kRT = 64;   // filters per workgroup (one wavefront)

// A contiguous slab of n doubles (n <= 128 U) held in registers between its global loads (issue)
// and its LDS writes (commit): 16-B loads when the slab is aligned, 8-B loads otherwise.  Several
// slabs issued before the first commit are all in flight together (slab_load called twice waits
// for the first slab's loads before it issues the second's).
template <int U>
struct SlabRegs {
    double2 v[U];
    bool wide;
    __device__ __forceinline__ void issue(const double* g, int n, int lane)
    {
        wide = ((uintptr_t)g & 15) == 0;
        if (wide) {
            const int n2 = (n + 1) >> 1;   // an odd tail: the last pair's .y is not loaded
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int j = u * kRT + lane;
                if (2 * j + 1 < n) v[u] = reinterpret_cast<const double2*>(g)[j];
                else if (j < n2) v[u].x = g[2 * j];
            }
        } else {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int e = 2 * u * kRT + lane;
                if (e < n) v[u].x = g[e];
                if (e + kRT < n) v[u].y = g[e + kRT];
            }
        }
    }
    // s[r * SW + c] = slab[r * W + c]
    __device__ __forceinline__ void commit(double* s, int SW, int W, int n, int lane) const
    {
        const SlabIdx ix(W);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int e0 = wide ? 2 * (u * kRT + lane) : 2 * u * kRT + lane;
            const int e1 = wide ? e0 + 1 : e0 + kRT;
            if (e0 < n) {
                const int r = ix.row(e0);
                s[r * SW + (e0 - r * W)] = v[u].x;
            }
            if (e1 < n) {
                const int r = ix.row(e1);
                s[r * SW + (e1 - r * W)] = v[u].y;
            }
        }
    }
};

__device__ __forceinline__ constexpr int tri(int a, int b, int N)   // a <= b: row-wise upper triangle
{
    return a * N - a * (a - 1) / 2 + (b - a);
}

// One scalar measurement row h (N), measurement y, variance r: the six lines of blf_c.h section 10.
// P holds the upper triangle; P[a][c] with a > c is read as P[c][a].
template <int N>
__device__ __forceinline__ void rls_row(double* x, double* P, const double* h, double y, double r,
                                        double lambda)
{
    double g[N];
#pragma unroll
    for (int a = 0; a < N; ++a) {
        double acc = P[tri(0, a, N)] * h[0];
#pragma unroll
        for (int c = 1; c < N; ++c) acc = acc + P[c < a ? tri(c, a, N) : tri(a, c, N)] * h[c];
        g[a] = acc;
    }
    double hg = h[0] * g[0];
    double hx = h[0] * x[0];
#pragma unroll
    for (int a = 1; a < N; ++a) {
        hg = hg + h[a] * g[a];
        hx = hx + h[a] * x[a];
    }
    const double s = (lambda * r) + hg;
    const double e = y - hx;
    const bool good = s > 0.0 && s < __builtin_inf();   // false for NaN, 0, negative, +inf
    const double nan = __builtin_nan("");
    double k[N];
#pragma unroll
    for (int a = 0; a < N; ++a) k[a] = g[a] / s;
#pragma unroll
    for (int a = 0; a < N; ++a) {
        const double xa = x[a] + k[a] * e;
        x[a] = good ? xa : nan;
#pragma unroll
        for (int b = a; b < N; ++b) {
            const double pab = P[tri(a, b, N)] - k[a] * g[b];
            P[tri(a, b, N)] = good ? pab : nan;
        }
    }
}

// The tile's state and covariance rows (LDS, strides N | 1 and (N N) | 1) -> registers.
template <int N>
__device__ __forceinline__ void rls_state_read(const double* s_x, const double* s_p, int lane,
                                               double* x, double* P)
{
    constexpr int SX = N | 1, SP = (N * N) | 1;
#pragma unroll
    for (int a = 0; a < N; ++a) {
        x[a] = s_x[lane * SX + a];
#pragma unroll
        for (int b = a; b < N; ++b) P[tri(a, b, N)] = s_p[lane * SP + a * N + b];
    }
}

// Registers -> the tile's state and covariance rows (the covariance mirrored, so exactly
// symmetric), through the same two LDS slabs.  The caller has passed a barrier since their last
// read.
template <int N>
__device__ __forceinline__ void rls_state_store(double* s_x, double* s_p, double* state, double* cov,
                                                int64_t p0, int rows, int lane, const double* x,
                                                const double* P)
{
    constexpr int SX = N | 1, SP = (N * N) | 1;
#pragma unroll
    for (int a = 0; a < N; ++a) {
        s_x[lane * SX + a] = x[a];
#pragma unroll
        for (int b = 0; b < N; ++b) s_p[lane * SP + a * N + b] = P[a <= b ? tri(a, b, N) : tri(b, a, N)];
    }
    __syncthreads();
    slab_store<kRT, 4>(cov + p0 * (N * N), N * N, s_p, SP, rows, N * N);
    slab_store<kRT, 2>(state + p0 * N, N, s_x, SX, rows, N);
}

// LDS: s_h [64][(8 N) | 1], s_y and s_r [64][9], s_p [64][(N N) | 1], s_x [64][N | 1].  The state,
// the covariance, the variances and the first step's samples are loaded together: a call with
// steps = 1 (a closed loop's) waits for HBM once, not once per array.
template <int N>
__global__ __launch_bounds__(kRT) void rls_advance_kernel(
    int m, double lambda, const double* __restrict__ meas_cov, int shared_cov,
    const double* __restrict__ regressor, const double* __restrict__ meas, int steps,
    double* state, double* cov, int64_t batch)
{
    constexpr int NP = N * (N + 1) / 2;
    constexpr int SHmax = (BLF_RLS_MAX_MEAS * N) | 1;
    constexpr int SY = BLF_RLS_MAX_MEAS | 1;
    constexpr int SX = N | 1, SP = (N * N) | 1;
    __shared__ double s_h[kRT * SHmax];
    __shared__ double s_y[kRT * SY];
    __shared__ double s_r[kRT * SY];
    __shared__ double s_p[kRT * SP];
    __shared__ double s_x[kRT * SX];
    const int lane = threadIdx.x;
    const int64_t p0 = (int64_t)blockIdx.x * kRT;
    const int rows = (int)((batch - p0) < kRT ? (batch - p0) : kRT);
    const int W = m * N;
    const int SH = W | 1;
    {
        SlabRegs<(N * N + 1) / 2> fp;
        SlabRegs<(N + 1) / 2> fx;
        SlabRegs<4 * N> fh;
        SlabRegs<4> fy, fr;
        fp.issue(cov + p0 * (N * N), rows * N * N, lane);
        fx.issue(state + p0 * N, rows * N, lane);
        fh.issue(regressor + p0 * W, rows * W, lane);
        fy.issue(meas + p0 * m, rows * m, lane);
        if (shared_cov) {
            // the measurement variances stay in LDS for the whole call (m is a run-time value)
            for (int j = 0; j < m; ++j) s_r[lane * SY + j] = meas_cov[j];
        } else {
            fr.issue(meas_cov + p0 * m, rows * m, lane);
            fr.commit(s_r, SY, m, rows * m, lane);
        }
        fp.commit(s_p, SP, N * N, rows * N * N, lane);
        fx.commit(s_x, SX, N, rows * N, lane);
        fh.commit(s_h, SH, W, rows * W, lane);
        fy.commit(s_y, SY, m, rows * m, lane);
    }
    __syncthreads();
    double x[N], P[NP];
    rls_state_read<N>(s_x, s_p, lane, x, P);
    for (int t = 0; t < steps; ++t) {
        if (t > 0) {
            const int64_t q0 = (int64_t)t * batch + p0;
            __syncthreads();   // the previous step's rows are consumed
            slab_load<kRT, 8>(s_h, SH, regressor + q0 * W, W, rows, W);
            slab_load<kRT, 2>(s_y, SY, meas + q0 * m, m, rows, m);
            __syncthreads();
        }
        if (lane < rows) {
            for (int j = 0; j < m; ++j) {
                double h[N];
#pragma unroll
                for (int c = 0; c < N; ++c) h[c] = s_h[lane * SH + j * N + c];
                rls_row<N>(x, P, h, s_y[lane * SY + j], s_r[lane * SY + j], lambda);
            }
#pragma unroll
            for (int i = 0; i < NP; ++i) P[i] = P[i] / lambda;
        }
    }
    // s_x / s_p were last read before the first step's arithmetic; every lane writes its own row
    rls_state_store<N>(s_x, s_p, state, cov, p0, rows, lane, x, P);
}

// The fused identification step: n = 2 (spring k, damper b), m = 6 (force, torque).
constexpr int kCRIn = 25;   // LDS row: twist 6 | pose 12 | wrench 6, odd stride
constexpr int kCRNull = 13;

__global__ __launch_bounds__(kRT) void contact_rls_kernel(
    double lambda, const double* __restrict__ meas_cov, int shared_cov,
    const double* __restrict__ geometry, int shared_geometry, const double* __restrict__ twist,
    const double* __restrict__ pose, const double* __restrict__ null_pose,
    const double* __restrict__ wrench, int steps, double* state, double* cov, int64_t batch)
{
    __shared__ double s_in[kRT * kCRIn];
    __shared__ double s_null[kRT * kCRNull];
    __shared__ double s_p[kRT * 5];
    __shared__ double s_x[kRT * 3];
    const int lane = threadIdx.x;
    const int64_t p0 = (int64_t)blockIdx.x * kRT;
    const int rows = (int)((batch - p0) < kRT ? (batch - p0) : kRT);
    const bool own = lane < rows;
    double r[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    double L = 0.0, Wd = 0.0;
    {
        // everything the first step needs, in flight together
        SlabRegs<2> fp;
        SlabRegs<1> fx;
        SlabRegs<6> fn, fq;
        SlabRegs<3> ft, fw;
        fp.issue(cov + p0 * 4, rows * 4, lane);
        fx.issue(state + p0 * 2, rows * 2, lane);
        fn.issue(null_pose + p0 * 12, rows * 12, lane);
        ft.issue(twist + p0 * 6, rows * 6, lane);
        fq.issue(pose + p0 * 12, rows * 12, lane);
        fw.issue(wrench + p0 * 6, rows * 6, lane);
        if (own) {
            const double* rq = shared_cov ? meas_cov : meas_cov + 6 * (p0 + lane);
#pragma unroll
            for (int j = 0; j < 6; ++j) r[j] = rq[j];
            const double* gq = shared_geometry ? geometry : geometry + 2 * (p0 + lane);
            L = gq[0];
            Wd = gq[1];
        }
        fp.commit(s_p, 5, 4, rows * 4, lane);
        fx.commit(s_x, 3, 2, rows * 2, lane);
        fn.commit(s_null, kCRNull, 12, rows * 12, lane);
        ft.commit(s_in, kCRIn, 6, rows * 6, lane);
        fq.commit(s_in + 6, kCRIn, 12, rows * 12, lane);
        fw.commit(s_in + 18, kCRIn, 6, rows * 6, lane);
    }
    __syncthreads();
    double x[2], P[3];
    rls_state_read<2>(s_x, s_p, lane, x, P);
    double ns[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) ns[i] = s_null[lane * kCRNull + i];
    for (int t = 0; t < steps; ++t) {
        if (t > 0) {
            const int64_t q0 = (int64_t)t * batch + p0;
            __syncthreads();
            slab_load<kRT, 4>(s_in, kCRIn, twist + q0 * 6, 6, rows, 6);
            slab_load<kRT, 8>(s_in + 6, kCRIn, pose + q0 * 12, 12, rows, 12);
            slab_load<kRT, 4>(s_in + 18, kCRIn, wrench + q0 * 6, 6, rows, 6);
            __syncthreads();
        }
        if (own) {
            double in[24];
#pragma unroll
            for (int i = 0; i < 24; ++i) in[i] = s_in[lane * kCRIn + i];
            double H[12];
            contact_regressor(L, Wd, in, in + 6, ns, H);
#pragma unroll
            for (int j = 0; j < 6; ++j) rls_row<2>(x, P, H + 2 * j, in[18 + j], r[j], lambda);
#pragma unroll
            for (int i = 0; i < 3; ++i) P[i] = P[i] / lambda;
        }
    }
    rls_state_store<2>(s_x, s_p, state, cov, p0, rows, lane, x, P);
}

template <int N>
void launch_rls_n(int m, double lambda, const double* meas_cov, int shared_cov,
                  const double* regressor, const double* meas, int steps, double* state,
                  double* cov, int64_t batch, hipStream_t s)
{
    hipLaunchKernelGGL(rls_advance_kernel<N>, dim3((unsigned)ceil_div(batch, kRT)), dim3(kRT), 0, s,
                       m, lambda, meas_cov, shared_cov, regressor, meas, steps, state, cov, batch);
}

}  // namespace

blf_status launch_rls_advance(int n, int m, double lambda, const double* meas_cov, int shared_cov,
                              const double* regressor, const double* meas, int32_t steps,
                              double* state, double* cov, int64_t batch, hipStream_t s)
{
    if (batch == 0) return BLF_OK;
    switch (n) {
    case 1: launch_rls_n<1>(m, lambda, meas_cov, shared_cov, regressor, meas, steps, state, cov, batch, s); break;
    case 2: launch_rls_n<2>(m, lambda, meas_cov, shared_cov, regressor, meas, steps, state, cov, batch, s); break;
    case 3: launch_rls_n<3>(m, lambda, meas_cov, shared_cov, regressor, meas, steps, state, cov, batch, s); break;
    case 4: launch_rls_n<4>(m, lambda, meas_cov, shared_cov, regressor, meas, steps, state, cov, batch, s); break;
    case 5: launch_rls_n<5>(m, lambda, meas_cov, shared_cov, regressor, meas, steps, state, cov, batch, s); break;
    case 6: launch_rls_n<6>(m, lambda, meas_cov, shared_cov, regressor, meas, steps, state, cov, batch, s); break;
    case 7: launch_rls_n<7>(m, lambda, meas_cov, shared_cov, regressor, meas, steps, state, cov, batch, s); break;
    case 8: launch_rls_n<8>(m, lambda, meas_cov, shared_cov, regressor, meas, steps, state, cov, batch, s); break;
    default: return set_error(BLF_ERR_UNSUPPORTED, "rls_advance_kernel: n=%d outside [1, %d]", n, BLF_RLS_MAX_STATE);
    }
    return check_hip(hipGetLastError(), "rls_advance_kernel launch");
}

blf_status launch_contact_rls(double lambda, const double* meas_cov, int shared_cov,
                              const double* geometry, int shared_geometry, const double* twist,
                              const double* pose, const double* null_pose, const double* wrench,
                              int32_t steps, double* state, double* cov, int64_t batch,
                              hipStream_t s)
{
    if (batch == 0) return BLF_OK;
    hipLaunchKernelGGL(contact_rls_kernel, dim3((unsigned)ceil_div(batch, kRT)), dim3(kRT), 0, s,
                       lambda, meas_cov, shared_cov, geometry, shared_geometry, twist, pose,
                       null_pose, wrench, steps, state, cov, batch);
    return check_hip(hipGetLastError(), "contact_rls_kernel launch");
}

}  // namespace blf
