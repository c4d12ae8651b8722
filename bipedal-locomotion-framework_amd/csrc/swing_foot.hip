// swing_foot.hip — SE(3) swing-foot trajectories over contact lists (SwingFootPlanner) and
// minimum-jerk SO(3) trajectories (SO3Planner); include/blf/blf_c.h section 11 is normative.
//
// swing_foot_eval_kernel: one lane per (list, query), 256 queries per workgroup.  A query reads
// 8 B and writes up to 200 B, so the kernel is a store stream: the outputs leave through slab.h
// (16-B non-temporal stores), the pose slab first and the twist / acceleration slabs after it in
// the same LDS buffer (one 24-double slab would be 51 KB a workgroup, three workgroups a CU; in
// turn it is 28 KB, and four fit).  The per-swing work (quaternion, atan2, divisions, six coefficient sets) is done
// once per (list, swing) of the workgroup's few consecutive lists, seven lanes a swing, into LDS
// records that the query lanes read after a barrier.  Workgroups whose lists do not fit the staging
// buffers (few queries per list) let every lane fit its own segment instead: the same expressions,
// the same bits.
#include "blf_internal.h"
#include "quintic_math.h"
#include "slab.h"
#include "so3_math.h"

namespace blf {
namespace {

constexpr int kSwBlock = 256;    // queries per workgroup
constexpr int kSwTab = 512;      // doubles of staged contact tables (poses + times) per workgroup
constexpr int kSwMaxRec = 24;    // staged (list, swing) records per workgroup
constexpr int kSwMaxLists = 36;  // kSwTab / 14 lists at one contact each
constexpr int kSwParts = 7;      // fit lanes per swing: 2 segments x 3 axes, and the rotation
// record: [0] apex time, [1] theta, [2..4] unit axis, [5 + (seg * 3 + axis) * 6 ..] coefficients
constexpr int kSwRec = 41;

struct SwingPrm {
    double h, rho, vland, aland;
};

// Coefficients of segment `seg` (0: lift -> apex, 1: apex -> land), axis d, of the swing from
// position pa at t0 to pb at t1 (section 11's knots).
__device__ __forceinline__ void swing_fit_axis(int seg, int d, const double* pa, const double* pb,
                                               double t0, double t1, const SwingPrm& prm, double* c)
{
    const double T = t1 - t0;
    const double tm = (1.0 - prm.rho) * t0 + prm.rho * t1;
    double pm, vm;
    if (d < 2) {
        pm = (1.0 - prm.rho) * pa[d] + prm.rho * pb[d];
        vm = (pb[d] - pa[d]) / T;
    } else {
        pm = (pa[2] > pb[2] ? pa[2] : pb[2]) + prm.h;
        vm = 0.0;
    }
    if (seg == 0)
        quintic_fit_coeffs(tm - t0, pa[d], 0.0, 0.0, pm, vm, 0.0, c);
    else
        quintic_fit_coeffs(t1 - tm, pm, vm, 0.0, pb[d], d == 2 ? prm.vland : 0.0,
                           d == 2 ? prm.aland : 0.0, c);
}

// LDS (40 KB) lets four workgroups share a CU: keep the registers at 4 waves per SIMD too
__global__ __launch_bounds__(kSwBlock) __attribute__((amdgpu_waves_per_eu(4)))
void swing_foot_eval_kernel(
    const double* __restrict__ cpose, const double* __restrict__ ctime,
    const int32_t* __restrict__ ncontacts, int32_t C, int64_t L, const double* __restrict__ tq,
    int32_t Q, SwingPrm prm, double* __restrict__ pose, double* __restrict__ twist,
    double* __restrict__ accel, int32_t* __restrict__ cidx, int32_t* __restrict__ incontact)
{
    __shared__ __attribute__((aligned(16))) double s_out[kSwBlock * 14];
    __shared__ __attribute__((aligned(16))) double s_tab[kSwTab];
    __shared__ double s_rec[kSwMaxRec * kSwRec];
    __shared__ int s_n[kSwMaxLists];     // contacts of each staged list (0: none usable)
    __shared__ int s_bad[kSwMaxLists];   // the list poisons its queries
    const int tid = threadIdx.x;
    const int64_t total = L * Q;
    const int64_t g0 = (int64_t)blockIdx.x * kSwBlock;
    const int64_t gid = g0 + tid;
    const int rows = (int)((total - g0) < kSwBlock ? (total - g0) : kSwBlock);
    const bool small = total < 0x7fffffffLL;   // 32-bit division when the launch fits
    auto list_of = [&](int64_t g) { return small ? (int64_t)((uint32_t)g / (uint32_t)Q) : g / Q; };
    const int64_t l0 = list_of(g0);
    const int nl = (int)(list_of(g0 + rows - 1) - l0 + 1);
    const int nrec = nl * (C - 1);
    const bool staged = nl * C * 14 <= kSwTab && nrec <= kSwMaxRec;
    const double kNaN = __builtin_nan("");

    double tt = 0.0;
    if (gid < total) tt = __builtin_nontemporal_load(tq + gid);   // streamed once
    double* s_pose = s_tab;
    double* s_time = s_tab + nl * C * 12;
    if (staged) {
        // the lists' tables are contiguous: coalesced, in flight together with the query times
        const double* gp = cpose + l0 * C * 12;
        const double* gt = ctime + l0 * C * 2;
        for (int j = tid; j < nl * C * 12; j += kSwBlock) s_pose[j] = gp[j];
        for (int j = tid; j < nl * C * 2; j += kSwBlock) s_time[j] = gt[j];
        if (tid < nl) {
            const int n = ncontacts[l0 + tid];
            const bool ok = n >= 1 && n <= C;
            s_n[tid] = ok ? n : 0;
            s_bad[tid] = ok ? 0 : 1;
        }
        __syncthreads();
        // a non-finite pose or time among a list's contacts poisons the list
        if (tid < nl * C) {
            const int ll = tid / C, c = tid - ll * C;
            if (c < s_n[ll]) {
                bool fin = so3_finite(s_time[tid * 2]) && so3_finite(s_time[tid * 2 + 1]);
                for (int e = 0; e < 12; ++e) fin = fin && so3_finite(s_pose[tid * 12 + e]);
                if (!fin) s_bad[ll] = 1;
            }
        }
        // each (list, swing) fitted once: lane j does part j % 7 of swing j / 7
        if (tid < nrec * kSwParts) {
            const int r = tid / kSwParts, part = tid - r * kSwParts;
            const int ll = r / (C - 1), c = r - ll * (C - 1);
            if (c + 1 < s_n[ll]) {
                const double* pa = s_pose + (ll * C + c) * 12;
                const double* pb = pa + 12;
                const double t0 = s_time[(ll * C + c) * 2 + 1];
                const double t1 = s_time[(ll * C + c + 1) * 2];
                double* rec = s_rec + r * kSwRec;
                if (part < 6) {
                    const int seg = part >= 3 ? 1 : 0;
                    swing_fit_axis(seg, part - 3 * seg, pa, pb, t0, t1, prm, rec + 5 + part * 6);
                } else {
                    double u[3], theta;
                    so3_log_rel(pb + 3, pa + 3, u, theta);
                    rec[0] = (1.0 - prm.rho) * t0 + prm.rho * t1;
                    rec[1] = theta;
                    rec[2] = u[0];
                    rec[3] = u[1];
                    rec[4] = u[2];
                }
            }
        }
        __syncthreads();
    }

    double P[12], V[6], A[6];
#pragma unroll
    for (int e = 0; e < 6; ++e) V[e] = A[e] = 0.0;
#pragma unroll
    for (int e = 0; e < 12; ++e) P[e] = 0.0;
    if (gid < total) {
        const int64_t l = list_of(gid);
        const int ll = (int)(l - l0);
        const double* tb = staged ? s_time + ll * C * 2 : ctime + l * C * 2;
        const double* pb0 = staged ? s_pose + ll * C * 12 : cpose + l * C * 12;
        int n;
        bool bad;
        if (staged) {
            n = s_n[ll];
            bad = s_bad[ll] != 0;
        } else {
            n = ncontacts[l];
            bad = !(n >= 1 && n <= C);
            if (bad) n = 0;
            for (int c = 0; c < n; ++c) {
                bool fin = so3_finite(tb[2 * c]) && so3_finite(tb[2 * c + 1]);
                for (int e = 0; e < 12; ++e) fin = fin && so3_finite(pb0[c * 12 + e]);
                bad = bad || !fin;
            }
        }
        bad = bad || !so3_finite(tt);
        int raw = -1, ic = 0;
        if (bad) {
#pragma unroll
            for (int e = 0; e < 12; ++e) P[e] = kNaN;
#pragma unroll
            for (int e = 0; e < 6; ++e) V[e] = A[e] = kNaN;
        } else {
            for (int c = 0; c < n; ++c)
                if (tb[2 * c] <= tt) raw = c;   // the last contact with activation <= t
            const int cs = raw < 0 ? 0 : raw;
            const double* pa = pb0 + cs * 12;
            const bool stance = raw >= 0 && tt < tb[2 * cs + 1];
            const bool swing = raw >= 0 && !stance && raw < n - 1;
            ic = stance ? 1 : 0;
            if (!swing) {
#pragma unroll
                for (int e = 0; e < 12; ++e) P[e] = pa[e];   // bit for bit
            } else {
                const double* pn = pa + 12;
                const double t0 = tb[2 * cs + 1], t1 = tb[2 * cs + 2];
                const double* rec = s_rec + (staged ? (ll * (C - 1) + cs) * kSwRec : 0);
                const double tm = staged ? rec[0] : (1.0 - prm.rho) * t0 + prm.rho * t1;
                const int seg = tm <= tt ? 1 : 0;   // the segment of the last knot <= t
                const double tl = tt - (seg ? tm : t0);
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    double c[6];
                    if (staged) {
#pragma unroll
                        for (int i = 0; i < 6; ++i) c[i] = rec[5 + (seg * 3 + d) * 6 + i];
                    } else {
                        swing_fit_axis(seg, d, pa, pn, t0, t1, prm, c);
                    }
                    quintic_horner(tl, c[0], c[1], c[2], c[3], c[4], c[5], P[d], V[d], A[d]);
                }
                double u[3], theta;
                if (staged) {
                    theta = rec[1];
                    u[0] = rec[2];
                    u[1] = rec[3];
                    u[2] = rec[4];
                } else {
                    so3_log_rel(pn + 3, pa + 3, u, theta);
                }
                if (theta == 0.0) {
#pragma unroll
                    for (int e = 3; e < 12; ++e) P[e] = pa[e];   // no rotation: R_raw bit for bit
                } else {
                    const double T = t1 - t0;
                    const double tau = (tt - t0) / T;
                    double s, sd, sdd;
                    so3_min_jerk(tau, T, s, sd, sdd);
                    so3_exp_apply(s * theta, u, pa + 3, P + 3);
#pragma unroll
                    for (int d = 0; d < 3; ++d) {
                        const double phi = theta * u[d];
                        V[3 + d] = sd * phi;
                        A[3 + d] = sdd * phi;
                    }
                }
            }
        }
        if (cidx) __builtin_nontemporal_store(raw, cidx + gid);
        if (incontact) __builtin_nontemporal_store(ic, incontact + gid);
        // the pose goes to its slab row at once (12 doubles fewer held across the barrier)
        if (pose) {
            double* o = s_out + tid * 13;
#pragma unroll
            for (int e = 0; e < 12; ++e) o[e] = P[e];
        }
    }
    if (pose) {
        __syncthreads();
        slab_store<kSwBlock, 6>(pose + g0 * 12, 12, s_out, 13, rows, 12);
        __syncthreads();
    }
    if (twist || accel) {
        double* ov = s_out + tid * 7;
        double* oa = s_out + kSwBlock * 7 + tid * 7;
#pragma unroll
        for (int e = 0; e < 6; ++e) {
            ov[e] = V[e];
            oa[e] = A[e];
        }
        __syncthreads();
        if (twist) slab_store<kSwBlock, 3>(twist + g0 * 6, 6, s_out, 7, rows, 6);
        if (accel) slab_store<kSwBlock, 3>(accel + g0 * 6, 6, s_out + kSwBlock * 7, 7, rows, 6);
    }
}

// one lane per (trajectory, query): R(t) = Exp(s phi) R0, omega = ds/dt phi, alpha = d2s/dt2 phi
__global__ __launch_bounds__(kSwBlock) void so3_eval_kernel(
    const double* __restrict__ R0, const double* __restrict__ R1, const double* __restrict__ duration,
    int64_t S, const double* __restrict__ tq, int32_t Q, double* __restrict__ rot,
    double* __restrict__ omega, double* __restrict__ alpha)
{
    __shared__ __attribute__((aligned(16))) double s_out[kSwBlock * 9];
    const int tid = threadIdx.x;
    const int64_t total = S * Q;
    const int64_t g0 = (int64_t)blockIdx.x * kSwBlock;
    const int64_t gid = g0 + tid;
    const int rows = (int)((total - g0) < kSwBlock ? (total - g0) : kSwBlock);
    const bool small = total < 0x7fffffffLL;
    const double kNaN = __builtin_nan("");
    double R[9], W[3], Al[3];
#pragma unroll
    for (int e = 0; e < 9; ++e) R[e] = 0.0;
#pragma unroll
    for (int e = 0; e < 3; ++e) W[e] = Al[e] = 0.0;
    if (gid < total) {
        const double tt = __builtin_nontemporal_load(tq + gid);
        const int64_t sp = small ? (int64_t)((uint32_t)gid / (uint32_t)Q) : gid / Q;
        const double T = duration[sp];
        double a[9], b[9];
        bool fin = so3_finite(tt) && so3_finite(T) && T > 0.0;
#pragma unroll
        for (int e = 0; e < 9; ++e) {
            a[e] = R0[sp * 9 + e];
            b[e] = R1[sp * 9 + e];
            fin = fin && so3_finite(a[e]) && so3_finite(b[e]);
        }
        if (!fin) {
#pragma unroll
            for (int e = 0; e < 9; ++e) R[e] = kNaN;
#pragma unroll
            for (int e = 0; e < 3; ++e) W[e] = Al[e] = kNaN;
        } else {
            double u[3], theta;
            so3_log_rel(b, a, u, theta);
            if (theta == 0.0) {
#pragma unroll
                for (int e = 0; e < 9; ++e) R[e] = a[e];
            } else {
                const double tc = tt < 0.0 ? 0.0 : (tt > T ? T : tt);
                const double tau = tc / T;
                double s, sd, sdd;
                so3_min_jerk(tau, T, s, sd, sdd);
                so3_exp_apply(s * theta, u, a, R);
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    const double phi = theta * u[d];
                    W[d] = sd * phi;
                    Al[d] = sdd * phi;
                }
            }
        }
    }
    if (rot) {
#pragma unroll
        for (int e = 0; e < 9; ++e) s_out[tid * 9 + e] = R[e];
        __syncthreads();
        slab_store<kSwBlock, 5>(rot + g0 * 9, 9, s_out, 9, rows, 9);
        __syncthreads();
    }
    if (omega || alpha) {
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            s_out[tid * 3 + e] = W[e];
            s_out[kSwBlock * 3 + tid * 3 + e] = Al[e];
        }
        __syncthreads();
        if (omega) slab_store<kSwBlock, 2>(omega + g0 * 3, 3, s_out, 3, rows, 3);
        if (alpha) slab_store<kSwBlock, 2>(alpha + g0 * 3, 3, s_out + kSwBlock * 3, 3, rows, 3);
    }
}

}  // namespace

blf_status launch_swing_foot_eval(const blf_swing_foot_params* p, const double* cpose,
                                  const double* ctime, const int32_t* ncontacts, int64_t L,
                                  const double* tq, int32_t Q, double* pose, double* twist,
                                  double* accel, int32_t* cidx, int32_t* incontact, hipStream_t s)
{
    const int64_t n = L * Q;
    if (n == 0) return BLF_OK;
    const SwingPrm prm{p->step_height, p->apex_ratio, p->landing_velocity, p->landing_acceleration};
    hipLaunchKernelGGL(swing_foot_eval_kernel, dim3((unsigned)ceil_div(n, kSwBlock)), dim3(kSwBlock),
                       0, s, cpose, ctime, ncontacts, p->max_contacts, L, tq, Q, prm, pose, twist,
                       accel, cidx, incontact);
    return check_hip(hipGetLastError(), "swing_foot_eval_kernel launch");
}

blf_status launch_so3_eval(const double* R0, const double* R1, const double* duration, int64_t S,
                           const double* tq, int32_t Q, double* rot, double* omega, double* alpha,
                           hipStream_t s)
{
    const int64_t n = S * Q;
    if (n == 0) return BLF_OK;
    hipLaunchKernelGGL(so3_eval_kernel, dim3((unsigned)ceil_div(n, kSwBlock)), dim3(kSwBlock), 0, s,
                       R0, R1, duration, S, tq, Q, rot, omega, alpha);
    return check_hip(hipGetLastError(), "so3_eval_kernel launch");
}

}  // namespace blf
