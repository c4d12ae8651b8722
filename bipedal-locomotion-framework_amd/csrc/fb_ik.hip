// fb_ik.hip -- whole-body inverse kinematics on the device (include/blf/blf_c.h section 12):
// IK::QPInverseKinematics with SE3Task, CoMTask and JointTrackingTask at priority 1, H nu = g by
// Cholesky, and IntegrationBasedIK's loop (solve, one ForwardEuler<FloatingBaseSystemKinematics>
// step, ...) fused into one launch with the state in LDS.
// One wavefront per robot, or per two robots of at most 32 rows (Half), everything in LDS:
//   1. forward kinematics (build_topo + fbd_kinematics of fb_common.h, zero velocities);
//   2. lane per link: mass moments m_l, m_l c_l; lane per SE3 task: frame pose and target;
//      lane per column: the column of every task row (<= 27 rows) into LDS;
//   3. H, lane per row: row i's lower part in registers, one fma per (task row, column) with the
//      task rows read back as LDS broadcasts (dense: structurally zero columns are not skipped);
//      g_i alongside;
//   4. Cholesky and the two substitutions: fbd_eval's steps 8-9 (the IK's own copy);
//      HARD kernels (section 12b), between the substitutions: the hard rows through the forward
//      substitution, S = Y^T Y lane per row, its Cholesky with the relative pivot rule, lambda, and
//      z - Y lambda into the backward substitution;
//   5. nu to LDS (S.rhs()), from where the Euler step or the store takes it.
// Built without the iterative-ILP scheduler of fb_dynamics.hip: LLVM's register allocator crashes
// on the 54-row instantiation with it (the reason this kernel has a file of its own).
#include "fb_common.h"
#include "fbk_math.h"
#include "so3_math.h"

namespace blf {
namespace {

struct IkTasks {
    int K;
    const int32_t* frame;
    const double *w, *kp, *pose, *twist, *cw, *cpos, *cvel, *jw, *jkp, *jpos, *jvel;
    double ckp, damp;
};

// Section 12b's hard rows as the kernel takes them: bit t marks row t of the task-row table (the
// CoM bits moved down to 6 K), and the relative pivot bound of S.  Read by the HARD kernels only.
struct IkHard {
    unsigned slots;
    double tau;
};

constexpr int kIkRows = 6 * BLF_IK_MAX_SE3_TASKS + 3;   // task rows at most
constexpr int kIkTs = 11;   // per-task scratch: frame origin 3 | target 6 | link 1 (odd stride)
constexpr int kIkMc = 5;    // per-link mass moments: m | m c (odd stride)

struct IkSmem {
    Smem S;   // the kinematics' compact layout; the IK's arrays follow it
    int o_rows, o_wt, o_col, o_ts, o_mc, o_sp;
    int rs;   // task-row stride: the register row's width (columns past NV hold zeros)
    size_t total;
    __host__ __device__ IkSmem(double* b, int n, int K, int nvmax) : S(b, n, 0, true)
    {
        const int NV = n + 6;
        rs = nvmax;
        size_t o = S.total;
        auto take = [&](size_t k) {
            const int at = (int)o;
            o += (k + 1) & ~size_t(1);
            return at;
        };
        // the task rows [kIkRows][rs]; once H is in registers the same space holds L (NV rows)
        const size_t tr = (size_t)kIkRows * rs, lm = (size_t)NV * S.ms;
        o_rows = take(tr > lm ? tr : lm);
        o_wt = take(2 * (size_t)kIkRows);    // row weights | row targets
        o_col = take(4 * (size_t)NV);        // the factorization's pivot columns (two sets of two)
        o_ts = take((size_t)kIkTs * (K > 0 ? K : 1));
        o_mc = take((size_t)kIkMc * (n + 1));
        o_sp = take(18 * (size_t)K + 6 + 2 * (size_t)n);   // set points: pose | twist | com | joints
        total = o;
    }
    __device__ __forceinline__ double* rows() const { return S.base + o_rows; }
    __device__ __forceinline__ double* wt() const { return S.base + o_wt; }
    __device__ __forceinline__ double* col() const { return S.base + o_col; }
    __device__ __forceinline__ double* ts() const { return S.base + o_ts; }
    __device__ __forceinline__ double* mc() const { return S.base + o_mc; }
    __device__ __forceinline__ double* sp() const { return S.base + o_sp; }
};

// One solve for the robot whose state sits in S.st() (zero velocities | bp | bR | jp) and whose
// set points sit in I.sp().  Leaves nu in S.rhs(); false if a pivot was not finite and positive.
// HARD (section 12b): the rows of hd.slots hold exactly; hdep: a pivot of S failed its rule.
template <int NVMAX, int HW, bool PRI, bool HARD>
__device__ __forceinline__ bool ik_solve(const Model& m, const IkSmem& I, const IkTasks& tk, const Topo& T,
                                         const IkHard& hd, bool& hdep)
{
    static_assert(NVMAX <= HW, "a robot's rows must fit its lanes");
    const Half<HW> H;
    const Smem& S = I.S;
    const int n = m.n, L = n + 1, NV = n + 6, MS = S.ms, K = tk.K;
    int lane = H.hl;
    asm volatile("" : "+v"(lane));   // see fbd_eval
    double* loc = S.st();
    const double* jp = loc + 18 + n;
    const double* sp = I.sp();
    const bool com = tk.cw != nullptr;
    const int M = 6 * K + (com ? 3 : 0);
    // 1. kinematics
    fbd_kinematics<HW, PRI>(m, S, loc, loc + 6, loc + 6 + n, loc + 9 + n, jp, T);
    // 2a. lane per link: m_l and m_l c_l; lane per task: the frame's origin, the target twist, the link
    if (com && lane < L) {
        const double* k = S.link() + S.lrec * lane;
        const double* R = k + kR;
        const double* cl = m.com + 3 * lane;
        const double ms = m.mass[lane];
        double* o = I.mc() + kIkMc * lane;
        o[0] = ms;
        for (int a = 0; a < 3; ++a)
            o[1 + a] = ms * (k[kP + a] + ((R[3 * a] * cl[0] + R[3 * a + 1] * cl[1]) + R[3 * a + 2] * cl[2]));
    }
    if (lane < K) {
        int f = tk.frame[lane];
        f = (f >= 0 && f < m.F) ? f : 0;   // out of range: the robot is BLF_IK_BAD_INPUT already
        const int l = m.flink[f];
        double pose[12], tw[6], u[3], th;
        frame_state(S.link() + S.lrec * l, m.fpose + 12 * f, pose, tw);
        const double* des = sp + 12 * lane;
        const double* ff = sp + 12 * K + 6 * lane;
        so3_log_rel(des + 3, pose + 3, u, th);
        const double kpl = tk.kp[2 * lane], kpa = tk.kp[2 * lane + 1];
        double* o = I.ts() + kIkTs * lane;
        for (int a = 0; a < 3; ++a) {
            o[a] = pose[a];
            o[3 + a] = ff[a] + kpl * (des[a] - pose[a]);
            o[6 + a] = ff[3 + a] + kpa * (th * u[a]);
        }
        o[9] = (double)l;
    }
    wave_sync();
    // 2b. lane per column c: its motion (angular axis w about the point o, linear part u) and from
    //     it column c of every task row: u + w x (x - o) | w for a point x the column moves
    {
        const double* pB = S.link() + kP;
        const int j = lane >= 6 && lane < NV ? lane - 6 : 0;
        const bool jc = lane >= 6 && lane < NV;
        const bool pri = PRI && jc && m.jtype[j] == BLF_JOINT_PRISMATIC;
        double w[3], u[3], o[3];
        for (int a = 0; a < 3; ++a) {
            const double z = S.jz()[3 * j + a];
            w[a] = jc ? (pri ? 0.0 : z) : (lane == 3 + a ? 1.0 : 0.0);
            u[a] = jc ? (pri ? z : 0.0) : (lane == a ? 1.0 : 0.0);
            o[a] = jc ? S.jo()[3 * j + a] : pB[a];
        }
        double* rows = I.rows();
        for (int k = 0; k < K; ++k) {
            const double* t = I.ts() + kIkTs * k;
            const unsigned long long an = S.anc()[(int)t[9]];
            const bool moves = lane < 6 || (jc && ((an >> j) & 1ull));
            double d[3], cr[3];
            for (int a = 0; a < 3; ++a) d[a] = t[a] - o[a];
            cross3(w, d, cr);
            if (lane < NVMAX)
                for (int a = 0; a < 3; ++a) {
                    rows[(6 * k + a) * I.rs + lane] = moves ? u[a] + cr[a] : 0.0;
                    rows[(6 * k + 3 + a) * I.rs + lane] = moves ? w[a] : 0.0;
                }
        }
        if (com) {
            double tm = 0.0, th[3] = {0.0, 0.0, 0.0}, sm = 0.0, sh[3] = {0.0, 0.0, 0.0};
            for (int l = 0; l < L; ++l) {
                const double* q = I.mc() + kIkMc * l;
                const bool in = jc && ((S.anc()[l] >> j) & 1ull);
                tm = tm + q[0];
                sm = in ? sm + q[0] : sm;
                for (int a = 0; a < 3; ++a) {
                    th[a] = th[a] + q[1 + a];
                    sh[a] = in ? sh[a] + q[1 + a] : sh[a];
                }
            }
            double c[3], d[3], cr[3];
            for (int a = 0; a < 3; ++a) {
                c[a] = th[a] / tm;
                d[a] = jc ? (sh[a] - sm * o[a]) / tm : c[a] - o[a];
            }
            cross3(w, d, cr);
            const double us = jc ? sm / tm : 1.0;
            if (lane < NVMAX)
                for (int a = 0; a < 3; ++a) rows[(6 * K + a) * I.rs + lane] = lane < NV ? u[a] * us + cr[a] : 0.0;
            if (lane < 3) {
                const double* cd = sp + 18 * K;
                // (selects, not a lane-indexed array: that would live in scratch)
                const double ca = lane == 0 ? c[0] : lane == 1 ? c[1] : c[2];
                I.wt()[kIkRows + 6 * K + lane] = cd[3 + lane] + tk.ckp * (cd[lane] - ca);
                I.wt()[6 * K + lane] = tk.cw[lane];
            }
        }
        if (lane < 6 * K) {
            I.wt()[lane] = tk.w[lane];
            I.wt()[kIkRows + lane] = I.ts()[kIkTs * (lane / 6) + 3 + lane % 6];
        }
    }
    wave_sync();
    // 3. row `lane` of H (its lower part; the entries above the diagonal are never read) and g
    double r[NVMAX], y = 0.0;
#pragma unroll
    for (int j = 0; j < NVMAX; ++j) r[j] = 0.0;
    for (int t = 0; t < M; ++t) {
        const double wr = I.wt()[t];
        if (wr == 0.0) continue;   // a dropped row (the weights are shared: wave-uniform)
        const double* a = I.rows() + t * I.rs;
        const double ai = lane < NV ? a[lane < NVMAX ? lane : 0] * wr : 0.0;
        y = fma(ai, I.wt()[kIkRows + t], y);
#pragma unroll
        for (int j = 0; j < NVMAX; ++j) r[j] = fma(ai, a[j], r[j]);
    }
    {
        const int j = lane >= 6 && lane < NV ? lane - 6 : 0;
        const double jw = tk.jw[j];
        const double dg = lane < 6 ? tk.damp : lane < NV ? jw : 0.0;
        const double sd = sp[18 * K + 6 + n + j] + tk.jkp[j] * (sp[18 * K + 6 + j] - jp[j]);
        y = lane >= 6 && lane < NV ? y + jw * sd : y;
#pragma unroll
        for (int k = 0; k < NVMAX; ++k) r[k] = lane == k ? r[k] + dg : r[k];
    }
    // 4. Cholesky H = L L^T and the substitutions: fbd_eval's steps 8 and 9 (see there), with the
    //    pivot also required to be finite
    bool ok = true;
    constexpr int CB = 2;
    static_assert(NVMAX % CB == 0, "block size divides the register row");
#pragma unroll
    for (int k = 0; k < NVMAX; k += CB) {
        if (k < NV) {
            double Lb[CB][CB], il[CB];
#pragma unroll
            for (int i = 0; i < CB; ++i) {
                const bool in = k + i < NV;
#pragma unroll
                for (int j = 0; j < i; ++j) {
                    double t = in ? H.bcast_k(r[k + j], k + i) : 0.0;
#pragma unroll
                    for (int c = 0; c < j; ++c) t = t - Lb[i][c] * Lb[j][c];
                    Lb[i][j] = t * il[j];
                }
                double d = in ? H.bcast_k(r[k + i], k + i) : 1.0;
#pragma unroll
                for (int c = 0; c < i; ++c) d = d - Lb[i][c] * Lb[i][c];
                ok = ok && (d > 0.0) && (d <= 1.7976931348623157e308);
                double q = __builtin_amdgcn_rsq(d);
                il[i] = q * (1.5 - (0.5 * d) * (q * q));
                Lb[i][i] = d * il[i];
            }
            double li[CB];
#pragma unroll
            for (int i = 0; i < CB; ++i) {
                double t = r[k + i];
#pragma unroll
                for (int c = 0; c < i; ++c) t = t - li[c] * Lb[i][c];
                li[i] = t * il[i];
            }
            double* col = I.col() + ((k / CB) & 1) * CB * NV;
#pragma unroll
            for (int i = 0; i < CB; ++i) {
                r[k + i] = lane >= k ? li[i] : r[k + i];
                if (lane < NV && k + i < NV) col[i * NV + lane] = r[k + i];
            }
            wave_sync();
#pragma unroll
            for (int j = k + CB; j < NVMAX; ++j) {
                const int jj = j < NV ? j : NV - 1;
                double t = r[j];
#pragma unroll
                for (int i = CB - 1; i >= 0; --i) t = fma(-r[k + i], col[i * NV + jj], t);
                r[j] = t;
            }
        }
    }
    const double idg = lane < NV ? 1.0 / bcast_own_diag<NVMAX>(r, lane) : 0.0;
#pragma unroll
    for (int k = 0; k < NVMAX; ++k) {
        y = lane == k ? y * idg : y;
        const double xk = H.bcast_k(y, k);
        const double f = lane > k ? r[k] : 0.0;
        y = y - f * xk;
    }
    if constexpr (HARD) {
        // 4b. the hard rows (section 12b).  L's rows are still in r[], z = L^-1 g in y, and the task
        //     rows intact in I.rows().  Hard row i (in row order) belongs to lane i from step (ii) on.
        const unsigned hm = hd.slots;   // wave-uniform
        const int mh = __builtin_popcount(hm);
        bool hok = mh <= NV;   // more hard rows than unknowns: dependent (and the factor would not fit)
        if (hok) {
            double* rows = I.rows();
            const int cl = lane < NVMAX ? lane : 0;
            // (i) Y = L^-1 A_h^T: the forward substitution above on each hard row, three right-hand
            //     sides at a time (independent chains), y_t written back over row t
            constexpr int G = 3;
            for (unsigned rest = hm; rest != 0u;) {
                int t[G];
                double v[G];
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    t[g] = rest != 0u ? __builtin_ctz(rest) : -1;
                    rest = rest != 0u ? rest & (rest - 1u) : 0u;
                    v[g] = t[g] >= 0 && lane < NV ? rows[t[g] * I.rs + cl] : 0.0;
                }
#pragma unroll
                for (int k = 0; k < NVMAX; ++k) {
                    const double f = lane > k ? r[k] : 0.0;
#pragma unroll
                    for (int g = 0; g < G; ++g) {
                        v[g] = lane == k ? v[g] * idg : v[g];
                        const double xk = H.bcast_k(v[g], k);
                        v[g] = v[g] - f * xk;
                    }
                }
#pragma unroll
                for (int g = 0; g < G; ++g)
                    if (t[g] >= 0 && lane < NVMAX) rows[t[g] * I.rs + lane] = v[g];
            }
            if (lane < NV) S.rhs()[lane] = y;   // z, for the lanes of (ii)
            wave_sync();
            // (ii) lane i < m_h: row i of S = Y^T Y, indexed by table row (entries of soft rows stay
            //      0 and are never read), and q_i = y_i . z - b_i
            int own = 0;
            {
                int p = 0;
#pragma unroll
                for (int t = 0; t < kIkRows; ++t)
                    if ((hm >> t) & 1u) {
                        own = lane == p ? t : own;
                        ++p;
                    }
            }
            double sr[kIkRows], q = 0.0;
#pragma unroll
            for (int t = 0; t < kIkRows; ++t) sr[t] = 0.0;
            {
                const double* yo = rows + own * I.rs;
                const double* z = S.rhs();
                for (int c = 0; c < NV; ++c) {
                    const double yi = yo[c];
                    q = fma(yi, z[c], q);
#pragma unroll
                    for (int t = 0; t < kIkRows; ++t)
                        if ((hm >> t) & 1u) sr[t] = fma(yi, rows[t * I.rs + c], sr[t]);
                }
                q = q - I.wt()[kIkRows + own];
            }
            double d0 = 0.0;   // S_ii before elimination
#pragma unroll
            for (int t = 0; t < kIkRows; ++t) d0 = own == t ? sr[t] : d0;
            // (iii) S = C C^T, lane per row: pivot p (table row t) is lane p's sr[t]; column p of C
            //       goes to LDS packed (entries p..m_h-1), over the link records, which are dead
            //       until the next kinematics: m_h (m_h + 1) / 2 <= 27 (n + 1) since m_h <= min(27, NV)
            double* ct = S.link();
            double cdi = 0.0;   // 1 / C_ii of the lane's own row
            {
                int p = 0;
#pragma unroll
                for (int t = 0; t < kIkRows; ++t)
                    if ((hm >> t) & 1u) {
                        const double d = H.bcast_k(sr[t], p);
                        const double dd = H.bcast_k(d0, p);
                        hok = hok && (d > hd.tau * dd) && (d <= 1.7976931348623157e308);
                        const double qq = __builtin_amdgcn_rsq(d);
                        const double il = qq * (1.5 - (0.5 * d) * (qq * qq));
                        const double l = sr[t] * il;
                        sr[t] = l;
                        cdi = lane == p ? il : cdi;
                        double* col = ct + (p * mh - (p * (p - 1)) / 2);
                        if (lane >= p && lane < mh) col[lane - p] = l;
                        wave_sync();
                        int pu = 1;
#pragma unroll
                        for (int u = t + 1; u < kIkRows; ++u)
                            if ((hm >> u) & 1u) {
                                sr[u] = fma(-l, col[pu], sr[u]);
                                ++pu;
                            }
                        ++p;
                    }
            }
            // (iv) lambda = C^-T C^-1 q
            {
                int p = 0;
#pragma unroll
                for (int t = 0; t < kIkRows; ++t)
                    if ((hm >> t) & 1u) {
                        q = lane == p ? q * cdi : q;
                        const double xk = H.bcast_k(q, p);
                        const double f = lane > p ? sr[t] : 0.0;
                        q = q - f * xk;
                        ++p;
                    }
            }
            {
                const int li = lane < mh ? lane : 0;
                const double* mycol = ct + (li * mh - (li * (li - 1)) / 2) - li;   // C[p][lane] at [p]
                for (int p = mh - 1; p >= 0; --p) {
                    q = lane == p ? q * cdi : q;
                    const double xk = H.bcast_k(q, p);
                    const double f = lane < p ? mycol[p] : 0.0;
                    q = q - f * xk;
                }
            }
            // (v) z - Y lambda
            {
                int p = 0;
#pragma unroll
                for (int t = 0; t < kIkRows; ++t)
                    if ((hm >> t) & 1u) {
                        const double lam = H.bcast_k(q, p);
                        const double yt = lane < NV ? rows[t * I.rs + cl] : 0.0;
                        y = y - yt * lam;
                        ++p;
                    }
            }
            wave_sync();   // the rows are read; L goes over them next
        }
        hdep = !hok;
    }
    double* Lr = I.rows();
    if (lane < NV)
#pragma unroll
        for (int j = 0; j < NVMAX; ++j)
            if (j < NV && j <= lane) Lr[MS * lane + j] = r[j];
    wave_sync();
    double lki = (lane < NV - 1) ? Lr[MS * (NV - 1) + lane] : 0.0;
    for (int k = NV - 1; k >= 0; --k) {
        const double lnext = (k > 0 && lane < k - 1) ? Lr[MS * (k - 1) + lane] : 0.0;
        if (lane == k) y = y * idg;
        const double xk = H.bcast_k(y, k);
        if (lane < k) y = y - lki * xk;
        lki = lnext;
    }
    // 5. nu
    if (lane < NV) S.rhs()[lane] = y;
    wave_sync();
    return H.ballot(!ok) == 0ull;
}

// blf_fb_ik_solve (steps == 0) and blf_fb_ik_integrate (steps >= 1): the set points staged in LDS
// once, the state in LDS over all the steps.
template <int NVMAX, int HW, bool PRI, bool HARD>
__global__ __launch_bounds__(64) void fb_ik_kernel(Model m, blf_fb_state st, IkTasks tk, int32_t steps,
                                                   double dT, double* __restrict__ nu,
                                                   int32_t* __restrict__ status, int64_t batch, IkHard hd)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const Half<HW> H;
    const int n = m.n, NV = n + 6, K = tk.K;
    const IkSmem I(smem + H.half * IkSmem(nullptr, n, K, NVMAX).total, n, K, NVMAX);
    const Smem& S = I.S;
    const int lane = H.hl;
    constexpr int per = kWave / HW;   // robots per wavefront
    const Topo T = build_topo<HW>(m, S);
    const int64_t i0 = (int64_t)blockIdx.x * per + H.half;
    const bool active = i0 < batch;   // see fbd_dynamics_kernel
    const int64_t q = active ? i0 : batch - 1;
    double* loc = S.st();   // zeros 6 + n (the velocities the kinematics takes) | bp 3 | bR 9 | jp n | dR 9
    double* dR = loc + 18 + 2 * n;
    for (int i = lane; i < 18 + 2 * n; i += HW) {
        double v = 0.0;
        if (i < 6 + n) v = 0.0;
        else if (i < 9 + n) v = st.base_pos[3 * q + (i - 6 - n)];
        else if (i < 18 + n) v = st.base_rot[9 * q + (i - 9 - n)];
        else v = st.joint_pos[(int64_t)n * q + (i - 18 - n)];
        loc[i] = v;
    }
    bool fin = true;
    for (int i = lane; i < 18 * K + 6 + 2 * n; i += HW) {
        double v = 0.0;
        if (i < 12 * K) v = tk.pose[q * 12 * K + i];
        else if (i < 18 * K) v = tk.twist ? tk.twist[q * 6 * K + (i - 12 * K)] : 0.0;
        else if (i < 18 * K + 3) v = tk.cw ? tk.cpos[3 * q + (i - 18 * K)] : 0.0;
        else if (i < 18 * K + 6) v = tk.cw && tk.cvel ? tk.cvel[3 * q + (i - 18 * K - 3)] : 0.0;
        else if (i < 18 * K + 6 + n) v = tk.jpos[(int64_t)n * q + (i - 18 * K - 6)];
        else v = tk.jvel ? tk.jvel[(int64_t)n * q + (i - 18 * K - 6 - n)] : 0.0;
        I.sp()[i] = v;
        fin = fin && so3_finite(v);
    }
    bool fbad = false;   // the frame indices are shared by the batch
    for (int k = 0; k < K; ++k) {
        const int f = tk.frame[k];
        fbad = fbad || f < 0 || f >= m.F;
    }
    const bool spbad = fbad || H.ballot(!fin) != 0ull;
    wave_sync();
    int stat = BLF_IK_OK;   // this robot's (the same in every lane of its half)
    const int iters = steps > 0 ? steps : 1;
    for (int it = 0; it < iters; ++it) {
        const bool alive = stat == BLF_IK_OK;
        if (!__ballot(alive)) break;
        bool sfin = true;
        for (int i = lane; i < 12 + n; i += HW) sfin = sfin && so3_finite(loc[6 + n + i]);
        const bool bad = spbad || H.ballot(!sfin) != 0ull;
        bool hdep = false;
        const bool ok = ik_solve<NVMAX, HW, PRI, HARD>(m, I, tk, T, hd, hdep);
        const int s1 = bad ? BLF_IK_BAD_INPUT
                       : !ok ? BLF_IK_NOT_POSITIVE
                       : HARD && hdep ? BLF_IK_HARD_DEPENDENT : BLF_IK_OK;
        stat = alive ? s1 : stat;
        if (steps > 0) {
            // one step of blf_fbk_euler_integrate with nu as its input; a failed robot stays where it is
            const bool go = stat == BLF_IK_OK;
            if (lane == 0) fbk_rot_rate(m.rho, loc + 9 + n, S.rhs() + 3, dR);
            wave_sync();
            if (go)
                for (int i = lane; i < 12 + n; i += HW) {
                    if (i < 3) loc[6 + n + i] = loc[6 + n + i] + S.rhs()[i] * dT;
                    else if (i < 12) loc[6 + n + i] = loc[6 + n + i] + dR[i - 3] * dT;
                    else loc[18 + n + (i - 12)] = loc[18 + n + (i - 12)] + S.rhs()[6 + (i - 12)] * dT;
                }
            wave_sync();
        }
    }
    if (!active) return;
    const double nan = __builtin_nan("");
    for (int c = lane; c < NV; c += HW) {
        const double v = stat == BLF_IK_OK ? S.rhs()[c] : nan;
        if (nu) nu[(int64_t)NV * q + c] = v;
        if (steps > 0) {
            if (c < 6) st.base_vel[6 * q + c] = v;
            else st.joint_vel[(int64_t)n * q + (c - 6)] = v;
        }
    }
    if (steps > 0)
        for (int i = lane; i < 12 + n; i += HW) {
            const double v = loc[6 + n + i];
            if (i < 3) st.base_pos[3 * q + i] = v;
            else if (i < 12) st.base_rot[9 * q + (i - 3)] = v;
            else st.joint_pos[(int64_t)n * q + (i - 12)] = v;
        }
    if (status && lane == 0) status[q] = stat;
}

}  // namespace

// Two robots per wavefront while a robot's rows fit half of one (n + 6 <= 32), as the dynamics
// kernels: at n = 24, B = 16 384 the solve takes 0.431 ms with two robots per wavefront and 0.965 ms
// with one, and 20 fused steps 6.29 against 15.24 ms (profiles/ik_bench.log).
size_t fb_ik_lds_bytes(int n, int K)
{
    return n + 6 <= 32 ? 2 * sizeof(double) * IkSmem(nullptr, n, K, 32).total
                       : sizeof(double) * IkSmem(nullptr, n, K, BLF_FBD_MAX_DOFS + 6).total;
}

// slots == 0: the soft kernels (section 12); otherwise the HARD ones (section 12b)
blf_status launch_fb_ik(const blf_fb_model* md, const blf_fb_state* st, const blf_ik_tasks* t, int64_t batch,
                        int32_t steps, double dT, double* nu, int32_t* status, hipStream_t s,
                        uint32_t slots, double tau)
{
    if (batch == 0) return BLF_OK;
    IkTasks tk;
    tk.K = t->nse3;
    tk.frame = t->frame;
    tk.w = t->se3_weight;
    tk.kp = t->se3_kp;
    tk.pose = t->se3_pose;
    tk.twist = t->se3_twist;
    tk.cw = t->com_weight;
    tk.cpos = t->com_pos;
    tk.cvel = t->com_vel;
    tk.jw = t->joint_weight;
    tk.jkp = t->joint_kp;
    tk.jpos = t->joint_pos;
    tk.jvel = t->joint_vel;
    tk.ckp = t->com_kp;
    tk.damp = t->base_damping;
    const bool pri = md->joint_type != nullptr;
    const size_t lds = fb_ik_lds_bytes(md->ndof, tk.K);
    const IkHard hd{slots, tau};
    constexpr int NW = BLF_FBD_MAX_DOFS + 6;
    if (md->ndof + 6 <= 32) {
        auto kern = slots ? (pri ? fb_ik_kernel<32, 32, true, true> : fb_ik_kernel<32, 32, false, true>)
                          : (pri ? fb_ik_kernel<32, 32, true, false> : fb_ik_kernel<32, 32, false, false>);
        hipLaunchKernelGGL(kern, dim3((unsigned)ceil_div(batch, 2)), dim3(kWave), lds, s, to_model(md), *st, tk,
                           steps, dT, nu, status, batch, hd);
    } else {
        auto kern = slots ? (pri ? fb_ik_kernel<NW, kWave, true, true> : fb_ik_kernel<NW, kWave, false, true>)
                          : (pri ? fb_ik_kernel<NW, kWave, true, false> : fb_ik_kernel<NW, kWave, false, false>);
        hipLaunchKernelGGL(kern, dim3((unsigned)batch), dim3(kWave), lds, s, to_model(md), *st, tk, steps, dT, nu,
                           status, batch, hd);
    }
    return check_hip(hipGetLastError(), "fb_ik_kernel launch");
}

}  // namespace blf
