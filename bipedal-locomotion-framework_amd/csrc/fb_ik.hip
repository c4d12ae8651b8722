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
// LIMITS kernels (section 12c, fb_ik_limits_kernel): an active-set iteration around steps 2b-5 on the
// joints held at a bound of their velocity box, which step 3b eliminates from the system in place.
// TRACK kernel (section 12d, fb_ik_track_kernel): the LIMITS loop with the set points and each robot's
// own hard rows of step t (ik_solve's TRACK: the union of a wavefront's two masks, null rows).
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
    int o_rows, o_wt, o_col, o_ts, o_mc, o_sp, o_lim;
    int rs;   // task-row stride: the register row's width (columns past NV hold zeros)
    size_t total;
    // lim: the LIMITS kernels' block (section 12c); without it the layout is that of sections 12, 12b
    __host__ __device__ IkSmem(double* b, int n, int K, int nvmax, bool lim = false) : S(b, n, 0, true)
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
        // the velocity box lo n | up n, the value each fixed joint is held at n, the base position 3
        o_lim = take(lim ? 3 * (size_t)n + 3 : 0);
        total = o;
    }
    __device__ __forceinline__ double* rows() const { return S.base + o_rows; }
    __device__ __forceinline__ double* wt() const { return S.base + o_wt; }
    __device__ __forceinline__ double* col() const { return S.base + o_col; }
    __device__ __forceinline__ double* ts() const { return S.base + o_ts; }
    __device__ __forceinline__ double* mc() const { return S.base + o_mc; }
    __device__ __forceinline__ double* sp() const { return S.base + o_sp; }
    __device__ __forceinline__ double* lo() const { return S.base + o_lim; }
    __device__ __forceinline__ double* up(int n) const { return S.base + o_lim + n; }
    __device__ __forceinline__ double* fx(int n) const { return S.base + o_lim + 2 * n; }
    __device__ __forceinline__ double* pb(int n) const { return S.base + o_lim + 3 * n; }
};

// fb_ik_track_kernel's layout (section 12d): the LIMITS one, and room for the packed factor of S where
// the link records cannot hold it (a wavefront's two robots factor the union of their hard rows, up to
// min(27, 6 K + 3) of them whatever n is).  A struct of its own, which ik_solve takes as a template
// argument: a field in IkSmem would be carried by every IK kernel.
struct IkTrackSmem : IkSmem {
    int o_cf;
    __host__ __device__ IkTrackSmem(double* b, int n, int K, int nvmax) : IkSmem(b, n, K, nvmax, true)
    {
        const int mu = 6 * K + 3 < kIkRows ? 6 * K + 3 : kIkRows;
        const size_t cf = (size_t)mu * (mu + 1) / 2;
        o_cf = S.o_link;
        if (cf > (size_t)S.lrec * (n + 1)) {
            o_cf = (int)total;
            total += (cf + 1) & ~size_t(1);
        }
    }
    __device__ __forceinline__ double* cf() const { return S.base + o_cf; }
};

// One solve for the robot whose state sits in S.st() (zero velocities | bp | bR | jp) and whose
// set points sit in I.sp().  Leaves nu in S.rhs(); false if a pivot was not finite and positive.
// HARD (section 12b): the rows of hd.slots hold exactly; hdep: a pivot of S failed its rule.
// LIMITS (section 12c) runs it in phases, PH: kPrep steps 1-2a once per state, kRows step 2b (again
// after every solve: L and Y overwrite the rows), kSolve steps 3-5 with the joints of `wm` (bit j:
// joint j, this lane's robot) fixed at I.fx(): they are eliminated from the system in place, a fixed
// lane's row of H becoming e_i and its g_i the bound, a free lane's fixed columns moving to g_i.  The
// hard rows' multipliers are then left in I.col() by table row.
// TRACK (section 12d, SM = IkTrackSmem): the hard rows differ between the two robots of a wavefront.
// hd.slots is the union of their masks (wave-uniform, so the unrolled loops of 4b stay scalar
// branches) and `hme` this robot's own.  A row of the union that this robot does not hold is a null
// row: its y is 0, its row of S is e_i and its q is 0, so it passes the pivot rule with lambda = 0 and
// adds exact zeros to every other row: the robot's own rows see the arithmetic they see alone.  The
// union may count more than NV rows (each robot's own count is judged by the kernel), and S's packed
// factor goes to I.cf().
constexpr int kPrep = 1, kRows = 2, kSolve = 4;
template <int NVMAX, int HW, bool PRI, bool HARD, bool LIMITS = false, int PH = kPrep | kRows | kSolve,
          bool TRACK = false, class SM = IkSmem>
__device__ __forceinline__ bool ik_solve(const Model& m, const SM& I, const IkTasks& tk, const Topo& T,
                                         const IkHard& hd, bool& hdep, unsigned long long wm = 0ull,
                                         unsigned hme = 0u)
{
    static_assert(NVMAX <= HW, "a robot's rows must fit its lanes");
    static_assert(LIMITS || PH == (kPrep | kRows | kSolve), "only the LIMITS kernels run in phases");
    static_assert(HARD || !LIMITS, "the LIMITS kernels are built on the HARD ones (slots may be 0)");
    static_assert(!TRACK || (HARD && LIMITS), "the TRACK kernel is built on the LIMITS ones");
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
    if constexpr ((PH & kPrep) != 0) fbd_kinematics<HW, PRI>(m, S, loc, loc + 6, loc + 6 + n, loc + 9 + n, jp, T);
    // (LIMITS: the base position, which 2b reads again after S's factor has gone over the link records)
    if (LIMITS && (PH & kPrep) && lane < 3) I.pb(n)[lane] = S.link()[kP + lane];
    // 2a. lane per link: m_l and m_l c_l; lane per task: the frame's origin, the target twist, the link
    if ((PH & kPrep) && com && lane < L) {
        const double* k = S.link() + S.lrec * lane;
        const double* R = k + kR;
        const double* cl = m.com + 3 * lane;
        const double ms = m.mass[lane];
        double* o = I.mc() + kIkMc * lane;
        o[0] = ms;
        for (int a = 0; a < 3; ++a)
            o[1 + a] = ms * (k[kP + a] + ((R[3 * a] * cl[0] + R[3 * a + 1] * cl[1]) + R[3 * a + 2] * cl[2]));
    }
    if ((PH & kPrep) && lane < K) {
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
    if constexpr ((PH & kRows) != 0) {
        const double* pB = LIMITS ? I.pb(n) : S.link() + kP;
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
    if constexpr ((PH & kSolve) == 0) return true;
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
    // 3b. LIMITS: the fixed joints leave the system (selects over the unrolled columns: the sets of
    //     a wavefront's two robots differ)
    bool fixed = false;   // this lane's column is one of them
    if constexpr (LIMITS) {
        const double* fx = I.fx(n);
        fixed = lane >= 6 && lane < NV && ((wm >> (lane - 6)) & 1ull);
#pragma unroll
        for (int j = 6; j < NVMAX; ++j) {
            const bool fj = (wm >> (j - 6)) & 1ull;   // (no bit at or above n is ever set)
            const double b = fx[j < NV ? j - 6 : 0];
            y = fj ? y - r[j] * b : y;
            r[j] = fj ? 0.0 : r[j];
        }
        y = fixed ? fx[fixed ? lane - 6 : 0] : y;
#pragma unroll
        for (int k = 0; k < NVMAX; ++k) r[k] = fixed ? (lane == k ? 1.0 : 0.0) : r[k];
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
        // more hard rows than unknowns: dependent (and the factor would not fit); TRACK: the union may
        // hold more than NV, each robot's own count is judged by the kernel and the factor has I.cf()
        bool hok = TRACK || mh <= NV;
        if constexpr (LIMITS) {
            if (lane < kIkRows) I.col()[lane] = 0.0;   // the multipliers by table row (H's factor is done with it)
            wave_sync();
        }
        if (hok && (!LIMITS || mh > 0)) {
            double* rows = I.rows();
            const int cl = lane < NVMAX ? lane : 0;
            // LIMITS: the fixed columns leave the hard rows too, a_t . (fixed values) leaves their targets
            double moved = 0.0;
            if constexpr (LIMITS) {
                int ow = 0, p = 0;
#pragma unroll
                for (int t = 0; t < kIkRows; ++t)
                    if ((hm >> t) & 1u) {
                        ow = lane == p ? t : ow;
                        ++p;
                    }
                const double* ao = rows + ow * I.rs + 6;
                const double* fx = I.fx(n);
                for (int j = 0; j < n; ++j) moved = fma(ao[j], fx[j], moved);
            }
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
                    const bool mine = !TRACK || ((hme >> (t[g] & 31)) & 1u);
                    v[g] = t[g] >= 0 && lane < NV && !fixed && mine ? rows[t[g] * I.rs + cl] : 0.0;
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
                q = q - (LIMITS ? I.wt()[kIkRows + own] - moved : I.wt()[kIkRows + own]);
            }
            if constexpr (TRACK) {
                const bool null = !((hme >> own) & 1u);
                q = null ? 0.0 : q;
#pragma unroll
                for (int t = 0; t < kIkRows; ++t) sr[t] = null ? (own == t ? 1.0 : 0.0) : sr[t];
            }
            double d0 = 0.0;   // S_ii before elimination
#pragma unroll
            for (int t = 0; t < kIkRows; ++t) d0 = own == t ? sr[t] : d0;
            // (iii) S = C C^T, lane per row: pivot p (table row t) is lane p's sr[t]; column p of C
            //       goes to LDS packed (entries p..m_h-1), over the link records, which are dead
            //       until the next kinematics: m_h (m_h + 1) / 2 <= 27 (n + 1) since m_h <= min(27, NV).
            //       TRACK: to I.cf(), which is the link records where the union's factor fits them
            double* ct = S.link();
            if constexpr (TRACK) ct = I.cf();
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
            if constexpr (LIMITS)
                if (lane < mh) I.col()[own] = q;
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

// Robot q's state (zeros 6 + n | bp 3 | bR 9 | jp n into S.st()) and set points (I.sp()) into LDS;
// true if a set point is not finite or a frame index is out of range.  fb_ik_kernel's staging and
// store, for fb_ik_limits_kernel: fb_ik_kernel keeps its own text, since calling these from it moves
// the register allocation of its eight instantiations (same instructions, other registers and order).
template <int HW>
__device__ __forceinline__ bool ik_stage(const Model& m, const IkSmem& I, const blf_fb_state& st, const IkTasks& tk,
                                         int64_t q)
{
    const Half<HW> H;
    const int n = m.n, K = tk.K, lane = H.hl;
    double* loc = I.S.st();
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
    return spbad;
}

// Robot q's results: nu (NaN unless its status is OK), after an integration the state, and the status.
template <int HW>
__device__ __forceinline__ void ik_store(const Model& m, const IkSmem& I, const blf_fb_state& st, int32_t steps,
                                         double* __restrict__ nu, int32_t* __restrict__ status, int64_t q, int stat)
{
    const Half<HW> H;
    const Smem& S = I.S;
    const int n = m.n, NV = n + 6, lane = H.hl;
    const double* loc = S.st();
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

// Section 12c's rho = g_soft - H_soft nu - A_h^T lambda of this lane's column (0 on the base columns),
// from the rebuilt task rows, nu in S.rhs() and the multipliers in I.col(): lane per task row t,
// e_t = w_t (t_t - a_t . nu) - lambda_t (over I.col(); each lane starts its dot at its own column, so
// the lanes' reads fall on different banks), then lane per column sum_t a_tc e_t + jw (sdot* - nu).
template <int HW>
__device__ __forceinline__ double ik_rho(const Model& m, const IkSmem& I, const IkTasks& tk)
{
    const Half<HW> H;
    const Smem& S = I.S;
    const int n = m.n, NV = n + 6, K = tk.K, lane = H.hl;
    const int M = 6 * K + (tk.cw != nullptr ? 3 : 0);
    const double* rows = I.rows();
    const double* x = S.rhs();
    double* e = I.col();
    if (lane < M) {
        const double w = I.wt()[lane];
        const double* a = rows + lane * I.rs;
        double d = 0.0;
        int c = lane % NV;
        for (int k = 0; k < NV; ++k) {
            d = fma(a[c], x[c], d);
            c = c + 1 == NV ? 0 : c + 1;
        }
        const double ev = w != 0.0 ? w * (I.wt()[kIkRows + lane] - d) - e[lane] : -e[lane];
        e[lane] = ev;   // (the lane's own slot)
    }
    wave_sync();
    double rho = 0.0;
    if (lane >= 6 && lane < NV) {
        const int j = lane - 6;
        for (int t = 0; t < M; ++t) rho = fma(rows[t * I.rs + lane], e[t], rho);
        const double* sp = I.sp();
        const double* jp = S.st() + 18 + n;
        const double sd = sp[18 * K + 6 + n + j] + tk.jkp[j] * (sp[18 * K + 6 + j] - jp[j]);
        rho = rho + tk.jw[j] * (sd - x[lane]);
    }
    wave_sync();
    return rho;
}

// Section 12c as the kernel takes it (shared by the batch).
struct IkLimits {
    const double *lower, *upper, *klim, *vmax;
    double sampling;
    int max_iter;
};

// blf_fb_ik_solve_limits (steps == 0) and blf_fb_ik_integrate_limits: fb_ik_kernel with section 12c's
// active-set iteration around the solve.  The working set (two masks), the mode and the counters
// are per robot (the same in every lane of its half); the iteration's trip count is wave-uniform by
// a ballot, a finished robot repeating its last solve unchanged while its neighbour goes on.
template <int NVMAX, int HW, bool PRI>
__global__ __launch_bounds__(64) void fb_ik_limits_kernel(Model m, blf_fb_state st, IkTasks tk, int32_t steps,
                                                          double dT, double* __restrict__ nu,
                                                          int32_t* __restrict__ status, int64_t batch, IkHard hd,
                                                          IkLimits lp, int32_t* __restrict__ iters_out,
                                                          unsigned long long* __restrict__ active_out)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const Half<HW> H;
    const int n = m.n, NV = n + 6, K = tk.K;
    const IkSmem I(smem + H.half * IkSmem(nullptr, n, K, NVMAX, true).total, n, K, NVMAX, true);
    const Smem& S = I.S;
    const int lane = H.hl;
    constexpr int per = kWave / HW;   // robots per wavefront
    const Topo T = build_topo<HW>(m, S);
    const int64_t i0 = (int64_t)blockIdx.x * per + H.half;
    const bool active = i0 < batch;   // see fbd_dynamics_kernel
    const int64_t q = active ? i0 : batch - 1;
    double* loc = S.st();
    double* dR = loc + 18 + 2 * n;
    const bool spbad = ik_stage<HW>(m, I, st, tk, q);
    const bool jc = lane >= 6 && lane < NV;   // this lane's column is joint j
    const int j = jc ? lane - 6 : 0;
    int stat = BLF_IK_OK, total = 0;
    unsigned long long wl = 0ull, wu = 0ull;   // joints held at their lower / upper bound
    const int iters = steps > 0 ? steps : 1;
    for (int it = 0; it < iters; ++it) {
        const bool alive = stat == BLF_IK_OK;
        if (!__ballot(alive)) break;
        bool sfin = true;
        for (int i = lane; i < 12 + n; i += HW) sfin = sfin && so3_finite(loc[6 + n + i]);
        const bool bad = spbad || H.ballot(!sfin) != 0ull;
        stat = alive && bad ? BLF_IK_BAD_INPUT : stat;
        // the box at this state
        if (lane < n) {
            const double s = loc[18 + n + lane], kl = lp.klim[lane];
            const double vm = lp.vmax ? lp.vmax[lane] : __builtin_inf();
            const double a = kl * (lp.lower[lane] - s) / lp.sampling, b = kl * (lp.upper[lane] - s) / lp.sampling;
            I.lo()[lane] = fmin(fmax(a, -vm), vm);
            I.up(n)[lane] = fmin(fmax(b, -vm), vm);
            I.fx(n)[lane] = 0.0;
        }
        bool hdep = false;
        ik_solve<NVMAX, HW, PRI, true, true, kPrep | kRows>(m, I, tk, T, hd, hdep);
        bool done = stat != BLF_IK_OK, block = true;
        int best = 0x7fffffff, stall = 0, nit = 0;
        unsigned long long pl = 0ull, pu = 0ull;   // the set before the last block update
        wl = 0ull;
        wu = 0ull;
        while (__ballot(!done)) {
            const unsigned long long wm = wl | wu;
            const bool ok = ik_solve<NVMAX, HW, PRI, true, true, kSolve>(m, I, tk, T, hd, hdep, wm);
            nit = done ? nit : nit + 1;
            const int s1 = !ok ? BLF_IK_NOT_POSITIVE : hdep && wm == 0ull ? BLF_IK_HARD_DEPENDENT : BLF_IK_OK;
            stat = done ? stat : s1;
            done = done || s1 != BLF_IK_OK;
            // a set that made the hard rows dependent: back to the one before it, one joint at a time from here
            const bool back = !done && hdep;
            if (back && !block) stat = BLF_IK_LIMITS_UNRESOLVED;
            done = done || (back && !block);
            wl = back ? pl : wl;
            wu = back ? pu : wu;
            block = back ? false : block;
            // free joints outside their box
            const double v = S.rhs()[jc ? lane : 0];
            const double lo = I.lo()[j], up = I.up(n)[j];
            const bool held = (wm >> j) & 1ull;
            const bool go = !done && !back;
            const unsigned long long vl = H.ballot(go && jc && !held && v < lo) >> 6;
            const unsigned long long vu = H.ballot(go && jc && !held && v > up) >> 6;
            unsigned long long rl = 0ull, ru = 0ull;   // held joints whose rho points into the box
            if (__ballot(!done)) ik_solve<NVMAX, HW, PRI, true, true, kRows>(m, I, tk, T, hd, hdep);
            if (__ballot(go && wm != 0ull)) {
                const double rho = ik_rho<HW>(m, I, tk);
                rl = H.ballot(go && jc && ((wl >> j) & 1ull) && rho > 0.0) >> 6;
                ru = H.ballot(go && jc && ((wu >> j) & 1ull) && rho < 0.0) >> 6;
            }
            const int ninf = __builtin_popcountll(vl | vu | rl | ru);
            done = done || (go && ninf == 0);
            const bool more = !done && go;
            if (more && nit >= lp.max_iter) stat = BLF_IK_LIMITS_UNRESOLVED;
            if (back && !done && nit >= lp.max_iter) stat = BLF_IK_LIMITS_UNRESOLVED;
            done = done || stat != BLF_IK_OK;
            const bool upd = more && !done;
            if (upd && block) {
                stall = ninf < best ? 0 : stall + 1;
                best = ninf < best ? ninf : best;
                block = stall < 8;
            }
            if (upd && block) {
                pl = wl;
                pu = wu;
                wl = (wl & ~rl) | vl;
                wu = (wu & ~ru) | vu;
            }
            if (__ballot(upd && !block)) {
                // one joint: the most violated free one (the lowest index among equals), else the
                // lowest-index held one of the wrong sign
                const double mag = v < lo ? lo - v : v - up;
                double bm = 0.0;
                int bj = -1;
                for (int c = 6; c < NV; ++c) {
                    const double mc = H.bcast_k(mag, c);
                    const bool in = ((vl | vu) >> (c - 6)) & 1ull;
                    bj = in && mc > bm ? c - 6 : bj;
                    bm = in && mc > bm ? mc : bm;
                }
                const unsigned long long rr = rl | ru;
                const unsigned long long pick = bj >= 0 ? 1ull << bj : rr & (~rr + 1ull);
                if (upd && !block) {
                    wl = bj >= 0 ? wl | (pick & vl) : wl & ~pick;
                    wu = bj >= 0 ? wu | (pick & vu) : wu & ~pick;
                }
            }
            if (jc) I.fx(n)[j] = ((wl >> j) & 1ull) ? lo : ((wu >> j) & 1ull) ? up : 0.0;
            wave_sync();
        }
        total += nit;
        if (steps > 0) {
            const bool step = stat == BLF_IK_OK;
            if (lane == 0) fbk_rot_rate(m.rho, loc + 9 + n, S.rhs() + 3, dR);
            wave_sync();
            if (step)
                for (int i = lane; i < 12 + n; i += HW) {
                    if (i < 3) loc[6 + n + i] = loc[6 + n + i] + S.rhs()[i] * dT;
                    else if (i < 12) loc[6 + n + i] = loc[6 + n + i] + dR[i - 3] * dT;
                    else loc[18 + n + (i - 12)] = loc[18 + n + (i - 12)] + S.rhs()[6 + (i - 12)] * dT;
                }
            wave_sync();
        }
    }
    if (!active) return;
    ik_store<HW>(m, I, st, steps, nu, status, q, stat);
    if (iters_out && lane == 0) iters_out[q] = total;
    if (active_out && lane < 2) active_out[2 * q + lane] = stat != BLF_IK_OK ? 0ull : lane == 0 ? wl : wu;
}

// Section 12d as the kernel takes it: the schedule's arrays, the masks in the kernel's row bits (the
// CoM bits moved down to 6 K, as IkHard::slots) and the trajectories.
struct IkTrack {
    int T;
    unsigned base, stance;   // hard->rows | the rows contact[b][k][t] makes hard for task k
    const int32_t* contact;
    const double *pose, *twist, *cpos, *cvel;
    double *jtraj, *btraj, *ntraj;
    int32_t* fail;
};

// blf_fb_ik_track: fb_ik_limits_kernel's step with the set points and the hard mask of step t, the
// state in LDS over the T steps.  Per step only the 18 K + 6 set points of that step are staged again
// (the joint task's are held), and each robot's mask is rebuilt from its contact flags; the solve
// takes the union of the wavefront's two masks (ik_solve's TRACK).  A robot whose own mask counts more
// than 6 + n rows solves with an empty one (all null rows, which cannot fail) and is marked
// dependent here.  lp.lower == nullptr: no box (every iteration ends after its first solve).
template <int NVMAX, int HW, bool PRI>
__global__ __launch_bounds__(64) void fb_ik_track_kernel(Model m, blf_fb_state st, IkTasks tk, IkTrack tr,
                                                         double dT, int32_t* __restrict__ status, int64_t batch,
                                                         double tau, IkLimits lp, int32_t* __restrict__ iters_out,
                                                         unsigned long long* __restrict__ active_out)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const Half<HW> H;
    const int n = m.n, NV = n + 6, K = tk.K;
    const IkTrackSmem I(smem + H.half * IkTrackSmem(nullptr, n, K, NVMAX).total, n, K, NVMAX);
    const Smem& S = I.S;
    const int lane = H.hl;
    constexpr int per = kWave / HW;   // robots per wavefront
    const Topo T = build_topo<HW>(m, S);
    const int64_t i0 = (int64_t)blockIdx.x * per + H.half;
    const bool active = i0 < batch;   // see fbd_dynamics_kernel
    const int64_t q = active ? i0 : batch - 1;
    const int64_t NT = tr.T;
    double* loc = S.st();
    double* dR = loc + 18 + 2 * n;
    // once: the state and the joint task's set points (held over the call)
    for (int i = lane; i < 18 + 2 * n; i += HW) {
        double v = 0.0;
        if (i < 6 + n) v = 0.0;
        else if (i < 9 + n) v = st.base_pos[3 * q + (i - 6 - n)];
        else if (i < 18 + n) v = st.base_rot[9 * q + (i - 9 - n)];
        else v = st.joint_pos[(int64_t)n * q + (i - 18 - n)];
        loc[i] = v;
    }
    bool jfin = true;
    for (int i = lane; i < 2 * n; i += HW) {
        const double v = i < n ? tk.jpos[(int64_t)n * q + i] : tk.jvel ? tk.jvel[(int64_t)n * q + (i - n)] : 0.0;
        I.sp()[18 * K + 6 + i] = v;
        jfin = jfin && so3_finite(v);
    }
    bool fbad = false;   // the frame indices are shared by the batch
    for (int k = 0; k < K; ++k) {
        const int f = tk.frame[k];
        fbad = fbad || f < 0 || f >= m.F;
    }
    const bool jbad = fbad || H.ballot(!jfin) != 0ull;
    wave_sync();
    const bool jc = lane >= 6 && lane < NV;   // this lane's column is joint j
    const int j = jc ? lane - 6 : 0;
    int stat = BLF_IK_OK, total = 0, fstep = -1;
    unsigned long long wl = 0ull, wu = 0ull;   // joints held at their lower / upper bound
    for (int t = 0; t < tr.T; ++t) {
        const bool alive = stat == BLF_IK_OK;
        if (!__ballot(alive)) break;
        // step t's set points and contact flags (a failed robot reads none)
        bool fin = true;
        if (alive)
            for (int i = lane; i < 18 * K + 6; i += HW) {
                double v = 0.0;
                if (i < 12 * K) {
                    v = tr.pose[((q * K + i / 12) * NT + t) * 12 + i % 12];
                } else if (i < 18 * K) {
                    const int e = i - 12 * K;
                    v = tr.twist ? tr.twist[((q * K + e / 6) * NT + t) * 6 + e % 6] : 0.0;
                } else if (i < 18 * K + 3) {
                    v = tk.cw ? tr.cpos[(q * NT + t) * 3 + (i - 18 * K)] : 0.0;
                } else {
                    v = tk.cw && tr.cvel ? tr.cvel[(q * NT + t) * 3 + (i - 18 * K - 3)] : 0.0;
                }
                I.sp()[i] = v;
                fin = fin && so3_finite(v);
            }
        const bool cin = alive && tr.contact != nullptr && lane < K && tr.contact[(q * K + lane) * NT + t] != 0;
        const unsigned cm = (unsigned)H.ballot(cin);   // bit k: task k is in contact
        unsigned mine = tr.base;
#pragma unroll
        for (int k = 0; k < BLF_IK_MAX_SE3_TASKS; ++k) mine |= ((cm >> k) & 1u) ? tr.stance & (0x3Fu << (6 * k)) : 0u;
        const bool over = __builtin_popcount(mine) > NV;   // judged on the robot's own count
        mine = over ? 0u : mine;
        unsigned un = mine;
        if (HW < kWave) un |= (unsigned)__shfl_xor((int)mine, HW, kWave);
        const IkHard hd{(unsigned)__builtin_amdgcn_readfirstlane((int)un), tau};
        const bool spbad = jbad || H.ballot(!fin) != 0ull;
        wave_sync();
        bool sfin = true;
        for (int i = lane; i < 12 + n; i += HW) sfin = sfin && so3_finite(loc[6 + n + i]);
        const bool bad = spbad || H.ballot(!sfin) != 0ull;
        stat = alive && bad ? BLF_IK_BAD_INPUT : stat;
        // the box at this state
        if (lane < n) {
            double lo = -__builtin_inf(), up = __builtin_inf();
            if (lp.lower != nullptr) {
                const double s = loc[18 + n + lane], kl = lp.klim[lane];
                const double vm = lp.vmax ? lp.vmax[lane] : __builtin_inf();
                const double a = kl * (lp.lower[lane] - s) / lp.sampling, b = kl * (lp.upper[lane] - s) / lp.sampling;
                lo = fmin(fmax(a, -vm), vm);
                up = fmin(fmax(b, -vm), vm);
            }
            I.lo()[lane] = lo;
            I.up(n)[lane] = up;
            I.fx(n)[lane] = 0.0;
        }
        bool hdep = false;
        ik_solve<NVMAX, HW, PRI, true, true, kPrep | kRows, true>(m, I, tk, T, hd, hdep);
        // the active-set iteration of fb_ik_limits_kernel (see there)
        bool done = stat != BLF_IK_OK, block = true;
        int best = 0x7fffffff, stall = 0, nit = 0;
        unsigned long long pl = 0ull, pu = 0ull;
        wl = 0ull;
        wu = 0ull;
        while (__ballot(!done)) {
            const unsigned long long wm = wl | wu;
            const bool ok = ik_solve<NVMAX, HW, PRI, true, true, kSolve, true>(m, I, tk, T, hd, hdep, wm, mine);
            hdep = hdep || over;
            nit = done ? nit : nit + 1;
            const int s1 = !ok ? BLF_IK_NOT_POSITIVE : hdep && wm == 0ull ? BLF_IK_HARD_DEPENDENT : BLF_IK_OK;
            stat = done ? stat : s1;
            done = done || s1 != BLF_IK_OK;
            const bool back = !done && hdep;
            if (back && !block) stat = BLF_IK_LIMITS_UNRESOLVED;
            done = done || (back && !block);
            wl = back ? pl : wl;
            wu = back ? pu : wu;
            block = back ? false : block;
            const double v = S.rhs()[jc ? lane : 0];
            const double lo = I.lo()[j], up = I.up(n)[j];
            const bool held = (wm >> j) & 1ull;
            const bool go = !done && !back;
            const unsigned long long vl = H.ballot(go && jc && !held && v < lo) >> 6;
            const unsigned long long vu = H.ballot(go && jc && !held && v > up) >> 6;
            unsigned long long rl = 0ull, ru = 0ull;
            if (__ballot(!done)) ik_solve<NVMAX, HW, PRI, true, true, kRows, true>(m, I, tk, T, hd, hdep);
            if (__ballot(go && wm != 0ull)) {
                const double rho = ik_rho<HW>(m, I, tk);
                rl = H.ballot(go && jc && ((wl >> j) & 1ull) && rho > 0.0) >> 6;
                ru = H.ballot(go && jc && ((wu >> j) & 1ull) && rho < 0.0) >> 6;
            }
            const int ninf = __builtin_popcountll(vl | vu | rl | ru);
            done = done || (go && ninf == 0);
            const bool more = !done && go;
            if (more && nit >= lp.max_iter) stat = BLF_IK_LIMITS_UNRESOLVED;
            if (back && !done && nit >= lp.max_iter) stat = BLF_IK_LIMITS_UNRESOLVED;
            done = done || stat != BLF_IK_OK;
            const bool upd = more && !done;
            if (upd && block) {
                stall = ninf < best ? 0 : stall + 1;
                best = ninf < best ? ninf : best;
                block = stall < 8;
            }
            if (upd && block) {
                pl = wl;
                pu = wu;
                wl = (wl & ~rl) | vl;
                wu = (wu & ~ru) | vu;
            }
            if (__ballot(upd && !block)) {
                const double mag = v < lo ? lo - v : v - up;
                double bm = 0.0;
                int bj = -1;
                for (int c = 6; c < NV; ++c) {
                    const double mc = H.bcast_k(mag, c);
                    const bool in = ((vl | vu) >> (c - 6)) & 1ull;
                    bj = in && mc > bm ? c - 6 : bj;
                    bm = in && mc > bm ? mc : bm;
                }
                const unsigned long long rr = rl | ru;
                const unsigned long long pick = bj >= 0 ? 1ull << bj : rr & (~rr + 1ull);
                if (upd && !block) {
                    wl = bj >= 0 ? wl | (pick & vl) : wl & ~pick;
                    wu = bj >= 0 ? wu | (pick & vu) : wu & ~pick;
                }
            }
            if (jc) I.fx(n)[j] = ((wl >> j) & 1ull) ? lo : ((wu >> j) & 1ull) ? up : 0.0;
            wave_sync();
        }
        total += nit;
        const bool step = stat == BLF_IK_OK;
        if (lane == 0) fbk_rot_rate(m.rho, loc + 9 + n, S.rhs() + 3, dR);
        wave_sync();
        if (step)
            for (int i = lane; i < 12 + n; i += HW) {
                if (i < 3) loc[6 + n + i] = loc[6 + n + i] + S.rhs()[i] * dT;
                else if (i < 12) loc[6 + n + i] = loc[6 + n + i] + dR[i - 3] * dT;
                else loc[18 + n + (i - 12)] = loc[18 + n + (i - 12)] + S.rhs()[6 + (i - 12)] * dT;
            }
        wave_sync();
        fstep = alive && !step ? t : fstep;
        // slice t: the state and nu after the step
        if (active && step) {
            const int64_t at = (int64_t)t * batch + q;
            for (int i = lane; i < 12 + n; i += HW) {
                const double v = loc[6 + n + i];
                if (i < 12) {
                    if (tr.btraj) tr.btraj[at * 12 + i] = v;
                } else if (tr.jtraj) {
                    tr.jtraj[at * n + (i - 12)] = v;
                }
            }
            if (tr.ntraj)
                for (int c = lane; c < NV; c += HW) tr.ntraj[at * NV + c] = S.rhs()[c];
        }
    }
    if (!active) return;
    if (fstep >= 0) {   // NaN from the failed step on
        const double nan = __builtin_nan("");
        for (int t = fstep; t < tr.T; ++t) {
            const int64_t at = (int64_t)t * batch + q;
            for (int i = lane; i < 12 + n; i += HW) {
                if (i < 12) {
                    if (tr.btraj) tr.btraj[at * 12 + i] = nan;
                } else if (tr.jtraj) {
                    tr.jtraj[at * n + (i - 12)] = nan;
                }
            }
            if (tr.ntraj)
                for (int c = lane; c < NV; c += HW) tr.ntraj[at * NV + c] = nan;
        }
    }
    ik_store<HW>(m, I, st, 1, nullptr, status, q, stat);
    if (tr.fail && lane == 0) tr.fail[q] = fstep;
    if (iters_out && lane == 0) iters_out[q] = total;
    if (active_out && lane < 2) active_out[2 * q + lane] = stat != BLF_IK_OK ? 0ull : lane == 0 ? wl : wu;
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
// a robot's LDS bytes in the layout of nvmax rows (32: two robots per wavefront, kNW: one)
static size_t ik_lds(int n, int K, int nvmax, bool limits)
{
    return sizeof(double) * IkSmem(nullptr, n, K, nvmax, limits).total;
}

static size_t ik_track_lds(int n, int K, int nvmax) { return sizeof(double) * IkTrackSmem(nullptr, n, K, nvmax).total; }

size_t fb_ik_lds_bytes(int n, int K, bool limits)
{
    return fb_launch_lds(n, ik_lds(n, K, 32, limits), ik_lds(n, K, kNW, limits));
}

size_t fb_ik_track_lds_bytes(int n, int K)
{
    return fb_launch_lds(n, ik_track_lds(n, K, 32), ik_track_lds(n, K, kNW));
}

static IkTasks to_tasks(const blf_ik_tasks* t)
{
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
    return tk;
}

// slots == 0: the soft kernels (section 12); otherwise the HARD ones (section 12b)
blf_status launch_fb_ik(const blf_fb_model* md, const blf_fb_state* st, const blf_ik_tasks* t, int64_t batch,
                        int32_t steps, double dT, double* nu, int32_t* status, hipStream_t s,
                        uint32_t slots, double tau)
{
    const IkTasks tk = to_tasks(t);
    const bool pri = md->joint_type != nullptr;
    const int n = md->ndof;
    const IkHard hd{slots, tau};
    auto k2 = slots ? (pri ? fb_ik_kernel<32, 32, true, true> : fb_ik_kernel<32, 32, false, true>)
                    : (pri ? fb_ik_kernel<32, 32, true, false> : fb_ik_kernel<32, 32, false, false>);
    auto k1 = slots ? (pri ? fb_ik_kernel<kNW, kWave, true, true> : fb_ik_kernel<kNW, kWave, false, true>)
                    : (pri ? fb_ik_kernel<kNW, kWave, true, false> : fb_ik_kernel<kNW, kWave, false, false>);
    return fb_launch("fb_ik_kernel launch", k2, ik_lds(n, tk.K, 32, false), k1, ik_lds(n, tk.K, kNW, false), n, batch,
                     s, to_model(md), *st, tk, steps, dT, nu, status, batch, hd);
}

// blf_ik_limits as the kernels take it; null: no box
static IkLimits to_limits(const blf_ik_limits* lim)
{
    if (lim == nullptr) return IkLimits{nullptr, nullptr, nullptr, nullptr, 1.0, BLF_IK_LIMITS_DEFAULT_MAX_ITER};
    return IkLimits{lim->pos_lower, lim->pos_upper, lim->klim, lim->vel_max, lim->sampling_time, lim->max_iter};
}

blf_status launch_fb_ik_limits(const blf_fb_model* md, const blf_fb_state* st, const blf_ik_tasks* t,
                               const blf_ik_limits* lim, int64_t batch, int32_t steps, double dT, double* nu,
                               int32_t* status, int32_t* iters, uint64_t* active, hipStream_t s, uint32_t slots,
                               double tau)
{
    const IkTasks tk = to_tasks(t);
    const bool pri = md->joint_type != nullptr;
    const int n = md->ndof;
    const IkHard hd{slots, tau};
    unsigned long long* act = reinterpret_cast<unsigned long long*>(active);
    return fb_launch("fb_ik_limits_kernel launch",
                     pri ? fb_ik_limits_kernel<32, 32, true> : fb_ik_limits_kernel<32, 32, false>,
                     ik_lds(n, tk.K, 32, true),
                     pri ? fb_ik_limits_kernel<kNW, kWave, true> : fb_ik_limits_kernel<kNW, kWave, false>,
                     ik_lds(n, tk.K, kNW, true), n, batch, s, to_model(md), *st, tk, steps, dT, nu, status, batch, hd,
                     to_limits(lim), iters, act);
}

blf_status launch_fb_ik_track(const blf_fb_model* md, const blf_fb_state* st, const blf_ik_tasks* t,
                              const blf_ik_limits* lim, const blf_ik_schedule* sch, int64_t batch, double dT,
                              double* joint_traj, double* base_traj, double* nu_traj, int32_t* status,
                              int32_t* fail_step, int32_t* iters, uint64_t* active, hipStream_t s, uint32_t base,
                              uint32_t stance, double tau)
{
    const IkTasks tk = to_tasks(t);
    const bool pri = md->joint_type != nullptr;
    const int n = md->ndof;
    const IkTrack tr{sch->steps, base, stance, sch->contact, sch->se3_pose, sch->se3_twist, sch->com_pos,
                     sch->com_vel, joint_traj, base_traj, nu_traj, fail_step};
    unsigned long long* act = reinterpret_cast<unsigned long long*>(active);
    return fb_launch("fb_ik_track_kernel launch",
                     pri ? fb_ik_track_kernel<32, 32, true> : fb_ik_track_kernel<32, 32, false>,
                     ik_track_lds(n, tk.K, 32),
                     pri ? fb_ik_track_kernel<kNW, kWave, true> : fb_ik_track_kernel<kNW, kWave, false>,
                     ik_track_lds(n, tk.K, kNW), n, batch, s, to_model(md), *st, tk, tr, dT, status, batch, tau,
                     to_limits(lim), iters, act);
}

}  // namespace blf
