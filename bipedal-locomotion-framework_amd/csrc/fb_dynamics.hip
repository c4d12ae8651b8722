// fb_dynamics.hip — FloatingBaseDynamicalSystem on the device.
//
// FloatingBaseSystemDynamics.cpp:102-251 takes the free-floating mass matrix M, the generalized
// bias forces h and the contact-frame Jacobians from iDynTree KinDynComputations and then solves
//   nu_dot = LLT(M [+ reg]) \ (-h + sum_c J_c^T w_c + [0; tau]).
// Here the rigid-body terms are computed directly, in the mixed representation (base velocity
// (dp_B/dt, w_B), world coordinates), for a kinematic tree of revolute joints, with spatial
// quantities taken about ONE FIXED POINT for the whole tree, where a composite inertia is a plain
// sum.  The point is the system's own base position at kernel entry (the reference point ref,
// fb_common.h load_state / kRef), not the world origin: nu_dot does not depend on the point, but the
// arithmetic takes it as differences of terms of size m |c|^2 (Ibar below, the subtree sums and their
// prefix differences), so about the world origin the rounding error grew with the SQUARE of the
// robot's distance from it -- measured on an MI355X against the 1e-9 bar: 7e-10 at 8 m, 2e-7 at
// 128 m, 2e-5 at 1 km, 1e-3 at 8 km (tests/test_gpu_fb_translation.py).  So every position below
// (c, o_j, p_B, the contact points) is relative to ref: the kernels hold base_pos - ref (zero at
// entry, exactly; the Euler kernel integrates it and writes ref + it back), subtract ref from the
// contacts' null-pose positions and add it to the positions fb_frame_state / fb_dcm write.  "The
// origin" below is that point:
//   link l:   spatial inertia I_l = (m, h = m c, Ibar = I_c + m(|c|^2 1 - c c^T)) (10 numbers),
//             spatial force   F_l = (tau_c + c x f, f),  f = m (a_c - g), tau_c = I_c al + w x I_c w
//             (accelerations at nu_dot = 0);
//   column:   motion axis S = (w, u): base linear e_a -> (0, e_a); base angular e_a -> (e_a, p_B x e_a);
//             joint j -> (z_j, o_j x z_j);
//   M_ij  = S_j^T (Ic_sub(i) S_i)  when column j acts on the subtree moved by column i (i >= j),
//   rhs_c = [tau] - S_c^T (sum of F_l over the subtree of c  -  contact wrenches on it, taken about
//           the origin),
// which is exactly sum_l m Jv^T Jv + Jw^T I Jw, h and J_c^T w_c of the Jacobian form
// (oracle/fb_dynamics.py evaluates that form; the two agree to rounding).
// One 64-lane workgroup (one wavefront) per system, or per two systems of at most 32 rows (struct
// Half), everything in LDS:
//   1. per-joint rotations, lane per joint;  2. forward kinematics by pointer jumping along the
//   ancestor chains (every joint lane at once, log2 of the depth rounds);  4. contact wrenches,
//   lane per contact (they run before step 3);  3. per-link spatial inertia / force with the
//   link's contact wrenches subtracted, lane per link.
// From there the default is the articulated-body solve (fbd_aba): one inward and one outward
// sweep over the tree levels, no mass matrix.  A model with a mass-matrix regularisation
// (mass_reg != NULL), which needs M itself, takes steps 5-9 instead:
//   5. subtree sums: a DPP prefix sum per component over DFS-ordered joints, otherwise level by
//   level from the leaves;  6. column axes, their composite products and the right-hand side, lane
//   per column;  7. M, lane per row (the row in registers);  8. Cholesky, right-looking, two
//   columns per step, lane per row, the pivot columns through LDS behind a wavefront fence (no
//   s_barrier);  9. forward and back substitution with the right-hand side in registers (lane per
//   row, the unknowns broadcast by v_readlane).
// The inverse dynamics (fbd_id_eval: blf_fb_inverse_dynamics and the computed-torque Euler kernel)
// shares steps 1, 4 and 3 and replaces the solve by one outward and one inward pass (its own header
// below).
#include "blf_internal.h"
#include "contact_math.h"
#include "dcm_qp_common.h"   // the DPP prefix-scan levels (qp::tree_fwd / tree_has)
#include "fb_common.h"       // the LDS layout, the model, the topology and steps 1-2 (shared with fb_ik.hip)
#include "fbk_math.h"

namespace blf {

#ifdef BLF_STAMPS
// Diagnostic build only (make stamps): per-phase cycle sums of lane 0 for the first 64 systems.
__device__ unsigned long long g_fbd_stamps[12];
#define FSTAMP(t) unsigned long long t = __builtin_amdgcn_s_memtime()
#define FSTAMP_ADD(slot, t0) \
    do { if (blockIdx.x < 64 && threadIdx.x == 0) atomicAdd(&g_fbd_stamps[slot], __builtin_amdgcn_s_memtime() - (t0)); } while (0)
extern "C" int blf_debug_fbd_stamps(unsigned long long* out, int reset)
{
    unsigned long long h[12];
    if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_fbd_stamps), sizeof(h)) != hipSuccess) return -1;
    for (int i = 0; i < 12; ++i) out[i] = h[i];
    if (reset) {
        unsigned long long z[12] = {};
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_fbd_stamps), z, sizeof(z)) != hipSuccess) return -1;
    }
    return 0;
}
#else
#define FSTAMP(t)
#define FSTAMP_ADD(slot, t0)
#endif

namespace {

// ---- The articulated-body solve (round 5): nu_dot without M, its factorization or the
//      substitutions.  With every spatial quantity about one point (the reference point) no
//      transform is needed between a link and its parent, and the accelerations relative to
//      nu_dot = 0 satisfy
//        da_c = da_p + s_j qdd_j   (joint j moves link c = j + 1 from its parent link p),
//        f_c  = F_c + I_c da_c     (F_c: step 3's force at nu_dot = 0, contacts subtracted),
//        s_j^T (sum of f over the subtree of c) = tau_j,
//      which the articulated inertias IA and biases pA solve in one inward and one outward sweep
//      over the tree levels (lane per joint):
//        IA_c = I_c + sum_children (IA_k - U_k U_k^T / D_k),  pA_c = F_c + sum_children (pA_k + U_k u_k / D_k),
//        U_j = IA_c s_j,  D_j = s_j^T U_j,  u_j = tau_j - s_j^T pA_c;
//        base: IA_0 da_0 = -pA_0 (6 x 6, every lane), qdd_B from da_0 = S_B qdd_B;
//        outward: qdd_j = (u_j - U_j^T da_p) / D_j,  da_c = da_p + s_j qdd_j.
//      The same solution as M nu_dot = rhs (Featherstone's ABA; the oracle's Jacobian form agrees
//      to rounding, tests/test_gpu_fb_dynamics.py at 1e-9 relative).  A model with a mass-matrix
//      regularisation (reg != NULL) keeps the factorization, which that term needs.
// 6 x 6 symmetric matrices as their upper triangle, row-major (21 entries).
__host__ __device__ constexpr int s6(int i, int j)
{
    return i <= j ? i * 6 - i * (i - 1) / 2 + (j - i) : j * 6 - j * (j - 1) / 2 + (i - j);
}

// the spatial inertia about the origin (m, h, Ibar xx xy xz yy yz zz) as a 6 x 6 on (w; u)
__device__ __forceinline__ void spatial6(const double* si, double (&I)[21])
{
    const double m = si[0], h0 = si[1], h1 = si[2], h2 = si[3];
    I[s6(0, 0)] = si[4]; I[s6(0, 1)] = si[5]; I[s6(0, 2)] = si[6];
    I[s6(1, 1)] = si[7]; I[s6(1, 2)] = si[8]; I[s6(2, 2)] = si[9];
    I[s6(0, 3)] = 0.0; I[s6(0, 4)] = -h2; I[s6(0, 5)] = h1;
    I[s6(1, 3)] = h2; I[s6(1, 4)] = 0.0; I[s6(1, 5)] = -h0;
    I[s6(2, 3)] = -h1; I[s6(2, 4)] = h0; I[s6(2, 5)] = 0.0;
    I[s6(3, 3)] = m; I[s6(3, 4)] = 0.0; I[s6(3, 5)] = 0.0;
    I[s6(4, 4)] = m; I[s6(4, 5)] = 0.0; I[s6(5, 5)] = m;
}

template <int HW, bool PRI>
__device__ __forceinline__ bool fbd_aba(const Model& m, const Smem& S, const double* tau, const double* bp,
                                        const Topo& T, int lane)
{
    const int n = m.n;
    const bool jl = lane < n;
    // joint j's slot: link j + 1's record (Smem aba), written after that link's spatial terms are read
    double* const rec = S.link();
    const int lr = S.lrec;
    bool ok = true;
    // this lane's joint axis s = (w; u) and torque
    double sv[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    double tq = 0.0;
    if (jl) {
        const double* z = S.jz() + 3 * lane;
        if (PRI && m.jtype[lane] == BLF_JOINT_PRISMATIC) {
            sv[3] = z[0]; sv[4] = z[1]; sv[5] = z[2];
        } else {
            sv[0] = z[0]; sv[1] = z[1]; sv[2] = z[2];
            cross3(S.jo() + 3 * lane, z, sv + 3);
        }
        tq = tau[lane];
    }
    double U[6], uD = 0.0, iD = 0.0;
#pragma unroll
    for (int a = 0; a < 6; ++a) U[a] = 0.0;
    // inward sweep, deepest joints first
    FSTAMP(a_in);
    for (int lev = T.maxdepth; lev >= 0; --lev) {
        if (jl && T.depth == lev) {
            const double* k = rec + lr * (lane + 1);
            double IA[21], pA[6];
            spatial6(k + kSIa, IA);
#pragma unroll
            for (int a = 0; a < 6; ++a) pA[a] = k[kSFa + a];
            for (unsigned long long b = T.cmask; b; b &= b - 1) {
                const double* c = rec + lr * (__builtin_ctzll(b) + 1);
#pragma unroll
                for (int e = 0; e < 21; ++e) IA[e] = IA[e] + c[e];
#pragma unroll
                for (int a = 0; a < 6; ++a) pA[a] = pA[a] + c[21 + a];
            }
#pragma unroll
            for (int a = 0; a < 6; ++a) {
                double t = 0.0;
#pragma unroll
                for (int b = 0; b < 6; ++b) t = fma(IA[s6(a, b)], sv[b], t);
                U[a] = t;
            }
            double D = 0.0, sp = 0.0;
#pragma unroll
            for (int a = 0; a < 6; ++a) {
                D = fma(sv[a], U[a], D);
                sp = fma(sv[a], pA[a], sp);
            }
            ok = ok && D > 0.0;
            iD = 1.0 / D;
            uD = (tq - sp) * iD;
            double* o = rec + lr * (lane + 1);
#pragma unroll
            for (int a = 0; a < 6; ++a) {
                const double Ua = U[a] * iD;
#pragma unroll
                for (int b = a; b < 6; ++b) o[s6(a, b)] = fma(-Ua, U[b], IA[s6(a, b)]);
                o[21 + a] = fma(U[a], uD, pA[a]);
            }
        }
        wave_sync();
    }
    FSTAMP_ADD(4, a_in);
    // the base: IA_0 da_0 = -pA_0 (every lane, from the base's children's slots)
    FSTAMP(a_base);
    double da[6];
    {
        double IA[21], pA[6];
        const double* k = rec;
        spatial6(k + kSIa, IA);
#pragma unroll
        for (int a = 0; a < 6; ++a) pA[a] = k[kSFa + a];
        for (unsigned long long b = T.bmask; b; b &= b - 1) {
            const double* c = rec + lr * (__builtin_ctzll(b) + 1);
#pragma unroll
            for (int e = 0; e < 21; ++e) IA[e] = IA[e] + c[e];
#pragma unroll
            for (int a = 0; a < 6; ++a) pA[a] = pA[a] + c[21 + a];
        }
        // LDL^T of IA_0 in registers, then the two substitutions
        double L[21], d[6], x[6];
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            double dj = IA[s6(j, j)];
#pragma unroll
            for (int c = 0; c < j; ++c) dj = dj - (L[s6(j, c)] * L[s6(j, c)]) * d[c];
            ok = ok && dj > 0.0;
            d[j] = dj;
            const double idj = 1.0 / dj;
#pragma unroll
            for (int i = j + 1; i < 6; ++i) {
                double t = IA[s6(i, j)];
#pragma unroll
                for (int c = 0; c < j; ++c) t = t - (L[s6(i, c)] * L[s6(j, c)]) * d[c];
                L[s6(i, j)] = t * idj;
            }
        }
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            double t = -pA[i];
#pragma unroll
            for (int c = 0; c < i; ++c) t = t - L[s6(i, c)] * x[c];
            x[i] = t;
        }
#pragma unroll
        for (int i = 5; i >= 0; --i) {
            double t = x[i] / d[i];
#pragma unroll
            for (int c = i + 1; c < 6; ++c) t = t - L[s6(c, i)] * da[c];
            da[i] = t;
        }
    }
    FSTAMP_ADD(5, a_base);
    // outward sweep: qdd_j and the joint's child link's da, shallowest first
    FSTAMP(a_out);
    double qdd = 0.0;
    for (int lev = 0; lev <= T.maxdepth; ++lev) {
        if (jl && T.depth == lev) {
            double dp[6];
            const double* src = rec + lr * T.P;   // the parent joint's slot (T.P = 0: the base, unused)
#pragma unroll
            for (int a = 0; a < 6; ++a) dp[a] = T.P > 0 ? src[a] : da[a];
            double Ud = 0.0;
#pragma unroll
            for (int a = 0; a < 6; ++a) Ud = fma(U[a], dp[a], Ud);
            qdd = fma(-Ud, iD, uD);
            double* o = rec + lr * (lane + 1);
#pragma unroll
            for (int a = 0; a < 6; ++a) o[a] = fma(sv[a], qdd, dp[a]);
        }
        wave_sync();
    }
    // nu_dot: base (linear: da_0's u - p_B x w; angular: w), then the joints (p_B from the state:
    // the base record's position now holds its spatial force)
    const double* pB = bp;
    if (lane < 6) {
        const double w[3] = {da[0], da[1], da[2]};
        double pw[3];
        cross3(pB, w, pw);
        // (selects, not a lane-indexed array: that would live in scratch)
        const double lin = lane == 0 ? da[3] - pw[0] : lane == 1 ? da[4] - pw[1] : da[5] - pw[2];
        const double ang = lane == 3 ? da[0] : lane == 4 ? da[1] : da[2];
        S.rhs()[lane] = lane < 3 ? lin : ang;
    }
    if (jl) S.rhs()[6 + lane] = qdd;
    wave_sync();
    FSTAMP_ADD(6, a_out);
    const Half<HW> H;
    return H.ballot(!ok) == 0ull;
}

// One evaluation of the dynamics for the system whose state sits in LDS (bv, jv, bp, bR, jp).
// Leaves the generalized acceleration in S.rhs() and returns false if the factorization failed.
// NVMAX >= n + 6 bounds the unrolled factorization loops (each lane keeps its row of M in
// registers).  Lane j < n owns joint j in steps 1, 2 and 5; lane i < NV owns row / column i in
// steps 6-9.
template <int NVMAX, int HW, bool PRI, bool CS, bool ABA>
__device__ __forceinline__ bool fbd_eval(const Model& m, const Smem& S, const double* bv,
                                         const double* jvel, const double* bp, const double* bR,
                                         const double* jp, const double* tau, const Contacts& ct,
                                         int64_t sys, const double* reg, const Topo& T, const double* ref)
{
    static_assert(NVMAX <= HW, "a system's rows must fit its lanes");
    const Half<HW> H;
    const int n = m.n, L = n + 1, NV = n + 6, MS = S.ms;
    // The lane index made opaque once per evaluation, so the lane masks of the unrolled loops
    // (lane == k, lane > k, ...) are recomputed by one compare each instead of being hoisted out of
    // the Euler loop into SGPRs, which spill to VGPR lanes and reload by v_readlane: 3.812 / 3.811
    // against 3.856 / 3.860 ms per c5 period, SGPR spills 595 -> 366, VGPR spills 17 -> 0
    // (profiles/r04_fbd_prefix_opq_ab.log)
    int lane = H.hl;
    asm volatile("" : "+v"(lane));
    const bool jl = lane < n;   // n <= 48 < 64: one joint per lane
    const int depth = T.depth, maxdepth = T.maxdepth;
    FSTAMP(f_t0);
    FSTAMP(f_t1);
    fbd_kinematics<HW, PRI>(m, S, bv, jvel, bp, bR, jp, T);
    FSTAMP_ADD(1, f_t1);
    // 4. contacts: frame state + ContinuousContactModel wrench, and the wrench about the origin.
    //    Before step 3, which needs the wrenches and overwrites the kinematics in the ABA layout.
    FSTAMP(f_t3);
    for (int c = lane; c < ct.C; c += HW) {
        int l;
        const double* fp;
        if constexpr (CS) {
            l = (int)S.cst()[c];
            fp = S.cst() + ct.C + 12 * c;
        } else {
            const int f = ct.frame[c];
            l = m.flink[f];
            fp = m.fpose + 12 * f;
        }
        double pose[12], tw[6];
        frame_state(S.link() + S.lrec * l, fp, pose, tw);
        double* sc = S.cscr() + kCs * c;
        if (given_wrench(ct, c)) {   // any ContactModel, evaluated by the caller
            const double* gw = ct.wrench + (sys * ct.C + c) * 6;
            for (int a = 0; a < 6; ++a) sc[3 + a] = gw[a];
        } else if constexpr (CS)
            contact_wrench(S.cst() + 25 * ct.C + 4 * c, tw, pose, S.cst() + 13 * ct.C + 12 * c, sc + 3);
        else {
            const double* np = ct.null_pose + (sys * ct.C + c) * 12;
            double ns[12];   // the null pose relative to the reference point
            for (int a = 0; a < 12; ++a) ns[a] = a < 3 ? np[a] - ref[a] : np[a];
            contact_wrench(ct.params + 4 * c, tw, pose, ns, sc + 3);
        }
        sc[0] = pose[0]; sc[1] = pose[1]; sc[2] = pose[2];
        sc[9] = (double)l;
        double xf[3];
        cross3(sc, sc + 3, xf);   // x_c x f_c
        for (int a = 0; a < 3; ++a) {
            sc[10 + a] = sc[6 + a] + xf[a];
            sc[13 + a] = sc[3 + a];
        }
    }
    wave_sync();
    FSTAMP_ADD(3, f_t3);
    // 3. per link: COM, world inertia, Newton-Euler force / moment, and the spatial inertia and
    //    force about the reference point (lane per link), with the contact wrenches on the link
    //    (about the origin) subtracted from its force here, once, instead of in every component
    //    group of the subtree sums: 4.070 / 4.078 against 4.198 / 4.200 ms per c5 period
    //    (profiles/r04_fbd_csub_ab.log)
    // (a lambda with one call: written as a plain block the same arithmetic compiles with some
    // commutative operands swapped, and this file's refactors are checked by identical assembly)
    auto link_step = [&]() {
    for (int l = lane; l < L; l += HW) {
        double* k = S.link() + S.lrec * l;
        const double* R = k + kR;
        const double* cl = m.com + 3 * l;
        const double* Ic = m.inertia + 9 * l;
        double rc[3], c[3];
        for (int a = 0; a < 3; ++a) {
            rc[a] = (R[3 * a] * cl[0] + R[3 * a + 1] * cl[1]) + R[3 * a + 2] * cl[2];
            c[a] = k[kP + a] + rc[a];
        }
        double RI[9];   // R Ic
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b)
                RI[3 * a + b] = (R[3 * a] * Ic[b] + R[3 * a + 1] * Ic[3 + b]) + R[3 * a + 2] * Ic[6 + b];
        const int ii[6] = {0, 0, 0, 1, 1, 2}, jj[6] = {0, 1, 2, 1, 2, 2};
        double Iw[6];
        for (int e = 0; e < 6; ++e) {
            const int a = ii[e], b = jj[e];
            Iw[e] = (RI[3 * a] * R[3 * b] + RI[3 * a + 1] * R[3 * b + 1]) + RI[3 * a + 2] * R[3 * b + 2];
        }
        double t1[3], t2[3], t3[3], f[3];
        cross3(k + kAl, rc, t1);
        cross3(k + kW, rc, t2);
        cross3(k + kW, t2, t3);
        const double ms = m.mass[l];
        const double g[3] = {m.g0, m.g1, m.g2};
        for (int a = 0; a < 3; ++a) f[a] = ms * (((k[kA + a] + t1[a]) + t3[a]) - g[a]);
        double Ia[3], Iwv[3], tq[3], cf[3];
        sym_mv(Iw, k + kAl, Ia);
        sym_mv(Iw, k + kW, Iwv);
        cross3(k + kW, Iwv, t1);
        for (int a = 0; a < 3; ++a) tq[a] = Ia[a] + t1[a];
        cross3(c, f, cf);
        const double cc = dot3(c, c);
        double* si = k + (ABA ? kSIa : kSI);   // (ABA: over the record's kinematics, read above)
        si[0] = ms;
        si[1] = ms * c[0]; si[2] = ms * c[1]; si[3] = ms * c[2];
        si[4] = Iw[0] + ms * (cc - c[0] * c[0]);
        si[5] = Iw[1] - ms * (c[0] * c[1]);
        si[6] = Iw[2] - ms * (c[0] * c[2]);
        si[7] = Iw[3] + ms * (cc - c[1] * c[1]);
        si[8] = Iw[4] - ms * (c[1] * c[2]);
        si[9] = Iw[5] + ms * (cc - c[2] * c[2]);
        double sfv[6];
        for (int a = 0; a < 3; ++a) {
            sfv[a] = tq[a] + cf[a];
            sfv[3 + a] = f[a];
        }
        for (int cc2 = 0; cc2 < ct.C; ++cc2) {   // branch-free: the loads do not wait for the test
            const double* sc = S.cscr() + kCs * cc2;
            const bool hit = (int)sc[9] == l;
            double w[6];
#pragma unroll
            for (int a = 0; a < 6; ++a) w[a] = sc[10 + a];
#pragma unroll
            for (int a = 0; a < 6; ++a) sfv[a] = hit ? sfv[a] - w[a] : sfv[a];
        }
        double* sf = k + (ABA ? kSFa : kSF);
        for (int a = 0; a < 6; ++a) sf[a] = sfv[a];
    }
    };
    FSTAMP(f_t2);
    link_step();
    wave_sync();
    FSTAMP_ADD(2, f_t2);
    if constexpr (ABA) {   // steps 5-9 replaced by the articulated-body solve (no regularisation)
        FSTAMP(f_t4a);
        const bool ok = fbd_aba<HW, PRI>(m, S, tau, bp, T, lane);
        FSTAMP_ADD(7, f_t4a);
        FSTAMP_ADD(9, f_t0);
        return ok;
    }
    FSTAMP(f_t4);
    // 5. subtree sums of the spatial inertias and (link - contact) forces.  DFS-ordered models
    //    (every subtree a contiguous run of joints, T.dfs): one inclusive prefix sum over the
    //    joints' link terms per component, subtree_j = prefix[last_j] - prefix[j - 1], the base's
    //    = prefix[n - 1] + its own link terms: 5-6 shuffle levels instead of one LDS round trip
    //    and wave sync per tree level.  Other orders: level by level from the leaves up.
    if (T.dfs) {
        constexpr int G = 4;   // components per group (registers)
#pragma unroll
        for (int g = 0; g < kComp; g += G) {
            double pre[G];
#pragma unroll
            for (int q = 0; q < G; ++q) pre[q] = jl ? S.link()[S.lrec * (lane + 1) + kSI + g + q] : 0.0;
            // inclusive prefix over the half's lanes by DPP (VALU moves, no LDS round trip): row
            // shifts 1, 2, 4, 8 inside each row of 16, then rows 1 / 3 add lane 15 of rows 0 / 2
            // (for HW = 64 also rows 2, 3 add lane 31) -- the QP kernels' forward tree levels
            const int wl = (int)threadIdx.x;
            auto level = [&](auto Lc) {
                constexpr int L = decltype(Lc)::value;
#pragma unroll
                for (int q = 0; q < G; ++q) {
                    const double t = qp::tree_fwd<L>(pre[q]);
                    if (qp::tree_has<L, true>(wl)) pre[q] = pre[q] + t;
                }
            };
            level(std::integral_constant<int, 0>{});
            level(std::integral_constant<int, 1>{});
            level(std::integral_constant<int, 2>{});
            level(std::integral_constant<int, 3>{});
            level(std::integral_constant<int, 4>{});
            if constexpr (HW == 64) level(std::integral_constant<int, 5>{});
            // the prefix sums go to LDS as they are: step 6 takes prefix[last_j] - prefix[j - 1]
            // itself (gathering them here by lane shuffles: 4.077 / 4.074 against 3.812 / 3.811 ms
            // per c5 period, profiles/r04_fbd_prefix_opq_ab.log)
#pragma unroll
            for (int q = 0; q < G; ++q)
                if (jl) S.comp()[kCompS * lane + g + q] = pre[q];
        }
        wave_sync();
    } else
    for (int lev = maxdepth; lev >= -1; --lev) {
        const bool mine = lev >= 0 ? (jl && depth == lev) : lane == 0;
        if (mine) {
            const int l = lev >= 0 ? lane + 1 : 0;               // the subtree's root link
            const unsigned long long ch = lev >= 0 ? T.cmask : T.bmask;
            double acc[kComp];
#pragma unroll
            for (int p = 0; p < kComp; ++p) acc[p] = S.link()[S.lrec * l + kSI + p];
            for (unsigned long long b = ch; b; b &= b - 1) {
                const double* cs = S.comp() + kCompS * __builtin_ctzll(b);
#pragma unroll
                for (int p = 0; p < kComp; ++p) acc[p] = acc[p] + cs[p];
            }
            double* dst = S.comp() + kCompS * (lev >= 0 ? lane : n);
#pragma unroll
            for (int p = 0; p < kComp; ++p) dst[p] = acc[p];
        }
        wave_sync();
    }
    FSTAMP_ADD(4, f_t4);
    FSTAMP(f_t5);
    // 6. lane c: column axis S_c = (w, u) (to LDS), F_c = Ic S_c with Ic the subtree sum the
    //    column moves (registers), rhs_c = [tau] - S_c^T (subtree force)
    const double* pB = S.link() + kP;
    double y = 0.0, Fc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (lane < NV) {
        const int c = lane;
        double w[3] = {0.0, 0.0, 0.0}, u[3] = {0.0, 0.0, 0.0};
        if (c < 3) {
            u[c] = 1.0;
        } else if (c < 6) {
            w[c - 3] = 1.0;
            cross3(pB, w, u);
        } else {
            const int j = c - 6;
            if (PRI && m.jtype[j] == BLF_JOINT_PRISMATIC) {   // S = (0; z): a pure translation
                for (int a = 0; a < 3; ++a) u[a] = S.jz()[3 * j + a];
            } else {
                for (int a = 0; a < 3; ++a) w[a] = S.jz()[3 * j + a];
                cross3(S.jo() + 3 * j, w, u);
            }
        }
        double Iv[kComp];
        if (T.dfs) {   // the subtree sums from the prefix sums step 5 left
            const int j = c - 6;
            const double* hp = S.comp() + kCompS * (c < 6 ? n - 1 : T.lastc);
            const double* lp = c < 6 ? S.link() + kSI : S.comp() + kCompS * (j > 0 ? j - 1 : 0);
#pragma unroll
            for (int p = 0; p < kComp; ++p) {
                const double h = hp[p], l = lp[p];
                Iv[p] = c < 6 ? l + h : (j > 0 ? h - l : h);
            }
        } else {
#pragma unroll
            for (int p = 0; p < kComp; ++p) Iv[p] = S.comp()[kCompS * (c < 6 ? n : c - 6) + p];
        }
        const double* I = Iv;
        double Iwv[3], hu[3], wh[3];
        sym_mv(I + 4, w, Iwv);
        cross3(I + 1, u, hu);
        cross3(w, I + 1, wh);
        double* sa = S.sax() + kSax * c;
        for (int a = 0; a < 3; ++a) {
            sa[a] = w[a];
            sa[3 + a] = u[a];
            Fc[a] = Iwv[a] + hu[a];
            Fc[3 + a] = wh[a] + I[0] * u[a];
        }
        y = (c >= 6 ? tau[c - 6] : 0.0) - (dot3(w, I + 10) + dot3(u, I + 13));
    }
    const unsigned long long myanc = (lane >= 6 && lane < NV) ? S.anc()[lane - 5] : 0ull;
    wave_sync();
    FSTAMP_ADD(5, f_t5);
    FSTAMP(f_t6);
    // 7. row i of M in registers: M_ij = S_j . F_i when column j moves the subtree of column i
    //    (j < 6, or joint j - 6 an ancestor of column i's link)
    // (no branch per column: a branch between an LDS read and its use serialises the reads; an
    // index past the last column is clamped and its value discarded by the row predicate)
    double r[NVMAX];
#pragma unroll
    for (int j = 0; j < NVMAX; ++j) {
        const double* sa = S.sax() + kSax * (j < NV ? j : NV - 1);   // every lane reads the same S_j
        const double v = dot3(sa, Fc) + dot3(sa + 3, Fc + 3);
        const bool vis = j <= lane && lane < NV && (j < 6 || ((myanc >> (j - 6)) & 1ull));
        r[j] = vis ? v : 0.0;
    }
    if (reg && lane < NV)
#pragma unroll
        for (int j = 0; j < NVMAX; ++j)
            if (j < NV && j <= lane) r[j] = r[j] + reg[NV * lane + j];
    FSTAMP_ADD(6, f_t6);
    FSTAMP(f_t7);
    // 8. Cholesky M = L L^T, right-looking, lane i keeps row i in registers, CB columns per step:
    //    every lane factors the step's CB x CB diagonal block from its broadcast entries (rows past
    //    the matrix: identity), computes its own CB entries by the same forward substitution (so a
    //    lane inside the block reproduces the block's row bit for bit), and the CB columns of the
    //    rows below go through one LDS buffer set (two sets, alternating) and are read back as
    //    broadcasts: one LDS round trip per CB pivots, where the dependent chain of pivot, column
    //    store and read-back is the Cholesky's time at one wavefront per SIMD
    bool ok = true;
    // the block must divide the register row (NVMAX = 54 for the largest model: 2)
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
                    double t = in ? H.bcast_k(r[k + j], k + i) : 0.0;   // M_{k+i,k+j}
#pragma unroll
                    for (int c = 0; c < j; ++c) t = t - Lb[i][c] * Lb[j][c];
                    Lb[i][j] = t * il[j];
                }
                double d = in ? H.bcast_k(r[k + i], k + i) : 1.0;       // M_{k+i,k+i}
#pragma unroll
                for (int c = 0; c < i; ++c) d = d - Lb[i][c] * Lb[i][c];
                ok = ok && (d > 0.0);
                // 1 / sqrt: v_rsq_f64 and one Newton step (parity with the oracle is at 1e-9)
                double q = __builtin_amdgcn_rsq(d);
                il[i] = q * (1.5 - (0.5 * d) * (q * q));
                Lb[i][i] = d * il[i];
            }
            // this lane's entries L_{lane,k..k+CB-1} (upper-triangle junk inside the block, unread)
            double li[CB];
#pragma unroll
            for (int i = 0; i < CB; ++i) {
                double t = r[k + i];
#pragma unroll
                for (int c = 0; c < i; ++c) t = t - li[c] * Lb[i][c];
                li[i] = t * il[i];
            }
            // the step's column set: CB columns at stride NV (a compile-time stride of NVMAX made
            // the Cholesky itself faster, 19.9k -> 14.8k cycles in fbd_dynamics_kernel, but one c5
            // period of the Euler kernel slower, 4.04 / 4.02 against 3.77 / 3.76 ms;
            // profiles/r04_fbd_colfix_cstage_ab.log)
            double* col = S.comp() + ((k / CB) & 1) * CB * NV;
#pragma unroll
            for (int i = 0; i < CB; ++i) {
                r[k + i] = lane >= k ? li[i] : r[k + i];
                if (lane < NV && k + i < NV) col[i * NV + lane] = r[k + i];
            }
            wave_sync();
            // No row predicate: a lane above row j only updates its upper-triangle entry r[j],
            // which nothing reads (pivots are diagonal, the substitutions and the stored L use
            // j <= lane), so the update is CB LDS broadcast reads and fmas per entry (parity with
            // the oracle is 1e-9 relative, not bitwise).  j >= NV touches only lanes past the matrix.
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
    FSTAMP_ADD(7, f_t7);
    FSTAMP(f_t8);
    // 9. L z = y with the rows in registers, then L^T x = z with row k of L read from LDS (the
    //    link records are dead by now); lane k scales its own entry, one broadcast per step.  Two
    //    unknowns per step (the 2 x 2 block solved by every lane, as in the factorization) measured
    //    the same: 6.054 / 6.069 against 6.081 / 6.073 ms per c5 period of the Euler kernel; the
    //    pivot scaling on the multipliers instead of the unknowns was slower, 3.914 / 3.904 against
    //    3.792 / 3.792 ms (profiles/r04_fbd_subst_ab.log)
    const double idg = lane < NV ? 1.0 / bcast_own_diag<NVMAX>(r, lane) : 0.0;
#pragma unroll
    for (int k = 0; k < NVMAX; ++k) {   // k >= NV changes only lanes past the matrix
        y = lane == k ? y * idg : y;
        const double xk = H.bcast_k(y, k);
        const double f = lane > k ? r[k] : 0.0;
        y = y - f * xk;
    }
    double* Lr = S.link();
    if (lane < NV)
#pragma unroll
        for (int j = 0; j < NVMAX; ++j)
            if (j < NV && j <= lane) Lr[MS * lane + j] = r[j];
    wave_sync();
    double lki = (lane < NV - 1) ? Lr[MS * (NV - 1) + lane] : 0.0;
    for (int k = NV - 1; k >= 0; --k) {
        const double lnext = (k > 0 && lane < k - 1) ? Lr[MS * (k - 1) + lane] : 0.0;   // read ahead
        if (lane == k) y = y * idg;
        const double xk = H.bcast_k(y, k);
        if (lane < k) y = y - lki * xk;
        lki = lnext;
    }
    if (lane < NV) S.rhs()[lane] = y;
    wave_sync();
    FSTAMP_ADD(8, f_t8);
    FSTAMP_ADD(9, f_t0);
    return ok;
}

template <int NVMAX, int HW, bool PRI, bool ABA>
__global__ __launch_bounds__(64) void fbd_dynamics_kernel(Model m, blf_fb_state st,
                                                          const double* __restrict__ tau,
                                                          Contacts ct, const double* reg,
                                                          blf_fb_state out, int64_t batch)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const Half<HW> H;
    const int n = m.n, NV = n + 6;
    const Smem S(smem + H.half * Smem(nullptr, n, ct.C, ABA).total, n, ct.C, ABA);
    // system of this half; a missing second system of the last wavefront recomputes the last one
    // and writes nothing
    const int64_t q0 = (int64_t)blockIdx.x * (kWave / HW) + H.half;
    const bool active = q0 < batch;
    const int64_t q = active ? q0 : batch - 1;
    const int lane = H.hl;
    double* loc = S.st();   // bv 6 | jv n | bp 3 | bR 9 | jp n
    for (int i = lane; i < 18 + 2 * n; i += HW) {
        double v;
        if (i < 6) v = st.base_vel[6 * q + i];
        else if (i < 6 + n) v = st.joint_vel[(int64_t)n * q + (i - 6)];
        else if (i < 9 + n) {   // the reference point; the position relative to it starts at zero
            loc[kRef(n) + (i - 6 - n)] = st.base_pos[3 * q + (i - 6 - n)];
            v = 0.0;
        } else if (i < 18 + n) v = st.base_rot[9 * q + (i - 9 - n)];
        else v = st.joint_pos[(int64_t)n * q + (i - 18 - n)];
        loc[i] = v;
    }
    wave_sync();
    const Topo T = build_topo<HW>(m, S);
    const bool ok = fbd_eval<NVMAX, HW, PRI, false, ABA>(m, S, loc, loc + 6, loc + 6 + n, loc + 9 + n, loc + 18 + n,
                                                         tau + (int64_t)n * q, ct, q, reg, T, loc + kRef(n));
    if (!active) return;
    const double nan = __builtin_nan("");
    for (int c = lane; c < NV; c += HW) {
        const double a = ok ? S.rhs()[c] : nan;
        if (c < 6) out.base_vel[6 * q + c] = a;
        else out.joint_vel[(int64_t)n * q + (c - 6)] = a;
    }
    if (lane == 0) {
        double dR[9];
        fbk_rot_rate(m.rho, loc + 9 + n, loc + 3, dR);
        for (int i = 0; i < 3; ++i) out.base_pos[3 * q + i] = loc[i];
        for (int i = 0; i < 9; ++i) out.base_rot[9 * q + i] = dR[i];
    }
    for (int j = lane; j < n; j += HW) out.joint_pos[(int64_t)n * q + j] = loc[6 + j];
}

// The closed loop's state -> plan map: the centre of mass, its velocity
// and the DCM of every system,
//   c = sum_l m_l (p_l + R_l com_l) / m,   cdot = sum_l m_l (v_l + w_l x R_l com_l) / m,
//   xi = c_xy + cdot_xy / omega_0
// (the LIP's divergent component with the plan's first-knot omega).  One wavefront per system:
// the forward kinematics of fbd_eval, then lane per link and one wave sum per quantity.
template <bool PRI>
__global__ __launch_bounds__(64) void fb_dcm_kernel(Model m, blf_fb_state st, const double* __restrict__ omega0,
                                                    int64_t ostride, double* __restrict__ com,
                                                    double* __restrict__ xi)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int n = m.n, L = n + 1;
    const Smem S(smem, n, 0, true);   // kinematics only: the compact (articulated-body) layout
    const int64_t q = blockIdx.x;
    const int lane = threadIdx.x;
    double* loc = S.st();
    load_state<kWave>(st, q, n, lane, loc);
    wave_sync();
    const Topo T = build_topo<kWave>(m, S);
    fbd_kinematics<kWave, PRI>(m, S, loc, loc + 6, loc + 6 + n, loc + 9 + n, loc + 18 + n, T);
    wave_sync();
    double a[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};   // m c (3), m cdot (3), m
    if (lane < L) {
        const double* k = S.link() + S.lrec * lane;
        const double* R = k + kR;
        const double* cl = m.com + 3 * lane;
        double rc[3], t[3];
        for (int i = 0; i < 3; ++i) rc[i] = (R[3 * i] * cl[0] + R[3 * i + 1] * cl[1]) + R[3 * i + 2] * cl[2];
        cross3(k + kW, rc, t);
        const double ms = m.mass[lane];
        for (int i = 0; i < 3; ++i) {
            a[i] = ms * (k[kP + i] + rc[i]);
            a[3 + i] = ms * (k[kV + i] + t[i]);
        }
        a[6] = ms;
    }
#pragma unroll
    for (int i = 0; i < 7; ++i) a[i] = wave_sum(a[i]);
    if (lane == 0) {
        double o[6];
        for (int i = 0; i < 6; ++i) o[i] = a[i] / a[6];
        for (int i = 0; i < 3; ++i) o[i] = loc[kRef(n) + i] + o[i];   // back to world coordinates
        for (int i = 0; i < 6; ++i) com[6 * q + i] = o[i];
        if (xi) {
            const double w0 = omega0[q * ostride];
            xi[2 * q] = o[0] + o[3] / w0;
            xi[2 * q + 1] = o[1] + o[4] / w0;
        }
    }
}

// The world transform and mixed twist of K frames of every system (blf_fb_frame_state): the state
// a caller hands a ContactModel it evaluates itself (BLF_CONTACT_WRENCH).  One wavefront per
// system: the forward kinematics of fbd_eval, then lane per frame with fbd_eval's own frame_state.
template <bool PRI>
__global__ __launch_bounds__(64) void fb_frame_state_kernel(Model m, blf_fb_state st, int K,
                                                            const int32_t* __restrict__ frames,
                                                            double* __restrict__ pose,
                                                            double* __restrict__ twist)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int n = m.n;
    const Smem S(smem, n, 0, true);   // kinematics only: the compact (articulated-body) layout
    const int64_t q = blockIdx.x;
    const int lane = threadIdx.x;
    double* loc = S.st();
    load_state<kWave>(st, q, n, lane, loc);
    wave_sync();
    const Topo T = build_topo<kWave>(m, S);
    fbd_kinematics<kWave, PRI>(m, S, loc, loc + 6, loc + 6 + n, loc + 9 + n, loc + 18 + n, T);
    wave_sync();
    for (int c = lane; c < K; c += kWave) {
        const int f = frames[c];
        double p[12], tw[6];
        if (f >= 0 && f < m.F) {
            frame_state(S.link() + S.lrec * m.flink[f], m.fpose + 12 * f, p, tw);
            for (int a = 0; a < 3; ++a) p[a] = loc[kRef(n) + a] + p[a];   // back to world coordinates
        } else {   // a frame index outside [0, nframes): NaN, never an out-of-bounds read
            for (int a = 0; a < 12; ++a) p[a] = __builtin_nan("");
            for (int a = 0; a < 6; ++a) tw[a] = __builtin_nan("");
        }
        if (pose)
            for (int a = 0; a < 12; ++a) pose[(q * K + c) * 12 + a] = p[a];
        if (twist)
            for (int a = 0; a < 6; ++a) twist[(q * K + c) * 6 + a] = tw[a];
    }
}

// The closed loop's plan -> robot map: the joint references held over one
// control period,
//   q_ref_j = q_nom_j + lean_j0 (r0_x - c_x) + lean_j1 (r0_y - c_y)
// with r0 the plan's first VRP and c the centre of mass; the joint impedance of
// fbd_euler_kernel tracks them.  Element per (system, joint).
__global__ __launch_bounds__(256) void posture_reference_kernel(int n, const double* __restrict__ qnom,
                                                                const double* __restrict__ lean,
                                                                const double* __restrict__ com,
                                                                const double* __restrict__ vrp,
                                                                int64_t vstride, int64_t total,
                                                                double* __restrict__ qref)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const int64_t q = e / n;
    const int j = (int)(e - q * n);
    const double ex = vrp[q * vstride] - com[6 * q];
    const double ey = vrp[q * vstride + 1] - com[6 * q + 1];
    qref[e] = (qnom[j] + lean[2 * j] * ex) + lean[2 * j + 1] * ey;
}

// The closed loop's plan -> CoM reference map (blf_dcm_com_reference, blf_c.h section 9b): the
// LIP's stable half integrated under the plan's first VRP, T explicit Euler steps of h.  Lane per
// (system, horizontal axis); the axis-0 lane also writes the height column.  A system with a
// non-finite input writes NaN to every output of its own.
__global__ __launch_bounds__(256) void com_reference_kernel(const double* __restrict__ xi0,
                                                            const double* __restrict__ vrp, int64_t vstride,
                                                            const double* __restrict__ omega0, int64_t ostride,
                                                            const double* __restrict__ zref, double* __restrict__ cref,
                                                            int32_t T, double h, int64_t batch,
                                                            double* __restrict__ cpos, double* __restrict__ cvel,
                                                            double* __restrict__ xiend)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= 2 * batch) return;
    const int64_t q = e >> 1;
    const int a = (int)(e & 1);
    const double w = omega0[q * ostride], z = zref[q];
    auto fin = [](double x) { return __builtin_isfinite(x); };
    // (a system's two lanes sit in one wavefront: both read cref here before either writes it below)
    const bool ok = fin(xi0[2 * q]) && fin(xi0[2 * q + 1]) && fin(vrp[q * vstride]) && fin(vrp[q * vstride + 1]) &&
                    fin(w) && fin(z) && fin(cref[2 * q]) && fin(cref[2 * q + 1]);
    const double nan = __builtin_nan("");
    const double nwr = -w * vrp[q * vstride + a];
    double xi = ok ? xi0[2 * q + a] : nan, c = ok ? cref[2 * q + a] : nan;
    double* p = cpos + 3 * (int64_t)T * q;
    double* v = cvel + 3 * (int64_t)T * q;
    for (int32_t t = 0; t < T; ++t) {
        const double vt = w * (xi - c);
        p[3 * t + a] = c;
        v[3 * t + a] = vt;
        if (a == 0) {
            p[3 * t + 2] = ok ? z : nan;
            v[3 * t + 2] = ok ? 0.0 : nan;
        }
        c = c + vt * h;
        xi = xi + ((w * xi) + nwr) * h;
    }
    cref[2 * q + a] = c;
    if (xiend) xiend[2 * q + a] = xi;
}

// ---- Inverse dynamics (blf_fb_inverse_dynamics, blf_c.h section 8b): the hybrid form, joint
//      accelerations prescribed and the base either free or prescribed.  In the reference-point
//      formulation of fbd_eval / fbd_aba no transform separates a link from its parent, so with
//      s_j joint j's motion axis about the point, I_l / F_l step 3's spatial inertia and nu_dot = 0
//      force (contacts subtracted) and da_0 the base's spatial acceleration relative to nu_dot = 0:
//        a'_l = sum_{j in anc(l)} s_j sdd_j          (a plain sum over the ancestor mask)
//        f_l  = F_l + I_l a'_l,   I_tot = sum_l I_l,   p_tot = sum_l f_l
//        free base:  I_tot da_0 = -p_tot              (the 6 x 6 LDL^T of fbd_aba's base step)
//        given base: da_0 = S_B nu_dot_B,  base wrench = S_B^T (p_tot + I_tot da_0)
//        tau_j = s_j^T sum_{l : j in anc(l)} (f_l + I_l da_0).
//      One sweep out, two wave sums and one sweep in: no level-by-level articulated sweep and no
//      (n + 6)^2 factorization.  The subtree sum of tau_j is taken by every joint lane over the
//      links' ancestor masks (n broadcast reads of 6 doubles, no wave sync per tree level and no
//      prefix differences, whatever the joint order).
// A link record's doubles 16..21 in the articulated-body layout: free once step 3 has run; they
// hold s_j sdd_j (joint j in link j + 1's record) and then f_l + I_l da_0 (link l's).
constexpr int kIDa = 16;

// (m, h, Ibar) times the motion vector (w; u): (Ibar w + h x u; w x h + m u)
__device__ __forceinline__ void spatial_mv(const double* I, const double* x, double* y)
{
    double Iw[3], hu[3], wh[3];
    sym_mv(I + 4, x, Iw);
    cross3(I + 1, x + 3, hu);
    cross3(x, I + 1, wh);
    for (int a = 0; a < 3; ++a) {
        y[a] = Iw[a] + hu[a];
        y[3 + a] = wh[a] + I[0] * x[3 + a];
    }
}

// The sum of v over the system's half of the wavefront, in every lane of it (a butterfly: the
// same bits in every lane).
template <int HW>
__device__ __forceinline__ double half_sum(double v)
{
#pragma unroll
    for (int off = HW / 2; off >= 1; off >>= 1) v = v + __shfl_xor(v, off, kWave);
    return v;
}

// One inverse-dynamics evaluation for the system whose state sits in LDS.  sdd (LDS, [n]): the
// joint accelerations on entry, the joint torques on return.  given: bacc is nu_dot_B (mixed) and
// bout receives the base wrench (force, torque; mixed, at the base origin); otherwise bout
// receives nu_dot_B.  Every lane returns the same bout.  Returns false if a pivot of I_tot was not
// a finite positive number.  Steps 1, 4 and 3 are fbd_eval's, as text of their own in the
// articulated-body layout (that function's instantiations keep their assembly).
template <int HW, bool PRI, bool CS>
__device__ __forceinline__ bool fbd_id_eval(const Model& m, const Smem& S, const double* bv, const double* jvel,
                                            const double* bp, const double* bR, const double* jp, double* sdd,
                                            const bool given, const double (&bacc)[6], double (&bout)[6],
                                            const Contacts& ct, int64_t sys, const Topo& T, const double* ref)
{
    const Half<HW> H;
    const int n = m.n, L = n + 1;
    const int lane = H.hl;
    const bool jl = lane < n;
    fbd_kinematics<HW, PRI>(m, S, bv, jvel, bp, bR, jp, T);
    // 4. contacts (fbd_eval's step 4)
    for (int c = lane; c < ct.C; c += HW) {
        int l;
        const double* fp;
        if constexpr (CS) {
            l = (int)S.cst()[c];
            fp = S.cst() + ct.C + 12 * c;
        } else {
            const int f = ct.frame[c];
            l = m.flink[f];
            fp = m.fpose + 12 * f;
        }
        double pose[12], tw[6];
        frame_state(S.link() + S.lrec * l, fp, pose, tw);
        double* sc = S.cscr() + kCs * c;
        if (given_wrench(ct, c)) {
            const double* gw = ct.wrench + (sys * ct.C + c) * 6;
            for (int a = 0; a < 6; ++a) sc[3 + a] = gw[a];
        } else if constexpr (CS)
            contact_wrench(S.cst() + 25 * ct.C + 4 * c, tw, pose, S.cst() + 13 * ct.C + 12 * c, sc + 3);
        else {
            const double* np = ct.null_pose + (sys * ct.C + c) * 12;
            double ns[12];   // the null pose relative to the reference point
            for (int a = 0; a < 12; ++a) ns[a] = a < 3 ? np[a] - ref[a] : np[a];
            contact_wrench(ct.params + 4 * c, tw, pose, ns, sc + 3);
        }
        sc[0] = pose[0]; sc[1] = pose[1]; sc[2] = pose[2];
        sc[9] = (double)l;
        double xf[3];
        cross3(sc, sc + 3, xf);
        for (int a = 0; a < 3; ++a) {
            sc[10 + a] = sc[6 + a] + xf[a];
            sc[13 + a] = sc[3 + a];
        }
    }
    wave_sync();
    // 3. per link: the spatial inertia and the nu_dot = 0 force about the reference point, contacts
    //    subtracted (fbd_eval's step 3), over the record's kinematics
    for (int l = lane; l < L; l += HW) {
        double* k = S.link() + S.lrec * l;
        const double* R = k + kR;
        const double* cl = m.com + 3 * l;
        const double* Ic = m.inertia + 9 * l;
        double rc[3], c[3];
        for (int a = 0; a < 3; ++a) {
            rc[a] = (R[3 * a] * cl[0] + R[3 * a + 1] * cl[1]) + R[3 * a + 2] * cl[2];
            c[a] = k[kP + a] + rc[a];
        }
        double RI[9];
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b)
                RI[3 * a + b] = (R[3 * a] * Ic[b] + R[3 * a + 1] * Ic[3 + b]) + R[3 * a + 2] * Ic[6 + b];
        const int ii[6] = {0, 0, 0, 1, 1, 2}, jj[6] = {0, 1, 2, 1, 2, 2};
        double Iw[6];
        for (int e = 0; e < 6; ++e) {
            const int a = ii[e], b = jj[e];
            Iw[e] = (RI[3 * a] * R[3 * b] + RI[3 * a + 1] * R[3 * b + 1]) + RI[3 * a + 2] * R[3 * b + 2];
        }
        double t1[3], t2[3], t3[3], f[3];
        cross3(k + kAl, rc, t1);
        cross3(k + kW, rc, t2);
        cross3(k + kW, t2, t3);
        const double ms = m.mass[l];
        const double g[3] = {m.g0, m.g1, m.g2};
        for (int a = 0; a < 3; ++a) f[a] = ms * (((k[kA + a] + t1[a]) + t3[a]) - g[a]);
        double Ia[3], Iwv[3], tq[3], cf[3];
        sym_mv(Iw, k + kAl, Ia);
        sym_mv(Iw, k + kW, Iwv);
        cross3(k + kW, Iwv, t1);
        for (int a = 0; a < 3; ++a) tq[a] = Ia[a] + t1[a];
        cross3(c, f, cf);
        const double cc = dot3(c, c);
        double sfv[6];
        for (int a = 0; a < 3; ++a) {
            sfv[a] = tq[a] + cf[a];
            sfv[3 + a] = f[a];
        }
        for (int cc2 = 0; cc2 < ct.C; ++cc2) {
            const double* sc = S.cscr() + kCs * cc2;
            const bool hit = (int)sc[9] == l;
#pragma unroll
            for (int a = 0; a < 6; ++a) sfv[a] = hit ? sfv[a] - sc[10 + a] : sfv[a];
        }
        double* si = k + kSIa;
        si[0] = ms;
        si[1] = ms * c[0]; si[2] = ms * c[1]; si[3] = ms * c[2];
        si[4] = Iw[0] + ms * (cc - c[0] * c[0]);
        si[5] = Iw[1] - ms * (c[0] * c[1]);
        si[6] = Iw[2] - ms * (c[0] * c[2]);
        si[7] = Iw[3] + ms * (cc - c[1] * c[1]);
        si[8] = Iw[4] - ms * (c[1] * c[2]);
        si[9] = Iw[5] + ms * (cc - c[2] * c[2]);
        double* sf = k + kSFa;
        for (int a = 0; a < 6; ++a) sf[a] = sfv[a];
    }
    wave_sync();
    double* const rec = S.link();
    const int lr = S.lrec;
    // joint lane: the motion axis s = (w; u), and s sdd into the joint's child link's record
    double sv[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (jl) {
        const double* z = S.jz() + 3 * lane;
        if (PRI && m.jtype[lane] == BLF_JOINT_PRISMATIC) {
            sv[3] = z[0]; sv[4] = z[1]; sv[5] = z[2];
        } else {
            sv[0] = z[0]; sv[1] = z[1]; sv[2] = z[2];
            cross3(S.jo() + 3 * lane, z, sv + 3);
        }
        const double qdd = sdd[lane];
        double* o = rec + lr * (lane + 1) + kIDa;
#pragma unroll
        for (int a = 0; a < 6; ++a) o[a] = sv[a] * qdd;
    }
    wave_sync();
    // link lane: a' over the ancestor joints (base to link), f = F + I a'
    double I[10], f[6];
#pragma unroll
    for (int e = 0; e < 10; ++e) I[e] = 0.0;
#pragma unroll
    for (int a = 0; a < 6; ++a) f[a] = 0.0;
    if (lane < L) {
        const double* k = rec + lr * lane;
#pragma unroll
        for (int e = 0; e < 10; ++e) I[e] = k[kSIa + e];
#pragma unroll
        for (int a = 0; a < 6; ++a) f[a] = k[kSFa + a];
        double ap[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (unsigned long long b = S.anc()[lane]; b; b &= b - 1) {
            const double* c = rec + lr * (__builtin_ctzll(b) + 1) + kIDa;
#pragma unroll
            for (int a = 0; a < 6; ++a) ap[a] = ap[a] + c[a];
        }
        double Ia[6];
        spatial_mv(I, ap, Ia);
#pragma unroll
        for (int a = 0; a < 6; ++a) f[a] = f[a] + Ia[a];
    }
    // the whole-body inertia and force (every lane)
    double It[10], pt[6];
#pragma unroll
    for (int e = 0; e < 10; ++e) It[e] = half_sum<HW>(I[e]);
#pragma unroll
    for (int a = 0; a < 6; ++a) pt[a] = half_sum<HW>(f[a]);
    double pB[3] = {bp[0], bp[1], bp[2]};
    double da[6];
    bool ok = true;
    if (given) {   // da_0 = S_B nu_dot_B: w = the angular part, u = the linear part + p_B x w
        double pw[3];
        cross3(pB, bacc + 3, pw);
        for (int a = 0; a < 3; ++a) {
            da[a] = bacc[3 + a];
            da[3 + a] = bacc[a] + pw[a];
        }
    } else {       // I_tot da_0 = -p_tot: fbd_aba's base step
        double IA[21];
        spatial6(It, IA);
        double Lw[21], d[6], x[6];
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            double dj = IA[s6(j, j)];
#pragma unroll
            for (int c = 0; c < j; ++c) dj = dj - (Lw[s6(j, c)] * Lw[s6(j, c)]) * d[c];
            ok = ok && dj > 0.0 && __builtin_isfinite(dj);
            d[j] = dj;
            const double idj = 1.0 / dj;
#pragma unroll
            for (int i = j + 1; i < 6; ++i) {
                double t = IA[s6(i, j)];
#pragma unroll
                for (int c = 0; c < j; ++c) t = t - (Lw[s6(i, c)] * Lw[s6(j, c)]) * d[c];
                Lw[s6(i, j)] = t * idj;
            }
        }
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            double t = -pt[i];
#pragma unroll
            for (int c = 0; c < i; ++c) t = t - Lw[s6(i, c)] * x[c];
            x[i] = t;
        }
#pragma unroll
        for (int i = 5; i >= 0; --i) {
            double t = x[i] / d[i];
#pragma unroll
            for (int c = i + 1; c < 6; ++c) t = t - Lw[s6(c, i)] * da[c];
            da[i] = t;
        }
    }
    if (given) {   // S_B^T (p_tot + I_tot da_0): the force, and the moment taken to the base origin
        double Id[6], P[6], pf[3];
        spatial_mv(It, da, Id);
        for (int a = 0; a < 6; ++a) P[a] = pt[a] + Id[a];
        cross3(pB, P + 3, pf);
        for (int a = 0; a < 3; ++a) {
            bout[a] = P[3 + a];
            bout[3 + a] = P[a] - pf[a];
        }
    } else {       // nu_dot_B from da_0, as at the end of fbd_aba
        double pw[3];
        cross3(pB, da, pw);
        for (int a = 0; a < 3; ++a) {
            bout[a] = da[3 + a] - pw[a];
            bout[3 + a] = da[a];
        }
    }
    wave_sync();   // every a' is read
    if (lane < L) {
        double Id[6];
        spatial_mv(I, da, Id);
        double* o = rec + lr * lane + kIDa;
#pragma unroll
        for (int a = 0; a < 6; ++a) o[a] = f[a] + Id[a];
    }
    wave_sync();
    // joint lane: tau = s^T (the sum over the links the joint moves)
    if (jl) {
        double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int l = 1; l <= n; ++l) {   // every lane reads the same record: broadcasts
            const bool hit = (S.anc()[l] >> lane) & 1ull;
            const double* c = rec + lr * l + kIDa;
#pragma unroll
            for (int a = 0; a < 6; ++a) acc[a] = hit ? acc[a] + c[a] : acc[a];
        }
        sdd[lane] = dot3(sv, acc) + dot3(sv + 3, acc + 3);
    }
    wave_sync();
    return H.ballot(!ok) == 0ull;
}

// blf_fb_inverse_dynamics: one system per wavefront, or two while n + 6 <= 32 (fbd_dynamics_kernel's
// layouts and staging).  bacc == nullptr: the free-base mode, bout = base_acc_out; otherwise the
// given-base mode, bout = base_wrench.
template <int HW, bool PRI>
__global__ __launch_bounds__(64) void fb_invdyn_kernel(Model m, blf_fb_state st, const double* __restrict__ sdd,
                                                       const double* __restrict__ bacc, Contacts ct,
                                                       double* __restrict__ tau, double* __restrict__ bout,
                                                       int32_t* __restrict__ status, int64_t batch)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const Half<HW> H;
    const int n = m.n;
    const Smem S(smem + H.half * Smem(nullptr, n, ct.C, true).total, n, ct.C, true);
    const int64_t q0 = (int64_t)blockIdx.x * (kWave / HW) + H.half;
    const bool active = q0 < batch;   // see fbd_dynamics_kernel
    const int64_t q = active ? q0 : batch - 1;
    const int lane = H.hl;
    double* loc = S.st();   // bv 6 | jv n | bp 3 | bR 9 | jp n
    bool fin = true;
    for (int i = lane; i < 18 + 2 * n; i += HW) {
        double v;
        if (i < 6) v = st.base_vel[6 * q + i];
        else if (i < 6 + n) v = st.joint_vel[(int64_t)n * q + (i - 6)];
        else if (i < 9 + n) {   // the reference point; the position relative to it starts at zero
            const double r = st.base_pos[3 * q + (i - 6 - n)];
            loc[kRef(n) + (i - 6 - n)] = r;
            fin = fin && __builtin_isfinite(r);
            v = 0.0;
        } else if (i < 18 + n) v = st.base_rot[9 * q + (i - 9 - n)];
        else v = st.joint_pos[(int64_t)n * q + (i - 18 - n)];
        fin = fin && __builtin_isfinite(v);
        loc[i] = v;
    }
    for (int j = lane; j < n; j += HW) {
        const double v = sdd ? sdd[(int64_t)n * q + j] : 0.0;
        fin = fin && __builtin_isfinite(v);
        S.tq()[j] = v;
    }
    double ba[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, bo[6];
    if (bacc)
        for (int a = 0; a < 6; ++a) {
            ba[a] = bacc[6 * q + a];
            fin = fin && __builtin_isfinite(ba[a]);
        }
    for (int c = lane; c < ct.C; c += HW)
        if (given_wrench(ct, c))
            for (int a = 0; a < 6; ++a) fin = fin && __builtin_isfinite(ct.wrench[(q * ct.C + c) * 6 + a]);
    wave_sync();
    const Topo T = build_topo<HW>(m, S);
    const bool pos = fbd_id_eval<HW, PRI, false>(m, S, loc, loc + 6, loc + 6 + n, loc + 9 + n, loc + 18 + n, S.tq(),
                                                 bacc != nullptr, ba, bo, ct, q, T, loc + kRef(n));
    if (!active) return;
    const bool bad = H.ballot(!fin) != 0ull;
    const bool ok = pos && !bad;
    const double nan = __builtin_nan("");
    for (int j = lane; j < n; j += HW) tau[(int64_t)n * q + j] = ok ? S.tq()[j] : nan;
    if (lane < 6) {
        // (selects, not a lane-indexed array: that would live in scratch)
        const double v = lane == 0 ? bo[0] : lane == 1 ? bo[1] : lane == 2 ? bo[2] : lane == 3 ? bo[3] : lane == 4 ? bo[4] : bo[5];
        bout[6 * q + lane] = ok ? v : nan;
    }
    if (status && lane == 0) status[q] = bad ? BLF_IK_BAD_INPUT : pos ? BLF_IK_OK : BLF_IK_NOT_POSITIVE;
}

// ---- The Euler kernel's three torque laws.  A law is a kernel argument and the kernel's last template
//      parameter; Reg is the type of the kernel's mass-matrix regularisation argument under that law.

// blf_fbd_euler_integrate_impedance: the joint impedance tau = kp (q_ref - q) - kd qdot, set as the
// control input before every Euler step (kp == nullptr: the constant torques `tau`, a kernel
// argument of this law alone).
struct Impedance {
    using Reg = const double*;
    const double *kp, *kd, *qref;
};

// blf_fbd_euler_integrate_impedance_traj: the impedance with the reference indexed by the
// integration step, slice s(i) = min(i / sps, T - 1) of qref [T][B][n], a velocity feed-forward
// qdref (or null) and a per-system bias qbias (or null):
//   r = qref (+ qbias),  tau = kp (r - q) - kd (qdot - qdref)   (qdref null: - kd qdot)
// Two systems per wavefront: r and qdref of the current slice sit in LDS (r in Smem's q_ref slot,
// qdref in n doubles behind Smem::total) and are restaged only at a step where the slice changes;
// one system per wavefront reads them from global memory every step, as the held form reads qref.
struct ImpedanceTraj {
    using Reg = const double*;
    const double *kp, *kd, *qref, *qdref, *qbias;
    int64_t qdstride;
    int32_t T, sps;
};

// blf_fbd_euler_integrate_computed_torque_traj: the trajectory law's schedule and slices with the
// torque replaced by the inverse dynamics of the commanded acceleration,
//   sdd = qddref + kp (qref + qbias - q) + kd (qdref - qdot),  tau = clamp(ID(sdd), tau_max),
// taken at every step's start state (the torques pass through Smem's tq slot), followed by the
// forward evaluation with that tau.  The references are read from global memory every step in both
// layouts.  Only the articulated-body path exists: the call refuses mass_reg, so the kernel's
// regularisation argument is empty (a null pointer where one is read).
struct ComputedTorqueTraj {
    struct Reg {
        __device__ operator const double*() const { return nullptr; }
    };
    const double *kp, *kd, *qref, *qdref, *qddref, *qbias, *taumax;
    double* taulast;
    int64_t qdstride, qddstride;
    int32_t T, sps;
};

// ForwardEuler<FloatingBaseDynamicalSystem>::integrate under one of the laws above: the state and
// (two systems per wavefront) the per-system constants staged in LDS, nsteps steps of the law's
// torque, fbd_eval and the pose / velocity update, and the write-back (NaN where an evaluation
// failed).  One text for the three laws, the law's blocks behind `if constexpr`: Tau is
// `const double* __restrict__` under Impedance and empty otherwise, so every instantiation keeps
// the argument layout, and with it the register allocation, of a kernel written for that law alone
// (where a law's value is computed decides the allocation too, see tq
// below).  ComputedTorqueTraj has no ABA = false instantiation; ABA stays a parameter so that an
// instantiation is named like its neighbours'.
// __launch_bounds__: two systems per wavefront (HW = 32) keep more state live per wave: capping it
// at 256 VGPRs for two waves per SIMD spills (9.40 ms per c5 period), one wave per SIMD does not
// (8.29 ms, against 9.29 ms with one system per wavefront at two waves per SIMD; tools/ab_c5.sh).
// kCS, the per-system constants of the Euler loop staged in LDS: the two-systems form only (LLVM's
// allocator crashes on the HW = 64 form).
template <int NVMAX, int HW, bool PRI, bool ABA, class Law, class... Tau>
__global__ __launch_bounds__(64, HW == 32 ? 1 : 2) void fbd_euler_kernel(Model m, blf_fb_state st, Tau... tau,
                                                          Contacts ct, typename Law::Reg reg,
                                                          int32_t nsteps, double dT, double dT_last,
                                                          Law law, int64_t batch)
{
    constexpr bool kHeld = std::is_same_v<Law, Impedance>, kTraj = std::is_same_v<Law, ImpedanceTraj>;
    constexpr bool kCtq = std::is_same_v<Law, ComputedTorqueTraj>;
    static_assert(kHeld || kTraj || kCtq, "an Euler torque law");
    static_assert(ABA || !kCtq, "computed torque: the articulated-body path only");
    static_assert(sizeof...(Tau) == (kHeld ? 1 : 0), "the constant torques: the held law's argument");
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const Half<HW> H;
    const int n = m.n, NV = n + 6;
    constexpr bool kCS = HW == 32;
    const int nx = kTraj && kCS ? (n + 1) & ~1 : 0;   // the slice's qdref behind the system's Smem block
    const Smem S(smem + H.half * (Smem(nullptr, n, ct.C, ABA).total + nx), n, ct.C, ABA);
    const int lane = H.hl;
    constexpr int per = kWave / HW;   // systems per wavefront
    const Topo T = build_topo<HW>(m, S);
    double* loc = S.st();   // bv 6 | jv n | bp 3 | bR 9 | jp n | dR 9
    double* dR = loc + 18 + 2 * n;
    const int64_t i0 = (int64_t)blockIdx.x * per + H.half;
    // a system past the end of an odd batch is computed (as the last system's copy, beside its
    // partner) and written nowhere
    const bool active = i0 < batch;   // see fbd_dynamics_kernel
    const int64_t q = active ? i0 : batch - 1;
    for (int i = lane; i < 18 + 2 * n; i += HW) {
        double v;
        if (i < 6) v = st.base_vel[6 * q + i];
        else if (i < 6 + n) v = st.joint_vel[(int64_t)n * q + (i - 6)];
        else if (i < 9 + n) {   // the reference point; the position relative to it starts at zero
            loc[kRef(n) + (i - 6 - n)] = st.base_pos[3 * q + (i - 6 - n)];
            v = 0.0;
        } else if (i < 18 + n) v = st.base_rot[9 * q + (i - 9 - n)];
        else v = st.joint_pos[(int64_t)n * q + (i - 18 - n)];
        loc[i] = v;
    }
    if constexpr (kCS) {   // this system's constants of the Euler loop, once (Smem o_cst / o_imp)
        const int C = ct.C;
        for (int i = lane; i < 29 * C; i += HW) {
            double v;
            if (i < C) v = (double)m.flink[ct.frame[i]];
            else if (i < 13 * C) v = m.fpose[12 * ct.frame[(i - C) / 12] + (i - C) % 12];
            else if (i < 25 * C) {   // null poses, their positions relative to the reference point
                const int e = (i - 13 * C) % 12;
                v = ct.null_pose[(q * C) * 12 + (i - 13 * C)];
                if (e < 3) v = v - st.base_pos[3 * q + e];
            }
            else v = ct.params[i - 25 * C];
            S.cst()[i] = v;
        }
        if constexpr (kHeld) {
            if (law.kp)
                for (int j = lane; j < n; j += HW) {
                    S.imp()[j] = law.kp[j];
                    S.imp()[n + j] = law.kd[j];
                    S.imp()[2 * n + j] = law.qref[(int64_t)n * q + j];
                }
        } else if constexpr (kTraj) {
            for (int j = lane; j < n; j += HW) {
                S.imp()[j] = law.kp[j];
                S.imp()[n + j] = law.kd[j];
            }
        }
    }
    wave_sync();
    bool ok = true;
    // where fbd_eval reads the step's torques: Smem's tq slot once a law has filled it (assigned in
    // each law's branch: initialised here it moves the trajectory laws' register allocation), the
    // held law without an impedance the constant ones
    const double* tq = nullptr;
    if constexpr (kHeld) tq = (tau, ...) + (int64_t)n * q;
    int32_t slice = -1, left = 0;   // the trajectory law: the slice in use and the steps it still holds
    for (int32_t step = 0; step < nsteps; ++step) {
        const double h = step + 1 < nsteps ? dT : dT_last;
        // the control input of this step from its start state, then the accelerations under it
        if constexpr (kHeld) {
            if (law.kp) {
                for (int j = lane; j < n; j += HW) {
                    if constexpr (kCS)
                        S.tq()[j] = S.imp()[j] * (S.imp()[2 * n + j] - loc[18 + n + j]) - S.imp()[n + j] * loc[6 + j];
                    else
                        S.tq()[j] = law.kp[j] * (law.qref[(int64_t)n * q + j] - loc[18 + n + j]) - law.kd[j] * loc[6 + j];
                }
                wave_sync();
                tq = S.tq();
            }
        } else if constexpr (kTraj) {
            double* const qdr = S.base + S.total;
            const bool next = left == 0 && slice + 1 < law.T;   // the last slice is held to the end
            if (next) {
                ++slice;
                left = law.sps;
            }
            --left;
            const int64_t at = (int64_t)slice * batch + q;   // element (slice, q, .)
            if constexpr (kCS) {
                if (next)
                    for (int j = lane; j < n; j += HW) {
                        double r = law.qref[at * n + j];
                        if (law.qbias) r = r + law.qbias[(int64_t)n * q + j];
                        S.imp()[2 * n + j] = r;
                        if (law.qdref) qdr[j] = law.qdref[at * law.qdstride + j];
                    }
            }
            for (int j = lane; j < n; j += HW) {
                if constexpr (kCS) {
                    if (law.qdref)
                        S.tq()[j] = S.imp()[j] * (S.imp()[2 * n + j] - loc[18 + n + j]) - S.imp()[n + j] * (loc[6 + j] - qdr[j]);
                    else
                        S.tq()[j] = S.imp()[j] * (S.imp()[2 * n + j] - loc[18 + n + j]) - S.imp()[n + j] * loc[6 + j];
                } else {
                    double r = law.qref[at * n + j];
                    if (law.qbias) r = r + law.qbias[(int64_t)n * q + j];
                    if (law.qdref)
                        S.tq()[j] = law.kp[j] * (r - loc[18 + n + j]) - law.kd[j] * (loc[6 + j] - law.qdref[at * law.qdstride + j]);
                    else
                        S.tq()[j] = law.kp[j] * (r - loc[18 + n + j]) - law.kd[j] * loc[6 + j];
                }
            }
            wave_sync();
            tq = S.tq();
        } else {
            const double zero6[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            int64_t sl = step / law.sps;
            if (sl > law.T - 1) sl = law.T - 1;     // the last slice is held to the end
            const int64_t at = sl * batch + q;      // element (slice, q, .)
            // the commanded joint accelerations
            for (int j = lane; j < n; j += HW) {
                double r = law.qref[at * n + j];
                if (law.qbias) r = r + law.qbias[(int64_t)n * q + j];
                double a = law.kp[j] * (r - loc[18 + n + j]);
                if (law.qdref) a = a + law.kd[j] * (law.qdref[at * law.qdstride + j] - loc[6 + j]);
                else a = a - law.kd[j] * loc[6 + j];
                if (law.qddref) a = law.qddref[at * law.qddstride + j] + a;
                S.tq()[j] = a;
            }
            wave_sync();
            double bo[6];
            ok = fbd_id_eval<HW, PRI, kCS>(m, S, loc, loc + 6, loc + 6 + n, loc + 9 + n, loc + 18 + n, S.tq(), false,
                                           zero6, bo, ct, q, T, loc + kRef(n)) && ok;
            if (law.taumax) {   // (selects: a NaN torque stays NaN)
                for (int j = lane; j < n; j += HW) {
                    const double t = S.tq()[j], mx = law.taumax[j];
                    S.tq()[j] = t > mx ? mx : t < -mx ? -mx : t;
                }
                wave_sync();
            }
            tq = S.tq();
        }
        ok = fbd_eval<NVMAX, HW, PRI, kCS, ABA>(m, S, loc, loc + 6, loc + 6 + n, loc + 9 + n, loc + 18 + n,
                                                tq, ct, q, reg, T, loc + kRef(n)) && ok;
        if (lane == 0) fbk_rot_rate(m.rho, loc + 9 + n, loc + 3, dR);
        wave_sync();
        // every element moves by its derivative at the start of the step (ForwardEuler.tpp:37-45):
        // positions first (they read the old velocities), then the velocities
        for (int i = lane; i < 12 + n; i += HW) {
            // base position (3), base rotation (9), joint positions (n)
            if (i < 3) loc[6 + n + i] = loc[6 + n + i] + loc[i] * h;
            else if (i < 12) loc[6 + n + i] = loc[6 + n + i] + dR[i - 3] * h;
            else loc[18 + n + (i - 12)] = loc[18 + n + (i - 12)] + loc[6 + (i - 12)] * h;
        }
        wave_sync();
        for (int i = lane; i < NV; i += HW) loc[i] = loc[i] + S.rhs()[i] * h;
        wave_sync();
    }
    if (active) {
        const double nan = __builtin_nan("");
        for (int i = lane; i < 18 + 2 * n; i += HW) {
            const double v = ok ? loc[i] : nan;
            if (i < 6) st.base_vel[6 * q + i] = v;
            else if (i < 6 + n) st.joint_vel[(int64_t)n * q + (i - 6)] = v;
            else if (i < 9 + n) st.base_pos[3 * q + (i - 6 - n)] = loc[kRef(n) + (i - 6 - n)] + v;
            else if (i < 18 + n) st.base_rot[9 * q + (i - 9 - n)] = v;
            else st.joint_pos[(int64_t)n * q + (i - 18 - n)] = v;
        }
        if constexpr (kCtq)
            if (law.taulast && nsteps > 0)
                for (int j = lane; j < n; j += HW) law.taulast[(int64_t)n * q + j] = ok ? S.tq()[j] : nan;
    }
}

Contacts to_contacts(const blf_fb_contacts* c)
{
    Contacts o;
    o.C = c ? c->ncontacts : 0;
    o.frame = c ? c->frame : nullptr;
    o.params = c ? c->params : nullptr;
    o.null_pose = c ? c->null_pose : nullptr;
    o.law = c ? c->law : nullptr;
    o.wrench = c ? c->wrench : nullptr;
    return o;
}

}  // namespace

size_t fbd_lds_bytes(int n, int C, bool aba) { return sizeof(double) * Smem(nullptr, n, C, aba).total; }

// The articulated-body solve (fbd_aba) unless the model carries a mass-matrix regularisation,
// which needs M itself; BLF_FBD_ABA=0 keeps the factorization for every model (A/B only).
static bool use_aba(const double* reg)
{
    static const bool on = [] {
        const char* e = getenv("BLF_FBD_ABA");
        return !(e && e[0] == '0');
    }();
    return on && reg == nullptr;
}

// The launchers below hand fb_launch (fb_common.h) the two layouts' kernels: NV = HW = 32 for two systems
// per wavefront, NV = kNW and HW = kWave for one.  FBD_KERNEL: kernel K's instantiation for the
// launcher's `pri` (the model has prismatic joints) and `aba`.
#define FBD_KERNEL(K, NV, HW) (pri ? (aba ? K<NV, HW, true, true> : K<NV, HW, true, false>) \
                                   : (aba ? K<NV, HW, false, true> : K<NV, HW, false, false>))

blf_status launch_fbd_dynamics(const blf_fb_model* md, const blf_fb_state* st, const double* tau,
                               const blf_fb_contacts* ct, const double* reg, int64_t batch,
                               const blf_fb_state* out, hipStream_t s)
{
    const Contacts c = to_contacts(ct);
    const bool pri = md->joint_type != nullptr, aba = use_aba(reg);
    const size_t lds = fbd_lds_bytes(md->ndof, c.C, aba);
    return fb_launch("fbd_dynamics_kernel launch", FBD_KERNEL(fbd_dynamics_kernel, 32, 32), lds,
                     FBD_KERNEL(fbd_dynamics_kernel, kNW, kWave), lds, md->ndof, batch, s, to_model(md), *st, tau, c,
                     reg, *out, batch);
}

// fbd_euler_kernel's instantiation for one layout, `pri` and `aba` under a law.  A law without a
// regularisation argument (ComputedTorqueTraj) has no mass-matrix form to pick.
template <int NV, int HW, class Law, class... Tau>
static auto fbd_euler_instance(bool pri, bool aba)
{
    if constexpr (std::is_same_v<typename Law::Reg, const double*>)
        if (!aba) return pri ? fbd_euler_kernel<NV, HW, true, false, Law, Tau...> : fbd_euler_kernel<NV, HW, false, false, Law, Tau...>;
    return pri ? fbd_euler_kernel<NV, HW, true, true, Law, Tau...> : fbd_euler_kernel<NV, HW, false, true, Law, Tau...>;
}

// The launch of fbd_euler_kernel under one law: `ext` bytes of LDS behind each system's block in
// the two-systems layout, `tau` the law's leading kernel arguments (Tau as the kernel has it).
template <class Law, class... Tau>
static blf_status launch_euler_law(const blf_fb_model* md, const blf_fb_state* st, const blf_fb_contacts* ct,
                                   typename Law::Reg reg, int64_t batch, int32_t nsteps, double dT, double dT_last,
                                   hipStream_t s, const Law& law, size_t ext, Tau... tau)
{
    const Contacts c = to_contacts(ct);
    const bool pri = md->joint_type != nullptr;
    bool aba = true;
    if constexpr (std::is_same_v<typename Law::Reg, const double*>) aba = use_aba(reg);
    const size_t lds = fbd_lds_bytes(md->ndof, c.C, aba);
    return fb_launch("fbd_euler_kernel launch", fbd_euler_instance<32, 32, Law, Tau...>(pri, aba), lds + ext,
                     fbd_euler_instance<kNW, kWave, Law, Tau...>(pri, aba), lds, md->ndof, batch, s, to_model(md), *st,
                     tau..., c, reg, nsteps, dT, dT_last, law, batch);
}

blf_status launch_fbd_euler(const blf_fb_model* md, const blf_fb_state* st, const double* tau,
                            const blf_fb_contacts* ct, const double* reg, int64_t batch,
                            int32_t nsteps, double dT, double dT_last, hipStream_t s,
                            const blf_joint_impedance* impedance)
{
    Impedance imp{nullptr, nullptr, nullptr};
    if (impedance) imp = Impedance{impedance->kp, impedance->kd, impedance->q_ref};
    return launch_euler_law<Impedance, const double* __restrict__>(md, st, ct, reg, batch, nsteps, dT, dT_last, s, imp,
                                                                   0, tau);
}

blf_status launch_fbd_euler_traj(const blf_fb_model* md, const blf_fb_state* st, const blf_fb_contacts* ct,
                                 const double* reg, int64_t batch, int32_t nsteps, double dT, double dT_last,
                                 hipStream_t s, const blf_joint_impedance_traj* it)
{
    const ImpedanceTraj imp{it->kp, it->kd, it->q_ref, it->qd_ref, it->q_bias, it->qd_stride, it->slices,
                            it->steps_per_slice};
    // two systems per wavefront: the slice's qdref behind each system's block (the kernel's nx)
    const size_t ext = sizeof(double) * (size_t)((md->ndof + 1) & ~1);
    return launch_euler_law(md, st, ct, reg, batch, nsteps, dT, dT_last, s, imp, ext);
}

blf_status launch_fbd_euler_ctq(const blf_fb_model* md, const blf_fb_state* st, const blf_fb_contacts* ct,
                                int64_t batch, int32_t nsteps, double dT, double dT_last, hipStream_t s,
                                const blf_computed_torque_traj* it)
{
    const ComputedTorqueTraj law{it->kp, it->kd, it->q_ref, it->qd_ref, it->qdd_ref, it->q_bias, it->tau_max,
                                 it->tau_last, it->qd_stride, it->qdd_stride, it->slices, it->steps_per_slice};
    return launch_euler_law(md, st, ct, {}, batch, nsteps, dT, dT_last, s, law, 0);
}

blf_status launch_fb_invdyn(const blf_fb_model* md, const blf_fb_state* st, const double* joint_acc,
                            const double* base_acc, const blf_fb_contacts* ct, int64_t batch, double* tau,
                            double* bout, int32_t* status, hipStream_t s)
{
    const Contacts c = to_contacts(ct);
    const bool pri = md->joint_type != nullptr;
    const size_t lds = fbd_lds_bytes(md->ndof, c.C, true);
    return fb_launch("fb_invdyn_kernel launch", pri ? fb_invdyn_kernel<32, true> : fb_invdyn_kernel<32, false>, lds,
                     pri ? fb_invdyn_kernel<kWave, true> : fb_invdyn_kernel<kWave, false>, lds, md->ndof, batch, s,
                     to_model(md), *st, joint_acc, base_acc, c, tau, bout, status, batch);
}

blf_status launch_com_reference(const double* xi0, const double* vrp, int64_t vstride, const double* omega0,
                                int64_t ostride, const double* zref, double* cref, int32_t T, double dT,
                                int64_t batch, double* cpos, double* cvel, double* xiend, hipStream_t s)
{
    if (batch == 0) return BLF_OK;
    hipLaunchKernelGGL(com_reference_kernel, dim3((unsigned)ceil_div(2 * batch, 256)), dim3(256), 0, s, xi0, vrp,
                       vstride, omega0, ostride, zref, cref, T, dT, batch, cpos, cvel, xiend);
    return check_hip(hipGetLastError(), "com_reference_kernel launch");
}

blf_status launch_fb_dcm(const blf_fb_model* md, const blf_fb_state* st, const double* omega0,
                         int64_t ostride, int64_t batch, double* com, double* xi, hipStream_t s)
{
    if (batch == 0) return BLF_OK;
    const size_t lds = fbd_lds_bytes(md->ndof, 0, true);
    hipLaunchKernelGGL((md->joint_type ? fb_dcm_kernel<true> : fb_dcm_kernel<false>), dim3((unsigned)batch),
                       dim3(kWave), lds, s, to_model(md), *st,
                       omega0, ostride, com, xi);
    return check_hip(hipGetLastError(), "fb_dcm_kernel launch");
}

blf_status launch_fb_frame_state(const blf_fb_model* md, const blf_fb_state* st, int32_t K,
                                 const int32_t* frames, int64_t batch, double* pose, double* twist,
                                 hipStream_t s)
{
    if (batch == 0 || K == 0) return BLF_OK;
    const size_t lds = fbd_lds_bytes(md->ndof, 0, true);
    hipLaunchKernelGGL((md->joint_type ? fb_frame_state_kernel<true> : fb_frame_state_kernel<false>),
                       dim3((unsigned)batch), dim3(kWave), lds, s, to_model(md), *st, (int)K, frames,
                       pose, twist);
    return check_hip(hipGetLastError(), "fb_frame_state_kernel launch");
}

blf_status launch_posture_reference(const blf_posture_law* law, const double* com, const double* vrp,
                                    int64_t vstride, int64_t batch, double* qref, hipStream_t s)
{
    const int64_t total = batch * law->ndof;
    if (total == 0) return BLF_OK;
    hipLaunchKernelGGL(posture_reference_kernel, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, s,
                       law->ndof, law->q_nominal, law->lean, com, vrp, vstride, total, qref);
    return check_hip(hipGetLastError(), "posture_reference_kernel launch");
}

}  // namespace blf
