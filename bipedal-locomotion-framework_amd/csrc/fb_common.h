// fb_common.h -- the device code the floating-base kernel files share (fb_dynamics.hip: dynamics,
// Euler integration, centre of mass, frame states; fb_ik.hip: whole-body inverse kinematics): the
// LDS layout, the model, the tree topology, the forward kinematics and the staging of a system's
// state.
#pragma once

#include "blf_internal.h"

namespace blf {
namespace {

// Every kernel built on this header runs one 64-lane wavefront per workgroup, and the LDS operations of a
// wavefront complete in program order, so lanes exchanging data through LDS need only a compiler
// barrier between the write and the read (no s_barrier, no full s_waitcnt).
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// link record: R 9 | p 3 | w 3 | v 3 | al 3 | a 3 | spatial inertia 10 (m, h, Ibar xx xy xz yy yz zz)
//              | spatial force 6 (tau_O, f)
// Per-lane records are read and written lane-strided (lane l at l * stride), so every stride is
// an ODD number of doubles: consecutive lanes then fall on distinct LDS bank pairs and an 8-byte
// access of 32 lanes is conflict-free.  With the even strides of the data sizes (40, 16, 12, 6
// doubles) SQ_LDS_BANK_CONFLICT was 83k quad-cycles per wave, 16 % of the Euler kernel's cycles
// (profiles/r03_fbd_euler_sq.json).
constexpr int kPad = 1;

constexpr int kLinkRec = 40 + kPad;   // record stride (40 doubles of data)
constexpr int kR = 0, kP = 9, kW = 12, kV = 15, kAl = 18, kA = 21, kSI = 24, kSF = 34;
// The articulated-body layout (Smem aba): 27-double records.  Step 3 writes a link's spatial
// inertia / force over the first 16 doubles of its own record once it has read the kinematics
// (no other lane reads that record afterwards: the contacts, which do, run before step 3), and
// fbd_aba keeps joint j's slot (articulated inertia 21 | bias 6, later da 6) in link j + 1's record
// after reading that link's spatial terms.
constexpr int kLinkRecA = 27;
constexpr int kSIa = 0, kSFa = 10;
constexpr int kComp = 16;             // subtree sum: spatial inertia 10 | spatial force 6
constexpr int kCompS = kComp + kPad;  // its stride
constexpr int kCs = 16 + kPad;        // contact scratch: point 3 | wrench 6 | link 1 | spatial wrench 6
constexpr int kSax = 6 + kPad;        // column axis (w, u)

struct Smem {
    // one base pointer (per system: the two halves of a wavefront have their own) and wave-uniform
    // offsets, so the per-half base costs one address, not one per array
    double* base;
    int o_link, o_jz, o_jo, o_comp, o_sax, o_rhs, o_cscr, o_st, o_tq, o_anc, o_cst, o_imp;
    int ms;   // row stride of L (odd: the per-lane row accesses do not conflict)
    int lrec;   // link record stride: kLinkRec, or kLinkRecA for the articulated-body solve
    size_t total;
    // aba: the layout of the articulated-body solve (fbd_aba): records of kLinkRecA doubles that
    // later hold the spatial terms (kSIa / kSFa) and the joint slots, no subtree-sum / pivot-column
    // or column-axis arrays -- 9.3 KB per 30-DoF system instead of 19.2 KB, so two wavefronts of two
    // systems fit per SIMD
    __host__ __device__ Smem(double* b, int n, int C, bool aba = false) : base(b)
    {
        const int L = n + 1, NV = n + 6;
        ms = NV | 1;
        lrec = aba ? kLinkRecA : kLinkRec;
        size_t o = 0;
        auto take = [&](size_t k) {
            const int at = (int)o;
            o += (k + 1) & ~size_t(1);
            return at;
        };
        // link records; after the mass matrix is assembled the same space holds L (NV rows)
        const size_t lk = (size_t)lrec * L, lm = aba ? 0 : (size_t)NV * ms;
        o_link = take(lk > lm ? lk : lm);
        o_jz = take(3 * (size_t)n);
        o_jo = take(3 * (size_t)n);
        // subtree sums [j] (joint j's subtree) and [n] (every link); later the pivot-column
        // buffers of the factorization (two sets of up to 4 columns, 8 NV)
        const size_t cp = (size_t)kCompS * (n + 1);
        const size_t cb = 8 * (size_t)(NV > 32 ? NV : 32);
        o_comp = take(aba ? 0 : cp > cb ? cp : cb);
        o_sax = take(aba ? 0 : kSax * (size_t)NV);
        o_rhs = take((size_t)NV);
        o_cscr = take((size_t)kCs * (C > 0 ? C : 1));
        o_st = take(18 + 2 * (size_t)n + (size_t)NV + 9);   // Euler state (6 + n + 3 + 9 + n) + dR + ref 3 (kRef)
        o_tq = take((size_t)n);                              // the joint impedance's torques
        o_anc = take((size_t)L);
        // fbd_euler_kernel's per-system constants, staged once instead of read from global memory
        // every Euler step: each contact's link, frame pose, null pose and parameters
        // [C | 12 C | 12 C | 4 C]; the impedance's kp, kd, q_ref (3.793 / 3.773 against 3.805 /
        // 3.785 ms per c5 period, profiles/r04_cstage_asopq_ab.log)
        o_cst = take(29 * (size_t)C);
        o_imp = take(3 * (size_t)n);
        total = o;
    }
    __device__ __forceinline__ double* link() const { return base + o_link; }
    __device__ __forceinline__ double* jz() const { return base + o_jz; }
    __device__ __forceinline__ double* jo() const { return base + o_jo; }
    __device__ __forceinline__ double* comp() const { return base + o_comp; }
    __device__ __forceinline__ double* sax() const { return base + o_sax; }
    __device__ __forceinline__ double* rhs() const { return base + o_rhs; }
    __device__ __forceinline__ double* cscr() const { return base + o_cscr; }
    __device__ __forceinline__ double* st() const { return base + o_st; }
    __device__ __forceinline__ double* tq() const { return base + o_tq; }
    __device__ __forceinline__ double* cst() const { return base + o_cst; }
    __device__ __forceinline__ double* imp() const { return base + o_imp; }
    __device__ __forceinline__ unsigned long long* anc() const
    {
        return reinterpret_cast<unsigned long long*>(base + o_anc);
    }
};

struct Model {
    int n, F;
    const int32_t* parent;
    const double *jorig, *jrot, *jaxis, *mass, *com, *inertia, *fpose;
    const int32_t* flink;
    double g0, g1, g2, rho;
    const int32_t* jtype;   // [n] or nullptr: BLF_JOINT_PRISMATIC marks a sliding joint
    // unused (always null): dropping them moves the register allocation of the prismatic Euler kernels
    const double* cpose;
    const double* clink;
};

struct Contacts {
    int C;
    const int32_t* frame;
    const double* params;
    const double* null_pose;   // [B][C][12]
    const int32_t* law;        // [C] or null (every contact BLF_CONTACT_CONTINUOUS)
    const double* wrench;      // [B][C][6] the BLF_CONTACT_WRENCH contacts' wrenches
};

// Whether contact c applies the caller's wrench (BLF_CONTACT_WRENCH) instead of the
// ContinuousContactModel law
__device__ __forceinline__ bool given_wrench(const Contacts& ct, int c)
{
    return ct.law != nullptr && ct.law[c] == BLF_CONTACT_WRENCH;
}

__device__ __forceinline__ void cross3(const double* a, const double* b, double* o)
{
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

__device__ __forceinline__ double dot3(const double* a, const double* b)
{
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
}

// sym 3x3 (xx xy xz yy yz zz) times vector
__device__ __forceinline__ void sym_mv(const double* I, const double* x, double* y)
{
    y[0] = (I[0] * x[0] + I[1] * x[1]) + I[2] * x[2];
    y[1] = (I[1] * x[0] + I[3] * x[1]) + I[4] * x[2];
    y[2] = (I[2] * x[0] + I[4] * x[1]) + I[5] * x[2];
}

__device__ __forceinline__ double bcast(double v, int src)
{
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)b, src);
    const int hi = __builtin_amdgcn_readlane((int)(b >> 32), src);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// Systems per wavefront.  A model with NV = n + 6 <= 32 fits half a wavefront (lane hl < 32 owns
// joint / row hl), so one wavefront integrates two systems side by side, one per half (HW = 32
// lanes per system); larger models take the whole wavefront (HW = 64).  Every loop, mask and
// broadcast below is per half; both halves run the same model, so their control flow is the same.
template <int HW>
struct Half {
    int hl, half;   // lane within the system's half, and which half
    __device__ __forceinline__ Half() : hl(threadIdx.x & (HW - 1)), half(HW == 64 ? 0 : (int)threadIdx.x / HW) {}
    // a ballot restricted to this half (bit i = lane i of the half)
    __device__ __forceinline__ unsigned long long ballot(bool p) const
    {
        const unsigned long long b = __ballot(p);
        return HW == 64 ? b : (b >> (HW * half)) & ((1ull << HW) - 1);
    }
    // v of lane `src` of this half
    __device__ __forceinline__ int shfl(int v, int src) const { return __shfl(v, HW * half + src, kWave); }
    // v of lane k of this half, as a broadcast (v_readlane; two of them and a select for halves)
    __device__ __forceinline__ double bcast_k(double v, int k) const
    {
        if (HW == 64) return bcast(v, k);
        const double a = bcast(v, k), b = bcast(v, HW + k);
        return half ? b : a;
    }
};

// r[lane] of a register row (the diagonal entry of the lane's own row), compile-time indexed.
template <int NVMAX>
__device__ __forceinline__ double bcast_own_diag(const double* r, int lane)
{
    double d = 0.0;
#pragma unroll
    for (int k = 0; k < NVMAX; ++k)
        if (lane == k) d = r[k];
    return d;
}

// Tree topology, the same for every system and every Euler step: built once per workgroup.
// Lane j < n: joint j's parent link, origin, depth and child mask; anc[l] (LDS) every link's
// ancestor-joint mask.
struct Topo {
    int P, depth, maxdepth;
    double o0, o1, o2;
    unsigned long long cmask, bmask;
    int last;   // the last joint of joint lane's subtree (DFS preorder: the run [lane, last])
    int lastc;  // the same for column lane's joint (lane - 6; lanes < 6: 0)
    bool dfs;   // the joints are in DFS preorder (wave-uniform): every subtree is a contiguous run
};

template <int HW>
__device__ __forceinline__ Topo build_topo(const Model& m, const Smem& S)
{
    const Half<HW> H;
    const int n = m.n, lane = H.hl;
    const bool jl = lane < n;
    Topo t;
    t.P = jl ? m.parent[lane] : 0;
    t.o0 = jl ? m.jorig[3 * lane] : 0.0;
    t.o1 = jl ? m.jorig[3 * lane + 1] : 0.0;
    t.o2 = jl ? m.jorig[3 * lane + 2] : 0.0;
    // walk to the base through the parents held by the other lanes (joint Q - 1 moves link Q)
    unsigned long long an = jl ? 1ull << lane : 0ull;
    int depth = 0, Q = t.P;
    for (int it = 0; it < n; ++it) {
        const bool up = jl && Q > 0;
        if (!__ballot(up)) break;   // both halves hold the same model
        const int q = H.shfl(t.P, up ? Q - 1 : 0);
        if (up) {
            ++depth;
            an |= 1ull << (Q - 1);
            Q = q;
        }
    }
    t.depth = depth;
    if (jl) S.anc()[lane + 1] = an;
    if (lane == 0) S.anc()[0] = 0ull;
    t.cmask = 0ull;
    for (int j = 0; j < n; ++j) {
        const unsigned long long b = H.ballot(jl && t.P == j + 1);
        if (lane == j) t.cmask = b;
    }
    t.bmask = H.ballot(jl && t.P == 0);
    // DFS preorder: joint k attaches to the base or to a link on the path to link k (joint k - 1's
    // child), i.e. its parent link's joint is among joint k - 1's ancestors; then the subtree of
    // joint j is the run [j, j + size_j - 1], size_j = the joints whose ancestor masks hold j
    {
        const int src = lane > 0 ? lane - 1 : 0;
        const int lo = H.shfl((int)an, src), hi = H.shfl((int)(an >> 32), src);
        const unsigned long long prev = ((unsigned long long)(unsigned)hi << 32) | (unsigned)lo;
        const bool ok = !jl || lane == 0 || t.P == 0 || ((prev >> (t.P - 1)) & 1ull);
        t.dfs = H.ballot(!ok) == 0ull;
        int size = 0;
        for (int j = 0; j < n; ++j) {
            const int c = __builtin_popcountll(H.ballot(jl && ((an >> j) & 1ull)));
            if (lane == j) size = c;
        }
        t.last = jl ? lane + size - 1 : 0;
        t.lastc = H.shfl(t.last, lane >= 6 && lane < n + 6 ? lane - 6 : 0);
    }
    int md = depth;
#pragma unroll
    for (int off = HW / 2; off >= 1; off >>= 1) {
        const int q = __shfl_xor(md, off, kWave);
        md = q > md ? q : md;
    }
    t.maxdepth = __builtin_amdgcn_readfirstlane(md);
    wave_sync();
    return t;
}

// motion cross product (w, v) x (w2, v2) = (w x w2, w x v2 + v x w2), accumulated into o
__device__ __forceinline__ void crm_add(const double* s, const double* t, double* o)
{
    double a[3], b[3], c[3];
    cross3(s, t, a);
    cross3(s, t + 3, b);
    cross3(s + 3, t, c);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        o[i] = o[i] + a[i];
        o[3 + i] = o[3 + i] + (b[i] + c[i]);
    }
}

// Steps 1-2 of fbd_eval: per-joint rotations and forward kinematics (poses, mixed velocities,
// nu_dot = 0 accelerations) of every link into the link records.
// PRI: the model may hold prismatic joints (blf_fb_model.joint_type != NULL); the launchers
// instantiate the kernels both ways, so all-revolute models (config 5) pay nothing for it.
// By pointer jumping along the ancestor chains: every joint lane runs at once, and a chain of
// depth D takes ceil(log2(D + 1)) rounds instead of D + 1 tree levels (4.238 / 4.239 against
// 4.688 / 4.704 ms per c5 period of fbd_euler_kernel, 15.3k -> 9.3k cycles per evaluation;
// profiles/r04_fbd_kinjump_ab.log).
//  * Poses: lane j holds the transform (R, p) from link ptr (initially its parent; the base's
//    world pose is folded in at once where the parent is the base, ptr = 0 then means "anchored in
//    the world") to its link j + 1.  A round composes the record of link ptr -- the segment from
//    that link's own ptr -- in front: (R, p) <- (R_X R, p_X + R_X p), ptr <- ptr_X.
//  * Velocities and nu_dot = 0 accelerations as spatial vectors about the origin of the frame bp is
//    given in (the callers' reference point, see load_state): with the
//    joint motion U_k = qdot_k S_k (S_k = (z_k, o_k x z_k), prismatic (0, z_k)),
//      V_c = V_B + sum_{k in chain(c)} U_k,   A_c = A_B + V_B x s + sum_{i before k} U_i x U_k,
//    so the chain element (s, x) = (sum U, sum of the ordered cross products) composes as
//    (s_X + s_Y, x_X + x_Y + s_X x s_Y) -- the same jumping rounds.  The link records' mixed
//    quantities follow: w = V_w, v = V_v + w x p, al = A_w, a = A_v + al x p + w x v (V_B =
//    (w_B, v_B + p_B x w_B), A_B = (0, -(w_B x v_B)): the base's nu_dot = 0).
// A lane reads its partner's record before it writes its own in the same round: the wavefront's
// LDS operations complete in program order, so every read sees the previous round's values.
// Rounding differs from a level-by-level recursion (parity is the 1e-9 bar of the fb tests).
template <int HW, bool PRI>
__device__ __forceinline__ void fbd_kinematics(const Model& m, const Smem& S, const double* bv,
                                               const double* jvel, const double* bp, const double* bR,
                                               const double* jp, const Topo& T)
{
    const Half<HW> H;
    const int n = m.n;
    const int lane = H.hl;
    const bool jl = lane < n;
    const int maxdepth = T.maxdepth;
    const double sd = jl ? jvel[lane] : 0.0;
    double Rb[9], pb[3], wb[3], vb[3];
#pragma unroll
    for (int i = 0; i < 9; ++i) Rb[i] = bR[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        pb[i] = bp[i];
        vb[i] = bv[i];
        wb[i] = bv[3 + i];
    }
    if (lane == 0) {
        double* b = S.link();
        for (int i = 0; i < 9; ++i) b[kR + i] = Rb[i];
        for (int i = 0; i < 3; ++i) {
            b[kP + i] = pb[i]; b[kV + i] = vb[i]; b[kW + i] = wb[i];
            b[kAl + i] = 0.0; b[kA + i] = 0.0;
        }
    }
    // 1. the joint's own transform: E_j Rot(a_j, s_j) (Rodrigues) and the origin o_j (+ E_j a_j q)
    double R[9], p[3], ax[3];
    const bool pri = PRI && jl && m.jtype[lane] == BLF_JOINT_PRISMATIC;
    {
        const int j = jl ? lane : 0;
        const double* a = m.jaxis + 3 * j;
        const double* E = m.jrot + 9 * j;
        ax[0] = a[0]; ax[1] = a[1]; ax[2] = a[2];
        double sn = 0.0, cs = 1.0;
        if (jl && !pri) sincos(jp[j], &sn, &cs);
        if (PRI && jl && m.jtype[j] != BLF_JOINT_PRISMATIC && m.jtype[j] != BLF_JOINT_REVOLUTE)
            sn = cs = __builtin_nan("");   // an unknown joint type: the robot's outputs are NaN
        const double c1 = 1.0 - cs;
        const double K[9] = {0.0, -a[2], a[1], a[2], 0.0, -a[0], -a[1], a[0], 0.0};
        double Rr[9];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double K2 = (K[3 * r] * K[c] + K[3 * r + 1] * K[3 + c]) + K[3 * r + 2] * K[6 + c];
                Rr[3 * r + c] = ((r == c ? 1.0 : 0.0) + sn * K[3 * r + c]) + c1 * K2;
            }
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c)
                R[3 * r + c] = (E[3 * r] * Rr[c] + E[3 * r + 1] * Rr[3 + c]) + E[3 * r + 2] * Rr[6 + c];
        p[0] = T.o0; p[1] = T.o1; p[2] = T.o2;
        if (pri) {
            const double qj = jp[j];
#pragma unroll
            for (int r = 0; r < 3; ++r)
                p[r] = p[r] + ((E[3 * r] * a[0] + E[3 * r + 1] * a[1]) + E[3 * r + 2] * a[2]) * qj;
        }
    }
    // the transform (RX, pX) in front of (R, p)
    auto compose = [&](const double* RX, const double* pX) {
        double Rn[9], pn[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int c = 0; c < 3; ++c)
                Rn[3 * r + c] = (RX[3 * r] * R[c] + RX[3 * r + 1] * R[3 + c]) + RX[3 * r + 2] * R[6 + c];
            pn[r] = pX[r] + ((RX[3 * r] * p[0] + RX[3 * r + 1] * p[1]) + RX[3 * r + 2] * p[2]);
        }
#pragma unroll
        for (int i = 0; i < 9; ++i) R[i] = Rn[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) p[i] = pn[i];
    };
    int ptr = jl ? T.P : 0;
    if (jl && ptr == 0) compose(Rb, pb);
    double* own = S.link() + S.lrec * (lane + 1);
    if (jl) {
#pragma unroll
        for (int i = 0; i < 9; ++i) own[kR + i] = R[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) own[kP + i] = p[i];
    }
    wave_sync();
    // 2a. poses: ceil(log2(maxdepth + 1)) rounds
    for (int span = 1; span <= maxdepth; span <<= 1) {
        const bool act = jl && ptr > 0;
        const int pn = H.shfl(ptr, act ? ptr - 1 : 0);
        if (act) {
            const double* x = S.link() + S.lrec * ptr;
            double RX[9], pX[3];
#pragma unroll
            for (int i = 0; i < 9; ++i) RX[i] = x[kR + i];
#pragma unroll
            for (int i = 0; i < 3; ++i) pX[i] = x[kP + i];
            compose(RX, pX);
#pragma unroll
            for (int i = 0; i < 9; ++i) own[kR + i] = R[i];
#pragma unroll
            for (int i = 0; i < 3; ++i) own[kP + i] = p[i];
            ptr = pn;
        }
        wave_sync();
    }
    // 2b. the joint's world axis z = R_child a (Rot(a, s) a = a) and origin o = p_child; its motion
    double z[3], s[6], x[6];
#pragma unroll
    for (int r = 0; r < 3; ++r) z[r] = (R[3 * r] * ax[0] + R[3 * r + 1] * ax[1]) + R[3 * r + 2] * ax[2];
    {
        double oz[3];
        cross3(p, z, oz);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            s[i] = pri ? 0.0 : z[i] * sd;
            s[3 + i] = pri ? z[i] * sd : oz[i] * sd;
            x[i] = 0.0;
            x[3 + i] = 0.0;
        }
    }
    if (jl) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            S.jz()[3 * lane + a] = z[a];
            S.jo()[3 * lane + a] = p[a];
        }
        // the chain element in the record's w, v, al, a slots until the end
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            own[kW + i] = s[i];
            own[kAl + i] = x[i];
        }
    }
    wave_sync();
    // 2c. the chain sums: the same rounds
    ptr = jl ? T.P : 0;
    for (int span = 1; span <= maxdepth; span <<= 1) {
        const bool act = jl && ptr > 0;
        const int pn = H.shfl(ptr, act ? ptr - 1 : 0);
        if (act) {
            const double* e = S.link() + S.lrec * ptr;
            double sX[6], xX[6];
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                sX[i] = e[kW + i];
                xX[i] = e[kAl + i];
            }
#pragma unroll
            for (int i = 0; i < 6; ++i) x[i] = xX[i] + x[i];
            crm_add(sX, s, x);
#pragma unroll
            for (int i = 0; i < 6; ++i) s[i] = sX[i] + s[i];
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                own[kW + i] = s[i];
                own[kAl + i] = x[i];
            }
            ptr = pn;
        }
        wave_sync();
    }
    // 2d. the records' mixed velocities and accelerations
    if (jl) {
        double VB[6], A[6], t[3];
        cross3(pb, wb, t);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            VB[i] = wb[i];
            VB[3 + i] = vb[i] + t[i];
        }
        cross3(wb, vb, t);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            A[i] = x[i];
            A[3 + i] = x[3 + i] - t[i];
        }
        crm_add(VB, s, A);
        double w[3], v[3], al[3], acc[3], u[3], q[3], r[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            w[i] = VB[i] + s[i];
            al[i] = A[i];
        }
        cross3(w, p, u);
#pragma unroll
        for (int i = 0; i < 3; ++i) v[i] = (VB[3 + i] + s[3 + i]) + u[i];
        cross3(al, p, q);
        cross3(w, v, r);
#pragma unroll
        for (int i = 0; i < 3; ++i) acc[i] = (A[3 + i] + q[i]) + r[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            own[kW + i] = w[i];
            own[kV + i] = v[i];
            own[kAl + i] = al[i];
            own[kA + i] = acc[i];
        }
    }
    wave_sync();
}

// World transform pose = (p, R row-major) and mixed twist tw = (v, w) of the frame whose pose in
// its link is fp, from the link's kinematics record k (the getWorldTransform / getFrameVel the
// reference hands each contact model, FloatingBaseSystemDynamics.cpp:225-226)
__device__ __forceinline__ void frame_state(const double* k, const double* fp, double* pose, double* tw)
{
    const double* R = k + kR;
    double d[3], t1[3];
    for (int a = 0; a < 3; ++a) {
        pose[a] = k[kP + a] + ((R[3 * a] * fp[0] + R[3 * a + 1] * fp[1]) + R[3 * a + 2] * fp[2]);
        for (int b = 0; b < 3; ++b)
            pose[3 + 3 * a + b] = (R[3 * a] * fp[3 + b] + R[3 * a + 1] * fp[6 + b]) + R[3 * a + 2] * fp[9 + b];
        d[a] = pose[a] - k[kP + a];
    }
    cross3(k + kW, d, t1);
    for (int a = 0; a < 3; ++a) {
        tw[a] = k[kV + a] + t1[a];
        tw[3 + a] = k[kW + a];
    }
}

// A system's state in LDS (Smem st), the layout every kernel hands fbd_kinematics:
//   bv 6 | jv n | bp 3 | bR 9 | jp n [| dR 9: the rotation's rate, in the kernels that integrate] | ref 3
// The kernels work in the world frame TRANSLATED to the reference point ref = the system's base_pos
// at kernel entry: the bp slot holds base_pos - ref (zero at entry, exactly) and ref sits at
// kRef(n).  The spatial quantities of fbd_eval are taken about that point, so their size is the
// robot's, not its distance from the world origin (fb_dynamics.hip's header says why); whatever
// reads or writes a world position subtracts or adds ref there.
// load_state stages system q's from HBM, the half's lanes striding over the elements (the caller
// fences).  Used by fb_dcm_kernel and fb_frame_state_kernel; fbd_dynamics_kernel, fbd_euler_kernel
// and fb_ik_kernel (which stays in world coordinates: its point Jacobians lose accuracy only
// linearly with the distance) keep this loop as their own text: through this function some of
// their instantiations allocate registers differently and measured 1 to 16 % slower (DESIGN.md
// 3.2, "Sharing device code between the floating-base kernels").
__host__ __device__ constexpr int kRef(int n) { return 27 + 2 * n; }

template <int HW>
__device__ __forceinline__ void load_state(const blf_fb_state& st, int64_t q, int n, int lane, double* loc)
{
    const int64_t nq = (int64_t)n * q;
    for (int i = lane; i < 18 + 2 * n; i += HW) {
        double v;
        if (i < 6) v = st.base_vel[6 * q + i];
        else if (i < 6 + n) v = st.joint_vel[nq + (i - 6)];
        else if (i < 9 + n) {
            loc[kRef(n) + (i - 6 - n)] = st.base_pos[3 * q + (i - 6 - n)];
            v = 0.0;
        } else if (i < 18 + n) v = st.base_rot[9 * q + (i - 9 - n)];
        else v = st.joint_pos[nq + (i - 18 - n)];
        loc[i] = v;
    }
}

Model to_model(const blf_fb_model* md)
{
    Model m;
    m.n = md->ndof;
    m.F = md->nframes;
    m.parent = md->parent;
    m.jorig = md->joint_origin;
    m.jrot = md->joint_rot;
    m.jaxis = md->joint_axis;
    m.mass = md->link_mass;
    m.com = md->link_com;
    m.inertia = md->link_inertia;
    m.flink = md->frame_link;
    m.fpose = md->frame_pose;
    m.cpose = nullptr;
    m.clink = nullptr;
    m.g0 = md->gravity[0];
    m.g1 = md->gravity[1];
    m.g2 = md->gravity[2];
    m.rho = md->rho;
    m.jtype = md->joint_type;
    return m;
}

// The launch of every per-system kernel (see Half): while a system fits half a wavefront, n + 6 <= 32,
// kernel k2 with a block per two systems, each with lds2 bytes of LDS; otherwise k1 with a block and
// lds1 bytes per system.  Both kernels take the same arguments.  An empty batch launches nothing.
constexpr int kNW = BLF_FBD_MAX_DOFS + 6;   // the rows (NVMAX) of the one-system-per-wavefront instantiations
inline size_t fb_launch_lds(int n, size_t lds2, size_t lds1) { return n + 6 <= 32 ? 2 * lds2 : lds1; }

template <class... P, class... A>
blf_status fb_launch(const char* what, void (*k2)(P...), size_t lds2, void (*k1)(P...), size_t lds1, int n,
                     int64_t batch, hipStream_t s, const A&... args)
{
    if (batch == 0) return BLF_OK;
    const size_t lds = fb_launch_lds(n, lds2, lds1);
    if (n + 6 <= 32)
        hipLaunchKernelGGL(k2, dim3((unsigned)ceil_div(batch, 2)), dim3(kWave), lds, s, args...);
    else
        hipLaunchKernelGGL(k1, dim3((unsigned)batch), dim3(kWave), lds, s, args...);
    return check_hip(hipGetLastError(), what);
}

}  // namespace
}  // namespace blf
