// odometry.hip -- Contacts::SchmittTriggerDetector and Estimators::LeggedOdometry on the device
// (include/blf/blf_c.h section 13; neither class is in the reference snapshot, the header defines them).
//
//  * schmitt_trigger_kernel: one lane per trigger, B K of them, looping over the T samples of a call
//    with the trigger's state and timers in registers; sample t + 1 is loaded before sample t's step.
//  * legged_odometry_kernel: T steps of one robot per wavefront, or of two while n + 6 <= 32 (Half,
//    fb_common.h).  The model's topology is built once; every step runs fb_common.h's forward
//    kinematics with the base at the identity and at rest, so a link record holds the link's pose and
//    velocity relative to the base in base coordinates, and lane c < K evaluates frame_state for slot
//    c's frame and steps slot c's trigger (schmitt_math.h, the stand-alone kernel's own step).  The
//    base pose, the fixed-frame switch and the base twist are a few dozen operations per robot and
//    step: lane 0 of the half does them on the K frame records in LDS, away from the kinematics, and
//    the half stores the step's outputs a lane per element.  Step t + 1's joint_pos, joint_vel and
//    normal_force are in flight (one register each) during step t's pointer-jumping rounds.
// Built with -ffp-contract=off; tests/odometry_reference.py restates the section in numpy.
#include "fb_common.h"
#include "schmitt_math.h"

namespace blf {
namespace {

constexpr int kTrigBlock = 256;

__global__ __launch_bounds__(kTrigBlock) void schmitt_trigger_kernel(TrigParams tp, int K,
                                                                     const double* __restrict__ time,
                                                                     const double* __restrict__ value, int32_t T,
                                                                     int32_t* __restrict__ state,
                                                                     double* __restrict__ timers,
                                                                     int32_t* __restrict__ state_out, int64_t total)
{
    const int64_t i = (int64_t)blockIdx.x * kTrigBlock + threadIdx.x;
    if (i >= total) return;
    double prm[4];
    trig_row(tp, (int)(i % K), prm);
    int32_t st = state[i];
    double edge = timers[2 * i], sw = timers[2 * i + 1];
    double v = value[i];
    for (int32_t t = 0; t < T; ++t) {
        const double vn = t + 1 < T ? value[(int64_t)(t + 1) * total + i] : 0.0;
        schmitt_step(prm, time[t], v, st, edge, sw);
        if (state_out) state_out[(int64_t)t * total + i] = st & 1;
        v = vn;
    }
    state[i] = st;
    timers[2 * i] = edge;
    timers[2 * i + 1] = sw;
}

// What blf_legged_odometry_advance streams and keeps, as the kernel's one argument block
struct Odom {
    int K;
    const int32_t* frames;
    const double *time, *jpos, *jvel, *force;
    int32_t T;
    int32_t *tstate, *fixed;
    double *timers, *fpose;
    double *bpos, *brot, *bvel;
    int32_t *contact, *fout, *status;
};

// Behind a system's Smem block: fixed_pose 12 | the step's base pose and twist (p 3, R 9, v 3, w 3)
constexpr int kOdomFix = 0, kOdomOut = 12, kOdomExt = 32;
// A slot's frame record in Smem's cst array: pose 12 | twist 6 | contact state | switch_time
constexpr int kFr = 20 + kPad;

__host__ __device__ inline size_t odom_doubles(int n, int K) { return Smem(nullptr, n, K, true).total + kOdomExt; }

template <int HW, bool PRI>
__global__ __launch_bounds__(64) void legged_odometry_kernel(Model m, TrigParams tp, Odom od, int64_t batch)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const Half<HW> H;
    const int n = m.n, K = od.K;
    const Smem S(smem + H.half * odom_doubles(n, K), n, K, true);
    double* const ext = S.base + S.total;
    double* const fr = S.cst();
    const int64_t q0 = (int64_t)blockIdx.x * (kWave / HW) + H.half;
    const bool active = q0 < batch;   // an idle half repeats the last robot and stores nothing
    const int64_t q = active ? q0 : batch - 1;
    const int lane = H.hl;
    const bool jl = lane < n, cl = lane < K;
    double* loc = S.st();   // bv 6 | jv n | bp 3 | bR 9 | jp n: the base at the identity and at rest
    for (int i = lane; i < 18 + n; i += HW)
        if (i < 6 || i >= 6 + n) loc[i] = i >= 9 + n && (i - 9 - n) % 4 == 0 ? 1.0 : 0.0;
    if (lane < 12) ext[kOdomFix + lane] = od.fpose[12 * q + lane];
    // slot c's frame, trigger and parameters in lane c
    const int fc = cl ? od.frames[lane] : 0;
    const bool fbad = H.ballot(cl && (fc < 0 || fc >= m.F)) != 0ull;
    const int fi = fc >= 0 && fc < m.F ? fc : 0;
    const int flk = cl && !fbad ? m.flink[fi] : 0;
    double prm[4];
    trig_row(tp, lane, prm);
    int32_t ts = cl ? od.tstate[q * K + lane] : 0;
    double edge = cl ? od.timers[(q * K + lane) * 2] : 0.0, sw = cl ? od.timers[(q * K + lane) * 2 + 1] : 0.0;
    int f = od.fixed[q];     // lane 0's copy is the one that counts
    bool bad = fbad;         // likewise: sticky once set
    wave_sync();
    const Topo T = build_topo<HW>(m, S);
    const int64_t B = batch;
    double jp = jl ? od.jpos[q * n + lane] : 0.0;
    double jv = jl && od.jvel ? od.jvel[q * n + lane] : 0.0;
    double fv = cl ? od.force[q * K + lane] : 0.0;
    const double nan = __builtin_nan("");
    for (int32_t t = 0; t < od.T; ++t) {
        if (jl) {
            loc[6 + lane] = jv;
            loc[18 + n + lane] = jp;
        }
        const bool fin = __builtin_isfinite(jp) && __builtin_isfinite(jv) &&
                         (lane >= 12 || __builtin_isfinite(ext[kOdomFix + lane]));
        const double tm = od.time[t];
        const double fnow = fv;
        if (t + 1 < od.T) {   // the next step's samples: in flight over this step's kinematics
            const int64_t r = (int64_t)(t + 1) * B + q;
            jp = jl ? od.jpos[r * n + lane] : 0.0;
            jv = jl && od.jvel ? od.jvel[r * n + lane] : 0.0;
            fv = cl ? od.force[r * K + lane] : 0.0;
        }
        const bool inbad = H.ballot(!fin) != 0ull;
        wave_sync();
        fbd_kinematics<HW, PRI>(m, S, loc, loc + 6, loc + 6 + n, loc + 9 + n, loc + 18 + n, T);
        // 1. the triggers; 2. the frames relative to the base
        schmitt_step(prm, tm, fnow, ts, edge, sw);
        if (cl) {
            double* r = fr + kFr * lane;
            if (!fbad) frame_state(S.link() + S.lrec * flk, m.fpose + 12 * fi, r, r + 12);
            r[18] = (double)(ts & 1);
            r[19] = sw;
            if (active && od.contact) od.contact[((int64_t)t * B + q) * K + lane] = ts & 1;
        }
        wave_sync();
        if (lane == 0) {
            bad = bad || inbad || f < 0 || f >= K;
            const int fo = f >= 0 && f < K ? f : 0;
            const double* a = fr + kFr * fo;   // (p_f, R_f)
            double* fx = ext + kOdomFix;       // (P, Q)
            double* o = ext + kOdomOut;
            double RB[9], pB[3];
            // 3. R_B = Q R_f^T, p_B = P - R_B p_f
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j)
                    RB[3 * i + j] = (fx[3 + 3 * i] * a[3 + 3 * j] + fx[3 + 3 * i + 1] * a[3 + 3 * j + 1]) +
                                    fx[3 + 3 * i + 2] * a[3 + 3 * j + 2];
            for (int i = 0; i < 3; ++i)
                pB[i] = fx[i] - ((RB[3 * i] * a[0] + RB[3 * i + 1] * a[1]) + RB[3 * i + 2] * a[2]);
            // 4. the switch: slot f while it is on, else the slot on with the greatest switch_time
            int f2 = fo;
            if (a[18] == 0.0) {
                int best = -1;
                double bt = 0.0;
                for (int c = 0; c < K; ++c) {
                    const double* rc = fr + kFr * c;
                    if (rc[18] != 0.0 && (best < 0 || rc[19] > bt)) {
                        best = c;
                        bt = rc[19];
                    }
                }
                if (best >= 0) f2 = best;
            }
            const double* g = fr + kFr * f2;   // the new fixed frame: (p, R, v, w) relative to the base
            double np[12];
            for (int i = 0; i < 3; ++i) {
                np[i] = pB[i] + ((RB[3 * i] * g[0] + RB[3 * i + 1] * g[1]) + RB[3 * i + 2] * g[2]);
                for (int j = 0; j < 3; ++j)
                    np[3 + 3 * i + j] = (RB[3 * i] * g[3 + j] + RB[3 * i + 1] * g[6 + j]) + RB[3 * i + 2] * g[9 + j];
            }
            // 5. w_B = -R_B w_f, v_B = -R_B v_f - w_B x (R_B p_f)
            double ra[3], wB[3], vB[3], cr[3];
            for (int i = 0; i < 3; ++i) {
                ra[i] = (RB[3 * i] * g[0] + RB[3 * i + 1] * g[1]) + RB[3 * i + 2] * g[2];
                wB[i] = -((RB[3 * i] * g[15] + RB[3 * i + 1] * g[16]) + RB[3 * i + 2] * g[17]);
                vB[i] = -((RB[3 * i] * g[12] + RB[3 * i + 1] * g[13]) + RB[3 * i + 2] * g[14]);
            }
            cross3(wB, ra, cr);
            for (int i = 0; i < 3; ++i) vB[i] = vB[i] - cr[i];
            bool okv = true;
            for (int i = 0; i < 3; ++i) okv = okv && __builtin_isfinite(pB[i]) && __builtin_isfinite(vB[i]) && __builtin_isfinite(wB[i]);
            for (int i = 0; i < 9; ++i) okv = okv && __builtin_isfinite(RB[i]);
            bad = bad || !okv;
            if (!bad && f2 != fo)
                for (int i = 0; i < 12; ++i) fx[i] = np[i];
            if (!bad) f = f2;
            if (bad)
                for (int i = 0; i < 12; ++i) fx[i] = nan;
            for (int i = 0; i < 3; ++i) {
                o[i] = bad ? nan : pB[i];
                o[12 + i] = bad ? nan : vB[i];
                o[15 + i] = bad ? nan : wB[i];
            }
            for (int i = 0; i < 9; ++i) o[3 + i] = bad ? nan : RB[i];
            if (active && od.fout) od.fout[(int64_t)t * B + q] = bad ? -1 : f;
        }
        wave_sync();
        if (active && lane < 18) {
            const int64_t r = (int64_t)t * B + q;
            const double v = ext[kOdomOut + lane];
            if (lane < 3) {
                if (od.bpos) od.bpos[3 * r + lane] = v;
            } else if (lane < 12) {
                if (od.brot) od.brot[9 * r + (lane - 3)] = v;
            } else if (od.bvel) od.bvel[6 * r + (lane - 12)] = v;
        }
    }
    if (!active) return;
    if (cl) {
        od.tstate[q * K + lane] = ts;
        od.timers[(q * K + lane) * 2] = edge;
        od.timers[(q * K + lane) * 2 + 1] = sw;
    }
    if (lane < 12) od.fpose[12 * q + lane] = ext[kOdomFix + lane];
    if (lane == 0) {
        od.fixed[q] = f;
        if (od.status) od.status[q] = bad ? BLF_IK_BAD_INPUT : BLF_IK_OK;
    }
}

}  // namespace

size_t odometry_lds_bytes(int n, int K) { return sizeof(double) * odom_doubles(n, K); }

blf_status launch_schmitt_trigger(const double* params, int shared, int32_t K, const double* time,
                                  const double* value, int32_t steps, int32_t* state, double* timers,
                                  int32_t* state_out, int64_t batch, hipStream_t s)
{
    const int64_t total = batch * K;
    if (total == 0) return BLF_OK;
    TrigParams tp;
    for (int c = 0; c < BLF_ODOM_MAX_CONTACTS; ++c)
        for (int i = 0; i < 4; ++i) tp.p[c][i] = params[4 * (shared || c >= K ? 0 : c) + i];
    hipLaunchKernelGGL(schmitt_trigger_kernel, dim3((unsigned)ceil_div(total, kTrigBlock)), dim3(kTrigBlock), 0, s,
                       tp, (int)K, time, value, steps, state, timers, state_out, total);
    return check_hip(hipGetLastError(), "schmitt_trigger_kernel launch");
}

blf_status launch_legged_odometry(const blf_fb_model* md, int32_t K, const int32_t* frames, const double* params,
                                  int shared, const double* time, const double* joint_pos, const double* joint_vel,
                                  const double* normal_force, int32_t steps, int32_t* trig_state, double* trig_timers,
                                  int32_t* fixed_frame, double* fixed_pose, double* base_pos, double* base_rot,
                                  double* base_vel, int32_t* contact_out, int32_t* fixed_out, int32_t* status,
                                  int64_t batch, hipStream_t s)
{
    TrigParams tp;
    for (int c = 0; c < BLF_ODOM_MAX_CONTACTS; ++c)
        for (int i = 0; i < 4; ++i) tp.p[c][i] = params[4 * (shared || c >= K ? 0 : c) + i];
    const Odom od{(int)K, frames, time, joint_pos, joint_vel, normal_force, steps, trig_state, fixed_frame,
                  trig_timers, fixed_pose, base_pos, base_rot, base_vel, contact_out, fixed_out, status};
    const bool pri = md->joint_type != nullptr;
    const size_t lds = odometry_lds_bytes(md->ndof, K);
    return fb_launch("legged_odometry_kernel launch",
                     pri ? legged_odometry_kernel<32, true> : legged_odometry_kernel<32, false>, lds,
                     pri ? legged_odometry_kernel<kWave, true> : legged_odometry_kernel<kWave, false>, lds, md->ndof,
                     batch, s, to_model(md), tp, od, batch);
}

}  // namespace blf
