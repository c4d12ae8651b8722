/*
 * blf_c.h — C ABI of the MI355X-native batched DCM-MPC planning path.
 *
 * This is the drop-in boundary.  Every entry point takes plain pointers and sizes (no C++ or
 * torch types), returns a blf_status, and is stream-ordered on the hipStream_t passed in
 * (passed as `void*` so this header needs no HIP include; NULL = the default stream).
 * All device buffers are caller-owned and must be device-resident (hipMalloc'd or a torch CUDA
 * tensor's data_ptr()).  Layout convention: PROBLEM-MAJOR ("[B][...]", batch outermost, each
 * problem's arrays contiguous), innermost index = the spatial coordinate.  One workgroup (or one
 * lane for the rollout/eval kernels) serves one problem; see DESIGN.md for why.
 *
 * Which reference interface each entry point replaces (paths relative to the reference root,
 * src/...):
 *   blf_lti_euler_integrate   System/include/BipedalLocomotion/System/FixedStepIntegrator.tpp:21-72
 *                             + ForwardEuler.tpp:18-49 + System/src/LinearTimeInvariantSystem.cpp:40-74
 *                             (ForwardEuler<LinearTimeInvariantSystem>::integrate(t0, T))
 *   blf_dcm_euler_rollout     the same ForwardEuler<LTI> step applied per knot with
 *                             A = omega_k I, B = -omega_k I (LinearTimeInvariantSystem.cpp:13-38, :71)
 *   blf_hull2d_hrep           Planners/src/ConvexHullHelper.cpp:35-99 (buildConvexHull/getA/getB)
 *   blf_hull2d_contains       Planners/src/ConvexHullHelper.cpp:101-117 (doesPointBelongToConvexHull)
 *   blf_hullnd_hrep           ConvexHullHelper.cpp:35-99 on n x p points, any n
 *   blf_hull3d_hrep           ConvexHullHelper.cpp:35-99 on 3 x p points (Planners/tests/
 *                             ConvexHullHelperTest.cpp:15-63 is 3-D)
 *   blf_halfspace_contains    ConvexHullHelper.cpp:101-117 in any dimension
 *   blf_quintic_fit/_eval     ABSENT in the reference (QuinticSpline); knot rule
 *                             of Planners/src/ContactList.cpp:190-202 (getPresentContact, `<=`)
 *   blf_contact_model_eval    ContactModels/src/ContinuousContactModel.cpp:79-171, 223-254 behind the
 *                             lazy getters of ContactModels/src/ContactModel.cpp:12-92
 *                             (getContactWrench / getAutonomousDynamics / getControlMatrix /
 *                             getRegressor)
 *   blf_contact_point_wrench  ContinuousContactModel.cpp:173-221 (getForceAtPoint,
 *                             getTorqueGeneratedAtPoint)
 *   blf_fbk_dynamics          System/src/FloatingBaseSystemKinematics.cpp:36-73
 *   blf_fbk_euler_integrate   ForwardEuler<FloatingBaseSystemKinematics>::integrate
 *                             (FixedStepIntegrator.tpp:21-72 + ForwardEuler.tpp:18-49)
 *   blf_fbd_dynamics          System/src/FloatingBaseSystemDynamics.cpp:102-251
 *                             (FloatingBaseDynamicalSystem::dynamics; the rigid-body terms that the
 *                             reference takes from iDynTree KinDynComputations are computed here)
 *   blf_fbd_euler_integrate   ForwardEuler<FloatingBaseDynamicalSystem>::integrate
 *   blf_dcm_phase_expand      Planners/src/ContactPhaseList.cpp:16-84 phases looked up per knot with the
 *                             getPresentContact rule (ContactList.cpp:190-202), SURVEY.md 8(f) item 2
 *   blf_dcm_mpc_solve_phased  blf_dcm_phase_expand + blf_dcm_mpc_solve_warm fused: one
 *                             Advanceable::advance() (System/Advanceable.h:24-46) of the planner
 *   blf_fb_dcm / blf_dcm_posture_reference  the state -> plan and plan -> input maps a user
 *                             writes around Advanceable::advance() and ForwardEuler::integrate in a
 *                             closed loop (config 5); no reference counterpart
 *   blf_fbd_euler_integrate_impedance  blf_fbd_euler_integrate with a joint impedance as the
 *                             control input of every step (the user's per-step setControlInput)
 *   blf_fbd_euler_integrate_impedance_traj / blf_dcm_com_reference  the same with the reference
 *                             indexed by the step (a joint trajectory followed in one launch), and
 *                             the plan -> CoM set point map that feeds blf_fb_ik_track; no reference
 *                             counterpart
 *   blf_dcm_mpc_solve[_warm]  ABSENT in the reference (TimeVaryingDCMPlanner QP),
 *                             driven through System/Advanceable.h:24-46 (advance()) by the C++ host
 *                             adapter blf::Planners::TimeVaryingDCMPlanner
 *   blf_rls_advance           Estimators/src/RecursiveLeastSquare.cpp:96-133
 *                             (RecursiveLeastSquare::advance(), T steps of a batch of filters)
 *   blf_contact_rls_advance   the same advance() with ContinuousContactModel::getRegressor()
 *                             (ContinuousContactModel.cpp:223-254) as the regressor function: the
 *                             online identification of a contact's spring and damper
 *   blf_swing_foot_eval / blf_so3_eval  ABSENT in the reference snapshot (SwingFootPlanner and
 *                             SO3Planner, added upstream later): defined by section 11 below; the
 *                             contact lookup is getPresentContact (ContactList.cpp:190-202)
 */
#ifndef BLF_C_H
#define BLF_C_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status ------------------------------------------------------------------------------- */
typedef int32_t blf_status;
#define BLF_OK                   0
#define BLF_ERR_INVALID_ARGUMENT 1  /* bad size / null pointer / bad parameter                   */
#define BLF_ERR_HIP              2  /* a HIP runtime call failed (see blf_last_error())          */
#define BLF_ERR_UNSUPPORTED      3  /* size outside what the kernels are built for               */
#define BLF_ERR_TIME_INTERVAL    4  /* reference rejects: initialTime > finalTime or dT <= 0     */
#define BLF_ERR_EMPTY_INTERVAL   5  /* initialTime == finalTime: the reference loops forever
                                       (FixedStepIntegrator.tpp:96-99, size_t vs -1); we refuse  */

/* per-problem solver status written by blf_dcm_mpc_solve */
#define BLF_QP_SOLVED        0
#define BLF_QP_MAX_ITER      1
#define BLF_QP_NUMERICAL     2   /* non-finite iterate or non-positive-definite KKT block        */
#define BLF_QP_BAD_FACETS    3   /* nfacets[k] outside [0, max_facets]                            */

typedef struct blf_handle blf_handle;

/* Create a handle bound to HIP device `device`.  Fails with BLF_ERR_HIP if no device.  A handle
 * keeps, per stream it solves QPs on, a small device work list (the problems the active-set
 * kernel hands to the interior point kernel; allocated at the first solve on the stream and grown,
 * after a synchronisation of that stream, when a batch outgrows it).  Solves on one handle and one
 * stream must be enqueued from one host thread at a time. */
blf_status blf_create(blf_handle** handle, int32_t device);
blf_status blf_destroy(blf_handle* handle);
/* Human-readable description of the last error on this thread (never NULL). */
const char* blf_last_error(void);
/* Version string of the library: "blf-mi355x <version> (abi <n>, ...) src <hash>".  ABI 3 (0.3.0)
 * is additive: it adds blf_rls_advance and blf_contact_rls_advance and changes no existing entry
 * point or struct.  blf_swing_foot_eval and blf_so3_eval, and later blf_fb_ik_solve_hard and
 * blf_fb_ik_integrate_hard (section 12b), then blf_fb_ik_solve_limits and
 * blf_fb_ik_integrate_limits (section 12c), then blf_fb_ik_track (section 12d), then blf_fbd_euler_integrate_impedance_traj
 * (section 9) and blf_dcm_com_reference (section 9b), then blf_fb_inverse_dynamics (section 8b) and
 * blf_fbd_euler_integrate_computed_torque_traj (section 9), were added within ABI 3 (no existing
 * entry point or struct changed, so the number stays): a caller detects them by symbol
 * (dlsym).  ABI 2 (0.2.0) added the optional pointer fields blf_dcm_mpc_solution.passes and blf_fb_contacts.law / .wrench:
 * a caller built against an older header must zero-initialise these structs (`= {0}`), since the
 * library reads every field as a device pointer or NULL.  Solves that use a stream's stage-2 list
 * (blf_dcm_mpc_solve*) are refused with BLF_ERR_UNSUPPORTED while that stream is being captured
 * into a graph: the list's slot is sequenced on the host. */
#define BLF_ABI_VERSION 3
const char* blf_version(void);
/* QP kernel routing for A/B and parity tests (no reference counterpart; the defaults are the
 * product's).  fuse_stage2 = 0: small cold batches with N <= 64 run the IPM's stage 2 as its own
 * launch instead of inside the active-set kernel; single_kernel = 1: every QP runs in the
 * interior point kernel alone (no active-set kernel).  -1 leaves a setting unchanged.  The initial
 * values come from BLF_QP_FUSE_STAGE2 / BLF_QP_SINGLE_KERNEL, read once at the first solve.  The
 * setting is process-wide (every handle and thread), not per handle. */
blf_status blf_set_qp_launch_mode(int32_t fuse_stage2, int32_t single_kernel);
/* ---- 0. FixedStepIntegrator::integrate's step schedule (FixedStepIntegrator.tpp:21-72) -------
 * The validation (in the reference's order) and schedule every batched integrator below uses:
 * iterations = (int)ceil((T - t0) / dT); steps i = 0..iterations-2 run at currentTime = t0 + dT*i
 * with step dT; the last step runs at the stale currentTime (t0 + dT*(iterations-2), or t0 when
 * iterations < 2), *t_last, with step *dT_last = T - *t_last.  Errors: BLF_ERR_TIME_INTERVAL
 * (t0 > T or dT <= 0), BLF_ERR_EMPTY_INTERVAL (t0 == T), BLF_ERR_UNSUPPORTED (>= 2e9 steps).
 * Host-only; used by include/blf/forward_euler_device.h to integrate user systems. */
blf_status blf_step_schedule(double initial_time, double final_time, double dT,
                             int32_t* iterations, double* dT_last, double* t_last);

/* ---- 1. ForwardEuler<LinearTimeInvariantSystem>::integrate(t0, T), batched ------------------
 * x_{i+1} = x_i + (A x_i + B u) * dT_i over the reference's step schedule:
 *   iters = (int)ceil((T - t0) / dT); steps i = 0..iters-2 advance by dT; the final step
 *   advances by (T - currentTime) with the stale currentTime = t0 + dT*(iters-2) (0 if iters<2).
 * A: [B][n][n] row-major, Bm: [B][n][m] (or a single shared matrix when `shared_matrices` != 0),
 * u: [B][m] (held constant, as setControlInput does), x: [B][n] updated in place.
 * n, m >= 1, any size (n, m <= 8: one lane per system, registers; up to 512: one 64-lane
 * workgroup per system, state in LDS; larger: one 256-thread workgroup per system, state in x and
 * a stream-ordered scratch — the same arithmetic order everywhere, so the same bits).  Arithmetic order (no FMA contraction): dx_r = (sum_c A_rc x_c) + (sum_c B_rc u_c),
 * each sum left to right; x_r = x_r + dx_r * dT_i.                                            */
blf_status blf_lti_euler_integrate(blf_handle* handle, int32_t n, int32_t m,
                                   const double* A, const double* Bm, int32_t shared_matrices,
                                   const double* u, double* x, int64_t batch,
                                   double initial_time, double final_time, double dT,
                                   void* stream);

/* LinearTimeInvariantSystem::dynamics (LinearTimeInvariantSystem.cpp:40-74), batched:
 * dx = A x + B u with the same summation order as blf_lti_euler_integrate; dx: [B][n]. */
blf_status blf_lti_dynamics(blf_handle* handle, int32_t n, int32_t m, const double* A,
                            const double* Bm, int32_t shared_matrices, const double* u,
                            const double* x, double* dx, int64_t batch, void* stream);

/* ---- 2. DCM rollout: one reference Euler step per knot -------------------------------------
 * xi_{k+1} = xi_k + ((omega_k * xi_k) + (-omega_k * r_k)) * dt,  k = 0..N-1
 * xi0: [B][2], omega: [B][N], vrp: [B][N][2], xi_out: [B][N+1][2] (xi_out[:,0] = xi0).       */
blf_status blf_dcm_euler_rollout(blf_handle* handle, const double* xi0, const double* omega,
                                 const double* vrp, int32_t horizon, double dt,
                                 double* xi_out, int64_t batch, void* stream);

/* ---- 3. Support polygon H-representation (ConvexHullHelper, 2-D) ---------------------------
 * pts: [B][P][2] (P <= BLF_HULL_MAX_POINTS), npts: [B] valid point count (<= P).
 * Output, padded to `max_facets` rows: A: [B][max_facets][2] unit outward normals,
 * b: [B][max_facets] offsets (inside: A x <= b), nfacets: [B] facet count (rows >= nfacets are
 * zero rows with b = 0).  Collinear boundary points are merged (Qhull "Qt" merges them too, see
 * ConvexHullHelper.cpp:54-58).  Facets are ordered counter-clockwise from the lowest-leftmost
 * vertex; Qhull's order is internal, so compare as sets.  If the hull needs more than
 * max_facets rows, or fewer than 3 distinct non-collinear points are given, nfacets = -1.     */
#define BLF_HULL_MAX_POINTS 16
blf_status blf_hull2d_hrep(blf_handle* handle, const double* pts, const int32_t* npts,
                           int32_t max_points, int32_t max_facets, int64_t batch,
                           double* A, double* b, int32_t* nfacets, void* stream);

/* doesPointBelongToConvexHull: inside[q] = 1 iff for all rows i < nfacets: (A p)_i <= b_i
 * (strict `>` rejects, no tolerance, ConvexHullHelper.cpp:110-114).  One query point per polygon:
 * query: [B][2], inside: [B] int32.  A polygon with nfacets < 0 or nfacets > max_facets gives 0
 * (a bad polygon: no row past its own max_facets is read).                                     */
blf_status blf_hull2d_contains(blf_handle* handle, const double* A, const double* b,
                               const int32_t* nfacets, int32_t max_facets, const double* query,
                               int64_t batch, int32_t* inside, void* stream);

/* 3-D H-representation (ConvexHullHelper on 3 x p points).  pts: [B][P][3] (P <=
 * BLF_HULL_MAX_POINTS), npts: [B].  Output padded to max_facets rows: A: [B][max_facets][3] unit
 * outward normals, b: [B][max_facets] (inside: A x <= b), nfacets: [B].  The rows are the distinct
 * supporting planes of the set (a face Qhull "Qt" splits into triangles is one row here; compare
 * as sets of planes), b = the largest n . p over the input points, so every input point is
 * inside exactly.  nfacets = -1 for fewer than 4 points, a flat set, or more than max_facets
 * planes.  Rule and tolerances: oracle orc_hull3d_hrep.                                       */
#define BLF_HULL3D_MAX_FACETS 64
blf_status blf_hull3d_hrep(blf_handle* handle, const double* pts, const int32_t* npts,
                           int32_t max_points, int32_t max_facets, int64_t batch,
                           double* A, double* b, int32_t* nfacets, void* stream);

/* n-D H-representation (ConvexHullHelper on n x p points, any n: ConvexHullHelper.cpp:35-99 hands
 * the matrix to Qhull).  pts: [B][P][dim] (1 <= dim <= BLF_HULLND_MAX_DIM, P <=
 * BLF_HULLND_MAX_POINTS, C(P, dim) <= BLF_HULLND_MAX_SUBSETS), npts: [B].  Output padded to
 * max_facets rows (<= BLF_HULLND_MAX_FACETS): A: [B][max_facets][dim] unit outward normals,
 * b: [B][max_facets] (inside: A x <= b), nfacets: [B].  The rows are the distinct supporting
 * hyperplanes through dim of the points (a facet Qhull "Qt" splits into simplices is one row;
 * compare as sets), b = the largest n . p over the points; dim = 1: the rows +1 / -1.
 * nfacets = -1 for fewer than dim + 1 points, a set spanning fewer than dim dimensions, or more
 * than max_facets planes.  One wavefront per set.  Rule and order: oracle orc_hullnd_hrep. */
#define BLF_HULLND_MAX_DIM 8
#define BLF_HULLND_MAX_POINTS 32
#define BLF_HULLND_MAX_FACETS 1024
#define BLF_HULLND_MAX_SUBSETS (1 << 20)
blf_status blf_hullnd_hrep(blf_handle* handle, int32_t dim, const double* pts, const int32_t* npts,
                           int32_t max_points, int32_t max_facets, int64_t batch, double* A,
                           double* b, int32_t* nfacets, void* stream);

/* doesPointBelongToConvexHull in `dim` dimensions: A: [B][max_facets][dim], b: [B][max_facets],
 * query: [B][dim]; inside[q] = 1 iff no row i < nfacets has (A p)_i > b_i (sum in column order
 * from 0.0).  nfacets < 0 or nfacets > max_facets gives 0.                                      */
blf_status blf_halfspace_contains(blf_handle* handle, const double* A, const double* b,
                                  const int32_t* nfacets, int32_t dim, int32_t max_facets,
                                  const double* query, int64_t batch, int32_t* inside,
                                  void* stream);

/* ---- 4. Quintic spline (swing foot) -------------------------------------------------------
 * A spline has K+1 knots t_0 < ... < t_K, and per knot and per axis (D axes, D <= 3) the
 * position, velocity and acceleration.  Segment j spans [t_j, t_{j+1}] and is the unique
 * quintic matching (p, v, a) at both ends.
 * fit:  knots_t: [S][K+1], knots_pva: [S][K+1][3 (p,v,a)][D]  ->  coeffs: [S][K][D][6]
 *       (c0..c5 of p(tau) = sum c_i tau^i, tau = t - t_j).
 * eval: query t: [S][Q]; segment = last knot j with t_j <= t, clamped to [0, K-1] (the
 *       getPresentContact rule, ContactList.cpp:190-202; t < t_0 -> segment 0); tau = t - t_j;
 *       pva out: [S][Q][3][D] (position, velocity, acceleration), knot_idx out: [S][Q].     */
blf_status blf_quintic_fit(blf_handle* handle, const double* knots_t, const double* knots_pva,
                           int32_t nknots, int32_t dim, int64_t nsplines, double* coeffs,
                           void* stream);
blf_status blf_quintic_eval(blf_handle* handle, const double* knots_t, const double* coeffs,
                            int32_t nknots, int32_t dim, int64_t nsplines, const double* tq,
                            int32_t nq, double* pva, int32_t* knot_idx, void* stream);

/* ---- 5. Time-varying DCM MPC QP (TimeVaryingDCMPlanner), batched ---------------------------
 * Per problem, with alpha_k = 1 + dt*omega_k, beta_k = dt*omega_k:
 *   min  sum_{k=0}^{N-1} 1/2|xi_k - xi_ref_k|^2_Q + 1/2|r_k - r_ref_k|^2_R + 1/2|xi_N - xi_ref_N|^2_P
 *   s.t. xi_0 = xi_init,  xi_{k+1} = xi_k + dt*omega_k*(xi_k - r_k)  (reference Euler step),
 *        A_k r_k <= b_k  (rows i < nfacets[k] of the support polygon H-rep)
 * Solved by a Mehrotra primal-dual interior point method whose Newton systems are factored by a
 * Riccati recursion over the knots (DESIGN.md section 4 gives the exact iteration).           */
typedef struct blf_dcm_mpc_params {
    int32_t horizon;       /* N >= 1                                                        */
    int32_t max_facets;    /* M, 1..16 (padded facet slots per knot; above 8 the interior     *
                            * point kernel alone: support polygons of three or four contacts) */
    int32_t max_iter;      /* IPM iteration cap (e.g. 50)                                   */
    int32_t reserved;      /* must be 0                                                     */
    double dt;             /* knot spacing [s]                                              */
    double w_xi[2];        /* Q diagonal                                                    */
    double w_vrp[2];       /* R diagonal                                                    */
    double w_terminal[2];  /* P diagonal                                                    */
    double tol_mu;         /* stop when mean complementarity <= tol_mu ...                   */
    double tol_primal;     /* ... and max |primal residual|, |dynamics defect| <= tol_primal */
    double tol_dual;       /* ... and the tracked dual residual bound <= tol_dual            */
    double tol_polish;     /* > 0: once mean complementarity <= tol_polish, try the active-set
                            * polish: one Newton step of the QP with the guessed
                            * active facets as equalities, accepted only if it certifies as the
                            * optimum (primal feasible, stationary, multipliers >= 0 to
                            * tol_primal / tol_dual); else the IPM goes on.  0: IPM only.     */
} blf_dcm_mpc_params;

typedef struct blf_dcm_mpc_problem {
    const double* xi_init;   /* [B][2]                                                      */
    const double* omega;     /* [B][N]      omega_k = sqrt(g / z_k)                          */
    const double* xi_ref;    /* [B][N+1][2]                                                 */
    const double* vrp_ref;   /* [B][N][2]   also the IPM's initial VRP guess                 */
    const double* A;         /* [B][N][M][2]                                                */
    const double* b;         /* [B][N][M]                                                   */
    const int32_t* nfacets;  /* [B][N]                                                      */
} blf_dcm_mpc_problem;

typedef struct blf_dcm_mpc_solution {
    double* xi;              /* [B][N+1][2]                                                 */
    double* vrp;             /* [B][N][2]                                                   */
    int32_t* status;         /* [B]  BLF_QP_*                                               */
    int32_t* iters;          /* [B]  IPM iterations taken                                   */
    int32_t* polished;       /* [B]  optional (NULL: not written): 1 if the solution is the
                              *      certified active-set polish, 0 if the IPM's own iterate    */
    int32_t* passes;         /* [B]  optional (NULL: not written): the drop/add passes the
                              *      active-set kernels ran (a cold start's fp32 search plus its
                              *      fp64 passes; a warm start's fp64 passes), what a warm start
                              *      saves; 0 for a problem the interior point kernel solves alone
                              *      (horizon > 128, max_facets > 8, tol_polish = 0)             */
} blf_dcm_mpc_solution;

/* Warm start of a receding-horizon re-solve (TimeVaryingDCMPlanner::advance()):
 * knot k of the new window starts from knot k + shift of a previous solution of the same plan
 * (shift = 1 after the window moved one knot):
 *   r_k = vrp[k + shift],  s_i = max(b_i - a_i r_k, floor),  lambda_i = max(lambda[k + shift][i], floor)
 * and the cold start's LQ step is skipped.  Knots with k + shift >= N are new to the window and
 * start cold (r_k = vrp_ref_k, s_i = max(b_i - a_i r_k, 1e-2), lambda_i = 1e-2 / s_i).
 * prev_status (optional): the status of the solve that produced vrp / lambda.  A problem whose
 * previous status is not BLF_QP_OK (e.g. BLF_QP_MAX_ITER) is not warm-started from that iterate:
 * it is solved exactly as the cold start (warm == NULL) solves it, so one failed window does not
 * poison the next (Advanceable::advance, System/include/BipedalLocomotion/System/Advanceable.h:24-46,
 * is called again after a failure with the planner's previous state).  A warm-started problem
 * (horizon <= 128, the active-set kernels' range) whose warm passes do not certify is solved
 * again from the cold start as well, the interior point method included (round 5; oracle
 * orc_dcm_mpc_solve_warm): the same result as a cold solve of it.               */
typedef struct blf_dcm_mpc_warm_start {
    const double* vrp;       /* [B][N][2]  VRPs of the previous solve (must not alias the output) */
    const double* lambda;    /* [B][N][M]  its multipliers (blf_dcm_mpc_solve_warm's lambda_out)  */
    int32_t shift;           /* >= 0                                                          */
    int32_t reserved;        /* must be 0                                                     */
    double floor;            /* > 0, e.g. 1e-2                                                */
    const int32_t* prev_status; /* [B] or NULL (NULL: every problem warm-started)             */
} blf_dcm_mpc_warm_start;

/* Batches of at most this many QPs (horizon <= 64) evaluate the solver's recursions in a
 * different association order (the DPP scan tree), tuned for latency; larger
 * batches use the throughput tree.  Both return the certified optimum; the two orders can differ
 * in the last bits, so a problem is bit-reproducible within either size class (and bit-identical to
 * the oracle, which follows the same rule). */
#define BLF_DPP_TREE_MAX_BATCH 1024

/* Fill `p` with the defaults used by the benchmark (dt 0.02, Q 1e2, R 1, P 1e3, tol_mu 1e-16,
 * tol_primal 1e-10, tol_dual 1e-9, tol_polish 3e-4, max_iter 50, max_facets 8). */
void blf_dcm_mpc_default_params(blf_dcm_mpc_params* p, int32_t horizon);

blf_status blf_dcm_mpc_solve(blf_handle* handle, const blf_dcm_mpc_params* params,
                             const blf_dcm_mpc_problem* problem, int64_t batch,
                             const blf_dcm_mpc_solution* solution, void* stream);

/* blf_dcm_mpc_solve from the warm start `warm` (NULL: the cold start, identical to
 * blf_dcm_mpc_solve).  lambda_out [B][N][M] (or NULL) receives the final multipliers, zero in
 * facet slots >= nfacets[k]; it is the next advance()'s warm->lambda.                         */
blf_status blf_dcm_mpc_solve_warm(blf_handle* handle, const blf_dcm_mpc_params* params,
                                  const blf_dcm_mpc_problem* problem,
                                  const blf_dcm_mpc_warm_start* warm, int64_t batch,
                                  const blf_dcm_mpc_solution* solution, double* lambda_out,
                                  void* stream);

/* ---- 5b. Knot -> contact-phase expansion (receding-horizon windows on the device) -----------
 * The phases of each problem's plan (ContactPhaseList::createPhases, Planners/src/
 * ContactPhaseList.cpp:16-84), sorted by begin time, with the H-rep of each phase's support
 * polygon (blf_hull2d_hrep over the phase's active-contact corners) and its reference point:
 *   begin, end: [B][P];  A: [B][P][M][2];  b: [B][P][M];  nfacets: [B][P];  ref: [B][P][2];
 *   nphases: [B] (phases >= nphases[q] are ignored).
 * For the window of knots t_k = (start_knot + k) dt, k = 0..N, knot k belongs to phase
 *   p = the last phase with begin_p <= t_k (the getPresentContact rule, ContactList.cpp:190-202)
 * when t_k < end_p, else to no phase.  Outputs (the blf_dcm_mpc_problem arrays of the window):
 *   A [B][N][M][2], b [B][N][M] = phase p's rows verbatim; nfacets [B][N] = phase p's count;
 *   xi_ref [B][N+1][2] and vrp_ref [B][N][2] = phase p's reference point; a knot outside every
 *   phase gets nfacets = -1 (the QP reports BLF_QP_BAD_FACETS) and zero rows / references.   */
typedef struct blf_phase_table {
    int32_t max_phases;        /* P >= 1                                                     */
    int32_t max_facets;        /* M, 1..16                                                   */
    const int32_t* nphases;    /* [B]                                                        */
    const double* begin;       /* [B][P]                                                     */
    const double* end;         /* [B][P]                                                     */
    const double* A;           /* [B][P][M][2]                                               */
    const double* b;           /* [B][P][M]                                                  */
    const int32_t* nfacets;    /* [B][P]                                                     */
    const double* ref;         /* [B][P][2]                                                  */
} blf_phase_table;

blf_status blf_dcm_phase_expand(blf_handle* handle, const blf_phase_table* phases,
                                int64_t start_knot, double dt, int32_t horizon, int64_t batch,
                                double* A, double* b, int32_t* nfacets, double* xi_ref,
                                double* vrp_ref, void* stream);

/* ---- 5c. Phase-indexed solve: one advance() of the receding horizon in one call ---------------
 * blf_dcm_phase_expand(phases, start_knot, params->dt, params->horizon) followed by
 * blf_dcm_mpc_solve_warm on the expanded window, with the same results bit for bit, for horizons
 * up to 128 (larger: BLF_ERR_UNSUPPORTED; use the two calls).  The window's rows are expanded from
 * the phase table into the solver's on-chip memory instead of through HBM: a problem reads its
 * phase table (a few KB) instead of the window's per-knot arrays (~19 KB at N = 100, M = 8).
 * phases->max_facets must equal params->max_facets.  omega: row q (the window's N values) at
 * omega + q * omega_stride (omega_stride >= N; e.g. the plan's omega shifted by start_knot, no
 * copy).  xi_init, warm, solution and lambda_out as blf_dcm_mpc_solve_warm.
 * window: blf_dcm_phase_expand's output arrays plus the window's omega (omega [B][N]), used as
 * scratch: a problem the active-set passes do not certify continues in the interior point method,
 * which reads its expanded window from there.  Only such problems' rows are written (none, with
 * the default parameters, in every workload measured); the contents are unspecified otherwise. */
typedef struct blf_dcm_mpc_window {
    double* omega;             /* [B][N]                                                     */
    double* xi_ref;            /* [B][N+1][2]                                                */
    double* vrp_ref;           /* [B][N][2]                                                  */
    double* A;                 /* [B][N][M][2]                                               */
    double* b;                 /* [B][N][M]                                                  */
    int32_t* nfacets;          /* [B][N]                                                     */
} blf_dcm_mpc_window;

blf_status blf_dcm_mpc_solve_phased(blf_handle* handle, const blf_dcm_mpc_params* params,
                                    const blf_phase_table* phases, int64_t start_knot,
                                    const double* xi_init, const double* omega,
                                    int64_t omega_stride, const blf_dcm_mpc_warm_start* warm,
                                    int64_t batch, const blf_dcm_mpc_window* window,
                                    const blf_dcm_mpc_solution* solution, double* lambda_out,
                                    void* stream);
/* ---- 6. Contact model (ContinuousContactModel), batched ------------------------------------
 * Rectangular L x W patch, spring k, damper b (ContinuousContactModel.h:22-57).
 * params: [B][4] = {length, width, spring_coeff, damper_coeff} (or one shared [4] when
 * shared_params != 0); twist: [B][6] = {v, w} in mixed representation; pose, null_pose:
 * [B][12] = {p[3], R[9] row-major} (world_T_link and the null-force transform).
 * Outputs (NULL = not computed): wrench [B][6] = {force, torque}; autonomous [B][6] and
 * control [B][36] (6x6 row-major), with d(wrench)/dt = autonomous + control * (dv, dw);
 * regressor [B][12] (6x2 row-major), wrench = regressor * (k, b).
 * As the reference: the wrench and the regressor scale by |R22|, the autonomous dynamics and
 * the control matrix by R22 (no abs, ContinuousContactModel.cpp:127-170).                   */
blf_status blf_contact_model_eval(blf_handle* handle, const double* params, int32_t shared_params,
                                  const double* twist, const double* pose,
                                  const double* null_pose, int64_t batch, double* wrench,
                                  double* autonomous, double* control, double* regressor,
                                  void* stream);

/* Force and torque (about the contact frame origin) generated at Q points (x, y) of each contact
 * surface: points [B][Q][2] -> force, torque [B][Q][3]; zero outside the rectangle.           */
blf_status blf_contact_point_wrench(blf_handle* handle, const double* params,
                                    int32_t shared_params, const double* twist, const double* pose,
                                    const double* null_pose, int64_t batch, const double* points,
                                    int32_t npoints, double* force, double* torque, void* stream);

/* ---- 7. Floating-base kinematics (FloatingBaseSystemKinematics), batched -------------------
 * State (p [B][3], R [B][9] row-major, s [B][ndof]); input (twist [B][6] mixed, s_dot [B][ndof]):
 *   dp = v,  dR = -R.colwise().cross(w) + rho/2 ((R R^T)^{-1} - I) R,  ds = s_dot
 * (Baumgarte parameter rho, default 0.01 in the reference).  ndof <= BLF_FBK_MAX_DOFS.      */
#define BLF_FBK_MAX_DOFS 64
blf_status blf_fbk_dynamics(blf_handle* handle, int32_t ndof, double rho, const double* rot,
                            const double* twist, const double* joint_vel, double* dpos,
                            double* drot, double* djoints, int64_t batch, void* stream);

/* ForwardEuler<FloatingBaseSystemKinematics>::integrate(t0, T) with the inputs held constant:
 * the step schedule and error codes of blf_lti_euler_integrate; every step updates each state
 * element x += dx * dT_i (no re-projection onto SO(3), as ForwardEuler.tpp:37-45).
 * pos, rot, joints are updated in place.                                                      */
blf_status blf_fbk_euler_integrate(blf_handle* handle, int32_t ndof, double rho, double* pos,
                                   double* rot, double* joints, const double* twist,
                                   const double* joint_vel, int64_t batch, double initial_time,
                                   double final_time, double dT, void* stream);

/* ---- 8. Floating-base dynamics (FloatingBaseDynamicalSystem), batched ----------------------
 * A kinematic tree of ndof revolute joints on a 6-DoF floating base (the robot model the reference
 * loads into iDynTree KinDynComputations; blf/robot.py documents the layout).  All pointers are
 * device memory.  Link 0 is the base; joint j moves link j + 1, whose parent link is parent[j]
 * (<= j).  Velocities are in the MIXED representation (iDynTree's default): the base twist is
 * (dp_B/dt, omega_B) in world coordinates.                                                      */
#define BLF_FBD_MAX_DOFS 48
#define BLF_FBD_MAX_CONTACTS 8
typedef struct blf_fb_model {
    int32_t ndof;                 /* n, 1..BLF_FBD_MAX_DOFS                                 */
    int32_t nframes;              /* F, frames contacts may be attached to                  */
    const int32_t* parent;        /* [n]                                                     */
    const double* joint_origin;   /* [n][3]  joint origin in the parent link frame           */
    const double* joint_rot;      /* [n][9]  fixed rotation parent link -> joint frame        */
    const double* joint_axis;     /* [n][3]  unit axis in the joint frame                    */
    const double* link_mass;      /* [n+1]                                                   */
    const double* link_com;       /* [n+1][3] COM in the link frame                         */
    const double* link_inertia;   /* [n+1][9] inertia about the COM, link frame              */
    const int32_t* frame_link;    /* [F]                                                     */
    const double* frame_pose;     /* [F][12] (p, R) of the frame in its link frame           */
    double gravity[3];            /* (0, 0, -9.81) in the reference                          */
    double rho;                   /* Baumgarte parameter of the base rotation rate           */
    const int32_t* joint_type;    /* [n] or NULL (every joint revolute): BLF_JOINT_REVOLUTE /
                                     BLF_JOINT_PRISMATIC (the child link slides along the axis
                                     by q; URDF "prismatic"); any other value makes every
                                     output of every robot NaN (the wrappers refuse it up
                                     front: the C++ adapter's setRobotModel returns false,
                                     blf.native raises).  Fixed joints carry no DoF: merge
                                     them into their parent link first (the C++ adapter's
                                     blf::reduceFixedJoints)                                  */
} blf_fb_model;
#define BLF_JOINT_REVOLUTE  0
#define BLF_JOINT_PRISMATIC 1

/* The state tuple (FloatingBaseSystemDynamics.h: base velocity, joint velocities, base position,
 * base orientation, joint positions); the same struct carries the state derivative (base
 * acceleration, joint accelerations, base linear velocity, base rotation rate, joint velocities). */
typedef struct blf_fb_state {
    double* base_vel;   /* [B][6]  */
    double* joint_vel;  /* [B][n]  */
    double* base_pos;   /* [B][3]  */
    double* base_rot;   /* [B][9]  row-major */
    double* joint_pos;  /* [B][n]  */
} blf_fb_state;

/* Contacts of the control input (the reference's std::vector<ContactWrench>, each a frame index
 * and a std::weak_ptr<ContactModel>; FloatingBaseSystemDynamics.cpp:198-228 maps every contact's
 * getContactWrench() through the frame Jacobian).  Each contact follows one of two laws:
 *   BLF_CONTACT_CONTINUOUS  a ContinuousContactModel (params, null_pose), updated on the device
 *                           with the frame's world transform and mixed velocity at every
 *                           evaluation, as the reference's setState + getContactWrench;
 *   BLF_CONTACT_WRENCH      any other ContactModel: the caller evaluates it (its setState from
 *                           blf_fb_frame_state, then getContactWrench) and passes the wrench,
 *                           (force, torque) in the mixed representation at the frame; held
 *                           constant over one blf_fbd_euler_integrate call (the C++ adapter
 *                           integrates step by step when a contact has this law).
 * law == NULL: every contact BLF_CONTACT_CONTINUOUS; any law value other than BLF_CONTACT_WRENCH
 * is taken as continuous.  params and null_pose are required for every contact (ignored for
 * BLF_CONTACT_WRENCH ones), wrench whenever law is given. */
#define BLF_CONTACT_CONTINUOUS 0
#define BLF_CONTACT_WRENCH     1
typedef struct blf_fb_contacts {
    int32_t ncontacts;            /* 0..BLF_FBD_MAX_CONTACTS                                  */
    const int32_t* frame;         /* [C] frame indices                                       */
    const double* params;         /* [C][4] (length, width, spring_coeff, damper_coeff)      */
    const double* null_pose;      /* [B][C][12] null-force transforms                        */
    const int32_t* law;           /* [C] BLF_CONTACT_* or NULL (all continuous)              */
    const double* wrench;         /* [B][C][6] wrenches of the BLF_CONTACT_WRENCH contacts   */
} blf_fb_contacts;

/* The world transform pose [B][K][12] = (p, R row-major) and the mixed velocity twist [B][K][6]
 * = (v, w) of K frames of every system (either output may be NULL): what the reference hands a
 * contact model through kinDyn getWorldTransform / getFrameVel (FloatingBaseSystemDynamics.cpp:
 * 225-226) before it asks for the wrench, for the caller's BLF_CONTACT_WRENCH models.  A frame
 * index outside [0, model->nframes) yields NaN pose and twist for that frame (no read past the
 * model).                                                                                        */
blf_status blf_fb_frame_state(blf_handle* handle, const blf_fb_model* model,
                              const blf_fb_state* state, int32_t nframes, const int32_t* frames,
                              int64_t batch, double* pose, double* twist, void* stream);

/* FloatingBaseDynamicalSystem::dynamics for a batch:
 *   nu_dot = LLT(M [+ mass_reg]) \ (-h + sum_c J_c^T w_c + [0; tau]),  dp = v_B,
 *   dR = -R.colwise().cross(w_B) + rho/2 ((R R^T)^{-1} - I) R,  ds = s_dot
 * joint_torque [B][n]; mass_reg [(n+6)^2] row-major or NULL; out receives the derivative. */
blf_status blf_fbd_dynamics(blf_handle* handle, const blf_fb_model* model,
                            const blf_fb_state* state, const double* joint_torque,
                            const blf_fb_contacts* contacts, const double* mass_reg,
                            int64_t batch, const blf_fb_state* out, void* stream);

/* ForwardEuler<FloatingBaseDynamicalSystem>::integrate(t0, T): the schedule and errors of
 * blf_lti_euler_integrate; each step evaluates the dynamics at the current state (torques and
 * contact parameters held constant) and updates every state element x += dx * dT_i.           */
blf_status blf_fbd_euler_integrate(blf_handle* handle, const blf_fb_model* model,
                                   const blf_fb_state* state, const double* joint_torque,
                                   const blf_fb_contacts* contacts, const double* mass_reg,
                                   int64_t batch, double initial_time, double final_time,
                                   double dT, void* stream);

/* ---- 8b. Floating-base inverse dynamics (KinDynComputations::inverseDynamics /
 *          generalizedBiasForces; the closed form of a TSID with joint-tracking, base-dynamics and
 *          joint-dynamics tasks under compliant contacts) ---------------------------------------
 * With M(q) and h(q, nu) the mass matrix and generalized bias forces of section 8 (mixed
 * representation), w_c contact c's wrench at the current state and J_c its frame's mixed Jacobian,
 * both exactly as blf_fbd_dynamics forms them (BLF_CONTACT_CONTINUOUS and BLF_CONTACT_WRENCH laws;
 * contacts NULL or ncontacts == 0: no contact), and sdd = joint_acc [B][n] (NULL: zero):
 *
 * Free-base mode (base_acc == NULL): base_acc_out [B][6] (mixed: linear then angular, the layout
 * of blf_fbd_dynamics' out->base_vel) and joint_torque [B][n] are the unique pair with
 *     M [nu_dot_B; sdd] + h = sum_c J_c^T w_c + [0; tau].
 *   base_acc_out and joint_torque are required; base_wrench is not written.
 *
 * Given-base mode (base_acc [B][6] given, mixed): joint_torque and base_wrench [B][6] (force then
 * torque, mixed, at the base origin) are together
 *     [base_wrench; tau] = M [base_acc; sdd] + h - sum_c J_c^T w_c,
 *   iDynTree's inverseDynamics.  With base_acc = 0, sdd = 0 and no contacts it is
 *   generalizedBiasForces; with nu = 0 as well, the gravity torques.  joint_torque and base_wrench
 *   are required; base_acc_out is not written.
 *
 * status [B] (or NULL) is per robot and reuses section 12's codes: BLF_IK_OK (0); BLF_IK_BAD_INPUT
 * when the robot's state, joint_acc, base_acc or a BLF_CONTACT_WRENCH wrench is not finite;
 * BLF_IK_NOT_POSITIVE when a pivot of the whole-body 6 x 6 inertia (free-base mode's LDL^T) is
 * not a finite positive number.  Either gives that robot NaN in every output of its own and touches
 * no other robot.  An unknown joint_type makes every output NaN, as in section 8.
 * BLF_ERR_INVALID_ARGUMENT: NULL handle, model, state, model array or (batch > 0) state buffer or
 * required output, reserved != 0, negative batch.  BLF_ERR_UNSUPPORTED as blf_fbd_dynamics: ndof
 * outside [1, BLF_FBD_MAX_DOFS], more than BLF_FBD_MAX_CONTACTS contacts.  batch == 0: BLF_OK.
 * One kernel launch on `stream`, no staged copy and no host synchronisation (capturable).  The
 * cost is one outward and one inward pass over the tree and a 6 x 6 solve: no mass matrix.        */
blf_status blf_fb_inverse_dynamics(blf_handle* handle, const blf_fb_model* model,
                                   const blf_fb_state* state, const double* joint_acc,
                                   const double* base_acc, const blf_fb_contacts* contacts,
                                   int64_t batch, double* joint_torque, double* base_acc_out,
                                   double* base_wrench, int32_t* status, int32_t reserved,
                                   void* stream);

/* ---- 9. Closed loop (BASELINE.json configs[4]): the maps between the robot and the planner ----
 * The reference has no closed-loop API: a user drives TimeVaryingDCMPlanner::advance()
 * (System/Advanceable.h:24-46) and ForwardEuler<FloatingBaseDynamicalSystem>::integrate
 * (ForwardEuler.tpp:18-49 over FloatingBaseSystemDynamics.cpp:102-251) in turn and maps the robot
 * state to the plan's initial DCM and the plan to the robot's input.  These two entry points are
 * those maps:
 *
 * blf_fb_dcm: state -> centre of mass c, its velocity cdot and the DCM
 *   c = sum_l m_l (p_l + R_l com_l) / m,  cdot = sum_l m_l (v_l + w_l x R_l com_l) / m,
 *   xi = c_xy + cdot_xy / omega0[b * omega0_stride]  (the plan's first-knot omega).
 *   com [B][6] = (c, cdot); xi [B][2] (may be the next solve's xi_init) or NULL.            */
blf_status blf_fb_dcm(blf_handle* handle, const blf_fb_model* model, const blf_fb_state* state,
                      const double* omega0, int64_t omega0_stride, int64_t batch, double* com,
                      double* xi, void* stream);

/* blf_dcm_posture_reference: plan -> joint references, held over the control period:
 *   q_ref[b][j] = q_nominal_j + lean_j0 (r0_x - c_x) + lean_j1 (r0_y - c_y)
 *   with r0 = vrp[b * vrp_stride + (0, 1)] (the plan's first VRP) and c = com[b][0..1].  The joint
 *   impedance of blf_fbd_euler_integrate_impedance tracks them.                               */
typedef struct blf_posture_law {
    int32_t ndof;                 /* n                                                       */
    int32_t reserved;             /* must be 0                                               */
    const double* q_nominal;      /* [n]                                                     */
    const double* lean;           /* [n][2] joint offset per metre of (r0 - c)              */
} blf_posture_law;
blf_status blf_dcm_posture_reference(blf_handle* handle, const blf_posture_law* law,
                                     const double* com, const double* vrp, int64_t vrp_stride,
                                     int64_t batch, double* q_ref, void* stream);
/* blf_fbd_euler_integrate_impedance: ForwardEuler<FloatingBaseDynamicalSystem>::integrate(t0, T)
 * (the schedule of blf_fbd_euler_integrate) with the control input set before EVERY step from a
 * joint impedance, tau = kp (q_ref - q) - kd qdot at the step's start state: the reference loop
 * `system->setControlInput(tau(x)); integrator.integrate(t_i, t_i + dT_i)` a user writes for a
 * joint-level controller faster than the planner, in one launch.                             */
typedef struct blf_joint_impedance {
    int32_t ndof;                 /* n, must match the model                                 */
    int32_t reserved;             /* must be 0                                               */
    const double* kp;             /* [n]                                                     */
    const double* kd;             /* [n]                                                     */
    const double* q_ref;          /* [B][n]                                                  */
} blf_joint_impedance;
blf_status blf_fbd_euler_integrate_impedance(blf_handle* handle, const blf_fb_model* model,
                                             const blf_fb_state* state,
                                             const blf_joint_impedance* impedance,
                                             const blf_fb_contacts* contacts,
                                             const double* mass_reg, int64_t batch,
                                             double initial_time, double final_time, double dT,
                                             void* stream);
/* blf_fbd_euler_integrate_impedance_traj: blf_fbd_euler_integrate_impedance with the reference
 * indexed by the integration step, a velocity feed-forward and a per-robot bias, so that a joint
 * trajectory (blf_fb_ik_track's joint_traj / nu_traj as they stand) is followed in one launch.  The
 * schedule is blf_step_schedule's, unchanged (the stale last step included).  Integration step i of
 * the call (0-based) uses slice
 *   s(i) = min(i / steps_per_slice, slices - 1)        (integer division; the last slice is held)
 * and, with r_j = q_ref[s][b][j] + q_bias[b][j] (q_bias NULL: r_j = q_ref[s][b][j], no addition),
 *   tau_j = kp_j (r_j - q_j) - kd_j (qdot_j - qd_ref[s][b][j])      (qd_ref NULL: - kd_j qdot_j,
 * the expression of blf_fbd_euler_integrate_impedance: with qd_ref and q_bias NULL and identical
 * slices the call equals that one bit for bit).  Slices past the last one used are never read.  A
 * non-finite reference of robot b gives that robot a NaN state and touches no other robot.
 * BLF_ERR_INVALID_ARGUMENT: what blf_fbd_euler_integrate_impedance refuses, slices < 1,
 * steps_per_slice < 1, reserved != 0, qd_stride < n with qd_ref set, ndof != the model's.           */
typedef struct blf_joint_impedance_traj {
    int32_t ndof;                 /* n, must match the model                                 */
    int32_t slices;               /* T >= 1                                                  */
    int32_t steps_per_slice;      /* >= 1                                                    */
    int32_t reserved;             /* must be 0                                               */
    const double* kp;             /* [n]                                                     */
    const double* kd;             /* [n]                                                     */
    const double* q_ref;          /* [T][B][n]: blf_fb_ik_track's joint_traj as it stands    */
    const double* qd_ref;         /* element (t,b,j) at qd_ref[(t*B + b)*qd_stride + j], or NULL
                                     (zero): nu_traj + 6 with qd_stride = 6 + n              */
    int64_t qd_stride;            /* >= n when qd_ref                                        */
    const double* q_bias;         /* [B][n] or NULL: added to every slice                    */
} blf_joint_impedance_traj;
blf_status blf_fbd_euler_integrate_impedance_traj(blf_handle* handle, const blf_fb_model* model,
                                                  const blf_fb_state* state,
                                                  const blf_joint_impedance_traj* impedance,
                                                  const blf_fb_contacts* contacts,
                                                  const double* mass_reg, int64_t batch,
                                                  double initial_time, double final_time, double dT,
                                                  void* stream);

/* blf_fbd_euler_integrate_computed_torque_traj: blf_fbd_euler_integrate_impedance_traj with the
 * torque law replaced by computed torque.  The schedule (blf_step_schedule's, the stale last step
 * included), the slice index s(i) = min(i / steps_per_slice, slices - 1) and the layouts of q_ref,
 * qd_ref and q_bias are that call's; qdd_ref is strided like qd_ref (NULL: zero).  kp and kd are
 * ACCELERATION gains (1/s^2 and 1/s).  Before every step, at the step's start state,
 *   sdd_j = qdd_ref[s][b][j] + kp_j (q_ref[s][b][j] + q_bias[b][j] - q_j) + kd_j (qd_ref[s][b][j] - qdot_j)
 *   tau   = the joint torques of blf_fb_inverse_dynamics' free-base mode at sdd, with the call's contacts
 *   tau_j = min(max(tau_j, -tau_max_j), tau_max_j)   when tau_max [n] (finite, > 0) is given
 * and the step is the forward evaluation of blf_fbd_dynamics with that tau as the control input
 * (always run, clamped or not: the torque is the actual input) and the Euler update of
 * blf_fbd_euler_integrate.  Unclamped, every joint then follows
 *   q_j += h qdot_j,  qdot_j += h sdd_j
 * whatever the base, the contacts and the other joints do.  The call does not check the gains
 * against the step: explicit Euler needs the eigenvalues of [[1, h], [-kp h, 1 - kd h]] inside the
 * unit circle for every step length h of the schedule, the 2 h of a stale last step included; for
 * kd = 2 sqrt(kp) the condition is sqrt(kp) h < 2.
 * tau_last [B][n] or NULL: the torque applied at the last step.  A non-finite reference of robot b
 * gives that robot a NaN state (and tau_last) and touches no other robot; so does a failed pivot
 * of either evaluation.  Slices past the last one used are never read.
 * BLF_ERR_INVALID_ARGUMENT: what blf_fbd_euler_integrate_impedance_traj refuses, and qdd_stride < n
 * with qdd_ref set.  BLF_ERR_UNSUPPORTED: mass_reg != NULL (inverse dynamics is defined without
 * the regularisation), and what blf_fbd_dynamics refuses as unsupported.                          */
typedef struct blf_computed_torque_traj {
    int32_t ndof;                 /* n, must match the model                                 */
    int32_t slices;               /* T >= 1                                                  */
    int32_t steps_per_slice;      /* >= 1                                                    */
    int32_t reserved;             /* must be 0                                               */
    const double* kp;             /* [n] 1/s^2                                               */
    const double* kd;             /* [n] 1/s                                                 */
    const double* q_ref;          /* [T][B][n]                                               */
    const double* qd_ref;         /* element (t,b,j) at qd_ref[(t*B + b)*qd_stride + j], or NULL */
    int64_t qd_stride;            /* >= n when qd_ref                                        */
    const double* qdd_ref;        /* element (t,b,j) at qdd_ref[(t*B + b)*qdd_stride + j], or NULL */
    int64_t qdd_stride;           /* >= n when qdd_ref                                       */
    const double* q_bias;         /* [B][n] or NULL: added to every slice                    */
    const double* tau_max;        /* [n] or NULL: the torque bound, finite and > 0           */
    double* tau_last;             /* [B][n] or NULL: the last step's applied torque          */
} blf_computed_torque_traj;
blf_status blf_fbd_euler_integrate_computed_torque_traj(blf_handle* handle, const blf_fb_model* model,
                                                        const blf_fb_state* state,
                                                        const blf_computed_torque_traj* law,
                                                        const blf_fb_contacts* contacts,
                                                        const double* mass_reg, int64_t batch,
                                                        double initial_time, double final_time,
                                                        double dT, void* stream);

/* ---- 9b. Closed loop: the plan -> centre-of-mass reference map ---------------------------------
 * blf_dcm_com_reference: the set points blf_ik_schedule reads (com_pos, com_vel [B][T][3]) from a
 * solved DCM window: the LIP's stable half cdot = omega (xi - c) integrated by T explicit Euler
 * steps of dT under the plan's first VRP r0 = vrp[b * vrp_stride + (0, 1)], held over the period,
 * with omega = omega0[b * omega0_stride].  Per robot b and horizontal axis a, in this order:
 *   xi_0 = xi0[b][a],  c_0 = c_ref[b][a],  nwr = -omega * r0_a
 *   for t = 0 .. T-1:
 *     v_t = omega * (xi_t - c_t)
 *     com_pos[b][t] = (c_t[0], c_t[1], z_ref[b]),  com_vel[b][t] = (v_t[0], v_t[1], 0)
 *     c_{t+1}  = c_t + v_t * dT
 *     xi_{t+1} = xi_t + ((omega * xi_t) + nwr) * dT                      (section 2's step)
 *   c_ref[b][a] = c_T (in place: the reference carries over to the next period; feedback enters
 *   through xi0 only),  xi_end[b][a] = xi_T when xi_end is given.
 * xi0 [B][2] (blf_fb_dcm's xi), z_ref [B], c_ref [B][2], xi_end [B][2] or NULL.  A robot with a
 * non-finite xi0, r0, omega, z_ref or c_ref gets NaN in every output of its own (com_pos, com_vel,
 * c_ref, xi_end); no other robot is touched.  NULL handle or buffer (batch > 0), steps < 1, a dT
 * that is not finite and positive, vrp_stride < 2 or a negative omega0_stride or batch:
 * BLF_ERR_INVALID_ARGUMENT, nothing written; batch == 0: BLF_OK.                                 */
blf_status blf_dcm_com_reference(blf_handle* handle, const double* xi0, const double* vrp,
                                 int64_t vrp_stride, const double* omega0, int64_t omega0_stride,
                                 const double* z_ref, double* c_ref, int32_t steps, double dT,
                                 int64_t batch, double* com_pos, double* com_vel, double* xi_end,
                                 void* stream);

/* ---- 10. Recursive least squares (Estimators::RecursiveLeastSquare), batched ------------------
 * B independent filters, each with state x (n), covariance P (n x n), forgetting factor lambda and
 * a diagonal measurement covariance R = diag(r) (m).  One step with regressor H (m x n) and
 * measurements y (m) is the reference's advance() (RecursiveLeastSquare.cpp:119-130):
 *   K = P H^T (lambda R + H P H^T)^-1;  x <- x + K (y - H x);  P <- (P - K H P) / lambda.
 * R is diagonal, so the step is evaluated as m sequential scalar updates and one division (the
 * same minimiser and the same P in exact arithmetic, P+ = (lambda P^-1 + H^T R^-1 H)^-1; no m x m
 * inverse).  Only the upper triangle of P is kept: the input covariance is read through its upper
 * triangle and the output is mirrored, so it is exactly symmetric.
 * Arithmetic order (no FMA contraction; every sum left to right, starting from its first term).
 * For each row j = 0..m-1 of H, h = H[j][:]:
 *   g_a = sum_c P[a][c] h_c                       (P[a][c] = P[c][a] for a > c)
 *   s   = (lambda * r_j) + sum_a h_a g_a
 *   e   = y_j - sum_a h_a x_a
 *   k_a = g_a / s
 *   x_a = x_a + k_a * e
 *   P[a][b] = P[a][b] - k_a * g_b                 (a <= b)
 * and after the m rows P[a][b] = P[a][b] / lambda.  If s is not a finite positive number (NaN, <=
 * 0 or +inf: e.g. r_j = 0 with a zero row), every element of that filter's x and P becomes NaN at
 * that row and stays NaN; other filters are unaffected.
 * Samples are STEP-MAJOR: regressor [T][B][m][n], measurements [T][B][m] (each step one contiguous
 * batch array, what blf_contact_model_eval produces per period; a closed loop calls with
 * steps = 1).  meas_cov: [m] when shared_cov != 0, else [B][m].  state [B][n] and covariance
 * [B][n][n] (row-major) are updated in place.  Errors: null handle or pointer, steps < 1,
 * batch < 0, lambda not finite or not positive: BLF_ERR_INVALID_ARGUMENT; n outside
 * 1..BLF_RLS_MAX_STATE or m outside 1..BLF_RLS_MAX_MEAS: BLF_ERR_UNSUPPORTED; batch == 0: BLF_OK. */
#define BLF_RLS_MAX_STATE 8
#define BLF_RLS_MAX_MEAS  8
blf_status blf_rls_advance(blf_handle* handle, int32_t n, int32_t m, double lambda,
                           const double* meas_cov, int32_t shared_cov, const double* regressor,
                           const double* measurements, int32_t steps, double* state,
                           double* covariance, int64_t batch, void* stream);

/* The identification of a ContinuousContactModel's (spring_coeff, damper_coeff) from measured
 * wrenches: blf_rls_advance with n = 2, m = 6, whose regressor of step t is
 * blf_contact_model_eval's `regressor` output for (geometry, twist[t], pose[t], null_pose), formed
 * on chip (bit-identical to the two calls in sequence).  geometry: {length, width}, [2] when
 * shared_geometry != 0, else [B][2]; meas_cov: [6] or [B][6]; twist [T][B][6], pose [T][B][12],
 * null_pose [B][12], wrench [T][B][6] (the measurements); state [B][2] = (k, b) and covariance
 * [B][2][2] in place.  Errors as blf_rls_advance. */
blf_status blf_contact_rls_advance(blf_handle* handle, double lambda, const double* meas_cov,
                                   int32_t shared_cov, const double* geometry,
                                   int32_t shared_geometry, const double* twist, const double* pose,
                                   const double* null_pose, const double* wrench, int32_t steps,
                                   double* state, double* covariance, int64_t batch, void* stream);

/* ---- 11. Swing-foot and SO(3) trajectories (Planners::SwingFootPlanner, SO3Planner), batched ----
 * Both classes are absent from the reference snapshot (upstream added them later); this section
 * defines them.  Poses are {p[3], R[9] row-major}; twists and accelerations are mixed: [0..2] the
 * linear part of the frame origin in the world, [3..5] the angular part in the world.  No FMA
 * contraction; every sum below is evaluated left to right.
 *
 * blf_swing_foot_eval: L contact lists (one foot each) of up to C = params->max_contacts contacts,
 *   contact_pose [L][C][12], contact_time [L][C][2] = (activation, deactivation), ncontacts [L];
 *   each list sorted and non-overlapping (as ContactList guarantees); queries tq [L][Q].
 * Outputs, each optional (NULL: not written): pose [L][Q][12], twist [L][Q][6], accel [L][Q][6],
 *   contact_idx [L][Q], in_contact [L][Q] (int32).
 * For one list of n contacts (pose_c, act_c, deact_c) and one query time t:
 *   raw = the last c < n with act_c <= t, or -1 (the getPresentContact rule, ContactList.cpp:
 *   190-202); contact_idx = raw.
 *   raw == -1:                      pose of contact 0, zero twist / accel, in_contact = 0
 *   t < deact_raw (stance):         pose of contact raw bit for bit, zeros, in_contact = 1
 *   t >= deact_raw, raw == n - 1:   pose of the last contact, zeros, in_contact = 0
 *   otherwise: swing from contact raw to raw + 1, in_contact = 0, with t0 = deact_raw,
 *   t1 = act_{raw+1}, T = t1 - t0, tau = (t - t0) / T.
 *   A query is poisoned when n is outside [1, C], when t is not finite, or when any pose or time
 *   value of its list's contacts c < n is not finite: every floating output of the query is NaN,
 *   contact_idx = -1, in_contact = 0; other queries are unaffected.
 * Swing translation: the 3-knot quintic spline of section 4 (the expressions of blf_quintic_fit /
 *   _eval in their order), h = step_height, rho = apex_ratio, p_a = p_raw, p_b = p_{raw+1}:
 *     lift knot  t0:  position p_a, zero velocity and acceleration
 *     apex knot  tm = (1 - rho) * t0 + rho * t1:  xy position (1 - rho) * p_a + rho * p_b,
 *                z position max(z_a, z_b) + h, velocity ((p_b - p_a)_xy / T, 0), zero acceleration
 *     land knot  t1:  position p_b, velocity (0, 0, landing_velocity), acceleration
 *                (0, 0, landing_acceleration)
 *   evaluated on the segment of the last knot <= t (t < tm: the first) at t - (that knot's time).
 * Swing rotation: minimum jerk on the geodesic, R(t) = Exp(s phi) R_a, omega = sdot phi,
 *   alpha = sddot phi, phi = Log(R_b R_a^T) = theta u, with
 *     s = ((tau*tau)*tau) * (10 + tau*(-15 + 6*tau))
 *     sdot = ((tau*tau) * (30 + tau*(-60 + 30*tau))) / T
 *     sddot = (tau * (60 + tau*(-180 + 120*tau))) / (T*T)
 * Log: E = R_b R_a^T, E_ij = (b_i0 a_j0 + b_i1 a_j1) + b_i2 a_j2; tr = (E00 + E11) + E22; the
 *   (unnormalised) quaternion of E by Shepperd's rule, the branch being the largest of tr, E00, E11,
 *   E22 (the first of equals, in that order):
 *     tr:  g = 2 sqrt(1 + tr);                w = g/4, x = (E21-E12)/g, y = (E02-E20)/g, z = (E10-E01)/g
 *     E00: g = 2 sqrt(((1 + E00) - E11) - E22); w = (E21-E12)/g, x = g/4, y = (E01+E10)/g, z = (E02+E20)/g
 *     E11: g = 2 sqrt(((1 + E11) - E00) - E22); w = (E02-E20)/g, x = (E01+E10)/g, y = g/4, z = (E12+E21)/g
 *     E22: g = 2 sqrt(((1 + E22) - E00) - E11); w = (E10-E01)/g, x = (E02+E20)/g, y = (E12+E21)/g, z = g/4
 *   negated when w < 0; nv = sqrt((x*x + y*y) + z*z), theta = 2 atan2(nv, w), u = (x, y, z) / nv.
 *   nv == 0 is the only special case: phi = 0 and R(t) is R_a copied bit for bit.  There is no
 *   small-angle threshold (the quaternion route is well conditioned from 0 up to pi).  At exactly
 *   pi (w == 0) the sign of u, hence the side the rotation turns through, is whichever the branch
 *   gives: the end points are the same, the path between them is one of two.
 * Exp: a = s * theta, sa = sin(a), sh = sin(0.5 * a), cv = 2 * (sh * sh);
 *   M_ii = 1 + cv * (u_i*u_i - 1);  M_ij = sa * K_ij + cv * (u_i*u_j) for i != j, with
 *   K = [u]x (K01 = -u2, K02 = u1, K10 = u2, K12 = -u0, K20 = -u1, K21 = u0);
 *   R_ij = (M_i0 a_0j + M_i1 a_1j) + M_i2 a_2j;  omega_i = sdot * (theta * u_i), alpha likewise.
 * Errors: null handle, params, input pointer or no output at all, negative batch / nq, reserved
 * != 0, step_height negative or not finite, apex_ratio outside (0, 1), a landing term not finite:
 * BLF_ERR_INVALID_ARGUMENT; max_contacts outside [1, BLF_SWING_MAX_CONTACTS]: BLF_ERR_UNSUPPORTED;
 * batch == 0 or nq == 0: BLF_OK. */
#define BLF_SWING_MAX_CONTACTS 16
typedef struct blf_swing_foot_params {
    int32_t max_contacts;         /* C, 1..BLF_SWING_MAX_CONTACTS (padded contacts per list)   */
    int32_t reserved;             /* must be 0                                                 */
    double step_height;           /* h >= 0 above the higher of the two contacts [m]           */
    double apex_ratio;            /* rho in (0, 1): the apex time as a fraction of the swing   */
    double landing_velocity;      /* vertical velocity at touch-down [m/s]                     */
    double landing_acceleration;  /* vertical acceleration at touch-down [m/s^2]               */
} blf_swing_foot_params;
blf_status blf_swing_foot_eval(blf_handle* handle, const blf_swing_foot_params* params,
                               const double* contact_pose, const double* contact_time,
                               const int32_t* ncontacts, int64_t batch, const double* tq,
                               int32_t nq, double* pose, double* twist, double* accel,
                               int32_t* contact_idx, int32_t* in_contact, void* stream);

/* blf_so3_eval: S minimum-jerk rotation trajectories from R0 [S][9] to R1 [S][9] over duration [S],
 * queried at tq [S][Q], clamped to [0, duration]: tau = clamp(t) / duration, T = duration, R_a = R0,
 * R_b = R1 in the rotation rule above.  Outputs, each optional: rot [S][Q][9], omega [S][Q][3],
 * alpha [S][Q][3].  A duration that is not finite and positive, or a non-finite t, R0 or R1 value,
 * gives NaN in that query's outputs.  Errors as blf_swing_foot_eval. */
blf_status blf_so3_eval(blf_handle* handle, const double* R0, const double* R1,
                        const double* duration, int64_t batch, const double* tq, int32_t nq,
                        double* rot, double* omega, double* alpha, void* stream);

/* ---- 12. Whole-body inverse kinematics (IK::QPInverseKinematics with SE3Task, CoMTask and
 *          JointTrackingTask, integrated by ForwardEuler<FloatingBaseSystemKinematics>), batched ----
 * Upstream's QPInverseKinematics with every task at priority 1 (weighted): the unconstrained
 * least-squares problem of one robot is solved in closed form.  The unknown is nu = (base mixed
 * twist, s_dot) in R^(6+n); the kinematics are taken at state->base_pos, base_rot and joint_pos (the
 * velocity fields of `state` are not read by blf_fb_ik_solve).  With p_B the base position, z_j /
 * o_j joint j's world axis / origin and anc(l) the joints between the base and link l:
 *   point Jacobian of a point x of link l (6 x (6+n), rows linear xyz then angular xyz):
 *     base linear column a:   (e_a, 0);    base angular column a:  (e_a x (x - p_B), e_a);
 *     joint j in anc(l):      revolute (z_j x (x - o_j), z_j), prismatic (z_j, 0);  otherwise 0.
 *   SE3 task k on frame f_k with world pose (p, R): J_k = the point Jacobian at p;
 *     v*_k = (v_ff + kp_lin (p_des - p),  w_ff + kp_ang (theta u)),  theta u = Log(R_des R^T) by
 *     section 11's Log (no small-angle branch other than nv == 0).
 *   CoM task: c_l = p_l + R_l com_l, m = sum_l m_l, c = (sum_l m_l c_l) / m (links in index order);
 *     for joint j, m_sub = sum of m_l and h_sub = sum of m_l c_l over the links l with j in anc(l)
 *     (index order): column j = z_j x ((h_sub - m_sub o_j) / m) (revolute), z_j (m_sub / m)
 *     (prismatic); base columns (e_a, and e_a x (c - p_B));  v*_c = cdot_des + com_kp (c_des - c).
 *   Joint task: sdot*_j = sdot_des_j + joint_kp_j (s_des_j - s_j).
 *   With the task rows a_r (row r of the stacked J_k, then J_c), their weights w_r and targets t_r:
 *     H = sum_r w_r a_r^T a_r + diag(base_damping x 6, joint_weight),
 *     g = sum_r w_r a_r t_r + (0_6, joint_weight o sdot*),
 *   both accumulated over r in that order with fused multiply-adds (rows of zero weight are
 *   skipped), the diagonal term added last; H nu = g by the Cholesky factorization and the two
 *   substitutions of the floating-base dynamics' mass-matrix path.  Device results agree with a
 *   float64 restatement to rounding (tests/ik_reference.py, 1e-9 relative), not bit for bit.
 * Per-robot status (status [B], may be NULL) and failures, none of which reads out of bounds or
 * touches another robot:
 *   BLF_IK_BAD_INPUT     a frame index outside [0, model->nframes) (the indices are shared, so
 *                        then every robot), or a non-finite value among the robot's base_pos,
 *                        base_rot, joint_pos or set points: nu = NaN;
 *   BLF_IK_NOT_POSITIVE  a Cholesky pivot that is not a finite positive number: nu = NaN.
 *   An unknown joint_type makes every robot's nu NaN (status BLF_IK_NOT_POSITIVE).
 * blf_fb_ik_integrate: `steps` iterations in one launch with the set points held; each solves at
 *   the current state and takes blf_fbk_euler_integrate's single step of dT with that nu as input
 *   (p += v dT, R += dR dT with section 7's dR and model->rho, s += s_dot dT), in place on
 *   base_pos, base_rot and joint_pos; base_vel and joint_vel receive the last step's nu.  The
 *   result is bit for bit that of `steps` x { blf_fb_ik_solve; blf_fbk_euler_integrate(0, dT, dT) }.
 *   A robot whose step fails keeps the state before that step, skips its remaining steps, keeps
 *   that status (the first non-zero one) and gets a NaN nu.
 * Call-level errors: null handle, model, state, tasks or a required pointer, reserved != 0,
 * negative batch, steps < 1, dT not finite or not positive, a non-finite or negative weight, kp or
 * base_damping, a non-positive joint_weight: BLF_ERR_INVALID_ARGUMENT; nse3 outside
 * [0, BLF_IK_MAX_SE3_TASKS] or ndof outside [1, BLF_FBD_MAX_DOFS]: BLF_ERR_UNSUPPORTED;
 * batch == 0: BLF_OK.  The shared weight and gain arrays (se3_weight, se3_kp, com_weight,
 * joint_weight, joint_kp) are checked on the host through a staged copy: both calls copy them from
 * the device on `stream` and wait for that copy before they launch (so neither call can be
 * captured into a graph). */
#define BLF_IK_MAX_SE3_TASKS 4
#define BLF_IK_OK            0
#define BLF_IK_NOT_POSITIVE  1   /* a Cholesky pivot was not a finite positive number */
#define BLF_IK_BAD_INPUT     2   /* frame index out of range, or a non-finite state / set point of this robot */
typedef struct blf_ik_tasks {
    int32_t nse3;               /* K, 0..BLF_IK_MAX_SE3_TASKS                                   */
    int32_t reserved;           /* must be 0                                                    */
    const int32_t* frame;       /* [K] frame indices of the model                               */
    const double* se3_weight;   /* [K][6] row weights (linear xyz, angular xyz), finite, >= 0;
                                   a zero drops the row: linear zeros = SO3Task, angular zeros = R3Task */
    const double* se3_kp;       /* [K][2] (kp_linear, kp_angular)                               */
    const double* se3_pose;     /* [B][K][12] desired (p, R row-major): blf_swing_foot_eval's
                                   pose output for L = B*K lists, Q = 1, as it stands           */
    const double* se3_twist;    /* [B][K][6] feed-forward mixed twist, or NULL (zero)            */
    const double* com_weight;   /* [3] or NULL: no CoM task                                     */
    double com_kp;
    const double* com_pos;      /* [B][3]; required iff com_weight                              */
    const double* com_vel;      /* [B][3] or NULL (zero)                                        */
    const double* joint_weight; /* [n], finite, > 0 (JointTrackingTask: the regulariser)        */
    const double* joint_kp;     /* [n]                                                          */
    const double* joint_pos;    /* [B][n] desired joint positions                               */
    const double* joint_vel;    /* [B][n] or NULL (zero)                                        */
    double base_damping;        /* finite, >= 0: added to the six base diagonal entries of H    */
} blf_ik_tasks;

blf_status blf_fb_ik_solve(blf_handle* handle, const blf_fb_model* model, const blf_fb_state* state,
                           const blf_ik_tasks* tasks, int64_t batch, double* nu /* [B][6+n] */,
                           int32_t* status /* [B] or NULL */, void* stream);

blf_status blf_fb_ik_integrate(blf_handle* handle, const blf_fb_model* model,
                               const blf_fb_state* state /* in place */, const blf_ik_tasks* tasks,
                               int64_t batch, int32_t steps, double dT,
                               double* nu /* [B][6+n], the last step's, or NULL */,
                               int32_t* status /* [B] or NULL: the first non-zero of the steps */,
                               void* stream);

/* ---- 12b. Hard (priority-0) tasks: task rows held as exact equality constraints ----
 * Section 12 defines the task rows a_r, their weights w_r and their targets t_r.  A 27-bit mask
 * `rows` marks some of them hard: bit 6k + a marks row a of SE3 task k (linear xyz, angular xyz),
 * bits 24 to 26 mark the CoM rows.  With A_h and b_h the hard rows and their targets, in row order,
 * m_h <= 27, the solve is
 *   minimise   1/2 sum_soft w_r (a_r nu - t_r)^2 + joint-tracking and base-damping terms of section 12
 *   subject to A_h nu = b_h,
 * computed as follows:
 *   1. H and g are assembled exactly as section 12 assembles them: hard rows are included with their
 *      weights, in the same order and with the same fmas.  A hard row's weight only conditions H; in
 *      exact arithmetic the result does not depend on it.
 *   2. H = L L^T with section 12's factorization;  z = L^-1 g;  Y = L^-1 A_h^T.
 *   3. S = Y^T Y (m_h x m_h) is factorized by Cholesky with a relative pivot rule: pivot i must
 *      satisfy d_i > tau * S_ii, S_ii the entry before elimination (and be finite); tau = 1e-8 by
 *      default.
 *   4. lambda = S^-1 (Y^T z - b_h)  and  nu = L^-T (z - Y lambda).
 * Every hard row also enters H, so H is positive definite whenever the constrained problem is well
 * posed, even with base_damping = 0 and the base held only by hard feet.
 * Per-robot status: section 12's, and BLF_IK_HARD_DEPENDENT when a pivot of S fails the rule (the
 * hard rows are linearly dependent, conflicting, or more than 6 + n): nu = NaN, other robots are
 * untouched.  When several apply: BLF_IK_BAD_INPUT, then BLF_IK_NOT_POSITIVE, then
 * BLF_IK_HARD_DEPENDENT.  blf_fb_ik_integrate_hard treats it like any failed step (section 12), and
 * is bit for bit `steps` x { blf_fb_ik_solve_hard; blf_fbk_euler_integrate(0, dT, dT) }.
 * hard == NULL or rows == 0: exactly blf_fb_ik_solve / blf_fb_ik_integrate, bit for bit.
 * Call-level errors: section 12's, and BLF_ERR_INVALID_ARGUMENT for a bit that names an SE3 task
 * >= nse3, a CoM bit without com_weight, a hard row whose weight is 0 (checked with the staged
 * weights, so only when batch > 0), bits above 26, reserved != 0, or a rel_pivot_min that is not
 * finite or outside [0, 1). */
#define BLF_IK_HARD_DEPENDENT 3   /* a pivot of S failed the rule: dependent / conflicting / too many hard rows */
typedef struct blf_ik_hard {
    uint32_t rows;          /* bit 6k+a: row a of SE3 task k; bits 24..26: CoM x, y, z */
    int32_t  reserved;      /* must be 0 */
    double   rel_pivot_min; /* tau; 0 selects the default 1e-8; finite, in [0, 1) */
} blf_ik_hard;

blf_status blf_fb_ik_solve_hard(blf_handle* handle, const blf_fb_model* model, const blf_fb_state* state,
                                const blf_ik_tasks* tasks, const blf_ik_hard* hard /* or NULL */,
                                int64_t batch, double* nu /* [B][6+n] */,
                                int32_t* status /* [B] or NULL */, void* stream);

blf_status blf_fb_ik_integrate_hard(blf_handle* handle, const blf_fb_model* model,
                                    const blf_fb_state* state /* in place */, const blf_ik_tasks* tasks,
                                    const blf_ik_hard* hard /* or NULL */, int64_t batch, int32_t steps,
                                    double dT, double* nu /* [B][6+n], the last step's, or NULL */,
                                    int32_t* status /* [B] or NULL */, void* stream);

/* ---- 12c. Joint position and velocity limits: a box on the joint velocities (IK::JointLimitsTask) ----
 * Sections 12 and 12b define H, g, the hard rows A_h, b_h and nu = (base twist, s_dot).  Every joint
 * j gets a box on its velocity, evaluated at the state of the solve (so in the fused loop it moves
 * with every step):
 *   lo_p = klim_j (pos_lower_j - s_j) / sampling_time      up_p = klim_j (pos_upper_j - s_j) / sampling_time
 *   lo_j = clamp(lo_p, -vel_max_j, +vel_max_j)             up_j = clamp(up_p, -vel_max_j, +vel_max_j)
 * (clamp(x, a, b) = min(max(x, a), b), evaluated in this order without fused multiply-adds): upstream's
 * JointLimitsTask (klim, sampling_time) intersected with a velocity limit.  -inf / +inf in pos_lower /
 * pos_upper and vel_max == NULL switch a side off.  pos_lower <= pos_upper, so lo <= up always, and a
 * joint outside its range gets a box that drives it back.  The solve is
 *   minimise section 12b's objective  subject to  A_h nu = b_h  and  lo <= s_dot <= up
 * (the base twist has no bound).  H is positive definite, so where a solution exists it is unique.
 * Method: a primal-dual active-set iteration on a working set W of joints held at a bound.
 *   1. W starts empty (at every step of the fused loop).
 *   2. An iteration solves the equality problem s_dot_j = bound_j (j in W), A_h nu = b_h: the held
 *      joints are eliminated from H, g and the hard rows (their columns move to the right-hand sides),
 *      then section 12b's steps 2-4 run on what is left.  An empty W is exactly section 12b's solve.
 *   3. rho = g_soft - H_soft nu - A_h^T lambda (zero on free columns).
 *   4. Infeasibilities: a free joint with nu_j < lo_j or nu_j > up_j (strict), a held joint whose rho
 *      points into the box (rho_j > 0 at a lower bound, rho_j < 0 at an upper bound).
 *   5. None: the robot is done, BLF_IK_OK.
 *   6. Block mode (the start): every violated joint is fixed at the bound it violates and every
 *      wrong-signed joint is released, at once.
 *   7. Block mode ends for good when the count of infeasibilities has not reached a new minimum in 8
 *      iterations in a row (that iteration already changes one joint), or when a block update made a
 *      pivot of S fail section 12b's rule: W goes back to the set before that update, and the next
 *      iteration solves it again.
 *   8. Outside block mode one joint changes per iteration: the most violated free joint (the lowest
 *      index among equals) is fixed, or, when none is violated, the lowest-index wrong-signed joint
 *      is released.
 *   9. A pivot of S that fails with W not empty outside block mode, or infeasibilities left after
 *      max_iter iterations (solves), give the per-robot status BLF_IK_LIMITS_UNRESOLVED and a NaN nu:
 *      the limits and the hard rows conflict, or the rule did not find the set.  The method is not a
 *      complete QP solver at the edge of feasibility: on 368 random instances 310 resolved, 53 ended
 *      here and were infeasible, 5 ended here although barely feasible.
 *  10. Status precedence: section 12b's (a pivot of S failing with W empty is BLF_IK_HARD_DEPENDENT),
 *      then BLF_IK_LIMITS_UNRESOLVED.
 * Results agree with tests/ik_limits_reference.py to rounding (1e-9 relative) and in iters / active
 * wherever no comparison of the rule is within rounding of a tie.
 * iters [B] (or NULL): the number of iterations (solves); 0 for a BLF_IK_BAD_INPUT robot.  active
 * [B][2] (or NULL): word 0 has bit j set when joint j ends on its lower bound, word 1 the same for
 * the upper bound; both 0 unless the status is BLF_IK_OK.  blf_fb_ik_integrate_limits: iters is the
 * sum over the steps the robot ran, active the last step's masks, and the call is bit for bit
 * `steps` x { blf_fb_ik_solve_limits; blf_fbk_euler_integrate(0, dT, dT) }.
 * limits == NULL: exactly blf_fb_ik_solve_hard / blf_fb_ik_integrate_hard, bit for bit, through the
 * same kernels (iters and active are then not written).  hard may be NULL (no hard rows).
 * The limit arrays are device memory shared by the batch, staged and checked on the host like
 * section 12's weights.  Call-level errors: section 12b's, and BLF_ERR_INVALID_ARGUMENT for
 * reserved != 0, a sampling_time that is not finite and positive, klim outside (0, 1], vel_max <= 0,
 * pos_lower > pos_upper, a NaN anywhere, a +inf pos_lower or -inf pos_upper, a null pos_lower,
 * pos_upper or klim, or max_iter < 0.  batch == 0: BLF_OK. */
#define BLF_IK_LIMITS_UNRESOLVED 4   /* the active-set iteration ended without a feasible optimal set */
#define BLF_IK_LIMITS_DEFAULT_MAX_ITER 32
typedef struct blf_ik_limits {
    const double* pos_lower;   /* [n] shared by the batch; -inf allowed */
    const double* pos_upper;   /* [n]; +inf allowed; pos_lower <= pos_upper */
    const double* klim;        /* [n] in (0, 1] */
    const double* vel_max;     /* [n] > 0, or NULL */
    double  sampling_time;     /* finite, > 0 */
    int32_t max_iter;          /* 0 selects the default */
    int32_t reserved;          /* must be 0 */
} blf_ik_limits;

blf_status blf_fb_ik_solve_limits(blf_handle* handle, const blf_fb_model* model, const blf_fb_state* state,
                                  const blf_ik_tasks* tasks, const blf_ik_hard* hard /* or NULL */,
                                  const blf_ik_limits* limits /* or NULL */, int64_t batch,
                                  double* nu /* [B][6+n] */, int32_t* status /* [B] or NULL */,
                                  int32_t* iters /* [B] or NULL */, uint64_t* active /* [B][2] or NULL */,
                                  void* stream);

blf_status blf_fb_ik_integrate_limits(blf_handle* handle, const blf_fb_model* model,
                                      const blf_fb_state* state /* in place */, const blf_ik_tasks* tasks,
                                      const blf_ik_hard* hard /* or NULL */,
                                      const blf_ik_limits* limits /* or NULL */, int64_t batch, int32_t steps,
                                      double dT, double* nu /* [B][6+n], the last step's, or NULL */,
                                      int32_t* status /* [B] or NULL */, int32_t* iters /* [B] or NULL */,
                                      uint64_t* active /* [B][2] or NULL */, void* stream);

/* ---- 12d. Reference tracking: per-step set points and a per-robot, per-step contact schedule ----
 * blf_fb_ik_track is blf_fb_ik_integrate_limits with the set points and the hard mask indexed by the
 * step: T steps in one launch, robot b following its own references with its own feet planted.  The
 * schedule's arrays are blf_swing_foot_eval's outputs for L = B*K lists (list b*K + k is SE3 task k of
 * robot b) and Q = T query times, as they stand.
 *   Per-step solve.  Step t = 0 .. T-1 of robot b runs section 12c's solve at the robot's current state
 *     with the set points of index t, then takes blf_fbk_euler_integrate's single step of dT.
 *   Set points.  tasks->se3_pose, se3_twist, com_pos and com_vel are not read and may be NULL; the
 *     joint task's joint_pos / joint_vel stay [B][n] and are held over the call.  Every shared array
 *     (weights, gains, frames, limits) is used as in section 12.
 *   Hard rows.  rows(b,t) = hard->rows | union over k of (contact[b][k][t] != 0 ? stance_rows &
 *     (0x3F << 6k) : 0).  "At most 6 + n hard rows" applies to each robot's own rows(b,t); a
 *     violation, like any failed pivot of S with W empty, is BLF_IK_HARD_DEPENDENT for that robot only.
 *     A hard row's weight only conditions H (section 12b).  tau is hard->rel_pivot_min, or the default
 *     when hard is NULL.
 *   Trajectories (each may be NULL) are step-major: slice t holds the state, or nu, after step t for the
 *     whole batch, so slice t of joint_traj is directly a blf_joint_impedance q_ref.
 *   Final state.  `state` ends at the state after the last completed step; base_vel and joint_vel
 *     receive the last nu (NaN for a failed robot, as in section 12).
 *   Failed robots.  A robot whose step fails keeps the state before that step (section 12); its status
 *     is the first non-zero one, fail_step [B] (or NULL) that step and -1 for a robot that did not
 *     fail; its trajectory entries from that step on are NaN; it reads no later set point.  A
 *     non-finite set point of step t makes the robot BLF_IK_BAD_INPUT at step t, not before (a
 *     non-finite joint set point or a bad frame index: at step 0).
 *   iters is summed over the steps the robot ran, active is the last step's (section 12c).
 *   limits == NULL: no box; every step is then section 12b's solve (to rounding, not bit for bit: the
 *     call still runs section 12c's iteration, which ends after its first solve; iters counts it).
 * Three equalities:
 *   P1  a T-step call equals, bit for bit, T one-step calls with the schedule's slices (for robots that
 *       do not fail: a one-step call starts every robot afresh);
 *   P2  when every robot has the same rows(.,t) at every step and limits != NULL, the call equals, bit
 *       for bit, T x blf_fb_ik_integrate_limits(steps = 1) with that mask and step t's set points;
 *   P3  a robot's result does not depend on which robot shares its wavefront: a row its neighbour
 *       holds hard and it does not enters its solve as a null row (zero in Y, e_i in S, zero right-hand
 *       side), which contributes exact zeros, so the equality is bit for bit.
 * Call-level errors: section 12c's, and BLF_ERR_INVALID_ARGUMENT for a null schedule, steps < 1, a
 * reserved field != 0, a stance_rows bit outside the SE3 tasks present, a row of hard->rows |
 * stance_rows whose weight is 0 (checked with the staged weights, so only when batch > 0), or a
 * missing required pointer (se3_pose when nse3 > 0, com_pos iff com_weight, state->base_vel /
 * joint_vel).  batch == 0: BLF_OK.  A refused call leaves every output untouched. */
typedef struct blf_ik_schedule {
    int32_t  steps;          /* T >= 1 */
    int32_t  reserved;       /* must be 0 */
    uint32_t stance_rows;    /* section 12b's bit layout, SE3 bits only (bits 0..6*nse3-1): the rows of
                                task k that are hard at a step where contact[b][k][t] != 0 */
    uint32_t reserved2;      /* must be 0 */
    const int32_t* contact;  /* [B][K][T] or NULL (never in contact): blf_swing_foot_eval's in_contact
                                for L = B*K lists, Q = T, as it stands */
    const double* se3_pose;  /* [B][K][T][12]: blf_swing_foot_eval's pose output as it stands */
    const double* se3_twist; /* [B][K][T][6] or NULL (zero): its twist output as it stands */
    const double* com_pos;   /* [B][T][3]; required iff tasks->com_weight */
    const double* com_vel;   /* [B][T][3] or NULL */
} blf_ik_schedule;

blf_status blf_fb_ik_track(blf_handle* handle, const blf_fb_model* model,
                           const blf_fb_state* state /* in place */, const blf_ik_tasks* tasks,
                           const blf_ik_hard* hard /* or NULL */, const blf_ik_limits* limits /* or NULL: no box */,
                           const blf_ik_schedule* schedule, int64_t batch, double dT,
                           double* joint_traj /* [T][B][n] or NULL */,
                           double* base_traj /* [T][B][12] (p, R) or NULL */,
                           double* nu_traj /* [T][B][6+n] or NULL */, int32_t* status /* [B] or NULL */,
                           int32_t* fail_step /* [B] or NULL */, int32_t* iters /* [B] or NULL */,
                           uint64_t* active /* [B][2] or NULL */, void* stream);

/* ---- 13. Contact detection and legged odometry (Contacts::SchmittTriggerDetector,
 *          Estimators::LeggedOdometry), batched ---------------------------------------------------
 * Both classes are absent from the reference snapshot (upstream added them later); this section
 * defines them.  Everything is fp64 with no FMA contraction.
 *
 * The trigger.  A trigger has parameters (on_threshold, off_threshold, switch_on_after,
 * switch_off_after), a state word (bit 0: the contact state, bit 1: an edge is pending; the other
 * bits are dropped by the first finite sample) and two timers (edge_time, switch_time).  One sample
 * (t, v), each test one subtraction and one comparison:
 *   if v or t is not finite: the state and the timers are left as they are; otherwise
 *   state off:  cross = v >= on_threshold,   after = switch_on_after
 *   state on:   cross = v <= off_threshold,  after = switch_off_after
 *   if cross and no edge is pending: pending, edge_time = t;  if not cross: not pending
 *   if pending and (t - edge_time) >= after: the state flips, switch_time = t, not pending
 * (so a delay of 0 switches on the sample that crosses, and a sample back inside the band clears a
 * pending edge: chatter shorter than the delay never switches).
 *
 * blf_schmitt_trigger_advance: B x K independent triggers over T samples, samples STEP-MAJOR as in
 * section 10.  params: HOST memory (read and validated during the call, never by the device), [4]
 * when shared_params != 0, else [K][4].  time [T] (one clock for the batch), value [T][B][K]; state
 * [B][K] int32 and timers [B][K][2] = (edge_time, switch_time) are updated in place; state_out
 * [T][B][K] int32 or NULL: bit 0 after each sample.  Every other pointer is device memory.
 * Errors: null handle, params or time, another null pointer with batch > 0 (state_out excepted),
 * steps < 1, batch < 0, a threshold or delay
 * that is not finite, a negative delay, on_threshold < off_threshold: BLF_ERR_INVALID_ARGUMENT;
 * ncontacts outside [1, BLF_ODOM_MAX_CONTACTS]: BLF_ERR_UNSUPPORTED (checked before the parameter
 * values); batch == 0: BLF_OK.                                                                    */
#define BLF_ODOM_MAX_CONTACTS 8
blf_status blf_schmitt_trigger_advance(blf_handle* handle, int32_t ncontacts, const double* params,
                                       int32_t shared_params, const double* time, const double* value,
                                       int32_t steps, int32_t* state, double* timers, int32_t* state_out,
                                       int64_t batch, void* stream);

/* blf_legged_odometry_advance: T steps of B estimators of the base pose and twist from the joint
 * kinematics and a frame held fixed in the world, in ONE launch on `stream` (no staged copy, no
 * host synchronisation: the call can be captured into a graph).
 * fb_model: the robot (gravity, masses and inertias are not read; the arrays must still be there).
 * frames [K]: the model's frame index of contact slot c.  params / shared_params / time: as above.  joint_pos
 * [T][B][n], joint_vel [T][B][n] or NULL (zero), normal_force [T][B][K].
 * Estimator state, in place: trig_state [B][K], trig_timers [B][K][2] (the K triggers), fixed_frame
 * [B] int32 (a SLOT in [0, K)), fixed_pose [B][12] = (p, R row-major): the world transform at which
 * that slot's frame is held.  To start from a known base pose, fixed_pose is blf_fb_frame_state's
 * `pose` of that frame at the known state, the trigger state and timers zero (or bit 0 set for the
 * feet on the ground).
 * Outputs, step-major, each may be NULL but not all: base_pos [T][B][3], base_rot [T][B][9],
 * base_vel [T][B][6] (mixed: blf_fb_state.base_vel's layout), contact_out [T][B][K] int32,
 * fixed_out [T][B] int32 (the fixed slot after the step), status [B] int32.
 * One step t of robot b:
 *   1. the K triggers take (time[t], normal_force[t][b][c]) exactly as above: contact_out is
 *      bit-identical to blf_schmitt_trigger_advance's state_out on the same samples
 *   2. the forward kinematics of section 8 at joint_pos[t], joint_vel[t] with the base at the
 *      identity and at rest: (p_c, R_c) the pose and (v_c, w_c) the mixed velocity of slot c's frame
 *      relative to the base, in base coordinates
 *   3. with f = fixed_frame and (P, Q) = fixed_pose:   R_B = Q R_f^T,   p_B = P - R_B p_f
 *   4. the switch: f stays while slot f's state is on; otherwise f' = the slot whose state is on
 *      with the greatest switch_time (the lowest slot among equals); if no slot is on, f stays (the
 *      estimate dead-reckons on the last foot; an all-zero contact_out row reports it).  On a change
 *      fixed_pose <- (p_B + R_B p_f', R_B R_f'), fixed_frame <- f'; the step's base pose is not
 *      changed by the switch
 *   5. the base twist that holds the (new) fixed frame at rest, in closed form:
 *      w_B = -R_B w_f,   v_B = -R_B v_f - w_B x (R_B p_f)
 * Rotations are composed and never re-orthonormalised (as ForwardEuler leaves base_rot): over a long
 * walk fixed_pose's rotation drifts from SO(3) at rounding level per switch.
 * A robot with a non-finite joint_pos, joint_vel or fixed_pose at some step, with fixed_frame
 * outside [0, K), or whose kinematics are not finite (an unknown joint_type: NaN as in section 8)
 * gets status BLF_IK_BAD_INPUT, NaN in base_pos / base_rot / base_vel from that step on and in
 * fixed_pose, fixed_out = -1 from that step on, and keeps its fixed_frame; its triggers run on
 * (contact_out, trig_state, trig_timers depend on the forces and times only).  A frames[c] outside
 * [0, fb_model->nframes) gives every robot that treatment (never a read past the model).  No other
 * robot is touched.  status is BLF_IK_OK otherwise.
 * Errors: null handle, model, model array, frames, params or time, another required pointer null or
 * no output requested with batch > 0, reserved != 0, steps < 1, batch < 0, a bad trigger parameter
 * (above): BLF_ERR_INVALID_ARGUMENT; ndof outside
 * [1, BLF_FBD_MAX_DOFS] or ncontacts outside [1, BLF_ODOM_MAX_CONTACTS]: BLF_ERR_UNSUPPORTED;
 * batch == 0: BLF_OK.                                                                             */
blf_status blf_legged_odometry_advance(blf_handle* handle, const blf_fb_model* fb_model, int32_t ncontacts,
                                       const int32_t* frames, const double* params, int32_t shared_params,
                                       const double* time, const double* joint_pos, const double* joint_vel,
                                       const double* normal_force, int32_t steps, int32_t* trig_state,
                                       double* trig_timers, int32_t* fixed_frame, double* fixed_pose,
                                       double* base_pos, double* base_rot, double* base_vel,
                                       int32_t* contact_out, int32_t* fixed_out, int32_t* status, int64_t batch,
                                       int32_t reserved, void* stream);

/* Algorithmic flop count of one IPM iteration of one problem (what the fp64 roofline field
 * of bench.py is computed from); `active_facets` = sum_k nfacets[k]. */
double blf_dcm_mpc_flops_per_iter(int32_t horizon, int64_t active_facets);

#ifdef __cplusplus
}
#endif

#endif /* BLF_C_H */
