// blf_capi.hip — the extern "C" boundary declared in include/blf/blf_c.h: argument validation,
// the reference's error semantics, and dispatch to the kernels' launchers.
#include <algorithm>
#include <cmath>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <type_traits>

#include "blf_internal.h"

namespace blf {

static thread_local char g_err[512] = "no error";

QpLaunchMode& qp_launch_mode()
{
    static QpLaunchMode mode{{[] {
                                 const char* fz = getenv("BLF_QP_FUSE_STAGE2");
                                 return !(fz && fz[0] == '0') ? 1 : 0;
                             }()},
                             {[] {
                                 const char* sk = getenv("BLF_QP_SINGLE_KERNEL");
                                 return (sk && sk[0] == '1') ? 1 : 0;
                             }()},
                             [] {
                                 const char* lg = getenv("BLF_QP_LIST_GRID");
                                 const int v = lg ? atoi(lg) : 0;
                                 return v > 0 ? v : kListGrid;
                             }()};
    return mode;
}

blf_status set_error(blf_status code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

blf_status check_hip(hipError_t e, const char* what)
{
    if (e == hipSuccess) return BLF_OK;
    return set_error(BLF_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
}

Handle::~Handle()
{
    for (auto& kv : lists) (void)hipFree(kv.second.buf);   // (hipFree waits for the device)
}

blf_status Handle::stage2_list(hipStream_t s, int64_t batch, Stage2List* out)
{
    // the list's slot toggles on the host between solves and may need a stream synchronisation to
    // grow: a captured graph would freeze one toggle and fail the synchronisation, so a solve under
    // stream capture is refused (the solve itself is capture-safe; its bookkeeping is not)
    hipStreamCaptureStatus cap_st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cap_st) == hipSuccess && cap_st != hipStreamCaptureStatusNone)
        return set_error(BLF_ERR_UNSUPPORTED, "DCM-MPC solve under stream capture (the stage-2 list is host-sequenced)");
    std::lock_guard<std::mutex> lock(mu);
    List& l = lists[s];
    if (l.cap < batch) {
        // the old list may still be read by the stream's last solve: let it finish first
        blf_status st = check_hip(hipStreamSynchronize(s), "stage-2 list: hipStreamSynchronize");
        if (st != BLF_OK) return st;
        if (l.buf) (void)hipFree(l.buf);
        l.buf = nullptr;
        l.cap = 0;
        const int64_t cap = std::max<int64_t>(batch, 4096);
        st = check_hip(hipMalloc(&l.buf, sizeof(int32_t) * (size_t)(cap + 2)), "stage-2 list: hipMalloc");
        if (st != BLF_OK) return st;
        st = check_hip(hipMemset(l.buf, 0, sizeof(int32_t) * 2), "stage-2 list: hipMemset");
        if (st != BLF_OK) {
            (void)hipFree(l.buf);
            l.buf = nullptr;
            return st;
        }
        l.cap = cap;
        l.slot = 0;
    }
    *out = Stage2List{l.buf, &l.slot, l.cap};
    return BLF_OK;
}

}  // namespace blf

using namespace blf;

struct blf_handle {
    Handle h;
};

#define BLF_REQUIRE(cond, ...)                                                             \
    do {                                                                                   \
        if (!(cond)) return set_error(BLF_ERR_INVALID_ARGUMENT, __VA_ARGS__);              \
    } while (0)

// FixedStepIntegrator::integrate's step schedule (FixedStepIntegrator.tpp:21-72): validation in
// the reference's order, iterations = ceil((T - t0) / dT); steps 0..iterations-2 advance by dT and
// the last one by T - currentTime with the stale currentTime = t0 + dT (iterations - 2) (:48-64).
static blf_status step_schedule(double initial_time, double final_time, double dT,
                                int* iterations_out, double* dT_last_out)
{
    if (initial_time > final_time)                                                      // :26-30
        return set_error(BLF_ERR_TIME_INTERVAL,
                         "[FixedStepIntegrator::integrate] The final time has to be greater than "
                         "the initial one.");
    if (!(dT > 0))                                                                      // :40-46
        return set_error(BLF_ERR_TIME_INTERVAL,
                         "[FixedStepIntegrator::integrate] The sampling time must be a strictly "
                         "positive number.");
    if (initial_time == final_time)
        return set_error(BLF_ERR_EMPTY_INTERVAL,
                         "integrate(t, t): the reference loops forever here "
                         "(FixedStepIntegrator.tpp:51, size_t i < -1); refused");
    const double q = ceil((final_time - initial_time) / dT);                            // :48
    if (!(q < 2.0e9)) return set_error(BLF_ERR_UNSUPPORTED, "too many integration steps");
    const int iterations = (int)q;
    double currentTime = initial_time;
    if (iterations >= 2) currentTime = initial_time + dT * (double)(iterations - 2);   // :53
    *iterations_out = iterations;
    *dT_last_out = final_time - currentTime;                                            // :64
    return BLF_OK;
}

// The schedule, then launch(iterations, dT_last): the end of every integrate call
template <class Launch>
static blf_status scheduled(double initial_time, double final_time, double dT, Launch launch)
{
    int iterations = 0;
    double dT_last = 0.0;
    const blf_status st = step_schedule(initial_time, final_time, dT, &iterations, &dT_last);
    return st != BLF_OK ? st : launch(iterations, dT_last);
}

extern "C" {

blf_status blf_create(blf_handle** handle, int32_t device)
{
    BLF_REQUIRE(handle != nullptr, "blf_create: null handle pointer");
    int count = 0;
    blf_status st = check_hip(hipGetDeviceCount(&count), "hipGetDeviceCount");
    if (st != BLF_OK) return st;
    if (device < 0 || device >= count)
        return set_error(BLF_ERR_HIP, "blf_create: device %d not present (%d devices)", device, count);
    st = check_hip(hipSetDevice(device), "hipSetDevice");
    if (st != BLF_OK) return st;
    blf_handle* h = new blf_handle;
    h->h.device = device;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) h->h.num_cus = prop.multiProcessorCount;
    *handle = h;
    return BLF_OK;
}

blf_status blf_destroy(blf_handle* handle)
{
    delete handle;
    return BLF_OK;
}

const char* blf_last_error(void) { return g_err; }

blf_status blf_step_schedule(double initial_time, double final_time, double dT, int32_t* iterations,
                             double* dT_last, double* t_last)
{
    BLF_REQUIRE(iterations && dT_last && t_last, "blf_step_schedule: null output");
    int it = 0;
    double last = 0.0;
    const blf_status st = step_schedule(initial_time, final_time, dT, &it, &last);
    if (st != BLF_OK) return st;
    *iterations = it;
    *dT_last = last;
    *t_last = it >= 2 ? initial_time + dT * (double)(it - 2) : initial_time;   // :53, as step_schedule
    return BLF_OK;
}

#ifndef BLF_SRC_HASH
#define BLF_SRC_HASH "unknown"
#endif
// The sources' hash (Makefile SRC_HASH) makes the loaded library traceable to the tree it was
// built from (blf/native.py build_provenance).
const char* blf_version(void) { return "blf-mi355x 0.3.0 (abi 3, gfx950, fp64, -ffp-contract=off) src " BLF_SRC_HASH; }


blf_status blf_set_qp_launch_mode(int32_t fuse_stage2, int32_t single_kernel)
{
    BLF_REQUIRE(fuse_stage2 >= -1 && fuse_stage2 <= 1 && single_kernel >= -1 && single_kernel <= 1,
                "blf_set_qp_launch_mode: settings are -1, 0 or 1");
    QpLaunchMode& m = qp_launch_mode();
    if (fuse_stage2 >= 0) m.fuse_stage2.store(fuse_stage2, std::memory_order_relaxed);
    if (single_kernel >= 0) m.single_kernel.store(single_kernel, std::memory_order_relaxed);
    return BLF_OK;
}

blf_status blf_lti_euler_integrate(blf_handle* handle, int32_t n, int32_t m, const double* A,
                                   const double* Bm, int32_t shared_matrices, const double* u,
                                   double* x, int64_t batch, double initial_time,
                                   double final_time, double dT, void* stream)
{
    BLF_REQUIRE(handle != nullptr, "blf_lti_euler_integrate: null handle");
    BLF_REQUIRE(n >= 1 && m >= 1, "blf_lti_euler_integrate: n=%d m=%d, both must be >= 1", n, m);
    BLF_REQUIRE(batch >= 0, "blf_lti_euler_integrate: negative batch");
    BLF_REQUIRE(batch == 0 || (A && Bm && u && x), "blf_lti_euler_integrate: null buffer");
    return scheduled(initial_time, final_time, dT, [&](int iterations, double dT_last) {
        return launch_lti_euler(n, m, A, Bm, shared_matrices, u, x, batch, iterations, dT, dT_last,
                                (hipStream_t)stream);
    });
}

blf_status blf_lti_dynamics(blf_handle* handle, int32_t n, int32_t m, const double* A,
                            const double* Bm, int32_t shared_matrices, const double* u,
                            const double* x, double* dx, int64_t batch, void* stream)
{
    BLF_REQUIRE(handle != nullptr, "blf_lti_dynamics: null handle");
    BLF_REQUIRE(n >= 1 && m >= 1, "blf_lti_dynamics: n=%d m=%d, both must be >= 1", n, m);
    BLF_REQUIRE(batch >= 0, "blf_lti_dynamics: negative batch");
    BLF_REQUIRE(batch == 0 || (A && Bm && u && x && dx), "blf_lti_dynamics: null buffer");
    return launch_lti_dynamics(n, m, A, Bm, shared_matrices, u, x, dx, batch, (hipStream_t)stream);
}

blf_status blf_dcm_euler_rollout(blf_handle* handle, const double* xi0, const double* omega,
                                 const double* vrp, int32_t horizon, double dt, double* xi_out,
                                 int64_t batch, void* stream)
{
    BLF_REQUIRE(handle != nullptr, "blf_dcm_euler_rollout: null handle");
    BLF_REQUIRE(horizon >= 1, "blf_dcm_euler_rollout: horizon %d < 1", horizon);
    BLF_REQUIRE(batch >= 0, "blf_dcm_euler_rollout: negative batch");
    BLF_REQUIRE(batch == 0 || (xi0 && omega && vrp && xi_out), "blf_dcm_euler_rollout: null buffer");
    return launch_dcm_rollout(xi0, omega, vrp, horizon, dt, xi_out, batch, (hipStream_t)stream);
}

blf_status blf_hull2d_hrep(blf_handle* handle, const double* pts, const int32_t* npts,
                           int32_t max_points, int32_t max_facets, int64_t batch, double* A,
                           double* b, int32_t* nfacets, void* stream)
{
    BLF_REQUIRE(handle != nullptr, "blf_hull2d_hrep: null handle");
    BLF_REQUIRE(max_points >= 1 && max_points <= BLF_HULL_MAX_POINTS,
                "blf_hull2d_hrep: max_points %d outside [1, %d]", max_points, BLF_HULL_MAX_POINTS);
    BLF_REQUIRE(max_facets >= 1 && max_facets <= 2 * BLF_HULL_MAX_POINTS,
                "blf_hull2d_hrep: max_facets %d", max_facets);
    BLF_REQUIRE(batch >= 0, "blf_hull2d_hrep: negative batch");
    BLF_REQUIRE(batch == 0 || (pts && npts && A && b && nfacets), "blf_hull2d_hrep: null buffer");
    return launch_hull2d(pts, npts, max_points, max_facets, batch, A, b, nfacets,
                         (hipStream_t)stream);
}

blf_status blf_hull2d_contains(blf_handle* handle, const double* A, const double* b,
                               const int32_t* nfacets, int32_t max_facets, const double* query,
                               int64_t batch, int32_t* inside, void* stream)
{
    BLF_REQUIRE(handle != nullptr, "blf_hull2d_contains: null handle");
    BLF_REQUIRE(max_facets >= 1, "blf_hull2d_contains: max_facets %d", max_facets);
    BLF_REQUIRE(batch >= 0, "blf_hull2d_contains: negative batch");
    BLF_REQUIRE(batch == 0 || (A && b && nfacets && query && inside),
                "blf_hull2d_contains: null buffer");
    return launch_hull2d_contains(A, b, nfacets, max_facets, query, batch, inside,
                                  (hipStream_t)stream);
}

blf_status blf_hull3d_hrep(blf_handle* handle, const double* pts, const int32_t* npts,
                           int32_t max_points, int32_t max_facets, int64_t batch, double* A,
                           double* b, int32_t* nfacets, void* stream)
{
    BLF_REQUIRE(handle != nullptr, "blf_hull3d_hrep: null handle");
    BLF_REQUIRE(max_points >= 1 && max_points <= BLF_HULL_MAX_POINTS,
                "blf_hull3d_hrep: max_points %d outside [1, %d]", max_points, BLF_HULL_MAX_POINTS);
    BLF_REQUIRE(max_facets >= 1 && max_facets <= BLF_HULL3D_MAX_FACETS,
                "blf_hull3d_hrep: max_facets %d outside [1, %d]", max_facets, BLF_HULL3D_MAX_FACETS);
    BLF_REQUIRE(batch >= 0, "blf_hull3d_hrep: negative batch");
    BLF_REQUIRE(batch == 0 || (pts && npts && A && b && nfacets), "blf_hull3d_hrep: null buffer");
    return launch_hull3d(pts, npts, max_points, max_facets, batch, A, b, nfacets,
                         (hipStream_t)stream);
}

blf_status blf_hullnd_hrep(blf_handle* handle, int32_t dim, const double* pts, const int32_t* npts,
                           int32_t max_points, int32_t max_facets, int64_t batch, double* A,
                           double* b, int32_t* nfacets, void* stream)
{
    BLF_REQUIRE(handle != nullptr, "blf_hullnd_hrep: null handle");
    BLF_REQUIRE(dim >= 1 && dim <= BLF_HULLND_MAX_DIM, "blf_hullnd_hrep: dim %d outside [1, %d]", dim,
                BLF_HULLND_MAX_DIM);
    BLF_REQUIRE(max_points >= 1 && max_points <= BLF_HULLND_MAX_POINTS,
                "blf_hullnd_hrep: max_points %d outside [1, %d]", max_points, BLF_HULLND_MAX_POINTS);
    BLF_REQUIRE(max_facets >= 1 && max_facets <= BLF_HULLND_MAX_FACETS,
                "blf_hullnd_hrep: max_facets %d outside [1, %d]", max_facets, BLF_HULLND_MAX_FACETS);
    BLF_REQUIRE(batch >= 0, "blf_hullnd_hrep: negative batch");
    BLF_REQUIRE(batch == 0 || (pts && npts && A && b && nfacets), "blf_hullnd_hrep: null buffer");
    int64_t subsets = 1;   // C(max_points, dim)
    for (int k = 1; k <= dim; ++k) subsets = subsets * (max_points - dim + k) / k;
    if (subsets > BLF_HULLND_MAX_SUBSETS)
        return set_error(BLF_ERR_UNSUPPORTED, "blf_hullnd_hrep: C(%d, %d) = %lld subsets above %d",
                         max_points, dim, (long long)subsets, BLF_HULLND_MAX_SUBSETS);
    return launch_hullnd(dim, pts, npts, max_points, max_facets, batch, A, b, nfacets,
                         (hipStream_t)stream);
}

blf_status blf_halfspace_contains(blf_handle* handle, const double* A, const double* b,
                                  const int32_t* nfacets, int32_t dim, int32_t max_facets,
                                  const double* query, int64_t batch, int32_t* inside, void* stream)
{
    BLF_REQUIRE(handle != nullptr, "blf_halfspace_contains: null handle");
    BLF_REQUIRE(dim >= 1, "blf_halfspace_contains: dim %d", dim);
    BLF_REQUIRE(max_facets >= 1, "blf_halfspace_contains: max_facets %d", max_facets);
    BLF_REQUIRE(batch >= 0, "blf_halfspace_contains: negative batch");
    BLF_REQUIRE(batch == 0 || (A && b && nfacets && query && inside),
                "blf_halfspace_contains: null buffer");
    return launch_halfspace_contains(A, b, nfacets, dim, max_facets, query, batch, inside,
                                     (hipStream_t)stream);
}

blf_status blf_quintic_fit(blf_handle* handle, const double* knots_t, const double* knots_pva,
                           int32_t nknots, int32_t dim, int64_t nsplines, double* coeffs,
                           void* stream)
{
    BLF_REQUIRE(handle != nullptr, "blf_quintic_fit: null handle");
    BLF_REQUIRE(nknots >= 2, "blf_quintic_fit: nknots %d < 2", nknots);
    BLF_REQUIRE(dim >= 1 && dim <= 3, "blf_quintic_fit: dim %d outside [1, 3]", dim);
    BLF_REQUIRE(nsplines >= 0, "blf_quintic_fit: negative nsplines");
    BLF_REQUIRE(nsplines == 0 || (knots_t && knots_pva && coeffs), "blf_quintic_fit: null buffer");
    return launch_quintic_fit(knots_t, knots_pva, nknots, dim, nsplines, coeffs,
                              (hipStream_t)stream);
}

blf_status blf_quintic_eval(blf_handle* handle, const double* knots_t, const double* coeffs,
                            int32_t nknots, int32_t dim, int64_t nsplines, const double* tq,
                            int32_t nq, double* pva, int32_t* knot_idx, void* stream)
{
    BLF_REQUIRE(handle != nullptr, "blf_quintic_eval: null handle");
    BLF_REQUIRE(nknots >= 2, "blf_quintic_eval: nknots %d < 2", nknots);
    BLF_REQUIRE(dim >= 1 && dim <= 3, "blf_quintic_eval: dim %d outside [1, 3]", dim);
    BLF_REQUIRE(nsplines >= 0 && nq >= 0, "blf_quintic_eval: negative size");
    BLF_REQUIRE(nsplines == 0 || nq == 0 || (knots_t && coeffs && tq && pva && knot_idx),
                "blf_quintic_eval: null buffer");
    return launch_quintic_eval(knots_t, coeffs, nknots, dim, nsplines, tq, nq, pva, knot_idx,
                               (hipStream_t)stream);
}

void blf_dcm_mpc_default_params(blf_dcm_mpc_params* p, int32_t horizon)
{
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->horizon = horizon;
    p->max_facets = 8;
    p->max_iter = 50;
    p->dt = 0.02;
    p->w_xi[0] = p->w_xi[1] = 1e2;
    p->w_vrp[0] = p->w_vrp[1] = 1.0;
    p->w_terminal[0] = p->w_terminal[1] = 1e3;
    p->tol_mu = 1e-16;
    p->tol_primal = 1e-10;
    p->tol_dual = 1e-9;
    p->tol_polish = 3e-4;
}

blf_status blf_dcm_phase_expand(blf_handle* handle, const blf_phase_table* ph,
                                int64_t start_knot, double dt, int32_t horizon, int64_t batch,
                                double* A, double* b, int32_t* nfacets, double* xi_ref,
                                double* vrp_ref, void* stream)
{
    BLF_REQUIRE(handle != nullptr, "blf_dcm_phase_expand: null handle");
    BLF_REQUIRE(ph != nullptr, "blf_dcm_phase_expand: null phase table");
    BLF_REQUIRE(ph->max_phases >= 1, "blf_dcm_phase_expand: max_phases %d < 1", ph->max_phases);
    BLF_REQUIRE(ph->max_facets >= 1 && ph->max_facets <= kMaxFacetsWide,
                "blf_dcm_phase_expand: max_facets %d outside [1, %d]", ph->max_facets, kMaxFacetsWide);
    BLF_REQUIRE(horizon >= 1, "blf_dcm_phase_expand: horizon %d < 1", horizon);
    BLF_REQUIRE(dt > 0 && std::isfinite(dt), "blf_dcm_phase_expand: dt must be finite and > 0");
    BLF_REQUIRE(start_knot >= 0, "blf_dcm_phase_expand: start_knot < 0");
    BLF_REQUIRE(batch >= 0, "blf_dcm_phase_expand: negative batch");
    BLF_REQUIRE(batch == 0 || (ph->nphases && ph->begin && ph->end && ph->A && ph->b &&
                               ph->nfacets && ph->ref && A && b && nfacets && xi_ref && vrp_ref),
                "blf_dcm_phase_expand: null buffer");
    return launch_phase_expand(ph->max_phases, ph->nphases, ph->begin, ph->end, ph->A, ph->b,
                               ph->nfacets, ph->ref, ph->max_facets, start_knot, dt, horizon,
                               batch, A, b, nfacets, xi_ref, vrp_ref, (hipStream_t)stream);
}

// The warm-start argument checks of every QP entry point.
static blf_status check_warm(const char* fn, const blf_dcm_mpc_warm_start* warm, int64_t batch,
                             const blf_dcm_mpc_solution* solution, const double* lambda_out)
{
    if (!warm) return BLF_OK;
    BLF_REQUIRE(batch == 0 || (warm->vrp && warm->lambda), "%s: null warm-start buffer", fn);
    BLF_REQUIRE(warm->shift >= 0, "%s: shift %d < 0", fn, warm->shift);
    BLF_REQUIRE(warm->reserved == 0, "%s: reserved must be 0", fn);
    BLF_REQUIRE(warm->floor > 0 && std::isfinite(warm->floor), "%s: floor must be finite and > 0", fn);
    BLF_REQUIRE(warm->vrp != solution->vrp && warm->lambda != lambda_out &&
                    (warm->prev_status == nullptr || warm->prev_status != solution->status),
                "%s: warm-start buffers must not alias the outputs", fn);
    return BLF_OK;
}

blf_status blf_dcm_mpc_solve_warm(blf_handle* handle, const blf_dcm_mpc_params* params,
                                  const blf_dcm_mpc_problem* problem,
                                  const blf_dcm_mpc_warm_start* warm, int64_t batch,
                                  const blf_dcm_mpc_solution* solution, double* lambda_out,
                                  void* stream)
{
    BLF_REQUIRE(handle != nullptr, "blf_dcm_mpc_solve: null handle");
    BLF_REQUIRE(params && problem && solution, "blf_dcm_mpc_solve: null argument");
    BLF_REQUIRE(params->horizon >= 1, "blf_dcm_mpc_solve: horizon %d < 1", params->horizon);
    BLF_REQUIRE(params->max_facets >= 1 && params->max_facets <= kMaxFacetsWide,
                "blf_dcm_mpc_solve: max_facets %d outside [1, %d]", params->max_facets, kMaxFacetsWide);
    BLF_REQUIRE(params->max_iter >= 0, "blf_dcm_mpc_solve: max_iter < 0");
    BLF_REQUIRE(params->reserved == 0, "blf_dcm_mpc_solve: reserved must be 0");
    BLF_REQUIRE(params->dt > 0, "blf_dcm_mpc_solve: dt must be > 0");
    BLF_REQUIRE(params->w_vrp[0] > 0 && params->w_vrp[1] > 0 && params->w_xi[0] >= 0 &&
                    params->w_xi[1] >= 0 && params->w_terminal[0] >= 0 && params->w_terminal[1] >= 0,
                "blf_dcm_mpc_solve: weights must be R > 0, Q >= 0, P >= 0");
    BLF_REQUIRE(batch >= 0, "blf_dcm_mpc_solve: negative batch");
    BLF_REQUIRE(batch == 0 || (problem->xi_init && problem->omega && problem->xi_ref &&
                               problem->vrp_ref && problem->A && problem->b && problem->nfacets &&
                               solution->xi && solution->vrp && solution->status && solution->iters),
                "blf_dcm_mpc_solve: null buffer");
    {
        const blf_status st = check_warm("blf_dcm_mpc_solve_warm", warm, batch, solution, lambda_out);
        if (st != BLF_OK) return st;
    }
    if (batch == 0) return BLF_OK;
    Stage2List list{};
    const blf_status st = handle->h.stage2_list((hipStream_t)stream, batch, &list);
    if (st != BLF_OK) return st;
    return launch_dcm_mpc(params, problem, warm, batch, solution, lambda_out, (hipStream_t)stream, list);
}

static blf_status phased_solve(const char* fn, blf_handle* handle,
                               const blf_dcm_mpc_params* params, const blf_phase_table* ph, int64_t start_knot,
                               const double* xi_init, const double* omega, int64_t omega_stride,
                               const blf_dcm_mpc_warm_start* warm, int64_t batch,
                               const blf_dcm_mpc_window* win, const blf_dcm_mpc_solution* solution,
                               double* lambda_out, void* stream)
{
    BLF_REQUIRE(handle != nullptr, "%s: null handle", fn);
    BLF_REQUIRE(params && ph && win && solution, "%s: null argument", fn);
    BLF_REQUIRE(ph->max_phases >= 1, "%s: max_phases %d < 1", fn, ph->max_phases);
    BLF_REQUIRE(ph->max_facets == params->max_facets,
                "%s: phase table max_facets %d != params max_facets %d", fn,
                ph->max_facets, params->max_facets);
    BLF_REQUIRE(start_knot >= 0, "%s: start_knot < 0", fn);
    BLF_REQUIRE(omega_stride >= params->horizon, "%s: omega_stride %lld < horizon %d", fn,
                (long long)omega_stride, params->horizon);
    BLF_REQUIRE(batch == 0 || (ph->nphases && ph->begin && ph->end && ph->A && ph->b && ph->nfacets &&
                               ph->ref && win->omega && win->xi_ref && win->vrp_ref && win->A &&
                               win->b && win->nfacets),
                "%s: null buffer", fn);
    // the QP arguments as blf_dcm_mpc_solve_warm checks them (the window scratch stands in for the
    // per-knot arrays, which this call does not read)
    const blf_dcm_mpc_problem pb{xi_init, omega, win->xi_ref, win->vrp_ref, win->A, win->b, win->nfacets};
    if (batch > 0) {
        BLF_REQUIRE(params->horizon >= 1 && params->horizon <= 128,
                    "%s: horizon %d outside [1, 128]", fn, params->horizon);
        BLF_REQUIRE(params->tol_polish > 0, "%s: tol_polish must be > 0", fn);
    }
    BLF_REQUIRE(params->max_facets >= 1 && params->max_facets <= kMaxFacetsWide,
                "%s: max_facets %d outside [1, %d]", fn, params->max_facets, kMaxFacetsWide);
    BLF_REQUIRE(params->max_iter >= 0, "%s: max_iter < 0", fn);
    BLF_REQUIRE(params->reserved == 0, "%s: reserved must be 0", fn);
    BLF_REQUIRE(params->dt > 0 && std::isfinite(params->dt), "%s: dt must be finite and > 0", fn);
    BLF_REQUIRE(params->w_vrp[0] > 0 && params->w_vrp[1] > 0 && params->w_xi[0] >= 0 &&
                    params->w_xi[1] >= 0 && params->w_terminal[0] >= 0 && params->w_terminal[1] >= 0,
                "%s: weights must be R > 0, Q >= 0, P >= 0", fn);
    BLF_REQUIRE(batch >= 0, "%s: negative batch", fn);
    BLF_REQUIRE(batch == 0 || (pb.xi_init && pb.omega && solution->xi && solution->vrp &&
                               solution->status && solution->iters),
                "%s: null buffer", fn);
    blf_status st = check_warm(fn, warm, batch, solution, lambda_out);
    if (st != BLF_OK || batch == 0) return st;
    Stage2List list{};
    st = handle->h.stage2_list((hipStream_t)stream, batch, &list);
    if (st != BLF_OK) return st;
    return launch_dcm_mpc_phased(params, ph, start_knot, xi_init, omega, omega_stride, warm, batch,
                                 win, solution, lambda_out, (hipStream_t)stream, list);
}

blf_status blf_dcm_mpc_solve_phased(blf_handle* handle, const blf_dcm_mpc_params* params,
                                    const blf_phase_table* ph, int64_t start_knot,
                                    const double* xi_init, const double* omega,
                                    int64_t omega_stride, const blf_dcm_mpc_warm_start* warm,
                                    int64_t batch, const blf_dcm_mpc_window* win,
                                    const blf_dcm_mpc_solution* solution, double* lambda_out,
                                    void* stream)
{
    return phased_solve("blf_dcm_mpc_solve_phased", handle, params, ph, start_knot, xi_init, omega,
                        omega_stride, warm, batch, win, solution, lambda_out, stream);
}

blf_status blf_dcm_mpc_solve(blf_handle* handle, const blf_dcm_mpc_params* params,
                             const blf_dcm_mpc_problem* problem, int64_t batch,
                             const blf_dcm_mpc_solution* solution, void* stream)
{
    return blf_dcm_mpc_solve_warm(handle, params, problem, nullptr, batch, solution, nullptr,
                                  stream);
}

double blf_dcm_mpc_flops_per_iter(int32_t horizon, int64_t active_facets)
{
    // Algorithmic flops of one IPM iteration, counted on the sequential restatement of the
    // algorithm (fp64 add/sub/mul/div = 1 flop, negation / fabs / compares
    // not counted) — the device's lane scans do more arithmetic than this on purpose:
    //   per knot:  residuals 20, E 10, Riccati step 40, H^-1 / M / G 45, two solves 2 x 66,
    //              update 8                                                         = 255
    //   per facet: residual 11, W-phase 22, affine ratio 16, mu_aff 18, corrector rhs 27,
    //              corrector step 31, update 12                                     = 137
    //   per facet pair (det W): 6, i.e. 3 m(m-1) per knot; taken as 12 per facet (m ~ 5)
    return 149.0 * (double)active_facets + 255.0 * (double)horizon;
}

}  // extern "C"

extern "C" {

blf_status blf_contact_model_eval(blf_handle* handle, const double* params, int32_t shared_params,
                                  const double* twist, const double* pose,
                                  const double* null_pose, int64_t batch, double* wrench,
                                  double* autonomous, double* control, double* regressor,
                                  void* stream)
{
    BLF_REQUIRE(handle != nullptr, "blf_contact_model_eval: null handle");
    BLF_REQUIRE(batch >= 0, "blf_contact_model_eval: negative batch");
    BLF_REQUIRE(batch == 0 || (params && twist && pose && null_pose),
                "blf_contact_model_eval: null input buffer");
    BLF_REQUIRE(wrench || autonomous || control || regressor,
                "blf_contact_model_eval: no output requested");
    return launch_contact_eval(params, shared_params, twist, pose, null_pose, batch, wrench,
                               autonomous, control, regressor, (hipStream_t)stream);
}

blf_status blf_contact_point_wrench(blf_handle* handle, const double* params,
                                    int32_t shared_params, const double* twist, const double* pose,
                                    const double* null_pose, int64_t batch, const double* points,
                                    int32_t npoints, double* force, double* torque, void* stream)
{
    BLF_REQUIRE(handle != nullptr, "blf_contact_point_wrench: null handle");
    BLF_REQUIRE(batch >= 0 && npoints >= 0, "blf_contact_point_wrench: negative size");
    BLF_REQUIRE(batch == 0 || npoints == 0 ||
                    (params && twist && pose && null_pose && points && force && torque),
                "blf_contact_point_wrench: null buffer");
    return launch_contact_point(params, shared_params, twist, pose, null_pose, batch, points,
                                npoints, force, torque, (hipStream_t)stream);
}

blf_status blf_fbk_dynamics(blf_handle* handle, int32_t ndof, double rho, const double* rot,
                            const double* twist, const double* joint_vel, double* dpos,
                            double* drot, double* djoints, int64_t batch, void* stream)
{
    BLF_REQUIRE(handle != nullptr, "blf_fbk_dynamics: null handle");
    BLF_REQUIRE(ndof >= 0 && ndof <= BLF_FBK_MAX_DOFS, "blf_fbk_dynamics: ndof=%d outside [0, %d]",
                ndof, BLF_FBK_MAX_DOFS);
    BLF_REQUIRE(batch >= 0, "blf_fbk_dynamics: negative batch");
    BLF_REQUIRE(batch == 0 || (rot && twist && dpos && drot && (ndof == 0 || (joint_vel && djoints))),
                "blf_fbk_dynamics: null buffer");
    return launch_fbk_dynamics(ndof, rho, rot, twist, joint_vel, dpos, drot, djoints, batch,
                               (hipStream_t)stream);
}

blf_status blf_fbk_euler_integrate(blf_handle* handle, int32_t ndof, double rho, double* pos,
                                   double* rot, double* joints, const double* twist,
                                   const double* joint_vel, int64_t batch, double initial_time,
                                   double final_time, double dT, void* stream)
{
    BLF_REQUIRE(handle != nullptr, "blf_fbk_euler_integrate: null handle");
    BLF_REQUIRE(ndof >= 0 && ndof <= BLF_FBK_MAX_DOFS,
                "blf_fbk_euler_integrate: ndof=%d outside [0, %d]", ndof, BLF_FBK_MAX_DOFS);
    BLF_REQUIRE(batch >= 0, "blf_fbk_euler_integrate: negative batch");
    BLF_REQUIRE(batch == 0 || (pos && rot && twist && (ndof == 0 || (joints && joint_vel))),
                "blf_fbk_euler_integrate: null buffer");
    return scheduled(initial_time, final_time, dT, [&](int iterations, double dT_last) {
        return launch_fbk_euler(ndof, rho, pos, rot, joints, twist, joint_vel, batch, iterations, dT,
                                dT_last, (hipStream_t)stream);
    });
}

}  // extern "C"

// The checks blf_rls_advance and blf_contact_rls_advance share (before any device work).
static blf_status check_rls(const char* fn, blf_handle* handle, double lambda, int32_t steps,
                            int64_t batch)
{
    BLF_REQUIRE(handle != nullptr, "%s: null handle", fn);
    BLF_REQUIRE(steps >= 1, "%s: steps=%d, must be >= 1", fn, steps);
    BLF_REQUIRE(batch >= 0, "%s: negative batch", fn);
    BLF_REQUIRE(std::isfinite(lambda) && lambda > 0.0, "%s: lambda=%g, must be finite and positive",
                fn, lambda);
    return BLF_OK;
}

extern "C" {

blf_status blf_rls_advance(blf_handle* handle, int32_t n, int32_t m, double lambda,
                           const double* meas_cov, int32_t shared_cov, const double* regressor,
                           const double* measurements, int32_t steps, double* state,
                           double* covariance, int64_t batch, void* stream)
{
    const blf_status st = check_rls("blf_rls_advance", handle, lambda, steps, batch);
    if (st != BLF_OK) return st;
    BLF_REQUIRE(meas_cov != nullptr, "blf_rls_advance: null meas_cov");
    BLF_REQUIRE(regressor != nullptr, "blf_rls_advance: null regressor");
    BLF_REQUIRE(measurements != nullptr, "blf_rls_advance: null measurements");
    BLF_REQUIRE(state != nullptr, "blf_rls_advance: null state");
    BLF_REQUIRE(covariance != nullptr, "blf_rls_advance: null covariance");
    if (n < 1 || n > BLF_RLS_MAX_STATE)
        return set_error(BLF_ERR_UNSUPPORTED, "blf_rls_advance: n=%d outside [1, %d]", n,
                         BLF_RLS_MAX_STATE);
    if (m < 1 || m > BLF_RLS_MAX_MEAS)
        return set_error(BLF_ERR_UNSUPPORTED, "blf_rls_advance: m=%d outside [1, %d]", m,
                         BLF_RLS_MAX_MEAS);
    return launch_rls_advance(n, m, lambda, meas_cov, shared_cov, regressor, measurements, steps,
                              state, covariance, batch, (hipStream_t)stream);
}

blf_status blf_contact_rls_advance(blf_handle* handle, double lambda, const double* meas_cov,
                                   int32_t shared_cov, const double* geometry,
                                   int32_t shared_geometry, const double* twist, const double* pose,
                                   const double* null_pose, const double* wrench, int32_t steps,
                                   double* state, double* covariance, int64_t batch, void* stream)
{
    const blf_status st = check_rls("blf_contact_rls_advance", handle, lambda, steps, batch);
    if (st != BLF_OK) return st;
    BLF_REQUIRE(meas_cov != nullptr, "blf_contact_rls_advance: null meas_cov");
    BLF_REQUIRE(geometry != nullptr, "blf_contact_rls_advance: null geometry");
    BLF_REQUIRE(twist != nullptr, "blf_contact_rls_advance: null twist");
    BLF_REQUIRE(pose != nullptr, "blf_contact_rls_advance: null pose");
    BLF_REQUIRE(null_pose != nullptr, "blf_contact_rls_advance: null null_pose");
    BLF_REQUIRE(wrench != nullptr, "blf_contact_rls_advance: null wrench");
    BLF_REQUIRE(state != nullptr, "blf_contact_rls_advance: null state");
    BLF_REQUIRE(covariance != nullptr, "blf_contact_rls_advance: null covariance");
    return launch_contact_rls(lambda, meas_cov, shared_cov, geometry, shared_geometry, twist, pose,
                              null_pose, wrench, steps, state, covariance, batch,
                              (hipStream_t)stream);
}

blf_status blf_swing_foot_eval(blf_handle* handle, const blf_swing_foot_params* params,
                               const double* contact_pose, const double* contact_time,
                               const int32_t* ncontacts, int64_t batch, const double* tq,
                               int32_t nq, double* pose, double* twist, double* accel,
                               int32_t* contact_idx, int32_t* in_contact, void* stream)
{
    BLF_REQUIRE(handle != nullptr, "blf_swing_foot_eval: null handle");
    BLF_REQUIRE(params != nullptr, "blf_swing_foot_eval: null params");
    BLF_REQUIRE(params->reserved == 0, "blf_swing_foot_eval: params->reserved must be 0");
    BLF_REQUIRE(std::isfinite(params->step_height) && params->step_height >= 0.0,
                "blf_swing_foot_eval: step_height=%g, must be finite and >= 0", params->step_height);
    BLF_REQUIRE(params->apex_ratio > 0.0 && params->apex_ratio < 1.0,
                "blf_swing_foot_eval: apex_ratio=%g outside (0, 1)", params->apex_ratio);
    BLF_REQUIRE(std::isfinite(params->landing_velocity),
                "blf_swing_foot_eval: landing_velocity is not finite");
    BLF_REQUIRE(std::isfinite(params->landing_acceleration),
                "blf_swing_foot_eval: landing_acceleration is not finite");
    BLF_REQUIRE(batch >= 0, "blf_swing_foot_eval: negative batch");
    BLF_REQUIRE(nq >= 0, "blf_swing_foot_eval: negative nq");
    BLF_REQUIRE(contact_pose != nullptr, "blf_swing_foot_eval: null contact_pose");
    BLF_REQUIRE(contact_time != nullptr, "blf_swing_foot_eval: null contact_time");
    BLF_REQUIRE(ncontacts != nullptr, "blf_swing_foot_eval: null ncontacts");
    BLF_REQUIRE(tq != nullptr, "blf_swing_foot_eval: null tq");
    BLF_REQUIRE(pose || twist || accel || contact_idx || in_contact,
                "blf_swing_foot_eval: no output requested");
    if (params->max_contacts < 1 || params->max_contacts > BLF_SWING_MAX_CONTACTS)
        return set_error(BLF_ERR_UNSUPPORTED, "blf_swing_foot_eval: max_contacts=%d outside [1, %d]",
                         params->max_contacts, BLF_SWING_MAX_CONTACTS);
    return launch_swing_foot_eval(params, contact_pose, contact_time, ncontacts, batch, tq, nq,
                                  pose, twist, accel, contact_idx, in_contact,
                                  (hipStream_t)stream);
}

blf_status blf_so3_eval(blf_handle* handle, const double* R0, const double* R1,
                        const double* duration, int64_t batch, const double* tq, int32_t nq,
                        double* rot, double* omega, double* alpha, void* stream)
{
    BLF_REQUIRE(handle != nullptr, "blf_so3_eval: null handle");
    BLF_REQUIRE(batch >= 0, "blf_so3_eval: negative batch");
    BLF_REQUIRE(nq >= 0, "blf_so3_eval: negative nq");
    BLF_REQUIRE(R0 != nullptr, "blf_so3_eval: null R0");
    BLF_REQUIRE(R1 != nullptr, "blf_so3_eval: null R1");
    BLF_REQUIRE(duration != nullptr, "blf_so3_eval: null duration");
    BLF_REQUIRE(tq != nullptr, "blf_so3_eval: null tq");
    BLF_REQUIRE(rot || omega || alpha, "blf_so3_eval: no output requested");
    return launch_so3_eval(R0, R1, duration, batch, tq, nq, rot, omega, alpha,
                           (hipStream_t)stream);
}

}  // extern "C"

// The argument checks of the floating-base calls (sections 8 to 12d).  A helper holds a run of checks
// that always come together and takes the entry point's name for its messages.  The order of the checks
// is part of the interface (tests/test_fb_refusals.py pins which reports first), and so is what differs
// between the families, which is an argument below, not a consequence of the helper a call reuses:
//   family      ndof outside [1, 48]              more than 8 contacts       LDS bound, layout
//   kinematics  INVALID, before batch             -                          -
//   kForward    INVALID, before batch             INVALID, with C < 0        160 KB, the mass matrix's
//   kInverse    UNSUPPORTED, after the pointers   UNSUPPORTED, after ndof    80 KB, the articulated body's
//   IK          UNSUPPORTED, after batch          -                          160 KB, the call's own
// kinematics: blf_fb_dcm, blf_fb_frame_state.  kForward: blf_fbd_dynamics, blf_fbd_euler_integrate and its
// _impedance and _impedance_traj forms; the bound is the mass matrix's whatever the call launches.
// kInverse: blf_fb_inverse_dynamics and the _computed_torque_traj integration; ndof comes after C < 0.
// IK: the seven blf_fb_ik_* calls; ndof comes before nse3, the bound after the staged copies.
// The joint torque is an argument of blf_fbd_dynamics and blf_fbd_euler_integrate only, which require
// it with the state buffers (check_dynamics' `inputs`); the laws of the other calls replace it.
static blf_status check_model_state(const char* fn, const blf_handle* handle, const blf_fb_model* model,
                                    const blf_fb_state* state)
{
    BLF_REQUIRE(handle != nullptr, "%s: null handle", fn);
    BLF_REQUIRE(model != nullptr && state != nullptr, "%s: null model / state", fn);
    return BLF_OK;
}

static blf_status check_ndof(const char* fn, const blf_fb_model* model, blf_status refused)
{
    if (model->ndof < 1 || model->ndof > BLF_FBD_MAX_DOFS)
        return set_error(refused, "%s: ndof=%d outside [1, %d]", fn, model->ndof, BLF_FBD_MAX_DOFS);
    return BLF_OK;
}

static blf_status check_model_arrays(const char* fn, const blf_fb_model* model)
{
    BLF_REQUIRE(model->parent && model->joint_origin && model->joint_rot && model->joint_axis &&
                    model->link_mass && model->link_com && model->link_inertia,
                "%s: null model array", fn);
    return BLF_OK;
}

// Where a family checks ndof (the table): in front of batch as an invalid argument, or after the pointers
enum NdofOrder { kNdofFirst, kNdofLater };

// The first checks of every call but the IK ones (which check their tasks in between): handle, model
// and state, ndof where the family checks it in front, batch >= 0, the model arrays.  nframes: the
// size blf_fb_frame_state checks along with batch (one check, one message).
static blf_status check_model(const char* fn, const blf_handle* handle, const blf_fb_model* model,
                              const blf_fb_state* state, NdofOrder order, int64_t batch, const int32_t* nframes = nullptr)
{
    blf_status st = check_model_state(fn, handle, model, state);
    if (st == BLF_OK && order == kNdofFirst) st = check_ndof(fn, model, BLF_ERR_INVALID_ARGUMENT);
    if (st != BLF_OK) return st;
    BLF_REQUIRE(batch >= 0 && (!nframes || *nframes >= 0), "%s: negative %s", fn, nframes ? "size" : "batch");
    return check_model_arrays(fn, model);
}

// Whether the state buffers a call reads are there: positions (the IK solves), velocities, or both
enum : int { kPos = 1, kVel = 2, kPosVel = kPos | kVel };
static bool state_given(const blf_fb_state* s, int which)
{
    return (!(which & kVel) || (s->base_vel && s->joint_vel)) &&
           (!(which & kPos) || (s->base_pos && s->base_rot && s->joint_pos));
}

static blf_status check_lds(const char* fn, size_t bytes, size_t bound = 160 * 1024)
{
    if (bytes > bound) return set_error(BLF_ERR_UNSUPPORTED, "%s: model too large for one workgroup's LDS", fn);
    return BLF_OK;
}

struct FbFamily {
    blf_status sizes;   // what an ndof outside [1, 48] and more than 8 contacts report
    NdofOrder order;    // kNdofFirst: also the contact count's range in one check; kNdofLater: ndof, then C > 8
    bool aba;           // the LDS layout the bound is taken of (fbd_lds_bytes)
    size_t lds;
};
constexpr FbFamily kForward{BLF_ERR_INVALID_ARGUMENT, kNdofFirst, false, 160 * 1024};
constexpr FbFamily kInverse{BLF_ERR_UNSUPPORTED, kNdofLater, true, 160 * 1024 / 2};

static blf_status check_contacts(const char* fn, const blf_fb_model* model, const blf_fb_contacts* contacts,
                                 int64_t batch, const FbFamily& fam)
{
    const int C = contacts ? contacts->ncontacts : 0;
    if (fam.order == kNdofFirst) {
        BLF_REQUIRE(C >= 0 && C <= BLF_FBD_MAX_CONTACTS, "%s: %d contacts outside [0, %d]", fn, C,
                    BLF_FBD_MAX_CONTACTS);
    } else {
        BLF_REQUIRE(C >= 0, "%s: %d contacts", fn, C);
        const blf_status st = check_ndof(fn, model, fam.sizes);
        if (st != BLF_OK) return st;
        if (C > BLF_FBD_MAX_CONTACTS)
            return set_error(fam.sizes, "%s: %d contacts, at most %d", fn, C, BLF_FBD_MAX_CONTACTS);
    }
    BLF_REQUIRE(C == 0 || (contacts->frame && contacts->params && contacts->null_pose &&
                           model->frame_link && model->frame_pose && model->nframes > 0),
                "%s: null contact buffer", fn);
    BLF_REQUIRE(C == 0 || contacts->law == nullptr || batch == 0 || contacts->wrench != nullptr,
                "%s: contact laws given without the wrench buffer", fn);
    return check_lds(fn, fbd_lds_bytes(model->ndof, C, fam.aba), fam.lds);
}

// The checks of the dynamics calls (kForward, kInverse).  inputs: whether the pointers the call
// requires along with the state buffers are there.
static blf_status check_dynamics(const char* fn, const blf_handle* handle, const blf_fb_model* model,
                                 const blf_fb_state* state, const blf_fb_contacts* contacts, int64_t batch,
                                 const FbFamily& fam, bool inputs = true)
{
    const blf_status st = check_model(fn, handle, model, state, fam.order, batch);
    if (st != BLF_OK) return st;
    BLF_REQUIRE(batch == 0 || (state_given(state, kPosVel) && inputs), "%s: null state buffer", fn);
    return check_contacts(fn, model, contacts, batch, fam);
}

// The fields the three torque laws share, in the calls' order; what: how the messages name the struct
template <class Law>
static blf_status check_law(const char* fn, const char* what, const Law* law, const blf_fb_model* model,
                            int64_t batch)
{
    BLF_REQUIRE(law != nullptr, "%s: null %s", fn, what);
    BLF_REQUIRE(law->reserved == 0, "%s: reserved must be 0", fn);
    if constexpr (!std::is_same<Law, blf_joint_impedance>::value) {
        BLF_REQUIRE(law->slices >= 1 && law->steps_per_slice >= 1,
                    "%s: slices=%d, steps_per_slice=%d, both must be >= 1", fn, law->slices, law->steps_per_slice);
    }
    BLF_REQUIRE(law->kp && law->kd && (batch == 0 || law->q_ref), "%s: null %s array", fn, what);
    BLF_REQUIRE(model != nullptr && law->ndof == model->ndof, "%s: %s ndof %d != model ndof %d", fn, what,
                law->ndof, model ? model->ndof : -1);
    if constexpr (!std::is_same<Law, blf_joint_impedance>::value) {
        BLF_REQUIRE(law->qd_ref == nullptr || law->qd_stride >= law->ndof, "%s: qd_stride=%lld below ndof=%d", fn,
                    (long long)law->qd_stride, law->ndof);
    }
    return BLF_OK;
}

extern "C" {

blf_status blf_fbd_dynamics(blf_handle* handle, const blf_fb_model* model,
                            const blf_fb_state* state, const double* joint_torque,
                            const blf_fb_contacts* contacts, const double* mass_reg,
                            int64_t batch, const blf_fb_state* out, void* stream)
{
    const char* fn = "blf_fbd_dynamics";
    const blf_status st = check_dynamics(fn, handle, model, state, contacts, batch, kForward, joint_torque != nullptr);
    if (st != BLF_OK) return st;
    BLF_REQUIRE(out != nullptr && (batch == 0 || state_given(out, kPosVel)), "%s: null output buffer", fn);
    return launch_fbd_dynamics(model, state, joint_torque, contacts, mass_reg, batch, out,
                               (hipStream_t)stream);
}

blf_status blf_fb_dcm(blf_handle* handle, const blf_fb_model* model, const blf_fb_state* state,
                      const double* omega0, int64_t omega0_stride, int64_t batch, double* com,
                      double* xi, void* stream)
{
    const char* fn = "blf_fb_dcm";
    const blf_status st = check_model(fn, handle, model, state, kNdofFirst, batch);
    if (st != BLF_OK) return st;
    BLF_REQUIRE(batch == 0 || (state_given(state, kPosVel) && com), "%s: null state / output buffer", fn);
    BLF_REQUIRE(xi == nullptr || omega0 != nullptr, "%s: xi requested without omega0", fn);
    BLF_REQUIRE(omega0_stride >= 0, "%s: negative omega0 stride", fn);
    return launch_fb_dcm(model, state, omega0, omega0_stride, batch, com, xi, (hipStream_t)stream);
}

blf_status blf_fb_frame_state(blf_handle* handle, const blf_fb_model* model,
                              const blf_fb_state* state, int32_t nframes, const int32_t* frames,
                              int64_t batch, double* pose, double* twist, void* stream)
{
    const char* fn = "blf_fb_frame_state";
    const blf_status st = check_model(fn, handle, model, state, kNdofFirst, batch, &nframes);
    if (st != BLF_OK) return st;
    BLF_REQUIRE(nframes == 0 || (frames && model->frame_link && model->frame_pose && model->nframes > 0),
                "%s: null frame buffer", fn);
    BLF_REQUIRE(batch == 0 || nframes == 0 || ((pose || twist) && state_given(state, kPosVel)),
                "%s: null state / output buffer", fn);
    return launch_fb_frame_state(model, state, nframes, frames, batch, pose, twist,
                                 (hipStream_t)stream);
}

blf_status blf_dcm_posture_reference(blf_handle* handle, const blf_posture_law* law,
                                     const double* com, const double* vrp, int64_t vrp_stride,
                                     int64_t batch, double* q_ref, void* stream)
{
    BLF_REQUIRE(handle != nullptr, "blf_dcm_posture_reference: null handle");
    BLF_REQUIRE(law != nullptr, "blf_dcm_posture_reference: null law");
    BLF_REQUIRE(law->reserved == 0, "blf_dcm_posture_reference: reserved must be 0");
    BLF_REQUIRE(law->ndof >= 1 && law->ndof <= BLF_FBD_MAX_DOFS,
                "blf_dcm_posture_reference: ndof=%d outside [1, %d]", law->ndof, BLF_FBD_MAX_DOFS);
    BLF_REQUIRE(law->q_nominal && law->lean, "blf_dcm_posture_reference: null law array");
    BLF_REQUIRE(batch >= 0 && vrp_stride >= 2, "blf_dcm_posture_reference: bad batch / vrp stride");
    BLF_REQUIRE(batch == 0 || (com && vrp && q_ref), "blf_dcm_posture_reference: null buffer");
    return launch_posture_reference(law, com, vrp, vrp_stride, batch, q_ref, (hipStream_t)stream);
}

blf_status blf_fbd_euler_integrate_impedance(blf_handle* handle, const blf_fb_model* model,
                                             const blf_fb_state* state,
                                             const blf_joint_impedance* impedance,
                                             const blf_fb_contacts* contacts,
                                             const double* mass_reg, int64_t batch,
                                             double initial_time, double final_time, double dT,
                                             void* stream)
{
    const char* fn = "blf_fbd_euler_integrate_impedance";
    blf_status st = check_law(fn, "impedance", impedance, model, batch);
    if (st == BLF_OK) st = check_dynamics(fn, handle, model, state, contacts, batch, kForward);
    if (st != BLF_OK) return st;
    return scheduled(initial_time, final_time, dT, [&](int iterations, double dT_last) {
        return launch_fbd_euler(model, state, nullptr, contacts, mass_reg, batch, iterations, dT, dT_last,
                                (hipStream_t)stream, impedance);
    });
}

blf_status blf_fbd_euler_integrate_impedance_traj(blf_handle* handle, const blf_fb_model* model,
                                                  const blf_fb_state* state,
                                                  const blf_joint_impedance_traj* impedance,
                                                  const blf_fb_contacts* contacts,
                                                  const double* mass_reg, int64_t batch,
                                                  double initial_time, double final_time, double dT,
                                                  void* stream)
{
    const char* fn = "blf_fbd_euler_integrate_impedance_traj";
    blf_status st = check_law(fn, "impedance", impedance, model, batch);
    if (st == BLF_OK) st = check_dynamics(fn, handle, model, state, contacts, batch, kForward);
    if (st != BLF_OK) return st;
    return scheduled(initial_time, final_time, dT, [&](int iterations, double dT_last) {
        return launch_fbd_euler_traj(model, state, contacts, mass_reg, batch, iterations, dT, dT_last,
                                     (hipStream_t)stream, impedance);
    });
}

blf_status blf_fb_inverse_dynamics(blf_handle* handle, const blf_fb_model* model,
                                   const blf_fb_state* state, const double* joint_acc,
                                   const double* base_acc, const blf_fb_contacts* contacts,
                                   int64_t batch, double* joint_torque, double* base_acc_out,
                                   double* base_wrench, int32_t* status, int32_t reserved,
                                   void* stream)
{
    const char* fn = "blf_fb_inverse_dynamics";
    BLF_REQUIRE(reserved == 0, "%s: reserved must be 0", fn);
    const blf_status st = check_dynamics(fn, handle, model, state, contacts, batch, kInverse);
    if (st != BLF_OK) return st;
    double* const bout = base_acc ? base_wrench : base_acc_out;
    BLF_REQUIRE(batch == 0 || (joint_torque && bout), "%s: null %s", fn,
                !joint_torque ? "joint_torque" : base_acc ? "base_wrench (given-base mode)" : "base_acc_out (free-base mode)");
    return launch_fb_invdyn(model, state, joint_acc, base_acc, contacts, batch, joint_torque, bout, status,
                            (hipStream_t)stream);
}

blf_status blf_fbd_euler_integrate_computed_torque_traj(blf_handle* handle, const blf_fb_model* model,
                                                        const blf_fb_state* state,
                                                        const blf_computed_torque_traj* law,
                                                        const blf_fb_contacts* contacts,
                                                        const double* mass_reg, int64_t batch,
                                                        double initial_time, double final_time,
                                                        double dT, void* stream)
{
    const char* fn = "blf_fbd_euler_integrate_computed_torque_traj";
    blf_status st = check_law(fn, "law", law, model, batch);
    if (st != BLF_OK) return st;
    BLF_REQUIRE(law->qdd_ref == nullptr || law->qdd_stride >= law->ndof, "%s: qdd_stride=%lld below ndof=%d", fn,
                (long long)law->qdd_stride, law->ndof);
    st = check_dynamics(fn, handle, model, state, contacts, batch, kInverse);
    if (st != BLF_OK) return st;
    if (mass_reg != nullptr)
        return set_error(BLF_ERR_UNSUPPORTED, "%s: mass_reg given (inverse dynamics is defined without it)", fn);
    return scheduled(initial_time, final_time, dT, [&](int iterations, double dT_last) {
        return launch_fbd_euler_ctq(model, state, contacts, batch, iterations, dT, dT_last, (hipStream_t)stream, law);
    });
}

blf_status blf_dcm_com_reference(blf_handle* handle, const double* xi0, const double* vrp,
                                 int64_t vrp_stride, const double* omega0, int64_t omega0_stride,
                                 const double* z_ref, double* c_ref, int32_t steps, double dT,
                                 int64_t batch, double* com_pos, double* com_vel, double* xi_end,
                                 void* stream)
{
    BLF_REQUIRE(handle != nullptr, "blf_dcm_com_reference: null handle");
    BLF_REQUIRE(steps >= 1, "blf_dcm_com_reference: steps=%d, must be >= 1", steps);
    BLF_REQUIRE(std::isfinite(dT) && dT > 0.0, "blf_dcm_com_reference: dT=%g, must be finite and positive", dT);
    BLF_REQUIRE(batch >= 0 && vrp_stride >= 2 && omega0_stride >= 0,
                "blf_dcm_com_reference: bad batch / vrp stride / omega0 stride");
    BLF_REQUIRE(batch == 0 || (xi0 && vrp && omega0 && z_ref && c_ref && com_pos && com_vel),
                "blf_dcm_com_reference: null buffer");
    return launch_com_reference(xi0, vrp, vrp_stride, omega0, omega0_stride, z_ref, c_ref, steps, dT, batch,
                                com_pos, com_vel, xi_end, (hipStream_t)stream);
}

blf_status blf_fbd_euler_integrate(blf_handle* handle, const blf_fb_model* model,
                                   const blf_fb_state* state, const double* joint_torque,
                                   const blf_fb_contacts* contacts, const double* mass_reg,
                                   int64_t batch, double initial_time, double final_time,
                                   double dT, void* stream)
{
    const blf_status st = check_dynamics("blf_fbd_euler_integrate", handle, model, state, contacts, batch, kForward,
                                         joint_torque != nullptr);
    if (st != BLF_OK) return st;
    return scheduled(initial_time, final_time, dT, [&](int iterations, double dT_last) {
        return launch_fbd_euler(model, state, joint_torque, contacts, mass_reg, batch, iterations, dT, dT_last,
                                (hipStream_t)stream);
    });
}

}  // extern "C"

// Section 13.  The checks both calls make alike: the sizes every sibling of section 10 checks, then the
// slot count, then the trigger parameters (host memory: read here, no staged copy).
static blf_status check_triggers(const char* fn, const blf_handle* handle, int32_t K, const double* params,
                                 int32_t shared, int32_t steps, int64_t batch)
{
    BLF_REQUIRE(handle != nullptr, "%s: null handle", fn);
    BLF_REQUIRE(steps >= 1, "%s: steps=%d, must be >= 1", fn, steps);
    BLF_REQUIRE(batch >= 0, "%s: negative batch", fn);
    BLF_REQUIRE(params != nullptr, "%s: null params", fn);
    if (K < 1 || K > BLF_ODOM_MAX_CONTACTS)
        return set_error(BLF_ERR_UNSUPPORTED, "%s: ncontacts=%d outside [1, %d]", fn, K, BLF_ODOM_MAX_CONTACTS);
    for (int c = 0; c < (shared ? 1 : K); ++c) {
        const double* p = params + 4 * c;
        BLF_REQUIRE(std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]) && std::isfinite(p[3]),
                    "%s: params[%d] holds a threshold or delay that is not finite", fn, c);
        BLF_REQUIRE(p[2] >= 0.0 && p[3] >= 0.0, "%s: params[%d] holds a negative delay", fn, c);
        BLF_REQUIRE(p[0] >= p[1], "%s: params[%d]: on_threshold=%g below off_threshold=%g", fn, c, p[0], p[1]);
    }
    return BLF_OK;
}

extern "C" {

blf_status blf_schmitt_trigger_advance(blf_handle* handle, int32_t ncontacts, const double* params,
                                       int32_t shared_params, const double* time, const double* value,
                                       int32_t steps, int32_t* state, double* timers, int32_t* state_out,
                                       int64_t batch, void* stream)
{
    const char* fn = "blf_schmitt_trigger_advance";
    const blf_status st = check_triggers(fn, handle, ncontacts, params, shared_params, steps, batch);
    if (st != BLF_OK) return st;
    BLF_REQUIRE(time != nullptr, "%s: null time", fn);
    BLF_REQUIRE(batch == 0 || value != nullptr, "%s: null value", fn);
    BLF_REQUIRE(batch == 0 || state != nullptr, "%s: null state", fn);
    BLF_REQUIRE(batch == 0 || timers != nullptr, "%s: null timers", fn);
    return launch_schmitt_trigger(params, shared_params, ncontacts, time, value, steps, state, timers, state_out,
                                  batch, (hipStream_t)stream);
}

blf_status blf_legged_odometry_advance(blf_handle* handle, const blf_fb_model* model, int32_t ncontacts,
                                       const int32_t* frames, const double* params, int32_t shared_params,
                                       const double* time, const double* joint_pos, const double* joint_vel,
                                       const double* normal_force, int32_t steps, int32_t* trig_state,
                                       double* trig_timers, int32_t* fixed_frame, double* fixed_pose,
                                       double* base_pos, double* base_rot, double* base_vel,
                                       int32_t* contact_out, int32_t* fixed_out, int32_t* status, int64_t batch,
                                       int32_t reserved, void* stream)
{
    const char* fn = "blf_legged_odometry_advance";
    BLF_REQUIRE(reserved == 0, "%s: reserved must be 0", fn);
    BLF_REQUIRE(model != nullptr, "%s: null model", fn);
    blf_status st = check_triggers(fn, handle, ncontacts, params, shared_params, steps, batch);
    if (st == BLF_OK) st = check_ndof(fn, model, BLF_ERR_UNSUPPORTED);
    if (st == BLF_OK) st = check_model_arrays(fn, model);
    if (st != BLF_OK) return st;
    BLF_REQUIRE(frames && model->frame_link && model->frame_pose && model->nframes > 0, "%s: null frame buffer", fn);
    BLF_REQUIRE(time != nullptr, "%s: null time", fn);
    BLF_REQUIRE(batch == 0 || joint_pos != nullptr, "%s: null joint_pos", fn);
    BLF_REQUIRE(batch == 0 || normal_force != nullptr, "%s: null normal_force", fn);
    BLF_REQUIRE(batch == 0 || (trig_state && trig_timers && fixed_frame && fixed_pose), "%s: null estimator state", fn);
    BLF_REQUIRE(batch == 0 || base_pos || base_rot || base_vel || contact_out || fixed_out || status,
                "%s: no output requested", fn);
    st = check_lds(fn, odometry_lds_bytes(model->ndof, ncontacts), kInverse.lds);
    if (st != BLF_OK) return st;
    return launch_legged_odometry(model, ncontacts, frames, params, shared_params, time, joint_pos, joint_vel,
                                  normal_force, steps, trig_state, trig_timers, fixed_frame, fixed_pose, base_pos,
                                  base_rot, base_vel, contact_out, fixed_out, status, batch, (hipStream_t)stream);
}

}  // extern "C"

// The checks blf_fb_ik_solve and blf_fb_ik_integrate share.  The shared weight and gain arrays are
// device memory: they are copied to the host on the call's stream and checked there before the
// launch (section 12: a staged copy).
// wout (or null): receives the staged se3_weight 6K | se3_kp 2K | com_weight 3 when batch > 0.
// setpoints = false (section 12d): tasks->se3_pose and com_pos are not read, so not required.
static blf_status check_ik(const char* fn, blf_handle* handle, const blf_fb_model* model,
                           const blf_fb_state* state, const blf_ik_tasks* t, int64_t batch,
                           hipStream_t s, double* wout = nullptr, bool setpoints = true)
{
    blf_status st = check_model_state(fn, handle, model, state);
    if (st != BLF_OK) return st;
    BLF_REQUIRE(t != nullptr, "%s: null tasks", fn);
    BLF_REQUIRE(t->reserved == 0, "%s: tasks->reserved must be 0", fn);
    BLF_REQUIRE(batch >= 0, "%s: negative batch", fn);
    st = check_ndof(fn, model, BLF_ERR_UNSUPPORTED);
    if (st != BLF_OK) return st;
    if (t->nse3 < 0 || t->nse3 > BLF_IK_MAX_SE3_TASKS)
        return set_error(BLF_ERR_UNSUPPORTED, "%s: nse3=%d outside [0, %d]", fn, t->nse3,
                         BLF_IK_MAX_SE3_TASKS);
    const int n = model->ndof, K = t->nse3;
    st = check_model_arrays(fn, model);
    if (st != BLF_OK) return st;
    BLF_REQUIRE(K == 0 || (t->frame && t->se3_weight && t->se3_kp && model->frame_link &&
                           model->frame_pose && model->nframes > 0),
                "%s: null SE3 task array", fn);
    BLF_REQUIRE(t->joint_weight && t->joint_kp, "%s: null joint task array", fn);
    BLF_REQUIRE(std::isfinite(t->base_damping) && t->base_damping >= 0.0,
                "%s: base_damping=%g, must be finite and >= 0", fn, t->base_damping);
    BLF_REQUIRE(t->com_weight == nullptr || (std::isfinite(t->com_kp) && t->com_kp >= 0.0),
                "%s: com_kp=%g, must be finite and >= 0", fn, t->com_kp);
    if (batch == 0) return BLF_OK;
    BLF_REQUIRE(state_given(state, kPos), "%s: null state buffer", fn);
    BLF_REQUIRE(!setpoints || K == 0 || t->se3_pose, "%s: null se3_pose", fn);
    BLF_REQUIRE(!setpoints || t->com_weight == nullptr || t->com_pos, "%s: com_weight given without com_pos", fn);
    BLF_REQUIRE(t->joint_pos != nullptr, "%s: null joint_pos set point", fn);
    // the staged copy: se3_weight 6K | se3_kp 2K | com_weight 3 | joint_weight n | joint_kp n
    double hbuf[8 * BLF_IK_MAX_SE3_TASKS + 3 + 2 * BLF_FBD_MAX_DOFS];
    const bool com = t->com_weight != nullptr;
    const struct { const double* src; int count; } parts[5] = {
        {t->se3_weight, 6 * K}, {t->se3_kp, 2 * K}, {t->com_weight, com ? 3 : 0},
        {t->joint_weight, n}, {t->joint_kp, n}};
    int at = 0;
    for (const auto& p : parts) {
        if (p.count > 0) {
            st = check_hip(hipMemcpyAsync(hbuf + at, p.src, sizeof(double) * p.count, hipMemcpyDeviceToHost, s),
                           "blf_fb_ik: staging the task weights");
            if (st != BLF_OK) return st;
        }
        at += p.count;
    }
    st = check_hip(hipStreamSynchronize(s), "blf_fb_ik: staging the task weights");
    if (st != BLF_OK) return st;
    const int jw0 = 8 * K + (com ? 3 : 0);
    for (int i = 0; i < at; ++i) {
        const double v = hbuf[i];
        const bool positive = i >= jw0 && i < jw0 + n;   // joint_weight
        BLF_REQUIRE(std::isfinite(v) && (positive ? v > 0.0 : v >= 0.0),
                    "%s: %s[%d]=%g, must be finite and %s", fn,
                    i < 6 * K ? "se3_weight" : i < 8 * K ? "se3_kp" : i < jw0 ? "com_weight"
                    : positive ? "joint_weight" : "joint_kp",
                    i < 6 * K ? i : i < 8 * K ? i - 6 * K : i < jw0 ? i - 8 * K : positive ? i - jw0 : i - jw0 - n,
                    v, positive ? "> 0" : ">= 0");
    }
    st = check_lds(fn, fb_ik_lds_bytes(n, K));
    if (st != BLF_OK) return st;
    if (wout)
        for (int i = 0; i < jw0; ++i) wout[i] = hbuf[i];
    return BLF_OK;
}

// Section 12b's checks after check_ik's: the mask against the task set (and, when batch > 0, against
// the staged weights), reserved and rel_pivot_min.  Leaves the kernel's row bits in *slots (0: the
// soft path) and the pivot bound in *tau.
static blf_status check_ik_hard(const char* fn, blf_handle* handle, const blf_fb_model* model,
                                const blf_fb_state* state, const blf_ik_tasks* t, const blf_ik_hard* hard,
                                int64_t batch, hipStream_t s, uint32_t* slots, double* tau,
                                double* wout = nullptr, bool setpoints = true)
{
    double wown[8 * BLF_IK_MAX_SE3_TASKS + 3];
    double* w = wout ? wout : wown;
    const blf_status st = check_ik(fn, handle, model, state, t, batch, s, w, setpoints);
    if (st != BLF_OK) return st;
    *slots = 0;
    *tau = 0.0;
    if (hard == nullptr) return BLF_OK;
    BLF_REQUIRE(hard->reserved == 0, "%s: hard->reserved must be 0", fn);
    BLF_REQUIRE(std::isfinite(hard->rel_pivot_min) && hard->rel_pivot_min >= 0.0 && hard->rel_pivot_min < 1.0,
                "%s: rel_pivot_min=%g, must be finite and in [0, 1)", fn, hard->rel_pivot_min);
    const uint32_t rows = hard->rows;
    const int K = t->nse3;
    BLF_REQUIRE((rows >> 27) == 0u, "%s: hard->rows=0x%x has bits above 26", fn, rows);
    const uint32_t se3 = rows & 0xffffffu, com = rows >> 24;
    BLF_REQUIRE((se3 >> (6 * K)) == 0u, "%s: hard->rows=0x%x names an SE3 task >= nse3=%d", fn, rows, K);
    BLF_REQUIRE(com == 0u || t->com_weight != nullptr, "%s: hard->rows=0x%x marks CoM rows without a CoM task",
                fn, rows);
    if (batch > 0) {
        for (int r = 0; r < 6 * K; ++r)
            BLF_REQUIRE(!((se3 >> r) & 1u) || w[r] > 0.0, "%s: hard row %d of SE3 task %d has weight 0", fn,
                        r % 6, r / 6);
        for (int a = 0; a < 3; ++a)
            BLF_REQUIRE(!((com >> a) & 1u) || w[8 * K + a] > 0.0, "%s: hard CoM row %d has weight 0", fn, a);
    }
    *slots = se3 | (com << (6 * K));
    *tau = hard->rel_pivot_min > 0.0 ? hard->rel_pivot_min : 1.0e-8;
    return BLF_OK;
}

// Section 12c's checks after check_ik_hard's: the struct's scalars (any batch) ...
static blf_status check_ik_limits_scalars(const char* fn, const blf_ik_limits* lim)
{
    BLF_REQUIRE(lim->reserved == 0, "%s: limits->reserved must be 0", fn);
    BLF_REQUIRE(std::isfinite(lim->sampling_time) && lim->sampling_time > 0.0,
                "%s: sampling_time=%g, must be finite and positive", fn, lim->sampling_time);
    BLF_REQUIRE(lim->max_iter >= 0, "%s: max_iter=%d, must be >= 0", fn, lim->max_iter);
    return BLF_OK;
}

// ... and, when batch > 0, the limit arrays through a staged copy like check_ik's.  Leaves the default
// in *max_iter when the caller gave 0.
static blf_status check_ik_limits(const char* fn, const blf_ik_limits* lim, int n, hipStream_t s, int32_t* max_iter)
{
    BLF_REQUIRE(lim->pos_lower && lim->pos_upper && lim->klim, "%s: null limit array", fn);
    double hbuf[4 * BLF_FBD_MAX_DOFS];
    const double* src[4] = {lim->pos_lower, lim->pos_upper, lim->klim, lim->vel_max};
    for (int a = 0; a < 4; ++a) {
        if (src[a] == nullptr) continue;
        const blf_status st = check_hip(
            hipMemcpyAsync(hbuf + a * n, src[a], sizeof(double) * n, hipMemcpyDeviceToHost, s),
            "blf_fb_ik: staging the joint limits");
        if (st != BLF_OK) return st;
    }
    const blf_status st = check_hip(hipStreamSynchronize(s), "blf_fb_ik: staging the joint limits");
    if (st != BLF_OK) return st;
    for (int j = 0; j < n; ++j) {
        const double lo = hbuf[j], up = hbuf[n + j], kl = hbuf[2 * n + j];
        BLF_REQUIRE(lo <= up && lo < HUGE_VAL && up > -HUGE_VAL,
                    "%s: pos_lower[%d]=%g, pos_upper[%d]=%g, must be ordered (and not NaN)", fn, j, lo, j, up);
        BLF_REQUIRE(kl > 0.0 && kl <= 1.0, "%s: klim[%d]=%g, must be in (0, 1]", fn, j, kl);
        BLF_REQUIRE(lim->vel_max == nullptr || hbuf[3 * n + j] > 0.0, "%s: vel_max[%d]=%g, must be > 0", fn, j,
                    lim->vel_max ? hbuf[3 * n + j] : 0.0);
    }
    *max_iter = lim->max_iter > 0 ? lim->max_iter : BLF_IK_LIMITS_DEFAULT_MAX_ITER;
    return BLF_OK;
}

// The first checks of the three blf_fb_ik_integrate* calls
static blf_status check_steps_dt(const char* fn, int32_t steps, double dT)
{
    BLF_REQUIRE(steps >= 1, "%s: steps=%d, must be >= 1", fn, steps);
    BLF_REQUIRE(std::isfinite(dT) && dT > 0.0, "%s: dT=%g, must be finite and positive", fn, dT);
    return BLF_OK;
}

// blf_fb_ik_solve_limits (steps == 0) and blf_fb_ik_integrate_limits after their own argument checks
static blf_status ik_limits_call(const char* fn, blf_handle* handle, const blf_fb_model* model,
                                 const blf_fb_state* state, const blf_ik_tasks* tasks, const blf_ik_hard* hard,
                                 const blf_ik_limits* limits, int64_t batch, int32_t steps, double dT, double* nu,
                                 int32_t* status, int32_t* iters, uint64_t* active, hipStream_t s)
{
    uint32_t slots = 0;
    double tau = 0.0;
    const blf_status st = check_ik_hard(fn, handle, model, state, tasks, hard, batch, s, &slots, &tau);
    if (st != BLF_OK) return st;
    BLF_REQUIRE(batch == 0 || steps > 0 || nu != nullptr, "%s: null nu", fn);
    BLF_REQUIRE(batch == 0 || steps == 0 || state_given(state, kVel), "%s: null state buffer", fn);
    if (limits == nullptr) return launch_fb_ik(model, state, tasks, batch, steps, dT, nu, status, s, slots, tau);
    blf_ik_limits lim = *limits;
    blf_status sl = check_ik_limits_scalars(fn, limits);
    if (sl == BLF_OK && batch > 0) sl = check_ik_limits(fn, limits, model->ndof, s, &lim.max_iter);
    if (sl == BLF_OK && batch > 0) sl = check_lds(fn, fb_ik_lds_bytes(model->ndof, tasks->nse3, true));
    if (sl != BLF_OK) return sl;
    return launch_fb_ik_limits(model, state, tasks, &lim, batch, steps, dT, nu, status, iters, active, s, slots, tau);
}

extern "C" {

blf_status blf_fb_ik_solve_limits(blf_handle* handle, const blf_fb_model* model, const blf_fb_state* state,
                                  const blf_ik_tasks* tasks, const blf_ik_hard* hard, const blf_ik_limits* limits,
                                  int64_t batch, double* nu, int32_t* status, int32_t* iters, uint64_t* active,
                                  void* stream)
{
    return ik_limits_call("blf_fb_ik_solve_limits", handle, model, state, tasks, hard, limits, batch, 0, 0.0, nu,
                          status, iters, active, (hipStream_t)stream);
}

blf_status blf_fb_ik_integrate_limits(blf_handle* handle, const blf_fb_model* model, const blf_fb_state* state,
                                      const blf_ik_tasks* tasks, const blf_ik_hard* hard,
                                      const blf_ik_limits* limits, int64_t batch, int32_t steps, double dT,
                                      double* nu, int32_t* status, int32_t* iters, uint64_t* active, void* stream)
{
    const char* fn = "blf_fb_ik_integrate_limits";
    const blf_status st = check_steps_dt(fn, steps, dT);
    if (st != BLF_OK) return st;
    return ik_limits_call(fn, handle, model, state, tasks, hard, limits, batch, steps, dT, nu, status, iters, active,
                          (hipStream_t)stream);
}

blf_status blf_fb_ik_track(blf_handle* handle, const blf_fb_model* model, const blf_fb_state* state,
                           const blf_ik_tasks* tasks, const blf_ik_hard* hard, const blf_ik_limits* limits,
                           const blf_ik_schedule* schedule, int64_t batch, double dT, double* joint_traj,
                           double* base_traj, double* nu_traj, int32_t* status, int32_t* fail_step, int32_t* iters,
                           uint64_t* active, void* stream)
{
    const char* fn = "blf_fb_ik_track";
    hipStream_t s = (hipStream_t)stream;
    BLF_REQUIRE(schedule != nullptr, "%s: null schedule", fn);
    // (check_steps_dt's two checks, with schedule->reserved between them)
    BLF_REQUIRE(schedule->steps >= 1, "%s: steps=%d, must be >= 1", fn, schedule->steps);
    BLF_REQUIRE(schedule->reserved == 0 && schedule->reserved2 == 0u, "%s: schedule->reserved must be 0", fn);
    BLF_REQUIRE(std::isfinite(dT) && dT > 0.0, "%s: dT=%g, must be finite and positive", fn, dT);
    uint32_t slots = 0;
    double tau = 0.0, w[8 * BLF_IK_MAX_SE3_TASKS + 3];
    blf_status st = check_ik_hard(fn, handle, model, state, tasks, hard, batch, s, &slots, &tau, w, false);
    if (st != BLF_OK) return st;
    const int K = tasks->nse3;
    const uint32_t stance = schedule->stance_rows;
    BLF_REQUIRE((uint64_t)stance >> (6 * K) == 0u, "%s: stance_rows=0x%x has bits outside the %d SE3 tasks", fn,
                stance, K);
    if (batch > 0)
        for (int r = 0; r < 6 * K; ++r)
            BLF_REQUIRE(!((stance >> r) & 1u) || w[r] > 0.0, "%s: stance row %d of SE3 task %d has weight 0", fn,
                        r % 6, r / 6);
    blf_ik_limits lim;
    if (limits != nullptr) {
        lim = *limits;
        st = check_ik_limits_scalars(fn, limits);
        if (st != BLF_OK) return st;
    }
    if (batch == 0) return BLF_OK;
    BLF_REQUIRE(state_given(state, kVel), "%s: null state buffer", fn);
    BLF_REQUIRE(K == 0 || schedule->se3_pose, "%s: null schedule->se3_pose", fn);
    BLF_REQUIRE(tasks->com_weight == nullptr || schedule->com_pos, "%s: com_weight given without schedule->com_pos",
                fn);
    if (limits != nullptr) st = check_ik_limits(fn, limits, model->ndof, s, &lim.max_iter);
    if (st == BLF_OK) st = check_lds(fn, fb_ik_track_lds_bytes(model->ndof, K));
    if (st != BLF_OK) return st;
    // tau of a call without `hard`: the default (stance rows may still be hard)
    return launch_fb_ik_track(model, state, tasks, limits ? &lim : nullptr, schedule, batch, dT, joint_traj,
                              base_traj, nu_traj, status, fail_step, iters, active, s, slots, stance,
                              tau > 0.0 ? tau : 1.0e-8);
}

blf_status blf_fb_ik_solve(blf_handle* handle, const blf_fb_model* model, const blf_fb_state* state,
                           const blf_ik_tasks* tasks, int64_t batch, double* nu, int32_t* status,
                           void* stream)
{
    const blf_status st = check_ik("blf_fb_ik_solve", handle, model, state, tasks, batch, (hipStream_t)stream);
    if (st != BLF_OK) return st;
    BLF_REQUIRE(batch == 0 || nu != nullptr, "blf_fb_ik_solve: null nu");
    return launch_fb_ik(model, state, tasks, batch, 0, 0.0, nu, status, (hipStream_t)stream);
}

blf_status blf_fb_ik_integrate(blf_handle* handle, const blf_fb_model* model, const blf_fb_state* state,
                               const blf_ik_tasks* tasks, int64_t batch, int32_t steps, double dT,
                               double* nu, int32_t* status, void* stream)
{
    const char* fn = "blf_fb_ik_integrate";
    blf_status st = check_steps_dt(fn, steps, dT);
    if (st == BLF_OK) st = check_ik(fn, handle, model, state, tasks, batch, (hipStream_t)stream);
    if (st != BLF_OK) return st;
    BLF_REQUIRE(batch == 0 || state_given(state, kVel), "%s: null state buffer", fn);
    return launch_fb_ik(model, state, tasks, batch, steps, dT, nu, status, (hipStream_t)stream);
}

blf_status blf_fb_ik_solve_hard(blf_handle* handle, const blf_fb_model* model, const blf_fb_state* state,
                                const blf_ik_tasks* tasks, const blf_ik_hard* hard, int64_t batch, double* nu,
                                int32_t* status, void* stream)
{
    uint32_t slots = 0;
    double tau = 0.0;
    const blf_status st = check_ik_hard("blf_fb_ik_solve_hard", handle, model, state, tasks, hard, batch,
                                        (hipStream_t)stream, &slots, &tau);
    if (st != BLF_OK) return st;
    BLF_REQUIRE(batch == 0 || nu != nullptr, "blf_fb_ik_solve_hard: null nu");
    return launch_fb_ik(model, state, tasks, batch, 0, 0.0, nu, status, (hipStream_t)stream, slots, tau);
}

blf_status blf_fb_ik_integrate_hard(blf_handle* handle, const blf_fb_model* model, const blf_fb_state* state,
                                    const blf_ik_tasks* tasks, const blf_ik_hard* hard, int64_t batch,
                                    int32_t steps, double dT, double* nu, int32_t* status, void* stream)
{
    const char* fn = "blf_fb_ik_integrate_hard";
    uint32_t slots = 0;
    double tau = 0.0;
    blf_status st = check_steps_dt(fn, steps, dT);
    if (st == BLF_OK) st = check_ik_hard(fn, handle, model, state, tasks, hard, batch, (hipStream_t)stream, &slots, &tau);
    if (st != BLF_OK) return st;
    BLF_REQUIRE(batch == 0 || state_given(state, kVel), "%s: null state buffer", fn);
    return launch_fb_ik(model, state, tasks, batch, steps, dT, nu, status, (hipStream_t)stream, slots, tau);
}

}  // extern "C"
