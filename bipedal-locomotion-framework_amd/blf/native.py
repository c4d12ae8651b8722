"""ctypes binding of the C ABI in include/blf/blf_c.h (lib/libblf.so, built for gfx950).

torch is used only as device-memory and stream plumbing: every function takes torch CUDA
tensors, checks dtype/shape/contiguity/device on the host, and passes raw device pointers plus
torch's current HIP stream to the library.  There is no CPU fallback: if lib/libblf.so is
missing or cannot be loaded, `lib()` raises, and every op raises with it.
"""
import ctypes
import os

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(_PKG, "lib", "libblf.so")
# diagnostic builds only (tools/kbench.py): BLF_LIB points at e.g. lib/libblf_stamps.so
LIB_PATH = os.environ.get("BLF_LIB", LIB_PATH)

BLF_OK = 0
STATUS_NAMES = {0: "BLF_OK", 1: "BLF_ERR_INVALID_ARGUMENT", 2: "BLF_ERR_HIP",
                3: "BLF_ERR_UNSUPPORTED", 4: "BLF_ERR_TIME_INTERVAL", 5: "BLF_ERR_EMPTY_INTERVAL"}
QP_SOLVED, QP_MAX_ITER, QP_NUMERICAL, QP_BAD_FACETS = 0, 1, 2, 3

# entry points removed in round 5 (measured slower, never the default; tests/test_abi.py checks
# that the library no longer exports them)
REMOVED = ["blf_set_qp_split_batch", "blf_stream_create_cu_range", "blf_stream_destroy",
           "blf_dcm_mpc_solve_phased_begin", "blf_dcm_mpc_solve_phased_finish",
           "blf_dcm_posture_reference_masked", "blf_fbd_euler_integrate_impedance_masked"]

_vp = ctypes.c_void_p
_i32 = ctypes.c_int32
_i64 = ctypes.c_int64
_f64 = ctypes.c_double


class FbModel(ctypes.Structure):
    """blf_fb_model (include/blf/blf_c.h); every pointer is device memory."""
    _fields_ = [("ndof", _i32), ("nframes", _i32), ("parent", _vp), ("joint_origin", _vp),
                ("joint_rot", _vp), ("joint_axis", _vp), ("link_mass", _vp), ("link_com", _vp),
                ("link_inertia", _vp), ("frame_link", _vp), ("frame_pose", _vp),
                ("gravity", _f64 * 3), ("rho", _f64), ("joint_type", _vp)]


class FbState(ctypes.Structure):
    _fields_ = [("base_vel", _vp), ("joint_vel", _vp), ("base_pos", _vp), ("base_rot", _vp),
                ("joint_pos", _vp)]


CONTACT_CONTINUOUS, CONTACT_WRENCH = 0, 1   # blf_fb_contacts.law (BLF_CONTACT_*)


class FbContacts(ctypes.Structure):
    _fields_ = [("ncontacts", _i32), ("frame", _vp), ("params", _vp), ("null_pose", _vp),
                ("law", _vp), ("wrench", _vp)]


class PostureLaw(ctypes.Structure):
    """blf_posture_law (include/blf/blf_c.h): the closed loop's plan -> joint reference map."""
    _fields_ = [("ndof", _i32), ("reserved", _i32), ("q_nominal", _vp), ("lean", _vp)]


class JointImpedance(ctypes.Structure):
    """blf_joint_impedance: tau = kp (q_ref - q) - kd qdot before every Euler step."""
    _fields_ = [("ndof", _i32), ("reserved", _i32), ("kp", _vp), ("kd", _vp), ("q_ref", _vp)]


class JointImpedanceTraj(ctypes.Structure):
    """blf_joint_impedance_traj: the impedance with the reference indexed by the integration step."""
    _fields_ = [("ndof", _i32), ("slices", _i32), ("steps_per_slice", _i32), ("reserved", _i32),
                ("kp", _vp), ("kd", _vp), ("q_ref", _vp), ("qd_ref", _vp), ("qd_stride", _i64),
                ("q_bias", _vp)]


class ComputedTorqueTraj(ctypes.Structure):
    """blf_computed_torque_traj: computed torque from inverse dynamics, references indexed by the step."""
    _fields_ = [("ndof", _i32), ("slices", _i32), ("steps_per_slice", _i32), ("reserved", _i32),
                ("kp", _vp), ("kd", _vp), ("q_ref", _vp), ("qd_ref", _vp), ("qd_stride", _i64),
                ("qdd_ref", _vp), ("qdd_stride", _i64), ("q_bias", _vp), ("tau_max", _vp), ("tau_last", _vp)]


class SwingFootParams(ctypes.Structure):
    """blf_swing_foot_params (include/blf/blf_c.h section 11)."""
    _fields_ = [("max_contacts", _i32), ("reserved", _i32), ("step_height", _f64),
                ("apex_ratio", _f64), ("landing_velocity", _f64), ("landing_acceleration", _f64)]


class IkTasks(ctypes.Structure):
    """blf_ik_tasks (include/blf/blf_c.h section 12); every pointer is device memory."""
    _fields_ = [("nse3", _i32), ("reserved", _i32), ("frame", _vp), ("se3_weight", _vp), ("se3_kp", _vp),
                ("se3_pose", _vp), ("se3_twist", _vp), ("com_weight", _vp), ("com_kp", _f64),
                ("com_pos", _vp), ("com_vel", _vp), ("joint_weight", _vp), ("joint_kp", _vp),
                ("joint_pos", _vp), ("joint_vel", _vp), ("base_damping", _f64)]


class IkHard(ctypes.Structure):
    """blf_ik_hard (include/blf/blf_c.h section 12b)."""
    _fields_ = [("rows", ctypes.c_uint32), ("reserved", _i32), ("rel_pivot_min", _f64)]


class IkLimits(ctypes.Structure):
    """blf_ik_limits (include/blf/blf_c.h section 12c); every pointer is device memory."""
    _fields_ = [("pos_lower", _vp), ("pos_upper", _vp), ("klim", _vp), ("vel_max", _vp),
                ("sampling_time", _f64), ("max_iter", _i32), ("reserved", _i32)]


class IkSchedule(ctypes.Structure):
    """blf_ik_schedule (include/blf/blf_c.h section 12d); every pointer is device memory."""
    _fields_ = [("steps", _i32), ("reserved", _i32), ("stance_rows", ctypes.c_uint32),
                ("reserved2", ctypes.c_uint32), ("contact", _vp), ("se3_pose", _vp), ("se3_twist", _vp),
                ("com_pos", _vp), ("com_vel", _vp)]


IK_OK, IK_NOT_POSITIVE, IK_BAD_INPUT = 0, 1, 2   # per-robot status of fb_ik_solve / fb_ik_integrate
IK_HARD_DEPENDENT = 3   # with hard rows: a pivot of S failed the rule (section 12b)
IK_LIMITS_UNRESOLVED = 4   # with limits: the active-set iteration found no feasible optimal set (section 12c)

SWING_OUTPUTS = ("pose", "twist", "accel", "contact_idx", "in_contact")
SO3_OUTPUTS = ("rot", "omega", "alpha")

FB_STATE_KEYS =("base_vel", "joint_vel", "base_pos", "base_rot", "joint_pos")


class BlfError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"{STATUS_NAMES.get(code, code)}: {msg}")
        self.code = code


class DcmMpcParams(ctypes.Structure):
    _fields_ = [("horizon", _i32), ("max_facets", _i32), ("max_iter", _i32), ("reserved", _i32),
                ("dt", _f64), ("w_xi", _f64 * 2), ("w_vrp", _f64 * 2), ("w_terminal", _f64 * 2),
                ("tol_mu", _f64), ("tol_primal", _f64), ("tol_dual", _f64), ("tol_polish", _f64)]


class DcmMpcProblem(ctypes.Structure):
    _fields_ = [("xi_init", _vp), ("omega", _vp), ("xi_ref", _vp), ("vrp_ref", _vp), ("A", _vp),
                ("b", _vp), ("nfacets", _vp)]


class DcmMpcSolution(ctypes.Structure):
    _fields_ = [("xi", _vp), ("vrp", _vp), ("status", _vp), ("iters", _vp), ("polished", _vp),
                ("passes", _vp)]


class PhaseTable(ctypes.Structure):
    _fields_ = [("max_phases", _i32), ("max_facets", _i32), ("nphases", _vp), ("begin", _vp),
                ("end", _vp), ("A", _vp), ("b", _vp), ("nfacets", _vp), ("ref", _vp)]


class DcmMpcWindow(ctypes.Structure):
    _fields_ = [("omega", _vp), ("xi_ref", _vp), ("vrp_ref", _vp), ("A", _vp), ("b", _vp),
                ("nfacets", _vp)]


class DcmMpcWarmStart(ctypes.Structure):
    _fields_ = [("vrp", _vp), ("lambda_", _vp), ("shift", _i32), ("reserved", _i32),
                ("floor", _f64), ("prev_status", _vp)]


def _sig(restype=_i32, **args):
    """A SIGNATURES entry: (result ctype, ((argument name, ctype), ...)); blf_status unless given."""
    return restype, tuple(args.items())


_P = ctypes.POINTER
_FB = dict(handle=_vp, model=_P(FbModel), state=_P(FbState))
_TIMES = dict(initial_time=_f64, final_time=_f64, dT=_f64)
# Every entry point include/blf/blf_c.h declares: its result type and its (argument name, ctype) pairs in the
# header's order (lambda_: the header's `lambda`).  lib() sets the prototypes from it; tests/test_abi.py parses
# the header and checks the table and the struct classes against it, and that the .so exports every name.
SIGNATURES = {
    "blf_create": _sig(handle=_P(_vp), device=_i32),
    "blf_destroy": _sig(handle=_vp),
    "blf_last_error": _sig(ctypes.c_char_p),
    "blf_version": _sig(ctypes.c_char_p),
    "blf_set_qp_launch_mode": _sig(fuse_stage2=_i32, single_kernel=_i32),
    "blf_step_schedule": _sig(**_TIMES, iterations=_vp, dT_last=_vp, t_last=_vp),
    "blf_lti_euler_integrate": _sig(handle=_vp, n=_i32, m=_i32, A=_vp, Bm=_vp, shared_matrices=_i32, u=_vp,
        x=_vp, batch=_i64, **_TIMES, stream=_vp),
    "blf_lti_dynamics": _sig(handle=_vp, n=_i32, m=_i32, A=_vp, Bm=_vp, shared_matrices=_i32, u=_vp, x=_vp,
        dx=_vp, batch=_i64, stream=_vp),
    "blf_dcm_euler_rollout": _sig(handle=_vp, xi0=_vp, omega=_vp, vrp=_vp, horizon=_i32, dt=_f64, xi_out=_vp,
        batch=_i64, stream=_vp),
    "blf_hull2d_hrep": _sig(handle=_vp, pts=_vp, npts=_vp, max_points=_i32, max_facets=_i32, batch=_i64, A=_vp,
        b=_vp, nfacets=_vp, stream=_vp),
    "blf_hull2d_contains": _sig(handle=_vp, A=_vp, b=_vp, nfacets=_vp, max_facets=_i32, query=_vp, batch=_i64,
        inside=_vp, stream=_vp),
    "blf_hull3d_hrep": _sig(handle=_vp, pts=_vp, npts=_vp, max_points=_i32, max_facets=_i32, batch=_i64, A=_vp,
        b=_vp, nfacets=_vp, stream=_vp),
    "blf_hullnd_hrep": _sig(handle=_vp, dim=_i32, pts=_vp, npts=_vp, max_points=_i32, max_facets=_i32,
        batch=_i64, A=_vp, b=_vp, nfacets=_vp, stream=_vp),
    "blf_halfspace_contains": _sig(handle=_vp, A=_vp, b=_vp, nfacets=_vp, dim=_i32, max_facets=_i32, query=_vp,
        batch=_i64, inside=_vp, stream=_vp),
    "blf_quintic_fit": _sig(handle=_vp, knots_t=_vp, knots_pva=_vp, nknots=_i32, dim=_i32, nsplines=_i64,
        coeffs=_vp, stream=_vp),
    "blf_quintic_eval": _sig(handle=_vp, knots_t=_vp, coeffs=_vp, nknots=_i32, dim=_i32, nsplines=_i64, tq=_vp,
        nq=_i32, pva=_vp, knot_idx=_vp, stream=_vp),
    "blf_dcm_mpc_default_params": _sig(None, p=_P(DcmMpcParams), horizon=_i32),
    "blf_dcm_mpc_solve": _sig(handle=_vp, params=_P(DcmMpcParams), problem=_P(DcmMpcProblem), batch=_i64,
        solution=_P(DcmMpcSolution), stream=_vp),
    "blf_dcm_mpc_solve_warm": _sig(handle=_vp, params=_P(DcmMpcParams), problem=_P(DcmMpcProblem),
        warm=_P(DcmMpcWarmStart), batch=_i64, solution=_P(DcmMpcSolution), lambda_out=_vp, stream=_vp),
    "blf_dcm_phase_expand": _sig(handle=_vp, phases=_P(PhaseTable), start_knot=_i64, dt=_f64, horizon=_i32,
        batch=_i64, A=_vp, b=_vp, nfacets=_vp, xi_ref=_vp, vrp_ref=_vp, stream=_vp),
    "blf_dcm_mpc_solve_phased": _sig(handle=_vp, params=_P(DcmMpcParams), phases=_P(PhaseTable),
        start_knot=_i64, xi_init=_vp, omega=_vp, omega_stride=_i64, warm=_P(DcmMpcWarmStart), batch=_i64,
        window=_P(DcmMpcWindow), solution=_P(DcmMpcSolution), lambda_out=_vp, stream=_vp),
    "blf_dcm_mpc_flops_per_iter": _sig(_f64, horizon=_i32, active_facets=_i64),
    "blf_contact_model_eval": _sig(handle=_vp, params=_vp, shared_params=_i32, twist=_vp, pose=_vp,
        null_pose=_vp, batch=_i64, wrench=_vp, autonomous=_vp, control=_vp, regressor=_vp, stream=_vp),
    "blf_contact_point_wrench": _sig(handle=_vp, params=_vp, shared_params=_i32, twist=_vp, pose=_vp,
        null_pose=_vp, batch=_i64, points=_vp, npoints=_i32, force=_vp, torque=_vp, stream=_vp),
    "blf_fbk_dynamics": _sig(handle=_vp, ndof=_i32, rho=_f64, rot=_vp, twist=_vp, joint_vel=_vp, dpos=_vp,
        drot=_vp, djoints=_vp, batch=_i64, stream=_vp),
    "blf_fbk_euler_integrate": _sig(handle=_vp, ndof=_i32, rho=_f64, pos=_vp, rot=_vp, joints=_vp, twist=_vp,
        joint_vel=_vp, batch=_i64, **_TIMES, stream=_vp),
    "blf_fbd_dynamics": _sig(**_FB, joint_torque=_vp, contacts=_P(FbContacts), mass_reg=_vp, batch=_i64,
        out=_P(FbState), stream=_vp),
    "blf_fbd_euler_integrate": _sig(**_FB, joint_torque=_vp, contacts=_P(FbContacts), mass_reg=_vp, batch=_i64,
        **_TIMES, stream=_vp),
    "blf_fb_dcm": _sig(**_FB, omega0=_vp, omega0_stride=_i64, batch=_i64, com=_vp, xi=_vp, stream=_vp),
    "blf_dcm_posture_reference": _sig(handle=_vp, law=_P(PostureLaw), com=_vp, vrp=_vp, vrp_stride=_i64,
        batch=_i64, q_ref=_vp, stream=_vp),
    "blf_fbd_euler_integrate_impedance": _sig(**_FB, impedance=_P(JointImpedance), contacts=_P(FbContacts),
        mass_reg=_vp, batch=_i64, **_TIMES, stream=_vp),
    "blf_fb_frame_state": _sig(**_FB, nframes=_i32, frames=_vp, batch=_i64, pose=_vp, twist=_vp, stream=_vp),
    "blf_rls_advance": _sig(handle=_vp, n=_i32, m=_i32, lambda_=_f64, meas_cov=_vp, shared_cov=_i32,
        regressor=_vp, measurements=_vp, steps=_i32, state=_vp, covariance=_vp, batch=_i64, stream=_vp),
    "blf_contact_rls_advance": _sig(handle=_vp, lambda_=_f64, meas_cov=_vp, shared_cov=_i32, geometry=_vp,
        shared_geometry=_i32, twist=_vp, pose=_vp, null_pose=_vp, wrench=_vp, steps=_i32, state=_vp,
        covariance=_vp, batch=_i64, stream=_vp),
    "blf_swing_foot_eval": _sig(handle=_vp, params=_P(SwingFootParams), contact_pose=_vp, contact_time=_vp,
        ncontacts=_vp, batch=_i64, tq=_vp, nq=_i32, pose=_vp, twist=_vp, accel=_vp, contact_idx=_vp,
        in_contact=_vp, stream=_vp),
    "blf_so3_eval": _sig(handle=_vp, R0=_vp, R1=_vp, duration=_vp, batch=_i64, tq=_vp, nq=_i32, rot=_vp,
        omega=_vp, alpha=_vp, stream=_vp),
    "blf_fb_ik_solve": _sig(**_FB, tasks=_P(IkTasks), batch=_i64, nu=_vp, status=_vp, stream=_vp),
    "blf_fb_ik_integrate": _sig(**_FB, tasks=_P(IkTasks), batch=_i64, steps=_i32, dT=_f64, nu=_vp, status=_vp,
        stream=_vp),
    "blf_fb_ik_solve_hard": _sig(**_FB, tasks=_P(IkTasks), hard=_P(IkHard), batch=_i64, nu=_vp, status=_vp,
        stream=_vp),
    "blf_fb_ik_integrate_hard": _sig(**_FB, tasks=_P(IkTasks), hard=_P(IkHard), batch=_i64, steps=_i32, dT=_f64,
        nu=_vp, status=_vp, stream=_vp),
    "blf_fb_ik_solve_limits": _sig(**_FB, tasks=_P(IkTasks), hard=_P(IkHard), limits=_P(IkLimits), batch=_i64,
        nu=_vp, status=_vp, iters=_vp, active=_vp, stream=_vp),
    "blf_fb_ik_integrate_limits": _sig(**_FB, tasks=_P(IkTasks), hard=_P(IkHard), limits=_P(IkLimits),
        batch=_i64, steps=_i32, dT=_f64, nu=_vp, status=_vp, iters=_vp, active=_vp, stream=_vp),
    "blf_fb_ik_track": _sig(**_FB, tasks=_P(IkTasks), hard=_P(IkHard), limits=_P(IkLimits),
        schedule=_P(IkSchedule), batch=_i64, dT=_f64, joint_traj=_vp, base_traj=_vp, nu_traj=_vp, status=_vp,
        fail_step=_vp, iters=_vp, active=_vp, stream=_vp),
    "blf_fbd_euler_integrate_impedance_traj": _sig(**_FB, impedance=_P(JointImpedanceTraj),
        contacts=_P(FbContacts), mass_reg=_vp, batch=_i64, **_TIMES, stream=_vp),
    "blf_dcm_com_reference": _sig(handle=_vp, xi0=_vp, vrp=_vp, vrp_stride=_i64, omega0=_vp, omega0_stride=_i64,
        z_ref=_vp, c_ref=_vp, steps=_i32, dT=_f64, batch=_i64, com_pos=_vp, com_vel=_vp, xi_end=_vp,
        stream=_vp),
    "blf_fb_inverse_dynamics": _sig(**_FB, joint_acc=_vp, base_acc=_vp, contacts=_P(FbContacts), batch=_i64,
        joint_torque=_vp, base_acc_out=_vp, base_wrench=_vp, status=_vp, reserved=_i32, stream=_vp),
    "blf_fbd_euler_integrate_computed_torque_traj": _sig(**_FB, law=_P(ComputedTorqueTraj),
        contacts=_P(FbContacts), mass_reg=_vp, batch=_i64, **_TIMES, stream=_vp),
    "blf_schmitt_trigger_advance": _sig(handle=_vp, ncontacts=_i32, params=_vp, shared_params=_i32, time=_vp,
        value=_vp, steps=_i32, state=_vp, timers=_vp, state_out=_vp, batch=_i64, stream=_vp),
    "blf_legged_odometry_advance": _sig(handle=_vp, fb_model=_P(FbModel), ncontacts=_i32, frames=_vp, params=_vp,
        shared_params=_i32, time=_vp, joint_pos=_vp, joint_vel=_vp, normal_force=_vp, steps=_i32, trig_state=_vp,
        trig_timers=_vp, fixed_frame=_vp, fixed_pose=_vp, base_pos=_vp, base_rot=_vp, base_vel=_vp,
        contact_out=_vp, fixed_out=_vp, status=_vp, batch=_i64, reserved=_i32, stream=_vp),
}
EXPORTED = list(SIGNATURES)


_LIB = None


def lib():
    """Load lib/libblf.so (raises if it is absent: there is no fallback path)."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: run __graft_entry__.build() (make -C "
                              f"bipedal-locomotion-framework_amd)")
        # One HIP runtime per process: libblf.so needs libamdhip64.so.7, and torch ships its own
        # copy.  Loaded after torch, libblf.so binds to torch's (same soname) and shares its
        # device memory and streams; loaded first, the process would hold two runtimes and the
        # one that initialises second sees no device.  So torch, when installed, is loaded first.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = ctypes.CDLL(LIB_PATH)
        for name, (restype, args) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, [t for _, t in args]
        _LIB = L
    return _LIB


def set_qp_launch_mode(fuse_stage2=-1, single_kernel=-1):
    """blf_set_qp_launch_mode: the QP kernel routing for A/B and parity tests (-1: unchanged).
    Returns nothing; the defaults are the product's (fuse_stage2 = 1, single_kernel = 0)."""
    _check(lib().blf_set_qp_launch_mode(int(fuse_stage2), int(single_kernel)))


def _check(code):
    if code != BLF_OK:
        raise BlfError(code, lib().blf_last_error().decode())


def last_error():
    return lib().blf_last_error().decode()


def version():
    return lib().blf_version().decode()


def source_hash():
    """The Makefile's SRC_HASH of the kernel / C-ABI sources in this tree (sha256 of csrc/*.hip and
    csrc/*.h in sorted path order, then include/blf/blf_c.h; first 16 hex digits), or None when
    the sources are not present."""
    import glob
    import hashlib
    pkg = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    names = sorted(os.path.relpath(f, pkg) for f in glob.glob(os.path.join(pkg, "csrc", "*.hip")) +
                   glob.glob(os.path.join(pkg, "csrc", "*.h")))
    hdr = os.path.join(os.path.dirname(pkg), "include", "blf", "blf_c.h")
    if not names or not os.path.exists(hdr):
        return None
    h = hashlib.sha256()
    for n in names:
        with open(os.path.join(pkg, n), "rb") as f:
            h.update(f.read())
    with open(hdr, "rb") as f:
        h.update(f.read())
    return h.hexdigest()[:16]


def build_provenance():
    """Which library this process loaded and whether it was built from the sources in this tree:
    {"lib": path, "lib_src_hash": hash in blf_version(), "tree_src_hash": source_hash(),
    "matches": bool}."""
    v = version()
    lib_hash = v.rsplit(" src ", 1)[1] if " src " in v else None
    tree = source_hash()
    return {"lib": LIB_PATH, "lib_src_hash": lib_hash, "tree_src_hash": tree,
            "matches": lib_hash is not None and lib_hash == tree}


def default_params(horizon, **kw):
    p = DcmMpcParams()
    lib().blf_dcm_mpc_default_params(ctypes.byref(p), horizon)
    for k, v in kw.items():
        if k in ("w_xi", "w_vrp", "w_terminal"):
            arr = getattr(p, k)
            arr[0], arr[1] = (v, v) if isinstance(v, (int, float)) else (v[0], v[1])
        else:
            setattr(p, k, v)
    return p


def flops_per_iter(horizon, active_facets):
    return lib().blf_dcm_mpc_flops_per_iter(horizon, active_facets)


# ---------------------------------------------------------------------------------------------
# device-side helpers (torch as plumbing)
# ---------------------------------------------------------------------------------------------
def _torch():
    import torch
    return torch


def _ptr(t, dtype, shape=None, name="tensor"):
    torch = _torch()
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch tensor")
    if t.device.type != "cuda":
        raise ValueError(f"{name} must be a device (cuda/hip) tensor, got {t.device}")
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} has shape {tuple(t.shape)}, expected {tuple(shape)}")
    return _vp(t.data_ptr())


def _stream(stream=None):
    torch = _torch()
    s = stream if stream is not None else torch.cuda.current_stream()
    return _vp(s.cuda_stream)


def _ref(x):
    """byref(x), or None (a null pointer) for None."""
    return ctypes.byref(x) if x is not None else None


def _upload(a, dtype, dev):
    """A host array as a contiguous tensor on the device."""
    return _torch().as_tensor(a, dtype=dtype).contiguous().to(dev)


def _on_device(a, dtype, dev):
    """A tensor as it stands (no copy; _ptr checks it later), a host array uploaded."""
    return a if isinstance(a, _torch().Tensor) else _upload(a, dtype, dev)


class _Held:
    """A C struct (.c) with the tensors it points into (.t), kept alive together, and the sizes its builder
    records for the calls that take it (.n, .batch, .nse3, .steps, .tau_last)."""

    def __init__(self, c, t, **sizes):
        self.c, self.t = c, t
        self.__dict__.update(sizes)


# A spec below is {name: (shape, torch dtype)} in the order of the C struct's members or the call's arguments.
def _new(spec, dev):
    torch = _torch()
    return {k: torch.empty(shape, dtype=dt, device=dev) for k, (shape, dt) in spec.items()}


def _ptrs(tensors, spec, prefix=""):
    return [_ptr(tensors[k], dt, shape, prefix + k) for k, (shape, dt) in spec.items()]


def _out(given, shape, dtype, dev, name, zero=False, optional=True):
    """An output argument as (tensor, pointer).  None: allocated here (torch.zeros if `zero`, else
    torch.empty); a tensor: checked and used; False, for an `optional` output: not requested, (None, None)."""
    torch = _torch()
    if given is False and optional:
        return None, None
    if given is None:
        given = (torch.zeros if zero else torch.empty)(shape, dtype=dtype, device=dev)
    return given, _ptr(given, dtype, shape, name)


def _outs(spec, given, dev, zero=False):
    """_out over a spec: ({name: tensor or None}, [pointer or None])."""
    pairs = {k: _out(given.get(k), shape, dt, dev, k, zero) for k, (shape, dt) in spec.items()}
    return {k: t for k, (t, _) in pairs.items()}, [p for _, p in pairs.values()]


def _requested(spec, outputs, out, dev):
    """The `outputs=` form: the names in `outputs` are computed (into out[name] when `out` holds it), the
    others are not requested.  Returns ({requested name: tensor}, [pointer or None for every name])."""
    res, ptrs = _outs(spec, {k: (out or {}).get(k) if k in outputs else False for k in spec}, dev)
    return {k: t for k, t in res.items() if k in outputs}, ptrs


def _window_spec(B, N, M):
    """A window's arrays in blf_dcm_mpc_window's order, which is blf_dcm_mpc_problem's after xi_init."""
    f64, i32 = _torch().float64, _torch().int32
    return dict(omega=((B, N), f64), xi_ref=((B, N + 1, 2), f64), vrp_ref=((B, N, 2), f64),
                A=((B, N, M, 2), f64), b=((B, N, M), f64), nfacets=((B, N), i32))


def _solution_spec(B, N):
    f64, i32 = _torch().float64, _torch().int32
    return dict(xi=((B, N + 1, 2), f64), vrp=((B, N, 2), f64), status=((B,), i32), iters=((B,), i32),
                polished=((B,), i32), passes=((B,), i32))


def _problem_struct(prob, B, N, M):
    return DcmMpcProblem(_ptr(prob["xi_init"], _torch().float64, (B, 2), "xi_init"),
                         *_ptrs(prob, _window_spec(B, N, M)))


def _solution_struct(out, B, N):
    """blf_dcm_mpc_solution over out; polished and passes are optional (absent: NULL, not written)."""
    spec = {k: v for k, v in _solution_spec(B, N).items() if k in out or k not in ("polished", "passes")}
    return DcmMpcSolution(**dict(zip(spec, _ptrs(out, spec))))


def _lambda_out(out, wanted, B, N, M):
    """The lambda_out pointer: out["lam"] [B,N,M] (allocated when absent), or None when not wanted."""
    torch = _torch()
    if not wanted:
        return None
    if "lam" not in out:
        out["lam"] = torch.empty((B, N, M), dtype=torch.float64, device=out["xi"].device)
    return _ptr(out["lam"], torch.float64, (B, N, M), "lam")


def _warm_start(warm, B, N, M):
    """blf_dcm_mpc_warm_start from a dict: vrp [B,N,2], lam [B,N,M], shift, floor and optionally
    status [B] int32 (the previous solve's statuses: problems with status != 0 start cold)."""
    torch = _torch()
    st = warm.get("status")
    return DcmMpcWarmStart(_ptr(warm["vrp"], torch.float64, (B, N, 2), "warm vrp"),
                           _ptr(warm["lam"], torch.float64, (B, N, M), "warm lam"),
                           int(warm.get("shift", 1)), 0, float(warm.get("floor", 1e-2)),
                           _ptr(st, torch.int32, (B,), "warm status") if st is not None else None)


def _phase_table_struct(table):
    """(blf_phase_table, B, M) of a phase table dict (Handle.phase_table() or the same keys)."""
    f64, i32 = _torch().float64, _torch().int32
    B, P = table["phase_begin"].shape
    M = table["phase_b"].shape[2]
    spec = dict(nphases=((B,), i32), phase_begin=((B, P), f64), phase_end=((B, P), f64),
                phase_A=((B, P, M, 2), f64), phase_b=((B, P, M), f64), phase_nf=((B, P), i32),
                phase_ref=((B, P, 2), f64))
    return PhaseTable(P, M, *_ptrs(table, spec)), B, M


class Handle:
    """RAII wrapper of blf_handle (one per device per thread)."""

    def __init__(self, device=0):
        self._h = _vp()
        _check(lib().blf_create(ctypes.byref(self._h), device))
        self.device = device

    def close(self):
        if self._h:
            lib().blf_destroy(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def ptr(self):
        return self._h

    # --- ForwardEuler<LinearTimeInvariantSystem>::integrate, batched, in place on x ---
    def lti_euler_integrate(self, A, Bm, u, x, t0, t1, dT, shared=False, stream=None):
        torch = _torch()
        n = x.shape[-1]
        m = u.shape[-1]
        batch = x.shape[0]
        ashape = (n, n) if shared else (batch, n, n)
        bshape = (n, m) if shared else (batch, n, m)
        _check(lib().blf_lti_euler_integrate(
            self._h, n, m, _ptr(A, torch.float64, ashape, "A"), _ptr(Bm, torch.float64, bshape, "B"),
            1 if shared else 0, _ptr(u, torch.float64, (batch, m), "u"),
            _ptr(x, torch.float64, (batch, n), "x"), batch, t0, t1, dT, _stream(stream)))
        return x

    def lti_dynamics(self, A, Bm, u, x, shared=False, stream=None):
        torch = _torch()
        batch, n = x.shape
        m = u.shape[-1]
        ashape = (n, n) if shared else (batch, n, n)
        bshape = (n, m) if shared else (batch, n, m)
        dx = torch.empty_like(x)
        _check(lib().blf_lti_dynamics(
            self._h, n, m, _ptr(A, torch.float64, ashape, "A"), _ptr(Bm, torch.float64, bshape, "B"),
            1 if shared else 0, _ptr(u, torch.float64, (batch, m), "u"),
            _ptr(x, torch.float64, (batch, n), "x"), _ptr(dx, torch.float64, (batch, n), "dx"),
            batch, _stream(stream)))
        return dx

    def dcm_euler_rollout(self, xi0, omega, vrp, dt, out=None, stream=None):
        torch = _torch()
        B, N = omega.shape
        if out is None:
            out = torch.empty((B, N + 1, 2), dtype=torch.float64, device=omega.device)
        _check(lib().blf_dcm_euler_rollout(
            self._h, _ptr(xi0, torch.float64, (B, 2), "xi0"), _ptr(omega, torch.float64, (B, N), "omega"),
            _ptr(vrp, torch.float64, (B, N, 2), "vrp"), N, dt,
            _ptr(out, torch.float64, (B, N + 1, 2), "xi_out"), B, _stream(stream)))
        return out

    def _hull_hrep(self, fn, dim, D, pts, npts, max_facets, out, stream):
        """blf_hull2d_hrep / blf_hull3d_hrep (dim = ()) and blf_hullnd_hrep (dim = (D,)) on pts [B, P, D]."""
        torch = _torch()
        B, P = pts.shape[0], pts.shape[1]
        spec = dict(A=((B, max_facets, D), torch.float64), b=((B, max_facets), torch.float64),
                    nfacets=((B,), torch.int32))
        A, b, nf = out if out is not None else _new(spec, pts.device).values()
        _check(fn(self._h, *dim, _ptr(pts, torch.float64, (B, P, D), "pts"), _ptr(npts, torch.int32, (B,), "npts"),
                  P, max_facets, B, *_ptrs(dict(A=A, b=b, nfacets=nf), spec), _stream(stream)))
        return A, b, nf

    def hull2d_hrep(self, pts, npts, max_facets=8, out=None, stream=None):
        return self._hull_hrep(lib().blf_hull2d_hrep, (), 2, pts, npts, max_facets, out, stream)

    def hull3d_hrep(self, pts, npts, max_facets=32, out=None, stream=None):
        """blf_hull3d_hrep: pts [B, P, 3], npts [B] -> A [B, max_facets, 3], b, nfacets."""
        return self._hull_hrep(lib().blf_hull3d_hrep, (), 3, pts, npts, max_facets, out, stream)

    def hullnd_hrep(self, pts, npts, max_facets=64, out=None, stream=None):
        """blf_hullnd_hrep: pts [B, P, dim], npts [B] -> A [B, max_facets, dim], b, nfacets."""
        _, _, D = pts.shape
        return self._hull_hrep(lib().blf_hullnd_hrep, (D,), D, pts, npts, max_facets, out, stream)

    def _contains(self, fn, dim, B, M, D, A, b, nf, query, stream):
        """blf_hull2d_contains (dim = ()) and blf_halfspace_contains (dim = (D,))."""
        torch = _torch()
        inside = torch.empty((B,), dtype=torch.int32, device=A.device)
        _check(fn(self._h, _ptr(A, torch.float64, (B, M, D), "A"), _ptr(b, torch.float64, (B, M), "b"),
                  _ptr(nf, torch.int32, (B,), "nfacets"), *dim, M, _ptr(query, torch.float64, (B, D), "query"),
                  B, _ptr(inside, torch.int32, (B,), "inside"), _stream(stream)))
        return inside

    def hull2d_contains(self, A, b, nf, query, stream=None):
        B, M = b.shape
        return self._contains(lib().blf_hull2d_contains, (), B, M, 2, A, b, nf, query, stream)

    def halfspace_contains(self, A, b, nf, query, stream=None):
        """blf_halfspace_contains: A [B, M, dim], b [B, M], nf [B], query [B, dim] -> inside [B]."""
        B, M, D = A.shape
        return self._contains(lib().blf_halfspace_contains, (D,), B, M, D, A, b, nf, query, stream)

    def quintic_fit(self, knots_t, knots_pva, stream=None):
        torch = _torch()
        S, K1 = knots_t.shape
        D = knots_pva.shape[-1]
        coeffs = torch.empty((S, K1 - 1, D, 6), dtype=torch.float64, device=knots_t.device)
        _check(lib().blf_quintic_fit(
            self._h, _ptr(knots_t, torch.float64, (S, K1), "knots_t"),
            _ptr(knots_pva, torch.float64, (S, K1, 3, D), "knots_pva"), K1, D, S,
            _ptr(coeffs, torch.float64, (S, K1 - 1, D, 6), "coeffs"), _stream(stream)))
        return coeffs

    def quintic_eval(self, knots_t, coeffs, tq, stream=None):
        torch = _torch()
        S, K1 = knots_t.shape
        D = coeffs.shape[2]
        Q = tq.shape[1]
        pva = torch.empty((S, Q, 3, D), dtype=torch.float64, device=tq.device)
        idx = torch.empty((S, Q), dtype=torch.int32, device=tq.device)
        _check(lib().blf_quintic_eval(
            self._h, _ptr(knots_t, torch.float64, (S, K1), "knots_t"),
            _ptr(coeffs, torch.float64, (S, K1 - 1, D, 6), "coeffs"), K1, D, S,
            _ptr(tq, torch.float64, (S, Q), "tq"), Q, _ptr(pva, torch.float64, (S, Q, 3, D), "pva"),
            _ptr(idx, torch.int32, (S, Q), "knot_idx"), _stream(stream)))
        return pva, idx

    def dcm_mpc_solve(self, prob, params=None, out=None, stream=None, warm=None,
                      lambda_out=False):
        """prob: dict of device tensors xi_init [B,2], omega [B,N], xi_ref [B,N+1,2],
        vrp_ref [B,N,2], A [B,N,M,2], b [B,N,M], nfacets [B,N] (int32).
        warm: None (cold start) or dict(vrp [B,N,2], lam [B,N,M], shift, floor)
        (blf_dcm_mpc_solve_warm); lambda_out: also return the final multipliers out["lam"].
        out["polished"] [B] says which solutions are the certified active-set polish; out["passes"]
        [B] how many drop/add passes the active-set kernels ran for each."""
        B, N = prob["omega"].shape
        M = prob["b"].shape[2]
        p = params if params is not None else default_params(N, max_facets=M)
        if p.horizon != N or p.max_facets != M:
            raise ValueError("params.horizon / max_facets do not match the problem arrays")
        if out is None:
            out = _new(_solution_spec(B, N), prob["omega"].device)
        pb = _problem_struct(prob, B, N, M)
        so = _solution_struct(out, B, N)
        ws = _warm_start(warm, B, N, M) if warm is not None else None
        lam = _lambda_out(out, lambda_out, B, N, M)
        if ws is None and lam is None:
            _check(lib().blf_dcm_mpc_solve(self._h, _ref(p), _ref(pb), B, _ref(so), _stream(stream)))
        else:
            _check(lib().blf_dcm_mpc_solve_warm(self._h, _ref(p), _ref(pb), _ref(ws), B, _ref(so), lam,
                                                _stream(stream)))
        return out

    def prepare_dcm_mpc_solve(self, prob, params, out, stream=None):
        """The cold blf_dcm_mpc_solve with its argument structs built once: returns f(), which
        makes just the C-ABI call (what a C++ caller holding its device buffers pays, e.g. the
        TimeVaryingDCMPlanner adapter), and the raw stream handle.  The tensors must outlive f."""
        torch = _torch()
        self.dcm_mpc_solve(prob, params, out=out, stream=stream)   # validates every argument
        B, N = prob["omega"].shape
        pb = _problem_struct(prob, B, N, prob["b"].shape[2])
        so = _solution_struct(out, B, N)
        s = _stream(stream)
        fn, h, pp, ppb, pso = lib().blf_dcm_mpc_solve, self._h, ctypes.byref(params), ctypes.byref(pb), ctypes.byref(so)
        keep = (pb, so, params, prob, out, torch)

        def f():
            st = fn(h, pp, ppb, B, pso, s)
            if st != 0:
                _check(st)
            return keep
        return f, s

    def phase_table(self, nphases, begin, end, corners, ncorners, max_facets=8, ref=None,
                    stream=None):
        """Device phase table: the H-rep of every phase's support polygon (blf_hull2d_hrep over
        corners [B,P,C,2] / ncorners [B,P]) plus the phases' times and centroid references.
        ref [B,P,2]: the phases' reference points (default: the centroid of the corners)."""
        torch = _torch()
        B, P, C, _ = corners.shape
        A, b, nf = self.hull2d_hrep(corners.reshape(B * P, C, 2).contiguous(),
                                    ncorners.reshape(B * P).contiguous(), max_facets,
                                    stream=stream)
        if ref is None:
            cnt = ncorners.to(torch.float64).clamp(min=1)[..., None]
            ref = (corners.sum(dim=2) / cnt).contiguous()
        return dict(nphases=nphases, phase_begin=begin, phase_end=end,
                    phase_A=A.view(B, P, max_facets, 2), phase_b=b.view(B, P, max_facets),
                    phase_nf=nf.view(B, P), phase_ref=ref)

    def dcm_phase_expand(self, table, start, dt, horizon, out=None, stream=None):
        """blf_dcm_phase_expand: window arrays (A, b, nfacets, xi_ref, vrp_ref) of knots
        (start + k) dt, k = 0..horizon, from a phase table (phase_table() or the same keys)."""
        tb, B, M = _phase_table_struct(table)
        N = horizon
        window = _window_spec(B, N, M)
        spec = {k: window[k] for k in ("A", "b", "nfacets", "xi_ref", "vrp_ref")}   # the call's order
        if out is None:
            out = _new(spec, table["phase_begin"].device)
        _check(lib().blf_dcm_phase_expand(self._h, _ref(tb), int(start), float(dt), N, B, *_ptrs(out, spec),
                                          _stream(stream)))
        return out

    def dcm_mpc_solve_phased(self, table, start, xi_init, omega, params=None, warm=None,
                             out=None, window=None, lambda_out=False, stream=None):
        """blf_dcm_mpc_solve_phased: dcm_phase_expand(table, start, params.dt, N) followed by
        dcm_mpc_solve on that window, fused (same results bit for bit, N <= 128).
        omega [B, N] or a row-strided view [B, N] of a longer [B, L] array (stride(1) == 1).
        window: scratch dict (omega, xi_ref, vrp_ref, A, b, nfacets) of the window's shapes, kept
        in out["window"] (allocated once when absent)."""
        torch = _torch()
        B, N = omega.shape
        M = table["phase_b"].shape[2]
        p = params if params is not None else default_params(N, max_facets=M)
        if p.horizon != N or p.max_facets != M:
            raise ValueError("params.horizon / max_facets do not match omega / the phase table")
        if omega.device.type != "cuda" or omega.dtype != torch.float64 or omega.stride(1) != 1:
            raise ValueError("omega must be a float64 device tensor with unit column stride")
        ostride = omega.stride(0) if B > 1 else N
        if out is None:
            out = _new(_solution_spec(B, N), omega.device)
        if window is None:
            window = out.get("window")
        if window is None:
            window = out["window"] = _new(_window_spec(B, N, M), omega.device)
        win = DcmMpcWindow(*_ptrs(window, _window_spec(B, N, M), "window "))
        tb = _phase_table_struct(table)[0]
        so = _solution_struct(out, B, N)
        ws = _warm_start(warm, B, N, M) if warm is not None else None
        lam = _lambda_out(out, lambda_out, B, N, M)
        _check(lib().blf_dcm_mpc_solve_phased(
            self._h, _ref(p), _ref(tb), int(start), _ptr(xi_init, torch.float64, (B, 2), "xi_init"),
            _vp(omega.data_ptr()), ostride, _ref(ws), B, _ref(win), _ref(so), lam, _stream(stream)))
        return out

    # --- C3 pipeline: corner sets -> polygons (device hull) -> QP arrays ---
    def assemble_constraints(self, corners, ncorners, max_facets=8, stream=None):
        """corners [B, N+1, P, 2], ncorners [B, N+1] (device) -> A [B,N,M,2], b [B,N,M],
        nfacets [B,N] for knots 0..N-1 via blf_hull2d_hrep."""
        B, N1, P, _ = corners.shape
        N = N1 - 1
        pts = corners[:, :N].reshape(B * N, P, 2).contiguous()
        npts = ncorners[:, :N].reshape(B * N).contiguous()
        A, b, nf = self.hull2d_hrep(pts, npts, max_facets, stream=stream)
        return A.view(B, N, max_facets, 2), b.view(B, N, max_facets), nf.view(B, N)

    # ---- config 5: contact model and floating-base kinematics ---------------------------------
    def _contact_inputs(self, params, twist, pose, null_pose):
        torch = _torch()
        B = twist.shape[0]
        shared = params.dim() == 1
        pp = _ptr(params, torch.float64, (4,) if shared else (B, 4), "params")
        return (B, shared, pp, _ptr(twist, torch.float64, (B, 6), "twist"),
                _ptr(pose, torch.float64, (B, 12), "pose"),
                _ptr(null_pose, torch.float64, (B, 12), "null_pose"))

    def contact_model_eval(self, params, twist, pose, null_pose,
                           outputs=("wrench", "autonomous", "control", "regressor"), stream=None):
        """ContinuousContactModel for a batch: params [B,4] or [4] (L, W, k, b), twist [B,6],
        pose / null_pose [B,12] = (p, R row-major).  Returns the requested outputs."""
        f64 = _torch().float64
        B, shared, pp, tw, ps, ns = self._contact_inputs(params, twist, pose, null_pose)
        spec = dict(wrench=((B, 6), f64), autonomous=((B, 6), f64), control=((B, 6, 6), f64),
                    regressor=((B, 6, 2), f64))
        out, ptrs = _requested(spec, outputs, None, twist.device)
        _check(lib().blf_contact_model_eval(self._h, pp, 1 if shared else 0, tw, ps, ns, B,
                                            *ptrs, _stream(stream)))
        return out

    def contact_point_wrench(self, params, twist, pose, null_pose, points, stream=None):
        """Force / torque at points [B,Q,2] of each contact surface -> ([B,Q,3], [B,Q,3])."""
        torch = _torch()
        B, shared, pp, tw, ps, ns = self._contact_inputs(params, twist, pose, null_pose)
        Q = points.shape[1]
        f = torch.empty((B, Q, 3), dtype=torch.float64, device=twist.device)
        t = torch.empty_like(f)
        _check(lib().blf_contact_point_wrench(
            self._h, pp, 1 if shared else 0, tw, ps, ns, B,
            _ptr(points, torch.float64, (B, Q, 2), "points"), Q, ctypes.c_void_p(f.data_ptr()),
            ctypes.c_void_p(t.data_ptr()), _stream(stream)))
        return f, t

    # ---- Estimators::RecursiveLeastSquare, batched, in place on state / covariance ------------
    def rls_advance(self, regressor, measurements, state, covariance, meas_cov, lam=1.0,
                    stream=None):
        """T steps of B recursive-least-squares filters (blf_rls_advance): regressor [T,B,m,n],
        measurements [T,B,m] (or without the T axis: one step), state [B,n], covariance [B,n,n],
        meas_cov [m] (shared) or [B,m].  Updates state and covariance in place, returns them."""
        torch = _torch()
        B, n = state.shape
        if regressor.dim() == 3:
            regressor, measurements = regressor.unsqueeze(0), measurements.unsqueeze(0)
        T, m = regressor.shape[0], regressor.shape[2]
        shared = meas_cov.dim() == 1
        _check(lib().blf_rls_advance(
            self._h, n, m, float(lam),
            _ptr(meas_cov, torch.float64, (m,) if shared else (B, m), "meas_cov"),
            1 if shared else 0, _ptr(regressor, torch.float64, (T, B, m, n), "regressor"),
            _ptr(measurements, torch.float64, (T, B, m), "measurements"), T,
            _ptr(state, torch.float64, (B, n), "state"),
            _ptr(covariance, torch.float64, (B, n, n), "covariance"), B, _stream(stream)))
        return state, covariance

    def contact_rls_advance(self, geometry, twist, pose, null_pose, wrench, state, covariance,
                            meas_cov, lam=1.0, stream=None):
        """T identification steps of B contacts' (spring, damper) from measured wrenches
        (blf_contact_rls_advance): geometry [2] or [B,2] = (length, width), twist [T,B,6], pose
        [T,B,12], wrench [T,B,6] (or without the T axis), null_pose [B,12], state [B,2], covariance
        [B,2,2], meas_cov [6] or [B,6].  Updates state and covariance in place, returns them."""
        torch = _torch()
        B = state.shape[0]
        if twist.dim() == 2:
            twist, pose, wrench = twist.unsqueeze(0), pose.unsqueeze(0), wrench.unsqueeze(0)
        T = twist.shape[0]
        shared_cov = meas_cov.dim() == 1
        shared_geo = geometry.dim() == 1
        _check(lib().blf_contact_rls_advance(
            self._h, float(lam),
            _ptr(meas_cov, torch.float64, (6,) if shared_cov else (B, 6), "meas_cov"),
            1 if shared_cov else 0,
            _ptr(geometry, torch.float64, (2,) if shared_geo else (B, 2), "geometry"),
            1 if shared_geo else 0, _ptr(twist, torch.float64, (T, B, 6), "twist"),
            _ptr(pose, torch.float64, (T, B, 12), "pose"),
            _ptr(null_pose, torch.float64, (B, 12), "null_pose"),
            _ptr(wrench, torch.float64, (T, B, 6), "wrench"), T,
            _ptr(state, torch.float64, (B, 2), "state"),
            _ptr(covariance, torch.float64, (B, 2, 2), "covariance"), B, _stream(stream)))
        return state, covariance

    # ---- Contacts::SchmittTriggerDetector / Estimators::LeggedOdometry, batched (section 13) ----
    @staticmethod
    def _trigger_params(params, K):
        """The trigger parameters as the HOST array the library reads: (array kept alive, shared, pointer)."""
        import numpy as np
        if isinstance(params, _torch().Tensor):
            params = params.detach().cpu().numpy()
        p = np.ascontiguousarray(params, dtype=np.float64)
        if p.shape not in ((4,), (K, 4)):
            raise ValueError(f"params has shape {p.shape}, expected (4,) or ({K}, 4)")
        return p, 1 if p.ndim == 1 else 0, _vp(p.ctypes.data)

    def schmitt_trigger_advance(self, params, time, value, state, timers, state_out=None, stream=None):
        """T samples of B x K Schmitt triggers (blf_schmitt_trigger_advance): params [4] (shared) or [K,4] =
        (on_threshold, off_threshold, switch_on_after, switch_off_after), a host array; time [T], value
        [T,B,K] (or [B,K] with time a scalar tensor [1]: one sample), state [B,K] int32, timers [B,K,2].
        Updates state and timers in place; returns (state, timers, state_out [T,B,K] int32, or None when
        state_out=False)."""
        torch = _torch()
        if value.dim() == 2:
            value = value.unsqueeze(0)
        T, B, K = value.shape
        p, shared, pp = self._trigger_params(params, K)
        out, op = _out(state_out, (T, B, K), torch.int32, value.device, "state_out")
        _check(lib().blf_schmitt_trigger_advance(
            self._h, K, pp, shared, _ptr(time, torch.float64, (T,), "time"),
            _ptr(value, torch.float64, (T, B, K), "value"), T, _ptr(state, torch.int32, (B, K), "state"),
            _ptr(timers, torch.float64, (B, K, 2), "timers"), op, B, _stream(stream)))
        return state, timers, out

    ODOMETRY_OUTPUTS = ("base_pos", "base_rot", "base_vel", "contact_out", "fixed_out", "status")

    def legged_odometry(self, dm, frames, params, time, joint_pos, joint_vel, normal_force, est,
                        outputs=ODOMETRY_OUTPUTS, out=None, stream=None):
        """T steps of B legged-odometry estimators in one launch (blf_legged_odometry_advance).  dm: fb_model's
        result; frames [K] int32 device tensor (the model's frame of each contact slot); params as in
        schmitt_trigger_advance; time [T], joint_pos [T,B,n], joint_vel [T,B,n] or None (zero), normal_force
        [T,B,K].  est: the estimator state, updated in place: dict(trig_state [B,K] int32, trig_timers [B,K,2],
        fixed_frame [B] int32, fixed_pose [B,12]) -- blf.robot.odometry_init builds it.  Returns a dict of the
        requested `outputs` (into out[name] where given): base_pos [T,B,3], base_rot [T,B,3,3], base_vel
        [T,B,6], contact_out [T,B,K] int32, fixed_out [T,B] int32, status [B] int32."""
        torch = _torch()
        T, B, n = joint_pos.shape
        if n != dm.n:
            raise ValueError(f"joint_pos has {n} joints, the model {dm.n}")
        K = frames.shape[0]
        dev = joint_pos.device
        p, shared, pp = self._trigger_params(params, K)
        i32, f64 = torch.int32, torch.float64
        spec = dict(base_pos=((T, B, 3), f64), base_rot=((T, B, 3, 3), f64), base_vel=((T, B, 6), f64),
                    contact_out=((T, B, K), i32), fixed_out=((T, B), i32), status=((B,), i32))
        unknown = set(outputs) - set(spec)
        if unknown:
            raise ValueError(f"unknown outputs {sorted(unknown)}")
        res, optrs = _requested(spec, outputs, out, dev)
        state_spec = dict(trig_state=((B, K), i32), trig_timers=((B, K, 2), f64), fixed_frame=((B,), i32),
                          fixed_pose=((B, 12), f64))
        _check(lib().blf_legged_odometry_advance(
            self._h, _ref(dm.c), K, _ptr(frames, i32, (K,), "frames"), pp, shared, _ptr(time, f64, (T,), "time"),
            _ptr(joint_pos, f64, (T, B, n), "joint_pos"),
            _ptr(joint_vel, f64, (T, B, n), "joint_vel") if joint_vel is not None else None,
            _ptr(normal_force, f64, (T, B, K), "normal_force"), T, *_ptrs(est, state_spec, "est."), *optrs, B, 0,
            _stream(stream)))
        return res

    # ---- Planners::SwingFootPlanner / SO3Planner, batched ------------------------------------
    def swing_foot_eval(self, contact_pose, contact_time, ncontacts, tq, step_height=0.05,
                        apex_ratio=0.5, landing_velocity=0.0, landing_acceleration=0.0,
                        outputs=SWING_OUTPUTS, out=None, stream=None):
        """SE(3) swing-foot trajectories (blf_swing_foot_eval): contact_pose [L,C,12], contact_time
        [L,C,2] = (activation, deactivation), ncontacts [L] int32, tq [L,Q].  Returns a dict of the
        requested outputs: pose [L,Q,12], twist / accel [L,Q,6], contact_idx / in_contact [L,Q]
        int32 (out: tensors to write into instead of new ones)."""
        torch = _torch()
        L, C = contact_pose.shape[0], contact_pose.shape[1]
        Q = tq.shape[1]
        prm = SwingFootParams(C, 0, float(step_height), float(apex_ratio), float(landing_velocity),
                              float(landing_acceleration))
        spec = dict(pose=((L, Q, 12), torch.float64), twist=((L, Q, 6), torch.float64),
                    accel=((L, Q, 6), torch.float64), contact_idx=((L, Q), torch.int32),
                    in_contact=((L, Q), torch.int32))
        res, ptrs = _requested(spec, outputs, out, tq.device)
        _check(lib().blf_swing_foot_eval(
            self._h, ctypes.byref(prm), _ptr(contact_pose, torch.float64, (L, C, 12), "contact_pose"),
            _ptr(contact_time, torch.float64, (L, C, 2), "contact_time"),
            _ptr(ncontacts, torch.int32, (L,), "ncontacts"), L, _ptr(tq, torch.float64, (L, Q), "tq"),
            Q, *ptrs, _stream(stream)))
        return res

    def so3_eval(self, R0, R1, duration, tq, outputs=SO3_OUTPUTS, out=None, stream=None):
        """Minimum-jerk SO(3) trajectories (blf_so3_eval): R0, R1 [S,3,3] or [S,9], duration [S],
        tq [S,Q] (clamped to [0, duration]).  Returns a dict of rot [S,Q,9], omega, alpha [S,Q,3]."""
        torch = _torch()
        S, Q = tq.shape
        R0, R1 = R0.reshape(S, 9), R1.reshape(S, 9)
        spec = dict(rot=((S, Q, 9), torch.float64), omega=((S, Q, 3), torch.float64),
                    alpha=((S, Q, 3), torch.float64))
        res, ptrs = _requested(spec, outputs, out, tq.device)
        _check(lib().blf_so3_eval(
            self._h, _ptr(R0, torch.float64, (S, 9), "R0"), _ptr(R1, torch.float64, (S, 9), "R1"),
            _ptr(duration, torch.float64, (S,), "duration"), S, _ptr(tq, torch.float64, (S, Q), "tq"),
            Q, *ptrs, _stream(stream)))
        return res

    def fbk_dynamics(self, rho, rot, twist, joint_vel, stream=None):
        """FloatingBaseSystemKinematics::dynamics: rot [B,3,3], twist [B,6], joint_vel [B,n]."""
        torch = _torch()
        B, n = joint_vel.shape
        dp = torch.empty((B, 3), dtype=torch.float64, device=twist.device)
        dR = torch.empty((B, 3, 3), dtype=torch.float64, device=twist.device)
        dq = torch.empty((B, n), dtype=torch.float64, device=twist.device)
        _check(lib().blf_fbk_dynamics(
            self._h, n, float(rho), _ptr(rot, torch.float64, (B, 3, 3), "rot"),
            _ptr(twist, torch.float64, (B, 6), "twist"),
            _ptr(joint_vel, torch.float64, (B, n), "joint_vel") if n else None,
            ctypes.c_void_p(dp.data_ptr()), ctypes.c_void_p(dR.data_ptr()),
            ctypes.c_void_p(dq.data_ptr()) if n else None, B, _stream(stream)))
        return dp, dR, dq

    def fbk_euler_integrate(self, rho, pos, rot, joints, twist, joint_vel, t0, t1, dT,
                            stream=None):
        """ForwardEuler<FloatingBaseSystemKinematics>::integrate in place on pos [B,3],
        rot [B,3,3], joints [B,n] with constant twist [B,6] and joint_vel [B,n]."""
        torch = _torch()
        B, n = joints.shape
        _check(lib().blf_fbk_euler_integrate(
            self._h, n, float(rho), _ptr(pos, torch.float64, (B, 3), "pos"),
            _ptr(rot, torch.float64, (B, 3, 3), "rot"),
            _ptr(joints, torch.float64, (B, n), "joints") if n else None,
            _ptr(twist, torch.float64, (B, 6), "twist"),
            _ptr(joint_vel, torch.float64, (B, n), "joint_vel") if n else None,
            B, float(t0), float(t1), float(dT), _stream(stream)))
        return pos, rot, joints

    # ---- config 5: floating-base dynamics ------------------------------------------------------
    def fb_model(self, model, rho=0.01, gravity=(0.0, 0.0, -9.81)):
        """Upload a blf/robot.py model; returns an object keeping the device arrays alive."""
        torch = _torch()
        dev = torch.device("cuda", self.device)
        kinds = dict(parent=torch.int32, joint_origin=torch.float64, joint_rot=torch.float64,
                     joint_axis=torch.float64, link_mass=torch.float64, link_com=torch.float64,
                     link_inertia=torch.float64, frame_link=torch.int32, frame_pose=torch.float64)
        t = {k: _upload(model[k], dt, dev) for k, dt in kinds.items()}
        if model.get("joint_type") is not None:   # absent: every joint revolute (NULL)
            jt = torch.as_tensor(model["joint_type"], dtype=torch.int32)
            if not ((jt == 0) | (jt == 1)).all():
                raise ValueError("joint_type: every entry must be 0 (revolute) or 1 (prismatic); merge fixed "
                                 "joints first (blf.robot.reduce_fixed_joints)")
            t["joint_type"] = _upload(jt, torch.int32, dev)
        c = FbModel()
        c.ndof = int(model["n"])
        c.nframes = int(len(model["frame_link"]))
        for k, v in t.items():
            setattr(c, k, _vp(v.data_ptr()))
        for i in range(3):
            c.gravity[i] = gravity[i]
        c.rho = rho
        return _Held(c, t, n=c.ndof)

    def _fb_state(self, st, B, n):
        torch = _torch()
        shapes = dict(base_vel=(B, 6), joint_vel=(B, n), base_pos=(B, 3), base_rot=(B, 3, 3),
                      joint_pos=(B, n))
        c = FbState()
        for k in FB_STATE_KEYS:
            setattr(c, k, _ptr(st[k], torch.float64, shapes[k], k))
        return c

    def _fb_contacts(self, contacts, B):
        torch = _torch()
        c = FbContacts()
        if not contacts:
            c.ncontacts = 0
            return c
        C = contacts["frame"].shape[0]
        c.ncontacts = C
        c.frame = _ptr(contacts["frame"], torch.int32, (C,), "frame")
        c.params = _ptr(contacts["params"], torch.float64, (C, 4), "params")
        c.null_pose = _ptr(contacts["null_pose"], torch.float64, (B, C, 12), "null_pose")
        if contacts.get("law") is not None:
            c.law = _ptr(contacts["law"], torch.int32, (C,), "law")
            w = contacts.get("wrench")   # required by the library (checked there)
            c.wrench = _ptr(w, torch.float64, (B, C, 6), "wrench") if w is not None else None
        return c

    def fbd_dynamics(self, dm, state, torque, contacts=None, mass_reg=None, stream=None):
        """FloatingBaseDynamicalSystem::dynamics for a batch.  state: dict of device tensors
        (base_vel [B,6], joint_vel [B,n], base_pos [B,3], base_rot [B,3,3], joint_pos [B,n]);
        torque [B,n]; contacts: dict(frame [C] int32, params [C,4], null_pose [B,C,12]) and
        optionally law [C] int32 (CONTACT_CONTINUOUS / CONTACT_WRENCH) with wrench [B,C,6] (the
        CONTACT_WRENCH contacts' (force, torque), mixed representation at the frame).
        Returns the derivative with the same keys (base_vel -> base acceleration, ...)."""
        torch = _torch()
        out = {k: torch.empty_like(state[k]) for k in FB_STATE_KEYS}
        B, n, st, ct, reg = self._fbd_args(state, contacts, mass_reg)
        oc = self._fb_state(out, B, n)
        _check(lib().blf_fbd_dynamics(self._h, _ref(dm.c), _ref(st), _ptr(torque, torch.float64, (B, n), "torque"),
                                      _ref(ct), reg, B, _ref(oc), _stream(stream)))
        return out

    def _fbd_args(self, state, contacts, mass_reg, law_batch=None):
        """What blf_fbd_dynamics and the four blf_fbd_euler_integrate* calls build alike: B, n, the state
        and contacts structs and the mass_reg pointer (law_batch: the robots a trajectory law holds)."""
        torch = _torch()
        B, n = state["joint_pos"].shape
        if law_batch is not None and law_batch != B:
            raise ValueError(f"the trajectory holds {law_batch} robots, the state {B}")
        reg = _ptr(mass_reg, torch.float64, (n + 6, n + 6), "mass_reg") if mass_reg is not None else None
        return B, n, self._fb_state(state, B, n), self._fb_contacts(contacts, B), reg

    def _fbd_euler(self, fn, dm, state, law, times, contacts, mass_reg, stream, law_batch=None):
        """The four blf_fbd_euler_integrate* calls, in place on `state`: `law` (B, n) gives the argument that
        holds the control input, a torque pointer or a law struct's reference."""
        B, n, st, ct, reg = self._fbd_args(state, contacts, mass_reg, law_batch)
        _check(fn(self._h, _ref(dm.c), _ref(st), law(B, n), _ref(ct), reg, B, *map(float, times), _stream(stream)))
        return state

    def fbd_euler_integrate(self, dm, state, torque, t0, t1, dT, contacts=None, mass_reg=None,
                            stream=None):
        """ForwardEuler<FloatingBaseDynamicalSystem>::integrate in place on `state`."""
        return self._fbd_euler(lib().blf_fbd_euler_integrate, dm, state,
                               lambda B, n: _ptr(torque, _torch().float64, (B, n), "torque"), (t0, t1, dT),
                               contacts, mass_reg, stream)

    def fb_frame_state(self, dm, state, frames, pose=None, twist=None, stream=None):
        """blf_fb_frame_state: world transform pose [B,K,12] = (p, R row-major) and mixed twist
        [B,K,6] = (v, w) of the frames [K] (int32 device tensor) of every system -- the state a
        CONTACT_WRENCH contact model is evaluated at."""
        torch = _torch()
        B, n = state["joint_pos"].shape
        K = frames.shape[0]
        dev = state["joint_pos"].device
        st = self._fb_state(state, B, n)
        fp = _ptr(frames, torch.int32, (K,), "frames")
        pose, pp = _out(pose, (B, K, 12), torch.float64, dev, "pose", optional=False)
        twist, tp = _out(twist, (B, K, 6), torch.float64, dev, "twist", optional=False)
        _check(lib().blf_fb_frame_state(self._h, _ref(dm.c), _ref(st), K, fp, B, pp, tp, _stream(stream)))
        return pose, twist

    def fb_inverse_dynamics(self, dm, state, joint_acc=None, base_acc=None, contacts=None, joint_torque=None,
                            base_acc_out=None, base_wrench=None, status=None, stream=None):
        """blf_fb_inverse_dynamics (include/blf/blf_c.h section 8b) at `state` with joint accelerations
        joint_acc [B,n] (None: zero).  base_acc None: the free-base mode, returns dict(joint_torque [B,n],
        base_acc [B,6], status [B] int32); base_acc [B,6] given: returns dict(joint_torque, base_wrench
        [B,6] (force, torque; mixed, at the base origin), status).  status False leaves it out."""
        torch = _torch()
        B, n = state["joint_pos"].shape
        dev = state["joint_pos"].device
        given = base_acc is not None
        six, xp = _out(base_wrench if given else base_acc_out, (B, 6), torch.float64, dev,
                       "base_wrench" if given else "base_acc_out", optional=False)
        st = self._fb_state(state, B, n)
        ap = _ptr(joint_acc, torch.float64, (B, n), "joint_acc") if joint_acc is not None else None
        bp = _ptr(base_acc, torch.float64, (B, 6), "base_acc") if given else None
        ct = self._fb_contacts(contacts, B)
        tau, tp = _out(joint_torque, (B, n), torch.float64, dev, "joint_torque", optional=False)
        status, sp = _out(status, (B,), torch.int32, dev, "status")
        _check(lib().blf_fb_inverse_dynamics(self._h, _ref(dm.c), _ref(st), ap, bp, _ref(ct), B, tp,
                                             None if given else xp, xp if given else None, sp, 0,
                                             _stream(stream)))
        return {"joint_torque": tau, "status": status, "base_wrench" if given else "base_acc": six}

    # ---- whole-body inverse kinematics (include/blf/blf_c.h section 12) ------------------------
    def ik_tasks(self, batch, ndof, frame=None, se3_weight=None, se3_kp=None, se3_pose=None, se3_twist=None,
                 com_weight=None, com_kp=0.0, com_pos=None, com_vel=None, joint_weight=None,
                 joint_kp=None, joint_pos=None, joint_vel=None, base_damping=0.0):
        """Build a blf_ik_tasks for `batch` robots of `ndof` joints (e.g. **robot.standing_ik_tasks):
        frame [K] int32, se3_weight [K,6], se3_kp [K,2], se3_pose [B,K,12], se3_twist [B,K,6] or
        None, com_weight [3] or None (no CoM task), com_pos / com_vel [B,3], joint_weight / joint_kp
        [n], joint_pos / joint_vel [B,n].  Host arrays are uploaded; device tensors are used as they
        are (so a blf_swing_foot_eval pose output feeds se3_pose without a copy).  Returns an object
        with the struct (.c) and the tensors (.t) it keeps alive."""
        torch = _torch()
        dev = torch.device("cuda", self.device)
        B, n = int(batch), int(ndof)
        K = 0 if frame is None else int(len(frame))
        spec = dict(frame=(frame, torch.int32, (K,)), se3_weight=(se3_weight, torch.float64, (K, 6)),
                    se3_kp=(se3_kp, torch.float64, (K, 2)), se3_pose=(se3_pose, torch.float64, (B, K, 12)),
                    se3_twist=(se3_twist, torch.float64, (B, K, 6)), com_weight=(com_weight, torch.float64, (3,)),
                    com_pos=(com_pos, torch.float64, (B, 3)), com_vel=(com_vel, torch.float64, (B, 3)),
                    joint_weight=(joint_weight, torch.float64, (n,)), joint_kp=(joint_kp, torch.float64, (n,)),
                    joint_pos=(joint_pos, torch.float64, (B, n)), joint_vel=(joint_vel, torch.float64, (B, n)))
        c = IkTasks()
        c.nse3, c.reserved = K, 0
        c.com_kp, c.base_damping = float(com_kp), float(base_damping)
        t = {}
        for k, (a, dt, shape) in spec.items():
            if a is None or (K == 0 and k in ("frame", "se3_weight", "se3_kp", "se3_pose", "se3_twist")):
                continue
            t[k] = _on_device(a, dt, dev)
            setattr(c, k, _ptr(t[k], dt, shape, k))
        return _Held(c, t, batch=B, n=n)

    @staticmethod
    def ik_hard(se3=(), com=(False, False, False), rel_pivot_min=0.0):
        """Build a blf_ik_hard (section 12b): se3 [K][6] bools mark the rows of SE3 task k (linear
        xyz, angular xyz) that hold exactly, com [3] bools the CoM rows; rel_pivot_min = tau (0: the
        default 1e-8).  E.g. **robot.standing_ik_hard(model)."""
        rows = 0
        se3 = [list(r) for r in se3]
        if len(se3) > 4 or any(len(r) != 6 for r in se3) or len(com) != 3:
            raise ValueError("ik_hard: se3 must be [K <= 4][6] bools and com [3] bools")
        for k, r in enumerate(se3):
            for a, on in enumerate(r):
                rows |= int(bool(on)) << (6 * k + a)
        for a, on in enumerate(com):
            rows |= int(bool(on)) << (24 + a)
        h = IkHard()
        h.rows, h.reserved, h.rel_pivot_min = rows, 0, float(rel_pivot_min)
        return h

    def ik_limits(self, pos_lower, pos_upper, klim, vel_max=None, sampling_time=0.01, max_iter=0):
        """Build a blf_ik_limits (section 12c) for a model of n joints, e.g.
        **robot.humanoid24_joint_limits(model): pos_lower / pos_upper [n] (-inf / +inf: no limit), klim
        [n] in (0, 1], vel_max [n] or None, shared by the batch.  Host arrays are uploaded.  Returns an
        object with the struct (.c) and the tensors (.t) it keeps alive."""
        torch = _torch()
        dev = torch.device("cuda", self.device)
        n = int(len(pos_lower))
        c = IkLimits()
        t = {}
        for k, a in (("pos_lower", pos_lower), ("pos_upper", pos_upper), ("klim", klim), ("vel_max", vel_max)):
            if a is None:
                continue
            t[k] = _on_device(a, torch.float64, dev)
            setattr(c, k, _ptr(t[k], torch.float64, (n,), k))
        c.sampling_time, c.max_iter, c.reserved = float(sampling_time), int(max_iter), 0
        return _Held(c, t, n=n)

    def _fb_ik(self, stem, steps, dm, state, tasks, nu, status, hard, limits, iters, active, stream):
        """The plain, _hard and _limits entry points of blf_fb_ik_solve (steps = ()) and blf_fb_ik_integrate
        (steps = (steps, dT)): one argument list, with the variant's structs and outputs spliced in.  Returns
        (nu, status) and, with limits, iters and active (None for what was not requested)."""
        torch = _torch()
        B, n = state["joint_pos"].shape
        dev = state["joint_pos"].device
        res = [_out(nu, (B, 6 + n), torch.float64, dev, "nu", optional=bool(steps)),
               _out(status, (B,), torch.int32, dev, "status")]
        if limits is not None:
            res += [_out(iters, (B,), torch.int32, dev, "iters", zero=True),
                    _out(active, (B, 2), torch.int64, dev, "active", zero=True)]
            fn, extra = stem + "_limits", (_ref(hard), _ref(limits.c))
        elif hard is not None:
            fn, extra = stem + "_hard", (_ref(hard),)
        else:
            fn, extra = stem, ()
        _check(getattr(lib(), fn)(self._h, _ref(dm.c), _ref(self._fb_state(state, B, n)), _ref(tasks.c), *extra, B,
                                  *steps, *(p for _, p in res), _stream(stream)))
        return tuple(t for t, _ in res)

    def fb_ik_solve(self, dm, state, tasks, nu=None, status=None, stream=None, hard=None, limits=None,
                    iters=None, active=None):
        """blf_fb_ik_solve: nu [B,6+n] = (base mixed twist, joint velocities) minimising the weighted
        task errors at the state's base_pos / base_rot / joint_pos, and the per-robot status [B]
        int32 (IK_OK / IK_NOT_POSITIVE / IK_BAD_INPUT; status=False: not requested).
        hard (an ik_hard()): blf_fb_ik_solve_hard, the marked rows held exactly (status may then be
        IK_HARD_DEPENDENT); None: today's call.
        limits (an ik_limits()): blf_fb_ik_solve_limits, the joint velocities kept in section 12c's box
        (status may then be IK_LIMITS_UNRESOLVED); the call then returns (nu, status, iters [B] int32,
        active [B,2] int64: the joints that end on their lower | upper bound, a bit each)."""
        return self._fb_ik("blf_fb_ik_solve", (), dm, state, tasks, nu, status, hard, limits, iters, active, stream)

    def fb_ik_integrate(self, dm, state, tasks, steps, dT, nu=None, status=None, stream=None, hard=None,
                        limits=None, iters=None, active=None):
        """blf_fb_ik_integrate: `steps` x (solve, one Euler step of dT) in one launch, in place on
        `state` (base_vel / joint_vel receive the last step's nu).  nu / status as fb_ik_solve;
        False: not requested.  hard as fb_ik_solve (blf_fb_ik_integrate_hard).  Returns (state, nu,
        status), and with limits (blf_fb_ik_integrate_limits) also iters (summed over the steps) and
        active (the last step's)."""
        return (state,) + self._fb_ik("blf_fb_ik_integrate", (int(steps), float(dT)), dm, state, tasks, nu, status,
                                      hard, limits, iters, active, stream)

    # ---- reference tracking (include/blf/blf_c.h section 12d) ------------------------------------
    def ik_schedule(self, batch, nse3, steps, stance_rows=0, contact=None, se3_pose=None, se3_twist=None,
                    com_pos=None, com_vel=None):
        """Build a blf_ik_schedule for `batch` robots, K = nse3 SE3 tasks and T = steps steps:
        stance_rows an int in ik_hard()'s bit layout (SE3 bits only, e.g. ik_hard(se3=...).rows), contact
        [B,K,T] int32 or None (never in contact), se3_pose [B,K,T,12], se3_twist [B,K,T,6] or None,
        com_pos / com_vel [B,T,3].  swing_foot_eval's outputs for B*K lists and T query times fit as they
        stand ([B*K,T,...] device tensors are passed on without a copy); host arrays are uploaded.
        Returns an object with the struct (.c) and the tensors (.t) it keeps alive."""
        torch = _torch()
        dev = torch.device("cuda", self.device)
        B, K, T = int(batch), int(nse3), int(steps)
        c = IkSchedule()
        c.steps, c.reserved, c.stance_rows, c.reserved2 = T, 0, int(stance_rows), 0
        spec = dict(contact=(contact, torch.int32, B * K * T), se3_pose=(se3_pose, torch.float64, B * K * T * 12),
                    se3_twist=(se3_twist, torch.float64, B * K * T * 6), com_pos=(com_pos, torch.float64, B * T * 3),
                    com_vel=(com_vel, torch.float64, B * T * 3))
        t = {}
        for k, (a, dt, count) in spec.items():
            if a is None or (K == 0 and k in ("contact", "se3_pose", "se3_twist")):
                continue
            t[k] = _on_device(a, dt, dev)
            if t[k].numel() != count:
                raise ValueError(f"ik_schedule: {k} has {t[k].numel()} elements, expected {count}")
            setattr(c, k, _ptr(t[k], dt, tuple(t[k].shape), k))
        return _Held(c, t, batch=B, nse3=K, steps=T)

    def fb_ik_track(self, dm, state, tasks, schedule, dT, hard=None, limits=None, joint_traj=None, base_traj=None,
                    nu_traj=None, status=None, fail_step=None, iters=None, active=None, stream=None):
        """blf_fb_ik_track: schedule.steps x (section 12c's solve with step t's set points and each
        robot's own hard rows of step t, one Euler step of dT) in one launch, in place on `state`.
        hard (an ik_hard()): rows hard at every step; limits (an ik_limits()) or None: no box.  Every
        output is optional (None: allocated, False: not requested).  Returns a dict: state, joint_traj
        [T,B,n], base_traj [T,B,12], nu_traj [T,B,6+n], status, fail_step, iters [B] int32, active
        [B,2] int64 (None for what was not requested)."""
        torch = _torch()
        B, n = state["joint_pos"].shape
        T = schedule.steps
        spec = dict(joint_traj=((T, B, n), torch.float64), base_traj=((T, B, 12), torch.float64),
                    nu_traj=((T, B, 6 + n), torch.float64), status=((B,), torch.int32),
                    fail_step=((B,), torch.int32), iters=((B,), torch.int32), active=((B, 2), torch.int64))
        given = dict(joint_traj=joint_traj, base_traj=base_traj, nu_traj=nu_traj, status=status,
                     fail_step=fail_step, iters=iters, active=active)
        out, ptrs = _outs(spec, given, state["joint_pos"].device, zero=True)
        _check(lib().blf_fb_ik_track(self._h, _ref(dm.c), _ref(self._fb_state(state, B, n)), _ref(tasks.c),
                                     _ref(hard), _ref(limits.c if limits is not None else None),
                                     _ref(schedule.c), B, float(dT), *ptrs, _stream(stream)))
        return dict(out, state=state)

    # ---- config 5: the closed loop's maps ----------------------------------
    def fb_dcm(self, dm, state, omega=None, column=0, com=None, xi=None, stream=None):
        """blf_fb_dcm: centre of mass and its velocity com [B,6] of every system and, when omega
        ([B,K] device tensor) is given, the DCM xi [B,2] = c_xy + cdot_xy / omega[:, column]."""
        torch = _torch()
        B, n = state["joint_pos"].shape
        dev = state["joint_pos"].device
        com = com if com is not None else torch.empty((B, 6), dtype=torch.float64, device=dev)
        optr, ostride = None, 0
        if omega is not None:
            K = omega.shape[1]
            _ptr(omega, torch.float64, (B, K), "omega")
            if not 0 <= column < K:
                raise ValueError(f"omega column {column} outside [0, {K})")
            optr, ostride = _vp(omega.data_ptr() + 8 * column), K
            xi = xi if xi is not None else torch.empty((B, 2), dtype=torch.float64, device=dev)
        elif xi is not None:
            raise ValueError("xi requested without omega")
        _check(lib().blf_fb_dcm(self._h, _ref(dm.c), _ref(self._fb_state(state, B, n)),
                                optr, ostride, B, _ptr(com, torch.float64, (B, 6), "com"),
                                _ptr(xi, torch.float64, (B, 2), "xi") if xi is not None else None,
                                _stream(stream)))
        return com, xi

    def posture_law(self, q_nominal, lean):
        """Upload a blf_posture_law: q_nominal [n], lean [n,2] (host arrays)."""
        torch = _torch()
        dev = torch.device("cuda", self.device)
        t = dict(q_nominal=_upload(q_nominal, torch.float64, dev), lean=_upload(lean, torch.float64, dev))
        n = t["q_nominal"].shape[0]
        if t["lean"].shape != (n, 2):
            raise ValueError("posture law: q_nominal [n] and lean [n,2]")
        c = PostureLaw()
        c.ndof = n
        c.q_nominal, c.lean = _vp(t["q_nominal"].data_ptr()), _vp(t["lean"].data_ptr())
        return _Held(c, t)

    def posture_reference(self, law, com, vrp, q_ref=None, stream=None):
        """blf_dcm_posture_reference: joint references [B,n] from the plan's first VRP (vrp
        [B,N,2], a blf_dcm_mpc_solve output) and the centre of mass com [B,6] (fb_dcm)."""
        torch = _torch()
        B, N = vrp.shape[0], vrp.shape[1]
        n = law.c.ndof
        q_ref = q_ref if q_ref is not None else torch.empty((B, n), dtype=torch.float64,
                                                            device=vrp.device)
        args = (self._h, ctypes.byref(law.c), _ptr(com, torch.float64, (B, 6), "com"),
                _ptr(vrp, torch.float64, (B, N, 2), "vrp"), 2 * N, B,
                _ptr(q_ref, torch.float64, (B, n), "q_ref"))
        _check(lib().blf_dcm_posture_reference(*args, _stream(stream)))
        return q_ref

    def joint_impedance(self, kp, kd):
        """Device copies of the impedance gains kp, kd [n] (host arrays)."""
        torch = _torch()
        dev = torch.device("cuda", self.device)
        return dict(kp=_upload(kp, torch.float64, dev), kd=_upload(kd, torch.float64, dev))

    def fbd_euler_integrate_impedance(self, dm, state, impedance, q_ref, t0, t1, dT, contacts=None,
                                      mass_reg=None, stream=None):
        """blf_fbd_euler_integrate_impedance in place on `state`: the control input of every
        Euler step is tau = kp (q_ref - q) - kd qdot (impedance: joint_impedance())."""
        torch = _torch()
        imp = JointImpedance()

        def law(B, n):
            imp.ndof = n
            imp.kp = _ptr(impedance["kp"], torch.float64, (n,), "kp")
            imp.kd = _ptr(impedance["kd"], torch.float64, (n,), "kd")
            imp.q_ref = _ptr(q_ref, torch.float64, (B, n), "q_ref")
            return ctypes.byref(imp)
        return self._fbd_euler(lib().blf_fbd_euler_integrate_impedance, dm, state, law, (t0, t1, dT), contacts,
                               mass_reg, stream)

    def joint_impedance_traj(self, impedance, q_ref, steps_per_slice, qd_ref=None, qd_offset=0, q_bias=None):
        """A blf_joint_impedance_traj: impedance (joint_impedance()), q_ref [T,B,n] (fb_ik_track's
        joint_traj), qd_ref [T,B,w] or None with the velocities at columns qd_offset .. qd_offset + n
        (fb_ik_track's nu_traj with qd_offset = 6), q_bias [B,n] or None.  Returns an object with the
        struct (.c) and the tensors (.t) it keeps alive."""
        torch = _torch()
        T, B, n = q_ref.shape
        c = JointImpedanceTraj()
        c.ndof, c.slices, c.steps_per_slice, c.reserved = n, T, int(steps_per_slice), 0
        c.kp = _ptr(impedance["kp"], torch.float64, (n,), "kp")
        c.kd = _ptr(impedance["kd"], torch.float64, (n,), "kd")
        c.q_ref = _ptr(q_ref, torch.float64, (T, B, n), "q_ref")
        t = dict(kp=impedance["kp"], kd=impedance["kd"], q_ref=q_ref, qd_ref=qd_ref, q_bias=q_bias)
        if qd_ref is not None:
            w = qd_ref.shape[-1]
            _ptr(qd_ref, torch.float64, (T, B, w), "qd_ref")
            if not 0 <= qd_offset <= w - n:
                raise ValueError(f"qd_ref: columns {qd_offset}..{qd_offset + n} outside [0, {w})")
            c.qd_ref, c.qd_stride = _vp(qd_ref.data_ptr() + 8 * int(qd_offset)), w
        if q_bias is not None:
            c.q_bias = _ptr(q_bias, torch.float64, (B, n), "q_bias")
        return _Held(c, t, batch=B)

    def fbd_euler_integrate_impedance_traj(self, dm, state, traj, t0, t1, dT, contacts=None, mass_reg=None,
                                           stream=None):
        """blf_fbd_euler_integrate_impedance_traj in place on `state`: integration step i tracks slice
        min(i // steps_per_slice, T - 1) of traj (joint_impedance_traj()),
        tau = kp (q_ref + q_bias - q) - kd (qdot - qd_ref)."""
        return self._fbd_euler(lib().blf_fbd_euler_integrate_impedance_traj, dm, state,
                               lambda B, n: ctypes.byref(traj.c), (t0, t1, dT), contacts, mass_reg, stream, traj.batch)

    def computed_torque_traj(self, kp, kd, q_ref, steps_per_slice, qd_ref=None, qd_offset=0, qdd_ref=None,
                             q_bias=None, tau_max=None, qdd_offset=0, tau_last=None):
        """A blf_computed_torque_traj: acceleration gains kp, kd (scalars or [n]; host values or device
        tensors), q_ref [T,B,n], qd_ref / qdd_ref [T,B,w] or None with the joint columns at qd_offset /
        qdd_offset (fb_ik_track's nu_traj with qd_offset = 6), q_bias [B,n] or None, tau_max (scalar or
        [n], finite and > 0) or None, tau_last [B,n] (True allocates) or None.  Returns an object with the
        struct (.c) and the tensors (.t) it keeps alive."""
        torch = _torch()
        T, B, n = q_ref.shape
        dev = q_ref.device

        def vec(a):
            if isinstance(a, torch.Tensor) and a.is_cuda:
                return a
            v = torch.as_tensor(a, dtype=torch.float64).reshape(-1)
            return _upload(v.expand(n) if v.numel() == 1 else v, torch.float64, dev)
        c = ComputedTorqueTraj()
        c.ndof, c.slices, c.steps_per_slice, c.reserved = n, T, int(steps_per_slice), 0
        t = dict(kp=vec(kp), kd=vec(kd), q_ref=q_ref, qd_ref=qd_ref, qdd_ref=qdd_ref, q_bias=q_bias)
        c.kp = _ptr(t["kp"], torch.float64, (n,), "kp")
        c.kd = _ptr(t["kd"], torch.float64, (n,), "kd")
        c.q_ref = _ptr(q_ref, torch.float64, (T, B, n), "q_ref")
        for name, ref, off in (("qd", qd_ref, qd_offset), ("qdd", qdd_ref, qdd_offset)):
            if ref is None:
                continue
            w = ref.shape[-1]
            _ptr(ref, torch.float64, (T, B, w), name + "_ref")
            if not 0 <= off <= w - n:
                raise ValueError(f"{name}_ref: columns {off}..{off + n} outside [0, {w})")
            setattr(c, name + "_ref", _vp(ref.data_ptr() + 8 * int(off)))
            setattr(c, name + "_stride", w)
        if q_bias is not None:
            c.q_bias = _ptr(q_bias, torch.float64, (B, n), "q_bias")
        if tau_max is not None:
            if not (isinstance(tau_max, torch.Tensor) and tau_max.is_cuda):   # host values: checked here
                tm = torch.as_tensor(tau_max, dtype=torch.float64)
                if not bool((torch.isfinite(tm) & (tm > 0)).all()):
                    raise ValueError("tau_max: every entry must be finite and > 0")
            t["tau_max"] = vec(tau_max)
            c.tau_max = _ptr(t["tau_max"], torch.float64, (n,), "tau_max")
        if tau_last is True:
            tau_last = torch.empty((B, n), dtype=torch.float64, device=dev)
        if tau_last is not None:
            c.tau_last = _ptr(tau_last, torch.float64, (B, n), "tau_last")
        t["tau_last"] = tau_last
        return _Held(c, t, batch=B, tau_last=tau_last)

    def fbd_euler_integrate_computed_torque_traj(self, dm, state, law, t0, t1, dT, contacts=None, mass_reg=None,
                                                 stream=None):
        """blf_fbd_euler_integrate_computed_torque_traj in place on `state`: before every step the torque
        is the free-base inverse dynamics of sdd = qdd_ref + kp (q_ref + q_bias - q) + kd (qd_ref - qdot),
        clamped to tau_max, then the forward step (law: computed_torque_traj()).  mass_reg is refused."""
        return self._fbd_euler(lib().blf_fbd_euler_integrate_computed_torque_traj, dm, state,
                               lambda B, n: ctypes.byref(law.c), (t0, t1, dT), contacts, mass_reg, stream, law.batch)

    def dcm_com_reference(self, xi0, vrp, omega, z_ref, c_ref, steps, dT, column=0, com_pos=None, com_vel=None,
                          xi_end=None, stream=None):
        """blf_dcm_com_reference: the CoM set points com_pos, com_vel [B,T,3] of an ik_schedule from the
        measured DCM xi0 [B,2] (fb_dcm), the plan's first VRP (vrp [B,N,2], a solve's output) and
        omega[:, column] ([B,K]); z_ref [B]; c_ref [B,2] is read and advanced in place.  xi_end [B,2]:
        None allocates, False leaves it out.  Returns (com_pos, com_vel, xi_end)."""
        torch = _torch()
        B, N = vrp.shape[0], vrp.shape[1]
        K = omega.shape[1]
        dev = vrp.device
        T = int(steps)
        _ptr(omega, torch.float64, (B, K), "omega")
        if not 0 <= column < K:
            raise ValueError(f"omega column {column} outside [0, {K})")
        args = (self._h, _ptr(xi0, torch.float64, (B, 2), "xi0"), _ptr(vrp, torch.float64, (B, N, 2), "vrp"), 2 * N,
                _vp(omega.data_ptr() + 8 * column), K, _ptr(z_ref, torch.float64, (B,), "z_ref"),
                _ptr(c_ref, torch.float64, (B, 2), "c_ref"), T, float(dT), B)
        com_pos, pp = _out(com_pos, (B, max(T, 0), 3), torch.float64, dev, "com_pos", optional=False)
        com_vel, vp = _out(com_vel, (B, max(T, 0), 3), torch.float64, dev, "com_vel", optional=False)
        xi_end, ep = _out(xi_end, (B, 2), torch.float64, dev, "xi_end")
        _check(lib().blf_dcm_com_reference(*args, pp, vp, ep, _stream(stream)))
        return com_pos, com_vel, xi_end
