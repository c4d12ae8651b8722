"""GPU pins of the binding itself (blf/native.py), not of the kernels: for every Handle method, what comes
back when the outputs are not given (shape, dtype, device), that given outputs come back as the same
objects, that False leaves an optional output out, the fill of the outputs the wrapper zero-fills, every
refusal the wrapper makes on the host (exception type and the argument's name), and that the variants
which share builders agree (phased solve == expand + solve bit for bit; the 2-D / 3-D / n-D hull calls on
their common domains).  Shapes are the smallest at which the wrapper can go wrong: B = 3 (odd: the
wavefront's last robot is a padding one), horizon 4 with 4 facets, 5 hull points, the 3-joint chain of
tests/fb_models.py with one SE3 task and T = 2 steps."""
import numpy as np
import pytest
import torch

import fb_models as FM
import gpu_util as GU
from blf import native, robot

pytestmark = pytest.mark.gpu

B, N, M, NJ, T = 3, 4, 4, 3, 2
F64, I32, I64 = torch.float64, torch.int32, torch.int64
d = GU.to_device


def is_dev(t, shape, dtype=F64):
    assert isinstance(t, torch.Tensor) and t.is_cuda and t.is_contiguous(), t
    assert tuple(t.shape) == tuple(shape) and t.dtype == dtype, (tuple(t.shape), t.dtype, shape, dtype)


def new(shape, dtype=F64):
    return torch.empty(shape, dtype=dtype, device="cuda")


def refused(exc, name, fn, *a, **kw):
    """fn raises `exc` and the message names the argument."""
    with pytest.raises(exc, match=name):
        fn(*a, **kw)


# ---- the QP, the phase table and the hulls ------------------------------------------------------------
BOX = np.array([[1.0, 0.0], [-1.0, 0.0], [0.0, 1.0], [0.0, -1.0]])
SOL = dict(xi=((B, N + 1, 2), F64), vrp=((B, N, 2), F64), status=((B,), I32), iters=((B,), I32),
           polished=((B,), I32), passes=((B,), I32))
WIN = dict(omega=((B, N), F64), xi_ref=((B, N + 1, 2), F64), vrp_ref=((B, N, 2), F64), A=((B, N, M, 2), F64),
           b=((B, N, M), F64), nfacets=((B, N), I32))


@pytest.fixture(scope="module")
def table():
    """Two phases per problem: a box of half-width 0.1 about the origin until 0.04 s, then one about
    (0.02, 0) of half-width 0.12."""
    rng = np.random.default_rng(7)
    ref = np.zeros((B, 2, 2))
    ref[:, 1, 0] = 0.02
    hw = np.array([0.1, 0.12])
    b = hw[None, :, None] + np.einsum("mk,bpk->bpm", BOX, ref)
    return dict(nphases=d(np.full(B, 2), I32), phase_begin=d(np.tile([0.0, 0.04], (B, 1))),
                phase_end=d(np.tile([0.04, 10.0], (B, 1))), phase_A=d(np.tile(BOX, (B, 2, 1, 1))), phase_b=d(b),
                phase_nf=d(np.full((B, 2), 4), I32), phase_ref=d(ref),
                xi_init=d(rng.normal(size=(B, 2)) * 0.02), omega=d(np.full((B, N + 1), 3.0)))


@pytest.fixture(scope="module")
def qp(handle, table):
    """The window of knots 0..N as a blf_dcm_mpc_problem dict."""
    ex = handle.dcm_phase_expand(table, 0, 0.02, N)
    return dict(ex, xi_init=table["xi_init"], omega=table["omega"][:, :N].contiguous())


def test_dcm_mpc_solve_outputs(handle, qp):
    out = handle.dcm_mpc_solve(qp)
    assert set(out) == set(SOL)
    for k, (shape, dt) in SOL.items():
        is_dev(out[k], shape, dt)
    lam = handle.dcm_mpc_solve(qp, lambda_out=True)
    assert set(lam) == set(SOL) | {"lam"}
    is_dev(lam["lam"], (B, N, M))
    mine = {k: new(*SOL[k]) for k in SOL}
    keep = dict(mine)
    assert handle.dcm_mpc_solve(qp, out=mine) is mine
    assert all(mine[k] is keep[k] for k in keep) and set(mine) == set(keep)
    lam_buf = new((B, N, M))
    mine["lam"] = lam_buf
    warm = dict(vrp=lam["vrp"], lam=lam["lam"], shift=1, floor=1e-3, status=lam["status"])
    assert handle.dcm_mpc_solve(qp, out=mine, warm=warm, lambda_out=True)["lam"] is lam_buf
    minimal = {k: new(*SOL[k]) for k in ("xi", "vrp", "status", "iters")}   # polished / passes are optional
    assert set(handle.dcm_mpc_solve(qp, out=minimal)) == set(minimal)
    torch.cuda.synchronize()
    assert (out["status"] == 0).all()
    for k in SOL:   # a call with warm = NULL is the cold call
        assert torch.equal(out[k], lam[k]), k


def test_dcm_mpc_solve_refusals(handle, qp):
    refused(ValueError, "params.horizon", handle.dcm_mpc_solve, qp, params=native.default_params(N + 1, max_facets=M))
    refused(ValueError, "max_facets", handle.dcm_mpc_solve, qp, params=native.default_params(N, max_facets=M + 1))
    refused(TypeError, "omega", handle.dcm_mpc_solve, dict(qp, omega=qp["omega"].float()))
    refused(TypeError, "nfacets", handle.dcm_mpc_solve, dict(qp, nfacets=qp["nfacets"].long()))
    refused(ValueError, "xi_init", handle.dcm_mpc_solve, dict(qp, xi_init=new((B, 3))))
    refused(ValueError, "A must be contiguous", handle.dcm_mpc_solve,
            dict(qp, A=new((B, N, 2, M)).transpose(2, 3)))
    refused(ValueError, "b must be a device", handle.dcm_mpc_solve, dict(qp, b=qp["b"].cpu()))
    refused(TypeError, "xi_ref must be a torch tensor", handle.dcm_mpc_solve, dict(qp, xi_ref=qp["xi_ref"].cpu().numpy()))
    refused(ValueError, "status has shape", handle.dcm_mpc_solve, qp,
            out=dict({k: new(*SOL[k]) for k in SOL}, status=new((B + 1,), I32)))
    refused(ValueError, "warm vrp", handle.dcm_mpc_solve, qp, warm=dict(vrp=new((B, N, 3)), lam=new((B, N, M))))
    refused(TypeError, "warm status", handle.dcm_mpc_solve, qp,
            warm=dict(vrp=new((B, N, 2)), lam=new((B, N, M)), status=new((B,), I64)))
    refused(ValueError, "lam", handle.dcm_mpc_solve, qp, out=dict({k: new(*SOL[k]) for k in SOL}, lam=new((B, N))),
            lambda_out=True)


def test_prepare_dcm_mpc_solve(handle, qp):
    params = native.default_params(N, max_facets=M)
    ref = handle.dcm_mpc_solve(qp, params)
    out = {k: new(*SOL[k]) for k in SOL}
    f, s = handle.prepare_dcm_mpc_solve(qp, params, out)
    assert s.value == native._stream().value
    for k in ("xi", "vrp"):
        out[k].fill_(float("nan"))
    keep = f()
    assert any(x is out for x in keep) and any(x is qp for x in keep)
    torch.cuda.synchronize()
    for k in SOL:
        assert torch.equal(out[k], ref[k]), k
    refused(ValueError, "params.horizon", handle.prepare_dcm_mpc_solve, qp, native.default_params(N + 2), out)


def test_phase_expand_outputs_and_refusals(handle, table):
    shapes = {k: WIN[k] for k in ("A", "b", "nfacets", "xi_ref", "vrp_ref")}
    ex = handle.dcm_phase_expand(table, 1, 0.02, N)
    assert set(ex) == set(shapes)
    for k, (shape, dt) in shapes.items():
        is_dev(ex[k], shape, dt)
    mine = {k: new(*shapes[k]) for k in shapes}
    keep = dict(mine)
    assert handle.dcm_phase_expand(table, 1, 0.02, N, out=mine) is mine
    torch.cuda.synchronize()
    for k in shapes:
        assert mine[k] is keep[k] and torch.equal(mine[k], ex[k]), k
    refused(ValueError, "phase_b", handle.dcm_phase_expand, dict(table, phase_b=new((B, 2, M, 1))), 0, 0.02, N)
    refused(TypeError, "nphases", handle.dcm_phase_expand, dict(table, nphases=table["nphases"].long()), 0, 0.02, N)
    refused(ValueError, "phase_ref", handle.dcm_phase_expand, dict(table, phase_ref=new((B, 3, 2))), 0, 0.02, N)
    refused(ValueError, "xi_ref", handle.dcm_phase_expand, table, 0, 0.02, N, out=dict(mine, xi_ref=new((B, N, 2))))


def test_phased_solve_equals_expand_then_solve(handle, table):
    """Through the shared builders, cold and warm, with the window offset as a strided view of omega."""
    prev = None
    for s in (0, 1):
        omega = table["omega"][:, s:s + N]
        warm = None if prev is None else dict(vrp=prev["vrp"], lam=prev["lam"], shift=1, floor=1e-3,
                                              status=prev["status"])
        got = handle.dcm_mpc_solve_phased(table, s, table["xi_init"], omega, warm=warm, lambda_out=True)
        ex = handle.dcm_phase_expand(table, s, 0.02, N)
        ref = handle.dcm_mpc_solve(dict(ex, xi_init=table["xi_init"], omega=omega.contiguous()), warm=warm,
                                   lambda_out=True)
        torch.cuda.synchronize()
        assert set(got) == set(ref) | {"window"}
        for k in ref:
            assert torch.equal(got[k], ref[k]), (k, s)
        assert (got["status"] == 0).all()
        prev = got


def test_phased_solve_outputs_and_refusals(handle, table):
    omega = table["omega"][:, :N]
    got = handle.dcm_mpc_solve_phased(table, 0, table["xi_init"], omega)
    assert set(got) == set(SOL) | {"window"} and set(got["window"]) == set(WIN)
    for k, (shape, dt) in SOL.items():
        is_dev(got[k], shape, dt)
    for k, (shape, dt) in WIN.items():
        is_dev(got["window"][k], shape, dt)
    win = got["window"]
    again = handle.dcm_mpc_solve_phased(table, 0, table["xi_init"], omega, out=got)   # the scratch is kept
    assert again is got and again["window"] is win
    mine = {k: new(*SOL[k]) for k in SOL}
    own = {k: new(*WIN[k]) for k in WIN}
    res = handle.dcm_mpc_solve_phased(table, 0, table["xi_init"], omega, out=mine, window=own, lambda_out=True)
    assert res is mine and "window" not in mine   # a caller's window stays the caller's
    is_dev(mine["lam"], (B, N, M))
    torch.cuda.synchronize()
    call = lambda **kw: handle.dcm_mpc_solve_phased(table, 0, table["xi_init"], omega, **kw)
    refused(ValueError, "params.horizon", call, params=native.default_params(N + 1, max_facets=M))
    refused(ValueError, "window vrp_ref", call, window=dict(own, vrp_ref=new((B, N, 3))))
    refused(ValueError, "omega", handle.dcm_mpc_solve_phased, table, 0, table["xi_init"],
            new((N, B)).t())                                             # column stride != 1
    refused(ValueError, "omega", handle.dcm_mpc_solve_phased, table, 0, table["xi_init"], omega.float())
    refused(ValueError, "xi_init", handle.dcm_mpc_solve_phased, table, 0, new((B, 3)), omega)
    refused(ValueError, "phase_end", handle.dcm_mpc_solve_phased, dict(table, phase_end=new((B, 3))), 0,
            table["xi_init"], omega)


def test_phase_table_and_assemble_constraints(handle):
    rng = np.random.default_rng(3)
    rect = np.array([[-1.0, -1.0], [1.0, -1.0], [1.0, 1.0], [-1.0, 1.0], [0.0, 0.0]]) * 0.05
    corners = rect[None, None] + rng.normal(size=(B, 2, 1, 2)) * 0.1            # [B, P = 2, C = 5, 2]
    ncorners = np.full((B, 2), 5)
    tab = handle.phase_table(d(np.full(B, 2), I32), d(np.zeros((B, 2))), d(np.ones((B, 2))), d(corners),
                             d(ncorners, I32), max_facets=M)
    shapes = dict(nphases=((B,), I32), phase_begin=((B, 2), F64), phase_end=((B, 2), F64),
                  phase_A=((B, 2, M, 2), F64), phase_b=((B, 2, M), F64), phase_nf=((B, 2), I32),
                  phase_ref=((B, 2, 2), F64))
    assert set(tab) == set(shapes)
    for k, (shape, dt) in shapes.items():
        is_dev(tab[k], shape, dt)
    torch.cuda.synchronize()
    assert (tab["phase_nf"] == 4).all()
    np.testing.assert_allclose(tab["phase_ref"].cpu().numpy(), corners.mean(axis=2), atol=1e-15)
    ref = d(np.zeros((B, 2, 2)))
    assert handle.phase_table(d(np.full(B, 2), I32), d(np.zeros((B, 2))), d(np.ones((B, 2))), d(corners),
                              d(ncorners, I32), max_facets=M, ref=ref)["phase_ref"] is ref
    A, b, nf = handle.assemble_constraints(d(np.concatenate([corners, corners[:, :1]], axis=1)),
                                           d(np.full((B, 3), 5), I32), max_facets=M)
    is_dev(A, (B, 2, M, 2)), is_dev(b, (B, 2, M)), is_dev(nf, (B, 2), I32)
    torch.cuda.synchronize()
    assert torch.equal(A, tab["phase_A"]) and torch.equal(b, tab["phase_b"])


def _facets(A, b, nf):
    return sorted(map(tuple, np.round(np.c_[A[:nf], b[:nf]], 12)))


def test_hull_wrappers(handle):
    """The three hrep calls and the two containment calls: outputs, given outputs, refusals, and agreement
    where their domains overlap (facet sets to 1e-12, as tests/test_gpu_kernels.py compares hulls as sets;
    containment exactly)."""
    rng = np.random.default_rng(11)
    P_ = 5
    npts = d(np.full(B, P_), I32)
    for D, fn, mf in ((2, handle.hull2d_hrep, 8), (3, handle.hull3d_hrep, 32)):
        pts = d(rng.normal(size=(B, P_, D)))
        A, b, nf = fn(pts, npts)
        is_dev(A, (B, mf, D)), is_dev(b, (B, mf)), is_dev(nf, (B,), I32)   # the default max_facets
        mine = (new((B, 6, D)), new((B, 6)), new((B,), I32))
        got = fn(pts, npts, 6, out=mine)
        assert all(x is y for x, y in zip(got, mine))
        An, bn, nn = handle.hullnd_hrep(pts, npts, 6)
        is_dev(An, (B, 6, D)), is_dev(bn, (B, 6)), is_dev(nn, (B,), I32)
        mine_n = (new((B, 6, D)), new((B, 6)), new((B,), I32))
        assert all(x is y for x, y in zip(handle.hullnd_hrep(pts, npts, 6, out=mine_n), mine_n))
        is_dev(handle.hullnd_hrep(pts, npts)[0], (B, 64, D))
        torch.cuda.synchronize()
        assert torch.equal(nn, mine[2]) and (nn >= D + 1).all()
        for i in range(B):
            np.testing.assert_allclose(np.array(_facets(An[i].cpu().numpy(), bn[i].cpu().numpy(), int(nn[i]))),
                                       np.array(_facets(mine[0][i].cpu().numpy(), mine[1][i].cpu().numpy(),
                                                        int(nn[i]))), atol=1e-12)
        q = d(rng.normal(size=(B, D)) * 0.7)
        inside = handle.halfspace_contains(mine[0], mine[1], mine[2], q)
        is_dev(inside, (B,), I32)
        if D == 2:
            in2 = handle.hull2d_contains(mine[0], mine[1], mine[2], q)
            is_dev(in2, (B,), I32)
            torch.cuda.synchronize()
            assert torch.equal(in2, inside)
            refused(ValueError, "query", handle.hull2d_contains, mine[0], mine[1], mine[2], new((B, 3)))
            refused(TypeError, "nfacets", handle.hull2d_contains, mine[0], mine[1], mine[2].long(), q)
        refused(ValueError, "query", handle.halfspace_contains, mine[0], mine[1], mine[2], new((B, D + 1)))
        refused(ValueError, "b has shape", handle.halfspace_contains, mine[0], new((B, 5)), mine[2], q)
        refused(TypeError, "npts", fn, pts, npts.long())
        refused(TypeError, "pts", fn, pts.float(), npts)
        refused(ValueError, "pts", fn, new((B, P_, D + 1)), npts)
        refused(ValueError, "A", fn, pts, npts, 6, out=(new((B, 6, D + 1)), mine[1], mine[2]))
        refused(ValueError, "npts", handle.hullnd_hrep, pts, new((B + 1,), I32))
        refused(ValueError, "nfacets", handle.hullnd_hrep, pts, npts, 6, out=(mine[0], mine[1], new((B, 1), I32)))


# ---- the small systems ----------------------------------------------------------------------------------
def test_lti_rollout_quintic(handle):
    rng = np.random.default_rng(2)
    A, Bm, u, x = d(rng.normal(size=(B, 2, 2))), d(rng.normal(size=(B, 2, 1))), d(rng.normal(size=(B, 1))), \
        d(rng.normal(size=(B, 2)))
    assert handle.lti_euler_integrate(A, Bm, u, x, 0.0, 0.02, 0.01) is x
    assert handle.lti_euler_integrate(A[0].contiguous(), Bm[0].contiguous(), u, x, 0.0, 0.02, 0.01, shared=True) is x
    is_dev(handle.lti_dynamics(A, Bm, u, x), (B, 2))
    refused(ValueError, "A", handle.lti_dynamics, A, Bm, u, x, shared=True)
    refused(ValueError, "B has shape", handle.lti_euler_integrate, A, Bm[0].contiguous(), u, x, 0.0, 0.02, 0.01)
    refused(TypeError, "u", handle.lti_dynamics, A, Bm, u.float(), x)
    xi0, om, vrp = d(rng.normal(size=(B, 2))), d(np.full((B, N), 3.0)), d(rng.normal(size=(B, N, 2)))
    is_dev(handle.dcm_euler_rollout(xi0, om, vrp, 0.02), (B, N + 1, 2))
    out = new((B, N + 1, 2))
    assert handle.dcm_euler_rollout(xi0, om, vrp, 0.02, out=out) is out
    refused(ValueError, "xi_out", handle.dcm_euler_rollout, xi0, om, vrp, 0.02, out=new((B, N, 2)))
    refused(ValueError, "vrp", handle.dcm_euler_rollout, xi0, om, new((B, N + 1, 2)), 0.02)
    kt = d(np.tile([0.0, 0.5, 1.0], (B, 1)))
    co = handle.quintic_fit(kt, d(rng.normal(size=(B, 3, 3, 2))))
    is_dev(co, (B, 2, 2, 6))
    pva, idx = handle.quintic_eval(kt, co, d(rng.uniform(0, 1, (B, 5))))
    is_dev(pva, (B, 5, 3, 2)), is_dev(idx, (B, 5), I32)
    refused(ValueError, "knots_pva", handle.quintic_fit, kt, new((B, 2, 3, 2)))
    refused(ValueError, "coeffs", handle.quintic_eval, kt, new((B, 3, 2, 6)), new((B, 5)))
    torch.cuda.synchronize()


def test_contact_and_rls(handle):
    rng = np.random.default_rng(4)
    prm = d([0.12, 0.09, 3.0e4, 300.0])
    pose = np.zeros((B, 12))
    pose[:, 3:] = np.eye(3).reshape(-1)
    tw, ps, ns = d(rng.normal(size=(B, 6)) * 0.1), d(pose), d(pose)
    out = handle.contact_model_eval(prm, tw, ps, ns)
    shapes = dict(wrench=(B, 6), autonomous=(B, 6), control=(B, 6, 6), regressor=(B, 6, 2))
    assert set(out) == set(shapes)
    for k in shapes:
        is_dev(out[k], shapes[k])
    assert set(handle.contact_model_eval(prm.repeat(B, 1), tw, ps, ns, outputs=("wrench",))) == {"wrench"}
    f, t = handle.contact_point_wrench(prm, tw, ps, ns, d(rng.normal(size=(B, 2, 2)) * 0.01))
    is_dev(f, (B, 2, 3)), is_dev(t, (B, 2, 3))
    refused(ValueError, "params", handle.contact_model_eval, new((B + 1, 4)), tw, ps, ns)
    refused(ValueError, "null_pose", handle.contact_model_eval, prm, tw, ps, new((B, 9)))
    refused(ValueError, "points", handle.contact_point_wrench, prm, tw, ps, ns, new((B + 1, 2, 2)))
    # the filters: in place, with and without the T axis, shared and per-filter covariances
    x, P_ = d(np.zeros((B, 2))), d(np.tile(np.eye(2), (B, 1, 1)))
    reg, meas = d(rng.normal(size=(T, B, 3, 2))), d(rng.normal(size=(T, B, 3)))
    res = handle.rls_advance(reg, meas, x, P_, d(np.ones(3)))
    assert res[0] is x and res[1] is P_
    res = handle.rls_advance(reg[0], meas[0], x, P_, d(np.ones((B, 3))))
    assert res[0] is x and res[1] is P_
    refused(ValueError, "meas_cov", handle.rls_advance, reg, meas, x, P_, new((4,)))
    refused(ValueError, "measurements", handle.rls_advance, reg, new((T, B, 2)), x, P_, new((3,)))
    refused(ValueError, "covariance", handle.rls_advance, reg, meas, x, new((B, 2)), new((3,)))
    wr = d(rng.normal(size=(T, B, 6)))
    twT, psT = tw.repeat(T, 1, 1), ps.repeat(T, 1, 1)
    res = handle.contact_rls_advance(d([0.12, 0.09]), twT, psT, ns, wr, x, P_, d(np.ones(6)))
    assert res[0] is x and res[1] is P_
    res = handle.contact_rls_advance(d(np.tile([0.12, 0.09], (B, 1))), tw, ps, ns, wr[0], x, P_, d(np.ones((B, 6))))
    assert res[0] is x and res[1] is P_
    refused(ValueError, "geometry", handle.contact_rls_advance, new((3,)), twT, psT, ns, wr, x, P_, new((6,)))
    refused(ValueError, "wrench", handle.contact_rls_advance, new((2,)), twT, psT, ns, new((T, B, 5)), x, P_, new((6,)))
    torch.cuda.synchronize()


def test_swing_foot_and_so3_outputs(handle):
    L, C, Q = B, 2, T
    pose = np.zeros((L, C, 12))
    pose[..., 3:] = np.eye(3).reshape(-1)
    pose[:, 1, 0] = 0.1
    args = (d(pose), d(np.tile([[0.0, 0.4], [0.8, 1.2]], (L, 1, 1))), d(np.full(L, C), I32),
            d(np.tile([0.2, 0.6], (L, 1))))
    shapes = dict(pose=((L, Q, 12), F64), twist=((L, Q, 6), F64), accel=((L, Q, 6), F64),
                  contact_idx=((L, Q), I32), in_contact=((L, Q), I32))
    res = handle.swing_foot_eval(*args)
    assert tuple(res) == native.SWING_OUTPUTS
    for k, (shape, dt) in shapes.items():
        is_dev(res[k], shape, dt)
    buf = new((L, Q, 12))
    part = handle.swing_foot_eval(*args, outputs=("pose", "in_contact"), out=dict(pose=buf, accel=new((L, Q, 6))))
    assert set(part) == {"pose", "in_contact"} and part["pose"] is buf
    torch.cuda.synchronize()
    assert torch.equal(part["pose"], res["pose"]) and torch.equal(part["in_contact"], res["in_contact"])
    refused(ValueError, "twist", handle.swing_foot_eval, *args, out=dict(twist=new((L, Q, 12))))
    refused(TypeError, "contact_idx", handle.swing_foot_eval, *args, out=dict(contact_idx=new((L, Q), I64)))
    refused(ValueError, "contact_time", handle.swing_foot_eval, args[0], new((L, C, 3)), args[2], args[3])
    R0 = d(np.tile(np.eye(3), (B, 1, 1)))
    R1 = d(np.stack([robot._rotvec(np.array([0.0, 0.0, 0.3 + i])) for i in range(B)]))
    so = (R0, R1.reshape(B, 9), d(np.ones(B)), d(np.tile([0.25, 0.5], (B, 1))))
    res = handle.so3_eval(*so)
    assert tuple(res) == native.SO3_OUTPUTS
    is_dev(res["rot"], (B, T, 9)), is_dev(res["omega"], (B, T, 3)), is_dev(res["alpha"], (B, T, 3))
    buf = new((B, T, 3))
    part = handle.so3_eval(*so, outputs=("omega",), out=dict(omega=buf))
    assert set(part) == {"omega"} and part["omega"] is buf
    refused(ValueError, "alpha", handle.so3_eval, *so, out=dict(alpha=new((B, T, 9))))
    refused(ValueError, "duration", handle.so3_eval, so[0], so[1], new((B, 1)), so[3])
    torch.cuda.synchronize()


# ---- the floating base: the 3-joint chain ------------------------------------------------------------------
class Chain:
    def __init__(self, handle):
        self.model = FM.tree_model(FM.chain(NJ), seed=5)
        self.dm = handle.fb_model(self.model)
        self.host = robot.random_states(self.model, B, seed=6)
        self.ct = GU.dev_contacts(FM.contact_set(self.model, self.host, [1], seed=8), B)
        pose = np.zeros((B, 1, 12))
        pose[..., 2] = 0.5
        pose[..., 3:] = np.eye(3).reshape(-1)
        self.pose = pose
        self.task_kw = dict(frame=np.array([1], dtype=np.int32), se3_weight=np.ones((1, 6)), se3_kp=np.ones((1, 2)),
                            joint_weight=np.full(NJ, 0.1), joint_kp=np.ones(NJ))
        self.tasks = handle.ik_tasks(B, NJ, se3_pose=pose, joint_pos=np.zeros((B, NJ)), **self.task_kw)
        self.hard = handle.ik_hard(se3=[[True] * 3 + [False] * 3])
        self.limits = handle.ik_limits(np.full(NJ, -2.0), np.full(NJ, 2.0), np.full(NJ, 0.5), vel_max=np.full(NJ, 9.0))
        self.schedule = handle.ik_schedule(B, 1, T, stance_rows=0x7, contact=np.ones((B, 1, T), dtype=np.int32),
                                           se3_pose=np.repeat(pose[:, :, None], T, axis=2))

    def state(self, rows=B):
        return GU.dev_state(self.host, slice(0, rows))

    def torque(self):
        return d(self.host["joint_torque"])


@pytest.fixture(scope="module")
def chain(handle):
    return Chain(handle)


def state_is(st):
    shapes = dict(base_vel=(B, 6), joint_vel=(B, NJ), base_pos=(B, 3), base_rot=(B, 3, 3), joint_pos=(B, NJ))
    assert tuple(st) == native.FB_STATE_KEYS
    for k in shapes:
        is_dev(st[k], shapes[k])


def test_holders(handle, chain):
    """What fb_model, posture_law, ik_tasks, ik_limits, ik_schedule and the trajectory laws return: the
    struct (.c), the tensors it points to (.t) and the sizes later calls read."""
    dm = chain.dm
    assert isinstance(dm.c, native.FbModel) and dm.n == NJ == dm.c.ndof and dm.c.nframes == 4
    assert set(dm.t) == {"parent", "joint_origin", "joint_rot", "joint_axis", "link_mass", "link_com",
                         "link_inertia", "frame_link", "frame_pose"}
    for k, t in dm.t.items():
        assert t.is_cuda and t.dtype == (I32 if k in ("parent", "frame_link") else F64)
        assert getattr(dm.c, k) == t.data_ptr(), k
    assert dm.c.joint_type is None and tuple(dm.c.gravity) == (0.0, 0.0, -9.81) and dm.c.rho == 0.01
    pri = handle.fb_model(dict(chain.model, joint_type=[0, 1, 0]), rho=0.5, gravity=(0.0, 1.0, 2.0))
    is_dev(pri.t["joint_type"], (NJ,), I32)
    assert pri.c.joint_type == pri.t["joint_type"].data_ptr() and pri.c.rho == 0.5 and tuple(pri.c.gravity) == (0.0, 1.0, 2.0)
    refused(ValueError, "joint_type", handle.fb_model, dict(chain.model, joint_type=[0, 2, 0]))
    tk = chain.tasks
    assert isinstance(tk.c, native.IkTasks) and (tk.batch, tk.n, tk.c.nse3) == (B, NJ, 1)
    assert set(tk.t) == {"frame", "se3_weight", "se3_kp", "se3_pose", "joint_weight", "joint_kp", "joint_pos"}
    is_dev(tk.t["frame"], (1,), I32), is_dev(tk.t["se3_pose"], (B, 1, 12))
    own = d(chain.pose)
    assert handle.ik_tasks(B, NJ, se3_pose=own, joint_pos=np.zeros((B, NJ)), **chain.task_kw).t["se3_pose"] is own
    refused(ValueError, "se3_pose", handle.ik_tasks, B, NJ, se3_pose=np.zeros((B, 2, 12)), **chain.task_kw)
    refused(TypeError, "joint_pos", handle.ik_tasks, B, NJ, joint_pos=new((B, NJ), torch.float32), **chain.task_kw)
    none = handle.ik_tasks(B, NJ, joint_weight=np.ones(NJ), joint_kp=np.ones(NJ), com_weight=np.ones(3), com_kp=2.0,
                           base_damping=0.5)
    assert none.c.nse3 == 0 and none.c.frame is None and (none.c.com_kp, none.c.base_damping) == (2.0, 0.5)
    lm = chain.limits
    assert isinstance(lm.c, native.IkLimits) and lm.n == NJ and set(lm.t) == {"pos_lower", "pos_upper", "klim", "vel_max"}
    assert (lm.c.sampling_time, lm.c.max_iter) == (0.01, 0) and lm.c.klim == lm.t["klim"].data_ptr()
    assert handle.ik_limits(np.zeros(NJ), np.ones(NJ), np.ones(NJ)).c.vel_max is None
    refused(ValueError, "klim", handle.ik_limits, np.zeros(NJ), np.ones(NJ), np.ones(NJ + 1))
    sc = chain.schedule
    assert isinstance(sc.c, native.IkSchedule) and (sc.batch, sc.nse3, sc.steps) == (B, 1, T)
    assert (sc.c.steps, sc.c.stance_rows) == (T, 0x7) and set(sc.t) == {"contact", "se3_pose"}
    flat = d(np.zeros((B * 1, T, 12)))                     # swing_foot_eval's layout is passed on as it stands
    assert handle.ik_schedule(B, 1, T, se3_pose=flat).t["se3_pose"] is flat
    refused(ValueError, "ik_schedule: se3_pose", handle.ik_schedule, B, 1, T, se3_pose=np.zeros((B, 1, T + 1, 12)))
    refused(ValueError, "ik_schedule: com_pos", handle.ik_schedule, B, 1, T, com_pos=np.zeros((B, T, 2)))
    refused(TypeError, "contact", handle.ik_schedule, B, 1, T, contact=new((B, 1, T), I64))
    h = chain.hard
    assert isinstance(h, native.IkHard) and (h.rows, h.rel_pivot_min) == (0x7, 0.0)
    assert native.Handle.ik_hard(com=(True, False, True), rel_pivot_min=1e-6).rows == (1 << 24) | (1 << 26)
    refused(ValueError, "ik_hard", handle.ik_hard, se3=[[True] * 5])
    refused(ValueError, "ik_hard", handle.ik_hard, com=(True, True))
    refused(ValueError, "ik_hard", handle.ik_hard, se3=[[False] * 6] * 5)
    law = handle.posture_law(np.zeros(NJ), np.ones((NJ, 2)))
    assert isinstance(law.c, native.PostureLaw) and law.c.ndof == NJ and set(law.t) == {"q_nominal", "lean"}
    assert law.c.lean == law.t["lean"].data_ptr()
    refused(ValueError, "posture law", handle.posture_law, np.zeros(NJ), np.ones((NJ, 3)))
    imp = handle.joint_impedance(np.ones(NJ), np.ones(NJ))
    assert set(imp) == {"kp", "kd"}
    is_dev(imp["kp"], (NJ,)), is_dev(imp["kd"], (NJ,))


def test_fbk_and_fbd_calls(handle, chain):
    st = chain.state()
    dp, dR, dq = handle.fbk_dynamics(0.01, st["base_rot"], st["base_vel"], st["joint_vel"])
    is_dev(dp, (B, 3)), is_dev(dR, (B, 3, 3)), is_dev(dq, (B, NJ))
    res = handle.fbk_euler_integrate(0.01, st["base_pos"], st["base_rot"], st["joint_pos"], st["base_vel"],
                                     st["joint_vel"], 0.0, 0.002, 0.001)
    assert res[0] is st["base_pos"] and res[1] is st["base_rot"] and res[2] is st["joint_pos"]
    refused(ValueError, "twist", handle.fbk_dynamics, 0.01, st["base_rot"], new((B, 5)), st["joint_vel"])
    refused(ValueError, "rot", handle.fbk_euler_integrate, 0.01, st["base_pos"], new((B, 9)), st["joint_pos"],
            st["base_vel"], st["joint_vel"], 0.0, 0.002, 0.001)
    st, tau = chain.state(), chain.torque()
    for ct, reg in ((None, None), (chain.ct, d(np.zeros((NJ + 6, NJ + 6))))):
        state_is(handle.fbd_dynamics(chain.dm, st, tau, contacts=ct, mass_reg=reg))
        assert handle.fbd_euler_integrate(chain.dm, st, tau, 0.0, 0.002, 0.001, contacts=ct, mass_reg=reg) is st
    refused(ValueError, "torque", handle.fbd_dynamics, chain.dm, st, new((B, NJ + 1)))
    refused(ValueError, "mass_reg", handle.fbd_dynamics, chain.dm, st, tau, mass_reg=new((NJ, NJ)))
    refused(ValueError, "base_rot", handle.fbd_dynamics, chain.dm, dict(st, base_rot=new((B, 9))), tau)
    refused(TypeError, "joint_vel", handle.fbd_euler_integrate, chain.dm, dict(st, joint_vel=st["joint_vel"].float()),
            tau, 0.0, 0.002, 0.001)
    refused(ValueError, "null_pose", handle.fbd_dynamics, chain.dm, st, tau,
            contacts=dict(chain.ct, null_pose=new((B + 1, 1, 12))))
    refused(TypeError, "frame", handle.fbd_dynamics, chain.dm, st, tau, contacts=dict(chain.ct, frame=new((1,), I64)))
    refused(ValueError, "wrench", handle.fbd_dynamics, chain.dm, st, tau,
            contacts=dict(chain.ct, law=d([1], I32), wrench=new((B, 1, 5))))
    frames = d([0, 3], I32)
    pose, twist = handle.fb_frame_state(chain.dm, st, frames)
    is_dev(pose, (B, 2, 12)), is_dev(twist, (B, 2, 6))
    got = handle.fb_frame_state(chain.dm, st, frames, pose=pose, twist=twist)
    assert got[0] is pose and got[1] is twist
    refused(TypeError, "frames", handle.fb_frame_state, chain.dm, st, frames.long())
    refused(ValueError, "pose", handle.fb_frame_state, chain.dm, st, frames, pose=new((B, 2, 6)))
    torch.cuda.synchronize()


def test_fb_inverse_dynamics_outputs(handle, chain):
    st = chain.state()
    free = handle.fb_inverse_dynamics(chain.dm, st)
    assert set(free) == {"joint_torque", "status", "base_acc"}
    is_dev(free["joint_torque"], (B, NJ)), is_dev(free["base_acc"], (B, 6)), is_dev(free["status"], (B,), I32)
    given = handle.fb_inverse_dynamics(chain.dm, st, joint_acc=d(np.zeros((B, NJ))), base_acc=d(np.zeros((B, 6))),
                                       contacts=chain.ct)
    assert set(given) == {"joint_torque", "status", "base_wrench"}
    is_dev(given["base_wrench"], (B, 6))
    tau, acc, wr, stat = new((B, NJ)), new((B, 6)), new((B, 6)), new((B,), I32)
    got = handle.fb_inverse_dynamics(chain.dm, st, joint_torque=tau, base_acc_out=acc, status=stat)
    assert got["joint_torque"] is tau and got["base_acc"] is acc and got["status"] is stat
    got = handle.fb_inverse_dynamics(chain.dm, st, base_acc=acc, joint_torque=tau, base_wrench=wr, status=False)
    assert got["joint_torque"] is tau and got["base_wrench"] is wr and got["status"] is None
    torch.cuda.synchronize()
    assert (free["status"] == 0).all()
    refused(ValueError, "base_acc_out", handle.fb_inverse_dynamics, chain.dm, st, base_acc_out=new((B, 5)))
    refused(ValueError, "base_wrench", handle.fb_inverse_dynamics, chain.dm, st, base_acc=acc, base_wrench=new((B, 5)))
    refused(ValueError, "joint_acc", handle.fb_inverse_dynamics, chain.dm, st, joint_acc=new((B, NJ + 1)))
    refused(ValueError, "base_acc", handle.fb_inverse_dynamics, chain.dm, st, base_acc=new((B, 7)))
    refused(ValueError, "joint_torque", handle.fb_inverse_dynamics, chain.dm, st, joint_torque=new((B + 1, NJ)))
    refused(TypeError, "status", handle.fb_inverse_dynamics, chain.dm, st, status=new((B,), I64))


def test_fb_ik_solve_and_integrate_outputs(handle, chain):
    """The plain, hard and limits entry points through both wrappers: allocated, given and False outputs."""
    dm, tk = chain.dm, chain.tasks
    for kw in ({}, dict(hard=chain.hard), dict(limits=chain.limits), dict(hard=chain.hard, limits=chain.limits)):
        lim = "limits" in kw
        st = chain.state()
        res = handle.fb_ik_solve(dm, st, tk, **kw)
        assert len(res) == (4 if lim else 2)
        is_dev(res[0], (B, 6 + NJ)), is_dev(res[1], (B,), I32)
        nu, stat = new((B, 6 + NJ)), new((B,), I32)
        got = handle.fb_ik_solve(dm, st, tk, nu=nu, status=stat, **kw)
        assert got[0] is nu and got[1] is stat
        assert handle.fb_ik_solve(dm, st, tk, status=False, **kw)[1] is None
        res = handle.fb_ik_integrate(dm, st, tk, T, 0.01, **kw)
        assert len(res) == (5 if lim else 3) and res[0] is st
        is_dev(res[1], (B, 6 + NJ)), is_dev(res[2], (B,), I32)
        got = handle.fb_ik_integrate(dm, st, tk, T, 0.01, nu=nu, status=stat, **kw)
        assert got[0] is st and got[1] is nu and got[2] is stat
        got = handle.fb_ik_integrate(dm, st, tk, T, 0.01, nu=False, status=False, **kw)
        assert got[0] is st and got[1] is None and got[2] is None
        if lim:
            it, ac = new((B,), I32), new((B, 2), I64)
            for call, at in ((lambda **k: handle.fb_ik_solve(dm, st, tk, **kw, **k), 2),
                             (lambda **k: handle.fb_ik_integrate(dm, st, tk, T, 0.01, **kw, **k), 3)):
                res = call()
                is_dev(res[at], (B,), I32), is_dev(res[at + 1], (B, 2), I64)
                res = call(iters=it, active=ac)
                assert res[at] is it and res[at + 1] is ac
                res = call(iters=False, active=False)
                assert res[at] is None and res[at + 1] is None
                res = call(iters=False)
                assert res[at] is None and tuple(res[at + 1].shape) == (B, 2)
                refused(TypeError, "active", call, active=new((B, 2), I32))
                refused(ValueError, "iters", call, iters=new((B, 1), I32))
        torch.cuda.synchronize()
    st = chain.state()
    refused(ValueError, "nu", handle.fb_ik_solve, dm, st, tk, nu=new((B, NJ)))
    for kw in ({}, dict(hard=chain.hard), dict(limits=chain.limits)):   # a solve without nu is no solve
        refused(TypeError, "nu must be a torch tensor", handle.fb_ik_solve, dm, st, tk, nu=False, **kw)
    refused(ValueError, "nu", handle.fb_ik_integrate, dm, st, tk, T, 0.01, nu=new((B, NJ)), hard=chain.hard)
    refused(TypeError, "status", handle.fb_ik_solve, dm, st, tk, status=new((B,), I64), limits=chain.limits)
    refused(ValueError, "base_pos", handle.fb_ik_integrate, dm, dict(st, base_pos=new((B, 2))), tk, T, 0.01)


def track_outputs(b):
    return dict(joint_traj=((T, b, NJ), F64), base_traj=((T, b, 12), F64), nu_traj=((T, b, 6 + NJ), F64),
                status=((b,), I32), fail_step=((b,), I32), iters=((b,), I32), active=((b, 2), I64))


TRACK = track_outputs(B)


def test_fb_ik_track_outputs(handle, chain):
    dm, tk, sc = chain.dm, chain.tasks, chain.schedule
    st = chain.state()
    res = handle.fb_ik_track(dm, st, tk, sc, 0.01, hard=chain.hard, limits=chain.limits)
    assert set(res) == set(TRACK) | {"state"} and res["state"] is st
    for k, (shape, dt) in TRACK.items():
        is_dev(res[k], shape, dt)
    mine = {k: new(*TRACK[k]) for k in TRACK}
    got = handle.fb_ik_track(dm, st, tk, sc, 0.01, **mine)
    assert all(got[k] is mine[k] for k in TRACK)
    got = handle.fb_ik_track(dm, st, tk, sc, 0.01, **{k: False for k in TRACK})
    assert set(got) == set(TRACK) | {"state"} and all(got[k] is None for k in TRACK)
    got = handle.fb_ik_track(dm, st, tk, sc, 0.01, nu_traj=False, iters=False)
    assert got["nu_traj"] is None and got["iters"] is None and got["status"] is not None
    torch.cuda.synchronize()
    refused(ValueError, "base_traj", handle.fb_ik_track, dm, st, tk, sc, 0.01, base_traj=new((T, B, 9)))
    refused(TypeError, "fail_step", handle.fb_ik_track, dm, st, tk, sc, 0.01, fail_step=new((B,), I64))
    refused(ValueError, "joint_traj", handle.fb_ik_track, dm, st, tk, sc, 0.01, joint_traj=new((T + 1, B, NJ)))


def test_zero_filled_outputs_on_an_empty_batch(handle, chain):
    """iters / active of the limits calls and every output of fb_ik_track are allocated with zeros.  The
    kernels write every robot of a batch (a failed robot's entries are NaN or 0 by the header), so there is
    no robot they leave alone: the fill is asserted on B = 0 calls, which the library accepts."""
    st = chain.state(0)
    tk = handle.ik_tasks(0, NJ, se3_pose=np.zeros((0, 1, 12)), joint_pos=np.zeros((0, NJ)), **chain.task_kw)
    res = handle.fb_ik_solve(chain.dm, st, tk, limits=chain.limits)
    assert tuple(res[2].shape) == (0,) and tuple(res[3].shape) == (0, 2) and not res[2].any() and not res[3].any()
    res = handle.fb_ik_integrate(chain.dm, st, tk, T, 0.01, limits=chain.limits)
    assert tuple(res[3].shape) == (0,) and tuple(res[4].shape) == (0, 2) and not res[3].any() and not res[4].any()
    sc = handle.ik_schedule(0, 1, T, se3_pose=np.zeros((0, 1, T, 12)))
    res = handle.fb_ik_track(chain.dm, st, tk, sc, 0.01, limits=chain.limits)
    for k, (shape, dt) in track_outputs(0).items():
        assert tuple(res[k].shape) == shape and res[k].dtype == dt and not res[k].any(), k
    torch.cuda.synchronize()


def test_closed_loop_maps(handle, chain):
    """fb_dcm, posture_reference, dcm_com_reference and the three control-law integrations."""
    dm, st = chain.dm, chain.state()
    com, xi = handle.fb_dcm(dm, st)
    is_dev(com, (B, 6))
    assert xi is None
    omega = d(np.full((B, 2), 3.0))
    com2, xi = handle.fb_dcm(dm, st, omega=omega, column=1, com=com)
    assert com2 is com
    is_dev(xi, (B, 2))
    assert handle.fb_dcm(dm, st, omega=omega, xi=xi)[1] is xi
    refused(ValueError, "omega column 2", handle.fb_dcm, dm, st, omega=omega, column=2)
    refused(ValueError, "omega column -1", handle.fb_dcm, dm, st, omega=omega, column=-1)
    refused(ValueError, "xi requested without omega", handle.fb_dcm, dm, st, xi=xi)
    refused(TypeError, "omega", handle.fb_dcm, dm, st, omega=omega.float())
    refused(ValueError, "com", handle.fb_dcm, dm, st, com=new((B, 3)))
    law = handle.posture_law(np.zeros(NJ), np.full((NJ, 2), 0.1))
    vrp = d(np.zeros((B, N, 2)))
    q_ref = handle.posture_reference(law, com, vrp)
    is_dev(q_ref, (B, NJ))
    assert handle.posture_reference(law, com, vrp, q_ref=q_ref) is q_ref
    refused(ValueError, "q_ref", handle.posture_reference, law, com, vrp, q_ref=new((B, NJ + 1)))
    refused(ValueError, "com", handle.posture_reference, law, new((B, 3)), vrp)
    # dcm_com_reference
    z, c = d(np.full(B, 0.7)), d(np.zeros((B, 2)))
    pos, vel, end = handle.dcm_com_reference(xi, vrp, omega, z, c, T, 0.01, column=1)
    is_dev(pos, (B, T, 3)), is_dev(vel, (B, T, 3)), is_dev(end, (B, 2))
    got = handle.dcm_com_reference(xi, vrp, omega, z, c, T, 0.01, com_pos=pos, com_vel=vel, xi_end=end)
    assert got[0] is pos and got[1] is vel and got[2] is end
    assert handle.dcm_com_reference(xi, vrp, omega, z, c, T, 0.01, xi_end=False)[2] is None
    refused(ValueError, "omega column 2", handle.dcm_com_reference, xi, vrp, omega, z, c, T, 0.01, column=2)
    refused(ValueError, "com_vel", handle.dcm_com_reference, xi, vrp, omega, z, c, T, 0.01, com_vel=new((B, T + 1, 3)))
    refused(ValueError, "z_ref", handle.dcm_com_reference, xi, vrp, omega, new((B, 1)), c, T, 0.01)
    refused(ValueError, "c_ref", handle.dcm_com_reference, xi, vrp, omega, z, c.t(), T, 0.01)
    # the control laws
    imp = handle.joint_impedance(np.full(NJ, 20.0), np.full(NJ, 2.0))
    assert handle.fbd_euler_integrate_impedance(dm, st, imp, q_ref, 0.0, 0.002, 0.001, contacts=chain.ct) is st
    refused(ValueError, "q_ref", handle.fbd_euler_integrate_impedance, dm, st, imp, new((B + 1, NJ)), 0.0, 0.002, 0.001)
    refused(ValueError, "kp", handle.fbd_euler_integrate_impedance, dm, st, dict(imp, kp=new((NJ + 1,))), q_ref,
            0.0, 0.002, 0.001)
    qT, nuT = d(np.zeros((T, B, NJ))), d(np.zeros((T, B, 6 + NJ)))
    bias = d(np.zeros((B, NJ)))
    tr = handle.joint_impedance_traj(imp, qT, 1, qd_ref=nuT, qd_offset=6, q_bias=bias)
    assert isinstance(tr.c, native.JointImpedanceTraj) and tr.batch == B
    assert (tr.c.ndof, tr.c.slices, tr.c.steps_per_slice, tr.c.qd_stride) == (NJ, T, 1, 6 + NJ)
    assert tr.c.qd_ref == nuT.data_ptr() + 48 and tr.c.q_bias == bias.data_ptr()
    assert tr.t["q_ref"] is qT and tr.t["qd_ref"] is nuT and tr.t["q_bias"] is bias and tr.t["kp"] is imp["kp"]
    assert handle.joint_impedance_traj(imp, qT, 2).c.qd_ref is None
    assert handle.fbd_euler_integrate_impedance_traj(dm, st, tr, 0.0, 0.002, 0.001, contacts=chain.ct) is st
    refused(ValueError, r"qd_ref: columns 7\.\.10", handle.joint_impedance_traj, imp, qT, 1, qd_ref=nuT, qd_offset=7)
    refused(ValueError, r"qd_ref: columns -1\.\.2", handle.joint_impedance_traj, imp, qT, 1, qd_ref=nuT, qd_offset=-1)
    refused(ValueError, "q_bias", handle.joint_impedance_traj, imp, qT, 1, q_bias=new((B, NJ + 1)))
    refused(ValueError, "the trajectory holds 3 robots, the state 2", handle.fbd_euler_integrate_impedance_traj, dm,
            chain.state(2), tr, 0.0, 0.002, 0.001)
    ct = handle.computed_torque_traj(100.0, np.full(NJ, 20.0), qT, 1, qd_ref=nuT, qd_offset=6, qdd_ref=nuT,
                                     qdd_offset=6, q_bias=bias, tau_max=50.0, tau_last=True)
    assert isinstance(ct.c, native.ComputedTorqueTraj) and ct.batch == B
    is_dev(ct.tau_last, (B, NJ)), is_dev(ct.t["kp"], (NJ,)), is_dev(ct.t["tau_max"], (NJ,))
    assert ct.t["tau_last"] is ct.tau_last and ct.c.tau_last == ct.tau_last.data_ptr()
    assert (ct.c.qd_stride, ct.c.qdd_stride) == (6 + NJ, 6 + NJ) and ct.c.qdd_ref == nuT.data_ptr() + 48
    plain = handle.computed_torque_traj(imp["kp"], imp["kd"], qT, 1)
    assert plain.tau_last is None and plain.t["kp"] is imp["kp"] and plain.c.tau_max is None and plain.c.qd_ref is None
    last = new((B, NJ))
    assert handle.computed_torque_traj(1.0, 1.0, qT, 1, tau_last=last).tau_last is last
    assert handle.fbd_euler_integrate_computed_torque_traj(dm, st, ct, 0.0, 0.002, 0.001, contacts=chain.ct) is st
    refused(ValueError, r"qdd_ref: columns 7\.\.10", handle.computed_torque_traj, 1.0, 1.0, qT, 1, qdd_ref=nuT,
            qdd_offset=7)
    refused(ValueError, "tau_max", handle.computed_torque_traj, 1.0, 1.0, qT, 1, tau_max=[1.0, -1.0, 1.0])
    refused(ValueError, "tau_max", handle.computed_torque_traj, 1.0, 1.0, qT, 1, tau_max=float("inf"))
    refused(ValueError, "tau_last", handle.computed_torque_traj, 1.0, 1.0, qT, 1, tau_last=new((B, NJ + 1)))
    refused(ValueError, "kd", handle.computed_torque_traj, 1.0, np.ones(NJ + 1), qT, 1)
    refused(ValueError, "the trajectory holds 3 robots, the state 2", handle.fbd_euler_integrate_computed_torque_traj,
            dm, chain.state(2), ct, 0.0, 0.002, 0.001)
    torch.cuda.synchronize()


def test_ptr_checks_in_order():
    """_ptr: tensor, device, dtype, contiguity, shape -- each message with the argument's name; a tensor with
    several defects reports the first of them."""
    t = new((4, 3)).t()
    refused(TypeError, "arg must be a torch tensor", native._ptr, [1.0], F64, None, "arg")
    refused(ValueError, "arg must be a device", native._ptr, torch.zeros(2, dtype=torch.float32), F64, (3,), "arg")
    refused(TypeError, "arg must be torch.float64", native._ptr, t.float(), F64, (9,), "arg")
    refused(ValueError, "arg must be contiguous", native._ptr, t, F64, (9,), "arg")
    refused(ValueError, r"arg has shape \(4, 3\), expected \(3, 4\)", native._ptr, t.t(), F64, (3, 4), "arg")
    refused(TypeError, "tensor must be", native._ptr, None, F64)
    x = new((2, 2))
    assert native._ptr(x, F64).value == x.data_ptr() == native._ptr(x, F64, (2, 2), "x").value
