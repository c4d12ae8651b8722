"""CPU tests of tests/fb_models.py: the tree builders, the floating-base oracle
(oracle/fb_dynamics.py) on trees other than the humanoid, and the conditioning of every case of the
GPU matrix (tests/test_gpu_fb_topologies.py).

The oracle identities are those of tests/test_fb_dynamics.py (same helpers and tolerances) on the
deepest, the widest, a level-numbered and a random tree of the largest size, some joints prismatic.
The conditioning test bounds the oracle's own solve error on every system the GPU tests compare
at a tenth of their 1e-9 bar, so that comparison measures the kernel and not LAPACK."""
import numpy as np
import pytest

import fb_dynamics as F
import fb_models as FM
import oracle as O
from blf import robot
from test_fb_dynamics import state_i

N = 48
TREES = {
    "chain": FM.tree_model(FM.chain(N), 1, prismatic=[0, 20, 21, N - 1]),
    "star": FM.tree_model(FM.star(N), 2, prismatic=[0, 7, N - 1]),
    "bfs_binary": FM.tree_model(FM.bfs_binary(N), 3, prismatic=[0, 1, 3, N - 1]),
    "random_tree": FM.tree_model(FM.random_tree(N, 4), 4, prismatic=[0, 5, 30, N - 1]),
}


def test_topology_builders():
    assert FM.chain(4) == [0, 1, 2, 3] and FM.star(3) == [0, 0, 0]
    assert FM.bfs_binary(6) == [0, 0, 1, 1, 2, 2]
    p = FM.random_tree(48, 5)
    assert all(0 <= p[j] <= j for j in range(48)) and p == FM.random_tree(48, 5)
    assert FM.depths(FM.chain(5)) == [0, 1, 2, 3, 4] and FM.depths(FM.star(3)) == [0, 0, 0]
    # the predicate: chains, stars and the humanoid are in DFS preorder, a level order is not
    assert FM.is_dfs_preorder(FM.chain(9)) and FM.is_dfs_preorder(FM.star(9))
    assert FM.is_dfs_preorder(robot.humanoid24()["parent"])
    assert FM.is_dfs_preorder(FM.bfs_binary(2)) and not FM.is_dfs_preorder(FM.bfs_binary(4))
    assert FM.is_dfs_preorder([0, 1, 1, 0, 4]) and not FM.is_dfs_preorder([0, 0, 1])


def test_tree_model_parameters():
    m = TREES["random_tree"]
    assert m["link_mass"][0] == 8.0 and (m["link_mass"][1:] >= 0.4).all()
    np.testing.assert_allclose(np.linalg.norm(m["joint_axis"], axis=1), 1.0, atol=1e-15)
    assert (np.sort(np.abs(m["joint_axis"]), axis=1)[:, 1] > 1e-3).all()   # not the coordinate axes
    for l in range(N + 1):
        d = np.linalg.eigvalsh(m["link_inertia"][l])
        assert d[0] > 0 and d[2] < d[0] + d[1]                 # the triangle inequality
    for f in range(len(m["frame_link"])):
        R = m["frame_pose"][f, 3:].reshape(3, 3)
        np.testing.assert_allclose(R @ R.T, np.eye(3), atol=1e-14)
        assert np.abs(R - np.eye(3)).max() > 1e-3 and np.abs(m["frame_pose"][f, :3]).max() > 1e-3
    assert abs(m["joint_origin"][:, 2].mean() + 0.1) < 0.02


@pytest.mark.parametrize("kind", sorted(TREES))
def test_mass_matrix_and_energy_on_trees(kind):
    MODEL = TREES[kind]
    st = state_i(robot.random_states(MODEL, 1, seed=5), 0)
    K = F.kinematics(MODEL, st["base_pos"], st["base_rot"], st["joint_pos"], st["base_vel"], st["joint_vel"])
    M, h = F.mass_and_bias(MODEL, K)
    assert np.abs(M - M.T).max() < 1e-13
    assert np.linalg.eigvalsh(M).min() > 0
    np.testing.assert_allclose(M[:3, :3], MODEL["link_mass"].sum() * np.eye(3), atol=1e-12)
    nu = np.concatenate([st["base_vel"], st["joint_vel"]])
    T = 0.0
    for l in range(MODEL["n"] + 1):
        R = K["R"][l]
        c = K["p"][l] + R @ MODEL["link_com"][l]
        vc = K["v"][l] + np.cross(K["w"][l], c - K["p"][l])
        T += 0.5 * MODEL["link_mass"][l] * vc @ vc
        T += 0.5 * K["w"][l] @ (R @ MODEL["link_inertia"][l] @ R.T) @ K["w"][l]
    assert abs(0.5 * nu @ M @ nu - T) < 1e-12 * max(1.0, T)


@pytest.mark.parametrize("kind", sorted(TREES))
def test_equation_of_motion_with_contacts_on_trees(kind):
    MODEL = TREES[kind]
    st = robot.random_states(MODEL, 2, seed=4)
    ct = FM.contact_set(MODEL, st, [0, 1, 2, 2], seed=9)
    for i in range(2):
        ba, ja, dp, dR, dq = F.dynamics(MODEL, st, i, **FM.oracle_kw(ct, i))
        s = state_i(st, i)
        K = F.kinematics(MODEL, s["base_pos"], s["base_rot"], s["joint_pos"], s["base_vel"], s["joint_vel"])
        M, h = F.mass_and_bias(MODEL, K)
        rhs = -h.copy()
        rhs[6:] += s["joint_torque"]
        for c, f in enumerate(ct["frame"]):
            pf, Rf, vel, J = F.frame_state(MODEL, K, f)
            wr = O.contact_eval(ct["params"][c], vel, np.concatenate([pf, Rf.reshape(-1)]),
                                ct["null_pose"][i][c])[0]
            assert 1e-3 < np.abs(wr[:3]).max() < 1e3            # null_poses_near: a physical force
            rhs += J.T @ wr
        acc = np.concatenate([ba, ja])
        np.testing.assert_allclose(M @ acc, rhs, atol=1e-8 * np.abs(rhs).max())
        np.testing.assert_array_equal(dp, s["base_vel"][:3])
        np.testing.assert_array_equal(dq, s["joint_vel"])
        # the helper the conditioning test and the GPU tests use assembles the same system
        A, b = FM.system_matrices(MODEL, st, i, ct)
        np.testing.assert_array_equal(A, M)
        np.testing.assert_allclose(b, rhs, rtol=0, atol=1e-12 * np.abs(rhs).max())


@pytest.mark.parametrize("kind", ["bfs_binary", "random_tree"])
def test_dfs_relabel_is_the_same_physical_tree(kind):
    """The relabelled model is in DFS preorder, has the same M up to the permutation, the same
    frames and the same accelerations (contacts included) on the oracle."""
    MODEL = TREES[kind]
    red = FM.dfs_relabel(MODEL)
    assert not FM.is_dfs_preorder(MODEL["parent"]) and FM.is_dfs_preorder(red["parent"])
    perm = red["perm"]
    rows = list(range(6)) + [6 + j for j in perm]
    st = robot.random_states(MODEL, 2, seed=6)
    sr = FM.permute_states(st, perm)
    ct = FM.contact_set(MODEL, st, [0, 1, 3], seed=2)
    cr = FM.contact_set(red, sr, [0, 1, 3], seed=2)
    for i in range(2):
        A, b = FM.system_matrices(MODEL, st, i, ct)
        Ar, br = FM.system_matrices(red, sr, i, cr)
        np.testing.assert_allclose(Ar, A[np.ix_(rows, rows)], rtol=0, atol=1e-12 * np.abs(A).max())
        np.testing.assert_allclose(br, b[rows], rtol=0, atol=1e-11 * np.abs(b).max())
        a = np.concatenate(F.dynamics(MODEL, st, i, **FM.oracle_kw(ct, i))[:2])
        ar = np.concatenate(F.dynamics(red, sr, i, **FM.oracle_kw(cr, i))[:2])
        assert FM.rel_err(ar, a[rows]) < 1e-9


def test_gpu_matrix_drives_the_arms_it_names():
    """The topology of every case of the GPU matrix is what its id says."""
    for cid, (topo, n, seed, opt) in FM.CASES.items():
        cs = FM.build_case(cid)
        parent = [int(p) for p in cs["model"]["parent"]]
        dfs = FM.is_dfs_preorder(parent)
        want = topo in ("chain", "star") or bool(opt.get("relabel")) or n <= 2
        assert dfs == want, cid
        assert cs["B"] == (5 if n <= 26 else 3), cid
        if topo == "chain":
            assert max(FM.depths(parent)) == n - 1, cid
        if topo == "star":
            assert max(FM.depths(parent)) == 0 and parent.count(0) == n, cid
    for cid in ("rand26-c8", "bfs48-c8", "rand48-c8mixed"):
        m = FM.build_case(cid)["model"]
        fl = [int(l) for l in m["frame_link"]]
        parent = [int(p) for p in m["parent"]]
        d = FM.depths(parent)
        assert len(fl) == 8 and fl[0] == 0 and fl[4] == m["n"], cid
        assert d[fl[1] - 1] == max(d) and fl[1] not in parent, cid          # the deepest leaf
        assert fl[2] == fl[3] and fl[2] in parent and fl[2] > 0, cid         # two on one interior link
    for cid in ("pri-chain26-c2", "pri-rand48-c2"):
        m = FM.build_case(cid)["model"]
        pri = [j for j in range(m["n"]) if m["joint_type"][j] == 1]
        assert 0 in pri and m["n"] - 1 in pri, cid
        assert any(0 < j < m["n"] - 1 and int(m["parent"][k]) == j + 1 for j in pri for k in pri), cid


def case_self_errors(cid, kinds):
    """max over the case's systems of rel_err(oracle's solve, refined solve), per kind."""
    cs = FM.build_case(cid)
    out = {}
    for kind in kinds:
        reg = FM.reg_of(cs["model"], "reg") if kind == "reg" else None
        worst = 0.0
        for i in range(cs["B"]):
            A, b = FM.system_matrices(cs["model"], cs["states"], i, cs["contacts"], reg)
            a = np.concatenate(FM.reference(cid, kind)[0][i][:2])
            worst = max(worst, FM.rel_err(a, FM.refined_solve(A, b).astype(np.float64)))
        out[kind] = worst
    return out


def test_oracle_self_error_over_the_gpu_matrix():
    """Condition on the inputs: on every system of every run of the GPU matrix the oracle's own
    Cholesky solve is within 1e-10 (a tenth of the 1e-9 bar) of np.linalg.solve improved by five
    rounds of iterative refinement with np.longdouble residuals.  Measured: the n = 48 chains
    1.6e-11 (1.1e-12 with the regularisation), the 26- to 33-joint chains 2e-13 to 6e-12, chain9
    3e-14, every other tree below 3e-15."""
    kinds = {}
    for cid, solve in FM.RUNS:   # mass_reg = zeros is the unregularised system ("none")
        kinds.setdefault(cid, set()).update(("none",) if solve == "aba" else ("none", "reg"))
    assert set(kinds) == set(FM.CASES)
    worst = {}
    for cid in FM.CASES:
        for k, e in case_self_errors(cid, sorted(kinds[cid])).items():
            worst[(cid, k)] = e
            print(f"{cid:22s} {k:5s} oracle self-error {e:.2e}")
    bad = {k: v for k, v in worst.items() if not v <= 1e-10}
    assert not bad, bad
