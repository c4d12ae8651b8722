"""The case matrix of the joint-limit IK tests (include/blf/blf_c.h section 12c):
tests/test_ik_limits_reference.py (CPU: certificate, conditioning band, default max_iter) and
tests/test_gpu_ik_limits.py (blf_fb_ik_solve_limits / blf_fb_ik_integrate_limits against
tests/ik_limits_reference.py) share it.  Plain helper module.

A case is a case of tests/ik_hard_cases.py (with its hard rows, or soft: rows = 0), of
tests/ik_cases.py (soft) or one built here, with a limits dict drawn by draw_limits(): the velocity
limit of about 60 % of the joints is 0.05 to 0.9 of the joint's speed without limits (the median over
the batch), the position range of every joint contains every robot of the batch with 0.2 to 1 rad to
spare, and the options then narrow single joints: a range whose upper end lies a few 1e-4 rad past
robot 0 (so other robots may start outside it), a one-sided range, a range of zero width.

Kinds: "ok" every robot resolves (status 0), inside the conditioning band (every comparison of the
rule at least 1e-7, relative, from a tie; pivots of S above 1e-5 in every solve that passes);
"infeasible" every robot's box contradicts the hard rows (scipy's LP agrees): status 4, NaN nu.
Draws outside the band were replaced by changing the seed."""
import functools

import numpy as np

import fb_models as FM
import ik_cases as IC
import ik_hard_cases as HC
import ik_limits_reference as LR
from blf import robot

CASES = {}


def _case(cid, base, seed, kind="ok", soft=False, **opt):
    CASES[cid] = (base, seed, kind, soft, opt)


# n = 1: the only joint (joint 0 = joint n - 1) ends on a bound; hard, and soft with a range of zero width
_case("chain1-hard-1", "chain1-k2com-1", 3, pin=(0,))
_case("chain1-soft-equal", "chain1-k2com", 3, soft=True, equal=(0,))
_case("chain3-hard-7", "chain3-k4-7", 2)
# n = 24, B = 3 (a wavefront with one live and one idle robot); robots 0 and 1 share a wavefront and
# need 3 and 2 iterations
_case("rand24-hard-15", "rand24-k2com-15", 4, frac=0.25)
# bounds active on joint 0 and joint n - 1
_case("rand24-hard-8-ends", "rand24-k2com-8", 3, frac=0.4, pin=(0, 23))
# ranges ending just past robot 0, a joint that starts outside its range, a range of zero width; the
# reference leaves block mode (13, 12 and 7 iterations)
_case("rand24-hard-9-block", "rand24-so3-r3-9", 3, frac=0.4, tight=(2, 7), outside=(5,), equal=(11,))
# soft, one-sided ranges, vel_max = NULL
_case("rand24-soft-onesided", "rand24-k2com", 3, soft=True, one_sided=True, tight=(0, 3, 9, 23))
# n = 26 | 27, prismatic joints at both layouts
_case("pri-chain26-hard-15", "pri-chain26-k2com-15", 3, frac=0.25, pin=(0, 25))
_case("pri-chain27-hard-15", "pri-chain27", 3, frac=0.3, pin=(0, 26))
# the same two with boxes wide enough to stay feasible over 20 steps (the integrated ones)
_case("pri-chain26-hard-15-wide", "pri-chain26-k2com-15", 1, frac=0.15)
_case("pri-chain27-hard-15-pos", "pri-chain27", 1, vel=False, tight=(0, 6, 13, 26))
# soft at one robot per wavefront: position ranges only (vel_max = NULL), outside, zero width
_case("chain27-soft-pos", "chain27-k2com", 3, soft=True, vel=False, tight=(0, 5, 26), outside=(8,), equal=(12,))
# n = 48: 12 hard rows, and the 27-row tree
_case("pri-rand48-hard-12", "pri-rand48-k2-12", 1)
_case("limbs48-hard-27", "limbs48-k4com-27", 2)
# far from the world origin (8 km)
_case("chain48-far-hard-15", "far:chain48-k2com-far-15", 1)
# the humanoid's standing set with robot.standing_ik_hard's rows at B = 130
_case("humanoid-hard-b130", "humanoid-15-nodamp-b130", 4, frac=0.25)
# infeasible: the box contradicts the hard rows on every robot
_case("rand24-hard-15-infeasible", "rand24-k2com-15", 1, kind="infeasible")
_case("pri-chain27-hard-15-infeasible", "pri-chain27", 2, kind="infeasible")
# robot 1 of 3 infeasible (it shares its wavefront with robot 0), the others resolve
_case("rand24-hard-15-mixed", "rand24-k2com-15", 3, kind="mixed", frac=0.25)

OK_CASES = sorted(c for c in CASES if CASES[c][2] == "ok")
INFEASIBLE_CASES = sorted(c for c in CASES if CASES[c][2] == "infeasible")
MIXED_CASE, MIXED_BAD = "rand24-hard-15-mixed", 1

# The cases that are also integrated over 1, 2 and 20 steps of DT: on each the rule's own trajectory
# and the certified one (LR.integrate(certified=True)) agree to 1e-10 over 20 steps and every step of
# every robot resolves (test_ik_limits_reference.py::test_integrate_case_conditioning).  The boxes of
# rand24-hard-15, pri-chain26-hard-15, pri-chain27-hard-15, limbs48-hard-27 and chain48-far-hard-15
# become infeasible for some robot within the 20 steps, so they are not integrated.
INTEGRATE_CASES = ["chain1-hard-1", "chain3-hard-7", "rand24-soft-onesided", "pri-chain26-hard-15-wide",
                   "pri-chain27-hard-15-pos", "chain27-soft-pos", "pri-rand48-hard-12", "humanoid-hard-b130"]


def draw_limits(states, speed, seed, frac=0.6, vel=True, tight=(), outside=(), one_sided=False, equal=(),
                pin=(), slack=(0.2, 1.0), sampling_time=0.01):
    """A limits dict for the batch `states` whose joints move at about `speed` [n] without limits.
    tight: joints whose upper end lies 0.05-0.9 of a step at `speed` past robot 0's position;
    outside: joints whose lower end lies 1e-3 above robot 0's position; equal: joints whose range has
    zero width, 1e-3 above robot 0; pin: joints whose velocity limit is 0.05-0.3 of `speed` whatever
    `frac` draws; one_sided: no lower ends and no velocity limits; vel: draw velocity limits at all."""
    rng = np.random.default_rng(seed)
    s = states["joint_pos"]
    n = s.shape[1]
    klim = rng.uniform(0.3, 1.0, n)
    lower = s.min(axis=0) - rng.uniform(*slack, n)
    upper = s.max(axis=0) + rng.uniform(*slack, n)
    vmax = np.where(rng.random(n) < frac, rng.uniform(0.05, 0.9, n) * speed, np.inf)
    for j in pin:
        vmax[j] = rng.uniform(0.05, 0.3) * speed[j]
    for j in tight:
        upper[j] = s[0, j] + rng.uniform(0.05, 0.9) * speed[j] * sampling_time / klim[j]
    for j in outside:
        lower[j] = s[0, j] + 1.0e-3
        upper[j] = max(upper[j], lower[j] + 0.1)
    for j in equal:
        lower[j] = upper[j] = s[0, j] + 1.0e-3
    if one_sided:
        lower[:] = -np.inf
    return dict(pos_lower=lower, pos_upper=upper, klim=klim, vel_max=vmax if vel and not one_sided else None,
                sampling_time=sampling_time, max_iter=0)


@functools.lru_cache(maxsize=None)
def _pri_chain27():
    """A 27-joint chain (one robot per wavefront) with prismatic joints, two SE3 tasks and the CoM."""
    n, seed, B = 27, 41, 3
    parent = FM._TOPO["chain"](n, seed)
    model = FM.tree_model(parent, seed, prismatic=[0, 13, 14, 26])
    states = robot.random_states(model, B, seed=seed + 7)
    return dict(model=model, B=B, states=states, tasks=IC.make_tasks(model, states, [1, 2], seed + 3))


@functools.lru_cache(maxsize=None)
def _far(base):
    """A hard case moved far from the world origin (fb_models.shift_ik's largest shift)."""
    cs = HC.build_case(base)
    _, (st, tk) = FM.shift_ik(cs["states"], cs["tasks"], len(FM.SHIFTS) - 1)
    return dict(cs, states=st, tasks=tk)


def _base(base, soft):
    if base == "pri-chain27":
        cs = _pri_chain27()
        return dict(cs, rows=0 if soft else HC.HR.mask([HC.ALL, HC.ALL], HC.COM))
    if base.startswith("far:"):
        cs = _far(base[4:])
    elif base in HC.CASES:
        cs = HC.build_case(base)
    else:
        cs = dict(IC.build_case(base), rows=0)
    return dict(cs, rows=0 if soft else cs["rows"])


@functools.lru_cache(maxsize=None)
def build_case(cid):
    """dict(model, B, states, tasks, rows, limits, kind) of case `cid`."""
    base, seed, kind, soft, opt = CASES[cid]
    cs = _base(base, soft)
    model, B = cs["model"], cs["B"]
    free = LR.no_limits(model["n"])
    nu0 = np.array([LR.solve(model, cs["states"], cs["tasks"], cs["rows"], free, i)["nu"][6:]
                    for i in range(min(B, 5))])
    speed = np.maximum(np.median(np.abs(nu0), axis=0), 1.0e-3)
    return dict(model=model, B=B, states=cs["states"], tasks=cs["tasks"], rows=cs["rows"],
                limits=draw_limits(cs["states"], speed, seed, **opt), kind=kind)


@functools.lru_cache(maxsize=None)
def reference(cid):
    """LR.solve of every robot of the case, computed once and shared (and never changed)."""
    cs = build_case(cid)
    return [LR.solve(cs["model"], cs["states"], cs["tasks"], cs["rows"], cs["limits"], i) for i in range(cs["B"])]


@functools.lru_cache(maxsize=None)
def certificate(cid):
    """LR.certify of every robot's final set: list of (nu, accepted)."""
    return [LR.certify(r["parts"], r["lo"], r["up"], r["side"]) for r in reference(cid)]


DT = HC.DT


@functools.lru_cache(maxsize=None)
def integrate_reference(cid, steps, certified=False):
    """LR.integrate of the case's first three robots over `steps` steps of DT, computed once."""
    cs = build_case(cid)
    return [LR.integrate(cs["model"], cs["states"], cs["tasks"], cs["rows"], cs["limits"], i, steps, DT,
                         certified=certified) for i in range(min(cs["B"], 3))]


@functools.lru_cache(maxsize=None)
def raised_com(dz=0.02):
    """What the limits are for: ik_hard_cases.planted_feet() (the humanoid on straight legs, hard feet)
    with the CoM target `dz` above the nominal height, which straight legs cannot reach.  On the
    reference, 20 steps of DT without limits push both knees (joints 3 and 9) about 0.011 rad past
    straight; with robot.humanoid24_joint_limits and sampling_time = DT the knees are held at their
    lower bound (0 exactly: the box's lower end is 0 there) and the soles stay planted.
    dict(model, B, states, tasks, rows, limits)."""
    cs = HC.planted_feet()
    com = cs["tasks"]["com_pos"].copy()
    com[:, 2] += dz
    limits = dict(robot.humanoid24_joint_limits(cs["model"], sampling_time=DT), max_iter=0)
    return dict(cs, tasks=dict(cs["tasks"], com_pos=com), limits=limits)
