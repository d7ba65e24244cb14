"""The six point-touching factor classes on the device, through the C ABI, against the 50-digit reference of
tests/point_factor_reference.py: PoseToPoint, Stereo, HybridMotion, StereoHybridMotion, LandmarkTernary and LandmarkMotionPose.

The graph is the helper's input table: 160 factors per class (more than one 128-lane workgroup of k_linearize, the last one partial),
each on variables of its own, each with a full non-symmetric sqrt-information R, with no / an active / an inactive Huber kernel and
one whose threshold sits 1e-3 (relative) from |Re|, with depths on both sides of the cheirality test, poses and points offset by
1e3, and local points at depths of 1e-2 and 1e4.  The reference differentiates its residuals in 50 digits; it restates no Jacobian.

Tolerances (point_factor_reference.tol): max(8 x measured, 8 eps x magnitude of the operands), `measured` the fp64 CPU oracle's
rounding error against the same reference per class and group; times the largest absolute row sum of R for whitened quantities;
plus robust_slack for an active Huber weight; a numeric Jacobian gets the residual's tolerance x 1 / (2 delta).  Nothing here is
taken from the device's output.  Every factor of the table is compared in the linearisation, error and noise tests, and every
container factor in its test: none is skipped.  The LM test solves one graph of all 960 (the table keeps its whitened Jacobians
below 1e6 so that fp64 can) and compares every factor of it."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from dynosam_amd import graph as G  # noqa: E402

from . import point_factor_reference as PR  # noqa: E402
from . import se3_reference as SR  # noqa: E402


@pytest.fixture(scope="module")
def full():
    """the table, its graph of six blocks and its reference: computed once and left unchanged"""
    specs = PR.table()
    g, var_of = PR.flat_graph(specs)
    return specs, g, PR.reference(specs), var_of


def context(g):
    from dynosam_amd.optimizer import Context
    c = Context()
    c.upload(g)
    return c


def test_linearisation_of_every_point_class(full):
    """J, b and the per-factor error of all 960 factors (k_linearize<T, 128> with its LDS write-out, k_linearize_numeric for
    LandmarkMotionPose); columns beyond a factor's slots and rows beyond its dimension are exactly zero; error() is the sum of the
    reference's costs."""
    specs, g, ref, _ = full
    assert [b.type for b in g.blocks] == list(PR.CLASSES) and all(b.count == 160 for b in g.blocks)
    c = context(g)
    J, b, e = c.linearize()
    PR.check_linearisation(J, b, e, ref)
    assert abs(c.error() - sum(r.cost for r in ref)) <= PR.cost_sum_tol(ref)
    c.close()


@pytest.mark.parametrize("t", PR.CLASSES, ids=lambda t: PR.NAMES[t])
def test_error_of_one_class(full, t):
    """a graph of ONE block takes the per-class k_error<T>, the graph of six k_error_fused: each gives the reference's sum"""
    specs, g, ref, _ = full
    mine = [s for s in specs if s.cls == t]
    rf = [r for r in ref if r.cls == t]
    g1, _ = PR.flat_graph(mine)
    assert len(g1.blocks) == 1 and g1.blocks[0].count == 160
    c = context(g1)
    assert abs(c.error() - sum(r.cost for r in rf)) <= PR.cost_sum_tol(rf)
    c.upload(g)
    assert abs(c.error() - sum(r.cost for r in ref)) <= PR.cost_sum_tol(ref)
    c.close()


# ---- one LM iteration ---------------------------------------------------------------------------------------------------------
def lm_graph(specs, split):
    """The graph of `specs` made well-posed: a unit-sigma prior on every pose (at its own value) and a unit-noise PoseToPoint observation
    of every point from the first pose of its factor.  Blocks: the six classes, the observations, the priors = 8 = FUSE_MAX; with
    `split` the first PoseToPoint block is cut in two (9 blocks: per-class launches).  Returns (graph, var_of, anchors, prior variables)."""
    rng = np.random.default_rng(91)
    g, var_of = PR.flat_graph(specs)
    anchors = []
    for f, sp in enumerate(specs):
        ps = PR.SLOTS[sp.cls].index("X")
        anchors += [(PR.anchor(sp, ps, s, rng), var_of[f][ps], var_of[f][s]) for s, k in enumerate(PR.SLOTS[sp.cls]) if k == "p"]
    blocks = list(g.blocks)
    assert [b.type for b in blocks] == list(PR.CLASSES)
    if split:
        b0 = blocks[0]
        m = np.arange(b0.count) < b0.count * 5 // 8
        blocks[0:1] = [b0.subset(m), b0.subset(~m)]
    nf = len(specs)
    blocks.append(G.FactorBlock(G.F_POSE_TO_POINT, np.arange(nf, nf + len(anchors)), [[p, l] for _, p, l in anchors], np.array([a.meas for a, _, _ in anchors]),
                                np.tile(np.eye(3).reshape(-1), (len(anchors), 1))))
    poses = np.flatnonzero(g.var_type == 0)
    nf += len(anchors)
    blocks.append(G.FactorBlock(G.F_PRIOR_POSE3, np.arange(nf, nf + len(poses)), poses.reshape(-1, 1), g.var_state[poses], np.ones((len(poses), 6))))
    return G.FlatGraph(g.var_keys, g.var_type, g.var_state, blocks), var_of, anchors, poses


def lm_reference(specs, var_of, anchors, poses, start, vals):
    """the cost of every factor of lm_graph at `vals` and its tolerance: (sum, summed tolerance)"""
    lins = [PR.Lin(sp, [vals[v] for v in var_of[f]], want_J=False) for f, sp in enumerate(specs)]
    lins += [PR.Lin(a, [vals[p], vals[l]], want_J=False) for a, p, l in anchors]
    total, tol = sum(r.cost for r in lins), PR.cost_sum_tol(lins)
    for v in poses:
        f = SR.prior(vals[v], start[v], np.ones(6))
        total += f.cost
        tol += SR.cost_tol(f, SR.regime_of(np.linalg.norm(f.e[:3])))
    return total, tol


@pytest.mark.parametrize("split", [False, True], ids=["fused_8_blocks", "per_class_9_blocks"])
def test_errors_around_one_lm_iteration(full, split):
    """error_before and error_after of a one-iteration optimize() are the reference's costs at the start state and at the downloaded
    values: k_error_fused and k_trial_errors_fused with 8 blocks, k_error<T> and k_lin_error<T> with 9, and k_retract on point
    variables in both."""
    from dynosam_amd.optimizer import LevenbergMarquardtParams
    specs, _, ref, _ = full
    sub = specs                      # the whole table: no factor is left out of the graph
    assert len(sub) == 6 * 160 and max(np.abs(r.J).max() for r in ref) <= PR.MAX_WJ * (1 + 1e-12)
    gl, var_of, anchors, poses = lm_graph(sub, split)
    assert len(gl.blocks) == (9 if split else 8)
    c = context(gl)
    P = LevenbergMarquardtParams()
    P.max_iterations = 1
    r = c.optimize(P)
    assert r.status == 0 and r.iterations == 1
    start = gl.var_state
    before, tol_before = lm_reference(sub, var_of, anchors, poses, start, start)
    assert abs(r.error_before - before) <= tol_before
    accepted = [i for i in range(r.trace_len) if r.trace_accepted[i]]
    assert len(accepted) == 1
    vals = c.values()
    assert np.abs(vals - start).max() > 1e-3
    after, tol_after = lm_reference(sub, var_of, anchors, poses, start, vals)
    assert abs(r.error_after - after) <= tol_after
    assert r.trace_error[accepted[0]] == r.error_after
    assert abs(c.error() - after) <= tol_after
    c.close()


# ---- linear containers --------------------------------------------------------------------------------------------------------
def test_linearised_containers_over_point_classes():
    """F_LINEARIZED | each of the six classes, 160 factors per class: random A and b, point slots 1e-3 ... 1 from their linearisation
    point, pose slots one generic Local away: r = sum_s A_s d_s - b, the record's b' = -r, J == A bit for bit, error |r|^2 / 2
    (res_linearized with 3-wide point slots in k_linearize and k_error_fused).  Tolerance of r, as for the pose-only containers:
    sum_s |A_s|_inf x (the error of d_s + 8 eps |d_s|) + 8 eps |r|; d_s = x - lin of a point is exact up to eps |x|, Local is a
    residual of the generic regime."""
    rng = np.random.default_rng(92)
    keys, vt, states, blocks, ref = [], [], [], [], []
    for cls in PR.CLASSES:
        var, meas, consts = [], [], []
        slots = PR.SLOTS[cls]
        for k in range(PR.REPLICAS * PR.ENTRIES):
            lins, xs, A, tol_d = [], [], [], []
            for kind in slots:
                if kind == "X":
                    lin = SR.generic_pose(rng)
                    ax = rng.normal(0, 1, 3)
                    xi = np.concatenate([rng.uniform(0.2, 2.5) * ax / np.linalg.norm(ax), rng.normal(0, 1, 3)])
                    x = SR.to12(SR.compose(SR.pose(lin), SR.true_exp(SR.vec(xi))))
                    tol_d.append(SR.tol("generic", "e", max(1.0, np.abs(lin[9:]).max(), np.abs(x[9:]).max(), np.abs(xi).max())))
                    A.append(rng.normal(0, 1, (3, 6)))
                else:
                    lin = rng.normal(0, 1, 3) * 10.0 ** rng.uniform(-1, 1)
                    d = rng.normal(0, 1, 3)
                    x = lin + 10.0 ** rng.uniform(-3, 0) * d / np.abs(d).max()
                    tol_d.append(8 * SR.EPS64 * max(np.abs(lin).max(), np.abs(x).max()))
                    A.append(rng.normal(0, 1, (3, 3)))
                lins.append(lin)
                xs.append(x)
            bb = rng.normal(0, 1, 3)
            mine = []
            for kind, x in zip(slots, xs):
                mine.append(len(keys))
                keys.append((PR.X_CHR if kind == "X" else PR.L_CHR) | len(keys))
                vt.append(0 if kind == "X" else 1)
                states.append(np.concatenate([x, np.zeros(12 - len(x))]))
            var.append(mine)
            meas.append(bb)
            consts.append(np.concatenate([a.reshape(-1) for a in A] + lins))
            r, cost, dmax = PR.linearized(cls, A, lins, xs, bb)
            t = sum(np.abs(a).sum(1).max() * (td + 8 * SR.EPS64 * dm) for a, td, dm in zip(A, tol_d, dmax)) + 8 * SR.EPS64 * np.abs(r).max()
            ref.append((cls, r, cost, A, t))
        blocks.append((cls | G.F_LINEARIZED, var, meas, consts))
    order = np.argsort(np.array(keys, dtype=np.uint64), kind="stable")
    new = np.empty(len(keys), dtype=np.int64)
    new[order] = np.arange(len(keys))
    fb, f0 = [], 0
    for t, var, meas, consts in blocks:
        fb.append(G.FactorBlock(t, np.arange(f0, f0 + len(var)), new[np.array(var)], np.array(meas), None, None, np.array(consts)))
        f0 += len(var)
    g = G.FlatGraph(np.array(keys, dtype=np.uint64)[order], np.array(vt, dtype=np.uint8)[order], np.array(states)[order], fb)
    c = context(g)
    J, b, e = c.linearize()
    assert len(ref) == 6 * 160 == len(b)
    for f, (cls, r, cost, A, t) in enumerate(ref):
        assert np.abs(b[f][:3] + r).max() <= t and not b[f][3:].any(), (f, PR.NAMES[cls], b[f], r)
        assert abs(e[f] - cost) <= np.abs(r).sum() * t + 8 * SR.EPS64 * cost, (f, PR.NAMES[cls])
        want = np.zeros((6, 24))
        for s, a in enumerate(A):
            want[:3, 6 * s:6 * s + a.shape[1]] = a
        assert np.array_equal(J[f], want), (f, PR.NAMES[cls])
    tot = sum(np.abs(r).sum() * t + 8 * SR.EPS64 * cost for _, r, cost, _, t in ref)
    assert abs(c.error() - sum(cost for _, _, cost, _, _ in ref)) <= tot
    c.close()


def test_transposed_noise_would_be_seen(full):
    """On the reference alone (CPU arithmetic): whitening with R^T instead of R leaves the tolerance of b or J on at least 90 % of the
    table's factors.  Guards the table's R against drifting back towards symmetric, where a transposed R would pass."""
    specs, _, ref, _ = full
    seen = 0
    for s, r in zip(specs, ref):
        wrong = PR.Lin(s, want_J=False, R=s.R.T, strict=False)
        slack = PR.robust_slack(r)
        Jt = wrong.sqrt_w * s.R.T @ r.Ju
        seen += bool(np.abs(wrong.b - r.b).max() > PR.tol(r, "e") + slack * np.abs(r.b).max() or
                     np.abs(Jt - r.J).max() > PR.tol(r, "numJ" if r.numeric else "J") + slack * np.abs(r.J).max())
    assert seen >= 0.9 * len(specs), seen
