"""tests/solve_reference.py on the CPU: the refinement reference against mpmath's direct solve of the exactly formed system, the
condition "every tolerance <= 1e-9" on every structure (linearised by the oracle; numpy's Cholesky and the oracle's Schur solve), what
each structure is for, and a guard: on the reference alone, a solve with lambda left out of the chained points' blocks leaves the
tolerance.  No GPU."""
import mpmath as mp
import numpy as np
import pytest

from dynosam_amd import graph as G

from . import solve_reference as SR

COMBOS = [(lam, False) for lam in SR.LAMBDAS] + [(SR.DIAG_LAMBDA, True)]


def linearised(name):
    return SR.graph(name), SR.oracle_records(name)


reference = SR.cpu_reference        # (name, lam, diag): cached, shared with the device test


@pytest.mark.parametrize("name,lam,diag", [("poses_17", 0.0, False), ("kept_chain", 1e-3, True)])
def test_refinement_equals_the_direct_solve_in_50_digits(oracle, name, lam, diag):
    """about 100 unknowns: H = sum_f J_f' J_f + P + lambda D and g formed exactly from the records, mpmath's Cholesky solve"""
    g, recs = linearised(name)
    ref = reference(name, lam, diag)
    n = len(ref.x)
    assert 90 <= n <= 130
    P, eta = SR.prior_system(g)
    with mp.workdps(SR.DPS):
        H, rhs = mp.zeros(n, n), mp.zeros(n, 1)
        for cols, Jf, bf in recs:
            for row, bi in zip(Jf, bf):
                for c1, a1 in zip(cols, row):
                    rhs[int(c1)] += mp.mpf(float(a1)) * mp.mpf(float(bi))
                    for c2, a2 in zip(cols, row):
                        H[int(c1), int(c2)] += mp.mpf(float(a1)) * mp.mpf(float(a2))
        for i in range(n):
            rhs[i] += mp.mpf(float(eta[i]))
            for j in range(n):
                H[i, j] += mp.mpf(float(P[i, j]))
        for i in range(n):
            d = min(max(H[i, i], mp.mpf(1e-6)), mp.mpf(1e32)) if diag else mp.mpf(1)
            H[i, i] += mp.mpf(float(lam)) * d
        x = mp.cholesky_solve(H, rhs)
        err = max(abs(x[i] - ref.x[i]) for i in range(n)) / max(abs(x[i]) for i in range(n))
        print(f"{name}: n = {n}, refinement corrections {['%.1e' % s for s in ref.steps]}, |refined - direct| / |direct| = {mp.nstr(err, 3)}")
        assert err <= mp.mpf("1e-30")


@pytest.mark.parametrize("name", sorted(SR.STRUCTURES))
def test_cpu_solvers_keep_every_tolerance_below_1e_9(oracle, name):
    g, recs = linearised(name)
    assert SR.dims(g)[1][-1] <= 810                                   # small enough for a few seconds per case
    for lam, diag in COMBOS:
        ref = reference(name, lam, diag)
        print(SR.report(name, ref, lam, diag))
        assert ("oracle" in ref.cpu) == (not diag and g.prior is None)
        for k, t in ref.tol.items():
            assert 64 * SR.EPS <= t <= SR.MAX_TOL, (name, lam, diag, k, t)


def degrees(g, ftypes):
    """point variable -> number of factors of the classes `ftypes` on it"""
    deg = {}
    for blk in g.blocks:
        if blk.type in ftypes:
            for row in blk.var_idx:
                for v in row:
                    if g.var_type[v] == G.VAR_POINT3:
                        deg[int(v)] = deg.get(int(v), 0) + 1
    return deg


def test_the_structures_are_what_they_are_for(oracle):
    deg = list(degrees(SR.graph("degree"), (G.F_POSE_TO_POINT,)).values())
    assert all(deg.count(d) == 3 for d in (1, 2, 3, 4, 5, 7, 8, 9))
    assert {b.type for b in SR.graph("degree").blocks} >= {G.F_STEREO_POINT, G.F_HYBRID_MOTION, G.F_STEREO_HYBRID_MOTION, G.F_HYBRID_SMOOTHING}
    for P in SR.PAIR_COUNTS:                                          # P points shared by two and P by three poses
        deg = list(degrees(SR.graph(f"pairs_{P}"), (G.F_POSE_TO_POINT,)).values())
        assert deg.count(2) == P and deg.count(3) == P
    g = SR.graph("chain_ternary")
    links = degrees(g, (G.F_LANDMARK_TERNARY,))
    tern = [b for b in g.blocks if b.type == G.F_LANDMARK_TERNARY][0]
    pairs = [tuple(r[:2]) for r in tern.var_idx]
    assert len(pairs) - len(set(pairs)) == 1                          # two factors on one link
    n_pts = int((g.var_type == G.VAR_POINT3).sum())
    assert n_pts == 2 + 3 + 14 + 15 + 40 and len(links) == n_pts
    assert {b.type for b in SR.graph("chain_wcpe").blocks} >= {G.F_LANDMARK_MOTION_POSE, G.F_LANDMARK_POSE_SMOOTHING}
    ref = reference("chain_weak", 10.0, False)                        # small components next to large ones
    assert np.abs(ref.x64[ref.point]).max() <= 1e-2 * np.abs(ref.x64[ref.pose]).max()
    for name in ("kept_hybrid", "kept_chain"):
        g = SR.graph(name)
        kinds = [int(g.var_type[g.key_index(int(k))]) for k in g.prior.keys]
        assert G.VAR_POSE3 in kinds and G.VAR_POINT3 in kinds
    g = SR.graph("kept_chain")
    assert any(SR.chained_mask(g)[SR.dims(g)[1][g.key_index(int(k))]] for k in g.prior.keys)     # a chained point in the prior
    g, recs = linearised("clip")                                      # the clip of diagonalDamping is active on one pose and one point
    J, _b = SR.dense(recs, SR.dims(g)[1][-1])
    h = (J * J).sum(0)
    d, off = SR.dims(g)
    low = {int(g.var_keys[i]) for i in range(g.n_vars) if (h[off[i]:off[i + 1]] < 1e-6).all()}
    assert low == set(g.meta["clipped"])
    assert (h[[off[i] for i in range(g.n_vars) if int(g.var_keys[i]) not in low]] > 1e-3).all()


@pytest.mark.parametrize("name", SR.CHAIN_STRUCTURES)
def test_lambda_left_out_of_the_chained_points_would_be_seen(oracle, name):
    """the reference solved once more with lambda missing on the diagonal of the chained points (what a chain kernel that forgets its
    damping term computes): the point class leaves the tolerance at both non-zero lambdas, in both damping modes"""
    g, recs = linearised(name)
    n = SR.dims(g)[1][-1]
    chained = SR.chained_mask(g)
    assert chained.any()
    P, eta = SR.prior_system(g)
    J, _b = SR.dense(recs, n)
    sysm = SR.System(recs, n, P, eta)
    for lam, diag in ((1e-3, False), (10.0, False), (SR.DIAG_LAMBDA, True)):
        ref = reference(name, lam, diag)
        x, _ = SR.reference_solve(sysm, J, P, lam, diag, lam_scale=(~chained).astype(np.float64))
        off = SR.measure(np.array([float(v) for v in x]), ref.x, ref.point)
        print(f"{name} lam {lam:g} {'diag' if diag else 'I'}: point class moves by {off:.2e}, tolerance {ref.tol['point']:.2e}")
        assert off > 10 * ref.tol["point"]
