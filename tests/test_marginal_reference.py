"""tests/marginal_reference.py on the CPU: the refinement columns against mpmath's inversion of the exactly formed H, their symmetry,
the condition 64 eps <= tolerance <= 1e-9 on every structure and class the device test uses, what the structures are for (edge counts,
a kept point), and a guard: five mistakes a covariance kernel could make, planted in the numpy restatement of the device's recurrence,
each leave the tolerance on every queried block they reach.  No GPU."""
import mpmath as mp
import numpy as np
import pytest

from . import marginal_reference as MR
from . import solve_reference as SR


def exact_hessian(g, recs):
    """H = sum_f J_f' J_f + P formed exactly from the records (mpmath)"""
    n = int(SR.dims(g)[1][-1])
    P, _eta = SR.prior_system(g)
    H = mp.zeros(n, n)
    for cols, Jf, _bf in recs:
        for row in Jf:
            for c1, a1 in zip(cols, row):
                for c2, a2 in zip(cols, row):
                    H[int(c1), int(c2)] += mp.mpf(float(a1)) * mp.mpf(float(a2))
    for i in range(n):
        for j in range(n):
            H[i, j] += mp.mpf(float(P[i, j]))
    return H


@pytest.mark.parametrize("name", ["clip", "poses_5"])
def test_columns_equal_the_direct_inverse_in_50_digits(oracle, name):
    """the two smallest structures, every column: mpmath's inverse of the exactly formed H (computed with 30 guard digits, so that what
    is measured is the refinement's own error)"""
    g, recs = SR.graph(name), SR.oracle_records(name)
    d, off = SR.dims(g)
    cols = MR.reference_columns(g, recs, range(g.n_vars))
    with mp.workdps(SR.DPS + 30):
        Sig = exact_hessian(g, recs) ** -1
        worst = mp.mpf(0)
        for v in range(g.n_vars):
            for k in range(d[v]):
                j = int(off[v]) + k
                scale = max(abs(Sig[i, j]) for i in range(off[-1]))
                worst = max(worst, max(abs(cols[v][k][i] - Sig[i, j]) for i in range(off[-1])) / scale)
    print(f"{name}: n = {off[-1]}, |refined - direct| / |column| = {mp.nstr(worst, 3)}, refinement steps {MR.refinement_steps(g)}")
    assert worst <= mp.mpf("1e-40")


def test_blocks_are_symmetric_in_50_digits(oracle):
    """Sigma_ij = Sigma_ji' although the two come from different columns: every diagonal and cross block of `degree`'s key list"""
    g = SR.graph("degree")
    ref = MR.cpu_reference("degree")
    worst = mp.mpf(0)
    with mp.workdps(SR.DPS):
        scale = {i: MR._max(MR.block(g, ref.columns, i, i)) for i in ref.vars}
        for i in ref.vars:
            for j in ref.vars:
                a, b = MR.block(g, ref.columns, i, j), MR.block(g, ref.columns, j, i)
                e = max(abs(a[r][c] - b[c][r]) for r in range(len(a)) for c in range(len(a[0])))
                worst = max(worst, e / mp.sqrt(scale[i] * scale[j]))
    print(f"degree: {len(ref.vars)} keys, asymmetry {mp.nstr(worst, 3)}")
    assert worst <= mp.mpf("1e-40")


@pytest.mark.parametrize("name", MR.PLAIN + MR.TREES)
def test_cpu_computations_keep_every_tolerance_below_1e_9(oracle, name):
    ref = MR.cpu_reference(name)
    print(MR.report(name, ref))
    assert set(ref.cpu) == {"inv", "cholesky", "selinv"} and ref.present
    for k in MR.MEASURES:
        assert 64 * SR.EPS <= ref.tol[k] <= SR.MAX_TOL, (name, k, ref.tol[k])
    for k in ref.present:                    # a class that is queried is measured: no computation returns it exactly
        assert name == "poses_1" or max(m[k] for m in ref.cpu.values()) > 0.0


def test_the_structures_hold_the_edge_counts_and_a_kept_point(oracle):
    """k_point_cov strides the e^2 edge pairs of a point over 64 lanes: below, at and above one, two and three passes"""
    squares = set()
    for name in ("degree", "degree_wide"):
        g = SR.graph(name)
        cls = MR.var_classes(g)
        ne = MR.edge_counts(g)
        assert all(cls[i] == "schur" for i in ne)
        squares |= {e * e for e in ne.values()}
        asked = {ne[i] for i in MR.query_vars(name) if cls[i] == "schur"}
        print(f"{name}: edge counts {sorted(set(ne.values()))}, queried {sorted(asked)}")
        if name == "degree_wide":            # every count of this structure is queried
            assert asked == set(ne.values()) == set(SR.WIDE_DEGREES) | {2 * k for k in SR.WIDE_HYBRID}
    assert squares >= {1, 4, 49, 64, 81, 121, 144, 169}
    for name in ("kept_hybrid", "kept_chain"):
        g = SR.graph(name)
        cls = MR.var_classes(g)
        assert any(cls[i] == "kept" for i in MR.query_vars(name)) and "chain" not in {cls[i] for i in MR.query_vars(name)}
    assert "chain" in MR.var_classes(SR.graph("kept_chain"))
    for name in MR.PLAIN + MR.TREES:         # the key lists follow their rule
        g = SR.graph(name)
        n = int(SR.dims(g)[1][-1])
        q = MR.query_vars(name)
        assert len(set(q)) == len(q) and (len(q) <= 12 if n > MR.SMALL else len(q) == sum(c != "chain" for c in MR.var_classes(g)))


def reached(g, plant):
    """the variables whose block a planted mistake changes: `identity` every Schur point; the others every tile of the selected inverse
    but the root's diagonal tile - a pose-like variable outside the last tile, a Schur point with an edge to one"""
    cls = MR.var_classes(g)
    if plant == "identity":
        return {i for i in range(g.n_vars) if cls[i] == "schur"}
    d, off = SR.dims(g)
    _p, c = MR.elimination_order(g)
    root = (len(c) - 1) // MR.TILE
    place = {int(s): k for k, s in enumerate(c)}
    below = {i for i in range(g.n_vars) if cls[i] in ("pose", "kept") and place[int(off[i])] // MR.TILE < root}
    out = set(below)
    for blk in g.blocks:
        for row in blk.var_idx:
            if any(int(v) in below for v in row):
                out |= {int(v) for v in row if cls[int(v)] == "schur"}
    return out


# kept_hybrid (weak priors next to 0.05 m observations: its CPU computations differ by 8e-12, tolerance 1.2e-10) hides a single entry
# off by 1e-8 in some pose blocks (error / tolerance 0.55 .. 33): that mistake is planted in the two better-conditioned structures
PLANTED = [(name, plant) for name in ("degree", "degree_wide", "kept_hybrid") for plant in MR.PLANTS if (name, plant) != ("kept_hybrid", "panel")]


@pytest.mark.parametrize("name,plant", PLANTED)
def test_planted_mistakes_leave_the_tolerance(oracle, name, plant):
    """on CPU arithmetic alone: the recurrence with one mistake, measured like the device; every queried block the mistake reaches is
    outside its class's tolerance (and the recurrence without the mistake is inside: it is one of the three the tolerance is made of)"""
    g, recs = SR.graph(name), SR.oracle_records(name)
    ref = MR.cpu_reference(name)
    cls = MR.var_classes(g)
    H = MR.hessian(g, recs)
    Sig = None if plant == "panel" else MR.takahashi(g, H, plant)
    hit = reached(g, plant)
    below = {i for i in hit if cls[i] != "schur"}
    seen = []
    for i in ref.vars:
        if i in hit:
            if plant == "panel":             # one entry of one tile: planted under the block's own variable (a point: under its poses)
                at = [i] if i in below else sorted({int(v) for blk in g.blocks for row in blk.var_idx if i in row for v in row} & below)
                Sig = MR.takahashi(g, H, plant, MR.rows_of(g, at))
            m = MR.measure_dense(g, ref.columns, (i,), Sig)[cls[i]]
            seen.append((m / ref.tol[cls[i]], cls[i], i))
    assert len(seen) >= 3 and {c for _r, c, _i in seen} >= ({"schur"} if plant == "identity" else {"pose", "schur"})
    print(f"{name} {plant}: {len(seen)} blocks reached, error / tolerance from {min(seen)[0]:.2e} to {max(seen)[0]:.2e}")
    for ratio, c, i in seen:
        assert ratio > 1.0, (name, plant, c, i, ratio)
