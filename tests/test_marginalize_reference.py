"""tests/marginalize_reference.py on the CPU: the refined marginal against mpmath's dense solve of the exactly formed H, the condition
64 eps <= tolerance <= 1e-9 on every case and measure the device test uses (with the printed table), WindowOracle.marginalize held to the
same reference (keys, merge rule, the re-wrap at a moved state), what the cuts are for, and a guard: seven mistakes a marginalisation
could make, planted in the numpy restatement of the device's computation, each leave the tolerance on at least one measure on every
case they reach.  No GPU."""
import mpmath as mp
import numpy as np
import pytest

from dynosam_amd import graph as G

from . import marginalize_reference as MZ
from . import solve_reference as SR

ALL = tuple(MZ.CASES) + tuple(MZ.TREES)
# (the dense mpmath solve costs 1.6 s at 63 marginalised scalars and 5.9 s at 102: one case per family)
EXACT = ("poses_5-old1", "poses_11-old6", "poses_17-old16", "degree-old", "degree_wide-points", "pairs_17-points", "pairs_16-old", "chain_wcpe-old",
         "kept_hybrid-pose-moved", "kept_hybrid-point-moved", "kept_hybrid-merge-moved", "kept_hybrid-empty-moved", "kept_chain-point-moved",
         "kept_chain-merge", "degree-cauchy-old")


@pytest.mark.parametrize("case", EXACT)
def test_refined_marginal_equals_the_direct_solve_in_50_digits(oracle, case):
    cc = MZ.cpu_case(case)
    assert len(cc.cut.M) <= MZ.EXACT_MAX
    worst = MZ.difference(cc.ref, MZ.exact(cc.cut, cc.recs))
    print(f"{case}: |M| = {len(cc.cut.M)}, |S| = {len(cc.cut.S)}, |refined - direct| on the measures' scales = {worst:.3g}, refinement steps {cc.ref.steps}")
    assert worst <= 1e-40


@pytest.mark.parametrize("case", ALL)
def test_tolerances_are_between_64_eps_and_1e_9(oracle, case):
    cc = MZ.cpu_case(case)
    print(MZ.report(case, cc), f"\n{'':34s} |M| = {len(cc.cut.M)}, |S| = {len(cc.cut.S)}, refinement steps {cc.ref.steps}, c / c0 = {cc.c_over_c0:.3g}")
    assert len(cc.cut.S) > 0 and cc.ref.c0 > 0
    for k in MZ.MEASURES:
        assert 64 * SR.EPS <= cc.tol[k] <= SR.MAX_TOL, (case, k, cc.tol[k])
    with mp.workdps(SR.DPS):         # the reference marginal is symmetric although its halves come from different columns' operands
        n = len(cc.ref.eta)
        assert all(cc.ref.Lambda[i][j] == cc.ref.Lambda[j][i] for i in range(n) for j in range(n))
        assert all(cc.ref.Lambda[i][i] > 0 for i in range(n))


WINDOW = ("poses_11-old5", "degree-old", "degree-points", "pairs_17-old", "chain_wcpe-old", "kept_hybrid-pose-moved", "kept_hybrid-point",
          "kept_hybrid-point-moved", "kept_hybrid-merge-moved", "kept_hybrid-empty-moved", "kept_chain-pose-moved", "kept_chain-point-moved",
          "kept_chain-merge", "kept_chain-empty")


@pytest.mark.parametrize("case", WINDOW)
def test_window_oracle_is_within_the_tolerance_of_the_reference(oracle, case):
    """WindowOracle.marginalize linearises for itself (the records of oracle_records_of) and restates the definition independently of the
    helper: same separator, same merge rule, same re-wrap; the containers are the untouched factors"""
    from oracle import window_oracle as WO
    cc = MZ.cpu_case(case)
    g, keys = MZ.case_graph(case)
    blocks, prior = WO.WindowOracle(g).marginalize(list(keys), g.var_state)
    assert np.array_equal(prior.keys, cc.cut.sep_keys)
    got = MZ.measure(cc.cut, cc.ref, prior.Lambda, prior.eta, prior.c)
    print(case, {k: f"{got[k]:.1e}" for k in cc.present})
    assert all(got[k] <= cc.tol[k] for k in MZ.MEASURES), got
    assert {(int(b.type) & 15, int(s)) for b in blocks for s in b.slot} == cc.cut.kept_slots


def test_what_the_cuts_are_for():
    d = {}
    for case in ALL:
        g, keys = MZ.case_graph(case)
        d[case] = MZ.Cut(g, keys)
    # the eliminated segment against the 32-row tile: 6, 30 (two rows of padding), 36 (into a second tile), 66, 96 (three full tiles)
    sizes = [len(d[c].M) for c in ("poses_5-old1", "poses_11-old5", "poses_11-old6", "poses_17-old11", "poses_17-old16")]
    assert sizes == [6, 30, 36, 66, 96]
    for c in ("poses_5-old1", "poses_11-old5", "poses_11-old6", "poses_17-old11"):
        assert len(d[c].Sv) > 1, c                                     # a loop closure reaches across the cut
    assert len(d["poses_17-old16"].Sv) == 1
    for c in MZ.TREES:                                                 # twelve eliminated tile columns (the last one with padding) and fill
        rows, n_elim, p, n_raw = MZ.layout(d[c])
        assert (n_raw, n_elim, len(p)) == (360, 12, 0) and len(d[c].Sv) >= 16
    for c, ct in d.items():
        rows, n_elim, p, n_raw = MZ.layout(ct)
        if c.endswith("-points"):                                      # nothing for the tile factorisation: the zero-column partial order
            assert n_elim == 0 and len(p) == len(ct.M) > 0, c
        if c.endswith("-poses"):                                       # every point the cut sees is retained and named
            assert len(p) == 0 and any(k == "point" for _a, _b, k in ct.sblocks), c
    for c in MZ.CHAIN_CASES:                                           # the cut severs point chains: a retained point shares a factor with an eliminated one
        ct, g = d[c], d[c].g
        severed = 0
        for f in np.nonzero(ct.touch)[0]:
            pts = [v for v in ct.fvars[f] if g.var_type[v] == G.VAR_POINT3]
            if len(pts) == 2 and ct.is_m[pts].sum() == 1:
                kept = next(v for v in pts if not ct.is_m[v])
                assert kept in ct.Sv                                   # the first retained point of the chain is named by the marginal
                severed += 1
        assert severed >= 2, c
    for name in ("kept_hybrid", "kept_chain"):
        assert d[f"{name}-pose"].prior_touch and all(g_.var_type[v] == G.VAR_POINT3 and v in d[f"{name}-pose"].Sv
                                                     for g_ in [d[f"{name}-pose"].g] for v in d[f"{name}-pose"].prior_vars if not d[f"{name}-pose"].is_m[v])
        ct = d[f"{name}-point"]
        rows, n_elim, p, n_raw = MZ.layout(ct)
        assert ct.prior_touch and len(ct.M) == 3 and n_elim == 1 and len(p) == 0            # eliminated by the tile factorisation, 3 wide in 6
        ct = d[f"{name}-merge"]
        assert not ct.prior_touch and ct.joins and set(ct.prior_vars) <= set(ct.Sv) and len(ct.Sv) > len(ct.prior_vars)
        ct = d[f"{name}-empty"]
        assert ct.rewrap and not ct.touch.any() and ct.Sv == sorted(ct.prior_vars)
        for which in ("pose", "point", "merge", "empty"):
            g0, g1 = d[f"{name}-{which}"].g, d[f"{name}-{which}-moved"].g
            assert np.array_equal(g0.prior.lin_state, g1.prior.lin_state) and not np.array_equal(g0.var_state, g1.var_state)
    step = lambda c: np.abs(d[c].g.var_state - SR.graph("kept_hybrid").var_state).max()      # noqa: E731
    for c in ("kept_hybrid-pose-moved1e-6", "kept_hybrid-merge-moved1e-6"):      # the second magnitude, beside the eight at 1e-2
        assert 1e-7 < step(c) < 1e-5
    for name in ("kept_hybrid", "kept_chain"):
        for which in ("pose", "point", "merge", "empty"):
            c = f"{name}-{which}-moved"
            assert 1e-3 < np.abs(d[c].g.var_state - SR.graph(name).var_state).max() < 1e-1, c


@pytest.mark.parametrize("kind", sorted(MZ.ROBUST_KINDS))
def test_robust_constant_splits_the_point_factors(oracle, kind):
    """at least a quarter of the point factors down-weighted (|b| > k: Huber's weight below 1, Cauchy's below 1 / 2) and a quarter not,
    and no |b| within 1e-3 of k: the device cannot decide differently"""
    g, k, dist = MZ.robust_graph(kind)
    down = (dist > k).mean()
    print(f"{kind}: k = {k:.4f}, {len(dist)} point factors, {down:.2f} beyond k, least | |b| - k | / k = {np.abs(dist / k - 1).min():.2e}")
    assert 0.25 <= down <= 0.75
    assert np.abs(dist / k - 1).min() > 1e-3
    assert all(b.loss == MZ.ROBUST_KINDS[kind] for b in g.blocks if b.huber_k is not None)
    plain, weighted = SR.oracle_records("degree"), MZ.oracle_records_of(g)
    changed = np.array([not np.array_equal(a[1], b[1]) for a, b in zip(plain, weighted)])
    assert changed.any() and not changed.all()


# ---------------------------------------------------------------------------------------------- planted mistakes
def reach(cc, plant):
    """can the plant change anything on this case?"""
    ct = cc.cut
    rows, n_elim, p, n_raw = MZ.layout(ct)
    moved = ct.g.prior is not None and not all(np.array_equal(ct.g.var_state[v], ct.g.prior.lin_state[k]) for k, v in enumerate(ct.prior_vars))
    return {"eta_offset": n_elim > 0 and n_raw % MZ.TILE != 0, "tile_short": n_elim > 0 and n_raw % MZ.TILE != 0, "untransposed": n_elim > 0,
            "yw_dropped": n_elim > 0, "uq2_dropped": len(p) > 0, "prior_gradient": moved}[plant]


# where conditioning hides a plant: (plant, case) -> why
HIDDEN = {}


@pytest.mark.parametrize("plant", [p for p in MZ.PLANTS if p != "loss_kind"])
def test_planted_mistakes_leave_the_tolerance(oracle, plant):
    seen = 0
    for case in ALL:
        cc = MZ.cpu_case(case)
        if not reach(cc, plant) or (plant, case) in HIDDEN:
            continue
        try:
            got = MZ.measure(cc.cut, cc.ref, *MZ.device_restatement(cc.cut, cc.recs, plant=plant))
        except np.linalg.LinAlgError:                # a later diagonal tile is no longer positive definite: the library would report it
            got = dict.fromkeys(MZ.MEASURES, np.inf)
        worst = max(got[k] / cc.tol[k] for k in MZ.MEASURES)
        print(f"{plant:14s} {case:34s} worst measure / tolerance {worst:.3g}")
        assert worst > 1.0, (plant, case, got)
        seen += 1
    assert seen >= 4, (plant, seen)


def test_ignored_loss_kind_leaves_the_tolerance(oracle):
    """Cauchy's weights replaced by Huber's (a scratch graph that drops the block's loss kind), and no weights at all (one that drops
    the constant): the marginal of those records against the reference of the Cauchy records"""
    from . import robust_oracle as RO
    cc = MZ.cpu_case("degree-cauchy-old")
    g = cc.g
    for what, other in (("huber for cauchy", RO.with_loss(g, RO.HUBER)), ("no loss", SR.graph("degree"))):
        got = MZ.measure(cc.cut, cc.ref, *MZ.device_restatement(cc.cut, MZ.oracle_records_of(other)))
        print(what, {k: f"{got[k] / cc.tol[k]:.3g}" for k in MZ.MEASURES})
        assert got["pose"] > 1e6 * cc.tol["pose"] and got["eta"] > 1e6 * cc.tol["eta"]


def test_bounds_of_the_nearly_singular_prior_separate_the_two_accumulations():
    """MZ.singular_prior_graph() on the CPU: the form cancels almost eight digits; eta - Lambda dx and Q(dx) evaluated with the rows
    accumulated in twice the working precision (Dot2: TwoProduct, TwoSum) are inside the bounds of MZ.prior_measures, a plain
    accumulation of the same rows is outside both by more than ten times"""
    g = MZ.singular_prior_graph()
    P = g.prior
    pv = [g.key_index(int(q)) for q in P.keys]
    dx = np.concatenate([(g.var_state[v, :3] - P.lin_state[k, :3]) if g.var_type[v] == G.VAR_POINT3 else np.zeros(6) for k, v in enumerate(pv)])

    def evaluate(twice):
        part, grad = 0.0, []
        for i in range(len(dx)):
            s = e = 0.0
            for a, b in zip(P.Lambda[i], dx):
                p = a * b
                pe = float(mp.mpf(float(a)) * mp.mpf(float(b)) - mp.mpf(p))          # the product's rounding error (an fma on the device)
                t = s + p
                z = t - s
                e += ((s - (t - z)) + (p - z)) + pe
                s = t
            v = s + e if twice else s
            grad.append(P.eta[i] - v)
            part += dx[i] * (0.5 * v - P.eta[i])
        return MZ.prior_measures(g, grad, part + P.c)

    with mp.workdps(SR.DPS):
        (fine, tol, cancel), (plain, _t, _c) = evaluate(True), evaluate(False)
    print(f"cancellation {cancel:.2e}; bounds {tol}; twice the precision {fine}; plain {plain}")
    assert cancel > 1e7
    assert fine["eta"] <= tol["eta"] and fine["c"] <= tol["c"]
    assert plain["eta"] > 10 * tol["eta"] and plain["c"] > 10 * tol["c"]
