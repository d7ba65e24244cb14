"""The numpy restatement of gtsam::GncOptimizer (tests/gnc_oracle.py) on a small HYBRID graph with injected gross outliers: what it
removes, where it stops, and its edge cases.  CPU only, no device call.

The graph: make_hybrid_graph(config(1, frames=6, static_points=16, dynamic_points_per_object=8, robust=False)), corrupt(seed=11):
149 factors, 24 of them outliers of 30..60 whitened sigmas; the prior, between and smoothing classes are known inliers."""
import functools

import numpy as np

from dynosam_amd import graph as G
from dynosam_amd import synth
from tests import gnc_oracle as N


@functools.lru_cache(maxsize=None)
def corrupted():
    g = synth.make_hybrid_graph(synth.config(1, frames=6, static_points=16, dynamic_points_per_object=8, robust=False))
    g2, out = N.corrupt(g, seed=11)
    return g, g2, out, N.structural_inliers(g2)


def test_the_injector():
    g, g2, out, ki = corrupted()
    assert (g2.n_factors, len(out), len(ki)) == (149, 24, 11)
    dims = N.factor_dims(g2)
    assert set(dims[ki]) == {6} and set(dims[out]) == {3}
    # one outlier per point at most, each 30..60 whitened sigmas away from the clean measurement
    f, pts = 0, []
    for b, b2 in zip(g.blocks, g2.blocks):
        for i in range(b.count):
            if f + i in out:
                u = b.noise[i].reshape(3, 3) @ (b2.meas[i] - b.meas[i])
                assert 30.0 <= np.linalg.norm(u) <= 60.0
                pts.append(int(b.var_idx[i, 1 if b.type == G.F_POSE_TO_POINT else 2]))
            else:
                assert np.array_equal(b.meas[i], b2.meas[i])
        f += b.count
    assert len(set(pts)) == len(pts) == 24


def test_tls_removes_exactly_the_injected_outliers(oracle):
    _g, g2, out, ki = corrupted()
    T = N.optimize(oracle, g2, loss=N.TLS, known_inliers=ki)
    assert (T["iterations"], T["stop_reason"], T["n_unknown"]) == (25, 2, 149 - 11)
    assert abs(T["mu_initial"] - 1.29e-3) < 1e-5
    w = T["weights"]
    clean = np.setdiff1d(np.where(T["unknown"])[0], out)
    assert np.all(w[out] == 0.0) and np.all(w[clean] == 1.0) and np.all(w[ki] == 1.0)
    assert (T["n_zero_weight"], T["n_unit_weight"]) == (24, 125)
    # ... and the values are those of LM on the graph without the 24 factors, bit for bit
    og = oracle.OracleGraph(N.pruned_graph(g2, out))
    og.optimize()
    assert np.array_equal(T["state"], og.state())
    # plain LM on the corrupted graph ends far away from it
    og2 = oracle.OracleGraph(g2)
    og2.optimize()
    assert np.abs(og2.state() - og.state()).max() > 10.0
    assert N.decision_margin(T) >= 1e-6


def test_gm_ends_by_the_mu_rule(oracle):
    _g, g2, out, ki = corrupted()
    T = N.optimize(oracle, g2, loss=N.GM, known_inliers=ki)
    assert T["stop_reason"] == 3 and T["mu_final"] == 1.0 and T["trace_mu"][-1] == 1.0
    w = T["weights"]
    clean = np.setdiff1d(np.where(T["unknown"])[0], out)
    print("GM: largest outlier weight", w[out].max(), "smallest clean weight", w[clean].min())
    assert w[out].max() < 1e-3 and w[clean].min() > 0.1
    assert np.all(w[ki] == 1.0)
    mu = np.array(T["trace_mu"][1:])
    assert np.allclose(mu[1:], np.maximum(1.0, mu[:-1] / 1.4), rtol=1e-15, atol=0)


def test_degenerate_start_on_a_clean_noiseless_graph(oracle):
    g = synth.make_hybrid_graph(synth.config(1, frames=6, static_points=16, dynamic_points_per_object=8, robust=False, noise_scale=0.0))
    T = N.optimize(oracle, g, loss=N.TLS, known_inliers=N.structural_inliers(g))
    assert (T["mu_initial"], T["iterations"], T["stop_reason"]) == (-1.0, 0, 4)
    assert len(T["trace_mu"]) == 1 and np.all(T["weights"] == 1.0)


def test_known_outliers_are_never_reweighted(oracle):
    _g, g2, out, ki = corrupted()
    clean = np.setdiff1d(np.arange(g2.n_factors), np.concatenate([out, ki]))[:3]
    ko = np.concatenate([out[:5], clean])
    for loss in (N.TLS, N.GM):
        T = N.optimize(oracle, g2, loss=loss, known_inliers=ki, known_outliers=ko)
        assert np.all(T["weights"][ko] == 0.0) and np.all(T["weights"][ki] == 1.0)
        for s in T["steps"]:
            assert np.all(s["w"][ko] == 0.0) and np.all(s["w"][ki] == 1.0)
        assert T["n_unknown"] == g2.n_factors - len(ki) - len(ko)
    # no unknown factor at all: the first LM is the answer
    T = N.optimize(oracle, g2, known_inliers=np.setdiff1d(np.arange(g2.n_factors), out), known_outliers=out)
    assert (T["iterations"], T["stop_reason"]) == (0, 4)


def test_an_unknown_six_row_factor_at_weight_zero_gives_finite_numbers(oracle):
    """a between factor with a grossly wrong measurement, left unknown: TLS drives it to weight 0, that is to infinite sigmas"""
    _g, g2, _out, _ki = corrupted()
    blocks, bad, f = [], None, 0
    for b in g2.blocks:
        if b.type == G.F_BETWEEN_POSE3:
            meas = b.meas.copy()
            meas[1, 9:12] += 5.0
            b = G.FactorBlock(b.type, b.slot, b.var_idx, meas, b.noise, b.huber_k, b.consts)
            bad = f + 1
        blocks.append(b)
        f += b.count
    g3 = G.FlatGraph(g2.var_keys, g2.var_type, g2.var_state, blocks, dict(g2.meta), g2.prior)
    ki = np.setdiff1d(N.structural_inliers(g3), [bad])
    T = N.optimize(oracle, g3, loss=N.TLS, known_inliers=ki)
    assert T["weights"][bad] == 0.0
    assert np.isfinite(T["state"]).all() and np.isfinite(T["trace_cost"]).all() and np.isfinite(T["error_after"])
    wg = N.weighted_graph(g3, T["weights"], T["state"])
    assert np.isinf(wg.blocks[[b.type for b in wg.blocks].index(G.F_BETWEEN_POSE3)].noise[1]).all()
    J, b, e = oracle.OracleGraph(wg).linearize()
    assert np.isfinite(J).all() and np.isfinite(b).all() and np.isfinite(e).all()
    assert not J[bad].any() and not b[bad].any() and e[bad] == 0.0
