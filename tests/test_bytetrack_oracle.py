"""tests/bytetrack_oracle.py is trusted before it judges the device (tests/test_gpu_bytetrack.py): its assignment is optimal, its
four-filter Kalman form is ByteTrack's dense 8-state filter, and every scenario of tests/bytetrack_scenarios.py exercises what it is
for.  CPU only, no device call."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import bytetrack_oracle as O  # noqa: E402
from tests import bytetrack_scenarios as S  # noqa: E402

f32 = np.float32


def _assignment_cases():
    """(cost rows with None for non-edges, qL): 320 seeded cases, sizes 1..12 on both sides, half the pairs non-edges; every case with
    k % 3 == 0 (107 of them, a third) has its costs on a grid of 2^17 (1/8 of the scale), so that many totals tie"""
    rng = np.random.default_rng(2022)
    for k in range(320):
        nr, nc = int(rng.integers(1, 13)), int(rng.integers(1, 13))
        qL = int(rng.integers(1, 9)) << 17 if k % 3 == 0 else int(rng.integers(1, O.QMAX + 2))
        if k % 3 == 0:
            q = rng.integers(0, 9, (nr, nc)) << 17
        else:
            q = rng.integers(0, O.QMAX + 1, (nr, nc))
        edge = (rng.random((nr, nc)) < 0.5) & (q < qL)
        yield [[int(q[i, j]) if edge[i, j] else None for j in range(nc)] for i in range(nr)], qL, k % 3 == 0


def test_assignment_is_optimal_and_potentials_stay_in_int32():
    """the total integer cost equals scipy.optimize.linear_sum_assignment's on rows x (columns + private columns), non-edges at a cost
    above any feasible total; no case is left out"""
    from scipy.optimize import linear_sum_assignment
    n_cases = n_tied = 0
    stats = {}
    for cost, qL, tied in _assignment_cases():
        nr, nc = len(cost), len(cost[0])
        big = 13 * (O.QMAX + 2)
        M = np.full((nr, nc + nr), big, np.int64)
        for i in range(nr):
            for j in range(nc):
                if cost[i][j] is not None:
                    M[i, j] = cost[i][j]
            M[i, nc + i] = qL
        r, c = linear_sum_assignment(M)
        best = int(M[r, c].sum())
        r2c, c2r = O.assign(cost, qL, stats)
        assert O.total_cost(cost, qL, r2c) == best, (n_cases, cost, qL)
        real = [c for c in r2c if c >= 0]
        assert len(set(real)) == len(real) and all(c == O.PRIVATE or cost[i][c] is not None for i, c in enumerate(r2c))
        assert all((c2r[c] == i) for i, c in enumerate(r2c) if c >= 0)
        n_cases += 1
        n_tied += tied
    assert n_cases >= 300 and 3 * n_tied >= n_cases
    assert stats["max_potential"] < (1 << 28)


def test_assignment_tie_rule():
    """all costs equal: rows take the columns in order (the lowest index on a tie); a pair at exactly qL is no edge"""
    cost = [[5, 5, 5], [5, 5, 5]]
    assert O.assign(cost, 6)[0] == [0, 1]
    assert O.assign([[None, 5], [5, 5]], 6)[0] == [1, 0]
    q = O.quant(f32(0.5))
    assert q == O.qlimit(0.5) == 1 << 19                    # q < qL is false at the limit: the caller passes None for it
    assert O.quant(f32(np.nan)) is None and O.quant(f32(-3.0)) == 0 and O.quant(f32(7.0)) == O.QMAX and O.qlimit(1e30) == O.QMAX + 1


def _dense_filter(zs):
    """ByteTrack's 8-state constant-velocity filter in float64, dense matrices: mean [8] = (cx, cy, a, h, vcx, vcy, va, vh)"""
    wp, wv = 1.0 / 20.0, 1.0 / 160.0
    Fm = np.eye(8)
    Fm[:4, 4:] = np.eye(4)
    H = np.eye(4, 8)
    z = zs[0]
    mean = np.concatenate([z, np.zeros(4)])
    std = [2 * wp * z[3], 2 * wp * z[3], 1e-2, 2 * wp * z[3], 10 * wv * z[3], 10 * wv * z[3], 1e-5, 10 * wv * z[3]]
    cov = np.diag(np.square(std))
    out = [(mean.copy(), cov.copy())]
    for z in zs[1:]:
        h = mean[3]
        Q = np.diag(np.square([wp * h, wp * h, 1e-2, wp * h, wv * h, wv * h, 1e-5, wv * h]))
        mean, cov = Fm @ mean, Fm @ cov @ Fm.T + Q
        h = mean[3]
        R = np.diag(np.square([wp * h, wp * h, 1e-1, wp * h]))
        Sm = H @ cov @ H.T + R
        K = cov @ H.T @ np.linalg.inv(Sm)
        mean, cov = mean + K @ (z - H @ mean), cov - K @ Sm @ K.T
        out.append((mean.copy(), cov.copy()))
    return out


# measured on this sequence (fp32 four-filter form against the float64 dense filter, relative to the largest entry of each quantity):
FILTER_MEAN_ERR, FILTER_COV_ERR = 6.1e-8, 3.0e-7


def test_four_filters_are_the_dense_filter():
    """Over 30 steps of a moving, growing box the four (position, velocity) filters agree with the dense float64 8-state filter
    (F P F' + Q, K = P H' S^-1).  Measured difference, relative to the largest entry: mean 6.1e-8, covariance 3.0e-7 (fp32 rounding
    accumulated over 30 steps); asserted at 4x those.  The dense filter's cross-coordinate covariance is exactly 0."""
    rng = np.random.default_rng(7)
    zs = []
    for f in range(31):
        w, h = 60 + 2.0 * f, 80 + 3.0 * f
        b = np.array([100 + 4.0 * f - w / 2, 120 + 2.5 * f - h / 2, 100 + 4.0 * f + w / 2, 120 + 2.5 * f + h / 2]) + rng.uniform(-1, 1, 4)
        zs.append(O.to_xyah(b.astype(f32)))
    dense = _dense_filter([z.astype(np.float64) for z in zs])
    kf = O.kf_initiate(zs[0])
    e_mean = e_cov = 0.0
    for k, z in enumerate(zs):
        if k:
            O.kf_predict(kf)
            O.kf_update(kf, z)
        mean, cov = dense[k]
        for a in range(8):
            for b in range(8):
                if a % 4 != b % 4:
                    assert cov[a, b] == 0.0
        got_mean = np.array([kf[5 * c] for c in range(4)] + [kf[5 * c + 1] for c in range(4)], np.float64)
        got_cov = np.zeros((8, 8))
        for c in range(4):
            got_cov[c, c], got_cov[c, 4 + c], got_cov[4 + c, c], got_cov[4 + c, 4 + c] = kf[5 * c + 2], kf[5 * c + 3], kf[5 * c + 3], kf[5 * c + 4]
        e_mean = max(e_mean, np.abs(got_mean - mean).max() / np.abs(mean).max())
        e_cov = max(e_cov, np.abs(got_cov - cov).max() / np.abs(cov).max())
    print(f"four-filter form vs dense float64 filter: mean {e_mean:.3e}, covariance {e_cov:.3e}")
    assert 0 < e_mean <= 4 * FILTER_MEAN_ERR and 0 < e_cov <= 4 * FILTER_COV_ERR


@pytest.mark.parametrize("name", sorted(S.SCENARIOS))
def test_scenario_exercises_what_it_is_for(name):
    frames, p, check = S.scenario(name)
    res = O.track(frames, p)
    check(res)
    for (r, t), (b, s, c) in zip(res, frames):
        assert len(r["labels"]) == len(b) and list(t["id"]) == sorted(t["id"]) and len(set(t["id"])) == len(t["id"])
        lab = r["labels"][r["labels"] > 0]
        assert len(set(lab)) == len(lab)                        # an id labels one detection
        assert r["n_tracks"] == len(r["tracks"]) and [k["id"] for k in r["tracks"]] == sorted(k["id"] for k in r["tracks"])


def test_cluster_cases_fill_the_assignment():
    """the cap cases of the device test: every pair of the cluster is an edge at a limit above 1, so the first association is a full
    256 x 256 problem; on the coarse grid many costs tie"""
    frames = S.cluster(12, 12, 1, grid=16.0)
    b = frames[0][0]
    d = [O.quant(f32(1) - O.iou(b[i], frames[-1][0][j])) for i in range(12) for j in range(12)]
    assert max(d) < O.QMAX and len(set(d)) < len(d) // 2        # all overlap; ties
    res = O.track(frames, dict(match_thresh=2.0))
    assert (res[-1][0]["labels"] > 0).sum() == 12


def test_staircase_has_long_augmenting_paths():
    t = O.Tracker(match_thresh=2.0)
    for b, s, c in S.staircase(40):
        r = t.update(b, s, c)
    assert t.stats["steps"] == 40 * 39 // 2 and (r["labels"] > 0).all() and t.stats["max_potential"] < (1 << 28)
