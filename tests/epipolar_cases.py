"""TEST INFRASTRUCTURE ONLY.  The scenes tests/test_epipolar_reference.py (the fp64 oracle, CPU) and
tests/test_gpu_epipolar_reference.py (the device) hold to tests/epipolar_reference.py, the per-hypothesis comparison they share and
a cache of the 50-digit models, so that a model is solved once per (scene, hypothesis) whoever asks first."""
from __future__ import annotations

import functools

import numpy as np

from oracle import ransac_oracle as RO
from tests import epipolar_reference as ER
from tests.test_ransac_oracle import planted, planted_stereo

FX, BASELINE = 700.0, 0.12
REF_CAP = 48          # hypotheses per case solved in 50 digits (~45 ms each); every hypothesis is compared with the oracle bit for bit


def general_motion(n=160, n_out=25, seed=0, noise=0.2, planar=False):
    """two views of a 3D scene under a rotation of a few degrees and a translation with all three components (not rectified)"""
    rng = np.random.default_rng(seed)
    K = np.array([[700.0, 0, 320], [0, 700.0, 240], [0, 0, 1]])
    X = np.c_[rng.uniform(-4, 4, n), rng.uniform(-3, 3, n), rng.uniform(4, 20, n)]
    if planar:
        X[:, 2] = 9.0 + 0.3 * X[:, 0] - 0.2 * X[:, 1]
    w = np.array([0.03, -0.05, 0.02])
    th = np.linalg.norm(w); k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
    t = np.array([0.4, -0.1, 0.25])
    p1 = X @ K.T; p2 = (X @ R.T + t) @ K.T
    a = p1[:, :2] / p1[:, 2:]; b = p2[:, :2] / p2[:, 2:] + rng.normal(0, noise, (n, 2))
    out = rng.choice(n, n_out, replace=False)
    b[out] += rng.uniform(6, 40, (n_out, 2)) * rng.choice([-1, 1], (n_out, 2))
    return a.astype(np.float32), b.astype(np.float32), out


def equal_rows(n=160, n_out=25, seed=0):
    """the production input after FeatureTracker.stereo_track: right row == left row exactly, float disparities"""
    rng = np.random.default_rng(seed)
    left = rng.uniform([30, 30], [610, 450], (n, 2)).astype(np.float32)
    right = left.copy()
    right[:, 0] = (left[:, 0].astype(np.float64) - FX * BASELINE / rng.uniform(2.0, 30.0, n)).astype(np.float32)
    out = rng.choice(n, n_out, replace=False)
    right[out, 1] += (rng.uniform(4, 30, n_out) * rng.choice([-1, 1], n_out)).astype(np.float32)
    return left, right, out


def constant_disparity(n=120, d=9.0, seed=0):
    rng = np.random.default_rng(seed)
    left = rng.uniform([30, 30], [610, 450], (n, 2)).astype(np.float32)
    right = left.copy(); right[:, 0] -= np.float32(d)
    return left, right


def _key(a, b):
    return (np.ascontiguousarray(a, np.float32).tobytes(), np.ascontiguousarray(b, np.float32).tobytes())


@functools.lru_cache(maxsize=None)
def _ref_h(key, h):
    a = np.frombuffer(key[0], np.float32).reshape(-1, 2); b = np.frombuffer(key[1], np.float32).reshape(-1, 2)
    idx = RO.sample(h, len(a))          # (the index generator is integer arithmetic, pinned by test_ransac_oracle)
    return None if idx is None else ER.homography4(a[idx], b[idx])


@functools.lru_cache(maxsize=None)
def _ref_f(key, h):
    a = np.frombuffer(key[0], np.float32).reshape(-1, 2); b = np.frombuffer(key[1], np.float32).reshape(-1, 2)
    idx = RO.sample7(h, len(a))
    return [] if idx is None else ER.seven_point(a[idx], b[idx])


def ref_homography(a, b, h):
    return _ref_h(_key(a, b), int(h))


def ref_fundamental(a, b, h):
    return _ref_f(_key(a, b), int(h))


def which(K, best, cap=REF_CAP):
    """the hypotheses of a case that are held to the 50-digit reference: the first `cap`, the winner, and the ends of the 256-strides"""
    hs = set(range(min(K, cap))) | {h for h in (best, 255, 256, 257, K - 1) if 0 <= h < K}
    return sorted(hs)


def check_homography(a, b, thr, K, best, mask, score, model, cap=REF_CAP):
    """every capped hypothesis with a positive score within MARGIN x sensitivity of the reference, its score between the reference's
    decided and decided + undecided inliers; the winner's mask equal to the reference's decisions but for the undecided (at most 2 %).
    returns dict(worst ratio, models compared, undecided)"""
    a = np.asarray(a, np.float32).reshape(-1, 2); b = np.asarray(b, np.float32).reshape(-1, 2)
    thr2 = float(np.float32(thr * thr))
    worst, cnt, und = 0.0, 0, 0
    for h in which(K, best, cap):
        if score[h] <= 0:
            continue
        ref = ref_homography(a, b, h)
        assert ref is not None, f"hypothesis {h}: a model where the 50-digit system is singular"
        r = ER.homography_ratio(ref, model[h])
        assert r <= ER.MARGIN_H, f"hypothesis {h}: H is {r:.3g} sensitivities from the reference (margin {ER.MARGIN_H:.3g})"
        d = ER.decisions("H", ref.m, a, b, thr2, ER.DELTA_H)
        lo, hi = int((d == 1).sum()), int((d >= 0).sum())
        assert hi - lo <= 0.02 * len(a), f"hypothesis {h}: {hi - lo} undecided of {len(a)}"
        assert lo <= score[h] <= hi, f"hypothesis {h}: score {score[h]} outside [{lo}, {hi}]"
        if h == best:
            dec = d != 0
            assert np.array_equal(np.asarray(mask, bool)[dec], d[dec] == 1), f"winner {h}: mask differs from the reference's decisions"
            und = int((~dec).sum())
        worst, cnt = max(worst, r), cnt + 1
    return dict(worst=worst, compared=cnt, undecided=und)


def check_fundamental(a, b, thr, K, best, mask, score, model, cap=REF_CAP):
    """as check_homography; the stored model must be within tolerance of ONE of the reference's real solutions"""
    a = np.asarray(a, np.float32).reshape(-1, 2); b = np.asarray(b, np.float32).reshape(-1, 2)
    thr2 = float(thr * thr)
    worst, cnt, und, nsol = 0.0, 0, 0, []
    for h in which(K, best, cap):
        sols = ref_fundamental(a, b, h)
        nsol.append(len(sols))
        if score[h] <= 0:
            continue
        assert sols, f"hypothesis {h}: a model where the reference has no solution"
        rs = [ER.fundamental_ratio(s, model[h]) for s in sols]
        k = int(np.argmin(rs))
        assert rs[k] <= ER.MARGIN_F, f"hypothesis {h}: F is {rs[k]:.3g} sensitivities from the nearest of {len(sols)} solutions (margin {ER.MARGIN_F:.3g})"
        d = ER.decisions("F", sols[k].m, a, b, thr2, ER.DELTA_F)
        lo, hi = int((d == 1).sum()), int((d >= 0).sum())
        assert hi - lo <= 0.02 * len(a), f"hypothesis {h}: {hi - lo} undecided of {len(a)}"
        assert lo <= score[h] <= hi, f"hypothesis {h}: score {score[h]} outside [{lo}, {hi}]"
        if h == best:
            dec = d != 0
            assert np.array_equal(np.asarray(mask, bool)[dec], d[dec] == 1), f"winner {h}: mask differs from the reference's decisions"
            und = int((~dec).sum())
        worst, cnt = max(worst, rs[k]), cnt + 1
    return dict(worst=worst, compared=cnt, undecided=und, solutions=nsol)


# ---- the cases: name -> (a, b, threshold, n_hypotheses argument (0: the default 512), hypotheses held to the 50-digit reference) ----
def planted_h(n, n_out, seed, noise=0.3, size=(640, 480), H=None, out_lo=15.0):
    rng = np.random.default_rng(seed)
    w, h = size
    a = rng.uniform([20, 20], [w - 20, h - 20], (n, 2)).astype(np.float32)
    H = np.array([[1.01, 0.02, 3.0], [-0.015, 0.99, -2.0], [2e-5 * 640 / w, -1e-5 * 640 / w, 1.0]]) if H is None else H
    p = np.c_[a, np.ones(n)] @ H.T
    with np.errstate(all="ignore"):
        b = p[:, :2] / p[:, 2:] + rng.normal(0, noise, (n, 2))
    out = rng.choice(n, n_out, replace=False)
    b[out] += rng.uniform(out_lo, 4 * out_lo, (n_out, 2)) * rng.choice([-1, 1], (n_out, 2))
    return a, b.astype(np.float32), out


def line_plus_three():
    """noise-free, every correspondence an inlier of one H (a translation by whole pixels: exact in float32): 60 points exactly on a
    line and three off it, at positions 0, 2 and 21.  A sample is valid only with two of those three, which the index generator first
    draws at hypothesis 302 (then 315, 455, 503, ...): every valid hypothesis scores n, the first of them lies beyond the first
    256-stride of the argmax, and the lowest index must win the tie."""
    k = np.arange(60, dtype=np.float64)
    a = np.c_[40 + 8 * k, 60 + 5 * k]
    for pos, p in zip((0, 2, 21), ([100.0, 400.0], [500.0, 90.0], [320.0, 30.0])):
        a = np.insert(a, pos, p, axis=0)
    a = a.astype(np.float32)
    return a, a + np.float32([4.0, -3.0])


def homography_cases():
    c = {}
    for n in (4, 5, 63, 64, 65, 255, 256, 257, 1000):
        a, b, _ = planted_h(n, 0 if n == 4 else max(1, n // 5), 100 + n)
        c[f"n{n}"] = (a, b, 5.0, 0, 16)
    a, b, _ = planted_h(200, 40, 0)
    for K in (1, 2, 255, 256, 257, 0, 1000):
        c[f"K{K}"] = (a, b, 5.0, K, 16)
    for thr in (0.5, 5.0, 50.0):
        c[f"thr{thr}"] = (a, b, thr, 0, REF_CAP)
    a, b, _ = planted_h(300, 60, 7, size=(4096, 3072), out_lo=20.0)
    c["4096x3072"] = (a, b, 5.0, 0, 24)
    a, b, _ = planted_h(150, 30, 8)
    c["negative_subpixel"] = ((a - np.float32([333.25, 251.625])) * np.float32(0.37), (b - np.float32([333.25, 251.625])) * np.float32(0.37), 1.0, 0, 24)
    a, b, _ = planted_h(60, 10, 9)
    a[20:40], b[20:40] = a[:20], b[:20]                                  # twenty points twice: a sample with a repeat is collinear
    c["repeated"] = (a, b, 5.0, 0, 24)
    a, b, _ = planted_h(100, 0, 10, noise=0.0)
    c["mirrored"] = (a, (np.float32([640, 0]) + b * np.float32([-1, 1])).astype(np.float32), 5.0, 0, 8)
    # line at infinity 0.002 x + 0.001 y - 1 = 0 through the points' area: on 12 points placed on it w = 0 exactly or nearly
    Hinf = np.array([[1.0, 0.01, 2.0], [-0.01, 1.0, 1.0], [-0.002, -0.001, 1.0]])
    a, b, _ = planted_h(120, 0, 11, H=Hinf)
    a[:12, 0] = np.float32(250.0); a[:12, 1] = np.float32(500.0)        # 0.002 * 250 + 0.001 * 500 = 1, exact in fp32 products? nearly
    a[:12] += np.float32([[k, -2 * k] for k in range(12)])              # stays on the line: 0.002 k - 0.002 k
    p = np.c_[a.astype(np.float64), np.ones(len(a))] @ Hinf.T
    with np.errstate(all="ignore"):
        b = (p[:, :2] / p[:, 2:]).astype(np.float32)
    b[:12] = np.float32([300.0, 200.0])
    c["line_at_infinity"] = (a, b, 5.0, 0, 24)
    a, b = line_plus_three()
    c["line_plus_three"] = (a, b, 5.0, 1000, 8)
    return c


def stereo_scene(n, n_out, seed, noise=0.15, size=(640, 480)):
    rng = np.random.default_rng(seed)
    w, h = size
    left = rng.uniform([30, 30], [w - 30, h - 30], (n, 2))
    right = left.copy(); right[:, 0] -= FX * (w / 640) * BASELINE / rng.uniform(2.0, 30.0, n)
    right += rng.normal(0, noise, (n, 2))
    out = rng.choice(n, n_out, replace=False)
    right[out, 1] += rng.uniform(4, 30, n_out) * rng.choice([-1, 1], n_out)
    return left.astype(np.float32), right.astype(np.float32), out


def fundamental_cases():
    """name -> (left, right, status, threshold, n_hypotheses argument, reference cap)"""
    c = {}
    for n in (8, 9, 63, 64, 65, 256, 257):
        l, r, _ = stereo_scene(n, n // 6, 200 + n)
        c[f"n{n}"] = (l, r, np.ones(n, np.uint8), 1.0, 0, 16)
        pad = np.float32([[5.0, 5.0], [9.0, 400.0], [600.0, 7.0]])
        c[f"n{n}_status"] = (np.r_[pad, l], np.r_[pad + 50, r], np.r_[np.zeros(3, np.uint8), np.ones(n, np.uint8)], 1.0, 0, 16)
    l, r, _, _ = planted_stereo()
    one = np.ones(len(l), np.uint8)
    for K in (1, 2, 255, 256, 257, 0, 1000):
        c[f"K{K}"] = (l, r, one, 1.0, K, 16)
    c["thr0.25"] = (l, r, one, 0.25, 0, REF_CAP)
    c["thr1"] = (l, r, one, 1.0, 0, 112)                                  # (enough hypotheses for 20 samples with one real solution)
    l, r, _ = equal_rows()
    c["equal_rows"] = (l, r, one, 1.0, 0, REF_CAP)
    l, r, _ = general_motion()
    c["general_motion"] = (l, r, one, 1.0, 0, REF_CAP)
    l, r, _ = general_motion(n_out=0, noise=0.0, seed=3)
    c["ties"] = (l, r, one, 1.0, 0, 16)
    l, r, _ = general_motion(planar=True, seed=4)
    c["planar"] = (l, r, one, 1.0, 0, REF_CAP)
    l, r, _ = stereo_scene(200, 30, 12, size=(4096, 3072))
    c["4096x3072"] = (l, r, np.ones(200, np.uint8), 1.0, 0, 24)
    l, r, _ = general_motion(120, 20, 13)
    c["negative_subpixel"] = ((l - np.float32([333.25, 251.625])) * np.float32(0.37), (r - np.float32([333.25, 251.625])) * np.float32(0.37),
                              np.ones(120, np.uint8), 0.25, 0, 24)
    l, r, _ = stereo_scene(60, 8, 14)
    l[20:40], r[20:40] = l[:20], r[:20]
    c["repeated"] = (l, r, np.ones(60, np.uint8), 1.0, 0, 24)
    return c


def nonfinite(kind):
    """200 correspondences, number 17 with a NaN and number 101 with an Inf coordinate"""
    if kind == "H":
        a, b, _ = planted_h(200, 40, 21)
    else:
        a, b, _ = stereo_scene(200, 30, 22)
    a, b = a.copy(), b.copy()
    b[17, 0] = np.nan; a[101, 1] = np.inf
    return a, b


def same_bits(x, y):
    """bit equality of two float arrays, any NaN equal to any NaN (the sign and payload of a NaN an operation produces are not IEEE's)"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    nx, ny = np.isnan(x), np.isnan(y)
    return x.shape == y.shape and np.array_equal(nx, ny) and np.array_equal(x[~nx].view(np.uint64), y[~ny].view(np.uint64))


def first_best(score):
    """the first index of the largest positive score, -1 where there is none"""
    score = np.asarray(score)
    return int(np.argmax(score)) if len(score) and score.max() > 0 else -1
