"""TEST INFRASTRUCTURE ONLY (never imported by the product).  What the CPU restatements of the batched motion-solver RANSACs
(tests/pnp_oracle.py, tests/pointcloud_oracle.py, tests/relpose_oracle.py) share, as dynosam_amd/csrc/ransac_batch.h is shared by their
kernels: the IEEE rounding helpers, the bearing, left . T, the K-slot prefix of the sampler of oracle/ransac_oracle.py and the selection -
every operation in Python floats (IEEE fp64, one rounding per operation) in the kernels' order.  No test_ prefix, pytest does not collect
it."""
from __future__ import annotations

import math

import numpy as np

from oracle.ransac_oracle import M64, MAX_ATTEMPTS, splitmix64

DEFAULT_HYPOTHESES = 512
IDENTITY12 = np.array([1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])


def _d(a, b):
    """a / b with IEEE semantics (Python raises where the device returns inf / nan)"""
    try:
        return a / b
    except ZeroDivisionError:
        return math.nan if a == 0.0 or a != a else math.copysign(math.inf, a) * math.copysign(1.0, b)


def _sqrt(x):
    return math.sqrt(x) if x >= 0.0 or x != x else math.nan


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def bearing(K, u, v):
    """ransac_bearing: the unit bearing of pixel (u, v) under K = (fx, fy, skew, u0, v0)"""
    fx, fy, skew, u0, v0 = (float(k) for k in K)
    y = _d(v - v0, fy)
    x = _d(u - u0 - skew * y, fx)
    n = _sqrt(x * x + y * y + 1.0)
    return (_d(x, n), _d(y, n), _d(1.0, n))


def compose(left, T):
    """ransac_compose: left . T (12 floats each)"""
    L = [float(v) for v in left]
    R = [(L[3 * i] * T[j] + L[3 * i + 1] * T[3 + j]) + L[3 * i + 2] * T[6 + j] for i in range(3) for j in range(3)]
    return np.array(R + [((L[3 * i] * T[9] + L[3 * i + 1] * T[10]) + L[3 * i + 2] * T[11]) + L[9 + i] for i in range(3)])


def sample_k(h: int, n: int, k: int):
    """ransac_sample<k>: k distinct indices in [0, n), slots 0..k-1 of the generator of oracle/ransac_oracle.py:sample (which draws four);
    None: MAX_ATTEMPTS duplicates in one slot"""
    idx = []
    for j in range(k):
        t = 0
        while True:
            c = splitmix64((h * 1315423911 + j * 2654435761 + t * 97) & M64) % n
            if c not in idx:
                idx.append(c)
                break
            t += 1
            if t >= MAX_ATTEMPTS:
                return None
    return idx


def select(n_hypotheses, hypothesis, inliers):
    """k_ransac_score + k_ransac_select: hypothesis(h) is the model of hypothesis h (None: no model), inliers(model) its bool mask.  The
    model with the most inliers wins, ties go to the lowest index, and its mask is computed again.
    returns (best index or -1, its count, its model, its mask - None, None without a winner -, the count of every hypothesis)"""
    best, best_n, best_T, sc = -1, 0, None, []
    for h in range(n_hypotheses if n_hypotheses > 0 else DEFAULT_HYPOTHESES):
        T = hypothesis(h)
        c = int(inliers(T).sum()) if T is not None else 0
        sc.append(c)
        if c > best_n:
            best, best_n, best_T = h, c, T
    return best, best_n, best_T, (inliers(best_T) if best >= 0 else None), sc
