"""tests/rectify_oracle.py against itself and against a 50-digit evaluation of the same formulas (CPU only): the reference the GPU tests of
tests/test_gpu_rectify.py compare the device with has to be right first."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import rectify_oracle as ro  # noqa: E402

K_RAW = np.array([[458.654, 0.0, 367.215], [0.0, 457.296, 248.375], [0.0, 0.0, 1.0]])
P_RECT = np.array([[420.0, 0.0, 320.0], [0.0, 420.0, 240.0], [0.0, 0.0, 1.0]])
D_RADTAN = [-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05, -0.004, 0.01, -0.002, 0.0005]
D_EQUI = [-0.013721808247486035, 0.020727425669427896, -0.012786476702685545, 0.0025242267320687625]


def rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    return (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]))


def test_fixed_point_bilinear_stays_within_its_quantisation_of_the_exact_value():
    """each coordinate is quantised to 1/32 px (at most 1/64 off, and a unit step in one coordinate moves a bilinear value of u8 data by at
    most 255 per pixel: 2 * 255 / 64 = 2^-5 * 255 for the two coordinates) and the output to a whole number (0.5)"""
    rng = np.random.default_rng(5)
    raw = rng.integers(0, 256, (37, 53, 3), dtype=np.uint8)
    raw[::5, ::3] = 0
    raw[1::5, 1::3] = 255
    mx = rng.uniform(-3.0, 56.0, (40, 64)).astype(np.float32)
    my = rng.uniform(-3.0, 40.0, (40, 64)).astype(np.float32)
    got = ro.remap_linear(raw, mx, my).astype(np.float64)
    exact = ro.bilinear_exact(raw, mx.astype(np.float64), my.astype(np.float64))
    err = np.abs(got - exact).max()
    print("fixed-point bilinear: largest difference from the exact value", err)
    assert err <= 0.5 + 2.0 ** -5 * 255


def _maps_mp(model, K, D, R, P, width, height, us, vs):
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    f = lambda a: [mp.mpf(float(v)) for v in np.asarray(a, np.float64).reshape(-1)]
    Km, d, Rm, Pm = f(K), f(list(D) + [0.0] * (8 - len(D))), mp.matrix(3, 3), mp.matrix(3, 3)
    for i in range(3):
        for j in range(3):
            Rm[i, j], Pm[i, j] = mp.mpf(float(R[i][j])), mp.mpf(float(P[i][j]))
    iM = (Pm * Rm) ** -1
    out = np.zeros((len(vs), len(us), 2))
    for a, v in enumerate(vs):
        for b, u in enumerate(us):
            q = iM * mp.matrix([u, v, 1])
            x, y = q[0] / q[2], q[1] / q[2]
            r2 = x * x + y * y
            if model == ro.RADTAN:
                kr = (1 + ((d[4] * r2 + d[1]) * r2 + d[0]) * r2) / (1 + ((d[7] * r2 + d[6]) * r2 + d[5]) * r2)
                xd = x * kr + 2 * d[2] * x * y + d[3] * (r2 + 2 * x * x)
                yd = y * kr + d[2] * (r2 + 2 * y * y) + 2 * d[3] * x * y
            elif model == ro.EQUIDISTANT:
                r = mp.sqrt(r2)
                t = mp.atan(r)
                s = 1 if r == 0 else t * (1 + d[0] * t ** 2 + d[1] * t ** 4 + d[2] * t ** 6 + d[3] * t ** 8) / r
                xd, yd = x * s, y * s
            else:
                xd, yd = x, y
            out[a, b] = float(Km[0] * xd + Km[1] * yd + Km[2]), float(Km[4] * yd + Km[5])
    return out


@pytest.mark.parametrize("model,D", [(ro.RADTAN, D_RADTAN), (ro.EQUIDISTANT, D_EQUI)])
def test_fp64_maps_agree_with_a_50_digit_evaluation(model, D):
    W, H = 640, 480
    R = rot(0.02, -0.03, 0.01)
    Ks = K_RAW.copy()
    Ks[0, 1] = 0.3                      # a skew, so that its term is exercised
    us, vs = np.linspace(0, W - 1, 9).round(), np.linspace(0, H - 1, 7).round()
    mx, my = ro.maps_f64(model, Ks, D, R, P_RECT, W, H)
    ref = _maps_mp(model, Ks, D, R, P_RECT, W, H, us, vs)
    got = np.stack([mx[np.ix_(vs.astype(int), us.astype(int))], my[np.ix_(vs.astype(int), us.astype(int))]], axis=2)
    err = np.abs(got - ref).max()
    print("maps against 50 digits, 9 x 7 grid: largest difference", err, "px")
    assert err <= 1e-10


def _grid_points(n=11, half=0.45):
    g = np.linspace(-half, half, n)
    x, y = np.meshgrid(g, g)
    return x.reshape(-1), y.reshape(-1)


def test_distort_then_undistort_returns_the_equidistant_point():
    x, y = _grid_points(half=0.9)
    u, v = ro.distort(ro.EQUIDISTANT, K_RAW, D_EQUI, x, y)
    back = ro.undistort_points(ro.EQUIDISTANT, K_RAW, D_EQUI, None, K_RAW, np.stack([u, v], 1))
    ideal = np.stack([K_RAW[0, 0] * x + K_RAW[0, 2], K_RAW[1, 1] * y + K_RAW[1, 2]], 1)
    err = np.abs(back - ideal).max()
    print("equidistant distort o undistort: largest residual", err, "px")
    assert err < 1e-9


def test_distort_then_undistort_radtan_residual_is_reported():
    """five fixed-point steps are not converged by design: the residual is printed (DESIGN.md section 7 records it), not gated"""
    x, y = _grid_points()
    for k1 in (-0.1, -0.05, 0.05, 0.1):
        D = [k1, 0.01, 0.0005, -0.0003]
        u, v = ro.distort(ro.RADTAN, K_RAW, D, x, y)
        back = ro.undistort_points(ro.RADTAN, K_RAW, D, None, K_RAW, np.stack([u, v], 1))
        ideal = np.stack([K_RAW[0, 0] * x + K_RAW[0, 2], K_RAW[1, 1] * y + K_RAW[1, 2]], 1)
        err = np.abs(back - ideal).max()
        print(f"radtan k1 = {k1:+.2f}: residual of the five-step inverse {err:.3e} px")
        assert np.isfinite(err)


def test_model_none_with_P_equal_K_is_the_identity():
    W, H = 64, 24
    mx, my = ro.maps(ro.NONE, P_RECT, None, None, P_RECT, W, H)
    v, u = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    assert np.array_equal(mx, u) and np.array_equal(my, v)
    rng = np.random.default_rng(1)
    rgb = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    mask = rng.integers(-5, 2 ** 31 - 1, (H, W)).astype(np.int32)
    depth = rng.uniform(0.1, 80.0, (H, W))
    assert np.array_equal(ro.remap_linear(rgb, mx, my), rgb)
    assert np.array_equal(ro.remap_nearest(mask, mx, my), mask) and np.array_equal(ro.remap_nearest(depth, mx, my), depth)
    assert ro.valid(mx, my, W, H)[:-1, :-1].all() and not ro.valid(mx, my, W, H)[-1].any() and not ro.valid(mx, my, W, H)[:, -1].any()


def test_coordinate_rules_ties_negatives_and_non_finite_values():
    raw = np.arange(1, 9, dtype=np.uint8).reshape(1, 8) * 30                    # one row: 30 60 ... 240
    row = lambda m: ro.remap_linear(raw, np.asarray([m], np.float32), np.zeros((1, len(m)), np.float32))[0]
    # 1/64 and 3/64 are ties of rintf(32 m): to even -> 0/32 and 2/32
    assert list(row([2 + 1 / 64, 2 + 3 / 64])) == [90, (30 * 32 * 32 * 90 + 2 * 32 * 32 * 120 + 16384) >> 15]
    # -1/32: arithmetic shift gives ix = -1, ax = 31; -1: every tap outside but one with weight 0
    assert list(row([-1 / 32, -1.0, 7.0, 7 + 1 / 32, 8.0])) == [(31 * 32 * 32 * 30 + 16384) >> 15, 0, 240, (31 * 32 * 32 * 240 + 16384) >> 15, 0]
    assert list(row([np.nan, np.inf, -np.inf, 16384.0, -16384.0, 1e30, -1e30])) == [0] * 7
    lab = np.arange(10, 18, dtype=np.int32).reshape(1, 8)
    near = ro.remap_nearest(lab, np.asarray([[0.5, 1.5, 2.5, -0.5, 7.5, np.nan, 16384.0]], np.float32), np.zeros((1, 7), np.float32))
    assert list(near[0]) == [10, 12, 12, 10, 0, 0, 0]                           # ties to even; 7.5 -> 8 is outside
