"""Pin the CPU oracle against every known-answer fixture the reference's own tests hold for the
hot path:

  dynosam/test/test_factors.cc:134-196         LandmarkMotionTernaryFactor
  dynosam/test/test_hybrid_motion.cc:46-258    HybridObjectMotion / HybridMotionFactor
  dynosam/test/test_dynamic_point_symbol.cc:57-104, test_backend_structures.cc:39-94   key encoding

The reference's random perturbations (utils::perturbWithNoise ignores its seed) are replaced by
fixed constants; every explicit constant below is the reference's.
"""
import numpy as np
import pytest

from dynosam_amd import graph as G
from dynosam_amd import symbols as S
from dynosam_amd import synth as Y


def pose12(R, t):
    return np.concatenate([np.asarray(R, float).reshape(9), np.asarray(t, float)])


def retract12(O, p12, xi):
    return O.call_pose("orc_pose_retract", p12, xi)


def num_jac(O, ftype, states, kinds, meas, consts, delta=1e-5):
    """gtsam::numericalDerivative: central differences on the manifold."""
    e0, _ = O.eval_factor(ftype, states, meas, consts, want_J=False)
    d = G.F_LAYOUT[ftype][1]
    cols = []
    for v, kind in enumerate(kinds):
        w = 6 if kind == "pose" else 3
        Jv = np.zeros((d, w))
        for j in range(w):
            outs = []
            for sgn in (+1, -1):
                dx = np.zeros(w)
                dx[j] = sgn * delta
                st = [np.array(s, float) for s in states]
                st[v] = retract12(O, st[v], dx) if kind == "pose" else st[v] + dx
                e, _ = O.eval_factor(ftype, st, meas, consts, want_J=False)
                outs.append(e[:d])
            Jv[:, j] = (outs[0] - outs[1]) / (2 * delta)
        cols.append(Jv)
    return cols


def split_J(ftype, J, kinds):
    d = G.F_LAYOUT[ftype][1]
    return [J[:d, 6 * v:6 * v + (6 if k == "pose" else 3)] for v, k in enumerate(kinds)]


# ---- LandmarkMotionTernaryFactor (test_factors.cc:134-196) ------------------------------------
H_TERN = pose12(Y.so3_exp(np.array([-0.1, 0.2, 0.25])), [0.05, -0.10, 0.20])  # Rot3::Rodrigues
P1 = np.array([0.4, 1.0, 0.8])


def test_ternary_zero_error(oracle):
    R, t = Y.from12(H_TERN)
    P2 = R @ P1 + t
    e, _ = oracle.eval_factor(G.F_LANDMARK_TERNARY, [P1, P2, H_TERN])
    assert np.allclose(e[:3], 0, atol=1e-4)      # the reference's tolerance
    assert np.abs(e[:3]).max() < 1e-15


def test_ternary_jacobians(oracle):
    R, t = Y.from12(H_TERN)
    P2 = R @ P1 + t
    Hp = retract12(oracle, H_TERN, np.array([0.11, -0.23, 0.17, 0.2, -0.31, 0.26]))  # "perturbWithNoise(H, 0.3)"
    kinds = ["point", "point", "pose"]
    _, J = oracle.eval_factor(G.F_LANDMARK_TERNARY, [P1, P2, Hp])
    num = num_jac(oracle, G.F_LANDMARK_TERNARY, [P1, P2, Hp], kinds, None, None)
    for a, b in zip(split_J(G.F_LANDMARK_TERNARY, J, kinds), num):
        assert np.allclose(a, b, atol=1e-9)  # gtsam::assert_equal default tolerance


# ---- HybridMotionTest fixture (test_hybrid_motion.cc:71-99) -----------------------------------
X_k = pose12(Y.ypr(0.1, 0.2, 0.3), [1, 2, 3])
E_k = pose12(Y.ypr(0.4, 0.1, -0.2), [-1, 0.5, 2])
L_e = pose12(Y.ypr(-0.1, 0.0, 0.1), [0.1, 0.0, 0.0])
m_L = np.array([1.5, -0.5, 2.0])


def proj_cam(O, X, E, L, m):
    out = np.zeros(3)
    import ctypes as C
    dp = C.POINTER(C.c_double)
    fn = O.lib().orc_project_to_camera3
    fn.argtypes = [dp] * 9
    J = [np.zeros(18), np.zeros(18), np.zeros(18), np.zeros(9)]
    args = [np.ascontiguousarray(a, dtype=float) for a in (X, E, L, m)]
    fn(*[a.ctypes.data_as(dp) for a in args], out.ctypes.data_as(dp), *[j.ctypes.data_as(dp) for j in J])
    return out, [J[0].reshape(3, 6), J[1].reshape(3, 6), J[2].reshape(3, 6), J[3].reshape(3, 3)]


def proj_obj(O, X, E, L, Z):
    out = np.zeros(3)
    import ctypes as C
    dp = C.POINTER(C.c_double)
    fn = O.lib().orc_project_to_object3
    fn.argtypes = [dp] * 8
    J = [np.zeros(18), np.zeros(18), np.zeros(18)]
    args = [np.ascontiguousarray(a, dtype=float) for a in (X, E, L, Z)]
    fn(*[a.ctypes.data_as(dp) for a in args], out.ctypes.data_as(dp), *[j.ctypes.data_as(dp) for j in J])
    return out, [j.reshape(3, 6) for j in J]


def proj_T(O, X, E, L):
    out = np.zeros(12)
    import ctypes as C
    dp = C.POINTER(C.c_double)
    fn = O.lib().orc_project_to_camera3_transform
    fn.argtypes = [dp] * 7
    J = [np.zeros(36), np.zeros(36), np.zeros(36)]
    args = [np.ascontiguousarray(a, dtype=float) for a in (X, E, L)]
    fn(*[a.ctypes.data_as(dp) for a in args], out.ctypes.data_as(dp), *[j.ctypes.data_as(dp) for j in J])
    return out, [j.reshape(6, 6) for j in J]


def test_hybrid_motion_factor_jacobians(oracle):
    """HybridMotionTest.JacobianEvaluation: Z_k = perfect prediction, analytic == numeric (1e-5)."""
    Z, _ = proj_cam(oracle, X_k, E_k, L_e, m_L)
    kinds = ["pose", "pose", "point"]
    e, J = oracle.eval_factor(G.F_HYBRID_MOTION, [X_k, E_k, m_L], Z, L_e)
    assert np.abs(e[:3]).max() < 1e-15
    num = num_jac(oracle, G.F_HYBRID_MOTION, [X_k, E_k, m_L], kinds, Z, L_e)
    for a, b in zip(split_J(G.F_HYBRID_MOTION, J, kinds), num):
        assert a.shape == b.shape
        assert np.allclose(a, b, atol=1e-5)
        assert np.allclose(a, b, atol=1e-8)  # and much tighter than the reference asks


def test_compare_original_chains(oracle):
    """HybridMotionTest.CompareOriginal_* (1e-9): simplified chains equal the original kinematic chains."""
    X, E, L = Y.from12(X_k), Y.from12(E_k), Y.from12(L_e)
    Z = np.array([-0.5, 1.2, 3.0])
    # Original::projectToObject3 (HybridFormulationFactors.cc:42-46 comment)
    k_H_s0_k = Y.inverse(Y.compose(Y.compose(Y.inverse(L), E), L))
    L_k = Y.compose(E, L)
    k_H_s0_W = Y.compose(Y.compose(L_k, k_H_s0_k), Y.inverse(L_k))
    orig = Y.act(Y.inverse(L), Y.act(k_H_s0_W, Y.act(X, Z)))
    new, _ = proj_obj(oracle, X_k, E_k, L_e, Z)
    assert np.allclose(orig, new, atol=1e-9)
    # projectToCamera3Transform = X^-1 E L
    T_orig = Y.to12(Y.compose(Y.compose(Y.inverse(X), E), L))
    T_new, _ = proj_T(oracle, X_k, E_k, L_e)
    assert np.allclose(T_orig, T_new, atol=1e-9)
    p_new, _ = proj_cam(oracle, X_k, E_k, L_e, m_L)
    assert np.allclose(Y.act(Y.from12(T_orig), m_L), p_new, atol=1e-9)


def test_projection_roundtrip(oracle):
    """HybridObjectMotion.testProjections: projectToObject3 inverts projectToCamera3."""
    rng = np.random.default_rng(21)
    for _ in range(5):
        E = retract12(oracle, pose12(np.eye(3), [0, 0, 0]), rng.normal(0, 0.5, 6))
        X = retract12(oracle, pose12(np.eye(3), [0, 0, 0]), rng.normal(0, 0.5, 6))
        L0 = retract12(oracle, pose12(np.eye(3), [0, 0, 0]), rng.normal(0, 0.5, 6))
        m = rng.normal(0, 1.5, 3)
        m_cam, _ = proj_cam(oracle, X, E, L0, m)
        m_obj, _ = proj_obj(oracle, X, E, L0, m_cam)
        m_cam2, _ = proj_cam(oracle, X, E, L0, m_obj)
        assert np.allclose(m_obj, m, atol=1e-9) and np.allclose(m_cam2, m_cam, atol=1e-9)


def _num_fn(O, fn, args, kinds, out_is_pose=False, delta=1e-5):
    base = fn(*args)
    res = []
    for v, kind in enumerate(kinds):
        w = 6 if kind == "pose" else 3
        Jv = np.zeros((6 if out_is_pose else 3, w))
        for j in range(w):
            vals = []
            for sgn in (1, -1):
                dx = np.zeros(w)
                dx[j] = sgn * delta
                a = [np.array(x, float) for x in args]
                a[v] = retract12(O, a[v], dx) if kind == "pose" else a[v] + dx
                y = fn(*a)
                vals.append(O.call_pose("orc_pose_local", base, y, out_len=6) if out_is_pose else y - base)
            Jv[:, j] = (vals[0] - vals[1]) / (2 * delta)
        res.append(Jv)
    return res


def test_helper_jacobians(oracle):
    """ProjectToObject3_Jacobians / ProjectToCamera3Transform_Jacobians / ProjectToCamera3_Jacobians (1e-5)."""
    Z, _ = proj_cam(oracle, X_k, E_k, L_e, m_L)
    _, Jo = proj_obj(oracle, X_k, E_k, L_e, Z)
    num = _num_fn(oracle, lambda x, e, l, z: proj_obj(oracle, x, e, l, z)[0], [X_k, E_k, L_e, Z], ["pose", "pose", "pose"])
    for a, b in zip(Jo, num):
        assert np.allclose(a, b, atol=1e-5)
    _, Jt = proj_T(oracle, X_k, E_k, L_e)
    num = _num_fn(oracle, lambda x, e, l: proj_T(oracle, x, e, l)[0], [X_k, E_k, L_e], ["pose", "pose", "pose"], out_is_pose=True)
    for a, b in zip(Jt, num):
        assert np.allclose(a, b, atol=1e-5)
    _, Jc = proj_cam(oracle, X_k, E_k, L_e, m_L)
    num = _num_fn(oracle, lambda x, e, l, m: proj_cam(oracle, x, e, l, m)[0], [X_k, E_k, L_e, m_L], ["pose", "pose", "pose", "point"])
    for a, b in zip(Jc, num):
        assert np.allclose(a, b, atol=1e-5)


# ---- GTSAM-owned factors: not tested by the reference (parity unpinned) → self-check analytic vs numeric
@pytest.mark.parametrize("ftype,kinds", [
    (G.F_POSE_TO_POINT, ["pose", "point"]),
    (G.F_STEREO_POINT, ["pose", "point"]),
    (G.F_BETWEEN_POSE3, ["pose", "pose"]),
])
def test_gtsam_factor_jacobians(oracle, ftype, kinds):
    rng = np.random.default_rng(5)
    X = retract12(oracle, X_k, rng.normal(0, 0.2, 6))
    if ftype == G.F_BETWEEN_POSE3:
        X2 = retract12(oracle, X, np.array([0.01, -0.02, 0.015, 0.1, 0.2, -0.1]))
        meas = retract12(oracle, pose12(np.eye(3), [0, 0, 0]), np.array([0.01, -0.02, 0.015, 0.1, 0.2, -0.1]))  # zero error
        states, consts = [X, X2], None
    else:
        R, t = Y.from12(X)
        l = R @ np.array([0.3, -0.2, 6.0]) + t
        states = [X, l]
        consts = np.array([1000, 1000, 0, 320, 240, 0.5]) if ftype == G.F_STEREO_POINT else None
        meas = np.array([350.0, 270.0, 205.0]) if ftype == G.F_STEREO_POINT else np.array([0.31, -0.22, 6.1])
    _, J = oracle.eval_factor(ftype, states, meas, consts)
    num = num_jac(oracle, ftype, states, kinds, meas, consts, delta=1e-6)
    for v, (a, b) in enumerate(zip(split_J(ftype, J, kinds), num)):
        if ftype == G.F_BETWEEN_POSE3:
            # GTSAM's BetweenFactor omits the Logmap derivative (no GTSAM_SLOW_BUT_CORRECT_BETWEENFACTOR):
            # exact only at zero error, which is where this fixture sits
            assert np.allclose(a, b, atol=1e-6)
        else:
            assert np.allclose(a, b, atol=1e-6 * max(1.0, np.abs(b).max()))


def test_prior_factor(oracle):
    P = X_k
    X = retract12(oracle, P, np.array([1e-3, -2e-3, 1.5e-3, 0.01, 0.02, -0.01]))
    e, J = oracle.eval_factor(G.F_PRIOR_POSE3, [X], P)
    assert np.allclose(e, [1e-3, -2e-3, 1.5e-3, 0.01, 0.02, -0.01], atol=1e-12)
    assert np.array_equal(J[:6, :6], np.eye(6))


def test_stereo_cheirality(oracle):
    X = pose12(np.eye(3), [0, 0, 0])
    e, J = oracle.eval_factor(G.F_STEREO_POINT, [X, np.array([0.1, 0.2, -1.0])], np.array([1.0, 2.0, 3.0]),
                              np.array([1000, 900, 0, 320, 240, 0.5]))
    assert np.array_equal(e[:3], [2000.0] * 3) and not J.any()


def test_smoothing_zero_at_constant_motion(oracle):
    M = retract12(oracle, pose12(np.eye(3), [0, 0, 0]), np.array([0.01, 0.02, -0.015, 0.2, 0.1, 0.05]))
    L0 = L_e
    Ls = [L0]
    for _ in range(2):
        Ls.append(oracle.call_pose("orc_pose_compose", Ls[-1], M))  # body-frame constant motion
    Linv = oracle.call_pose("orc_pose_inverse", L0)
    Hs = [oracle.call_pose("orc_pose_compose", L, Linv) for L in Ls]
    e, J = oracle.eval_factor(G.F_HYBRID_SMOOTHING, Hs, None, L0)
    assert np.abs(e).max() < 1e-12
    num = num_jac(oracle, G.F_HYBRID_SMOOTHING, Hs, ["pose"] * 3, None, L0)
    for a, b in zip(split_J(G.F_HYBRID_SMOOTHING, J, ["pose"] * 3), num):
        assert np.allclose(a, b, atol=1e-12)  # the factor's Jacobian IS the central difference


def test_expmap_logmap_roundtrip(oracle):
    rng = np.random.default_rng(0)
    # pi - 1e-5 is inside SO3::Logmap's near-pi branch (pi - theta < 0.0316), whose first-order formula is good to ~5e-11 there
    for s in (1e-12, 1e-6, 1e-2, 1.0, 3.0, np.pi - 1e-5):
        xi = rng.normal(0, 1, 6)
        xi[:3] *= s / np.linalg.norm(xi[:3])
        T = oracle.call_pose("orc_pose_expmap", xi)
        back = oracle.call_pose("orc_pose_logmap", T, out_len=6)
        assert np.allclose(back, xi, atol=1e-9), (s, back, xi)
        R = T[:9].reshape(3, 3)
        assert np.allclose(R @ R.T, np.eye(3), atol=1e-12)
    # numpy twin used by the generator agrees with the C oracle
    xi = np.array([0.3, -0.2, 0.1, 1.0, 2.0, -0.5])
    assert np.allclose(Y.to12(Y.se3_exp(xi)), oracle.call_pose("orc_pose_expmap", xi), atol=1e-14)
    assert np.allclose(Y.se3_log(*Y.se3_exp(xi)), xi, atol=1e-12)


def test_noise_models(oracle):
    import ctypes as C
    dp = C.POINTER(C.c_double)
    fn = oracle.lib().orc_whiten
    fn.argtypes = [C.c_int, dp, C.c_double, dp, dp, dp, dp]

    def whiten(d, noise, hk, e):
        we, w, l = np.zeros(6), C.c_double(), C.c_double()
        n, ee = np.ascontiguousarray(noise, float), np.ascontiguousarray(e, float)
        fn(d, n.ctypes.data_as(dp), hk, ee.ctypes.data_as(dp), we.ctypes.data_as(dp), C.byref(w), C.byref(l))
        return we[:d], w.value, l.value

    e = np.array([0.3, -0.4, 1.2])
    # Isotropic sigma 0.1: whitened = e/0.1, loss = 0.5 * |.|^2
    we, w, l = whiten(3, np.diag([10.0] * 3).reshape(-1), 0.0, e)
    assert np.allclose(we, e * 10) and w == 1.0 and np.isclose(l, 0.5 * 100 * e @ e)
    # Huber k: inside -> quadratic; outside -> k(|r| - k/2), weights k/|r|, blocks scaled by sqrt(w)
    r = np.linalg.norm(e * 10)
    we, w, l = whiten(3, np.diag([10.0] * 3).reshape(-1), 1e-4, e)
    assert np.isclose(w, 1e-4 / r) and np.isclose(l, 1e-4 * (r - 0.5e-4)) and np.allclose(we, e * 10 * np.sqrt(w))
    we, w, l = whiten(3, np.diag([10.0] * 3).reshape(-1), 100.0, e)
    assert w == 1.0 and np.isclose(l, 0.5 * r * r)
    # Diagonal sigmas on a 6-vector
    e6 = np.arange(1, 7) * 0.1
    sg = np.array([0.01] * 3 + [0.1] * 3)
    we, w, l = whiten(6, sg, 0.0, e6)
    assert np.allclose(we, e6 / sg) and np.isclose(l, 0.5 * np.sum((e6 / sg) ** 2))


# ---- key encoding ------------------------------------------------------------------------------
def test_cantor_and_symbols(oracle):
    L = oracle.lib()
    import ctypes as C
    for x, y in [(15, 79), (46528, 1), (46528, 0)]:
        z = S.cantor_pair(x, y)
        assert z == L.orc_cantor_pair(x, y)
        assert S.cantor_depair(z) == (x, y)
        a, b = C.c_uint64(), C.c_uint64()
        L.orc_cantor_depair(z, C.byref(a), C.byref(b))
        assert (a.value, b.value) == (x, y)
    k = S.DynamicLandmarkSymbol(79, 15)           # DynamicPointSymbol('m', 15, 79)
    assert S.symbol_chr(k) == ord("m") and S.cantor_depair(S.symbol_index(k)) == (15, 79)
    assert k == L.orc_symbol(ord("m"), S.cantor_pair(15, 79))
    k = S.DynamicLandmarkSymbol(0, 46528)         # special case of the reference
    assert S.cantor_depair(S.symbol_index(k)) == (46528, 0)
    ok, obj, fr = S.reconstructMotionInfo(S.ObjectMotionSymbol(12, 10))
    assert ok and obj == 12 and fr == 10
    assert S.ObjectMotionSymbol(12, 10) == L.orc_labeled_symbol(ord("H"), 12 + ord("0"), 10)
    ok, obj, fr = S.reconstructPoseInfo(S.ObjectPoseSymbol(12, 12))
    assert ok and obj == 12 and fr == 12
    assert not S.reconstructMotionInfo(S.CameraPoseSymbol(10))[0]
    assert not S.reconstructMotionInfo(S.ObjectPoseSymbol(10, 12))[0]
    assert S.DynoChrExtractor(S.ObjectMotionSymbol(12, 10)) == ord("H")
    assert S.DynoChrExtractor(S.CameraPoseSymbol(2)) == ord("X")
    assert S.DynoChrExtractor(S.DynamicLandmarkSymbol(2, 10)) == ord("m")
    assert S.DynoChrExtractor(S.StaticLandmarkSymbol(2)) == ord("l")
    with pytest.raises(ValueError):
        S.DynamicLandmarkSymbol(0, -1)
