"""oracle/ransac_oracle.py (the fp64 restatement the device is bit-identical to) held to tests/epipolar_reference.py (50 digits):
solve4, seven_point and cubic_roots on every case the device test runs, the regimes of the cubic, and a search over 1e5 seven-point
samples for inputs that reach the regime in which the bisection of rf_cubic_roots used to stop early.  CPU only.

Tolerances.  Models: MARGIN_H / MARGIN_F x the model's own sensitivity (epipolar_reference.py).  A root t of a cubic:
8 x its eps-conditioning.  Bisection ends with two adjacent doubles around a sign change of the COMPUTED P; Horner's rule in fp64
gives P to within gamma_6 sum |c_i t^i| (Higham, Accuracy and Stability, eq. 5.3 with n = 3: 2n = 6 roundings), so the sign change lies within
6 u sum|c_i t^i| / |P'(t)| of t, and the midpoint of adjacent doubles within |t| 2^-52 = 2 x (|t| 2^-53): 6 + 2 = 8."""
import mpmath as mp
import numpy as np
import pytest

from oracle import ransac_oracle as RO
from tests import epipolar_cases as EC
from tests import epipolar_reference as ER
from tests.test_ransac_oracle import planted, planted_stereo

ROOT_TOL = 8


# ---- the margin ----
def measure_ratios(n_hyp=96):
    """largest (error / sensitivity) of the oracle's models over the first n_hyp hypotheses of the well-conditioned planted cases"""
    a, b, _o, _H = planted(200, 40, 0)
    rh = []
    for h in range(n_hyp):
        idx = RO.sample(h, len(a))
        if RO._degenerate(a[idx], b[idx]):
            continue
        rh.append(ER.homography_ratio(EC.ref_homography(a, b, h), RO.solve4(a[idx], b[idx])))
    rf, counts = {}, {}
    for name, (l, r) in dict(planted_stereo=planted_stereo()[:2], general_motion=EC.general_motion()[:2], equal_rows=EC.equal_rows()[:2]).items():
        rs, cnt = [], [0, 0, 0, 0]
        for h in range(n_hyp):
            idx = RO.sample7(h, len(l))
            Fs, sols = RO.seven_point(l[idx], r[idx]), EC.ref_fundamental(l, r, h)
            assert len(Fs) == len(sols), (name, h)
            cnt[len(sols)] += 1
            rs += [min(ER.fundamental_ratio(s, F) for s in sols) for F in Fs]
        rf[name], counts[name] = rs, cnt
    return dict(homography=rh, fundamental=rf, solutions=counts)


def test_margin_is_sixteen_times_the_oracles_measured_ratio():
    m = measure_ratios()
    worst_h, worst_f = max(m["homography"]), max(max(v) for v in m["fundamental"].values())
    print(f"homography: {len(m['homography'])} models, worst ratio {worst_h:.4g}; fundamental: "
          f"{sum(len(v) for v in m['fundamental'].values())} models, worst ratio {worst_f:.4g}; solutions {m['solutions']}")
    assert worst_h <= ER.MEASURED_H and worst_f <= ER.MEASURED_F           # what profiles/epipolar_reference.txt records
    assert ER.MARGIN_H == 16 * ER.MEASURED_H and ER.MARGIN_F == 16 * ER.MEASURED_F
    assert worst_h > ER.MEASURED_H / 1.01 and worst_f > ER.MEASURED_F / 1.01   # ... and not a looser number


# ---- every case of the device test, with the oracle in the device's place ----
H_CASES, F_CASES = EC.homography_cases(), EC.fundamental_cases()


@pytest.mark.parametrize("name", list(H_CASES))
def test_oracle_homography_cases(name):
    a, b, thr, K, cap = H_CASES[name]
    K = K or 512
    mask, best, H, sc, md = RO.verify_homography(a, b, thr, K, True, True)
    assert best == EC.first_best(sc) and (best < 0 or (mask.sum() == sc[best] and np.array_equal(md[best], H)))
    r = EC.check_homography(a, b, thr, K, best, mask, sc, md, cap)
    print(name, r)


@pytest.mark.parametrize("name", list(F_CASES))
def test_oracle_fundamental_cases(name):
    l, r, st, thr, K, cap = F_CASES[name]
    K = K or 512
    o = RO.stereo_track(l, r, st, EC.FX, EC.BASELINE, thr, K, True, True)
    g = st != 0
    assert o["ok"] == 1 and o["best"] == EC.first_best(o["scores"]) and o["n_inliers"] == o["scores"][o["best"]]
    res = EC.check_fundamental(l[g], r[g], thr, K, o["best"], o["code"][g] != 2, o["scores"], o["models"], cap)
    print(name, {k: v for k, v in res.items() if k != "solutions"}, np.bincount(res["solutions"], minlength=4).tolist())
    if name == "thr1":      # samples with one and with three real solutions both occur, 20 times at least
        n = np.bincount(res["solutions"], minlength=4)
        assert n[1] >= 20 and n[3] >= 20 and n[2] == 0


def test_equal_rows_succeed_and_constant_disparity_has_no_model():
    l, r, out = EC.equal_rows()
    o = RO.stereo_track(l, r, np.ones(len(l), np.uint8), EC.FX, EC.BASELINE)
    assert o["ok"] == 1 and (o["code"][out] == 2).all() and o["n_inliers"] == len(l) - len(out)
    l, r = EC.constant_disparity()
    o = RO.stereo_track(l, r, np.ones(len(l), np.uint8), EC.FX, EC.BASELINE, scores=True, models=True)
    assert o["ok"] == 1 and (o["code"] == 2).all() and not o["F"].any() and not o["scores"].any() and o["best"] == -1
    for h in range(12):      # the reference agrees: the 7x9 matrix of every sample has rank below 7
        assert EC.ref_fundamental(l, r, h) == []


@pytest.mark.parametrize("kind", ["H", "F"])
def test_nonfinite_correspondences_are_never_inliers(kind):
    a, b = EC.nonfinite(kind)
    if kind == "H":
        mask, best, M, sc, md = RO.verify_homography(a, b, 5.0, 512, True, True)
    else:
        mask, best, M, sc, md = RO.find_fundamental(a, b, 1.0, 512, True, True)
    assert best >= 0 and best == EC.first_best(sc) and np.isfinite(M).all() and not mask[17] and not mask[101] and mask.sum() == sc[best] > 100
    assert np.isfinite(md[sc > 0]).all()


def test_ties_go_to_the_lowest_index_beyond_the_first_stride():
    a, b, thr, K, _cap = H_CASES["line_plus_three"]
    _m, best, _H, sc = RO.verify_homography(a, b, thr, K, scores=True)
    top = np.nonzero(sc == sc.max())[0]
    assert sc.max() == len(a) and len(top) >= 4 and top[0] > 255 and (top < 512).sum() >= 2 and best == top[0]     # the precondition
    assert np.count_nonzero(sc) == len(top)


# ---- the cubic ----
def _poly(roots):
    """fp64 coefficients (c0..c3) of prod (t - r), rounded from the exact product"""
    with mp.workdps(60):
        c = [mp.mpf(1)]
        for r in roots:
            c = [(c[i - 1] if i else 0) - mp.mpf(r) * (c[i] if i < len(c) else 0) for i in range(len(c) + 1)]
        return tuple(float(v) for v in c)     # c[i] multiplies t^i


def cubic_set():
    """name -> (c0, c1, c2, c3)"""
    rng = np.random.default_rng(5)
    s = {}
    for k in range(24):
        s[f"three{k}"] = _poly(np.sort(rng.uniform(-5, 5, 3)) + np.array([-1.0, 0.0, 1.0]))
    for k in range(12):
        p, q, r = rng.uniform(-3, 3), rng.uniform(-2, 2), rng.uniform(0.3, 3)
        s[f"one{k}"] = tuple(np.polymul([1.0, -2 * q, q * q + r * r], [1.0, -p])[::-1])     # (t - p)((t - q)^2 + r^2)
    s["wide0"] = _poly([1e-3, 7.0, 1e5]); s["wide1"] = _poly([-1e5, 2e-3, 3.0]); s["wide2"] = _poly([-4e-3, -50.0, 9e4])
    s["double0"] = _poly([1.0, 1.001, 4.0]); s["double1"] = _poly([-2.0, 0.5, 0.5002]); s["double2"] = _poly([-3.0003, -3.0, 8.0])
    s["critical0"] = (2.0, -3.0, 0.0, 1.0)            # (t - 1)^2 (t + 2): the root 1 is a critical point and P(1) = 0 exactly
    s["critical1"] = (-4.0, 0.0, 3.0, 1.0)            # (t + 2)^2 (t - 1)
    A = 2.0 ** 60
    s["atR+"] = (-A, 1.0, -A, 1.0)                    # (t - A)(t^2 + 1): R = 1 + A rounds to A, P(R) = 0
    s["atR-"] = (A, 1.0, A, 1.0)
    for e in (14, 17, 20, 25, 30):
        s[f"c3small{e}"] = (-2.0, 1.0, 3.0, 10.0 ** -e)
        s[f"c3small{e}n"] = (1.0, -4.0, 3.0, -(10.0 ** -e))
    return s


REGIMES = ("three", "one", "wide", "double", "critical", "atR", "c3small")


def regimes_of(c):
    """the regimes a cubic belongs to, judged by the reference alone"""
    c0, c1, c2, c3 = c
    ref = ER.cubic_roots(*c)
    t = [float(r) for r, _ in ref]
    out = set()
    R = 1.0 + max(abs(c0 / c3), abs(c1 / c3), abs(c2 / c3))
    if len(t) == 3 and min(t[1] - t[0], t[2] - t[1]) > 1e-2 * max(1.0, max(abs(v) for v in t)):
        out.add("three")
    if len(t) == 1:
        out.add("one")
    if len(t) == 3 and min(abs(v) for v in t) <= 1e-2 and max(abs(v) for v in t) >= 1e4 and max(abs(v) for v in t) <= 1e6:
        out.add("wide")
    if len(t) == 3 and 0 < min(t[1] - t[0], t[2] - t[1]) <= 1.001e-3 * max(1.0, max(abs(v) for v in t)):
        out.add("double")
    if any(not mp.isfinite(cond) for _, cond in ref):
        out.add("critical")
    if any(abs(v) == R for v in t):
        out.add("atR")
    if abs(c3) <= 1e-14 * max(abs(c0), abs(c1), abs(c2)):
        out.add("c3small")
    return out


def cubic_errors(c):
    """[(reference root, |oracle - reference| / (ROOT_TOL x conditioning), well separated)] and the two root counts"""
    ref, got = ER.cubic_roots(*c), RO.cubic_roots(*c)
    rows = []
    with mp.workdps(ER.DPS):
        for k, (t, cond) in enumerate(ref):
            tol = ROOT_TOL * cond
            others = [abs(t - u) for j, (u, _) in enumerate(ref) if j != k]
            sep = mp.isfinite(cond) and all(d > 1000 * tol for d in others)
            err = min((abs(mp.mpf(g) - t) for g in got), default=mp.inf)
            rows.append((float(t), float(err / tol) if mp.isfinite(cond) else float("nan"), bool(sep)))
    return rows, len(ref), len(got)


CUBICS = cubic_set()


def test_every_cubic_regime_occurs():
    seen = set()
    for c in CUBICS.values():
        seen |= regimes_of(c)
    assert seen == set(REGIMES), set(REGIMES) - seen


@pytest.mark.parametrize("name", list(CUBICS))
def test_cubic_roots_against_the_reference(name):
    c = CUBICS[name]
    rows, n_ref, n_got = cubic_errors(c)
    print(name, c, rows, n_ref, n_got)
    if all(sep for _t, _e, sep in rows):
        assert n_got == n_ref
    for t, e, sep in rows:
        if sep:
            assert e <= 1.0, f"{name}: root {t!r} is {e:.4g} tolerances from the reference"
    if name.startswith("critical"):
        dbl = 1.0 if name == "critical0" else -2.0
        assert dbl in RO.cubic_roots(*c)                                  # P(critical point) = 0 exactly: returned as it is
    if name.startswith("atR"):
        assert RO.cubic_roots(*c) == [2.0 ** 60 if name == "atR+" else -(2.0 ** 60)]


def test_random_cubics_with_separated_roots():
    rng = np.random.default_rng(11)
    worst = 0.0
    for _ in range(150):
        mags = 10.0 ** rng.uniform(-3, 4, 3) * rng.choice([-1, 1], 3)
        c = _poly(np.sort(mags))
        rows, n_ref, n_got = cubic_errors(c)
        if all(sep for _t, _e, sep in rows):
            assert n_got == n_ref, c
        for t, e, sep in rows:
            if sep:
                assert e <= 1.0, (c, t, e)
                worst = max(worst, e)
    print("worst root error / tolerance:", worst)


def test_eighty_halvings_miss_the_small_c3_cubics(monkeypatch):
    """the defect this test file was written against: with the bisection stopped after 80 steps (as it was) the c3-small cubics are
    outside the tolerance, so the tolerance is one that sees it"""
    monkeypatch.setattr(RO, "REFINE", False)
    bad = [n for n, c in CUBICS.items() if n.startswith("c3small") and any(sep and e > 1.0 for _t, e, sep in cubic_errors(c)[0])]
    assert len(bad) == sum(n.startswith("c3small") for n in CUBICS), bad
    ok = [n for n, c in CUBICS.items() if not n.startswith("c3small") and all(e <= 1.0 for _t, e, sep in cubic_errors(c)[0] if sep)]
    assert len(ok) == sum(not n.startswith("c3small") for n in CUBICS)


def test_converged_brackets_keep_their_bits(monkeypatch):
    """where 80 halvings had converged nothing changes: the planted cases give the same bits as before, every hypothesis of them.
    Exactly equal rows are where they had not: a solution at t = 0, found as 5e-24 by 80 halvings from R ~ 10 - the same winner, mask
    and scores, models that differ far below the last bit of a unit F"""
    now = {}
    for name in ("thr1", "general_motion", "planar", "ties", "negative_subpixel", "equal_rows"):
        l, r, _st, thr, _K, _cap = F_CASES[name]
        now[name] = RO.find_fundamental(l, r, thr, 512, True, True)
    monkeypatch.setattr(RO, "REFINE", False)
    for name, new in now.items():
        l, r, _st, thr, _K, _cap = F_CASES[name]
        old = RO.find_fundamental(l, r, thr, 512, True, True)
        if name != "equal_rows":
            assert old[1] == new[1] and all(np.array_equal(p, q) for p, q in zip(old, new)), name
            continue
        assert old[1] == new[1] and np.array_equal(old[0], new[0]) and np.array_equal(old[3], new[3])
        differ = np.nonzero((old[4] != new[4]).any(1))[0]
        assert len(differ) >= 100
        unit = lambda m: m / np.linalg.norm(m, axis=1, keepdims=True)      # noqa: E731
        assert np.abs(unit(old[4][differ]) - unit(new[4][differ])).max() < 2.0 ** -56        # (an eighth of the last bit of an entry near 1)


# ---- the search: can seven float32 correspondences reach R / |t| >= 2^26 ? ----
def cubic_batch(a, b):
    """RO.seven_point_cubic over a batch ([B, 7, 2] float32 each): the same operations in the same order, vectorised.
    returns (ok [B], c [B, 4])"""
    x1, y1, x2, y2 = (v.astype(np.float64) for v in (a[..., 0], a[..., 1], b[..., 0], b[..., 1]))
    M = np.stack([x2 * x1, x2 * y1, x2, y2 * x1, y2 * y1, y2, x1, y1, np.ones_like(x1)], -1)
    B = len(M); ar = np.arange(B)
    perm = np.tile(np.arange(9), (B, 1))
    ok = np.ones(B, bool)
    with np.errstate(all="ignore"):
        for k in range(7):
            sub = np.abs(M[:, k:, k:]).reshape(B, -1)
            idx = np.argmax(sub, 1)
            ok &= sub[ar, idx] > 1e-9
            pr, pc = k + idx // (9 - k), k + idx % (9 - k)
            rk, rp = M[ar, k].copy(), M[ar, pr].copy()
            M[ar, k], M[ar, pr] = rp, rk
            ck, cp = M[ar, :, k].copy(), M[ar, :, pc].copy()
            M[ar, :, k], M[ar, :, pc] = cp, ck
            pk, pp = perm[ar, k].copy(), perm[ar, pc].copy()
            perm[ar, k], perm[ar, pc] = pp, pk
            M[:, k, k:] = M[:, k, k:] / M[:, k, k][:, None]
            f = M[:, :, k].copy(); f[:, k] = 0.0
            keep = M[:, k, k:].copy()
            M[:, :, k:] = M[:, :, k:] - f[:, :, None] * keep[:, None, :]
            M[:, k, k:] = keep
        f1, f2 = np.zeros((B, 9)), np.zeros((B, 9))
        for k in range(7):
            f1[ar, perm[:, k]] = -M[:, k, 7]; f2[ar, perm[:, k]] = -M[:, k, 8]
        f1[ar, perm[:, 7]], f1[ar, perm[:, 8]], f2[ar, perm[:, 7]], f2[ar, perm[:, 8]] = 1.0, 0.0, 0.0, 1.0

        def det3(m):
            return (m[:, 0] * (m[:, 4] * m[:, 8] - m[:, 5] * m[:, 7]) - m[:, 1] * (m[:, 3] * m[:, 8] - m[:, 5] * m[:, 6])
                    + m[:, 2] * (m[:, 3] * m[:, 7] - m[:, 4] * m[:, 6]))
        c0, c3, c1, c2 = det3(f1), det3(f2), np.zeros(B), np.zeros(B)
        for r in range(3):
            t = f1.copy(); t[:, 3 * r:3 * r + 3] = f2[:, 3 * r:3 * r + 3]; c1 = c1 + det3(t)
            t = f2.copy(); t[:, 3 * r:3 * r + 3] = f1[:, 3 * r:3 * r + 3]; c2 = c2 + det3(t)
    return ok, np.stack([c0, c1, c2, c3], 1)


def search_scenes():
    """(kind, left, right): the four scene kinds - rectified with 0 .. 0.15 px row noise (near-rectified pairs), exactly equal rows,
    general motion, a plane - and each again with one noise-free correspondence moved to the origin of both images: then F33 = 0, the
    true solution has no component along one of the two free columns, which puts it at t = 0 or along f2 (t = infinity)"""
    out = []
    for seed in range(3):
        for noise in (0.0, 3e-5, 1e-3, 0.15):
            l, r, _ = EC.stereo_scene(160, 0, 300 + seed, noise)
            out.append((f"rectified {noise}", l, r))
        out.append(("equal rows", *EC.equal_rows(160, 0, 310 + seed)[:2]))
        out.append(("general motion", *EC.general_motion(160, 0, 320 + seed)[:2]))
        out.append(("planar", *EC.general_motion(160, 0, 330 + seed, planar=True)[:2]))
        for kind, (l, r) in (("equal rows, origin", EC.equal_rows(160, 0, 340 + seed)[:2]), ("general motion, origin", EC.general_motion(160, 0, 350 + seed, noise=0.0)[:2]),
                             ("rectified 0.001, origin", EC.stereo_scene(160, 0, 360 + seed, 1e-3)[:2])):
            out.append((kind, l - l[0], r - r[0]))
    return out


def search(per_scene=3400, seed=0):
    """over len(search_scenes()) x per_scene random seven-point samples: per scene kind the largest R / |t| over the real roots;
    the 40 samples with the largest ratio and 40 at random are held to the 50-digit reference.
    returns dict(samples, by_kind, worst_ratio, checked, worst_model_ratio, outside)"""
    rng = np.random.default_rng(seed)
    by_kind, pool, total = {}, [], 0
    for kind, l, r in search_scenes():
        idx = np.argsort(rng.random((per_scene, len(l))), 1)[:, :7]
        ok, c = cubic_batch(l[idx], r[idx])
        with np.errstate(all="ignore"):
            ok &= np.abs(c[:, 3]) > 1e-300
            c, idx = c[ok], idx[ok]
            R = 1.0 + np.abs(c[:, :3] / c[:, 3:]).max(1)
            comp = np.zeros((len(c), 3, 3)); comp[:, 1, 0] = comp[:, 2, 1] = 1.0
            comp[:, :, 2] = -c[:, :3] / c[:, 3:]
            fin = np.isfinite(comp).all((1, 2))
            ev = np.full((len(c), 3), np.nan, complex); ev[fin] = np.linalg.eigvals(comp[fin])
            real = np.abs(ev.imag) <= 1e-6 * np.abs(ev)
            ratio = np.where(real, R[:, None] / np.abs(ev), 0.0)
            ratio = np.nan_to_num(ratio, nan=0.0).max(1)
        total += len(c)
        k = by_kind.setdefault(kind, dict(samples=0, worst=0.0))
        k["samples"] += len(c); k["worst"] = max(k["worst"], float(ratio.max()))
        top = np.argsort(-ratio)[:4]
        pool += [(float(ratio[j]), kind, l[idx[j]], r[idx[j]]) for j in set(top.tolist()) | set(rng.choice(len(c), 4, replace=False).tolist())]
    pool.sort(key=lambda p: -p[0])
    checked = pool[:40] + [pool[j] for j in rng.choice(np.arange(40, len(pool)), 40, replace=False)]
    worst, outside = 0.0, []
    for ratio, kind, a, b in checked:
        sols = ER.seven_point(a, b)
        Fs = RO.seven_point(a, b)
        for F in Fs:
            m = min((ER.fundamental_ratio(s, F) for s in sols), default=float("inf"))
            worst = max(worst, m)
            if m > ER.MARGIN_F:
                outside.append((kind, ratio, m))
        if len(Fs) != len(sols):
            outside.append((kind, ratio, f"{len(Fs)} models, reference {len(sols)}"))
    return dict(samples=total, by_kind=by_kind, worst_ratio=max(k["worst"] for k in by_kind.values()), checked=len(checked), worst_model_ratio=worst, outside=outside)


def test_the_batched_cubic_is_the_oracles():
    l, r, _o, _z = planted_stereo()
    idx = np.array([RO.sample7(h, len(l)) for h in range(64)])
    ok, c = cubic_batch(l[idx], r[idx])
    for h in range(64):
        ref = RO.seven_point_cubic(l[idx[h]], r[idx[h]])
        assert ok[h] == (ref is not None) and (ref is None or np.array_equal(c[h], np.array(ref[2:])))


def test_search_for_seven_point_samples_in_the_bad_regime():
    s = search()
    print(s)
    assert s["samples"] >= 100000 and len(s["by_kind"]) >= 8
    # what the search found is recorded in profiles/epipolar_reference.txt; what must hold is that the models of the samples it
    # singled out are inside the tolerance now (a sample outside it would be a device case of tests/test_gpu_epipolar_reference.py)
    assert not s["outside"], s["outside"]
