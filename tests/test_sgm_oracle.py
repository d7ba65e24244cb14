"""tests/sgm_oracle.py judged on its own (CPU): the recursion against a scalar triple loop, the subpixel floor against exact fractions,
the tie rules on a flat image, and the quality of the result against the known disparity of a rendered scene."""
import fractions
import functools

import numpy as np

from tests import sgm_oracle as O


@functools.lru_cache(maxsize=None)
def _rendered(seed=1):
    left, right, truth = O.render_pair(128, 64, 0, 32, seed)
    out = O.stereo_dense(left, right, 721.5377, 0.5371, num_disparities=32)
    return out, truth


def _brute_sums(C, p1, p2, paths):
    """S by the definition, one pixel and one disparity at a time"""
    H, W, D = C.shape
    S = np.zeros((H, W, D), np.int64)
    for dx, dy in O.DIRECTIONS[:paths]:
        L = np.zeros((H, W, D), np.int64)
        ys = range(H) if dy >= 0 else range(H - 1, -1, -1)
        xs = range(W) if dx >= 0 else range(W - 1, -1, -1)
        for y in ys:
            for x in xs:
                px, py = x - dx, y - dy
                for k in range(D):
                    if not (0 <= px < W and 0 <= py < H):
                        L[y, x, k] = C[y, x, k]
                        continue
                    prev = L[py, px]
                    m = min(int(v) for v in prev)
                    terms = [int(prev[k]), m + p2]
                    if k - 1 >= 0:
                        terms.append(int(prev[k - 1]) + p1)
                    if k + 1 < D:
                        terms.append(int(prev[k + 1]) + p1)
                    L[y, x, k] = int(C[y, x, k]) + min(terms) - m
        S += L
    return S


def test_sums_equal_the_scalar_recursion():
    """16 x 8, D = 8, both path counts: a plain-array case of the oracle (the 64 / 8 size rule is the context's, not the oracle's)"""
    rng = np.random.default_rng(5)
    gl, gr = rng.integers(0, 256, (8, 16)).astype(np.uint8), rng.integers(0, 256, (8, 16)).astype(np.uint8)
    C = O.cost_volume(O.census(gl), O.census(gr), 1, 8)
    assert C.max() == 64 and C.min() < 40 and (C[:, 0] == 64).all()
    for paths in (4, 8):
        assert np.array_equal(O.aggregate(C, 3, 20, paths), _brute_sums(C, 3, 20, paths))
    assert np.array_equal(O.stereo_dense_gray(gl, gr, min_disparity=1, num_disparities=8, p1=3, p2=20)["S"], _brute_sums(C, 3, 20, 8))


def test_census_is_the_window_comparison():
    rng = np.random.default_rng(6)
    g = rng.integers(0, 4, (9, 11)).astype(np.uint8)            # few levels: many equal neighbours, which do not count
    c = O.census(g)
    for (y, x) in ((0, 0), (4, 5), (8, 10), (0, 10), (3, 1)):
        n = sum(int(g[min(max(y + dy, 0), 8), min(max(x + dx, 0), 10)] < g[y, x]) for dy in range(-3, 4) for dx in range(-4, 5) if (dy, dx) != (0, 0))
        assert bin(int(c[y, x])).count("1") == n
    assert int(c.max()) < 1 << 62


def test_subpixel_offset_is_the_floor():
    """f = floor(((a - b) 16 + den) / (2 den)) on every pixel of a rendered pair, which holds pixels with a negative numerator"""
    out, _ = _rendered()
    a, b, s, f, inner = (out[k].ravel() for k in ("a", "b", "smin", "f", "inner"))
    assert inner.sum() > 0.9 * inner.size
    negative = truncation_differs = 0
    for i in np.flatnonzero(inner):
        den = max(int(a[i]) + int(b[i]) - 2 * int(s[i]), 1)
        num = (int(a[i]) - int(b[i])) * 16 + den
        q = fractions.Fraction(num, 2 * den)
        assert int(f[i]) == q.numerator // q.denominator            # Fraction's floor
        negative += num < 0
        truncation_differs += int(num / (2 * den)) != int(f[i])
    assert negative > 0.05 * inner.sum() and truncation_differs > 0
    assert (out["f"][~out["inner"]] == 0).all() and out["f"].min() >= -8 and out["f"].max() <= 8


def test_flat_image_takes_the_lowest_disparity():
    """every sum ties: k* = 0 at x >= dmin, code 3 left of it"""
    g = np.full((16, 64), 90, np.uint8)
    for dmin in (0, 5):
        out = O.stereo_dense_gray(g, g, 1.0, 1.0, min_disparity=dmin, num_disparities=32)
        assert (out["k"][:, dmin:] == 0).all() and (out["code"][:, :dmin] == 3).all()
        assert (out["disparity"][out["code"] != 0] == (dmin - 1) * 16).all() and (out["depth"][out["code"] != 0] == 0.0).all()
        assert (out["kr"][:, :64 - dmin] == 0).all()


def test_quality_against_the_rendered_truth():
    """render_pair(128, 64, 0, 32, seed = 1) with the default parameters, measured on this oracle:
        valid pixels within 1 px of the truth                 0.985   (floor 0.955)
        valid pixels among those with x >= true disparity     0.946   (floor 0.916)
    The floors are the measured values minus 0.03; the seed moves both at the 0.01 level."""
    out, truth = _rendered()
    valid = out["code"] == 0
    within = (np.abs(out["disparity"] / 16.0 - truth) <= 1.0)[valid].mean()
    visible = np.arange(128)[None, :] >= truth
    share = valid[visible].mean()
    print(f"within 1 px: {within:.4f}, valid among visible: {share:.4f}")
    assert within >= 0.955 and share >= 0.916
    assert out["n_valid"] + out["n_not_unique"] + out["n_lr"] + out["n_outside"] == truth.size


def test_depth_is_one_product_one_scaling_one_division():
    out, _ = _rendered()
    d, code = out["disparity"], out["code"]
    fb = np.float64(721.5377) * np.float64(0.5371)
    ok = (code == 0) & (d > 0)
    assert ok.any() and (~ok).any()
    assert np.array_equal(out["depth"][ok], fb / (d[ok].astype(np.float64) * 0.0625)) and (out["depth"][~ok] == 0.0).all()
    xy = np.array([[0.5, 0.5], [1.5, 2.5], [127.4, 62.5], [127.5, 3.0], [-0.5, 0.0], [-0.6, 0.0], [5.0, 64.0]], np.float32)
    depth, c = O.depth_at(out["depth"], code, xy)
    want = [(0, 0), (2, 2), (127, 62), None, (0, 0), None, None]      # round half to even; None: outside
    for i, w in enumerate(want):
        assert (depth[i], c[i]) == ((0.0, 3) if w is None else (out["depth"][w[1], w[0]], code[w[1], w[0]]))
