"""Image contents that the sum-of-sinusoids texture of dynosam_amd/synth_images.py never produces: exact ties, flat and saturated
regions, periodic patterns, step edges, low contrast, nothing at all.  Shared by tests/test_image_contents.py (CPU: the oracles alone
take the branches these contents are for) and tests/test_gpu_image_contents.py (the frontend kernels against the oracles).

    checker8    ((x//8 + y//8) & 1) * 255              massive exact ties, maximum contrast
    stripes16   ((x//8) & 1) * 255                     the aperture problem: the minimum eigenvalue is 0 everywhere
    steps       a random grey level per 32x24 block    flat interiors, step edges, plateaus in the 3x3 non-maximum test
    saturated   clip((base - 128) * 4 + 128, 0, 255)   large runs of 0 and 255
    noise       iid uniform uint8                      no spatial coherence
    half_flat   base, right half 255, the top third of the left half 0     flat regions beside texture
    dim4        120 + (base >> 2)                      contrast between ORB's two FAST thresholds (20 and 7)
    flat        90 everywhere                          nothing at all

base is the grey image of synth_images.make_pair(W, H, objects=1, seed=4)["rgb0"].  Frame 1 of a pair is frame 0 moved by np.roll, so
both frames hold the same multiset of pixels and every tie of frame 0 is a tie of frame 1."""
import functools

import numpy as np

from dynosam_amd import synth_images as SI
from oracle import klt_oracle as K

NAMES = ("checker8", "stripes16", "steps", "saturated", "noise", "half_flat", "dim4", "flat")


@functools.lru_cache(maxsize=None)
def _base(W, H):
    return K.gray_u8(SI.make_pair(W, H, objects=1, seed=4)["rgb0"]).astype(np.int32)


def textured(W, H):
    """the grey image the other contents are cut from (uint8): the ordinary texture of the other frontend modules"""
    return _base(W, H).astype(np.uint8)


def contents(W, H):
    """{name: [H, W] uint8 grey image}, in the order of NAMES"""
    ys, xs = np.mgrid[0:H, 0:W]
    base = _base(W, H)
    levels = np.random.default_rng(11).integers(0, 256, ((H + 23) // 24, (W + 31) // 32))
    half_flat = base.copy()
    half_flat[:, W // 2:] = 255
    half_flat[:H // 3, :W // 2] = 0
    out = dict(checker8=((xs // 8 + ys // 8) & 1) * 255,
               stripes16=((xs // 8) & 1) * 255,
               steps=levels[ys // 24, xs // 32],
               saturated=np.clip((base - 128) * 4 + 128, 0, 255),
               noise=np.random.default_rng(12).integers(0, 256, (H, W)),
               half_flat=half_flat,
               dim4=120 + (base >> 2),
               flat=np.full((H, W), 90))
    assert tuple(out) == NAMES and all(0 <= v.min() and v.max() <= 255 for v in out.values())
    return {k: np.ascontiguousarray(v, np.uint8) for k, v in out.items()}


def object_mask(W, H):
    """a motion mask with one object, a fixed rectangle (the contents carry no objects of their own)"""
    m = np.zeros((H, W), np.int32)
    m[H // 4:H // 2, W // 3:(2 * W) // 3] = 1
    return m


def rgb(g):
    """the grey image in three equal channels: klt_oracle.gray_u8 and flow_oracle.gray of it give g back exactly"""
    return np.ascontiguousarray(np.repeat(np.asarray(g, np.uint8)[..., None], 3, axis=-1))


def pair(g, dx=3, dy=-2):
    """(rgb0, rgb1): frame 0 is g, frame 1 is g moved by (dx, dy) pixels with wrap-around"""
    return rgb(g), rgb(np.roll(g, (dy, dx), axis=(0, 1)))


# ---------------------------------------------------------------- the oracles' answers, computed once per (content, size) and shared

R = 6                                  # search_radius_cells of the trackers the tests make
# the mask / parameter sets of test_gpu_frontend_sizes.test_gftt_identical_to_oracle: no mask with the defaults, then the detection mask with these
DETECT_SETS = (dict(max_corners=800, quality_level=0.001, min_distance=8.0), dict(max_corners=50, quality_level=0.05, min_distance=20.0),
               dict(max_corners=300, quality_level=0.01, min_distance=0.0))


def detection_mask(W, H):
    """the static tracker's detection mask: background only, discs of radius 8 around features already tracked, last row / column open"""
    mask = (object_mask(W, H) == 0).astype(np.uint8) * 255
    ys, xs = np.mgrid[0:H, 0:W]
    for (x, y) in ((W // 6, H // 5), (W // 2, H // 2), (W - 20, H - 12)):
        mask[(xs - x) ** 2 + (ys - y) ** 2 <= 64] = 0
    return mask


def klt_points(W, H, seed, n, lo=-30.0, hi=30.0):
    """test_gpu_frontend_sizes._klt_points: from |lo| px outside the image to hi px beyond the far edge (negative: inside)"""
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(lo, W + hi, n), rng.uniform(lo, H + hi, n)], -1).astype(np.float32)


def tie_counts(d0, d1, w, h, radius=R):
    """per coarse cell p: how many candidates of its window attain the float64 maximum of the score.  Every candidate's 64 products
    are summed in the same order, so equal rows give equal sums."""
    from oracle import flow_oracle as FO
    A, B = FO.bf16_to_f32(d0).astype(np.float64), FO.bf16_to_f32(d1).astype(np.float64)
    out = np.zeros(w * h, np.int64)
    for p in range(w * h):
        x, y = p % w, p // w
        xs, ys = np.arange(max(0, x - radius), min(w - 1, x + radius) + 1), np.arange(max(0, y - radius), min(h - 1, y + radius) + 1)
        c = (B[(ys[:, None] * w + xs[None, :]).ravel()] * A[p]).sum(1)
        out[p] = (c == c.max()).sum()
    return out


class Ref:
    """what the oracles say about one content at one size: each answer is computed on first use, kept, and handed out read-only"""

    def __init__(self, name, W, H):
        self.name, self.W, self.H = name, W, H
        self.rgb0, self.rgb1 = pair(contents(W, H)[name])
        self.g = (K.gray_u8(self.rgb0), K.gray_u8(self.rgb1))
        self._kept = {}

    def _once(self, key, make):
        if key not in self._kept:
            v = make()
            for a in (v if isinstance(v, (tuple, list)) else (v,)):
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
            self._kept[key] = v
        return self._kept[key]

    def pyramid(self, frame):
        from oracle import flow_oracle as FO
        return self._once(("pyr", frame), lambda: FO.pyramid((self.rgb0, self.rgb1)[frame]))

    def descriptors(self, frame):
        from oracle import flow_oracle as FO
        return self._once(("desc", frame), lambda: FO.descriptors(self.pyramid(frame)[3]))

    def argmax_f32(self):
        from oracle import flow_oracle as FO
        return self._once("f32", lambda: FO.corr_argmax(self.descriptors(0), self.descriptors(1), self.W // 8, self.H // 8, R)[0])

    def argmax_f64(self):
        from oracle import flow_oracle as FO
        return self._once("f64", lambda: FO.corr_argmax_f64(self.descriptors(0), self.descriptors(1), self.W // 8, self.H // 8, R))

    def ties(self):
        return self._once("ties", lambda: tie_counts(self.descriptors(0), self.descriptors(1), self.W // 8, self.H // 8))

    def dense_flow(self):
        from oracle import flow_oracle as FO
        return self._once("flow", lambda: FO.dense_flow(self.rgb0, self.rgb1, R=R))

    def klt(self, with_init):
        """(points, initial guesses or None, K.track_points' answer): 160 points from 30 px outside to 30 px inside, or 40 interior points
        with an initial guess 3 px off"""
        def make():
            pts = klt_points(self.W, self.H, 8, 40, lo=12.0, hi=-12.0) if with_init else klt_points(self.W, self.H, 7, 160)
            init = pts + np.float32(3.0) if with_init else None
            return (pts, init) + tuple(K.track_points(self.g[0], self.g[1], pts, init))
        return self._once(("klt", with_init), make)

    def clahe(self, frame):
        from oracle import clahe_oracle as CO
        return self._once(("clahe", frame), lambda: CO.clahe(self.g[frame]))

    def image(self, frame, use_clahe):
        return self.clahe(frame) if use_clahe else self.g[frame]

    def gftt(self, use_harris, use_clahe, which=None):
        """frame 0's corners: which None = no mask and the defaults, else DETECT_SETS[which] under detection_mask"""
        from oracle import gftt_oracle as G
        def make():
            if which is None:
                return G.good_features_to_track(self.image(0, use_clahe), use_harris=use_harris)[0]
            return G.good_features_to_track(self.image(0, use_clahe), detection_mask(self.W, self.H), use_harris=use_harris, **DETECT_SETS[which])[0]
        return self._once(("gftt", use_harris, use_clahe, which), make)

    def subpix_points(self, use_clahe):
        """the oracle's own corners of frame 1 (at most 300) plus 40 random interior points"""
        from oracle import gftt_oracle as G
        def make():
            c = G.good_features_to_track(self.image(1, use_clahe), max_corners=300)[0]
            rng = np.random.default_rng(5)
            extra = np.stack([rng.uniform(8, self.W - 8, 40), rng.uniform(8, self.H - 8, 40)], -1)
            return np.concatenate([c, extra]).astype(np.float32)
        return self._once(("subpix_pts", use_clahe), make)

    def subpix(self, use_clahe):
        from oracle import subpix_oracle as SO
        return self._once(("subpix", use_clahe), lambda: SO.corner_sub_pix(self.image(1, use_clahe), self.subpix_points(use_clahe)))

    def orb(self, n_levels, ini_th=20, min_th=7, frame=0):
        from oracle import orb_oracle as O
        return self._once(("orb", n_levels, ini_th, min_th, frame), lambda: O.detect(self.g[frame], O.OrbParams(2000, 1.2, n_levels, ini_th, min_th)))


@functools.lru_cache(maxsize=None)
def ref(name, W=192, H=136):
    return Ref(name, W, H)
