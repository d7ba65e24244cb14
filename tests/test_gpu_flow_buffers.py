"""The grow-only buffers of the frontend library (csrc/flow_buffers.h) under the calls that use them: every entry point with a packed round
trip or a per-call scratch list is called three times on one FlowTracker - small, large, small again - where the large call forces every
grow-only buffer of the call to be reallocated between two uses.  The third result must equal the first and the large result must equal
the same call on a fresh context, bit for bit: nothing may depend on what a buffer held before it grew or on how large it has become.
The inputs are those of the entry points' own tests."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_pnp as PNP  # noqa: E402
import test_gpu_pointcloud as PC  # noqa: E402
import test_gpu_relpose as RP  # noqa: E402
from test_gpu_frontend_sizes import _klt_points  # noqa: E402
from test_motion_refine import K as K_MOTION, scene as motion_scene  # noqa: E402
from test_ransac_oracle import planted, planted_stereo  # noqa: E402
from tests import yolo_oracle as Y  # noqa: E402
from tests.test_refine_oracle import K as K_FLOW, scene as flow_scene  # noqa: E402
from dynosam_amd import synth_images as SI  # noqa: E402

pytestmark = pytest.mark.gpu

SIZE = (64, 64)          # no image is read by most of these calls: the smallest square context the frontend tests build
KLT_SIZE = (192, 136)    # sparse LK needs a pair with texture and more than one pyramid level


def _bytes(x):
    """a result as nested tuples of raw bytes: equality is bitwise (NaNs and signed zeros included)"""
    if isinstance(x, dict):
        return tuple((k, _bytes(v)) for k, v in sorted(x.items()))
    if isinstance(x, (list, tuple)):
        return tuple(_bytes(v) for v in x)
    if x is None:
        return None
    a = np.asarray(x)
    return (str(a.dtype), a.shape, np.ascontiguousarray(a).tobytes())


def _small_large_small(call, small, large, size=SIZE, prepare=None):
    from dynosam_amd.flow import FlowTracker

    def make():
        t = FlowTracker(*size)
        if prepare:
            prepare(t)
        return t
    t, fresh = make(), None
    try:
        first, big, third = _bytes(call(t, small)), _bytes(call(t, large)), _bytes(call(t, small))
        fresh = make()
        big_fresh = _bytes(call(fresh, large))
    finally:
        t.close()
        if fresh:
            fresh.close()
    assert third == first
    assert big == big_fresh


def test_refine_flow_pose():
    small = [flow_scene(3, seed=1, n_out=0)[0]]
    large = [flow_scene(200, seed=10 + k, n_out=10)[0] for k in range(4)]
    _small_large_small(lambda t, prs: t.refine_flow_pose(prs, K_FLOW), small, large)


def test_refine_motion():
    def problems(scenes):
        return [dict(X_prev=s["X0"], X_cur=s["X1"], motion_init=s["H0"], kp_prev=s["kp0"], kp_cur=s["kp1"], lmk_prev_world=s["l0"], lmk_cur_world=s["l1"]) for s in scenes]
    small = problems([motion_scene(3, seed=1, n_out=0)])
    large = problems([motion_scene(200, seed=10 + k, n_out=10) for k in range(4)])
    _small_large_small(lambda t, prs: t.refine_motion(prs, K_MOTION), small, large)


def test_pnp_ransac():
    Kc, small, _ = PNP._frame(1, sizes=(9,))
    _, large, _ = PNP._frame(2, sizes=(300, 300, 300))
    _small_large_small(lambda t, a: t.pnp_ransac(a[0], Kc, PNP.THR, n_hypotheses=a[1]), (small, 64), (large, 256))


def test_point_cloud_ransac():
    small, _ = PC._frame(1, sizes=(9,))
    large, _ = PC._frame(2, sizes=(300, 300, 300))
    _small_large_small(lambda t, a: t.point_cloud_ransac(a[0], PC.THR[0], n_hypotheses=a[1]), (small, 64), (large, 256))


@pytest.mark.parametrize("alg", [0, 1])
def test_relative_pose_ransac(alg):
    small, large = RP._frame(1, (9,)), RP._frame(2, (300, 300, 300))
    _small_large_small(lambda t, a: t.relative_pose_ransac(a[0], RP.K, RP.THR, algorithm=alg, n_hypotheses=a[1]), (small, 64), (large, 256))


def test_track_points_klt_verified():
    sc = SI.make_pair(width=KLT_SIZE[0], height=KLT_SIZE[1], objects=2, seed=4)
    small, large = _klt_points(KLT_SIZE, 7, 16, lo=8.0, hi=-8.0), _klt_points(KLT_SIZE, 8, 400)
    _small_large_small(lambda t, pts: t.track_points_klt_verified(pts, True, 5.0), small, large, size=KLT_SIZE,
                       prepare=lambda t: t.upload(sc["rgb0"], sc["mask0"], sc["rgb1"], sc["mask1"]))


def test_verify_homography():
    _small_large_small(lambda t, ab: t.verify_homography(ab[0], ab[1], 5.0), planted(16, 3, 1)[:2], planted(400, 80, 2)[:2])


def test_stereo_track_with_given_matches():
    def case(n, n_out, seed):
        left, right, _, _ = planted_stereo(n, n_out, seed)
        st = np.ones(n, np.uint8); st[:3] = 0
        return left, right, st
    _small_large_small(lambda t, a: t.stereo_track(a[0], 700.0, 0.12, matches=(a[1], a[2])), case(16, 3, 1), case(400, 60, 2))


def test_yolo_detect_and_masks():
    W, H, nw, nh, gain, px, py, _ph, _pw = Y.MASK_GEOMS[0]
    assert (W, H) == SIZE
    pred, proto = Y.mask_scene(Y.MASK_GEOMS[0], 32, 0)

    def call(t, max_det):
        d = t.yolo_detect(pred, proto, (nw, nh), gain, (px, py), iou=0.7, max_det=max_det)
        mask, pixels = t.yolo_masks(want_pixels=True)
        return d.n_det, d.n_candidates, d.anchor, d.class_id, d.score, d.boxes, mask, pixels
    _small_large_small(call, 4, 100)
