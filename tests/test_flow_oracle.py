"""CPU tests of the frontend path's oracle (oracle/flow_oracle.py) and host logic: no GPU.
The dense-flow producer has no reference arithmetic (the reference consumes an off-line RAFT image):
the oracle is checked against the exactly known flow of the synthetic scene instead."""
import numpy as np
import pytest

from dynosam_amd import synth_images as SI
from oracle import flow_oracle as FO


@pytest.fixture(scope="module")
def scene():
    return SI.make_pair(width=320, height=256, objects=2, seed=11, max_flow=6.0)


def test_oracle_flow_recovers_the_known_motion(scene):
    flow, match = FO.dense_flow(scene["rgb0"], scene["rgb1"])
    e = np.linalg.norm(flow - scene["flow_gt"], axis=-1)[scene["valid"]]
    # errors concentrate at object boundaries (patches straddling two motions): robust statistics
    assert np.median(e) < 0.2 and (e < 1.0).mean() > 0.92 and e.mean() < 0.8


def test_bf16_rounding_is_nearest_even():
    x = np.array([1.0, 1.00390625, 1.01171875, -2.5, 3.140625, 1e-3], np.float32)   # 1+2^-8 ties to even
    b = FO.to_bf16_bits(x)
    assert b[0] == 0x3F80 and b[1] == 0x3F80 and b[2] == 0x3F82
    assert np.all(np.abs(FO.bf16_to_f32(b) - x) <= np.abs(x) * 2.0 ** -8)


def test_track_dynamic_branches_in_reference_order():
    H, W = 48, 64
    mask = np.zeros((H, W), np.int32); mask[10:30, 10:40] = 3; mask[30:40, 10:40] = 4
    flow = np.zeros((H, W, 2), np.float32); flow[..., 0] = 1.5; flow[..., 1] = -0.5
    flow[12, 12] = (0.0, 1.0)
    kp = [(15.7, 15.2), (16.2, 15.9), (5.0, 5.0), (15.0, 32.0), (-1.0, 3.0), (12.3, 12.9), (38.9, 11.0), (20.0, 20.0)]
    prev = [3, 3, 3, 3, 3, 3, 3, 3]
    r = FO.track_dynamic(kp, prev, [0, 1, 2, 3, 4, 5, 30, 7], range(8), flow, mask, max_age=25, min_distance=2, next_tracklet_id=100)
    # 0 kept; 1 falls inside the disc blanked by 0; 2 background; 3 label 4 != 3; 4 not contained; 5 zero flow x; 6 kept, too old -> new tracklet
    assert list(r["code"]) == [FO.KEPT, FO.MASKED_OUT, FO.BACKGROUND, FO.LABEL_CHANGED, FO.NOT_CONTAINED, FO.ZERO_FLOW, FO.KEPT, FO.KEPT]
    assert r["new_tracklet_id"][6] == 100 and r["new_age"][6] == 0 and r["next_tracklet_id"] == 101
    assert r["new_age"][0] == 1 and np.allclose(r["predicted_kp"][0], (17.2, 14.7))


def test_shrunken_image_test_uses_truncated_coordinates():
    H, W = 32, 32
    mask = np.ones((H, W), np.int32)
    flow = np.zeros((H, W, 2), np.float32); flow[..., 0] = 20.0; flow[..., 1] = 0.25
    r = FO.track_dynamic([(20.0, 10.0), (5.0, 10.0)], [1, 1], [0, 0], [0, 1], flow, mask, shrink_row=2, shrink_col=2)
    assert list(r["code"]) == [FO.OUTSIDE_SHRUNKEN, FO.KEPT]


def test_fp64_corr_argmax_agrees_with_the_float32_oracle_and_measures_a_planted_error():
    """oracle/flow_oracle.corr_argmax_f64 (the float64 reference the GPU arg-max is judged by at sizes with padding) against
    corr_argmax on a small scene whose coarse grid (24 x 17 = 408 cells) is not a multiple of 32, at a narrow, the default and
    a grid-covering radius.  numpy's float32 sum is within CORR_G of the exact one, so wherever the two disagree the float64
    score of the float32 choice is within 2 CORR_G of the float64 maximum; a planted wrong match has a deficit far above that.
    Flat patches (zero descriptors) take the fall-back q = p in both."""
    sc = SI.make_pair(width=192, height=136, objects=1, seed=3, max_flow=5.0)
    rgb0 = sc["rgb0"].copy(); rgb0[:, 96:] = 90                                 # a flat half: its cells (zero descriptors) have no positive score
    p0, p1 = FO.pyramid(rgb0), FO.pyramid(sc["rgb1"])
    h3, w3 = p0[3].shape
    assert (w3, h3) == (24, 17)
    d0, d1 = FO.descriptors(p0[3]), FO.descriptors(p1[3])
    n = w3 * h3
    for R in (2, 6, 24):
        m32, C = FO.corr_argmax(d0, d1, w3, h3, R)
        m64, deficit = FO.corr_argmax_f64(d0, d1, w3, h3, R, got=m32)
        assert np.array_equal(FO.corr_argmax_f64(d0, d1, w3, h3, R), m64)
        differ = m32 != m64
        assert differ.mean() <= 0.005 and np.all(deficit[~differ] == 0) and np.all(deficit >= 0) and deficit.max() <= 2 * FO.CORR_G, (R, int(differ.sum()), deficit.max())
        px, py = np.arange(n) % w3, np.arange(n) // w3
        assert np.all(np.abs(m64 % w3 - px) <= R) and np.all(np.abs(m64 // w3 - py) <= R)
        # the float64 maximum itself agrees with the float32 matrix to float32 accuracy
        top32 = C[np.arange(n), m32]
        top64 = (FO.bf16_to_f32(d0).astype(np.float64) * FO.bf16_to_f32(d1[m64]).astype(np.float64)).sum(1)
        pos = top32 > 0
        assert pos.sum() > 200 and (~pos).sum() > 50 and np.all(m64[~pos] == np.arange(n)[~pos])
        assert np.abs(top32[pos] - top64[pos]).max() <= FO.CORR_G
        # a planted error: the neighbouring candidate instead of the best one
        bad = m64.copy()
        p = int(np.nonzero(pos & (m64 % w3 + 1 < w3) & (np.abs(m64 % w3 + 1 - px) <= R))[0][0])
        bad[p] = m64[p] + 1
        _, dbad = FO.corr_argmax_f64(d0, d1, w3, h3, R, got=bad)
        assert dbad[p] > 1e-3 and np.count_nonzero(dbad) == 1
    assert 3.7e-6 < FO.CORR_G < 3.9e-6
