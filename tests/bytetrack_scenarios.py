"""Seeded ByteTrack scenarios (boxes with constant velocity plus noise) shared by tests/test_bytetrack_oracle.py and
tests/test_gpu_bytetrack.py.  Each one comes with a check ON THE ORACLE'S OUTPUT that it exercises what it is for, so a device test
on it cannot pass vacuously.  scenario(name) -> (frames, params, check); frames = [(boxes [n, 4], score [n], class_id [n]), ...]."""
import numpy as np

from tests import bytetrack_oracle as O

f32 = np.float32


def obj(x, y, w, h, vx=0.0, vy=0.0, score=0.9, cls=0, grow=0.0):
    """an object: centre, size, velocity per frame; score: a number or f(frame) -> number / None (None: not detected in that frame)"""
    return dict(x=x, y=y, w=w, h=h, vx=vx, vy=vy, score=score if callable(score) else (lambda f, s=score: s), cls=cls, grow=grow)


def make(objs, n_frames, seed, noise=0.5):
    rng = np.random.default_rng(seed)
    frames, who = [], []
    for f in range(1, n_frames + 1):
        b, s, c, w = [], [], [], []
        for k, o in enumerate(objs):
            e = rng.uniform(-noise, noise, 4)          # drawn for every object and frame: the sequence does not depend on who is visible
            sc = o["score"](f)
            if sc is None:
                continue
            cx, cy = o["x"] + o["vx"] * (f - 1), o["y"] + o["vy"] * (f - 1)
            ww, hh = o["w"] + o["grow"] * (f - 1), o["h"] + o["grow"] * (f - 1)
            b.append([cx - ww / 2 + e[0], cy - hh / 2 + e[1], cx + ww / 2 + e[2], cy + hh / 2 + e[3]])
            s.append(sc); c.append(o["cls"]); w.append(k)
        frames.append((np.array(b, f32).reshape(-1, 4), np.array(s, f32), np.array(c, np.int32)))
        who.append(w)
    return frames, who


def label_of(res, who, f, k):
    """the label object k carries in frame f (1-based), None if it was not detected there"""
    return int(res[f - 1][0]["labels"][who[f - 1].index(k)]) if k in who[f - 1] else None


def ids(res, f):
    return [int(v) for v in res[f - 1][1]["id"]]


def _a():
    frames, who = make([obj(100, 100, 60, 80, 3, 1, score=lambda f: 0.3 if f == 4 else 0.9), obj(300, 200, 50, 50, -2, 0)], 6, 1)

    def check(res):
        i = label_of(res, who, 1, 0)
        assert i > 0 and all(label_of(res, who, f, 0) == i for f in range(1, 7))
        assert frames[3][1][who[3].index(0)] < f32(0.5)        # the label of frame 4 comes through the second association
    return frames, {}, check


def _b():
    frames, who = make([obj(100, 100, 60, 80, 2, 1), obj(300, 200, 50, 70, -1, 1, score=lambda f: None if 4 <= f <= 6 else 0.9)], 9, 2)

    def check(res):
        i = label_of(res, who, 3, 1)
        assert i > 0 and label_of(res, who, 7, 1) == i
        for f in (4, 5, 6):
            t = res[f - 1][1]
            assert t["state"][list(t["id"]).index(i)] == O.LOST
        t = res[6][1]
        assert t["tracklet_len"][list(t["id"]).index(i)] == 0 and t["state"][list(t["id"]).index(i)] == O.TRACKED   # re_activate
    return frames, {}, check


def _c():
    frames, who = make([obj(100, 100, 60, 80, 2, 1), obj(300, 200, 50, 70, 0, 0, score=lambda f: None if 3 <= f <= 7 else 0.9)], 10, 3)

    def check(res):
        i = label_of(res, who, 2, 1)
        assert i in ids(res, 4) and i not in ids(res, 5)        # last seen at frame 2, max_time_lost 2: Removed when frame - 2 > 2
        assert label_of(res, who, 8, 1) == 0                    # a new, unconfirmed track
        j = label_of(res, who, 9, 1)
        assert j > 0 and j != i
    return frames, dict(track_buffer=2), check


def _d():
    frames, who = make([obj(100, 100, 60, 80, 2, 1), obj(300, 200, 50, 70, 1, 0, score=lambda f: None if f < 3 else 0.9)], 5, 4)

    def check(res):
        assert label_of(res, who, 1, 0) > 0                     # frame 1: labelled at once
        assert label_of(res, who, 3, 1) == 0
        j = label_of(res, who, 4, 1)
        assert j > 0 and label_of(res, who, 5, 1) == j
        t = res[2][1]
        assert t["activated"][list(t["id"]).index(j)] == 0
    return frames, {}, check


def _e():
    frames, who = make([obj(100, 100, 60, 80, 2, 1), obj(300, 200, 50, 70, 1, 0, score=lambda f: 0.9 if f == 3 else None)], 5, 5)

    def check(res):
        assert len(ids(res, 3)) == 2 and res[2][1]["activated"][1] == 0
        assert len(ids(res, 4)) == 1 and res[3][0]["n_removed"] == 1 and res[3][0]["n_lost"] == 0
    return frames, {}, check


def _f(direction):
    # B stands at x = 400 for a while and is then missed (Lost, at rest); A walks onto it.  direction 0: A is the older track, the Lost B is
    # dropped.  direction 1: B is older, the Tracked A is dropped - and the detection re-activates B on the next frame.
    if direction == 0:
        a = obj(280, 200, 60, 80, 8, 0)
        b = obj(400, 200, 60, 80, 0, 0, score=lambda f: 0.9 if 3 <= f <= 6 else None)
    else:
        a = obj(280 - 8 * 4, 200, 60, 80, 8, 0, score=lambda f: None if f < 5 else 0.9)
        b = obj(400, 200, 60, 80, 0, 0, score=lambda f: 0.9 if f <= 4 else None)
    frames, who = make([a, b], 22, 6 + direction, noise=0.25)

    def check(res):
        ia = label_of(res, who, 8, 0)
        ib = label_of(res, who, 4, 1)
        assert ia > 0 and ib > 0 and ia != ib
        gone = [(f, set(ids(res, f - 1)) - set(ids(res, f))) for f in range(2, 23)]
        gone = [(f, g) for f, g in gone if g]
        assert len(gone) == 1, gone
        f, g = gone[0]
        assert g == ({ib} if direction == 0 else {ia})
        t = res[f - 2][1]                                       # the frame before: both there, B Lost and not yet old
        assert t["state"][list(t["id"]).index(ib)] == O.LOST and f - t["end_frame"][list(t["id"]).index(ib)] <= 30
        if direction == 1:
            assert label_of(res, who, f, 0) == 0 and label_of(res, who, f + 1, 0) == ib
    return frames, {}, check


def _g():
    # two objects at rest, 60 apart, 100 wide; in frame 4 both detections jump left: the second one lands nearer to the FIRST track
    # than to its own.  Nearest-first takes that pair and leaves the other track without a partner; the optimum pairs both.
    frames, who = make([obj(200, 200, 100, 120), obj(260, 200, 100, 120)], 3, 8, noise=0.1)
    y0, y1 = 140.0, 260.0
    frames.append((np.array([[150 - 35, y0, 250 - 35, y1], [150 + 25, y0, 250 + 25, y1]], f32), np.array([0.9, 0.9], f32), np.zeros(2, np.int32)))
    who.append([0, 1])

    def check(res):
        t = res[2][1]
        kf = [t["filter"][r].copy() for r in range(2)]
        for k in kf:
            O.kf_predict(k)
        d = [[f32(1) - O.iou(O.box_of(kf[r]), frames[3][0][c]) for c in range(2)] for r in range(2)]
        pairs = sorted((d[r][c], r, c) for r in range(2) for c in range(2))
        assert pairs[0][1:] == (0, 1) and d[1][0] >= f32(0.8)   # nearest-first: track 0 takes detection 1, track 1 is left alone
        assert [int(v) for v in res[3][0]["labels"]] == [int(t["id"][0]), int(t["id"][1])]   # the optimum
    return frames, {}, check


def _h():
    # one track, two high detections: the nearer one has the lower score; with fuse_score the farther, confident one wins
    frames, who = make([obj(200, 200, 100, 100)], 3, 9, noise=0.1)
    frames.append((np.array([[150 + 25, 150, 250 + 25, 250], [150 - 33, 150, 250 - 33, 250]], f32), np.array([0.55, 0.95], f32), np.zeros(2, np.int32)))

    def check(res):
        plain = O.track(frames, {})
        assert [int(v) for v in plain[3][0]["labels"]] == [1, 0] and [int(v) for v in res[3][0]["labels"]] == [0, 1]
    return frames, dict(fuse_score=1), check


def _i():
    frames, who = make([obj(100 + 120 * k, 100 + 20 * k, 60, 80, 2, 1) for k in range(5)], 3, 10)

    def check(res):
        assert res[0][0]["n_not_started"] == 2 and res[0][0]["n_new"] == 3 and len(ids(res, 3)) == 3
        assert [int(v) for v in res[0][0]["labels"]] == [1, 2, 3, 0, 0]
    return frames, dict(max_tracks=3), check


def _j():
    nan, inf = float("nan"), float("inf")
    frames, who = make([obj(100, 100, 60, 80, 2, 1), obj(300, 300, 50, 50)], 3, 11)
    bad = np.array([[nan, 10, 50, 60], [10, 10, inf, 60], [10, 10, 10, 60], [50, 10, 10, 60], [10, 60, 50, 10], [500, 400, 560, 480], [10, -inf, 50, 60]], f32)
    bad_s = np.array([0.9, 0.9, 0.9, 0.9, 0.9, nan, 0.9], f32)
    frames = [(np.concatenate([bad[:3], b, bad[3:]]), np.concatenate([bad_s[:3], s, bad_s[3:]]), np.concatenate([np.zeros(3, np.int32), c, np.zeros(4, np.int32)]))
              for b, s, c in frames]

    def check(res):
        for r, t in res:
            assert [int(v) for v in r["labels"]] == [0, 0, 0, 1, 2, 0, 0, 0, 0] and list(t["id"]) == [1, 2]
    return frames, {}, check


SCENARIOS = {"a_low_score": _a, "b_reactivate": _b, "c_removed_new_id": _c, "d_confirmation": _d, "e_unconfirmed_removed": _e,
             "f_duplicate_lost_dropped": lambda: _f(0), "f_duplicate_tracked_dropped": lambda: _f(1), "g_optimal_not_greedy": _g,
             "h_fuse_score": _h, "i_max_tracks": _i, "j_invalid": _j}


def scenario(name):
    return SCENARIOS[name]()


def cluster(n_tracks, n_dets, seed, grid=0.0, n_frames=3):
    """n_tracks objects in one cluster of heavily overlapping boxes (every pair of boxes overlaps: every pair is an edge at a limit above
    1) for n_frames - 1 frames, then n_dets detections in the same cluster.  grid > 0: all coordinates on that grid, so many costs tie."""
    rng = np.random.default_rng(seed)

    def boxes(n):
        c = rng.uniform(-20, 20, (n, 2)) + 300
        wh = rng.uniform(180, 220, (n, 2))
        b = np.concatenate([c - wh / 2, c + wh / 2], axis=1)
        if grid:
            b = np.round(b / grid) * grid
        return b.astype(f32)
    base = boxes(n_tracks)
    frames = []
    for f in range(n_frames - 1):
        frames.append((base.copy(), np.full(n_tracks, 0.9, f32), (np.arange(n_tracks) % 3).astype(np.int32)))
    frames.append((boxes(n_dets), rng.uniform(0.2, 0.99, n_dets).astype(f32), (np.arange(n_dets) % 5).astype(np.int32)))
    return frames


def staircase(n):
    """n wide boxes 3 pixels apart for two frames, then the same row of boxes shifted by 1.6 and listed in REVERSE order: every pair is an
    edge at a limit above 1, and the column a row likes best is held by an earlier row again and again - the augmenting path of row i
    visits i columns (n (n - 1) / 2 steps in all, asserted on the oracle)."""
    x = 3.0 * np.arange(n)

    def boxes(x):
        return np.stack([x, np.full(n, 100.0), x + 300, np.full(n, 400.0)], axis=1).astype(f32)
    s, c = np.full(n, 0.9, f32), np.zeros(n, np.int32)
    return [(boxes(x), s, c), (boxes(x), s, c), (boxes(x[::-1] + 1.6), s, c)]
