"""Host logic of the joint marginals: the factorisation schedule of tile_sym.h runs on the CPU with dense tile arithmetic, keeping the
panel products where the GPU keeps them, then X = S^-1 G for the unit columns of several poses runs the JointSchedule launches with their
tasks in shuffled order (csrc/joint_check.cpp, g++).  X on the whole elimination-tree closure and the joint blocks are compared with a
dense inverse; running the column blocks one batch at a time must give the same X bit for bit.  No GPU."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "dynosam_amd", "csrc")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("joint") / "joint_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", os.path.join(CSRC, "joint_check.cpp"), "-o", exe])
    return exe


def run(exe, *args, **env):
    out = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=300, env=dict(os.environ, **env))
    assert out.returncode == 0, out.stdout + out.stderr
    kv = dict(tok.split("=") for tok in out.stdout.split() if "=" in tok)
    return {k: float(v) for k, v in kv.items()}


def check(r):
    assert r["rel"] < 1e-10 and r["rel_joint"] < 1e-10
    # forward: one launch per height of the closure C (T^-1 fused into it); backward: one per depth below the root(s)
    assert r["launches"] == r["expect"]
    assert r["cols"] <= r["nt"] and r["products"] <= r["every_products"]
    return r


# the parameter sets of tests/test_selinv_schedule.py (band, twisted, extra links, a single pose)
@pytest.mark.parametrize("args", [(60, 5, 0, 1), (60, 5, 1, 1), (200, 14, 1, 2), (37, 3, 1, 3, 10), (5, 2, 1, 4), (1, 0, 1, 5),
                                  (120, 8, 1, 6, 5), (90, 6, 1, 7, 0, 20)])
def test_joint_columns_match_dense_inverse(checker, args):
    r = check(run(checker, *args))
    if args[0] >= 8:
        # the first and the latest pose, the middle and random ones: more than one 32-wide column block
        assert r["keys"] >= 6 and r["blocks"] >= 2


def test_row_tasks_and_deferred_updates(checker):
    for args, env in (((200, 14, 1, 2), {"TS_ROW_MIN": "0"}), ((120, 8, 1, 6, 5), {"TS_ROW_MIN": "0"}),
                      ((330, 3, 2, 5, 0, 10), {"TS_SRC_CAP": "1"}), ((330, 3, 2, 5, 0, 10), {"TS_SRC_CAP": "2", "TS_ROW_MIN": "0"})):
        check(run(checker, *args, **env))


def test_split_targets(checker):
    used = 0
    for args in ((330, 3, 2, 5, 0, 10), (330, 3, 2, 2, 20, 10), (200, 14, 1, 2)):
        for sp in (1, 2):
            r = check(run(checker, *args, TS_SPLIT=str(sp), TS_ROW_MIN="0"))
            used += int(r["scratch"] > 0)
    assert used >= 2


def test_a_latest_pose_query_touches_only_its_ancestor_path(checker):
    """a chain in frame order: the last pose's columns are the root of the tree, its query computes those columns only"""
    r = check(run(checker, 200, 14, 0, 3, TS_PROBE="-1"))
    assert r["cols"] <= 2 and r["launches"] <= 3 and r["products"] < 0.01 * r["every_products"]


def test_a_middle_pose_query_pays_for_its_path_only(checker):
    """the middle of a frame-order chain: its path to the root is half the chain, both passes walk it once"""
    r = check(run(checker, 200, 14, 0, 3, TS_PROBE="100"))
    assert r["cols"] < 0.6 * r["nt"] and r["launches"] == r["expect"] and r["products"] < 0.6 * r["every_products"]
