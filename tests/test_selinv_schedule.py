"""Host logic of the selected inversion (marginal covariances): the factorisation schedule of tile_sym.h is executed on the CPU with
dense tile arithmetic, keeping the panel products where the GPU keeps them, then the selected-inversion launches (SelSchedule) run
with their tasks in shuffled order (csrc/selinv_check.cpp, g++) and every tile of Z = S^-1 on the pattern is compared with a dense
inverse; a query restricted to one pose's columns must give the same tiles bit for bit.  No GPU."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "dynosam_amd", "csrc")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sel") / "selinv_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", os.path.join(CSRC, "selinv_check.cpp"), "-o", exe])
    return exe


def run(exe, *args, **env):
    out = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=300, env=dict(os.environ, **env))
    assert out.returncode == 0, out.stdout + out.stderr
    kv = dict(tok.split("=") for tok in out.stdout.split() if "=" in tok)
    return {k: float(v) for k, v in kv.items()}


# the parameter sets of tests/test_tile_schedule.py (band, twisted, extra links, a single pose)
@pytest.mark.parametrize("args", [(60, 5, 0, 1), (60, 5, 1, 1), (200, 14, 1, 2), (37, 3, 1, 3, 10), (5, 2, 1, 4), (1, 0, 1, 5),
                                  (120, 8, 1, 6, 5), (90, 6, 1, 7, 0, 20)])
def test_selected_inverse_matches_dense_inverse(checker, args):
    r = run(checker, *args)
    assert r["rel"] < 1e-10
    assert r["part_cols"] <= r["nt"] and r["part_products"] <= r["products"]


def test_row_tasks_and_deferred_updates(checker):
    """the panel products come from the diagonal-target updates whatever the schedule packs into row tasks or defers (src_cap)"""
    for args, env in (((200, 14, 1, 2), {"TS_ROW_MIN": "0"}), ((120, 8, 1, 6, 5), {"TS_ROW_MIN": "0"}),
                      ((330, 3, 2, 5, 0, 10), {"TS_SRC_CAP": "1"}), ((330, 3, 2, 5, 0, 10), {"TS_SRC_CAP": "2", "TS_ROW_MIN": "0"})):
        assert run(checker, *args, **env)["rel"] < 1e-10


def test_split_targets(checker):
    """split tasks: the parts of a diagonal target that run in scratch tiles still store their sources' panel products"""
    used = 0
    for args in ((330, 3, 2, 5, 0, 10), (330, 3, 2, 2, 20, 10), (200, 14, 1, 2)):
        for sp in (1, 2):
            r = run(checker, *args, TS_SPLIT=str(sp), TS_ROW_MIN="0")
            assert r["rel"] < 1e-10
            used += int(r["scratch"] > 0)
    assert used >= 2


def test_a_latest_pose_query_does_not_pay_for_the_whole_inverse(checker):
    """a chain in frame order: the last pose's columns are the root of the tree, its query computes a few columns only"""
    r = run(checker, 200, 14, 0, 3, TS_PROBE="-1")
    assert r["rel"] < 1e-10
    assert r["part_cols"] <= 2 and r["part_products"] < 0.01 * r["products"]
