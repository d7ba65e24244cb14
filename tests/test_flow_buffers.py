"""The buffer idiom of csrc/flow_buffers.h (DB, PinBuf, Events, Packed), exercised by csrc/flow_buffers_check.cpp on the host: the
runtime calls are stand-ins over malloc / memcpy that can be told to fail, the checker is a stand-alone program built with the address
and undefined-behaviour sanitizers and run as a child process (no GPU).  What it checks is listed at the top of the checker."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "dynosam_amd", "csrc")
CHECKS = ("failure_state", "grow_only", "put", "up_down", "events")


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fbc") / "flow_buffers_check")
    # the sanitizer runtimes are linked into the program: it then runs the same whatever else the loader brings in before them
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan",
                           os.path.join(CSRC, "flow_buffers_check.cpp"), "-o", exe])
    return subprocess.run([exe], capture_output=True, text=True, timeout=120)


def test_checker_passes_under_the_sanitizers(run):
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.rstrip().endswith("ALL OK"), run.stdout + run.stderr
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr


def test_every_check_ran(run):
    lines = [line for line in run.stdout.splitlines() if line.startswith("check=")]
    assert lines == ["check=%s OK" % name for name in CHECKS], run.stdout
