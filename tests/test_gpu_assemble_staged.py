"""k_assemble_rhs stages the Z rows of a chunk's Schur pairs through LDS, ASM_STAGE contributions at a time (kernels.h:
asm_chunks_body).  It can go wrong where a stage or a chunk (64 contributions) ends, so these graphs put exact pair counts
into single blocks: with static_track=(F, F) every static point is born in frame 0 and seen in all F frames, hence every
camera-camera block receives P static Schur pairs plus a small fixed number from the dynamic points.  Sweeping P over whole
ranges puts every count around 16, 32, 48, 64, 128 (and 1, odd counts) into a block whatever that fixed offset is.

Each case: Context.solve_damped(lam) against oracle.OracleGraph(g).solve_damped(lam), the tolerances of test_gpu_parity.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from dynosam_amd import synth  # noqa: E402

SWEEP_A = list(range(40, 73)) + list(range(118, 135))   # one chunk, a full chunk, chunk + 1; two chunks +- 1; every stage end between
SWEEP_B = list(range(1, 21))                            # single-stage chunks: n = 1, odd n, n below / at / above 16
TWO_FRAMES = [1, 63, 64, 65, 129]                       # few blocks per pose; the gradient loop's trip count changes at 64 edges per pose
THREE_LAMBDAS = {(3, 64), (3, 129), (2, 65)}


@pytest.fixture(scope="module")
def lib_loaded():
    """Fail loudly if the HIP extension is missing: no fallback exists."""
    from dynosam_amd import _lib
    return _lib.load()


def ctx_for(g):
    from dynosam_amd.optimizer import Context
    c = Context()
    c.upload(g)
    return c


def graph(F, P):
    return synth.make_hybrid_graph(synth.config(1, frames=F, objects=1, static_points=P, dynamic_points_per_object=8,
                                                static_track=(F, F), dynamic_track=(F, F), seed=7))


def check(F, P, oracle):
    g = graph(F, P)
    c, og = ctx_for(g), oracle.OracleGraph(g)
    try:
        for lam in ((1e-5, 1e-3, 10.0) if (F, P) in THREE_LAMBDAS else (1e-3,)):
            d, dec = c.solve_damped(lam)
            bad, dr, decr = og.solve_damped(lam)
            assert bad == 0, (F, P, lam)
            assert np.abs(d - dr).max() <= 1e-6 * max(1.0, np.abs(dr).max()), (F, P, lam)
            assert abs(dec - decr) <= 1e-9 * abs(decr), (F, P, lam)
    finally:
        c.close()


@pytest.mark.parametrize("P", SWEEP_A)
def test_chunk_and_stage_boundaries(lib_loaded, oracle, P):
    check(3, P, oracle)


@pytest.mark.parametrize("P", SWEEP_B)
def test_single_stage_chunks(lib_loaded, oracle, P):
    check(3, P, oracle)


@pytest.mark.parametrize("P", TWO_FRAMES)
def test_two_frames(lib_loaded, oracle, P):
    check(2, P, oracle)
