"""Create, train, destroy, again: the testbed's streams, events, pinned blocks and communicator are owned by handles
(neus2_amd/csrc/handle.h, host_util.h) and released by ~NeusTestbed in a fixed order. One cycle creates a testbed,
trains 34 steps in one call (occupancy updates, loss readbacks, lookahead steps and the call's last steps, where the
cuts are off), reads the parameters and destroys the testbed through neus_testbed_destroy, whose status is checked
(Testbed.__del__ discards it). Three cycles per variant (two of the last: creating its communicator takes ~2 s):
  plain     nothing switched on: the lazily created lookahead stream, its events and the abort word;
  timed     phase profiling, inference timing and exchange timing on: the phase-event sets and the inference-timing
            events (at one rank the exchange timing records nothing: no collective is issued);
  exchange  as timed, with a forced one-rank RCCL communicator: the communicator, the exchange stream, its events and
            the exchange-timing ring.
Every destroy returns 0, the parameter vectors of a variant's cycles are bitwise equal, and so are the variants' (timing
changes no result, and a one-rank all-reduce is the identity). Reads nothing outside the package and configs/."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, CYCLES = 34, 3
BATCH = 4096  # the smallest batch the suite trains at anywhere (a multiple of the 256-sample blocks)


def _cycle(sc, variant):
    from neus2_amd import pyngp
    from neus2_amd._lib import check, lib
    tb = pyngp.Testbed(pyngp.TestbedMode.Nerf)
    tb.set_dataset(sc["images"], sc["focal"], sc["principal"], sc["xforms"], 1)
    tb.reload_network_from_file(os.path.join(ROOT, "configs", "nerf", "base.json"), batch_size=BATCH)
    if variant == "exchange":
        tb.init_data_parallel(0, 1, pyngp.nccl_unique_id(), force_collectives=True)
    if variant != "plain":
        tb.set_profiling(True)
        check(lib().neus_testbed_set_infer_timing(tb.handle, C.c_int(1)))
        tb.set_exchange_timing(True)
    tb.train_steps(STEPS)
    params = tb.get_params().copy()
    assert tb.stats()["training_step"] == STEPS
    status = lib().neus_testbed_destroy(tb.handle)
    tb._h = None  # (destroyed: nothing left for __del__)
    check(status)
    return status, params


@pytest.fixture(scope="module")
def scene(torch_cuda):
    from neus2_amd import scenes
    return scenes.sphere_scene(8, 96, 72)


@pytest.fixture(scope="module")
def plain(scene):
    return [_cycle(scene, "plain") for _ in range(CYCLES)]


def _check(runs, ref):
    assert [s for s, _ in runs] == [0] * len(runs)
    assert np.all(np.isfinite(ref)) and np.any(ref != 0)
    for k, (_, p) in enumerate(runs):
        np.testing.assert_array_equal(p.view(np.uint32), ref.view(np.uint32), err_msg=f"cycle {k}")


def test_plain_cycles(plain):
    _check(plain, plain[0][1])


@pytest.mark.parametrize("variant, cycles", [("timed", CYCLES), ("exchange", 2)])
def test_instrumented_cycles_match_plain(scene, plain, variant, cycles):
    _check([_cycle(scene, variant) for _ in range(cycles)], plain[0][1])
