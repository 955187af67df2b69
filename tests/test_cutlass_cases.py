"""CutlassMLP on the CPU: the exact-integer shapes of test_gpu_cutlass_exact.py hold the domain in which the device's
arithmetic is exact (tests/int_net.py), and the network config is validated before any device call (through the C ABI)."""
import ctypes as C
import os

import pytest

import cutlass_cases
import int_net


@pytest.mark.parametrize("shape", cutlass_cases.SHAPES, ids=lambda s: "-".join(map(str, s[:5])))
def test_cutlass_shapes_hold_the_exact_domain(shape):
    n_in, n_out, W, N, n, capacity, seed = shape
    assert n <= capacity and n % 128 == 0
    int_net.check_domain(int_net.make(n_in, n_out, W, N, n, seed))


def _create(net):
    from neus2_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libneus2_hip.so not built")
    lib = _lib.lib()
    h = C.c_void_p()
    rc = lib.neus_module_create_network(C.c_uint32(3), C.c_uint32(3), net.encode(), C.c_uint32(1024), C.byref(h))
    return rc, lib.neus_last_error().decode()


@pytest.mark.parametrize("width", [24, 0, 520, 1024])
def test_cutlass_mlp_refuses_other_widths(width):
    rc, err = _create('{"otype": "CutlassMLP", "n_neurons": %d, "n_hidden_layers": 2}' % width)
    assert rc != 0, "created"
    for word in ("CutlassMLP", "n_neurons", "multiple of 16", "16 to 512", str(width)):
        assert word in err, err


def test_fully_fused_mlp_keeps_its_widths():
    rc, err = _create('{"otype": "FullyFusedMLP", "n_neurons": 256, "n_hidden_layers": 2}')
    assert rc != 0 and "FullyFusedMLP only supports 16, 32, 64, and 128 neurons, but got 256" in err, err
