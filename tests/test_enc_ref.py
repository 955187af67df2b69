"""The float64 references of the parameter-free encodings (tests/enc_ref.py) against independent facts, and the config
validation of the native factories, which runs before any device call (no GPU needed)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import enc_ref as E
from torch_ref import sh4


def test_sh_degree4_matches_explicit_formulas():
    rng = np.random.default_rng(0)
    x = torch.tensor(rng.uniform(-0.2, 1.2, (500, 3)))
    err = (E.sh(x, 4) - sh4(x)).abs().max().item()
    assert err <= 1e-13, err


def test_sh_degree8_is_orthonormal_on_the_sphere():
    """Gram matrix of the 64 functions over the unit sphere: 24-point Gauss-Legendre in z times 48 equispaced azimuths
    integrates products of two degree-7 harmonics (degree 14) exactly."""
    z, wz = np.polynomial.legendre.leggauss(24)
    phi = 2 * np.pi * np.arange(48) / 48
    Z, P = np.meshgrid(z, phi, indexing="ij")
    s = np.sqrt(1 - Z ** 2)
    pts = np.stack([s * np.cos(P), s * np.sin(P), Z], axis=-1).reshape(-1, 3)
    w = np.repeat(wz, 48) * (2 * np.pi / 48)
    Y = E.sh(torch.tensor((pts + 1) / 2), 8).numpy()
    gram = (Y * w[:, None]).T @ Y
    err = np.abs(gram - np.eye(64)).max()
    assert err <= 1e-12, err


def test_frequency_is_exact_at_half_integers():
    x = torch.tensor([[0.0], [0.5], [1.0]], dtype=torch.float64)
    F = 16
    y = E.frequency(x, F).numpy().reshape(3, F, 2)
    for k in range(F):
        tol = 1e-15 * 2.0 ** k
        for i, xv in enumerate((0.0, 0.5, 1.0)):
            a = 2.0 ** k * xv  # half turns: an integer or an integer + 1/2
            want = (round(np.sin(np.pi * (a % 2))), round(np.cos(np.pi * (a % 2))))
            assert want[0] in (-1, 0, 1) and want[1] in (-1, 0, 1)
            assert abs(y[i, k, 0] - want[0]) <= tol and abs(y[i, k, 1] - want[1]) <= tol, (k, xv, y[i, k])


def test_composite_concatenates_and_pads():
    x = torch.tensor(np.random.default_rng(1).uniform(0, 1, (5, 9)))
    nested = [{"otype": "Identity", "n_dims_to_encode": 3, "scale": 2.0, "offset": -1.0},
              {"otype": "Frequency", "n_dims_to_encode": 3, "n_frequencies": 4}, {"otype": "SphericalHarmonics", "degree": 4}]
    e = E.composite(x, nested)
    assert e.shape == (5, 3 + 24 + 16)
    assert torch.equal(e[:, :3], 2.0 * x[:, :3] - 1.0) and torch.equal(e[:, 27:], E.sh(x[:, 6:], 4))
    p = E.pad_ones(e)
    assert p.shape == (5, 48) and torch.equal(p[:, 43:], torch.ones(5, 5, dtype=torch.float64))
    assert E.pad_ones(p) is p


NET = '{"otype": "FullyFusedMLP", "n_neurons": 64, "n_hidden_layers": 2}'
SH = lambda deg: '{"otype": "SphericalHarmonics", "degree": %d}' % deg
FREQ = lambda f: '{"otype": "Frequency", "n_frequencies": %d}' % f
BAD = [
    (3, SH(0), "must have positive degree"),
    (3, SH(9), "only implemented up to degree 8"),
    (2, SH(4), "3 input dims"),
    (3, FREQ(0), "n_frequencies must be in 1..16"),
    (3, FREQ(17), "n_frequencies must be in 1..16"),
    (6, '{"otype": "Composite", "nested": [{"otype": "HashGrid", "n_dims_to_encode": 3}, {"otype": "Identity"}]}',
     "Composite: nested encodings must be Identity, Frequency or SphericalHarmonics"),
    (6, '{"otype": "Composite", "nested": [{"otype": "Composite", "n_dims_to_encode": 3, "nested": []}, {"otype": "Identity"}]}',
     "Composite: nested encodings must be Identity, Frequency or SphericalHarmonics"),
    (7, '{"otype": "Composite", "nested": [{"otype": "Identity", "n_dims_to_encode": 3}, {"otype": "SphericalHarmonics", "n_dims_to_encode": 3}]}',
     "sum to 6, but n_input_dims is 7"),
]


def _lib():
    from neus2_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libneus2_hip.so not built")
    return _lib.lib()


@pytest.mark.parametrize("n_in,enc,msg", BAD)
def test_create_encoding_validates_config(n_in, enc, msg):
    lib = _lib()
    h = C.c_void_p()
    rc = lib.neus_module_create_encoding(C.c_uint32(n_in), enc.encode(), C.c_int(1), C.c_uint32(1024), C.byref(h))
    assert rc != 0 and msg in lib.neus_last_error().decode(), lib.neus_last_error().decode()


@pytest.mark.parametrize("n_in,enc,msg", BAD + [(9, FREQ(8), "1..128 input dims")])
def test_create_network_with_input_encoding_validates_config(n_in, enc, msg):
    """(9 dims x 8 frequencies = an encoded width of 144, above the FullyFusedMLP's 128 input dims)"""
    lib = _lib()
    h = C.c_void_p()
    rc = lib.neus_module_create_network_with_input_encoding(C.c_uint32(n_in), C.c_uint32(3), enc.encode(), NET.encode(), C.c_uint32(1024),
                                                            C.byref(h))
    assert rc != 0 and msg in lib.neus_last_error().decode(), lib.neus_last_error().decode()


def test_sh_tables_header_is_the_generators_output():
    """neus2_amd/csrc/sh_tables.h is scripts/gen_sh_tables.py's output, and its constants are the reference's c_m K_l^|m|."""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("gen_sh_tables", os.path.join(root, "scripts", "gen_sh_tables.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    assert open(gen.OUT).read() == gen.render()
    # Y_l^l at (x, y, z) = (1, 0, 0): T_l^l = (2l - 1)!!, H_l = 1
    x = torch.tensor([[1.0, 0.5, 0.5]], dtype=torch.float64)
    y = E.sh(x, 8)[0]
    for l in range(8):
        assert abs(gen.ck(l, l) * gen.double_factorial(l) - y[l * l + 2 * l].item()) <= 1e-13 * max(1.0, abs(y[l * l + 2 * l].item()))
