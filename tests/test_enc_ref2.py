"""The float64 references of TriangleWave, OneBlob and NRC (tests/enc_ref2.py) against independent facts, and the config
validation of the native factories for these otypes, which runs before any device call (no GPU needed)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import enc_ref2 as E2


def _x(seed, n, D, lo=-0.25, hi=1.25):
    return torch.tensor(np.random.default_rng(seed).uniform(lo, hi, (n, D)).astype(np.float32).astype(np.float64))


@pytest.mark.parametrize("B", [2, 4, 8, 64, 128])
def test_oneblob_rows_sum_to_one(B):
    """the three images tile the line: the bins of one input dim are a partition of unity"""
    y = E2.oneblob(_x(B, 400, 3), B).reshape(400, 3, B)
    err = (y.sum(dim=2) - 1.0).abs().max().item()
    assert err <= 1e-15, err


@pytest.mark.parametrize("B", [4, 8, 64, 128])
def test_oneblob_has_at_most_three_nonzeros_per_dim(B):
    x = torch.cat([_x(B, 400, 2), torch.tensor([[0.0, 1.0], [0.5, 0.25], [-1.0, 2.0], [-1.5, 2.5]], dtype=torch.float64)])
    y = E2.oneblob(x, B).reshape(-1, 2, B)
    assert int((y != 0).sum(dim=2).max()) <= 3
    assert float(y.min()) >= 0.0 and float(y.max()) <= 1.0


@pytest.mark.parametrize("B", [1, 2, 4, 16])
def test_oneblob_autograd_matches_the_closed_forms(B):
    """the first and second derivative from autograd are the stated closed forms (q and q')"""
    x = torch.cat([_x(10 + B, 200, 2), torch.tensor([[0.0, 1.0], [0.5, 0.25]], dtype=torch.float64)]).requires_grad_(True)
    y = E2.oneblob(x, B)
    d1, d2 = E2.oneblob_dx(x.detach(), B), E2.oneblob_d2x(x.detach(), B)
    for k in range(y.shape[1]):
        d = k // B
        g, = torch.autograd.grad(y[:, k].sum(), x, create_graph=True)
        h, = torch.autograd.grad(g[:, d].sum(), x, retain_graph=True)
        assert (g.detach()[:, d] - d1[:, k]).abs().max().item() <= 1e-12 and not g.detach()[:, 1 - d].any()
        assert (h[:, d] - d2[:, k]).abs().max().item() <= 1e-12


def test_triangle_wave_range_and_known_values():
    F = 16
    y = E2.triangle_wave(_x(2, 500, 3), F)
    assert y.shape == (500, 3 * F) and float(y.min()) >= -1.0 and float(y.max()) <= 1.0
    # val = x 2^(k-1) + k / 4 at x = 0, 0.5, 1 is a multiple of 1/4: y = 1, 0, -1, 0 at f = 0, 1/4, 1/2, 3/4
    x = torch.tensor([[0.0], [0.5], [1.0]], dtype=torch.float64, requires_grad=True)
    y = E2.triangle_wave(x, F)
    table = {0.0: 1.0, 0.25: 0.0, 0.5: -1.0, 0.75: 0.0}
    for k in range(F):
        g, = torch.autograd.grad(y[:, k].sum(), x, retain_graph=True)
        for i, xv in enumerate((0.0, 0.5, 1.0)):
            val = xv * 2.0 ** (k - 1) + k / 4.0
            assert y[i, k].item() == table[val % 1.0], (k, xv)
            want = -2.0 ** (k + 1) if int(np.floor(2.0 * val)) % 2 == 0 else 2.0 ** (k + 1)
            assert g[i, 0].item() == want, (k, xv, g[i, 0].item(), want)


def test_triangle_wave_has_no_second_derivative():
    x = _x(3, 50, 2).requires_grad_(True)
    g, = torch.autograd.grad(E2.triangle_wave(x, 5).sum(), x, create_graph=True)
    assert not g.requires_grad  # piecewise constant: the graph ends at the detached sign


def test_nrc_is_the_explicit_composite():
    for D in (8, 9, 11):
        x = _x(D, 40, D)
        a = E2.encode(x, {"otype": "NRC", "n_frequencies": 5, "n_bins": 8})
        b = E2.encode(x, {"otype": "Composite", "nested": E2.nrc_nested(D, 5, 8)})
        c = E2.encode(x, {"otype": "OneBlobFrequency", "n_frequencies": 5, "n_bins": 8})
        assert a.shape == (40, 15 + 40 + D - 8) and torch.equal(a, b) and torch.equal(a, c)
        assert torch.equal(a[:, 55:], x[:, 8:])
    assert E2.encode(_x(0, 4, 9), {"otype": "NRC"}).shape == (4, 36 + 20 + 1)
    assert [s[:3] for s in E2.segments({"otype": "NRC"}, 9)] == [("TriangleWave", 0, 36), ("OneBlob", 36, 20), ("Identity", 56, 1)]


def test_encode_falls_through_to_enc_ref():
    import enc_ref as E
    x = _x(5, 20, 3)
    cfg = {"otype": "Frequency", "n_frequencies": 3}
    assert torch.equal(E2.encode(x, cfg), E.encode(x, cfg))


NET = '{"otype": "FullyFusedMLP", "n_neurons": 64, "n_hidden_layers": 2}'
BLOB = lambda b: '{"otype": "OneBlob", "n_bins": %d}' % b
TRI = lambda f: '{"otype": "TriangleWave", "n_frequencies": %d}' % f
BAD = [
    (3, BLOB(0), "n_bins must be in 1..128"),
    (3, BLOB(3), "Number of bins must be a power of 2"),
    (3, BLOB(256), "n_bins must be in 1..128"),
    (3, TRI(0), "n_frequencies must be in 1..16"),
    (3, TRI(17), "n_frequencies must be in 1..16"),
    (7, '{"otype": "NRC"}', "n_input_dims must be at least 8"),
    (7, '{"otype": "OneBlobFrequency"}', "n_input_dims must be at least 8"),
    (4, '{"otype": "Composite", "nested": [{"otype": "OneBlob", "n_dims_to_encode": 2, "n_bins": 6}, {"otype": "TriangleWave"}]}',
     "Number of bins must be a power of 2"),
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


@pytest.mark.parametrize("n_in,enc,msg", BAD + [(3, BLOB(64), "1..128 input dims")])
def test_create_network_with_input_encoding_validates_config(n_in, enc, msg):
    """(3 dims x 64 bins = an encoded width of 192, above the FullyFusedMLP's 128 input dims)"""
    lib = _lib()
    h = C.c_void_p()
    rc = lib.neus_module_create_network_with_input_encoding(C.c_uint32(n_in), C.c_uint32(3), enc.encode(), NET.encode(), C.c_uint32(1024),
                                                            C.byref(h))
    assert rc != 0 and msg in lib.neus_last_error().decode(), lib.neus_last_error().decode()


def test_refusals_name_the_new_otypes():
    """the unknown-otype messages list what is accepted"""
    lib = _lib()
    h = C.c_void_p()
    rc = lib.neus_module_create_encoding(C.c_uint32(3), b'{"otype": "HannWindowFrequency"}', C.c_int(1), C.c_uint32(1024), C.byref(h))
    msg = lib.neus_last_error().decode()
    assert rc != 0 and all(w in msg for w in ("TriangleWave", "OneBlob", "NRC", "implemented on gfx950")), msg
