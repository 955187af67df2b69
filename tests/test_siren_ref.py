"""tests/siren_ref.py against itself and against known answers (CPU): the unrounded Sine chain must be torch.autograd on the
float64 network, or the floors the GPU tests derive from it mean nothing; and the SIREN initialisation's bounds and first
draws are pinned, so the GPU test that compares the device's initialize_params with the restatement compares it with the
rule of CutlassMLP::initialize_params."""
import numpy as np
import pytest
import torch

import siren_ref as S


def _shape(seed, n, n_in, W, N, n_out):
    rng = np.random.default_rng(seed)
    in_pad, out_pad = (n_in + 15) // 16 * 16, (n_out + 15) // 16 * 16
    shapes = [(W, in_pad)] + [(W, W)] * (N - 1) + [(out_pad, W)]
    scale = [30.0 / in_pad] + [np.sqrt(6.0 / k) for _, k in shapes[1:]]
    mats = [torch.tensor(rng.uniform(-s, s, sh)) for s, sh in zip(scale, shapes)]
    x, u = torch.tensor(rng.uniform(-1, 1, (n, n_in))), torch.tensor(rng.normal(0, 1, (n, n_in)))
    g = torch.tensor(rng.normal(0, 1, (n, out_pad)))
    return (lambda v, tab: v), x, None, u, mats, g, 1.0


@pytest.mark.parametrize("shape", [(1, 40, 3, 16, 1, 1), (2, 24, 12, 48, 3, 2)])
def test_unrounded_chain_is_autograd(shape):
    args = _shape(*shape)
    truth, model = S.truth(*args), S.model(*args, rounded=False)
    for key in ("y", "dx1", "ddo", "dx"):
        assert truth[key].abs().max() > 0
        assert S.rel(model[key].numpy(), truth[key].numpy()) <= 1e-12, key
    for key in ("dW1", "dW"):
        for a, b in zip(model[key], truth[key]):
            assert b.abs().max() > 0 and S.rel(a.numpy(), b.numpy()) <= 1e-12, key


def test_rounding_moves_the_chain_by_fp16_noise():
    """the rounded model is a different computation (the floor is not zero) at the size of fp16 storage noise"""
    args = _shape(3, 64, 3, 32, 2, 1)
    h = lambda v: v.to(torch.float16).to(torch.float64)
    args = (args[0], h(args[1]), None, h(args[3]), [h(m) for m in args[4]], h(args[5]), 1.0)
    truth, model = S.truth(*args), S.model(*args, rounded=True)
    for key in ("y", "dx1", "ddo", "dx"):
        assert 1e-5 < S.rel(model[key].numpy(), truth[key].numpy()) < 5e-3, key


def test_siren_initialisation_known_answer():
    """pcg32{7}'s first draws (the generator's own known answer) through next_float() * 2 scale - scale in float32, with
    scale = 30 / fan_in for the first matrix and sqrt(6 / fan_in) for the others; the grid's block stays within +-1e-4"""
    import oracle as O
    shapes = [(16, 16), (16, 16)]
    raw = O.pcg32(7, 1, 0, 260)
    assert [int(v) for v in raw[:3]] == [0x840D99CA, 0x12C757DE, 0x7481B420] and int(raw[256]) == 0x3122FCC3
    b = S.siren_bounds(shapes)
    assert float(b[0]) == 1.875 and float(b[1]) == float(np.sqrt(np.float32(6.0) / np.float32(16.0)))
    p = S.initialize_params(7, shapes, 1000)
    assert p.dtype == np.float32 and p.size == 512 + 1000
    assert [float(v).hex() for v in p[:3]] == ["0x1.e65f400000000p-5", "-0x1.99947e0000000p+0", "-0x1.58cce00000000p-3"]
    assert float(p[256]).hex() == "-0x1.8259940000000p-2"
    assert np.abs(p[:256]).max() <= b[0] and np.abs(p[:256]).max() > 0.95 * b[0]
    assert np.abs(p[256:512]).max() <= b[1] and np.abs(p[256:512]).max() > 0.95 * b[1]
    assert 0 < np.abs(p[512:]).max() <= 1e-4 and float(p[512]).hex() == "-0x1.68d75e0000000p-14"
    np.testing.assert_array_equal(S.initialize_params(7, shapes, 0), p[:512])
