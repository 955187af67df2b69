"""tests/act_ref.py against torch.autograd, on the CPU in float64: the unrounded chain of the exact double backward (the
fronts, the backs from the output delta, the curvature adjoints e with act'' and the second weight-gradient product) equals
autograd on the same network to 1e-12 for every activation pair the GPU tests use, bare and behind an encoding; and the
derivative formulas written in the post-activation value are the derivatives."""
import numpy as np
import pytest
import torch

import act_ref as A

PAIRS = A.PAIRS + [("ReLU", "Sigmoid")]


def _close(got, want, what):
    scale = max(want.abs().max().item(), 1e-30)
    err = (got - want).abs().max().item() / scale
    assert err <= 1e-12, (what, err)


def _case(seed, n, n_in, W, N, out_pad):
    rng = np.random.default_rng(seed)
    in_pad = (n_in + 15) // 16 * 16
    shapes = [(W, in_pad)] + [(W, W)] * (N - 1) + [(out_pad, W)]
    mats = [torch.tensor(rng.uniform(-1, 1, s) * np.sqrt(6.0 / sum(s)) * 0.8) for s in shapes]
    x = torch.tensor(rng.uniform(-1, 1, (n, n_in)))
    u = torch.tensor(rng.normal(0, 1, (n, n_in)))
    g = torch.tensor(rng.normal(0, 1, (n, out_pad)))
    return mats, x, u, g


@pytest.mark.parametrize("name", ["Exponential", "Sigmoid", "Softplus", "Squareplus"])
def test_derivatives_from_the_output_value(name):
    x = torch.linspace(-1.5, 1.5, 61, dtype=torch.float64, requires_grad=True)
    y = A.act(name, x)
    d1, = torch.autograd.grad(y.sum(), x, create_graph=True)
    d2, = torch.autograd.grad(d1.sum(), x)
    _close(A.dact(name, y.detach()), d1.detach(), name + "'")
    _close(A.d2act(name, y.detach()), d2, name + "''")


@pytest.mark.parametrize("act_name,out_name", PAIRS)
def test_unrounded_chain_is_autograd(act_name, out_name):
    mats, x, u, g = _case(1, 48, 16, 32, 2, 16)
    X0 = x.clone().requires_grad_(True)
    ms = [m.clone().requires_grad_(True) for m in mats]
    gl = g.clone().requires_grad_(True)
    gx, = torch.autograd.grad((A.network(ms, X0, act_name, out_name) * gl).sum(), X0, create_graph=True)
    want = torch.autograd.grad((gx * u).sum(), ms + [gl, X0], allow_unused=True)
    got = A.chain(mats, x, u, g, act_name, out_name)
    for l, (a, b) in enumerate(zip(got["dW"], want[:3])):
        _close(a, b, f"dW{l}")
    _close(got["ddo"], want[3], "ddo")
    _close(got["dX0"], gx.detach(), "dX0")
    if want[4] is None:
        assert not got["q"].any()
    else:
        _close(got["q"], want[4], "q")


@pytest.mark.parametrize("act_name,out_name", PAIRS)
@pytest.mark.parametrize("encoding", ["identity", "frequency"])
def test_unrounded_chain_behind_an_encoding_is_autograd(act_name, out_name, encoding):
    import enc_ref
    mats, x, u, g = _case(2, 32, 3, 16, 2, 16) if encoding == "identity" else _case(2, 32, 2, 16, 1, 16)
    enc = (lambda xt, tab: xt * 0.5 + 0.25) if encoding == "identity" else (lambda xt, tab: enc_ref.frequency(xt, 4))
    want = A.truth(enc, x, None, u, mats, g, act_name, out_name, 1.0)
    got = A.bbi(enc, x, None, u, mats, g, act_name, out_name, 1.0, rounded=False)
    for l, (a, b) in enumerate(zip(got["dW"], want["dW"])):
        _close(a, b, f"dW{l}")
    _close(got["ddo"], want["ddo"], "ddo")
    _close(got["dx"], want["dx"], "dx")


def test_rounded_chain_is_close_to_the_unrounded_one():
    """the model's fp16 storage noise is small against an act'' term left out (an error of order one)"""
    mats, x, u, g = _case(3, 128, 16, 32, 2, 16)
    x, u, g = A.r16(x), A.r16(u), A.r16(g)
    mats = [A.r16(m) for m in mats]
    exact = A.chain(mats, x, u, g, "Softplus", "None")
    model = A.chain(mats, x, u, g, "Softplus", "None", rounded=True)
    no_curv = A.chain(mats, x, u, g, "None", "None")
    for l in range(3):
        assert A.rel(model["dW"][l], exact["dW"][l]) <= 5e-3
    assert A.rel(model["q"], exact["q"]) <= 5e-3 and not no_curv["q"].any()
