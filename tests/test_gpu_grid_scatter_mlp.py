""""gradient_scatter": "binned" of a general grid in front of a FullyFusedMLP: case B of test_gpu_grid_nd.py (2-D, 4 features,
Smoothstep) in front of a 64-wide network with two hidden layers, n = 256, parameters from grid_nd_ref.network_params.

* ReLU: both gradients (the matrices and the grid block) against float64 autograd with the fp16 modelling of
  tests/grid_nd_ref.grid_network, at the bars test_gpu_grid_nd_mlp.py holds the atomic module to: rel-L2 <= 2e-3 and
  1 - cosine <= 1e-5.
* Softplus with "second_order": "exact": backward_backward_input runs Enc::backward_curved, whose sums the binned path adds
  onto backward_backward's in one fp32 add per parameter. grid_network models ReLU only, so the yardstick here is the atomic
  module of the same config on the same operands, which the existing suite pins: the matrices never pass through the
  scatter and must be bitwise its own, the grid block holds the same bars, and more tightly the float-atomic tolerance of
  test_gpu_grid_nd_mlp.py (rtol 1e-5, atol 2e-5 x the largest magnitude): both sum the same fp32 contributions, the atomics
  in an order of their own, the binned path with at most 2^-33 per contribution.
* both: the whole dL_dparams vector of either gradient is bitwise equal over two calls."""
import numpy as np
import pytest

import grid_nd_ref as G
from bbi_ref import flat, rel_cos
from test_gpu_grid_nd import CASES, N, config, dev, inputs, tables

pytestmark = pytest.mark.gpu

W, NH, N_OUT = 64, 2, 16
CASE = "B"


def _net(act, **extra):
    return dict({"otype": "FullyFusedMLP", "activation": act, "output_activation": "None", "n_neurons": W, "n_hidden_layers": NH,
                 "gradient_precision": "fp32"}, **extra)


def _gradients(t, m, params, x, u, dlo):
    from neus2_amd.module import GradientMode
    ctx, y = m.forward(x, params, prepare_input_gradients=True)
    g = t.full((m.n_params,), float("nan"), dtype=t.float32, device="cuda")
    gs = t.full((m.n_params,), float("nan"), dtype=t.float32, device="cuda")
    ddo = t.zeros((N, 16), dtype=t.float16, device="cuda")
    ddx = t.zeros((N, CASES[CASE][0]), dtype=t.float32, device="cuda")
    m.backward(ctx, x, dlo, params, dL_dparams=g, mode=GradientMode.Overwrite, output=y)
    m.backward_backward_input(ctx, x, u, dlo, params, dL_dparams=gs, dL_ddLdoutput=ddo, mode=GradientMode.Overwrite, dL_dinput=ddx)
    return g.cpu().numpy(), gs.cpu().numpy()


def _setup(t, net):
    from neus2_amd.module import Module
    D, F, ty, ip, L, *_ = CASES[CASE]
    off, res = tables(CASE)
    width = F * L
    shapes = [(W, (width + 15) // 16 * 16), (W, W), (16, W)]
    rng = np.random.default_rng(61)
    ph = G.network_params(rng, shapes, width, D, off[-1] * F)
    pos, left_out = inputs(CASE)
    assert left_out <= 0.05
    make = lambda **enc: Module.create_network_with_input_encoding(D, N_OUT, config(CASE, **enc), net, batch_capacity=N)
    return make, shapes, ph, pos, rng


def _same(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_relu(torch_cuda):
    import torch
    t = torch_cuda
    D, F, ty, ip, L, *_ = CASES[CASE]
    off, res = tables(CASE)
    make, shapes, ph, pos, rng = _setup(t, _net("ReLU"))
    n_mlp = sum(r * k for r, k in shapes)
    m = make(gradient_scatter="binned")
    assert m.hyperparams()["encoding"]["gradient_scatter"] == "binned" and m.gradient_scatter == "binned"
    ref = G.grid_network(ph, pos, shapes, off, res, F, ty, ip)
    amb = ref["ambiguous"]
    assert amb.mean() <= 0.05
    dlo = rng.normal(0, 1, (N, 16)).astype(np.float16)
    v = rng.normal(0, 1, (N, D)).astype(np.float32)
    dlo[amb] = 0
    v[amb] = 0
    dlo_t = torch.tensor(dlo.astype(np.float64), requires_grad=True)
    g1 = torch.autograd.grad((ref["out"] * dlo_t).sum(), ref["leaves"] + [ref["xt"]], create_graph=True)
    g2 = torch.autograd.grad((g1[-1] * torch.tensor(v.astype(np.float64))).sum(), ref["leaves"] + [dlo_t, ref["xt"]])
    args = (dev(t, ph), dev(t, pos), dev(t, v), dev(t, dlo))
    gm, gsm = _gradients(t, m, *args)
    pairs = {"network": (gm[:n_mlp], flat(g1[:-2])), "grid": (gm[n_mlp:], flat(g1[-2:-1])),
             "network_2nd": (gsm[:n_mlp], flat(g2[:-3])), "grid_2nd": (gsm[n_mlp:], flat(g2[-3:-2]))}
    for k, (a, b) in pairs.items():
        rel, cos = rel_cos(a, b)
        print(f"binned ReLU {k}: rel {rel:.3e} 1-cos {1 - cos:.3e}")
        assert rel <= 2e-3 and 1 - cos <= 1e-5, (k, rel, cos)
    gm_b, gsm_b = _gradients(t, m, *args)
    assert _same(gm_b, gm) and _same(gsm_b, gsm)


def test_softplus_exact_second_order(torch_cuda):
    t = torch_cuda
    D = CASES[CASE][0]
    make, shapes, ph, pos, rng = _setup(t, _net("Softplus", second_order="exact"))
    n_mlp = sum(r * k for r, k in shapes)
    dlo = rng.normal(0, 1, (N, 16)).astype(np.float16)
    v = rng.normal(0, 1, (N, D)).astype(np.float32)
    args = (dev(t, ph), dev(t, pos), dev(t, v), dev(t, dlo))
    binned, atomic = make(gradient_scatter="binned"), make()
    gm, gsm = _gradients(t, binned, *args)
    am, asm = _gradients(t, atomic, *args)
    assert np.isfinite(gm).all() and np.isfinite(gsm).all() and gsm[n_mlp:].any()
    for k, got, want in (("first", gm, am), ("second", gsm, asm)):
        assert _same(got[:n_mlp], want[:n_mlp]), k
        rel, cos = rel_cos(got[n_mlp:], want[n_mlp:])
        print(f"binned Softplus, grid block of the {k}-order gradient against the atomic module: rel {rel:.3e} 1-cos {1 - cos:.3e}")
        assert rel <= 2e-3 and 1 - cos <= 1e-5, (k, rel, cos)
        np.testing.assert_allclose(got[n_mlp:], want[n_mlp:], rtol=1e-5, atol=2e-5 * max(1.0, np.abs(want[n_mlp:]).max()))
    gm_b, gsm_b = _gradients(t, binned, *args)
    assert _same(gm_b, gm) and _same(gsm_b, gsm)
