"""The general grid encoding in front of a FullyFusedMLP (create_network_with_input_encoding, module kind NdGridMlp): cases B
(2-D, 4 features, Smoothstep) and F (4-D, 2 features, Linear) of test_gpu_grid_nd.py in front of a 64-wide MLP with two
hidden ReLU layers and 16 outputs, n = 256, against float64 autograd with the fp16 modelling of tests/bbi_ref.py
(tests/grid_nd_ref.grid_network). Samples with a hidden pre-activation within 1e-4 of 0 are removed from both sides
(dL_doutput = 0 and dL_ddLdinput = 0; share <= 0.05). Bars: the project's fp16 bars, rel-L2 <= 2e-3 and 1 - cosine <= 1e-5
(test_gpu_grid_mlp.py, test_gpu_bbi_full.py)."""
import numpy as np
import pytest

import grid_nd_ref as G
from bbi_ref import flat, rel_cos
from test_gpu_grid_nd import CASES, N, config, dev, inputs, record, tables

pytestmark = pytest.mark.gpu

W, NH, N_OUT = 64, 2, 16
NET = {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": W, "n_hidden_layers": NH}


@pytest.mark.parametrize("case", ["B", "F"])
def test_grid_nd_mlp_module(torch_cuda, case):
    import torch
    from neus2_amd.module import GradientMode, Module
    t = torch_cuda
    D, F, ty, ip, L, *_ = CASES[case]
    off, res = tables(case)
    width = F * L
    in_pad = (width + 15) // 16 * 16
    shapes = [(W, in_pad), (W, W), (16, W)]
    n_mlp = sum(r * k for r, k in shapes)
    m = Module.create_network_with_input_encoding(D, N_OUT, config(case), dict(NET, gradient_precision="fp32"), batch_capacity=N)
    hp = m.hyperparams()
    assert m.n_params == n_mlp + off[-1] * F and m.n_input_dims == D and m.n_output_dims == 16
    assert m.info["grid_offset"] == n_mlp and m.info["n_levels"] == L
    assert hp["otype"] == "NetworkWithInputEncoding" and hp["encoding"]["interpolation"] == ip and hp["encoding"]["n_input_dims"] == D
    assert hp["encoding"]["n_features_per_level"] == F and hp["encoding"]["type"] == ty
    # initialize_params: the network block is create_network's on the encoded width, then the grid's rule
    p0 = m.initialize_params(11)
    plain = Module.create_network(width, N_OUT, NET, batch_capacity=N)
    assert plain.n_params == n_mlp and t.equal(p0[:n_mlp], plain.initialize_params(11))
    pg = p0[n_mlp:].cpu().numpy()
    assert 0 < np.abs(pg).max() <= 1e-4
    rng = np.random.default_rng(40 + ord(case))
    ph = G.network_params(rng, shapes, width, D, off[-1] * F)
    pos, left_out = inputs(case)
    assert left_out <= 0.05
    ref = G.grid_network(ph, pos, shapes, off, res, F, ty, ip)
    amb = ref["ambiguous"]
    print(f"case {case}: ambiguous share {amb.mean():.4f}")
    assert amb.mean() <= 0.05
    dlo = rng.normal(0, 1, (N, 16)).astype(np.float16)
    v = rng.normal(0, 1, (N, D)).astype(np.float32)
    dlo[amb] = 0
    v[amb] = 0
    dlo_t = torch.tensor(dlo.astype(np.float64), requires_grad=True)
    g1 = torch.autograd.grad((ref["out"] * dlo_t).sum(), ref["leaves"] + [ref["xt"]], create_graph=True)
    g2 = torch.autograd.grad((g1[-1] * torch.tensor(v.astype(np.float64))).sum(), ref["leaves"] + [dlo_t, ref["xt"]])
    params, x, u, dlo_dev = dev(t, ph), dev(t, pos), dev(t, v), dev(t, dlo)
    ctx, y = m.forward(x, params, prepare_input_gradients=True)
    assert y.dtype == t.float16 and tuple(y.shape) == (N, 16)
    g = t.full((m.n_params,), 7.0, dtype=t.float32, device="cuda")
    dx = t.full((N, D), 7.0, dtype=t.float32, device="cuda")
    m.backward(ctx, x, dlo_dev, params, dL_dparams=g, dL_dinput=dx, mode=GradientMode.Overwrite, output=y)
    gs = t.full((m.n_params,), 7.0, dtype=t.float32, device="cuda")
    ddo = t.full((N, 16), 7.0, dtype=t.float16, device="cuda")
    ddx = t.full((N, D), 7.0, dtype=t.float32, device="cuda")
    m.backward_backward_input(ctx, x, u, dlo_dev, params, dL_dparams=gs, dL_ddLdoutput=ddo, mode=GradientMode.Overwrite, dL_dinput=ddx)
    gm, gsm = g.cpu().numpy(), gs.cpu().numpy()
    pairs = {
        "forward": (y.float().cpu().numpy(), ref["out"].detach().numpy()),
        "network": (gm[:n_mlp], flat(g1[:-2])), "grid": (gm[n_mlp:], flat(g1[-2:-1])), "dinput": (dx.cpu().numpy(), g1[-1].detach().numpy()),
        "network_2nd": (gsm[:n_mlp], flat(g2[:-3])), "grid_2nd": (gsm[n_mlp:], flat(g2[-3:-2])),
        "ddLdoutput": (ddo.float().cpu().numpy(), g2[-2].numpy()), "dinput_2nd": (ddx.cpu().numpy(), g2[-1].numpy()),
    }
    met = {}
    for k, (a, b) in pairs.items():
        rel, cos = rel_cos(a, b)
        met[f"rel_{k}"], met[f"one_minus_cos_{k}"] = rel, 1 - cos
    record(f"grid_nd_mlp_{case}", ambiguous=amb.mean(), **met)
    print(f"case {case}:", {k: f"{val:.3e}" for k, val in met.items()})
    for k in pairs:
        assert met[f"rel_{k}"] <= 2e-3 and met[f"one_minus_cos_{k}"] <= 1e-5, (k, met)
    # the outputs alone (Ignore): bitwise the same; Accumulate adds
    ddo2 = t.full((N, 16), -3.0, dtype=t.float16, device="cuda")
    ddx2 = t.full((N, D), -3.0, dtype=t.float32, device="cuda")
    m.backward_backward_input(ctx, x, u, dlo_dev, params, dL_ddLdoutput=ddo2, mode=GradientMode.Ignore, dL_dinput=ddx2)
    assert t.equal(ddo2, ddo) and t.equal(ddx2, ddx)
    acc = g.clone()
    m.backward_backward_input(ctx, x, u, dlo_dev, params, dL_dparams=acc, mode=GradientMode.Accumulate)
    np.testing.assert_allclose(acc.cpu().numpy(), gm + gsm, rtol=1e-5, atol=2e-5 * max(1.0, np.abs(gm + gsm).max()))
