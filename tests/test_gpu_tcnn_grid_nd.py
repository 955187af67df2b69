"""The general grid encoding through the PyTorch modules (`import tinycudann as tcnn`), B = 200: a 2-D hash grid encoding,
a 2-D Smoothstep grid network to first order, a 3-D Smoothstep grid network under the eikonal loss of
test_gpu_torch_modules.py (params.grad and x.grad need all three backward_backward_input outputs, and with Smoothstep the
grid's diagonal second derivatives), and one Adam step. References: tests/grid_nd_ref.grid_network with the loss scale 128
the modules apply; bars: the project's fp16 bars, rel-L2 <= 2e-3 and 1 - cosine <= 1e-5. The 200 inputs are the first of 256
candidates away from the cell borders and without a hidden pre-activation within 1e-4 of 0 (share left out <= 0.05 each)."""
import numpy as np
import pytest

import grid_nd_ref as G
from bbi_ref import flat, rel_cos
from test_gpu_grid_nd import CASES, MARGIN, config, record, tables

pytestmark = pytest.mark.gpu

B = 200
W, NH = 64, 2
NET = {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": W, "n_hidden_layers": NH}


def _shapes(case):
    D, F, ty, ip, L, *_ = CASES[case]
    return [(W, (F * L + 15) // 16 * 16), (W, W), (16, W)]


def _params(case, rng):
    D, F, ty, ip, L, *_ = CASES[case]
    off, _ = tables(case)
    return G.network_params(rng, _shapes(case), F * L, D, off[-1] * F)


def _network(case, ph, pos, scale=1.0, interpolation=None):
    D, F, ty, ip, L, *_ = CASES[case]
    off, res = tables(case)
    return G.grid_network(ph, pos, _shapes(case), off, res, F, ty, interpolation or ip, scale)


def _select(case, ph, rng):
    D = CASES[case][0]
    _, res = tables(case)
    cand = rng.uniform(0.02, 0.98, (256, D)).astype(np.float32)
    border = G.fraction_margin(cand, res) < MARGIN
    amb = _network(case, ph, cand)["ambiguous"]
    print(f"case {case}: near a cell border {border.mean():.4f}, ambiguous {amb.mean():.4f}")
    assert border.mean() <= 0.05 and amb.mean() <= 0.05
    pos = np.ascontiguousarray(cand[~(border | amb)][:B])
    assert pos.shape[0] == B
    return pos


def _eikonal(y, x, torch):
    n, = torch.autograd.grad(y.sum(), x, create_graph=True)
    return ((n.norm(dim=1) - 1) ** 2).mean() + (y ** 2).mean()


def _check(tag, got, ref):
    out = {}
    for k in got:
        rel, cos = rel_cos(got[k], ref[k])
        out[f"rel_{k}"], out[f"one_minus_cos_{k}"] = rel, 1 - cos
    record(tag, **out)
    print(tag, {k: f"{v:.3e}" for k, v in out.items()})
    for k in got:
        assert out[f"rel_{k}"] <= 2e-3 and out[f"one_minus_cos_{k}"] <= 1e-5, (k, out)


def test_encoding_2d(torch_cuda):
    import torch
    import tinycudann as tcnn
    D, F, ty, ip, L, *_ = CASES["A"]
    off, res = tables("A")
    m = tcnn.Encoding(2, config("A"))
    assert m.n_input_dims == 2 and m.n_output_dims == F * L and m.dtype == torch.float16
    assert m.params.dtype == torch.float32 and m.params.numel() == off[-1] * F
    assert m._backend.supports_double_backward
    rng = np.random.default_rng(31)
    table = rng.uniform(-1, 1, (off[-1], F)).astype(np.float16)
    with torch.no_grad():
        m.params.copy_(torch.from_numpy(table.ravel().astype(np.float32)))
    pos = rng.uniform(0.02, 0.98, (B, 2)).astype(np.float32)
    with torch.no_grad():
        y = m(torch.from_numpy(pos).cuda())
    assert y.shape == (B, F * L) and y.dtype == torch.float16
    ref = G.grid_encode(torch.tensor(pos.astype(np.float64)), torch.tensor(table.astype(np.float64)), off, res, ty, ip).numpy()
    assert np.abs(y.float().cpu().numpy() - ref).max() <= 2.0 ** -10  # values in +-1: one fp16 rounding and the fp32 error


def test_network_2d_smoothstep_first_order(torch_cuda):
    import torch
    import tinycudann as tcnn
    case = "B"
    m = tcnn.NetworkWithInputEncoding(2, 3, config(case), NET)
    assert m.n_output_dims == 3 and m.dtype == torch.float16 and m._backend.supports_double_backward
    rng = np.random.default_rng(33)
    ph = _params(case, rng)
    assert m.params.numel() == ph.size
    pos = _select(case, ph, rng)
    with torch.no_grad():
        m.params.copy_(torch.from_numpy(ph.astype(np.float32)))
    x = torch.from_numpy(pos).cuda().requires_grad_(True)
    y = m(x)
    assert y.shape == (B, 3) and y.dtype == torch.float16
    (y.float() ** 2).mean().backward()
    ref = _network(case, ph, pos, scale=128.0)
    rel, cos = rel_cos(y.detach().float().cpu().numpy(), ref["out"][:, :3].detach().numpy())
    assert rel <= 2e-3 and 1 - cos <= 1e-5, (rel, cos)
    grads = torch.autograd.grad((ref["out"][:, :3] ** 2).mean(), ref["leaves"] + [ref["xt"]])
    _check("tcnn_grid_nd_B_first_order", {"params": m.params.grad.cpu().numpy(), "x": x.grad.cpu().numpy()},
           {"params": flat(grads[:-1]), "x": grads[-1].numpy()})


def test_network_3d_smoothstep_eikonal(torch_cuda):
    import torch
    import tinycudann as tcnn
    case = "E"
    F = CASES[case][1]
    off, _ = tables(case)
    n_mlp = sum(r * k for r, k in _shapes(case))
    rng = np.random.default_rng(35)
    ph = _params(case, rng)
    pos = _select(case, ph, rng)
    grads = {}
    for ip in ("Smoothstep", "Linear"):
        m = tcnn.NetworkWithInputEncoding(3, 1, config(case, interpolation=ip), NET)
        assert m.params.numel() == ph.size == n_mlp + off[-1] * F
        with torch.no_grad():
            m.params.copy_(torch.from_numpy(ph.astype(np.float32)))
        x = torch.from_numpy(pos).cuda().requires_grad_(True)
        _eikonal(m(x).float(), x, torch).backward()
        grads[ip] = (m.params.grad.cpu().numpy(), x.grad.cpu().numpy())
    ref = _network(case, ph, pos, scale=128.0)
    rg = torch.autograd.grad(_eikonal(ref["out"][:, :1], ref["xt"], torch), ref["leaves"] + [ref["xt"]])
    _check("tcnn_grid_nd_E_eikonal", {"params": grads["Smoothstep"][0], "x": grads["Smoothstep"][1]},
           {"params": flat(rg[:-1]), "x": rg[-1].numpy()})
    # the Smoothstep terms are live: the grid block's gradient is not the Linear run's
    rel, _ = rel_cos(grads["Smoothstep"][0][n_mlp:], grads["Linear"][0][n_mlp:])
    print(f"grid gradient, Smoothstep vs Linear: rel {rel:.3e}")
    assert rel > 0.05


def test_adam_step_changes_the_table(torch_cuda):
    import torch
    import tinycudann as tcnn
    case = "B"
    m = tcnn.NetworkWithInputEncoding(2, 3, config(case), NET, seed=5)
    n_mlp = sum(r * k for r, k in _shapes(case))
    before = m.params.detach().clone()
    opt = torch.optim.Adam(m.parameters(), lr=1e-2)
    x = torch.from_numpy(np.random.default_rng(37).uniform(0.05, 0.95, (B, 2)).astype(np.float32)).cuda().requires_grad_(True)
    y = m(x).float()
    target = torch.sin(6.0 * x.detach()).sum(dim=1, keepdim=True).expand(-1, 3)
    n, = torch.autograd.grad(y.sum(), x, create_graph=True)
    loss = ((y - target) ** 2).mean() + 0.1 * ((n.norm(dim=1) - 1) ** 2).mean()
    loss.backward()
    opt.step()
    assert torch.isfinite(m.params).all()
    changed = (m.params.detach() != before)
    assert changed[n_mlp:].any().item() and changed[:n_mlp].any().item()
