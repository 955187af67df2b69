"""neus2_amd.tcnn with a 256-wide CutlassMLP behind the HashGrid: the eikonal step of test_gpu_tcnn_second_order.py,
    y = m(x); n = grad(y.sum(), x, create_graph=True); loss = ((n.norm(dim=1) - 1)^2).mean(); loss.backward()
through ffmlp.hip's wide kernels (before, the module refused the width at construction). params.grad and x.grad are held
against float64 autograd on the unrounded network by the same rule: rel-L2 <= 4 floor, the floor being the fp16-storage
model's own distance from the truth for these inputs, and never beyond rel-L2 2e-2 / cosine 0.999."""
import numpy as np
import pytest

import act_ref as A
import bbi_ref as R

pytestmark = pytest.mark.gpu

B, W = 200, 256
NET = {"otype": "CutlassMLP", "activation": "Softplus", "output_activation": "None", "n_neurons": W, "n_hidden_layers": 2}
SHAPES = [(W, 16), (W, W), (16, W)]
N_MLP = sum(r * k for r, k in SHAPES)


def _reference(ph, pos, rounded):
    """(dL/dparams, dL/dx) of the eikonal loss in float64: rounded = the device's model, else autograd on the whole graph"""
    import torch
    from torch_ref import hash_grid
    enc = lambda x, tab: hash_grid(x, tab, R.OFF, R.RES)
    pd = torch.tensor(ph.astype(np.float64))
    mats, o = [], 0
    for r, k in SHAPES:
        mats.append(pd[o:o + r * k].reshape(r, k))
        o += r * k
    table = pd[o:].reshape(-1, 2)
    x = torch.tensor(pos.astype(np.float64))
    if not rounded:
        xt, tab = x.clone().requires_grad_(True), table.clone().requires_grad_(True)
        ms = [m.clone().requires_grad_(True) for m in mats]
        y = A.network(ms, A.rows(enc(xt, tab), 0.0), "Softplus", "None")[:, :1]
        n, = torch.autograd.grad(y.sum(), xt, create_graph=True)
        gr = torch.autograd.grad(((n.norm(dim=1) - 1) ** 2).mean(), ms + [tab, xt])
        return R.flat(gr[:-1]), gr[-1].numpy()
    g = torch.zeros(B, 16, dtype=torch.float64)
    g[:, 0] = 1.0
    n = A.input_gradient(enc, x, table, mats, g, "Softplus", "None", 0.0, True)
    nn = n.norm(dim=1, keepdim=True)
    u = (2.0 / B) * (nn - 1) * n / nn  # dL/dn, as autograd hands it to the double backward (fp32 on the device)
    out = A.bbi(enc, x, table, u, mats, g, "Softplus", "None", 0.0, True)
    return R.flat(out["dW"] + [out["dtable"]]), out["dx"].numpy()


def _held(tag, got, truth, model):
    floor = A.rel(model, truth)
    rel, cos = R.rel_cos(got, truth)
    R.record(tag, rel=rel, one_minus_cos=1 - cos, floor=floor)
    print(f"{tag}: rel {rel:.3e} floor {floor:.3e} 1-cos {1 - cos:.3e}")
    return rel <= min(4.0 * floor, 2e-2) and cos >= 0.999, (tag, rel, floor, cos)


def test_cutlass_softplus_eikonal_step(torch_cuda):
    import torch
    from neus2_amd import tcnn
    m = tcnn.NetworkWithInputEncoding(3, 1, R.ENC_CFG, NET)
    hyper = m._backend.m.hyperparams()["network"]
    assert m._backend.supports_double_backward and hyper["second_order"] == "exact" and hyper["otype"] == "CutlassMLP" and hyper["n_neurons"] == W
    rng = np.random.default_rng(71)
    ph = np.concatenate([rng.normal(0, 1.2 / np.sqrt(k), (r, k)).ravel() for r, k in SHAPES] + [rng.uniform(-1, 1, R.N_GRID)]).astype(np.float16)
    assert m.params.numel() == ph.size == N_MLP + R.N_GRID
    pos = rng.uniform(0.02, 0.98, (B, 3)).astype(np.float32)
    with torch.no_grad():
        m.params.copy_(torch.from_numpy(ph.astype(np.float32)))
    x = torch.from_numpy(pos).cuda().requires_grad_(True)
    y = m(x).float()
    assert y.shape == (B, 1)
    n, = torch.autograd.grad(y.sum(), x, create_graph=True)
    ((n.norm(dim=1) - 1) ** 2).mean().backward()
    gp, gx = m.params.grad.cpu().numpy(), x.grad.cpu().numpy()
    assert np.isfinite(gp).all() and np.isfinite(gx).all() and np.abs(gp).max() > 0 and np.abs(gx).max() > 0
    (tp, tx), (mp, mx) = _reference(ph, pos, False), _reference(ph, pos, True)
    results = [_held("tcnn_cutlass_eikonal_params", gp, tp, mp), _held("tcnn_cutlass_eikonal_x", gx, tx, mx)]
    assert all(ok for ok, _ in results), results


def test_network_takes_a_wide_cutlass_mlp(torch_cuda):
    """tcnn.Network passes the config through: a 512-wide network runs forward and backward"""
    import torch
    from neus2_amd import tcnn
    net = tcnn.Network(8, 3, dict(NET, activation="ReLU", n_neurons=512, n_hidden_layers=1))
    x = torch.from_numpy(np.random.default_rng(73).uniform(-1, 1, (B, 8)).astype(np.float32)).cuda().requires_grad_(True)
    y = net(x).float()
    assert y.shape == (B, 3)
    (y ** 2).sum().backward()
    assert torch.isfinite(net.params.grad).all() and net.params.grad.abs().sum().item() > 0
    assert torch.isfinite(x.grad).all() and x.grad.abs().sum().item() > 0
