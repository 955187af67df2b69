"""neus2_amd.tcnn with a Softplus network: the eikonal loss of an SDF written in PyTorch,
    y = m(x); n = grad(y.sum(), x, create_graph=True); loss = ((n.norm(dim=1) - 1)^2).mean(); loss.backward()
needs the exact double backward (the act'' terms), which the modules now create their networks with; before, the backward
raised "double backward is not supported". params.grad and x.grad are held against float64 autograd on the unrounded
network by the rule of test_gpu_ffmlp_second_order.py: rel-L2 <= 4 floor, the floor being the fp16-storage model's own
distance from the truth for these inputs, and never beyond rel-L2 2e-2 / cosine 0.999. Also: twenty Adam steps lower the
eikonal term, a Sigmoid output double-backwards, and SphericalHarmonics in front is still refused."""
import numpy as np
import pytest

import act_ref as A
import bbi_ref as R

pytestmark = pytest.mark.gpu

B = 200
NET = {"otype": "FullyFusedMLP", "activation": "Softplus", "output_activation": "None", "n_neurons": 16, "n_hidden_layers": 2}
SHAPES = [(16, 16), (16, 16), (16, 16)]


def _reference(ph, pos, rounded):
    """(dL/dparams, dL/dx) of the eikonal loss in float64: rounded = the device's model, else autograd on the whole graph"""
    import torch
    from torch_ref import hash_grid
    enc = lambda x, tab: hash_grid(x, tab, R.OFF, R.RES)
    pd = torch.tensor(ph.astype(np.float64))
    mats = [pd[256 * i:256 * (i + 1)].reshape(16, 16) for i in range(3)]
    table = pd[768:].reshape(-1, 2)
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


def test_softplus_eikonal_step(torch_cuda):
    import torch
    from neus2_amd import tcnn
    m = tcnn.NetworkWithInputEncoding(3, 1, R.ENC_CFG, NET)
    assert m._backend.supports_double_backward and m._backend.m.hyperparams()["network"]["second_order"] == "exact"
    rng = np.random.default_rng(61)
    ph = R.net_params("gridmlp", rng)
    assert m.params.numel() == ph.size
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
    results = [_held("tcnn_softplus_eikonal_params", gp, tp, mp), _held("tcnn_softplus_eikonal_x", gx, tx, mx)]
    assert all(ok for ok, _ in results), results


def test_softplus_eikonal_training(torch_cuda):
    """twenty Adam steps of eikonal + y^2 on a fixed batch lower the eikonal term (no rate is claimed)"""
    import torch
    from neus2_amd import tcnn
    m = tcnn.NetworkWithInputEncoding(3, 1, R.ENC_CFG, NET, seed=7)
    rng = np.random.default_rng(63)
    with torch.no_grad():
        m.params.copy_(torch.from_numpy(R.net_params("gridmlp", rng).astype(np.float32)))
    opt = torch.optim.Adam(m.parameters(), lr=1e-2)
    pos = torch.from_numpy(rng.uniform(0.05, 0.95, (B, 3)).astype(np.float32)).cuda()
    eik = []
    for _ in range(20):
        x = pos.clone().requires_grad_(True)
        y = m(x).float()
        n, = torch.autograd.grad(y.sum(), x, create_graph=True)
        e = ((n.norm(dim=1) - 1) ** 2).mean()
        opt.zero_grad()
        (e + (y ** 2).mean()).backward()
        opt.step()
        eik.append(e.item())
    print(f"eikonal term: {eik[0]:.4f} -> {eik[-1]:.4f}")
    assert np.isfinite(eik).all() and torch.isfinite(m.params).all()
    assert eik[-1] < eik[0]


def test_sigmoid_output_double_backward(torch_cuda):
    import torch
    from neus2_amd import tcnn
    net = tcnn.Network(8, 3, dict(NET, activation="ReLU", output_activation="Sigmoid", n_neurons=64, n_hidden_layers=1))
    assert net._backend.supports_double_backward
    x = torch.from_numpy(np.random.default_rng(65).uniform(-1, 1, (B, 8)).astype(np.float32)).cuda().requires_grad_(True)
    n, = torch.autograd.grad(net(x).float().sum(), x, create_graph=True)
    (n ** 2).sum().backward()
    assert torch.isfinite(net.params.grad).all() and net.params.grad.abs().sum().item() > 0
    assert torch.isfinite(x.grad).all() and x.grad.abs().sum().item() > 0  # zeros without the output's act'' term


def test_spherical_harmonics_in_front_is_still_refused(torch_cuda):
    import torch
    from neus2_amd import tcnn
    m = tcnn.NetworkWithInputEncoding(3, 1, {"otype": "SphericalHarmonics", "degree": 2}, NET)
    assert not m._backend.supports_double_backward
    x = torch.from_numpy(np.random.default_rng(67).uniform(0.1, 0.9, (B, 3)).astype(np.float32)).cuda().requires_grad_(True)
    n, = torch.autograd.grad(m(x).float().sum(), x, create_graph=True)
    with pytest.raises(RuntimeError, match="not supported"):
        (n ** 2).sum().backward()
