"""neus2_amd.tcnn with a SIREN: tcnn.Network(3, 1, CutlassMLP / Sine, 256 neurons, 2 hidden layers) under the eikonal loss of
an SDF written in PyTorch,
    y = m(x); n = grad(y.sum(), x, create_graph=True); loss = ((n.norm(dim=1) - 1)^2).mean(); loss.backward()
Before the CutlassMLP took Sine the construction raised "Sine has no backward". params.grad and x.grad are held against
float64 autograd on the unrounded network by the rule of test_gpu_ffmlp_second_order.py: rel-L2 <= 4 floor, the floor being
the fp16-storage model's own distance from the truth for these inputs (tests/siren_ref.py), never beyond rel-L2 2e-2 /
cosine 0.999. The parameters are initialize_params(seed) as drawn. Also: twenty Adam steps lower the eikonal term."""
import numpy as np
import pytest

import act_ref as A
import bbi_ref as R
import siren_ref as S

pytestmark = pytest.mark.gpu

B = 200
NET = {"otype": "CutlassMLP", "activation": "Sine", "n_neurons": 256, "n_hidden_layers": 2}
SHAPES = [(256, 16), (256, 256), (16, 256)]
SEED = 71


def _reference(ph, pos, rounded):
    """(dL/dparams, dL/dx) of the eikonal loss in float64: rounded = the device's model, else autograd on the whole graph"""
    import torch
    pd = torch.tensor(ph.astype(np.float64))
    mats, o = [], 0
    for r, k in SHAPES:
        mats.append(pd[o:o + r * k].reshape(r, k))
        o += r * k
    x = torch.tensor(pos.astype(np.float64))
    if not rounded:
        xt = x.clone().requires_grad_(True)
        ms = [m.clone().requires_grad_(True) for m in mats]
        y = S.network(ms, A.rows(xt, 1.0))[:, :1]
        n, = torch.autograd.grad(y.sum(), xt, create_graph=True)
        gr = torch.autograd.grad(((n.norm(dim=1) - 1) ** 2).mean(), ms + [xt])
        return R.flat(gr[:-1]), gr[-1].numpy()
    g = torch.zeros(B, 16, dtype=torch.float64)
    g[:, 0] = 1.0
    enc = lambda v, tab: v
    n = S.model(enc, x, None, torch.zeros_like(x), mats, g, 1.0, True)["dx1"]
    nn = n.norm(dim=1, keepdim=True)
    u = (2.0 / B) * (nn - 1) * n / nn  # dL/dn, as autograd hands it to the double backward (fp32 on the device)
    out = S.model(enc, x, None, u, mats, g, 1.0, True)
    return R.flat(out["dW"]), out["dx"].numpy()


def _held(tag, got, truth, model):
    floor = A.rel(model, truth)
    rel, cos = R.rel_cos(got, truth)
    R.record(tag, rel=rel, one_minus_cos=1 - cos, floor=floor)
    print(f"{tag}: rel {rel:.3e} floor {floor:.3e} 1-cos {1 - cos:.3e}")
    return floor <= 5e-3 and rel <= min(4.0 * floor, 2e-2) and cos >= 0.999, (tag, rel, floor, cos)


def _siren(seed):
    import torch
    from neus2_amd import tcnn
    m = tcnn.Network(3, 1, NET, seed=seed)
    ph = S.initialize_params(seed, SHAPES).astype(np.float16)
    assert m.params.numel() == ph.size
    with torch.no_grad():  # initialize_params(seed) as drawn (test_gpu_siren.py pins the device's against the restatement), in fp16
        m.params.copy_(torch.from_numpy(ph.astype(np.float32)))
    return m, ph


def test_siren_eikonal_step(torch_cuda):
    import torch
    m, ph = _siren(SEED)
    net = m._backend.m.hyperparams()["network"]
    assert m._backend.supports_double_backward and net["otype"] == "CutlassMLP" and net["activation"] == "Sine" and net["second_order"] == "exact"
    rng = np.random.default_rng(SEED)
    pos = rng.uniform(-1, 1, (B, 3)).astype(np.float16).astype(np.float32)  # the Identity encoding reads fp16
    x = torch.from_numpy(pos).cuda().requires_grad_(True)
    y = m(x).float()
    assert y.shape == (B, 1)
    n, = torch.autograd.grad(y.sum(), x, create_graph=True)
    ((n.norm(dim=1) - 1) ** 2).mean().backward()
    gp, gx = m.params.grad.cpu().numpy(), x.grad.cpu().numpy()
    assert np.isfinite(gp).all() and np.isfinite(gx).all() and np.abs(gp).max() > 0 and np.abs(gx).max() > 0
    (tp, tx), (mp, mx) = _reference(ph, pos, False), _reference(ph, pos, True)
    results = [_held("tcnn_siren_eikonal_params", gp, tp, mp), _held("tcnn_siren_eikonal_x", gx, tx, mx)]
    assert all(ok for ok, _ in results), results


def test_siren_eikonal_training(torch_cuda):
    """twenty Adam steps of eikonal + y^2 on a fixed batch lower the eikonal term (no rate is claimed)"""
    import torch
    m, _ = _siren(SEED + 1)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    pos = torch.from_numpy(np.random.default_rng(SEED + 1).uniform(-1, 1, (B, 3)).astype(np.float32)).cuda()
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
    R.record("tcnn_siren_eikonal_training", start=eik[0], end=eik[-1])
    assert np.isfinite(eik).all() and torch.isfinite(m.params).all()
    assert eik[-1] < eik[0]
