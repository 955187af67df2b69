"""neus2_amd.tcnn on the GPU: an eikonal-shaped loss written in PyTorch,
    y = m(x); n = grad(y.sum(), x, create_graph=True); loss = ((n.norm(dim=1) - 1)^2).mean() + (y^2).mean(); loss.backward()
whose params.grad and x.grad need all three outputs' worth of backward_backward_input, against the float64 references of
tests/bbi_ref.py (the same modelling and bars as test_gpu_bbi_full.py: fp16 modules rel-L2 <= 2e-3 and cosine >= 0.99999,
the fp32 encoding <= 3e-5), B = 200 on the 4-level grid. For the networks the 200 inputs are the first of 256 candidates
without a hidden pre-activation within 1e-4 of 0 (share of such candidates <= 0.05), decided by the reference alone.
Also: Network's first-order gradients, the batch-capacity regrowth, the `tinycudann` name, and 100 Adam steps on a sphere
SDF with the eikonal term (a wiring guard against a misplaced loss scale, not a quality bar)."""
import numpy as np
import pytest

import bbi_ref as R

pytestmark = pytest.mark.gpu

B = 200


def _eikonal(y, x, torch):
    n, = torch.autograd.grad(y.sum(), x, create_graph=True)
    return ((n.norm(dim=1) - 1) ** 2).mean() + (y ** 2).mean()


def _check(tag, got, ref, f32=False):
    out = {}
    for k in got:
        rel, cos = R.rel_cos(got[k], ref[k])
        out[f"rel_{k}"], out[f"one_minus_cos_{k}"] = rel, 1 - cos
    R.record(tag, **out)
    print(tag, {k: f"{v:.3e}" for k, v in out.items()})
    for k in got:
        if f32:
            assert out[f"rel_{k}"] <= 3e-5, (k, out)
        else:
            assert out[f"rel_{k}"] <= 2e-3 and out[f"one_minus_cos_{k}"] <= 1e-5, (k, out)


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_encoding_eikonal(torch_cuda, precision):
    import torch
    from neus2_amd import tcnn
    f32 = precision == "fp32"
    m = tcnn.Encoding(3, R.ENC_CFG, dtype=torch.float32 if f32 else None)
    assert m.n_input_dims == 3 and m.n_output_dims == 2 * R.L and m.params.dtype == torch.float32 and m.params.numel() == R.N_GRID
    assert m.dtype == (torch.float32 if f32 else torch.float16) and m.loss_scale == (1.0 if f32 else 128.0)
    p0 = m.params.detach().cpu().numpy()
    assert 0 < np.abs(p0).max() <= 1e-4  # GridEncoding::initialize_params
    rng = np.random.default_rng(21)
    ph = rng.uniform(-1, 1, R.N_GRID).astype(np.float32 if f32 else np.float16)
    pos = rng.uniform(0.02, 0.98, (B, 3)).astype(np.float32)
    with torch.no_grad():
        m.params.copy_(torch.from_numpy(ph.astype(np.float32)))
    x = torch.from_numpy(pos).cuda().requires_grad_(True)
    y = m(x)
    assert y.shape == (B, 2 * R.L) and y.dtype == m.dtype
    _eikonal(y.float(), x, torch).backward()
    tab = torch.tensor(ph.astype(np.float64).reshape(-1, 2), requires_grad=True)
    xt = torch.tensor(pos.astype(np.float64), requires_grad=True)
    e = R.hash_grid(xt, tab, R.OFF, R.RES)
    if not f32:
        e = R.r16_fn(128.0)(e + (torch.tensor(R.oracle_features(ph, pos)) - e).detach())
    gt, gx = torch.autograd.grad(_eikonal(e, xt, torch), [tab, xt])
    _check(f"tcnn_encoding_{precision}", {"params": m.params.grad.cpu().numpy(), "x": x.grad.cpu().numpy()},
           {"params": gt.numpy(), "x": gx.numpy()}, f32)


def _select(name, ph, rng):
    """The first B of 256 candidate inputs without an ambiguous ReLU (by the float64 reference alone)."""
    cand = rng.uniform(0.02, 0.98, (256, 3)).astype(np.float32)
    amb = R.network(name, ph, cand)["ambiguous"]
    print(f"{name}: ambiguous share {amb.mean():.4f}")
    assert amb.mean() <= 0.05
    return np.ascontiguousarray(cand[~amb][:B])


@pytest.mark.parametrize("name", ["dnet", "gridmlp"])
def test_network_with_input_encoding_eikonal(torch_cuda, name):
    import torch
    from neus2_amd import tcnn
    _, W, NH, n_out = R.NETS[name]
    m = tcnn.NetworkWithInputEncoding(3, n_out, R.ENC_CFG, R.net_cfg(name))
    assert m.n_output_dims == n_out and m.dtype == torch.float16 and m.loss_scale == 128.0
    rng = np.random.default_rng(23)
    ph = R.net_params(name, rng, 0.3 if name == "dnet" else None)
    assert m.params.numel() == ph.size
    pos = _select(name, ph, rng)
    with torch.no_grad():
        m.params.copy_(torch.from_numpy(ph.astype(np.float32)))
    x = torch.from_numpy(pos).cuda().requires_grad_(True)
    y = m(x)
    assert y.shape == (B, n_out) and y.dtype == torch.float16
    _eikonal(y.float(), x, torch).backward()
    ref = R.network(name, ph, pos, scale=128.0)
    grads = torch.autograd.grad(_eikonal(ref["out"][:, :n_out], ref["xt"], torch), ref["leaves"] + [ref["xt"]])
    _check(f"tcnn_network_{name}", {"params": m.params.grad.cpu().numpy(), "x": x.grad.cpu().numpy()},
           {"params": R.flat(grads[:-1]), "x": grads[-1].numpy()})


def test_network_first_order(torch_cuda):
    import torch
    from neus2_amd import tcnn
    m = tcnn.Network(3, 1, R.net_cfg("mlp"))
    rng = np.random.default_rng(25)
    ph = R.net_params("mlp", rng)
    pos = _select("mlp", ph, rng)
    with torch.no_grad():
        m.params.copy_(torch.from_numpy(ph.astype(np.float32)))
    x = torch.from_numpy(pos).cuda().requires_grad_(True)
    y = m(x)
    assert y.shape == (B, 1) and y.dtype == torch.float16
    (y.float() ** 2).mean().backward()
    ref = R.network("mlp", ph, pos, scale=128.0)
    grads = torch.autograd.grad((ref["out"][:, :1] ** 2).mean(), ref["leaves"] + [ref["xt"]])
    _check("tcnn_network_mlp_first_order", {"params": m.params.grad.cpu().numpy(), "x": x.grad.cpu().numpy()},
           {"params": R.flat(grads[:-1]), "x": grads[-1].numpy()})


def test_batch_capacity_regrowth(torch_cuda, monkeypatch):
    """B = 200 then B = 1000 on a module created for 256 rows: the native module is re-created larger, the rows both
    batches share are bitwise equal, and a graph recorded before the regrowth still runs its backward."""
    import torch
    from neus2_amd import tcnn
    monkeypatch.setattr(tcnn, "INITIAL_BATCH_CAPACITY", 256)
    m = tcnn.NetworkWithInputEncoding(3, 1, R.ENC_CFG, R.net_cfg("dnet"))
    rng = np.random.default_rng(27)
    with torch.no_grad():
        m.params.copy_(torch.from_numpy(R.net_params("dnet", rng, 0.3).astype(np.float32)))
    x = torch.from_numpy(rng.uniform(0.02, 0.98, (1000, 3)).astype(np.float32)).cuda()
    be0 = m._backend
    assert be0.batch_capacity == 256
    xs = x[:B].clone().requires_grad_(True)
    y0 = m(xs)
    assert m._backend is be0
    y1 = m(x)
    assert m._backend is not be0 and m._backend.batch_capacity >= 1024 and y1.shape == (1000, 1)
    np.testing.assert_array_equal(y1[:B].detach().cpu().numpy().view(np.uint16), y0.detach().cpu().numpy().view(np.uint16))
    y0.float().sum().backward()
    g0, gx0 = m.params.grad.clone(), xs.grad.clone()
    m.params.grad = None
    xs2 = x[:B].clone().requires_grad_(True)
    m(xs2).float().sum().backward()
    np.testing.assert_array_equal(m.params.grad.cpu().numpy(), g0.cpu().numpy())
    np.testing.assert_array_equal(xs2.grad.cpu().numpy(), gx0.cpu().numpy())
    with torch.no_grad():
        y2 = m(x[:1])
    assert y2.shape == (1, 1)


def test_tinycudann_name(torch_cuda):
    import tinycudann as tcnn
    from neus2_amd import tcnn as native
    assert tcnn.Encoding is native.Encoding and tcnn.Network is native.Network
    assert tcnn.NetworkWithInputEncoding is native.NetworkWithInputEncoding


def test_sphere_sdf_fit(torch_cuda):
    """100 Adam steps on a sphere SDF with the eikonal term from the module's own initialisation: finite parameters and a
    loss below the first step's."""
    import pickle
    import torch
    from neus2_amd import tcnn
    m = tcnn.NetworkWithInputEncoding(3, 1, R.ENC_CFG, R.net_cfg("dnet"), seed=7)
    opt = torch.optim.Adam(m.parameters(), lr=1e-2)
    rng = np.random.default_rng(29)
    losses = []
    for _ in range(100):
        x = torch.from_numpy(rng.uniform(0.05, 0.95, (B, 3)).astype(np.float32)).cuda().requires_grad_(True)
        target = (x.detach() - 0.5).norm(dim=1, keepdim=True) - 0.3
        y = m(x).float()
        n, = torch.autograd.grad(y.sum(), x, create_graph=True)
        loss = ((y - target) ** 2).mean() + 0.1 * ((n.norm(dim=1) - 1) ** 2).mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    print(f"sphere fit: loss {losses[0]:.4f} -> {losses[-1]:.4f}")
    assert torch.isfinite(m.params).all() and np.isfinite(losses).all()
    assert losses[-1] < losses[0]
    # pickling leaves the native handle behind and the copy works
    m2 = pickle.loads(pickle.dumps(m))
    assert m2._backend is None
    with torch.no_grad():
        xa = torch.from_numpy(rng.uniform(0.05, 0.95, (B, 3)).astype(np.float32)).cuda()
        np.testing.assert_array_equal(m2(xa).cpu().numpy().view(np.uint16), m(xa).cpu().numpy().view(np.uint16))
