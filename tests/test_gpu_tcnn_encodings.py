"""neus2_amd.tcnn (importable as tinycudann) with the parameter-free encodings, B = 200: the colour-network pattern
(SphericalHarmonics on the view direction, concatenated in torch with features, into a Network) and the NeuS SDF pattern
(Frequency -> MLP under the eikonal loss of test_gpu_torch_modules.py), against float64 autograd with the modelling of
tests/bbi_ref.py at the project's fp16 bars (rel-L2 <= 2e-3, 1 - cosine <= 1e-5). The 200 inputs are the first of 256
candidates without a hidden pre-activation within 1e-4 of 0 (share of such candidates <= 0.05, by the reference alone)."""
import numpy as np
import pytest

import bbi_ref as R
import enc_ref as E
from test_gpu_enc_mlp import FREQ, SH4, _reference_graph
from test_gpu_torch_modules import _check, _eikonal

pytestmark = pytest.mark.gpu

B = 200
NET = {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 64, "n_hidden_layers": 2}


def _colour_graph(ph, dirs, feats, scale):
    import torch
    r16 = R.r16_fn(scale)
    mats = E.mlp_mats(ph, E.mlp_shapes(32, 64, 2))
    ft = torch.tensor(feats.astype(np.float64), requires_grad=True)
    e = r16(E.sh(torch.tensor(dirs.astype(np.float64)), 4))  # the encoding's fp16 output
    out, amb = E.mlp(r16(E.pad_ones(torch.cat([e, ft], dim=1))), mats, r16, R.AMBIGUOUS)
    return dict(ft=ft, leaves=mats, out=out, ambiguous=amb)


def test_colour_network_first_order(torch_cuda):
    import torch
    import tinycudann as tcnn
    enc = tcnn.Encoding(3, SH4)
    net = tcnn.Network(16 + 8, 3, NET)
    assert enc.n_input_dims == 3 and enc.n_output_dims == 16 and enc.dtype == torch.float16
    assert enc.params.numel() == 0 and enc.params.dtype == torch.float32
    rng = np.random.default_rng(41)
    ph = E.mlp_params(rng, E.mlp_shapes(32, 64, 2))
    assert net.params.numel() == ph.size
    d = rng.normal(size=(256, 3))
    d = ((d / np.linalg.norm(d, axis=1, keepdims=True) + 1) * 0.5).astype(np.float32)
    f = rng.uniform(-1, 1, (256, 8)).astype(np.float16).astype(np.float32)
    amb = _colour_graph(ph, d, f, 128.0)["ambiguous"]
    print(f"colour network: ambiguous share {amb.mean():.4f}")
    assert amb.mean() <= 0.05
    d, f = np.ascontiguousarray(d[~amb][:B]), np.ascontiguousarray(f[~amb][:B])
    with torch.no_grad():
        net.params.copy_(torch.from_numpy(ph.astype(np.float32)))
    dirs = torch.from_numpy(d).cuda()
    feats = torch.from_numpy(f).cuda().requires_grad_(True)
    sh = enc(dirs)
    assert sh.shape == (B, 16) and sh.dtype == torch.float16
    y = net(torch.cat([sh.float(), feats], dim=1))
    assert y.shape == (B, 3)
    (y.float() ** 2).mean().backward()
    assert enc.params.grad is None or enc.params.grad.numel() == 0
    ref = _colour_graph(ph, d, f, 128.0)
    grads = torch.autograd.grad((ref["out"][:, :3] ** 2).mean(), ref["leaves"] + [ref["ft"]])
    _check("tcnn_colour_network_sh4", {"params": net.params.grad.cpu().numpy(), "features": feats.grad.cpu().numpy()},
           {"params": R.flat(grads[:-1]), "features": grads[-1].numpy()})


def test_frequency_network_eikonal(torch_cuda):
    import torch
    import tinycudann as tcnn
    m = tcnn.NetworkWithInputEncoding(3, 1, FREQ, NET)
    assert m.n_output_dims == 1 and m.dtype == torch.float16 and m.loss_scale == 128.0
    rng = np.random.default_rng(43)
    ph = E.mlp_params(rng, E.mlp_shapes(32, 64, 2))
    assert m.params.numel() == ph.size
    cand = rng.uniform(0.02, 0.98, (256, 3)).astype(np.float32)
    amb = _reference_graph(ph, cand)["ambiguous"]
    print(f"frequency network: ambiguous share {amb.mean():.4f}")
    assert amb.mean() <= 0.05
    pos = np.ascontiguousarray(cand[~amb][:B])
    with torch.no_grad():
        m.params.copy_(torch.from_numpy(ph.astype(np.float32)))
    x = torch.from_numpy(pos).cuda().requires_grad_(True)
    y = m(x)
    assert y.shape == (B, 1) and y.dtype == torch.float16
    _eikonal(y.float(), x, torch).backward()
    ref = _reference_graph(ph, pos, scale=128.0)
    grads = torch.autograd.grad(_eikonal(ref["out"][:, :1], ref["xt"], torch), ref["leaves"] + [ref["xt"]])
    _check("tcnn_network_frequency", {"params": m.params.grad.cpu().numpy(), "x": x.grad.cpu().numpy()},
           {"params": R.flat(grads[:-1]), "x": grads[-1].numpy()})


@pytest.mark.parametrize("kind", ["encoding", "network"])
def test_second_order_through_sh_is_refused(torch_cuda, kind):
    import torch
    import tinycudann as tcnn
    m = tcnn.Encoding(3, SH4) if kind == "encoding" else tcnn.NetworkWithInputEncoding(3, 3, SH4, NET)
    assert not m._backend.supports_double_backward
    x = torch.from_numpy(np.random.default_rng(45).uniform(0.1, 0.9, (B, 3)).astype(np.float32)).cuda().requires_grad_(True)
    y = m(x).float()
    n, = torch.autograd.grad(y.sum(), x, create_graph=True)
    assert n.shape == (B, 3) and torch.isfinite(n).all()
    with pytest.raises(RuntimeError, match="not supported"):
        (n ** 2).sum().backward()


def test_empty_params_and_optimizer_step(torch_cuda):
    import torch
    import tinycudann as tcnn
    for cfg, n_in, w in ((SH4, 3, 16), (FREQ, 2, 16), ({"otype": "Identity"}, 5, 5)):
        m = tcnn.Encoding(n_in, cfg)
        assert m.params.numel() == 0 and m.n_output_dims == w and len(list(m.parameters())) == 1
        opt = torch.optim.Adam(m.parameters(), lr=1e-2)
        x = torch.from_numpy(np.random.default_rng(47).uniform(0, 1, (B, n_in)).astype(np.float32)).cuda().requires_grad_(True)
        y = m(x)
        assert y.shape == (B, w)
        y.float().sum().backward()
        assert x.grad is not None and torch.isfinite(x.grad).all()
        opt.step()
        assert m.params.numel() == 0
        with torch.no_grad():
            assert torch.equal(m(x.detach()), y.detach())
    # the Frequency encoding supports the double backward
    assert tcnn.Encoding(3, FREQ)._backend.supports_double_backward


def test_sigmoid_output_colour_network_backward(torch_cuda):
    """The colour network's usual output activation: the first backward hands the forward's output to the native module
    (it raised "the forward output is needed" before) and equals the Module-level backward bitwise."""
    import torch
    import tinycudann as tcnn
    from neus2_amd.module import GradientMode
    cfg = dict(NET, output_activation="Sigmoid")
    net = tcnn.Network(16 + 8, 3, cfg)
    enc = tcnn.Encoding(3, SH4)
    rng = np.random.default_rng(49)
    d = torch.from_numpy(rng.uniform(0, 1, (256, 3)).astype(np.float32)).cuda()
    f = torch.from_numpy(rng.uniform(-1, 1, (256, 8)).astype(np.float32)).cuda()
    h = torch.cat([enc(d).float(), f], dim=1).detach().requires_grad_(True)
    y = net(h)
    assert y.shape == (256, 3) and (y > 0).all() and (y < 1).all()
    w = torch.from_numpy(rng.normal(0, 1, (256, 3)).astype(np.float32)).cuda()
    (y.float() * w).sum().backward()
    assert torch.isfinite(net.params.grad).all() and net.params.grad.abs().sum().item() > 0
    m = net._backend.m
    p16 = net.params.detach().half().contiguous()
    ctx, y_m = m.forward(h.detach().contiguous(), p16, prepare_input_gradients=True)
    assert torch.equal(y_m[:, :3], y.detach())
    dlo = torch.zeros((256, 16), dtype=torch.float16, device="cuda")
    dlo[:, :3] = (w.half().float() * net.loss_scale).half()  # the cotangent reaches the module through the fp16 output
    g = m.gradient_buffer()
    dx = torch.zeros((256, 24), dtype=torch.float32, device="cuda")
    m.backward(ctx, h.detach().contiguous(), dlo, p16, dL_dparams=g, dL_dinput=dx, mode=GradientMode.Overwrite, output=y_m)
    assert torch.equal(net.params.grad, g / net.loss_scale) and torch.equal(h.grad, dx / net.loss_scale)
