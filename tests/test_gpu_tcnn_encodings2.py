"""neus2_amd.tcnn (importable as tinycudann) with the OneBlob, TriangleWave and NRC encodings, B = 200: OneBlob in front of a
Softplus network under the eikonal loss of test_gpu_torch_modules.py (the SDF pattern: OneBlob has a continuous second
derivative, so the loss goes through it exactly) against float64 autograd with the modelling of tests/bbi_ref.py (an fp16
rounding at every point where the device stores fp16, forward and backward) at that file's bars, rel-L2 <= 2e-3 and
1 - cosine <= 1e-5; the NRC encoding's shapes; and tiny-cuda-nn's OneBlob image-fit configuration (data/config_oneblob.json:
2 -> 3, n_bins 64, FullyFusedMLP 128 x 5) on a synthetic smooth target, where 30 Adam steps lower the loss (that it trains,
not a parity test: in that shape almost half the samples have a hidden pre-activation within 1e-4 of 0)."""
import numpy as np
import pytest

import act_ref as A
import bbi_ref as R
import enc_ref as E
import enc_ref2 as E2
from test_gpu_torch_modules import _check, _eikonal

pytestmark = pytest.mark.gpu

B = 200
BLOB8 = {"otype": "OneBlob", "n_bins": 8}
SOFTPLUS = {"otype": "FullyFusedMLP", "activation": "Softplus", "output_activation": "None", "n_neurons": 64, "n_hidden_layers": 2}
SHAPES = E.mlp_shapes(32, 64, 2)


def _softplus_graph(ph, pos, scale):
    """OneBlob(3 dims, 8 bins) -> 24 features + 8 ones -> W 64, 2 hidden Softplus layers, 16 padded outputs in float64"""
    import torch
    r16 = R.r16_fn(scale)
    mats = E.mlp_mats(ph, SHAPES)
    xt = torch.tensor(pos.astype(np.float64), requires_grad=True)
    h = r16(E.pad_ones(E2.encode(xt, BLOB8)))
    for li, Wm in enumerate(mats):
        z = r16(h @ Wm.T)
        if li < len(mats) - 1:
            h = r16(A.act("Softplus", z))
    return dict(xt=xt, leaves=mats, out=z)


def test_oneblob_softplus_network_eikonal(torch_cuda):
    import torch
    import tinycudann as tcnn
    m = tcnn.NetworkWithInputEncoding(3, 1, BLOB8, SOFTPLUS)
    assert m.n_output_dims == 1 and m.dtype == torch.float16 and m.loss_scale == 128.0
    hp = m._backend.m.hyperparams()["encoding"]
    assert m._backend.supports_double_backward and hp["otype"] == "OneBlob" and hp["n_bins"] == 8
    rng = np.random.default_rng(71)
    ph = E.mlp_params(rng, SHAPES)
    assert m.params.numel() == ph.size
    pos = rng.uniform(0.02, 0.98, (B, 3)).astype(np.float32)
    with torch.no_grad():
        m.params.copy_(torch.from_numpy(ph.astype(np.float32)))
    x = torch.from_numpy(pos).cuda().requires_grad_(True)
    y = m(x)
    assert y.shape == (B, 1) and y.dtype == torch.float16
    _eikonal(y.float(), x, torch).backward()
    ref = _softplus_graph(ph, pos, 128.0)
    grads = torch.autograd.grad(_eikonal(ref["out"][:, :1], ref["xt"], torch), ref["leaves"] + [ref["xt"]])
    _check("tcnn_network_oneblob_softplus", {"params": m.params.grad.cpu().numpy(), "x": x.grad.cpu().numpy()},
           {"params": R.flat(grads[:-1]), "x": grads[-1].numpy()})


def test_nrc_encoding_shapes(torch_cuda):
    import torch
    import tinycudann as tcnn
    for name in ("NRC", "OneBlobFrequency"):
        m = tcnn.Encoding(9, {"otype": name})
        assert m.n_input_dims == 9 and m.n_output_dims == 3 * 12 + 5 * 4 + 1 and m.dtype == torch.float16
        assert m.params.numel() == 0 and m.params.dtype == torch.float32 and m._backend.supports_double_backward
        pos = np.random.default_rng(73).uniform(0, 1, (B, 9)).astype(np.float32)
        x = torch.from_numpy(pos).cuda().requires_grad_(True)
        y = m(x)
        assert y.shape == (B, 57) and y.dtype == torch.float16
        want = E2.encode(torch.tensor(pos.astype(np.float64)), {"otype": name}).numpy()
        assert np.abs(y.detach().float().cpu().numpy() - want).max() <= 2.0 ** -11 + 2.0 ** -20  # |features| <= 1: one fp16 rounding
        y.float().sum().backward()
        assert x.grad.shape == (B, 9) and torch.isfinite(x.grad).all() and bool((x.grad[:, 8] == 1).all())
    for cfg, n_in in (({"otype": "TriangleWave", "n_frequencies": 3}, 2), ({"otype": "OneBlob"}, 2)):
        assert tcnn.Encoding(n_in, cfg)._backend.supports_double_backward


def test_oneblob_image_fit_config_trains(torch_cuda):
    """tiny-cuda-nn's data/config_oneblob.json (encoding and network) on a smooth 2-D -> RGB target"""
    import torch
    import tinycudann as tcnn
    enc = {"otype": "OneBlob", "n_bins": 64}
    net = {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 128, "n_hidden_layers": 5}
    m = tcnn.NetworkWithInputEncoding(2, 3, enc, net, seed=5)
    assert m.n_input_dims == 2 and m.n_output_dims == 3 and m.params.numel() == 128 * 128 * 5 + 16 * 128
    opt = torch.optim.Adam(m.parameters(), lr=1e-2, betas=(0.9, 0.99), eps=1e-8)
    rng = np.random.default_rng(75)
    xy = torch.from_numpy(rng.uniform(0, 1, (B, 2)).astype(np.float32)).cuda()
    target = torch.stack([torch.sin(6.0 * xy[:, 0]) * 0.5 + 0.5, xy[:, 0] * xy[:, 1], torch.cos(4.0 * xy[:, 1]) * 0.5 + 0.5], dim=1)
    losses = []
    for _ in range(30):
        loss = ((m(xy).float() - target) ** 2).mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    print(f"oneblob image fit: loss {losses[0]:.4f} -> {losses[-1]:.4f}")
    assert np.isfinite(losses).all() and torch.isfinite(m.params).all()
    assert losses[-1] < losses[0]
