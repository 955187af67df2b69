"""NetworkWithInputEncoding(TriangleWave / OneBlob / NRC -> FullyFusedMLP) at the Module level, n = 256 and 384, as
tests/test_gpu_enc_mlp.py tests the other parameter-free encodings. The encoding kernel writes the MLP's fp16 input rows
directly; everything behind them is the existing MLP path, so

  * the forward and dL_dparams are BITWISE those of create_network(encoded width, n_out, net) fed with the stand-alone Fp16
    encoding's output (converted to float) and the same parameters, and initialize_params(seed) is bitwise equal too: the
    ones padding (8 columns behind OneBlob's 24, 15 behind NRC's 33) and the column order are pinned with no tolerance;
  * dL_dinput = J_enc^T d0 with d0 that module's fp32 dL_dinput and J_enc the float64 reference Jacobian, per entry
    |err| <= (in_pad + 2) 2^-24 sum_k |d0_k J_kd| + 2^-20 sum_k |d0_k| c_k, c_k = max(1, |J_kd|) or n_bins for a OneBlob column
    (tests/test_gpu_encodings2.py);
  * backward_backward_input, all three results, against float64 autograd modelled as tests/bbi_ref.py models the networks
    (fp16-rounded weights, a rounding at every fp16 storage point, samples with a hidden pre-activation within 1e-4 of 0
    removed from both sides, their share <= 0.05 by the reference alone) at the project's fp16 bars: rel-L2 <= 2e-3,
    cosine >= 0.99999. The shares for these inputs and parameters (n = 256 / 384): tri 0.000 / 0.003, oneblob 0.023 /
    0.013, nrc 0.020 / 0.008;
  * OneBlob in front of a Softplus network created with "second_order": "exact": the floor-based bar of
    tests/test_gpu_ffmlp_second_order.py (device rel-L2 <= 4 x the fp16-rounded chain's own distance from float64, never
    beyond 2e-2, cosine >= 0.999).
"""
import functools

import numpy as np
import pytest

import act_ref as A
import bbi_ref as R
import enc_ref as E
import enc_ref2 as E2

pytestmark = pytest.mark.gpu

W, NH, N_OUT = 64, 2, 1
# name -> (n_input_dims, encoding, encoded width, in_pad)
NETS = {
    "tri": (3, {"otype": "TriangleWave", "n_frequencies": 4}, 12, 16),
    "oneblob": (3, {"otype": "OneBlob", "n_bins": 8}, 24, 32),
    "nrc": (9, {"otype": "NRC", "n_frequencies": 4, "n_bins": 4}, 33, 48),
}
NET_CFG = {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": W, "n_hidden_layers": NH,
           "gradient_precision": "fp32"}


@functools.lru_cache(maxsize=None)
def _inputs(name, n):
    x = np.random.default_rng(31 + n).uniform(0.02, 0.98, (n, NETS[name][0])).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _jacobian(name, n):
    D, enc, _, _ = NETS[name]
    _, J = E2.jacobian(_inputs(name, n), enc)
    c = E2.derivative_scale(enc, D, J)
    J.setflags(write=False)
    c.setflags(write=False)
    return J, c


@pytest.mark.parametrize("n", [256, 384])
@pytest.mark.parametrize("name", list(NETS))
def test_forward_and_backward_against_identity_mlp(torch_cuda, name, n):
    t = torch_cuda
    from neus2_amd.module import GradientMode, Module
    D, enc, w, in_pad = NETS[name]
    m = Module.create_network_with_input_encoding(D, N_OUT, enc, NET_CFG, batch_capacity=512)
    e = Module.create_encoding(dict(enc, output_layout="AoS"), batch_capacity=512, n_input_dims=D)
    assert e.n_output_dims == w
    ref = Module.create_network(w, N_OUT, NET_CFG, batch_capacity=512)
    hp = m.hyperparams()
    assert hp["otype"] == "NetworkWithInputEncoding" and hp["network"]["n_neurons"] == W
    assert hp["encoding"]["otype"] == ("Composite" if name == "nrc" else enc["otype"])
    assert m.n_params == ref.n_params and m.n_input_dims == D and m.n_output_dims == 16 and m.info["n_levels"] == 0
    assert t.equal(m.initialize_params(11), ref.initialize_params(11))
    rng = np.random.default_rng(7)
    ph = E.mlp_params(rng, E.mlp_shapes(in_pad, W, NH))
    assert ph.size == m.n_params
    params = t.from_numpy(ph).cuda()
    x = t.from_numpy(_inputs(name, n).copy()).cuda()
    feats = e.inference(x, None).float().contiguous()
    assert feats.shape == (n, w)
    ctx, y = m.forward(x, params, prepare_input_gradients=True)
    ctx_r, y_r = ref.forward(feats, params, prepare_input_gradients=True)
    assert t.equal(y.view(t.int16), y_r.view(t.int16))
    assert t.equal(m.inference(x, params).view(t.int16), y_r.view(t.int16))
    dlo = t.from_numpy(rng.normal(0, 1, (n, 16)).astype(np.float16)).cuda()
    g, g_r = m.gradient_buffer(), ref.gradient_buffer()
    dx = t.full((n, D), 7.0, dtype=t.float32, device="cuda")  # overwritten, not accumulated
    d0 = t.zeros((n, w), dtype=t.float32, device="cuda")
    m.backward(ctx, x, dlo, params, dL_dparams=g, dL_dinput=dx, mode=GradientMode.Overwrite, output=y)
    ref.backward(ctx_r, feats, dlo, params, dL_dparams=g_r, dL_dinput=d0, mode=GradientMode.Overwrite, output=y_r)
    assert g.dtype == t.float32 and g.abs().sum().item() > 0
    assert t.equal(g, g_r)
    J, c = _jacobian(name, n)
    d0n = d0.cpu().numpy().astype(np.float64)
    want = np.einsum("nk,nkd->nd", d0n, J)
    bound = ((in_pad + 2) * 2.0 ** -24 * np.einsum("nk,nkd->nd", np.abs(d0n), np.abs(J))
             + 2.0 ** -20 * np.einsum("nk,nkd->nd", np.abs(d0n), c))
    err = np.abs(dx.cpu().numpy().astype(np.float64) - want)
    print(f"{name} n={n}: dL_dinput max err/bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
    assert np.abs(want).max() > 0 and (err <= bound).all()
    dx2 = t.full((n, D), -3.0, dtype=t.float32, device="cuda")
    m.backward(ctx, x, dlo, params, dL_dinput=dx2, mode=GradientMode.Ignore, output=y)
    assert t.equal(dx2, dx)


def _reference_graph(name, ph, pos):
    """encoding -> W 64, 2 hidden ReLU layers, 16 padded outputs, as a float64 graph"""
    import torch
    _, enc, _, in_pad = NETS[name]
    r16 = R.r16_fn(1.0)
    mats = E.mlp_mats(ph, E.mlp_shapes(in_pad, W, NH))
    xt = torch.tensor(pos.astype(np.float64), requires_grad=True)
    out, amb = E.mlp(r16(E.pad_ones(E2.encode(xt, enc))), mats, r16, R.AMBIGUOUS)
    return dict(xt=xt, leaves=mats, out=out, ambiguous=amb)


@pytest.mark.parametrize("n", [256, 384])
@pytest.mark.parametrize("name", list(NETS))
def test_double_backward_relu(torch_cuda, name, n):
    import torch
    t = torch_cuda
    from neus2_amd.module import GradientMode, Module
    D, enc, w, in_pad = NETS[name]
    m = Module.create_network_with_input_encoding(D, N_OUT, enc, NET_CFG, batch_capacity=512)
    rng = np.random.default_rng(17)
    ph = E.mlp_params(rng, E.mlp_shapes(in_pad, W, NH))
    pos = _inputs(name, n)
    ref = _reference_graph(name, ph, pos)
    amb = ref["ambiguous"]
    print(f"{name} n={n}: ambiguous share {amb.mean():.4f}")
    assert amb.mean() <= 0.05
    dlo = rng.normal(0, 1, (n, 16)).astype(np.float16)
    v = rng.normal(0, 1, (n, D)).astype(np.float32)
    dlo[amb] = 0
    v[amb] = 0
    dlo_t = torch.tensor(dlo.astype(np.float64), requires_grad=True)
    gx, = torch.autograd.grad((ref["out"] * dlo_t).sum(), ref["xt"], create_graph=True)
    g2 = torch.autograd.grad((gx * torch.tensor(v.astype(np.float64))).sum(), ref["leaves"] + [dlo_t, ref["xt"]], allow_unused=True)
    assert all(a is not None for a in g2[:-1])
    dx_ref = np.zeros((n, D)) if g2[-1] is None else g2[-1].numpy()  # TriangleWave -> ReLU is piecewise linear in x
    params, x, u, dlo_dev = t.from_numpy(ph).cuda(), t.from_numpy(pos.copy()).cuda(), t.from_numpy(v).cuda(), t.from_numpy(dlo).cuda()
    ctx, y = m.forward(x, params, prepare_input_gradients=True)
    gp = m.gradient_buffer()
    ddo = t.full((n, 16), 7.0, dtype=t.float16, device="cuda")
    ddx = t.full((n, D), 7.0, dtype=t.float32, device="cuda")
    m.backward_backward_input(ctx, x, u, dlo_dev, params, dL_dparams=gp, dL_ddLdoutput=ddo, mode=GradientMode.Overwrite, dL_dinput=ddx)
    got = {"dL_dparams": gp.cpu().numpy(), "dL_ddLdoutput": ddo.float().cpu().numpy(), "dL_dinput": ddx.cpu().numpy()}
    want = {"dL_dparams": R.flat(g2[:-2]), "dL_ddLdoutput": g2[-2].numpy(), "dL_dinput": dx_ref}
    if name == "tri":  # no second derivative anywhere: exact zeros on both sides
        assert not got["dL_dinput"].any() and not want["dL_dinput"].any()
        del got["dL_dinput"]
    metrics = {k: R.rel_cos(got[k], want[k]) for k in got}
    print(f"{name} n={n}:", {k: f"rel {r:.3e} 1-cos {1 - c:.3e}" for k, (r, c) in metrics.items()})
    for k, (rel, cos) in metrics.items():
        assert rel <= 2e-3 and cos >= 0.99999, (k, rel, cos)
    # the outputs alone (Ignore): dL_dinput bitwise the same
    ddx2 = t.full((n, D), -3.0, dtype=t.float32, device="cuda")
    m.backward_backward_input(ctx, x, u, dlo_dev, params, mode=GradientMode.Ignore, dL_dinput=ddx2)
    assert t.equal(ddx2, ddx)


CEIL_REL, MIN_COS, FACTOR = 2e-2, 0.999, 4.0  # tests/test_gpu_ffmlp_second_order.py


def test_exact_double_backward_oneblob_softplus(torch_cuda):
    """OneBlob(3 dims, 8 bins) -> Softplus W 16, 1 hidden layer, "second_order": "exact", n = 128: the truth is autograd on
    the unrounded float64 network, the model the same chain with an fp16 rounding wherever the device stores fp16."""
    import torch
    t = torch_cuda
    from neus2_amd.module import GradientMode, Module
    D, enc, w, in_pad = NETS["oneblob"]
    Ws, n, out_pad = 16, 128, 16
    cfg = {"otype": "FullyFusedMLP", "n_neurons": Ws, "n_hidden_layers": 1, "activation": "Softplus", "output_activation": "None",
           "gradient_precision": "fp32", "second_order": "exact"}
    m = Module.create_network_with_input_encoding(D, 1, enc, cfg, batch_capacity=128)
    rng = np.random.default_rng(23)
    x = rng.uniform(0.02, 0.98, (n, D)).astype(np.float32)
    u = rng.normal(0, 1, (n, D)).astype(np.float16).astype(np.float32)
    g = rng.normal(0, 1, (n, out_pad)).astype(np.float16)
    shapes = [(Ws, in_pad), (out_pad, Ws)]
    ph = (m.initialize_params(seed=3).cpu().numpy() * 0.8).astype(np.float16)
    assert ph.size == m.n_params == sum(r * k for r, k in shapes)
    mats, o = [], 0
    for r, k in shapes:
        mats.append(torch.tensor(ph[o:o + r * k].astype(np.float64).reshape(r, k)))
        o += r * k
    args = (lambda xx, tab: E2.encode(xx, enc), torch.tensor(x.astype(np.float64)), None, torch.tensor(u.astype(np.float64)), mats,
            torch.tensor(g.astype(np.float64)), "Softplus", "None", 1.0)
    truth, model = A.truth(*args), A.bbi(*args, rounded=True)
    dev16 = lambda a: t.from_numpy(a.view(np.int16).copy()).cuda().view(t.float16)
    params, xd, ud, gd = dev16(ph), t.from_numpy(x).cuda(), t.from_numpy(u).cuda(), dev16(g)
    outs = []
    for _ in range(2):
        ctx, _y = m.forward(xd, params, prepare_input_gradients=True)
        gp = t.full((m.n_params,), 7.0, dtype=t.float32, device="cuda")
        ddo = t.full((n, out_pad), 7.0, dtype=t.float16, device="cuda")
        ddx = t.full((n, D), 7.0, dtype=t.float32, device="cuda")
        m.backward_backward_input(ctx, xd, ud, gd, params, dL_dparams=gp, dL_ddLdoutput=ddo, mode=GradientMode.Overwrite, dL_dinput=ddx)
        outs.append((gp.cpu().numpy(), ddo.float().cpu().numpy(), ddx.cpu().numpy()))
    for p, q in zip(*outs):
        np.testing.assert_array_equal(p, q)
    gp, ddo, ddx = outs[0]
    assert truth["dx"].abs().max().item() > 0
    pairs, o = [], 0
    for l, (r, k) in enumerate(shapes):
        pairs.append((f"dW{l}", gp[o:o + r * k], truth["dW"][l].numpy(), model["dW"][l].numpy()))
        o += r * k
    pairs += [("dL_ddLdoutput", ddo, truth["ddo"].numpy(), model["ddo"].numpy()), ("dL_dinput", ddx, truth["dx"].numpy(), model["dx"].numpy())]
    failures = []
    for what, got, tr, mo in pairs:
        floor = A.rel(mo, tr)
        rel, cos = R.rel_cos(got, tr)
        bound = min(FACTOR * floor, CEIL_REL)
        print(f"oneblob_softplus {what}: rel {rel:.3e} floor {floor:.3e} bound {bound:.3e} 1-cos {1 - cos:.3e}")
        if not (rel <= bound and cos >= MIN_COS):
            failures.append((what, rel, floor, bound, cos))
    assert not failures, failures
