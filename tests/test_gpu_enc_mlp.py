"""NetworkWithInputEncoding(Frequency / SphericalHarmonics / Composite -> FullyFusedMLP) at the Module level, n = 256 and
384. The encoding kernel writes the MLP's fp16 input rows directly; everything behind them is the existing MLP path, so

  * the forward and dL_dparams are BITWISE those of create_network(encoded width, n_out, net) fed with the stand-alone Fp16
    encoding's output (converted to float) and the same parameters, and initialize_params(seed) is bitwise equal too: the
    ones padding and the column order are pinned with no tolerance;
  * dL_dinput = J_enc^T d0 with d0 that module's fp32 dL_dinput and J_enc the float64 reference Jacobian, per entry
    |err| <= (in_pad + 2) 2^-24 sum_k |d0_k J_kd| + 2^-20 sum_k |d0_k| max(1, |J_kd|) (the fp32 sum, the derivative's error);
  * backward_backward_input (Frequency -> ReLU network) against float64 autograd modelled as tests/bbi_ref.py models the
    networks (fp16-rounded weights, a rounding at every fp16 storage point, samples with a hidden pre-activation within
    1e-4 of 0 removed from both sides, their share <= 0.05 by the reference alone) at the project's fp16 bars: rel-L2 <= 2e-3,
    cosine >= 0.99999.

Double backward measured on an MI355X (rel-L2 / 1 - cosine): see DESIGN.md section 3.11."""
import functools

import numpy as np
import pytest

import bbi_ref as R
import enc_ref as E

pytestmark = pytest.mark.gpu

FREQ = {"otype": "Frequency", "n_frequencies": 4}
SH4 = {"otype": "SphericalHarmonics", "degree": 4}
COMP = {"otype": "Composite", "nested": [{"otype": "Identity", "n_dims_to_encode": 6}, {"otype": "SphericalHarmonics", "degree": 4}]}
# name -> (n_input_dims, encoding, n_neurons, n_hidden_layers, n_output_dims, output_activation)
NETS = {"freq": (3, FREQ, 64, 2, 1, "None"), "sh": (3, SH4, 16, 1, 3, "None"), "composite": (9, COMP, 64, 2, 3, "Sigmoid")}


def _net_cfg(name):
    _, _, W, NH, _, oa = NETS[name]
    return {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": oa, "n_neurons": W, "n_hidden_layers": NH,
            "gradient_precision": "fp32"}


@functools.lru_cache(maxsize=None)
def _inputs(name, n):
    D = NETS[name][0]
    x = np.random.default_rng(31 + n).uniform(0.02, 0.98, (n, D)).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _jacobian(name, n):
    y, J = E.jacobian(_inputs(name, n), NETS[name][1])
    J.setflags(write=False)
    return J


@pytest.mark.parametrize("n", [256, 384])
@pytest.mark.parametrize("name", list(NETS))
def test_forward_and_backward_against_identity_mlp(torch_cuda, name, n):
    t = torch_cuda
    from neus2_amd.module import GradientMode, Module
    D, enc, W, NH, n_out, _ = NETS[name]
    cfg = _net_cfg(name)
    m = Module.create_network_with_input_encoding(D, n_out, enc, cfg, batch_capacity=512)
    e = Module.create_encoding(dict(enc, output_layout="AoS"), batch_capacity=512, n_input_dims=D)
    w = e.n_output_dims
    ref = Module.create_network(w, n_out, cfg, batch_capacity=512)
    in_pad = (w + 15) // 16 * 16
    hp = m.hyperparams()
    assert hp["otype"] == "NetworkWithInputEncoding" and hp["encoding"]["otype"] == enc["otype"] and hp["network"]["n_neurons"] == W
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
    J = _jacobian(name, n)
    d0n = d0.cpu().numpy().astype(np.float64)
    want = np.einsum("nk,nkd->nd", d0n, J)
    bound = ((in_pad + 2) * 2.0 ** -24 * np.einsum("nk,nkd->nd", np.abs(d0n), np.abs(J))
             + 2.0 ** -20 * np.einsum("nk,nkd->nd", np.abs(d0n), np.maximum(1.0, np.abs(J))))
    err = np.abs(dx.cpu().numpy().astype(np.float64) - want)
    print(f"{name} n={n}: dL_dinput max err/bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
    assert np.abs(want).max() > 0 and (err <= bound).all()
    dx2 = t.full((n, D), -3.0, dtype=t.float32, device="cuda")
    m.backward(ctx, x, dlo, params, dL_dinput=dx2, mode=GradientMode.Ignore, output=y)
    assert t.equal(dx2, dx)


def _reference_graph(ph, pos, scale=1.0):
    """Frequency(3, F = 4) -> W 64, 2 hidden ReLU layers, 16 padded outputs, as a float64 graph"""
    import torch
    D, enc, W, NH, _, _ = NETS["freq"]
    r16 = R.r16_fn(scale)
    mats = E.mlp_mats(ph, E.mlp_shapes(32, W, NH))
    xt = torch.tensor(pos.astype(np.float64), requires_grad=True)
    out, amb = E.mlp(r16(E.pad_ones(E.encode(xt, enc))), mats, r16, R.AMBIGUOUS)
    return dict(xt=xt, leaves=mats, out=out, ambiguous=amb)


@pytest.mark.parametrize("n", [256, 384])
def test_double_backward_frequency_relu(torch_cuda, n):
    import torch
    t = torch_cuda
    from neus2_amd.module import GradientMode, Module
    D, enc, W, NH, n_out, _ = NETS["freq"]
    m = Module.create_network_with_input_encoding(D, n_out, enc, _net_cfg("freq"), batch_capacity=512)
    rng = np.random.default_rng(17)
    ph = E.mlp_params(rng, E.mlp_shapes(32, W, NH))
    pos = _inputs("freq", n)
    ref = _reference_graph(ph, pos)
    amb = ref["ambiguous"]
    print(f"freq n={n}: ambiguous share {amb.mean():.4f}")
    assert amb.mean() <= 0.05
    dlo = rng.normal(0, 1, (n, 16)).astype(np.float16)
    v = rng.normal(0, 1, (n, D)).astype(np.float32)
    dlo[amb] = 0
    v[amb] = 0
    dlo_t = torch.tensor(dlo.astype(np.float64), requires_grad=True)
    gx, = torch.autograd.grad((ref["out"] * dlo_t).sum(), ref["xt"], create_graph=True)
    g2 = torch.autograd.grad((gx * torch.tensor(v.astype(np.float64))).sum(), ref["leaves"] + [dlo_t, ref["xt"]])
    params, x, u, dlo_dev = t.from_numpy(ph).cuda(), t.from_numpy(pos.copy()).cuda(), t.from_numpy(v).cuda(), t.from_numpy(dlo).cuda()
    ctx, y = m.forward(x, params, prepare_input_gradients=True)
    gp = m.gradient_buffer()
    ddo = t.full((n, 16), 7.0, dtype=t.float16, device="cuda")
    ddx = t.full((n, D), 7.0, dtype=t.float32, device="cuda")
    m.backward_backward_input(ctx, x, u, dlo_dev, params, dL_dparams=gp, dL_ddLdoutput=ddo, mode=GradientMode.Overwrite, dL_dinput=ddx)
    got = {"dL_dparams": gp.cpu().numpy(), "dL_ddLdoutput": ddo.float().cpu().numpy(), "dL_dinput": ddx.cpu().numpy()}
    want = {"dL_dparams": R.flat(g2[:-2]), "dL_ddLdoutput": g2[-2].numpy(), "dL_dinput": g2[-1].numpy()}
    metrics = {}
    for k in got:
        metrics[k] = R.rel_cos(got[k], want[k])
    print(f"freq n={n}:", {k: f"rel {r:.3e} 1-cos {1 - c:.3e}" for k, (r, c) in metrics.items()})
    for k, (rel, cos) in metrics.items():
        assert rel <= 2e-3 and cos >= 0.99999, (k, rel, cos)
    # the outputs alone (Ignore): dL_dinput bitwise the same
    ddx2 = t.full((n, D), -3.0, dtype=t.float32, device="cuda")
    m.backward_backward_input(ctx, x, u, dlo_dev, params, mode=GradientMode.Ignore, dL_dinput=ddx2)
    assert t.equal(ddx2, ddx)


def test_double_backward_refusals(torch_cuda):
    """The Sigmoid-output network keeps the existing "ReLU or None" refusal; a SphericalHarmonics encoding in front of a
    ReLU network gives dL_ddLdoutput and the parameter gradients but no dL_dinput."""
    t = torch_cuda
    from neus2_amd import NeusError
    from neus2_amd.module import GradientMode, Module
    n = 256
    rng = np.random.default_rng(19)
    for name, msg in (("composite", "ReLU or None"), ("sh", "not supported.*SphericalHarmonics")):
        D, enc, W, NH, n_out, _ = NETS[name]
        m = Module.create_network_with_input_encoding(D, n_out, enc, _net_cfg(name), batch_capacity=256)
        params = t.from_numpy(E.mlp_params(rng, E.mlp_shapes(32 if name == "composite" else 16, W, NH))).cuda()
        x = t.from_numpy(_inputs(name, n).copy()).cuda()
        u = t.from_numpy(rng.normal(0, 1, (n, D)).astype(np.float32)).cuda()
        dlo = t.from_numpy(rng.normal(0, 1, (n, 16)).astype(np.float16)).cuda()
        ctx, _ = m.forward(x, params, prepare_input_gradients=True)
        g = m.gradient_buffer()
        ddx = t.zeros((n, D), dtype=t.float32, device="cuda")
        with pytest.raises(NeusError, match=msg):
            m.backward_backward_input(ctx, x, u, dlo, params, dL_dparams=g, mode=GradientMode.Overwrite, dL_dinput=ddx)
        if name == "sh":
            ddo = t.full((n, 16), 7.0, dtype=t.float16, device="cuda")
            m.backward_backward_input(ctx, x, u, dlo, params, dL_dparams=g, dL_ddLdoutput=ddo, mode=GradientMode.Overwrite)
            assert g.abs().sum().item() > 0 and not (ddo == 7.0).all(dim=1).any().item()
