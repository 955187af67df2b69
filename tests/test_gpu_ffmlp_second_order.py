"""backward_backward_input of networks created with "second_order": "exact", whose hidden or output activation has a second
derivative (Softplus, Squareplus, Sigmoid, Exponential): dL_dparams per matrix and per table, dL_ddLdoutput and dL_dinput
against torch.autograd on the unrounded float64 network (the truth, tests/act_ref.py), behind the Identity encoding, the
fp16 HashGrid, a general (2-dim Smoothstep) grid, Frequency and SphericalHarmonics.

Tolerance. For its own inputs each case computes floor = rel-L2(model, truth) on the CPU, the model being the same chain in
float64 with an fp16 rounding wherever the device stores fp16: the storage noise of the chain. The device is held to
rel-L2(device, truth) <= 4 floor (it sums in fp32 on MFMA and uses expf where the model has float64, and its rounding
points need not match the model's one for one), and never beyond the project's ceiling for these quantities, rel-L2 <=
2e-2 and cosine >= 0.999 (test_gpu_ffmlp.py). A missing act'' term is an error of order one. Every measured value and its
floor go to parity_metrics.jsonl.

Also: bitwise repeatability, the null-pointer cases, that "exact" changes nothing for ReLU / None networks, that the
default mode is unchanged (refusal included), and the parsing of the key."""
import functools

import numpy as np
import pytest

import act_ref as A
import bbi_ref as R

pytestmark = pytest.mark.gpu

CEIL_REL, MIN_COS, FACTOR = 2e-2, 0.999, 4.0

# act / out_act, W, N, n_in, n_out, n (of capacity): W 16 is one zero-padded 32-row tile, W 128 all four M tiles, n = 2176
# of 4096 three ragged weight-gradient blocks; ReLU / Sigmoid is the colour-network shape, where only e_o is non-zero
NET_CASES = {
    "softplus_w16": dict(act="Softplus", out="None", W=16, N=1, n_in=3, n_out=1, n=128, cap=128),
    "squareplus_w128": dict(act="Squareplus", out="None", W=128, N=3, n_in=12, n_out=2, n=128, cap=128),
    "sigmoid_sigmoid_w32": dict(act="Sigmoid", out="Sigmoid", W=32, N=2, n_in=8, n_out=3, n=128, cap=128),
    "softplus_exp_w64_n2176": dict(act="Softplus", out="Exponential", W=64, N=2, n_in=20, n_out=1, n=2176, cap=4096),
    "relu_sigmoid_w64": dict(act="ReLU", out="Sigmoid", W=64, N=1, n_in=3, n_out=3, n=128, cap=128),
}
GRID2 = {"otype": "Grid", "type": "Hash", "n_levels": 4, "n_features_per_level": 2, "log2_hashmap_size": 9, "base_resolution": 4,
         "per_level_scale": 2.0, "interpolation": "Smoothstep"}
# encoding, n_in, act, W, N, n_out (n = 128)
ENC_CASES = {
    "hashgrid_softplus": dict(enc=R.ENC_CFG, n_in=3, act="Softplus", W=16, N=2, n_out=3),
    "grid2_smoothstep_squareplus": dict(enc=GRID2, n_in=2, act="Squareplus", W=32, N=1, n_out=1),
    "frequency_softplus": dict(enc={"otype": "Frequency", "n_frequencies": 4}, n_in=3, act="Softplus", W=16, N=1, n_out=1),
    "sh_softplus": dict(enc={"otype": "SphericalHarmonics", "degree": 2}, n_in=3, act="Softplus", W=16, N=1, n_out=1),
}
BITWISE = [k for k in list(NET_CASES) + list(ENC_CASES) if k != "grid2_smoothstep_squareplus"]  # the general grid sums by atomics


def _net_cfg(c, second_order="exact"):
    cfg = {"otype": "FullyFusedMLP", "n_neurons": c["W"], "n_hidden_layers": c["N"], "activation": c["act"],
           "output_activation": c.get("out", "None"), "gradient_precision": "fp32"}
    if second_order:
        cfg["second_order"] = second_order
    return cfg


def _module(name, second_order="exact"):
    from neus2_amd.module import Module
    if name in NET_CASES:
        c = NET_CASES[name]
        return Module.create_network(c["n_in"], c["n_out"], _net_cfg(c, second_order), batch_capacity=c["cap"])
    c = ENC_CASES[name]
    return Module.create_network_with_input_encoding(c["n_in"], c["n_out"], c["enc"], _net_cfg(c, second_order), batch_capacity=128)


def _encoder(name):
    """(enc(x, table) in float64, the table's feature count or None, the rows' padding value)"""
    import enc_ref
    import grid_nd_ref as G
    from torch_ref import hash_grid
    if name in NET_CASES:
        return (lambda x, tab: x), None, 1.0
    cfg = ENC_CASES[name]["enc"]
    if name == "hashgrid_softplus":
        return (lambda x, tab: hash_grid(x, tab, R.OFF, R.RES)), 2, 0.0
    if name == "grid2_smoothstep_squareplus":
        off, res = G.level_tables(2, 4, 9, 4, 2.0, "Hash")
        return (lambda x, tab: G.grid_encode(x, tab, off, res, "Hash", "Smoothstep")), 2, 0.0
    return (lambda x, tab: enc_ref.encode(x, cfg)), None, 1.0


@functools.lru_cache(maxsize=None)
def _case(name):
    """The case's inputs (numpy, as the device gets them) with truth and model, computed once on the CPU and shared."""
    import torch
    import grid_nd_ref as G
    m = _module(name)
    c = NET_CASES.get(name) or dict(ENC_CASES[name], out="None", n=128)
    n, n_in, W, N = c["n"], c["n_in"], c["W"], c["N"]
    enc, F, pad_value = _encoder(name)
    rng = np.random.default_rng(sorted(list(NET_CASES) + list(ENC_CASES)).index(name) + 100)
    grid = name in ("hashgrid_softplus", "grid2_smoothstep_squareplus")
    # inputs: fp16 values where the device reads fp16 (the Identity encoding's x and u), fp32 positions for the rest
    if name in NET_CASES:
        x = rng.uniform(-1, 1, (n, n_in)).astype(np.float16).astype(np.float32)
    else:
        x = rng.uniform(0.02, 0.98, (n, n_in)).astype(np.float32)
    u = rng.normal(0, 1, (n, n_in)).astype(np.float16).astype(np.float32)
    out_pad = m.n_output_dims
    g = rng.normal(0, 1, (n, out_pad)).astype(np.float16)
    with torch.no_grad():
        width = enc(torch.zeros(1, n_in, dtype=torch.float64), torch.zeros(1 << 14, F, dtype=torch.float64) if F else None).shape[1]
    in_pad = (width + 15) // 16 * 16
    shapes = [(W, in_pad)] + [(W, W)] * (N - 1) + [(out_pad, W)]
    n_mlp = sum(r * k for r, k in shapes)
    if name == "hashgrid_softplus":
        ph = R.net_params("gridmlp", rng)
    elif name == "grid2_smoothstep_squareplus":
        ph = G.network_params(rng, shapes, width, 2, m.n_params - n_mlp)
    else:  # as test_ffmlp_backward_backward_input scales them
        ph = (m.initialize_params(seed=3).cpu().numpy() * 0.8).astype(np.float16)
    assert ph.size == m.n_params and (grid or ph.size == n_mlp)
    mats, o = [], 0
    for r, k in shapes:
        mats.append(torch.tensor(ph[o:o + r * k].astype(np.float64).reshape(r, k)))
        o += r * k
    table = torch.tensor(ph[o:].astype(np.float64).reshape(-1, F)) if grid else None
    ambiguous = 0.0
    if c["act"] == "ReLU":  # samples whose hidden pre-activation may take the other branch on the device: out of g and u
        h0 = A.r16(A.rows(torch.tensor(x.astype(np.float64)), 1.0))
        amb = (np.abs(A.r16(h0 @ mats[0].T).numpy()) < R.AMBIGUOUS).any(axis=1)
        g[amb] = 0
        u[amb] = 0
        ambiguous = amb.mean()
    args = (enc, torch.tensor(x.astype(np.float64)), table, torch.tensor(u.astype(np.float64)), mats, torch.tensor(g.astype(np.float64)),
            c["act"], c["out"], pad_value)
    return dict(c=c, x=x, u=u, g=g, ph=ph, shapes=shapes, n_mlp=n_mlp, truth=A.truth(*args), model=A.bbi(*args, rounded=True),
                ambiguous=ambiguous, sh=name == "sh_softplus")


def _run(t, m, k, want_dx=True, want_ddo=True, want_g=True):
    """One forward and one backward_backward_input on the device: (dL_dparams, dL_ddLdoutput, dL_dinput) as numpy."""
    from neus2_amd.module import GradientMode
    dev16 = lambda a: t.from_numpy(a.view(np.int16).copy()).cuda()
    params, x, u, g = dev16(k["ph"]), t.from_numpy(k["x"]).cuda(), t.from_numpy(k["u"]).cuda(), dev16(k["g"])
    n = k["x"].shape[0]
    ctx, _ = m.forward(x, params, prepare_input_gradients=True)
    gp = t.full((m.n_params,), 7.0, dtype=t.float32, device="cuda") if want_g else None
    ddo = t.full((n, m.n_output_dims), 7.0, dtype=t.float16, device="cuda") if want_ddo else None
    ddx = t.full((n, m.n_input_dims), 7.0, dtype=t.float32, device="cuda") if want_dx else None
    m.backward_backward_input(ctx, x, u, g, params, dL_dparams=gp, dL_ddLdoutput=ddo,
                              mode=GradientMode.Overwrite if want_g else GradientMode.Ignore, dL_dinput=ddx)
    t.cuda.synchronize()
    return tuple(None if a is None else a.cpu().numpy() for a in (gp, ddo, ddx))


def _held(name, what, got, truth, model, failures):
    floor = A.rel(model, truth)
    rel, cos = R.rel_cos(got, truth)
    bound = min(FACTOR * floor, CEIL_REL)
    R.record(f"second_order_{name}_{what}", rel=rel, one_minus_cos=1 - cos, floor=floor)
    print(f"{name} {what}: rel {rel:.3e} floor {floor:.3e} bound {bound:.3e} 1-cos {1 - cos:.3e}")
    if not (rel <= bound and cos >= MIN_COS):
        failures.append((what, rel, floor, bound, cos))


@pytest.mark.parametrize("name", list(NET_CASES) + list(ENC_CASES))
def test_exact_double_backward(torch_cuda, name):
    from neus2_amd import NeusError
    t = torch_cuda
    k = _case(name)
    assert k["ambiguous"] <= 0.05
    m = _module(name)
    if k["sh"]:
        with pytest.raises(NeusError, match="not supported.*SphericalHarmonics"):
            _run(t, m, k)
    gp, ddo, ddx = _run(t, m, k, want_dx=not k["sh"])
    truth, model, failures = k["truth"], k["model"], []
    o = 0
    for l, (r, c) in enumerate(k["shapes"]):
        _held(name, f"dW{l}", gp[o:o + r * c], truth["dW"][l].numpy(), model["dW"][l].numpy(), failures)
        o += r * c
    if truth["dtable"] is not None:
        _held(name, "dtable", gp[o:], truth["dtable"].numpy(), model["dtable"].numpy(), failures)
    _held(name, "dL_ddLdoutput", ddo.astype(np.float32), truth["ddo"].numpy(), model["ddo"].numpy(), failures)
    if not k["sh"]:
        assert truth["dx"].abs().max().item() > 0  # behind the Identity encoding it was zeros before
        _held(name, "dL_dinput", ddx, truth["dx"].numpy(), model["dx"].numpy(), failures)
    assert not failures, failures


@pytest.mark.parametrize("name", BITWISE)
def test_repeatable_and_null_pointers(torch_cuda, name):
    from neus2_amd.module import GradientMode
    t = torch_cuda
    k = _case(name)
    m = _module(name)
    dx = not k["sh"]
    a, b = _run(t, m, k, want_dx=dx), _run(t, m, k, want_dx=dx)
    for p, q in zip(a, b):
        if p is not None:
            np.testing.assert_array_equal(p.view(np.uint8), q.view(np.uint8))
    # dL_ddLdoutput alone (Ignore): bitwise the full call's
    only = _run(t, m, k, want_dx=False, want_g=False)
    np.testing.assert_array_equal(only[1].view(np.uint16), a[1].view(np.uint16))
    if dx:  # dL_dinput alone needs the fronts and the curvature chain all the same
        np.testing.assert_array_equal(_run(t, m, k, want_ddo=False, want_g=False)[2].view(np.uint8), a[2].view(np.uint8))
    # all three null: nothing to do, and no error
    assert _run(t, m, k, want_dx=False, want_ddo=False, want_g=False) == (None, None, None)


@pytest.mark.parametrize("name", list(R.NETS))
def test_exact_changes_nothing_for_relu_networks(torch_cuda, name):
    """ReLU hidden layers and a linear output: act'' = 0, and a module created with "exact" takes the default one's launches."""
    from neus2_amd.module import Module
    t = torch_cuda
    enc, W, NH, n_out = R.NETS[name]
    rng = np.random.default_rng(5)
    ph = R.net_params(name, rng, 0.3 if name == "dnet" else None)
    k = dict(ph=ph, x=rng.uniform(0.02, 0.98, (128, 3)).astype(np.float32), u=rng.normal(0, 1, (128, 3)).astype(np.float32),
             g=rng.normal(0, 1, (128, 16)).astype(np.float16))
    outs = []
    for so in (None, "exact"):
        cfg = dict(R.net_cfg(name), gradient_precision="fp32")
        if so:
            cfg["second_order"] = so
        m = (Module.create_network_with_input_encoding(3, n_out, R.ENC_CFG, cfg, batch_capacity=128) if enc
             else Module.create_network(3, n_out, cfg, batch_capacity=128))
        assert m.n_params == ph.size
        outs.append(_run(t, m, k))
    for p, q in zip(*outs):
        np.testing.assert_array_equal(p.view(np.uint8), q.view(np.uint8))
    assert np.abs(outs[0][0]).max() > 0


def test_default_mode_is_unchanged(torch_cuda):
    from neus2_amd import NeusError
    t = torch_cuda
    name = "hashgrid_softplus"
    k = _case(name)
    with pytest.raises(NeusError, match="ReLU or None"):
        _run(t, _module(name, None), k, want_ddo=False)
    with pytest.raises(NeusError, match="ReLU or None"):
        _run(t, _module(name, "tcnn"), k, want_dx=False)
    g0 = _run(t, _module(name, None), k, want_dx=False, want_ddo=False)[0]
    g1 = _run(t, _module(name, "tcnn"), k, want_dx=False, want_ddo=False)[0]
    np.testing.assert_array_equal(g0.view(np.uint8), g1.view(np.uint8))
    ge = _run(t, _module(name), k, want_dx=False, want_ddo=False)[0]
    assert np.isfinite(g0).all() and np.abs(g0).max() > 0
    assert A.rel(g0[:k["n_mlp"]], ge[:k["n_mlp"]]) > 1e-2 and A.rel(g0[k["n_mlp"]:], ge[k["n_mlp"]:]) > 1e-2


def test_default_mode_refuses_an_output_activation_behind_a_grid(torch_cuda):
    """The default chain is not handed the forward's output: where the grid's gradient needs the output activation's delta,
    the call says so on the host and launches nothing (it read a null pointer on the device before)."""
    from neus2_amd import NeusError
    from neus2_amd.module import Module
    t = torch_cuda
    rng = np.random.default_rng(9)
    k = dict(ph=R.net_params("gridmlp", rng), x=rng.uniform(0.02, 0.98, (128, 3)).astype(np.float32),
             u=rng.normal(0, 1, (128, 3)).astype(np.float32), g=rng.normal(0, 1, (128, 16)).astype(np.float16))
    cfg = dict(R.net_cfg("gridmlp"), output_activation="Sigmoid", gradient_precision="fp32")
    m = Module.create_network_with_input_encoding(3, 3, R.ENC_CFG, cfg, batch_capacity=128)
    with pytest.raises(NeusError, match="second_order"):
        _run(t, m, k, want_dx=False, want_ddo=False)
    gp = _run(t, Module.create_network_with_input_encoding(3, 3, R.ENC_CFG, dict(cfg, second_order="exact"), batch_capacity=128), k)[0]
    assert np.isfinite(gp).all() and np.abs(gp).max() > 0


def test_config_parsing(torch_cuda):
    from neus2_amd import NeusError
    with pytest.raises(NeusError, match="second_order"):
        _module("softplus_w16", "fast")
    assert _module("softplus_w16").hyperparams()["network"]["second_order"] == "exact"
    assert "second_order" not in _module("softplus_w16", None).hyperparams()["network"]
    assert "second_order" not in _module("softplus_w16", "tcnn").hyperparams()["network"]
    assert "second_order" not in _module("hashgrid_softplus", None).hyperparams()["network"]
    assert _module("hashgrid_softplus").hyperparams()["network"]["second_order"] == "exact"
