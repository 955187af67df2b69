"""CutlassMLP networks with the Sine activation (SIREN): the forward output, the first backward's dL_dparams / dL_dinput and
the three results of backward_backward_input with "second_order": "exact", per matrix and per table, against
torch.autograd on the unrounded float64 network (the truth, tests/siren_ref.py). The parameters are initialize_params(seed)
as drawn, so the first layer has SIREN's real scale (|z| up to about 15 behind the Identity encoding).

Tolerance: the floor rule of test_gpu_ffmlp_second_order.py, unchanged. floor = rel-L2(model, truth) on the CPU, the model
being the chain in float64 with an fp16 rounding wherever the device stores fp16 (z, h = sin z, c = cos z, p, f, t, d, e, q).
The device is held to rel-L2(device, truth) <= 4 floor, never beyond rel-L2 2e-2, with cosine >= 0.999. Every floor is
asserted <= 5e-3, so that 4 floor stays under the ceiling and the ceiling never hides a failure. Every measured value and
its floor go to parity_metrics.jsonl.

Also: the kept sine and cosine over every finite fp16 argument, inference against forward, bitwise repeatability, the
null-pointer cases, the default mode's refusal, initialize_params against the restatement, and the config's echo and
refusals."""
import functools

import numpy as np
import pytest

import act_ref as A
import bbi_ref as R
import siren_ref as S

pytestmark = pytest.mark.gpu

CEIL_REL, MIN_COS, FACTOR, MAX_FLOOR = 2e-2, 0.999, 4.0, 5e-3
FREQ = {"otype": "Frequency", "n_frequencies": 4}
GRID2 = {"otype": "Grid", "type": "Hash", "n_levels": 4, "n_features_per_level": 2, "log2_hashmap_size": 9, "base_resolution": 4,
         "per_level_scale": 2.0, "interpolation": "Smoothstep"}
# encoding (None: create_network's Identity), n_in, W, hidden layers, n_out, n of capacity, and the seed of initialize_params
# and of the inputs. W 16 is one zero-padded 32-row tile, W 128 all four M tiles of the narrow kernel, W 256 / 512 the wide
# kernels, n = 2176 of 4096 ragged weight-gradient slices. A case whose own floor exceeds 5e-3 changes its seed, not the bar.
CASES = {
    "w16": dict(enc=None, n_in=3, W=16, N=1, n_out=1, n=128, cap=128, seed=400),
    "w64": dict(enc=None, n_in=3, W=64, N=2, n_out=1, n=128, cap=128, seed=401),
    "w128": dict(enc=None, n_in=12, W=128, N=3, n_out=2, n=128, cap=128, seed=402),
    "w256": dict(enc=None, n_in=3, W=256, N=2, n_out=1, n=128, cap=128, seed=403),
    "w512_n2176": dict(enc=None, n_in=3, W=512, N=1, n_out=1, n=2176, cap=4096, seed=404),
    "frequency_w64": dict(enc=FREQ, n_in=3, W=64, N=2, n_out=1, n=128, cap=128, seed=405),
    "grid2_w32": dict(enc=GRID2, n_in=2, W=32, N=1, n_out=1, n=128, cap=128, seed=406),
    "hashgrid_w16": dict(enc=R.ENC_CFG, n_in=3, W=16, N=2, n_out=3, n=128, cap=128, seed=407),
}
BITWISE = [k for k in CASES if k != "grid2_w32"]  # the general grid's table sums by atomics


def _net_cfg(c, second_order="exact", **over):
    cfg = {"otype": "CutlassMLP", "n_neurons": c["W"], "n_hidden_layers": c["N"], "activation": "Sine", "output_activation": "None",
           "gradient_precision": "fp32"}
    if second_order:
        cfg["second_order"] = second_order
    return dict(cfg, **over)


def _module(name, second_order="exact", **over):
    from neus2_amd.module import Module
    c = CASES[name]
    if c["enc"] is None:
        return Module.create_network(c["n_in"], c["n_out"], _net_cfg(c, second_order, **over), batch_capacity=c["cap"])
    return Module.create_network_with_input_encoding(c["n_in"], c["n_out"], c["enc"], _net_cfg(c, second_order, **over), batch_capacity=c["cap"])


def _encoder(c):
    """(enc(x, table) in float64, the table's feature count or None, the table's entries, the rows' padding value)"""
    import enc_ref
    import grid_nd_ref as G
    from torch_ref import hash_grid
    if c["enc"] is None:
        return (lambda x, tab: x), None, 0, 1.0
    if c["enc"] is R.ENC_CFG:
        return (lambda x, tab: hash_grid(x, tab, R.OFF, R.RES)), 2, R.OFF[-1], 0.0
    if c["enc"] is GRID2:
        off, res = G.level_tables(2, 4, 9, 4, 2.0, "Hash")
        return (lambda x, tab: G.grid_encode(x, tab, off, res, "Hash", "Smoothstep")), 2, off[-1], 0.0
    return (lambda x, tab: enc_ref.encode(x, c["enc"])), None, 0, 1.0


def shapes_of(c, width):
    out_pad, in_pad = (c["n_out"] + 15) // 16 * 16, (width + 15) // 16 * 16
    return [(c["W"], in_pad)] + [(c["W"], c["W"])] * (c["N"] - 1) + [(out_pad, c["W"])]


@functools.lru_cache(maxsize=None)
def case(name):
    """The case's inputs (numpy, as the device gets them) with truth and model, computed once on the CPU and shared."""
    import torch
    c = CASES[name]
    n, n_in = c["n"], c["n_in"]
    enc, F, entries, pad_value = _encoder(c)
    rng = np.random.default_rng(c["seed"])
    # inputs: fp16 values where the device reads fp16 (the Identity encoding's x and u), fp32 positions for the rest
    if c["enc"] is None:
        x = rng.uniform(-1, 1, (n, n_in)).astype(np.float16).astype(np.float32)
    else:
        x = rng.uniform(0.02, 0.98, (n, n_in)).astype(np.float32)
    u = rng.normal(0, 1, (n, n_in)).astype(np.float16).astype(np.float32)
    with torch.no_grad():
        width = enc(torch.zeros(1, n_in, dtype=torch.float64), torch.zeros(max(entries, 1), F, dtype=torch.float64) if F else None).shape[1]
    shapes = shapes_of(c, width)
    n_mlp = sum(r * k for r, k in shapes)
    g = rng.normal(0, 1, (n, shapes[-1][0])).astype(np.float16)
    p32 = S.initialize_params(c["seed"], shapes, (F or 0) * entries)  # as drawn
    ph = p32.astype(np.float16)
    mats, o = [], 0
    for r, k in shapes:
        mats.append(torch.tensor(ph[o:o + r * k].astype(np.float64).reshape(r, k)))
        o += r * k
    table = torch.tensor(ph[o:].astype(np.float64).reshape(-1, F)) if F else None
    args = (enc, torch.tensor(x.astype(np.float64)), table, torch.tensor(u.astype(np.float64)), mats, torch.tensor(g.astype(np.float64)), pad_value)
    return dict(c=c, x=x, u=u, g=g, p32=p32, ph=ph, shapes=shapes, n_mlp=n_mlp, truth=S.truth(*args), model=S.model(*args, rounded=True))


def quantities(k):
    """(name, key, slice of the parameter vector or None) of everything compared, per matrix and per table"""
    out, o = [("output", "y", None)], 0
    spans = []
    for l, (r, c) in enumerate(k["shapes"]):
        spans.append((l, slice(o, o + r * c)))
        o += r * c
    for tag, kw, kt, kx in (("bwd", "dW1", "dtable1", "dx1"), ("bbi", "dW", "dtable", "dx")):
        out += [(f"{tag}_dW{l}", (kw, l), sl) for l, sl in spans]
        if k["truth"][kt] is not None:
            out.append((f"{tag}_dtable", kt, slice(o, None)))
        out.append((f"{tag}_dL_dinput", kx, None))
    return out + [("bbi_dL_ddLdoutput", "ddo", None)]


def pick(d, key):
    return (d[key[0]][key[1]] if isinstance(key, tuple) else d[key]).numpy()


def _run(t, m, k, want_dx=True, want_ddo=True, want_g=True, first=True):
    """forward, backward and backward_backward_input on the device, as numpy: dict(y, dW1 (dL_dparams), dx1, dW, ddo, dx)"""
    from neus2_amd.module import GradientMode
    dev16 = lambda a: t.from_numpy(a.view(np.int16).copy()).cuda()
    params, x, u, g = dev16(k["ph"]), t.from_numpy(k["x"]).cuda(), t.from_numpy(k["u"]).cuda(), dev16(k["g"])
    n = k["x"].shape[0]
    full = lambda shape, dtype: t.full(shape, 7.0, dtype=dtype, device="cuda")
    ctx, y = m.forward(x, params, prepare_input_gradients=True)
    out = dict(y=y)
    if first:
        out["g1"], out["dx1"] = full((m.n_params,), t.float32), full((n, m.n_input_dims), t.float32)
        m.backward(ctx, x, g, params, dL_dparams=out["g1"], dL_dinput=out["dx1"], mode=GradientMode.Overwrite, output=y)
    out["g2"] = full((m.n_params,), t.float32) if want_g else None
    out["ddo"] = full((n, m.n_output_dims), t.float16) if want_ddo else None
    out["dx"] = full((n, m.n_input_dims), t.float32) if want_dx else None
    m.backward_backward_input(ctx, x, u, g, params, dL_dparams=out["g2"], dL_ddLdoutput=out["ddo"],
                              mode=GradientMode.Overwrite if want_g else GradientMode.Ignore, dL_dinput=out["dx"])
    t.cuda.synchronize()
    return {key: None if a is None else a.cpu().numpy() for key, a in out.items()}


def device_value(got, what, key, sl):
    if sl is not None:
        return got["g1" if what.startswith("bwd") else "g2"][sl]
    return got[{"y": "y", "dx1": "dx1", "dx": "dx", "ddo": "ddo"}[key]].astype(np.float32)


@pytest.mark.parametrize("name", list(CASES))
def test_siren_parity(torch_cuda, name):
    t = torch_cuda
    k = case(name)
    m = _module(name)
    assert m.n_params == k["ph"].size
    got = _run(t, m, k)
    failures = []
    for what, key, sl in quantities(k):
        truth, model = pick(k["truth"], key), pick(k["model"], key)
        assert np.abs(truth).max() > 0, what
        floor = A.rel(model, truth)
        rel, cos = R.rel_cos(device_value(got, what, key, sl), truth)
        bound = min(FACTOR * floor, CEIL_REL)
        R.record(f"siren_{name}_{what}", rel=rel, one_minus_cos=1 - cos, floor=floor)
        print(f"{name} {what}: rel {rel:.3e} floor {floor:.3e} bound {bound:.3e} 1-cos {1 - cos:.3e}")
        if not floor <= MAX_FLOOR:
            failures.append((what, "floor", floor))
        if not (rel <= bound and cos >= MIN_COS):
            failures.append((what, rel, floor, bound, cos))
    assert not failures, failures


def test_sine_and_cosine_over_every_fp16_argument(torch_cuda):
    """Identity matrices make z = x exactly: the output is sin(x) as stored, and the first backward's dL_dinput with
    dL_doutput = 1 is cos(x) as kept, for all 63,488 finite fp16 values x (|x| <= 65504). Bound: 2^-11 absolute, one fp16 ulp
    in [0.5, 1): half an ulp for the rounding to fp16 and as much again for the evaluation, whose hardware sine and cosine
    are good to about 2^-17. An argument reduced with a single fp32 product is off by up to 3e-3 rad at 65504."""
    from neus2_amd.module import GradientMode, Module
    t = torch_cuda
    bits = np.arange(1 << 16, dtype=np.uint16)
    vals = bits.view(np.float16)
    vals = vals[np.isfinite(vals)]
    assert vals.size == 63488
    n = vals.size // 16  # 3968 = 31 x 128 samples of 16 inputs
    x = vals.reshape(n, 16).astype(np.float32)
    m = Module.create_network(16, 16, _net_cfg(dict(W=16, N=1), None), batch_capacity=n)
    eye = np.eye(16, dtype=np.float16)
    params = t.from_numpy(np.concatenate([eye.ravel(), eye.ravel()]).view(np.int16).copy()).cuda()
    xd = t.from_numpy(x).cuda()
    ctx, y = m.forward(xd, params, prepare_input_gradients=True)
    dx = t.zeros((n, 16), dtype=t.float32, device="cuda")
    m.backward(ctx, xd, t.ones((n, 16), dtype=t.float16, device="cuda"), params, dL_dinput=dx, mode=GradientMode.Ignore, output=y)
    t.cuda.synchronize()
    es = np.abs(y.cpu().numpy().astype(np.float64) - np.sin(x.astype(np.float64)))
    ec = np.abs(dx.cpu().numpy().astype(np.float64) - np.cos(x.astype(np.float64)))
    R.record("siren_sincos_all_fp16", max_abs_sin=es.max(), max_abs_cos=ec.max())
    print(f"max |sin - truth| {es.max():.3e} at {x.ravel()[es.argmax()]}, max |cos - truth| {ec.max():.3e} at {x.ravel()[ec.argmax()]}")
    assert es.max() <= 2.0 ** -11 and ec.max() <= 2.0 ** -11


@pytest.mark.parametrize("name", ["w64", "w256"])
def test_inference_is_the_forward(torch_cuda, name):
    t = torch_cuda
    k = case(name)
    m = _module(name)
    params, x = t.from_numpy(k["ph"].view(np.int16).copy()).cuda(), t.from_numpy(k["x"]).cuda()
    _, y = m.forward(x, params, prepare_input_gradients=True)
    yi = m.inference(x, params)
    t.cuda.synchronize()
    np.testing.assert_array_equal(y.cpu().numpy().view(np.uint16), yi.cpu().numpy().view(np.uint16))
    assert np.abs(y.cpu().numpy().astype(np.float32)).max() > 0


@pytest.mark.parametrize("name", BITWISE)
def test_repeatable_and_null_pointers(torch_cuda, name):
    t = torch_cuda
    k = case(name)
    m = _module(name)
    a, b = _run(t, m, k), _run(t, m, k)
    for key in a:
        np.testing.assert_array_equal(a[key].view(np.uint8), b[key].view(np.uint8))
    # dL_ddLdoutput alone (Ignore), dL_dinput alone: bitwise the full call's
    only = _run(t, m, k, want_dx=False, want_g=False, first=False)
    np.testing.assert_array_equal(only["ddo"].view(np.uint16), a["ddo"].view(np.uint16))
    only = _run(t, m, k, want_ddo=False, want_g=False, first=False)
    np.testing.assert_array_equal(only["dx"].view(np.uint8), a["dx"].view(np.uint8))
    # all three null: nothing to do, and no error
    none = _run(t, m, k, want_dx=False, want_ddo=False, want_g=False, first=False)
    assert none["g2"] is None and none["ddo"] is None and none["dx"] is None


def test_general_grid_repeats_but_for_its_table(torch_cuda):
    t = torch_cuda
    k = case("grid2_w32")
    m = _module("grid2_w32")
    a, b = _run(t, m, k), _run(t, m, k)
    n_mlp = k["n_mlp"]
    for key in a:
        p, q = (a[key][:n_mlp], b[key][:n_mlp]) if key in ("g1", "g2") else (a[key], b[key])
        np.testing.assert_array_equal(p.view(np.uint8), q.view(np.uint8))


def test_a_context_without_the_cosine_is_refused(torch_cuda):
    """a context of another module's forward has activations but no cos z: refused on the host, nothing launched"""
    from neus2_amd import NeusError
    from neus2_amd.module import GradientMode
    t = torch_cuda
    k = case("w64")
    sine, other = _module("w64"), _module("w64", activation="ReLU")
    dev16 = lambda a: t.from_numpy(a.view(np.int16).copy()).cuda()
    params, x, u, g = dev16(k["ph"]), t.from_numpy(k["x"]).cuda(), t.from_numpy(k["u"]).cuda(), dev16(k["g"])
    ctx, y = other.forward(x, params, prepare_input_gradients=True)
    gp = t.zeros(sine.n_params, dtype=t.float32, device="cuda")
    with pytest.raises(NeusError, match="not from this module's forward"):
        sine.backward(ctx, x, g, params, dL_dparams=gp, mode=GradientMode.Overwrite, output=y)
    with pytest.raises(NeusError, match="needs the forward's context"):
        sine.backward_backward_input(ctx, x, u, g, params, dL_dparams=gp, mode=GradientMode.Overwrite)
    other.backward(ctx, x, g, params, dL_dparams=gp, mode=GradientMode.Overwrite, output=y)  # its own module takes it
    t.cuda.synchronize()
    assert bool(t.isfinite(gp).all()) and gp.abs().max().item() > 0


def test_default_mode_keeps_its_refusal(torch_cuda):
    from neus2_amd import NeusError
    t = torch_cuda
    k = case("w64")
    for so in (None, "tcnn"):
        with pytest.raises(NeusError, match="ReLU or None"):
            _run(t, _module("w64", so), k, want_ddo=False, first=False)
        with pytest.raises(NeusError, match="ReLU or None"):
            _run(t, _module("w64", so), k, want_dx=False, first=False)
    g0 = _run(t, _module("w64", "tcnn"), k, want_dx=False, want_ddo=False, first=False)["g2"]
    ge = _run(t, _module("w64"), k, want_dx=False, want_ddo=False, first=False)["g2"]
    assert np.isfinite(g0).all() and np.abs(g0).max() > 0 and A.rel(g0, ge) > 1e-2  # the default chain has no act'' term


@pytest.mark.parametrize("name", ["w64", "w256", "hashgrid_w16", "grid2_w32"])
def test_initialize_params_is_the_restatement(torch_cuda, name):
    k = case(name)
    p32 = _module(name).initialize_params(seed=CASES[name]["seed"]).cpu().numpy()
    np.testing.assert_array_equal(p32.view(np.uint32), k["p32"].view(np.uint32))
    bounds = S.siren_bounds(k["shapes"])
    assert bounds[0] == np.float32(30.0 / k["shapes"][0][1]) and np.abs(p32[:k["shapes"][0][0] * k["shapes"][0][1]]).max() > 0.9 * bounds[0]


def test_config(torch_cuda):
    from neus2_amd import NeusError
    from neus2_amd.module import Module
    net = _module("w64").hyperparams()["network"]
    assert net["otype"] == "CutlassMLP" and net["activation"] == "Sine" and net["second_order"] == "exact"
    net = _module("hashgrid_w16", None).hyperparams()["network"]
    assert net["otype"] == "CutlassMLP" and net["activation"] == "Sine" and "second_order" not in net
    for W in (16, 48, 128, 144, 512):  # every kind of width the otype takes
        assert Module.create_network(3, 1, _net_cfg(dict(W=W, N=1)), batch_capacity=128).hyperparams()["network"]["activation"] == "Sine"
    for otype in ("FullyFusedMLP", "MegakernelMLP"):
        with pytest.raises(NeusError, match="Sine has no backward"):
            _module("w64", otype=otype)
    for otype in ("FullyFusedMLP", "CutlassMLP"):
        with pytest.raises(NeusError, match="output_activation"):
            _module("w64", otype=otype, activation="ReLU", output_activation="Sine")
        with pytest.raises(NeusError, match="output_activation"):
            _module("hashgrid_w16", otype=otype, activation="ReLU", output_activation="Sine")
