"""The general grid encoding (neus2_amd/csrc/grid_nd.hip) as a stand-alone operator module on the MI355X: 2 / 3 / 4 input
dims, 1 / 2 / 4 / 8 features per level, Hash / Dense / Tiled tables, Linear / Smoothstep interpolation, fp32 and fp16
tables. Forward, dL_dparams, dL_dinput and the three backward_backward_input outputs against float64 autograd of
tests/grid_nd_ref.grid_encode, n = 256.

Table values and dL_doutput are fp16-representable, so both precisions share one reference. The inputs are the first 256
of 320 candidates whose fp32 level position x * scale + 0.5 stays 1e-4 away from every integer (the derivative jumps
there); the share left out must stay <= 0.05.

Bars:
* fp32, Linear: rel-L2 <= 3e-5 and cosine >= 0.9999999 for parameter gradients, the project's fp32 grid bar
  (test_gpu_module.test_encoding_module_fp32): the position x * scale + 0.5 carries ~2^-24 scale of its fraction, and the
  scale here (<= 60) is smaller than there (~270).
* fp32, Smoothstep: 4 x the worst rel-L2 measured over the Smoothstep cases B, E, I on an MI355X (SMOOTH_MEASURED below),
  and never above 1.8e-4 = 6 x 3e-5 with 6 = max |smoothstep''|.
* fp16: each forward element within one fp16 rounding (2^-11 relative, 2^-25 absolute in the subnormals) of the float64
  value, plus the fp32 bar times the largest |value| (the fp32 error of an element scales with the table's magnitude, not
  with the element's own); dL_ddLdoutput the same; gradients (gradient_precision fp32) at the fp32 bars, because the table
  is exact in fp16.
* dL_dparams is a float-atomic sum: two calls agree within rtol 1e-5, atol 2e-5 only; everything else is bitwise
  repeatable."""
import functools

import numpy as np
import pytest

import grid_nd_ref as G

pytestmark = pytest.mark.gpu

N = 256
N_CAND = 320
MARGIN = 1e-4
LINEAR_BAR = 3e-5
# worst rel-L2 of any fp32 Smoothstep output over cases B, E, I, measured on an MI355X
SMOOTH_MEASURED = 4.113e-6  # case E, dL_dinput of backward_backward_input
SMOOTH_BAR = min(4 * SMOOTH_MEASURED, 1.8e-4)
ATOMIC_TOL = dict(rtol=1e-5, atol=2e-5)

# name -> (D, F, type, interpolation, L, log2_hashmap_size, base_resolution, per_level_scale)
CASES = {
    "A": (2, 2, "Hash", "Linear", 6, 10, 8, 1.5),
    "B": (2, 4, "Hash", "Smoothstep", 6, 10, 8, 1.5),
    "C": (3, 1, "Hash", "Linear", 6, 12, 8, 1.5),
    "D": (3, 8, "Hash", "Linear", 4, 12, 8, 1.5),
    "E": (3, 2, "Hash", "Smoothstep", 6, 12, 8, 1.5),
    "F": (4, 2, "Hash", "Linear", 4, 12, 4, 1.5),
    "G": (3, 2, "Dense", "Linear", 3, 19, 4, 2.0),
    "H": (2, 2, "Tiled", "Linear", 4, 19, 8, 2.0),
    "I": (4, 4, "Hash", "Smoothstep", 4, 12, 4, 1.5),
}


def config(case, **extra):
    D, F, ty, ip, L, log2, base, pls = CASES[case]
    cfg = {"otype": "Grid", "type": ty, "n_levels": L, "n_features_per_level": F, "base_resolution": base, "per_level_scale": pls,
           "interpolation": ip}
    if ty == "Hash":
        cfg["log2_hashmap_size"] = log2
    cfg.update(extra)
    return cfg


def tables(case):
    D, F, ty, ip, L, log2, base, pls = CASES[case]
    return G.level_tables(D, L, log2, base, pls, ty)


def inputs(case, seed=7):
    """(positions [N, D] fp32, share of candidates left out)"""
    D = CASES[case][0]
    _, res = tables(case)
    cand = np.random.default_rng(seed).uniform(0.02, 0.98, (N_CAND, D)).astype(np.float32)
    out = G.fraction_margin(cand, res) < MARGIN
    return np.ascontiguousarray(cand[~out][:N]), out.mean()


def rel_cos(x, y):
    x, y = np.asarray(x, np.float64).ravel(), np.asarray(y, np.float64).ravel()
    return np.linalg.norm(x - y) / max(np.linalg.norm(y), 1e-30), x @ y / max(np.linalg.norm(x) * np.linalg.norm(y), 1e-30)


def record(test, **metrics):
    from test_gpu_module import _record
    _record(test, **metrics)


@functools.lru_cache(maxsize=None)
def reference(case, n=N, valid=None):
    """float64 autograd of the first n inputs: every output of forward, backward and backward_backward_input. Computed
    once per (case, n, valid) and shared by the tests; the arrays are read-only."""
    import torch
    D, F, ty, ip, L, *_ = CASES[case]
    off, res = tables(case)
    pos, left_out = inputs(case)
    pos = pos[:n]
    rng = np.random.default_rng(100 + ord(case))
    table = rng.uniform(-1, 1, (off[-1], F)).astype(np.float16)
    dly = rng.normal(0, 1, (N, F * L)).astype(np.float16)[:n]
    u = rng.normal(0, 1, (N, D)).astype(np.float32)[:n]
    tab = torch.tensor(table.astype(np.float64), requires_grad=True)
    xt = torch.tensor(pos.astype(np.float64), requires_grad=True)
    dly_t = torch.tensor(dly.astype(np.float64), requires_grad=True)
    y = G.grid_encode(xt, tab, off, res, ty, ip, valid)
    g_tab, g_x = torch.autograd.grad((y * dly_t).sum(), (tab, xt), create_graph=True)
    g2_tab, g2_dly, g2_x = torch.autograd.grad((g_x * torch.tensor(u.astype(np.float64))).sum(), (tab, dly_t, xt))
    r = dict(pos=pos, table=table, dly=dly, u=u, left_out=left_out, y=y.detach().numpy(), g_tab=g_tab.detach().numpy().ravel(),
             g_x=g_x.detach().numpy(), g2_tab=g2_tab.numpy().ravel(), g2_dly=g2_dly.numpy(), g2_x=g2_x.numpy())
    for a in r.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return r


def dev(t, a):
    return t.from_numpy(a.view(np.int16).copy() if a.dtype == np.float16 else a.copy()).cuda()


def fp16_close(got, ref, bar):
    """every element within one fp16 rounding of the float64 value plus the fp32 bar (module docstring)"""
    tol = np.abs(ref) * 2.0 ** -11 + 2.0 ** -25 + bar * np.abs(ref).max()
    return np.abs(np.asarray(got, np.float64) - ref) <= tol


def create(case, precision, capacity=N, **extra):
    from neus2_amd.module import Module, Precision
    D = CASES[case][0]
    return Module.create_encoding(config(case, gradient_precision="fp32", **extra), batch_capacity=capacity, n_input_dims=D,
                                  requested_precision=Precision.Fp32 if precision == "fp32" else Precision.Fp16)


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_grid_nd_module(torch_cuda, precision, case):
    from neus2_amd.module import GradientMode
    t = torch_cuda
    D, F, ty, ip, L, *_ = CASES[case]
    f32 = precision == "fp32"
    smooth = ip == "Smoothstep"
    bar = SMOOTH_BAR if smooth else LINEAR_BAR
    off, res = tables(case)
    m = create(case, precision)
    hp = m.hyperparams()
    assert m.n_params == off[-1] * F and m.n_input_dims == D and m.n_output_dims == F * L and m.info["n_levels"] == L
    assert (hp["n_input_dims"], hp["n_features_per_level"], hp["type"], hp["interpolation"]) == (D, F, ty, ip)
    assert hp["precision"] == precision and m.output_shape(N) == (N, F * L)
    p0 = m.initialize_params(3).cpu().numpy()
    assert p0.size == m.n_params and 0 < np.abs(p0).max() <= 1e-4
    r = reference(case)
    print(f"case {case} {precision}: share of candidates left out {r['left_out']:.4f}")
    assert r["left_out"] <= 0.05 and r["pos"].shape[0] == N
    dt = np.float32 if f32 else np.float16
    tdt = t.float32 if f32 else t.float16
    params, x, u = dev(t, r["table"].ravel().astype(dt)), dev(t, r["pos"]), dev(t, r["u"])
    dly = dev(t, r["dly"].astype(dt))
    if not f32:
        params, dly = params.view(t.float16), dly.view(t.float16)
    ctx, y = m.forward(x, params, prepare_input_gradients=True)
    assert y.dtype == tdt and tuple(y.shape) == (N, F * L)
    g = t.full((m.n_params,), 7.0, dtype=t.float32, device="cuda")  # Overwrite must not read the old contents
    dx = t.full((N, D), 7.0, dtype=t.float32, device="cuda")
    m.backward(ctx, x, dly, params, dL_dparams=g, dL_dinput=dx, mode=GradientMode.Overwrite)
    g2 = t.full((m.n_params,), -5.0, dtype=t.float32, device="cuda")
    ddo = t.full((N, F * L), 7.0, dtype=tdt, device="cuda")
    ddx = t.full((N, D), 7.0, dtype=t.float32, device="cuda")
    m.backward_backward_input(ctx, x, u, dly, params, dL_dparams=g2, dL_ddLdoutput=ddo, mode=GradientMode.Overwrite, dL_dinput=ddx)
    yn, ddon = y.float().cpu().numpy(), ddo.float().cpu().numpy()
    met = {}
    met["rel_forward"], _ = rel_cos(yn, r["y"])
    met["rel_params"], met["cos_params"] = rel_cos(g.cpu().numpy(), r["g_tab"])
    met["rel_dinput"], _ = rel_cos(dx.cpu().numpy(), r["g_x"])
    met["rel_params_2nd"], met["cos_params_2nd"] = rel_cos(g2.cpu().numpy(), r["g2_tab"])
    met["rel_ddLdoutput"], _ = rel_cos(ddon, r["g2_dly"])
    met["rel_dinput_2nd"], _ = rel_cos(ddx.cpu().numpy(), r["g2_x"])
    record(f"grid_nd_{case}_{precision}", left_out=r["left_out"], **met)
    print(f"case {case} {precision}:", {k: f"{v:.3e}" if k.startswith("rel") else f"1-{1 - v:.1e}" for k, v in met.items()})
    if f32:
        assert met["rel_forward"] <= bar and met["rel_ddLdoutput"] <= bar, met
    else:
        assert fp16_close(yn, r["y"], bar).all(), np.abs(yn - r["y"]).max()
        assert fp16_close(ddon, r["g2_dly"], bar).all(), np.abs(ddon - r["g2_dly"]).max()
    for k in ("rel_params", "rel_dinput", "rel_params_2nd", "rel_dinput_2nd"):
        assert met[k] <= bar, (k, met)
    assert met["cos_params"] >= 0.9999999 and met["cos_params_2nd"] >= 0.9999999, met
    # repeatability: everything but the float-atomic parameter gradients is bitwise the same on a second call
    _, y_b = m.forward(x, params, prepare_input_gradients=True)
    assert t.equal(y_b, y) and t.equal(m.inference(x, params), y)
    g_b = t.full((m.n_params,), 1.0, dtype=t.float32, device="cuda")
    dx_b = t.full((N, D), -3.0, dtype=t.float32, device="cuda")
    m.backward(ctx, x, dly, params, dL_dparams=g_b, dL_dinput=dx_b, mode=GradientMode.Overwrite)
    assert t.equal(dx_b, dx)
    np.testing.assert_allclose(g_b.cpu().numpy(), g.cpu().numpy(), **ATOMIC_TOL)
    # Ignore: dL_dparams untouched, the other outputs the same
    keep = t.full((m.n_params,), 2.5, dtype=t.float32, device="cuda")
    ddo_b = t.full((N, F * L), -3.0, dtype=tdt, device="cuda")
    ddx_b = t.full((N, D), -3.0, dtype=t.float32, device="cuda")
    m.backward_backward_input(ctx, x, u, dly, params, dL_dparams=keep, dL_ddLdoutput=ddo_b, mode=GradientMode.Ignore, dL_dinput=ddx_b)
    assert t.equal(ddo_b, ddo) and t.equal(ddx_b, ddx)
    assert (keep == 2.5).all().item()
    m.backward(ctx, x, dly, params, dL_dparams=keep, mode=GradientMode.Ignore)
    assert (keep == 2.5).all().item()
    # Accumulate adds: the second-order gradient onto the first-order one
    acc = g.clone()
    m.backward_backward_input(ctx, x, u, dly, params, dL_dparams=acc, mode=GradientMode.Accumulate)
    np.testing.assert_allclose(acc.cpu().numpy(), g.cpu().numpy() + g2.cpu().numpy(), **ATOMIC_TOL)


@pytest.mark.parametrize("layout", ["SoA"])
def test_grid_nd_soa_and_fp16_gradients(torch_cuda, layout):
    """output_layout SoA ([F L, n] tensors) equals the AoS results transposed, bitwise; the default gradient precision of an
    fp16 module is fp16: the fp32 gradient rounded once (within the atomics' tolerance)."""
    from neus2_amd.module import GradientMode, Module, Precision
    t = torch_cuda
    case = "B"
    D, F, ty, ip, L, *_ = CASES[case]
    r = reference(case)
    a = create(case, "fp16")
    b = create(case, "fp16", output_layout=layout)
    assert b.output_layout == "SoA" and b.output_shape(N) == (F * L, N)
    params, x, u = dev(t, r["table"].ravel()).view(t.float16), dev(t, r["pos"]), dev(t, r["u"])
    dly = dev(t, r["dly"]).view(t.float16)
    dly_s = dly.T.contiguous()
    ca, ya = a.forward(x, params)
    cb, yb = b.forward(x, params)
    assert t.equal(yb.T, ya)
    dxa, dxb = t.zeros((N, D), device="cuda"), t.zeros((N, D), device="cuda")
    a.backward(ca, x, dly, params, dL_dinput=dxa, mode=GradientMode.Ignore)
    b.backward(cb, x, dly_s, params, dL_dinput=dxb, mode=GradientMode.Ignore)
    assert t.equal(dxa, dxb)
    oa, ob = t.zeros((N, F * L), dtype=t.float16, device="cuda"), t.zeros((F * L, N), dtype=t.float16, device="cuda")
    a.backward_backward_input(ca, x, u, dly, params, dL_ddLdoutput=oa, mode=GradientMode.Ignore, dL_dinput=dxa)
    b.backward_backward_input(cb, x, u, dly_s, params, dL_ddLdoutput=ob, mode=GradientMode.Ignore, dL_dinput=dxb)
    assert t.equal(ob.T, oa) and t.equal(dxa, dxb)
    h = Module.create_encoding(config(case), batch_capacity=N, n_input_dims=D, requested_precision=Precision.Fp16)
    assert h.gradient_precision == "fp16"
    g16 = h.gradient_buffer()
    ch, _ = h.forward(x, params)
    h.backward(ch, x, dly, params, dL_dparams=g16, mode=GradientMode.Overwrite)
    assert g16.dtype == t.float16
    ref = r["g_tab"]
    np.testing.assert_allclose(g16.float().cpu().numpy(), ref, rtol=2.0 ** -10, atol=2e-5 + SMOOTH_BAR * np.abs(ref).max())


@pytest.mark.parametrize("n", [1, 200])
def test_grid_nd_batch_sizes(torch_cuda, n):
    """Any n <= batch_capacity on the stand-alone encoding (one lane per sample and level: a partial last block)."""
    from neus2_amd.module import GradientMode
    t = torch_cuda
    case = "A"
    D, F, ty, ip, L, *_ = CASES[case]
    r = reference(case, n)
    m = create(case, "fp32")
    params, x, u, dly = dev(t, r["table"].ravel().astype(np.float32)), dev(t, r["pos"]), dev(t, r["u"]), dev(t, r["dly"].astype(np.float32))
    ctx, y = m.forward(x, params, prepare_input_gradients=True)
    assert tuple(y.shape) == (n, F * L)
    g, dx = t.full((m.n_params,), 7.0, device="cuda"), t.full((n, D), 7.0, device="cuda")
    m.backward(ctx, x, dly, params, dL_dparams=g, dL_dinput=dx, mode=GradientMode.Overwrite)
    g2, ddo, ddx = t.full((m.n_params,), 7.0, device="cuda"), t.full((n, F * L), 7.0, device="cuda"), t.full((n, D), 7.0, device="cuda")
    m.backward_backward_input(ctx, x, u, dly, params, dL_dparams=g2, dL_ddLdoutput=ddo, mode=GradientMode.Overwrite, dL_dinput=ddx)
    got = dict(y=y, g_tab=g, g_x=dx, g2_tab=g2, g2_dly=ddo, g2_x=ddx)
    for k, v in got.items():
        rel, _ = rel_cos(v.cpu().numpy(), r[k])
        assert rel <= LINEAR_BAR, (n, k, rel)


def test_grid_nd_progressive_levels(torch_cuda):
    """set_training_step(1) with tcnn's defaults: valid level ceil(0.5 * 6) = 3, so levels 0..3 of case C are active; the
    upper two output zeros and receive no gradient."""
    from neus2_amd.module import GradientMode
    t = torch_cuda
    case = "C"
    D, F, ty, ip, L, *_ = CASES[case]
    off, _ = tables(case)
    full, r = reference(case), reference(case, N, 3)
    m = create(case, "fp32")
    params, x, u, dly = dev(t, r["table"].ravel().astype(np.float32)), dev(t, r["pos"]), dev(t, r["u"]), dev(t, r["dly"].astype(np.float32))
    _, y_full = m.forward(x, params)
    m.set_training_step(1)
    ctx, y = m.forward(x, params, prepare_input_gradients=True)
    yn = y.cpu().numpy()
    assert not yn[:, 4 * F:].any() and np.array_equal(yn[:, :4 * F], y_full.cpu().numpy()[:, :4 * F])
    assert full["y"][:, 4 * F:].any()
    g, dx = t.full((m.n_params,), 7.0, device="cuda"), t.full((N, D), 7.0, device="cuda")
    m.backward(ctx, x, dly, params, dL_dparams=g, dL_dinput=dx, mode=GradientMode.Overwrite)
    g2, ddo, ddx = t.full((m.n_params,), 7.0, device="cuda"), t.full((N, F * L), 7.0, device="cuda"), t.full((N, D), 7.0, device="cuda")
    m.backward_backward_input(ctx, x, u, dly, params, dL_dparams=g2, dL_ddLdoutput=ddo, mode=GradientMode.Overwrite, dL_dinput=ddx)
    assert not g.cpu().numpy()[off[4] * F:].any() and not g2.cpu().numpy()[off[4] * F:].any()
    assert not ddo.cpu().numpy()[:, 4 * F:].any()
    for k, v in dict(y=y, g_tab=g, g_x=dx, g2_tab=g2, g2_dly=ddo, g2_x=ddx).items():
        rel, _ = rel_cos(v.cpu().numpy(), r[k])
        assert rel <= LINEAR_BAR, (k, rel)


def test_grid_nd_parity_with_the_3d_kernels(torch_cuda):
    """The config of test_gpu_module.test_encoding_module_fp32 as it is (grid_f32.hip) and with "implementation": "general"
    (grid_nd.hip): n_params and initialize_params bitwise; forward and dL_dinput to rel-L2 <= 1e-6 (the fraction and the
    weights are identical, only the order of an 8-term fp32 sum differs); parameter gradients within the atomics' tolerance."""
    from neus2_amd.module import GradientMode, Module, Precision
    t = torch_cuda
    n, L = 1024, 8
    cfg = {"otype": "HashGrid", "n_levels": L, "n_features_per_level": 2, "log2_hashmap_size": 14, "base_resolution": 16,
           "per_level_scale": 1.5, "output_layout": "AoS"}
    a = Module.create_encoding(cfg, batch_capacity=n, requested_precision=Precision.Fp32)
    b = Module.create_encoding(dict(cfg, implementation="general"), batch_capacity=n, requested_precision=Precision.Fp32)
    assert a.name() == "HashGrid" and b.name() == "Grid" and b.hyperparams()["type"] == "Hash"
    assert a.n_params == b.n_params and a.n_output_dims == b.n_output_dims == 2 * L
    assert t.equal(a.initialize_params(1337), b.initialize_params(1337))
    rng = np.random.default_rng(19)
    params = t.from_numpy(rng.uniform(-1, 1, a.n_params).astype(np.float32)).cuda()
    x = t.from_numpy(rng.uniform(0.02, 0.98, (n, 3)).astype(np.float32)).cuda()
    dly = t.from_numpy(rng.normal(0, 1, (n, 2 * L)).astype(np.float32)).cuda()
    out = []
    for m in (a, b):
        ctx, y = m.forward(x, params, prepare_input_gradients=True)
        g, dx = t.zeros(m.n_params, device="cuda"), t.zeros((n, 3), device="cuda")
        m.backward(ctx, x, dly, params, dL_dparams=g, dL_dinput=dx, mode=GradientMode.Overwrite)
        out.append((y.cpu().numpy(), dx.cpu().numpy(), g.cpu().numpy()))
    rel_y, _ = rel_cos(out[1][0], out[0][0])
    rel_x, _ = rel_cos(out[1][1], out[0][1])
    record("grid_nd_parity_3d", rel_forward=rel_y, rel_dinput=rel_x)
    print(f"parity: forward rel {rel_y:.3e}, dL_dinput rel {rel_x:.3e}")
    assert rel_y <= 1e-6 and rel_x <= 1e-6, (rel_y, rel_x)
    np.testing.assert_allclose(out[1][2], out[0][2], **ATOMIC_TOL)


def test_grid_nd_refusals(torch_cuda):
    from neus2_amd import NeusError
    from neus2_amd.module import Module, Precision
    enc = lambda case, d, **kw: Module.create_encoding(config(case, **kw), batch_capacity=N, n_input_dims=d)
    with pytest.raises(NeusError, match="Nearest"):
        enc("A", 2, interpolation="Nearest")
    with pytest.raises(NeusError, match="stochastic_interpolation"):
        enc("A", 2, stochastic_interpolation=True)
    with pytest.raises(NeusError, match="n_input_dims must be 2, 3 or 4"):
        enc("A", 5)
    with pytest.raises(NeusError, match="n_features_per_level must be 1, 2, 4 or 8"):
        enc("A", 2, n_features_per_level=3)
    with pytest.raises(NeusError, match="paired"):
        enc("A", 2, output_layout="paired")
    with pytest.raises(NeusError, match="paired"):
        Module.create_encoding(config("A", output_layout="paired"), batch_capacity=N, n_input_dims=2, requested_precision=Precision.Fp32)
    # Dense, 3-D, base 1024 doubling: level 1 alone is 2047^3 > 2^31 entries; refused on the host, before any allocation
    with pytest.raises(NeusError, match="Dense grid: the table would exceed 2\\^31 entries"):
        Module.create_encoding({"otype": "DenseGrid", "n_levels": 2, "n_features_per_level": 2, "base_resolution": 1024, "per_level_scale": 2.0},
                               batch_capacity=N, n_input_dims=3)
    net = {"otype": "FullyFusedMLP", "n_neurons": 64, "n_hidden_layers": 2, "activation": "ReLU", "output_activation": "None"}
    # 17 levels of 8 features: the width check of a network's encoding comes before the level count's
    with pytest.raises(NeusError, match="encoded width .* exceeds the 128"):
        Module.create_network_with_input_encoding(2, 16, config("B", n_levels=17, n_features_per_level=8), net, batch_capacity=N)
    # a type or an implementation the factory does not know names itself
    with pytest.raises(NeusError, match="type must be Hash, Dense or Tiled"):
        enc("A", 2, type="Sparse")
    with pytest.raises(NeusError, match="implementation must be auto or general"):
        enc("A", 2, implementation="fast")
