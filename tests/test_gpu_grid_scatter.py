""""gradient_scatter": "binned" of the general grid (neus2_amd/csrc/grid_nd_scatter.hip) on the MI355X: dL_dparams of backward
and of backward_backward_input as int64 fixed-point sums (resolution 2^-32) converted to fp32 once, so that the result is
bitwise independent of the order of the samples, of the batch capacity and of scheduling.

* exact: the cases of tests/grid_scatter_cases.py, where every fp32 sum in any order is exact: bitwise equal to the
  contract's reference, for "binned" and for "atomic" alike (the case, not a tolerance, carries the test);
* rounded once: exact contributions whose sum spans more than 24 bits give the exact sum's fp32 rounding, in any order;
* parity: cases A - I of test_gpu_grid_nd.py with "binned", all six outputs at that file's own bars (the fixed point adds
  at most 2^-33 per contribution);
* order independence, progressive levels, non-finite contributions and the config key."""
import numpy as np
import pytest

import grid_scatter_cases as S
from test_gpu_grid_nd import CASES, LINEAR_BAR, SMOOTH_BAR, config, create, dev, reference, rel_cos, tables

pytestmark = pytest.mark.gpu

N = 256


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def x_create(case, precision, n, **extra):
    from neus2_amd.module import Module, Precision
    D = S.X_CASES[case][0][0]
    return Module.create_encoding(S.x_config(case, gradient_precision="fp32", **extra), batch_capacity=(n + 127) // 128 * 128, n_input_dims=D,
                                  requested_precision=Precision.Fp32 if precision == "fp32" else Precision.Fp16)


def operands(t, r, precision):
    """params, x, dL_doutput, u of a reference dict on the device, in the module's precision"""
    dt = np.float32 if precision == "fp32" else np.float16
    params, dly = dev(t, r["table"].ravel().astype(dt)), dev(t, r["dly"].astype(dt))
    if precision != "fp32":
        params, dly = params.view(t.float16), dly.view(t.float16)
    return params, dev(t, r["pos"]), dly, dev(t, r["u"])


def both_gradients(t, m, params, x, dly, u, fill=float("nan")):
    """dL_dparams of backward and of backward_backward_input, Overwrite into buffers filled with `fill`"""
    from neus2_amd.module import GradientMode
    ctx, _ = m.forward(x, params, prepare_input_gradients=True)
    g = t.full((m.n_params,), fill, dtype=t.float32, device="cuda")
    g2 = t.full((m.n_params,), fill, dtype=t.float32, device="cuda")
    m.backward(ctx, x, dly, params, dL_dparams=g, mode=GradientMode.Overwrite)
    m.backward_backward_input(ctx, x, u, dly, params, dL_dparams=g2, mode=GradientMode.Overwrite)
    return g.cpu().numpy(), g2.cpu().numpy()


@pytest.mark.parametrize("n", [S.N, 1])
@pytest.mark.parametrize("precision", ["fp32", "fp16"])
@pytest.mark.parametrize("case", list(S.X_CASES))
def test_exact(torch_cuda, case, precision, n):
    t = torch_cuda
    r = S.x_reference(case, n)
    args = operands(t, r, precision)
    for scatter in ("binned", "atomic"):
        m = x_create(case, precision, n, gradient_scatter=scatter)
        assert m.gradient_scatter == scatter
        for call in range(2):
            g, g2 = both_gradients(t, m, *args)
            assert same_bits(g, r["g_tab"]), (scatter, call, np.abs(g - r["g_tab"]).max())
            assert same_bits(g2, r["g2_tab"]), (scatter, call, np.abs(g2 - r["g2_tab"]).max())


def test_sum_is_rounded_once(torch_cuda):
    """Four identical rows of case X1 (fraction 3/4, corner weights 9/16, 3/16, 3/16, 1/16), dL_doutput 32768 in one row and
    2^-10 in three: every contribution is exact, their sum spans more than 24 bits. The exact sum rounded once to fp32 is
    what the contract gives, in any order; a chain of fp32 adds that starts from the large term loses the three small ones
    (each below half an ulp of it), so here the case separates the two paths."""
    t = torch_cuda
    case = "X1"
    (D, F, ty, ip, L, log2, base, pls), _ = S.X_CASES[case]
    off, res = S.x_tables(case)
    pos = np.repeat(S.x_inputs(case)[0][:1], 4, axis=0)
    dly = np.zeros((4, F * L), np.float32)
    dly[:, 0] = [32768.0, 2.0 ** -10, 2.0 ** -10, 2.0 ** -10]
    u = np.ones((4, D), np.float32)
    idx, val = S.contributions(pos, dly, u, off, res, F, ty, ip, False)
    exact = np.zeros(off[-1] * F)
    np.add.at(exact, idx, val.astype(np.float64))
    want = S.fixed_point_sum(idx, val, off[-1] * F)
    assert same_bits(want, exact.astype(np.float32))
    chain = np.float32(9 / 16 * 32768.0)
    for _ in range(3):
        chain = np.float32(chain + np.float32(9 / 16 * 2.0 ** -10))
    assert chain == 18432.0 and want.max() == np.float32(18432.0 + 2.0 ** -9)
    m = x_create(case, "fp32", 4, gradient_scatter="binned")
    params = dev(t, np.zeros(m.n_params, np.float32))
    for order in ([0, 1, 2, 3], [3, 2, 1, 0], [1, 0, 3, 2]):
        g, _ = both_gradients(t, m, params, dev(t, pos), dev(t, dly[order]), dev(t, u))
        assert same_bits(g, want), order


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_parity(torch_cuda, precision, case):
    from neus2_amd.module import GradientMode
    from test_gpu_grid_nd import fp16_close
    t = torch_cuda
    D, F, ty, ip, L, *_ = CASES[case]
    f32 = precision == "fp32"
    bar = SMOOTH_BAR if ip == "Smoothstep" else LINEAR_BAR
    r = reference(case)
    assert r["left_out"] <= 0.05 and r["pos"].shape[0] == N
    m = create(case, precision, gradient_scatter="binned")
    params, x, dly, u = operands(t, r, precision)
    tdt = t.float32 if f32 else t.float16
    ctx, y = m.forward(x, params, prepare_input_gradients=True)
    g = t.full((m.n_params,), 7.0, dtype=t.float32, device="cuda")
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
    print(f"binned case {case} {precision}:", {k: f"{v:.3e}" if k.startswith("rel") else f"1-{1 - v:.1e}" for k, v in met.items()})
    if f32:
        assert met["rel_forward"] <= bar and met["rel_ddLdoutput"] <= bar, met
    else:
        assert fp16_close(yn, r["y"], bar).all() and fp16_close(ddon, r["g2_dly"], bar).all()
    for k in ("rel_params", "rel_dinput", "rel_params_2nd", "rel_dinput_2nd"):
        assert met[k] <= bar, (k, met)
    assert met["cos_params"] >= 0.9999999 and met["cos_params_2nd"] >= 0.9999999, met


ORDER_CFG = {"otype": "Grid", "type": "Hash", "n_levels": 4, "n_features_per_level": 4, "log2_hashmap_size": 8, "base_resolution": 8,
             "per_level_scale": 1.5, "interpolation": "Smoothstep", "gradient_precision": "fp32", "gradient_scatter": "binned"}
ORDER_N = 2176


def test_order_independence(torch_cuda):
    """One non-exact case (3-D, 4 features, 256-entry hashed levels, Smoothstep, n = 2176, normal dL_doutput and u): both
    parameter gradients are bitwise the same over repeated calls, for another batch capacity and for permuted rows;
    Accumulate is one fp32 add onto the prior buffer and Ignore leaves it alone."""
    from neus2_amd.module import GradientMode, Module, Precision
    t = torch_cuda
    n, D, F, L = ORDER_N, 3, 4, 4
    rng = np.random.default_rng(77)
    pos = rng.uniform(0.02, 0.98, (n, D)).astype(np.float32)
    dly = rng.normal(0, 1, (n, F * L)).astype(np.float32)
    u = rng.normal(0, 1, (n, D)).astype(np.float32)
    make = lambda cap: Module.create_encoding(ORDER_CFG, batch_capacity=cap, n_input_dims=D, requested_precision=Precision.Fp32)
    m = make(n)
    params = t.from_numpy(rng.uniform(-1, 1, m.n_params).astype(np.float32)).cuda()
    args = (params, dev(t, pos), dev(t, dly), dev(t, u))
    g, g2 = both_gradients(t, m, *args)
    assert np.isfinite(g).all() and np.isfinite(g2).all() and g.any() and g2.any()
    for call in range(2):
        gb, g2b = both_gradients(t, m, *args, fill=3.0)
        assert same_bits(gb, g) and same_bits(g2b, g2), call
    gc, g2c = both_gradients(t, make(8192), *args)
    assert same_bits(gc, g) and same_bits(g2c, g2)
    perm = np.random.default_rng(78).permutation(n)
    gp, g2p = both_gradients(t, m, params, dev(t, pos[perm]), dev(t, dly[perm]), dev(t, u[perm]))
    assert same_bits(gp, g) and same_bits(g2p, g2)
    # Accumulate: prior + result, one fp32 add per parameter; Ignore: untouched
    ctx, _ = m.forward(args[1], params, prepare_input_gradients=True)
    prior = rng.normal(0, 1, m.n_params).astype(np.float32)
    for second, want in ((False, g), (True, g2)):
        acc, keep = dev(t, prior), dev(t, prior)
        if second:
            m.backward_backward_input(ctx, args[1], args[3], args[2], params, dL_dparams=acc, mode=GradientMode.Accumulate)
            m.backward_backward_input(ctx, args[1], args[3], args[2], params, dL_dparams=keep, mode=GradientMode.Ignore)
        else:
            m.backward(ctx, args[1], args[2], params, dL_dparams=acc, mode=GradientMode.Accumulate)
            m.backward(ctx, args[1], args[2], params, dL_dparams=keep, mode=GradientMode.Ignore)
        assert same_bits(acc.cpu().numpy(), prior + want), second
        assert same_bits(keep.cpu().numpy(), prior), second


def test_progressive_levels(torch_cuda):
    """Case C after set_training_step(1): levels 0..3 are active; the blocks of levels 4 and 5 are exact zeros in both
    gradients (Overwrite into NaN), the rest at LINEAR_BAR."""
    t = torch_cuda
    case = "C"
    F = CASES[case][1]
    off, _ = tables(case)
    r = reference(case, N, 3)
    m = create(case, "fp32", gradient_scatter="binned")
    m.set_training_step(1)
    g, g2 = both_gradients(t, m, *operands(t, r, "fp32"))
    for got, key in ((g, "g_tab"), (g2, "g2_tab")):
        assert not bits(got[off[4] * F:]).any(), key
        rel, _ = rel_cos(got, r[key])
        assert rel <= LINEAR_BAR, (key, rel)


def test_non_finite(torch_cuda):
    """Case A, one row's dL_doutput +inf in one level's columns: exactly the entries that row touches in that level are NaN
    (a GradScaler-style check still sees the overflow), every other entry is bitwise what the row's zeroed dL_doutput gives."""
    import torch
    import grid_nd_ref as G
    t = torch_cuda
    case, row, level = "A", 37, 2
    D, F, ty, ip, L, *_ = CASES[case]
    off, res = tables(case)
    r = reference(case)
    m = create(case, "fp32", gradient_scatter="binned")
    params, x, _, u = operands(t, r, "fp32")
    dly_inf, dly_zero = r["dly"].astype(np.float32), r["dly"].astype(np.float32)
    dly_inf[row, level * F:(level + 1) * F] = np.inf
    dly_zero[row, level * F:(level + 1) * F] = 0
    # the entries of `row` in `level`, by the reference's index
    p = r["pos"][row].astype(np.float32) * np.float32(res[level] - 1) + np.float32(0.5)
    corner = np.floor(p).astype(np.int64)
    cells = torch.tensor([[corner[d] + ((c >> d) & 1) for d in range(D)] for c in range(1 << D)])
    entries = np.unique(G.index(off[level + 1] - off[level], res[level], cells, ty).numpy()) + off[level]
    touched = np.zeros(off[-1] * F, bool)
    for f in range(F):
        touched[entries * F + f] = True
    gi, g2i = both_gradients(t, m, params, x, dev(t, dly_inf), u)
    gz, g2z = both_gradients(t, m, params, x, dev(t, dly_zero), u)
    for got, base in ((gi, gz), (g2i, g2z)):
        assert np.isfinite(base).all()
        assert np.array_equal(np.isnan(got), touched)
        assert same_bits(got[~touched], base[~touched])
    # the next call is clean: the poison does not outlive its call
    gn, _ = both_gradients(t, m, params, x, dev(t, dly_zero), u)
    assert same_bits(gn, gz)


def test_config(torch_cuda):
    from neus2_amd import NeusError
    from neus2_amd.module import Module, Precision
    t = torch_cuda
    m = create("A", "fp32", gradient_scatter="binned")
    assert m.hyperparams()["gradient_scatter"] == "binned" and m.gradient_scatter == "binned"
    plain = create("A", "fp32")
    assert "gradient_scatter" not in plain.hyperparams() and plain.gradient_scatter == "atomic"
    with pytest.raises(NeusError, match="gradient_scatter"):
        create("A", "fp32", gradient_scatter="sorted")
    # the 3-D 2-feature hashed linear grid keeps its own kernels: fp32 (float atomics) refuses, and names the way out
    cfg = {"otype": "HashGrid", "n_levels": 4, "n_features_per_level": 2, "log2_hashmap_size": 12, "base_resolution": 8, "per_level_scale": 1.5,
           "gradient_precision": "fp32"}
    n = 256
    with pytest.raises(NeusError, match="implementation"):
        Module.create_encoding(dict(cfg, gradient_scatter="binned"), batch_capacity=n, requested_precision=Precision.Fp32)
    general = Module.create_encoding(dict(cfg, gradient_scatter="binned", implementation="general"), batch_capacity=n, requested_precision=Precision.Fp32)
    assert general.hyperparams()["gradient_scatter"] == "binned" and general.name() == "Grid"
    # fp16: the binned int64 scatter of grid.hip as it is; the key is accepted, echoed and changes nothing
    a = Module.create_encoding(cfg, batch_capacity=n, requested_precision=Precision.Fp16)
    b = Module.create_encoding(dict(cfg, gradient_scatter="binned"), batch_capacity=n, requested_precision=Precision.Fp16)
    assert "gradient_scatter" not in a.hyperparams() and b.hyperparams()["gradient_scatter"] == "binned" and b.name() == "HashGrid"
    rng = np.random.default_rng(9)
    params = dev(t, rng.uniform(-1, 1, a.n_params).astype(np.float16)).view(t.float16)
    x, u = dev(t, rng.uniform(0.02, 0.98, (n, 3)).astype(np.float32)), dev(t, rng.normal(0, 1, (n, 3)).astype(np.float32))
    dly = dev(t, rng.normal(0, 1, (n, 8)).astype(np.float16)).view(t.float16)
    ga, g2a = both_gradients(t, a, params, x, dly, u)
    gb, g2b = both_gradients(t, b, params, x, dly, u)
    assert ga.any() and g2a.any() and same_bits(ga, gb) and same_bits(g2a, g2b)
