"""The stand-alone parameter-free encodings (create_encoding with Identity / Frequency / SphericalHarmonics / Composite)
against the float64 references of tests/enc_ref.py: every case in Fp16 and Fp32, AoS and SoA, at n = 1, 63, 65, 257 and
1000 (the wave and block edges), inputs in [-0.25, 1.25] with exact 0, 0.5 and 1 among them.

Bars (from the number formats, not from the device's results):
  forward Fp32   |err| <= 2^-20 max(1, |ref|): the argument of the trigonometry is reduced exactly, a 1-2 ulp sincos is
                 ~1.2e-7; the spherical harmonics are evaluated in fp64 and rounded once
  forward Fp16   |err| <= 2^-11 |ref| + 2^-20 + 2^-25: one more rounding of such a value
  dL_dinput      |err| <= (w + 2) 2^-24 sum_k |dL_dy_k J_kd| + 2^-20 sum_k |dL_dy_k| max(1, |J_kd|): the fp32 sum over the w
                 columns and the derivative's own error
  double backward (Fp32) rel-L2 <= 3e-5, the project's fp32 bar (test_gpu_bbi_full.py)
"""
import functools

import numpy as np
import pytest

import enc_ref as E

pytestmark = pytest.mark.gpu

NS = (1, 63, 65, 257, 1000)
COMPOSITE = {"otype": "Composite", "nested": [
    {"otype": "Identity", "n_dims_to_encode": 3, "scale": 2.0, "offset": -1.0},
    {"otype": "Frequency", "n_dims_to_encode": 3, "n_frequencies": 4},
    {"otype": "SphericalHarmonics", "degree": 4}]}
COMPOSITE_NO_SH = {"otype": "Composite", "nested": [
    {"otype": "Identity", "n_dims_to_encode": 3, "scale": 2.0, "offset": -1.0},
    {"otype": "Frequency", "n_frequencies": 4}]}
CASES = {
    "freq_d1_f1": (1, {"otype": "Frequency", "n_frequencies": 1}),
    "freq_d3_f6": (3, {"otype": "Frequency", "n_frequencies": 6}),
    "freq_d5_f16": (5, {"otype": "Frequency", "n_frequencies": 16}),
    "sh1": (3, {"otype": "SphericalHarmonics", "degree": 1}),
    "sh4": (3, {"otype": "SphericalHarmonics", "degree": 4}),
    "sh5": (3, {"otype": "SphericalHarmonics", "degree": 5}),
    "sh8": (3, {"otype": "SphericalHarmonics", "degree": 8}),
    "composite": (9, COMPOSITE),
    "composite_no_sh": (6, COMPOSITE_NO_SH),
}
FIRST_ORDER = [c for c in CASES if c != "composite_no_sh"]


def _inputs(case, n):
    D = CASES[case][0]
    rng = np.random.default_rng(1000 * sorted(CASES).index(case) + n)
    x = rng.uniform(-0.25, 1.25, (n, D)).astype(np.float32)
    flat = x.reshape(-1)
    for i, v in enumerate((0.5, 0.0, 1.0)[:flat.size]):
        flat[i] = v
    return x


@functools.lru_cache(maxsize=None)
def _reference(case, n):
    """(x float32, y float64 [n, w], J float64 [n, w, D]): computed once, shared by the precisions and layouts, never
    modified"""
    x = _inputs(case, n)
    y, J = E.jacobian(x, CASES[case][1])
    for a in (x, y, J):
        a.setflags(write=False)
    return x, y, J


def _module(case, precision, layout, cap=1024):
    from neus2_amd.module import Module, Precision
    D, cfg = CASES[case]
    return Module.create_encoding(dict(cfg, output_layout=layout), batch_capacity=cap, n_input_dims=D,
                                  requested_precision=Precision.Fp32 if precision == "fp32" else Precision.Fp16)


def _to_layout(a, layout):
    return np.ascontiguousarray(a if layout == "AoS" else a.T)


def _from_layout(t, layout):
    a = t.float().cpu().numpy().astype(np.float64)
    return a if layout == "AoS" else a.T


@pytest.mark.parametrize("layout", ["AoS", "SoA"])
@pytest.mark.parametrize("precision", ["fp16", "fp32"])
@pytest.mark.parametrize("case", FIRST_ORDER)
def test_forward_and_input_gradient(torch_cuda, case, precision, layout):
    t = torch_cuda
    from neus2_amd.module import GradientMode
    m = _module(case, precision, layout)
    f32 = precision == "fp32"
    dt = np.float32 if f32 else np.float16
    D = CASES[case][0]
    assert m.n_params == 0 and m.n_input_dims == D and m.info["n_levels"] == 0
    hp = m.hyperparams()
    assert hp["otype"] == CASES[case][1]["otype"] and hp["output_layout"] == layout and hp["precision"] == precision
    if case == "composite":
        assert [e["otype"] for e in hp["nested"]] == ["Identity", "Frequency", "SphericalHarmonics"]
    empty = t.empty(0, dtype=t.float32 if f32 else t.float16, device="cuda")
    assert m.initialize_params(7).numel() == 0
    worst = {}
    for n in NS:
        x32, y_ref, J = _reference(case, n)
        w = y_ref.shape[1]
        assert m.n_output_dims == w and m.output_shape(n) == ((n, w) if layout == "AoS" else (w, n))
        x = t.from_numpy(x32.copy()).cuda()
        # null params (None) and an empty tensor are both accepted; inference and forward agree bitwise
        y_inf = m.inference(x, None)
        ctx, y = m.forward(x, empty, prepare_input_gradients=True)
        assert tuple(y.shape) == m.output_shape(n) and y.dtype == (t.float32 if f32 else t.float16)
        assert t.equal(y, y_inf)
        got = _from_layout(y, layout)
        err = np.abs(got - y_ref)
        bar = 2.0 ** -20 * np.maximum(1.0, np.abs(y_ref)) if f32 else 2.0 ** -11 * np.abs(y_ref) + 2.0 ** -20 + 2.0 ** -25
        worst[n] = (float((err / bar).max()),)
        print(f"{case} {precision} {layout} n={n}: forward max err/bar {worst[n][0]:.3f}")
        assert (err <= bar).all(), (n, float((err / bar).max()))
        # dL_dinput with dL_doutput ~ normal(0, 1) in the module's precision
        rng = np.random.default_rng(n)
        dy = rng.normal(0, 1, (n, w)).astype(dt)
        dy64 = dy.astype(np.float64)
        ref = np.einsum("nk,nkd->nd", dy64, J)
        absJ = np.abs(J)
        bound = ((w + 2) * 2.0 ** -24 * np.einsum("nk,nkd->nd", np.abs(dy64), absJ)
                 + 2.0 ** -20 * np.einsum("nk,nkd->nd", np.abs(dy64), np.maximum(1.0, absJ)))
        dy_dev = t.from_numpy(_to_layout(dy, layout)).cuda()
        dx = t.full((n, D), 7.0, dtype=t.float32, device="cuda")  # overwritten, not accumulated
        m.backward(ctx, x, dy_dev, None, dL_dparams=None, dL_dinput=dx, mode=GradientMode.Overwrite)
        gerr = np.abs(dx.cpu().numpy().astype(np.float64) - ref)
        print(f"{case} {precision} {layout} n={n}: dL_dinput max err/bound {float((gerr / bound).max()):.3f}")
        assert (gerr <= bound).all(), (n, float((gerr / bound).max()))
        dx2 = t.full((n, D), -3.0, dtype=t.float32, device="cuda")
        m.backward(ctx, x, dy_dev, empty, dL_dparams=empty, dL_dinput=dx2, mode=GradientMode.Overwrite)
        assert t.equal(dx2, dx)  # fixed summation order: bitwise repeatable
        y2 = m.inference(x, empty)
        assert t.equal(y2, y)


def test_paired_layout_is_refused(torch_cuda):
    from neus2_amd import NeusError
    with pytest.raises(NeusError, match="AoS or SoA"):
        _module("sh4", "fp16", "paired")


@pytest.mark.parametrize("layout", ["AoS", "SoA"])
@pytest.mark.parametrize("case", ["freq_d3_f6", "composite_no_sh"])
def test_double_backward_fp32(torch_cuda, case, layout):
    """S = u . dL/dx: dL_ddLdoutput = dS/d(dL_doutput) = J u and dL_dinput = dS/dx against float64 autograd."""
    import torch
    t = torch_cuda
    n = 257
    D, cfg = CASES[case]
    m = _module(case, "fp32", layout)
    x32, _, J = _reference(case, n)
    w = J.shape[1]
    rng = np.random.default_rng(3)
    dy = rng.normal(0, 1, (n, w)).astype(np.float32)
    u = rng.normal(0, 1, (n, D)).astype(np.float32)
    xt = torch.tensor(x32.astype(np.float64), requires_grad=True)
    gx, = torch.autograd.grad((E.encode(xt, cfg) * torch.tensor(dy.astype(np.float64))).sum(), xt, create_graph=True)
    g2, = torch.autograd.grad((gx * torch.tensor(u.astype(np.float64))).sum(), xt)
    ddo_ref = np.einsum("nkd,nd->nk", J, u.astype(np.float64))
    x, u_dev = t.from_numpy(x32.copy()).cuda(), t.from_numpy(u).cuda()
    dy_dev = t.from_numpy(_to_layout(dy, layout)).cuda()
    ctx, y = m.forward(x, None, prepare_input_gradients=True)
    ddo = t.full(m.output_shape(n), 7.0, dtype=t.float32, device="cuda")
    ddx = t.full((n, D), 7.0, dtype=t.float32, device="cuda")
    m.backward_backward_input(ctx, x, u_dev, dy_dev, None, dL_ddLdoutput=ddo, dL_dinput=ddx)
    rel_o = np.linalg.norm(_from_layout(ddo, layout) - ddo_ref) / np.linalg.norm(ddo_ref)
    rel_x = np.linalg.norm(ddx.cpu().numpy() - g2.numpy()) / np.linalg.norm(g2.numpy())
    print(f"{case} {layout}: dL_ddLdoutput rel {rel_o:.3e}, dL_dinput rel {rel_x:.3e}")
    assert rel_o <= 3e-5 and rel_x <= 3e-5, (rel_o, rel_x)
    if case == "composite_no_sh":  # the Identity dims have no second derivative
        assert not ddx.cpu().numpy()[:, :3].any() and not g2.numpy()[:, :3].any()
    ddx2 = t.full((n, D), -3.0, dtype=t.float32, device="cuda")
    m.backward_backward_input(ctx, x, u_dev, dy_dev, None, dL_dinput=ddx2)
    assert t.equal(ddx2, ddx)


@pytest.mark.parametrize("case", ["sh4", "composite"])
def test_double_backward_with_sh(torch_cuda, case):
    """With a SphericalHarmonics segment dL_ddLdoutput = J u (first derivatives only) is provided; dL_dinput is refused."""
    t = torch_cuda
    from neus2_amd import NeusError
    n = 257
    D, cfg = CASES[case]
    m = _module(case, "fp32", "AoS")
    x32, _, J = _reference(case, n)
    rng = np.random.default_rng(4)
    dy = rng.normal(0, 1, (n, J.shape[1])).astype(np.float32)
    u = rng.normal(0, 1, (n, D)).astype(np.float32)
    ddo_ref = np.einsum("nkd,nd->nk", J, u.astype(np.float64))
    x, u_dev, dy_dev = t.from_numpy(x32.copy()).cuda(), t.from_numpy(u).cuda(), t.from_numpy(dy).cuda()
    ctx, y = m.forward(x, None, prepare_input_gradients=True)
    ddo = t.full(m.output_shape(n), 7.0, dtype=t.float32, device="cuda")
    m.backward_backward_input(ctx, x, u_dev, dy_dev, None, dL_ddLdoutput=ddo)
    rel_o = np.linalg.norm(_from_layout(ddo, "AoS") - ddo_ref) / np.linalg.norm(ddo_ref)
    print(f"{case}: dL_ddLdoutput rel {rel_o:.3e}")
    assert rel_o <= 3e-5, rel_o
    ddx = t.zeros((n, D), dtype=t.float32, device="cuda")
    with pytest.raises(NeusError, match="not supported.*SphericalHarmonics"):
        m.backward_backward_input(ctx, x, u_dev, dy_dev, None, dL_ddLdoutput=ddo, dL_dinput=ddx)
