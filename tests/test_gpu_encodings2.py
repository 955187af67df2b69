"""The stand-alone TriangleWave, OneBlob and OneBlobFrequency / NRC encodings (create_encoding), alone and nested in a
Composite, against the float64 references of tests/enc_ref2.py, as tests/test_gpu_encodings.py tests the other
parameter-free encodings: every case in Fp16 and Fp32, AoS and SoA, at n = 1, 63, 65, 257 and 1000 (the wave and block
edges), inputs in [-0.25, 1.25] with exact 0, 0.5 and 1 among them (for TriangleWave these sit on kinks); for OneBlob
also 8 rows at x = -1.5, -1, -1 + 1/B, 2 - 1/B, 2, 2.5, 1e6, -1e6 (the edge of the reference kernels' range, and beyond it
the three-image sum that is the definition).

Bars (from the number formats, not from the device's results):
  forward Fp32   |err| <= 2^-20 max(1, |ref|): the arguments are reduced exactly (TriangleWave) or rounded once (OneBlob),
                 the rest is a handful of fp32 operations on values of order 1
  forward Fp16   |err| <= 2^-11 |ref| + 2^-20 + 2^-25: one more rounding of such a value
  dL_dinput      |err| <= (w + 2) 2^-24 sum_k |dL_dy_k J_kd| + 2^-20 sum_k |dL_dy_k| c_k: the fp32 sum over the w columns and
                 the derivative's own error, c_k = max(1, |J_kd|), and c_k = n_bins for a OneBlob column: its derivative is
                 n_bins times a difference of two O(1) terms, so its error scales with n_bins even where J_kd cancels to 0
  double backward (Fp32) rel-L2 <= 3e-5, the project's fp32 bar (test_gpu_bbi_full.py); TriangleWave has no second
                 derivative: its dL_dinput is exactly zero
"""
import functools

import numpy as np
import pytest

import enc_ref2 as E2

pytestmark = pytest.mark.gpu

NS = (1, 63, 65, 257, 1000)
COMPOSITE = {"otype": "Composite", "nested": [
    {"otype": "OneBlob", "n_dims_to_encode": 2, "n_bins": 4},
    {"otype": "Frequency", "n_dims_to_encode": 1, "n_frequencies": 3},
    {"otype": "TriangleWave", "n_frequencies": 2}]}
CASES = {
    "tri_d1_f1": (1, {"otype": "TriangleWave", "n_frequencies": 1}),
    "tri_d3_f6": (3, {"otype": "TriangleWave", "n_frequencies": 6}),
    "tri_d5_f16": (5, {"otype": "TriangleWave", "n_frequencies": 16}),
    "blob_d1_b1": (1, {"otype": "OneBlob", "n_bins": 1}),
    "blob_d2_b2": (2, {"otype": "OneBlob", "n_bins": 2}),
    "blob_d3_b8": (3, {"otype": "OneBlob", "n_bins": 8}),
    "blob_d2_b64": (2, {"otype": "OneBlob", "n_bins": 64}),
    "blob_d1_b128": (1, {"otype": "OneBlob", "n_bins": 128}),
    "nrc": (9, {"otype": "NRC", "n_frequencies": 4, "n_bins": 4}),
    "composite": (5, COMPOSITE),
}
WIDTHS = {"tri_d1_f1": 1, "tri_d3_f6": 18, "tri_d5_f16": 80, "blob_d1_b1": 1, "blob_d2_b2": 4, "blob_d3_b8": 24, "blob_d2_b64": 128,
          "blob_d1_b128": 128, "nrc": 12 + 20 + 1, "composite": 8 + 6 + 4}
EDGE = 8  # the pseudo batch size of OneBlob's out-of-range rows


def _inputs(case, n):
    D, cfg = CASES[case]
    if n == EDGE:
        B = cfg["n_bins"]
        col = np.array([-1.5, -1.0, -1.0 + 1.0 / B, 2.0 - 1.0 / B, 2.0, 2.5, 1e6, -1e6], np.float32)
        return np.stack([np.roll(col, d) for d in range(D)], axis=1)
    rng = np.random.default_rng(1000 * sorted(CASES).index(case) + n)
    x = rng.uniform(-0.25, 1.25, (n, D)).astype(np.float32)
    flat = x.reshape(-1)
    for i, v in enumerate((0.5, 0.0, 1.0)[:flat.size]):
        flat[i] = v
    return x


def _ns(case):
    return NS + ((EDGE,) if CASES[case][1]["otype"] == "OneBlob" else ())


@functools.lru_cache(maxsize=None)
def _reference(case, n):
    """(x float32, y float64 [n, w], J float64 [n, w, D], c float64 [n, w, D]): computed once, shared by the precisions and
    layouts, never modified"""
    D, cfg = CASES[case]
    x = _inputs(case, n)
    y, J = E2.jacobian(x, cfg)
    c = E2.derivative_scale(cfg, D, J)
    for a in (x, y, J, c):
        a.setflags(write=False)
    return x, y, J, c


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
@pytest.mark.parametrize("case", list(CASES))
def test_forward_and_input_gradient(torch_cuda, case, precision, layout):
    t = torch_cuda
    from neus2_amd.module import GradientMode
    m = _module(case, precision, layout)
    f32 = precision == "fp32"
    dt = np.float32 if f32 else np.float16
    D, cfg = CASES[case]
    assert m.n_params == 0 and m.n_input_dims == D and m.n_output_dims == WIDTHS[case] and m.info["n_levels"] == 0
    hp = m.hyperparams()
    assert hp["output_layout"] == layout and hp["precision"] == precision
    if case == "nrc":  # the Composite it stands for is echoed
        assert hp["otype"] == "Composite" and [(e["otype"], e["n_dims_to_encode"]) for e in hp["nested"]] == [
            ("TriangleWave", 3), ("OneBlob", 5), ("Identity", 1)]
        assert hp["nested"][0]["n_frequencies"] == 4 and hp["nested"][1]["n_bins"] == 4
    elif case == "composite":
        assert hp["otype"] == "Composite" and [e["otype"] for e in hp["nested"]] == ["OneBlob", "Frequency", "TriangleWave"]
    else:
        key = "n_bins" if cfg["otype"] == "OneBlob" else "n_frequencies"
        assert hp["otype"] == cfg["otype"] and hp[key] == cfg[key]
    empty = t.empty(0, dtype=t.float32 if f32 else t.float16, device="cuda")
    assert m.initialize_params(7).numel() == 0
    for n in _ns(case):
        x32, y_ref, J, c = _reference(case, n)
        w = y_ref.shape[1]
        assert m.n_output_dims == w and m.output_shape(n) == ((n, w) if layout == "AoS" else (w, n))
        x = t.from_numpy(x32.copy()).cuda()
        y_inf = m.inference(x, None)
        ctx, y = m.forward(x, empty, prepare_input_gradients=True)
        assert tuple(y.shape) == m.output_shape(n) and y.dtype == (t.float32 if f32 else t.float16)
        assert t.equal(y, y_inf)
        got = _from_layout(y, layout)
        err = np.abs(got - y_ref)
        bar = 2.0 ** -20 * np.maximum(1.0, np.abs(y_ref)) if f32 else 2.0 ** -11 * np.abs(y_ref) + 2.0 ** -20 + 2.0 ** -25
        print(f"{case} {precision} {layout} n={n}: forward max err/bar {float((err / bar).max()):.3f}")
        assert (err <= bar).all(), (n, float((err / bar).max()))
        if cfg["otype"] == "OneBlob" and cfg["n_bins"] >= 4:  # the bins no blob reaches are exact zeros
            assert int((got.reshape(n, D, -1) != 0).sum(axis=2).max()) <= 3
        # dL_dinput with dL_doutput ~ normal(0, 1) in the module's precision
        rng = np.random.default_rng(n)
        dy = rng.normal(0, 1, (n, w)).astype(dt)
        dy64 = dy.astype(np.float64)
        ref = np.einsum("nk,nkd->nd", dy64, J)
        bound = ((w + 2) * 2.0 ** -24 * np.einsum("nk,nkd->nd", np.abs(dy64), np.abs(J))
                 + 2.0 ** -20 * np.einsum("nk,nkd->nd", np.abs(dy64), c))
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
    for case in ("tri_d3_f6", "blob_d3_b8", "nrc"):
        with pytest.raises(NeusError, match="AoS or SoA"):
            _module(case, "fp16", "paired")


def test_nrc_on_eight_dims_has_no_identity_segment(torch_cuda):
    from neus2_amd.module import Module
    m = Module.create_encoding({"otype": "OneBlobFrequency"}, batch_capacity=128, n_input_dims=8)
    hp = m.hyperparams()
    assert m.n_output_dims == 3 * 12 + 5 * 4 and [e["otype"] for e in hp["nested"]] == ["TriangleWave", "OneBlob"]
    assert hp["nested"][0]["n_frequencies"] == 12 and hp["nested"][1]["n_bins"] == 4


@pytest.mark.parametrize("layout", ["AoS", "SoA"])
@pytest.mark.parametrize("case", ["tri_d3_f6", "blob_d1_b1", "blob_d3_b8", "blob_d2_b64", "nrc", "composite"])
def test_double_backward_fp32(torch_cuda, case, layout):
    """S = u . dL/dx: dL_ddLdoutput = dS/d(dL_doutput) = J u and dL_dinput = dS/dx against float64 autograd."""
    import torch
    t = torch_cuda
    n = 257
    D, cfg = CASES[case]
    m = _module(case, "fp32", layout)
    x32, _, J, _ = _reference(case, n)
    w = J.shape[1]
    rng = np.random.default_rng(3)
    dy = rng.normal(0, 1, (n, w)).astype(np.float32)
    u = rng.normal(0, 1, (n, D)).astype(np.float32)
    xt = torch.tensor(x32.astype(np.float64), requires_grad=True)
    gx, = torch.autograd.grad((E2.encode(xt, cfg) * torch.tensor(dy.astype(np.float64))).sum(), xt, create_graph=True)
    if gx.requires_grad:
        g2 = torch.autograd.grad((gx * torch.tensor(u.astype(np.float64))).sum(), xt)[0].numpy()
    else:  # TriangleWave alone: dL/dx does not depend on x
        g2 = np.zeros((n, D))
    ddo_ref = np.einsum("nkd,nd->nk", J, u.astype(np.float64))
    x, u_dev = t.from_numpy(x32.copy()).cuda(), t.from_numpy(u).cuda()
    dy_dev = t.from_numpy(_to_layout(dy, layout)).cuda()
    ctx, y = m.forward(x, None, prepare_input_gradients=True)
    ddo = t.full(m.output_shape(n), 7.0, dtype=t.float32, device="cuda")
    ddx = t.full((n, D), 7.0, dtype=t.float32, device="cuda")
    m.backward_backward_input(ctx, x, u_dev, dy_dev, None, dL_ddLdoutput=ddo, dL_dinput=ddx)
    got_x = ddx.cpu().numpy()
    rel_o = np.linalg.norm(_from_layout(ddo, layout) - ddo_ref) / np.linalg.norm(ddo_ref)
    # the dims without a second derivative are exact zeros on both sides: TriangleWave's, and the Identity dim of NRC
    flat = {"tri_d3_f6": [0, 1, 2], "nrc": [0, 1, 2, 8], "composite": [3, 4]}.get(case, [])
    assert not got_x[:, flat].any() and not g2[:, flat].any()
    if len(flat) == D:
        rel_x = 0.0
    else:
        rel_x = np.linalg.norm(got_x - g2) / np.linalg.norm(g2)
    print(f"{case} {layout}: dL_ddLdoutput rel {rel_o:.3e}, dL_dinput rel {rel_x:.3e}")
    assert rel_o <= 3e-5 and rel_x <= 3e-5, (rel_o, rel_x)
    ddx2 = t.full((n, D), -3.0, dtype=t.float32, device="cuda")
    ddo2 = t.full(m.output_shape(n), -3.0, dtype=t.float32, device="cuda")
    m.backward_backward_input(ctx, x, u_dev, dy_dev, None, dL_ddLdoutput=ddo2, dL_dinput=ddx2)
    assert t.equal(ddx2, ddx) and t.equal(ddo2, ddo)
