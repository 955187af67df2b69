"""create_encoding at batch sizes that are no multiple of anything: n = 1, 33 and 1000 on a module of capacity 1024, in
every output layout (AoS [n][2L], SoA [2L][n], paired [L][n][2]: with n odd the SoA / paired row stride is odd too).
No tolerance of its own: a sample's output and dL_dinput rows depend on that sample alone, so re-laid to [n][2L] they equal
the first n rows of the AoS module's 1024-batch bit for bit; the fp16 table's dL_dparams (the scatter: records summed as
integers, zero records add exact zeros) equals bit for bit that of the 1024-batch whose dL_doutput rows >= n are zero; the
fp32 table's dL_dparams is a float-atomic sum and is held to test_gpu_module.py's rtol 1e-5 / atol 2e-5 for it."""
import types

import numpy as np
import pytest

from test_gpu_module import _from_nf, _to_nf

pytestmark = pytest.mark.gpu

CAP, L = 1024, 8
ENC_CFG = {"otype": "HashGrid", "n_levels": L, "n_features_per_level": 2, "log2_hashmap_size": 14, "base_resolution": 16,
           "per_level_scale": 1.5, "gradient_precision": "fp32"}


def _module(precision, layout):
    from neus2_amd.module import Module, Precision
    return Module.create_encoding(dict(ENC_CFG, output_layout=layout), batch_capacity=CAP,
                                  requested_precision=Precision.Fp32 if precision == "fp32" else Precision.Fp16)


def _dev(t, a):
    return t.from_numpy(a.view(np.int16).copy() if a.dtype == np.float16 else a.copy()).cuda()


def _call(t, m, params, pos, dly_nf, layout):
    """forward and backward of the rows given: output and dL_dinput as [n][2L] / [n][3], dL_dparams (host)"""
    from neus2_amd.module import GradientMode
    n = pos.shape[0]
    x = _dev(t, pos)
    ctx, y = m.forward(x, params, prepare_input_gradients=True)
    assert tuple(y.shape) == m.output_shape(n)
    g = t.full((m.n_params,), 7.0, dtype=t.float32, device="cuda")
    dx = t.full((n, 3), 7.0, dtype=t.float32, device="cuda")
    m.backward(ctx, x, _dev(t, _from_nf(dly_nf, layout, n, L)), params, dL_dparams=g, dL_dinput=dx, mode=GradientMode.Overwrite)
    return _to_nf(y.cpu().numpy(), layout, n, L), dx.cpu().numpy(), g.cpu().numpy()


@pytest.fixture(scope="module")
def refs(torch_cuda):
    """per precision: parameters, positions, dL_doutput and the AoS module's 1024-batch results"""
    t, out = torch_cuda, {}
    for precision, dt in (("fp16", np.float16), ("fp32", np.float32)):
        m = _module(precision, "AoS")
        rng = np.random.default_rng(23)
        ph = rng.uniform(-1, 1, m.n_params).astype(dt)
        pos = rng.uniform(0.02, 0.98, (CAP, 3)).astype(np.float32)
        dly = rng.normal(0, 1, (CAP, 2 * L)).astype(dt)
        r = types.SimpleNamespace(t=t, m=m, params=_dev(t, ph), pos=pos, dly=dly, grads={})
        r.y, r.dx, _ = _call(t, m, r.params, pos, dly, "AoS")
        out[precision] = r
    return out


def _grad_of_prefix(r, n):
    """dL_dparams of the 1024-batch with the dL_doutput rows >= n zeroed"""
    if n not in r.grads:
        dly = r.dly.copy()
        dly[n:] = 0
        r.grads[n] = _call(r.t, r.m, r.params, r.pos, dly, "AoS")[2]
    return r.grads[n]


def _bits(a):
    return a.view(np.uint16 if a.dtype == np.float16 else np.uint32)


@pytest.mark.parametrize("n", [1, 33, 1000])
@pytest.mark.parametrize("layout", ["AoS", "SoA", "paired"])
def test_encoding_fp16_ragged(refs, layout, n):
    r = refs["fp16"]
    y, dx, g = _call(r.t, _module("fp16", layout), r.params, r.pos[:n], r.dly[:n], layout)
    np.testing.assert_array_equal(_bits(y), _bits(r.y[:n]))
    np.testing.assert_array_equal(_bits(dx), _bits(r.dx[:n]))
    want = _grad_of_prefix(r, n)
    assert want.any()
    np.testing.assert_array_equal(_bits(g), _bits(want))


@pytest.mark.parametrize("n", [33, 1000])
@pytest.mark.parametrize("layout", ["AoS", "SoA"])
def test_encoding_fp32_ragged(refs, layout, n):
    r = refs["fp32"]
    y, dx, g = _call(r.t, _module("fp32", layout), r.params, r.pos[:n], r.dly[:n], layout)
    np.testing.assert_array_equal(_bits(y), _bits(r.y[:n]))
    np.testing.assert_array_equal(_bits(dx), _bits(r.dx[:n]))
    want = _grad_of_prefix(r, n)
    assert want.any()
    # (float atomics, as GridEncoding<float>'s: the summation order varies from call to call; test_gpu_module.py's bar)
    np.testing.assert_allclose(g, want, rtol=1e-5, atol=2e-5)
