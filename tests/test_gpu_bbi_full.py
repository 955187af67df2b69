"""The complete backward_backward_input at the raw Module level: with S = dL_ddLdinput . dL/dx, the two outputs that were
missing, dL_dinput = dS/dx (every module kind) and dL_ddLdoutput = dS/d(dL_doutput) (the network modules), against float64
autograd (tests/bbi_ref.py), N = 256 on the 4-level grid with two dense and two hashed levels.

Bars are the project's for the sibling outputs of the same kernels: fp16 modules rel-L2 <= 2e-3 and cosine >= 0.99999
(test_gpu_grid_mlp.py), the fp32 encoding rel-L2 <= 3e-5 (test_gpu_module.py). Samples with a hidden pre-activation within
1e-4 of 0 (the device may take the other ReLU branch) are removed from both sides: dL_doutput = 0, and dL_ddLdinput = 0 as
well, because dL_ddLdoutput = J u does not depend on dL_doutput; their share must stay <= 0.05.

Measured on an MI355X (rel-L2 / 1 - cosine): see DESIGN.md section 6."""
import numpy as np
import pytest

import bbi_ref as R

pytestmark = pytest.mark.gpu

N = 256
ENC_CASES = [("fp16", "AoS", 0), ("fp16", "paired", 0), ("fp32", "AoS", 0), ("fp32", "SoA", 0), ("fp16", "AoS", 1), ("fp32", "AoS", 1)]


def _from_nf(a, layout):
    """[N, 2L] feature-major reference -> the module's layout"""
    if layout == "AoS":
        return np.ascontiguousarray(a)
    if layout == "SoA":
        return np.ascontiguousarray(a.T)
    return np.ascontiguousarray(a.reshape(N, R.L, 2).transpose(1, 0, 2))


@pytest.mark.parametrize("precision,layout,step", ENC_CASES)
def test_encoding_dL_dinput(torch_cuda, precision, layout, step):
    """HashGrid dL_dinput (threw before): the closed form of kernel_grid_backward_input_backward_input, fp16 and fp32
    tables, every dL_doutput layout, and set_training_step(1) (levels 0..2 of 4 active: the top level contributes 0)."""
    import torch
    from neus2_amd.module import GradientMode, Module, Precision
    t = torch_cuda
    f32 = precision == "fp32"
    m = Module.create_encoding(dict(R.ENC_CFG, output_layout=layout, gradient_precision="fp32"), batch_capacity=N,
                               requested_precision=Precision.Fp32 if f32 else Precision.Fp16)
    rng = np.random.default_rng(11)
    dt = np.float32 if f32 else np.float16
    ph = rng.uniform(-1, 1, m.n_params).astype(dt)
    pos = rng.uniform(0.02, 0.98, (N, 3)).astype(np.float32)
    dly_nf = rng.normal(0, 1, (N, 2 * R.L)).astype(dt)
    v = rng.normal(0, 1, (N, 3)).astype(np.float32)
    valid = None
    if step:
        m.set_training_step(step)
        valid = 2
    dev = lambda a: t.from_numpy(a.view(np.int16).copy() if a.dtype == np.float16 else a.copy()).cuda()
    params, x, dly, u = dev(ph), dev(pos), dev(_from_nf(dly_nf, layout)), dev(v)
    ctx, y = m.forward(x, params, prepare_input_gradients=True)
    if step:
        yy = y.float().cpu().numpy()
        top = yy[:, 6:] if layout == "AoS" else yy[3]
        assert not top.any()
    tab = torch.tensor(ph.astype(np.float64).reshape(-1, 2), requires_grad=True)
    xt = torch.tensor(pos.astype(np.float64), requires_grad=True)
    S = (R.hash_grid(xt, tab, R.OFF, R.RES, valid) * torch.tensor(dly_nf.astype(np.float64))).sum()
    gx, = torch.autograd.grad(S, xt, create_graph=True)
    g2x, = torch.autograd.grad((gx * torch.tensor(v.astype(np.float64))).sum(), xt)
    ddx = t.full((N, 3), 7.0, dtype=t.float32, device="cuda")  # overwritten, not accumulated
    g2 = t.zeros(m.n_params, dtype=t.float32, device="cuda")
    m.backward_backward_input(ctx, x, u, dly, params, dL_dparams=g2, mode=GradientMode.Overwrite, dL_dinput=ddx)
    rel, cos = R.rel_cos(ddx.cpu().numpy(), g2x.numpy())
    R.record(f"bbi_full_encoding_{precision}_{layout}_step{step}", rel_dL_dinput=rel, one_minus_cos_dL_dinput=1 - cos)
    print(f"encoding {precision} {layout} step {step}: dL_dinput rel {rel:.3e} 1-cos {1 - cos:.3e}")
    if f32:
        assert rel <= 3e-5 and cos >= 0.9999999, (rel, cos)
    else:
        assert rel <= 2e-3 and cos >= 0.99999, (rel, cos)
    # a sample's levels are summed in a fixed order: bitwise the same on a second call, here without parameter gradients
    ddx2 = t.full((N, 3), -3.0, dtype=t.float32, device="cuda")
    m.backward_backward_input(ctx, x, u, dly, params, mode=GradientMode.Ignore, dL_dinput=ddx2)
    np.testing.assert_array_equal(ddx2.cpu().numpy(), ddx.cpu().numpy())
    if not f32:  # (the fp32 table's parameter gradient is a float-atomic sum: not repeatable by design)
        g2b = t.zeros(m.n_params, dtype=t.float32, device="cuda")
        m.backward_backward_input(ctx, x, u, dly, params, dL_dparams=g2b, mode=GradientMode.Overwrite)
        np.testing.assert_array_equal(g2b.cpu().numpy(), g2.cpu().numpy())


@pytest.mark.parametrize("name", list(R.NETS))
def test_network_new_outputs(torch_cuda, name):
    """dL_ddLdoutput (a poisoned buffer was left untouched before) and dL_dinput of the network modules: the fused k_dnet
    path (W 64, 1 hidden layer), the GridMlp path (W 16, 2 hidden layers, 3 outputs) and create_network (dL_dinput = 0)."""
    import torch
    from neus2_amd.module import GradientMode, Module
    t = torch_cuda
    enc, W, NH, n_out = R.NETS[name]
    cfg = dict(R.net_cfg(name), gradient_precision="fp32")
    m = (Module.create_network_with_input_encoding(3, n_out, R.ENC_CFG, cfg, batch_capacity=N) if enc
         else Module.create_network(3, n_out, cfg, batch_capacity=N))
    rng = np.random.default_rng(5)
    ph = R.net_params(name, rng, 0.3 if name == "dnet" else None)
    assert ph.size == m.n_params and m.n_output_dims == 16
    pos = rng.uniform(0.02, 0.98, (N, 3)).astype(np.float32)
    ref = R.network(name, ph, pos)
    amb = ref["ambiguous"]
    print(f"{name}: ambiguous share {amb.mean():.4f}")
    assert amb.mean() <= 0.05
    dlo = rng.normal(0, 1, (N, 16)).astype(np.float16)
    v = rng.normal(0, 1, (N, 3)).astype(np.float32)
    dlo[amb] = 0
    v[amb] = 0
    dlo_t = torch.tensor(dlo.astype(np.float64), requires_grad=True)
    gx, = torch.autograd.grad((ref["out"] * dlo_t).sum(), ref["xt"], create_graph=True)
    g2 = torch.autograd.grad((gx * torch.tensor(v.astype(np.float64))).sum(), [dlo_t, ref["xt"]], allow_unused=True)
    params = t.from_numpy(ph.view(np.int16).copy()).cuda()
    x, u = t.from_numpy(pos).cuda(), t.from_numpy(v).cuda()
    dlo_dev = t.from_numpy(dlo.view(np.int16).copy()).cuda()
    ctx, y = m.forward(x, params, prepare_input_gradients=True)
    gp0 = t.zeros(m.n_params, dtype=t.float32, device="cuda")
    m.backward_backward_input(ctx, x, u, dlo_dev, params, dL_dparams=gp0, mode=GradientMode.Overwrite)
    poison = np.float16(7.0)
    ddo = t.full((N, 16), float(poison), dtype=t.float16, device="cuda")
    ddx = t.full((N, 3), 7.0, dtype=t.float32, device="cuda")
    gp1 = t.zeros(m.n_params, dtype=t.float32, device="cuda")
    m.backward_backward_input(ctx, x, u, dlo_dev, params, dL_dparams=gp1, dL_ddLdoutput=ddo, mode=GradientMode.Overwrite, dL_dinput=ddx)
    # the parameter gradients do not change with the new pointers
    np.testing.assert_array_equal(gp1.cpu().numpy(), gp0.cpu().numpy())
    ddo_np, ddx_np = ddo.float().cpu().numpy(), ddx.cpu().numpy()
    assert not (ddo_np == float(poison)).all(axis=1).any()
    rel_o, cos_o = R.rel_cos(ddo_np, g2[0].numpy())
    metrics = dict(rel_dL_ddLdoutput=rel_o, one_minus_cos_dL_ddLdoutput=1 - cos_o, ambiguous=amb.mean())
    if enc:
        rel_x, cos_x = R.rel_cos(ddx_np, g2[1].numpy())
        metrics.update(rel_dL_dinput=rel_x, one_minus_cos_dL_dinput=1 - cos_x)
    R.record(f"bbi_full_network_{name}", **metrics)
    print(name, {k: f"{val:.3e}" for k, val in metrics.items()})
    assert rel_o <= 2e-3 and cos_o >= 0.99999, (rel_o, cos_o)
    if enc:
        assert rel_x <= 2e-3 and cos_x >= 0.99999, (rel_x, cos_x)
    else:  # piecewise-linear in x: the second derivative is identically zero
        assert g2[1] is None or not g2[1].numpy().any()
        assert not ddx_np.any()
    # the new outputs alone (Ignore): the same values, dL_dinput bitwise
    ddo2 = t.full((N, 16), float(poison), dtype=t.float16, device="cuda")
    ddx2 = t.full((N, 3), -3.0, dtype=t.float32, device="cuda")
    m.backward_backward_input(ctx, x, u, dlo_dev, params, dL_ddLdoutput=ddo2, mode=GradientMode.Ignore, dL_dinput=ddx2)
    np.testing.assert_array_equal(ddx2.cpu().numpy(), ddx_np)
    np.testing.assert_array_equal(ddo2.cpu().numpy().view(np.uint16), ddo.cpu().numpy().view(np.uint16))


def test_non_relu_network_is_refused(torch_cuda):
    """The fronts / backs chain has no act'' term: a Sigmoid network with a non-null dL_dinput or dL_ddLdoutput is an error
    that says so; its parameter gradients (both pointers null) stay available."""
    from neus2_amd import NeusError
    from neus2_amd.module import GradientMode, Module
    t = torch_cuda
    m = Module.create_network_with_input_encoding(3, 3, R.ENC_CFG, dict(R.net_cfg("gridmlp", "Sigmoid"), gradient_precision="fp32"),
                                                  batch_capacity=N)
    rng = np.random.default_rng(2)
    params = t.from_numpy(R.net_params("gridmlp", rng).view(np.int16).copy()).cuda()
    x = t.from_numpy(rng.uniform(0.02, 0.98, (N, 3)).astype(np.float32)).cuda()
    u = t.from_numpy(rng.normal(0, 1, (N, 3)).astype(np.float32)).cuda()
    dlo = t.from_numpy(rng.normal(0, 1, (N, 16)).astype(np.float16).view(np.int16).copy()).cuda()
    ctx, _ = m.forward(x, params, prepare_input_gradients=True)
    g = t.zeros(m.n_params, dtype=t.float32, device="cuda")
    m.backward_backward_input(ctx, x, u, dlo, params, dL_dparams=g, mode=GradientMode.Overwrite)
    assert g.abs().sum().item() > 0
    ddx = t.zeros((N, 3), dtype=t.float32, device="cuda")
    with pytest.raises(NeusError, match="ReLU or None"):
        m.backward_backward_input(ctx, x, u, dlo, params, dL_dparams=g, mode=GradientMode.Overwrite, dL_dinput=ddx)
    ddo = t.zeros((N, 16), dtype=t.float16, device="cuda")
    with pytest.raises(NeusError, match="ReLU or None"):
        m.backward_backward_input(ctx, x, u, dlo, params, dL_ddLdoutput=ddo, mode=GradientMode.Ignore)
