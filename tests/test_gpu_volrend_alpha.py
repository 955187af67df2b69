"""volrend.neus_alpha (volrend.hip k_vr_alpha_fwd / k_vr_alpha_bwd) against the float64 restatement on the same fp32
inputs.

Forward: |err| <= 32 * 2^-24 / (c + 1e-5) per element, c from the reference: each logistic is good to a few units of
2^-24 absolute, p is a difference of two of them, and the quotient divides by c + 1e-5; 32 is that bound with slack.
Gradients: rel-L2 <= 4 x the rel-L2 of the fp32 stock-PyTorch formulation evaluated on the CPU against the same
float64 truth, plus 2^-22. Each test prints its worst ratio (DESIGN.md §3.13 records them)."""
import numpy as np
import pytest
import torch

import volrend_ref as VR

pytestmark = pytest.mark.gpu
U = 2.0 ** -24


def rel_l2(x, ref):
    x, ref = np.asarray(x, np.float64).ravel(), np.asarray(ref, np.float64).ravel()
    return float(np.linalg.norm(x - ref) / np.linalg.norm(ref))


def gpu_alpha(sdf, cos, dt, inv_s, ratio, g=None, dt_float=False, s_float=False):
    """alpha (and with g the three gradients) from the operator, as numpy."""
    from neus2_amd import volrend
    x, c = (torch.from_numpy(v).cuda().requires_grad_(g is not None) for v in (sdf, cos))
    s = float(inv_s) if s_float else torch.tensor(float(inv_s), device="cuda", requires_grad=g is not None)
    d = float(dt[0]) if dt_float else torch.from_numpy(dt).cuda()
    alpha = volrend.neus_alpha(x, c, d, s, ratio)
    if g is None:
        return alpha.detach().cpu().numpy()
    alpha.backward(torch.from_numpy(g).cuda())
    return alpha.detach().cpu().numpy(), x.grad.cpu().numpy(), c.grad.cpu().numpy(), s.grad.cpu().numpy()


def cpu_grads(dtype, sdf, cos, dt, inv_s, ratio, g):
    x, c, s = (torch.tensor(v, dtype=dtype, requires_grad=True) for v in (sdf, cos, float(inv_s)))
    VR.neus_alpha(x, c, torch.tensor(dt, dtype=dtype), s, ratio).backward(torch.tensor(g, dtype=dtype))
    return x.grad.numpy(), c.grad.numpy(), s.grad.numpy()


@pytest.mark.parametrize("dt_float", [False, True])
@pytest.mark.parametrize("inv_s,ratio", VR.ALPHA_CASES)
@pytest.mark.parametrize("S", VR.ALPHA_SIZES)
def test_forward_within_the_logistic_bound(torch_cuda, S, inv_s, ratio, dt_float):
    sdf, cos, dt, _ = VR.alpha_case(S)
    f64 = lambda v: torch.from_numpy(v.astype(np.float64))
    q, c = VR.alpha_terms(f64(sdf), f64(cos), f64(dt), float(inv_s), ratio)
    got = gpu_alpha(sdf, cos, dt, inv_s, ratio, dt_float=dt_float)
    err = np.abs(got.astype(np.float64) - q.clamp(0, 1).numpy())
    bound = 32 * U / (c.numpy() + 1e-5)
    print(f"alpha forward S={S} inv_s={inv_s} dt_float={dt_float}: worst err / bound = {(err / bound).max():.4f}")
    assert (err <= bound).all()


@pytest.mark.parametrize("dt_float", [False, True])
@pytest.mark.parametrize("inv_s,ratio", VR.ALPHA_CASES)
@pytest.mark.parametrize("S", VR.ALPHA_SIZES[1:])
def test_gradients_within_four_times_the_stock_fp32_floor(torch_cuda, S, inv_s, ratio, dt_float):
    sdf, cos, dt, g = VR.alpha_case(S)
    truth = cpu_grads(torch.float64, sdf, cos, dt, inv_s, ratio, g)
    stock = cpu_grads(torch.float32, sdf, cos, dt, inv_s, ratio, g)
    got = gpu_alpha(sdf, cos, dt, inv_s, ratio, g, dt_float=dt_float)[1:]
    for name, x, f, ref in zip(("sdf", "true_cos", "inv_s"), got, stock, truth):
        e, floor = rel_l2(x, ref), rel_l2(f, ref)
        print(f"alpha grad {name} S={S} inv_s={inv_s} dt_float={dt_float}: rel-L2 {e:.3e}, floor {floor:.3e}, ratio {e / max(floor, 1e-300):.4f}")
        assert np.isfinite(x).all() and e <= 4 * floor + 2.0 ** -22, name


def test_inv_s_gradient_repeats_and_ignores_zero_gradient_padding(torch_cuda):
    sdf, cos, dt, g = VR.alpha_case(3001)
    a = gpu_alpha(sdf, cos, dt, 64.0, 0.0, g)
    b = gpu_alpha(sdf, cos, dt, 64.0, 0.0, g)
    assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))
    for pad in (1, 255, 5000):
        z = np.zeros(pad, np.float32)
        p = gpu_alpha(np.concatenate([sdf, z]), np.concatenate([cos, z + 0.5]), np.concatenate([dt, z + VR.DT]), 64.0, 0.0, np.concatenate([g, z]))
        assert p[3].view(np.uint32) == a[3].view(np.uint32), pad
        assert np.array_equal(p[1][:3001].view(np.uint32), a[1].view(np.uint32)) and (p[1][3001:] == 0).all()


def test_a_python_float_inv_s_gives_the_tensor_bits(torch_cuda):
    sdf, cos, dt, _ = VR.alpha_case(3001)
    for inv_s, ratio in VR.ALPHA_CASES:
        a = gpu_alpha(sdf, cos, dt, inv_s, ratio)
        b = gpu_alpha(sdf, cos, dt, inv_s, ratio, s_float=True)
        c = gpu_alpha(sdf, cos, dt, inv_s, ratio, s_float=True, dt_float=True)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.array_equal(a.view(np.uint32), c.view(np.uint32))


def test_clamp_and_relu_cut_the_gradient_and_second_order_raises(torch_cuda):
    from neus2_amd import volrend
    # cos = 1: a1 = a2 = 0, so p = 0 and alpha = 1e-5 / (c + 1e-5) with no gradient to cos; cos = -1, a huge inv_s: clamp at 1
    x = torch.tensor([0.01, -0.2], device="cuda", requires_grad=True)
    c = torch.tensor([1.0, -1.0], device="cuda", requires_grad=True)
    s = torch.tensor([4000.0], device="cuda", requires_grad=True)
    alpha = volrend.neus_alpha(x, c, 0.5, s, 1.0)
    assert s.grad is None and float(alpha.detach()[1]) == 1.0
    g, = torch.autograd.grad(alpha.sum(), c, create_graph=True)
    assert float(g[0]) == 0.0 and float(g[1]) == 0.0
    with pytest.raises(RuntimeError, match="once_differentiable|does not require grad"):
        g.sum().backward()
    alpha = volrend.neus_alpha(x, c, 0.5, s, 1.0)
    alpha.sum().backward()
    assert s.grad.shape == (1,) and float(x.grad[1]) == 0.0 and torch.isfinite(s.grad).all()
