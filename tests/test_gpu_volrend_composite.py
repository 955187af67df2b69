"""volrend.composite (volrend.hip k_vr_comp_*) against the float64 loops of tests/volrend_ref.py.

Per element: |err| <= 4 (n_r + 4) 2^-24 A + 1e-30, n_r the ray's sample count and A the same expression evaluated in
float64 with every term replaced by its absolute value: the standard error bound of a product of n factors summed over n
terms, the 4 covering serial or tree order. Rays where some T_i lies within a relative 1e-3 of t_stop are dropped from
both sides (the cut index may differ by rounding); tests/test_volrend_ref.py bounds their share."""
import numpy as np
import pytest
import torch

import volrend_ref as VR

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
_ref_cache = {}


def reference(R, C, t_stop):
    """(inputs, float64 loops, kept rays, per-sample ray, per-sample kept): computed once per case and left unchanged."""
    key = (R, C, t_stop)
    if key not in _ref_cache:
        alpha, values, ranges, g = VR.composite_case(R, C)
        L = VR.composite_loops(alpha, values, ranges, t_stop, *g)
        f64 = lambda x: torch.from_numpy(x.astype(np.float64))
        T = VR.composite(f64(alpha), f64(values), ranges, t_stop)[4]
        keep = ~VR.ambiguous_rays(T, ranges, t_stop)
        ray = np.repeat(np.arange(R), ranges[:, 1])
        _ref_cache[key] = ((alpha, values, ranges, g), L, keep, ray, keep[ray])
    return _ref_cache[key]


def gpu_composite(alpha, values, ranges, t_stop, g_out=None, g_op=None, g_w=None):
    from neus2_amd import volrend
    a, v = (torch.from_numpy(x).cuda().requires_grad_() for x in (alpha, values))
    out, op, w, n = volrend.composite(a, v, torch.from_numpy(ranges).cuda(), t_stop)
    assert n.dtype == torch.int32 and not n.requires_grad
    loss = sum((y * torch.from_numpy(g).cuda()).sum() for y, g in ((out, g_out), (op, g_op), (w, g_w)) if g is not None)
    loss.backward()
    return {k: x.detach().cpu().numpy() for k, x in (("out", out), ("opacity", op), ("weights", w), ("n", n), ("g_alpha", a.grad), ("g_values", v.grad))}


def check(got, L, ranges, keep, ray, skeep, keys):
    n_r = ranges[:, 1].astype(np.float64)
    for key in keys:
        per_ray = key in ("out", "opacity")
        k = keep if per_ray else skeep
        nn = n_r if per_ray else n_r[ray]
        nn = nn[:, None] if L[key].ndim == 2 else nn
        bound = 4 * (nn + 4) * U * L["A_" + key] + 1e-30
        err = np.abs(got[key].astype(np.float64) - L[key])
        worst = float((err / bound)[k].max()) if k.any() and err.size else 0.0
        print(f"composite {key}: worst err / bound = {worst:.4f}")
        assert np.isfinite(got[key]).all() and (err <= bound)[k].all(), key


@pytest.mark.parametrize("t_stop", VR.T_STOPS)
@pytest.mark.parametrize("C", VR.CHANNELS)
@pytest.mark.parametrize("R", VR.RAYS)
def test_forward_and_both_gradients_within_the_product_sum_bound(torch_cuda, R, C, t_stop):
    (alpha, values, ranges, g), L, keep, ray, skeep = reference(R, C, t_stop)
    got = gpu_composite(alpha, values, ranges, t_stop, *g)
    assert np.array_equal(got["n"][keep], L["n"][keep])
    check(got, L, ranges, keep, ray, skeep, ("out", "opacity", "weights", "g_alpha", "g_values"))
    # from the stop on: exactly zero weight and gradient
    past = (np.arange(len(alpha)) - ranges[ray, 0] >= got["n"][ray])
    assert (got["weights"][past] == 0).all() and (got["g_alpha"][past] == 0).all() and (got["g_values"][past] == 0).all()
    if t_stop > 0 and R > 1:
        assert past.any() and (got["n"] < ranges[:, 1]).any()


@pytest.mark.parametrize("which", ["out", "opacity", "weights"])
def test_each_cotangent_alone(torch_cuda, which):
    (alpha, values, ranges, g), _, keep, ray, skeep = reference(200, 7, 1e-4)
    gs = [x if name == which else None for name, x in zip(("out", "opacity", "weights"), g)]
    L = VR.composite_loops(alpha, values, ranges, 1e-4, *[np.zeros_like(x) if y is None else x for x, y in zip(g, gs)])
    got = gpu_composite(alpha, values, ranges, 1e-4, *gs)
    check(got, L, ranges, keep, ray, skeep, ("g_alpha", "g_values"))
    assert np.abs(got["g_alpha"]).max() > 0


@pytest.mark.parametrize("t_stop", VR.T_STOPS)
def test_an_opaque_sample_gives_finite_gradients(torch_cuda, t_stop):
    (alpha, values, ranges, g), _, _, ray, _ = reference(65, 3, t_stop)
    alpha = alpha.copy()
    for r in np.nonzero(ranges[:, 1] >= 15)[0]:  # alpha = 1 in rays of both kernels, at varying depths
        alpha[ranges[r, 0] + (3 + r) % 15] = 1.0
    L = VR.composite_loops(alpha, values, ranges, t_stop, *g)
    got = gpu_composite(alpha, values, ranges, t_stop, *g)
    f64 = lambda x: torch.from_numpy(x.astype(np.float64))
    keep = ~VR.ambiguous_rays(VR.composite(f64(alpha), f64(values), ranges, t_stop)[4], ranges, t_stop)
    assert keep.mean() >= 0.95 and np.array_equal(got["n"][keep], L["n"][keep])
    check(got, L, ranges, keep, ray, keep[ray], ("out", "opacity", "weights", "g_alpha", "g_values"))


def test_two_runs_are_bitwise_equal(torch_cuda):
    (alpha, values, ranges, g), *_ = reference(200, 7, 1e-4)
    a, b = gpu_composite(alpha, values, ranges, 1e-4, *g), gpu_composite(alpha, values, ranges, 1e-4, *g)
    assert all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in a)


def test_ranges_outside_the_samples_are_empty_and_second_order_raises(torch_cuda):
    from neus2_amd import volrend
    a = torch.full((40,), 0.1, device="cuda", requires_grad=True)
    v = torch.ones((40, 2), device="cuda")
    ranges = torch.tensor([[0, 40], [30, 20], [-1, 4], [40, 0]], dtype=torch.int32, device="cuda")
    out, op, w, n = volrend.composite(a, v, ranges, 0.0)
    assert n.tolist() == [40, 0, 0, 0] and out[1:].abs().sum() == 0
    g, = torch.autograd.grad(op.sum(), a, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable|does not require grad"):
        g.sum().backward()
