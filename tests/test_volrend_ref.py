"""The rendering operators' references (tests/volrend_ref.py) against each other, the Python argument checks of
neus2_amd/volrend.py, the C-ABI group, and the input conditions of the GPU cases, all without a GPU."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import volrend_ref as VR

f64 = lambda x: torch.from_numpy(np.asarray(x, np.float64))


# ---------------------------------------------------------------------------------------------- the references
@pytest.mark.parametrize("t_stop", VR.T_STOPS)
def test_composite_float64_equals_the_loops_and_their_recurrence(t_stop):
    alpha, values, ranges, (g_out, g_op, g_w) = VR.composite_case(65, 3)
    alpha = alpha.copy()
    alpha[ranges[5, 0] + 3] = 1.0  # an opaque sample: the recurrence divides by nothing
    a, v = f64(alpha).requires_grad_(), f64(values).requires_grad_()
    out, op, w, n, _ = VR.composite(a, v, ranges, t_stop)
    L = VR.composite_loops(alpha, values, ranges, t_stop, g_out, g_op, g_w)
    assert np.array_equal(n, L["n"])
    for got, key in ((out, "out"), (op, "opacity"), (w, "weights")):
        assert np.abs(got.detach().numpy() - L[key]).max() <= 1e-13, key
    ((out * f64(g_out)).sum() + (op * f64(g_op)).sum() + (w * f64(g_w)).sum()).backward()
    assert np.abs(a.grad.numpy() - L["g_alpha"]).max() <= 1e-13
    assert np.abs(v.grad.numpy() - L["g_values"]).max() <= 1e-13
    assert np.isfinite(L["g_alpha"]).all()
    if t_stop > 0:
        assert (n < ranges[:, 1]).any(), "no ray stops early"
        past = np.concatenate([np.arange(s + k, s + c) for (s, c), k in zip(ranges.tolist(), n)])
        assert (L["weights"][past] == 0).all() and (a.grad.numpy()[past] == 0).all()


def test_stock_formulation_agrees_with_float64():
    alpha, values, ranges, _ = VR.composite_case(65, 3)
    for t_stop in VR.T_STOPS:
        out, op, w, n, T = VR.composite(f64(alpha), f64(values), ranges, t_stop)
        keep = ~VR.ambiguous_rays(T, ranges, t_stop)
        so, sp, sw, sn = VR.composite_stock(torch.from_numpy(alpha), torch.from_numpy(values), torch.from_numpy(ranges), t_stop)
        assert np.array_equal(sn.numpy()[keep], n[keep])
        assert np.abs(so.numpy() - out.numpy())[keep].max() < 1e-4 and np.abs(sp.numpy() - op.numpy())[keep].max() < 1e-4


# ---------------------------------------------------------------------------------------------- argument checks
def _march_args(**kw):
    a = dict(rays_o=torch.zeros(4, 3), rays_d=torch.zeros(4, 3), t_min=torch.zeros(4), t_max=torch.ones(4),
             occupancy=torch.ones((8, 8, 8), dtype=torch.uint8), dt=0.01, max_per_ray=16)
    a.update(kw)
    return a


@pytest.mark.parametrize("name,value", [
    ("rays_o", torch.zeros(4, 2)), ("rays_o", np.zeros((4, 3), np.float32)), ("rays_d", torch.zeros(5, 3)),
    ("rays_d", torch.zeros(4, 3, dtype=torch.float64)), ("t_min", torch.zeros(4, 1)), ("t_max", torch.zeros(8)[::2]),
    ("occupancy", torch.ones((6, 6, 6), dtype=torch.uint8)), ("occupancy", torch.ones((8, 8, 4), dtype=torch.uint8)),
    ("occupancy", torch.ones((8, 8, 8), dtype=torch.bool)), ("occupancy", torch.ones((1024, 1, 1), dtype=torch.uint8)),
    ("dt", 0.0), ("dt", -1.0), ("dt", float("nan")), ("dt", torch.tensor(0.1)), ("max_per_ray", -1), ("max_per_ray", 1.5),
    ("rays_o", torch.zeros(4, 3)),  # everything valid but the device
])
def test_march_checks_its_arguments(name, value):
    from neus2_amd import volrend
    with pytest.raises(ValueError, match="^" + name + ":"):
        volrend.march(**_march_args(**{name: value}))


def _alpha_args(**kw):
    a = dict(sdf=torch.zeros(6), true_cos=torch.zeros(6), dt=torch.full((6,), 0.01), inv_s=torch.tensor(20.0), cos_anneal_ratio=0.5)
    a.update(kw)
    return a


@pytest.mark.parametrize("name,value", [
    ("sdf", torch.zeros(6, 1)), ("sdf", torch.zeros(6, dtype=torch.float16)), ("true_cos", torch.zeros(5)), ("dt", torch.zeros(7)),
    ("dt", 0.0), ("dt", -0.5), ("dt", torch.full((6,), 0.01, requires_grad=True)), ("inv_s", torch.zeros(2)),
    ("inv_s", torch.tensor(20.0, dtype=torch.float64)), ("inv_s", "20"), ("cos_anneal_ratio", 1.5), ("cos_anneal_ratio", -0.1),
    ("cos_anneal_ratio", torch.tensor(0.5)), ("sdf", torch.zeros(6)),
])
def test_neus_alpha_checks_its_arguments(name, value):
    from neus2_amd import volrend
    with pytest.raises(ValueError, match="^" + name + ":"):
        volrend.neus_alpha(**_alpha_args(**{name: value}))


def _comp_args(**kw):
    a = dict(alpha=torch.zeros(6), values=torch.zeros(6, 3), ranges=torch.tensor([[0, 4], [4, 2]], dtype=torch.int32), t_stop=1e-4)
    a.update(kw)
    return a


@pytest.mark.parametrize("name,value", [
    ("alpha", torch.zeros(6, 1)), ("alpha", torch.zeros(6, dtype=torch.float64)), ("values", torch.zeros(5, 3)), ("values", torch.zeros(6)),
    ("values", torch.zeros(6, 9)), ("values", torch.zeros(6, 0)), ("values", torch.zeros(3, 6).t()),
    ("ranges", torch.tensor([[0, 4], [4, 2]])), ("ranges", torch.zeros(2, 3, dtype=torch.int32)), ("ranges", torch.zeros(4, dtype=torch.int32)),
    ("t_stop", -1e-4), ("t_stop", float("nan")), ("t_stop", None), ("alpha", torch.zeros(6)),
])
def test_composite_checks_its_arguments(name, value):
    from neus2_amd import volrend
    with pytest.raises(ValueError, match="^" + name + ":"):
        volrend.composite(**_comp_args(**{name: value}))


@pytest.mark.parametrize("name,value", [
    ("normals", torch.zeros(6, 2)), ("dirs", torch.zeros(5, 3)), ("rgb", torch.zeros(6, 4)), ("t", torch.zeros(6, 1)),
    ("ranges", torch.zeros(2, 2)), ("sdf", torch.zeros(6)),
])
def test_render_neus_checks_its_arguments(name, value):
    from neus2_amd import volrend
    a = dict(sdf=torch.zeros(6), normals=torch.zeros(6, 3), dirs=torch.zeros(6, 3), dt=0.01, rgb=torch.zeros(6, 3), t=torch.zeros(6),
             inv_s=20.0, ranges=torch.tensor([[0, 4], [4, 2]], dtype=torch.int32), cos_anneal_ratio=0.5)
    a[name] = value
    with pytest.raises(ValueError, match="^" + name + ":"):
        volrend.render_neus(**a)


# ---------------------------------------------------------------------------------------------- the C-ABI group
SYMBOLS = ["neus_volrend_march_count", "neus_volrend_march_write", "neus_volrend_alpha_forward", "neus_volrend_alpha_backward",
           "neus_volrend_composite_forward", "neus_volrend_composite_backward"]


def test_library_exports_the_group_and_reports_abi_9():
    from neus2_amd import _lib
    assert set(SYMBOLS) <= set(_lib.EXPORTS) and _lib.ABI_VERSION == 9
    l = _lib.lib()  # raises unless the library reports ABI 9
    v = C.c_uint32(0)
    assert l.neus_abi_version(C.byref(v)) == 0 and v.value == 9
    assert all(hasattr(l, s) for s in SYMBOLS)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "neus2_hip.h")).read()
    assert "#define NEUS_ABI_VERSION 9u" in header


def test_host_validation_goes_through_last_error():
    """A bad size is an error status with a message, before any device call (no GPU needed)."""
    from neus2_amd import _lib
    l = _lib.lib()
    rc = l.neus_volrend_composite_forward(None, C.c_uint32(1), C.c_uint32(1), C.c_uint32(9), None, None, None, C.c_float(0.0), None, None, None, None, None)
    assert rc != 0 and "n_channels must be 1..8" in l.neus_last_error().decode()
    rc = l.neus_volrend_march_count(None, C.c_uint32(1), C.c_void_p(8), C.c_void_p(8), C.c_void_p(8), C.c_void_p(8), C.c_void_p(8), C.c_uint32(12),
                                    C.c_float(0.1), C.c_uint32(4), C.c_void_p(8))
    assert rc != 0 and "power of two" in l.neus_last_error().decode()


# ---------------------------------------------------------------------------------------------- input conditions of the GPU cases
@pytest.mark.parametrize("inv_s,ratio", VR.ALPHA_CASES)
@pytest.mark.parametrize("S", VR.ALPHA_SIZES)
def test_alpha_inputs_stay_off_the_clamp_and_the_relu_kinks(S, inv_s, ratio):
    sdf, cos, dt, _ = VR.alpha_case(S)
    q, _ = VR.alpha_terms(f64(sdf), f64(cos), f64(dt), inv_s, ratio)
    assert 1e-4 < float(q.min()) and float(q.max()) < 1 - 1e-4, (float(q.min()), float(q.max()))
    c = np.abs(cos.astype(np.float64))
    assert (c >= 0.05 - 1e-7).all() and (c <= 0.95 + 1e-7).all()
    assert (c > 1e-3).all() and (np.abs(c - 1) > 1e-3).all()


def test_alpha_worst_corner_of_the_input_box_stays_above_the_bound():
    """Not only the drawn samples: the corner of the box (sdf = 0.05, cos = 0.95) that minimises q."""
    for inv_s, ratio in VR.ALPHA_CASES:
        q, _ = VR.alpha_terms(f64([0.05, -0.05, 0.05, -0.05]), f64([0.95, 0.95, -0.95, -0.95]), f64([VR.DT] * 4), inv_s, ratio)
        assert 1e-4 < float(q.min()) and float(q.max()) < 1 - 1e-4, (inv_s, ratio, q)


@pytest.mark.parametrize("R", VR.RAYS)
@pytest.mark.parametrize("C_", VR.CHANNELS)
def test_composite_inputs_have_few_ambiguous_rays_and_reach_every_branch(R, C_):
    alpha, values, ranges, _ = VR.composite_case(R, C_)
    n = ranges[:, 1]
    assert ranges[:, 0].tolist() == np.concatenate([[0], np.cumsum(n)[:-1]]).tolist()
    if R >= 65:
        assert set(n.tolist()) == set(VR.LENGTHS)
    _, _, _, taken, T = VR.composite(f64(alpha), f64(values), ranges, 1e-4)
    amb = VR.ambiguous_rays(T, ranges, 1e-4)
    assert amb.mean() <= 0.05, amb.mean()
    long_ = n == 300
    assert ((taken[long_] > 64) & (taken[long_] < 300)).all(), "the 300-sample rays stop mid-ray"
    assert not VR.ambiguous_rays(T, ranges, 0.0).any()


def test_march_restatement_is_the_same_in_two_evaluation_orders():
    o, d, t_min, t_max, occ = VR.march_case()
    dt = float(np.float32(np.sqrt(3.0) / 64))
    a = VR.march_by_ray(o, d, t_min, t_max, occ, dt, 48)
    b = VR.march_by_step(o, d, t_min, t_max, occ, dt, 48)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8))
    n = a[0][:, 1]
    assert (n == 48).any() and (n == 0).sum() >= 20 and ((n > 0) & (n < 48)).sum() > 50 and n.sum() == len(a[1])
    assert (n[-20:] == 0).all()  # the rays that miss the cube and those with t_min >= t_max
    # the restatement with max_per_ray out of reach: the capped rays really had more occupied steps
    assert (VR.march_by_ray(o, d, t_min, t_max, occ, dt, 1 << 20)[0][:, 1] > 48).any()
