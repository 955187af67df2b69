"""The call protocol every operator module shares (neus_module_backward / _backward_backward_input: context check, batch
capacity, gradient modes), for one configuration per encoding x network combination, n = 128 on a capacity of 256,
"gradient_precision": "fp32":

  Accumulate    into a dL_dparams pre-filled with C = 0.5 equals C + the Overwrite result. Bitwise where the gradient has no
                floating-point atomics (the Accumulate epilogue is one fp32 add per entry, as torch's C + g). The general
                grid's and the fp32 HashGrid's table gradients are summed by atomics in no fixed order: the accumulated entry
                is an fp32 sum of K' = K + 1 terms (the K scattered ones and C) in two orders, which differ by at most
                2 (K' - 1) 2^-24 (S + |C|) with S the sum of the scattered terms' absolute values. K <= n 2^D; S is the same
                scatter on absolute values in float64 (atomic_sums below; in front of an MLP |dL/dX0| is bounded by |dL_doutput|
                carried through the absolute weight matrices, x 1.01 for the fp16 roundings of the chain).
  Ignore        with no other output asked for leaves a poisoned dL_dparams untouched.
  context       a context of a forward over another n is refused ("... context ...").
  capacity      n > batch_capacity is refused by forward and inference.

CONFIGS, make and case_tensors also serve an A/B of two builds of the library (NEUS2_HIP_LIB), one process per build."""
import os

import numpy as np
import pytest

import grid_nd_ref as G

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, CAP, C0 = 128, 256, 0.5

NET16 = {"otype": "FullyFusedMLP", "n_neurons": 16, "n_hidden_layers": 1, "activation": "ReLU", "output_activation": "None"}
NET64 = {"otype": "FullyFusedMLP", "n_neurons": 64, "n_hidden_layers": 2, "activation": "ReLU", "output_activation": "None"}
NET64_SIGMOID = dict(NET64, output_activation="Sigmoid")
DNET = dict(NET64, n_hidden_layers=1)
FREQ = {"otype": "Frequency", "n_frequencies": 4}
COMPOSITE = {"otype": "Composite", "nested": [{"otype": "Frequency", "n_dims_to_encode": 3, "n_frequencies": 4},
                                             {"otype": "SphericalHarmonics", "degree": 3}]}
# three levels of resolution 4, 8, 16: the coarsest dense (64 entries), the finer two hashed into 2^8
HASH = {"otype": "HashGrid", "n_levels": 3, "n_features_per_level": 2, "log2_hashmap_size": 8, "base_resolution": 4, "per_level_scale": 2.0}
ND2 = {"otype": "Grid", "type": "Dense", "interpolation": "Smoothstep", "n_levels": 3, "n_features_per_level": 4, "base_resolution": 4,
       "per_level_scale": 2.0, "log2_hashmap_size": 8}
ND3 = {"otype": "Grid", "type": "Tiled", "n_levels": 3, "n_features_per_level": 1, "base_resolution": 4, "per_level_scale": 2.0,
       "log2_hashmap_size": 8}

# name -> (constructor, n_input_dims, n_output_dims, encoding, network, precision, training_step)
CONFIGS = {
    "mlp16": ("network", 5, 3, None, NET16, "fp16", 0),
    "mlp64_sigmoid": ("network", 20, 7, None, NET64_SIGMOID, "fp16", 0),
    "identity_scaled_mlp": ("nwie", 5, 3, {"otype": "Identity", "scale": 2.0, "offset": 0.25}, NET16, "fp16", 0),
    "frequency": ("encoding", 3, 0, FREQ, None, "fp16", 0),
    "composite_aos_fp16": ("encoding", 6, 0, COMPOSITE, None, "fp16", 0),
    "composite_soa_fp16": ("encoding", 6, 0, dict(COMPOSITE, output_layout="SoA"), None, "fp16", 0),
    "composite_aos_fp32": ("encoding", 6, 0, COMPOSITE, None, "fp32", 0),
    "composite_soa_fp32": ("encoding", 6, 0, dict(COMPOSITE, output_layout="SoA"), None, "fp32", 0),
    "composite_mlp": ("nwie", 6, 4, COMPOSITE, NET64, "fp16", 0),
    "hash_aos_fp16": ("encoding", 3, 0, HASH, None, "fp16", 0),
    "hash_soa_fp16": ("encoding", 3, 0, dict(HASH, output_layout="SoA"), None, "fp16", 0),
    "hash_paired_fp16": ("encoding", 3, 0, dict(HASH, output_layout="paired"), None, "fp16", 0),
    "hash_aos_fp32": ("encoding", 3, 0, HASH, None, "fp32", 0),
    "hash_soa_fp32": ("encoding", 3, 0, dict(HASH, output_layout="SoA"), None, "fp32", 0),
    "hash_dnet": ("nwie", 3, 16, HASH, DNET, "fp16", 0),
    "hash_mlp": ("nwie", 3, 5, HASH, NET64, "fp16", 0),
    "nd2_dense_smoothstep": ("encoding", 2, 0, ND2, None, "fp32", 0),
    "nd3_tiled": ("encoding", 3, 0, dict(ND3, output_layout="SoA"), None, "fp16", 0),
    "nd2_dense_smoothstep_mlp": ("nwie", 2, 4, ND2, NET64, "fp16", 0),
    "nd3_tiled_mlp": ("nwie", 3, 4, ND3, NET16, "fp16", 0),
    "nerf": ("nerf", 7, 16, None, None, "fp16", 0),
    # set_training_step(1): tcnn's defaults give ceil(0.5 * 3) = 2 valid levels, the finest is masked
    "hash_aos_fp16_step1": ("encoding", 3, 0, HASH, None, "fp16", 1),
    "hash_mlp_step1": ("nwie", 3, 5, HASH, NET64, "fp16", 1),
}
# the table gradient is accumulated by floating-point atomics: name -> (grid config, grid type, interpolation)
ATOMIC = {
    "hash_aos_fp32": (HASH, "Hash", "Linear"), "hash_soa_fp32": (HASH, "Hash", "Linear"),
    "nd2_dense_smoothstep": (ND2, "Dense", "Smoothstep"), "nd3_tiled": (ND3, "Tiled", "Linear"),
    "nd2_dense_smoothstep_mlp": (ND2, "Dense", "Smoothstep"), "nd3_tiled_mlp": (ND3, "Tiled", "Linear"),
}


def make(name, capacity=CAP):
    from neus2_amd import config
    from neus2_amd.module import Module, Precision
    kind, n_in, n_out, enc, net, prec, step = CONFIGS[name]
    if kind == "network":
        m = Module.create_network(n_in, n_out, dict(net, gradient_precision="fp32"), batch_capacity=capacity)
    elif kind == "nwie":
        m = Module.create_network_with_input_encoding(n_in, n_out, enc, dict(net, gradient_precision="fp32"), batch_capacity=capacity)
    elif kind == "encoding":
        m = Module.create_encoding(dict(enc, gradient_precision="fp32"), batch_capacity=capacity, n_input_dims=n_in,
                                   requested_precision=Precision.Fp32 if prec == "fp32" else Precision.Fp16)
    else:
        cfg = config.load_json(os.path.join(ROOT, "configs", "nerf", "base.json"))
        m = Module.create_nerf_network(dict(cfg, gradient_precision="fp32"), batch_capacity=capacity)
    if step:
        m.set_training_step(step)
    return m


def case_tensors(t, m, name, n, seed=0):
    """input, params (the module's precision; the tables scaled up from their 1e-4 initialisation), dL_doutput, dL_ddLdinput"""
    kind, n_in, *_ = CONFIGS[name]
    g = t.Generator(device="cpu").manual_seed(1000 * seed + n)
    x = t.rand((n, n_in), generator=g) * 0.9 + 0.05
    if kind == "nerf":  # NerfCoordinate: position, dt, direction mapped to [0, 1]
        d = t.randn((n, 3), generator=g)
        x[:, 3] = 0.01
        x[:, 4:] = (d / d.norm(dim=1, keepdim=True) + 1) * 0.5
    p = m.initialize_params(7 + seed)
    if kind != "nerf" and m.info["n_levels"]:
        p[m.info["grid_offset"]:] *= 1000.0
    params = p if m.precision == "fp32" else p.half()
    shape = m.output_shape(n)
    dlo = t.randn(shape, generator=g).to(t.float32 if m.precision == "fp32" else t.float16)
    u = t.randn((n, n_in), generator=g)
    return x.cuda().contiguous(), params.contiguous(), dlo.cuda().contiguous(), u.cuda().contiguous()


def bbi_asks(name):
    """which of (dL_ddLdoutput, dL_dinput) backward_backward_input provides for the configuration"""
    if name == "mlp64_sigmoid":  # not exact with an output activation: the parameter gradients alone
        return False, False
    return True, "composite" not in name  # no second derivative of the spherical harmonics


def atomic_sums(x, dy_abs, u, cfg, n_dims, grid_type, interpolation):
    """Per table entry [n_entries, F] in float64: the sum of |w_c| |dy| over samples and corners (backward's terms) and of
    |sum_d u_d dw_c/dx_d| |dy| (backward_backward_input's)."""
    import torch
    F, L = cfg["n_features_per_level"], cfg["n_levels"]
    off, res = G.level_tables(n_dims, L, cfg["log2_hashmap_size"], cfg["base_resolution"], cfg["per_level_scale"], grid_type)
    S1 = torch.zeros(off[-1], F, dtype=torch.float64)
    S2 = torch.zeros(off[-1], F, dtype=torch.float64)
    x = x.double().clone().requires_grad_(True)
    for l in range(L):
        p = x * float(res[l] - 1) + 0.5
        g = torch.floor(p.detach()).to(torch.int64)
        w1 = G.interpolation_weight(p - g.to(x.dtype), interpolation)
        for c in range(1 << n_dims):
            bits = [(c >> d) & 1 for d in range(n_dims)]
            w = 1
            for d in range(n_dims):
                w = w * (w1[:, d] if bits[d] else 1 - w1[:, d])
            a = (torch.autograd.grad(w.sum(), x, retain_graph=True)[0] * u).sum(1).abs()
            e = G.index(off[l + 1] - off[l], res[l], g + torch.tensor(bits, dtype=torch.int64), grid_type) + off[l]
            dy = dy_abs[:, l * F:(l + 1) * F]
            S1.index_add_(0, e, w.detach().abs()[:, None] * dy)
            S2.index_add_(0, e, a[:, None] * dy)
    return S1.reshape(-1).numpy(), S2.reshape(-1).numpy()


def atomic_tolerance(t, m, name, x, params, dlo, u, n, c=C0):
    """2 K 2^-24 (S + |c|) per table entry for backward and backward_backward_input, K = n 2^D (c: the pre-filled constant)"""
    kind, n_in, n_out, enc, net, *_ = CONFIGS[name]
    cfg, ty, ip = ATOMIC[name]
    width = cfg["n_features_per_level"] * cfg["n_levels"]
    dy = dlo.double().cpu().abs()
    if m.output_layout == "SoA":
        dy = dy.T
    if net is not None:  # |dL/dX0| <= |dL_doutput| |W_N| ... |W_0|
        W, nh = net["n_neurons"], net["n_hidden_layers"]
        in_pad = (width + 15) // 16 * 16
        shapes = [(W, in_pad)] + [(W, W)] * (nh - 1) + [(16, W)]
        mats, o = [], 0
        for r, k in shapes:
            mats.append(params[o:o + r * k].double().cpu().abs().reshape(r, k))
            o += r * k
        for M in reversed(mats):
            dy = dy @ M
        dy = dy[:, :width] * 1.01
    S1, S2 = atomic_sums(x.cpu(), dy, u.double().cpu(), cfg, n_in, ty, ip)
    k = 2.0 * n * (1 << n_in) * 2.0 ** -24
    return k * (S1 + abs(c)), k * (S2 + abs(c))


def check_accumulated(t, name, what, m, ow, acc, tol):
    """acc = C0 + ow: bitwise, except the atomically accumulated table gradient (tol per entry)"""
    exp = ow + C0
    go = m.info["grid_offset"] if name in ATOMIC else m.n_params
    assert t.equal(acc[:go], exp[:go]), f"{name} {what}: Accumulate != C + Overwrite in the atomic-free gradients"
    if go < m.n_params:
        d = (acc[go:].double() - exp[go:].double()).abs().cpu().numpy()
        print(f"{name} {what}: max |Accumulate - (C + Overwrite)| = {d.max():.3e}, smallest bound {tol.min():.3e}")
        assert (d <= tol).all(), f"{name} {what}: {d.max():.3e} above the summation bound at entry {int(np.argmax(d - tol))}"


@pytest.mark.parametrize("name", list(CONFIGS))
def test_module_protocol(torch_cuda, name):
    from neus2_amd._lib import NeusError
    from neus2_amd.module import GradientMode
    t = torch_cuda
    m = make(name)
    n_in = CONFIGS[name][1]
    x, params, dlo, u = case_tensors(t, m, name, N)
    P = m.n_params
    tol1, tol2 = atomic_tolerance(t, m, name, x, params, dlo, u, N) if name in ATOMIC else (None, None)
    full = lambda v: t.full((P,), v, dtype=t.float32, device="cuda")
    ctx, y = m.forward(x, params, prepare_input_gradients=True)

    # n > capacity, and a context of a forward over another n
    big = t.zeros((CAP + 128, n_in), dtype=t.float32, device="cuda")
    with pytest.raises(NeusError, match="n_elements exceeds the module's batch capacity"):
        m.forward(big, params)
    with pytest.raises(NeusError, match="n_elements exceeds the module's batch capacity"):
        m.inference(big, params)
    ctx2, y2 = m.forward(t.cat([x, x]), params, prepare_input_gradients=True)

    # backward
    ow, dx = full(7.0), t.full((N, n_in), 7.0, dtype=t.float32, device="cuda")
    m.backward(ctx, x, dlo, params, dL_dparams=ow, dL_dinput=dx, mode=GradientMode.Overwrite, output=y)
    acc, dx_acc = full(C0), t.full((N, n_in), 7.0, dtype=t.float32, device="cuda")
    m.backward(ctx, x, dlo, params, dL_dparams=acc, dL_dinput=dx_acc, mode=GradientMode.Accumulate, output=y)
    check_accumulated(t, name, "backward", m, ow, acc, tol1)
    assert t.equal(dx, dx_acc) and bool(t.isfinite(dx).all())
    poison = full(float("nan"))
    m.backward(ctx, x, dlo, params, dL_dparams=poison, dL_dinput=None, mode=GradientMode.Ignore, output=y)
    assert bool(t.isnan(poison).all())
    ctx2.n = N
    with pytest.raises(NeusError, match="module backward: the context is not from a forward over n_elements"):
        m.backward(ctx2, x, dlo, params, dL_dparams=full(0.0), dL_dinput=None, mode=GradientMode.Overwrite, output=y)
    ctx2.n = 2 * N
    if name == "nerf":  # its second order is part of backward
        return

    # backward_backward_input, with what the configuration provides
    want_ddo, want_dx = bbi_asks(name)
    out = lambda want, ref: t.full(tuple(ref.shape), 7.0, dtype=ref.dtype, device="cuda") if want else None
    ow, ddo, ddx = full(7.0), out(want_ddo, y), out(want_dx, x)
    m.backward_backward_input(ctx, x, u, dlo, params, dL_dparams=ow, dL_ddLdoutput=ddo, mode=GradientMode.Overwrite, dL_dinput=ddx)
    acc, ddo_acc, ddx_acc = full(C0), out(want_ddo, y), out(want_dx, x)
    m.backward_backward_input(ctx, x, u, dlo, params, dL_dparams=acc, dL_ddLdoutput=ddo_acc, mode=GradientMode.Accumulate, dL_dinput=ddx_acc)
    check_accumulated(t, name, "backward_backward_input", m, ow, acc, tol2)
    assert ddo is None or t.equal(ddo, ddo_acc)
    assert ddx is None or t.equal(ddx, ddx_acc)
    poison = full(float("nan"))
    m.backward_backward_input(ctx, x, u, dlo, params, dL_dparams=poison, dL_ddLdoutput=None, mode=GradientMode.Ignore, dL_dinput=None)
    assert bool(t.isnan(poison).all())
    ctx2.n = N
    with pytest.raises(NeusError, match="backward_backward_input: needs the forward's context"):
        m.backward_backward_input(ctx2, x, u, dlo, params, dL_dparams=full(0.0), dL_ddLdoutput=None, mode=GradientMode.Overwrite)
    ctx2.n = 2 * N
