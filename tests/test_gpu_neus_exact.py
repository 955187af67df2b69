"""The fused NeuS network kernels of mlp.hip (k_nerf_infer, k_nerf_density, k_mlp_train_rgb, k_mlp_train_density,
k_mlp_grad_reduce) against exact references, bit for bit and element by element, for all seven NEUS_MLP_CONFIGS.

* Forward and backward on the exact domain of tests/neus_int_net.py ({-1, 0, 1} matrices, a zero table, positions in
  eighths, axis directions, integer dL/doutput): every fp32 accumulation is exact whatever its order, tile mapping or block
  split, so the device must reproduce the float64 reference's bytes. The training kernels run alone through
  neus_debug_mlp_train on caller-given integer encodings and dyadic dy/dx (with a zero table load_enc, load_dydx, the
  encoding columns of dW_d0, the G . dy/dx contraction, the dy/dx . v entries of u and the genc / dLdenc writes see
  nothing but zeros); the same hook on zero encodings equals neus_net_backward_pos on the zero table, which ties it to the
  production path. The persistent loops get one chunk more than the launchers' largest possible grids.
* The fused encode (fused_levels, slot_value, slot_dydx, the overflow slots, the host-side din permutation) on a random
  +-0.1 table: selector matrices route one density-input column at a time to the output, where it must equal the
  oracle's encode of the same position bit for bit, feature and dy/dx, through k_nerf_infer (both variants) and through
  k_nerf_density (neus_testbed_sdf_on_grid)."""
import ctypes as C
import os

import numpy as np
import pytest

import neus_int_net as N
from edge_positions import edge_positions
from gpu_util import dev, host, ptr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [f"L{L}_W{W}" for L, W in N.CONFIGS]
BATCH = 4096
OUT_FILL = np.int16(0x7b7b)
F32_FILL = np.float32(-123.456)


@pytest.fixture(scope="module")
def scene():
    from neus2_amd import scenes
    return scenes.small_scene(n_views=8, width=64, height=48)


def _testbed(scene, L, W, batch):
    from neus2_amd import config, pyngp
    cfg = config.load_json(os.path.join(ROOT, "configs", "nerf", "base.json"))
    cfg["encoding"]["n_levels"] = L
    cfg["network"]["n_neurons"] = W
    cfg["rgb_network"]["n_neurons"] = W
    tb = pyngp.Testbed(pyngp.TestbedMode.Nerf)
    tb.set_dataset(scene["images"], scene["focal"], scene["principal"], scene["xforms"], 1)
    tb.reload_network_from_json(cfg, batch_size=batch)
    lay = tb.layout()
    assert lay["n_levels"] == L and lay["density_input_width"] == N.din_width(L)
    assert lay["n_matrix"] == N.din_width(L) * W + 16 * W + 48 * W + W * W + 16 * W and lay["grid_offset"] == lay["n_matrix"]
    return tb


@pytest.fixture(scope="module")
def beds(torch_cuda, scene):
    """Testbeds by config, made on first use (batch_size 4096; base.json with n_levels / n_neurons overridden)."""
    made = {}

    def get(L, W):
        if (L, W) not in made:
            made[(L, W)] = _testbed(scene, L, W, BATCH)
        return made[(L, W)]
    return get


def _variance(tb):
    lay = tb.layout()
    return float(tb.get_params()[lay["variance_offset"]])


def _forward(t, tb, coords, valid, pad=64):
    """neus_net_forward over a sentinel-filled buffer of n + pad rows: (rows [n][16] u16, the tail's bytes)."""
    from neus2_amd._lib import check, lib
    n = len(coords)
    out = t.from_numpy(np.full((n + pad, 16), OUT_FILL, np.int16)).cuda()
    check(lib().neus_net_forward(tb.handle, None, C.c_uint32(n), ptr(dev(t, coords)), C.c_uint32(valid), ptr(out)))
    t.cuda.synchronize()
    o = host(out, np.uint16)
    return o[:n], o[n:]


# ---------------------------------------------------------------------------------------- forward, zero table
@pytest.mark.parametrize("cfg", N.CONFIGS, ids=IDS)
def test_forward_rows_bitwise(beds, torch_cuda, cfg):
    """All 16 output columns of every row equal the reference's bytes at n = 1 .. 4097 (partial waves, one and several
    blocks), with every level valid (the ALL instantiation of k_nerf_infer) and with valid_level 0 (the other one; the
    table is zero, so the rows are the same); the buffer past row n keeps its sentinel."""
    t = torch_cuda
    L, W = cfg
    tb = beds(L, W)
    var = _variance(tb)
    for n in N.FWD_SIZES:
        net = N.make(L, W, n, N.seed_of(L, W, n), variance=var, backward=False)
        N.check_domain(net)
        tb.set_params(N.param_vector(net, tb.get_params()))
        for valid in (L, 0):
            got, tail = _forward(t, tb, net.coords, valid)
            assert np.all(tail == OUT_FILL.view(np.uint16)), (n, valid, "written past row n")
            np.testing.assert_array_equal(got, net.out.view(np.uint16), err_msg=f"n={n} valid_level={valid}")


def test_forward_second_persistent_iteration(beds, torch_cuda):
    """(14, 64) at n = 128 * 8192 + 33: one chunk more than the launcher's largest grid, so block 0 runs a second
    iteration whatever the device's resident capacity, and the last wave is partial. The first and last 4096 rows and
    4096 random ones against the reference."""
    t = torch_cuda
    L, W, n = 14, 64, N.FWD_LARGE
    tb = beds(L, W)
    rows = N.large_forward_rows(n)
    net = N.make(L, W, n, N.seed_of(L, W, n), variance=_variance(tb), rows=rows, backward=False)
    N.check_domain(net)
    tb.set_params(N.param_vector(net, tb.get_params()))
    got, tail = _forward(t, tb, net.coords, L)
    assert np.all(tail == OUT_FILL.view(np.uint16))
    np.testing.assert_array_equal(got[rows], net.out.view(np.uint16))


# ---------------------------------------------------------------------------------------- the training kernels alone
def _train(t, tb, net, enc, dydx, n_params):
    """neus_debug_mlp_train on the net's operands; every output over a sentinel-filled buffer."""
    from neus2_amd._lib import check, lib
    n, L = net.n, net.L
    fill16 = lambda *s: t.from_numpy(np.full(s, OUT_FILL, np.int16)).cuda()
    fill32 = lambda *s: t.from_numpy(np.full(s, F32_FILL, np.float32)).cuda()
    g, dpos, v = fill32(n_params), fill32(n, 4), fill32(n, 4)
    genc, dlde, d1 = fill16(L, n, 2), fill16(L, n, 2), fill16(16, n)
    check(lib().neus_debug_mlp_train(tb.handle, None, C.c_uint32(n), ptr(dev(t, net.coords)), ptr(dev(t, N.paired(enc.astype(np.float16), L))),
                                     ptr(dev(t, N.dydx_rows(dydx))), ptr(dev(t, net.dL)), C.c_uint32(net.indeed), ptr(g), ptr(dpos),
                                     ptr(genc), ptr(dlde), ptr(d1), ptr(v)))
    t.cuda.synchronize()
    return dict(g=host(g, np.uint32), dpos=host(dpos, np.uint32), v=host(v, np.uint32), genc=host(genc, np.uint16),
                dLdenc=host(dlde, np.uint16), d1_delta=host(d1, np.uint16))


def _assert_train(got, net, lay, label):
    """Every element of the five matrix blocks, the variance gradient, dpos, genc, dLdenc, d1_delta and v."""
    nm, vo = lay["n_matrix"], lay["variance_offset"]
    g = got["g"]
    off = 0
    for name, ref in zip(("d0", "d1", "r0", "r1", "r2"), net.grads):
        np.testing.assert_array_equal(g[off:off + ref.size].reshape(ref.shape), ref.astype(np.float32).view(np.uint32), err_msg=f"{label}: dW {name}")
        off += ref.size
    assert off == nm
    np.testing.assert_array_equal(g[vo:vo + 4], np.float32([net.var_grad, 0, 0, 0]).view(np.uint32), err_msg=f"{label}: variance")
    assert not np.any(g[nm:vo]), f"{label}: the grid block of grads_out is not zero"
    np.testing.assert_array_equal(got["dpos"], net.dpos.view(np.uint32), err_msg=f"{label}: dpos")
    np.testing.assert_array_equal(got["v"], net.v.view(np.uint32), err_msg=f"{label}: v")
    np.testing.assert_array_equal(got["d1_delta"], np.ascontiguousarray(net.d1_delta.T).view(np.uint16), err_msg=f"{label}: d1_delta")
    np.testing.assert_array_equal(got["genc"], N.paired(net.genc, net.L).view(np.uint16), err_msg=f"{label}: genc")
    np.testing.assert_array_equal(got["dLdenc"], N.paired(net.dLdenc, net.L).view(np.uint16), err_msg=f"{label}: dLdenc")


@pytest.mark.parametrize("cfg", N.CONFIGS, ids=IDS)
def test_train_kernels_bitwise(beds, torch_cuda, cfg):
    """n = 128, 384, 1152 with dense integer dL/doutput, integer encodings and dyadic dy/dx."""
    t = torch_cuda
    L, W = cfg
    tb = beds(L, W)
    lay = tb.layout()
    for n in N.BWD_SIZES:
        seed = N.seed_of(L, W, n)
        enc, dydx = N.caller_encodings(L, n, seed)
        net = N.make(L, W, n, seed, enc, dydx)
        N.check_domain(net)
        tb.set_params(N.param_vector(net, tb.get_params()))
        _assert_train(_train(t, tb, net, enc, dydx, lay["n_params"]), net, lay, f"n={n}")


@pytest.mark.parametrize("cfg", N.CONFIGS, ids=IDS)
def test_train_hook_on_zero_encodings_is_the_production_backward(beds, torch_cuda, cfg):
    """enc = dy/dx = 0 through the hook equals the reference and neus_net_backward_pos on the zero table (encode, training
    kernels, reduction, scatter) in its matrix, variance and dpos outputs."""
    from neus2_amd._lib import check, lib
    t = torch_cuda
    L, W = cfg
    tb = beds(L, W)
    lay = tb.layout()
    nm, vo = lay["n_matrix"], lay["variance_offset"]
    for n in N.BWD_SIZES:
        net = N.make(L, W, n, N.seed_of(L, W, n))
        N.check_domain(net)
        tb.set_params(N.param_vector(net, tb.get_params()))
        got = _train(t, tb, net, np.zeros((n, 2 * L)), np.zeros((n, 2 * L, 3)), lay["n_params"])
        _assert_train(got, net, lay, f"n={n} zero encodings")
        g = t.from_numpy(np.full(lay["n_params"], F32_FILL, np.float32)).cuda()
        dpos = t.from_numpy(np.full((n, 4), F32_FILL, np.float32)).cuda()
        check(lib().neus_net_backward_pos(tb.handle, None, C.c_uint32(n), ptr(dev(t, net.coords)), C.c_uint32(L), ptr(dev(t, net.dL)),
                                          C.c_uint32(net.indeed), ptr(g), ptr(dpos)))
        t.cuda.synchronize()
        gp = host(g, np.uint32)
        np.testing.assert_array_equal(gp[:nm], got["g"][:nm], err_msg=f"n={n}: matrix blocks")
        np.testing.assert_array_equal(gp[vo:vo + 4], got["g"][vo:vo + 4], err_msg=f"n={n}: variance")
        np.testing.assert_array_equal(host(dpos, np.uint32), got["dpos"], err_msg=f"n={n}: dpos")


@pytest.mark.parametrize("cfg", N.BWD_LARGE_CONFIGS, ids=lambda c: f"L{c[0]}_W{c[1]}")
def test_train_kernels_second_persistent_iteration(torch_cuda, scene, cfg):
    """n = batch_size = 128 * 2049: one chunk more than mlp_train_blocks' largest grid, so block 0 accumulates its weight
    gradients over two chunks (register accumulators carried over, weights re-based) on any device. dL/doutput is nonzero
    on every row of chunks 0 and 2048 and on about 1 row in 320 elsewhere: the colour layers' sum |terms| stays below
    2^24 2^-12 (check_domain)."""
    t = torch_cuda
    L, W = cfg
    n, seed = N.BWD_LARGE, N.seed_of(L, W, N.BWD_LARGE)
    enc, dydx = N.caller_encodings(L, n, seed)
    net = N.make(L, W, n, seed, enc, dydx, dl_density=N.DL_DENSITY_LARGE)
    N.check_domain(net)
    tb = _testbed(scene, L, W, n)
    lay = tb.layout()
    tb.set_params(N.param_vector(net, tb.get_params()))
    _assert_train(_train(t, tb, net, enc, dydx, lay["n_params"]), net, lay, f"n={n}")


# ---------------------------------------------------------------------------------------- selector probes: the fused encode
def _selector(L, W, c):
    """The five matrices that route density-input column c to the output: D1[0] = D1[1] = din_c exactly (relu(t) -
    relu(-t)), passed through the colour layers to out[0]."""
    DIN = N.din_width(L)
    d0, d1, r0, r1, r2 = np.zeros((W, DIN)), np.zeros((16, W)), np.zeros((W, 48)), np.zeros((W, W)), np.zeros((16, W))
    d0[0, c], d0[1, c] = 1, -1
    d1[0, 0], d1[0, 1] = 1, -1
    d1[1, 0], d1[1, 1] = 1, -1
    r0[0, 1], r0[1, 1] = 1, -1
    r1[0, 0] = r1[1, 1] = 1
    r2[0, 0], r2[0, 1] = 1, -1
    return np.concatenate([m.ravel() for m in (d0, d1, r0, r1, r2)]).astype(np.float32)


def _h(a):
    return np.asarray(a).astype(np.float16)


def _probe_levels(L):
    return tuple(sorted({0, L // 2, L - 1}))


@pytest.fixture(scope="module")
def probe(beds, torch_cuda):
    """Per config: the testbed on a random +-0.1 table (as test_gpu_encode_edges sets it), the probe positions (that
    file's cell boundaries, level vertices, cube corners and outside positions, plus 1000 uniform ones) and the oracle's
    encode of them per valid level."""
    import oracle as O
    made = {}

    def get(L, W):
        if (L, W) in made:
            return made[(L, W)]
        tb = beds(L, W)
        lay = tb.layout()
        cfg = O.make_cfg(n_levels=L, width=W, per_level_scale=tb._net_cfg.per_level_scale)
        p = tb.get_params().copy()
        g0, g1 = lay["grid_offset"], lay["variance_offset"]
        p[g0:g1] = np.random.default_rng(21).uniform(-0.1, 0.1, g1 - g0).astype(np.float32)
        x = np.concatenate([edge_positions(O, cfg, 300, _probe_levels(L)), np.random.default_rng(23).uniform(0, 1, (1000, 3)).astype(np.float32)])
        c = np.zeros((len(x), 7), np.float32)
        c[:, :3] = x
        c[:, 4:] = np.random.default_rng(24).uniform(0, 1, (len(x), 3))
        made[(L, W)] = dict(tb=tb, O=O, cfg=cfg, params=p, coords=c, lay=lay)
        return made[(L, W)]
    return get


def _din_reference(e, L, valid, x=None):
    """The density input [n][3 + 2L] (fp16) and its dy/dx [n][3 + 2L][3] (fp32) at positions x from the oracle's encode."""
    x = e["coords"][:, :3] if x is None else x
    enc, dydx = e["O"].grid_forward(e["cfg"], e["params"], x, valid)
    n = len(x)
    din = np.zeros((n, 3 + 2 * L), np.float16)
    din[:, :3] = _h(_h(x).astype(np.float32) - np.float32(0.5))
    din[:, 3:] = _h(enc)
    dd = np.zeros((n, 3 + 2 * L, 3), np.float32)
    dd[:, :3] = np.eye(3, dtype=np.float32)
    dd[:, 3:] = dydx
    return din, dd


@pytest.mark.parametrize("cfg", N.CONFIGS, ids=IDS)
def test_selector_probes_fused_encode_in_inference(probe, torch_cuda, cfg):
    """One neus_net_forward per density-input column c and valid level (all levels: the ALL kernel; about L / 2):
    out[0] = din_c (fp16(fp16(x_c) - 0.5) for c < 3, else the oracle's feature c - 3), out[3] = fp16(din_c + fp16(bias))
    in one rounding, out[4:7] = fp16 of the oracle's fp32 dy/dx of that feature (e_c for c < 3) where din_c != 0 and 0
    where din_c = 0 (both ReLU masks are off there, x_c = 0.5 included); the other columns are 0, fp16(variance) and
    fp16(direction)."""
    t = torch_cuda
    L, W = cfg
    e = probe(L, W)
    tb, lay, c7 = e["tb"], e["lay"], e["coords"]
    nm = lay["n_matrix"]
    bias, var = _h(N.SDF_BIAS).astype(np.float64), _h(e["params"][lay["variance_offset"]])
    for valid in sorted({L, L // 2}):
        din, dd = _din_reference(e, L, valid)
        for c in range(3 + 2 * L):
            p = e["params"].copy()
            p[:nm] = _selector(L, W, c)
            tb.set_params(p)
            got, _ = _forward(t, tb, c7, valid)
            want = np.zeros((len(c7), 16), np.float16)
            want[:, 0] = din[:, c]
            want[:, 3] = _h(din[:, c].astype(np.float64) + bias)
            on = din[:, c] != 0
            want[:, 4:7] = np.where(on[:, None], _h(dd[:, c] + np.float32(0)), np.float16(0))
            want[:, 7] = var
            want[:, 8:11] = _h(c7[:, 4:7])
            np.testing.assert_array_equal(got, want.view(np.uint16), err_msg=f"column {c} valid_level {valid}")


def _sdf_grid_positions(res, amin, amax):
    """The float32 positions launch_sdf_grid generates: p = fma(g * (1 / res), max - min, min), then the warp into the
    training aabb [0, 1] (p - 0) / 1 = p. With the render aabb below the fma is evaluated exactly in float64 (g / res in
    fp32, times 1.5: at most 26 bits; minus 0.25: dyadic, far inside 53 bits) and rounded once to fp32, as the device's."""
    iz, iy, ix = np.meshgrid(np.arange(res[2]), np.arange(res[1]), np.arange(res[0]), indexing="ij")
    g = np.stack([ix.ravel(), iy.ravel(), iz.ravel()], 1).astype(np.float32)
    inv = (np.float32(1) / np.asarray(res, np.float32)).astype(np.float32)
    tq = (g * inv).astype(np.float32)
    diag = (np.asarray(amax, np.float32) - np.asarray(amin, np.float32)).astype(np.float32)
    p = (tq.astype(np.float64) * diag.astype(np.float64) + np.asarray(amin, np.float32).astype(np.float64)).astype(np.float32)
    return ((p - np.float32(0)) / np.float32(1)).astype(np.float32)


@pytest.mark.parametrize("cfg", N.CONFIGS, ids=IDS)
def test_selector_probes_fused_encode_in_density_kernel(probe, torch_cuda, cfg):
    """k_nerf_density (fused_levels<L, false>, a separate instantiation) through neus_testbed_sdf_on_grid at 17 x 13 x 11
    over the aabb [-0.25, 1.25]^3 (cells inside and outside the unit cube): with the selector for column c the value is
    float(fp16(din_c + fp16(bias))), bit for bit. The grid's positions are recomputed bitwise on the CPU
    (_sdf_grid_positions); the inference (EMA) weights the entry point reads are set from the parameters by
    neus_testbed_restore_state."""
    from neus2_amd._lib import NeusRestoreState, check, lib
    L, W = cfg
    e = probe(L, W)
    tb, lay = e["tb"], e["lay"]
    nm = lay["n_matrix"]
    res, amin, amax = (17, 13, 11), (-0.25,) * 3, (1.25,) * 3
    x = _sdf_grid_positions(res, amin, amax)
    din, _ = _din_reference(e, L, L, x)
    bias = _h(N.SDF_BIAS).astype(np.float64)
    st = NeusRestoreState(0, 4096, 0, 0, 0.0, 0)
    out = np.zeros(len(x), np.float32)
    for c in range(3 + 2 * L):
        p = e["params"].copy()
        p[:nm] = _selector(L, W, c)
        tb.set_params(p)
        check(lib().neus_testbed_restore_state(tb.handle, C.byref(st)))
        check(lib().neus_testbed_sdf_on_grid(tb.handle, (C.c_int32 * 3)(*res), (C.c_float * 3)(*amin), (C.c_float * 3)(*amax), C.c_void_p(out.ctypes.data)))
        want = _h(din[:, c].astype(np.float64) + bias).astype(np.float32)
        np.testing.assert_array_equal(out.view(np.uint32), want.view(np.uint32), err_msg=f"column {c}")


def test_train_hook_rejects_bad_arguments(beds, torch_cuda):
    """n not a multiple of 128, n above batch_size, n = 0 or a null operand is an error, not a launch."""
    from neus2_amd._lib import NeusError, check, lib
    t = torch_cuda
    tb = beds(1, 16)
    buf = t.zeros(16, dtype=t.float32, device="cuda")
    for n, first in ((100, buf), (BATCH + 128, buf), (0, buf), (128, None)):
        with pytest.raises(NeusError):
            check(lib().neus_debug_mlp_train(tb.handle, None, C.c_uint32(n), ptr(first), ptr(buf), ptr(buf), ptr(buf), C.c_uint32(8), ptr(buf),
                                             None, None, None, None, None))
