"""The float64 reference chain of tests/neus_int_net.py, pinned without a device: inside its exact domain for every shape
tests/test_gpu_neus_exact.py runs (generated at full size), bitwise equal to the oracle on the zero table for all seven
network configs (in the domain the oracle's fp32 sums are exact too), and, for the terms a zero table leaves dead (the
encodings in din, the G . dy/dx normal, the dy/dx . v entries of u, the grid part of dpos), within the oracle's own
summation-order spread on a natural +-0.1 table."""
import numpy as np
import pytest

import neus_int_net as N

IDS = [f"L{L}_W{W}" for L, W in N.CONFIGS]
VARIANCE = 0.3


def _oracle(L, W):
    import oracle as O
    cfg = O.make_cfg(n_levels=L, width=W)
    return O, cfg, O.layout(cfg)


def _params(lay, net, grid=None):
    p = np.zeros(lay["n_params"], np.float32)
    assert lay["n_matrix"] == net.params.size and lay["grid_off"] == lay["n_matrix"]
    p[:lay["n_matrix"]] = net.params
    if grid is not None:
        p[lay["grid_off"]:lay["var_off"]] = grid
    p[lay["var_off"]] = VARIANCE
    return p


@pytest.mark.parametrize("cfg", N.CONFIGS, ids=IDS)
def test_domain_backward_shapes(cfg):
    """Zero encodings (the production path's zero table) and the hook's caller encodings, at every backward size."""
    L, W = cfg
    for n in N.BWD_SIZES:
        seed = N.seed_of(L, W, n)
        N.check_domain(N.make(L, W, n, seed))
        enc, dydx = N.caller_encodings(L, n, seed)
        net = N.make(L, W, n, seed, enc, dydx)
        worst = max(float(np.max(net.sums.sabs[k])) / 2.0 ** (N.SUM_BITS + u) for k, u in net.sums.unit.items())
        print(f"L{L} W{W} n={n}: alive {net.alive}, largest sum|terms| / (2^24 q) = {worst:.3f}")
        N.check_domain(net)


@pytest.mark.parametrize("cfg", N.CONFIGS, ids=IDS)
def test_domain_forward_shapes(cfg):
    L, W = cfg
    for n in N.FWD_SIZES:
        N.check_domain(N.make(L, W, n, N.seed_of(L, W, n), backward=False))


@pytest.mark.parametrize("cfg", N.BWD_LARGE_CONFIGS, ids=lambda c: f"L{c[0]}_W{c[1]}")
def test_domain_persistent_loop_shape(cfg):
    """n = 128 * 2049: dL/doutput on every row of the first and last chunk, on about 1 row in 320 elsewhere."""
    L, W = cfg
    n, seed = N.BWD_LARGE, N.seed_of(L, W, N.BWD_LARGE)
    enc, dydx = N.caller_encodings(L, n, seed)
    net = N.make(L, W, n, seed, enc, dydx, dl_density=N.DL_DENSITY_LARGE)
    on = net.dL.astype(np.float32).any(1)
    assert on[:128].all() and on[-128:].all() and 0.5 * N.DL_DENSITY_LARGE < on[128:-128].mean() < 2 * N.DL_DENSITY_LARGE
    N.check_domain(net)


def test_domain_large_forward_shape():
    n = N.FWD_LARGE
    rows = N.large_forward_rows(n)
    assert len(rows) == 3 * 4096 and rows[0] == 0 and rows[8191] == n - 1
    N.check_domain(N.make(14, 64, n, N.seed_of(14, 64, n), rows=rows, backward=False))


@pytest.mark.parametrize("cfg", N.CONFIGS, ids=IDS)
def test_zero_grid_chain_equals_oracle_bitwise(cfg):
    """Zero table, n = 384: output rows, the five matrix blocks, the variance gradient and dpos, bit for bit."""
    L, W = cfg
    O, ocfg, lay = _oracle(L, W)
    n = 384
    net = N.make(L, W, n, N.seed_of(L, W, n), variance=VARIANCE)
    N.check_domain(net)
    p = _params(lay, net)
    out = O.network_forward(ocfg, p, net.coords, L)
    np.testing.assert_array_equal(out, net.out.view(np.uint16))
    g, dpos = O.network_backward_pos(ocfg, p, net.coords, L, net.dL.view(np.uint16), net.indeed)
    off = 0
    for name, ref in zip(("d0", "d1", "r0", "r1", "r2"), net.grads):
        got = g[off:off + ref.size].reshape(ref.shape)
        np.testing.assert_array_equal(got.view(np.uint32), ref.astype(np.float32).view(np.uint32), err_msg=name)
        off += ref.size
    assert off == lay["n_matrix"]
    np.testing.assert_array_equal(g[lay["var_off"]:lay["var_off"] + 4], np.float32([net.var_grad, 0, 0, 0]))
    np.testing.assert_array_equal(dpos.view(np.uint32), net.dpos.view(np.uint32))


def _blocks(lay, L, W, g, dpos):
    shapes = [(W, N.din_width(L)), (16, W), (W, 48), (W, W), (16, W)]
    out, off = {}, 0
    for name, (r, k) in zip(("d0", "d1", "r0", "r1", "r2"), shapes):
        out[name] = g[off:off + r * k].astype(np.float64)
        off += r * k
    out["dpos"] = dpos[:, :3].astype(np.float64).ravel()
    return out


def _rel(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


@pytest.mark.parametrize("cfg", N.CONFIGS, ids=IDS)
def test_natural_grid_chain_within_oracle_sum_order_spread(cfg):
    """A random +-0.1 table, enc / dy/dx from the oracle's encode fed to the chain with the same +-1 matrices, n = 384:
    every block's rel-L2 (five matrix blocks and dpos) against O.network_backward_pos at most 10 x the floor, the largest
    rel-L2 over the blocks between the oracle's default run and its own reversed / pairwise / blocked summation orders.
    Measured: the floor is 0 for L = 1 (a sum of two features has one order; the 4-term layer sums of these matrices did
    not move either) and 5.0e-8 (L = 2), 6.1e-8 (4), 8.3e-8 (8), 9.1e-8 (14), 9.8e-8 (16), all of it in dpos; the chain's
    distance is 0 in every block of every config. It was 2e-8 .. 5e-8 in dpos and, through single fp16 flips of
    h(dy/dx . v), up to 9e-6 in dW_d0 / dW_d1 while the chain summed its three per-sample dy/dx contractions in float64:
    with +-1 matrices those are the only sums of more than four terms, and the oracle's order switch does not reach
    dy/dx . v, so the chain forms them as the oracle does (neus_int_net._dot32) - the same value inside the exact domain."""
    L, W = cfg
    O, ocfg, lay = _oracle(L, W)
    n = 384
    seed = N.seed_of(L, W, n)
    grid = np.random.default_rng(seed + 3).uniform(-0.1, 0.1, lay["n_grid_params"]).astype(np.float32)
    zero = N.make(L, W, n, seed, backward=False)
    p = _params(lay, zero, grid)
    enc, dydx = O.grid_forward(ocfg, p, zero.coords[:, :3], L)
    net = N.make(L, W, n, seed, enc, dydx, variance=VARIANCE, track=False)
    mine = _blocks(lay, L, W, net.dL_dparams.astype(np.float32), net.dpos)
    dl = net.dL.view(np.uint16)
    try:
        ref = _blocks(lay, L, W, *O.network_backward_pos(ocfg, p, net.coords, L, dl, net.indeed))
        floor = 0.0
        for order in (1, 2, 3):
            O.set_sum_order(order)
            alt = _blocks(lay, L, W, *O.network_backward_pos(ocfg, p, net.coords, L, dl, net.indeed))
            floor = max(floor, max(_rel(alt[k], ref[k]) for k in ref))
    finally:
        O.set_sum_order(0)
    dist = {k: _rel(mine[k], ref[k]) for k in ref}
    print(f"L{L} W{W}: floor {floor:.3e}, chain {', '.join(f'{k} {v:.3e}' for k, v in dist.items())}")
    assert all(np.linalg.norm(ref[k]) > 0 for k in ref)
    for k, v in dist.items():
        assert v <= 10 * floor, (k, v, floor)
