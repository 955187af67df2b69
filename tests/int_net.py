"""Exact-integer FullyFusedMLP networks and their int64 references — TEST INFRASTRUCTURE ONLY (CPU, numpy).

A ReLU network with a linear output, weights in {-1, 0, 1} (4 nonzeros per row), inputs in [-2, 2] and dL_doutput /
dL_ddLdinput in {-1, 0, 1}: every value the kernels store in fp16 is an integer of magnitude <= 2048 and every fp32 sum an
integer below 2^24, so each result is exact whatever the summation order, block split or tile mapping, and must equal the
int64 reference below bit for bit. The caller asserts the domain figures (`check_domain`) before it looks at a device
result; if a seed breaks one, the seed changes, not the condition.

The chains are ffmlp.hip's: a_0 = [x | ones] (k_ff_input), z_l = a_l W_l^T, a_{l+1} = relu(z_l), out = z_N;
backward D_N = dL, dW_l = D_l^T a_l, D_{l-1} = relu'(a_l) (D_l W_l), dL_dinput = (D_0 W_0)[:, :n_in];
backward_backward_input (ff_bbi_chain): fronts f_0 = [u | zeros], f_i = relu'(a_i) (f_{i-1} W_{i-1}^T),
dL_ddLdoutput = f_N W_N^T; backs b_N = dL, dW_l = b_l^T f_l, b_{l-1} = relu'(a_l) (b_l W_l). relu'(0) = 0 on both sides."""
import types

import numpy as np

STORED_MAX = 2048   # integers up to here are exact in fp16
SUM_MAX = 1 << 24   # integer sums below this are exact in fp32
NNZ = 4

# n_in, n_out, W, N, n, batch capacity, seed (test_gpu_ffmlp_exact.py; the CPU test asserts the domain of every one)
SHAPES = [
    (3, 16, 16, 1, 128, 128, 0),
    (8, 5, 32, 2, 1024, 2048, 1),
    (8, 5, 32, 2, 1152, 2048, 1),
    (20, 3, 64, 2, 2176, 4096, 2),
    (40, 4, 128, 3, 1152, 1152, 3),
    (128, 128, 128, 1, 256, 256, 4),
    (3, 16, 16, 1, 131200, 131200, 5),
]


def shapes(n_in, n_out, W, N):
    in_pad, out_pad = (n_in + 15) // 16 * 16, (n_out + 15) // 16 * 16
    return [(W, in_pad)] + [(W, W)] * (N - 1) + [(out_pad, W)], in_pad, out_pad


def _gemm(a, b):
    """Exact integer a @ b: float64 BLAS (every product and partial sum stays far below 2^53), back to int64."""
    return np.rint(a.astype(np.float64) @ b.astype(np.float64)).astype(np.int64)


def make(n_in, n_out, W, N, n, seed):
    """The network (matrices first from the generator: the same seed gives the same parameters at every n), its
    operands and the int64 references."""
    rng = np.random.default_rng(seed)
    shp, in_pad, out_pad = shapes(n_in, n_out, W, N)
    mats = []
    for r, k in shp:
        m = np.zeros((r, k), np.int64)
        for row in m:
            row[rng.choice(k, NNZ, replace=False)] = rng.choice([-1, 1], NNZ)
        mats.append(m)
    x = rng.integers(-2, 3, (n, n_in))
    dL = rng.integers(-1, 2, (n, out_pad))
    u = rng.integers(-1, 2, (n, n_in))

    stored, terms, alive = 0, 0, []

    def keep(v):
        nonlocal stored
        stored = max(stored, int(np.abs(v).max()))
        return v

    def wgrad(d, a):
        nonlocal terms
        terms = max(terms, int(_gemm(np.abs(d).T, np.abs(a)).max()))
        return _gemm(d.T, a)

    # forward
    acts = [keep(np.concatenate([x, np.ones((n, in_pad - n_in), np.int64)], 1))]
    for l in range(N):
        z = keep(_gemm(acts[l], mats[l].T))
        alive.append(float((z > 0).mean()))
        acts.append(np.maximum(z, 0))
    out = keep(_gemm(acts[N], mats[N].T))
    # backward
    g, d = [None] * (N + 1), keep(dL)
    for l in range(N, -1, -1):
        g[l] = wgrad(d, acts[l])
        d = keep(_gemm(d, mats[l]))
        if l > 0:
            d = d * (acts[l] > 0)
    dinput = d[:, :n_in]
    # backward_backward_input
    fronts = [keep(np.concatenate([u, np.zeros((n, in_pad - n_in), np.int64)], 1))]
    for i in range(1, N + 1):
        fronts.append(keep(_gemm(fronts[i - 1], mats[i - 1].T)) * (acts[i] > 0))
    ddo = keep(_gemm(fronts[N], mats[N].T))
    g2, b = [None] * (N + 1), dL
    for l in range(N, -1, -1):
        g2[l] = wgrad(b, fronts[l])
        if l > 0:
            b = keep(_gemm(b, mats[l])) * (acts[l] > 0)
    return types.SimpleNamespace(
        n_in=n_in, n_out=n_out, W=W, N=N, n=n, in_pad=in_pad, out_pad=out_pad, shapes=shp, mats=mats,
        params=np.concatenate([m.ravel() for m in mats]).astype(np.float16),
        x=x.astype(np.float32), dL=dL.astype(np.float16), u=u.astype(np.float32),
        out=out, dL_dparams=np.concatenate([a.ravel() for a in g]), dL_dinput=dinput,
        bbi_dL_dparams=np.concatenate([a.ravel() for a in g2]), bbi_dL_ddLdoutput=ddo,
        grads=g, bbi_grads=g2, max_stored=stored, max_terms=terms, alive=alive)


def check_domain(net):
    """The conditions under which the device's fp16 / fp32 arithmetic is exact and the comparison means something."""
    assert net.max_stored <= STORED_MAX, net.max_stored
    assert net.max_terms < SUM_MAX, net.max_terms
    assert all(0.2 <= a <= 0.8 for a in net.alive), net.alive
    assert all(a.any() for a in net.grads + net.bbi_grads)
    for a in (net.params, net.x, net.dL, net.u):  # the operands survive their storage types
        assert np.array_equal(a.astype(np.int64).astype(a.dtype), a)
