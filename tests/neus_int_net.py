"""Exact NeuS networks (mlp.hip's fused density + colour MLPs) and their float64 references — TEST INFRASTRUCTURE ONLY
(CPU, numpy), in the style of tests/int_net.py.

The domain. Five matrices with entries in {-1, 0, 1} (4 nonzeros per row), an all-zero hash table, positions in multiples
of 1/8 inside [0, 1], the six axis directions, dL/doutput in {-1, 0, 1} on columns 0..10 and a power-of-two
indeed_batch_size; optionally caller-given encodings (integers in [-2, 2]) and dy/dx (values in {-1, -1/2, 0, 1/2, 1}) in
place of the encode's outputs. Every fp32 accumulation of the kernels is then exact whatever its order, tile mapping or
block split, by one condition (`check_domain` asserts it for every accumulation):

    all addends are multiples of a power of two q, and  sum |addend| < 2^24 q

(every partial sum is then a multiple of q below 2^24 q, i.e. an fp32 value). Products of an fp16 operand with a weight in
{-1, 0, 1} are multiples of 2^-24 at the least; here q is 2^-3 on the density side (positions), 2^-12 in the colour layers
(the fp16 spherical-harmonics row) and 1 or 2^-3 for the deltas. Every fp16 rounding is therefore the rounding of an
exactly known number: the reference computes in float64 (exact: all values are dyadic, far inside 53 bits; the three
per-sample contractions with dy/dx in fp32, see _dot32) and rounds with np.float16 at the kernels' storage points, which are the oracle's (oracle/neus_oracle.cpp net_forward_one /
net_backward_one):

    forward   din = [h(h(x) - 0.5), enc, 0..]; H0 = h(relu(W0 din)); D1 = h(W1 H0); Gh = relu'(H0) . W1[0];
              Gi = h(W0^T Gh); grad = sum_k Gi[3 + k] dy/dx[k] + Gi[0:3] (fp32); rin = [D1, h(sh(wd)), h(x), h(grad), 0..];
              H1 = h(relu(R0 rin)); H2 = h(relu(R1 H1)); O = h(R2 H2);
              out = [O[0:3], h(D1[0] + h(bias)), h(grad), h(variance), h(wd), O[11:16]]
    backward  dO = dL[0:3]; dR2 += dO (x) H2; dH2 = h(relu'(H2) . R2^T dO); dR1 += dH2 (x) H1; dH1 = h(relu'(H1) . R1^T dH2);
              dR0 += dH1 (x) rin; dRin = h(R0^T dH1); dD1 = dRin[0:16], dD1[0] = h(dD1[0] + dL[3]);
              v = dRin[35:38] + dL[4:7] / indeed + dL[8:11] (fp32); dW1 += dD1 (x) H0; dH0 = h(relu'(H0) . W1^T dD1);
              dW0 += dH0 (x) din; dDin = h(W0^T dH0); dpos = (sum_k dDin[3 + k] dy/dx[k] + dRin[32:35]) + dDin[0:3];
              u = [h(v), h(dy/dx . v), 0..]; h1' = h(relu'(H0) . (W0 u)); dW0 += Gh (x) u; dW1[0] += h1';
              variance gradient = sum dL[7]; hand-offs d1_delta = dD1, v, genc = Gi[3:], dLdenc = dDin[3:]
(h = fp16 rounding, relu'(0) = 0). Nothing here reads the encode: with a zero table its outputs are zeros, which is what
`enc` / `dydx` default to."""
import types

import numpy as np

NNZ = 4
CONFIGS = [(1, 16), (1, 64), (2, 64), (4, 64), (8, 64), (14, 64), (16, 64)]  # NEUS_MLP_CONFIGS
SDF_BIAS = -0.1
INDEED = 8            # indeed_batch_size: v = integer + integer / 8 stays an fp16 value
SUM_BITS = 24         # fp32: integers below 2^24 are exact
BLOCK = 16384         # rows per pass of the chain (bounds the float64 temporaries at the large sizes)

# shapes of the GPU tests (tests/test_gpu_neus_exact.py); tests/test_neus_int_net.py asserts the domain of every one
FWD_SIZES = (1, 31, 32, 33, 127, 128, 129, 1000, 4097)
FWD_LARGE = 128 * 8192 + 33      # one chunk more than the inference launcher's largest grid, the last wave partial
BWD_SIZES = (128, 384, 1152)
BWD_LARGE = 128 * 2049           # one chunk more than the training kernels' largest grid
BWD_LARGE_CONFIGS = [(14, 64), (1, 16)]
DL_DENSITY_LARGE = 1.0 / 320     # share of rows with a nonzero dL/doutput outside the first and last chunk: the colour weight
                                 # gradients' sum |terms| stays below 2^24 2^-12 = 4096 (at 1 / 256 the (14, 64) case reached 4333)

SH_C = np.float32([0.28209479177387814, 0.48860251190291987, 1.0925484305920792, 0.94617469575755997, 0.31539156525251999,
                   0.54627421529603959, 0.59004358992664352, 2.8906114426405538, 0.45704579946446572, 0.3731763325901154,
                   1.4453057213202769])


def din_width(L):
    return (3 + 2 * L + 15) // 16 * 16


# One seed per config (one network at every size), found by trying seeds in order until check_domain held at every size
# the tests use; a failing domain check is answered here, never by a weaker condition.
SEEDS = {(1, 16): 1, (1, 64): 0, (2, 64): 0, (4, 64): 0, (8, 64): 0, (14, 64): 26, (16, 64): 10}


def seed_of(L, W, n=0):
    return SEEDS.get((L, W, n), SEEDS[(L, W)])


def h(a):
    """fp16 storage rounding of exactly known float64 values."""
    return np.asarray(a, np.float64).astype(np.float16).astype(np.float64)


def matrices(L, W, seed):
    """d0 [W][DIN], d1 [16][W], r0 [W][48], r1 [W][W], r2 [16][W] in {-1, 0, 1}, 4 nonzeros per row. A d0 row takes two of
    the xyz columns, one encoding column and one of all the columns from 3 on (pads included: their inputs are 0), so the
    hidden layer is alive on a zero table as well; the other matrices take any 4 columns (r0's 38..47 meet zero inputs)."""
    rng = np.random.default_rng(seed)
    DIN = din_width(L)
    d0 = np.zeros((W, DIN), np.float64)
    for row in d0:
        cols = list(rng.choice(3, 2, replace=False)) + [3 + int(rng.integers(0, 2 * L))]
        rest = [c for c in range(3, DIN) if c != cols[2]]
        cols.append(int(rng.choice(rest)))
        row[cols] = rng.choice([-1.0, 1.0], NNZ)
    mats = [d0]
    for r, k in ((16, W), (W, 48), (W, W), (16, W)):
        m = np.zeros((r, k), np.float64)
        for row in m:
            row[rng.choice(k, NNZ, replace=False)] = rng.choice([-1.0, 1.0], NNZ)
        mats.append(m)
    return mats


def sh_rows(wd):
    """The degree-4 spherical harmonics of mlp.hip sh16 in float32, operation by operation, -> fp16 values (float64)."""
    wd = np.asarray(wd, np.float32)
    one, two = np.float32(1), np.float32(2)
    x, y, z = (wd[:, k] * two - one for k in range(3))
    xy, xz, yz, x2, y2, z2 = x * y, x * z, y * z, x * x, y * y, z * z
    c = SH_C
    o = np.zeros((len(wd), 16), np.float32)
    o[:, 0] = c[0]
    o[:, 1] = -c[1] * y
    o[:, 2] = c[1] * z
    o[:, 3] = -c[1] * x
    o[:, 4] = c[2] * xy
    o[:, 5] = -c[2] * yz
    o[:, 6] = c[3] * z2 - c[4]
    o[:, 7] = -c[2] * xz
    o[:, 8] = c[5] * x2 - c[5] * y2
    o[:, 9] = c[6] * y * (np.float32(-3) * x2 + y2)
    o[:, 10] = c[7] * xy * z
    o[:, 11] = c[8] * y * (one - np.float32(5) * z2)
    o[:, 12] = c[9] * z * (np.float32(5) * z2 - np.float32(3))
    o[:, 13] = c[8] * x * (one - np.float32(5) * z2)
    o[:, 14] = c[10] * z * (x2 - y2)
    o[:, 15] = c[6] * x * (-x2 + np.float32(3) * y2)
    return o


def sh_rows_f64(wd):
    """The same polynomials in float64 (check_domain: distance of every value from an fp16 rounding boundary)."""
    wd = np.asarray(wd, np.float32).astype(np.float64)
    x, y, z = (wd[:, k] * 2 - 1 for k in range(3))
    c = SH_C.astype(np.float64)
    x2, y2, z2 = x * x, y * y, z * z
    return np.stack([np.full_like(x, c[0]), -c[1] * y, c[1] * z, -c[1] * x, c[2] * x * y, -c[2] * y * z, c[3] * z2 - c[4], -c[2] * x * z,
                     c[5] * x2 - c[5] * y2, c[6] * y * (-3 * x2 + y2), c[7] * x * y * z, c[8] * y * (1 - 5 * z2), c[9] * z * (5 * z2 - 3),
                     c[8] * x * (1 - 5 * z2), c[10] * z * (x2 - y2), c[6] * x * (-x2 + 3 * y2)], 1)


def _unit(a):
    """The largest power of two that divides every entry of a, as its exponent (None if all are zero). Every value of the
    chain is a multiple of 2^-24 (fp16 values are; so are their products with the weights, dy/dx and 1 / indeed)."""
    k = np.abs(np.asarray(a, np.float64)).ravel() * 2.0 ** 24
    ki = k.astype(np.int64)
    assert np.array_equal(ki, k), "a value of the chain is not a multiple of 2^-24"
    o = int(np.bitwise_or.reduce(ki)) if ki.size else 0
    return None if o == 0 else (o & -o).bit_length() - 1 - 24


def _dot32(a, b):
    """sum_k a[n][k] b[n][k][:] as the oracle forms its three per-sample contractions over the features or the axes (grad
    sdf, dpos, dy/dx . v): fp32 products added in index order. In the domain every order and precision gives the same,
    exact, value; on a natural table (tests/test_neus_int_net.py) this keeps the chain on the oracle's arithmetic."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    s = np.zeros((a.shape[0], b.shape[2]), np.float32)
    for k in range(a.shape[1]):
        s = s + a[:, k, None] * b[:, k, :]
    return s


class _Sums:
    """The accumulations of the chain: per name the smallest unit exponent of the addends and the largest sum |addend|."""

    def __init__(self, track=True):
        self.unit, self.sabs, self.track = {}, {}, track

    def note(self, name, a, b, sabs):
        if not self.track:
            return
        ua, ub = _unit(a), _unit(b)
        if ua is None or ub is None:
            return
        self.unit[name] = min(self.unit.get(name, 1 << 30), ua + ub)
        self.sabs[name] = sabs if name not in self.sabs else self.sabs[name] + sabs

    def rows(self, name, a, b):
        """a [n][k] @ b [k][m], one accumulation per output element, independent over the rows."""
        self.note(name, a, b, 0.0)
        if name in self.unit:
            self.sabs[name] = np.maximum(self.sabs[name], float((np.abs(a) @ np.abs(b)).max(initial=0.0)))
        return a @ b

    def batch(self, name, d, a):
        """d^T a over the samples: the weight-gradient sums, accumulated over the passes of the chain."""
        self.note(name, d, a, np.abs(d).T @ np.abs(a) if self.track else 0.0)
        return d.T @ a


def _forward(mats, L, coords, enc, dydx, variance, S, keep):
    d0, d1, r0, r1, r2 = mats
    n, DIN = len(coords), d0.shape[1]
    x, wd = coords[:, :3].astype(np.float64), coords[:, 4:7]
    din = np.zeros((n, DIN))
    din[:, :3] = h(h(x) - 0.5)
    din[:, 3:3 + 2 * L] = enc
    H0 = h(np.maximum(S.rows("d0 forward", din, d0.T), 0))
    D1 = h(S.rows("d1 forward", H0, d1.T))
    Gh = np.where(H0 > 0, d1[0], 0.0)
    Gi = keep("Gi", S.rows("W0^T Gh", Gh, d0))
    S.note("grad sdf", Gi[:, 3:3 + 2 * L], dydx, float((np.abs(Gi[:, 3:3 + 2 * L, None]) * np.abs(dydx)).sum(1).max(initial=0.0) + np.abs(Gi[:, :3]).max()))
    grad = (_dot32(Gi[:, 3:3 + 2 * L], dydx) + Gi[:, :3].astype(np.float32)).astype(np.float64)
    rin = np.zeros((n, 48))
    rin[:, :16] = D1
    rin[:, 16:32] = sh_rows(wd).astype(np.float16).astype(np.float64)
    rin[:, 32:35] = h(x)
    rin[:, 35:38] = h(grad)
    H1 = h(np.maximum(S.rows("r0 forward", rin, r0.T), 0))
    H2 = h(np.maximum(S.rows("r1 forward", H1, r1.T), 0))
    O = h(S.rows("r2 forward", H2, r2.T))
    out = O.copy()
    out[:, 3] = h(D1[:, 0] + h(SDF_BIAS))
    out[:, 4:7] = h(grad)
    out[:, 7] = h(variance)
    out[:, 8:11] = h(wd.astype(np.float64))
    return dict(din=din, H0=H0, D1=D1, Gh=Gh, Gi=Gi, rin=rin, H1=H1, H2=H2, out=(out + 0.0).astype(np.float16))


def _backward(mats, L, f, dL, dydx, indeed, S, keep):
    d0, d1, r0, r1, r2 = mats
    n = len(dL)
    dO = np.zeros((n, 16))
    dO[:, :3] = dL[:, :3]
    g = {}
    g["r2"] = S.batch("dW r2", dO, f["H2"])
    dH2 = keep("dH2", np.where(f["H2"] > 0, S.rows("r2 backward", dO, r2), 0.0))
    g["r1"] = S.batch("dW r1", dH2, f["H1"])
    dH1 = keep("dH1", np.where(f["H1"] > 0, S.rows("r1 backward", dH2, r1), 0.0))
    g["r0"] = S.batch("dW r0", dH1, f["rin"])
    dRin = keep("dRin", S.rows("r0 backward", dH1, r0))
    dD1 = dRin[:, :16].copy()
    dD1[:, 0] = keep("dD1[0]", dD1[:, 0] + dL[:, 3])
    v = dRin[:, 35:38] + dL[:, 4:7] / indeed + dL[:, 8:11]  # fp32 on the device: not rounded (u's copy is)
    keep("v", v)
    g1 = S.batch("dW d1", dD1, f["H0"])
    dH0 = keep("dH0", np.where(f["H0"] > 0, S.rows("d1 backward", dD1, d1), 0.0))
    g0 = S.batch("dW d0", dH0, f["din"])
    dDin = keep("dDin", S.rows("d0 backward", dH0, d0))
    fe = slice(3, 3 + 2 * L)
    S.note("dpos", dDin[:, fe], dydx, float(((np.abs(dDin[:, fe, None]) * np.abs(dydx)).sum(1) + np.abs(dRin[:, 32:35]) + np.abs(dDin[:, :3])).max(initial=0.0)))
    dpos = np.zeros((n, 4))
    dpos[:, :3] = (_dot32(dDin[:, fe], dydx) + dRin[:, 32:35].astype(np.float32)) + dDin[:, :3].astype(np.float32)
    u = np.zeros_like(f["din"])
    u[:, :3] = v
    S.note("dy/dx . v", dydx, v, float((np.abs(dydx) * np.abs(v[:, None, :])).sum(2).max(initial=0.0)))
    u[:, fe] = _dot32(v, dydx.transpose(0, 2, 1))
    u = keep("u", u)
    h1p = keep("h1'", np.where(f["H0"] > 0, S.rows("W0 u", u, d0.T), 0.0))
    # second order, into the same accumulators as the first
    g0 = g0 + S.batch("dW d0", f["Gh"], u)
    e0 = np.zeros((n, 16))
    e0[:, 0] = 1
    g1 = g1 + S.batch("dW d1", e0, h1p)
    g["d0"], g["d1"] = g0, g1
    S.note("variance", dL[:, 7], np.ones(1), float(np.abs(dL[:, 7]).sum()))
    v4 = np.zeros((n, 4))
    v4[:, :3] = v
    # (+ 0.0: a -0.0 of the float64 chain becomes the +0.0 the kernels' zero-initialised accumulators give)
    return g, dict(var=dL[:, 7].sum(), dpos=(dpos + 0.0).astype(np.float32), v=(v4 + 0.0).astype(np.float32), d1_delta=(dD1 + 0.0).astype(np.float16),
                   genc=(f["Gi"][:, fe] + 0.0).astype(np.float16), dLdenc=(dDin[:, fe] + 0.0).astype(np.float16))


def operands(L, n, seed, dl_density=None):
    """coords [n][7] f32 and dL/doutput [n][16] fp16; dl_density: the share of rows outside the first and the last 128
    that get a nonzero dL (None: every row)."""
    rng = np.random.default_rng(seed + 1)
    c = np.zeros((n, 7), np.float32)
    c[:, :3] = rng.integers(0, 9, (n, 3)) / 8.0
    axis, sign = rng.integers(0, 3, n), rng.integers(0, 2, n)
    c[:, 4:7] = 0.5
    c[np.arange(n), 4 + axis] = sign
    dL = np.zeros((n, 16), np.float64)
    dL[:, :11] = rng.integers(-1, 2, (n, 11))
    if dl_density is not None:
        on = rng.random(n) < dl_density
        on[:128] = on[-128:] = True
        dL[~on] = 0
    return c, dL.astype(np.float16)


def make(L, W, n, seed, enc=None, dydx=None, *, variance=0.0, indeed=INDEED, dl_density=None, rows=None, backward=True, track=True):
    """The network, its operands and the float64 references. enc [n][2L] / dydx [n][2L][3]: the caller's encodings (None:
    zeros, the zero table's). rows: compute the references for these rows only (forward only; the operands are still
    made for all n). track=False: no domain bookkeeping (operands outside the domain: the chain is then the oracle's up
    to float64 sums). The matrices come first from their own generator: one seed gives one network at every n."""
    mats = matrices(L, W, seed)
    coords, dL = operands(L, n, seed, dl_density)
    idx = np.arange(n) if rows is None else np.asarray(rows)
    assert rows is None or not backward
    S, stored = _Sums(track), {}

    def keep(name, a):
        """a is stored in fp16 and, in the domain, survives it: returns h(a), records whether it did and the largest magnitude"""
        ok, mx = stored.get(name, (True, 0.0))
        r = h(a)
        stored[name] = (ok and bool(np.array_equal(r, a)), max(mx, float(np.abs(a).max(initial=0.0))))
        return r

    outs, per, alive = [], [], []
    grads = None
    for b0 in range(0, len(idx), BLOCK):
        r = idx[b0:b0 + BLOCK]
        e = np.zeros((len(r), 2 * L)) if enc is None else np.asarray(enc, np.float64)[r]
        dy = np.zeros((len(r), 2 * L, 3)) if dydx is None else np.asarray(dydx, np.float64)[r]
        f = _forward(mats, L, coords[r], e, dy, variance, S, keep)
        outs.append(f["out"])
        alive.append([float((f[k] > 0).sum()) for k in ("H0", "H1", "H2")])
        if backward:
            # a row whose dL/doutput is all zero has every delta, v and u zero: it adds nothing to any sum and its
            # per-sample results are zeros, except genc, which is the forward's. The chain runs on the other rows.
            dl = dL[r].astype(np.float64)
            on = np.flatnonzero(dl.any(1))
            g, q = _backward(mats, L, {k: a[on] for k, a in f.items()}, dl[on], dy[on], float(indeed), S, keep)
            grads = g if grads is None else {k: grads[k] + g[k] for k in g}
            p = dict(var=q["var"], genc=(f["Gi"][:, 3:3 + 2 * L] + 0.0).astype(np.float16))
            for k in ("dpos", "v", "d1_delta", "dLdenc"):
                p[k] = np.zeros((len(r),) + q[k].shape[1:], q[k].dtype)
                p[k][on] = q[k]
            per.append(p)
    net = types.SimpleNamespace(L=L, W=W, n=n, DIN=din_width(L), mats=mats, coords=coords, dL=dL, indeed=indeed, rows=idx, variance=variance,
                                enc=enc, dydx=dydx, params=np.concatenate([m.ravel() for m in mats]).astype(np.float32),
                                out=np.concatenate(outs), alive=(np.sum(alive, 0) / (len(idx) * W)).tolist(), sums=S, stored=stored,
                                sh64=sh_rows_f64(np.unique(coords[:, 4:7], axis=0)))
    if backward:
        net.grads = [grads[k] + 0.0 for k in ("d0", "d1", "r0", "r1", "r2")]
        net.dL_dparams = np.concatenate([a.ravel() for a in net.grads])
        net.var_grad = float(sum(p["var"] for p in per))
        for k in ("dpos", "v", "d1_delta", "genc", "dLdenc"):
            setattr(net, k, np.concatenate([p[k] for p in per]))
    return net


def check_domain(net):
    """The conditions under which the device's fp16 / fp32 arithmetic is exact and the comparison means something."""
    S = net.sums
    for name, ue in S.unit.items():
        assert float(np.max(S.sabs[name])) < 2.0 ** (SUM_BITS + ue), (name, ue, float(np.max(S.sabs[name])))
    for name, (ok, mx) in net.stored.items():
        assert ok, (name, mx)
    assert all(0.2 <= a <= 0.8 for a in net.alive), net.alive
    # no spherical-harmonics value within 2^-20 (relative) of an fp16 rounding boundary: the fp16 row is the same
    # whether or not the polynomial's multiply-adds are contracted
    s = net.sh64
    lo = s.astype(np.float16).astype(np.float64)
    up = np.nextafter(lo.astype(np.float16), np.where(s >= lo, np.float16(np.inf), np.float16(-np.inf)).astype(np.float16)).astype(np.float64)
    mid = (lo + up) / 2
    assert np.all(np.abs(s - mid) > 2.0 ** -20 * np.abs(s)), "a spherical-harmonics value on an fp16 rounding boundary"
    for a in (net.coords, net.dL.astype(np.float32)):
        assert np.all(np.isfinite(a))
    assert np.array_equal(h(net.coords[:, :3]), net.coords[:, :3]) and np.array_equal(net.coords[:, :3] * 8, np.rint(net.coords[:, :3] * 8))
    if hasattr(net, "grads"):
        assert all(a.any() for a in net.grads), [bool(a.any()) for a in net.grads]
        assert net.dpos.any() and net.v.any() and net.d1_delta.any() and net.genc.any() and net.dLdenc.any()
        assert all(np.array_equal(a.astype(np.float32).astype(np.float64), a) for a in net.grads)  # fp32 values


def param_vector(net, base):
    """base (the testbed's parameters) with the five matrices replaced and the hash table zeroed (the variance stays)."""
    p = np.array(base, np.float32, copy=True)
    nm = net.params.size
    p[:nm] = net.params
    p[nm:p.size - 4] = 0
    return p


def caller_encodings(L, n, seed):
    """enc [n][2L] integers in [-2, 2] and dy/dx [n][2L][3] in {-1, -1/2, 0, 1/2, 1} for the training-kernel hook."""
    rng = np.random.default_rng(seed + 2)
    return rng.integers(-2, 3, (n, 2 * L)).astype(np.float64), rng.integers(-2, 3, (n, 2 * L, 3)) / 2.0


def paired(a, L):
    """[n][2L] -> the training buffers' [L][n] half2 layout."""
    return np.ascontiguousarray(np.asarray(a).reshape(len(a), L, 2).transpose(1, 0, 2))


def dydx_rows(d):
    """[n][2L][3] -> [6L][n] f32 (row 3 k + d)."""
    n = len(d)
    return np.ascontiguousarray(np.asarray(d, np.float32).transpose(1, 2, 0).reshape(-1, n))


def large_forward_rows(n):
    """The rows of the large forward case that get a reference: the first and the last 4096 and 4096 random ones."""
    return np.concatenate([np.arange(4096), np.arange(n - 4096, n), np.random.default_rng(n).integers(4096, n - 4096, 4096)])
