"""A CutlassMLP with the Sine activation (a SIREN) in float64 — TEST INFRASTRUCTURE ONLY (shared by test_siren_ref.py,
test_gpu_siren.py and test_gpu_tcnn_siren.py). Written beside act_ref.chain, whose `rows`, `r16` and `rel` it uses.

Sine is the one activation whose derivative is not a function of the stored post-activation value: the device keeps
c_i = cos z_i beside h_i = sin z_i. With z_i = W_{i-1} h_{i-1} the chain of act_ref.chain holds with act' = c_i and
act'' = -h_i (the output is linear):
    f_i = c_i p_i,  d_i = c_i t_i,  e_i = -h_i p_i t_i + c_i (W_i^T e_{i+1}),  dW_{i-1} = d_i f_{i-1}^T + e_i h_{i-1}^T,  q = W_0^T e_1

* `chain`: that chain layer by layer with an optional fp16 rounding at every point where the device stores fp16 (z, h, c,
  p, f, t, d, e, q). With rounding it is the *model* of the device; without, it must equal the *truth* (test_siren_ref.py).
* `truth`: torch.autograd on the unrounded float64 network behind enc(x, table): the forward, the first backward and the
  double backward of S = u . dL/dx.
* `model`: the chain behind enc, the encoding's own terms by autograd (as act_ref.bbi and act_ref.input_gradient).
* `initialize_params`: CutlassMLP::initialize_params' SIREN branch restated from pcg32: the first matrix U(+-30 / fan_in),
  every other U(+-sqrt(6 / fan_in)), fan_in the padded column count; then the grid's block U(+-1e-4).

Both `truth` and `model` return dict(y, dW1, dx1, dtable1, dW, ddo, dx, dtable): the output, the first backward's results
and backward_backward_input's."""
import numpy as np
import torch

from act_ref import r16, rel, rows  # noqa: F401  (rel: for the tests that import this module alone)


def network(mats, X0):
    """y [n, out_pad] of the encoded rows X0 [n, in_pad], unrounded and differentiable"""
    h = X0
    for Wm in mats[:-1]:
        h = torch.sin(h @ Wm.T)
    return h @ mats[-1].T


def chain(mats, X0, f0, g, rounded=False):
    """X0 = the encoded rows h_0, f0 = J_enc u the front rows, g = dL_doutput [n, out_pad]. Returns dict(y, dW1 = the first
    backward's weight gradients, dX0 = its dL/dX0, dW = backward_backward_input's, ddo, q = dS/dX0 along the forward path)."""
    r = r16 if rounded else (lambda v: v)
    with torch.no_grad():
        N = len(mats) - 1
        h, c = [X0], [None]
        for i in range(1, N + 1):
            z = r(h[i - 1] @ mats[i - 1].T)
            h.append(r(torch.sin(z)))
            c.append(r(torch.cos(z)))
        y = r(h[N] @ mats[N].T)
        f, p = [f0], [None]
        for i in range(1, N + 1):
            p.append(r(f[i - 1] @ mats[i - 1].T))
            f.append(r(c[i] * p[i]))
        ddo = r(f[N] @ mats[N].T)
        d, e = g, None  # the linear output has no curvature adjoint of its own
        dW, dW1 = [None] * (N + 1), [None] * (N + 1)
        for l in range(N, -1, -1):
            dW1[l] = d.T @ h[l]
            dW[l] = d.T @ f[l] + (0 if e is None else e.T @ h[l])
            if l > 0:
                t = r(d @ mats[l])
                below = 0 if e is None else c[l] * r(e @ mats[l])
                e = r(-h[l] * p[l] * t + below)
                d = r(c[l] * t)
        return dict(y=y, dW1=dW1, dX0=r(d @ mats[0]), dW=dW, ddo=ddo, q=r(e @ mats[0]))


def _leaves(x, table):
    xt = x.detach().clone().requires_grad_(True)
    tab = None if table is None else table.detach().clone().requires_grad_(True)
    return xt, tab


def _z(v, like):
    return torch.zeros_like(like) if v is None else v.detach()


def truth(enc, x, table, u, mats, g, pad_value):
    xt, tab = _leaves(x, table)
    ms = [m.detach().clone().requires_grad_(True) for m in mats]
    gl = g.detach().clone().requires_grad_(True)
    n = len(ms)
    y = network(ms, rows(enc(xt, tab), pad_value))
    first = torch.autograd.grad((y * gl).sum(), ms + [xt] + ([tab] if tab is not None else []), create_graph=True, allow_unused=True)
    gx = first[n]
    wrt = ms + [gl, xt] + ([tab] if tab is not None else [])
    gr = torch.autograd.grad((gx * u).sum(), wrt, allow_unused=True)
    return dict(y=y.detach(), dW1=[_z(a, m) for a, m in zip(first[:n], ms)], dx1=gx.detach(),
                dtable1=None if tab is None else _z(first[n + 1], tab),
                dW=[_z(a, m) for a, m in zip(gr[:n], ms)], ddo=_z(gr[n], gl), dx=_z(gr[n + 1], xt),
                dtable=None if tab is None else _z(gr[n + 2], tab))


def model(enc, x, table, u, mats, g, pad_value, rounded=True):
    r = r16 if rounded else (lambda v: v)
    xt, tab = _leaves(x, table)
    E = rows(enc(xt, tab), pad_value)
    cot = torch.zeros_like(E, requires_grad=True)
    Jc, = torch.autograd.grad((E * cot).sum(), xt, create_graph=True)
    f0, = torch.autograd.grad((Jc * u).sum(), cot, retain_graph=True)
    out = chain(mats, r(E.detach()), r(f0.detach()), g, rounded)
    leaves = [xt] + ([tab] if tab is not None else [])
    # the first backward: dL/dX0 through the encoding's Jacobian (float32 sums on the device: unrounded)
    Jd, = torch.autograd.grad((E * out["dX0"]).sum(), xt, create_graph=True)
    g1 = torch.autograd.grad((E * out["dX0"]).sum(), leaves, retain_graph=True, allow_unused=True)
    # the double backward: dX0 as the second-order term's cotangent, q through the first-order backward
    g2 = torch.autograd.grad((Jd * u).sum() + (E * out["q"]).sum(), leaves, allow_unused=True)
    return dict(y=out["y"], dW1=out["dW1"], dx1=_z(g1[0], xt), dtable1=None if tab is None else _z(g1[1], tab),
                dW=out["dW"], ddo=out["ddo"], dx=_z(g2[0], xt), dtable=None if tab is None else _z(g2[1], tab))


def siren_bounds(shapes):
    """the half-width of each matrix's uniform distribution, in float32 as the host computes it"""
    return [np.float32(30.0) / np.float32(k) if l == 0 else np.float32(np.sqrt(np.float32(6.0) / np.float32(k))) for l, (_, k) in enumerate(shapes)]


def initialize_params(seed, shapes, n_grid=0):
    """float32 parameters [matrices in order | grid] of initialize_params(seed) for a Sine network: pcg32{seed} draws
    next_float() * 2 scale - scale matrix by matrix; then generate_random_uniform's block for the grid: thread i of a grid
    padded to whole blocks of 128 takes draws 4 i .. 4 i + 3 for the elements i + n_threads k."""
    import oracle as O
    P = sum(r * k for r, k in shapes)
    n_pad = ((n_grid + 3) // 4 + 127) // 128 * 128
    draws = O.pcg32(seed, 1, 0, P + 4 * n_pad)
    f = ((draws >> np.uint32(9)) | np.uint32(0x3F800000)).view(np.float32) - np.float32(1)
    out, off = np.zeros(P + n_grid, np.float32), 0
    for (r, k), sc in zip(shapes, siren_bounds(shapes)):
        out[off:off + r * k] = f[off:off + r * k] * np.float32(2) * sc - sc
        off += r * k
    if n_grid:
        fg = f[P:].reshape(n_pad, 4)
        idx = np.arange(n_pad)[:, None] + n_pad * np.arange(4)[None, :]
        vals = fg * (np.float32(1e-4) - np.float32(-1e-4)) + np.float32(-1e-4)
        keep = idx < n_grid
        out[P + idx[keep]] = vals[keep]
    return out
