"""The exact double backward of a FullyFusedMLP with smooth hidden / output activations, in float64 — TEST INFRASTRUCTURE
ONLY (shared by test_act_ref.py, test_gpu_ffmlp_second_order.py and test_gpu_tcnn_second_order.py).

* `act`, `dact`, `d2act`: the activations and their first and second derivatives, the derivatives written in the stored
  post-activation value y as the kernels take them (K = 10 is tcnn's Softplus / Squareplus constant).
* `chain`: the fronts / backs / curvature-adjoint chain of backward_backward_input restated layer by layer, with an
  optional fp16 rounding at each point where the device stores fp16. With rounding it is the *model* of the device;
  without, it must equal the *truth*, torch.autograd on the unrounded float64 network (`truth`), which test_act_ref.py pins.
* `bbi`: the chain behind an encoding given as a differentiable float64 function: the encoding's own terms by autograd.

With S = u . dL/dx and g = dL_doutput the results are dW = dS/dW per matrix, dtable = dS/d(table), ddo = dS/dg
(dL_ddLdoutput) and dx = dS/dx (dL_dinput)."""
import numpy as np
import torch

K = 10.0
PAIRS = [("Softplus", "None"), ("Squareplus", "None"), ("Sigmoid", "Sigmoid"), ("Softplus", "Exponential"), ("Sigmoid", "None")]


def act(name, x):
    if name == "ReLU":
        return torch.relu(x)
    if name == "Exponential":
        return torch.exp(x)
    if name == "Sigmoid":
        return torch.sigmoid(x)
    if name == "Softplus":
        return torch.nn.functional.softplus(x, beta=K, threshold=1e9)
    if name == "Squareplus":
        return 0.5 * (x * K + torch.sqrt((x * K) ** 2 + 4.0)) / K
    assert name == "None", name
    return x


def dact(name, y):
    """act'(x) from y = act(x)"""
    if name == "ReLU":
        return (y > 0).to(y.dtype)
    if name == "Exponential":
        return y
    if name == "Sigmoid":
        return y * (1 - y)
    if name == "Softplus":
        return 1 - torch.exp(-K * y)
    if name == "Squareplus":
        t = K * y
        return t * t / (t * t + 1)
    return torch.ones_like(y)


def d2act(name, y):
    """act''(x) from y = act(x)"""
    if name == "Exponential":
        return y
    if name == "Sigmoid":
        return y * (1 - y) * (1 - 2 * y)
    if name == "Softplus":
        p = 1 - torch.exp(-K * y)
        return K * p * (1 - p)
    if name == "Squareplus":
        t = K * y
        return 2 * K * t ** 3 / (t * t + 1) ** 3
    return torch.zeros_like(y)


def r16(v):
    return v.to(torch.float16).to(torch.float64)


def network(mats, X0, act_name, out_name):
    """y [n, out_pad] of the encoded rows X0 [n, in_pad], unrounded and differentiable"""
    h = X0
    for Wm in mats[:-1]:
        h = act(act_name, h @ Wm.T)
    return act(out_name, h @ mats[-1].T)


def chain(mats, X0, f0, g, act_name, out_name, rounded=False):
    """X0 = the encoded rows h_0, f0 = J_enc u the front rows, g = dL_doutput [n, out_pad]. Returns dict(dW = [N + 1 matrices],
    ddo, q = dS/dX0 along the forward path, dX0 = the first-order dL/dX0, hidden = the pre-activations' post-activation
    values h_1 .. h_N)."""
    r = r16 if rounded else (lambda v: v)
    with torch.no_grad():
        N = len(mats) - 1
        h = [X0]
        for i in range(1, N + 1):
            h.append(r(act(act_name, r(h[i - 1] @ mats[i - 1].T))))
        y = r(act(out_name, r(h[N] @ mats[N].T)))
        f, p = [f0], [None]
        for i in range(1, N + 1):
            p.append(r(f[i - 1] @ mats[i - 1].T))
            f.append(r(r(dact(act_name, h[i])) * p[i]))
        po = r(f[N] @ mats[N].T)
        ddo = r(r(dact(out_name, y)) * po)
        e = r(d2act(out_name, y) * po * g)
        d = g if out_name == "None" else r(g * r(dact(out_name, y)))
        dW = [None] * (N + 1)
        for l in range(N, -1, -1):
            dW[l] = d.T @ f[l] + e.T @ h[l]
            if l > 0:
                t = r(d @ mats[l])
                a1 = r(dact(act_name, h[l]))
                e = r(d2act(act_name, h[l]) * p[l] * t + a1 * r(e @ mats[l]))
                d = r(a1 * t)
        return dict(dW=dW, ddo=ddo, q=r(e @ mats[0]), dX0=r(d @ mats[0]), hidden=h[1:])


def rows(e, pad_value):
    """the encoding's output as the network's input rows: padded to a multiple of 16 columns"""
    pad = -e.shape[1] % 16
    return torch.cat([e, torch.full((e.shape[0], pad), float(pad_value), dtype=e.dtype)], dim=1) if pad else e


def _leaves(x, table):
    xt = x.detach().clone().requires_grad_(True)
    tab = None if table is None else table.detach().clone().requires_grad_(True)
    return xt, tab


def truth(enc, x, table, u, mats, g, act_name, out_name, pad_value):
    """torch.autograd on the unrounded network behind enc(x, table) -> [n, w]. dict(dW, dtable, ddo, dx)."""
    xt, tab = _leaves(x, table)
    ms = [m.detach().clone().requires_grad_(True) for m in mats]
    gl = g.detach().clone().requires_grad_(True)
    y = network(ms, rows(enc(xt, tab), pad_value), act_name, out_name)
    gx, = torch.autograd.grad((y * gl).sum(), xt, create_graph=True)
    wrt = ms + [gl, xt] + ([tab] if tab is not None else [])
    gr = torch.autograd.grad((gx * u).sum(), wrt, allow_unused=True)
    z = lambda v, like: torch.zeros_like(like) if v is None else v
    n = len(ms)
    return dict(dW=[z(a, m) for a, m in zip(gr[:n], ms)], ddo=z(gr[n], gl), dx=z(gr[n + 1], xt),
                dtable=None if tab is None else z(gr[n + 2], tab))


def bbi(enc, x, table, u, mats, g, act_name, out_name, pad_value, rounded):
    """The chain behind enc: the front rows J_enc u and the encoding's part of dtable and dx by autograd on enc alone, with
    the chain's dX0 (second-order term) and q (first-order backward) as constant cotangents. dict(dW, dtable, ddo, dx,
    hidden)."""
    r = r16 if rounded else (lambda v: v)
    xt, tab = _leaves(x, table)
    E = rows(enc(xt, tab), pad_value)
    c = torch.zeros_like(E, requires_grad=True)
    Jc, = torch.autograd.grad((E * c).sum(), xt, create_graph=True)
    f0, = torch.autograd.grad((Jc * u).sum(), c, retain_graph=True)
    out = chain(mats, r(E.detach()), r(f0.detach()), g, act_name, out_name, rounded)
    Jd, = torch.autograd.grad((E * out["dX0"]).sum(), xt, create_graph=True)
    S = (Jd * u).sum() + (E * out["q"]).sum()
    gr = torch.autograd.grad(S, [xt] + ([tab] if tab is not None else []), allow_unused=True)
    z = lambda v, like: torch.zeros_like(like) if v is None else v
    return dict(dW=out["dW"], ddo=out["ddo"], dx=z(gr[0], xt), dtable=None if tab is None else z(gr[1], tab), hidden=out["hidden"])


def input_gradient(enc, x, table, mats, g, act_name, out_name, pad_value, rounded):
    """dL/dx of the first backward: the chain's dL/dX0 through the encoding's Jacobian (a float32 sum on the device: unrounded)"""
    r = r16 if rounded else (lambda v: v)
    xt, tab = _leaves(x, table)
    E = rows(enc(xt, tab), pad_value)
    out = chain(mats, r(E.detach()), torch.zeros_like(E), g, act_name, out_name, rounded)
    return torch.autograd.grad((E * out["dX0"]).sum(), xt)[0]


def rel(x, y):
    x, y = np.asarray(x, np.float64).ravel(), np.asarray(y, np.float64).ravel()
    return np.linalg.norm(x - y) / max(np.linalg.norm(y), 1e-30)
