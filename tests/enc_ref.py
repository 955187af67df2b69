"""Float64 torch references of the parameter-free encodings (Identity, Frequency, SphericalHarmonics, Composite), written
from their definitions and differentiable with autograd to any order — TEST INFRASTRUCTURE ONLY (shared by
test_enc_ref.py and the test_gpu_*enc* files).

  Frequency(F):          feature d 2F + 2k + j = sin(pi 2^k x_d + j pi / 2), the argument reduced modulo 2 exactly first
  SphericalHarmonics(G): (x, y, z) = 2 in - 1, not normalised; feature l^2 + l + m = c_m K_l^|m| T_l^|m|(z) H_m(x, y) with
                         K_l^a = sqrt((2l + 1) / (4 pi) (l - a)! / (l + a)!), T_l^a = d^a P_l / dz^a, H_0 = 1,
                         H_m = Re (x + iy)^m (m > 0) or Im (x + iy)^|m| (m < 0), c_0 = 1, c_m = (-1)^m sqrt 2
  Identity:              x scale + offset
  Composite:             nested encodings over consecutive input dims, outputs concatenated
"""
import math

import numpy as np
import torch
from numpy.polynomial import legendre, polynomial


def frequency(x, F):
    """x [n, D] float64 -> [n, 2 D F]"""
    t = x[:, :, None] * (2.0 ** torch.arange(F, dtype=torch.float64))
    r = t - 2.0 * torch.round(t / 2.0).detach()  # exact for float32-valued x; in [-1, 1]
    a = math.pi * r
    return torch.stack([torch.sin(a), torch.cos(a)], dim=-1).reshape(x.shape[0], -1)


def _legendre_derivative(l, a):
    """monomial coefficients (ascending) of d^a P_l / dz^a"""
    c = legendre.leg2poly([0.0] * l + [1.0])
    return polynomial.polyder(c, a) if a else c


def sh(x, G):
    """x [n, 3] float64 -> [n, G^2]"""
    X, Y, Z = 2.0 * x[:, 0] - 1.0, 2.0 * x[:, 1] - 1.0, 2.0 * x[:, 2] - 1.0
    re, im = [torch.ones_like(X)], [torch.zeros_like(X)]
    for _ in range(1, G):
        re, im = re + [X * re[-1] - Y * im[-1]], im + [X * im[-1] + Y * re[-1]]
    out = []
    for l in range(G):
        for m in range(-l, l + 1):
            a = abs(m)
            K = math.sqrt((2 * l + 1) / (4.0 * math.pi) * math.factorial(l - a) / math.factorial(l + a))
            c = 1.0 if m == 0 else (-1.0) ** m * math.sqrt(2.0)
            T = torch.zeros_like(Z)
            for coef in _legendre_derivative(l, a)[::-1]:  # Horner
                T = T * Z + float(coef)
            H = re[a] if m >= 0 else im[a]
            out.append(c * K * T * H)
    return torch.stack(out, dim=1)


def identity(x, scale=1.0, offset=0.0):
    return x * scale + offset


def encode_one(x, cfg):
    ot = cfg["otype"]
    if ot == "Frequency":
        return frequency(x, cfg.get("n_frequencies", 12))
    if ot == "SphericalHarmonics":
        return sh(x, cfg.get("degree", 4))
    if ot == "Identity":
        return identity(x, cfg.get("scale", 1.0), cfg.get("offset", 0.0))
    raise ValueError(ot)


def composite(x, nested):
    outs, d0 = [], 0
    for i, cfg in enumerate(nested):
        k = cfg.get("n_dims_to_encode", x.shape[1] - d0)
        outs.append(encode_one(x[:, d0:d0 + k], cfg))
        d0 += k
    assert d0 == x.shape[1]
    return torch.cat(outs, dim=1)


def encode(x, cfg):
    """any accepted encoding config on x [n, n_input_dims]"""
    return composite(x, cfg["nested"]) if cfg["otype"] == "Composite" else encode_one(x, cfg)


def pad_ones(e):
    """padded to a multiple of 16 columns with ones, as the input rows of the FullyFusedMLP"""
    pad = -e.shape[1] % 16
    return torch.cat([e, torch.ones(e.shape[0], pad, dtype=e.dtype)], dim=1) if pad else e


def jacobian(x32, cfg):
    """(y [n, w], J [n, w, D]) in float64 numpy for float32 inputs: the samples are independent, so column k of the
    Jacobian is the gradient of sum_n y[n, k]."""
    xt = torch.tensor(np.asarray(x32, np.float64), requires_grad=True)
    y = encode(xt, cfg)
    cols = []
    for k in range(y.shape[1]):
        g, = torch.autograd.grad(y[:, k].sum(), xt, retain_graph=True, allow_unused=True)
        cols.append(torch.zeros_like(xt) if g is None else g)
    return y.detach().numpy(), torch.stack(cols, dim=1).numpy()


def mlp(h, mats, r16, ambiguous_below=1e-4):
    """The FullyFusedMLP as tests/bbi_ref.py models it: an fp16 rounding (r16) at every point where the device stores fp16,
    hidden ReLU, linear output. h [n, in_pad] (already rounded). Returns (out [n, out_pad], ambiguous [n] bool: a hidden
    pre-activation within ambiguous_below of 0)."""
    amb = np.zeros(h.shape[0], bool)
    for li, W in enumerate(mats):
        z = r16(h @ W.T)
        if li < len(mats) - 1:
            amb |= (np.abs(z.detach().numpy()) < ambiguous_below).any(axis=1)
            h = r16(torch.relu(z))
    return z, amb


def mlp_shapes(in_pad, W, n_hidden, out_pad=16):
    return [(W, in_pad)] + [(W, W)] * (n_hidden - 1) + [(out_pad, W)]


def mlp_params(rng, shapes):
    """fp16 parameter vector (matrices in order) with O(1) activations"""
    return np.concatenate([rng.normal(0, 1.2 / np.sqrt(k), (r, k)).ravel() for r, k in shapes]).astype(np.float16)


def mlp_mats(ph, shapes):
    pd, mats, o = torch.tensor(ph.astype(np.float64)), [], 0
    for r, k in shapes:
        mats.append(pd[o:o + r * k].reshape(r, k).clone().requires_grad_(True))
        o += r * k
    return mats
