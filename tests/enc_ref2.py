"""Float64 torch references of the TriangleWave, OneBlob and OneBlobFrequency / NRC encodings, written from their
definitions and differentiable with autograd to second order — TEST INFRASTRUCTURE ONLY (shared by test_enc_ref2.py and
the test_gpu_*2 files). Everything else falls through to tests/enc_ref.py.

  TriangleWave(F): val = x 2^(k-1) + k / 4, f = val - floor(val), feature d F + k = 4 |f - 1/2| - 1. The derivative is
                   -2^(k+1) where floor(2 val) is even and +2^(k+1) where it is odd, kinks included: the sign and the
                   floor are detached, so autograd yields exactly that; the second derivative is 0.
  OneBlob(B):      C(u) = clamp(15/16 u (1 - 2/3 u^2 + 1/5 u^4) + 1/2, 0, 1), u_ks = (k + s B) - B x,
                   feature d B + k = sum over s in {0, -1, 1} of C(u_ks + 1) - C(u_ks)  (the wrap-around form)
                   dy_k/dx = B sum_s q(u_ks) - q(u_ks + 1),       q(u)  = 15/16 max(1 - u^2, 0)^2
                   d2y_k/dx2 = B^2 sum_s q'(u_ks + 1) - q'(u_ks), q'(u) = -15/4 u (1 - u^2) for |u| < 1, else 0
  NRC(F, B):       Composite [TriangleWave(F) over 3 dims | OneBlob(B) over 5 dims | Identity over the rest]
"""
import numpy as np
import torch

import enc_ref as E


def triangle_wave(x, F):
    """x [n, D] float64 -> [n, D F]"""
    k = torch.arange(F, dtype=torch.float64)
    t = x[:, :, None] * 2.0 ** (k - 1.0)
    val = (t - torch.floor(t).detach()) + k / 4.0  # x 2^(k-1) reduced modulo 1 first: exact for float32-valued x
    f = val - torch.floor(val).detach()
    sign = torch.where(torch.floor(2.0 * f) % 2 == 0, -1.0, 1.0).detach()  # the parity of floor(2 val)
    return (4.0 * sign * (f - 0.5) - 1.0).reshape(x.shape[0], -1)


def blob_cdf(u):
    u2 = u * u
    return torch.clamp(15.0 / 16.0 * u * (1.0 - 2.0 / 3.0 * u2 + 0.2 * u2 * u2) + 0.5, 0.0, 1.0)


def blob_q(u):
    return 15.0 / 16.0 * torch.clamp(1.0 - u * u, min=0.0) ** 2


def blob_dq(u):
    return torch.where(u.abs() < 1.0, -3.75 * u * (1.0 - u * u), torch.zeros_like(u))


def _blob_u(x, B):
    """u_ks [3, n, D, B] for s = 0, -1, 1"""
    k = torch.arange(B, dtype=torch.float64)
    return torch.stack([(k + s * B) - B * x[:, :, None] for s in (0, -1, 1)])


def oneblob(x, B):
    """x [n, D] float64 -> [n, D B]"""
    u = _blob_u(x, B)
    return (blob_cdf(u + 1.0) - blob_cdf(u)).sum(dim=0).reshape(x.shape[0], -1)


def oneblob_dx(x, B):
    """the closed form of d(feature d B + k) / dx_d, [n, D B]"""
    u = _blob_u(x, B)
    return (B * (blob_q(u) - blob_q(u + 1.0))).sum(dim=0).reshape(x.shape[0], -1)


def oneblob_d2x(x, B):
    """the closed form of d2(feature d B + k) / dx_d^2, [n, D B]"""
    u = _blob_u(x, B)
    return (B * B * (blob_dq(u + 1.0) - blob_dq(u))).sum(dim=0).reshape(x.shape[0], -1)


def nrc_nested(n_input_dims, F=12, B=4):
    """the Composite that OneBlobFrequency / NRC stands for; no Identity segment at exactly 8 dims"""
    assert n_input_dims >= 8
    nested = [{"otype": "TriangleWave", "n_dims_to_encode": 3, "n_frequencies": F}, {"otype": "OneBlob", "n_dims_to_encode": 5, "n_bins": B}]
    return nested + ([{"otype": "Identity"}] if n_input_dims > 8 else [])


def nrc(x, F=12, B=4):
    parts = [triangle_wave(x[:, :3], F), oneblob(x[:, 3:8], B)]
    return torch.cat(parts + ([x[:, 8:]] if x.shape[1] > 8 else []), dim=1)


def encode_one(x, cfg):
    ot = cfg["otype"]
    if ot == "TriangleWave":
        return triangle_wave(x, cfg.get("n_frequencies", 12))
    if ot == "OneBlob":
        return oneblob(x, cfg.get("n_bins", 16))
    return E.encode_one(x, cfg)


def encode(x, cfg):
    """any accepted encoding config on x [n, n_input_dims]"""
    ot = cfg["otype"]
    if ot in ("OneBlobFrequency", "NRC"):
        return nrc(x, cfg.get("n_frequencies", 12), cfg.get("n_bins", 4))
    if ot == "Composite":
        outs, d0 = [], 0
        for c in cfg["nested"]:
            k = c.get("n_dims_to_encode", x.shape[1] - d0)
            outs.append(encode_one(x[:, d0:d0 + k], c))
            d0 += k
        assert d0 == x.shape[1]
        return torch.cat(outs, dim=1)
    if ot in ("TriangleWave", "OneBlob"):
        return encode_one(x, cfg)
    return E.encode(x, cfg)


def segments(cfg, n_input_dims):
    """[(otype, first column, width, param)] of the accepted config: which columns are OneBlob's, and their n_bins"""
    ot = cfg["otype"]
    if ot in ("OneBlobFrequency", "NRC"):
        nested = nrc_nested(n_input_dims, cfg.get("n_frequencies", 12), cfg.get("n_bins", 4))
    elif ot == "Composite":
        nested = cfg["nested"]
    else:
        nested = [cfg]
    out, d0, c0 = [], 0, 0
    for c in nested:
        dims = c.get("n_dims_to_encode", n_input_dims - d0)
        o = c["otype"]
        if o == "OneBlob":
            param, w = c.get("n_bins", 16), dims * c.get("n_bins", 16)
        elif o == "TriangleWave":
            param, w = c.get("n_frequencies", 12), dims * c.get("n_frequencies", 12)
        elif o == "Frequency":
            param, w = c.get("n_frequencies", 12), 2 * dims * c.get("n_frequencies", 12)
        elif o == "SphericalHarmonics":
            param, w = c.get("degree", 4), c.get("degree", 4) ** 2
        else:
            param, w = 0, dims
        out.append((o, c0, w, param))
        d0, c0 = d0 + dims, c0 + w
    assert d0 == n_input_dims
    return out


def derivative_scale(cfg, n_input_dims, J):
    """c_k [n, w, D] of the dL_dinput bars: max(1, |J_kd|), and n_bins for a OneBlob column (its derivative is n_bins times
    a difference of two O(1) terms, so its error scales with n_bins even where J_kd cancels to 0)"""
    c = np.maximum(1.0, np.abs(J))
    for ot, c0, w, param in segments(cfg, n_input_dims):
        if ot == "OneBlob":
            c[:, c0:c0 + w, :] = float(param)
    return c


def jacobian(x32, cfg):
    """(y [n, w], J [n, w, D]) in float64 numpy for float32 inputs, as enc_ref.jacobian"""
    xt = torch.tensor(np.asarray(x32, np.float64), requires_grad=True)
    y = encode(xt, cfg)
    cols = []
    for k in range(y.shape[1]):
        g, = torch.autograd.grad(y[:, k].sum(), xt, retain_graph=True, allow_unused=True)
        cols.append(torch.zeros_like(xt) if g is None else g)
    return y.detach().numpy(), torch.stack(cols, dim=1).numpy()
