"""Exact-integer cases for the general grid's "gradient_scatter": "binned", and a numpy restatement of its arithmetic
contract - TEST INFRASTRUCTURE ONLY.

Contract (neus2_amd/csrc/grid_nd_scatter.hip): each contribution c = weight * dL_dy_f is an fp32 product (weight w_c, the
corner's interpolation weight, for backward; a_c, its directional derivative along u, for backward_backward_input); each
becomes int64 fixed point on its own, rint(c 2^32); an entry's contributions are summed as integers; the sum becomes fp32
once, round to nearest. A contribution that is not finite, or of magnitude >= 2^31, makes its parameter NaN.

The cases: every level has the same power-of-two scale (per_level_scale 1, base_resolution 2^m + 1), x = (k + 1/4) / scale
with integer k, so every interpolation fraction is exactly 3/4; dL_dy are integers in [-8, 8] and u integers in [-2, 2].
Every contribution is then a multiple of 2^-q with few bits, every per-entry sum of magnitudes stays below 2^24 units, and
any fp32 evaluation in any order is exact - as is the 2^-32 fixed point. The first 64 rows are identical (a whole wave
hits one entry), and the 32- and 64-entry hashed tables collide heavily."""
from __future__ import annotations

import functools

import numpy as np

import grid_nd_ref as G

N = 384
SEED = 5
# name -> ((D, F, type, interpolation, L, log2_hashmap_size, base_resolution, per_level_scale), q)
X_CASES = {
    "X1": ((2, 1, "Dense", "Linear", 2, None, 9, 1.0), 4),
    "X2": ((3, 8, "Hash", "Linear", 3, 5, 9, 1.0), 6),
    "X3": ((2, 4, "Hash", "Smoothstep", 2, 5, 9, 1.0), 10),
    "X4": ((4, 2, "Hash", "Linear", 2, 6, 5, 1.0), 8),
}


def x_config(case, **extra):
    (D, F, ty, ip, L, log2, base, pls), _ = X_CASES[case]
    cfg = {"otype": "Grid", "type": ty, "n_levels": L, "n_features_per_level": F, "base_resolution": base, "per_level_scale": pls,
           "interpolation": ip}
    if log2 is not None:
        cfg["log2_hashmap_size"] = log2
    cfg.update(extra)
    return cfg


def x_tables(case):
    (D, F, ty, ip, L, log2, base, pls), _ = X_CASES[case]
    return G.level_tables(D, L, log2 if log2 is not None else 19, base, pls, ty)


@functools.lru_cache(maxsize=None)
def x_inputs(case):
    """pos [N, D] fp32, table [entries, F] fp16 (integers), dly [N, F L] fp16 (integers), u [N, D] fp32 (integers); read-only"""
    (D, F, ty, ip, L, log2, base, pls), _ = X_CASES[case]
    off, res = x_tables(case)
    scale = res[0] - 1
    assert all(r == res[0] for r in res) and scale & (scale - 1) == 0
    rng = np.random.default_rng(SEED)
    k = rng.integers(0, scale, (N, D))
    k[:64] = k[0]
    pos = ((k + 0.25) / scale).astype(np.float32)
    table = rng.integers(-4, 5, (off[-1], F)).astype(np.float16)
    dly = rng.integers(-8, 9, (N, F * L)).astype(np.float16)
    dly[:64] = dly[0]
    u = rng.integers(-2, 3, (N, D)).astype(np.float32)
    u[:64] = u[0]
    for a in (pos, table, dly, u):
        a.setflags(write=False)
    return pos, table, dly, u


def _fma(a, b, c):
    """fp32 fused multiply-add (the float64 product of two fp32 values is exact)"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def contributions(pos, dly, u, off, res, F, grid_type, interpolation, second, valid_level=None):
    """The fp32 contributions of the contract, in the kernels' operation order: (parameter index [M], value [M] fp32)"""
    import torch
    pos, dly = np.asarray(pos, np.float32), np.asarray(dly, np.float32)
    n, D = pos.shape
    one = np.float32(1)
    idx, val = [], []
    for l in range(len(res)):
        if valid_level is not None and l > valid_level:
            continue
        scale = np.float32(res[l] - 1)
        p = _fma(pos, np.full_like(pos, scale), np.full_like(pos, 0.5))
        fl = np.floor(p)
        t = p - fl
        if interpolation == "Smoothstep":
            w1 = t * t * (np.float32(3) - np.float32(2) * t)
            dw = np.float32(6) * t * (one - t)
        else:
            w1, dw = t, np.ones_like(t)
        g = fl.astype(np.int64)
        for c in range(1 << D):
            bits = [(c >> d) & 1 for d in range(D)]
            side = [w1[:, d] if bits[d] else one - w1[:, d] for d in range(D)]
            if not second:
                w = np.ones(n, np.float32)
                for d in range(D):
                    w = w * side[d]
            else:
                w = np.zeros(n, np.float32)
                for j in range(D):
                    dwc = np.full(n, 1 if bits[j] else -1, np.float32)
                    for d in range(D):
                        if d != j:
                            dwc = dwc * side[d]
                    w = _fma(np.asarray(u, np.float32)[:, j] * (scale * dw[:, j]), dwc, w)
            e = G.index(off[l + 1] - off[l], res[l], torch.from_numpy(g + np.array(bits)), grid_type).numpy() + off[l]
            for f in range(F):
                idx.append(e * F + f)
                val.append(w * dly[:, l * F + f])
    return np.concatenate(idx), np.concatenate(val)


def fixed_point_sum(idx, val, n_params):
    """The contract's sum: rint(c 2^32) per contribution as int64, integer sums, one conversion to fp32; NaN where poisoned"""
    bad = ~(np.abs(val) < np.float32(2.0 ** 31))
    q = np.rint(np.where(bad, 0, val).astype(np.float64) * 2.0 ** 32).astype(np.int64)
    acc = np.zeros(n_params, np.int64)
    np.add.at(acc, idx, q)
    out = acc.astype(np.float32) * np.float32(2.0 ** -32)
    out[np.unique(idx[bad])] = np.nan
    return out


@functools.lru_cache(maxsize=None)
def x_reference(case, n=N):
    """The contract's dL_dparams of backward (g_tab) and of backward_backward_input (g2_tab) for the first n rows"""
    (D, F, ty, ip, L, log2, base, pls), _ = X_CASES[case]
    off, res = x_tables(case)
    pos, table, dly, u = (a[:n] if i != 1 else a for i, a in enumerate(x_inputs(case)))
    r = dict(pos=pos, table=table, dly=dly, u=u)
    for key, second in (("g_tab", False), ("g2_tab", True)):
        idx, val = contributions(pos, dly, u, off, res, F, ty, ip, second)
        r[key] = fixed_point_sum(idx, val, off[-1] * F)
        r[key].setflags(write=False)
    return r
