"""Float64 PyTorch (CPU) restatement of the general grid encoding (neus2_amd/csrc/grid_nd.hip) - TEST INFRASTRUCTURE ONLY.

Written from the encoding's definition (my_tcnn encodings/grid.h), in the style of tests/torch_ref.hash_grid, for any number
of input dims D, features per level F, grid type (Hash / Dense / Tiled) and interpolation (Linear / Smoothstep):

  level tables   resolution ceil(exp2(l log2(per_level_scale)) base - 1) + 1 in fp32, scale = resolution - 1, entries
                 next_multiple(res^D, 8) capped at base^D (Tiled) or 2^log2_hashmap_size (Hash)          (grid.h:1472-1508)
  index          strides accumulate while stride <= level size; a Hash level smaller than its resolution takes the xor
                 of pos[d] * prime[d]; modulo the level size                                                (grid.h:137-153)
  interpolation  p = x scale + 0.5, corner floor(p), fraction t = p - floor(p); weight t or t^2 (3 - 2 t) per axis

The table is [n_entries, F] (parameter layout [level][entry][F]); the output [N, F L]. Everything is differentiable in x
and the table by autograd, to any order.
"""
from __future__ import annotations

import numpy as np
import torch

PRIMES = (1, 2654435761, 805459861, 3674653429)
M32 = 0xFFFFFFFF


def level_tables(n_dims, n_levels, log2_hashmap_size, base_resolution, per_level_scale, grid_type="Hash"):
    """Level offsets (in entries) and resolutions."""
    off, res = [0], []
    for l in range(n_levels):
        s = np.float32(np.exp2(np.float32(l) * np.float32(np.log2(np.float64(per_level_scale))))) * np.float32(base_resolution) - np.float32(1)
        r = int(np.ceil(s)) + 1
        p = (min(r ** n_dims, M32 // 2) + 7) // 8 * 8
        if grid_type == "Tiled":
            p = min(p, base_resolution ** n_dims)
        elif grid_type == "Hash":
            p = min(p, 1 << log2_hashmap_size)
        elif grid_type != "Dense":
            raise ValueError(grid_type)
        res.append(r)
        off.append(off[-1] + p)
    return off, res


def index(hsize, res, g, grid_type="Hash"):
    """g: [..., D] int64 corner positions -> entry within the level."""
    D = g.shape[-1]
    stride, idx = 1, torch.zeros_like(g[..., 0])
    for d in range(D):
        if stride > hsize:
            break
        idx = (idx + g[..., d] * stride) & M32
        stride = (stride * res) & M32
    if grid_type == "Hash" and hsize < stride:
        idx = torch.zeros_like(g[..., 0])
        for d in range(D):
            idx = idx ^ ((g[..., d] * PRIMES[d]) & M32)
    return idx % hsize


def interpolation_weight(t, interpolation):
    if interpolation == "Linear":
        return t
    if interpolation == "Smoothstep":
        return t * t * (3 - 2 * t)
    raise ValueError(interpolation)


def grid_encode(x, table, off, res, grid_type="Hash", interpolation="Linear", valid_level=None):
    """x: [N, D] float64; table: [n_entries, F] float64. Returns [N, F L]."""
    N, D = x.shape
    F = table.shape[1]
    outs = []
    for l in range(len(res)):
        if valid_level is not None and l > valid_level:
            outs.append(torch.zeros(N, F, dtype=x.dtype))
            continue
        scale = float(res[l] - 1)
        p = x * scale + 0.5
        g = torch.floor(p.detach()).to(torch.int64)
        w1 = interpolation_weight(p - g.to(x.dtype), interpolation)
        acc = 0
        for c in range(1 << D):
            bits = [(c >> d) & 1 for d in range(D)]
            w = 1
            for d in range(D):
                w = w * (w1[:, d] if bits[d] else 1 - w1[:, d])
            e = index(off[l + 1] - off[l], res[l], g + torch.tensor(bits, dtype=torch.int64), grid_type) + off[l]
            acc = acc + w[:, None] * table[e]
        outs.append(acc)
    return torch.cat(outs, dim=1)


def fraction_margin(x32, res):
    """Per sample, the smallest distance of the fp32 level position fmaf(x, scale, 0.5) to an integer over the levels and
    dims (the derivative of the encoding jumps at the integers). x32: [N, D] float32 numpy."""
    m = np.full(x32.shape[0], np.inf)
    for r in res:
        p = (x32.astype(np.float64) * float(r - 1) + 0.5).astype(np.float32).astype(np.float64)
        m = np.minimum(m, np.abs(p - np.rint(p)).min(axis=1))
    return m


def grid_network(ph, pos, shapes, off, res, n_features, grid_type, interpolation, scale=1.0, ambiguous_below=1e-4):
    """The float64 graph of a general grid in front of a ReLU FullyFusedMLP with a linear output, with the fp16 modelling of
    tests/bbi_ref.py: an fp16 rounding (forward value and backward gradient, the latter times the loss `scale`) wherever the
    device stores fp16 - here the grid's features too, which the device computes in fp32 and rounds once.
    ph: fp16 parameters [matrices in order | table]; shapes: the matrices' (rows, cols), the first with the padded input
    width. Returns dict(xt, leaves = [matrices..., table], out [n, out_pad], ambiguous [n] bool: a hidden pre-activation
    within `ambiguous_below` of 0, where the device's fp32 sum may take the other ReLU branch)."""
    from bbi_ref import r16_fn
    r16 = r16_fn(scale)
    pd = torch.tensor(ph.astype(np.float64))
    mats, o = [], 0
    for r, k in shapes:
        mats.append(pd[o:o + r * k].reshape(r, k).clone().requires_grad_(True))
        o += r * k
    tab = pd[o:].reshape(-1, n_features).clone().requires_grad_(True)
    xt = torch.tensor(pos.astype(np.float64), requires_grad=True)
    e = r16(grid_encode(xt, tab, off, res, grid_type, interpolation))
    h = torch.nn.functional.pad(e, (0, shapes[0][1] - e.shape[1]))
    ambiguous = np.zeros(pos.shape[0], bool)
    for li, Wm in enumerate(mats):
        z = r16(h @ Wm.T)
        if li < len(mats) - 1:
            ambiguous |= (np.abs(z.detach().numpy()) < ambiguous_below).any(axis=1)
            h = r16(torch.relu(z))
    return dict(xt=xt, leaves=mats + [tab], out=z, ambiguous=ambiguous)


def network_params(rng, shapes, width, n_dims, n_table):
    """fp16 parameters [matrices | table uniform in +-1] with O(1) pre-activations, so that few of them fall within the
    ambiguity threshold of 0: a D-linear interpolation of uniform +-1 values has rms 3^-1/2 (2/3)^(D/2) (each axis mixes
    two values with weights t, 1 - t: E[t^2 + (1 - t)^2] = 2/3), so the first matrix, which reads `width` live columns of
    it, is drawn with sigma 1.2 / (rms sqrt(width)); the others with 1.2 / sqrt(fan_in) as tests/bbi_ref.net_params."""
    rms = 3.0 ** -0.5 * (2.0 / 3.0) ** (n_dims / 2.0)
    sig = [1.2 / (rms * np.sqrt(width))] + [1.2 / np.sqrt(k) for _, k in shapes[1:]]
    return np.concatenate([rng.normal(0, s, (r, k)).ravel() for s, (r, k) in zip(sig, shapes)] + [rng.uniform(-1, 1, n_table)]).astype(np.float16)
