"""Differentiable NeuS rendering operators over packed rays (include/neus2_hip.h neus_volrend_*, csrc/volrend.hip):
the half of a NeuS between the networks of neus2_amd.tcnn and the pixel loss.

    ranges, t, ray_idx = march(rays_o, rays_d, t_min, t_max, occupancy, dt, max_per_ray)
    alpha = neus_alpha(sdf, true_cos, dt, inv_s, cos_anneal_ratio)
    out, opacity, weights, n_composited = composite(alpha, values, ranges, t_stop)
    color, opacity, depth, normal, weights, n_composited = render_neus(...)

Rays are packed: `ranges` is int32 [R, 2] = (start, count), a ray's samples contiguous in [start, start + count), in
ray order; a count of 0 is allowed. Tensors are contiguous CUDA tensors and the work goes on
torch.cuda.current_stream(). Arguments are checked before any native call (ValueError naming the argument). The
operators are once differentiable: a NeuS step needs no second order through them.
"""
from __future__ import annotations

import ctypes as C

import torch
from torch.autograd.function import once_differentiable

from ._lib import check, lib

__all__ = ["march", "neus_alpha", "composite", "render_neus"]

ALPHA_BLOCK = 256  # samples per partial sum of d/d inv_s (volrend.hip VR_BLOCK)


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _tensor(name, x, dtype, shape):
    """x is a contiguous tensor of the dtype and shape (None in `shape` = any size); returns its shape. The device is
    checked last (_on_cuda), after every other argument."""
    if not isinstance(x, torch.Tensor):
        raise ValueError(f"{name}: expected a torch.Tensor, got {type(x).__name__}")
    if x.dtype != dtype:
        raise ValueError(f"{name}: expected dtype {dtype}, got {x.dtype}")
    want = "[" + ", ".join("*" if s is None else str(s) for s in shape) + "]"
    if x.dim() != len(shape) or any(s is not None and s != g for s, g in zip(shape, x.shape)):
        raise ValueError(f"{name}: expected shape {want}, got {list(x.shape)}")
    if not x.is_contiguous():
        raise ValueError(f"{name}: expected a contiguous tensor")
    return tuple(x.shape)


def _on_cuda(**tensors):
    dev = None
    for name, x in tensors.items():
        if not isinstance(x, torch.Tensor):
            continue
        if not x.is_cuda:
            raise ValueError(f"{name}: expected a CUDA tensor, got device {x.device}")
        if dev is not None and x.device != dev:
            raise ValueError(f"{name}: on {x.device}, the other tensors are on {dev}")
        dev = x.device
    return dev


def _number(name, x, positive=False, lo=None, hi=None):
    if isinstance(x, bool) or not isinstance(x, (int, float)):
        raise ValueError(f"{name}: expected a Python number, got {type(x).__name__}")
    x = float(x)
    if x != x or (positive and not x > 0.0) or (lo is not None and x < lo) or (hi is not None and x > hi):
        raise ValueError(f"{name}: {x} is out of range")
    return x


def _ranges(ranges, n_samples):
    _tensor("ranges", ranges, torch.int32, (None, 2))
    if n_samples >= 2 ** 31:
        raise ValueError("ranges: int32 ranges address fewer than 2^31 samples")
    return ranges.shape[0]


# ---------------------------------------------------------------------------------------------------- march
def march(rays_o, rays_d, t_min, t_max, occupancy, dt, max_per_ray):
    """Samples along rays through an occupancy grid over the unit cube -> (ranges [R, 2] int32, t [S] f32, ray_idx [S]
    int32). No autograd. Step k of a ray has t_k = t_min + (k + 0.5) dt in fp32 (a multiply, then an add); the ray ends at
    the first t_k >= t_max; p = o + t_k d; the step is kept when p lies in [0, 1)^3, the byte occupancy[z, y, x] of
    its cell (int)(p G) is non-zero and fewer than max_per_ray steps of the ray were kept. The caller computes the
    ray-box interval (t_min, t_max); a ray with t_min >= t_max gets no samples. Two passes (count, then write) with one
    host synchronisation between them to size the outputs."""
    R = _tensor("rays_o", rays_o, torch.float32, (None, 3))[0]
    _tensor("rays_d", rays_d, torch.float32, (R, 3))
    _tensor("t_min", t_min, torch.float32, (R,))
    _tensor("t_max", t_max, torch.float32, (R,))
    G = _tensor("occupancy", occupancy, torch.uint8, (None, None, None))[0]
    if tuple(occupancy.shape) != (G, G, G) or G < 1 or G > 512 or G & (G - 1):
        raise ValueError(f"occupancy: expected a [G, G, G] grid with G a power of two from 1 to 512, got {list(occupancy.shape)}")
    dt = _number("dt", dt, positive=True)
    if dt == float("inf"):
        raise ValueError("dt: must be finite")
    if isinstance(max_per_ray, bool) or not isinstance(max_per_ray, int) or not 0 <= max_per_ray < 2 ** 31:
        raise ValueError(f"max_per_ray: expected an int in [0, 2^31), got {max_per_ray!r}")
    dev = _on_cuda(rays_o=rays_o, rays_d=rays_d, t_min=t_min, t_max=t_max, occupancy=occupancy)
    l = lib()
    counts = torch.empty(R, dtype=torch.int32, device=dev)
    args = (_stream(), C.c_uint32(R), _p(rays_o), _p(rays_d), _p(t_min), _p(t_max), _p(occupancy), C.c_uint32(G), C.c_float(dt),
            C.c_uint32(max_per_ray))
    with torch.cuda.device(dev):
        check(l.neus_volrend_march_count(*args, _p(counts)))
        ends = torch.cumsum(counts, 0, dtype=torch.int64)
        S = int(ends[-1].item()) if R else 0  # the one host synchronisation
        if S >= 2 ** 31:
            raise RuntimeError(f"march: {S} samples do not fit int32 ranges (lower max_per_ray or march fewer rays)")
        ranges = torch.stack(((ends - counts).to(torch.int32), counts), 1).contiguous()
        t = torch.empty(S, dtype=torch.float32, device=dev)
        ray_idx = torch.empty(S, dtype=torch.int32, device=dev)
        if S:
            check(l.neus_volrend_march_write(*args, _p(ranges), C.c_uint32(S), _p(t), _p(ray_idx)))
    return ranges, t, ray_idx


# ---------------------------------------------------------------------------------------------------- alpha
def _alpha_args(sdf, true_cos, dt, inv_s, ratio):
    n = sdf.shape[0]
    dt_t = dt if isinstance(dt, torch.Tensor) else None
    s_t = inv_s if isinstance(inv_s, torch.Tensor) else None
    return (_stream(), C.c_uint32(n), _p(sdf), _p(true_cos), _p(dt_t), C.c_float(0.0 if dt_t is not None else dt),
            _p(s_t), C.c_float(0.0 if s_t is not None else inv_s), C.c_float(ratio))


class _NeusAlpha(torch.autograd.Function):
    @staticmethod
    def forward(ctx, sdf, true_cos, inv_s, dt, ratio):
        alpha = torch.empty_like(sdf)
        with torch.cuda.device(sdf.device):
            check(lib().neus_volrend_alpha_forward(*_alpha_args(sdf, true_cos, dt, inv_s, ratio), _p(alpha)))
        ctx.save_for_backward(sdf, true_cos, *(x for x in (inv_s, dt) if isinstance(x, torch.Tensor)))
        ctx.inv_s = None if isinstance(inv_s, torch.Tensor) else inv_s
        ctx.dt = None if isinstance(dt, torch.Tensor) else dt
        ctx.ratio = ratio
        return alpha

    @staticmethod
    @once_differentiable
    def backward(ctx, g_alpha):
        sdf, true_cos, *rest = ctx.saved_tensors
        inv_s = rest.pop(0) if ctx.inv_s is None else ctx.inv_s
        dt = rest.pop(0) if ctx.dt is None else ctx.dt
        n = sdf.shape[0]
        g_alpha = g_alpha.contiguous()
        g_sdf, g_cos = torch.empty_like(sdf), torch.empty_like(sdf)
        n_part = (n + ALPHA_BLOCK - 1) // ALPHA_BLOCK
        partials = torch.empty(max(n_part, 1), dtype=torch.float64, device=sdf.device)
        g_s = torch.empty(1, dtype=torch.float32, device=sdf.device)
        with torch.cuda.device(sdf.device):
            check(lib().neus_volrend_alpha_backward(*_alpha_args(sdf, true_cos, dt, inv_s, ctx.ratio), _p(g_alpha), _p(g_sdf), _p(g_cos),
                                                    _p(partials), C.c_uint32(partials.shape[0]), _p(g_s)))
        g_inv_s = g_s.reshape(inv_s.shape) if isinstance(inv_s, torch.Tensor) and ctx.needs_input_grad[2] else None
        return g_sdf, g_cos, g_inv_s, None, None


def neus_alpha(sdf, true_cos, dt, inv_s, cos_anneal_ratio):
    """The NeuS SDF-to-alpha conversion, one value per sample: a1 = relu(0.5 - 0.5 cos), a2 = relu(-cos),
    iter_cos = -(a1 (1 - r) + a2 r), prev/next_sdf = sdf -/+ iter_cos dt / 2, c = sigmoid(prev_sdf inv_s),
    p = c - sigmoid(next_sdf inv_s), alpha = clamp((p + 1e-5) / (c + 1e-5), 0, 1). sdf, true_cos: [S] f32; dt: an [S] f32
    tensor or a positive float; inv_s: a 0-dim or [1] f32 tensor, or a float; cos_anneal_ratio: a float in [0, 1].
    Differentiable in sdf, true_cos and (when a tensor) inv_s; d/d inv_s is a fixed-order sum, bitwise repeatable."""
    S = _tensor("sdf", sdf, torch.float32, (None,))[0]
    _tensor("true_cos", true_cos, torch.float32, (S,))
    if isinstance(dt, torch.Tensor):
        _tensor("dt", dt, torch.float32, (S,))
        if dt.requires_grad:
            raise ValueError("dt: neus_alpha has no gradient for dt (pass dt.detach())")
    else:
        dt = _number("dt", dt, positive=True)
    if isinstance(inv_s, torch.Tensor):
        _tensor("inv_s", inv_s, torch.float32, () if inv_s.dim() == 0 else (1,))
    else:
        inv_s = _number("inv_s", inv_s)
    ratio = _number("cos_anneal_ratio", cos_anneal_ratio, lo=0.0, hi=1.0)
    _on_cuda(sdf=sdf, true_cos=true_cos, dt=dt, inv_s=inv_s)
    return _NeusAlpha.apply(sdf, true_cos, inv_s, dt, ratio)


# ---------------------------------------------------------------------------------------------------- composite
class _Composite(torch.autograd.Function):
    @staticmethod
    def forward(ctx, alpha, values, ranges, t_stop):
        S, Cn = values.shape
        R = ranges.shape[0]
        dev = alpha.device
        out = torch.empty((R, Cn), dtype=torch.float32, device=dev)
        opacity = torch.empty(R, dtype=torch.float32, device=dev)
        n_comp = torch.empty(R, dtype=torch.int32, device=dev)
        # the kernels write the samples inside a range; a sample no ray owns has no weight
        weights = torch.zeros(S, dtype=torch.float32, device=dev)
        trans = torch.zeros(S, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            check(lib().neus_volrend_composite_forward(_stream(), C.c_uint32(R), C.c_uint32(S), C.c_uint32(Cn), _p(alpha), _p(values), _p(ranges),
                                                       C.c_float(t_stop), _p(out), _p(opacity), _p(weights), _p(trans), _p(n_comp)))
        ctx.save_for_backward(alpha, values, ranges, trans, n_comp)
        ctx.mark_non_differentiable(n_comp)
        ctx.set_materialize_grads(False)
        return out, opacity, weights, n_comp

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out, g_opacity, g_weights, _g_n):
        alpha, values, ranges, trans, n_comp = ctx.saved_tensors
        S, Cn = values.shape
        R = ranges.shape[0]
        dev = alpha.device
        g_out = torch.zeros((R, Cn), dtype=torch.float32, device=dev) if g_out is None else g_out.contiguous()
        g_opacity = torch.zeros(R, dtype=torch.float32, device=dev) if g_opacity is None else g_opacity.contiguous()
        g_weights = None if g_weights is None else g_weights.contiguous()
        g_alpha = torch.zeros_like(alpha)
        g_values = torch.zeros_like(values)
        with torch.cuda.device(dev):
            check(lib().neus_volrend_composite_backward(_stream(), C.c_uint32(R), C.c_uint32(S), C.c_uint32(Cn), _p(alpha), _p(values), _p(ranges),
                                                        _p(trans), _p(n_comp), _p(g_out), _p(g_opacity), _p(g_weights), _p(g_alpha), _p(g_values)))
        return g_alpha, g_values, None, None


def composite(alpha, values, ranges, t_stop=1e-4):
    """Transmittance compositing of packed rays -> (out [R, C], opacity [R], weights [S], n_composited [R] int32).
    Per ray, in sample order, from T = 1: stop when T < t_stop (0 never stops); otherwise w = alpha T, out += w v,
    opacity += w, T *= 1 - alpha. Samples from the stop on have weight 0 and no gradient; n_composited counts the samples
    taken. alpha [S] f32, values [S, C] f32 with C from 1 to 8 (colour, depth, normals, features as columns), ranges [R, 2]
    int32. Differentiable in alpha and values for cotangents on out, opacity and weights; alpha = 1 is legal (the backward
    divides by nothing)."""
    S = _tensor("alpha", alpha, torch.float32, (None,))[0]
    _tensor("values", values, torch.float32, (S, None))
    if not 1 <= values.shape[1] <= 8:
        raise ValueError(f"values: expected 1 to 8 columns, got {values.shape[1]}")
    _ranges(ranges, S)
    t_stop = _number("t_stop", t_stop, lo=0.0)
    _on_cuda(alpha=alpha, values=values, ranges=ranges)
    return _Composite.apply(alpha, values, ranges, t_stop)


def render_neus(sdf, normals, dirs, dt, rgb, t, inv_s, ranges, cos_anneal_ratio, t_stop=1e-4):
    """A NeuS render of packed rays from per-sample network outputs -> (color [R, 3], opacity [R], depth [R],
    normal [R, 3], weights [S], n_composited [R]). sdf [S], normals [S, 3] (the SDF gradient), dirs [S, 3], rgb [S, 3],
    t [S]; true_cos = (dirs * normals).sum(-1) is taken in torch, so the normals' gradient flows through autograd."""
    S = _tensor("sdf", sdf, torch.float32, (None,))[0]
    _tensor("normals", normals, torch.float32, (S, 3))
    _tensor("dirs", dirs, torch.float32, (S, 3))
    _tensor("rgb", rgb, torch.float32, (S, 3))
    _tensor("t", t, torch.float32, (S,))
    _ranges(ranges, S)
    _on_cuda(sdf=sdf, normals=normals, dirs=dirs, rgb=rgb, t=t, ranges=ranges)
    true_cos = (dirs * normals).sum(-1)
    alpha = neus_alpha(sdf, true_cos, dt, inv_s, cos_anneal_ratio)
    values = torch.cat((rgb, t[:, None], normals), 1)
    out, opacity, weights, n_comp = composite(alpha, values, ranges, t_stop)
    return out[:, 0:3], opacity, out[:, 3], out[:, 4:7], weights, n_comp
