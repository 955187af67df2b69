"""References for the rendering operators of neus2_amd/volrend.py, and the inputs the tests share.

* float64 torch restatements of neus_alpha and composite (differentiable, the serial definition);
* a float64 numpy composite written as plain loops, forward and backward (the B_i recurrence), with the same
  expressions evaluated on absolute values (the A of the tests' error bound);
* a numpy float32 restatement of march, in two evaluation orders (ray by ray with scalars, step by step with arrays);
* the fp32 stock-PyTorch formulation a user would write without the operators: the per-ray exclusive product from a
  global cumsum of log1p(-alpha) with per-ray offsets, the early stop as a mask. It is the accuracy floor of the
  gradient tests and the timing baseline of scripts/bench_volrend.py.

Nothing here touches the library.
"""
import numpy as np
import torch

EPS = 1e-5
DT = float(np.float32(np.sqrt(3.0) / 1024))
LENGTHS = (0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 300)  # 32 / 33: either side of the long-ray threshold
RAYS = (1, 65, 200)
T_STOPS = (0.0, 1e-4)
CHANNELS = (1, 3, 7)
ALPHA_CASES = ((20.0, 0.5), (64.0, 0.0))  # (inv_s, cos_anneal_ratio)
AMBIGUOUS_REL = 1e-3


# ------------------------------------------------------------------------------------------------ shared inputs
def ray_lengths(R, seed=0):
    if R == 1:
        return np.array([300], np.int64)
    if R <= 65:
        return np.array([LENGTHS[(i * 7 + 3) % len(LENGTHS)] for i in range(R)], np.int64)
    rng = np.random.default_rng(1000 + seed)
    n = np.concatenate([np.array(LENGTHS), rng.choice(np.array(LENGTHS), R - len(LENGTHS), p=_length_p())])
    return rng.permutation(n).astype(np.int64)


def _length_p():
    p = np.ones(len(LENGTHS))
    p[-1] = 0.25  # few 300-sample rays: S stays a few thousand
    return p / p.sum()


def ranges_of(lengths):
    starts = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    return np.stack([starts, lengths], 1).astype(np.int32)


def composite_case(R, C, seed=0):
    """alpha [S], values [S, C], ranges [R, 2] and cotangents (g_out, g_opacity, g_weights), fp32 numpy. The 300-sample
    rays carry alphas of 0.01 - 0.12 (T passes 1e-4 mid-ray), the others 0.01 - 0.5."""
    n = ray_lengths(R, seed)
    rng = np.random.default_rng(seed * 7919 + R * 31 + C)
    S = int(n.sum())
    hi = np.repeat(np.where(n == 300, 0.12, 0.5), n)
    alpha = (0.01 + rng.uniform(0, 1, S) * (hi - 0.01)).astype(np.float32)
    values = rng.uniform(-1, 1, (S, C)).astype(np.float32)
    g = (rng.uniform(-1, 1, (R, C)).astype(np.float32), rng.uniform(-1, 1, R).astype(np.float32), rng.uniform(-1, 1, S).astype(np.float32))
    return alpha, values, ranges_of(n), g


def alpha_case(S, seed=0):
    """sdf in +-0.05, true_cos in +-[0.05, 0.95], dt = sqrt(3) / 1024 and a cotangent, fp32 numpy."""
    rng = np.random.default_rng(seed * 104729 + S)
    sdf = rng.uniform(-0.05, 0.05, S).astype(np.float32)
    cos = (rng.choice([-1.0, 1.0], S) * rng.uniform(0.05, 0.95, S)).astype(np.float32)
    cos = np.clip(cos, -0.95, 0.95)
    cos = np.where(np.abs(cos) < 0.05, np.sign(cos) * np.float32(0.05), cos).astype(np.float32)
    g = rng.uniform(-1, 1, S).astype(np.float32)
    return sdf, cos, np.full(S, DT, np.float32), g


ALPHA_SIZES = (1, 255, 257, 3001)  # one lane, either side of a 256-sample block, several blocks with a ragged end


def march_case(R=200, G=16, seed=0):
    """Rays towards the unit cube, ~30 % occupancy: rays that miss the cube, rays with t_min >= t_max, rays along which
    more than 48 steps are occupied (a band of full occupancy)."""
    rng = np.random.default_rng(seed + 77)
    occ = (rng.uniform(0, 1, (G, G, G)) < 0.3).astype(np.uint8)
    occ[:, G // 2 - 1:G // 2 + 1, :] = 1  # a slab: rays running inside it keep every step and hit max_per_ray
    o = rng.uniform(-0.5, 1.5, (R, 3)).astype(np.float32)
    target = rng.uniform(0.1, 0.9, (R, 3)).astype(np.float32)
    k = R // 4
    o[:k, 1] = 0.5
    target[:k, 1] = 0.5  # inside the slab
    o[0], target[0] = (-0.1, 0.5, -0.1), (0.9, 0.5, 0.9)  # its diagonals: more than 48 occupied steps
    o[1], target[1] = (1.1, 0.5, -0.1), (0.1, 0.5, 0.9)
    d = target - o
    d[R - 20:R - 10] = np.abs(d[R - 20:R - 10]) + 0.1
    o[R - 20:R - 10] = 1.2  # pointing away: they miss the cube
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.float32(1) / d
        ta, tb = (np.float32(0) - o) * inv, (np.float32(1) - o) * inv
    t_min = np.maximum(np.minimum(ta, tb).max(1), np.float32(0)).astype(np.float32)
    t_max = np.maximum(ta, tb).min(1).astype(np.float32)
    t_min[R - 10:R - 5] = t_max[R - 10:R - 5]            # t_min == t_max
    t_min[R - 5:] = t_max[R - 5:] + np.float32(0.25)     # t_min > t_max
    return o, d, t_min, t_max, occ


# ------------------------------------------------------------------------------------------------ neus_alpha
def alpha_terms(sdf, cos, dt, inv_s, ratio):
    """(q, c) with q = (p + 1e-5) / (c + 1e-5) before the clamp, in the dtype of the inputs (torch)."""
    a1 = torch.relu(0.5 - 0.5 * cos)
    a2 = torch.relu(-cos)
    iter_cos = -(a1 * (1.0 - ratio) + a2 * ratio)
    h = iter_cos * dt * 0.5
    c = torch.sigmoid((sdf - h) * inv_s)
    p = c - torch.sigmoid((sdf + h) * inv_s)
    return (p + EPS) / (c + EPS), c


def neus_alpha(sdf, cos, dt, inv_s, ratio):
    """float64 reference when given float64 tensors; the stock fp32 formulation when given fp32 tensors."""
    return torch.clamp(alpha_terms(sdf, cos, dt, inv_s, ratio)[0], 0.0, 1.0)


neus_alpha_stock = neus_alpha


# ------------------------------------------------------------------------------------------------ composite
def composite(alpha, values, ranges, t_stop):
    """float64 torch, differentiable, ray by ray in sample order -> (out, opacity, weights, n_composited, T) with T the
    transmittance before each sample whether or not it is taken."""
    R, C = len(ranges), values.shape[1]
    out, op, w_all, T_all, n_all = [], [], [], [], []
    for start, count in np.asarray(ranges).tolist():
        a, v = alpha[start:start + count], values[start:start + count]
        T = torch.cat([torch.ones(1, dtype=alpha.dtype), torch.cumprod(1.0 - a, 0)])[:count]
        below = (T.detach() < t_stop).nonzero()
        n = int(below[0]) if len(below) else count
        w = torch.cat([a[:n] * T[:n], torch.zeros(count - n, dtype=alpha.dtype)])
        out.append((w[:, None] * v).sum(0))
        op.append(w.sum())
        w_all.append(w)
        T_all.append(T.detach())
        n_all.append(n)
    cat = lambda xs, shape: torch.cat(xs) if xs else torch.zeros(shape, dtype=alpha.dtype)
    return (torch.stack(out) if R else torch.zeros((0, C), dtype=alpha.dtype), torch.stack(op) if R else torch.zeros(0, dtype=alpha.dtype),
            cat(w_all, 0), np.array(n_all, np.int32), cat(T_all, 0))


def ambiguous_rays(T, ranges, t_stop):
    """Rays where some T_i lies within a relative 1e-3 of t_stop: the cut index may differ by rounding."""
    T = np.asarray(T, np.float64)
    near = np.abs(T - t_stop) <= AMBIGUOUS_REL * t_stop if t_stop > 0 else np.zeros(len(T), bool)
    return np.array([bool(near[s:s + c].any()) for s, c in np.asarray(ranges).tolist()], bool)


def composite_loops(alpha, values, ranges, t_stop, g_out, g_opacity, g_weights):
    """float64 numpy, plain loops: the forward as defined, the backward by the reverse recurrence
    B_{i-1} = alpha_i G_i + (1 - alpha_i) B_i, and each result's expression over absolute values (keys 'A_*')."""
    alpha, values = np.asarray(alpha, np.float64), np.asarray(values, np.float64)
    g_out, g_opacity, g_weights = (np.asarray(x, np.float64) for x in (g_out, g_opacity, g_weights))
    S, C = values.shape
    R = len(ranges)
    r = {k: np.zeros((R, C)) for k in ("out", "A_out")}
    r.update({k: np.zeros(R) for k in ("opacity", "A_opacity")})
    r.update({k: np.zeros(S) for k in ("weights", "A_weights", "T", "g_alpha", "A_g_alpha")})
    r.update({k: np.zeros((S, C)) for k in ("g_values", "A_g_values")})
    r["n"] = np.zeros(R, np.int32)
    for ray, (start, count) in enumerate(np.asarray(ranges).tolist()):
        T, n = 1.0, 0
        for i in range(start, start + count):
            if T < t_stop:
                break
            w = alpha[i] * T
            r["T"][i], r["weights"][i], r["A_weights"][i] = T, w, abs(w)
            r["out"][ray] += w * values[i]
            r["A_out"][ray] += abs(w) * np.abs(values[i])
            r["opacity"][ray] += w
            r["A_opacity"][ray] += abs(w)
            T *= 1.0 - alpha[i]
            n += 1
        r["n"][ray] = n
        B = Babs = 0.0
        for i in range(start + n - 1, start - 1, -1):
            G = g_weights[i] + g_opacity[ray] + float(g_out[ray] @ values[i])
            Gabs = abs(g_weights[i]) + abs(g_opacity[ray]) + float(np.abs(g_out[ray]) @ np.abs(values[i]))
            r["g_alpha"][i] = r["T"][i] * (G - B)
            r["A_g_alpha"][i] = abs(r["T"][i]) * (Gabs + Babs)
            r["g_values"][i] = r["weights"][i] * g_out[ray]
            r["A_g_values"][i] = np.abs(r["weights"][i] * g_out[ray])
            B = alpha[i] * G + (1.0 - alpha[i]) * B
            Babs = abs(alpha[i]) * Gabs + abs(1.0 - alpha[i]) * Babs
    return r


def ray_index(ranges):
    """[S] int64 ray of each sample (torch), from packed ranges that tile [0, S)."""
    counts = ranges[:, 1].long()
    return torch.repeat_interleave(torch.arange(len(ranges), device=ranges.device), counts)


def composite_stock(alpha, values, ranges, t_stop, ray_idx=None):
    """fp32 stock PyTorch: exclusive per-ray product from a global cumsum of log1p(-alpha) with per-ray offsets, the
    early stop as a mask (T is non-increasing, so the mask is a prefix of the ray), sums by index_add. alpha is kept
    below 1 so one opaque sample does not put -inf into every later ray."""
    if ray_idx is None:
        ray_idx = ray_index(ranges)
    R = ranges.shape[0]
    l = torch.log1p(-alpha.clamp(max=1.0 - 1e-7))
    excl = torch.cumsum(l, 0) - l
    T = torch.exp(excl - excl[ranges[:, 0].long()[ray_idx]]) if len(alpha) else alpha
    take = T >= t_stop
    w = torch.where(take, alpha * T, torch.zeros_like(T))
    out = torch.zeros((R, values.shape[1]), dtype=alpha.dtype, device=alpha.device).index_add_(0, ray_idx, w[:, None] * values)
    opacity = torch.zeros(R, dtype=alpha.dtype, device=alpha.device).index_add_(0, ray_idx, w)
    n = torch.zeros(R, dtype=torch.int32, device=alpha.device).index_add_(0, ray_idx, take.to(torch.int32))
    return out, opacity, w, n


# ------------------------------------------------------------------------------------------------ march
F = np.float32
MAX_STEPS = 1 << 24


def march_by_ray(o, d, t_min, t_max, occ, dt, max_per_ray):
    """numpy float32, one ray at a time with scalars: t_k = t_min + (f32(k) + 0.5) * dt, p = o + t_k * d, every product
    and sum rounded to fp32 on its own -> (ranges, t, ray_idx)."""
    G = occ.shape[0]
    dt, Gf = F(dt), F(G)
    counts, ts, rs = [], [], []
    for r in range(len(o)):
        n, k = 0, 0
        while k < MAX_STEPS and n < max_per_ray:
            t = F(t_min[r] + F(F(F(k) + F(0.5)) * dt))
            if not t < t_max[r]:
                break
            p = [F(o[r, c] + F(t * d[r, c])) for c in range(3)]
            k += 1
            if not all(F(0) <= x < F(1) for x in p):
                continue
            x, y, z = (int(F(q * Gf)) for q in p)
            if occ[z, y, x]:
                ts.append(t)
                rs.append(r)
                n += 1
        counts.append(n)
    return ranges_of(np.array(counts, np.int64)), np.array(ts, F), np.array(rs, np.int32)


def march_by_step(o, d, t_min, t_max, occ, dt, max_per_ray):
    """The same arithmetic, all rays at once for each step k."""
    R, G = len(o), occ.shape[0]
    dt, Gf = F(dt), F(G)
    alive = np.ones(R, bool)
    n = np.zeros(R, np.int64)
    per_ray = [[] for _ in range(R)]
    k = 0
    with np.errstate(invalid="ignore", over="ignore"):
        while alive.any() and k < MAX_STEPS:
            t = (t_min + (F(k) + F(0.5)) * dt).astype(F)
            alive &= (t < t_max) & (n < max_per_ray)
            p = (o + (t[:, None] * d).astype(F)).astype(F)
            inside = ((p >= F(0)) & (p < F(1))).all(1)
            cell = np.where(inside[:, None], (p * Gf).astype(F), 0).astype(np.int64)
            keep = alive & inside & (occ[cell[:, 2], cell[:, 1], cell[:, 0]] != 0)
            for r in np.nonzero(keep)[0]:
                per_ray[r].append(t[r])
            n += keep
            k += 1
    ts = np.array([x for pr in per_ray for x in pr], F)
    rs = np.repeat(np.arange(R, dtype=np.int32), n)
    return ranges_of(n), ts, rs
