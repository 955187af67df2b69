"""Float64 autograd references for the complete backward_backward_input and the torch modules on top of it — TEST
INFRASTRUCTURE ONLY (shared by test_gpu_bbi_full.py and test_gpu_torch_modules.py).

The grid: 4 levels, log2_hashmap_size 9, base_resolution 4, per_level_scale 2 -> level offsets [0, 64, 576, 1088, 1600]:
two dense and two hashed levels. Networks are modelled as test_gpu_grid_mlp.py does: torch_ref.hash_grid in float64 with
the oracle's bit-exact fp16 features substituted for the forward values, and an fp16 rounding (R16) at every point where
the device stores fp16 (each layer's pre-activation and activation, forward and backward)."""
import numpy as np
import torch

from torch_ref import grid_tables, hash_grid

L, LOG2T, BASE, PLS = 4, 9, 4, 2.0
DE = 16
ENC_CFG = {"otype": "HashGrid", "n_levels": L, "n_features_per_level": 2, "log2_hashmap_size": LOG2T, "base_resolution": BASE,
           "per_level_scale": PLS}
OFF, RES = grid_tables(L, LOG2T, BASE, PLS)
assert OFF == [0, 64, 576, 1088, 1600]
N_GRID = 2 * OFF[-1]
AMBIGUOUS = 1e-4  # |hidden pre-activation| below this: the device's fp32 sum may take the other ReLU branch

# name -> (HashGrid in front?, n_neurons, n_hidden_layers, n_output_dims)
NETS = {"dnet": (True, 64, 1, 1), "gridmlp": (True, 16, 2, 3), "mlp": (False, 16, 2, 1)}


def net_cfg(name, activation="ReLU"):
    _, W, NH, _ = NETS[name]
    return {"otype": "FullyFusedMLP", "activation": activation, "output_activation": "None", "n_neurons": W, "n_hidden_layers": NH}


def net_shapes(name):
    _, W, NH, _ = NETS[name]
    return [(W, 16)] + [(W, W)] * (NH - 1) + [(16, W)]


def net_params(name, rng, sigma=None):
    """fp16 parameter vector [matrices in order | grid (HashGrid networks)] with O(1) activations."""
    enc = NETS[name][0]
    mats = [rng.normal(0, sigma if sigma else 1.2 / np.sqrt(k), (r, k)) for r, k in net_shapes(name)]
    parts = [a.ravel() for a in mats] + ([rng.uniform(-1, 1, N_GRID)] if enc else [])
    return np.concatenate(parts).astype(np.float16)


def r16_fn(scale=1.0):
    """fp16 storage point: rounds the value forward and the gradient backward (the gradient times `scale`, the loss
    scale the device applies to dL_dy; the double backward's fronts are rounded unscaled, as the device stores them)."""
    class R16(torch.autograd.Function):
        @staticmethod
        def forward(ctx, v):
            return v.to(torch.float16).to(torch.float64)

        @staticmethod
        def backward(ctx, g):
            return R16B.apply(g)

    class R16B(torch.autograd.Function):
        @staticmethod
        def forward(ctx, g):
            return (g * scale).to(torch.float16).to(torch.float64) / scale

        @staticmethod
        def backward(ctx, gg):
            return R16.apply(gg)
    return R16.apply


def oracle_features(grid_h, pos):
    """GridEncoding<__half>'s features bit for bit (fp16 accumulation, grid.h:275-297) from the CPU oracle."""
    import oracle as O
    ocfg = O.make_cfg(n_levels=L, log2_hashmap_size=LOG2T, base_resolution=BASE, per_level_scale=PLS)
    olay = O.layout(ocfg)
    op = np.zeros(olay["n_params"], np.float32)
    op[olay["grid_off"]:olay["grid_off"] + N_GRID] = grid_h.astype(np.float32)
    renc, _ = O.grid_forward(ocfg, op, pos, L)
    return np.asarray(renc, np.float64)


def network(name, ph, pos, scale=1.0):
    """The float64 graph of a network: dict(xt, leaves = [matrices..., table?], out [n, 16], ambiguous [n] bool)."""
    enc = NETS[name][0]
    r16 = r16_fn(scale)
    pd = torch.tensor(ph.astype(np.float64))
    mats, o = [], 0
    for r, k in net_shapes(name):
        mats.append(pd[o:o + r * k].reshape(r, k).clone().requires_grad_(True))
        o += r * k
    xt = torch.tensor(pos.astype(np.float64), requires_grad=True)
    leaves = list(mats)
    if enc:
        tab = pd[o:].reshape(-1, 2).clone().requires_grad_(True)
        leaves.append(tab)
        e = hash_grid(xt, tab, OFF, RES)
        e = e + (torch.tensor(oracle_features(ph[o:], pos)) - e).detach()
        h = torch.nn.functional.pad(e, (0, DE - 2 * L))
    else:  # the Identity encoding pads the input to 16 with ones (identity.h:44-70); the MLP reads it as fp16
        h = r16(torch.cat([xt, torch.ones(pos.shape[0], 16 - pos.shape[1], dtype=torch.float64)], 1))
    ambiguous = np.zeros(pos.shape[0], bool)
    for li, Wm in enumerate(mats):
        z = r16(h @ Wm.T)
        if li < len(mats) - 1:
            ambiguous |= (np.abs(z.detach().numpy()) < AMBIGUOUS).any(axis=1)
            h = r16(torch.relu(z))
    return dict(xt=xt, leaves=leaves, out=z, ambiguous=ambiguous)


def flat(grads):
    return np.concatenate([np.zeros(0)] + [g.detach().numpy().ravel() for g in grads])


def rel_cos(x, y):
    x, y = np.asarray(x, np.float64).ravel(), np.asarray(y, np.float64).ravel()
    return np.linalg.norm(x - y) / max(np.linalg.norm(y), 1e-30), x @ y / max(np.linalg.norm(x) * np.linalg.norm(y), 1e-30)


def record(test, **metrics):
    """One line of measured values into the suite's parity_metrics.jsonl, through the sibling test's recorder."""
    from test_gpu_grid_mlp import _record
    _record(test, **metrics)
