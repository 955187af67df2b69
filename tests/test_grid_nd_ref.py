"""tests/grid_nd_ref.py (the float64 restatement the general grid's GPU tests compare against) checked on the CPU:
* for 3 dims, 2 features, Hash, Linear its tables and output equal tests/torch_ref.grid_tables / hash_grid exactly;
* the level sizes of the Tiled and Dense types, and of the 2-D and 4-D hashed configs the GPU tests use;
* the Tiled index tiles, the Dense index is the plain row-major one;
* the Smoothstep first derivative against a central difference."""
import numpy as np
import torch

import grid_nd_ref as G
from torch_ref import grid_tables, hash_grid


def test_matches_torch_ref_for_the_3d_hash_grid():
    for cfg in [(8, 14, 16, 1.5), (4, 9, 4, 2.0), (6, 12, 8, 1.5)]:
        off, res = G.level_tables(3, *cfg)
        assert (off, res) == grid_tables(*cfg)
        rng = np.random.default_rng(1)
        tab = torch.tensor(rng.uniform(-1, 1, (off[-1], 2)))
        x = torch.tensor(rng.uniform(0.0, 1.0, (64, 3)))
        assert torch.equal(G.grid_encode(x, tab, off, res), hash_grid(x, tab, off, res))
        assert torch.equal(G.grid_encode(x, tab, off, res, valid_level=1), hash_grid(x, tab, off, res, 1))


def test_level_sizes():
    sizes = lambda off: [b - a for a, b in zip(off, off[1:])]
    # 2-D hash, base 8, x1.5: resolutions 8 .. 61; 2^10 entries cap levels 4 and 5 (41^2, 61^2 > 1024)
    off, res = G.level_tables(2, 6, 10, 8, 1.5)
    assert res == [8, 12, 18, 27, 41, 61]
    assert sizes(off) == [64, 144, 328, 736, 1024, 1024]
    # 3-D hash, 2^12: levels 2 .. 5 hashed
    off, res = G.level_tables(3, 6, 12, 8, 1.5)
    assert [r ** 3 > 4096 for r in res] == [False, False, True, True, True, True]
    assert sizes(off) == [512, 1728, 4096, 4096, 4096, 4096]
    # 4-D hash, base 4: resolutions 4, 6, 9, 14; levels 2 and 3 hashed
    off, res = G.level_tables(4, 4, 12, 4, 1.5)
    assert res == [4, 6, 9, 14] and sizes(off) == [256, 1296, 4096, 4096]
    # Dense is not capped: 4^3, 8^3, 16^3
    off, res = G.level_tables(3, 3, 19, 4, 2.0, "Dense")
    assert res == [4, 8, 16] and sizes(off) == [64, 512, 4096]
    # Tiled: every level capped at base^D
    off, res = G.level_tables(2, 4, 19, 8, 2.0, "Tiled")
    assert res == [8, 16, 32, 64] and sizes(off) == [64, 64, 64, 64]


def test_tiled_and_dense_index():
    g = torch.tensor([[3, 5], [11, 5], [3, 13], [63, 63]])
    # Tiled, 64 entries at resolution 32: stride 1, then 32 (<= 64), then 1024 stops the loop: (x + 32 y) mod 64
    assert G.index(64, 32, g, "Tiled").tolist() == [(3 + 32 * 5) % 64, (11 + 32 * 5) % 64, (3 + 32 * 13) % 64, (63 + 32 * 63) % 64]
    # the same level as a Hash level is hashed instead
    assert G.index(64, 32, g, "Hash").tolist() == [int((x ^ ((y * G.PRIMES[1]) & G.M32)) % 64) for x, y in g.tolist()]
    # Dense: row-major, x fastest
    g3 = torch.tensor([[1, 2, 3], [7, 0, 5]])
    assert G.index(512, 8, g3, "Dense").tolist() == [1 + 8 * 2 + 64 * 3, 7 + 64 * 5]


def test_smoothstep_first_derivative():
    for D, F in [(2, 4), (3, 2), (4, 1)]:
        off, res = G.level_tables(D, 3, 10, 4, 1.5)
        rng = np.random.default_rng(D)
        tab = torch.tensor(rng.uniform(-1, 1, (off[-1], F)))
        x0 = rng.uniform(0.05, 0.95, (32, D))
        x0 = x0[G.fraction_margin(x0.astype(np.float32), res) > 1e-3]
        x = torch.tensor(x0, requires_grad=True)
        dly = torch.tensor(rng.normal(0, 1, (x.shape[0], 3 * F)))
        y = G.grid_encode(x, tab, off, res, interpolation="Smoothstep")
        gx, = torch.autograd.grad((y * dly).sum(), x)
        h = 1e-6
        for d in range(D):
            e = torch.zeros(D, dtype=torch.float64)
            e[d] = h
            yp = G.grid_encode(x.detach() + e, tab, off, res, interpolation="Smoothstep")
            ym = G.grid_encode(x.detach() - e, tab, off, res, interpolation="Smoothstep")
            fd = ((yp - ym) * dly).sum(dim=1) / (2 * h)
            assert torch.allclose(gx[:, d], fd, rtol=1e-6, atol=1e-6)
        # Smoothstep is flat at the cell borders and equals Linear at the cell centres
        xc = (torch.floor(x.detach() * (res[0] - 1) + 0.5) + 0.0) / (res[0] - 1)  # fraction 0.5 at level 0
        a = G.grid_encode(xc, tab, off[:2], res[:1], interpolation="Smoothstep")
        b = G.grid_encode(xc, tab, off[:2], res[:1], interpolation="Linear")
        assert torch.allclose(a, b, atol=1e-12)
