"""Positions at the edges of the hash-grid encode's index arithmetic — TEST INFRASTRUCTURE ONLY (shared by
test_gpu_encode_edges.py and the selector probes of test_gpu_neus_exact.py)."""
import numpy as np

import scatter_cases as SC


def edge_positions(O, cfg, n, levels=(0, 5, 13), seed=22):
    """n float32 positions: 100 uniform in the unit cube; per level of `levels` 16 exactly on a cell boundary, 16 on a
    vertex and 8 on a boundary along one axis only; the corners of the unit cube; positions outside it (negative cells and
    cells past the resolution: the dense levels' true modulo); the rest uniform in [-0.4, 1.4]."""
    _, res, scale, _ = O.grid_tables(cfg)
    rng = np.random.default_rng(seed)
    parts = [rng.uniform(0.0, 1.0, (100, 3))]
    for l in levels:
        s, r = np.float64(scale[l]), int(res[l])
        k = rng.integers(0, r, (32, 3)).astype(np.float64)
        parts.append((k[:16] - 0.5) / s)  # fmaf(x, scale, 0.5) an integer: the boundary between two cells
        parts.append(k[16:] / s)          # a vertex of the level
        mixed = rng.uniform(0.0, 1.0, (8, 3))
        mixed[:, l % 3] = (k[:8, 0] - 0.5) / s  # on a boundary along one axis only
        parts.append(mixed)
    parts.append(np.array([[(i >> d) & 1 for d in range(3)] for i in range(8)], np.float64))  # 0.0 and 1.0
    parts.append(SC.OUTSIDE.astype(np.float64))
    parts.append(np.float64([[-0.3, 0.5, 0.5], [1.7, 0.5, 0.5], [0.5, -0.3, 1.7], [1.7, 1.7, 1.7], [-0.3, -0.3, -0.3]]))
    x = np.concatenate(parts)
    x = np.concatenate([x, rng.uniform(-0.4, 1.4, (n - len(x), 3))]).astype(np.float32)
    assert x.shape == (n, 3)
    return x
