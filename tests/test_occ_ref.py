"""CPU checks of tests/occ_ref.py: the plain occupancy references against the oracle's restatement and the scene
helpers, the restated device-order mean against float64, and the domain of the step networks."""
import numpy as np
import pytest

import occ_ref as R


def _sparse_grid(seed, frac, value=1.0, negatives=0.01):
    rng = np.random.default_rng(seed)
    g = np.zeros(R.G3, np.float32)
    u = rng.random(R.G3)
    g[u < frac] = value
    g[u > 1 - negatives] = -1.0
    return g


def order_free_grid(k=37, seed=5):
    return R.order_free_grid(k, seed)


def test_morton_is_a_bijection_with_the_scene_helper():
    from neus2_amd import scenes
    i = np.arange(R.G)
    X, Y, Z = np.meshgrid(i, i, i, indexing="ij")
    m = scenes._morton_expand(X) | (scenes._morton_expand(Y) << 1) | (scenes._morton_expand(Z) << 2)
    np.testing.assert_array_equal(R.MORTON, m.astype(np.uint32))
    assert np.array_equal(np.sort(R.MORTON.reshape(-1)), np.arange(R.G3))
    d = np.random.default_rng(0).random((R.G,) * 3).astype(np.float32)
    np.testing.assert_array_equal(R.to_dense(R.from_dense(d)), d)


@pytest.mark.parametrize("frac,value", [(0.01, 1.0), (0.5, 1.0), (1e-4, 0.5)])
def test_bitfield_equals_the_oracles(frac, value):
    """Zero samples and decay 1 leave the grid as it is; the oracle then writes the mean, mip 0 and the seven pools. The
    grid's cells are 0, `value` or -1 and its mean far from all three, so the oracle's double-summed mean and the device-
    order one give the same cells."""
    import oracle as O
    g = _sparse_grid(11, frac, value)
    cfg = O.make_cfg()
    params = np.zeros(O.layout(cfg)["n_params"], np.float32)
    rg, rbf = g.copy(), np.full(R.NBYTES * 8, 0xff, np.uint8)
    _, mean = O.density_grid_update(cfg, params, 14, 0, 0, 1, 1234, 1, rg, rbf, decay=1.0)
    np.testing.assert_array_equal(rg, g)
    dm = R.device_mean(g)
    assert abs(float(dm) - mean) <= R.mean_bound(g) + 2.0 ** -24 * mean
    assert min(abs(float(R.threshold(dm)) - v) for v in (0.0, value, -1.0)) > 1000 * R.mean_bound(g) > 0
    np.testing.assert_array_equal(R.bitfield_from_grid(g, R.threshold(dm)), rbf)
    assert (frac * value >= 0.1) == (R.threshold(dm) == R.MIN_OPTICAL_THICKNESS)


def test_bitfield_equals_the_scene_helper():
    from neus2_amd import scenes
    occ = np.random.default_rng(2).random((R.G,) * 3) < 0.003
    np.testing.assert_array_equal(R.pack_mips(R.mips_from_occupancy(occ)), scenes.bitfield_from_occupancy(occ))
    shell = scenes.shell_bitfield()
    mips = R.unpack_mips(shell)
    np.testing.assert_array_equal(R.pack_mips(R.mips_from_occupancy(mips[0])), shell)
    for m in range(1, 8):
        assert not mips[m][:32].any() and not mips[m][96:].any() and not mips[m][:, :, :32].any()


def test_pool_and_words_by_hand():
    occ = np.zeros((R.G,) * 3, bool)
    occ[0, 0, 0] = occ[127, 127, 127] = occ[5, 66, 97] = True
    mips = R.mips_from_occupancy(occ)
    for m in range(1, 8):
        want = {tuple(64 + ((c - 64) >> m) for c in cell) for cell in ((0, 0, 0), (127, 127, 127), (5, 66, 97))}
        assert {tuple(int(v) for v in c) for c in np.argwhere(mips[m])} == want
    w = R.linear_words(occ)
    nz = {int(i): int(w[i]) for i in np.flatnonzero(w)}
    assert nz == {0: 1, (127 << 9) | (127 << 2) | 3: 1 << 31, (5 << 9) | (66 << 2) | 3: 1 << 1}
    # the packed field: bit i & 7 of byte i >> 3, i the Morton index; (1, 0, 0) -> 1, (0, 1, 0) -> 2, (0, 0, 1) -> 4
    b = R.pack(occ)
    assert b[0] == 1 and b[-1] == 0x80
    one = np.zeros((R.G,) * 3, bool)
    one[1, 0, 0] = one[0, 0, 1] = True
    assert R.pack(one)[0] == (1 << 1) | (1 << 4)
    np.testing.assert_array_equal(R.unpack(b), occ)


def test_bbox_by_hand():
    f = np.float32
    empty = [np.zeros((R.G,) * 3, bool)] * 8
    np.testing.assert_array_equal(R.bbox(empty), f([R.FLT_MAX] * 3 + [-R.FLT_MAX] * 3))
    occ = np.zeros((R.G,) * 3, bool)
    occ[0, 64, 127] = True
    got = R.bbox([occ] + empty[1:])
    want = f([f(0) - f(1e-4), f(0.5) - f(1e-4), f(127 / 128) - f(1e-4), f(1 / 128) + f(1e-4), f(65 / 128) + f(1e-4), f(1) + f(1e-4)])
    np.testing.assert_array_equal(got, want)
    # a corner cell of mip 7 alone: 0.5 +- 64 and the pad 1e-4 * 128
    top = np.zeros((R.G,) * 3, bool)
    top[0, 0, 127] = True
    got = R.bbox(empty[:7] + [top])
    pad = f(1e-4) * f(128)
    want = f([f(-63.5) - pad, f(-63.5) - pad, f(63.5) - pad, f(-62.5) + pad, f(-62.5) + pad, f(64.5) + pad])
    np.testing.assert_array_equal(got, want)
    # a full grid pools to cells 63 and 64 of mip 7, one cell (of 1.0) either side of the centre: the widest box
    full = R.bbox(R.mips_from_occupancy(np.ones((R.G,) * 3, bool)))
    np.testing.assert_array_equal(full, f([f(-0.5) - pad] * 3 + [f(1.5) + pad] * 3))


def test_single_cells_cover_every_byte_offset():
    """The single-cell cases of tests/test_gpu_occ_build.py: in the mips the pool's upward walk writes (2..7, through
    32-bit ORs on the word that holds the byte) the one nonzero byte sits at every offset 0..3 of its word in some case."""
    seen = set()
    for cell in R.CORNERS + R.INNER_CORNERS:
        occ = np.zeros((R.G,) * 3, bool)
        occ[cell] = True
        bf = R.pack_mips(R.mips_from_occupancy(occ)).reshape(R.N_MIPS, R.NBYTES)
        seen |= {int(np.flatnonzero(bf[m])[0]) & 3 for m in range(2, R.N_MIPS)}
    assert seen == {0, 1, 2, 3}


def test_one_ulp_cells_leave_the_order_free_mean():
    """The threshold case of tests/test_gpu_occ_build.py: four 2^-8 cells raised and four lowered by one ulp; in the
    restated order the mean is still exactly 2^-8."""
    g, cells = R.order_free_grid()
    k1 = 8192 - 37
    m = np.float32(2.0 ** -8)
    g[cells[k1:k1 + 4]], g[cells[k1 + 4:k1 + 8]] = np.nextafter(m, np.float32(1)), np.nextafter(m, np.float32(0))
    assert R.device_mean(g) == m


def test_device_mean_within_the_summation_bound():
    rng = np.random.default_rng(3)
    for g in (rng.random(R.G3, dtype=np.float32), (rng.normal(0.05, 1.0, R.G3)).astype(np.float32),
              rng.exponential(0.02, R.G3).astype(np.float32), _sparse_grid(4, 0.3, 0.7)):
        exact = np.maximum(g.astype(np.float64), 0).mean()
        assert abs(float(R.device_mean(g)) - exact) <= R.mean_bound(g)
        assert R.mean_bound(g) <= 1e-5 * exact


def test_device_mean_exact_on_order_free_grids():
    g, _ = order_free_grid()
    assert R.device_mean(g) == np.float32(2.0 ** -8) == np.float32(g.astype(np.float64).mean())
    for frac, value in ((0.25, 1.0), (0.01, 0.5), (0.0, 1.0)):
        g = _sparse_grid(8, frac, value)
        assert float(R.device_mean(g)) == np.maximum(g.astype(np.float64), 0).mean()
    assert R.device_mean(np.full(R.G3, -3.0, np.float32)) == 0 and R.device_mean(np.full(R.G3, 0.75, np.float32)) == np.float32(0.75)


@pytest.mark.parametrize("name", sorted(R.STEP_NETS))
@pytest.mark.parametrize("variance", sorted(R.D0))
def test_step_network_domain(name, variance):
    """Over every representable density-input value of the columns the network reads: nothing overflows, the density is
    exactly 0 off the surface and D0 on it, and both stay so when the two exponentials are off by +-2^-16 relative."""
    v = R.din_values()
    assert v.min() == -0.5 and v.max() == 0.5 and np.array_equal(v * 4096, np.rint(v * 4096))
    rows, _ = R.STEP_NETS[name]
    cols = sorted({c for row in rows for c in range(3) if row[c]})
    if len(cols) <= 1:
        din = np.zeros((len(v), 3))
        din[:, cols] = v[:, None]
    elif name == "octant":  # units on separate columns: the extremes of the other two with every value of one
        ext = np.array([-0.5, -2.0 ** -12, 0.0, 2.0 ** -12, 0.5])
        parts = []
        for c in range(3):
            a, b = np.meshgrid(ext, ext, indexing="ij")
            for aa, bb in zip(a.ravel(), b.ravel()):
                d = np.zeros((len(v), 3))
                d[:, c] = v
                d[:, (c + 1) % 3], d[:, (c + 2) % 3] = aa, bb
                parts.append(d)
        din = np.concatenate(parts)
    else:  # two summed columns: the units read din_a + din_b only; one pair for every sum the columns can reach
        # matters. Every value of one column with the other's extremes, zero and its three values nearest to the opposite
        # (the zero sum where it exists and the smallest nonzero sums)
        k = np.clip(np.searchsorted(v, -v), 1, len(v) - 2)
        other = np.stack([np.full_like(v, -0.5), np.full_like(v, 0.5), np.zeros_like(v), v[k - 1], v[k], v[k + 1]], 1)
        din = np.zeros((other.size, 3))
        din[:, cols[0]], din[:, cols[1]] = np.repeat(v, other.shape[1]), other.ravel()
        s = din[:, cols[0]] + din[:, cols[1]]
        assert (s == 0).sum() > 1000 and np.abs(s[s != 0]).min() == 2.0 ** -12 and np.abs(s).max() == 1.0
    rep = {}
    on = R.step_net_on_surface(name, din)
    assert on.any() and (name == "all" or (~on).any())
    ref = R.step_net_density(name, din, variance, report=rep)
    assert rep["hidden_max"] <= 2.0 ** 15 and rep["sum_max"] < 65504, rep
    d0 = R.D0[variance]
    assert np.float16(d0) == d0
    for e1 in (0.0, -R.PERTURB, R.PERTURB):
        for e2 in (0.0, -R.PERTURB, R.PERTURB):
            d = ref if (e1, e2) == (0.0, 0.0) else R.step_net_density(name, din, variance, e1, e2)
            assert np.all(np.isfinite(d))
            np.testing.assert_array_equal(d[on], d0)
            np.testing.assert_array_equal(d[~on], 0.0)
    # the decayed values the updates leave behind are single float32 products above the 0.1 threshold for three steps
    x = np.float32(d0)
    for _ in range(3):
        x = x * np.float32(0.95)
        assert x > R.MIN_OPTICAL_THICKNESS
