"""The fused occupancy update (sample generation, k_nerf_density<L, W, 2>, splat, EMA, mean, bitfield, pools, linear
words, cull box) through neus_occ_update, bit for bit against oracle.density_grid_update and tests/occ_ref.py.

The density is made exactly computable by the step networks of tests/occ_ref.py (their domain is checked on the CPU in
tests/test_occ_ref.py): one hidden layer of +-2^15 units on the position columns, a zero hash table. A sample whose
position is on the network's surface has the density D0, every other sample exactly 0, so which cells of the grid are set
is decided by the bits of every sample's jittered position and by the cell its value is splatted into - and by nothing
else. The thin sets (slab: fp16(x) == 0.5, sheet: fp16(x) + fp16(y) == 1) keep a cell only when its own jitter falls into
a window of 2^-13 .. 2^-12.

Compared after every update, with no tolerance and no excluded cell: the density grid (as u32), all 8 mips of the
bitfield and the advanced density_grid_rng against the oracle; the testbed's linear words, the cull box and the mean (in
the device's summation order) against occ_ref on the oracle's grid and field."""
import ctypes as C
import os

import numpy as np
import pytest

import occ_ref as R
from gpu_util import env, occ_buffer

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
G3 = R.G3
Q = G3 // 4
DECAY = F(0.95)


class Bed:
    """A testbed, its oracle config and the occupancy state the test tracks beside it (the EMA step is not readable)."""

    def __init__(self, scene, L=14, W=64, **environment):
        import oracle as O
        from neus2_amd import config, pyngp
        cfg = config.load_json(os.path.join(ROOT, "configs", "nerf", "base.json"))
        cfg["encoding"]["n_levels"] = L
        cfg["network"]["n_neurons"] = W
        cfg["rgb_network"]["n_neurons"] = W
        with env(**environment):
            tb = pyngp.Testbed(pyngp.TestbedMode.Nerf)
            tb.set_dataset(scene["images"], scene["focal"], scene["principal"], scene["xforms"], 1)
            tb.reload_network_from_json(cfg, batch_size=4096)
        self.tb, self.L, self.W = tb, L, W
        self.lay = tb.layout()
        self.base = tb.get_params().copy()
        self.cfg = O.make_cfg(n_levels=L, width=W, per_level_scale=tb._net_cfg.per_level_scale)
        assert O.layout(self.cfg)["n_params"] == self.lay["n_params"] and self.lay["density_input_width"] == self.cfg.density_in
        self.ema_step = None
        self.params = None

    def load(self, name, variance=0.0):
        self.params = R.step_net_params(name, self.base, self.lay, self.W, int(self.lay["density_input_width"]), variance)
        self.tb.set_params(self.params)

    def restore(self, training_step):
        from neus2_amd._lib import NeusRestoreState, check, lib
        st = NeusRestoreState(training_step, 4096, 0, 0, 0.0, 0)
        check(lib().neus_testbed_restore_state(self.tb.handle, C.byref(st)))

    def occ_update(self, n_u, n_nu):
        from neus2_amd._lib import check, lib
        check(lib().neus_occ_update(self.tb.handle, None, C.c_uint32(n_u), C.c_uint32(n_nu)))

    def begin_at_step0(self):
        """The state before the first update of a training run: the update itself clears the grid and the EMA step."""
        self.restore(0)
        self.ema_step = 0

    def begin_after_step0(self, prev):
        """A state at training step 1 with EMA step 1 and the grid prev: one 1-sample update at step 0 resets the EMA step
        (and advances it to 1), then the step and the grid are set."""
        self.restore(0)
        self.occ_update(1, 0)
        self.restore(1)
        self.tb.set_density_grid(prev)
        self.ema_step = 1


def reference(bed, prev, n_u, n_nu):
    """The oracle's update from bed's state (parameters, rng, EMA step) and the grid prev, plus occ_ref's products of it."""
    import oracle as O
    rs, ri = bed.tb.get_rng()[2:4]
    rg = np.array(prev, F, copy=True)
    rbf = np.full(R.NBYTES * R.N_MIPS, 0xa5, np.uint8)
    st, mean = O.density_grid_update(bed.cfg, bed.params, bed.L, n_u, n_nu, bed.ema_step, rs, ri, rg, rbf, decay=float(DECAY))
    ref = dict(rng_in=(rs, ri), rng_out=st, grid=rg, bitfield=rbf, oracle_mean=mean, mean=R.device_mean(rg), **R.expected_from_bitfield(rbf))
    # the oracle sums the mean in double: its field is the device's as long as no cell sits between the two means
    lo, hi = sorted((float(ref["mean"]), float(F(mean))))
    assert not np.any((rg >= lo) & (rg <= hi) & (rg != 0)) or lo >= 0.1, "a cell between the oracle's mean and the device-order mean"
    return ref


def update_and_compare(bed, ref, n_u, n_nu, tag=""):
    """One neus_occ_update on bed (whose state must be the one ref was computed from) against ref; -> the device's grid."""
    tb = bed.tb
    assert tuple(tb.get_rng()[2:4]) == ref["rng_in"], f"{tag}: the beds' density_grid_rng differ"
    bed.occ_update(n_u, n_nu)
    bed.ema_step += 1
    g, bf = tb.get_density_grid()
    assert tb.get_rng()[2] == ref["rng_out"], tag
    bad = np.flatnonzero(g.view(np.uint32) != ref["grid"].view(np.uint32))
    assert bad.size == 0, (tag, "density grid", bad.size, [(int(i), [int(v) for v in np.argwhere(R.MORTON == i)[0]], float(g[i]), float(ref["grid"][i])) for i in bad[:8]])
    bf, wbf = bf.reshape(R.N_MIPS, R.NBYTES), ref["bitfield"].reshape(R.N_MIPS, R.NBYTES)
    for m in range(R.N_MIPS):
        np.testing.assert_array_equal(bf[m], wbf[m], err_msg=f"{tag}: mip {m}")
    np.testing.assert_array_equal(occ_buffer(tb, "lin"), ref["lin"], err_msg=f"{tag}: linear words")
    np.testing.assert_array_equal(occ_buffer(tb, "bbox").view(np.uint32), ref["bbox"].view(np.uint32), err_msg=f"{tag}: box {ref['bbox']}")
    got_mean = occ_buffer(tb, "mean")
    assert got_mean.view(np.uint32)[0] == np.array([ref["mean"]], F).view(np.uint32)[0], (tag, got_mean[0], ref["mean"])
    return g


def run(bed, prev, n_u, n_nu, tag=""):
    ref = reference(bed, prev, n_u, n_nu)
    update_and_compare(bed, ref, n_u, n_nu, tag)
    return ref


def seeded_grid(seed, d0, occupied=0.005, negative=0.005):
    """A previous grid: zeros, `occupied` of the cells at d0 (targets of the occupancy-biased samples) and `negative` of
    them at -1 (never trained: refused by both sample passes, kept by the EMA, 0 in the mean, never occupied)."""
    u = np.random.default_rng(seed).random(G3)
    g = np.zeros(G3, F)
    g[u < occupied] = d0
    g[u > 1 - negative] = -1.0
    return g


@pytest.fixture(scope="module")
def scene(torch_cuda):
    from neus2_amd import scenes
    return scenes.small_scene(n_views=4, width=64, height=48)


@pytest.fixture(scope="module")
def bed(scene):
    return Bed(scene)


@pytest.fixture(scope="module")
def bed_w16(scene):
    return Bed(scene, 1, 16)


def _assert_set(name, grid, d0):
    """What the occupied set must look like on the oracle's grid (guards the test's own construction)."""
    d = R.to_dense(grid)
    assert set(np.unique(grid).tolist()) <= {0.0, float(d0)}
    occ = d > 0
    half = {"half_x": 0, "half_y": 1, "half_z": 2}
    if name == "all":
        assert occ.all()
    elif name in half:
        o = np.moveaxis(occ, half[name], 0)
        assert o[:64].all() and not o[65:].any() and 0 < o[64].mean() < 0.1  # layer 64: the jitters below 2^-5 of a cell
    elif name == "octant":
        assert occ[:64, :64, :64].all() and not occ[65:].any() and not occ[:, 65:].any() and not occ[:, :, 65:].any()
    elif name == "slab_x":
        assert not occ[:63].any() and not occ[65:].any()
        assert 100 < occ[63].sum() < 600 and 200 < occ[64].sum() < 1200  # about 1 / 64 and 1 / 32 of 16384 cells
    elif name == "sheet_xy":
        i = np.arange(R.G)
        far = np.abs(i[:, None] + i[None, :] - 127) > 1
        assert not occ[far].any() and 300 < occ.sum() < 20000


@pytest.mark.parametrize("name,variance", [("all", 0.0), ("half_x", 0.0), ("half_y", 0.0), ("half_z", 0.3), ("octant", 0.0), ("slab_x", 0.0),
                                           ("sheet_xy", 0.0)])
def test_step0_exclusive_pass(bed, name, variance):
    """training_step 0, 128^3 uniform samples, no biased ones: the all-cells path (the sample of a cell from the inverse
    of the uniform hash, a plain store for the splat) on a grid the update clears itself."""
    bed.load(name, variance)
    bed.begin_at_step0()
    bed.tb.set_density_grid(np.full(G3, 7.0, F))  # the update at step 0 starts from zeros whatever the grid held
    ref = run(bed, np.zeros(G3, F), G3, 0, name)
    _assert_set(name, ref["grid"], R.D0[variance])


@pytest.mark.parametrize("name", ["slab_x", "sheet_xy", "half_y"])
def test_three_consecutive_updates(bed, name):
    """Updates at EMA steps 1, 2, 3 with a quarter of the cells sampled uniformly and as many biased to occupied cells, on
    a grid that is not reset (slab and sheet: sparse, mean below 0.1; half-space: mean above): D0 0.95^k appear as single float32 products, the biased pass retries against the previous
    grid, cells seeded negative stay as they are. The first update's splat target is read on its own: where the grid was
    0 before, the new grid is the splat itself."""
    d0 = F(R.D0[0.0])
    bed.load(name)
    prev = seeded_grid(3, d0)
    if name == "half_y":  # the half-space as a step-0 pass leaves it, so the mean is above 0.1: the threshold's other branch
        d = R.to_dense(prev)
        d[:, :64][d[:, :64] == 0] = d0
        prev = R.from_dense(d)
    bed.begin_after_step0(prev)
    seen = set()
    for k in range(3):
        ref = reference(bed, prev, Q, Q)
        g = update_and_compare(bed, ref, Q, Q, f"{name} update {k + 1}")
        if k == 0:
            tmp = occ_buffer(bed.tb, "density_tmp")
            assert set(np.unique(tmp).tolist()) <= {0.0, float(d0)}
            np.testing.assert_array_equal(tmp[prev == 0], ref["grid"][prev == 0])
            assert (tmp > 0).sum() > 50
        np.testing.assert_array_equal(g[prev < 0], prev[prev < 0])
        seen |= set(np.unique(g).tolist())
        assert (ref["mean"] >= 0.1) == (name == "half_y"), ref["mean"]
        prev = g
    decayed = [float(d0)]
    for _ in range(3):
        decayed.append(float(F(decayed[-1]) * DECAY))
    assert seen == set(decayed) | {0.0, -1.0}, (sorted(seen), decayed)
    assert bed.ema_step == 4


def test_ragged_sample_counts(bed):
    """Counts that end in a partial wave, that have only one of the two passes, that put the first biased sample inside a
    wave of uniform ones, and one with twelve times as many biased samples as there are cells for them to land in (many
    samples splat into one cell). Consecutive updates: the EMA step advances through the cases."""
    d0 = F(R.D0[0.0])
    bed.load("octant")
    prev = seeded_grid(5, d0)
    bed.begin_after_step0(prev)
    assert (1 << 17) > 10 * (prev > 0).sum()
    for n_u, n_nu in ((1, 0), (0, 1), (31, 33), (1000, 37), (0, 5000), (4097, 0), (1 << 15, 1 << 17)):
        ref = reference(bed, prev, n_u, n_nu)
        prev = update_and_compare(bed, ref, n_u, n_nu, f"n_u {n_u} n_nu {n_nu}")


def test_sample_order_switches(scene):
    """The uniform samples in index order (NEUS_OCC_SORT=0) and the biased ones binned by coarse cell
    (NEUS_OCC_NU_SORT=1) against the same oracle results as the default order: a quarter / quarter update and two ragged
    ones. The three testbeds therefore agree with each other. (Fresh testbeds: their density_grid_rng starts equal.)"""
    d0 = F(R.D0[0.0])
    beds = (Bed(scene), Bed(scene, NEUS_OCC_SORT="0"), Bed(scene, NEUS_OCC_NU_SORT="1"))
    bed = beds[0]
    prev = seeded_grid(8, d0)
    for b in beds:
        b.load("half_x")
        b.begin_after_step0(prev)
    for n_u, n_nu in ((Q, Q), (1000, 37), (31, 33)):
        ref = reference(bed, prev, n_u, n_nu)
        got = [update_and_compare(b, ref, n_u, n_nu, f"{tag}: n_u {n_u} n_nu {n_nu}") for b, tag in zip(beds, ("default", "unsorted", "nu sorted"))]
        prev = got[0]


def test_width_16_config(bed_w16):
    """(1 level, width 16): the kernel's half-tile branches. One exclusive pass and one quarter / quarter update."""
    d0 = F(R.D0[0.0])
    b = bed_w16
    b.load("slab_z")
    b.begin_at_step0()
    ref = run(b, np.zeros(G3, F), G3, 0, "exclusive")
    d = R.to_dense(ref["grid"]) > 0
    assert not d[:, :, :63].any() and not d[:, :, 65:].any() and 300 < d.sum() < 1800
    b.load("octant")
    prev = seeded_grid(9, d0)
    b.begin_after_step0(prev)
    run(b, prev, Q, Q, "quarter")
