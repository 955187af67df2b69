"""The chain grid -> mean -> bitfield -> seven pooled mips -> the march's linear words -> the ray generation's cull box,
byte for byte against the plain references of tests/occ_ref.py, without a network in the way.

set_density_grid(grid) + neus_testbed_restore_state(rebuild_bitfield = 1) runs k_grid_mean_partial / k_grid_mean_final,
k_grid_to_bitfield, k_bitfield_pool_all (without the linear words), k_bitfield_linear and k_occ_bbox_partial / _final on
the testbed's own buffers; set_density_grid(bitfield = ...) runs the last two on a caller's field. Read back: the grid and
all 8 mips (get_density_grid), and bf_lin, occ_bbox and grid_mean through neus_debug_get_buffer. Before every rebuild the
device's field is filled with ones, so a byte the rebuild does not write shows.

No tolerance anywhere: the mean is compared with the device's summation order restated in float32, the box with the
float32 formula (its one rounding is the pad's add)."""
import ctypes as C
import os

import numpy as np
import pytest

import occ_ref as R
from gpu_util import occ_buffer

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
CORNERS, INNER_CORNERS = R.CORNERS, R.INNER_CORNERS


@pytest.fixture(scope="module")
def tb(torch_cuda):
    from neus2_amd import pyngp, scenes
    sc = scenes.small_scene(n_views=4, width=64, height=48)
    t = pyngp.Testbed(pyngp.TestbedMode.Nerf)
    t.set_dataset(sc["images"], sc["focal"], sc["principal"], sc["xforms"], 1)
    t.reload_network_from_file(os.path.join(ROOT, "configs", "nerf", "base.json"), batch_size=4096)
    return t


def _dense(cells=(), value=1.0):
    d = np.zeros((R.G,) * 3, F)
    for c in cells:
        d[c] = value
    return d


def _rebuild(tb, grid):
    from neus2_amd._lib import NeusRestoreState, check, lib
    tb.set_density_grid(bitfield=np.full(R.NBYTES * R.N_MIPS, 0xff, np.uint8))
    tb.set_density_grid(grid)
    st = NeusRestoreState(1, 4096, 0, 0, 0.0, 1)
    check(lib().neus_testbed_restore_state(tb.handle, C.byref(st)))


def _assert_products(tb, want, tag=""):
    _, bf = tb.get_density_grid()
    bf, wbf = bf.reshape(R.N_MIPS, R.NBYTES), want["bitfield"].reshape(R.N_MIPS, R.NBYTES)
    for m in range(R.N_MIPS):
        np.testing.assert_array_equal(bf[m], wbf[m], err_msg=f"{tag}: mip {m}")
    np.testing.assert_array_equal(occ_buffer(tb, "lin"), want["lin"], err_msg=f"{tag}: linear words")
    np.testing.assert_array_equal(occ_buffer(tb, "bbox").view(np.uint32), want["bbox"].view(np.uint32), err_msg=f"{tag}: box {want['bbox']}")


def _check_grid(tb, grid, tag=""):
    """Rebuilds the field from grid (device order) and compares everything; -> the reference's products."""
    grid = np.ascontiguousarray(grid, F)
    want = R.expected_build(grid)
    _rebuild(tb, grid)
    g, _ = tb.get_density_grid()
    np.testing.assert_array_equal(g.view(np.uint32), grid.view(np.uint32), err_msg=f"{tag}: the rebuild changed the grid")
    got_mean = occ_buffer(tb, "mean")
    assert got_mean.view(np.uint32)[0] == np.array([want["mean"]], F).view(np.uint32)[0], (tag, got_mean[0], want["mean"])
    _assert_products(tb, want, tag)
    return want


def test_empty_grids(tb):
    """All zero, and all negative ("never trained"): the mean and so the threshold are 0, no cell passes the strict
    comparison, every mip is empty and the box is the empty box."""
    for g in (np.zeros(R.G3, F), np.full(R.G3, -1.0, F)):
        want = _check_grid(tb, g)
        assert want["mean"] == 0 and not want["bitfield"].any() and not want["lin"].any()
        np.testing.assert_array_equal(want["bbox"], F([R.FLT_MAX] * 3 + [-R.FLT_MAX] * 3))


def test_full_grid(tb):
    want = _check_grid(tb, np.ones(R.G3, F))
    assert want["mean"] == 1 and np.all(want["bitfield"][:R.NBYTES] == 0xff) and np.all(want["lin"] == 0xffffffff)
    # mip m holds the cells 64 + ((c - 64) >> m) of c = 0 .. 127 per axis: 128 >> m of them, and the two cells either side
    # of the centre at mip 7
    for m in range(1, R.N_MIPS):
        side = (64 + (63 >> m)) - (64 + (-64 >> m)) + 1
        assert side == max(128 >> m, 2)
        assert np.unpackbits(want["bitfield"][m * R.NBYTES:(m + 1) * R.NBYTES]).sum() == side ** 3


@pytest.mark.parametrize("cell", CORNERS + INNER_CORNERS, ids=lambda c: "_".join(map(str, c)))
def test_single_cell_climbs_every_mip(tb, cell):
    """One occupied cell: its bit climbs the seven mips alone, after the first pool through the sub-word ORs. (The 16 cells
    put the byte that is written at every offset 0..3 of its 32-bit word at some mip: tests/test_occ_ref.py.)"""
    want = _check_grid(tb, R.from_dense(_dense([cell])), str(cell))
    bf = want["bitfield"].reshape(R.N_MIPS, R.NBYTES)
    assert all(np.unpackbits(bf[m]).sum() == 1 for m in range(R.N_MIPS))
    assert want["mean"] == F(2.0 ** -21)


def test_all_corner_cells_at_once(tb):
    _check_grid(tb, R.from_dense(_dense(CORNERS + INNER_CORNERS)))


def test_one_cell_per_wave_in_its_last_byte(tb):
    """One cell in every 8x8x8 block (the 64 bytes one wave of the pool reads), in the block's last byte: the ballot's top
    lane and the last of the 8 parent bytes, for every wave of mip 0."""
    d = np.zeros((R.G,) * 3, F)
    d[7::8, 7::8, 6::8] = 1.0
    g = R.from_dense(d)
    by = np.flatnonzero(np.packbits(g > 0, bitorder="little"))
    assert len(by) == 16 ** 3 and np.all(by % 64 == 63)
    _check_grid(tb, g)


def test_one_cell_in_three_percent_of_the_4x4x4_blocks(tb):
    rng = np.random.default_rng(41)
    d = np.zeros((32, 4, 32, 4, 32, 4), F)
    blocks = np.argwhere(rng.random((32, 32, 32)) < 0.03)
    off = rng.integers(0, 4, (len(blocks), 3))
    d[blocks[:, 0], off[:, 0], blocks[:, 1], off[:, 1], blocks[:, 2], off[:, 2]] = 1.0
    _check_grid(tb, R.from_dense(d.reshape((R.G,) * 3)))


@pytest.mark.parametrize("frac", [1e-4, 0.01, 0.5])
def test_random_occupancy(tb, frac):
    """At a half, most waves of every level race for the same parent bytes; at 1e-4 most bits climb alone."""
    d = (np.random.default_rng(int(frac * 1e6)).random((R.G,) * 3) < frac).astype(F)
    want = _check_grid(tb, R.from_dense(d), f"{frac}")
    assert (want["mean"] >= 0.1) == (frac >= 0.1)


def test_thin_shell(tb):
    from neus2_amd import scenes
    occ = R.unpack(scenes.shell_bitfield()[:R.NBYTES])
    want = _check_grid(tb, R.from_dense(occ.astype(F) * F(0.75)))
    np.testing.assert_array_equal(want["bitfield"], scenes.shell_bitfield())


def test_threshold_at_a_tenth(tb):
    """Mean >= 0.1: the threshold is float32(0.1). Cells at it and one ulp below are empty, one ulp above occupied."""
    rng = np.random.default_rng(6)
    t = F(0.1)
    below, above = np.nextafter(t, F(0)), np.nextafter(t, F(1))
    g = (rng.random(R.G3) < 0.5).astype(F)
    free = np.flatnonzero(g == 0)
    pick = rng.choice(free, 3000, replace=False)
    g[pick[:1000]], g[pick[1000:2000]], g[pick[2000:]] = t, below, above
    want = _check_grid(tb, g)
    assert want["mean"] >= 0.1
    bits = np.unpackbits(want["bitfield"][:R.NBYTES], bitorder="little")
    assert not bits[pick[:2000]].any() and bits[pick[2000:]].all()


def test_threshold_at_the_mean_on_an_order_free_grid(tb):
    """Mean < 0.1: the threshold is the mean. 8192 - k cells of 1.0 and 256 k of 2^-8 sum exactly in any order, the mean
    is 2^-8 whatever the tree: the 2^-8 cells are on the threshold and read empty. Then four of them go one ulp up and
    four one ulp down: each such term loses its last bit in the first add that meets another term (a tie, rounded to the
    even multiple of 2^-29), so the mean stays 2^-8 - asserted on the restated order - and the raised cells alone read
    occupied."""
    g, cells = R.order_free_grid()
    k1 = 8192 - 37
    want = _check_grid(tb, g, "exact")
    assert want["mean"] == F(2.0 ** -8)
    bits = np.unpackbits(want["bitfield"][:R.NBYTES], bitorder="little")
    assert bits.sum() == k1 and bits[cells[:k1]].all()
    m = F(2.0 ** -8)
    up, down = cells[k1:k1 + 4], cells[k1 + 4:k1 + 8]
    g[up], g[down] = np.nextafter(m, F(1)), np.nextafter(m, F(0))
    want = _check_grid(tb, g, "one ulp")
    assert want["mean"] == m
    bits = np.unpackbits(want["bitfield"][:R.NBYTES], bitorder="little")
    assert bits.sum() == k1 + 4 and bits[up].all() and not bits[down].any()


def test_negative_cells_beside_occupied_ones(tb):
    """Negative cells are never occupied and count 0 in the mean, also where they share a byte with occupied cells."""
    rng = np.random.default_rng(12)
    d = (rng.random((R.G,) * 3) < 0.02).astype(F)
    neg = (np.roll(d, 1, 0) + np.roll(d, 1, 1) + np.roll(d, -1, 2) > 0) & (d == 0)
    d[neg] = -4.0
    g = R.from_dense(d)
    want = _check_grid(tb, g)
    assert want["mean"] == R.device_mean(np.maximum(g, 0)) and want["mean"] < 0.1
    np.testing.assert_array_equal(np.unpackbits(want["bitfield"][:R.NBYTES], bitorder="little"), g > 0)


@pytest.mark.parametrize("kind", ["uniform", "exponential", "normal"])
def test_dense_random_float_grids(tb, kind):
    """Every cell a different float. "uniform": mean 0.5, threshold 0.1. "exponential" and "normal" (a third of the cells
    negative): the threshold is the mean itself, which only the restated summation order reproduces to the bit."""
    rng = np.random.default_rng(77)
    g = {"uniform": lambda: rng.random(R.G3, dtype=F), "exponential": lambda: rng.exponential(0.02, R.G3).astype(F),
         "normal": lambda: rng.normal(0.02, 0.05, R.G3).astype(F)}[kind]()
    want = _check_grid(tb, g, kind)
    assert (want["mean"] >= 0.1) == (kind == "uniform")


def _check_bitfield(tb, bf, tag=""):
    bf = np.ascontiguousarray(bf, np.uint8)
    tb.set_density_grid(bitfield=bf)
    want = dict(bitfield=bf, **R.expected_from_bitfield(bf))
    _assert_products(tb, want, tag)
    return want


@pytest.mark.parametrize("mip,cell", [(3, (0, 0, 0)), (3, (127, 0, 127)), (7, (0, 127, 0)), (7, (127, 127, 127))])
def test_user_bitfield_single_bit(tb, mip, cell):
    """A caller's field (snapshots, teacher-forced tests) may hold bits no pool would give: one bit at a corner of a coarse
    mip. The linear words follow mip 0 (empty), the box follows the bit: out to 0.5 +- 64 and the pad at mip 7."""
    mips = [np.zeros((R.G,) * 3, bool) for _ in range(R.N_MIPS)]
    mips[mip][cell] = True
    want = _check_bitfield(tb, R.pack_mips(mips), f"mip {mip} {cell}")
    assert not want["lin"].any()
    sc = F(2 ** mip)
    for d in range(3):
        assert want["bbox"][d] == (F(0.5) + (F(cell[d]) / F(128) - F(0.5)) * sc) - F(1e-4) * sc
        assert want["bbox"][3 + d] == (F(0.5) + (F(cell[d] + 1) / F(128) - F(0.5)) * sc) + F(1e-4) * sc


def test_user_bitfield_random_bits_in_every_mip(tb):
    rng = np.random.default_rng(90)
    bf = np.packbits(rng.random(R.G3 * R.N_MIPS) < 1e-4, bitorder="little")
    want = _check_bitfield(tb, bf)
    assert want["lin"].any() and want["bbox"][0] < -60 and want["bbox"][5] > 60
    # and back to a field of its own making: the user's coarse bits are gone
    _check_grid(tb, R.from_dense(_dense([(3, 4, 5)])))
