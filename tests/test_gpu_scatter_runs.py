"""The region scatter's shared run structure (grid.hip level_run_plan / corner_run_sums) against the binned path, bitwise.

k_scatter_bin_r forms a level's 8 corner entries without a division (corner_entries) and, when the 8 corners' head
masks of a wave are equal, works out the wave's run structure once for all 16 partial sums; when they differ it goes
through wave_run_sum per corner. The binned mode (k_scatter_hist / k_scatter_bin) still computes grid_index and
wave_run_sum per corner: the independent implementation. Both must give the same grid gradient, bit for bit, on waves
built to hit every shape of run: a whole wave in one finest cell, runs ending on the 16-lane row boundaries, a run across
three rows, no run at all, alternating cells, outside-cube positions (the dense levels' wrap), a run cut by the device
side sample count, and adjacent lanes of different cells that collide on one corner's entry only (the mixed-mask
fall-back)."""
import ctypes as C
import functools

import numpy as np
import pytest

import scatter_cases as SC
from gpu_util import dev, ptr, scatter_testbed

pytestmark = pytest.mark.gpu

N_CAP = 1024
FINEST = SC.L - 1


@functools.lru_cache(maxsize=1)
def _tables():
    import oracle as O
    off, res, scale, _ = O.grid_tables(O.make_cfg(n_levels=SC.L))
    return off.astype(np.int64), res.astype(np.int64), scale.astype(np.float32)


def _cells(x, scale):
    """Cell of each position on a level: floor(fmaf(x, scale, 0.5)), the product exact in float64 (test_oracle.py)."""
    p = (np.asarray(x, np.float32).astype(np.float64) * np.float64(scale) + 0.5).astype(np.float32)
    return np.floor(p).astype(np.int64)


def _index(hs, res, c):
    """grid_index (grid.h:118-153) of integer corner coordinates c [..., 3], as test_oracle.py's numpy restatement."""
    c = (np.asarray(c, np.int64) & 0xFFFFFFFF).astype(np.uint32)
    stride, index, dims = 1, np.zeros(c.shape[:-1], np.uint32), 0
    while dims < 3 and stride <= hs:
        index = index + c[..., dims] * np.uint32(stride & 0xFFFFFFFF)
        stride *= int(res)
        dims += 1
    if hs < stride:
        index = c[..., 0] ^ (c[..., 1] * np.uint32(2654435761)) ^ (c[..., 2] * np.uint32(805459861))
    return index % np.uint32(hs)


CORNERS = np.array([[(i >> d) & 1 for d in range(3)] for i in range(8)], np.int64)


def _at(cell, scale, frac=0.3):
    """A position well inside `cell` of the level with this scale: fmaf(x, scale, 0.5) = cell + 0.5 + frac."""
    return ((np.asarray(cell, np.float64) + frac) / np.float64(scale)).astype(np.float32)


@functools.lru_cache(maxsize=1)
def _collision_pairs(n_pairs):
    """Pairs of different in-cube cells of the finest (hashed) level that meet on one corner's entry and not on all eight:
    B = (xb, yb, zb) with yb, zb drawn at random and xb chosen so that corner 0 of A and of B hash alike (possible when
    the two (y, z) hash terms agree in the entry's bits above the 11 of an x coordinate: one draw in 256)."""
    off, res, scale = _tables()
    hs, r = int(off[FINEST + 1] - off[FINEST]), int(res[FINEST])
    assert r ** 3 > hs and hs & (hs - 1) == 0  # a hashed level
    pairs = []
    rng = np.random.default_rng(77)
    yz = lambda y, z: (int(y) * 2654435761) ^ (int(z) * 805459861)
    for _ in range(200000):
        a, b = rng.integers(1, r - 2, 3), rng.integers(1, r - 2, 3)
        b[0] = (int(a[0]) ^ yz(a[1], a[2]) ^ yz(b[1], b[2])) & (hs - 1)
        if not 0 <= b[0] <= r - 2 or np.all(a == b):
            continue
        same = _index(hs, r, a + CORNERS) == _index(hs, r, b + CORNERS)
        if same[0] and not same.all():
            pairs.append((a, b))
            if len(pairs) == n_pairs:
                break
    return pairs, scale[FINEST]


def _positions(collide=True):
    """16 waves of 64 positions (see the module docstring); the cells named are finest-level cells."""
    _, res, scale = _tables()
    s13 = scale[FINEST]
    rng = np.random.default_rng(31)
    x = rng.uniform(0.02, 0.98, (N_CAP, 3)).astype(np.float32)
    cell = lambda: rng.integers(8, int(res[FINEST]) - 8, 3)
    w = lambda k: slice(64 * k, 64 * k + 64)
    # wave 0: all 64 lanes in one finest-level cell (jittered inside it)
    x[w(0)] = _at(cell() + rng.uniform(-0.15, 0.15, (64, 3)), s13)
    # wave 1: runs ending on lanes 15/16, 31/32, 47/48
    x[w(1)] = np.repeat(np.stack([_at(cell(), s13) for _ in range(4)]), 16, axis=0)
    # wave 2: one run over lanes 10..53, single lanes around it
    x[64 * 2 + 10:64 * 2 + 54] = _at(cell(), s13)
    # wave 3: no two adjacent lanes in one cell at any level (steps of 0.13 > 1 / 15, the coarsest cell)
    k = np.arange(64)
    x[w(3)] = np.stack([0.1 + 0.13 * (k % 6), 0.1 + 0.13 * ((k // 6) % 6), 0.1 + 0.13 * (k // 36)], axis=1).astype(np.float32)
    # wave 4: cells alternating A B A B
    ab = np.stack([_at(cell(), s13), _at(cell(), s13)])
    x[w(4)] = ab[k % 2]
    # wave 5: positions outside the unit cube (-0.3 and 1.7) beside in-cube ones, in runs of 8 and singly
    out = np.float32([[-0.3, 0.5, 0.5], [1.7, 1.7, -0.3], [0.4, -0.3, 1.7], [1.7, 0.2, 0.6]])
    inside = rng.uniform(0.1, 0.9, (4, 3)).astype(np.float32)
    x[w(5)] = np.concatenate([np.repeat(np.stack([out[j], inside[j]]), 4, axis=0) for j in range(4)]
                             + [np.stack([out[j % 4], inside[j % 4]])[[0, 1]] for j in range(16)])
    # wave 6: ray-like samples (runs on the coarse levels that break up on the fine ones), two rays of 32
    t = np.linspace(0, 0.02, 32)[:, None].astype(np.float32)
    x[w(6)] = np.concatenate([rng.uniform(0.1, 0.9, 3).astype(np.float32) + t, rng.uniform(0.1, 0.9, 3).astype(np.float32) + t * [1, -1, 0.5]])
    # wave 7: lanes 2k / 2k + 1 on two cells that collide on one corner's entry of the finest level only
    if collide:
        pairs, _ = _collision_pairs(32)
        x[w(7)] = np.concatenate([np.stack([_at(a, s13), _at(b, s13)]) for a, b in pairs])
    # wave 15: a run from lane 16 to the end of the batch: it ends on the last valid lane when n_valid = 1000
    x[64 * 15 + 16:] = _at(cell(), s13)
    return x


def _case(n_valid, valid_level):
    rng = np.random.default_rng(1000 + 16 * valid_level + (n_valid != N_CAP))
    x = _positions()
    dl = (rng.normal(0, 1, (N_CAP, 2 * SC.L)) * SC.BENCH).astype(np.float16)
    g = (rng.normal(0, 1, (N_CAP, 2 * SC.L)) * SC.BENCH).astype(np.float16)
    v = rng.normal(0, 1e-3, (N_CAP, 3)).astype(np.float32)
    x[n_valid:] = 1e6  # past the device-side count: large finite garbage that must not reach the result
    dl[n_valid:] = 60000.0
    g[n_valid:] = -60000.0
    v[n_valid:] = 1e30
    return dict(x=x, dl=dl, g=g, v=v, n_valid=n_valid, valid_level=valid_level)


@pytest.fixture(scope="module")
def beds(torch_cuda):
    from neus2_amd import scenes
    sc = scenes.small_scene(n_views=8, width=64, height=48)
    made = {}

    def get(mode):
        if mode not in made:
            made[mode] = scatter_testbed(sc, mode, N_CAP)
        return made[mode]
    return get


def _run(t, tb, c):
    from neus2_amd._lib import check, lib
    n_grid = tb.layout()["n_grid_params"]
    assert tb.layout()["n_levels"] == SC.L
    out = t.from_numpy(np.full(n_grid, SC.SENTINEL, np.float32)).cuda()
    pair = lambda a: np.ascontiguousarray(a.reshape(N_CAP, SC.L, 2).transpose(1, 0, 2))  # [n][2L] -> [L][n] half2
    v4 = np.zeros((N_CAP, 4), np.float32)
    v4[:, :3] = c["v"]
    nv = C.c_uint32(c["n_valid"])
    x, dl, g, v = dev(t, c["x"]), dev(t, pair(c["dl"])), dev(t, pair(c["g"])), dev(t, v4)
    t.cuda.synchronize()
    check(lib().neus_debug_grid_scatter(tb.handle, None, C.c_uint32(N_CAP), C.byref(nv) if c["n_valid"] != N_CAP else None, ptr(x),
                                        C.c_uint32(3), C.c_uint32(c["valid_level"]), ptr(dl), ptr(g), ptr(v), ptr(out)))
    t.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32)


def _assert_modes_equal(t, beds, c):
    off, _, _ = _tables()
    end = 2 * int(off[c["valid_level"] + 1])
    want = _run(t, beds("binned"), c)
    assert np.any(want[:end] != SC.SENTINEL.view(np.uint32)) and np.any(want[:end])  # the binned path wrote a gradient
    for mode in ("regions", "regions1024"):
        got = _run(t, beds(mode), c)
        np.testing.assert_array_equal(got[:end], want[:end], err_msg=f"{mode} against binned")


def test_case_set_holds_its_patterns():
    """The positions are what the docstring says, by the CPU index formula (no device)."""
    off, res, scale = _tables()
    x = _positions()
    cells = [_cells(x, scale[l]) for l in range(SC.L)]
    fin = cells[FINEST]
    same = lambda a, b, l=FINEST: bool(np.all(cells[l][a] == cells[l][b]))
    assert all(same(0, k) for k in range(64))
    for k in (15, 31, 47):
        assert same(64 + k - 1, 64 + k) and not same(64 + k, 64 + k + 1)
    assert all(same(128 + 10, 128 + k) for k in range(10, 54)) and not same(128 + 9, 128 + 10) and not same(128 + 53, 128 + 54)
    assert not any(same(192 + k, 192 + k + 1, l) for k in range(63) for l in range(SC.L))
    assert all(same(256 + k, 256 + k + 2) and not same(256 + k, 256 + k + 1) for k in range(62))
    assert np.any(fin[320:384] < 0) and np.any(fin[320:384] >= res[FINEST]) and np.any((fin[320:384] >= 0).all(axis=1))
    assert all(same(960 + 16, k) for k in range(960 + 16, 1024))


@pytest.mark.parametrize("valid_level", (13, 3, 0))
@pytest.mark.parametrize("n_valid", (N_CAP, 1000))
def test_region_modes_match_binned_bitwise(beds, torch_cuda, n_valid, valid_level):
    """regions (512-sample workgroups) and regions1024 against binned: every parameter of every level up to the valid one."""
    _assert_modes_equal(torch_cuda, beds, _case(n_valid, valid_level))


def test_mixed_head_masks_fall_back(beds, torch_cuda):
    """4a. Lanes 2k and 2k + 1 of wave 7 sit in two different in-cube cells of hashed level 13 whose corner 0 shares an entry
    while other corners do not: the corners' head masks differ in that wave, so the level goes through wave_run_sum per
    corner. The precondition is asserted on the CPU first; then the same bitwise equality."""
    off, res, scale = _tables()
    hs, r = int(off[FINEST + 1] - off[FINEST]), int(res[FINEST])
    c = _case(N_CAP, FINEST)
    cells = _cells(c["x"][64 * 7:64 * 8], scale[FINEST])
    a, b = cells[0::2], cells[1::2]
    assert np.all((a >= 0) & (a < r - 1) & (b >= 0) & (b < r - 1)), "cells inside the cube"
    assert np.all(np.any(a != b, axis=1)), "different cells"
    same = _index(hs, r, a[:, None, :] + CORNERS) == _index(hs, r, b[:, None, :] + CORNERS)  # [pair, corner]
    assert np.all(same.any(axis=1) & ~same.all(axis=1)), "each pair meets on one corner's entry and not on all eight"
    _assert_modes_equal(torch_cuda, beds, c)


def test_generic_binning_kernel_matches_direct(beds, torch_cuda):
    """The generic k_scatter_bin_r (grid_index, wave_run_sum per corner: what a level table that is neither dense nor a
    power of two gets), forced by the test hook, against the direct form on the same testbed: bitwise, whole case set."""
    from neus2_amd._lib import check, lib
    c = _case(1000, FINEST)
    for mode in ("regions", "regions1024"):
        direct = _run(torch_cuda, beds(mode), c)
        check(lib().neus_debug_set_grid_generic(C.c_uint32(1)))
        try:
            generic = _run(torch_cuda, beds(mode), c)
        finally:
            check(lib().neus_debug_set_grid_generic(C.c_uint32(0)))
        np.testing.assert_array_equal(generic, direct, err_msg=mode)
