"""The hash-grid gradient scatter (grid.hip) and the variance gradient's batch sum (mlp.hip) against exact references.

The scatter runs alone through neus_debug_grid_scatter on caller-given operands and is compared, entry by entry, with the
oracle's exact float64 sum (oracle.grid_scatter) under the error bound its record format implies (scatter_cases.bound,
derived in DESIGN §6 from the format alone: fp16 records with a per-record power-of-two scale, summed in 2^-38 fixed
point): at unit operand scale, at the bench loss scale 2^-11, down to the k = 31 clamp and up to k = 0, with feature
pairs 2^20 apart, outside the unit cube, with whole waves and 200 samples on one entry, every sample on one cell, a
device-side sample count below the capacity, fewer sample chunks (8) than the parts (32) of a level-0 bucket, and valid
levels 13, 3 and 0. The same inputs pass through the CPU emulation of the format in tests/test_oracle.py, which shows the
bound is not too tight without a device."""
import ctypes as C

import numpy as np
import pytest

import scatter_cases as SC
from gpu_util import dev, ptr, scatter_testbed
from test_gpu_parity import record

pytestmark = pytest.mark.gpu

# The device against the emulation, per level: the two differ only in the order of the fp32 run sum and in FMA
# contraction of a0 = dl * wc + g * w2. Either moves a record's fp32 value by a few fp32 ulps (2^-24 relative) and so flips
# an fp16 rounding only where the value sits within that distance of a rounding boundary - where the rounding error is
# half an fp16 ulp either way. The error norms can therefore differ by about 2^-24 / 2^-12 relative; 1.5 leaves room for a
# level with a handful of entries (one sample: 16 values) and still fails a scatter whose error is twice the format's.
MARGIN = 1.5
# the two cases that also compare the scatter modes bitwise (test_scatter_paths_bitwise_equal: unit scale, in-cube only)
MODE_CASES = ("bench_scale", "outside_cube")


@pytest.fixture(scope="module")
def beds(torch_cuda):
    """Testbeds by (mode, batch), made on first use: base.json (L = 14) on the small scene; the scene only makes a testbed."""
    from neus2_amd import scenes
    sc = scenes.small_scene(n_views=8, width=64, height=48)
    made = {}

    def get(mode, batch):
        if (mode, batch) not in made:
            made[(mode, batch)] = scatter_testbed(sc, mode, batch)
        return made[(mode, batch)]
    return get


def _run(t, tb, c):
    """One call of the scatter alone on case c: the grid gradient (2 x entries f32) over a sentinel-filled buffer."""
    from neus2_amd._lib import check, lib
    n_cap, L = c["n_cap"], SC.L
    n_grid = c["exact"].size
    assert tb.layout()["n_grid_params"] == n_grid and tb.layout()["n_levels"] == L
    out = t.from_numpy(np.full(n_grid, SC.SENTINEL, np.float32)).cuda()
    pair = lambda a: np.ascontiguousarray(a.reshape(n_cap, L, 2).transpose(1, 0, 2))  # [n][2L] -> [L][n] half2
    v4 = np.zeros((n_cap, 4), np.float32)
    v4[:, :3] = c["v"]
    nv = C.c_uint32(c["n_valid"])
    x, dl, g, v = dev(t, c["x"]), dev(t, pair(c["dl"])), dev(t, pair(c["g"])), dev(t, v4)
    t.cuda.synchronize()
    check(lib().neus_debug_grid_scatter(tb.handle, None, C.c_uint32(n_cap), C.byref(nv) if c["n_valid"] != n_cap else None, ptr(x),
                                        C.c_uint32(3), C.c_uint32(c["valid_level"]), ptr(dl), ptr(g), ptr(v), ptr(out)))
    t.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("name", SC.NAMES)
def test_scatter_within_record_bound(beds, torch_cuda, name):
    """Every entry of every level up to the valid one within the format's bound of the exact sum; entries without a hit
    exactly +0.0 (the sentinel gone); every level above the valid one untouched; per level the device's rel-L2 against the
    exact sum at most MARGIN x the emulation's on the same inputs (the floor is the oracle's, never the kernel's)."""
    t = torch_cuda
    c = SC.case(name)
    got = _run(t, beds("regions", c["n_cap"]), c)
    off = c["offsets"]
    end = 2 * off[c["valid_level"] + 1]
    bits = got.view(np.uint32)
    assert np.all(np.isfinite(got[:end]))
    dev_m, emu_m = SC.level_metrics(c, got), SC.level_metrics(c, c["emu"])
    for (l, ratio, n_past, rel), (_, e_ratio, _, e_rel) in zip(dev_m, emu_m):
        print(f"{name} level {l}: max err/bound {ratio:.3f} (emulation {e_ratio:.3f}), rel-L2 device {rel} emulation {e_rel}")
        record(f"scatter_exact/{name}/level{l}", max_err_over_bound=ratio, entries_past_bound=n_past,
               rel_l2_device=-1.0 if rel is None else rel, rel_l2_emulation=-1.0 if e_rel is None else e_rel)
    untouched = np.repeat(c["hits"][:end // 2] == 0, 2)
    assert not np.any(bits[:end][untouched]), "an entry without a hit is not +0.0"
    assert np.all(bits[end:] == SC.SENTINEL.view(np.uint32)), "a level above the valid one was written"
    for (l, ratio, n_past, rel), (_, _, _, e_rel) in zip(dev_m, emu_m):
        assert n_past == 0, (name, l, ratio, n_past)
        if rel is None:  # the exact sum of the level is all zero: the bound is zero there, the output exact zeros
            assert not np.any(bits[2 * off[l]:2 * off[l + 1]]), (name, l)
        else:
            assert rel <= MARGIN * e_rel, (name, l, rel, e_rel)
    if name == "small_zero":
        assert not np.any(bits[:end])
    if name in MODE_CASES:  # every level is valid in these: all modes write every entry
        assert c["valid_level"] == SC.L - 1
        for mode in ("seg", "binned"):
            other = _run(t, beds(mode, c["n_cap"]), c)
            np.testing.assert_array_equal(other.view(np.uint32), bits, err_msg=f"{name}: {mode} against regions")


def test_scatter_entry_point_rejects_oversized_call(beds, torch_cuda):
    """n_cap above the testbed's batch capacity, or n_valid above n_cap, is an error, not a launch."""
    from neus2_amd._lib import NeusError, check, lib
    t = torch_cuda
    tb = beds("regions", SC.SMALL)
    buf = t.zeros(16, dtype=t.float32, device="cuda")
    for n_cap, n_valid in ((SC.SMALL + 1, None), (SC.SMALL, SC.SMALL + 1), (0, None)):
        nv = C.c_uint32(n_valid or 0)
        with pytest.raises(NeusError):
            check(lib().neus_debug_grid_scatter(tb.handle, None, C.c_uint32(n_cap), C.byref(nv) if n_valid else None, ptr(buf), C.c_uint32(3),
                                                C.c_uint32(13), ptr(buf), ptr(buf), ptr(buf), ptr(buf)))


# ---------------------------------------------------------------- the variance gradient
# Longest chain of fp32 additions a term of the batch sum of dL/dout[7] passes through (mlp.hip k_mlp_train_rgb and
# k_mlp_grad_reduce): the lane's serial loop over its chunks - one chunk per wave at these sizes (the grid is n / 128
# workgroups of 4 waves x 32 samples while n / 128 is below the resident-block cap, >= 256 on this device) = 1; the 6-step
# shuffle tree over the wave = 6; (s0 + s1) + (s2 + s3) over the 4 wave partials = 2; thread t's strided loop over the
# block partials t, t + 256, ... (at most 32 blocks here) = 1; the 8-step tree over the 256 threads = 8.
VAR_DEPTH = 1 + 6 + 2 + 1 + 8


@pytest.mark.parametrize("n", (1024, 4096))
def test_variance_gradient_is_the_exact_column_sum(beds, torch_cuda, n):
    """neus_net_backward with a caller-given fp16 dL/dout: the variance gradient is the fp32 sum of column 7 in a fixed
    tree, so |var_grad - sum_64| <= d 2^-24 sum |dl16[:, 7]| against the float64 sum, d = VAR_DEPTH; the other three slots
    of the variance block are exactly 0. Two columns: one that cancels (pairs +/- x shuffled over the batch plus a
    remainder of 2^-10 sum |x|: a bar relative to the sum would be useless, the absolute one is sharp) and one all
    positive. Known difference, not asserted: the oracle rounds this sum to fp16 as the reference's `T gradients`
    does (nerf_network.h:461-474); the device keeps fp32, and is compared with the float64 sum here."""
    from neus2_amd._lib import check, lib
    t = torch_cuda
    tb = beds("regions", SC.SMALL)
    lay = tb.layout()
    rng = np.random.default_rng(100 + n)
    c = np.zeros((n, 7), np.float32)
    c[:, :3] = rng.uniform(0.05, 0.95, (n, 3))
    d = rng.normal(size=(n, 3))
    c[:, 4:] = (d / np.linalg.norm(d, axis=1, keepdims=True) + 1) * 0.5
    xs = np.abs(rng.normal(0, 1e-2, n // 2)).astype(np.float16).astype(np.float64)
    cancel = np.concatenate([xs, -xs])
    rem = 2.0 ** -10 * np.abs(cancel).sum()
    cancel[: n // 2] += rem / (n // 2)
    rng.shuffle(cancel)
    positive = np.abs(rng.normal(0, 1e-2, n))
    for label, col in (("cancelling", cancel), ("positive", positive)):
        dl = np.zeros((n, 16), np.float32)
        dl[:, :4] = rng.normal(0, 1e-2, (n, 4))
        dl[:, 4:7] = rng.normal(0, 1.0, (n, 3))
        dl[:, 7] = col
        dl16 = dl.astype(np.float16)
        col16 = dl16[:, 7].astype(np.float64)
        want, sabs = col16.sum(), np.abs(col16).sum()
        if label == "cancelling":
            assert abs(want) < 2.0 ** -8 * sabs  # the column cancels to about the remainder
        g = t.zeros(lay["n_params"], dtype=t.float32, device="cuda")
        check(lib().neus_net_backward(tb.handle, None, C.c_uint32(n), ptr(dev(t, c)), C.c_uint32(SC.L), ptr(dev(t, dl16)), C.c_uint32(n), ptr(g)))
        t.cuda.synchronize()
        var = g[lay["variance_offset"]:lay["variance_offset"] + 4].cpu().numpy()
        err, bar = abs(float(var[0]) - want), VAR_DEPTH * 2.0 ** -24 * sabs
        print(f"variance n={n} {label}: got {var[0]!r} want {want!r} err {err:.3e} bar {bar:.3e}")
        record(f"variance_sum/{label}/n{n}", err=err, bar=bar, sum=want, sum_abs=sabs)
        assert err <= bar, (label, n, float(var[0]), want, err, bar)
        assert not np.any(var[1:].view(np.uint32)), var
