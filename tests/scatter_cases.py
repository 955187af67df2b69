"""Input sets and the per-entry error bound of the grid-gradient scatter tests: shared by the CPU test of the record
format's emulation (test_oracle.py) and the device test (test_gpu_scatter_exact.py), so the bound is shown to hold for
the reference's own rounding model on exactly the inputs the device is then held to.

A case is one n_cap-sample call of the scatter on base.json's grid (L = 14): positions x [n_cap, 3], dL/denc and the
second-order operand genc [n_cap, 2L] (fp16), v [n_cap, 3] (fp32), the device-side sample count n_valid and the valid
level. Operands past n_valid are large finite garbage that must not reach the result. n_cap 16384 is 32 chunks of 512
samples, 4096 is 8: fewer than the 32 parts a level-0 / level-1 bucket is split over, so parts get an empty slice.

Domain of the bound: every record (a run-summed corner contribution) |a| < 2^15 and every per-entry sum < 2^25 (the int64
headroom); max_record of the oracle is asserted against the first where the references are made."""
import functools

import numpy as np

L = 14
BIG, SMALL = 16384, 4096
SENTINEL = np.float32(-123.456)
# test_network_forward_outside_unit_cube's points: negative cells, cells past the resolution, both far outside
OUTSIDE = np.float32([[-1e-3, 0.5, 0.5], [1.0, 1.0, 1.0], [-2.5, 3.0, 0.2], [0.5, -0.75, 1.9],
                      [1.0 - 1e-7, 0.0, 0.0], [0.0, 0.0, 0.0], [7.0, -7.0, 0.5], [0.25, 0.5, -1e-6]])


def _pos_mixed(rng, n):
    """Uniform samples; ray-like runs (32 consecutive samples 0.02 / 31 apart: the wave run merge at the coarse levels);
    64 identical positions from a multiple of 64 (a whole wave on one entry, runs across the 16-lane rows) and 200
    identical positions from lane 40 of a wave (a run across wave boundaries)."""
    x = rng.uniform(0.02, 0.98, (n, 3))
    q = n // 4
    x[q:2 * q] = np.repeat(rng.uniform(0.1, 0.9, (q // 32, 3)), 32, axis=0) + np.tile(np.linspace(0, 0.02, 32), q // 32)[:, None]
    x[2 * q:2 * q + 64] = rng.uniform(0.1, 0.9, 3)
    x[2 * q + 168:2 * q + 368] = rng.uniform(0.1, 0.9, 3)
    return x.astype(np.float32)


def _pos_outside(rng, n):
    x = rng.uniform(-0.4, 1.4, (n, 3)).astype(np.float32)
    x[:8] = OUTSIDE
    return x


def _pos_one(rng, n):
    return np.tile(rng.uniform(0.1, 0.9, 3).astype(np.float32), (n, 1))


def _case(name, n_cap, pos, seed, sigma=1e-2, sigma1=None, v_sigma=1e-3, spikes=False, first=True, second=True, n_valid=None,
          valid_level=L - 1):
    """dLdenc and genc ~ N(0, sigma) (feature 1: sigma1 if given), rounded to fp16; v ~ N(0, v_sigma)."""
    rng = np.random.default_rng(seed)
    n_valid = n_cap if n_valid is None else n_valid
    x = pos(rng, n_cap)
    sig = np.full(2 * L, sigma)
    if sigma1 is not None:
        sig[1::2] = sigma1
    dl = rng.normal(0, 1, (n_cap, 2 * L)) * sig
    g = rng.normal(0, 1, (n_cap, 2 * L)) * sig
    v = rng.normal(0, v_sigma, (n_cap, 3))
    if spikes:  # |a| in [2^10, 2^15): scale exponents 0 .. 4; on the uniform samples (no runs), first order only
        i, c = rng.integers(0, n_cap // 4, 48), rng.integers(0, 2 * L, 48)
        dl[i, c] = rng.choice([-2000.0, 2000.0], 48)
        # and k = 0: a vertex of level 0 (scale 15), where one corner's weight is ~1 and |a| ~ 30000
        x[5] = np.float32(2.5 / 15)
        dl[5, :2] = [30000.0, -29000.0]
    if not first:
        dl[:] = 0
    if not second:
        g[:] = 0
        v[:] = 0
    dl, g, v = dl.astype(np.float16), g.astype(np.float16), v.astype(np.float32)
    x[n_valid:] = 1e6
    dl[n_valid:] = 60000.0
    g[n_valid:] = -60000.0
    v[n_valid:] = 1e30
    return dict(name=name, n_cap=n_cap, n_valid=n_valid, valid_level=valid_level, x=x, dl=dl, g=g, v=v)


BENCH = 1e-2 * 2.0 ** -11  # the bench shape's loss scale 128 / R = 2^-11 on the unit-scale operands
_CASES = {
    # operand scales, mixed positions, every level, 32 chunks
    "unit": lambda: _case("unit", BIG, _pos_mixed, 1),
    "bench_scale": lambda: _case("bench_scale", BIG, _pos_mixed, 2, sigma=BENCH),
    # contributions down to the k = 31 clamp and to fp16-subnormal records
    "tiny": lambda: _case("tiny", BIG, _pos_mixed, 3, sigma=2.0 ** -20, v_sigma=1e-6),
    "large": lambda: _case("large", BIG, _pos_mixed, 4, sigma=30.0, spikes=True),
    # the pair shares one scale: feature 1 sits 2^20 below feature 0
    "pair_2p20": lambda: _case("pair_2p20", BIG, _pos_mixed, 5, sigma=1.0, sigma1=2.0 ** -20),
    "outside_cube": lambda: _case("outside_cube", BIG, _pos_outside, 6),
    # every sample on one cell: the split buckets' heaviest load (16384 x |a| < 2^25 at sigma = 8)
    "one_point": lambda: _case("one_point", BIG, _pos_one, 7, sigma=8.0),
    "partial_10000": lambda: _case("partial_10000", BIG, _pos_mixed, 8, sigma=BENCH, n_valid=10000),
    "level_3": lambda: _case("level_3", BIG, _pos_mixed, 9, valid_level=3),
    # 8 chunks: fewer than the 32 parts of the level-0 and level-1 buckets
    "small_bench_scale": lambda: _case("small_bench_scale", SMALL, _pos_mixed, 10, sigma=BENCH),
    "small_first_order": lambda: _case("small_first_order", SMALL, _pos_mixed, 11, second=False),
    "small_second_order": lambda: _case("small_second_order", SMALL, _pos_mixed, 12, first=False),
    "small_zero": lambda: _case("small_zero", SMALL, _pos_mixed, 13, first=False, second=False),
    "small_one_point": lambda: _case("small_one_point", SMALL, _pos_one, 14, sigma=BENCH),
    "small_one_sample": lambda: _case("small_one_sample", SMALL, _pos_outside, 15, n_valid=1),
    "small_level_0_partial": lambda: _case("small_level_0_partial", SMALL, _pos_outside, 16, sigma=BENCH, n_valid=3000, valid_level=0),
}
NAMES = tuple(_CASES)


@functools.lru_cache(maxsize=1)
def case(name):
    """The case's inputs and its references (computed once, shared, read-only): exact / sabs / hits / emu of
    oracle.grid_scatter on the n_valid samples, the per-parameter bound, and the level offsets (entries)."""
    import oracle as O
    c = _CASES[name]()
    cfg = O.make_cfg(n_levels=L)
    nv = c["n_valid"]
    r = O.grid_scatter(cfg, c["x"][:nv], c["valid_level"], c["dl"][:nv].astype(np.float32), c["g"][:nv].astype(np.float32), c["v"][:nv])
    c.update(r)
    c["offsets"] = O.grid_tables(cfg)[0].astype(np.int64)
    c["bound"] = bound(r["exact"], r["sabs"], r["hits"])
    for k in ("x", "dl", "g", "v", "exact", "sabs", "hits", "emu", "bound"):
        c[k].setflags(write=False)
    return c


def bound(exact, sabs, hits):
    """Per grid parameter (entry e, feature f), against the exact sum (DESIGN §6 derives it from the record format):
        |g - exact| <= (2^-11 + 2^-19) S_f(e) + hits(e) 2^-38 + 2^-38 S_{1-f}(e) + 2^-24 |exact|
    2^-11 S: half an ulp of an 11-bit significand per record, a record being at most the sum of its terms' absolute
    values; 2^-19 S: the fp32 arithmetic before the record (at most 11 roundings of 2^-24: 5 in the corner's contribution,
    6 levels of the run sum); hits 2^-38: the integer rounding of a record below its pair's scale (2^-39 each, at most one
    record per hit); 2^-38 S_other: the pair's smaller value when it is fp16-subnormal under the larger one's scale;
    2^-24 |exact|: the final fp32 store."""
    S = sabs.reshape(-1, 2)
    b = (2.0 ** -11 + 2.0 ** -19) * S + (hits.astype(np.float64) * 2.0 ** -38)[:, None] + 2.0 ** -38 * S[:, ::-1] \
        + 2.0 ** -24 * np.abs(exact.reshape(-1, 2))
    return b.reshape(-1)


def level_metrics(c, got):
    """Per level up to the case's valid one: (level, max(error / bound) over the parameters with a nonzero bound, the
    number of parameters past their bound, rel-L2 of got against the exact sum or None where that is all zero)."""
    out = []
    off = c["offsets"]
    for l in range(c["valid_level"] + 1):
        a, b = 2 * off[l], 2 * off[l + 1]
        err = np.abs(got[a:b].astype(np.float64) - c["exact"][a:b])
        bd = c["bound"][a:b]
        nz = bd > 0
        ratio = float((err[nz] / bd[nz]).max()) if nz.any() else 0.0
        norm = np.linalg.norm(c["exact"][a:b])
        out.append((l, ratio, int(np.count_nonzero(err > bd)), float(np.linalg.norm(err) / norm) if norm > 0 else None))
    return out
