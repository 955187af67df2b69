"""Plain references of what the occupancy update and the bitfield rebuild produce, and the step networks that make the
update's density exactly computable - TEST INFRASTRUCTURE ONLY (CPU, numpy).

Everything is stated on dense [x][y][z] arrays of the 128^3 grid. The only place the device's storage order appears is
`MORTON` (cell (x, y, z) -> its index: bit b of x, y, z at bits 3b, 3b + 1, 3b + 2), used to move between the device's
flat buffers and the dense arrays; no reference below indexes by bytes or words of the packed field.

  to_dense / from_dense    device-order flat array <-> dense [x][y][z]
  pack / unpack            dense bool mip <-> its 128^3 / 8 bytes (bit i & 7 of byte i >> 3 is cell index i)
  pool                     the next mip: 2x2x2 OR of a mip, written into the inner [32, 96)^3
  bitfield_from_grid       all 8 mips' bytes from the device-order float grid and a threshold (strict >)
  linear_words             the march's words of mip 0
  bbox                     the ray generation's cull box of an 8-mip field
  device_mean              the mean of max(grid, 0) in the device's fixed summation order
  threshold                min(0.1, mean)

The step networks (part two, `step_net`) give the density MLP one hidden layer whose units are +-2^15 on position columns:
the density of a sample is then exactly 0 (off the surface) or one constant D0 (on it), see `density_chain`."""
import numpy as np

G = 128
G3 = G ** 3
NBYTES = G3 // 8
N_MIPS = 8
MIN_OPTICAL_THICKNESS = np.float32(0.1)   # NERF_MIN_OPTICAL_THICKNESS
FLT_MAX = np.float32(3.402823466e+38)
PAD = np.float32(1e-4)
# single occupied cells of the GPU tests: the grid's corners and the corners of the inner [32, 96)^3
CORNERS = [(x, y, z) for x in (0, 127) for y in (0, 127) for z in (0, 127)]
INNER_CORNERS = [(x, y, z) for x in (32, 95) for y in (32, 95) for z in (32, 95)]


def _morton():
    i = np.arange(G, dtype=np.uint32)
    x, y, z = np.meshgrid(i, i, i, indexing="ij")
    m = np.zeros((G, G, G), np.uint32)
    for b in range(7):
        m |= (((x >> b) & 1) << (3 * b)) | (((y >> b) & 1) << (3 * b + 1)) | (((z >> b) & 1) << (3 * b + 2))
    return m


MORTON = _morton()


def to_dense(flat):
    """Device-order flat [128^3] -> dense [x][y][z]."""
    return np.asarray(flat).reshape(-1)[MORTON]


def from_dense(dense):
    """Dense [x][y][z] -> device-order flat [128^3]."""
    out = np.zeros(G3, np.asarray(dense).dtype)
    out[MORTON.reshape(-1)] = np.asarray(dense).reshape(-1)
    return out


def pack(occ):
    """Dense bool [x][y][z] -> the mip's bytes."""
    return np.packbits(from_dense(np.asarray(occ, bool)), bitorder="little")


def unpack(mip_bytes):
    """One mip's bytes -> dense bool [x][y][z]."""
    return to_dense(np.unpackbits(np.asarray(mip_bytes, np.uint8), bitorder="little").astype(bool))


def pool(occ):
    """The next mip of a dense bool mip: cell (32 + i, 32 + j, 32 + k) is the OR of the 2x2x2 block at (2i, 2j, 2k); the
    cells outside the inner [32, 96)^3 are empty."""
    o = np.asarray(occ, bool).reshape(64, 2, 64, 2, 64, 2).any(axis=(1, 3, 5))
    nxt = np.zeros((G, G, G), bool)
    nxt[32:96, 32:96, 32:96] = o
    return nxt


def mips_from_occupancy(occ):
    """The 8 dense mips of a dense bool mip 0."""
    mips = [np.asarray(occ, bool)]
    for _ in range(1, N_MIPS):
        mips.append(pool(mips[-1]))
    return mips


def pack_mips(mips):
    return np.concatenate([pack(m) for m in mips])


def unpack_mips(bitfield):
    bf = np.asarray(bitfield, np.uint8).reshape(N_MIPS, NBYTES)
    return [unpack(bf[m]) for m in range(N_MIPS)]


def threshold(mean):
    return np.minimum(MIN_OPTICAL_THICKNESS, np.float32(mean))


def bitfield_from_grid(grid_flat, thresh):
    """All 8 mips' bytes from the device-order float32 grid: mip 0 is grid > thresh (strict: a cell on the threshold, a
    zero and a negative cell are empty), the others are pooled."""
    occ = to_dense(np.asarray(grid_flat, np.float32)) > np.float32(thresh)
    return pack_mips(mips_from_occupancy(occ))


def linear_words(occ0):
    """The march's words of mip 0: word w = (ix << 9) | (iy << 2) | q holds cells (ix, iy, 32 q + b) at bit b."""
    bits = np.asarray(occ0, bool).reshape(G, G, 4, 32).astype(np.uint32)
    w = np.zeros((G, G, 4), np.uint32)
    for b in range(32):
        w |= bits[..., b] << np.uint32(b)
    return w.reshape(-1)


def bbox(mips):
    """The box of every occupied cell of every dense mip in float32: cell c of mip m covers, per axis,
    0.5 + (c / 128 - 0.5) 2^m .. 0.5 + ((c + 1) / 128 - 0.5) 2^m, padded by 1e-4 2^m. Every operation before the pad is
    exact in float32 (dyadic values below 2^7 with 7 + m fraction bits at the most), so the pad's add is the one
    rounding. An empty field gives lo = +FLT_MAX, hi = -FLT_MAX. -> float32 [6]: lo xyz, hi xyz."""
    f = np.float32
    lo, hi = np.full(3, FLT_MAX, f), np.full(3, -FLT_MAX, f)
    for m, occ in enumerate(mips):
        if not occ.any():
            continue
        sc = f(2 ** m)
        pad = PAD * sc
        for d in range(3):
            c = np.flatnonzero(occ.any(axis=tuple(a for a in range(3) if a != d))).astype(f)
            l = (f(0.5) + (c / f(G) - f(0.5)) * sc) - pad
            h = (f(0.5) + ((c + f(1)) / f(G) - f(0.5)) * sc) + pad
            lo[d] = min(lo[d], l.min())
            hi[d] = max(hi[d], h.max())
    return np.concatenate([lo, hi]).astype(f)


def _tree256(s):
    """The halving tree over the last axis (256 wide): s[t] += s[t + off] for off = 128, 64 .. 1; -> s[..., 0]."""
    s = s.copy()
    off = 128
    while off:
        s[..., :off] = s[..., :off] + s[..., off:2 * off]
        off >>= 1
    return s[..., 0]


def device_mean(grid_flat):
    """mean(max(grid, 0)) of cascade 0 in the device's order, float32 throughout: every cell divided by 128^3; block b of
    2048 takes cells 1024 b + 256 k + t, thread t adds its four (k = 0..3) in turn, a 256-wide halving tree gives the
    block's partial; the final block's thread t adds partials t + 256 k (k = 0..7) in turn, then the same tree."""
    f = np.float32
    v = np.maximum(np.asarray(grid_flat, f).reshape(-1)[:G3], f(0)) / f(G3)
    v = v.reshape(G3 // 1024, 4, 256)
    acc = np.zeros((G3 // 1024, 256), f)
    for k in range(4):
        acc = acc + v[:, k]
    partial = _tree256(acc)
    p = partial.reshape(8, 256)
    acc = np.zeros(256, f)
    for k in range(8):
        acc = acc + p[k]
    return f(_tree256(acc))


def mean_bound(grid_flat):
    """A bound of |device_mean - exact mean|: 4 + 8 + 3 + 8 = 23 float32 additions deep at the most, each within 2^-24
    relative of a partial sum that is at most the sum of the (non-negative) terms: 23 2^-24 mean, doubled for slack."""
    g = np.maximum(np.asarray(grid_flat, np.float64), 0)
    return 2 * 23 * 2.0 ** -24 * g.mean()


def order_free_grid(k=37, seed=5):
    """8192 - k cells of 1.0 and 256 k cells of 2^-8 at random places, the rest 0: the mean is exactly 2^-8, and so is
    every partial sum of it in any order (multiples of 2^-29 up to 2^-8 are float32 values). -> (grid, the permutation
    of the cells: the first 8192 - k are the 1.0 cells, the next 256 k the 2^-8 cells, the rest empty)."""
    rng = np.random.default_rng(seed)
    cells = rng.permutation(G3)
    g = np.zeros(G3, np.float32)
    g[cells[:8192 - k]] = 1.0
    g[cells[8192 - k:8192 - k + 256 * k]] = 2.0 ** -8
    return g, cells


def expected_build(grid_flat):
    """What the rebuild of the field from a grid must give: dict(mean, bitfield, lin, bbox)."""
    mean = device_mean(grid_flat)
    bf = bitfield_from_grid(grid_flat, threshold(mean))
    return dict(mean=mean, bitfield=bf, **expected_from_bitfield(bf))


def expected_from_bitfield(bitfield):
    mips = unpack_mips(bitfield)
    return dict(lin=linear_words(mips[0]), bbox=bbox(mips))


# ------------------------------------------------------------------------------------------------------------------
# Step networks: density MLPs with one hidden layer whose density is exactly 0 or D0.
#
#   din_c = h(h(x_c) - 0.5)  (c = 0, 1, 2; every other density input is 0 on a zero hash table)
#   H_j   = h(relu(sum_c d0[j][c] din_c)),  sdf = h(h(sum_j d1[0][j] H_j) + h(-0.1))
#   s = h(exp(h(h(variance) 10))),  sig = h(1 / (1 + exp(-h(sdf s)))),  density = h(h(s sig) h(1 - sig))
#
# (h: fp16 rounding.) din_c is a multiple of 2^-12 in [-0.5, 0.5]. With d0 entries +-2^15 a nonzero combination gives a
# hidden value of 8 at the least; d1 is chosen so the SDF is then large enough for sig to round to 1 (density exactly 0)
# and small enough to stay finite. Where every unit is 0 the SDF is h(-0.1) and the density one constant D0.
# ------------------------------------------------------------------------------------------------------------------
SDF_BIAS = -0.1
D0 = {0.0: 0.2493896484375, 0.1: 0.6669921875, 0.2: 1.6162109375, 0.3: 2.095703125}
UNIT = 2.0 ** 15
PERTURB = 2.0 ** -16

# name -> (rows of (column weights), d1 weight). A row is the three position-column weights of one hidden unit.
STEP_NETS = {
    "all": ([], 2.0),
    "half_x": ([(UNIT, 0, 0)], 2.0),
    "half_y": ([(0, UNIT, 0)], 2.0),
    "half_z": ([(0, 0, UNIT)], 2.0),
    # three units can each reach 2^14: d1 = 1.25 keeps their sum at 61440 (2 would give 98304, past fp16), and the
    # smallest nonzero SDF at 10 - 0.1
    "octant": ([(UNIT, 0, 0), (0, UNIT, 0), (0, 0, UNIT)], 1.25),
    "slab_x": ([(UNIT, 0, 0), (-UNIT, 0, 0)], 2.0),
    "slab_z": ([(0, 0, UNIT), (0, 0, -UNIT)], 2.0),
    # din_0 + din_1 reaches 1: the hidden value 2^15, and 1.25 of it 40960
    "sheet_xy": ([(UNIT, UNIT, 0), (-UNIT, -UNIT, 0)], 1.25),
}


def h16(a):
    return np.asarray(a, np.float64).astype(np.float16).astype(np.float64)


def din_values():
    """Every value din_c can take: h(h(x) - 0.5) over all fp16 values h(x) of x in [0, 1]."""
    bits = np.arange(0, 0x3c01, dtype=np.uint16)  # +0 .. 1.0
    hx = bits.view(np.float16).astype(np.float64)
    return np.unique(h16(hx - 0.5))


def density_chain(sdf_pre, variance, e1=0.0, e2=0.0):
    """The density of k_nerf_density from the second layer's fp32 result, with the two exponentials perturbed by the
    relative errors e1, e2 (0: float64 exp rounded through float32, as an exact expf would give)."""
    sdf = h16(h16(sdf_pre) + h16(SDF_BIAS))
    s = h16(np.float32(np.exp(h16(h16(variance) * 10.0)) * (1 + e1)))
    with np.errstate(over="ignore"):
        ex = np.float32(np.exp(-h16(sdf * s)) * (1 + e2))
    sig = h16(np.float32(1.0) / (np.float32(1.0) + ex))
    return h16(h16(s * sig) * h16(1.0 - sig))


def step_net_density(name, din, variance=0.0, e1=0.0, e2=0.0, report=None):
    """The density of step network `name` at density inputs din [n][3] (float64 fp16 values). report (a dict) receives the
    largest hidden value and second-layer sum seen."""
    rows, d1 = STEP_NETS[name]
    din = np.asarray(din, np.float64)
    pre = np.zeros(len(din))
    hmax = 0.0
    for row in rows:
        a = din @ np.asarray(row, np.float64)  # exact: multiples of 2^3 below 2^16
        H = h16(np.maximum(a, 0))
        hmax = max(hmax, float(np.abs(a).max(initial=0.0)))
        pre = pre + d1 * H
    if report is not None:
        report["hidden_max"] = hmax
        report["sum_max"] = float(np.abs(pre).max(initial=0.0))
    return density_chain(pre, variance, e1, e2)


def step_net_on_surface(name, din):
    """True where every unit of the network is 0: the occupied set."""
    rows, _ = STEP_NETS[name]
    on = np.ones(len(din), bool)
    for row in rows:
        on &= (np.asarray(din, np.float64) @ np.asarray(row, np.float64)) <= 0
    return on


def step_net_params(name, base, lay, W, din_w, variance):
    """base (the testbed's parameters) with the density MLP replaced by the step network, the colour MLP kept, the hash
    table zeroed and the variance parameter set."""
    rows, d1 = STEP_NETS[name]
    assert len(rows) <= W
    p = np.array(base, np.float32, copy=True)
    d0 = np.zeros((W, din_w), np.float32)
    w1 = np.zeros((16, W), np.float32)
    for j, row in enumerate(rows):
        d0[j, :3] = row
        w1[0, j] = d1
    p[:W * din_w] = d0.ravel()
    p[W * din_w:W * din_w + 16 * W] = w1.ravel()
    g0, v0 = int(lay["grid_offset"]), int(lay["variance_offset"])
    p[g0:v0] = 0
    p[v0] = variance
    return p
