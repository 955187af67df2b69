"""neus_grid_encode (grid.hip k_grid_encode) against the oracle's encode at the edges of its index arithmetic, bitwise.

The encode forms a level's corner entries without a division and addresses its rows by 32-bit offsets. The oracle
restates the reference's grid_index with its `% hashmap_size`. n = 300 samples in rows of ld = 512: uniform positions,
positions exactly on cell boundaries and on vertices of levels 0, 5 and 13, the corners of the unit cube, and positions
outside it (negative cells and cells past the resolution: the dense levels' true modulo). Rows of a level above the valid
one are exactly zero and the row tails [n, ld) keep the caller's bytes."""
import ctypes as C
import os

import numpy as np
import pytest

from edge_positions import edge_positions
from gpu_util import dev, host, ptr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, LD = 300, 512
ENC_FILL, DY_FILL = np.int16(0x7b7b), np.float32(-123.456)


@pytest.fixture(scope="module")
def env(torch_cuda):
    from neus2_amd import pyngp, scenes
    import oracle as O
    sc = scenes.small_scene(n_views=8, width=64, height=48)
    tb = pyngp.Testbed(pyngp.TestbedMode.Nerf)
    tb.set_dataset(sc["images"], sc["focal"], sc["principal"], sc["xforms"], 1)
    tb.reload_network_from_file(os.path.join(ROOT, "configs", "nerf", "base.json"), batch_size=1024)
    cfg = O.make_cfg(per_level_scale=tb._net_cfg.per_level_scale)
    # O(0.1) grid values: every corner's term counts in the fp16 feature sum
    lay = tb.layout()
    p = tb.get_params().copy()
    g0, g1 = lay["grid_offset"], lay["variance_offset"]
    p[g0:g1] = np.random.default_rng(21).uniform(-0.1, 0.1, g1 - g0).astype(np.float32)
    tb.set_params(p)
    return dict(tb=tb, O=O, cfg=cfg, params=p, t=torch_cuda)


def _positions(O, cfg):
    return edge_positions(O, cfg, N)


def _encode(env, valid):
    """neus_grid_encode of the positions over sentinel-filled rows: (coords, enc [L][LD][2] u16, dy/dx [6 L][LD] u32)."""
    from neus2_amd._lib import check, lib
    t, O, tb, cfg = env["t"], env["O"], env["tb"], env["cfg"]
    Lv = cfg.n_levels
    c = np.zeros((N, 7), np.float32)
    c[:, :3] = _positions(O, cfg)
    enc = t.from_numpy(np.full((Lv, LD, 2), ENC_FILL, np.int16)).cuda()
    dydx = t.from_numpy(np.full((6 * Lv, LD), DY_FILL, np.float32)).cuda()
    check(lib().neus_grid_encode(tb.handle, None, C.c_uint32(N), C.c_uint32(LD), ptr(dev(t, c)), C.c_uint32(7), C.c_uint32(valid), ptr(enc), ptr(dydx)))
    t.cuda.synchronize()
    return c, host(enc, np.uint16).reshape(Lv, LD, 2), host(dydx, np.uint32).reshape(6 * Lv, LD)


@pytest.mark.parametrize("valid", (13, 3, 0))
def test_encode_edges_match_oracle_bitwise(env, valid):
    O, cfg = env["O"], env["cfg"]
    Lv = cfg.n_levels
    c, e, d = _encode(env, valid)
    assert np.all(e[:, N:] == ENC_FILL.view(np.uint16)), "enc written past n"
    assert np.all(d[:, N:] == DY_FILL.view(np.uint32)), "dy/dx written past n"
    assert not np.any(e[valid + 1:, :N]) and not np.any(d[6 * (valid + 1):, :N]), "a level above the valid one is not exactly zero"
    got = e[:, :N].view(np.float16).astype(np.float32).transpose(1, 0, 2).reshape(N, 2 * Lv)
    gdy = d[:, :N].reshape(Lv, 2, 3, N).transpose(3, 0, 1, 2).reshape(N, 2 * Lv, 3)
    ref, rdy = O.grid_forward(cfg, env["params"], c[:, :3], valid)
    np.testing.assert_array_equal(got.view(np.uint32), ref.astype(np.float32).view(np.uint32))
    np.testing.assert_array_equal(gdy, rdy.view(np.uint32))


def test_generic_encode_kernel_matches_direct(env):
    """The generic k_grid_encode (grid_index, 64-bit offsets: what other level tables or larger shapes get), forced by
    the test hook, writes the same bytes as the direct form, row tails included."""
    from neus2_amd._lib import check, lib
    _, e, d = _encode(env, 3)
    check(lib().neus_debug_set_grid_generic(C.c_uint32(1)))
    try:
        _, eg, dg = _encode(env, 3)
    finally:
        check(lib().neus_debug_set_grid_generic(C.c_uint32(0)))
    np.testing.assert_array_equal(eg, e)
    np.testing.assert_array_equal(dg, d)
