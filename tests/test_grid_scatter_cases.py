"""The exact-integer cases of tests/grid_scatter_cases.py carry the bitwise GPU tests (test_gpu_grid_scatter.py) only if
their premises hold for the drawn inputs: every contribution a multiple of 2^-q, every per-entry sum of magnitudes below
2^24 units of it (so any fp32 sum in any order is exact), and the contract's fixed-point result equal to the float64
autograd of grid_nd_ref.grid_encode rounded once to fp32. If a changed seed ever breaks the first two, shrink the integer
ranges of the inputs; these are conditions of the cases, not properties of the code under test."""
import numpy as np
import pytest

import grid_nd_ref as G
import grid_scatter_cases as S


@pytest.mark.parametrize("case", list(S.X_CASES))
def test_contributions_are_exact(case):
    (D, F, ty, ip, L, log2, base, pls), q = S.X_CASES[case]
    off, res = S.x_tables(case)
    pos, table, dly, u = S.x_inputs(case)
    assert pos.shape == (S.N, D) and (pos[:64] == pos[0]).all()
    # the interpolation fraction is exactly 3/4 at every level
    p = pos.astype(np.float64) * (res[0] - 1) + 0.5
    assert (p - np.floor(p) == 0.75).all()
    for second in (False, True):
        idx, val = S.contributions(pos, dly, u, off, res, F, ty, ip, second)
        units = val.astype(np.float64) * 2.0 ** q
        assert (units == np.rint(units)).all()
        mag = np.zeros(off[-1] * F)
        np.add.at(mag, idx, np.abs(units))
        count = np.bincount(idx, minlength=off[-1] * F)
        print(f"{case} {'second' if second else 'first'} order: max bits {np.log2(mag.max()):.1f}, up to {count.max()} contributions per parameter")
        assert mag.max() < 2.0 ** 24
        assert count.max() >= 64  # the identical rows meet in one entry


@pytest.mark.parametrize("case", list(S.X_CASES))
def test_contract_reference_is_the_rounded_float64_gradient(case):
    import torch
    (D, F, ty, ip, L, log2, base, pls), _ = S.X_CASES[case]
    off, res = S.x_tables(case)
    r = S.x_reference(case)
    tab = torch.tensor(r["table"].astype(np.float64), requires_grad=True)
    xt = torch.tensor(r["pos"].astype(np.float64), requires_grad=True)
    dly = torch.tensor(r["dly"].astype(np.float64))
    y = G.grid_encode(xt, tab, off, res, ty, ip)
    g_tab, g_x = torch.autograd.grad((y * dly).sum(), (tab, xt), create_graph=True)
    g2_tab, = torch.autograd.grad((g_x * torch.tensor(r["u"].astype(np.float64))).sum(), (tab,))
    for key, g in (("g_tab", g_tab), ("g2_tab", g2_tab)):
        want = g.detach().numpy().ravel().astype(np.float32)
        assert want.any()
        assert np.array_equal(r[key].view(np.uint32), want.view(np.uint32)), key


def test_fixed_point_sum_poisons_and_rounds_once():
    idx = np.array([0, 0, 1, 2, 2, 3])
    val = np.array([0.5, np.inf, 2.0 ** 31, 2.0 ** -33, 2.0 ** -33, -3.0], np.float32)
    out = S.fixed_point_sum(idx, val, 5)
    assert np.isnan(out[0]) and np.isnan(out[1])
    # 2^-33 is half a unit: rint goes to the even 0, per contribution, before the sum
    assert out[2] == 0 and out[3] == -3 and out[4] == 0 and not np.signbit(out[4])
