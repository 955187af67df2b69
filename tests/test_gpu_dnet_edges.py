"""The fused HashGrid -> MLP module (k_dnet: W 64, one hidden ReLU layer, tests/bbi_ref.py's grid) at the batch sizes its
other tests never reach: n = 1, 33 (a partial wave), 1000, 2100 (17 blocks = 17 partial rows, ending in a partial wave)
and 65569 = 512 x 128 + 33 (past dnet_blocks' cap of 512 blocks: the grid-stride second trip, where the weight-gradient
accumulators carry over, ending in a partial wave); n odd is an odd row stride of the paired [L][n] buffers.

Two invariants, neither with a tolerance:
* a row of the forward output, dL_dinput, backward_backward_input's dL_ddLdoutput and dL_dinput depends on that sample
  alone: the first n rows of an n-batch equal the first n rows of the 65569-batch bit for bit;
* a parameter gradient whose dL_doutput is nonzero on one row only is one term plus exact zeros (the MLP blocks: products
  with a zero operand; the grid block: the scatter's records carry their own scale and are summed as integers, run merges
  add exact zeros), so it equals, as numbers (+0 == -0), that of the 1-batch holding the row alone, wherever the row sits:
  rows 0, 31, 32, 127, 128, n - 1 (wave, block and tail boundaries) and 65535, 65536 (the stride trip's boundary).
Against float64 autograd (bbi_ref.network) at n = 1000 and 65569 under test_gpu_bbi_full.py's bars for this network
(rel-L2 <= 2e-3, cosine >= 0.99999). The positions are 65569 of 70000 candidates that the reference does not call
ambiguous (a hidden pre-activation within 1e-4 of 0); the ambiguous share must stay <= 0.05."""
import types

import numpy as np
import pytest

import bbi_ref as R

pytestmark = pytest.mark.gpu

N_MAX, N_CAND, CAPACITY = 65569, 70000, 65664
SIZES = [1, 33, 1000, 2100, N_MAX]
W = R.NETS["dnet"][1]
N_MLP = W * R.DE + 16 * W


def _probe_rows(n):
    return sorted({p for p in (0, 31, 32, 127, 128, n - 1, 65535, 65536) if p < n})


@pytest.fixture(scope="module")
def S(torch_cuda):
    from neus2_amd.module import GradientMode, Module
    t = torch_cuda
    m = Module.create_network_with_input_encoding(3, 1, R.ENC_CFG, dict(R.net_cfg("dnet"), gradient_precision="fp32"),
                                                  batch_capacity=CAPACITY)
    rng = np.random.default_rng(41)
    ph = R.net_params("dnet", rng, 0.3)
    assert ph.size == m.n_params == N_MLP + R.N_GRID and m.n_output_dims == 16
    cand = rng.uniform(0.02, 0.98, (N_CAND, 3)).astype(np.float32)
    amb = R.network("dnet", ph, cand)["ambiguous"]
    print(f"dnet edges: ambiguous share {amb.mean():.4f} of {N_CAND}")
    assert amb.mean() <= 0.05
    pos = cand[~amb][:N_MAX]
    assert pos.shape[0] == N_MAX
    dlo = rng.normal(0, 1, (N_MAX, 16)).astype(np.float16)
    v = rng.normal(0, 1, (N_MAX, 3)).astype(np.float32)
    s = types.SimpleNamespace(t=t, m=m, ph=ph, pos=pos, dlo=dlo, v=v, Overwrite=GradientMode.Overwrite)
    s.params = t.from_numpy(ph.view(np.int16).copy()).cuda()
    s.x, s.u = t.from_numpy(pos).cuda(), t.from_numpy(v).cuda()
    s.dl = t.from_numpy(dlo.view(np.int16).copy()).cuda()
    s.runs, s.single = {}, {}
    return s


def _grads(s, ctx, x, u, dl):
    """dL_dparams of backward and of backward_backward_input (host)"""
    t, m = s.t, s.m
    g1 = t.full((m.n_params,), 7.0, dtype=t.float32, device="cuda")
    g2 = t.full((m.n_params,), 7.0, dtype=t.float32, device="cuda")
    m.backward(ctx, x, dl, s.params, dL_dparams=g1, mode=s.Overwrite)
    m.backward_backward_input(ctx, x, u, dl, s.params, dL_dparams=g2, mode=s.Overwrite)
    return g1.cpu().numpy(), g2.cpu().numpy()


def _run(s, n):
    """Everything the module computes on the first n rows (once per n)."""
    if n in s.runs:
        return s.runs[n]
    t, m = s.t, s.m
    x, u, dl = s.x[:n], s.u[:n], s.dl[:n]
    ctx, y = m.forward(x, s.params, prepare_input_gradients=True)
    g1 = t.full((m.n_params,), 7.0, dtype=t.float32, device="cuda")
    dx = t.full((n, 3), 7.0, dtype=t.float32, device="cuda")
    m.backward(ctx, x, dl, s.params, dL_dparams=g1, dL_dinput=dx, mode=s.Overwrite)
    g2 = t.full((m.n_params,), 7.0, dtype=t.float32, device="cuda")
    ddo = t.full((n, 16), 7.0, dtype=t.float16, device="cuda")
    ddx = t.full((n, 3), 7.0, dtype=t.float32, device="cuda")
    m.backward_backward_input(ctx, x, u, dl, s.params, dL_dparams=g2, dL_ddLdoutput=ddo, mode=s.Overwrite, dL_dinput=ddx)
    r = types.SimpleNamespace(ctx=ctx, x=x, u=u, y=y.cpu().numpy(), g1=g1.cpu().numpy(), dx=dx.cpu().numpy(), g2=g2.cpu().numpy(),
                              ddo=ddo.cpu().numpy(), ddx=ddx.cpu().numpy())
    s.runs[n] = r
    return r


def _single(s, p):
    """The parameter gradients of the 1-batch holding sample p alone."""
    if p not in s.single:
        x, u, dl = s.x[p:p + 1].clone(), s.u[p:p + 1].clone(), s.dl[p:p + 1].clone()
        ctx, _ = s.m.forward(x, s.params, prepare_input_gradients=True)
        s.single[p] = _grads(s, ctx, x, u, dl)
    return s.single[p]


@pytest.mark.parametrize("n", SIZES)
def test_prefix_invariance(S, n):
    full, part = _run(S, N_MAX), _run(S, n)
    for name, bits in (("y", np.uint16), ("dx", np.uint32), ("ddo", np.uint16), ("ddx", np.uint32)):
        a, b = getattr(part, name), getattr(full, name)[:n]
        np.testing.assert_array_equal(a.view(bits), b.view(bits), err_msg=f"{name} at n = {n}")


@pytest.mark.parametrize("n", [33, 2100, N_MAX])
def test_single_row_probes(S, n):
    t = S.t
    r = _run(S, n)
    for p in _probe_rows(n):
        dl = t.zeros((n, 16), dtype=t.int16, device="cuda")
        dl[p] = S.dl[p]
        g1, g2 = _grads(S, r.ctx, r.x, r.u, dl)
        s1, s2 = _single(S, p)
        assert s1[:N_MLP].any() and s1[N_MLP:].any() and s2[:N_MLP].any() and s2[N_MLP:].any()
        for order, got, want in (("backward", g1, s1), ("backward_backward_input", g2, s2)):
            np.testing.assert_array_equal(got[:N_MLP], want[:N_MLP], err_msg=f"{order} MLP block, n = {n}, row {p}")
            np.testing.assert_array_equal(got[N_MLP:], want[N_MLP:], err_msg=f"{order} grid block, n = {n}, row {p}")


@pytest.mark.parametrize("n", [1000, N_MAX])
def test_against_float64(S, n):
    import torch
    r = _run(S, n)
    ref = R.network("dnet", S.ph, S.pos[:n])
    assert not ref["ambiguous"].any()  # (chosen so; nothing is masked)
    dlo_t = torch.tensor(S.dlo[:n].astype(np.float64), requires_grad=True)
    leaves = ref["leaves"]
    g1 = torch.autograd.grad((ref["out"] * dlo_t).sum(), leaves + [ref["xt"]], create_graph=True)
    g2 = torch.autograd.grad((g1[-1] * torch.tensor(S.v[:n].astype(np.float64))).sum(), leaves + [dlo_t, ref["xt"]])
    blocks = {"W0": slice(0, W * R.DE), "W1": slice(W * R.DE, N_MLP), "grid": slice(N_MLP, None)}
    f1, f2 = R.flat(g1[:3]), R.flat(g2[:3])
    pairs = {"forward": (r.y, ref["out"].detach().numpy()), "dL_dinput": (r.dx, g1[-1].detach().numpy()),
             "dL_ddLdoutput_2nd": (r.ddo, g2[3].numpy()), "dL_dinput_2nd": (r.ddx, g2[4].numpy())}
    for name, sl in blocks.items():
        pairs[name] = (r.g1[sl], f1[sl])
        pairs[name + "_2nd"] = (r.g2[sl], f2[sl])
    res = {name: R.rel_cos(a, b) for name, (a, b) in pairs.items()}
    R.record(f"dnet_edges_n{n}", **{f"rel_{k}": rc[0] for k, rc in res.items()}, **{f"one_minus_cos_{k}": 1 - rc[1] for k, rc in res.items()})
    print(n, {k: f"{rc[0]:.3e} / {1 - rc[1]:.3e}" for k, rc in res.items()})
    for name, (rel, cos) in res.items():
        assert rel <= 2e-3 and cos >= 0.99999, (name, rel, cos)
