"""neus2_amd.tcnn's autograd layer on the CPU: the two autograd Functions (forward; backward, whose own backward is the
double backward in the input) over a stand-in backend written in plain torch for y_k = sum_ij P_kij x_i x_j, whose second
derivatives are nonzero in every slot (x, params, grad_output). Compared with float64 autograd of the formula itself:
forward, autograd.grad, and the double backward with respect to x, params and grad_output, at B = 200 (padded to 256
rows inside; the padded rows must carry zero gradients) and loss_scale = 128 (it must cancel in every result that is
linear in dL_dy and must not enter dL_ddLdoutput). fp32 at rtol 1e-5; the absolute floor 1e-6 max|ref| is fp32's
rounding (6e-8) through the handful of operations between the stand-in's float64 arithmetic and the result."""
import numpy as np
import pytest
import torch

from neus2_amd import tcnn

B, D, K = 200, 3, 2


class QuadraticBackend:
    """y_k = sum_ij P_kij x_i x_j with explicit first and second derivatives (float64 inside, fp32 at the interface)."""
    n_input_dims, n_output_dims, n_params = D, K, K * D * D
    param_dtype = output_dtype = torch.float32
    supports_double_backward = True
    batch_capacity = None

    def __init__(self):
        self.calls = []
        self.seen = {}

    def with_capacity(self, n):
        return self

    def initialize_params(self, seed):
        return torch.from_numpy(np.random.default_rng(seed).normal(0, 1, self.n_params).astype(np.float32))

    def _P(self, p):
        P = p.double().reshape(K, D, D)
        return P, P + P.transpose(1, 2)

    def inference(self, x, p):
        self.calls.append("inference")
        P, _ = self._P(p)
        return torch.einsum("kij,ni,nj->nk", P, x.double(), x.double()).float()

    def fwd(self, x, p, prepare_input_gradients):
        self.calls.append(("fwd", bool(prepare_input_gradients)))
        assert x.shape[0] % 128 == 0 and x.dtype == torch.float32 and x.is_contiguous()
        P, _ = self._P(p)
        return None, torch.einsum("kij,ni,nj->nk", P, x.double(), x.double()).float()

    def bwd(self, ctx, x, p, dL_dy, want_dx, want_dparams):
        self.calls.append(("bwd", bool(want_dx), bool(want_dparams)))
        self.seen["g"] = dL_dy.clone()
        _, Q = self._P(p)
        g, xd = dL_dy.double(), x.double()
        dx = torch.einsum("nk,kaj,nj->na", g, Q, xd).float() if want_dx else None
        dp = torch.einsum("nk,ni,nj->kij", g, xd, xd).reshape(-1).float() if want_dparams else None
        return dx, dp

    def bwd_bwd_input(self, ctx, x, p, u, dL_dy, want_dparams, want_ddLdy, want_dx):
        self.calls.append(("bbi", bool(want_dparams), bool(want_ddLdy), bool(want_dx)))
        self.seen["u"] = u.clone()
        _, Q = self._P(p)
        g, xd, ud = dL_dy.double(), x.double(), u.double()
        dp = (torch.einsum("nk,ni,nj->kij", g, ud, xd) + torch.einsum("nk,ni,nj->kij", g, xd, ud)).reshape(-1).float() if want_dparams else None
        ddy = torch.einsum("na,kaj,nj->nk", ud, Q, xd).float() if want_ddLdy else None
        dx = torch.einsum("nk,na,kaj->nj", g, ud, Q).float() if want_dx else None
        return dp, ddy, dx


def _formula(x, P):
    return torch.einsum("kij,ni,nj->nk", P.reshape(K, D, D), x, x)


def _close(got, ref):
    ref = ref.detach().double().numpy()
    np.testing.assert_allclose(got.detach().double().numpy(), ref, rtol=1e-5, atol=1e-6 * np.abs(ref).max())


@pytest.fixture()
def setup():
    be = QuadraticBackend()
    m = tcnn.Module(seed=3, backend=be, loss_scale=128)
    rng = np.random.default_rng(0)
    x = torch.from_numpy(rng.normal(0, 1, (B, D)).astype(np.float32))
    w = torch.from_numpy(rng.normal(0, 1, (B, K)).astype(np.float32))
    return be, m, x, w


def test_attributes_and_forward(setup):
    be, m, x, _ = setup
    assert isinstance(m, torch.nn.Module) and m.params.dtype == torch.float32 and m.params.shape == (be.n_params,)
    assert m.n_input_dims == D and m.n_output_dims == K and m.loss_scale == 128 and m.dtype == torch.float32
    assert "n_input_dims=3" in repr(m)
    m.free_temporary_memory()
    y = m(x.clone().requires_grad_(True))
    assert y.shape == (B, K) and be.calls[-1] == ("fwd", True)
    _close(y, _formula(x.double(), m.params.detach().double()))
    with pytest.raises(ValueError):
        m(x[:, :2])


def test_first_order(setup):
    be, m, x, w = setup
    xg = x.clone().requires_grad_(True)
    gx, gp = torch.autograd.grad(m(xg), (xg, m.params), grad_outputs=w)
    xr, pr = x.double().requires_grad_(True), m.params.detach().double().requires_grad_(True)
    rx, rp = torch.autograd.grad(_formula(xr, pr), (xr, pr), grad_outputs=w.double())
    _close(gx, rx)
    _close(gp, rp)
    # the padded rows carry a zero dL_dy into the backend, which saw the loss-scaled value
    assert be.seen["g"].shape == (256, K) and not be.seen["g"][B:].any()
    np.testing.assert_array_equal(be.seen["g"][:B].numpy(), w.numpy() * 128)


def test_double_backward(setup):
    be, m, x, w = setup
    xg, wg = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = m(xg)
    n, = torch.autograd.grad(y, xg, grad_outputs=wg, create_graph=True)
    loss = (n ** 2).sum() + (y ** 2).mean()
    loss.backward()
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    pr = m.params.detach().double().requires_grad_(True)
    yr = _formula(xr, pr)
    nr, = torch.autograd.grad(yr, xr, grad_outputs=wr, create_graph=True)
    ((nr ** 2).sum() + (yr ** 2).mean()).backward()
    _close(n, nr)
    _close(xg.grad, xr.grad)
    _close(m.params.grad, pr.grad)
    _close(wg.grad, wr.grad)
    assert ("bbi", True, True, True) in be.calls
    assert be.seen["u"].shape == (256, D) and not be.seen["u"][B:].any()


def test_frozen_params(setup):
    be, m, x, w = setup
    m.params.requires_grad_(False)
    xg = x.clone().requires_grad_(True)
    y = m(xg)
    n, = torch.autograd.grad(y, xg, grad_outputs=w, create_graph=True)
    (n ** 2).sum().backward()
    xr = x.double().requires_grad_(True)
    nr, = torch.autograd.grad(_formula(xr, m.params.detach().double()), xr, grad_outputs=w.double(), create_graph=True)
    (nr ** 2).sum().backward()
    _close(xg.grad, xr.grad)
    assert m.params.grad is None
    assert ("bwd", True, False) in be.calls and ("bbi", False, False, True) in be.calls


def test_input_without_grad(setup):
    be, m, x, w = setup
    (m(x) * w).sum().backward()
    pr = m.params.detach().double().requires_grad_(True)
    (_formula(x.double(), pr) * w.double()).sum().backward()
    _close(m.params.grad, pr.grad)
    assert be.calls == [("fwd", False), ("bwd", False, True)]


def test_no_grad_runs_inference(setup):
    be, m, x, _ = setup
    with torch.no_grad():
        y = m(x)
    assert be.calls == ["inference"] and y.shape == (B, K) and not y.requires_grad
    _close(y, _formula(x.double(), m.params.detach().double()))


def test_unsupported_double_backward(setup):
    be, m, x, w = setup
    xg = x.clone().requires_grad_(True)
    gp, = torch.autograd.grad(m(xg), m.params, grad_outputs=w, create_graph=True)
    with pytest.raises(RuntimeError, match="not supported"):
        (gp ** 2).sum().backward()
    be.supports_double_backward = False
    n, = torch.autograd.grad(m(xg), xg, grad_outputs=w, create_graph=True)
    with pytest.raises(RuntimeError, match="not supported"):
        (n ** 2).sum().backward()


def test_pickle_drops_the_backend(setup):
    import pickle
    be, m, x, _ = setup
    state = pickle.loads(pickle.dumps(m.__getstate__()))
    assert state["_backend"] is None and m._backend is be
    np.testing.assert_array_equal(state["_parameters"]["params"].detach().numpy(), m.params.detach().numpy())
