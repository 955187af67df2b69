"""The int64 reference of tests/int_net.py, pinned without a device: equal to float64 torch autograd on a small shape
(every float64 value there is an exact integer, so the comparison is assert_array_equal), and inside its exact domain
(stored values <= 2048, sum of |terms| < 2^24, alive share in [0.2, 0.8], nonzero gradients) for every shape that
test_gpu_ffmlp_exact.py runs."""
import numpy as np
import pytest

import int_net


def test_reference_equals_float64_autograd():
    import torch
    net = int_net.make(5, 3, 32, 2, 96, seed=1)
    int_net.check_domain(net)
    mats = [torch.tensor(m.astype(np.float64), requires_grad=True) for m in net.mats]
    x = torch.tensor(net.x.astype(np.float64), requires_grad=True)
    dL = torch.tensor(net.dL.astype(np.float64), requires_grad=True)
    h = torch.cat([x, torch.ones(net.n, net.in_pad - net.n_in, dtype=torch.float64)], 1)
    for l, Wm in enumerate(mats):
        h = h @ Wm.T
        if l < net.N:
            h = torch.relu(h)
    np.testing.assert_array_equal(h.detach().numpy(), net.out)
    grads = torch.autograd.grad((h * dL).sum(), mats + [x], create_graph=True)
    np.testing.assert_array_equal(np.concatenate([g.detach().numpy().ravel() for g in grads[:-1]]), net.dL_dparams)
    np.testing.assert_array_equal(grads[-1].detach().numpy(), net.dL_dinput)
    S = (grads[-1] * torch.tensor(net.u.astype(np.float64))).sum()
    g2 = torch.autograd.grad(S, mats + [dL, x], allow_unused=True)
    np.testing.assert_array_equal(np.concatenate([g.numpy().ravel() for g in g2[:net.N + 1]]), net.bbi_dL_dparams)
    np.testing.assert_array_equal(g2[-2].numpy(), net.bbi_dL_ddLdoutput)
    assert g2[-1] is None or not g2[-1].numpy().any()  # piecewise linear in x


@pytest.mark.parametrize("shape", int_net.SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_domain(shape):
    n_in, n_out, W, N, n, capacity, seed = shape
    assert n <= capacity and n % 128 == 0
    net = int_net.make(n_in, n_out, W, N, n, seed)
    print(f"max stored {net.max_stored}, max sum|terms| {net.max_terms}, alive {net.alive}")
    int_net.check_domain(net)
