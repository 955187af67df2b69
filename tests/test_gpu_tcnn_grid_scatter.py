""""gradient_scatter": "binned" through the PyTorch modules (`import tinycudann as tcnn`): a 2-D Smoothstep grid with 4
features per level in front of a Softplus network under the eikonal loss of test_gpu_tcnn_grid_nd.py, B = 200. The double
backward runs the grid's first-order scatter (backward), its second-order scatter (backward_backward_input) and the
curvature cotangent on top of it (backward_curved). Two independent passes give bitwise equal params.grad, and it agrees
with the atomic module's within the tolerance the suite holds float-atomic sums to (test_gpu_grid_nd_mlp.py: rtol 1e-5,
atol 2e-5 x the largest magnitude)."""
import numpy as np
import pytest

from test_gpu_grid_nd import CASES, config

pytestmark = pytest.mark.gpu

B = 200
NET = {"otype": "FullyFusedMLP", "activation": "Softplus", "output_activation": "None", "n_neurons": 64, "n_hidden_layers": 2}


def _eikonal(y, x, torch):
    n, = torch.autograd.grad(y.sum(), x, create_graph=True)
    return ((n.norm(dim=1) - 1) ** 2).mean() + (y ** 2).mean()


def test_eikonal_params_grad_is_repeatable(torch_cuda):
    import torch
    import tinycudann as tcnn
    case = "B"
    assert CASES[case][:4] == (2, 4, "Hash", "Smoothstep")
    pos = np.random.default_rng(51).uniform(0.02, 0.98, (B, 2)).astype(np.float32)
    grads = {}
    for scatter in ("binned", "atomic"):
        extra = {"gradient_scatter": "binned"} if scatter == "binned" else {}
        m = tcnn.NetworkWithInputEncoding(2, 1, config(case, **extra), NET, seed=7)
        if scatter == "binned":
            first = m.params.detach().clone()
            with torch.no_grad():  # a table away from its tiny initial values, so that the grid's terms are live
                m.params.add_(0.05 * torch.randn(m.params.shape, generator=torch.Generator().manual_seed(3)).cuda())
            params = m.params.detach().clone()
        else:
            assert torch.equal(m.params.detach(), first)
            with torch.no_grad():
                m.params.copy_(params)
        runs = []
        for _ in range(2):
            m.params.grad = None
            x = torch.from_numpy(pos).cuda().requires_grad_(True)
            _eikonal(m(x).float(), x, torch).backward()
            runs.append(m.params.grad.detach().cpu().numpy().copy())
        grads[scatter] = runs
    a, b = grads["binned"]
    assert np.isfinite(a).all() and a.any()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    want = grads["atomic"][0]
    np.testing.assert_allclose(a, want, rtol=1e-5, atol=2e-5 * max(1.0, np.abs(want).max()))
