"""create_network with a CutlassMLP (fp32 gradient precision) on exact-integer networks (tests/int_net.py), by the scheme
of test_gpu_ffmlp_exact.py: every fp16 value the kernels store is an integer <= 2048 and every fp32 sum an integer < 2^24,
so the forward output, dL_dparams, dL_dinput and backward_backward_input's dL_dparams / dL_ddLdoutput must equal the int64
reference exactly, whatever the row tiling, the k chunks, the sample slices or their summation order. The shapes and what
each reaches in the wide kernels: tests/cutlass_cases.py (test_cutlass_cases.py asserts their domain on the CPU).

The kernels write only what they own: output, dL_dinput and dL_ddLdoutput carry 128 extra rows of a sentinel that must
survive, dL_dparams starts as the sentinel under Overwrite and every entry must be written."""
import numpy as np
import pytest

import cutlass_cases
import int_net

pytestmark = pytest.mark.gpu

SENTINEL = 0.5  # never an integer result
GROUPS = {}
for _s in cutlass_cases.SHAPES:
    GROUPS.setdefault((_s[:4], _s[5], _s[6]), []).append(_s[4])
GROUPS = [(k, ns) for k, ns in GROUPS.items()]


@pytest.mark.parametrize("group", GROUPS, ids=lambda g: "-".join(map(str, g[0][0])) + "-n" + "_".join(map(str, g[1])))
def test_cutlass_exact(torch_cuda, group):
    from neus2_amd.module import GradientMode, Module
    t = torch_cuda
    ((n_in, n_out, W, N), capacity, seed), ns = group
    m = Module.create_network(n_in, n_out, {"otype": "CutlassMLP", "n_neurons": W, "n_hidden_layers": N, "activation": "ReLU",
                                            "output_activation": "None", "gradient_precision": "fp32"}, batch_capacity=capacity)
    params = None
    for n in ns:
        net = int_net.make(n_in, n_out, W, N, n, seed)
        int_net.check_domain(net)
        assert m.n_params == net.params.size and m.n_output_dims == net.out_pad
        if params is None:
            params, p_host = t.from_numpy(net.params.view(np.int16).copy()).cuda(), net.params
        np.testing.assert_array_equal(net.params, p_host)  # the same parameters at every n of a module
        x, u = t.from_numpy(net.x).cuda(), t.from_numpy(net.u).cuda()
        dL = t.from_numpy(net.dL.view(np.int16).copy()).cuda()
        pad = n + 128

        def guarded(cols, dtype):
            return t.full((pad, cols), SENTINEL, dtype=dtype, device="cuda")

        def rows(buf, what):
            a = buf.float().cpu().numpy()
            assert (a[n:] == SENTINEL).all(), f"{what}: rows past n were written"
            return a[:n]

        y = guarded(net.out_pad, t.float16)
        ctx, _ = m.forward(x, params, output=y)
        np.testing.assert_array_equal(rows(y, "output"), net.out)
        g = t.full((m.n_params,), SENTINEL, dtype=t.float32, device="cuda")
        dx = guarded(n_in, t.float32)
        m.backward(ctx, x, dL, params, dL_dparams=g, dL_dinput=dx, mode=GradientMode.Overwrite, output=y)
        np.testing.assert_array_equal(g.cpu().numpy(), net.dL_dparams)
        np.testing.assert_array_equal(rows(dx, "dL_dinput"), net.dL_dinput)
        g2 = t.full((m.n_params,), SENTINEL, dtype=t.float32, device="cuda")
        ddo, ddx = guarded(net.out_pad, t.float16), guarded(n_in, t.float32)
        m.backward_backward_input(ctx, x, u, dL, params, dL_dparams=g2, dL_ddLdoutput=ddo, mode=GradientMode.Overwrite, dL_dinput=ddx)
        np.testing.assert_array_equal(g2.cpu().numpy(), net.bbi_dL_dparams)
        np.testing.assert_array_equal(rows(ddo, "dL_ddLdoutput"), net.bbi_dL_ddLdoutput)
        assert not rows(ddx, "backward_backward_input dL_dinput").any()
