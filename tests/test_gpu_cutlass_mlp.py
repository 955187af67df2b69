"""CutlassMLP networks of widths above 128 (ffmlp.hip's wide kernels) in floating point, by the rule of
test_gpu_ffmlp_second_order.py: the forward output, the first backward's dL_dparams / dL_dinput and
backward_backward_input's dL_dparams (per matrix and per table), dL_ddLdoutput and dL_dinput against torch.autograd on the
unrounded float64 network (the truth, tests/act_ref.py), behind the Identity encoding, the fp16 HashGrid and Frequency.

Tolerance. For its own inputs each case computes floor = rel-L2(model, truth) on the CPU, the model being the same chain in
float64 with an fp16 rounding wherever the device stores fp16. The device is held to rel-L2(device, truth) <= 4 floor and
never beyond rel-L2 2e-2 and cosine 0.999: the factor and the ceilings of test_gpu_ffmlp_second_order.py, which explains
them. Every measured value and its floor go to parity_metrics.jsonl.

The cases: Softplus W 256 (two row tiles, four k chunks, every epilogue of a curved hidden layer), Sigmoid / Sigmoid W 144
(all curved epilogues, the output's included, on a ragged second row tile), ReLU / Sigmoid W 512 (the colour-network shape
at the largest width). All are "second_order": "exact", n = 128.

Also: bitwise repeatability of two calls, initialize_params for W 256 (the xavier rule as test_gpu_ffmlp.py restates it,
bit-exact), and that a CutlassMLP of width 64 is bitwise the FullyFusedMLP of width 64."""
import functools

import numpy as np
import pytest

import act_ref as A
import bbi_ref as R

pytestmark = pytest.mark.gpu

CEIL_REL, MIN_COS, FACTOR = 2e-2, 0.999, 4.0
N = 128
FREQ = {"otype": "Frequency", "n_frequencies": 4}
# encoding (None: create_network's Identity), n_in, act / out, W, hidden layers, n_out, and the seed of the case's inputs (if
# one leaves more than 5 % of a ReLU case's samples on a branch boundary, the seed changes, not the condition)
CASES = {
    "softplus_w256": dict(enc=None, n_in=12, act="Softplus", out="None", W=256, N=2, n_out=2, seed=300),
    "sigmoid_sigmoid_w144": dict(enc=None, n_in=8, act="Sigmoid", out="Sigmoid", W=144, N=1, n_out=3, seed=301),
    "relu_sigmoid_w512": dict(enc=None, n_in=3, act="ReLU", out="Sigmoid", W=512, N=1, n_out=3, seed=313),
    "hashgrid_softplus_w256": dict(enc=R.ENC_CFG, n_in=3, act="Softplus", out="None", W=256, N=2, n_out=3, seed=303),
    "frequency_softplus_w256": dict(enc=FREQ, n_in=3, act="Softplus", out="None", W=256, N=2, n_out=1, seed=304),
}


def _net_cfg(c, otype="CutlassMLP"):
    return {"otype": otype, "n_neurons": c["W"], "n_hidden_layers": c["N"], "activation": c["act"], "output_activation": c["out"],
            "gradient_precision": "fp32", "second_order": "exact"}


def _module(c, otype="CutlassMLP"):
    from neus2_amd.module import Module
    if c["enc"] is None:
        return Module.create_network(c["n_in"], c["n_out"], _net_cfg(c, otype), batch_capacity=N)
    return Module.create_network_with_input_encoding(c["n_in"], c["n_out"], c["enc"], _net_cfg(c, otype), batch_capacity=N)


def _encoder(c):
    """(enc(x, table) in float64, the table's feature count or None, the rows' padding value)"""
    import enc_ref
    from torch_ref import hash_grid
    if c["enc"] is None:
        return (lambda x, tab: x), None, 1.0
    if c["enc"] is R.ENC_CFG:
        return (lambda x, tab: hash_grid(x, tab, R.OFF, R.RES)), 2, 0.0
    return (lambda x, tab: enc_ref.encode(x, c["enc"])), None, 1.0


def first_order(enc, x, table, mats, g, act, out, pad_value, rounded):
    """The forward and the first backward: dict(y, dW, dtable, dx). Unrounded it is torch.autograd on A.network; rounded it
    is the device's chain with an fp16 rounding at each of its storage points (every sum, activation and delta), the
    encoding's Jacobian by autograd with the chain's dL/dX0 as a constant cotangent."""
    import torch
    xt = x.detach().clone().requires_grad_(True)
    tab = None if table is None else table.detach().clone().requires_grad_(True)
    leaves = [xt] + ([tab] if tab is not None else [])
    E = A.rows(enc(xt, tab), pad_value)
    z = lambda v, like: torch.zeros_like(like) if v is None else v
    if not rounded:
        ms = [m.detach().clone().requires_grad_(True) for m in mats]
        y = A.network(ms, E, act, out)
        gr = torch.autograd.grad((y * g).sum(), ms + leaves, allow_unused=True)
        return dict(y=y.detach(), dW=list(gr[:len(ms)]), dx=z(gr[len(ms)], xt), dtable=None if tab is None else z(gr[len(ms) + 1], tab))
    r = A.r16
    with torch.no_grad():
        n_h = len(mats) - 1
        h = [r(E.detach())]
        for i in range(n_h):
            h.append(r(A.act(act, r(h[i] @ mats[i].T))))
        y = r(A.act(out, r(h[n_h] @ mats[n_h].T)))
        d = g if out == "None" else r(g * r(A.dact(out, y)))
        dW = [None] * (n_h + 1)
        for l in range(n_h, -1, -1):
            dW[l] = d.T @ h[l]
            if l > 0:
                d = r(r(A.dact(act, h[l])) * r(d @ mats[l]))
        dX0 = r(d @ mats[0])
    gr = torch.autograd.grad((E * dX0).sum(), leaves, allow_unused=True)
    return dict(y=y, dW=dW, dx=z(gr[0], xt), dtable=None if tab is None else z(gr[1], tab))


@functools.lru_cache(maxsize=None)
def _case(name):
    """The case's inputs (numpy, as the device gets them) with truth and model of both passes, computed once and shared."""
    import torch
    c = CASES[name]
    n_in, W, NH = c["n_in"], c["W"], c["N"]
    enc, F, pad_value = _encoder(c)
    rng = np.random.default_rng(c["seed"])
    # inputs: fp16 values where the device reads fp16 (the Identity encoding's x and u), fp32 positions for the rest
    if c["enc"] is None:
        x = rng.uniform(-1, 1, (N, n_in)).astype(np.float16).astype(np.float32)
    else:
        x = rng.uniform(0.02, 0.98, (N, n_in)).astype(np.float32)
    u = rng.normal(0, 1, (N, n_in)).astype(np.float16).astype(np.float32)
    out_pad = (c["n_out"] + 15) // 16 * 16
    g = rng.normal(0, 1, (N, out_pad)).astype(np.float16)
    with torch.no_grad():
        width = enc(torch.zeros(1, n_in, dtype=torch.float64), torch.zeros(1 << 14, F, dtype=torch.float64) if F else None).shape[1]
    in_pad = (width + 15) // 16 * 16
    shapes = [(W, in_pad)] + [(W, W)] * (NH - 1) + [(out_pad, W)]
    n_mlp = sum(r * k for r, k in shapes)
    # O(1) activations at every width (as bbi_ref.net_params draws them); the grid's features in [-1, 1]
    parts = [rng.normal(0, 1.2 / np.sqrt(k), (r, k)).ravel() for r, k in shapes] + ([rng.uniform(-1, 1, R.N_GRID)] if F else [])
    ph = np.concatenate(parts).astype(np.float16)
    mats, o = [], 0
    for r, k in shapes:
        mats.append(torch.tensor(ph[o:o + r * k].astype(np.float64).reshape(r, k)))
        o += r * k
    table = torch.tensor(ph[o:].astype(np.float64).reshape(-1, F)) if F else None
    ambiguous = 0.0
    if c["act"] == "ReLU":  # samples whose hidden pre-activation may take the other branch on the device: out of g and u
        h0 = A.r16(A.rows(torch.tensor(x.astype(np.float64)), 1.0))
        amb = (np.abs(A.r16(h0 @ mats[0].T).numpy()) < R.AMBIGUOUS).any(axis=1)
        g[amb] = 0
        u[amb] = 0
        ambiguous = amb.mean()
    xt, ut, gt = torch.tensor(x.astype(np.float64)), torch.tensor(u.astype(np.float64)), torch.tensor(g.astype(np.float64))
    args = (enc, xt, table, ut, mats, gt, c["act"], c["out"], pad_value)
    fo = (enc, xt, table, mats, gt, c["act"], c["out"], pad_value)
    return dict(c=c, x=x, u=u, g=g, ph=ph, shapes=shapes, n_mlp=n_mlp, ambiguous=ambiguous,
                truth=A.truth(*args), model=A.bbi(*args, rounded=True), truth1=first_order(*fo, False), model1=first_order(*fo, True))


def _run(t, m, k):
    """forward, backward and backward_backward_input on the device, as numpy:
    (output, dL_dparams, dL_dinput, bbi dL_dparams, bbi dL_ddLdoutput, bbi dL_dinput)"""
    from neus2_amd.module import GradientMode
    dev16 = lambda a: t.from_numpy(a.view(np.int16).copy()).cuda()
    params, x, u, g = dev16(k["ph"]), t.from_numpy(k["x"]).cuda(), t.from_numpy(k["u"]).cuda(), dev16(k["g"])
    full = lambda shape, dtype: t.full(shape, 7.0, dtype=dtype, device="cuda")
    ctx, y = m.forward(x, params, prepare_input_gradients=True)
    g1, dx1 = full((m.n_params,), t.float32), full((N, m.n_input_dims), t.float32)
    m.backward(ctx, x, g, params, dL_dparams=g1, dL_dinput=dx1, mode=GradientMode.Overwrite, output=y)
    g2, ddo, dx2 = full((m.n_params,), t.float32), full((N, m.n_output_dims), t.float16), full((N, m.n_input_dims), t.float32)
    m.backward_backward_input(ctx, x, u, g, params, dL_dparams=g2, dL_ddLdoutput=ddo, mode=GradientMode.Overwrite, dL_dinput=dx2)
    t.cuda.synchronize()
    return tuple(a.cpu().numpy() for a in (y, g1, dx1, g2, ddo, dx2))


def _held(name, what, got, truth, model, failures):
    floor = A.rel(model, truth)
    rel, cos = R.rel_cos(got, truth)
    bound = min(FACTOR * floor, CEIL_REL)
    R.record(f"cutlass_{name}_{what}", rel=rel, one_minus_cos=1 - cos, floor=floor)
    print(f"{name} {what}: rel {rel:.3e} floor {floor:.3e} bound {bound:.3e} 1-cos {1 - cos:.3e}")
    if not (rel <= bound and cos >= MIN_COS):
        failures.append((what, rel, floor, bound, cos))


@pytest.mark.parametrize("name", list(CASES))
def test_cutlass_mlp_parity(torch_cuda, name):
    t = torch_cuda
    k = _case(name)
    assert k["ambiguous"] <= 0.05
    m = _module(k["c"])
    assert m.n_params == k["ph"].size and m.hyperparams()["network"]["otype"] == "CutlassMLP"
    y, g1, dx1, g2, ddo, dx2 = _run(t, m, k)
    failures = []
    _held(name, "output", y.astype(np.float32), k["truth1"]["y"].numpy(), k["model1"]["y"].numpy(), failures)
    for tag, gp, dx, truth, model in (("bwd", g1, dx1, k["truth1"], k["model1"]), ("bbi", g2, dx2, k["truth"], k["model"])):
        o = 0
        for l, (r, c) in enumerate(k["shapes"]):
            _held(name, f"{tag}_dW{l}", gp[o:o + r * c], truth["dW"][l].numpy(), model["dW"][l].numpy(), failures)
            o += r * c
        if truth["dtable"] is not None:
            _held(name, f"{tag}_dtable", gp[o:], truth["dtable"].numpy(), model["dtable"].numpy(), failures)
        assert truth["dx"].abs().max().item() > 0
        _held(name, f"{tag}_dL_dinput", dx, truth["dx"].numpy(), model["dx"].numpy(), failures)
    _held(name, "bbi_dL_ddLdoutput", ddo.astype(np.float32), k["truth"]["ddo"].numpy(), k["model"]["ddo"].numpy(), failures)
    assert not failures, failures


@pytest.mark.parametrize("name", list(CASES))
def test_cutlass_mlp_is_repeatable(torch_cuda, name):
    t = torch_cuda
    k = _case(name)
    m = _module(k["c"])
    for p, q in zip(_run(t, m, k), _run(t, m, k)):
        np.testing.assert_array_equal(p.view(np.uint8), q.view(np.uint8))


def test_initialize_params_w256(torch_cuda):
    """pcg32{seed} xavier-uniform per matrix in order, as test_gpu_ffmlp.py restates it, bit-exact"""
    import oracle as O
    c = CASES["softplus_w256"]
    m = _module(c)
    shapes = [(256, 16), (256, 256), (16, 256)]
    P = sum(r * k for r, k in shapes)
    assert m.n_params == P
    p32 = m.initialize_params(seed=7).cpu().numpy()
    u = O.pcg32(7, 1, 0, P)
    f = ((u >> np.uint32(9)) | np.uint32(0x3F800000)).view(np.float32) - np.float32(1)
    ref, off = np.zeros(P, np.float32), 0
    for r, k in shapes:
        sc = np.float32(np.sqrt(np.float32(6.0) / np.float32(r + k)))
        ref[off: off + r * k] = f[off: off + r * k] * np.float32(2) * sc - sc
        off += r * k
    np.testing.assert_array_equal(p32, ref)


def test_width_64_is_the_fully_fused_network(torch_cuda):
    """a width that FullyFusedMLP has takes the same kernels under either otype: bitwise the same results, the same echo"""
    t = torch_cuda
    c = dict(CASES["softplus_w256"], W=64)
    rng = np.random.default_rng(77)
    shapes = [(64, 16), (64, 64), (16, 64)]
    ph = np.concatenate([rng.normal(0, 1.2 / np.sqrt(k), (r, k)).ravel() for r, k in shapes]).astype(np.float16)
    k = dict(ph=ph, x=rng.uniform(-1, 1, (N, 12)).astype(np.float32), u=rng.normal(0, 1, (N, 12)).astype(np.float32),
             g=rng.normal(0, 1, (N, 16)).astype(np.float16))
    a, b = _module(c, "CutlassMLP"), _module(c, "FullyFusedMLP")
    assert a.hyperparams() == b.hyperparams() and a.hyperparams()["network"]["otype"] == "FullyFusedMLP"
    outs = _run(t, a, k), _run(t, b, k)
    for p, q in zip(*outs):
        np.testing.assert_array_equal(p.view(np.uint8), q.view(np.uint8))
    assert all(np.abs(p.astype(np.float32)).max() > 0 for p in outs[0])
