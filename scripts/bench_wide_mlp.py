#!/usr/bin/env python3
"""Times the wide CutlassMLP kernels (ffmlp.hip: k_ff_layer_wide, k_ff_wgrad_wide) against two yardsticks of the same run:

    create_network(3 inputs, 1 output), 2 hidden layers, Softplus / None, "second_order": "exact", "gradient_precision":
    "fp32", n = 2^18, at n_neurons 128 (FullyFusedMLP: the existing kernels, the project's own rate), 256 and 512
    (CutlassMLP: the wide kernels)

    forward    Module.forward
    backward   Module.backward with dL_dparams and dL_dinput
    bbi        Module.backward_backward_input with dL_dparams, dL_ddLdoutput and dL_dinput

    matmul     torch.matmul in fp16 (the vendor library's rate) on the three distinct products of one hidden layer, for
               W = 256 and 512: [n, W] x [W, W] (nn), [n, W] x [W, W]^T (nt) and [W, n] x [n, W] (tn, the weight gradient)

Everything runs in one process on one stream. A window is --calls calls of one item between two HIP events
(torch.cuda.Event) after --warmup untimed calls of each; the items alternate window by window, so all see the same machine.
Reported per item: the median, fastest, 10th and 90th percentile window per call, and the achieved FLOP/s of the median:
2 n O K per matrix product the pass launches, on the matrices' own (16-padded) sizes, so neither tile padding nor epilogue
work counts. The last line is a summary with the ratios. The whole run stops at --time-limit seconds.

    python scripts/bench_wide_mlp.py [--log profiles/wide_mlp_bench.log] [--only w512_bbi,...]
"""
import argparse
import json
import os
import signal
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_IN, N_OUT, HIDDEN = 3, 1, 2
WIDTHS = (128, 256, 512)


def products(W):
    """matrix products (O x K, counted as O K) of each pass, as ff_forward / ff_backward_chain / ff_bbi_chain launch them for
    Softplus hidden layers, a linear output and every result asked for"""
    mats = [W * 16] + [W * W] * (HIDDEN - 1) + [16 * W]  # layer l: rows x cols
    P = sum(mats)
    fwd = P
    bwd = P + P  # one weight gradient per matrix; the delta through every matrix (layer 0: dL_dinput)
    # fronts through every matrix (the last: dL_ddLdoutput); backs t through matrices N .. 1; the curvature adjoint's product
    # through matrices N - 1 .. 1 (below the linear output there is none) and q through matrix 0; weight gradients: one
    # product for the output matrix, two for every other
    bbi = P + sum(mats[1:]) + sum(mats[1:-1]) + mats[0] + mats[-1] + 2 * sum(mats[:-1])
    return {"forward": fwd, "backward": bwd, "bbi": bbi}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 18)
    ap.add_argument("--calls", type=int, default=20, help="calls per timed window")
    ap.add_argument("--windows", type=int, default=9, help="timed windows per item")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default=None, help="comma-separated subset of the items (w128_forward, ..., mm512_tn)")
    ap.add_argument("--time-limit", type=int, default=240)
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    signal.alarm(a.time_limit)  # the default action ends the process
    import numpy as np
    import torch
    from neus2_amd.module import GradientMode, Module
    if not torch.cuda.is_available():
        raise SystemExit("bench_wide_mlp: needs a GPU (no fallback)")
    n = a.n
    only = set(a.only.split(",")) if a.only else None
    want = lambda item: only is None or item in only
    rng = np.random.default_rng(0)
    x = torch.from_numpy(rng.uniform(-1, 1, (n, N_IN)).astype(np.float32)).cuda()
    u = torch.from_numpy(rng.normal(0, 1, (n, N_IN)).astype(np.float32)).cuda()
    dlo = torch.zeros((n, 16), dtype=torch.float16, device="cuda")
    dlo[:, 0] = 1.0
    items, flop = {}, {}
    for W in WIDTHS:
        if not any(want(f"w{W}_{p}") for p in ("forward", "backward", "bbi")):
            continue
        cfg = {"otype": "FullyFusedMLP" if W == 128 else "CutlassMLP", "n_neurons": W, "n_hidden_layers": HIDDEN, "activation": "Softplus",
               "output_activation": "None", "second_order": "exact", "gradient_precision": "fp32"}
        m = Module.create_network(N_IN, N_OUT, cfg, batch_capacity=n)
        params = m.initialize_params(seed=1).half().contiguous()
        ctx, y = m.forward(x, params, prepare_input_gradients=True)
        g = torch.zeros(m.n_params, dtype=torch.float32, device="cuda")
        ddo = torch.zeros((n, 16), dtype=torch.float16, device="cuda")
        dx = torch.zeros((n, N_IN), dtype=torch.float32, device="cuda")
        keep = (m, ctx, y, params, g, ddo, dx)

        def forward(keep=keep):
            keep[0].forward(x, keep[3], output=keep[2], prepare_input_gradients=True)

        def backward(keep=keep):
            m, ctx, y, params, g, ddo, dx = keep
            m.backward(ctx, x, dlo, params, dL_dparams=g, dL_dinput=dx, mode=GradientMode.Overwrite, output=y)

        def bbi(keep=keep):
            m, ctx, y, params, g, ddo, dx = keep
            m.backward_backward_input(ctx, x, u, dlo, params, dL_dparams=g, dL_ddLdoutput=ddo, mode=GradientMode.Overwrite, dL_dinput=dx)
        for name, fn in (("forward", forward), ("backward", backward), ("bbi", bbi)):
            if want(f"w{W}_{name}"):
                items[f"w{W}_{name}"] = fn
                flop[f"w{W}_{name}"] = 2.0 * n * products(W)[name]
        backward()
        bbi()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(g).all()) and bool(torch.isfinite(dx).all()) and g.abs().sum().item() > 0
    for W in WIDTHS[1:]:
        act = torch.randn((n, W), dtype=torch.float16, device="cuda")
        act2 = torch.randn((n, W), dtype=torch.float16, device="cuda")
        w = torch.randn((W, W), dtype=torch.float16, device="cuda")
        out, outw = torch.empty((n, W), dtype=torch.float16, device="cuda"), torch.empty((W, W), dtype=torch.float16, device="cuda")
        for name, fn in (("nn", lambda act=act, w=w, out=out: torch.matmul(act, w, out=out)),
                         ("nt", lambda act=act, w=w, out=out: torch.matmul(act, w.t(), out=out)),
                         ("tn", lambda act=act, act2=act2, outw=outw: torch.matmul(act.t(), act2, out=outw))):
            if want(f"mm{W}_{name}"):
                items[f"mm{W}_{name}"] = fn
                flop[f"mm{W}_{name}"] = 2.0 * n * W * W
    for fn in items.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in items}
    for _ in range(a.windows):
        for name, fn in items.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.calls):
                fn()
            e1.record()
            e1.synchronize()
            t[name].append(e0.elapsed_time(e1) * 1e3 / a.calls)  # us per call
    lines, rate = [], {}
    for name, v in t.items():
        v = np.sort(np.asarray(v))
        med = float(np.median(v))
        rate[name] = flop[name] / (med * 1e-6) / 1e12
        lines.append(json.dumps({"item": name, "n": n, "median_us": round(med, 1), "min_us": round(float(v[0]), 1),
                                 "p10_us": round(float(np.percentile(v, 10)), 1), "p90_us": round(float(np.percentile(v, 90)), 1),
                                 "gflop": round(flop[name] / 1e9, 2), "tflops": round(rate[name], 2)}))
        print(lines[-1], flush=True)
    summary = {"summary": "bench_wide_mlp", "device": torch.cuda.get_device_name(0), "calls_per_window": a.calls, "windows": a.windows,
               "warmup": a.warmup}
    mm = {W: [rate[k] for k in (f"mm{W}_nn", f"mm{W}_nt", f"mm{W}_tn") if k in rate] for W in WIDTHS[1:]}
    for W in WIDTHS[1:]:
        for p in ("forward", "backward", "bbi"):
            k = f"w{W}_{p}"
            if k in rate and f"w128_{p}" in rate:
                summary[f"{k}_over_w128"] = round(rate[k] / rate[f"w128_{p}"], 3)
            if k in rate and len(mm[W]) == 3:
                summary[f"{k}_over_matmul"] = round(rate[k] / (3.0 / sum(1.0 / r for r in mm[W])), 3)  # the three products' harmonic mean
    lines.append(json.dumps(summary))
    print(lines[-1])
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
