#!/usr/bin/env python3
"""Times a SIREN (CutlassMLP, Sine, "second_order": "exact") against the same shape with Softplus exact and with ReLU:

    create_network 3 -> 1 (Identity encoding), --widths 64,256 neurons, 2 hidden layers, n = 2^18, "gradient_precision": "fp32"

    inference   the forward without a context: Sine evaluates the sin / cos pair and stores sin alone
    forward     with a context: Sine also stores cos z [2][n][W] fp16 (forward - inference = the cos buffer's write traffic;
                Sine inference - ReLU inference = the sincos evaluation and the vector epilogue)
    bbi         backward_backward_input, all three results: the Sine epilogues read cos z where the others evaluate
                act' / act'' from the stored activation

All variants run in one process on one stream. A window is --calls calls of one (variant, pass) between two HIP events
(torch.cuda.Event), after --warmup untimed calls of each; the variants alternate window by window, so all see the same
machine. Reported per (width, variant, pass): the median, fastest, 10th and 90th percentile window per call. With
NEUS2_HIP_LIB set to a library of another commit and --variants relu,softplus_exact the same script times that commit's
kernels. The whole run stops at --time-limit seconds. One JSON line per (width, variant, pass).

    python scripts/bench_siren.py [--log profiles/siren_bench.log]
"""
import argparse
import json
import os
import signal
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VARIANTS = {
    "sine_exact": {"activation": "Sine", "second_order": "exact"},
    "softplus_exact": {"activation": "Softplus", "second_order": "exact"},
    "relu": {"activation": "ReLU"},
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 18)
    ap.add_argument("--widths", default="64,256")
    ap.add_argument("--calls", type=int, default=20, help="calls per timed window")
    ap.add_argument("--windows", type=int, default=9, help="timed windows per variant and pass")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--variants", default=",".join(VARIANTS), help="comma-separated subset of: " + ", ".join(VARIANTS))
    ap.add_argument("--tag", default="", help="copied into every line (which library ran)")
    ap.add_argument("--time-limit", type=int, default=240)
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    signal.alarm(a.time_limit)  # the default action ends the process
    import numpy as np
    import torch
    from neus2_amd.module import GradientMode, Module
    if not torch.cuda.is_available():
        raise SystemExit("bench_siren: needs a GPU (no fallback)")
    n = a.n
    rng = np.random.default_rng(0)
    x = torch.from_numpy(rng.uniform(-1, 1, (n, 3)).astype(np.float32)).cuda()
    u = torch.from_numpy(rng.normal(0, 1, (n, 3)).astype(np.float32)).cuda()
    dlo = torch.zeros((n, 16), dtype=torch.float16, device="cuda")
    dlo[:, 0] = 1.0
    lines = []
    for W in [int(w) for w in a.widths.split(",")]:
        calls = {}
        for name in a.variants.split(","):
            cfg = dict({"otype": "CutlassMLP", "output_activation": "None", "n_neurons": W, "n_hidden_layers": 2, "gradient_precision": "fp32"}, **VARIANTS[name])
            m = Module.create_network(3, 1, cfg, batch_capacity=n)
            params = m.initialize_params(seed=1).half().contiguous()
            ctx, y = m.forward(x, params, prepare_input_gradients=True)
            g = torch.zeros(m.n_params, dtype=torch.float32, device="cuda")
            ddo = torch.zeros((n, 16), dtype=torch.float16, device="cuda")
            ddx = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
            keep = (m, ctx, params, g, ddo, ddx, y)

            def bbi(keep=keep):
                m, ctx, params, g, ddo, ddx, _ = keep
                m.backward_backward_input(ctx, x, u, dlo, params, dL_dparams=g, dL_ddLdoutput=ddo, mode=GradientMode.Overwrite, dL_dinput=ddx)

            def forward(keep=keep):
                keep[0].forward(x, keep[2], prepare_input_gradients=True, output=keep[6])

            def inference(keep=keep):
                keep[0].inference(x, keep[2], output=keep[6])
            for fn in (inference, forward, bbi):
                for _ in range(a.warmup):
                    fn()
                calls[(name, fn.__name__)] = fn
            torch.cuda.synchronize()
            assert bool(torch.isfinite(g).all()) and bool(torch.isfinite(ddx).all()) and g.abs().sum().item() > 0
        t = {k: [] for k in calls}
        for _ in range(a.windows):
            for key, fn in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.calls):
                    fn()
                e1.record()
                e1.synchronize()
                t[key].append(e0.elapsed_time(e1) * 1e3 / a.calls)  # us per call
        for (name, what), v in t.items():
            v = np.sort(np.asarray(v))
            lines.append(json.dumps({"tag": a.tag, "width": W, "variant": name, "pass": what, "n": n, "median_us": round(float(np.median(v)), 1),
                                     "min_us": round(float(v[0]), 1), "p10_us": round(float(np.percentile(v, 10)), 1),
                                     "p90_us": round(float(np.percentile(v, 90)), 1)}))
            print(lines[-1], flush=True)
    lines.append(json.dumps({"summary": "bench_siren", "tag": a.tag, "device": torch.cuda.get_device_name(0), "calls_per_window": a.calls,
                             "windows": a.windows, "warmup": a.warmup}))
    print(lines[-1])
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
