#!/usr/bin/env python3
"""Times backward_backward_input of an SDF-shaped module with the exact double backward against the same shape with ReLU:

    HashGrid (14 levels, 2 features, T = 2^19, base 16, per_level_scale 1.4142: the README's) -> FullyFusedMLP of 64
    neurons, 2 hidden layers, 1 output, n = 2^18, "gradient_precision": "fp32", all three results asked for

    softplus_exact   "activation": "Softplus", "second_order": "exact": the chain with the act'' terms (the fronts keep p,
                     the backs t, one curvature epilogue per hidden layer, two products per weight gradient, q through the
                     grid's first-order backward in the one scatter)
    relu             "activation": "ReLU": the fronts / backs chain (act'' = 0), the same launches as before this key

Both run in one process on one stream. A window is --calls calls of one variant between two HIP events (torch.cuda.Event),
after --warmup untimed calls of each; the variants alternate window by window, so both see the same machine. Reported per
variant: the median, fastest, 10th and 90th percentile window per call, and the ratio of the medians with the ReLU
variant's spread beside it (--variants relu with NEUS2_HIP_LIB set to a library of another commit times
that commit's chain: the key is this build's, the ReLU variant runs anywhere). The whole run stops at --time-limit seconds. One JSON line per variant, the last line a
summary with the ratio.

    python scripts/bench_second_order.py [--log profiles/second_order_bench.log]
"""
import argparse
import json
import os
import signal
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ENC = {"otype": "HashGrid", "n_levels": 14, "n_features_per_level": 2, "log2_hashmap_size": 19, "base_resolution": 16,
       "per_level_scale": 1.4142}
VARIANTS = {
    "softplus_exact": {"activation": "Softplus", "second_order": "exact"},
    "relu": {"activation": "ReLU"},
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 18)
    ap.add_argument("--calls", type=int, default=100, help="calls per timed window")
    ap.add_argument("--windows", type=int, default=15, help="timed windows per variant")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--variants", default=",".join(VARIANTS), help="comma-separated subset of: " + ", ".join(VARIANTS))
    ap.add_argument("--time-limit", type=int, default=240)
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    signal.alarm(a.time_limit)  # the default action ends the process
    import numpy as np
    import torch
    from neus2_amd.module import GradientMode, Module
    if not torch.cuda.is_available():
        raise SystemExit("bench_second_order: needs a GPU (no fallback)")
    n = a.n
    rng = np.random.default_rng(0)
    x = torch.from_numpy(rng.uniform(0.02, 0.98, (n, 3)).astype(np.float32)).cuda()
    u = torch.from_numpy(rng.normal(0, 1, (n, 3)).astype(np.float32)).cuda()
    dlo = torch.zeros((n, 16), dtype=torch.float16, device="cuda")
    dlo[:, 0] = 1.0
    calls = {}
    for name in a.variants.split(","):
        keys = VARIANTS[name]
        cfg = dict({"otype": "FullyFusedMLP", "output_activation": "None", "n_neurons": 64, "n_hidden_layers": 2, "gradient_precision": "fp32"}, **keys)
        m = Module.create_network_with_input_encoding(3, 1, ENC, cfg, batch_capacity=n)
        p32 = m.initialize_params(seed=1)
        p32[m.info["grid_offset"]:].uniform_(-0.5, 0.5, generator=torch.Generator(device="cuda").manual_seed(1))  # a grid off its 1e-4 start
        params = p32.half().contiguous()
        ctx, _ = m.forward(x, params, prepare_input_gradients=True)
        g = torch.zeros(m.n_params, dtype=torch.float32, device="cuda")
        ddo = torch.zeros((n, 16), dtype=torch.float16, device="cuda")
        ddx = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
        keep = (m, ctx, params, g, ddo, ddx)

        def call(keep=keep):
            m, ctx, params, g, ddo, ddx = keep
            m.backward_backward_input(ctx, x, u, dlo, params, dL_dparams=g, dL_ddLdoutput=ddo, mode=GradientMode.Overwrite, dL_dinput=ddx)
        for _ in range(a.warmup):
            call()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(g).all()) and bool(torch.isfinite(ddx).all()) and g.abs().sum().item() > 0
        calls[name] = call
    t = {k: [] for k in calls}
    for _ in range(a.windows):
        for name, call in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.calls):
                call()
            e1.record()
            e1.synchronize()
            t[name].append(e0.elapsed_time(e1) * 1e3 / a.calls)  # us per call
    lines, med = [], {}
    for name, v in t.items():
        v = np.sort(np.asarray(v))
        med[name] = float(np.median(v))
        lines.append(json.dumps({"variant": name, "n": n, "median_us": round(med[name], 1), "min_us": round(float(v[0]), 1),
                                 "p10_us": round(float(np.percentile(v, 10)), 1), "p90_us": round(float(np.percentile(v, 90)), 1),
                                 "ns_per_sample": round(med[name] * 1e3 / n, 3)}))
        print(lines[-1], flush=True)
    summary = {"summary": "bench_second_order", "device": torch.cuda.get_device_name(0), "calls_per_window": a.calls, "windows": a.windows,
               "warmup": a.warmup}
    if len(med) == len(VARIANTS):
        vr = np.asarray(t["relu"])
        summary.update(softplus_exact_over_relu=round(med["softplus_exact"] / med["relu"], 3),
                       relu_spread=round(float(np.percentile(vr, 90) - np.percentile(vr, 10)) / med["relu"], 4))
    lines.append(json.dumps(summary))
    print(lines[-1])
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
