#!/usr/bin/env python3
"""Times the general grid's parameter gradient with "gradient_scatter": "binned" (grid_nd_scatter.hip) against the float
atomics of the same build (grid_nd.hip), with the method of scripts/bench_grid_nd.py: launches captured into a graph, one
replay between two HIP events is one window, the two sides alternate window by window, median (p10 - p90) per launch.

Each side issues what the operator module issues for it:
    param_grad  atomic: memset of dL_dparams + k_gnd_backward          binned: k_gnds_lds + k_gnds_direct + k_gnds_finish
    bbi_all     atomic: memset + k_gnd_bbi (all outputs) + k_gnd_sum   binned: the scatter kernels with the weights a_c +
                                                                               k_gnd_bbi without dL_dparams + k_gnd_sum
at n = 2^18 on the three shapes of DESIGN.md section 3.12 (14 levels, log2_hashmap_size 19, base 16, per-level scale
128^(1/13)): 3-D 2 features Linear fp32, 2-D 4 features Smoothstep fp16, 4-D 4 features Smoothstep fp16. After each pair
the two sides' gradients are compared (rel-L2), and the binned one with a second replay of itself (bitwise).

    python scripts/bench_grid_nd_scatter.py [--log profiles/grid_nd_binned_bench.log]
"""
import argparse
import ctypes as C
import json
import os
import signal
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_grid_nd import GridNd, PfView, grid, launcher  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 18)
    ap.add_argument("--launches", type=int, default=20, help="launches per timed window")
    ap.add_argument("--windows", type=int, default=21, help="timed windows per side")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--time-limit", type=int, default=300)
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    signal.alarm(a.time_limit)  # the default action ends the process
    import numpy as np
    import torch
    from neus2_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("bench_grid_nd_scatter: needs a GPU (no fallback)")
    lib = _lib.lib()
    P, u32, vp = C.POINTER, C.c_uint32, C.c_void_p
    L_ = lambda name, args: launcher(lib, _lib.LIB_PATH, name, args)
    nd_bwd = L_("launch_grid_nd_backward", [vp, u32, P(GridNd), u32, vp, P(PfView), vp])
    nd_bbi = L_("launch_grid_nd_bbi", [vp, u32, P(GridNd), u32, vp, vp, C.c_bool, vp, P(PfView), vp, P(PfView), u32, vp, vp])
    nd_sc = L_("launch_grid_nd_scatter", [vp, u32, P(GridNd), u32, vp, vp, P(PfView), vp, C.c_bool, vp, vp])
    values = L_("grid_nd_scatter_values", [P(GridNd)])
    values.restype = C.c_uint64
    n = a.n
    rng = np.random.default_rng(0)
    lines = []

    def measure(sides):
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        for f in sides.values():
            for _ in range(a.warmup):
                f(stream)
        torch.cuda.synchronize()
        graphs = {}
        for key, f in sides.items():
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                cap = C.c_void_p(torch.cuda.current_stream().cuda_stream)
                for _ in range(a.launches):
                    f(cap)
            g.replay()
            graphs[key] = g
        torch.cuda.synchronize()
        t = {k: [] for k in sides}
        for _ in range(a.windows):
            for key in sides:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                graphs[key].replay()
                e1.record()
                e1.synchronize()
                t[key].append(e0.elapsed_time(e1) * 1e3 / a.launches)  # us per launch
        out = {}
        for key, v in t.items():
            v = np.sort(np.asarray(v))
            out[key] = {"median_us": round(float(np.median(v)), 3), "min_us": round(float(v[0]), 3),
                        "p10_us": round(float(np.percentile(v, 10)), 3), "p90_us": round(float(np.percentile(v, 90)), 3)}
        return out, graphs

    L = 14
    for name, D, F, smooth, f32 in (("bench_shape", 3, 2, False, True), ("B_like", 2, 4, True, False), ("I_like", 4, 4, True, False)):
        G = grid(D, F, smooth, L, 19, 16, 128.0 ** (1.0 / 13.0))
        P_ = G.gl.offset[L] * F
        dt, tdt = (np.float32, torch.float32) if f32 else (np.float16, torch.float16)
        x = torch.from_numpy(rng.uniform(0, 1, (n, D)).astype(np.float32)).cuda()
        u = torch.from_numpy(rng.normal(0, 1, (n, D)).astype(np.float32)).cuda()
        table = torch.from_numpy(rng.uniform(-1, 1, P_).astype(dt)).cuda()
        dly = torch.from_numpy(rng.normal(0, 1, (n, F * L)).astype(dt)).cuda()
        ddo = torch.zeros((n, F * L), dtype=tdt, device="cuda")
        ga, gb = torch.zeros(P_, device="cuda"), torch.zeros(P_, device="cuda")
        part, dx = torch.zeros((D * L, n), device="cuda"), torch.zeros((n, D), device="cuda")
        n_acc = int(values(C.byref(G)))
        acc, poison = torch.zeros(n_acc, dtype=torch.int64, device="cuda"), torch.zeros(n_acc, dtype=torch.uint8, device="cuda")
        vd, vq = PfView(dly.data_ptr(), F * L, 1, int(f32)), PfView(ddo.data_ptr(), F * L, 1, int(f32))
        shape = {"n": n, "n_input_dims": D, "n_features_per_level": F, "n_levels": L, "entries": int(G.gl.offset[L]), "table": "fp32" if f32 else "fp16",
                 "interpolation": "Smoothstep" if smooth else "Linear", "workspace_bytes": 9 * n_acc}

        def atomic_grad(s):
            ga.zero_()
            nd_bwd(s, n, C.byref(G), L, x.data_ptr(), C.byref(vd), ga.data_ptr())

        def binned_grad(s):
            nd_sc(s, n, C.byref(G), L, x.data_ptr(), None, C.byref(vd), gb.data_ptr(), False, acc.data_ptr(), poison.data_ptr())

        def atomic_bbi(s):
            ga.zero_()
            nd_bbi(s, n, C.byref(G), L, x.data_ptr(), table.data_ptr(), f32, u.data_ptr(), C.byref(vd), ga.data_ptr(), C.byref(vq), 0, part.data_ptr(),
                   dx.data_ptr())

        def binned_bbi(s):
            nd_sc(s, n, C.byref(G), L, x.data_ptr(), u.data_ptr(), C.byref(vd), gb.data_ptr(), False, acc.data_ptr(), poison.data_ptr())
            nd_bbi(s, n, C.byref(G), L, x.data_ptr(), table.data_ptr(), f32, u.data_ptr(), C.byref(vd), None, C.byref(vq), 0, part.data_ptr(),
                   dx.data_ptr())

        for kname, sides in (("param_grad", {"atomic": atomic_grad, "binned": binned_grad}), ("bbi_all", {"atomic": atomic_bbi, "binned": binned_bbi})):
            stats, graphs = measure(sides)
            torch.cuda.synchronize()
            first = gb.clone()
            graphs["binned"].replay()
            torch.cuda.synchronize()
            rec = {"case": name, "kernel": kname, **shape, **stats}
            rec["binned_over_atomic"] = round(stats["binned"]["median_us"] / stats["atomic"]["median_us"], 4)
            rec["binned_bitwise_repeatable"] = bool(torch.equal(first.view(torch.int32), gb.view(torch.int32)))
            rec["rel_l2_binned_vs_atomic"] = float((gb.double() - ga.double()).norm() / ga.double().norm())
            rec["accumulators_left_zero"] = not bool(acc.any()) and not bool(poison.any())
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
            del graphs
        del table, dly, ddo, ga, gb, part, dx, acc, poison
    lines.append(json.dumps({"summary": "bench_grid_nd_scatter", "device": torch.cuda.get_device_name(0), "launches_per_window": a.launches,
                             "windows": a.windows, "warmup": a.warmup}))
    print(lines[-1])
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
