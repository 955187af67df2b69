#!/usr/bin/env python3
"""Times the general grid encoding's kernels (grid_nd.hip) at n = 2^18, with the method of scripts/bench_encodings.py.

1. On the bench shape's grid (3-D, 2 features, 14 levels, log2_hashmap_size 19, base 16, per-level scale 128^(1/13), Hash,
   Linear, fp32 table) against the existing fp32 kernels (grid_f32.hip), pair by pair:
       forward      k_gnd_forward              vs k_grid_f32_forward without dy/dx (inference)
       forward_ctx  k_gnd_forward              vs k_grid_f32_forward storing dy/dx [6L][n] (what its input gradient reads)
       param_grad   k_gnd_backward             vs k_grid_f32_backward      (both: one float atomic per corner and feature)
       input_grad   k_gnd_dx + k_gnd_sum       vs k_grid_f32_input_grad    (a gather of the table again vs a read of dy/dx)
2. Alone, a case-B-like grid (2-D, 4 features, Smoothstep) and a case-I-like grid (4-D, 4 features, Smoothstep), both with
   14 levels, log2_hashmap_size 19, base 16, fp16 table and output: forward, param_grad, input_grad and the
   backward_backward_input kernel with all three outputs.

The launchers are C++ functions of libneus2_hip.so, found by name in its dynamic symbol table and called through ctypes
with their by-reference arguments as pointers. --launches launches are captured once into a graph; one replay between two
HIP events is one window; the two sides of a pair alternate window by window. Reported per kernel: median, fastest and
10th / 90th percentile window per launch; for the gradient kernels the bytes added by float atomics (4 per corner, feature,
level and sample) per second beside the chip-wide rate of ~1.3 TB/s that well-shaped float atomics reach on this chip.
One process; the whole run stops at --time-limit seconds. One JSON line per measurement, the last line a summary.

    python scripts/bench_grid_nd.py [--log profiles/grid_nd_bench.log]
"""
import argparse
import ctypes as C
import json
import os
import signal
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ATOMIC_RATE = 1.3e12
MAX_LEVELS = 16
HASH, DENSE, TILED = 0, 1, 2


class GridLevels(C.Structure):
    _fields_ = [("n_levels", C.c_uint32), ("offset", C.c_uint32 * (MAX_LEVELS + 1)), ("res", C.c_uint32 * MAX_LEVELS),
                ("scale", C.c_float * MAX_LEVELS), ("dense_bits", C.c_uint32)]


class GridNd(C.Structure):
    _fields_ = [("gl", GridLevels), ("D", C.c_uint32), ("F", C.c_uint32), ("type", C.c_uint32), ("smooth", C.c_uint32)]


class PfView(C.Structure):
    _fields_ = [("p", C.c_void_p), ("ss", C.c_uint64), ("sk", C.c_uint64), ("f32", C.c_uint32)]


def grid(D, F, smooth, L, log2, base, pls):
    """The Hash level tables (grid.h:1472-1508), as make_grid_nd builds them."""
    import numpy as np
    G = GridNd()
    G.D, G.F, G.type, G.smooth = D, F, HASH, int(smooth)
    G.gl.n_levels = L
    off = 0
    for l in range(L):
        s = np.float32(np.exp2(np.float32(l) * np.log2(np.float32(pls)))) * np.float32(base) - np.float32(1)
        r = int(np.ceil(s)) + 1
        p = min((min(r ** D, 0xFFFFFFFF // 2) + 7) // 8 * 8, 1 << log2)
        G.gl.offset[l], G.gl.res[l], G.gl.scale[l] = off, r, float(r - 1)
        if r ** D <= p:
            G.gl.dense_bits |= 1 << l
        off += p
    G.gl.offset[L] = off
    return G


def launcher(lib, lib_path, name, argtypes):
    out = subprocess.run(["nm", "-D", "--defined-only", lib_path], capture_output=True, text=True, check=True).stdout
    syms = [l.split()[-1] for l in out.splitlines() if name in l and " T " in l]
    if len(syms) != 1:
        raise RuntimeError(f"{name}: expected one exported symbol, found {syms}")
    f = getattr(lib, syms[0])
    f.restype, f.argtypes = None, argtypes
    return f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 18)
    ap.add_argument("--launches", type=int, default=100, help="launches per timed window")
    ap.add_argument("--windows", type=int, default=21, help="timed windows per kernel")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--time-limit", type=int, default=240)
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    signal.alarm(a.time_limit)  # the default action ends the process
    import numpy as np
    import torch
    from neus2_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("bench_grid_nd: needs a GPU (no fallback)")
    lib = _lib.lib()
    P, u32, vp = C.POINTER, C.c_uint32, C.c_void_p
    L_ = lambda name, args: launcher(lib, _lib.LIB_PATH, name, args)
    nd_fwd = L_("launch_grid_nd_forward", [vp, u32, P(GridNd), u32, vp, vp, C.c_bool, P(PfView), u32])
    nd_bwd = L_("launch_grid_nd_backward", [vp, u32, P(GridNd), u32, vp, P(PfView), vp])
    nd_dx = L_("launch_grid_nd_input_grad", [vp, u32, P(GridNd), u32, vp, vp, C.c_bool, P(PfView), vp, vp])
    nd_bbi = L_("launch_grid_nd_bbi", [vp, u32, P(GridNd), u32, vp, vp, C.c_bool, vp, P(PfView), vp, P(PfView), u32, vp, vp])
    f_fwd = L_("launch_grid_f32_forward", [vp, u32, P(GridLevels), u32, vp, vp, vp, u32, vp])
    f_bwd = L_("launch_grid_f32_backward", [vp, u32, P(GridLevels), u32, vp, vp, u32, vp, vp, vp])
    n = a.n
    rng = np.random.default_rng(0)
    lines = []

    def measure(sides):
        """sides: {name: f(stream)}; graph-replayed windows, the sides alternating. -> {name: stats}"""
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
        return out

    def atomics(rec, G, per_corner):
        """bytes added by float atomics per launch: 4 per corner, feature, level and sample (x per_corner)"""
        b = 4 * (1 << G.D) * G.F * G.gl.n_levels * n * per_corner
        rec["atomic_bytes"] = b
        for k in rec:
            if isinstance(rec[k], dict):
                rec[k]["atomic_TBps"] = round(b / (rec[k]["median_us"] * 1e-6) / 1e12, 4)
                rec[k]["share_of_chip_rate"] = round(b / (rec[k]["median_us"] * 1e-6) / ATOMIC_RATE, 4)

    def emit(rec):
        if "baseline" in rec:
            b = rec["baseline"]
            rec["new_over_baseline"] = round(rec["new"]["median_us"] / b["median_us"], 4)
            rec["baseline_spread"] = round((b["p90_us"] - b["p10_us"]) / b["median_us"], 4)
            rec["no_slower_beyond_spread"] = rec["new"]["median_us"] <= b["median_us"] * (1 + rec["baseline_spread"])
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    # ---- 1. the bench shape's grid, fp32, against grid_f32.hip
    L, F, D = 14, 2, 3
    G = grid(D, F, False, L, 19, 16, 128.0 ** (1.0 / 13.0))
    P_ = G.gl.offset[L] * F
    x = torch.from_numpy(rng.uniform(0, 1, (n, D)).astype(np.float32)).cuda()
    table = torch.from_numpy(rng.uniform(-1, 1, P_).astype(np.float32)).cuda()
    dly = torch.from_numpy(rng.normal(0, 1, (n, F * L)).astype(np.float32)).cuda()
    out_a, out_b = torch.zeros((n, F * L), device="cuda"), torch.zeros((n, F * L), device="cuda")
    dydx = torch.zeros((3 * F * L, n), device="cuda")
    ga, gb = torch.zeros(P_, device="cuda"), torch.zeros(P_, device="cuda")
    part = torch.zeros((D * L, n), device="cuda")
    dxa, dxb = torch.zeros((n, D), device="cuda"), torch.zeros((n, D), device="cuda")
    va = PfView(out_a.data_ptr(), F * L, 1, 1)
    vd = PfView(dly.data_ptr(), F * L, 1, 1)
    shape = {"n": n, "n_input_dims": D, "n_features_per_level": F, "n_levels": L, "entries": int(G.gl.offset[L]), "table": "fp32"}
    new_f = lambda s: nd_fwd(s, n, C.byref(G), L, x.data_ptr(), table.data_ptr(), True, C.byref(va), 0)
    old_f = lambda s: f_fwd(s, n, C.byref(G.gl), L, x.data_ptr(), table.data_ptr(), out_b.data_ptr(), 0, None)
    old_fc = lambda s: f_fwd(s, n, C.byref(G.gl), L, x.data_ptr(), table.data_ptr(), out_b.data_ptr(), 0, dydx.data_ptr())
    emit({"case": "bench_shape", "kernel": "forward", **shape, **measure({"new": new_f, "baseline": old_f})})
    assert torch.allclose(out_a, out_b, rtol=1e-5, atol=1e-6)
    emit({"case": "bench_shape", "kernel": "forward_ctx", **shape, **measure({"new": new_f, "baseline": old_fc})})
    new_b = lambda s: nd_bwd(s, n, C.byref(G), L, x.data_ptr(), C.byref(vd), ga.data_ptr())
    old_b = lambda s: f_bwd(s, n, C.byref(G.gl), L, x.data_ptr(), dly.data_ptr(), 0, gb.data_ptr(), None, None)
    rec = {"case": "bench_shape", "kernel": "param_grad", **shape, **measure({"new": new_b, "baseline": old_b})}
    atomics(rec, G, 1)
    emit(rec)
    new_d = lambda s: nd_dx(s, n, C.byref(G), L, x.data_ptr(), table.data_ptr(), True, C.byref(vd), part.data_ptr(), dxa.data_ptr())
    old_d = lambda s: f_bwd(s, n, C.byref(G.gl), L, x.data_ptr(), dly.data_ptr(), 0, None, dydx.data_ptr(), dxb.data_ptr())
    emit({"case": "bench_shape", "kernel": "input_grad", **shape, **measure({"new": new_d, "baseline": old_d})})
    assert torch.allclose(dxa, dxb, rtol=1e-4, atol=1e-2)
    del table, dly, out_a, out_b, dydx, ga, gb, part

    # ---- 2. Smoothstep grids of other shapes, fp16 table and output, alone
    for name, D, F in (("B_like", 2, 4), ("I_like", 4, 4)):
        G = grid(D, F, True, L, 19, 16, 128.0 ** (1.0 / 13.0))
        P_ = G.gl.offset[L] * F
        x = torch.from_numpy(rng.uniform(0, 1, (n, D)).astype(np.float32)).cuda()
        u = torch.from_numpy(rng.normal(0, 1, (n, D)).astype(np.float32)).cuda()
        table = torch.from_numpy(rng.uniform(-1, 1, P_).astype(np.float16)).cuda()
        dly = torch.from_numpy(rng.normal(0, 1, (n, F * L)).astype(np.float16)).cuda()
        out, ddo = torch.zeros((n, F * L), dtype=torch.float16, device="cuda"), torch.zeros((n, F * L), dtype=torch.float16, device="cuda")
        g = torch.zeros(P_, device="cuda")
        part, dx = torch.zeros((D * L, n), device="cuda"), torch.zeros((n, D), device="cuda")
        vo, vd, vq = PfView(out.data_ptr(), F * L, 1, 0), PfView(dly.data_ptr(), F * L, 1, 0), PfView(ddo.data_ptr(), F * L, 1, 0)
        shape = {"n": n, "n_input_dims": D, "n_features_per_level": F, "n_levels": L, "entries": int(G.gl.offset[L]), "table": "fp16",
                 "interpolation": "Smoothstep"}
        kernels = {
            "forward": (lambda s: nd_fwd(s, n, C.byref(G), L, x.data_ptr(), table.data_ptr(), False, C.byref(vo), 0), 0),
            "param_grad": (lambda s: nd_bwd(s, n, C.byref(G), L, x.data_ptr(), C.byref(vd), g.data_ptr()), 1),
            "input_grad": (lambda s: nd_dx(s, n, C.byref(G), L, x.data_ptr(), table.data_ptr(), False, C.byref(vd), part.data_ptr(), dx.data_ptr()), 0),
            "bbi_all": (lambda s: nd_bbi(s, n, C.byref(G), L, x.data_ptr(), table.data_ptr(), False, u.data_ptr(), C.byref(vd), g.data_ptr(),
                                         C.byref(vq), 0, part.data_ptr(), dx.data_ptr()), 1),
        }
        for kname, (f, per_corner) in kernels.items():
            rec = {"case": name, "kernel": kname, **shape, **measure({"new": f})}
            if per_corner:
                atomics(rec, G, per_corner)
            emit(rec)
        assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(dx).all())
    lines.append(json.dumps({"summary": "bench_grid_nd", "device": torch.cuda.get_device_name(0), "launches_per_window": a.launches,
                             "windows": a.windows, "warmup": a.warmup, "chip_wide_atomic_rate_TBps": ATOMIC_RATE / 1e12}))
    print(lines[-1])
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
