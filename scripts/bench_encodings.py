#!/usr/bin/env python3
"""Times the encoding kernel that writes a FullyFusedMLP's fp16 input rows X0 [n][in_pad] (encodings.hip,
launch_pf_rows) against k_ff_input (ffmlp.hip, launch_ff_input: the Identity kernel, which writes the same n in_pad
halves with no arithmetic) at n = 2^18:

    sh4         SphericalHarmonics(4)                                      3 dims -> in_pad 16
    freq6       Frequency(3, F = 6)                                        3 dims -> in_pad 48
    composite   [Identity(6) | SphericalHarmonics(4)]                      9 dims -> in_pad 32 (22 columns + 10 ones)
    tri12       TriangleWave(3, F = 12)                                    3 dims -> in_pad 48 (36 columns + 12 ones)
    oneblob64   OneBlob(2, n_bins = 64)                                    2 dims -> in_pad 128
    nrc         NRC: [TriangleWave(3, 12) | OneBlob(5, 4) | Identity(1)]   9 dims -> in_pad 64 (57 columns + 7 ones)

Both launchers are C++ functions of libneus2_hip.so (not part of the C ABI); they are found by name in the library's
dynamic symbol table and called through ctypes with their by-reference arguments as pointers. A kernel of a few
microseconds cannot be timed through per-launch host calls (the host would be the limit), so --launches launches of each
kernel are captured once into a graph on one stream; timing is by HIP events (torch.cuda.Event) around one replay
(= one window), after --warmup eager launches and one untimed replay of each; the two kernels alternate window by window,
so both see the same machine. Reported per kernel: the median, the
fastest and the 10th / 90th percentile window (per launch), the bytes the algorithm needs per sample (4 D in + 2 in_pad out)
over the median, and that rate over the HBM peak of 8 TB/s. At these sizes (4 - 36 MB) the rows fit the 256 MB Infinity
Cache, so the share is of a bound the kernel is not actually held to: read it as a common scale for the two kernels.
One process; the whole run stops at --time-limit seconds. One JSON line per case, the last line a summary.

    python scripts/bench_encodings.py [--cases sh4,freq6,composite] [--log profiles/encodings_bench.log]
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
HBM_PEAK = 8.0e12

PF_IDENTITY, PF_FREQUENCY, PF_SH, PF_TRIANGLE_WAVE, PF_ONEBLOB = 0, 1, 2, 3, 4


class PfSegment(C.Structure):
    _fields_ = [("type", C.c_uint32), ("in0", C.c_uint32), ("dims", C.c_uint32), ("out0", C.c_uint32), ("param", C.c_uint32),
                ("scale", C.c_float), ("offset", C.c_float)]


class PfEnc(C.Structure):
    _fields_ = [("n_seg", C.c_uint32), ("n_in", C.c_uint32), ("width", C.c_uint32), ("seg", PfSegment * 8)]


def descriptor(segments):
    """segments: (type, dims, param, scale, offset) in order"""
    E = PfEnc()
    for i, (ty, dims, param, scale, offset) in enumerate(segments):
        w = {PF_SH: param * param, PF_FREQUENCY: 2 * dims * param, PF_TRIANGLE_WAVE: dims * param, PF_ONEBLOB: dims * param}.get(ty, dims)
        E.seg[i] = PfSegment(ty, E.n_in, dims, E.width, param, scale, offset)
        E.n_in += dims
        E.width += w
    E.n_seg = len(segments)
    return E


CASES = {
    "sh4": [(PF_SH, 3, 4, 1.0, 0.0)],
    "freq6": [(PF_FREQUENCY, 3, 6, 1.0, 0.0)],
    "composite": [(PF_IDENTITY, 6, 0, 1.0, 0.0), (PF_SH, 3, 4, 1.0, 0.0)],
    "tri12": [(PF_TRIANGLE_WAVE, 3, 12, 1.0, 0.0)],
    "oneblob64": [(PF_ONEBLOB, 2, 64, 1.0, 0.0)],
    "nrc": [(PF_TRIANGLE_WAVE, 3, 12, 1.0, 0.0), (PF_ONEBLOB, 5, 4, 1.0, 0.0), (PF_IDENTITY, 1, 0, 1.0, 0.0)],
}


def launcher(lib_path, name):
    out = subprocess.run(["nm", "-D", "--defined-only", lib_path], capture_output=True, text=True, check=True).stdout
    syms = [l.split()[-1] for l in out.splitlines() if name in l and " T " in l]
    if len(syms) != 1:
        raise RuntimeError(f"{name}: expected one exported symbol, found {syms}")
    return syms[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 18)
    ap.add_argument("--launches", type=int, default=2000, help="launches per timed window")
    ap.add_argument("--windows", type=int, default=21, help="timed windows per kernel")
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--time-limit", type=int, default=240)
    ap.add_argument("--cases", default=",".join(CASES), help="comma-separated case names")
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    signal.alarm(a.time_limit)  # the default action ends the process
    import numpy as np
    import torch
    from neus2_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("bench_encodings: needs a GPU (no fallback)")
    lib = _lib.lib()
    pf_rows = getattr(lib, launcher(_lib.LIB_PATH, "launch_pf_rows"))
    ff_input = getattr(lib, launcher(_lib.LIB_PATH, "launch_ff_input"))
    pf_rows.restype = ff_input.restype = None
    pf_rows.argtypes = [C.c_void_p, C.POINTER(PfEnc), C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
    ff_input.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_bool]
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    n = a.n
    lines = []
    for name in a.cases.split(","):
        E = descriptor(CASES[name])
        D, in_pad = E.n_in, (E.width + 15) // 16 * 16
        x = torch.from_numpy(np.random.default_rng(0).uniform(0, 1, (n, D)).astype(np.float32)).cuda()
        rows = torch.zeros((n, in_pad), dtype=torch.float16, device="cuda")
        base = torch.zeros((n, in_pad), dtype=torch.float16, device="cuda")
        new = lambda: pf_rows(stream, C.byref(E), n, x.data_ptr(), None, rows.data_ptr(), in_pad)
        old = lambda: ff_input(stream, n, D, in_pad, x.data_ptr(), 1.0, 0.0, base.data_ptr(), False)
        for f in (new, old):
            for _ in range(a.warmup):
                f()
        torch.cuda.synchronize()
        assert bool((rows[:, E.width:] == 1).all()) and bool(torch.isfinite(rows).all())
        graphs = {}
        for key, f in (("new", new), ("baseline", old)):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                cap = C.c_void_p(torch.cuda.current_stream().cuda_stream)
                for _ in range(a.launches):
                    if key == "new":
                        pf_rows(cap, C.byref(E), n, x.data_ptr(), None, rows.data_ptr(), in_pad)
                    else:
                        ff_input(cap, n, D, in_pad, x.data_ptr(), 1.0, 0.0, base.data_ptr(), False)
            g.replay()
            graphs[key] = g
        torch.cuda.synchronize()
        t = {"new": [], "baseline": []}
        for _ in range(a.windows):
            for key in ("new", "baseline"):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                graphs[key].replay()
                e1.record()
                e1.synchronize()
                t[key].append(e0.elapsed_time(e1) * 1e3 / a.launches)  # us per launch
        nbytes = n * (4 * D + 2 * in_pad)
        rec = {"case": name, "n": n, "n_input_dims": D, "width": E.width, "in_pad": in_pad, "bytes": nbytes}
        for key, v in t.items():
            v = np.sort(np.asarray(v))
            med = float(np.median(v))
            rec[key] = {"median_us": round(med, 3), "min_us": round(float(v[0]), 3), "p10_us": round(float(np.percentile(v, 10)), 3),
                        "p90_us": round(float(np.percentile(v, 90)), 3), "GBps": round(nbytes / med / 1e3, 1),
                        "hbm_share": round(nbytes / (med * 1e-6) / HBM_PEAK, 4)}
        b = rec["baseline"]
        rec["new_over_baseline"] = round(rec["new"]["median_us"] / b["median_us"], 4)
        rec["baseline_spread"] = round((b["p90_us"] - b["p10_us"]) / b["median_us"], 4)
        rec["no_slower_beyond_spread"] = rec["new"]["median_us"] <= b["median_us"] * (1 + rec["baseline_spread"])
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    lines.append(json.dumps({"summary": "bench_encodings", "device": torch.cuda.get_device_name(0), "launches_per_window": a.launches,
                             "windows": a.windows, "warmup": a.warmup}))
    print(lines[-1])
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
