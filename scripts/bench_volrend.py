#!/usr/bin/env python3
"""Times the rendering operators of neus2_amd/volrend.py (volrend.hip) against the fp32 stock-PyTorch formulation of
tests/volrend_ref.py (what one writes without them: a global cumsum of log1p(-alpha) with per-ray offsets, the early stop
as a mask, index_add sums) on the same GPU, at S = 2^18 samples in two ray-length distributions:

    late    mean 16 samples per ray, R = 16384, geometric lengths (a trained occupancy grid)
    early   mean 256 samples per ray, R = 1024, geometric lengths (the first steps)

C = 7 value columns (rgb, depth, normal). Timed per distribution: neus_alpha forward and forward + backward, composite
forward and forward + backward (through autograd, cotangents on out, opacity and weights), each for the operator and the
baseline; the backward alone is the difference of the two medians. march is timed alone (its two kernels, G = 128, without
the host's scan between them) and has no baseline.

Method (that of scripts/bench_encodings.py): a call of a few microseconds cannot be timed through per-launch host calls, so
--launches calls are captured once into a graph; a window is one replay between two HIP events; operator and baseline
alternate window by window, so both see the same machine. Reported: the median and the 10th / 90th percentile window per
call, the bytes the kernels must move (inputs read once, outputs written once; the zero fills of the Python layer are not
counted) and that rate over the HBM peak of 8 TB/s. At these sizes the tensors fit the 256 MB Infinity Cache: read the share
as a common scale, not as a bound that holds the kernel. One JSON line per case, the last line a summary.

    python scripts/bench_volrend.py [--log profiles/volrend_bench.log]
"""
import argparse
import ctypes as C
import json
import os
import signal
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-samples", type=int, default=18)
    ap.add_argument("--channels", type=int, default=7)
    ap.add_argument("--launches", type=int, default=100, help="calls per timed window")
    ap.add_argument("--windows", type=int, default=15, help="timed windows per side")
    ap.add_argument("--time-limit", type=int, default=420)
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    signal.alarm(a.time_limit)  # the default action ends the process
    import numpy as np
    import torch
    import volrend_ref as VR
    from neus2_amd import _lib, volrend
    if not torch.cuda.is_available():
        raise SystemExit("bench_volrend: needs a GPU (no fallback)")
    S, Cn = 1 << a.log2_samples, a.channels
    lines = []

    def timed(pairs):
        """pairs: {side: callable}; returns {side: sorted us per call} over alternating graph-replay windows."""
        graphs = {}
        for side, f in pairs.items():
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                for _ in range(3):
                    f()
            torch.cuda.current_stream().wait_stream(s)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                for _ in range(a.launches):
                    f()
            g.replay()
            graphs[side] = g
        torch.cuda.synchronize()
        t = {side: [] for side in pairs}
        for _ in range(a.windows):
            for side, g in graphs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                g.replay()
                e1.record()
                e1.synchronize()
                t[side].append(e0.elapsed_time(e1) * 1e3 / a.launches)
        return {side: np.sort(np.asarray(v)) for side, v in t.items()}

    def record(case, dist, nbytes, t, extra=None):
        rec = {"case": case, "distribution": dist, "n_samples": S, "bytes": nbytes}
        rec.update(extra or {})
        for side, v in t.items():
            med = float(np.median(v))
            rec[side] = {"median_us": round(med, 3), "p10_us": round(float(np.percentile(v, 10)), 3), "p90_us": round(float(np.percentile(v, 90)), 3),
                         "GBps": round(nbytes / med / 1e3, 1), "hbm_share": round(nbytes / (med * 1e-6) / HBM_PEAK, 4)}
        if "baseline" in rec:
            rec["new_over_baseline"] = round(rec["new"]["median_us"] / rec["baseline"]["median_us"], 4)
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        return rec

    rng = np.random.default_rng(0)
    for dist, R, mean in (("late", S // 16, 16), ("early", S // 256, 256)):
        n = rng.geometric(1.0 / mean, R).astype(np.int64)
        n = np.maximum((n * (S / n.sum())).astype(np.int64), 0)
        n[-1] += S - n.sum()  # exactly S samples
        assert n.min() >= 0 and n.sum() == S
        ranges = torch.from_numpy(VR.ranges_of(n)).cuda()
        ray_idx = VR.ray_index(ranges)
        stats = {"n_rays": R, "mean_len": round(float(n.mean()), 2), "max_len": int(n.max()), "long_ray_share": round(float((n > 32).mean()), 4)}
        dev = lambda x, grad=False: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda().requires_grad_(grad)
        sdf, cos = dev(rng.uniform(-0.05, 0.05, S), True), dev(rng.choice([-1.0, 1.0], S) * rng.uniform(0.05, 0.95, S), True)
        dt = dev(np.full(S, VR.DT))
        inv_s = torch.tensor(64.0, device="cuda", requires_grad=True)
        g_a = dev(rng.uniform(-1, 1, S))
        # alphas that let a 256-sample ray pass T = 1e-4 around its middle
        alpha = dev(rng.uniform(0.0, 2 * 9.2 / max(mean, 64) if mean > 64 else 0.3, S), True)
        values = dev(rng.uniform(-1, 1, (S, Cn)), True)
        g_out, g_op, g_w = dev(rng.uniform(-1, 1, (R, Cn))), dev(rng.uniform(-1, 1, R)), dev(rng.uniform(-1, 1, S))

        def alpha_fwd(f):
            return lambda: f(sdf, cos, dt, inv_s, 0.5)

        def alpha_fb(f):
            return lambda: torch.autograd.grad(f(sdf, cos, dt, inv_s, 0.5), (sdf, cos, inv_s), g_a)

        def comp_new():
            return volrend.composite(alpha, values, ranges, 1e-4)[:3]

        def comp_old():
            return VR.composite_stock(alpha, values, ranges, 1e-4, ray_idx)[:3]

        def comp_fb(f):
            return lambda: torch.autograd.grad(f(), (alpha, values), (g_out, g_op, g_w))

        with torch.no_grad():
            fa = record("alpha_forward", dist, 16 * S, timed({"new": alpha_fwd(volrend.neus_alpha), "baseline": alpha_fwd(VR.neus_alpha_stock)}))
            fc = record("composite_forward", dist, 4 * S * (3 + Cn) + 4 * R * (Cn + 4), timed({"new": comp_new, "baseline": comp_old}), stats)
        ba = record("alpha_forward_backward", dist, (16 + 24) * S, timed({"new": alpha_fb(volrend.neus_alpha), "baseline": alpha_fb(VR.neus_alpha_stock)}))
        bc = record("composite_forward_backward", dist, 4 * S * (3 + Cn) + 4 * S * (4 + 2 * Cn) + 8 * R * (Cn + 4),
                    timed({"new": comp_fb(comp_new), "baseline": comp_fb(comp_old)}))
        for name, f, b, nbytes in (("alpha_backward", fa, ba, 24 * S), ("composite_backward", fc, bc, 4 * S * (4 + 2 * Cn) + 4 * R * (Cn + 4))):
            rec = {"case": name, "distribution": dist, "bytes": nbytes, "derived": "forward_backward median - forward median"}
            for side in ("new", "baseline"):
                us = b[side]["median_us"] - f[side]["median_us"]
                rec[side] = {"median_us": round(us, 3), "GBps": round(nbytes / us / 1e3, 1), "hbm_share": round(nbytes / (us * 1e-6) / HBM_PEAK, 4)}
            rec["new_over_baseline"] = round(rec["new"]["median_us"] / rec["baseline"]["median_us"], 4)
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)

    # march alone: its two kernels at G = 128, 30 % occupancy, dt = sqrt(3) / 1024, 4096 rays through the cube
    G, R = 128, 4096
    occ = torch.from_numpy((rng.uniform(0, 1, (G, G, G)) < 0.3).astype(np.uint8)).cuda()
    o = torch.from_numpy(rng.uniform(-0.5, 1.5, (R, 3)).astype(np.float32)).cuda()
    d = torch.nn.functional.normalize(torch.from_numpy(rng.uniform(0.1, 0.9, (R, 3)).astype(np.float32)).cuda() - o, dim=1).contiguous()
    ta, tb = (0.0 - o) / d, (1.0 - o) / d
    t_min, t_max = torch.minimum(ta, tb).amax(1).clamp(min=0.0).contiguous(), torch.maximum(ta, tb).amin(1).contiguous()
    ranges, t, ray_idx = volrend.march(o, d, t_min, t_max, occ, VR.DT, 1024)
    counts = torch.empty(R, dtype=torch.int32, device="cuda")
    l, p = _lib.lib(), lambda x: C.c_void_p(x.data_ptr())

    def march_kernels():
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        args = (s, C.c_uint32(R), p(o), p(d), p(t_min), p(t_max), p(occ), C.c_uint32(G), C.c_float(VR.DT), C.c_uint32(1024))
        _lib.check(l.neus_volrend_march_count(*args, p(counts)))
        _lib.check(l.neus_volrend_march_write(*args, p(ranges), C.c_uint32(len(t)), p(t), p(ray_idx)))

    # per kept sample 8 B written; per step of both passes one occupancy byte read (cached: 2 MB grid)
    record("march_count_and_write", "G=128", 8 * len(t) + 2 * R * 32, timed({"new": march_kernels}),
           {"n_rays": R, "n_samples_out": len(t), "mean_kept_per_ray": round(len(t) / R, 1)})
    lines.append(json.dumps({"summary": "bench_volrend", "device": torch.cuda.get_device_name(0), "launches_per_window": a.launches,
                             "windows": a.windows, "channels": Cn}))
    print(lines[-1])
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
