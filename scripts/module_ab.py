#!/usr/bin/env python3
"""Bitwise A/B of the operator modules' network kernels between two builds of the library (the modules' counterpart of
scripts/golden_params.py, which fingerprints the training step): every output of forward, backward and
backward_backward_input, and initialize_params, of

    relu            HashGrid -> FullyFusedMLP 64 x 2, ReLU (the default chain)
    softplus_exact  HashGrid -> FullyFusedMLP 64 x 2, Softplus, "second_order": "exact" (every curved epilogue)
    softplus_w256   Identity -> CutlassMLP 256 x 2, Softplus, exact (the wide kernels)

on fixed inputs (n = 2176 of a capacity of 4096), written to an .npz. With --compare OTHER.npz every array must equal the
other file's bit for bit (exit status 1 otherwise).

    NEUS2_HIP_LIB=golden_ref/libneus2_hip_base.so python scripts/module_ab.py bench_out/module_base.npz
    python scripts/module_ab.py bench_out/module_new.npz --compare bench_out/module_base.npz
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ENC = {"otype": "HashGrid", "n_levels": 4, "n_features_per_level": 2, "log2_hashmap_size": 9, "base_resolution": 4, "per_level_scale": 2.0}
MODULES = {
    "relu": (ENC, {"otype": "FullyFusedMLP", "activation": "ReLU", "n_neurons": 64, "n_hidden_layers": 2}),
    "softplus_exact": (ENC, {"otype": "FullyFusedMLP", "activation": "Softplus", "n_neurons": 64, "n_hidden_layers": 2, "second_order": "exact"}),
    "softplus_w256": (None, {"otype": "CutlassMLP", "activation": "Softplus", "n_neurons": 256, "n_hidden_layers": 2, "second_order": "exact"}),
}
N, CAP = 2176, 4096


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--compare", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from neus2_amd.module import GradientMode, Module
    if not torch.cuda.is_available():
        raise SystemExit("module_ab: needs a GPU (no fallback)")
    got = {}
    for name, (enc, net) in MODULES.items():
        net = dict(net, output_activation="None", gradient_precision="fp32")
        m = (Module.create_network_with_input_encoding(3, 1, enc, net, batch_capacity=CAP) if enc
             else Module.create_network(3, 1, net, batch_capacity=CAP))
        rng = np.random.default_rng(11)
        p32 = m.initialize_params(seed=5)
        got[f"{name}_init"] = p32.cpu().numpy()
        params = torch.from_numpy(rng.normal(0, 0.15, m.n_params).astype(np.float16).view(np.int16)).cuda()
        x = torch.from_numpy(rng.uniform(0.02, 0.98, (N, 3)).astype(np.float32)).cuda()
        u = torch.from_numpy(rng.normal(0, 1, (N, 3)).astype(np.float32)).cuda()
        g = torch.from_numpy(rng.normal(0, 1, (N, 16)).astype(np.float16).view(np.int16)).cuda()
        ctx, y = m.forward(x, params, prepare_input_gradients=True)
        yi = m.inference(x, params)
        g1 = torch.zeros(m.n_params, dtype=torch.float32, device="cuda")
        dx1 = torch.zeros((N, 3), dtype=torch.float32, device="cuda")
        m.backward(ctx, x, g, params, dL_dparams=g1, dL_dinput=dx1, mode=GradientMode.Overwrite, output=y)
        g2 = torch.zeros(m.n_params, dtype=torch.float32, device="cuda")
        ddo = torch.zeros((N, 16), dtype=torch.float16, device="cuda")
        dx2 = torch.zeros((N, 3), dtype=torch.float32, device="cuda")
        m.backward_backward_input(ctx, x, u, g, params, dL_dparams=g2, dL_ddLdoutput=ddo, mode=GradientMode.Overwrite, dL_dinput=dx2)
        torch.cuda.synchronize()
        for key, v in (("y", y), ("inference", yi), ("bwd_dparams", g1), ("bwd_dinput", dx1), ("bbi_dparams", g2), ("bbi_ddo", ddo), ("bbi_dinput", dx2)):
            arr = v.cpu().numpy()
            assert np.isfinite(arr.astype(np.float32)).all() and np.abs(arr.astype(np.float32)).max() > 0, (name, key)
            got[f"{name}_{key}"] = arr.view(np.uint16 if arr.dtype == np.float16 else np.uint32)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez(a.out, **got)
    print(f"module_ab: {len(got)} arrays -> {a.out}")
    if a.compare:
        other = np.load(a.compare)
        bad = [k for k in got if k not in other or not np.array_equal(got[k].view(np.uint8), other[k].view(np.uint8))]
        for k in got:
            print(f"  {k}: {'DIFFERS' if k in bad else 'bitwise equal'}")
        if bad or set(other.files) != set(got):
            print("MODULE_AB_MISMATCH")
            raise SystemExit(1)
        print("MODULE_AB_EQUAL")


if __name__ == "__main__":
    main()
