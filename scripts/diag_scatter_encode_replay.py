"""Replays the grid scatter and the training encode (neus_testbed_time_kernel ids 7 and 8, as bench.py --full does) on
the bench-shaped training state after WARM steps: the launches to count under `rocprofv3 --pmc ... --kernel-include-regex
"k_scatter_bin_r|k_scatter_accum_r|k_grid_encode"` (counters in a run of their own, no tracing options). With a
directory argument it instead reads that run's counter CSV and prints per kernel the mean of every counter over the
replayed launches (the last ITERS of each kernel)."""
import csv, glob, os, re, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ITERS = int(os.environ.get("ITERS", "5"))


def table(d):
    f = glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True)[0]
    acc = {}
    for r in csv.DictReader(open(f)):
        k = re.sub(r"^void |neus::|\(.*", "", r["Kernel_Name"])
        acc.setdefault(k, {}).setdefault(r["Counter_Name"], []).append((int(r["Dispatch_Id"]), float(r["Counter_Value"])))
    names = sorted({c for v in acc.values() for c in v})
    print("| kernel | launches | " + " | ".join(names) + " |")
    print("|---|---:|" + "---:|" * len(names))
    for k, v in sorted(acc.items()):
        last = {c: [x for _, x in sorted(v[c])[-ITERS:]] for c in v}
        print(f"| `{k}` | {len(next(iter(last.values())))} | " + " | ".join(f"{sum(last[c]) / len(last[c]):.4g}" if c in last else "-" for c in names) + " |")


if len(sys.argv) > 1:
    table(sys.argv[1])
    sys.exit(0)
sys.path.insert(0, ROOT)
import torch
from neus2_amd import pyngp, scenes
torch.cuda.set_device(0)
sc = scenes.sphere_scene(49, 1600, 1200, principal=(823.2 / 1600, 619.1 / 1200))
tb = pyngp.Testbed(pyngp.TestbedMode.Nerf)
tb.set_dataset(sc["images"], sc["focal"], sc["principal"], sc["xforms"], 1)
tb.reload_network_from_file(os.path.join(ROOT, "configs", "nerf", "base.json"), batch_size=1 << 18, fixed_rays_per_batch=1 << 18)
tb.train_steps(int(os.environ.get("WARM", "800")))
for name, kid in (("grid_scatter", 7), ("train_encode", 8)):
    ms, units = tb.time_kernel(kid, ITERS)
    print(f"{name}: {ms * 1e3:.1f} us over {units} samples", flush=True)
