"""GPU parity of the training-step pieces around the network: the Ema(Adam) optimizer, the occupancy-grid
update, fill_rollover and a free-running multi-step train trajectory, each through the C-ABI against the
CPU oracle (oracle/neus_oracle.cpp, oracle/cpu_step.py) on the same seeded inputs."""
import ctypes as C
import os

import numpy as np
import pytest

from gpu_util import dev, host, ptr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH = 4096


def _lib():
    from neus2_amd._lib import check, lib
    return lib(), check


def _record(test, **metrics):
    import json
    os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
    with open(os.path.join(ROOT, "gpurun_out", "parity_metrics.jsonl"), "a") as f:
        f.write(json.dumps({"test": test, **{k: float(v) for k, v in metrics.items()}}) + "\n")


def _testbed(sc, batch=BATCH, config="base.json", **kw):
    from neus2_amd import pyngp
    tb = pyngp.Testbed(pyngp.TestbedMode.Nerf)
    tb.set_dataset(sc["images"], sc["focal"], sc["principal"], sc["xforms"], 1)
    tb.reload_network_from_file(os.path.join(ROOT, "configs", "nerf", config), batch_size=batch, **kw)
    return tb


@pytest.fixture(scope="module")
def scene(torch_cuda):
    from neus2_amd import scenes
    return scenes.small_scene(n_views=8, width=64, height=48)


@pytest.mark.parametrize("beta2", [0.99999, 0.99])
def test_optimizer_step_counts_width(scene, torch_cuda, beta2):
    """per-parameter Adam step counts (uint32 in the reference, adam.h:106). With betas whose bias correction has
    not converged by step 4096 (beta2 = 0.99999) the device keeps them in 32 bits: a state with counts far above 65535
    round-trips exactly, and one step at those counts matches the oracle's Adam (bias correction at the true count). With
    the default betas (0.99: converged) they are 16-bit and read back saturated at 65535, and the step still matches the
    oracle at the true counts, since every count past 4095 gives the same update."""
    import oracle as O
    from neus2_amd import config as _config
    from neus2_amd import pyngp
    t = torch_cuda
    lib, check = _lib()
    cfg = _config.load_json(os.path.join(ROOT, "configs", "nerf", "base.json"))
    cfg["optimizer"]["nested"]["nested"]["beta2"] = beta2
    tb = pyngp.Testbed(pyngp.TestbedMode.Nerf)
    tb.set_dataset(scene["images"], scene["focal"], scene["principal"], scene["xforms"], 1)
    tb.reload_network_from_json(cfg, batch_size=BATCH)
    lay = tb.layout()
    P, n_matrix = lay["n_params"], lay["n_matrix"]
    rng = np.random.default_rng(4)
    st = tb.get_optimizer_state()
    steps = rng.integers(0, 200000, P).astype(np.uint32)
    steps[:64] = 65535 + np.arange(64, dtype=np.uint32)
    # moments of a unit-variance gradient (the step's gradient / loss scale below): updates of O(lr)
    m1 = rng.normal(0, 0.1, P).astype(np.float32)
    m2 = rng.uniform(0.5, 1.5, P).astype(np.float32)
    st.update(current_step=10, param_steps=steps, m1=m1, m2=m2)
    tb.set_optimizer_state(st)
    back = tb.get_optimizer_state()["param_steps"]
    wide = beta2 == 0.99999
    np.testing.assert_array_equal(back, steps if wide else np.minimum(steps, 65535))
    w = tb.get_params().copy()
    g = rng.normal(0, 1.0, P).astype(np.float32) * 128.0
    g[rng.random(P) < 0.3] = 0.0
    check(lib.neus_optimizer_step(tb.handle, None, ptr(dev(t, g))))
    s_o, e_tmp, e_out = steps.copy(), np.zeros(P, np.float32), np.zeros(P, np.float32)
    O.adam_ema_step(w, g, m1, m2, s_o, e_tmp, e_out, n_matrix, 11, lr=1e-3, beta1=0.9, beta2=beta2, eps=1e-15, l2=1e-6)
    got = tb.get_params()
    dw = np.abs(got - w) / np.maximum(np.abs(w), 1e-3)
    assert dw.max() <= 2e-6, (dw.argmax(), got[dw.argmax()], w[dw.argmax()])
    back = tb.get_optimizer_state()["param_steps"]
    np.testing.assert_array_equal(back, s_o if wide else np.minimum(s_o, 65535))


def test_optimizer_step_parity(scene, torch_cuda):
    """Trainer::optimizer_step = Ema(ExponentialDecay(Adam)) (adam.h:51-160, ema.h:45-110) for three steps
    against or_adam_ema_step: fp32 master weights and the fp32 EMA within 2e-6 relative to max(|w|, lr) (device
    powf/sqrtf vs libm: an ulp or two of the update; a weight that a step brings near zero keeps the absolute
    error of the O(lr) terms it cancelled). Covers the zero-gradient skip of non-matrix (grid, variance) params, the L2 term
    and per-parameter step counts (a grid param first updated at step 2 gets step-1 bias correction)."""
    import oracle as O
    t = torch_cuda
    lib, check = _lib()
    tb = _testbed(scene)
    lay = tb.layout()
    P, n_matrix, g0, v0 = lay["n_params"], lay["n_matrix"], lay["grid_offset"], lay["variance_offset"]
    w = tb.get_params().copy()
    m1, m2 = np.zeros(P, np.float32), np.zeros(P, np.float32)
    steps = np.zeros(P, np.uint32)
    ema_tmp, ema_out = np.zeros(P, np.float32), np.zeros(P, np.float32)
    rng = np.random.default_rng(3)
    w_init = w.copy()
    for k in range(3):
        g = rng.normal(0, 1.0, P).astype(np.float32) * 128.0
        zero = rng.random(P) < 0.3
        zero[:n_matrix] = rng.random(n_matrix) < 0.1  # zero matrix grads still take the L2 + momentum update
        if k == 0:
            zero[v0:] = True  # variance untouched at step 1: its first update is at step 2
        g[zero] = 0.0
        check(lib.neus_optimizer_step(tb.handle, None, ptr(dev(t, g))))
        O.adam_ema_step(w, g, m1, m2, steps, ema_tmp, ema_out, n_matrix, k + 1, lr=1e-3, beta1=0.9, beta2=0.99, eps=1e-15, l2=1e-6)
        got = tb.get_params()
        got_ema = tb.get_ema_params()
        dw = np.abs(got - w) / np.maximum(np.abs(w), 1e-3)
        de = np.abs(got_ema - ema_tmp) / np.maximum(np.abs(ema_tmp), 1e-4)
        _record(f"adam_step{k + 1}", max_rel_w=dw.max(), max_rel_ema=de.max(), frac_ema_gt_2e6=(de > 2e-6).mean())
        assert dw.max() <= 2e-6, (k, dw.argmax(), got[dw.argmax()], w[dw.argmax()])
        # the EMA averages the fp16 copy of the weights: a last-ulp fp32 difference can round a weight to the
        # neighbouring half: one fp16 ulp (2^-10 relative) on that parameter's EMA, which the later steps carry
        assert de.max() <= 2 ** -9, (k, de.argmax())
        assert (de > 2e-6).mean() <= 5e-4, (k, (de > 2e-6).mean())
    # a grid param whose gradient was zero every step never moved; the variance moved from step 2 on
    still = w[g0:v0] == w_init[g0:v0]  # grid params the oracle never updated
    assert still.sum() > 0
    np.testing.assert_array_equal(got[g0:v0][still], w_init[g0:v0][still])
    assert got[v0] != w_init[v0]
    # the update is Adam, not its sign: |dw| at step 3 varies across params (sign-SGD would give lr for all)
    assert np.std(np.abs(got[:n_matrix] - w_init[:n_matrix])) > 1e-5


def test_fill_rollover_parity(scene, torch_cuda):
    """fill_rollover_and_rescale (common_device.h:515-535) bit-exact vs or_fill_rollover, ragged n_in."""
    import oracle as O
    t = torch_cuda
    lib, check = _lib()
    tb = _testbed(scene)
    rng = np.random.default_rng(9)
    n = 4096
    for n_in in (1, 1000, 4095, 4096, 5000, 0):
        co = rng.uniform(0, 1, (n, 7)).astype(np.float32)
        dl = rng.normal(0, 1, (n, 16)).astype(np.float16).view(np.uint16)
        cd, dd = dev(t, co), dev(t, dl)
        check(lib.neus_fill_rollover(tb.handle, None, C.c_uint32(n), C.c_uint32(n_in), ptr(cd), ptr(dd)))
        rc, rd = co.copy(), dl.copy()
        O.fill_rollover(n, min(n_in, n), rc, rd)
        np.testing.assert_array_equal(host(cd, np.uint32), rc.view(np.uint32))
        np.testing.assert_array_equal(host(dd, np.uint16), rd)


def test_occupancy_update_parity(scene, torch_cuda):
    """update_density_grid_nerf (testbed_nerf.cu:3293-3397): sample positions/cells from density_grid_rng,
    NerfNetwork::density, splat max, EMA, mean, bitfield + 8 max-pooled mips, against or_density_grid_update.
    Step 0 (all 128^3 cells uniform) and step 1 (quarter uniform + quarter occupied-biased, valid level 3) on
    trained parameters. The device density runs through the fused fp16 MFMA kernel, so grid values are
    compared with an fp16-accumulation tolerance and the bitfield by mismatch fraction (a cell flips only when
    its density sits at the threshold)."""
    import oracle as O
    lib, check = _lib()
    tb = _testbed(scene)
    cfg = O.make_cfg(per_level_scale=tb._net_cfg.per_level_scale)
    G3 = 128 ** 3

    def compare(tag, grid_prev, n_u, n_nu, ema_step, valid):
        rs, ri = tb.get_rng()[2:4]
        params = tb.get_params()
        check(lib.neus_occ_update(tb.handle, None, C.c_uint32(n_u), C.c_uint32(n_nu)))
        g, bf = tb.get_density_grid()
        rg = grid_prev.copy()
        rbf = np.zeros(G3 // 8 * 8, np.uint8)
        st, mean = O.density_grid_update(cfg, params, valid, n_u, n_nu, ema_step, rs, ri, rg, rbf)
        assert tb.get_rng()[2] == st  # density_grid_rng advanced twice, like the reference
        err = np.abs(g - rg)
        ok = err <= 2e-2 * np.abs(rg) + 2e-3
        bits = np.unpackbits(bf) != np.unpackbits(rbf)
        _record(f"occupancy_{tag}", frac_within_tol=ok.mean(), max_abs=err.max(), bit_mismatch=bits.mean(), mean_ref=mean,
                occupied=np.unpackbits(rbf[: G3 // 8]).mean())
        assert ok.mean() >= 0.999, (tag, ok.mean())
        assert bits.mean() <= 2e-3, (tag, bits.mean())
        assert np.unpackbits(rbf[: G3 // 8]).mean() > 0.001  # the test exercises occupied cells
        return g

    compare("step0", np.zeros(G3, np.float32), G3, 0, 0, 14)
    # one training step (its occupancy update restarts the grid at step 0), then the step-1 update on its state
    tb.train_steps(1)
    g_prev, _ = tb.get_density_grid()
    compare("step1", g_prev, G3 // 4, G3 // 4, 1, 3)


def test_train_trajectory_vs_oracle(scene, torch_cuda):
    """24 free-running Testbed::train steps (adaptive rays per batch, occupancy updates at the reference
    cadence, Adam + EMA) on the device and in oracle/cpu_step.py from the same initial parameters. The two
    runs see the same rays; the fp16 network noise can move a transmittance cut-off or an occupancy cell, so
    the trajectories are compared by statistics: per-step compacted counts and rays per batch close, and the
    parameter change of every block pointing the same way (cosine) with a bounded relative L2 difference."""
    import oracle as O
    from cpu_step import CpuTrainer
    tb = _testbed(scene)
    lay = tb.layout()
    p0 = tb.get_params()
    cfg = O.make_cfg(per_level_scale=tb._net_cfg.per_level_scale)
    ds = O.Dataset(scene["images"], scene["focal"], scene["principal"], scene["xforms"])
    tr = CpuTrainer(cfg, ds, p0, batch=BATCH, rays_per_batch=BATCH)
    n_steps = 24
    gpu_R, cpu_R, gpu_c, cpu_c = [], [], [], []
    for _ in range(n_steps):
        gpu_R.append(tb.stats()["rays_per_batch"])
        cpu_R.append(tr.R)
        tb.train_steps(1)
        tr.step()
        gpu_c.append(tb.stats()["measured_batch_size"])
        cpu_c.append(tr.last["compacted"])
    gpu_c, cpu_c = np.array(gpu_c, np.float64), np.array(cpu_c, np.float64)
    rel_c = np.abs(gpu_c - cpu_c) / cpu_c
    dR = np.abs(np.array(gpu_R) - np.array(cpu_R))
    p_gpu = tb.get_params().astype(np.float64)
    p_cpu = tr.params.astype(np.float64)
    blocks = {"density": (0, lay["n_density"]), "rgb": (lay["n_density"], lay["n_matrix"]),
              "grid": (lay["grid_offset"], lay["variance_offset"]), "variance": (lay["variance_offset"], lay["variance_offset"] + 1)}
    res = {}
    for name, (a, b) in blocks.items():
        x, y = p_gpu[a:b] - p0[a:b], p_cpu[a:b] - p0[a:b]
        res[name] = (x @ y / max(np.linalg.norm(x) * np.linalg.norm(y), 1e-30), np.linalg.norm(x - y) / max(np.linalg.norm(y), 1e-30))
    # per hash-grid level drift of the parameter change (a systematic error confined to one level shows here)
    off, _, _, _ = O.grid_tables(cfg)
    g0 = lay["grid_offset"]
    lev = {}
    for l in range(len(off) - 1):
        a, b = g0 + 2 * int(off[l]), g0 + 2 * int(off[l + 1])
        x, y = p_gpu[a:b] - p0[a:b], p_cpu[a:b] - p0[a:b]
        if np.linalg.norm(y) > 0:
            lev[l] = (x @ y / max(np.linalg.norm(x) * np.linalg.norm(y), 1e-30), np.linalg.norm(x - y) / np.linalg.norm(y))
    _record("trajectory", max_rel_compacted=rel_c.max(), max_dR=dR.max(), steps=n_steps,
            **{f"cos_{k}": v[0] for k, v in res.items()}, **{f"rel_{k}": v[1] for k, v in res.items()},
            **{f"rel_grid_L{l}": v[1] for l, v in lev.items()}, **{f"cos_grid_L{l}": v[0] for l, v in lev.items()})
    for l, (cos, rel) in lev.items():
        assert cos >= 0.95 and rel <= 0.35, (l, cos, rel)
    assert rel_c.max() <= 0.01, (gpu_c, cpu_c)
    assert dR.max() <= 256, (gpu_R, cpu_R)
    assert gpu_R[0] == cpu_R[0] == BATCH
    for name, (cos, rel) in res.items():
        if name == "variance":
            assert np.sign(p_gpu[blocks[name][0]] - p0[blocks[name][0]]) == np.sign(p_cpu[blocks[name][0]] - p0[blocks[name][0]])
            continue
        assert cos >= 0.98 and rel <= 0.25, (name, cos, rel)


def test_teacher_forced_steps_vs_oracle(scene, torch_cuda):
    """Teacher-forced training: 24 consecutive Testbed::train steps (100..123 after 100 free-running ones: the
    progressive valid level moves from 3 to 4 at step 111 (grid.h:2427-2440), the occupancy grid is updated at steps
    102, 108, 112 and 119), each compared with the oracle's step from the device's state before it: parameters, rays per
    batch, rng, n_rays_total, the pre-compaction cap, and the occupancy grid the step sampled with (the device's, after
    the step's own update, which runs before the sampling). Per step: the march is bit-exact (requested samples, kept
    samples), the compacted count equal up to the transmittance cut-offs that fp16 network noise moves, the rays-per-
    batch adaptation equal, and every gradient block (density MLP, colour MLP, hash grid, variance) within single-step
    tolerance: cosine >= 0.9999 and rel-L2 <= 2e-3 (measured on MI355X: every step's compacted count equal, grid rel-L2
    <= 5.5e-4, profiles/r03b_parity_metrics.jsonl)."""
    import oracle as O
    from cpu_step import CpuTrainer
    tb = _testbed(scene)
    tb.train_steps(100)
    lay = tb.layout()
    cfg = O.make_cfg(per_level_scale=tb._net_cfg.per_level_scale)
    ds = O.Dataset(scene["images"], scene["focal"], scene["principal"], scene["xforms"])
    tr = CpuTrainer(cfg, ds, tb.get_params(), batch=BATCH, rays_per_batch=BATCH)
    blocks = {"density": (0, lay["n_density"]), "rgb": (lay["n_density"], lay["n_matrix"]),
              "grid": (lay["grid_offset"], lay["variance_offset"]), "variance": (lay["variance_offset"], lay["variance_offset"] + 1)}
    worst = {k: [1.0, 0.0] for k in blocks}
    levels = set()
    n_comp_equal = 0
    max_comp = 0.0
    for k in range(24):
        st = tb.stats()
        rng = tb.get_rng()
        tr.params = tb.get_params().copy()
        tr.R = st["rays_per_batch"]
        tr.training_step = st["training_step"]
        tr.n_rays_total = st["n_rays_total"]
        tr.rng_state, tr.rng_inc = rng[0], rng[1]
        before = st["measured_batch_size_before_compaction"]
        tr.max_inference = (min(before, tr.max_samples) + 127) // 128 * 128 if before else tr.max_samples
        levels.add(tr.valid_level(tr.training_step))
        tb.train_steps(1)
        g = tb.get_gradients().astype(np.float64)
        grid, bf = tb.get_density_grid()
        st1 = tb.stats()
        tr.density_grid[:] = grid
        tr.bitfield[:] = bf
        gr = tr.grads(skip_occupancy=True).astype(np.float64)
        assert st1["measured_batch_size_before_compaction"] == tr.last["numsteps_counter"], k
        comp_d, comp_o = st1["measured_batch_size"], tr.last["compacted"]
        n_comp_equal += comp_d == comp_o
        max_comp = max(max_comp, abs(comp_d - comp_o) / max(comp_o, 1))
        assert abs(comp_d - comp_o) <= max(2, 1e-3 * comp_o), (k, comp_d, comp_o)
        if comp_d == comp_o:
            measured = comp_o
            r = int(np.float32(tr.R) * np.float32(BATCH) / np.float32(measured))
            assert st1["rays_per_batch"] == min((r + 127) // 128 * 128, 1 << 18), k
        for name, (a, b) in blocks.items():
            x, y = g[a:b], gr[a:b]
            cos = x @ y / max(np.linalg.norm(x) * np.linalg.norm(y), 1e-30)
            rel = np.linalg.norm(x - y) / max(np.linalg.norm(y), 1e-30)
            worst[name][0] = min(worst[name][0], cos)
            worst[name][1] = max(worst[name][1], rel)
    _record("teacher_forced_24", steps=24, compacted_equal_steps=n_comp_equal, max_rel_compacted=max_comp,
            levels_min=min(levels), levels_max=max(levels),
            **{f"min_cos_{k}": v[0] for k, v in worst.items()}, **{f"max_rel_{k}": v[1] for k, v in worst.items()})
    assert len(levels) >= 2  # the span crosses a progressive-level change
    for name, (cos, rel) in worst.items():
        assert cos >= 0.9999 and rel <= 2e-3, (name, cos, rel)


def _progress(msg):
    """A progress line under gpurun_out/ (long oracle comparisons keep the GPU call visibly alive)."""
    import time
    os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
    with open(os.path.join(ROOT, "gpurun_out", "progress.log"), "a") as f:
        f.write(f"{time.strftime('%H:%M:%S')} {msg}\n")


FLOOR_ORDERS = ("reversed", "pairwise", "blocked")


def _variance_sum_depth(batch):
    """Longest chain of fp32 additions a term of the variance gradient's batch sum passes through (mlp.hip
    k_mlp_train_rgb, k_mlp_grad_reduce): the lane's serial loop over its wave's 32-sample chunks - the grid is
    min(batch / 128, resident workgroups) workgroups of 4 waves, and at least one workgroup is resident on each of the 256
    CUs; the 6-step shuffle tree; (s0 + s1) + (s2 + s3) over the workgroup's waves; in the reduction thread t's strided
    loop over the workgroup partials t, t + 256, ... (at most 2048 of them) and the 8-step tree over the 256 threads."""
    blocks_min = min(-(-batch // 128), 256)
    blocks_max = min(-(-batch // 128), 2048)
    return -(-batch // (128 * blocks_min)) + 6 + 2 + -(-blocks_max // 256) + 8


def _teacher_forced_all_levels(sc, tag, progressive, n_steps=14, prepare=700, short_step=5, fixed_rays=False, prepare_batch=None,
                               batch=BATCH, floor_factor=1.5, level_bar=True):
    """Teacher-forced training at the all-levels state: the device trains `prepare` free-running steps
    first, so all 14 levels are active (hashed levels 5-13: 2^19-entry tables, the 2048-entry region scatter of hashed
    buckets) and the occupancy grid is shaped by hundreds of updates. Then n_steps consecutive steps, each compared with
    the oracle's step from the device's state before it (as test_teacher_forced_steps_vs_oracle). One step runs with half
    the rays, so its compacted count is below the batch and the rollover fused into k_grid_encode fills the rest
    (fill_rollover_and_rescale, common_device.h:515-535). Per step: the march bit-exact, the compacted count equal up to
    fp16-moved cut-offs, every gradient block cos >= 0.9999 and rel-L2 <= max(2e-3, floor_factor x the noise floor); per
    hash level the worst rel-L2 is asserted the same way against that level's floor (round 6; level_bar) and recorded beside
    the distance of the reference's own fp16 operand (each corner contribution rounded to fp16, grid.h:418-421: the
    oracle's "ref_operand" mode) from the exact sum. The noise floor of a block is the largest rel-L2 between the oracle's step and
    the same oracle step with the network's layer products summed in another order (reversed, pairwise, blocked): the
    spread any fp32 accumulation order has on a network with fp16 activations. progressive: None leaves the auto rule on
    (asserted to have run the rounds), 2 forces the rounds. fixed_rays: R fixed at this many rays every step
    (fixed_rays_per_batch; no short step there: the rays composite more than Nc samples). prepare_batch: the `prepare` steps
    run in a second testbed at this batch (and as many fixed rays), whose parameters, optimizer state, occupancy grid and
    step count are then moved into the `batch`-sample one. Returns the per-step records.
    Reference: testbed_nerf.cu:3723-4001, grid.h:371-500, 880-1007, 2427-2440."""
    import ctypes as C
    import oracle as O
    from cpu_step import CpuTrainer
    from neus2_amd._lib import NeusRestoreState, check, lib
    tb = _testbed(sc, batch=batch, fixed_rays_per_batch=fixed_rays) if fixed_rays else _testbed(sc, batch=batch)
    if progressive is not None:
        tb.set_progressive_inference(progressive, (32, 64, 96))
    if prepare_batch:
        big = _testbed(sc, batch=prepare_batch, fixed_rays_per_batch=prepare_batch)
        big.train_steps(prepare)
        tb.set_params(big.get_params())
        tb.set_optimizer_state(big.get_optimizer_state())
        grid, bf = big.get_density_grid()
        tb.set_density_grid(grid, bf)
        st = big.stats()
        rs = NeusRestoreState(training_step=st["training_step"], rays_per_batch=fixed_rays or batch, measured_batch_size=batch,
                              measured_batch_size_before_compaction=16 * batch, loss=st["loss"], rebuild_bitfield=0)
        check(lib().neus_testbed_restore_state(tb.handle, C.byref(rs)))
        del big
        tb.train_steps(2)  # the auto rule reads the previous step's composited / kept ratio
    else:
        tb.train_steps(prepare)
    _progress(f"{tag}: device prepared ({prepare} steps)")
    lay = tb.layout()
    cfg = O.make_cfg(per_level_scale=tb._net_cfg.per_level_scale)
    assert tb.stats()["valid_level"] + 1 >= cfg.n_levels, "not every level is active"
    ds = O.Dataset(sc["images"], sc["focal"], sc["principal"], sc["xforms"])
    tr = CpuTrainer(cfg, ds, tb.get_params(), batch=batch, rays_per_batch=fixed_rays or batch, fixed_rays=bool(fixed_rays))
    blocks = {"density": (0, lay["n_density"]), "rgb": (lay["n_density"], lay["n_matrix"]),
              "grid": (lay["grid_offset"], lay["variance_offset"]), "variance": (lay["variance_offset"], lay["variance_offset"] + 1)}
    off, _, _, _ = O.grid_tables(cfg)
    g0 = lay["grid_offset"]
    worst = {k: [1.0, 0.0] for k in blocks}
    floor = {k: 0.0 for k in blocks}
    floor_by_order = {o: {k: 0.0 for k in blocks} for o in FLOOR_ORDERS}
    lev_rel, lev_floor, lev_refop = np.zeros(cfg.n_levels), np.zeros(cfg.n_levels), np.zeros(cfg.n_levels)
    var_cond = 0.0  # the variance gradient's conditioning bar (below)
    var_exact_ratio = 0.0  # the variance gradient against the device's own column sum: worst error / absolute bar
    var_terms_min = batch  # ... and the fewest nonzero terms of that column over the steps (the check is not vacuous)
    prog0 = tb.stats()["progressive_steps"]
    short_seen, n_comp_equal, later_rounds, evaluated, kept = False, 0, 0, 0, 0
    records = []
    for k in range(n_steps):
        st = tb.stats()
        if short_step is not None and k == short_step:  # half the rays for this step: the compaction falls short of the batch
            rs = NeusRestoreState(training_step=st["training_step"], rays_per_batch=max(128, st["rays_per_batch"] // 256 * 128),
                                  measured_batch_size=st["measured_batch_size"],
                                  measured_batch_size_before_compaction=st["measured_batch_size_before_compaction"], loss=st["loss"],
                                  rebuild_bitfield=0)
            check(lib().neus_testbed_restore_state(tb.handle, C.byref(rs)))
            st = tb.stats()
        rng = tb.get_rng()
        tr.params = tb.get_params().copy()
        tr.R = st["rays_per_batch"]
        tr.training_step = st["training_step"]
        tr.n_rays_total = st["n_rays_total"]
        tr.rng_state, tr.rng_inc = rng[0], rng[1]
        before = st["measured_batch_size_before_compaction"]
        tr.max_inference = (min(before, tr.max_samples) + 127) // 128 * 128 if before else tr.max_samples
        assert tr.valid_level(tr.training_step) == cfg.n_levels
        chunk_end = st["progressive_chunk_end"]
        prog_before = st["progressive_steps"]
        tb.train_steps(1)
        g = tb.get_gradients().astype(np.float64)
        grid, bf = tb.get_density_grid()
        st1 = tb.stats()
        nreq_d, cc, ns_d = tb.ray_counts(tr.R)
        # the variance gradient against the device's own batch, exactly: it is the fp32 sum, in a fixed tree, of column 7
        # of the step's compacted fp16 dL/doutput (after the rollover's copies, which the step's encode writes into the same
        # buffer), so it sits within depth x 2^-24 x sum |x| of that column's float64 sum - an absolute bar that does not
        # widen when the terms cancel, unlike the conditioning bar against the oracle's batch below. The buffer holds the
        # step's batch under every option this function runs with: the lookahead of the next step samples rays into
        # buffers of its own and the next loss, which rewrites dL/doutput, runs inside the next step.
        dl_dev = np.zeros((batch, 16), np.uint16)
        check(lib().neus_debug_get_batch(tb.handle, None, C.c_void_p(dl_dev.ctypes.data), None))
        col7 = dl_dev.view(np.float16)[:, 7].astype(np.float64)
        var_err = abs(g[lay["variance_offset"]] - col7.sum())
        var_bar = _variance_sum_depth(batch) * 2.0 ** -24 * np.abs(col7).sum()
        var_exact_ratio = max(var_exact_ratio, var_err / max(var_bar, 1e-300))
        var_terms_min = min(var_terms_min, int(np.count_nonzero(col7)))
        assert np.all(np.isfinite(col7)) and np.count_nonzero(col7) > 0 and var_err <= var_bar, (k, float(g[lay["variance_offset"]]), col7.sum(), var_err, var_bar)
        step_prog = st1["progressive_steps"] > prog_before
        step_later = int((cc > chunk_end).sum()) if step_prog else 0
        later_rounds += step_later
        evaluated += st1["evaluated_samples_last"]
        tr.density_grid[:] = grid
        tr.bitfield[:] = bf
        m = tr.march(skip_occupancy=True)
        gr = tr.grads_from_march(m).astype(np.float64)
        alt = {o: v.astype(np.float64) for o, v in tr.grads_alt_orders(m).items()}
        g_refop = tr.grads_grid_mode(m, "ref_operand").astype(np.float64)
        # the variance gradient is one batch sum of the fp16 dL/doutput[7] (nerf_network.h:461-474): each term is rounded
        # to fp16 from an fp32 value that the network outputs' fp16 noise moves, so two implementations can differ by an
        # fp16 ulp (2^-10 relative) per term; relative to the sum that is 2^-10 sum|x| / |sum x|, large when the terms cancel
        dl7 = tr.last["dL_dout"].view(np.float16)[:, 7].astype(np.float64)
        var_cond = max(var_cond, 2.0 ** -10 * np.abs(dl7).sum() / max(abs(dl7.sum()), 1e-30))
        _progress(f"{tag}: step {k + 1}/{n_steps} compared")
        kept += tr.last["n_kept"]
        # per-ray sample counts of the march, bit-exact over the kept ray slots (canonical ray order; past the kept extent
        # the device's prefix-limited march does not run the second pass, and the oracle keeps nothing there)
        n_o = m["numsteps"][:, 0]
        n_ext = int(np.nonzero(n_o)[0].max()) + 1 if n_o.any() else 0
        np.testing.assert_array_equal(nreq_d[:n_ext], n_o[:n_ext])
        assert int(n_o.sum()) == tr.last["n_kept"]
        # the requested-sample counter: equal below the cap; past it the device's prefix-limited march (k_march's
        # second pass skipped once the first pass's rays request max_samples) reads some value >= the cap, which is
        # all the reference uses of it (min(counter, max_samples), testbed_nerf.cu:3036-3039)
        req_d, req_o = st1["measured_batch_size_before_compaction"], tr.last["numsteps_counter"]
        if req_o >= tr.max_samples:
            assert req_d >= tr.max_samples, (k, req_d, req_o)
        else:
            assert req_d == req_o, (k, req_d, req_o)
        comp_d, comp_o = st1["measured_batch_size"], tr.last["compacted"]
        n_comp_equal += comp_d == comp_o
        assert abs(comp_d - comp_o) <= max(2, 1e-3 * comp_o), (k, comp_d, comp_o)
        short_seen |= comp_o < batch
        rec = {"step": st["training_step"], "compacted_device": comp_d, "compacted_oracle": comp_o, "kept": tr.last["n_kept"],
               "evaluated": st1["evaluated_samples_last"], "progressive": bool(step_prog), "chunk_end": chunk_end,
               "later_round_rays": step_later}
        for name, (a, b) in blocks.items():
            x, y = g[a:b], gr[a:b]
            ny = max(np.linalg.norm(y), 1e-30)
            cos = x @ y / max(np.linalg.norm(x) * np.linalg.norm(y), 1e-30)
            rel = np.linalg.norm(x - y) / ny
            worst[name][0] = min(worst[name][0], cos)
            worst[name][1] = max(worst[name][1], rel)
            for o, ga in alt.items():
                fo = np.linalg.norm(ga[a:b] - y) / ny
                floor_by_order[o][name] = max(floor_by_order[o][name], fo)
                floor[name] = max(floor[name], fo)
            rec[f"cos_{name}"], rec[f"rel_{name}"] = float(cos), float(rel)
        for l in range(cfg.n_levels):
            a, b = g0 + 2 * int(off[l]), g0 + 2 * int(off[l + 1])
            y = gr[a:b]
            if np.linalg.norm(y) > 0:
                lev_rel[l] = max(lev_rel[l], np.linalg.norm(g[a:b] - y) / np.linalg.norm(y))
                lev_floor[l] = max(lev_floor[l], max(np.linalg.norm(ga[a:b] - y) for ga in alt.values()) / np.linalg.norm(y))
                lev_refop[l] = max(lev_refop[l], np.linalg.norm(g_refop[a:b] - y) / np.linalg.norm(y))
        records.append(rec)
    prog = tb.stats()["progressive_steps"] - prog0
    _record(f"teacher_forced_all_levels_{tag}", steps=n_steps, start_step=prepare, batch=batch, compacted_equal_steps=n_comp_equal,
            progressive_steps=prog, evaluated_over_kept=evaluated / max(kept, 1), later_round_rays=later_rounds,
            short_step_compacted_below_batch=short_seen, floor_factor=floor_factor,
            **{f"min_cos_{k}": v[0] for k, v in worst.items()}, **{f"max_rel_{k}": v[1] for k, v in worst.items()},
            **{f"max_rel_grid_L{l}": lev_rel[l] for l in range(cfg.n_levels)},
            **{f"floor_rel_{k}": v for k, v in floor.items()},
            **{f"floor_{o}_{k}": v for o, d in floor_by_order.items() for k, v in d.items()},
            **{f"floor_rel_grid_L{l}": lev_floor[l] for l in range(cfg.n_levels)},
            **{f"ref_operand_rel_grid_L{l}": lev_refop[l] for l in range(cfg.n_levels)}, variance_conditioning_bar=var_cond,
            variance_exact_err_over_bar=var_exact_ratio, variance_exact_nonzero_terms_min=var_terms_min)
    st = tb.stats()
    assert prog >= n_steps - 1, (f"progressive inference ran on {prog} of {n_steps} steps (last step: {st['measured_batch_size']} "
                                 f"compacted of {st['measured_batch_size_before_compaction']} requested)")
    assert evaluated < kept, "the rounds evaluated every kept sample: the cut-off never skipped work"
    assert later_rounds > 0, "no ray composited past the first chunk: the later rounds had no work"
    assert short_seen or short_step is None, "no step compacted fewer samples than the batch: the rollover did not run"
    # per block: cos >= 0.9999 and rel-L2 <= 2e-3, or within floor_factor x the oracle's own largest spread over three
    # alternative summation orders (a converged state's gradients are sums of nearly cancelling fp16 terms: their rel-L2
    # floor rises above 2e-3)
    for name, (cos, rel) in worst.items():
        bar = max(2e-3, floor_factor * floor[name], var_cond if name == "variance" else 0.0)
        assert cos >= 0.9999 and rel <= bar, (name, cos, rel, floor[name], bar)
    # per hash level: the fine levels' gradient is a sum of contributions far below fp16's normal range
    # at small loss scales; the device's scaled records (grid.hip, record format) must keep each level at the floor
    if level_bar:
        bad = [(l, float(lev_rel[l]), float(lev_floor[l])) for l in range(cfg.n_levels)
               if lev_rel[l] > max(2e-3, floor_factor * lev_floor[l])]
        assert not bad, f"per-level grid rel-L2 above max(2e-3, {floor_factor} x floor): {bad}"
    return tb, records


def test_teacher_forced_all_levels_vs_oracle(scene, torch_cuda):
    """_teacher_forced_all_levels on the 8-view 64x48 scene with the progressive rounds forced on: the auto rule keeps
    this small scene one-pass (over 70 % of its kept samples are composited at step 700), so the rounds are forced with
    the same kernels the auto rule runs."""
    _teacher_forced_all_levels(scene, "small_forced", progressive=2)


def test_teacher_forced_all_levels_config_s_auto(torch_cuda):
    """_teacher_forced_all_levels on the bench's scene (Config S: 49 views of 1600x1200, DTU-scan24 intrinsics) at a
    4096-sample batch and the bench's ray shape (R = Nc fixed), from a state trained 800 steps at 2^16 samples per step
    (the bench trains at 2^18; a network trained on 4096-sample steps is far less opaque and composites nearly every
    kept sample: measured 65120 of 65536), with progressive inference left on its auto rule, which turns the rounds on
    when under 70 % of the kept samples are composited."""
    from neus2_amd import scenes
    sc = scenes.sphere_scene(49, 1600, 1200, principal=(823.2 / 1600, 619.1 / 1200))
    _teacher_forced_all_levels(sc, "config_s_auto", progressive=None, prepare=800, short_step=None, fixed_rays=BATCH,
                               prepare_batch=1 << 16)


def test_teacher_forced_bench_shape(torch_cuda):
    """the bench's exact step against the oracle. Config S (49 views of 1600x1200, DTU-scan24 intrinsics,
    bench.py's scene), base.json (L=14), R = Nc = 2^18 fixed, 800 free-running steps at 2^18 (bench.py's --prepare), then
    2 consecutive steps each compared with the oracle's step from the device's state: progressive inference on its auto
    rule with the adaptive chunk ends, the spatial ray order (k_ray_hist / k_ray_sort_place, one eighth of the surface per
    XCD), the region scatter with its heavy dense-level buckets split over several workgroups (64-bit integer atomics),
    64-tile look-back scans over 2^18 rays, ~2 M evaluated samples per step. Asserts as _teacher_forced_all_levels (march
    bit-exact per ray, compacted count equal up to fp16-moved cut-offs, per block cos >= 0.9999 and rel-L2 <= max(2e-3,
    1.5 x the largest floor over three summation orders)), plus: every compared step ran the progressive rounds with work
    past the first chunk, and the scatter ran split buckets that received records.
    Reference: testbed_nerf.cu:3723-4001, grid.h:371-500, 880-1007."""
    import ctypes as C
    from neus2_amd import scenes
    from neus2_amd._lib import check, lib
    assert os.environ.get("NEUS_RAY_SORT", "1") != "0" and "NEUS_CHUNK_ENDS" not in os.environ
    sc = scenes.sphere_scene(49, 1600, 1200, principal=(823.2 / 1600, 619.1 / 1200))
    n = 1 << 18
    tb, recs = _teacher_forced_all_levels(sc, "bench_shape", progressive=None, n_steps=2, prepare=800, short_step=None,
                                          fixed_rays=n, batch=n)
    L = tb.layout()["n_levels"]
    parts = np.zeros(L, np.uint32)
    check(lib().neus_debug_scatter_parts(tb.handle, C.c_void_p(parts.ctypes.data)))
    rec_lvl = np.zeros(L, np.uint64)
    mx = C.c_uint32(0)
    check(lib().neus_debug_scatter_stats(tb.handle, C.c_void_p(rec_lvl.ctypes.data), C.byref(mx)))
    split_levels = [l for l in range(L) if parts[l] > 1 and rec_lvl[l] > 0]
    with open(os.path.join(ROOT, "gpurun_out", "parity_bench_shape.json"), "w") as f:
        import json
        json.dump({"steps": recs, "parts_per_level": parts.tolist(), "records_per_level": rec_lvl.tolist()}, f, indent=1)
    assert all(r["progressive"] for r in recs), recs
    assert all(r["later_round_rays"] > 0 for r in recs), recs
    assert all(r["evaluated"] < r["kept"] for r in recs), recs
    assert split_levels, (parts, rec_lvl)


def test_training_is_bitwise_reproducible(scene, torch_cuda):
    """Two testbeds, same seed and data, 50 free-running steps each: parameters, EMA weights, occupancy grid and
    losses are bitwise equal. Every reduction of the step is fixed-order (scan compaction, int64 fixed-point grid
    scatter, split-ordered weight-gradient and variance sums, deterministic grid mean); the only atomics left are
    the occupancy splat's atomicMax (order-independent)."""
    tbs = [_testbed(scene) for _ in range(2)]
    for tb in tbs:
        tb.train_steps(50)
    a, b = tbs
    np.testing.assert_array_equal(a.get_params(), b.get_params())
    np.testing.assert_array_equal(a.get_ema_params(), b.get_ema_params())
    np.testing.assert_array_equal(a.get_density_grid()[0], b.get_density_grid()[0])
    sa, sb = a.stats(), b.stats()
    assert sa["loss"] == sb["loss"] and sa["rays_per_batch"] == sb["rays_per_batch"]
