"""GPU parity tests: the HIP path (through the C-ABI) against the CPU oracle on the same seeded
inputs. Bit-exact for integer/index data (ray slots, numsteps, compaction, sample coordinates);
fp16-scale tolerances (stated per test) for floating-point outputs and gradients."""
import ctypes as C
import os

import numpy as np
import pytest

from gpu_util import dev, host, ptr, env as _env

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH = 4096


@pytest.fixture(scope="module")
def env(torch_cuda):
    from neus2_amd import pyngp, scenes
    import oracle as O
    sc = scenes.small_scene(n_views=8, width=64, height=48)
    tb = pyngp.Testbed(pyngp.TestbedMode.Nerf)
    tb.set_dataset(sc["images"], sc["focal"], sc["principal"], sc["xforms"], 1)
    tb.reload_network_from_file(os.path.join(ROOT, "configs", "nerf", "base.json"), batch_size=BATCH)
    cfg = O.make_cfg(per_level_scale=tb._net_cfg.per_level_scale)
    ds = O.Dataset(sc["images"], sc["focal"], sc["principal"], sc["xforms"])
    return dict(tb=tb, O=O, cfg=cfg, ds=ds, sc=sc, t=torch_cuda, scenes=scenes)


def L():
    from neus2_amd._lib import check, lib
    return lib(), check


def record(test, **metrics):
    """Append measured parity metrics to gpurun_out/parity_metrics.jsonl (evidence for DESIGN.md)."""
    import json
    os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
    with open(os.path.join(ROOT, "gpurun_out", "parity_metrics.jsonl"), "a") as f:
        f.write(json.dumps({"test": test, **{k: float(v) for k, v in metrics.items()}}) + "\n")


def test_mfma_f16_layout_exact(torch_cuda):
    """v_mfma_f32_32x32x16_f16 lane maps (natural k order) with exact small-integer data, asymmetric B."""
    t = torch_cuda
    rng = np.random.default_rng(0)
    A = rng.integers(-4, 5, size=(32, 16)).astype(np.float16)
    B = rng.integers(-4, 5, size=(16, 32)).astype(np.float16)
    B[0, 1] = 7  # asymmetric
    Cd = t.zeros((32, 32), dtype=t.float32, device="cuda")
    lib, check = L()
    check(lib.neus_mfma_probe(ptr(dev(t, A)), ptr(dev(t, B)), ptr(Cd)))
    np.testing.assert_array_equal(Cd.cpu().numpy(), A.astype(np.float32) @ B.astype(np.float32))


def test_param_init_matches_oracle(env):
    """Trainer init (seed_seq{1337} -> pcg32; xavier; grid U(+-1e-4); variance 0.3) bit-exact."""
    O, tb = env["O"], env["tb"]
    geo = tb._geo
    ref = np.zeros(O.layout(env["cfg"])["n_params"], np.float32)
    O.lib().or_init_params(C.byref(env["cfg"]), C.c_uint32(1337), O.P(geo), O.P(ref))
    got = tb.get_params()
    np.testing.assert_array_equal(got, ref)


def _perturbed(env, seed=11):
    """Parameters that exercise every path: nonzero encoding columns of W0 and O(0.1) grid values."""
    tb = env["tb"]
    lay = tb.layout()
    rng = np.random.default_rng(seed)
    p = tb.get_params().copy()
    din = lay["density_input_width"]
    w0 = p[: 64 * din].reshape(64, din)
    w0[:, 3:31] = rng.normal(0, 0.3, (64, 28))
    p[: 64 * din] = w0.reshape(-1)
    g0, g1 = lay["grid_offset"], lay["variance_offset"]
    p[g0:g1] = rng.uniform(-0.1, 0.1, g1 - g0).astype(np.float32)
    tb.set_params(p)
    return p


def _coords(n, seed=0):
    rng = np.random.default_rng(seed)
    c = np.zeros((n, 7), np.float32)
    c[:, :3] = rng.uniform(0.05, 0.95, (n, 3))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    c[:, 4:] = (d + 1) * 0.5
    return c


def test_grid_encode_parity(env):
    """Hash-grid forward: enc (fp16-accumulated like the reference) and dy/dx (FMA-accumulated f32)
    bit-exact against the oracle."""
    t, O, tb = env["t"], env["O"], env["tb"]
    lib, check = L()
    n = 1024
    c = _coords(n, 1)
    Lv = env["cfg"].n_levels
    params = _perturbed(env)
    for valid in (Lv, 3):
        enc = t.zeros((Lv, n, 2), dtype=t.int16, device="cuda")
        dydx = t.zeros((6 * Lv, n), dtype=t.float32, device="cuda")
        check(lib.neus_grid_encode(tb.handle, None, C.c_uint32(n), C.c_uint32(n), ptr(dev(t, c)), C.c_uint32(7), C.c_uint32(valid), ptr(enc), ptr(dydx)))
        t.cuda.synchronize()
        got = host(enc, np.float16).astype(np.float32).transpose(1, 0, 2).reshape(n, 2 * Lv)
        gdy = host(dydx, np.float32).reshape(Lv, 2, 3, n).transpose(3, 0, 1, 2).reshape(n, 2 * Lv, 3)
        ref, rdy = O.grid_forward(env["cfg"], params, c[:, :3], valid)
        os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
        np.savez(os.path.join(ROOT, "gpurun_out", f"grid_diag_{valid}.npz"), c=c, got=got, gdy=gdy, ref=ref, rdy=rdy)
        np.testing.assert_array_equal(got.view(np.uint32), ref.astype(np.float32).view(np.uint32))
        np.testing.assert_array_equal(gdy.view(np.uint32), rdy.view(np.uint32))


def test_network_forward_parity(env):
    """NerfNetwork forward (AoS16 fp16 out): rows 0..10 within fp16-accumulation tolerance."""
    t, O, tb = env["t"], env["O"], env["tb"]
    lib, check = L()
    n = 2048
    c = _coords(n, 2)
    params = _perturbed(env, 12)
    out = t.zeros((n, 16), dtype=t.int16, device="cuda")
    for valid in (14, 4):
        check(lib.neus_net_forward(tb.handle, None, C.c_uint32(n), ptr(dev(t, c)), C.c_uint32(valid), ptr(out)))
        t.cuda.synchronize()
        got = host(out, np.float16).astype(np.float32)
        ref = O.network_forward(env["cfg"], params, c, valid).view(np.float16).astype(np.float32)
        err = np.abs(got[:, :11] - ref[:, :11])
        tol = 2e-3 + 4e-3 * np.abs(ref[:, :11])
        # fp16 storage noise can flip a ReLU mask of a near-zero hidden unit, which moves that sample's
        # dSDF/dx (and the rgb logits fed by it) discontinuously; the reference has the same behaviour.
        ok_samples = np.all(err <= tol, axis=1)
        record(f"forward_valid{valid}", frac_within_tol=ok_samples.mean(), median_abs_err=np.median(err), max_abs_err=err.max())
        assert ok_samples.mean() >= 0.995, (ok_samples.mean(), np.argwhere(err > tol)[:5])
        assert np.median(err) < 1e-3


def test_network_forward_outside_unit_cube(env):
    """Positions outside [0,1]^3 (a DeltaNetwork-moved sample, a grid point past the aabb): the dense levels' corner
    index wraps with the reference's `% hashmap_size` (grid.h:118-153), also for negative cells (huge unsigned
    values) - the fused kernel's in-cube shortcut must not be taken there. Forward within the tolerance of
    test_network_forward_parity against the oracle."""
    t, O, tb = env["t"], env["O"], env["tb"]
    lib, check = L()
    n = 2048
    c = _coords(n, 21)
    rng = np.random.default_rng(22)
    c[:, :3] = rng.uniform(-0.4, 1.4, (n, 3)).astype(np.float32)
    c[:8, :3] = np.float32([[-1e-3, 0.5, 0.5], [1.0, 1.0, 1.0], [-2.5, 3.0, 0.2], [0.5, -0.75, 1.9],
                            [1.0 - 1e-7, 0.0, 0.0], [0.0, 0.0, 0.0], [7.0, -7.0, 0.5], [0.25, 0.5, -1e-6]])
    params = _perturbed(env, 23)
    out = t.zeros((n, 16), dtype=t.int16, device="cuda")
    check(lib.neus_net_forward(tb.handle, None, C.c_uint32(n), ptr(dev(t, c)), C.c_uint32(14), ptr(out)))
    t.cuda.synchronize()
    got = host(out, np.float16).astype(np.float32)
    ref = O.network_forward(env["cfg"], params, c, 14).view(np.float16).astype(np.float32)
    err = np.abs(got[:, :11] - ref[:, :11])
    ok = np.all(err <= 2e-3 + 4e-3 * np.abs(ref[:, :11]), axis=1)
    record("forward_outside_cube", frac_within_tol=ok.mean(), median_abs_err=np.median(err))
    assert ok.mean() >= 0.995 and np.median(err) < 1e-3, ok.mean()


def test_network_backward_parity(env):
    """First + second order parameter gradients: cosine >= 0.999 per block, rel-L2 <= 2e-2."""
    t, O, tb = env["t"], env["O"], env["tb"]
    lib, check = L()
    n = 1024
    c = _coords(n, 3)
    params = _perturbed(env, 13)
    rng = np.random.default_rng(4)
    dl = np.zeros((n, 16), np.float32)
    dl[:, :4] = rng.normal(0, 1e-2, (n, 4))
    dl[:, 4:7] = rng.normal(0, 1.0, (n, 3))
    dl[:, 7] = rng.normal(0, 1e-2, n)
    dl[:, 8:11] = rng.normal(0, 1e-2, (n, 3))
    dl16 = dl.astype(np.float16)
    lay = tb.layout()
    g = t.zeros(lay["n_params"], dtype=t.float32, device="cuda")
    check(lib.neus_net_backward(tb.handle, None, C.c_uint32(n), ptr(dev(t, c)), C.c_uint32(14), ptr(dev(t, dl16)), C.c_uint32(n), ptr(g)))
    t.cuda.synchronize()
    got = g.cpu().numpy()
    ref = O.network_backward(env["cfg"], params, c, 14, dl16.view(np.uint16), n)
    blocks = {"density": (0, lay["n_density"]), "rgb": (lay["n_density"], lay["n_matrix"]),
              "grid": (lay["grid_offset"], lay["variance_offset"]), "variance": (lay["variance_offset"], lay["variance_offset"] + 1)}
    for name, (a, b) in blocks.items():
        x, y = got[a:b].astype(np.float64), ref[a:b].astype(np.float64)
        rel = np.linalg.norm(x - y) / max(np.linalg.norm(y), 1e-30)
        cos = x @ y / max(np.linalg.norm(x) * np.linalg.norm(y), 1e-30)
        record(f"backward_{name}", rel=rel, cos=cos)
        assert rel <= 2e-2 and cos >= 0.999, (name, rel, cos)


def _bitfield(env):
    return env["scenes"].shell_bitfield(thickness=6.0 / 128)


def test_sample_rays_bit_exact(env):
    """Ray sampling + occupancy march: rays, numsteps, coords bit-identical to the oracle."""
    t, O, tb = env["t"], env["O"], env["tb"]
    lib, check = L()
    bf = _bitfield(env)
    n_rays, max_samples = 4096, 4096 * 16
    rng_state, rng_inc = 0x1234567890ABCDEF, 0xDA3E39CB94B95BDB | 1
    # the last case uses the Testbed's own stream increment (3): the device advances by its jump-ahead table
    for (max_s, world, rank, total, inc) in [(max_samples, 1, 0, 0, rng_inc), (20000, 1, 0, 12345, rng_inc), (max_samples, 2, 1, 8192, rng_inc),
                                             (max_samples, 1, 0, 777, 3)]:
        rays = t.zeros((n_rays, 6), dtype=t.float32, device="cuda")
        ns = t.zeros((n_rays, 2), dtype=t.int32, device="cuda")
        co = t.zeros((max_s, 7), dtype=t.float32, device="cuda")
        cnt = (C.c_uint32 * 3)()
        check(lib.neus_sample_rays(tb.handle, None, C.c_uint32(n_rays), C.c_uint32(rank), C.c_uint32(world), C.c_uint32(total),
                                   C.c_uint64(rng_state), C.c_uint64(inc), C.c_uint32(max_s), ptr(dev(t, bf)),
                                   ptr(rays), ptr(ns), ptr(co), cnt))
        r_rays, r_ns, r_co, r_cnt, r_nr = O.generate_samples(env["ds"], bf, n_rays, total, rng_state, inc, max_s,
                                                             ray_offset=rank * n_rays, n_rays_global=world * n_rays)
        g_ns = host(ns, np.uint32)
        np.testing.assert_array_equal(g_ns, r_ns)
        assert cnt[0] == r_cnt and cnt[2] == r_nr
        np.testing.assert_array_equal(host(rays, np.uint32), r_rays.view(np.uint32))
        nk = int(cnt[1])
        assert nk == int((r_ns[:, 0]).sum())
        np.testing.assert_array_equal(host(co, np.uint32)[:nk], r_co.view(np.uint32)[:nk])
        assert nk > 0


def test_sample_rays_culled_bit_exact(env):
    """A small off-centre occupied blob: most rays miss the occupied cells' box and are culled by the ray generation
    (k_ray_gen, launch_occ_bbox) instead of marched; rays, numsteps and coords stay bit-identical to the oracle's full
    march, including the rays grazing the box."""
    t, O, tb = env["t"], env["O"], env["tb"]
    lib, check = L()
    G = 128
    c = (np.arange(G) + 0.5) / G
    X, Y, Z = np.meshgrid(c, c, c, indexing="ij")
    occ = (X - 0.62) ** 2 + (Y - 0.45) ** 2 + (Z - 0.55) ** 2 < 0.09 ** 2
    bf = env["scenes"].bitfield_from_occupancy(occ)
    n_rays, max_s = 4096, 4096 * 16
    rays = t.zeros((n_rays, 6), dtype=t.float32, device="cuda")
    ns = t.zeros((n_rays, 2), dtype=t.int32, device="cuda")
    co = t.zeros((max_s, 7), dtype=t.float32, device="cuda")
    cnt = (C.c_uint32 * 3)()
    rs, ri = 0x0123456789ABCDEF, 0xDA3E39CB94B95BDB | 1
    check(lib.neus_sample_rays(tb.handle, None, C.c_uint32(n_rays), C.c_uint32(0), C.c_uint32(1), C.c_uint32(0), C.c_uint64(rs), C.c_uint64(ri),
                               C.c_uint32(max_s), ptr(dev(t, bf)), ptr(rays), ptr(ns), ptr(co), cnt))
    r_rays, r_ns, r_co, r_cnt, r_nr = O.generate_samples(env["ds"], bf, n_rays, 0, rs, ri, max_s)
    np.testing.assert_array_equal(host(ns, np.uint32), r_ns)
    assert cnt[0] == r_cnt and cnt[2] == r_nr
    np.testing.assert_array_equal(host(rays, np.uint32), r_rays.view(np.uint32))
    nk = int(cnt[1])
    np.testing.assert_array_equal(host(co, np.uint32)[:nk], r_co.view(np.uint32)[:nk])
    # the blob is hit by a minority of the rays: the cull had most of them to skip
    assert 0 < r_nr < n_rays // 2, r_nr


def test_sample_rays_block_grid_bit_exact(env):
    """Single occupied cells in 3 % of the 4^3-cell blocks: most rays alternate long empty skips with one-cell sample
    runs (segment joins landing after skips, many short records), 16384 rays against the oracle; rays, numsteps and coords
    bit-identical. (Written for round 5's exact empty-block skip, measured and not adopted: DESIGN §3.1.)"""
    t, O, tb = env["t"], env["O"], env["tb"]
    lib, check = L()
    G = 128
    rng = np.random.default_rng(5)
    occ = np.zeros((G, G, G), bool)
    bi = np.argwhere(rng.random((G // 4,) * 3) < 0.03)
    occ[tuple((4 * bi + rng.integers(0, 4, size=bi.shape)).T)] = True
    bf = env["scenes"].bitfield_from_occupancy(occ)
    n_rays, max_s = 16384, 16384 * 16
    rays = t.zeros((n_rays, 6), dtype=t.float32, device="cuda")
    ns = t.zeros((n_rays, 2), dtype=t.int32, device="cuda")
    co = t.zeros((max_s, 7), dtype=t.float32, device="cuda")
    cnt = (C.c_uint32 * 3)()
    rs, ri = 0x0F1E2D3C4B5A6978, 0xDA3E39CB94B95BDB | 1
    check(lib.neus_sample_rays(tb.handle, None, C.c_uint32(n_rays), C.c_uint32(0), C.c_uint32(1), C.c_uint32(0), C.c_uint64(rs), C.c_uint64(ri),
                               C.c_uint32(max_s), ptr(dev(t, bf)), ptr(rays), ptr(ns), ptr(co), cnt))
    r_rays, r_ns, r_co, r_cnt, r_nr = O.generate_samples(env["ds"], bf, n_rays, 0, rs, ri, max_s)
    np.testing.assert_array_equal(host(ns, np.uint32), r_ns)
    assert cnt[0] == r_cnt and cnt[2] == r_nr
    np.testing.assert_array_equal(host(rays, np.uint32), r_rays.view(np.uint32))
    nk = int(cnt[1])
    np.testing.assert_array_equal(host(co, np.uint32)[:nk], r_co.view(np.uint32)[:nk])
    assert nk > 1000, nk


@pytest.mark.parametrize("n_rays", [4096, 1000])
def test_loss_compaction_parity(env, n_rays):
    """Composite/loss/compaction on fixed network outputs: compaction bit-exact, dL/dout fp16-close. 1000 rays: a ray
    count that is not a multiple of the wave (k_loss_ray's wave-wide sample-map fill masks the lanes past
    the last ray instead of refusing the call)."""
    t, O, tb = env["t"], env["O"], env["tb"]
    lib, check = L()
    bf = _bitfield(env)
    max_s = n_rays * 16
    rs, ri = 0x0BADF00D12345678, 0xDA3E39CB94B95BDB | 1
    r_rays, r_ns, r_co, r_cnt, _ = O.generate_samples(env["ds"], bf, n_rays, 0, rs, ri, max_s)
    nk = int(r_ns[:, 0].sum())
    net = O.network_forward(env["cfg"], tb.get_params(), r_co[:nk], 14)
    rng = np.random.default_rng(7)
    net = net.view(np.float16).copy()
    net[:, 3] = rng.normal(0.0, 0.05, nk).astype(np.float16)  # sdf spread so alphas vary
    net[:, 7] = np.float16(0.35)
    net = net.view(np.uint16)
    for max_c in (BATCH, 2000):
        nsd = dev(t, r_ns)
        co = t.zeros((max_c, 7), dtype=t.float32, device="cuda")
        dlo = t.zeros((max_c, 16), dtype=t.int16, device="cuda")
        loss = t.zeros(n_rays, dtype=t.float32, device="cuda"); ek = t.zeros_like(loss); mk = t.zeros_like(loss)
        cnt = (C.c_uint32 * 1)()
        check(lib.neus_loss_compact(tb.handle, None, C.c_uint32(n_rays), C.c_uint32(0), C.c_uint32(1), C.c_uint32(0),
                                    C.c_uint64(rs), C.c_uint64(ri), C.c_uint32(max_c), ptr(dev(t, r_rays)), ptr(nsd),
                                    ptr(dev(t, r_co)), ptr(dev(t, net)), ptr(co), ptr(dlo), ptr(loss), ptr(ek), ptr(mk), cnt))
        ref = O.compute_loss(env["ds"], n_rays, 0, rs, ri, max_c, r_rays, r_ns, r_co, net)
        assert cnt[0] == ref["counter"]
        np.testing.assert_array_equal(host(nsd, np.uint32), ref["numsteps"])
        nc = min(ref["counter"], max_c)
        np.testing.assert_array_equal(host(co, np.uint32)[:nc], ref["coords"].view(np.uint32)[:nc])
        g = host(dlo, np.float16).astype(np.float32)[:nc, :11]
        r = ref["dL_dout"].view(np.float16).astype(np.float32)[:nc, :11]
        np.testing.assert_allclose(g, r, rtol=2e-3, atol=1e-6)
        np.testing.assert_allclose(loss.cpu().numpy(), ref["loss"], rtol=1e-4, atol=1e-9)


def test_masked_dataset_sampling_and_loss_parity(env):
    """Dynamic masks (nerf_loader.cu:571-590): views prepared with a mask (pyngp.prepare_image -> the hot-pink key
    0x00FF00FF) read as negative targets (read_rgba, common_device.cuh:635-667), so the sampler drops 10 % of the rays
    that hit them, with an extra rng draw (testbed_nerf.cu:1310-1312) and the loss of the kept ones takes the masked
    branch (rgb target from -1 texels, mask_gt 0). Sampling (rays, numsteps, coordinates) bit-exact and the loss /
    compaction as test_loss_compaction_parity, against the oracle on the same prepared images."""
    from neus2_amd import pyngp
    t, O = env["t"], env["O"]
    lib, check = L()
    sc = env["sc"]
    rng = np.random.default_rng(21)
    images = []
    n_masked = 0
    for img in sc["images"]:
        mask = np.zeros_like(img)
        mask[..., 0] = (rng.random(img.shape[:2]) < 0.4) * 255
        out, key = pyngp.prepare_image(img, mask=mask)
        assert key == 0x00FF00FF
        n_masked += int((out.view(np.uint32)[..., 0] == 0x00FF00FF).sum())
        images.append(out)
    assert n_masked > 0
    tb = pyngp.Testbed(pyngp.TestbedMode.Nerf)
    tb.set_dataset(images, sc["focal"], sc["principal"], sc["xforms"], 1)
    tb.reload_network_from_file(os.path.join(ROOT, "configs", "nerf", "base.json"), batch_size=BATCH)
    ds = O.Dataset(images, sc["focal"], sc["principal"], sc["xforms"])
    bf = _bitfield(env)
    n_rays, max_s = 4096, 4096 * 16
    rs, ri = 0x2545F4914F6CDD1D, 0xDA3E39CB94B95BDB | 1
    rays = t.zeros((n_rays, 6), dtype=t.float32, device="cuda")
    ns = t.zeros((n_rays, 2), dtype=t.int32, device="cuda")
    co = t.zeros((max_s, 7), dtype=t.float32, device="cuda")
    cnt = (C.c_uint32 * 3)()
    check(lib.neus_sample_rays(tb.handle, None, C.c_uint32(n_rays), C.c_uint32(0), C.c_uint32(1), C.c_uint32(0),
                               C.c_uint64(rs), C.c_uint64(ri), C.c_uint32(max_s), ptr(dev(t, bf)), ptr(rays), ptr(ns), ptr(co), cnt))
    r_rays, r_ns, r_co, r_cnt, r_nr = O.generate_samples(ds, bf, n_rays, 0, rs, ri, max_s)
    np.testing.assert_array_equal(host(ns, np.uint32), r_ns)
    np.testing.assert_array_equal(host(rays, np.uint32), r_rays.view(np.uint32))
    nk = int(cnt[1])
    assert nk == int(r_ns[:, 0].sum()) and nk > 0
    np.testing.assert_array_equal(host(co, np.uint32)[:nk], r_co.view(np.uint32)[:nk])
    # the masks change the sampling (their extra rng draw and the 10 % drop of rays on masked texels)
    _, r_ns_plain, _, r_cnt_plain, _ = O.generate_samples(env["ds"], bf, n_rays, 0, rs, ri, max_s)
    assert r_cnt != r_cnt_plain and not np.array_equal(r_ns, r_ns_plain)
    net = O.network_forward(env["cfg"], tb.get_params(), r_co[:nk], 14).view(np.float16).copy()
    net[:, 3] = rng.normal(0.0, 0.05, nk).astype(np.float16)
    net[:, 7] = np.float16(0.35)
    net = net.view(np.uint16)
    nsd = dev(t, r_ns)
    co_c = t.zeros((BATCH, 7), dtype=t.float32, device="cuda")
    dlo = t.zeros((BATCH, 16), dtype=t.int16, device="cuda")
    loss = t.zeros(n_rays, dtype=t.float32, device="cuda"); ek = t.zeros_like(loss); mk = t.zeros_like(loss)
    c1 = (C.c_uint32 * 1)()
    check(lib.neus_loss_compact(tb.handle, None, C.c_uint32(n_rays), C.c_uint32(0), C.c_uint32(1), C.c_uint32(0),
                                C.c_uint64(rs), C.c_uint64(ri), C.c_uint32(BATCH), ptr(dev(t, r_rays)), ptr(nsd),
                                ptr(dev(t, r_co)), ptr(dev(t, net)), ptr(co_c), ptr(dlo), ptr(loss), ptr(ek), ptr(mk), c1))
    ref = O.compute_loss(ds, n_rays, 0, rs, ri, BATCH, r_rays, r_ns, r_co, net)
    assert c1[0] == ref["counter"]
    np.testing.assert_array_equal(host(nsd, np.uint32), ref["numsteps"])
    nc = min(ref["counter"], BATCH)
    np.testing.assert_array_equal(host(co_c, np.uint32)[:nc], ref["coords"].view(np.uint32)[:nc])
    g = host(dlo, np.float16).astype(np.float32)[:nc, :11]
    r = ref["dL_dout"].view(np.float16).astype(np.float32)[:nc, :11]
    np.testing.assert_allclose(g, r, rtol=2e-3, atol=1e-6)
    np.testing.assert_allclose(loss.cpu().numpy(), ref["loss"], rtol=1e-4, atol=1e-9)


def test_loss_target_options_parity(env):
    """The loss targets under the reference's training options (testbed_nerf.cu:1642-1671): a fixed background
    (random_bg_color False, background_color) and the SRGB colour space / linear_colors target modes, against the
    oracle with the same options. Compaction bit-exact, dL/dout and loss fp16-close as above; the options must
    change the loss (they are exercised)."""
    t, O, tb = env["t"], env["O"], env["tb"]
    from neus2_amd import pyngp
    lib, check = L()
    bf = _bitfield(env)
    n_rays, max_s, max_c = 2048, 2048 * 16, BATCH
    rs, ri = 0x0BADF00D12345678, 0xDA3E39CB94B95BDB | 1
    ds = env["ds"]
    r_rays, r_ns, r_co, _, _ = O.generate_samples(ds, bf, n_rays, 0, rs, ri, max_s)
    nk = int(r_ns[:, 0].sum())
    net = O.network_forward(env["cfg"], tb.get_params(), r_co[:nk], 14).view(np.float16).copy()
    net[:, 3] = np.random.default_rng(8).normal(0.0, 0.05, nk).astype(np.float16)
    net[:, 7] = np.float16(0.35)
    net = net.view(np.uint16)
    losses = []
    cases = [(True, None, 0), (False, (1.0, 1.0, 1.0), 0), (False, (0.2, 0.5, 0.9), 1), (True, None, 1), (False, (1.0, 1.0, 1.0), 2)]
    try:
        for random_bg, bgc, mode in cases:
            tb.nerf.training.random_bg_color = random_bg
            if bgc is not None:
                tb.background_color = [*bgc, 1.0]
            tb.color_space = pyngp.ColorSpace.SRGB if mode == 1 else pyngp.ColorSpace.Linear
            tb.nerf.training.linear_colors = mode == 2
            ds.set_target(None if random_bg else tb.background_color[:3], mode)
            nsd = dev(t, r_ns)
            co = t.zeros((max_c, 7), dtype=t.float32, device="cuda")
            dlo = t.zeros((max_c, 16), dtype=t.int16, device="cuda")
            loss = t.zeros(n_rays, dtype=t.float32, device="cuda"); ek = t.zeros_like(loss); mk = t.zeros_like(loss)
            cnt = (C.c_uint32 * 1)()
            check(lib.neus_loss_compact(tb.handle, None, C.c_uint32(n_rays), C.c_uint32(0), C.c_uint32(1), C.c_uint32(0),
                                        C.c_uint64(rs), C.c_uint64(ri), C.c_uint32(max_c), ptr(dev(t, r_rays)), ptr(nsd),
                                        ptr(dev(t, r_co)), ptr(dev(t, net)), ptr(co), ptr(dlo), ptr(loss), ptr(ek), ptr(mk), cnt))
            ref = O.compute_loss(ds, n_rays, 0, rs, ri, max_c, r_rays, r_ns, r_co, net)
            assert cnt[0] == ref["counter"]
            np.testing.assert_array_equal(host(nsd, np.uint32), ref["numsteps"])
            nc = min(ref["counter"], max_c)
            g = host(dlo, np.float16).astype(np.float32)[:nc, :11]
            r = ref["dL_dout"].view(np.float16).astype(np.float32)[:nc, :11]
            np.testing.assert_allclose(g, r, rtol=2e-3, atol=1e-6)
            np.testing.assert_allclose(loss.cpu().numpy(), ref["loss"], rtol=1e-4, atol=1e-9)
            losses.append(float(ref["loss"].sum()))
    finally:
        tb.nerf.training.random_bg_color = True
        tb.nerf.training.linear_colors = False
        tb.color_space = pyngp.ColorSpace.Linear
        tb.background_color = [0.0, 0.0, 0.0, 1.0]
        ds.set_target(None, 0)
    # the scene's alpha is 0 or 1, where the SRGB and Linear targets coincide (cases 0 and 3); the other options
    # each change the loss
    assert len(set(np.round(losses, 6))) == 4 and abs(losses[0] - losses[3]) < 1e-9, losses


def test_train_steps_reduce_loss(env):
    """End-to-end Testbed::train on the small synthetic scene: loss decreases, state consistent."""
    from neus2_amd import pyngp
    sc = env["sc"]
    tb = pyngp.Testbed(pyngp.TestbedMode.Nerf)
    tb.set_dataset(sc["images"], sc["focal"], sc["principal"], sc["xforms"], 1)
    tb.reload_network_from_file(os.path.join(ROOT, "configs", "nerf", "base.json"), batch_size=BATCH)
    tb.train_steps(32)
    l0 = tb.stats()["ray_loss"]
    tb.train_steps(288)
    st = tb.stats()
    assert st["training_step"] == 320
    assert np.isfinite(st["ray_loss"]) and st["ray_loss"] < 0.7 * l0, (l0, st)
    assert st["measured_batch_size"] > 0 and st["zero_records"] == 0


def test_snapshot_round_trip(env, tmp_path):
    """save_snapshot -> load_snapshot into a fresh testbed (testbed.cu:3144-3254): params are the fp16 EMA
    weights, grid fp16, counters / step / loss / movement restored, the occupancy bitfield rebuilt from the
    grid is the saved one, the two testbeds render the same image (up to the progressive-level state a load
    resets), and training resumes."""
    from neus2_amd import pyngp
    sc = env["sc"]
    tb = pyngp.Testbed(pyngp.TestbedMode.Nerf)
    tb.set_dataset(sc["images"], sc["focal"], sc["principal"], sc["xforms"], 1)
    tb.reload_network_from_file(os.path.join(ROOT, "configs", "nerf", "base.json"), batch_size=BATCH)
    tb.train_steps(48)
    p = str(tmp_path / "s.msgpack")
    tb.save_snapshot(p)
    st0 = tb.stats()
    tb2 = pyngp.Testbed(pyngp.TestbedMode.Nerf)
    tb2.set_dataset(sc["images"], sc["focal"], sc["principal"], sc["xforms"], 1)
    tb2.reload_network_from_file(os.path.join(ROOT, "configs", "nerf", "base.json"), batch_size=BATCH)
    tb2.load_snapshot(p)
    st1 = tb2.stats()
    for k in ("training_step", "rays_per_batch", "measured_batch_size", "measured_batch_size_before_compaction"):
        assert st1[k] == st0[k], k
    assert st1["loss"] == pytest.approx(st0["loss"])
    ema16 = tb.get_ema_params().astype(np.float16).astype(np.float32)
    np.testing.assert_array_equal(tb2.get_params(), ema16)
    g0, b0 = tb.get_density_grid()
    g1, b1 = tb2.get_density_grid()
    np.testing.assert_array_equal(g1, g0.astype(np.float16).astype(np.float32))
    # the bitfield is rebuilt from the fp16 grid: equal to the saved one except where fp16 rounding crosses the
    # occupancy threshold
    assert (np.unpackbits(b0[: 128 ** 3 // 8]) != np.unpackbits(b1[: 128 ** 3 // 8])).mean() < 1e-3
    tb2.set_density_grid(bitfield=b0)
    # the inference weights the renderer reads: fp16(fp32 EMA) on the device == the snapshot's fp16 params
    h0, h1 = tb.get_half_params(inference=True), tb2.get_half_params(inference=True)
    bad = np.flatnonzero(h0.view(np.uint16) != h1.view(np.uint16))
    assert bad.size == 0, (bad[:8], h0[bad[:8]], h1[bad[:8]], ema16[bad[:8]])
    for t in (tb, tb2):
        t.snap_to_pixel_centers = True
        t.set_camera_to_training_view(0)
    # tb renders with its fp32-derived fp16 EMA weights at the progressive level of its last step; tb2 with the same
    # fp16 values but, like the reference after load_snapshot (a fresh GridEncoding, grid.h:1465, until the next
    # train step sets its step), with every level. The levels above the trained ones hold init-scale features the
    # density MLP's zero-initialised columns barely read, so the images agree closely, not bitwise.
    assert st0["valid_level"] < tb.layout()["n_levels"] and st1["valid_level"] == tb.layout()["n_levels"]
    a, b = tb.render(64, 48, spp=1), tb2.render(64, 48, spp=1)
    record("snapshot_render", mean_abs=np.abs(a - b).mean(), max_abs=np.abs(a - b).max())
    assert np.abs(a - b).mean() < 1e-3, np.abs(a - b).mean()
    tb2.train_steps(16)
    st2 = tb2.stats()
    assert st2["training_step"] == st0["training_step"] + 16 and np.isfinite(st2["ray_loss"])


def test_render_parity(torch_cuda):
    """Testbed::render (NerfTracer: init/advance, compaction, generate_next, inference on the EMA weights,
    composite + shade, linear accumulation over spp) against the oracle's restatement after a short
    training run. The march is bit-identical; the network output carries fp16 noise that can move a
    transmittance cut-off by one sample, so the image is compared with a tolerance: mean |diff| <= 2e-3
    over rgba and at most 1 % of values off by more than 1e-2."""
    from neus2_amd import pyngp, scenes
    import oracle as O
    sc = scenes.small_scene(n_views=8, width=64, height=48)
    tb = pyngp.Testbed(pyngp.TestbedMode.Nerf)
    tb.set_dataset(sc["images"], sc["focal"], sc["principal"], sc["xforms"], 1)
    tb.reload_network_from_file(os.path.join(ROOT, "configs", "nerf", "base.json"), batch_size=BATCH)
    tb.train_steps(60)
    st = tb.stats()
    tb.snap_to_pixel_centers = True
    tb.nerf.rendering_min_transmittance = 1e-4
    tb.set_camera_to_training_view(0)
    img = tb.render_accumulation(64, 48, spp=2)
    # render() = the accumulation through tonemap_kernel; a transparent black background and the Linear /
    # Identity defaults leave it unchanged
    tb.background_color = [0.0, 0.0, 0.0, 0.0]
    np.testing.assert_array_equal(tb.render(64, 48, spp=2), img)
    cfg = O.make_cfg(per_level_scale=tb._net_cfg.per_level_scale)
    ds = O.Dataset(sc["images"], sc["focal"], sc["principal"], sc["xforms"])
    _, bf = tb.get_density_grid()
    ref, it_ref = O.render(cfg, tb.get_ema_params(), st["valid_level"], ds, bf, sc["xforms"][0], sc["focal"][0],
                           sc["principal"][0], 64, 48, spp=2, snap=True, min_transmittance=1e-4, cos_anneal=1.0)
    d = np.abs(img - ref)
    record("render", mean_abs=d.mean(), max_abs=d.max(), frac_gt_1e2=(d > 1e-2).mean(), alpha_mean=ref[..., 3].mean(),
           iters=tb.last_render_iterations, iters_ref=it_ref)
    assert ref[..., 3].max() > 0.05, "oracle render is empty: the test would not exercise the composite"
    assert np.isfinite(img).all()
    assert d.mean() <= 2e-3, d.mean()
    assert (d > 1e-2).mean() <= 0.01, (d > 1e-2).mean()
    # PSNR against the training image itself (host metric, render_utils.py:252-359)
    psnr, _ = pyngp.eval_psnr(img, sc["images"][0])
    psnr_ref, _ = pyngp.eval_psnr(ref, sc["images"][0])
    record("render_psnr", psnr=psnr, psnr_oracle=psnr_ref)
    assert abs(psnr - psnr_ref) < 0.5


def test_free_camera_render_parity(torch_cuda):
    """render() from a free camera (camera_matrix + fov / fov_axis, python_api.cu:425-430): focal length =
    fov_to_focal_length(1, fov) * resolution[fov_axis] and screen centre 0.5 (calc_focal_length,
    render_screen_center, testbed.cu:2738-2746), against the oracle's render of the same camera (tolerance as
    test_render_parity). fov_axis 0 scales by the width."""
    from neus2_amd import pyngp
    import oracle as O
    tb = _mc_testbed()
    tb.train_steps(60)
    st = tb.stats()
    sc = tb._scene
    tb.snap_to_pixel_centers = True
    tb.nerf.rendering_min_transmittance = 1e-4
    tb.background_color = [0.0, 0.0, 0.0, 0.0]
    cfg = O.make_cfg(per_level_scale=tb._net_cfg.per_level_scale)
    ds = O.Dataset(sc["images"], sc["focal"], sc["principal"], sc["xforms"])
    _, bf = tb.get_density_grid()
    for axis, fov in ((1, 40.0), (0, 55.0)):
        tb.fov_axis = axis
        tb.fov = fov
        tb.camera_matrix = sc["xforms"][3]
        img = tb.render(64, 48, spp=1)
        fl = np.float32(pyngp.fov_to_focal_length(1, fov)) * np.float32((64, 48)[axis])
        ref, _ = O.render(cfg, tb.get_ema_params(), st["valid_level"], ds, bf, sc["xforms"][3], np.float32([fl, fl]),
                          np.float32([0.5, 0.5]), 64, 48, spp=1, snap=True, min_transmittance=1e-4, cos_anneal=1.0)
        d = np.abs(img - ref)
        record("render_free_camera", axis=axis, mean_abs=d.mean(), frac_gt_1e2=(d > 1e-2).mean(), alpha_mean=ref[..., 3].mean())
        assert ref[..., 3].max() > 0.05
        assert d.mean() <= 2e-3 and (d > 1e-2).mean() <= 0.01, (axis, d.mean(), (d > 1e-2).mean())


def test_prepare_for_test_delta_sdf(torch_cuda):
    """prepare_for_test on frame 1 with the movement training (m_use_delta, testbed.cu:1987-1999): the SDF grid
    is the network at R (x + t) (NerfNetwork::sdf through the DeltaNetwork, nerf_network.h:664-676) - against the
    oracle forward at oracle/motion.py's moved grid points; render and mesh colours go through it too (the image
    changes). On frame 0 the flag is off."""
    import motion as M
    import oracle as O
    from neus2_amd import pyngp, scenes
    frames = scenes.dynamic_scene(n_frames=2, shift=(0.02, 0.0, 0.0))
    tb = pyngp.Testbed(pyngp.TestbedMode.Nerf)
    tb.set_dataset_frames(frames)
    tb.reload_network_from_file(os.path.join(ROOT, "configs", "nerf", "base.json"), batch_size=BATCH)
    tb.train_steps(60)
    assert tb.prepare_for_test() is False
    assert tb.training_network_next_frame()
    tb.train_steps(4)  # global-movement phase: train_delta
    assert tb.prepare_for_test() is True
    p = _moved_local()
    tb.set_movement(local=p)
    st = tb.stats()
    res = (12, 10, 9)
    amin, amax = np.float32([0.2, 0.1, 0.15]), np.float32([0.8, 0.9, 0.85])
    sdf = tb.get_sdf_on_grid(res, aabb=(amin, amax))
    gz, gy, gx = np.meshgrid(*[np.arange(r, dtype=np.float32) for r in res[::-1]], indexing="ij")
    pos = np.zeros((sdf.size, 3), np.float32)
    for k, (g, r) in enumerate(zip((gx, gy, gz), res)):
        a = (g.reshape(-1) * np.float32(1.0 / r)).astype(np.float32)
        pos[:, k] = (a.astype(np.float64) * np.float64(amax[k] - amin[k]) + np.float64(amin[k])).astype(np.float32)
    coords = np.zeros((sdf.size, 7), np.float32)
    coords[:, :3] = M.delta_apply(p, pos)
    coords[:, 4:] = 0.5
    cfg = O.make_cfg(per_level_scale=tb._net_cfg.per_level_scale)
    ref = O.network_forward(cfg, tb.get_ema_params(), coords, st["valid_level"]).view(np.float16)[:, 3].astype(np.float32)
    err = np.abs(sdf.reshape(-1) - ref)
    ok = err <= 2e-3 + 4e-3 * np.abs(ref)
    record("delta_sdf_on_grid", frac_within_tol=ok.mean(), median_abs_err=np.median(err))
    assert ok.mean() >= 0.995 and np.median(err) < 1e-3, (ok.mean(), err.max())
    tb.set_camera_to_training_view(0)
    a = tb.render_accumulation(32, 24)
    ident = np.zeros(12, np.float32); ident[4] = 1; ident[8] = 1
    tb.set_movement(local=ident)
    b = tb.render_accumulation(32, 24)
    assert np.isfinite(a).all() and np.abs(a - b).max() > 1e-4
    R, t = tb.saved_transform()
    g, _ = tb.get_movement()
    np.testing.assert_allclose(R, g[:, :3], atol=1e-3)  # identity local movement: the accumulated one


def _moved_local():
    p = np.zeros(12, np.float32)
    p[:3] = [0.01, -0.02, 0.005]
    p[4:10] = [0.99, 0.05, -0.02, -0.04, 1.01, 0.03]
    return p


def test_delta_network_parity(env):
    """DeltaNetwork forward (add_global_movement_with_rotation_6d) bit-exact against oracle/motion.py on
    NerfCoordinate and NerfPosition records; backward (add_loss_to_rotation_6d_each + reduce_sum) equal to the
    restatement's fp16 gradients within one fp16 ulp (the device sums per-sample fp16 values in fp32)."""
    import motion as M
    t, tb = env["t"], env["tb"]
    lib, check = L()
    p = _moved_local()
    tb.set_movement(local=p)
    try:
        rng = np.random.default_rng(21)
        n = 3000
        c7 = np.zeros((n, 7), np.float32)
        c7[:, :3] = rng.uniform(0.05, 0.95, (n, 3))
        d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
        c7[:, 4:] = (d + 1) * 0.5
        c7[:, 3] = rng.uniform(0, 1, n)
        for stride in (7, 3):
            cin = np.ascontiguousarray(c7[:, :stride])
            out = t.zeros((n, stride), dtype=t.float32, device="cuda")
            check(lib.neus_delta_apply(tb.handle, None, C.c_uint32(n), C.c_uint32(stride), ptr(dev(t, cin)), ptr(out)))
            t.cuda.synchronize()
            np.testing.assert_array_equal(host(out, np.uint32), M.delta_apply(p, cin).view(np.uint32))
        g = rng.normal(0, 1.0, (n, 4)).astype(np.float32)
        g[:, 3] = 0
        got = np.zeros(12, np.float32)
        check(lib.neus_delta_backward(tb.handle, None, C.c_uint32(n), C.c_uint32(7), ptr(dev(t, c7)), ptr(dev(t, g)),
                                      C.c_void_p(got.ctypes.data)))
        ref = M.delta_grad(p, c7, g)
        record("delta_backward", max_rel=float(np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1e-3))))
        np.testing.assert_allclose(got, ref, rtol=2e-3, atol=1e-3)
    finally:
        ident = np.zeros(12, np.float32); ident[4] = 1; ident[8] = 1
        tb.set_movement(local=ident)


def test_net_backward_pos_parity(env):
    """dL/d(position) of the training MLP kernels (grid input gradient + density/rgb input xyz rows, the
    DeltaNetwork's upstream gradient) against the oracle: per-sample cosine and rel-L2 over the batch."""
    t, O, tb = env["t"], env["O"], env["tb"]
    lib, check = L()
    n = 1024
    c = _coords(n, 5)
    params = _perturbed(env, 15)
    rng = np.random.default_rng(6)
    dl = np.zeros((n, 16), np.float32)
    dl[:, :4] = rng.normal(0, 1e-2, (n, 4))
    dl[:, 4:7] = rng.normal(0, 1.0, (n, 3))
    dl16 = dl.astype(np.float16)
    lay = tb.layout()
    g = t.zeros(lay["n_params"], dtype=t.float32, device="cuda")
    dp = t.zeros((n, 4), dtype=t.float32, device="cuda")
    check(lib.neus_net_backward_pos(tb.handle, None, C.c_uint32(n), ptr(dev(t, c)), C.c_uint32(14), ptr(dev(t, dl16)), C.c_uint32(n),
                                    ptr(g), ptr(dp)))
    t.cuda.synchronize()
    got = dp.cpu().numpy()[:, :3].astype(np.float64)
    _, rdp = O.network_backward_pos(env["cfg"], params, c, 14, dl16.view(np.uint16), n)
    ref = rdp[:, :3].astype(np.float64)
    rel = np.linalg.norm(got - ref) / np.linalg.norm(ref)
    cos = np.sum(got * ref) / (np.linalg.norm(got) * np.linalg.norm(ref))
    record("net_backward_pos", rel=rel, cos=cos)
    assert rel <= 2e-2 and cos >= 0.999, (rel, cos)


def test_sample_rays_moved_bit_exact(env):
    """Training rays under an accumulated global movement (frames >= 1): o' = R o + t, d' = R d before the
    march (testbed_nerf.cu:1380-1387); rays, numsteps and sample coords bit-identical to the oracle."""
    t, O, tb = env["t"], env["O"], env["tb"]
    lib, check = L()
    th = 0.05
    Rt = np.zeros((3, 4), np.float32)
    Rt[:, :3] = [[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1]]
    Rt[:, 3] = [0.02, -0.01, 0.015]
    Rt = np.float16(Rt).astype(np.float32)  # the accumulated buffers are fp16
    tb.set_movement(global_Rt=Rt)
    ds = O.Dataset(env["sc"]["images"], env["sc"]["focal"], env["sc"]["principal"], env["sc"]["xforms"])
    ds.set_motion(Rt)
    try:
        bf = _bitfield(env)
        n_rays, max_s = 4096, 4096 * 16
        rs, ri = 0x7777AAAA12345678, 0xDA3E39CB94B95BDB | 1
        rays = t.zeros((n_rays, 6), dtype=t.float32, device="cuda")
        ns = t.zeros((n_rays, 2), dtype=t.int32, device="cuda")
        co = t.zeros((max_s, 7), dtype=t.float32, device="cuda")
        cnt = (C.c_uint32 * 3)()
        check(lib.neus_sample_rays(tb.handle, None, C.c_uint32(n_rays), C.c_uint32(0), C.c_uint32(1), C.c_uint32(0),
                                   C.c_uint64(rs), C.c_uint64(ri), C.c_uint32(max_s), ptr(dev(t, bf)), ptr(rays), ptr(ns), ptr(co), cnt))
        r_rays, r_ns, r_co, r_cnt, r_nr = O.generate_samples(ds, bf, n_rays, 0, rs, ri, max_s)
        np.testing.assert_array_equal(host(ns, np.uint32), r_ns)
        assert cnt[0] == r_cnt and cnt[2] == r_nr and r_nr > 0
        np.testing.assert_array_equal(host(rays, np.uint32), r_rays.view(np.uint32))
        nk = int(cnt[1])
        np.testing.assert_array_equal(host(co, np.uint32)[:nk], r_co.view(np.uint32)[:nk])
    finally:
        tb.set_movement(global_Rt=np.concatenate([np.eye(3, dtype=np.float32), np.zeros((3, 1), np.float32)], 1))


def test_dynamic_sequence_training(torch_cuda):
    """Config 4 (incremental training with predict_global_movement): frame 0 trains the canonical model; the
    next frame (the sphere shifted by +0.02 in x) starts with the global-movement phase (canonical frozen, only
    the DeltaNetwork trains), then canonical training with movement finetuning. The learned translation
    points the right way (rays map the moved frame back to the canonical sphere: t_x < 0), the phases switch
    at the configured step, and the next frame switch folds the movement into the ray transform."""
    from neus2_amd import pyngp, scenes
    frames = scenes.dynamic_scene(n_frames=3, shift=(0.02, 0.0, 0.0))
    tb = pyngp.Testbed(pyngp.TestbedMode.Nerf)
    tb.set_dataset_frames(frames)
    tb.reload_network_from_file(os.path.join(ROOT, "configs", "nerf", "base.json"), batch_size=BATCH)
    assert tb.all_training_time_frame == 3
    tb.train_steps(300)
    assert tb.training_network_next_frame()
    fs = tb.frame_state()
    assert fs["frame"] == 1 and not fs["train_canonical"] and fs["train_delta"] and tb.training_step == 0
    tb.train_steps(50)
    _, loc50 = tb.get_movement()
    tb.train_steps(1)
    fs = tb.frame_state()
    assert fs["train_canonical"] and fs["train_delta"], fs
    tb.train_steps(249)
    _, loc = tb.get_movement()
    st = tb.stats()
    record("dynamic", t50_x=loc50[0], t_x=loc[0], t_y=loc[1], t_z=loc[2], loss=st["ray_loss"])
    assert np.isfinite(loc).all() and np.isfinite(st["ray_loss"])
    assert loc50[0] < 0 and loc[0] < loc50[0], (loc50, loc)
    assert abs(loc[0]) > 2 * max(abs(loc[1]), abs(loc[2])), loc
    assert tb.training_network_next_frame()
    glob, loc2 = tb.get_movement()
    assert glob[0, 3] < 0 and abs(glob[0, 3] - np.float16(loc[0])) < 2e-3, (glob, loc)
    np.testing.assert_array_equal(loc2[:3], 0)
    assert not tb.training_network_next_frame() or tb.current_training_time_frame == 2


def _mc_testbed():
    from neus2_amd import pyngp, scenes
    sc = scenes.small_scene(n_views=8, width=64, height=48)
    tb = pyngp.Testbed(pyngp.TestbedMode.Nerf)
    tb.set_dataset(sc["images"], sc["focal"], sc["principal"], sc["xforms"], 1)
    tb.reload_network_from_file(os.path.join(ROOT, "configs", "nerf", "base.json"), batch_size=BATCH)
    tb._scene = sc
    return tb


def test_marching_cubes_parity(torch_cuda):
    """Testbed::marching_cubes on a given density grid (gen_vertices / gen_faces, marching_cubes.cu:276-420)
    against the oracle: vertices bit-exact (the same fma expression), triangles identical (both sides emit the
    canonical order: vertices by (grid point, axis), triangles by (cube, case-table row)). Ragged resolutions,
    several 2048-point chunks, a non-zero threshold, an offset aabb, empty and full grids."""
    import oracle as O
    t = torch_cuda
    tb = _mc_testbed()
    rng = np.random.default_rng(5)
    ax = lambda n: (np.arange(n) / n).astype(np.float32)
    z, y, x = np.meshgrid(ax(41), ax(33), ax(37), indexing="ij")
    sphere = (np.sqrt((x - .5) ** 2 + (y - .5) ** 2 + (z - .5) ** 2) - 0.3).astype(np.float32)
    cases = [
        (rng.normal(size=(9, 10, 11)).astype(np.float32), 0.1, (0, 0, 0), (1, 1, 1)),
        (sphere, 0.0, (-0.5, -0.25, 0.0), (1.5, 1.25, 1.0)),
        (rng.normal(size=(2, 2, 2)).astype(np.float32), 0.0, (0, 0, 0), (1, 1, 1)),
        (np.full((4, 5, 6), -1.0, np.float32), 0.0, (0, 0, 0), (1, 1, 1)),
        (np.full((4, 5, 6), 1.0, np.float32), 0.0, (0, 0, 0), (1, 1, 1)),
    ]
    for d, th, amin, amax in cases:
        m = tb.compute_marching_cubes_mesh(resolution=d.shape[::-1], aabb=(amin, amax), thresh=th, density_grid=dev(t, d))
        V, F = O.marching_cubes(d, th, amin, amax)
        assert m["V"].shape == V.shape and m["F"].shape == F.shape, (d.shape, m["V"].shape, V.shape, m["F"].shape, F.shape)
        np.testing.assert_array_equal(m["V"].view(np.uint32), V.view(np.uint32))
        np.testing.assert_array_equal(m["F"].astype(np.uint32), F)
    record("marching_cubes", n_verts_sphere=len(O.marching_cubes(sphere, 0.0)[0]))


def test_sdf_on_grid_and_mesh(torch_cuda):
    """get_density_on_grid (generate_grid_samples_nerf_uniform + NerfNetwork::sdf on the EMA weights) against
    the oracle's network forward at the same grid points (fp16-accumulation tolerance, as the forward test),
    then Testbed::marching_cubes through the network: resolution rounded to multiples of 16, a closed mesh
    inside the aabb, vertex colours in [0, 1]."""
    import oracle as O
    tb = _mc_testbed()
    tb.train_steps(60)
    st = tb.stats()
    res = (20, 17, 12)
    amin, amax = np.float32([0.1, 0.0, 0.2]), np.float32([0.9, 1.0, 0.8])
    sdf = tb.get_sdf_on_grid(res, aabb=(amin, amax))
    gz, gy, gx = np.meshgrid(*[np.arange(r, dtype=np.float32) for r in res[::-1]], indexing="ij")
    coords = np.zeros((sdf.size, 7), np.float32)
    for k, (g, r) in enumerate(zip((gx, gy, gz), res)):
        a = (g.reshape(-1) * np.float32(1.0 / r)).astype(np.float32)
        coords[:, k] = (a.astype(np.float64) * np.float64(amax[k] - amin[k]) + np.float64(amin[k])).astype(np.float32)
    coords[:, 4:] = 0.5
    cfg = O.make_cfg(per_level_scale=tb._net_cfg.per_level_scale)
    ref = O.network_forward(cfg, tb.get_ema_params(), coords, st["valid_level"]).view(np.float16)[:, 3].astype(np.float32)
    got = sdf.reshape(-1)
    err = np.abs(got - ref)
    ok = err <= 2e-3 + 4e-3 * np.abs(ref)
    record("sdf_on_grid", frac_within_tol=ok.mean(), median_abs_err=np.median(err), max_abs_err=err.max())
    assert ok.mean() >= 0.995 and np.median(err) < 1e-3, (ok.mean(), err.max())
    m = tb.compute_marching_cubes_mesh(resolution=(40, 40, 40))  # rounded up to 48^3
    V, F, Cc = m["V"], m["F"], m["C"]
    assert len(V) > 100 and len(F) > 100
    assert F.min() >= 0 and F.max() < len(V)
    assert (V >= -1e-6).all() and (V <= 1 + 1e-6).all()
    assert np.isfinite(Cc).all() and (Cc >= 0).all() and (Cc <= 1).all()
    import collections
    E = collections.Counter()
    for a, b, c in F:
        for u, v in ((a, b), (b, c), (c, a)):
            E[(int(u), int(v))] += 1
    # consistently oriented 2-manifold: every directed edge once; open edges only where the surface leaves the grid
    paired = np.mean([(v, u) in E for (u, v) in E])
    record("mc_network", n_verts=len(V), n_tris=len(F), paired_edges=paired)
    assert max(E.values()) == 1 and paired > 0.98


def test_marching_cubes_1024_network_subblocks(torch_cuda):
    """Config 5 at full size: Testbed::marching_cubes at 1024^3 through the network. Rows of the 2^30-point SDF grid
    (at the start, middle and end of the linear index range) against the oracle's forward at the same grid points
    (the fp16 tolerance of test_sdf_on_grid_and_mesh), then the mesh: indices in range, vertices inside the aabb
    and on a sign change of the SDF grid."""
    import ctypes as C
    import oracle as O
    from neus2_amd._lib import check, lib
    tb = _mc_testbed()
    tb.train_steps(60)
    st = tb.stats()
    R = 1024
    res = (C.c_int32 * 3)(R, R, R)
    lo, hi = (C.c_float * 3)(0.0, 0.0, 0.0), (C.c_float * 3)(1.0, 1.0, 1.0)
    nv, nt = C.c_uint32(), C.c_uint32()
    check(lib().neus_testbed_marching_cubes(tb.handle, res, lo, hi, C.c_float(0.0), None, C.byref(nv), C.byref(nt)))
    cfg = O.make_cfg(per_level_scale=tb._net_cfg.per_level_scale)
    ema = tb.get_ema_params()
    rows = [(0, 0), (511, 517), (1023, 1023)]  # (y, z) rows of 1024 x-consecutive points
    for y, z in rows:
        off = (z * R + y) * R
        got = np.zeros(R, np.float32)
        check(lib().neus_testbed_mc_density(tb.handle, C.c_uint64(off), C.c_uint64(R), C.c_void_p(got.ctypes.data)))
        coords = np.zeros((R, 7), np.float32)
        inv = np.float32(1.0 / R)
        coords[:, 0] = (np.arange(R, dtype=np.float32) * inv).astype(np.float32)
        coords[:, 1] = np.float32(y) * inv
        coords[:, 2] = np.float32(z) * inv
        coords[:, 4:] = 0.5
        ref = O.network_forward(cfg, ema, coords, st["valid_level"]).view(np.float16)[:, 3].astype(np.float32) + np.float32(0.0)
        err = np.abs(got - ref)
        ok = err <= 2e-3 + 4e-3 * np.abs(ref)
        record("mc1024_row", y=y, z=z, frac_within_tol=ok.mean(), max_abs_err=err.max())
        assert ok.mean() >= 0.99, ((y, z), ok.mean(), err.max())
    V = np.zeros((nv.value, 3), np.float32)
    F = np.zeros((nt.value, 3), np.uint32)
    check(lib().neus_testbed_get_mesh(tb.handle, C.c_void_p(V.ctypes.data), C.c_void_p(F.ctypes.data)))
    record("mc1024_mesh", n_verts=nv.value, n_tris=nt.value)
    assert nv.value > 10000 and nt.value > 10000
    assert F.max() < nv.value
    assert (V >= 0).all() and (V <= 1).all()
    # every edge of a triangle joins two vertices at most one grid cell apart
    e = np.linalg.norm(V[F[:, 0]] - V[F[:, 1]], axis=1)
    assert e.max() <= np.sqrt(3) / R * 1.001


def test_marching_cubes_64bit_grid_index(torch_cuda):
    """A 1664^3 grid (4.6e9 points: point, vertex-slot and cube indices beyond 2^32, where the reference's uint32
    index math wraps, marching_cubes.cu:285-287) of an analytic sphere's SDF, meshed from a device density grid:
    every vertex lies on the sphere to within a grid spacing, including those whose grid points sit past linear
    index 2^32, the vertex count matches the surface area, and faces reference existing vertices."""
    import ctypes as C
    from neus2_amd._lib import check, lib
    t = torch_cuda
    R = 1664
    c, rad = 0.5, 0.45
    d = t.empty((R, R, R), dtype=t.float32, device="cuda")
    ax = (t.arange(R, device="cuda", dtype=t.float32) / R)
    yy, xx = t.meshgrid(ax, ax, indexing="ij")
    base = (xx - c) ** 2 + (yy - c) ** 2
    for z in range(R):
        d[z] = t.sqrt(base + (float(z) / R - c) ** 2) - rad
    del yy, xx, base
    tb = _mc_testbed()
    res = (C.c_int32 * 3)(R, R, R)
    lo, hi = (C.c_float * 3)(0.0, 0.0, 0.0), (C.c_float * 3)(1.0, 1.0, 1.0)
    nv, nt = C.c_uint32(), C.c_uint32()
    check(lib().neus_testbed_marching_cubes(tb.handle, res, lo, hi, C.c_float(0.0), C.c_void_p(d.data_ptr()), C.byref(nv), C.byref(nt)))
    del d
    t.cuda.empty_cache()
    V = np.zeros((nv.value, 3), np.float32)
    F = np.zeros((nt.value, 3), np.uint32)
    check(lib().neus_testbed_get_mesh(tb.handle, C.c_void_p(V.ctypes.data), C.c_void_p(F.ctypes.data)))
    r = np.linalg.norm(V.astype(np.float64) - c, axis=1)
    h = 1.0 / R
    beyond = V[:, 2] * R * R * R + V[:, 1] * R * R >= 2.0 ** 32  # vertices owned by grid points past 2^32
    record("mc_64bit", n_verts=nv.value, n_tris=nt.value, n_beyond=beyond.sum(), max_dev=np.abs(r - rad).max() / h)
    assert beyond.sum() > 1000
    assert np.abs(r - rad).max() <= h
    assert F.max() < nv.value
    # one vertex per crossing edge: about 1.5 x area / h^2 for a sphere (x, y, z edge crossings ~ |n_x|+|n_y|+|n_z|)
    expect = 4 * np.pi * rad * rad / (h * h) * 1.5
    assert 0.9 * expect < nv.value < 1.1 * expect, (nv.value, expect)


def test_multilane_march_equals_single_lane(env):
    """The 4-, 8- and 16-lanes-per-ray segmented march (march.hip k_march<.., MG>: lanes start at slices of the ray's step
    sequence, join the previous segment's exit, re-march when they missed it) and the balanced march (k_march_bal, the
    default: a wave's 64 lanes shared by its 8 rays by length, 1-16 per ray; "8" below, "8u" the fixed 8 lanes) against the
    one-lane march, bit for bit (rays, numsteps, coordinates, counters), on random occupancy grids from sparse to full
    (many empty-cell skips landing across segment starts, long sample runs, the NERF_STEPS cap on the full grid), on
    the training bitfield and on grids of isolated occupied cells (long skips between short runs)."""
    t = env["t"]
    lib, check = L()
    from neus2_amd import pyngp
    sc = env["sc"]
    tbs = {}
    for key, lanes, bal in (("1", "1", "1"), ("4", "4", "1"), ("8", "8", "1"), ("8u", "8", "0"), ("16", "16", "1")):
        with _env(NEUS_MARCH_LANES=lanes, NEUS_MARCH_BALANCE=bal):
            tb = pyngp.Testbed(pyngp.TestbedMode.Nerf)
            tb.set_dataset(sc["images"], sc["focal"], sc["principal"], sc["xforms"], 1)
            tb.reload_network_from_file(os.path.join(ROOT, "configs", "nerf", "base.json"), batch_size=BATCH)
        tbs[key] = tb
    rng = np.random.default_rng(17)
    n_rays, max_s = 8192, 8192 * 64
    bfs = [_bitfield(env)]
    for p in (0.03, 0.3, 0.8, 1.0):
        bf = np.zeros(128 ** 3 // 8 * 8, np.uint8)
        bf[: 128 ** 3 // 8] = np.packbits(rng.random(128 ** 3) < p, bitorder="little")
        bfs.append(bf)
    # long empty stretches beside occupied cells: a blob, and single cells in 3 % of the 4^3 blocks
    G = 128
    c = (np.arange(G) + 0.5) / G
    X, Y, Z = np.meshgrid(c, c, c, indexing="ij")
    bfs.append(env["scenes"].bitfield_from_occupancy((X - 0.62) ** 2 + (Y - 0.45) ** 2 + (Z - 0.55) ** 2 < 0.09 ** 2))
    occ = np.zeros((G, G, G), bool)
    blk = rng.random((G // 4,) * 3) < 0.03
    bi = np.argwhere(blk)
    off = rng.integers(0, 4, size=bi.shape)
    occ[tuple((4 * bi + off).T)] = True
    bfs.append(env["scenes"].bitfield_from_occupancy(occ))
    for k, bf in enumerate(bfs):
        out = {}
        for lanes, tb in tbs.items():
            rays = t.zeros((n_rays, 6), dtype=t.float32, device="cuda")
            ns = t.zeros((n_rays, 2), dtype=t.int32, device="cuda")
            co = t.zeros((max_s, 7), dtype=t.float32, device="cuda")
            cnt = (C.c_uint32 * 3)()
            check(lib.neus_sample_rays(tb.handle, None, C.c_uint32(n_rays), C.c_uint32(0), C.c_uint32(1), C.c_uint32(0),
                                       C.c_uint64(0x243F6A8885A308D3 + k), C.c_uint64(0x13198A2E03707345 | 1), C.c_uint32(max_s), ptr(dev(t, bf)),
                                       ptr(rays), ptr(ns), ptr(co), cnt))
            out[lanes] = (host(rays, np.uint32).copy(), host(ns, np.uint32).copy(), host(co, np.uint32).copy(), tuple(cnt))
        a = out["1"]
        nk = int(a[3][1])
        for lanes in ("4", "8", "8u", "16"):
            b = out[lanes]
            assert a[3] == b[3], (k, lanes, a[3], b[3])
            np.testing.assert_array_equal(a[0], b[0])
            np.testing.assert_array_equal(a[1], b[1])
            np.testing.assert_array_equal(a[2][:nk], b[2][:nk])
        record("march_lanes", case=k, samples=nk, per_ray=nk / n_rays)
