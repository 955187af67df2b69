"""The two forms of a progressive round's chunk scan (march.hip k_loss_scan_chunk: one lane per ray;
k_loss_scan_chunk_group: 16 lanes per ray), each run alone through neus_debug_loss_scan_chunk and compared, as raw bits,
with a sequential np.float32 loop per ray (the reference order: w = a T; rgb += w c; ws += w; ek += e; T *= 1 - a, while
T >= 1e-4): the rays' state, the whole checkpoint arrays (pre-filled with a sentinel, so a checkpoint stored for a sample
that is not live shows up), and the appended next-round samples and open rays as sets, each ray's samples contiguous.
Rounds continue from the state the round before stored; the schedules cover chunks of 1, 5, 8 and 128 samples and rays
closed earlier (shorter than e0, stopped before e0, stopped exactly at e0). The alpha patterns put the T < 1e-4 stop at
samples 15, 16 and 17 of a chunk, on a checkpoint sample, right after an alpha of 1, nowhere (all 0), and behind a NaN
(not below the threshold: the ray stays live; which of its words are NaN is compared, not a NaN's sign, which IEEE 754
leaves open and the two kernels' operand orders decide). A training run at the bench's shape compares NEUS_SCAN_FORM=lane
and auto bitwise."""
import ctypes as C
import os

import numpy as np
import pytest

from gpu_util import dev, env, host, ptr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = 16
MAXU = 0xFFFFFFFF
SENT = 0xC2F7A5A5  # the sentinel word (about -123.8: no computation here produces it)
F = np.float32
SCHEDULES = {
    "1": [(0, 1, 2), (1, 2, MAXU), (2, MAXU, MAXU)],
    "8": [(0, 8, 16), (8, 16, MAXU), (16, MAXU, MAXU)],
    "128": [(0, 128, MAXU), (128, MAXU, MAXU)],
    "5": [(0, 5, 9), (5, 9, 20), (9, 20, MAXU), (20, MAXU, MAXU)],
}
NS = [0, 1, G - 1, G, G + 1, 2 * G, 127, 128, 129, 300]
# where a ramp ray stops (its first sample that is not live): samples G-1, G, G+1 of the chunks starting at 0, 5 and 128;
# -1: the first checkpoint sample (global index a multiple of 8) at or after the ray's sample 8
STOPS = [G - 1, G, G + 1, 5 + G - 1, 5 + G, 5 + G + 1, 128 + G - 1, 128 + G, 128 + G + 1, -1, 8, 9]
PATTERNS = ["zero", "one", "ramp", "random", "ramp", "weak", "ramp"]


def _scene(n_rays, seed=0):
    """numsteps, sa, ekt, and per ramp ray the sample it must stop at. Ray r: PATTERNS[r % 7], a sample count of NS (a ramp ray: by its stop)."""
    rng = np.random.default_rng(1000 * n_rays + seed)
    numsteps = np.zeros((n_rays, 2), np.uint32)
    base = 3
    want_stop = {}
    alphas = []
    for r in range(n_rays):
        base += r % 3  # gaps: bases are no multiples of 8 or 16
        ns = NS[(r + r // 10 + 7) % len(NS)]
        pat = PATTERNS[r % len(PATTERNS)]
        if n_rays >= 17 and r == 16:
            pat = "nan"
        j = 0
        if pat == "ramp":
            j = STOPS[(r // len(PATTERNS)) % len(STOPS)]
            if j < 0:
                j = 8 + (-(base + 8)) % 8
            ns = (j + 1, j + G, 300)[r % 3]  # the stop on the ray's last sample, inside it, far from its end
        numsteps[r] = (ns, base)
        a = np.zeros(ns, F)
        if pat == "one" and ns:
            a[(ns // 2) if r % 2 else 0] = 1.0
        elif pat == "random":
            a[:] = rng.uniform(0.0, 0.3, ns)
        elif pat == "weak":
            a[:] = rng.uniform(0.0, 0.02, ns)
        elif pat == "nan" and ns > 3:
            a[:] = rng.uniform(0.0, 0.05, ns)
            a[3] = np.nan
        elif pat == "ramp":
            n = min(j, 12)  # T = 0.9e-4 (rounded) after the n samples before j, above 1e-4 one sample earlier
            a[j - n:j] = 1.0 - 0.9e-4 ** (1.0 / n)
            want_stop[r] = j
        alphas.append(a)
        base += ns
    total = base + 1
    sa = rng.uniform(0.0, 1.0, (total, 4)).astype(F)
    sa[:, 0] = 0.5  # between the rays: never read
    ekt = rng.uniform(0.0, 2.0, total).astype(F)
    for r in range(n_rays):
        ns, b = int(numsteps[r, 0]), int(numsteps[r, 1])
        sa[b:b + ns, 0] = alphas[r]
    return numsteps, sa, ekt, want_stop


class State:
    def __init__(self, n_rays, n_samples):
        self.ccount = np.full(n_rays, SENT, np.uint32)
        self.racc = np.full((n_rays, 4), SENT, np.uint32).view(F)
        self.rT = np.full(n_rays, SENT, np.uint32).view(F)
        self.rek = np.full(n_rays, SENT, np.uint32).view(F)
        self.ck4 = np.full((n_samples // 8 + 1, 4), SENT, np.uint32).view(F)
        self.cke = np.full(n_samples // 8 + 1, SENT, np.uint32).view(F)

    def arrays(self):
        return {k: getattr(self, k) for k in ("ccount", "racc", "rT", "rek", "ck4", "cke")}


def _ref_round(numsteps, sa, ekt, st, e0, e1, e2, rays):
    """The round for `rays` on the state st (in place); returns {ray: (first sample, length)} of the next round's chunks."""
    nxt = {}
    thr = F(1e-4)
    one = F(1.0)
    with np.errstate(invalid="ignore"):
        for i in rays:
            ns, base = int(numsteps[i, 0]), int(numsteps[i, 1])
            T, r0, r1, r2, ws, ek, cn = one, F(0), F(0), F(0), F(0), F(0), 0
            is_open = e0 == 0 or ns > 0
            if e0 > 0:
                cn = int(st.ccount[i])
                if not is_open or cn != e0 or e0 >= ns or st.rT[i] < thr:
                    is_open = False
                else:
                    T, (r0, r1, r2, ws), ek = st.rT[i], st.racc[i], st.rek[i]
            to = min(ns, e1)
            k = e0
            while is_open and k < to and not (T < thr):
                s = base + k
                if s % 8 == 0:
                    st.ck4[s // 8] = (T, r0, r1, r2)
                    st.cke[s // 8] = ek
                a = sa[s, 0]
                w = a * T
                r0 = r0 + w * sa[s, 1]
                r1 = r1 + w * sa[s, 2]
                r2 = r2 + w * sa[s, 3]
                ws = ws + w
                ek = ek + ekt[s]
                T = T * (one - a)
                cn += 1
                k += 1
            if is_open:
                st.ccount[i] = cn
                st.racc[i] = (r0, r1, r2, ws)
                st.rT[i] = T
                st.rek[i] = ek
                if cn == e1 and e1 < ns and T >= thr:
                    nxt[i] = (base + e1, min(ns, e2) - e1)
    return nxt


def _gpu_round(t, form, numsteps_d, sa_d, ekt_d, st, e0, e1, e2, rays_in, n_rays, list_cap):
    """One launch of `form` on copies of the state st; returns the new state arrays and the two appended lists."""
    from neus2_amd._lib import check, lib
    d = {k: dev(t, v.view(np.uint32)) for k, v in st.arrays().items()}
    lst = t.full((list_cap + 1,), -1, dtype=t.int32, device="cuda")
    rout = t.full((n_rays + 1,), -1, dtype=t.int32, device="cuda")
    cnt = t.zeros(2, dtype=t.int32, device="cuda")
    rin = nin = None
    if rays_in is not None:
        rin = dev(t, np.concatenate([rays_in.astype(np.uint32), np.full(40, n_rays - 1, np.uint32)]))  # past the count: never read
        nin = dev(t, np.array([len(rays_in)], np.uint32))
    stream = C.c_void_p(t.cuda.current_stream().cuda_stream)
    check(lib().neus_debug_loss_scan_chunk(
        stream, C.c_int(form), C.c_uint32(n_rays), ptr(numsteps_d), ptr(sa_d), ptr(ekt_d), C.c_uint32(e0), C.c_uint32(e1), C.c_uint32(e2),
        ptr(rin), ptr(nin), ptr(d["ccount"]), ptr(d["racc"]), ptr(d["rT"]), ptr(d["rek"]), ptr(d["ck4"]), ptr(d["cke"]),
        ptr(lst), C.c_void_p(cnt.data_ptr()), ptr(rout), C.c_void_p(cnt.data_ptr() + 4)))
    out = {k: host(v, np.uint32).reshape(st.arrays()[k].shape) for k, v in d.items()}
    n_list, n_out = (int(x) for x in host(cnt, np.uint32))
    return out, host(lst, np.uint32), n_list, host(rout, np.uint32), n_out


def _bits(a):
    """The words of a state array, every float NaN as one word: IEEE 754 leaves a propagated NaN's sign and payload to the
    implementation, and the GPU's differ from numpy's, so against the reference only where the NaNs are is compared (the
    counts and the sentinel are no NaN patterns)."""
    w = np.ascontiguousarray(a).view(np.uint32).copy()
    w[np.isnan(w.view(F))] = 0x7FC00000
    return w


def _check_lists(nxt, lst, n_list, rout, n_out, where):
    assert n_out == len(nxt) and n_list == sum(m for _, m in nxt.values()), where
    assert sorted(rout[:n_out].tolist()) == sorted(nxt), where
    assert (rout[n_out:] == MAXU).all() and (lst[n_list:] == MAXU).all(), where  # nothing written past the reservations
    got = lst[:n_list].astype(np.int64)
    # each ray's chunk contiguous: the list is a concatenation of ascending runs, one per open ray
    cuts = np.flatnonzero(np.diff(got) != 1) + 1
    runs = sorted((int(r[0]), len(r)) for r in np.split(got, cuts)) if n_list else []
    assert runs == sorted(nxt.values()), where


def _run_schedule(t, n_rays, sched, permute):
    numsteps, sa, ekt, _ = _scene(n_rays)
    rng = np.random.default_rng(n_rays)
    # with a ray list: a permutation that leaves out every seventh ray, whose state stays the sentinel
    rays_in = np.array([r for r in rng.permutation(n_rays) if r % 7 != 6 or n_rays < 7], np.uint32) if permute else None
    st = State(n_rays, sa.shape[0])
    numsteps_d, sa_d, ekt_d = dev(t, numsteps), dev(t, sa), dev(t, ekt)
    rays = list(range(n_rays)) if rays_in is None else [int(r) for r in rays_in]
    for k, (e0, e1, e2) in enumerate(SCHEDULES[sched]):
        before = {key: v.copy() for key, v in st.arrays().items()}
        tmp = State(n_rays, sa.shape[0])
        for key, v in before.items():
            setattr(tmp, key, v.copy())
        nxt = _ref_round(numsteps, sa, ekt, tmp, e0, e1, e2, rays)
        for form in (0, 1):
            out, lst, n_list, rout, n_out = _gpu_round(t, form, numsteps_d, sa_d, ekt_d, st, e0, e1, e2,
                                                       None if rays_in is None else np.array(rays, np.uint32), n_rays, sa.shape[0])
            where = f"rays {n_rays} schedule {sched} round {k} form {form}"
            for key, ref in tmp.arrays().items():
                np.testing.assert_array_equal(_bits(out[key]), _bits(ref), err_msg=f"{where}: {key}")
            _check_lists(nxt, lst, n_list, rout, n_out, where)
        st = tmp
        if rays_in is not None:
            rays = sorted(nxt)[::-1]  # the next round visits the open rays (in some order)
    return st


def test_reference_stops_where_intended():
    """CPU only in effect: the ramp rays of the reference stop at the intended sample, the all-zero and NaN rays never."""
    numsteps, sa, ekt, want = _scene(200)
    st = State(200, sa.shape[0])
    _ref_round(numsteps, sa, ekt, st, 0, MAXU, MAXU, range(200))
    assert {j for j in want.values()} >= {j for j in STOPS if j > 0}
    for r, j in want.items():
        assert st.ccount[r] == j and st.rT[r] < F(1e-4), (r, j, st.ccount[r], st.rT[r])
        T_prev = st.rT[r] / (F(1) - sa[int(numsteps[r, 1]) + j - 1, 0])
        assert T_prev >= 1.2e-4, (r, T_prev)
    assert any((int(numsteps[r, 1]) + j) % 8 == 0 for r, j in want.items())
    assert np.isnan(st.rT[16]) and st.ccount[16] == numsteps[16, 0] > 3
    zero = [r for r in range(200) if PATTERNS[r % 7] == "zero" and r != 16]
    assert all(st.rT[r] == 1 and st.ccount[r] == numsteps[r, 0] for r in zero)


@pytest.mark.parametrize("permute", [False, True])
@pytest.mark.parametrize("n_rays", [1, 15, 16, 17, 63, 64, 65, 200])
def test_chunk_scan_forms_match_reference(torch_cuda, n_rays, permute):
    final = [_run_schedule(torch_cuda, n_rays, sched, permute) for sched in SCHEDULES]
    # the composited state of a ray does not depend on the schedule
    for other in final[1:]:
        # (but for a NaN ray: the next-round lists drop it, T >= 1e-4 being false, while a round over every slot continues it)
        ok = ~(np.isnan(final[0].rT) | np.isnan(other.rT))
        for key in ("ccount", "racc", "rT", "rek"):
            np.testing.assert_array_equal(other.arrays()[key].view(np.uint32)[ok], final[0].arrays()[key].view(np.uint32)[ok])


def test_last_round_alone(torch_cuda):
    """(128, 2^32-1, 2^32-1) on a state written by hand: rays with cn != e0, with e0 >= ns, and with a stored T < 1e-4 stay
    closed, the others run to their end."""
    t = torch_cuda
    n_rays = 65
    numsteps, sa, ekt, _ = _scene(n_rays, seed=1)
    st = State(n_rays, sa.shape[0])
    rng = np.random.default_rng(5)
    st.ccount[:] = np.where(np.arange(n_rays) % 4 == 1, 100, 128)
    st.rT[:] = np.where(np.arange(n_rays) % 4 == 2, F(5e-5), rng.uniform(0.01, 1.0, n_rays)).astype(F)
    st.racc[:] = rng.uniform(0, 1, (n_rays, 4)).astype(F)
    st.rek[:] = rng.uniform(0, 9, n_rays).astype(F)
    ref = State(n_rays, sa.shape[0])
    for key, v in st.arrays().items():
        setattr(ref, key, v.copy())
    nxt = _ref_round(numsteps, sa, ekt, ref, 128, MAXU, MAXU, range(n_rays))
    assert not nxt and (ref.ccount > 128).sum() >= 3
    numsteps_d, sa_d, ekt_d = dev(t, numsteps), dev(t, sa), dev(t, ekt)
    for form in (0, 1):
        out, lst, n_list, rout, n_out = _gpu_round(t, form, numsteps_d, sa_d, ekt_d, st, 128, MAXU, MAXU, None, n_rays, sa.shape[0])
        for key, r in ref.arrays().items():
            np.testing.assert_array_equal(_bits(out[key]), _bits(r), err_msg=f"form {form}: {key}")
        _check_lists(nxt, lst, n_list, rout, n_out, f"form {form}")


def test_training_scan_forms_bitwise(torch_cuda):
    """Config S with the bench's rays and batch (R = Nc = 2^18 fixed) on the bench's scene at half the resolution and 12
    views, progressive inference on, 96 steps in one call with NEUS_SCAN_FORM=lane and auto:
    the same parameters, gradients, EMA weights, occupancy grid and counters; the run had cut steps (where auto takes the
    16-lane form)."""
    from neus2_amd import pyngp, scenes
    sc = scenes.sphere_scene(12, 800, 600, focal=(1446.0, 1446.0), principal=(823.2 / 1600, 619.1 / 1200))
    n = 1 << 18
    res = {}
    for form in ("lane", "auto"):
        with env(NEUS_SCAN_FORM=form):
            tb = pyngp.Testbed(pyngp.TestbedMode.Nerf)
            tb.set_dataset(sc["images"], sc["focal"], sc["principal"], sc["xforms"], 1)
            tb.reload_network_from_file(os.path.join(ROOT, "configs", "nerf", "base.json"), batch_size=n, fixed_rays_per_batch=n)
        tb.set_progressive_inference(2)
        tb.train_steps(96)
        res[form] = (tb.stats(), tb.get_params(), tb.get_gradients(), tb.get_ema_params(), tb.get_density_grid()[0])
        del tb
    assert res["auto"][0]["cut_steps"] > 30, res["auto"][0]["cut_steps"]
    for k in ("training_step", "measured_batch_size", "measured_batch_size_before_compaction", "n_rays_total",
              "n_rays_with_samples", "progressive_steps", "cut_steps", "loss"):
        assert res["auto"][0][k] == res["lane"][0][k], k
    for x, y in zip(res["auto"][1:], res["lane"][1:]):
        np.testing.assert_array_equal(x.view(np.uint32), y.view(np.uint32))
