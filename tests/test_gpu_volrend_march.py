"""volrend.march (volrend.hip k_vr_march) against the numpy float32 restatement of tests/volrend_ref.py: exact ranges and
ray indices, t bit for bit."""
import numpy as np
import pytest

import volrend_ref as VR

pytestmark = pytest.mark.gpu
DT = float(np.float32(np.sqrt(3.0) / 64))


def run(torch, o, d, t_min, t_max, occ, dt, cap):
    from neus2_amd import volrend
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    ranges, t, ray_idx = volrend.march(dev(o), dev(d), dev(t_min), dev(t_max), dev(occ), dt, cap)
    assert ranges.dtype == torch.int32 and t.dtype == torch.float32 and ray_idx.dtype == torch.int32
    assert ranges.shape == (len(o), 2) and t.shape == ray_idx.shape == (int(ranges[:, 1].sum()),)
    return ranges.cpu().numpy(), t.cpu().numpy(), ray_idx.cpu().numpy()


@pytest.fixture(scope="module")
def case():
    c = VR.march_case()
    return c, VR.march_by_ray(*c, DT, 48)


def test_march_equals_the_float32_restatement(torch_cuda, case):
    c, (ranges, t, ray_idx) = case
    got = run(torch_cuda, *c, DT, 48)
    assert np.array_equal(got[0], ranges)
    assert np.array_equal(got[2], ray_idx)
    assert np.array_equal(got[1].view(np.uint32), t.view(np.uint32))
    n = ranges[:, 1]
    assert (n == 48).any() and (n == 0).any() and len(t) > 2000


def test_march_repeats_bit_for_bit(torch_cuda, case):
    c, _ = case
    a, b = run(torch_cuda, *c, DT, 48), run(torch_cuda, *c, DT, 48)
    assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))


def test_one_ray_and_an_empty_grid_give_empty_outputs(torch_cuda, case):
    (o, d, t_min, t_max, occ), _ = case
    ranges, t, ray_idx = run(torch_cuda, o[:1], d[:1], t_min[:1], t_max[:1], np.zeros_like(occ), DT, 48)
    assert ranges.tolist() == [[0, 0]] and t.shape == (0,) and ray_idx.shape == (0,)
    ranges, t, ray_idx = run(torch_cuda, o[:0], d[:0], t_min[:0], t_max[:0], occ, DT, 48)
    assert ranges.shape == (0, 2) and t.shape == (0,)


@pytest.mark.parametrize("G", [1, 64])
def test_other_grid_sizes_and_a_cap_of_zero(torch_cuda, case, G):
    (o, d, t_min, t_max, _), _ = case
    occ = (np.random.default_rng(G).uniform(0, 1, (G, G, G)) < (1.0 if G == 1 else 0.3)).astype(np.uint8)
    got = run(torch_cuda, o[:65], d[:65], t_min[:65], t_max[:65], occ, DT, 1000)
    ref = VR.march_by_ray(o[:65], d[:65], t_min[:65], t_max[:65], occ, DT, 1000)
    assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(got, ref)) and len(ref[1]) > 500
    assert run(torch_cuda, o[:65], d[:65], t_min[:65], t_max[:65], occ, DT, 0)[0][:, 1].sum() == 0
