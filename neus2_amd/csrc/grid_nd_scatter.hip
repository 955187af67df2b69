// "gradient_scatter": "binned" of the general grid (grid_nd.hip): dL_dparams without float atomics, independent of the
// order of the samples, of the batch capacity and of scheduling.
// Contract: every contribution c = weight * dL_dy_f is the fp32 product k_gnd_backward (weight w_c) / k_gnd_bbi (weight
// a_c) form; each goes on its own to int64 fixed point, rint(c 2^32) (the resolution of grid.hip's scatter); an
// entry's contributions are summed as integers; the sum becomes fp32 once, round to nearest. A contribution that is not
// finite or whose magnitude is 2^31 or more poisons its parameter: the result is NaN. Integer addition commutes, so
// nothing here depends on an order; the sum of the magnitudes of one parameter's contributions must stay below 2^31.
//   k_gnds_lds   : a level whose F hsize accumulators fit ND_LDS_VALUES int64 of LDS is binned there: a block walks
//                  ND_LDS_SAMPLES samples with 64-bit LDS integer adds and joins its non-zero sums with 64-bit integer
//                  global atomics (all n 2^D records of a coarse level would otherwise meet in a handful of addresses)
//   k_gnds_direct: every other level: one lane per (sample, level, feature), one 64-bit integer global atomic per corner;
//                  a sample's F lanes are adjacent, so one instruction's atomics reach 64 / F pieces of 8 F bytes
//   k_gnds_finish: int64 -> fp32 once per parameter (NaN where poisoned), written (Overwrite, zeros included: no memset)
//                  or added onto what is there in one fp32 add (backward_curved on top of backward_backward); it leaves
//                  the accumulators and the poison bytes zero for the next call
// Workspace: one int64 accumulator and one poison byte per parameter of the levels in flight (9 bytes), at most
// ND_SCATTER_CAP_BYTES: when the table needs more, consecutive groups of levels go through it one after the other.
#include "grid_nd_common.h"
#include <algorithm>
#include <cmath>
#include <stdexcept>
#include <string>

namespace neus {

namespace {

constexpr uint32_t ND_LDS_VALUES = 8192;   // 64 KiB of int64 accumulators per block
constexpr uint32_t ND_LDS_SAMPLES = 2048;  // samples per block of k_gnds_lds
constexpr uint64_t ND_SCATTER_VALUE_BYTES = 9;

struct NdLevelList { uint8_t l[MAX_LEVELS]; };

// rint(c 2^32) as int64; false: c is not finite or |c| >= 2^31
__device__ __forceinline__ bool nd_fixed(float c, long long& q) {
	if (!(fabsf(c) < 2147483648.f)) return false;
	q = (long long)rintf(c * 4294967296.f);
	return true;
}

// One (sample, level, feature): its 2^D contributions, added to acc[e F + f] (LDS: the block's LDS copy of the level, else
// the level's accumulators in global memory); poison is the level's bytes in global memory. The F features of a sample
// are F adjacent lanes: each recomputes the sample's position and weights (a few dozen fp32 operations), and the F
// atomics of one corner leave in one instruction for one 8 F-byte piece of one cache line, where a lane per sample would
// send F instructions to that line.
template <int D, int F, bool SECOND, bool LDS>
__device__ __forceinline__ void nd_scatter_lane(const GridNd& G, uint32_t l, uint32_t i, uint32_t f, const float* __restrict__ coords,
                                                const float* __restrict__ ddx, const PfView& dLdy, long long* acc, uint8_t* __restrict__ poison) {
	float x[D], u[D];
	const float g = view_load(dLdy, i, l * F + f);
	nd_coords<D>(coords, i, x);
	if (SECOND) nd_coords<D>(ddx, i, u);
	const NdPos<D> s = nd_setup<D>(G, l, x);
#pragma unroll
	for (uint32_t c = 0; c < (1u << D); ++c) {
		const uint32_t e = nd_index<D>(s, c);
		float w;
		if (SECOND) {  // a_c as k_gnd_bbi forms it
			w = 0.f;
#pragma unroll
			for (int d = 0; d < D; ++d) w = __builtin_fmaf(u[d] * (s.scale * s.dw[d]), nd_dweight<D>(s, c, d), w);
		} else {
			w = nd_weight<D>(s, c);
		}
		const size_t k = (size_t)e * F + f;
		long long q;
		if (!nd_fixed(w * g, q)) poison[k] = 1;
		else if (q != 0) atomicAdd((unsigned long long*)(acc + k), (unsigned long long)q);
	}
}

template <int D, int F, bool SECOND>
__global__ void __launch_bounds__(256) k_gnds_direct(uint32_t n, const GridNd G, const NdLevelList lv, uint32_t base, const float* __restrict__ coords,
                                                     const float* __restrict__ ddx, const PfView dLdy, long long* __restrict__ acc,
                                                     uint8_t* __restrict__ poison) {
	const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, l = lv.l[blockIdx.y];  // n F <= 2^27
	const uint32_t i = t / F, f = t % F;
	if (i >= n) return;
	const size_t o = (size_t)(G.gl.offset[l] - base) * F;
	nd_scatter_lane<D, F, SECOND, false>(G, l, i, f, coords, ddx, dLdy, acc + o, poison + o);
}

template <int D, int F, bool SECOND>
__global__ void __launch_bounds__(256) k_gnds_lds(uint32_t n, const GridNd G, const NdLevelList lv, uint32_t base, const float* __restrict__ coords,
                                                  const float* __restrict__ ddx, const PfView dLdy, long long* __restrict__ acc,
                                                  uint8_t* __restrict__ poison) {
	__shared__ long long sh[ND_LDS_VALUES];
	const uint32_t l = lv.l[blockIdx.y];
	const uint32_t values = (G.gl.offset[l + 1] - G.gl.offset[l]) * F;  // <= ND_LDS_VALUES: the host's choice of this kernel
	const size_t o = (size_t)(G.gl.offset[l] - base) * F;
	for (uint32_t k = threadIdx.x; k < values; k += blockDim.x) sh[k] = 0;
	__syncthreads();
	const uint32_t t0 = blockIdx.x * ND_LDS_SAMPLES * F, t1 = min(n, (blockIdx.x + 1) * ND_LDS_SAMPLES) * F;
	for (uint32_t t = t0 + threadIdx.x; t < t1; t += blockDim.x) nd_scatter_lane<D, F, SECOND, true>(G, l, t / F, t % F, coords, ddx, dLdy, sh, poison + o);
	__syncthreads();
	for (uint32_t k = threadIdx.x; k < values; k += blockDim.x) {
		const long long v = sh[k];
		if (v != 0) atomicAdd((unsigned long long*)(acc + o + k), (unsigned long long)v);
	}
}

__global__ void __launch_bounds__(256) k_gnds_finish(uint64_t count, long long* __restrict__ acc, uint8_t* __restrict__ poison, float* __restrict__ out,
                                                     uint32_t add) {
	const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (k >= count) return;
	const long long v = acc[k];
	const uint8_t p = poison[k];
	if (v != 0) acc[k] = 0;
	if (p) poison[k] = 0;
	const float r = p ? __builtin_nanf("") : (float)v * 0x1p-32f;
	out[k] = add ? out[k] + r : r;
}

uint64_t nd_level_values(const GridNd& G, uint32_t l) { return (uint64_t)(G.gl.offset[l + 1] - G.gl.offset[l]) * G.F; }
// levels [l0, end) share the workspace: as many consecutive levels as the cap holds
uint32_t nd_group_end(const GridNd& G, uint32_t l0, uint32_t l_end) {
	const uint64_t cap = ND_SCATTER_CAP_BYTES / ND_SCATTER_VALUE_BYTES;
	uint64_t sum = 0;
	uint32_t l = l0;
	for (; l < l_end && sum + nd_level_values(G, l) <= cap; ++l) sum += nd_level_values(G, l);
	if (l == l0)
		throw std::runtime_error("grid encoding: gradient_scatter binned: level " + std::to_string(l0) + " alone needs " +
		                         std::to_string(nd_level_values(G, l0) * ND_SCATTER_VALUE_BYTES) + " bytes of accumulators, above the cap of " +
		                         std::to_string(ND_SCATTER_CAP_BYTES) + " (use gradient_scatter atomic)");
	return l;
}
void nd_scatter_check(const GridNd& G) {
	if (G.D < 2 || G.D > 4 || (G.F != 1 && G.F != 2 && G.F != 4 && G.F != 8) || G.gl.n_levels == 0 || G.gl.n_levels > MAX_LEVELS)
		throw std::runtime_error("grid encoding: no scatter kernel for this (n_input_dims, n_features_per_level, n_levels)");
}
void nd_memset(hipStream_t s, void* p, size_t bytes) {
	if (bytes && hipMemsetAsync(p, 0, bytes, s) != hipSuccess) throw std::runtime_error("grid encoding: hipMemsetAsync failed");
}

}  // namespace

uint64_t grid_nd_scatter_values(const GridNd& G) {
	nd_scatter_check(G);
	uint64_t most = 0;
	for (uint32_t l0 = 0; l0 < G.gl.n_levels;) {
		const uint32_t l1 = nd_group_end(G, l0, G.gl.n_levels);
		most = std::max<uint64_t>(most, (uint64_t)(G.gl.offset[l1] - G.gl.offset[l0]) * G.F);
		l0 = l1;
	}
	return most;
}

void launch_grid_nd_scatter(hipStream_t s, uint32_t n, const GridNd& G, uint32_t valid_level, const float* coords, const float* ddx, const PfView& dLdy,
                            float* grads, bool add, long long* acc, uint8_t* poison) {
	nd_scatter_check(G);
	const uint32_t L = G.gl.n_levels, F = G.F;
	const uint32_t na = !n ? 0 : (valid_level >= L ? L : valid_level + 1);
	// the levels above the valid one (n = 0: every level) receive nothing: exact zeros
	if (!add) nd_memset(s, grads + (size_t)G.gl.offset[na] * F, (size_t)(G.gl.offset[L] - G.gl.offset[na]) * F * sizeof(float));
	for (uint32_t l0 = 0; l0 < na;) {
		const uint32_t l1 = nd_group_end(G, l0, na), base = G.gl.offset[l0];
		NdLevelList in_lds{}, direct{};
		uint32_t n_lds = 0, n_direct = 0;
		for (uint32_t l = l0; l < l1; ++l) {
			if (nd_level_values(G, l) <= ND_LDS_VALUES) in_lds.l[n_lds++] = (uint8_t)l;
			else direct.l[n_direct++] = (uint8_t)l;
		}
		const dim3 grid_lds((n + ND_LDS_SAMPLES - 1) / ND_LDS_SAMPLES, n_lds), grid_direct((n * F + 255) / 256, n_direct);
#define ND_SCATTER(d, f) \
	case d * 16 + f: \
		if (ddx) { \
			if (n_lds) k_gnds_lds<d, f, true><<<grid_lds, 256, 0, s>>>(n, G, in_lds, base, coords, ddx, dLdy, acc, poison); \
			if (n_direct) k_gnds_direct<d, f, true><<<grid_direct, 256, 0, s>>>(n, G, direct, base, coords, ddx, dLdy, acc, poison); \
		} else { \
			if (n_lds) k_gnds_lds<d, f, false><<<grid_lds, 256, 0, s>>>(n, G, in_lds, base, coords, ddx, dLdy, acc, poison); \
			if (n_direct) k_gnds_direct<d, f, false><<<grid_direct, 256, 0, s>>>(n, G, direct, base, coords, ddx, dLdy, acc, poison); \
		} \
		break;
		switch (G.D * 16 + F) {
			ND_SCATTER(2, 1) ND_SCATTER(2, 2) ND_SCATTER(2, 4) ND_SCATTER(2, 8)
			ND_SCATTER(3, 1) ND_SCATTER(3, 2) ND_SCATTER(3, 4) ND_SCATTER(3, 8)
			ND_SCATTER(4, 1) ND_SCATTER(4, 2) ND_SCATTER(4, 4) ND_SCATTER(4, 8)
		}
#undef ND_SCATTER
		const uint64_t count = (uint64_t)(G.gl.offset[l1] - base) * F;
		k_gnds_finish<<<(uint32_t)((count + 255) / 256), 256, 0, s>>>(count, acc, poison, grads + (size_t)base * F, add ? 1u : 0u);
		l0 = l1;
	}
}

}  // namespace neus
