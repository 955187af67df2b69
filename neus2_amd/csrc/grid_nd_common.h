// What the general grid's kernels share (grid_nd.hip, grid_nd_scatter.hip): the per-level position of a sample, the
// table index of a corner, the corner weights and their derivatives, and the access to a caller's tensor (PfView).
#pragma once
#include "kernels.h"

namespace neus {

namespace {

template <int D> struct NdPos {
	uint32_t g[D];
	float w[D], dw[D], ddw[D];  // interpolation weight of the upper corner along d, its first and second derivative in the fraction
	float scale;
	uint32_t hsize, res;
	bool hash, pow2;
};

// pos_fract (common_device.h:404-434): fmaf(x, scale, 0.5f), floor and fraction as level_setup (grid_common.h); Smoothstep
// t^2 (3 - 2 t), derivative 6 t (1 - t), second derivative 6 - 12 t
template <int D> __device__ __forceinline__ NdPos<D> nd_setup(const GridNd& G, uint32_t l, const float* __restrict__ x) {
	NdPos<D> s;
	s.scale = G.gl.scale[l]; s.res = G.gl.res[l]; s.hsize = G.gl.offset[l + 1] - G.gl.offset[l];
	s.hash = G.type == GRID_ND_HASH;
	s.pow2 = (s.hsize & (s.hsize - 1)) == 0;
#pragma unroll
	for (int d = 0; d < D; ++d) {
		const float p = __builtin_fmaf(x[d], s.scale, 0.5f);
		const float fl = floorf(p);
		s.g[d] = (uint32_t)(int)fl;
		const float t = p - fl;
		if (G.smooth) {
			s.w[d] = t * t * (3.f - 2.f * t);
			s.dw[d] = 6.f * t * (1.f - t);
			s.ddw[d] = 6.f - 12.f * t;
		} else {
			s.w[d] = t; s.dw[d] = 1.f; s.ddw[d] = 0.f;
		}
	}
	return s;
}

// grid_index (grid.h:137-153): strides accumulate while stride <= level size (the early exit makes a Tiled level tile), a
// Hash level smaller than its resolution takes the xor of pos[d] * prime[d]; modulo the level size
template <int D> __device__ __forceinline__ uint32_t nd_index(const NdPos<D>& s, uint32_t c) {
	constexpr uint32_t primes[4] = {1u, 2654435761u, 805459861u, 3674653429u};
	uint32_t stride = 1, index = 0, h = 0;
#pragma unroll
	for (int d = 0; d < D; ++d) {
		const uint32_t p = s.g[d] + ((c >> d) & 1u);
		if (stride <= s.hsize) { index += p * stride; stride *= s.res; }
		h ^= p * primes[d];
	}
	if (s.hash && s.hsize < stride) index = h;
	return s.pow2 ? index & (s.hsize - 1) : index % s.hsize;
}

template <int D> __device__ __forceinline__ float nd_side(const NdPos<D>& s, uint32_t c, int d) { return (c & (1u << d)) ? s.w[d] : 1.f - s.w[d]; }
// the corner's interpolation weight
template <int D> __device__ __forceinline__ float nd_weight(const NdPos<D>& s, uint32_t c) {
	float w = 1.f;
#pragma unroll
	for (int d = 0; d < D; ++d) w *= nd_side(s, c, d);
	return w;
}
// sigma_cj prod_{d != j} side_d: the corner's weight differentiated in the weight of axis j (sigma = +-1 by corner bit j)
template <int D> __device__ __forceinline__ float nd_dweight(const NdPos<D>& s, uint32_t c, int j) {
	float w = (c & (1u << j)) ? 1.f : -1.f;
#pragma unroll
	for (int d = 0; d < D; ++d) if (d != j) w *= nd_side(s, c, d);
	return w;
}
// sigma_ci sigma_cj prod_{d != i, j} side_d
template <int D> __device__ __forceinline__ float nd_ddweight(const NdPos<D>& s, uint32_t c, int i, int j) {
	float w = (((c >> i) ^ (c >> j)) & 1u) ? -1.f : 1.f;
#pragma unroll
	for (int d = 0; d < D; ++d) if (d != i && d != j) w *= nd_side(s, c, d);
	return w;
}

__device__ __forceinline__ float view_load(const PfView& v, uint32_t i, uint32_t k) {
	const size_t a = (size_t)i * v.ss + (size_t)k * v.sk;
	return v.f32 ? ((const float*)v.p)[a] : (float)((const half_t*)v.p)[a];
}
__device__ __forceinline__ void view_store(const PfView& v, uint32_t i, uint32_t k, float x) {
	const size_t a = (size_t)i * v.ss + (size_t)k * v.sk;
	if (v.f32) ((float*)v.p)[a] = x; else ((half_t*)v.p)[a] = (half_t)x;
}
template <int D> __device__ __forceinline__ void nd_coords(const float* __restrict__ coords, uint32_t i, float x[D]) {
#pragma unroll
	for (int d = 0; d < D; ++d) x[d] = coords[(size_t)i * D + d];
}

}  // namespace

}  // namespace neus
