// The general grid encoding of the operator modules (my_tcnn encodings/grid.h, GridEncodingTemplated): 2, 3 or 4 input
// dims, 1, 2, 4 or 8 features per level, Hash / Dense / Tiled tables, Linear or Smoothstep interpolation, fp16 or fp32
// table. The 3-D, 2-feature, hashed, linear grid keeps its own kernels (grid.hip, grid_f32.hip); this file serves every
// other config, and that one too when its config says "implementation": "general".
//   k_gnd_forward : kernel_grid (grid.h:174-369)
//   k_gnd_backward: kernel_grid_backward (grid.h:371-500): one fp32 atomicAdd per corner and feature. As in grid_f32.hip
//                   the order of the float atomics varies from call to call, so dL_dparams is NOT bitwise repeatable
//                   ("gradient_scatter": "binned" takes grid_nd_scatter.hip instead, here and for k_gnd_bbi's dL_dparams)
//   k_gnd_dx      : kernel_grid_backward_input (grid.h:804-830), the Jacobian gathered again from the input: per (level,
//                   sample) terms into a scratch [D l + d][n], added in level order by k_gnd_sum (bitwise repeatable)
//   k_gnd_bbi     : backward_backward_input (grid.h:880-1181): the second-order dL_dparams (atomics), dL_ddLdoutput = J u
//                   and the per-level terms of dL_dinput, which with Smoothstep has the diagonal second derivatives too
// Templated on <dims, features, table type>; the interpolation and the grid type are wave-uniform runtime flags. One
// lane per (sample, level), blockIdx.y = level (a level's table stays in the XCD's L2 while its blocks run); the F
// features of one corner are one vector load of 2 to 32 bytes. All arithmetic is fp32; an fp16 module rounds its output
// once. Nothing per sample is kept from the forward: every backward pass gathers again from `input`.
// Tensors of the caller (output, dL_doutput, dL_ddLdoutput) go through a PfView (pointer, sample stride, column stride,
// precision), so the same kernels serve the stand-alone AoS / SoA tensors and a FullyFusedMLP's fp16 rows [n][in_pad]
// (`pad` zero columns after the F L features).
#include "grid_nd_common.h"
#include <algorithm>
#include <cmath>
#include <stdexcept>
#include <string>

namespace neus {

namespace {

// the F features of one table row as one vector load
template <int F, class T> struct alignas(F * sizeof(T) > 16 ? 16 : F * sizeof(T)) NdRow { T v[F]; };
template <int F, class T> __device__ __forceinline__ void nd_load(const T* __restrict__ p, float v[F]) {
	const NdRow<F, T> r = *(const NdRow<F, T>*)p;
#pragma unroll
	for (int f = 0; f < F; ++f) v[f] = (float)r.v[f];
}

template <int D, int F, class T>
__global__ void __launch_bounds__(256) k_gnd_forward(uint32_t n, const GridNd G, uint32_t valid_level, const float* __restrict__ coords,
                                                     const T* __restrict__ table, const PfView out, uint32_t pad) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, l = blockIdx.y;
	if (i >= n) return;
	float acc[F];
#pragma unroll
	for (int f = 0; f < F; ++f) acc[f] = 0.f;
	if (l <= valid_level) {
		float x[D];
		nd_coords<D>(coords, i, x);
		const NdPos<D> s = nd_setup<D>(G, l, x);
		const T* tp = table + (size_t)G.gl.offset[l] * F;
#pragma unroll
		for (uint32_t c = 0; c < (1u << D); ++c) {
			float v[F];
			nd_load<F, T>(tp + (size_t)nd_index<D>(s, c) * F, v);
			const float w = nd_weight<D>(s, c);
#pragma unroll
			for (int f = 0; f < F; ++f) acc[f] = __builtin_fmaf(w, v[f], acc[f]);
		}
	}
#pragma unroll
	for (int f = 0; f < F; ++f) view_store(out, i, l * F + f, acc[f]);
	if (l == 0) for (uint32_t k = 0; k < pad; ++k) view_store(out, i, G.gl.n_levels * F + k, 0.f);
}

template <int D, int F>
__global__ void __launch_bounds__(256) k_gnd_backward(uint32_t n, const GridNd G, uint32_t valid_level, const float* __restrict__ coords,
                                                      const PfView dLdy, float* __restrict__ grads) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, l = blockIdx.y;
	if (i >= n || l > valid_level) return;
	float g[F], x[D];
#pragma unroll
	for (int f = 0; f < F; ++f) g[f] = view_load(dLdy, i, l * F + f);
	nd_coords<D>(coords, i, x);
	const NdPos<D> s = nd_setup<D>(G, l, x);
	float* gp = grads + (size_t)G.gl.offset[l] * F;
#pragma unroll
	for (uint32_t c = 0; c < (1u << D); ++c) {
		float* row = gp + (size_t)nd_index<D>(s, c) * F;
		const float w = nd_weight<D>(s, c);
#pragma unroll
		for (int f = 0; f < F; ++f) atomicAdd(row + f, w * g[f]);
	}
}

// dL/dx_j of one level = scale w'_j sum over the corner pairs (c, c + axis j) of prod_{d != j} side_d (t[c + j] - t[c]),
// t[c] = T[corner c] . dL_dy of the level (right - left differences, as grid.h:330-362)
template <int D, int F, class T>
__global__ void __launch_bounds__(256) k_gnd_dx(uint32_t n, const GridNd G, const float* __restrict__ coords, const T* __restrict__ table,
                                                const PfView dLdy, float* __restrict__ partial) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, l = blockIdx.y;
	if (i >= n) return;
	float g[F], x[D], t[1 << D];
#pragma unroll
	for (int f = 0; f < F; ++f) g[f] = view_load(dLdy, i, l * F + f);
	nd_coords<D>(coords, i, x);
	const NdPos<D> s = nd_setup<D>(G, l, x);
	const T* tp = table + (size_t)G.gl.offset[l] * F;
#pragma unroll
	for (uint32_t c = 0; c < (1u << D); ++c) {
		float v[F];
		nd_load<F, T>(tp + (size_t)nd_index<D>(s, c) * F, v);
		t[c] = 0.f;
#pragma unroll
		for (int f = 0; f < F; ++f) t[c] = __builtin_fmaf(v[f], g[f], t[c]);
	}
#pragma unroll
	for (int j = 0; j < D; ++j) {
		float r = 0.f;
#pragma unroll
		for (uint32_t c = 0; c < (1u << D); ++c)
			if (!(c & (1u << j))) r = __builtin_fmaf(-nd_dweight<D>(s, c, j), t[c | (1u << j)] - t[c], r);
		partial[(size_t)(D * l + j) * n + i] = r * (s.scale * s.dw[j]);
	}
}

// dLdx[i][d] = sum over the active levels, in level order, of partial[D l + d][i]
__global__ void __launch_bounds__(256) k_gnd_sum(uint32_t n, uint32_t D, uint32_t n_active, const float* __restrict__ partial, float* __restrict__ dLdx) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	for (uint32_t d = 0; d < D; ++d) {
		float r = 0.f;
		for (uint32_t l = 0; l < n_active; ++l) r += partial[(size_t)(D * l + d) * n + i];
		dLdx[(size_t)i * D + d] = r;
	}
}

// With u = dL_ddLdinput, a_c = sum_j u_j scale w'_j sigma_cj prod_{d != j} side_d (the corner weight's directional
// derivative along u):
//   dL_ddLdoutput_f = sum_c a_c T[c][f]                 (J u)
//   dL_dparams[c][f] += a_c dL_dy_f                     (second order)
//   dL_dinput_j = scale^2 (sum_{i != j} u_i w'_i w'_j sum_c sigma_ci sigma_cj prod_{d != i, j} side_d t[c]
//                          + u_j w''_j sum_c sigma_cj prod_{d != j} side_d t[c])       (w'' = 0 for Linear)
template <int D, int F, class T>
__global__ void __launch_bounds__(256) k_gnd_bbi(uint32_t n, const GridNd G, uint32_t valid_level, const float* __restrict__ coords,
                                                 const T* __restrict__ table, const float* __restrict__ ddx, const PfView dLdy,
                                                 float* __restrict__ grads, const PfView ddLdy, uint32_t pad, float* __restrict__ partial) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, l = blockIdx.y;
	if (i >= n) return;
	if (ddLdy.p && l == 0) for (uint32_t k = 0; k < pad; ++k) view_store(ddLdy, i, G.gl.n_levels * F + k, 0.f);
	if (l > valid_level) {
		if (ddLdy.p) {
#pragma unroll
			for (int f = 0; f < F; ++f) view_store(ddLdy, i, l * F + f, 0.f);
		}
		return;
	}
	float x[D], u[D], g[F], ju[F], r[D];
	nd_coords<D>(coords, i, x);
	nd_coords<D>(ddx, i, u);
	const NdPos<D> s = nd_setup<D>(G, l, x);
	const bool want_g = grads || partial;
#pragma unroll
	for (int f = 0; f < F; ++f) { g[f] = want_g ? view_load(dLdy, i, l * F + f) : 0.f; ju[f] = 0.f; }
#pragma unroll
	for (int d = 0; d < D; ++d) r[d] = 0.f;
	const T* tp = table + (size_t)G.gl.offset[l] * F;
	float* gp = grads ? grads + (size_t)G.gl.offset[l] * F : nullptr;
	const bool gather = ddLdy.p || partial;
#pragma unroll
	for (uint32_t c = 0; c < (1u << D); ++c) {
		const uint32_t e = nd_index<D>(s, c);
		float dwc[D], a = 0.f;
#pragma unroll
		for (int d = 0; d < D; ++d) {
			dwc[d] = nd_dweight<D>(s, c, d);
			a = __builtin_fmaf(u[d] * (s.scale * s.dw[d]), dwc[d], a);
		}
		if (gp) {
#pragma unroll
			for (int f = 0; f < F; ++f) atomicAdd(gp + (size_t)e * F + f, a * g[f]);
		}
		if (gather) {
			float v[F], t = 0.f;
			nd_load<F, T>(tp + (size_t)e * F, v);
#pragma unroll
			for (int f = 0; f < F; ++f) { ju[f] = __builtin_fmaf(a, v[f], ju[f]); t = __builtin_fmaf(v[f], g[f], t); }
#pragma unroll
			for (int j = 0; j < D; ++j) {
				float m = u[j] * s.ddw[j] * dwc[j];
#pragma unroll
				for (int k = 0; k < D; ++k)
					if (k != j) m = __builtin_fmaf(u[k] * (s.dw[k] * s.dw[j]), nd_ddweight<D>(s, c, k, j), m);
				r[j] = __builtin_fmaf(m, t, r[j]);
			}
		}
	}
	if (ddLdy.p) {
#pragma unroll
		for (int f = 0; f < F; ++f) view_store(ddLdy, i, l * F + f, ju[f]);
	}
	if (partial) {
		const float s2 = s.scale * s.scale;
#pragma unroll
		for (int d = 0; d < D; ++d) partial[(size_t)(D * l + d) * n + i] = r[d] * s2;
	}
}

void nd_check(const GridNd& G) {
	if (G.D < 2 || G.D > 4) throw std::runtime_error("grid encoding: n_input_dims must be 2, 3 or 4");
	if (G.F != 1 && G.F != 2 && G.F != 4 && G.F != 8) throw std::runtime_error("grid encoding: n_features_per_level must be 1, 2, 4 or 8");
	if (G.gl.n_levels == 0 || G.gl.n_levels > MAX_LEVELS) throw std::runtime_error("grid encoding: 1..16 levels supported");
}
uint32_t nd_active(const GridNd& G, uint32_t valid_level) { return valid_level >= G.gl.n_levels ? G.gl.n_levels : valid_level + 1; }

#define ND_CASE(d, f, CALL) \
	case d * 16 + f: if (table_f32) { CALL(d, f, float); } else { CALL(d, f, half_t); } break;
#define ND_SWITCH(CALL) \
	switch (G.D * 16 + G.F) { \
		ND_CASE(2, 1, CALL) ND_CASE(2, 2, CALL) ND_CASE(2, 4, CALL) ND_CASE(2, 8, CALL) \
		ND_CASE(3, 1, CALL) ND_CASE(3, 2, CALL) ND_CASE(3, 4, CALL) ND_CASE(3, 8, CALL) \
		ND_CASE(4, 1, CALL) ND_CASE(4, 2, CALL) ND_CASE(4, 4, CALL) ND_CASE(4, 8, CALL) \
		default: throw std::runtime_error("grid encoding: no kernel for this (n_input_dims, n_features_per_level)"); \
	}

}  // namespace

// Level tables (grid.h:1472-1508): resolution ceil(exp2(l log2(per_level_scale)) base - 1) + 1 in fp32, scale = resolution
// - 1, entries next_multiple(res^D, 8) capped at base^D (Tiled) or 2^log2_hashmap_size (Hash); Dense is not capped
GridNd make_grid_nd(uint32_t D, uint32_t F, uint32_t type, bool smooth, uint32_t n_levels, uint32_t log2_hashmap_size, uint32_t base_resolution,
                    float per_level_scale) {
	GridNd G{};
	G.D = D; G.F = F; G.type = type; G.smooth = smooth ? 1u : 0u;
	G.gl.n_levels = n_levels;
	nd_check(G);
	if (type > GRID_ND_TILED) throw std::runtime_error("grid encoding: type must be Hash, Dense or Tiled");
	if (base_resolution == 0) throw std::runtime_error("grid encoding: base_resolution must be positive");
	if (type == GRID_ND_HASH && log2_hashmap_size > 31) throw std::runtime_error("grid encoding: log2_hashmap_size must be at most 31");
	if (!(per_level_scale > 0.f)) throw std::runtime_error("grid encoding: per_level_scale must be positive");
	static const char* names[3] = {"Hash", "Dense", "Tiled"};
	const uint64_t limit = 1ull << 31;
	auto powd = [&](uint64_t b) { uint64_t r = 1; for (uint32_t d = 0; d < D; ++d) r = std::min<uint64_t>(r * b, limit * 2); return r; };
	uint64_t offset = 0;
	for (uint32_t i = 0; i < n_levels; ++i) {
		const float scale = exp2f(i * std::log2(per_level_scale)) * base_resolution - 1.0f;
		if (!(scale < 1e9f)) throw std::runtime_error("grid encoding: level " + std::to_string(i) + " has a resolution beyond 2^30");
		const uint32_t resolution = (uint32_t)(std::ceil(scale)) + 1;
		const uint64_t max_params = 0xffffffffu / 2;
		uint64_t pil = std::min<uint64_t>(powd(resolution), max_params);
		pil = (pil + 7) / 8 * 8;
		if (type == GRID_ND_TILED) pil = std::min<uint64_t>(pil, powd(base_resolution));
		else if (type == GRID_ND_HASH) pil = std::min<uint64_t>(pil, 1ull << log2_hashmap_size);
		G.gl.offset[i] = (uint32_t)offset; G.gl.res[i] = resolution; G.gl.scale[i] = (float)(resolution - 1);
		offset += pil;
		if (offset > limit)
			throw std::runtime_error(std::string(names[type]) + " grid: the table would exceed 2^31 entries (levels 0.." + std::to_string(i) +
			                         ", resolution " + std::to_string(resolution) + " in " + std::to_string(D) + " dims)");
	}
	G.gl.offset[n_levels] = (uint32_t)offset;
	if (offset * F > 0xffffffffull) throw std::runtime_error(std::string(names[type]) + " grid: the table would exceed 2^32 - 1 parameters");
	return G;
}

void launch_grid_nd_forward(hipStream_t s, uint32_t n, const GridNd& G, uint32_t valid_level, const float* coords, const void* table,
                            bool table_f32, const PfView& out, uint32_t pad) {
	nd_check(G);
	if (!n) return;
	const dim3 grid((n + 255) / 256, G.gl.n_levels);
#define ND_FWD(d, f, T) k_gnd_forward<d, f, T><<<grid, 256, 0, s>>>(n, G, valid_level, coords, (const T*)table, out, pad)
	ND_SWITCH(ND_FWD)
#undef ND_FWD
}

void launch_grid_nd_backward(hipStream_t s, uint32_t n, const GridNd& G, uint32_t valid_level, const float* coords, const PfView& dLdy, float* grads) {
	nd_check(G);
	if (!n) return;
	const bool table_f32 = true;  // no table is read
	const dim3 grid((n + 255) / 256, nd_active(G, valid_level));
#define ND_BWD(d, f, T) k_gnd_backward<d, f><<<grid, 256, 0, s>>>(n, G, valid_level, coords, dLdy, grads)
	ND_SWITCH(ND_BWD)
#undef ND_BWD
}

void launch_grid_nd_input_grad(hipStream_t s, uint32_t n, const GridNd& G, uint32_t valid_level, const float* coords, const void* table,
                               bool table_f32, const PfView& dLdy, float* partial, float* dLdx) {
	nd_check(G);
	if (!n) return;
	const uint32_t na = nd_active(G, valid_level);
	const dim3 grid((n + 255) / 256, na);
#define ND_DX(d, f, T) k_gnd_dx<d, f, T><<<grid, 256, 0, s>>>(n, G, coords, (const T*)table, dLdy, partial)
	ND_SWITCH(ND_DX)
#undef ND_DX
	k_gnd_sum<<<(n + 255) / 256, 256, 0, s>>>(n, G.D, na, partial, dLdx);
}

void launch_grid_nd_bbi(hipStream_t s, uint32_t n, const GridNd& G, uint32_t valid_level, const float* coords, const void* table, bool table_f32,
                        const float* ddx, const PfView& dLdy, float* grads, const PfView& ddLdy, uint32_t pad, float* partial, float* dLdx) {
	nd_check(G);
	if (!n) return;
	if (dLdx && !partial) throw std::runtime_error("grid encoding: dL_dinput needs the per-level scratch");
	if (!grads && !ddLdy.p && !dLdx) return;
	const uint32_t na = nd_active(G, valid_level);
	const dim3 grid((n + 255) / 256, ddLdy.p ? G.gl.n_levels : na);
	float* part = dLdx ? partial : nullptr;
#define ND_BBI(d, f, T) k_gnd_bbi<d, f, T><<<grid, 256, 0, s>>>(n, G, valid_level, coords, (const T*)table, ddx, dLdy, grads, ddLdy, pad, part)
	ND_SWITCH(ND_BBI)
#undef ND_BBI
	if (dLdx) k_gnd_sum<<<(n + 255) / 256, 256, 0, s>>>(n, G.D, na, partial, dLdx);
}

}  // namespace neus
