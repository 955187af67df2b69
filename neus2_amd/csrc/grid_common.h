// One hash-grid level for one position: shared by the stand-alone encode kernel (grid.hip) and the
// fused encode+MLP kernels (mlp.hip), so both produce bit-identical features and dy/dx.
// Restates kernel_grid (my_tcnn grid.h:174-369) for N_POS_DIMS = 3, 2 features, linear interpolation.
#pragma once
#include "common.h"

namespace neus {

struct LevelSetup { float pos[3]; uint32_t g[3]; float scale; uint32_t hsize, res; };

__device__ __forceinline__ LevelSetup level_setup(float scale, uint32_t res, uint32_t hsize, float x, float y, float z) {
	LevelSetup s;
	s.scale = scale; s.res = res; s.hsize = hsize;
	const float in[3] = {x, y, z};
#pragma unroll
	for (int d = 0; d < 3; ++d) {
		// pos_fract (common_device.h:404-434), linear interpolation. `input * scale + 0.5f` is one
		// expression that nvcc (--fmad=true, the default) emits as a single FFMA: fused here too.
		float p = __builtin_fmaf(in[d], s.scale, 0.5f);
		float fl = floorf(p);
		s.g[d] = (uint32_t)(int)fl;
		s.pos[d] = p - fl;
	}
	return s;
}
__device__ __forceinline__ LevelSetup level_setup(const GridLevels& gl, uint32_t l, float x, float y, float z) {
	return level_setup(gl.scale[l], gl.res[l], gl.offset[l + 1] - gl.offset[l], x, y, z);
}

// 8 corner gathers (half2 each) of one level, issued together. gp points at the level's table.
__device__ __forceinline__ void gather_corners(const LevelSetup& s, const half_t* __restrict__ gp, h2 v[8]) {
#pragma unroll
	for (uint32_t idx = 0; idx < 8; ++idx) {
		const uint32_t gx = s.g[0] + (idx & 1), gy = s.g[1] + ((idx >> 1) & 1), gz = s.g[2] + ((idx >> 2) & 1);
		const uint32_t e = grid_index(s.hsize, s.res, gx, gy, gz);
		v[idx] = *(const h2*)(gp + 2 * (size_t)e);
	}
}

// The 8 corner entries of one level without a division: e[idx] == grid_index(hsize, res, corner idx) for every input,
// on a level the host has classified (grid_levels_direct_index, grid.hip; `dense` is the level's dense_bits bit, so the
// branch is wave-uniform). The y and z terms are formed once for the four (y, z) pairs.
//   hashed: the table size is a power of two, so `% hashmap_size` is a mask.
//   dense:  a cell inside the unit cube has every coordinate <= res - 1, so a corner index is at most
//           res + res^2 + res^3 < 2 hsize and one conditional subtract is the modulo. Cells outside it (negative ones
//           wrap to huge unsigned values) take the true modulo, on the rare lanes that need it.
__device__ __forceinline__ void corner_entries(const LevelSetup& s, bool dense, uint32_t e[8]) {
	const uint32_t hs = s.hsize;
	if (dense) {
		const uint32_t rr = s.res * s.res;
		const uint32_t y0 = s.g[1] * s.res, y1 = y0 + s.res, z0 = s.g[2] * rr, z1 = z0 + rr;
		const uint32_t yz[4] = {y0 + z0, y1 + z0, y0 + z1, y1 + z1};
		if (__builtin_expect(s.g[0] >= s.res || s.g[1] >= s.res || s.g[2] >= s.res, 0)) {
#pragma unroll
			for (uint32_t idx = 0; idx < 8; ++idx) e[idx] = (s.g[0] + (idx & 1) + yz[idx >> 1]) % hs;
		} else {
#pragma unroll
			for (uint32_t idx = 0; idx < 8; ++idx) {
				const uint32_t ed = s.g[0] + (idx & 1) + yz[idx >> 1];
				e[idx] = min(ed, ed - hs);  // ed < 2 hs
			}
		}
	} else {
		const uint32_t y0 = s.g[1] * 2654435761u, y1 = y0 + 2654435761u, z0 = s.g[2] * 805459861u, z1 = z0 + 805459861u;
		const uint32_t yz[4] = {y0 ^ z0, y1 ^ z0, y0 ^ z1, y1 ^ z1};
#pragma unroll
		for (uint32_t idx = 0; idx < 8; ++idx) e[idx] = ((s.g[0] + (idx & 1)) ^ yz[idx >> 1]) & (hs - 1u);
	}
}

// Features: fp16 accumulation of fp16-rounded terms, as the reference (result[f] += (T)(weight * data)).
__device__ __forceinline__ h2 interp_features(const LevelSetup& s, const h2 v[8]) {
	half_t r0 = (half_t)0.f, r1 = (half_t)0.f;
#pragma unroll
	for (uint32_t idx = 0; idx < 8; ++idx) {
		float w = 1.f;
#pragma unroll
		for (int d = 0; d < 3; ++d) w *= (idx & (1u << d)) ? s.pos[d] : 1.f - s.pos[d];
		r0 = (half_t)((float)r0 + (float)(half_t)(w * (float)v[idx][0]));
		r1 = (half_t)((float)r1 + (float)(half_t)(w * (float)v[idx][1]));
	}
	h2 out; out[0] = r0; out[1] = r1;
	return out;
}

// d(feature f)/d(x_d): grads += weight * (right - left) * pos_derivative(=1), one FFMA per term
// under nvcc --fmad=true (grid.h:330-362).
__device__ __forceinline__ void interp_dydx(const LevelSetup& s, const h2 v[8], float gr[2][3]) {
#pragma unroll
	for (int f = 0; f < 2; ++f)
#pragma unroll
		for (int d = 0; d < 3; ++d) gr[f][d] = 0.f;
#pragma unroll
	for (int gd = 0; gd < 3; ++gd) {
#pragma unroll
		for (uint32_t idx = 0; idx < 4; ++idx) {
			float w = s.scale;
			uint32_t cl = 0;
#pragma unroll
			for (int ngd = 0; ngd < 2; ++ngd) {
				const int d = ngd >= gd ? ngd + 1 : ngd;
				if (idx & (1u << ngd)) { w *= s.pos[d]; cl |= 1u << d; } else { w *= 1.f - s.pos[d]; }
			}
			const uint32_t cr = cl | (1u << gd);
			gr[0][gd] = __builtin_fmaf(w, (float)v[cr][0] - (float)v[cl][0], gr[0][gd]);
			gr[1][gd] = __builtin_fmaf(w, (float)v[cr][1] - (float)v[cl][1], gr[1][gd]);
		}
	}
}

// One level's term of d/dx (u . dL/dx), the dL_dinput of backward_backward_input (kernel_grid_backward_input_backward_input,
// grid.h:1010-1181, linear interpolation): with t[c] = T[corner c] . dL_dy of the level,
//   r[j] = scale^2 sum_{i != j} u[i] sum_c sigma_ci sigma_cj w_ck t[c]
// (sigma_cd = +-1 by corner bit d, k the axis that is neither i nor j, w_ck its interpolation weight; the i = j terms are
// zero because the weights are linear in each axis). The mixed term of a pair (i, j) serves r[i] and r[j].
__device__ __forceinline__ void level_ddx(const LevelSetup& s, const float t[8], const float u[3], float r[3]) {
	r[0] = r[1] = r[2] = 0.f;
#pragma unroll
	for (int k = 0; k < 3; ++k) {
		const int i = k == 0 ? 1 : 0, j = k == 2 ? 1 : 2;
		float m = 0.f;
#pragma unroll
		for (uint32_t c = 0; c < 8; ++c) {
			const float w = (c & (1u << k)) ? s.pos[k] : 1.f - s.pos[k];
			const bool same = ((c >> i) & 1u) == ((c >> j) & 1u);
			m += same ? w * t[c] : -(w * t[c]);
		}
		r[j] = __builtin_fmaf(u[i], m, r[j]);
		r[i] = __builtin_fmaf(u[j], m, r[i]);
	}
	const float s2 = s.scale * s.scale;
#pragma unroll
	for (int d = 0; d < 3; ++d) r[d] *= s2;
}

} // namespace neus
