// Stand-alone, differentiable NeuS rendering operators over packed rays (neus_volrend_*): the
// occupancy march, the SDF-to-alpha conversion, and the transmittance compositing with its early stop. No Testbed,
// no dataset, no RNG: device pointers, sizes and the caller's stream. Compiled without FMA contraction, so the
// march's t and positions are one multiply then one add (a numpy float32 restatement reproduces them bit for bit).
//
// Packed rays: ranges [R][2] int32 = (start, count), a ray's samples contiguous in [start, start + count). A range
// that does not lie inside [0, n_samples) is treated as empty by every kernel (no access outside the tensors).
//
// No atomics anywhere in this file: every output has one writer and every sum a fixed order, so all results are
// bitwise repeatable run to run.
#include "kernels.h"
#include <stdexcept>
#include <string>

namespace neus {
namespace {

constexpr uint32_t VR_BLOCK = 256;
// Rays with more samples than this take the wave-per-ray kernels (coalesced loads, wave-level scans); the others one
// lane per ray. Depends on `ranges` alone: both kernels of a pair are launched over all rays and each ray is taken by
// exactly one of them.
constexpr int32_t VR_LONG_RAY = 32;
// The march ends a ray after this many steps whatever t_max says (k stays exact in fp32; an infinite or NaN interval
// cannot spin a lane forever).
constexpr uint32_t VR_MAX_STEPS = 1u << 24;

// ---------------------------------------------------------------- wave64 scans (DPP, every lane active)
__device__ __forceinline__ float wave_incl_sum_f(float x) {
	x += dpp_f32<DPP_ROW_SHR + 1>(0.f, x);
	x += dpp_f32<DPP_ROW_SHR + 2>(0.f, x);
	x += dpp_f32<DPP_ROW_SHR + 4>(0.f, x);
	x += dpp_f32<DPP_ROW_SHR + 8>(0.f, x);
	x += dpp_f32<DPP_BCAST15, 0xa>(0.f, x);
	x += dpp_f32<DPP_BCAST31, 0xc>(0.f, x);
	return x;
}
__device__ __forceinline__ float wave_lane_f(float x, int lane) {
	return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), lane));
}
__device__ __forceinline__ float wave_sum_f(float x) { return wave_lane_f(wave_incl_sum_f(x), 63); }
__device__ __forceinline__ float wave_incl_prod_f(float x) {
	x *= dpp_f32<DPP_ROW_SHR + 1>(1.f, x);
	x *= dpp_f32<DPP_ROW_SHR + 2>(1.f, x);
	x *= dpp_f32<DPP_ROW_SHR + 4>(1.f, x);
	x *= dpp_f32<DPP_ROW_SHR + 8>(1.f, x);
	x *= dpp_f32<DPP_BCAST15, 0xa>(1.f, x);
	x *= dpp_f32<DPP_BCAST31, 0xc>(1.f, x);
	return x;
}
// One step of the inclusive scan of affine maps x -> m x + b under composition, the earlier lanes' map applied first:
// (m, b) := (m, b) o (pm, pb).
template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ void affine_step(float& m, float& b) {
	const float pm = dpp_f32<CTRL, ROW_MASK>(1.f, m), pb = dpp_f32<CTRL, ROW_MASK>(0.f, b);
	b = m * pb + b;
	m = m * pm;
}
__device__ __forceinline__ void wave_incl_affine(float& m, float& b) {
	affine_step<DPP_ROW_SHR + 1>(m, b);
	affine_step<DPP_ROW_SHR + 2>(m, b);
	affine_step<DPP_ROW_SHR + 4>(m, b);
	affine_step<DPP_ROW_SHR + 8>(m, b);
	affine_step<DPP_BCAST15, 0xa>(m, b);
	affine_step<DPP_BCAST31, 0xc>(m, b);
}

// (start, count) of ray r, empty unless it lies inside [0, n_samples)
__device__ __forceinline__ void ray_range(const int32_t* __restrict__ ranges, uint32_t r, uint32_t n_samples, int32_t& start, int32_t& count) {
	start = ranges[2 * r]; count = ranges[2 * r + 1];
	if (start < 0 || count < 0 || (uint64_t)(uint32_t)start + (uint32_t)count > n_samples) { start = 0; count = 0; }
}

// ---------------------------------------------------------------- march
// Step k: t_k = t_min + (k + 0.5) dt; the ray ends at the first t_k >= t_max; p = o + t_k d; kept when p is in [0, 1)^3,
// its cell is occupied and fewer than max_per_ray steps were kept. WRITE = false counts, WRITE = true fills t / ray_idx.
template <bool WRITE>
__global__ void __launch_bounds__(64) k_vr_march(uint32_t n_rays, const float* __restrict__ rays_o, const float* __restrict__ rays_d,
                                                 const float* __restrict__ t_min, const float* __restrict__ t_max,
                                                 const uint8_t* __restrict__ occ, uint32_t G, float dt, uint32_t max_per_ray,
                                                 int32_t* __restrict__ counts, const int32_t* __restrict__ ranges, uint32_t n_samples,
                                                 float* __restrict__ t_out, int32_t* __restrict__ ray_idx) {
	const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
	if (r >= n_rays) return;
	const float o[3] = {rays_o[3 * r], rays_o[3 * r + 1], rays_o[3 * r + 2]};
	const float d[3] = {rays_d[3 * r], rays_d[3 * r + 1], rays_d[3 * r + 2]};
	const float t0 = t_min[r], t1 = t_max[r], Gf = (float)G;
	uint32_t cap = max_per_ray;
	int32_t start = 0;
	if (WRITE) {
		int32_t count;
		ray_range(ranges, r, n_samples, start, count);
		cap = min(cap, (uint32_t)count);
	}
	uint32_t n = 0;
	for (uint32_t k = 0; k < VR_MAX_STEPS && n < cap; ++k) {
		const float t = t0 + ((float)k + 0.5f) * dt;
		if (!(t < t1)) break;
		const float p[3] = {o[0] + t * d[0], o[1] + t * d[1], o[2] + t * d[2]};
		if (!(p[0] >= 0.f && p[0] < 1.f && p[1] >= 0.f && p[1] < 1.f && p[2] >= 0.f && p[2] < 1.f)) continue;
		const uint32_t x = (uint32_t)(int)(p[0] * Gf), y = (uint32_t)(int)(p[1] * Gf), z = (uint32_t)(int)(p[2] * Gf);
		if (!occ[((size_t)z * G + y) * G + x]) continue;
		if (WRITE) { t_out[start + n] = t; ray_idx[start + n] = (int32_t)r; }
		++n;
	}
	if (!WRITE) counts[r] = (int32_t)n;
}

// ---------------------------------------------------------------- NeuS alpha
__device__ __forceinline__ float vr_logistic(float x) { return 1.0f / (1.0f + expf(-x)); }

// (p + 1e-5) / (c + 1e-5), before the clamp
__device__ __forceinline__ float alpha_ratio(float sdf, float cosv, float dt, float inv_s, float ratio) {
	const float u1 = 0.5f - 0.5f * cosv, u2 = -cosv;
	const float a1 = u1 > 0.f ? u1 : 0.f, a2 = u2 > 0.f ? u2 : 0.f;
	const float iter_cos = -(a1 * (1.f - ratio) + a2 * ratio);
	const float h = iter_cos * (dt * 0.5f);
	const float c = vr_logistic((sdf - h) * inv_s), n = vr_logistic((sdf + h) * inv_s);
	return ((c - n) + 1e-5f) / (c + 1e-5f);
}

__global__ void __launch_bounds__(VR_BLOCK) k_vr_alpha_fwd(uint32_t n, const float* __restrict__ sdf, const float* __restrict__ true_cos,
                                                            const float* __restrict__ dt, float dt_value, const float* __restrict__ inv_s,
                                                            float inv_s_value, float ratio, float* __restrict__ alpha) {
	const uint32_t i = blockIdx.x * VR_BLOCK + threadIdx.x;
	if (i >= n) return;
	const float s = inv_s ? inv_s[0] : inv_s_value;
	alpha[i] = fminf(fmaxf(alpha_ratio(sdf[i], true_cos[i], dt ? dt[i] : dt_value, s, ratio), 0.f), 1.f);
}

// Recomputes the forward from its inputs, in fp64: d alpha / d sdf is the difference of two nearly equal logistic slopes
// (prev_sdf and next_sdf lie dt apart), which in fp32 keeps three or four digits; the kernel moves 28 B per sample, so
// the fp64 arithmetic hides behind its memory traffic. d/d inv_s: the block's 256 fp64 terms are summed in a fixed order
// (wave scan, then the four waves in order) into partial[blockIdx.x]; k_vr_sum_partials adds the partials.
__device__ __forceinline__ double wave_sum_d(double x) {
#pragma unroll
	for (int o = 1; o < 64; o <<= 1) x += __shfl_xor(x, o);  // butterfly: the same order on every lane and run
	return x;
}
__global__ void __launch_bounds__(VR_BLOCK) k_vr_alpha_bwd(uint32_t n, const float* __restrict__ sdf, const float* __restrict__ true_cos,
                                                            const float* __restrict__ dt, float dt_value, const float* __restrict__ inv_s,
                                                            float inv_s_value, float ratio_f, const float* __restrict__ g_alpha,
                                                            float* __restrict__ g_sdf, float* __restrict__ g_cos, double* __restrict__ partial) {
	__shared__ double s_part[VR_BLOCK / 64];
	const uint32_t i = blockIdx.x * VR_BLOCK + threadIdx.x;
	double gs = 0.0;
	if (i < n) {
		const double s = inv_s ? inv_s[0] : inv_s_value, ratio = ratio_f;
		const double x = sdf[i], cosv = true_cos[i], half_dt = 0.5 * (double)(dt ? dt[i] : dt_value);
		const double u1 = 0.5 - 0.5 * cosv, u2 = -cosv;
		const double a1 = u1 > 0.0 ? u1 : 0.0, a2 = u2 > 0.0 ? u2 : 0.0;
		const double h = -(a1 * (1.0 - ratio) + a2 * ratio) * half_dt;
		const double prev = x - h, next = x + h;
		const double c = 1.0 / (1.0 + exp(-prev * s)), nn = 1.0 / (1.0 + exp(-next * s));
		const double den = c + 1e-5, q = ((c - nn) + 1e-5) / den;
		const double g = (q >= 0.0 && q <= 1.0) ? (double)g_alpha[i] : 0.0;  // the clamp passes no gradient where it cuts
		// q = (c - n + eps) / (c + eps): dq/dc = n / (c + eps)^2, dq/dn = -1 / (c + eps)
		const double g_xp = g * (nn / (den * den)) * (c * (1.0 - c));
		const double g_xn = -(g / den) * (nn * (1.0 - nn));
		g_sdf[i] = (float)(s * (g_xp + g_xn));
		gs = g_xp * prev + g_xn * next;
		const double g_iter = s * (g_xn - g_xp) * half_dt;
		g_cos[i] = (float)(g_iter * (0.5 * (1.0 - ratio) * (u1 > 0.0 ? 1.0 : 0.0) + ratio * (u2 > 0.0 ? 1.0 : 0.0)));
	}
	const double ws = wave_sum_d(gs);
	if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = ws;
	__syncthreads();
	if (threadIdx.x == 0) partial[blockIdx.x] = ((s_part[0] + s_part[1]) + s_part[2]) + s_part[3];
}

// One block: thread t adds partial[t], partial[t + 256], ... in index order, then the 256 sums go through the same
// fixed wave and block order; the fp64 total is rounded to fp32 once. Appending zero partials changes no bit of it.
__global__ void __launch_bounds__(VR_BLOCK) k_vr_sum_partials(uint32_t n, const double* __restrict__ partial, float* __restrict__ out) {
	__shared__ double s_part[VR_BLOCK / 64];
	double acc = 0.0;
	for (uint32_t i = threadIdx.x; i < n; i += VR_BLOCK) acc += partial[i];
	const double ws = wave_sum_d(acc);
	if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = ws;
	__syncthreads();
	if (threadIdx.x == 0) out[0] = (float)(((s_part[0] + s_part[1]) + s_part[2]) + s_part[3]);
}

// ---------------------------------------------------------------- composite, rays of at most VR_LONG_RAY samples
// One lane per ray, the serial definition as written. Consecutive rays' samples are consecutive in memory, so a wave's
// loads fall on few lines while the rays are short; the loads of U samples are issued together (clamped indices, ahead
// of the data-dependent stop) before they go through the recurrence.
template <int C>
__global__ void __launch_bounds__(64) k_vr_comp_fwd_lane(uint32_t n_rays, uint32_t n_samples, const float* __restrict__ alpha,
                                                         const float* __restrict__ values, const int32_t* __restrict__ ranges, float t_stop,
                                                         float* __restrict__ out, float* __restrict__ opacity, float* __restrict__ weights,
                                                         float* __restrict__ trans, int32_t* __restrict__ n_comp) {
	const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
	if (r >= n_rays) return;
	int32_t start, count;
	ray_range(ranges, r, n_samples, start, count);
	if (count > VR_LONG_RAY) return;
	constexpr int U = 8;
	float T = 1.f, op = 0.f, acc[C];
#pragma unroll
	for (int c = 0; c < C; ++c) acc[c] = 0.f;
	int32_t n = 0;
	bool live = true;
	for (int32_t base = 0; base < count; base += U) {
		float a[U], v[U][C];
#pragma unroll
		for (int u = 0; u < U; ++u) {
			const size_t s = (size_t)start + min(base + u, count - 1);
			a[u] = alpha[s];
#pragma unroll
			for (int c = 0; c < C; ++c) v[u][c] = values[s * C + c];
		}
#pragma unroll
		for (int u = 0; u < U; ++u) {
			if (base + u < count) {
				const size_t s = (size_t)start + base + u;
				live = live && !(T < t_stop);
				const float w = live ? a[u] * T : 0.f;
				weights[s] = w;
				trans[s] = live ? T : 0.f;
				if (live) {
#pragma unroll
					for (int c = 0; c < C; ++c) acc[c] += w * v[u][c];
					op += w;
					T *= 1.f - a[u];
					++n;
				}
			}
		}
	}
#pragma unroll
	for (int c = 0; c < C; ++c) out[(size_t)r * C + c] = acc[c];
	opacity[r] = op;
	n_comp[r] = n;
}

template <int C>
__global__ void __launch_bounds__(64) k_vr_comp_bwd_lane(uint32_t n_rays, uint32_t n_samples, const float* __restrict__ alpha,
                                                         const float* __restrict__ values, const int32_t* __restrict__ ranges,
                                                         const float* __restrict__ trans, const int32_t* __restrict__ n_comp,
                                                         const float* __restrict__ g_out, const float* __restrict__ g_opacity,
                                                         const float* __restrict__ g_weights, float* __restrict__ g_alpha,
                                                         float* __restrict__ g_values) {
	const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
	if (r >= n_rays) return;
	int32_t start, count;
	ray_range(ranges, r, n_samples, start, count);
	if (count > VR_LONG_RAY) return;
	const int32_t n = min(max(n_comp[r], 0), count);
	float go[C];
#pragma unroll
	for (int c = 0; c < C; ++c) go[c] = g_out[(size_t)r * C + c];
	const float gop = g_opacity[r];
	for (int32_t i = n; i < count; ++i) {  // from the stop on: no gradient
		const size_t s = (size_t)start + i;
		g_alpha[s] = 0.f;
#pragma unroll
		for (int c = 0; c < C; ++c) g_values[s * C + c] = 0.f;
	}
	constexpr int U = 8;
	float B = 0.f;
	for (int32_t hi = n; hi > 0; hi -= U) {
		float a[U], T[U], gw[U], v[U][C];
#pragma unroll
		for (int u = 0; u < U; ++u) {
			const size_t s = (size_t)start + max(hi - 1 - u, 0);
			a[u] = alpha[s]; T[u] = trans[s]; gw[u] = g_weights ? g_weights[s] : 0.f;
#pragma unroll
			for (int c = 0; c < C; ++c) v[u][c] = values[s * C + c];
		}
#pragma unroll
		for (int u = 0; u < U; ++u) {
			if (hi - 1 - u >= 0) {
				const size_t s = (size_t)start + (hi - 1 - u);
				float Gi = gw[u] + gop;
#pragma unroll
				for (int c = 0; c < C; ++c) Gi += go[c] * v[u][c];
				g_alpha[s] = T[u] * (Gi - B);
				const float w = a[u] * T[u];
#pragma unroll
				for (int c = 0; c < C; ++c) g_values[s * C + c] = w * go[c];
				B = a[u] * Gi + (1.f - a[u]) * B;
			}
		}
	}
}

// ---------------------------------------------------------------- composite, rays of more than VR_LONG_RAY samples
// One wave per ray, 64 samples per round with coalesced loads. Forward: the inclusive product of (1 - alpha) over the
// lanes (DPP scan) times the carried T gives every sample's T_i at once; the stop is the first lane whose T_i is below
// t_stop (ballot); the channel sums are wave sums added to the carry in round order.
template <int C>
__global__ void __launch_bounds__(VR_BLOCK) k_vr_comp_fwd_wave(uint32_t n_rays, uint32_t n_samples, const float* __restrict__ alpha,
                                                                const float* __restrict__ values, const int32_t* __restrict__ ranges, float t_stop,
                                                                float* __restrict__ out, float* __restrict__ opacity, float* __restrict__ weights,
                                                                float* __restrict__ trans, int32_t* __restrict__ n_comp) {
	const uint32_t r = blockIdx.x * (VR_BLOCK / 64) + (threadIdx.x >> 6);
	const int32_t lane = (int32_t)(threadIdx.x & 63);
	if (r >= n_rays) return;  // wave-uniform
	int32_t start, count;
	ray_range(ranges, r, n_samples, start, count);
	if (count <= VR_LONG_RAY) return;
	float T = 1.f, op = 0.f, acc[C];
#pragma unroll
	for (int c = 0; c < C; ++c) acc[c] = 0.f;
	int32_t n = 0, base = 0;
	for (; base < count; base += 64) {
		const int32_t i = base + lane, nvalid = min(64, count - base);
		const bool valid = lane < nvalid;
		const size_t s = (size_t)start + (valid ? i : count - 1);
		const float a = valid ? alpha[s] : 0.f;
		float v[C];
#pragma unroll
		for (int c = 0; c < C; ++c) v[c] = values[s * C + c];
		const float incl = wave_incl_prod_f(1.f - a);
		const float Ti = T * dpp_f32<DPP_WAVE_SHR1>(1.f, incl);
		const uint64_t stop = __ballot(valid && Ti < t_stop);
		const int32_t take = stop ? min((int32_t)__builtin_ctzll(stop), nvalid) : nvalid;
		const bool live = lane < take;
		const float w = live ? a * Ti : 0.f;
		if (valid) { weights[s] = w; trans[s] = live ? Ti : 0.f; }
#pragma unroll
		for (int c = 0; c < C; ++c) acc[c] += wave_sum_f(live ? w * v[c] : 0.f);
		op += wave_sum_f(w);
		n += take;
		if (take < nvalid) { base += 64; break; }
		T *= wave_lane_f(incl, 63);
	}
	for (int32_t i = base + lane; i < count; i += 64) { weights[(size_t)start + i] = 0.f; trans[(size_t)start + i] = 0.f; }  // past the stop
	if (lane == 0) {
#pragma unroll
		for (int c = 0; c < C; ++c) out[(size_t)r * C + c] = acc[c];
		opacity[r] = op;
		n_comp[r] = n;
	}
}

// Backward: lane l of a round holds sample hi - 1 - l (the ray walked from its last composited sample down), so the
// reverse recurrence B_{i-1} = alpha_i G_i + (1 - alpha_i) B_i is a forward scan of affine maps over the lanes; B_i of a
// lane is the scan's value one lane earlier (the carry for lane 0). No division by 1 - alpha.
template <int C>
__global__ void __launch_bounds__(VR_BLOCK) k_vr_comp_bwd_wave(uint32_t n_rays, uint32_t n_samples, const float* __restrict__ alpha,
                                                                const float* __restrict__ values, const int32_t* __restrict__ ranges,
                                                                const float* __restrict__ trans, const int32_t* __restrict__ n_comp,
                                                                const float* __restrict__ g_out, const float* __restrict__ g_opacity,
                                                                const float* __restrict__ g_weights, float* __restrict__ g_alpha,
                                                                float* __restrict__ g_values) {
	const uint32_t r = blockIdx.x * (VR_BLOCK / 64) + (threadIdx.x >> 6);
	const int32_t lane = (int32_t)(threadIdx.x & 63);
	if (r >= n_rays) return;  // wave-uniform
	int32_t start, count;
	ray_range(ranges, r, n_samples, start, count);
	if (count <= VR_LONG_RAY) return;
	const int32_t n = min(max(n_comp[r], 0), count);
	float go[C];
#pragma unroll
	for (int c = 0; c < C; ++c) go[c] = g_out[(size_t)r * C + c];
	const float gop = g_opacity[r];
	for (int32_t i = n + lane; i < count; i += 64) {  // from the stop on: no gradient
		const size_t s = (size_t)start + i;
		g_alpha[s] = 0.f;
#pragma unroll
		for (int c = 0; c < C; ++c) g_values[s * C + c] = 0.f;
	}
	float B = 0.f;
	for (int32_t hi = n; hi > 0; hi -= 64) {
		const int32_t i = hi - 1 - lane;
		const bool valid = i >= 0;
		const size_t s = (size_t)start + (valid ? i : 0);
		const float a = valid ? alpha[s] : 0.f, Ti = trans[s];
		float Gi = (g_weights ? g_weights[s] : 0.f) + gop;
#pragma unroll
		for (int c = 0; c < C; ++c) Gi += go[c] * values[s * C + c];
		if (!valid) Gi = 0.f;
		float m = 1.f - a, b = a * Gi;  // a lane without a sample carries the identity map
		wave_incl_affine(m, b);
		const float X = m * B + b;
		const float Bi = dpp_f32<DPP_WAVE_SHR1>(B, X);
		if (valid) {
			g_alpha[s] = Ti * (Gi - Bi);
			const float w = a * Ti;
#pragma unroll
			for (int c = 0; c < C; ++c) g_values[s * C + c] = w * go[c];
		}
		B = wave_lane_f(X, 63);
	}
}

void vr_check(hipError_t e, const char* what) {
	if (e != hipSuccess) throw std::runtime_error(std::string(what) + " failed: " + hipGetErrorString(e));
}
void vr_need(bool ok, const char* msg) { if (!ok) throw std::runtime_error(msg); }

#define VR_DISPATCH_C(C_, CALL)                                                                  \
	switch (C_) {                                                                                \
		case 1: { constexpr int C = 1; CALL; break; } case 2: { constexpr int C = 2; CALL; break; } \
		case 3: { constexpr int C = 3; CALL; break; } case 4: { constexpr int C = 4; CALL; break; } \
		case 5: { constexpr int C = 5; CALL; break; } case 6: { constexpr int C = 6; CALL; break; } \
		case 7: { constexpr int C = 7; CALL; break; } case 8: { constexpr int C = 8; CALL; break; } \
		default: throw std::runtime_error("neus_volrend_composite: n_channels must be 1..8");     \
	}

}  // namespace

void launch_volrend_march_count(hipStream_t s, uint32_t n_rays, const float* rays_o, const float* rays_d, const float* t_min, const float* t_max,
                                const uint8_t* occupancy, uint32_t grid, float dt, uint32_t max_per_ray, int32_t* counts) {
	if (n_rays == 0) return;
	vr_need(rays_o && rays_d && t_min && t_max && occupancy && counts, "neus_volrend_march_count: null pointer");
	vr_need(grid >= 1 && grid <= 512 && (grid & (grid - 1)) == 0, "neus_volrend_march_count: grid must be a power of two from 1 to 512");
	vr_need(dt > 0.f && dt < __builtin_huge_valf(), "neus_volrend_march_count: dt must be positive and finite");
	vr_need(max_per_ray <= 0x7fffffffu, "neus_volrend_march_count: max_per_ray must fit an int32");
	k_vr_march<false><<<(n_rays + 63) / 64, 64, 0, s>>>(n_rays, rays_o, rays_d, t_min, t_max, occupancy, grid, dt, max_per_ray, counts, nullptr, 0, nullptr, nullptr);
	vr_check(hipGetLastError(), "neus_volrend_march_count: launch");
}

void launch_volrend_march_write(hipStream_t s, uint32_t n_rays, const float* rays_o, const float* rays_d, const float* t_min, const float* t_max,
                                const uint8_t* occupancy, uint32_t grid, float dt, uint32_t max_per_ray, const int32_t* ranges, uint32_t n_samples,
                                float* t, int32_t* ray_idx) {
	if (n_rays == 0 || n_samples == 0) return;
	vr_need(rays_o && rays_d && t_min && t_max && occupancy && ranges && t && ray_idx, "neus_volrend_march_write: null pointer");
	vr_need(grid >= 1 && grid <= 512 && (grid & (grid - 1)) == 0, "neus_volrend_march_write: grid must be a power of two from 1 to 512");
	vr_need(dt > 0.f && dt < __builtin_huge_valf(), "neus_volrend_march_write: dt must be positive and finite");
	vr_need(n_samples <= 0x7fffffffu, "neus_volrend_march_write: n_samples must fit an int32");
	k_vr_march<true><<<(n_rays + 63) / 64, 64, 0, s>>>(n_rays, rays_o, rays_d, t_min, t_max, occupancy, grid, dt, max_per_ray, nullptr, ranges, n_samples, t, ray_idx);
	vr_check(hipGetLastError(), "neus_volrend_march_write: launch");
}

void launch_volrend_alpha_forward(hipStream_t s, uint32_t n, const float* sdf, const float* true_cos, const float* dt, float dt_value,
                                  const float* inv_s, float inv_s_value, float cos_anneal_ratio, float* alpha) {
	if (n == 0) return;
	vr_need(sdf && true_cos && alpha, "neus_volrend_alpha_forward: null pointer");
	vr_need(dt || dt_value > 0.f, "neus_volrend_alpha_forward: dt must be positive");
	k_vr_alpha_fwd<<<(n + VR_BLOCK - 1) / VR_BLOCK, VR_BLOCK, 0, s>>>(n, sdf, true_cos, dt, dt_value, inv_s, inv_s_value, cos_anneal_ratio, alpha);
	vr_check(hipGetLastError(), "neus_volrend_alpha_forward: launch");
}

void launch_volrend_alpha_backward(hipStream_t s, uint32_t n, const float* sdf, const float* true_cos, const float* dt, float dt_value,
                                   const float* inv_s, float inv_s_value, float cos_anneal_ratio, const float* g_alpha, float* g_sdf,
                                   float* g_true_cos, double* partials, uint32_t n_partials, float* g_inv_s) {
	vr_need(g_inv_s != nullptr, "neus_volrend_alpha_backward: g_inv_s is null");
	const uint32_t nb = (n + VR_BLOCK - 1) / VR_BLOCK;
	if (n > 0) {
		vr_need(sdf && true_cos && g_alpha && g_sdf && g_true_cos && partials, "neus_volrend_alpha_backward: null pointer");
		vr_need(dt || dt_value > 0.f, "neus_volrend_alpha_backward: dt must be positive");
		vr_need(n_partials >= nb, "neus_volrend_alpha_backward: partials needs ceil(n / 256) doubles");
		k_vr_alpha_bwd<<<nb, VR_BLOCK, 0, s>>>(n, sdf, true_cos, dt, dt_value, inv_s, inv_s_value, cos_anneal_ratio, g_alpha, g_sdf, g_true_cos, partials);
		vr_check(hipGetLastError(), "neus_volrend_alpha_backward: launch");
	}
	k_vr_sum_partials<<<1, VR_BLOCK, 0, s>>>(nb, partials, g_inv_s);
	vr_check(hipGetLastError(), "neus_volrend_alpha_backward: reduction launch");
}

void launch_volrend_composite_forward(hipStream_t s, uint32_t n_rays, uint32_t n_samples, uint32_t n_channels, const float* alpha, const float* values,
                                      const int32_t* ranges, float t_stop, float* out, float* opacity, float* weights, float* trans, int32_t* n_composited) {
	vr_need(n_channels >= 1 && n_channels <= 8, "neus_volrend_composite_forward: n_channels must be 1..8");
	vr_need(n_samples <= 0x7fffffffu, "neus_volrend_composite_forward: n_samples must fit an int32");
	vr_need(t_stop >= 0.f, "neus_volrend_composite_forward: t_stop must not be negative");
	if (n_rays == 0) return;
	vr_need(ranges && out && opacity && n_composited, "neus_volrend_composite_forward: null pointer");
	vr_need(n_samples == 0 || (alpha && values && weights && trans), "neus_volrend_composite_forward: null pointer");
	VR_DISPATCH_C(n_channels, (k_vr_comp_fwd_lane<C><<<(n_rays + 63) / 64, 64, 0, s>>>(n_rays, n_samples, alpha, values, ranges, t_stop, out, opacity, weights, trans, n_composited)));
	vr_check(hipGetLastError(), "neus_volrend_composite_forward: launch");
	if (n_samples > (uint32_t)VR_LONG_RAY) {  // no ray can be long otherwise
		VR_DISPATCH_C(n_channels, (k_vr_comp_fwd_wave<C><<<(n_rays + 3) / 4, VR_BLOCK, 0, s>>>(n_rays, n_samples, alpha, values, ranges, t_stop, out, opacity, weights, trans, n_composited)));
		vr_check(hipGetLastError(), "neus_volrend_composite_forward: long-ray launch");
	}
}

void launch_volrend_composite_backward(hipStream_t s, uint32_t n_rays, uint32_t n_samples, uint32_t n_channels, const float* alpha, const float* values,
                                       const int32_t* ranges, const float* trans, const int32_t* n_composited, const float* g_out,
                                       const float* g_opacity, const float* g_weights, float* g_alpha, float* g_values) {
	vr_need(n_channels >= 1 && n_channels <= 8, "neus_volrend_composite_backward: n_channels must be 1..8");
	vr_need(n_samples <= 0x7fffffffu, "neus_volrend_composite_backward: n_samples must fit an int32");
	if (n_rays == 0 || n_samples == 0) return;
	vr_need(alpha && values && ranges && trans && n_composited && g_out && g_opacity && g_alpha && g_values, "neus_volrend_composite_backward: null pointer");
	VR_DISPATCH_C(n_channels, (k_vr_comp_bwd_lane<C><<<(n_rays + 63) / 64, 64, 0, s>>>(n_rays, n_samples, alpha, values, ranges, trans, n_composited, g_out, g_opacity, g_weights, g_alpha, g_values)));
	vr_check(hipGetLastError(), "neus_volrend_composite_backward: launch");
	if (n_samples > (uint32_t)VR_LONG_RAY) {
		VR_DISPATCH_C(n_channels, (k_vr_comp_bwd_wave<C><<<(n_rays + 3) / 4, VR_BLOCK, 0, s>>>(n_rays, n_samples, alpha, values, ranges, trans, n_composited, g_out, g_opacity, g_weights, g_alpha, g_values)));
		vr_check(hipGetLastError(), "neus_volrend_composite_backward: long-ray launch");
	}
}

}  // namespace neus
