// tcnn's FullyFusedMLP (my_tcnn src/fully_fused_mlp.cu) behind its Identity encoding: the network of tcnn::cpp::
// create_network(n_input_dims, n_output_dims, network) (my_tcnn src/cpp_api.cu:170-172), on v_mfma_f32_32x32x16_f16.
//
// Layout: activations sample-major [n][features] fp16 (the column-major matrices cpp::Module hands its caller), so a
// B fragment (k = feature, column = sample) is one 16-byte load per lane; weights row-major [out][in] fp16 staged in LDS
// per block (transposed when a backward pass multiplies by W^T). One wave computes 32 samples x every output row.
//
// The layer kernel covers every product of the network: the forward (activation applied to the fp16-rounded sum, as
// warp_activation on the half accumulator), the backward deltas and the backward-backward "front"/"back" chains (the
// activation derivative from the stored forward values, warp_activation_backward, common_device.h:174-225), the output
// layer and dL/dinput. Weight gradients dW = D^T X sum over samples with the sample on the MFMA k axis: both operands are
// staged transposed through LDS, per-block fp32 partial rows, summed in a fixed block order by k_mlp_grad_reduce
// (deterministic, where tcnn's split-K fp16 GEMM is not).
//
// A CutlassMLP (my_tcnn src/cutlass_mlp.cu) is the same network at any width up to 512. Matrices of at most 128 x 128 take
// the two kernels above; larger ones take k_ff_layer_wide / k_ff_wgrad_wide below, which tile the output rows over the
// grid and stage the reduction axis in chunks, with the same arithmetic per element. A CutlassMLP also takes the Sine
// activation (cutlass_mlp.cu:102), the one whose derivative the stored post-activation value does not give: its forward keeps
// cos z beside sin z, and both layer kernels have Sine instantiations of their own (ff_sine_epilogue).
#include "kernels.h"
#include <algorithm>
#include <stdexcept>

namespace neus {

namespace {
__device__ __forceinline__ f16v ff_mfma(h8 a, h8 b, f16v c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
// accumulator register i of lane half h holds row (i & 3) + 8 (i >> 2) + 4 h of the 32-row tile (natural k order)
__device__ __forceinline__ constexpr int ff_row(int i, int h) { return (i & 3) + 8 * (i >> 2) + 4 * h; }
constexpr float FF_K_ACT = 10.0f;  // common_device.h:66

// warp_activation (common_device.h:68-113) on an fp16 value
__device__ __forceinline__ float ff_act(uint32_t act, float x) {
	switch (act) {
	case FF_RELU: return x > 0.f ? x : 0.f;
	case FF_EXP: return expf(x);
	case FF_SIGMOID: return 1.0f / (1.0f + expf(-x));
	case FF_SQUAREPLUS: { const float y = x * FF_K_ACT; return 0.5f * (y + sqrtf(y * y + 4)) / FF_K_ACT; }
	case FF_SOFTPLUS: return logf(expf(x * FF_K_ACT) + 1.0f) / FF_K_ACT;
	default: return x;
	}
}
// warp_activation_backward (common_device.h:174-225): the derivative factor from the forward's post-activation value y
__device__ __forceinline__ float ff_dact(uint32_t act, float y) {
	switch (act) {
	case FF_RELU: return y > 0.f ? 1.f : 0.f;
	case FF_EXP: return y;
	case FF_SIGMOID: return (float)(half_t)(y * (float)(half_t)(1.0f - y));  // (T)(y * ((T)1 - y)) in half
	case FF_SQUAREPLUS: { const float t = y * FF_K_ACT; return t * t / (t * t + 1); }
	case FF_SOFTPLUS: return 1.0f - expf(-y * FF_K_ACT);
	default: return 1.f;
	}
}
// the second derivative act''(x), also from the post-activation value y (0 for ReLU and None)
__device__ __forceinline__ float ff_d2act(uint32_t act, float y) {
	switch (act) {
	case FF_EXP: return y;
	case FF_SIGMOID: return y * (1.0f - y) * (1.0f - 2.0f * y);
	case FF_SQUAREPLUS: { const float t = y * FF_K_ACT, q = t * t + 1; return 2.0f * FF_K_ACT * t * t * t / (q * q * q); }
	case FF_SOFTPLUS: { const float p = 1.0f - expf(-y * FF_K_ACT); return FF_K_ACT * p * (1.0f - p); }
	default: return 0.f;
	}
}
// sin and cos of an fp16 value x (exact in fp32, |x| <= 65504) for FF_SINE. With 1 / (2 pi) in two floats and r the whole
// turns, the fraction of a turn is x hi - r from one fma (the exact product minus an integer, rounded once: 2^-25 turns)
// plus x lo, so it is good to about 2^-24 turns at any magnitude the argument can have, where a single fp32 product is off
// by up to 5e-4 turns at 65504 (3e-3 rad, six fp16 ulps of the result). Every multiply-add is written as an fma: a form
// that corrects a rounded product by its error counts the error twice once the compiler contracts the product. v_sin_f32 /
// v_cos_f32 take turns and are good to about 2^-17 absolute, a thirtieth of the fp16 rounding that follows.
__device__ __forceinline__ void ff_sincos(float x, float& sn, float& cs) {
	constexpr float INV_2PI_HI = 0x1.45f306p-3f, INV_2PI_LO = 0x1.b9391p-28f;  // 1 / (2 pi) = hi + lo to 2^-52
	const float r = __builtin_rintf(x * INV_2PI_HI);
	const float f = __builtin_fmaf(x, INV_2PI_LO, __builtin_fmaf(x, INV_2PI_HI, -r));
	sn = __builtin_amdgcn_sinf(f);
	cs = __builtin_amdgcn_cosf(f);
}
// four consecutive fp16 of a row as floats / back (accumulator registers 4j .. 4j + 3 are four consecutive output rows)
__device__ __forceinline__ void ff_load4(const half_t* p, float v[4]) {
	const h4 x = *(const h4*)p;
#pragma unroll
	for (int k = 0; k < 4; ++k) v[k] = (float)x[k];
}
__device__ __forceinline__ void ff_store4(half_t* p, const float v[4]) {
	h4 x;
#pragma unroll
	for (int k = 0; k < 4; ++k) x[k] = (half_t)v[k];
	*(h4*)p = x;
}
}  // namespace

// Out[s][o] = f(sum_k A[o][k] In[s][k]), o < O, k < K (multiple of 16), A = W [O][K] or (trans) W^T with W [K][O].
//   mode FF_MODE_ACT : f = act on the fp16-rounded sum, fp16 out
//   mode FF_MODE_DACT: f = (fp16 sum) * dact(aux[s][o]) rounded to fp16, fp16 out
//   mode FF_MODE_F32 : float out = (float)(fp16 sum), written for o < o_lim only
// With d = dact(aux[s][o]) and c = d2act(aux[s][o]), the exact double backward's epilogues (fp16 out, O a multiple of 4):
//   mode FF_MODE_DACT with out2: out2 = the fp16 sum itself, beside out (the front pass keeps p, the back pass t)
//   mode FF_MODE_CURV    : out = c p[s][o] t[s][o] + d (fp16 sum): the curvature adjoint of a hidden layer in one pass
//   mode FF_MODE_OUT_CURV: out = d (fp16 sum) (skipped when null), out2 = c (fp16 sum) t[s][o]: the output layer's
//                          dL_ddLdoutput and curvature adjoint from the front carried through the last matrix
// One instantiation per mode: the MFMA body is shared, and no epilogue holds another's registers.
//
// FF_SINE (SINE instantiations of modes ACT, DACT and CURV, for both kernels; O a multiple of 4, vector accesses throughout):
// act' = cos z is not a function of the stored sin z, so
//   mode ACT : out = sin(fp16 sum), out2 (when given) = cos(fp16 sum), the pair from one reduction of the argument
//   mode DACT: out = (fp16 sum) auxc[s][o], out2 as above (aux is not read)
//   mode CURV: out = -aux[s][o] p[s][o] t[s][o] + auxc[s][o] (fp16 sum)       (act'' = -sin z = -aux)
// on one sample's 4 row tiles from row o_blk on. The other activations' instantiations do not contain any of this.
template <uint32_t MODE>
__device__ __forceinline__ void ff_sine_epilogue(const FfLayer& L, const f16v (&acc)[4], uint32_t s, uint32_t o_blk, uint32_t MT, int h) {
	static_assert(MODE == FF_MODE_ACT || MODE == FF_MODE_DACT || MODE == FF_MODE_CURV, "Sine is a hidden activation");
#pragma unroll
	for (int mt = 0; mt < 4; ++mt) {
		if ((uint32_t)mt >= MT) break;
#pragma unroll
		for (int j = 0; j < 4; ++j) {
			const uint32_t o0 = o_blk + 32 * mt + ff_row(4 * j, h);
			if (o0 >= L.O) continue;
			const size_t at = (size_t)s * L.ldo + o0;
			float x[4], r0[4], r1[4], c[4], y[4], pv[4], tv[4];
			if constexpr (MODE != FF_MODE_ACT) ff_load4(L.auxc + (size_t)s * L.ldx + o0, c);
			if constexpr (MODE == FF_MODE_CURV) {
				ff_load4(L.aux + (size_t)s * L.ldx + o0, y);
				ff_load4(L.p + at, pv);
				ff_load4(L.t + at, tv);
			}
#pragma unroll
			for (int k = 0; k < 4; ++k) {
				x[k] = (float)(half_t)acc[mt][4 * j + k];
				if constexpr (MODE == FF_MODE_ACT) {
					ff_sincos(x[k], r0[k], r1[k]);
				} else {
					r0[k] = x[k] * c[k];
					if constexpr (MODE == FF_MODE_CURV) r0[k] = -y[k] * pv[k] * tv[k] + r0[k];
					r1[k] = x[k];
				}
			}
			ff_store4(L.out + at, r0);
			if constexpr (MODE != FF_MODE_CURV) if (L.out2) ff_store4(L.out2 + at, r1);
		}
	}
}

template <uint32_t MODE, bool SINE = false> __global__ void __launch_bounds__(256) k_ff_layer(FfLayer L) {
	extern __shared__ half_t s_w[];
	const uint32_t Op = (L.O + 31) / 32 * 32, lda = L.K + 8;
	// stage A [Op][K] (+ 8 halves of row padding); rows >= O are zero
	for (uint32_t e = threadIdx.x; e < Op * L.K; e += blockDim.x) {
		const uint32_t o = e / L.K, k = e % L.K;
		half_t v = (half_t)0.f;
		if (o < L.O) v = L.trans ? L.W[(size_t)k * L.O + o] : L.W[(size_t)o * L.K + k];
		s_w[o * lda + k] = v;
	}
	__syncthreads();
	const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
	const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
	const uint32_t MT = Op / 32, KS = L.in ? L.K / 16 : 0;
	for (uint32_t s0 = wave * 32; s0 < L.n; s0 += n_waves * 32) {
		const uint32_t s = s0 + r;
		const bool valid = s < L.n;
		f16v acc[4];
#pragma unroll
		for (int mt = 0; mt < 4; ++mt)
#pragma unroll
			for (int i = 0; i < 16; ++i) acc[mt][i] = 0.f;
		for (uint32_t ks = 0; ks < KS; ++ks) {
			h8 b = (h8){0, 0, 0, 0, 0, 0, 0, 0};
			if (valid) b = *(const h8*)(L.in + (size_t)s * L.ldi + 16 * ks + 8 * h);
#pragma unroll
			for (int mt = 0; mt < 4; ++mt) {
				if ((uint32_t)mt >= MT) break;
				const h8 a = *(const h8*)(s_w + (32 * mt + r) * lda + 16 * ks + 8 * h);
				acc[mt] = ff_mfma(a, b, acc[mt]);
			}
		}
		if (!valid) continue;
		if constexpr (SINE) {
			ff_sine_epilogue<MODE>(L, acc, s, 0, MT, h);
		} else if constexpr (MODE != FF_MODE_ACT && MODE != FF_MODE_F32) {
			// O is a multiple of 4 here (launch_ff_layer): registers 4j .. 4j + 3 are rows o0 .. o0 + 3, so every operand of the
			// epilogue is one 8-byte load and every result one 8-byte store per lane
#pragma unroll
			for (int mt = 0; mt < 4; ++mt) {
				if ((uint32_t)mt >= MT) break;
#pragma unroll
				for (int j = 0; j < 4; ++j) {
					const uint32_t o0 = 32 * mt + ff_row(4 * j, h);
					if (o0 >= L.O) continue;
					const size_t at = (size_t)s * L.ldo + o0;
					float x[4], y[4], r0[4], r1[4], pv[4], tv[4];
					ff_load4(L.aux + (size_t)s * L.ldx + o0, y);
					if constexpr (MODE == FF_MODE_CURV) ff_load4(L.p + at, pv);
					if constexpr (MODE != FF_MODE_DACT) ff_load4(L.t + at, tv);
#pragma unroll
					for (int k = 0; k < 4; ++k) {
						x[k] = (float)(half_t)acc[mt][4 * j + k];
						const float d = (float)(half_t)ff_dact(L.act, y[k]);
						r0[k] = x[k] * d;
						if constexpr (MODE == FF_MODE_CURV) r0[k] = ff_d2act(L.act, y[k]) * pv[k] * tv[k] + r0[k];
						if constexpr (MODE == FF_MODE_OUT_CURV) r1[k] = ff_d2act(L.act, y[k]) * x[k] * tv[k];
						else r1[k] = x[k];
					}
					if (L.out) ff_store4(L.out + at, r0);
					if (L.out2) ff_store4(L.out2 + at, r1);
				}
			}
		} else {
#pragma unroll
			for (int mt = 0; mt < 4; ++mt) {
				if ((uint32_t)mt >= MT) break;
#pragma unroll
				for (int i = 0; i < 16; ++i) {
					const uint32_t o = 32 * mt + ff_row(i, h);
					if (o >= L.O) continue;
					const float x = (float)(half_t)acc[mt][i];
					if constexpr (MODE == FF_MODE_F32) {
						if (o < L.o_lim) L.out_f[(size_t)s * L.ldo + o] = x * L.out_scale;
					} else {
						L.out[(size_t)s * L.ldo + o] = (half_t)ff_act(L.act, x);
					}
				}
			}
		}
	}
}

// dW[o][i] (partial over this block's samples) = sum_s D[s][o] X[s][i] (+ D2[s][o] X2[s][i], chunk by chunk after the first
// product: the exact double backward's curvature term) -> prow[block][off + o I + i] (fp32)
__global__ void __launch_bounds__(256) k_ff_wgrad(FfWgrad G) {
	extern __shared__ half_t s_t[];
	const uint32_t Op = (G.O + 31) / 32 * 32, Ip = (G.I + 31) / 32 * 32;
	half_t* Dt = s_t;                 // [Op][40]: the chunk's deltas, sample on the row
	half_t* Xt = s_t + Op * 40;       // [Ip][40]
	const uint32_t per = (G.n + gridDim.x - 1) / gridDim.x;
	const uint32_t b0 = blockIdx.x * per, b1 = min(G.n, b0 + per);
	const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5, wv = threadIdx.x >> 6;
	const uint32_t TO = Op / 32, TI = Ip / 32, NT = TO * TI;
	f16v acc[4];
#pragma unroll
	for (int t = 0; t < 4; ++t)
#pragma unroll
		for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;
	const uint32_t n_prod = G.D2 ? 2 : 1;  // the chunk's second product follows its first into the same accumulators
	for (uint32_t c0 = b0; c0 < b1; c0 += 32)
	for (uint32_t pr = 0; pr < n_prod; ++pr) {
		const half_t* D = pr ? G.D2 : G.D;
		const half_t* X = pr ? G.X2 : G.X;
		__syncthreads();
		for (uint32_t e = threadIdx.x; e < 32 * Op; e += blockDim.x) {
			const uint32_t k = e / Op, o = e % Op, s = c0 + k;
			Dt[o * 40 + k] = (s < b1 && o < G.O) ? D[(size_t)s * G.ldd + o] : (half_t)0.f;
		}
		for (uint32_t e = threadIdx.x; e < 32 * Ip; e += blockDim.x) {
			const uint32_t k = e / Ip, i = e % Ip, s = c0 + k;
			Xt[i * 40 + k] = (s < b1 && i < G.I) ? X[(size_t)s * G.ldx + i] : (half_t)0.f;
		}
		__syncthreads();
#pragma unroll
		for (int t = 0; t < 4; ++t) {
			const uint32_t tile = (uint32_t)wv + 4 * (uint32_t)t;
			if (tile >= NT) break;
			const uint32_t to = tile / TI, ti = tile % TI;
#pragma unroll
			for (int ks = 0; ks < 2; ++ks) {
				const h8 a = *(const h8*)(Dt + (32 * to + r) * 40 + 16 * ks + 8 * h);
				const h8 b = *(const h8*)(Xt + (32 * ti + r) * 40 + 16 * ks + 8 * h);
				acc[t] = ff_mfma(a, b, acc[t]);
			}
		}
	}
	float* prow = G.partial + (size_t)blockIdx.x * G.ld_partial + G.off;
#pragma unroll
	for (int t = 0; t < 4; ++t) {
		const uint32_t tile = (uint32_t)wv + 4 * (uint32_t)t;
		if (tile >= NT) break;
		const uint32_t to = tile / TI, ti = tile % TI;
#pragma unroll
		for (int i = 0; i < 16; ++i) {
			const uint32_t o = 32 * to + ff_row(i, h), c = 32 * ti + r;
			if (o < G.O && c < G.I) prow[(size_t)o * G.I + c] = acc[t][i];
		}
	}
}

// ---------------------------------------------------------------- wide matrices (CutlassMLP widths above 128)
// The same products for O or K (wgrad: O or I) above 128, where neither the whole matrix nor a whole partial row fits a
// block. Output rows are tiled over the grid and the reduction axis is staged through LDS in chunks of 64.
namespace {
constexpr uint32_t FF_WIDE_LAYER_BLOCKS = 512;  // sample blocks of k_ff_layer_wide's grid (x): beyond 2^17 samples a block takes a second trip
constexpr uint32_t FF_WIDE_SLICES = 32;         // sample slices (= partial rows) of k_ff_wgrad_wide at most
constexpr uint32_t FFW_OT = 128;           // output rows (wgrad: rows and columns) of a block
constexpr uint32_t FFW_KC = 64;            // reduction elements staged at a time
constexpr uint32_t FFW_RS = FFW_KC + 8;    // row stride of a [row][k] image: 16-byte reads, as k_ff_layer's s_w
// row stride of a [k][row] image: 320 B = 16 dwords mod 64, so the four k rows x 64 B that a half-wave reads through one
// transposing read land on distinct banks
constexpr uint32_t FFW_TS = FFW_OT + 32;
constexpr uint32_t FFW_IMG = FFW_KC * FFW_TS;  // halves of one image (>= FFW_OT * FFW_RS)
static_assert(FFW_IMG >= FFW_OT * FFW_RS, "one LDS image serves both layouts");
typedef __fp16 ff_trh4 __attribute__((__vector_size__(4 * sizeof(__fp16))));

// The MFMA operand of lane (r, h): img[k0 + 8 h .. + 7][c0 + r] of a [k][row] image, through ds_read_b64_tr_b16. Each
// group of 16 lanes reads 4 k rows x 16 columns and gets them column-major: lane 4 q + p of the group points at k row q,
// columns 4 p .. 4 p + 3, and lane i receives column i with k row q in element q. Groups 0 / 1 are columns 0-15 / 16-31
// of h = 0, groups 2 / 3 those of h = 1. Every lane of the wave must be active.
__device__ __forceinline__ h8 ff_frag_tr(const half_t* img, uint32_t k0, uint32_t c0, int lane) {
	const int li = lane & 15, g = lane >> 4;
	const half_t* p = img + (k0 + 8 * (g >> 1) + (li >> 2)) * FFW_TS + c0 + 16 * (g & 1) + 4 * (li & 3);
	typedef __attribute__((address_space(3))) ff_trh4* lds_ptr;
	const h4 lo = __builtin_bit_cast(h4, __builtin_amdgcn_ds_read_tr16_b64_v4f16((lds_ptr)p));
	const h4 hi = __builtin_bit_cast(h4, __builtin_amdgcn_ds_read_tr16_b64_v4f16((lds_ptr)(p + 4 * FFW_TS)));
	return (h8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}
// Staging goes through registers, 4 x 16 bytes per thread of a 256-thread block, so that the next chunk's global loads are
// in flight while the MFMAs read the current one from LDS.
// rows [r0, r0 + FFW_KC) x columns [c0, c0 + FFW_OT) of the row-major src [.][ld], to become a [k][row] image; rows >= r1
// and columns >= c1 (a multiple of 8) are zero
__device__ __forceinline__ void ff_get_rows(h8 (&v)[4], const half_t* __restrict__ src, uint32_t ld, uint32_t r0, uint32_t r1, uint32_t c0, uint32_t c1) {
#pragma unroll
	for (int q = 0; q < 4; ++q) {
		const uint32_t e = threadIdx.x + 256 * q, k = e / (FFW_OT / 8), c = c0 + 8 * (e % (FFW_OT / 8));
		v[q] = (h8){0, 0, 0, 0, 0, 0, 0, 0};
		if (r0 + k < r1 && c < c1) v[q] = *(const h8*)(src + (size_t)(r0 + k) * ld + c);
	}
}
__device__ __forceinline__ void ff_put_rows(half_t* img, const h8 (&v)[4]) {
#pragma unroll
	for (int q = 0; q < 4; ++q) {
		const uint32_t e = threadIdx.x + 256 * q;
		*(h8*)(img + e / (FFW_OT / 8) * FFW_TS + 8 * (e % (FFW_OT / 8))) = v[q];
	}
}
// rows [r0, r0 + FFW_OT) x columns [c0, c0 + FFW_KC) of the row-major src [.][ld], to become a [row][k] image; rows >= r1
// and columns >= c1 (a multiple of 8) are zero
__device__ __forceinline__ void ff_get_cols(h8 (&v)[4], const half_t* __restrict__ src, uint32_t ld, uint32_t r0, uint32_t r1, uint32_t c0, uint32_t c1) {
#pragma unroll
	for (int q = 0; q < 4; ++q) {
		const uint32_t e = threadIdx.x + 256 * q, o = e / (FFW_KC / 8), c = c0 + 8 * (e % (FFW_KC / 8));
		v[q] = (h8){0, 0, 0, 0, 0, 0, 0, 0};
		if (r0 + o < r1 && c < c1) v[q] = *(const h8*)(src + (size_t)(r0 + o) * ld + c);
	}
}
__device__ __forceinline__ void ff_put_cols(half_t* img, const h8 (&v)[4]) {
#pragma unroll
	for (int q = 0; q < 4; ++q) {
		const uint32_t e = threadIdx.x + 256 * q;
		*(h8*)(img + e / (FFW_KC / 8) * FFW_RS + 8 * (e % (FFW_KC / 8))) = v[q];
	}
}
}  // namespace

// k_ff_layer's epilogues on one sample's 4 row tiles from row o_blk on (the same arithmetic, statement for statement)
template <uint32_t MODE>
__device__ __forceinline__ void ff_wide_epilogue(const FfLayer& L, const f16v (&acc)[4], uint32_t s, uint32_t o_blk, uint32_t MT, int h) {
	if constexpr (MODE != FF_MODE_ACT && MODE != FF_MODE_F32) {
		// as k_ff_layer: O is a multiple of 4, registers 4j .. 4j + 3 are four consecutive rows
#pragma unroll
		for (int mt = 0; mt < 4; ++mt) {
			if ((uint32_t)mt >= MT) break;
#pragma unroll
			for (int j = 0; j < 4; ++j) {
				const uint32_t o0 = o_blk + 32 * mt + ff_row(4 * j, h);
				if (o0 >= L.O) continue;
				const size_t at = (size_t)s * L.ldo + o0;
				float x[4], y[4], r0[4], r1[4], pv[4], tv[4];
				ff_load4(L.aux + (size_t)s * L.ldx + o0, y);
				if constexpr (MODE == FF_MODE_CURV) ff_load4(L.p + at, pv);
				if constexpr (MODE != FF_MODE_DACT) ff_load4(L.t + at, tv);
#pragma unroll
				for (int k = 0; k < 4; ++k) {
					x[k] = (float)(half_t)acc[mt][4 * j + k];
					const float d = (float)(half_t)ff_dact(L.act, y[k]);
					r0[k] = x[k] * d;
					if constexpr (MODE == FF_MODE_CURV) r0[k] = ff_d2act(L.act, y[k]) * pv[k] * tv[k] + r0[k];
					if constexpr (MODE == FF_MODE_OUT_CURV) r1[k] = ff_d2act(L.act, y[k]) * x[k] * tv[k];
					else r1[k] = x[k];
				}
				if (L.out) ff_store4(L.out + at, r0);
				if (L.out2) ff_store4(L.out2 + at, r1);
			}
		}
	} else {
#pragma unroll
		for (int mt = 0; mt < 4; ++mt) {
			if ((uint32_t)mt >= MT) break;
#pragma unroll
			for (int i = 0; i < 16; ++i) {
				const uint32_t o = o_blk + 32 * mt + ff_row(i, h);
				if (o >= L.O) continue;
				const float x = (float)(half_t)acc[mt][i];
				if constexpr (MODE == FF_MODE_F32) {
					if (o < L.o_lim) L.out_f[(size_t)s * L.ldo + o] = x * L.out_scale;
				} else {
					L.out[(size_t)s * L.ldo + o] = (half_t)ff_act(L.act, x);
				}
			}
		}
	}
}

// k_ff_layer's product and epilogues (the same arithmetic: fp32 accumulation over all of K, one rounding to fp16, the
// epilogue on that value) for one 128-row tile of the output (blockIdx.y) and 256 samples at a time: each wave holds
// 64 samples x 4 row tiles. The matrix tile comes through LDS 64 k at a time: W [O][K] as a [row][k] image read 16 bytes
// per lane; W^T of W [K][O] (TRANS) as the [k][row] image of its rows as they lie in memory, read transposed. A wave's
// input fragments of a chunk are loaded before the chunk is staged, and the matrix tile of the next chunk into registers
// while the MFMAs run on the current one.
template <uint32_t MODE, bool TRANS, bool SINE = false> __global__ void __launch_bounds__(256) k_ff_layer_wide(FfLayer L) {
	__shared__ __attribute__((aligned(16))) half_t s_a[FFW_IMG];
	const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5, wv = threadIdx.x >> 6;
	const uint32_t o_blk = blockIdx.y * FFW_OT;
	const uint32_t MT = min(4u, (L.O - o_blk + 31) / 32), K = L.in ? L.K : 0;
	for (uint32_t g0 = blockIdx.x * 256; g0 < L.n; g0 += gridDim.x * 256) {
		const uint32_t sb = g0 + 64 * wv;
		f16v acc[2][4];
#pragma unroll
		for (int g = 0; g < 2; ++g)
#pragma unroll
			for (int mt = 0; mt < 4; ++mt)
#pragma unroll
				for (int i = 0; i < 16; ++i) acc[g][mt][i] = 0.f;
		// this thread's part of the matrix tile of chunk k0
		const auto load_tile = [&](uint32_t k0, h8 (&va)[4]) {
			const uint32_t k1 = min(K, k0 + FFW_KC);
			if constexpr (TRANS) ff_get_rows(va, L.W, L.O, k0, k1, o_blk, L.O);
			else ff_get_cols(va, L.W, L.K, o_blk, L.O, k0, k1);
		};
		h8 va[4];
		if (K) load_tile(0, va);
		for (uint32_t k0 = 0; k0 < K; k0 += FFW_KC) {
			const uint32_t kc = min(FFW_KC, K - k0);
			h8 b[2][4];  // this wave's input fragments: zero past the chunk's end and for rows >= n
#pragma unroll
			for (int g = 0; g < 2; ++g)
#pragma unroll
				for (int ks = 0; ks < 4; ++ks) {
					const uint32_t s = sb + 32 * g + r;
					b[g][ks] = (h8){0, 0, 0, 0, 0, 0, 0, 0};
					if (s < L.n && 16u * ks < kc) b[g][ks] = *(const h8*)(L.in + (size_t)s * L.ldi + k0 + 16 * ks + 8 * h);
				}
			__syncthreads();  // the chunk before has been read
			if constexpr (TRANS) ff_put_rows(s_a, va);
			else ff_put_cols(s_a, va);
			__syncthreads();
			if (k0 + FFW_KC < K) load_tile(k0 + FFW_KC, va);  // in flight over this chunk's MFMAs
#pragma unroll
			for (int ks = 0; ks < 4; ++ks) {
				if (16u * ks >= kc) break;
#pragma unroll
				for (int mt = 0; mt < 4; ++mt) {
					if ((uint32_t)mt >= MT) break;
					h8 a;
					if constexpr (TRANS) a = ff_frag_tr(s_a, 16 * ks, 32 * mt, lane);
					else a = *(const h8*)(s_a + (32 * mt + r) * FFW_RS + 16 * ks + 8 * h);
					acc[0][mt] = ff_mfma(a, b[0][ks], acc[0][mt]);
					acc[1][mt] = ff_mfma(a, b[1][ks], acc[1][mt]);
				}
			}
		}
		if constexpr (SINE) {
			if (sb + r < L.n) ff_sine_epilogue<MODE>(L, acc[0], sb + r, o_blk, MT, h);
			if (sb + 32 + r < L.n) ff_sine_epilogue<MODE>(L, acc[1], sb + 32 + r, o_blk, MT, h);
		} else {
			if (sb + r < L.n) ff_wide_epilogue<MODE>(L, acc[0], sb + r, o_blk, MT, h);
			if (sb + 32 + r < L.n) ff_wide_epilogue<MODE>(L, acc[1], sb + 32 + r, o_blk, MT, h);
		}
	}
}

// k_ff_wgrad's sums for one 128 x 128 tile of dW (blockIdx.x) over one slice of `per` samples (blockIdx.y) ->
// prow[slice][off + o I + i]. The deltas and the layer inputs of 64 samples are staged as they lie in memory ([sample][row]
// images, the sample being the MFMA k axis) and both operands are read transposed; the next 64 samples are loaded into
// registers meanwhile. Each wave owns 64 x 64 of the tile and skips the 32 x 32 parts that lie outside the matrix.
__global__ void __launch_bounds__(256) k_ff_wgrad_wide(FfWgrad G, uint32_t per) {
	__shared__ __attribute__((aligned(16))) half_t s_d[FFW_IMG], s_x[FFW_IMG];
	const uint32_t TI = (G.I + FFW_OT - 1) / FFW_OT;
	const uint32_t o_blk = blockIdx.x / TI * FFW_OT, i_blk = blockIdx.x % TI * FFW_OT;
	const uint32_t b0 = blockIdx.y * per, b1 = min(G.n, b0 + per);
	const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5, wv = threadIdx.x >> 6;
	const uint32_t wo = 64 * (wv >> 1), wi = 64 * (wv & 1);
	bool on[2][2];
#pragma unroll
	for (int a = 0; a < 2; ++a)
#pragma unroll
		for (int b = 0; b < 2; ++b) on[a][b] = o_blk + wo + 32 * a < G.O && i_blk + wi + 32 * b < G.I;
	f16v acc[2][2];
#pragma unroll
	for (int a = 0; a < 2; ++a)
#pragma unroll
		for (int b = 0; b < 2; ++b)
#pragma unroll
			for (int i = 0; i < 16; ++i) acc[a][b][i] = 0.f;
	const uint32_t n_prod = G.D2 ? 2 : 1;  // the chunk's second product follows its first into the same accumulators
	const uint32_t n_it = b0 < b1 ? (b1 - b0 + FFW_KC - 1) / FFW_KC * n_prod : 0;
	const auto load_chunk = [&](uint32_t it, h8 (&vd)[4], h8 (&vx)[4]) {
		const uint32_t c0 = b0 + it / n_prod * FFW_KC, pr = it % n_prod;
		ff_get_rows(vd, pr ? G.D2 : G.D, G.ldd, c0, b1, o_blk, G.O);
		ff_get_rows(vx, pr ? G.X2 : G.X, G.ldx, c0, b1, i_blk, G.I);
	};
	h8 vd[4], vx[4];
	if (n_it) load_chunk(0, vd, vx);
	for (uint32_t it = 0; it < n_it; ++it) {
		const uint32_t c0 = b0 + it / n_prod * FFW_KC;
		__syncthreads();
		ff_put_rows(s_d, vd);
		ff_put_rows(s_x, vx);
		__syncthreads();
		if (it + 1 < n_it) load_chunk(it + 1, vd, vx);  // in flight over this chunk's MFMAs
#pragma unroll
		for (int ks = 0; ks < 4; ++ks) {
			if (c0 + 16 * ks >= b1) break;
			h8 fa[2], fb[2];
#pragma unroll
			for (int a = 0; a < 2; ++a) fa[a] = ff_frag_tr(s_d, 16 * ks, wo + 32 * a, lane);
#pragma unroll
			for (int b = 0; b < 2; ++b) fb[b] = ff_frag_tr(s_x, 16 * ks, wi + 32 * b, lane);
#pragma unroll
			for (int a = 0; a < 2; ++a)
#pragma unroll
				for (int b = 0; b < 2; ++b)
					if (on[a][b]) acc[a][b] = ff_mfma(fa[a], fb[b], acc[a][b]);
		}
	}
	float* prow = G.partial + (size_t)blockIdx.y * G.ld_partial + G.off;
#pragma unroll
	for (int a = 0; a < 2; ++a)
#pragma unroll
		for (int b = 0; b < 2; ++b)
#pragma unroll
			for (int i = 0; i < 16; ++i) {
				const uint32_t o = o_blk + wo + 32 * a + ff_row(i, h), c = i_blk + wi + 32 * b + r;
				if (o < G.O && c < G.I) prow[(size_t)o * G.I + c] = acc[a][b][i];
			}
}

// Identity encoding (identity.h:44-70): X0[s][k] =(half)(in[s][k] scale + offset) for k < n_in, 1 for the padding
// k < ld (the bias input of tcnn's padded encodings); mode 1: the backward-backward front, dL_ddLdinput scaled, padding 0
__global__ void k_ff_input(uint32_t n, uint32_t n_in, uint32_t ld, const float* __restrict__ in, float scale, float offset, half_t* __restrict__ x,
                           uint32_t grad) {
	for (uint64_t e = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; e < (uint64_t)n * ld; e += (uint64_t)gridDim.x * blockDim.x) {
		const uint64_t s = e / ld;
		const uint32_t k = (uint32_t)(e % ld);
		float v = grad ? 0.f : 1.f;
		if (k < n_in) v = grad ? in[s * n_in + k] * scale : in[s * n_in + k] * scale + offset;
		x[e] = (half_t)v;
	}
}
// the output activation's backward on dL/doutput (fully_fused_mlp.cu:985-1000): D[s][o] = dL[s][o] dact(out[s][o])
__global__ void k_ff_out_delta(uint32_t n, uint32_t ld, uint32_t act, const half_t* __restrict__ dL, const half_t* __restrict__ out, half_t* __restrict__ d) {
	for (uint64_t e = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; e < (uint64_t)n * ld; e += (uint64_t)gridDim.x * blockDim.x) {
		const float g = (float)dL[e];
		d[e] = act == FF_NONE ? dL[e] : (half_t)(g * (float)(half_t)ff_dact(act, (float)out[e]));
	}
}

static uint32_t ff_blocks(uint64_t n, uint32_t per, uint32_t cap) { return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n + per - 1) / per, cap)); }

// a product takes k_ff_layer / k_ff_wgrad where its whole matrix fits them, and the wide kernels otherwise
static bool ff_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
template <uint32_t MODE, bool SINE = false> static void ff_launch_wide(hipStream_t s, const FfLayer& L) {
	const dim3 grid(ff_blocks(L.n, 256, FF_WIDE_LAYER_BLOCKS), (L.O + FFW_OT - 1) / FFW_OT);
	if (L.trans) k_ff_layer_wide<MODE, true, SINE><<<grid, 256, 0, s>>>(L);
	else k_ff_layer_wide<MODE, false, SINE><<<grid, 256, 0, s>>>(L);
}
template <uint32_t MODE> static void ff_launch_sine(hipStream_t s, const FfLayer& L, bool wide, uint32_t blocks, size_t smem) {
	if (wide) ff_launch_wide<MODE, true>(s, L);
	else k_ff_layer<MODE, true><<<blocks, 256, smem, s>>>(L);
}
void launch_ff_layer(hipStream_t s, const FfLayer& L) {
	if (L.K % 16 || L.K == 0 || L.O == 0 || L.O > 512 || L.K > 512) throw std::runtime_error("ff layer: K must be a multiple of 16, 1 <= O, K <= 512");
	const bool wide = L.O > 128 || L.K > 128;
	if (wide && (L.O % 8 || L.ldi % 8 || !ff_al16(L.W) || !ff_al16(L.in)))
		throw std::runtime_error("ff layer: a matrix above 128 rows or columns needs O and the input stride multiples of 8 and 16-byte aligned tensors");
	if (L.mode > FF_MODE_OUT_CURV || (!L.in && L.mode != FF_MODE_CURV)) throw std::runtime_error("ff layer: unknown mode / null input");
	const auto al8 = [](const void* p) { return ((uintptr_t)p & 7) == 0; };
	if (L.mode != FF_MODE_ACT && L.mode != FF_MODE_F32) {  // the vector epilogue: whole groups of four rows, 8-byte aligned rows
		if (L.O % 4 || L.ldo % 4 || L.ldx % 4 || !L.aux || !al8(L.aux) || !al8(L.out) || !al8(L.out2) || !al8(L.p) || !al8(L.t))
			throw std::runtime_error("ff layer: the derivative epilogues need O and the row strides multiples of 4 and 8-byte aligned tensors");
		if ((L.mode == FF_MODE_DACT && !L.out) || (L.mode == FF_MODE_CURV && (!L.out || !L.p || !L.t)) || (L.mode == FF_MODE_OUT_CURV && (!L.out2 || !L.t)))
			throw std::runtime_error("ff layer: a tensor of the epilogue is null");
	}
	const size_t smem = (size_t)((L.O + 31) / 32 * 32) * (L.K + 8) * sizeof(half_t);
	const uint32_t blocks = ff_blocks(L.n, 128, 1024);
	if (L.act == FF_SINE) {  // its own instantiations: a hidden activation, so the modes that hidden layers run
		const bool dv = L.mode != FF_MODE_ACT;
		if (L.mode != FF_MODE_ACT && L.mode != FF_MODE_DACT && L.mode != FF_MODE_CURV) throw std::runtime_error("ff layer: Sine is a hidden activation (modes ACT, DACT, CURV)");
		if (L.O % 4 || L.ldo % 4 || !L.out || !al8(L.out) || !al8(L.out2) || (dv && (!L.auxc || !al8(L.auxc))))
			throw std::runtime_error("ff layer: Sine needs O and the row stride multiples of 4, 8-byte aligned tensors and, for its derivative, the forward's cos values");
		switch (L.mode) {
		case FF_MODE_ACT: ff_launch_sine<FF_MODE_ACT>(s, L, wide, blocks, smem); break;
		case FF_MODE_DACT: ff_launch_sine<FF_MODE_DACT>(s, L, wide, blocks, smem); break;
		default: ff_launch_sine<FF_MODE_CURV>(s, L, wide, blocks, smem); break;
		}
		return;
	}
	if (wide) {
		switch (L.mode) {
		case FF_MODE_ACT: ff_launch_wide<FF_MODE_ACT>(s, L); break;
		case FF_MODE_DACT: ff_launch_wide<FF_MODE_DACT>(s, L); break;
		case FF_MODE_F32: ff_launch_wide<FF_MODE_F32>(s, L); break;
		case FF_MODE_CURV: ff_launch_wide<FF_MODE_CURV>(s, L); break;
		default: ff_launch_wide<FF_MODE_OUT_CURV>(s, L); break;
		}
		return;
	}
	switch (L.mode) {
	case FF_MODE_ACT: k_ff_layer<FF_MODE_ACT><<<blocks, 256, smem, s>>>(L); break;
	case FF_MODE_DACT: k_ff_layer<FF_MODE_DACT><<<blocks, 256, smem, s>>>(L); break;
	case FF_MODE_F32: k_ff_layer<FF_MODE_F32><<<blocks, 256, smem, s>>>(L); break;
	case FF_MODE_CURV: k_ff_layer<FF_MODE_CURV><<<blocks, 256, smem, s>>>(L); break;
	default: k_ff_layer<FF_MODE_OUT_CURV><<<blocks, 256, smem, s>>>(L); break;
	}
}
// wide: at most FF_WIDE_SLICES sample slices of at least 256 samples, so a wide network's partial rows do not grow with n
uint32_t ff_wgrad_blocks(uint32_t n, bool wide) { return wide ? ff_blocks(n, 256, FF_WIDE_SLICES) : ff_blocks(n, 1024, 512); }
void launch_ff_wgrad(hipStream_t s, const FfWgrad& G) {
	if (G.O == 0 || G.I == 0 || G.O > 512 || G.I > 512) throw std::runtime_error("ff wgrad: 1..512 rows and columns");
	if (!G.D2 != !G.X2) throw std::runtime_error("ff wgrad: the second product needs both of its factors");
	if (G.O > 128 || G.I > 128) {
		if (G.O % 8 || G.I % 8 || G.ldd % 8 || G.ldx % 8 || !ff_al16(G.D) || !ff_al16(G.X) || !ff_al16(G.D2) || !ff_al16(G.X2))
			throw std::runtime_error("ff wgrad: a matrix above 128 rows or columns needs its sizes and strides multiples of 8 and 16-byte aligned tensors");
		const uint32_t slices = ff_wgrad_blocks(G.n, true);
		const dim3 grid(((G.O + FFW_OT - 1) / FFW_OT) * ((G.I + FFW_OT - 1) / FFW_OT), slices);
		k_ff_wgrad_wide<<<grid, 256, 0, s>>>(G, (G.n + slices - 1) / slices);
		return;
	}
	const size_t smem = (size_t)((G.O + 31) / 32 * 32 + (G.I + 31) / 32 * 32) * 40 * sizeof(half_t);
	k_ff_wgrad<<<ff_wgrad_blocks(G.n), 256, smem, s>>>(G);
}
void launch_ff_input(hipStream_t s, uint32_t n, uint32_t n_in, uint32_t ld, const float* in, float scale, float offset, half_t* x, bool grad) {
	k_ff_input<<<ff_blocks((uint64_t)n * ld, 256, 4096), 256, 0, s>>>(n, n_in, ld, in, scale, offset, x, grad ? 1u : 0u);
}
void launch_ff_out_delta(hipStream_t s, uint32_t n, uint32_t ld, uint32_t act, const half_t* dL, const half_t* out, half_t* d) {
	k_ff_out_delta<<<ff_blocks((uint64_t)n * ld, 256, 4096), 256, 0, s>>>(n, ld, act, dL, out, d);
}

}  // namespace neus
