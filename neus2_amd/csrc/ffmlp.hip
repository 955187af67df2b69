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
template <uint32_t MODE> __global__ void __launch_bounds__(256) k_ff_layer(FfLayer L) {
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
		if constexpr (MODE != FF_MODE_ACT && MODE != FF_MODE_F32) {
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

// Identity encoding (identity.h:44-70): X0[s][k] = (half)(in[s][k] scale + offset) for k < n_in, 1 for the padding
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

void launch_ff_layer(hipStream_t s, const FfLayer& L) {
	if (L.K % 16 || L.K == 0 || L.O == 0 || L.O > 128) throw std::runtime_error("ff layer: K must be a multiple of 16, 1 <= O <= 128");
	if (L.mode > FF_MODE_OUT_CURV || (!L.in && L.mode != FF_MODE_CURV)) throw std::runtime_error("ff layer: unknown mode / null input");
	if (L.mode != FF_MODE_ACT && L.mode != FF_MODE_F32) {  // the vector epilogue: whole groups of four rows, 8-byte aligned rows
		const auto al8 = [](const void* p) { return ((uintptr_t)p & 7) == 0; };
		if (L.O % 4 || L.ldo % 4 || L.ldx % 4 || !L.aux || !al8(L.aux) || !al8(L.out) || !al8(L.out2) || !al8(L.p) || !al8(L.t))
			throw std::runtime_error("ff layer: the derivative epilogues need O and the row strides multiples of 4 and 8-byte aligned tensors");
		if ((L.mode == FF_MODE_DACT && !L.out) || (L.mode == FF_MODE_CURV && (!L.out || !L.p || !L.t)) || (L.mode == FF_MODE_OUT_CURV && (!L.out2 || !L.t)))
			throw std::runtime_error("ff layer: a tensor of the epilogue is null");
	}
	const size_t smem = (size_t)((L.O + 31) / 32 * 32) * (L.K + 8) * sizeof(half_t);
	const uint32_t blocks = ff_blocks(L.n, 128, 1024);
	switch (L.mode) {
	case FF_MODE_ACT: k_ff_layer<FF_MODE_ACT><<<blocks, 256, smem, s>>>(L); break;
	case FF_MODE_DACT: k_ff_layer<FF_MODE_DACT><<<blocks, 256, smem, s>>>(L); break;
	case FF_MODE_F32: k_ff_layer<FF_MODE_F32><<<blocks, 256, smem, s>>>(L); break;
	case FF_MODE_CURV: k_ff_layer<FF_MODE_CURV><<<blocks, 256, smem, s>>>(L); break;
	default: k_ff_layer<FF_MODE_OUT_CURV><<<blocks, 256, smem, s>>>(L); break;
	}
}
uint32_t ff_wgrad_blocks(uint32_t n) { return ff_blocks(n, 1024, 512); }
void launch_ff_wgrad(hipStream_t s, const FfWgrad& G) {
	if (G.O == 0 || G.I == 0 || G.O > 128 || G.I > 128) throw std::runtime_error("ff wgrad: 1..128 rows and columns");
	if (!G.D2 != !G.X2) throw std::runtime_error("ff wgrad: the second product needs both of its factors");
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
