// The operator surface of the C-ABI (include/neus2_hip.h): the tcnn-shaped modules (neus_module_*, neus_context_destroy)
// and the stateless rendering operators (neus_volrend_*). None of it is part of the training step. A module's core is a
// testbed of its own, which this unit sees only through core.h: the type stays incomplete here.
#include "kernels.h"
#include "json_lite.h"
#include "host_util.h"
#include "core.h"
#include "../../include/neus2_hip.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

using namespace neus;

// ============================================================ tcnn-shaped operator modules (cpp_api.h:66-110)
// A module is tcnn's NetworkWithInputEncoding = encoding x network, held as two parts, with the call protocol (checks,
// stream, gradient modes) written once in each neus_module_* entry point:
//   Enc    the encoding part: Identity (the MLP's own input stage, ffmlp.hip), a parameter-free encoding (Identity,
//          Frequency, SphericalHarmonics or a Composite of them, encodings.hip), the 3-D 2-feature HashGrid in fp16
//          (grid.hip's paired-layout kernels; its context keeps dy/dx) or in fp32 (grid_f32.hip, stand-alone only), or
//          the general grid (grid_nd.hip). encode / backward / backward_backward are one switch each and read or write
//          either a caller tensor (stand-alone encoding: AoS / SoA / paired) or the MLP's fp16 rows [n][in_pad] (EncIO).
//   FfNet  the network part: none, or a FullyFusedMLP (ffmlp.hip) with its workspace FfWork.
// The parameters are [network | encoding] and come in through the explicit `params` pointer of every call, as
// tcnn::cpp::Module does; gradients leave through dL_dparams with EGradientMode semantics (object.h:90-94).
// Two fused specials are explicit cases beside the composed path (NeusModule::Fused): the NeuS NerfNetwork
// (nerf_network.h: encoding + density MLP + rgb MLP + variance, input NerfCoordinate [n][7] f32, output [n][16] fp16),
// which delegates to the core's net_forward / net_backward, and HashGrid -> one hidden ReLU layer -> <= 16 linear
// outputs on the fused k_dnet kernel (mlp.hip), which shares the HashGrid variant's encode / scatter / ddx steps.
// A module owns a private testbed as its core and touches it only through what core.h declares.
namespace {

std::string fmt_float(float v) { char b[32]; std::snprintf(b, sizeof(b), "%.9g", (double)v); return b; }
// `standalone`: a HashGrid module (create_encoding): tcnn's defaults for the keys a config omits
// (create_grid_encoding_templated, grid.h:2499-2525); otherwise the NeuS Testbed's (testbed.cu:2175-2187, base.json)
NeusNetworkConfig module_config(const JsonValue& enc, const JsonValue& net, const JsonValue& rgb, uint32_t batch, bool standalone = false) {
	NeusNetworkConfig c{};
	const uint32_t nf = (uint32_t)enc.number("n_features_per_level", 2);
	c.n_levels = enc.number("n_features", 0) > 0 ? (uint32_t)enc.number("n_features", 0) / nf : (uint32_t)enc.number("n_levels", 16);
	c.n_features_per_level = nf;
	c.log2_hashmap_size = (uint32_t)enc.number("log2_hashmap_size", standalone ? 19 : 15);
	c.base_resolution = (uint32_t)enc.number("base_resolution", standalone ? 16 : 0);
	if (!c.base_resolution) c.base_resolution = 1u << (c.log2_hashmap_size / 3);
	c.per_level_scale = (float)enc.number("per_level_scale", standalone ? 2.0 : 0.0);
	c.top_resolution = (float)enc.number("top_resolution", 2048.0);
	c.valid_level_scale = (float)enc.number("valid_level_scale", standalone ? 0.01 : 0.02);
	c.base_valid_level_scale = (float)enc.number("base_valid_level_scale", standalone ? 0.5 : 0.2);
	c.base_training_step = (uint32_t)enc.number("base_training_step", standalone ? 200 : 100);
	c.n_neurons = (uint32_t)net.number("n_neurons", 64);
	if ((uint32_t)rgb.number("n_neurons", c.n_neurons) != c.n_neurons) throw std::runtime_error("density and rgb networks must share n_neurons");
	c.n_density_hidden = (uint32_t)net.number("n_hidden_layers", 1);
	c.n_rgb_hidden = (uint32_t)rgb.number("n_hidden_layers", 2);
	c.batch_size = batch;
	c.sdf_bias = -0.1f;
	c.seed = 1337;
	return c;
}

struct StreamSwap {  // run a call's launches on the caller's stream (NULL: the null stream, as tcnn's cudaStream_t 0)
	Core& t; hipStream_t saved;
	StreamSwap(Core& tb, void* s) : t(tb), saved(tb.stream) { t.stream = (hipStream_t)s; }
	~StreamSwap() { t.stream = saved; }
};

}  // namespace

struct NeusContext {
	uint32_t n = 0;
	Dev<float> dydx;     // HashGrid: dy/dx [6L][n] of the forward (prepare_input_gradients)
	Dev<uint32_t> enc;   // HashGrid in front of a network: the forward's paired encoding [L][n] (k_dnet's input)
	Dev<half_t> acts;    // FullyFusedMLP: the forward's input X0 [n][in_pad] and hidden outputs [N][n][W] (post-activation)
	Dev<half_t> cosz;    // a Sine network only: cos of the hidden pre-activations [N][n][W], the derivative sin z does not give
};

namespace {

// ---------------------------------------------------------------- the network part
// tcnn FullyFusedMLP shape (fully_fused_mlp.cu:816-879): weight matrices [W][in_pad], (N - 1) x [W][W], [out_pad][W]; P = 0: no network
struct FfNet {
	uint32_t W = 0, N = 0, n_in = 0, in_pad = 0, n_out = 0, out_pad = 0, act = FF_RELU, out_act = FF_NONE;
	std::vector<uint32_t> off, rows, cols;
	uint32_t P = 0;
	bool exact = false;  // "second_order": "exact": backward_backward_input carries the act'' terms
	bool cutlass = false;  // a CutlassMLP that is no FullyFusedMLP: another width, or Sine (the hyperparams echo the otype)
	// above 128 every matrix has more than 128 rows or columns and takes ffmlp.hip's wide kernels
	bool wide() const { return W > 128; }
	uint32_t wgrad_rows(uint32_t n) const { return ff_wgrad_blocks(n, wide()); }  // partial rows of a batch's weight gradients
	// where act'' != 0: the hidden activation / any of the two (only then does an exact module differ from a default one)
	bool hidden_curved() const { return act != FF_RELU && act != FF_NONE; }
	bool sine() const { return act == FF_SINE; }  // the forward keeps cos z in the context (NeusContext::cosz)
	bool curved() const { return exact && (hidden_curved() || out_act != FF_NONE); }
	void build() {
		off.clear(); rows.clear(); cols.clear(); P = 0;
		for (uint32_t l = 0; l <= N; ++l) {
			const uint32_t r = l == N ? out_pad : W, c = l == 0 ? in_pad : W;
			off.push_back(P); rows.push_back(r); cols.push_back(c); P += r * c;
		}
	}
	size_t acts_halves(uint32_t n) const { return (size_t)n * (in_pad + (size_t)N * W); }
	// `sine`: a CutlassMLP's hidden activation (cutlass_mlp.cu:102). tcnn's fully fused kernels keep only post-activations,
	// and warp_activation_backward cannot recover cos z from sin z (common_device.h:196-200)
	static uint32_t activation(const std::string& s, bool sine = false) {
		if (s == "Sine" && sine) return FF_SINE;
		if (s == "None") return FF_NONE;
		if (s == "ReLU") return FF_RELU;
		if (s == "Exponential") return FF_EXP;
		if (s == "Sigmoid") return FF_SIGMOID;
		if (s == "Squareplus") return FF_SQUAREPLUS;
		if (s == "Softplus") return FF_SOFTPLUS;
		throw std::runtime_error("FullyFusedMLP: activation '" + s + "' is not supported on gfx950 (None, ReLU, Exponential, Sigmoid, Squareplus, "
		                         "Softplus; Sine has no backward in tcnn's fully fused MLP: a CutlassMLP takes it as its hidden \"activation\")");
	}
};
// A FullyFusedMLP from its config (fully_fused_mlp.cu:816-879): n_neurons 16 / 32 / 64 / 128, n_hidden_layers >= 1, input and
// output padded to multiples of 16 (cpp::Module::n_output_dims = the padded output width). A CutlassMLP (cutlass_mlp.cu:
// 104-150) has the same matrices, padding and initialisation at any width: n_neurons a multiple of 16 up to 512. Host only.
FfNet ff_from_json(const JsonValue& j, uint32_t n_input_dims, uint32_t n_output_dims) {
	const std::string ot = j.string("otype", "FullyFusedMLP");
	if (ot != "FullyFusedMLP" && ot != "MegakernelMLP" && ot != "CutlassMLP")
		throw std::runtime_error("only FullyFusedMLP networks are implemented on gfx950");
	FfNet f;
	f.W = (uint32_t)j.number("n_neurons", 64);
	const double nn = j.number("n_neurons", 64);
	const bool ff_width = f.W == 16 || f.W == 32 || f.W == 64 || f.W == 128;
	if (ot == "CutlassMLP") {
		if (!(nn >= 16 && nn <= 512) || nn != (double)f.W || f.W % 16)
			throw std::runtime_error("CutlassMLP: n_neurons must be a multiple of 16 from 16 to 512 on gfx950, but got " + fmt_float((float)nn));
		f.cutlass = !ff_width;
	} else if (!ff_width) {
		throw std::runtime_error("FullyFusedMLP only supports 16, 32, 64, and 128 neurons, but got " + std::to_string(f.W));
	}
	const double nh = j.number("n_hidden_layers", 1);
	if (nh < 1 || nh > 32) throw std::runtime_error("FullyFusedMLP requires at least 1 hidden layer (3 layers in total).");
	f.N = (uint32_t)nh;
	if (n_input_dims == 0 || n_input_dims > 128) throw std::runtime_error("FullyFusedMLP: 1..128 input dims on gfx950");
	if (n_output_dims == 0 || n_output_dims > 128) throw std::runtime_error("FullyFusedMLP: 1..128 output dims on gfx950");
	f.n_in = n_input_dims; f.in_pad = (n_input_dims + 15) / 16 * 16;
	f.n_out = n_output_dims; f.out_pad = (n_output_dims + 15) / 16 * 16;
	f.act = FfNet::activation(j.string("activation", "ReLU"), ot == "CutlassMLP");
	if (f.sine()) f.cutlass = true;  // at a FullyFusedMLP width too: that otype has no Sine
	// a SIREN's output layer is linear, and the output-activation path would need a stored cos of its own
	if (j.string("output_activation", "None") == "Sine")
		throw std::runtime_error(ot + ": \"output_activation\": \"Sine\" is not supported on gfx950 (Sine is a CutlassMLP's hidden \"activation\" only)");
	f.out_act = FfNet::activation(j.string("output_activation", "None"));
	const std::string so = j.string("second_order", "tcnn");
	if (so != "tcnn" && so != "exact") throw std::runtime_error("FullyFusedMLP: second_order must be tcnn or exact, but got '" + so + "'");
	f.exact = so == "exact";
	f.build();
	return f;
}
std::string ff_hyper(const FfNet& f) {
	static const char* an[7] = {"None", "ReLU", "Exponential", "Sigmoid", "Squareplus", "Softplus", "Sine"};
	return std::string("{\"otype\": \"") + (f.cutlass ? "CutlassMLP" : "FullyFusedMLP") + "\", \"n_neurons\": " + std::to_string(f.W) + ", \"n_hidden_layers\": " + std::to_string(f.N) +
	       ", \"activation\": \"" + an[f.act] + "\", \"output_activation\": \"" + an[f.out_act] + "\"" +
	       (f.exact ? ", \"second_order\": \"exact\"" : "") + "}";
}
// the network's workspace for one batch of `capacity` samples: inference activations, backward-backward fronts, the delta
// ping-pong and the per-block weight-gradient rows; for a network with act'' terms (FfNet::curved) also the curvature
// adjoints' ping-pong e, the fronts before their activation derivative p [N][n][W] and one layer's back before its t [n][W]
// (hidden act'' != 0), and the output y [n][out_pad], recomputed for the output activation's derivatives
struct FfWork {
	Dev<half_t> acts, front, d[2];
	Dev<half_t> e[2], p, t, y;
	Dev<float> partial, dummy;
	void alloc(const FfNet& f, uint32_t capacity) {
		acts.alloc(f.acts_halves(capacity));
		front.alloc((size_t)capacity * (f.in_pad + (size_t)f.N * f.W));
		const uint32_t dmax = std::max(std::max(f.W, f.out_pad), f.in_pad);
		d[0].alloc((size_t)capacity * dmax); d[1].alloc((size_t)capacity * dmax);
		partial.alloc((size_t)f.wgrad_rows(capacity) * f.P);
		dummy.alloc(4);
		if (!f.curved()) return;
		e[0].alloc((size_t)capacity * dmax); e[1].alloc((size_t)capacity * dmax);
		if (f.hidden_curved()) { p.alloc((size_t)capacity * f.N * f.W); t.alloc((size_t)capacity * f.W); }
		if (f.out_act != FF_NONE) y.alloc((size_t)capacity * f.out_pad);
	}
};
// where the backward's layer 0 puts dL/d(network input): fp16 rows [n][in_pad] for the encoding's backward, or, behind the
// Identity encoding (`direct`), W_0^T D_0 x scale straight into the caller's fp32 dL_dinput [n][n_in] (null: not computed)
struct FfSink { bool direct; float* dL_dinput; float scale; };

// FullyFusedMLP passes (ffmlp.hip). acts: X0 [n][in_pad] then hidden l at n (in_pad + l W), each [n][W].
const half_t* ff_mat(const FfNet& f, const void* params, uint32_t l) { return (const half_t*)params + f.off[l]; }
half_t* ff_hidden(const FfNet& f, const half_t* acts, uint32_t n, uint32_t l) { return const_cast<half_t*>(acts) + (size_t)n * f.in_pad + (size_t)l * n * f.W; }
// hidden layer l's cos values in a Sine network's kept buffer [N][n][W] (null for every other network)
half_t* ff_kept_cos(const FfNet& f, const half_t* cosz, uint32_t n, uint32_t l) { return cosz ? const_cast<half_t*>(cosz) + (size_t)l * n * f.W : nullptr; }
FfLayer ff_layer(const half_t* W, uint32_t O, uint32_t K, bool trans, const half_t* in, uint32_t ldi, uint32_t n) {
	FfLayer L{};
	L.W = W; L.O = O; L.K = K; L.trans = trans ? 1u : 0u; L.in = in; L.ldi = ldi; L.n = n;
	return L;
}
// forward (mlp_fused_forward, fully_fused_mlp.cu:678-812) on the encoded rows X0 in acts: hidden layers act(W x), output
// out_act(W_N h). A Sine network with a context also writes cos(W x) [N][n][W] to cosz (null: inference, nothing kept)
void ff_forward(const FfNet& f, hipStream_t s, uint32_t n, const void* params, half_t* acts, half_t* output, half_t* cosz = nullptr) {
	const half_t* x = acts;
	uint32_t ldx = f.in_pad;
	for (uint32_t l = 0; l <= f.N; ++l) {
		FfLayer L = ff_layer(ff_mat(f, params, l), f.rows[l], f.cols[l], false, x, ldx, n);
		L.mode = FF_MODE_ACT;
		L.act = l == f.N ? f.out_act : f.act;
		L.out = l == f.N ? output : ff_hidden(f, acts, n, l);
		L.ldo = l == f.N ? f.out_pad : f.W;
		if (l < f.N) L.out2 = ff_kept_cos(f, cosz, n, l);
		launch_ff_layer(s, L);
		x = L.out; ldx = f.W;
	}
}
// the output y = out_act(W_N h_N) again from a forward's activations (bitwise the forward's): the values its derivatives are taken from
void ff_output(const FfNet& f, hipStream_t s, uint32_t n, const void* params, const half_t* acts, half_t* y) {
	FfLayer L = ff_layer(ff_mat(f, params, f.N), f.rows[f.N], f.cols[f.N], false, ff_hidden(f, acts, n, f.N - 1), f.W, n);
	L.mode = FF_MODE_ACT; L.act = f.out_act; L.out = y; L.ldo = f.out_pad;
	launch_ff_layer(s, L);
}
// delta through layer l (l >= 1) to the input of layer l: act'(h_{l-1}) (W_l^T d); keep (when given): W_l^T d itself
void ff_back_through(const FfNet& f, hipStream_t s, uint32_t n, const void* params, uint32_t l, const half_t* d, uint32_t ldd, const half_t* acts_fwd,
                     const half_t* cosz, half_t* out, half_t* keep = nullptr) {
	FfLayer L = ff_layer(ff_mat(f, params, l), f.cols[l], f.rows[l], true, d, ldd, n);
	L.mode = FF_MODE_DACT; L.act = f.act; L.out = out; L.out2 = keep; L.ldo = f.W;
	L.aux = ff_hidden(f, acts_fwd, n, l - 1); L.ldx = f.W; L.auxc = ff_kept_cos(f, cosz, n, l - 1);
	launch_ff_layer(s, L);
}
void ff_wgrad(const FfNet& f, hipStream_t s, uint32_t n, uint32_t l, const half_t* d, uint32_t ldd, const half_t* x, uint32_t ldx, float* partial,
              const half_t* d2 = nullptr, const half_t* x2 = nullptr) {
	FfWgrad G{};
	G.D = d; G.ldd = ldd; G.O = f.rows[l]; G.X = x; G.ldx = ldx; G.I = f.cols[l]; G.D2 = d2; G.X2 = x2;
	G.partial = partial; G.ld_partial = f.P; G.off = f.off[l]; G.n = n;
	launch_ff_wgrad(s, G);
}
// FullyFusedMLP::backward_impl (fully_fused_mlp.cu:967-1085): the output activation's backward on dL/doutput, the deltas
// through the hidden layers (activation derivative from the stored outputs), with wgrad dW = D^T x per layer into the
// partials, and layer 0 into the sink: dL/dX0 as fp16 rows (returned; the delta ping-pong buffer), or dL/dinput = W_0^T D_0
// through the Identity encoding's backward (identity.h:86-104: x scale)
const half_t* ff_backward_chain(const FfNet& f, FfWork& w, hipStream_t s, uint32_t n, const void* params, const half_t* acts, const half_t* cosz,
                                const half_t* dL_doutput, const half_t* output, bool wgrad, const FfSink& sink) {
	const half_t* d = dL_doutput;
	int pp = 0;
	if (f.out_act != FF_NONE) { launch_ff_out_delta(s, n, f.out_pad, f.out_act, d, output, w.d[0].p); d = w.d[0].p; pp = 1; }
	uint32_t ldd = f.out_pad;
	for (uint32_t l = f.N + 1; l-- > 0;) {
		const half_t* x = l == 0 ? acts : ff_hidden(f, acts, n, l - 1);
		if (wgrad) ff_wgrad(f, s, n, l, d, ldd, x, l == 0 ? f.in_pad : f.W, w.partial.p);
		if (l > 0) {
			ff_back_through(f, s, n, params, l, d, ldd, acts, cosz, w.d[pp].p);
			d = w.d[pp].p; pp ^= 1; ldd = f.W;
		} else if (!sink.direct) {
			FfLayer L = ff_layer(ff_mat(f, params, 0), f.in_pad, f.W, true, d, ldd, n);
			L.mode = FF_MODE_ACT; L.act = FF_NONE; L.out = w.d[pp].p; L.ldo = f.in_pad;
			launch_ff_layer(s, L);
			d = w.d[pp].p;
		} else if (sink.dL_dinput) {
			FfLayer L = ff_layer(ff_mat(f, params, 0), f.in_pad, f.W, true, d, ldd, n);
			L.mode = FF_MODE_F32; L.out_f = sink.dL_dinput; L.ldo = f.n_in; L.o_lim = f.n_in; L.out_scale = sink.scale;
			launch_ff_layer(s, L);
		}
	}
	return d;
}
// FullyFusedMLP::backward_backward_input_impl (fully_fused_mlp.cu:1088-1198) with the front f_0 = the network's
// dL_ddLdinput already in w.front as rows [n][in_pad]: fronts f_i = act'(h_{i-1}) (W_{i-1} f_{i-1}); dL_ddLdoutput (when
// asked for) = the front carried through the output matrix, f_{N+1} = W_N f_N, as [n][out_pad] fp16; with wgrad the backs
// b_{N+2} = dL_doutput, b_i = act'(h_{i-2}) (W_{i-1}^T b_{i+1}) and dW_{i-1} = b_{i+1} f_{i-1}^T into the partials.
//
// That chain is exact where act'' = 0. For a network with act'' terms (FfNet::curved; the output y is in w.y) it becomes the
// exact one. With z the pre-activations, p_i = W_{i-1} f_{i-1} the fronts before their derivative (kept beside f_i), the backs
// started from the output delta d_o = dL_doutput act_o'(z_o) and t_i = W_i^T d_{i+1} the backs before theirs (kept beside d_i):
//   dL_ddLdoutput = act_o'(z_o) p_o,   e_o = act_o''(z_o) p_o dL_doutput                   (one epilogue of the last front)
//   e_i = act''(z_i) p_i t_i + act'(z_i) (W_i^T e_{i+1})                                   (one epilogue per hidden layer)
//   dW_{i-1} = d_i f_{i-1}^T + e_i h_{i-1}^T                                               (both products in one launch)
// and q = W_0^T e_1 = d(dL_ddLdinput . dL/dx)/dX0 along the forward path leaves through the sink when want_q: behind the
// Identity encoding x scale into dL_dinput, else as fp16 rows [n][in_pad] (returned) for the encoding's backward.
// A Sine network takes act'(z_i) = cos z_i from the forward's kept cosz and act''(z_i) = -h_i from acts; nothing else differs.
const half_t* ff_bbi_chain(const FfNet& f, FfWork& w, hipStream_t s, uint32_t n, const void* params, const half_t* acts, const half_t* cosz,
                           const half_t* dL_doutput, bool wgrad, half_t* dL_ddLdoutput, bool want_q = false, const FfSink& sink = FfSink{false, nullptr, 1.f}) {
	const bool cv = f.curved(), hc = cv && f.hidden_curved(), oc = cv && f.out_act != FF_NONE;
	half_t* fr = w.front.p;
	auto front = [&](uint32_t i) { return i == 0 ? fr : fr + (size_t)n * f.in_pad + (size_t)(i - 1) * n * f.W; };
	auto kept_p = [&](uint32_t i) { return w.p.p + (size_t)(i - 1) * n * f.W; };
	for (uint32_t i = 1; i <= f.N; ++i) {
		FfLayer L = ff_layer(ff_mat(f, params, i - 1), f.rows[i - 1], f.cols[i - 1], false, front(i - 1), i == 1 ? f.in_pad : f.W, n);
		L.mode = FF_MODE_DACT; L.act = f.act; L.out = front(i); L.ldo = f.W;
		L.aux = ff_hidden(f, acts, n, i - 1); L.ldx = f.W; L.auxc = ff_kept_cos(f, cosz, n, i - 1);
		if (hc) L.out2 = kept_p(i);
		launch_ff_layer(s, L);
	}
	want_q = want_q && cv;
	const half_t* e = nullptr;  // the curvature adjoint entering the layer below
	int ep = 0;
	if (oc && (dL_ddLdoutput || wgrad || want_q)) {
		FfLayer L = ff_layer(ff_mat(f, params, f.N), f.rows[f.N], f.cols[f.N], false, front(f.N), f.W, n);
		L.mode = FF_MODE_OUT_CURV; L.act = f.out_act; L.out = dL_ddLdoutput; L.out2 = w.e[0].p; L.ldo = f.out_pad;
		L.aux = w.y.p; L.ldx = f.out_pad; L.t = dL_doutput;
		launch_ff_layer(s, L);
		e = w.e[0].p; ep = 1;
	} else if (dL_ddLdoutput) {
		FfLayer L = ff_layer(ff_mat(f, params, f.N), f.rows[f.N], f.cols[f.N], false, front(f.N), f.W, n);
		L.mode = FF_MODE_ACT; L.act = FF_NONE; L.out = dL_ddLdoutput; L.ldo = f.out_pad;
		launch_ff_layer(s, L);
	}
	if (!wgrad && !want_q) return nullptr;
	const half_t* b = dL_doutput;
	uint32_t ldb = f.out_pad;
	int pp = 0;
	if (oc) { launch_ff_out_delta(s, n, f.out_pad, f.out_act, b, w.y.p, w.d[0].p); b = w.d[0].p; pp = 1; }
	for (uint32_t l = f.N + 1; l-- > 0;) {
		if (wgrad) ff_wgrad(f, s, n, l, b, ldb, front(l), l == 0 ? f.in_pad : f.W, w.partial.p, e, e ? (l == 0 ? acts : ff_hidden(f, acts, n, l - 1)) : nullptr);
		if (l > 0) {
			if (wgrad || hc) ff_back_through(f, s, n, params, l, b, ldb, acts, cosz, w.d[pp].p, hc ? w.t.p : nullptr);  // d_l, and t_l for the act'' term
			if (hc) {  // e_l; below a linear output there is no e_{l+1}: no product
				FfLayer L = ff_layer(ff_mat(f, params, l), f.cols[l], f.rows[l], true, e, ldb, n);
				L.mode = FF_MODE_CURV; L.act = f.act; L.out = w.e[ep].p; L.ldo = f.W;
				L.aux = ff_hidden(f, acts, n, l - 1); L.ldx = f.W; L.auxc = ff_kept_cos(f, cosz, n, l - 1); L.p = kept_p(l); L.t = w.t.p;
				launch_ff_layer(s, L);
			} else if (e) {
				ff_back_through(f, s, n, params, l, e, ldb, acts, cosz, w.e[ep].p);
			}
			if (hc || e) { e = w.e[ep].p; ep ^= 1; }
			b = w.d[pp].p; pp ^= 1; ldb = f.W;
		} else if (want_q && (!sink.direct || sink.dL_dinput)) {
			FfLayer L = ff_layer(ff_mat(f, params, 0), f.in_pad, f.W, true, e, ldb, n);
			if (sink.direct) { L.mode = FF_MODE_F32; L.out_f = sink.dL_dinput; L.ldo = f.n_in; L.o_lim = f.n_in; L.out_scale = sink.scale; }
			else { L.mode = FF_MODE_ACT; L.act = FF_NONE; L.out = w.e[ep].p; L.ldo = f.in_pad; }
			launch_ff_layer(s, L);
			return sink.direct ? nullptr : w.e[ep].p;
		}
	}
	return nullptr;
}
// the weight gradients from the per-block partials (fixed order), into the head of g
void ff_reduce(const FfNet& f, FfWork& w, hipStream_t s, uint32_t n_blocks, float* g) {
	launch_mlp_grad_reduce(s, MlpGradReduce{w.partial.p, n_blocks, f.P, g, nullptr, nullptr, 0, w.dummy.p});
}

// ---------------------------------------------------------------- the encoding part
// tcnn's parameter-free encodings from their config (encoding.cu create_encoding; identity.h, frequency.h,
// spherical_harmonics.h, triangle_wave.h, oneblob.h, composite.h): one segment, or a Composite's nested encodings over
// consecutive input dims (the last may leave n_dims_to_encode out and takes the rest); OneBlobFrequency / NRC is the
// Composite encoding.cu:108-129 expands it into. Host only: every check runs before a device call.
bool pf_segment_otype(const std::string& ot) {
	return ot == "Identity" || ot == "Frequency" || ot == "SphericalHarmonics" || ot == "TriangleWave" || ot == "OneBlob";
}
bool pf_nrc_otype(const std::string& ot) { return ot == "OneBlobFrequency" || ot == "NRC"; }
bool pf_otype(const std::string& ot) { return pf_segment_otype(ot) || pf_nrc_otype(ot) || ot == "Composite"; }
JsonValue json_number(double v) { JsonValue j; j.kind = JsonValue::Number; j.num = v; return j; }
void pf_add_segment(PfEnc& E, const JsonValue& j, const std::string& ot, uint32_t dims) {
	if (E.n_seg == PF_MAX_SEGMENTS) throw std::runtime_error("Composite: at most 8 nested encodings");
	if (dims == 0) throw std::runtime_error(ot + ": at least 1 input dim to encode");
	PfSegment g{};
	g.in0 = E.n_in; g.dims = dims; g.out0 = E.width; g.scale = 1.f; g.offset = 0.f;
	uint32_t w = dims;
	if (ot == "SphericalHarmonics") {
		const double deg = j.number("degree", 4);
		if (deg < 1) throw std::runtime_error("SH encoding must have positive degree.");
		if (deg > 8) throw std::runtime_error("The SH encoding is only implemented up to degree 8, but got " + std::to_string((long)deg));
		if (dims != 3) throw std::runtime_error("SphericalHarmonics: can only encode 3 input dims (a direction), but got " + std::to_string(dims));
		g.type = PF_SH; g.param = (uint32_t)deg; w = g.param * g.param;
	} else if (ot == "Frequency") {
		const double nf = j.number("n_frequencies", 12);
		if (nf < 1 || nf > 16) throw std::runtime_error("Frequency: n_frequencies must be in 1..16 on gfx950");
		g.type = PF_FREQUENCY; g.param = (uint32_t)nf; w = 2 * dims * g.param;
	} else if (ot == "TriangleWave") {
		const double nf = j.number("n_frequencies", 12);
		if (nf < 1 || nf > 16) throw std::runtime_error("TriangleWave: n_frequencies must be in 1..16 on gfx950");
		g.type = PF_TRIANGLE_WAVE; g.param = (uint32_t)nf; w = dims * g.param;
	} else if (ot == "OneBlob") {
		const double nb = j.number("n_bins", 16);
		if (nb < 1 || nb > 128) throw std::runtime_error("OneBlob: n_bins must be in 1..128 on gfx950");
		g.param = (uint32_t)nb;
		if ((double)g.param != nb || (g.param & (g.param - 1)) != 0) throw std::runtime_error("OneBlob: Number of bins must be a power of 2");
		g.type = PF_ONEBLOB; w = dims * g.param;
	} else {
		g.type = PF_IDENTITY; g.scale = (float)j.number("scale", 1.0); g.offset = (float)j.number("offset", 0.0);
	}
	E.seg[E.n_seg++] = g;
	E.n_in += dims; E.width += w;
}
PfEnc pf_from_json(const JsonValue& j, uint32_t n_input_dims) {
	if (n_input_dims == 0 || n_input_dims > (1u << 16)) throw std::runtime_error("encoding module: n_input_dims must be in 1..65536");
	PfEnc E{};
	const std::string ot = j.string("otype", "");
	if (pf_nrc_otype(ot)) {  // [TriangleWave over 3 dims | OneBlob over 5 | Identity over the rest], none at 8 dims (composite.h:92)
		if (n_input_dims < 8)
			throw std::runtime_error(ot + ": n_input_dims must be at least 8 (3 TriangleWave dims and 5 OneBlob dims), but got " + std::to_string(n_input_dims));
		JsonValue tw, ob, id;
		tw.kind = ob.kind = id.kind = JsonValue::Object;
		tw.obj["n_frequencies"] = json_number(j.number("n_frequencies", 12));
		ob.obj["n_bins"] = json_number(j.number("n_bins", 4));
		pf_add_segment(E, tw, "TriangleWave", 3);
		pf_add_segment(E, ob, "OneBlob", 5);
		if (n_input_dims > 8) pf_add_segment(E, id, "Identity", n_input_dims - 8);
		return E;
	}
	if (ot != "Composite") { pf_add_segment(E, j, ot, n_input_dims); return E; }
	if (!j.has("nested") || j.at("nested").kind != JsonValue::Array || j.at("nested").arr.empty())
		throw std::runtime_error("Composite: 'nested' must be a non-empty array of encodings");
	const std::vector<JsonValue>& nested = j.at("nested").arr;
	for (size_t i = 0; i < nested.size(); ++i) {
		const JsonValue& e = nested[i];
		if (e.kind != JsonValue::Object) throw std::runtime_error("Composite: 'nested' must be a non-empty array of encodings");
		const std::string eo = e.string("otype", "");
		if (!pf_segment_otype(eo))
			throw std::runtime_error("Composite: nested encodings must be Identity, Frequency or SphericalHarmonics, or TriangleWave or OneBlob");
		uint32_t dims = 0;
		if (e.has("n_dims_to_encode")) {
			const double d = e.number("n_dims_to_encode", 0);
			if (d < 1 || d > (double)n_input_dims) throw std::runtime_error("Composite: n_dims_to_encode must be in 1..n_input_dims");
			dims = (uint32_t)d;
		} else if (i + 1 == nested.size() && E.n_in < n_input_dims) {
			dims = n_input_dims - E.n_in;
		} else {
			throw std::runtime_error("Composite: only the last nested encoding may omit n_dims_to_encode (it takes the remaining dims)");
		}
		pf_add_segment(E, e, eo, dims);
	}
	if (E.n_in != n_input_dims)
		throw std::runtime_error("Composite: the nested encodings' n_dims_to_encode sum to " + std::to_string(E.n_in) + ", but n_input_dims is " +
		                         std::to_string(n_input_dims));
	return E;
}
std::string pf_hyper_segment(const PfSegment& g) {
	if (g.type == PF_SH) return "\"otype\": \"SphericalHarmonics\", \"degree\": " + std::to_string(g.param);
	if (g.type == PF_FREQUENCY) return "\"otype\": \"Frequency\", \"n_frequencies\": " + std::to_string(g.param);
	if (g.type == PF_TRIANGLE_WAVE) return "\"otype\": \"TriangleWave\", \"n_frequencies\": " + std::to_string(g.param);
	if (g.type == PF_ONEBLOB) return "\"otype\": \"OneBlob\", \"n_bins\": " + std::to_string(g.param);
	return "\"otype\": \"Identity\", \"scale\": " + fmt_float(g.scale) + ", \"offset\": " + fmt_float(g.offset);
}
// The grid otypes and what decides between the 3-D 2-feature kernels and the general grid (grid_nd.hip). Host only.
bool grid_otype(const std::string& ot) { return ot == "HashGrid" || ot == "Grid" || ot == "DenseGrid" || ot == "TiledGrid"; }
// scatter: "gradient_scatter" (this build's key): 0 = not set, 1 = "atomic" (what not set means), 2 = "binned": dL_dparams of the
// general grid as order-independent int64 fixed-point sums (grid_nd_scatter.hip); the fp16 3-D 2-feature kernels are binned as they are
struct GridChoice { bool general; uint32_t type; bool smooth; uint32_t scatter; };
GridChoice grid_choice(const JsonValue& j, uint32_t n_input_dims) {
	const std::string ot = j.string("otype", "HashGrid");
	const std::string ty = j.string("type", ot == "DenseGrid" ? "Dense" : (ot == "TiledGrid" ? "Tiled" : "Hash"));
	GridChoice c{};
	if (ty == "Hash") c.type = GRID_ND_HASH;
	else if (ty == "Dense") c.type = GRID_ND_DENSE;
	else if (ty == "Tiled" || ty == "Tile") c.type = GRID_ND_TILED;
	else throw std::runtime_error("grid encoding: type must be Hash, Dense or Tiled, but got '" + ty + "'");
	const std::string ip = j.string("interpolation", "Linear");
	if (ip == "Nearest") throw std::runtime_error("grid encoding: interpolation Nearest is not implemented on gfx950 (Linear or Smoothstep)");
	if (ip != "Linear" && ip != "Smoothstep") throw std::runtime_error("grid encoding: interpolation must be Linear or Smoothstep, but got '" + ip + "'");
	c.smooth = ip == "Smoothstep";
	if (j.number("stochastic_interpolation", 0) != 0)
		throw std::runtime_error("grid encoding: stochastic_interpolation is not implemented on gfx950");
	const std::string im = j.string("implementation", "auto");
	if (im != "auto" && im != "general") throw std::runtime_error("grid encoding: implementation must be auto or general");
	if (n_input_dims < 2 || n_input_dims > 4) throw std::runtime_error("grid encoding: n_input_dims must be 2, 3 or 4, but got " + std::to_string(n_input_dims));
	const double nf = j.number("n_features_per_level", 2);
	if (nf != 1 && nf != 2 && nf != 4 && nf != 8) throw std::runtime_error("grid encoding: n_features_per_level must be 1, 2, 4 or 8");
	c.general = im == "general" || n_input_dims != 3 || nf != 2 || c.type != GRID_ND_HASH || c.smooth;
	if (j.has("gradient_scatter")) {
		const std::string gs = j.string("gradient_scatter", "");
		if (gs != "atomic" && gs != "binned") throw std::runtime_error("grid encoding: gradient_scatter must be atomic or binned, but got '" + gs + "'");
		c.scatter = gs == "binned" ? 2 : 1;
	}
	return c;
}

// a tensor of an encoding operation: ld = 0: the caller's (the stand-alone encoding's output, dL_doutput or dL_ddLdoutput in
// the module's layout and precision); ld > 0: fp16 rows [n][ld] of the network (features in columns [0, width))
struct EncIO { void* p; uint32_t ld; };
EncIO enc_io(const void* p, uint32_t ld) { return EncIO{const_cast<void*>(p), ld}; }

// what the create-time parser decides, host only (enc_from_json)
struct EncSpec {
	enum Type { Identity, Pf, Hash16, Hash32, Nd } type = Identity;
	uint32_t n_in = 0;
	float scale = 1.f, offset = 0.f;  // Identity in front of a network (identity.h:44-70)
	PfEnc pf{};                       // Pf: the segments
	bool composite = false;
	GridChoice gc{};                  // Nd
	NeusNetworkConfig cfg{};          // the grids: levels, table sizes, progressive-level settings
	uint32_t width() const {
		switch (type) {
		case Identity: return n_in;
		case Pf: return pf.width;
		default: return cfg.n_features_per_level * cfg.n_levels;
		}
	}
};

struct Enc : EncSpec {
	Core* core = nullptr;             // the grids: tables (gl), layout, progressive-level settings, scatter workspace
	GridNd nd{};                      // Nd: the level tables
	uint32_t capacity = 0;
	// stand-alone output layout (ENC_LAYOUT_*): AoS [n][width] = the column-major matrix tcnn's cpp::Module wraps around the
	// caller's buffer (cpp_api.cu:58-70); SoA [width][n] = GridEncoding::preferred_output_layout (grid.h:2357-2359);
	// paired [L][n] half2 = features 2l, 2l+1 of level l adjacent, the fp16 HashGrid kernels' own
	uint32_t layout = ENC_LAYOUT_AOS;
	bool f32 = false;                 // stand-alone with requested_precision fp32: float params / output / gradients
	int training_step = 0;            // GridEncoding::set_training_step (grid.h:2427-2437): 0 = every level
	Dev<uint32_t> enc_tmp, denc_tmp;  // Hash16: paired-layout staging of non-paired I/O
	Dev<uint32_t> u_tmp;              // Hash16 in front of a network: dy/dx . dL_ddLdinput, paired
	Dev<float4> v4, zero_v;           // Hash16: dL_ddLdinput as float4 / the scatter's absent second-order term
	Dev<half_t> zero_h;
	Dev<float> partial;               // the grids: dL_dinput's per-level terms [n_in L][capacity] (first use)
	Dev<float> dx_tmp;                // in front of a network with act'' terms: the forward-path part of dL_dinput [capacity][n_in] (first use)
	Dev<long long> sc_acc;            // Nd, "gradient_scatter": "binned": int64 accumulators and poison bytes, zero between calls (first use)
	Dev<uint8_t> sc_poison;

	// ---- description
	bool keeps_dydx() const { return type == Hash16 || type == Hash32; }
	bool binned() const { return type == Nd && gc.scatter == 2; }
	// "gradient_scatter" is echoed only when the config set it
	std::string hyper_scatter() const {
		return gc.scatter ? std::string(", \"gradient_scatter\": \"") + (gc.scatter == 2 ? "binned" : "atomic") + "\"" : "";
	}
	uint32_t L() const { return core->lay.L; }
	uint32_t valid() const { return valid_level_at(core->tb, training_step); }
	uint64_t n_params() const {
		switch (type) {
		case Hash16: case Hash32: return core->lay.n_grid;
		case Nd: return (uint64_t)nd.gl.offset[nd.gl.n_levels] * nd.F;
		default: return 0;
		}
	}
	// the accepted config back as JSON members (no braces): the otype with its own keys, nested types included
	std::string hyper_members(bool standalone) const {
		const NeusNetworkConfig& c = core->cfg;
		switch (type) {
		case Identity: return "\"otype\": \"Identity\", \"scale\": " + fmt_float(scale) + ", \"offset\": " + fmt_float(offset);
		case Pf: {
			if (!composite) return pf_hyper_segment(pf.seg[0]);
			std::string s = "\"otype\": \"Composite\", \"nested\": [";
			for (uint32_t q = 0; q < pf.n_seg; ++q)
				s += std::string(q ? ", " : "") + "{\"n_dims_to_encode\": " + std::to_string(pf.seg[q].dims) + ", " + pf_hyper_segment(pf.seg[q]) + "}";
			return s + "]";
		}
		case Nd: {
			static const char* tn[3] = {"Hash", "Dense", "Tiled"};
			return "\"otype\": \"Grid\", \"type\": \"" + std::string(tn[nd.type]) + "\", \"n_input_dims\": " + std::to_string(nd.D) + ", \"n_levels\": " +
			       std::to_string(c.n_levels) + ", \"n_features_per_level\": " + std::to_string(nd.F) + ", \"log2_hashmap_size\": " +
			       std::to_string(c.log2_hashmap_size) + ", \"base_resolution\": " + std::to_string(c.base_resolution) + ", \"per_level_scale\": " +
			       fmt_float(c.per_level_scale) + ", \"interpolation\": \"" + (nd.smooth ? "Smoothstep" : "Linear") + "\", \"valid_level_scale\": " +
			       fmt_float(c.valid_level_scale) + ", \"base_valid_level_scale\": " + fmt_float(c.base_valid_level_scale) + ", \"base_training_step\": " +
			       std::to_string(c.base_training_step) + hyper_scatter();
		}
		default: {  // in front of a network the progressive-level settings are not echoed
			const std::string s = "\"otype\": \"HashGrid\", \"n_levels\": " + std::to_string(c.n_levels) + ", \"n_features_per_level\": 2, \"log2_hashmap_size\": " +
			                      std::to_string(c.log2_hashmap_size) + ", \"base_resolution\": " + std::to_string(c.base_resolution) +
			                      ", \"per_level_scale\": " + fmt_float(c.per_level_scale);
			if (!standalone) return s + hyper_scatter();
			return s + hyper_scatter() + ", \"valid_level_scale\": " + fmt_float(c.valid_level_scale) + ", \"base_valid_level_scale\": " + fmt_float(c.base_valid_level_scale) +
			       ", \"base_training_step\": " + std::to_string(c.base_training_step);
		}
		}
	}
	// the module's own "n_input_dims" member: the HashGrid has none (3), the stand-alone general grid echoes it among its own
	std::string hyper_dims(bool standalone) const {
		if (keeps_dydx() || (standalone && type == Nd)) return "";
		return ", \"n_input_dims\": " + std::to_string(n_in);
	}
	// tables and workspace (`standalone`: the I/O is the caller's, in `layout`; otherwise a network's rows or k_dnet's paired input)
	void setup(uint32_t cap, bool standalone) {
		capacity = cap;
		switch (type) {
		case Hash16:
			setup_network(core->tb, cfg, nullptr, false);
			v4.alloc(cap); zero_h.alloc((size_t)2 * L() * cap); zero_v.alloc(cap);
			if (!standalone || layout != ENC_LAYOUT_PAIRED) { enc_tmp.alloc((size_t)L() * cap); denc_tmp.alloc((size_t)L() * cap); }
			if (!standalone) u_tmp.alloc((size_t)L() * cap);
			HIP_CHECK(hipMemset(zero_h.p, 0, zero_h.n * sizeof(half_t)));
			HIP_CHECK(hipMemset(zero_v.p, 0, zero_v.n * sizeof(float4)));
			break;
		case Hash32: setup_network(core->tb, cfg, nullptr, false); break;
		case Nd:  // no Testbed network is set up: the tables, and the progressive-level settings for valid_level_at
			nd = make_grid_nd(n_in, cfg.n_features_per_level, gc.type, gc.smooth, cfg.n_levels, cfg.log2_hashmap_size, cfg.base_resolution, cfg.per_level_scale);
			core_set_levels(core->tb, cfg);
			break;
		default: break;
		}
	}
	float* scratch() { partial.alloc((size_t)n_in * L() * capacity); return partial.p; }
	// the binned scatter of the general grid: w_c dy (u null) or a_c dy into g, every parameter written; `add`: added onto g
	void nd_scatter(hipStream_t s, uint32_t n, const float* input, const float* u, EncIO dy, float* g, bool add) {
		if (!sc_acc.p) {
			const uint64_t values = grid_nd_scatter_values(nd);
			sc_acc.alloc(values); sc_poison.alloc(values);
			HIP_CHECK(hipMemsetAsync(sc_acc.p, 0, values * sizeof(long long), s));
			HIP_CHECK(hipMemsetAsync(sc_poison.p, 0, values, s));
		}
		launch_grid_nd_scatter(s, n, nd, valid(), input, u, view(dy, n), g, add, sc_acc.p, sc_poison.p);
	}
	// backward_backward_input's dL_dinput needs the encoding's second derivative: none is implemented for the spherical
	// harmonics (nor has tcnn's SphericalHarmonicsEncoding a backward_backward_input)
	void check_bbi_sh(const float* dL_dinput) const {
		bool sh = false;
		for (uint32_t q = 0; q < pf.n_seg; ++q) sh = sh || pf.seg[q].type == PF_SH;
		if (dL_dinput && sh)
			throw std::runtime_error("backward_backward_input: dL_dinput is not supported with a SphericalHarmonics segment (the second "
			                         "derivative of the spherical harmonics is not implemented); dL_ddLdoutput and the parameter gradients are");
	}
	// the pointers backward_backward_input needs beside dL_ddLdinput (a network in front asks for dL_doutput and params itself)
	bool bbi_args(const float* input, const void* dL_doutput, const void* params, const float* dL_dinput) const {
		if (type == Identity) return true;
		if (type == Pf) return input && (dL_doutput || !dL_dinput);
		return input && dL_doutput && (params || type != Nd);
	}
	// backward_backward reads dL/d(encoding output) for its parameter gradient and for dL_dinput; Identity has neither
	bool bbi_reads_dy(const float* g, const float* dL_dinput) const { return type != Identity && (g || dL_dinput); }
	// where the network's backward puts dL/d(its input): rows for this encoding's backward; Identity is the network's own input stage
	FfSink sink(float* dL_dinput) const { return FfSink{type == Identity, dL_dinput, scale}; }
	// what backward needs of the context and the call, checked before the first launch
	void check_backward(const NeusContext* ctx, const void* params, const float* dL_dinput, bool standalone) const {
		if (keeps_dydx() && !standalone && !ctx->dydx.p) throw std::runtime_error("module backward: the context is not from this module's forward");
		if (keeps_dydx() && dL_dinput && !ctx->dydx.p) throw std::runtime_error("encoding backward: dL_dinput needs the forward's dy/dx");
		if (type == Nd && dL_dinput && !params) throw std::runtime_error("module: null params");
	}

	// ---- tensors
	// a tensor of the parameter-free encodings' and the general grid's kernels: unpadded AoS / SoA, or the network's rows
	PfView view(EncIO t, uint32_t n) const {
		if (t.ld) return PfView{t.p, t.ld, 1, 0u};
		return layout == ENC_LAYOUT_SOA ? PfView{t.p, 1, n, f32 ? 1u : 0u} : PfView{t.p, width(), 1, f32 ? 1u : 0u};
	}
	uint32_t pad(EncIO t) const { return t.ld ? t.ld - width() : 0; }  // the rows' padding columns (zero, grid.h:1540-1550)
	// ---- the fp16 HashGrid's steps (also the fused k_dnet network's)
	// the stand-alone encoding's per-call copy of params into the core's buffer
	const half_t* load_params(const void* params, hipStream_t s) {
		if (!params) throw std::runtime_error("module: null params");
		half_t* grid = core->params_h + core->lay.grid_off;
		HIP_CHECK(hipMemcpyAsync(grid, params, (size_t)core->lay.n_grid * 2, hipMemcpyDeviceToDevice, s));
		return grid;
	}
	// a caller-layout dL_doutput as the kernels' paired layout
	const half_t* paired_in(const void* x, uint32_t n, hipStream_t s) {
		if (layout == ENC_LAYOUT_PAIRED) return (const half_t*)x;
		launch_enc_from_layout(s, n, L(), (const half_t*)x, layout, denc_tmp.p);
		return (const half_t*)denc_tmp.p;
	}
	// the paired encoding in front of a network: kept in the context of a forward
	uint32_t* paired_out(NeusContext* ctx, uint32_t n) {
		if (!ctx) return enc_tmp.p;
		ctx->enc.alloc((size_t)L() * std::max(1u, n));
		return ctx->enc.p;
	}
	// kernel_grid (grid.h) into the paired layout; a forward's context keeps dy/dx for dL_dinput and second order
	void hash_encode(hipStream_t s, uint32_t n, const float* input, const half_t* grid, NeusContext* ctx, uint32_t* paired) {
		float* dydx = nullptr;
		if (ctx) { ctx->dydx.alloc((size_t)6 * L() * std::max(1u, n)); dydx = ctx->dydx.p; }
		const uint32_t gx = std::max<uint32_t>(1, std::min<uint32_t>((n + 255) / 256, 4096));
		launch_grid_encode(s, nullptr, n, n, input, 3, core->gl, valid(), grid, paired, dydx, gx);
	}
	// the fused binned scatter: kernel_grid_backward (grid.h:371-500) with (first = dL_doutput, second = zero_h, v = zero_v);
	// kernel_grid_backward_input_backward_grid (grid.h:880-1007) with (zero_h, dL_doutput, v4 = dL_ddLdinput)
	void hash_scatter(hipStream_t s, uint32_t n, const float* input, const half_t* first, const half_t* second, const float4* v, float* g) {
		launch_grid_scatter(s, nullptr, n, n, input, 3, core->gl, valid(), first, second, v, g, core->swork, core->scan_tmp, core->scan_tmp_bytes);
	}
	// kernel_grid_backward_input_backward_input (grid.h:1010-1181)
	void hash_ddx(hipStream_t s, uint32_t n, const float* input, const half_t* grid, const half_t* dly, const float* u, float* dL_dinput) {
		launch_grid_ddx(s, n, n, input, core->gl, valid(), grid, dly, u, scratch(), dL_dinput);
	}

	// ---- operations. params: the encoding's own (behind the network's)
	// input -> out; a forward's context is filled where the variant keeps one
	void encode(hipStream_t s, uint32_t n, const float* input, const void* params, NeusContext* ctx, EncIO out) {
		switch (type) {
		case Identity:  // padded to the rows' width with ones (identity.h:44-70)
			launch_ff_input(s, n, n_in, out.ld, input, scale, offset, (half_t*)out.p, false);
			break;
		case Pf:  // rows: padded with ones, as tcnn's encodings pad
			if (out.ld) launch_pf_rows(s, pf, n, input, nullptr, (half_t*)out.p, out.ld);
			else launch_pf_out(s, pf, n, input, nullptr, view(out, n));
			break;
		case Hash16:
			if (out.ld) {  // zero-padded to the MLP's input width (grid.h:1540-1550)
				uint32_t* enc = paired_out(ctx, n);
				hash_encode(s, n, input, (const half_t*)params, ctx, enc);
				launch_enc_to_rows(s, n, L(), enc, (half_t*)out.p, out.ld);
			} else {
				const half_t* grid = load_params(params, s);
				uint32_t* enc = layout == ENC_LAYOUT_PAIRED ? (uint32_t*)out.p : enc_tmp.p;
				hash_encode(s, n, input, grid, ctx, enc);
				if (layout != ENC_LAYOUT_PAIRED) launch_enc_to_layout(s, n, L(), enc, (half_t*)out.p, layout);
			}
			break;
		case Hash32: {  // GridEncoding<float>::forward (kernel_grid with T = float)
			float* dydx = nullptr;
			if (ctx) { ctx->dydx.alloc((size_t)6 * L() * std::max(1u, n)); dydx = ctx->dydx.p; }
			launch_grid_f32_forward(s, n, core->gl, valid(), input, (const float*)params, (float*)out.p, layout, dydx);
			break;
		}
		case Nd:
			launch_grid_nd_forward(s, n, nd, valid(), input, params, !out.ld && f32, view(out, n), pad(out));
			break;
		}
	}
	// dy = dL/d(encoding output), the caller's dL_doutput or the network's dL/dX0 rows: the parameter gradient into g (this
	// encoding's part of the module's; null: skipped) and dL_dinput = J^T dy (null: skipped)
	void backward(hipStream_t s, uint32_t n, const NeusContext* ctx, const float* input, EncIO dy, const void* params, float* g, float* dL_dinput) {
		switch (type) {
		case Identity: break;  // no parameters; the network's layer 0 wrote dL_dinput (FfSink)
		case Pf:  // the Jacobian recomputed from the input
			if (dL_dinput) launch_pf_input_grad(s, pf, n, input, view(dy, n), nullptr, dL_dinput);
			break;
		case Hash16: {  // the grid gradient through the fused binned scatter, second-order term zero; dL_dinput from dy/dx
			const half_t* dly = (const half_t*)denc_tmp.p;
			if (dy.ld) launch_enc_from_rows(s, n, L(), (const half_t*)dy.p, dy.ld, denc_tmp.p);
			else { load_params(params, s); dly = paired_in(dy.p, n, s); }
			if (!dy.ld && dL_dinput) launch_enc_input_grad(s, n, n, L(), dly, ctx->dydx.p, dL_dinput, 3);
			if (g) hash_scatter(s, n, input, dly, zero_h.p, zero_v.p, g);
			if (dy.ld && dL_dinput) launch_enc_input_grad(s, n, n, L(), dly, ctx->dydx.p, dL_dinput, 3);
			break;
		}
		case Hash32:  // GridEncoding<float>::backward: kernel_grid_backward (float atomics) and dL_dinput from dy/dx
			if (g) HIP_CHECK(hipMemsetAsync(g, 0, (size_t)n_params() * 4, s));
			launch_grid_f32_backward(s, n, core->gl, valid(), input, (const float*)dy.p, layout, g, ctx->dydx.p, dL_dinput);
			break;
		case Nd:  // kernel_grid_backward by fp32 atomics into a zeroed buffer; dL_dinput with the Jacobian gathered again from the input
			if (g && binned()) {
				nd_scatter(s, n, input, nullptr, dy, g, false);
			} else if (g) {
				HIP_CHECK(hipMemsetAsync(g, 0, (size_t)n_params() * 4, s));
				launch_grid_nd_backward(s, n, nd, valid(), input, view(dy, n), g);
			}
			if (dL_dinput) launch_grid_nd_input_grad(s, n, nd, valid(), input, params, !dy.ld && f32, view(dy, n), scratch(), dL_dinput);
			break;
		}
	}
	// GridEncoding::backward_backward_input (grid.h:880-1181) and its parameter-free counterparts. u = dL_ddLdinput, dy =
	// dL/d(encoding output): the second-order parameter gradient into g, J u into Ju (the caller's dL_ddLdoutput or the
	// network's front rows) and dL_dinput; each is skipped when null. `curved`: a network with act'' terms follows, whose
	// chain's q = dS/dX0 comes back through backward_curved: what that call completes is left to it
	void backward_backward(hipStream_t s, uint32_t n, const NeusContext* ctx, const float* input, const float* u, EncIO dy, const void* params, float* g,
	                       EncIO Ju, float* dL_dinput, bool curved = false) {
		switch (type) {
		case Identity:
			// identity.h:182-206: the network's dL_ddLdinput = scale x u (the padded rows, which the reference leaves uninitialised,
			// are 0: the constant padding has no input gradient); dL_dinput = 0: with act'' = 0 the first derivative is piecewise
			// constant in the input (curved: the network's chain writes scale x q)
			if (dL_dinput && !curved) HIP_CHECK(hipMemsetAsync(dL_dinput, 0, (size_t)n * n_in * 4, s));
			if (Ju.p) launch_ff_input(s, n, n_in, Ju.ld, u, scale, 0.f, (half_t*)Ju.p, true);
			break;
		case Pf:
			// J u from first derivatives only; dL_dinput_d = u_d sum_k dy_k d2y_k/dx_d^2 (every feature depends on one input dim,
			// except the spherical harmonics': refused)
			if (dL_dinput) launch_pf_input_grad(s, pf, n, input, view(dy, n), u, dL_dinput);
			if (Ju.p && Ju.ld) launch_pf_rows(s, pf, n, input, u, (half_t*)Ju.p, Ju.ld);
			else if (Ju.p) launch_pf_out(s, pf, n, input, u, view(Ju, n));
			break;
		case Hash16:
			// pos_encoding_dy = dy/dx . u (kernel_grid_backward_input_backward_dLdoutput, grid.h:1697-1800; also u as float4 for the
			// scatter), the second-order grid gradient and the grid's second derivative in x
			if (Ju.ld) {
				const half_t* dly = (const half_t*)denc_tmp.p;
				if (dy.p) launch_enc_from_rows(s, n, L(), (const half_t*)dy.p, dy.ld, denc_tmp.p);
				if (g || Ju.p) launch_enc_ddLdoutput(s, n, n, L(), u, ctx->dydx.p, (half_t*)u_tmp.p, v4.p);
				if (g && !curved) hash_scatter(s, n, input, zero_h.p, dly, v4.p, g);  // curved: with q as its first-order cotangent
				if (dL_dinput) hash_ddx(s, n, input, (const half_t*)params, dly, u, dL_dinput);
				if (Ju.p) launch_enc_to_rows(s, n, L(), u_tmp.p, (half_t*)Ju.p, Ju.ld);
			} else {
				const bool relay = layout != ENC_LAYOUT_PAIRED && Ju.p;
				launch_enc_ddLdoutput(s, n, n, L(), u, ctx->dydx.p, relay ? (half_t*)enc_tmp.p : (half_t*)Ju.p, v4.p);
				if (relay) launch_enc_to_layout(s, n, L(), enc_tmp.p, (half_t*)Ju.p, layout);
				if (g || dL_dinput) {
					const half_t* grid = load_params(params, s);
					const half_t* dly = paired_in(dy.p, n, s);
					if (g) hash_scatter(s, n, input, zero_h.p, dly, v4.p, g);
					if (dL_dinput) hash_ddx(s, n, input, grid, dly, u, dL_dinput);
				}
			}
			break;
		case Hash32:  // GridEncoding<float>::backward_backward_input (grid.h:880-1007 with GRAD_T = float; grid.h:1010-1181)
			if (dL_dinput && !params) throw std::runtime_error("module: null params");
			if (g) HIP_CHECK(hipMemsetAsync(g, 0, (size_t)n_params() * 4, s));
			launch_grid_f32_bbi(s, n, core->gl, valid(), input, u, (const float*)dy.p, layout, g, ctx->dydx.p, (float*)Ju.p);
			if (dL_dinput) launch_grid_f32_ddx(s, n, core->gl, valid(), input, (const float*)params, (const float*)dy.p, layout, u, scratch(), dL_dinput);
			break;
		case Nd:  // one launch: atomics into a zeroed buffer, J u, and dL_dinput (mixed terms, and the diagonal ones with Smoothstep)
			if (g && binned()) nd_scatter(s, n, input, u, dy, g, false);  // the scatter on its own; the launch below without it
			else if (g) HIP_CHECK(hipMemsetAsync(g, 0, (size_t)n_params() * 4, s));
			launch_grid_nd_bbi(s, n, nd, valid(), input, params, !Ju.ld && f32, u, view(dy, n), binned() ? nullptr : g, view(Ju, n), pad(Ju),
			                   dL_dinput ? scratch() : nullptr, dL_dinput);
			break;
		}
	}
	// The rest of backward_backward in front of a network with act'' terms: q = dS/dX0 [n][q.ld] from the network's chain
	// goes through this encoding's first-order backward, J_theta^T q added into g and J^T q into dL_dinput
	void backward_curved(hipStream_t s, uint32_t n, const NeusContext* ctx, const float* input, EncIO q, const void* params, float* g, float* dL_dinput) {
		float* dx = nullptr;
		if (dL_dinput && type != Identity) { dx_tmp.alloc((size_t)n_in * capacity); dx = dx_tmp.p; }
		switch (type) {
		case Pf:
			if (dx) launch_pf_input_grad(s, pf, n, input, view(q, n), nullptr, dx);
			break;
		case Hash16: {  // the deferred scatter takes q beside the second-order cotangent (denc_tmp, v4: backward_backward's)
			if (!g && !dx) break;
			launch_enc_from_rows(s, n, L(), (const half_t*)q.p, q.ld, enc_tmp.p);
			if (g) hash_scatter(s, n, input, (const half_t*)enc_tmp.p, (const half_t*)denc_tmp.p, v4.p, g);
			if (dx) launch_enc_input_grad(s, n, n, L(), (const half_t*)enc_tmp.p, ctx->dydx.p, dx, 3);
			break;
		}
		case Nd:  // atomics on top of backward_backward's: its memset stands for both (binned: its sums added onto backward_backward's, one fp32 add each)
			if (g && binned()) nd_scatter(s, n, input, nullptr, q, g, true);
			else if (g) launch_grid_nd_backward(s, n, nd, valid(), input, view(q, n), g);
			if (dx) launch_grid_nd_input_grad(s, n, nd, valid(), input, params, false, view(q, n), scratch(), dx);
			break;
		default: break;  // Identity: the network's layer 0 wrote dL_dinput (FfSink)
		}
		if (dx) launch_add_f32(s, n * n_in, dx, dL_dinput);
	}
};

// The create-time parser of the encoding part (`with_net`: in front of a network, where Identity is the MLP's own input
// stage). Host only: every check runs before a device call.
EncSpec enc_from_json(const JsonValue& j, uint32_t n_input_dims, uint32_t batch_capacity, bool with_net) {
	EncSpec e;
	const std::string ot = j.string("otype", "HashGrid");
	e.n_in = n_input_dims;
	if (with_net && ot == "Identity") {
		e.type = EncSpec::Identity; e.scale = (float)j.number("scale", 1.0); e.offset = (float)j.number("offset", 0.0);
		return e;
	}
	if (pf_otype(ot)) {
		e.type = EncSpec::Pf; e.pf = pf_from_json(j, n_input_dims); e.composite = !pf_segment_otype(ot);
		return e;
	}
	if (!grid_otype(ot))
		throw std::runtime_error(with_net ? "network with input encoding: the encoding must be Identity, Frequency, SphericalHarmonics, TriangleWave, "
		                                    "OneBlob, OneBlobFrequency / NRC, Composite or a grid (HashGrid / Grid / DenseGrid / TiledGrid) on gfx950"
		                                  : "encoding module: HashGrid / Grid / DenseGrid / TiledGrid, Identity, Frequency, SphericalHarmonics, "
		                                    "TriangleWave, OneBlob, OneBlobFrequency / NRC and Composite are implemented on gfx950");
	e.gc = grid_choice(j, n_input_dims);
	e.type = e.gc.general ? EncSpec::Nd : EncSpec::Hash16;
	JsonValue none; none.kind = JsonValue::Object;
	e.cfg = module_config(j, none, none, batch_capacity, true);
	if (with_net && e.gc.general && (uint64_t)e.cfg.n_levels * e.cfg.n_features_per_level > 128)
		throw std::runtime_error("network with input encoding: the grid's encoded width n_features_per_level * n_levels = " +
		                         std::to_string((uint64_t)e.cfg.n_levels * e.cfg.n_features_per_level) +
		                         " exceeds the 128 input dims of the FullyFusedMLP on gfx950");
	if (e.cfg.n_levels == 0 || e.cfg.n_levels > MAX_LEVELS)
		throw std::runtime_error(std::string(e.gc.general ? "grid encoding" : "GridEncoding") + ": 1..16 levels supported");
	return e;
}

}  // namespace

struct NeusModule {
	// Composed: enc (and ff, when it has a network) through the shared path; the two fused specials: Nerf = the NeuS
	// NerfNetwork on the core's own kernels, Dnet = HashGrid -> FullyFusedMLP(1 hidden ReLU layer, <= 16 linear outputs) on
	// k_dnet, the network whose backward_backward_input tcnn implements (network_with_input_encoding.h:159-250,
	// fully_fused_mlp.cu:1088-1198)
	enum Fused { Composed = 0, Nerf = 1, Dnet = 2 } fused = Composed;
	Enc enc;                     // Nerf: only its tag (a HashGrid) and training_step
	FfNet ff;                    // P = 0: a stand-alone encoding; Dnet: the fused network's shape
	FfWork fw;                   // Dnet: only k_dnet's per-block weight-gradient rows (partial) and dummy
	std::unique_ptr<Core, void (*)(Core*)> core;
	uint32_t capacity = 0, n_in = 0, n_out = 0;
	uint64_t P = 0;              // n_params = [network | encoding]
	uint32_t enc_off = 0;        // the parameters ahead of the encoding's (neus_module_info's grid_offset)
	uint32_t indeed_batch = 0;   // NeuS backward normalisation of the eikonal entries; 0 = the call's n
	std::string hyper;
	bool grad_fp16 = true;       // dL_dparams in param precision (fp16, trainer.h:72-109) or fp32
	Dev<float> gtmp;             // gradients of an Accumulate call (and of every fp16-gradient call)
	Dev<float4> dpos;            // Nerf: dL/dposition of net_backward
	explicit NeusModule(int device) : core(core_create(device), core_destroy) { enc.core = core.get(); }
	bool net() const { return fused == Composed && ff.P; }
	const void* enc_params(const void* params) const { return (const half_t*)params + enc_off; }
	void check_n(uint32_t n, bool backward) const {
		if (n > capacity) throw std::runtime_error("module: n_elements exceeds the module's batch capacity");
		if (backward && fused == Nerf && (n == 0 || n % 128 != 0))
			throw std::runtime_error("module backward: n_elements must be a positive multiple of 128 (fully_fused_mlp.cu:779-781)");
		if (net() && n % 128 != 0) throw std::runtime_error("FullyFusedMLP: batch size must be a multiple of 128 (fully_fused_mlp.cu:779-781)");
	}
	// the destination of this call's parameter gradients (Overwrite: dL_dparams itself; Accumulate: a scratch buffer); null
	// with Ignore and for a module without parameters
	float* grad_target(void* dL_dparams, int mode) {
		if (!P || mode == NEUS_GRADIENT_IGNORE) return nullptr;
		if (!dL_dparams) throw std::runtime_error("module: dL_dparams is null with a gradient mode other than Ignore");
		if (mode != NEUS_GRADIENT_OVERWRITE && mode != NEUS_GRADIENT_ACCUMULATE) throw std::runtime_error("module: unknown gradient mode");
		if (mode == NEUS_GRADIENT_OVERWRITE && !grad_fp16) return (float*)dL_dparams;
		return gtmp.p;
	}
	// the epilogue of a call with parameter gradients: the network's weight gradients from its partials, then g into dL_dparams
	void finish_grad(float* g, uint32_t n, void* dL_dparams, int mode, hipStream_t s) {
		if (!g) return;
		if (net()) ff_reduce(ff, fw, s, ff.wgrad_rows(n), g);
		if (grad_fp16) launch_grad_to_half(s, (uint32_t)P, gtmp.p, (half_t*)dL_dparams, mode == NEUS_GRADIENT_ACCUMULATE);
		else if (mode == NEUS_GRADIENT_ACCUMULATE) launch_add_f32(s, (uint32_t)P, gtmp.p, (float*)dL_dparams);
	}
	// backward_backward_input's dL_ddLdoutput / dL_dinput of a network: the fronts / backs chain has no act'' term, so they
	// are exact only where act'' = 0 (hidden ReLU or None) and the output is linear
	void check_bbi_exact(const void* dL_ddLdoutput, const float* dL_dinput) const {
		if (!ff.P || ff.exact || (!dL_ddLdoutput && !dL_dinput)) return;
		if ((ff.act == FF_RELU || ff.act == FF_NONE) && ff.out_act == FF_NONE) return;
		throw std::runtime_error("backward_backward_input: dL_ddLdoutput and dL_dinput are exact only for hidden activation ReLU or None with "
		                         "output activation None (the second derivative of any other activation is not implemented); pass null "
		                         "for both to get the parameter gradients alone");
	}
	// a context of this module's forward
	bool ctx_ok(const NeusContext* ctx) const {
		return (!enc.keeps_dydx() || ctx->dydx.p) && (!net() || (ctx->acts.p && (!ff.sine() || ctx->cosz.p))) && (fused != Dnet || ctx->enc.p);
	}
};

// ---------------------------------------------------------------- creation
static void check_capacity(uint32_t batch_capacity) {
	if (batch_capacity == 0 || batch_capacity % 128 != 0 || batch_capacity > (1u << 24))
		throw std::runtime_error("batch_capacity must be a positive multiple of 128 (<= 2^24)");
}
// cpp_api.cu:174-180: Fp32 -> an encoding with float params, output and gradients, Fp16 -> __half
static bool precision_f32(int requested_precision) {
	if (requested_precision != NEUS_PRECISION_FP32 && requested_precision != NEUS_PRECISION_FP16)
		throw std::runtime_error("create_encoding: requested_precision must be NEUS_PRECISION_FP32 or NEUS_PRECISION_FP16");
	return requested_precision == NEUS_PRECISION_FP32;
}
// A module of the parsed parts with its options (this build's keys, beside tcnn's): "gradient_precision": "fp16" (default,
// tcnn's param precision) | "fp32"; encoding "output_layout": "AoS" (default: cpp::Module's column-major view) | "SoA" | "paired";
// network "second_order": "tcnn" (default: tcnn's double-backward chain, without act'') | "exact" (ff_from_json)
static std::unique_ptr<NeusModule> new_module(const EncSpec& e, const FfNet& f, const JsonValue& j, uint32_t batch_capacity) {
	int dev = 0;
	HIP_CHECK(hipGetDevice(&dev));
	auto m = std::make_unique<NeusModule>(dev);
	static_cast<EncSpec&>(m->enc) = e;
	m->ff = f;
	m->capacity = batch_capacity;
	const std::string gp = j.string("gradient_precision", "fp16");
	if (gp != "fp16" && gp != "fp32") throw std::runtime_error("module: gradient_precision must be fp16 or fp32");
	m->grad_fp16 = gp == "fp16";
	const std::string ol = j.string("output_layout", "AoS");
	if (ol == "AoS") m->enc.layout = ENC_LAYOUT_AOS;
	else if (ol == "SoA") m->enc.layout = ENC_LAYOUT_SOA;
	else if (ol == "paired") m->enc.layout = ENC_LAYOUT_PAIRED;
	else throw std::runtime_error("encoding module: output_layout must be AoS, SoA or paired");
	return m;
}
static std::string hyper_gradient_precision(const NeusModule* m) {
	return std::string(", \"gradient_precision\": \"") + (m->grad_fp16 ? "fp16" : "fp32") + "\"";
}
// the accepted config back as JSON: the encoding's members, the network's, and the common tail
static std::string module_hyper(const NeusModule* m) {
	static const char* lay_names[3] = {"AoS", "SoA", "paired"};
	const Enc& e = m->enc;
	if (!m->ff.P)
		return "{" + e.hyper_members(true) + e.hyper_dims(true) + ", \"output_layout\": \"" + lay_names[e.layout] + "\"" + hyper_gradient_precision(m) +
		       ", \"precision\": \"" + (e.f32 ? "fp32" : "fp16") + "\"}";
	return "{\"otype\": \"NetworkWithInputEncoding\", \"encoding\": {" + e.hyper_members(false) + "}, \"network\": " + ff_hyper(m->ff) + e.hyper_dims(false) +
	       ", \"n_output_dims\": " + std::to_string(m->ff.n_out) + hyper_gradient_precision(m) + "}";
}
// the parts are set: their tables and workspace, the sizes both are asked for, the hyper-parameters
static NeusModule* module_finish(std::unique_ptr<NeusModule> m) {
	const bool standalone = !m->ff.P;
	m->enc.setup(m->capacity, standalone);
	m->enc_off = m->ff.P;
	m->P = m->enc_off + m->enc.n_params();
	m->n_in = m->enc.n_in;
	m->n_out = standalone ? m->enc.width() : m->ff.out_pad;  // cpp::Module::n_output_dims = the padded output width
	m->gtmp.alloc(m->P);
	if (m->fused == NeusModule::Dnet) { m->fw.partial.alloc((size_t)dnet_blocks(m->capacity) * m->ff.P); m->fw.dummy.alloc(4); }
	else if (m->ff.P) m->fw.alloc(m->ff, m->capacity);
	m->hyper = module_hyper(m.get());
	HIP_CHECK(hipStreamSynchronize(m->core->stream));
	return m.release();
}

int neus_module_create_nerf_network(const char* config_json, uint32_t batch_capacity, NeusModule** out) {
	return guard([&] {
		if (!config_json || !out) throw std::runtime_error("neus_module_create_nerf_network: null argument");
		check_capacity(batch_capacity);
		const JsonValue j = parse_json(config_json);
		EncSpec e;
		e.type = EncSpec::Hash16;
		auto m = new_module(e, FfNet{}, j, batch_capacity);
		m->fused = NeusModule::Nerf;
		m->enc.layout = ENC_LAYOUT_AOS;
		setup_network(m->core->tb, module_config(j.object("encoding"), j.object("network"), j.object("rgb_network"), batch_capacity), nullptr);
		m->n_in = COORD_W; m->n_out = OUT_W;
		m->P = m->core->lay.P; m->enc_off = m->core->lay.grid_off;
		const NeusNetworkConfig& c = m->core->cfg;
		m->hyper = "{\"otype\": \"NerfNetwork\", \"n_levels\": " + std::to_string(c.n_levels) + ", \"n_neurons\": " + std::to_string(c.n_neurons) +
		           ", \"log2_hashmap_size\": " + std::to_string(c.log2_hashmap_size) + ", \"per_level_scale\": " + fmt_float(c.per_level_scale) +
		           hyper_gradient_precision(m.get()) + "}";
		m->gtmp.alloc(m->P);
		m->dpos.alloc(batch_capacity);
		HIP_CHECK(hipStreamSynchronize(m->core->stream));
		*out = m.release();
	});
}

// create_encoding: a parameter-free encoding (any n_input_dims), the HashGrid (3 inputs, 2 features; fp32: GridEncoding<float>)
// or the general grid; any n <= batch_capacity, output [n][width] (AoS) or [width][n] (SoA) in the requested precision,
// unpadded (the fp16 HashGrid also paired)
int neus_module_create_encoding(uint32_t n_input_dims, const char* encoding_json, int requested_precision, uint32_t batch_capacity,
                                NeusModule** out) {
	return guard([&] {
		if (!encoding_json || !out) throw std::runtime_error("neus_module_create_encoding: null argument");
		const JsonValue j = parse_json(encoding_json);
		check_capacity(batch_capacity);
		const bool f32 = precision_f32(requested_precision);
		EncSpec e = enc_from_json(j, n_input_dims, batch_capacity, false);
		if (j.string("output_layout", "AoS") == "paired") {
			if (e.type == EncSpec::Pf) throw std::runtime_error("parameter-free encoding: output_layout AoS or SoA (paired is the HashGrid kernels' layout)");
			if (e.type == EncSpec::Nd) throw std::runtime_error("general grid encoding: output_layout AoS or SoA (paired is the 3-D, 2-feature fp16 kernels' layout)");
			if (f32) throw std::runtime_error("fp32 HashGrid: output_layout AoS or SoA (paired is the fp16 kernels' layout)");
		}
		if (f32 && e.type == EncSpec::Hash16 && e.gc.scatter == 2)
			throw std::runtime_error("fp32 HashGrid: gradient_scatter binned is not implemented on the 3-D 2-feature fp32 kernels; "
			                         "\"implementation\": \"general\" runs this config on the general grid, which has it");
		if (f32 && e.type == EncSpec::Hash16) e.type = EncSpec::Hash32;
		auto m = new_module(e, FfNet{}, j, batch_capacity);
		m->enc.f32 = f32;
		if (f32 && e.type != EncSpec::Pf) m->grad_fp16 = false;  // float parameters: float gradients
		*out = module_finish(std::move(m));
	});
}

// create_network_with_input_encoding (cpp_api.h:108; network_with_input_encoding.h): any encoding of create_encoding, or
// Identity with scale / offset (any input width), in front of a FullyFusedMLP (or CutlassMLP: ff_from_json) of any depth, width and
// activations. HashGrid -> one hidden ReLU layer -> linear network of width 16 / 64 runs on the fused k_dnet kernel.
int neus_module_create_network_with_input_encoding(uint32_t n_input_dims, uint32_t n_output_dims, const char* encoding_json,
                                                   const char* network_json, uint32_t batch_capacity, NeusModule** out) {
	return guard([&] {
		if (!encoding_json || !network_json || !out) throw std::runtime_error("neus_module_create_network_with_input_encoding: null argument");
		check_capacity(batch_capacity);
		const JsonValue je = parse_json(encoding_json), jn = parse_json(network_json);
		const EncSpec e = enc_from_json(je, n_input_dims, batch_capacity, true);
		const FfNet f = ff_from_json(jn, e.width(), n_output_dims);
		auto m = new_module(e, f, jn, batch_capacity);
		m->enc.layout = ENC_LAYOUT_AOS;
		if (e.type == EncSpec::Hash16 && f.act == FF_RELU && f.out_act == FF_NONE && f.N == 1 && n_output_dims <= 16 && dnet_supported(e.cfg.n_levels, f.W))
			m->fused = NeusModule::Dnet;
		*out = module_finish(std::move(m));
	});
}

// tcnn::cpp::create_network(n_input_dims, n_output_dims, network) (cpp_api.cu:170-172): NetworkWithInputEncoding with an
// Identity encoding (scale 1, offset 0; padded to 16 inputs with ones, identity.h:44-70) and a FullyFusedMLP
int neus_module_create_network(uint32_t n_input_dims, uint32_t n_output_dims, const char* network_json, uint32_t batch_capacity, NeusModule** out) {
	return guard([&] {
		if (!network_json || !out) throw std::runtime_error("neus_module_create_network: null argument");
		check_capacity(batch_capacity);
		const JsonValue j = parse_json(network_json);
		EncSpec e;
		e.n_in = n_input_dims;
		auto m = new_module(e, ff_from_json(j, n_input_dims, n_output_dims), j, batch_capacity);
		*out = module_finish(std::move(m));
	});
}

int neus_module_destroy(NeusModule* m) { return guard([&] { delete m; }); }
int neus_context_destroy(NeusContext* c) { return guard([&] { delete c; }); }

int neus_module_info(const NeusModule* m, NeusModuleInfo* o) {
	return guard([&] {
		if (!m || !o) throw std::runtime_error("neus_module_info: null argument");
		o->n_params = m->P;
		o->n_input_dims = m->n_in;
		o->n_output_dims = m->n_out;
		o->param_precision = m->enc.f32 ? NEUS_PRECISION_FP32 : NEUS_PRECISION_FP16;
		o->output_precision = m->enc.f32 ? NEUS_PRECISION_FP32 : NEUS_PRECISION_FP16;
		o->gradient_precision = NEUS_PRECISION_FP32;
		o->batch_capacity = m->capacity;
		o->n_levels = m->enc.n_params() ? m->core->lay.L : 0;
		o->grid_offset = m->enc_off;
		o->per_level_scale = m->core->cfg.per_level_scale;
	});
}

int neus_module_hyperparams(const NeusModule* m, char* buf, uint64_t cap, uint64_t* len) {
	return guard([&] {
		if (!m) throw std::runtime_error("neus_module_hyperparams: null module");
		if (len) *len = m->hyper.size();
		if (buf && cap) { const size_t k = std::min<size_t>(cap - 1, m->hyper.size()); std::memcpy(buf, m->hyper.data(), k); buf[k] = 0; }
	});
}

int neus_module_set_training_step(NeusModule* m, int training_step) { return guard([&] { m->enc.training_step = training_step; }); }
int neus_module_set_indeed_batch_size(NeusModule* m, uint32_t n) { return guard([&] { m->indeed_batch = n; }); }

int neus_module_initialize_params(NeusModule* m, uint64_t seed, float* params_full_precision) {
	return guard([&] {
		if (!m || (!params_full_precision && m->P)) throw std::runtime_error("neus_module_initialize_params: null argument");
		if (m->P == 0) return;  // a parameter-free encoding
		HIP_CHECK(hipSetDevice(m->core->device));
		std::vector<float> h;
		// cpp::Module::initialize_params draws from pcg32{seed} (cpp_api.cu:162-165; the Trainer's seed_seq is not involved)
		if (m->fused == NeusModule::Nerf) {
			h = initial_params_rng(m->core->tb, make_pcg32(seed), nullptr);
		} else {
			// NetworkWithInputEncoding::initialize_params: the network, then the encoding. FullyFusedMLP::initialize_params
			// (fully_fused_mlp.cu:1229-1256): every matrix xavier-uniform in order, U(+-sqrt(6 / (fan_in + fan_out)))
			// (gpu_matrix.h:292-306); GridEncoding::initialize_params: generate_random_uniform(rnd, n_params, -1e-4, 1e-4)
			// (grid.h:2375-2380); the parameter-free encodings have none
			h.assign(m->P, 0.f);
			pcg32 rnd = make_pcg32(seed);
			size_t off = 0;
			auto xavier = [&](uint32_t out, uint32_t in) {
				const float scale = std::sqrt(6.0f / (float)(in + out));
				for (uint32_t i = 0; i < out * in; ++i) h[off + i] = rnd.next_float() * 2.0f * scale - scale;
				off += (size_t)out * in;
			};
			// a Sine network: CutlassMLP::initialize_params' SIREN branch (cutlass_mlp.cu:1090-1098): the first matrix
			// U(+-30 / fan_in), every other U(+-sqrt(6 / fan_in)), fan_in the matrix's padded column count (gpu_matrix.h:343-375);
			// the same draws in the same order
			auto siren = [&](uint32_t out, uint32_t in, bool first) {
				const float scale = first ? 30.0f / (float)in : std::sqrt(6.0f / (float)in);
				for (uint32_t i = 0; i < out * in; ++i) h[off + i] = rnd.next_float() * 2.0f * scale - scale;
				off += (size_t)out * in;
			};
			for (size_t l = 0; l < m->ff.rows.size(); ++l) {
				if (m->ff.sine()) siren(m->ff.rows[l], m->ff.cols[l], l == 0);
				else xavier(m->ff.rows[l], m->ff.cols[l]);
			}
			float* hg = h.data() + off;
			const size_t N = h.size() - off, per = 4, n_threads = (N + per - 1) / per, n_pad = (n_threads + 127) / 128 * 128;
			for (size_t i = 0; i < n_pad; ++i) {
				pcg32 r = rnd; r.advance((int64_t)(i * per));
				for (size_t k = 0; k < per; ++k) {
					const size_t idx = i + n_pad * k;
					if (idx >= N) break;
					hg[idx] = r.next_float() * (1e-4f - -1e-4f) + -1e-4f;
				}
			}
		}
		HIP_CHECK(hipMemcpy(params_full_precision, h.data(), h.size() * 4, hipMemcpyHostToDevice));
	});
}

// ---------------------------------------------------------------- the two fused specials
namespace {
// the NeuS NerfNetwork: params into the core's fp16 buffer and its transposed weight copies, then the Testbed's kernels
void nerf_load_params(NeusModule* m, const void* params, hipStream_t s) {
	if (!params) throw std::runtime_error("module: null params");
	HIP_CHECK(hipMemcpyAsync(m->core->params_h, params, (size_t)m->core->lay.P * 2, hipMemcpyDeviceToDevice, s));
	prepare_weights(m->core->tb);
}
void nerf_forward(NeusModule* m, hipStream_t s, uint32_t n, const float* input, void* output, const void* params) {
	nerf_load_params(m, params, s);
	net_forward(m->core->tb, nullptr, n, n, input, m->enc.valid(), (half_t*)output, s);
}
// NerfNetwork::backward (nerf_network.h:330-601): first and second order in one pass; the Testbed's forward-recompute +
// backward writes every parameter gradient (Overwrite) into g
void nerf_backward(NeusModule* m, hipStream_t s, uint32_t n, const float* input, const void* dL_doutput, const void* params, float* g, float* dL_dinput) {
	Core& t = *m->core;
	nerf_load_params(m, params, s);
	float* gg = g ? g : m->gtmp.p;
	HIP_CHECK(hipMemsetAsync(gg, 0, (size_t)t.lay.P * 4, s));
	const float saved = t.tbuf.indeed_batch;
	t.tbuf.indeed_batch = (float)(m->indeed_batch ? m->indeed_batch : n);
	t.tbuf.dpos = dL_dinput ? m->dpos.p : nullptr;
	net_backward(t.tb, nullptr, nullptr, n, input, m->enc.valid(), (const half_t*)dL_doutput, gg, s);
	t.tbuf.dpos = nullptr;
	t.tbuf.indeed_batch = saved;
	if (dL_dinput) {  // position columns; dt and direction columns are 0 (the direction gradient is not propagated)
		HIP_CHECK(hipMemset2DAsync(dL_dinput, COORD_W * 4, 0, COORD_W * 4, n, s));
		HIP_CHECK(hipMemcpy2DAsync(dL_dinput, COORD_W * 4, m->dpos.p, 16, 12, n, hipMemcpyDeviceToDevice, s));
	}
}

// k_dnet: the HashGrid's paired encoding straight into one fused kernel per pass; the encoding's steps are Enc's
DNetLaunch dnet_args(const NeusModule* m, const void* params, const uint32_t* enc) {
	DNetLaunch d{};
	d.w0 = (const half_t*)params; d.w1 = d.w0 + (size_t)m->ff.W * m->ff.in_pad; d.enc = enc;
	return d;
}
// NetworkWithInputEncoding::forward (network_with_input_encoding.h:84-111): encoding, then the MLP on it
void dnet_forward(NeusModule* m, hipStream_t s, uint32_t n, const float* input, void* output, const void* params, NeusContext* ctx) {
	uint32_t* enc = m->enc.paired_out(ctx, n);
	m->enc.hash_encode(s, n, input, (const half_t*)m->enc_params(params), ctx, enc);
	DNetLaunch d = dnet_args(m, params, enc);
	d.out = (half_t*)output;
	launch_dnet(s, m->enc.L(), m->ff.W, 0, n, d);
}
// NetworkWithInputEncoding::backward (network_with_input_encoding.h:113-156): the MLP backward gives its weight gradients
// and dL/d(encoding); the encoding's backward the grid gradients and dL_dinput
void dnet_backward(NeusModule* m, hipStream_t s, uint32_t n, const NeusContext* ctx, const float* input, const void* dL_doutput, const void* params,
                   float* g, float* dL_dinput) {
	Enc& e = m->enc;
	if (!params) throw std::runtime_error("module: null params");
	if (!m->ctx_ok(ctx)) throw std::runtime_error("module backward: the context is not from this module's forward");
	DNetLaunch d = dnet_args(m, params, ctx->enc.p);
	d.dL = (const half_t*)dL_doutput; d.denc = e.denc_tmp.p; d.wpartial = m->fw.partial.p;
	launch_dnet(s, e.L(), m->ff.W, 1, n, d);
	const half_t* denc = (const half_t*)e.denc_tmp.p;
	if (g) {
		ff_reduce(m->ff, m->fw, s, dnet_blocks(n), g);
		e.hash_scatter(s, n, input, denc, e.zero_h.p, e.zero_v.p, g + m->enc_off);
	}
	if (dL_dinput) launch_enc_input_grad(s, n, n, e.L(), denc, ctx->dydx.p, dL_dinput, 3);
}
// NetworkWithInputEncoding::backward_backward_input (network_with_input_encoding.h:159-250): u = dy/dx . dL_ddLdinput
// (kernel_grid_backward_input_backward_dLdoutput), the MLP's backward-backward (fully_fused_mlp.cu:1088-1198: b2 =
// relu'(H0) W1^T dL, h1' = relu'(H0) W0 u; dW0 = b2 u^T, dW1 = dL h1'^T) and the encoding's second-order grid
// gradient with dL/d(encoding) = W0^T b2. dL_ddLdoutput = W1 h1' (one more MFMA of the fused kernel); dL_dinput = the
// HashGrid's second derivative in x (k_grid_ddx) with dL/d(encoding) as its dL_doutput.
void dnet_bbi(NeusModule* m, hipStream_t s, uint32_t n, const NeusContext* ctx, const float* input, const float* u, const void* dL_doutput,
              const void* params, float* g, void* dL_ddLdoutput, float* dL_dinput) {
	Enc& e = m->enc;
	launch_enc_ddLdoutput(s, n, n, e.L(), u, ctx->dydx.p, (half_t*)e.u_tmp.p, e.v4.p);
	DNetLaunch d = dnet_args(m, params, ctx->enc.p);
	d.dL = (const half_t*)dL_doutput; d.u = e.u_tmp.p; d.denc = e.denc_tmp.p; d.wpartial = m->fw.partial.p; d.out = (half_t*)dL_ddLdoutput;
	launch_dnet(s, e.L(), m->ff.W, 2, n, d);
	const half_t* denc = (const half_t*)e.denc_tmp.p;
	if (g) {
		ff_reduce(m->ff, m->fw, s, dnet_blocks(n), g);
		e.hash_scatter(s, n, input, e.zero_h.p, denc, e.v4.p, g + m->enc_off);
	}
	if (dL_dinput) e.hash_ddx(s, n, input, (const half_t*)m->enc_params(params), denc, u, dL_dinput);
}
}  // namespace

// ---------------------------------------------------------------- the calls
// NetworkWithInputEncoding::forward (network_with_input_encoding.h:113-124): the encoding, straight into the FullyFusedMLP's
// fp16 input rows where there is a network, then its layers
static void module_forward(NeusModule* m, void* stream, uint32_t n, const float* input, void* output, const void* params, NeusContext* ctx) {
	if (!input || !output) throw std::runtime_error("module forward: null input / output");
	if (!params && m->P) throw std::runtime_error("module: null params");
	m->check_n(n, false);
	HIP_CHECK(hipSetDevice(m->core->device));
	StreamSwap sw(*m->core, stream);
	hipStream_t s = m->core->stream;
	if (m->fused == NeusModule::Nerf) nerf_forward(m, s, n, input, output, params);
	else if (m->fused == NeusModule::Dnet) dnet_forward(m, s, n, input, output, params, ctx);
	else {
		const FfNet& f = m->ff;
		const bool net = m->net();
		half_t* acts = m->fw.acts.p;
		if (net && ctx) { ctx->acts.alloc(std::max<size_t>(1, f.acts_halves(n))); acts = ctx->acts.p; }
		if (net && ctx && f.sine()) ctx->cosz.alloc(std::max<size_t>(1, (size_t)n * f.N * f.W));
		m->enc.encode(s, n, input, m->enc_params(params), ctx, net ? enc_io(acts, f.in_pad) : enc_io(output, 0));
		if (net) ff_forward(f, s, n, params, acts, (half_t*)output, ctx ? ctx->cosz.p : nullptr);
	}
	HIP_CHECK(hipGetLastError());
}

int neus_module_inference(NeusModule* m, void* stream, uint32_t n, const float* input, void* output, const void* params) {
	return guard([&] { module_forward(m, stream, n, input, output, params, nullptr); });
}

int neus_module_forward(NeusModule* m, void* stream, uint32_t n, const float* input, void* output, const void* params,
                        int prepare_input_gradients, NeusContext** ctx_out) {
	return guard([&] {
		if (!ctx_out) throw std::runtime_error("neus_module_forward: null context output");
		auto ctx = std::make_unique<NeusContext>();
		ctx->n = n;
		// the NerfNetwork's backward recomputes its forward; the HashGrid keeps dy/dx for dL_dinput and second order, the
		// network its activations
		(void)prepare_input_gradients;
		module_forward(m, stream, n, input, output, params, ctx.get());
		*ctx_out = ctx.release();
	});
}

// NetworkWithInputEncoding::backward (network_with_input_encoding.h:126-156): the FullyFusedMLP's backward (weight
// gradients, dL/dX0 as fp16 rows), then the encoding's backward of that (its parameter gradient, dL_dinput)
int neus_module_backward(NeusModule* m, void* stream, const NeusContext* ctx, uint32_t n, float* dL_dinput, const void* dL_doutput,
                         void* dL_dparams, const float* input, const void* output, const void* params, int gradient_mode) {
	return guard([&] {
		if (!ctx || ctx->n != n) throw std::runtime_error("module backward: the context is not from a forward over n_elements");
		if (!input || !dL_doutput) throw std::runtime_error("module backward: null input / dL_doutput");
		m->check_n(n, true);
		HIP_CHECK(hipSetDevice(m->core->device));
		StreamSwap sw(*m->core, stream);
		hipStream_t s = m->core->stream;
		float* g = m->grad_target(dL_dparams, gradient_mode);
		if (!g && !dL_dinput) return;
		if (m->fused == NeusModule::Nerf) nerf_backward(m, s, n, input, dL_doutput, params, g, dL_dinput);
		else if (m->fused == NeusModule::Dnet) dnet_backward(m, s, n, ctx, input, dL_doutput, params, g, dL_dinput);
		else {
			const FfNet& f = m->ff;
			const bool net = m->net();
			if (net) {
				if (!params) throw std::runtime_error("module: null params");
				if (!ctx->acts.p || (f.sine() && !ctx->cosz.p)) throw std::runtime_error("module backward: the context is not from this module's forward");
				if (f.out_act != FF_NONE && !output) throw std::runtime_error("FullyFusedMLP backward: the forward output is needed for its output activation");
			}
			m->enc.check_backward(ctx, params, dL_dinput, !net);
			EncIO dy = enc_io(dL_doutput, 0);
			if (net)
				dy = enc_io(ff_backward_chain(f, m->fw, s, n, params, ctx->acts.p, ctx->cosz.p, (const half_t*)dL_doutput, (const half_t*)output, g != nullptr,
				                              m->enc.sink(dL_dinput)), f.in_pad);
			m->enc.backward(s, n, ctx, input, dy, m->enc_params(params), g && m->enc.n_params() ? g + m->enc_off : nullptr, dL_dinput);
		}
		m->finish_grad(g, n, dL_dparams, gradient_mode, s);
		HIP_CHECK(hipGetLastError());
	});
}

// NetworkWithInputEncoding::backward_backward_input (network_with_input_encoding.h:159-250): (1) the network's backward
// gives dL/dX0 (parameter gradients ignored); (2) the encoding's backward_backward_input with it as dL_doutput: the
// second-order encoding gradient, J_enc dL_ddLdinput into the network's front rows, and dL_dinput, the encoding's own
// second-derivative term (the MLP's part is 0: act'' = 0); (3) the FullyFusedMLP's backward_backward_input on that front
// (fully_fused_mlp.cu:1088-1198): its weight gradients and dL_ddLdoutput = J_mlp J_enc dL_ddLdinput. A stand-alone
// encoding is step (2) alone on the caller's tensors.
// A network created with "second_order": "exact" whose hidden or output activation has a second derivative (FfNet::curved)
// runs the exact chain instead (ff_bbi_chain): step (1) starts from the output activation's delta, step (3) also runs when
// only dL_dinput is asked for and returns q = dS/dX0 along the forward path, and (4) the encoding's first-order backward of
// q is added to its parameter gradient and to dL_dinput (Enc::backward_curved; behind the Identity encoding layer 0 writes
// scale x q itself). The fp16 HashGrid's scatter waits for q and takes both cotangents in its one call.
int neus_module_backward_backward_input(NeusModule* m, void* stream, const NeusContext* ctx, uint32_t n, const float* dL_ddLdinput,
                                        const float* input, const void* dL_doutput, void* dL_dparams, void* dL_ddLdoutput, float* dL_dinput,
                                        const void* params, int gradient_mode) {
	return guard([&] {
		if (m->fused == NeusModule::Nerf)
			throw std::runtime_error("NerfNetwork: the eikonal second-order term is part of backward (nerf_network.h:330-601); "
			                         "backward_backward_input is provided by the HashGrid and network-with-input-encoding modules "
			                         "(the reference's NerfNetwork does not implement it either: object.h:222-232)");
		if (!ctx || ctx->n != n || !m->ctx_ok(ctx))
			throw std::runtime_error(std::string("backward_backward_input: needs the forward's context") + (!m->ff.P && m->enc.keeps_dydx() ? " (dy/dx)" : ""));
		if (!dL_ddLdinput || !m->enc.bbi_args(input, dL_doutput, params, dL_dinput) || (m->ff.P && (!dL_doutput || !params)))
			throw std::runtime_error("backward_backward_input: null input");
		m->check_n(n, true);
		m->check_bbi_exact(dL_ddLdoutput, dL_dinput);
		m->enc.check_bbi_sh(dL_dinput);
		HIP_CHECK(hipSetDevice(m->core->device));
		StreamSwap sw(*m->core, stream);
		hipStream_t s = m->core->stream;
		float* g = m->grad_target(dL_dparams, gradient_mode);
		if (!g && !dL_ddLdoutput && !dL_dinput) return;
		if (m->fused == NeusModule::Dnet) dnet_bbi(m, s, n, ctx, input, dL_ddLdinput, dL_doutput, params, g, dL_ddLdoutput, dL_dinput);
		else {
			const FfNet& f = m->ff;
			const bool net = m->net();
			float* ge = g && m->enc.n_params() ? g + m->enc_off : nullptr;
			EncIO dy = enc_io(dL_doutput, 0), Ju = enc_io(dL_ddLdoutput, 0);
			const bool curved = net && f.curved();  // act'' terms: dL_dinput needs the fronts too, and the chain's q the encoding's backward
			if (net) {
				dy = enc_io(nullptr, f.in_pad);
				// the default chain has no forward output to take the output activation's delta from (the call does not receive it)
				if (!curved && f.out_act != FF_NONE && m->enc.bbi_reads_dy(ge, dL_dinput))
					throw std::runtime_error("backward_backward_input: an output activation other than None behind this encoding needs the network's "
					                         "\"second_order\": \"exact\" (the default chain has no forward output for its backward)");
				if (curved && f.out_act != FF_NONE) ff_output(f, s, n, params, ctx->acts.p, m->fw.y.p);
				if (m->enc.bbi_reads_dy(ge, dL_dinput))
					dy.p = const_cast<half_t*>(ff_backward_chain(f, m->fw, s, n, params, ctx->acts.p, ctx->cosz.p, (const half_t*)dL_doutput, curved ? m->fw.y.p : nullptr,
					                                             false, FfSink{false, nullptr, 1.f}));
				Ju = enc_io(g || dL_ddLdoutput || (curved && dL_dinput) ? m->fw.front.p : nullptr, f.in_pad);
			}
			m->enc.backward_backward(s, n, ctx, input, dL_ddLdinput, dy, m->enc_params(params), ge, Ju, dL_dinput, curved);
			if (net && Ju.p) {
				const half_t* q = ff_bbi_chain(f, m->fw, s, n, params, ctx->acts.p, ctx->cosz.p, (const half_t*)dL_doutput, g != nullptr, (half_t*)dL_ddLdoutput,
				                               ge || dL_dinput, m->enc.sink(dL_dinput));
				if (q) m->enc.backward_curved(s, n, ctx, input, enc_io(q, f.in_pad), m->enc_params(params), ge, dL_dinput);
			}
		}
		m->finish_grad(g, n, dL_dparams, gradient_mode, s);
		HIP_CHECK(hipGetLastError());
	});
}

extern "C" {

// Rendering operators (volrend.hip): stateless, on the caller's stream; the launchers validate and throw.
int neus_volrend_march_count(void* stream, uint32_t n_rays, const float* rays_o, const float* rays_d, const float* t_min, const float* t_max,
                             const uint8_t* occupancy, uint32_t grid, float dt, uint32_t max_per_ray, int32_t* counts) {
	return guard([&] { launch_volrend_march_count((hipStream_t)stream, n_rays, rays_o, rays_d, t_min, t_max, occupancy, grid, dt, max_per_ray, counts); });
}
int neus_volrend_march_write(void* stream, uint32_t n_rays, const float* rays_o, const float* rays_d, const float* t_min, const float* t_max,
                             const uint8_t* occupancy, uint32_t grid, float dt, uint32_t max_per_ray, const int32_t* ranges, uint32_t n_samples,
                             float* t, int32_t* ray_idx) {
	return guard([&] { launch_volrend_march_write((hipStream_t)stream, n_rays, rays_o, rays_d, t_min, t_max, occupancy, grid, dt, max_per_ray, ranges, n_samples, t, ray_idx); });
}
int neus_volrend_alpha_forward(void* stream, uint32_t n, const float* sdf, const float* true_cos, const float* dt, float dt_value,
                               const float* inv_s, float inv_s_value, float cos_anneal_ratio, float* alpha) {
	return guard([&] { launch_volrend_alpha_forward((hipStream_t)stream, n, sdf, true_cos, dt, dt_value, inv_s, inv_s_value, cos_anneal_ratio, alpha); });
}
int neus_volrend_alpha_backward(void* stream, uint32_t n, const float* sdf, const float* true_cos, const float* dt, float dt_value,
                                const float* inv_s, float inv_s_value, float cos_anneal_ratio, const float* g_alpha, float* g_sdf,
                                float* g_true_cos, double* partials, uint32_t n_partials, float* g_inv_s) {
	return guard([&] {
		launch_volrend_alpha_backward((hipStream_t)stream, n, sdf, true_cos, dt, dt_value, inv_s, inv_s_value, cos_anneal_ratio, g_alpha, g_sdf, g_true_cos,
		                              partials, n_partials, g_inv_s);
	});
}
int neus_volrend_composite_forward(void* stream, uint32_t n_rays, uint32_t n_samples, uint32_t n_channels, const float* alpha, const float* values,
                                   const int32_t* ranges, float t_stop, float* out, float* opacity, float* weights, float* trans, int32_t* n_composited) {
	return guard([&] {
		launch_volrend_composite_forward((hipStream_t)stream, n_rays, n_samples, n_channels, alpha, values, ranges, t_stop, out, opacity, weights, trans, n_composited);
	});
}
int neus_volrend_composite_backward(void* stream, uint32_t n_rays, uint32_t n_samples, uint32_t n_channels, const float* alpha, const float* values,
                                    const int32_t* ranges, const float* trans, const int32_t* n_composited, const float* g_out,
                                    const float* g_opacity, const float* g_weights, float* g_alpha, float* g_values) {
	return guard([&] {
		launch_volrend_composite_backward((hipStream_t)stream, n_rays, n_samples, n_channels, alpha, values, ranges, trans, n_composited, g_out, g_opacity,
		                                  g_weights, g_alpha, g_values);
	});
}

} // extern "C"
