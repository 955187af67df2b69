// Host orchestration of the NeuS2 training hot path on gfx950 and the testbed part of the C-ABI (include/neus2_hip.h):
// every entry point that takes a NeusTestbed and the debug hooks. The operator modules and the rendering operators are
// in operators.cpp, which uses a testbed only through the functions of core.h, defined here. The data-parallel exchange
// (transports, exchange stream, all-reduces, the groups' entry points) is neus::Exchange, exchange.h: the step here
// decides when and what is exchanged.
//
// NeusTestbed restates the training-relevant part of the reference Testbed
// (include/neural-graphics-primitives/testbed.h:63-940; src/testbed.cu:2084-2349, 2640-2736;
// src/testbed_nerf.cu:3293-3548, 3723-4016) MI355X-first:
//   * one HIP stream per testbed, every counter device-resident (no host sync inside a step);
//   * deterministic count -> scan -> write compaction instead of atomic appends;
//   * fp32 gradients and master weights, fp16 weights for the kernels (the reference keeps fp16
//     gradients), RCCL all-reduce of the gradient buffer for data parallelism over ray batches.
#include <rocprofiler-sdk-roctx/roctx.h>
#include "kernels.h"
#include "scan_lookback.h"
#include "json_lite.h"
#include "options.h"
#include "step_plan.h"
#include "host_util.h"
#include "exchange.h"
#include "core.h"
#include "../../include/neus2_hip.h"

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <functional>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>

using namespace neus;

namespace {

thread_local std::string g_err;

// Debug (options.h NeusAllocDebug): the fill / the listing of the fresh device allocations, numbered from the last
// neus_testbed_create, where the pair is latched for the process
std::atomic<uint64_t> g_alloc_seq{0}, g_alloc_base{0};
NeusAllocDebug g_alloc_dbg;

// Every owner of a HIP resource is single: none copies (a copy would release twice); the handles move without throwing,
// the device buffers do not move at all (nothing needs it)
template <class T> constexpr bool no_copy = !std::is_copy_constructible_v<T> && !std::is_copy_assignable_v<T>;
static_assert(no_copy<Dev<float>> && no_copy<ScanTemp> && no_copy<Stream> && no_copy<Event> && no_copy<Pinned<float>>);
static_assert(std::is_nothrow_move_constructible_v<Stream> && std::is_nothrow_move_constructible_v<Event> &&
              std::is_nothrow_move_constructible_v<Pinned<float>>);

} // namespace

void neus::set_last_error(const char* what) { g_err = what; }
void neus::dbg_poison(void* p, size_t bytes) {
	const uint64_t k = g_alloc_seq++ - g_alloc_base.load();
	const NeusAllocDebug& d = g_alloc_dbg;
	if (d.log) std::fprintf(stderr, "neus alloc %llu %zu\n", (unsigned long long)k, bytes);
	if (d.poison && k >= d.lo && k < d.hi) HIP_CHECK(hipMemset(p, (int)d.byte, bytes));
}

namespace {

constexpr uint32_t MAX_RAYS = 1u << 18;  // testbed_nerf.cu:3435 cap on rays_per_batch
constexpr float LOSS_SCALE = 128.f;      // testbed.h:246

// ld_random_pixel_offset (random_val.cuh:254-288, 317-322): scrambled Sobol 2-D value of the spp index,
// offset = fract(0.5 - v(0) + v(spp)). Sobol dimension 0 is the bit reversal; dimension 1 has direction
// numbers d[0] = 2^31, d[b] = d[b-1] ^ (d[b-1] >> 1).
uint32_t rev_bits(uint32_t x) {
	x = ((x & 0xaaaaaaaau) >> 1) | ((x & 0x55555555u) << 1); x = ((x & 0xccccccccu) >> 2) | ((x & 0x33333333u) << 2);
	x = ((x & 0xf0f0f0f0u) >> 4) | ((x & 0x0f0f0f0fu) << 4); x = ((x & 0xff00ff00u) >> 8) | ((x & 0x00ff00ffu) << 8);
	return (x >> 16) | (x << 16);
}
uint32_t nus_scramble(uint32_t x, uint32_t seed) {
	x = rev_bits(x);
	x += seed; x ^= x * 0x6c50b47cu; x ^= x * 0xb82f1e52u; x ^= x * 0xc7afe638u; x ^= x * 0x8d22f6e6u;
	return rev_bits(x);
}
uint32_t sobol_dim(uint32_t index, uint32_t dim) {
	uint32_t X = 0, d = 0x80000000u;
	for (uint32_t bit = 0; bit < 32; ++bit) {
		const uint32_t dir = dim == 0 ? (0x80000000u >> bit) : d;
		if ((index >> bit) & 1) X ^= dir;
		d ^= d >> 1;
	}
	return X;
}
void ld_random_val_2d(uint32_t index, uint32_t seed, float out[2]) {
	const float S = float(1.0 / 4294967296.0);
	index = nus_scramble(index, seed);
	for (uint32_t i = 0; i < 2; ++i) out[i] = (float)nus_scramble(sobol_dim(index, i), seed ^ (i + (seed << 6) + (seed >> 2))) * S;
}
void ld_pixel_offset(uint32_t spp, float out[2]) {
	float a[2], b[2];
	ld_random_val_2d(0, 0xdeadbeefu, a);
	ld_random_val_2d(spp, 0xdeadbeefu, b);
	for (int k = 0; k < 2; ++k) { const float v = (0.5f - a[k]) + b[k]; out[k] = v - std::floor(v); }
}

} // namespace

struct NeusTestbed {
	const NeusOptions opt = NeusOptions::from_env();  // the NEUS_* switches, read once: they hold for the testbed's life
	int device = 0;
	// The current stream: the testbed's own (stream_own) except while a module call runs on its caller's (operators.cpp
	// StreamSwap writes it through Core::stream); only stream_own is ever drained for good or destroyed
	Stream stream_own;
	hipStream_t stream = nullptr;
	// side stream of the backward: the weight-gradient GEMM runs there beside the grid scatter (disjoint inputs and
	// outputs; both deterministic), forked from and joined back into the step's stream by events
	Stream aux_stream;
	Event ev_fork, ev_join;
	// Lookahead (opt.lookahead): the next step's ray sampling (ray generation, march, march write, ray sort) issued on
	// la_stream behind this step's counters (their stream: the step's, or the exchange stream with a group), beside its
	// backward and optimizer, which read none of its outputs. At any world size; only between steps of one
	// neus_testbed_train call (nothing pending between calls); which steps look ahead: step_plan.h StepPlan::la_go.
	// opt.adam_overlap: the step's Adam parameters; next: the first parameter not issued; on: the exchange stream the pieces
	// follow their ranges' all-reduces on (data parallel), or null (one rank: ad_stream, behind the step's stream)
	struct AdamSplit { AdamParams p; uint32_t next; hipStream_t on; };
	bool la_pending = false, la_next_in_call = false;
	uint64_t la_steps = 0, adam_split_steps = 0;  // (stats: lookahead_steps, adam_split_steps)
	// Where in the backward the pending lookahead is issued (one rank; with a group it goes out with the counters'
	// exchange): 0 right after the loss, 1 after the training encode, 2 after the training MLP kernels, 3 after the
	// weight-gradient reduction, 4 after the scatter. A cut march's sampling is small and goes after the encode, where it no
	// longer shares the gather-bound encode (opt.la_at_cut); a full march goes right after the loss (opt.la_at_full).
	int la_at = 0;
	std::function<void()> la_deferred;
	void la_fire(int at) {
		if (la_deferred && at >= la_at) { auto f = std::move(la_deferred); la_deferred = nullptr; f(); }
	}
	int main_prio = 0;  // the step's streams' priority (0: created without one; the communication stream follows it)
	Stream la_stream;
	Event ev_la_start, ev_la_done;
	// development (NEUS_LA_STAT=1): per lookahead, timing events around its sampling (la stream) and around the next
	// step's wait for it (main stream); summed and printed at the end of each neus_testbed_train call
	std::vector<Event> la_stat_ev;
	size_t la_stat_used = 0;
	hipEvent_t la_stat_next() {
		if (la_stat_used == la_stat_ev.size()) la_stat_ev.push_back(make_event());
		return la_stat_ev[la_stat_used++].get();
	}
	void la_stat_report() {
		if (la_stat_used < 4) { la_stat_used = 0; return; }
		HIP_CHECK(hipDeviceSynchronize());
		// groups of 4: la begin, la end (previous step), wait begin, wait end (this step)
		double wait = 0, dur = 0, slack = 0;
		size_t n = 0;
		for (size_t k = 0; k + 4 <= la_stat_used; k += 4, ++n) {
			float a = 0, b = 0, c = 0;
			HIP_CHECK(hipEventElapsedTime(&a, la_stat_ev[k + 2].get(), la_stat_ev[k + 3].get()));
			HIP_CHECK(hipEventElapsedTime(&b, la_stat_ev[k].get(), la_stat_ev[k + 1].get()));
			HIP_CHECK(hipEventElapsedTime(&c, la_stat_ev[k + 1].get(), la_stat_ev[k + 2].get()));
			wait += a; dur += b; slack += c;
		}
		std::fprintf(stderr, "la_stat n=%zu wait_us=%.1f sampling_us=%.1f slack_us=%.1f\n", n, 1e3 * wait / n, 1e3 * dur / n, 1e3 * slack / n);
		la_stat_used = 0;
	}
	NeusNetworkConfig cfg{};
	bool have_net = false, have_data = false;
	Layout lay{};
	GridLevels gl{};
	// dataset
	Dev<uint32_t> pixels; Dev<uint64_t> pix_off; Dev<int32_t> res; Dev<float> focal, pp, xform;
	DevDataset ds{};
	Dev<float> srgb_lut;  // read_rgba's byte -> linear table
	std::vector<float> host_focal, host_pp, host_xform;
	std::vector<int32_t> host_res;
	uint32_t max_cascade = 0;
	float aabb_scale = 1.f;
	// parameters
	Dev<float> params_fp, grads, m1, m2, ema_tmp;
	// per-parameter Adam steps: u16 [P] saturating at 65535 while the bias table is converged (optim.hip AdamSteps), else
	// u32 [P] (steps32); P x 4 B either way
	Dev<uint32_t> adam_steps;
	bool steps32 = false;
	Dev<half_t> params_h, ema_h, wT;
	MlpPtrs mlp{};
	DinPerm din_perm{};
	// inference params (EMA weights, the reference's Ema::custom_weights) for rendering
	Dev<half_t> wT_ema;
	// The fp16 EMA (inference) weights are only read outside the training step (render, SDF grid, mesh colours, snapshots,
	// the frame restart), so the step updates the fp32 EMA alone and the fp16 copy is cast from it when first read: the
	// same bits the Adam kernel would have written (ema_h = half(ema_tmp) after every step), 2 B per parameter less per step
	bool ema_h_stale = false;
	void sync_ema_h() {
		if (!ema_h_stale) return;
		launch_cast_half(stream, lay.P, ema_tmp.p, ema_h.p);
		HIP_CHECK(hipGetLastError());
		HIP_CHECK(hipStreamSynchronize(stream));  // (readers may use another stream or the host)
		ema_h_stale = false;
	}
	MlpPtrs mlp_ema{};
	// renderer workspace (NerfTracer, testbed_nerf.cu:2397-2630)
	Dev<uint8_t> r_rays[2];
	ScanTemp r_scan_tmp;
	Dev<uint32_t> r_flags, r_base, r_alive;
	Dev<float> r_coords, r_coords_def;
	Dev<half_t> r_out;
	Dev<float4> r_frame, r_accum;
	size_t r_scan_bytes = 0;
	// marching cubes workspace and the last mesh (Testbed::m_mesh, testbed.h:596-610)
	Dev<float> mc_density, mesh_v;
	Dev<uint32_t> mc_vidx, mc_cnt, mesh_f;
	ScanTemp mc_scan_tmp;
	size_t mc_scan_bytes = 0;
	uint32_t mesh_nv = 0, mesh_nt = 0;
	// dynamic scenes (testbed.h:455-477, 889-890): frame, phase flags, the DeltaNetwork state on the device,
	// deformed copies of the sample coordinates, dL/d(position) of the training batch
	uint32_t cur_frame = 0, canonical_step = 0, delta_step = 0;
	bool train_canonical = true, train_delta = false;
	bool nonfinite = false, aborted = false;  // training health (consume_loss); cleared by reset_network
	bool render_delta = false;     // prepare_for_test (testbed.cu:1987-1999): render / mesh through the DeltaNetwork
	float near_distance = 0.f;     // nerf.training.near_distance: stored; the NeuS sampler does not read it (testbed_nerf.cu:1525)
	// nerf.training.depth_supervision_lambda (testbed.h:649): stored. The reference's loss kernel computes the depth term
	// (testbed_nerf.cu:1697-1698, 1836) but adds it to no gradient and no loss output, so it never changes training; the
	// step here keeps that (no depth term; tests/test_gpu_depth.py checks a lambda > 0 run against lambda = 0 bitwise)
	float depth_lambda = 0.f;
	int32_t color_space_when_linear = 0;  // color_space as set while linear_colors overrides it
	float delta_lr_factor = 1.f;
	Dev<DeltaState> delta;
	Dev<float> delta_partial, coords_def, coords_cdef;
	Dev<float4> dpos;
	// occupancy grid
	Dev<float> density_grid, density_tmp, grid_mean, grid_partial, occ_pos, occ_density;
	Dev<uint32_t> occ_idx;
	Dev<uint32_t> occ_ulist;  // the cell-ordered uniform samples, OccSampling::ulist
	Dev<uint8_t> bitfield;
	Dev<uint32_t> bf_lin;   // mip-0 occupancy in (x, y, z/32) word order for the constant-step march
	Dev<float> occ_bbox;    // world box of the occupied cells of every mip (+ stage-1 scratch): the ray generation's cull
	Dev<float> adam_bias;   // Adam bias-correction table (AdamParams::bias_tab) for betas bias_b1 / bias_b2
	float bias_b1 = -1.f, bias_b2 = -1.f;
	bool bias_conv = false;
	Dev<uint32_t> dbg_enc;  // debug timing only (neus_debug_time_kernel 11): [L][16 Nc] encodings of the inference samples
	uint32_t dbg_lds_fill = 0;  // tests (neus_debug_set_lds_fill): garbage-fill every CU's LDS before the step's march write
	Dev<float> dbg_co; Dev<half_t> dbg_dl;
	static constexpr int DBG_SNAP_N = 15;
	Dev<uint8_t> dbg_snap[DBG_SNAP_N];  // the loss-gradient inputs right after its launch (ids 0..14 of neus_debug_get_buffer)
	uint32_t dbg_lds_fill_all = 0;  // tests (neus_debug_set_lds_fill_all): ... before every kernel of the step (g_dbg_lds_fill)
	uint32_t dbg_xcd_shift = 0;     // tests (neus_debug_set_xcd_shift): workgroups of a no-op kernel before every kernel of the step
	Dev<PcgJump> pcg_tab;   // pcg32 jump-ahead table (common.h PcgJumpTable)
	uint32_t density_grid_ema_step = 0;
	uint64_t occ_samples = 0;  // occupancy-grid samples this rank evaluated since the network was loaded
	uint32_t occ_updates = 0;
	// step workspace
	uint32_t batch = 0, max_samples = 0;
	Dev<float> rays, startt, coords, coords_c, loss, ek, mask, loss_sum;
	Dev<uint32_t> health_buf;  // [0] march fail flags, [1] scan give-ups (all-reduced at every loss readback); [2..3] setting checks
	Dev<uint32_t> nreq, base, numsteps, ccount, cbase, enc, march_nrec, march_queue;
	Dev<uint2> march_rec, march_seg;
	MarchWork mwork{};
	Dev<float> dydx;
	Dev<half_t> net_out, dL_dout, trainbuf;
	Dev<float4> vbuf;
	Dev<float> wgrad_partial, var_partial;  // per-block MLP weight-gradient rows, per-block variance sums
	uint32_t mlp_blocks = 0;                // grid of the training MLP kernels at the batch capacity
	ScanTemp scan_tmp, scan_tmp_la;  // (scan_tmp_la: the lookahead's march scans, on la_stream)
	size_t scan_tmp_bytes = 0;
	Dev<StepState> st;
	ScatterWork swork{};
	Dev<uint32_t> sc_counts, sc_offs, sc_jobs, sc_split_done;
	Dev<unsigned long long> sc_split;
	std::vector<uint32_t> sc_jobs_before;  // [n_buckets + 1] accumulation jobs of the buckets below b
	uint32_t sc_zero_from = 0;             // the grads' grid part is known zero from this bucket on
	Dev<uint32_t> sc_jobs2;
	Dev<uint16_t> sc_rtab;
	std::vector<uint32_t> sc_jobs2_before;  // [L + 1] region-scatter jobs of the levels below l
	uint32_t sc_zero_from_e = 0;            // region scatter: grid entries from here on hold zero gradients
	Dev<h2> sc_rec_g;
	Dev<uint16_t> sc_rec_i;
	// restructured loss scratch (kernels.h LossWork)
	Dev<float4> l_sa, l_ck4, l_racc, l_rgr;
	Dev<float> l_ekt, l_cke, l_rT, l_rek;
	Dev<uint32_t> sample_ray;
	Dev<uint32_t> cmap;  // compacted sample -> ray (LossWork::cmap)
	// progressive (cut-off-aware) inference: its mode, the rounds' chunk ends and the rule that chooses them (step_plan.h)
	ChunkSchedule sched{opt};
	Dev<uint32_t> chunk_list, chunk_cnt;  // chunk_cnt: [k] round k's sample list length, [16] the long-ray list's, [32 + k] open rays
	Dev<uint32_t> open_rays[2];          // the rays still open after a round (ping-pong: round k reads [(k - 1) & 1])
	// spatial ray order of the progressive rounds (RaySort; without opt.ray_sort: slot order, one-XCD-agnostic lists)
	Dev<uint32_t> rs_hist, rs_off, rs_perm;
	Dev<uint16_t> rs_key;
	static constexpr uint32_t OPEN_CNT = 32;
	static constexpr uint32_t RS_N_PERM = 48;  // chunk_cnt slot: the ray order's length (k_ray_sort_scan)
	static constexpr uint32_t RAW_CNT = 49;    // chunk_cnt [49 + k]: rays open after round k, before the compaction cut (k = 0)
	// The compaction cut (march.hip k_prog_cut): with fixed rays per batch the later progressive rounds skip the rays whose
	// compaction base is already past the batch after a round. Training is bitwise the same; what changes is the summed
	// composited count of such a step (a lower bound, still >= the batch), which with fixed rays feeds no result - only the
	// logged loss scale, the chunk-end rule and the stats. Which steps cut: step_plan.h plan_sampling (none that the host
	// reads back, so every value the host sees is the uncut one).
	// With the spatial ray order, round 0 itself is split too: the sort puts the rays of the slots below the previous step's
	// cut (+ 1/4, + 1024: cutw[CW_EST]) first (pass A); once pass A is scanned the cut is known whenever the prefix reaches
	// the batch in those slots, and pass B (the rest of round 0) then has nothing to do.
	Dev<uint32_t> open_raw, cutw;  // the rays open after round 0, before the cut; the cut words (kernels.h CW_*)
	uint64_t cut_steps = 0;
	uint32_t call_left = 0;        // steps of the current train call after the current one
	SamplingPlan la_plan;          // the sampling the pending lookahead issued: the next step's, which uses it whole
	// The march cut: on a cut step the compaction cut lies, nearly always, well inside the slots below the
	// split estimate (cutw[CW_EST]: at the bench's step 800, 5.6 K of the 41 K kept slots), and no ray past it contributes a
	// training sample. So such a step generates and marches only those slots (MarchWork::est_cut). Two things make that
	// step's training differ from the full march's, and k_loss_ray checks both (the witness): the marched slots may not
	// fill the batch, and - on the step after - the reference's cap on the pre-compaction samples (max_inference, from the
	// cut step's requested count) is then known only to be at least the marched slots' count, so a contributing ray past
	// that bound might have been dropped there. Either sets StepState::cut_abort (all-reduced with the step's counters):
	// the optimizer and the step counters of that step then change nothing, the host sees the word before it queues the
	// next step, restores its own state to the step's start and runs the step again with the full march (after recounting
	// the step before it in full when that one was cut, which makes its cap exact). The trained parameters are those of
	// the full march in every case. Which steps cut the march: step_plan.h plan_sampling (chosen so that the loss readback
	// and the end of a call need no extra wait).
	bool force_full = false;      // the step being re-run marches every slot
	Dev<uint32_t> occ_nu_key, occ_nu_list, occ_nu_bins;  // opt.occ_nu_sort: the occupancy-biased samples binned by their coarse cell
	bool abort_direct = false;            // the last risky step's word comes through abort_word (one rank)
	Pinned<volatile uint32_t> abort_word;     // host-coherent pinned word k_loss_grad stores the witness to (one rank)
	bool mc_hist[2] = {false, false};  // the march of the last issued step / of the one before it was cut
	struct StepSnap {
		uint32_t training_step = 0, canonical_step = 0, adam_step = 0, call_left = 0;
		int enc_step = 0;
		float lr_factor = 1.f;
		pcg32 rng{};
		uint64_t la_steps = 0, cut_steps = 0, adam_split_steps = 0, mcut_steps = 0;
	};
	StepSnap snap[2];             // the host's step state at the start of the last issued step / of the one before it
	bool abort_pending = false;   // the last issued step's abort word is on its way to pinned[100] (ev_abort)
	Event ev_abort, ev_abort_src;
	uint64_t mcut_steps = 0, mcut_reruns = 0;
	Dev<StepState> st_recount;
	Dev<uint32_t> long_rays;  // the loss scan's wave-per-ray list (+ its counter in chunk_cnt[16])
	TrainBufs tbuf{};
	// RNG + counters (testbed.cu:2087-2101)
	pcg32 rng, density_grid_rng;
	uint32_t training_step = 0;
	uint32_t adam_step = 0;
	float lr_factor = 1.f;
	// the grid encoding's training step (GridEncoding::set_training_step, testbed.cu:2651-2657): set by every train
	// step (minus the global-movement steps on frames >= 1), 0 for a fresh network; render / SDF grid / mesh colours
	// use its progressive level, as the reference's inference does
	int enc_step = 0;
	// stats
	float loss_scalar_ema = 0.f, last_loss = 0.f, ek_loss = 0.f, mask_loss = 0.f, ray_loss = 0.f;
	uint32_t last_rays_with_samples = 0;
	bool loss_ema_init = false;
	Pinned<float> pinned;     // [0..3]: loss sum, ek sum, mask sum, grid mean; [32..47] render / mesh counts; [48]: the step scans'
	                          // give-up count; [64..]: StepState copy
	bool loss_pending = false;
	Event ev_loss;  // after the logged step's readback copies (consume_loss waits on it, not on the stream)
	// data parallel (exchange.h): the transport, this rank's place in it, the exchange stream, the all-reduces and their
	// counters; bound to the current stream and the step's priority
	Exchange x{stream, main_prio, opt.exchange_overlap};
	DPInfo dp_info() const { return DPInfo{x.rank(), x.world()}; }
	// One of the exchange's attaches (neus_testbed_init_*): the loss normalisation follows the world size the attach left,
	// also when it threw after setting it
	template <class F> void attach(F&& f) {
		struct Renorm { NeusTestbed* t; ~Renorm() { t->tbuf.indeed_batch = (float)t->batch * (float)t->x.world(); } } renorm{this};
		f();
	}
	static constexpr uint32_t X_GROUPS = 3;   // grid level groups of the overlapped exchange (~equal bytes at L=14)
	// level groups of the overlapped exchange: the active levels cut where the cumulative parameter count passes 1/3, 2/3
	ScatterSplit x_split(uint32_t valid, float* grid_grads) {
		ScatterSplit sp{};
		const uint32_t n_act = std::min(valid + 1, gl.n_levels);
		sp.n_groups = X_GROUPS;
		const uint64_t tot = gl.offset[n_act];
		uint32_t gi = 0;
		for (uint32_t l = 1; l < n_act && gi + 1 < X_GROUPS; ++l)
			if ((uint64_t)gl.offset[l] * X_GROUPS >= tot * (gi + 1)) sp.level_end[gi++] = l;
		for (; gi + 1 < X_GROUPS; ++gi) sp.level_end[gi] = n_act;
		sp.level_end[X_GROUPS - 1] = n_act;
		sp.done = [this, grid_grads](uint32_t lo, uint32_t hi) {
			hipStream_t xs = x.gated();
			x.allreduce_f32(grid_grads + 2 * (size_t)gl.offset[lo], 2 * (size_t)(gl.offset[hi] - gl.offset[lo]), false, xs);
		};
		return sp;
	}
	// profiling
	bool profiling = false;
	static constexpr int N_PHASES = NEUS_N_PHASES;
	// Two sets of phase events (steps alternate), so reading one step's timings never idles the GPU:
	// the step after it is already queued. The phase marks skip the system-scope release fence (it
	// writes back and invalidates the caches, which would slow the kernel after every mark).
	Event ev[2][N_PHASES + 1];
	Event ev_done[2];
	Pinned<StepState> prof_st;  // pinned, one StepState copy per event set
	bool prof_pending[2] = {false, false};
	int prof_par = 0;
	double phase_ms[N_PHASES] = {};
	double phase_npre = 0, phase_ntrain = 0;
	uint32_t phase_steps = 0;

	NeusTestbed(int dev) : device(dev) {
		HIP_CHECK(hipSetDevice(device));
		{
			// The step's streams at the highest priority, the lookahead's at the lowest (train_step). With the step's
			// streams at the default priority, a testbed created after another one was destroyed ran the 16-level bench leg
			// at 1.91 ms/step instead of 1.27 with the lookahead at the lowest priority (profiles/r05l16_priorities_ab.txt),
			// presumably from how the runtime maps the streams onto its few hardware queues; explicit priorities on every
			// stream keep it at 1.24. Without opt.main_prio: the default priority.
			int lo = 0, hi = 0;
			HIP_CHECK(hipDeviceGetStreamPriorityRange(&lo, &hi));
			main_prio = hi;
			if (opt.main_prio) {
				stream_own = make_stream(hipStreamNonBlocking, hi);
				aux_stream = make_stream(hipStreamNonBlocking, hi);
			} else {
				main_prio = 0;
				stream_own = make_stream(hipStreamNonBlocking);
				aux_stream = make_stream(hipStreamNonBlocking);
			}
			stream = stream_own.get();
		}
		ev_fork = make_event(hipEventDisableTiming);
		ev_join = make_event(hipEventDisableTiming);
		ev_loss = make_event(hipEventDisableTiming);
		pinned = make_pinned<float>(128);
		for (auto& set : ev)
			for (auto& e : set) e = make_event(hipEventDisableSystemFence);
		for (auto& e : ev_done) e = make_event();
		prof_st = make_pinned<StepState>(2);
		st.alloc(1);
		HIP_CHECK(hipMemset(st.p, 0, sizeof(StepState)));
		// pcg32 jump-ahead table of the streams this Testbed draws from (pcg32{seed} / pcg32{next_uint()}: increment 3)
		std::vector<PcgJump> jt(PCG_JUMP_LEVELS * PCG_JUMP_N);
		for (uint32_t j = 0; j < PCG_JUMP_LEVELS; ++j)
			for (uint32_t k = 0; k < PCG_JUMP_N; ++k) jt[j * PCG_JUMP_N + k] = pcg_jump(PCG_INC, (uint64_t)k << (j * PCG_JUMP_BITS));
		pcg_tab.alloc(jt.size());
		HIP_CHECK(hipMemcpy(pcg_tab.p, jt.data(), jt.size() * sizeof(PcgJump), hipMemcpyHostToDevice));
	}
	static constexpr uint64_t PCG_INC = 3u;  // make_pcg32(s) = pcg32 stream 1: inc = (1 << 1) | 1
	PcgJumpTable jump_table() const { return PcgJumpTable{pcg_tab.p, PCG_INC}; }
	~NeusTestbed() {
		// every stream of the testbed idle before anything is released: no queued work then reads an event, a pinned block or
		// a device buffer, so the members (Dev buffers included) may go in any order, before or after the streams
		for (hipStream_t q : {stream_own.get(), aux_stream.get(), la_stream.get(), x.stream()})
			if (q) (void)hipStreamSynchronize(q);
		x.release_comm();  // the communicator before any stream: it was issuing on the exchange stream or the step's
		// the streams in the order they have always gone back to the runtime (it is not neutral to that, see the
		// constructor): by these explicit resets, declaration order would give comm, la, aux, step
		aux_stream.reset(); la_stream.reset(); x.release_stream(); stream_own.reset();
	}

	// ------------------------------------------------------------ dataset (load_nerf, testbed_nerf.cu:2964-3095)
	void set_dataset(uint32_t n_images, const NeusImage* imgs, float aabb_scale_) {
		if (n_images == 0) throw std::runtime_error("set_dataset: no images");
		aabb_scale = aabb_scale_;
		const int s = (int)aabb_scale;
		if (s < 1 || (s & (s - 1)) != 0) throw std::runtime_error("NeRF dataset's `aabb_scale` must be a power of two");
		if (s > (1 << (NERF_CASCADES - 1))) throw std::runtime_error("NeRF dataset must have aabb_scale <= 128");
		std::vector<uint64_t> offs(n_images);
		std::vector<int32_t> r(2 * n_images);
		std::vector<float> f(2 * n_images), p(2 * n_images), x(12 * n_images);
		uint64_t total = 0;
		for (uint32_t i = 0; i < n_images; ++i) {
			offs[i] = total;
			total += (uint64_t)imgs[i].width * imgs[i].height;
			r[2 * i] = imgs[i].width; r[2 * i + 1] = imgs[i].height;
			f[2 * i] = imgs[i].focal[0]; f[2 * i + 1] = imgs[i].focal[1];
			p[2 * i] = imgs[i].principal[0]; p[2 * i + 1] = imgs[i].principal[1];
			std::memcpy(&x[12 * i], imgs[i].xform, 12 * sizeof(float));
		}
		pixels.alloc(total); pix_off.alloc(n_images); res.alloc(2 * n_images); focal.alloc(2 * n_images); pp.alloc(2 * n_images); xform.alloc(12 * n_images);
		for (uint32_t i = 0; i < n_images; ++i)
			HIP_CHECK(hipMemcpy(pixels.p + offs[i], imgs[i].rgba8, (size_t)imgs[i].width * imgs[i].height * 4, hipMemcpyHostToDevice));
		HIP_CHECK(hipMemcpy(pix_off.p, offs.data(), n_images * 8, hipMemcpyHostToDevice));
		HIP_CHECK(hipMemcpy(res.p, r.data(), r.size() * 4, hipMemcpyHostToDevice));
		HIP_CHECK(hipMemcpy(focal.p, f.data(), f.size() * 4, hipMemcpyHostToDevice));
		HIP_CHECK(hipMemcpy(pp.p, p.data(), p.size() * 4, hipMemcpyHostToDevice));
		HIP_CHECK(hipMemcpy(xform.p, x.data(), x.size() * 4, hipMemcpyHostToDevice));
		ds.pixels = pixels.p; ds.pix_off = pix_off.p; ds.res = res.p; ds.focal = focal.p; ds.pp = pp.p; ds.xform = xform.p;
		srgb_lut.alloc(256);
		launch_srgb_lut(stream, srgb_lut.p);
		HIP_CHECK(hipStreamSynchronize(stream));
		ds.lin_lut = srgb_lut.p;
		ds.n_images = n_images;
		host_focal = f; host_pp = p; host_xform = x; host_res = r;
		const float infl = 0.5f * (float)std::min(1 << (NERF_CASCADES - 1), s);
		for (int d = 0; d < 3; ++d) { ds.aabb_min[d] = 0.5f - infl; ds.aabb_max[d] = 0.5f + infl; }
		max_cascade = 0;
		while ((1 << max_cascade) < s) ++max_cascade;
		ds.cone_angle = s <= 1 ? 0.0f : (1.0f / 256.0f);
		have_data = true;
		const uint32_t n_cells = GRID3 * (max_cascade + 1);
		density_grid.alloc(n_cells); density_tmp.alloc(n_cells);
		HIP_CHECK(hipMemset(density_grid.p, 0, n_cells * 4));
		bitfield.alloc(GRID3 / 8 * NERF_CASCADES);
		HIP_CHECK(hipMemset(bitfield.p, 0xff, GRID3 / 8 * NERF_CASCADES));
		bf_lin.alloc(LIN_WORDS);
		launch_bitfield_linear(stream, bitfield.p, bf_lin.p);
		occ_bbox.alloc(occ_bbox_scratch_floats());
		launch_occ_bbox(stream, bitfield.p, occ_bbox.p);
		grid_mean.alloc(4); grid_partial.alloc(GRID3 / 1024);
		HIP_CHECK(hipMemset(grid_mean.p, 0, 16));
	}

	// ------------------------------------------------------------ network (reset_network, testbed.cu:2084-2349)
	void reset_network(const NeusNetworkConfig& c, const float* geo) {
		if (!have_data) throw std::runtime_error("reload_network: load training data first");
		setup_network(c, geo);
		alloc_step_workspace();
	}

	// initial parameters (trainer.h:54-109): seed_seq{seed} -> pcg32; xavier MLPs (the density MLP replaced by
	// `geo` when given), hash grid U(-1e-4, 1e-4), variance 0.3
	std::vector<float> initial_params(uint32_t seed, const float* geo) const {
		std::seed_seq seq{seed};
		std::vector<uint32_t> seeds(2);
		seq.generate(seeds.begin(), seeds.end());
		return initial_params_rng(make_pcg32(seeds.front()), geo);
	}
	// NerfNetwork::initialize_params (nerf_network.h:741-886) drawing from `rnd`
	std::vector<float> initial_params_rng(pcg32 rnd, const float* geo) const {
		const Layout& l = lay;
		const uint32_t P = l.P;
		std::vector<float> h(P, 0.f);
		{
			auto xavier = [&](uint32_t off, uint32_t out, uint32_t in) {
				const float scale = std::sqrt(6.0f / (float)(in + out));
				for (uint32_t i = 0; i < out * in; ++i) h[off + i] = rnd.next_float() * 2.0f * scale - scale;
			};
			xavier(l.off_d0, l.W, l.din); xavier(l.off_d1, 16, l.W);
			if (geo) std::memcpy(h.data(), geo, sizeof(float) * l.n_density);
			xavier(l.off_r0, l.W, 48); xavier(l.off_r1, l.W, l.W); xavier(l.off_r2, 16, l.W);
			// grid: generate_random_uniform(rnd, n, -1e-4, 1e-4) (random.h:67-91; 128-thread blocks)
			const size_t N = l.n_grid, per = 4, n_threads = (N + per - 1) / per, n_pad = (n_threads + 127) / 128 * 128;
			for (size_t i = 0; i < n_pad; ++i) {
				pcg32 r = rnd; r.advance((int64_t)(i * per));
				for (size_t j = 0; j < per; ++j) {
					const size_t idx = i + n_pad * j;
					if (idx >= N) break;
					h[l.grid_off + idx] = r.next_float() * (1e-4f - -1e-4f) + -1e-4f;
				}
			}
			rnd.advance((int64_t)N);
			for (int k = 0; k < 4; ++k) h[l.var_off + k] = 0.3f;  // nerf_network.h:881-882
		}
		return h;
	}

	// The network half of reset_network: config checks, grid tables, parameter layout and initial parameters, the
	// fp16 / transposed weight copies and the workspace of one forward + backward over `batch` samples (encode,
	// training MLP, weight gradients, grid scatter). The tcnn-shaped operator modules (neus_module_*) use only this.
	void setup_network(const NeusNetworkConfig& c, const float* geo, bool with_mlp = true) {
		if (c.n_features_per_level != 2) throw std::runtime_error("GridEncoding: only n_features_per_level = 2 is supported");
		if (c.n_levels == 0 || c.n_levels > MAX_LEVELS) throw std::runtime_error("GridEncoding: 1..16 levels supported");
		if (with_mlp && (c.n_density_hidden != 1 || c.n_rgb_hidden != 2)) throw std::runtime_error("NerfNetwork: density 1 hidden layer, rgb 2 hidden layers required on gfx950");
		if (with_mlp && !mlp_supported(c.n_levels, c.n_neurons)) throw std::runtime_error("NerfNetwork: unsupported (n_levels, n_neurons) combination for the gfx950 MLP kernels");
		if (c.batch_size == 0 || c.batch_size % 128 != 0) throw std::runtime_error("batch_size must be a positive multiple of 128");
		cfg = c;
		// per_level_scale (testbed.cu:2184-2187), grid tables (grid.h:1466-1501)
		float pls = c.per_level_scale;
		if (pls <= 0.f) pls = c.n_levels > 1 ? std::exp(std::log(c.top_resolution * aabb_scale / (float)c.base_resolution) / (c.n_levels - 1)) : 2.0f;
		cfg.per_level_scale = pls;
		gl = GridLevels{};
		gl.n_levels = c.n_levels;
		uint32_t offset = 0;
		for (uint32_t i = 0; i < c.n_levels; ++i) {
			const float scale = exp2f(i * std::log2(pls)) * c.base_resolution - 1.0f;
			const uint32_t resolution = (uint32_t)(std::ceil(scale)) + 1;
			const uint32_t max_params = 0xffffffffu / 2;
			uint32_t pil = std::pow((float)resolution, 3) > (float)max_params ? max_params : resolution * resolution * resolution;
			pil = next_multiple(pil, 8u);
			pil = std::min(pil, 1u << c.log2_hashmap_size);
			gl.offset[i] = offset; gl.res[i] = resolution; gl.scale[i] = (float)(resolution - 1);
			offset += pil;
		}
		gl.offset[c.n_levels] = offset;
		gl.dense_bits = 0;
		for (uint32_t i = 0; i < c.n_levels; ++i) {
			const uint64_t r = gl.res[i], hs = gl.offset[i + 1] - gl.offset[i];
			if (r * r * r <= hs) gl.dense_bits |= 1u << i;
			else if ((hs & (hs - 1)) != 0) throw std::runtime_error("hashed grid level with a non-power-of-two table");
		}
		// parameter layout (nerf_network.h:741-785)
		Layout& l = lay;
		l.L = c.n_levels; l.W = c.n_neurons; l.din = next_multiple(3 + 2 * c.n_levels, 16);
		l.off_d0 = 0; l.off_d1 = l.W * l.din; l.n_density = l.off_d1 + 16 * l.W;
		l.off_r0 = l.n_density; l.off_r1 = l.off_r0 + l.W * 48; l.off_r2 = l.off_r1 + l.W * l.W;
		l.n_rgb = l.off_r2 + 16 * l.W - l.n_density;
		l.n_matrix = l.n_density + l.n_rgb;
		l.grid_off = l.n_matrix; l.n_grid = offset * 2;
		l.var_off = l.grid_off + l.n_grid; l.P = l.var_off + 4;
		const uint32_t P = l.P;
		params_fp.alloc(P); grads.alloc(P); m1.alloc(P); m2.alloc(P); ema_tmp.alloc(P); adam_steps.alloc(P);
		params_h.alloc(P); ema_h.alloc(P);
		wT.alloc(l.din * l.W + l.W * 16 + 48 * l.W + l.W * l.W + l.W * 16 + 2 * l.din * l.W + 64);
		wT_ema.alloc(wT.n);
		const std::vector<float> h = initial_params(c.seed, geo);
		HIP_CHECK(hipMemcpy(params_fp.p, h.data(), (size_t)P * 4, hipMemcpyHostToDevice));
		HIP_CHECK(hipMemset(m1.p, 0, (size_t)P * 4)); HIP_CHECK(hipMemset(m2.p, 0, (size_t)P * 4));
		HIP_CHECK(hipMemset(ema_tmp.p, 0, (size_t)P * 4)); HIP_CHECK(hipMemset(adam_steps.p, 0, (size_t)P * 4));
		HIP_CHECK(hipMemset(ema_h.p, 0, (size_t)P * 2)); HIP_CHECK(hipMemset(grads.p, 0, (size_t)P * 4));
		ema_h_stale = false;
		launch_cast_half(stream, P, params_fp.p, params_h.p);
		setup_mlp_ptrs();
		prepare_weights();
		// RNG state (testbed.cu:2087-2101)
		rng = make_pcg32(c.seed);
		density_grid_rng = make_pcg32(rng.next_uint());
		(void)rng.next_uint();  // tv_loss_rng
		training_step = 0; adam_step = 0; lr_factor = 1.f; density_grid_ema_step = 0; enc_step = 0;
		occ_samples = 0; occ_updates = 0;
		loss_ema_init = false; loss_scalar_ema = last_loss = ek_loss = mask_loss = 0.f; loss_pending = false;
		nonfinite = aborted = false;
		// forward + backward workspace of one training batch
		batch = c.batch_size;
		max_samples = batch * 16;  // testbed_nerf.cu:3725
		enc.alloc((size_t)l.L * batch); dydx.alloc((size_t)6 * l.L * batch);  // training batch only: inference fuses the encode
		const size_t ld = batch;
		trainbuf.alloc(16 * ld + 2 * (2 * (size_t)l.L * ld) + 64);
		vbuf.alloc(batch);
		half_t* q = trainbuf.p;
		auto take = [&](size_t k) { half_t* r = q; q += (k + 7) / 8 * 8; return r; };
		tbuf = TrainBufs{};
		tbuf.d1_delta = take(16 * ld);
		tbuf.dLdenc = take(2 * (size_t)l.L * ld); tbuf.genc = take(2 * (size_t)l.L * ld);
		tbuf.v = vbuf.p;
		tbuf.var_grad = grads.p + l.var_off;
		mlp_blocks = mlp_train_blocks(l.L, l.W, batch);
		var_partial.alloc(mlp_blocks);
		tbuf.var_partial = var_partial.p;
		// one row of MLP weight-gradient partials per training-kernel block
		wgrad_partial.alloc((size_t)mlp_blocks * l.n_matrix);
		tbuf.wpartial = wgrad_partial.p;
		tbuf.n_matrix = l.n_matrix; tbuf.off_d1 = l.off_d1; tbuf.off_r0 = l.off_r0; tbuf.off_r1 = l.off_r1; tbuf.off_r2 = l.off_r2;
		tbuf.indeed_batch = (float)batch * (float)x.world();
		// binned grid-gradient scatter workspace (grid.hip)
		swork = ScatterWork{};
		swork.n_blocks = (batch + 255) / 256;
		// the path (per-block record regions unless opt.scatter_mode says otherwise) and its workgroups' samples
		swork.mode = opt.scatter_mode;
		swork.chunk = opt.scatter_chunk;
		swork.n_chunks = (batch + swork.chunk - 1) / swork.chunk;
		swork.level_groups = opt.scatter_level_groups;
		swork.n_buckets = scatter_n_buckets(gl);
		if (swork.n_buckets > SB_MAX_BUCKETS) throw std::runtime_error("hash grid too large for the scatter buckets");
		const size_t n_bins = (size_t)swork.n_buckets * swork.n_blocks + 1;
		sc_counts.alloc(n_bins); sc_offs.alloc(n_bins);
		const size_t n_rec = std::max(scatter_records_capacity(swork.n_blocks * 256, l.L), (size_t)l.L * swork.n_chunks * swork.chunk * 8);
		sc_rec_g.alloc(n_rec); sc_rec_i.alloc(n_rec);
		swork.counts = sc_counts.p; swork.offs = sc_offs.p; swork.rec_g = sc_rec_g.p; swork.rec_i = sc_rec_i.p;
		{
			uint32_t n_split = 0;
			const std::vector<uint32_t> jobs = scatter_accum_jobs(gl, swork.n_buckets, n_split);
			sc_jobs.alloc(jobs.size());
			HIP_CHECK(hipMemcpy(sc_jobs.p, jobs.data(), jobs.size() * 4, hipMemcpyHostToDevice));
			uint32_t n_split2 = 0;
			const std::vector<uint32_t> jobs2 = scatter_region_jobs(gl, n_split2, sc_jobs2_before);
			sc_jobs2.alloc(jobs2.size());
			HIP_CHECK(hipMemcpy(sc_jobs2.p, jobs2.data(), jobs2.size() * 4, hipMemcpyHostToDevice));
			swork.jobs2 = (const uint4*)sc_jobs2.p; swork.n_jobs2 = (uint32_t)(jobs2.size() / 4);
			swork.xcd_group = opt.scatter_xcd_group;
			if (sc_jobs2_before.size() > 17) throw std::runtime_error("region scatter: at most 16 levels");
			for (size_t k = 0; k < sc_jobs2_before.size(); ++k) swork.jobs2_before[k] = sc_jobs2_before[k];
			sc_rtab.alloc((size_t)l.L * swork.n_chunks * (SB_LEVEL_BUCKETS + 1));
			swork.rtab = sc_rtab.p;
			n_split = std::max(n_split, n_split2);
			sc_split.alloc(std::max<size_t>(1, (size_t)n_split * 2 * SB_SIZE)); sc_split_done.alloc(std::max(1u, n_split));
			HIP_CHECK(hipMemset(sc_split.p, 0, sc_split.n * sizeof(unsigned long long)));
			HIP_CHECK(hipMemset(sc_split_done.p, 0, sc_split_done.n * 4));
			swork.jobs = (const uint4*)sc_jobs.p; swork.split = sc_split.p; swork.split_done = sc_split_done.p;
			swork.n_jobs = (uint32_t)(jobs.size() / 4);
			swork.n_active = swork.n_buckets;
			sc_jobs_before.assign(swork.n_buckets + 1, 0u);
			for (size_t j = 0; j < jobs.size() / 4; ++j) sc_jobs_before[jobs[4 * j] + 1] = (uint32_t)j + 1;
			for (uint32_t b = 1; b <= swork.n_buckets; ++b) sc_jobs_before[b] = std::max(sc_jobs_before[b], sc_jobs_before[b - 1]);
			sc_zero_from = swork.n_buckets;  // nothing assumed
			sc_zero_from_e = gl.offset[gl.n_levels];
		}
		scan_tmp_bytes = std::max({scan_temp_bytes(MAX_RAYS), scan_temp_bytes((uint32_t)n_bins),
		                           scan_temp_bytes(2 * (2 * RS_BINS + 1) * ray_sort_blocks(MAX_RAYS))});
		scan_tmp.alloc(scan_tmp_bytes + 256);
		scan_temp_reset(stream, scan_tmp.p);
		HIP_CHECK(hipStreamSynchronize(stream));
	}

	// The training-step half of reset_network: ray / march / loss / compaction buffers (per-step state sized for
	// MAX_RAYS rays and 16 x batch samples), occupancy-update scratch, device counters, dynamic-scene state.
	void alloc_step_workspace() {
		rays.alloc(6 * (size_t)MAX_RAYS); startt.alloc((size_t)MAX_RAYS);
		march_rec.alloc((size_t)MAX_RAYS * NERF_STEPS); march_nrec.alloc(MAX_RAYS); march_queue.alloc(2);
		march_seg.alloc((size_t)MAX_RAYS * MARCH_SEG_RECS);
		mwork = MarchWork{march_rec.p, march_nrec.p, march_queue.p, opt.march_waves, march_seg.p, opt.march_lanes, jump_table()};
		mwork.balanced = opt.march_balance ? 1u : 0u;
		nreq.alloc(MAX_RAYS); base.alloc(MAX_RAYS);
		numsteps.alloc(2 * (size_t)MAX_RAYS); ccount.alloc(MAX_RAYS); cbase.alloc(MAX_RAYS);
		l_sa.alloc(max_samples); l_ekt.alloc(max_samples); sample_ray.alloc(max_samples); cmap.alloc(batch);
		l_ck4.alloc(max_samples / 8 + 1); l_cke.alloc(max_samples / 8 + 1);
		l_racc.alloc(MAX_RAYS); l_rgr.alloc(MAX_RAYS); l_rT.alloc(MAX_RAYS); l_rek.alloc(MAX_RAYS);
		// (the split round 0 of the compaction cut: pass B's list from max_samples, its rays from MAX_RAYS)
		chunk_list.alloc(2 * (size_t)max_samples); chunk_cnt.alloc(64); long_rays.alloc(MAX_RAYS);
		open_rays[0].alloc(MAX_RAYS); open_rays[1].alloc(MAX_RAYS); open_raw.alloc(MAX_RAYS); cutw.alloc(CW_WORDS);
		{ uint32_t w[CW_WORDS] = {}; w[CW_EST] = MAX_RAYS; HIP_CHECK(hipMemcpy(cutw.p, w, sizeof(w), hipMemcpyHostToDevice)); }
		rs_hist.alloc(2 * (size_t)(2 * RS_BINS + 1) * ray_sort_blocks(MAX_RAYS)); rs_off.alloc(rs_hist.n);
		rs_perm.alloc(2 * (size_t)MAX_RAYS); rs_key.alloc(MAX_RAYS);
		loss.alloc(MAX_RAYS); ek.alloc(MAX_RAYS); mask.alloc(MAX_RAYS); loss_sum.alloc(4); health_buf.alloc(4);
		coords.alloc((size_t)max_samples * COORD_W); net_out.alloc((size_t)max_samples * OUT_W);
		coords_c.alloc((size_t)batch * COORD_W); dL_dout.alloc((size_t)batch * OUT_W);
		const NeusNetworkConfig& c = cfg;
		const uint32_t n_occ = GRID3 * (max_cascade + 1) * 2;
		occ_pos.alloc(3 * (size_t)n_occ); occ_idx.alloc(n_occ); occ_density.alloc(n_occ);
		// device step state (Counters, testbed.h:596-616)
		StepState s{};
		s.rays_per_batch = c.fixed_rays_per_batch ? c.fixed_rays_per_batch : (1u << 12);
		s.max_inference = max_samples;
		HIP_CHECK(hipMemcpy(st.p, &s, sizeof(s), hipMemcpyHostToDevice));
		HIP_CHECK(hipMemset(density_grid.p, 0, density_grid.n * 4));
		// dynamic scenes: identity accumulated movement, identity local movement (DeltaNetwork::initialize_params,
		// transform_network.h:335-383; NerfNetwork::init_accumulation_movement, nerf_network.h:1042-1105)
		coords_def.alloc((size_t)max_samples * COORD_W); coords_cdef.alloc((size_t)batch * COORD_W); dpos.alloc(batch);
		delta.alloc(1); delta_partial.alloc(delta_partial_floats());
		reset_delta();
		ds.motion = RayMotion{};
		ds.motion.R[0] = ds.motion.R[4] = ds.motion.R[8] = 1.f;
		// the frame index and the phase flags belong to the Testbed, not the network: reset_network keeps them
		// (testbed.cu:2084-2349; load_snapshot on frame k of run_dynamic.py's test pass relies on it)
		canonical_step = 0;
		HIP_CHECK(hipStreamSynchronize(stream));
		have_net = true;
	}

	// a fresh global-move trainer: identity local movement, zero Adam state (testbed.cu:2569-2578)
	void reset_delta() {
		DeltaState h{};
		h.p[4] = 1.f; h.p[8] = 1.f;  // rotation 6D (1, 0, 0, 0, 1, 0)
		HIP_CHECK(hipMemcpyAsync(delta.p, &h, sizeof(h), hipMemcpyHostToDevice, stream));
		launch_delta_prepare(stream, delta.p);
		delta_step = 0; delta_lr_factor = 1.f;
	}

	// ------------------------------------------------------------ dynamic scenes: next frame (testbed.cu:2001-2082)
	void next_frame(uint32_t n_images, const NeusImage* imgs) {
		if (!have_net) throw std::runtime_error("next_frame: no network");
		HIP_CHECK(hipStreamSynchronize(stream));
		consume_loss();
		// accumulate_global_movement: fold this frame's local movement into the ray transform
		DeltaState h{};
		HIP_CHECK(hipMemcpy(&h, delta.p, sizeof(h), hipMemcpyDeviceToHost));
		RayMotion m = ds.motion;
		host_accumulate_movement(h.p, m.R, m.t);
		m.on = 1;
		// load_nerf(frame): the next frame's images and cameras (same aabb_scale)
		set_dataset(n_images, imgs, aabb_scale);
		ds.motion = m;
		++cur_frame;
		training_step = 0; canonical_step = 0;
		// save/load_snapshot_incremental: the new trainer starts from the serialized inference (EMA) weights,
		// fp16, with fresh optimizer state (Adam moments, per-parameter steps, EMA)
		const uint32_t P = lay.P;
		{
			std::vector<half_t> eh(P);
			sync_ema_h();
			HIP_CHECK(hipMemcpy(eh.data(), ema_h.p, (size_t)P * 2, hipMemcpyDeviceToHost));
			std::vector<float> ef(P);
			for (uint32_t i = 0; i < P; ++i) ef[i] = (float)eh[i];
			HIP_CHECK(hipMemcpy(params_fp.p, ef.data(), (size_t)P * 4, hipMemcpyHostToDevice));
			HIP_CHECK(hipMemcpy(params_h.p, eh.data(), (size_t)P * 2, hipMemcpyHostToDevice));
		}
		HIP_CHECK(hipMemset(m1.p, 0, (size_t)P * 4)); HIP_CHECK(hipMemset(m2.p, 0, (size_t)P * 4));
		HIP_CHECK(hipMemset(adam_steps.p, 0, (size_t)P * 4));
		// the fp32 EMA starts at the loaded weights: the first EMA step weighs it by 1 - decay^0 = 0, and until the
		// canonical optimizer steps (after the global-movement phase) it is what get_ema_params reports
		HIP_CHECK(hipMemcpy(ema_tmp.p, params_fp.p, (size_t)P * 4, hipMemcpyDeviceToDevice));
		adam_step = 0; lr_factor = 1.f;
		prepare_weights();
		// reset_network_incremental (testbed.cu:2351-2370): m_rng = seed, rays_per_batch = 4096, counters
		rng = make_pcg32(cfg.seed);
		StepState s{};
		s.rays_per_batch = cfg.fixed_rays_per_batch ? cfg.fixed_rays_per_batch : (1u << 12);
		s.max_inference = max_samples;
		HIP_CHECK(hipMemcpy(st.p, &s, sizeof(s), hipMemcpyHostToDevice));
		reset_delta();
		train_canonical = false;
		train_delta = cfg.predict_global_movement != 0;
		HIP_CHECK(hipStreamSynchronize(stream));
	}
	// Testbed::change_to_frame (testbed.cu:1939-1985): load frame `k`'s images and restart the step count with a
	// fresh optimizer (Adam moments, steps, EMA state); parameters, density grid state of the network, the ray
	// movement and the training phase flags stay (run_dynamic.py follows it with load_snapshot).
	void change_frame(uint32_t k, uint32_t n_images, const NeusImage* imgs) {
		if (!have_net) throw std::runtime_error("change_to_frame: no network");
		HIP_CHECK(hipStreamSynchronize(stream));
		consume_loss();
		const RayMotion m = ds.motion;
		set_dataset(n_images, imgs, aabb_scale);
		ds.motion = m;
		cur_frame = k;
		training_step = 0; canonical_step = 0;
		const uint32_t P = lay.P;
		HIP_CHECK(hipMemset(m1.p, 0, (size_t)P * 4)); HIP_CHECK(hipMemset(m2.p, 0, (size_t)P * 4));
		HIP_CHECK(hipMemset(adam_steps.p, 0, (size_t)P * 4));
		{  // the fp32 EMA restarts from the inference weights (weighted by 0 at the next EMA step)
			std::vector<half_t> eh(P);
			sync_ema_h();
			HIP_CHECK(hipMemcpy(eh.data(), ema_h.p, (size_t)P * 2, hipMemcpyDeviceToHost));
			std::vector<float> ef(P);
			for (uint32_t i = 0; i < P; ++i) ef[i] = (float)eh[i];
			HIP_CHECK(hipMemcpy(ema_tmp.p, ef.data(), (size_t)P * 4, hipMemcpyHostToDevice));
		}
		adam_step = 0; lr_factor = 1.f;
		HIP_CHECK(hipStreamSynchronize(stream));
	}
	uint32_t gm_steps() const { return cfg.predict_global_movement ? cfg.global_movement_steps : 0u; }

	void setup_mlp_ptrs() {
		setup_mlp_ptrs_for(params_h.p, wT.p, mlp);
		setup_mlp_ptrs_for(ema_h.p, wT_ema.p, mlp_ema);
		din_perm = DinPerm{};
		mlp_din_permutation(lay.L, din_perm.p);
		din_perm.din = lay.din; din_perm.W = lay.W;
	}
	void setup_mlp_ptrs_for(const half_t* base, half_t* t, MlpPtrs& mlp) {
		const Layout& l = lay;
		mlp.d0 = base + l.off_d0; mlp.d1 = base + l.off_d1;
		mlp.r0 = base + l.off_r0; mlp.r1 = base + l.off_r1; mlp.r2 = base + l.off_r2;
		auto take = [&](size_t k) { half_t* r = t; t += (k + 7) / 8 * 8; return r; };
		mlp.d0T = take(l.din * l.W); mlp.d1T = take(l.W * 16); mlp.r0T = take(48 * l.W); mlp.r1T = take(l.W * l.W); mlp.r2T = take(l.W * 16);
		mlp.d0p = take(l.din * l.W); mlp.d0Tp = take(l.din * l.W);
		mlp.var = base + l.var_off;
		mlp.sdf_bias = cfg.sdf_bias;
	}
	void prepare_weights() { prepare_weights_for(mlp); }
	void prepare_weights_for(const MlpPtrs& mlp) {
		const Layout& l = lay;
		TransposeJobs tj{};
		tj.j[0] = {mlp.d0, (half_t*)mlp.d0T, l.W, l.din};
		tj.j[1] = {mlp.d1, (half_t*)mlp.d1T, 16, l.W};
		tj.j[2] = {mlp.r0, (half_t*)mlp.r0T, l.W, 48};
		tj.j[3] = {mlp.r1, (half_t*)mlp.r1T, l.W, l.W};
		tj.j[4] = {mlp.r2, (half_t*)mlp.r2T, 16, l.W};
		tj.n = 5;
		launch_transpose_permute(stream, tj, mlp.d0, (half_t*)mlp.d0p, (half_t*)mlp.d0Tp, din_perm);
	}

	// progressive levels (grid.h:2427-2440)
	uint32_t valid_level_at(int step) const {
		if (step <= 0) return cfg.n_levels;
		const float v = std::ceil(cfg.base_valid_level_scale * cfg.n_levels + cfg.valid_level_scale * std::max(0, (int)(step - (int)cfg.base_training_step)));
		return std::min(cfg.n_levels, (uint32_t)v);
	}
	float cos_anneal() const { return cfg.anneal_end == 0 ? 1.0f : std::min(1.0f, (float)training_step / cfg.anneal_end); }

	// ------------------------------------------------------------ network stages
	void encode(const uint32_t* n_ptr, uint32_t n_fixed, uint32_t n_cap, uint32_t ld, const float* c, uint32_t stride, uint32_t valid, bool want_dydx, hipStream_t s,
	            const EncodeRollover* ro = nullptr) {
		const uint32_t gx = std::max<uint32_t>(1, std::min<uint32_t>((n_cap + 255) / 256, 2048));
		launch_grid_encode(s, n_ptr, n_fixed, ld, c, stride, gl, valid, params_h.p + lay.grid_off, enc.p, want_dydx ? dydx.p : nullptr, gx, ro);
	}
	void net_forward(const uint32_t* n_ptr, uint32_t n_fixed, uint32_t n_cap, const float* c, uint32_t valid, half_t* out, hipStream_t s) {
		const uint32_t blocks = std::max<uint32_t>(1, std::min<uint32_t>((n_cap + 127) / 128, 8192));
		launch_nerf_infer(s, lay.L, lay.W, n_ptr, n_fixed, c, gl, valid, params_h.p + lay.grid_off, mlp, out, blocks);
	}
	// the reduction of the training kernels' per-block weight-gradient rows (and variance partials) into g
	MlpGradReduce grad_reduce(uint32_t n, float* g, const uint32_t* n_valid) const {
		MlpGradReduce r{};
		r.partial = wgrad_partial.p; r.n_blocks = mlp_train_blocks(lay.L, lay.W, n); r.n_matrix = lay.n_matrix; r.g = g;
		r.n_valid = n_valid; r.var_partial = var_partial.p; r.var_blocks = r.n_blocks; r.var_grad = g + lay.var_off;
		return r;
	}
	// The grid-gradient buckets past the progressive valid level get no records: their gradient is zero. For the
	// testbed's own gradient buffer the scatter skips them once they hold zeros (early in training ~2,500 of ~2,600
	// buckets, each a 64 KB-LDS workgroup), zeroing first the range a lower valid level than the previous step's
	// leaves stale (a reloaded network, a frame switch).
	ScatterWork scatter_work_for(float* g_grid, uint32_t valid, hipStream_t s) {
		if (g_grid != grads.p + lay.grid_off || sc_jobs_before.empty()) return swork;
		const uint32_t L = gl.n_levels, n_entries = gl.offset[L];
		if (opt.scatter_noskip) {  // A/B reference: the whole grid gradient zeroed before every scatter
			HIP_CHECK(hipMemsetAsync(g_grid, 0, (size_t)n_entries * 2 * sizeof(float), s));
			sc_zero_from = swork.n_buckets; sc_zero_from_e = n_entries;
			return swork;
		}
		if (swork.mode == 2) {
			// the accumulation writes exactly the entries of the levels up to the valid one
			const uint32_t lv = std::min(valid + 1, L), e_end = gl.offset[lv];
			if (sc_zero_from_e > e_end) HIP_CHECK(hipMemsetAsync(g_grid + 2 * (size_t)e_end, 0, (size_t)(sc_zero_from_e - e_end) * 2 * sizeof(float), s));
			sc_zero_from_e = e_end;
			ScatterWork w = swork;
			w.n_jobs2 = sc_jobs2_before[lv];
			return w;
		}
		const uint32_t sb = valid + 1 >= L ? swork.n_buckets : std::min(swork.n_buckets, (gl.offset[valid + 1] + SB_SIZE - 1) / SB_SIZE);
		if (sc_zero_from > sb) {
			const size_t e_lo = (size_t)sb * SB_SIZE, e_hi = std::min<size_t>((size_t)sc_zero_from * SB_SIZE, n_entries);
			if (e_hi > e_lo) HIP_CHECK(hipMemsetAsync(g_grid + 2 * e_lo, 0, (e_hi - e_lo) * 2 * sizeof(float), s));
		}
		sc_zero_from = sb;
		ScatterWork w = swork;
		w.n_jobs = sc_jobs_before[sb];
		w.n_active = sb;  // histogram and scan only the buckets that can receive records
		return w;
	}
	// forward recompute + backward into g (fp32 [P], zeroed by the caller)
	void net_backward(const uint32_t* n_valid_ptr, const uint32_t* n_train_ptr, uint32_t n, const float* c, uint32_t valid,
	                  const half_t* dlo, float* g, hipStream_t s, bool marks = false, bool canonical = true, const EncodeRollover* ro = nullptr,
	                  bool exchange = false, AdamSplit* as = nullptr) {
		const uint32_t ld = n;
		encode(n_train_ptr, n, n, ld, c, COORD_W, valid, true, s, ro);
		la_fire(1);
		if (marks) mark(5);
		TrainBufs t = tbuf;
		t.var_grad = g + lay.var_off;
		launch_mlp_train(s, lay.L, lay.W, n_valid_ptr, n, ld, c, (const half_t*)enc.p, dydx.p, dlo, mlp, t);
		la_fire(2);
		if (marks) mark(6);
		if (!canonical) { if (marks) mark(7); return; }  // global-movement phase: canonical gradients unused
		// the MLP weight gradients were accumulated inside the training kernels: one small fixed-order reduction
		launch_mlp_grad_reduce(s, grad_reduce(n, g, n_train_ptr));
		la_fire(3);
		if (exchange) {  // the MLP blocks and the variance are final: their exchange runs beside the grid scatter
			hipStream_t xs = x.gated();
			x.allreduce_f32(g, lay.grid_off, false, xs);
			x.allreduce_f32(g + lay.var_off, lay.P - lay.var_off, false, xs);
			if (as) as->on = xs;  // (the optimizer's pieces follow their ranges' all-reduces on the exchange stream)
		}
		if (as) adam_issue(*as, lay.grid_off, g, true);  // the MLP blocks (and their transposed copies) beside the scatter
		if (marks) mark(7);
		const ScatterWork sw = scatter_work_for(g + lay.grid_off, valid, s);
		ScatterSplit sp = exchange && sw.mode == 2 ? x_split(valid, g + lay.grid_off) : ScatterSplit{};
		const bool a_split = as && sw.mode == 2;
		if (a_split) {  // the level groups of the overlapped exchange; each group's Adam once its accumulation (and exchange) is queued
			if (!exchange) sp = x_split(valid, g + lay.grid_off);
			auto xdone = exchange ? sp.done : std::function<void(uint32_t, uint32_t)>();
			sp.done = [this, as, g, xdone](uint32_t lo, uint32_t hi) {
				if (xdone) xdone(lo, hi);
				adam_issue(*as, lay.grid_off + 2 * gl.offset[hi], g, false);
			};
		}
		launch_grid_scatter(s, n_train_ptr, n, ld, c, COORD_W, gl, valid, tbuf.dLdenc, tbuf.genc, tbuf.v, g + lay.grid_off, sw, scan_tmp.p,
		                    scan_tmp_bytes, (exchange || a_split) && sw.mode == 2 ? &sp : nullptr);
		if (exchange && sw.mode != 2) {  // other scatter modes: the grid exchange after the whole scatter
			const size_t grid_act = 2 * (size_t)gl.offset[std::min(valid + 1, gl.n_levels)];
			x.allreduce_f32(g + lay.grid_off, grid_act, false, x.gated());
		}
	}

	// ------------------------------------------------------------ occupancy grid (testbed_nerf.cu:3293-3397, 4003-4016)
	void occ_update(uint32_t n_uniform, uint32_t n_nonuniform, uint32_t valid, bool use_delta = false) {
		hipStream_t s = stream;
		const uint32_t n_cells = GRID3 * (max_cascade + 1);
		if (training_step == 0) { HIP_CHECK(hipMemsetAsync(density_grid.p, 0, n_cells * 4, s)); density_grid_ema_step = 0; }
		// the first 256 steps' all-cells uniform pass writes every cell exactly once (fused path, one cascade): on a
		// single GPU no clearing is needed; with shards each rank writes only its cells, the rest must read 0
		const bool exclusive = !use_delta && n_nonuniform == 0 && n_uniform == GRID3 && max_cascade == 0;
		const uint32_t rank = x.rank(), world = x.world();
		if (!exclusive || world > 1) HIP_CHECK(hipMemsetAsync(density_tmp.p, 0, n_cells * 4, s));
		// data parallel: rank r evaluates the global samples [lo, hi) (same density_grid_rng on every rank; in the
		// exclusive pass the cells [lo, hi), i.e. the samples that land there); the max-splatted grids are then
		// max-all-reduced, which equals the single-GPU splat (max is exact)
		const uint32_t NT = n_uniform + n_nonuniform;
		const uint32_t lo = (uint32_t)((uint64_t)NT * rank / world), hi = (uint32_t)((uint64_t)NT * (rank + 1) / world);
		const uint32_t N = hi - lo;
		occ_samples += N; ++occ_updates;
		const pcg32 rng_u = density_grid_rng;
		density_grid_rng.advance();
		const pcg32 rng_nu = density_grid_rng;
		density_grid_rng.advance();
		if (!use_delta) {
			// sample generation + NerfNetwork::density + splat in one kernel
			OccSampling os{};
			os.n_u = n_uniform; os.n_nu = n_nonuniform; os.lo = lo;
			os.rng_u_state = rng_u.state; os.rng_u_inc = rng_u.inc; os.rng_nu_state = rng_nu.state; os.rng_nu_inc = rng_nu.inc;
			os.step = density_grid_ema_step; os.n_cascades = max_cascade + 1; os.thresh_nu = NERF_MIN_OPTICAL_THICKNESS;
			for (int d = 0; d < 3; ++d) { os.amin[d] = ds.aabb_min[d]; os.diag[d] = ds.aabb_max[d] - ds.aabb_min[d]; }
			os.grid_in = density_grid.p; os.grid_tmp = density_tmp.p;
			os.jt = jump_table();
			os.exclusive = exclusive ? 1u : 0u;
			// the uniform part in cell order (spatially coherent gathers; the max splat is order-independent): one cascade
			// of cells or fewer uniform samples, so the uniform hash is a bijection onto the cells
			const uint32_t u_lo = std::min(lo, n_uniform), u_hi = std::min(hi, n_uniform);
			if (!exclusive && opt.occ_sort && u_hi > u_lo && n_uniform <= GRID3) {
				if (!occ_ulist.p) occ_ulist.alloc(GRID3);
				launch_occ_uniform_list(s, n_uniform, density_grid_ema_step, u_lo, u_hi, occ_ulist.p, scan_tmp.p);
				os.ulist = occ_ulist.p; os.n_ulist = u_hi - u_lo;
				// (opt.occ_nu_sort: the occupancy-biased samples binned by their coarse cell as well; in index order the biased half
				// takes 294 of the pass's 479 us, the cell-ordered uniform half 187 - profiles/r06occ_split.txt)
				const uint32_t nu_lo = std::max(lo, n_uniform), n_nu_rank = hi > nu_lo ? hi - nu_lo : 0u;
				if (opt.occ_nu_sort && n_nu_rank) {
					if (occ_nu_key.n < n_nu_rank) { occ_nu_key.alloc(n_nu_rank); occ_nu_list.alloc(n_nu_rank); }
					occ_nu_bins.alloc(2 * 4096 * (size_t)(max_cascade + 1));
					launch_occ_nu_list(s, n_nu_rank, nu_lo - n_uniform, os, occ_nu_key.p, occ_nu_bins.p, occ_nu_list.p, scan_tmp.p, scan_tmp_bytes);
					os.nulist = occ_nu_list.p;
				}
			}
			launch_occ_density(s, lay.L, lay.W, N, os, gl, valid, params_h.p + lay.grid_off, mlp);
		} else {
			launch_grid_samples(s, n_uniform, std::min(lo, n_uniform), std::min(hi, n_uniform), 0, rng_u.state, rng_u.inc, density_grid_ema_step,
			                    ds.aabb_min, ds.aabb_max, density_grid.p, occ_pos.p, occ_idx.p, max_cascade + 1, -0.01f, jump_table());
			launch_grid_samples(s, n_nonuniform, std::max(lo, n_uniform) - n_uniform, std::max(hi, n_uniform) - n_uniform,
			                    std::max(lo, n_uniform) - lo, rng_nu.state, rng_nu.inc, density_grid_ema_step, ds.aabb_min, ds.aabb_max,
			                    density_grid.p, occ_pos.p, occ_idx.p, max_cascade + 1, NERF_MIN_OPTICAL_THICKNESS, jump_table());
			// NerfNetwork::density on the moved positions (the DeltaNetwork is active, nerf_network.h:664-675)
			launch_delta_apply(s, nullptr, N, 3, occ_pos.p, occ_pos.p, delta.p);
			launch_nerf_density(s, lay.L, lay.W, N, occ_pos.p, gl, valid, params_h.p + lay.grid_off, mlp, occ_density.p);
			launch_splat_max(s, N, occ_idx.p, occ_density.p, density_tmp.p);
		}
		x.allreduce_f32(density_tmp.p, n_cells, true);
		// EMA + mean partials (one launch), final mean, bitfield, mip pools + the march's linear words (one launch)
		launch_ema_mean(s, n_cells, cfg.density_grid_decay, density_grid.p, density_tmp.p, grid_partial.p, grid_mean.p);
		++density_grid_ema_step;
		launch_bitfield(s, density_grid.p, bitfield.p, grid_mean.p, max_cascade + 1, bf_lin.p);
		launch_occ_bbox(s, bitfield.p, occ_bbox.p);
	}

	// ------------------------------------------------------------ optimizer (trainer.h:170-172)
	void optimizer_step(const float* g, const StepCounterArgs* counters = nullptr) {
		const AdamParams p = adam_params();
		const AdamTranspose tr = adam_transpose();  // the transposed / permuted MLP copies are written by the Adam launch itself
		launch_adam_ema(stream, p, params_fp.p, params_h.p, g, m1.p, m2.p, adam_steps.p, steps32, ema_tmp.p, ema_h.p, counters, &tr);
		if (p.skip_ema_h) ema_h_stale = true;
	}
	// The host side of one optimizer step (advances the step count and the learning-rate decay): call once per step
	AdamParams adam_params() {
		// ExponentialDecay (exponential_decay.h:61-80): evaluated with the nested step count before the Adam step
		const uint32_t sb = adam_step;
		if (sb == 0) lr_factor = 1.0f;
		if (sb >= cfg.decay_start && (sb - cfg.decay_start) % cfg.decay_interval == 0 && sb <= 10000000u) lr_factor *= cfg.decay_base;
		++adam_step;
		AdamParams p{};
		p.n = lay.P; p.n_matrix = lay.n_matrix; p.loss_scale = LOSS_SCALE;
		p.lr = (cur_frame ? cfg.after_learning_rate : cfg.learning_rate) * lr_factor;  // testbed.cu:2695-2702
		p.beta1 = cfg.beta1; p.beta2 = cfg.beta2; p.eps = cfg.epsilon; p.l2_reg = cfg.l2_reg;
		p.ema_decay = cfg.ema_decay;
		p.ema_debias_old = 1 - (float)std::pow(cfg.ema_decay, adam_step - 1);
		p.ema_debias_new = 1.0f / (1 - (float)std::pow(cfg.ema_decay, adam_step));
		p.optimize_matrix = 1; p.optimize_non_matrix = 1;
		int e2 = 0;
		p.pow2_scale = std::frexp(p.loss_scale, &e2) == 0.5f ? 1u : 0u;
		p.inv_loss_scale = 1.0f / p.loss_scale;
		ensure_bias_table();
		p.bias_tab = adam_bias.p; p.bias_converged = bias_conv ? 1u : 0u;
		p.skip_ema_h = opt.eager_ema_h ? 0u : 1u;
		p.abort = &st.p->cut_abort;  // (the march cut's witness: a step that is re-run applies nothing)
		return p;
	}
	// Adam in pieces beside the backward (opt.adam_overlap; static scenes): the MLP blocks once the weight-gradient
	// reduction is done (beside the grid scatter), each grid level group once its accumulation launch is done (beside the
	// next group's), on ad_stream at one rank - the step's stream joins it where the one Adam launch used to be - and under
	// data parallel on the exchange stream, each piece behind its range's all-reduce. Elementwise, so the parameters are
	// bitwise those of the one launch. Cut points are rounded down to 4 parameters (the kernel's 16-B groups): a range may
	// start with the last few parameters of the level before it, whose gradient is final already.
	// ad_stream is the step's side stream (aux_stream, created with the step's stream at its priority): a stream of its own
	// would be a fifth HIP stream of the process over GPU_MAX_HW_QUEUES = 4 hardware queues and share one - measured
	// 1.12 -> 1.99 ms/step when it landed behind the lookahead's low-priority march (profiles/r06b_adam_overlap_mlp_grid_ab.txt)
	hipStream_t ad_stream = nullptr;
	Event ad_ev[8], ad_done;
	int ad_n = 0;
	void adam_issue(AdamSplit& a, uint32_t hi, const float* g, bool with_tr) {
		if (!ad_stream) {
			ad_stream = aux_stream.get();
			for (auto& e : ad_ev) e = make_event(hipEventDisableTiming);
			ad_done = make_event(hipEventDisableTiming);
		}
		hi = hi >= lay.P ? lay.P : hi / 4 * 4;
		if (hi <= a.next) return;
		hipStream_t on = a.on;
		if (!on) {
			hipEvent_t e = ad_ev[ad_n++ % 8].get();
			HIP_CHECK(hipEventRecord(e, stream));
			HIP_CHECK(hipStreamWaitEvent(ad_stream, e, 0));
			on = ad_stream;
		}
		const AdamTranspose tr = with_tr ? adam_transpose() : AdamTranspose{};
		launch_adam_ema_range(on, a.p, a.next, hi, params_fp.p, params_h.p, g, m1.p, m2.p, adam_steps.p, steps32, ema_tmp.p, ema_h.p,
		                      with_tr ? &tr : nullptr);
		a.next = hi;
	}
	void adam_join(AdamSplit& a, const float* g) {
		adam_issue(a, lay.P, g, false);  // (whatever is left: the levels past the valid one, the variance)
		if (!a.on) {  // (on the exchange stream the step's join has waited for every piece already)
			HIP_CHECK(hipEventRecord(ad_done.get(), ad_stream));
			HIP_CHECK(hipStreamWaitEvent(stream, ad_done.get(), 0));
		}
		if (a.p.skip_ema_h) ema_h_stale = true;
	}
	// bias-correction table for the config's betas (rebuilt only when they change), and the step counts' width for it:
	// u16 while the table is converged, u32 otherwise (moved through the host when the betas change)
	void ensure_bias_table() {
		const float b1 = cfg.beta1, b2 = cfg.beta2;
		if (b1 == bias_b1 && b2 == bias_b2) return;
		adam_bias.alloc(2 * ADAM_BIAS_TAB);
		launch_adam_bias_table(stream, b1, b2, adam_bias.p);
		float last[2];
		HIP_CHECK(hipStreamSynchronize(stream));
		HIP_CHECK(hipMemcpy(&last[0], adam_bias.p + ADAM_BIAS_TAB - 1, 4, hipMemcpyDeviceToHost));
		HIP_CHECK(hipMemcpy(&last[1], adam_bias.p + 2 * ADAM_BIAS_TAB - 1, 4, hipMemcpyDeviceToHost));
		const double k = ADAM_BIAS_TAB - 1;
		bias_conv = last[0] == 1.0f && last[1] == 1.0f && std::pow((double)b1, k) < 0x1p-30 && std::pow((double)b2, k) < 0x1p-30;
		bias_b1 = b1; bias_b2 = b2;
		if (steps32 == bias_conv) {
			std::vector<uint32_t> h(lay.P);
			get_steps(h.data());
			steps32 = !bias_conv;
			put_steps(h.data());
		}
	}
	void get_steps(uint32_t* out) {
		if (steps32) { HIP_CHECK(hipMemcpy(out, adam_steps.p, lay.P * 4, hipMemcpyDeviceToHost)); return; }
		std::vector<uint16_t> h(lay.P);
		HIP_CHECK(hipMemcpy(h.data(), adam_steps.p, lay.P * 2, hipMemcpyDeviceToHost));
		for (size_t i = 0; i < lay.P; ++i) out[i] = h[i];
	}
	void put_steps(const uint32_t* in) {  // in = nullptr: zeros
		if (!in) { HIP_CHECK(hipMemset(adam_steps.p, 0, lay.P * 4)); return; }
		if (steps32) { HIP_CHECK(hipMemcpy(adam_steps.p, in, lay.P * 4, hipMemcpyHostToDevice)); return; }
		std::vector<uint16_t> h(lay.P);
		for (size_t i = 0; i < lay.P; ++i) h[i] = (uint16_t)std::min<uint32_t>(in[i], 0xffffu);
		HIP_CHECK(hipMemcpy(adam_steps.p, h.data(), lay.P * 2, hipMemcpyHostToDevice));
	}
	AdamTranspose adam_transpose() const {
		const Layout& l = lay;
		AdamTranspose t{};
		t.n = 5;
		const uint32_t off[5] = {l.off_d0, l.off_d1, l.off_r0, l.off_r1, l.off_r2}, rows[5] = {l.W, 16, l.W, l.W, 16}, cols[5] = {l.din, l.W, 48, l.W, l.W};
		half_t* dst[5] = {(half_t*)mlp.d0T, (half_t*)mlp.d1T, (half_t*)mlp.r0T, (half_t*)mlp.r1T, (half_t*)mlp.r2T};
		for (int j = 0; j < 5; ++j) { t.off[j] = off[j]; t.rows[j] = rows[j]; t.cols[j] = cols[j]; t.dst[j] = dst[j]; }
		for (int k = 0; k < 48; ++k) t.inv[k] = -1;
		for (uint32_t q = 0; q < din_perm.din && q < 48; ++q) if (din_perm.p[q] >= 0 && din_perm.p[q] < 48) t.inv[din_perm.p[q]] = (int32_t)q;
		t.d0p = (half_t*)mlp.d0p; t.d0Tp = (half_t*)mlp.d0Tp; t.din = din_perm.din; t.W = din_perm.W;
		return t;
	}

	// each phase mark also closes the previous roctx range and opens the phase's (host enqueue spans of the step's kernel
	// groups in `rocprofv3 --marker-trace`; the calls are no-ops without a tool attached)
	int rx_open = -1;
	void mark(int i) {
		static const char* const names[N_PHASES] = {"neus:occupancy", "neus:march", "neus:inference", "neus:loss", "neus:encode",
		                                            "neus:mlp", "neus:wgrad", "neus:scatter", "neus:exchange", "neus:optimizer"};
		if (profiling) HIP_CHECK(hipEventRecord(ev[prof_par][i].get(), stream));
		if (rx_open >= 0) roctxRangePop();
		rx_open = i < N_PHASES ? i : -1;
		if (rx_open >= 0) roctxRangePushA(names[i]);
	}
	// Inference timing (neus_testbed_set_infer_timing): every pre-compaction network launch of the step (the one pass, or
	// each progressive round's k_nerf_infer) records a pair of hipEvents at its kernel's start and end (launched through
	// hipExtLaunchKernelGGL: events recorded between launches also counted the dispatch gap and overlapped the previous
	// kernel's tail, 182 against the kernel trace's 146 us per launch), summed per step after the step (host waits: timing
	// passes only, never the bench's timed region)
	bool infer_timing = false;
	static constexpr int IT_MAX = 16;
	Event it_ev[2 * IT_MAX];
	int it_n = 0;
	double it_ms = 0.0;
	uint64_t it_launches = 0, it_steps = 0;
	void it_arm() {
		if (!infer_timing || it_n + 2 > 2 * IT_MAX) return;
		for (int k = 0; k < 2; ++k) ensure_event(it_ev[it_n + k]);
		g_infer_ev[0] = it_ev[it_n].get();
		g_infer_ev[1] = it_ev[it_n + 1].get();
		it_n += 2;
	}
	void it_collect() {
		if (!infer_timing || it_n < 2) { it_n = 0; return; }
		HIP_CHECK(hipEventSynchronize(it_ev[it_n - 1].get()));
		for (int i = 0; i + 1 < it_n; i += 2) {
			float ms = 0.f;
			HIP_CHECK(hipEventElapsedTime(&ms, it_ev[i].get(), it_ev[i + 1].get()));
			it_ms += ms;
			++it_launches;
		}
		++it_steps;
		it_n = 0;
	}

	// ------------------------------------------------------------ rendering (render_to_cpu, python_api.cu:123-169)
	// NerfTracer::init_rays_from_camera + trace (testbed_nerf.cu:2397-2600) once per spp, accumulated in linear
	// colour. The alive count is read back every iteration (it sets the steps per iteration, as the reference).
	uint32_t render(const NeusRenderRequest& rq, float* host_rgba) {
		if (!have_net) throw std::runtime_error("render: no network (reload_network first)");
		if (rq.width <= 0 || rq.height <= 0) throw std::runtime_error("render: empty resolution");
		const uint64_t n64 = (uint64_t)rq.width * (uint64_t)rq.height;
		if (n64 > (1ull << 26)) throw std::runtime_error("render: at most 2^26 pixels per call");
		const uint32_t n = (uint32_t)n64;
		RenderCamera cam{};
		cam.width = (uint32_t)rq.width; cam.height = (uint32_t)rq.height;
		if (rq.training_view >= 0) {
			if ((uint32_t)rq.training_view >= ds.n_images) throw std::runtime_error("render: training_view out of range");
			const uint32_t v = (uint32_t)rq.training_view;
			std::memcpy(cam.xform, &host_xform[12 * v], 12 * sizeof(float));
			// set_camera_to_training_view: relative focal length = focal / res[fov_axis = 1], rescaled to the render height
			for (int k = 0; k < 2; ++k) {
				cam.focal[k] = host_focal[2 * v + k] / (float)host_res[2 * v + 1] * (float)rq.height;
				cam.screen_center[k] = host_pp[2 * v + k];
			}
		} else {
			std::memcpy(cam.xform, rq.xform, sizeof(cam.xform));
			cam.focal[0] = rq.focal[0]; cam.focal[1] = rq.focal[1];
			cam.screen_center[0] = rq.screen_center[0]; cam.screen_center[1] = rq.screen_center[1];
		}
		hipStream_t s = stream;
		const size_t rb = render_ray_bytes();
		r_rays[0].alloc(n * rb); r_rays[1].alloc(n * rb);
		r_flags.alloc(n); r_base.alloc(n); r_alive.alloc(1);
		r_coords.alloc((size_t)n * MAX_STEPS_INBETWEEN_COMPACTION * COORD_W);
		r_out.alloc((size_t)n * MAX_STEPS_INBETWEEN_COMPACTION * OUT_W);
		r_frame.alloc(n); r_accum.alloc(n);
		const size_t sb = scan_temp_bytes(n);
		if (sb > r_scan_bytes || !r_scan_tmp.p) { r_scan_tmp.alloc(sb + 256); r_scan_bytes = sb; scan_temp_reset(s, r_scan_tmp.p); }
		const MlpPtrs& w = rq.use_ema ? mlp_ema : mlp;
		const half_t* grid = (rq.use_ema ? ema_h.p : params_h.p) + lay.grid_off;
		if (rq.use_ema) { sync_ema_h(); prepare_weights_for(mlp_ema); }
		const uint32_t valid = valid_level_at(enc_step);
		const uint32_t spp = std::max(1u, rq.spp);
		// m_use_delta (prepare_for_test): the network sees the sample positions through the DeltaNetwork
		const bool use_delta = render_delta && cur_frame >= 1;
		if (use_delta) { r_coords_def.alloc((size_t)n * MAX_STEPS_INBETWEEN_COMPACTION * COORD_W); launch_delta_prepare(s, delta.p); }
		uint32_t iters = 0;
		for (uint32_t sp = 0; sp < spp; ++sp) {
			const uint32_t offs_index = rq.snap_to_pixel_centers ? 0 : sp;
			ld_pixel_offset(offs_index, cam.pixel_offset);
			launch_render_init(s, cam, sp, ds, bitfield.p, bf_lin.p, r_rays[0].p, r_frame.p);
			uint32_t n_alive = n, cur = 0;
			iters = 0;
			for (uint32_t i = 1; i < MARCH_ITER;) {
				launch_render_compact(s, n_alive, r_rays[cur].p, r_flags.p, r_base.p, r_rays[cur ^ 1].p, r_alive.p, r_scan_tmp.p, r_scan_bytes);
				cur ^= 1;
				HIP_CHECK(hipMemcpyAsync(pinned.get() + 32, r_alive.p, 4, hipMemcpyDeviceToHost, s));
				HIP_CHECK(hipStreamSynchronize(s));
				std::memcpy(&n_alive, pinned.get() + 32, 4);
				if (n_alive == 0) break;
				const uint32_t n_steps = std::min(MAX_STEPS_INBETWEEN_COMPACTION, std::max(1u, n / n_alive));
				launch_render_gen(s, n_alive, n_steps, ds, bitfield.p, bf_lin.p, r_rays[cur].p, r_coords.p);
				const uint32_t n_el = n_alive * n_steps;
				const float* c_in = r_coords.p;
				if (use_delta) { launch_delta_apply(s, nullptr, n_el, COORD_W, r_coords.p, r_coords_def.p, delta.p); c_in = r_coords_def.p; }
				launch_nerf_infer(s, lay.L, lay.W, nullptr, n_el, c_in, gl, valid, grid, w, r_out.p,
				                  std::max<uint32_t>(1, std::min<uint32_t>((n_el + 127) / 128, 8192)));
				launch_render_composite(s, n_alive, n_steps, r_coords.p, r_out.p, cos_anneal(), rq.min_transmittance, ds.target.mode == 2,
				                        r_rays[cur].p, r_frame.p);
				i += n_steps;
				++iters;
			}
			launch_render_accumulate(s, n, sp, r_frame.p, r_accum.p);
		}
		HIP_CHECK(hipMemcpyAsync(host_rgba, r_accum.p, (size_t)n * 16, hipMemcpyDeviceToHost, s));
		HIP_CHECK(hipStreamSynchronize(s));
		return iters;
	}

	// ------------------------------------------------------------ marching cubes (testbed_nerf.cu:4096-4226)
	// get_density_on_grid: raw SDF of the inference (EMA) weights at every grid point, written to dst.
	void sdf_on_grid(const uint32_t res[3], const float amin[3], const float amax[3], float* dst) {
		if (!have_net) throw std::runtime_error("sdf_on_grid: no network");
		sync_ema_h(); prepare_weights_for(mlp_ema);
		const uint64_t n = (uint64_t)res[0] * res[1] * res[2];
		const uint32_t valid = valid_level_at(enc_step);
		const bool use_delta = render_delta && cur_frame >= 1;
		if (use_delta) launch_delta_prepare(stream, delta.p);
		for (uint64_t off = 0; off < n; off += (1ull << 30)) {
			const uint32_t cnt = (uint32_t)std::min<uint64_t>(n - off, 1ull << 30);
			launch_sdf_grid(stream, lay.L, lay.W, res, amin, amax, ds.aabb_min, ds.aabb_max, off, cnt, gl, valid, ema_h.p + lay.grid_off, mlp_ema,
			                dst + off, use_delta ? delta.p : nullptr);
		}
	}
	// Testbed::marching_cubes: SDF grid (unless a device density grid is given), then the deterministic
	// count / scan / emit passes of mc.hip. The mesh stays on the device until get_mesh.
	void marching_cubes(const int32_t res_in[3], const float amin[3], const float amax[3], float thresh, const float* density_dev) {
		uint32_t res[3];
		for (int k = 0; k < 3; ++k) {
			if (res_in[k] < 2) throw std::runtime_error("marching_cubes: resolution must be >= 2");
			res[k] = density_dev ? (uint32_t)res_in[k] : next_multiple((uint32_t)res_in[k], 16u);  // testbed_nerf.cu:4176-4178
		}
		const uint64_t n = (uint64_t)res[0] * res[1] * res[2];
		if (n >= (1ull << 36)) throw std::runtime_error("marching_cubes: grid too large");
		hipStream_t s = stream;
		const float* d = density_dev;
		if (!d) {
			mc_density.alloc(n);
			sdf_on_grid(res, amin, amax, mc_density.p);
			d = mc_density.p;
		}
		const uint32_t nc = mc_n_chunks(res);
		mc_cnt.alloc(4 * (size_t)nc + 4);
		uint32_t *cv = mc_cnt.p, *ct = cv + nc, *ov = ct + nc, *ot = ov + nc;
		launch_mc_count(s, res, amin, amax, thresh, d, cv, ct);
		const size_t sb = scan_temp_bytes(nc);
		if (sb > mc_scan_bytes || !mc_scan_tmp.p) { mc_scan_tmp.alloc(sb + 256); mc_scan_bytes = sb; scan_temp_reset(s, mc_scan_tmp.p); }
		launch_exclusive_scan(s, mc_scan_tmp.p, mc_scan_bytes, cv, ov, nc);
		launch_exclusive_scan(s, mc_scan_tmp.p, mc_scan_bytes, ct, ot, nc);
		uint32_t last[4];
		HIP_CHECK(hipMemcpyAsync(pinned.get() + 40, cv + nc - 1, 4, hipMemcpyDeviceToHost, s));
		HIP_CHECK(hipMemcpyAsync(pinned.get() + 41, ct + nc - 1, 4, hipMemcpyDeviceToHost, s));
		HIP_CHECK(hipMemcpyAsync(pinned.get() + 42, ov + nc - 1, 4, hipMemcpyDeviceToHost, s));
		HIP_CHECK(hipMemcpyAsync(pinned.get() + 43, ot + nc - 1, 4, hipMemcpyDeviceToHost, s));
		HIP_CHECK(hipStreamSynchronize(s));
		std::memcpy(last, pinned.get() + 40, 16);
		const uint64_t nv = (uint64_t)last[2] + last[0], nt = (uint64_t)last[3] + last[1];
		if (nv >= (1ull << 32) || 3 * nt >= (1ull << 32)) throw std::runtime_error("marching_cubes: mesh exceeds 32-bit indices");
		mesh_v.alloc(3 * std::max<uint64_t>(nv, 1));
		mc_vidx.alloc(n);
		mesh_f.alloc(3 * std::max<uint64_t>(nt, 1));
		launch_mc_emit(s, res, amin, amax, thresh, d, ov, ot, mesh_v.p, mc_vidx.p, mesh_f.p);
		if (!density_dev) launch_mesh_unmove(s, (uint32_t)nv, ds.motion, mesh_v.p);  // transform_mesh_with_6d
		HIP_CHECK(hipStreamSynchronize(s));
		mesh_nv = (uint32_t)nv; mesh_nt = (uint32_t)nt;
	}

	// compute_mesh_vertex_colors (testbed_nerf.cu:4071-4094): network colour (inference weights) at each vertex,
	// looking outward from the aabb centre; sRGB (the network is trained on sRGB targets).
	void mesh_colors(float* host_rgb) {
		if (!mesh_nv) return;
		sync_ema_h(); prepare_weights_for(mlp_ema);
		Dev<float> c; Dev<half_t> o;
		c.alloc((size_t)mesh_nv * COORD_W); o.alloc((size_t)mesh_nv * OUT_W);
		launch_mesh_coords(stream, mesh_nv, mesh_v.p, ds, c.p);
		if (render_delta && cur_frame >= 1) {  // m_use_delta: the vertices go through the DeltaNetwork too
			launch_delta_prepare(stream, delta.p);
			launch_delta_apply(stream, nullptr, mesh_nv, COORD_W, c.p, c.p, delta.p);
		}
		launch_nerf_infer(stream, lay.L, lay.W, nullptr, mesh_nv, c.p, gl, valid_level_at(enc_step), ema_h.p + lay.grid_off, mlp_ema, o.p,
		                  std::max<uint32_t>(1, std::min<uint32_t>((mesh_nv + 127) / 128, 8192)));
		std::vector<half_t> h((size_t)mesh_nv * OUT_W);
		HIP_CHECK(hipMemcpyAsync(h.data(), o.p, h.size() * sizeof(half_t), hipMemcpyDeviceToHost, stream));
		HIP_CHECK(hipStreamSynchronize(stream));
		for (size_t i = 0; i < mesh_nv; ++i)
			for (int k = 0; k < 3; ++k) host_rgb[3 * i + k] = 1.0f / (1.0f + std::exp(-(float)h[i * OUT_W + k]));
	}

	// ------------------------------------------------------------ one Testbed::train step (testbed.cu:2640-2736)
	void train_step() {
		if (abort_pending) check_abort();
		train_step_body();
	}
	// The witness word (64 B, allocated at the first step that needs it) set to the sentinel for the step being issued
	uint32_t* arm_abort_word() {
		if (!abort_word) abort_word = make_pinned<volatile uint32_t>(16, hipHostMallocCoherent | hipHostMallocMapped);
		*abort_word.get() = ~0u;
		return (uint32_t*)abort_word.get();
	}
	// The last issued step's march-cut witness (opt.march_cut): when it aborted, its state changes were withheld on the
	// device; the host state goes back to its start and the step runs again with the full march.
	void check_abort() {
		abort_pending = false;
		uint32_t a = 0;
		if (abort_direct) {
			// one rank: k_loss_grad stored the word to host-coherent memory (sentinel ~0 before the step): poll it, and
			// after a bounded spin wait for the step's stream (the kernel has then run)
			const volatile uint32_t* w = abort_word.get();
			for (uint32_t k = 0; k < (1u << 22) && *w == ~0u; ++k) __builtin_ia32_pause();
			if (*w == ~0u) HIP_CHECK(hipStreamSynchronize(stream));
			a = *w;
			if (a == ~0u) throw std::runtime_error("march cut: the witness word was not written");
		} else {
			HIP_CHECK(hipEventSynchronize(ev_abort.get()));
			std::memcpy(&a, pinned.get() + 100, 4);
		}
		if (!a) return;
		// this testbed's streams drained (not the device's: another rank of an in-process group may share it)
		for (hipStream_t q : {stream_own.get(), aux_stream.get(), la_stream.get(), x.stream()})
			if (q) HIP_CHECK(hipStreamSynchronize(q));
		la_pending = false;
		la_deferred = nullptr;
		const uint32_t left = call_left;
		const StepSnap s0 = snap[0], s1 = snap[1];
		const bool prev_mc = mc_hist[1];
		training_step = s0.training_step; canonical_step = s0.canonical_step; adam_step = s0.adam_step; call_left = s0.call_left;
		enc_step = s0.enc_step; lr_factor = s0.lr_factor; rng = s0.rng;
		la_steps = s0.la_steps; cut_steps = s0.cut_steps; adam_split_steps = s0.adam_split_steps; mcut_steps = s0.mcut_steps;
		StepState h{};
		HIP_CHECK(hipMemcpy(&h, st.p, sizeof(h), hipMemcpyDeviceToHost));
		if (prev_mc) {
			// the step before was cut too: its requested count in full (its rays again, from its rng and its n_rays_total), so
			// that this step's cap is the reference's exactly (the bitfield is the one it marched: no occupancy update since)
			StepState t = h;
			t.n_rays_total = h.n_rays_total - h.rays_per_batch * x.world();
			st_recount.alloc(1);
			HIP_CHECK(hipMemcpy(st_recount.p, &t, sizeof(t), hipMemcpyHostToDevice));
			launch_march_count(stream, MAX_RAYS, max_samples, st_recount.p, dp_info(), ds, bitfield.p, bf_lin.p, s1.rng.state, s1.rng.inc,
			                   rays.p, startt.p, nreq.p, mwork, nullptr, 0, opt.ray_cull ? occ_bbox.p : nullptr);
			launch_march_write(stream, MAX_RAYS, st_recount.p, ds, rays.p, mwork, nreq.p, base.p, numsteps.p, coords.p, nullptr, max_samples,
			                   scan_tmp.p, nullptr, 0);
			HIP_CHECK(hipStreamSynchronize(stream));
			HIP_CHECK(hipMemcpy(&t, st_recount.p, sizeof(t), hipMemcpyDeviceToHost));
			const uint32_t before = t.numsteps_counter;
			h.measured_before = before;
			h.max_inference = (std::min(before, max_samples) + 127u) / 128u * 128u;
		}
		h.mi_lb = 0;
		h.cut_abort = 0;
		HIP_CHECK(hipMemcpy(st.p, &h, sizeof(h), hipMemcpyHostToDevice));
		HIP_CHECK(hipMemset(cutw.p + CW_ABORT, 0, 2 * sizeof(uint32_t)));
		snap[0] = s1;
		mc_hist[0] = prev_mc;
		++mcut_reruns;
		force_full = true;
		try { train_step_body(); } catch (...) { force_full = false; throw; }
		force_full = false;
		call_left = left;
	}
	void train_step_body() {
		if (!have_net) throw std::runtime_error("train: no network (reload_network first)");
		hipStream_t s = stream;
		snap[1] = snap[0];
		snap[0] = StepSnap{training_step, canonical_step, adam_step, call_left, enc_step, lr_factor, rng, la_steps, cut_steps, adam_split_steps, mcut_steps};
		mc_hist[1] = mc_hist[0];
		mc_hist[0] = false;
		x.check();
		if (x.unverified()) { health_buf.alloc(4); x.verify_uniform(health_buf.p + 2); }
		// the readback of 16 steps back (long done on the device) is checked at this step boundary, before anything of
		// this step is queued: a health failure (all-reduced, so every rank sees it) stops every rank on the same step
		// with no collective half-issued and no step half-applied; the host stays at most 16 steps ahead of the device
		if (readback_at(training_step) && loss_pending) consume_loss();
		// dynamic scenes (testbed.cu:2651-2712): progressive levels count from the end of the global-movement
		// phase; at its end canonical training starts (and the movement keeps training when finetuned)
		const bool dyn = cur_frame >= 1;
		if (dyn && training_step == gm_steps()) {
			train_canonical = true;
			if (!cfg.finetune_global_movement) train_delta = false;
			if (cfg.reset_density_grid_after_global_movement) {
				HIP_CHECK(hipMemsetAsync(density_grid.p, 0, density_grid.n * 4, s));
				density_grid_ema_step = 0;
			}
		}
		const bool use_delta = dyn && train_delta;
		const bool la_have = la_pending;
		la_pending = false;
		render_delta = use_delta;  // m_nerf_network->m_use_delta follows the training step (testbed.cu:2704-2710)
		enc_step = dyn ? (int)training_step - (int)gm_steps() : (int)training_step;
		const uint32_t valid = valid_level_at(enc_step);
		if (use_delta) launch_delta_prepare(s, delta.p);
		// every decision about this step's shape, from the host state as it stands here (step_plan.h); a step whose samples
		// came from the previous step's lookahead takes the sampling that lookahead planned and issued
		StepFacts facts;
		facts.step = training_step; facts.canonical_step = canonical_step; facts.left = call_left; facts.next_in_call = la_next_in_call;
		facts.dyn = dyn; facts.use_delta = use_delta; facts.train_canonical = train_canonical;
		facts.fixed_rays = cfg.fixed_rays_per_batch; facts.profiling = profiling;
		facts.balanced = mwork.balanced; facts.lanes_per_ray = mwork.lanes_per_ray; facts.cone_angle = ds.cone_angle;
		facts.occ_cells = GRID3 * (max_cascade + 1);
		facts.force_full = force_full; facts.prev_mcut = mc_hist[1]; facts.loss_pending = loss_pending;
		facts.dbg_hook = dbg_lds_fill || g_dbg_lds_fill != 0 || g_dbg_xcd_shift != 0;
		facts.x_on = x.on(); facts.x_overlap = x.overlap();
		const StepPlan p = la_have ? plan_step(opt, facts, la_plan) : plan_step(opt, sched, facts);
		const SamplingPlan& sp = p.sampling;
		mark(0);
		if (p.occ_update) occ_update(p.occ_uniform, p.occ_nonuniform, valid, use_delta);
		// ---- train_nerf_step (testbed_nerf.cu:3723-4001)
		if (training_step == 0 || canonical_step == 0) HIP_CHECK(hipMemsetAsync(&st.p->n_rays_total, 0, 4, s));
		const uint32_t world = x.world();
		const DPInfo dp = dp_info();  // (n_kept, n_rays_with_samples: zeroed by k_ray_gen)
		mark(1);
		const RaySort rsort{rs_hist.p, rs_off.p, rs_key.p, rs_perm.p, chunk_cnt.p + RS_N_PERM};
		if (la_have) {
			if (p.occ_update) throw std::runtime_error("train: lookahead issued before an occupancy update");
			++la_steps;
			if (opt.la_stat && la_stat_used % 4 == 2) HIP_CHECK(hipEventRecord(la_stat_next(), s));
			HIP_CHECK(hipStreamWaitEvent(s, ev_la_done.get(), 0));  // this step's samples came from the previous step's lookahead
			if (opt.la_stat && la_stat_used % 4 == 3) HIP_CHECK(hipEventRecord(la_stat_next(), s));
		}
		if (!la_have) issue_march(s, dp, rng, sp, scan_tmp.p);
		mc_hist[0] = sp.mcut;
		if (sp.cut) ++cut_steps;
		if (sp.mcut) ++mcut_steps;
		mark(2);
		// DeltaNetwork forward on the samples (nerf_network.h:162-182); the loss keeps the undeformed records
		const float* c_in = coords.p;
		if (use_delta) { launch_delta_apply(s, &st.p->n_kept, max_samples, COORD_W, coords.p, coords_def.p, delta.p); c_in = coords_def.p; }
		LossParams lp{};
		lp.loss_scale = LOSS_SCALE; lp.ek_w = cfg.ek_loss_weight; lp.mask_w = cfg.mask_loss_weight; lp.cos_anneal = cos_anneal();
		lp.max_compacted = batch; lp.rng_state = rng.state; lp.rng_inc = rng.inc; lp.jt = jump_table();
		lp.abort_w = cutw.p + CW_ABORT; lp.abort_slot = training_step & 1u;
		if (p.risky && !x.on()) {
			// one rank: the word goes straight from k_loss_grad to host memory (no copy, no event on the step's streams)
			lp.abort_host = arm_abort_word();
		}
		lp.dbg_fence = opt.dbg_loss_fence ? 1u : 0u;
		const LossWork w = loss_work(base.p);
		if (sp.progressive) {
			// rounds of per-ray chunks, each: network on the round's samples, alpha, the recurrence continued (march.hip);
			// the "infer" phase mark then covers the composite as well
			uint32_t e0 = 0;
			const uint32_t nch = sp.nch;
			for (uint32_t k = 0; k < nch; ++k) {
				const uint32_t e1 = k + 1 < nch ? sp.ends[k] : 0xffffffffu;
				const uint32_t e2 = k + 2 < nch ? sp.ends[k + 1] : 0xffffffffu;
				// the loss's alpha terms in the inference epilogue (k_loss_alpha's work on the round's samples)
				const InferAlpha ia{w.sa, w.ekt, lp.cos_anneal, ds.cone_angle == 0.0f ? 1u : 0u, nullptr, sp.sorted_rays ? 8u : 0u};
				it_arm();
				launch_nerf_infer(s, lay.L, lay.W, chunk_cnt.p + k, 0, c_in, gl, valid, params_h.p + lay.grid_off, mlp, net_out.p, 8192, chunk_list.p,
				                  use_delta ? nullptr : &ia);
				if (use_delta) launch_loss_alpha_list(s, max_samples, chunk_cnt.p + k, chunk_list.p, coords.p, net_out.p, lp.cos_anneal, w, ds.cone_angle == 0.0f);
				const bool more = k + 1 < nch;
				// the cut after round 0 (the rays of the later rounds are then all at or before it: each round continues
				// only the rays of the round before it)
				const bool cut_k = sp.cut && k == 0 && more;
				launch_loss_scan_chunk(s, MAX_RAYS, numsteps.p, w, ccount.p, e0, e1, e2, more && !cut_k ? chunk_list.p : nullptr, chunk_cnt.p + k + 1,
				                       k ? open_rays[(k - 1) & 1].p : (sp.sorted_rays ? rs_perm.p : nullptr),
				                       k ? chunk_cnt.p + OPEN_CNT + k - 1 : (sp.sorted_rays ? rsort.n_perm : nullptr),
				                       more ? (cut_k ? open_raw.p : open_rays[k & 1].p) : nullptr,
				                       more ? chunk_cnt.p + (cut_k ? RAW_CNT : OPEN_CNT) + k : nullptr, p.scan_group);
				if (cut_k) {
					// the cut after this round (cbase as the scan's scratch: the compaction rewrites it after the rounds), then
					// the next round's rays and samples from the open rays at or before it
					// a cut march's step: pass B (the slots past the estimate) was not marched, so it is skipped; pass A's
					// slots must reach the batch, or the step is re-run (the witness word, set by the cut below)
					const bool split_b = p.split && !sp.mcut;
					if (split_b) {
						// pass A was the rays below the estimate: its cut, then pass B (empty when the cut lies in pass A's slots)
						launch_scan_prog_cut(s, scan_tmp.p, ccount.p, cbase.p, MAX_RAYS, batch, cutw.p, 0, nullptr);
						const InferAlpha iab{w.sa, w.ekt, lp.cos_anneal, ds.cone_angle == 0.0f ? 1u : 0u, nullptr, 8u};
						it_arm();
						launch_nerf_infer(s, lay.L, lay.W, cutw.p + CW_LENB_EFF, 0, c_in, gl, valid, params_h.p + lay.grid_off, mlp, net_out.p, 8192,
						                  chunk_list.p + max_samples, &iab);
						launch_loss_scan_chunk(s, MAX_RAYS, numsteps.p, w, ccount.p, 0, e1, e2, nullptr, nullptr, rs_perm.p + MAX_RAYS,
						                       cutw.p + CW_NB_EFF, open_raw.p, chunk_cnt.p + RAW_CNT + k, p.scan_group);
					}
					launch_scan_prog_cut(s, scan_tmp.p, ccount.p, cbase.p, MAX_RAYS, batch, cutw.p, 1, split_b ? chunk_cnt.p : nullptr,
					                     sp.mcut ? cutw.p + CW_ABORT + (training_step & 1u) : nullptr);
					launch_prog_next(s, MAX_RAYS, open_raw.p, chunk_cnt.p + RAW_CNT + k, numsteps.p, cutw.p + CW_CUT, e1, e2, chunk_list.p,
					                 chunk_cnt.p + k + 1, open_rays[k & 1].p, chunk_cnt.p + OPEN_CNT + k);
				}
				e0 = e1;
			}
			mark(3);
		} else {
			const InferAlpha ia{w.sa, w.ekt, lp.cos_anneal, ds.cone_angle == 0.0f ? 1u : 0u, w.n_long};
			it_arm();
			launch_nerf_infer(s, lay.L, lay.W, &st.p->n_kept, 0, c_in, gl, valid, params_h.p + lay.grid_off, mlp, net_out.p, 8192, nullptr,
			                  use_delta ? nullptr : &ia);
			mark(3);
			if (use_delta) launch_loss_alpha(s, max_samples, st.p, coords.p, net_out.p, lp.cos_anneal, w, ds.cone_angle == 0.0f);
			launch_loss_scan_ray(s, MAX_RAYS, numsteps.p, w, ccount.p);
		}
		launch_exclusive_scan(s, scan_tmp.p, scan_tmp_bytes, ccount.p, cbase.p, MAX_RAYS);
		launch_loss_ray(s, MAX_RAYS, st.p, dp, ds, lp, numsteps.p, ccount.p, cbase.p, w, loss.p, ek.p, mask.p);
		launch_loss_grad(s, max_samples, st.p, dp, lp, coords.p, net_out.p, numsteps.p, w, coords_c.p, dL_dout.p);
		if (opt.dbg_loss_replay) {  // development (NEUS_DBG_LOSS_REPLAY=1): the same launch again, into separate outputs, and
			                     // copies of the loss-gradient kernel's inputs as they were right after it
			dbg_co.alloc((size_t)batch * COORD_W); dbg_dl.alloc((size_t)batch * OUT_W);
			launch_loss_grad(s, max_samples, st.p, dp, lp, coords.p, net_out.p, numsteps.p, w, dbg_co.p, dbg_dl.p);
			const std::pair<const void*, size_t> src[DBG_SNAP_N] = {
				{l_sa.p, l_sa.n * 16}, {l_ekt.p, l_ekt.n * 4}, {l_ck4.p, l_ck4.n * 16}, {l_cke.p, l_cke.n * 4}, {l_racc.p, l_racc.n * 16},
				{l_rgr.p, l_rgr.n * 16}, {l_rT.p, l_rT.n * 4}, {l_rek.p, l_rek.n * 4}, {ccount.p, ccount.n * 4}, {net_out.p, net_out.n * 2},
				{coords.p, coords.n * 4}, {base.p, base.n * 4}, {numsteps.p, numsteps.n * 4}, {cmap.p, cmap.n * 4}, {nreq.p, nreq.n * 4}};
			for (int k = 0; k < DBG_SNAP_N; ++k) {
				dbg_snap[k].alloc(src[k].second);
				HIP_CHECK(hipMemcpyAsync(dbg_snap[k].p, src[k].first, src[k].second, hipMemcpyDeviceToDevice, s));
			}
		}
		// ---- the step's counters over the ranks (data parallel): the compacted count and the rays with samples, summed
		// right after the loss into StepState::compacted_global / rays_ws_global (compacted_counter stays this rank's
		// training batch for the backward). On the communication stream with the overlapped exchange, so the backward
		// does not wait for it; the gradients' collectives follow on the same stream, in the same order on every rank.
		x.reset_step_bytes();
		hipStream_t cs = s;  // the stream the counters (and the lookahead's start) are ordered on
		Event* xt = x.timing_slot();
		if (xt) HIP_CHECK(hipEventRecord(xt[0].get(), s));
		if (x.on()) {
			cs = p.xo ? x.gated() : stream;
			x.begin();
			x.allreduce_u32(&st.p->compacted_global, 3, cs);  // (+ cut_abort: every rank re-runs the step, or none)
			x.end();
		}
		if (p.risky) {
			abort_pending = true;
			abort_direct = !x.on();
		}
		// ---- lookahead: the next step's ray sampling beside this step's backward (opt.lookahead; see the members)
		const StepCounterArgs sca{st.p, batch, max_samples, world, cfg.fixed_rays_per_batch, sp.progressive ? chunk_cnt.p : nullptr, sp.nch};
		bool counters_done = false;
		// with a group, the all-reduced word goes to the host from the step counters' launch that the lookahead puts right
		// behind the exchange (a system-scope store, as k_loss_grad's at one rank); otherwise by a copy and an event
		uint32_t* abort_host_ctr = nullptr;
		if (p.risky && x.on() && p.la_go) {
			abort_host_ctr = arm_abort_word();
			abort_direct = true;
		}
		if (p.risky && !abort_direct) {
			// the all-reduced abort word to the host, off the step's stream (the backward starts at once)
			if (!ev_abort) {
				ev_abort = make_event(hipEventDisableTiming);
				ev_abort_src = make_event(hipEventDisableTiming);
			}
			HIP_CHECK(hipEventRecord(ev_abort_src.get(), cs));
			HIP_CHECK(hipStreamWaitEvent(aux_stream.get(), ev_abort_src.get(), 0));
			*(volatile uint32_t*)(pinned.get() + 100) = ~0u;
			HIP_CHECK(hipMemcpyAsync(pinned.get() + 100, &st.p->cut_abort, 4, hipMemcpyDeviceToHost, aux_stream.get()));
			HIP_CHECK(hipEventRecord(ev_abort.get(), aux_stream.get()));
			abort_pending = true;
		}
		{
			if (p.la_go) {
				// the host's StepState readback first (its place in the step without the lookahead: nothing it reads is
				// written between here and there - the ranks' counts are already summed), then the step counters the next
				// step's sampling reads; both behind the counters' exchange (cs)
				if (p.get_loss) HIP_CHECK(hipMemcpyAsync(pinned.get() + 64, st.p, sizeof(StepState), hipMemcpyDeviceToHost, cs));
				launch_step_counters(cs, st.p, batch, max_samples, world, cfg.fixed_rays_per_batch, sca.eval_cnt, sca.n_eval, abort_host_ctr);
				counters_done = true;
				if (!la_stream) {
					// the lookahead stream at the lowest priority: the backward's workgroups are dispatched first and the march's
					// fill what they leave (1.154 -> 1.107 ms/step at the bench state; the default priority 1.139, the highest
					// 1.141: profiles/r05lap_lookahead_priority_ab.txt). opt.la_prio: -1 lowest, 0 default, 1 highest.
					const int want = opt.la_prio;
					int lo = 0, hi = 0;
					HIP_CHECK(hipDeviceGetStreamPriorityRange(&lo, &hi));  // (lo: least urgent, hi: most urgent; hi <= lo numerically)
					la_stream = want == 0 ? make_stream(hipStreamNonBlocking) : make_stream(hipStreamNonBlocking, want > 0 ? hi : lo);
					// (device-side hand-offs between the step's and the lookahead's kernels: no system-scope fence - its
					// L2 write-back held the step's stream ~6 us at the record; opt.ev_sysfence keeps it, for A/B)
					const unsigned fl = hipEventDisableTiming | (opt.ev_sysfence ? 0u : hipEventDisableSystemFence);
					ev_la_start = make_event(fl);
					ev_la_done = make_event(fl);
				}
				if (!scan_tmp_la.p || scan_tmp_la.n < scan_tmp_bytes + 256) {
					scan_tmp_la.alloc(scan_tmp_bytes + 256);
					scan_temp_reset(s, scan_tmp_la.p);
				}
				pcg32 r1 = rng;
				r1.advance();
				// The next step's sampling, planned here and used whole by that step. It is the plan that step would make for
				// itself: its facts are these with the counters moved on, and the schedule cannot change in between - only a
				// loss readback changes it, and la_go excludes a next step that starts with one (or with an occupancy update)
				// and a readback still pending on this one. One exception, as it always was: a re-run step (force_full) hands
				// its force_full on through next(), so the step after a re-run never cuts its march, where on its own it might.
				la_plan = plan_step(opt, sched, facts.next()).sampling;
				const SamplingPlan sp1 = la_plan;
				la_at = sp1.mcut ? opt.la_at_cut : opt.la_at_full;
				la_deferred = [this, cs, dp, r1, sp1] {
					hipStream_t ls = la_stream.get();
					HIP_CHECK(hipEventRecord(ev_la_start.get(), cs));
					HIP_CHECK(hipStreamWaitEvent(ls, ev_la_start.get(), 0));
					if (opt.la_stat) { la_stat_used -= la_stat_used % 4; HIP_CHECK(hipEventRecord(la_stat_next(), ls)); }
					issue_march(ls, dp, r1, sp1, scan_tmp_la.p);
					if (opt.la_stat) HIP_CHECK(hipEventRecord(la_stat_next(), ls));
					HIP_CHECK(hipEventRecord(ev_la_done.get(), ls));
				};
				if (cs != s) la_fire(0x7fffffff);  // (the communication stream: issued now, before the gradients' collectives queue there)
				la_fire(0);
				la_pending = true;
			}
		}
		// the rollover copies are made by the training encode (static scenes); the DeltaNetwork reads the whole batch first
		if (use_delta) launch_rollover(s, batch, st.p, coords_c.p, dL_dout.p);
		const EncodeRollover ro{&st.p->compacted_counter, batch, dL_dout.p, coords_c.p};
		// the canonical backward writes every gradient entry (weight tiles and variance by k_wgrad_reduce, every grid
		// entry by k_scatter_accum, zeros with no samples); the global-movement phase skips it: zero the buffer there
		if (!p.canon_opt) HIP_CHECK(hipMemsetAsync(grads.p, 0, (size_t)lay.P * 4, s));
		mark(4);
		// the overlapped exchange (p.xo): the canonical backward all-reduces its gradient ranges as they finish; opt.adam_overlap
		// (static scenes; one rank, or behind the overlapped exchange): the optimizer step in pieces beside the scatter
		AdamSplit asp{};
		if (p.a_over) asp.p = adam_params();
		if (use_delta) {
			// the training forward runs on the deformed batch; dL/d(position) feeds the DeltaNetwork backward
			launch_delta_apply(s, nullptr, batch, COORD_W, coords_c.p, coords_cdef.p, delta.p);
			tbuf.dpos = dpos.p;
			net_backward(&st.p->compacted_counter, &st.p->n_train, batch, coords_cdef.p, valid, dL_dout.p, grads.p, s, true, train_canonical, nullptr, p.xo);
			tbuf.dpos = nullptr;
		} else {
			net_backward(&st.p->compacted_counter, &st.p->n_train, batch, coords_c.p, valid, dL_dout.p, grads.p, s, true, train_canonical, &ro, p.xo,
			             p.a_over ? &asp : nullptr);
		}
		la_fire(99);  // (issued by now in any case)
		// DeltaNetwork gradient partial sums (the first half of its backward; the Adam step follows the exchange)
		if (use_delta) launch_delta_grad(s, &st.p->n_train, batch, coords_c.p, COORD_W, dpos.p, delta.p, delta_partial.p);
		mark(8);
		if (p.get_loss) {
			launch_sum_f32(s, scan_tmp.p, scan_tmp_bytes, loss.p, loss_sum.p + 0, MAX_RAYS);
			launch_sum_f32(s, scan_tmp.p, scan_tmp_bytes, ek.p, loss_sum.p + 1, MAX_RAYS);
			launch_sum_f32(s, scan_tmp.p, scan_tmp_bytes, mask.p, loss_sum.p + 2, MAX_RAYS);
			// this rank's health words, summed over the ranks with the loss sums (any rank's failure stops all of them)
			HIP_CHECK(hipMemcpyAsync(health_buf.p, &st.p->fail_flags, 4, hipMemcpyDeviceToDevice, s));
			HIP_CHECK(hipMemcpyAsync(health_buf.p + 1, scan_tmp.p + offsetof(ScanState, fail), 4, hipMemcpyDeviceToDevice, s));
		}
		if (x.on()) {
			// collective 1 (gradients; DeltaNetwork partials) and 3 (counters, loss scalars) of SURVEY §8(e). The gradient
			// of the grid levels past the progressive valid level is zero on every rank: the scatter writes no records there
			// and keeps that range zeroed (scatter_work_for's sc_zero_from / sc_zero_from_e invariant: every grid entry from
			// gl.offset[valid + 1] on holds 0 after the backward, on every rank), so only the MLP blocks, the active levels'
			// tables and the variance move. Overlapped: the gradients went out during the backward (net_backward).
			const size_t grid_act = 2 * (size_t)gl.offset[std::min(valid + 1, gl.n_levels)];
			if (xt) HIP_CHECK(hipEventRecord(xt[1].get(), s));  // the backward is done (and the loss sums, when logged)
			hipStream_t xs = p.xo ? x.gated() : stream;
			x.begin();
			if (!p.xo) {
				x.allreduce_f32(grads.p, (size_t)lay.grid_off + grid_act);
				x.allreduce_f32(grads.p + lay.var_off, lay.P - lay.var_off);
			}
			if (use_delta) x.allreduce_f32(delta_partial.p, delta_partial_floats(), false, xs);
			if (p.get_loss) { x.allreduce_f32(loss_sum.p, 3, false, xs); x.allreduce_u32(health_buf.p, 2, xs); }
			x.end();
			if (p.a_over) adam_issue(asp, lay.P, grads.p, false);  // the optimizer's last piece, behind the exchange
			if (xt) HIP_CHECK(hipEventRecord(xt[2].get(), xs));
			x.join();
		}
		if (p.get_loss) {
			if (loss_pending) consume_loss();  // (consumed at this step's start already; a restored state may leave one)
			HIP_CHECK(hipMemcpyAsync(pinned.get(), loss_sum.p, 3 * 4, hipMemcpyDeviceToHost, s));
			HIP_CHECK(hipMemcpyAsync(pinned.get() + 52, health_buf.p, 8, hipMemcpyDeviceToHost, s));
			if (!counters_done) HIP_CHECK(hipMemcpyAsync(pinned.get() + 64, st.p, sizeof(StepState), hipMemcpyDeviceToHost, s));
			HIP_CHECK(hipMemcpyAsync(pinned.get() + 48, scan_tmp.p + offsetof(ScanState, fail), 4, hipMemcpyDeviceToHost, s));
			HIP_CHECK(hipEventRecord(ev_loss.get(), s));
			loss_pending = true;
		}
		// the step-end counters ride on the Adam launch when the canonical optimizer steps (k_step_counters otherwise)
		// (progressive inference: the samples evaluated are the rounds' list lengths chunk_cnt[0, nch))
		if (!p.canon_opt && !counters_done) launch_step_counters(s, st.p, batch, max_samples, world, cfg.fixed_rays_per_batch, sca.eval_cnt, sca.n_eval);
		rng.advance();
		mark(9);
		// ---- optimizers (testbed_nerf.cu:3503-3508): the canonical trainer, the global-move trainer
		if (p.canon_opt && p.a_over) {
			++adam_split_steps;
			if (!counters_done) launch_step_counters(s, st.p, batch, max_samples, world, cfg.fixed_rays_per_batch, sca.eval_cnt, sca.n_eval);
			adam_join(asp, grads.p);
		} else if (p.canon_opt) {
			optimizer_step(grads.p, counters_done ? nullptr : &sca);
		}
		if (use_delta) {
			// ExponentialDecay of the globalmove optimizer (exponential_decay.h:61-80), its own step count
			if (delta_step == 0) delta_lr_factor = 1.f;
			if (delta_step >= cfg.gm_decay_start && (delta_step - cfg.gm_decay_start) % std::max(1u, cfg.gm_decay_interval) == 0)
				delta_lr_factor *= cfg.gm_decay_base;
			++delta_step;
			DeltaAdam a{cfg.gm_learning_rate * delta_lr_factor, cfg.gm_beta1, cfg.gm_beta2, cfg.gm_epsilon, LOSS_SCALE, 1u};
			launch_delta_step(s, delta_partial.p, delta.p, a);
		}
		mark(10);
		++training_step;
		// m_canonical_training_step (testbed_nerf.cu:3512-3527)
		if (!cfg.predict_global_movement || cur_frame == 0) canonical_step = training_step;
		else if (training_step >= gm_steps()) canonical_step = training_step - gm_steps();
		if (profiling) {
			HIP_CHECK(hipMemcpyAsync(&prof_st.get()[prof_par], st.p, sizeof(StepState), hipMemcpyDeviceToHost, stream));
			HIP_CHECK(hipEventRecord(ev_done[prof_par].get(), stream));
			prof_pending[prof_par] = true;
			prof_par ^= 1;
			if (prof_pending[prof_par]) accumulate_phases(prof_par);  // the previous step
		}
		it_collect();
	}

	// A step's ray sampling: ray generation + the march's two passes, the coordinate write (and round 0's list, unsorted
	// progressive), the spatial ray sort (sorted progressive); rng / sp: the step's own (train_step, or the
	// lookahead for the next step), scan: the look-back state of the stream it runs on.
	void issue_march(hipStream_t s, const DPInfo& dp, const pcg32& r, const SamplingPlan& sp, uint8_t* scan) {
		const Round0List r0{sp.ends[0], cbase.p, chunk_list.p, chunk_cnt.p, sp.nch + 1};
		MarchWork mw = mwork;
		if (sp.mcut) mw.est_cut = cutw.p + CW_EST;  // (the split sort's estimate: pass A's slots are the marched ones)
		mw.est_div = opt.march_cut_div;
		launch_march_count(s, MAX_RAYS, max_samples, st.p, dp, ds, bitfield.p, bf_lin.p, r.state, r.inc, rays.p, startt.p, nreq.p, mw,
		                   sp.progressive ? chunk_cnt.p : nullptr, RAW_CNT + sp.nch, opt.ray_cull ? occ_bbox.p : nullptr);  // list lengths + open-ray counts
		launch_march_write(s, MAX_RAYS, st.p, ds, rays.p, mw, nreq.p, base.p, numsteps.p, coords.p, nullptr, max_samples, scan,
		                   sp.progressive && !sp.sorted_rays ? &r0 : nullptr, dbg_lds_fill);
		const RaySort rsort{rs_hist.p, rs_off.p, rs_key.p, rs_perm.p, chunk_cnt.p + RS_N_PERM};
		const RaySplit split{cutw.p + CW_EST, ccount.p, cutw.p, MAX_RAYS, max_samples};
		if (sp.sorted_rays)
			launch_ray_sort(s, MAX_RAYS, numsteps.p, coords.p, sp.ends[0], rsort, chunk_list.p, chunk_cnt.p, scan, scan_tmp_bytes, sp.cut ? &split : nullptr);
	}

	LossWork loss_work(const uint32_t* rbase) {
		LossWork w{};
		w.sa = l_sa.p; w.ck4 = l_ck4.p; w.cke = l_cke.p; w.ekt = l_ekt.p; w.sample_ray = sample_ray.p; w.rbase = rbase; w.cmap = cmap.p;
		w.racc = l_racc.p; w.rT = l_rT.p; w.rgr = l_rgr.p; w.rek = l_rek.p;
		w.long_rays = long_rays.p; w.n_long = chunk_cnt.p + 16;
		return w;
	}

	void accumulate_phases(int par) {
		HIP_CHECK(hipEventSynchronize(ev_done[par].get()));
		for (int i = 0; i < N_PHASES; ++i) {
			float ms = 0.f;
			HIP_CHECK(hipEventElapsedTime(&ms, ev[par][i].get(), ev[par][i + 1].get()));
			phase_ms[i] += ms;
		}
		const StepState& h = prof_st.get()[par];
		phase_npre += h.n_kept;
		phase_ntrain += std::min(h.compacted_global / std::max(1u, x.world()), batch);
		++phase_steps;
		prof_pending[par] = false;
	}
	void flush_phases() {
		// oldest first: the set about to be reused is the older one
		if (prof_pending[prof_par]) accumulate_phases(prof_par);
		if (prof_pending[prof_par ^ 1]) accumulate_phases(prof_par ^ 1);
	}

	// raise = false (stats): record the health bits and the abort without throwing
	void consume_loss(bool raise = true) {
		if (!loss_pending) return;
		HIP_CHECK(hipEventSynchronize(ev_loss.get()));
		const float* const pin = pinned.get();  // (the readback copies are complete)
		const StepState* sst = (const StepState*)(pin + 64);
		const float measured = (float)sst->compacted_global / (float)x.world();
		const float scale = measured / (float)batch;
		last_loss = pin[0] * scale;
		ek_loss = pin[1] * scale;
		mask_loss = pin[2] * scale;
		last_rays_with_samples = sst->rays_ws_global;
		sched.on_readback(sst->compacted_global, sst->rays_ws_global, sst->n_kept, x.world());
		ray_loss = sst->rays_ws_global ? pin[0] * (float)(sst->rays_per_batch * x.world()) / (float)sst->rays_ws_global : 0.f;
		if (!loss_ema_init) { loss_scalar_ema = last_loss; loss_ema_init = true; }
		else loss_scalar_ema = 0.99f * loss_scalar_ema + 0.01f * last_loss;
		// health: a non-finite loss sum (a NaN / Inf flag on the loss; the sums are all-reduced, so every
		// rank raises it on the same step), and the zero-sample guard (testbed_nerf.cu:3542-3548: loss scalars 0,
		// training stops - the Python frame() loop reads training_aborted)
		if (!std::isfinite(pin[0]) || !std::isfinite(pin[1]) || !std::isfinite(pin[2])) { nonfinite = true; aborted = true; }
		if (sst->compacted_global == 0) {
			loss_scalar_ema = last_loss = ek_loss = mask_loss = 0.f;
			aborted = true;
		}
		loss_pending = false;
		// device health (sticky): a march that met a non-finite / negative t, a look-back scan that gave up waiting. Either
		// means corrupted sampling or compaction bases: training stops with an error instead of continuing on bad data.
		uint32_t scan_fail = 0, all[2] = {0, 0};
		std::memcpy(&scan_fail, pin + 48, 4);
		std::memcpy(all, pin + 52, 8);  // the health words summed over the ranks (this rank's alone at world 1)
		const uint32_t local = sst->fail_flags | (scan_fail ? STEP_FAIL_SCAN : 0u);
		// the words are sums over the ranks, not bit sets: word 0 sums the ranks' fail_flags (the march sets only
		// STEP_FAIL_MARCH_T there), word 1 the scans' give-up counters; any nonzero sum names its cause
		const uint32_t global = (all[0] ? STEP_FAIL_MARCH_T : 0u) | (all[1] ? STEP_FAIL_SCAN : 0u);
		health_raise(local | (x.on() ? global : 0u), local == 0 && x.on() && global != 0, raise);
	}
	uint32_t fail_seen = 0;
	void health_raise(uint32_t flags, bool other_rank = false, bool raise = true) {
		if (!flags) return;
		fail_seen |= flags;
		aborted = true;
		if (!raise) return;
		std::string m = other_rank ? "training step: device health check failed on another rank:" : "training step: device health check failed:";
		if (flags & STEP_FAIL_MARCH_T) m += " the occupancy march met a non-finite or negative t (corrupted sampling state);";
		if (flags & STEP_FAIL_SCAN) m += " a look-back scan gave up waiting for a predecessor tile (compaction bases are wrong);";
		throw std::runtime_error(m);
	}
};

// ============================================================ a testbed as an operator module's core (core.h)
namespace neus {
Core* core_create(int device) {
	NeusTestbed* t = new NeusTestbed(device);
	return new Core{*t, t->device, t->stream, t->cfg, t->lay, t->gl, t->swork, t->scan_tmp.p, t->scan_tmp_bytes, t->params_h.p, t->tbuf};
}
void core_destroy(Core* c) {
	if (!c) return;
	delete &c->tb;
	delete c;
}
void setup_network(NeusTestbed& tb, const NeusNetworkConfig& c, const float* geo, bool with_mlp) { tb.setup_network(c, geo, with_mlp); }
void core_set_levels(NeusTestbed& tb, const NeusNetworkConfig& c) { tb.cfg = c; tb.lay.L = c.n_levels; }
void prepare_weights(NeusTestbed& tb) { tb.prepare_weights(); }
std::vector<float> initial_params_rng(const NeusTestbed& tb, pcg32 rnd, const float* geo) { return tb.initial_params_rng(rnd, geo); }
uint32_t valid_level_at(const NeusTestbed& tb, int step) { return tb.valid_level_at(step); }
void net_forward(NeusTestbed& tb, const uint32_t* n_ptr, uint32_t n_fixed, uint32_t n_cap, const float* c, uint32_t valid, half_t* out, hipStream_t s) {
	tb.net_forward(n_ptr, n_fixed, n_cap, c, valid, out, s);
}
void net_backward(NeusTestbed& tb, const uint32_t* n_valid_ptr, const uint32_t* n_train_ptr, uint32_t n, const float* c, uint32_t valid,
                  const half_t* dlo, float* g, hipStream_t s) {
	tb.net_backward(n_valid_ptr, n_train_ptr, n, c, valid, dlo, g, s);
}
} // namespace neus

namespace {
hipStream_t as_stream(NeusTestbed* tb, void* s) { return s ? (hipStream_t)s : tb->stream; }
}

extern "C" {

const char* neus_last_error(void) { return g_err.c_str(); }
int neus_abi_version(uint32_t* out) {
	if (!out) return 1;
	*out = NEUS_ABI_VERSION;
	return 0;
}
int neus_device_count(int* count) { return guard([&] { HIP_CHECK(hipGetDeviceCount(count)); }); }
int neus_device_synchronize(void) { return guard([&] { HIP_CHECK(hipDeviceSynchronize()); }); }

int neus_testbed_create(int device, NeusTestbed** out) {
	return guard([&] {
		g_alloc_base = g_alloc_seq.load();
		g_alloc_dbg = alloc_debug_from_env();
		*out = new NeusTestbed(device);
	});
}
int neus_testbed_destroy(NeusTestbed* tb) { return guard([&] { delete tb; }); }
int neus_testbed_set_dataset(NeusTestbed* tb, uint32_t n_images, const NeusImage* images, float aabb_scale) {
	return guard([&] { tb->set_dataset(n_images, images, aabb_scale); });
}
int neus_testbed_reload_network(NeusTestbed* tb, const NeusNetworkConfig* cfg, const float* geo) {
	return guard([&] { tb->reset_network(*cfg, geo); });
}
int neus_testbed_layout(NeusTestbed* tb, NeusNetLayout* o) {
	return guard([&] {
		if (!tb->have_net) throw std::runtime_error("no network");
		const Layout& l = tb->lay;
		o->n_params = l.P; o->n_density = l.n_density; o->n_rgb = l.n_rgb; o->grid_offset = l.grid_off; o->n_grid_params = l.n_grid;
		o->variance_offset = l.var_off; o->n_matrix = l.n_matrix; o->density_input_width = l.din; o->rgb_input_width = 48;
		o->per_level_scale = tb->cfg.per_level_scale; o->n_levels = l.L;
	});
}
int neus_testbed_train(NeusTestbed* tb, uint32_t n_steps) {
	return guard([&] {
		HIP_CHECK(hipSetDevice(tb->device));
		// the LDS-garbage test hook is this thread's while its steps are queued (other testbeds / threads unaffected);
		// the pattern alternates with its complement from step to step
		struct FillScope { ~FillScope() { g_dbg_lds_fill = 0; g_dbg_xcd_shift = 0; } } fill_scope;
		// (a lookahead left pending by a step that threw is dropped: the next step marches again, the same samples)
		struct LaScope { NeusTestbed* t; ~LaScope() { if (t->la_pending) { (void)hipStreamSynchronize(t->la_stream.get()); t->la_pending = false; } t->la_next_in_call = false; if (t->opt.la_stat) t->la_stat_report(); } } la_scope{tb};
		for (uint32_t i = 0; i < n_steps; ++i) {
			g_dbg_lds_fill = tb->dbg_lds_fill_all ? ((tb->training_step & 1) ? ~tb->dbg_lds_fill_all : tb->dbg_lds_fill_all) : 0u;
			g_dbg_xcd_shift = tb->dbg_xcd_shift;
			tb->la_next_in_call = i + 1 < n_steps;
			tb->call_left = n_steps - i - 1;
			tb->train_step();
		}
	});
}
int neus_testbed_get_stats(NeusTestbed* tb, NeusTrainStats* o) {
	return guard([&] {
		tb->consume_loss(false);  // health bits and the abort are reported below, not raised
		HIP_CHECK(hipStreamSynchronize(tb->stream));
		StepState s{};
		HIP_CHECK(hipMemcpy(&s, tb->st.p, sizeof(s), hipMemcpyDeviceToHost));
		float mean = 0.f;
		if (tb->grid_mean.p) HIP_CHECK(hipMemcpy(&mean, tb->grid_mean.p, 4, hipMemcpyDeviceToHost));
		o->training_step = tb->training_step; o->rays_per_batch = s.rays_per_batch; o->measured_batch_size = s.measured_batch_size;
		o->measured_batch_size_before_compaction = s.measured_before; o->n_rays_total = s.n_rays_total;
		o->valid_level = tb->valid_level_at(tb->enc_step); o->zero_records = s.zero_records;
		o->loss = tb->loss_scalar_ema; o->ek_loss = tb->ek_loss; o->mask_loss = tb->mask_loss; o->last_loss = tb->last_loss;
		o->density_grid_mean = mean;
		o->ray_loss = tb->ray_loss; o->n_rays_with_samples = tb->last_rays_with_samples;
		o->trained_samples_total = s.trained_total;
		o->march_first_pass_rays = s.march_est; o->kept_ray_extent = s.kept_extent;
		o->nonfinite_loss = tb->nonfinite ? 1u : 0u;
		o->training_aborted = (tb->aborted || (tb->training_step > 0 && s.zero_records)) ? 1u : 0u;
		o->pre_samples_total = s.pre_total; o->rays_total = s.rays_total;
		o->occ_samples_total = tb->occ_samples; o->occ_updates = tb->occ_updates;
		o->progressive_chunk_end = tb->sched.ends.empty() ? 0u : tb->sched.ends[0];
		o->lookahead_steps = tb->la_steps;
		o->cut_steps = tb->cut_steps;
		o->march_cut_steps = tb->mcut_steps;
		o->march_cut_reruns = tb->mcut_reruns;
		o->adam_split_steps = tb->adam_split_steps;
		o->health_flags = s.fail_flags | tb->fail_seen | (scan_failures(tb->scan_tmp.p) ? STEP_FAIL_SCAN : 0u);
		o->evaluated_samples_total = s.eval_total; o->progressive_steps = s.prog_steps; o->evaluated_samples_last = s.eval_last;
	});
}
static int copy_param_vec(NeusTestbed* tb, const float* dev, float* host, uint64_t n) {
	return guard([&] {
		if (!tb->have_net || n != tb->lay.P) throw std::runtime_error("parameter count mismatch");
		HIP_CHECK(hipStreamSynchronize(tb->stream));
		HIP_CHECK(hipMemcpy(host, dev, n * 4, hipMemcpyDeviceToHost));
	});
}
int neus_testbed_get_params(NeusTestbed* tb, float* o, uint64_t n) { return copy_param_vec(tb, tb->params_fp.p, o, n); }
int neus_testbed_get_gradients(NeusTestbed* tb, float* o, uint64_t n) { return copy_param_vec(tb, tb->grads.p, o, n); }
int neus_testbed_get_ema_params(NeusTestbed* tb, float* o, uint64_t n) { return copy_param_vec(tb, tb->ema_tmp.p, o, n); }
int neus_testbed_get_half_params(NeusTestbed* tb, int which, uint16_t* o, uint64_t n) {
	return guard([&] {
		if (!tb->have_net || n != tb->lay.P) throw std::runtime_error("parameter count mismatch");
		if (which != 0 && which != 1) throw std::runtime_error("get_half_params: which must be 0 (training) or 1 (inference)");
		if (which) tb->sync_ema_h();
		HIP_CHECK(hipStreamSynchronize(tb->stream));
		HIP_CHECK(hipMemcpy(o, which ? tb->ema_h.p : tb->params_h.p, n * 2, hipMemcpyDeviceToHost));
	});
}
int neus_testbed_set_params(NeusTestbed* tb, const float* in, uint64_t n) {
	return guard([&] {
		if (!tb->have_net || n != tb->lay.P) throw std::runtime_error("parameter count mismatch");
		HIP_CHECK(hipStreamSynchronize(tb->stream));
		HIP_CHECK(hipMemcpy(tb->params_fp.p, in, n * 4, hipMemcpyHostToDevice));
		launch_cast_half(tb->stream, (uint32_t)n, tb->params_fp.p, tb->params_h.p);
		tb->prepare_weights();
		HIP_CHECK(hipStreamSynchronize(tb->stream));
	});
}
int neus_testbed_get_density_grid(NeusTestbed* tb, float* g, uint8_t* bf) {
	return guard([&] {
		HIP_CHECK(hipStreamSynchronize(tb->stream));
		if (g) HIP_CHECK(hipMemcpy(g, tb->density_grid.p, (size_t)GRID3 * 4, hipMemcpyDeviceToHost));
		if (bf) HIP_CHECK(hipMemcpy(bf, tb->bitfield.p, GRID3 / 8 * NERF_CASCADES, hipMemcpyDeviceToHost));
	});
}
int neus_testbed_set_density_grid(NeusTestbed* tb, const float* g, const uint8_t* bf) {
	return guard([&] {
		HIP_CHECK(hipStreamSynchronize(tb->stream));
		if (g) HIP_CHECK(hipMemcpy(tb->density_grid.p, g, (size_t)GRID3 * 4, hipMemcpyHostToDevice));
		if (bf) {
			HIP_CHECK(hipMemcpy(tb->bitfield.p, bf, GRID3 / 8 * NERF_CASCADES, hipMemcpyHostToDevice));
			launch_bitfield_linear(tb->stream, tb->bitfield.p, tb->bf_lin.p);
			launch_occ_bbox(tb->stream, tb->bitfield.p, tb->occ_bbox.p);
			HIP_CHECK(hipStreamSynchronize(tb->stream));
		}
	});
}
// Testbed::load_snapshot after reset_network + Trainer::deserialize (testbed.cu:3197-3254, trainer.h:295-304):
// training step, loss scalar, adaptive-batch counters; the inference (EMA) weights start as the loaded ones
// (Trainer::set_params writes m_params_inference too); density grid mean + bitfield rebuilt
// (update_density_grid_mean_and_bitfield, testbed.cu:3240).
int neus_testbed_restore_state(NeusTestbed* tb, const NeusRestoreState* in) {
	return guard([&] {
		if (!in) throw std::runtime_error("restore_state: null argument");
		if (!tb->have_net) throw std::runtime_error("restore_state: no network (reload_network first)");
		if (in->rays_per_batch == 0 || in->rays_per_batch > MAX_RAYS || in->rays_per_batch % 128 != 0)
			throw std::runtime_error("restore_state: rays_per_batch must be a positive multiple of 128 <= 2^18");
		HIP_CHECK(hipSetDevice(tb->device));
		HIP_CHECK(hipStreamSynchronize(tb->stream));
		tb->consume_loss();
		StepState s{};
		HIP_CHECK(hipMemcpy(&s, tb->st.p, sizeof(s), hipMemcpyDeviceToHost));
		s.rays_per_batch = in->rays_per_batch;
		s.measured_batch_size = in->measured_batch_size;
		s.measured_before = in->measured_batch_size_before_compaction;
		HIP_CHECK(hipMemcpy(tb->st.p, &s, sizeof(s), hipMemcpyHostToDevice));
		tb->training_step = in->training_step;
		tb->loss_scalar_ema = tb->last_loss = in->loss;
		tb->loss_ema_init = true;
		HIP_CHECK(hipMemcpy(tb->ema_h.p, tb->params_h.p, (size_t)tb->lay.P * 2, hipMemcpyDeviceToDevice));
		tb->ema_h_stale = false;
		// the fp32 EMA follows the loaded inference weights (the first EMA step after a reload weighs it by 0)
		HIP_CHECK(hipMemcpy(tb->ema_tmp.p, tb->params_fp.p, (size_t)tb->lay.P * 4, hipMemcpyDeviceToDevice));
		if (in->rebuild_bitfield) {
			launch_grid_mean(tb->stream, tb->density_grid.p, tb->grid_partial.p, tb->grid_mean.p);
			launch_bitfield(tb->stream, tb->density_grid.p, tb->bitfield.p, tb->grid_mean.p, tb->max_cascade + 1);
			launch_bitfield_linear(tb->stream, tb->bitfield.p, tb->bf_lin.p);
			launch_occ_bbox(tb->stream, tb->bitfield.p, tb->occ_bbox.p);
		}
		HIP_CHECK(hipStreamSynchronize(tb->stream));
	});
}
int neus_testbed_get_optimizer_state(NeusTestbed* tb, NeusOptimizerState* st, float* m1, float* m2, uint32_t* steps, uint16_t* ema_half) {
	return guard([&] {
		if (!tb->have_net) throw std::runtime_error("optimizer state: no network");
		tb->sync_ema_h();
		HIP_CHECK(hipStreamSynchronize(tb->stream));
		const size_t P = tb->lay.P;
		if (st) {
			st->n_params = (uint32_t)P;
			st->current_step = tb->adam_step;
			st->learning_rate = tb->cur_frame ? tb->cfg.after_learning_rate : tb->cfg.learning_rate;
			st->learning_rate_factor = tb->lr_factor;
		}
		if (m1) HIP_CHECK(hipMemcpy(m1, tb->m1.p, P * 4, hipMemcpyDeviceToHost));
		if (m2) HIP_CHECK(hipMemcpy(m2, tb->m2.p, P * 4, hipMemcpyDeviceToHost));
		if (steps) tb->get_steps(steps);  // (saturated at 65535 while the bias table is converged: optim.hip AdamSteps)
		if (ema_half) HIP_CHECK(hipMemcpy(ema_half, tb->ema_h.p, P * 2, hipMemcpyDeviceToHost));
	});
}
int neus_testbed_set_optimizer_state(NeusTestbed* tb, const NeusOptimizerState* st, const float* m1, const float* m2, const uint32_t* steps,
                                     const uint16_t* ema_half) {
	return guard([&] {
		if (!tb->have_net) throw std::runtime_error("optimizer state: no network");
		if (!st || !m1 || !m2 || !ema_half) throw std::runtime_error("set_optimizer_state: state, moments and EMA weights are required");
		const size_t P = tb->lay.P;
		if (st->n_params != P) throw std::runtime_error("set_optimizer_state: parameter count mismatch");
		HIP_CHECK(hipSetDevice(tb->device));
		HIP_CHECK(hipStreamSynchronize(tb->stream));
		HIP_CHECK(hipMemcpy(tb->m1.p, m1, P * 4, hipMemcpyHostToDevice));
		HIP_CHECK(hipMemcpy(tb->m2.p, m2, P * 4, hipMemcpyHostToDevice));
		// Adam::deserialize: param_steps absent -> zeros (adam.h:437-442)
		tb->ensure_bias_table();  // (the counts' width follows the betas' bias table)
		tb->put_steps(steps);
		// Ema::deserialize (ema.h:189-194): the EMA weights, and the fp32 accumulator cast from them
		HIP_CHECK(hipMemcpy(tb->ema_h.p, ema_half, P * 2, hipMemcpyHostToDevice));
		tb->ema_h_stale = false;
		std::vector<float> f(P);
		for (size_t i = 0; i < P; ++i) { half_t h; std::memcpy(&h, &ema_half[i], 2); f[i] = (float)h; }
		HIP_CHECK(hipMemcpy(tb->ema_tmp.p, f.data(), P * 4, hipMemcpyHostToDevice));
		tb->adam_step = st->current_step;
		tb->lr_factor = st->learning_rate_factor;
		tb->sync_ema_h(); tb->prepare_weights_for(tb->mlp_ema);
		HIP_CHECK(hipStreamSynchronize(tb->stream));
	});
}
int neus_testbed_render(NeusTestbed* tb, const NeusRenderRequest* rq, float* rgba_out, uint32_t* n_iterations) {
	return guard([&] {
		if (!rq || !rgba_out) throw std::runtime_error("render: null argument");
		HIP_CHECK(hipSetDevice(tb->device));
		const uint32_t it = tb->render(*rq, rgba_out);
		if (n_iterations) *n_iterations = it;
	});
}
int neus_testbed_sdf_on_grid(NeusTestbed* tb, const int32_t res[3], const float aabb_min[3], const float aabb_max[3], float* host_out) {
	return guard([&] {
		HIP_CHECK(hipSetDevice(tb->device));
		uint32_t r[3];
		for (int k = 0; k < 3; ++k) { if (res[k] < 1) throw std::runtime_error("sdf_on_grid: empty resolution"); r[k] = (uint32_t)res[k]; }
		const uint64_t n = (uint64_t)r[0] * r[1] * r[2];
		tb->mc_density.alloc(n);
		tb->sdf_on_grid(r, aabb_min, aabb_max, tb->mc_density.p);
		HIP_CHECK(hipMemcpyAsync(host_out, tb->mc_density.p, n * 4, hipMemcpyDeviceToHost, tb->stream));
		HIP_CHECK(hipStreamSynchronize(tb->stream));
	});
}
int neus_testbed_marching_cubes(NeusTestbed* tb, const int32_t res[3], const float aabb_min[3], const float aabb_max[3], float thresh,
                                const float* density_dev, uint32_t* n_verts, uint32_t* n_tris) {
	return guard([&] {
		HIP_CHECK(hipSetDevice(tb->device));
		tb->marching_cubes(res, aabb_min, aabb_max, thresh, density_dev);
		if (n_verts) *n_verts = tb->mesh_nv;
		if (n_tris) *n_tris = tb->mesh_nt;
	});
}
int neus_testbed_mc_density(NeusTestbed* tb, uint64_t offset, uint64_t count, float* host_out) {
	return guard([&] {
		if (!host_out || offset + count > tb->mc_density.n) throw std::runtime_error("mc_density: range outside the last SDF grid");
		HIP_CHECK(hipStreamSynchronize(tb->stream));
		HIP_CHECK(hipMemcpy(host_out, tb->mc_density.p + offset, count * 4, hipMemcpyDeviceToHost));
	});
}
int neus_testbed_get_mesh(NeusTestbed* tb, float* verts, uint32_t* tris) {
	return guard([&] {
		HIP_CHECK(hipStreamSynchronize(tb->stream));
		if (verts && tb->mesh_nv) HIP_CHECK(hipMemcpy(verts, tb->mesh_v.p, (size_t)tb->mesh_nv * 12, hipMemcpyDeviceToHost));
		if (tris && tb->mesh_nt) HIP_CHECK(hipMemcpy(tris, tb->mesh_f.p, (size_t)tb->mesh_nt * 12, hipMemcpyDeviceToHost));
	});
}
int neus_testbed_mesh_vertex_colors(NeusTestbed* tb, float* rgb) {
	return guard([&] {
		if (!rgb) throw std::runtime_error("mesh_vertex_colors: null output");
		HIP_CHECK(hipSetDevice(tb->device));
		tb->mesh_colors(rgb);
	});
}
int neus_mc_table(int8_t* out) { return guard([&] { mc_table_host(out); }); }
int neus_prepare_image_rgba8(uint8_t* rgba, uint32_t w, uint32_t h, const uint8_t* alpha_rgba, const uint8_t* mask_rgba, uint32_t flags,
                             uint32_t* mask_color_out) {
	return guard([&] {
		if (!rgba) throw std::runtime_error("prepare_image: null image");
		const uint64_t n = (uint64_t)w * h;
		if (alpha_rgba) {
			// srgb_to_linear (common_device.cuh:31-37) of the alpha image's red channel, as a 256-entry table
			uint8_t lut[256];
			for (int v = 0; v < 256; ++v) {
				const float srgb = (float)v * (1.f / 255.f);
				const float lin = srgb <= 0.04045f ? srgb / 12.92f : std::pow((srgb + 0.055f) / 1.055f, 2.4f);
				lut[v] = (uint8_t)(255.0f * lin);
			}
			for (uint64_t i = 0; i < n; ++i) rgba[4 * i + 3] = lut[alpha_rgba[4 * i]];
		}
		const uint32_t key = mask_rgba ? 0x00FF00FFu : 0u;  // hot pink
		if (mask_rgba)
			for (uint64_t i = 0; i < n; ++i)
				if (mask_rgba[4 * i] != 0) std::memcpy(rgba + 4 * i, &key, 4);
		const bool wt = flags & NEUS_IMAGE_WHITE_TRANSPARENT, bt = flags & NEUS_IMAGE_BLACK_TRANSPARENT;
		if (wt || bt || key)
			for (uint64_t i = 0; i < n; ++i) {
				uint8_t* p = rgba + 4 * i;
				if (wt && p[0] == 255 && p[1] == 255 && p[2] == 255) p[3] = 0;
				if (bt && p[0] == 0 && p[1] == 0 && p[2] == 0) p[3] = 0;
				uint32_t v;
				std::memcpy(&v, p, 4);
				if (key != 0 && v == key) { p[0] = 0xFF; p[1] = 0x00; p[2] = 0xFF; p[3] = 0x00; }
			}
		if (mask_color_out) *mask_color_out = key;
	});
}
int neus_testbed_next_frame(NeusTestbed* tb, uint32_t n_images, const NeusImage* images) {
	return guard([&] {
		HIP_CHECK(hipSetDevice(tb->device));
		tb->next_frame(n_images, images);
	});
}
int neus_testbed_change_frame(NeusTestbed* tb, uint32_t frame, uint32_t n_images, const NeusImage* images) {
	return guard([&] {
		HIP_CHECK(hipSetDevice(tb->device));
		tb->change_frame(frame, n_images, images);
	});
}
int neus_testbed_prepare_for_test(NeusTestbed* tb, int* out_use_delta) {
	return guard([&] {
		tb->render_delta = tb->cur_frame != 0 && tb->train_delta;
		if (out_use_delta) *out_use_delta = tb->render_delta ? 1 : 0;
	});
}
int neus_testbed_saved_transform(NeusTestbed* tb, float* out12) {
	return guard([&] {
		if (!out12) throw std::runtime_error("saved_transform: null output");
		if (!tb->have_net) throw std::runtime_error("save_transform: no network");
		HIP_CHECK(hipStreamSynchronize(tb->stream));
		DeltaState h{};
		HIP_CHECK(hipMemcpy(&h, tb->delta.p, sizeof(h), hipMemcpyDeviceToHost));
		float R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3] = {0, 0, 0};
		if (tb->ds.motion.on) { std::memcpy(R, tb->ds.motion.R, sizeof(R)); std::memcpy(t, tb->ds.motion.t, sizeof(t)); }
		host_accumulate_movement(h.p, R, t);
		std::memcpy(out12, R, sizeof(R)); std::memcpy(out12 + 9, t, sizeof(t));
	});
}
int neus_testbed_get_training_options(NeusTestbed* tb, NeusTrainingOptions* o) {
	return guard([&] {
		if (!o) throw std::runtime_error("get_training_options: null output");
		const TrainTarget& t = tb->ds.target;
		o->random_bg_color = t.fixed_bg ? 0 : 1;
		for (int k = 0; k < 3; ++k) o->background_color[k] = t.bg[k];
		o->color_space = t.mode == 1 ? 1 : 0;
		o->linear_colors = t.mode == 2 ? 1 : 0;
		if (t.mode == 2) o->color_space = tb->color_space_when_linear;
		o->cone_angle_constant = tb->ds.cone_angle;
		o->near_distance = tb->near_distance;
		o->depth_supervision_lambda = tb->depth_lambda;
	});
}
int neus_testbed_set_progressive_inference(NeusTestbed* tb, int mode, const uint32_t* chunk_ends, uint32_t n_ends) {
	return guard([&] {
		tb->sched.set(mode, chunk_ends, n_ends);
	});
}

int neus_testbed_set_training_options(NeusTestbed* tb, const NeusTrainingOptions* o) {
	return guard([&] {
		if (!o) throw std::runtime_error("set_training_options: null options");
		if (o->color_space != 0 && o->color_space != 1) throw std::runtime_error("color_space must be 0 (Linear) or 1 (SRGB)");
		if (!(o->cone_angle_constant >= 0.0f)) throw std::runtime_error("cone_angle_constant must be >= 0");
		HIP_CHECK(hipStreamSynchronize(tb->stream));  // kernels in flight read ds by value; later steps see the new targets
		TrainTarget t{};
		t.fixed_bg = o->random_bg_color ? 0u : 1u;
		for (int k = 0; k < 3; ++k) t.bg[k] = o->background_color[k];
		// train_in_linear_colors wins over the colour space (testbed_nerf.cu:1658)
		t.mode = o->linear_colors ? 2u : (o->color_space == 1 ? 1u : 0u);
		tb->color_space_when_linear = o->color_space;
		tb->ds.target = t;
		tb->ds.cone_angle = o->cone_angle_constant;
		tb->near_distance = o->near_distance;
		if (!(o->depth_supervision_lambda >= 0.f)) throw std::runtime_error("depth_supervision_lambda must be >= 0");
		tb->depth_lambda = o->depth_supervision_lambda;
	});
}
int neus_testbed_get_movement(NeusTestbed* tb, float* global12, float* local12) {
	return guard([&] {
		if (global12) { std::memcpy(global12, tb->ds.motion.R, 9 * 4); std::memcpy(global12 + 9, tb->ds.motion.t, 3 * 4); }
		if (local12) {
			if (!tb->have_net) throw std::runtime_error("get_movement: no network");
			DeltaState h{};
			HIP_CHECK(hipStreamSynchronize(tb->stream));
			HIP_CHECK(hipMemcpy(&h, tb->delta.p, sizeof(h), hipMemcpyDeviceToHost));
			std::memcpy(local12, h.p, DELTA_PARAMS * 4);
		}
	});
}
int neus_testbed_set_movement(NeusTestbed* tb, const float* global12, const float* local12) {
	return guard([&] {
		if (global12) {
			std::memcpy(tb->ds.motion.R, global12, 9 * 4); std::memcpy(tb->ds.motion.t, global12 + 9, 3 * 4);
			const float I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
			bool ident = global12[9] == 0.f && global12[10] == 0.f && global12[11] == 0.f;
			for (int k = 0; k < 9; ++k) ident = ident && global12[k] == I[k];
			tb->ds.motion.on = ident ? 0u : 1u;
		}
		if (local12) {
			if (!tb->have_net) throw std::runtime_error("set_movement: no network");
			DeltaState h{};
			HIP_CHECK(hipStreamSynchronize(tb->stream));
			HIP_CHECK(hipMemcpy(&h, tb->delta.p, sizeof(h), hipMemcpyDeviceToHost));
			std::memcpy(h.p, local12, DELTA_PARAMS * 4);
			HIP_CHECK(hipMemcpy(tb->delta.p, &h, sizeof(h), hipMemcpyHostToDevice));
			launch_delta_prepare(tb->stream, tb->delta.p);
			HIP_CHECK(hipStreamSynchronize(tb->stream));
		}
	});
}
int neus_testbed_frame_state(NeusTestbed* tb, uint32_t* o) {
	return guard([&] { o[0] = tb->cur_frame; o[1] = tb->canonical_step; o[2] = tb->train_canonical; o[3] = tb->train_delta; });
}
int neus_testbed_get_rng(NeusTestbed* tb, uint64_t* o) {
	return guard([&] { o[0] = tb->rng.state; o[1] = tb->rng.inc; o[2] = tb->density_grid_rng.state; o[3] = tb->density_grid_rng.inc; });
}
int neus_testbed_ray_counts(NeusTestbed* tb, uint32_t n, uint32_t* nreq, uint32_t* ccount, uint32_t* numsteps) {
	return guard([&] {
		if (!tb->have_net) throw std::runtime_error("no network");
		n = std::min(n, MAX_RAYS);
		HIP_CHECK(hipStreamSynchronize(tb->stream));
		if (nreq) HIP_CHECK(hipMemcpy(nreq, tb->nreq.p, (size_t)n * 4, hipMemcpyDeviceToHost));
		if (ccount) HIP_CHECK(hipMemcpy(ccount, tb->ccount.p, (size_t)n * 4, hipMemcpyDeviceToHost));
		if (numsteps) HIP_CHECK(hipMemcpy(numsteps, tb->numsteps.p, (size_t)n * 8, hipMemcpyDeviceToHost));
	});
}
static void time_kernel_impl(NeusTestbed* tb, int kernel, int variant, int iters, float* ms_out);
int neus_debug_time_kernel(NeusTestbed* tb, int kernel, int variant, int iters, float* ms_out) {
	return guard([&] { time_kernel_impl(tb, kernel, variant, iters, ms_out); });
}
int neus_testbed_time_kernel(NeusTestbed* tb, int kernel, int iters, float* ms_out, uint32_t* units_out) {
	return guard([&] {
		time_kernel_impl(tb, kernel, 0, iters, ms_out);
		StepState h{};
		HIP_CHECK(hipMemcpy(&h, tb->st.p, sizeof(StepState), hipMemcpyDeviceToHost));
		// work units of one launch: ray slots (march), pre-compaction samples (write, inference, loss),
		// compacted training samples (encode, MLP, weight gradients, grid scatter), parameters (Adam / EMA)
		*units_out = kernel == 0 ? MAX_RAYS : kernel <= 4 ? h.n_kept : kernel == 12 ? tb->lay.P : tb->batch;
		if (kernel == 13) {  // the slots a cut march generates and marches
			uint32_t est = MAX_RAYS;
			HIP_CHECK(hipMemcpy(&est, tb->cutw.p + CW_EST, 4, hipMemcpyDeviceToHost));
			const uint32_t e0 = h.march_est ? std::min(h.march_est, MAX_RAYS) : MAX_RAYS;
			*units_out = std::min(est, e0);
		}
	});
}
static void time_kernel_impl(NeusTestbed* tb, int kernel, int variant, int iters, float* ms_out) {
	{
		if (!tb->have_net) throw std::runtime_error("no network");
		NeusTestbed& t = *tb;
		hipStream_t s = t.stream;
		const DPInfo dp = t.dp_info();
		const uint32_t valid = t.valid_level_at((int)t.training_step);
		const uint32_t* lin = t.bf_lin.p;
		auto march = [&]() {
			launch_march_count(s, MAX_RAYS, t.max_samples, t.st.p, dp, t.ds, t.bitfield.p, lin, t.rng.state, t.rng.inc, t.rays.p, t.startt.p, t.nreq.p, t.mwork,
			                   nullptr, 0, t.opt.ray_cull ? t.occ_bbox.p : nullptr);
			launch_march_write(s, MAX_RAYS, t.st.p, t.ds, t.rays.p, t.mwork, t.nreq.p, t.base.p, t.numsteps.p, t.coords.p,
			                   t.sample_ray.p, t.max_samples, t.scan_tmp.p);
		};
		const LossWork w = t.loss_work(t.base.p);
		if (variant != 99) {  // 99: no re-preparation (counter runs: only the timed kernel is launched)
			march();
			launch_nerf_infer(s, t.lay.L, t.lay.W, &t.st.p->n_kept, 0, t.coords.p, t.gl, valid, t.params_h.p + t.lay.grid_off, t.mlp, t.net_out.p, 8192);
			launch_loss_alpha(s, t.max_samples, t.st.p, t.coords.p, t.net_out.p, t.cos_anneal(), w);
		}
		// one event between consecutive launches (fence-free: timing only); the median launch is reported
		iters = std::max(1, iters);
		std::vector<Event> evs((size_t)iters + 1);
		for (auto& e : evs) e = make_event(hipEventDisableSystemFence);
		for (int k = 0; k < iters; ++k) {
			// (variant 98: no event between the launches - back to back, for the queue gaps of a kernel trace)
			if (variant != 98 || k == 0) HIP_CHECK(hipEventRecord(evs[k].get(), s));
			switch (kernel) {
			case 0: launch_march_count(s, MAX_RAYS, t.max_samples, t.st.p, dp, t.ds, t.bitfield.p, lin, t.rng.state, t.rng.inc, t.rays.p, t.startt.p, t.nreq.p, t.mwork,
			                   nullptr, 0, t.opt.ray_cull ? t.occ_bbox.p : nullptr); break;
			case 1: launch_march_write(s, MAX_RAYS, t.st.p, t.ds, t.rays.p, t.mwork, t.nreq.p, t.base.p, t.numsteps.p,
			                           t.coords.p, t.sample_ray.p, t.max_samples, t.scan_tmp.p); break;
			case 2: debug_launch_loss_scan(s, variant, MAX_RAYS, t.numsteps.p, w, t.ccount.p); break;
			case 3: launch_nerf_infer(s, t.lay.L, t.lay.W, &t.st.p->n_kept, 0, t.coords.p, t.gl, valid, t.params_h.p + t.lay.grid_off, t.mlp,
			                          t.net_out.p, 8192); break;
			case 4: launch_loss_alpha(s, t.max_samples, t.st.p, t.coords.p, t.net_out.p, t.cos_anneal(), w); break;
			case 5: case 9: case 10: {  // the training-MLP kernels (5 both, 9 colour, 10 density) on the last compacted batch
				TrainBufs tbuf = t.tbuf;
				tbuf.var_grad = t.grads.p + t.lay.var_off;
				launch_mlp_train(s, t.lay.L, t.lay.W, nullptr, t.batch, t.batch, t.coords_c.p, (const half_t*)t.enc.p, t.dydx.p, t.dL_dout.p, t.mlp, tbuf,
				                 kernel == 5 ? 0 : kernel - 8);
				break;
			}
			case 6: launch_mlp_grad_reduce(s, t.grad_reduce(t.batch, t.grads.p, nullptr)); break;
			case 7:
				launch_grid_scatter(s, nullptr, t.batch, t.batch, t.coords_c.p, COORD_W, t.gl, valid, t.tbuf.dLdenc, t.tbuf.genc, t.tbuf.v,
				                    t.grads.p + t.lay.grid_off, t.swork, t.scan_tmp.p, t.scan_tmp_bytes);
				t.sc_zero_from = t.swork.n_buckets;  // the replay wrote every bucket: nothing is known zero for the next step
				t.sc_zero_from_e = t.gl.offset[t.gl.n_levels];
				break;
			case 8: t.encode(nullptr, t.batch, t.batch, t.batch, t.coords_c.p, COORD_W, valid, true, s); break;
			case 11: {
				// level-partitioned gather experiment: the level-major encode (enc only, no dy/dx) over the
				// inference's pre-compaction samples; variant = workgroups per level (0: 2048)
				if (!t.dbg_enc.p) t.dbg_enc.alloc((size_t)t.lay.L * t.max_samples);
				launch_grid_encode(s, &t.st.p->n_kept, 0, t.max_samples, t.coords.p, COORD_W, t.gl, valid, t.params_h.p + t.lay.grid_off,
				                   t.dbg_enc.p, nullptr, variant > 0 && variant != 99 ? (uint32_t)variant : 2048u, nullptr);
				break;
			}
			case 12: t.optimizer_step(t.grads.p); break;  // the Adam / EMA pass on the last gradient (advances the optimizer)
			case 14: {  // development: the occupancy update's density pass (k_nerf_density MODE 2 into the scratch grid) on the
				        // current state: variant 0 both halves (after step 256), 1 the uniform half, 2 the occupancy-biased half
				const uint32_t nc = GRID3 * (t.max_cascade + 1);
				const uint32_t n_u = variant == 2 ? 0u : nc / 4, n_nu = variant == 1 ? 0u : nc / 4;
				pcg32 r = t.density_grid_rng;
				const pcg32 rng_u = r;
				r.advance();
				const pcg32 rng_nu = r;
				OccSampling os{};
				os.n_u = n_u; os.n_nu = n_nu; os.lo = 0;
				os.rng_u_state = rng_u.state; os.rng_u_inc = rng_u.inc; os.rng_nu_state = rng_nu.state; os.rng_nu_inc = rng_nu.inc;
				os.step = t.density_grid_ema_step; os.n_cascades = t.max_cascade + 1; os.thresh_nu = NERF_MIN_OPTICAL_THICKNESS;
				for (int d = 0; d < 3; ++d) { os.amin[d] = t.ds.aabb_min[d]; os.diag[d] = t.ds.aabb_max[d] - t.ds.aabb_min[d]; }
				os.grid_in = t.density_grid.p; os.grid_tmp = t.density_tmp.p;
				os.jt = t.jump_table();
				if (n_u) {
					if (!t.occ_ulist.p) t.occ_ulist.alloc(GRID3);
					launch_occ_uniform_list(s, n_u, t.density_grid_ema_step, 0, n_u, t.occ_ulist.p, t.scan_tmp.p);
					os.ulist = t.occ_ulist.p; os.n_ulist = n_u;
				}
				launch_occ_density(s, t.lay.L, t.lay.W, n_u + n_nu, os, t.gl, valid, t.params_h.p + t.lay.grid_off, t.mlp);
				break;
			}
			case 13: {  // the march of a cut step: ray generation + the march over the slots below the cut's estimate
				MarchWork mw = t.mwork;
				mw.est_cut = t.cutw.p + CW_EST;
				launch_march_count(s, MAX_RAYS, t.max_samples, t.st.p, dp, t.ds, t.bitfield.p, lin, t.rng.state, t.rng.inc, t.rays.p, t.startt.p, t.nreq.p,
				                   mw, nullptr, 0, t.opt.ray_cull ? t.occ_bbox.p : nullptr);
				break;
			}
			default: throw std::runtime_error("unknown kernel id");
			}
		}
		HIP_CHECK(hipEventRecord(evs[iters].get(), s));
		HIP_CHECK(hipStreamSynchronize(s));
		std::vector<float> d((size_t)iters);
		if (variant == 98) {
			float all = 0.f;
			HIP_CHECK(hipEventElapsedTime(&all, evs[0].get(), evs[iters].get()));
			for (auto& x : d) x = all / (float)iters;
		} else
			for (int k = 0; k < iters; ++k) HIP_CHECK(hipEventElapsedTime(&d[k], evs[k].get(), evs[k + 1].get()));
		std::sort(d.begin(), d.end());
		*ms_out = d[(size_t)iters / 2];
	}
}
int neus_debug_march_stats(NeusTestbed* tb, uint32_t n, uint32_t* out) {
	return guard([&] {
		if (!tb->have_net) throw std::runtime_error("no network");
		if (tb->ds.cone_angle != 0.0f) throw std::runtime_error("march stats: cone_angle 0 only");
		n = std::min(n, MAX_RAYS);
		Dev<uint32_t> o; o.alloc(3 * (size_t)n);
		debug_launch_march_stats(tb->stream, n, tb->rays.p, tb->startt.p, tb->bf_lin.p, tb->ds, tb->bitfield.p, o.p);
		HIP_CHECK(hipStreamSynchronize(tb->stream));
		HIP_CHECK(hipMemcpy(out, o.p, 12 * (size_t)n, hipMemcpyDeviceToHost));
	});
}
int neus_debug_scatter_stats(NeusTestbed* tb, uint64_t* records_per_level, uint32_t* max_region) {
	return guard([&] {
		if (!tb->have_net || tb->swork.mode != 2) throw std::runtime_error("scatter stats: region mode only");
		HIP_CHECK(hipStreamSynchronize(tb->stream));
		const uint32_t L = tb->lay.L, nb = tb->swork.n_chunks;
		std::vector<uint16_t> h((size_t)L * nb * (SB_LEVEL_BUCKETS + 1));
		HIP_CHECK(hipMemcpy(h.data(), tb->sc_rtab.p, h.size() * 2, hipMemcpyDeviceToHost));
		uint32_t mx = 0;
		for (uint32_t l = 0; l < L; ++l) {
			const uint32_t size = tb->gl.offset[l + 1] - tb->gl.offset[l], nlb = (size + SB_SIZE - 1) / SB_SIZE;
			uint64_t t = 0;
			for (uint32_t b = 0; b < nb; ++b) {
				const uint32_t r = h[((size_t)l * nb + b) * (SB_LEVEL_BUCKETS + 1) + nlb];
				t += r; mx = std::max(mx, r);
			}
			if (records_per_level) records_per_level[l] = t;
		}
		if (max_region) *max_region = mx;
	});
}
int neus_debug_scatter_parts(NeusTestbed* tb, uint32_t* parts_per_level) {
	return guard([&] {
		if (!tb->have_net || tb->swork.mode != 2) throw std::runtime_error("scatter parts: region mode only");
		std::vector<uint32_t> jobs(4 * (size_t)tb->swork.n_jobs2);
		HIP_CHECK(hipMemcpy(jobs.data(), tb->sc_jobs2.p, jobs.size() * 4, hipMemcpyDeviceToHost));
		for (uint32_t l = 0; l < tb->lay.L; ++l) parts_per_level[l] = 0;
		for (size_t j = 0; j < jobs.size() / 4; ++j) parts_per_level[jobs[4 * j]] = std::max(parts_per_level[jobs[4 * j]], jobs[4 * j + 2] >> 16);
	});
}
int neus_debug_grid_scatter(NeusTestbed* tb, void* stream, uint32_t n_cap, const uint32_t* n_valid, const float* coords,
                            uint32_t coord_stride, uint32_t valid_level, const void* dLdenc, const void* genc, const float* v,
                            float* grid_grad_out) {
	return guard([&] {
		if (!tb->have_net) throw std::runtime_error("no network");
		if (n_cap == 0 || n_cap > tb->batch) throw std::runtime_error("neus_debug_grid_scatter: n_cap must be in [1, batch_size]");
		if (n_valid && *n_valid > n_cap) throw std::runtime_error("neus_debug_grid_scatter: n_valid exceeds n_cap");
		if (coord_stride < 3) throw std::runtime_error("neus_debug_grid_scatter: coord_stride must be at least 3");
		if (!coords || !dLdenc || !genc || !v || !grid_grad_out) throw std::runtime_error("neus_debug_grid_scatter: null buffer");
		hipStream_t s = as_stream(tb, stream);
		Dev<uint32_t> n_dev;
		if (n_valid) {
			n_dev.alloc(1);
			HIP_CHECK(hipMemcpyAsync(n_dev.p, n_valid, 4, hipMemcpyHostToDevice, s));
		}
		// the caller's buffer: the plain workspace, as the HashGrid module's backward (no scatter_work_for)
		launch_grid_scatter(s, n_dev.p, n_cap, n_cap, coords, coord_stride, tb->gl, valid_level, (const half_t*)dLdenc, (const half_t*)genc,
		                    (const float4*)v, grid_grad_out, tb->swork, tb->scan_tmp.p, tb->scan_tmp_bytes);
		HIP_CHECK(hipGetLastError());
		HIP_CHECK(hipStreamSynchronize(s));
	});
}
int neus_debug_mlp_train(NeusTestbed* tb, void* stream, uint32_t n, const float* coords, const uint16_t* enc, const float* dydx,
                         const uint16_t* dL_dout, uint32_t indeed_batch_size, float* grads_out, float* dpos, uint16_t* genc_out,
                         uint16_t* dLdenc_out, uint16_t* d1_delta_out, float* v_out) {
	return guard([&] {
		if (!tb->have_net) throw std::runtime_error("no network");
		if (n == 0 || n % 128 != 0) throw std::runtime_error("neus_debug_mlp_train: n must be a positive multiple of 128");
		if (n > tb->batch) throw std::runtime_error("neus_debug_mlp_train: n exceeds batch_size");
		if (indeed_batch_size == 0) throw std::runtime_error("neus_debug_mlp_train: indeed_batch_size must be positive");
		if (!coords || !enc || !dydx || !dL_dout || !grads_out) throw std::runtime_error("neus_debug_mlp_train: null buffer");
		hipStream_t s = as_stream(tb, stream);
		const Layout& l = tb->lay;
		HIP_CHECK(hipMemsetAsync(grads_out, 0, (size_t)l.P * 4, s));
		// the testbed's hand-off buffers with ld = n: rows [.][n] are contiguous, as the caller's
		TrainBufs t = tb->tbuf;
		t.indeed_batch = (float)indeed_batch_size;
		t.dpos = (float4*)dpos;
		t.var_grad = grads_out + l.var_off;
		launch_mlp_train(s, l.L, l.W, nullptr, n, n, coords, (const half_t*)enc, dydx, (const half_t*)dL_dout, tb->mlp, t);
		launch_mlp_grad_reduce(s, tb->grad_reduce(n, grads_out, nullptr));
		HIP_CHECK(hipGetLastError());
		const size_t pair = (size_t)l.L * n * 2 * sizeof(half_t);
		if (genc_out) HIP_CHECK(hipMemcpyAsync(genc_out, t.genc, pair, hipMemcpyDeviceToDevice, s));
		if (dLdenc_out) HIP_CHECK(hipMemcpyAsync(dLdenc_out, t.dLdenc, pair, hipMemcpyDeviceToDevice, s));
		if (d1_delta_out) HIP_CHECK(hipMemcpyAsync(d1_delta_out, t.d1_delta, (size_t)16 * n * sizeof(half_t), hipMemcpyDeviceToDevice, s));
		if (v_out) HIP_CHECK(hipMemcpyAsync(v_out, t.v, (size_t)n * sizeof(float4), hipMemcpyDeviceToDevice, s));
		HIP_CHECK(hipStreamSynchronize(s));
	});
}
int neus_debug_march_profile(NeusTestbed* tb, unsigned long long* out, uint32_t max_waves, uint32_t* n_waves) {
	return guard([&] {
		if (!tb->have_net) throw std::runtime_error("no network");
		NeusTestbed& t = *tb;
		hipStream_t s = t.stream;
		const uint32_t waves = MAX_RAYS * t.mwork.lanes_per_ray / 64;
		Dev<unsigned long long> buf; buf.alloc((size_t)waves * 8);
		HIP_CHECK(hipMemsetAsync(buf.p, 0, (size_t)waves * 64, s));
		MarchWork mw = t.mwork;
		mw.prof = buf.p;
		mw.dbg = t.opt.march_dbg;
		launch_march_count(s, MAX_RAYS, t.max_samples, t.st.p, t.dp_info(), t.ds, t.bitfield.p, t.bf_lin.p, t.rng.state, t.rng.inc,
		                   t.rays.p, t.startt.p, t.nreq.p, mw, nullptr, 0, t.opt.ray_cull ? t.occ_bbox.p : nullptr);
		HIP_CHECK(hipStreamSynchronize(s));
		const uint32_t n = std::min(waves, max_waves);
		HIP_CHECK(hipMemcpy(out, buf.p, (size_t)n * 64, hipMemcpyDeviceToHost));
		if (n_waves) *n_waves = n;
	});
}
int neus_debug_exclusive_scan(void* stream, const uint32_t* in, uint32_t* out, uint32_t n, int reps, uint32_t* failures) {
	return guard([&] {
		hipStream_t s = (hipStream_t)stream;
		const size_t tb_ = scan_temp_bytes(std::max(1u, n));
		ScanTemp tmp; tmp.alloc(tb_ + 256); scan_temp_reset(s, tmp.p);
		for (int r = 0; r < std::max(1, reps); ++r) launch_exclusive_scan(s, tmp.p, tb_, in, out, n);
		HIP_CHECK(hipStreamSynchronize(s));
		if (failures) *failures = scan_failures(tmp.p);
	});
}
int neus_debug_loss_scan_chunk(void* stream, int form, uint32_t n_rays, const uint32_t* numsteps, const float* sa, const float* ekt, uint32_t e0,
                               uint32_t e1, uint32_t e2, const uint32_t* rays_in, const uint32_t* n_rays_in, uint32_t* ccount, float* racc, float* rT,
                               float* rek, float* ck4, float* cke, uint32_t* list, uint32_t* list_counter, uint32_t* rays_out,
                               uint32_t* rays_out_counter) {
	return guard([&] {
		if (form != 0 && form != 1) throw std::runtime_error("neus_debug_loss_scan_chunk: form is 0 (lane) or 1 (group)");
		if ((rays_in != nullptr) != (n_rays_in != nullptr) || (list && !list_counter) || (rays_out && !rays_out_counter))
			throw std::runtime_error("neus_debug_loss_scan_chunk: a list without its counter");
		hipStream_t s = (hipStream_t)stream;
		LossWork w{};
		w.sa = (float4*)sa; w.ekt = (float*)ekt; w.ck4 = (float4*)ck4; w.cke = cke; w.racc = (float4*)racc; w.rT = rT; w.rek = rek;
		launch_loss_scan_chunk(s, n_rays, numsteps, w, ccount, e0, e1, e2, list, list_counter, rays_in, n_rays_in, rays_out, rays_out_counter,
		                       form == 1);
		HIP_CHECK(hipGetLastError());
		HIP_CHECK(hipStreamSynchronize(s));
	});
}
int neus_testbed_stream(NeusTestbed* tb, void** s) { return guard([&] { *s = (void*)tb->stream; }); }
int neus_testbed_synchronize(NeusTestbed* tb) { return guard([&] { HIP_CHECK(hipStreamSynchronize(tb->stream)); }); }
int neus_testbed_set_profiling(NeusTestbed* tb, int on) {
	return guard([&] {
		tb->flush_phases();
		tb->profiling = on != 0;
		for (auto& m : tb->phase_ms) m = 0;
		tb->phase_steps = 0; tb->phase_npre = tb->phase_ntrain = 0;
	});
}
int neus_testbed_set_infer_timing(NeusTestbed* tb, int on) {
	return guard([&] {
		tb->infer_timing = on != 0;
		tb->it_n = 0; tb->it_ms = 0.0; tb->it_launches = 0; tb->it_steps = 0;
	});
}
int neus_testbed_infer_timing(NeusTestbed* tb, double* ms_total, uint64_t* launches, uint64_t* steps) {
	return guard([&] {
		if (ms_total) *ms_total = tb->it_ms;
		if (launches) *launches = tb->it_launches;
		if (steps) *steps = tb->it_steps;
	});
}
int neus_testbed_set_exchange_timing(NeusTestbed* tb, int on) { return guard([&] { tb->x.set_timing(on != 0); }); }
int neus_testbed_exchange_timing(NeusTestbed* tb, double* exposed_ms_total, double* span_ms_total, uint64_t* steps) {
	return guard([&] {
		HIP_CHECK(hipSetDevice(tb->device));
		tb->x.timing(exposed_ms_total, span_ms_total, steps);
	});
}
int neus_testbed_kernel_times(NeusTestbed* tb, float* ms) {
	return guard([&] {
		tb->flush_phases();
		for (int i = 0; i < NeusTestbed::N_PHASES; ++i) ms[i] = tb->phase_steps ? (float)(tb->phase_ms[i] / tb->phase_steps) : 0.f;
		ms[NeusTestbed::N_PHASES] = (float)tb->phase_steps;
		ms[NeusTestbed::N_PHASES + 1] = tb->phase_steps ? (float)(tb->phase_npre / tb->phase_steps) : 0.f;
		ms[NeusTestbed::N_PHASES + 2] = tb->phase_steps ? (float)(tb->phase_ntrain / tb->phase_steps) : 0.f;
	});
}

// ------------------------------------------------------------ data parallel (exchange.h; the groups' own entry points: exchange.cpp)
int neus_testbed_init_data_parallel_ex(NeusTestbed* tb, int rank, int world, const uint8_t* uid, uint32_t flags) {
	return guard([&] { tb->attach([&] { tb->x.attach_rccl(tb->device, rank, world, uid, flags); }); });
}
int neus_testbed_init_data_parallel(NeusTestbed* tb, int rank, int world, const uint8_t* uid) {
	return neus_testbed_init_data_parallel_ex(tb, rank, world, uid, 0u);
}
int neus_testbed_init_local_group(NeusTestbed* tb, NeusLocalGroup* g, int rank) {
	return guard([&] { tb->attach([&] { tb->x.attach_local(g, rank); }); });
}
int neus_testbed_init_host_group(NeusTestbed* tb, NeusHostGroup* g) {
	return guard([&] { tb->attach([&] { tb->x.attach_host(tb->device, g); }); });
}
int neus_testbed_set_exchange_overlap(NeusTestbed* tb, int on) { return guard([&] { tb->x.set_overlap(on != 0); }); }
int neus_testbed_data_parallel_info(NeusTestbed* tb, NeusDataParallelInfo* o) { return guard([&] { tb->x.info(o); }); }

// ------------------------------------------------------------ operator surface
int neus_grid_encode(NeusTestbed* tb, void* stream, uint32_t n, uint32_t ld, const float* coords, uint32_t stride, uint32_t valid,
                     uint16_t* enc, float* dydx) {
	return guard([&] {
		if (!tb->have_net) throw std::runtime_error("no network");
		const uint32_t gx = std::max<uint32_t>(1, std::min<uint32_t>((n + 255) / 256, 4096));
		launch_grid_encode(as_stream(tb, stream), nullptr, n, ld, coords, stride, tb->gl, valid, tb->params_h.p + tb->lay.grid_off,
		                   (uint32_t*)enc, dydx, gx);
		HIP_CHECK(hipGetLastError());
	});
}
int neus_net_forward(NeusTestbed* tb, void* stream, uint32_t n, const float* coords, uint32_t valid, uint16_t* out) {
	return guard([&] {
		if (!tb->have_net) throw std::runtime_error("no network");
		tb->net_forward(nullptr, n, n, coords, valid, (half_t*)out, as_stream(tb, stream));
		HIP_CHECK(hipGetLastError());
	});
}
int neus_net_backward(NeusTestbed* tb, void* stream, uint32_t n, const float* coords, uint32_t valid, const uint16_t* dlo,
                      uint32_t indeed, float* grads_out) {
	return guard([&] {
		if (!tb->have_net) throw std::runtime_error("no network");
		if (n == 0 || n % 128 != 0) throw std::runtime_error("neus_net_backward: batch must be a positive multiple of 128 (fully_fused_mlp.cu:779-781)");
		if (n > tb->batch) throw std::runtime_error("neus_net_backward: n exceeds batch_size");
		hipStream_t s = as_stream(tb, stream);
		HIP_CHECK(hipMemsetAsync(grads_out, 0, (size_t)tb->lay.P * 4, s));
		const float saved = tb->tbuf.indeed_batch;
		tb->tbuf.indeed_batch = (float)indeed;
		tb->net_backward(nullptr, nullptr, n, coords, valid, (const half_t*)dlo, grads_out, s);
		tb->tbuf.indeed_batch = saved;
		HIP_CHECK(hipGetLastError());
	});
}
int neus_net_backward_pos(NeusTestbed* tb, void* stream, uint32_t n, const float* coords, uint32_t valid, const uint16_t* dlo,
                          uint32_t indeed, float* grads_out, float* dpos) {
	return guard([&] {
		if (!tb->have_net) throw std::runtime_error("no network");
		if (n == 0 || n % 128 != 0) throw std::runtime_error("neus_net_backward_pos: batch must be a positive multiple of 128");
		if (n > tb->batch) throw std::runtime_error("neus_net_backward_pos: n exceeds batch_size");
		hipStream_t s = as_stream(tb, stream);
		HIP_CHECK(hipMemsetAsync(grads_out, 0, (size_t)tb->lay.P * 4, s));
		const float saved = tb->tbuf.indeed_batch;
		tb->tbuf.indeed_batch = (float)indeed;
		tb->tbuf.dpos = (float4*)dpos;
		tb->net_backward(nullptr, nullptr, n, coords, valid, (const half_t*)dlo, grads_out, s);
		tb->tbuf.dpos = nullptr;
		tb->tbuf.indeed_batch = saved;
		HIP_CHECK(hipGetLastError());
	});
}
int neus_delta_apply(NeusTestbed* tb, void* stream, uint32_t n, uint32_t stride, const float* in, float* out) {
	return guard([&] {
		if (!tb->have_net) throw std::runtime_error("no network");
		if (stride != 3 && stride != COORD_W) throw std::runtime_error("neus_delta_apply: stride must be 3 or 7");
		hipStream_t s = as_stream(tb, stream);
		launch_delta_prepare(s, tb->delta.p);
		launch_delta_apply(s, nullptr, n, stride, in, out, tb->delta.p);
		HIP_CHECK(hipGetLastError());
	});
}
int neus_delta_backward(NeusTestbed* tb, void* stream, uint32_t n, uint32_t stride, const float* coords, const float* dpos, float* grads12) {
	return guard([&] {
		if (!tb->have_net) throw std::runtime_error("no network");
		hipStream_t s = as_stream(tb, stream);
		launch_delta_prepare(s, tb->delta.p);
		DeltaAdam a{0.f, 0.f, 0.f, 0.f, LOSS_SCALE, 0u};
		launch_delta_backward(s, nullptr, n, coords, stride, (const float4*)dpos, tb->delta.p, tb->delta_partial.p, a);
		DeltaState h{};
		HIP_CHECK(hipMemcpyAsync(&h, tb->delta.p, sizeof(h), hipMemcpyDeviceToHost, s));
		HIP_CHECK(hipStreamSynchronize(s));
		std::memcpy(grads12, h.grad, DELTA_PARAMS * 4);
	});
}
static void sample_rays_impl(NeusTestbed* tb, void* stream, uint32_t n_rays, uint32_t rank, uint32_t world, uint32_t n_rays_total,
                             uint64_t rng_state, uint64_t rng_inc, uint32_t max_samples, const uint8_t* bitfield, float* rays, uint32_t* numsteps,
                             float* coords, uint32_t* counters_out, uint32_t e1, uint32_t* list, uint32_t* list_len, uint32_t lds_fill);
int neus_sample_rays(NeusTestbed* tb, void* stream, uint32_t n_rays, uint32_t rank, uint32_t world, uint32_t n_rays_total,
                     uint64_t rng_state, uint64_t rng_inc, uint32_t max_samples, const uint8_t* bitfield, float* rays, uint32_t* numsteps,
                     float* coords, uint32_t* counters_out) {
	return guard([&] {
		sample_rays_impl(tb, stream, n_rays, rank, world, n_rays_total, rng_state, rng_inc, max_samples, bitfield, rays, numsteps, coords, counters_out,
		                 0u, nullptr, nullptr, 0u);
	});
}
int neus_debug_sample_rays_round0(NeusTestbed* tb, void* stream, uint32_t n_rays, uint32_t n_rays_total, uint64_t rng_state, uint64_t rng_inc,
                                  uint32_t max_samples, const uint8_t* bitfield, float* rays, uint32_t* numsteps, float* coords, uint32_t* counters_out,
                                  uint32_t chunk_end, uint32_t* list, uint32_t* list_len, uint32_t lds_fill) {
	return guard([&] {
		if (chunk_end == 0 || !list || !list_len) throw std::runtime_error("sample_rays_round0: chunk_end > 0, list and list_len required");
		sample_rays_impl(tb, stream, n_rays, 0u, 1u, n_rays_total, rng_state, rng_inc, max_samples, bitfield, rays, numsteps, coords, counters_out,
		                 chunk_end, list, list_len, lds_fill);
	});
}
int neus_debug_scan_giveup(void* stream, const uint32_t* in, uint32_t* out, uint32_t n, uint32_t* failures) {
	return guard([&] {
		hipStream_t s = (hipStream_t)stream;
		ScanTemp tmp; tmp.alloc(scan_temp_bytes(n) + 256); scan_temp_reset(s, tmp.p);
		debug_scan_skip_first_tile(s, tmp.p, in, out, n);
		HIP_CHECK(hipStreamSynchronize(s));
		*failures = scan_failures(tmp.p);
	});
}
int neus_debug_set_lds_fill(NeusTestbed* tb, uint32_t pattern) { return guard([&] { tb->dbg_lds_fill = pattern; }); }
int neus_debug_set_lds_fill_all(NeusTestbed* tb, uint32_t pattern) { return guard([&] { tb->dbg_lds_fill_all = pattern; }); }
int neus_debug_set_xcd_shift(NeusTestbed* tb, uint32_t n_blocks) { return guard([&] { tb->dbg_xcd_shift = n_blocks; }); }
int neus_debug_set_grid_generic(uint32_t on) { return guard([&] { g_dbg_grid_generic = on; }); }
// Diagnostic: `launches` launches of the fp32-denormal probe on a stream of its own (device `device`), each compared with
// the CPU's bits; stats as debug_denorm_probe (march.hip)
int neus_debug_denorm_probe(int device, uint32_t n, uint32_t launches, uint64_t* stats) {
	return guard([&] {
		if (!stats || n == 0) throw std::runtime_error("neus_debug_denorm_probe: bad argument");
		HIP_CHECK(hipSetDevice(device));
		const Stream s = make_stream(hipStreamNonBlocking);
		debug_denorm_probe(s.get(), n, launches, stats);
	});
}
// Development: raw bytes of one step-workspace buffer (ids: 0 sa, 1 ekt, 2 ck4, 3 cke, 4 racc, 5 rgr, 6 rT, 7 rek,
// 8 ccount, 9 net_out, 10 coords, 11 base, 12 numsteps, 13 cmap, 14 nreq; the occupancy update's products: 40 bf_lin,
// 41 occ_bbox, 42 grid_mean, 43 density_tmp)
int neus_debug_get_buffer(NeusTestbed* tb, int id, uint64_t offset, uint64_t nbytes, void* host) {
	return guard([&] {
		if (!tb->have_net) throw std::runtime_error("no network");
		const void* p = nullptr;
		size_t cap = 0;
		auto pick = [&](const void* q, size_t bytes) { p = q; cap = bytes; };
		switch (id) {
		case 0: pick(tb->l_sa.p, tb->l_sa.n * 16); break;
		case 1: pick(tb->l_ekt.p, tb->l_ekt.n * 4); break;
		case 2: pick(tb->l_ck4.p, tb->l_ck4.n * 16); break;
		case 3: pick(tb->l_cke.p, tb->l_cke.n * 4); break;
		case 4: pick(tb->l_racc.p, tb->l_racc.n * 16); break;
		case 5: pick(tb->l_rgr.p, tb->l_rgr.n * 16); break;
		case 6: pick(tb->l_rT.p, tb->l_rT.n * 4); break;
		case 7: pick(tb->l_rek.p, tb->l_rek.n * 4); break;
		case 8: pick(tb->ccount.p, tb->ccount.n * 4); break;
		case 9: pick(tb->net_out.p, tb->net_out.n * 2); break;
		case 10: pick(tb->coords.p, tb->coords.n * 4); break;
		case 11: pick(tb->base.p, tb->base.n * 4); break;
		case 12: pick(tb->numsteps.p, tb->numsteps.n * 4); break;
		case 13: pick(tb->cmap.p, tb->cmap.n * 4); break;
		case 14: pick(tb->nreq.p, tb->nreq.n * 4); break;
		case 15: pick(tb->dbg_dl.p, tb->dbg_dl.n * 2); break;
		case 20: case 21: case 22: case 23: case 24: case 25: case 26: case 27: case 28: case 29: case 30: case 31: case 32: case 33: case 34:
			pick(tb->dbg_snap[id - 20].p, tb->dbg_snap[id - 20].n); break;
		case 40: pick(tb->bf_lin.p, (size_t)LIN_WORDS * 4); break;
		case 41: pick(tb->occ_bbox.p, 6 * 4); break;
		case 42: pick(tb->grid_mean.p, 4); break;
		case 43: pick(tb->density_tmp.p, (size_t)GRID3 * 4); break;
		default: throw std::runtime_error("debug_get_buffer: unknown id");
		}
		if (offset + nbytes > cap) throw std::runtime_error("debug_get_buffer: range past the buffer");
		HIP_CHECK(hipStreamSynchronize(tb->stream));
		HIP_CHECK(hipMemcpy(host, (const char*)p + offset, nbytes, hipMemcpyDeviceToHost));
	});
}
// Development: k_loss_grad replayed on the last step's state (same inputs as the step's launch) into separate outputs;
// dl_dout_out: batch x 16 fp16 bits (host). Valid after a static-scene step at the default options.
int neus_debug_replay_loss_grad(NeusTestbed* tb, uint16_t* dl_dout_out) {
	return guard([&] {
		if (!tb->have_net) throw std::runtime_error("no network");
		NeusTestbed& t = *tb;
		hipStream_t s = t.stream;
		LossParams lp{};
		lp.loss_scale = LOSS_SCALE; lp.ek_w = t.cfg.ek_loss_weight; lp.mask_w = t.cfg.mask_loss_weight;
		// the cos-anneal of the step that ran (training_step was incremented after it)
		const int ts = (int)t.training_step - 1;
		lp.cos_anneal = t.cfg.anneal_end == 0 ? 1.0f : std::min(1.0f, (float)std::max(ts, 0) / t.cfg.anneal_end);
		lp.max_compacted = t.batch;
		const LossWork w = t.loss_work(t.base.p);
		Dev<float> co; co.alloc((size_t)t.batch * COORD_W);
		Dev<half_t> dl; dl.alloc((size_t)t.batch * OUT_W);
		HIP_CHECK(hipMemsetAsync(dl.p, 0, dl.n * 2, s));
		launch_loss_grad(s, t.max_samples, t.st.p, t.dp_info(), lp, t.coords.p, t.net_out.p, t.numsteps.p, w, co.p, dl.p);
		HIP_CHECK(hipStreamSynchronize(s));
		HIP_CHECK(hipMemcpy(dl_dout_out, dl.p, dl.n * 2, hipMemcpyDeviceToHost));
	});
}
int neus_debug_get_batch(NeusTestbed* tb, float* coords_out, uint16_t* dl_dout_out, float* loss_out) {
	return guard([&] {
		if (!tb->have_net) throw std::runtime_error("no network");
		HIP_CHECK(hipStreamSynchronize(tb->stream));
		if (coords_out) HIP_CHECK(hipMemcpy(coords_out, tb->coords_c.p, (size_t)tb->batch * COORD_W * 4, hipMemcpyDeviceToHost));
		if (dl_dout_out) HIP_CHECK(hipMemcpy(dl_dout_out, tb->dL_dout.p, (size_t)tb->batch * OUT_W * 2, hipMemcpyDeviceToHost));
		if (loss_out) HIP_CHECK(hipMemcpy(loss_out, tb->loss.p, (size_t)MAX_RAYS * 4, hipMemcpyDeviceToHost));
	});
}
int neus_debug_inject_health(NeusTestbed* tb, uint32_t flags) {
	return guard([&] {
		if (!tb->have_net) throw std::runtime_error("no network");
		HIP_CHECK(hipStreamSynchronize(tb->stream));
		if (flags & STEP_FAIL_MARCH_T) {
			StepState h{};
			HIP_CHECK(hipMemcpy(&h, tb->st.p, sizeof(h), hipMemcpyDeviceToHost));
			h.fail_flags |= STEP_FAIL_MARCH_T;
			HIP_CHECK(hipMemcpy(tb->st.p, &h, sizeof(h), hipMemcpyHostToDevice));
		}
		if (flags & STEP_FAIL_SCAN) {
			const uint32_t one = 1;
			HIP_CHECK(hipMemcpy(tb->scan_tmp.p + offsetof(ScanState, fail), &one, 4, hipMemcpyHostToDevice));
		}
	});
}
static void sample_rays_impl(NeusTestbed* tb, void* stream, uint32_t n_rays, uint32_t rank, uint32_t world, uint32_t n_rays_total,
                             uint64_t rng_state, uint64_t rng_inc, uint32_t max_samples, const uint8_t* bitfield, float* rays, uint32_t* numsteps,
                             float* coords, uint32_t* counters_out, uint32_t e1, uint32_t* list, uint32_t* list_len, uint32_t lds_fill) {
	{
		if (!tb->have_data || !tb->have_net) throw std::runtime_error("no dataset/network");
		if (n_rays == 0 || n_rays > MAX_RAYS) throw std::runtime_error("n_rays out of range");
		hipStream_t s = as_stream(tb, stream);
		Dev<StepState> sst; sst.alloc(1);
		StepState h{}; h.rays_per_batch = n_rays; h.max_inference = max_samples; h.n_rays_total = n_rays_total;
		HIP_CHECK(hipMemcpyAsync(sst.p, &h, sizeof(h), hipMemcpyHostToDevice, s));
		Dev<float> st_t; st_t.alloc(n_rays); Dev<uint32_t> nr, bs, nrec, q; nr.alloc(n_rays); bs.alloc(n_rays); nrec.alloc(n_rays); q.alloc(2);
		Dev<uint2> rec; rec.alloc((size_t)n_rays * NERF_STEPS);
		Dev<uint2> seg; seg.alloc((size_t)n_rays * MARCH_SEG_RECS);
		MarchWork mw{rec.p, nrec.p, q.p, tb->mwork.waves, seg.p, tb->mwork.lanes_per_ray};
		mw.balanced = tb->mwork.balanced;
		ScanTemp tmp; const size_t tb_ = scan_temp_bytes(n_rays); tmp.alloc(tb_ + 256); scan_temp_reset(s, tmp.p);
		Dev<uint32_t> lin; lin.alloc(LIN_WORDS);
		launch_bitfield_linear(s, bitfield, lin.p);
		// the occupied-box cull of the training step, from this bitfield (exact: culled rays march to zero samples)
		Dev<float> bb; bb.alloc(occ_bbox_scratch_floats());
		launch_occ_bbox(s, bitfield, bb.p);
		// progressive round 0's list (the training step's, written by the march): its slots and counters
		Dev<uint32_t> c0, cnt;
		if (list) { c0.alloc(n_rays); cnt.alloc(2); }
		const Round0List r0{e1, c0.p, list, cnt.p, 2u};
		launch_march_count(s, n_rays, max_samples, sst.p, DPInfo{rank, world}, tb->ds, bitfield, lin.p, rng_state, rng_inc, rays, st_t.p, nr.p, mw,
		                   list ? cnt.p : nullptr, list ? 2u : 0u, tb->opt.ray_cull ? bb.p : nullptr);
		Dev<uint32_t> sr; sr.alloc(std::max<uint32_t>(1, max_samples));
		launch_march_write(s, n_rays, sst.p, tb->ds, rays, mw, nr.p, bs.p, numsteps, coords, sr.p, max_samples, tmp.p, list ? &r0 : nullptr, lds_fill);
		HIP_CHECK(hipMemcpyAsync(&h, sst.p, sizeof(h), hipMemcpyDeviceToHost, s));
		if (list) HIP_CHECK(hipMemcpyAsync(list_len, cnt.p, 4, hipMemcpyDeviceToHost, s));
		HIP_CHECK(hipStreamSynchronize(s));
		if (h.fail_flags) throw std::runtime_error("sample_rays: the march met a non-finite or negative t");
		if (scan_failures(tmp.p)) throw std::runtime_error("sample_rays: the look-back scan gave up");
		counters_out[0] = h.numsteps_counter; counters_out[1] = h.n_kept; counters_out[2] = h.n_rays_with_samples;
	}
}
int neus_loss_compact(NeusTestbed* tb, void* stream, uint32_t n_rays, uint32_t rank, uint32_t world, uint32_t n_rays_total,
                      uint64_t rng_state, uint64_t rng_inc, uint32_t max_compacted, const float* rays, uint32_t* numsteps,
                      const float* coords, const uint16_t* net_out, float* coords_out, uint16_t* dlo, float* loss, float* ek,
                      float* mask, uint32_t* counters_out) {
	return guard([&] {
		if (!tb->have_data || !tb->have_net) throw std::runtime_error("no dataset/network");
		if (n_rays == 0 || n_rays > MAX_RAYS) throw std::runtime_error("n_rays out of range");
		hipStream_t s = as_stream(tb, stream);
		// sample count of the caller's layout (operator path only; the training step keeps it on the device)
		std::vector<uint32_t> hn(2 * (size_t)n_rays);
		HIP_CHECK(hipMemcpyAsync(hn.data(), numsteps, hn.size() * 4, hipMemcpyDeviceToHost, s));
		HIP_CHECK(hipStreamSynchronize(s));
		uint32_t n_samples = 1;
		for (uint32_t i = 0; i < n_rays; ++i) if (hn[2 * i]) n_samples = std::max(n_samples, hn[2 * i] + hn[2 * i + 1]);
		Dev<StepState> sst; sst.alloc(1);
		StepState h{}; h.rays_per_batch = n_rays; h.n_rays_total = n_rays_total;
		HIP_CHECK(hipMemcpyAsync(sst.p, &h, sizeof(h), hipMemcpyHostToDevice, s));
		Dev<uint32_t> cc, cb, rb, sr; cc.alloc(n_rays); cb.alloc(n_rays); rb.alloc(n_rays); sr.alloc(n_samples);
		Dev<float4> sa, ck4, racc, rgr; sa.alloc(n_samples); ck4.alloc(n_samples / 8 + 1); racc.alloc(n_rays); rgr.alloc(n_rays);
		Dev<float> ekt, cke, rT; ekt.alloc(n_samples); cke.alloc(n_samples / 8 + 1); rT.alloc(n_rays);
		ScanTemp tmp; const size_t tb_ = scan_temp_bytes(n_rays); tmp.alloc(tb_ + 256); scan_temp_reset(s, tmp.p);
		LossParams lp{};
		lp.loss_scale = LOSS_SCALE; lp.ek_w = tb->cfg.ek_loss_weight; lp.mask_w = tb->cfg.mask_loss_weight; lp.cos_anneal = tb->cos_anneal();
		lp.max_compacted = max_compacted; lp.rng_state = rng_state; lp.rng_inc = rng_inc;
		LossWork w{};
		w.sa = sa.p; w.ck4 = ck4.p; w.cke = cke.p; w.ekt = ekt.p; w.sample_ray = sr.p; w.rbase = rb.p; w.racc = racc.p; w.rT = rT.p; w.rgr = rgr.p;
		Dev<uint32_t> cm; cm.alloc(std::max(1u, max_compacted)); w.cmap = cm.p;
		Dev<uint32_t> lr, nl; lr.alloc(n_rays); nl.alloc(1);
		w.long_rays = lr.p; w.n_long = nl.p;
		const DPInfo dp{rank, world};
		launch_ray_index(s, n_rays, numsteps, sst.p, sr.p, rb.p);
		launch_loss_alpha(s, n_samples, sst.p, coords, (const half_t*)net_out, lp.cos_anneal, w);
		launch_loss_scan_ray(s, n_rays, numsteps, w, cc.p);
		launch_exclusive_scan(s, tmp.p, tb_, cc.p, cb.p, n_rays);
		launch_loss_ray(s, n_rays, sst.p, dp, tb->ds, lp, numsteps, cc.p, cb.p, w, loss, ek, mask);
		launch_loss_grad(s, n_samples, sst.p, dp, lp, coords, (const half_t*)net_out, numsteps, w, coords_out, (half_t*)dlo);
		HIP_CHECK(hipMemcpyAsync(&h, sst.p, sizeof(h), hipMemcpyDeviceToHost, s));
		HIP_CHECK(hipStreamSynchronize(s));
		counters_out[0] = h.compacted_counter;
	});
}
int neus_optimizer_step(NeusTestbed* tb, void* stream, const float* grads) {
	return guard([&] {
		if (!tb->have_net) throw std::runtime_error("no network");
		if (stream && (hipStream_t)stream != tb->stream) HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
		tb->optimizer_step(grads);
		HIP_CHECK(hipStreamSynchronize(tb->stream));
	});
}
int neus_fill_rollover(NeusTestbed* tb, void* stream, uint32_t n_elements, uint32_t n_in, float* coords, uint16_t* dL_dout) {
	return guard([&] {
		if (!tb) throw std::runtime_error("fill_rollover: null testbed");
		hipStream_t s = as_stream(tb, stream);
		Dev<StepState> sst; sst.alloc(1);
		StepState h{}; h.compacted_counter = n_in;
		HIP_CHECK(hipMemcpyAsync(sst.p, &h, sizeof(h), hipMemcpyHostToDevice, s));
		launch_rollover(s, n_elements, sst.p, coords, (half_t*)dL_dout);
		HIP_CHECK(hipStreamSynchronize(s));
	});
}
int neus_occ_update(NeusTestbed* tb, void* stream, uint32_t n_uniform, uint32_t n_nonuniform) {
	return guard([&] {
		if (!tb->have_net) throw std::runtime_error("no network");
		(void)stream;
		tb->occ_update(n_uniform, n_nonuniform, tb->valid_level_at((int)tb->training_step));
		HIP_CHECK(hipStreamSynchronize(tb->stream));
	});
}
int neus_mfma_probe(const uint16_t* A, const uint16_t* B, float* C) {
	return guard([&] {
		launch_mfma_probe(nullptr, (const half_t*)A, (const half_t*)B, C);
		HIP_CHECK(hipDeviceSynchronize());
	});
}

} // extern "C"
