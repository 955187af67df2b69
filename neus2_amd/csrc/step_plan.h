// The shape of a training step, decided in one place: which steps update the occupancy grid, read the loss back, run the
// progressive rounds, cut the compaction or the march, look ahead to the next step's sampling. Pure host arithmetic on a
// few integers and flags (StepFacts), the NEUS_* switches (options.h) and the chunk schedule; the step (testbed.cpp
// train_step_body) plans once at its top and then only issues. The lookahead plans the step after it with the same
// function on StepFacts::next().
//
// Host only, plain C++17: no HIP here, so the host-only test program (tests/host/step_plan_main.cpp) builds it under the
// address and undefined-behaviour sanitizers and checks every rule below over a sweep of the facts.
#pragma once

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <vector>

#include "options.h"

namespace neus {

// ---- the cadence
// The occupancy grid is updated at every canonical step below 32, then every (step / 16)-th up to every 16th from 256 on
// (testbed.cu:2660-2690)
inline bool occ_update_at(uint32_t canonical_step) {
	const uint32_t n_prep = std::min(16u, std::max(1u, canonical_step / 16u));
	return canonical_step % n_prep == 0;
}
// The host reads the loss sums and the step's counters back at every 16th step (and at the end of a train call)
inline bool readback_at(uint32_t step) { return step % 16 == 0; }

// ---- progressive (cut-off-aware) inference: whether a step runs in rounds of per-ray chunks, and the chunk ends of the
// rounds before the last (march.hip). mode 0 off, 1 auto (when under PROGRESSIVE_RATIO of the kept samples were
// composited at the last loss readback), 2 always.
struct ChunkSchedule {
	static constexpr float PROGRESSIVE_RATIO = 0.7f;
	static constexpr uint32_t MAX_ENDS = 14;
	int mode = 1;
	std::vector<uint32_t> ends;      // 1 to MAX_ENDS increasing values
	std::vector<uint32_t> ends_cut;  // the chunk ends of a cut step (chosen with ends; empty: ends)
	bool auto_ends;                  // no explicit ends given: on_readback chooses them
	float keep_ratio = 1.f;          // composited / kept samples at the last loss readback
	float chunk_scale;
	int chunk_rounds;

	explicit ChunkSchedule(const NeusOptions& opt)
		: ends(opt.chunk_ends.empty() ? std::vector<uint32_t>{32, 64, 96} : opt.chunk_ends), auto_ends(opt.chunk_ends.empty()),
		  chunk_scale(opt.chunk_scale), chunk_rounds(opt.chunk_rounds) {}

	// neus_testbed_set_progressive_inference: explicit ends (n > 0) switch the auto rule off for good
	void set(int new_mode, const uint32_t* new_ends, uint32_t n) {
		if (new_mode < 0 || new_mode > 2) throw std::runtime_error("progressive inference mode must be 0 (off), 1 (auto) or 2 (always)");
		if (new_ends && n) {
			if (n > MAX_ENDS) throw std::runtime_error("at most 14 chunk ends");
			for (uint32_t k = 0; k < n; ++k)
				if (new_ends[k] == 0 || (k && new_ends[k] <= new_ends[k - 1])) throw std::runtime_error("chunk ends must increase from >= 1");
			ends.assign(new_ends, new_ends + n);
			ends_cut.clear();
			auto_ends = false;
		}
		mode = new_mode;
	}

	// A loss readback's counters (all-reduced: the same on every rank): the keep ratio, and with the auto rule the chunk
	// ends. The mean composited samples per ray with samples, mc, sets three rounds {e, 2e, rest} with e = 0.5 mc + 12
	// rounded to 8 in [24, 128]. Measured at the bench workload (Config S, R = Nc = 2^18,
	// profiles/r04fg_chunk_ends_sweep.txt, r04hi_*): step 800 (mc ~117) best at e = 64 (1.237 ms vs 1.283 for
	// {32, 64, 96}), step 1600 (mc ~39) best at e = 32 (1.203 ms vs 1.308 for e = 64). The rounds only change which
	// samples are evaluated, never a result (bit-identical to the one pass).
	void on_readback(uint32_t compacted_global, uint32_t rays_ws_global, uint32_t n_kept, uint32_t world) {
		const float measured = (float)compacted_global / (float)world;
		keep_ratio = n_kept ? measured / (float)n_kept : 1.f;
		if (!auto_ends || rays_ws_global == 0) return;
		const float mc = (float)compacted_global / (float)rays_ws_global;
		const uint32_t e = std::min(128u, std::max(24u, 8u * (uint32_t)std::lround((0.5f * mc + 12.f) / 8.f)));
		ends.assign({e, 2 * e});
		// With the compaction cut (and the march cut) the later rounds see only the rays before the cut (a few thousand at
		// the bench's shape), so their fixed cost - launches, scans, the cut - outweighs the samples a third round saves:
		// two rounds, the first twice as long (opt.chunk_scale, opt.chunk_rounds).
		const uint32_t ec = std::min(256u, std::max(24u, 8u * (uint32_t)std::lround(chunk_scale * (0.5f * mc + 12.f) / 8.f)));
		if (chunk_rounds == 2) ends_cut.assign({ec});
		else ends_cut.assign({ec, 2 * ec});
	}

	bool progressive() const { return mode == 2 || (mode == 1 && keep_ratio < PROGRESSIVE_RATIO); }
	const std::vector<uint32_t>& ends_for(bool cut) const { return cut && !ends_cut.empty() ? ends_cut : ends; }
};

// ---- the host state a step's decisions read, as it stands when the step starts
struct StepFacts {
	uint32_t step = 0, canonical_step = 0;  // training_step, canonical_step
	uint32_t left = 0;                      // steps of the current train call after this one
	bool next_in_call = false;              // the train call's loop goes on after the step being issued
	bool dyn = false, use_delta = false, train_canonical = true;  // dynamic scenes: frame >= 1, the DeltaNetwork trains, the canonical one does
	bool fixed_rays = false;                // cfg.fixed_rays_per_batch
	bool profiling = false;
	bool balanced = false;                  // the march: MarchWork::balanced, lanes_per_ray; the dataset's cone angle
	uint32_t lanes_per_ray = 8;
	float cone_angle = 0.f;
	uint32_t occ_cells = 0;                 // cells of the occupancy grid's cascades (an update's sample counts)
	bool force_full = false;                // a re-run step: marches every slot
	bool prev_mcut = false;                 // the march of the step issued before this one was cut
	bool loss_pending = false;              // a loss readback is on its way to the host
	bool dbg_hook = false;                  // a test hook that fills LDS or shifts workgroups is set
	bool x_on = false, x_overlap = false;   // the data-parallel exchange: attached, overlapped with the backward

	// The step after this one within the same train call, on a static scene. Every flag as it is, force_full included: the
	// lookahead of a re-run step plans a full march for the step after it
	StepFacts next() const {
		StepFacts n = *this;
		n.step = step + 1;
		n.canonical_step = canonical_step + 1;
		n.left = left ? left - 1 : 0;
		return n;
	}
};

// ---- a step's ray sampling and inference rounds: what issue_march and the rounds' loop need. The lookahead computes the
// next step's and hands it over.
struct SamplingPlan {
	bool progressive = false;  // rounds of per-ray chunks; round 0's list is written by the march
	bool sorted_rays = false;  // round 0's list in the spatial ray order (k_ray_sort_place), not by the march write
	bool cut = false;          // the compaction cut after round 0
	bool mcut = false;         // the march cut: only the slots below the split estimate are generated and marched
	uint32_t nch = 0;          // rounds
	std::array<uint32_t, ChunkSchedule::MAX_ENDS> ends{};  // [nch - 1] chunk ends of the rounds before the last
	bool operator==(const SamplingPlan& o) const {
		return progressive == o.progressive && sorted_rays == o.sorted_rays && cut == o.cut && mcut == o.mcut && nch == o.nch && ends == o.ends;
	}
};

struct StepPlan {
	bool occ_update = false;   // the step starts with an occupancy-grid update ...
	uint32_t occ_uniform = 0, occ_nonuniform = 0;  // ... of this many uniform / occupancy-biased samples
	SamplingPlan sampling;
	bool split = false;        // round 0 in two passes around the cut estimate (the split sort)
	bool scan_group = false;   // the chunk scans' form: 16 lanes per ray
	bool get_loss = false;     // the host reads this step's loss and counters back
	bool risky = false;        // a march-cut witness can fail on this step: the host waits for its word
	bool la_go = false;        // the next step's sampling is issued beside this step's backward
	bool xo = false;           // the gradients' exchange overlaps the backward
	bool a_over = false;       // the optimizer steps in pieces beside the scatter
	bool canon_opt = false;    // the canonical optimizer steps
};

// The compaction cut changes the summed composited count of its step, which feeds the logged loss scale, the chunk-end
// rule and the stats: a step that the host reads back (a loss readback step, the last step of a train call) never cuts.
// It needs fixed rays per batch and a static scene. The number of rounds is that of the uncut schedule.
// The march cut rides on a cut step with the spatial ray order, on the balanced 8-lane march without cones. Its witness
// reaches the host a step late, so it never runs on the last two steps of a train call or before a loss readback step,
// and never at or before an occupancy update (the re-run recounts the step before on the same bitfield; the rule reads
// the training step).
inline SamplingPlan plan_sampling(const NeusOptions& opt, const ChunkSchedule& sched, const StepFacts& f) {
	SamplingPlan p;
	p.progressive = sched.progressive();
	p.sorted_rays = p.progressive && opt.ray_sort;
	const uint32_t nch_full = (uint32_t)sched.ends.size() + 1;
	p.cut = opt.prog_cut && p.progressive && f.fixed_rays && !f.dyn && !readback_at(f.step) && f.left != 0 && nch_full >= 2 && nch_full <= 15;
	p.mcut = opt.march_cut && !f.force_full && p.cut && p.sorted_rays && !f.profiling && f.balanced && f.lanes_per_ray == 8 &&
	         f.cone_angle == 0.0f && !readback_at(f.step + 1) && f.left >= 2 && !occ_update_at(f.step) && !occ_update_at(f.step + 1);
	const std::vector<uint32_t>& ce = sched.ends_for(p.cut);
	p.nch = (uint32_t)ce.size() + 1;
	std::copy(ce.begin(), ce.end(), p.ends.begin());
	return p;
}

// Everything else of a step, given its sampling: the step's own (plan_step below), or the one the previous step's
// lookahead planned and issued
inline StepPlan plan_step(const NeusOptions& opt, const StepFacts& f, const SamplingPlan& sp) {
	StepPlan p;
	p.occ_update = occ_update_at(f.canonical_step);
	p.occ_uniform = f.step < 256 ? f.occ_cells : f.occ_cells / 4;
	p.occ_nonuniform = f.step < 256 ? 0 : f.occ_cells / 4;
	p.sampling = sp;
	p.split = sp.cut && sp.sorted_rays;
	// (16 lanes per ray on a cut step, whose rounds visit a few thousand rays with chunks of 64 samples and
	// more; one lane per ray on every other step - many rays, short chunks)
	p.scan_group = opt.scan_form == 2 || (opt.scan_form == 0 && sp.cut);
	p.get_loss = readback_at(f.step);
	// (a re-run step is exact by construction: not cut, and the step before it recounted when that one was cut)
	p.risky = (sp.mcut || f.prev_mcut) && !f.force_full;
	// The lookahead: between steps of one train call, on static scenes, and not before a step that starts with a loss
	// readback or an occupancy update (the next step's canonical step is step + 1 there)
	p.la_go = opt.lookahead && f.next_in_call && !f.dyn && !f.use_delta && !f.profiling && !opt.dbg_loss_replay && !f.dbg_hook &&
	          !readback_at(f.step + 1) && !occ_update_at(f.step + 1) && !(p.get_loss && f.loss_pending);
	p.canon_opt = !f.dyn || f.train_canonical;
	p.xo = f.x_on && f.x_overlap && p.canon_opt;
	p.a_over = opt.adam_overlap && !f.dyn && (!f.x_on || p.xo);
	return p;
}

inline StepPlan plan_step(const NeusOptions& opt, const ChunkSchedule& sched, const StepFacts& f) {
	return plan_step(opt, f, plan_sampling(opt, sched, f));
}

} // namespace neus
