// The NEUS_* tuning switches: the one place under csrc/ that reads the environment (hostgroup.h's rendezvous settings
// aside). Plain C++17, no HIP header. Three times of effect, one function each:
//   NeusOptions::from_env()   at testbed creation; holds for that testbed's life (reloads, snapshots, frames included)
//   process_options()         at the first launch of the process: the MLP launchers, which the module API calls with no testbed
//   alloc_debug_from_env()    at neus_testbed_create: the allocation debug pair, for every allocation of the process until the next
// DESIGN.md "Options" lists every variable with its kind and the test or profile that uses it.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace neus_env {
inline bool on_unless_0(const char* name) { const char* e = std::getenv(name); return !(e && e[0] == '0'); }  // default on
inline bool off_unless_1(const char* name) { const char* e = std::getenv(name); return e && e[0] == '1'; }    // default off
inline bool is(const char* name, const char* value) { const char* e = std::getenv(name); return e && std::strcmp(e, value) == 0; }
inline int as_int(const char* name, int def) { const char* e = std::getenv(name); return e ? std::atoi(e) : def; }
inline uint32_t as_u32(const char* name, uint32_t def) { const char* e = std::getenv(name); return e ? (uint32_t)std::strtoul(e, nullptr, 10) : def; }
inline float as_float(const char* name, float def) { const char* e = std::getenv(name); return e ? (float)std::atof(e) : def; }
// "e0,e1,...": 1 to 14 values, the first > 0, strictly increasing; anything else is ignored (empty result)
inline std::vector<uint32_t> increasing_list(const char* name) {
	std::vector<uint32_t> v;
	const char* e = std::getenv(name);
	if (!e) return v;
	for (const char* p = e; *p;) { char* q = nullptr; const unsigned long x = std::strtoul(p, &q, 10); if (q == p) break; v.push_back((uint32_t)x); p = *q ? q + 1 : q; }
	bool ok = !v.empty() && v.size() <= 14 && v[0] > 0;
	for (size_t k = 1; k < v.size(); ++k) ok = ok && v[k] > v[k - 1];
	if (!ok) v.clear();
	return v;
}
}  // namespace neus_env

struct NeusOptions {
	// ---- streams and the lookahead
	// NEUS_MAIN_PRIO=0: the step's streams at the default priority, not the highest. Explicit priorities keep a testbed created
	// after another was destroyed at 1.24 ms/step (16-level leg) where the default ran 1.91 (profiles/r05l16_priorities_ab.txt)
	bool main_prio = true;
	// NEUS_LOOKAHEAD=0: no sampling of the next step beside this step's backward (A/B reference; step_plan.h StepPlan::la_go)
	bool lookahead = true;
	// NEUS_LA_AT: where in the backward a cut march's lookahead is issued (NeusTestbed::la_at). 1, after the encode: 0.770 ->
	// 0.759 ms/step at step 800, 0.876 -> 0.854 at step 1600 against 0 (profiles/r06la_issue_point_ab.txt)
	int la_at_cut = 1;
	// NEUS_LA_AT_FULL: the same for a full march, which needs the whole backward to hide in. 0, right after the loss (round 5:
	// 1 as 0, 2 and 3 slower, profiles/r05la_issue_point_ab.txt)
	int la_at_full = 0;
	// NEUS_LA_PRIO: the lookahead stream's priority, -1 lowest, 0 default, 1 highest. Lowest: 1.154 -> 1.107 ms/step at the
	// bench state (default 1.139, highest 1.141: profiles/r05lap_lookahead_priority_ab.txt)
	int la_prio = -1;
	// NEUS_EV_SYSFENCE=1: keep the system-scope fence on the events between the step's and the lookahead's streams (A/B; its
	// L2 write-back held the step's stream ~6 us at the record)
	bool ev_sysfence = false;
	// NEUS_LA_STAT=1: development; timing events around every lookahead, summed on stderr at the end of each train call
	bool la_stat = false;
	// NEUS_ADAM_OVERLAP=1: the optimizer in pieces beside the grid scatter, bitwise the one launch (A/B; test_gpu_overlap.py,
	// profiles/r06b_adam_overlap_mlp_grid_ab.txt)
	bool adam_overlap = false;
	// NEUS_EXCHANGE_OVERLAP=0: one grouped gradient exchange after the backward (A/B reference). The initial value
	// of NeusTestbed::exchange_overlap, which neus_testbed_set_exchange_overlap changes
	bool exchange_overlap = true;
	// NEUS_EAGER_EMA_H=1: the Adam kernel writes the fp16 EMA weights every step instead of a cast at their first read
	bool eager_ema_h = false;

	// ---- sampling: march, ray order, progressive rounds, cuts
	// NEUS_MARCH_WAVES: march waves launched; 0 = one lane per ray slot. The march is latency-bound and every wave fewer was
	// slower (R = 2^18: 4096 waves 0.58 ms, 2048 0.75 ms, 1024 1.28 ms)
	uint32_t march_waves = 0;
	// NEUS_MARCH_LANES: lanes marching one ray, 1 / 4 / 16; anything else gives 8. Config S, R = 2^18, step 5: sampling 0.52 ms
	// with 1 lane, 0.24 with 4, 0.21 with 8 (test_gpu_parity.py compares them bitwise)
	uint32_t march_lanes = 8;
	// NEUS_MARCH_BALANCE=0: a fixed 8 lanes per ray instead of a wave's lanes shared by ray length (A/B reference)
	bool march_balance = true;
	// NEUS_MARCH_DBG: development; MarchWork::dbg of neus_debug_march_profile's march
	uint32_t march_dbg = 0;
	// NEUS_RAY_CULL=0: march every ray, without the occupied cells' bounding-box cull (A/B reference)
	bool ray_cull = true;
	// NEUS_RAY_SORT=0: the progressive rounds' rays in slot order, not the spatial order (A/B reference)
	bool ray_sort = true;
	// NEUS_PROG_CUT=0: no compaction cut (A/B reference; step_plan.h plan_sampling: cut)
	bool prog_cut = true;
	// NEUS_MARCH_CUT=0: no march cut (A/B reference; step_plan.h plan_sampling: mcut)
	bool march_cut = true;
	// NEUS_DBG_MARCH_CUT_DIV: test hook, at least 1; divides the march cut's estimate so that witnesses fail and steps re-run
	uint32_t march_cut_div = 1;
	// NEUS_CHUNK_ENDS="e0,e1,...": fixed chunk ends of the progressive rounds instead of the auto rule (A/B of schedules,
	// profiles/r04fg_chunk_ends_sweep.txt); empty = auto
	std::vector<uint32_t> chunk_ends;
	// NEUS_CHUNK_SCALE / NEUS_CHUNK_ROUNDS (2 or 3): a cut step's first chunk relative to the auto rule's, and its rounds (sweeps).
	// Two rounds, twice as long: steps 800 / 1600 0.815 / 0.895 -> 0.773 / 0.878 ms/step (profiles/r06y_chunk_ends_cut_sweep.txt)
	float chunk_scale = 2.f;
	int chunk_rounds = 2;
	// NEUS_SCAN_FORM=lane / group: the progressive rounds' chunk scans one lane per ray (1) or 16 lanes per ray (2) on every step
	// (bitwise A/B references; test_gpu_scan_chunk_forms.py); auto (0): 16 lanes per ray on the cut steps
	uint32_t scan_form = 0;

	// ---- occupancy update
	// NEUS_OCC_SORT=0: the uniform samples in index order, not cell order (A/B reference)
	bool occ_sort = true;
	// NEUS_OCC_NU_SORT=1: the occupancy-biased samples binned by coarse cell too. Bitwise the same grid, but 0.756-0.764 ->
	// 0.765-0.771 ms/step at step 800 (profiles/r06occ_nu_sort_ab.txt: the binning's atomics cost more than the pass saves)
	bool occ_nu_sort = false;

	// ---- grid-gradient scatter
	// NEUS_SCATTER=wide / binned: the wide-block (0) or the 256-sample (1) histogram / scan / bin paths instead of the per-block
	// record regions (2) (bitwise A/B references; test_gpu_scatter.py)
	uint32_t scatter_mode = 2;
	// NEUS_SCATTER_CHUNK=1024 / 256: samples per binning workgroup; anything else gives 512. Modes 0 and 1 have no 256: 512
	uint32_t scatter_chunk = 512;
	// NEUS_SCATTER_LG=k: k workgroups per chunk, each binning every k-th level; 0 = one per level
	uint32_t scatter_level_groups = 0;
	// NEUS_SC_XCD_GROUP: ScatterWork::xcd_group of the region scatter's accumulation, at least 1
	uint32_t scatter_xcd_group = 4;
	// NEUS_SCATTER_NOSKIP=1: zero the whole grid gradient before every scatter (A/B reference; test_gpu_scatter.py)
	bool scatter_noskip = false;

	// ---- loss debugging
	// NEUS_DBG_LOSS_REPLAY=1: development; the loss-gradient launch again into separate outputs (and no lookahead)
	bool dbg_loss_replay = false;
	// NEUS_DBG_LOSS_FENCE=1: development; an agent-scope acquire fence at the loss-gradient kernel's start
	bool dbg_loss_fence = false;

	static NeusOptions from_env() {
		using namespace neus_env;
		NeusOptions o;
		o.main_prio = on_unless_0("NEUS_MAIN_PRIO");
		o.lookahead = on_unless_0("NEUS_LOOKAHEAD");
		o.la_at_cut = as_int("NEUS_LA_AT", o.la_at_cut);
		o.la_at_full = as_int("NEUS_LA_AT_FULL", o.la_at_full);
		o.la_prio = as_int("NEUS_LA_PRIO", o.la_prio);
		o.ev_sysfence = off_unless_1("NEUS_EV_SYSFENCE");
		o.la_stat = off_unless_1("NEUS_LA_STAT");
		o.adam_overlap = off_unless_1("NEUS_ADAM_OVERLAP");
		o.exchange_overlap = on_unless_0("NEUS_EXCHANGE_OVERLAP");
		o.eager_ema_h = off_unless_1("NEUS_EAGER_EMA_H");
		o.march_waves = as_u32("NEUS_MARCH_WAVES", o.march_waves);
		{ const uint32_t v = as_u32("NEUS_MARCH_LANES", 8); o.march_lanes = v == 1 || v == 4 || v == 16 ? v : 8u; }
		o.march_balance = on_unless_0("NEUS_MARCH_BALANCE");
		o.march_dbg = as_u32("NEUS_MARCH_DBG", o.march_dbg);
		o.ray_cull = on_unless_0("NEUS_RAY_CULL");
		o.ray_sort = on_unless_0("NEUS_RAY_SORT");
		o.prog_cut = on_unless_0("NEUS_PROG_CUT");
		o.march_cut = on_unless_0("NEUS_MARCH_CUT");
		o.march_cut_div = (uint32_t)std::max(1, as_int("NEUS_DBG_MARCH_CUT_DIV", 1));
		o.chunk_ends = increasing_list("NEUS_CHUNK_ENDS");
		o.chunk_scale = as_float("NEUS_CHUNK_SCALE", o.chunk_scale);
		o.chunk_rounds = as_int("NEUS_CHUNK_ROUNDS", o.chunk_rounds);
		o.scan_form = is("NEUS_SCAN_FORM", "lane") ? 1u : is("NEUS_SCAN_FORM", "group") ? 2u : 0u;
		o.occ_sort = on_unless_0("NEUS_OCC_SORT");
		o.occ_nu_sort = off_unless_1("NEUS_OCC_NU_SORT");
		o.scatter_mode = is("NEUS_SCATTER", "binned") ? 1u : is("NEUS_SCATTER", "wide") ? 0u : 2u;
		o.scatter_chunk = is("NEUS_SCATTER_CHUNK", "1024") ? 1024u : is("NEUS_SCATTER_CHUNK", "256") ? 256u : 512u;
		if (o.scatter_mode != 2 && o.scatter_chunk == 256) o.scatter_chunk = 512;
		o.scatter_level_groups = (uint32_t)std::max(0, as_int("NEUS_SCATTER_LG", 0));
		o.scatter_xcd_group = std::max(1u, as_u32("NEUS_SC_XCD_GROUP", o.scatter_xcd_group));
		o.scatter_noskip = off_unless_1("NEUS_SCATTER_NOSKIP");
		o.dbg_loss_replay = off_unless_1("NEUS_DBG_LOSS_REPLAY");
		o.dbg_loss_fence = off_unless_1("NEUS_DBG_LOSS_FENCE");
		return o;
	}
};

// The MLP launchers' switches (mlp.hip), process-wide: read once, at the first launch.
struct NeusProcessOptions {
	bool infer_xcd_parts = false;   // NEUS_INFER_XCD_PARTS=1: part x of the inference list on XCD x (scripts/exp_xcd_infer.py)
	bool infer_pipe = true;         // NEUS_INFER_PIPE=0: never the all-levels (pipelined) inference kernel (A/B reference)
	uint32_t infer_grid = 0;        // NEUS_INFER_GRID: development; a cap on the inference grid, 0 = none
	uint32_t mlp_blocks_pct = 100;  // NEUS_MLP_BLOCKS_PCT: development; the training MLP grid in % of the resident capacity
	static NeusProcessOptions from_env() {
		using namespace neus_env;
		NeusProcessOptions o;
		o.infer_xcd_parts = off_unless_1("NEUS_INFER_XCD_PARTS");
		o.infer_pipe = on_unless_0("NEUS_INFER_PIPE");
		o.infer_grid = (uint32_t)as_int("NEUS_INFER_GRID", 0);
		o.mlp_blocks_pct = (uint32_t)as_int("NEUS_MLP_BLOCKS_PCT", 100);
		return o;
	}
};
inline const NeusProcessOptions& process_options() {
	static const NeusProcessOptions o = NeusProcessOptions::from_env();
	return o;
}

// NEUS_DBG_POISON="byte[:lo:hi]" fills the fresh device allocations number lo .. hi-1 (counted from the last
// neus_testbed_create) with `byte`; NEUS_DBG_ALLOC_LOG (set at all) lists them (number, bytes) on stderr. A result that
// changes with the fill reads memory no kernel wrote, i.e. depends on what a recycled allocation held (scripts/diag_recycle.py).
struct NeusAllocDebug {
	bool log = false, poison = false;
	unsigned byte = 0;
	unsigned long long lo = 0, hi = ~0ull;
};
inline NeusAllocDebug alloc_debug_from_env() {
	NeusAllocDebug d;
	d.log = std::getenv("NEUS_DBG_ALLOC_LOG") != nullptr;
	const char* e = std::getenv("NEUS_DBG_POISON");
	d.poison = e && std::sscanf(e, "%u:%llu:%llu", &d.byte, &d.lo, &d.hi) >= 1;
	return d;
}
