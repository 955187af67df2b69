// Stand-alone check of neus2_amd/csrc/step_plan.h (tests/test_step_plan.py builds it with the address and
// undefined-behaviour sanitizers and runs it). No HIP and no library: the header includes none.
//   a. plan_step against the rules as the training step spelled them out before they moved into the header (the two
//      cuts, the occupancy cadence, the progressive rule, the lookahead's conjunction and its hand-shifted arguments for the next
//      step, risky, split, scan_group, xo, a_over, canon_opt), restated below, field by field over the sweep;
//   b. the invariants the comments promise: no cut on a step the host reads back, the march cut's distance from call
//      ends, readbacks and occupancy updates, and that the sampling a lookahead plans for the next step is the one that
//      step would plan for itself;
//   c. the chunk-end rule at hand-computed points, and ChunkSchedule::set's validation.
// The sweep: steps 0..527 (the cadence's three regimes, two periods of the last), 0..3 steps left in the call, modes
// 0 / 1 / 2 with keep ratios 0.5 / 0.7 / 1.0, 1 / 2 / 3 / 14 explicit chunk ends, prog_cut, march_cut, ray_sort,
// fixed_rays, dyn, profiling, balanced, force_full, 4 / 8 lanes, cone angle 0 / 0.01: the full product. To it the same
// product over three schedules whose cut ends differ from their ends in number and value (the auto rule's with two and
// three rounds of a cut step; cut ends beside no ends), each with the four mode / ratio pairs named below: 104 M
// points in all, with the other
// inputs those of a plain step of a call on one rank. The inputs that no sampling rule reads are crossed with that
// product in two more passes: the lookahead's six (lookahead, next_in_call, use_delta, the debug hook, loss_pending,
// dbg_loss_replay: 64 combinations) at steps 0..40 and 250..290, and the rest (scan_form, adam_overlap, x_on, x_overlap,
// train_canonical, prev_mcut: 96 combinations) at steps 254..274, which hold readbacks, occupancy updates, the step-256
// change of an update's counts and steps that cut the march. Under the sanitizers a point costs ~0.2 us, so these two
// passes keep 8 of the schedules, one for each way a rule reads one: the mode and keep ratio only through
// progressive() - mode 0 (off at ratio 0.5), mode 1 at 0.5 (on), mode 1 at 0.7 (the threshold itself: off), mode 2 at
// 1.0 (on) - and the ends through their number, 1 and 14 (nch = 2 and 15, the bounds of the cut's rule), and values.
// The sweep runs on up to 16 threads.
// Exit status: 0 and "ok", or 1 after the first failed checks.
#include "step_plan.h"

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <thread>

using namespace neus;

namespace {

std::atomic<int> g_failed{0};
std::mutex g_print;

// ---- the rules as they read in NeusTestbed before step_plan.h
bool old_occ_update_slow(uint32_t cs) { const uint32_t n_prep = std::min(16u, std::max(1u, cs / 16u)); return cs % n_prep == 0; }
// (a table of it: the sweep asks several times per point)
const std::vector<uint8_t> g_occ_tab = [] { std::vector<uint8_t> t(1024); for (uint32_t cs = 0; cs < 1024; ++cs) t[cs] = old_occ_update_slow(cs); return t; }();
bool old_occ_update(uint32_t cs) { return cs < 1024 ? g_occ_tab[cs] != 0 : old_occ_update_slow(cs); }
bool old_progressive(int progressive_mode, float last_keep_ratio) {
	return progressive_mode == 2 || (progressive_mode == 1 && last_keep_ratio < 0.7f);
}
bool old_cut(const NeusOptions& opt, const ChunkSchedule& sc, const StepFacts& f, uint32_t step, bool progressive, bool last_in_call, bool dyn) {
	const uint32_t nch = (uint32_t)sc.ends.size() + 1;
	return opt.prog_cut && progressive && f.fixed_rays && !dyn && step % 16 != 0 && !last_in_call && nch >= 2 && nch <= 15;
}
bool old_march_cut(const NeusOptions& opt, const StepFacts& f, uint32_t step, bool cut, uint32_t left_at_step) {
	if (!opt.march_cut || f.force_full || !cut || f.profiling || !f.balanced || f.lanes_per_ray != 8 || f.cone_angle != 0.0f) return false;
	return (step + 1) % 16 != 0 && left_at_step >= 2 && !old_occ_update(step) && !old_occ_update(step + 1);
}

void report(const char* what, const NeusOptions& opt, const ChunkSchedule& sc, const StepFacts& f) {
	if (++g_failed > 20) return;
	std::lock_guard<std::mutex> lock(g_print);
	std::printf("FAIL %s: step %u cs %u left %u mode %d keep %.2f ends %zu | prog_cut %d march_cut %d ray_sort %d scan_form %u lookahead %d "
	            "replay %d adam %d | fixed %d dyn %d delta %d canon %d prof %d bal %d lanes %u cone %.2f full %d prev %d pend %d hook %d nic %d x %d/%d\n",
	            what, f.step, f.canonical_step, f.left, sc.mode, sc.keep_ratio, sc.ends.size(), opt.prog_cut, opt.march_cut, opt.ray_sort,
	            opt.scan_form, opt.lookahead, opt.dbg_loss_replay, opt.adam_overlap, f.fixed_rays, f.dyn, f.use_delta, f.train_canonical,
	            f.profiling, f.balanced, f.lanes_per_ray, f.cone_angle, f.force_full, f.prev_mcut, f.loss_pending, f.dbg_hook, f.next_in_call,
	            f.x_on, f.x_overlap);
}
#define CHECK(cond) do { if (!(cond)) report(#cond, opt, sc, f); } while (0)

void check_point(const NeusOptions& opt, const ChunkSchedule& sc, const StepFacts& f) {
	const StepPlan p = plan_step(opt, sc, f);
	const SamplingPlan& s = p.sampling;
	const uint32_t training_step = f.step, canonical_step = f.canonical_step, call_left = f.left;

	// ---- a. the rules as they were
	CHECK(p.occ_update == old_occ_update(canonical_step));
	CHECK(occ_update_at(canonical_step) == old_occ_update(canonical_step));
	CHECK(p.occ_uniform == (training_step < 256 ? f.occ_cells : f.occ_cells / 4) && p.occ_nonuniform == (training_step < 256 ? 0u : f.occ_cells / 4));
	const bool progressive = old_progressive(sc.mode, sc.keep_ratio);
	const bool sorted_rays = progressive && opt.ray_sort;
	const bool cut = old_cut(opt, sc, f, training_step, progressive, call_left == 0, f.dyn);
	const bool mcut = old_march_cut(opt, f, training_step, cut && sorted_rays, call_left);
	const std::vector<uint32_t>& ce = cut && !sc.ends_cut.empty() ? sc.ends_cut : sc.ends;
	CHECK(s.progressive == progressive);
	CHECK(s.sorted_rays == sorted_rays);
	CHECK(s.cut == cut);
	CHECK(s.mcut == mcut);
	CHECK(s.nch == (uint32_t)ce.size() + 1);
	CHECK(std::equal(ce.begin(), ce.end(), s.ends.begin()));
	CHECK(p.split == (cut && sorted_rays));
	CHECK(p.scan_group == (opt.scan_form == 2 || (opt.scan_form == 0 && cut)));
	const bool get_loss = training_step % 16 == 0;
	CHECK(p.get_loss == get_loss && readback_at(training_step) == get_loss);
	CHECK(p.risky == ((mcut || f.prev_mcut) && !f.force_full));
	const uint32_t cs1 = training_step + 1;
	const uint32_t n_prep1 = std::min(16u, std::max(1u, cs1 / 16u));
	const bool la_go = opt.lookahead && f.next_in_call && !f.dyn && !f.use_delta && !f.profiling && !opt.dbg_loss_replay && !f.dbg_hook &&
	                   cs1 % 16 != 0 && cs1 % n_prep1 != 0 && !(get_loss && f.loss_pending);
	CHECK(p.la_go == la_go);
	const bool xo = f.x_on && f.x_overlap && (!f.dyn || f.train_canonical);
	CHECK(p.xo == xo);
	CHECK(p.a_over == (opt.adam_overlap && !f.dyn && (!f.x_on || xo)));
	CHECK(p.canon_opt == (!f.dyn || f.train_canonical));

	// ---- b. the invariants
	if (readback_at(f.step) || f.left == 0) CHECK(!s.cut && !s.mcut);
	if (s.mcut) {
		CHECK(s.cut && s.sorted_rays && s.progressive);
		CHECK(f.left >= 2 && !occ_update_at(f.step) && !occ_update_at(f.step + 1) && !readback_at(f.step + 1));
	}
	if (p.la_go) {
		CHECK(!readback_at(f.step + 1) && !occ_update_at(f.step + 1));
		const SamplingPlan nx = plan_step(opt, sc, f.next()).sampling;
		// the next step's plan as the lookahead worked it out by hand: the same functions, every argument shifted
		const bool cut1 = old_cut(opt, sc, f, training_step + 1, progressive, call_left <= 1, false);
		const bool mcut1 = old_march_cut(opt, f, training_step + 1, cut1 && opt.ray_sort, call_left - 1);
		CHECK(nx.progressive == progressive && nx.sorted_rays == sorted_rays && nx.cut == cut1 && nx.mcut == mcut1);
		if (f.left >= 1) {
			// ... and as the next step would plan it for itself, had there been no lookahead (a step in a call has left >= 1
			// when another follows it). A re-run step's lookahead alone differs, as it always did: it never cuts the next
			// step's march (the march cut's rule read the re-running step's force_full), where that step on its own might.
			StepFacts g = f;
			g.step = f.step + 1; g.canonical_step = f.canonical_step + 1; g.left = f.left - 1;
			g.next_in_call = g.left > 0; g.force_full = false; g.prev_mcut = s.mcut;
			SamplingPlan own = plan_step(opt, sc, g).sampling;
			if (f.force_full) own.mcut = false;
			CHECK(nx == own);
		}
	}
}

struct Extra { bool lookahead_inputs, other_inputs; };

void sweep(uint32_t step_lo, uint32_t step_hi, Extra ex) {
	static const uint32_t ends14[14] = {1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610};
	const uint32_t n_la = ex.lookahead_inputs ? 64 : 1, n_other = ex.other_inputs ? 96 : 1;
	// the schedules: all 36, or with the extra inputs the 8 that differ in what a rule reads (the header of this file)
	// ne: that many explicit ends (no cut ends), or the auto rule's after a readback: {72, 144} with cut ends {144}
	// (AUTO_2) or {144, 288} (AUTO_3), or - a state no call reaches, for the lower bound of the cut's round count, which
	// is taken from the ends and never from the cut ends - no ends at all beside cut ends {144} (NO_ENDS)
	const uint32_t AUTO_2 = 100, AUTO_3 = 101, NO_ENDS = 102;
	struct Sched { int mode; float ratio; uint32_t ne; };
	const Sched four[4] = {{0, 0.5f, 0}, {1, 0.5f, 0}, {1, 0.7f, 0}, {2, 1.0f, 0}};  // (the ways progressive() reads mode and ratio)
	std::vector<Sched> scheds;
	if (n_la * n_other == 1) {
		for (int mode = 0; mode < 3; ++mode) for (float ratio : {0.5f, 0.7f, 1.0f}) for (uint32_t ne : {1u, 2u, 3u, 14u}) scheds.push_back({mode, ratio, ne});
		for (uint32_t ne : {AUTO_2, AUTO_3, NO_ENDS}) for (Sched sc : four) scheds.push_back({sc.mode, sc.ratio, ne});
	} else {
		for (uint32_t ne : {1u, 14u}) for (Sched sc : four) scheds.push_back({sc.mode, sc.ratio, ne});
	}
	// the schedules times the three sampling switches, shared out among the threads
	const uint32_t n_items = (uint32_t)scheds.size() * 8;
	std::atomic<uint32_t> next_item{0};
	auto work = [&] {
	for (uint32_t item; (item = next_item++) < n_items;) {
	const int mode = scheds[item / 8].mode;
	const float ratio = scheds[item / 8].ratio;
	const uint32_t ne = scheds[item / 8].ne, ob = item % 8;
	for (uint32_t la = 0; la < n_la; ++la) for (uint32_t ot = 0; ot < n_other; ++ot) {
		NeusOptions opt;
		opt.prog_cut = ob & 1; opt.march_cut = ob & 2; opt.ray_sort = ob & 4;
		opt.chunk_rounds = ne == AUTO_3 ? 3 : 2;
		ChunkSchedule sc(opt);
		sc.set(mode, ends14, ne <= 14 ? ne : 0);
		if (ne > 14) sc.on_readback(117000, 1000, 117000, 1);
		if (ne == NO_ENDS) sc.ends.clear();
		sc.keep_ratio = ratio;
		StepFacts f;
		f.occ_cells = 128u * 128u * 128u * 3u;
		// (the defaults of the inputs a pass does not sweep: a plain step of a call on one rank)
		opt.lookahead = ex.lookahead_inputs ? (la & 1) : true;
		f.use_delta = la & 4; f.dbg_hook = la & 8; f.loss_pending = la & 16; opt.dbg_loss_replay = la & 32;
		opt.scan_form = ot % 3;
		const uint32_t ob2 = ot / 3;
		opt.adam_overlap = ob2 & 1; f.x_on = ob2 & 2; f.x_overlap = ob2 & 4; f.train_canonical = ex.other_inputs ? (ob2 & 8) : true; f.prev_mcut = ob2 & 16;
		for (uint32_t fb = 0; fb < 32; ++fb) for (uint32_t lanes : {4u, 8u}) for (float cone : {0.f, 0.01f}) for (uint32_t left = 0; left < 4; ++left) {
			f.fixed_rays = fb & 1; f.dyn = fb & 2; f.profiling = fb & 4; f.balanced = fb & 8; f.force_full = fb & 16;
			f.lanes_per_ray = lanes; f.cone_angle = cone; f.left = left;
			f.next_in_call = ex.lookahead_inputs ? (la & 2) : left > 0;
			for (uint32_t step = step_lo; step <= step_hi; ++step) {
				f.step = step;
				f.canonical_step = f.dyn ? step / 3 + 1 : step;  // (dynamic scenes count the canonical steps apart)
				check_point(opt, sc, f);
			}
		}
	}
	}
	};
	std::vector<std::thread> threads;
	for (uint32_t k = 1; k < std::min(16u, std::max(1u, std::thread::hardware_concurrency())); ++k) threads.emplace_back(work);
	work();
	for (std::thread& t : threads) t.join();
}

// ---- c. the chunk-end rule and set()
bool ends_are(const std::vector<uint32_t>& v, std::initializer_list<uint32_t> want) { return v.size() == want.size() && std::equal(v.begin(), v.end(), want.begin()); }
void expect(bool ok, const char* what) { if (!ok) { ++g_failed; std::printf("FAIL %s\n", what); } }
void expect_throw(ChunkSchedule& sc, int mode, const uint32_t* e, uint32_t n, const char* msg) {
	const ChunkSchedule before = sc;
	try { sc.set(mode, e, n); } catch (const std::runtime_error& err) {
		expect(std::strcmp(err.what(), msg) == 0, msg);
		expect(sc.mode == before.mode && sc.ends == before.ends && sc.ends_cut == before.ends_cut && sc.auto_ends == before.auto_ends, "a rejected set() changes nothing");
		return;
	}
	expect(false, msg);
}
void chunk_rule() {
	NeusOptions opt;
	expect(opt.chunk_scale == 2.f && opt.chunk_rounds == 2, "default chunk_scale / chunk_rounds");
	{
		ChunkSchedule sc(opt);
		expect(sc.mode == 1 && ends_are(sc.ends, {32, 64, 96}) && sc.ends_cut.empty() && sc.auto_ends && sc.keep_ratio == 1.f && !sc.progressive(), "the default schedule");
		sc.on_readback(0, 1000, 1000, 1);
		expect(ends_are(sc.ends, {24, 48}) && ends_are(sc.ends_cut, {24}) && sc.keep_ratio == 0.f && sc.progressive(), "(0, 1000)");
		sc.on_readback(39000, 1000, 78000, 1);
		expect(ends_are(sc.ends, {32, 64}) && ends_are(sc.ends_cut, {64}) && sc.keep_ratio == 0.5f, "(39000, 1000)");
		sc.on_readback(117000, 1000, 117000, 1);
		expect(ends_are(sc.ends, {72, 144}) && ends_are(sc.ends_cut, {144}) && sc.keep_ratio == 1.f && !sc.progressive(), "(117000, 1000)");
		expect(&sc.ends_for(false) == &sc.ends && &sc.ends_for(true) == &sc.ends_cut, "ends_for");
		sc.on_readback(400000, 1000, 0, 1);
		expect(ends_are(sc.ends, {128, 256}) && ends_are(sc.ends_cut, {256}) && sc.keep_ratio == 1.f, "(400000, 1000)");
		sc.on_readback(39000, 0, 1000, 1);
		expect(ends_are(sc.ends, {128, 256}) && ends_are(sc.ends_cut, {256}), "no rays with samples: the ends stay");
		// two ranks: the keep ratio from this rank's share, the ends from the global counts
		sc.on_readback(78000, 2000, 78000, 2);
		expect(ends_are(sc.ends, {32, 64}) && ends_are(sc.ends_cut, {64}) && sc.keep_ratio == 0.5f, "(78000, 2000) at world 2");
	}
	{
		NeusOptions o3;
		o3.chunk_rounds = 3;
		ChunkSchedule sc(o3);
		sc.on_readback(117000, 1000, 117000, 1);
		expect(ends_are(sc.ends, {72, 144}) && ends_are(sc.ends_cut, {144, 288}), "(117000, 1000), three rounds");
	}
	{
		ChunkSchedule sc(opt);
		sc.on_readback(117000, 1000, 117000, 1);
		const uint32_t e[3] = {16, 48, 112};
		sc.set(2, e, 3);
		expect(sc.mode == 2 && ends_are(sc.ends, {16, 48, 112}) && sc.ends_cut.empty() && !sc.auto_ends && sc.progressive(), "explicit ends");
		expect(&sc.ends_for(true) == &sc.ends, "ends_for without cut ends");
		sc.on_readback(39000, 1000, 78000, 1);
		expect(ends_are(sc.ends, {16, 48, 112}) && sc.ends_cut.empty() && sc.keep_ratio == 0.5f, "explicit ends stay on a readback");
		sc.set(0, nullptr, 0);
		expect(sc.mode == 0 && ends_are(sc.ends, {16, 48, 112}) && !sc.auto_ends && !sc.progressive(), "a mode alone");
		uint32_t inc[15];
		for (uint32_t k = 0; k < 15; ++k) inc[k] = k + 1;
		expect_throw(sc, 3, e, 3, "progressive inference mode must be 0 (off), 1 (auto) or 2 (always)");
		expect_throw(sc, -1, nullptr, 0, "progressive inference mode must be 0 (off), 1 (auto) or 2 (always)");
		expect_throw(sc, 1, inc, 15, "at most 14 chunk ends");
		const uint32_t zero[2] = {0, 4}, flat[3] = {4, 8, 8}, down[2] = {8, 4};
		expect_throw(sc, 1, zero, 2, "chunk ends must increase from >= 1");
		expect_throw(sc, 1, flat, 3, "chunk ends must increase from >= 1");
		expect_throw(sc, 1, down, 2, "chunk ends must increase from >= 1");
		sc.set(1, inc, 14);
		expect(sc.mode == 1 && sc.ends.size() == 14, "14 ends");
	}
	{
		NeusOptions oe;
		oe.chunk_ends = {32, 80};
		ChunkSchedule sc(oe);
		sc.on_readback(117000, 1000, 117000, 1);
		expect(ends_are(sc.ends, {32, 80}) && sc.ends_cut.empty() && !sc.auto_ends, "ends from the options are explicit");
	}
}

}  // namespace

int main() {
	chunk_rule();
	sweep(0, 527, Extra{false, false});
	sweep(0, 40, Extra{true, false});
	sweep(250, 290, Extra{true, false});
	sweep(254, 274, Extra{false, true});
	if (g_failed) { std::printf("%d checks failed\n", g_failed.load()); return 1; }
	std::printf("ok\n");
	return 0;
}
