// The data-parallel exchange of one testbed: the transport (an RCCL communicator, the cross-process host
// group of hostgroup.h or the in-process group of localgroup.h), this rank's place in it, the exchange stream with the
// events that gate it behind the step's stream and join it back, the two all-reduces with their counters, the check
// that every rank runs the same exchange setting, and the exchange timing. The training step (testbed.cpp) decides when
// and what is exchanged and reaches all of it through this interface; exchange.cpp holds the transports and the group
// and unique-id entry points of the C-ABI that take no testbed.
#pragma once
#include "host_util.h"
#include "../../include/neus2_hip.h"

struct ncclComm;

namespace neus {

void comm_destroy(ncclComm* c);  // (ncclCommDestroy, without RCCL's header here)

class Exchange {
public:
	// Bound to the testbed's current stream (a reference: operators.cpp StreamSwap rewrites it) and to the priority of the
	// step's streams, which the exchange stream follows (0: created without one)
	Exchange(const hipStream_t& step_stream, const int& main_prio, bool overlap) : step_(step_stream), main_prio_(main_prio), overlap_(overlap) {}

	uint32_t rank() const { return rank_; }
	uint32_t world() const { return world_; }
	// whether the step issues its collectives: several ranks, or a forced one-rank communicator (tests)
	bool on() const { return world_ > 1 || force_; }
	// Overlapped gradient exchange: each finished gradient range is all-reduced as soon as its producer
	// finishes - the MLP blocks after the weight-gradient reduction, the grid levels group by group beside the scatter's
	// accumulation of the later groups - on the exchange stream (RCCL; one stream keeps every rank's collectives in one
	// order), which the step's stream joins before the optimizer. Off (NEUS_EXCHANGE_OVERLAP=0,
	// neus_testbed_set_exchange_overlap): one grouped exchange after the backward. Elementwise sums are the same either way
	// (bitwise with two ranks).
	bool overlap() const { return overlap_; }
	void set_overlap(bool on);  // (after the step's stream has drained; the setting is checked again at the next step)

	// The three transports. The attach paths differ in what they refuse and in what they reset, and the difference is
	// inherited, not designed: each states its row.
	//                                        RCCL           host group     local group
	//   refuses a testbed that already has   any of three   any of three   an RCCL communicator
	//   sets the device                      yes            yes            no
	//   zeroes the counters                  yes            yes            no
	//   clears the setting check             yes            yes            yes
	void attach_rccl(int device, int rank, int world, const uint8_t* uid, uint32_t flags);
	void attach_host(int device, NeusHostGroup* g);
	void attach_local(NeusLocalGroup* g, int rank);
	void info(NeusDataParallelInfo* o) const;

	// The exchange stream (created at the first gated use, with its join event) after the work queued so far on the
	// step's stream; without a communicator or a host group, the step's stream: the in-process group stages on the host
	hipStream_t gated();
	void join();  // the step's stream waits for every exchange issued on the exchange stream
	hipStream_t stream() const { return comm_stream_.get(); }  // (null until the first gated use)
	// The testbed's destructor spells out the order these go back to the runtime (the runtime is not neutral to it)
	void release_comm() { comm_.reset(); }
	void release_stream() { comm_stream_.reset(); }

	// In-place all-reduces of device memory, on `on` or the step's stream (RCCL), staged on the exchange stream (host group:
	// gated and joined here unless `on` is that stream already) or host-synchronous on the step's stream (local group);
	// begin / end bracket a group of them (one RCCL launch). Nothing without on() or elements.
	void begin();
	void end();
	void allreduce_f32(float* p, size_t n, bool max_op = false, hipStream_t on = nullptr);
	void allreduce_u32(uint32_t* p, size_t n, hipStream_t on = nullptr);
	void reset_step_bytes() { bytes_step_ = 0; }
	void check();  // raises what a host-group collective left behind (a host function cannot throw)
	// Every rank must run the same exchange (overlapped or grouped: they issue different collective sequences): at the first
	// step after an attach or a change of the setting, the sum of the setting over the ranks must be 0 or world.
	// `scratch`: two device words; host-synchronous
	bool unverified() const { return !verified_ && on(); }
	void verify_uniform(uint32_t* scratch);

	// Exchange timing (neus_testbed_set_exchange_timing): per step, an event on the step's stream where the backward is
	// done (the gradients' last use before the join) and one on the exchange's stream after its last collective. exposed =
	// max(0, done - backward done): what the join before Adam waits for; span = done - the loss's end (the counters'
	// exchange starts there). A ring of event sets collected lazily (the oldest has long completed when the ring wraps, the
	// host running at most 16 steps ahead), so timing runs inside timed regions without a per-step sync.
	void set_timing(bool on);
	// this step's [loss end (step stream), backward done (step stream), exchange done (exchange stream)], or null: off
	Event* timing_slot();
	void timing(double* exposed_ms_total, double* span_ms_total, uint64_t* steps);

private:
	void host_allreduce(void* dev, size_t bytes, uint32_t type, uint32_t op, hipStream_t on);
	bool count(size_t n);
	void collect_one();
	void collect_all() { while (xt_n_) collect_one(); }

	const hipStream_t& step_;
	const int& main_prio_;
	// RCCL communicator (production), an in-process group, or a cross-process host-staged group: every collective of the
	// last staged on the exchange stream through a pinned buffer
	Handle<ncclComm*, comm_destroy> comm_;
	NeusLocalGroup* group_ = nullptr;
	NeusHostGroup* hgroup_ = nullptr;
	Pinned<uint8_t> hg_stage_;
	size_t hg_stage_bytes_ = 0;
	uint32_t rank_ = 0, world_ = 1;
	bool verified_ = false;
	bool force_ = false;  // issue the collectives at world 1 too
	bool overlap_;
	Stream comm_stream_;
	Event ev_x_[16];
	uint32_t ev_x_n_ = 0;
	Event ev_xdone_;
	bool pending_ = false;
	uint64_t calls_ = 0, bytes_ = 0, bytes_step_ = 0;
	bool xt_on_ = false;
	static constexpr int XT_RING = 64;
	Event xt_ev_[XT_RING][3];
	int xt_head_ = 0, xt_n_ = 0;
	double xt_exposed_ms_ = 0.0, xt_span_ms_ = 0.0;
	uint64_t xt_steps_ = 0;
};

} // namespace neus
