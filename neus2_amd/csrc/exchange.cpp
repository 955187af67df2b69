// neus::Exchange (exchange.h): the three transports of the data-parallel exchange, and the part of the C-ABI
// (include/neus2_hip.h) that makes an RCCL unique id or a group and takes no testbed.
#include "exchange.h"
#include "hostgroup.h"
#include "localgroup.h"

#include <rccl/rccl.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

#define NCCL_CHECK(x)                                                                                  \
	do {                                                                                               \
		ncclResult_t r_ = (x);                                                                         \
		if (r_ != ncclSuccess) throw std::runtime_error(std::string(#x) + " failed: " + ncclGetErrorString(r_)); \
	} while (0)

namespace neus {

void comm_destroy(ncclComm* c) { (void)ncclCommDestroy(c); }

namespace {

// The in-process group's all-reduce of n elements of T on the device, in place, on `s` (host-synchronous)
template <class T> void local_allreduce(NeusLocalGroup& g, uint32_t rank, T* dev, size_t n, NeusLocalGroup::Op op, hipStream_t s) {
	void* mine = g.stage_for(rank, n * sizeof(T));
	HIP_CHECK(hipMemcpyAsync(mine, dev, n * sizeof(T), hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipStreamSynchronize(s));
	std::vector<T> out(n);
	g.allreduce_staged(out.data(), n, op);
	HIP_CHECK(hipMemcpyAsync(dev, out.data(), n * sizeof(T), hipMemcpyHostToDevice, s));
	HIP_CHECK(hipStreamSynchronize(s));
}

} // namespace

// ------------------------------------------------------------ attach
void Exchange::attach_rccl(int device, int rank, int world, const uint8_t* uid, uint32_t flags) {
	if (world < 1 || rank < 0 || rank >= world) throw std::runtime_error("invalid rank/world");
	// refuses any of the three; sets the device; zeroes the counters; clears the setting check
	if (comm_ || group_ || hgroup_) throw std::runtime_error("init_data_parallel: the testbed already has a communicator");
	HIP_CHECK(hipSetDevice(device));
	rank_ = (uint32_t)rank; world_ = (uint32_t)world;
	force_ = (flags & NEUS_DP_FORCE_COLLECTIVES) != 0;
	verified_ = false;
	calls_ = bytes_ = bytes_step_ = 0;
	if (world > 1 || force_) {
		if (!uid) throw std::runtime_error("init_data_parallel: no unique id");
		ncclUniqueId id;
		std::memcpy(&id, uid, 128);
		ncclComm_t c = nullptr;
		NCCL_CHECK(ncclCommInitRank(&c, world, id, rank));
		comm_.reset(c);
	}
}
void Exchange::attach_host(int device, NeusHostGroup* g) {
	if (!g) throw std::runtime_error("invalid host group");
	// refuses any of the three; sets the device; zeroes the counters; clears the setting check
	if (comm_ || group_ || hgroup_) throw std::runtime_error("init_host_group: the testbed already has a communicator");
	HIP_CHECK(hipSetDevice(device));
	hgroup_ = g; rank_ = (uint32_t)g->rank; world_ = (uint32_t)g->world;
	calls_ = bytes_ = bytes_step_ = 0;
	verified_ = false;
}
void Exchange::attach_local(NeusLocalGroup* g, int rank) {
	if (!g || rank < 0 || (uint32_t)rank >= g->world) throw std::runtime_error("invalid local group / rank");
	// refuses an RCCL communicator only; leaves the device and the counters; clears the setting check
	if (comm_) throw std::runtime_error("testbed already has an RCCL communicator");
	group_ = g; rank_ = (uint32_t)rank; world_ = g->world;
	verified_ = false;
}
void Exchange::info(NeusDataParallelInfo* o) const {
	o->rank = rank_; o->world = world_;
	o->has_communicator = comm_ ? 1u : 0u; o->local_group = group_ ? 1u : 0u; o->host_group = hgroup_ ? 1u : 0u;
	o->collective_calls = calls_; o->allreduce_bytes = bytes_; o->last_step_allreduce_bytes = bytes_step_;
}
void Exchange::set_overlap(bool on) {
	HIP_CHECK(hipStreamSynchronize(step_));
	overlap_ = on;
	verified_ = false;
}

// ------------------------------------------------------------ the exchange stream
hipStream_t Exchange::gated() {
	if (!comm_ && !hgroup_) return step_;
	if (!comm_stream_) {
		comm_stream_ = main_prio_ ? make_stream(hipStreamNonBlocking, main_prio_) : make_stream(hipStreamNonBlocking);
		ev_xdone_ = make_event(hipEventDisableTiming);
	}
	Event& e = ev_x_[ev_x_n_++ % 16];
	ensure_event(e, hipEventDisableTiming);
	HIP_CHECK(hipEventRecord(e.get(), step_));
	HIP_CHECK(hipStreamWaitEvent(comm_stream_.get(), e.get(), 0));
	pending_ = true;
	return comm_stream_.get();
}
void Exchange::join() {
	if (!pending_) return;
	HIP_CHECK(hipEventRecord(ev_xdone_.get(), comm_stream_.get()));
	HIP_CHECK(hipStreamWaitEvent(step_, ev_xdone_.get(), 0));
	pending_ = false;
}

// ------------------------------------------------------------ collectives
void Exchange::begin() { if (comm_) NCCL_CHECK(ncclGroupStart()); }
void Exchange::end() { if (comm_) NCCL_CHECK(ncclGroupEnd()); }
bool Exchange::count(size_t n) {
	if (!on() || n == 0) return false;
	++calls_; bytes_ += n * 4; bytes_step_ += n * 4;
	return true;
}
void Exchange::allreduce_f32(float* p, size_t n, bool max_op, hipStream_t on) {
	if (!count(n)) return;
	if (comm_) NCCL_CHECK(ncclAllReduce(p, p, n, ncclFloat32, max_op ? ncclMax : ncclSum, comm_.get(), on ? on : step_));
	else if (hgroup_) host_allreduce(p, n * 4, NeusHostGroup::F32, max_op ? NeusHostGroup::MAX : NeusHostGroup::SUM, on);
	else if (group_) local_allreduce<float>(*group_, rank_, p, n, max_op ? NeusLocalGroup::MAX : NeusLocalGroup::SUM, step_);
	else throw std::runtime_error("data parallel: no communicator");
}
void Exchange::allreduce_u32(uint32_t* p, size_t n, hipStream_t on) {
	if (!count(n)) return;
	if (comm_) NCCL_CHECK(ncclAllReduce(p, p, n, ncclUint32, ncclSum, comm_.get(), on ? on : step_));
	else if (hgroup_) host_allreduce(p, n * 4, NeusHostGroup::U32, NeusHostGroup::SUM, on);
	else if (group_) local_allreduce<uint32_t>(*group_, rank_, p, n, NeusLocalGroup::SUM, step_);
	else throw std::runtime_error("data parallel: no communicator");
}
// A host-group collective on the exchange stream: device -> pinned stage, the socket exchange in a host function, stage ->
// device. Issued from the step's stream (on == nullptr / the step's stream), it is gated after the work queued there and
// the step's stream waits for it; issued on the exchange stream (the overlapped exchange), the stream order is the gate.
void Exchange::host_allreduce(void* dev, size_t bytes, uint32_t type, uint32_t op, hipStream_t on) {
	const bool own = !(on && on == comm_stream_.get());
	hipStream_t cs = own ? gated() : on;
	if (bytes > hg_stage_bytes_) {  // grow: the queued collectives still read the old stage
		if (comm_stream_) HIP_CHECK(hipStreamSynchronize(comm_stream_.get()));
		hg_stage_.reset();  // (freed before the larger one is allocated)
		hg_stage_bytes_ = 0;
		hg_stage_ = make_pinned<uint8_t>(std::max(bytes, (size_t)1 << 20));
		hg_stage_bytes_ = std::max(bytes, (size_t)1 << 20);
	}
	HIP_CHECK(hipMemcpyAsync(hg_stage_.get(), dev, bytes, hipMemcpyDeviceToHost, cs));
	auto c = std::make_unique<HostCollCall>(HostCollCall{hgroup_, hg_stage_.get(), bytes, type, op});
	HIP_CHECK(hipLaunchHostFunc(cs, [](void* a) {
		std::unique_ptr<HostCollCall> c((HostCollCall*)a);
		c->g->allreduce_host(c->host, c->bytes, c->type, c->op);
	}, c.get()));
	(void)c.release();  // the queued host function owns it from here
	HIP_CHECK(hipMemcpyAsync(dev, hg_stage_.get(), bytes, hipMemcpyHostToDevice, cs));
	if (own) join();
}
void Exchange::check() { if (hgroup_) hgroup_->check(); }
void Exchange::verify_uniform(uint32_t* scratch) {
	if (!unverified()) return;
	const uint32_t v[2] = {overlap_ ? 1u : 0u, 1u};
	HIP_CHECK(hipMemcpyAsync(scratch, v, 8, hipMemcpyHostToDevice, step_));
	allreduce_u32(scratch, 2);
	uint32_t h[2] = {0, 0};
	HIP_CHECK(hipMemcpyAsync(h, scratch, 8, hipMemcpyDeviceToHost, step_));
	HIP_CHECK(hipStreamSynchronize(step_));
	check();
	if (h[1] != world_) throw std::runtime_error("data parallel: the exchange-setting check saw " + std::to_string(h[1]) + " of " + std::to_string(world_) + " ranks");
	if (h[0] != 0 && h[0] != world_)
		throw std::runtime_error("data parallel: the exchange overlap is on for " + std::to_string(h[0]) + " of " + std::to_string(world_) +
		                         " ranks (neus_testbed_set_exchange_overlap / NEUS_EXCHANGE_OVERLAP must be the same on every rank)");
	verified_ = true;
}

// ------------------------------------------------------------ exchange timing
void Exchange::set_timing(bool on) {
	collect_all();
	xt_on_ = on;
	xt_exposed_ms_ = xt_span_ms_ = 0.0; xt_steps_ = 0;
}
Event* Exchange::timing_slot() {
	if (!on() || !xt_on_) return nullptr;
	if (xt_n_ == XT_RING) collect_one();
	Event* e = xt_ev_[(xt_head_ + xt_n_) % XT_RING];
	for (int k = 0; k < 3; ++k) ensure_event(e[k]);
	++xt_n_;
	return e;
}
void Exchange::collect_one() {
	Event* e = xt_ev_[xt_head_];
	HIP_CHECK(hipEventSynchronize(e[2].get()));
	HIP_CHECK(hipEventSynchronize(e[1].get()));
	float exposed = 0.f, span = 0.f;
	HIP_CHECK(hipEventElapsedTime(&exposed, e[1].get(), e[2].get()));
	HIP_CHECK(hipEventElapsedTime(&span, e[0].get(), e[2].get()));
	xt_exposed_ms_ += std::max(0.f, exposed);
	xt_span_ms_ += span;
	++xt_steps_;
	xt_head_ = (xt_head_ + 1) % XT_RING;
	--xt_n_;
}
void Exchange::timing(double* exposed_ms_total, double* span_ms_total, uint64_t* steps) {
	collect_all();
	if (exposed_ms_total) *exposed_ms_total = xt_exposed_ms_;
	if (span_ms_total) *span_ms_total = xt_span_ms_;
	if (steps) *steps = xt_steps_;
}

} // namespace neus

using namespace neus;

// ------------------------------------------------------------ C-ABI: the unique id and the groups (no testbed)
int neus_nccl_unique_id(uint8_t* out) {
	return guard([&] {
		ncclUniqueId id;
		NCCL_CHECK(ncclGetUniqueId(&id));
		static_assert(sizeof(id) == 128, "ncclUniqueId size");
		std::memcpy(out, &id, 128);
	});
}

int neus_local_group_create(int world, NeusLocalGroup** out) {
	return guard([&] {
		if (world < 1 || world > 64) throw std::runtime_error("local group: world must be 1..64");
		*out = new NeusLocalGroup((uint32_t)world);
	});
}
int neus_local_group_destroy(NeusLocalGroup* g) { return guard([&] { delete g; }); }

int neus_host_group_create(int rank, int world, const char* host, int port, uint64_t job_token, NeusHostGroup** out) {
	return guard([&] {
		if (world < 1 || world > 64 || rank < 0 || rank >= world) throw std::runtime_error("host group: world must be 1..64, 0 <= rank < world");
		if (port <= 0 || port > 65535) throw std::runtime_error("host group: invalid port");
		*out = new NeusHostGroup(rank, world, host ? host : "127.0.0.1", port, job_token);
	});
}
int neus_host_group_destroy(NeusHostGroup* g) { return guard([&] { delete g; }); }
int neus_debug_host_group_allreduce(NeusHostGroup* g, void* host, uint64_t n, int type, int op) {
	return guard([&] {
		if (!g) throw std::runtime_error("invalid host group");
		g->allreduce_host(host, (size_t)n * 4, type ? NeusHostGroup::U32 : NeusHostGroup::F32, op ? NeusHostGroup::MAX : NeusHostGroup::SUM);
		g->check();
	});
}
