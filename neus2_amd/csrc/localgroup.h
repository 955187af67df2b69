// In-process data-parallel group (NeusLocalGroup, include/neus2_hip.h neus_local_group_create): `world` testbeds driven
// from `world` host threads exchange through host staging buffers (sum in rank order, max), with the same call sequence
// as the RCCL path. It lets the data-parallel step (sharded occupancy update, gradient / counter / loss / DeltaNetwork
// all-reduces) run with several ranks on one device, e.g. in tests; production ranks use RCCL
// (neus_testbed_init_data_parallel).
//
// Host only: no HIP here, so the host-only test program (tests/host/groups_main.cpp) builds it under the thread and
// address sanitizers. The device side of a collective (exchange.cpp) copies its operand into stage_for(rank), calls
// allreduce_staged and copies the result back.
#pragma once

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstddef>
#include <cstdint>
#include <mutex>
#include <stdexcept>
#include <vector>

namespace neus {

// One step of the rank-order reduction both host groups compute (out = v0, then out = out + v1, ...: one rounding per
// rank; max is exact and keeps `out` when either side is NaN)
template <class T> void reduce_into(T* out, const T* v, size_t n, bool max_op) {
	if (!max_op) for (size_t k = 0; k < n; ++k) out[k] = (T)(out[k] + v[k]);
	else for (size_t k = 0; k < n; ++k) out[k] = out[k] < v[k] ? v[k] : out[k];
}

} // namespace neus

struct NeusLocalGroup {
	enum Op { SUM, MAX };
	const uint32_t world;
	const std::chrono::milliseconds wait;  // how long a rank waits at a barrier for the others
	std::mutex mu;
	std::condition_variable cv;
	uint32_t arrived = 0, generation = 0;
	bool failed = false;  // a rank timed out: every later collective fails fast instead of pairing the wrong ranks
	std::vector<std::vector<uint8_t>> stage;
	explicit NeusLocalGroup(uint32_t w, std::chrono::milliseconds wait_ = std::chrono::seconds(120)) : world(w), wait(wait_), stage(w) {}
	void barrier() {
		std::unique_lock<std::mutex> lk(mu);
		if (failed) throw std::runtime_error("local group: a previous collective failed (the group is poisoned)");
		const uint32_t gen = generation;
		if (++arrived == world) { arrived = 0; ++generation; cv.notify_all(); return; }
		if (!cv.wait_for(lk, wait, [&] { return generation != gen || failed; }) || failed) {
			if (generation == gen) --arrived;  // this rank's arrival is withdrawn
			failed = true;
			cv.notify_all();
			throw std::runtime_error("local group: barrier timeout (a rank did not reach the collective)");
		}
	}
	// this rank's operand of the next collective: `bytes` of host memory the caller fills before allreduce_staged
	void* stage_for(uint32_t rank, size_t bytes) {
		stage[rank].resize(bytes);
		return stage[rank].data();
	}
	// every rank's staged n elements of T reduced into out, in rank order; called by every rank
	template <class T> void allreduce_staged(T* out, size_t n, Op op) {
		barrier();
		for (uint32_t r = 0; r < world; ++r) {
			const T* v = (const T*)stage[r].data();
			if (r == 0) std::copy(v, v + n, out);
			else neus::reduce_into(out, v, n, op == MAX);
		}
		barrier();  // every rank has read every stage before the next collective overwrites one
	}
};
