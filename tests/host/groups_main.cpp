// Stand-alone check of neus2_amd/csrc/localgroup.h (tests/test_local_group.py builds it with the thread sanitizer and
// with the address and undefined-behaviour sanitizers, and runs both): the in-process group driven by one thread per
// rank, as the testbeds of a group are. No HIP and no library: the header includes none.
//   * worlds 1, 2 and 3, 50 collectives back to back on one group (f32 sums of 1, 3 and 1000 elements, a u32 sum, an f32
//     max, in turn): every rank's result is bitwise the rank-order loop written out below (v0, + v1, + v2: one rounding per
//     rank), on values spanning seven decades so that another order of addition would show;
//   * a rank that misses a collective: the caller's barrier times out (a group built with a 300 ms wait), its arrival is
//     withdrawn, and the group is poisoned: the next collective fails on every rank without waiting.
// Exit status: the number of failed checks.
#include "localgroup.h"

#include <cstdio>
#include <cstring>
#include <string>
#include <thread>

#if defined(__SANITIZE_THREAD__)
// The thread sanitizer's runtime of GCC 11 intercepts pthread_cond_wait and pthread_cond_timedwait but not
// pthread_cond_clockwait, which std::condition_variable::wait_for calls: it never sees that wait release the mutex and
// reports the next rank's lock as a double lock, and every barrier as a race. This build alone routes the call to the
// intercepted wait, the steady clock's deadline restated on the realtime clock; the header under test is unchanged.
#include <pthread.h>
#include <time.h>
extern "C" int pthread_cond_clockwait(pthread_cond_t* cond, pthread_mutex_t* mutex, clockid_t clock, const struct timespec* abstime) {
	struct timespec on_clock, real;
	clock_gettime(clock, &on_clock);
	clock_gettime(CLOCK_REALTIME, &real);
	real.tv_sec += abstime->tv_sec - on_clock.tv_sec;
	real.tv_nsec += abstime->tv_nsec - on_clock.tv_nsec;
	while (real.tv_nsec < 0) { real.tv_nsec += 1000000000L; --real.tv_sec; }
	while (real.tv_nsec >= 1000000000L) { real.tv_nsec -= 1000000000L; ++real.tv_sec; }
	return pthread_cond_timedwait(cond, mutex, &real);
}
#endif

namespace {

int g_failed = 0;
std::mutex g_print;
void fail(const std::string& what) {
	std::lock_guard<std::mutex> lk(g_print);
	std::printf("FAIL %s\n", what.c_str());
	++g_failed;
}

uint32_t mix(uint32_t rank, uint32_t it, uint32_t k) {
	uint32_t h = rank * 0x9e3779b9u + it * 0x85ebca6bu + k * 0xc2b2ae35u + 0x27d4eb2fu;
	h ^= h >> 15; h *= 0x2c1b3c6du; h ^= h >> 12; h *= 0x297a2d39u; h ^= h >> 15;
	return h;
}
// rank's element k of collective `it`: a signed three-digit mantissa times 10^-3 .. 10^3
float f32_value(uint32_t rank, uint32_t it, uint32_t k) {
	static const float decade[7] = {1e-3f, 1e-2f, 1e-1f, 1.f, 1e1f, 1e2f, 1e3f};
	const uint32_t h = mix(rank, it, k);
	return (float)((int)(h % 2001u) - 1000) * 1.001f * decade[(h >> 11) % 7u];
}
uint32_t u32_value(uint32_t rank, uint32_t it, uint32_t k) { return mix(rank, it, k) >> 3; }

struct Kind { bool is_float; NeusLocalGroup::Op op; size_t n; const char* name; };
const Kind KINDS[5] = {{true, NeusLocalGroup::SUM, 1, "f32 sum n=1"}, {true, NeusLocalGroup::SUM, 3, "f32 sum n=3"},
                       {true, NeusLocalGroup::SUM, 1000, "f32 sum n=1000"}, {false, NeusLocalGroup::SUM, 257, "u32 sum"},
                       {true, NeusLocalGroup::MAX, 1000, "f32 max"}};

// one rank's collective `it` of kind `kd`: stage, all-reduce, compare with the sequential rank-order reference
template <class T, class V> void one_collective(NeusLocalGroup& g, uint32_t rank, uint32_t it, const Kind& kd, V value) {
	T* mine = (T*)g.stage_for(rank, kd.n * sizeof(T));
	for (size_t k = 0; k < kd.n; ++k) mine[k] = value(rank, it, (uint32_t)k);
	std::vector<T> out(kd.n), ref(kd.n);
	g.allreduce_staged(out.data(), kd.n, kd.op);
	for (size_t k = 0; k < kd.n; ++k) {
		T acc = value(0u, it, (uint32_t)k);
		for (uint32_t r = 1; r < g.world; ++r) {
			const T v = value(r, it, (uint32_t)k);
			if (kd.op == NeusLocalGroup::SUM) acc = (T)(acc + v);
			else acc = acc < v ? v : acc;
		}
		ref[k] = acc;
	}
	if (std::memcmp(out.data(), ref.data(), kd.n * sizeof(T)) != 0)
		fail(std::string(kd.name) + ": world " + std::to_string(g.world) + " rank " + std::to_string(rank) + " collective " + std::to_string(it) +
		     " differs from the rank-order reference");
}

void sums(uint32_t world) {
	NeusLocalGroup g(world);
	std::vector<std::thread> ranks;
	for (uint32_t rank = 0; rank < world; ++rank)
		ranks.emplace_back([&g, rank] {
			try {
				for (uint32_t it = 0; it < 50; ++it) {
					const Kind& kd = KINDS[it % 5];
					if (kd.is_float) one_collective<float>(g, rank, it, kd, f32_value);
					else one_collective<uint32_t>(g, rank, it, kd, u32_value);
				}
			} catch (const std::exception& e) {
				fail("world " + std::to_string(g.world) + " rank " + std::to_string(rank) + " threw: " + e.what());
			}
		});
	for (auto& t : ranks) t.join();
	if (g.arrived != 0 || g.generation != 100 || g.failed) fail("world " + std::to_string(world) + ": the barrier state after 50 collectives");
}

// what one rank's collective on g threw ("" when it returned), and how long the call took
std::string thrown_by(NeusLocalGroup& g, uint32_t rank, std::chrono::milliseconds* took) {
	const auto t0 = std::chrono::steady_clock::now();
	std::string what;
	try {
		float* mine = (float*)g.stage_for(rank, sizeof(float));
		mine[0] = 1.f;
		float out = 0.f;
		g.allreduce_staged(&out, 1, NeusLocalGroup::SUM);
	} catch (const std::exception& e) {
		what = e.what();
	}
	*took = std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - t0);
	return what;
}

void timeout_and_poison() {
	const std::chrono::milliseconds wait(300);
	NeusLocalGroup g(2, wait);
	std::chrono::milliseconds took[2] = {};
	std::string what[2];
	std::thread lone([&] { what[0] = thrown_by(g, 0, &took[0]); });  // rank 1 never calls
	lone.join();
	if (what[0] != "local group: barrier timeout (a rank did not reach the collective)") fail("lone rank: threw '" + what[0] + "'");
	if (took[0] + std::chrono::milliseconds(1) < wait) fail(  // (took is rounded down to the millisecond)
		"lone rank: gave up after " + std::to_string(took[0].count()) + " ms, before the wait ran out");
	if (g.arrived != 0) fail("lone rank: its arrival was not withdrawn (arrived = " + std::to_string(g.arrived) + ")");
	if (!g.failed) fail("lone rank: the group is not marked failed");
	std::thread r0([&] { what[0] = thrown_by(g, 0, &took[0]); }), r1([&] { what[1] = thrown_by(g, 1, &took[1]); });
	r0.join(); r1.join();
	for (int r = 0; r < 2; ++r) {
		if (what[r] != "local group: a previous collective failed (the group is poisoned)") fail("poisoned group, rank " + std::to_string(r) + ": threw '" + what[r] + "'");
		if (took[r] >= wait) fail("poisoned group, rank " + std::to_string(r) + ": waited " + std::to_string(took[r].count()) + " ms");
	}
	if (g.arrived != 0) fail("poisoned group: arrived = " + std::to_string(g.arrived));
}

} // namespace

int main() {
	for (uint32_t world = 1; world <= 3; ++world) sums(world);
	timeout_and_poison();
	if (g_failed) std::printf("%d checks failed\n", g_failed);
	else std::printf("ok\n");
	return g_failed;
}
