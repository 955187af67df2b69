// Host helpers shared by the host units (testbed.cpp, operators.cpp): the HIP error check, the owners of every HIP
// resource (device buffers; streams, events and pinned memory as handle.h Handles, with the functions that create them)
// and the C-ABI's exception guard. What they rest on (the allocation debug state, the thread's last error) has its one
// definition in testbed.cpp.
#pragma once
#include "kernels.h"
#include "handle.h"

#include <exception>
#include <stdexcept>
#include <string>

#define HIP_CHECK(x)                                                                                   \
	do {                                                                                               \
		hipError_t e_ = (x);                                                                           \
		if (e_ != hipSuccess) throw std::runtime_error(std::string(#x) + " failed: " + hipGetErrorString(e_)); \
	} while (0)

namespace neus {

// Debug (options.h NeusAllocDebug): the fill / the listing of the fresh device allocations (testbed.cpp)
void dbg_poison(void* p, size_t bytes);

template <class T> struct Dev {
	T* p = nullptr;
	size_t n = 0;
	Dev() = default;
	Dev(const Dev&) = delete;  // (a copy would free twice; ScanTemp inherits the deletion)
	Dev& operator=(const Dev&) = delete;
	void alloc(size_t k) {
		if (k <= n && p) return;
		release();
		if (k == 0) return;
		HIP_CHECK(hipMalloc((void**)&p, k * sizeof(T)));
		dbg_poison(p, k * sizeof(T));
		n = k;
	}
	void release() { if (p) (void)hipFree(p); p = nullptr; n = 0; }
	~Dev() { release(); }
};
// A scan temp buffer (scan_temp_bytes: look-back state + hipCUB scratch): its host-side launch tag (scan.hip) is dropped
// with the buffer
struct ScanTemp : Dev<uint8_t> {
	void alloc(size_t k) { if (k <= n && p) return; release(); Dev<uint8_t>::alloc(k); }
	void release() { if (p) scan_temp_release(p); Dev<uint8_t>::release(); }
	~ScanTemp() { release(); }
};

// Owned streams (drained, then destroyed), events and pinned host memory: created only here, each throwing as HIP_CHECK
inline void stream_drain_destroy(hipStream_t s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); }
template <class T> void pinned_free(T* p) { (void)hipHostFree((void*)p); }
using Stream = Handle<hipStream_t, stream_drain_destroy>;
using Event = Handle<hipEvent_t, hipEventDestroy>;
template <class T> using Pinned = Handle<T*, pinned_free<T>>;
inline Stream make_stream(unsigned flags) { hipStream_t s = nullptr; HIP_CHECK(hipStreamCreateWithFlags(&s, flags)); return Stream(s); }
inline Stream make_stream(unsigned flags, int priority) { hipStream_t s = nullptr; HIP_CHECK(hipStreamCreateWithPriority(&s, flags, priority)); return Stream(s); }
inline Event make_event(unsigned flags = hipEventDefault) { hipEvent_t e = nullptr; HIP_CHECK(hipEventCreateWithFlags(&e, flags)); return Event(e); }
inline void ensure_event(Event& e, unsigned flags = hipEventDefault) { if (!e) e = make_event(flags); }
template <class T> Pinned<T> make_pinned(size_t n, unsigned flags = hipHostMallocDefault) {
	void* p = nullptr;
	HIP_CHECK(hipHostMalloc(&p, n * sizeof(T), flags));
	return Pinned<T>((T*)p);
}

inline uint32_t next_multiple(uint32_t v, uint32_t m) { return (v + m - 1) / m * m; }

// The C-ABI's guard: an entry point returns 0, or 1 with the message kept for neus_last_error on the calling thread
void set_last_error(const char* what);
template <class F> int guard(F&& f) {
	try { f(); return 0; }
	catch (const std::exception& e) { set_last_error(e.what()); return 1; }
	catch (...) { set_last_error("unknown error"); return 1; }
}

} // namespace neus
