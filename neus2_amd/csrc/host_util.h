// Host helpers shared by the host units (testbed.cpp, operators.cpp): the HIP error check, the owning device buffers and
// the C-ABI's exception guard. What they rest on (the allocation debug state, the thread's last error) has its one
// definition in testbed.cpp.
#pragma once
#include "kernels.h"

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

inline uint32_t next_multiple(uint32_t v, uint32_t m) { return (v + m - 1) / m * m; }

// The C-ABI's guard: an entry point returns 0, or 1 with the message kept for neus_last_error on the calling thread
void set_last_error(const char* what);
template <class F> int guard(F&& f) {
	try { f(); return 0; }
	catch (const std::exception& e) { set_last_error(e.what()); return 1; }
	catch (...) { set_last_error("unknown error"); return 1; }
}

} // namespace neus
