// The one owning handle of the host units: a T that is null (T{}) or owned, handed to Destroy exactly once. Move-only;
// no HIP here, so the host-only test program (tests/host/handles_main.cpp) builds it with a counting destroyer.
#pragma once
#include <utility>

namespace neus {

template <class T, auto Destroy> struct Handle {
	Handle() = default;
	explicit Handle(T v) : v_(v) {}
	Handle(Handle&& o) noexcept : v_(o.release()) {}
	Handle& operator=(Handle&& o) noexcept {
		if (this != &o) reset(o.release());
		return *this;
	}
	Handle(const Handle&) = delete;
	Handle& operator=(const Handle&) = delete;
	~Handle() { reset(); }
	T get() const { return v_; }
	explicit operator bool() const { return v_ != T{}; }
	// the old value is destroyed first (its result ignored, as a destructor must), then v adopted
	void reset(T v = T{}) {
		if (v_ != T{}) (void)Destroy(v_);
		v_ = v;
	}
	T release() { return std::exchange(v_, T{}); }

private:
	T v_{};
};

} // namespace neus
