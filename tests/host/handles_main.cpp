// Stand-alone check of neus2_amd/csrc/handle.h (tests/test_host_handles.py builds it with the address and
// undefined-behaviour sanitizers and runs it): Handle over an int with a destroyer that counts its calls and sums the
// values it was given. No HIP: the header includes none. Exit status: the number of failed checks.
#include "handle.h"

#include <cstdio>
#include <type_traits>
#include <utility>
#include <vector>

namespace {

int g_calls = 0;
long g_sum = 0;
int destroy(int v) { ++g_calls; g_sum += v; return 7; }  // (a result the handle must ignore, as hipEventDestroy's)
using H = neus::Handle<int, destroy>;

static_assert(!std::is_copy_constructible_v<H>, "Handle copies");
static_assert(!std::is_copy_assignable_v<H>, "Handle copy-assigns");
static_assert(std::is_nothrow_move_constructible_v<H>, "Handle's move may throw");
static_assert(std::is_nothrow_move_assignable_v<H>, "Handle's move assignment may throw");

int g_failed = 0;
// the destroyer ran `calls` times since the last check, over values summing to `sum`
void expect(const char* what, bool ok, int calls, long sum) {
	if (!ok || g_calls != calls || g_sum != sum) {
		std::printf("FAIL %s: ok=%d, %d destroys (sum %ld), expected %d (sum %ld)\n", what, ok ? 1 : 0, g_calls, g_sum, calls, sum);
		++g_failed;
	}
	g_calls = 0;
	g_sum = 0;
}

} // namespace

int main() {
	{ H h; expect("empty: is empty", !h && h.get() == 0, 0, 0); }
	expect("empty: destroys nothing", true, 0, 0);

	{ H h(5); expect("adopted: holds the value", bool(h) && h.get() == 5, 0, 0); }
	expect("adopted: destroyed once", true, 1, 5);

	{
		H a(6);
		H b(std::move(a));
		expect("move: source empty, target holds", !a && a.get() == 0 && b.get() == 6, 0, 0);
	}
	expect("move: one destroy in total", true, 1, 6);

	{
		H a(1), b(2);
		a = std::move(b);
		expect("move-assign: the old value destroyed first, once", a.get() == 2 && !b, 1, 1);
	}
	expect("move-assign: the new value destroyed once at the end", true, 1, 2);

	{
		H a(9);
		H& r = a;  // (through a reference: -Wself-move)
		a = std::move(r);
		expect("self-move-assign: keeps the value", a.get() == 9, 0, 0);
	}
	expect("self-move-assign: destroyed once", true, 1, 9);

	{
		H a(3);
		a.reset();
		a.reset();
		expect("reset twice: one destroy", !a, 1, 3);
		a.reset(4);
		a.reset(8);
		expect("reset(v): adopts, destroying the old value", a.get() == 8, 1, 4);
	}
	expect("reset: the last value destroyed once", true, 1, 8);

	{
		H a(11);
		const int v = a.release();
		expect("release: hands the value out", v == 11 && !a, 0, 0);
	}
	expect("release: destroys nothing", true, 0, 0);

	{
		H ev[2][11] = {};  // (the shape of the testbed's phase events)
		bool empty = true;
		for (auto& set : ev)
			for (auto& e : set) empty = empty && !e;
		expect("2-D array: all empty", empty, 0, 0);
	}
	expect("2-D array: destroys nothing", true, 0, 0);

	{
		std::vector<H> v;
		v.reserve(2);
		long sum = 0;
		for (int k = 1; k <= 100; ++k) { v.emplace_back(k); sum += k; }  // grown past its capacity several times
		bool held = v.size() == 100;
		for (int k = 0; k < 100; ++k) held = held && v[k].get() == k + 1;
		expect("vector: growth moves, destroying nothing", held, 0, 0);
		v.clear();
		expect("vector: each element destroyed once", true, 100, sum);
	}
	expect("vector: nothing left to destroy", true, 0, 0);

	if (g_failed) std::printf("%d checks failed\n", g_failed);
	else std::printf("ok\n");
	return g_failed;
}
