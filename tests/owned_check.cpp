// Stand-alone check of pcramp_amd/csrc/pcr_owned.hpp (no GPU, no HIP): built with a sanitizer and run by test_owned_host.py.
// The HIP entry points the header calls are malloc-backed fakes here that keep a ledger of every block, event and stream
// they handed out, and that can be told to fail the N-th allocation.  Exit status 0 and a last line "owned ok" when every
// check holds.
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <map>
#include <type_traits>
#include <string>
#include <vector>

#include "../include/pcramp_hip.h"             // PCR_OK, PCR_ERR_DEVICE

#define CHECK(cond) do{ if(!(cond)){ fprintf(stderr, "owned_check: %s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } }while(0)

// ---- the fakes
typedef int hipError_t;
enum { hipSuccess = 0, hipErrorOutOfMemory = 2 };
typedef struct FakeEvent *hipEvent_t;
typedef struct FakeStream *hipStream_t;
enum { hipDeviceMallocFinegrained = 1, hipHostMallocMapped = 2, hipHostMallocCoherent = 0x40000000, hipEventDefault = 0, hipEventDisableTiming = 2,
	hipStreamDefault = 0, hipStreamNonBlocking = 1 };

struct Ledger {
	std::map<void *, int> frees;              // every address ever handed out -> times it was given back
	std::map<void *, size_t> bytes;
	int n_alloc = 0, n_free = 0;
	void *give(size_t n) { void *p = malloc(n ? n : 1); CHECK(p); CHECK(!frees.count(p) || frees[p] == 1); frees[p] = 0; bytes[p] = n; ++n_alloc; return p; }
	void take(void *p) { CHECK(frees.count(p)); CHECK(frees[p] == 0); frees[p] = 1; ++n_free; free(p); }
	bool all_freed_once() const { for(const auto &kv : frees){ if(kv.second != 1) return false; } return true; }
};
static Ledger g_dev, g_fine, g_host, g_events, g_streams;
static int g_fail_in = 0;                      // > 0: the g_fail_in-th allocation from now fails
static int g_stream_destroys = 0;
static bool fail_now() { return g_fail_in > 0 && --g_fail_in == 0; }

static const char *hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : "out of memory (fake)"; }
static hipError_t hipMalloc(void **p, size_t n) { if(fail_now()){ *p = nullptr; return hipErrorOutOfMemory; } *p = g_dev.give(n); return hipSuccess; }
static hipError_t hipExtMallocWithFlags(void **p, size_t n, unsigned flags)
{
	CHECK(flags == hipDeviceMallocFinegrained);
	if(fail_now()){ *p = nullptr; return hipErrorOutOfMemory; }
	*p = g_fine.give(n); return hipSuccess;
}
static hipError_t hipFree(void *p) { if(g_fine.frees.count(p) && g_fine.frees[p] == 0) g_fine.take(p); else g_dev.take(p); return hipSuccess; }
static hipError_t hipHostMalloc(void **p, size_t n, unsigned flags)
{
	CHECK(flags == (unsigned)(hipHostMallocMapped | hipHostMallocCoherent));
	if(fail_now()){ *p = nullptr; return hipErrorOutOfMemory; }
	*p = g_host.give(n); return hipSuccess;
}
static bool g_fail_device_pointer = false;
static hipError_t hipHostGetDevicePointer(void **d, void *h, unsigned) { if(g_fail_device_pointer) return hipErrorOutOfMemory; *d = h; return hipSuccess; }
static hipError_t hipHostFree(void *p) { g_host.take(p); return hipSuccess; }
static hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) { if(fail_now()){ *e = nullptr; return hipErrorOutOfMemory; } *e = (hipEvent_t)g_events.give(8); return hipSuccess; }
static hipError_t hipEventDestroy(hipEvent_t e) { g_events.take(e); return hipSuccess; }
static hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned) { if(fail_now()){ *s = nullptr; return hipErrorOutOfMemory; } *s = (hipStream_t)g_streams.give(8); return hipSuccess; }
static hipError_t hipStreamDestroy(hipStream_t s) { ++g_stream_destroys; g_streams.take(s); return hipSuccess; }

static thread_local std::string g_err;

#include "../pcramp_amd/csrc/pcr_owned.hpp"

using pcrown::DevBuf; using pcrown::MappedBuf; using pcrown::Event; using pcrown::Stream;
static uint64_t live(int k) { return pcrown::g_live[k].load(); }

int main()
{
	{   // ensure: nothing below or at capacity, one free + one allocation above it, at least 16 elements
		DevBuf<uint32_t> b;
		CHECK(b.p == nullptr && b.cap == 0 && b.generation == 0);
		CHECK(b.ensure(0) == PCR_OK && g_dev.n_alloc == 0 && b.generation == 0);
		CHECK(b.ensure(5) == PCR_OK && b.cap == 16 && b.p && b.generation == 1 && g_dev.n_alloc == 1 && g_dev.n_free == 0);
		CHECK(g_dev.bytes[b.p] == 16*sizeof(uint32_t) && live(0) == 16*sizeof(uint32_t));
		CHECK(b.ensure(7) == PCR_OK && b.ensure(16) == PCR_OK && g_dev.n_alloc == 1 && g_dev.n_free == 0 && b.generation == 1);
		CHECK(b.ensure(100) == PCR_OK && b.cap == 100 && b.generation == 2 && g_dev.n_alloc == 2 && g_dev.n_free == 1);
		CHECK(live(0) == 100*sizeof(uint32_t));
		b.p[99] = 7;                             // (the sanitizer watches the block's bounds)
		// ensure_slack: a quarter plus 1024 when it has to grow, nothing otherwise
		CHECK(b.ensure_slack(100) == PCR_OK && b.cap == 100 && b.generation == 2);
		CHECK(b.ensure_slack(1000) == PCR_OK && b.cap == 1000 + 250 + 1024 && b.generation == 3 && g_dev.n_alloc == 3 && g_dev.n_free == 2);
		// a failed allocation: the old block is gone (free first, then allocate), the buffer is empty, the error is set
		g_fail_in = 1; g_err.clear();
		CHECK(b.ensure(5000) == PCR_ERR_DEVICE && b.p == nullptr && b.cap == 0 && b.generation == 4 && !g_err.empty());
		CHECK(g_dev.n_free == 3 && live(0) == 0);
		CHECK(b.ensure(20) == PCR_OK && b.cap == 20 && b.generation == 5);
		// release twice
		b.release(); b.release();
		CHECK(b.p == nullptr && b.cap == 0 && g_dev.n_free == 4 && live(0) == 0);
		CHECK(b.ensure(1) == PCR_OK);            // (freed by the destructor)
	}
	CHECK(g_dev.n_alloc == g_dev.n_free && live(0) == 0);
	{   // moves empty the source; the destination's old block is freed exactly once
		DevBuf<uint64_t> a, b;
		CHECK(a.ensure(32) == PCR_OK && b.ensure(64) == PCR_OK);
		uint64_t *const pa = a.p, *const pb = b.p;
		const int frees = g_dev.n_free;
		DevBuf<uint64_t> c(std::move(a));
		CHECK(a.p == nullptr && a.cap == 0 && c.p == pa && c.cap == 32 && c.generation == 1 && g_dev.n_free == frees);
		c = std::move(b);
		CHECK(b.p == nullptr && b.cap == 0 && c.p == pb && c.cap == 64 && g_dev.n_free == frees + 1 && g_dev.frees[pa] == 1);
		c = std::move(c);
		CHECK(c.p == pb && g_dev.n_free == frees + 1);
		CHECK(live(0) == 64*sizeof(uint64_t));
		static_assert(!std::is_copy_constructible<DevBuf<uint64_t> >::value && !std::is_copy_assignable<DevBuf<uint64_t> >::value, "move-only");
		std::vector<DevBuf<uint8_t> > v(3);
		for(size_t i = 0;i < v.size();++i) CHECK(v[i].ensure(100*(i + 1)) == PCR_OK);
		v.resize(40);                            // reallocates: moves
		CHECK(v[2].cap == 300 && live(0) == 64*sizeof(uint64_t) + 600);
	}
	CHECK(g_dev.n_alloc == g_dev.n_free && live(0) == 0);
	{   // fine-grained device memory is a flag of the same type
		DevBuf<uint8_t> f(true);
		CHECK(f.ensure(1 << 17) == PCR_OK && g_fine.n_alloc == 1 && f.cap == (1u << 17) && live(0) == (1u << 17));
		CHECK(f.ensure(1 << 18) == PCR_OK && g_fine.n_alloc == 2 && g_fine.n_free == 1);
		g_fail_in = 1;
		CHECK(f.ensure(1 << 19) == PCR_ERR_DEVICE && f.p == nullptr && f.cap == 0 && live(0) == 0);
	}
	CHECK(g_fine.n_alloc == 2 && g_fine.n_free == 2 && g_dev.n_alloc == g_dev.n_free);
	{   // host-mapped memory
		MappedBuf<uint8_t> m;
		CHECK(m.ensure(0) == PCR_OK && m.host == nullptr);
		CHECK(m.ensure(100, 1 << 16) == PCR_OK && m.cap == (1u << 16) && m.host && m.dev == m.host && live(1) == (1u << 16));
		uint8_t *const first = m.host;
		CHECK(m.ensure(1 << 16, 1 << 20) == PCR_OK && m.host == first && g_host.n_alloc == 1);
		CHECK(m.ensure((1 << 16) + 1, 2*((1 << 16) + 1)) == PCR_OK && m.cap == 2*((1u << 16) + 1) && g_host.n_alloc == 2 && g_host.n_free == 1);
		m.host[m.cap - 1] = 1;
		CHECK(m.ensure(1 << 20) == PCR_OK && m.cap == (1u << 20) && live(1) == (1u << 20));
		g_fail_in = 1; g_err.clear();
		CHECK(m.ensure(1 << 21) == PCR_ERR_DEVICE && m.host == nullptr && m.dev == nullptr && m.cap == 0 && live(1) == 0 && !g_err.empty());
		g_fail_device_pointer = true;            // the block is had but not its device address: given back
		CHECK(m.ensure(64) == PCR_ERR_DEVICE && m.host == nullptr && m.cap == 0 && live(1) == 0);
		g_fail_device_pointer = false;
		CHECK(m.ensure(64) == PCR_OK);
		static_assert(!std::is_copy_constructible<MappedBuf<uint8_t> >::value && !std::is_move_constructible<MappedBuf<uint8_t> >::value, "stays where it is");
		MappedBuf<uint8_t> o;
		CHECK(o.ensure(128) == PCR_OK && live(1) == 64 + 128);
		o.release(); o.release();
		CHECK(o.host == nullptr && o.cap == 0 && live(1) == 64);
	}
	CHECK(g_host.n_alloc == g_host.n_free);
	{   // events, and a vector of event pairs as the profiler keeps them
		Event e;
		CHECK(!e && e.create(hipEventDisableTiming) == hipSuccess && e && live(2) == 1);
		Event f(std::move(e));
		CHECK(!e && f && live(2) == 1);
		g_fail_in = 1;
		CHECK(e.create() != hipSuccess && !e && live(2) == 1);
		std::vector<std::pair<Event, Event> > pairs;
		for(int i = 0;i < 100;++i){
			Event a, b;
			CHECK(a.create() == hipSuccess && b.create() == hipSuccess);
			pairs.emplace_back(std::move(a), std::move(b));
			CHECK(!a && !b);
		}
		CHECK(live(2) == 201 && g_events.n_free == 0);
		pairs.clear();
		CHECK(live(2) == 1 && g_events.n_free == 200);
		f.release(); f.release();
		CHECK(live(2) == 0);
	}
	CHECK(g_events.n_alloc == g_events.n_free);
	{   // a borrowed stream is never destroyed, an owned one exactly once
		FakeStream *theirs = (FakeStream *)malloc(8);
		{
			Stream s;
			CHECK(!s);
			s.borrow(theirs);
			CHECK((hipStream_t)s == theirs && !s.owned && live(3) == 0);
			s.release(); s.release();
			s.borrow(theirs);
		}
		CHECK(g_stream_destroys == 0 && live(3) == 0);
		{
			Stream s;
			CHECK(s.create(hipStreamNonBlocking) == hipSuccess && s && s.owned && live(3) == 1);
		}
		CHECK(g_stream_destroys == 1 && live(3) == 0);
		{
			Stream s;
			g_fail_in = 1;
			CHECK(s.create() != hipSuccess && !s && !s.owned && live(3) == 0);
			CHECK(s.create() == hipSuccess);
			s.borrow(theirs);                    // gives its own stream up first
			CHECK(g_stream_destroys == 2 && live(3) == 0 && (hipStream_t)s == theirs);
		}
		CHECK(g_stream_destroys == 2);
		free(theirs);
	}
	for(int k = 0;k < 4;++k) CHECK(live(k) == 0);
	for(const Ledger *l : {&g_dev, &g_fine, &g_host, &g_events, &g_streams}) CHECK(l->n_alloc == l->n_free && l->all_freed_once());
	CHECK(g_fail_in == 0);
	printf("owned ok\n");
	return 0;
}
