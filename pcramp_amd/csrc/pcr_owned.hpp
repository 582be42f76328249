// The owners of a handle's HIP resources: device memory, host-mapped pinned memory, events and streams.  Each frees what it
// holds when it is destroyed, so a member of pcr_ctx / SeqSet or a local needs no line anywhere else to be given back; the
// allocating and freeing HIP entry points are called here and nowhere else in the library.  Nothing may be in flight on a
// resource when its owner dies: the caller synchronises first (pcr_destroy: synchronise, then delete).  No owner may have static
// or thread storage duration (the HIP runtime may be gone when such destructors run).
//
// Needs from the including file: the HIP runtime declarations, PCR_OK / PCR_ERR_DEVICE (include/pcramp_hip.h) and the
// thread's error string g_err.  tests/owned_check.cpp includes it over malloc-backed fakes.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <algorithm>
#include <atomic>
#include <string>
#include <utility>

namespace pcrown {

// what the owners of this process hold right now (pcr_live_resources): device bytes, mapped host bytes, events, owned streams
enum { LIVE_DEVICE_BYTES = 0, LIVE_MAPPED_BYTES = 1, LIVE_EVENTS = 2, LIVE_STREAMS = 3 };
inline std::atomic<uint64_t> g_live[4];

template<class T> struct DevBuf {
	T *p = nullptr; size_t cap = 0;
	uint64_t generation = 0;     // bumped by every (re)allocation: the contents are undefined afterwards
	bool finegrained = false;    // fine-grained device memory, which the CPU may store into (the lean staging ring)
	explicit DevBuf(bool fine = false) : finegrained(fine) {}
	DevBuf(DevBuf &&o) noexcept { *this = std::move(o); }            // (move-only: declaring the moves deletes the copies)
	DevBuf &operator=(DevBuf &&o) noexcept
	{
		if(this != &o){ release(); p = o.p; cap = o.cap; generation = o.generation; finegrained = o.finegrained; o.p = nullptr; o.cap = 0; }
		return *this;
	}
	~DevBuf() { release(); }
	int ensure(size_t n)
	{
		if(n <= cap) return PCR_OK;
		++generation;
		release();
		const size_t want = std::max<size_t>(n, 16);
		const hipError_t e = finegrained ? hipExtMallocWithFlags((void **)&p, want*sizeof(T), hipDeviceMallocFinegrained) : hipMalloc((void **)&p, want*sizeof(T));
		if(e != hipSuccess){ p = nullptr; g_err = std::string("hipMalloc: ") + hipGetErrorString(e); return PCR_ERR_DEVICE; }
		cap = want; g_live[LIVE_DEVICE_BYTES] += cap*sizeof(T);
		return PCR_OK;
	}
	// for lists that grow a little at a time (the irregular words after every batch of splits): a quarter of slack, so that a hipFree +
	// hipMalloc pair -- a device-wide wait each -- is not paid on every growth
	int ensure_slack(size_t n) { return (n <= cap) ? PCR_OK : ensure(n + n/4 + 1024); }
	void release() { if(p){ (void)hipFree(p); g_live[LIVE_DEVICE_BYTES] -= cap*sizeof(T); p = nullptr; cap = 0; } }
};

// Pinned host memory that the device reads and writes in place (mapped, coherent): the host address, the device's address
// of the same bytes, and the capacity in bytes.
template<class T> struct MappedBuf {
	T *host = nullptr, *dev = nullptr; size_t cap = 0;
	MappedBuf() = default;
	MappedBuf(const MappedBuf &) = delete; MappedBuf &operator=(const MappedBuf &) = delete;
	~MappedBuf() { release(); }
	// room for `bytes`; a buffer that has to grow is freed (the caller has made sure that nothing reads it any more) and
	// allocated again with max(bytes, at_least) bytes: the call site's growth factor and minimum size go into at_least
	int ensure(size_t bytes, size_t at_least = 0)
	{
		if(bytes <= cap) return PCR_OK;
		release();
		const size_t want = std::max(bytes, at_least);
		hipError_t e = hipHostMalloc((void **)&host, want, hipHostMallocMapped | hipHostMallocCoherent);
		if(e != hipSuccess) host = nullptr;
		else{
			cap = want; g_live[LIVE_MAPPED_BYTES] += cap;
			if((e = hipHostGetDevicePointer((void **)&dev, host, 0)) != hipSuccess) release();
		}
		if(e != hipSuccess){ g_err = std::string("mapped host allocation: ") + hipGetErrorString(e); return PCR_ERR_DEVICE; }
		return PCR_OK;
	}
	void release() { if(host){ (void)hipHostFree(host); g_live[LIVE_MAPPED_BYTES] -= cap; host = dev = nullptr; cap = 0; } }
};

struct Event {
	hipEvent_t e = nullptr;
	Event() = default;
	Event(Event &&o) noexcept : e(o.e) { o.e = nullptr; }              // (move-only)
	Event &operator=(Event &&o) noexcept { if(this != &o){ release(); e = o.e; o.e = nullptr; } return *this; }
	~Event() { release(); }
	operator hipEvent_t() const { return e; }
	hipError_t create(unsigned flags = hipEventDefault)
	{
		release();
		const hipError_t rc = hipEventCreateWithFlags(&e, flags);
		if(rc != hipSuccess) e = nullptr; else ++g_live[LIVE_EVENTS];
		return rc;
	}
	void release() { if(e){ (void)hipEventDestroy(e); --g_live[LIVE_EVENTS]; e = nullptr; } }
};

// A stream this object created, or the caller's, which it only borrows: release() destroys the first kind alone.
struct Stream {
	hipStream_t s = nullptr; bool owned = false;
	Stream() = default;
	Stream(const Stream &) = delete; Stream &operator=(const Stream &) = delete;
	~Stream() { release(); }
	operator hipStream_t() const { return s; }
	void borrow(hipStream_t theirs) { release(); s = theirs; }
	hipError_t create(unsigned flags = hipStreamDefault)
	{
		release();
		const hipError_t rc = hipStreamCreateWithFlags(&s, flags);
		if(rc != hipSuccess) s = nullptr; else{ owned = true; ++g_live[LIVE_STREAMS]; }
		return rc;
	}
	void release() { if(owned){ (void)hipStreamDestroy(s); --g_live[LIVE_STREAMS]; } s = nullptr; owned = false; }
};

} // namespace pcrown
