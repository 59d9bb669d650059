// hip_res.h -- the one place the library's host code obtains a HIP resource: device memory, page-locked memory, streams, events, and the
// temporary storage of a rocprim call.  Host code only.  Every type owns what it holds, releases it in its destructor (which never throws), moves
// and does not copy.  Outside this file a hipMalloc, hipHostMalloc, hipStreamCreate* or hipEventCreate* needs a reason in a comment (DESIGN.md s8:
// HipRT::palloc / pfree, the runtime interface that the host double mirrors).
#pragma once
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <utility>
#include "hip_launch.h"

namespace arx {

// hipMalloc found no room.  The free and total bytes are read where it is thrown, before unwinding frees anything, so that a caller's message
// states what the failed request met (hip_index_build.h: "F of T MiB free"; arx_bgzf.hip turns it into ARX_E_TOO_LARGE for the BAM sort)
struct HipOutOfMemory : HipError {
	size_t wanted, free_bytes = 0, total_bytes = 0;
	explicit HipOutOfMemory(size_t n) : HipError("hipMalloc: out of device memory (" + std::to_string(n >> 20) + " MiB were asked for)"), wanted(n) { (void)hipMemGetInfo(&free_bytes, &total_bytes); }
};

struct DevMem {
	static void *get(size_t n)
	{
		void *p = nullptr;
		const hipError_t e = hipMalloc(&p, n);
		if (e == hipErrorOutOfMemory) { (void)hipGetLastError(); throw HipOutOfMemory(n); } // (the error is sticky: cleared, the next check is not blamed for it)
		hip_check(e, "hipMalloc(...)");
		return p;
	}
	static void put(void *p) { (void)hipFree(p); }
};
struct PinnedMem {
	static void *get(size_t n) { void *p = nullptr; hip_check(hipHostMalloc(&p, n, hipHostMallocDefault), "hipHostMalloc(...)"); return p; }
	static void put(void *p) { (void)hipHostFree(p); }
};
// memory with a scope.  bytes: what was asked for (an empty request still gets a small block, so that p is not null)
template <class Mem> struct Buf {
	void *p = nullptr; size_t bytes = 0;
	Buf() {}
	explicit Buf(size_t n) { alloc(n); }
	Buf(Buf &&o) noexcept : p(std::exchange(o.p, nullptr)), bytes(std::exchange(o.bytes, 0)) {}
	Buf &operator=(Buf &&o) noexcept { if (this != &o) { release(); p = std::exchange(o.p, nullptr); bytes = std::exchange(o.bytes, 0); } return *this; }
	void alloc(size_t n) { release(); p = Mem::get(n ? n : 8); bytes = n; }
	void release() { if (p) Mem::put(p); p = nullptr; bytes = 0; }
	~Buf() { release(); }
	template <class T> T *as() const { return (T *)p; }
};
using DevBuf = Buf<DevMem>;       // hipMalloc / hipFree
using PinnedBuf = Buf<PinnedMem>; // hipHostMalloc / hipHostFree

// a non-blocking stream; empty until create().  Its destructor waits for what is on it: declare it before what is used on it
struct Stream {
	hipStream_t s = nullptr;
	Stream() {}
	Stream(Stream &&o) noexcept : s(std::exchange(o.s, nullptr)) {}
	Stream &operator=(Stream &&o) noexcept { if (this != &o) { release(); s = std::exchange(o.s, nullptr); } return *this; }
	void create() { release(); ARX_HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking)); }
	void release() { if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); } s = nullptr; }
	~Stream() { release(); }
	operator hipStream_t() const { return s; }
};
// an event; empty until create().  hipEventDefault for the pairs that time a launch (HipRT), hipEventDisableTiming for the ones that order work
struct Event {
	hipEvent_t e = nullptr;
	Event() {}
	explicit Event(unsigned flags) { create(flags); }
	Event(Event &&o) noexcept : e(std::exchange(o.e, nullptr)) {}
	Event &operator=(Event &&o) noexcept { if (this != &o) { release(); e = std::exchange(o.e, nullptr); } return *this; }
	void create(unsigned flags) { release(); ARX_HIP_CHECK(hipEventCreateWithFlags(&e, flags)); }
	void release() { if (e) (void)hipEventDestroy(e); e = nullptr; }
	~Event() { release(); }
	operator hipEvent_t() const { return e; }
};

// makes `device` the calling thread's current device.  none: the caller's text where there is no such device; range: its text for an index
// outside the visible devices where that differs
inline void select_device(int device, const char *none, const char *range = nullptr)
{
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) throw HipError(none);
	if (device < 0 || device >= n) throw HipError(range ? range : none);
	ARX_HIP_CHECK(hipSetDevice(device));
}

// one value read home; returns when it is there
template <class T> inline T dev_get(const T *d, hipStream_t st)
{
	T v{};
	ARX_HIP_CHECK(hipMemcpyAsync(&v, d, sizeof(T), hipMemcpyDeviceToHost, st));
	ARX_HIP_CHECK(hipStreamSynchronize(st));
	return v;
}

// temporary storage of the device-wide primitives, grown on demand with a quarter to spare and kept from call to call
struct DevScratch {
	DevBuf buf;
	void *get(size_t bytes) { if (bytes > buf.bytes) buf.alloc(bytes + (bytes >> 2)); return buf.p; }
};
// a rocprim call is made twice: without storage it only says how much it needs.  call(tmp, bytes) -> hipError_t; what: its name in an error
template <class Call> inline void dev_two_pass(DevScratch &sc, const char *what, Call call)
{
	size_t bytes = 0;
	hip_check(call(nullptr, bytes), what);
	void *tmp = sc.get(bytes);
	hip_check(call(tmp, bytes), what);
}
// (kout, vout) = (kin, vin) ordered by the low `bits` bits of the keys, equal keys in their order
template <class K, class V> inline void dev_sort_pairs(DevScratch &sc, const K *kin, K *kout, const V *vin, V *vout, size_t n, int bits, hipStream_t st)
{
	dev_two_pass(sc, "rocprim::radix_sort_pairs", [&](void *tmp, size_t &bytes) { return rocprim::radix_sort_pairs(tmp, bytes, kin, kout, vin, vout, n, 0u, (unsigned)bits, st); });
}

} // namespace arx
