// Internal to libvp8hip.so: the owning types of what a context holds (vp8hip_ctx.hip.h) -- buffers, events, streams.  Each frees
// its handle in its destructor, so a member of one of these types needs no line in vp8hip_destroy, in a failure path or in
// whatever gives memory back (reset()); none can be copied.  The device of the context must be current when one is destroyed.
#pragma once
#include <hip/hip_runtime.h>
#include <stdlib.h>

// where a Buf's memory comes from: the device, page-locked host memory (plain or mapped), the (zeroed) heap
struct DeviceMem {
    static hipError_t alloc(void **p, size_t bytes) { return hipMalloc(p, bytes); }
    static void release(void *p) { (void)hipFree(p); }
};
struct PinnedMem {
    static hipError_t alloc(void **p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
    static void release(void *p) { (void)hipHostFree(p); }
};
struct MappedMem {       // page-locked and mapped into the device's address space (hipHostGetDevicePointer)
    static hipError_t alloc(void **p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocMapped); }
    static void release(void *p) { (void)hipHostFree(p); }
};
struct HeapMem {
    static hipError_t alloc(void **p, size_t bytes) { return (*p = calloc(1, bytes)) ? hipSuccess : hipErrorOutOfMemory; }
    static void release(void *p) { free(p); }
};

// A typed pointer and its capacity, counted in whatever unit the call site counts in (elements, bytes, digests).  Reads as the
// pointer it holds.
template <class T, class Mem> struct Buf {
    T *p = nullptr;
    size_t cap = 0;
    Buf() = default;
    Buf(Buf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    ~Buf() { reset(); }
    operator T *() const { return p; }
    void reset()
    {
        if (p) Mem::release(p);
        p = nullptr; cap = 0;
    }
    // THE place a buffer grows: room for `want` units, which take `bytes` bytes.  Enough already: nothing happens; else what is
    // there is freed -- the caller has waited for whatever may still read it, and has rounded `want` as it sees fit -- and the
    // capacity is recorded once the allocation has succeeded.  On failure the buffer is {nullptr, 0}, the runtime's sticky error
    // is cleared and the error returned.
    hipError_t grow(size_t want, size_t bytes)
    {
        if (p && want <= cap) return hipSuccess;
        reset();
        const hipError_t e = Mem::alloc((void **)&p, bytes);
        if (e != hipSuccess) { (void)hipGetLastError(); p = nullptr; return e; }
        cap = want;
        return hipSuccess;
    }
    hipError_t grow(size_t n) { return grow(n, n * sizeof(T)); }      // ... counted in elements
};
// Buffers that are used together -- a device table and its staging -- grow together: the capacity of the set is its smallest, so
// after a failure part-way (that buffer is {nullptr, 0}) the next call grows again, and grow() returns at once for those with room.
template <class A, class B> static inline size_t vp8hip_cap(const A &a, const B &b) { return a.cap < b.cap ? a.cap : b.cap; }
template <class T> using DevBuf = Buf<T, DeviceMem>;
template <class T> using PinnedBuf = Buf<T, PinnedMem>;
template <class T> using MappedBuf = Buf<T, MappedMem>;
template <class T> using HeapBuf = Buf<T, HeapMem>;

// An event / a stream, null until ensure() -- "create if absent" -- has succeeded.  (A stream of priority 0 is the stream
// hipStreamCreateWithFlags makes.)
struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(const Event &) = delete;
    ~Event() { if (e) (void)hipEventDestroy(e); }
    operator hipEvent_t() const { return e; }
    hipError_t ensure(unsigned flags = hipEventDisableTiming) { return e ? hipSuccess : hipEventCreateWithFlags(&e, flags); }
};
struct Stream {
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(const Stream &) = delete;
    ~Stream() { if (s) (void)hipStreamDestroy(s); }
    operator hipStream_t() const { return s; }
    hipError_t ensure(int priority = 0) { return s ? hipSuccess : hipStreamCreateWithPriority(&s, hipStreamNonBlocking, priority); }
};
