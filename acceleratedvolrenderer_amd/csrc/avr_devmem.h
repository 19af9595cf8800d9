// avr_devmem.h — ownership of device memory in the host code (avr_capi.hip, avr_render.hip,
// avr_graph_capi.hip): an owning buffer and a per-call scratch arena, both templated on an
// allocator policy. HipAlloc is the library's; MallocAlloc lets this header (and its tests)
// compile with a plain host compiler. Host code only: nothing here is seen by a kernel, the view
// structs the kernels take (DevMedium, DevFilm, PathSoA, ...) stay plain pointers filled from get().
//
// A policy provides
//   error_t, ok, stream_t
//   error_t alloc(void **p, size_t bytes)     the block
//   void    free(void *p, size_t bytes)
//   error_t drain(stream_t s)                 wait for the work queued on s
//   error_t room(size_t bytes, bool *fits)    whether `bytes` may be taken (the headroom rule)
//   void    clear_error()                     forget a failed alloc (HIP's sticky last error)
#pragma once

#include <atomic>
#include <cstddef>
#include <cstdlib>
#include <utility>

namespace avr {
namespace devmem {

struct MallocAlloc {
    using error_t = int;
    using stream_t = void *;
    static constexpr error_t ok = 0;
    static error_t alloc(void **p, size_t bytes) { return (*p = std::malloc(bytes)) ? ok : 1; }
    static void free(void *p, size_t) { std::free(p); }
    static error_t drain(stream_t) { return ok; }
    static error_t room(size_t, bool *fits) { *fits = true; return ok; }
    static void clear_error() {}
};

#if defined(__HIPCC__)
// device memory this process holds through HipAlloc (avr_debug_live_device_bytes)
inline std::atomic<unsigned long long> g_live_bytes{0}, g_live_blocks{0};

struct HipAlloc {
    using error_t = hipError_t;
    using stream_t = hipStream_t;
    static constexpr error_t ok = hipSuccess;
    static error_t alloc(void **p, size_t bytes) {
        const error_t e = hipMalloc(p, bytes);
        if (e == ok) g_live_bytes += bytes, ++g_live_blocks;
        return e;
    }
    static void free(void *p, size_t bytes) {
        (void)hipFree(p);
        g_live_bytes -= bytes, --g_live_blocks;
    }
    static error_t drain(stream_t s) { return hipStreamSynchronize(s); }
    // optional copies and tables (a fat or bricked density copy, a ZSobol pass table) are made
    // only with 8 GiB of HBM to spare: path state, film and other ranks' traffic come first
    static error_t room(size_t bytes, bool *fits) {
        size_t freeB = 0, totalB = 0;
        const error_t e = hipMemGetInfo(&freeB, &totalB);
        *fits = e == ok && bytes + (8ull << 30) < freeB;
        return e;
    }
    static void clear_error() { (void)hipGetLastError(); }
};
using DefaultAlloc = HipAlloc;
#else
using DefaultAlloc = MallocAlloc;
#endif

// n entries of T on the device, freed with the buffer. size() is the entry count asked for; the
// block holds at least one entry, so a buffer of 0 entries still has an address.
template <typename T, typename A = DefaultAlloc>
class Buffer {
  public:
    using error_t = typename A::error_t;
    Buffer() = default;
    Buffer(Buffer &&o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr, o.n_ = 0; }
    Buffer &operator=(Buffer &&o) noexcept {
        if (this != &o) {
            reset();
            std::swap(p_, o.p_);
            std::swap(n_, o.n_);
        }
        return *this;
    }
    ~Buffer() { reset(); }   // (move-only: the move operations above delete the copies)

    T *get() const { return p_; }
    size_t size() const { return n_; }
    explicit operator bool() const { return p_ != nullptr; }
    void reset() {
        if (p_) A::free(p_, bytes(n_));
        p_ = nullptr;
        n_ = 0;
    }
    // exactly n entries, contents undefined: the old block goes first, and a failure leaves the
    // buffer empty
    error_t alloc(size_t n) {
        reset();
        void *q = nullptr;
        const error_t e = A::alloc(&q, bytes(n));
        if (e == A::ok) p_ = static_cast<T *>(q), n_ = n;
        return e;
    }
    // ... only when the policy's headroom rule admits them. No room is no error: the buffer is
    // empty then, and the failed attempt is forgotten. An error is the room query's only.
    error_t alloc_if_room(size_t n) {
        reset();
        bool fits = false;
        const error_t e = A::room(bytes(n), &fits);
        if (e != A::ok) return e;
        if (!fits || alloc(n) != A::ok) A::clear_error();
        return A::ok;
    }
    // at least n entries (contents are not kept when it grows). drain: work queued on that stream
    // may still read the old block, so the stream is drained before the block is freed.
    error_t reserve(size_t n) { return n <= n_ ? A::ok : alloc(n); }
    error_t reserve(size_t n, typename A::stream_t drain) {
        if (n <= n_) return A::ok;
        const error_t e = A::drain(drain);
        return e != A::ok ? e : alloc(n);
    }

  private:
    static size_t bytes(size_t n) { return (n ? n : 1) * sizeof(T); }
    T *p_ = nullptr;
    size_t n_ = 0;
};

// The scratch of one entry-point call on one stream: reserve the typed sub-ranges (each aligned
// to 16 B), commit() the one block, take the pointers. The destructor drains the stream and then
// frees the block, so a return from anywhere leaves no kernel or copy behind that reads the
// block or the caller's host arrays.
template <typename A = DefaultAlloc>
class Arena {
  public:
    template <typename T>
    struct Range {
        size_t offset, n;   // bytes into the block, entries
        size_t bytes() const { return n * sizeof(T); }
    };
    explicit Arena(typename A::stream_t s) : s_(s) {}
    Arena(const Arena &) = delete;
    Arena &operator=(const Arena &) = delete;
    ~Arena() {
        if (!base_) return;
        (void)A::drain(s_);
        A::free(base_, bytes_ ? bytes_ : 1);
    }
    template <typename T>
    Range<T> reserve(size_t n) {
        const Range<T> r{bytes_, n};
        bytes_ += (n * sizeof(T) + 15) & ~(size_t)15;
        return r;
    }
    typename A::error_t commit() {
        void *q = nullptr;
        const typename A::error_t e = A::alloc(&q, bytes_ ? bytes_ : 1);
        if (e == A::ok) base_ = static_cast<char *>(q);
        return e;
    }
    template <typename T>
    T *get(Range<T> r) const { return reinterpret_cast<T *>(base_ + r.offset); }
    size_t bytes() const { return bytes_; }

  private:
    typename A::stream_t s_;
    size_t bytes_ = 0;
    char *base_ = nullptr;
};

#if defined(__HIPCC__)
// A stream, an event or pinned host memory destroyed with its owner
template <typename H, hipError_t (*Destroy)(H)>
struct Handle {
    H h = nullptr;
    Handle() = default;
    Handle(Handle &&o) noexcept : h(o.h) { o.h = nullptr; }   // (move-only)
    ~Handle() { if (h) (void)Destroy(h); }
    operator H() const { return h; }
};
using Stream = Handle<hipStream_t, hipStreamDestroy>;
using Event = Handle<hipEvent_t, hipEventDestroy>;
inline hipError_t free_pinned(int *p) { return hipHostFree(p); }
using PinnedInts = Handle<int *, free_pinned>;
#endif

}  // namespace devmem
}  // namespace avr
