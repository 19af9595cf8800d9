// A counting allocator policy for csrc/avr_devmem.h over its malloc-backed one: what the host
// tests (tests/test_devmem_header.py, tests/sanitize_devmem_main.cpp) observe and inject.
#pragma once

#include "../acceleratedvolrenderer_amd/csrc/avr_devmem.h"

struct Counting {
    using error_t = int;
    using stream_t = int *;   // a "stream" is a counter of its drains
    static constexpr error_t ok = 0;
    static inline long allocs = 0, frees = 0, drains = 0, cleared = 0;
    static inline long long live_bytes = 0;
    static inline long fail_in = -1;                       // the alloc that fails: 0 the next one, -1 none
    static inline unsigned long long room_bytes = ~0ull;   // what the headroom rule admits
    static inline int room_error = 0;                      // what the room query returns
    static void reset() {
        allocs = frees = drains = cleared = 0, live_bytes = 0, fail_in = -1, room_bytes = ~0ull, room_error = 0;
    }
    static error_t alloc(void **p, size_t bytes) {
        if (fail_in >= 0 && fail_in-- == 0) return 1;
        const error_t e = avr::devmem::MallocAlloc::alloc(p, bytes);
        if (e == ok) ++allocs, live_bytes += (long long)bytes;
        return e;
    }
    static void free(void *p, size_t bytes) {
        avr::devmem::MallocAlloc::free(p, bytes);
        ++frees, live_bytes -= (long long)bytes;
    }
    static error_t drain(stream_t s) {
        ++drains;
        if (s) ++*s;
        return ok;
    }
    static error_t room(size_t bytes, bool *fits) {
        *fits = room_error == 0 && bytes <= room_bytes;
        return room_error;
    }
    static void clear_error() { ++cleared; }
};
