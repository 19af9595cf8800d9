// ASan + UBSan run of csrc/avr_devmem.h on the host: the operations of tests/test_devmem_header.py
// over the counting malloc policy, every byte of every block written, plus early returns out of a
// function that holds an arena and three buffers (tests/test_sanitize.py builds and runs this).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "devmem_counting.h"

using avr::devmem::Arena;
using avr::devmem::Buffer;

#define CHECK(cond)                                                            \
    do {                                                                       \
        if (!(cond)) {                                                         \
            std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            std::abort();                                                      \
        }                                                                      \
    } while (0)

struct R12 { float x, y, z; };

// the walks entry point's layout, every range written to its last byte and read back
static void arena_layouts() {
    int drains = 0;
    for (size_t n : {(size_t)0, (size_t)1, (size_t)5, (size_t)63}) {
        Arena<Counting> a(&drains);
        const auto rO = a.reserve<R12>(n), rD = a.reserve<R12>(n);
        const auto rT = a.reserve<float>(n);
        const auto rI = a.reserve<long long>(n);
        const auto rP = a.reserve<R12>(n * 7);
        const auto rC = a.reserve<int>(n);
        const auto rZ = a.reserve<int>(0);
        const auto rB = a.reserve<unsigned char>(3);
        CHECK(a.commit() == Counting::ok);
        for (size_t off : {rO.offset, rD.offset, rT.offset, rI.offset, rP.offset, rC.offset, rZ.offset, rB.offset})
            CHECK(off % 16 == 0 && off <= a.bytes());
        std::memset(a.get(rO), 1, n * sizeof(R12));
        std::memset(a.get(rD), 2, n * sizeof(R12));
        for (size_t i = 0; i < n; ++i) a.get(rT)[i] = 3.f, a.get(rI)[i] = 4, a.get(rC)[i] = 6;
        std::memset(a.get(rP), 5, n * 7 * sizeof(R12));
        std::memset(a.get(rB), 8, 3);
        for (size_t i = 0; i < n; ++i) {
            CHECK(a.get(rT)[i] == 3.f && a.get(rI)[i] == 4 && a.get(rC)[i] == 6);
            CHECK(((unsigned char *)a.get(rO))[i * 12 + 11] == 1 && ((unsigned char *)a.get(rD))[i * 12] == 2);
        }
        CHECK(a.get(rB)[2] == 8);
        CHECK((char *)a.get(rZ) == (char *)a.get(rB));   // a zero-length range takes no room
    }
    CHECK(drains == 4 && Counting::allocs == 4 && Counting::frees == 4);
    {   // offsets past 2^31 bytes, never committed: nothing allocated, nothing drained
        Arena<Counting> a(&drains);
        const auto r0 = a.reserve<int>(5);
        const auto r1 = a.reserve<unsigned char>(((size_t)1 << 31) + 8);
        const auto r2 = a.reserve<long long>(3);
        CHECK(r0.offset == 0 && r1.offset == 32 && r2.offset == 32 + ((size_t)1 << 31) + 16);
        CHECK(a.bytes() == r2.offset + 32);
    }
    CHECK(drains == 4 && Counting::allocs == 4);
}

static void buffers() {
    Buffer<int, Counting> b;
    CHECK(!b && b.get() == nullptr && b.size() == 0);
    CHECK(b.alloc(10) == Counting::ok && b.size() == 10);
    for (size_t i = 0; i < b.size(); ++i) b.get()[i] = (int)i;
    CHECK(b.alloc(0) == Counting::ok && b && b.size() == 0);
    b.get()[0] = 1;   // at least one entry
    // a failing allocation leaves it empty; a later one works
    Counting::fail_in = 0;
    CHECK(b.alloc(4) != Counting::ok && !b && b.size() == 0);
    CHECK(b.alloc(4) == Counting::ok && b.size() == 4);
    b.get()[3] = 3;
    // reserve grows only
    int drains = 0;
    const int *p = b.get();
    CHECK(b.reserve(4, &drains) == Counting::ok && b.reserve(1) == Counting::ok && b.get() == p && drains == 0);
    CHECK(b.reserve(9, &drains) == Counting::ok && b.size() == 9 && drains == 1);
    b.get()[8] = 8;
    // moves
    Buffer<int, Counting> c(std::move(b));
    CHECK(!b && b.size() == 0 && c.size() == 9 && c.get()[8] == 8);
    Buffer<int, Counting> d;
    CHECK(d.alloc(2) == Counting::ok);
    d = std::move(c);
    CHECK(!c && d.size() == 9 && d.get()[8] == 8);
    b = std::move(d);
    CHECK(b.size() == 9 && !d);
    // the headroom variant: no room and a failed allocation are no errors, a failed query is
    Buffer<R12, Counting> e;
    Counting::room_bytes = 119;
    CHECK(e.alloc_if_room(10) == Counting::ok && !e);
    Counting::room_bytes = 120;
    CHECK(e.alloc_if_room(10) == Counting::ok && e.size() == 10);
    e.get()[9].z = 1.f;
    Counting::fail_in = 0;
    CHECK(e.alloc_if_room(10) == Counting::ok && !e);
    Counting::room_error = 7;
    CHECK(e.alloc_if_room(10) == 7 && !e);
    Counting::room_error = 0;
    Counting::room_bytes = ~0ull;
    std::vector<Buffer<int, Counting>> pool(3);   // a member array's worth, moved by the vector's growth
    for (auto &q : pool) CHECK(q.alloc(3) == Counting::ok);
    pool.resize(40);
    CHECK(pool[2].size() == 3 && !pool[39]);
}

// An entry point's shape: an arena and three buffers, left at `stop` (0 .. 5) by an early return
static int entry_point(int stop, int *drains) {
    Buffer<float, Counting> a, b;
    if (a.alloc(7) != Counting::ok) return 1;
    if (stop == 0) return 10;
    Arena<Counting> scratch(drains);
    const auto r0 = scratch.reserve<int>(11);
    const auto r1 = scratch.reserve<R12>(3);
    if (stop == 1) return 11;              // reserved, never committed
    if (scratch.commit() != Counting::ok) return 2;
    scratch.get(r0)[10] = 1;
    scratch.get(r1)[2].z = 2.f;
    if (stop == 2) return 12;
    if (b.alloc(5) != Counting::ok) return 3;
    b.get()[4] = 4.f;
    if (stop == 3) return 13;
    Buffer<long long, Counting> c;
    if (c.reserve(2, drains) != Counting::ok) return 4;
    c.get()[1] = 5;
    if (stop == 4) return 14;
    a = std::move(b);
    return 0;
}

static void early_returns() {
    for (int stop = 0; stop <= 5; ++stop) {
        int drains = 0;
        const long before = Counting::allocs;
        CHECK(entry_point(stop, &drains) == (stop < 5 ? 10 + stop : 0));
        CHECK(Counting::allocs == Counting::frees && Counting::live_bytes == 0);
        CHECK(Counting::allocs - before == (stop == 0 ? 1 : stop == 1 ? 1 : stop == 2 ? 2 : stop == 3 ? 3 : 4));
        CHECK(drains == (stop < 2 ? 0 : stop < 4 ? 1 : 2));   // the arena's, and reserve's
    }
    // and with every allocation of the function failing in turn
    for (long k = 0; k < 4; ++k) {
        int drains = 0;
        Counting::fail_in = k;
        CHECK(entry_point(5, &drains) == (int)k + 1);
        CHECK(Counting::allocs == Counting::frees && Counting::live_bytes == 0);
    }
    Counting::fail_in = -1;
}

int main() {
    Counting::reset();
    arena_layouts();
    buffers();
    early_returns();
    CHECK(Counting::allocs == Counting::frees && Counting::live_bytes == 0 && Counting::allocs > 20);
    std::puts("sanitize devmem ok");
    return 0;
}
