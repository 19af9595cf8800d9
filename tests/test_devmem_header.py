"""The device-memory owners of the host code (csrc/avr_devmem.h), compiled for the host with g++
over the malloc-backed allocator policy behind a counting wrapper (tests/devmem_counting.h): the
scratch arena's layout (every sub-range aligned to 16 B, inside the block, none overlapping) on
the layouts the entry points reserve, and the owning buffer's rules (empty after a failed
allocation, grow-only reserve, moves, the headroom variant, one free per allocation)."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHIM = r"""
#include <cstring>
#include <new>
#include "%s"
typedef unsigned long long u64;
using avr::devmem::Arena;
using avr::devmem::Buffer;
struct R12 { char b[12]; };
typedef Buffer<int, Counting> Buf;
template <typename T>
static u64 take(Arena<Counting> &a, u64 n) { return a.reserve<T>((size_t)n).offset; }
extern "C" {
// Reserve n ranges of count[i] entries of elem[i] bytes (1, 4, 8 or 12) on one arena: their
// offsets and the block's size; with commit, also the block's and the ranges' addresses, every
// range filled with its own byte and read back (-1 - i: range i was overwritten by another)
int arena_layout(int n, const int *elem, const u64 *count, int commit, u64 *offset, u64 *bytes, u64 *base,
                 u64 *addr, int *drains) {
  *drains = 0;
  int rc = 0;
  {
    Arena<Counting> a(drains);
    for (int i = 0; i < n; ++i)
      offset[i] = elem[i] == 1 ? take<char>(a, count[i]) : elem[i] == 4 ? take<float>(a, count[i])
                : elem[i] == 8 ? take<long long>(a, count[i]) : take<R12>(a, count[i]);
    *bytes = a.bytes();
    if (!commit) return 0;
    if (a.commit() != Counting::ok) return 1;
    *base = (u64)a.get(Arena<Counting>::Range<char>{0, 0});
    for (int i = 0; i < n; ++i) {
      char *p = a.get(Arena<Counting>::Range<char>{(size_t)offset[i], 0});
      addr[i] = (u64)p;
      std::memset(p, i + 1, (size_t)(count[i] * elem[i]));
    }
    for (int i = 0; i < n && !rc; ++i)
      for (u64 k = 0; k < count[i] * elem[i]; ++k)
        if (((char *)addr[i])[k] != (char)(i + 1)) { rc = -1 - i; break; }
  }
  return rc;
}
// typed pointers come from the handles: a range's address is the block's plus its offset
int arena_typed_get() {
  int drains = 0;
  Arena<Counting> a(&drains);
  const auto r0 = a.reserve<int>(3);
  const auto r1 = a.reserve<long long>(2);
  const auto r2 = a.reserve<R12>(5);
  if (a.commit() != Counting::ok) return 1;
  int *p0 = a.get(r0);
  long long *p1 = a.get(r1);
  R12 *p2 = a.get(r2);
  return ((char *)p1 - (char *)p0 == 16 && (char *)p2 - (char *)p1 == 16 && r2.n == 5) ? 0 : 2;
}
void counters(long long *out) {
  out[0] = Counting::allocs; out[1] = Counting::frees; out[2] = Counting::live_bytes; out[3] = Counting::drains;
  out[4] = Counting::cleared;
}
void counting_reset() { Counting::reset(); }
void fail_in(long k) { Counting::fail_in = k; }
void set_room(u64 bytes, int error) { Counting::room_bytes = bytes; Counting::room_error = error; }
Buf *buf_new() { return new Buf(); }
void buf_delete(Buf *b) { delete b; }
int buf_alloc(Buf *b, u64 n) { return b->alloc((size_t)n); }
int buf_alloc_if_room(Buf *b, u64 n) { return b->alloc_if_room((size_t)n); }
int buf_reserve(Buf *b, u64 n, int *drain) { return drain ? b->reserve((size_t)n, drain) : b->reserve((size_t)n); }
void buf_reset(Buf *b) { b->reset(); }
u64 buf_ptr(const Buf *b) { return (u64)b->get(); }
u64 buf_size(const Buf *b) { return b->size(); }
int buf_bool(const Buf *b) { return *b ? 1 : 0; }
Buf *buf_move_construct(Buf *from) { return new Buf(std::move(*from)); }
void buf_move_assign(Buf *to, Buf *from) { *to = std::move(*from); }
void buf_fill(Buf *b, int v) { for (size_t i = 0; i < b->size(); ++i) b->get()[i] = v; }
}
"""

U64 = ctypes.c_ulonglong
PU64 = ctypes.POINTER(U64)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("devmem")
    src = d / "shim.cpp"
    src.write_text(SHIM % os.path.join(ROOT, "tests", "devmem_counting.h"))
    so = d / "shim.so"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", str(src), "-o", str(so)])
    L = ctypes.CDLL(str(so))
    ip = ctypes.POINTER(ctypes.c_int)
    L.arena_layout.argtypes = [ctypes.c_int, ip, PU64, ctypes.c_int, PU64, PU64, PU64, PU64, ip]
    L.counters.argtypes = [ctypes.POINTER(ctypes.c_longlong)]
    L.counters.restype = None
    L.fail_in.argtypes = [ctypes.c_long]
    L.set_room.argtypes = [U64, ctypes.c_int]
    L.buf_new.restype = ctypes.c_void_p
    L.buf_move_construct.restype = ctypes.c_void_p
    L.buf_move_construct.argtypes = [ctypes.c_void_p]
    L.buf_move_assign.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    for name in ("buf_delete", "buf_reset"):
        getattr(L, name).argtypes = [ctypes.c_void_p]
        getattr(L, name).restype = None
    for name in ("buf_alloc", "buf_alloc_if_room"):
        getattr(L, name).argtypes = [ctypes.c_void_p, U64]
    L.buf_reserve.argtypes = [ctypes.c_void_p, U64, ip]
    L.buf_fill.argtypes = [ctypes.c_void_p, ctypes.c_int]
    for name in ("buf_ptr", "buf_size"):
        getattr(L, name).argtypes = [ctypes.c_void_p]
        getattr(L, name).restype = U64
    L.buf_bool.argtypes = [ctypes.c_void_p]
    return L


def counters(lib):
    out = (ctypes.c_longlong * 5)()
    lib.counters(out)
    return dict(zip(("allocs", "frees", "live_bytes", "drains", "cleared"), out))


@pytest.fixture
def clean(lib):
    """Counters at zero before, and allocations equal to frees after every scope has closed."""
    lib.counting_reset()
    yield lib
    c = counters(lib)
    assert c["allocs"] == c["frees"] and c["live_bytes"] == 0, c
    lib.counting_reset()


def layout(lib, ranges, commit=True):
    n = len(ranges)
    elem = (ctypes.c_int * max(n, 1))(*[e for e, _ in ranges])
    count = (U64 * max(n, 1))(*[k for _, k in ranges])
    offset, addr = (U64 * max(n, 1))(), (U64 * max(n, 1))()
    nbytes, base, drains = U64(), U64(), ctypes.c_int()
    rc = lib.arena_layout(n, elem, count, int(commit), offset, ctypes.byref(nbytes), ctypes.byref(base), addr,
                          ctypes.byref(drains))
    assert rc == 0, rc
    return list(offset)[:n], nbytes.value, base.value, list(addr)[:n], drains.value


def check_layout(ranges, offsets, nbytes):
    """16-B alignment, inside [0, nbytes), ascending without overlap, no more padding than 15 B each."""
    end = 0
    for (elem, count), off in zip(ranges, offsets):
        assert off % 16 == 0
        assert end <= off <= end + 15
        end = off + elem * count
        assert end <= nbytes
    assert nbytes % 16 == 0
    assert nbytes - sum(e * k for e, k in ranges) <= 15 * len(ranges)


# The layouts the entry points reserve, at sizes that are no multiple of 16 B
# (elem bytes, entries): 4 int / float, 8 long long / u64, 12 a float3 record, 1 raw bytes
LAYOUTS = {
    "start_rays": [(4, 49), (4, 49), (12, 49)],
    "walks": [(12, 5), (12, 5), (4, 5), (8, 5), (12, 5 * 3 * 7), (4, 15)],
    "reinforce": [(4, 3), (12, 3), (12, 9), (12, 9), (4, 9), (4, 9)],
    "light": [(12, 7), (4, 7), (12, 7 * 25), (4, 7), (4, 7 * 25 * 3)],
    "propagate": [(4, 8), (4, 13), (4, 13), (4, 7), (4, 7)],
    "merge": [(12, 21), (12, 21), (8, 1), (4, 28), (4, 11), (4, 11), (4, 11), (4, 11), (4, 11), (4, 1), (4, 256)],
    "light_probe": [(4, 6), (4, 9), (4, 12), (4, 9), (4, 3), (4, 12), (4, 3), (4, 12)],
    "voxels": [(1, 333), (4, 333), (4, 333), (4, 1)],
    "zero_first": [(4, 0), (8, 3), (12, 0), (4, 1)],
    "zero_only": [(4, 0), (8, 0)],
    "single": [(12, 1)],
    "single_one_byte": [(1, 1)],
    "none": [],
}


@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_arena_ranges_are_aligned_disjoint_and_inside_the_block(clean, name):
    ranges = LAYOUTS[name]
    offsets, nbytes, base, addr, drains = layout(clean, ranges)
    check_layout(ranges, offsets, nbytes)
    assert [a - base for a in addr] == offsets
    assert base % 16 == 0   # the allocator's own alignment carries the offsets'
    # one block, drained once on its stream and then freed, when the arena goes
    c = counters(clean)
    assert (c["allocs"], c["frees"], drains, c["drains"]) == (1, 1, 1, 1)
    # the offsets do not depend on the commit
    assert layout(clean, ranges, commit=False)[:2] == (offsets, nbytes)


def test_arena_offsets_past_two_gib(clean):
    """A range of 2^31 + 8 bytes between two others: the offsets only, nothing is allocated."""
    big = 2 ** 31 + 8
    ranges = [(4, 5), (1, big), (8, 3), (12, (big + 11) // 12), (4, 1)]
    offsets, nbytes, _, _, drains = layout(clean, ranges, commit=False)
    check_layout(ranges, offsets, nbytes)
    assert offsets[2] == 32 + big + 8 and offsets[2] > 2 ** 31
    assert offsets[4] > 2 ** 32 and nbytes == offsets[4] + 16
    c = counters(clean)
    assert (c["allocs"], c["frees"], drains) == (0, 0, 0)   # an arena never committed drains nothing


def test_arena_typed_pointers(clean):
    assert clean.arena_typed_get() == 0


def test_failed_arena_commit_frees_nothing(clean):
    clean.fail_in(0)
    elem, count = (ctypes.c_int * 1)(4), (U64 * 1)(10)
    o, a, nb, base, dr = (U64 * 1)(), (U64 * 1)(), U64(), U64(), ctypes.c_int()
    assert clean.arena_layout(1, elem, count, 1, o, ctypes.byref(nb), ctypes.byref(base), a, ctypes.byref(dr)) == 1
    c = counters(clean)
    assert (c["allocs"], c["frees"], c["drains"]) == (0, 0, 0)


def test_buffer_alloc_records_entries_and_keeps_one_entry_at_least(clean):
    b = clean.buf_new()
    assert (clean.buf_ptr(b), clean.buf_size(b), clean.buf_bool(b)) == (0, 0, 0)
    assert clean.buf_alloc(b, 10) == 0
    assert clean.buf_size(b) == 10 and clean.buf_bool(b) == 1 and counters(clean)["live_bytes"] == 40
    clean.buf_fill(b, 7)
    assert clean.buf_alloc(b, 0) == 0    # the old block goes first; 0 entries still have an address
    assert clean.buf_size(b) == 0 and clean.buf_ptr(b) != 0 and counters(clean)["live_bytes"] == 4
    clean.buf_reset(b)
    assert (clean.buf_ptr(b), clean.buf_size(b), counters(clean)["live_bytes"]) == (0, 0, 0)
    clean.buf_reset(b)   # twice is once
    clean.buf_delete(b)
    c = counters(clean)
    assert (c["allocs"], c["frees"]) == (2, 2)


def test_failed_allocation_leaves_the_buffer_empty_and_a_later_one_works(clean):
    b = clean.buf_new()
    assert clean.buf_alloc(b, 5) == 0
    clean.fail_in(0)
    assert clean.buf_alloc(b, 6) != 0
    assert (clean.buf_ptr(b), clean.buf_size(b), clean.buf_bool(b)) == (0, 0, 0)
    c = counters(clean)
    assert (c["allocs"], c["frees"], c["live_bytes"]) == (1, 1, 0)   # the old block went first
    assert clean.buf_alloc(b, 6) == 0 and clean.buf_size(b) == 6
    clean.buf_fill(b, 1)
    # the same through reserve
    clean.fail_in(0)
    assert clean.buf_reserve(b, 7, None) != 0
    assert (clean.buf_ptr(b), clean.buf_size(b)) == (0, 0)
    assert clean.buf_reserve(b, 7, None) == 0 and clean.buf_size(b) == 7
    clean.buf_delete(b)


def test_reserve_reallocates_only_when_asked_for_more(clean):
    b = clean.buf_new()
    drains = ctypes.c_int(0)
    assert clean.buf_reserve(b, 0, drains) == 0   # nothing asked of an empty buffer: nothing made
    assert clean.buf_ptr(b) == 0 and counters(clean)["allocs"] == 0 and drains.value == 0
    assert clean.buf_reserve(b, 8, drains) == 0
    p = clean.buf_ptr(b)
    assert counters(clean)["allocs"] == 1 and drains.value == 1   # drained before the (empty) old block went
    for n in (8, 3, 0):
        assert clean.buf_reserve(b, n, drains) == 0
        assert (clean.buf_ptr(b), clean.buf_size(b)) == (p, 8)
    assert counters(clean)["allocs"] == 1 and drains.value == 1
    assert clean.buf_reserve(b, 9, drains) == 0
    c = counters(clean)
    assert clean.buf_size(b) == 9 and (c["allocs"], c["frees"], drains.value) == (2, 1, 2)
    assert clean.buf_reserve(b, 10, None) == 0    # without a stream: no drain
    assert counters(clean)["drains"] == 2 and clean.buf_size(b) == 10
    clean.buf_delete(b)


def test_moved_from_buffer_frees_nothing(clean):
    a = clean.buf_new()
    assert clean.buf_alloc(a, 4) == 0
    p = clean.buf_ptr(a)
    b = clean.buf_move_construct(a)
    assert (clean.buf_ptr(a), clean.buf_size(a)) == (0, 0) and (clean.buf_ptr(b), clean.buf_size(b)) == (p, 4)
    clean.buf_delete(a)
    assert counters(clean)["frees"] == 0
    c = clean.buf_new()
    assert clean.buf_alloc(c, 2) == 0
    clean.buf_move_assign(c, b)          # c's own block is freed, b's is taken
    assert counters(clean)["frees"] == 1
    assert (clean.buf_ptr(c), clean.buf_size(c)) == (p, 4) and (clean.buf_ptr(b), clean.buf_size(b)) == (0, 0)
    clean.buf_fill(c, 3)
    clean.buf_move_assign(c, c)          # onto itself: nothing happens
    assert (clean.buf_ptr(c), clean.buf_size(c)) == (p, 4)
    clean.buf_delete(b)
    assert counters(clean)["frees"] == 1
    clean.buf_delete(c)
    assert counters(clean)["frees"] == 2


def test_alloc_if_room_is_no_error_without_room(clean):
    b = clean.buf_new()
    assert clean.buf_alloc(b, 3) == 0
    clean.set_room(39, 0)
    assert clean.buf_alloc_if_room(b, 10) == 0     # 40 B asked, 39 admitted: empty, the attempt forgotten
    c = counters(clean)
    assert clean.buf_bool(b) == 0 and (c["allocs"], c["frees"], c["cleared"]) == (1, 1, 1)
    clean.set_room(40, 0)
    assert clean.buf_alloc_if_room(b, 10) == 0 and clean.buf_size(b) == 10
    assert counters(clean)["cleared"] == 1
    clean.fail_in(0)                               # room, but the allocation fails: also no error
    assert clean.buf_alloc_if_room(b, 10) == 0 and clean.buf_bool(b) == 0 and counters(clean)["cleared"] == 2
    clean.set_room(1 << 40, 5)                     # the query itself fails: its error, nothing cleared
    assert clean.buf_alloc_if_room(b, 10) == 5 and clean.buf_bool(b) == 0 and counters(clean)["cleared"] == 2
    clean.buf_delete(b)


def test_header_is_in_the_library_sources():
    from acceleratedvolrenderer_amd import build
    assert os.path.join(build.CSRC, "avr_devmem.h") in build.DEPS
