"""CPU test of the triangle-overlap ABI (rt_tri_overlaps_scratch_bytes, rt_tri_overlaps_count, rt_tri_overlaps_collect): the
header declares the entry points, the flag and the status bits, the library exports them, the scratch size is the range
query's, and every argument error -- unknown flag bits included -- is refused before any GPU work (the pointers below are never
dereferenced: a correct library returns before it touches them)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000          # a 256-byte aligned "device pointer" that must never be used
FAKE_4 = FAKE + 4       # 4-byte aligned only


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rt_abi.h")).read(), flags=re.S)


def test_header_declares_the_entry_points():
    src = _header()
    assert re.search(r"\bsize_t\s+rt_tri_overlaps_scratch_bytes\s*\(\s*uint32_t\s+num_queries\s*\)", src)
    assert re.search(r"\bint\s+rt_tri_overlaps_count\s*\(\s*const\s+rt_accel\s*\*\s*as\s*,\s*const\s+rt_triangle\s*\*\s*queries\s*,"
                     r"\s*uint32_t\s+num_queries\s*,\s*uint32_t\s+flags\s*,\s*uint64_t\s*\*\s*offsets\s*,\s*void\s*\*\s*scratch\s*,"
                     r"\s*uint64_t\s*\*\s*counters\s*,\s*uint32_t\s*\*\s*status\s*,\s*void\s*\*\s*stream\s*\)", src)
    assert re.search(r"\bint\s+rt_tri_overlaps_collect\s*\(\s*const\s+rt_accel\s*\*\s*as\s*,\s*const\s+rt_triangle\s*\*\s*queries\s*,"
                     r"\s*uint32_t\s+num_queries\s*,\s*uint32_t\s+flags\s*,\s*const\s+uint64_t\s*\*\s*offsets\s*,"
                     r"\s*uint32_t\s*\*\s*ids\s*,\s*uint32_t\s*\*\s*counts\s*,\s*uint64_t\s*\*\s*counters\s*,"
                     r"\s*uint32_t\s*\*\s*status\s*,\s*void\s*\*\s*stream\s*\)", src)
    assert "RT_TRI_SELF = 1" in src
    assert "RT_TRI_STACK_OVERFLOW = 1" in src and "RT_TRI_TRUNCATED = 2" in src


def test_exports_and_constants(rt):
    assert rt.kTriSelf == 1 and (rt.RT_TRI_STACK_OVERFLOW, rt.RT_TRI_TRUNCATED) == (1, 2)
    assert rt.TRIANGLE.itemsize == 36
    for name in ("rt_tri_overlaps_scratch_bytes", "rt_tri_overlaps_count", "rt_tri_overlaps_collect"):
        assert name in rt.EXPORTS
        getattr(rt.lib(), name)
    assert "trioverlap:" in rt.version()
    for f in (rt.TriOverlapsScratchBytes, rt.TriOverlapsCount, rt.TriOverlapsCollect, rt.TriOverlaps, rt.tri_overlap_status):
        assert callable(f)


def test_scratch_bytes(rt):
    # one uint64 per workgroup of 256 queries, 256-byte aligned, never 0: rt_range_scratch_bytes's rule
    assert rt.TriOverlapsScratchBytes(0) == 256 and rt.TriOverlapsScratchBytes(1) == 256
    assert rt.TriOverlapsScratchBytes(32 * 256) == 256 and rt.TriOverlapsScratchBytes(32 * 256 + 1) == 512
    assert rt.TriOverlapsScratchBytes(0xFFFFFFFF) == (1 << 24) * 8
    for n in (0, 1, 255, 256, 257, 1000, 1 << 20, (1 << 20) + 1, 1 << 28, 0xFFFFFFFF):
        assert rt.TriOverlapsScratchBytes(n) == rt.RangeScratchBytes(n)


def _accel(rt, count=2, nodes=FAKE, triangles=FAKE):
    return ctypes.byref(rt._Accel(triangles, nodes, 0, count))


def test_count_argument_errors(rt):
    L = rt.lib()

    def count(as_=None, queries=FAKE, n=5, flags=0, offsets=FAKE, scratch=FAKE, counters=None, status=None):
        return L.rt_tri_overlaps_count(_accel(rt) if as_ is None else as_, queries, n, flags, offsets, scratch, counters, status,
                                       None)

    assert L.rt_tri_overlaps_count(None, FAKE, 5, 0, FAKE, FAKE, None, None, None) == -1             # no accel
    assert count(queries=None) == -1 and count(offsets=None) == -1 and count(scratch=None) == -1
    assert count(as_=_accel(rt, nodes=0)) == -1 and count(as_=_accel(rt, triangles=0)) == -1         # a tree without nodes / leaves
    for c in (8, 9, 0xFFFFFFFF):
        assert count(as_=_accel(rt, count=c)) == -1
    for flags in (2, 3, 4, 0x80000000, 0xFFFFFFFF):
        assert count(flags=flags) == -1                                                              # unknown flag bits
    for off in (1, 2, 3):
        assert count(queries=FAKE + off) == -1 and count(status=FAKE + off) == -1                    # queries, status: 4 bytes
    assert count(offsets=FAKE_4) == -1                                                               # offsets: 8 bytes
    assert count(scratch=FAKE + 128) == -1                                                           # scratch: 256 bytes
    # errors win over an empty batch
    assert count(n=0, flags=2) == -1 and count(n=0, scratch=None) == -1 and count(n=0, as_=_accel(rt, count=8)) == -1


def test_collect_argument_errors(rt):
    L = rt.lib()

    def collect(as_=None, queries=FAKE, n=5, flags=0, offsets=FAKE, ids=FAKE, counts=None, counters=None, status=None):
        return L.rt_tri_overlaps_collect(_accel(rt) if as_ is None else as_, queries, n, flags, offsets, ids, counts, counters,
                                         status, None)

    assert L.rt_tri_overlaps_collect(None, FAKE, 5, 0, FAKE, FAKE, None, None, None, None) == -1
    assert collect(queries=None) == -1 and collect(offsets=None) == -1 and collect(ids=None) == -1
    assert collect(as_=_accel(rt, nodes=0)) == -1 and collect(as_=_accel(rt, triangles=0)) == -1
    for c in (8, 9, 0xFFFFFFFF):
        assert collect(as_=_accel(rt, count=c)) == -1
    for flags in (2, 3, 4, 0x80000000, 0xFFFFFFFF):
        assert collect(flags=flags) == -1
    assert collect(offsets=FAKE_4) == -1
    for off in (1, 2, 3):
        assert collect(queries=FAKE + off) == -1
        assert collect(ids=FAKE + off) == -1 and collect(counts=FAKE + off) == -1 and collect(status=FAKE + off) == -1
    # errors win over an empty batch; an empty batch with valid arguments does nothing and returns 0
    assert collect(n=0, flags=2) == -1 and collect(n=0, ids=None) == -1 and collect(n=0, counts=FAKE + 2) == -1
    assert collect(n=0) == 0 and collect(n=0, flags=1, queries=FAKE_4, counts=FAKE_4, counters=FAKE, status=FAKE_4) == 0
    # an empty tree needs no node or leaf pointer
    assert collect(n=0, as_=_accel(rt, count=0, nodes=0, triangles=0)) == 0
