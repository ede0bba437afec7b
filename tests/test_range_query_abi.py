"""CPU test of the range-query ABI (rt_range_scratch_bytes, rt_range_count, rt_range_collect): the header declares the entry
points, the box record, the shapes and the status flags, the library exports them, the dtypes match the struct layouts, and
every argument error is refused before any GPU work (the pointers below are never dereferenced: a correct library returns
before it touches them)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000          # a 256-byte aligned "device pointer" that must never be used
FAKE_8 = FAKE + 8       # 8-byte aligned only
FAKE_4 = FAKE + 4       # 4-byte aligned only


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rt_abi.h")).read(), flags=re.S)


def test_header_declares_the_range_entry_points():
    src = _header()
    assert re.search(r"\bsize_t\s+rt_range_scratch_bytes\s*\(\s*uint32_t\s+num_queries\s*\)", src)
    assert re.search(r"\bint\s+rt_range_count\s*\(\s*const\s+rt_accel\s*\*\s*as\s*,\s*const\s+void\s*\*\s*queries\s*,"
                     r"\s*uint32_t\s+num_queries\s*,\s*int\s+shape\s*,\s*uint64_t\s*\*\s*offsets\s*,\s*void\s*\*\s*scratch\s*,"
                     r"\s*uint64_t\s*\*\s*counters\s*,\s*uint32_t\s*\*\s*status\s*,\s*void\s*\*\s*stream\s*\)", src)
    assert re.search(r"\bint\s+rt_range_collect\s*\(\s*const\s+rt_accel\s*\*\s*as\s*,\s*const\s+void\s*\*\s*queries\s*,"
                     r"\s*uint32_t\s+num_queries\s*,\s*int\s+shape\s*,\s*const\s+uint64_t\s*\*\s*offsets\s*,"
                     r"\s*uint32_t\s*\*\s*ids\s*,\s*uint32_t\s*\*\s*counts\s*,\s*uint64_t\s*\*\s*counters\s*,"
                     r"\s*uint32_t\s*\*\s*status\s*,\s*void\s*\*\s*stream\s*\)", src)
    assert re.search(r"typedef\s+struct\s+rt_range_box\s*\{\s*rt_float3\s+lo;\s*uint32_t\s+pad0;\s*rt_float3\s+hi;\s*uint32_t\s+pad1;"
                     r"\s*\}\s*rt_range_box;", src)
    assert "RT_RANGE_SPHERE = 0" in src and "RT_RANGE_BOX = 1" in src
    assert "RT_RANGE_STACK_OVERFLOW = 1" in src and "RT_RANGE_TRUNCATED = 2" in src


def test_range_layouts_and_exports(rt):
    assert rt.RANGE_BOX.itemsize == 32
    f = rt.RANGE_BOX.fields
    assert (f["lo"][1], f["pad0"][1], f["hi"][1], f["pad1"][1]) == (0, 12, 16, 28)
    assert (rt.kRangeSphere, rt.kRangeBox) == (0, 1)
    assert (rt.RT_RANGE_STACK_OVERFLOW, rt.RT_RANGE_TRUNCATED) == (1, 2)
    for name in ("rt_range_scratch_bytes", "rt_range_count", "rt_range_collect"):
        assert name in rt.EXPORTS
        getattr(rt.lib(), name)
    assert "range:" in rt.version()
    for f in (rt.RangeScratchBytes, rt.RangeCount, rt.RangeCollect, rt.RangeQuery, rt.range_status):
        assert callable(f)


def test_scratch_bytes(rt):
    # one uint64 per workgroup of 256 queries, 256-byte aligned, never 0
    assert rt.RangeScratchBytes(0) == 256 and rt.RangeScratchBytes(1) == 256 and rt.RangeScratchBytes(32 * 256) == 256
    assert rt.RangeScratchBytes(32 * 256 + 1) == 512
    assert rt.RangeScratchBytes(0xFFFFFFFF) == (1 << 24) * 8
    sizes = [rt.RangeScratchBytes(n) for n in (0, 1000, 1 << 20, 1 << 28)]
    assert all(s % 256 == 0 for s in sizes) and sizes == sorted(sizes)


def _accel(rt, count=2, nodes=FAKE, triangles=FAKE):
    return ctypes.byref(rt._Accel(triangles, nodes, 0, count))


def test_range_count_argument_errors(rt):
    L = rt.lib()

    def count(as_=None, queries=FAKE, n=5, shape=0, offsets=FAKE, scratch=FAKE, counters=None, status=None):
        return L.rt_range_count(_accel(rt) if as_ is None else as_, queries, n, shape, offsets, scratch, counters, status, None)

    assert L.rt_range_count(None, FAKE, 5, 0, FAKE, FAKE, None, None, None) == -1                 # no accel
    assert count(queries=None) == -1 and count(offsets=None) == -1 and count(scratch=None) == -1
    assert count(as_=_accel(rt, nodes=0)) == -1 and count(as_=_accel(rt, triangles=0)) == -1      # a tree without nodes / leaves
    for c in (8, 9, 0xFFFFFFFF):
        assert count(as_=_accel(rt, count=c)) == -1
    for shape in (-1, 2, 7):
        assert count(shape=shape) == -1
    assert count(queries=FAKE_8) == -1 and count(queries=FAKE_8, shape=1) == -1                   # queries: 16 bytes
    assert count(offsets=FAKE_4) == -1                                                            # offsets: 8 bytes
    assert count(scratch=FAKE + 128) == -1                                                        # scratch: 256 bytes
    for off in (1, 2, 3):
        assert count(status=FAKE + off) == -1                                                     # status: 4 bytes
    # errors win over an empty batch
    assert count(n=0, shape=3) == -1 and count(n=0, scratch=None) == -1 and count(n=0, as_=_accel(rt, count=8)) == -1


def test_range_collect_argument_errors(rt):
    L = rt.lib()

    def collect(as_=None, queries=FAKE, n=5, shape=0, offsets=FAKE, ids=FAKE, counts=None, counters=None, status=None):
        return L.rt_range_collect(_accel(rt) if as_ is None else as_, queries, n, shape, offsets, ids, counts, counters,
                                  status, None)

    assert L.rt_range_collect(None, FAKE, 5, 0, FAKE, FAKE, None, None, None, None) == -1
    assert collect(queries=None) == -1 and collect(offsets=None) == -1 and collect(ids=None) == -1
    assert collect(as_=_accel(rt, nodes=0)) == -1 and collect(as_=_accel(rt, triangles=0)) == -1
    for c in (8, 9, 0xFFFFFFFF):
        assert collect(as_=_accel(rt, count=c)) == -1
    for shape in (-1, 2, 7):
        assert collect(shape=shape) == -1
    assert collect(queries=FAKE_8) == -1 and collect(offsets=FAKE_4) == -1
    for off in (1, 2, 3):
        assert collect(ids=FAKE + off) == -1 and collect(counts=FAKE + off) == -1 and collect(status=FAKE + off) == -1
    # errors win over an empty batch; an empty batch with valid arguments does nothing and returns 0
    assert collect(n=0, shape=2) == -1 and collect(n=0, ids=None) == -1 and collect(n=0, counts=FAKE + 2) == -1
    assert collect(n=0) == 0 and collect(n=0, shape=1, counts=FAKE_4, counters=FAKE, status=FAKE_4) == 0
    # an empty tree needs no node or leaf pointer
    assert collect(n=0, as_=_accel(rt, count=0, nodes=0, triangles=0)) == 0
