"""CPU test of the closest-point ABI (rt_closest_points): the header declares the entry point, the two record types and the
status flag, the library exports it, the dtypes match the struct layouts, and every argument error is refused before any GPU
work (the pointers below are never dereferenced: a correct library returns before it touches them)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000          # a 16-byte aligned "device pointer" that must never be used
FAKE_ODD = FAKE + 8     # 8-byte aligned only


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rt_abi.h")).read(), flags=re.S)


def test_header_declares_the_point_query_entry_point():
    src = _header()
    assert re.search(r"\bint\s+rt_closest_points\s*\(\s*const\s+rt_accel\s*\*\s*as\s*,\s*const\s+rt_point_query\s*\*\s*queries\s*,"
                     r"\s*rt_point_hit\s*\*\s*hits\s*,\s*uint32_t\s+num_queries\s*,\s*uint64_t\s*\*\s*counters\s*,"
                     r"\s*uint32_t\s*\*\s*status\s*,\s*void\s*\*\s*stream\s*\)", src)
    assert re.search(r"typedef\s+struct\s+rt_point_query\s*\{\s*rt_float3\s+p;\s*float\s+dist2_max;\s*\}\s*rt_point_query;", src)
    assert re.search(r"typedef\s+struct\s+rt_point_hit\s*\{\s*float\s+dist2;\s*uint32_t\s+primitive_id;\s*float\s+u,\s*v;\s*\}"
                     r"\s*rt_point_hit;", src)
    assert "RT_POINT_STACK_OVERFLOW = 1" in src


def test_point_layouts_and_exports(rt):
    assert rt.POINT_QUERY.itemsize == 16 and rt.POINT_HIT.itemsize == 16
    f = rt.POINT_QUERY.fields
    assert (f["p"][1], f["dist2_max"][1]) == (0, 12)
    f = rt.POINT_HIT.fields
    assert (f["dist2"][1], f["primitive_id"][1], f["u"][1], f["v"][1]) == (0, 4, 8, 12)
    assert rt.RT_POINT_STACK_OVERFLOW == 1
    assert "rt_closest_points" in rt.EXPORTS
    getattr(rt.lib(), "rt_closest_points")
    assert "points:" in rt.version()
    assert callable(rt.ClosestPoints) and callable(rt.point_status)


def _accel(rt, count=2, nodes=FAKE, triangles=FAKE):
    return ctypes.byref(rt._Accel(triangles, nodes, 0, count))


def test_closest_points_argument_errors(rt):
    L = rt.lib()
    assert L.rt_closest_points(None, FAKE, FAKE, 5, None, None, None) == -1                       # no accel
    assert L.rt_closest_points(_accel(rt), None, FAKE, 5, None, None, None) == -1                # no queries
    assert L.rt_closest_points(_accel(rt), FAKE, None, 5, None, None, None) == -1                # no hits
    assert L.rt_closest_points(_accel(rt, nodes=0), FAKE, FAKE, 5, None, None, None) == -1       # a tree without nodes
    assert L.rt_closest_points(_accel(rt, triangles=0), FAKE, FAKE, 5, None, None, None) == -1   # ... without leaves
    for count in (8, 9, 0xFFFFFFFF):
        assert L.rt_closest_points(_accel(rt, count=count), FAKE, FAKE, 5, None, None, None) == -1
    assert L.rt_closest_points(_accel(rt), FAKE_ODD, FAKE, 5, None, None, None) == -1            # queries not 16-byte aligned
    assert L.rt_closest_points(_accel(rt), FAKE, FAKE_ODD, 5, None, None, None) == -1            # hits not 16-byte aligned
    for off in (1, 2, 3):
        assert L.rt_closest_points(_accel(rt), FAKE, FAKE, 5, None, FAKE + off, None) == -1      # status not 4-byte aligned
    # errors win over an empty batch; an empty batch with valid arguments does nothing
    assert L.rt_closest_points(_accel(rt, count=8), FAKE, FAKE, 0, None, None, None) == -1
    assert L.rt_closest_points(_accel(rt), FAKE, FAKE, 0, None, FAKE + 2, None) == -1
    assert L.rt_closest_points(_accel(rt), FAKE, FAKE, 0, None, None, None) == 0
    assert L.rt_closest_points(_accel(rt), FAKE, FAKE, 0, FAKE, FAKE + 4, None) == 0
    # an empty tree needs no node or leaf pointer
    assert L.rt_closest_points(_accel(rt, count=0, nodes=0, triangles=0), FAKE, FAKE, 0, None, None, None) == 0
