"""CPU test of the signed-distance / occupancy ABI (rt_signed_distance, rt_occupancy, rt_generate_grid_points): the header
declares the entry points, the record type, the limit and the flags, the library exports them, the dtype matches the struct
layout, and every argument error is refused before any GPU work (the device pointers below are never dereferenced: a correct
library returns before it touches them)."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000          # a 16-byte aligned "device pointer" that must never be used
FAKE_8 = FAKE + 8       # 8-byte aligned only


def _header(strip=True):
    src = open(os.path.join(ROOT, "include", "rt_abi.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S) if strip else src


def test_header_declares_the_sdf_entry_points():
    src = _header()
    common = (r"\s*\(\s*const\s+rt_accel\s*\*\s*as\s*,\s*const\s+rt_point_query\s*\*\s*queries\s*,\s*uint32_t\s+num_queries\s*,"
              r"\s*uint32_t\s+votes\s*,\s*const\s+float\s*\*\s*dirs\s*,\s*%s\s*,\s*uint64_t\s*\*\s*counters\s*,"
              r"\s*uint32_t\s*\*\s*status\s*,\s*void\s*\*\s*stream\s*\)")
    assert re.search(r"\bint\s+rt_signed_distance" + common % r"rt_sdf_hit\s*\*\s*out", src)
    assert re.search(r"\bint\s+rt_occupancy" + common % r"uint8_t\s*\*\s*inside", src)
    assert re.search(r"\bint\s+rt_generate_grid_points\s*\(\s*const\s+float\s+origin\[3\]\s*,\s*const\s+float\s+spacing\[3\]\s*,"
                     r"\s*const\s+uint32_t\s+dims\[3\]\s*,\s*float\s+dist2_max\s*,\s*int\s+layout\s*,"
                     r"\s*rt_point_query\s*\*\s*queries\s*,\s*void\s*\*\s*stream\s*\)", src)
    assert re.search(r"typedef\s+struct\s+rt_sdf_hit\s*\{\s*float\s+sdist;\s*uint32_t\s+primitive_id;\s*\}\s*rt_sdf_hit;", src)
    assert re.search(r"#define\s+RT_SDF_MAX_VOTES\s+3\b", src)
    assert "RT_SDF_STACK_OVERFLOW = 1" in src
    assert re.search(r"RT_GRID_ROW_MAJOR\s*=\s*0\s*,\s*RT_GRID_BRICKS\s*=\s*1", src)


def test_default_directions_match_the_header(rt):
    """the constants the header writes down are the binding's SDF_DEFAULT_DIRS"""
    src = _header(strip=False)
    for j in range(3):
        m = re.search(r"D%d\s*=\s*\(\s*(-?[0-9.]+)f\s*,\s*(-?[0-9.]+)f\s*,\s*(-?[0-9.]+)f\s*\)" % j, src)
        assert m, f"D{j} is not in the header"
        assert [np.float32(x) for x in m.groups()] == rt.SDF_DEFAULT_DIRS[j].tolist()
    d = np.abs(rt.SDF_DEFAULT_DIRS)
    assert rt.SDF_DEFAULT_DIRS.dtype == np.float32 and rt.SDF_DEFAULT_DIRS.shape == (3, 3)
    assert (d > 0).all() and all(len(set(row.tolist())) == 3 for row in d)       # not axis-aligned, no equal magnitudes


def test_sdf_layout_and_exports(rt):
    assert rt.SDF_HIT.itemsize == 8
    f = rt.SDF_HIT.fields
    assert (f["sdist"][1], f["primitive_id"][1]) == (0, 4)
    assert rt.RT_SDF_STACK_OVERFLOW == 1 and rt.RT_SDF_MAX_VOTES == 3 and (rt.kGridRowMajor, rt.kGridBricks) == (0, 1)
    for name in ("rt_signed_distance", "rt_occupancy", "rt_generate_grid_points"):
        assert name in rt.EXPORTS
        getattr(rt.lib(), name)
    assert "sdf:" in rt.version()
    for f in (rt.SignedDistance, rt.Occupancy, rt.sdf_status, rt.GridPointCount, rt.GenerateGridPoints):
        assert callable(f)
    assert rt.GridPointCount((5, 3, 9)) == 135 and rt.GridPointCount((5, 3, 9), bricks=True) == 2 * 1 * 3 * 64
    assert rt.GridPointCount((4, 0, 2)) == 0 and rt.GridPointCount((4, 0, 2), bricks=True) == 0


def _accel(rt, count=2, nodes=FAKE, triangles=FAKE):
    return ctypes.byref(rt._Accel(triangles, nodes, 0, count))


def test_signed_distance_and_occupancy_argument_errors(rt):
    L = rt.lib()
    dirs = (ctypes.c_float * 9)(*rt.SDF_DEFAULT_DIRS.reshape(-1).tolist())
    for f, out_align in ((L.rt_signed_distance, 8), (L.rt_occupancy, 1)):
        assert f(None, FAKE, 5, 3, None, FAKE, None, None, None) == -1                        # no accel
        assert f(_accel(rt), None, 5, 3, None, FAKE, None, None, None) == -1                 # no queries
        assert f(_accel(rt), FAKE, 5, 3, None, None, None, None, None) == -1                 # no out / inside
        for votes in (0, 2, 4, 5, 0xFFFFFFFF):
            assert f(_accel(rt), FAKE, 5, votes, None, FAKE, None, None, None) == -1         # votes not in {1, 3}
            assert f(_accel(rt), FAKE, 5, votes, dirs, FAKE, None, None, None) == -1
        assert f(_accel(rt, nodes=0), FAKE, 5, 3, None, FAKE, None, None, None) == -1        # a tree without nodes
        assert f(_accel(rt, triangles=0), FAKE, 5, 3, None, FAKE, None, None, None) == -1    # ... without leaves
        for count in (8, 9, 0xFFFFFFFF):
            assert f(_accel(rt, count=count), FAKE, 5, 3, None, FAKE, None, None, None) == -1
        assert f(_accel(rt), FAKE_8, 5, 3, None, FAKE, None, None, None) == -1               # queries not 16-byte aligned
        for off in (1, 2, 4):
            expect = -1 if off % out_align else 0
            assert f(_accel(rt), FAKE, 0, 3, None, FAKE + off, None, None, None) == expect   # out: 8-byte; inside: any
        for off in (1, 2, 3):
            assert f(_accel(rt), FAKE, 5, 3, None, FAKE, None, FAKE + off, None) == -1       # status not 4-byte aligned
        # errors win over an empty batch; an empty batch with valid arguments does nothing
        assert f(_accel(rt, count=8), FAKE, 0, 3, None, FAKE, None, None, None) == -1
        assert f(_accel(rt), FAKE, 0, 2, None, FAKE, None, None, None) == -1
        assert f(_accel(rt), FAKE, 0, 3, None, FAKE, None, FAKE + 2, None) == -1
        assert f(_accel(rt), FAKE_8, 0, 3, None, FAKE, None, None, None) == -1
        assert f(_accel(rt), FAKE, 0, 3, None, FAKE_8, None, None, None) == 0                # out: 8-byte alignment is enough
        for votes in (1, 3):
            assert f(_accel(rt), FAKE, 0, votes, None, FAKE, FAKE, FAKE + 4, None) == 0
            assert f(_accel(rt), FAKE, 0, votes, dirs, FAKE, FAKE, FAKE + 4, None) == 0
        # an empty tree needs no node or leaf pointer
        assert f(_accel(rt, count=0, nodes=0, triangles=0), FAKE, 0, 3, None, FAKE, None, None, None) == 0


def test_generate_grid_points_argument_errors(rt):
    f = rt.lib().rt_generate_grid_points
    o, s = (ctypes.c_float * 3)(0, 0, 0), (ctypes.c_float * 3)(1, 1, 1)
    dims = lambda *d: (ctypes.c_uint32 * 3)(*d)
    inf = float("inf")
    assert f(None, s, dims(2, 2, 2), inf, 0, FAKE, None) == -1
    assert f(o, None, dims(2, 2, 2), inf, 0, FAKE, None) == -1
    assert f(o, s, None, inf, 0, FAKE, None) == -1
    assert f(o, s, dims(2, 2, 2), inf, 0, None, None) == -1
    assert f(o, s, dims(2, 2, 2), inf, 0, FAKE_8, None) == -1                               # queries not 16-byte aligned
    for layout in (-1, 2, 7):
        assert f(o, s, dims(2, 2, 2), inf, layout, FAKE, None) == -1
    # a record count that does not fit 32 bits
    assert f(o, s, dims(65536, 65536, 1), inf, 0, FAKE, None) == -3
    assert f(o, s, dims(0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF), inf, 0, FAKE, None) == -3
    assert f(o, s, dims(0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF), inf, 1, FAKE, None) == -3
    assert f(o, s, dims(65536, 65536, 1), inf, 1, FAKE, None) == -3                         # 16384 * 16384 bricks of 64
    assert f(o, s, dims(1625, 1625, 1625), inf, 1, FAKE, None) == -3                        # 4.29e9 row-major fits; 407^3 * 64 does not
    # a lattice with a zero dimension runs nothing, whatever the other two are -- errors still win
    for layout in (0, 1):
        assert f(o, s, dims(0, 5, 5), inf, layout, FAKE, None) == 0
        assert f(o, s, dims(0xFFFFFFFF, 0, 0xFFFFFFFF), inf, layout, FAKE, None) == 0
        assert f(o, s, dims(5, 5, 0), inf, layout, FAKE_8, None) == -1
