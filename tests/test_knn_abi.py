"""CPU test of the k-nearest ABI (rt_k_nearest): the header declares the entry point, the record type, the limit and the status
flag, the library exports it, the dtype matches the struct layout, and every argument error is refused before any GPU work
(the pointers below are never dereferenced: a correct library returns before it touches them)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000          # a 16-byte aligned "device pointer" that must never be used
FAKE_8 = FAKE + 8       # 8-byte aligned only


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rt_abi.h")).read(), flags=re.S)


def test_header_declares_the_k_nearest_entry_point():
    src = _header()
    assert re.search(r"\bint\s+rt_k_nearest\s*\(\s*const\s+rt_accel\s*\*\s*as\s*,\s*const\s+rt_point_query\s*\*\s*queries\s*,"
                     r"\s*uint32_t\s+num_queries\s*,\s*uint32_t\s+k\s*,\s*rt_knn_hit\s*\*\s*out\s*,\s*uint64_t\s*\*\s*counters\s*,"
                     r"\s*uint32_t\s*\*\s*status\s*,\s*void\s*\*\s*stream\s*\)", src)
    assert re.search(r"typedef\s+struct\s+rt_knn_hit\s*\{\s*float\s+dist2;\s*uint32_t\s+primitive_id;\s*\}\s*rt_knn_hit;", src)
    assert re.search(r"#define\s+RT_KNN_MAX_K\s+32\b", src)
    assert "RT_KNN_STACK_OVERFLOW = 1" in src


def test_knn_layout_and_exports(rt):
    assert rt.KNN_HIT.itemsize == 8
    f = rt.KNN_HIT.fields
    assert (f["dist2"][1], f["primitive_id"][1]) == (0, 4)
    assert rt.RT_KNN_STACK_OVERFLOW == 1 and rt.RT_KNN_MAX_K == 32
    assert "rt_k_nearest" in rt.EXPORTS
    getattr(rt.lib(), "rt_k_nearest")
    assert "knn:" in rt.version()
    assert callable(rt.KNearest) and callable(rt.knn_status)


def _accel(rt, count=2, nodes=FAKE, triangles=FAKE):
    return ctypes.byref(rt._Accel(triangles, nodes, 0, count))


def test_k_nearest_argument_errors(rt):
    L = rt.lib()
    f = L.rt_k_nearest
    assert f(None, FAKE, 5, 4, FAKE, None, None, None) == -1                        # no accel
    assert f(_accel(rt), None, 5, 4, FAKE, None, None, None) == -1                 # no queries
    assert f(_accel(rt), FAKE, 5, 4, None, None, None, None) == -1                 # no out
    for k in (0, 33, 64, 0xFFFFFFFF):
        assert f(_accel(rt), FAKE, 5, k, FAKE, None, None, None) == -1             # k = 0 or k > RT_KNN_MAX_K
    assert f(_accel(rt, nodes=0), FAKE, 5, 4, FAKE, None, None, None) == -1        # a tree without nodes
    assert f(_accel(rt, triangles=0), FAKE, 5, 4, FAKE, None, None, None) == -1    # ... without leaves
    for count in (8, 9, 0xFFFFFFFF):
        assert f(_accel(rt, count=count), FAKE, 5, 4, FAKE, None, None, None) == -1
    assert f(_accel(rt), FAKE_8, 5, 4, FAKE, None, None, None) == -1               # queries not 16-byte aligned
    for off in (1, 2, 4):
        assert f(_accel(rt), FAKE, 5, 4, FAKE + off, None, None, None) == -1       # out not 8-byte aligned
    for off in (1, 2, 3):
        assert f(_accel(rt), FAKE, 5, 4, FAKE, None, FAKE + off, None) == -1       # status not 4-byte aligned
    # errors win over an empty batch; an empty batch with valid arguments does nothing
    assert f(_accel(rt, count=8), FAKE, 0, 4, FAKE, None, None, None) == -1
    assert f(_accel(rt), FAKE, 0, 0, FAKE, None, None, None) == -1
    assert f(_accel(rt), FAKE, 0, 33, FAKE, None, None, None) == -1
    assert f(_accel(rt), FAKE, 0, 4, FAKE, None, FAKE + 2, None) == -1
    assert f(_accel(rt), FAKE, 0, 4, FAKE_8, None, None, None) == 0                # out: 8-byte alignment is enough
    for k in (1, 32):
        assert f(_accel(rt), FAKE, 0, k, FAKE, FAKE, FAKE + 4, None) == 0
    # an empty tree needs no node or leaf pointer
    assert f(_accel(rt, count=0, nodes=0, triangles=0), FAKE, 0, 4, FAKE, None, None, None) == 0
