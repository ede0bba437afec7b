"""CPU test of the first-K ray-query ABI (rt_ray_first_hits): the header declares the entry point, the limit and the status
flag, the library exports it, the Python names exist, every argument error is refused before any GPU work (the pointers below
are never dereferenced: a correct library returns before it touches them), and the binding refuses a wrong k or shape."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000          # a 256-byte aligned "device pointer" that must never be used
FAKE_8 = FAKE + 8       # 8-byte aligned only
FAKE_4 = FAKE + 4       # 4-byte aligned only


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rt_abi.h")).read(), flags=re.S)


def test_header_declares_the_entry_point():
    src = _header()
    assert re.search(r"\bint\s+rt_ray_first_hits\s*\(\s*const\s+rt_accel\s*\*\s*as\s*,\s*const\s+rt_ray\s*\*\s*rays\s*,"
                     r"\s*uint32_t\s+num_rays\s*,\s*uint32_t\s+k\s*,\s*rt_hit\s*\*\s*out\s*,\s*uint64_t\s*\*\s*counters\s*,"
                     r"\s*uint32_t\s*\*\s*status\s*,\s*void\s*\*\s*stream\s*\)", src)
    assert re.search(r"#define\s+RT_RAY_FIRST_MAX_K\s+32\b", src) and "RT_RAY_FIRST_STACK_OVERFLOW = 1" in src


def test_exports_and_python_names(rt):
    assert (rt.RT_RAY_FIRST_MAX_K, rt.RT_RAY_FIRST_STACK_OVERFLOW) == (32, 1)
    assert "rt_ray_first_hits" in rt.EXPORTS
    getattr(rt.lib(), "rt_ray_first_hits")
    assert "rayfirst:" in rt.version()
    assert callable(rt.RayFirstHits) and callable(rt.ray_first_status)


def _accel(rt, count=2, nodes=FAKE, triangles=FAKE):
    return ctypes.byref(rt._Accel(triangles, nodes, 0, count))


def test_argument_errors(rt):
    L = rt.lib()

    def first(as_=None, rays=FAKE, n=5, k=4, out=FAKE, counters=None, status=None):
        return L.rt_ray_first_hits(_accel(rt) if as_ is None else as_, rays, n, k, out, counters, status, None)

    assert L.rt_ray_first_hits(None, FAKE, 5, 4, FAKE, None, None, None) == -1                    # no accel
    assert first(rays=None) == -1 and first(out=None) == -1
    for k in (0, 33, 64, 0xFFFFFFFF):
        assert first(k=k) == -1                                                                   # k outside 1 .. 32
    for c in (8, 9, 0xFFFFFFFF):
        assert first(as_=_accel(rt, count=c)) == -1                                               # count > 7
    assert first(as_=_accel(rt, nodes=0)) == -1 and first(as_=_accel(rt, triangles=0)) == -1      # a tree without nodes / leaves
    assert first(rays=FAKE_8) == -1 and first(rays=FAKE_4) == -1                                  # rays: 16 bytes
    assert first(out=FAKE_8) == -1 and first(out=FAKE_4) == -1                                    # out: 16 bytes
    for off in (1, 2, 3):
        assert first(status=FAKE + off) == -1                                                     # status: 4 bytes
    for off in (1, 2, 4, 6):
        assert first(counters=FAKE + off) == -1                                                   # counters: 8 bytes
    # errors win over an empty batch; an empty batch with valid arguments does nothing and returns 0
    assert first(n=0, out=None) == -1 and first(n=0, k=0) == -1 and first(n=0, k=33) == -1 and first(n=0, rays=FAKE_8) == -1
    assert first(n=0, as_=_accel(rt, count=8)) == -1 and first(n=0, status=FAKE + 2) == -1 and first(n=0, counters=FAKE_4) == -1
    assert first(n=0) == 0 and first(n=0, k=1) == 0 and first(n=0, k=32, counters=FAKE_8, status=FAKE_4) == 0
    # an empty tree needs no node or leaf pointer
    assert first(n=0, as_=_accel(rt, count=0, nodes=0, triangles=0)) == 0


def test_binding_refuses_a_wrong_k_or_shape(rt):
    import torch
    rays = torch.zeros((5, 8), dtype=torch.float32)           # host tensors: every check below comes before any pointer is used
    tri = nod = torch.zeros(64, dtype=torch.uint8)

    def call(k, out, r=rays):
        return rt.RayFirstHits(tri, nod, 0, 2, r, k, out)

    for k in (0, -1, 33, 1000):
        with pytest.raises(ValueError):
            call(k, torch.zeros((5, max(k, 1), 4)))
    for shape in ((5, 3, 4), (5, 4, 3), (4, 4, 4), (6, 4, 4), (5, 16), (80,)):
        with pytest.raises(ValueError):
            call(4, torch.zeros(shape))
    with pytest.raises(ValueError):
        call(4, torch.zeros((5, 4, 4), dtype=torch.float64))
    with pytest.raises(ValueError):
        call(4, torch.zeros((5, 4, 8))[:, :, ::2])            # not contiguous
    with pytest.raises(ValueError):
        call(4, torch.zeros((5, 4, 4)), torch.zeros((5, 7)))  # rays: not 32-byte records
    assert call(4, torch.zeros((0, 4, 4)), torch.zeros((0, 8))) == 0      # an empty batch: nothing runs
