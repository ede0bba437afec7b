"""CPU test of the all-hit ray-query ABI (rt_ray_hits_scratch_bytes, rt_ray_hits_count, rt_ray_hits_collect): the header
declares the entry points and the status flags, the library exports them, the Python names exist, and every argument error is
refused before any GPU work (the pointers below are never dereferenced: a correct library returns before it touches them)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000          # a 256-byte aligned "device pointer" that must never be used
FAKE_8 = FAKE + 8       # 8-byte aligned only
FAKE_4 = FAKE + 4       # 4-byte aligned only


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rt_abi.h")).read(), flags=re.S)


def test_header_declares_the_ray_hits_entry_points():
    src = _header()
    assert re.search(r"\bsize_t\s+rt_ray_hits_scratch_bytes\s*\(\s*uint32_t\s+num_rays\s*\)", src)
    assert re.search(r"\bint\s+rt_ray_hits_count\s*\(\s*const\s+rt_accel\s*\*\s*as\s*,\s*const\s+rt_ray\s*\*\s*rays\s*,"
                     r"\s*uint32_t\s+num_rays\s*,\s*uint64_t\s*\*\s*offsets\s*,\s*void\s*\*\s*scratch\s*,"
                     r"\s*uint64_t\s*\*\s*counters\s*,\s*uint32_t\s*\*\s*status\s*,\s*void\s*\*\s*stream\s*\)", src)
    assert re.search(r"\bint\s+rt_ray_hits_collect\s*\(\s*const\s+rt_accel\s*\*\s*as\s*,\s*const\s+rt_ray\s*\*\s*rays\s*,"
                     r"\s*uint32_t\s+num_rays\s*,\s*const\s+uint64_t\s*\*\s*offsets\s*,\s*rt_hit\s*\*\s*hits\s*,"
                     r"\s*uint32_t\s*\*\s*counts\s*,\s*uint64_t\s*\*\s*counters\s*,\s*uint32_t\s*\*\s*status\s*,"
                     r"\s*void\s*\*\s*stream\s*\)", src)
    assert "RT_RAY_HITS_STACK_OVERFLOW = 1" in src and "RT_RAY_HITS_TRUNCATED = 2" in src


def test_ray_hits_exports_and_python_names(rt):
    assert (rt.RT_RAY_HITS_STACK_OVERFLOW, rt.RT_RAY_HITS_TRUNCATED) == (1, 2)
    for name in ("rt_ray_hits_scratch_bytes", "rt_ray_hits_count", "rt_ray_hits_collect"):
        assert name in rt.EXPORTS
        getattr(rt.lib(), name)
    assert "rayhits:" in rt.version()
    for f in (rt.RayHitsScratchBytes, rt.RayHitsCount, rt.RayHitsCollect, rt.RayHits, rt.ray_hits_status):
        assert callable(f)


def test_scratch_bytes(rt):
    # one uint64 per workgroup of 256 rays, 256-byte aligned, never 0
    assert rt.RayHitsScratchBytes(0) == 256 and rt.RayHitsScratchBytes(1) == 256 and rt.RayHitsScratchBytes(8192) == 256
    assert rt.RayHitsScratchBytes(8193) == 512
    assert rt.RayHitsScratchBytes(0xFFFFFFFF) == (1 << 24) * 8
    sizes = [rt.RayHitsScratchBytes(n) for n in (0, 1, 1000, 8192, 8193, 1 << 20, 1 << 28, 0xFFFFFFFF)]
    assert all(s % 256 == 0 for s in sizes) and sizes == sorted(sizes)


def _accel(rt, count=2, nodes=FAKE, triangles=FAKE):
    return ctypes.byref(rt._Accel(triangles, nodes, 0, count))


def test_ray_hits_count_argument_errors(rt):
    L = rt.lib()

    def count(as_=None, rays=FAKE, n=5, offsets=FAKE, scratch=FAKE, counters=None, status=None):
        return L.rt_ray_hits_count(_accel(rt) if as_ is None else as_, rays, n, offsets, scratch, counters, status, None)

    assert L.rt_ray_hits_count(None, FAKE, 5, FAKE, FAKE, None, None, None) == -1                 # no accel
    assert count(rays=None) == -1 and count(offsets=None) == -1 and count(scratch=None) == -1
    assert count(as_=_accel(rt, nodes=0)) == -1 and count(as_=_accel(rt, triangles=0)) == -1      # a tree without nodes / leaves
    for c in (8, 9, 0xFFFFFFFF):
        assert count(as_=_accel(rt, count=c)) == -1
    assert count(rays=FAKE_8) == -1 and count(rays=FAKE_4) == -1                                  # rays: 16 bytes
    assert count(offsets=FAKE_4) == -1                                                            # offsets: 8 bytes
    assert count(scratch=FAKE + 128) == -1                                                        # scratch: 256 bytes
    for off in (1, 2, 3):
        assert count(status=FAKE + off) == -1                                                     # status: 4 bytes
    # errors win over an empty batch
    assert count(n=0, scratch=None) == -1 and count(n=0, as_=_accel(rt, count=8)) == -1 and count(n=0, offsets=FAKE_4) == -1


def test_ray_hits_collect_argument_errors(rt):
    L = rt.lib()

    def collect(as_=None, rays=FAKE, n=5, offsets=FAKE, hits=FAKE, counts=None, counters=None, status=None):
        return L.rt_ray_hits_collect(_accel(rt) if as_ is None else as_, rays, n, offsets, hits, counts, counters, status, None)

    assert L.rt_ray_hits_collect(None, FAKE, 5, FAKE, FAKE, None, None, None, None) == -1
    assert collect(rays=None) == -1 and collect(offsets=None) == -1 and collect(hits=None) == -1
    assert collect(as_=_accel(rt, nodes=0)) == -1 and collect(as_=_accel(rt, triangles=0)) == -1
    for c in (8, 9, 0xFFFFFFFF):
        assert collect(as_=_accel(rt, count=c)) == -1
    assert collect(rays=FAKE_8) == -1 and collect(hits=FAKE_8) == -1 and collect(hits=FAKE_4) == -1   # rays / hits: 16 bytes
    assert collect(offsets=FAKE_4) == -1
    for off in (1, 2, 3):
        assert collect(counts=FAKE + off) == -1 and collect(status=FAKE + off) == -1
    # errors win over an empty batch; an empty batch with valid arguments does nothing and returns 0
    assert collect(n=0, hits=None) == -1 and collect(n=0, counts=FAKE + 2) == -1 and collect(n=0, rays=FAKE_8) == -1
    assert collect(n=0) == 0 and collect(n=0, counts=FAKE_4, counters=FAKE, status=FAKE_4) == 0
    # an empty tree needs no node or leaf pointer
    assert collect(n=0, as_=_accel(rt, count=0, nodes=0, triangles=0)) == 0
