"""CPU test of the hit-filter ABI (rt_intersect_rays_filtered, rt_ray_hits_count_filtered, rt_ray_hits_collect_filtered,
rt_ray_first_hits_filtered): the header declares the four entry points, the flags and the two records, the library exports
them, the Python names exist, the records have the header's sizes, and every argument error -- the sibling's and the filter's
own -- is refused before any GPU work (the pointers below are never dereferenced: a correct library returns before it touches
them)."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000          # a 256-byte aligned "device pointer" that must never be used
NAMES = ("rt_intersect_rays_filtered", "rt_ray_hits_count_filtered", "rt_ray_hits_collect_filtered", "rt_ray_first_hits_filtered")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rt_abi.h")).read(), flags=re.S)


def _sig(*params):
    return r"\(\s*" + r"\s*,\s*".join(p.replace(" ", r"\s+").replace("*", r"\s*\*\s*") for p in params) + r"\s*\)"


def test_header_declares_the_entry_points():
    src = _header()
    flt = "const rt_hit_filter* filter"
    assert re.search(r"\bint\s+rt_intersect_rays_filtered\s*" + _sig(
        "const rt_accel* as", "const rt_ray* rays", "rt_hit* hits", "uint32_t num_rays", "int mode", "uint32_t num_primitives",
        flt, "uint64_t* counters", "void* stream"), src)
    assert re.search(r"\bint\s+rt_ray_hits_count_filtered\s*" + _sig(
        "const rt_accel* as", "const rt_ray* rays", "uint32_t num_rays", flt, "uint64_t* offsets", "void* scratch",
        "uint64_t* counters", "uint32_t* status", "void* stream"), src)
    assert re.search(r"\bint\s+rt_ray_hits_collect_filtered\s*" + _sig(
        "const rt_accel* as", "const rt_ray* rays", "uint32_t num_rays", flt, "const uint64_t* offsets", "rt_hit* hits",
        "uint32_t* counts", "uint64_t* counters", "uint32_t* status", "void* stream"), src)
    assert re.search(r"\bint\s+rt_ray_first_hits_filtered\s*" + _sig(
        "const rt_accel* as", "const rt_ray* rays", "uint32_t num_rays", "uint32_t k", flt, "rt_hit* out",
        "uint64_t* counters", "uint32_t* status", "void* stream"), src)
    assert "RT_FILTER_CULL_BACK = 1" in src and "RT_FILTER_CULL_FRONT = 2" in src
    assert re.search(r"typedef\s+struct\s+rt_ray_filter\s*\{\s*uint32_t\s+mask;\s*uint32_t\s+skip_id;\s*\}\s*rt_ray_filter;", src)
    assert re.search(r"typedef\s+struct\s+rt_hit_filter\s*\{\s*uint32_t\s+flags;\s*uint32_t\s+ray_mask;\s*uint32_t\s+num_primitives;"
                     r"\s*uint32_t\s+pad;\s*const\s+uint32_t\s*\*\s*prim_masks;\s*const\s+rt_ray_filter\s*\*\s*per_ray;\s*\}", src)


def test_exports_python_names_and_sizes(rt):
    for n in NAMES:
        assert n in rt.EXPORTS
        getattr(rt.lib(), n)
    assert (rt.RT_FILTER_CULL_BACK, rt.RT_FILTER_CULL_FRONT) == (1, 2)
    assert rt.RAY_FILTER.itemsize == 8 and rt.RAY_FILTER.names == ("mask", "skip_id")
    assert rt.RAY_FILTER.fields["skip_id"][1] == 4
    assert ctypes.sizeof(rt._HitFilter) == 32
    assert (rt._HitFilter.prim_masks.offset, rt._HitFilter.per_ray.offset) == (16, 24)
    assert "rayfilter:" in rt.version()
    for f in (rt.HitFilter, rt.IntersectRaysFiltered, rt.RayHitsCountFiltered, rt.RayHitsCollectFiltered, rt.RayFirstHitsFiltered):
        assert callable(f)
    f = rt.HitFilter()
    assert (f.flags, f.ray_mask, f.prim_masks, f.per_ray) == (0, 0xFFFFFFFF, None, None)


def _accel(rt, count=2, nodes=FAKE, triangles=FAKE):
    return ctypes.byref(rt._Accel(triangles, nodes, 0, count))


def _filter(rt, flags=0, ray_mask=0xFFFFFFFF, num_primitives=0, prim_masks=None, per_ray=None):
    return ctypes.byref(rt._HitFilter(flags, ray_mask, num_primitives, 0, prim_masks, per_ray))


def _calls(rt):
    """the four entry points as functions of (accel, filter, overrides): each returns the library's code"""
    L = rt.lib()

    def closest(as_, flt, rays=FAKE, hits=FAKE, n=5, mode=0, **_):
        return L.rt_intersect_rays_filtered(as_, rays, hits, n, mode, 0, flt, None, None)

    def count(as_, flt, rays=FAKE, n=5, offsets=FAKE, scratch=FAKE, status=None, **_):
        return L.rt_ray_hits_count_filtered(as_, rays, n, flt, offsets, scratch, None, status, None)

    def collect(as_, flt, rays=FAKE, n=5, offsets=FAKE, hits=FAKE, counts=None, status=None, **_):
        return L.rt_ray_hits_collect_filtered(as_, rays, n, flt, offsets, hits, counts, None, status, None)

    def first(as_, flt, rays=FAKE, n=5, k=4, hits=FAKE, counters=None, status=None, **_):
        return L.rt_ray_first_hits_filtered(as_, rays, n, k, flt, hits, counters, status, None)

    return {"closest": closest, "count": count, "collect": collect, "first": first}


@pytest.mark.parametrize("which", ("closest", "count", "collect", "first"))
def test_argument_errors(rt, which):
    call = _calls(rt)[which]
    ok = _filter(rt)
    # the filter's own: unknown flag bits, prim_masks not 4-byte aligned, per_ray not 8-byte aligned -- also for an empty batch
    for n in (5, 0):
        for flags in (4, 8, 0x80000000, 0xFFFFFFFF, 1 | 4):
            assert call(_accel(rt), _filter(rt, flags=flags), n=n) == -1
        for off in (1, 2, 3):
            assert call(_accel(rt), _filter(rt, num_primitives=9, prim_masks=FAKE + off), n=n) == -1
        for off in (1, 2, 4, 6):
            assert call(_accel(rt), _filter(rt, per_ray=FAKE + off), n=n) == -1
    # the sibling's, with a valid filter
    assert call(None, ok) == -1
    assert call(_accel(rt), ok, rays=None) == -1
    assert call(_accel(rt), ok, rays=FAKE + 8) == -1
    for c in (8, 0xFFFFFFFF):
        assert call(_accel(rt, count=c), ok) == -1
    assert call(_accel(rt, nodes=0), ok) == -1 and call(_accel(rt, triangles=0), ok) == -1
    if which == "closest":
        assert call(_accel(rt), ok, mode=2) == -1 and call(_accel(rt), ok, hits=FAKE + 8) == -1
    if which in ("count", "collect"):
        assert call(_accel(rt), ok, offsets=None) == -1 and call(_accel(rt), ok, offsets=FAKE + 4) == -1
        assert call(_accel(rt), ok, status=FAKE + 2) == -1
    if which == "count":
        assert call(_accel(rt), ok, scratch=None) == -1 and call(_accel(rt), ok, scratch=FAKE + 128) == -1
    if which == "collect":
        assert call(_accel(rt), ok, hits=None) == -1 and call(_accel(rt), ok, hits=FAKE + 8) == -1
        assert call(_accel(rt), ok, counts=FAKE + 2) == -1
    if which == "first":
        for k in (0, 33, 0xFFFFFFFF):
            assert call(_accel(rt), ok, k=k) == -1
        assert call(_accel(rt), ok, hits=None) == -1 and call(_accel(rt), ok, hits=FAKE + 8) == -1
        assert call(_accel(rt), ok, status=FAKE + 2) == -1 and call(_accel(rt), ok, counters=FAKE + 4) == -1
    # filter = NULL forwards to the unfiltered entry point: its errors come back
    assert call(None, None) == -1 and call(_accel(rt), None, rays=FAKE + 8) == -1 and call(_accel(rt, count=8), None) == -1
    # legal filters on an empty batch of the calls that then do nothing: both cull bits, num_primitives > 0 with a null
    # prim_masks, aligned arrays
    if which != "count":                                           # (the count call launches its scan for n = 0 too)
        for flt in (ok, None, _filter(rt, flags=3), _filter(rt, num_primitives=77), _filter(rt, flags=1, ray_mask=0, num_primitives=9,
                                                                                             prim_masks=FAKE + 4, per_ray=FAKE + 8)):
            assert call(_accel(rt), flt, n=0) == 0
        assert call(_accel(rt, count=0, nodes=0, triangles=0), ok, n=0) == 0


def test_binding_refuses_bad_filter_tensors(rt):
    import torch
    with pytest.raises(ValueError):
        rt.HitFilter(prim_masks=torch.zeros(7, dtype=torch.uint8))             # not 4-byte records
    with pytest.raises(ValueError):
        rt.HitFilter(per_ray=torch.zeros((5, 2), dtype=torch.int32)[:, :1])    # not contiguous
    with pytest.raises(ValueError):
        rt.HitFilter(per_ray=torch.zeros(3, dtype=torch.int32))                # not 8-byte records
    rays = torch.zeros((5, 8), dtype=torch.float32)            # host tensors: every check below comes before any pointer is used
    tri = nod = torch.zeros(64, dtype=torch.uint8)
    short = rt.HitFilter(per_ray=torch.zeros((4, 2), dtype=torch.int32))
    with pytest.raises(ValueError):
        rt.IntersectRaysFiltered(tri, nod, 0, 2, rays, torch.zeros((5, 4)), short)
    with pytest.raises(ValueError):
        rt.RayFirstHitsFiltered(tri, nod, 0, 2, rays, 2, short, torch.zeros((5, 2, 4)))
    with pytest.raises(ValueError):
        rt.RayHitsCollectFiltered(tri, nod, 0, 2, rays, short, torch.zeros(6, dtype=torch.int64), torch.zeros((9, 4)))
    with pytest.raises(ValueError):
        rt.RayFirstHitsFiltered(tri, nod, 0, 2, rays, 33, None, torch.zeros((5, 33, 4)))
    s = rt.HitFilter(flags=3, ray_mask=5, prim_masks=torch.zeros(9, dtype=torch.int32))._struct(5)
    assert (s.flags, s.ray_mask, s.num_primitives, s.pad, s.per_ray) == (3, 5, 9, 0, None)
    assert np.dtype(rt.RAY_FILTER).itemsize == 8
