"""CPU test of the instance-filter ABI (rt_intersect_rays_instanced_filtered): the header declares the entry point, the flags
and the three records, the library exports it, the Python names exist, the records have the header's sizes (8 / 16 / 32), and
every argument error -- the sibling's and the filter's own -- is refused before any GPU work (the pointers below are never
dereferenced: a correct library returns before it touches them)."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000          # a 256-byte aligned "device pointer" that must never be used
NAME = "rt_intersect_rays_instanced_filtered"


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rt_abi.h")).read(), flags=re.S)


def _sig(*params):
    return r"\(\s*" + r"\s*,\s*".join(p.replace(" ", r"\s+").replace("*", r"\s*\*\s*") for p in params) + r"\s*\)"


SIBLING = ("const rt_accel* tlas", "const rt_instance_record* records", "uint32_t num_instances", "const rt_accel* blas_table",
           "uint32_t num_blas", "const rt_ray* rays", "rt_hit* hits", "uint32_t* instance_ids", "uint32_t num_rays", "int mode",
           "uint32_t num_primitives")


def test_header_declares_the_entry_point():
    src = _header()
    # every argument of the sibling, unchanged in type and meaning, then filter, counters, stream
    assert re.search(r"\bint\s+rt_intersect_rays_instanced\s*" + _sig(*SIBLING, "uint64_t* counters", "void* stream"), src)
    assert re.search(r"\bint\s+" + NAME + r"\s*" + _sig(*SIBLING, "const rt_instance_hit_filter* filter", "uint64_t* counters",
                                                       "void* stream"), src)
    assert "RT_INSTANCE_FILTER_CULL_DISABLE = 1" in src and "RT_INSTANCE_FILTER_FLIP_FACING = 2" in src
    assert re.search(r"typedef\s+struct\s+rt_instance_filter\s*\{\s*uint32_t\s+mask;\s*uint32_t\s+flags;\s*\}\s*rt_instance_filter;",
                     src)
    assert re.search(r"typedef\s+struct\s+rt_instance_ray_filter\s*\{\s*uint32_t\s+mask;\s*uint32_t\s+skip_instance;\s*"
                     r"uint32_t\s+skip_id;\s*uint32_t\s+pad;\s*\}\s*rt_instance_ray_filter;", src)
    assert re.search(r"typedef\s+struct\s+rt_instance_hit_filter\s*\{\s*uint32_t\s+flags;\s*uint32_t\s+ray_mask;\s*"
                     r"uint32_t\s+num_instance_filters;\s*uint32_t\s+pad;\s*const\s+rt_instance_filter\s*\*\s*per_instance;\s*"
                     r"const\s+rt_instance_ray_filter\s*\*\s*per_ray;\s*\}\s*rt_instance_hit_filter;", src)
    # the hit-filter block no longer calls the instanced query out of scope
    full = open(os.path.join(ROOT, "include", "rt_abi.h")).read()
    assert "Out of scope: the instanced and indexed ray queries" not in full


def test_exports_python_names_and_sizes(rt):
    assert NAME in rt.EXPORTS
    getattr(rt.lib(), NAME)
    assert (rt.RT_INSTANCE_FILTER_CULL_DISABLE, rt.RT_INSTANCE_FILTER_FLIP_FACING) == (1, 2)
    assert rt.INSTANCE_FILTER.itemsize == 8 and rt.INSTANCE_FILTER.names == ("mask", "flags")
    assert rt.INSTANCE_RAY_FILTER.itemsize == 16
    assert rt.INSTANCE_RAY_FILTER.names == ("mask", "skip_instance", "skip_id", "pad")
    assert [rt.INSTANCE_RAY_FILTER.fields[n][1] for n in rt.INSTANCE_RAY_FILTER.names] == [0, 4, 8, 12]
    assert ctypes.sizeof(rt._InstanceHitFilter) == 32
    assert (rt._InstanceHitFilter.num_instance_filters.offset, rt._InstanceHitFilter.per_instance.offset,
            rt._InstanceHitFilter.per_ray.offset) == (8, 16, 24)
    assert "instancefilter:" in rt.version()
    assert callable(rt.InstanceHitFilter) and callable(rt.IntersectRaysInstancedFiltered)
    f = rt.InstanceHitFilter()
    assert (f.flags, f.ray_mask, f.per_instance, f.per_ray) == (0, 0xFFFFFFFF, None, None)


def _accel(rt, count=2, nodes=FAKE, triangles=FAKE):
    return ctypes.byref(rt._Accel(triangles, nodes, 0, count))


def _filter(rt, flags=0, ray_mask=0xFFFFFFFF, num=0, per_instance=None, per_ray=None):
    return ctypes.byref(rt._InstanceHitFilter(flags, ray_mask, num, 0, per_instance, per_ray))


def _call(rt, as_, flt, records=FAKE, num_instances=3, table=FAKE, num_blas=2, rays=FAKE, hits=FAKE, ids=FAKE, n=5, mode=0):
    return rt.lib().rt_intersect_rays_instanced_filtered(as_, records, num_instances, table, num_blas, rays, hits, ids, n, mode,
                                                         0, flt, None, None)


def test_argument_errors(rt):
    ok = _filter(rt)
    # the filter's own: unknown flag bits, per_instance not 8-byte aligned, per_ray not 16-byte aligned -- also for an empty batch
    for n in (5, 0):
        for flags in (4, 8, 0x80000000, 0xFFFFFFFF, 1 | 4):
            assert _call(rt, _accel(rt), _filter(rt, flags=flags), n=n) == -1
        for off in (1, 2, 4, 6):
            assert _call(rt, _accel(rt), _filter(rt, num=3, per_instance=FAKE + off), n=n) == -1
        for off in (1, 2, 4, 8, 12):
            assert _call(rt, _accel(rt), _filter(rt, per_ray=FAKE + off), n=n) == -1
    # the sibling's, with a valid filter and with none (NULL forwards to the unfiltered entry point: its errors come back)
    for flt in (ok, None):
        assert _call(rt, None, flt) == -1
        for name in ("rays", "hits", "ids"):
            assert _call(rt, _accel(rt), flt, **{name: None}) == -1
        assert _call(rt, _accel(rt), flt, rays=FAKE + 8) == -1 and _call(rt, _accel(rt), flt, hits=FAKE + 8) == -1
        assert _call(rt, _accel(rt), flt, ids=FAKE + 2) == -1
        assert _call(rt, _accel(rt), flt, records=FAKE + 8) == -1 and _call(rt, _accel(rt), flt, table=FAKE + 4) == -1
        assert _call(rt, _accel(rt), flt, records=None) == -1 and _call(rt, _accel(rt), flt, table=None) == -1
        assert _call(rt, _accel(rt), flt, num_blas=0) == -1
        for c in (8, 0xFFFFFFFF):
            assert _call(rt, _accel(rt, count=c), flt) == -1
        assert _call(rt, _accel(rt, nodes=0), flt) == -1 and _call(rt, _accel(rt, triangles=0), flt) == -1
        for mode in (2, -1):
            assert _call(rt, _accel(rt), flt, mode=mode) == -1
    # legal filters on an empty batch: both cull bits, num_instance_filters > 0 with a null per_instance, aligned arrays,
    # no instances at all (records and table may then be null)
    for flt in (ok, None, _filter(rt, flags=3), _filter(rt, num=77),
                _filter(rt, flags=1, ray_mask=0, num=9, per_instance=FAKE + 8, per_ray=FAKE + 16)):
        assert _call(rt, _accel(rt), flt, n=0) == 0
        assert _call(rt, _accel(rt), flt, n=0, num_instances=0, records=None, table=None, num_blas=0) == 0
    assert _call(rt, _accel(rt, count=0, nodes=0, triangles=0), ok, n=0) == 0


def test_binding_refuses_bad_filter_tensors(rt):
    import torch
    with pytest.raises(ValueError):
        rt.InstanceHitFilter(per_instance=torch.zeros(7, dtype=torch.int32))             # not 8-byte records
    with pytest.raises(ValueError):
        rt.InstanceHitFilter(per_instance=torch.zeros((5, 4), dtype=torch.int32)[:, :2])  # not contiguous
    with pytest.raises(ValueError):
        rt.InstanceHitFilter(per_ray=torch.zeros((5, 2), dtype=torch.int32)[:3])          # not 16-byte records
    with pytest.raises(ValueError):
        rt.InstanceHitFilter(per_ray=torch.zeros((5, 8), dtype=torch.int32)[:, :4])       # not contiguous
    rays = torch.zeros((5, 8), dtype=torch.float32)            # host tensors: every check below comes before any pointer is used
    tri = nod = rec = tab = torch.zeros(64, dtype=torch.uint8)
    hits, ids = torch.zeros((5, 4)), torch.zeros(5, dtype=torch.int32)
    short = rt.InstanceHitFilter(per_ray=torch.zeros((4, 4), dtype=torch.int32))
    with pytest.raises(ValueError):
        rt.IntersectRaysInstancedFiltered(tri, nod, 0, 2, rec, 1, tab, 1, rays, hits, ids, short)
    with pytest.raises(ValueError):                                                      # a single-tree HitFilter is another struct
        rt.IntersectRaysInstancedFiltered(tri, nod, 0, 2, rec, 1, tab, 1, rays, hits, ids, rt.HitFilter())
    with pytest.raises(ValueError):
        rt.IntersectRaysInstancedFiltered(tri, nod, 0, 2, rec, 1, tab, 1, rays, torch.zeros((4, 4)), ids, None)
    with pytest.raises(ValueError):
        rt.IntersectRaysInstancedFiltered(tri, nod, 0, 2, rec, 1, tab, 1, rays, hits, torch.zeros(4, dtype=torch.int32), None)
    with pytest.raises(ValueError):
        rt.IntersectRaysInstancedFiltered(tri, nod, 0, 2, rec, 1, tab, 1, torch.zeros((5, 7)), hits, ids, None)
    s = rt.InstanceHitFilter(flags=3, ray_mask=5, per_instance=torch.zeros((9, 2), dtype=torch.int32))._struct(5)
    assert (s.flags, s.ray_mask, s.num_instance_filters, s.pad, s.per_ray) == (3, 5, 9, 0, None)
    assert np.dtype(rt.INSTANCE_FILTER).itemsize == 8
