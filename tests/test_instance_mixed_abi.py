"""CPU test of the mixed-instancing ABI (rt_intersect_rays_instanced_mixed): the header declares the entry point and rt_geometry,
the library exports it, the record is the 16 bytes the binding's dtype says, every argument error is refused before any GPU
work (the pointers below are never dereferenced: a correct library returns before it touches them), geom_table == NULL reaches
the sibling's argument checks, and the Python wrapper refuses bad buffers."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000          # a 16-byte aligned "device pointer" that must never be used


def _header():
    return open(os.path.join(ROOT, "include", "rt_abi.h")).read()


def test_header_declares_the_entry_point(rt):
    h = _header()
    src = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    assert re.search(r"\bint\s+rt_intersect_rays_instanced_mixed\s*\(\s*const\s+rt_accel\s*\*", src)
    assert re.search(r"enum\s*\{\s*RT_GEOM_TRIANGLES\s*=\s*0\s*,\s*RT_GEOM_SPHERES\s*=\s*1\s*\}", src)
    assert "rt_intersect_rays_instanced_mixed" in rt.EXPORTS and rt.lib().rt_intersect_rays_instanced_mixed is not None
    assert (rt.RT_GEOM_TRIANGLES, rt.RT_GEOM_SPHERES) == (0, 1)
    for name in ("IntersectRaysInstancedMixed", "geometry_table"):
        assert callable(getattr(rt, name)), name
    assert "instance_mixed:" in rt.version()
    # the block sits after the sphere block and says what it must
    assert h.index("---- sphere primitives") < h.index("---- mixed instancing") < h.index("---- closest-point queries")
    block = h[h.index("---- mixed instancing"):h.index("enum { RT_GEOM_TRIANGLES")]
    for words in ("NO num_primitives hint", "pair-prefetch", "ONE 16-byte load", "NOT ENTERED", "data is null",
                  "count == 0 enters the instance and tests nothing", "id >= count", "ellipsoid", "One tmax",
                  "first accepted primitive of either kind", "geom_table == NULL", "16-byte aligned", "Out of scope",
                  "filtered, motion, indexed, all-hit and first-K", "inside one BLAS", "rt_cli"):
        assert words in block, words
    # the sphere block no longer lists spheres under a TLAS as out of scope: it points here
    sphere = h[h.index("---- sphere primitives"):h.index("typedef struct rt_sphere")]
    out = sphere[sphere.index("Out of scope"):]
    assert "BLAS kind" not in out and "mixed-instancing block" in sphere


def test_struct_layout(rt):
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    body = re.search(r"typedef struct rt_geometry \{(.*?)\} rt_geometry;", src, flags=re.S).group(1)
    assert re.sub(r"\s+", " ", body).strip() == "const void* data; uint32_t count; uint32_t kind;"
    f = rt.GEOMETRY.fields
    assert rt.GEOMETRY.itemsize == 16                                                # sizeof(rt_geometry)
    assert (f["data"][1], f["count"][1], f["kind"][1]) == (0, 8, 12)

    class Geometry(ctypes.Structure):                                                # the C layout on this ABI
        _fields_ = [("data", ctypes.c_void_p), ("count", ctypes.c_uint32), ("kind", ctypes.c_uint32)]
    assert ctypes.sizeof(Geometry) == 16 and (Geometry.data.offset, Geometry.count.offset, Geometry.kind.offset) == (0, 8, 12)


def _call(rt, fn="rt_intersect_rays_instanced_mixed", tlas_count=2, tlas_nodes=FAKE, tlas_tris=FAKE, rec=FAKE, n_inst=3, table=FAKE,
          geom=FAKE, nb=2, rays=FAKE, hits=FAKE, ids=FAKE, n=5, mode=0, tlas=True):
    a = ctypes.byref(rt._Accel(tlas_tris, tlas_nodes, 0, tlas_count)) if tlas else None
    return rt.lib().rt_intersect_rays_instanced_mixed(a, rec, n_inst, table, geom, nb, rays, hits, ids, n, mode, None, None)


@pytest.mark.parametrize("geom", (FAKE, None), ids=("table", "null-table"))
def test_argument_errors(rt, geom):
    """the sibling's errors, with a table and with geom_table == NULL (the call forwards to rt_intersect_rays_instanced, whose
    checks refuse the same arguments)"""
    def call(**kw):
        return _call(rt, geom=geom, **kw)

    assert call(tlas=False) == -1
    assert call(tlas_count=8) == -1
    assert call(tlas_nodes=0) == -1
    assert call(tlas_tris=0) == -1
    for k in ("rec", "table", "rays", "hits", "ids"):
        assert call(**{k: None}) == -1, k
    for k in ("rec", "rays", "hits"):
        assert call(**{k: FAKE + 8}) == -1, k                # not 16-byte aligned
    assert call(table=FAKE + 4) == -1                        # not 8-byte aligned
    assert call(ids=FAKE + 2) == -1                          # not 4-byte aligned
    for mode in (-1, 2, 7):
        assert call(mode=mode) == -1
        assert call(mode=mode, n=0) == -1
    assert call(nb=0) == -1                                  # instances but no BLAS
    # errors win over an empty batch; an empty batch with valid arguments does nothing
    assert call(n=0, tlas_count=8) == -1
    assert call(n=0, nb=0) == -1
    assert call(n=0) == 0
    assert call(n=0, mode=1) == 0
    # an empty scene (no instances, an empty TLAS): arguments are valid, nothing is read
    assert call(n=0, n_inst=0, table=None, nb=0, rec=None, tlas_count=0, tlas_nodes=0, tlas_tris=0) == 0


def test_geometry_table_alignment(rt):
    for bad in (FAKE + 8, FAKE + 4, FAKE + 1):
        assert _call(rt, geom=bad) == -1, bad
        assert _call(rt, geom=bad, n=0) == -1, bad           # errors win over an empty batch
    assert _call(rt, geom=FAKE, n=0) == 0


def test_python_wrapper_refuses_bad_buffers(rt):
    import torch
    rays = torch.zeros((4, 8), dtype=torch.float32)
    hits = torch.zeros((4, 4), dtype=torch.float32)
    ids = torch.zeros(4, dtype=torch.int32)
    geom = torch.zeros(2 * 16, dtype=torch.uint8)
    buf = torch.zeros(256, dtype=torch.uint8)

    def query(**kw):
        a = dict(rays=rays, hits=hits, ids=ids, geom=geom)
        a.update(kw)
        rt.IntersectRaysInstancedMixed(buf, buf, 0, 2, buf, 3, buf, a["geom"], 2, a["rays"], a["hits"], a["ids"])

    for bad in (dict(hits=hits[:3]), dict(hits=torch.zeros((4, 8))[:, ::2]), dict(rays=torch.zeros((4, 16))[:, ::2]),
                dict(rays=torch.zeros(33, dtype=torch.uint8)), dict(ids=ids[:3]), dict(ids=torch.zeros(8, dtype=torch.int32)[::2]),
                dict(geom=geom[:31]), dict(geom=torch.zeros(64, dtype=torch.uint8)[::2])):
        with pytest.raises(ValueError):
            query(**bad)
    # an empty batch returns before the library is called
    rt.IntersectRaysInstancedMixed(buf, buf, 0, 2, buf, 3, buf, geom, 2, rays[:0], hits, ids)
    # geometry_table: an entry per BLAS, None for triangles, (spheres, count) for spheres; a short sphere buffer is refused
    sph = torch.zeros((3, 4), dtype=torch.float32)
    tab = rt.geometry_table([None, (sph, 3), (sph, 0)], device="cpu")
    got = tab.numpy().view(rt.GEOMETRY).reshape(-1)
    assert got["kind"].tolist() == [0, 1, 1] and got["count"].tolist() == [0, 3, 0]
    assert got["data"].tolist() == [0, sph.data_ptr(), sph.data_ptr()]
    with pytest.raises(ValueError):
        rt.geometry_table([(sph, 4)], device="cpu")
    with pytest.raises(ValueError):
        rt.geometry_table([(torch.zeros((3, 8))[:, ::2], 3)], device="cpu")


def test_the_dtypes_are_the_reference_module_s(rt):
    import instance_mixed_ref as mr
    assert mr.RAY == rt.RAY and mr.HIT == rt.HIT and mr.MISS == rt.MISS
    assert (mr.TRIANGLES, mr.SPHERES) == (rt.RT_GEOM_TRIANGLES, rt.RT_GEOM_SPHERES)
    assert np.dtype(mr.world().instances.dtype) == rt.INSTANCE
