"""CPU test of the instanced first-K ABI (rt_ray_first_hits_instanced): the header declares the entry point behind the first-K
block, the Python name and EXPORTS are present, and every argument error is refused before any GPU work (the pointers below are
never dereferenced: a correct library returns before it touches them)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000          # a 256-byte aligned "device pointer" that must never be used


def test_header_declares_the_entry_point():
    raw = open(os.path.join(ROOT, "include", "rt_abi.h")).read()
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    m = re.search(r"\bint\s+rt_ray_first_hits_instanced\s*\((.*?)\)\s*;", src, flags=re.S)
    assert m, "rt_ray_first_hits_instanced is not declared"
    names = [re.sub(r".*[\s*]", "", a.strip()) for a in m.group(1).split(",")]
    assert names == ["tlas", "records", "num_instances", "blas_table", "num_blas", "rays", "num_rays", "k", "hits",
                     "instance_ids", "counters", "status", "stream"]
    # behind the first-K block, whose constants it shares: no new limit, no new flag
    assert src.index("rt_ray_first_hits(") < m.start() < src.index("rt_ray_first_hits_filtered(")
    assert len(re.findall(r"#define\s+RT_RAY_FIRST_MAX_K\b", src)) == 1 and "RT_RAY_FIRST_STACK_OVERFLOW = 1" in src
    assert "instanced first-K ray queries" in raw and "(t, instance, primitive_id)" in raw


def test_python_names_and_exports(rt):
    assert "rt_ray_first_hits_instanced" in rt.EXPORTS and rt.lib().rt_ray_first_hits_instanced is not None
    for name in ("RayFirstHitsInstanced", "ray_first_status"):
        assert callable(getattr(rt, name)), name
    assert "ray_first_instanced:" in rt.version()
    assert (rt.RT_RAY_FIRST_MAX_K, rt.RT_RAY_FIRST_STACK_OVERFLOW) == (32, 1)


OK = dict(tlas=True, tlas_count=2, tlas_nodes=FAKE, tlas_tris=FAKE, rec=FAKE, n_inst=3, table=FAKE, nb=2, rays=FAKE, n=5, k=4,
          hits=FAKE, ids=FAKE, counters=None, status=FAKE)


def _call(rt, **kw):
    a = dict(OK, **kw)
    tlas = ctypes.byref(rt._Accel(a["tlas_tris"], a["tlas_nodes"], 0, a["tlas_count"])) if a["tlas"] else None
    return rt.lib().rt_ray_first_hits_instanced(tlas, a["rec"], a["n_inst"], a["table"], a["nb"], a["rays"], a["n"], a["k"],
                                                a["hits"], a["ids"], a["counters"], a["status"], None)


def test_argument_errors(rt):
    # (every call below has num_rays = 0 where it must succeed: nothing runs; the errors win over the empty batch)
    # -1: RT_ERR_INVALID_ARGUMENT
    assert _call(rt, n=0) == 0
    for n in (0, 5):
        assert _call(rt, n=n, tlas=False) == -1
        assert _call(rt, n=n, tlas_count=8) == -1
        assert _call(rt, n=n, tlas_nodes=0) == -1
        assert _call(rt, n=n, tlas_tris=0) == -1
        for key in ("rec", "table", "rays", "hits", "ids"):
            assert _call(rt, n=n, **{key: None}) == -1, key
        assert _call(rt, n=n, nb=0) == -1                           # instances but no BLAS
        for key in ("rec", "rays", "hits"):
            assert _call(rt, n=n, **{key: FAKE + 8}) == -1, key     # not 16-byte aligned
        assert _call(rt, n=n, table=FAKE + 4) == -1                 # not 8-byte aligned
        assert _call(rt, n=n, counters=FAKE + 4) == -1              # not 8-byte aligned
        assert _call(rt, n=n, ids=FAKE + 2) == -1                   # not 4-byte aligned
        assert _call(rt, n=n, status=FAKE + 2) == -1                # not 4-byte aligned
        assert _call(rt, n=n, k=0) == -1
        assert _call(rt, n=n, k=rt.RT_RAY_FIRST_MAX_K + 1) == -1
    # k at its limits, optional arguments null, an empty scene (no instances, an empty TLAS): valid, and nothing is read
    assert _call(rt, n=0, k=1) == 0 and _call(rt, n=0, k=rt.RT_RAY_FIRST_MAX_K) == 0
    assert _call(rt, n=0, status=None, counters=None) == 0
    assert _call(rt, n=0, n_inst=0, table=None, nb=0, rec=None, tlas_count=0, tlas_nodes=0, tlas_tris=0) == 0


def test_python_wrapper_checks_its_buffers(rt):
    """the wrapper's own checks, on host tensors that are never handed to the library"""
    import torch
    rays = torch.zeros((4, 8), dtype=torch.float32)
    hits = torch.zeros((4, 3, 4), dtype=torch.float32)
    ids = torch.zeros((4, 3), dtype=torch.int32)
    tree = (None, None, 0, 0, None, 0, None, 0)
    for k in (0, 33):
        with pytest.raises(ValueError):
            rt.RayFirstHitsInstanced(*tree, rays, k, hits, ids)
    with pytest.raises(ValueError):
        rt.RayFirstHitsInstanced(*tree, rays, 2, hits, ids)                      # rows of 3, k = 2
    with pytest.raises(ValueError):
        rt.RayFirstHitsInstanced(*tree, rays, 3, hits, ids[:, :2])
    with pytest.raises(ValueError):
        rt.RayFirstHitsInstanced(*tree, rays, 3, hits, ids.to(torch.int64))
    with pytest.raises(ValueError):
        rt.RayFirstHitsInstanced(*tree, rays, 3, hits.to(torch.float64), ids)
    with pytest.raises(ValueError):
        rt.RayFirstHitsInstanced(*tree, rays[:, :7], 3, hits, ids)
    # an empty batch runs nothing and needs no library call
    assert rt.RayFirstHitsInstanced(*tree, rays[:0], 3, hits[:0], ids[:0]) == 0
