"""CPU test of the instanced all-hit ABI (rt_ray_hits_count_instanced, rt_ray_hits_collect_instanced): the header declares both
entry points, the Python names and EXPORTS are present, and every argument error is refused before any GPU work (the pointers
below are never dereferenced: a correct library returns before it touches them)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000          # a 256-byte aligned "device pointer" that must never be used


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rt_abi.h")).read(), flags=re.S)


def test_header_declares_the_entry_points():
    src = _header()
    m = re.search(r"\bint\s+rt_ray_hits_count_instanced\s*\((.*?)\)\s*;", src, flags=re.S)
    assert m, "rt_ray_hits_count_instanced is not declared"
    names = [re.sub(r".*[\s*]", "", a.strip()) for a in m.group(1).split(",")]
    assert names == ["tlas", "records", "num_instances", "blas_table", "num_blas", "rays", "num_rays", "offsets", "scratch",
                     "counters", "status", "stream"]
    m = re.search(r"\bint\s+rt_ray_hits_collect_instanced\s*\((.*?)\)\s*;", src, flags=re.S)
    assert m, "rt_ray_hits_collect_instanced is not declared"
    names = [re.sub(r".*[\s*]", "", a.strip()) for a in m.group(1).split(",")]
    assert names == ["tlas", "records", "num_instances", "blas_table", "num_blas", "rays", "num_rays", "offsets", "hits",
                     "instance_ids", "counts", "counters", "status", "stream"]
    assert "RT_RAY_HITS_STACK_OVERFLOW = 1" in src and "RT_RAY_HITS_TRUNCATED = 2" in src
    # no new size function: the scratch is rt_ray_hits_scratch_bytes's
    assert not re.search(r"rt_ray_hits\w*instanced\w*scratch_bytes|rt_ray_hits_scratch_bytes_instanced", src)


def test_python_names_and_exports(rt):
    for name in ("rt_ray_hits_count_instanced", "rt_ray_hits_collect_instanced"):
        assert name in rt.EXPORTS and getattr(rt.lib(), name) is not None
    for name in ("RayHitsCountInstanced", "RayHitsCollectInstanced", "RayHitsInstanced", "ray_hits_status"):
        assert callable(getattr(rt, name)), name
    assert "ray_hits_instanced:" in rt.version()
    assert (rt.RT_RAY_HITS_STACK_OVERFLOW, rt.RT_RAY_HITS_TRUNCATED) == (1, 2)


def _tlas(rt, a):
    return ctypes.byref(rt._Accel(a["tlas_tris"], a["tlas_nodes"], 0, a["tlas_count"])) if a["tlas"] else None


OK = dict(tlas=True, tlas_count=2, tlas_nodes=FAKE, tlas_tris=FAKE, rec=FAKE, n_inst=3, table=FAKE, nb=2, rays=FAKE, n=5,
          offsets=FAKE, scratch=FAKE, hits=FAKE, ids=FAKE, counts=FAKE, counters=None, status=FAKE)


def _count(rt, **kw):
    a = dict(OK, **kw)
    return rt.lib().rt_ray_hits_count_instanced(_tlas(rt, a), a["rec"], a["n_inst"], a["table"], a["nb"], a["rays"], a["n"],
                                                a["offsets"], a["scratch"], a["counters"], a["status"], None)


def _collect(rt, **kw):
    a = dict(OK, **kw)
    return rt.lib().rt_ray_hits_collect_instanced(_tlas(rt, a), a["rec"], a["n_inst"], a["table"], a["nb"], a["rays"], a["n"],
                                                  a["offsets"], a["hits"], a["ids"], a["counts"], a["counters"], a["status"],
                                                  None)


def test_argument_errors_both_calls(rt):
    # (every call below has num_rays = 0 where it must succeed: nothing runs; the errors win over the empty batch)
    for call in (_count, _collect):
        assert call(rt, n=0) == 0
        for n in (0, 5):
            assert call(rt, n=n, tlas=False) == -1
            assert call(rt, n=n, tlas_count=8) == -1
            assert call(rt, n=n, tlas_nodes=0) == -1
            assert call(rt, n=n, tlas_tris=0) == -1
            for k in ("rec", "table", "rays", "offsets"):
                assert call(rt, n=n, **{k: None}) == -1, k
            for k in ("rec", "rays"):
                assert call(rt, n=n, **{k: FAKE + 8}) == -1, k      # not 16-byte aligned
            assert call(rt, n=n, offsets=FAKE + 4) == -1            # not 8-byte aligned
            assert call(rt, n=n, table=FAKE + 4) == -1              # not 8-byte aligned
            assert call(rt, n=n, status=FAKE + 2) == -1             # not 4-byte aligned
            assert call(rt, n=n, nb=0) == -1                        # instances but no BLAS
        # optional arguments may be null; an empty scene (no instances, an empty TLAS) is valid and reads nothing
        assert call(rt, n=0, status=None, counters=None) == 0
        assert call(rt, n=0, n_inst=0, table=None, nb=0, rec=None, tlas_count=0, tlas_nodes=0, tlas_tris=0) == 0


def test_argument_errors_count(rt):
    for n in (0, 5):
        assert _count(rt, n=n, scratch=None) == -1
        assert _count(rt, n=n, scratch=FAKE + 128) == -1            # not 256-byte aligned
        assert _count(rt, n=n, scratch=FAKE + 16) == -1


def test_argument_errors_collect(rt):
    for n in (0, 5):
        assert _collect(rt, n=n, hits=None) == -1
        assert _collect(rt, n=n, ids=None) == -1
        assert _collect(rt, n=n, hits=FAKE + 8) == -1               # not 16-byte aligned
        assert _collect(rt, n=n, ids=FAKE + 2) == -1                # not 4-byte aligned
        assert _collect(rt, n=n, counts=FAKE + 2) == -1
    assert _collect(rt, n=0, counts=None) == 0


def test_python_wrappers_check_their_buffers(rt):
    """the wrappers' own checks, on host tensors that are never handed to the library"""
    import pytest
    import torch
    rays = torch.zeros((4, 8), dtype=torch.float32)
    off = torch.zeros(5, dtype=torch.int64)
    hits = torch.zeros((8, 4), dtype=torch.float32)
    ids = torch.zeros(8, dtype=torch.int32)
    tree = (None, None, 0, 0, None, 0, None, 0)
    with pytest.raises(ValueError):
        rt.RayHitsCountInstanced(*tree, rays, off[:4])
    with pytest.raises(ValueError):
        rt.RayHitsCountInstanced(*tree, rays[:, :7], off)
    with pytest.raises(ValueError):
        rt.RayHitsCollectInstanced(*tree, rays, off[:4], hits, ids)
    with pytest.raises(ValueError):
        rt.RayHitsCollectInstanced(*tree, rays, off, hits, ids, counts=torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError):
        rt.RayHitsCollectInstanced(*tree, rays, off, hits.t(), ids)
    # an empty batch runs nothing and needs no library call
    assert rt.RayHitsCountInstanced(*tree, rays[:0], off) == 0
    assert rt.RayHitsCollectInstanced(*tree, rays[:0], off, hits, ids) == 0
