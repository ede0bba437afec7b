"""CPU test of the ABI of the filtered instanced all-hit and first-K queries (rt_ray_hits_count_instanced_filtered,
rt_ray_hits_collect_instanced_filtered, rt_ray_first_hits_instanced_filtered): the header declares each as its sibling's
signature with `filter` before the outputs and carries the instanced set-filter block, the library exports them, the Python
names exist, and every argument error -- the sibling's and the filter's own -- is refused before any GPU work (the pointers
below are never dereferenced: a correct library returns before it touches them).  A NULL filter forwards to the sibling: checked
here for argument-error parity only."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000          # a 256-byte aligned "device pointer" that must never be used
NAMES = ("rt_ray_hits_count_instanced_filtered", "rt_ray_hits_collect_instanced_filtered",
         "rt_ray_first_hits_instanced_filtered")


def _raw():
    return open(os.path.join(ROOT, "include", "rt_abi.h")).read()


def _params(src, name):
    m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", src, flags=re.S)
    assert m, f"{name} is not declared"
    return [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")], m.start()


def test_header_declares_the_entry_points():
    raw = _raw()
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    flt = "const rt_instance_hit_filter* filter"
    for name, before in (("rt_ray_hits_count_instanced", "uint64_t* offsets"),
                         ("rt_ray_hits_collect_instanced", "const uint64_t* offsets"),
                         ("rt_ray_first_hits_instanced", "rt_hit* hits")):
        sib, _ = _params(src, name)
        got, at = _params(src, name + "_filtered")
        j = sib.index(before)
        assert got == sib[:j] + [flt] + sib[j:], f"{name}_filtered is not its sibling's signature with `filter` before the outputs"
        assert at > src.index("} rt_instance_hit_filter;"), "declared before the struct it takes"
    # the block and its contracts
    assert "instanced set-filter" in raw
    block = raw[raw.index("instance filters for the instanced all-hit and first-K ray queries"):]
    block = block[:block.index("*/")]
    for words in ("Instance rule", "Candidate rule", "BEFORE the instance record is read", "slab test in the TLAS is still counted",
                  "The window never moves", "moves only on kept items", "Keep-all", "Composition", "Closest hit", "Masks",
                  "One identity instance", "filter == NULL forwards", "before any GPU work", "8-byte aligned", "16-byte aligned",
                  "Out of scope: per-primitive masks, instance motion, mixed / sphere BLASes, an indexed form, the host mirror",
                  "rt_cli", "DESIGN section 31"):
        assert words in block, words
    # the siblings' and the instance-filter block's "out of scope" sentences no longer name the filter
    assert "Out of scope: hit filters and instance masks" not in raw
    assert "take no filter" not in raw[raw.index("hit filters and instance masks for the instanced ray query"):
                                       raw.index("instance filters for the instanced all-hit and first-K")]
    # the struct, its flags and records are the existing ones: declared once
    for pat in (r"\}\s*rt_instance_hit_filter;", r"\}\s*rt_instance_filter;", r"\}\s*rt_instance_ray_filter;",
                r"RT_INSTANCE_FILTER_CULL_DISABLE\s*="):
        assert len(re.findall(pat, src)) == 1, pat


def test_exports_and_python_names(rt):
    for name in NAMES:
        assert name in rt.EXPORTS and getattr(rt.lib(), name) is not None
    for name in ("RayHitsCountInstancedFiltered", "RayHitsCollectInstancedFiltered", "RayHitsInstancedFiltered",
                 "RayFirstHitsInstancedFiltered", "InstanceHitFilter"):
        assert callable(getattr(rt, name)), name
    assert "instance_set_filter:" in rt.version()


def _tlas(rt, a):
    return ctypes.byref(rt._Accel(a["tlas_tris"], a["tlas_nodes"], 0, a["tlas_count"])) if a["tlas"] else None


def _filter(rt, flags=0, ray_mask=0xFFFFFFFF, num=0, per_instance=None, per_ray=None):
    return ctypes.byref(rt._InstanceHitFilter(flags, ray_mask, num, 0, per_instance, per_ray))


OK = dict(tlas=True, tlas_count=2, tlas_nodes=FAKE, tlas_tris=FAKE, rec=FAKE, n_inst=3, table=FAKE, nb=2, rays=FAKE, n=5, k=4,
          offsets=FAKE, scratch=FAKE, hits=FAKE, ids=FAKE, counts=FAKE, counters=None, status=FAKE, flt="ok")


def _flt(rt, a):
    return _filter(rt) if a["flt"] == "ok" else a["flt"]


def _count(rt, **kw):
    a = dict(OK, **kw)
    return rt.lib().rt_ray_hits_count_instanced_filtered(_tlas(rt, a), a["rec"], a["n_inst"], a["table"], a["nb"], a["rays"],
                                                         a["n"], _flt(rt, a), a["offsets"], a["scratch"], a["counters"],
                                                         a["status"], None)


def _collect(rt, **kw):
    a = dict(OK, **kw)
    return rt.lib().rt_ray_hits_collect_instanced_filtered(_tlas(rt, a), a["rec"], a["n_inst"], a["table"], a["nb"], a["rays"],
                                                           a["n"], _flt(rt, a), a["offsets"], a["hits"], a["ids"], a["counts"],
                                                           a["counters"], a["status"], None)


def _first(rt, **kw):
    a = dict(OK, **kw)
    return rt.lib().rt_ray_first_hits_instanced_filtered(_tlas(rt, a), a["rec"], a["n_inst"], a["table"], a["nb"], a["rays"],
                                                         a["n"], a["k"], _flt(rt, a), a["hits"], a["ids"], a["counters"],
                                                         a["status"], None)


CALLS = (_count, _collect, _first)


def test_the_filters_own_errors(rt):
    for call in CALLS:
        for n in (5, 0):                                            # also for an empty batch: the errors win
            for flags in (4, 8, 0x80000000, 0xFFFFFFFF, 1 | 4):
                assert call(rt, n=n, flt=_filter(rt, flags=flags)) == -1, (call.__name__, flags)
            for off in (1, 2, 4, 6):
                assert call(rt, n=n, flt=_filter(rt, num=3, per_instance=FAKE + off)) == -1
            for off in (1, 2, 4, 8, 12):
                assert call(rt, n=n, flt=_filter(rt, per_ray=FAKE + off)) == -1
        # legal filters on an empty batch: both cull bits, num_instance_filters > 0 with a null per_instance, aligned arrays
        for flt in ("ok", None, _filter(rt, flags=3), _filter(rt, num=77),
                    _filter(rt, flags=1, ray_mask=0, num=9, per_instance=FAKE + 8, per_ray=FAKE + 16)):
            assert call(rt, n=0, flt=flt) == 0
            assert call(rt, n=0, flt=flt, n_inst=0, table=None, nb=0, rec=None, tlas_count=0, tlas_nodes=0, tlas_tris=0) == 0


def test_the_siblings_errors_with_a_filter_and_with_none(rt):
    """with a valid filter and with NULL (which forwards to the sibling) the same calls are refused"""
    for flt in ("ok", None):
        for call in CALLS:
            assert call(rt, n=0, flt=flt) == 0
            for n in (0, 5):
                assert call(rt, n=n, flt=flt, tlas=False) == -1
                assert call(rt, n=n, flt=flt, tlas_count=8) == -1
                assert call(rt, n=n, flt=flt, tlas_nodes=0) == -1
                assert call(rt, n=n, flt=flt, tlas_tris=0) == -1
                for key in ("rec", "table", "rays"):
                    assert call(rt, n=n, flt=flt, **{key: None}) == -1, key
                for key in ("rec", "rays"):
                    assert call(rt, n=n, flt=flt, **{key: FAKE + 8}) == -1, key
                assert call(rt, n=n, flt=flt, table=FAKE + 4) == -1
                assert call(rt, n=n, flt=flt, status=FAKE + 2) == -1
                assert call(rt, n=n, flt=flt, nb=0) == -1
            assert call(rt, n=0, flt=flt, status=None, counters=None) == 0
        for n in (0, 5):
            for call in (_count, _collect):
                assert call(rt, n=n, flt=flt, offsets=None) == -1
                assert call(rt, n=n, flt=flt, offsets=FAKE + 4) == -1
            assert _count(rt, n=n, flt=flt, scratch=None) == -1
            assert _count(rt, n=n, flt=flt, scratch=FAKE + 128) == -1
            for call in (_collect, _first):
                assert call(rt, n=n, flt=flt, hits=None) == -1
                assert call(rt, n=n, flt=flt, ids=None) == -1
                assert call(rt, n=n, flt=flt, hits=FAKE + 8) == -1
                assert call(rt, n=n, flt=flt, ids=FAKE + 2) == -1
            assert _collect(rt, n=n, flt=flt, counts=FAKE + 2) == -1
            assert _first(rt, n=n, flt=flt, counters=FAKE + 4) == -1          # (the first-K sibling's check alone)
            assert _first(rt, n=n, flt=flt, k=0) == -1
            assert _first(rt, n=n, flt=flt, k=rt.RT_RAY_FIRST_MAX_K + 1) == -1
        assert _collect(rt, n=0, flt=flt, counts=None) == 0
        assert _first(rt, n=0, flt=flt, k=1) == 0 and _first(rt, n=0, flt=flt, k=rt.RT_RAY_FIRST_MAX_K) == 0


def test_python_wrappers_check_their_arguments(rt):
    """the wrappers' own checks, on host tensors that are never handed to the library"""
    import torch
    rays = torch.zeros((4, 8), dtype=torch.float32)
    off = torch.zeros(5, dtype=torch.int64)
    hits = torch.zeros((8, 4), dtype=torch.float32)
    ids = torch.zeros(8, dtype=torch.int32)
    rows, row_ids = torch.zeros((4, 3, 4), dtype=torch.float32), torch.zeros((4, 3), dtype=torch.int32)
    tree = (None, None, 0, 0, None, 0, None, 0)
    short = rt.InstanceHitFilter(per_ray=torch.zeros((3, 4), dtype=torch.int32))
    for bad in (short, rt.HitFilter(), "x"):
        with pytest.raises(ValueError):
            rt.RayHitsCountInstancedFiltered(*tree, rays, bad, off)
        with pytest.raises(ValueError):
            rt.RayHitsCollectInstancedFiltered(*tree, rays, bad, off, hits, ids)
        with pytest.raises(ValueError):
            rt.RayFirstHitsInstancedFiltered(*tree, rays, 3, bad, rows, row_ids)
    with pytest.raises(ValueError):
        rt.RayHitsCountInstancedFiltered(*tree, rays, None, off[:4])
    with pytest.raises(ValueError):
        rt.RayHitsCollectInstancedFiltered(*tree, rays, None, off[:4], hits, ids)
    with pytest.raises(ValueError):
        rt.RayHitsCollectInstancedFiltered(*tree, rays, None, off, hits, ids, counts=torch.zeros(3, dtype=torch.int32))
    for k in (0, 33):
        with pytest.raises(ValueError):
            rt.RayFirstHitsInstancedFiltered(*tree, rays, k, None, rows, row_ids)
    with pytest.raises(ValueError):
        rt.RayFirstHitsInstancedFiltered(*tree, rays, 2, None, rows, row_ids)
    with pytest.raises(ValueError):
        rt.RayFirstHitsInstancedFiltered(*tree, rays, 3, None, rows, row_ids.to(torch.int64))
    # an empty batch runs nothing and needs no library call
    flt = rt.InstanceHitFilter(flags=1)
    assert rt.RayHitsCountInstancedFiltered(*tree, rays[:0], flt, off[:1]) == 0
    assert rt.RayHitsCollectInstancedFiltered(*tree, rays[:0], flt, off[:1], hits, ids) == 0
    assert rt.RayFirstHitsInstancedFiltered(*tree, rays[:0], 3, flt, rows[:0], row_ids[:0]) == 0
