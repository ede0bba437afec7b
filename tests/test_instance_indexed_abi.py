"""CPU test of the indexed forms of the instanced and motion ray queries (rt_intersect_rays_instanced_indexed,
rt_intersect_rays_instanced_motion_indexed, rt_intersect_rays_instanced_mixed_indexed, rt_intersect_rays_motion_indexed): the
header declares them and the library exports them; a null or misaligned `order` and every argument error of the sibling is
refused before any GPU work (the pointers below are never dereferenced: a correct library returns before it touches them);
num_indices == 0 succeeds and runs nothing; the Python wrappers refuse bad buffers."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000          # a 16-byte aligned "device pointer" that must never be used
FAKE_ODD = FAKE + 8     # 8-byte aligned only
FAKE_WORD = FAKE + 4    # 4-byte aligned only
FAKE_BYTE = FAKE + 2    # 2-byte aligned only
NAMES = ("rt_intersect_rays_instanced_indexed", "rt_intersect_rays_instanced_motion_indexed",
         "rt_intersect_rays_instanced_mixed_indexed", "rt_intersect_rays_motion_indexed")


def _header():
    return open(os.path.join(ROOT, "include", "rt_abi.h")).read()


def test_header_and_exports(rt):
    h = _header()
    src = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    L = rt.lib()
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in rt.EXPORTS and getattr(L, name) is not None, name
    for name in ("IntersectRaysInstancedIndexed", "IntersectRaysInstancedMotionIndexed", "IntersectRaysInstancedMixedIndexed",
                 "IntersectRaysMotionIndexed"):
        assert callable(getattr(rt, name)), name
    # (order, num_indices) follow num_rays, the output arrays follow them: rt_intersect_rays_indexed's shape
    for name in NAMES:
        decl = re.sub(r"\s+", " ", re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, src, flags=re.S).group(1))
        assert "uint32_t num_rays, const uint32_t* order, uint32_t num_indices, rt_hit* hits" in decl, name
    decl = re.sub(r"\s+", " ", re.search(r"\bint\s+rt_intersect_rays_instanced_indexed\s*\((.*?)\)\s*;", src, flags=re.S).group(1))
    assert decl.endswith("uint32_t* instance_ids, int mode, uint32_t num_primitives, const rt_instance_hit_filter* filter, "
                         "uint64_t* counters, void* stream")
    # the block says what it must, and nothing says any more that these queries have no indexed form
    block = h[h.index("---- indexed forms of the instanced and motion ray queries"):h.index("int rt_intersect_rays_instanced_indexed(")]
    for words in ("rt_intersect_rays_indexed's contract", "i = order[j]", "i >= num_rays", "never by j", "filter->per_ray[i]",
                  "times[i]", "instance_ids[i]", "reload of the world ray", "not written, in neither array",
                  "writes the same bytes twice", "counters[0] and [1] equal the sibling's", "identity list all four",
                  "null order or one", "num_indices = 0", "hipGraph-capturable", "no separate filtered-indexed symbol",
                  "Out of scope", "set-valued queries", "sort key that knows about instances", "rt_cli"):
        assert words in block, words
    flat = re.sub(r"\s*\n \*\s*", " ", h)
    assert "the indexed query has no instanced form" not in flat
    assert "filtered, indexed, all-hit and first-K motion forms" not in flat


# ------------------------------------------------------------------ argument errors
def _accel(rt, count=2, nodes=FAKE, tris=FAKE):
    return ctypes.byref(rt._Accel(tris, nodes, 0, count))


def _maccel(rt, count=2, **null):
    p = dict(triangles0=FAKE, nodes0=FAKE, triangles1=FAKE, nodes1=FAKE)
    p.update(null)
    return ctypes.byref(rt._MotionAccel(p["triangles0"], p["nodes0"], p["triangles1"], p["nodes1"], 0, count))


def _caller(rt, name):
    """name -> call(**overrides): the entry point with valid arguments (5 rays, 4 indices) except the overrides"""
    f = getattr(rt.lib(), name)
    if name == "rt_intersect_rays_instanced_indexed":
        good = dict(tlas=_accel(rt), records=FAKE, num_instances=3, table=FAKE_ODD, num_blas=2, rays=FAKE, num_rays=5,
                    order=FAKE_WORD, num_indices=4, hits=FAKE, ids=FAKE_WORD, mode=0, num_primitives=0, filter=None,
                    counters=None, stream=None)
    elif name == "rt_intersect_rays_instanced_motion_indexed":
        good = dict(tlas=_maccel(rt), records=FAKE, num_instances=3, table=FAKE_ODD, num_blas=2, rays=FAKE, times=FAKE_WORD,
                    num_rays=5, order=FAKE_WORD, num_indices=4, hits=FAKE, ids=FAKE_WORD, mode=0, counters=None, stream=None)
    elif name == "rt_intersect_rays_instanced_mixed_indexed":
        good = dict(tlas=_accel(rt), records=FAKE, num_instances=3, table=FAKE_ODD, geom=FAKE, num_blas=2, rays=FAKE, num_rays=5,
                    order=FAKE_WORD, num_indices=4, hits=FAKE, ids=FAKE_WORD, mode=0, counters=None, stream=None)
    else:
        good = dict(tlas=_maccel(rt), rays=FAKE, times=FAKE_WORD, num_rays=5, order=FAKE_WORD, num_indices=4, hits=FAKE, mode=0,
                    counters=None, stream=None)

    def call(**kw):
        assert set(kw) <= set(good), kw
        a = dict(good)
        a.update(kw)
        return f(*a.values())
    call.has = lambda k: k in good
    return call


@pytest.mark.parametrize("name", NAMES)
def test_order_errors_and_empty_lists(rt, name):
    call = _caller(rt, name)
    assert call(order=None) == -1                                   # a null order
    for bad in (FAKE_BYTE, FAKE + 1, FAKE + 3):
        assert call(order=bad) == -1, bad                           # not 4-byte aligned
    # errors win over an empty list and an empty batch
    assert call(order=None, num_indices=0) == -1
    assert call(order=FAKE_BYTE, num_indices=0) == -1
    assert call(order=None, num_rays=0) == -1
    assert call(num_indices=0, mode=2) == -1
    assert call(num_indices=0, hits=None) == -1
    # an empty list or an empty batch with valid arguments: success, nothing runs
    assert call(num_indices=0) == 0
    assert call(num_indices=0, mode=1, counters=FAKE) == 0
    assert call(num_rays=0) == 0
    assert call(num_rays=0, num_indices=0) == 0


@pytest.mark.parametrize("name", NAMES)
def test_the_siblings_argument_errors(rt, name):
    call = _caller(rt, name)
    motion = "motion" in name
    accel = _maccel if motion else _accel
    assert call(tlas=None) == -1
    assert call(tlas=accel(rt, count=8)) == -1                      # count > 7
    if motion:
        for field in ("triangles0", "nodes0", "triangles1", "nodes1"):
            assert call(tlas=_maccel(rt, **{field: 0})) == -1, field    # a null tree pointer with count > 0
    else:
        assert call(tlas=_accel(rt, nodes=0)) == -1 and call(tlas=_accel(rt, tris=0)) == -1
    nulls = [k for k in ("records", "table", "rays", "times", "hits", "ids") if call.has(k)]
    for k in nulls:
        assert call(**{k: None}) == -1, k
        assert call(**{k: None}, num_indices=0) == -1, k            # ... before the empty list is looked at
    align = dict(rays=FAKE_ODD, hits=FAKE_ODD, records=FAKE_ODD, table=FAKE_WORD, times=FAKE_BYTE, ids=FAKE_BYTE, geom=FAKE_ODD)
    for k, bad in align.items():
        if call.has(k):
            assert call(**{k: bad}) == -1, k
    for mode in (-1, 2, 7):
        assert call(mode=mode) == -1
    if call.has("num_blas"):
        assert call(num_blas=0) == -1                               # instances but no BLAS
        # no instances: records and the table may be null; an empty TLAS needs no tree pointers
        assert call(num_indices=0, records=None, table=None, num_instances=0, num_blas=0) == 0
    empty = _maccel(rt, count=0, triangles0=0, nodes0=0, triangles1=0, nodes1=0) if motion else _accel(rt, count=0, nodes=0, tris=0)
    assert call(num_indices=0, tlas=empty) == 0


def test_the_filter_s_argument_errors(rt):
    """rt_intersect_rays_instanced_indexed with a filter: rt_intersect_rays_instanced_filtered's checks"""
    call = _caller(rt, "rt_intersect_rays_instanced_indexed")

    def flt(flags=0, per_instance=None, per_ray=None):
        return ctypes.byref(rt._InstanceHitFilter(flags, 0xFFFFFFFF, 0, 0, per_instance, per_ray))
    for bad in (flt(flags=4), flt(flags=0x80000001), flt(per_instance=FAKE_WORD), flt(per_ray=FAKE_ODD)):
        assert call(filter=bad) == -1
        assert call(filter=bad, num_indices=0) == -1
    for good in (flt(), flt(flags=3), flt(per_instance=FAKE_ODD, per_ray=FAKE)):
        assert call(filter=good, num_indices=0) == 0
        assert call(filter=good, order=None) == -1                  # the order's checks hold with a filter too


def test_mixed_without_a_table_reaches_the_instanced_checks(rt):
    call = _caller(rt, "rt_intersect_rays_instanced_mixed_indexed")
    assert call(geom=None, order=None) == -1
    assert call(geom=None, order=FAKE_BYTE) == -1
    assert call(geom=None, rays=FAKE_ODD) == -1
    assert call(geom=None, num_indices=0) == 0


# ------------------------------------------------------------------ the Python wrappers
def test_python_wrappers_refuse_bad_buffers(rt):
    import torch
    rays = torch.zeros((4, 8), dtype=torch.float32)
    hits = torch.zeros((4, 4), dtype=torch.float32)
    ids = torch.zeros(4, dtype=torch.int32)
    times = torch.zeros(4)
    order = torch.zeros(6, dtype=torch.int32)
    buf = torch.zeros(256, dtype=torch.uint8)
    pose = (buf, buf)
    geom = torch.zeros(2 * 16, dtype=torch.uint8)

    def calls(a):
        yield lambda: rt.IntersectRaysInstancedIndexed(buf, buf, 0, 2, buf, 2, buf, 2, a["rays"], a["order"], a["hits"], a["ids"],
                                                       num_indices=a["k"], filter=a["filter"])
        yield lambda: rt.IntersectRaysInstancedMotionIndexed(pose, pose, 0, 2, buf, 2, buf, 2, a["rays"], a["times"], a["order"],
                                                             a["hits"], a["ids"], num_indices=a["k"])
        yield lambda: rt.IntersectRaysInstancedMixedIndexed(buf, buf, 0, 2, buf, 2, buf, geom, 2, a["rays"], a["order"], a["hits"],
                                                            a["ids"], num_indices=a["k"])
        yield lambda: rt.IntersectRaysMotionIndexed(pose, pose, 0, 2, a["rays"], a["times"], a["order"], a["hits"], num_indices=a["k"])

    good = dict(rays=rays, times=times, order=order, hits=hits, ids=ids, k=0, filter=None)
    for call in calls(good):
        call()                                                      # num_indices = 0 returns before the library is called
    for call in calls(dict(good, rays=rays[:0], k=None)):
        call()                                                      # and so does an empty batch
    for bad in (dict(hits=hits[:3]), dict(hits=torch.zeros((4, 8))[:, ::2]), dict(rays=torch.zeros((4, 16))[:, ::2]),
                dict(rays=torch.zeros(33, dtype=torch.uint8)), dict(order=torch.zeros(12, dtype=torch.int32)[::2]), dict(k=7)):
        for call in calls(dict(good, **bad)):
            with pytest.raises(ValueError):
                call()
    for bad, which in ((dict(ids=ids[:3]), (0, 1, 2)), (dict(ids=torch.zeros(8, dtype=torch.int32)[::2]), (0, 1, 2)),
                       (dict(times=times[:3]), (1, 3)), (dict(times=torch.zeros(8)[::2]), (1, 3)), (dict(filter="cull"), (0,)),
                       (dict(filter=rt.InstanceHitFilter(per_ray=torch.zeros((3, 4), dtype=torch.int32))), (0,))):
        for k, call in enumerate(calls(dict(good, **bad))):
            if k in which:
                with pytest.raises(ValueError):
                    call()
