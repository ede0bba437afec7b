"""CPU test of the capsule ABI (rt_prepare_capsules, rt_intersect_rays_capsules): the header declares both and the library
exports them, rt_capsule is the 32-byte record the binding's dtype says, and every argument error is refused before any GPU work
(the pointers below are never dereferenced: a correct library returns before it touches them)."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000          # a 16-byte aligned "device pointer" that must never be used
FAKE_ODD = FAKE + 8     # 8-byte aligned only
FAKE_WORD = FAKE + 4    # 4-byte aligned only
FAKE_BYTE = FAKE + 2    # 2-byte aligned only


def _header():
    return open(os.path.join(ROOT, "include", "rt_abi.h")).read()


def test_header_declares_the_entry_points(rt):
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"\bint\s+rt_prepare_capsules\s*\(", src)
    assert re.search(r"\bint\s+rt_intersect_rays_capsules\s*\(", src)
    assert re.search(r"enum\s*\{\s*RT_CAPSULE_BAD\s*=\s*1\s*\}", src)
    assert "rt_prepare_capsules" in rt.EXPORTS and "rt_intersect_rays_capsules" in rt.EXPORTS
    L = rt.lib()
    assert L.rt_prepare_capsules is not None and L.rt_intersect_rays_capsules is not None
    assert "capsules:" in rt.version()
    assert rt.RT_CAPSULE_BAD == 1
    # the block sits after the sphere block and says what it must
    h = _header()
    assert h.index("---- sphere primitives") < h.index("---- capsule primitives") < h.index("---- mixed instancing")
    block = h[h.index("---- capsule primitives"):h.index("typedef struct rt_capsule")]
    for words in ("2^-18", "point proxy", "primitive_id_0", "rt_refit", "rt_sort_rays", "p0 == p1", "radius == 0", "bit for bit",
                  "nearest the capsule's midpoint", "A  = nn*a - nd*nd", "C  = nn*(qq - r*r) - nq*nq", "tau1", "y1 <= -hn",
                  "no crack at the seams", "!(A > 0)", "t_far", "byte for byte", "Out of scope", "per-vertex radii",
                  "rt_geometry", "first-K", "point queries against capsules", "other kinds in one tree", "rt_cli"):
        assert words in block, words


def test_struct_layout(rt):
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    body = re.search(r"typedef struct rt_capsule \{(.*?)\} rt_capsule;", src, flags=re.S).group(1)
    assert re.sub(r"\s+", " ", body).strip() == "rt_float3 p0; float radius; rt_float3 p1; uint32_t pad;"
    assert rt.CAPSULE.itemsize == 32                                                 # sizeof(rt_capsule)
    assert [rt.CAPSULE.fields[k][1] for k in ("p0", "radius", "p1", "pad")] == [0, 12, 16, 28]
    assert rt.CAPSULE["p0"].shape == (3,) and rt.CAPSULE["p1"].shape == (3,)
    a = np.arange(16, dtype=np.float32).reshape(2, 8).view(rt.CAPSULE).reshape(-1)   # float32 [n, 8] is an rt_capsule array
    assert a["p0"].tolist() == [[0, 1, 2], [8, 9, 10]] and a["radius"].tolist() == [3, 11]
    assert a["p1"].tolist() == [[4, 5, 6], [12, 13, 14]]


def test_prepare_argument_errors(rt):
    p = rt.lib().rt_prepare_capsules
    #        capsules, n, proxies, status, stream
    good = [FAKE, 3, FAKE, FAKE_WORD, None]
    for k in (0, 2, 3):                                                              # a null pointer with a non-zero count
        a = list(good)
        a[k] = None
        assert p(*a) == -1, k
    for k, bad in ((0, FAKE_ODD), (2, FAKE_ODD), (3, FAKE_BYTE)):                    # alignment
        a = list(good)
        a[k] = bad
        assert p(*a) == -1, k
    # the status word is needed even for an empty batch (prepare clears it); alignment errors win over an empty batch
    assert p(None, 0, None, None, None) == -1
    assert p(None, 0, None, FAKE_BYTE, None) == -1
    assert p(FAKE_ODD, 0, None, FAKE_WORD, None) == -1


def _accel(rt, count=2, triangles=FAKE, nodes=FAKE):
    return ctypes.byref(rt._Accel(triangles, nodes, 0, count))


def test_query_argument_errors(rt):
    q = rt.lib().rt_intersect_rays_capsules

    def args(**kw):
        #        as, capsules, num_capsules, rays, num_rays, order, num_indices, hits, mode, counters, stream
        a = dict(tree=_accel(rt), capsules=FAKE, num_capsules=3, rays=FAKE, num_rays=5, order=None, num_indices=0, hits=FAKE,
                 mode=0, counters=None, stream=None)
        a.update(kw)
        return list(a.values())

    for null in ("tree", "capsules", "rays", "hits"):                                # null with a non-zero count
        assert q(*args(**{null: None})) == -1, null
    assert q(*args(tree=_accel(rt, count=8))) == -1                                  # count > 7
    for field in ("triangles", "nodes"):                                             # a null tree pointer with count > 0
        assert q(*args(tree=_accel(rt, **{field: 0}))) == -1, field
    for name, bad in (("capsules", FAKE_ODD), ("rays", FAKE_ODD), ("hits", FAKE_ODD), ("order", FAKE_BYTE)):
        assert q(*args(**{name: bad})) == -1, name
        assert q(*args(**{name: bad}, num_rays=0)) == -1, name                       # errors win over an empty batch
    assert q(*args(order=FAKE_BYTE, num_indices=4)) == -1
    for mode in (-1, 2, 7):
        assert q(*args(mode=mode)) == -1
        assert q(*args(mode=mode, num_rays=0)) == -1
    assert q(*args(tree=None, num_rays=0)) == -1
    assert q(*args(tree=_accel(rt, count=8), num_rays=0)) == -1
    # zero counts run nothing: no rays, or an index list without an entry
    assert q(*args(num_rays=0)) == 0
    assert q(*args(num_rays=0, rays=None, hits=None, mode=1, counters=FAKE)) == 0
    assert q(*args(order=FAKE_WORD, num_indices=0)) == 0
    assert q(*args(num_rays=0, order=FAKE_WORD, num_indices=9)) == 0
    assert q(*args(num_rays=0, capsules=None, num_capsules=0)) == 0
    assert q(*args(num_rays=0, tree=_accel(rt, count=0, triangles=0, nodes=0))) == 0


def test_python_wrappers_refuse_bad_buffers(rt):
    import torch
    rays = torch.zeros((4, 8), dtype=torch.float32)
    hits = torch.zeros((4, 4), dtype=torch.float32)
    cap = torch.zeros((3, 8), dtype=torch.float32)
    order = torch.zeros(4, dtype=torch.int32)
    tree = (torch.zeros(64, dtype=torch.uint8), torch.zeros(64, dtype=torch.uint8))

    def query(**kw):
        a = dict(rays=rays, hits=hits, capsules=cap, order=None, num_indices=None)
        a.update(kw)
        rt.IntersectRaysCapsules(tree[0], tree[1], 0, 2, a["capsules"], 3, a["rays"], a["hits"], order=a["order"],
                                 num_indices=a["num_indices"])

    for bad in (dict(hits=hits[:3]), dict(hits=torch.zeros((4, 8))[:, ::2]), dict(rays=torch.zeros((4, 16))[:, ::2]),
                dict(rays=torch.zeros(33, dtype=torch.uint8)), dict(capsules=cap[:2]), dict(capsules=torch.zeros((3, 4))),
                dict(capsules=torch.zeros((3, 16))[:, ::2]), dict(order=order, num_indices=5),
                dict(order=torch.zeros(8, dtype=torch.int32)[::2])):
        with pytest.raises(ValueError):
            query(**bad)
    prox = torch.zeros(3 * 36, dtype=torch.uint8)
    status = torch.zeros(4, dtype=torch.uint8)
    for bad in (dict(capsules=cap[:2]), dict(capsules=torch.zeros((3, 4))), dict(proxies=prox[:107]),
                dict(proxies=torch.zeros(6 * 36, dtype=torch.uint8)[::2])):
        a = dict(capsules=cap, proxies=prox)
        a.update(bad)
        with pytest.raises(ValueError):
            rt.PrepareCapsules(a["capsules"], 3, a["proxies"], status)


def test_the_dtypes_are_the_reference_modules(rt):
    import capsule_ref as cr
    assert cr.RAY == rt.RAY and cr.HIT == rt.HIT and cr.MISS == rt.MISS and cr.RT_CAPSULE_BAD == rt.RT_CAPSULE_BAD
    assert cr.gpu_scene("strand").view(rt.CAPSULE).shape == (1004, 1)
    assert (cr.gpu_scene("far").view(rt.CAPSULE)["pad"] == 0).all()
