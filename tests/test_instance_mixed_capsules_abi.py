"""CPU test of the ABI of mixed instancing with capsules (rt_intersect_rays_instanced_mixed_capsules): the header declares the
entry point and RT_GEOM_CAPSULES, the library exports it, every argument error is refused before any GPU work (the pointers
below are never dereferenced: a correct library returns before it touches them), errors win over empty batches, a null
geom_table is an error here, and the Python wrapper and geometry_table refuse bad buffers."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000          # a 16-byte aligned "device pointer" that must never be used
FN = "rt_intersect_rays_instanced_mixed_capsules"


def _header():
    return open(os.path.join(ROOT, "include", "rt_abi.h")).read()


def test_header_declares_the_entry_point(rt):
    h = _header()
    src = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    assert re.search(r"\bint\s+" + FN + r"\s*\(\s*const\s+rt_accel\s*\*", src)
    assert re.search(r"\bRT_GEOM_CAPSULES\s*=\s*2\b", src)
    assert FN in rt.EXPORTS and getattr(rt.lib(), FN) is not None
    assert (rt.RT_GEOM_TRIANGLES, rt.RT_GEOM_SPHERES, rt.RT_GEOM_CAPSULES) == (0, 1, 2)
    assert callable(rt.IntersectRaysInstancedMixedCapsules)
    assert "instance_mixed_capsules:" in rt.version()
    block = h[h.index("---- mixed instancing with capsules"):h.index("enum { RT_GEOM_CAPSULES")]
    for words in ("order == NULL is the direct form", "NOT ENTERED", "none of the three", "data is null",
                  "count == 0 enters the instance and tests nothing", "id >= count", "two independent 16-byte loads",
                  "affine image", "p0 == p1", "byte for byte", "One tmax", "first accepted primitive of any kind",
                  "geom_table == NULL", "Out of scope", "filtered, motion, all-hit and first-K", "stack-depth pin",
                  "inside one BLAS", "rt_cli"):
        assert words in block, words
    # the old mixed block stays true; the capsule block no longer lists the capsule kind as out of scope
    mixed = h[h.index("---- mixed instancing"):h.index("enum { RT_GEOM_TRIANGLES")]
    assert "neither RT_GEOM_TRIANGLES nor" in mixed and "neither RT_GEOM_* value" not in mixed
    capsule = h[h.index("---- capsule primitives"):h.index("typedef struct rt_capsule")]
    assert "a capsule kind in rt_geometry" not in capsule[capsule.index("Out of scope"):]


def _call(rt, tlas_count=2, tlas_nodes=FAKE, tlas_tris=FAKE, rec=FAKE, n_inst=3, table=FAKE, geom=FAKE, nb=2, rays=FAKE,
          hits=FAKE, ids=FAKE, n=5, order=None, k=0, mode=0, tlas=True):
    a = ctypes.byref(rt._Accel(tlas_tris, tlas_nodes, 0, tlas_count)) if tlas else None
    return getattr(rt.lib(), FN)(a, rec, n_inst, table, geom, nb, rays, n, order, k, hits, ids, mode, None, None)


@pytest.mark.parametrize("order", (None, FAKE), ids=("direct", "indexed"))
def test_argument_errors(rt, order):
    """the two siblings' errors, in the direct form and through an index list"""
    def call(**kw):
        return _call(rt, order=order, k=4, **kw)

    assert call(tlas=False) == -1
    assert call(tlas_count=8) == -1                          # count > 7
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
    assert call(n=0, hits=FAKE + 8) == -1
    assert call(n=0) == 0
    assert call(n=0, mode=1) == 0
    # an empty scene (no instances, an empty TLAS): arguments are valid, nothing is read
    assert call(n=0, n_inst=0, table=None, nb=0, rec=None, tlas_count=0, tlas_nodes=0, tlas_tris=0) == 0


def test_geometry_table_is_required_and_aligned(rt):
    for order in (None, FAKE):
        assert _call(rt, geom=None, order=order, k=4) == -1, "a null geom_table is an argument error here"
        assert _call(rt, geom=None, order=order, k=4, n=0) == -1
        for bad in (FAKE + 8, FAKE + 4, FAKE + 1):
            assert _call(rt, geom=bad, order=order, k=4) == -1, bad
            assert _call(rt, geom=bad, order=order, k=4, n=0) == -1, bad       # errors win over an empty batch
        assert _call(rt, geom=FAKE, order=order, k=4, n=0) == 0
    # ... while the old calls keep their all-triangle shortcut (their own checks pass a null table on to the sibling)
    a = ctypes.byref(rt._Accel(FAKE, FAKE, 0, 2))
    assert rt.lib().rt_intersect_rays_instanced_mixed(a, FAKE, 3, FAKE, None, 2, FAKE, FAKE, FAKE, 0, 0, None, None) == 0


def test_order_list_errors(rt):
    for bad in (FAKE + 2, FAKE + 1):
        assert _call(rt, order=bad, k=4) == -1               # not 4-byte aligned
        assert _call(rt, order=bad, k=4, n=0) == -1
        assert _call(rt, order=bad, k=0) == -1               # errors win over an empty list
    assert _call(rt, order=FAKE, k=0) == 0                   # an index list without an entry runs nothing
    assert _call(rt, order=FAKE, k=0, mode=5) == -1


def test_python_wrapper_refuses_bad_buffers(rt):
    import torch
    rays = torch.zeros((4, 8), dtype=torch.float32)
    hits = torch.zeros((4, 4), dtype=torch.float32)
    ids = torch.zeros(4, dtype=torch.int32)
    geom = torch.zeros(2 * 16, dtype=torch.uint8)
    order = torch.zeros(4, dtype=torch.int32)
    buf = torch.zeros(256, dtype=torch.uint8)

    def query(**kw):
        a = dict(rays=rays, hits=hits, ids=ids, geom=geom, order=None, num_indices=None)
        a.update(kw)
        rt.IntersectRaysInstancedMixedCapsules(buf, buf, 0, 2, buf, 3, buf, a["geom"], 2, a["rays"], a["hits"], a["ids"],
                                               a["order"], num_indices=a["num_indices"])

    for bad in (dict(hits=hits[:3]), dict(hits=torch.zeros((4, 8))[:, ::2]), dict(rays=torch.zeros((4, 16))[:, ::2]),
                dict(rays=torch.zeros(33, dtype=torch.uint8)), dict(ids=ids[:3]), dict(ids=torch.zeros(8, dtype=torch.int32)[::2]),
                dict(geom=geom[:31]), dict(geom=torch.zeros(64, dtype=torch.uint8)[::2]), dict(geom=None),
                dict(order=torch.zeros(8, dtype=torch.int32)[::2]), dict(order=order, num_indices=5),
                dict(order=order, hits=hits[:3])):
        with pytest.raises(ValueError):
            query(**bad)
    # an empty batch and an empty index list return before the library is called
    query(rays=rays[:0])
    query(order=order[:0])
    query(order=order, num_indices=0)


def test_geometry_table_entries(rt):
    import torch
    sph = torch.zeros((3, 4), dtype=torch.float32)
    cap = torch.zeros((3, 8), dtype=torch.float32)
    tab = rt.geometry_table([None, (sph, 3), (cap, 3, rt.RT_GEOM_CAPSULES), (cap, 0, 2), (sph, 2, rt.RT_GEOM_SPHERES), (sph, 0)],
                            device="cpu")
    got = tab.numpy().view(rt.GEOMETRY).reshape(-1)
    assert got["kind"].tolist() == [0, 1, 2, 2, 1, 1] and got["count"].tolist() == [0, 3, 3, 0, 2, 0]
    assert got["data"].tolist() == [0, sph.data_ptr(), cap.data_ptr(), cap.data_ptr(), sph.data_ptr(), sph.data_ptr()]
    for bad in ([(cap, 4, 2)],                                         # a short capsule buffer: 32 * n bytes are needed
                [(sph, 2, 2)],                                         # 48 bytes hold one capsule, not two
                [(torch.zeros((3, 16))[:, ::2], 3, 2)],                # not contiguous
                [(cap, 3, 7)], [(cap, 3, 0)], [(cap, 3, 3)],           # an unknown kind; triangles are written as None
                [(sph, 4)], [(sph, 4, 1)]):                            # the sphere checks as before
        with pytest.raises(ValueError):
            rt.geometry_table(bad, device="cpu")


def test_the_constants_are_the_reference_module_s(rt):
    import instance_capsule_ref as icr
    assert icr.RAY == rt.RAY and icr.HIT == rt.HIT and icr.MISS == rt.MISS
    assert (icr.TRIANGLES, icr.SPHERES, icr.CAPSULES) == (rt.RT_GEOM_TRIANGLES, rt.RT_GEOM_SPHERES, rt.RT_GEOM_CAPSULES)
    assert icr.far_capsules().dtype == rt.CAPSULE["p0"].base and icr.far_capsules().shape[1] * 4 == rt.CAPSULE.itemsize
