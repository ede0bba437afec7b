"""CPU test of the instancing ABI (rt_prepare_instances, rt_intersect_rays_instanced): the header declares both entry points, the
rt_instance / rt_instance_record layouts and flags match the Python dtypes, and every argument error is refused before any GPU
work (the pointers below are never dereferenced: a correct library returns before it touches them)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000          # a 16-byte aligned "device pointer" that must never be used


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rt_abi.h")).read(), flags=re.S)


def test_header_declares_the_instancing_entry_points_and_layouts():
    src = _header()
    assert re.search(r"\bint\s+rt_prepare_instances\s*\(\s*const\s+rt_instance\s*\*", src)
    assert re.search(r"\bint\s+rt_intersect_rays_instanced\s*\(\s*const\s+rt_accel\s*\*", src)
    for flag in ("RT_INSTANCE_BAD_BLAS = 1", "RT_INSTANCE_SINGULAR = 2"):
        assert flag in src, flag
    m = re.search(r"typedef struct rt_instance \{(.*?)\} rt_instance;", src, flags=re.S)
    assert m and re.findall(r"(\w+)\s+(\w+)\[?(\d*)\]?;", m.group(1)) == [
        ("float", "object_to_world", "12"), ("uint32_t", "blas", ""), ("uint32_t", "pad", "3")]
    m = re.search(r"typedef struct rt_instance_record \{(.*?)\} rt_instance_record;", src, flags=re.S)
    assert m and re.findall(r"(\w+)\s+(\w+)\[?(\d*)\]?;", m.group(1)) == [
        ("float", "world_to_object", "12"), ("uint32_t", "blas", ""), ("uint32_t", "flags", ""), ("uint32_t", "spare", "2")]


def test_layouts_and_python_names(rt):
    f = rt.INSTANCE.fields
    assert rt.INSTANCE.itemsize == 64 and (f["object_to_world"][1], f["blas"][1], f["pad"][1]) == (0, 48, 52)
    f = rt.INSTANCE_RECORD.fields
    assert rt.INSTANCE_RECORD.itemsize == 64
    assert (f["world_to_object"][1], f["blas"][1], f["flags"][1], f["spare"][1]) == (0, 48, 52, 56)
    f = rt.ACCEL.fields
    assert rt.ACCEL.itemsize == ctypes.sizeof(rt._Accel) == 24 and (f["nodes"][1], f["root"][1], f["count"][1]) == (8, 16, 20)
    assert (rt.RT_INSTANCE_BAD_BLAS, rt.RT_INSTANCE_SINGULAR) == (1, 2)
    for name in ("rt_prepare_instances", "rt_intersect_rays_instanced"):
        assert name in rt.EXPORTS and getattr(rt.lib(), name) is not None
    for name in ("PrepareInstances", "IntersectRaysInstanced", "instance_status", "accel_table"):
        assert callable(getattr(rt, name)), name
    assert "instances:" in rt.version()


def test_prepare_argument_errors(rt):
    L = rt.lib()
    P = L.rt_prepare_instances
    ok = dict(inst=FAKE, n=3, table=FAKE, nb=2, prox=FAKE, rec=FAKE, status=FAKE)

    def call(**kw):
        a = dict(ok, **kw)
        return P(a["inst"], a["n"], a["table"], a["nb"], a["prox"], a["rec"], a["status"], None)

    assert call(status=None) == -1
    assert call(status=FAKE + 2) == -1                      # status not 4-byte aligned
    for k in ("inst", "table", "prox", "rec"):
        assert call(**{k: None}) == -1, k
    for k in ("inst", "prox", "rec"):
        assert call(**{k: FAKE + 8}) == -1, k               # not 16-byte aligned
    assert call(table=FAKE + 4) == -1                       # table not 8-byte aligned
    assert call(nb=0) == -1                                 # instances but no BLAS
    # errors win over an empty input
    assert call(n=0, status=None) == -1
    assert call(n=0, status=FAKE + 1) == -1


def test_query_argument_errors(rt):
    L = rt.lib()
    Q = L.rt_intersect_rays_instanced

    def call(tlas_count=2, tlas_nodes=FAKE, tlas_tris=FAKE, rec=FAKE, n_inst=3, table=FAKE, nb=2, rays=FAKE, hits=FAKE,
             ids=FAKE, n=5, mode=0, tlas=True):
        a = ctypes.byref(rt._Accel(tlas_tris, tlas_nodes, 0, tlas_count)) if tlas else None
        return Q(a, rec, n_inst, table, nb, rays, hits, ids, n, mode, 0, None, None)

    assert call(tlas=False) == -1
    assert call(tlas_count=8) == -1
    assert call(tlas_nodes=0) == -1
    assert call(tlas_tris=0) == -1
    for k in ("rec", "table", "rays", "hits", "ids"):
        assert call(**{k: None}) == -1, k
    for k in ("rec", "rays", "hits"):
        assert call(**{k: FAKE + 8}) == -1, k
    assert call(table=FAKE + 4) == -1
    assert call(ids=FAKE + 2) == -1
    for mode in (-1, 2, 7):
        assert call(mode=mode) == -1
    assert call(nb=0) == -1                                 # instances but no BLAS
    # errors win over an empty batch; an empty batch with valid arguments does nothing
    assert call(n=0, tlas_count=8) == -1
    assert call(n=0, nb=0) == -1
    assert call(n=0) == 0
    assert call(n=0, mode=1) == 0
    # an empty scene (no instances, an empty TLAS): arguments are valid, nothing is read
    assert call(n=0, n_inst=0, table=None, nb=0, rec=None, tlas_count=0, tlas_nodes=0, tlas_tris=0) == 0


def test_reference_prepare_restatement():
    """tests/instance_ref.py on a hand-worked case: the identity and a translation give the padded box exactly"""
    import numpy as np
    import instance_ref as ir
    inst = ir.instance_array([np.eye(3, 4), np.hstack([np.eye(3), [[4.0], [0.0], [-2.0]]]), np.zeros((3, 4))], [0, 0, 1])
    box = (np.array([-1, 0, 1], np.float32), np.array([1, 2, 3], np.float32))
    prox, inv, flags = ir.prepare(inst, [box, None])
    pad = np.float32(3 * 2.0 ** -12)
    assert (prox[0, :3] == np.array([-1, 0, 1], np.float32) - pad).all()
    assert (prox[0, 3:6] == np.array([1, 2, 3], np.float32) + pad).all()
    assert (inv[0] == np.eye(3, 4)).all() and (inv[1, :, 3] == [-4, 0, 2]).all()
    assert flags.tolist() == [0, 0, ir.BAD_BLAS | ir.SINGULAR] and (prox[2] == 0).all()
    assert ((prox[:2, 6:] >= prox[:2, :3]) & (prox[:2, 6:] <= prox[:2, 3:6])).all()
