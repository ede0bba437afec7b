"""CPU test of the instance-motion ABI (rt_prepare_motion_instances, rt_intersect_rays_instanced_motion): the header declares
both and the library exports them, the two 128-byte structs match their numpy dtypes and ctypes mirrors, and every argument
error is refused before any GPU work (the pointers below are never dereferenced: a correct library returns before it touches
them)."""
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
    assert re.search(r"\bint\s+rt_prepare_motion_instances\s*\(", src)
    assert re.search(r"\bint\s+rt_intersect_rays_instanced_motion\s*\(", src)
    assert "rt_prepare_motion_instances" in rt.EXPORTS and "rt_intersect_rays_instanced_motion" in rt.EXPORTS
    L = rt.lib()
    assert L.rt_prepare_motion_instances is not None and L.rt_intersect_rays_instanced_motion is not None
    assert "instance_motion:" in rt.version()
    # the block sits after the instancing block and says what it must
    h = _header()
    assert h.index("---- instancing") < h.index("---- instance motion") < h.index("---- closest-point queries")
    block = h[h.index("---- instance motion"):h.index("typedef struct rt_motion_instance {")]
    for words in ("byte for byte", "opposite sign", "NOT ENTERED BY THIS RAY", "rt_motion_validate", "Out of scope",
                  "a deforming BLAS inside a moving instance", "rotations interpolated as rotations", "rt_cli"):
        assert words in block, words


def test_struct_layouts(rt):
    fields = {"rt_motion_instance": ("_MotionInstance", rt.MOTION_INSTANCE,
                                     {"object_to_world0": 0, "object_to_world1": 48, "blas": 96, "pad": 100}),
              "rt_motion_instance_record": ("_MotionInstanceRecord", rt.MOTION_INSTANCE_RECORD,
                                            {"object_to_world0": 0, "object_to_world1": 48, "blas": 96, "flags": 100,
                                             "spare": 104})}
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name, (mirror, dtype, offsets) in fields.items():
        c = getattr(rt, mirror)
        assert ctypes.sizeof(c) == 128 and dtype.itemsize == 128
        for f, off in offsets.items():
            assert getattr(c, f).offset == off and dtype.fields[f][1] == off, (name, f)
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), src, flags=re.S).group(1)
        assert re.findall(r"(\w+)(?:\[\d+\])?\s*[;,]", body) == list(offsets)
    assert rt.MOTION_INSTANCE["object_to_world0"].shape == (3, 4) and rt.MOTION_INSTANCE["pad"].shape == (7,)
    assert rt.MOTION_INSTANCE_RECORD["spare"].shape == (6,)


def _accel(rt, count=2, **null):
    p = dict(triangles0=FAKE, nodes0=FAKE, triangles1=FAKE, nodes1=FAKE)
    p.update(null)
    return ctypes.byref(rt._MotionAccel(p["triangles0"], p["nodes0"], p["triangles1"], p["nodes1"], 0, count))


def test_prepare_argument_errors(rt):
    p = rt.lib().rt_prepare_motion_instances
    #           instances, n, table, num_blas, proxies0, proxies1, records, status, stream
    good = [FAKE, 3, FAKE_ODD, 2, FAKE, FAKE, FAKE, FAKE_WORD, None]
    for k in (0, 2, 4, 5, 6, 7):                                                   # a null pointer
        a = list(good)
        a[k] = None
        assert p(*a) == -1, k
    for k, bad in ((0, FAKE_ODD), (4, FAKE_ODD), (5, FAKE_ODD), (6, FAKE_ODD), (2, FAKE_WORD), (7, FAKE_BYTE)):   # alignment
        a = list(good)
        a[k] = bad
        assert p(*a) == -1, k
    a = list(good)
    a[3] = 0                                                                        # instances without a table entry
    assert p(*a) == -1
    # the status word is needed even for an empty batch
    assert p(None, 0, None, 0, None, None, None, None, None) == -1
    assert p(None, 0, None, 0, None, None, None, FAKE_BYTE, None) == -1


def test_query_argument_errors(rt):
    q = rt.lib().rt_intersect_rays_instanced_motion
    #            tlas, records, n_inst, table, n_blas, rays, times, hits, ids, n_rays, mode, counters, stream

    def args(**kw):
        a = dict(tlas=_accel(rt), records=FAKE, num_instances=3, table=FAKE_ODD, num_blas=2, rays=FAKE, times=FAKE_WORD,
                 hits=FAKE, ids=FAKE_WORD, num_rays=5, mode=0, counters=None, stream=None)
        a.update(kw)
        return list(a.values())

    for null in ("tlas", "records", "table", "rays", "times", "hits", "ids"):
        assert q(*args(**{null: None})) == -1, null
    assert q(*args(num_blas=0)) == -1
    for field in ("triangles0", "nodes0", "triangles1", "nodes1"):                 # a null TLAS pointer with count > 0
        assert q(*args(tlas=_accel(rt, **{field: 0}))) == -1, field
    assert q(*args(tlas=_accel(rt, count=8))) == -1                                # count > 7
    for name, bad in (("rays", FAKE_ODD), ("hits", FAKE_ODD), ("records", FAKE_ODD), ("table", FAKE_WORD), ("times", FAKE_BYTE),
                      ("ids", FAKE_BYTE)):
        assert q(*args(**{name: bad})) == -1, name
    for mode in (-1, 2, 7):
        assert q(*args(mode=mode)) == -1
    # errors win over an empty batch; an empty batch with valid arguments does nothing
    assert q(*args(num_rays=0, tlas=_accel(rt, count=8))) == -1
    assert q(*args(num_rays=0, times=FAKE_BYTE)) == -1
    assert q(*args(num_rays=0, times=None)) == -1
    assert q(*args(num_rays=0, mode=3)) == -1
    assert q(*args(num_rays=0)) == 0
    assert q(*args(num_rays=0, mode=1, counters=FAKE)) == 0
    # no instances: records and the table may be null; an empty TLAS needs no tree pointers
    assert q(*args(num_rays=0, records=None, table=None, num_instances=0, num_blas=0)) == 0
    assert q(*args(num_rays=0, tlas=_accel(rt, count=0, triangles0=0, nodes0=0, triangles1=0, nodes1=0))) == 0


def test_python_wrappers_refuse_bad_buffers(rt):
    import torch
    rays = torch.zeros((4, 8), dtype=torch.float32)
    hits = torch.zeros((4, 4), dtype=torch.float32)
    ids = torch.zeros(4, dtype=torch.int32)
    times = torch.zeros(4)
    pose = (torch.zeros(64, dtype=torch.uint8), torch.zeros(64, dtype=torch.uint8))
    rec = torch.zeros(2 * 128, dtype=torch.uint8)
    tab = torch.zeros(24, dtype=torch.uint8)

    def query(**kw):
        a = dict(rays=rays, times=times, hits=hits, ids=ids, records=rec)
        a.update(kw)
        rt.IntersectRaysInstancedMotion(pose, pose, 0, 2, a["records"], 2, tab, 1, a["rays"], a["times"], a["hits"], a["ids"])

    for bad in (dict(times=torch.zeros(3)), dict(hits=hits[:3]), dict(ids=ids[:3]), dict(times=torch.zeros(8)[::2]),
                dict(hits=torch.zeros((4, 8))[:, ::2]), dict(rays=torch.zeros((4, 16))[:, ::2]), dict(records=rec[:128]),
                dict(rays=torch.zeros(33, dtype=torch.uint8))):
        with pytest.raises(ValueError):
            query(**bad)
    inst = torch.zeros(2 * 128, dtype=torch.uint8)
    prox = torch.zeros(2 * 36, dtype=torch.uint8)
    status = torch.zeros(4, dtype=torch.uint8)
    for bad in (dict(instances=inst[:200]), dict(proxies0=prox[:36]), dict(proxies1=prox[:71]), dict(records=rec[:128]),
                dict(proxies1=torch.zeros(4 * 36, dtype=torch.uint8)[::2])):
        a = dict(instances=inst, proxies0=prox, proxies1=prox, records=rec)
        a.update(bad)
        with pytest.raises(ValueError):
            rt.PrepareMotionInstances(a["instances"], 2, tab, 1, a["proxies0"], a["proxies1"], a["records"], status)


def test_the_dtypes_are_the_reference_modules(rt):
    import instance_motion_ref as imr
    assert imr.MOTION_INSTANCE == rt.MOTION_INSTANCE
    assert np.zeros(1, rt.MOTION_INSTANCE_RECORD)["flags"][0] == 0
