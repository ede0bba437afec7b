"""CPU test of the motion-query ABI (rt_intersect_rays_motion, rt_motion_validate): the header declares both and the library
exports them, rt_motion_accel's layout matches the ctypes mirror, and every argument error is refused before any GPU work
(the pointers below are never dereferenced: a correct library returns before it touches them)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000          # a 16-byte aligned "device pointer" that must never be used
FAKE_ODD = FAKE + 8     # 8-byte aligned only
FAKE_BYTE = FAKE + 2    # 2-byte aligned only


def _header():
    return open(os.path.join(ROOT, "include", "rt_abi.h")).read()


def test_header_declares_the_motion_entry_points(rt):
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"\bint\s+rt_intersect_rays_motion\s*\(", src)
    assert re.search(r"\bint\s+rt_motion_validate\s*\(", src)
    assert "RT_MOTION_TOPOLOGY_MISMATCH = 1" in src and rt.RT_MOTION_TOPOLOGY_MISMATCH == 1
    assert "rt_intersect_rays_motion" in rt.EXPORTS and "rt_motion_validate" in rt.EXPORTS
    L = rt.lib()
    assert L.rt_intersect_rays_motion is not None and L.rt_motion_validate is not None
    assert "motion:" in rt.version()
    # what the header must say
    block = _header()[_header().index("motion-blur ray queries"):]
    block = block[:block.index("rt_intersect_rays_motion(const")]
    assert "main.cu:125-192" in block and "identity-refitted" in block and "Out of scope" in block


def test_motion_accel_layout(rt):
    m = rt._MotionAccel
    assert ctypes.sizeof(m) == 40
    assert [getattr(m, f).offset for f in ("triangles0", "nodes0", "triangles1", "nodes1", "root", "count")] == [0, 8, 16, 24, 32, 36]
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    body = re.search(r"typedef struct rt_motion_accel \{(.*?)\} rt_motion_accel;", src, flags=re.S).group(1)
    assert re.findall(r"(\w+)\s*[;,]", body) == ["triangles0", "nodes0", "triangles1", "nodes1", "root", "count"]


def _accel(rt, count=2, **null):
    p = dict(triangles0=FAKE, nodes0=FAKE, triangles1=FAKE, nodes1=FAKE)
    p.update(null)
    return ctypes.byref(rt._MotionAccel(p["triangles0"], p["nodes0"], p["triangles1"], p["nodes1"], 0, count))


def test_intersect_rays_motion_argument_errors(rt):
    q = rt.lib().rt_intersect_rays_motion
    assert q(None, FAKE, FAKE, FAKE, 5, 0, None, None) == -1                       # no accel
    assert q(_accel(rt), None, FAKE, FAKE, 5, 0, None, None) == -1                 # no rays
    assert q(_accel(rt), FAKE, None, FAKE, 5, 0, None, None) == -1                 # no times
    assert q(_accel(rt), FAKE, FAKE, None, 5, 0, None, None) == -1                 # no hits
    for field in ("triangles0", "nodes0", "triangles1", "nodes1"):                 # a null tree pointer with count > 0
        assert q(_accel(rt, **{field: 0}), FAKE, FAKE, FAKE, 5, 0, None, None) == -1, field
    assert q(_accel(rt, count=8), FAKE, FAKE, FAKE, 5, 0, None, None) == -1        # count > 7
    assert q(_accel(rt), FAKE_ODD, FAKE, FAKE, 5, 0, None, None) == -1             # rays not 16-byte aligned
    assert q(_accel(rt), FAKE, FAKE, FAKE_ODD, 5, 0, None, None) == -1             # hits not 16-byte aligned
    assert q(_accel(rt), FAKE, FAKE_BYTE, FAKE, 5, 0, None, None) == -1            # times not 4-byte aligned
    for mode in (-1, 2, 7):
        assert q(_accel(rt), FAKE, FAKE, FAKE, 5, mode, None, None) == -1
    # errors win over an empty batch; an empty batch with valid arguments does nothing
    assert q(_accel(rt, count=8), FAKE, FAKE, FAKE, 0, 0, None, None) == -1
    assert q(_accel(rt), FAKE, FAKE_BYTE, FAKE, 0, 0, None, None) == -1
    assert q(_accel(rt), FAKE, FAKE, FAKE, 0, 0, None, None) == 0
    assert q(_accel(rt), FAKE, FAKE + 4, FAKE, 0, 1, FAKE, None) == 0              # times need 4-byte alignment only
    # an empty tree needs no tree pointers
    assert q(_accel(rt, count=0, triangles0=0, nodes0=0, triangles1=0, nodes1=0), FAKE, FAKE, FAKE, 0, 0, None, None) == 0


def test_motion_validate_argument_errors(rt):
    v = rt.lib().rt_motion_validate
    assert v(None, 10, FAKE, None) == -1
    assert v(_accel(rt), 10, None, None) == -1
    assert v(_accel(rt), 10, FAKE_BYTE, None) == -1
    for field in ("triangles0", "nodes0", "triangles1", "nodes1"):
        assert v(_accel(rt, **{field: 0}), 10, FAKE, None) == -1, field
        assert v(_accel(rt, **{field: FAKE_ODD}), 10, FAKE, None) == -1, field
    assert v(_accel(rt, count=8), 10, FAKE, None) == -1
    assert v(_accel(rt), (1 << 27), FAKE, None) < 0                                # beyond RT_REFIT_MAX_TRIANGLES


def test_python_wrappers_refuse_bad_buffers(rt):
    import pytest
    import torch
    rays = torch.zeros((4, 8), dtype=torch.float32)
    hits = torch.zeros((4, 4), dtype=torch.float32)
    pose = (torch.zeros(64, dtype=torch.uint8), torch.zeros(64, dtype=torch.uint8))
    with pytest.raises(ValueError):
        rt.IntersectRaysMotion(pose, pose, 0, 2, rays, torch.zeros(3), hits)       # a time is missing
    with pytest.raises(ValueError):
        rt.IntersectRaysMotion(pose, pose, 0, 2, rays, torch.zeros(4), hits[:3])
    with pytest.raises(ValueError):
        rt.IntersectRaysMotion(pose, pose, 0, 2, rays, torch.zeros(8)[::2], hits)  # not contiguous
