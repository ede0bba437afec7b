"""CPU test of the ray-query ABI (rt_intersect_rays, rt_generate_camera_rays): the header declares both, the rt_ray / rt_hit
layouts match the Python dtypes, and every argument error is refused before any GPU work (the pointers below are never
dereferenced: a correct library returns before it touches them)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000          # a 16-byte aligned "device pointer" that must never be used
FAKE_ODD = FAKE + 8     # 8-byte aligned only


def _header():
    return open(os.path.join(ROOT, "include", "rt_abi.h")).read()


def test_header_declares_the_ray_query_entry_points():
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"\bint\s+rt_intersect_rays\s*\(", src)
    assert re.search(r"\bint\s+rt_generate_camera_rays\s*\(", src)
    assert re.search(r"#define\s+RT_MISS\s+0xFFFFFFFFu", src)
    for name in ("RT_RAY_CLOSEST_HIT = 0", "RT_RAY_ANY_HIT = 1", "RT_RAYS_ROW_MAJOR = 0", "RT_RAYS_TILED = 1"):
        assert name in src, name


def test_ray_and_hit_layouts(rt):
    assert rt.RAY.itemsize == 32 and rt.HIT.itemsize == 16
    f = rt.RAY.fields
    assert (f["origin"][1], f["tmin"][1], f["dir"][1], f["tmax"][1]) == (0, 12, 16, 28)
    f = rt.HIT.fields
    assert (f["t"][1], f["primitive_id"][1], f["u"][1], f["v"][1]) == (0, 4, 8, 12)
    assert rt.MISS == 0xFFFFFFFF and (rt.kClosestHit, rt.kAnyHit) == (0, 1) and (rt.kRaysRowMajor, rt.kRaysTiled) == (0, 1)
    assert "rt_intersect_rays" in rt.EXPORTS and "rt_generate_camera_rays" in rt.EXPORTS
    assert "rays:" in rt.version()


def _accel(rt, count=2, nodes=FAKE, triangles=FAKE):
    return ctypes.byref(rt._Accel(triangles, nodes, 0, count))


def test_intersect_rays_argument_errors(rt):
    L = rt.lib()
    ok = dict(rays=FAKE, hits=FAKE)
    assert L.rt_intersect_rays(None, FAKE, FAKE, 5, 0, 0, None, None) == -1                   # no accel
    assert L.rt_intersect_rays(_accel(rt), None, FAKE, 5, 0, 0, None, None) == -1            # no rays
    assert L.rt_intersect_rays(_accel(rt), FAKE, None, 5, 0, 0, None, None) == -1            # no hits
    assert L.rt_intersect_rays(_accel(rt, nodes=0), FAKE, FAKE, 5, 0, 0, None, None) == -1   # a tree without nodes
    assert L.rt_intersect_rays(_accel(rt, triangles=0), FAKE, FAKE, 5, 0, 0, None, None) == -1
    assert L.rt_intersect_rays(_accel(rt, count=8), FAKE, FAKE, 5, 0, 0, None, None) == -1   # count > 7
    for mode in (-1, 2, 7):
        assert L.rt_intersect_rays(_accel(rt), FAKE, FAKE, 5, mode, 0, None, None) == -1
    assert L.rt_intersect_rays(_accel(rt), FAKE_ODD, FAKE, 5, 0, 0, None, None) == -1        # rays not 16-byte aligned
    assert L.rt_intersect_rays(_accel(rt), FAKE, FAKE_ODD, 5, 0, 0, None, None) == -1        # hits not 16-byte aligned
    # errors win over an empty batch; an empty batch with valid arguments does nothing
    assert L.rt_intersect_rays(_accel(rt, count=8), FAKE, FAKE, 0, 0, 0, None, None) == -1
    assert L.rt_intersect_rays(_accel(rt), ok["rays"], ok["hits"], 0, 0, 0, None, None) == 0
    assert L.rt_intersect_rays(_accel(rt), FAKE, FAKE, 0, 1, 10_000_000, FAKE, None) == 0


def test_generate_camera_rays_argument_errors(rt):
    L = rt.lib()
    assert L.rt_generate_camera_rays(None, 8, 8, 1, 0, FAKE, None) == -1
    assert L.rt_generate_camera_rays(FAKE, 8, 8, 1, 0, None, None) == -1
    assert L.rt_generate_camera_rays(FAKE, 8, 8, 1, 0, FAKE_ODD, None) == -1
    for layout in (-1, 2):
        assert L.rt_generate_camera_rays(FAKE, 8, 8, 1, layout, FAKE, None) == -1
    for spp in (0, 2, 3, 8, 17):
        assert L.rt_generate_camera_rays(FAKE, 8, 8, spp, 0, FAKE, None) == -1
    for w, h in ((0, 8), (8, 0), (0, 0)):
        assert L.rt_generate_camera_rays(FAKE, w, h, 4, 1, FAKE, None) == 0
    assert L.rt_generate_camera_rays(FAKE, 0, 8, 3, 1, FAKE, None) == -1       # errors win over an empty frame


def test_ray_counts(rt):
    assert rt.CameraRayCount(1920, 1080) == 1920 * 1080
    assert rt.CameraRayCount(1920, 1080, tiled=True) == 240 * 135 * 64
    assert rt.CameraRayCount(13, 9, spp=4, tiled=True) == 2 * 2 * 4 * 64
    assert rt.CameraRayCount(13, 9, spp=16) == 13 * 9 * 16
