"""CPU test of the deferred-shading ABI (rt_generate_shadow_rays, rt_shade_frame): the header declares the two, the Python
binding lists them, and every argument error is refused before any GPU work (the pointers below are never dereferenced: a
correct library returns before it touches them)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000          # a 256-byte aligned "device pointer" that must never be used
FAKE_8 = FAKE + 8       # 8-byte aligned only
FAKE_2 = FAKE + 2       # 2-byte aligned only
NAMES = ("rt_generate_shadow_rays", "rt_shade_frame")
SUPPORTED = (0, 3, 4, 5, 6, 7, 8)


def test_header_declares_the_shading_entry_points(rt):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rt_abi.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in rt.EXPORTS and getattr(rt.lib(), name) is not None, name
    assert callable(rt.GenerateShadowRays) and callable(rt.ShadeFrame)
    assert "shade:" in rt.version()


def _light():
    return (ctypes.c_float * 3)(1.0, 2.0, 3.0)


def test_generate_shadow_rays_argument_errors(rt):
    f = rt.lib().rt_generate_shadow_rays        # (rays, hits, num_rays, num_triangles, light, shadow_rays, stream)
    li = _light()
    assert f(None, FAKE, 5, 9, li, FAKE, None) == -1
    assert f(FAKE, None, 5, 9, li, FAKE, None) == -1
    assert f(FAKE, FAKE, 5, 9, None, FAKE, None) == -1
    assert f(FAKE, FAKE, 5, 9, li, None, None) == -1
    assert f(FAKE_8, FAKE, 5, 9, li, FAKE, None) == -1                 # rays not 16-byte aligned
    assert f(FAKE, FAKE_8, 5, 9, li, FAKE, None) == -1                 # hits not 16-byte aligned
    assert f(FAKE, FAKE, 5, 9, li, FAKE_8, None) == -1                 # shadow_rays not 16-byte aligned
    # errors win over an empty batch; an empty batch with valid arguments does nothing
    assert f(FAKE, FAKE_8, 0, 9, li, FAKE, None) == -1
    assert f(FAKE, FAKE, 0, 9, li, FAKE, None) == 0
    assert f(FAKE, FAKE, 0, 0, li, FAKE + 16, None) == 0


def _scene(rt, attributes=FAKE, materials=FAKE, textures=FAKE, num_materials=4, num_textures=5):
    return ctypes.byref(rt._Scene(attributes, materials, textures, 0, _light(), 100, num_materials, num_textures))


def _shade(rt, scene="default", tris=FAKE, n=100, rays=FAKE, hits=FAKE, shadow=FAKE, w=16, h=8, spp=1, layout=0, mode=0,
           rgba=FAKE):
    # (scene, triangles, num_triangles, rays, hits, shadow_hits, w, h, spp, layout, render_type, rgba8, stream)
    return rt.lib().rt_shade_frame(_scene(rt) if scene == "default" else scene, tris, n, rays, hits, shadow, w, h, spp, layout,
                                   mode, rgba, None)


def test_shade_frame_argument_errors(rt):
    for mode in SUPPORTED:
        assert _shade(rt, scene=None, mode=mode) == -1
        assert _shade(rt, tris=None, mode=mode) == -1
        assert _shade(rt, rays=None, mode=mode) == -1
        assert _shade(rt, hits=None, mode=mode) == -1
        assert _shade(rt, rgba=None, mode=mode) == -1
        assert _shade(rt, rays=FAKE_8, mode=mode) == -1                # rays not 16-byte aligned
        assert _shade(rt, hits=FAKE_8, mode=mode) == -1                # hits not 16-byte aligned
        assert _shade(rt, rgba=FAKE_2, mode=mode) == -1                # rgba8 not 4-byte aligned
        assert _shade(rt, tris=FAKE_2, mode=mode) == -1                # triangles not 4-byte aligned
        for spp in (0, 2, 3, 8, 32):
            assert _shade(rt, spp=spp, mode=mode) == -1
        for layout in (-1, 2, 5):
            assert _shade(rt, layout=layout, mode=mode) == -1
    for mode in (-1, 9, 100):
        assert _shade(rt, mode=mode) == -1
    assert _shade(rt, mode=8, shadow=None) == -1                       # mode 8 needs the shadow records
    for mode in (0, 3, 4, 5, 6, 7):
        assert _shade(rt, mode=mode, shadow=None, w=0) == 0            # ... the others ignore them
    # the surface modes need attributes and materials, as rt_trace does
    for mode in (3, 4, 5, 6, 7, 8):
        assert _shade(rt, scene=_scene(rt, attributes=None), mode=mode) == -1
        assert _shade(rt, scene=_scene(rt, materials=None), mode=mode) == -1
        assert _shade(rt, scene=_scene(rt, num_materials=0), mode=mode) == -1
    assert _shade(rt, scene=_scene(rt, textures=None), mode=6) == -1   # textures counted but not given
    assert _shade(rt, scene=_scene(rt, attributes=None, materials=None, textures=None), mode=0, w=0) == 0


def test_test_count_render_types_are_unsupported(rt):
    for mode in (1, 2):
        assert _shade(rt, mode=mode) == -2
        assert _shade(rt, mode=mode, w=0) == -2
        assert rt.lib().rt_error_string(-2).decode() == "unsupported option"


def test_empty_frames_run_nothing(rt):
    for mode in SUPPORTED:
        for w, h in ((0, 8), (16, 0), (0, 0)):
            for layout in (0, 1):
                for spp in (1, 4, 16):
                    assert _shade(rt, w=w, h=h, layout=layout, spp=spp, mode=mode) == 0
        assert _shade(rt, w=0, rays=FAKE_8, mode=mode) == -1            # errors win over an empty frame
        assert _shade(rt, w=0, tris=FAKE + 4, rgba=FAKE + 4, mode=mode) == 0
