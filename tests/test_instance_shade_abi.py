"""CPU test of the instanced deferred-shading ABI (rt_shade_frame_instanced): the header declares the entry point, rt_shade_geometry
and RT_SHADE_RENORMALIZE, the library exports the call, the struct is the 32 bytes the binding's dtype says, every argument
error is refused before any GPU work (the pointers below are never dereferenced: a correct library returns before it touches
them), and the Python wrapper refuses bad buffers."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000          # a 16-byte aligned "device pointer" that must never be used


def _header():
    return open(os.path.join(ROOT, "include", "rt_abi.h")).read()


def test_header_declares_the_entry_point(rt):
    h = _header()
    src = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    assert re.search(r"\bint\s+rt_shade_frame_instanced\s*\(\s*const\s+rt_scene\s*\*\s*scene\s*,\s*const\s+rt_shade_geometry\s*\*", src)
    assert re.search(r"enum\s*\{\s*RT_SHADE_RENORMALIZE\s*=\s*1\s*\}", src)
    assert "rt_shade_frame_instanced" in rt.EXPORTS and rt.lib().rt_shade_frame_instanced is not None
    assert rt.RT_SHADE_RENORMALIZE == 1
    for name in ("ShadeFrameInstanced", "shade_geometry_table"):
        assert callable(getattr(rt, name)), name
    assert "instance_shade:" in rt.version()
    # the block sits after the deferred-shading block and says what it must
    assert h.index("---- deferred shading") < h.index("---- instanced deferred shading") < h.index("typedef struct rt_shade_geometry")
    block = h[h.index("---- instanced deferred shading"):h.index("typedef struct rt_shade_geometry")]
    for words in ("rt_generate_camera_rays -> rt_intersect_rays_instanced -> rt_generate_shadow_rays(num_triangles = RT_MISS)",
                  "rt_intersect_rays_instanced(any hit) -> rt_shade_frame_instanced", "rt_intersect_rays_instanced_filtered",
                  "rt_intersect_rays_instanced_motion", "pose they want shaded", "records[k].flags == 0",
                  "((M[r][0]*x + M[r][1]*y) + M[r][2]*z) + M[r][3]", "(W[0][r]*nx + W[1][r]*ny) + W[2][r]*nz",
                  "RT_SHADE_RENORMALIZE", "1.0f / sqrtf(l2)", "material_base", "instance_materials[k] >= 0",
                  "shadow_instance_ids[i] < num_instances", "MIRRORED", "flattened scene", "byte for byte", "-0 + 0 = +0",
                  "Out of scope", "sphere BLASes", "host mirror", "rt_cli", "hipGraph-capturable", "num_instances = 0",
                  "unknown flag bits", "16-byte aligned", "4-byte aligned"):
        assert words in block, words


def test_struct_layout(rt):
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    body = re.search(r"typedef struct rt_shade_geometry \{(.*?)\} rt_shade_geometry;", src, flags=re.S).group(1)
    assert re.sub(r"\s+", " ", body).strip() == ("const rt_triangle* triangles; const rt_attributes* attributes; "
                                                  "uint32_t num_triangles; int32_t material_base; uint32_t pad[2];")
    f = rt.SHADE_GEOMETRY.fields
    assert rt.SHADE_GEOMETRY.itemsize == 32                                          # sizeof(rt_shade_geometry)
    assert (f["triangles"][1], f["attributes"][1], f["num_triangles"][1], f["material_base"][1]) == (0, 8, 16, 20)
    assert f["material_base"][0] == np.dtype("<i4")

    class Geometry(ctypes.Structure):                                                # the C layout on this ABI
        _fields_ = [("triangles", ctypes.c_void_p), ("attributes", ctypes.c_void_p), ("num_triangles", ctypes.c_uint32),
                    ("material_base", ctypes.c_int32), ("pad", ctypes.c_uint32 * 2)]
    assert ctypes.sizeof(Geometry) == 32
    assert (Geometry.triangles.offset, Geometry.attributes.offset, Geometry.num_triangles.offset,
            Geometry.material_base.offset) == (0, 8, 16, 20)
    import instance_shade_ref as isr
    assert isr.SHADE_GEOMETRY == rt.SHADE_GEOMETRY and isr.ATTRIBUTES == rt.ATTRIBUTES and isr.HIT == rt.HIT
    assert isr.MISS == rt.MISS


def _call(rt, scene=True, materials=FAKE, num_materials=4, textures=FAKE, num_textures=2, geom=FAKE, nb=2, inst=FAKE, rec=FAKE,
          ni=3, imat=None, rays=FAKE, hits=FAKE, ids=FAKE, sids=FAKE, w=8, h=8, spp=1, layout=0, mode=0, flags=1, rgba=FAKE):
    s = rt._Scene(0, materials, textures, 0, (ctypes.c_float * 3)(0, 0, 0), 0, num_materials, num_textures)
    return rt.lib().rt_shade_frame_instanced(ctypes.byref(s) if scene else None, geom, nb, inst, rec, ni, imat, rays, hits, ids,
                                             sids, w, h, spp, layout, mode, flags, rgba, None)


@pytest.mark.parametrize("mode", (0, 3, 4, 5, 6, 7, 8))
def test_argument_errors(rt, mode):
    """every error wins over an empty frame (w * h = 0), where valid arguments do nothing"""
    def call(**kw):
        a, b = _call(rt, mode=mode, **kw), _call(rt, mode=mode, w=0, **kw)
        assert a == b, kw
        return a

    assert _call(rt, mode=mode, w=0) == 0 and _call(rt, mode=mode, h=0) == 0
    assert call(scene=False) == -1
    for k in ("rays", "hits", "ids", "rgba", "geom", "inst", "rec"):
        assert call(**{k: None}) == -1, k
    for k in ("geom", "inst", "rec", "rays", "hits"):
        assert call(**{k: FAKE + 8}) == -1, k                    # not 16-byte aligned
        assert call(**{k: FAKE + 4}) == -1, k
    for k in ("ids", "sids", "imat", "rgba"):
        assert call(**{k: FAKE + 2}) == -1, k                    # not 4-byte aligned
        assert call(**{k: FAKE + 1}) == -1, k
    assert _call(rt, mode=mode, w=0, imat=FAKE + 4, ids=FAKE + 4, sids=FAKE + 4, rgba=FAKE + 4) == 0   # 4-byte aligned will do
    for spp in (0, 2, 3, 8, 32):
        assert call(spp=spp) == -1
    for layout in (-1, 2):
        assert call(layout=layout) == -1
    for flags in (2, 3, 0x80000000, 0xFFFFFFFF):
        assert call(flags=flags) == -1                           # unknown flag bits
    assert _call(rt, mode=mode, w=0, flags=0) == 0
    assert call(nb=0) == -1                                      # instances but no BLAS
    # an empty scene: no instances, the three arrays may be null
    assert _call(rt, mode=mode, w=0, ni=0, nb=0, geom=None, inst=None, rec=None) == 0
    # materials and textures as rt_shade_frame requires them
    def refused(expected, **kw):                                 # (a call that is not refused is only made with w = 0)
        assert _call(rt, mode=mode, w=0, **kw) == (-1 if expected else 0), kw
        if expected:
            assert _call(rt, mode=mode, **kw) == -1, kw

    refused(mode != 0, materials=None)
    refused(mode != 0, num_materials=0)
    refused(mode in (4, 6, 7, 8), textures=None)
    refused(False, textures=None, num_textures=0)
    refused(mode == 8, sids=None)                                # mode 8 needs the shadow instance ids


def test_render_types_without_records(rt):
    for mode in (1, 2):
        assert _call(rt, mode=mode) == -2 and _call(rt, mode=mode, w=0) == -2       # RT_ERR_UNSUPPORTED, nothing runs
    for mode in (-1, 9, 100):
        assert _call(rt, mode=mode) == -1 and _call(rt, mode=mode, w=0) == -1


def test_python_wrapper_refuses_bad_buffers(rt):
    import torch
    w, h = 8, 4
    n = w * h
    good = dict(geometry=torch.zeros(2 * 32, dtype=torch.uint8), instances=torch.zeros(3 * 64, dtype=torch.uint8),
                records=torch.zeros(3 * 64, dtype=torch.uint8), rays=torch.zeros((n, 8), dtype=torch.float32),
                hits=torch.zeros((n, 4), dtype=torch.float32), instance_ids=torch.zeros(n, dtype=torch.int32),
                rgba8=torch.zeros(n * 4, dtype=torch.uint8))

    def shade(kw=None, **opt):
        a = dict(good)
        a.update(kw or {})
        rt.ShadeFrameInstanced(a["geometry"], 2, a["instances"], a["records"], 3, a["rays"], a["hits"], a["instance_ids"],
                               a["rgba8"], (w, h), **opt)

    for bad in (dict(rays=good["rays"][:n - 1]), dict(hits=good["hits"][:n - 1]), dict(instance_ids=good["instance_ids"][:n - 1]),
                dict(rgba8=good["rgba8"][:4 * n - 1]), dict(geometry=good["geometry"][:63]), dict(instances=good["instances"][:191]),
                dict(records=good["records"][:191]), dict(hits=torch.zeros((n, 8))[:, ::2]),
                dict(instance_ids=torch.zeros(2 * n, dtype=torch.int32)[::2]), dict(geometry=torch.zeros(128, dtype=torch.uint8)[::2])):
        with pytest.raises(ValueError):
            shade(bad)
    with pytest.raises(ValueError):
        shade(shadow_instance_ids=torch.zeros(n - 1, dtype=torch.int32), render_type=8)
    with pytest.raises(ValueError):
        shade(instance_materials=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError):
        shade(instance_materials=torch.zeros(3, dtype=torch.int64))
    # the tiled layout asks for whole tiles
    with pytest.raises(ValueError):
        shade(tiled=True)                                        # 8 x 4 tiled needs 64 records
    # shade_geometry_table: (triangles, attributes, count[, base]) or None per BLAS; short buffers are refused
    tris = torch.zeros((5, 9), dtype=torch.float32)
    attrs = torch.zeros(5 * 72, dtype=torch.uint8)
    tab = rt.shade_geometry_table([(tris, attrs, 5), None, (tris, attrs, 4, -3)], device="cpu")
    got = tab.numpy().view(rt.SHADE_GEOMETRY).reshape(-1)
    assert got["triangles"].tolist() == [tris.data_ptr(), 0, tris.data_ptr()]
    assert got["attributes"].tolist() == [attrs.data_ptr(), 0, attrs.data_ptr()]
    assert got["num_triangles"].tolist() == [5, 0, 4] and got["material_base"].tolist() == [0, 0, -3]
    assert (got["pad"] == 0).all()
    for bad in ((tris, attrs, 6), (tris[:4], attrs, 5), (tris, attrs[:359], 5), (torch.zeros((5, 18))[:, ::2], attrs, 5)):
        with pytest.raises(ValueError):
            rt.shade_geometry_table([bad], device="cpu")
