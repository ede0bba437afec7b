"""GPU tests of instanced deferred shading (rt_shade_frame_instanced) -- frames from the records of the instanced ray query.

A. the frame equals rt_shade_frame's on the FLATTENED scene (tests/instance_shade_ref.py: numpy-made corners, normals, material
   ids and remapped records), byte for byte: seven instances of two BLASes, records from the real instanced chain, seven modes,
   both layouts, spp 1 / 4 / 16, two frame sizes, renormalisation on and off;
B. one identity instance without renormalisation equals rt_trace's frame on the BLAS, byte for byte;
C. the transform against float64: tests/shade_ref.py's reference on float64-placed corners and inverse-transpose unit normals,
   under its own tolerances and mask bounds;
D. edges: every kind of record that must shade as a miss, guard bytes, edge tiles, tiny scenes, no instances, material ids per
   pixel on the 251-material soup;
E. prepare + TLAS build + the five-call chain in one HIP graph, replayed after the instances are rewritten in place."""
import numpy as np
import pytest

import instance_ref as ir
import instance_shade_ref as isr
import shade_ref
import texture_scene
from test_gpu_instances import Instanced
from test_gpu_shade_frame import _assert_same, _trace
from test_gpu_shading_trees import _gpu_tree

pytestmark = pytest.mark.gpu

MODES = (0, 3, 4, 5, 6, 7, 8)
SIZES = ((160, 100), (130, 101))
MISS_RGBA = {m: (255, 0, 255, 255) if m == 4 else (0, 0, 0, 255) for m in MODES}


class Blases:
    """the device side of a list of BLASes: built trees, the BLAS table entries, the shading table, materials and textures"""

    def __init__(self, rt, tris, attrs, bases, kinds, materials, textures):
        self.rt, self.tris, self.attrs, self.bases = rt, list(tris), list(attrs), list(bases)
        self.trees = [_gpu_tree(rt, t, kind) for t, kind in zip(tris, kinds)]
        self.entries = [(g["inp"].triangles_out, g["inp"].nodes_out, root, count) for g, root, count in self.trees]
        self.dev_attrs = [rt.to_device(np.ascontiguousarray(a)) for a in attrs]
        self.table_entries = [(g[0]["inp"].triangles_in, a, t.shape[0], b)
                              for g, a, t, b in zip(self.trees, self.dev_attrs, tris, bases)]
        self.geometry = rt.shade_geometry_table(self.table_entries)
        self.materials = materials
        self.kw = dict(materials=rt.to_device(materials), num_materials=materials.shape[0],
                       textures=rt.DeviceTextures(textures) if textures else None)


def _chain(rt, sc, cam, light, w, h, spp=1, tiled=False, shadows=True, bufs=None, stream=None):
    """camera rays -> instanced closest hit -> shadow rays (num_triangles = RT_MISS) -> instanced any hit"""
    import torch
    n = rt.CameraRayCount(w, h, spp, tiled)
    if bufs is None:
        f = dict(dtype=torch.float32, device="cuda")
        bufs = dict(rays=torch.zeros((n, 8), **f), hits=torch.zeros((n, 4), **f), srays=torch.zeros((n, 8), **f),
                    shits=torch.zeros((n, 4), **f), ids=torch.zeros(n, dtype=torch.int32, device="cuda"),
                    sids=torch.full((n,), -1, dtype=torch.int32, device="cuda"))
    rt.GenerateCameraRays(cam, w, h, bufs["rays"], spp=spp, tiled=tiled, stream=stream)
    sc.query(bufs["rays"], bufs["hits"], bufs["ids"], stream=stream)
    if shadows:
        rt.GenerateShadowRays(bufs["rays"], bufs["hits"], rt.MISS, light, bufs["srays"], stream=stream)
        sc.query(bufs["srays"], bufs["shits"], bufs["sids"], any_hit=True, stream=stream)
    return bufs


def _shade(rt, bl, sc, rec, w, h, mode, light, spp=1, tiled=False, renormalize=True, instance_materials=None, rgba=None,
           stream=None, geometry=None, num_blas=None, records=None, hits=None, ids=None, num_instances=None):
    import torch
    own = rgba is None
    if own:
        rgba = torch.zeros(w * h * 4, dtype=torch.uint8, device="cuda")
    rt.ShadeFrameInstanced(bl.geometry if geometry is None else geometry, len(bl.entries) if num_blas is None else num_blas,
                           sc.instances, sc.records if records is None else records, sc.n if num_instances is None else num_instances,
                           rec["rays"], rec["hits"] if hits is None else hits, rec["ids"] if ids is None else ids, rgba, (w, h),
                           render_type=mode, spp=spp, tiled=tiled, renormalize=renormalize, instance_materials=instance_materials,
                           shadow_instance_ids=rec["sids"] if mode == 8 else None, light=light, stream=stream, **bl.kw)
    if not own:
        return None
    torch.cuda.synchronize()
    return rgba.cpu().numpy().reshape(h, w, 4)


def _words(rt, a):
    """a numpy array of 32-bit words as a device int32 tensor"""
    import torch
    return rt.to_device(np.ascontiguousarray(a)).view(torch.int32)


def _host(t, dtype):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy().reshape(-1).view(dtype).copy()


class Flat:
    """the flattened scene on the device, and rt_shade_frame on it with remapped records"""

    def __init__(self, rt, bl, instances, records, instance_materials, renormalize, tris=None, attrs=None):
        self.rt, self.bl = rt, bl
        self.world, self.at, self.base = isr.flatten(bl.tris if tris is None else tris, bl.attrs if attrs is None else attrs,
                                                     bl.bases, instances, records, instance_materials, renormalize)
        self.n = self.world.shape[0]
        self.num_instances = len(instances)
        self.d_world = rt.to_device(self.world if self.n else np.zeros((1, 9), np.float32))
        self.d_at = rt.to_device(self.at if self.n else np.zeros(1, isr.ATTRIBUTES))

    def records(self, hits, ids, sids):
        """host instanced records -> the device records of the flattened scene"""
        rt = self.rt
        return rt.to_device(isr.remap(hits, ids, self.base)), rt.to_device(isr.remap_shadow(sids, self.num_instances))

    def shade(self, rays, flat_hits, flat_shits, w, h, mode, light, spp=1, tiled=False):
        import torch
        rt = self.rt
        rgba = torch.zeros(w * h * 4, dtype=torch.uint8, device="cuda")
        rt.ShadeFrame(self.d_world, self.n, rays, flat_hits, rgba, (w, h), render_type=mode, spp=spp, tiled=tiled,
                      shadow_hits=flat_shits if mode == 8 else None, attributes=self.d_at, light=light, **self.bl.kw)
        torch.cuda.synchronize()
        return rgba.cpu().numpy().reshape(h, w, 4)


# ------------------------------------------------------------------ A: equals the flattened scene
@pytest.fixture(scope="module")
def scene_a(rt, scenes, ora):
    s = isr.scene_a(scenes, ora)
    bl = Blases(rt, s["tris"], s["attrs"], s["bases"], ("bottom_up", "sah_pairs"), s["materials"], s["textures"])
    sc = Instanced(rt, bl.entries, s["instances"], "bottom_up")
    sc.frame()
    assert rt.instance_status(sc.status) == 0
    s.update(bl=bl, sc=sc, cam_dev=rt.to_device(s["cam"]), imat_dev=_words(rt, s["instance_materials"]),
             records=sc.host_records())
    s["flat"] = {rn: Flat(rt, bl, s["instances"], s["records"], s["instance_materials"], rn) for rn in (False, True)}
    assert s["flat"][True].n == 6 * 288 + 200
    return s


def _check_a(rt, s, w, h, spp, tiled, modes):
    bl, sc, light = s["bl"], s["sc"], s["light"]
    rec = _chain(rt, sc, s["cam_dev"], light, w, h, spp=spp, tiled=tiled)
    hits, ids, sids = _host(rec["hits"], rt.HIT), _host(rec["ids"], np.uint32), _host(rec["sids"], np.uint32)
    # the frame sees every instance, has misses, and has shadowed and lit hits
    live = ids < sc.n
    seen = np.bincount(ids[live], minlength=sc.n)
    assert (seen >= 20 * spp).all(), f"samples per instance {seen.tolist()}"
    assert ((ids == rt.MISS) == (hits["primitive_id"] == rt.MISS)).all() and (~live).sum() > 1000
    assert (sids[~live] == rt.MISS).all(), "a miss has no shadow ray"
    shadowed = sids[live] < sc.n
    assert shadowed.sum() > 100 * spp and (~shadowed).sum() > 100 * spp, "shadowed and lit hits"
    what = f"{w}x{h} spp {spp} {'tiled' if tiled else 'row-major'}"
    for rn in (False, True):
        flat = s["flat"][rn]
        fh, fs = flat.records(hits, ids, sids)
        for mode in modes:
            got = _shade(rt, bl, sc, rec, w, h, mode, light, spp=spp, tiled=tiled, renormalize=rn, instance_materials=s["imat_dev"])
            exp = flat.shade(rec["rays"], fh, fs, w, h, mode, light, spp=spp, tiled=tiled)
            _assert_same(got, exp, f"{what} mode {mode} renormalize {rn}")
            # (not a flat frame: grey levels, the 8 hues, the LOD steps, shaded colours)
            assert len(np.unique(got.reshape(-1, 4), axis=0)) > {3: 4, 4: 1}.get(mode, 20), f"{what} mode {mode}: a flat frame"
    return rec


@pytest.mark.parametrize("tiled", [False, True], ids=["row-major", "tiled"])
@pytest.mark.parametrize("spp", [1, 4])
def test_frame_equals_the_flattened_scene(scene_a, rt, spp, tiled):
    for (w, h) in SIZES:
        _check_a(rt, scene_a, w, h, spp, tiled, MODES)


@pytest.mark.parametrize("tiled", [False, True], ids=["row-major", "tiled"])
def test_frame_equals_the_flattened_scene_spp16(scene_a, rt, tiled):
    _check_a(rt, scene_a, 130, 101, 16, tiled, (0, 4, 8))


def test_renormalisation_and_override_show_in_the_frame(scene_a, rt):
    """the switches under test change the frame: otherwise A would compare two frames that ignore them"""
    s, (w, h) = scene_a, SIZES[0]
    rec = _chain(rt, s["sc"], s["cam_dev"], s["light"], w, h)
    on = _shade(rt, s["bl"], s["sc"], rec, w, h, 5, s["light"], renormalize=True, instance_materials=s["imat_dev"])
    off = _shade(rt, s["bl"], s["sc"], rec, w, h, 5, s["light"], renormalize=False, instance_materials=s["imat_dev"])
    ids = _host(rec["ids"], np.uint32).reshape(h, w)
    changed = (on != off).any(axis=-1)
    assert changed[ids == 1].mean() > 0.2, "the scaled instance is lit differently once its normals are unit again"
    assert changed[ids == 4].mean() < 0.05, "a translated instance's normals keep their length (to an ulp)"
    plain = _shade(rt, s["bl"], s["sc"], rec, w, h, 3, s["light"])
    over = _shade(rt, s["bl"], s["sc"], rec, w, h, 3, s["light"], instance_materials=s["imat_dev"])
    diff = (plain != over).any(axis=-1)
    assert diff[ids == 4].mean() > 0.5 and not diff[ids != 4].any()
    assert len(np.unique(over[ids == 4], axis=0)) == 1 and len(np.unique(plain[ids == 4], axis=0)) >= 2


# ------------------------------------------------------------------ B: identity instance == rt_trace
@pytest.fixture(scope="module")
def smooth12(rt, scenes, ora):
    sc = texture_scene.make_smooth(scenes, ora, G=12)
    sc["cam"] = scenes.make_camera((1.0, 7.0, 1.0), -0.785, 0.7, 120.0)
    sc["kw"] = dict(attributes=sc["attributes"], materials=sc["materials"], light=sc["light"], textures=sc["textures"])
    sc["n"] = sc["tris"].shape[0]
    return sc


@pytest.mark.parametrize("tree", ["bottom_up", "sah"])
def test_identity_instance_equals_rt_trace(smooth12, rt, tree):
    import torch
    bl = Blases(rt, [smooth12["tris"]], [smooth12["attributes"]], [0], (tree,), smooth12["materials"], smooth12["textures"])
    world = dict(smooth12, gpu={tree: bl.trees[0]})          # what test_gpu_shade_frame._trace reads
    g, root, count = bl.trees[0]
    inp = g["inp"]
    sc = Instanced(rt, bl.entries, ir.instance_array([np.eye(3, 4)], [0]), "bottom_up")
    sc.frame()
    assert rt.instance_status(sc.status) == 0
    cam = rt.to_device(world["cam"])
    for (w, h) in SIZES:
        for spp in (1, 4):
            exp = {mode: _trace(world, tree, mode, w, h, spp) for mode in MODES}
            for tiled in (False, True):
                rec = _chain(rt, sc, cam, world["light"], w, h, spp=spp, tiled=tiled)
                # the instanced records are rt_intersect_rays's on the BLAS (test_gpu_instances item 3)
                plain = torch.zeros_like(rec["hits"])
                rt.IntersectRays(inp.triangles_out, inp.nodes_out, root, count, rec["rays"], plain)
                hits = _host(rec["hits"], rt.HIT)
                assert hits.tobytes() == _host(plain, rt.HIT).tobytes()
                n_hit = int((hits["primitive_id"] < world["n"]).sum())
                assert 1000 * spp < n_hit < hits.size, "the frame has hits and misses"
                for mode in MODES:
                    got = _shade(rt, bl, sc, rec, w, h, mode, world["light"], spp=spp, tiled=tiled, renormalize=False)
                    _assert_same(got, exp[mode], f"{tree} {w}x{h} spp {spp} {'tiled' if tiled else 'row-major'} mode {mode}")


# ------------------------------------------------------------------ C: float64
def test_against_float64(rt, scenes, ora):
    s = isr.scene_c(scenes, ora)
    w, h = 160, 100
    bl = Blases(rt, s["tris"], s["attrs"], s["bases"], ("bottom_up", "sah_pairs"), s["materials"], s["textures"])
    sc = Instanced(rt, bl.entries, s["instances"], "sah")
    sc.frame()
    assert rt.instance_status(sc.status) == 0
    tris, at = isr.flatten_f64(s["tris"], s["attrs"], s["bases"], s["instances"], None)
    f64 = shade_ref.Reference(tris, at, s["materials"], s["textures"], s["light"], s["cam"], w, h)
    assert int(f64.hit.sum()) >= 10_000
    cam = rt.to_device(s["cam"])
    for tiled in (False, True):
        rec = _chain(rt, sc, cam, s["light"], w, h, tiled=tiled)
        for mode in (3, 4, 5, 6, 7, 8):
            got = _shade(rt, bl, sc, rec, w, h, mode, s["light"], tiled=tiled, renormalize=True)
            r = shade_ref.compare(got, f64, mode)
            print(f"{'tiled' if tiled else 'row-major'} mode {mode}: masked {100 * r['masked_fraction']:.2f} %, "
                  f"max |diff| {r['max_diff']}, {r['n_bad']} bad of {r['stable_hit']} stable hits")
            assert r["n_bad"] == 0, f"mode {mode}: {r['n_bad']} stable pixels out of tolerance (max {r['max_diff']})"
            assert r["masked_fraction"] <= shade_ref.MASK_BOUND[mode]


# ------------------------------------------------------------------ D: edges
@pytest.mark.parametrize("tiled", [False, True], ids=["row-major", "tiled"])
def test_records_that_shade_as_miss_and_guard_bytes(scene_a, rt, tiled):
    import torch
    s, bl, sc = scene_a, scene_a["bl"], scene_a["sc"]
    w, h, spp, light = 130, 101, 4, s["light"]
    rec = _chain(rt, sc, s["cam_dev"], light, w, h, spp=spp, tiled=tiled)
    hits, ids, sids = _host(rec["hits"], rt.HIT), _host(rec["ids"], np.uint32), _host(rec["sids"], np.uint32)
    rng = np.random.default_rng(5)
    # records: instance 2 flagged singular, instance 3 names a BLAS outside the table, instance 5 a null table entry
    records = s["records"].copy()
    records["flags"][2] = rt.RT_INSTANCE_SINGULAR
    records["blas"][3] = 9
    records["blas"][5] = 2
    geometry = rt.shade_geometry_table(bl.table_entries + [None])
    # hits: every eighth hit of instance 0 gets an instance id >= num_instances, every eighth of instance 1 a primitive id
    # >= its BLAS's count; the untouched misses get junk in their other fields
    i0, i1 = np.nonzero(ids == 0)[0][::8], np.nonzero(ids == 1)[0][::8]
    assert i0.size > 10 and i1.size > 10 and all((ids == k).sum() > 50 for k in (2, 3, 5))
    ids[i0] = np.where(np.arange(i0.size) % 2 == 0, sc.n, rng.integers(sc.n, 1 << 32, i0.size)).astype(np.uint32)
    hits["primitive_id"][i1] = np.where(np.arange(i1.size) % 2 == 0, 288, rng.integers(288, 1 << 32, i1.size)).astype(np.uint32)
    miss = np.nonzero(ids == rt.MISS)[0]
    junk = rng.choice(np.float32([np.nan, -1.0, 0.0, 1e30, 5.0, -np.inf]), (miss.size, 3))
    hits["t"][miss], hits["u"][miss], hits["v"][miss] = junk[:, 0], junk[:, 1], junk[:, 2]
    hits["primitive_id"][miss[::3]] = 7                           # a miss is decided by the instance id alone
    sids[miss[::5]] = sc.n + 3                                    # shadow ids are only compared with num_instances
    d_hits, d_ids = rt.to_device(hits), _words(rt, ids)
    rec2 = dict(rec, sids=_words(rt, sids))
    d_records = rt.to_device(records)
    flat = Flat(rt, bl, s["instances"], records, s["instance_materials"], True, tris=bl.tris + [None], attrs=bl.attrs + [None])
    assert flat.n == 3 * 288 + 200
    fh, fs = flat.records(hits, ids, sids)
    flat_ids = _host(fh, rt.HIT)["primitive_id"]
    assert (flat_ids[np.concatenate([i0, i1])] == rt.MISS).all() and (flat_ids != rt.MISS).sum() > 1000
    guard = 64
    for mode in MODES:
        buf = torch.full((w * h * 4 + guard,), 0xA5, dtype=torch.uint8, device="cuda")
        _shade(rt, bl, sc, rec2, w, h, mode, light, spp=spp, tiled=tiled, instance_materials=s["imat_dev"], rgba=buf,
               geometry=geometry, num_blas=3, records=d_records, hits=d_hits, ids=d_ids)
        torch.cuda.synchronize()
        out = buf.cpu().numpy()
        assert (out[w * h * 4:] == 0xA5).all(), f"mode {mode}: bytes after rgba8 were written"
        exp = flat.shade(rec["rays"], fh, fs, w, h, mode, light, spp=spp, tiled=tiled)
        _assert_same(out[:w * h * 4].reshape(h, w, 4), exp, f"mode {mode}: records that shade as miss")


@pytest.mark.parametrize("dims", [(9, 7), (1, 1)])
def test_edge_tiles(scene_a, rt, dims):
    """tiled frames smaller than their tiles: the records of off-frame lanes hold garbage that names no valid instance, the
    frame is the row-major one and nothing is written behind it"""
    import torch
    s, bl, sc, (w, h), light = scene_a, scene_a["bl"], scene_a["sc"], dims, scene_a["light"]
    cam = s["cam_dev"]
    for spp in (1, 4):
        row = _chain(rt, sc, cam, light, w, h, spp=spp)
        til = _chain(rt, sc, cam, light, w, h, spp=spp, tiled=True)
        tiles_x = (w + 7) // 8
        lane = np.arange(64)
        lx = (lane & 1) | ((lane >> 1) & 2) | ((lane >> 2) & 4)
        ly = ((lane >> 1) & 1) | ((lane >> 2) & 2) | ((lane >> 3) & 4)
        n = rt.CameraRayCount(w, h, spp, True)
        j = np.arange(n)
        tile = j // (64 * spp)
        off = ((tile % tiles_x) * 8 + lx[j % 64] >= w) | ((tile // tiles_x) * 8 + ly[j % 64] >= h)
        assert off.sum() == n - w * h * spp
        ids, hits = _host(til["ids"], np.uint32), _host(til["hits"], np.float32).reshape(-1, 4)
        rays = _host(til["rays"], np.float32).reshape(-1, 8)
        ids[off], hits[off], rays[off] = 0x7FFFFFF0, np.nan, np.nan
        sids = _host(til["sids"], np.uint32)
        sids[off] = 0x7FFFFFF0
        dirty = dict(rays=rt.to_device(rays).view(torch.float32).view(-1, 8), hits=rt.to_device(hits).view(torch.float32).view(-1, 4),
                     ids=_words(rt, ids), sids=_words(rt, sids))
        for mode in MODES:
            exp = _shade(rt, bl, sc, row, w, h, mode, light, spp=spp, instance_materials=s["imat_dev"])
            buf = torch.full((w * h * 4 + 64,), 0xA5, dtype=torch.uint8, device="cuda")
            _shade(rt, bl, sc, dirty, w, h, mode, light, spp=spp, tiled=True, instance_materials=s["imat_dev"], rgba=buf)
            torch.cuda.synchronize()
            out = buf.cpu().numpy()
            assert (out[w * h * 4:] == 0xA5).all(), f"{w}x{h} mode {mode}: pixels beyond w*h were written"
            _assert_same(out[:w * h * 4].reshape(h, w, 4), exp, f"{w}x{h} spp {spp} mode {mode}: tiled against row-major")


def test_one_instance_of_one_triangle(rt, scenes, ora):
    tri = np.float32([[0, 0, 0, 4, 0.5, 0, 0, 0.25, 4]])
    at = scenes.smooth_uv_attributes(tri, np.array([1], np.int32), seed=3)
    mats, chains = texture_scene.materials_and_chains(scenes, ora, 4)
    bl = Blases(rt, [tri], [at], [1], ("bottom_up",), mats, chains)
    inst = ir.instance_array([isr._affine(ir.rotation(0.2, 0.4, -0.3) @ np.diag([1.5, 1.0, 0.8]), (0.5, 0.0, 0.3))], [0])
    sc = Instanced(rt, bl.entries, inst, "bottom_up")
    sc.frame()
    assert rt.instance_status(sc.status) == 0
    cam = rt.to_device(scenes.make_camera((2.5, 4.0, 2.0), 0.0, 1.5, 50.0))
    light, (w, h) = (1.0, 8.0, -2.0), (40, 30)
    flat = Flat(rt, bl, inst, sc.host_records(), None, True)
    assert flat.n == 1 and flat.at["material_id"].tolist() == [2]
    for tiled in (False, True):
        rec = _chain(rt, sc, cam, light, w, h, tiled=tiled)
        hits, ids, sids = _host(rec["hits"], rt.HIT), _host(rec["ids"], np.uint32), _host(rec["sids"], np.uint32)
        assert 30 < (ids == 0).sum() < w * h and (hits["primitive_id"][ids == 0] == 0).all()
        fh, fs = flat.records(hits, ids, sids)
        for mode in MODES:
            _assert_same(_shade(rt, bl, sc, rec, w, h, mode, light, tiled=tiled),
                         flat.shade(rec["rays"], fh, fs, w, h, mode, light, tiled=tiled), f"one triangle, mode {mode}")


def test_no_instances_is_an_all_miss_frame(scene_a, rt):
    import torch
    s, (w, h) = scene_a, (33, 17)
    for tiled in (False, True):
        rec = _chain(rt, s["sc"], s["cam_dev"], s["light"], w, h, tiled=tiled)     # records full of hits: none of them counts
        for mode in MODES:
            buf = torch.full((w * h * 4 + 64,), 0xA5, dtype=torch.uint8, device="cuda")
            rt.ShadeFrameInstanced(None, 0, None, None, 0, rec["rays"], rec["hits"], rec["ids"], buf, (w, h), render_type=mode,
                                   tiled=tiled, shadow_instance_ids=rec["sids"] if mode == 8 else None, light=s["light"],
                                   **s["bl"].kw)
            torch.cuda.synchronize()
            out = buf.cpu().numpy()
            assert (out[w * h * 4:] == 0xA5).all()
            assert (out[:w * h * 4].reshape(-1, 4) == np.uint8(MISS_RGBA[mode])).all(), f"mode {mode}"


def test_material_ids_per_pixel_on_the_soup(rt, scenes, ora):
    """mode 3 on the 251-material soup: the hue names the resolved material id, so material_base (two table entries over one
    tree, bases 0 and 100: ids up to 350 leave the table) and the override show per pixel"""
    s = texture_scene.make_soup251(scenes, ora)
    tris, at = s["tris"], s["attributes"]
    bl = Blases(rt, [tris], [at], [0], ("sah",), s["materials"], None)
    bl.entries = bl.entries * 2
    bl.tris, bl.attrs, bl.bases = [tris, tris], [at, at], [0, 100]
    e = bl.table_entries[0]
    bl.geometry = rt.shade_geometry_table([e, (e[0], e[1], e[2], 100)])
    mats = [isr._affine(np.eye(3) * 0.5, (0, 0, 0)), isr._affine(np.eye(3) * 0.5, (0.5, 0, 0.5)),
            isr._affine(ir.rotation(0, 0.5, 0) * 0.5, (0.1, 0.5, 0.1)), isr._affine(np.eye(3) * 0.5, (0.5, 0.5, 0))]
    inst = ir.instance_array(mats, [0, 1, 1, 0])
    imat = np.array([-1, -1, -7, 200], np.int32)
    sc = Instanced(rt, bl.entries, inst, "bottom_up")
    sc.frame()
    assert rt.instance_status(sc.status) == 0
    w, h, light = 160, 100, s["light"]
    rec = _chain(rt, sc, rt.to_device(s["cameras"]["box"]), light, w, h, shadows=False)
    hits, ids = _host(rec["hits"], rt.HIT), _host(rec["ids"], np.uint32)
    assert all((ids == k).sum() > 100 for k in range(4))
    flat = Flat(rt, bl, inst, sc.host_records(), imat, True)
    fh, fs = flat.records(hits, ids, np.full(ids.size, rt.MISS, np.uint32))
    got = _shade(rt, bl, sc, rec, w, h, 3, light, instance_materials=_words(rt, imat))
    _assert_same(got, flat.shade(rec["rays"], fh, fs, w, h, 3, light), "soup, mode 3")
    # the hue of every hit pixel is the one of its resolved id (float64 hue, one truncation: shade_ref.TOLERANCE[3])
    live = ids < 4
    resolved = flat.at["material_id"][_host(fh, rt.HIT)["primitive_id"][live]].astype(np.int64)
    base_id = at["material_id"][hits["primitive_id"][live]].astype(np.int64)
    k = ids[live]
    assert (resolved == np.where(k == 0, base_id, np.where(k == 3, 200, base_id + 100))).all()
    assert resolved.max() > 251 and len(set(resolved[k == 1].tolist())) > 30
    exp = shade_ref._hsv_rgb255(np.clip(resolved / 251.0, 0.0, 1.0))
    diff = np.abs(got.reshape(-1, 4)[live][:, :3].astype(np.int64) - np.floor(exp).astype(np.int64))
    assert diff.max() <= shade_ref.TOLERANCE[3]


# ------------------------------------------------------------------ E: the whole frame in a HIP graph
def test_prepare_build_and_chain_in_a_hip_graph(scene_a, rt, scenes, ora):
    import torch
    s, bl = scene_a, scene_a["bl"]
    w, h, spp, mode, light = 160, 100, 4, 8, scene_a["light"]
    moved = isr.scene_a(scenes, ora, moved=True)["instances"]
    sc = Instanced(rt, bl.entries, s["instances"], "bottom_up")
    frame = torch.zeros(w * h * 4, dtype=torch.uint8, device="cuda")
    bufs = {}

    def one_frame():   # prepare, TLAS build, five calls: one stream, no branches
        sc.frame()
        bufs.update(_chain(rt, sc, s["cam_dev"], light, w, h, spp=spp, tiled=True, bufs=bufs or None))
        _shade(rt, bl, sc, bufs, w, h, mode, light, spp=spp, tiled=True, instance_materials=s["imat_dev"], rgba=frame)

    expected = {}
    for key, instances in (("a", s["instances"]), ("b", moved)):
        sc.instances.copy_(rt.to_device(instances))
        one_frame()
        flat = Flat(rt, bl, instances, sc.host_records(), s["instance_materials"], True)
        fh, fs = flat.records(_host(bufs["hits"], rt.HIT), _host(bufs["ids"], np.uint32), _host(bufs["sids"], np.uint32))
        expected[key] = flat.shade(bufs["rays"], fh, fs, w, h, mode, light, spp=spp, tiled=True)
        _assert_same(frame.cpu().numpy().reshape(h, w, 4), expected[key], f"eager frame {key}")
    assert (expected["a"] != expected["b"]).any(), "the moved scene must give another frame"

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        one_frame()
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            one_frame()
    torch.cuda.current_stream().wait_stream(side)
    for key in ("a", "b", "a"):
        sc.instances.copy_(rt.to_device(s["instances"] if key == "a" else moved))   # rewritten in place: same buffer
        for t in list(bufs.values()) + [frame]:
            t.zero_()
        sc.records.fill_(0xFF)
        graph.replay()
        torch.cuda.synchronize()
        _assert_same(frame.cpu().numpy().reshape(h, w, 4), expected[key], f"graph replay {key}")
