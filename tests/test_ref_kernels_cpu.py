"""The oracle against the reference's own kernels, run on the CPU (oracle/_ref/libref_kernels.so: BottomUpBuilder.cu and
Tracer.cu compiled from the reference tree, launches emulated by oracle/ref_kernels_driver.cpp).  Morton codes, the
radix tree, leaf records and boxes of the LBVH (plain and pairs), and frames and test counters of TraceRays on every
tree type: all exact.  The last tests show that each comparison catches a one-bit Morton flip, two swapped equal-key
values, a reversed traversal tie-break and a box one ulp off."""
import numpy as np
import pytest

import edge_scenes
import ref_compare as rc
import texture_scene
from oracle import oracle_py

pytestmark = pytest.mark.skipif(not oracle_py.ref_kernels_available(),
                                reason="oracle/_ref/libref_kernels.so not built (the reference tree is not on this machine)")

STACK_LIMIT = 63     # TraceRay's stack has 64 entries and the reference writes past it when full: undefined on a host


def box_of(ora, tris):
    b = ora.scene_aabb(tris)
    return ora.ordered_to_float(b[:3]), ora.ordered_to_float(b[3:])


def point_tris(points):
    """degenerate triangles (three equal corners) at the given points"""
    p = np.asarray(points, np.float32).reshape(-1, 1, 3)
    return np.repeat(p, 3, axis=1).reshape(-1, 9)


def morton_edge_scene():
    """A unit scene box (two corner points) and centroids exactly on its faces and around x * 1024 = 1023 and 1024,
    where Morton3D's clamp to 1023 and the (unsigned) truncation meet."""
    f32 = np.float32
    vals = [f32(0.0), f32(-0.0), f32(1.0), np.nextafter(f32(1.0), f32(0)), f32(1023 / 1024),
            np.nextafter(f32(1023 / 1024), f32(0)), np.nextafter(f32(1023 / 1024), f32(2)), f32(1022.5 / 1024),
            f32(0.5), np.nextafter(f32(0.5), f32(0)), f32(1 / 1024), np.nextafter(f32(1 / 1024), f32(0))]
    pts = [(0, 0, 0), (1, 1, 1)]
    for i, a in enumerate(vals):
        for j, b in enumerate(vals):
            pts.append((a, b, vals[(i + j) % len(vals)]))
    return point_tris(pts)


def morton_scenes(scenes):
    flat_z = scenes.grid_mesh(12, 4).reshape(-1, 3, 3).copy()
    flat_z[:, :, 2] = np.float32(-3.0)
    return {"grid17": scenes.grid_mesh(17, 3), "soup5000": scenes.soup(5000, 1), "flat8": scenes.flat_mesh(8, 1),
            "grid24": scenes.grid_mesh(24, 1), "soup2048": scenes.soup(2048, 7), "flat12": scenes.flat_mesh(12, 3),
            "soup700dup": scenes.soup(700, 3, dup_fraction=0.6), "soup64": scenes.soup(64, 9, dup_fraction=0.0),
            "grid9": scenes.grid_mesh(9, 1), "edges": morton_edge_scene(), "flat_z": flat_z.reshape(-1, 9),
            "one": scenes.soup(1, 5), "signed_zero": edge_scenes.signed_zero_mesh(scenes)}


def test_morton_codes_match_the_reference_kernel(ora, scenes):
    for name, tris in morton_scenes(scenes).items():
        aabb = ora.scene_aabb(tris)
        codes, vals = ora.morton_codes(tris, aabb)
        rcodes, rvals = ora.ref_morton(tris, aabb)
        rc.assert_codes_equal(codes, rcodes, name)
        rc.assert_codes_equal(vals, rvals, name + " values")
    # the edge scene does reach the clamp and both sides of the 1023 cell boundary on every axis
    c, _ = ora.ref_morton(morton_edge_scene(), ora.scene_aabb(morton_edge_scene()))
    x = np.zeros_like(c)
    for b in range(10):
        x |= ((c >> np.uint32(3 * b + 2)) & np.uint32(1)) << np.uint32(b)
    assert {0, 1022, 1023} <= set(x.tolist())


def hierarchy_sizes():
    out = [2, 3, 4]
    for k in (9, 12, 16):
        out += [2 ** k - 1, 2 ** k, 2 ** k + 1]
    return out


@pytest.mark.parametrize("n", hierarchy_sizes())
def test_lbvh_matches_the_reference_kernels(n, ora, scenes):
    """Morton -> stable sort -> GenerateHierarchy -> GenerateTriangles -> GenerateAABBs of the reference against
    ora_build: every Node word, every defined TrianglePair byte, sorted codes and indices."""
    tris = scenes.soup(n, 11 + n % 7, dup_fraction=0.3)
    o = ora.build_bvh(tris)
    r = ora.ref_build_lbvh(tris)
    rc.assert_build_equal(o, r, f"soup{n}")
    # the radix tree alone, on the oracle's sorted codes
    nodes, _ = ora.ref_hierarchy(o["codes"])
    assert (nodes["w28"] == o["nodes"]["w28"]).all()
    assert ((nodes["w12"] & rc.PARENT) == (o["nodes"]["w12"] & rc.PARENT)).all()


def test_lbvh_duplicate_codes_and_big_soup_match_the_reference_kernels(ora, scenes):
    """Runs of equal Morton codes (cpl's 32 + __clz(i ^ j) branch), a flat scene and a 200k-triangle soup."""
    dup = np.repeat(scenes.soup(40, 3, dup_fraction=0.0), 37, axis=0)                 # 37 copies of each triangle
    cases = {"copies": dup, "one_point": point_tris(np.zeros((300, 3))), "flat12": scenes.flat_mesh(12, 3),
             "soup700dup": scenes.soup(700, 3, dup_fraction=0.6), "soup200k": scenes.soup(200_000, 5),
             "signed_zero": edge_scenes.signed_zero_mesh(scenes)}
    for name, tris in cases.items():
        o = ora.build_bvh(tris)
        if name in ("copies", "one_point"):
            assert np.unique(o["codes"]).size <= 40 and np.unique(o["codes"]).size < o["n"] // 30
        rc.assert_build_equal(o, ora.ref_build_lbvh(tris), name)


def test_single_triangle_is_the_documented_difference(ora, scenes):
    """n = 1 (Q8): GenerateHierarchy has no thread, so the reference leaves slot 0 without a child or type (a frame of
    nothing); the oracle defines slot 0 as the leaf.  Everything else agrees."""
    tris = scenes.soup(1, 5)
    o, r = ora.build_bvh(tris), ora.ref_build_lbvh(tris)
    rc.assert_codes_equal(o["codes"], r["codes"])
    rc.assert_leaves_equal(o["leaves"], r["leaves"], r["indices"])
    assert int(r["nodes"]["w28"][0]) == 0 and int(o["nodes"]["w28"][0]) == 2 << 29
    assert (o["nodes"]["min"][0] == r["nodes"]["min"][0]).all() and (o["nodes"]["max"][0] == r["nodes"]["max"][0]).all()
    assert (o["nodes"]["w12"] == r["nodes"]["w12"]).all()


@pytest.mark.parametrize("scene", ["grid16", "grid24_rolled", "soup500", "grid4_31", "signed_zero", "soup3000"])
def test_pairs_match_the_reference_kernels(scene, ora, scenes):
    tris = {"grid16": scenes.grid_mesh(16, 2), "grid24_rolled": texture_scene.roll_corners(scenes.grid_mesh(24, 3)),
            "soup500": scenes.soup(500, 1, dup_fraction=0.0), "grid4_31": scenes.grid_mesh(4, 1)[:31],
            "signed_zero": edge_scenes.signed_zero_mesh(scenes), "soup3000": scenes.soup(3000, 4)}[scene]
    o = ora.build_pairs(tris)
    r = ora.ref_build_lbvh(tris, pairs=True)
    assert r["L"] == o["L"]
    rc.assert_pair_leaves_multiset_equal(o, r, scene)
    # threads run in gid order here, which is the oracle's slot rule (prefix sum in input order): whole tree exact
    rc.assert_build_equal(o, r, scene)


# ---------------------------------------------------------------- traversal
def all_trees(ora, tris):
    b = ora.build_bvh(tris)
    yield "lbvh", b["leaves"], b["nodes"], 0, 2
    p = ora.build_pairs(tris)
    yield "pairs", p["leaves"], p["nodes"], 0, 2
    h = ora.build_hybrid(tris)
    yield "hybrid", h["leaves"], h["nodes"], h["root"], 2
    for name, pr, sp in (("sah", False, False), ("sah+pairs", True, False), ("sah+splits", False, True)):
        s = ora.build_sah(tris, pairs=pr, splits=sp)
        yield name, s["leaves"], s["nodes"], 0, 1


def compare_traces(ora, tris, cam, w, h, modes, what, **kw):
    for tree, leaves, nodes, root, count in all_trees(ora, tris):
        for m in modes:
            img, c = ora.trace(leaves, nodes, root, count, cam, w, h, render_type=m, **kw)
            assert int(c[2]) < STACK_LIMIT and int(c[3]) == 0, (what, tree, c)
            rimg, rcnt = ora.ref_trace(leaves, nodes, root, count, cam, w, h, render_type=m, **kw)
            rc.assert_frames_equal(img, c, rimg, rcnt, f"{what} {tree} mode {m}")
            if m == 0:
                assert int(c[0]) > 0 and int(c[1]) > 0, (what, tree, c)


def lit_scene(ora, scenes, tris, k=3):
    lo, hi = box_of(ora, tris)
    at = scenes.flat_attributes(tris, np.arange(tris.shape[0], dtype=np.int32) % k)
    return scenes.camera_for_box(lo, hi), dict(attributes=at, materials=scenes.default_materials(k),
                                               light=tuple(float(x) for x in hi + (hi - lo) * 0.5))


@pytest.mark.parametrize("scene,w,h", [("grid24", 97, 53), ("soup2048", 64, 48), ("flat12", 33, 31), ("grid30", 128, 72)])
def test_trace_matches_the_reference_kernel(scene, w, h, ora, scenes):
    """TraceRays of the reference on the oracle's six trees: kDepth, kBoxtests, kTriangleTests, kMaterialID, kLODs
    (untextured: magenta) and kDiffuse; frames byte for byte, sum of box tests and of triangle tests exact."""
    tris = {"grid24": scenes.grid_mesh(24, 1), "soup2048": scenes.soup(2048, 7), "flat12": scenes.flat_mesh(12, 3),
            "grid30": scenes.grid_mesh(30, 2)}[scene]
    cam, kw = lit_scene(ora, scenes, tris)
    compare_traces(ora, tris, cam, w, h, range(6), scene, **kw)


def test_trace_edge_scenes_match_the_reference_kernel(ora, scenes):
    """Signed zeros and degenerate triangles; axis-parallel rays from a camera on box planes (0 * inf = NaN in the slab
    test); the deepest fractal scene whose stack stays below 64 entries."""
    tris = edge_scenes.signed_zero_mesh(scenes)
    cam = scenes.make_camera((0.0, 6.0, 0.0), 0.3, 1.2, 60.0)
    compare_traces(ora, tris, cam, 96, 64, (0, 1, 2, 3, 5), "signed_zero", **lit_scene(ora, scenes, tris)[1])

    G = 16
    tris = scenes.grid_mesh(G, 2)
    ys = np.sort(tris.reshape(-1, 3)[:, 1])
    cam = edge_scenes.axis_camera(scenes, (G // 2, float(ys[ys.size // 2]), -3.0), 64.0)
    compare_traces(ora, tris, cam, 65, 49, (0, 1, 2, 5), "axis_parallel", **lit_scene(ora, scenes, tris)[1])

    tris = scenes.fractal_corner(4000, 3)
    cam = scenes.diagonal_camera(2.0 ** -10, 2.0 ** 45)
    b, s = ora.build_bvh(tris), ora.build_sah(tris)
    deepest = 0
    for leaves, nodes, root, count in ((b["leaves"], b["nodes"], 0, 2), (s["leaves"], s["nodes"], 0, 1)):
        for m in (0, 1):
            img, c = ora.trace(leaves, nodes, root, count, cam, 33, 25, render_type=m)
            assert int(c[2]) < STACK_LIMIT and int(c[3]) == 0, c
            deepest = max(deepest, int(c[2]))
            rimg, rcnt = ora.ref_trace(leaves, nodes, root, count, cam, 33, 25, render_type=m)
            rc.assert_frames_equal(img, c, rimg, rcnt, f"fractal mode {m}")
    assert deepest >= 40


@pytest.mark.parametrize("which", ["make", "smooth"])
def test_textured_modes_match_the_reference_kernel(which, ora, scenes):
    """kLODs, kDiffuse, kTexture, kTextureLit, kTextureLitShadows on the texture scenes, all six trees.
    Here the reference's shaders call libm (log2f, powf(2, lod), the double pow of the specular term) and the oracle
    calls csrc/rt_math.h; test_rt_math_against_libm holds rt_math.h to libm's correctly rounded results, so the frames are
    required to match exactly, and they do.  Were a last bit ever to differ, it could only show on textured pixels or on
    pixels with a specular term: the pixels of the untextured material (material 3: no texture, no bump map), with its
    specular colour set to zero, are checked on their own below, so such a difference would be told apart."""
    s = (texture_scene.make if which == "make" else texture_scene.make_smooth)(scenes, ora)
    mats = s["materials"]
    assert mats["texture"][3] == -1 and mats["bump"][3] == -1 and mats["disp"][3] == -1
    kw = dict(attributes=s["attributes"], materials=mats, light=s["light"], textures=s["textures"])
    for cname, cam in s["cameras"].items():
        compare_traces(ora, s["tris"], cam, 96, 72, (4, 5, 6, 7, 8), f"{which}/{cname}", **kw)
    # the untextured material's pixels: kMaterialID paints material 3 of 4 with HsvToRgb(0.75, 1, 1) = (127, 0, 255)
    mats = mats.copy()
    mats["specular"][3] = 0
    kw["materials"] = mats
    b = ora.build_bvh(s["tris"])
    cam = s["cameras"]["oblique"]
    ids, _ = ora.trace(b["leaves"], b["nodes"], 0, 2, cam, 96, 72, render_type=3, **kw)
    plain = (ids[..., :3] == np.array([127, 0, 255], np.uint8)).all(-1)
    assert plain.sum() > 300, int(plain.sum())
    for m in (5, 6, 7, 8):
        img, _ = ora.trace(b["leaves"], b["nodes"], 0, 2, cam, 96, 72, render_type=m, **kw)
        rimg, _ = ora.ref_trace(b["leaves"], b["nodes"], 0, 2, cam, 96, 72, render_type=m, **kw)
        assert (img[plain] == rimg[plain]).all(), m


# ---------------------------------------------------------------- teeth: each comparison catches a small corruption
def test_teeth_one_morton_bit(ora, scenes):
    tris = scenes.grid_mesh(17, 3)
    aabb = ora.scene_aabb(tris)
    codes, _ = ora.morton_codes(tris, aabb)
    rcodes, _ = ora.ref_morton(tris, aabb)
    rc.assert_codes_equal(codes, rcodes)
    bad = codes.copy()
    bad[123] ^= np.uint32(1 << 4)
    with pytest.raises(AssertionError):
        rc.assert_codes_equal(bad, rcodes)


def test_teeth_swapped_equal_key_values(ora, scenes):
    tris = np.repeat(scenes.soup(50, 3, dup_fraction=0.0), 4, axis=0)
    o, r = ora.build_bvh(tris), ora.ref_build_lbvh(tris)
    rc.assert_build_equal(o, r)
    k = int(np.nonzero(o["codes"][1:] == o["codes"][:-1])[0][7])
    bad = dict(o)
    bad["indices"] = o["indices"].copy()
    bad["indices"][[k, k + 1]] = bad["indices"][[k + 1, k]]
    with pytest.raises(AssertionError):
        rc.assert_build_equal(bad, r)


def test_teeth_reversed_tie_break(ora, scenes):
    """A height field seen from above: sibling boxes that share their highest vertex are entered through the same top
    plane at the same t, and which one is opened first decides what the other's children are culled against.  The
    oracle traces the same tree with its pairs stored in reverse order, so every tie goes the other way; the
    comparison with the reference on the original tree must fail on the counters."""
    tris = scenes.grid_mesh(32, 1)
    b = ora.build_bvh(tris)
    lo, hi = box_of(ora, tris)
    cam = scenes.make_camera(((lo[0] + hi[0]) / 2, 40.0, (lo[2] + hi[2]) / 2), 0.0, 1.2, 200.0)
    rimg, rcnt = ora.ref_trace(b["leaves"], b["nodes"], 0, 2, cam, 64, 64)
    img, c = ora.trace(b["leaves"], b["nodes"], 0, 2, cam, 64, 64)
    rc.assert_frames_equal(img, c, rimg, rcnt)
    rev, root = rc.reverse_pair_order(b["nodes"], 0, 2)
    img2, c2 = ora.trace(b["leaves"], rev, root, 2, cam, 64, 64)
    assert (img2[..., 0] > 0).mean() > 0.15
    with pytest.raises(AssertionError):
        rc.assert_frames_equal(img2, c2, rimg, rcnt)
    # and the reference itself on the reversed tree agrees with the oracle there: the tie-break, not the tree, differs
    rimg2, rcnt2 = ora.ref_trace(b["leaves"], rev, root, 2, cam, 64, 64)
    rc.assert_frames_equal(img2, c2, rimg2, rcnt2)


def test_teeth_box_one_ulp(ora, scenes):
    tris = scenes.soup(3000, 5)
    o, r = ora.build_bvh(tris), ora.ref_build_lbvh(tris)
    rc.assert_build_equal(o, r)
    for f, slot, axis in (("max", 1234, 1), ("min", 17, 0)):
        bad = dict(o)
        bad["nodes"] = o["nodes"].copy()
        v = bad["nodes"][f][slot, axis]
        bad["nodes"][f][slot, axis] = np.nextafter(v, np.float32(np.inf) if f == "max" else np.float32(-np.inf))
        with pytest.raises(AssertionError):
            rc.assert_build_equal(bad, r)
