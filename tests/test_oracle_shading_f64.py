"""The oracle's surface render types (modes 3-8: kMaterialID, kLODs, kDiffuse, kTexture, kTextureLit,
kTextureLitShadows) against an independent float64 evaluation of Tracer.cu's shaders (tests/shade_ref.py), on every
tree the oracle builds.

GPU == oracle is byte-exact elsewhere in the suite, but the oracle restates the reference's shaders statement by
statement and shares rt_math.h with the kernels: a misreading of Tracer.cu (a rotation taken the wrong way, bu / bv
swapped, a tangent-frame sign, (int)lod one level off) would be reproduced by both and pass every parity test.  The
float64 side takes brute-force closest hits on the ORIGINAL triangles and each triangle's own corner order -- no tree,
no pair layout, no RotateAttributes -- so those readings are checked against the statements themselves.

Compared on the pixels whose outcome float32 cannot legitimately change (shade_ref's stability mask, bounded per case
below), with the channel tolerances of shade_ref.TOLERANCE.  The sensitivity tests feed the oracle attributes that
simulate each defect and require the comparison to fail on a large share of the stable pixels."""
import numpy as np
import pytest

import shade_ref
import texture_scene

W, H = 160, 100
MODES = (3, 4, 5, 6, 7, 8)
TREES = ("bottom_up", "pairs", "hybrid", "sah", "sah_pairs", "sah_splits", "sah_pairs_splits")
SCENES = {"height": (texture_scene.make, "oblique", MODES),
          "smooth": (texture_scene.make_smooth, "oblique", MODES),
          "soup251": (texture_scene.make_soup251, "box", (3, 5))}


def build_tree(ora, tris, tree):
    """(leaves, nodes, root, count) of one oracle build"""
    if tree == "bottom_up":
        o = ora.build_bvh(tris)
        return o["leaves"], o["nodes"], 0, 2
    if tree == "pairs":
        o = ora.build_pairs(tris)
        return o["leaves"], o["nodes"], 0, 2
    if tree == "hybrid":
        o = ora.build_hybrid(tris)
        return o["leaves"], o["nodes"], o["root"], 2
    o = ora.build_sah(tris, pairs="pairs" in tree, splits="splits" in tree)
    return o["leaves"], o["nodes"], 0, 1


_cache = {}


def world(name, scenes, ora):
    if name not in _cache:
        make, cam_name, modes = SCENES[name]
        sc = make(scenes, ora)
        cam = sc["cameras"][cam_name]
        ref = shade_ref.Reference(sc["tris"], sc["attributes"], sc["materials"], sc["textures"], sc["light"], cam, W, H)
        _cache[name] = (sc, cam, ref, modes)
    return _cache[name]


def oracle_frame(ora, sc, cam, tree_bufs, mode, attributes=None):
    leaves, nodes, root, count = tree_bufs
    img, _ = ora.trace(leaves, nodes, root, count, cam, W, H, render_type=mode,
                       attributes=sc["attributes"] if attributes is None else attributes, materials=sc["materials"],
                       light=sc["light"], textures=sc["textures"])
    return img


def check_frame(img, ref, mode, what):
    r = shade_ref.compare(img, ref, mode)
    print(f"{what} mode {mode}: {r['hits']} hits, masked {100 * r['masked_fraction']:.2f} %, "
          f"max |diff| on stable pixels {r['max_diff']}, {r['n_bad']} out of tolerance")
    assert r["masked_fraction"] <= shade_ref.MASK_BOUND[mode], f"{what} mode {mode}: the stability mask grew to {r['masked_fraction']:.4f}"
    assert r["stable_hit"] > 1000, f"{what} mode {mode}: too few stable hit pixels to mean anything"
    if r["n_bad"]:
        ys, xs = np.nonzero(r["bad"])
        exp = ref.frame(mode)[0]
        raise AssertionError(f"{what} mode {mode}: {r['n_bad']} stable pixels out of +-{shade_ref.TOLERANCE[mode]} "
                             f"(max {r['max_diff']}); first at (x={xs[0]}, y={ys[0]}): got {img[ys[0], xs[0]].tolist()} "
                             f"float64 {exp[ys[0], xs[0]].tolist()}")


@pytest.mark.parametrize("tree", TREES)
@pytest.mark.parametrize("scene", list(SCENES))
def test_oracle_surface_modes_match_float64(scene, tree, scenes, ora):
    sc, cam, ref, modes = world(scene, scenes, ora)
    bufs = build_tree(ora, sc["tris"], tree)
    # hit / miss: kDepth > 0 exactly where the brute-force float64 ray hits (stable pixels)
    depth = oracle_frame(ora, sc, cam, bufs, 0)
    _, stable, hit = ref.frame(3)
    assert ((depth[..., 0] > 0) == hit)[stable].all(), f"{scene} {tree}: hit / miss differs from brute force"
    for mode in modes:
        check_frame(oracle_frame(ora, sc, cam, bufs, mode), ref, mode, f"{scene} {tree}")


def test_mode3_tolerance_separates_251_material_hues():
    """The premise of mode 3's +-1 tolerance on the soup251 scene: with 251 materials every two material ids differ by
    more than 2 LSB in some channel of kMaterialID, so a frame within +-1 of the float64 one names the primitive that
    was hit modulo 251 (the comparison itself, on every tree, is test_oracle_surface_modes_match_float64)."""
    hues = shade_ref._u8(shade_ref._hsv_rgb255(np.arange(251) / 251.0))
    d = np.abs(hues[:, None, :] - hues[None, :, :]).max(axis=-1) + np.eye(251, dtype=np.int64) * 99
    assert d.min() >= 3, "two material hues are within twice the +-1 tolerance"


@pytest.mark.parametrize("tree", ["pairs", "sah_pairs", "sah_pairs_splits"])
def test_smooth_scene_pairs_hold_every_rotation(tree, scenes, ora):
    """The pair trees of the smooth scene store every rotation of the first and of the second triangle of a pair
    (RotateAttributes cases 0, 1, 2 on both sides, Tracer.cu:57-82), so the comparisons above reach all of them."""
    sc, _, _, _ = world("smooth", scenes, ora)
    rot = texture_scene.pair_rotations(build_tree(ora, sc["tris"], tree)[0])
    assert rot.shape[0] > 1000
    for side in (0, 1):
        counts = np.bincount(rot[:, side], minlength=3)
        assert counts.shape[0] == 3 and (counts > rot.shape[0] // 5).all(), f"rotations[{side}] counts {counts.tolist()}"


def _rotate_corners(at):
    out = at.copy()
    out["normal"] = np.roll(at["normal"], 1, axis=1)
    out["uv"] = np.roll(at["uv"], 1, axis=1)
    return out


def _swap_uv12(at):
    out = at.copy()
    out["uv"][:, 1], out["uv"][:, 2] = at["uv"][:, 2], at["uv"][:, 1]
    return out


def _negate_odd_normals(at):
    out = at.copy()
    out["normal"][1::2] = -at["normal"][1::2]
    return out


# defect -> (attribute transform, {mode that reads the damaged data: least share of stable hit pixels that must fail}).
# Negating the normals of odd triangles reaches at most half of the pixels, and in modes 7 / 8 only half of those: the
# bump- and normal-mapped materials take their normal from the tangent frame, not from the corner normals (measured
# ~50 % in mode 5, ~22 % in mode 7, ~15 % of the lit pixels in mode 8).
DEFECTS = {"rotated_corners": (_rotate_corners, {5: 0.2, 6: 0.2, 7: 0.2}),
           "swapped_bu_bv": (_swap_uv12, {6: 0.2, 7: 0.2}),
           "negated_frame": (_negate_odd_normals, {5: 0.2, 7: 0.1, 8: 0.1})}


@pytest.mark.parametrize("tree", ["bottom_up", "pairs", "sah_pairs_splits"])
@pytest.mark.parametrize("defect", list(DEFECTS))
def test_comparison_catches_attribute_defects(defect, tree, scenes, ora):
    """The oracle traces attributes that simulate a defect while the float64 side keeps the true ones: the comparison
    must fail on a large share of the stable hit pixels of every mode that reads the damaged data -- otherwise the
    tolerances or the mask would be too loose to see the bug they are there for."""
    sc, cam, ref, _ = world("smooth", scenes, ora)
    transform, least = DEFECTS[defect]
    bufs = build_tree(ora, sc["tris"], tree)
    bad_at = transform(sc["attributes"])
    for mode in least:
        r = shade_ref.compare(oracle_frame(ora, sc, cam, bufs, mode, attributes=bad_at), ref, mode)
        share = r["n_bad_hit"] / r["stable_hit"]
        if mode == 8:      # a shadowed pixel shows no normal (diffuse = specular = 0): count the lit ones
            lit = np.zeros(W * H, bool)
            lit[ref.idx] = ~ref.shadow()["hit"]
            _, stable, _ = ref.frame(8)
            lit = lit.reshape(H, W) & stable
            share = int((r["bad"] & lit).sum()) / max(int(lit.sum()), 1)
        print(f"{defect} {tree} mode {mode}: {100 * share:.1f} % of stable hit pixels fail")
        assert share >= least[mode], f"{defect} {tree} mode {mode}: only {share:.3f} of stable hit pixels fail"


@pytest.mark.parametrize("tree", ["pairs", "sah_pairs_splits"])
@pytest.mark.parametrize("side", [0, 1])
def test_comparison_catches_a_wrong_rotation_case(side, tree, scenes, ora):
    """Pair leaves whose rotation 1 and rotation 2 are exchanged on one side -- what a RotateAttributes that mixed up
    its two non-trivial cases would shade -- must fail on a large share of the stable hit pixels.  One side of a pair is
    half of the triangles and two thirds of those carry rotation 1 or 2, so at most about a third of the pixels can
    change (measured 21-30 %)."""
    sc, cam, ref, _ = world("smooth", scenes, ora)
    leaves, nodes, root, count = build_tree(ora, sc["tris"], tree)
    bad_leaves = leaves.copy()
    r = bad_leaves["rotations"][:, side]
    bad_leaves["rotations"][:, side] = np.where(r == 1, 2, np.where(r == 2, 1, r))
    for mode in (5, 6, 7):
        res = shade_ref.compare(oracle_frame(ora, sc, cam, (bad_leaves, nodes, root, count), mode), ref, mode)
        share = res["n_bad_hit"] / res["stable_hit"]
        print(f"rotations[{side}] 1 <-> 2, {tree} mode {mode}: {100 * share:.1f} % of stable hit pixels fail")
        assert share >= 0.1, f"{tree} mode {mode}: only {share:.3f} of stable hit pixels fail"
