"""The textured test scene shared by the CPU and GPU texture tests: a 40 x 40 height field with planar uv,
4 materials (diffuse texture only / texture + bump / texture + normal map in `disp` / untextured) and 5 textures
(power-of-two, non-power-of-two, 1 x 1, a noise height map and a normal map)."""
import numpy as np


def make(scenes, ora):
    tris = scenes.grid_mesh(40, 9)
    n = tris.shape[0]
    mat_ids = (np.arange(n, dtype=np.int32) // 2 // 5) % 4           # runs of 5 cells share a material
    at = scenes.planar_uv_attributes(tris, mat_ids, uv_scale=0.21)
    mats = scenes.default_materials(4)
    chains = make_textures(scenes, ora)
    mats[0]["texture"] = 0
    mats[1]["texture"], mats[1]["bump"] = 1, 3
    mats[2]["texture"], mats[2]["disp"] = 0, 4
    mats[3]["texture"] = -1
    cams = {"oblique": scenes.make_camera((4.0, 9.0, 4.0), -0.785, 0.7, 120.0),
            "top": scenes.make_camera((20.0, 30.0, 20.0), 0.0, 1.5, 120.0),
            "grazing": scenes.make_camera((-3.0, 4.0, 20.0), -1.5708, 0.25, 120.0)}
    light = (20.0, 3.0, -10.0)    # low over the height field: about a quarter of the hits are shadowed
    return dict(tris=tris, attributes=at, materials=mats, textures=chains, cameras=cams, light=light)


def materials_and_chains(scenes, ora, k):
    """k materials cycling through the four of make() (texture / texture + bump / texture + normal map / untextured)
    and make()'s five mip chains."""
    base = make_textures(scenes, ora)
    mats = scenes.default_materials(k)
    kind = np.arange(k) % 4
    mats["texture"] = np.where(kind == 3, -1, np.where(kind == 1, 1, 0))
    mats["bump"] = np.where(kind == 1, 3, -1)
    mats["disp"] = np.where(kind == 2, 4, -1)
    return mats, base


def make_textures(scenes, ora):
    return [ora.generate_lods(scenes.procedural_texture(64, 64, 1, "checker")),
            ora.generate_lods(scenes.procedural_texture(37, 21, 2, "checker")),
            ora.generate_lods(scenes.procedural_texture(1, 1, 3, "checker")),
            ora.generate_lods(scenes.procedural_texture(32, 16, 4, "noise")),
            ora.generate_lods(scenes.procedural_texture(16, 16, 5, "normal"))]


def roll_corners(tris):
    """The grid's triangles with their corners cyclically rolled, so that pair trees see every rotation: cell c rolls
    its first triangle by c % 3 and its second by (c // 3) % 3.  The pairing then stores all nine (rot_a, rot_b)
    combinations in about equal numbers (a plain grid_mesh pairs every cell as (0, 1))."""
    t = tris.reshape(-1, 3, 3).copy()
    i = np.arange(t.shape[0])
    cell = i // 2
    shift = np.where(i % 2 == 0, cell % 3, (cell // 3) % 3)
    for s in (1, 2):
        t[shift == s] = np.roll(t[shift == s], s, axis=1)
    return t.reshape(-1, 9)


def pair_rotations(leaves):
    """rotations (rot_a, rot_b) of the leaves that hold a triangle pair (CreateTrianglePair ids a, a + 1)"""
    paired = leaves["primitive_id_1"] == leaves["primitive_id_0"] + 1
    return leaves["rotations"][paired]


def make_smooth(scenes, ora, G=40, seed=11):
    """A G x G height field (corners rolled by roll_corners) with smooth, distinct per-corner normals and jittered
    per-corner uv (scenes.smooth_uv_attributes), make()'s materials and textures.  Every corner of every triangle
    carries its own normal and uv and the pair trees hold every rotation of both triangles of a pair, so a wrong
    attribute rotation shows in the surface modes."""
    tris = roll_corners(scenes.grid_mesh(G, seed))
    n = tris.shape[0]
    mat_ids = ((np.arange(n, dtype=np.int32) // 2 // 5) % 4).astype(np.int32)
    at = scenes.smooth_uv_attributes(tris, mat_ids, seed=seed, uv_scale=0.21)
    mats, chains = materials_and_chains(scenes, ora, 4)
    cams = {"oblique": scenes.make_camera((4.0, 9.0, 4.0), -0.785, 0.7, 120.0),
            "top": scenes.make_camera((20.0, 30.0, 20.0), 0.0, 1.5, 120.0)}
    return dict(tris=tris, attributes=at, materials=mats, textures=chains, cameras=cams, light=(20.0, 3.0, -10.0))


def make_soup251(scenes, ora, n=2000, seed=21):
    """n separate triangles (no duplicates) with material id i % 251 over 251 materials: kMaterialID's hue then names
    the primitive that was hit modulo 251 (hue steps of 360 / 251 degrees, about 4 LSB).  For kMaterialID and kDiffuse."""
    tris = scenes.soup(n, seed, dup_fraction=0.0, size=0.12)
    mat_ids = (np.arange(n, dtype=np.int32) % 251).astype(np.int32)
    at = scenes.smooth_uv_attributes(tris, mat_ids, seed=seed, uv_jitter=0.01, facing=(-1.0, 1.0, -1.0))
    mats = scenes.default_materials(251)      # untextured: random triangles project to slivers in planar uv
    cams = {"box": scenes.camera_for_box([0, 0, 0], [1, 1, 1])}
    return dict(tris=tris, attributes=at, materials=mats, textures=None, cameras=cams, light=(-1.0, 2.5, -0.5))
