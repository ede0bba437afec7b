"""numpy restatement of instanced deferred shading's gather (rt_abi.h, instanced deferred-shading block): the FLATTENED scene of
an instanced one -- placed corners, placed normals and resolved material ids in float32, in the header's operation order -- and
the mapping of instanced hit records onto it.  rt_shade_frame_instanced's frame is defined as rt_shade_frame's on these arrays.
Also the two scenes of the instanced shading tests (CPU and GPU) and their float64 counterpart.  No GPU."""
from __future__ import annotations

import numpy as np

import instance_ref as ir

MISS = 0xFFFFFFFF
HIT = np.dtype([("t", "<f4"), ("primitive_id", "<u4"), ("u", "<f4"), ("v", "<f4")])
ATTRIBUTES = np.dtype([("normal", "<f4", (3, 3)), ("pad0", "<u4"), ("uv", "<f4", (3, 2)), ("material_id", "<i4"), ("pad1", "<u4")])
SHADE_GEOMETRY = np.dtype([("triangles", "<u8"), ("attributes", "<u8"), ("num_triangles", "<u4"), ("material_base", "<i4"),
                           ("pad", "<u4", 2)])


def place_normals(W, normals, renormalize):
    """n'_r = (W[0][r]*nx + W[1][r]*ny) + W[2][r]*nz in float32 (the transpose of world_to_object's 3x3), then under
    `renormalize` n' * (1 / sqrt((n'x*n'x + n'y*n'y) + n'z*n'z)) where that squared length is positive and finite.
    W float32 [3, 4]; normals [..., 3]."""
    f = np.float32
    W, n = np.asarray(W, f), np.asarray(normals, f)
    nx, ny, nz = n[..., 0], n[..., 1], n[..., 2]
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        out = np.stack([(W[0, r] * nx + W[1, r] * ny) + W[2, r] * nz for r in range(3)], axis=-1).astype(f)
        if renormalize:
            l2 = ((out[..., 0] * out[..., 0] + out[..., 1] * out[..., 1]) + out[..., 2] * out[..., 2]).astype(f)
            ok = (l2 > 0) & np.isfinite(l2)
            inv = (f(1.0) / np.sqrt(np.where(ok, l2, f(1.0)), dtype=f)).astype(f)
            out = np.where(ok[..., None], (out * inv[..., None]).astype(f), out)
    return out.astype(f)


def resolve_material_ids(material_ids, material_base, override=None):
    """attributes[].material_id + material_base (int32, wrapping), replaced by `override` when that is >= 0; the shader's range
    check (outside the table: material 0) comes after and is not applied here"""
    ids = (np.asarray(material_ids, np.int64) + int(material_base) + 2 ** 31) % 2 ** 32 - 2 ** 31
    if override is not None and int(override) >= 0:
        ids = np.full_like(ids, int(override))
    return ids.astype(np.int32)


def flatten(blas_tris, blas_attrs, material_bases, instances, records, instance_materials=None, renormalize=True):
    """The flattened scene.  blas_tris[b] float32 [T_b, 9] (None: a table entry with null pointers), blas_attrs[b] ATTRIBUTES
    [T_b], material_bases[b]; instances (INSTANCE) and records (INSTANCE_RECORD: world_to_object, blas, flags) host arrays;
    instance_materials: None or one int per instance.  An instance whose record is flagged, whose blas is outside the table or
    whose table entry is null contributes no triangle.  Returns (world triangles float32 [N, 9], ATTRIBUTES [N], base int64
    [n + 1]): the flattened id of primitive p of instance k is base[k] + p, for p < base[k + 1] - base[k]."""
    n = len(instances)
    tris, attrs, base = [np.zeros((0, 9), np.float32)], [np.zeros(0, ATTRIBUTES)], np.zeros(n + 1, np.int64)
    for k in range(n):
        base[k + 1] = base[k]
        b = int(records["blas"][k])
        if int(records["flags"][k]) != 0 or b >= len(blas_tris) or blas_tris[b] is None or blas_attrs[b] is None:
            continue
        T = np.asarray(blas_tris[b], np.float32).reshape(-1, 3, 3)
        with np.errstate(over="ignore", invalid="ignore"):
            world = ir.affine_f32(instances["object_to_world"][k], T)
        at = np.zeros(T.shape[0], ATTRIBUTES)
        at["uv"] = blas_attrs[b]["uv"]
        at["normal"] = place_normals(records["world_to_object"][k], blas_attrs[b]["normal"], renormalize)
        at["material_id"] = resolve_material_ids(blas_attrs[b]["material_id"], material_bases[b],
                                                 None if instance_materials is None else instance_materials[k])
        tris.append(world.reshape(-1, 9))
        attrs.append(at)
        base[k + 1] = base[k] + T.shape[0]
    return np.concatenate(tris), np.concatenate(attrs), base


def remap(hits, instance_ids, base):
    """instanced records -> records of the flattened scene: primitive_id = base[k] + p; a record that rt_shade_frame_instanced
    shades as a miss (k outside the instances, a dropped instance, p outside its BLAS) gets RT_MISS, its other fields kept"""
    out = np.array(hits, HIT).reshape(-1).copy()
    k = np.asarray(instance_ids).reshape(-1).view(np.uint32).astype(np.int64)
    n = base.size - 1
    kk = np.minimum(k, max(n - 1, 0))
    count = (base[kk + 1] - base[kk]) if n else np.zeros_like(k)
    p = out["primitive_id"].astype(np.int64)
    ok = (k < n) & (p < count)
    out["primitive_id"] = np.where(ok, (base[kk] if n else 0) + p, MISS).astype(np.uint32)
    return out


def remap_shadow(shadow_instance_ids, num_instances):
    """shadow records for rt_shade_frame on the flattened scene: primitive_id 0 (< N) where the any-hit instanced query named a
    live instance, RT_MISS elsewhere (rt_shade_frame reads nothing else of them)"""
    k = np.asarray(shadow_instance_ids).reshape(-1).view(np.uint32)
    out = np.zeros(k.size, HIT)
    out["primitive_id"] = np.where(k < num_instances, 0, MISS).astype(np.uint32)
    return out


# ------------------------------------------------------------------ float64 counterpart
def exact_records(instances, num_blas):
    """world_to_object as the float64 inverse rounded to float32 (what rt_prepare_instances writes, to a few ulp), blas, flags"""
    rec = np.zeros(len(instances), np.dtype([("world_to_object", "<f4", (3, 4)), ("blas", "<u4"), ("flags", "<u4"),
                                             ("spare", "<u4", 2)]))
    for k in range(len(instances)):
        M = instances["object_to_world"][k].astype(np.float64)
        W3 = np.linalg.inv(M[:, :3])
        rec["world_to_object"][k] = np.hstack([W3, (-W3 @ M[:, 3])[:, None]])
        rec["blas"][k] = instances["blas"][k]
        rec["flags"][k] = 0 if int(instances["blas"][k]) < num_blas else ir.BAD_BLAS
    return rec


def flatten_f64(blas_tris, blas_attrs, material_bases, instances, instance_materials=None):
    """The flattened scene in float64: corners M * p, unit normals of the float64 inverse-transpose; rounded to float32 only
    when stored.  Returns (world triangles float32 [N, 9], ATTRIBUTES [N])."""
    tris, attrs = [], []
    for k in range(len(instances)):
        b = int(instances["blas"][k])
        M = instances["object_to_world"][k].astype(np.float64)
        T = np.asarray(blas_tris[b], np.float64).reshape(-1, 3, 3)
        world = T @ M[:, :3].T + M[:, 3]
        nrm = blas_attrs[b]["normal"].astype(np.float64) @ np.linalg.inv(M[:, :3])     # rows: (M^-T n)^T = n^T M^-1
        nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
        at = np.zeros(T.shape[0], ATTRIBUTES)
        at["uv"], at["normal"] = blas_attrs[b]["uv"], nrm
        at["material_id"] = resolve_material_ids(blas_attrs[b]["material_id"], material_bases[b],
                                                 None if instance_materials is None else instance_materials[k])
        tris.append(world.reshape(-1, 9).astype(np.float32))
        attrs.append(at)
    return np.concatenate(tris), np.concatenate(attrs)


# ------------------------------------------------------------------ the test scenes
def _affine(R, t=(0, 0, 0)):
    return np.hstack([np.asarray(R, np.float64), np.asarray(t, np.float64).reshape(3, 1)])


def _two_blases(scenes, ora):
    """BLAS 0: texture_scene.make_smooth(G=12) (smooth per-corner normals and uv, materials 0..3); BLAS 1: texture_scene.make's
    planar grid at G=10 with its own attributes and material_base 4; one table of 8 materials, make()'s five textures"""
    import texture_scene
    a = texture_scene.make_smooth(scenes, ora, G=12)
    tb = scenes.grid_mesh(10, 9)
    ids = ((np.arange(tb.shape[0], dtype=np.int32) // 2 // 5) % 4).astype(np.int32)
    ab = scenes.planar_uv_attributes(tb, ids, uv_scale=0.21)
    mats, chains = texture_scene.materials_and_chains(scenes, ora, 8)
    return dict(tris=[a["tris"], tb], attrs=[a["attributes"], ab], bases=[0, 4], materials=mats, textures=chains)


def scene_a(scenes, ora, moved=False):
    """Test A: seven instances of the kinds of test_gpu_instances item 4 (rotation, non-uniform scale, mirror, shear,
    translation, a copy overlapping the first, the second BLAS), instance 4 with a material override; laid out on the ground
    plane under an oblique camera, the light low on one side.  moved: another placement of the same instances (the graph test)"""
    sc = _two_blases(scenes, ora)
    R = ir.rotation(0.3, -0.5, 0.9)
    mats = [
        _affine(R, (2, 3, 2)),                                                   # rotation
        _affine(np.diag([0.9, 0.6, 1.3]), (17, 0, 0)),                           # non-uniform scale
        _affine(np.diag([-1.0, 1.0, 1.0]), (12, 0, 17)),                         # mirror (negative determinant)
        _affine([[1, 0.4, 0], [0, 1, 0.3], [0.2, 0, 1]], (15, 0, 17)),           # shear
        _affine(np.eye(3), (29, 1, 3)),                                          # translation
        _affine(R, (2.8, 2.7, 1.7)),                                             # overlaps instance 0
        _affine(ir.rotation(0.1, 0.2, 0.3) * 1.2, (30, 2, 18)),                  # the second BLAS
    ]
    if moved:
        for k, m in enumerate(mats):
            m[:, 3] += (0.4 * k, 0.15 * k, -0.3 * k)
    sc["instances"] = ir.instance_array(mats, [0, 0, 0, 0, 0, 0, 1])
    sc["instance_materials"] = np.array([-1, -1, -1, -1, 6, -1, -1], np.int32)
    sc["cam"] = scenes.make_camera((20.0, 20.0, -11.0), 0.0, 0.8, 200.0)
    sc["light"] = (-12.0, 30.0, 12.0)
    return sc


def scene_c(scenes, ora):
    """Test C: disjoint instances -- rotated, non-uniformly scaled and mirrored copies of BLAS 0, a rotated, scaled BLAS 1 and a
    small rotated copy floating above them that casts the shadows -- seen from above so that most of the frame is covered.

    Every instance flattens the height field (y scale 0.2 - 0.25), which makes the normal matrix matter (the inverse-transpose
    stretches a normal's y five times) and keeps the light off the faces' planes.  The latter is an input condition of the
    float64 comparison (tests/test_instance_shade_ref_cpu.py asserts it): the float32 hit point of a primary ray lies up to
    e ~ 1e-5 off its triangle's plane (an ulp of coordinates below 32 is 3.8e-6; the sum o + d*t and the rounding of t each
    add one), so a shadow ray that leaves at sin(angle to the plane) = |n.l| crosses its own triangle again at t = e / |n.l|,
    beyond its tmin = 0.001 once |n.l| < 0.01 -- a self-shadow the float64 reference, whose hit point is on the plane, neither
    has nor masks.  With a light 30 above the ground and faces tilted at most about 30 degrees |n.l| stays above 0.05."""
    sc = _two_blases(scenes, ora)
    flat = np.diag([1.0, 0.2, 1.0])
    mats = [
        _affine(ir.rotation(0.04, 0.6, -0.03) @ flat, (-2.0, 0.3, 5.0)),          # rotation (mostly about y) of the flattened field
        _affine(np.diag([0.9, 0.25, 1.2]), (15.5, 0, 0)),                        # non-uniform scale
        _affine(np.diag([-1.0, 0.2, 1.0]), (12.5, 0, 15.5)),                     # mirror
        _affine(ir.rotation(0.0, -0.3, 0.0) @ flat * 1.15, (16.5, 0, 18.0)),     # the second BLAS
        _affine(ir.rotation(0.05, 0.4, 0.1) @ np.diag([0.55, 0.2, 0.55]), (8.0, 5.0, 9.0)),   # the occluder, above the others
    ]
    sc["instances"] = ir.instance_array(mats, [0, 0, 0, 1, 0])
    sc["instance_materials"] = None
    sc["cam"] = scenes.make_camera((14.0, 15.0, 14.5), 0.0, 1.5, 200.0)
    sc["light"] = (-16.0, 30.0, 14.0)
    return sc


def grazing(ref):
    """|n.l| per hit pixel of a shade_ref.Reference: the geometric unit normal of the hit triangle against the unit vector from
    the hit point to the light"""
    e1, e2 = ref.Vk[:, 1] - ref.Vk[:, 0], ref.Vk[:, 2] - ref.Vk[:, 0]
    n = np.cross(e1, e2)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    l = ref.light - ref.P
    l /= np.linalg.norm(l, axis=1, keepdims=True)
    return np.abs((n * l).sum(axis=1))
