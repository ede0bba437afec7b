"""CPU tests of tests/instance_shade_ref.py: the conditions on the inputs that the GPU tests of instanced deferred shading
(tests/test_gpu_instance_shade.py) rely on.

1. an identity instance returns the input bytes, on a scene asserted to have no -0 component in corners or normals;
2. the flattened normals agree with the float64 inverse-transpose to a few ulp under rotation, non-uniform scale, mirror and
   shear; a rigid rotation keeps their length to 1e-6 without renormalisation;
3. material_base and the per-instance override resolve as specified (a negative override keeps the based id; ids may leave
   the table); remap() sends every record the shader treats as a miss to RT_MISS;
4. the stability mask of the float64 reference of test C's scene stays within shade_ref.MASK_BOUND in modes 3..8, and the scene
   has the hit count test C asks for."""
import numpy as np
import pytest

import instance_ref as ir
import instance_shade_ref as isr
import shade_ref


@pytest.fixture(scope="module")
def blases(scenes, ora):
    return isr._two_blases(scenes, ora)


def test_identity_instance_returns_the_input_bytes(blases):
    for b in (0, 1):
        tris, at = blases["tris"][b], blases["attrs"][b]
        assert not np.signbit(tris[tris == 0]).any() and not np.signbit(at["normal"][at["normal"] == 0]).any(), "no -0 component"
        inst = ir.instance_array([np.eye(3, 4)], [b])
        rec = isr.exact_records(inst, 2)
        assert (rec["world_to_object"][0] == np.eye(3, 4, dtype=np.float32)).all()
        world, flat, base = isr.flatten(blases["tris"], blases["attrs"], [0, 0], inst, rec, None, renormalize=False)
        assert base.tolist() == [0, tris.shape[0]]
        assert world.tobytes() == tris.tobytes()
        assert flat.tobytes() == np.ascontiguousarray(at).tobytes()
        assert flat.dtype == at.dtype


@pytest.mark.parametrize("kind", ["rotation", "scale", "mirror", "shear"])
def test_normals_agree_with_the_float64_inverse_transpose(blases, kind):
    R = {"rotation": ir.rotation(0.3, -0.5, 0.9), "scale": np.diag([1.5, 0.6, 2.0]), "mirror": np.diag([-1.0, 1.0, 1.0]),
         "shear": np.array([[1, 0.4, 0], [0, 1, 0.3], [0.2, 0, 1.0]])}[kind]
    inst = ir.instance_array([isr._affine(R, (3, -2, 5))], [0])
    rec = isr.exact_records(inst, 2)
    n = blases["attrs"][0]["normal"]
    M = inst["object_to_world"][0].astype(np.float64)[:, :3]
    exact = n.astype(np.float64) @ np.linalg.inv(M)                        # rows n^T M^-1 = (M^-T n)^T
    got = isr.place_normals(rec["world_to_object"][0], n, False).astype(np.float64)
    # float32 entries of W (half an ulp each), three products and two sums: a few ulp of the largest term
    scale = np.abs(exact).max(axis=-1, keepdims=True)
    assert (np.abs(got - exact) <= 4 * np.spacing(scale.astype(np.float32))).all()
    unit = isr.place_normals(rec["world_to_object"][0], n, True).astype(np.float64)
    expu = exact / np.linalg.norm(exact, axis=-1, keepdims=True)
    assert np.abs(unit - expu).max() <= 8 * np.spacing(np.float32(1.0))
    if kind == "rotation":
        assert np.abs(np.linalg.norm(got, axis=-1) - np.linalg.norm(n.astype(np.float64), axis=-1)).max() <= 1e-6
    else:
        assert np.abs(np.linalg.norm(got, axis=-1) - 1).max() > 1e-3 or kind == "mirror"
    # the flattened scene carries exactly these normals
    _, flat, _ = isr.flatten(blases["tris"], blases["attrs"], [0, 4], inst, rec, None, renormalize=True)
    assert flat["normal"].tobytes() == isr.place_normals(rec["world_to_object"][0], n, True).tobytes()


def test_renormalisation_keeps_degenerate_normals():
    W = np.eye(3, 4, dtype=np.float32)
    n = np.float32([[0, 0, 0], [np.inf, 0, 0], [np.nan, 1, 0], [1e30, 1e30, 0], [3, 4, 0]])
    got = isr.place_normals(W, n, True)
    assert got[:4].tobytes() == isr.place_normals(W, n, False)[:4].tobytes()      # l2 is 0, inf or NaN: kept
    assert got[4].tolist() == (np.float32([3, 4, 0]) * (np.float32(1) / np.sqrt(np.float32(25)))).tolist()


def test_material_ids_resolve_as_specified(blases):
    ids = np.array([0, 1, 3, -1, 250], np.int32)
    assert isr.resolve_material_ids(ids, 4).tolist() == [4, 5, 7, 3, 254]
    assert isr.resolve_material_ids(ids, 4, -1).tolist() == [4, 5, 7, 3, 254]      # a negative override keeps the based id
    assert isr.resolve_material_ids(ids, 4, 0).tolist() == [0] * 5
    assert isr.resolve_material_ids(ids, 4, 9).tolist() == [9] * 5                 # (may leave the table: the shader's check)
    assert isr.resolve_material_ids(ids, -3).tolist() == [-3, -2, 0, -4, 247]
    assert isr.resolve_material_ids(np.array([2 ** 31 - 1], np.int32), 1).tolist() == [-2 ** 31]   # int32, wrapping
    inst = ir.instance_array([np.eye(3, 4)] * 3, [0, 1, 1])
    rec = isr.exact_records(inst, 2)
    _, flat, base = isr.flatten(blases["tris"], blases["attrs"], blases["bases"], inst, rec, np.array([-1, -1, 2]))
    a, b = blases["attrs"][0]["material_id"], blases["attrs"][1]["material_id"]
    assert (flat["material_id"][base[0]:base[1]] == a).all()
    assert (flat["material_id"][base[1]:base[2]] == b + 4).all() and set(b.tolist()) == {0, 1, 2, 3}
    assert (flat["material_id"][base[2]:base[3]] == 2).all()


def test_remap_sends_what_the_shader_calls_a_miss_to_miss(blases):
    inst = ir.instance_array([np.eye(3, 4)] * 4, [0, 1, 7, 1])
    rec = isr.exact_records(inst, 2)
    assert rec["flags"].tolist() == [0, 0, ir.BAD_BLAS, 0]
    rec["flags"][3] = ir.SINGULAR
    na, nb = blases["tris"][0].shape[0], blases["tris"][1].shape[0]
    _, _, base = isr.flatten(blases["tris"], blases["attrs"], blases["bases"], inst, rec)
    assert base.tolist() == [0, na, na + nb, na + nb, na + nb]
    hits = np.zeros(8, isr.HIT)
    hits["t"] = np.arange(8)
    hits["primitive_id"] = [5, na - 1, na, 0, nb, 3, 3, isr.MISS]
    ids = np.array([0, 0, 0, 1, 1, 2, 3, isr.MISS], np.uint32)
    got = isr.remap(hits, ids, base)
    assert got["primitive_id"].tolist() == [5, na - 1, isr.MISS, na, isr.MISS, isr.MISS, isr.MISS, isr.MISS]
    assert (got["t"] == hits["t"]).all()
    assert isr.remap(hits, np.full(8, 4, np.uint32), base)["primitive_id"].tolist() == [isr.MISS] * 8
    assert isr.remap(hits, ids, np.zeros(1, np.int64))["primitive_id"].tolist() == [isr.MISS] * 8     # no instances
    # a null table entry drops its instances
    _, _, base2 = isr.flatten([blases["tris"][0], None], [blases["attrs"][0], None], blases["bases"], inst, rec)
    assert base2.tolist() == [0, na, na, na, na]
    assert isr.remap_shadow(np.array([0, 3, 4, isr.MISS], np.uint32), 4)["primitive_id"].tolist() == [0, 0, isr.MISS, isr.MISS]


def test_scene_c_mask_within_bounds(scenes, ora):
    sc = isr.scene_c(scenes, ora)
    tris, at = isr.flatten_f64(sc["tris"], sc["attrs"], sc["bases"], sc["instances"], sc["instance_materials"])
    ref = shade_ref.Reference(tris, at, sc["materials"], sc["textures"], sc["light"], sc["cam"], 160, 100)
    assert int(ref.hit.sum()) >= 10_000
    dets = [np.linalg.det(m[:, :3].astype(np.float64)) for m in sc["instances"]["object_to_world"]]
    assert min(dets) < 0 < max(dets), "a mirrored instance among the others"
    # disjoint instances: no two world boxes overlap
    bounds = np.cumsum([0] + [sc["tris"][int(b)].shape[0] for b in sc["instances"]["blas"]])
    boxes = [(tris[a:b].reshape(-1, 3).min(axis=0), tris[a:b].reshape(-1, 3).max(axis=0)) for a, b in zip(bounds[:-1], bounds[1:])]
    for i in range(len(boxes)):
        for j in range(i):
            assert (boxes[i][0] > boxes[j][1]).any() or (boxes[j][0] > boxes[i][1]).any(), f"instances {j} and {i} overlap"
    # no grazing light (scene_c's docstring: a float32 hit point then shadows itself beyond tmin, which float64 does not see),
    # and the shadow mode has both kinds of pixel
    assert isr.grazing(ref).min() >= 0.05
    shadow = ref.shadow()
    assert int(shadow["hit"].sum()) >= 500 and int((~shadow["hit"] & ~shadow["unstable"]).sum()) >= 5000
    for mode in (3, 4, 5, 6, 7, 8):
        _, stable, hit = ref.frame(mode)
        masked = float((hit & ~stable).sum()) / int(hit.sum())
        print(f"mode {mode}: masked {100 * masked:.2f} %")
        assert masked <= shade_ref.MASK_BOUND[mode], f"mode {mode}: {masked:.4f}"
    # the float32 flattening of the same scene is the float64 one to float32 rounding
    rec = isr.exact_records(sc["instances"], 2)
    w32, a32, base = isr.flatten(sc["tris"], sc["attrs"], sc["bases"], sc["instances"], rec, None, True)
    assert base[-1] == tris.shape[0] and np.abs(w32.astype(np.float64) - tris).max() <= 1e-5
    assert np.abs(a32["normal"].astype(np.float64) - at["normal"]).max() <= 1e-6
    assert (a32["material_id"] == at["material_id"]).all()
