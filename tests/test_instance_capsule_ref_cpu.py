"""CPU test of tests/instance_capsule_ref.py, the numpy restatement the GPU tests of rt_intersect_rays_instanced_mixed_capsules
are held against: the world is the issue's composition (the fibres where the lattice was, a rotation, a mirror, a non-uniform
scale and a shear on the capsule BLAS, the two added instances clear of the others); for every seed the GPU tests use the
unstable share is within instance_mixed_ref's cap, each of the three kinds has at least 200 stable hits and each capsule
instance is hit; the far-root problem has at least 50 stable far-root hits; the float32 per-instance arithmetic of the header
agrees with the float64 winner on stable capsule hits within T_TOL, which is the measurement rounded up and nothing more; and
no stable capsule hit is culled by its padded leaf box in object space."""
import numpy as np
import pytest

import capsule_ref as cr
import instance_capsule_ref as icr
import instance_mixed_ref as mr

F = np.float32


def test_world_is_the_issue_s_composition():
    w, base = icr.world(), mr.world()
    assert w.n == 10 and len(w.data) == 4 and w.kinds == (0, 0, 1, 2)
    assert all(w.data[b] is base.data[b] or (w.data[b] == base.data[b]).all() for b in (0, 1, 2))
    assert w.data[3].shape == (1504, 8) and (~cr.valid(w.data[3])).sum() == 4
    assert w.instances[:8].tobytes() == base.instances.tobytes(), "instances 0..7 are instance_mixed_ref's"
    assert w.capsule_inst.tolist() == [2, 5, 8, 9] and w.sphere_inst.tolist() == [1, 3, 7]
    # the capsule placements: a mirror, a rotation, a non-uniform scale, a shear
    L = {i: w.M[i][:, :3] for i in w.capsule_inst}
    assert np.linalg.det(L[2]) < 0
    G = L[5].T @ L[5]
    assert np.allclose(G, G[0, 0] * np.eye(3), rtol=1e-6, atol=1e-5) and not np.allclose(L[5], np.diag(np.diag(L[5])))
    assert np.count_nonzero(L[8] - np.diag(np.diag(L[8]))) == 0 and len(set(np.diag(L[8]).tolist())) == 3
    G = L[9].T @ L[9]
    assert np.abs(G - np.diag(np.diag(G))).max() > 0.1 * G.max(), "instance 9 is not sheared"
    # instance 5 (capsules) overlaps instance 0 (triangles); 8 and 9 are clear of every other instance
    b = w.boxes()
    assert (np.maximum(b[0][0], b[5][0]) < np.minimum(b[0][1], b[5][1])).all()
    for i in (8, 9):
        for j in range(w.n):
            assert j == i or not (np.maximum(b[i][0], b[j][0]) < np.minimum(b[i][1], b[j][1])).all(), (i, j)


@pytest.mark.parametrize("seed", icr.SEEDS)
def test_unstable_share_and_coverage(seed):
    ref = icr.reference(seed)
    w, f, st = ref.world, ref.f64, ref.stable
    assert ref.rays.size <= 3000 and (ref.rays["tmax"] < np.inf).sum() == ref.rays.size // 2
    hit = st & f["hit"]
    kinds = [hit & (f["kind"] == k) for k in (icr.TRIANGLES, icr.SPHERES, icr.CAPSULES)]
    per_inst = {int(i): int((hit & (f["inst"] == i)).sum()) for i in w.capsule_inst}
    print(f"seed {seed}: unstable {100 * ref.unstable_share:.2f} %, stable hits on triangles {kinds[0].sum()}, on spheres "
          f"{kinds[1].sum()}, on capsules {kinds[2].sum()} (per instance {per_inst}), far-root capsule hits "
          f"{int((kinds[2] & f['far']).sum())}")
    assert ref.unstable_share <= icr.CAP
    assert all(k.sum() >= 200 for k in kinds)
    assert all(n > 0 for n in per_inst.values()), "a capsule instance is never hit"
    for k, m in enumerate(kinds):
        assert (w.inst_kind[f["inst"][m]] == k).all()
    # the invalid capsules are never the answer
    for i in w.capsule_inst:
        assert cr.valid(w.data[w.blas[i]])[f["prim"][kinds[2] & (f["inst"] == i)]].all()


def test_far_root_problem():
    ref = icr.far_reference()
    f, st = ref.f64, ref.stable
    far = st & f["hit"] & f["far"]
    print(f"far problem: {ref.rays.size} rays, unstable {100 * ref.unstable_share:.2f} %, stable far-root hits {far.sum()}, "
          f"near-root hits {int((st & f['hit'] & ~f['far']).sum())}")
    assert ref.unstable_share <= icr.CAP
    assert far.sum() >= 50
    assert (f["kind"][st & f["hit"]] == icr.CAPSULES).all()
    L = ref.world.M[0][:, :3]
    G = L.T @ L
    assert G.max() > 3.9 * np.diag(G).min(), "the placement is not non-uniform"


def test_t_tolerance_is_the_measurement():
    errs = [icr.t_error_f32(icr.reference(seed)) for seed in icr.SEEDS]
    far = icr.t_error_f32(icr.far_reference())
    print("float32 restatement against float64, |t32 - t64| / max(1, |t64|): world " +
          ", ".join(f"{e:.3g}" for e in errs) + f"; far problem {far:.3g}")
    pair = icr.t_error_f32(icr.pair_reference())
    graph = [icr.t_error_f32(r) for r in icr.graph_references().values()]
    print(f"two-capsule set {pair:.3g}; graph poses " + ", ".join(f"{e:.3g}" for e in graph))
    for r in (icr.pair_reference(), *icr.graph_references().values()):
        assert r.unstable_share <= icr.CAP
    for got, const in ((max(errs), icr.T_TOL), (far, icr.T_TOL_FAR), (pair, icr.T_TOL_PAIR), (max(graph), icr.T_TOL_GRAPH)):
        assert got <= const, f"measured {got:.3g} exceeds the constant {const:.3g}"
        assert const <= 1.1 * got, f"the constant {const:.3g} is more than the measurement {got:.3g} rounded up to two digits"


@pytest.mark.parametrize("seed", icr.SEEDS)
def test_float32_per_instance_agrees_with_float64_and_no_hit_is_culled(seed):
    ref = icr.reference(seed)
    w, f, st, rays = ref.world, ref.f64, ref.stable, ref.rays
    caps = st & f["hit"] & (f["kind"] == icr.CAPSULES)
    for i in w.capsule_inst:
        m = np.flatnonzero(caps & (f["inst"] == i))
        data = w.data[w.blas[i]]
        t, far, v = icr.capsule_f32(w, rays[m], i, f["prim"][m])
        assert not np.isnan(t).any(), f"instance {i}: a stable capsule hit is rejected in float32"
        assert (far == f["far"][m]).all(), f"instance {i}: another root than float64's"
        assert ((v >= 0) & (v <= 1)).all()
        # no stable capsule hit is culled by its padded leaf box: the slab test on the object ray with tmax shrunk to the hit
        prox, _, _ = cr.prepare_f32(data)
        obj = mr.ir.object_rays(rays[m], w.inverse32(i))
        ok = cr.slab_f32(obj, prox[f["prim"][m], 0:3], prox[f["prim"][m], 3:6], t)
        assert ok.all(), f"instance {i}: {int((~ok).sum())} stable hits culled by their padded box"
