"""CPU test of tests/instance_mixed_ref.py, the numpy restatement the GPU tests of rt_intersect_rays_instanced_mixed are held
against: for the mixed world and every seed the GPU tests use, the unstable share is within the cap, the batch covers both
kinds of instance, the float32 per-instance arithmetic of the header agrees with the float64 winner on stable rays, and no
stable sphere hit is culled by its padded leaf box in object space."""
import numpy as np
import pytest

import instance_mixed_ref as mr
import sphere_ref as sr

F = np.float32


@pytest.mark.parametrize("seed", mr.SEEDS)
def test_unstable_share_and_coverage(seed):
    ref = mr.reference(seed)
    w, f, st = ref.world, ref.f64, ref.stable
    assert ref.rays.size <= 3000 and (ref.rays["tmax"] < np.inf).sum() == ref.rays.size // 2
    hit = st & f["hit"]
    tri, sph = hit & (f["kind"] == mr.TRIANGLES), hit & (f["kind"] == mr.SPHERES)
    print(f"seed {seed}: unstable {100 * ref.unstable_share:.2f} %, stable hits on triangles {tri.sum()}, on spheres {sph.sum()}, "
          f"far roots {int((sph & f['far']).sum())}, instances {sorted(set(f['inst'][hit].tolist()))}")
    assert ref.unstable_share <= mr.CAP
    assert tri.sum() >= 200 and sph.sum() >= 200
    assert len(set(f["inst"][hit].tolist())) >= 6
    assert (sph & f["far"]).sum() > 0, "no far-root sphere hit in the batch"
    assert (w.inst_kind[f["inst"][tri]] == mr.TRIANGLES).all() and (w.inst_kind[f["inst"][sph]] == mr.SPHERES).all()
    # the invalid spheres of both sets are never the answer
    for i in w.sphere_inst:
        ids = f["prim"][sph & (f["inst"] == i)]
        assert sr.valid(w.data[w.blas[i]])[ids].all()


def test_world_is_the_issue_s_composition():
    w = mr.world()
    assert w.n == 8 and len(w.data) == 4 and w.kinds == (0, 0, 1, 1)
    assert 900 <= w.data[0].shape[0] <= 1300 and w.data[1].shape[0] == 512
    assert (~sr.valid(w.data[2])).sum() == 4 and (~sr.valid(w.data[3])).sum() == 4
    dets = [np.linalg.det(w.M[i][:, :3]) for i in range(8)]
    assert dets[2] < 0 and all(d != 0 for d in dets)
    # instance 5 (spheres) overlaps instance 0 (triangles)
    b = w.boxes()
    assert w.inst_kind[5] == mr.SPHERES and w.inst_kind[0] == mr.TRIANGLES
    assert (np.maximum(b[0][0], b[5][0]) < np.minimum(b[0][1], b[5][1])).all()


@pytest.mark.parametrize("seed", mr.SEEDS)
def test_float32_per_instance_agrees_with_float64_and_no_hit_is_culled(seed):
    ref = mr.reference(seed)
    w, f, st, rays = ref.world, ref.f64, ref.stable, ref.rays
    n = rays.size
    # float32 minimum over the sphere instances
    best_t, best_inst, best_id, best_far = np.full(n, np.inf, F), np.full(n, -1), np.full(n, -1), np.zeros(n, bool)
    objs = {}
    for i in w.sphere_inst:
        t, arg, far, objs[i] = mr.sphere_f32(w, rays, i)
        take = t < best_t
        best_t, best_inst, best_id, best_far = (np.where(take, v, b) for v, b in ((t, best_t), (i, best_inst), (arg, best_id),
                                                                                   (far, best_far)))
    t64 = f["t"]
    sph = st & f["hit"] & (f["kind"] == mr.SPHERES)
    assert (best_inst[sph] == f["inst"][sph]).all(), "float32 picks another sphere instance than float64 on a stable ray"
    for i in w.sphere_inst:
        m = sph & (f["inst"] == i)
        assert (w.canon[w.blas[i]][best_id[m]] == f["prim"][m]).all(), f"instance {i}: another sphere than float64's"
    assert (best_far[sph] == f["far"][sph]).all()
    assert (np.abs(best_t[sph] - t64[sph]) <= 1e-5 * np.maximum(1, t64[sph])).all()
    # a stable triangle winner or a stable miss: no sphere instance comes first in float32
    assert (best_t[st & ~f["hit"]] == np.inf).all()
    tri = st & f["hit"] & (f["kind"] == mr.TRIANGLES)
    assert (best_t[tri] > t64[tri]).all()
    # ... and the triangle itself is hit by the float32 object ray at float64's t
    for i in np.unique(f["inst"][tri]):
        m = np.flatnonzero(tri & (f["inst"] == i))
        obj = mr.ir.object_rays(rays[m], w.inverse32(i))
        t = mr.tri_t_f32(w.data[w.blas[i]], obj, f["prim"][m])
        assert not np.isnan(t).any(), f"instance {i}: a stable triangle hit is rejected in float32"
        assert (np.abs(t - t64[m]) <= 1e-5 * np.maximum(1, t64[m])).all()
    # no stable sphere hit is culled by its padded leaf box: the slab test on the object ray with tmax shrunk to the hit
    for i in w.sphere_inst:
        m = np.flatnonzero(sph & (f["inst"] == i))
        prox, _, _ = sr.prepare_f32(w.data[w.blas[i]])
        ids = best_id[m]
        ok = sr.slab_f32(objs[i][m], prox[ids, 0:3], prox[ids, 3:6], best_t[m])
        assert ok.all(), f"instance {i}: {int((~ok).sum())} stable hits culled by their padded box"
