"""CPU tests of tests/instance_motion_ref.py, the numpy restatement the GPU test of instance motion is held to:
- the restated float32 object rays agree with the float64 inverse of the float64 M(t), within what the instancing tests' own
  tolerance (t: 1e-5 relative) allows;
- the interpolated proxy box contains the float64 world box of every instance at sampled times (DESIGN section 23's argument);
- identity matrices at times {0, 0.25, 0.5, 1} give W = I and o' = o exactly;
- the flags;
- the float64 unstable share of the GPU test's own ray sets and times is within the cap that test asserts."""
import numpy as np
import pytest

import instance_motion_ref as imr
import instance_ref as ir
import test_gpu_instances as tgi

SAMPLED = np.concatenate([imr.TIMES, np.linspace(0, 1, 21).astype(np.float32)])


@pytest.fixture(scope="module", autouse=True)
def _record_layout(rt):
    """the scenes below go to the library as they are: the restatement's record must be the library's"""
    assert imr.MOTION_INSTANCE == rt.MOTION_INSTANCE


@pytest.fixture(scope="module")
def comp(scenes):
    return imr.composition(scenes)


def _boxes(blas_tris):
    """the object boxes a tree's root run would give: the triangles' own bounds"""
    return [(t.reshape(-1, 3).min(axis=0), t.reshape(-1, 3).max(axis=0)) for t in blas_tris]


def _scenes(comp):
    blas_tris, inst = comp
    return [("composition", inst), ("static", imr.static_instances(inst)), ("many", imr.many_rigid(blas_tris))]


def test_object_rays_agree_with_the_float64_inverse(comp):
    """The hit distance t is a ratio of lengths measured in object space, so a relative error e of the object ray against the
    exact one moves t by a few e.  Measured here as |x' - x'_64| / (|W_64| (|o - T| + |d|)): the error relative to the magnitude
    of the terms the row sums add, which is what float32 rounding scales with.  The yardstick is the instancing tests' 1e-5."""
    blas_tris, _ = comp
    worst = 0.0
    for name, inst in _scenes(comp):
        rays = tgi._world_rays(imr.union_triangles(blas_tris, inst), 400, seed=5).astype(tgi.RAY)
        times = imr.fixed_times(rays.size, seed=6)
        for k in range(inst.size):
            got, entered = imr.object_rays(rays, times, inst["object_to_world0"][k], inst["object_to_world1"][k])
            assert entered.all(), f"{name}: instance {k} not entered"
            t = times.astype(np.float64)[:, None, None]
            M = (1 - t) * inst["object_to_world0"][k].astype(np.float64) + t * inst["object_to_world1"][k].astype(np.float64)
            W = np.linalg.inv(M[:, :, :3])
            q = rays["origin"].astype(np.float64) - M[:, :, 3]
            o64, d64 = np.einsum("nij,nj->ni", W, q), np.einsum("nij,nj->ni", W, rays["dir"].astype(np.float64))
            scale = np.abs(W).max(axis=(1, 2)) * (np.abs(q).max(axis=1) + np.abs(rays["dir"]).max(axis=1))
            err = max((np.abs(got["origin"] - o64).max(axis=1) / scale).max(), (np.abs(got["dir"] - d64).max(axis=1) / scale).max())
            worst = max(worst, err)
    print(f"object rays: worst relative error {worst:.3e}")
    assert worst <= 1e-5 / 4, f"object rays {worst:.3e} off the float64 inverse: no room under the 1e-5 bound on t"


def test_interpolated_proxy_boxes_contain_the_moving_instances(comp):
    blas_tris, _ = comp
    boxes = _boxes(blas_tris)
    for name, inst in _scenes(comp):
        prox0, prox1, fl = imr.prepare(inst, boxes)
        assert (fl == 0).all()
        for tau in SAMPLED:
            lo, hi = imr.interpolated_proxy_box(prox0, prox1, tau)
            M = imr.matrices_f64(inst, tau)
            for i in range(inst.size):
                blo, bhi = boxes[int(inst["blas"][i])]
                corners = np.array([[(bhi if c & 1 else blo)[0], (bhi if c & 2 else blo)[1], (bhi if c & 4 else blo)[2]]
                                    for c in range(8)], np.float64)
                w = corners @ M[i][:, :3].T + M[i][:, 3]      # an affine image of a box lies in the hull of its corners' images
                assert (w.min(axis=0) >= lo[i]).all() and (w.max(axis=0) <= hi[i]).all(), f"{name}: instance {i} at {tau}"


def test_identity_is_exact(scenes):
    tris = scenes.grid_mesh(8, 2)
    rays = tgi._positive_zeros(tgi._world_rays(tris.astype(np.float64), 200, seed=3).astype(tgi.RAY))
    eye = np.eye(3, 4, dtype=np.float32)
    for tau in (0.0, 0.25, 0.5, 1.0):
        times = np.full(rays.size, tau, np.float32)
        m = imr.matrix_at(eye, eye, times)
        assert (m == eye).all()
        W, det, entered = imr.inverse_f32(m)
        assert entered.all() and (det == 1).all() and (W == np.eye(3, dtype=np.float32)).all()
        got, _ = imr.object_rays(rays, times, eye, eye)
        assert got.tobytes() == rays.tobytes(), f"time {tau}: the identity changed a ray"


def test_flags(comp):
    blas_tris, inst = comp
    boxes = _boxes(blas_tris) + [None]
    eye, nan, zero, mirror = np.eye(3, 4), np.full((3, 4), np.nan), np.zeros((3, 4)), np.diag([-1.0, 1.0, 1.0, 0.0])[:3]
    bad = imr.motion_instance_array([eye, eye, eye, nan, eye, zero, eye, mirror], [eye, eye, nan, eye, zero, eye, mirror, eye],
                                    [5, 2, 0, 0, 0, 0, 0, 0])
    allinst = np.concatenate([inst, bad, imr.half_turn(inst)])
    prox0, prox1, fl = imr.prepare(allinst, boxes)
    assert fl.tolist() == [0] * inst.size + [1, 1, 2, 2, 2, 2, 2, 2] + [0]
    assert (prox0[fl != 0] == 0).all() and (prox1[fl != 0] == 0).all()
    one = ir.prepare(ir.instance_array(list(inst["object_to_world1"]), list(inst["blas"])), boxes)[0]
    assert prox1[:inst.size].tobytes() == one.tobytes()
    # the half turn is not flagged, and at time 0.5 no ray enters it
    half = imr.half_turn(inst)
    _, det, entered = imr.inverse_f32(imr.matrix_at(half["object_to_world0"][0], half["object_to_world1"][0], [0.5, 0.25]))
    assert det[0] == 0 and not entered[0] and entered[1]


# ------------------------------------------------------------------ the GPU test's ray sets: their float64 unstable share
def _unstable_share(blas_tris, inst, rays, times):
    worst = 0.0
    for tau in np.unique(times):
        sel = times == tau
        wt, _, _ = imr.world_triangles(blas_tris, inst, tau)
        ref = tgi._f64_world(wt, rays[sel])
        stable = ref["stable"] & tgi._window_ok(wt, rays[sel], ref)
        worst = max(worst, 1 - stable.mean())
    return worst


def test_unstable_share_of_the_gpu_tests_rays(comp):
    import test_gpu_instance_motion as gim
    blas_tris, _ = comp
    for what, inst, rays, times in gim.ray_sets(blas_tris, comp[1]):
        share = _unstable_share(blas_tris, inst, rays, times)
        print(f"{what}: {rays.size} rays, worst unstable share over its times {100 * share:.2f} %")
        assert share <= 0.02, f"{what}: unstable share {share:.4f}"
