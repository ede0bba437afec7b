"""GPU test of the traversal-stack edges of the capsule ray query (rt_intersect_rays_capsules): every level of the stack, the
hand-over from LDS to the private spill at level 16 and the dropped pushes beyond 64.

A capsule with p0 == p1 is a sphere, and its test is the sphere block's bit for bit.  So a set of such capsules walked by
rt_intersect_rays_capsules must give, on the same tree, the records and all four counters of rt_intersect_rays_spheres over the
corresponding spheres, byte for byte -- and that query is pinned to the oracle's walker, stack level by stack level, on these very
scenes by tests/test_gpu_stack_depths.py.  Closest hit, any hit and the indexed instantiation, on

  * stack_scenes.sphere_comb(L) for the comb lengths of that file (two leaves hold ids >= the count, one radius is negative);
  * stack_scenes.fractal_spheres of the "deep" fractal on every builder and of the "full" fractal on the SAH builder, with
    stack_scenes.sphere_rays."""
import numpy as np
import pytest

import stack_scenes as sc
import test_gpu_spheres as tgs

pytestmark = pytest.mark.gpu

F = np.float32


def _as_capsules(spheres):
    s = np.ascontiguousarray(spheres, F).reshape(-1, 4)
    c = np.zeros((s.shape[0], 8), F)
    c[:, 0:4] = s
    c[:, 4:7] = s[:, 0:3]
    c[:, 7] = np.nan            # the pad is never read
    return c


def _launch(rt, n, call):
    import torch
    hits = torch.full((n, 4), 0, dtype=torch.int32, device="cuda").fill_(0x5A5A5A5A)
    ctr = torch.zeros(4, dtype=torch.int64, device="cuda")
    call(hits, ctr)
    torch.cuda.synchronize()
    return hits.cpu().numpy().view(np.uint32), ctr.cpu().numpy().astype(np.uint64)


def _same_as_spheres(rt, triangles, nodes, root, count, spheres, rays, what):
    import torch
    n = len(rays)
    d = tgs._dev_rays(rt, rays)
    sp = rt.to_device(np.ascontiguousarray(spheres, F))
    cp = rt.to_device(_as_capsules(spheres))
    ns = len(spheres)
    perm = np.random.default_rng(3).permutation(n)[: 2 * n // 3].astype(np.uint32)
    order = torch.from_numpy(perm.view(np.int32)).cuda()
    hit_rays = 0
    for kw in (dict(), dict(any_hit=True), dict(order=order), dict(order=order, any_hit=True)):
        exp, ectr = _launch(rt, n, lambda h, c: rt.IntersectRaysSpheres(triangles, nodes, root, count, sp, ns, d, h, counters=c, **kw))
        got, gctr = _launch(rt, n, lambda h, c: rt.IntersectRaysCapsules(triangles, nodes, root, count, cp, ns, d, h, counters=c,
                                                                         **kw))
        bad = (got != exp).any(axis=1)
        assert not bad.any(), f"{what} {sorted(kw)}: {bad.sum()} of {n} records differ from the sphere query's (first: ray " \
                              f"{np.nonzero(bad)[0][:5]})"
        assert (gctr == ectr).all(), f"{what} {sorted(kw)}: counters {gctr} vs the sphere query's {ectr}"
        assert ectr[0] > 0 and ectr[1] > 0
        if "order" in kw:
            listed = np.zeros(n, bool)
            listed[perm] = True
            assert (got[~listed] == 0x5A5A5A5A).all(), "unlisted records were written"
        else:
            hit_rays = int((got[:, 1] != sc.MISS).sum())
            assert hit_rays >= sc.AIMED
    print(f"IntersectRaysCapsules {what}: {hit_rays} of {n} rays hit; records and counters are the sphere query's")


@pytest.mark.parametrize("L", sc.COMB_L)
def test_capsule_combs(rt, L):
    c = sc.sphere_comb(L)
    triangles, nodes = rt.to_device(c["leaves"]), rt.to_device(c["nodes"])
    _same_as_spheres(rt, triangles, nodes, c["root"], c["count"], c["spheres"], sc.comb_rays(c["aim"], seed=37 + L), f"comb {L}")


@pytest.mark.parametrize("name,kind", [("deep", k) for k in tgs.KINDS] + [("full", "sah")])
def test_capsule_fractals(rt, scenes, name, kind):
    """deep: every builder; full: the SAH builder's tree alone fills the stack"""
    tris, cam = sc.fractal(name, scenes)
    spheres = sc.fractal_spheres(tris, name)
    s = tgs.Spheres(rt, spheres, kind).frame()
    assert rt.sphere_status(s.status) == 0
    root, count = s.root
    # the capsule proxies of these capsules are the sphere proxies, so this is also the tree rt_prepare_capsules would give
    import torch
    prox = [torch.zeros(36 * len(spheres), dtype=torch.uint8, device="cuda") for _ in range(2)]
    status = torch.zeros((2, 4), dtype=torch.uint8, device="cuda")
    rt.PrepareSpheres(s.spheres, len(spheres), prox[0], status[0])
    rt.PrepareCapsules(rt.to_device(_as_capsules(spheres)), len(spheres), prox[1], status[1])
    torch.cuda.synchronize()
    assert rt.sphere_status(status[0]) == 0 and rt.capsule_status(status[1]) == 0
    assert torch.equal(prox[0], prox[1]) and bool(prox[1].any())
    _same_as_spheres(rt, s.tree.triangles_out, s.tree.nodes_out, root, count, spheres, sc.sphere_rays(name, spheres, cam),
                     f"{name}/{kind}")
