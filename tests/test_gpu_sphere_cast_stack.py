"""GPU test of the traversal-stack edges of the sphere cast (rt_sphere_cast): every level of the stack, the hand-over from LDS
to the private spill at level 16 and the dropped pushes beyond 64.

A ray of radius 0 runs the ray query's tests on boxes grown by exactly 0.  So with `radii` all zero rt_sphere_cast must give,
on the same tree, the records and the counters of rt_intersect_rays, byte for byte -- and that query is pinned to the oracle's
walker, stack level by stack level, on these very scenes by tests/test_gpu_stack_depths.py, so the oracle needs no sweep walker.
Closest hit, any hit and the indexed instantiation (against rt_intersect_rays_indexed), on

  * stack_scenes.tri_comb(L) for the comb lengths of that file;
  * the "deep" fractal through every builder and the "full" fractal through the SAH builder (full stack, dropped pushes),
    with stack_scenes.fractal_rays.

All four counters are compared, the wave steps [2] and [3] too: the two loops' vote shapes coincide here.  rt_intersect_rays
takes its plain (no hold-at-pop) vote / park loop, the cast's loop is that loop, and these trees are far below the
primitive count at which rt_intersect_rays switches to its pair-prefetch instantiation (whose votes are the same, but the
claim is only made for the plain one); with every radius 0 each lane's phase sequence is the ray query's, so every ballot is.
A second pass with the uniform `radius` = 0 and no `radii` array must give the same bytes."""
import numpy as np
import pytest

import stack_scenes as sc
import test_gpu_ray_queries as rq

pytestmark = pytest.mark.gpu

F = np.float32
KINDS = ("bottom_up", "hybrid", "sah")


def _launch(rt, n, call):
    import torch
    hits = torch.full((n, 4), 0, dtype=torch.int32, device="cuda").fill_(0x5A5A5A5A)
    ctr = torch.zeros(4, dtype=torch.int64, device="cuda")
    call(hits, ctr)
    torch.cuda.synchronize()
    return hits.cpu().numpy().view(np.uint32), ctr.cpu().numpy().astype(np.uint64)


def _same_as_ray_query(rt, triangles, nodes, root, count, rays, what):
    import torch
    n = len(rays)
    d = rt.to_device(np.ascontiguousarray(rays, rt.RAY)).view(torch.float32).view(-1, 8)
    zeros = torch.zeros(n, dtype=torch.float32, device="cuda")
    perm = np.random.default_rng(3).permutation(n)[: 2 * n // 3].astype(np.uint32)
    order = torch.from_numpy(perm.view(np.int32)).cuda()
    hit_rays = 0
    for any_hit in (False, True):
        for indexed in (False, True):
            if indexed:
                exp, ectr = _launch(rt, n, lambda h, c: rt.IntersectRaysIndexed(triangles, nodes, root, count, d, order, h,
                                                                                any_hit=any_hit, counters=c))
            else:
                exp, ectr = _launch(rt, n, lambda h, c: rt.IntersectRays(triangles, nodes, root, count, d, h, any_hit=any_hit,
                                                                         counters=c))
            kw = dict(order=order) if indexed else {}
            for radii in (zeros, None):
                feats = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
                got, gctr = _launch(rt, n, lambda h, c: rt.SphereCast(triangles, nodes, root, count, d, h, radii=radii, radius=0.0,
                                                                      features=feats, any_hit=any_hit, counters=c, **kw))
                mode = f"{what} any_hit={any_hit} indexed={indexed} radii={'array' if radii is not None else 'uniform'}"
                bad = (got != exp).any(axis=1)
                assert not bad.any(), f"{mode}: {bad.sum()} of {n} records differ from the ray query's (first: ray " \
                                      f"{np.nonzero(bad)[0][:5]})"
                assert (gctr == ectr).all(), f"{mode}: counters {gctr} vs the ray query's {ectr}"
                assert ectr[0] > 0 and ectr[1] > 0
                f = feats.cpu().numpy().view(np.uint32)
                written = got[:, 1] != 0x5A5A5A5A
                assert (f[written] == np.where(got[written, 1] != sc.MISS, rt.RT_SWEEP_FACE, rt.RT_SWEEP_NONE)).all(), mode
                if indexed:
                    listed = np.zeros(n, bool)
                    listed[perm] = True
                    assert (got[~listed] == 0x5A5A5A5A).all() and (f[~listed] == 0x5A5A5A5A).all(), "unlisted records were written"
                else:
                    hit_rays = int((got[:, 1] != sc.MISS).sum())
                    assert hit_rays >= sc.AIMED
    print(f"SphereCast {what}: {hit_rays} of {n} rays hit; records and counters are the ray query's")


@pytest.mark.parametrize("L", sc.COMB_L)
def test_cast_combs(rt, L):
    c = sc.tri_comb(L)
    triangles, nodes = rt.to_device(c["leaves0"]), rt.to_device(c["nodes0"])
    _same_as_ray_query(rt, triangles, nodes, c["root"], c["count"], sc.comb_rays(c["aim"], seed=41 + L), f"comb {L}")


@pytest.mark.parametrize("name,kind", [("deep", k) for k in KINDS] + [("full", "sah")])
def test_cast_fractals(rt, scenes, name, kind):
    """deep: every builder; full: the SAH builder's tree alone fills the stack"""
    tris, cam = sc.fractal(name, scenes)
    inp, root, count = rq._gpu_tree(rt, tris, kind)
    _same_as_ray_query(rt, inp.triangles_out, inp.nodes_out, root, count, sc.fractal_rays(name, tris, cam), f"{name}/{kind}")
