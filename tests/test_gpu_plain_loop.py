"""The plain-loop queries take the same steps when their primitives are the same.

The motion, sphere, capsule and sphere-cast queries walk through one vote / park loop (csrc/rt_plain_traverse.hpp), which is
the loop rt_intersect_rays takes below the pair-prefetch size (trace_ray's plain arm).  So on one tree and one batch of rays

  * rt_sphere_cast with radius 0 (the grown boxes are the stored ones: x - +0 == x; the leaf test is intersect_tri alone),
  * rt_intersect_rays_motion with both poses the SAME arrays and every time 0 (w0 = 1, tau = 0: 1 * a + 0 * a is a), and
  * rt_intersect_rays (num_primitives = 0: the instantiation without the pair prefetch and without the hold at pop)

make the same box tests ([0]) and leaf visits ([1]) per ray and, wave by wave, the same votes: [2] (two box steps per vote
that did not end the box phase) and [3] (leaf phases) are equal too, and so are the records.  Closest hit and any hit, one
tree per builder, a scene of 288 triangles (wide_trees' grid) and a three-triangle tree (small_scenes' n3), 200 rays of
the scene's own ray set (from outside and inside the box, aimed at triangles): three full waves and a partial one.  A
change to the park rule, the two-steps-per-vote rule or the leaf tail that reaches one of the loops and not the others
moves [2] / [3] of that query alone.  The sphere and capsule queries are not compared here: their primitives are not
triangles, so no other query walks the same leaves; their own files hold them to their references."""
import numpy as np
import pytest

import small_scenes as ss
import test_gpu_ray_queries as rq
import wide_trees as wt

pytestmark = pytest.mark.gpu

SCENES = ("grid", "n3")
NUM_RAYS = 200


@pytest.fixture(scope="module")
def batches(scenes):
    """{scene: (triangles, 200 rays spread over every kind of the scene's ray set)}"""
    out = {}
    for name in SCENES:
        src = wt if name == "grid" else ss
        t = src.tris(name, scenes)
        r = src.rays(name, t)
        assert len(r) >= NUM_RAYS
        out[name] = (t, np.ascontiguousarray(r[np.linspace(0, len(r) - 1, NUM_RAYS).astype(np.int64)]))
    return out


def _run(rt, launch, n):
    """launch(hits, counters) -> (HIT [n], counters uint64[4])"""
    import torch
    hits = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    ctr = torch.zeros(4, dtype=torch.int64, device="cuda")
    launch(hits, ctr)
    torch.cuda.synchronize()
    return hits.cpu().numpy().view(rt.HIT).reshape(-1), ctr.cpu().numpy().astype(np.uint64)


@pytest.mark.parametrize("tree", rq.TREES)
@pytest.mark.parametrize("name", SCENES)
def test_same_steps_on_the_same_primitives(rt, batches, name, tree):
    import torch
    tris, rays = batches[name]
    inp, root, count = rq._gpu_tree(rt, tris, tree)
    d = rt.to_device(np.ascontiguousarray(rays, rt.RAY)).view(torch.float32).view(-1, 8)
    zeros = torch.zeros(NUM_RAYS, dtype=torch.float32, device="cuda")
    tl, nd = inp.triangles_out, inp.nodes_out
    for any_hit in (False, True):
        got = {
            "rays": _run(rt, lambda h, c: rt.IntersectRays(tl, nd, root, count, d, h, any_hit=any_hit, counters=c), NUM_RAYS),
            "cast": _run(rt, lambda h, c: rt.SphereCast(tl, nd, root, count, d, h, radius=0.0, any_hit=any_hit, counters=c),
                         NUM_RAYS),
            "motion": _run(rt, lambda h, c: rt.IntersectRaysMotion(inp, inp, root, count, d, zeros, h, any_hit=any_hit,
                                                                   counters=c), NUM_RAYS),
        }
        exp_hits, exp_ctr = got["rays"]
        for k in ("cast", "motion"):
            hits, ctr = got[k]
            what = f"{name} {tree} any_hit={any_hit}: {k}"
            assert (ctr == exp_ctr).all(), f"{what} counters {ctr.tolist()} vs the ray query's {exp_ctr.tolist()}"
            assert hits.tobytes() == exp_hits.tobytes(), f"{what}: records differ from the ray query's"
        assert exp_ctr[2] > 0 and exp_ctr[3] > 0, "no vote was counted"
