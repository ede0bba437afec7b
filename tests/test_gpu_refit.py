"""GPU tests of the refit (rt_build_refit_plan + rt_refit) on every tree the builders make (the eight of
test_gpu_ray_queries.TREES) and five scenes.
1. identity: refit with the build's own triangles gives back the build's bytes over the whole nodes_out / triangles_out
   buffers (signed_zero: boxes equal as numbers; split trees: equal to the numpy reference refit, tests/refit_ref.py);
2. scale by 2: Refit(tree(P), 2P) equals a GPU build(2P) byte for byte on every reachable slot and record (no splits);
3. smooth deformation: nodes and leaves equal refit_ref over the whole buffers, the reference's checker accepts the tree,
   rt_trace kDepth / kDiffuse frames and counters equal the oracle's over the same bytes, IntersectRays closest hits agree with
   a float64 brute force over the deformed triangles;
4. broken pairs: RT_REFIT_PAIR_BROKEN on the pair trees only; the other trees still pass 3's checks;
5. a round trip P0 -> 2 P0 -> P1 -> P0 gives the identity refit's bytes back (the arrival counters clean up after themselves);
6. plan misuse: another tree's nodes, root or count set RT_REFIT_PLAN_MISMATCH and write nothing;
7. n = 1, 2, 3;  8. Refit + IntersectRays captured in a HIP graph, replayed with three vertex sets;  9. the 1M bench mesh."""
import numpy as np
import pytest

import refit_ref
import test_gpu_ray_queries as rq

pytestmark = pytest.mark.gpu

TREES, SCENES = rq.TREES, rq.SCENES
W, H = 67, 45


# ------------------------------------------------------------------ helpers
def _smooth(tris, amp=0.05, phase=0.0):
    """p + amp * E * sin(3 q.yzx + phase), q = (p - lo) / E: a function of the position alone, so shared corners stay shared"""
    P = tris.reshape(-1, 3).astype(np.float64)
    lo, E = P.min(axis=0), float(np.ptp(P, axis=0).max()) or 1.0
    q = (P - lo) / E
    return (P + amp * E * np.sin(3.0 * q[:, [1, 2, 0]] + phase)).astype(np.float32).reshape(-1, 9)


def _bytes(t):
    return t.cpu().numpy().copy()


def _arrays(inp, rt):
    """the whole nodes_out / triangles_out buffers as NODE / TRIANGLE_PAIR arrays"""
    nodes = _bytes(inp.nodes_out)
    leaves = _bytes(inp.triangles_out)
    return leaves[:leaves.size // 64 * 64].view(rt.TRIANGLE_PAIR), nodes.view(rt.NODE)


def _reachable(nodes, root, count):
    """reachable slots, walked level by level in numpy"""
    r = np.zeros(nodes.shape[0], bool)
    f, k = np.array([root], np.int64), np.array([count], np.int64)
    while f.size:
        s = np.repeat(f, k) + (np.arange(k.sum()) - np.repeat(np.cumsum(k) - k, k))
        r[s] = True
        box = s[(nodes["w28"][s] >> 29) == 1]
        f, k = (nodes["w28"][box] & 0x1FFFFFFF).astype(np.int64), (nodes["w12"][box] >> 29).astype(np.int64)
    return r


def _refit(rt, inp, root, count, plan, tris):
    import torch
    inp.triangles_in.copy_(rt.to_device(np.ascontiguousarray(tris, np.float32)))
    rt.Refit(inp, root, count, plan)
    torch.cuda.synchronize()
    return rt.refit_status(plan, inp.num_triangles)


def _plan(rt, inp, root, count):
    plan = rt.device_bytes(rt.RefitPlanBytes(inp.num_triangles))
    rt.BuildRefitPlan(inp, root, count, plan)
    assert rt.refit_status(plan, inp.num_triangles) == 0
    return plan


def _same_boxes_numerically(a, b):
    """boxes equal as numbers (+0 == -0) or as bytes (slots the builder never wrote may hold NaN patterns)"""
    def eq(f):
        return ((a[f] == b[f]) | (a[f].view(np.uint32) == b[f].view(np.uint32))).all()
    return eq("min") and eq("max") and (a["w12"] == b["w12"]).all() and (a["w28"] == b["w28"]).all()


def _check_against_reference(rt, ora, before, after, root, count, tris, what):
    """after == refit_ref(before, tris) over the whole buffers; the reference's checker accepts it.  (The checker unions a
    run's NONE slots too, whose boxes a refit leaves alone: it applies where no box slot's run holds one -- every tree here
    but the one-leaf trees.)"""
    (l0, n0), (l1, n1) = before, after
    el, en, broken = refit_ref.refit_ref(l0, n0, root, count, tris)
    assert l1.tobytes() == el.tobytes(), f"{what}: leaf records differ from the reference refit"
    assert n1.tobytes() == en.tobytes(), f"{what}: nodes differ from the reference refit"
    runs = refit_ref.walk(n0, root, count)
    none_in_runs = any(p is not None and ((n0["w28"][f:f + k] >> 29) == 0).any() for f, k, p in runs)
    leaves = sum(int(((n0["w28"][f:f + k] >> 29) == 2).sum()) for f, k, _ in runs)
    assert not none_in_runs or leaves == 1, f"{what}: a NONE slot inside a run of a tree with {leaves} leaves"
    if not none_in_runs and ora.ref_available():
        assert ora.ref_verify_hierarchy(n1, root, count) == "", what
    return broken


def _check_trace(rt, ora, scenes, inp, root, count, leaves, nodes, tris, cam, what):
    """rt_trace kDepth and kDiffuse frames and counters through the refitted tree == the oracle over the same bytes"""
    import torch
    at = scenes.flat_attributes(tris, np.arange(tris.shape[0]) % 3)
    mats = scenes.default_materials(3)
    light = (0.3, 5.0, -2.0)
    for rtype in (rt.kDepth, rt.kDiffuse):
        kw = {} if rtype == rt.kDepth else dict(attributes=at, materials=mats, light=light)
        oi, oc = ora.trace(leaves, nodes, root, count, cam, W, H, render_type=rtype, **kw)
        rgba = torch.zeros(W * H * 4, dtype=torch.uint8, device="cuda")
        ctr = torch.zeros(4, dtype=torch.int64, device="cuda")
        dkw = {} if rtype == rt.kDepth else dict(attributes=rt.to_device(at), materials=rt.to_device(mats), num_materials=3,
                                                  light=light)
        rt.Trace(inp.triangles_out, inp.nodes_out, rgba, (W, H), rt.to_device(cam), root, count, render_type=rtype,
                 counters=ctr, **dkw)
        torch.cuda.synchronize()
        gi = rgba.cpu().numpy().reshape(H, W, 4)
        assert (gi == oi).all(), f"{what}: render type {rtype}: {(gi != oi).any(axis=2).sum()} pixels differ from the oracle"
        assert (ctr.cpu().numpy().astype(np.uint64)[:2] == oc[:2]).all(), f"{what}: counters"


def _check_rays(rt, name, g, tris, what):
    if name not in ("grid", "soup", "cornell"):
        return
    rays = rq._ray_sets(tris, seed=23)["outside"]
    hits, _ = rq._query(rt, g, rays)
    ref = rq._f64(tris, rays)
    rq._check_against_f64(tris, rays, hits, ref, ref["stable"], what, bound=0.05 if name == "cornell" else 0.01)


# ------------------------------------------------------------------ 1, 2, 3, 5
@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("tree", TREES)
def test_refit_identity_scale_smooth_round_trip(rt, scenes, ora, name, tree):
    tris, cam = rq._scene(name, scenes)
    n = tris.shape[0]
    inp, root, count = rq._gpu_tree(rt, tris, tree)
    built = _arrays(inp, rt)
    plan = _plan(rt, inp, root, count)
    reach = _reachable(built[1], root, count)
    splits = "splits" in tree
    what = f"{name}/{tree}"

    # 1. identity
    assert _refit(rt, inp, root, count, plan, tris) == 0
    ident = _arrays(inp, rt)
    assert ident[0].tobytes() == built[0].tobytes(), f"{what}: identity changed leaf records"
    if splits:
        _check_against_reference(rt, ora, built, ident, root, count, tris, what + " identity")
    elif name == "signed_zero":
        assert _same_boxes_numerically(ident[1], built[1]), f"{what}: identity boxes differ as numbers"
    else:
        assert ident[1].tobytes() == built[1].tobytes(), f"{what}: identity changed nodes"

    # 2. scale by 2 against a GPU build of 2P
    t2 = (tris * np.float32(2)).astype(np.float32)
    assert _refit(rt, inp, root, count, plan, t2) == 0
    scaled = _arrays(inp, rt)
    assert scaled[1][~reach].tobytes() == built[1][~reach].tobytes(), f"{what}: unreachable slots were written"
    if not splits:
        b2, r2, c2 = rq._gpu_tree(rt, t2, tree)
        assert (r2, c2) == (root, count)
        bl, bn = _arrays(b2, rt)
        nrec = int(built[1]["w28"][reach & ((built[1]["w28"] >> 29) == 2)].astype(np.int64).max(initial=-1) & 0x1FFFFFFF) + 1
        assert scaled[0][:nrec].tobytes() == bl[:nrec].tobytes(), f"{what}: 2P records differ from build(2P)"
        if name == "signed_zero":
            assert _same_boxes_numerically(scaled[1][reach], bn[reach]), f"{what}: 2P boxes differ from build(2P)"
        else:
            assert scaled[1][reach].tobytes() == bn[reach].tobytes(), f"{what}: 2P slots differ from build(2P)"
    else:
        _check_against_reference(rt, ora, ident, scaled, root, count, t2, what + " 2P")

    # 3. smooth deformation
    p1 = _smooth(tris)
    assert _refit(rt, inp, root, count, plan, p1) == 0, f"{what}: a smooth deformation breaks no pair"
    moved = _arrays(inp, rt)
    _check_against_reference(rt, ora, scaled, moved, root, count, p1, what + " smooth")
    _check_trace(rt, ora, scenes, inp, root, count, moved[0], moved[1], p1, cam, what + " smooth")
    _check_rays(rt, name, (inp, root, count), p1, what + " smooth")

    # 5. back to P0: the identity refit's bytes
    assert _refit(rt, inp, root, count, plan, tris) == 0
    back = _arrays(inp, rt)
    assert back[0].tobytes() == ident[0].tobytes() and back[1].tobytes() == ident[1].tobytes(), f"{what}: round trip"
    lay = rt.refit_plan_layout(n)
    arr = _bytes(plan)[lay.arrivals:lay.arrivals + rt.NodesBytes(n) // 32]     # one byte per slot (then padding)
    assert ((arr & 0x7F) == 0).all(), f"{what}: arrival counters not back to zero"


# ------------------------------------------------------------------ 4
@pytest.mark.parametrize("name", ("grid", "soup", "cornell"))
@pytest.mark.parametrize("tree", TREES)
def test_broken_pairs(rt, scenes, ora, name, tree):
    tris, cam = rq._scene(name, scenes)
    inp, root, count = rq._gpu_tree(rt, tris, tree)
    built = _arrays(inp, rt)
    plan = _plan(rt, inp, root, count)
    p = _smooth(tris).reshape(-1, 3, 3)
    E = float(np.ptp(tris.reshape(-1, 3), axis=0).max())
    p[1::2] += (np.float32(1e-3 * E) * np.arange(1, 4, dtype=np.float32))[:, None]   # B's corners move on their own
    p = p.reshape(-1, 9).astype(np.float32)
    status = _refit(rt, inp, root, count, plan, p)
    moved = _arrays(inp, rt)
    broken = _check_against_reference(rt, ora, built, moved, root, count, p, f"{name}/{tree} broken")
    assert status == (rt.RT_REFIT_PAIR_BROKEN if broken else 0), f"{name}/{tree}: status {status}"
    if name == "grid":
        assert broken == ("pairs" in tree), "the grid's pair trees hold pairs"
    if "pairs" not in tree:
        assert not broken
        _check_trace(rt, ora, scenes, inp, root, count, moved[0], moved[1], p, cam, f"{name}/{tree} broken")
        _check_rays(rt, name, (inp, root, count), p, f"{name}/{tree} broken")


# ------------------------------------------------------------------ 6
def test_plan_misuse(rt, scenes):
    tris = scenes.grid_mesh(20, 3)
    a, ra, ca = rq._gpu_tree(rt, tris, "bottom_up")
    b, rb, cb = rq._gpu_tree(rt, _smooth(tris), "bottom_up")
    c, rc_, cc = rq._gpu_tree(rt, tris, "hybrid")
    plan = _plan(rt, a, ra, ca)
    p1 = _smooth(tris, phase=1.0)
    for inp, root, count in ((b, rb, cb), (a, ra, 1), (c, rc_, cc), (a, ra + 2, ca)):
        before = _arrays(inp, rt)
        flags = _refit(rt, inp, root, count, plan, p1)
        assert flags & rt.RT_REFIT_PLAN_MISMATCH
        after = _arrays(inp, rt)
        assert after[0].tobytes() == before[0].tobytes() and after[1].tobytes() == before[1].tobytes()
    # a tree that is not one: a run reached twice
    bad, rb2, cb2 = rq._gpu_tree(rt, tris, "bottom_up")
    nodes = _arrays(bad, rt)[1]
    box = np.nonzero((nodes["w28"][:200] >> 29) == 1)[0]
    nodes["w28"][box[1]] = nodes["w28"][box[0]]
    bad.nodes_out.copy_(rt.to_device(nodes))
    plan2 = rt.device_bytes(rt.RefitPlanBytes(bad.num_triangles))
    rt.BuildRefitPlan(bad, rb2, cb2, plan2)
    assert rt.refit_status(plan2, bad.num_triangles) & rt.RT_REFIT_BAD_TREE
    before = _arrays(bad, rt)
    assert _refit(rt, bad, rb2, cb2, plan2, p1) & rt.RT_REFIT_BAD_TREE
    after = _arrays(bad, rt)
    assert after[0].tobytes() == before[0].tobytes() and after[1].tobytes() == before[1].tobytes()


# ------------------------------------------------------------------ 7
@pytest.mark.parametrize("n", (1, 2, 3))
@pytest.mark.parametrize("tree", TREES)
def test_tiny_inputs(rt, scenes, ora, n, tree):
    tris = scenes.grid_mesh(4, 1)[:n].copy()
    inp, root, count = rq._gpu_tree(rt, tris, tree)
    built = _arrays(inp, rt)
    plan = _plan(rt, inp, root, count)
    assert _refit(rt, inp, root, count, plan, tris) == 0
    ident = _arrays(inp, rt)
    if "splits" in tree:
        _check_against_reference(rt, ora, built, ident, root, count, tris, f"n={n} {tree}")
    else:
        assert ident[0].tobytes() == built[0].tobytes() and _same_boxes_numerically(ident[1], built[1])
    p1 = _smooth(tris)
    assert _refit(rt, inp, root, count, plan, p1) == 0
    _check_against_reference(rt, ora, ident, _arrays(inp, rt), root, count, p1, f"n={n} {tree} smooth")


# ------------------------------------------------------------------ 8
def test_refit_and_queries_in_a_hip_graph(rt, scenes):
    import torch
    tris = scenes.grid_mesh(40, 3)
    inp, root, count = rq._gpu_tree(rt, tris, "sah")
    plan = _plan(rt, inp, root, count)
    rays = rt.to_device(rq._ray_sets(tris, seed=9)["outside"].astype(rt.RAY)).view(torch.float32).view(-1, 8)
    hits = torch.empty((rays.shape[0], 4), dtype=torch.float32, device="cuda")
    sets = [_smooth(tris, phase=ph) for ph in (0.0, 0.7, 1.9)]

    def frame():
        rt.Refit(inp, root, count, plan)
        rt.IntersectRays(inp.triangles_out, inp.nodes_out, root, count, rays, hits)

    eager = []
    for p in sets:
        inp.triangles_in.copy_(rt.to_device(p))
        frame()
        torch.cuda.synchronize()
        eager.append((_bytes(inp.nodes_out), _bytes(inp.triangles_out), _bytes(hits.view(torch.uint8))))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        frame()
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            frame()
    torch.cuda.current_stream().wait_stream(side)
    for p, (en, el, eh) in zip(sets, eager):
        inp.triangles_in.copy_(rt.to_device(p))
        hits.fill_(0)
        graph.replay()
        torch.cuda.synchronize()
        assert (_bytes(inp.nodes_out) == en).all() and (_bytes(inp.triangles_out) == el).all()
        assert (_bytes(hits.view(torch.uint8)) == eh).all()
    assert rt.refit_status(plan, inp.num_triangles) == 0


# ------------------------------------------------------------------ 9
@pytest.mark.parametrize("tree", ("bottom_up", "sah"))
def test_bench_mesh(rt, scenes, tree):
    tris = scenes.grid_mesh(708)
    inp, root, count = rq._gpu_tree(rt, tris, tree)
    built = _arrays(inp, rt)
    plan = _plan(rt, inp, root, count)
    reach = _reachable(built[1], root, count)
    assert _refit(rt, inp, root, count, plan, tris) == 0
    ident = _arrays(inp, rt)
    assert ident[0].tobytes() == built[0].tobytes() and ident[1].tobytes() == built[1].tobytes()
    t2 = (tris * np.float32(2)).astype(np.float32)
    assert _refit(rt, inp, root, count, plan, t2) == 0
    scaled = _arrays(inp, rt)
    b2 = rq._gpu_tree(rt, t2, tree)[0]
    bl, bn = _arrays(b2, rt)
    n = tris.shape[0]
    assert scaled[0][:n].tobytes() == bl[:n].tobytes()
    assert scaled[1][reach].tobytes() == bn[reach].tobytes()
    assert scaled[1][~reach].tobytes() == built[1][~reach].tobytes()
