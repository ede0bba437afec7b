"""GPU tests of the instanced first-K ray query on the trees where a traversal goes wrong first (the call and its sentinels:
tests/ray_first_instanced_gpu.py; the reference: tests/ray_first_instanced_ref.py on the bytes the device reads).

1. stack edges: stack_scenes.two_level_case -- a comb TLAS of D pending instance leaves over comb BLASes of B pending leaves.
   Every box holds every ray's origin, so every front is negative: no bound ever prunes a slot, ties send the lower slot first
   and the other to the stack, and one stack of 64 serves both levels.  The depths are not assumed: the sequential model
   (tests/ray_first_instanced_model.py) is run in the shipped order on the device's records and says how deep the stack gets
   and at which depths instances are entered.  The largest D + B that fits gives status 0 and rows equal to E; one beyond gives
   RT_RAY_FIRST_STACK_OVERFLOW and rows that are sorted subsets of W; instances are entered at depths 15, 16 and 17, the ends of
   the LDS column;
2. tiny trees: BLASes of one to five triangles and the degenerate scenes flat / points / giant under TLASes of one to five
   instances;
3. wide trees: wide_trees.repack (runs of 1..7 slots, NONE slots first, in the middle and last) on the BLASes, on the TLAS, and
   on both."""
import numpy as np
import pytest

import instance_ref as ir
import ray_first_instanced_gpu as fg
import ray_first_instanced_model as rfm
import ray_first_instanced_ref as rfi
import ray_hits_instanced_gpu as g
import small_scenes as ss
import stack_scenes as sc
import test_gpu_instances as tgi
import test_gpu_ray_hits_instanced_edges as hie
import test_gpu_stack_depths as tsd
from test_gpu_ray_queries import _gpu_tree

pytestmark = pytest.mark.gpu

F = np.float32
STACK_CASES = ((12, 8), (15, 1), (16, 4), (17, 4), (60, 4), (61, 4), (70, 8))
KS = (1, 3)


# ------------------------------------------------------------------ 1: stack edges
def _comb_scene(rt, case):
    tl, b = case["tlas"], case["blas"]
    D = case["D"]
    blas_dev = rt.to_device(b["leaves0"]), rt.to_device(b["nodes0"])
    entries = [(blas_dev[0], blas_dev[1], b["root"], b["count"]), (blas_dev[0], blas_dev[1], 0, 0)]
    inst = tgi.Instanced(rt, entries, ir.instance_array(case["mats0"], case["blas_of"]))
    inst.prepare()                                               # the records; the TLAS is the hand-made comb
    tlas_dev = rt.to_device(tl["leaves"]), rt.to_device(tl["nodes0"])
    trees = [(b["leaves0"], b["nodes0"], b["root"], b["count"]), (b["leaves0"], b["nodes0"], 0, 0)]
    return g.Scene(rt, tlas_dev, (tl["leaves"], tl["nodes0"], tl["root"], tl["count"]), inst.records, D + 1, inst.table, 2, trees,
                   keep=(inst, blas_dev))


@pytest.mark.parametrize("D,B", STACK_CASES)
def test_two_level_combs(rt, D, B):
    case = sc.two_level_case(D, B)
    s = _comb_scene(rt, case)
    rays = case["rays"].astype(rt.RAY)
    what = f"comb ({D}, {B})"
    # what the definition, walked in the shipped order without a limit, needs: the same for every ray of a comb
    need = [rfm.model(s.tlas, s.records, s.trees, rays[i], 1) for i in (0, len(rays) - 1)]
    assert need[0].max_depth == need[1].max_depth == D + B, f"{what}: the model needs {need[0].max_depth} entries"
    fits = need[0].max_depth <= sc.STACK
    walk = fg.Walk(s, rays)
    assert sum(len(x) for x in walk.rows) > len(rays)
    for k in KS:
        rows, ctr, status = fg.first(rt, s.args, rays, k)
        if fits:
            assert status == 0, f"{what}: k {k}: status {status}"
            assert all(e[1] for e in walk.expected(k)), "every front of a comb is negative: every ray is decided"
            assert fg.check_rows(rows, walk, k, what) == 0
            assert ctr[0] == walk.box_tests and ctr[1] == walk.leaf_visits, "no bound prunes a comb"
            continue
        assert status == rt.RT_RAY_FIRST_STACK_OVERFLOW, f"{what}: k {k}: status {status}"
        for i in range(len(rays)):
            assert fg.is_sorted_subset(rows[i], walk.rows[i]), f"{what}: k {k}: ray {i}: not a sorted subset of W"
        assert ctr[0] < walk.box_tests and ctr[1] < walk.leaf_visits, "dropped pushes are subtrees that were not visited"
        # the model with the kernel's 64 entries drops the same pushes: the same rows
        for i in (0, len(rays) - 1):
            run = rfm.model(s.tlas, s.records, s.trees, rays[i], k, limit=sc.STACK)
            assert run.overflow and run.row.tobytes() == rows[i].tobytes(), f"{what}: k {k}: ray {i}: {rows[i]} != the model's {run.row}"


# ------------------------------------------------------------------ 2: tiny trees
@pytest.mark.parametrize("name", ss.TINY[:5] + ("flat", "points", "giant"))
def test_tiny_blases_under_tiny_tlases(rt, scenes, name):
    tris = np.array(ss.tris(name, scenes))
    ext = float(np.ptp(tris.reshape(-1, 3), axis=0).max())
    src = ss.all_rays(name, tris).astype(rt.RAY)
    seen = 0
    for K in (1, 2, 3, 4, 5):
        blas_kind = ("bottom_up", "sah_pairs", "sah")[K % 3]
        tlas_kind = tgi.TLAS_KINDS[K % 3]
        inp, root, count = _gpu_tree(rt, tris, blas_kind)
        leaves, nodes = tsd._host_tree(rt, inp)
        mats = hie._spread(K, ext, seed=100 + K)
        inst = tgi.Instanced(rt, [(inp.triangles_out, inp.nodes_out, root, count)], ir.instance_array(mats, [0] * K), tlas_kind)
        inst.frame()
        assert rt.instance_status(inst.status) == 0
        s = g.from_instanced(rt, inst, [(leaves, nodes, root, count)])
        rays = sc.through_instances(src[K % 2::2], mats).astype(rt.RAY)      # every object ray, seen through every instance
        walk = fg.Walk(s, rays)
        for k in (1, 2, 32):
            rows, ctr, status = fg.first(rt, s.args, rays, k)
            assert status == 0
            fg.check_rows(rows, walk, k, f"{name}: {K} instances, BLAS {blas_kind}, TLAS {tlas_kind}")
            assert ctr[0] <= walk.box_tests and ctr[1] <= walk.leaf_visits
            live = rows["primitive_id"] != rfi.MISS
            assert not live.any() or rows["instance"][live].max() < K
            seen += int(live.sum())
    assert seen > 0 or name == "points", f"{name}: no ray crossed anything"


# ------------------------------------------------------------------ 3: wide trees
@pytest.fixture(scope="module")
def wide(rt, scenes):
    return hie._Wide(rt, scenes)


@pytest.mark.parametrize("tlas_kind", ("bottom_up", "sah"))
@pytest.mark.parametrize("wide_blas,wide_tlas", ((True, False), (False, True), (True, True)))
def test_wide_trees(wide, wide_blas, wide_tlas, tlas_kind):
    s = wide.scene(wide_blas, wide_tlas, tlas_kind)
    walk = fg.Walk(s, wide.rays)
    what = f"wide BLAS {wide_blas}, wide TLAS {wide_tlas}, TLAS {tlas_kind}"
    assert walk.nonempty > len(wide.rays) // 4 and walk.longest >= 4
    for k in (1, 4):
        rows, ctr, status = fg.first(wide.rt, s.args, wide.rays, k)
        assert status == 0
        differ = fg.check_rows(rows, walk, k, what)
        assert ctr[0] <= walk.box_tests and ctr[1] <= walk.leaf_visits
        print(f"{what}: k {k}: {100 * walk.share(k):.3f} % undecided, {differ} rows differ from E")
    rows, _, _ = fg.first(wide.rt, s.args, wide.rays, 4)
    assert len(np.unique(rows["instance"][rows["primitive_id"] != rfi.MISS])) >= 20
