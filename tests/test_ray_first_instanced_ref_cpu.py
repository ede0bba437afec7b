"""CPU tests of the instanced first-K reference (tests/ray_first_instanced_ref.py), the yardstick of
tests/test_gpu_ray_first_instanced.py, on the two scenes of tests/ray_first_instanced_scene.py built with the oracle's builders:

1. the shares the GPU test rests on: on the main scene at most ray_first_ref.CAP (2 %) of the rays with a non-empty all-hit row
   are undecided for every (TLAS kind, k); on the Cornell-twins scene the share at k = 1 is above zero, so the envelope code is
   really exercised;
2. the sequential pure-Python model of the definition (tests/ray_first_instanced_model.py) gives E on every decided ray and
   satisfies claims 1 and 3 on every ray -- in the kernel's order and in the opposite one, with and without the re-test on pop --
   on both scenes;
3. an identity placement reproduces ray_first_ref on the tree, instance 0;
4. on the main scene the rows for k >= the longest row are the sorted rows of ray_hits_instanced_ref.walk, counts included."""
import numpy as np
import pytest

import instance_ref as ir
import range_sets as rs
import ray_first_instanced_model as rfm
import ray_first_instanced_ref as rfi
import ray_first_instanced_scene as fsc
import ray_first_ref as rf
import ray_hits_instanced_ref as rhi
import wide_trees as wt

F = np.float32
BLAS_KINDS = ("bottom_up", "sah", "hybrid")      # of "grid", "soup", "cornell"
TLAS_KINDS = ("bottom_up", "sah")
KS = (1, 2, 4, 8, 32)
MODEL_KS = (1, 2, 5)
ORDERS = ((False, False), (True, False), (False, True), (True, True))     # (reverse, recull); the first is the kernel's


class Scene:
    pass


def build(ora, blas_tris, trees, inst):
    s = Scene()
    s.inst = inst
    s.prox, s.rec = fsc.host_scene(inst, trees)
    s.tlas = {kind: wt.ora_tree(ora, s.prox, kind) for kind in TLAS_KINDS}
    s.world, _, _ = ir.world_triangles(blas_tris, inst[:9])
    s.rays = fsc.scene_rays(s.world)
    s.walks = {}
    for kind, tl in s.tlas.items():
        s.walks[kind] = rfi.walk_gated(tl[1], tl[0], tl[2], tl[3], s.rec, trees, s.rays)
    return s


@pytest.fixture(scope="module")
def world(scenes, ora):
    w = Scene()
    w.blas_tris = [rs.scene_tris(name, scenes) for name in fsc.BLAS_SCENES]
    w.trees = [wt.ora_tree(ora, t, kind) for t, kind in zip(w.blas_tris, BLAS_KINDS)]
    w.trees.append((w.trees[0][0], w.trees[0][1], 0, 0))                 # table entry 3: an empty tree
    w.main = build(ora, w.blas_tris, w.trees, fsc.main_instances(w.blas_tris))
    w.twins = build(ora, w.blas_tris, w.trees, fsc.twins_instances(w.blas_tris))
    return w


# ------------------------------------------------------------------ 1: the shares
def test_main_scene_is_the_twins_scene_with_the_twins_on_the_grid(world):
    a, b = world.main.inst, world.twins.inst
    assert a.size == b.size == 12 and 1900 <= len(world.main.rays) <= 2100
    others = [k for k in range(12) if k not in fsc.TWINS]
    assert a[others].tobytes() == b[others].tobytes()
    assert a["blas"][list(fsc.TWINS)].tolist() == [0, 0] and b["blas"][list(fsc.TWINS)].tolist() == [2, 2]
    assert (a["object_to_world"][5] == a["object_to_world"][6]).all()
    assert world.main.rec["flags"].tolist() == [0] * 9 + [ir.SINGULAR, ir.BAD_BLAS, ir.BAD_BLAS]
    rows = world.main.walks["bottom_up"][0]
    assert np.unique(np.concatenate(rows)["instance"]).tolist() == list(range(9))


@pytest.mark.parametrize("kind", TLAS_KINDS)
def test_undecided_share_of_the_main_scene(world, kind):
    s = world.main
    rows, gates, _, _ = s.walks[kind]
    dd = rfi.dedup_all(rows, gates)
    assert max(len(r) for r in rows) <= 32
    for k in KS:
        share = rfi.undecided_share(rfi.expected(rows, gates, k, s.rays["tmax"], dd), rows)
        print(f"main/{kind}: k {k}: {100 * share:.3f} % of {sum(len(r) > 0 for r in rows)} rays undecided")
        assert share <= rfi.CAP, f"main/{kind}: k {k}: {100 * share:.2f} % undecided"


@pytest.mark.parametrize("kind", TLAS_KINDS)
def test_twins_scene_has_undecided_rays(world, kind):
    s = world.twins
    rows, gates, _, _ = s.walks[kind]
    share = rfi.undecided_share(rfi.expected(rows, gates, 1, s.rays["tmax"]), rows)
    print(f"twins/{kind}: k 1: {100 * share:.3f} % of {sum(len(r) > 0 for r in rows)} rays undecided")
    assert share > 0, "the Cornell twins no longer leave a ray undecided: the envelope is not exercised"


def test_walk_gated_rows_are_the_all_hit_walks(world):
    s = world.main
    tl = s.tlas["bottom_up"]
    rows, gates, box_tests, leaf_visits = s.walks["bottom_up"]
    ref_rows, bt, lv = rhi.walk(tl[1], tl[0], tl[2], tl[3], s.rec, world.trees, s.rays)
    rhi.assert_rows_equal(rows, ref_rows, "walk_gated against ray_hits_instanced_ref.walk")
    assert (box_tests, leaf_visits) == (bt, lv)
    assert all(len(g) == len(r) for g, r in zip(gates, rows))


# ------------------------------------------------------------------ 2: the model
def check_model(s, trees, kind, picks, what):
    tl = s.tlas[kind]
    rows, gates, _, _ = s.walks[kind]
    decided = undecided = 0
    for k in MODEL_KS:
        exp = rfi.expected(rows, gates, k, s.rays["tmax"])
        for reverse, recull in ORDERS:
            for i in picks:
                run = rfm.model(tl, s.rec, trees, s.rays[i], k, reverse=reverse, recull=recull)
                why = rfi.envelope_violation(run.row, rows[i], gates[i], k, s.rays["tmax"][i])
                assert why is None, f"{what}: k {k}, reverse {reverse}, recull {recull}, ray {i}: {why}"
                E, dec, _ = exp[i]
                if dec:
                    want = rfi.pad_items(k)
                    want[:len(E)] = E
                    assert run.row.tobytes() == want.tobytes(), \
                        f"{what}: k {k}, reverse {reverse}, recull {recull}, decided ray {i}: {run.row} is not E = {E}"
        decided += sum(exp[i][1] for i in picks)
        undecided += sum(not exp[i][1] for i in picks)
    return decided, undecided


def test_model_on_the_main_scene(world):
    s = world.main
    rows = s.walks["sah"][0]
    hit = [i for i in range(len(s.rays)) if len(rows[i]) > 0]
    picks = hit[::6] + [i for i in range(len(s.rays)) if len(rows[i]) == 0][:8]
    decided, _ = check_model(s, world.trees, "sah", picks, "main/sah")
    assert decided >= len(MODEL_KS) * len(picks) * 0.9
    assert max(len(rows[i]) for i in picks) >= 5, "the picked rays are not trivial"


def test_model_on_the_twins_scene(world):
    s = world.twins
    rows, gates, _, _ = s.walks["bottom_up"]
    exp = rfi.expected(rows, gates, 1, s.rays["tmax"])
    und = [i for i in range(len(s.rays)) if not exp[i][1]]
    picks = und[:24] + [i for i in range(len(s.rays)) if len(rows[i]) > 0][::40]
    decided, undecided = check_model(s, world.trees, "bottom_up", picks, "twins/bottom_up")
    assert undecided > 0 and decided > 0


def test_model_counts_are_the_walks_when_the_bound_never_moves(world):
    """claim 4's equality, one ray at a time: with k above the row's length the model examines the slots the walk examines"""
    s = world.main
    tl = s.tlas["bottom_up"]
    for i in range(0, len(s.rays), 97):
        one = s.rays[i:i + 1]
        _, _, bt, lv = rfi.walk_gated(tl[1], tl[0], tl[2], tl[3], s.rec, world.trees, one)
        run = rfm.model(tl, s.rec, world.trees, s.rays[i], 32)
        assert (run.box_tests, run.leaf_visits) == (bt, lv), f"ray {i}"
        low = rfm.model(tl, s.rec, world.trees, s.rays[i], 1)
        assert low.box_tests <= bt and low.leaf_visits <= lv


def test_the_comb_cases_of_the_gpu_test_sit_on_the_stack_edges():
    """what tests/test_gpu_ray_first_instanced_edges.py rests on, by the model alone in the shipped order, on host records:
    a comb TLAS of D pending leaves over comb BLASes of B needs D + B entries -- (60, 4) fills the stack of 64 exactly, (61, 4)
    is one push too many --, and (17, 4) enters instances at depths 15, 16 and 17, the ends of the LDS column"""
    import stack_scenes as sc
    depth, enters, rows = {}, {}, {}
    for D, B in ((17, 4), (60, 4), (61, 4)):
        case = sc.two_level_case(D, B)
        tl, b = case["tlas"], case["blas"]
        rec = sc.host_records(case["mats0"], case["blas_of"])
        trees = [(b["leaves0"], b["nodes0"], b["root"], b["count"]), (b["leaves0"], b["nodes0"], 0, 0)]
        tlas = (tl["leaves"], tl["nodes0"], tl["root"], tl["count"])
        run = rfm.model(tlas, rec, trees, case["rays"][0], 2)
        depth[D, B], enters[D, B] = run.max_depth, run.enter_depths
        cut = rfm.model(tlas, rec, trees, case["rays"][0], 2, limit=sc.STACK)
        assert cut.overflow == (D + B > sc.STACK)
        rows[D, B] = run.row, cut.row
    assert depth[60, 4] == sc.STACK and depth[61, 4] == sc.STACK + 1
    assert {sc.LDS_LEVELS - 1, sc.LDS_LEVELS, sc.LDS_LEVELS + 1} <= set(enters[17, 4])
    assert rows[60, 4][0].tobytes() == rows[60, 4][1].tobytes()


# ------------------------------------------------------------------ 3: identity
@pytest.mark.parametrize("which", (0, 1, 2))
def test_identity_placement_reproduces_the_first_k_reference(world, ora, which):
    leaves, nodes, root, count = world.trees[which]
    inst = ir.instance_array([np.eye(3, 4)], [which])
    prox, rec = fsc.host_scene(inst, world.trees)
    assert (rec["world_to_object"][0] == np.eye(3, 4, dtype=F)).all() and rec["flags"][0] == 0
    rays = rf.ray_sets(world.blas_tris[which], 11 + which, per_kind=96).astype(rf.RAY)
    for f in ("origin", "dir"):
        rays[f] = rays[f] + F(0)                      # no -0 component: the identity then reproduces every bit
    ref_rows, ref_gates, _, ref_leaf = rf.walk_gated(nodes, leaves, root, count, rays)
    tl = wt.ora_tree(ora, prox, "bottom_up")
    rows, gates, _, leaf_visits = rfi.walk_gated(tl[1], tl[0], tl[2], tl[3], rec, world.trees, rays)
    rhi.assert_rows_equal(rows, [rfi.items(0, r) for r in ref_rows], f"identity over BLAS {which}")
    assert leaf_visits == ref_leaf
    both = 0
    for k in (1, 4):
        exp, ref = rfi.expected(rows, gates, k, rays["tmax"]), rf.expected(ref_rows, ref_gates, k, rays["tmax"])
        for (E, dec, _), (RE, rdec, _) in zip(exp, ref):
            if dec and rdec:
                assert E.tobytes() == rfi.items(0, RE).tobytes()
                both += 1
    assert both > len(rays)


# ------------------------------------------------------------------ 4: k above the longest row
@pytest.mark.parametrize("kind", TLAS_KINDS)
def test_rows_at_large_k_are_the_sorted_all_hit_rows(world, kind):
    s = world.main
    tl = s.tlas[kind]
    rows, gates, _, _ = s.walks[kind]
    ref_rows, _, _ = rhi.walk(tl[1], tl[0], tl[2], tl[3], s.rec, world.trees, s.rays)
    longest = max(len(r) for r in ref_rows)
    assert 5 <= longest <= 32
    for k in (longest, 32):
        exp = rfi.expected(rows, gates, k, s.rays["tmax"])
        assert all(e[1] for e in exp), "a ray with |Ws| <= k is decided"
        out = rfi.padded(exp, k)
        for i, r in enumerate(ref_rows):
            want = rfi.pad_items(k)
            want[:len(r)] = rfi.sorted_row(r)
            assert out[i].tobytes() == want.tobytes(), f"{kind}: k {k}: ray {i}"
