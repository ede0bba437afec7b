"""CPU tests of the motion query's arithmetic and of its reference (tests/motion_ref.py).
- conservativeness: on two poses of one oracle tree (tests/refit_ref.py outputs; grid / soup / cornell; LBVH, pairs, hybrid, SAH
  with and without pairs and splits), at every test time, the interpolated box of every reachable leaf slot bounds its record's
  interpolated corners and the interpolated box of every box slot bounds its children's interpolated boxes -- compared exactly
  in float32.  The interpolation is motion_ref.lerp32, the form include/rt_abi.h defines;
- the delta form a + tau * (b - a) is NOT conservative on random bounds, the defined form is;
- endpoints: lerp32 gives pose 0 at tau = 0 and pose 1 at tau = 1, as numbers;
- the unstable fraction of the GPU test's ray sets and times stays within the cap test_gpu_motion.py asserts: the cap is met
  by the inputs, not by the kernel."""
import numpy as np
import pytest

import motion_ref as mr
import refit_ref
import small_scenes as ss
from test_refit_ref_cpu import TREES, _tree

F = np.float32
MASK = 0x1FFFFFFF


@pytest.fixture(scope="module")
def cache(scenes):
    return {name: mr.poses(name, scenes) for name in mr.SCENES}


def _check_conservative(p0, p1, root, count, tau, what):
    (l0, n0), (l1, n1) = p0, p1
    lo = mr.lerp32(n0["min"], n1["min"], tau)
    hi = mr.lerp32(n0["max"], n1["max"], tau)
    typ, child, cnt = n0["w28"] >> 29, (n0["w28"] & MASK).astype(np.int64), (n0["w12"] >> 29).astype(np.int64)
    reach = np.concatenate([np.arange(f, f + k) for f, k, _ in refit_ref.walk(n0, root, count)])
    leaf = reach[typ[reach] == refit_ref.TRI]
    assert leaf.size
    rec = child[leaf]
    for v in ("v0", "v1", "v2", "v3"):     # (a single's v3 is its v2)
        c = mr.lerp32(l0[v][rec], l1[v][rec], tau)
        bad = (c < lo[leaf]) | (c > hi[leaf])
        assert not bad.any(), f"{what} tau {tau}: {bad.any(axis=1).sum()} leaf slots do not bound corner {v}"
    box = reach[typ[reach] == refit_ref.BOX]
    par = np.repeat(box, cnt[box])
    kid = np.repeat(child[box], cnt[box]) + (np.arange(cnt[box].sum()) - np.repeat(np.cumsum(cnt[box]) - cnt[box], cnt[box]))
    on = typ[kid] != refit_ref.NONE
    par, kid = par[on], kid[on]
    bad = (lo[kid] < lo[par]) | (hi[kid] > hi[par])
    assert not bad.any(), f"{what} tau {tau}: {bad.any(axis=1).sum()} box slots do not bound a child"
    return leaf.size, box.size


@pytest.mark.parametrize("name", mr.SCENES)
@pytest.mark.parametrize("tree", TREES)
def test_interpolated_boxes_bound_exactly(cache, ora, name, tree):
    tris0, tris1 = cache[name]
    leaves, nodes, root, count = _tree(ora, tris0, tree)
    # pose 0 is identity-refitted (a no-op but for split trees, whose built leaf boxes are clipped), pose 1 refitted from it
    l0, n0, b0 = refit_ref.refit_ref(leaves, nodes, root, count, tris0)
    l1, n1, b1 = refit_ref.refit_ref(l0, n0, root, count, tris1)
    assert not b0 and not b1, "a displacement that is a function of position keeps pairs whole"
    if "pairs" in tree and name == "grid":
        assert (l0["primitive_id_1"] != 0).any(), "the grid's pair trees hold pairs"
    for tau in mr.TIMES:
        _check_conservative((l0, n0), (l1, n1), root, count, tau, f"{name}/{tree}")


def test_split_tree_needs_the_identity_refit(cache, ora):
    """the header's warning: a built split tree's clipped leaf boxes, interpolated with pose 1's unclipped ones, do not bound"""
    tris0, tris1 = cache["grid"]
    leaves, nodes, root, count = _tree(ora, tris0, "sah_splits")
    l1, n1, _ = refit_ref.refit_ref(leaves, nodes, root, count, tris1)
    with pytest.raises(AssertionError):
        _check_conservative((leaves, nodes), (l1, n1), root, count, F(0.25), "unrefitted pose 0")


def test_the_delta_form_is_not_conservative():
    rng = np.random.default_rng(5)
    n = 1 << 20
    viol_def = viol_delta = 0
    for scale in (1.0, 1e3, 1e-3):
        lo0, lo1 = (rng.normal(size=n) * scale).astype(F), (rng.normal(size=n) * scale).astype(F)
        # v >= lo in both poses, by zero to two float32 steps: a corner that lies on or just inside its box
        v0, v1 = lo0.copy(), lo1.copy()
        for k in (1, 2):
            v0 = np.where(rng.integers(0, 3, n) >= k, np.nextafter(v0, F(np.inf)), v0)
            v1 = np.where(rng.integers(0, 3, n) >= k, np.nextafter(v1, F(np.inf)), v1)
        assert (v0 >= lo0).all() and (v1 >= lo1).all()
        tau = rng.random(n).astype(F)
        w0 = (F(1) - tau).astype(F)
        d_lo = ((w0 * lo0).astype(F) + (tau * lo1).astype(F)).astype(F)
        d_v = ((w0 * v0).astype(F) + (tau * v1).astype(F)).astype(F)
        viol_def += int((d_lo > d_v).sum())
        x_lo = (lo0 + (tau * (lo1 - lo0).astype(F)).astype(F)).astype(F)
        x_v = (v0 + (tau * (v1 - v0).astype(F)).astype(F)).astype(F)
        viol_delta += int((x_lo > x_v).sum())
    assert viol_def == 0, "the defined form is monotone"
    assert viol_delta > 0, "a + tau * (b - a) puts lower bounds above the values they bound"


def test_endpoints(cache):
    rng = np.random.default_rng(6)
    a = np.concatenate([cache["soup"][0].reshape(-1), (rng.normal(size=4096) * 1e4).astype(F), F([0.0, -0.0, 1e-40, -1e-40])])
    b = np.concatenate([cache["soup"][1].reshape(-1), (rng.normal(size=4096) * 1e-4).astype(F), F([-0.0, 0.0, -3.0, 1e30])])
    assert (mr.lerp32(a, b, 0.0) == a).all() and (mr.lerp32(a, b, 1.0) == b).all()
    t0, t1 = cache["cornell"]
    assert (mr.lerp_tris(t0, t1, 0.0) == t0).all() and (mr.lerp_tris(t0, t1, 1.0) == t1).all()
    h = mr.lerp32(F([1.0, 3.0]), F([2.0, 7.0]), 0.25)
    assert h.dtype == F and (h == F([1.25, 4.0])).all()


@pytest.mark.parametrize("name", mr.SCENES)
def test_unstable_fraction_of_the_gpu_tests_rays(cache, name):
    tris0, tris1 = cache[name]
    for kind, (rays, times) in mr.ray_cases(name, tris0, tris1).items():
        assert len(rays) <= 1300 and np.isin(times, mr.TIMES).all() and len(np.unique(times)) == len(mr.TIMES)
        ref, tris_all, base = mr.brute(tris0, tris1, rays, times, window=kind == "window")
        frac = 1 - ref["stable"].mean()
        print(f"{name} {kind}: unstable {100 * frac:.2f} %, hits {ref['hit'].mean():.2f}")
        assert frac <= mr.CAP[name], f"{name} {kind}: unstable fraction {frac:.4f}"
        assert ref["hit"].mean() > 0.1, "the rays meet the moving scene"


SMALL = ("n1", "n2", "n5", "twins", "n65", "stack", "giant")


@pytest.mark.parametrize("name", SMALL)
def test_unstable_fraction_of_the_small_scenes_rays(scenes, name):
    assert name not in ss.NO_F64_CAST
    tris0 = ss.tris(name, scenes)
    tris1 = mr.translated(tris0)
    rays = ss.rays(name, tris0)
    times = mr.TIMES[np.arange(len(rays)) % len(mr.TIMES)]
    ref, _, _ = mr.brute(tris0, tris1, rays, times)
    frac = 1 - ref["stable"].mean()
    print(f"{name}: unstable {100 * frac:.2f} %, hits {ref['hit'].mean():.2f}")
    assert frac <= 0.01, f"{name}: unstable fraction {frac:.4f}"
