"""CPU test of the ray-sort ABI (rt_ray_sort_scratch_bytes, rt_ray_sort_layout_get, rt_sort_rays, rt_intersect_rays_indexed):
the header declares the four, the Python binding lists them, the scratch layout is consistent, every argument error is refused
before any GPU work (the pointers below are never dereferenced: a correct library returns before it touches them), and the
numpy restatement of the key (tests/ray_sort_ref.py) has the properties the header promises."""
import ctypes
import os
import re

import numpy as np

import ray_sort_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000          # a 256-byte aligned "device pointer" that must never be used
FAKE_8 = FAKE + 8       # 8-byte aligned only
FAKE_2 = FAKE + 2       # 2-byte aligned only
FAKE_16 = FAKE + 16     # 16- but not 256-byte aligned
RAY = np.dtype([("origin", "<f4", 3), ("tmin", "<f4"), ("dir", "<f4", 3), ("tmax", "<f4")])
NAMES = ("rt_ray_sort_scratch_bytes", "rt_ray_sort_layout_get", "rt_sort_rays", "rt_intersect_rays_indexed")


def test_header_declares_the_ray_sort_entry_points(rt):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rt_abi.h")).read(), flags=re.S)
    assert re.search(r"\bsize_t\s+rt_ray_sort_scratch_bytes\s*\(", src)
    for name in NAMES[1:]:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
    assert re.search(r"#define\s+RT_RAY_KEY_DEAD\s+\(1u << 29\)", src) and re.search(r"#define\s+RT_RAY_KEY_BITS\s+30\b", src)
    for name in NAMES:
        assert name in rt.EXPORTS and getattr(rt.lib(), name) is not None, name
    assert rt.RAY_KEY_DEAD == int(ray_sort_ref.DEAD) == 1 << 29 and rt.RAY_KEY_BITS == ray_sort_ref.KEY_BITS == 30
    assert "raysort:" in rt.version()


def test_scratch_layout(rt):
    sizes = []
    for n in (0, 1, 63, 64, 65, 257, 4096, 4097, 1 << 20, 1920 * 1080, 5_000_000, 0x3FFFFFFF):
        lay = rt.ray_sort_layout(n)
        offs = [lay.box, lay.keys, lay.tmp_keys, lay.tmp_values, lay.sort, lay.total]
        assert all(o % 256 == 0 for o in offs), (n, offs)
        assert offs == sorted(offs) and lay.box == 0 and lay.keys == 256
        assert lay.box < lay.num_live < 256 and lay.num_live % 4 == 0 and lay.num_live >= 32   # inside the header, after the box
        m = max(n, 1)
        assert lay.tmp_keys - lay.keys >= 4 * m and lay.tmp_values - lay.tmp_keys >= 4 * m and lay.sort - lay.tmp_values >= 4 * m
        assert lay.total - lay.sort >= rt.RadixSortScratchBytes(n)
        assert lay.total == rt.RaySortScratchBytes(n)
        sizes.append(lay.total)
    assert sizes == sorted(sizes), "the scratch size is monotone in num_rays"
    assert rt.lib().rt_ray_sort_layout_get(100, None) == -1


def _accel(rt, count=2, nodes=FAKE, triangles=FAKE):
    return ctypes.byref(rt._Accel(triangles, nodes, 0, count))


def test_sort_rays_argument_errors(rt):
    L = rt.lib()
    A = _accel(rt)
    assert L.rt_sort_rays(None, FAKE, 5, FAKE, FAKE, None) == -1                     # no accel
    assert L.rt_sort_rays(A, None, 5, FAKE, FAKE, None) == -1                        # no rays
    assert L.rt_sort_rays(A, FAKE, 5, None, FAKE, None) == -1                        # no order
    assert L.rt_sort_rays(A, FAKE, 5, FAKE, None, None) == -1                        # no scratch
    assert L.rt_sort_rays(A, FAKE_8, 5, FAKE, FAKE, None) == -1                      # rays not 16-byte aligned
    assert L.rt_sort_rays(A, FAKE, 5, FAKE_2, FAKE, None) == -1                      # order not 4-byte aligned
    assert L.rt_sort_rays(A, FAKE, 5, FAKE, FAKE_16, None) == -1                     # scratch not 256-byte aligned
    assert L.rt_sort_rays(_accel(rt, count=8), FAKE, 5, FAKE, FAKE, None) == -1      # count > 7
    assert L.rt_sort_rays(_accel(rt, nodes=0), FAKE, 5, FAKE, FAKE, None) == -1      # a tree without nodes
    assert L.rt_sort_rays(A, FAKE, 0x40000000, FAKE, FAKE, None) == -3               # beyond the sort's limit
    assert L.rt_sort_rays(A, FAKE, 0xFFFFFFFF, FAKE, FAKE, None) == -3
    # errors win over an empty batch; an empty batch with valid arguments does nothing
    assert L.rt_sort_rays(_accel(rt, count=8), FAKE, 0, FAKE, FAKE, None) == -1
    assert L.rt_sort_rays(A, FAKE, 0, FAKE_2, FAKE, None) == -1
    assert L.rt_sort_rays(A, FAKE, 0, FAKE, FAKE, None) == 0
    assert L.rt_sort_rays(_accel(rt, count=0, nodes=0, triangles=0), FAKE, 0, FAKE + 4, FAKE, None) == 0   # an empty tree is fine
    assert L.rt_sort_rays(_accel(rt, triangles=0), FAKE, 0, FAKE, FAKE, None) == 0    # the leaves are never read


def test_intersect_rays_indexed_argument_errors(rt):
    L = rt.lib()
    A = _accel(rt)
    f = L.rt_intersect_rays_indexed       # (as, rays, num_rays, order, num_indices, hits, mode, num_primitives, counters, stream)
    assert f(None, FAKE, 5, FAKE, 5, FAKE, 0, 0, None, None) == -1
    assert f(A, None, 5, FAKE, 5, FAKE, 0, 0, None, None) == -1
    assert f(A, FAKE, 5, None, 5, FAKE, 0, 0, None, None) == -1                      # no order
    assert f(A, FAKE, 5, FAKE, 5, None, 0, 0, None, None) == -1
    assert f(_accel(rt, nodes=0), FAKE, 5, FAKE, 5, FAKE, 0, 0, None, None) == -1
    assert f(_accel(rt, triangles=0), FAKE, 5, FAKE, 5, FAKE, 0, 0, None, None) == -1
    assert f(_accel(rt, count=8), FAKE, 5, FAKE, 5, FAKE, 0, 0, None, None) == -1
    for mode in (-1, 2, 7):
        assert f(A, FAKE, 5, FAKE, 5, FAKE, mode, 0, None, None) == -1
    assert f(A, FAKE_8, 5, FAKE, 5, FAKE, 0, 0, None, None) == -1                    # rays not 16-byte aligned
    assert f(A, FAKE, 5, FAKE, 5, FAKE_8, 0, 0, None, None) == -1                    # hits not 16-byte aligned
    assert f(A, FAKE, 5, FAKE_2, 5, FAKE, 0, 0, None, None) == -1                    # order not 4-byte aligned
    # errors win over an empty list; an empty list with valid arguments does nothing (whatever num_rays is)
    assert f(_accel(rt, count=8), FAKE, 5, FAKE, 0, FAKE, 0, 0, None, None) == -1
    assert f(A, FAKE, 5, FAKE_2, 0, FAKE, 0, 0, None, None) == -1
    assert f(A, FAKE, 5, FAKE + 4, 0, FAKE, 0, 0, None, None) == 0
    assert f(A, FAKE, 0, FAKE, 0, FAKE, 1, 10_000_000, FAKE, None) == 0


# ------------------------------------------------------------------ the reference's own properties
def _fuzz(n, seed):
    rng = np.random.default_rng(seed)
    r = np.zeros(n, RAY)
    r["origin"] = rng.uniform(-3, 3, (n, 3))
    r["dir"] = rng.normal(size=(n, 3))
    r["tmin"], r["tmax"] = 0.0, np.inf
    k = n // 8
    r["origin"][:k] = rng.choice(np.array([np.inf, -np.inf, 1e30, -1e30, 0.0, 1.0, -1.0], np.float32), (k, 3))
    r["dir"][k:2 * k] = rng.choice(np.array([0.0, -0.0, 1e-42, -1e-42, 1.0, np.inf], np.float32), (k, 3))
    r["tmax"][2 * k:3 * k] = -1.0                    # dead: empty range
    r["tmin"][3 * k:3 * k + 5] = np.nan              # dead: NaN
    r["origin"][3 * k + 5:3 * k + 10, 1] = np.nan
    r["dir"][3 * k + 10:3 * k + 15, 2] = np.nan
    r["tmax"][3 * k + 15:3 * k + 20] = np.nan
    return r, slice(2 * k, 3 * k + 20)


def test_reference_key_properties():
    rays, dead = _fuzz(4000, 7)
    lo, hi = np.float32([-1, -1, -1]), np.float32([1, 2, 1])
    alive = ray_sort_ref.live(rays)
    assert not alive[dead].any() and alive[:dead.start].all() and alive[dead.stop:].all()
    for box in ((lo, hi), (lo, lo), (np.zeros(3, np.float32), np.zeros(3, np.float32)),     # a box, a point, the empty tree's
                (np.float32([-np.inf, 0, 0]), np.float32([np.inf, 0, 1])),                  # an infinite axis, a flat one
                (np.float32([np.nan, 0, 0]), np.float32([1, np.nan, 1]))):
        k = ray_sort_ref.keys(rays, *box)
        assert k.dtype == np.uint32 and (k < (1 << ray_sort_ref.KEY_BITS)).all(), "the key fits 30 bits"
        assert (k[~alive] == ray_sort_ref.DEAD).all() and (k[alive] < ray_sort_ref.DEAD).all(), "dead keys above every live key"
        assert (k[alive] < (1 << 27)).all()
    # origins clamp to the border cells
    far = np.zeros(2, rays.dtype)
    far["origin"][0], far["origin"][1], far["dir"][:] = -np.inf, np.inf, 1.0
    oc, dc = ray_sort_ref.cells(far, lo, hi)
    assert (oc[0] == 0).all() and (oc[1] == 127).all() and (dc == 3).all()
    zero = np.zeros(1, rays.dtype)                                 # a zero direction: 0 / 0 -> cell 0
    assert (ray_sort_ref.cells(zero, lo, hi)[1] == 0).all()
    # the direction's length does not matter: scaling by a positive power of two leaves the key alone
    sel = alive & np.isfinite(rays["dir"]).all(axis=1) & ((np.abs(rays["dir"]) > 1e-20) | (rays["dir"] == 0)).all(axis=1)
    base = ray_sort_ref.keys(rays[sel], lo, hi)
    for s in (2.0 ** -40, 0.5, 2.0, 2.0 ** 60):
        scaled = rays[sel].copy()
        scaled["dir"] = scaled["dir"] * np.float32(s)
        assert np.isfinite(scaled["dir"]).all()
        assert (ray_sort_ref.keys(scaled, lo, hi) == base).all(), f"key changed under scaling by {s}"
    # stable order: ties by index, dead rays last in index order
    nodes = np.zeros(2, np.dtype([("min", "<f4", 3), ("w12", "<u4"), ("max", "<f4", 3), ("w28", "<u4")]))
    nodes["min"], nodes["max"], nodes["w28"] = [[-1, -1, -1], [0, 0, 0]], [[0.5, 2, 1], [1, 1, 1]], [1 << 29, 0]
    out = ray_sort_ref.sort(rays, nodes, 0, 2)
    assert (out["box"][0] == [-1, -1, -1]).all() and (out["box"][1] == [0.5, 2, 1]).all(), "NONE slots do not count"
    assert out["num_live"] == int(alive.sum())
    assert (out["order"][out["num_live"]:] == np.nonzero(~alive)[0]).all()
    ks = out["keys"][out["order"]]
    assert (np.diff(ks.astype(np.int64)) >= 0).all()
    same = np.diff(ks.astype(np.int64)) == 0
    assert (np.diff(out["order"].astype(np.int64))[same] > 0).all()
    assert ray_sort_ref.root_box(nodes, 0, 0)[0].tolist() == [0, 0, 0]
