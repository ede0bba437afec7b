"""CPU test of the signed-distance reference (tests/sdf_ref.py) against itself: on each closed test mesh the float64 vote of the
three default directions equals an inside test that casts no ray, on every stable point -- and the stable filter keeps at least
95 % of the candidates, so the GPU tests that use these points test most of space, not a hand-picked remainder."""
import numpy as np
import pytest

import sdf_ref as sr

F = np.float32


@pytest.mark.parametrize("name", sr.MESHES)
def test_meshes_are_closed(name):
    tris = sr.mesh(name).reshape(-1, 3, 3)
    assert len(tris) == {"box": 12, "icosphere": 320, "torus": 512, "shell": 24}[name]
    # every directed edge has its opposite exactly once (bit-identical shared vertices): closed and consistently oriented
    edges = {}
    for t in tris:
        k = [v.tobytes() for v in t]
        for a, b in ((0, 1), (1, 2), (2, 0)):
            edges[k[a], k[b]] = edges.get((k[a], k[b]), 0) + 1
    assert all(n == 1 for n in edges.values()) and all((b, a) in edges for a, b in edges)
    # outward orientation: the winding number far outside is 0 and at an interior point of the solid 1
    inner = {"box": (0.0, 0.0, 0.0), "icosphere": (0.1, -0.05, 0.2), "shell": (0.5, 0.7, 0.4)}
    far = sr.winding_f64(tris, [(9.0, 8.0, 7.0)])
    assert abs(far[0]) < 1e-9
    if name in inner:
        assert abs(sr.winding_f64(tris, [inner[name]])[0] - 1) < 1e-9
    if name == "shell":
        assert abs(sr.winding_f64(tris, [(-0.05, 0.15, -0.15)])[0]) < 1e-9      # the cavity: outer + flipped inner = 0


def test_noisy_sphere_scene_is_closed(scenes):
    """the measurement scene of tools/sdf_bench.py: triangle count, bit-identical shared vertices across the cube's faces, every
    directed edge met by its opposite exactly once, outward orientation"""
    assert scenes.noisy_sphere(289).shape == (1002252, 9)
    for S in (1, 6, 7):
        tris = scenes.noisy_sphere(S, seed=3).reshape(-1, 3, 3)
        assert tris.dtype == F and len(tris) == 12 * S * S
        edges = {}
        for t in tris:
            k = [v.tobytes() for v in t]
            for a, b in ((0, 1), (1, 2), (2, 0)):
                edges[k[a], k[b]] = edges.get((k[a], k[b]), 0) + 1
        assert all(n == 1 for n in edges.values()) and all((b, a) in edges for a, b in edges)
        assert len({v.tobytes() for v in tris.reshape(-1, 3)}) == 6 * S * S + 2          # the surface lattice of the cube
        w = sr.winding_f64(tris, [(0.0, 0.0, 0.0), (0.3, -0.2, 0.1), (3.0, 3.0, 3.0)])
        assert abs(w[0] - 1) < 1e-9 and abs(w[1] - 1) < 1e-9 and abs(w[2]) < 1e-9
        r = np.linalg.norm(tris.reshape(-1, 3).astype(np.float64), axis=1)
        assert r.min() >= 1 - 1e-6 and r.max() <= 1.05 + 1e-6
    assert scenes.noisy_sphere(6).tobytes() == scenes.noisy_sphere(6).tobytes() != scenes.noisy_sphere(6, seed=2).tobytes()


@pytest.mark.parametrize("name", sr.MESHES)
def test_float64_vote_equals_the_analytic_inside(name):
    s = sr.truth_set(name)
    n = len(s["points"])
    print(f"{name}: {s['candidates']} candidates, {s['near']} within {sr.NEAR} of the surface, {n} stable "
          f"({n / s['candidates']:.4f}), inside {int(s['inside'].sum())}")
    assert n >= sr.STABLE_SHARE * s["candidates"], f"{name}: the stable filter keeps only {n} of {s['candidates']}"
    assert (sr.vote(s["counts"]) == s["inside"]).all(), f"{name}: the float64 vote itself is wrong"
    # on stable points even a single ray decides
    for j in range(3):
        assert ((s["counts"][j] % 2 == 1) == s["inside"]).all(), f"{name}: direction {j}"
    assert s["inside"].sum() >= 50 and (~s["inside"]).sum() >= 50
    assert (s["dist"] >= sr.NEAR).all()
    if name == "shell":
        cav = sr.in_cavity(s["points"])
        assert cav.sum() >= 50 and not s["inside"][cav].any() and (s["counts"][:, cav] == 2).all()
    if name == "torus":
        assert s["counts"].max() == 4                                           # genus 1: 0, 2 or 4 crossings from outside


def test_winding_agrees_with_the_boxes():
    rng = np.random.default_rng(3)
    p = rng.uniform(-1.2, 1.2, (500, 3))
    for name in ("box", "shell"):
        keep = sr.brute_f64(sr.mesh(name), p.astype(F), sr.DEFAULT_DIRS[:1])["dist"] > 1e-3
        w = sr.winding_f64(sr.mesh(name), p.astype(F)[keep])
        assert ((np.abs(w) > 0.5) == sr.analytic_inside(name, p.astype(F)[keep])).all()


@pytest.mark.parametrize("n", (600, 2048, 4096, 7))
def test_mixed_points_size(n):
    p = sr.mixed_points("torus", n)
    assert p.shape == (n, 3) and p.dtype == F


def test_lattice_layouts():
    o, s = (-1.0, 0.5, 0.25), (0.1, 0.3, 0.7)
    for dims in ((1, 1, 1), (4, 4, 4), (5, 3, 9), (17, 1, 2)):
        row = sr.lattice(o, s, dims)
        br = sr.lattice(o, s, dims, bricks=True)
        assert len(row) == dims[0] * dims[1] * dims[2]
        assert len(br) == 64 * ((dims[0] + 3) // 4) * ((dims[1] + 3) // 4) * ((dims[2] + 3) // 4)
        idx = sr.brick_index(dims)
        assert len(np.unique(idx)) == len(idx) and br[idx].tobytes() == row.tobytes()
        dead = np.ones(len(br), bool)
        dead[idx] = False
        assert (br["dist2_max"][dead] == -1).all() and (br["p"][dead] == 0).all()
    q = sr.lattice(o, s, (5, 3, 9))
    assert q["p"][(2 * 3 + 1) * 5 + 4].tolist() == [F(-1.0) + F(4) * F(0.1), F(0.5) + F(1) * F(0.3), F(0.25) + F(2) * F(0.7)]
    assert len(sr.lattice(o, s, (3, 0, 2))) == 0
