"""CPU test of the sphere-cast ABI (rt_sphere_cast): the header declares it and the library exports it, the RT_SWEEP_* values
are the header's, and every argument error is refused before any GPU work, with and without a radii array (the pointers below
are never dereferenced: a correct library returns before it touches them)."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000          # a 16-byte aligned "device pointer" that must never be used
FAKE_ODD = FAKE + 8     # 8-byte aligned only
FAKE_WORD = FAKE + 4    # 4-byte aligned only
FAKE_BYTE = FAKE + 2    # 2-byte aligned only


def _header():
    return open(os.path.join(ROOT, "include", "rt_abi.h")).read()


def test_header_declares_the_entry_point(rt):
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"\bint\s+rt_sphere_cast\s*\(", src)
    assert re.search(r"enum\s*\{\s*RT_SWEEP_NONE\s*=\s*0\s*,\s*RT_SWEEP_FACE\s*=\s*1\s*,\s*RT_SWEEP_EDGE\s*=\s*2\s*,\s*"
                     r"RT_SWEEP_CORNER\s*=\s*3\s*,\s*RT_SWEEP_OVERLAP\s*=\s*4\s*\}", src)
    assert "rt_sphere_cast" in rt.EXPORTS
    assert rt.lib().rt_sphere_cast is not None
    assert "spherecast:" in rt.version()
    assert (rt.RT_SWEEP_NONE, rt.RT_SWEEP_FACE, rt.RT_SWEEP_EDGE, rt.RT_SWEEP_CORNER, rt.RT_SWEEP_OVERLAP) == (0, 1, 2, 3, 4)
    # the block sits after the capsule block and says what it must
    h = _header()
    assert h.index("---- capsule primitives") < h.index("---- sphere cast") < h.index("---- mixed instancing")
    block = h[h.index("---- sphere cast"):h.index("enum { RT_SWEEP_NONE")]
    for words in ("Minkowski", "radii == NULL", "NOT TRACED", "2^-18", "root run", "growth exactly 0", "clipped box",
                  "closest-point block", "rt_range_count", "bit for bit", "byte for byte", "n = e1 x e2", "!(len > 0)",
                  "no far root is ever taken", "tau1", "shared edge v1-v2 is tested TWICE", "the later wins", "RT_SWEEP_CORNER",
                  "(o + t*d - contact) / rad", "hipGraph", "Out of scope", "swept capsules or boxes", "first-K",
                  "sphere or capsule", "rt_cli"):
        assert words in block, words


def _accel(rt, count=2, triangles=FAKE, nodes=FAKE):
    return ctypes.byref(rt._Accel(triangles, nodes, 0, count))


@pytest.mark.parametrize("with_radii", (False, True))
def test_argument_errors(rt, with_radii):
    q = rt.lib().rt_sphere_cast

    def args(**kw):
        #        as, rays, radii, radius, num_rays, order, num_indices, hits, features, mode, counters, stream
        a = dict(tree=_accel(rt), rays=FAKE, radii=FAKE_WORD if with_radii else None, radius=0.5, num_rays=5, order=None,
                 num_indices=0, hits=FAKE, features=FAKE_WORD, mode=0, counters=None, stream=None)
        a.update(kw)
        return list(a.values())

    for null in ("tree", "rays", "hits"):                                            # null with a non-zero count
        assert q(*args(**{null: None})) == -1, null
    assert q(*args(tree=_accel(rt, count=8))) == -1                                  # count > 7
    for field in ("triangles", "nodes"):                                             # a null tree pointer with count > 0
        assert q(*args(tree=_accel(rt, **{field: 0}))) == -1, field
    for name, bad in (("rays", FAKE_ODD), ("hits", FAKE_ODD), ("order", FAKE_BYTE), ("radii", FAKE_BYTE),
                      ("features", FAKE_BYTE)):
        assert q(*args(**{name: bad})) == -1, name
        assert q(*args(**{name: bad}, num_rays=0)) == -1, name                       # errors win over an empty batch
    assert q(*args(order=FAKE_BYTE, num_indices=4)) == -1
    for mode in (-1, 2, 7):
        assert q(*args(mode=mode)) == -1
        assert q(*args(mode=mode, num_rays=0)) == -1
    assert q(*args(tree=None, num_rays=0)) == -1
    assert q(*args(tree=_accel(rt, count=8), num_rays=0)) == -1
    # the one radius of a call without radii must be finite and not negative; with radii it is not read
    for bad in (-1.0, -1e-30, float("nan"), float("inf"), float("-inf")):
        if with_radii:
            assert q(*args(radius=bad, num_rays=0)) == 0, bad
        else:
            assert q(*args(radius=bad)) == -1, bad
            assert q(*args(radius=bad, num_rays=0)) == -1, bad                       # wins over an empty batch
    for ok in (0.0, 1e-30, 3e38):
        assert q(*args(radius=ok, num_rays=0)) == 0
    # zero counts run nothing: no rays, or an index list without an entry
    assert q(*args(num_rays=0)) == 0
    assert q(*args(num_rays=0, rays=None, hits=None, features=None, mode=1, counters=FAKE)) == 0
    assert q(*args(order=FAKE_WORD, num_indices=0)) == 0
    assert q(*args(num_rays=0, order=FAKE_WORD, num_indices=9)) == 0
    assert q(*args(num_rays=0, tree=_accel(rt, count=0, triangles=0, nodes=0))) == 0


def test_python_wrapper_refuses_bad_buffers(rt):
    import torch
    rays = torch.zeros((4, 8), dtype=torch.float32)
    hits = torch.zeros((4, 4), dtype=torch.float32)
    radii = torch.zeros(4, dtype=torch.float32)
    feats = torch.zeros(4, dtype=torch.int32)
    order = torch.zeros(4, dtype=torch.int32)
    tree = (torch.zeros(64, dtype=torch.uint8), torch.zeros(64, dtype=torch.uint8))

    def cast(**kw):
        a = dict(rays=rays, hits=hits, radii=radii, radius=0.0, features=feats, order=None, num_indices=None)
        a.update(kw)
        rt.SphereCast(tree[0], tree[1], 0, 2, a["rays"], a["hits"], radii=a["radii"], radius=a["radius"], features=a["features"],
                      order=a["order"], num_indices=a["num_indices"])

    for bad in (dict(hits=hits[:3]), dict(hits=torch.zeros((4, 8))[:, ::2]), dict(rays=torch.zeros((4, 16))[:, ::2]),
                dict(rays=torch.zeros(33, dtype=torch.uint8)), dict(radii=radii[:3]), dict(radii=torch.zeros(8)[::2]),
                dict(radii=torch.zeros(4, dtype=torch.float64)), dict(radii=torch.zeros(4, dtype=torch.int32)),
                dict(features=feats[:3]), dict(features=torch.zeros(8, dtype=torch.int32)[::2]),
                dict(features=torch.zeros(4, dtype=torch.uint8)), dict(order=order, num_indices=5),
                dict(order=torch.zeros(8, dtype=torch.int32)[::2]),
                dict(radii=None, radius=-1.0), dict(radii=None, radius=float("nan")), dict(radii=None, radius=float("inf"))):
        with pytest.raises(ValueError):
            cast(**bad)
    # an empty batch and an empty index list run nothing (no device is touched)
    rt.SphereCast(tree[0], tree[1], 0, 2, rays[:0], hits[:0], radius=1.0)
    cast(order=order, num_indices=0)


def test_the_constants_are_the_reference_modules(rt):
    import sphere_cast_ref as sc
    assert sc.RAY == rt.RAY and sc.HIT == rt.HIT and sc.MISS == rt.MISS
    assert (sc.NONE, sc.FACE, sc.EDGE, sc.CORNER, sc.OVERLAP) == (rt.RT_SWEEP_NONE, rt.RT_SWEEP_FACE, rt.RT_SWEEP_EDGE,
                                                                  rt.RT_SWEEP_CORNER, rt.RT_SWEEP_OVERLAP)
    assert sc.scene("sheet").shape == (2 * 24 * 24, 9) and sc.scene("soup").shape == (1500, 9)
    far = sc.scene("far").reshape(-1, 3, 3)
    assert (far[::10, 1] == far[::10, 2]).all() and far.shape[0] == 800
    rays, radii = sc.make_rays(sc.scene("soup"), sc.SEEDS[0])
    assert rays.shape == (sc.NUM_RAYS,) and radii.dtype == np.float32 and (radii[::8] == 0).all() and (radii[1::8] > 0).all()
    assert 0.45 <= np.isfinite(rays["tmax"]).mean() <= 0.55
