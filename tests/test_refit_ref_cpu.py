"""CPU test of the numpy reference refit (tests/refit_ref.py) on the oracle's trees: LBVH, pairs, hybrid, SAH with and without
pairs and splits, on five scenes.
- identity: refitting a tree to its own triangles gives back the oracle's bytes (signed_zero: boxes equal as numbers; splits:
  the unclipped leaf boxes are held to the reference checker only);
- scale by 2: scaling every coordinate by 2 is exact in float32 and changes no build decision, so refit(tree(P), 2P) equals
  build(2P) byte for byte on the reachable slots, and the unreachable ones keep tree(P)'s bytes;
- the reference's own hierarchy checker (oracle/_ref) accepts every refitted tree."""
import importlib.util
import os

import numpy as np
import pytest

import edge_scenes
import refit_ref

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TREES = ("bottom_up", "pairs", "hybrid", "sah", "sah_pairs", "sah_splits", "sah_pairs_splits")
SCENES = ("grid", "soup", "cornell", "signed_zero", "fractal")


def _scene(name, scenes):
    if name == "grid":
        return scenes.grid_mesh(24, 5)
    if name == "soup":
        return scenes.soup(1500, 11, size=0.15)
    if name == "cornell":
        spec = importlib.util.spec_from_file_location("make_golden", os.path.join(GOLD, "make_golden.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return np.ascontiguousarray(mod.fixture_scenes()["cornell34"][0], np.float32).reshape(-1, 9)
    if name == "signed_zero":
        return edge_scenes.signed_zero_mesh(scenes)
    return scenes.fractal_corner(4000, 3)


def _tree(ora, tris, tree):
    """(leaves, nodes, root, count) of the oracle's build"""
    if tree == "bottom_up":
        o = ora.build_bvh(tris)
        return o["leaves"], o["nodes"], 0, 2
    if tree == "pairs":
        o = ora.build_pairs(tris)
        return o["leaves"], o["nodes"], 0, 2
    if tree == "hybrid":
        o = ora.build_hybrid(tris)
        return o["leaves"], o["nodes"], o["root"], 2
    o = ora.build_sah(tris, pairs="pairs" in tree, splits="splits" in tree)
    return o["leaves"], o["nodes"], 0, 1


def _reachable(nodes, root, count):
    r = np.zeros(nodes.shape[0], bool)
    for f, k, _ in refit_ref.walk(nodes, root, count):
        r[f:f + k] = True
    return r


def _words(a):
    return np.ascontiguousarray(a).view(np.uint32).reshape(a.shape[0], -1)


@pytest.fixture(scope="module")
def cache(scenes):
    return {name: _scene(name, scenes) for name in SCENES}


@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("tree", TREES)
def test_refit_reference(cache, ora, name, tree):
    tris = cache[name]
    leaves, nodes, root, count = _tree(ora, tris, tree)
    reach = _reachable(nodes, root, count)
    # identity
    l1, n1, broken = refit_ref.refit_ref(leaves, nodes, root, count, tris)
    assert not broken, "the build's own positions break no pair"
    assert l1.tobytes() == leaves.tobytes(), "identity: leaf records"
    assert (_words(n1)[:, [3, 7]] == _words(nodes)[:, [3, 7]]).all(), "w12 / w28 untouched"
    assert n1[~reach].tobytes() == nodes[~reach].tobytes(), "unreachable slots untouched"
    if "splits" not in tree:
        if name == "signed_zero":
            assert (n1["min"] == nodes["min"]).all() and (n1["max"] == nodes["max"]).all(), "identity: boxes (as numbers)"
        else:
            assert n1.tobytes() == nodes.tobytes(), "identity: nodes"
    else:
        # unclipped leaf boxes contain the build's clipped ones
        assert (n1["min"][reach] <= nodes["min"][reach]).all() and (n1["max"][reach] >= nodes["max"][reach]).all()
    # scale by 2
    t2 = (tris * np.float32(2)).astype(np.float32)
    l2, n2, broken2 = refit_ref.refit_ref(leaves, nodes, root, count, t2)
    assert not broken2
    if "splits" not in tree:
        bl, bn, broot, bcount = _tree(ora, t2, tree)
        assert (broot, bcount) == (root, count) and bn.shape == nodes.shape
        assert l2.tobytes() == bl.tobytes(), "scale by 2: leaf records equal build(2P)"
        if name == "signed_zero":
            assert (n2["min"][reach] == bn["min"][reach]).all() and (n2["max"][reach] == bn["max"][reach]).all()
        else:
            assert n2[reach].tobytes() == bn[reach].tobytes(), "scale by 2: reachable slots equal build(2P)"
        assert n2[~reach].tobytes() == nodes[~reach].tobytes()
    # the reference's own checker
    if ora.ref_available():
        for nn in (n1, n2):
            assert ora.ref_verify_hierarchy(nn, root, count) == ""
    assert ora.verify_hierarchy(n2, root, count) == 0


def test_reference_flags_a_broken_pair(ora, scenes):
    tris = scenes.grid_mesh(12, 2)
    leaves, nodes, root, count = _tree(ora, tris, "pairs")
    assert (leaves["primitive_id_1"] != 0).any()
    moved = tris.copy().reshape(-1, 3, 3)
    moved[1::2] += np.float32(0.01)          # B moves off A's edge
    _, _, broken = refit_ref.refit_ref(leaves, nodes, root, count, moved.reshape(-1, 9))
    assert broken
    _, _, broken = refit_ref.refit_ref(leaves, nodes, root, count, (tris + np.float32(0.25)).astype(np.float32))
    assert not broken, "a translation moves shared corners together"
