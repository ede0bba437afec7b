"""The GPU's own binned-SAH trees (RunSahBuild, and the hybrid top tree of RunBottomUpBuild) against the reference's
SharedTaskBuild run on the CPU (oracle/_ref/libref_sah.so), with no oracle in between: the node array is read back, the
reference's launches are fed from it and the two trees are compared in canonical form (tests/sah_canon.py; the rules
and the median-region exception are described there).  Block width 64 throughout: the cost is the CPU emulation."""
import numpy as np
import pytest

import sah_canon as sc
from oracle import oracle_py

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not oracle_py.ref_sah_available(),
                                 reason="oracle/_ref/libref_sah.so not built (the reference tree is not on this machine)")]

F32 = np.float32


def gpu_sah(rt, tris, pairs=False):
    import torch
    tri = np.ascontiguousarray(tris, F32).reshape(-1, 9)
    n = tri.shape[0]
    inp = rt.BuildInput.allocate(tri, sah=True)
    inp.nodes_out.fill_(0xCD)
    rt.RunSahBuild(inp, rt.Arguments(build_type=rt.kSAH, enable_pairs=pairs, enable_splits=False))
    torch.cuda.synchronize()
    lay = rt.sah_scratch_layout(n)
    status = rt.to_host(inp.scratch, np.uint32, 8, lay.status)
    assert status[0] == 0, f"build reported error flags {status[0]:#x}"
    L = int(status[1])
    return dict(L=L, nodes=rt.to_host(inp.nodes_out, rt.NODE, 128 + 2 * L),
                cells=rt.to_host(inp.scratch, np.uint32, 64, lay.cell_counts))


def test_grid60(rt, scenes):
    """block-parallel tasks of >= 32 items and their deferred small children"""
    tris = scenes.grid_mesh(60, 2)
    g = gpu_sah(rt, tris)
    st, feed, _ = sc.check_sah(g["nodes"], g["cells"], tris)
    assert feed["L"] == g["L"] == 7200
    assert st["big"] > 64 and st["small"] > 1000 and st["leaf_groups"] > 1000 and st["bit_diffs"] == []


def test_repeated_soup_median_regions(rt, scenes):
    """coincident centroids: median regions of more than 32 items (12 triangles x 50: one cell splits over two of them)"""
    tris = np.repeat(scenes.soup(12, 3, dup_fraction=0), 50, axis=0)
    g = gpu_sah(rt, tris)
    st, _, _ = sc.check_sah(g["nodes"], g["cells"], tris)
    assert st["median_big"] >= 10 and any(path != "root" for path, _ in st["median_roots"])
    tris = np.repeat(scenes.soup(6, 3, dup_fraction=0), 100, axis=0)
    g = gpu_sah(rt, tris)
    st, _, _ = sc.check_sah(g["nodes"], g["cells"], tris)
    assert st["median_big"] == 6


def test_symmetric_lattice_axis_ties(rt):
    """equal centroid extents on three axes (-> x) and on y and z (-> y), in block-parallel and in deferred tasks"""
    tris = sc.lattice(16, 16, 16)
    g = gpu_sah(rt, tris)
    st, _, _ = sc.check_sah(g["nodes"], g["cells"], tris, record_tasks=True)
    seen = set()
    for t in st["tasks"]:
        axis, tied = sc.select_axis(t["c"])
        if len(tied) < 2:
            continue
        assert axis == {(0, 1, 2): 0, (1, 2): 1}[tied]
        ctr, left = sc.centroids(t["boxes"]), t["on_left"]
        assert ctr[left][:, axis].max() < ctr[~left][:, axis].min() and t["left"] * 2 == t["n"]
        seen.add((tied, t["n"] >= sc.SMALL or t["path"] == "root"))
    assert seen == {((0, 1, 2), True), ((0, 1, 2), False), ((1, 2), True), ((1, 2), False)}
    assert st["bit_diffs"] == []


@pytest.mark.parametrize("k", [28, 56])
def test_equal_score_planes_highest_wins(k, rt):
    """seven evenly spaced columns: planes 2, 3 and 4 score the same, the sweep 6 -> 0 with strict < keeps plane 4
    (8 | 6 items); as a cell's root (28 columns) and as a child task (56)"""
    tris = sc.columns(k)
    g = gpu_sah(rt, tris)
    st, _, _ = sc.check_sah(g["nodes"], g["cells"], tris, record_tasks=True)
    tied = [t for t in st["tasks"] if t["n"] == 14]
    assert len(tied) == (4 if k == 28 else 8) and all(t["left"] == 8 for t in tied)
    assert all((t["path"] == "root") == (k == 28) for t in tied)


@pytest.mark.parametrize("shifted", [False, True])
def test_bin_constant_last_place(shifted, rt):
    """the middle column of 17 sits on the edge between bins 3 and 4: 9 | 8 columns plain, 8 | 9 shifted by 2^-21; a bin
    constant one place off exchanges them (see tests/test_ref_sah_cpu.py)"""
    tris, xs = sc.bin_edge_scene(shifted, 2)
    g = gpu_sah(rt, tris)
    st, _, _ = sc.check_sah(g["nodes"], g["cells"], tris, record_tasks=True)
    rows = [t for t in st["tasks"] if t["n"] == 17]
    assert len(rows) == 2 and all(t["left"] == (8 if shifted else 9) for t in rows)


def test_pairs(rt, scenes):
    tris = scenes.grid_mesh(16, 2)
    g = gpu_sah(rt, tris, pairs=True)
    st, feed, _ = sc.check_sah(g["nodes"], g["cells"], tris)
    assert (feed["prims"][:feed["L"], 1] == 2).sum() > 100 and g["L"] < tris.shape[0]
    assert st["big"] > 0 and st["small"] > 0 and st["bit_diffs"] == []


def test_hybrid_top_tree(rt, scenes):
    import torch
    tris = scenes.grid_mesh(24, 1)
    n = tris.shape[0]
    inp = rt.BuildInput.allocate(tris)
    inp.nodes_out.fill_(0)
    rt.RunBottomUpBuild(inp, hybrid=True)
    torch.cuda.synchronize()
    nodes = rt.to_host(inp.nodes_out, rt.NODE, 2 * n + 2 * 256 + 8)
    # the scene box the build hands to ExtractDepth, read back from the tree: the union of the LBVH's root pair
    box = np.concatenate([np.minimum(nodes["min"][0], nodes["min"][1]), np.maximum(nodes["max"][0], nodes["max"][1])])
    bits = box.astype(F32).view(np.int32)
    ordered = np.where(bits >= 0, bits, bits ^ np.int32(0x7FFFFFFF)).astype(np.int32)
    st, sub, _, _ = sc.check_hybrid(nodes, n, ordered)
    assert sub.shape[0] == 176 and st["big"] > 0 and st["small"] > 0 and st["bit_diffs"] == []
