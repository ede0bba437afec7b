"""Comparisons against the reference's own kernels run on the CPU (oracle/_ref/libref_kernels.so), shared by
tests/test_ref_kernels_cpu.py (oracle side) and tests/test_gpu_ref_kernels.py (GPU side).  Each raises AssertionError
with the first differing items."""
import numpy as np

PARENT = np.uint32(0x1FFFFFFF)


def assert_codes_equal(got, exp, what=""):
    got, exp = np.asarray(got, np.uint32), np.asarray(exp, np.uint32)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    bad = np.nonzero(got != exp)[0]
    assert bad.size == 0, f"{what}: {bad.size} codes differ, first at {bad[:6]}: {got[bad[:4]]} vs {exp[bad[:4]]}"


def assert_nodes_equal(got, exp, what=""):
    """Every Node word bit for bit; boxes by float value (-0.0 == +0.0)."""
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    for f in ("w28", "w12"):
        bad = np.nonzero(got[f] != exp[f])[0]
        assert bad.size == 0, f"{what}: Node.{f} differs at {bad[:6]} ({bad.size} slots): {got[f][bad[:4]]} vs {exp[f][bad[:4]]}"
    for f in ("min", "max"):
        bad = np.nonzero((got[f] != exp[f]).any(axis=1))[0]
        assert bad.size == 0, (f"{what}: Node.{f} differs at {bad[:6]} ({bad.size} slots): {got[f][bad[:2]].tolist()} vs "
                               f"{exp[f][bad[:2]].tolist()}")


def defined_leaf_bytes(leaves, sorted_indices):
    """The bytes of each TrianglePair that GenerateTriangles defines: v0..v3 for every leaf; primitive ids and rotations
    too for a pair (sorted value with the MSB set).  A single leaf's ids, rotations and pad3 come from an uninitialised
    local in the reference (Q1): those bytes are zeroed in the returned copy."""
    a = np.ascontiguousarray(leaves).copy()
    single = (np.asarray(sorted_indices, np.uint32) >> 31) == 0
    for f in ("primitive_id_0", "primitive_id_1", "rotations"):
        a[f][single] = 0
    a["pad3"] = 0
    return a.view(np.uint8).reshape(a.shape[0], -1)


def assert_leaves_equal(got, exp, sorted_indices, what=""):
    g, e = defined_leaf_bytes(got, sorted_indices), defined_leaf_bytes(exp, sorted_indices)
    assert g.shape == e.shape, (what, g.shape, e.shape)
    bad = np.nonzero((g != e).any(axis=1))[0]
    assert bad.size == 0, f"{what}: TrianglePair differs at {bad[:6]} ({bad.size} leaves)"


def assert_build_equal(got, ref, what=""):
    """An LBVH (oracle or GPU, dict with nodes / leaves / codes / indices) against ref_build_lbvh: exact."""
    assert_codes_equal(got["codes"], ref["codes"], what + " sorted codes")
    assert_codes_equal(got["indices"], ref["indices"], what + " sorted indices")
    assert_leaves_equal(got["leaves"], ref["leaves"], ref["indices"], what + " leaves")
    assert_nodes_equal(got["nodes"], ref["nodes"], what + " nodes")


def assert_pair_leaves_multiset_equal(got, ref, what=""):
    """Pairs path: the reference claims leaf slots in atomic arrival order, so only the multiset of leaves is its
    contract.  Leaves are keyed by their sorted value (first triangle's index, MSB = pair); per key the Morton code and
    the defined bytes of the record must be equal."""
    gi, ri = np.asarray(got["indices"], np.uint32), np.asarray(ref["indices"], np.uint32)
    assert gi.shape == ri.shape, (what, gi.shape, ri.shape)
    go, ro = np.argsort(gi, kind="stable"), np.argsort(ri, kind="stable")
    assert_codes_equal(gi[go], ri[ro], what + " leaf keys")
    assert_codes_equal(np.asarray(got["codes"])[go], np.asarray(ref["codes"])[ro], what + " leaf Morton codes")
    g = defined_leaf_bytes(np.asarray(got["leaves"])[go], gi[go])
    r = defined_leaf_bytes(np.asarray(ref["leaves"])[ro], ri[ro])
    bad = np.nonzero((g != r).any(axis=1))[0]
    assert bad.size == 0, f"{what}: leaf records differ for keys {gi[go][bad[:6]]}"


def assert_frames_equal(img, counters, ref_img, ref_counters, what=""):
    """Frame bytes exact, sum of box tests and sum of triangle tests exact."""
    diff = (img != ref_img).any(axis=-1)
    ys, xs = np.nonzero(diff)
    assert not diff.any(), (f"{what}: {int(diff.sum())} pixels differ, first (y, x) {list(zip(ys[:4], xs[:4]))}: "
                            f"{img[ys[:2], xs[:2]].tolist()} vs {ref_img[ys[:2], xs[:2]].tolist()}")
    assert int(counters[0]) == int(ref_counters[0]), f"{what}: box tests {int(counters[0])} vs {int(ref_counters[0])}"
    assert int(counters[1]) == int(ref_counters[1]), f"{what}: triangle tests {int(counters[1])} vs {int(ref_counters[1])}"


def reverse_pair_order(nodes, root, count):
    """The same tree with its sibling pairs stored in reverse order (pair p -> pair K-1-p, box children re-pointed).
    Every comparison of two box children's indices in TraceRay's tie-break (`dist == child_dist && node.child >
    child_buffer.index`) flips, nothing else changes.  Returns (nodes, root)."""
    k = nodes.shape[0] // 2
    out = nodes.reshape(k, 2)[::-1].reshape(-1).copy()
    box = (out["w28"] >> 29) == 1
    child = out["w28"] & PARENT
    out["w28"][box] = (np.uint32(1) << 29) | (2 * (k - 1 - child[box] // 2) + child[box] % 2).astype(np.uint32)
    return out, 2 * (k - 1 - root // 2) + root % 2
