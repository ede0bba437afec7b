"""What tests/test_gpu_ray_first_instanced.py and tests/test_gpu_ray_first_instanced_edges.py share: the device call of the
instanced first-K query with sentinels behind both output buffers, the reference of one (scene, ray set) computed once from the
device's own bytes (tests/ray_first_instanced_ref.py), and the check of device rows against it.  The scenes are
ray_hits_instanced_gpu.Scene objects.  Not a test file."""
import numpy as np

import ray_first_instanced_ref as rfi
import ray_hits_instanced_gpu as g
import ray_hits_ref as rh

SENT = g.SENT
PAD = g.PAD


def first(rt, args, rays, k):
    """-> (rows: ITEM [n, k], counters uint64[2], status).  Sentinels lie behind both buffers and must survive; every record
    and every id of every row must have been written; counters[2:4] are not touched."""
    import torch
    rd = g.dev_rays(rt, rays)
    n = rd.shape[0]
    hbuf = torch.full(((n * k + PAD) * 4,), SENT, dtype=torch.int32, device="cuda")
    ibuf = torch.full((n * k + PAD,), SENT, dtype=torch.int32, device="cuda")
    hits = hbuf[:n * k * 4].view(torch.float32).view(n, k, 4)
    ids = ibuf[:n * k].view(n, k)
    ctr = torch.zeros(4, dtype=torch.int64, device="cuda")
    ctr[2], ctr[3] = 1234, 5678
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert rt.RayFirstHitsInstanced(*args, rd, k, hits, ids, counters=ctr, status=st) == n
    torch.cuda.synchronize()
    h, i = hbuf.cpu().numpy().view(np.uint32), ibuf.cpu().numpy().view(np.uint32)
    assert (h[n * k * 4:] == SENT).all(), "RayFirstHitsInstanced wrote records past the last row"
    assert (i[n * k:] == SENT).all(), "RayFirstHitsInstanced wrote instance ids past the last row"
    assert (h[:n * k * 4].reshape(-1, 4) != SENT).any(1).all(), "a record of a row was not written"
    assert (i[:n * k] != SENT).all(), "an instance id of a row was not written"
    c = ctr.cpu().numpy().astype(np.uint64)
    assert c[2] == 1234 and c[3] == 5678, "counters[2:4] were touched"
    rows = rfi.items(i[:n * k], h[:n * k * 4].view(rh.HIT)).reshape(n, k)
    return rows, c[:2], rt.ray_first_status(st)


class Walk:
    """the reference of one (scene, ray set): W with gates, its counters, and Ws -- computed once, never changed"""

    def __init__(self, scene, rays):
        leaves, nodes, root, count = scene.tlas
        self.rays = rays
        self.rows, self.gates, self.box_tests, self.leaf_visits = rfi.walk_gated(nodes, leaves, root, count, scene.records,
                                                                                 scene.trees, rays)
        self.dedup = rfi.dedup_all(self.rows, self.gates)
        self.nonempty = int(sum(len(r) > 0 for r in self.rows))
        self.longest = max([len(ws) for ws, _ in self.dedup] + [0])

    def expected(self, k):
        return rfi.expected(self.rows, self.gates, k, self.rays["tmax"], dedup=self.dedup)

    def share(self, k):
        return rfi.undecided_share(self.expected(k), self.rows)


def check_rows(rows, walk, k, what):
    """the row of every decided ray is E bit for bit (20 bytes an item; on a split BLAS E is taken from Ws); claims 1 and 3 on
    every ray, decided or not.  -> number of rows that differ from E"""
    exp = walk.expected(k)
    n = len(walk.rays)
    want = rfi.padded(exp, k)
    equal = (np.ascontiguousarray(rows).view(np.uint32).reshape(n, -1) == want.view(np.uint32).reshape(n, -1)).all(1)
    decided = np.array([e[1] for e in exp], bool)
    wrong = np.nonzero(decided & ~equal)[0]
    assert len(wrong) == 0, f"{what}: k {k}: {len(wrong)} decided rays differ from E; ray {wrong[0]}: {rows[wrong[0]]} != {want[wrong[0]]}"
    for i in range(n):
        if equal[i] and decided[i] and len(walk.rows[i]) == 0:
            continue                                                     # a row of pads for an empty W: nothing to envelope
        why = rfi.envelope_violation(rows[i], walk.rows[i], walk.gates[i], k, walk.rays["tmax"][i])
        assert why is None, f"{what}: k {k}: ray {i}: {why}"
    return int((~equal).sum())


def is_sorted_subset(row, W):
    """a row of k ITEMs: live items strictly ascending by key, each an item of W bit for bit, pads behind"""
    live = row["primitive_id"] != rfi.MISS
    m = int(live.sum())
    if live[m:].any() or row[m:].tobytes() != rfi.pad_items(len(row) - m).tobytes():
        return False
    got = np.ascontiguousarray(row[:m])
    if m > 1 and not rfi.below_all(got[:-1], got[1:]).all():
        return False
    ww = np.ascontiguousarray(W).view(np.uint32).reshape(len(W), 5)
    return bool((got.view(np.uint32).reshape(m, 5)[:, None, :] == ww[None]).all(2).any(1).all())
