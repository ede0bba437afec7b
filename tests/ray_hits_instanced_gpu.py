"""What tests/test_gpu_ray_hits_instanced.py and tests/test_gpu_ray_hits_instanced_edges.py share: the device calls of the
instanced all-hit queries with sentinels behind every output buffer, and a two-level scene whose bytes are read back for the
numpy walk (tests/ray_hits_instanced_ref.py).  Not a test file."""
import numpy as np

import ray_hits_instanced_ref as rhi
import ray_hits_ref as rh

SENT = 0x5EA7BEEF        # sentinel word of every output buffer
PAD = 64                 # sentinel words / records behind every output buffer


class Result:
    pass


def dev_rays(rt, rays):
    import torch
    return rt.to_device(np.ascontiguousarray(rays, rt.RAY)).view(torch.float32).view(-1, 8)


class Scene:
    """the eight arguments both calls begin with, the device buffers behind them kept alive, and the host copies the walk reads:
    tlas = (leaves, nodes, root, count) host arrays, records (host), trees[b] = (leaves, nodes, root, count) host arrays"""

    def __init__(self, rt, tlas_dev, tlas_host, records_dev, num_instances, table, num_blas, trees, keep=()):
        self.rt, self.tlas_dev, self.tlas = rt, tlas_dev, tlas_host
        self.records_dev, self.n, self.table, self.num_blas, self.trees, self.keep = records_dev, num_instances, table, num_blas, trees, keep
        self.records = rt.to_host(records_dev, rt.INSTANCE_RECORD, num_instances) if num_instances else np.zeros(0, rhi.RECORD)

    @property
    def args(self):
        leaves, nodes, root, count = self.tlas
        return (self.tlas_dev[0], self.tlas_dev[1], root, count, self.records_dev, self.n, self.table, self.num_blas)

    def walk(self, rays):
        leaves, nodes, root, count = self.tlas
        return rhi.walk(nodes, leaves, root, count, self.records, self.trees, rays)

    def entered(self, rays):
        leaves, nodes, root, count = self.tlas
        return rhi.entered(nodes, leaves, root, count, self.records, [t[3] for t in self.trees], rays)


def from_instanced(rt, sc, trees):
    """a Scene from a framed test_gpu_instances.Instanced (its TLAS and records read back) and the BLASes' host trees"""
    import torch
    torch.cuda.synchronize()
    root, count = sc.root
    n = max(sc.n, 1)
    nodes = rt.to_host(sc.tlas.nodes_out, rt.NODE)
    leaves = rt.to_host(sc.tlas.triangles_out, rt.TRIANGLE_PAIR, n)
    return Scene(rt, (sc.tlas.triangles_out, sc.tlas.nodes_out), (leaves, nodes, root, count), sc.records, sc.n, sc.table,
                 len(sc.entries), trees, keep=(sc,))


def count(rt, args, rd):
    """-> (offsets int64[n+1] numpy, counters uint64[4], status, the device offsets)"""
    import torch
    n = rd.shape[0]
    off = torch.full((n + 1 + PAD,), SENT, dtype=torch.int64, device="cuda")
    ctr = torch.zeros(4, dtype=torch.int64, device="cuda")
    ctr[2], ctr[3] = 1234, 5678                     # [2] and [3] are not touched
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert rt.RayHitsCountInstanced(*args, rd, off[:n + 1], counters=ctr, status=st) == n
    torch.cuda.synchronize()
    o, c = off.cpu().numpy(), ctr.cpu().numpy().astype(np.uint64)
    assert (o[n + 1:] == SENT).all(), "RayHitsCountInstanced wrote past offsets[n]"
    assert c[2] == 1234 and c[3] == 5678, "counters[2:4] were touched"
    return o[:n + 1], c[:2], rt.ray_hits_status(st), off


def collect(rt, args, rd, off_dev, capacity):
    """-> (ITEM records [capacity] with untouched ones left as sentinel words, counts uint32[n], counters, status)"""
    import torch
    n = rd.shape[0]
    hits = torch.full(((capacity + PAD) * 4,), SENT, dtype=torch.int32, device="cuda")
    ids = torch.full((capacity + PAD,), SENT, dtype=torch.int32, device="cuda")
    cnt = torch.full((n + PAD,), SENT, dtype=torch.int32, device="cuda")
    ctr = torch.zeros(4, dtype=torch.int64, device="cuda")
    ctr[2], ctr[3] = 1234, 5678
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert rt.RayHitsCollectInstanced(*args, rd, off_dev[:n + 1], hits, ids, counts=cnt[:n], counters=ctr, status=st) == n
    torch.cuda.synchronize()
    h, i, c = hits.cpu().numpy().view(np.uint32), ids.cpu().numpy().view(np.uint32), cnt.cpu().numpy().view(np.uint32)
    k = ctr.cpu().numpy().astype(np.uint64)
    assert (h[capacity * 4:] == SENT).all(), "RayHitsCollectInstanced wrote records past the last segment"
    assert (i[capacity:] == SENT).all(), "RayHitsCollectInstanced wrote instance ids past the last segment"
    assert (c[n:] == SENT).all(), "RayHitsCollectInstanced wrote counts past num_rays"
    assert k[2] == 1234 and k[3] == 5678, "counters[2:4] were touched"
    rec = h[:capacity * 4].view(rh.HIT)
    assert ((rec.view(np.uint32).reshape(-1, 4) != SENT).any(1) == (i[:capacity] != SENT)).all(), \
        "a record without its instance id, or the other way round"
    return rhi.items(i[:capacity], rec), c[:n], k[:2], rt.ray_hits_status(st)


def hits(rt, args, rays):
    """count, then collect into exactly offsets[n] records.  Asserts what must hold on ANY scene: offsets monotone, counts ==
    diff(offsets), every segment filled, count's and collect's counters and status equal."""
    r = Result()
    rd = dev_rays(rt, rays)
    n = len(rays)
    r.offsets, r.ctr_count, r.st_count, off = count(rt, args, rd)
    assert r.offsets[0] == 0 and (np.diff(r.offsets) >= 0).all()
    total = int(r.offsets[n])
    recs, r.counts, r.ctr_collect, r.st_collect = collect(rt, args, rd, off, total)
    assert (r.counts.astype(np.int64) == np.diff(r.offsets)).all(), "collect's counts differ from the differences of offsets"
    assert (recs["instance"] != SENT).all(), "a segment was not filled"
    assert (r.ctr_count == r.ctr_collect).all(), f"counters differ: count {r.ctr_count}, collect {r.ctr_collect}"
    assert r.st_count == r.st_collect and not (r.st_collect & rt.RT_RAY_HITS_TRUNCATED)
    r.rows = [recs[r.offsets[k]:r.offsets[k + 1]] for k in range(n)]
    return r


def check_against_walk(r, ref, what, status=0):
    ref_rows, box_tests, leaf_visits = ref
    assert r.st_count == status, f"{what}: status {r.st_count}"
    assert (r.offsets == rhi.offsets(ref_rows)).all(), f"{what}: offsets differ from the prefix sum of the walk's lengths"
    rhi.assert_rows_equal(r.rows, ref_rows, what)
    assert r.ctr_count[0] == box_tests and r.ctr_count[1] == leaf_visits, \
        f"{what}: counters {r.ctr_count}, the walk counts {box_tests}, {leaf_visits}"
