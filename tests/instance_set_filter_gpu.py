"""What the GPU tests of the filtered instanced all-hit and first-K queries share: the device calls with sentinels behind every
output buffer (tests/ray_hits_instanced_gpu.py's and tests/ray_first_instanced_gpu.py's, with a filter), and the reference of
one (scene, ray set, filter) computed once from the device's own bytes (tests/instance_set_filter_ref.py).  The scenes are
ray_hits_instanced_gpu.Scene objects.  Not a test file."""
import numpy as np

import instance_set_filter_ref as isf
import ray_first_instanced_ref as rfi
import ray_hits_instanced_gpu as g
import ray_hits_instanced_ref as rhi
import ray_hits_ref as rh

SENT = g.SENT
PAD = g.PAD
UNFILTERED = "unfiltered"        # the unfiltered sibling (a None filter is the filtered entry point with filter = NULL)


def dev_filter(rt, flt):
    """instance_filter_ref.InstanceFilter (host arrays) -> rt.InstanceHitFilter (device arrays); None stays None"""
    import torch
    if flt is None:
        return None
    pi = None if flt.per_instance is None else rt.to_device(flt.per_instance).view(torch.int32).view(-1, 2)
    pr = None if flt.per_ray is None else rt.to_device(flt.per_ray).view(torch.int32).view(-1, 4)
    return rt.InstanceHitFilter(flt.flags, flt.ray_mask, pi, pr)


def count(rt, args, rd, hf):
    """-> (offsets int64[n+1] numpy, counters uint64[2], status, the device offsets)"""
    import torch
    n = rd.shape[0]
    off = torch.full((n + 1 + PAD,), SENT, dtype=torch.int64, device="cuda")
    ctr = torch.zeros(4, dtype=torch.int64, device="cuda")
    ctr[2], ctr[3] = 1234, 5678                     # [2] and [3] are not touched
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    if hf is UNFILTERED:
        assert rt.RayHitsCountInstanced(*args, rd, off[:n + 1], counters=ctr, status=st) == n
    else:
        assert rt.RayHitsCountInstancedFiltered(*args, rd, hf, off[:n + 1], counters=ctr, status=st) == n
    torch.cuda.synchronize()
    o, c = off.cpu().numpy(), ctr.cpu().numpy().astype(np.uint64)
    assert (o[n + 1:] == SENT).all(), "the count call wrote past offsets[n]"
    assert c[2] == 1234 and c[3] == 5678, "counters[2:4] were touched"
    return o[:n + 1], c[:2], rt.ray_hits_status(st), off


def collect(rt, args, rd, hf, off_dev, capacity):
    """-> (ITEM records [capacity] with untouched ones left as sentinel words, counts uint32[n], counters, status)"""
    import torch
    n = rd.shape[0]
    hits = torch.full(((capacity + PAD) * 4,), SENT, dtype=torch.int32, device="cuda")
    ids = torch.full((capacity + PAD,), SENT, dtype=torch.int32, device="cuda")
    cnt = torch.full((n + PAD,), SENT, dtype=torch.int32, device="cuda")
    ctr = torch.zeros(4, dtype=torch.int64, device="cuda")
    ctr[2], ctr[3] = 1234, 5678
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    if hf is UNFILTERED:
        assert rt.RayHitsCollectInstanced(*args, rd, off_dev[:n + 1], hits, ids, counts=cnt[:n], counters=ctr, status=st) == n
    else:
        assert rt.RayHitsCollectInstancedFiltered(*args, rd, hf, off_dev[:n + 1], hits, ids, counts=cnt[:n], counters=ctr,
                                                  status=st) == n
    torch.cuda.synchronize()
    h, i, c = hits.cpu().numpy().view(np.uint32), ids.cpu().numpy().view(np.uint32), cnt.cpu().numpy().view(np.uint32)
    k = ctr.cpu().numpy().astype(np.uint64)
    assert (h[capacity * 4:] == SENT).all(), "the collect call wrote records past the last segment"
    assert (i[capacity:] == SENT).all(), "the collect call wrote instance ids past the last segment"
    assert (c[n:] == SENT).all(), "the collect call wrote counts past num_rays"
    assert k[2] == 1234 and k[3] == 5678, "counters[2:4] were touched"
    rec = h[:capacity * 4].view(rh.HIT)
    assert ((rec.view(np.uint32).reshape(-1, 4) != SENT).any(1) == (i[:capacity] != SENT)).all(), \
        "a record without its instance id, or the other way round"
    return rhi.items(i[:capacity], rec), c[:n], k[:2], rt.ray_hits_status(st)


def hits(rt, args, rays, hf):
    """count, then collect into exactly offsets[n] records, both under `hf` (a device filter, None, or UNFILTERED).  Asserts
    what must hold for ANY filter: offsets monotone, counts == diff(offsets), every segment filled, count's and collect's
    counters and status equal."""
    r = g.Result()
    rd = g.dev_rays(rt, rays)
    n = len(rays)
    r.offsets, r.ctr_count, r.st_count, off = count(rt, args, rd, hf)
    assert r.offsets[0] == 0 and (np.diff(r.offsets) >= 0).all()
    total = int(r.offsets[n])
    recs, r.counts, r.ctr_collect, r.st_collect = collect(rt, args, rd, hf, off, total)
    assert (r.counts.astype(np.int64) == np.diff(r.offsets)).all(), "collect's counts differ from the differences of offsets"
    assert (recs["instance"] != SENT).all(), "a segment was not filled"
    assert (r.ctr_count == r.ctr_collect).all(), f"counters differ: count {r.ctr_count}, collect {r.ctr_collect}"
    assert r.st_count == r.st_collect and not (r.st_collect & rt.RT_RAY_HITS_TRUNCATED)
    r.rows = [recs[r.offsets[k]:r.offsets[k + 1]] for k in range(n)]
    return r


def first(rt, args, rays, k, hf):
    """-> (rows: ITEM [n, k], counters uint64[2], status).  Sentinels lie behind both buffers and must survive; every record
    and every id of every row must have been written; counters[2:4] are not touched."""
    import torch
    rd = g.dev_rays(rt, rays)
    n = rd.shape[0]
    hbuf = torch.full(((n * k + PAD) * 4,), SENT, dtype=torch.int32, device="cuda")
    ibuf = torch.full((n * k + PAD,), SENT, dtype=torch.int32, device="cuda")
    h4 = hbuf[:n * k * 4].view(torch.float32).view(n, k, 4)
    ids = ibuf[:n * k].view(n, k)
    ctr = torch.zeros(4, dtype=torch.int64, device="cuda")
    ctr[2], ctr[3] = 1234, 5678
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    if hf is UNFILTERED:
        assert rt.RayFirstHitsInstanced(*args, rd, k, h4, ids, counters=ctr, status=st) == n
    else:
        assert rt.RayFirstHitsInstancedFiltered(*args, rd, k, hf, h4, ids, counters=ctr, status=st) == n
    torch.cuda.synchronize()
    h, i = hbuf.cpu().numpy().view(np.uint32), ibuf.cpu().numpy().view(np.uint32)
    assert (h[n * k * 4:] == SENT).all(), "the first-K call wrote records past the last row"
    assert (i[n * k:] == SENT).all(), "the first-K call wrote instance ids past the last row"
    assert (h[:n * k * 4].reshape(-1, 4) != SENT).any(1).all(), "a record of a row was not written"
    assert (i[:n * k] != SENT).all(), "an instance id of a row was not written"
    c = ctr.cpu().numpy().astype(np.uint64)
    assert c[2] == 1234 and c[3] == 5678, "counters[2:4] were touched"
    rows = rfi.items(i[:n * k], h[:n * k * 4].view(rh.HIT)).reshape(n, k)
    return rows, c[:2], rt.ray_first_status(st)


class Walk:
    """the reference of one (scene, ray set, filter): the filtered W with gates, its counters, and Ws -- computed once, never
    changed.  The attributes are ray_first_instanced_gpu.Walk's, so its check_rows serves the filtered rows too."""

    def __init__(self, scene, rays, flt):
        leaves, nodes, root, count = scene.tlas
        self.rays, self.flt = rays, flt
        self.rows, self.gates, self.box_tests, self.leaf_visits = isf.walk_gated(nodes, leaves, root, count, scene.records,
                                                                                 scene.trees, rays, flt)
        self.hits_box_tests = self.box_tests
        if scene.n == 0:                      # the all-hit query still counts its TLAS slots on a scene without instances
            _, self.hits_box_tests, _ = isf.walk(nodes, leaves, root, count, scene.records, scene.trees, rays, flt)
        self.dedup = rfi.dedup_all(self.rows, self.gates)
        self.nonempty = int(sum(len(r) > 0 for r in self.rows))
        self.longest = max([len(ws) for ws, _ in self.dedup] + [0])

    def expected(self, k):
        return rfi.expected(self.rows, self.gates, k, self.rays["tmax"], dedup=self.dedup)

    def share(self, k):
        return rfi.undecided_share(self.expected(k), self.rows)


def check_hits(r, walk, what, status=0):
    """the all-hit Result against the reference: offsets, rows as sorted items, exact counters"""
    assert r.st_count == status, f"{what}: status {r.st_count}"
    assert (r.offsets == rhi.offsets(walk.rows)).all(), f"{what}: offsets differ from the prefix sum of the walk's lengths"
    rhi.assert_rows_equal(r.rows, walk.rows, what)
    assert r.ctr_count[0] == walk.hits_box_tests and r.ctr_count[1] == walk.leaf_visits, \
        f"{what}: counters {r.ctr_count}, the walk counts {walk.hits_box_tests}, {walk.leaf_visits}"
