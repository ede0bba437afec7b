"""ctypes front-end of the CPU oracle (oracle/liboracle.so) and of the reference's own hierarchy checker
(oracle/_ref/libref_utilities.so = /root/reference/src/Utilities.cpp compiled unmodified).

TEST INFRASTRUCTURE ONLY: imported by tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg -- never by
the product package.
"""
from __future__ import annotations

import ctypes
import os
import subprocess
import tempfile

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "liboracle.so")
REF_PATH = os.path.join(_HERE, "_ref", "libref_utilities.so")

NODE = np.dtype([("min", "<f4", 3), ("w12", "<u4"), ("max", "<f4", 3), ("w28", "<u4")])
TRIANGLE_PAIR = np.dtype([("v0", "<f4", 3), ("primitive_id_0", "<u4"), ("v1", "<f4", 3), ("primitive_id_1", "<u4"),
                          ("v2", "<f4", 3), ("rotations", "<u2", 2), ("v3", "<f4", 3), ("pad3", "<f4")])

_lib = None


def build() -> None:
    subprocess.check_call(["make", "-s", "-C", _HERE, "all"])


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            build()
        L = ctypes.CDLL(LIB_PATH)
        vp, u32 = ctypes.c_void_p, ctypes.c_uint32
        L.ora_set_threads.argtypes = [ctypes.c_int]
        L.ora_get_threads.restype = ctypes.c_int
        L.ora_scene_aabb.argtypes = [vp, u32, vp]
        L.ora_morton_codes.argtypes = [vp, u32, vp, vp, vp]
        L.ora_radix_sort.argtypes = [vp, vp, vp, vp, u32]
        L.ora_build.argtypes = [vp, u32, vp, vp, vp, vp, vp]
        L.ora_build_pairs.argtypes = [vp, u32, vp, vp, vp, vp, vp]
        L.ora_build_pairs.restype = u32
        L.ora_build_hybrid_top.argtypes = [vp, u32, vp, vp]
        L.ora_build_hybrid_top.restype = u32
        L.ora_count_nodes.argtypes = [vp, u32, u32, vp]
        L.ora_verify_hierarchy.argtypes = [vp, u32, u32]
        L.ora_verify_hierarchy.restype = ctypes.c_int
        L.ora_trace.argtypes = [vp, vp, u32, u32, vp, vp, u32, vp, vp, ctypes.c_int, vp, u32, u32, u32, u32, u32, vp]
        L.ora_trace.restype = ctypes.c_int
        _lib = L
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def set_threads(n: int) -> None:
    lib().ora_set_threads(int(n))


def scene_aabb(tris: np.ndarray) -> np.ndarray:
    t = np.ascontiguousarray(tris, dtype=np.float32).reshape(-1, 9)
    out = np.zeros(6, dtype=np.int32)
    lib().ora_scene_aabb(_p(t), t.shape[0], _p(out))
    return out


def ordered_to_float(a: np.ndarray) -> np.ndarray:
    a = np.asarray(a, dtype=np.int32)
    return np.where(a >= 0, a, a ^ np.int32(0x7FFFFFFF)).astype(np.int32).view(np.float32)


def morton_codes(tris: np.ndarray, aabb_ordered: np.ndarray):
    t = np.ascontiguousarray(tris, dtype=np.float32).reshape(-1, 9)
    n = t.shape[0]
    codes, vals = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    a = np.ascontiguousarray(aabb_ordered, dtype=np.int32)
    lib().ora_morton_codes(_p(t), n, _p(a), _p(codes), _p(vals))
    return codes, vals


def radix_sort(keys: np.ndarray, vals: np.ndarray):
    k, v = np.ascontiguousarray(keys, np.uint32).copy(), np.ascontiguousarray(vals, np.uint32).copy()
    tk, tv = np.zeros_like(k), np.zeros_like(v)
    lib().ora_radix_sort(_p(k), _p(v), _p(tk), _p(tv), k.shape[0])
    return k, v


def build_bvh(tris: np.ndarray) -> dict:
    """RunBottomUpBuild on the CPU: returns nodes (2*max(n-1,1) slots), leaves, sorted codes/indices, scene box."""
    t = np.ascontiguousarray(tris, dtype=np.float32).reshape(-1, 9)
    n = t.shape[0]
    nodes = np.zeros(2 * max(n - 1, 1), dtype=NODE)
    leaves = np.zeros(max(n, 1), dtype=TRIANGLE_PAIR)
    codes, idx = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint32)
    aabb = np.zeros(6, np.int32)
    lib().ora_build(_p(t), n, _p(nodes), _p(leaves), _p(codes), _p(idx), _p(aabb))
    return dict(nodes=nodes, leaves=leaves[:n], codes=codes[:n], indices=idx[:n], aabb=aabb, n=n)


def build_pairs(tris: np.ndarray) -> dict:
    """RunBottomUpBuild with enable_pairs: shared-edge triangle pairs become quad leaves (deterministic slots)."""
    t = np.ascontiguousarray(tris, dtype=np.float32).reshape(-1, 9)
    n = t.shape[0]
    nodes = np.zeros(2 * max(n - 1, 1), dtype=NODE)
    leaves = np.zeros(max(n, 1), dtype=TRIANGLE_PAIR)
    codes, idx = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint32)
    aabb = np.zeros(6, np.int32)
    L = int(lib().ora_build_pairs(_p(t), n, _p(nodes), _p(leaves), _p(codes), _p(idx), _p(aabb)))
    return dict(nodes=nodes[:2 * max(L - 1, 1)], leaves=leaves[:L], codes=codes[:L], indices=idx[:L], aabb=aabb, n=n, L=L)


def build_hybrid(tris: np.ndarray) -> dict:
    """RunBottomUpBuild(hybrid=true): the LBVH plus the deterministic SAH top tree at slots >= 2L.
    Trace root = (root, 2) with root = 2L+1 (main.cu:222-223)."""
    b = build_bvh(tris)
    n = b["n"]
    nodes = np.zeros(2 * max(n, 1) + 2 * 256 + 8, dtype=NODE)
    nodes[:b["nodes"].shape[0]] = b["nodes"]
    sub = np.zeros(256, np.uint32)
    k = lib().ora_build_hybrid_top(_p(nodes), n, _p(b["aabb"]), _p(sub))
    b.update(nodes=nodes, subroots=sub[:k], root=max(2 * n, 2) + 1)
    return b


def build_sah(tris: np.ndarray, pairs: bool = False, splits: bool = False) -> dict:
    """RunSahBuild, deterministic restatement.  Trace root = (0, 1) (main.cu:222-223).
    nodes: the 2*64 + 2L slots in use (top tree in [0, 128), cell trees above); L = items (leaves, or leaf references
    with splits); leaves: the R TrianglePair records."""
    t = np.ascontiguousarray(tris, dtype=np.float32).reshape(-1, 9)
    n = t.shape[0]
    nodes = np.zeros(128 + 2 * (n + n // 5) + 2, dtype=NODE)
    leaves = np.zeros(max(n, 1), dtype=TRIANGLE_PAIR)
    cells = np.zeros(64, np.uint32)
    nrec = np.zeros(1, np.uint32)
    L = lib()
    L.ora_build_sah.restype = ctypes.c_uint32
    L.ora_build_sah.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    nl = int(L.ora_build_sah(_p(t), n, int(bool(pairs)), int(bool(splits)), _p(nodes), _p(leaves), _p(cells), _p(nrec)))
    return dict(nodes=nodes[:128 + 2 * nl], leaves=leaves[:int(nrec[0])], n=n, L=nl, R=int(nrec[0]), root=0, count=1,
                cell_counts=cells)


def count_nodes(nodes: np.ndarray, root: int, count: int) -> tuple:
    out = np.zeros(3, np.int32)
    lib().ora_count_nodes(_p(np.ascontiguousarray(nodes)), root, count, _p(out))
    return int(out[0]), int(out[1]), int(out[2])


def verify_hierarchy(nodes: np.ndarray, root: int, count: int) -> int:
    return int(lib().ora_verify_hierarchy(_p(np.ascontiguousarray(nodes)), root, count))


NUM_LODS = 13


class _Texture(ctypes.Structure):  # ora_texture
    _fields_ = [("mips", ctypes.c_void_p * NUM_LODS), ("size_x", ctypes.c_int32 * NUM_LODS),
                ("size_y", ctypes.c_int32 * NUM_LODS), ("max_lod", ctypes.c_uint32), ("pad", ctypes.c_uint32)]


def generate_lods(mip0: np.ndarray) -> list:
    """Texture::GenerateLODs: mip0 is [sy, sx] uint32 (r | g<<8 | b<<16 | a<<24); returns the list of levels."""
    L = lib()
    L.ora_lod_sizes.restype = ctypes.c_uint32
    L.ora_lod_sizes.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]
    L.ora_generate_lod.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p]
    mip0 = np.ascontiguousarray(mip0, np.uint32)
    sx, sy = np.zeros(NUM_LODS, np.int32), np.zeros(NUM_LODS, np.int32)
    max_lod = L.ora_lod_sizes(mip0.shape[1], mip0.shape[0], _p(sx), _p(sy))
    mips = [mip0]
    for l in range(1, max_lod + 1):
        dst = np.zeros((sy[l], sx[l]), np.uint32)
        L.ora_generate_lod(_p(mips[-1]), int(sx[l - 1]), int(sy[l - 1]), _p(dst))
        mips.append(dst)
    return mips


def _texture_table(textures):
    """textures: list of mip chains (each a list of [sy, sx] uint32 arrays).  Returns (ctypes array, keepalive)."""
    arr = (_Texture * len(textures))()
    keep = []
    for t, chain in enumerate(textures):
        assert 1 <= len(chain) <= NUM_LODS
        for l, m in enumerate(chain):
            m = np.ascontiguousarray(m, np.uint32)
            keep.append(m)
            arr[t].mips[l] = m.ctypes.data
            arr[t].size_x[l], arr[t].size_y[l] = m.shape[1], m.shape[0]
        arr[t].max_lod = len(chain) - 1
    return arr, keep


def trace(leaves, nodes, root, count, camera, w, h, *, render_type=0, attributes=None, materials=None, light=(0, 0, 0),
          rows=None, spp=1, textures=None):
    """TraceRays on the CPU.  Returns (rgba8 [h, w, 4] uint8, counters [box, tri, max_stack, dropped_pushes]).
    textures: list of mip chains (see generate_lods) indexed by Material.texture / .bump / .disp."""
    L = lib()
    L.ora_set_textures.argtypes = [ctypes.c_void_p, ctypes.c_uint32]
    if textures:
        table, _keep = _texture_table(textures)
        L.ora_set_textures(ctypes.cast(table, ctypes.c_void_p), len(textures))
    else:
        L.ora_set_textures(None, 0)
    try:
        return _trace(leaves, nodes, root, count, camera, w, h, render_type, attributes, materials, light, rows, spp)
    finally:
        L.ora_set_textures(None, 0)


def _trace(leaves, nodes, root, count, camera, w, h, render_type, attributes, materials, light, rows, spp):
    rgba = np.zeros((h, w, 4), np.uint8)
    counters = np.zeros(4, np.uint64)
    y0, y1 = (0, h) if rows is None else rows
    lt = np.asarray(light, np.float32)
    cam = np.ascontiguousarray(camera)
    nm = 0 if materials is None else materials.shape[0]
    rc = lib().ora_trace(_p(np.ascontiguousarray(leaves)), _p(np.ascontiguousarray(nodes)), root, count,
                         _p(None if attributes is None else np.ascontiguousarray(attributes)),
                         _p(None if materials is None else np.ascontiguousarray(materials)), nm, _p(cam), _p(lt),
                         render_type, _p(rgba), w, h, y0, y1, spp, _p(counters))
    if rc != 0:
        raise ValueError(f"oracle: unsupported render type {render_type}")
    return rgba, counters


# ---------------------------------------------------------------- ordered per-ray walkers (rt_oracle.h, ora_walk_rays*)
RAY = np.dtype([("origin", "<f4", 3), ("tmin", "<f4"), ("dir", "<f4", 3), ("tmax", "<f4")])
HIT = np.dtype([("t", "<f4"), ("primitive_id", "<u4"), ("u", "<f4"), ("v", "<f4")])
WALK_BOX, WALK_TRI, WALK_DEPTH, WALK_DROPPED, WALK_LOW_BASE_DEPTH, WALK_HIGH_BASE_DROPPED = range(6)   # columns of `stats`


def _walk_fn(name):
    f = getattr(lib(), name)
    f.restype = None
    f.argtypes = None
    return f


def _tree_args(leaves, nodes):
    lv, nd = np.ascontiguousarray(leaves), np.ascontiguousarray(nodes)
    assert lv.dtype.itemsize == 64 and nd.dtype.itemsize == 32
    return lv, nd


def _ray_args(rays):
    r = np.ascontiguousarray(rays)
    assert r.dtype.itemsize == 32, "RAY records"
    return r, np.zeros(r.shape[0], HIT)


def _u32(v):
    return ctypes.c_uint32(int(v))


def walk_rays(leaves, nodes, root, count, rays, any_hit=False, stack_limit=64):
    """trace_ray over RAY records -> (HIT [n], stats uint32 [n, 4]: box tests, triangle tests, greatest stack depth, dropped
    pushes).  stack_limit (every walker takes it): 64, the kernels'; up to 1024 to see what a walk that drops nothing does"""
    lv, nd = _tree_args(leaves, nodes)
    r, hits = _ray_args(rays)
    stats = np.zeros((r.shape[0], 4), np.uint32)
    _walk_fn("ora_walk_rays")(_p(lv), _p(nd), _u32(root), _u32(count), _p(r), _u32(r.shape[0]), int(bool(any_hit)),
                              _u32(stack_limit), _p(hits), _p(stats))
    return hits, stats


def walk_rays_motion(leaves0, nodes0, leaves1, nodes1, root, count, rays, times, any_hit=False, stack_limit=64):
    """the motion arm: two poses of one tree and a time per ray -> as walk_rays"""
    l0, n0 = _tree_args(leaves0, nodes0)
    l1, n1 = _tree_args(leaves1, nodes1)
    assert l0.shape == l1.shape and n0.shape == n1.shape
    r, hits = _ray_args(rays)
    t = np.ascontiguousarray(np.broadcast_to(np.asarray(times, np.float32), (r.shape[0],)))
    stats = np.zeros((r.shape[0], 4), np.uint32)
    _walk_fn("ora_walk_rays_motion")(_p(l0), _p(n0), _p(l1), _p(n1), _u32(root), _u32(count), _p(r), _p(t), _u32(r.shape[0]),
                                     int(bool(any_hit)), _u32(stack_limit), _p(hits), _p(stats))
    return hits, stats


def walk_rays_spheres(leaves, nodes, root, count, spheres, rays, any_hit=False, num_spheres=None, stack_limit=64):
    """the sphere arm: a leaf's primitive_id_0 indexes `spheres` (float32 [k, 4]) -> as walk_rays, records {t, index, far root, 0}"""
    lv, nd = _tree_args(leaves, nodes)
    s = np.ascontiguousarray(spheres, np.float32).reshape(-1, 4)
    r, hits = _ray_args(rays)
    stats = np.zeros((r.shape[0], 4), np.uint32)
    _walk_fn("ora_walk_rays_spheres")(_p(lv), _p(nd), _u32(root), _u32(count), _p(s),
                                      _u32(s.shape[0] if num_spheres is None else num_spheres), _p(r), _u32(r.shape[0]),
                                      int(bool(any_hit)), _u32(stack_limit), _p(hits), _p(stats))
    return hits, stats


def walk_rays_instanced(tlas_leaves, tlas_nodes, root, count, blas, rays, object_rays, enterable, any_hit=False,
                        tlas_nodes1=None, times=None, cull=None, stack_limit=64):
    """the two-level arm.  blas[k] = (leaves, nodes, root, count) of instance k's BLAS; object_rays: float32 [n, K, 6] (origin,
    direction of ray i inside instance k); enterable: bool [n, K]; cull: None or uint8 [K] (0, 1: a < 0 rejected, 2: a > 0);
    tlas_nodes1 / times: the TLAS's second pose and a time per ray (both or neither).
    -> (HIT [n], instance ids uint32 [n], stats uint32 [n, 6]: walk_rays's four, the greatest depth inside an instance entered
    below depth 16, the pushes dropped inside instances entered above depth 16)"""
    tl, tn = _tree_args(tlas_leaves, tlas_nodes)
    r, hits = _ray_args(rays)
    n, K = r.shape[0], len(blas)
    keep = [_tree_args(b[0], b[1]) for b in blas]
    ptr = ctypes.c_void_p * max(K, 1)
    pl = ptr(*[k[0].ctypes.data for k in keep])
    pn = ptr(*[k[1].ctypes.data for k in keep])
    roots = np.array([b[2] for b in blas], np.uint32)
    counts = np.array([b[3] for b in blas], np.uint32)
    obj = np.ascontiguousarray(object_rays, np.float32)
    ent = np.ascontiguousarray(enterable, np.uint8)
    assert obj.shape == (n, K, 6) and ent.shape == (n, K)
    assert (tlas_nodes1 is None) == (times is None)
    tn1 = t = None
    if times is not None:
        tn1 = np.ascontiguousarray(tlas_nodes1)
        assert tn1.shape == tn.shape and tn1.dtype.itemsize == 32
        t = np.ascontiguousarray(np.broadcast_to(np.asarray(times, np.float32), (n,)))
    cl = None if cull is None else np.ascontiguousarray(cull, np.uint8)
    assert cl is None or cl.shape == (K,)
    ids = np.zeros(n, np.uint32)
    stats = np.zeros((n, 6), np.uint32)
    _walk_fn("ora_walk_rays_instanced")(_p(tl), _p(tn), _p(tn1), _u32(root), _u32(count), _u32(K), pl, pn, _p(roots), _p(counts),
                                        _p(cl), _p(r), _p(t), _u32(n), _p(obj), _p(ent), int(bool(any_hit)),
                                        _u32(stack_limit), _p(hits), _p(ids), _p(stats))
    return hits, ids, stats


# ---------------------------------------------------------------- the reference's own checker (oracle/_ref)
class _HierarchyStats(ctypes.Structure):  # Utilities.h:3-7
    _fields_ = [("numNodes", ctypes.c_int), ("numLeafNodes", ctypes.c_int), ("numTreeNodes", ctypes.c_int)]


_ref = None


def ref_available() -> bool:
    return os.path.exists(REF_PATH)


def _reflib():
    global _ref
    if _ref is None:
        R = ctypes.CDLL(REF_PATH)
        R.count = getattr(R, "_Z10CountNodesP4Nodejj")           # HierarchyStats CountNodes(Node*, unsigned, unsigned)
        R.count.restype = _HierarchyStats
        R.count.argtypes = [ctypes.c_void_p, ctypes.c_uint, ctypes.c_uint]
        R.verify = getattr(R, "_Z15VerifyHierarchyP4Nodejj")    # void VerifyHierarchy(Node*, unsigned, unsigned)
        R.verify.restype = None
        R.verify.argtypes = [ctypes.c_void_p, ctypes.c_uint, ctypes.c_uint]
        _ref = R
    return _ref


def ref_count_nodes(nodes: np.ndarray, root: int, count: int) -> tuple:
    """Reference CountNodes (Utilities.cpp:32-44), the compiled reference code itself."""
    s = _reflib().count(_p(np.ascontiguousarray(nodes)), root, count)
    return s.numNodes, s.numLeafNodes, s.numTreeNodes


def ref_verify_hierarchy(nodes: np.ndarray, root: int, count: int) -> str:
    """Reference VerifyHierarchy (Utilities.cpp:77-83).  It reports by printing to stderr; returns what it printed
    ('' = hierarchy valid)."""
    import sys
    R = _reflib()
    a = np.ascontiguousarray(nodes)
    sys.stderr.flush()
    libc = ctypes.CDLL(None)
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        saved = os.dup(2)
        try:
            os.dup2(tmp.fileno(), 2)
            R.verify(_p(a), root, count)
            libc.fflush(None)
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        return tmp.read().decode(errors="replace")


# ---------------------------------------------------------------- the reference's camera and argument parser (oracle/_ref)
class _InputState(ctypes.Structure):  # Input.cuh:4-15
    _fields_ = [(k, ctypes.c_bool) for k in ("w", "a", "s", "d", "q", "e", "space", "mouse_down")] + \
               [("prev_x", ctypes.c_int), ("prev_y", ctypes.c_int)]


class _AABB(ctypes.Structure):
    _fields_ = [("v", ctypes.c_float * 6)]


class _RefArguments(ctypes.Structure):  # Arguments.h:28-33
    _fields_ = [("build_type", ctypes.c_int), ("enable_splits", ctypes.c_bool), ("enable_pairs", ctypes.c_bool),
                ("render_type", ctypes.c_int)]


def ref_camera_available() -> bool:
    return os.path.exists(os.path.join(_HERE, "_ref", "libref_camera.so"))


def _refcam():
    R = ctypes.CDLL(os.path.join(_HERE, "_ref", "libref_camera.so"))
    vp = ctypes.c_void_p
    R.update = getattr(R, "_Z12UpdateCameraR6Camera"); R.update.argtypes = [vp]
    R.init = getattr(R, "_Z16InitialiseCameraR6Camera4AABB"); R.init.argtypes = [vp, _AABB]
    R.zoom = getattr(R, "_Z16UpdateCameraZoomR6Camerai"); R.zoom.argtypes = [vp, ctypes.c_int]
    R.move = getattr(R, "_Z20UpdateCameraPositionR6Camera10InputState"); R.move.argtypes = [vp, _InputState]
    R.look = getattr(R, "_Z21UpdateCameraLookDeltaR6Cameraff"); R.look.argtypes = [vp, ctypes.c_float, ctypes.c_float]
    return R


def ref_update_camera(cam: np.ndarray) -> np.ndarray:
    """Camera.cu:8-29 (the reference's own code): cam is a 64-byte Camera record; returns the updated copy."""
    c = np.ascontiguousarray(cam).copy()
    _refcam().update(_p(c))
    return c


def ref_initialise_camera(aabb) -> np.ndarray:
    """Camera.cu:62-91"""
    c = np.zeros(64, np.uint8)
    box = _AABB()
    for k in range(6):
        box.v[k] = float(aabb[k])
    _refcam().init(_p(c), box)
    return c


def ref_camera_controls(cam: np.ndarray, keys=(), look=None, zoom=None) -> np.ndarray:
    """UpdateCameraPosition / UpdateCameraLookDelta / UpdateCameraZoom (Camera.cu:31-60) in that order."""
    c = np.ascontiguousarray(cam).copy()
    R = _refcam()
    if keys:
        st = _InputState()
        for k in keys:
            setattr(st, k, True)
        R.move(_p(c), st)
    if look is not None:
        R.look(_p(c), ctypes.c_float(look[0]), ctypes.c_float(look[1]))
    if zoom is not None:
        R.zoom(_p(c), int(zoom))
    return c


def ref_parse_cmd(argv) -> tuple:
    """Arguments.cpp:47-63 ParseCmd (the reference's own code): returns (build_type, enable_splits, enable_pairs, render_type)."""
    R = ctypes.CDLL(os.path.join(_HERE, "_ref", "libref_arguments.so"))
    f = getattr(R, "_Z8ParseCmdiPPc")
    f.restype = _RefArguments
    f.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_char_p)]
    arr = (ctypes.c_char_p * len(argv))(*[a.encode() for a in argv])
    a = f(len(argv), arr)
    return int(a.build_type), bool(a.enable_splits), bool(a.enable_pairs), int(a.render_type)


# ---------------------------------------------------------------- the reference's Pairing.cuh (oracle/_ref/libref_pairing.so)
def ref_pairing_available() -> bool:
    return os.path.exists(os.path.join(_HERE, "_ref", "libref_pairing.so"))


def ref_pair_decision(a9: np.ndarray, b9: np.ndarray) -> tuple:
    """CanFormTrianglePair && ShouldFormTrianglePair (Pairing.cuh:35-58) on two 9-float triangles: (merge, rot_a, rot_b)."""
    R = ctypes.CDLL(os.path.join(_HERE, "_ref", "libref_pairing.so"))
    R.ref_pair_decision.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    rot = np.zeros(2, np.int32)
    m = R.ref_pair_decision(_p(np.ascontiguousarray(a9, np.float32)), _p(np.ascontiguousarray(b9, np.float32)), _p(rot))
    return bool(m), int(rot[0]), int(rot[1])


def ref_create_pair(a9, b9, a_id: int, b_id: int, rot_a: int, rot_b: int) -> np.ndarray:
    """CreateTrianglePair (Pairing.cuh:60-77): the 64-byte TrianglePair record (pad3, bytes 60..63, is not set by the reference)."""
    R = ctypes.CDLL(os.path.join(_HERE, "_ref", "libref_pairing.so"))
    R.ref_create_pair.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint, ctypes.c_uint, ctypes.c_int, ctypes.c_int,
                                  ctypes.c_void_p]
    out = np.zeros(64, np.uint8)
    R.ref_create_pair(_p(np.ascontiguousarray(a9, np.float32)), None if b9 is None else _p(np.ascontiguousarray(b9, np.float32)),
                      a_id, b_id, rot_a, rot_b, _p(out))
    return out


def ref_struct_layout() -> np.ndarray:
    """sizeof / offsetof of the reference's Triangle, Node, TrianglePair, Camera, Attributes, AABB (30 ints, see the driver)."""
    R = ctypes.CDLL(os.path.join(_HERE, "_ref", "libref_pairing.so"))
    out = np.zeros(30, np.int32)
    R.ref_struct_layout(_p(out))
    return out


def ref_pack_node(mn, mx, parent: int, count: int, child: int, type_: int) -> np.ndarray:
    R = ctypes.CDLL(os.path.join(_HERE, "_ref", "libref_pairing.so"))
    R.ref_pack_node.argtypes = [ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_uint] * 4 + [ctypes.c_void_p]
    out = np.zeros(1, NODE)
    R.ref_pack_node(_p(np.asarray(mn, np.float32)), _p(np.asarray(mx, np.float32)), parent, count, child, type_, _p(out))
    return out


# ---------------------------------------------------------------- Common.cuh's small host-callable arithmetic, both sides
def box_helpers(which: str):
    """(triangle_centre, triangle_box, box_centre, box_combine, box_intersection) of the oracle (`which` = "ora": the helpers
    its build paths call) or of the reference's Common.cuh compiled from its tree (`which` = "ref").  Each takes / returns
    float32 arrays; box_intersection returns (box, valid)."""
    L = lib() if which == "ora" else ctypes.CDLL(os.path.join(_HERE, "_ref", "libref_pairing.so"))
    pre = "ora_" if which == "ora" else "ref_"
    vp = ctypes.c_void_p

    def call(name, ins, nout, ret_int=False):
        f = getattr(L, pre + name)
        f.argtypes = [vp] * (len(ins) + 1)
        f.restype = ctypes.c_int if ret_int else None
        arrs = [np.ascontiguousarray(a, np.float32) for a in ins]
        out = np.zeros(nout, np.float32)
        r = f(*[_p(a) for a in arrs], _p(out))
        return (out, bool(r)) if ret_int else out

    return (lambda v9: call("triangle_centre", [v9], 3), lambda v9: call("triangle_box", [v9], 6),
            lambda b6: call("box_centre", [b6], 3), lambda a6, b6: call("box_combine", [a6, b6], 6),
            lambda a6, b6: call("box_intersection", [a6, b6], 6, ret_int=True))


# ---------------------------------------------------------------- the reference's own kernels, run on the CPU
# oracle/_ref/libref_kernels.so: BottomUpBuilder.cu and Tracer.cu from the reference tree, #included by
# oracle/ref_kernels_driver.cpp, which emulates each launch serially (TraceRays: rows on up to 16 threads).
REF_KERNELS_PATH = os.path.join(_HERE, "_ref", "libref_kernels.so")
_refk = None


def ref_kernels_available() -> bool:
    return os.path.exists(REF_KERNELS_PATH)


def _refkernels():
    global _refk
    if _refk is None:
        R = ctypes.CDLL(REF_KERNELS_PATH)
        vp, u32 = ctypes.c_void_p, ctypes.c_uint32
        R.ref_morton.argtypes = [vp, u32, vp, vp, vp]
        R.ref_morton.restype = None
        R.ref_morton_pairs.argtypes = [vp, u32, vp, vp, vp]
        R.ref_morton_pairs.restype = u32
        R.ref_hierarchy.argtypes = [vp, u32, vp, vp]
        R.ref_hierarchy.restype = None
        R.ref_triangles.argtypes = [vp, vp, vp, u32]
        R.ref_triangles.restype = None
        R.ref_aabbs.argtypes = [vp, vp, vp, vp, u32]
        R.ref_aabbs.restype = None
        R.ref_trace.argtypes = [vp, vp, u32, u32, vp, vp, u32, vp, u32, vp, u32, vp, ctypes.c_int, ctypes.c_int,
                                ctypes.c_int, vp, vp]
        R.ref_trace.restype = None
        _refk = R
    return _refk


def _tris9(tris):
    return np.ascontiguousarray(tris, dtype=np.float32).reshape(-1, 9)


def ref_morton(tris: np.ndarray, aabb_ordered: np.ndarray):
    """GenerateMortonCodes (BottomUpBuilder.cu:98-115): (codes, values) in input order."""
    t = _tris9(tris)
    n = t.shape[0]
    codes, vals = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint32)
    _refkernels().ref_morton(_p(t), n, _p(np.ascontiguousarray(aabb_ordered, np.int32)), _p(codes), _p(vals))
    return codes[:n], vals[:n]


def ref_morton_pairs(tris: np.ndarray, aabb_ordered: np.ndarray):
    """GenerateMortonCodesPairs (BottomUpBuilder.cu:117-164), threads in gid order: (codes, values) of the L leaves in
    slot order.  values: first triangle's index, | 0x80000000 for a pair."""
    t = _tris9(tris)
    n = t.shape[0]
    codes, vals = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint32)
    L = int(_refkernels().ref_morton_pairs(_p(t), n, _p(np.ascontiguousarray(aabb_ordered, np.int32)), _p(codes),
                                           _p(vals)))
    return codes[:L], vals[:L]


def ref_hierarchy(sorted_codes: np.ndarray):
    """GenerateHierarchy (BottomUpBuilder.cu:167-215) over L sorted codes: (nodes [2*max(L-1,1)], leaf_indices [L]).
    Only the child / type / parent words are written; boxes and counts stay zero."""
    c = np.ascontiguousarray(sorted_codes, np.uint32).copy()
    L = c.shape[0]
    nodes = np.zeros(2 * max(L - 1, 1), dtype=NODE)
    leaf_idx = np.zeros(max(L, 1), np.uint32)
    _refkernels().ref_hierarchy(_p(c), L, _p(nodes), _p(leaf_idx))
    return nodes, leaf_idx[:L]


def ref_triangles(sorted_indices: np.ndarray, tris: np.ndarray) -> np.ndarray:
    """GenerateTriangles (BottomUpBuilder.cu:287-312).  The kernel copies an uninitialised local into a single leaf's
    primitive ids, rotations and pad3, and into every leaf's pad3 (Q1): those bytes are indeterminate, not compared."""
    t = _tris9(tris)
    t1 = np.zeros((t.shape[0] + 1, 9), np.float32)     # the kernel reads the triangle after each leaf's first one
    t1[:t.shape[0]] = t
    s = np.ascontiguousarray(sorted_indices, np.uint32)
    L = s.shape[0]
    out = np.zeros(max(L, 1), TRIANGLE_PAIR)
    _refkernels().ref_triangles(_p(s), _p(t1), _p(out), L)
    return out[:L]


def ref_aabbs(nodes: np.ndarray, leaf_indices: np.ndarray, sorted_indices: np.ndarray, leaves: np.ndarray) -> np.ndarray:
    """GenerateAABBs (BottomUpBuilder.cu:217-285), zeroed locks, serial: returns a copy of nodes with boxes and counts."""
    out = np.ascontiguousarray(nodes).copy()
    li = np.ascontiguousarray(leaf_indices, np.uint32)
    _refkernels().ref_aabbs(_p(out), _p(li), _p(np.ascontiguousarray(sorted_indices, np.uint32)),
                            _p(np.ascontiguousarray(leaves)), li.shape[0])
    return out


def ref_build_lbvh(tris: np.ndarray, pairs: bool = False, aabb_ordered=None) -> dict:
    """RunBottomUpBuild through the reference's kernels: Morton (plain or pairs) -> stable sort by key (the radix sort's
    contract; RadixSort.cu itself is not emulated) -> GenerateHierarchy -> GenerateTriangles -> GenerateAABBs.  The
    scene box is the oracle's (ora_scene_aabb) unless given.  Same dict shape as build_bvh / build_pairs.
    With pairs=True the leaf order before the sort is the serial arrival order (see the driver)."""
    t = _tris9(tris)
    n = t.shape[0]
    aabb = scene_aabb(t) if aabb_ordered is None else np.ascontiguousarray(aabb_ordered, np.int32)
    codes, vals = (ref_morton_pairs if pairs else ref_morton)(t, aabb)
    order = np.argsort(codes, kind="stable")
    sc, sv = codes[order], vals[order]
    L = sc.shape[0]
    nodes, leaf_idx = ref_hierarchy(sc)
    leaves = ref_triangles(sv, t)
    if L == 1:
        # GenerateHierarchy writes nothing for one leaf; GenerateAABBs then reads leaf_indices[0] = 0 (the caller's
        # zeroed buffer) and stops at once
        nodes = nodes[:2]
    nodes = ref_aabbs(nodes, leaf_idx, sv, leaves)
    out = dict(nodes=nodes, leaves=leaves, codes=sc, indices=sv, leaf_indices=leaf_idx, aabb=aabb, n=n, L=L)
    return out


def ref_trace(leaves, nodes, root, count, camera, w, h, *, render_type=0, attributes=None, materials=None,
              light=(0, 0, 0), textures=None):
    """TraceRays (Tracer.cu:471-595) of the reference, run on the CPU over a w x h frame.  Returns (rgba8 [h, w, 4],
    counters [box_tests, tri_tests]): box_tests is the kernel's own counter, tri_tests the sum of its per-ray
    TraceStats.tri_tests (read by the driver when the kernel hands its record to atomicAdd).
    TraceRays reads attributes[primitive_id] and materials[material_id] for every pixel, whatever the render type:
    without attributes / materials, zeroed attributes for every primitive id of the leaves and one default material
    stand in (render types 0-2 do not use them)."""
    lv = np.ascontiguousarray(leaves)
    if attributes is None:
        k = 1 if lv.shape[0] == 0 else int(max(lv["primitive_id_0"].max(), lv["primitive_id_1"].max())) + 1
        attributes = np.zeros(k, np.dtype([("b", "u1", 72)]))
    at = np.ascontiguousarray(attributes)
    if materials is None:
        materials = np.zeros(1, np.dtype([("f", "<f4", 10), ("i", "<i4", 3)]))
        materials["i"] = -1
    mt = np.ascontiguousarray(materials)
    assert at.dtype.itemsize == 72 and mt.dtype.itemsize == 52
    table, _keep = _texture_table(textures) if textures else (None, None)
    rgba = np.zeros((h, w, 4), np.uint8)
    tests = np.zeros(2, np.uint64)
    lt = np.asarray(light, np.float32)
    _refkernels().ref_trace(_p(lv), _p(np.ascontiguousarray(nodes)), root, count, _p(np.ascontiguousarray(camera)),
                            _p(at), at.shape[0], _p(mt), mt.shape[0],
                            None if table is None else ctypes.cast(table, ctypes.c_void_p), len(textures or ()),
                            _p(lt), w, h, render_type, _p(rgba), _p(tests))
    return rgba, tests


# ---------------------------------------------------------------- the reference's SAH task builder, run on the CPU
# oracle/_ref/libref_sah.so: SharedTaskBuilder.cu from the reference tree, #included by oracle/ref_sah_driver.cpp, which
# runs a block with one host thread per CUDA thread and hands the turn round in threadIdx.x order between barriers;
# and ExtractDepth of BottomUpBuilder.cu (oracle/ref_extract_depth_driver.cpp).  Nothing here loads libref_kernels.so.
REF_SAH_PATH = os.path.join(_HERE, "_ref", "libref_sah.so")
AABB6 = np.dtype(("<f4", 6))
_refs = None

CHILD_BOX, CHILD_TRI = 1, 2     # ChildType (Common.cuh:36-42)


def ref_sah_available() -> bool:
    return os.path.exists(REF_SAH_PATH)


def _refsah():
    global _refs
    if _refs is None:
        R = ctypes.CDLL(REF_SAH_PATH)
        vp, u32, ci = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int
        R.ref_shared_task_build.argtypes = [u32, u32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, u32, vp]
        R.ref_shared_task_build.restype = ci
        R.ref_extract_depth.argtypes = [vp, vp, vp, vp, vp, u32, u32, u32]
        R.ref_extract_depth.restype = ci
        _refs = R
    return _refs


def ref_shared_task_build(blocks: int, width: int, c_aabbs, p_aabbs, nodes: np.ndarray, aabbs, prim_ids, ids,
                          block_counts, block_scan, num_leaves: int, top_of_tree: bool, leaf_type: int,
                          base_write_offset: int) -> np.ndarray:
    """SharedTaskBuild<<<blocks, width>>> (SharedTaskBuilder.cu:909-995) of the reference, run on the CPU; arguments as
    the kernel names them.  nodes (NODE records) is written in place.  ids: the first id buffer (`scratch`): position
    block_scan[b] + i holds the i-th item of block b; the second buffer and the task queue are allocated here.
    c_aabbs / p_aabbs: one box (6 floats) per block; aabbs: one box per item id; prim_ids: (id, count) per item id.
    Returns the kernel's `error` flag per block."""
    _refsah()
    counts = np.ascontiguousarray(block_counts, np.int32)
    scan = np.ascontiguousarray(block_scan, np.int32)
    ids = np.ascontiguousarray(ids, np.int32)
    c = np.ascontiguousarray(c_aabbs, np.float32).reshape(-1, 6)
    p = np.ascontiguousarray(p_aabbs, np.float32).reshape(-1, 6)
    boxes = np.ascontiguousarray(aabbs, np.float32).reshape(-1, 6)
    prims = np.ascontiguousarray(prim_ids, np.uint32).reshape(-1, 2)
    assert nodes.dtype == NODE and nodes.flags.c_contiguous and nodes.flags.writeable
    assert counts.shape[0] >= blocks and c.shape[0] >= blocks and p.shape[0] >= blocks
    ends = [int(scan[b]) + int(counts[b]) for b in range(blocks) if counts[b]]
    span = max(ends, default=0)
    assert span <= num_leaves and ids.shape[0] >= span
    used = np.concatenate([ids[int(scan[b]):int(scan[b]) + int(counts[b])] for b in range(blocks)] or [ids[:0]])
    if top_of_tree:      # the items are block indices: their boxes, and their scan for the sub-root slot
        assert used.size == 0 or (0 <= used.min() and used.max() < min(boxes.shape[0], scan.shape[0]))
        assert nodes.shape[0] >= 128 + 2 * (int(scan[used].max()) if used.size else 0) + 1
    else:
        assert used.size == 0 or (0 <= used.min() and used.max() < min(boxes.shape[0], prims.shape[0]))
    first = base_write_offset if top_of_tree else base_write_offset + 2 * int(min(scan[:blocks]))
    assert nodes.shape[0] >= first + 2 * span + 2, "every task claims at most two slots per item"
    scratch = np.zeros(2 * max(num_leaves, 1), np.int32)
    scratch[:span] = ids[:span]
    tasks = np.zeros(max(num_leaves, 1) + 64, np.dtype(("<u4", 16)))
    nl = np.array([num_leaves], np.int32)
    errors = np.zeros(blocks, np.int32)
    rc = _refsah().ref_shared_task_build(blocks, width, _p(tasks), _p(c), _p(p), _p(nodes), _p(boxes), _p(prims),
                                         _p(scratch), _p(counts), _p(scan), _p(nl), int(bool(top_of_tree)),
                                         int(leaf_type), base_write_offset, _p(errors))
    assert rc == 0, "ref_shared_task_build: width outside [64, 1024] or a thread could not be started"
    return errors


def ref_extract_depth(nodes: np.ndarray, aabb_ordered: np.ndarray, num_leaves: int):
    """ExtractDepth<<<1, 256>>>(nodes, ..., root 0, depth 8, num_leaves) (BottomUpBuilder.cu:314-371), threads in tid
    order (oracle/ref_extract_depth_driver.cpp, part of libref_sah.so).  Returns (sub-root pair slots [K], their boxes [K, 6], c_aabb: the union of those boxes grown from the empty
    float box, p_aabb: the scene box as floats)."""
    _refsah()
    nd = np.ascontiguousarray(nodes).copy()
    idx = np.zeros((256, 2), np.uint32)
    boxes = np.zeros((256, 6), np.float32)
    fmax = np.finfo(np.float32).max
    c = np.array([fmax] * 3 + [-fmax] * 3, np.float32)          # empty_float_aabb (BuildWrapper.cu:290-291)
    p = np.ascontiguousarray(aabb_ordered, np.int32).copy()
    k = int(_refsah().ref_extract_depth(_p(nd), _p(idx), _p(boxes), _p(c), _p(p), 0, 8, num_leaves))
    assert (idx[:k, 1] == 2).all()
    return idx[:k, 0].copy(), boxes[:k].copy(), c, p.view(np.float32)
