"""The smallest trees that take a lane of the motion, sphere and instanced ray queries to each level of its traversal stack,
and the inputs tests/test_stack_walk_ref_cpu.py and tests/test_gpu_stack_depths.py share.

A lane's stack holds levels 0..15 in an LDS column and 16..63 in a private array; a push onto 64 entries is dropped, the
nearest child's included (oracle/rt_oracle.c, trace_ray and the walkers ora_walk_rays*).

COMBS (the _comb of tests/test_gpu_ray_first.py, generalised).  Every box is [-50, 50]^3 and every ray starts within 0.05 of
the origin, so every slot is entered with one front distance and ties decide: the first slot of a pair is the nearest child
and the second is pushed.

  tri_comb(L), sphere_comb(L)   node k = (box child k+1, leaf k), k < L; the last node = (leaf L, leaf L-1).  The closest-hit
      traversals test a leaf slot the moment it is entered -- only Box children are ever pushed -- so "leaf k" is a Box child
      whose run is ONE slot, the leaf (a lone-slot step on the device).  After node k, k + 1 leaves are pending: L before the
      first pop, on levels 0..L-1.
  tlas_comb(D)                  the same comb over D + 1 instance leaves.  A TLAS leaf IS an entry (index, count 0), so the leaf
      slots are plain leaf slots.  One ray enters instance leaf D at stack bottom D, then D-1 at D-1, .. , 0 at 0.

What the oracle's rule makes of a comb (expect_comb, expect_two_level): the walker's depth counts the nearest child's push, as
ora_trace's counters[2] does, so a comb of L pending leaves reports min(L + 1, 64).  And the first dropped push of a descent is
the NEAREST child's (the deferred leaf of that node still found room): the chain below is lost and the entry under it is
popped instead.  So a comb ray drops exactly one push when L >= 64 -- and never sees leaves 64..L, which is what makes the rule
observable: rays aimed at those leaves, the nearest ones, report a farther hit than the brute force.

NATURAL TREES: scenes.fractal_corner(4000, 3) (stack levels 26..48) and fractal_corner(8000, 3, octaves=140, top_exp=42) (a
full stack) under the 33 x 25 frame of the diagonal camera; as BLASes under a comb TLAS they are seen through an 11 x 7 frame
mapped through every instance (transforms that are exact in float32: signed axis permutations and power-of-two scales).
On the 140-octave tree the stack fills only where triangles are too small to be hit, so its dropped pushes show in the
counters alone; fractal_corner(16000, 3, octaves=75, top_exp=42, size=0.1) ("dense") under rays aimed at its triangles
fills the stack where a dropped push loses hits: there the records differ from the brute force (fractal, aimed_rays)."""
import numpy as np

import instance_filter_ref as ifr
import instance_motion_ref as imr
import instance_ref as ir
import ray_hits_ref as rh
import sphere_ref as sr

F = np.float32
NODE = np.dtype([("min", "<f4", 3), ("w12", "<u4"), ("max", "<f4", 3), ("w28", "<u4")])
TRIANGLE_PAIR = np.dtype([("v0", "<f4", 3), ("primitive_id_0", "<u4"), ("v1", "<f4", 3), ("primitive_id_1", "<u4"),
                          ("v2", "<f4", 3), ("rotations", "<u2", 2), ("v3", "<f4", 3), ("pad3", "<f4")])
RAY, HIT = rh.RAY, rh.HIT
MISS = 0xFFFFFFFF
BOX, TRI = 1, 2
STACK, LDS_LEVELS = 64, 16
COMB_L = (15, 16, 17, 63, 64, 65, 80)
TWO_LEVEL = ((12, 8), (16, 4), (15, 1), (60, 8), (63, 4), (70, 8))
TAUS = (0.0, 0.5, 1.0, 0.3)
COMB_RAYS = 70                       # the batch ends inside the second wave
AIMED = 8                            # the first rays of a comb batch are aimed at leaves L, L-1, ..
FRAME, SMALL_FRAME = (33, 25), (11, 7)
BIG = 10_000_000                     # the scene-size hint that selects the pair-prefetch instantiations


# ------------------------------------------------------------------ what the oracle's rule makes of a comb
def expect_comb(L):
    """(greatest depth, dropped pushes) of every closest-hit ray on a comb of L pending leaves.  Node k is stepped with k
    entries on the stack: its leaf is pushed (k + 1 entries) and then its nearest child (k + 2), which is popped at once.  With
    k = 63 the leaf takes the last entry and the nearest child's push is dropped: one drop, and the descent ends there."""
    return min(L + 1, STACK), int(L >= STACK)


def expect_two_level(D, B, enter):
    """(greatest depth, dropped pushes, greatest depth inside an instance entered below level 16, pushes dropped inside instances
    entered above level 16) of a closest-hit ray on tlas_comb(D) over tri_comb(B) BLASes; enter[j]: is the instance of TLAS leaf
    j entered.  The TLAS is a comb of D pending leaves; leaf j is then entered at stack bottom min(j, 63) -- at 63 for the leaf
    that survives a dropped descent -- and its BLAS comb of B pending leaves stacks on top of that bottom."""
    depth, dropped = expect_comb(D)
    low = high = 0
    for j in range(min(D, STACK - 1), -1, -1):
        if not enter[j]:
            continue
        inner, d = min(j + B + 1, STACK), int(j + B >= STACK)
        depth, dropped = max(depth, inner), dropped + d
        if j < LDS_LEVELS:
            low = max(low, inner)
        if j > LDS_LEVELS:
            high += d
    return depth, dropped, low, high


# ------------------------------------------------------------------ combs
def _box(nodes, s, half):
    nodes["min"][s], nodes["max"][s] = (-half,) * 3, (half,) * 3


def _comb_nodes(L, half=50.0):
    """slots [0, L]: the one-slot runs of leaves 0..L; the comb's pairs from slot H on.  -> (nodes, root, count)"""
    H = (L + 2) & ~1
    nodes = np.zeros(H + 2 * L, NODE)
    for j in range(L + 1):
        _box(nodes, j, half)
        nodes["w28"][j] = (TRI << 29) | j                     # (w12's count 0: a single triangle)
    for k in range(L):
        a, b = H + 2 * k, H + 2 * k + 1
        _box(nodes, a, half)
        _box(nodes, b, half)
        if k < L - 1:
            nodes["w12"][a], nodes["w28"][a] = 2 << 29, (BOX << 29) | (H + 2 * (k + 1))
        else:
            nodes["w12"][a], nodes["w28"][a] = 1 << 29, (BOX << 29) | L
        nodes["w12"][b], nodes["w28"][b] = 1 << 29, (BOX << 29) | k      # ties go to the larger child index: never this one
    return nodes, H, 2


def _directions(n, rng):
    c = rng.normal(size=(n, 3))
    return c / np.linalg.norm(c, axis=1)[:, None]


def _radii(L):
    """leaf L is the nearest (2), leaf 0 the farthest (8): the leaves a dropped descent loses are the ones a ray meets first"""
    return 8.0 - 6.0 * np.arange(L + 1) / L


def tri_comb(L, seed=5):
    """-> dict(nodes0, nodes1, leaves0, leaves1, root, count, tris0, tris1): L + 1 large triangles around the origin, triangle
    k facing it from direction c[k] at radius _radii; pose 1 has the same words, every corner moved and other (still enclosing)
    boxes"""
    rng = np.random.default_rng(seed + 1000 * L)
    c = _directions(L + 1, rng)
    r = _radii(L)
    tris = np.zeros((L + 1, 3, 3))
    for k in range(L + 1):
        e1 = np.cross(c[k], (0.3, 0.5, 0.8))
        e1 /= np.linalg.norm(e1)
        e2 = np.cross(c[k], e1)
        tris[k] = (c[k] * r[k] - 2 * e1 - 2 * e2, c[k] * r[k] + 3 * e1 - 2 * e2, c[k] * r[k] - 2 * e1 + 3 * e2)
    tris0 = tris.astype(F)
    tris1 = (tris * rng.uniform(0.9, 1.2, (L + 1, 1, 1)) + rng.uniform(-0.3, 0.3, (L + 1, 1, 3))).astype(F)
    nodes0, root, count = _comb_nodes(L)
    nodes1, _, _ = _comb_nodes(L, half=64.0)      # (one box for every slot in pose 1 too: the interpolated fronts still tie)
    out = dict(nodes0=nodes0, nodes1=nodes1, root=root, count=count, tris0=tris0.reshape(-1, 9), tris1=tris1.reshape(-1, 9),
               aim=(c * r[:, None]))
    for key, t in (("leaves0", tris0), ("leaves1", tris1)):
        lv = np.zeros(L + 1, TRIANGLE_PAIR)
        lv["v0"], lv["v1"], lv["v2"], lv["v3"] = t[:, 0], t[:, 1], t[:, 2], t[:, 2]
        lv["primitive_id_0"] = np.arange(L + 1)
        out[key] = lv
    return out


def sphere_comb(L, seed=9):
    """-> dict(nodes, leaves, root, count, spheres): leaf j holds sphere index perm[j]; two leaves hold indices >= num_spheres
    and one sphere has a negative radius (none of the three is among the AIMED nearest leaves)"""
    rng = np.random.default_rng(seed + 1000 * L)
    c = _directions(L + 1, rng)
    r = _radii(L)
    perm = rng.permutation(L + 1)
    spheres = np.zeros((L + 1, 4), F)
    spheres[perm, :3] = c * r[:, None]
    spheres[perm, 3] = rng.uniform(0.8, 1.6, L + 1)
    ids = perm.astype(np.uint32)
    ids[1], ids[L // 2] = L + 1, 0xFFFFFFF0
    spheres[perm[3], 3] = -1.0
    nodes, root, count = _comb_nodes(L)
    leaves = np.zeros(L + 1, TRIANGLE_PAIR)
    leaves["primitive_id_0"] = ids
    return dict(nodes=nodes, leaves=leaves, root=root, count=count, spheres=spheres, aim=c * r[:, None])


def tlas_comb(D, half=50.0, seed=13):
    """-> dict(nodes0, nodes1, leaves, root, count, ids): pair k in slots (2k, 2k + 1) = (box child k + 1, instance leaf k), the
    last pair = (leaf D, leaf D - 1); TLAS leaf j names instance ids[j] (a permutation: a leaf index is no instance id); pose 1
    has the same words and other (still enclosing) boxes"""
    rng = np.random.default_rng(seed + 1000 * D)
    nodes = np.zeros(2 * D, NODE)
    for k in range(D):
        a, b = 2 * k, 2 * k + 1
        _box(nodes, a, half)
        _box(nodes, b, half)
        if k < D - 1:
            nodes["w12"][a], nodes["w28"][a] = 2 << 29, (BOX << 29) | (2 * (k + 1))
        else:
            nodes["w12"][a], nodes["w28"][a] = 1 << 29, (TRI << 29) | D
        nodes["w12"][b], nodes["w28"][b] = 1 << 29, (TRI << 29) | k
    nodes1 = nodes.copy()                          # (one box for every slot in pose 1 too: the interpolated fronts still tie)
    nodes1["min"], nodes1["max"] = nodes["min"] * F(0.75), nodes["max"] * F(0.75)
    ids = rng.permutation(D + 1).astype(np.uint32)
    leaves = np.zeros(D + 1, TRIANGLE_PAIR)
    leaves["primitive_id_0"] = ids
    return dict(nodes0=nodes, nodes1=nodes1, leaves=leaves, root=0, count=2, ids=ids)


def comb_rays(aim, seed, n=COMB_RAYS):
    """n rays from within 0.05 of the origin: the first AIMED ones at the nearest leaves (L, L-1, ..), the others anywhere; four
    have a finite window"""
    rng = np.random.default_rng(seed)
    rays = np.zeros(n, RAY)
    rays["origin"] = rng.uniform(-0.05, 0.05, (n, 3))
    d = rng.normal(size=(n, 3))
    k = min(AIMED, len(aim))
    d[:k] = aim[::-1][:k] - rays["origin"][:k].astype(np.float64) + rng.uniform(-0.05, 0.05, (k, 3))
    rays["dir"] = d
    rays["tmin"], rays["tmax"] = 0.0, np.inf
    rays["tmin"][n - 4:], rays["tmax"][n - 4:] = 0.5, 30.0
    return rays


# ------------------------------------------------------------------ instances
def comb_matrices(K, seed=17):
    """K distinct object_to_world matrices: rotations with power-of-two scales, one mirror, translations below 0.01"""
    rng = np.random.default_rng(seed)
    mats = []
    for k in range(K):
        R = ir.rotation(*rng.uniform(-3, 3, 3)) * 2.0 ** int(rng.integers(-1, 2))
        if k == 2:
            R = R @ np.diag([-1.0, 1.0, 1.0])
        mats.append(np.hstack([R, rng.uniform(-0.01, 0.01, (3, 1))]))
    return mats


def moved_matrices(mats, singular, seed=19):
    """pose 1 of comb_matrices: every instance turned by up to 0.5 rad about a random axis; instance `singular` by a half turn
    about z (its interpolated matrix is singular at time 0.5 and at no other time of TAUS)"""
    rng = np.random.default_rng(seed)
    out = [imr.axis_rotation(rng.normal(size=3), rng.uniform(-0.5, 0.5)) @ np.asarray(M) for M in mats]
    out[singular] = np.diag([-1.0, -1.0, 1.0]) @ np.asarray(mats[singular])
    return out


def exact_matrices(K, one_sided=False):
    """K distinct transforms that are exact in float32, inverse included: a signed axis permutation times a power of two.
    one_sided: at most one sign is negative, so that no instance's octant is the point reflection of another's -- a ray
    aimed through the corner at a small triangle of one instance then meets no other instance's small triangles on its way
    to the corner"""
    perms = [(0, 1, 2), (1, 2, 0), (2, 0, 1), (0, 2, 1), (2, 1, 0), (1, 0, 2)]
    mats = []
    for k in range(K):
        P = np.zeros((3, 3))
        signs = [1 - 2 * ((k >> b) & 1) for b in range(3)]
        if one_sided:
            signs = [-1 if k % 4 == b + 1 else 1 for b in range(3)]
        for row, col in enumerate(perms[k % 6]):
            P[row, col] = signs[row]
        mats.append(np.hstack([P * 2.0 ** ((k % 5) - 2), np.zeros((3, 1))]))
    return mats


def through_instances(rays, mats):
    """every ray of `rays` (object space) as the world ray that instance k maps back onto it, for every k: [K * n] rays"""
    out = []
    for M in mats:
        M = np.asarray(M, np.float64)
        w = rays.copy()
        w["origin"] = rays["origin"].astype(np.float64) @ M[:, :3].T + M[:, 3]
        w["dir"] = rays["dir"].astype(np.float64) @ M[:, :3].T
        out.append(w)
    return np.concatenate(out)


def static_object_rays(rays, records, blas_counts):
    """what the walker's two-level arm needs, from the device's own INSTANCE_RECORDs: (object rays float32 [n, K, 6] through
    instance_ref.object_rays, enterable bool [n, K]: the record is unflagged and names a BLAS with a root run of 1..7 slots)"""
    n, K = len(rays), len(records)
    obj = np.zeros((n, K, 6), F)
    ent = np.zeros((n, K), bool)
    for k in range(K):
        b = int(records["blas"][k])
        ok = int(records["flags"][k]) == 0 and b < len(blas_counts) and 1 <= blas_counts[b] <= 7
        if ok:
            o = ir.object_rays(rays, records["world_to_object"][k].astype(F))
            obj[:, k, :3], obj[:, k, 3:] = o["origin"], o["dir"]
        ent[:, k] = ok
    return obj, ent


def motion_object_rays(rays, times, records, blas_counts):
    """the same from MOTION_INSTANCE_RECORDs, through instance_motion_ref.object_rays: an instance whose interpolated matrix
    cannot be inverted at a ray's time is not enterable for that ray"""
    n, K = len(rays), len(records)
    obj = np.zeros((n, K, 6), F)
    ent = np.zeros((n, K), bool)
    times = np.broadcast_to(np.asarray(times, F), (n,))
    for k in range(K):
        b = int(records["blas"][k])
        if int(records["flags"][k]) == 0 and b < len(blas_counts) and 1 <= blas_counts[b] <= 7:
            o, entered = imr.object_rays(rays, times, records["object_to_world0"][k], records["object_to_world1"][k])
            obj[:, k, :3], obj[:, k, 3:] = o["origin"], o["dir"]
            ent[:, k] = entered
    with np.errstate(invalid="ignore"):
        obj[~ent] = 0
    return obj, ent


def cull_back(records):
    """the walker's per-instance cull word under RT_FILTER_CULL_BACK: the bits swap where the record's 3x3 determinant
    (instance_filter_ref.det_f32) is negative"""
    return np.array([ifr.CULL_FRONT if ifr.det_f32(W) < 0 else ifr.CULL_BACK for W in records["world_to_object"]], np.uint8)


INSTANCE_RECORD = np.dtype([("world_to_object", "<f4", (3, 4)), ("blas", "<u4"), ("flags", "<u4"), ("spare", "<u4", 2)])
MOTION_INSTANCE_RECORD = np.dtype([("object_to_world0", "<f4", (3, 4)), ("object_to_world1", "<f4", (3, 4)), ("blas", "<u4"),
                                   ("flags", "<u4"), ("spare", "<u4", 6)])


def two_level_case(D, B):
    """tlas_comb(D) over D + 1 instances of tri_comb(B) -> dict: tlas, blas (the comb), mats0 / mats1 (object_to_world, two
    poses), blas_of (BLAS table index per instance: 0, and 1 -- an empty tree -- for instance `bad`), `masked` (the instance the
    filtered arm masks out), `singular` (the instance whose motion is singular at time 0.5), rays.  `bad` and `masked` sit on TLAS leaves that a
    ray reaches; the AIMED rays go for the nearest BLAS leaf of the instances entered first (or, past 64 pending leaves, never)"""
    tl = tlas_comb(D)
    K = D + 1
    ids = tl["ids"]
    reach = min(D, STACK - 1)
    mats0 = comb_matrices(K, seed=17 + D)
    blas = tri_comb(B)
    blas_of = np.zeros(K, np.uint32)
    bad, masked, singular = int(ids[reach - 9]), int(ids[reach - 10]), int(ids[reach - 11])
    blas_of[bad] = 1
    aim = np.array([np.asarray(mats0[int(ids[j])])[:, :3] @ blas["aim"][B] + np.asarray(mats0[int(ids[j])])[:, 3]
                    for j in range(D - AIMED + 1, D + 1)])
    return dict(tlas=tl, blas=blas, mats0=mats0, mats1=moved_matrices(mats0, singular, seed=19 + D), blas_of=blas_of, bad=bad,
                masked=masked, singular=singular, rays=comb_rays(aim, seed=23 + D), D=D, B=B)


def host_records(mats, blas_of):
    """INSTANCE_RECORDs as rt_prepare_instances would write them for the CPU test (the GPU test reads the device's own): the
    float64 inverse rounded to float32; flag 1 (a bad BLAS) where blas_of is not 0"""
    rec = np.zeros(len(mats), INSTANCE_RECORD)
    for k, M in enumerate(mats):
        M = np.asarray(M, F).astype(np.float64)
        W3 = np.linalg.inv(M[:, :3])
        rec["world_to_object"][k] = np.hstack([W3, (-W3 @ M[:, 3])[:, None]])
    rec["blas"], rec["flags"] = blas_of, (np.asarray(blas_of) != 0).astype(np.uint32)
    return rec


def host_motion_records(mats0, mats1, blas_of):
    rec = np.zeros(len(mats0), MOTION_INSTANCE_RECORD)
    rec["object_to_world0"], rec["object_to_world1"] = np.asarray(mats0, F), np.asarray(mats1, F)
    rec["blas"], rec["flags"] = blas_of, (np.asarray(blas_of) != 0).astype(np.uint32)
    return rec


def leaf_enter(case, ent_row):
    """expect_two_level's `enter` (by TLAS leaf) from one ray's row of the enterable array (by instance)"""
    return [bool(ent_row[int(case["tlas"]["ids"][j])]) for j in range(case["D"] + 1)]


# ------------------------------------------------------------------ natural trees
AIMED_RAYS = 300
SPHERE_RADIUS = {"deep": 1.0, "full": 0.25, "dense": 0.25}     # of the first edge's length


def fractal(name, scenes):
    """-> (triangles, camera): "deep" reaches stack levels 26..48 and never fills the stack; "full" fills it, but only below
    the scale at which a triangle can still be hit; "dense" (about 1.1 tree levels per octave, against 0.6) fills it some
    twenty octaves above that scale, so that a dropped push loses hits"""
    if name == "deep":
        tris = scenes.fractal_corner(4000, 3)
    elif name == "full":
        tris = scenes.fractal_corner(8000, 3, octaves=140, top_exp=42)
    else:
        tris = scenes.fractal_corner(16000, 3, octaves=75, top_exp=42, size=0.1)
    return tris, scenes.diagonal_camera(2.0 ** -10, 2.0 ** 45)


def aimed_rays(points, cam, n=AIMED_RAYS, seed=7, length=2.0 ** 36, below=None):
    """n rays from the camera's position, each through one of `points` (chosen by seed), with a direction of the given
    length; below: only points nearer the corner than that are chosen.  The frame's rays leave the corner region within
    2^-10 of it and so miss everything much smaller; these meet the small triangles they are aimed at.  The direction's
    length moves the window of testable triangles: Moller-Trumbore's determinant is |direction| * edge^2, which at 2^36
    passes its 1e-9 down to edges of 2^-33, while no product on the 2^42 triangles (2^39 edges) passes 2^124."""
    c = cam[0] if cam.shape else cam
    points = np.asarray(points, np.float64)
    if below is not None:
        points = points[np.linalg.norm(points, axis=1) < below]
    pick = np.random.default_rng(seed).choice(len(points), n, replace=False)
    rays = np.zeros(n, RAY)
    rays["origin"] = c["position"]
    d = points[pick] - rays["origin"].astype(np.float64)
    rays["dir"] = (d * (length / np.linalg.norm(d, axis=1))[:, None]).astype(F)
    rays["tmin"], rays["tmax"] = 0.0, np.inf
    return rays


def fractal_rays(name, tris, cam, frame=FRAME, n=AIMED_RAYS, below=None):
    """the rays of a fractal case: the frame of the diagonal camera; for "dense", rays aimed at triangle centroids"""
    if name == "dense":
        return aimed_rays(np.asarray(tris, F).reshape(-1, 3, 3).mean(axis=1), cam, n, below=below)
    return camera_rays_f32(cam, *frame)


def sphere_rays(name, spheres, cam):
    """the rays of a fractal sphere case: the frame; for "full", also unit-scale rays aimed at sphere centres (the sphere test
    squares the direction, and has no epsilon: a small sphere that a ray meets is hit)"""
    rays = camera_rays_f32(cam, *FRAME)
    if name == "full":
        rays = np.concatenate([rays, aimed_rays(spheres[:, :3], cam, length=1.0)])
    return rays


TWO_LEVEL_FRACTALS = (("deep", "lbvh", 12), ("deep", "sah", 12), ("full", "sah", 30), ("deep", "sah", 30), ("dense", "sah", 30))


def two_level_fractal_rays(name, tris, cam, mats):
    """the small frame -- for "dense", eight rays aimed at triangles below 2^-18 -- mapped through every instance"""
    return through_instances(fractal_rays(name, tris, cam, frame=SMALL_FRAME, n=8, below=2.0 ** -18), mats)


def moved_fractal(tris):
    """pose 1 of a fractal: every triangle scaled about the origin corner by its own factor in [1, 1.03] and pushed outwards"""
    t = tris.reshape(-1, 3, 3).astype(np.float64)
    k = 1.0 + 0.03 * ((np.arange(len(t)) * 0.6180339887) % 1.0)
    return (t * k[:, None, None]).astype(F).reshape(-1, 9)


def fractal_spheres(tris, name="deep"):
    """a sphere at every triangle's centroid with SPHERE_RADIUS[name] times the length of its first edge as radius.  With the
    whole edge every sphere of an octave holds the corner and the SAH tree stays shallow (37 levels on "full"); with a
    quarter of it the spheres are as separate as the triangles and the nesting survives"""
    t = tris.reshape(-1, 3, 3).astype(np.float64)
    r = SPHERE_RADIUS[name] * np.linalg.norm(t[:, 1] - t[:, 0], axis=1)
    return np.ascontiguousarray(np.hstack([t.mean(axis=1), r[:, None]]), F)


def camera_rays_f32(cam, w, h):
    """the primary rays of a w x h frame, one centred sample per pixel, row-major: the ray generator's float32 arithmetic
    restated (ndc = 2 * ((x + 0.5) / w) - 1; p = (ndc.x * u + ndc.y * v) + 1 * w; d = p * (1 / sqrt((px*px + py*py) + pz*pz));
    tmin = 1e-5, tmax = max_depth)"""
    c = cam[0] if cam.shape else cam
    y, x = np.mgrid[0:h, 0:w].astype(F)
    ndcx = (F(2) * ((x + F(0.5)) / F(w)) - F(1)).reshape(-1, 1)
    ndcy = (F(2) * ((y + F(0.5)) / F(h)) - F(1)).reshape(-1, 1)
    u, v, ww = c["u"].astype(F), c["v"].astype(F), c["w"].astype(F)
    p = ((ndcx * u).astype(F) + (ndcy * v).astype(F)).astype(F) + F(1.0) * ww
    inv = F(1.0) / np.sqrt(((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]).astype(F) + p[:, 2] * p[:, 2]).astype(F))
    rays = np.zeros(w * h, RAY)
    rays["origin"], rays["dir"] = c["position"], (p * inv[:, None]).astype(F)
    rays["tmin"], rays["tmax"] = F(0.00001), c["max_depth"]
    return rays


# ------------------------------------------------------------------ brute force (no tree, no stack)
def brute_triangles_t(tris, rays, chunk=64):
    """the smallest accepted t of every ray over all triangles, float32 Moller-Trumbore (ray_hits_ref.mt_f32); +inf: none"""
    T = np.ascontiguousarray(tris, F).reshape(-1, 3, 3)
    m = T.shape[0]
    out = np.full(len(rays), np.inf, F)
    alive = rh.live(rays)
    for s in range(0, len(rays), chunk):
        r = rays[s:s + chunk]
        k = len(r)
        rep = lambda a: np.repeat(a, m, axis=0)
        ok, t, _, _ = rh.mt_f32(np.tile(T[:, 0], (k, 1)), np.tile(T[:, 1], (k, 1)), np.tile(T[:, 2], (k, 1)), rep(r["origin"]),
                                rep(r["dir"]), rep(r["tmin"]), rep(r["tmax"]))
        t = np.where(ok, t, F(np.inf)).reshape(k, m)
        out[s:s + chunk] = t.min(axis=1)
    return np.where(alive, out, F(np.inf))


def brute_leaves_t(leaves, rays, leaves1=None, tau=None):
    """brute_triangles_t over a tree's own leaf records -- A = (v0, v1, v2) and, where v3 != v2, B = (v2, v1, v3), the corners
    in the order the builder left them, which is the order the traversal tests them in (another order rounds t otherwise, and
    near the determinant's epsilon accepts otherwise); with leaves1 and tau, every corner is fl(fl(w0*a) + fl(tau*b))"""
    c = {k: np.asarray(leaves[k], F) for k in ("v0", "v1", "v2", "v3")}
    if leaves1 is not None:
        tau = F(tau)
        w0 = F(1) - tau
        c = {k: ((w0 * v).astype(F) + (tau * np.asarray(leaves1[k], F)).astype(F)).astype(F) for k, v in c.items()}
    return brute_triangles_t(_corners(c), rays)


def _corners(c):
    b = (c["v3"] != c["v2"]).any(axis=1)
    return np.concatenate([np.stack([c["v0"], c["v1"], c["v2"]], axis=1), np.stack([c["v2"], c["v1"], c["v3"]], axis=1)[b]]).reshape(-1, 9)


def leaf_triangles(leaves):
    """the triangles of a tree's leaf records, corners in the records' order, float32 [m, 9]"""
    return _corners({k: np.asarray(leaves[k], F) for k in ("v0", "v1", "v2", "v3")})


def brute_two_level_t(blas_tris, obj, ent, rays):
    """the smallest accepted t of every ray over every enterable instance's triangles, on the walker's own object rays"""
    best = np.full(len(rays), np.inf, F)
    for k in range(obj.shape[1]):
        sel = np.nonzero(ent[:, k])[0]
        if sel.size:
            r = rays[sel].copy()
            r["origin"], r["dir"] = obj[sel, k, :3], obj[sel, k, 3:]
            best[sel] = np.minimum(best[sel], brute_triangles_t(blas_tris[k], r))
    return best


def brute_spheres_t(spheres, rays):
    return sr.dense_f32(rays, spheres)[0]
