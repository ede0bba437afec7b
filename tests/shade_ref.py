"""An independent float64 evaluation of the surface render types (kMaterialID .. kTextureLitShadows, modes 3-8) of the
reference's Tracer.cu, for checking the oracle and the kernels against something other than a second float32 reading
of the same shaders.

It does not use the oracle, a tree, the pair layout or RotateAttributes: the closest hit comes from brute force over
the ORIGINAL triangles (Moller-Trumbore in float64, every triangle against every ray), and the shading uses each
triangle's own corner order -- its v0, v1, v2 and the attribute corners 0, 1, 2 as the caller supplied them.  A pair
tree stores the second triangle as (v2, v1, v3) of the quad with rotated attributes; interpolation, the tangent frame
and the LOD gradients are invariant under that consistent relabelling, so a correct tracer agrees with this evaluation
up to float32 rounding.  What float32 rounding may legitimately change is excluded by the stability mask (below); what
remains is compared with a small per-channel tolerance for the final float -> uchar truncation.

Statements restated (reference src/Tracer.cu): the primary ray (:475-494), HsvToRgb (:15-40), InterpolateUVs /
InterpolateNormals (:42-55), TangentMatrix (:84-101), BilinearSample / TrilinearSample (:122-155), Bump2Normal
(:157-185), RayTriangleGradients / ComputeLOD (:202-254), AmbientShader (:376-469), the mode switch (:526-593); the
range checks of material and texture indices follow the oracle's documented rule (material outside the table ->
material 0, texture index outside the table -> untextured).

Stability mask -- a pixel is excluded when float32 may take a different branch than float64:

* BARY_MARGIN = 2e-4: the closest hit lies within this barycentric distance of an edge of its triangle.  float32
  Moller-Trumbore on coordinates up to ~50 carries barycentric errors of ~1e-6 (a few ulp of the products, divided by
  the cosine of the incidence angle, > 0.05 here): 2e-4 is two orders of magnitude above that.  Near an edge the tracer
  may pick the neighbouring triangle, whose per-corner attributes differ.
* T_REL_MARGIN = 1e-4: another triangle is hit (with the loosened barycentric test) within this relative distance
  of the closest hit -- float32 t carries ~1e-7 relative error.
* LOD_MARGIN = 1e-3: for modes 4, 7, 8 the raw log2 level (ComputeLOD before the clamp) of the texture that is
  sampled at (int)lod lies within this distance of a level boundary 1 .. max_lod.  The LOD of float32 is a difference
  of barycentrics of rays one pixel apart: relative error ~1e-6, i.e. ~1e-6 in log2.
* UV_MARGIN = 1e-4: a sampled uv lies within this distance of an integer (fracf wraps from 1 to 0 and the bilinear
  footprint jumps to the other border of the texture).  uv reach ~10 here: float32 ulp 1e-6.
* UCHAR_MARGIN = 5e-4: an INTERMEDIATE texture sample that feeds further arithmetic (the three bump-map taps, the
  normal-map texel, the texel that becomes the lit diffuse colour) is within this distance of a uchar truncation
  boundary.  One LSB in a bump tap tilts the bump normal by 4 / 256 (Bump2Normal's d = 4): several output LSB.  The
  float32 drift of these samples is measured well below 5e-4 on the test scenes (without this mask one pixel in
  ~40000 differed, by 5).  A trilinear blend that is exactly an integer c (two equal taps) is not masked but read
  both ways: float32 may round w0 * c + w1 * c to just below c, so the comparison accepts a pixel when any of the
  2^MAX_AMBIGUOUS combinations of c / c - 1 for its first MAX_AMBIGUOUS = 3 such texels is within tolerance; a pixel
  with more of them is masked.  A bilinear tap that is exactly an integer (four equal texels) is still masked.
  Final conversions are not masked: the comparison's channel tolerance absorbs them.
* Shadow rays (mode 8): the decision of the brute-force shadow ray flips when the triangle test is loosened by
  BARY_MARGIN or the [tmin, tmax] interval by SHADOW_T_MARGIN = 1e-4 (absolute) + T_REL_MARGIN (relative).

The tests bound the masked fraction per case (MASK_BOUND) and print it.
"""
from __future__ import annotations

import numpy as np

BARY_MARGIN = 2e-4
T_REL_MARGIN = 1e-4
LOD_MARGIN = 1e-3
UV_MARGIN = 1e-4
UCHAR_MARGIN = 5e-4
SHADOW_T_MARGIN = 1e-4
MAX_AMBIGUOUS = 3
CHUNK = 192

MISS = np.array([0, 0, 0, 255], np.uint8)
MAGENTA = np.array([255, 0, 255, 255], np.uint8)


# ------------------------------------------------------------------ small float64 vector helpers (last axis = xyz)
def _dot(a, b):
    return (a * b).sum(axis=-1)


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _normalize(a):
    return a / np.sqrt(_dot(a, a))[..., None]


def _u8(x):
    """float -> uchar as the device converts (truncate, NaN and negatives -> 0, saturate at 255)"""
    x = np.nan_to_num(np.asarray(x, np.float64), nan=-1.0)
    return np.clip(np.floor(x), 0, 255).astype(np.int64)


def _u8_margin(x):
    """distance of a pre-truncation value to the nearest boundary where its uchar changes (inf where saturated)"""
    x = np.asarray(x, np.float64)
    d = np.minimum(x - np.floor(x), np.ceil(x) - x)
    d = np.where(x - np.floor(x) == 0, 0.0, d)
    return np.where((x < -0.5) | (x > 255.5), np.inf, d)


# ------------------------------------------------------------------ brute-force ray casting
def cast(orig, dirs, tris, tmin, tmax):
    """Closest hit of every ray against every triangle, float64.  orig [N, 3] (or [3]), dirs [N, 3], tris [T, 9];
    tmin / tmax scalars or [N].  Returns dict(hit, t, tri, u, v, stable, any_loose, any_strict):
      stable     the closest hit is BARY_MARGIN inside its triangle and no other (loosely tested) triangle lies within
                 T_REL_MARGIN of it, or: nothing is hit even with the loosened test;
      any_loose  some triangle is hit with the test loosened by the margins (barycentric and t);
      any_strict some triangle is hit with the test tightened by them (the two differ where an any-hit decision such
                 as a shadow ray's is unstable)."""
    V = np.asarray(tris, np.float64).reshape(-1, 3, 3)
    v0, e1, e2 = V[:, 0], V[:, 1] - V[:, 0], V[:, 2] - V[:, 0]
    dirs = np.asarray(dirs, np.float64)
    N = dirs.shape[0]
    orig = np.broadcast_to(np.asarray(orig, np.float64), (N, 3))
    tmin = np.broadcast_to(np.asarray(tmin, np.float64), (N,))
    tmax = np.broadcast_to(np.asarray(tmax, np.float64), (N,))
    out = dict(hit=np.zeros(N, bool), t=np.full(N, np.inf), tri=np.full(N, -1, np.int64), u=np.zeros(N), v=np.zeros(N),
               stable=np.ones(N, bool), any_loose=np.zeros(N, bool), any_strict=np.zeros(N, bool))
    m = BARY_MARGIN
    for c0 in range(0, N, CHUNK):
        sl = slice(c0, min(N, c0 + CHUNK))
        d = dirs[sl][:, None, :]
        o = orig[sl][:, None, :]
        h = _cross(d, e2[None])
        a = _dot(e1[None], h)
        with np.errstate(divide="ignore", invalid="ignore"):
            f = 1.0 / a
            s = o - v0[None]
            u = f * _dot(s, h)
            q = _cross(s, e1[None])
            v = f * _dot(d, q)
            t = f * _dot(e2[None], q)
        ok = np.abs(a) > 1e-12
        w = 1.0 - u - v
        edge = np.minimum(np.minimum(u, v), w)
        lo, hi = tmin[sl][:, None], tmax[sl][:, None]
        tm = SHADOW_T_MARGIN + T_REL_MARGIN * np.abs(t)
        exact = ok & (edge >= 0) & (t >= lo) & (t <= hi)
        loose = ok & (edge >= -m) & (t >= lo - tm) & (t <= hi + tm)
        strict = ok & (edge >= m) & (t >= lo + tm) & (t <= hi - tm)
        te = np.where(exact, t, np.inf)
        k = np.argmin(te, axis=1)
        r = np.arange(k.shape[0])
        hit = np.isfinite(te[r, k])
        out["hit"][sl], out["t"][sl], out["tri"][sl] = hit, te[r, k], np.where(hit, k, -1)
        out["u"][sl], out["v"][sl] = u[r, k], v[r, k]
        out["any_loose"][sl], out["any_strict"][sl] = loose.any(axis=1), strict.any(axis=1)
        # closest-hit stability: the nearest loose candidate is the exact hit, deep inside, with no rival nearby
        tl = np.where(loose, t, np.inf)
        tl2 = tl.copy()
        kl = np.argmin(tl, axis=1)
        tl2[r, kl] = np.inf
        second = tl2.min(axis=1)
        first = tl[r, kl]
        st = np.where(hit, (kl == k) & (edge[r, k] >= m) & (second > first * (1 + T_REL_MARGIN) + 1e-12),
                      ~np.isfinite(first))
        out["stable"][sl] = st
    return out


def primary_rays(cam, w, h):
    """TraceRays (:475-494): one centred sample per pixel, float64; returns origin [3], directions [h*w, 3]"""
    c = cam[0] if cam.shape else cam
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    ndcx = 2 * ((x + 0.5) / w) - 1
    ndcy = 2 * ((y + 0.5) / h) - 1
    p = ndcx[..., None] * c["u"].astype(np.float64) + ndcy[..., None] * c["v"].astype(np.float64) + c["w"].astype(np.float64)
    return c["position"].astype(np.float64), _normalize(p.reshape(-1, 3))


# ------------------------------------------------------------------ textures
class _Tex:
    def __init__(self, chain):
        self.mips = [np.ascontiguousarray(m, np.uint32) for m in chain]
        self.max_lod = len(chain) - 1
        self.sx = np.array([m.shape[1] for m in chain])
        self.sy = np.array([m.shape[0] for m in chain])

    def texel(self, ix, iy, lod):
        """Sample(Texture&, int2, lod): coordinates clamped, float4 of the bytes; lod per element"""
        out = np.zeros(ix.shape + (4,))
        for l in np.unique(lod):
            sel = lod == l
            m = self.mips[l]
            xx = np.clip(ix[sel], 0, m.shape[1] - 1)
            yy = np.clip(iy[sel], 0, m.shape[0] - 1)
            px = m[yy, xx]
            out[sel] = np.stack([(px >> np.uint32(8 * c)) & np.uint32(255) for c in range(4)], axis=-1)
        return out

    def bilinear(self, uv, lod):
        """BilinearSample (:122-140) -> (pre-truncation float [K, 4], uchar [K, 4])"""
        lod = np.asarray(lod, np.int64)
        fx, fy = uv[:, 0] - np.floor(uv[:, 0]), uv[:, 1] - np.floor(uv[:, 1])
        cx = fx * self.sx[lod] - 0.5
        cy = self.sy[lod] - (fy * self.sy[lod] - 0.5)
        ix, iy = np.trunc(cx).astype(np.int64), np.trunc(cy).astype(np.int64)
        dx, dy = (cx - ix)[:, None], (cy - iy)[:, None]
        val = (self.texel(ix, iy, lod) * ((1 - dx) * dy) + self.texel(ix + 1, iy, lod) * (dx * dy) +
               self.texel(ix, iy - 1, lod) * ((1 - dx) * (1 - dy)) + self.texel(ix + 1, iy - 1, lod) * (dx * (1 - dy)))
        return val, _u8(val)

    def trilinear(self, uv, lod):
        """TrilinearSample (:142-155) -> (pre-truncation float, uchar, uchar margin, ambiguous): the margin is the
        smallest distance to a truncation boundary of the two bilinear taps and of the blend.  A blend that is exactly
        an integer c with fracf(lod) > 0 (in practice two equal taps, a * (1 - f) + a * f) is `ambiguous`: float32 may
        round it to just below c, so the device has c or c - 1 (Reference tries both).  With fracf(lod) = 0 the blend
        is a * 1 + b * 0 = a in float32 too: exact."""
        lo = np.clip(np.floor(lod).astype(np.int64), 0, self.max_lod)
        hi = np.clip(np.floor(lod).astype(np.int64) + 1, 0, self.max_lod)
        fa, a = self.bilinear(uv, lo)
        fb, b = self.bilinear(uv, hi)
        fr = (lod - np.floor(lod))[:, None]
        val = a * (1 - fr) + b * fr
        mv = _u8_margin(val)
        amb = (fr > 0) & (mv == 0) & (val >= 1) & (val <= 255)
        margin = np.minimum(_u8_margin(fa), np.where(fr > 0, np.minimum(_u8_margin(fb), np.where(amb, np.inf, mv)), np.inf))
        return val, _u8(val), margin, amb


def _uv_near_wrap(uv):
    return (np.abs(uv - np.round(uv)) < UV_MARGIN).any(axis=-1)


# ------------------------------------------------------------------ the shading statements
def _interp(corners, u, v):
    """InterpolateUVs / InterpolateNormals: c0 * (1 - u - v) + c1 * u + c2 * v"""
    return corners[:, 0] * (1 - u - v)[:, None] + corners[:, 1] * u[:, None] + corners[:, 2] * v[:, None]


def _plane_barys(orig, d, V):
    """barycentrics of the ray's hit with the triangle's plane (the u, v formulas of Moller-Trumbore)"""
    e1, e2 = V[:, 1] - V[:, 0], V[:, 2] - V[:, 0]
    s = orig - V[:, 0]
    h = _cross(d, e2)
    f = 1.0 / _dot(e1, h)
    return f * _dot(s, h), f * _dot(d, _cross(s, e1))


def _raw_lod(orig, d, t, spread, V, uvc, u, v, tex_size0):
    """ComputeLOD (:237-254) before the clamp: log2 of the texel footprint of a one-pixel step in x and in y"""
    up = np.array([0.0, 1.0, 0.0])
    x = _normalize(_cross(d, up)) * (t * spread)[:, None]
    y = _normalize(_cross(d, x)) * (t * spread)[:, None]
    hp = orig + d * t[:, None]
    dirx, diry = _normalize(hp + x - orig), _normalize(hp + y - orig)
    uv = _interp(uvc, u, v)
    ux = _interp(uvc, *_plane_barys(orig, dirx, V))
    uy = _interp(uvc, *_plane_barys(orig, diry, V))
    dx, dy = np.abs(ux - uv) * tex_size0, np.abs(uy - uv) * tex_size0
    with np.errstate(divide="ignore"):
        return np.log2(np.maximum(np.sqrt(_dot(dx, dx)), np.sqrt(_dot(dy, dy))))


def _lod_unstable(raw, max_lod):
    k = np.round(raw)
    return (np.abs(raw - k) < LOD_MARGIN) & (k >= 1) & (k <= max_lod)


def _tangent_rows(V, uvc):
    """TangentMatrix (:84-101): rows (tangent.i, bitangent.i, normal.i)"""
    e1, e2 = V[:, 1] - V[:, 0], V[:, 2] - V[:, 0]
    d1, d2 = uvc[:, 1] - uvc[:, 0], uvc[:, 2] - uvc[:, 0]
    f = 1.0 / (d1[:, 0] * d2[:, 1] - d1[:, 1] * d2[:, 0])
    n = _normalize(_cross(e1, e2))
    tg = _normalize(f[:, None] * (e1 * d2[:, 1:2] - e2 * d1[:, 1:2]))
    bt = _normalize(f[:, None] * (e2 * d1[:, 0:1] - e1 * d2[:, 0:1]))
    return np.stack([tg, bt, n], axis=-1)        # [K, 3 rows, 3]: row i = (tg[i], bt[i], n[i])


def _hsv_rgb255(hue):
    """HsvToRgb(h, 1, 1) (:15-40) before the uchar conversion"""
    h = np.clip(hue, 0, 1) * 360.0
    c = 1.0
    x = c * (1 - np.abs((np.trunc(h).astype(np.int64) % 120) / 60.0 - 1))
    z = np.zeros_like(h)
    sector = np.minimum((h // 60).astype(np.int64), 5)
    r = np.choose(sector, [c + z, x, z, z, x, c + z])
    g = np.choose(sector, [x, c + z, c + z, x, z, z])
    b = np.choose(sector, [z, z, x, c + z, c + z, x])
    return np.stack([r, g, b], axis=-1) * 255


class Reference:
    """Float64 frames of one scene seen from one camera.  `frame(mode)` -> (rgba int64 [h, w, 4], mask bool [h, w]
    of stable pixels, hit bool [h, w])."""

    def __init__(self, tris, attributes, materials, textures, light, cam, w, h):
        self.tris = np.asarray(tris, np.float32).reshape(-1, 9)
        self.V = self.tris.astype(np.float64).reshape(-1, 3, 3)
        self.at, self.mats = attributes, materials
        self.tex = [_Tex(c) for c in (textures or [])]
        self.light = np.asarray(light, np.float64)
        self.w, self.h = w, h
        self.orig, self.dirs = primary_rays(cam, w, h)
        self.tmax0 = float(np.float32((cam[0] if cam.shape else cam)["max_depth"]))
        r = cast(self.orig, self.dirs, self.tris, 0.00001, self.tmax0)
        self.hit, self.base_stable = r["hit"], r["stable"]
        i = np.nonzero(self.hit)[0]
        self.idx, self.k = i, r["tri"][i]
        self.t, self.u, self.v = r["t"][i], r["u"][i], r["v"][i]
        self.d = self.dirs[i]
        self.P = self.orig + self.d * self.t[:, None]
        mid = attributes["material_id"][self.k].astype(np.int64)
        self.mid = mid
        mid = np.where((mid >= 0) & (mid < len(materials)), mid, 0)
        M = materials[mid]
        nt = len(self.tex)
        self.m_tex, self.m_bump, self.m_disp = [np.where((M[f] >= 0) & (M[f] < nt), M[f], -1) for f in ("texture", "bump", "disp")]
        self.M = M
        self.nc = attributes["normal"][self.k].astype(np.float64)
        self.uvc = attributes["uv"][self.k].astype(np.float64)
        self.Vk = self.V[self.k]
        self.spread = 2.0 / w
        self._shadow = None
        self._frames = {}

    # -- per-texture helpers over the hit pixels that use texture slot `field`
    def _lod(self, sel, tex_index):
        T = self.tex[tex_index]
        raw = _raw_lod(self.orig, self.d[sel], self.t[sel], self.spread, self.Vk[sel], self.uvc[sel], self.u[sel],
                       self.v[sel], np.array([T.sx[0], T.sy[0]], np.float64))
        return raw, np.clip(raw, 0.0, float(T.max_lod))

    def _frame(self, rgba_hit, unstable_hit, miss_colour):
        out = np.broadcast_to(miss_colour.astype(np.int64), (self.h * self.w, 4)).copy()
        out[self.idx] = rgba_hit
        st = self.base_stable.copy()
        st[self.idx] &= ~unstable_hit
        return out.reshape(self.h, self.w, 4), st.reshape(self.h, self.w), self.hit.reshape(self.h, self.w)

    def frame(self, mode, variant=0):
        """variant (modes 7 / 8): bit j set -> the j-th ambiguous intermediate texel of each pixel is taken as c - 1"""
        key = (mode, variant if mode in (7, 8) else 0)
        if key not in self._frames:
            self._frames[key] = self._frame_uncached(mode, key[1])
        return self._frames[key]

    def _frame_uncached(self, mode, variant):
        K = self.idx.shape[0]
        bad = np.zeros(K, bool)
        if mode == 3:                              # kMaterialID (:526-534)
            rgb = _u8(_hsv_rgb255(self.mid.astype(np.float64) / len(self.mats)))
            return self._frame(np.concatenate([rgb, np.full((K, 1), 255)], axis=1), bad, MISS)
        if mode == 4:                              # kLODs (:543-555)
            out = np.broadcast_to(MAGENTA.astype(np.int64), (K, 4)).copy()
            for ti in np.unique(self.m_tex[self.m_tex >= 0]):
                sel = self.m_tex == ti
                raw, lod = self._lod(sel, ti)
                out[sel] = (np.trunc(lod).astype(np.int64) * 20 % 256)[:, None]
                bad[sel] |= _lod_unstable(raw, self.tex[ti].max_lod)
            return self._frame(out, bad, MAGENTA)
        if mode == 6:                              # kTexture (:556-576)
            out = np.zeros((K, 4), np.int64)
            out[:, :3] = _u8(self.M["diffuse"].astype(np.float64) * 255)
            out[:, 3] = 255
            for ti in np.unique(self.m_tex[self.m_tex >= 0]):
                sel = self.m_tex == ti
                _, lod = self._lod(sel, ti)
                uv = _interp(self.uvc[sel], self.u[sel], self.v[sel])
                out[sel] = self.tex[ti].trilinear(uv, lod)[1]
                bad[sel] |= _uv_near_wrap(uv)
            return self._frame(out, bad, MISS)
        if mode in (5, 7, 8):
            rgb, bad = self._ambient(use_tex=mode != 5, use_shadows=mode == 8, use_bump=mode != 5, variant=variant)
            return self._frame(np.concatenate([rgb, np.full((K, 1), 255)], axis=1), bad, MISS)
        raise ValueError(mode)

    def _ambient(self, use_tex, use_shadows, use_bump, variant=0):
        """AmbientShader (:376-469).  Ambiguous intermediate texels (see _Tex.trilinear) are counted per pixel and
        lowered to c - 1 as the bits of `variant` say; a pixel with more than MAX_AMBIGUOUS of them is masked."""
        K = self.idx.shape[0]
        bad = np.zeros(K, bool)
        n_amb = np.zeros(K, np.int64)

        def resolve(sel, smp, amb):
            si = np.nonzero(sel)[0]
            for ch in range(amb.shape[1]):
                bit = (variant >> np.minimum(n_amb[si], 62)) & 1
                smp[:, ch] -= np.where(amb[:, ch], bit, 0)
                n_amb[si] += amb[:, ch]

        light_colour = np.array([1.0, 0.9, 0.8])
        normal = _interp(self.nc, self.u, self.v)
        uv = _interp(self.uvc, self.u, self.v)
        if use_bump:
            for ti in np.unique(self.m_disp[self.m_disp >= 0]):          # normal map (:388-404)
                sel = self.m_disp == ti
                _, lod = self._lod(sel, ti)
                tbn = _tangent_rows(self.Vk[sel], self.uvc[sel])
                _, smp, margin, amb = self.tex[ti].trilinear(uv[sel], lod)
                resolve(sel, smp, amb[:, :3])
                nrm = _normalize(smp[:, :3] / 255.0 * 2.0 - 1.0)
                normal[sel] = _normalize(np.einsum("kij,kj->ki", tbn, nrm))
                bad[sel] |= _uv_near_wrap(uv[sel]) | (margin[:, :3].min(axis=-1) < UCHAR_MARGIN)
            for ti in np.unique(self.m_bump[(self.m_bump >= 0) & (self.m_disp < 0)]):   # bump map (:406-416)
                sel = (self.m_bump == ti) & (self.m_disp < 0)
                _, lod = self._lod(sel, ti)
                tbn = _tangent_rows(self.Vk[sel], self.uvc[sel])
                T = self.tex[ti]
                ts = 2.0 ** lod
                step = ts[:, None] / np.array([T.sx[0], T.sy[0]], np.float64)
                u0 = uv[sel]
                taps = [u0 - step * 0.5, u0 + np.stack([step[:, 0] * 0.5, 0 * ts], -1), u0 + np.stack([0 * ts, step[:, 1] * 0.5], -1)]
                vals = []
                for tp in taps:
                    _, smp, margin, amb = T.trilinear(tp, lod)
                    resolve(sel, smp, amb[:, :1])
                    vals.append(smp[:, 0].astype(np.float64))
                    bad[sel] |= _uv_near_wrap(tp) | (margin[:, 0] < UCHAR_MARGIN)
                gx, gy = vals[1] - vals[0], vals[2] - vals[0]
                dd = 4.0
                zx, zy = dd * gx / (ts * 256.0), dd * gy / (ts * 256.0)
                bn = _normalize(_cross(np.stack([1 + 0 * zx, 0 * zx, zx], -1), np.stack([0 * zy, 1 + 0 * zy, zy], -1)))
                normal[sel] = _normalize(np.einsum("kij,kj->ki", tbn, bn))
        to_light = self.light - self.P
        L = _normalize(to_light)
        ambient = 0.2 * light_colour
        diffuse = np.maximum(_dot(normal, L), 0.0)[:, None] * light_colour
        refl = -L - 2.0 * normal * _dot(normal, -L)[:, None]
        spec_base = np.maximum(_dot(-self.d, refl), 0.0)
        specular = (spec_base ** self.M["specular_exp"].astype(np.float64))[:, None] * light_colour
        obj_diffuse = self.M["diffuse"].astype(np.float64)
        if use_tex:                                                        # (:432-444): BilinearSample at (int)lod
            obj_diffuse = obj_diffuse.copy()
            for ti in np.unique(self.m_tex[self.m_tex >= 0]):
                sel = self.m_tex == ti
                raw, lod = self._lod(sel, ti)
                fv, smp = self.tex[ti].bilinear(uv[sel], np.trunc(lod).astype(np.int64))
                obj_diffuse[sel] = smp[:, :3] / 255.0
                bad[sel] |= _lod_unstable(raw, self.tex[ti].max_lod) | _uv_near_wrap(uv[sel])
                bad[sel] |= _u8_margin(fv[:, :3]).min(axis=-1) < UCHAR_MARGIN
        if use_shadows:                                                    # (:446-462)
            s = self.shadow()
            diffuse = np.where(s["hit"][:, None], 0.0, diffuse)
            specular = np.where(s["hit"][:, None], 0.0, specular)
            bad |= s["unstable"]
        bad |= n_amb > MAX_AMBIGUOUS
        colour = diffuse * obj_diffuse + ambient * self.M["ambient"].astype(np.float64) + \
            specular * self.M["specular"].astype(np.float64)
        return _u8(np.clip(colour, 0.0, 1.0) * 255), bad

    def shadow(self):
        """brute-force shadow rays from the float64 hit points: tmin 0.001, tmax = distance to the light"""
        if self._shadow is None:
            to_light = self.light - self.P
            dist = np.sqrt(_dot(to_light, to_light))
            r = cast(self.P, to_light / dist[:, None], self.tris, 0.001, dist)
            self._shadow = dict(hit=r["any_loose"] & r["any_strict"], unstable=r["any_loose"] != r["any_strict"])
        return self._shadow


# upper bound on the share of hit pixels the stability mask may exclude, per mode (measured on the test scenes:
# <= 0.4 % in modes 3-6, 3.3-3.6 % in modes 7 and 8, where the intermediate texels of the bump and normal maps add to it)
MASK_BOUND = {3: 0.02, 4: 0.02, 5: 0.02, 6: 0.02, 7: 0.05, 8: 0.05}

TOLERANCE = {
    3: 1,   # HsvToRgb: float32 h = id / 251 * 360 vs float64, then one uchar truncation
    4: 0,   # int(lod) * 20: exact wherever the level is not within LOD_MARGIN of a boundary (masked)
    5: 1,   # one truncation of a smooth float expression (float32 error << 1 LSB)
    6: 1,   # two bilinear truncations blended with weights summing to 1, then one truncation: <= 1 LSB apart
    7: 2,   # the lit diffuse texel (/255) times the light, plus normal-map / bump normals from uchar taps: the final
            # truncation and up to ~1 LSB of float32 drift through the normalisations and the specular pow
    8: 2,   # as 7; the shadow decision itself is masked where it is marginal
}


def compare(frame, ref: Reference, mode, tol=None):
    """Compare an rgba8 frame [h, w, 4] with the float64 reference on its stable pixels.  Returns dict(bad, stable_hit,
    masked_fraction, max_diff, hitmiss_bad): bad = stable pixels out of tolerance (hit or miss)."""
    exp, stable, hit = ref.frame(mode)
    tol = TOLERANCE[mode] if tol is None else tol
    diff = np.abs(frame.astype(np.int64) - exp).max(axis=-1)
    if mode in (7, 8):      # the closest of the c / c - 1 readings of the ambiguous texels
        for variant in range(1, 1 << MAX_AMBIGUOUS):
            diff = np.minimum(diff, np.abs(frame.astype(np.int64) - ref.frame(mode, variant)[0]).max(axis=-1))
    bad = stable & (diff > tol)
    nh = max(int(hit.sum()), 1)
    return dict(bad=bad, n_bad=int(bad.sum()), n_bad_hit=int((bad & hit).sum()), stable_hit=int((stable & hit).sum()),
                masked_fraction=float((hit & ~stable).sum()) / nh, max_diff=int(diff[stable].max()) if stable.any() else 0,
                hits=int(hit.sum()))
