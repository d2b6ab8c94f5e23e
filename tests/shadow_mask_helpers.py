"""Helpers of the shadow-mask tests: the light sample's shadow segment and the kernels' primitive tests restated in
numpy float32, operation for operation (csrc/nh_shade.h emitter_sample, csrc/nh_traverse.h trace / tri_test_nb /
sphere_test), and float64 versions of the same tests with a tolerance. Arrays of float32 keep every numpy operation a
single IEEE single-precision operation, as the kernels are built (no contraction)."""
import numpy as np

from primary_mask_records import is_sphere

F = np.float32
EPS = F(1e-4)  # kEps (csrc/nh_device.h)


def _dot32(a, b):
    """nhd::dot: a.x * b.x + (a.y * b.y + a.z * b.z)"""
    return a[..., 0] * b[..., 0] + (a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2])


def _cross32(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _normalized32(a):
    n = _dot32(a, a)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where((n > 0)[..., None], a / np.sqrt(n)[..., None], a)


def face_normals32(faces):
    """emit_face_kernel: normalized(cross(p1 - p0, p2 - p0)) per face, float32. faces: (n, 9)."""
    f = np.asarray(faces, F).reshape(-1, 3, 3)
    return _normalized32(_cross32(f[:, 1] - f[:, 0], f[:, 2] - f[:, 0]))


def face_points32(faces, rng, n_random):
    """Per face its three corners and n_random points bu p0 + bv p1 + bw p2 as Mesh::sampleSurface forms them (float32).
    Returns (points (m, 3), face index (m,))."""
    f = np.asarray(faces, F).reshape(-1, 3, 3)
    pts, idx = [], []
    for i, (p0, p1, p2) in enumerate(f):
        bary = [(F(1), F(0), F(0)), (F(0), F(1), F(0)), (F(0), F(0), F(1))]
        for _ in range(n_random):
            sx, sy = F(rng.random()), F(rng.random())
            su1 = np.sqrt(sx)
            bu = F(1) - su1
            bv = sy * su1
            bary.append((bu, bv, F(1) - bu - bv))
        for bu, bv, bw in bary:
            pts.append((bu * p0 + bv * p1) + bw * p2)
            idx.append(i)
    return np.array(pts, F), np.array(idx)


def shadow_segments32(p, n, ref):
    """emitter_sample's shadow ray from light point p (normal n) to ref, all (m, 3) float32: (so, sd, mint, maxt, traced).
    traced: the kernel queries it -- dot(n, -wi) >= 0 and a finite direction."""
    p, n, ref = np.asarray(p, F), np.asarray(n, F), np.asarray(ref, F)
    pr = p - ref
    wi = _normalized32(pr)
    sd = -wi
    maxt = np.sqrt(_dot32(pr, pr)) - EPS
    traced = (_dot32(n, sd) >= 0) & np.isfinite(sd).all(axis=-1) & (_dot32(pr, pr) > 0)
    # trace(): the adaptive epsilon
    mint = np.maximum(EPS, EPS * np.abs(p).max(axis=-1)).astype(F)
    return p, sd, mint, maxt.astype(F), traced


def accepts32(rec, o, d, mint, maxt):
    """(m,) bool: tri_test_nb / sphere_test of record rec (12 float32) accepts the rays, in float32."""
    r = np.asarray(rec, F)
    with np.errstate(all="ignore"):
        if is_sphere(r):
            L = o - r[0:3]
            qa = _dot32(d, d)
            qb = F(2) * _dot32(d, L)
            qc = _dot32(L, L) - r[3] * r[3]
            discr = qb * qb - (F(4) * qa) * qc
            s = np.sqrt(discr)
            tmin = ((-qb - s) / F(2)) / qa
            tmax = ((-qb + s) / F(2)) / qa
            return ~(discr < 0) & (((mint <= tmin) & (maxt >= tmin)) | ((mint <= tmax) & (maxt >= tmax)))
        p0 = r[0:3]
        e1, e2 = r[4:7] - p0, r[8:11] - p0
        pvec = _cross32(d, e2[None, :])
        det = _dot32(e1[None, :], pvec)
        inv = F(1) / det
        tvec = o - p0
        u = _dot32(tvec, pvec) * inv
        qvec = _cross32(tvec, e1[None, :])
        v = _dot32(d, qvec) * inv
        t = _dot32(e2[None, :], qvec) * inv
        ok_det = ~((det > F(-1e-8)) & (det < F(1e-8)))
        ok_u = ~((u < 0) | (u > 1))
        ok_v = ~((v < 0) | (u + v > 1))
        assert inv.dtype == F and t.dtype == F and u.dtype == F and v.dtype == F
        return ok_det & ok_u & ok_v & (t >= mint) & (t <= maxt)


def meets64(rec, o, d, mint, maxt, tol):
    """(m,) bool: in float64 the ray o + t d, t in [mint - tol, maxt + tol], comes within about tol of the record."""
    r = np.asarray(rec, np.float64)
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    mint, maxt = np.asarray(mint, np.float64) - tol, np.asarray(maxt, np.float64) + tol
    with np.errstate(all="ignore"):
        if is_sphere(rec):
            L = o - r[0:3]
            qa, qb, qc = (d * d).sum(-1), 2.0 * (d * L).sum(-1), (L * L).sum(-1) - (r[3] + tol) ** 2
            disc = qb * qb - 4.0 * qa * qc
            s = np.sqrt(np.maximum(disc, 0.0))
            t0, t1 = (-qb - s) / (2 * qa), (-qb + s) / (2 * qa)
            return (disc >= 0) & (((t0 >= mint) & (t0 <= maxt)) | ((t1 >= mint) & (t1 <= maxt)))
        p0, e1, e2 = r[0:3], r[4:7] - r[0:3], r[8:11] - r[0:3]
        pvec = np.cross(d, e2)
        det = pvec @ e1
        u = ((o - p0) * pvec).sum(-1) / det
        qvec = np.cross(o - p0, e1)
        v = (d * qvec).sum(-1) / det
        t = (qvec @ e2) / det
        tu, tv = tol / np.linalg.norm(e1), tol / np.linalg.norm(e2)
        return (det != 0) & (u >= -tu) & (v >= -tv) & (u + v <= 1 + max(tu, tv)) & (t >= mint) & (t <= maxt)


def first_hits64(records, o, d):
    """The closest hit of rays (o, d) (m, 3) over the records in float64: (found (m,), point (m, 3))."""
    best = np.full(len(d), np.inf)
    for k, rec in enumerate(records):
        r = rec.astype(np.float64)
        with np.errstate(all="ignore"):
            if is_sphere(rec):
                L = o - r[0:3]
                qa, qb, qc = (d * d).sum(-1), 2.0 * (d @ L), L @ L - r[3] * r[3]
                disc = qb * qb - 4.0 * qa * qc
                s = np.sqrt(np.maximum(disc, 0.0))
                t0, t1 = (-qb - s) / (2 * qa), (-qb + s) / (2 * qa)
                t = np.where(t0 > 1e-6, t0, t1)
                ok = (disc >= 0) & (t > 1e-6)
            else:
                p0, e1, e2 = r[0:3], r[4:7] - r[0:3], r[8:11] - r[0:3]
                pvec = np.cross(d, e2)
                det = pvec @ e1
                u = (pvec @ (o - p0)) / det
                qvec = np.cross(o - p0, e1)
                v = (d @ qvec) / det
                t = (e2 @ qvec) / det
                ok = (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 1e-6)
        best = np.where(ok & (t < best), t, best)
    found = np.isfinite(best)
    return found, o + np.where(found, best, 0.0)[:, None] * d


def scene_box(records):
    """(lo, hi) of the records' boxes, float64."""
    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
    for rec in records:
        a, b = record_box(rec)
        lo, hi = np.minimum(lo, a), np.maximum(hi, b)
    return lo, hi


def record_box(rec):
    r = rec.astype(np.float64)
    if is_sphere(rec):
        return r[0:3] - r[3], r[0:3] + r[3]
    pts = np.stack([r[0:3], r[4:7], r[8:11]])
    return pts.min(0), pts.max(0)
