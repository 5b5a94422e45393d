"""TEST INFRASTRUCTURE for tests/test_core_ref_host.py and tests/test_gpu_core_ref.py: the deterministic core of the reference --
instance transform, intersections, closest hit, normals, UVs, texels, camera, shadow rule, fold, mirror recurrence -- restated
in plain numpy from the text of src/rt.rs and src/lin.rs (every function cites its lines) and from DESIGN.md §6 (D4, the
clamped texel index).  Nothing here comes from the oracle, the x86 build of the kernel headers or the C sources; the candidate
rule of mesh triangles is restated here too (the host test holds it equal to vattr_ref._candidates).

Every function takes a dtype.  float64 is the reference the tests hold the code to.  float32 is NOT a second reference: it runs
the same formulas in the reference's operation order with every intermediate rounded to float32, and shows how much error plain
float32 arithmetic carries on them; that figure is printed next to the error of the code under test.

Every function that returns an answer also returns margins, taken from float64 quantities only: how far the discrete
decisions behind the answer are from flipping.  The thresholds the tests apply are the module constants below."""
import numpy as np

E32 = float(np.float32(0.0001))          # const E: f32, src/rt.rs:7 -- the float32 number, whatever the dtype
REL = 1e-3                               # hit / miss, runner-up gap and edge margins: relative
CHORD = 0.05                             # a sphere's half-chord as a share of its radius
# The sign of a length the reference offsets by E itself (the shadow origin hit + E l against the surface it leaves: t = -E or
# t1 = -E) cannot hold REL.  The decision is sound while |q| exceeds the float32 error of its own operands, at most ~10 roundings
# of 2^-24 S (a subtraction, two matrix products, a dot product; S = the magnitudes that enter it) in the worst case and a third of
# that when they add up at random.  SIGN = 16 roundings.
SIGN = 16 * 2.0 ** -24
TEXEL = 1e-3                             # texel units
BOX_P = 1e-3                             # units of p = 2 (hit - pos) / sizes


# ---- src/lin.rs ----------------------------------------------------------------------------------------------------------------
def _a(v, dtype):
    return np.asarray(v, np.float64).astype(dtype)


def dot(a, b):
    """Vec3f * Vec3f, src/lin.rs:259-264: x x + y y + z z, left to right."""
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross(a, b):
    """src/lin.rs:52-58."""
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def norm(a):
    """Vec3f::norm, src/lin.rs:60-66: self * mag().recip()."""
    one = a.dtype.type(1.0)
    with np.errstate(all="ignore"):
        return a * (one / np.sqrt((a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1]) + a[..., 2] * a[..., 2]))[..., None]


def reflect(v, n):
    """Vec3f::reflect, src/lin.rs:68-70: self - n * (2 * (self * n))."""
    return v - n * (v.dtype.type(2.0) * dot(v, n))[..., None]


def rotate_y(dir4, dtype=np.float64):
    """Mat3f::rotate_y, src/lin.rs:175-183: rows (cw, 0, w), (0, 1, 0), (-w, 0, cw) with cw = sqrt(1 - w^2)."""
    d = _a(dir4, dtype)
    w = d[0]
    cw = np.sqrt(dtype(1.0) - w * w)
    return np.array([[cw, 0, w], [0, 1, 0], [-w, 0, cw]], dtype)


def lookat(dir4, dtype=np.float64):
    """Mat4f::lookat(dir, up = (0, 0, 1)), src/lin.rs:197-208: fwd = (x, y, z).norm(), right = fwd x up, normalised, n_up =
    right x fwd; rows (right.x, -right.y, right.z), (-fwd.x, fwd.y, -fwd.z), (n_up.x, -n_up.y, n_up.z)."""
    d = _a(dir4, dtype)
    fwd = norm(d[1:4])
    right = norm(cross(fwd, np.array([0, 0, 1], dtype)))
    up = cross(right, fwd)
    return np.array([[right[0], -right[1], right[2]], [-fwd[0], fwd[1], -fwd[2]], [up[0], -up[1], up[2]]], dtype)


def _mul(m, v):
    """Mat * Vec3f, src/lin.rs:344-365: each row left to right."""
    return np.stack([(m[k, 0] * v[..., 0] + m[k, 1] * v[..., 1]) + m[k, 2] * v[..., 2] for k in range(3)], -1)


class Frame:
    """The transform of Renderer::intersect / normal / to_uv, src/rt.rs:725-733, 776-793, 795-798: rot_y = rotate_y(-dir),
    look = lookat(-dir); a point becomes pos + rot_y (look (p - pos)), a direction rot_y (look d), and the normal goes BACK
    through the same two matrices (not their inverse) before it is normalised."""

    def __init__(self, pos, dir4, dtype):
        self.pos = _a(pos, dtype)
        neg = -np.asarray(dir4, np.float64)
        self.rot, self.look = rotate_y(neg, dtype), lookat(neg, dtype)

    def vec(self, d):
        return _mul(self.rot, _mul(self.look, d))

    def point(self, p):
        return self.pos + self.vec(p - self.pos)


# ---- intersections: (hit, t0, t1, i0, i1, margin, t_pot) ---------------------------------------------------------------------------
# margin: the instance's own hit / miss decision as a multiple of its threshold (>= 1: sound); t_pot: the t0 the instance would
# have if its decision flipped (so that a near miss far behind the winner does not count against the ray).
def _len(v):
    return np.sqrt(np.sum(v * v, -1))


def sphere(o, d, pos, r):
    """Sphere::intersect, src/rt.rs:335-358: disc < 0 -> none; t0 < 0 -> none (a ray from inside has no hit)."""
    T = o.dtype.type
    q = o - pos
    a = dot(d, d)
    b = T(2.0) * dot(q, d)
    c = dot(q, q) - T(r) * T(r)
    disc = b * b - T(4.0) * a * c
    with np.errstate(all="ignore"):
        s = np.sqrt(disc)
        t0 = (-b - s) / (T(2.0) * a)
        t1 = (-b + s) / (T(2.0) * a)
    hit = (disc >= 0) & (t0 >= 0)
    la = np.sqrt(a)
    S = _len(o) + _len(pos) + r
    chord = np.sqrt(np.abs(disc)) / (T(2.0) * a) * la / T(r)
    with np.errstate(all="ignore"):
        margin = np.where(disc >= 0, np.minimum(chord / CHORD, np.abs(t0) * la / S / SIGN), chord / CHORD)
        # a ray that moves away from the centre (q . d > 0) has two negative roots or none: no hit either way, whatever the
        # discriminant says; only the sign of q . d decides (the shadow ray that leaves its own sphere near the terminator)
        margin = np.where(b > 0, (T(0.5) * b) / (S * la) / SIGN, margin)
        t_pot = np.where(disc >= 0, t0, -b / (T(2.0) * a))
    return hit, t0, t1, None, None, margin, t_pot, chord, None


def box(o, d, pos, sizes):
    """Box::intersect, src/rt.rs:299-333: an infinite reciprocal becomes 1/E (either sign); t0 > t1 || t1 < 0 -> none, so a
    negative t0 (the origin inside) is a hit."""
    T = o.dtype.type
    with np.errstate(all="ignore"):
        m = T(1.0) / d
    m = np.where(np.isinf(m), T(1.0) / T(E32), m)
    n = (o - pos) * m
    k = (T(0.5) * sizes) * np.abs(m)
    a, b = -n - k, -n + k
    t0 = np.maximum(np.maximum(a[..., 0], a[..., 1]), a[..., 2])
    t1 = np.minimum(np.minimum(b[..., 0], b[..., 1]), b[..., 2])
    hit = ~((t0 > t1) | (t1 < 0))
    ld = _len(d)
    S = _len(o) + _len(pos) + _len(sizes)
    margin = np.where(t0 > t1, (t0 - t1) * ld / S / REL, np.minimum((t1 - t0) * ld / S / REL, np.abs(t1) * ld / S / SIGN))
    return hit, t0, t1, None, None, margin, t0, None, None


def plane(o, d, pos, n):
    """Plane::intersect, src/rt.rs:400-412: t = -(o . n^ - pos . n^) / (d . n^); t <= 0 -> none."""
    T = o.dtype.type
    nn = norm(n)
    d0 = dot(-nn, pos)
    num = dot(o, nn) + d0
    den = dot(d, nn)
    with np.errstate(all="ignore"):
        t = -num / den
    hit = t > 0
    S = _len(o) + _len(pos)
    # two ways to flip: the numerator changes sign (t passes through 0) or the denominator does (t passes through infinity, so
    # the plane comes or goes at |t|, far behind a nearer winner): the second is returned apart, with the t it acts at
    m_num, m_den = np.abs(num) / S / SIGN, np.abs(den) / _len(d) / REL
    return hit, t, t, None, None, m_num, np.where(hit, t, 0.0), None, (m_den, np.abs(t))


def _triangle(o, d, pos, v0, v1, v2):
    """Triangle::intersect, src/rt.rs:361-398, for rays [n][3] against triangles [m][3]: ([n][m] hit, t, margin)."""
    T = o.dtype.type
    e0, e1 = v1 - v0, v2 - v0
    p = cross(d[:, None, :], e1[None])
    det = dot(e0[None], p)
    reject = (det < T(E32)) & (det > -T(E32))
    with np.errstate(all="ignore"):
        inv = T(1.0) / det
        tv = o[:, None, :] - (v0 + pos)[None]
        u = dot(tv, p) * inv
        q = cross(tv, e0[None])
        v = dot(d[:, None, :], q) * inv
        t = dot(e1[None], q) * inv
        hit = ~reject & ~((u < 0) | (u > 1)) & ~((v < 0) | ((u + v) > 1)) & ~(t < 0)
        inside = np.minimum(np.minimum(u, v), T(1.0) - u - v)
        S = (_len(o) + _len(pos))[:, None] + _len(v0)[None]
        m_det = np.abs(np.abs(det) - E32) / (_len(e0) * _len(e1))[None] / _len(d)[:, None] / REL
        margin = np.minimum(m_det, np.abs(inside) / REL)
        margin = np.where(inside > 0, np.minimum(margin, np.abs(t) * _len(d)[:, None] / S / SIGN), margin)
    return hit, t, np.where(np.isfinite(margin), margin, 0.0)


def triangle(o, d, pos, vtx):
    h, t, m = _triangle(o, d, pos, vtx[None, 0], vtx[None, 1], vtx[None, 2])
    return h[:, 0], t[:, 0], t[:, 0], None, None, m[:, 0], t[:, 0], None, None


def _cells(o_rel, d, tris, pads):
    """The candidate rule of Renderer::intersect_bvh, src/rt.rs:630-723, 742-746, in the words of vattr_ref._candidates, which the
    host test holds it equal to at pad 0 (a triangle is tested when the ray passes the octree leaf of one of its vertices; leaves:
    the 8 x 8 x 8 grid over [-M, M]; a vertex on a leaf boundary lies in both leaves, whose union is a box again), with every leaf
    grown by pad * M: pad = 0 is the rule, +-pad tells whether the answer hangs on a ray grazing a leaf.  [rays][tris] per pad."""
    m = np.abs(tris).reshape(-1, 3).max(0)
    cell = 2.0 * m / 8.0
    g = (tris.reshape(-1, 3) + m) / cell
    lo = -m + np.clip(np.ceil(g) - 1, 0, 7) * cell
    hi = -m + (np.clip(np.floor(g), 0, 7) + 1) * cell
    boxes, back = np.unique(np.concatenate([lo, hi], 1), axis=0, return_inverse=True)
    back = back.reshape(-1, 3)
    out = []
    with np.errstate(all="ignore"):
        inv = 1.0 / d[:, None, :]
        for pad in pads:
            t1, t2 = (boxes[None, :, :3] - pad * m - o_rel[:, None, :]) * inv, (boxes[None, :, 3:] + pad * m - o_rel[:, None, :]) * inv
            tn, tf = np.max(np.minimum(t1, t2), -1), np.min(np.maximum(t1, t2), -1)
            ok = (tn <= tf) & (tf >= 0)
            out.append(ok[:, back[:, 0]] | ok[:, back[:, 1]] | ok[:, back[:, 2]])
    return out


def mesh(o, d, pos, tris):
    """RendererKind::Mesh of Renderer::intersect, src/rt.rs:740-772: the triangles the candidate rule lets the ray test; t0 is
    the FIRST minimum over their hits and t1 the LAST maximum (min_by / max_by), each with its triangle."""
    n = o.shape[0]
    o64, d64, p64, t64 = (np.asarray(x, np.float64) for x in (o, d, pos, tris))
    # rays that pass no leaf at all (the grid's own box, grown like the leaves) test nothing
    M = np.abs(t64).reshape(-1, 3).max(0) * (1 + 2 * REL)
    with np.errstate(all="ignore"):
        a, b = (-M - (o64 - p64)) / d64, (M - (o64 - p64)) / d64
        sub = np.flatnonzero((np.max(np.minimum(a, b), -1) <= np.min(np.maximum(a, b), -1)) & (np.min(np.maximum(a, b), -1) >= 0))
    hit, t0, t1 = np.zeros(n, bool), np.full(n, np.inf, o.dtype), np.full(n, np.inf, o.dtype)
    i0, i1, margin = np.zeros(n, np.int64), np.zeros(n, np.int64), np.full(n, np.inf)
    if sub.size:
        h, t, m = _triangle(o[sub], d[sub], pos, tris[:, 0], tris[:, 1], tris[:, 2])
        cands = _cells(o64[sub] - p64, d64[sub], t64, (0.0, REL, -REL))
        out = []
        for can in cands:
            hh = h & can
            with np.errstate(all="ignore"):
                lo, hi = np.where(hh, t, np.inf), np.where(hh, t, -np.inf)
            j0 = np.argmin(lo, 1)
            j1 = lo.shape[1] - 1 - np.argmax(hi[:, ::-1], 1)
            r = np.arange(lo.shape[0])
            out.append((hh.any(1), lo[r, j0], hi[r, j1], j0, j1))
        stable = np.ones(sub.size, bool)
        for other in out[1:]:
            stable &= (other[0] == out[0][0]) & (~out[0][0] | ((other[3] == out[0][3]) & (other[4] == out[0][4])))
        hit[sub], i0[sub], i1[sub] = out[0][0], out[0][3], out[0][4]
        t0[sub], t1[sub] = np.where(out[0][0], out[0][1], np.inf), np.where(out[0][0], out[0][2], np.inf)
        # every triangle the padded rule lets the ray test must be sound in its own decision: any of them can move t0 or t1
        margin[sub] = np.where(stable, np.min(np.where(cands[1], m, np.inf), 1), 0.0)
    return hit, t0, t1, i0, i1, margin, np.where(hit, t0, -np.inf), None, None


def intersect(rd, frame, o, d):
    """Renderer::intersect, src/rt.rs:725-773, on world rays: the ray goes into the instance's frame, then to its kind."""
    T = o.dtype.type
    no, nd = frame.point(o), frame.vec(d)
    if rd.kind == "sphere":
        return sphere(no, nd, frame.pos, rd.r)
    if rd.kind == "box":
        return box(no, nd, frame.pos, _a(rd.sizes, T))
    if rd.kind == "plane":
        return plane(no, nd, frame.pos, _a(rd.n, T))
    if rd.kind == "triangle":
        return triangle(no, nd, frame.pos, _a(rd.vtx, T))
    return mesh(no, nd, frame.pos, _a(rd.mesh, T))


def frames(render, dtype):
    return [[Frame(p, q, dtype) for p, q in rd.inst] for rd in render.scene.renderer]


def closest_hit(render, o, d, dtype=np.float64, fr=None):
    """RayTracer::closest_hit, src/rt.rs:867-898: the FIRST minimum of t0 over renderers x instances in scene order; a negative
    t0 (a box around the origin) takes part.  Returns a dict: hit, rend, inst (-1: none), t0, t1, i0, i1 (mesh triangles), and
    the float64-only margins `decide` (the smallest own-decision margin of any instance that could change the answer, as a
    multiple of its threshold), `gap` (relative t0 gap to the runner-up), `chord` (the winner's half-chord share, spheres),
    `any_decide` (the same for the shadow verdict: the best hit when blocked, the worst miss when clear)."""
    o, d = _a(o, dtype), _a(d, dtype)
    fr = fr or frames(render, dtype)
    n = o.shape[0]
    best = np.full(n, np.inf, dtype)
    out = {"hit": np.zeros(n, bool), "rend": np.full(n, -1), "inst": np.full(n, -1), "t0": np.full(n, np.inf, dtype), "t1": np.full(n, np.inf, dtype),
           "i0": np.zeros(n, np.int64), "i1": np.zeros(n, np.int64), "chord": np.full(n, np.inf)}
    per = []
    for ri, rd in enumerate(render.scene.renderer):
        for ii, f in enumerate(fr[ri]):
            hit, t0, t1, i0, i1, margin, t_pot, chord, alt = intersect(rd, f, o, d)
            per.append((hit, t0, margin, t_pot, _len(f.pos), alt))
            with np.errstate(invalid="ignore"):
                better = hit & (~out["hit"] | (t0 < best))
            best = np.where(better, t0, best)
            out["hit"] |= hit
            for key, val in (("rend", ri), ("inst", ii), ("t0", t0), ("t1", t1), ("i0", i0), ("i1", i1), ("chord", chord)):
                if val is not None:
                    out[key] = np.where(better, val, out[key])
                elif key == "chord":
                    out[key] = np.where(better, np.inf, out[key])
    # margins
    lo = _len(o) * 1.0
    decide, gap = np.full(n, np.inf), np.full(n, np.inf)
    best_hit, worst_miss = np.zeros(n), np.full(n, np.inf)
    ld = _len(d)
    for hit, t0, margin, t_pot, lp, alt in per:
        S = lo + lp + 1e-30
        with np.errstate(all="ignore"):
            winner = hit & (t0 == best)
            far = np.where(out["hit"], best, np.inf) + REL * S / ld
            # a flip matters when it removes the winner, or brings in an instance in front of it (a hit behind the winner may go)
            matters = winner | (~hit & ~(t_pot > far))
            decide = np.where(matters, np.minimum(decide, margin), decide)
            full = margin
            if alt is not None:
                decide = np.where(winner | (~hit & ~(alt[1] > far)), np.minimum(decide, alt[0]), decide)
                full = np.minimum(margin, alt[0])
            g = np.where(hit & ~winner, (t0 - best) * ld / (np.abs(best) * ld + S), np.inf)
        gap = np.minimum(gap, np.where(np.isnan(g), 0.0, g))
        best_hit = np.where(hit, np.maximum(best_hit, full), best_hit)
        worst_miss = np.where(~hit, np.minimum(worst_miss, full), worst_miss)
    out["decide"], out["gap"] = decide, gap
    out["any_decide"] = np.where(out["hit"], best_hit, worst_miss)
    return out


def tame(h, o, render):
    """The rays whose answer float32 arithmetic cannot flip: decide >= 1 (hit / miss and edges at REL, signs at SIGN, half-chord
    at CHORD), a runner-up gap >= REL, the shadow verdict likewise, |o - instance pos| <= 16."""
    pos = np.array([render.scene.renderer[r].inst[i][0] if r >= 0 else np.zeros(3) for r, i in zip(h["rend"], h["inst"])], np.float64)
    return (h["decide"] >= 1) & (h["gap"] >= REL) & (h["any_decide"] >= 1) & (~h["hit"] | (_len(np.asarray(o, np.float64) - pos) <= 16))


# ---- normals, UVs, texels, material ---------------------------------------------------------------------------------------------------
def _in(x, lo, hi):
    """Range::contains of lo..hi, src/rt.rs:418-419: lo <= x < hi."""
    return (x >= lo) & (x < hi)


def box_face(p):
    """The branch chain shared by Box::normal and Box::uv, src/rt.rs:414-445, 468-516: +x, -x, +y, -y are an else-if chain; the
    z tests FOLLOW it as a separate `if` (`} if`), so a z face overrides whatever the chain chose.  Returns the face 0..5
    (+x -x +y -y +z -z; -1: none), the face Box::uv takes (its chain RETURNS, so z never overrides there), the margins `second` (the distance of the nearest OTHER |p_k| from 1 +- E: edges and
    corners) and `window` (how far inside the E window the face's own coordinate lies, as a share of E), and the sorted distances
    of the three |p_k| from 1."""
    T = p.dtype.type
    e = T(E32)
    pr = [_in(p[..., k], T(1.0) - e, T(1.0) + e) for k in range(3)]
    nr = [_in(p[..., k], T(-1.0) - e, T(-1.0) + e) for k in range(3)]
    face = np.where(pr[0], 0, np.where(nr[0], 1, np.where(pr[1], 2, np.where(nr[1], 3, -1))))
    uv_face = np.where(face >= 0, face, np.where(pr[2], 4, np.where(nr[2], 5, -1)))      # Box::uv RETURNS from the chain: no override
    face = np.where(pr[2], 4, np.where(nr[2], 5, face))
    dist = np.sort(np.abs(np.abs(np.asarray(p, np.float64)) - 1.0), -1)
    return face, uv_face, np.maximum(dist[..., 1] - E32, 0.0), (E32 - dist[..., 0]) / E32, dist


_FACE_N = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [0, 0, 0]], np.float64)


def surface(render, h, o, d, which, dtype=np.float64, fr=None, want_uv=True):
    """Renderer::normal and Renderer::to_uv, src/rt.rs:776-809 with the Normal / UV impls, src/rt.rs:414-542, at the hit point
    o + d t (From<&Ray>, src/rt.rs:193-197) of closest_hit's answer h; which: "t0" | "t1".  Returns (point, unit normal, uv, face,
    margins {"box": second-axis distance in units of p, "window"}).  Triangles and meshes have no UV (todo!(), src/rt.rs:544-548,
    805-807)."""
    o, d = _a(o, dtype), _a(d, dtype)
    T = dtype
    fr = fr or frames(render, dtype)
    n = o.shape[0]
    t = np.where(h["hit"], h[which], 0).astype(dtype)
    p = o + d * t[:, None]
    nrm, uv = np.zeros((n, 3), dtype), np.zeros((n, 2), dtype)
    face = np.full(n, -1)
    mb, mw = np.full(n, np.inf), np.full(n, np.inf)
    chain, dists = np.full(n, -1), np.full((n, 3), np.inf)
    idx = h["i0"] if which == "t0" else h["i1"]
    for ri, rd in enumerate(render.scene.renderer):
        for ii, f in enumerate(fr[ri]):
            k = np.flatnonzero(h["hit"] & (h["rend"] == ri) & (h["inst"] == ii))
            if k.size == 0:
                continue
            nh = f.point(p[k])
            if rd.kind == "sphere":
                raw = nh - f.pos
                v = norm(raw)
                with np.errstate(all="ignore"):
                    uv[k] = np.stack([T(0.5) + T(0.5) * np.arctan2(v[:, 0], -v[:, 1]).astype(dtype) / T(np.float32(np.pi)), T(0.5) - T(0.5) * v[:, 2]], -1)
            elif rd.kind == "plane":
                raw = np.broadcast_to(_a(rd.n, dtype), nh.shape)
                x = nh[:, :2] + T(0.5)
                x = x - np.trunc(x)                                      # f32::fract
                uv[k] = np.where(x < 0, T(1.0) + x, x)
            elif rd.kind == "box":
                q = (nh - f.pos) * (T(1.0) / _a(rd.sizes, dtype) * T(2.0))
                fc, uf, second, window, dist = box_face(q)
                face[k], mb[k], mw[k], chain[k], dists[k] = fc, second, window, uf, dist
                raw = _FACE_N[fc].astype(dtype)
                a, b, c = T(0.5) + T(0.5) * q, T(0.5) - T(0.5) * q, T(1.0) / T(3.0)
                qt, th = T(4.0), T(3.0)
                ux = [a[:, 1] / qt + T(2.0) / qt, b[:, 1] / qt, b[:, 0] / qt + T(3.0) / qt, a[:, 0] / qt + T(1.0) / qt, a[:, 0] / qt + T(1.0) / qt, a[:, 0] / qt + T(1.0) / qt]
                uy = [b[:, 2] / th + c, b[:, 2] / th + c, b[:, 2] / th + c, b[:, 2] / th + c, b[:, 1] / th, a[:, 1] / th + T(2.0) / th]
                sel = np.clip(uf, 0, 5)
                r = np.arange(k.size)
                uv[k] = np.where((uf >= 0)[:, None], np.stack([np.stack(ux, 1)[r, sel], np.stack(uy, 1)[r, sel]], -1), T(0.0))
            else:
                tr = _a(rd.vtx, dtype)[None] if rd.kind == "triangle" else _a(rd.mesh, dtype)[idx[k]]
                raw = cross(tr[:, 1] - tr[:, 0], tr[:, 2] - tr[:, 0])
            with np.errstate(all="ignore"):
                nrm[k] = norm(f.vec(np.broadcast_to(raw, nh.shape)))
    return p, nrm, uv, face, {"box": mb, "window": mw, "chain": chain, "dist": dists}


def texel(tex, uv, dtype=np.float64):
    """Texture::get_color, src/rt.rs:618-628: x = (uv.x * w) as usize, y likewise (`as` truncates, saturates at 0), the texel at
    x + y * w; D4: that flat index is clamped to the last texel where the reference would panic.  Returns (rgb, margin in texel
    units from the nearest texel boundary)."""
    fx, fy = uv[:, 0] * dtype(tex.w), uv[:, 1] * dtype(tex.h)
    with np.errstate(all="ignore"):
        ix, iy = np.maximum(np.trunc(fx), 0).astype(np.int64), np.maximum(np.trunc(fy), 0).astype(np.int64)
    i = np.minimum(ix + iy * tex.w, tex.w * tex.h - 1)
    fx, fy = np.asarray(fx, np.float64), np.asarray(fy, np.float64)
    near = np.minimum(np.abs(fx - np.round(fx)), np.abs(fy - np.round(fy)))
    return _a(tex.dat, dtype).reshape(-1, 3)[i], near


def material(render, h, uv, dtype=np.float64):
    """The six getters, src/rt.rs:811-863, for the hits of h: colour = albedo (x) texel; rough, metal, glass, opacity, emit = the
    map's red channel where there is a map, else the material's scalar.  Returns (dict, texel margin)."""
    n = uv.shape[0]
    out = {"color": np.zeros((n, 3), dtype), "mat_metal": np.zeros(n, dtype)}
    for key in ("rough", "metal", "glass", "opacity", "emit"):
        out[key] = np.zeros(n, dtype)
    near = np.full(n, np.inf)
    for ri, rd in enumerate(render.scene.renderer):
        k = np.flatnonzero(h["hit"] & (h["rend"] == ri))
        if k.size == 0:
            continue
        m = rd.mat
        maps = (m.tex, m.rmap, m.mmap, m.gmap, m.omap, m.emap)
        assert rd.kind in ("sphere", "plane", "box") or all(t is None for t in maps), "Triangle::uv is todo!(), src/rt.rs:544-548"
        out["color"][k] = _a(m.albedo, dtype)
        out["mat_metal"][k] = dtype(m.metal)
        if m.tex is not None:
            c, nr = texel(m.tex, uv[k], dtype)
            out["color"][k] = _a(m.albedo, dtype) * c
            near[k] = np.minimum(near[k], nr)
        for key, t in zip(("rough", "metal", "glass", "opacity", "emit"), maps[1:]):
            out[key][k] = dtype(getattr(m, key))
            if t is not None:
                c, nr = texel(t, uv[k], dtype)
                out[key][k] = c[:, 0]
                near[k] = np.minimum(near[k], nr)
    return out, near


# ---- camera ---------------------------------------------------------------------------------------------------------------------------
def camera_rays(render, dtype=np.float64):
    """RayTracer::iter and ::cast with aprt 0, src/rt.rs:900-954: uv = (aspect (x - w/2) / w, (y - h/2) / h) of the supersampled
    frame (w = res.0 * ssaa, aspect = w / h), dir = (uv.x, 1 / (2 tan(fov / 2)), -uv.y).norm(); the lens point is cam.pos, the
    focus point cam.pos + dir E + dir foc, so new_dir = (that - cam.pos).norm(); the ray leaves cam.pos + D E along D = rot_y
    (look new_dir), with rot_y = rotate_y(cam.dir), look = lookat(cam.dir) (NOT negated).  Returns (o, D), row-major pixels."""
    T = dtype
    fr, cam = render.frame, render.frame.cam
    assert cam.aprt == 0
    f32 = np.float32
    w32, h32 = f32(fr.res[0]) * f32(fr.ssaa), f32(fr.res[1]) * f32(fr.ssaa)
    nw, nh = int(w32), int(h32)
    w, h = T(w32), T(h32)
    yy, xx = np.mgrid[0:nh, 0:nw].astype(dtype)
    aspect = w / h
    tan_fov = np.tan(np.radians(T(0.5) * T(cam.fov))).astype(dtype)
    ux, uy = aspect * (xx - T(0.5) * w) / w, (yy - T(0.5) * h) / h
    d = norm(np.stack([ux, np.full_like(ux, T(1.0) / (T(2.0) * tan_fov)), -uy], -1).reshape(-1, 3))
    pos = _a(cam.pos, T)
    p = (pos + d * T(E32)) + d * T(cam.foc)
    nd = norm(p - pos)
    D = _mul(rotate_y(cam.dir, T), _mul(lookat(cam.dir, T), nd))
    return pos + D * T(E32), D, (nh, nw)


# ---- the path and the fold ------------------------------------------------------------------------------------------------------------
def check_deterministic(render):
    """The conditions under which the reference draws no random number that matters: aprt 0, opacity 1 everywhere, emit 0 or 1."""
    assert render.frame.cam.aprt == 0
    for rd in render.scene.renderer:
        m = rd.mat
        assert m.opacity == 1 and m.omap is None and m.emit in (0.0, 1.0), rd
        assert m.emap is None or np.isin(np.asarray(m.emap.dat)[:, 0], (0.0, 1.0)).all()


def light_dirs(render, p, dtype):
    """l of src/rt.rs:975-978 / 1029-1032 per light, normalised: pos - hit for a point light, -dir.norm() for a directional one."""
    out = []
    for lt in render.scene.light:
        v = _a(lt.v, dtype)
        out.append(norm(v - p) if lt.kind == "point" else norm(np.broadcast_to(-norm(v), p.shape)))
    return out


def render_image(render, dtype=np.float64):
    """One sample of every pixel (aprt 0: every sample is this one): RaytraceIterator::next, src/rt.rs:1014-1065, followed through
    mirror reflections (Ray::reflect, src/rt.rs:559-572, with rand(n, 0) = n.norm(): dir.reflect(n).norm(), origin hit + E dir, pwr
    (1 - loss.min(1)), bounce + 1) while bounce <= rt.bounce, then RayTracer::reduce_light, src/rt.rs:956-994.  Returns a dict:
    img [nh][nw][3], random (the path meets a surface that scatters at random before its last segment), ids (per segment: the
    (renderer, instance) images), vis (per segment, per light: the visibility images), depth (segments that hit), margins
    (decide, gap, texel, box, window, shadow: the minimum over the path's segments and shadow rays), shadow_rays (o, l) of segment
    0, and per segment faces (box face), t0, beyond (per light: shadowed only by something beyond the light); mirror_depth =
    mirror reflections the path makes."""
    check_deterministic(render)
    T = dtype
    fr = frames(render, dtype)
    o, d, (nh, nw) = camera_rays(render, dtype)
    n = o.shape[0]
    sky = render.scene.sky
    alive = np.ones(n, bool)
    random = np.zeros(n, bool)
    pwr = np.ones(n, dtype)
    items, ids, vis, faces, t0s, beyond = [], [], [], [], [], []
    mirror_depth = np.zeros(n, np.int64)
    marg = {k: np.full(n, np.inf) for k in ("decide", "gap", "texel", "box", "window", "shadow")}
    shadow_rays = None
    loss = T(1.0) - min(T(render.rt.loss), T(1.0))
    for seg in range(render.rt.bounce + 1):
        h = closest_hit(render, o, d, dtype, fr)
        h["hit"] &= alive
        p, nrm, uv, face, mb = surface(render, h, o, d, "t0", dtype, fr)
        mat, near = material(render, h, uv, dtype)
        hit = h["hit"]
        for key, val in (("decide", h["decide"]), ("gap", h["gap"])):
            marg[key] = np.where(alive, np.minimum(marg[key], val), marg[key])
        for key, val in (("texel", near), ("box", mb["box"]), ("window", mb["window"])):
            marg[key] = np.where(hit, np.minimum(marg[key], val), marg[key])
        ids.append((np.where(hit, h["rend"], -1).reshape(nh, nw), np.where(hit, h["inst"], -1).reshape(nh, nw)))
        ls = light_dirs(render, p, dtype)
        seen, far = [], []
        faces.append(np.where(hit, face, -1)); t0s.append(np.where(hit, h["t0"], np.inf))
        for lt, l in zip(render.scene.light, ls):
            so = p + l * T(E32)                       # Ray::cast_default(hit, l.norm()), src/rt.rs:1034, 555-557
            sh = closest_hit(render, so, l, dtype, fr)
            seen.append(hit & ~sh["hit"])
            # blocked by nothing in front of a point light: the occluder lies beyond it (no distance limit, src/rt.rs:1036)
            far.append(hit & sh["hit"] & (lt.kind == "point") & (np.asarray(sh["t0"], np.float64) > _len(np.asarray(_a(lt.v, T) - p, np.float64))))
            marg["shadow"] = np.where(hit & (mat["emit"] != 1), np.minimum(marg["shadow"], sh["any_decide"]), marg["shadow"])
            if seg == 0:
                shadow_rays = (shadow_rays or []) + [(so[hit], l[hit])]
        vis.append([s.reshape(nh, nw) for s in seen])
        beyond.append(far)
        items.append((hit.copy(), d.copy(), nrm, mat, ls, seen, pwr.copy()))
        # the path ends the fold at an emitter (its colour replaces everything behind it), so what follows one is never seen
        emitter = hit & (mat["emit"] == 1)
        mirror = (mat["mat_metal"] != 0) & (mat["rough"] == 0)
        if seg < render.rt.bounce:
            random |= hit & ~emitter & ~mirror
        alive = hit & ~emitter & mirror
        if seg < render.rt.bounce:
            mirror_depth += alive
        with np.errstate(all="ignore"):
            nd = norm(reflect(d, norm(nrm)))
        o = np.where(alive[:, None], p + nd * T(E32), o)                          # Ray::cast, src/rt.rs:551-553
        d = np.where(alive[:, None], nd, d)
        pwr = pwr * loss
    # reduce_light, src/rt.rs:956-994
    first = items[0][0]
    col = np.broadcast_to(_a(sky.color, T) * T(sky.pwr), (n, 3)).copy()
    for hit, rd_, nrm, mat, ls, seen, pw in reversed(items):
        l_col = np.zeros((n, 3), dtype)
        for lt, l, s in zip(render.scene.light, ls, seen):
            with np.errstate(all="ignore"):
                diff = np.maximum(dot(l, nrm), T(0.0))
                sp = np.maximum(dot(rd_, reflect(l, nrm)), T(0.0))
                spec = sp
                for _ in range(5):                                       # powi(32)
                    spec = spec * spec
                spec = spec * (T(1.0) - mat["rough"])
                o_col = mat["color"] * (T(1.0) - mat["metal"])[:, None]
                term = ((o_col * diff[:, None]) * _a(lt.color, T) + spec[:, None]) * T(lt.pwr)
            l_col = l_col + np.where(s[:, None], term, T(0.0))
        d_col = T(0.5) * col + mat["color"] * col
        new = np.where((mat["emit"] == 1)[:, None], mat["color"], (d_col + l_col) * pw[:, None])
        col = np.where(hit[:, None], new, col)
    img = np.where(first[:, None], col, _a(sky.color, T))
    depth = np.sum([it[0] for it in items], 0)
    return {"img": img.reshape(nh, nw, 3), "random": random.reshape(nh, nw), "ids": ids, "vis": vis, "depth": depth.reshape(nh, nw),
            "margins": {k: v.reshape(nh, nw) for k, v in marg.items()}, "shadow_rays": shadow_rays, "items": items, "shape": (nh, nw),
            "faces": faces, "t0": t0s, "beyond": beyond, "mirror_depth": mirror_depth.reshape(nh, nw)}


def ray_words(render, o, d, dtype=np.float64):
    """The ray query of the float64 core on rays as given (no shift, no normalisation): closest_hit, then the normal at t0.
    Returns (closest_hit's dict + "normal", tame mask)."""
    h = closest_hit(render, o, d, dtype)
    _, nrm, _, face, mb = surface(render, h, o, d, "t0", dtype)
    h["normal"], h["face"], h["box"], h["window"], h["chain"], h["dist"] = nrm, face, mb["box"], mb["window"], mb["chain"], mb["dist"]
    ok = tame(h, o, render) & (~h["hit"] | ((mb["box"] >= BOX_P) & (mb["window"] >= 0.5)))
    return h, ok
