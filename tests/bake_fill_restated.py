"""numpy restatement of the atlas completion (include/lasr_ops.h: lasr_bake_mirror / lasr_bake_blend, DESIGN.md 4.11 "Fill"), written
from the header text, and the fixtures tests/test_bake_fill_cpu.py and tests/test_bake_fill_gpu.py share.  The fill is this
project's own addition, so this file is what the kernels are checked against: the blend in float32 with the stated operation
order (the device result must equal it bit for bit), the mirror in float64 and in float32."""
import functools

import numpy as np

import bake_restated as br

EDGE_ENDS = ((1, 2), (2, 0), (0, 1))                   # face edge k lies opposite corner k: from corner p to corner q
FAR, NORMAL, UNSEEN, NO_FACE = 0, 1, 2, 3               # src = -1 - reason
KEEP, PULL = 1. - 2. ** -20, 2. ** -20 / 3.             # b' = b KEEP + PULL: the closest point pulled towards the face centroid


# ---- adjacency ----------------------------------------------------------------------------------------------------------------------
def face_neighbours(faces, num_verts=None):
    """nbr [F,3]: (g * 3 + k') * 2 + same, or -1 (an edge without exactly two faces; a face with a repeated or out-of-range index)."""
    faces = np.asarray(faces)
    F = faces.shape[0]
    good = [(min(t) >= 0 and (num_verts is None or max(t) < num_verts) and len(set(t)) == 3) for t in faces.tolist()]
    edges = {}
    for f in range(F):
        if good[f]:
            for k, (p, q) in enumerate(EDGE_ENDS):
                a, b = int(faces[f, p]), int(faces[f, q])
                edges.setdefault((min(a, b), max(a, b)), []).append((f, k, a))
    nbr = -np.ones((F, 3), np.int64)
    for users in edges.values():
        if len(users) == 2:
            (f, k, a), (g, k2, a2) = users
            same = int(a == a2)
            nbr[f, k] = (g * 3 + k2) * 2 + same
            nbr[g, k2] = (f * 3 + k) * 2 + same
    return nbr


def _lower(ix, iy, R):
    return iy * R + ix


def _upper(cx, cy, R):
    return (R - 1 - cy) * R + (R - 1 - cx)


def _across(nbr, f, k, s, F, R):
    code = int(nbr[f, k])
    if code < 0 or code // 6 >= F:
        return -1
    g, k2, same = code // 6, (code // 2) % 3, code & 1
    s2 = s if same else R - 1 - s
    ix, iy = ((0, R - 1 - s2), (s2, 0), (R - 1 - s2, s2))[k2]
    return g * R * R + _lower(ix, iy, R)


def texel_neighbours(nbr, R):
    """[F*R*R, 3]: the texel index of n0, n1, n2 of every texel, or -1."""
    F, RR = nbr.shape[0], R * R
    out = -np.ones((F * RR, 3), np.int64)
    for f in range(F):
        for j in range(RR):
            iy, ix = divmod(j, R)
            if ix + iy <= R - 1:
                n = (f * RR + _upper(ix - 1, iy, R) if ix >= 1 else _across(nbr, f, 0, R - 1 - iy, F, R),
                     f * RR + _upper(ix, iy - 1, R) if iy >= 1 else _across(nbr, f, 1, ix, F, R),
                     f * RR + _upper(ix, iy, R) if ix + iy <= R - 2 else _across(nbr, f, 2, iy, F, R))
            else:
                cx, cy = R - 1 - ix, R - 1 - iy
                n = (f * RR + _lower(cx + 1, cy, R), f * RR + _lower(cx, cy + 1, R), f * RR + _lower(cx, cy, R))
            out[f * RR + j] = n
    return out


def blend(textures, fixed, nbr, R, iters, dtype=np.float32):
    """`iters` Jacobi iterations: out = (((0 + n0) + n1) + n2) / count over the neighbours that exist; fixed texels and texels
    without a neighbour keep their value.  textures [F,R*R,3] -> the same shape in `dtype`."""
    F = nbr.shape[0]
    cur = np.asarray(textures, dtype).reshape(F * R * R, 3).copy()
    tn = texel_neighbours(nbr, R)
    has = tn >= 0
    count = has.sum(1)
    move = (np.asarray(fixed).reshape(-1) == 0) & (count > 0)
    div = np.maximum(count, 1).astype(dtype)[:, None]
    for _ in range(int(iters)):
        s = np.zeros_like(cur)
        for k in range(3):
            s = np.where(has[:, k, None], s + cur[np.maximum(tn[:, k], 0)], s)
        cur = np.where(move[:, None], s / div, cur)
    return cur.reshape(F, R * R, 3)


# ---- mirror -------------------------------------------------------------------------------------------------------------------------
def _dot(u, v):
    return u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1] + u[..., 2] * v[..., 2]


def point_triangle(p, a, b, c):
    """csrc/point_triangle.h in the dtype of its arguments (broadcast over leading axes): -> d2, (w0, w1, w2)."""
    dt = p.dtype.type
    ab, ac, ap, bp, cp = b - a, c - a, p - a, p - b, p - c
    d1, d2, d3, d4, d5, d6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
    va, vb, vc = d3 * d6 - d5 * d4, d5 * d2 - d1 * d6, d1 * d4 - d3 * d2
    eps, one, zero = dt(1e-12), dt(1), dt(0)
    shape = np.broadcast(d1, d1).shape
    best = dict(d2=np.full(shape, np.inf, p.dtype), w=[np.full(shape, v, p.dtype) for v in (1, 0, 0)])

    def consider(w0, w1, w2, mask=True):
        q = w0[..., None] * a + w1[..., None] * b + w2[..., None] * c - p
        e = zero + q[..., 0] * q[..., 0] + q[..., 1] * q[..., 1] + q[..., 2] * q[..., 2]
        upd = (e < best['d2']) & mask
        best['d2'] = np.where(upd, e, best['d2'])
        best['w'] = [np.where(upd, n, o) for n, o in zip((w0, w1, w2), best['w'])]

    den = np.maximum(va + vb + vc, eps)
    v, w = vb / den, vc / den
    consider(one - v - w, v, w, (va >= 0) & (vb >= 0) & (vc >= 0))
    clamp = lambda x: np.minimum(np.maximum(x, zero), one)                          # noqa: E731
    tab = clamp(d1 / np.maximum(d1 - d3, eps))
    tac = clamp(d2 / np.maximum(d2 - d6, eps))
    tbc = clamp((d4 - d3) / np.maximum((d4 - d3) + (d5 - d6), eps))
    z = np.zeros(shape, p.dtype)
    consider(one - tab, tab, z)
    consider(one - tac, z, tac)
    consider(z, one - tbc, tbc)
    return best['d2'], best['w']


def source_texel(b0, b1, R):
    """j' = surface_texel(b0', b1', R), b' = b (1 - 2^-20) + 2^-20 / 3, in the dtype of b0."""
    dt = type(b0)
    return br.surface_texel(b0 * dt(KEEP) + dt(PULL), b1 * dt(KEEP) + dt(PULL), R)


def sample_points(rest, faces, texels, R, dtype):
    """The centroid sample points p [M,3] of the listed texels on the rest mesh, in `dtype`."""
    c0, c1, _ = br.centroids(R)
    c0, c1 = c0.astype(dtype), c1.astype(dtype)
    if dtype == np.float32:                                                        # the kernel's own float32 expressions
        j = np.arange(R * R)
        iy, ix = j // R, j % R
        low = ix + iy <= R - 1
        inv, third, two = np.float32(1) / np.float32(R), np.float32(1) / np.float32(3), np.float32(2) / np.float32(3)
        c0 = np.where(low, (ix.astype(np.float32) + third) * inv, ((R - 1 - ix).astype(np.float32) + two) * inv)
        c1 = np.where(low, (iy.astype(np.float32) + third) * inv, ((R - 1 - iy).astype(np.float32) + two) * inv)
    c2 = dtype(1) - c0 - c1
    f, j = np.asarray(texels) // (R * R), np.asarray(texels) % (R * R)
    tri = np.asarray(rest, dtype)[np.asarray(faces)[f]]                            # M,3,3
    return c0[j, None] * tri[:, 0] + c1[j, None] * tri[:, 1] + c2[j, None] * tri[:, 2]


def normals(rest, faces, dtype):
    tri = np.asarray(rest, dtype)[np.asarray(faces)]
    e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    return np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                     e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)


def mirror(rest, faces, texels, weight, R, axis, max_d2, dtype=np.float64):
    """-> dict(src [M] (g R R + j' or -1 - reason), d2 [M], g [M], all_d2 [M,F], all_w [M,F,2] (b0, b1 of every face's closest
    point; inf / 0 for faces that take no part), dots [M] (n(f)' . n(g), nan where there is no g))."""
    rest, faces, texels = np.asarray(rest, dtype), np.asarray(faces), np.asarray(texels)
    V, F, RR, M = rest.shape[0], faces.shape[0], R * R, texels.shape[0]
    valid = ((faces >= 0) & (faces < V)).all(1)
    safe = np.where(valid[:, None], faces, 0)
    inlist = (texels >= 0) & (texels < F * RR)
    tl = np.where(inlist, texels, 0)
    live = inlist & valid[tl // RR]
    p = sample_points(rest, safe, tl, R, dtype)
    p[:, axis] = -p[:, axis]
    tri = rest[safe]
    all_d2, w = point_triangle(p[:, None, :], tri[None, :, 0], tri[None, :, 1], tri[None, :, 2])
    all_d2 = np.where(valid[None, :] & live[:, None], all_d2, np.inf)
    g = np.where(np.isfinite(all_d2).any(1), all_d2.argmin(1), -1)                 # argmin: the first, i.e. lowest, index
    rows = np.arange(M)
    d2 = np.where(g >= 0, all_d2[rows, np.maximum(g, 0)], np.inf).astype(dtype)
    n = normals(rest, safe, dtype)
    nf = n[tl // RR].copy()
    nf[:, axis] = -nf[:, axis]
    ng = n[np.maximum(g, 0)]
    dots = np.where(g >= 0, nf[:, 0] * ng[:, 0] + nf[:, 1] * ng[:, 1] + nf[:, 2] * ng[:, 2], np.nan)
    weight = np.asarray(weight).reshape(F, RR)
    src = np.empty(M, np.int64)
    for m in range(M):
        if g[m] < 0:
            src[m] = -1 - NO_FACE
        elif not d2[m] <= max_d2:
            src[m] = -1 - FAR
        elif not dots[m] > 0:
            src[m] = -1 - NORMAL
        else:
            j = min(max(source_texel(w[0][m, g[m]], w[1][m, g[m]], R), 0), RR - 1)
            src[m] = g[m] * RR + j if weight[g[m], j] > 0 else -1 - UNSEEN
    return dict(src=src, d2=d2, g=g, all_d2=all_d2, all_w=np.stack([w[0], w[1]], 2), dots=dots)


def region_violation(b0, b1, j, R):
    """How far outside the region of texel j the point (b0, b1) lies, in cell widths (0 inside): the largest of its distances to
    the three half planes that bound the region."""
    x, y = b0 * R, b1 * R
    iy, ix = divmod(int(j), R)
    if ix + iy <= R - 1:
        u, v = x - ix, y - iy
    else:
        u, v = (R - ix) - x, (R - iy) - y                                          # upper triangle of cell (R-1-ix, R-1-iy), turned
    return max(-u, -v, (u + v - 1.) / np.sqrt(2.), 0.)


# ---- fixtures -----------------------------------------------------------------------------------------------------------------------
def grid_case(seed=3, n=4):
    """An n x n planar grid of unit quads split into 2 n^2 triangles, every face with a seeded random corner rotation and winding
    (so that both `same` values occur).  verts float32 [(n+1)^2, 3], faces int64."""
    rng = np.random.default_rng(seed)
    vid = lambda x, y: y * (n + 1) + x                                              # noqa: E731
    verts = np.array([[x, y, 0.] for y in range(n + 1) for x in range(n + 1)], np.float32)
    faces = []
    for y in range(n):
        for x in range(n):
            for t in ([vid(x, y), vid(x + 1, y), vid(x + 1, y + 1)], [vid(x, y), vid(x + 1, y + 1), vid(x, y + 1)]):
                t = np.roll(t, int(rng.integers(3)))
                faces.append(t[::-1] if rng.integers(2) else t)
    return verts, np.asarray(faces, np.int64)


def sphere_case():
    from lasr_amd import synth
    v, f = synth.geodesic_sphere(2)
    return v, f


JITTER_SEED, JITTER, JITTER_TOL = 11, 0.03, 0.05


def jittered_sphere():
    """The sphere with every vertex moved radially by a seeded factor in 1 +- 3 %: no longer symmetric, so the mirrored sample
    points lie off the surface."""
    v, f = sphere_case()
    rng = np.random.default_rng(JITTER_SEED)
    return (v * (1. + JITTER * rng.uniform(-1, 1, (v.shape[0], 1)))).astype(np.float32), f


def swollen_sphere():
    """The jittered sphere with the half x < 0 blown up by a tenth: the mirrored sample points float a tenth of the radius above
    the other half, so closest points on edges and at corners, with their exact ties between the faces that share them, are
    common."""
    v, f = jittered_sphere()
    return (v * np.where(v[:, :1] < 0, np.float32(1.1), np.float32(1))).astype(np.float32), f


MIRROR_FIXTURES = {'jittered': jittered_sphere, 'swollen': swollen_sphere}


def max_d2_of(rest, tol):
    """(tol x bounding-box diagonal)^2 as nnutils/bake.py:mirror_fill forms it: the diagonal in float32, the rest in Python floats."""
    rest = np.asarray(rest, np.float32)
    return (tol * float(np.linalg.norm(rest.max(0) - rest.min(0)))) ** 2


def unseen_by_x(rest, faces, R, cut=-0.05):
    """weight [F,R*R]: 0 where the texel's centroid has x < cut, else 1."""
    F = faces.shape[0]
    p = sample_points(rest, faces, np.arange(F * R * R), R, np.float64)
    return (p[:, 0] >= cut).astype(np.float32).reshape(F, R * R), p.reshape(F, R * R, 3)


@functools.lru_cache(maxsize=None)
def mirror_margins(name, R):
    """The float64 and float32 restatements of a fixture of MIRROR_FIXTURES about axis 0 with every texel of x < -0.05 listed, and
    the bound the device is held to: 4 x the largest |d2_f32 - d2_f64| plus one float32 ulp of the largest d2.  Computed once per
    (name, R) and shared; the callers leave it unchanged."""
    rest, faces = MIRROR_FIXTURES[name]()
    weight, points = unseen_by_x(rest, faces, R)
    texels = np.nonzero(weight.reshape(-1) == 0)[0]
    max_d2 = max_d2_of(rest, JITTER_TOL)
    m64 = mirror(rest, faces, texels, weight, R, 0, max_d2, np.float64)
    m32 = mirror(rest, faces, texels, weight, R, 0, max_d2, np.float32)
    ulp = float(np.spacing(np.float32(m64['d2'].max())))
    bound = 4. * float(np.abs(m32['d2'].astype(np.float64) - m64['d2']).max()) + ulp
    return dict(rest=rest, faces=faces, weight=weight, points=points, texels=texels, max_d2=max_d2, m64=m64, m32=m32, bound=bound)
