"""Restatement of the neighbour pass of the shape scores (scripts/eval_shape.py --neighbours; include/lasr_ops.h, DESIGN.md section
4.18) in plain numpy, and the fixtures tests/test_meshnbr_cpu.py and tests/test_meshnbr_gpu.py share.  Nothing here imports the
package or torch: the kernels of lasr_amd/csrc/meshnbr.hip and scripts/shape_neighbours.py are compared against this file, not the
other way round.  orient, pierces and the spheres are those of tests/meshcheck_restated.py.

This file is the definition.  The pair pass of meshcheck_restated never tests two faces that share a vertex; this pass tests
exactly those, and nothing else.

Topology (faces only, once for all frames).  A face with a repeated index is DEGENERATE: counted, and part of nothing.  For
non-degenerate faces i < j let s be the number of corners of i whose index is a corner of j.  s = 0: no neighbour.  s = 1: a VERTEX
pair; ca, cb = the position (0..2) of the shared corner in i and in j.  s = 2: an EDGE pair; ca, cb = the position of the corner that
is NOT shared (the apex) in i and in j, and `same` is set when the shared edge runs in the same direction in both cyclic orders (an
inconsistent orientation: a consistently oriented surface walks the edge in opposite directions).  s = 3: a DUPLICATE, counted and
never tested.  The list is every vertex pair and edge pair in lexicographic (i, j) order; an entry is the 64-bit key
i << 32 | j << 8 | ca | cb << 2 | edge << 4 | same << 5.

Vertex pair, A = tri(i), B = tri(j) in stored corner order: PIERCED iff pierces(A[(ca+1)%3], A[(ca+2)%3], B0, B1, B2) or
pierces(B[(cb+1)%3], B[(cb+2)%3], A0, A1, A2).  Only the edge opposite the shared corner is tested: the planes of the two triangles
meet in a line through the shared vertex, and if the triangles overlap beyond that vertex the overlap segment ends where the nearer
opposite edge enters the other triangle.  The edges through the shared vertex touch the other triangle in that vertex: their plane
determinants are zero in exact arithmetic and noise in float32, so they must not be tested.

Edge pair: nA = (A1 - A0) x (A2 - A0), nB likewise (the component order of orient's cross product); d = (nAx nBx + nAy nBy) + nAz nBz,
negated when `same` is set; qa = (nAx^2 + nAy^2) + nAz^2, qb likewise, q = qa qb; k = cos^2(fold_deg), computed in double and rounded
once to float32.  CREASED iff d < 0 and d d > k q, strictly, with q > 0 and both products finite: the interior dihedral angle is then
below fold_deg.  Non-coplanar faces that share an edge cannot intersect outside that edge, so this is an angle criterion, not an
intersection test.  Edge lengths from about 1e-4 to 1e4 keep q (the eighth power of a length) inside float32.  min_cos of a frame
is the minimum over the edge pairs with q > 0 of d / sqrt(q) (NaN without one); min_dihedral = 180 - acos(clamp(min_cos)) degrees.
The default fold_deg = 20 is derived from nothing measured on a real reconstruction.
"""
import functools
import math

import numpy as np

from meshcheck_restated import COPY_GRID, COPY_STEP, fixture as mc_fixture, icosphere, orient, pierces  # noqa: F401

FOLD_DEG = 20.
VERTEX, EDGE = 0, 1                                                               # the kind of a list entry; of a hit: pierced, creased


def fold_k(fold_deg=FOLD_DEG):
    """cos^2(fold_deg) in double, rounded once to float32."""
    return np.float32(math.cos(math.radians(float(fold_deg))) ** 2)


def pack(i, j, ca, cb, kind, same):
    i, j, ca, cb, kind, same = (np.asarray(x).astype(np.int64) for x in (i, j, ca, cb, kind, same))
    return (i << 32) | (j << 8) | ca | (cb << 2) | (kind << 4) | (same << 5)


def unpack(keys):
    """int64 keys -> (i, j, ca, cb, kind, same)."""
    k = np.asarray(keys).astype(np.int64)
    return k >> 32, (k >> 8) & 0xffffff, k & 3, (k >> 2) & 3, (k >> 4) & 1, (k >> 5) & 1


def topology(faces):
    """faces [F,3] -> dict: keys int64 [n] in lexicographic (i, j) order, i, j, ca, cb, kind, same (the fields of the keys), and the
    counts n_list, n_vertex, n_edge, n_duplicate, n_degenerate, n_same."""
    f = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    F = len(f)
    deg = (f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2])
    keys, n_dup = [], 0
    for lo in range(0, F, 512):                                                   # rows of i, 512 at a time: F^2 fits nowhere at once
        a = f[lo:lo + 512]
        eq = a[:, None, :, None] == f[None, :, None, :]                           # [n,F,3,3]: corner x of i is corner y of j
        ok = ~deg[lo:lo + 512, None] & ~deg[None] & (np.arange(lo, lo + len(a))[:, None] < np.arange(F)[None])
        ma, mb = eq.any(3), eq.any(2)                                             # corner x of i lies in j; corner y of j lies in i
        s = ma.sum(2) * ok
        n_dup += int((s == 3).sum())
        for kind in (VERTEX, EDGE):
            ii, jj = np.nonzero(s == kind + 1)
            want = kind == VERTEX                                                 # the one shared corner, or the one that is not
            ca, cb = np.argmax(ma[ii, jj] == want, 1), np.argmax(mb[ii, jj] == want, 1)
            gi = ii + lo
            same = (f[gi, (ca + 1) % 3] == f[jj, (cb + 1) % 3]) & (kind == EDGE)
            keys.append(pack(gi, jj, ca, cb, kind, same))
    keys = np.sort(np.concatenate(keys)) if keys else np.zeros(0, np.int64)
    i, j, ca, cb, kind, same = unpack(keys)
    return dict(keys=keys, i=i, j=j, ca=ca, cb=cb, kind=kind, same=same, n_list=len(keys), n_vertex=int((kind == VERTEX).sum()),
                n_edge=int((kind == EDGE).sum()), n_duplicate=n_dup, n_degenerate=int(deg.sum()), n_same=int(same.sum()))


def _frames(verts):
    verts = np.asarray(verts, np.float32)
    return verts[None] if verts.ndim == 2 else verts


def _normal(T, dt):
    """(b - a) x (c - a) of triangles [n,3,3] in dt, the component order of orient."""
    ux, uy, uz = (T[:, 1, c] - T[:, 0, c] for c in range(3))
    wx, wy, wz = (T[:, 2, c] - T[:, 0, c] for c in range(3))
    return (uy * wz - uz * wy).astype(dt), (uz * wx - ux * wz).astype(dt), (ux * wy - uy * wx).astype(dt)


def vertex_pairs(v, faces, top, dt=np.float64):
    """One frame -> (pierced bool [n], dets [n,10]) over the vertex pairs of the list: the opposite edge of i against j, then the
    opposite edge of j against i, five determinants each (two plane, three edge)."""
    m = top['kind'] == VERTEX
    tri = np.asarray(v, np.float32)[np.asarray(faces)].astype(dt)
    A, B, ca, cb = tri[top['i'][m]], tri[top['j'][m]], top['ca'][m], top['cb'][m]
    n = np.arange(len(A))
    h1, d1 = pierces(A[n, (ca + 1) % 3], A[n, (ca + 2) % 3], B[:, 0], B[:, 1], B[:, 2], dt)
    h2, d2 = pierces(B[n, (cb + 1) % 3], B[n, (cb + 2) % 3], A[:, 0], A[:, 1], A[:, 2], dt)
    return h1 | h2, np.concatenate([d1, d2], -1).reshape(len(A), 10)


def edge_pairs(v, faces, top, k, dt=np.float64):
    """One frame -> (creased bool [n], d [n], q [n], margin = d d - k q [n]) over the edge pairs of the list, all in dt."""
    m = top['kind'] == EDGE
    tri = np.asarray(v, np.float32)[np.asarray(faces)].astype(dt)
    ax, ay, az = _normal(tri[top['i'][m]], dt)
    bx, by, bz = _normal(tri[top['j'][m]], dt)
    with np.errstate(over='ignore', invalid='ignore'):
        d = ((ax * bx + ay * by) + az * bz).astype(dt)
        d = np.where(top['same'][m] == 1, -d, d).astype(dt)
        qa, qb = ((ax * ax + ay * ay) + az * az).astype(dt), ((bx * bx + by * by) + bz * bz).astype(dt)
        q, dd = (qa * qb).astype(dt), (d * d).astype(dt)
        kq = (dt(k) * q).astype(dt)
        creased = (d < 0) & (dd > kq) & (q > 0) & np.isfinite(q) & np.isfinite(dd)
        return creased, d, q, (dd - kq).astype(dt)


def neighbour_tests(verts, faces, fold_deg=FOLD_DEG, dt=np.float64, top=None):
    """-> per frame a dict: n_pierced, n_creased, nbr_count int32 [2,F] (per face: pierced by, creased with), hits int64 [n,3] =
    (i, j, kind) sorted, min_cos (NaN without an edge pair of q > 0), n_neighbour_faces."""
    faces = np.asarray(faces)
    top = top or topology(faces)
    F, k, out = faces.shape[0], fold_k(fold_deg), []
    vi, vj = top['i'][top['kind'] == VERTEX], top['j'][top['kind'] == VERTEX]
    ei, ej = top['i'][top['kind'] == EDGE], top['j'][top['kind'] == EDGE]
    for v in _frames(verts):
        pierced, _ = vertex_pairs(v, faces, top, dt)
        creased, d, q, _ = edge_pairs(v, faces, top, k, dt)
        count = np.stack([np.bincount(np.concatenate([vi[pierced], vj[pierced]]), minlength=F),
                          np.bincount(np.concatenate([ei[creased], ej[creased]]), minlength=F)]).astype(np.int32)
        hits = np.concatenate([np.stack([vi[pierced], vj[pierced], np.full(pierced.sum(), VERTEX)], -1),
                               np.stack([ei[creased], ej[creased], np.full(creased.sum(), EDGE)], -1)]).astype(np.int64).reshape(-1, 3)
        hits = hits[np.lexsort((hits[:, 2], hits[:, 1], hits[:, 0]))]
        good = (q > 0) & np.isfinite(q)
        with np.errstate(invalid='ignore', divide='ignore'):
            min_cos = float((d[good] / np.sqrt(q[good])).min()) if good.any() else float('nan')
        out.append(dict(n_pierced=int(pierced.sum()), n_creased=int(creased.sum()), nbr_count=count, hits=hits, min_cos=min_cos,
                        n_neighbour_faces=int((count.sum(0) > 0).sum())))
    return out


def dihedral(min_cos):
    """180 - acos(clamp(min_cos)) in degrees; NaN stays NaN."""
    c = np.asarray(min_cos, np.float64)
    with np.errstate(invalid='ignore'):
        return 180. - np.degrees(np.arccos(np.clip(c, -1., 1.)))


def evaluate(verts, faces, fold_deg=FOLD_DEG):
    """The keys scripts/eval_shape.py --neighbours adds, per frame, in float64, and the topology."""
    top = topology(faces)
    res = neighbour_tests(verts, faces, fold_deg, np.float64, top)
    min_cos = np.array([r['min_cos'] for r in res], np.float64)
    return dict(n_pierced=np.array([r['n_pierced'] for r in res], np.int64), n_creased=np.array([r['n_creased'] for r in res], np.int64),
                n_neighbour_faces=np.array([r['n_neighbour_faces'] for r in res], np.int64), min_cos=min_cos, min_dihedral=dihedral(min_cos),
                nbr_count=np.stack([r['nbr_count'] for r in res]) if res else np.zeros((0, 2, len(np.asarray(faces))), np.int32),
                hits=[r['hits'] for r in res], nbr_truncated=np.zeros(len(res), bool),
                topology={k: top[k] for k in ('n_list', 'n_vertex', 'n_edge', 'n_duplicate', 'n_degenerate', 'n_same')})


def margins(verts, faces, fold_deg=FOLD_DEG):
    """The condition behind the GPU equalities: -> (worst |det64| / |det32 - det64| over the ten determinants of every vertex pair
    of every frame, the same for d d - k q over every edge pair; inf where the two precisions give the same number)."""
    top, k = topology(faces), fold_k(fold_deg)
    worst = [np.inf, np.inf]
    for v in _frames(verts):
        d64, d32 = vertex_pairs(v, faces, top, np.float64)[1], vertex_pairs(v, faces, top, np.float32)[1].astype(np.float64)
        m64, m32 = edge_pairs(v, faces, top, k, np.float64)[3], edge_pairs(v, faces, top, k, np.float32)[3].astype(np.float64)
        for n, (a, b) in enumerate(((d64, d32), (m64, m32))):
            diff = np.abs(a - b)
            if a.size and (diff > 0).any():
                worst[n] = min(worst[n], float((np.abs(a)[diff > 0] / diff[diff > 0]).min()))
            if a.size and (a == 0).any():
                worst[n] = 0.
    return tuple(worst)


# ---- fixtures ----------------------------------------------------------------------------------------------------------------------
def crease(level, seed, s, h):
    """A jittered sphere with the vertex of largest x pushed s ring radii towards its first ring neighbour and h along the ring's
    normal (negative: below the surface): folds between the faces around it, none between distant faces for s <= 1.5."""
    v, f = icosphere(level, seed)
    v = v.copy()
    k = int(np.argmax(v[:, 0]))
    ring = np.array(sorted(set(f[(f == k).any(1)].reshape(-1).tolist()) - {k}))
    c = v[ring].astype(np.float64).mean(0)
    n = c / np.linalg.norm(c)
    v[k] = (c + s * (v[ring[0]].astype(np.float64) - c) + h * n).astype(np.float32)
    return v[None], f


def _flip1():
    v, f = icosphere(2, 2)
    f = f.copy()
    f[100] = f[100, ::-1]
    return v[None], f


def _batch3():
    """Three frames on one topology: the clean sphere of seed 41, creaseA, creaseB."""
    v, f = icosphere(2, 41)
    return np.stack([v, crease(2, 41, 1.5, -0.05)[0][0], crease(2, 41, 2.0, -0.05)[0][0]]), f


FIXTURES = {
    'ico1': lambda: mc_fixture('ico1'), 'ico2': lambda: mc_fixture('ico2'), 'inverted': lambda: mc_fixture('inverted'),
    'pinch2': lambda: mc_fixture('pinch2'), 'tile257': lambda: mc_fixture('tile257'), 'two2': lambda: mc_fixture('two2'),
    'wobble': lambda: mc_fixture('wobble'),
    'creaseA': lambda: crease(2, 41, 1.5, -0.05),
    'creaseB': lambda: crease(2, 41, 2.0, -0.05),
    'crease3': lambda: crease(3, 43, 2.0, -0.03),
    'flip1': _flip1,
    'batch3': _batch3,
}


@functools.lru_cache(None)
def fixture(name):
    """-> (verts float32 [T,V,3], faces int32 [F,3])."""
    verts, faces = FIXTURES[name]()
    return np.ascontiguousarray(verts, np.float32), np.ascontiguousarray(faces, np.int32)


@functools.lru_cache(None)
def expected(name, fold_deg=FOLD_DEG):
    """The float64 restatement of a fixture, computed once and shared: evaluate() plus the topology's keys."""
    verts, faces = fixture(name)
    return dict(evaluate(verts, faces, fold_deg), keys=topology(faces)['keys'])


@functools.lru_cache(None)
def copies_base():
    """creaseB with every coordinate rounded to a multiple of 2^-16."""
    verts, faces = fixture('creaseB')
    return (np.round(verts.astype(np.float64) / COPY_GRID) * COPY_GRID).astype(np.float32), faces


@functools.lru_cache(None)
def copies_case(n=8):
    """n exact translates of copies_base() in one face list (copy k moved by 8 (k % 8, k / 8 % 8, k / 64), as
    meshcheck_restated.copies_case): 320 n faces, so hits in tile pairs beyond the first, whose answer is n times the base's.  Every
    difference of two vertices of a copy is the base's, exactly, in float32 as in float64; no face of one copy shares a vertex with
    a face of another.  -> (verts [1,162 n,3], faces [320 n,3], expected: keys, n_pierced, n_creased, nbr_count [2,320 n], hits,
    min_cos, topology)."""
    v0, f0 = copies_base()
    V0, F0 = v0.shape[1], f0.shape[0]
    shift = np.array([[k % 8, k // 8 % 8, k // 64] for k in range(n)], np.float64) * COPY_STEP
    verts = (v0[0].astype(np.float64)[None] + shift[:, None]).reshape(1, n * V0, 3)
    assert (verts == verts.astype(np.float32)).all() and np.abs(verts).max() < 64
    faces = (f0[None].astype(np.int64) + V0 * np.arange(n)[:, None, None]).reshape(n * F0, 3).astype(np.int32)
    top = topology(f0)
    base = neighbour_tests(v0, f0, top=top)[0]
    i, j, ca, cb, kind, same = unpack(top['keys'])
    keys = np.concatenate([pack(i + F0 * c, j + F0 * c, ca, cb, kind, same) for c in range(n)])
    hits = np.concatenate([base['hits'] + np.array([F0 * c, F0 * c, 0]) for c in range(n)]).reshape(-1, 3)
    counts = {k: n * top[k] for k in ('n_list', 'n_vertex', 'n_edge', 'n_duplicate', 'n_degenerate', 'n_same')}
    return verts.astype(np.float32), faces, dict(keys=keys, n_pierced=n * base['n_pierced'], n_creased=n * base['n_creased'],
                                                 nbr_count=np.tile(base['nbr_count'], (1, n)), hits=hits, min_cos=base['min_cos'],
                                                 topology=counts)
