"""Independent numpy restatement of the re-meshing in csrc/manifold.hip: the well-composed repair, the refill, the boundary
extraction in the orders include/lasr_ops.h documents, and topology checks of a triangle mesh.  Shared by test_manifold_cpu.py and
test_manifold_gpu.py."""
import itertools

import numpy as np


def _checker(a, b, c, d):
    return (a == d) & (b == c) & (a != b)


def repair_sweep(solid):
    """One Jacobi sweep: every empty voxel of a critical configuration (a checkerboard 2x2 square of an axis plane, or a 2x2x2
    block whose only voxels of one value are an antipodal pair) becomes solid.  Voxels outside the grid are empty."""
    S = solid.shape[0]
    P = np.pad(solid.astype(bool), 1)
    add = np.zeros_like(P)
    n = S + 1                                             # anchors 0..S of the padded grid along an axis of the configuration

    def cell(off, ext):
        return tuple(slice(o, o + e) for o, e in zip(off, ext))

    for a, b in ((0, 1), (0, 2), (1, 2)):                 # squares of the (a, b) plane, every position along the third axis
        ext = [S + 2] * 3
        ext[a] = ext[b] = n
        ea, eb = np.eye(3, dtype=int)[a], np.eye(3, dtype=int)[b]
        offs = [np.zeros(3, int), ea, eb, ea + eb]         # A, B, C, D: diagonals (A, D) and (B, C)
        A, B, C, D = (P[cell(o, ext)] for o in offs)
        crit = _checker(A, B, C, D)
        for o in offs:
            add[cell(o, ext)] |= crit
    corners = list(itertools.product((0, 1), repeat=3))
    v = {c: P[cell(c, (n, n, n))] for c in corners}
    crit = np.zeros((n, n, n), bool)
    for p in corners[:4]:
        q = tuple(1 - x for x in p)
        others = [v[c] for c in corners if c not in (p, q)]
        anyo, allo = np.logical_or.reduce(others), np.logical_and.reduce(others)
        crit |= (v[p] & v[q] & ~anyo) | (~v[p] & ~v[q] & allo)
    for c in corners:
        add[cell(c, (n, n, n))] |= crit
    return solid.astype(bool) | add[1:-1, 1:-1, 1:-1]


def repair(solid):
    """-> (repaired solid, sweeps run; the last one changes nothing)."""
    cur = solid.astype(bool)
    sweeps = 0
    while True:
        nxt = repair_sweep(cur)
        sweeps += 1
        if (nxt == cur).all():
            return cur, sweeps
        cur = nxt


def fill(solid):
    """solid | every empty voxel not 6-connected through empty voxels to the grid's boundary."""
    from scipy import ndimage
    empty = ~solid.astype(bool)
    lab, _ = ndimage.label(empty, structure=ndimage.generate_binary_structure(3, 1))
    border = np.unique(np.concatenate([lab[0].ravel(), lab[-1].ravel(), lab[:, 0].ravel(), lab[:, -1].ravel(),
                                       lab[:, :, 0].ravel(), lab[:, :, -1].ravel()]))
    outside = np.isin(lab, border[border > 0])
    return ~outside


# (axis, sign) in the documented order -c0, +c0, -c1, +c1, -c2, +c2
DIRS = [(a, s) for a in range(3) for s in (0, 1)]


def quad_corners(a, s):
    """Offsets from the voxel's corner of the quad of direction (a, s): q0..q3, counter-clockwise seen from the empty side."""
    b, c = (a + 1) % 3, (a + 2) % 3
    order = [0, 1, 2, 3] if s else [0, 3, 2, 1]
    base = [(0, 0), (1, 0), (1, 1), (0, 1)]
    out = []
    for j in order:
        o = [0, 0, 0]
        o[a] = s
        o[b], o[c] = base[j]
        out.append(o)
    return np.array(out)


def extract(solid):
    """Boundary of the solid -> (verts [V,3] int lattice coordinates by lattice linear index, faces [F,3] int64 by voxel linear
    index, then direction, then the two triangles (q0, q1, q2), (q0, q2, q3) of the quad)."""
    s = solid.astype(bool)
    S = s.shape[0]
    P = np.pad(s, 1)
    # lattice point p has voxels p-1 and p along each axis: padded indices p and p+1
    blocks = [P[i:i + S + 1, j:j + S + 1, k:k + S + 1] for i, j, k in itertools.product((0, 1), repeat=3)]
    anyv, allv = np.logical_or.reduce(blocks), np.logical_and.reduce(blocks)
    is_vert = anyv & ~allv
    vid = np.full(is_vert.shape, -1, np.int64)
    vid[is_vert] = np.arange(int(is_vert.sum()))
    verts = np.argwhere(is_vert)
    emit = np.zeros(s.shape + (6,), bool)
    for d, (a, sg) in enumerate(DIRS):
        off = [1, 1, 1]
        off[a] += 1 if sg else -1
        nb = P[off[0]:off[0] + S, off[1]:off[1] + S, off[2]:off[2] + S]
        emit[..., d] = s & ~nb
    vox_dir = np.argwhere(emit)                           # C order: voxel linear index, then direction
    faces = np.zeros((2 * len(vox_dir), 3), np.int64)
    for d, (a, sg) in enumerate(DIRS):
        sel = vox_dir[:, 3] == d
        if not sel.any():
            continue
        base = vox_dir[sel, :3]
        q = [vid[tuple((base + o).T)] for o in quad_corners(a, sg)]
        rows = np.nonzero(sel)[0]
        faces[2 * rows] = np.stack([q[0], q[1], q[2]], 1)
        faces[2 * rows + 1] = np.stack([q[0], q[2], q[3]], 1)
    return verts, faces


def pipeline(solid):
    """repair, refill, extract -> (solid, sweeps, verts, faces)."""
    rep, sweeps = repair(solid)
    rep = fill(rep)
    v, f = extract(rep)
    return rep, sweeps, v, f


# ---- topology -------------------------------------------------------------------------------------------------------------
def directed_edges(faces):
    f = np.asarray(faces)
    return np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])


def closed_oriented(faces):
    """Every directed edge appears once and its reverse once."""
    e = directed_edges(faces)
    if len(e) == 0:
        return False
    keys = e[:, 0].astype(np.int64) * (1 << 32) + e[:, 1]
    rkeys = e[:, 1].astype(np.int64) * (1 << 32) + e[:, 0]
    u, c = np.unique(keys, return_counts=True)
    return bool((c == 1).all()) and bool(np.isin(rkeys, u).all())


def vertex_links_are_cycles(faces, V):
    """Around every vertex, the opposite edges of its faces form one cycle."""
    f = np.asarray(faces)
    nxt = {}
    for t in f:
        for i in range(3):
            v, a, b = t[i], t[(i + 1) % 3], t[(i + 2) % 3]
            d = nxt.setdefault(int(v), {})
            if int(a) in d:
                return False
            d[int(a)] = int(b)
    if len(nxt) != V:
        return False
    for d in nxt.values():
        start = next(iter(d))
        cur, n = start, 0
        while True:
            cur = d.get(cur)
            n += 1
            if cur is None:
                return False
            if cur == start:
                break
        if n != len(d):
            return False
    return True


def is_closed_manifold(faces, V):
    return closed_oriented(faces) and vertex_links_are_cycles(faces, V)


def euler(faces, V):
    f = np.asarray(faces)
    e = np.sort(directed_edges(f), 1)
    E = len(np.unique(e[:, 0].astype(np.int64) * (1 << 32) + e[:, 1]))
    return V - E + len(f)


def components(faces, V):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    e = directed_edges(faces)
    m = coo_matrix((np.ones(len(e)), (e[:, 0], e[:, 1])), shape=(V, V))
    return connected_components(m, directed=False)[0]


def signed_volume(verts, faces):
    v = np.asarray(verts, np.float64)
    t = v[np.asarray(faces)]
    return float(np.einsum('ij,ij->i', t[:, 0], np.cross(t[:, 1], t[:, 2])).sum() / 6)


def random_solid(S, density, seed, margin=2, smooth=0):
    """A random solid with `margin` empty outer layers; smooth > 0 blurs the noise first (blobs instead of salt)."""
    rng = np.random.default_rng(seed)
    x = rng.random((S, S, S))
    if smooth:
        from scipy import ndimage
        x = ndimage.uniform_filter(x, smooth)
        x = (x - x.min()) / max(x.max() - x.min(), 1e-12)
        thr = np.quantile(x[margin:S - margin, margin:S - margin, margin:S - margin], 1 - density)
        s = x > thr
    else:
        s = x < density
    m = np.zeros_like(s)
    m[margin:S - margin, margin:S - margin, margin:S - margin] = True
    return s & m
