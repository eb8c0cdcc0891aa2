"""float64 numpy restatement of the dense point tracks (include/lasr_ops.h: lasr_track_anchor, lasr_track_project,
lasr_track_splat_keys / lasr_track_splat_resolve), written from the header text.  The tracks are this project's own
addition, so this file is what the kernels are checked against.  It takes the raster's face-index planes as an input and flags the
(frame, query) entries whose discrete choices sit so close to a boundary that float32 and float64 may legitimately differ."""
import numpy as np

UNDECIDED_PX = 1e-3          # u or v this close to a pixel border
UNDECIDED_COS = 1e-4         # |n . P| / (|n| |P|) below this: the facing sign is a matter of rounding
UNDECIDED_CLAMP = 1e-6       # an unclamped barycentric this close to 0 or 1
SPLAT_ALPHA = 192


def _face_frame(verts_t, tri):
    """verts_t [V,3], tri [..., 3] vertex indices -> V0, e1, e2, n = e1 x e2."""
    V0, V1, V2 = verts_t[tri[..., 0]], verts_t[tri[..., 1]], verts_t[tri[..., 2]]
    e1, e2 = V1 - V0, V2 - V0
    return V0, e1, e2, np.cross(e1, e2)


def _named(plane, r, c, F):
    g = plane[r, c]
    return int(g) if 0 <= g < F else -1


def anchor(verts, faces, K, planes, queries, H, W, snap_radius=0):
    """planes [T, >= H, >= W]: plane 1 of the hard raster per frame.  -> dict of face [Q] (-1: none), bary [Q,3] (c0, c1, c2),
    facing [Q], snapped [Q,2] (v, u), shaky [Q] bool (an unclamped barycentric within UNDECIDED_CLAMP of a clamp, or the facing
    sign within UNDECIDED_COS of edge-on)."""
    verts, K, queries = np.asarray(verts, np.float64), np.asarray(K, np.float64), np.asarray(queries, np.float64)
    faces = np.asarray(faces)
    T, V, F, Q = verts.shape[0], verts.shape[1], faces.shape[0], queries.shape[0]
    face = -np.ones(Q, np.int64)
    bary = np.zeros((Q, 3))
    bary[:, 0] = 1.                                                   # c0 = 1 - c1 - c2 of an empty record
    facing = np.zeros(Q)
    snapped = queries[:, 1:3].copy()
    shaky = np.zeros(Q, bool)
    for q in range(Q):
        t, v, u = queries[q]
        if not (0 <= t < T):
            continue
        t = int(t)
        if not (0 <= u < W and 0 <= v < H):
            continue
        row, col = int(np.floor(v)), int(np.floor(u))
        f = _named(planes[t], row, col, F)
        if f < 0 and snap_radius > 0:
            best = np.inf
            for r in range(max(row - snap_radius, 0), min(row + snap_radius, H - 1) + 1):
                for c in range(max(col - snap_radius, 0), min(col + snap_radius, W - 1) + 1):
                    g = _named(planes[t], r, c, F)
                    d = (c + 0.5 - u) ** 2 + (r + 0.5 - v) ** 2
                    if g >= 0 and d < best:                            # row-major scan, strict <: the lowest flat index on ties
                        best, f, br, bc = d, g, r, c
            if f >= 0:
                u, v = bc + 0.5, br + 0.5
        snapped[q] = (v, u)
        if f < 0:
            continue
        tri = faces[f]
        if tri.min() < 0 or tri.max() >= V:
            continue
        V0, e1, e2, n = _face_frame(verts[t], tri)
        d = np.array([(u - K[t, 2]) / K[t, 0], (v - K[t, 3]) / K[t, 1], 1.])
        p = np.cross(d, e2)
        det = e1 @ p
        if not (n @ n > 0) or det == 0:
            continue
        s = V0[2] * d - V0
        b1 = (s @ p) / det
        b2 = (d @ np.cross(s, e1)) / det
        if not (np.isfinite(b1) and np.isfinite(b2)):
            continue
        b = np.array([1. - b1 - b2, b1, b2])
        shaky[q] = bool((np.minimum(np.abs(b), np.abs(b - 1.)) < UNDECIDED_CLAMP).any())
        a = np.clip(b, 0., 1.)
        a = a / a.sum()
        P = V0 + a[1] * e1 + a[2] * e2
        nP = n @ P
        shaky[q] |= abs(nP) < UNDECIDED_COS * np.linalg.norm(n) * np.linalg.norm(P)
        face[q], bary[q], facing[q] = f, a, (1. if nP >= 0 else -1.)
    return dict(face=face, bary=bary, facing=facing, snapped=snapped, shaky=shaky)


def project(verts, faces, K, planes, anc, H, W, window=1):
    """-> tracks [Q,T,2] (u, v), state [Q,T] uint8, undecided [Q,T] bool."""
    verts, K = np.asarray(verts, np.float64), np.asarray(K, np.float64)
    faces = np.asarray(faces)
    T, V, F = verts.shape[0], verts.shape[1], faces.shape[0]
    face, bary, facing = anc['face'], anc['bary'], anc['facing']
    Q = face.shape[0]
    tracks = np.full((Q, T, 2), np.nan)
    state = np.zeros((Q, T), np.uint8)
    undecided = np.zeros((Q, T), bool)
    ok = (face >= 0) & (face < F)
    tri = faces[np.where(ok, face, 0)] if F else np.zeros((Q, 3), np.int64)
    ok &= (tri.min(1) >= 0) & (tri.max(1) < V)
    tri = np.where(ok[:, None], tri, 0)
    for t in range(T):
        V0, e1, e2, n = _face_frame(verts[t], tri)
        P = V0 + bary[:, 1:2] * e1 + bary[:, 2:3] * e2
        front = ok & (P[:, 2] > 0)
        z = np.where(front, P[:, 2], 1.)
        u = K[t, 0] * P[:, 0] / z + K[t, 2]
        v = K[t, 1] * P[:, 1] / z + K[t, 3]
        inside = front & (u >= 0) & (u < W) & (v >= 0) & (v < H)
        nP = (n * P).sum(1)
        same = np.where(nP >= 0, 1., -1.) == facing
        col = np.clip(np.floor(u), 0, W - 1).astype(int)
        row = np.clip(np.floor(v), 0, H - 1).astype(int)
        hit = np.zeros(Q, bool)
        for dy in range(-window, window + 1):
            for dx in range(-window, window + 1):
                r, c = row + dy, col + dx
                valid = (r >= 0) & (r < H) & (c >= 0) & (c < W)
                g = planes[t][np.clip(r, 0, H - 1), np.clip(c, 0, W - 1)]
                valid &= (g >= 0) & (g < F)
                gi = np.where(valid, g, 0).astype(int)
                shares = (faces[gi][:, :, None] == tri[:, None, :]).any((1, 2)) if F else np.zeros(Q, bool)
                hit |= valid & ((gi == face) | shares)
        st = np.where(same & hit, 1, 2)
        st = np.where(inside, st, 3)
        st = np.where(front, st, 4)
        st = np.where(ok, st, 0)
        state[:, t] = st
        shown = ok & front
        tracks[shown, t, 0], tracks[shown, t, 1] = u[shown], v[shown]
        near = (np.abs(u - np.round(u)) < UNDECIDED_PX) | (np.abs(v - np.round(v)) < UNDECIDED_PX)
        edge_on = np.abs(nP) < UNDECIDED_COS * np.linalg.norm(n, axis=1) * np.linalg.norm(P, axis=1)
        undecided[:, t] = shown & (near | edge_on | anc['shaky'])
    return tracks, state, undecided


def splat(frames, tracks, state, colors, radius):
    """frames uint8 [T,H,W,3], tracks [Q,T,2] (u, v), state [Q,T], colors uint8 [Q,3] -> (uint8 [T,H,W,3], keys [T,H,W])."""
    frames = np.asarray(frames)
    T, H, W = frames.shape[:3]
    Q = tracks.shape[0]
    keys = np.zeros((T, H, W), np.int64)
    for q in range(Q):
        for t in range(T):
            if state[q, t] != 1:
                continue
            u, v = tracks[q, t]
            if not (0 <= u < W and 0 <= v < H):
                continue
            col, row = int(np.floor(u)), int(np.floor(v))
            for dy in range(-radius, radius + 1):
                for dx in range(-radius, radius + 1):
                    r, c = row + dy, col + dx
                    if 0 <= r < H and 0 <= c < W and dx * dx + dy * dy <= radius * radius:
                        keys[t, r, c] = max(keys[t, r, c], q + 1)
    out = frames.copy()
    on = keys > 0
    col = np.asarray(colors).astype(np.int64)[np.maximum(keys, 1) - 1]                # T,H,W,3
    blend = (SPLAT_ALPHA * col + (255 - SPLAT_ALPHA) * frames.astype(np.int64) + 127) // 255
    out[on] = blend[on].astype(np.uint8)
    return out, keys
