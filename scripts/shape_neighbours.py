"""Folds between neighbouring faces: the second pass of scripts/eval_shape.py, --neighbours.

lasr_amd/nnutils/meshcheck.py tests every pair of faces that share no vertex, so a fold between two neighbours goes unseen there:
a vertex that slid across its own ring, a fin folded flat, a limb tip turned inside out.  This module lists the pairs of faces
that do share a vertex or an edge, once per topology (lasr_meshnbr_list), and tests them in every frame (lasr_meshnbr_test, on the
face records lasr_meshcheck_faces left): a vertex pair is PIERCED when the edge opposite the shared corner of one face passes
through the other, an edge pair is CREASED when its interior dihedral angle is below fold_deg.  Non-coplanar faces that share an
edge cannot intersect outside that edge, so creasing is an angle criterion, not an intersection test.  include/lasr_ops.h states
the arithmetic, tests/meshnbr_restated.py is the definition, lasr_amd/csrc/meshnbr.hip holds the kernels.  The default
fold_deg = 20 is derived from nothing measured on a real reconstruction; min_dihedral is reported so that a user can judge.

All tensors live on the device.  The topology costs one small host read (the size of the list); `evaluate` reads everything it
returns in one copy at the end.
"""
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from lasr_amd import _lib                       # noqa: E402
from lasr_amd.nnutils import meshcheck          # noqa: E402

DEFAULT_FOLD_DEG = 20.                          # unmeasured on any real reconstruction
DEFAULT_MAX_PAIRS = meshcheck.DEFAULT_MAX_PAIRS
CAPACITY_PER_FACE = 16                          # a closed manifold has about 6 entries per face
VERTEX, EDGE = 0, 1                             # the kind of a list entry; of a hit: pierced, creased
COUNTERS = ('n_list', 'n_duplicate', 'n_degenerate', 'n_same')


def fold_k(fold_deg):
    """cos^2(fold_deg) in double, rounded once to float32; refused: an angle outside (0, 90]."""
    deg = float(fold_deg)
    if not (math.isfinite(deg) and 0. < deg <= 90.):
        raise ValueError('shape_neighbours: fold_deg must be inside (0, 90], got %s' % fold_deg)
    return float(np.float32(math.cos(math.radians(deg)) ** 2))


def _max_pairs(max_pairs, T):
    max_pairs = int(max_pairs)
    if max_pairs < 0 or 3 * T * max_pairs > 0x7fffffff:
        raise ValueError('shape_neighbours: max_pairs must be at least 0 and 3 T max_pairs below 2^31, got %d' % max_pairs)
    return max_pairs


def _faces(faces):
    if not torch.is_tensor(faces):
        raise TypeError('shape_neighbours: faces must be a tensor')
    _lib.need_cuda(faces)
    if faces.ndimension() != 2 or faces.shape[1] != 3 or faces.is_floating_point() or faces.dtype == torch.bool:
        raise ValueError('shape_neighbours: faces must be integers [F,3], got %s %s' % (faces.dtype, tuple(faces.shape)))
    if faces.shape[0] > _lib.MESHCHECK_MAX_FACES:
        raise ValueError('shape_neighbours: %d faces exceed the limit of %d' % (faces.shape[0], _lib.MESHCHECK_MAX_FACES))
    return faces.contiguous().int()


def neighbour_list(faces, capacity=None):
    """faces [F,3] -> (keys int64 [n], sorted: lexicographic (i, j) order; counts: a dict of int64 scalars on the device, n_list,
    n_vertex, n_edge, n_duplicate, n_degenerate, n_same).  A key is i << 32 | j << 8 | ca | cb << 2 | edge << 4 | same << 5.
    capacity: the entries the first pass has room for (default 16 F); a list that does not fit is made once more at its exact size."""
    faces = _faces(faces)
    dev, F = faces.device, faces.shape[0]
    capacity = CAPACITY_PER_FACE * F if capacity is None else int(capacity)
    if capacity < 0 or capacity > 0x7fffffff:
        raise ValueError('shape_neighbours: the capacity of the list must be 0 .. 2^31 - 1, got %d' % capacity)
    counters = torch.zeros(_lib.MESHNBR_COUNTERS, dtype=torch.int64, device=dev)
    n = 0
    if F:
        keys = torch.empty(max(capacity, 1), dtype=torch.int64, device=dev)
        _lib.call('lasr_meshnbr_list', faces, keys if capacity > 0 else None, counters, F, capacity, on=dev)
        n = int(counters[0])                                                       # the one host read of a topology
        if n > 0x7fffffff:
            raise ValueError('shape_neighbours: %d pairs of neighbouring faces exceed 2^31 - 1' % n)
        if n > capacity:                                                           # the counts are exact: once more, at that size
            keys = torch.empty(n, dtype=torch.int64, device=dev)
            _lib.call('lasr_meshnbr_list', faces, keys, counters, F, n, on=dev)
    keys = torch.sort(keys[:n])[0] if n else torch.zeros(0, dtype=torch.int64, device=dev)
    n_edge = ((keys >> 4) & 1).sum()
    counts = dict(zip(COUNTERS, counters.unbind(0)), n_edge=n_edge, n_vertex=keys.numel() - n_edge)
    return keys, counts


def _tests(ws, nbytes, keys, k, T, F, max_pairs, dev):
    """The test pass on the records of `ws`: -> (totals int64 [T,2], nbr_count int32 [T,2,F], hits int32 [T,max_pairs,3],
    min_cos float32 [T])."""
    n = keys.numel()
    hits = torch.zeros(T, max_pairs, 3, dtype=torch.int32, device=dev)             # (the tail past the cursor is never written)
    if T == 0 or F == 0 or n == 0:                                                 # nothing is launched: zeros, and no angle
        return (torch.zeros(T, 2, dtype=torch.int64, device=dev), torch.zeros(T, 2, F, dtype=torch.int32, device=dev), hits,
                torch.full((T,), float('nan'), dtype=torch.float32, device=dev))
    totals = torch.empty(T, 2, dtype=torch.int64, device=dev)                      # the kernel's uint64 totals: below 2^40
    nbr_count = torch.empty(T, 2, F, dtype=torch.int32, device=dev)
    cursor = torch.empty(T, dtype=torch.int32, device=dev)
    min_cos = torch.empty(T, dtype=torch.float32, device=dev)
    _lib.call('lasr_meshnbr_test', ws, nbytes, keys, n, k, nbr_count, totals, cursor, hits if max_pairs > 0 else None, min_cos, T, F,
              max_pairs, on=dev)
    return totals, nbr_count, hits, min_cos


def neighbour_tests(verts, faces, fold_deg=DEFAULT_FOLD_DEG, max_pairs=DEFAULT_MAX_PAIRS, nbr=None):
    """verts [T,V,3] (or [V,3]), faces [F,3] -> a dict of device tensors: n_pierced, n_creased int64 [T]; nbr_count int32 [T,2,F],
    per face the neighbours it is pierced by and creased with; hits int32 [T,max_pairs,3] = (i, j, kind) in no defined order,
    complete for a frame iff n_pierced + n_creased <= max_pairs; min_cos float32 [T], the cosine of the sharpest dihedral angle
    (NaN when the topology has no edge pair); nbr = (keys, counts) of neighbour_list, which may be handed in again."""
    k = fold_k(fold_deg)
    verts, faces, T, V, F = meshcheck._prepare(verts, faces)
    max_pairs = _max_pairs(max_pairs, T)
    dev = verts.device
    keys, counts = nbr if nbr is not None else neighbour_list(faces)
    ws, nbytes, _, _ = meshcheck._records(verts, faces, T, V, F)
    totals, nbr_count, hits, min_cos = _tests(ws, nbytes, keys, k, T, F, max_pairs, dev)
    return dict(n_pierced=totals[:, 0], n_creased=totals[:, 1], nbr_count=nbr_count, hits=hits, min_cos=_no_edge_is_nan(min_cos, counts),
                nbr=(keys, counts))


def _no_edge_is_nan(min_cos, counts):
    return torch.where(counts['n_edge'] > 0, min_cos, torch.full_like(min_cos, float('nan')))


def sort_hits(hits, n_hits, max_pairs):
    """numpy hits [T,max_pairs,3] and n_hits [T] -> per frame the sorted [n,3] int64 array, or None where n exceeds max_pairs."""
    out = []
    for h, n in zip(hits, n_hits):
        if n > max_pairs:
            out.append(None)
            continue
        h = np.asarray(h[:int(n)], np.int64).reshape(-1, 3)
        out.append(h[np.lexsort((h[:, 2], h[:, 1], h[:, 0]))])
    return out


def dihedral(min_cos):
    """180 - acos(clamp(min_cos)) in degrees, float64; NaN stays NaN."""
    c = np.asarray(min_cos, np.float64)
    with np.errstate(invalid='ignore'):
        return 180. - np.degrees(np.arccos(np.clip(c, -1., 1.)))


def evaluate(verts, faces, max_pairs=DEFAULT_MAX_PAIRS, fold_deg=DEFAULT_FOLD_DEG):
    """meshcheck.evaluate's dict (the same values) plus, as numpy arrays per frame: n_pierced, n_creased, n_neighbour_faces (faces
    with either count > 0) int64, min_cos float32, min_dihedral float64 (degrees; NaN without an edge pair), nbr_truncated bool,
    nbr_count int32 [T,2,F], hits (per frame the sorted (i, j, kind) int64 [n,3], None where truncated); and `topology`, a dict of
    ints: n_list, n_vertex, n_edge, n_duplicate, n_degenerate, n_same."""
    k = fold_k(fold_deg)
    verts, faces, T, V, F = meshcheck._prepare(verts, faces)
    max_pairs = _max_pairs(max_pairs, T)
    dev = verts.device
    ws, nbytes, volume, area = meshcheck._records(verts, faces, T, V, F)
    n_pairs, face_count, pairs = meshcheck._pairs(ws, nbytes, T, F, max_pairs, dev)
    keys, counts = neighbour_list(faces)
    totals, nbr_count, hits, min_cos = _tests(ws, nbytes, keys, k, T, F, max_pairs, dev)
    min_cos = _no_edge_is_nan(min_cos, counts)
    n_faces, n_nbr = (face_count > 0).sum(1), (nbr_count.sum(1) > 0).sum(1)
    names = sorted(counts)
    topo = torch.stack([counts[c].reshape(()).long() for c in names])
    n, nf, vol, ar, jit, fc, p, tot, nn, nc, h, mc, tp = meshcheck.read_together(
        [n_pairs, n_faces, volume, area, meshcheck.jitter(verts), face_count, pairs, totals, n_nbr, nbr_count, hits, min_cos, topo])
    n_hits = tot.sum(1)
    return dict(n_pairs=n, n_faces=nf, ratio=nf / float(F) if F else np.zeros(T), volume=vol, area=ar, jitter=jit, inverted=vol < 0,
                truncated=n > max_pairs, face_count=fc, pairs=meshcheck.sort_pairs(p, n, max_pairs),
                n_pierced=tot[:, 0].copy(), n_creased=tot[:, 1].copy(), n_neighbour_faces=nn, min_cos=mc, min_dihedral=dihedral(mc),
                nbr_truncated=n_hits > max_pairs, nbr_count=nc, hits=sort_hits(h, n_hits, max_pairs),
                topology={c: int(x) for c, x in zip(names, tp)})
