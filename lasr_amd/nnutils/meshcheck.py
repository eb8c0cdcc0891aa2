"""Shape scores of a reconstruction (scripts/eval_shape.py).

This is the project's own addition: the reference has no counterpart.  Per frame of a sequence of meshes with one topology: the
pairs of faces that pass through each other (csrc/meshcheck.hip: an exact, strict triangle-pair test over all pairs of faces that
share no vertex), the signed volume (negative for a mesh turned inside out), the area, and the temporal jitter of the vertices.
include/lasr_ops.h states the arithmetic of the entry points, tests/meshcheck_restated.py is the definition.  Touching and
coplanar overlap do not count, and a fold between two faces that share a vertex goes unseen.

All tensors live on the device.  The face indices are checked there before anything is launched (one small host read);
`evaluate` then reads everything it returns in one copy at the end.
"""
import numpy as np
import torch

from .. import _lib

DEFAULT_MAX_PAIRS = 4096


def check_indices(faces, V):
    """ValueError unless every index of faces lies in [0, V): the precondition of the C ABI."""
    if faces.numel() and bool(((faces < 0) | (faces >= V)).any()):
        raise ValueError('meshcheck: a face index lies outside [0, %d)' % V)


def _prepare(verts, faces):
    """-> (verts float32 [T,V,3], faces int32 [F,3], T, V, F), validated."""
    for name, t in (('verts', verts), ('faces', faces)):
        if not torch.is_tensor(t):
            raise TypeError('meshcheck: %s must be a tensor' % name)
    _lib.need_cuda(verts, faces)
    if verts.ndimension() == 2:
        verts = verts[None]
    if verts.ndimension() != 3 or verts.shape[2] != 3:
        raise ValueError('meshcheck: verts must be [T,V,3], got %s' % (tuple(verts.shape),))
    if faces.ndimension() != 2 or faces.shape[1] != 3 or faces.is_floating_point():
        raise ValueError('meshcheck: faces must be integers [F,3], got %s %s' % (faces.dtype, tuple(faces.shape)))
    if faces.device != verts.device:
        raise ValueError('meshcheck: verts on %s, faces on %s' % (verts.device, faces.device))
    T, V, F = verts.shape[0], verts.shape[1], faces.shape[0]
    if T > _lib.MESHCHECK_MAX_FRAMES or F > _lib.MESHCHECK_MAX_FACES or T * F > 0x7fffffff or 3 * V > 0x7fffffff:
        raise ValueError('meshcheck: %d frames of %d faces exceed the limits (%d frames, %d faces, T F < 2^31)'
                         % (T, F, _lib.MESHCHECK_MAX_FRAMES, _lib.MESHCHECK_MAX_FACES))
    check_indices(faces, V)
    return _lib.f32(verts), faces.contiguous().int(), T, V, F


def _records(verts, faces, T, V, F):
    """The per-face pass: -> (workspace, volume [T], area [T])."""
    dev = verts.device
    nbytes = _lib.lib().lasr_meshcheck_workspace_bytes(T, F)
    ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=dev)
    volume, area = torch.zeros(T, dtype=torch.float64, device=dev), torch.zeros(T, dtype=torch.float64, device=dev)
    _lib.call('lasr_meshcheck_faces', verts, faces, ws, nbytes, volume, area, T, V, F, on=dev)
    return ws, nbytes, volume, area


def _pairs(ws, nbytes, T, F, max_pairs, dev):
    """The pair pass: -> (n_pairs int64 [T], face_count int32 [T,F], pairs int32 [T,max_pairs,2])."""
    max_pairs = int(max_pairs)
    if max_pairs < 0 or 2 * T * max_pairs > 0x7fffffff:
        raise ValueError('meshcheck: max_pairs must be at least 0 and 2 T max_pairs below 2^31, got %d' % max_pairs)
    n_pairs = torch.zeros(T, dtype=torch.int64, device=dev)                    # the kernel's uint64 total: below 2^40
    face_count = torch.zeros(T, F, dtype=torch.int32, device=dev)
    cursor = torch.zeros(max(T, 1), dtype=torch.int32, device=dev)
    pairs = torch.zeros(T, max_pairs, 2, dtype=torch.int32, device=dev)
    _lib.call('lasr_meshcheck_pairs', ws, nbytes, face_count, n_pairs, cursor, pairs if max_pairs > 0 else None, T, F, max_pairs, on=dev)
    return n_pairs, face_count, pairs


def sort_pairs(pairs, n_pairs, max_pairs):
    """numpy pairs [T,max_pairs,2] and n_pairs [T] -> per frame the sorted [n,2] int64 array, or None where n exceeds max_pairs."""
    out = []
    for p, n in zip(pairs, n_pairs):
        if n > max_pairs:
            out.append(None)
            continue
        p = np.asarray(p[:int(n)], np.int64).reshape(-1, 2)
        out.append(p[np.lexsort((p[:, 1], p[:, 0]))])
    return out


def self_intersections(verts, faces, max_pairs=DEFAULT_MAX_PAIRS):
    """verts [T,V,3] (or [V,3]), faces [F,3] -> (n_pairs int64 [T], face_count int32 [T,F], pairs, truncated bool [T]): the number
    of intersecting pairs of faces per frame, per face the number of faces it intersects, per frame the pairs (i, j), i < j, as a
    sorted int64 [n,2] numpy array, or None for a frame with more than max_pairs of them (truncated; its counts stay exact)."""
    verts, faces, T, V, F = _prepare(verts, faces)
    dev = verts.device
    ws, nbytes, _, _ = _records(verts, faces, T, V, F)
    n_pairs, face_count, pairs = _pairs(ws, nbytes, T, F, max_pairs, dev)
    n, p = read_together([n_pairs, pairs])
    return n_pairs, face_count, sort_pairs(p, n, int(max_pairs)), n_pairs > int(max_pairs)


def volume_area(verts, faces):
    """-> (volume [T], area [T]) float64 on the device: sum_f a . (b x c) / 6, positive for outward-facing faces, and the area."""
    verts, faces, T, V, F = _prepare(verts, faces)
    _, _, volume, area = _records(verts, faces, T, V, F)
    return volume, area


def jitter(verts):
    """[T] float64 on the device: the mean over the vertices of |v_{t+1} - 2 v_t + v_{t-1}| over the diagonal of frame t's bounding
    box; NaN for the first and the last frame."""
    if not torch.is_tensor(verts):
        raise TypeError('meshcheck: verts must be a tensor')
    _lib.need_cuda(verts)
    if verts.ndimension() != 3 or verts.shape[2] != 3:
        raise ValueError('meshcheck: verts must be [T,V,3], got %s' % (tuple(verts.shape),))
    v = verts.double()
    out = torch.full((v.shape[0],), float('nan'), dtype=torch.float64, device=v.device)
    if v.shape[0] >= 3 and v.shape[1] >= 1:
        d = (v[2:] - 2. * v[1:-1]) + v[:-2]
        extent = v[1:-1].amax(1) - v[1:-1].amin(1)
        out[1:-1] = d.norm(dim=-1).mean(1) / extent.norm(dim=-1)
    return out


def read_together(tensors):
    """Device tensors -> numpy arrays of the same dtypes and shapes through one copy to the host."""
    if not tensors:
        return []
    flat = [t.contiguous().reshape(-1).view(torch.uint8) for t in tensors]
    buf = torch.cat(flat).cpu().numpy()
    out, off = [], 0
    for t, f in zip(tensors, flat):
        n = f.numel()
        dt = np.dtype(str(t.dtype).replace('torch.', ''))
        out.append(np.frombuffer(buf[off:off + n].tobytes(), dtype=dt).reshape(tuple(t.shape)))
        off += n
    return out


def evaluate(verts, faces, max_pairs=DEFAULT_MAX_PAIRS):
    """Everything scripts/eval_shape.py reports, as numpy arrays per frame: n_pairs, n_faces (faces with a partner) int64, ratio =
    n_faces / F, volume, area, jitter float64, inverted (volume < 0) and truncated bool, face_count int32 [T,F], and pairs (the
    list of self_intersections)."""
    verts, faces, T, V, F = _prepare(verts, faces)
    dev = verts.device
    ws, nbytes, volume, area = _records(verts, faces, T, V, F)
    n_pairs, face_count, pairs = _pairs(ws, nbytes, T, F, max_pairs, dev)
    n_faces = (face_count > 0).sum(1)
    n, nf, vol, ar, jit, fc, p = read_together([n_pairs, n_faces, volume, area, jitter(verts), face_count, pairs])
    return dict(n_pairs=n, n_faces=nf, ratio=nf / float(F) if F else np.zeros(T), volume=vol, area=ar, jitter=jit, inverted=vol < 0,
                truncated=n > int(max_pairs), face_count=fc, pairs=sort_pairs(p, n, int(max_pairs)))
