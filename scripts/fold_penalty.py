"""The fold penalty of the optimiser: optimize.py --fold_wt / --pierce_wt.

scripts/eval_shape.py --neighbours reports the folds between neighbouring faces of the meshes extract.py writes: pairs that share
an edge and are CREASED (the interior dihedral angle is below a threshold) and pairs that share a vertex and are PIERCED (the edge
opposite the shared corner of one passes through the other).  This module is the loss that acts on that report, on the posed meshes
of every optimisation step: per edge pair max(0, phi - theta)^2 of the interior dihedral angle theta, per vertex pair the depth of
the shallower end of a piercing edge.  The crease term is a function of the angle and not of its cosine, so it has a gradient at the
complete fold; the pierce term is linear in the depth, so a descent step carries the end point across the plane.  Both are zero
exactly where the report is clean.  include/lasr_ops.h states the arithmetic, tests/foldpen_restated.py is the definition,
lasr_amd/csrc/foldpen.hip holds the kernels; the list of pairs is scripts/shape_neighbours.py's.  The trainer's defaults (both
weights 0: off; fold_deg 30, above the evaluation's 20 so that a shape the penalty has released clears the report's threshold) are
derived from nothing measured on a real reconstruction.

All tensors live on the device.  The topology costs the list's one small host read and one for the inverted index; a call launches
two kernels forward and one backward, reads nothing on the host and allocates static shapes: it can be captured into a graph.
"""
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)
from lasr_amd import _lib                       # noqa: E402
import shape_neighbours                         # noqa: E402

DEFAULT_FOLD_DEG = 30.                          # unmeasured on any real reconstruction
SLOTS = 5                                       # 3-vectors of a contribution row (include/lasr_ops.h: the roles)


def fold_phi(fold_deg):
    """radians(fold_deg) in double, rounded once to float32; refused: an angle outside (0, 90]."""
    deg = float(fold_deg)
    if not (math.isfinite(deg) and 0. < deg <= 90.):
        raise ValueError('fold_penalty: fold_deg must be inside (0, 90], got %s' % fold_deg)
    return float(np.float32(math.radians(deg)))


def inverted_index(keys, faces, n_verts):
    """keys int64 [n] (sorted), faces int32 [F,3], V -> (vstart int32 [V+1], inc int32 [n_inc]): per vertex its incidences
    (entry 5 + slot) 2 + edge in ascending order.  An entry the kernel skips (a face outside [0, F), a vertex outside [0, V)) names
    no vertex.  Two torch sorts on the device; the number of incidences is one host read."""
    dev, n, F, V = keys.device, keys.numel(), faces.shape[0], int(n_verts)
    if n == 0 or F == 0 or V == 0:
        return torch.zeros(V + 1, dtype=torch.int32, device=dev), torch.zeros(0, dtype=torch.int32, device=dev)
    i, j, ca, cb, edge = keys >> 32, (keys >> 8) & 0xffffff, keys & 3, (keys >> 2) & 3, (keys >> 4) & 1
    ok = (i >= 0) & (i < F) & (j < F) & (ca < 3) & (cb < 3)
    fl = faces.long()
    fa, fb = fl[i.clamp(0, F - 1)], fl[j.clamp(0, F - 1)]
    ok = ok & ((fa >= 0) & (fa < V)).all(1) & ((fb >= 0) & (fb < V)).all(1)
    ca, cb = ca.clamp(max=2), cb.clamp(max=2)
    pick = lambda f, c: f.gather(1, (c % 3)[:, None])[:, 0]                        # noqa: E731
    vert = torch.stack([pick(fa, ca), pick(fa, ca + 1), pick(fa, ca + 2), torch.where(edge == 1, pick(fb, cb), pick(fb, cb + 1)),
                        torch.where(edge == 1, torch.full_like(i, -1), pick(fb, cb + 2))], 1)
    code = (torch.arange(n, device=dev)[:, None] * SLOTS + torch.arange(SLOTS, device=dev)[None]) * 2 + edge[:, None]
    packed = torch.sort(((vert << 32) | code)[ok[:, None] & (vert >= 0)])[0]
    vstart = torch.searchsorted(packed >> 32, torch.arange(V + 1, device=dev))
    return vstart.int(), (packed & 0xffffffff).int()


class _Penalty(torch.autograd.Function):
    @staticmethod
    def forward(ctx, verts, pen):
        loss, _, rows = pen.launch_forward(verts, ctx.needs_input_grad[0])
        ctx.pen, ctx.shape = pen, tuple(verts.shape)
        ctx.save_for_backward(rows)
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        rows, = ctx.saved_tensors
        return ctx.pen.launch_backward(rows, grad_loss, ctx.shape), None


class FoldPenalty:
    """FoldPenalty(faces [F,3], fold_deg=30.)(verts [N,V,3]) -> [N,2]: the crease sum and the pierce sum of every mesh, with a
    gradient by verts.  n_verts: the V of the calls to come (default: the largest index of faces + 1, one host read); keys: the
    sorted list of shape_neighbours.neighbour_list, which may be handed in."""

    def __init__(self, faces, fold_deg=DEFAULT_FOLD_DEG, n_verts=None, keys=None):
        self.phi = fold_phi(fold_deg)
        self.fold_deg = float(fold_deg)
        self.faces = shape_neighbours._faces(faces)
        if keys is None:
            keys = shape_neighbours.neighbour_list(self.faces)[0]
        if not torch.is_tensor(keys):
            raise TypeError('fold_penalty: keys must be a tensor')
        _lib.need_cuda(keys)
        if keys.dtype != torch.int64 or keys.ndimension() != 1 or keys.device != self.faces.device:
            raise ValueError('fold_penalty: keys must be int64 [n] on the device of faces, got %s %s' % (keys.dtype, tuple(keys.shape)))
        if keys.numel() > _lib.FOLDPEN_MAX_LIST:
            raise ValueError('fold_penalty: %d pairs of neighbouring faces exceed the limit of %d' % (keys.numel(), _lib.FOLDPEN_MAX_LIST))
        self.keys = keys.contiguous()
        if n_verts is None:
            n_verts = int(self.faces.max()) + 1 if self.faces.numel() else 0
        self._index = {}
        self.index(int(n_verts))

    def index(self, V):
        """The inverted index for meshes of V vertices, built once."""
        if V not in self._index:
            self._index[V] = inverted_index(self.keys, self.faces, V)
        return self._index[V]

    def _prepare(self, verts):
        if not torch.is_tensor(verts):
            raise TypeError('fold_penalty: verts must be a tensor')
        _lib.need_cuda(verts)
        if verts.ndimension() != 3 or verts.shape[2] != 3 or not verts.is_floating_point():
            raise ValueError('fold_penalty: verts must be floating point [N,V,3], got %s %s' % (verts.dtype, tuple(verts.shape)))
        if verts.device != self.faces.device:
            raise ValueError('fold_penalty: verts on %s, faces on %s' % (verts.device, self.faces.device))
        if verts.shape[0] > _lib.MESHCHECK_MAX_FRAMES or verts.shape[0] * max(self.keys.numel(), 1) > 0x7fffffff:
            raise ValueError('fold_penalty: %d meshes of %d pairs exceed the limits' % (verts.shape[0], self.keys.numel()))
        return _lib.f32(verts)

    def launch_forward(self, verts, want_rows):
        """-> (loss [N,2], values [N,n_list], rows [N,n_list,5,3] or an empty tensor)."""
        x = self._prepare(verts)
        dev, (N, V), n, F = x.device, x.shape[:2], self.keys.numel(), self.faces.shape[0]
        if N == 0 or n == 0 or F == 0:                                             # nothing is launched
            return (torch.zeros(N, 2, dtype=torch.float32, device=dev), torch.zeros(N, n, dtype=torch.float32, device=dev),
                    torch.zeros(0, dtype=torch.float32, device=dev))
        nbytes = int(_lib.lib().lasr_foldpen_scratch_bytes(N, n))
        scratch = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
        loss = torch.empty(N, 2, dtype=torch.float32, device=dev)
        values = torch.empty(N, n, dtype=torch.float32, device=dev)
        rows = torch.empty(N, n, SLOTS, 3, dtype=torch.float32, device=dev) if want_rows else None
        _lib.call('lasr_foldpen_forward', x, self.faces, self.keys, n, self.phi, values, rows, scratch, nbytes, loss, N, V, F, on=dev)
        return loss, values, rows if want_rows else torch.zeros(0, dtype=torch.float32, device=dev)

    def launch_backward(self, rows, grad_loss, shape):
        N, V = shape[:2]
        dev, n = self.faces.device, self.keys.numel()
        if N == 0 or V == 0:
            return torch.zeros(shape, dtype=torch.float32, device=dev)
        vstart, inc = self.index(V)
        if rows.numel() == 0:
            n = 0
        gverts = torch.empty(N, V, 3, dtype=torch.float32, device=dev)
        _lib.call('lasr_foldpen_backward', rows if n else None, vstart, inc if inc.numel() else None, inc.numel() if n else 0,
                  _lib.f32(grad_loss), gverts, N, V, n, on=dev)
        return gverts

    def entries(self, verts):
        """-> (loss [N,2], values [N,n_list]): the value of every list entry, without a gradient."""
        with torch.no_grad():
            loss, values, _ = self.launch_forward(verts, False)
        return loss, values

    def __call__(self, verts):
        return _Penalty.apply(self._prepare(verts), self)
