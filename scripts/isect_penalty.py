"""The intersection penalty of the optimiser: optimize.py --isect_wt.

scripts/eval_shape.py reports three kinds of damage on a posed mesh: creased edge pairs, pierced vertex pairs, and intersecting pairs
of faces that share no vertex (n_pairs).  scripts/fold_penalty.py acts on the first two; this module is the loss that acts on the
third, on the posed meshes of every optimisation step.  The pairs are the report's own (faces i < j that share no vertex and whose
boxes overlap, the six strict directed edge-against-triangle tests), the value of a test that holds is the fold penalty's depth of
the shallower end of the piercing edge: linear, so that a descent step carries the end across the plane.  The penalty is zero exactly
where n_pairs is zero.  include/lasr_ops.h states the arithmetic, tests/isectpen_restated.py is the definition,
lasr_amd/csrc/isectpen.hip holds the kernels.  The pair set depends on the geometry of the step, so the contributions are added in
fixed point (2^40) by 64-bit integer atomics: the same bits on every run and under any order of the faces.  The trainer's default
(weight 0: off) is derived from nothing measured, and the effect on real footage is unverified.  The term clears shallow
pass-throughs; it does not separate two bodies that overlap wholesale.

All tensors live on the device.  A call launches three kernels (zero, pairs, finalise) and one broadcast multiply in the backward,
reads nothing on the host and allocates static shapes: it can be captured into a graph.
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from lasr_amd import _lib                       # noqa: E402


def _faces(faces):
    if not torch.is_tensor(faces):
        raise TypeError('isect_penalty: faces must be a tensor')
    _lib.need_cuda(faces)
    if faces.ndimension() != 2 or faces.shape[1] != 3 or faces.is_floating_point():
        raise ValueError('isect_penalty: faces must be integers [F,3], got %s %s' % (faces.dtype, tuple(faces.shape)))
    if faces.shape[0] > _lib.MESHCHECK_MAX_FACES:
        raise ValueError('isect_penalty: %d faces exceed the limit of %d' % (faces.shape[0], _lib.MESHCHECK_MAX_FACES))
    return faces.contiguous().int()


class _Penalty(torch.autograd.Function):
    @staticmethod
    def forward(ctx, verts, pen):
        want = ctx.needs_input_grad[0]
        loss, gunit, _, _ = pen.launch(verts, want)
        if want:
            ctx.save_for_backward(gunit)
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        gunit, = ctx.saved_tensors
        return grad_loss.float()[:, None, None] * gunit, None      # loss[n] is a plain sum: one broadcast multiply


class IsectPenalty:
    """IsectPenalty(faces [F,3])(verts [N,V,3]) -> [N]: per mesh the sum over its intersecting pairs of faces that share no vertex of
    the depths of the piercing edges, with a gradient by verts.  n_verts: the V of the calls to come (it sizes nothing here: a face
    with an index outside [0, V) takes part in nothing, so the indices are not read on the host)."""

    def __init__(self, faces, n_verts=None):
        self.faces = _faces(faces)
        if n_verts is not None and int(n_verts) < 0:
            raise ValueError('isect_penalty: n_verts must be at least 0, got %s' % n_verts)
        self.n_verts = None if n_verts is None else int(n_verts)

    def _prepare(self, verts):
        if not torch.is_tensor(verts):
            raise TypeError('isect_penalty: verts must be a tensor')
        _lib.need_cuda(verts)
        if verts.ndimension() != 3 or verts.shape[2] != 3 or not verts.is_floating_point():
            raise ValueError('isect_penalty: verts must be floating point [N,V,3], got %s %s' % (verts.dtype, tuple(verts.shape)))
        if verts.device != self.faces.device:
            raise ValueError('isect_penalty: verts on %s, faces on %s' % (verts.device, self.faces.device))
        N, V, F = verts.shape[0], verts.shape[1], self.faces.shape[0]
        if self.n_verts is not None and V != self.n_verts:
            raise ValueError('isect_penalty: built for meshes of %d vertices, got %d' % (self.n_verts, V))
        if N > _lib.MESHCHECK_MAX_FRAMES or N * F > 0x7fffffff or N * V * 3 > 0x7fffffff:
            raise ValueError('isect_penalty: %d meshes of %d vertices and %d faces exceed the limits' % (N, V, F))
        return _lib.f32(verts)

    def launch(self, verts, want_grad):
        """-> (loss [N] float32, gunit [N,V,3] float32 or None, n_pairs [N] int64, n_dropped [N] int64)."""
        x = self._prepare(verts)
        dev, (N, V), F = x.device, x.shape[:2], self.faces.shape[0]
        if N == 0 or F == 0 or V == 0:                                             # nothing is launched
            return (torch.zeros(N, dtype=torch.float32, device=dev), torch.zeros(N, V, 3, dtype=torch.float32, device=dev) if want_grad else None,
                    torch.zeros(N, dtype=torch.int64, device=dev), torch.zeros(N, dtype=torch.int64, device=dev))
        nbytes = int(_lib.lib().lasr_isectpen_scratch_bytes(N, V))
        scratch = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
        loss = torch.empty(N, dtype=torch.float32, device=dev)
        gunit = torch.empty(N, V, 3, dtype=torch.float32, device=dev) if want_grad else None
        n_pairs = torch.empty(N, dtype=torch.int64, device=dev)                    # the kernel's uint64 counts: below 2^40
        n_dropped = torch.empty(N, dtype=torch.int64, device=dev)
        _lib.call('lasr_isectpen_forward', x, self.faces, scratch, nbytes, loss, gunit, n_pairs, n_dropped, N, V, F, on=dev)
        return loss, gunit, n_pairs, n_dropped

    def counts(self, verts):
        """-> (n_pairs [N], n_dropped [N]) int64: the intersecting pairs as scripts/eval_shape.py counts them and the directed tests
        left out of the sums, without a gradient."""
        with torch.no_grad():
            _, _, n_pairs, n_dropped = self.launch(verts, False)
        return n_pairs, n_dropped

    def __call__(self, verts):
        return _Penalty.apply(self._prepare(verts), self)
