"""chamfer_3DFunction / chamfer_3DDist with the reference's call shape (/root/reference/third_party/chamfer3D/dist_chamfer_3D.py:26-74):

    dist1, dist2, idx1, idx2 = chamfer_3DDist()(input1, input2)        # [N,P,3], [N,Q,3] -> [N,P], [N,Q], int32 [N,P], [N,Q]

Squared distances to, and indices of, the nearest point of the other set (lowest index on ties); both inputs receive gradients
with the indices fixed, the indices none.  The searches run on the tiled kernel of lasr_amd/csrc/chamfer.hip (lasr_nn_tiled), the
backward on a gather over the inverse index maps, so two backward calls give the same bits (the reference scatters with atomics).
GPU tensors only.  The kernels are fp32: inputs of another floating dtype are cast to float32, distances and gradients come back as
float32 whatever the inputs were (the reference's extension takes float32 only).  chamfer_3DFunction.apply takes a third argument,
the split count of the search (0: chosen by the library), which the tests use to force the merge path; chamfer_3DDist passes 0."""
import torch
from torch import nn
from torch.autograd import Function

from .. import _lib

NN_TILE = _lib.NN_TILE                                          # target points per LDS tile of the search (LASR_NN_TILE)


def _workspace(nbytes, dev):
    return torch.empty(max(int(nbytes), 8) // 8, dtype=torch.int64, device=dev)


def nn_tiled(a, b, R=None, T=None, splits=0):
    """a [N,P,3], b [N,Q,3] -> (squared distance [N,P], index [N,P] int32) of the nearest b point of every a R + T (row vectors;
    R [N,3,3], T [N,3] on the device, or neither).  splits: runs of the target set searched by separate blocks and merged; 0 lets
    the library choose.  Not differentiable."""
    _lib.need_cuda(a, b, R, T)
    if (R is None) != (T is None):
        raise ValueError('R and T come together')
    a, b = _lib.f32(a.detach(), b.detach())
    if a.dim() != 3 or b.dim() != 3 or a.shape[2] != 3 or b.shape[2] != 3 or a.shape[0] != b.shape[0]:
        raise ValueError('expected a [N,P,3] and b [N,Q,3], got %s and %s' % (tuple(a.shape), tuple(b.shape)))
    N, P, Q = a.shape[0], a.shape[1], b.shape[1]
    if R is not None:
        R, T = _lib.f32(R.detach(), T.detach())
        if R.shape != (N, 3, 3) or T.shape != (N, 3):
            raise ValueError('expected R [N,3,3] and T [N,3]')
    h = _lib.lib()
    d2 = torch.empty(N, P, dtype=torch.float32, device=a.device)
    idx = torch.empty(N, P, dtype=torch.int32, device=a.device)
    nbytes = h.lasr_chamfer3d_workspace_bytes(N, P, 0)
    ws = _workspace(nbytes, a.device)
    _lib.call('lasr_nn_tiled', a, b, R, T, d2, idx, ws, nbytes, N, P, Q, splits)
    return d2, idx


def _inverse_csr(idx, rows):
    """idx int32 [N,M] with values in [0, rows) -> (row_ptr int32 [N,rows+1], col int32 [N,M]): for every value the positions that
    hold it, ascending (a stable sort)."""
    key, col = torch.sort(idx, dim=1, stable=True)
    bounds = torch.arange(rows + 1, device=idx.device, dtype=key.dtype).expand(idx.shape[0], -1).contiguous()
    row_ptr = torch.searchsorted(key.contiguous(), bounds)
    return row_ptr.int().contiguous(), col.int().contiguous()


class chamfer_3DFunction(Function):
    @staticmethod
    def forward(ctx, xyz1, xyz2, splits):
        _lib.need_cuda(xyz1, xyz2)
        if xyz1.dim() != 3 or xyz2.dim() != 3 or xyz1.shape[2] != 3 or xyz2.shape[2] != 3 or xyz1.shape[0] != xyz2.shape[0]:
            raise ValueError('expected [N,P,3] and [N,Q,3], got %s and %s' % (tuple(xyz1.shape), tuple(xyz2.shape)))
        x1, x2 = _lib.f32(xyz1.detach(), xyz2.detach())
        N, P, Q = x1.shape[0], x1.shape[1], x2.shape[1]
        dev = x1.device
        h = _lib.lib()
        dist1, dist2 = torch.empty(N, P, dtype=torch.float32, device=dev), torch.empty(N, Q, dtype=torch.float32, device=dev)
        idx1, idx2 = torch.empty(N, P, dtype=torch.int32, device=dev), torch.empty(N, Q, dtype=torch.int32, device=dev)
        nbytes = h.lasr_chamfer3d_workspace_bytes(N, P, Q)
        ws = _workspace(nbytes, dev)
        _lib.call('lasr_chamfer3d_forward', x1, x2, dist1, dist2, idx1, idx2, ws, nbytes, N, P, Q, splits)
        ctx.save_for_backward(x1, x2, idx1, idx2)
        ctx.mark_non_differentiable(idx1, idx2)
        return dist1, dist2, idx1, idx2

    @staticmethod
    def backward(ctx, graddist1, graddist2, _gradidx1=None, _gradidx2=None):
        x1, x2, idx1, idx2 = ctx.saved_tensors
        N, P, Q = x1.shape[0], x1.shape[1], x2.shape[1]
        g1 = graddist1.contiguous().float() if graddist1 is not None else torch.zeros(N, P, device=x1.device)
        g2 = graddist2.contiguous().float() if graddist2 is not None else torch.zeros(N, Q, device=x1.device)
        row_ptr1, col1 = _inverse_csr(idx2, P)                  # per xyz1 point: the xyz2 points that chose it
        row_ptr2, col2 = _inverse_csr(idx1, Q)
        gx1, gx2 = torch.empty_like(x1), torch.empty_like(x2)
        _lib.call('lasr_chamfer3d_backward', x1, x2, idx1, idx2, g1, g2, row_ptr1, col1, row_ptr2, col2, gx1, gx2, N, P, Q)
        return gx1, gx2, None


class chamfer_3DDist(nn.Module):
    def __init__(self):
        super(chamfer_3DDist, self).__init__()

    def forward(self, input1, input2):
        return chamfer_3DFunction.apply(input1, input2, 0)
