"""Keypoint transfer of scripts/eval_badja.py (reference: scripts/eval_badja.py:225-242) on lasr_kp_transfer (csrc/keypoints.hip).

Each keypoint of a reference frame moves with the flow of the nearest valid pixel of the H x W crop; the flow comes straight
from the colour planes of render_flow_soft_3's raster, read in place.  DESIGN.md section 4.5 states the arithmetic.
"""
import torch

from .. import _lib

MAX_JOINTS = 64                  # LASR_KP_MAX_JOINTS (include/lasr_ops.h)
MAX_SIZE = 16384                 # LASR_KP_MAX_SIZE


def kp_transfer(colors, kp, H, W):
    """colors [B,4,S,S] float32 (the raster of render_flow_soft_3, before its background fill), or None for the zero flow;
    kp [B,J,2] or [J,2] (row, col) in pixels of the top-left H x W crop.
    -> (idx int64 [B,J], pred float32 [B,J,2]): the flat index r * W + c of the pixel each keypoint takes its flow from, and
    (row + flow_y * H / 2, col + flow_x * W / 2), the reference's scaling (rows by H / 2 even for a non-square crop).
    With colors=None, B is kp's leading size."""
    if kp.dim() == 2:
        kp = kp[None].expand(colors.shape[0] if colors is not None else 1, -1, -1)
    if kp.dim() != 3 or kp.shape[2] != 2:
        raise ValueError('kp must be [B,J,2] or [J,2], got %s' % (tuple(kp.shape),))
    B, J = kp.shape[:2]
    if not 1 <= J <= MAX_JOINTS:
        raise ValueError('kp_transfer takes 1 to %d keypoints, got %d' % (MAX_JOINTS, J))
    _lib.need_cuda(kp, colors)
    S = None
    if colors is not None:
        if colors.dim() != 4 or colors.shape[0] != B or colors.shape[1] != 4 or colors.shape[2] != colors.shape[3]:
            raise ValueError('colors must be [B,4,S,S] with B = %d, got %s' % (B, tuple(colors.shape)))
        if colors.dtype != torch.float32:
            raise TypeError('colors must be float32')
        colors = colors.contiguous()
        S = int(colors.shape[2])
    else:
        S = max(int(H), int(W), 2)
    H, W = int(H), int(W)
    if not (2 <= S <= MAX_SIZE and 1 <= H <= S and 1 <= W <= S):
        raise ValueError('crop %dx%d does not fit the %d x %d raster (2 <= S <= %d)' % (H, W, S, S, MAX_SIZE))
    kp = kp.to(device=(colors if colors is not None else kp).device, dtype=torch.float32).contiguous()
    idx = torch.empty(B, J, dtype=torch.int64, device=kp.device)
    pred = torch.empty(B, J, 2, dtype=torch.float32, device=kp.device)
    _lib.call('lasr_kp_transfer', colors, kp, idx, pred, B, J, S, H, W)
    return idx, pred
