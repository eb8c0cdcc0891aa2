"""Middlebury colour coding of optical flow (reference: third_party/ext_utils/flowlib.py:45-173 `flow_to_image`, `compute_color`,
`make_color_wheel`) on the device: lasr_flow_to_image of lasr_amd/csrc/flowvis.hip, two launches for a whole batch.  DESIGN.md
section 4.10 states the definition and where it departs from the reference (NaN samples, float32 arithmetic).

There is no CPU path: a numpy array is uploaded, coded on the HIP device and read back.
"""
import numpy as np
import torch

from .. import _lib

UNKNOWN_FLOW_THRESH = 1e7

_scratch = {}


def _stats_scratch(dev, B):
    """Zeroed statistics words of the device (the kernels leave them zero), grown on demand."""
    h = _lib.lib()
    need = h.lasr_flow_to_image_scratch_bytes(B) // 4
    key = (dev.type, dev.index if dev.index is not None else torch.cuda.current_device())
    buf = _scratch.get(key)
    if buf is None or buf.numel() < need:
        buf = _scratch[key] = torch.zeros(max(need, 64), dtype=torch.int32, device=dev)
    return buf


def flow_to_image(flow, mask=None):
    """flow: numpy [H,W,2|3] or device tensor [B,H,W,2|3] (channels 0, 1 = u, v) -> uint8 RGB of the same kind, [H,W,3] or
    [B,H,W,3].  mask (same leading shape, optional): u = v = 0 where it is 0, before the maximum radius is taken.  Every image is
    normalised by its own maximum radius."""
    is_np = isinstance(flow, np.ndarray)
    if is_np:
        if flow.ndim != 3:
            raise ValueError('flow_to_image: a numpy flow is [H,W,2|3], got %r' % (flow.shape,))
        if not torch.cuda.is_available():
            raise RuntimeError('flow_to_image needs a HIP device (there is no CPU path)')
        t = torch.from_numpy(np.ascontiguousarray(flow, dtype=np.float32)).cuda()[None]
        m = None if mask is None else torch.from_numpy(np.ascontiguousarray(mask, dtype=np.float32)).cuda()[None]
    else:
        t, m = flow, mask
        _lib.need_cuda(t, m)
        if t.ndim != 4:
            raise ValueError('flow_to_image: a tensor flow is [B,H,W,2|3], got %r' % (tuple(t.shape),))
    B, H, W, C = t.shape
    if C not in (2, 3):
        raise ValueError('flow_to_image: last dimension must hold 2 or 3 channels, got %d' % C)
    t = t.detach().float().contiguous()
    if m is not None:
        if tuple(m.shape) != (B, H, W):
            raise ValueError('flow_to_image: mask %r does not match flow %r' % (tuple(m.shape), (B, H, W)))
        m = m.detach().float().contiguous()
    out = torch.empty(B, H, W, 3, dtype=torch.uint8, device=t.device)
    if out.numel():
        _lib.call('lasr_flow_to_image', t, m, out, _stats_scratch(t.device, B), B, H, W, C)
    return out[0].cpu().numpy() if is_np else out
