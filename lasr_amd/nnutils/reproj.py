"""Reprojection scores of a reconstruction (scripts/eval_reproj.py).

This is the project's own addition: the reference has no counterpart.  Per frame the predicted mesh is rasterised with its camera
and compared with what the loader was trained on: the annotation (region similarity J and boundary measure F, as DAVIS defines
them), the forward optical flow (end-point error of the rendered flow) and the frame's colours (PSNR of the vertex colours).
include/lasr_ops.h states the arithmetic of the three entry points (csrc/reproj.hip); the anchoring of a pixel on the surface is
the code of lasr_track_anchor.

Scenes are the posed sequences of lasr_amd/nnutils/posed.py, which states the conventions and holds the raster of side IS =
max(H, W).  Frames are walked CHUNK_FRAMES at a time (posed.py's default): one raster, the pixel pass with its reduce launch and
the two boundary launches per chunk.  The successor of a chunk's last frame is the first frame of the next chunk, and
every frame is scored on its own, so the result does not depend on the chunk size.
"""
import math

import numpy as np
import torch

from .. import _lib
from . import posed

CHUNK_FRAMES = posed.CHUNK_FRAMES
COUNTS = ('inter', 'union', 'n_pred', 'n_gt', 'n_pb', 'n_gb', 'pm', 'gm', 'n_flow', 'n_le1', 'n_le3', 'n_rgb')
DEFAULT_BOUND_TH = 0.008


def radius_of(bound_th, H, W):
    """Tolerance radius in pixels of the boundary measure: bound_th itself when it is at least 1 (a whole number of pixels), else
    ceil(bound_th * hypot(H, W)), DAVIS's share of the image diagonal; 0 means exact coincidence."""
    bound_th = float(bound_th)
    if not bound_th >= 0:
        raise ValueError('reproj: bound_th must be at least 0, got %r' % bound_th)
    if bound_th >= 1:
        if bound_th != int(bound_th):
            raise ValueError('reproj: a bound_th of 1 or more is a whole number of pixels, got %r' % bound_th)
        radius = int(bound_th)
    else:
        radius = int(math.ceil(bound_th * math.hypot(H, W)))
    if radius > _lib.REPROJ_MAX_RADIUS:
        raise ValueError('reproj: the boundary tolerance of %d pixels exceeds the limit of %d' % (radius, _lib.REPROJ_MAX_RADIUS))
    return radius


def _ratio(num, den):
    """num / den in float64, NaN where den is 0."""
    num, den = np.asarray(num, np.float64), np.asarray(den, np.float64)
    return np.where(den > 0, num / np.where(den > 0, den, 1.), np.nan)


def metrics(counts, sums):
    """counts [T,12] (COUNTS order) and sums [T,2] (sum of epe, sum of squared colour differences) -> dict of per-frame float64
    arrays J, precision, recall, F, epe, pck1, pck3, psnr; NaN where a denominator is 0 (no flow pixels, no colour pixels)."""
    c = {k: np.asarray(counts)[:, i].astype(np.float64) for i, k in enumerate(COUNTS)}
    sums = np.asarray(sums, np.float64)
    J = np.where(c['union'] > 0, c['inter'] / np.maximum(c['union'], 1.), 1.)
    P = np.where(c['n_pb'] > 0, c['pm'] / np.maximum(c['n_pb'], 1.), 1.)
    R = np.where(c['n_gb'] > 0, c['gm'] / np.maximum(c['n_gb'], 1.), 1.)
    P = np.where((c['n_gb'] == 0) & (c['n_pb'] > 0), 0., P)
    R = np.where((c['n_pb'] == 0) & (c['n_gb'] > 0), 0., R)
    F = np.where(P + R > 0, 2. * P * R / np.where(P + R > 0, P + R, 1.), 0.)
    with np.errstate(divide='ignore', invalid='ignore'):
        psnr = np.where(c['n_rgb'] > 0, 10. * np.log10(255. ** 2 * 3. * c['n_rgb'] / sums[:, 1]), np.nan)
    return dict(J=J, precision=P, recall=R, F=F, epe=_ratio(sums[:, 0], c['n_flow']), pck1=_ratio(c['n_le1'], c['n_flow']),
                pck3=_ratio(c['n_le3'], c['n_flow']), psnr=psnr)


def unpack_bits(words, W):
    """uint64 / int64 words [..., WW] of a bit map (column c = bit c & 63 of word c >> 6) -> bool [..., W], numpy on the host."""
    w = np.ascontiguousarray(np.asarray(words)).view(np.uint64)
    b = (w[..., :, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)
    return b.reshape(w.shape[:-1] + (-1,))[..., :W].astype(bool)


def evaluate(verts, faces, K, masks, flows=None, occs=None, frames=None, colors=None, bound_th=DEFAULT_BOUND_TH, raster=None):
    """verts [T,V,3] camera space, faces [F,3] (shared), K [T,4] = fx fy px py (pixels), masks [T,H,W] (non-zero = annotated
    foreground), flows [T-1,H,W,3] float (u, v, valid) from frame i to i + 1 and occs [T-1,H,W] (valid means channel 2 != 0 and
    occ < 10, the loader's rule; occs may be None alone), frames uint8 [T,H,W,3] with colors uint8 [T,V,3] (vertex colours per
    frame), bound_th the boundary tolerance (radius_of).  All on the device.  raster is a hook of the tests: a ready aggrs_info
    [T,2,IS,IS] in place of the hard-mode raster of verts.
    -> dict of per-frame numpy arrays: the twelve COUNTS (int64), J, precision, recall, F, epe, pck1, pck3, psnr (float64; NaN
    where a denominator is 0, so epe of the last frame is NaN) and radius; and on the device 'counts' int64 [T,12], 'sums'
    float64 [T,2], 'bits' and 'boundary_bits' int64 [T,2,H,WW] (maps pred, gt; unpack_bits reads them)."""
    named = (('masks', masks), ('flows', flows), ('occs', occs), ('frames', frames), ('colors', colors), ('raster', raster))
    for name, t in named:
        if t is not None and not torch.is_tensor(t):
            raise TypeError('reproj.evaluate: %s must be a tensor' % name)
    _lib.need_cuda(*(t for _, t in named))
    H, W = masks.shape[1:3] if masks.ndimension() == 3 else (1, 1)        # masks of another rank are refused below, by name
    seq = posed.sequence('reproj.evaluate', verts, faces, K, H, W, _lib.TRACK_MAX_SIZE)
    dev, verts, faces32, K = seq.device, seq.verts, seq.faces32, seq.K
    T, V, F, IS, H, W = seq.T, seq.V, seq.F, seq.IS, seq.H, seq.W
    if masks.ndimension() != 3 or masks.shape[0] != T:
        raise ValueError('reproj.evaluate: masks must be [T = %d, H, W], got %s' % (T, tuple(masks.shape)))
    radius = radius_of(bound_th, H, W)
    if occs is not None and flows is None:
        raise ValueError('reproj.evaluate: occs comes with flows')
    if flows is not None and (tuple(flows.shape) != (max(T - 1, 0), H, W, 3) or not flows.is_floating_point()):
        raise ValueError('reproj.evaluate: flows must be floating point [T - 1 = %d, %d, %d, 3], got %s %s'
                         % (max(T - 1, 0), H, W, flows.dtype, tuple(flows.shape)))
    if occs is not None and tuple(occs.shape) != (max(T - 1, 0), H, W):
        raise ValueError('reproj.evaluate: occs must be [T - 1 = %d, %d, %d], got %s' % (max(T - 1, 0), H, W, tuple(occs.shape)))
    if (frames is None) != (colors is None):
        raise ValueError('reproj.evaluate: frames and colors come together')
    if frames is not None:
        if frames.dtype != torch.uint8 or tuple(frames.shape) != (T, H, W, 3):
            raise ValueError('reproj.evaluate: frames must be uint8 [%d, %d, %d, 3], got %s %s' % (T, H, W, frames.dtype, tuple(frames.shape)))
        if colors.dtype != torch.uint8 or tuple(colors.shape) != (T, V, 3):
            raise ValueError('reproj.evaluate: colors must be uint8 [T = %d, V = %d, 3], got %s %s' % (T, V, colors.dtype, tuple(colors.shape)))
    if raster is not None and (tuple(raster.shape) != (T, 2, IS, IS) or raster.dtype != torch.float32):
        raise ValueError('reproj.evaluate: raster must be float32 [%d, 2, %d, %d], got %s %s' % (T, IS, IS, raster.dtype, tuple(raster.shape)))

    gt = (masks != 0).to(torch.uint8).contiguous()
    if flows is not None:
        flows = flows.detach().float().contiguous()
        occs = occs.detach().float().contiguous() if occs is not None else None
    if frames is not None:
        frames, colors = frames.contiguous(), colors.contiguous()
    WW = (W + 63) // 64
    counts = torch.zeros(T, len(COUNTS), dtype=torch.int64, device=dev)
    sums = torch.zeros(T, 2, dtype=torch.float64, device=dev)
    bits = torch.zeros(T, 2, H, WW, dtype=torch.int64, device=dev)
    bbits = torch.zeros(T, 2, H, WW, dtype=torch.int64, device=dev)
    for i, j, v, k, r in seq.chunks(CHUNK_FRAMES, raster=raster is None):
        n = j - i
        if raster is not None:
            r = raster[i:j].contiguous()
        vn = kn = fl = oc = None
        if flows is not None:
            if j < T:                                                 # the successor of the chunk's last frame opens the next chunk
                vn, kn, fl, oc = verts[i + 1:j + 1], K[i + 1:j + 1], flows[i:j], occs[i:j] if occs is not None else None
            else:                                                     # the last frame has none: its flow row is all invalid
                vn, kn = torch.cat([verts[i + 1:j], verts[j - 1:j]]), torch.cat([K[i + 1:j], K[j - 1:j]])
                fl = torch.cat([flows[i:j - 1], torch.zeros(1, H, W, 3, dtype=torch.float32, device=dev)])
                oc = torch.cat([occs[i:j - 1], torch.zeros(1, H, W, dtype=torch.float32, device=dev)]) if occs is not None else None
        ws = torch.empty(max(int(_lib.lib().lasr_reproj_workspace_bytes(n, H, W)), 8) // 8, dtype=torch.float64, device=dev)
        _lib.call('lasr_reproj_pixels', v, vn, faces32 if F else None, k, kn, r, gt[i:j], fl, oc,
                  frames[i:j] if frames is not None else None, colors[i:j] if colors is not None else None, bits[i:j], counts[i:j],
                  sums[i:j], ws, n, V, F, IS, H, W)
        _lib.call('lasr_reproj_boundary', bits[i:j], bbits[i:j], counts[i:j], n, H, W, radius)
    host_counts, host_sums = counts.cpu().numpy(), sums.cpu().numpy()
    out = {name: host_counts[:, s].copy() for s, name in enumerate(COUNTS)}
    out.update(metrics(host_counts, host_sums))
    out['radius'] = np.full(T, radius, np.int64)
    out.update(counts=counts, sums=sums, bits=bits, boundary_bits=bbits)
    return out
