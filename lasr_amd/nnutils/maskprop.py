"""Carry an annotated silhouette through a video along the optical flow (preprocess/propagate_mask.py).

This is the project's own addition: the reference fills Annotations/ with a detector (preprocess/mask.py), which stays out of
scope.  Here the user paints the object in one frame, or a few, and every other frame's mask is reached step by step: colour
histograms of the source frame (lasr_maskprop_hist), a unary field from the backward warp, the forward-backward flow consistency
and the histograms' log ratio (lasr_maskprop_unary), K edge-aware mean-field iterations (lasr_maskprop_meanfield), and on the host
a connected-component filter, because the loader crops by the mask's bounding box and a stray speck would widen it.

Frames and state stay on the device.  Per step the host computes the histogram window, launches the kernels and reads the final
q once for the component filter (scipy.ndimage.label, 8-connectivity).
"""
import numpy as np
import torch

from .. import _lib

DEFAULTS = dict(hi=0.9, lo=0.1, tau=1., w_p=1., w_a=0.5, eps=1e-3, U=6., R=4, sigma_i=12., sigma_s=3., w_s=0.3, K=5,
                min_component=0.05)


class EmptyPropagation(ValueError):
    """A propagated mask became empty; .frame is the index of the frame."""

    def __init__(self, frame):
        ValueError.__init__(self, 'the propagated mask of frame %d is empty: annotate a frame closer to it (another --key)' % frame)
        self.frame = frame


def params(**over):
    p = dict(DEFAULTS)
    unknown = set(over) - set(p)
    if unknown:
        raise TypeError('maskprop: unknown parameters %s' % sorted(unknown))
    p.update(over)
    if not 0 <= int(p['R']) <= _lib.MASKPROP_MAX_RADIUS:
        raise ValueError('maskprop: R must be 0..%d, got %s' % (_lib.MASKPROP_MAX_RADIUS, p['R']))
    if int(p['K']) < 0:
        raise ValueError('maskprop: K must be >= 0, got %s' % p['K'])
    return p


def window_of(P):
    """(x0, y0, x1, y1) of the histogram window: the bounding box of P > 0.5 grown by half its width / height plus 8 px, clipped
    to the image; None when nothing is above 0.5.  P is a numpy array or a tensor."""
    fg = (P > 0.5)
    fg = fg.cpu().numpy() if torch.is_tensor(fg) else np.asarray(fg)
    ys, xs = np.nonzero(fg)
    if xs.size == 0:
        return None
    H, W = fg.shape
    w, h = int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1)
    return (max(0, int(xs.min()) - w // 2 - 8), max(0, int(ys.min()) - h // 2 - 8),
            min(W, int(xs.max()) + 1 + w // 2 + 8), min(H, int(ys.max()) + 1 + h // 2 + 8))


def component_filter(q, min_component=0.05):
    """numpy q [H,W] -> q * (the 8-connected components of q > 0.5 whose area is at least min_component times the largest)."""
    from scipy import ndimage
    lab, n = ndimage.label(q > 0.5, structure=np.ones((3, 3), int))
    if n == 0:
        return q * 0
    area = np.bincount(lab.ravel(), minlength=n + 1)
    area[0] = 0
    keep = area >= min_component * area.max()
    keep[0] = False
    return q * keep[lab]


def _image(img, name):
    if not torch.is_tensor(img):
        raise TypeError('maskprop: %s must be a tensor' % name)
    _lib.need_cuda(img)
    if img.dtype != torch.uint8 or img.ndimension() != 3 or img.shape[2] != 3:
        raise ValueError('maskprop: %s must be uint8 [H, W, 3], got %s %s' % (name, img.dtype, tuple(img.shape)))
    H, W = int(img.shape[0]), int(img.shape[1])
    if H > _lib.MASKPROP_MAX_SIZE or W > _lib.MASKPROP_MAX_SIZE or 3 * H * W > 0x7fffffff:
        raise ValueError('maskprop: a %d x %d image is too large (sides up to %d)' % (H, W, _lib.MASKPROP_MAX_SIZE))
    return img.contiguous()


def _field(t, shape, name):
    if not torch.is_tensor(t):
        raise TypeError('maskprop: %s must be a tensor' % name)
    _lib.need_cuda(t)
    if tuple(t.shape) != tuple(shape):
        raise ValueError('maskprop: %s must be %s, got %s' % (name, tuple(shape), tuple(t.shape)))
    return t.detach().float().contiguous()


def histogram(img, P, window, hist=None, hi=0.9, lo=0.1):
    """Adds the colour counts of the window (x0, y0, x1, y1) of img to hist (uint32 [2, 4096] as an int32 tensor: row 1 counts
    P >= hi, row 0 P <= lo); hist None starts from zero.  -> hist."""
    img = _image(img, 'img')
    H, W = img.shape[:2]
    P = _field(P, (H, W), 'P')
    if hist is None:
        hist = torch.zeros(2, _lib.MASKPROP_BINS, dtype=torch.int32, device=img.device)
    elif hist.dtype != torch.int32 or tuple(hist.shape) != (2, _lib.MASKPROP_BINS) or not hist.is_contiguous():
        raise ValueError('maskprop: hist must be a contiguous int32 [2, %d] tensor' % _lib.MASKPROP_BINS)
    _lib.need_cuda(hist)
    x0, y0, x1, y1 = (int(v) for v in window)
    _lib.call('lasr_maskprop_hist', img, P, hist, H, W, x0, y0, x1, y1, float(hi), float(lo))
    return hist


def unary(img_t, P_s, flow_ts, flow_st, hist, tau=1., w_p=1., w_a=0.5, eps=1e-3, U=6.):
    """-> (u, q0), fp32 [H,W]: the unary logit of frame t and its sigmoid (include/lasr_ops.h)."""
    img_t = _image(img_t, 'img_t')
    H, W = img_t.shape[:2]
    P_s = _field(P_s, (H, W), 'P_s')
    flow_ts, flow_st = _field(flow_ts, (H, W, 2), 'flow_ts'), _field(flow_st, (H, W, 2), 'flow_st')
    if hist.dtype != torch.int32 or tuple(hist.shape) != (2, _lib.MASKPROP_BINS):
        raise ValueError('maskprop: hist must be an int32 [2, %d] tensor' % _lib.MASKPROP_BINS)
    _lib.need_cuda(hist)
    hist = hist.contiguous()
    dev = img_t.device
    table = torch.empty(_lib.MASKPROP_BINS, dtype=torch.float32, device=dev)
    u, q0 = torch.empty(H, W, dtype=torch.float32, device=dev), torch.empty(H, W, dtype=torch.float32, device=dev)
    _lib.call('lasr_maskprop_unary', img_t, P_s, flow_ts, flow_st, hist, table, u, q0, H, W, float(tau), float(w_p), float(w_a),
              float(eps), float(U))
    return u, q0


def meanfield(img, u, q, K=5, R=4, sigma_i=12., sigma_s=3., w_s=0.3, every=False):
    """K edge-aware mean-field iterations from q, ping-pong between two buffers, one launch each.  -> q after K iterations (q
    itself for K = 0), or with every=True the list of the K intermediate fields."""
    img = _image(img, 'img')
    H, W = img.shape[:2]
    u, q = _field(u, (H, W), 'u'), _field(q, (H, W), 'q')
    out = []
    bufs = [torch.empty_like(q), torch.empty_like(q)]
    for k in range(int(K)):
        dst = torch.empty_like(q) if every else bufs[k & 1]
        _lib.call('lasr_maskprop_meanfield', img, u, q, dst, H, W, int(R), float(sigma_i), float(sigma_s), float(w_s))
        q = dst
        out.append(q)
    return out if every else q


def step(img_s, img_t, P_s, flow_ts, flow_st, key_hist, p):
    """One propagation step s -> t on the device.  -> q [H,W] fp32 before the component filter."""
    win = window_of(P_s)
    hist = key_hist.clone()
    if win is not None:
        histogram(img_s, P_s, win, hist, p['hi'], p['lo'])
    u, q = unary(img_t, P_s, flow_ts, flow_st, hist, p['tau'], p['w_p'], p['w_a'], p['eps'], p['U'])
    return meanfield(img_t, u, q, p['K'], p['R'], p['sigma_i'], p['sigma_s'], p['w_s'])


class _Video:
    """The frames on the device and on the host, and the flows of the ordered frame pairs asked for so far."""

    def __init__(self, frames, flow_fn, device):
        self.host = [np.array(f, copy=True, order='C') for f in frames]     # own, writable copies (PIL hands out read-only views)
        if not self.host:
            raise ValueError('maskprop: no frames')
        shape = self.host[0].shape
        for f in self.host:
            if f.dtype != np.uint8 or f.ndim != 3 or f.shape != shape or shape[2] != 3:
                raise ValueError('maskprop: frames must be uint8 [H, W, 3] of one size')
        self.dev = [torch.from_numpy(f).to(device) for f in self.host]
        self.flow_fn, self.device, self.flows = flow_fn, device, {}
        self.H, self.W, self.T = shape[0], shape[1], len(self.host)

    def flow(self, a, b):
        if (a, b) not in self.flows:
            f = self.flow_fn(self.host[a], self.host[b])[0]
            f = f if torch.is_tensor(f) else torch.from_numpy(np.ascontiguousarray(np.asarray(f)[..., :2], dtype=np.float32))
            f = f[..., :2].float().to(self.device).contiguous()
            if tuple(f.shape) != (self.H, self.W, 2):
                raise ValueError('maskprop: flow_fn returned %s for %d x %d frames' % (tuple(f.shape), self.H, self.W))
            self.flows[(a, b)] = f
        return self.flows[(a, b)]


def _filtered(q, p, frame):
    """Device q -> (device P = q * kept components, its area); raises when nothing is left."""
    P = component_filter(q.cpu().numpy(), p['min_component'])
    area = int((P > 0.5).sum())
    if area == 0:
        raise EmptyPropagation(frame)
    return torch.from_numpy(P).to(q.device), area


def _chain(video, start, P0, stop, key_hist, p):
    """From frame start (soft mask P0 on the device) to frame stop inclusive.  -> {t: q before the filter}; the state carried on
    is the filtered q."""
    out, P, s = {}, P0, start
    d = 1 if stop > start else -1
    while s != stop:
        t = s + d
        q = step(video.dev[s], video.dev[t], P, video.flow(t, s), video.flow(s, t), key_hist, p)
        P, _ = _filtered(q, p, t)
        out[t] = q
        s = t
    return out


def _key_histogram(video, key_masks, p):
    hist = torch.zeros(2, _lib.MASKPROP_BINS, dtype=torch.int32, device=video.device)
    for k, P in key_masks.items():
        win = window_of(P)
        if win is None:
            raise ValueError('maskprop: the annotation of frame %d is empty' % k)
        histogram(video.dev[k], P, win, hist, p['hi'], p['lo'])
    return hist


def _keys(key_masks, video):
    out = {}
    for k, m in key_masks.items():
        k = int(k)
        m = m.cpu().numpy() if torch.is_tensor(m) else np.asarray(m)
        if not 0 <= k < video.T or m.shape != (video.H, video.W):
            raise ValueError('maskprop: key %d must be a [%d, %d] mask of one of the %d frames' % (k, video.H, video.W, video.T))
        out[k] = torch.from_numpy((m > 0).astype(np.float32)).to(video.device)
    if not out:
        raise ValueError('maskprop: at least one key mask is needed')
    return dict(sorted(out.items()))


def _logit(q):
    q = q.clamp(1e-6, 1 - 1e-6)
    return torch.log(q / (1 - q))


def propagate(frames, key_masks, flow_fn, device='cuda', **over):
    """frames uint8 [T,H,W,3] (array or list), key_masks {frame index: bool mask}, flow_fn(imgA, imgB) -> (flow A -> B [H,W,>=2] in
    pixels, occ) as auto_gen.run takes it.  -> (masks [T,H,W] bool, soft [T,H,W] float32, report) as numpy arrays.
    One key: a pass forward and a pass backward from it.  Several: a frame between the keys a < b is reached from both, and the two
    logit fields are averaged with weights (b-t)/(b-a) and (t-a)/(b-a) before the threshold and the filter; key frames keep their
    annotation.  Raises EmptyPropagation when a propagated mask becomes empty."""
    p = params(**over)
    video = _Video(frames, flow_fn, torch.device(device))
    keys = _keys(key_masks, video)
    order = list(keys)
    kh = _key_histogram(video, keys, p)
    soft = torch.zeros(video.T, video.H, video.W, dtype=torch.float32, device=video.device)
    for k, P in keys.items():
        soft[k] = P
    ends = [(order[0], 0), (order[-1], video.T - 1)]
    for start, stop in ends:
        for t, q in _chain(video, start, keys[start], stop, kh, p).items():
            soft[t] = _filtered(q, p, t)[0]
    for a, b in zip(order[:-1], order[1:]):
        if b - a < 2:
            continue
        fw, bw = _chain(video, a, keys[a], b - 1, kh, p), _chain(video, b, keys[b], a + 1, kh, p)
        for t in range(a + 1, b):
            wa, wb = float(b - t) / (b - a), float(t - a) / (b - a)
            q = torch.sigmoid(wa * _logit(fw[t]) + wb * _logit(bw[t]))
            soft[t] = _filtered(q, p, t)[0]
    soft = soft.cpu().numpy()
    masks = soft > 0.5
    report = dict(params=p, keys=order, areas=[int(m.sum()) for m in masks], flow_pairs=len(video.flows))
    return masks, soft, report


def roundtrip(frames, key, mask, flow_fn, device='cuda', **over):
    """A diagnostic for a video without ground truth: one pass from the key frame to the last frame, then back to the key frame.
    -> the IoU of what returns with the annotation (1.0 when the key is the last frame: there is nothing to traverse)."""
    p = params(**over)
    video = _Video(frames, flow_fn, torch.device(device))
    keys = _keys({key: mask}, video)
    key = next(iter(keys))
    kh = _key_histogram(video, keys, p)
    P = keys[key]
    last = video.T - 1
    if key != last:
        P, _ = _filtered(_chain(video, key, P, last, kh, p)[last], p, last)
        P, _ = _filtered(_chain(video, last, P, key, kh, p)[key], p, key)
    a, b = (P > 0.5), (keys[key] > 0.5)
    return float((a & b).sum()) / max(float((a | b).sum()), 1.)
