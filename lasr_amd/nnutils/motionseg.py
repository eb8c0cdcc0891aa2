"""Silhouettes from motion alone: the key masks of preprocess/auto_mask.py.

This is the project's own addition: the reference finds the object with a detector (preprocess/mask.py), which stays out of
scope.  Here the object is what moves differently from the camera.  Per ordered frame pair the forward-backward confidence of the
flow (lasr_motionseg_conf), `iters` IRLS iterations of an 8-parameter motion model whose sums and solve stay on the device
(lasr_motionseg_moments, lasr_motionseg_solve) and the evidence map (lasr_motionseg_evidence); per frame the summed evidence of its
two pairs, the mean field of maskprop.py, and on the host the largest component and a score.  The best-scoring frames become the
key masks maskprop.propagate starts from.

Nothing is read back inside a pair; per frame the host reads q once for the component filter and the evidence once for the score.
"""
import numpy as np
import torch

from .. import _lib
from . import maskprop

MODELS = {'translation': 0, 'affine': 1, 'quadratic': 2}
DEFAULTS = dict(tau=1., model='quadratic', iters=8, k_sigma=3., sigma_min=0.25, ridge=1e-9, kappa=4., U=6., gap=1, min_share=0.01,
                max_share=0.5, min_spacing=10, min_score=1., n_keys=1)


class NoMovingObject(ValueError):
    """No frame shows a region that moves against the dominant motion clearly enough."""


def params(**over):
    p = dict(DEFAULTS)
    unknown = set(over) - set(p)
    if unknown:
        raise TypeError('motionseg: unknown parameters %s' % sorted(unknown))
    p.update(over)
    if p['model'] not in MODELS:
        raise ValueError('motionseg: model must be one of %s, got %r' % (sorted(MODELS), p['model']))
    if int(p['iters']) < 0 or int(p['gap']) < 1 or int(p['n_keys']) < 1 or int(p['min_spacing']) < 0:
        raise ValueError('motionseg: iters >= 0, gap >= 1, n_keys >= 1 and min_spacing >= 0 are needed')
    return p


def _flow(t, name):
    if not torch.is_tensor(t):
        raise TypeError('motionseg: %s must be a tensor' % name)
    _lib.need_cuda(t)
    if t.ndimension() != 3 or t.shape[2] != 2:
        raise ValueError('motionseg: %s must be [H, W, 2], got %s' % (name, tuple(t.shape)))
    if t.shape[0] > _lib.MOTIONSEG_MAX_SIZE or t.shape[1] > _lib.MOTIONSEG_MAX_SIZE:
        raise ValueError('motionseg: a %d x %d field is too large (sides up to %d)' % (t.shape[0], t.shape[1], _lib.MOTIONSEG_MAX_SIZE))
    return t.detach().float().contiguous()


def _field(t, shape, name):
    if not torch.is_tensor(t):
        raise TypeError('motionseg: %s must be a tensor' % name)
    _lib.need_cuda(t)
    if tuple(t.shape) != tuple(shape):
        raise ValueError('motionseg: %s must be %s, got %s' % (name, tuple(shape), tuple(t.shape)))
    return t.detach().float().contiguous()


def _state(t):
    if not torch.is_tensor(t):
        raise TypeError('motionseg: state must be a tensor')
    _lib.need_cuda(t)
    if t.dtype != torch.float64 or tuple(t.shape) != (_lib.MOTIONSEG_STATE,) or not t.is_contiguous():
        raise ValueError('motionseg: state must be a contiguous float64 [%d] tensor' % _lib.MOTIONSEG_STATE)
    return t


def initial_state(device):
    s = torch.zeros(_lib.MOTIONSEG_STATE, dtype=torch.float64, device=device)
    s[8] = float('inf')
    return s


def confidence(f_ab, f_ba, tau=1.):
    """-> conf fp32 [H,W] of the pair a -> b: the forward-backward agreement of its flows (include/lasr_ops.h)."""
    f_ab = _flow(f_ab, 'f_ab')
    H, W = f_ab.shape[:2]
    f_ba = _field(f_ba, (H, W, 2), 'f_ba')
    conf = torch.empty(H, W, dtype=torch.float32, device=f_ab.device)
    _lib.call('lasr_motionseg_conf', f_ab, f_ba, conf, H, W, float(tau))
    return conf


def _sums(partials, hist):
    for t, dtype, shape, name in ((partials, torch.float64, (_lib.MOTIONSEG_BLOCKS, _lib.MOTIONSEG_MOMENTS), 'partials'),
                                  (hist, torch.int32, (_lib.MOTIONSEG_BINS,), 'hist')):
        if not torch.is_tensor(t):
            raise TypeError('motionseg: %s must be a tensor' % name)
        _lib.need_cuda(t)
        if t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError('motionseg: %s must be a contiguous %s %s tensor' % (name, dtype, list(shape)))


def moments(flow, conf, state, partials=None, hist=None):
    """The launches of one IRLS iteration before the solve.  -> (partials float64 [BLOCKS, MOMENTS], hist int32 [BINS], zeroed here)."""
    flow = _flow(flow, 'flow')
    H, W = flow.shape[:2]
    conf, state = _field(conf, (H, W), 'conf'), _state(state)
    if partials is None:
        partials = torch.empty(_lib.MOTIONSEG_BLOCKS, _lib.MOTIONSEG_MOMENTS, dtype=torch.float64, device=flow.device)
    if hist is None:
        hist = torch.empty(_lib.MOTIONSEG_BINS, dtype=torch.int32, device=flow.device)
    _sums(partials, hist)
    hist.zero_()
    _lib.call('lasr_motionseg_moments', flow, conf, state, partials, hist, H, W)
    return partials, hist


def solve(partials, hist, state, H, W, model='quadratic', k_sigma=3., sigma_min=0.25, ridge=1e-9):
    """state <- the next IRLS state, on the device.  -> state."""
    _sums(partials, hist)
    _lib.call('lasr_motionseg_solve', partials, hist, _state(state), int(H), int(W), MODELS[model], float(k_sigma), float(sigma_min),
              float(ridge))
    return state


def fit(flow, conf, model='quadratic', iters=8, k_sigma=3., sigma_min=0.25, ridge=1e-9, state=None):
    """`iters` IRLS iterations (a memset, the moments, the solve) from `state` (default theta = 0, sigma = inf), without a host
    synchronisation.  -> the state tensor, float64 [12] on the device: theta[8], sigma, med, n, status."""
    flow = _flow(flow, 'flow')
    H, W = flow.shape[:2]
    conf = _field(conf, (H, W), 'conf')
    if model not in MODELS:
        raise ValueError('motionseg: model must be one of %s, got %r' % (sorted(MODELS), model))
    state = initial_state(flow.device) if state is None else _state(state).clone()
    partials = hist = None
    for _ in range(int(iters)):
        partials, hist = moments(flow, conf, state, partials, hist)
        solve(partials, hist, state, H, W, model, k_sigma, sigma_min, ridge)
    return state


def evidence(flow, conf, state, kappa=4., U=6., out=None):
    """-> e fp32 [H,W] = conf clamp(r^2 / sigma^2 - kappa, -U, U); with `out` the evidence is added to it."""
    flow = _flow(flow, 'flow')
    H, W = flow.shape[:2]
    conf, state = _field(conf, (H, W), 'conf'), _state(state)
    acc = out is not None
    if acc:
        _lib.need_cuda(out)
        if out.dtype != torch.float32 or tuple(out.shape) != (H, W) or not out.is_contiguous():
            raise ValueError('motionseg: out must be a contiguous float32 [%d, %d] tensor' % (H, W))
    else:
        out = torch.empty(H, W, dtype=torch.float32, device=flow.device)
    _lib.call('lasr_motionseg_evidence', flow, conf, state, out, H, W, float(kappa), float(U), int(acc))
    return out


def largest_component(fg):
    """numpy bool [H,W] -> its largest 8-connected component (the lowest label among equals); all False when fg is empty."""
    from scipy import ndimage
    lab, n = ndimage.label(fg, structure=np.ones((3, 3), int))
    if n == 0:
        return np.zeros(fg.shape, bool)
    area = np.bincount(lab.ravel(), minlength=n + 1)
    area[0] = 0
    return lab == int(np.argmax(area))


def score(u, P, fits_ok, p):
    """The score of a frame (float64 on the host): 0 when a fit is degenerate, no pair exists or the mask's share of the frame is
    outside [min_share, max_share]; else (mean u inside P - mean u outside) (1 - b), b = the part of P's boundary on the frame's rim."""
    from scipy import ndimage
    share = float(P.mean())
    if not fits_ok or not p['min_share'] <= share <= p['max_share']:
        return 0.
    u = np.asarray(u, np.float64)
    edge = P & ~ndimage.binary_erosion(P, structure=np.ones((3, 3), bool), border_value=0)
    rim = np.zeros(P.shape, bool)
    rim[0, :], rim[-1, :], rim[:, 0], rim[:, -1] = True, True, True, True
    b = min(1., float((P & rim).sum()) / float(edge.sum()))
    return float((u[P].mean() - u[~P].mean()) * (1 - b))


def select_keys(scores, p):
    """Greedy by descending score, ties to the lower index; a frame within min_spacing of a chosen key is skipped; stops at n_keys
    or at the first score below min_score.  -> the sorted key frames; raises NoMovingObject when there is none."""
    keys = []
    for t in sorted(range(len(scores)), key=lambda t: (-scores[t], t)):
        if len(keys) >= int(p['n_keys']) or scores[t] < p['min_score']:
            break
        if all(abs(t - k) >= int(p['min_spacing']) for k in keys):
            keys.append(t)
    if not keys:
        raise NoMovingObject('no frame shows a region that moves against the dominant motion (best score %.3g, min_score %g)'
                             % (max(scores) if len(scores) else 0., p['min_score']))
    return sorted(keys)


def caching_flow_fn(flow_fn):
    """flow_fn(imgA, imgB) memoised on the content of the frame pair: maskprop.propagate builds its own video, and the flows
    computed for the keys must not be computed again.  .calls counts the calls that reached flow_fn."""
    cache = {}

    def cached(imgA, imgB):
        key = (np.ascontiguousarray(imgA).tobytes(), np.ascontiguousarray(imgB).tobytes())
        if key not in cache:
            cached.calls += 1
            cache[key] = flow_fn(imgA, imgB)
        return cache[key]
    cached.calls = 0
    return cached


def segment(frames, flow_fn, device='cuda', **over):
    """frames uint8 [T,H,W,3] (array or list), flow_fn(imgA, imgB) -> (flow A -> B [H,W,>=2] in pixels, occ) as auto_gen.run takes
    it.  -> (masks [T,H,W] bool, soft [T,H,W] float32 = q after the mean field, scores float64 [T], report) as numpy arrays; the
    report holds the parameters, the scores and theta, sigma, n, status of every ordered pair."""
    p = params(**over)
    mp = maskprop.params()
    video = maskprop._Video(frames, flow_fn, torch.device(device))
    T, g = video.T, int(p['gap'])
    masks, soft, scores, pairs = [], [], [], []
    for t in range(T):
        u, states = None, []
        for s in (t - g, t + g):
            if not 0 <= s < T:
                continue
            f = video.flow(t, s)
            c = confidence(f, video.flow(s, t), p['tau'])
            S = fit(f, c, p['model'], p['iters'], p['k_sigma'], p['sigma_min'], p['ridge'])
            u = evidence(f, c, S, p['kappa'], p['U'], out=u)
            states.append((s, S))
        if u is None:
            u = torch.zeros(video.H, video.W, dtype=torch.float32, device=video.device)
        q = maskprop.meanfield(video.dev[t], u, torch.sigmoid(u), mp['K'], mp['R'], mp['sigma_i'], mp['sigma_s'], mp['w_s'])
        P = largest_component(q.cpu().numpy() > 0.5)
        ok = bool(states)
        for s, S in states:
            S = S.cpu().numpy()
            ok = ok and S[11] == 0
            pairs.append(dict(frame=t, to=s, theta=[float(v) for v in S[:8]], sigma=float(S[8]), n=int(S[10]), status=int(S[11])))
        masks.append(P)
        soft.append(q.cpu().numpy())
        scores.append(score(u.cpu().numpy(), P, ok, p))
    report = dict(params=p, scores=[float(v) for v in scores], pairs=pairs, flow_pairs=len(video.flows))
    return np.stack(masks), np.stack(soft), np.array(scores, np.float64), report


def auto_keys(frames, flow_fn, device='cuda', report=None, **over):
    """-> {t: bool mask} of the chosen key frames; raises NoMovingObject.  `report`, a dict, receives segment's report and 'keys'."""
    masks, _, scores, rep = segment(frames, flow_fn, device, **over)
    keys = select_keys(list(scores), rep['params'])
    if report is not None:
        report.update(rep, keys=keys)
    return {t: masks[t] for t in keys}
