"""Classical variational optical flow on the device (preprocess/auto_gen.py --flow_method variational).

This is the project's own addition: the reference estimates flow with a network whose checkpoint is a download.  Here the flow
needs no learned weights: a coarse-to-fine, warping, robust variational estimate (Brox et al. 2004, simplified to brightness
constancy) solved by red-black SOR, one kernel per stage (include/lasr_ops.h, lasr_amd/csrc/varflow.hip): a Burt-Adelson pyramid
(lasr_varflow_reduce), flow upsampling (lasr_varflow_expand), the linearisation around the current flow (lasr_varflow_tensor), the
lagged robust weights (lasr_varflow_weights), the solver (lasr_varflow_sor) and the forward-backward consistency map written
where VCN's occlusion map is (lasr_varflow_occ).  The definition is tests/varflow_restated.py.

Everything takes device tensors and stays on the device; flow() launches and never synchronises.  Inside the solver a flow field is
planar [2,H,W] = (u, v) in pixels; flow() and occlusion() speak the public layout [H,W,2], I1(p) ~ I2(p + f(p)).
"""
import numpy as np
import torch

from .. import _lib

DEFAULTS = dict(alpha=0.03, eps=1e-3, omega=1.8, NW=5, NO=3, NI=10)
OCC_TAU, OCC_S = 1.0, 0.5


def params(**over):
    p = dict(DEFAULTS)
    unknown = set(over) - set(p)
    if unknown:
        raise TypeError('varflow: unknown parameters %s' % sorted(unknown))
    p.update(over)
    if not (float(p['alpha']) > 0 and float(p['eps']) > 0 and 0 < float(p['omega']) < 2):
        raise ValueError('varflow: alpha and eps must be positive and omega inside (0, 2), got %s' % p)
    if min(int(p['NW']), int(p['NO']), int(p['NI'])) < 1:
        raise ValueError('varflow: NW, NO and NI must be at least 1, got %s' % p)
    return p


def level_shapes(H, W):
    """[(H, W), (ceil(H/2), ceil(W/2)), ...]: REDUCE repeats while the smaller side of the last level is >= 32."""
    out = [(int(H), int(W))]
    while min(out[-1]) >= 32:
        h, w = out[-1]
        out.append(((h + 1) // 2, (w + 1) // 2))
    return out


def _sides(H, W, what):
    if not (_lib.VARFLOW_MIN_SIZE <= H <= _lib.VARFLOW_MAX_SIZE and _lib.VARFLOW_MIN_SIZE <= W <= _lib.VARFLOW_MAX_SIZE):
        raise ValueError('varflow: %s is %d x %d, sides must be %d..%d' % (what, H, W, _lib.VARFLOW_MIN_SIZE, _lib.VARFLOW_MAX_SIZE))


def _f32(t, shape, name):
    if not torch.is_tensor(t):
        raise TypeError('varflow: %s must be a tensor' % name)
    _lib.need_cuda(t)
    if tuple(t.shape) != tuple(shape):
        raise ValueError('varflow: %s must be %s, got %s' % (name, tuple(shape), tuple(t.shape)))
    return t.detach().float().contiguous()


def _planar(t, name, sides=True):
    """A planar field [2,H,W]; sides=False: H or W may be 1 (the coarse input of expand)."""
    if not torch.is_tensor(t):
        raise TypeError('varflow: %s must be a tensor' % name)
    _lib.need_cuda(t)
    if t.ndimension() != 3 or t.shape[0] != 2:
        raise ValueError('varflow: %s must be [2, H, W], got %s' % (name, tuple(t.shape)))
    if sides:
        _sides(int(t.shape[1]), int(t.shape[2]), name)
    return t.detach().float().contiguous()


def reduce(img):
    """uint8 [H,W,3] -> (level0 fp32 [H,W,3] = img / 255, its REDUCE [ceil(H/2), ceil(W/2), 3]); fp32 [H,W,3] -> its REDUCE."""
    if not torch.is_tensor(img):
        raise TypeError('varflow: img must be a tensor')
    _lib.need_cuda(img)
    if img.ndimension() != 3 or img.shape[2] != 3 or img.dtype not in (torch.uint8, torch.float32):
        raise ValueError('varflow: img must be uint8 or float32 [H, W, 3], got %s %s' % (img.dtype, tuple(img.shape)))
    H, W = int(img.shape[0]), int(img.shape[1])
    _sides(H, W, 'img')
    img = img.contiguous()
    out = torch.empty((H + 1) // 2, (W + 1) // 2, 3, dtype=torch.float32, device=img.device)
    if img.dtype == torch.uint8:
        level0 = torch.empty(H, W, 3, dtype=torch.float32, device=img.device)
        _lib.call('lasr_varflow_reduce', img, None, level0, out, H, W)
        return level0, out
    _lib.call('lasr_varflow_reduce', None, img, None, out, H, W)
    return out


def pyramid(img):
    """uint8 [H,W,3] -> the list of fp32 levels [h,w,3], finest first."""
    if not torch.is_tensor(img):
        raise TypeError('varflow: img must be a tensor')
    _lib.need_cuda(img)
    if img.dtype != torch.uint8 or img.ndimension() != 3 or img.shape[2] != 3:
        raise ValueError('varflow: img must be uint8 [H, W, 3], got %s %s' % (img.dtype, tuple(img.shape)))
    H, W = int(img.shape[0]), int(img.shape[1])
    _sides(H, W, 'img')
    shapes = level_shapes(H, W)
    if len(shapes) == 1:
        level0 = torch.empty(H, W, 3, dtype=torch.float32, device=img.device)
        _lib.call('lasr_varflow_reduce', img.contiguous(), None, level0, None, H, W)
        return [level0]
    levels = list(reduce(img))
    for _ in shapes[2:]:
        levels.append(reduce(levels[-1]))
    return levels


def expand(uv, h, w):
    """[2,hc,wc] -> [2,h,w] with hc = ceil(h/2), wc = ceil(w/2): twice the bilinear sample at (y/2, x/2)."""
    uv = _planar(uv, 'uv', sides=False)
    h, w = int(h), int(w)
    _sides(h, w, 'the finer level')
    if (int(uv.shape[1]), int(uv.shape[2])) != ((h + 1) // 2, (w + 1) // 2):
        raise ValueError('varflow: a %d x %d level expands to %d x %d only from %d x %d' % (h, w, h, w, (h + 1) // 2, (w + 1) // 2))
    out = torch.empty(2, h, w, dtype=torch.float32, device=uv.device)
    _lib.call('lasr_varflow_expand', uv, out, int(uv.shape[1]), int(uv.shape[2]), h, w)
    return out


def tensor(I1, I2, uv):
    """I1, I2 fp32 [H,W,3], uv [2,H,W] -> J [6,H,W] = (J11, J12, J22, J13, J23, J33), zero where p + uv(p) leaves the frame."""
    uv = _planar(uv, 'uv')
    H, W = int(uv.shape[1]), int(uv.shape[2])
    I1, I2 = _f32(I1, (H, W, 3), 'I1'), _f32(I2, (H, W, 3), 'I2')
    J = torch.empty(6, H, W, dtype=torch.float32, device=uv.device)
    _lib.call('lasr_varflow_tensor', I1, I2, uv, J, H, W)
    return J


def weights(J, uv, d, eps=1e-3):
    """-> psi [2,H,W] = (psi_d, psi_s) of the increment d [2,H,W] around uv."""
    uv = _planar(uv, 'uv')
    H, W = int(uv.shape[1]), int(uv.shape[2])
    J, d = _f32(J, (6, H, W), 'J'), _f32(d, (2, H, W), 'd')
    psi = torch.empty(2, H, W, dtype=torch.float32, device=uv.device)
    _lib.call('lasr_varflow_weights', J, uv, d, psi, H, W, float(eps))
    return psi


def sor(J, psi, uv, d, alpha=0.03, omega=1.8, iters=10, scratch=None):
    """`iters` red-black SOR iterations on d [2,H,W], IN PLACE (d must be a contiguous fp32 tensor); -> d.  scratch [2,H,W] is the
    second buffer of the ping-pong (allocated when None)."""
    uv = _planar(uv, 'uv')
    H, W = int(uv.shape[1]), int(uv.shape[2])
    J, psi = _f32(J, (6, H, W), 'J'), _f32(psi, (2, H, W), 'psi')
    for t, name in ((d, 'd'), (scratch, 'scratch')):
        if t is None and name == 'scratch':
            continue
        if not torch.is_tensor(t):
            raise TypeError('varflow: %s must be a tensor' % name)
        _lib.need_cuda(t)
        if t.dtype != torch.float32 or tuple(t.shape) != (2, H, W) or not t.is_contiguous():
            raise ValueError('varflow: %s must be a contiguous float32 [2, %d, %d] tensor' % (name, H, W))
    if scratch is None:
        scratch = torch.empty_like(d)
    if int(iters) < 0:
        raise ValueError('varflow: iters must be >= 0, got %s' % iters)
    _lib.call('lasr_varflow_sor', J, psi, uv, d, scratch, H, W, float(alpha), float(omega), int(iters))
    return d


def occlusion(f_ab, f_ba, tau=OCC_TAU, s=OCC_S):
    """f_ab, f_ba [H,W,2] -> occ [H,W]: clamp((|f_ab(p) + f_ba(p + f_ab(p))| - tau) / s, -6, 6), +6 where p + f_ab(p) leaves the
    frame, never exactly 0 (the loader reads 0 as padding)."""
    if not torch.is_tensor(f_ab):
        raise TypeError('varflow: f_ab must be a tensor')
    _lib.need_cuda(f_ab)
    if f_ab.ndimension() != 3 or f_ab.shape[2] != 2:
        raise ValueError('varflow: f_ab must be [H, W, 2], got %s' % (tuple(f_ab.shape),))
    H, W = int(f_ab.shape[0]), int(f_ab.shape[1])
    _sides(H, W, 'f_ab')
    f_ab, f_ba = _f32(f_ab, (H, W, 2), 'f_ab'), _f32(f_ba, (H, W, 2), 'f_ba')
    occ = torch.empty(H, W, dtype=torch.float32, device=f_ab.device)
    _lib.call('lasr_varflow_occ', f_ab, f_ba, occ, H, W, float(tau), float(s))
    return occ


def flow_planar(imgA, imgB, init=None, **over):
    """uint8 [H,W,3] x 2 -> uv [2,H,W]: the whole estimate A -> B.  Launches only: no host synchronisation.  init(level, uv) -> uv,
    when given, sees the flow a level starts from: after expand, and the zero field of the coarsest level (preprocess/flow_match.py)."""
    p = params(**over)
    if not (torch.is_tensor(imgA) and torch.is_tensor(imgB)):
        raise TypeError('varflow: imgA and imgB must be tensors')
    _lib.need_cuda(imgA, imgB)
    if tuple(imgA.shape) != tuple(imgB.shape):
        raise ValueError('varflow: the two frames differ in size: %s and %s' % (tuple(imgA.shape), tuple(imgB.shape)))
    A, B = pyramid(imgA), pyramid(imgB)
    uv = None
    for lev in range(len(A) - 1, -1, -1):
        I1, I2 = A[lev], B[lev]
        h, w = int(I1.shape[0]), int(I1.shape[1])
        uv = torch.zeros(2, h, w, dtype=torch.float32, device=I1.device) if uv is None else expand(uv, h, w)
        if init is not None:
            uv = init(lev, uv)
        d, scratch = torch.empty_like(uv), torch.empty_like(uv)
        for _ in range(int(p['NW'])):
            J = tensor(I1, I2, uv)
            d.zero_()
            for _ in range(int(p['NO'])):
                psi = weights(J, uv, d, p['eps'])
                sor(J, psi, uv, d, p['alpha'], p['omega'], p['NI'], scratch)
            uv = uv + d
    return uv


def flow(imgA, imgB, init=None, **over):
    """uint8 [H,W,3] x 2 on the device -> flow A -> B, fp32 [H,W,2] in pixels."""
    return flow_planar(imgA, imgB, init, **over).permute(1, 2, 0).contiguous()


def flow_pair(imgA, imgB, **over):
    """-> (f_ab, occ_ab, f_ba, occ_ba): both directions and their consistency maps."""
    f_ab, f_ba = flow(imgA, imgB, **over), flow(imgB, imgA, **over)
    return f_ab, occlusion(f_ab, f_ba), f_ba, occlusion(f_ba, f_ab)


def make_flow_fn(device='cuda', pair=None, **over):
    """-> flow_fn(imgA, imgB) as auto_gen.run and maskprop.propagate take it: numpy uint8 [H,W,3] (or [H,W]) in, (flow [H,W,3]
    float32 with a ones channel, occ [H,W] float32) out, both numpy.  The first call of a pair computes both directions (the
    consistency map needs them); the reverse call is served from a cache of that one pair.  flow_fn.stats counts pairs computed
    and calls served from the cache.  pair(imgA, imgB, **over) stands in for flow_pair (preprocess/robust_flow.py passes its own)."""
    params(**over)
    cache = {}
    stats = dict(computed=0, cached=0)

    def key(a, b):
        return (a.shape, a.tobytes(), b.tobytes())

    def with_ones(f):
        return np.concatenate([f, np.ones(f.shape[:2] + (1,), np.float32)], -1)

    def flow_fn(imgA, imgB):
        # own, writable copies (PIL hands out read-only views, which torch.from_numpy warns about)
        a, b = (np.array(np.tile(x[:, :, None], (1, 1, 3)) if x.ndim == 2 else x, order='C', copy=True)
                for x in (np.asarray(imgA), np.asarray(imgB)))
        if a.dtype != np.uint8 or b.dtype != np.uint8 or a.shape != b.shape or a.ndim != 3 or a.shape[2] != 3:
            raise ValueError('varflow: flow_fn takes two uint8 [H, W, 3] frames of one size')
        k = key(a, b)
        if k in cache:
            stats['cached'] += 1
            return cache.pop(k)
        dev = torch.device(device)
        out = (pair or flow_pair)(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev), **over)
        f_ab, occ_ab, f_ba, occ_ba = (t.cpu().numpy() for t in out)
        stats['computed'] += 1
        cache.clear()
        cache[key(b, a)] = (with_ones(f_ba), occ_ba)
        return with_ones(f_ab), occ_ab
    flow_fn.stats = stats
    return flow_fn
