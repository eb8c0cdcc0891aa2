"""The definition of the SSIM texture term (include/lasr_ops.h), restated in numpy.  It runs in float64
and in float32 with the operations in the stated order; lasr_amd/csrc/ssim.hip follows the float32 form.  The reference has no
counterpart: this file is the definition, and the tests compare the kernels and the torch composition with it.

a [M,3,H,W] observed images (no gradient), b [N,3,H,W] renders, N = M rep; image i of b is compared with image i // rep of a.
Window: Wang et al. 2004, 11 taps of a Gaussian of sigma 1.5, valid region only (Ho = H - 10, Wo = W - 10)."""
import numpy as np

K, HALO = 11, 10
TILE_W, TILE_H = 32, 16                 # the tile of the block sums (LASR_SSIM_TILE_W / _H)
MIN_SIZE, MAX_SIZE = 11, 4096


def window(dtype=np.float64):
    """g[k] = exp(-(k - 5)^2 / (2 1.5^2)), normalised to sum 1 in float64, then rounded once to the working precision."""
    k = np.arange(K, dtype=np.float64)
    g = np.exp(-(k - 5.) ** 2 / (2. * 1.5 ** 2))
    return (g / g.sum()).astype(dtype)


def constants(L, dtype=np.float64):
    t = np.dtype(dtype).type
    c1, c2 = t(0.01) * t(L), t(0.03) * t(L)
    return c1 * c1, c2 * c2


def _check(a, b, rep):
    if a.ndim != 4 or b.ndim != 4 or a.shape[1] != 3 or b.shape[1] != 3 or a.shape[2:] != b.shape[2:]:
        raise ValueError('a [M,3,H,W] and b [N,3,H,W]')
    if rep < 1 or a.shape[0] * rep != b.shape[0] or a.shape[0] < 1:
        raise ValueError('N = M rep')
    H, W = a.shape[2:]
    if not (MIN_SIZE <= H <= MAX_SIZE and MIN_SIZE <= W <= MAX_SIZE):
        raise ValueError('sides %d x %d outside %d .. %d' % (H, W, MIN_SIZE, MAX_SIZE))


def blur(p, g, taps=None):
    """Horizontally, then vertically; each pass: acc = 0; for k ascending: acc = acc + g[k] p[. + k]."""
    taps = g if taps is None else taps
    Wo = p.shape[-1] - HALO
    acc = np.zeros(p.shape[:-1] + (Wo,), p.dtype)
    for k in range(K):
        acc = acc + taps[k] * p[..., k:k + Wo]
    Ho = p.shape[-2] - HALO
    out = np.zeros(acc.shape[:-2] + (Ho, Wo), p.dtype)
    for k in range(K):
        out = out + taps[k] * acc[..., k:k + Ho, :]
    return out


def ssim_map(a, b, rep=1, L=1., dtype=np.float64, planes=False):
    """s [N,3,Ho,Wo]; planes: also its derivatives by mu_b (the mu terms of the variances folded in), E[bb] and E[ab]."""
    _check(a, b, rep)
    t = np.dtype(dtype).type
    g = window(dtype)
    a = np.repeat(np.asarray(a, dtype), rep, 0)
    b = np.asarray(b, dtype)
    C1, C2 = constants(L, dtype)
    mua, mub, eaa, ebb, eab = blur(a, g), blur(b, g), blur(a * a, g), blur(b * b, g), blur(a * b, g)
    saa, sbb, sab = eaa - mua * mua, ebb - mub * mub, eab - mua * mub
    A1, A2 = t(2) * mua * mub + C1, t(2) * sab + C2
    B1, B2 = (mua * mua + mub * mub) + C1, (saa + sbb) + C2
    den = B1 * B2
    s = (A1 * A2) / den
    if not planes:
        return s
    u = (t(2) * mub) * s
    p1 = ((t(2) * mua) * (A2 - A1)) / den - (u / B1 - u / B2)
    p2 = -(s / B2)
    p3 = (t(2) * A1) / den
    return s, p1, p2, p3


def block_sums(s):
    """The sum of s per TILE_W x TILE_H tile of each (image, channel) in the working precision, in the order the kernel's block
    uses: thread t of 256 adds s at row t // 32 and at row t // 32 + 8 of column t % 32 (0 outside the map); the 64 lanes of a wave
    fold as lane l += lane l + o for o = 32, 16, ..., 1; the four waves as ((w0 + w1) + w2) + w3.  -> [N,3,tile rows,tile columns]"""
    N, C, Ho, Wo = s.shape
    nty, ntx = -(-Ho // TILE_H), -(-Wo // TILE_W)
    pad = np.zeros((N, C, nty * TILE_H, ntx * TILE_W), s.dtype)
    pad[:, :, :Ho, :Wo] = s
    tiles = pad.reshape(N, C, nty, TILE_H, ntx, TILE_W).transpose(0, 1, 2, 4, 3, 5)
    zero = np.zeros((), s.dtype)
    per_thread = (zero + tiles[..., :8, :]) + tiles[..., 8:, :]                     # [.., 8, 32]: thread t = row * 32 + column
    v = per_thread.reshape(N, C, nty, ntx, 4, 64).copy()
    for o in (32, 16, 8, 4, 2, 1):
        v[..., :o] = v[..., :o] + v[..., o:2 * o]
    w = v[..., 0]
    return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]


def distance(a, b, rep=1, L=1., dtype=np.float64):
    """d [N] = 1 - sum(s) / (3 Ho Wo): block sums in the working precision, folded per image in float64 in the order channel,
    tile row, tile column (one addition after the other), the result rounded to the working precision."""
    s = ssim_map(a, b, rep, L, dtype)
    part = block_sums(s).astype(np.float64).reshape(s.shape[0], -1)
    total = np.cumsum(part, axis=1)[:, -1]                                            # cumsum adds in index order
    return (1. - total / (3. * s.shape[2] * s.shape[3])).astype(dtype)


def grad_b(a, b, grad_d, rep=1, L=1., dtype=np.float64):
    """The hand-derived gradient of sum_i grad_d[i] d[i] by b: the three derivative planes, padded with zeros, go through the
    transposed window (horizontally, then vertically, taps g[10 - k] for k ascending) and are combined with a(q) and b(q):
    grad_b(q) = -(g_d / P) sum_p w(p, q) [P1(p) + 2 b(q) P2(p) + a(q) P3(p)], P = 3 Ho Wo."""
    t = np.dtype(dtype).type
    _, p1, p2, p3 = ssim_map(a, b, rep, L, dtype, planes=True)
    g = window(dtype)
    N, _, Ho, Wo = p1.shape
    T = []
    for p in (p1, p2, p3):
        pad = np.zeros((N, 3, Ho + 2 * HALO, Wo + 2 * HALO), dtype)
        pad[:, :, HALO:HALO + Ho, HALO:HALO + Wo] = p
        T.append(blur(pad, g, taps=g[::-1]))
    a = np.repeat(np.asarray(a, dtype), rep, 0)
    b = np.asarray(b, dtype)
    v = T[0] + (t(2) * b) * T[1]
    v = v + a * T[2]
    coef = (-np.asarray(grad_d, np.float64) / (3. * Ho * Wo)).astype(dtype)
    return coef[:, None, None, None] * v


def distance_torch64(a, b, rep=1, L=1.):
    """The forward in torch float64 (autograd gives the gradient the hand-derived one is checked against): the same expressions,
    the sums in torch's own order."""
    import torch
    g = torch.from_numpy(window(np.float64))
    a = a.double().repeat_interleave(rep, 0)
    b = b.double()

    def tblur(p):
        Wo, Ho = p.shape[-1] - HALO, p.shape[-2] - HALO
        acc = sum(g[k] * p[..., k:k + Wo] for k in range(K))
        return sum(g[k] * acc[..., k:k + Ho, :] for k in range(K))
    C1, C2 = constants(L)
    mua, mub = tblur(a), tblur(b)
    saa, sbb, sab = tblur(a * a) - mua * mua, tblur(b * b) - mub * mub, tblur(a * b) - mua * mub
    s = ((2 * mua * mub + C1) * (2 * sab + C2)) / ((mua * mua + mub * mub + C1) * (saa + sbb + C2))
    return 1. - s.sum((1, 2, 3)) / (3. * s.shape[2] * s.shape[3])


def pyramid(x, scales):
    """x, avg_pool2d(x, 2), ...: scale j is torch's F.avg_pool2d(., 2) applied j times (numpy in, numpy out, same dtype).  A scale
    whose smaller side falls below 11 is refused."""
    import torch
    import torch.nn.functional as F
    out, cur = [], torch.tensor(np.asarray(x))
    for j in range(scales):
        if min(cur.shape[-2:]) < MIN_SIZE:
            raise ValueError('scale %d is %d x %d: below the %d x %d window' % (j, cur.shape[-2], cur.shape[-1], K, K))
        out.append(cur.numpy())
        if j + 1 < scales:
            cur = F.avg_pool2d(cur, 2)
    return out


def multiscale_distance(a, b, rep=1, L=1., scales=3, dtype=np.float64):
    """D = mean over the scales of d_j (a plain mean over an average-pooled pyramid, not MS-SSIM's weighted product)."""
    pa, pb = pyramid(np.asarray(a, dtype), scales), pyramid(np.asarray(b, dtype), scales)
    t = np.dtype(dtype).type
    total = None
    for xa, xb in zip(pa, pb):
        d = distance(xa, xb, rep, L, dtype)
        total = d if total is None else total + d
    return total / t(scales)


# ---- fixtures of tests/test_ssim_gpu.py (and of the conditioning test of tests/test_ssim_cpu.py) ------------------------------
def texture_pair(M, rep, H, W, seed, unit_range=True):
    """Seeded band-limited textures masked by an ellipse onto black and onto white (the two forms of obspair), the observed side
    quantised to 1/255, the render side a perturbed float copy.  -> a [M,3,H,W], b [M rep,3,H,W] float32; unit_range False: both
    mapped to [-1, 1]."""
    rng = np.random.RandomState(seed)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    a = np.zeros((M, 3, H, W))
    for m in range(M):
        for c in range(3):
            img = np.full((H, W), 0.5)
            for _ in range(6):
                fy, fx = rng.uniform(-0.35, 0.35, 2)
                img += rng.uniform(0.03, 0.12) * np.cos(2 * np.pi * (fy * yy + fx * xx) + rng.uniform(0, 2 * np.pi))
            a[m, c] = np.clip(img, 0., 1.)
        cy, cx = H * rng.uniform(0.4, 0.6), W * rng.uniform(0.4, 0.6)
        inside = ((yy - cy) / (0.42 * H)) ** 2 + ((xx - cx) / (0.38 * W)) ** 2 <= 1.
        a[m] = np.where(inside, a[m], 0. if m % 2 == 0 else 1.)                     # on black | on white
    a = np.round(a * 255.) / 255.
    b = np.repeat(a, rep, 0)
    b = b + 0.08 * rng.standard_normal(b.shape) * rng.uniform(0.3, 1., (M * rep, 1, 1, 1))
    b = np.clip(b + rng.uniform(-0.05, 0.05, (M * rep, 3, 1, 1)), 0., 1.)
    if not unit_range:
        a, b = 2. * a - 1., 2. * b - 1.
    return a.astype(np.float32), b.astype(np.float32)
