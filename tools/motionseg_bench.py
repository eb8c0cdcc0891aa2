#!/usr/bin/env python3
"""What does one frame pair of the motion segmentation cost?  (lasr_amd/nnutils/motionseg.py, csrc/motionseg.hip)

    python tools/motionseg_bench.py [--sizes 480x854,1080x1920] [--iters 20] [--runs 3] [--json out.json]

One ordered pair on a seeded synthetic flow (a quadratic background motion, an ellipse that moves against it, smooth noise; default
parameters: quadratic model, 8 IRLS iterations) is timed, warm-up excluded, each figure the median over --iters repetitions
between device events, the whole measurement --runs times with the variants alternating inside a run:
  pair      lasr_motionseg_conf + 8 x (memset, lasr_motionseg_moments, lasr_motionseg_solve) + lasr_motionseg_evidence
  torch     the same sums written in plain torch on the same device: the 28 moments as float64 products and sums, the histogram
            by bincount, the 8 x 8 solve by torch.linalg in float64, no host synchronisation either; the only baseline there is
and the split of `pair` into conf, one moments launch, one solve launch and evidence.  theta of the two is compared before
anything is timed.  No test asserts a time.
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lasr_amd.nnutils import motionseg   # noqa: E402

THETA = (2.5, 0.8, -0.3, -1.0, 0.3, 0.6, 0.2, -0.15)
EXPONENTS = [(d - j, j) for d in range(5) for j in range(d + 1)]
B_U = [(0, 0), (1, 0), (0, 1), None, None, None, (2, 0), (1, 1)]
B_V = [None, None, None, (0, 0), (1, 0), (0, 1), (1, 1), (0, 2)]


def coords(H, W, dev):
    s = 0.5 * max(H, W)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64, device=dev), torch.arange(W, dtype=torch.float64, device=dev),
                            indexing='ij')
    return (xs - 0.5 * (W - 1)) / s, (ys - 0.5 * (H - 1)) / s


def model(theta, X, Y):
    return (theta[0] + theta[1] * X + theta[2] * Y + theta[6] * X * X + theta[7] * X * Y,
            theta[3] + theta[4] * X + theta[5] * Y + theta[6] * X * Y + theta[7] * Y * Y)


def make_pair(H, W, dev, seed=0):
    """-> (flow a -> b, flow b -> a) fp32 [H,W,2]: the background follows THETA (the flow back is its negative, consistent to
    the model's gradient), an ellipse moves 1 % of the width against it, smooth noise of 0.3 px on both."""
    g = torch.Generator(device='cpu').manual_seed(seed)
    X, Y = coords(H, W, dev)
    u, v = model(THETA, X, Y)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64, device=dev), torch.arange(W, dtype=torch.float64, device=dev),
                            indexing='ij')
    obj = ((xs - 0.45 * W) / (0.12 * W)) ** 2 + ((ys - 0.5 * H) / (0.25 * H)) ** 2 <= 1
    f = torch.stack([u, v], -1)
    f[obj] = f[obj] + torch.tensor([0.01 * W, 0.004 * H], dtype=torch.float64, device=dev)

    def noise():
        low = torch.randn(1, 2, max(H // 32, 2), max(W // 32, 2), generator=g)
        return 0.1 * F.interpolate(low, size=(H, W), mode='bicubic', align_corners=False)[0].permute(1, 2, 0).to(dev)
    return (f + noise()).float().contiguous(), (-f + noise()).float().contiguous()


def torch_fit(flow, conf, iters=8, k_sigma=3., sigma_min=0.25, ridge=1e-9):
    """motionseg.fit from torch operators (quadratic model; every pixel weighted, conf 0 included: the inputs are finite).
    -> (theta float64 [8], sigma) on the device."""
    H, W = conf.shape
    X, Y = coords(H, W, flow.device)
    mono = torch.stack([X ** i * Y ** j for i, j in EXPONENTS], 0).reshape(15, -1)
    u, v = flow[..., 0].reshape(-1), flow[..., 1].reshape(-1)
    c = conf.reshape(-1)
    slot = {e: k for k, e in enumerate(EXPONENTS)}
    # the assembly as gathers: A = sum over (B_U, B_V) of M[slot of the product], b likewise from the u and v moments
    iA, mA = torch.zeros(2, 8, 8, dtype=torch.long), torch.zeros(2, 8, 8, dtype=torch.float64)
    iB, mB = torch.zeros(2, 8, dtype=torch.long), torch.zeros(2, 8, dtype=torch.float64)
    for k, B in enumerate((B_U, B_V)):
        for i in range(8):
            if B[i] is None:
                continue
            iB[k, i], mB[k, i] = slot[B[i]], 1
            for j in range(8):
                if B[j] is not None:
                    iA[k, i, j], mA[k, i, j] = slot[(B[i][0] + B[j][0], B[i][1] + B[j][1])], 1
    iA, mA, iB, mB = (t.to(flow.device) for t in (iA, mA, iB, mB))
    theta = torch.zeros(8, dtype=torch.float64, device=flow.device)
    sigma = None
    Xf, Yf = X.float().reshape(-1), Y.float().reshape(-1)
    for _ in range(iters):
        th = theta.float()
        um, vm = model(th, Xf, Yf)
        r2 = (u - um) ** 2 + (v - vm) ** 2
        w = c if sigma is None else c / (1 + r2 / (sigma * sigma)) ** 2
        wd = w.double()
        M = mono @ wd
        Mu, Mv = mono[:6] @ (wd * u.double()), mono[:6] @ (wd * v.double())
        A = (M[iA] * mA).sum(0)
        b = Mu[iB[0]] * mB[0] + Mv[iB[1]] * mB[1]
        lam = ridge * torch.diagonal(A).sum() / 8
        L = torch.linalg.cholesky_ex(A + lam * torch.eye(8, dtype=torch.float64, device=flow.device))[0]
        theta = theta + torch.cholesky_solve((b - A @ theta)[:, None], L)[:, 0]
        sel = c >= 0.5
        bins = torch.clamp(torch.floor(16 * torch.sqrt(r2)), max=1023).long()
        hist = torch.bincount(bins[sel], minlength=1024)
        cum = torch.cumsum(hist, 0)
        med = (torch.searchsorted(cum, (cum[-1] + 1) // 2).double() + 0.5) / 16
        sigma = torch.clamp(k_sigma * med, min=sigma_min).float()
    return theta, sigma


def timed(fn, iters):
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {'median_ms': statistics.median(ms), 'min_ms': min(ms), 'max_ms': max(ms)}


def bench_size(H, W, iters, runs, dev):
    p = motionseg.params()
    f, fb = make_pair(H, W, dev)
    conf = motionseg.confidence(f, fb)
    state = motionseg.fit(f, conf)

    def pair():
        c = motionseg.confidence(f, fb, p['tau'])
        S = motionseg.fit(f, c, p['model'], p['iters'], p['k_sigma'], p['sigma_min'], p['ridge'])
        return motionseg.evidence(f, c, S, p['kappa'], p['U'])

    def composed():
        return torch_fit(f, conf, p['iters'], p['k_sigma'], p['sigma_min'], p['ridge'])

    theta_t, sigma_t = composed()
    torch.cuda.synchronize()
    res = {'H': H, 'W': W, 'theta': [float(v) for v in state[:8]], 'sigma': float(state[8]), 'status': int(state[11]),
           'max_abs_theta_diff_torch_vs_kernels': float((theta_t - state[:8]).abs().max()), 'sigma_torch': float(sigma_t), 'runs': []}
    partials, hist = motionseg.moments(f, conf, state)
    scratch = state.clone()
    parts = {'conf': lambda: motionseg.confidence(f, fb),
             'moments_x1': lambda: motionseg.moments(f, conf, state, partials, hist),
             'solve_x1': lambda: motionseg.solve(partials, hist, scratch, H, W),
             'evidence': lambda: motionseg.evidence(f, conf, state)}
    for fn in (pair, composed):
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for _ in range(runs):
        run = {'pair': timed(pair, iters), 'torch': timed(composed, max(iters // 4, 3))}
        run.update({name: timed(fn, iters) for name, fn in parts.items()})
        res['runs'].append(run)
        print(json.dumps(dict(run, H=H, W=W)), flush=True)
    for name in res['runs'][0]:
        med = [r[name]['median_ms'] for r in res['runs']]
        res[name] = {'median_ms': statistics.median(med), 'min_of_medians_ms': min(med), 'max_of_medians_ms': max(med)}
    res['moments_gb_per_s'] = 12. * H * W / (res['moments_x1']['median_ms'] * 1e-3) / 1e9      # flow 8 B + conf 4 B per pixel
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='480x854,1080x1920')
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--json', default='')
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        sys.exit('motionseg_bench.py: no HIP device: times are measured on the GPU or not at all')
    dev = torch.device('cuda:0')
    out = {'device': torch.cuda.get_device_name(0), 'iters': args.iters, 'sizes': []}
    for s in args.sizes.split(','):
        H, W = (int(v) for v in s.split('x'))
        out['sizes'].append(bench_size(H, W, args.iters, args.runs, dev))
        torch.cuda.empty_cache()
    print(json.dumps(out))
    if args.json:
        with open(args.json, 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
