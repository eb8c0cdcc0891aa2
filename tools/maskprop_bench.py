#!/usr/bin/env python3
"""What does one step of the silhouette propagation cost?  (lasr_amd/nnutils/maskprop.py, csrc/maskprop.hip)

    python tools/maskprop_bench.py [--sizes 1080x1920,480x854] [--iters 20] [--runs 3] [--json out.json]

One step s -> t on a seeded synthetic pair (a textured ellipse that moves over a textured background, default parameters: R 4,
K 5) is timed three ways, warm-up excluded, each as the median over --iters steps with device events, and the whole measurement
--runs times, the variants alternating inside a run:
  kernels   lasr_maskprop_hist + lasr_maskprop_unary + K x lasr_maskprop_meanfield, window given (no host work in the window)
  step      maskprop.step + the read-back of q and the host component filter (scipy.ndimage.label): what a frame costs
  torch     the same mathematics composed from torch operators on the same GPU: bincount (histograms), grid_sample (warp and
            flow consistency), unfold (the 80 taps; the bilateral weights are computed once per step and kept, which favours it)
and the per-kernel split of `kernels` (events around each launch group).  The torch composition's q is compared with the
kernels' before anything is timed.  No test asserts a time.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lasr_amd.nnutils import maskprop   # noqa: E402


def make_pair(H, W, dev, seed=0):
    """Two frames of a textured ellipse moving by (0.012 W, 0.004 H) over a textured background, the mask of the first, and the
    closed-form flows both ways."""
    g = torch.Generator(device='cpu').manual_seed(seed)

    def texture(base):
        low = torch.randn(1, 3, max(H // 24, 2), max(W // 24, 2), generator=g)
        t = F.interpolate(low, size=(H, W), mode='bicubic', align_corners=False)[0].permute(1, 2, 0)
        return t * 12 + torch.tensor(base)
    bg, obj = texture([60., 120., 170.]), texture([200., 80., 60.])
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing='ij')
    d = (round(0.012 * W), round(0.004 * H))
    frames, masks = [], []
    for t in range(2):
        m = ((xs - 0.45 * W - t * d[0]) / (0.16 * W)) ** 2 + ((ys - 0.5 * H - t * d[1]) / (0.3 * H)) ** 2 <= 1
        o = torch.roll(obj, shifts=(t * d[1], t * d[0]), dims=(0, 1))
        img = torch.where(m[..., None], o, bg) + torch.randint(-2, 3, (H, W, 3), generator=g)
        frames.append(img.round().clamp(0, 255).to(torch.uint8).to(dev))
        masks.append(m)
    dv = torch.tensor([float(d[0]), float(d[1])])
    flow_st = (masks[0][..., None] * dv).to(dev).contiguous()
    flow_ts = (masks[1][..., None] * -dv).to(dev).contiguous()
    return frames[0], frames[1], masks[0].float().to(dev), flow_ts, flow_st


def bins(img):
    i = img.long()
    return ((i[..., 0] >> 4) << 8) | ((i[..., 1] >> 4) << 4) | (i[..., 2] >> 4)


def torch_step(img_s, img_t, P_s, flow_ts, flow_st, key_hist, win, p):
    """maskprop.step from torch operators.  -> q fp32 [H,W]."""
    H, W = P_s.shape
    x0, y0, x1, y1 = win
    b, ps = bins(img_s)[y0:y1, x0:x1], P_s[y0:y1, x0:x1]
    hist = key_hist.long().clone()
    hist[1] += torch.bincount(b[ps >= p['hi']], minlength=4096)
    hist[0] += torch.bincount(b[ps <= p['lo']], minlength=4096)
    Nb, Nf = hist[0].sum().clamp(min=1).float(), hist[1].sum().clamp(min=1).float()
    app = torch.log((hist[1].float() / Nf + p['eps']) / (hist[0].float() / Nb + p['eps']))
    ys, xs = torch.meshgrid(torch.arange(H, device=P_s.device, dtype=torch.float32),
                            torch.arange(W, device=P_s.device, dtype=torch.float32), indexing='ij')
    qx, qy = xs + flow_ts[..., 0], ys + flow_ts[..., 1]
    inside = (qx >= 0) & (qx <= W - 1) & (qy >= 0) & (qy <= H - 1)
    grid = torch.stack([2 * qx / max(W - 1, 1) - 1, 2 * qy / max(H - 1, 1) - 1], -1)[None]
    src = torch.cat([P_s[None], flow_st.permute(2, 0, 1)], 0)[None]
    smp = F.grid_sample(src, grid, mode='bilinear', padding_mode='border', align_corners=True)[0]
    prior = torch.where(inside, smp[0], torch.zeros_like(smp[0]))
    ex, ey = flow_ts[..., 0] + smp[1], flow_ts[..., 1] + smp[2]
    conf = torch.where(inside, torch.exp(-(ex * ex + ey * ey) / (2 * p['tau'] ** 2)), torch.zeros_like(ex))
    pc = prior.clamp(1e-3, 1 - 1e-3)
    u = (p['w_p'] * conf * torch.log(pc / (1 - pc)) + p['w_a'] * app[bins(img_t)]).clamp(-p['U'], p['U'])
    q = torch.sigmoid(u)
    R = int(p['R'])
    n = 2 * R + 1
    I = img_t.float().permute(2, 0, 1)[None]
    taps = F.unfold(I, n, padding=R).view(3, n * n, H * W)
    valid = F.unfold(torch.ones(1, 1, H, W, device=I.device), n, padding=R)[0]
    d2 = ((taps - I.view(3, 1, H * W)) ** 2).sum(0)
    dy, dx = torch.meshgrid(torch.arange(-R, R + 1, device=I.device), torch.arange(-R, R + 1, device=I.device), indexing='ij')
    ds2 = (dx * dx + dy * dy).float().view(-1, 1)
    k = torch.exp(-d2 / (2 * p['sigma_i'] ** 2) - ds2 / (2 * p['sigma_s'] ** 2)) * valid
    k[n * n // 2] = 0
    del taps, d2
    for _ in range(int(p['K'])):
        s = F.unfold((2 * q - 1)[None, None], n, padding=R)[0]
        q = torch.sigmoid(u + p['w_s'] * (k * s).sum(0).view(H, W))
    return q


def timed(fn, iters):
    """Median / min / max milliseconds of fn over iters calls, each between two device events."""
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {'median_ms': statistics.median(ms), 'min_ms': min(ms), 'max_ms': max(ms)}


def host_timed(fn, iters):
    ms = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {'median_ms': statistics.median(ms), 'min_ms': min(ms), 'max_ms': max(ms)}


def bench_size(H, W, iters, runs, dev):
    p = maskprop.params()
    img_s, img_t, P_s, flow_ts, flow_st = make_pair(H, W, dev)
    win = maskprop.window_of(P_s)
    key_hist = maskprop.histogram(img_s, P_s, win)

    def kernels():
        hist = key_hist.clone()
        maskprop.histogram(img_s, P_s, win, hist, p['hi'], p['lo'])
        u, q = maskprop.unary(img_t, P_s, flow_ts, flow_st, hist, p['tau'], p['w_p'], p['w_a'], p['eps'], p['U'])
        return maskprop.meanfield(img_t, u, q, p['K'], p['R'], p['sigma_i'], p['sigma_s'], p['w_s'])

    def whole():
        q = maskprop.step(img_s, img_t, P_s, flow_ts, flow_st, key_hist, p)
        return maskprop.component_filter(q.cpu().numpy(), p['min_component'])

    def composed():
        return torch_step(img_s, img_t, P_s, flow_ts, flow_st, key_hist, win, p)

    q_native, q_torch = kernels(), composed()
    torch.cuda.synchronize()
    res = {'H': H, 'W': W, 'window': win, 'max_abs_diff_torch_vs_kernels': float((q_native - q_torch).abs().max()),
           'mask_area': int((q_native > 0.5).sum()), 'runs': []}
    hist = key_hist.clone()
    maskprop.histogram(img_s, P_s, win, hist)
    u, q0 = maskprop.unary(img_t, P_s, flow_ts, flow_st, hist)
    parts = {'hist': lambda: maskprop.histogram(img_s, P_s, win, hist),
             'unary': lambda: maskprop.unary(img_t, P_s, flow_ts, flow_st, hist),
             'meanfield_x%d' % p['K']: lambda: maskprop.meanfield(img_t, u, q0, p['K'])}
    for fn in (kernels, whole, composed):                                  # warm-up: every shape of the timed window
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for _ in range(runs):
        run = {'kernels': timed(kernels, iters), 'step': host_timed(whole, iters), 'torch': timed(composed, max(iters // 4, 3))}
        run.update({name: timed(fn, iters) for name, fn in parts.items()})
        res['runs'].append(run)
        print(json.dumps(dict(run, H=H, W=W)), flush=True)
    for name in res['runs'][0]:
        med = [r[name]['median_ms'] for r in res['runs']]
        res[name] = {'median_ms': statistics.median(med), 'min_of_medians_ms': min(med), 'max_of_medians_ms': max(med)}
    taps = ((2 * p['R'] + 1) ** 2 - 1) * p['K'] * H * W
    res['meanfield_gtaps_per_s'] = taps / (res['meanfield_x%d' % p['K']]['median_ms'] * 1e-3) / 1e9
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='1080x1920,480x854')
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--json', default='')
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        sys.exit('maskprop_bench.py: no HIP device: times are measured on the GPU or not at all')
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
