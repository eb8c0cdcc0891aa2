#!/usr/bin/env python3
"""A library built from another commit against the tree's, alternating run by run on one box, one process per run (LASR_HIP_LIB):
   python tools/prof/ab_alternate.py time <other.so> <alternations> [size ...]   rows as they come, then per size the means, the
                                                                                 same-library spreads and the project's rule
   python tools/prof/ab_alternate.py outputs <other.so>                           bench.py --dump-outputs of both at 256 and 16 frames, compared
sizes: f256 (the headline), f16, f64_512, f8_teams (the two-team pair walk), six16 / nine16 (six / nine channels, 16 meshes of 1280
faces, forward only through the operator).  The process that alternates never opens the GPU; a child that fails or runs into its time limit ends the
session.  profiles/r12_chunk_deal_ab.txt was taken with it."""
import collections
import json
import os
import subprocess
import sys
import tempfile

R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
BENCH = [sys.executable, os.path.join(R, 'bench.py'), '--full', '--no-cpu-baseline', '--no-lbs', '--no-sweep', '--no-step-profile', '--lasr-iters', '0']
SIZES = {
    'f256': BENCH + ['--frames', '256', '--steps', '80', '--warmup', '5'],
    'f16': BENCH + ['--frames', '16', '--steps', '600', '--warmup', '20'],
    'f64_512': BENCH + ['--frames', '64', '--image-size', '512', '--steps', '40', '--warmup', '5'],
    'f8_teams': BENCH + ['--frames', '8', '--steps', '1000', '--warmup', '20'],
    'six16': [sys.executable, os.path.abspath(__file__), 'nine', '300', '6'],
    'nine16': [sys.executable, os.path.abspath(__file__), 'nine', '300'],
}


def nine(reps, C=9):
    import numpy as np
    import torch
    sys.path.insert(0, R)
    import bench
    from lasr_amd import _lib, synth
    from lasr_amd.soft_renderer import functional as srf
    dev = torch.device('cuda:0')
    fv, ft, near, far = synth.raster_batch(8, 3, count=16)
    rng = np.random.default_rng(9)
    tex = np.concatenate([ft] + [rng.uniform(-2, 2, ft.shape).astype(np.float32) for _ in range(C // 3 - 1)], -1)
    kw = dict(synth.LASR_MODES, near=near, far=far, background_color=[0.1 * k for k in range(C)])
    tfv, tft = torch.from_numpy(fv).to(dev), torch.from_numpy(tex).to(dev)
    h = _lib.lib()
    stream = torch.cuda.current_stream(dev).cuda_stream
    for _ in range(10):
        srf.soft_rasterize(tfv, tft, 256, **kw)
    torch.cuda.synchronize()
    h.lasr_prof_enable(stream, 1)
    for _ in range(reps):
        srf.soft_rasterize(tfv, tft, 256, **kw)
    torch.cuda.synchronize()
    t = bench.collect_kernel_times(h, stream)
    h.lasr_prof_enable(stream, 0)
    print('RESULT ' + json.dumps({k: v[0] for k, v in t.items()}))


def child(cmd, lib, limit=200):
    env = dict(os.environ)
    if lib:
        env['LASR_HIP_LIB'] = os.path.abspath(lib)
    else:
        env.pop('LASR_HIP_LIB', None)
    try:
        p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        raise SystemExit('time limit: %s -- nothing more is started' % ' '.join(cmd[1:]))
    if p.returncode != 0:
        raise SystemExit('exit %d: %s -- nothing more is started\n%s' % (p.returncode, ' '.join(cmd[1:]), p.stderr[-3000:]))
    return p.stdout


def time_(other, alts, sizes):
    rows = collections.OrderedDict()
    for size in sizes:
        for i in range(1, alts + 1):
            for name, lib in (('parent', other), ('branch', None)):
                out = child(SIZES[size], lib)
                d = collections.OrderedDict()
                if size in ('six16', 'nine16'):
                    k = json.loads([l for l in out.splitlines() if l.startswith('RESULT ')][0][7:])
                else:
                    j = json.loads([l for l in out.splitlines() if l.startswith('{')][-1])
                    d['ms/step'] = j['ms_per_step']
                    k = j['roofline']['all_kernels_avg_ms']
                for n in sorted(k):
                    d[n.replace('sr_', '').replace('_kernel', '')] = k[n]
                rows.setdefault(size, []).append((name, i, d))
                print('%-9s %s_%d  %s' % (size, name, i, ' '.join('%s %.4f' % kv for kv in d.items())), flush=True)
    for size, rs in rows.items():
        print('\n---- %s (%s)' % (size, ' '.join(SIZES[size][2:])))
        print('%-38s %9s %9s %9s %9s %9s  %s' % ('column', 'parent', 'branch', 'diff', 'spread_p', 'spread_b',
                                                'lower in every alternation?  |diff| / largest same-library spread'))
        for c in rs[0][2]:
            p = [d[c] for n, i, d in rs if n == 'parent']
            b = [d[c] for n, i, d in rs if n == 'branch']
            mp, mb = sum(p) / len(p), sum(b) / len(b)
            sp, sb = max(p) - min(p), max(b) - min(b)
            print('%-38s %9.4f %9.4f %+9.4f %9.4f %9.4f  %-3s  %.1f' % (c, mp, mb, mb - mp, sp, sb, 'yes' if all(y < x for x, y in zip(p, b)) else 'no',
                                                                     abs(mb - mp) / max(sp, sb, 1e-9)))


def outputs(other):
    import numpy as np
    with tempfile.TemporaryDirectory() as tmp:
        for frames in (256, 16):
            for name, lib in (('parent', other), ('branch', None)):
                child([sys.executable, os.path.join(R, 'bench.py'), '--frames', str(frames), '--steps', '3', '--warmup', '1',
                       '--dump-outputs', os.path.join(tmp, '%s_%d' % (name, frames))], lib)
            for arr in ('soft_colors', 'grad_faces', 'grad_textures', 'mesh_grad'):
                a = np.load(os.path.join(tmp, 'parent_%d' % frames, arr + '.npy'))
                b = np.load(os.path.join(tmp, 'branch_%d' % frames, arr + '.npy'))
                dmax, amax = float(np.abs(a.astype(np.float64) - b).max()), float(np.abs(a).max())
                print('frames %3d %-14s %-20s max |parent - branch| %.3e   max |parent| %.3e   ratio %.3e   bit-identical %s   finite %s'
                      % (frames, arr, a.shape, dmax, amax, dmax / amax, np.array_equal(a, b), bool(np.isfinite(b).all())), flush=True)


if __name__ == '__main__':
    if sys.argv[1] == 'nine':
        nine(int(sys.argv[2]), int(sys.argv[3]) if len(sys.argv) > 3 else 9)
    elif sys.argv[1] == 'outputs':
        outputs(sys.argv[2])
    else:
        time_(sys.argv[2], int(sys.argv[3]), sys.argv[4:] or list(SIZES))
