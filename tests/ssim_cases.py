"""The fixtures tests/test_ssim_gpu.py runs the SSIM kernels on, and their references from the restatement alone
(tests/ssim_restated.py): computed once per case and shared; tests/test_ssim_cpu.py checks their conditioning without a GPU."""
import functools

import numpy as np

import ssim_restated as sr


def shapes(tile_w, tile_h):
    """One output pixel, one row / column more, odd sizes, more than one block each way, and outputs one pixel short of, equal to
    and one pixel past the kernel's tile each way."""
    fixed = [(11, 11), (12, 11), (11, 40), (26, 27), (27, 26), (43, 33), (64, 80)]
    tile = [(tile_h + dy + sr.HALO, tile_w + dx + sr.HALO) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dy == dx or dy == -dx]
    return fixed + [s for s in tile if s not in fixed]


def cases(tile_w, tile_h):
    """(M, rep, H, W, L): every shape with every M in {1, 2}, rep in {1, 3} and L in {1, 2}."""
    return [(M, rep, H, W, L) for (H, W) in shapes(tile_w, tile_h) for M in (1, 2) for rep in (1, 3) for L in (1., 2.)]


@functools.lru_cache(maxsize=None)
def reference(case):
    """a, b, the upstream gradient gd (float32) and the restatement's distance and gradient in float64 (d64, g64) and float32
    (d32, g32).  Read-only: the arrays are shared between the tests."""
    M, rep, H, W, L = case
    a, b = sr.texture_pair(M, rep, H, W, seed=1000 * H + 10 * W + 2 * M + rep, unit_range=L == 1.)
    gd = np.random.RandomState(H * W + M).uniform(0.25, 1., M * rep).astype(np.float32) * \
        np.where(np.arange(M * rep) % 2 == 0, 1., -1.).astype(np.float32)
    out = dict(a=a, b=b, gd=gd,
               d64=sr.distance(a, b, rep, L, np.float64), d32=sr.distance(a, b, rep, L, np.float32),
               g64=sr.grad_b(a, b, gd, rep, L, np.float64), g32=sr.grad_b(a, b, gd, rep, L, np.float32))
    for v in out.values():
        v.setflags(write=False)
    return out


def bounds(ref):
    """The bars of the comparison with the float64 restatement: 4 x max |float32 restatement - float64 restatement|, at least one
    float32 ulp of the largest magnitude; computed from the restatement alone."""
    eps = float(np.finfo(np.float32).eps)
    bv = max(4. * np.abs(ref['d32'].astype(np.float64) - ref['d64']).max(), eps * np.abs(ref['d64']).max())
    bg = max(4. * np.abs(ref['g32'].astype(np.float64) - ref['g64']).max(), eps * np.abs(ref['g64']).max())
    return float(bv), float(bg)
