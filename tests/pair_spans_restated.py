"""The forward pair walk's span classification and 64 x 64 bit transpose (lasr_amd/csrc/sr_forward_pairs.h: span_edge, span_row,
wave_transpose64), restated in numpy with the kernel's float32 operations, next to what they are held against: the per-pixel test
they replace (w_k < far[k] on the unfused float32 barycentrics) and a float64 point-triangle distance.

Everything works on PAIRS of (face, 16x16 tile): arrays with a leading axis P.  Masks are [P, 16, 16] booleans, [row of the tile
from the top, column]."""
import math

import numpy as np

from lasr_amd import synth

F32 = np.float32
TILE = 16
SLACK = F32(1. / 128.)                      # PW_SPAN_SLACK
GMAX = F32(2. ** 40)
BIG = F32(1e9)


def threshold():
    """The launch's squared distance threshold as the C ABI forms it from the float arguments (dist_thr * sigma)."""
    m = synth.LASR_MODES
    return F32(F32(math.log(1. / m['dist_eps'] - 1.)) * F32(m['sigma_val']))


def pix_center(i, IS):
    return (F32(2) * np.asarray(i, F32) + F32(1 - IS)) / F32(IS)        # exact integer numerator, one rounding: sr_device.h: pix_center


def fma(a, b, c):
    """float32 fused multiply-add: the product of two floats is exact in float64; the sum rounds once there and once to float32
    (a double rounding shows in about one result in 2^29: nothing here counts on the last bit)."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)


def _first_pixel_ge(lo, IS):
    c = pix_center(np.arange(IS), IS)
    return int(np.searchsorted(c, lo, 'left'))                           # smallest i with centre >= lo; IS = none


def _last_pixel_le(hi, IS):
    c = pix_center(np.arange(IS), IS)
    return int(np.searchsorted(c, hi, 'right')) - 1                      # largest i with centre <= hi; -1 = none


def records(fv, IS, thr):
    """What sr_device.h: build_record and the staging derive of faces fv [F, 3, 3] (float32 operations): inv [F, 9], far [F, 3],
    well [F] (flags bit 4), rect [F, 4] = first / last column, first / last row from the top (empty: 32767, -1, 32767, -1)."""
    fv = np.asarray(fv, F32)
    x0, y0, x1, y1, x2, y2 = fv[:, 0, 0], fv[:, 0, 1], fv[:, 1, 0], fv[:, 1, 1], fv[:, 2, 0], fv[:, 2, 1]
    adj = np.stack([y1 - y2, x2 - x1, x1 * y2 - x2 * y1, y2 - y0, x0 - x2, x2 * y0 - x0 * y2, y0 - y1, x1 - x0, x0 * y1 - x1 * y0], 1)
    det0 = x2 * (y0 - y1) + x0 * (y1 - y2) + x1 * (y2 - y0)
    det = np.where(det0 > 0, np.maximum(det0.astype(np.float64), 1e-10), np.minimum(det0.astype(np.float64), -1e-10)).astype(F32)
    inv = adj / det[:, None]
    px, py = fv[:, :, 0], fv[:, :, 1]
    hk2 = np.zeros((len(fv), 3), F32)
    well = np.ones(len(fv), bool)
    with np.errstate(divide='ignore', invalid='ignore'):
        for k in range(3):
            b, c = (k + 1) % 3, (k + 2) % 3
            ex, ey = px[:, c] - px[:, b], py[:, c] - py[:, b]
            l2 = ex * ex + ey * ey
            h2 = np.where(l2 > 0, det0 * det0 / l2, F32(0)).astype(F32)
            hk2[:, k] = h2
            well &= (h2 > F32(1e-4)) & (h2 < F32(1e4)) & (l2 < F32(16))
        far = np.where(well[:, None], -np.sqrt(F32(thr * F32(1.05)) / hk2), F32(-np.inf)).astype(F32)
    margin = np.sqrt(F32(thr))
    rect = np.zeros((len(fv), 4), np.int64)
    for i in range(len(fv)):
        c0, c1 = _first_pixel_ge(px[i].min() - margin, IS), _last_pixel_le(px[i].max() + margin, IS)
        yi0, yi1 = _first_pixel_ge(py[i].min() - margin, IS), _last_pixel_le(py[i].max() + margin, IS)
        r0, r1 = IS - 1 - yi1, IS - 1 - yi0
        rect[i] = (32767, -1, 32767, -1) if c0 > c1 or r0 > r1 else (c0, c1, r0, r1)
    return dict(inv=inv.astype(F32), far=far, well=well, rect=rect, fv=fv)


def tile_pairs(rec, IS):
    """(face, tx, ty) of every 16x16 tile a face's pixel rect overlaps: int arrays [P]."""
    out = []
    for i, (c0, c1, r0, r1) in enumerate(rec['rect']):
        if c0 > c1:
            continue
        for ty in range(r0 // TILE, r1 // TILE + 1):
            for tx in range(c0 // TILE, c1 // TILE + 1):
                out.append((i, tx, ty))
    return np.asarray(out, np.int64).reshape(-1, 3).T


def _rect_in_tile(rec, face, tx, ty):
    c0, c1, r0, r1 = rec['rect'][face].T
    a0 = np.minimum(np.maximum(c0 - tx * TILE, 0), TILE)
    a1 = np.maximum(np.minimum(c1 - tx * TILE, TILE - 1), -1)
    rows = np.arange(TILE)[None, :]
    row_in = (rows >= (r0 - ty * TILE)[:, None]) & (rows <= (r1 - ty * TILE)[:, None])
    return a0, a1, row_in


def rect_masks(rec, face, tx, ty):
    a0, a1, row_in = _rect_in_tile(rec, face, tx, ty)
    cols = np.arange(TILE)[None, None, :]
    return row_in[:, :, None] & (cols >= a0[:, None, None]) & (cols <= a1[:, None, None])


def span_masks(rec, face, tx, ty, IS, tame=None):
    """The kernel's spans: span_edge once per edge, span_row per row of the tile, rounded outward, cut with the rect."""
    P = len(face)
    inv, far = rec['inv'][face], rec['far'][face]
    span = rec['well'][face] & (np.ones(P, bool) if tame is None else tame[face])
    a0, a1, row_in = _rect_in_tile(rec, face, tx, ty)
    half_is = F32(0.5) * F32(IS)
    off = (F32(0.5) * F32(IS - 1) - (tx * TILE).astype(F32)).astype(F32)
    yrow = pix_center(IS - 1 - (ty[:, None] * TILE + np.arange(TILE)[None, :]), IS)          # [P, 16]
    lo = np.full((P, TILE), -BIG, F32)
    hi = np.full((P, TILE), BIG, F32)
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        for k in range(3):
            a, b, c = inv[:, 3 * k], inv[:, 3 * k + 1], inv[:, 3 * k + 2]
            g = np.clip((F32(1) / a) * half_is, -GMAX, GMAX).astype(F32)
            p = (-b * g).astype(F32)
            q = fma((far[:, k] - c).astype(F32), g, off)
            lower, upper = span & (g > 0), span & (g < 0)
            pl, ql = np.where(lower, p, F32(0)), np.where(lower, q - SLACK, -BIG).astype(F32)
            pu, qu = np.where(upper, p, F32(0)), np.where(upper, q + SLACK, BIG).astype(F32)
            lo = np.maximum(lo, fma(yrow, pl[:, None], ql[:, None]))
            hi = np.minimum(hi, fma(yrow, pu[:, None], qu[:, None]))
    a0f, a1f = a0.astype(F32)[:, None], a1.astype(F32)[:, None]
    lcol = np.clip(np.ceil(lo), a0f, F32(16))                  # v_med3_f32(ceil(lo), a0, 16): 0 <= a0 <= 16
    hcol = np.clip(np.floor(hi), F32(-1), a1f)                 # v_med3_f32(floor(hi), -1, a1): -1 <= a1 <= 15
    cols = np.arange(TILE, dtype=F32)[None, None, :]
    return row_in[:, :, None] & (cols >= lcol[:, :, None]) & (cols <= hcol[:, :, None])


def _bary32(rec, face, tx, ty, IS):
    inv = rec['inv'][face]
    xp = pix_center(tx[:, None] * TILE + np.arange(TILE)[None, :], IS)[:, None, :]                       # [P, 1, 16]
    yp = pix_center(IS - 1 - (ty[:, None] * TILE + np.arange(TILE)[None, :]), IS)[:, :, None]            # [P, 16, 1]
    e = lambda j: inv[:, j][:, None, None]                                                                 # noqa: E731
    with np.errstate(invalid='ignore', over='ignore'):
        return [((e(3 * k) * xp).astype(F32) + (e(3 * k + 1) * yp).astype(F32)).astype(F32) + e(3 * k + 2) for k in range(3)]


def pixel_test_masks(rec, face, tx, ty, IS):
    """The per-pixel classification the spans replace: in the rect, and inside the face or not far (unfused float32 barycentrics)."""
    w = _bary32(rec, face, tx, ty, IS)
    far = rec['far'][face]
    is_far = (w[0] < far[:, 0, None, None]) | (w[1] < far[:, 1, None, None]) | (w[2] < far[:, 2, None, None])
    return rect_masks(rec, face, tx, ty) & ~is_far


def exact_masks(rec, face, tx, ty, IS, thr):
    """float64: the pixel centre lies inside the face or closer to it than sqrt(thr) (squared distance to the three segments)."""
    t = rec['fv'][face].astype(np.float64)
    X = ((2. * (tx[:, None] * TILE + np.arange(TILE)[None, :]) + 1. - IS) / IS)[:, None, :]
    Y = ((2. * (IS - 1 - (ty[:, None] * TILE + np.arange(TILE)[None, :])) + 1. - IS) / IS)[:, :, None]
    best = np.full((len(face), TILE, TILE), np.inf)
    sign = []
    for i, j in ((0, 1), (1, 2), (2, 0)):
        px_, py_ = t[:, i, 0, None, None], t[:, i, 1, None, None]
        ex, ey = t[:, j, 0, None, None] - px_, t[:, j, 1, None, None] - py_
        s = np.clip(((X - px_) * ex + (Y - py_) * ey) / np.maximum(ex * ex + ey * ey, 1e-300), 0, 1)
        best = np.minimum(best, (px_ + s * ex - X) ** 2 + (py_ + s * ey - Y) ** 2)
        sign.append(ex * (Y - py_) - ey * (X - px_))
    inside = ((sign[0] > 0) & (sign[1] > 0) & (sign[2] > 0)) | ((sign[0] < 0) & (sign[1] < 0) & (sign[2] < 0))
    return inside | (best < float(thr))


# ---- the transpose: the kernel's six stages on 64 words of 64 bits (lane e holds words[e])

def _rot16(v):
    return ((v >> 16) | (v << 16)) & 0xffffffff


def transpose64(words):
    """out[p] bit e = words[e] bit p, stage by stage as wave_transpose64 moves the bits between lanes."""
    lo = [int(w) & 0xffffffff for w in words]
    hi = [int(w) >> 32 for w in words]
    # stage 5, v_permlane32_swap(lo, hi): lo of the lanes 32..63 <-> hi of the lanes 0..31
    for L in range(32):
        hi[L], lo[L + 32] = lo[L + 32], hi[L]
    # stage 4, v_permlane16_swap(x, rot16(x)): the odd rows of the first operand <-> the even rows of the second, then one merge
    for reg in (lo, hi):
        a, b = list(reg), [_rot16(v) for v in reg]
        for L in range(64):
            if (L >> 4) & 1 == 0:
                a[L + 16], b[L] = b[L], a[L + 16]
        for L in range(64):
            reg[L] = (a[L] & 0xffff) | ((b[L] << 16) & 0xffffffff)
    # stages 3..0: the partner's word from lane L ^ J (row_ror:8, ds_swizzle xor 4, quad_perm), own bits kept under `keep`
    for J, M in ((8, 0x00ff00ff), (4, 0x0f0f0f0f), (2, 0x33333333), (1, 0x55555555)):
        for reg in (lo, hi):
            t = [reg[L ^ J] for L in range(64)]
            for L in range(64):
                up = (L & J) != 0
                keep = (~M & 0xffffffff) if up else M
                moved = (t[L] >> J) if up else ((t[L] << J) & 0xffffffff)
                reg[L] = (reg[L] & keep) | (moved & ~keep & 0xffffffff)
    return [(hi[L] << 32) | lo[L] for L in range(64)]


def transpose64_numpy(words):
    bits = np.array([[(int(w) >> p) & 1 for p in range(64)] for w in words], np.uint8)        # [e, p]
    return [int(sum(int(b) << e for e, b in enumerate(col))) for col in bits.T]
