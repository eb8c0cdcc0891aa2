"""float64 numpy restatement of the reprojection scores (include/lasr_ops.h: lasr_reproj_pixels, lasr_reproj_boundary; DESIGN.md
4.15), written from the header text, with scipy.ndimage.binary_dilation and an explicit disk for the boundary matching.  The scores
are this project's own addition, so this file is what the kernels are checked against.  It takes the raster's face-index planes
as an input, as tests/tracks_restated.py does, so coverage is not a matter of rounding.  `dtype` lets the flow and colour groups run
in float32 as well: the spread between the two is what the GPU tolerances are derived from (tests/test_reproj_cpu.py)."""
import math
import os

import numpy as np
from scipy import ndimage

COUNTS = ('inter', 'union', 'n_pred', 'n_gt', 'n_pb', 'n_gb', 'pm', 'gm', 'n_flow', 'n_le1', 'n_le3', 'n_rgb')
MAX_RADIUS = 96
# The largest per-pixel difference between this restatement run in float32 and in float64 on flow_fixture() (hand-made planes):
# measured 1.494e-5 px in epe and 0.3091 in the squared colour difference (values up to 1.07e5, i.e. 1.6e-5 relative: the
# barycentrics' rounding times the colour contrast).  tests/test_reproj_cpu.py re-measures both; the GPU tolerances are 8 x these.
EPE_SPREAD = 1.5e-5
SQ_SPREAD = 0.31


# ---- silhouette -------------------------------------------------------------------------------------------------------------------------
def radius_of(bound_th, H, W):
    return int(bound_th) if bound_th >= 1 else int(math.ceil(bound_th * math.hypot(H, W)))


def boundary(seg):
    """b(seg): a pixel differs from its east, south or south-east neighbour (0 beyond the image); then the last row is seg ^ e, the
    last column seg ^ s, the last pixel 0."""
    seg = np.asarray(seg, bool)
    e, s, se = np.zeros_like(seg), np.zeros_like(seg), np.zeros_like(seg)
    e[:, :-1] = seg[:, 1:]
    s[:-1, :] = seg[1:, :]
    se[:-1, :-1] = seg[1:, 1:]
    b = (seg ^ e) | (seg ^ s) | (seg ^ se)
    b[-1, :] = seg[-1, :] ^ e[-1, :]
    b[:, -1] = seg[:, -1] ^ s[:, -1]
    b[-1, -1] = False
    return b


def disk(rho):
    y, x = np.mgrid[-rho:rho + 1, -rho:rho + 1]
    return x * x + y * y <= rho * rho


def dilate(m, rho):
    """Disk dilation, clipped to the image (scipy pads with False)."""
    return ndimage.binary_dilation(np.asarray(m, bool), structure=disk(rho)) if m.any() else np.zeros_like(m, bool)


def dilate_rows(m, rho):
    """The row-run form the kernel uses: for the row offset dy, every bit within |dx| <= floor(sqrt(rho^2 - dy^2))."""
    m = np.asarray(m, bool)
    H, W = m.shape
    out = np.zeros_like(m)
    for dy in range(-rho, rho + 1):
        hx = math.isqrt(rho * rho - dy * dy)
        src = np.zeros_like(m)
        if dy >= 0:
            src[:H - dy] = m[dy:] if dy < H else False
        else:
            src[-dy:] = m[:H + dy] if -dy < H else False
        run = np.zeros_like(m)
        for dx in range(-min(hx, W - 1), min(hx, W - 1) + 1):
            if dx >= 0:
                run[:, :W - dx] |= src[:, dx:]
            else:
                run[:, -dx:] |= src[:, :W + dx]
        out |= run
    return out


def silhouette_counts(pred, gt, rho):
    """-> dict of the counts 0-7."""
    pred, gt = np.asarray(pred, bool), np.asarray(gt, bool)
    bp, bg = boundary(pred), boundary(gt)
    return dict(inter=int((pred & gt).sum()), union=int((pred | gt).sum()), n_pred=int(pred.sum()), n_gt=int(gt.sum()),
                n_pb=int(bp.sum()), n_gb=int(bg.sum()), pm=int((bp & dilate(bg, rho)).sum()), gm=int((bg & dilate(bp, rho)).sum()))


def scores(c):
    """J, precision, recall, F of one frame's counts, in float64."""
    J = c['inter'] / c['union'] if c['union'] else 1.
    if c['n_pb'] == 0 and c['n_gb'] > 0:
        P, R = 1., 0.
    elif c['n_gb'] == 0 and c['n_pb'] > 0:
        P, R = 0., 1.
    elif c['n_pb'] == 0 and c['n_gb'] == 0:
        P = R = 1.
    else:
        P, R = c['pm'] / c['n_pb'], c['gm'] / c['n_gb']
    return dict(J=J, precision=P, recall=R, F=0. if P + R == 0 else 2 * P * R / (P + R))


def pack_bits(m):
    """bool [H,W] -> uint64 [H, ceil(W/64)]: column c is bit c & 63 of word c >> 6."""
    m = np.asarray(m, bool)
    H, W = m.shape
    WW = (W + 63) // 64
    padded = np.zeros((H, WW * 64), np.uint64)
    padded[:, :W] = m
    return (padded.reshape(H, WW, 64) << np.arange(64, dtype=np.uint64)).sum(-1, dtype=np.uint64)


def pair(H, W):
    """The mask pair of the parity tests: gt an ellipse, pred a shifted, differently shaped ellipse plus a 2 x 3 speck in the
    top-right corner that touches the last column.  -> (pred, gt) bool [H,W]."""
    r, c = np.mgrid[:H, :W].astype(np.float64)
    gt = ((r - 0.5 * H) / (0.3 * H)) ** 2 + ((c - 0.45 * W) / (0.3 * W)) ** 2 <= 1.
    pred = ((r - (0.5 * H + 1.5)) / (0.33 * H)) ** 2 + ((c - (0.45 * W + 2.2)) / (0.27 * W)) ** 2 <= 1.
    pred[:2, W - 3:] = True
    return pred, gt


# ---- flow and colour ----------------------------------------------------------------------------------------------------------------------
def anchors(verts_t, faces, K_t, plane, both, dtype=np.float64):
    """Step 3 of lasr_track_anchor at the centres of the pixels of `both` [H,W]: -> rows, cols, tri [M,3], c1, c2, ok [M]."""
    f = dtype
    r, c = np.nonzero(both)
    face = plane[r, c].astype(np.int64)
    tri = np.asarray(faces)[face]
    v = np.asarray(verts_t, f)
    V0, V1, V2 = v[tri[:, 0]], v[tri[:, 1]], v[tri[:, 2]]
    e1, e2 = V1 - V0, V2 - V0
    k = np.asarray(K_t, f)
    u, w = (c + 0.5).astype(f), (r + 0.5).astype(f)
    d = np.stack([(u - k[2]) / k[0], (w - k[3]) / k[1], np.ones_like(u)], 1).astype(f)
    p = np.cross(d, e2)
    det = (e1 * p).sum(1)
    s = V0[:, 2:3] * d - V0
    n = np.cross(e1, e2)
    with np.errstate(divide='ignore', invalid='ignore'):
        b1 = (s * p).sum(1) / det
        b2 = (d * np.cross(s, e1)).sum(1) / det
    ok = ((n * n).sum(1) > 0) & (det != 0) & np.isfinite(b1) & np.isfinite(b2)
    b1, b2 = np.where(ok, b1, 0), np.where(ok, b2, 0)
    a = np.clip(np.stack([1 - b1 - b2, b1, b2], 1), 0, 1).astype(f)
    a = a / a.sum(1, keepdims=True)
    return r, c, tri, a[:, 1], a[:, 2], ok


def flow_pred(verts_next, K_next, r, c, tri, c1, c2, dtype=np.float64):
    """-> (flow_pred [M,2] (u, v), front [M]): the anchored points on the successor's mesh, projected, minus the pixel centres."""
    f = dtype
    v = np.asarray(verts_next, f)
    V0 = v[tri[:, 0]]
    e1, e2 = v[tri[:, 1]] - V0, v[tri[:, 2]] - V0
    P = V0 + (c1[:, None] * e1 + c2[:, None] * e2)
    front = P[:, 2] > 0
    z = np.where(front, P[:, 2], 1).astype(f)
    k = np.asarray(K_next, f)
    u = k[0] * P[:, 0] / z + k[2] - (c + 0.5).astype(f)
    w = k[1] * P[:, 1] / z + k[3] - (r + 0.5).astype(f)
    return np.stack([u, w], 1), front


def evaluate(verts, faces, K, planes, masks, flows=None, occs=None, frames=None, colors=None, bound_th=0.008, dtype=np.float64):
    """The whole definition on face-index planes [T, >= H, >= W].  -> dict of per-frame arrays: the twelve counts, sum_epe, sum_sq,
    J, precision, recall, F, epe, pck1, pck3, psnr, radius, and per frame the lists 'epe_px' and 'sq_px' (the epe and the squared colour
    difference of every counted pixel) and 'flow_px' ((rows, cols, flow_pred))."""
    masks = np.asarray(masks)
    T, H, W = masks.shape
    faces = np.asarray(faces)
    F = faces.shape[0]
    rho = radius_of(bound_th, H, W)
    assert 0 <= rho <= MAX_RADIUS
    out = {k: np.zeros(T, np.int64) for k in COUNTS}
    out.update(sum_epe=np.zeros(T), sum_sq=np.zeros(T), radius=np.full(T, rho), epe_px=[], sq_px=[], flow_px=[])
    sc = {k: np.zeros(T) for k in ('J', 'precision', 'recall', 'F')}
    for t in range(T):
        plane = np.asarray(planes[t])[:H, :W]
        pred = (plane >= 0) & (plane < F)
        gt = masks[t] != 0
        c = silhouette_counts(pred, gt, rho)
        for k, v in c.items():
            out[k][t] = v
        for k, v in scores(c).items():
            sc[k][t] = v
        epe_px, sq_px, flow_px = np.zeros(0), np.zeros(0), (np.zeros(0, int), np.zeros(0, int), np.zeros((0, 2)))
        if flows is not None or frames is not None:
            r, cc, tri, c1, c2, ok = anchors(verts[t], faces, K[t], plane, pred & gt, dtype)
            r, cc, tri, c1, c2 = r[ok], cc[ok], tri[ok], c1[ok], c2[ok]
            if frames is not None:
                C = np.asarray(colors[t]).astype(dtype)
                d = ((1 - c1 - c2)[:, None] * C[tri[:, 0]] + c1[:, None] * C[tri[:, 1]] + c2[:, None] * C[tri[:, 2]]) - \
                    np.asarray(frames[t])[r, cc].astype(dtype)
                out['n_rgb'][t] = len(r)
                sq_px = (d * d).sum(1).astype(np.float64)
                out['sum_sq'][t] = float(sq_px.sum())
            if flows is not None and t < T - 1:
                fl = np.asarray(flows[t])[r, cc]
                valid = (fl[:, 2] != 0) & np.isfinite(fl[:, 0]) & np.isfinite(fl[:, 1])
                if occs is not None:
                    valid &= np.asarray(occs[t])[r, cc] < 10
                fp, front = flow_pred(verts[t + 1], K[t + 1], r, cc, tri, c1, c2, dtype)
                flow_px = (r[front], cc[front], fp[front])
                valid &= front
                dd = fp[valid] - fl[valid, :2].astype(dtype)
                epe_px = np.sqrt((dd * dd).sum(1)).astype(np.float64)
                out['n_flow'][t], out['n_le1'][t], out['n_le3'][t] = len(epe_px), (epe_px <= 1).sum(), (epe_px <= 3).sum()
                out['sum_epe'][t] = epe_px.sum()
        out['epe_px'].append(epe_px)
        out['sq_px'].append(sq_px)
        out['flow_px'].append(flow_px)
    out.update(sc)
    with np.errstate(divide='ignore', invalid='ignore'):
        nf, nr = out['n_flow'].astype(float), out['n_rgb'].astype(float)
        out['epe'] = np.where(nf > 0, out['sum_epe'] / nf, np.nan)
        out['pck1'] = np.where(nf > 0, out['n_le1'] / nf, np.nan)
        out['pck3'] = np.where(nf > 0, out['n_le3'] / nf, np.nan)
        out['psnr'] = np.where(nr > 0, 10 * np.log10(255. ** 2 * 3 * nr / out['sum_sq']), np.nan)
    return out


def flow_fixture(seed=3):
    """The flow / colour fixture on tracks_cases.sphere_case() (5 frames, 48 x 64) with the hand-made raster planes replaced by
    whatever `planes` the caller passes to observed_flow: see there."""
    import tracks_cases as tc
    verts, faces, K = tc.sphere_case()
    rng = np.random.default_rng(seed)
    colors = rng.integers(0, 256, (verts.shape[0], verts.shape[1], 3), dtype=np.uint8)
    frames = rng.integers(0, 256, (verts.shape[0], tc.H, tc.W, 3), dtype=np.uint8)
    return dict(verts=verts, faces=faces, K=K, colors=colors, frames=frames, H=tc.H, W=tc.W, seed=seed)


def observed_flow(fx, planes, seed=None):
    """The "observed" flow of the fixture: the restatement's own rendered flow (float64, on `planes`) plus a seeded smooth field
    that spreads epe over 0-5 px; a band of columns is invalid through channel 2, a band of rows through occ >= 10.  Uncovered
    pixels hold the smooth field alone.  -> masks [T,H,W] uint8 (everything annotated), flows [T-1,H,W,3] float32, occs."""
    H, W, verts = fx['H'], fx['W'], fx['verts']
    T = verts.shape[0]
    rng = np.random.default_rng(fx['seed'] if seed is None else seed)
    masks = np.ones((T, H, W), np.uint8)
    base = evaluate(verts, fx['faces'], fx['K'], planes, masks, flows=np.zeros((T - 1, H, W, 3), np.float32))
    r, c = np.mgrid[:H, :W].astype(np.float64)
    flows = np.zeros((T - 1, H, W, 3), np.float32)
    occs = np.zeros((T - 1, H, W), np.float32)
    for t in range(T - 1):
        a, b, p, q = rng.uniform(0, 2 * np.pi, 4)
        mag = 2.5 + 2.5 * np.sin(2 * np.pi * r / H * 1.3 + a) * np.cos(2 * np.pi * c / W * 0.9 + b)     # 0 .. 5 px
        ang = 2 * np.pi * (r / H + c / W) + p + np.sin(q + c / 7.)
        fl = np.stack([mag * np.cos(ang), mag * np.sin(ang)], -1)
        rr, cc, fp = base['flow_px'][t]
        fl[rr, cc] += fp
        flows[t, :, :, :2] = fl
        flows[t, :, :, 2] = 1.
        flows[t, :, 30:34, 2] = 0.                                    # invalid through channel 2
        occs[t, 20:23] = 10. + t                                      # occluded
    return masks, flows, occs


# ---- a sequence on disk ---------------------------------------------------------------------------------------------------------------------
def write_sequence(root, name, verts, faces, K, frames, masks, flows=None, occs=None, colors=None, dframe=1, ext='png'):
    """What eval_reproj.py reads, in the DAVIS layout under `root`: configs/<name>.config, frames, annotations, per frame
    pred<i>.ply (with colours) or .obj and cam<i>.txt, and FlowFW maps between consecutive listed frames."""
    from PIL import Image
    import torch
    from lasr_amd.ext_utils.ply import write_ply
    from lasr_amd.ext_utils.util_flow import write_pfm
    from lasr_amd.soft_renderer.functional import save_obj
    base = os.path.join(root, 'database', 'DAVIS')
    img_dir = os.path.join(base, 'JPEGImages', 'Full-Resolution', name)
    ann_dir = os.path.join(base, 'Annotations', 'Full-Resolution', name)
    flo_dir = os.path.join(base, 'FlowFW', 'Full-Resolution', name if dframe == 1 else '%s_%02d' % (name, dframe))
    test = os.path.join(root, 'out-' + name)
    for d in (img_dir, ann_dir, flo_dir, test, os.path.join(root, 'configs')):
        os.makedirs(d, exist_ok=True)
    with open(os.path.join(root, 'configs', '%s.config' % name), 'w') as f:
        f.write('[data]\ndatapath = database/DAVIS/JPEGImages/Full-Resolution/%s/\ndframe = %d\ncan_frame = 0\ninit_frame = 0\n'
                'end_frame = -1\n' % (name, dframe))
    filler = np.zeros_like(frames[0])
    for i in range(len(verts)):
        fr = i * dframe
        Image.fromarray(frames[i]).save(os.path.join(img_dir, '%05d.%s' % (fr, ext)))
        Image.fromarray(masks[i]).save(os.path.join(ann_dir, '%05d.png' % fr))
        for skipped in range(fr + 1, fr + dframe if i + 1 < len(verts) else fr + 1):      # frames the config's dframe skips
            Image.fromarray(filler).save(os.path.join(img_dir, '%05d.%s' % (skipped, ext)))
        if colors is not None:
            write_ply(os.path.join(test, 'pred%d.ply' % fr), verts[i], faces, colors=colors[i])
        else:
            save_obj(os.path.join(test, 'pred%d.obj' % fr), torch.from_numpy(verts[i]), torch.from_numpy(faces))
        rtk = np.eye(4)
        rtk[3] = K[i]
        np.savetxt(os.path.join(test, 'cam%d.txt' % fr), rtk)
        if flows is not None and i + 1 < len(verts):
            write_pfm(os.path.join(flo_dir, 'flo-%05d.pfm' % fr), np.ascontiguousarray(flows[i], np.float32))
            if occs is not None:
                write_pfm(os.path.join(flo_dir, 'occ-%05d.pfm' % fr), np.ascontiguousarray(occs[i], np.float32))
    return test
