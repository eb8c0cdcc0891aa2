"""numpy (float64) restatement of lasr_vis_shade (lasr_amd/csrc/vis.hip): given the same face-index maps the GPU rasteriser
produced (camera layers and light), the per-vertex and per-face records and the parameters, the expected uint8 frames.  The GPU
tests hold the kernel to it within 1/255, which isolates the shading pass from visibility."""
import numpy as np


def barycentric(sx, sy, xp, yp):
    """Screen-space barycentrics of points (xp, yp) [P] in triangles with NDC corners sx, sy [P,3] -> [P,3]."""
    x0, x1, x2 = sx.T
    y0, y1, y2 = sy.T
    den = (x1 - x0) * (y2 - y0) - (x2 - x0) * (y1 - y0)
    w0 = ((x1 - xp) * (y2 - yp) - (x2 - xp) * (y1 - yp)) / den
    w1 = ((x2 - xp) * (y0 - yp) - (x0 - xp) * (y2 - yp)) / den
    w2 = ((x0 - xp) * (y1 - yp) - (x1 - xp) * (y0 - yp)) / den
    return np.stack([w0, w1, w2], 1)


def pixel_centres(IS, H, W):
    """NDC of the pixel centres of the H x W crop, the rasteriser's convention (row 0 at NDC y = +1)."""
    r, c = np.mgrid[:H, :W]
    return (2. * c + 1 - IS) / IS, (2. * (IS - 1 - r) + 1 - IS) / IS


def _shade_layer(fmap, g_off, F_layer, vrec, faces, frec, smap, xf, S, F, xp, yp, p):
    """-> rgb [P,3], z [P], covered [P] for one layer of one frame."""
    P = xp.size
    g = fmap.reshape(-1)
    ok = (g >= 0) & (g < F_layer)
    gi = np.where(ok, g, 0).astype(np.int64) + g_off
    vi = faces[gi, :3]
    V = vrec.shape[0]
    ok &= ((vi >= 0) & (vi < V)).all(1)
    vi = np.where(vi >= 0, np.minimum(vi, V - 1), 0)
    rec = vrec[vi]                                                               # P,3,12
    pos, sx, nrm, sy, col = rec[..., 0:3], rec[..., 3], rec[..., 4:7], rec[..., 7], rec[..., 8:11]
    w = np.clip(barycentric(sx, sy, xp.reshape(-1), yp.reshape(-1)), 0, 1)
    lam = w / pos[..., 2]
    lam = lam / lam.sum(1, keepdims=True)
    P3 = (lam[..., None] * pos).sum(1)
    fr = frec[gi]
    if p['smooth']:
        n = (lam[..., None] * nrm).sum(1)
        nn = np.linalg.norm(n, axis=1, keepdims=True)
        n = np.where(nn > 1e-12, n / np.maximum(nn, 1e-30), fr[:, :3])
    else:
        n = fr[:, :3].copy()
    n = np.where(((n * P3).sum(1) > 0)[:, None], -n, n)
    d, u, v = np.asarray(p['light_d']), np.asarray(p['light_u']), np.asarray(p['light_v'])
    ndl = np.maximum(0., -(n @ d))
    pu, pv, pw = P3 @ u, P3 @ v, P3 @ d
    h = 2. / (xf[2] * S)
    lit = np.zeros(P)
    margin = np.full(P, np.inf)            # how far (in texels) the closest tap decision is from flipping
    for j in (-1, 0, 1):
        for i in (-1, 0, 1):
            qu, qv = pu + i * h, pv + j * h
            tx = ((qu - xf[0]) * xf[2] + 1) * 0.5 * S
            ty = ((qv - xf[1]) * xf[2] + 1) * 0.5 * S
            inside = (tx >= 0) & (tx < S) & (ty >= 0) & (ty < S)
            col_ = np.clip(np.floor(tx), 0, S - 1).astype(np.int64)
            row = S - 1 - np.clip(np.floor(ty), 0, S - 1).astype(np.int64)
            fo = smap[row, col_]
            occ_ok = inside & (fo >= 0) & (fo < F) & (fo.astype(np.int64) != gi)
            # depths at the centre of the tap's texel: the stored face's plane, the receiver's plane extended
            uc = xf[0] + (2 * col_ + 1 - S) / S / xf[2]
            vc = xf[1] + (2 * (S - 1 - row) + 1 - S) / S / xf[2]
            pl = frec[np.where(occ_ok, fo, 0).astype(np.int64), 4:7]
            w_occ = pl[:, 0] * uc + pl[:, 1] * vc + pl[:, 2]
            w_rec = pw + fr[:, 4] * (uc - pu) + fr[:, 5] * (vc - pv)
            lit += ~(occ_ok & (w_rec > w_occ + p['shadow_bias']))
            edge = np.minimum(np.abs(tx - np.round(tx)), np.abs(ty - np.round(ty)))
            depth = np.where(occ_ok, np.abs(w_rec - w_occ - p['shadow_bias']) / h, np.inf)
            margin = np.minimum(margin, np.minimum(edge, depth))
    s = np.where(ndl > 0, lit / 9., 1.)
    k = p['k_ambient'] + p['k_diffuse'] * ndl * s
    rgb = np.clip(0.6 * (lam[..., None] * col).sum(1) * k[:, None], 0, 1)
    return rgb, P3[:, 2], ok, s, np.where(ok & (ndl > 0), margin, np.inf)


def shade(maps, H, W):
    """Expected output of lasr_vis_shade for the inputs vis.shade(..., return_maps=True) handed to it -> uint8 [N,H,W,3] and
    the margin [N,H,W] of each pixel's shadow decisions in texels (float32 and float64 may decide a tap closer than ~1e-4 texel
    differently)."""
    t = lambda x: None if x is None else x.detach().cpu().numpy().astype(np.float64)
    vrec, frec, r0, r1, sh, xfs = (t(maps[k]) for k in ('vert_rec', 'face_rec', 'raster0', 'raster1', 'shadow', 'shadow_xf'))
    faces = maps['faces'].cpu().numpy().astype(np.int64)
    pr = maps['params']
    p = dict(light_u=list(pr.light_u), light_v=list(pr.light_v), light_d=list(pr.light_d), k_ambient=pr.k_ambient,
             k_diffuse=pr.k_diffuse, alpha=pr.surface_alpha, shadow_bias=pr.shadow_bias, bg=list(pr.background), smooth=pr.smooth)
    IS, S, F0 = maps['IS'], maps['S'], maps['F0']
    F = faces.shape[0]
    N = vrec.shape[0]
    xp, yp = pixel_centres(IS, H, W)
    out = np.zeros((N, H, W, 3), np.uint8)
    margin = np.full((N, H * W), np.inf)
    for n in range(N):
        crop = lambda r: r[n, 1, :H, :W]
        args = (vrec[n], faces, frec[n], sh[n, 1], xfs[n], S, F, xp, yp, p)
        rgb0, z0, ok0, _, m0 = _shade_layer(crop(r0), 0, F0, *args)
        margin[n] = m0
        rgb = np.where(ok0[:, None], rgb0, np.asarray(p['bg'])[None])
        if r1 is not None:
            rgb1, z1, ok1, _, m1 = _shade_layer(crop(r1), F0, F - F0, *args)
            margin[n] = np.minimum(margin[n], m1)
            use = ok1 & ~(ok0 & (z0 < z1))
            rgb = np.where(use[:, None], p['alpha'] * rgb1 + (1 - p['alpha']) * rgb, rgb)
        u8 = np.rint(np.clip(rgb, 0, 1) * 255)
        if maps['frames'] is not None:
            fr = maps['frames'][n].cpu().numpy().reshape(-1).view(np.uint8).reshape(-1, 4)[:, :3].astype(np.float64)
            u8 = np.rint(0.5 * u8 + 0.5 * fr)
        out[n] = u8.reshape(H, W, 3).astype(np.uint8)
    return out, margin.reshape(N, H, W)


def shadow_fraction(maps, H, W, n=0):
    """s of every pixel of layer 0 of frame n ([H,W], 1 where no face or the face is turned from the light)."""
    t = lambda x: x.detach().cpu().numpy().astype(np.float64)
    pr = maps['params']
    p = dict(light_u=list(pr.light_u), light_v=list(pr.light_v), light_d=list(pr.light_d), k_ambient=pr.k_ambient,
             k_diffuse=pr.k_diffuse, shadow_bias=pr.shadow_bias, smooth=pr.smooth)
    faces = maps['faces'].cpu().numpy().astype(np.int64)
    xp, yp = pixel_centres(maps['IS'], H, W)
    _, _, ok, s, _ = _shade_layer(t(maps['raster0'])[n, 1, :H, :W], 0, maps['F0'], t(maps['vert_rec'])[n], faces,
                               t(maps['face_rec'])[n], t(maps['shadow'])[n, 1], t(maps['shadow_xf'])[n], maps['S'],
                               faces.shape[0], xp, yp, p)
    return np.where(ok, s, 1.).reshape(H, W), ok.reshape(H, W)
