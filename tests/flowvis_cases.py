"""Inputs of the flow colour-coding, contact-sheet and scalar-ring tests (tests/test_flowvis_cpu.py checks their properties without
a device, tests/test_flowvis_gpu.py runs them).  Float32 arrays, fixed seeds."""
import numpy as np

EXCLUDE_BAND = 1e-5          # pixels whose normalised radius is this close to 1: the `rad <= 1` branch decides a 0.75 darkening
EXCLUDE_MAX_PER_IMAGE = 4


def colour_cases():
    """name -> (flow [B,H,W,C] float32, mask [B,H,W] float32 or None)."""
    rng = np.random.default_rng(7)
    out = {}
    out['one_pixel'] = (np.array([[[[3., -4.]]]], np.float32), None)
    out['zeros_8x8'] = (np.zeros((1, 8, 8, 2), np.float32), None)
    f = (4. * rng.standard_normal((1, 37, 53, 2))).astype(np.float32)          # no multiple of 64 or of 4; two blocks of 4-pixel lanes
    f[0, -1, -1] = (30., 40.)                                                   # the maximum radius sits in the last pixel
    out['odd_37x53_max_last'] = (f, None)
    f = rng.standard_normal((3, 19, 23, 2))
    for b, top in enumerate((0.01, 1., 300.)):                                  # a reduction that leaks across images shows
        f[b] *= top / np.sqrt((f[b] ** 2).sum(-1)).max()
    out['batch3_maxima'] = (f.astype(np.float32), None)
    f = rng.standard_normal((1, 16, 16, 2)).astype(np.float32)
    f[0, 3, 5, 0] = 2e7
    f[0, 11, 2, 1] = np.nan
    out['unknown_and_nan'] = (f, None)
    out['three_channels'] = ((2. * rng.standard_normal((2, 12, 20, 3))).astype(np.float32), None)
    f = (25. * rng.standard_normal((2, 24, 24, 2))).astype(np.float32)
    out['masked'] = (f, (rng.random((2, 24, 24)) > 0.4).astype(np.float32))
    out['large_256'] = ((3. * rng.standard_normal((1, 256, 256, 2))).astype(np.float32), None)
    return out


def sheet_case(IS, n_bones, constant_error=False, seed=11):
    """Tensors as the trainer holds them for n_hypo = 2, batch_size = 2 (so img2 is imgs[2]) and optim_cam = 1.
    -> dict of float32 arrays in the model's layouts."""
    rng = np.random.default_rng(seed + IS + n_bones)
    H, B = 2, 2
    n2, N = 2 * B, 2 * B * H
    c = dict(IS=IS, n_hypo=H, batch_size=B, n_bones=n_bones, optim_cam=1)
    c['flow'] = (3. * rng.standard_normal((n2, 3, IS, IS))).astype(np.float32)
    c['flow_rd'] = (2. * rng.standard_normal((N, IS, IS, 2))).astype(np.float32)
    c['vis_mask'] = (rng.random((n2, H, IS, IS)) > 0.3).astype(np.uint8)
    c['flow_rd_map'] = np.full((n2, H, IS, IS), 0.25, np.float32) if constant_error else rng.random((n2, H, IS, IS)).astype(np.float32)
    if constant_error:
        c['vis_mask'][0, 1] = 1                           # error * mask is constant over the whole panel
    c['px'] = rng.random((N, 10, IS, IS)).astype(np.float32)        # the wide render: texture = planes 0..2, mask_pred = plane 9
    c['px'][:, :3] = c['px'][:, :3] * 1.2 - 0.1                     # some texels outside 0..1: clipped
    c['masks'] = (rng.random((n2, IS, IS)) > 0.5).astype(np.float32)
    c['imgs'] = rng.random((n2, 3, IS, IS)).astype(np.float32)
    if n_bones > 1:
        c['part_render'] = rng.random((1, 4, IS, IS)).astype(np.float32)[:, :3]
        ctl = (0.6 * rng.standard_normal((N, n_bones - 1, 3))).astype(np.float32)
        ctl[1, 0, :2] = (1.6, 0.2)                        # outside the tile
        ctl[1, 1, :2] = (-1., 0.1)                        # on its border: half a ring
        ctl[1, 2, :2] = (0.13, -0.37)
        c['ctl_proj'] = ctl
    return c


def sheet_planes(c):
    """The planes of a sheet_case as tests/flowvis_restated.sheet takes them (float32, planar)."""
    cam, B, H, IS = c['optim_cam'], c['batch_size'], c['n_hypo'], c['IS']
    p = dict(flow_obs=c['flow'][0, :2], flow_rd=c['flow_rd'].reshape(2 * B, H, IS, IS, 2)[0, cam].transpose(2, 0, 1),
             vis_mask=c['vis_mask'][0, cam].astype(np.float32), flow_err=c['flow_rd_map'][0, cam], mask_pred=c['px'][cam, 9],
             mask_gt=c['masks'][0], part=c['part_render'][0] if c['n_bones'] > 1 else None, img1=c['imgs'][0], img2=c['imgs'][B],
             texture=c['px'][cam, :3], ctl=None, palette=None)
    if c['n_bones'] > 1:
        from lasr_amd import synth
        p['ctl'], p['palette'] = c['ctl_proj'][cam], synth.label_palette(c['n_bones'] - 1)
    return p


SHEET_CASES = ((16, 4, False), (32, 4, False), (16, 1, False), (32, 4, True))     # (IS, n_bones, constant flow_error panel)

RING_COUNTS = (1, 8, 65, 1024)


def ring_pushes(n_push=5, seed=3):
    """n_push lists of len(RING_COUNTS) float32 arrays."""
    rng = np.random.default_rng(seed)
    return [[(rng.standard_normal(n) * 3 + 1).astype(np.float32) for n in RING_COUNTS] for _ in range(n_push)]
