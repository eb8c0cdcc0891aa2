"""What the raster tests share: the mode scalars and launch options, the direct C-ABI calls (lasr_sr_forward_opt, lasr_sr_plan_forward,
lasr_sr_backward_ex), the call through the operator, the oracle reference triple by triple, the workspace layout of
lasr_amd/csrc/sr_raster.hip (sr_layout), the comparisons and the scenes that more than one file renders.  A plain module: no fixtures;
the `oracle` and `cuda` fixtures of tests/conftest.py are passed in as arguments.  A test file keeps what is its own -- its scenes,
case tables, tolerances, messages and assertions -- and where two files differ in a detail (a fill, a background, an offset) it is
a parameter here and each file passes its value."""
import ctypes
import importlib
import math
import types

import numpy as np
import torch

from lasr_amd import _lib, synth
from lasr_amd.soft_renderer import functional as srf

# ---- mode scalars, options, bars ------------------------------------------------------------------------------------------------------
BIG = 10 ** 12
#                  coop8_max  coop_max  choose_max  order_max  pair_min_tiles      (lasr_sr_options, include/lasr_sr.h)
PAIR_WALK = (0, 0, 0, -1, 0)              # every launch through the pair-walk kernel
PAIR_WALK_FIXED = (0, 0, 0, 0, 0)         # ... in the fixed tile order
PAIR_WALK_OWN = (0, 0, 0, BIG, 0)         # ... in the launch's own order wherever one can be built
ONE_WAVE = (0, 0, 0, -1, BIG)             # one wave per 8x8 tile, faces in index order
PAIR_TOL = 1e-6                           # the pair walk's image against the oracle and against the reference-order kernels
GRAD_REL = 1e-3                           # gradients, of the largest reference gradient

_DIST = {'hard': 0, 'barycentric': 1, 'euclidean': 2}
_RGB = {'hard': 0, 'softmax': 1}
_ALPHA = {'hard': 0, 'sum': 1, 'prod': 2}
_TEX = {'surface': 0, 'vertex': 1}


def tail(sigma=None, alpha='prod', **overrides):
    """The nine scalars every raster entry point takes after near / far (include/lasr_sr.h) for synth.LASR_MODES, with another
    sigma_val, aggr_func_alpha or any other mode given by name."""
    m = dict(synth.LASR_MODES, aggr_func_alpha=alpha)
    m.update(overrides)
    if sigma is not None:
        m['sigma_val'] = sigma
    return (float(m['eps']), float(m['sigma_val']), _DIST[m['dist_func']], float(math.log(1. / m['dist_eps'] - 1.)), float(m['gamma_val']),
            _RGB[m['aggr_func_rgb']], _ALPHA[m['aggr_func_alpha']], _TEX[m['texture_type']], 1 if m['fill_back'] else 0)


_cache = {}


def cached(key, fn):
    """fn() computed once per key (scenes, oracle references: the tests leave them unchanged)."""
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


# ---- direct ABI calls -----------------------------------------------------------------------------------------------------------------
def _on(dev, x, shape=None):
    t = x if torch.is_tensor(x) else torch.from_numpy(np.array(x, np.float32))
    t = t.to(dev)
    return (t.reshape(*shape) if shape is not None else t).contiguous()


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def carve_at_offset(dev, shape, offset_floats):
    """A NaN-filled float tensor of `shape` that starts `offset_floats` floats into its (256-byte aligned) buffer."""
    n = int(np.prod(shape))
    buf = torch.full((n + offset_floats,), float('nan'), dtype=torch.float32, device=dev)
    t = buf[offset_floats:].view(*shape)
    assert t.data_ptr() % 16 == (4 * offset_floats) % 16
    return t


def carve_odd(dev, shapes, poison):
    """Tensors of `shapes` inside one `poison`-filled float buffer: the first starts one float behind the (256-byte aligned)
    allocation, the gaps are odd numbers of floats, so every start is 4-byte aligned and no more."""
    sizes = [int(np.prod(s)) for s in shapes]
    buf = torch.full((sum(sizes) + 8 * len(sizes) + 8,), poison, device=dev)
    assert buf.data_ptr() % 256 == 0
    out, at = [], 1
    for s, n in zip(shapes, sizes):
        t = buf[at:at + n].view(*s)
        assert t.data_ptr() % 8 == 4 and t.is_contiguous()
        out.append(t)
        at += n + (4 if n % 2 == 0 else 3)                          # the next start stays odd
    return buf, out


def plan(N, F, C, IS, options, flags=0, scalars=None):
    """What lasr_sr_plan_forward says of a launch (host only)."""
    t = scalars if scalars is not None else tail()
    opt = options if isinstance(options, _lib.SrOptions) else _lib.SrOptions(*options)
    p = _lib.SrPlan()
    _lib.check(_lib.lib().lasr_sr_plan_forward(N, F, 3, C, IS, t[2], t[5], t[6], t[7], t[8], flags, ctypes.byref(opt), ctypes.byref(p)),
               'lasr_sr_plan_forward')
    return p


def forward(dev, fv, tex, near, far, IS, *, options=None, flags=0, background=None, prefill=None, out=None, plain_entry=False,
            faces_info=False, scalars=None, fill=float('nan')):
    """lasr_sr_forward_opt (or the plain lasr_sr_forward) on face_vertices [N, F, 3, 3] and attributes [N, F, 3, C], numpy arrays or
    tensors.  The image and the aggregates start as `fill`, the workspace as lasr_sr_workspace_bytes zeroed bytes, unless `out`
    brings tensors of the caller's ('colors', 'aggrs', 'ws', 'faces_info': carved, guarded or kept from an earlier call);
    `prefill` writes a background into the image for a call without the background argument.  `options`: a lasr_sr_options tuple
    (the plan is then asked first) or None.  Returns a record of fv, tex, colors, aggrs, ws, faces_info and plan."""
    h = _lib.lib()
    N, F = fv.shape[:2]
    C = int(tex.shape[-1])
    assert tex.ndim == 4 and tex.shape[2] == 3
    out = dict(out or {})
    t = scalars if scalars is not None else tail()
    rec = types.SimpleNamespace(fv=_on(dev, fv, (N, F, 9)), tex=_on(dev, tex), plan=None)
    rec.colors = out['colors'] if 'colors' in out else torch.full((N, C + 1, IS, IS), fill, dtype=torch.float32, device=dev)
    rec.aggrs = out['aggrs'] if 'aggrs' in out else torch.full((N, 2, IS, IS), fill, dtype=torch.float32, device=dev)
    if prefill is not None:                                    # no background argument: the caller's image is the background
        for k in range(C):
            rec.colors[:, k] = prefill[k]
    rec.ws = out['ws'] if 'ws' in out else torch.zeros(h.lasr_sr_workspace_bytes(N, F, 3, IS), dtype=torch.uint8, device=dev)
    rec.faces_info = out.get('faces_info', torch.zeros(N, F, 27, device=dev) if faces_info else None)
    info = rec.faces_info.data_ptr() if rec.faces_info is not None else None
    if plain_entry:
        assert C == 3 and background is None and options is None
        _lib.check(h.lasr_sr_forward(rec.fv.data_ptr(), rec.tex.data_ptr(), info, rec.aggrs.data_ptr(), rec.colors.data_ptr(), rec.ws.data_ptr(),
                                     rec.ws.numel(), N, F, 3, IS, float(near), float(far), *t, _stream(dev)), 'lasr_sr_forward')
    else:
        opt = None
        if options is not None:
            opt = options if isinstance(options, _lib.SrOptions) else _lib.SrOptions(*options)
            rec.plan = plan(N, F, C, IS, opt, flags, t)
        cbg = (ctypes.c_float * C)(*background) if background is not None else None
        _lib.check(h.lasr_sr_forward_opt(rec.fv.data_ptr(), rec.tex.data_ptr(), info, rec.aggrs.data_ptr(), rec.colors.data_ptr(),
                                         rec.ws.data_ptr(), rec.ws.numel(), N, F, 3, C, IS, float(near), float(far), None, *t, cbg, flags,
                                         ctypes.byref(opt) if opt is not None else None, _stream(dev)), 'lasr_sr_forward_opt')
    torch.cuda.synchronize()
    return rec


def record(fv, tex, colors, aggrs, ws):
    """A forward's record from tensors a test filled through another entry point: what backward() reads."""
    return types.SimpleNamespace(fv=fv, tex=tex, colors=colors, aggrs=aggrs, ws=ws, faces_info=None, plan=None)


def backward(dev, rec, g, near, far, IS, *, flags=0, colors=None, aggrs=None, into=None, scalars=None, ws=None, nbytes=None,
             check=True):
    """lasr_sr_backward_ex on a forward's record -> (grad_faces [N, F, 9], grad_textures [N, F, 3, C]), tensors.  `colors` / `aggrs`:
    re-housed copies of what the backward reads; `into`: the caller's (grad_faces, grad_textures) instead of zeroed ones; `ws` /
    `nbytes`: another workspace, another size told.  check=False: the return code, nothing raised."""
    N, F = rec.fv.shape[:2]
    C = rec.colors.shape[1] - 1
    t = scalars if scalars is not None else tail()
    g = _on(dev, g)
    gf, gt = into if into is not None else (torch.zeros(N, F, 9, device=dev), torch.zeros(N, F, 3, C, device=dev))
    colors, aggrs, ws = (rec.colors if colors is None else colors), (rec.aggrs if aggrs is None else aggrs), (rec.ws if ws is None else ws)
    rc = _lib.lib().lasr_sr_backward_ex(rec.fv.data_ptr(), rec.tex.data_ptr(), colors.data_ptr(), aggrs.data_ptr(), gf.data_ptr(),
                                        gt.data_ptr(), g.data_ptr(), ws.data_ptr(), ws.numel() if nbytes is None else nbytes, N, F, 3, C, IS,
                                        float(near), float(far), None, *t, flags, _stream(dev))
    if not check:
        return rc
    _lib.check(rc, 'lasr_sr_backward_ex')
    torch.cuda.synchronize()
    return gf, gt


# ---- through the operator -------------------------------------------------------------------------------------------------------------
class _Ctx:                                 # what SoftRasterizeFunction.forward needs of an autograd context: it keeps aggrs_info
    def save_for_backward(self, *t):
        self.saved = t

    def mark_non_differentiable(self, *t):
        pass


def render(dev, scene, IS, background=None, *, want_aggrs=True, grad=None, raw=False, numpy=True, **modes):
    """A scene (face_vertices, textures, near, far) through the operator in LASR's modes (`modes`: others by name), with the launch
    thresholds and forward flags in force.  grad: the upstream gradient -> (image, grad_faces, grad_textures) through autograd;
    raw: (image, aggrs_info) of soft_rasterize_raw, which pre-fills the background; want_aggrs: (image, aggrs_info) of the
    Function's forward on a stand-in context; else the image of soft_rasterize.  numpy=False leaves the results on the device."""
    fv, ft = scene[:2]
    kw = dict(synth.LASR_MODES, **modes)
    if len(scene) == 4:                     # (a scene of two leaves near and far to `modes`)
        kw['near'], kw['far'] = scene[2:]
    if background is not None:
        kw['background_color'] = background
    a = fv if torch.is_tensor(fv) else torch.from_numpy(fv).to(dev)
    b = ft if torch.is_tensor(ft) else torch.from_numpy(ft).to(dev)
    if grad is not None:
        a, b = a.requires_grad_(True), b.requires_grad_(True)
        img = srf.soft_rasterize(a, b, IS, **kw)
        img.backward(grad if torch.is_tensor(grad) else torch.from_numpy(grad).to(dev))
        res = (img.detach(), a.grad, b.grad)
    elif raw:
        res = srf.soft_rasterize_raw(a, b, IS, **kw)
    elif want_aggrs:
        ctx = _Ctx()
        sr_mod = importlib.import_module('lasr_amd.soft_renderer.functional.soft_rasterize')
        res = (sr_mod.SoftRasterizeFunction.forward(ctx, a, b, IS, **kw), ctx.saved[3])
    else:
        res = (srf.soft_rasterize(a, b, IS, **kw),)
    if numpy:
        torch.cuda.synchronize()
        res = tuple(r.cpu().numpy() for r in res)
    return res if len(res) > 1 else res[0]


def operator_workspace(dev):
    """The workspace the operator's calls on the current stream share."""
    sr_mod = importlib.import_module('lasr_amd.soft_renderer.functional.soft_rasterize')
    return sr_mod._workspaces[(dev.index, _stream(dev))]


def peek_choice(dev, N, F):
    """The word the device-side kernel choice of the operator's last forward left in its workspace (lasr_sr_peek_choice)."""
    c = ctypes.c_int(-1)
    _lib.check(_lib.lib().lasr_sr_peek_choice(operator_workspace(dev).data_ptr(), N, F, ctypes.byref(c), None), 'lasr_sr_peek_choice')
    return c.value


# ---- the oracle, triple by triple -----------------------------------------------------------------------------------------------------
def oracle_reference(oracle, fv, tex, IS, background, modes, *, g=None, dtype=np.float32):
    """(image [N, C + 1, IS, IS], grad_faces [N, F, 3, 3], grad_textures [N, F, 3, C]) of oracle/sr_oracle for C = 3, 6 or 9
    attributes: the oracle renders three channels, the channels are independent, so every triple is a render of its own with its
    three values of `background` (None: the modes' own).  Alpha comes last in the image, and its upstream gradient g[:, C] is counted
    with the first triple only.  The gradients are None without g.  Read-only arrays."""
    N, F = fv.shape[:2]
    C = int(tex.shape[-1])
    kw = dict(modes)
    img = np.zeros((N, C + 1, IS, IS), dtype)
    gf, gt = None, None
    if g is not None:
        gf, gt = 0, np.zeros((N, F, 3, C), dtype)
    if F == 0:                              # (the oracle's wrapper cannot shape zero faces: K.cu:458-482 with no fragment)
        img[:, :C] = np.asarray(background, dtype)[None, :, None, None]
        gf = np.zeros((N, 0, 3, 3), dtype) if g is not None else None
    for k in range(0, C if F else 0, 3):
        if background is not None:
            kw['background_color'] = background[k:k + 3]
        ref = oracle.forward(fv, np.ascontiguousarray(tex[..., k:k + 3]), IS, dtype=dtype, **kw)
        img[:, k:k + 3], img[:, C] = ref['soft_colors'][:, :3], ref['soft_colors'][:, 3]
        if g is not None:
            gk = np.concatenate([g[:, k:k + 3], g[:, C:C + 1] if k == 0 else np.zeros_like(g[:, C:C + 1])], 1)
            gf_k, gt_k = oracle.backward(ref, gk, IS, dtype=dtype, **kw)
            gf = gf + gf_k
            gt[..., k:k + 3] = gt_k
    for a in (img, gf, gt):
        if a is not None:
            a.setflags(write=False)
    return img, gf, gt


# ---- the workspace layout (sr_raster.hip: sr_layout) ----------------------------------------------------------------------------------
REC_FLOATS = 48                             # sr_device.h: REC, floats per face record
GROUP = 64                                  # faces per group rect


def layout(ws, N, F, IS):
    """Byte offsets of the workspace's parts from the start of `ws` (a uint8 tensor, or its address): records, pixel rects, group
    rects, the choice word, the order table; `total` is the size lasr_sr_workspace_bytes asks for."""
    up = lambda v: (v + 255) // 256 * 256                      # noqa: E731
    ptr = ws if isinstance(ws, int) else ws.data_ptr()
    t8 = (IS + 7) // 8 if IS > 0 else 0
    L = types.SimpleNamespace(recs=(-ptr) % 256)
    L.rects = L.recs + up(N * F * REC_FLOATS * 4)
    L.grects = L.rects + up(N * F * 8)
    L.choice = L.grects + up(N * ((F + GROUP - 1) // GROUP) * 8)
    L.order = L.choice + 256
    L.total = L.order - L.recs + up(N * t8 * t8 * 4) + up(N * t8 * t8) + 256
    return L


def order_table(ws, N, F, IS, tile):
    """The block -> tile table the last forward left in `ws`, for a launch in tiles of `tile` (8 or 16) pixels."""
    t = (IS + tile - 1) // tile
    o = layout(ws, N, F, IS).order
    return ws[o:o + N * t * t * 4].view(torch.int32).cpu().numpy()


def pixel_rects(ws, N, F):
    """The set-up kernel's pixel rects [N, F, 4]: x0, x1, y0, y1."""
    o = layout(ws, N, F, 0).rects
    return ws[o:o + N * F * 8].view(torch.int16).reshape(N, F, 4).cpu().numpy().astype(np.int64)


# ---- comparisons ----------------------------------------------------------------------------------------------------------------------
def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def check_grad(what, got, ref, rel=GRAD_REL):
    scale = float(np.abs(ref).max())
    d = float(np.abs(got - ref).max())
    print('%s: max diff %.3e, largest gradient %.3e (%.2e of it)' % (what, d, scale, d / scale if scale > 0 else float('inf')))
    assert np.isfinite(got).all() and scale > 0 and d <= rel * scale, '%s: max diff %.3e vs largest gradient %.3e' % (what, d, scale)


# ---- scenes that more than one file renders -------------------------------------------------------------------------------------------
def blob(N, scale=None, shift=(0., 0.)):
    """(face_vertices [N, 320, 3, 3], near, far): N frames of the level-4 blob's turn, x and y scaled, then shifted."""
    fv, _, near, far = synth.raster_batch(4, max(N, 3), count=N)
    fv = fv.copy()
    if scale is not None:
        fv[..., :2] *= scale
    for k in range(2):
        if shift[k]:
            fv[..., k] += shift[k]
    return np.ascontiguousarray(fv), float(near), float(far)


def raster_batch(N, F):
    """(face_vertices [N,F,3,3], near, far): the first F faces of the level-4 blob (320 faces), N frames of its turn."""
    fv, _, near, far = synth.raster_batch(4, max(N, 3), count=N)
    assert 1 <= F <= fv.shape[1]
    fv = fv[:, np.linspace(0, fv.shape[1] - 1, F).astype(np.int64)]
    return np.ascontiguousarray(fv), near, far


def stack(K):
    """K identical triangles at distinct depths over one 16x16 image: the vertical edge at x = -0.03 puts the pixel centres of
    columns 0..7 inside every face; all K pixel rects hold the whole tile's left half, so the tile's list has exactly K entries."""
    fv = np.zeros((1, K, 3, 3), np.float32)
    fv[0, :, :, :2] = np.asarray([[-0.03, -2.5], [-0.03, 2.5], [-3., 0.]], np.float32)
    fv[0, :, :, 2] = (2. + 0.02 * np.arange(K, dtype=np.float32))[:, None]
    ft = np.random.default_rng(K).uniform(0, 1, fv.shape).astype(np.float32)
    return fv, ft, 1.0, 5.0


def not_tame():
    """Two frames of the level-4 blob with a sliver, a zero-area face, a face in front of the near plane and huge coordinates among
    the tame faces of the same chunks."""
    fv, ft, near, far = synth.raster_batch(4, 3, count=2)
    fv = fv.copy()
    fv[0, 0] = [[0, 0, 3], [0.5, 0.5, 3], [1e-7, 0, 3]]
    fv[0, 1] = [[0.1, 0.1, 3], [0.1, 0.1, 3], [0.1, 0.1, 3]]
    fv[1, 2, :, 2] = 1e-9
    fv[1, 3] = [[-3e4, -2e4, 3], [4e4, -1e4, 3], [0, 5e4, 3]]
    return fv, ft, near, far


def hand_made():
    """name -> one face [3, 3]; coordinates chosen for 32 pixels (centres at odd multiples of 1/32)."""
    z = 3.
    return {
        'sliver': [[-0.8, -0.31, z], [0.7, -0.29, z], [0.7, -0.315, z]],                                  # 0.02 high: well conditioned, barely
        'edge-on, flag 16 clear': [[0., 0., z], [0.5, 0.5, z], [1e-7, 0., z]],
        'A == 0 on a pixel-centre row': [[-0.4, 0.03125, z], [0.5, 0.03125, z], [0.1, 0.6, z]],
        'edge through pixel centres': [[-0.46875, -0.46875, z], [0.53125, 0.53125, z], [-0.5, 0.5, z]],
        'half outside the image': [[0.6, -0.3, z], [1.8, 0.2, z], [0.7, 0.9, z]],
        'cut by the ragged edge': [[0.55, -0.95, z], [0.98, -0.6, z], [0.7, -0.2, z]],
        'rect covers a whole tile': [[-1.1, -0.5, z], [0.45, -0.45, z], [-0.5, 1.2, z]],
    }


def more_channels(ft, C, rng, lo=-2, hi=2):
    """Vertex colours [N, F, 3, 3] and C // 3 - 1 random attribute triples behind them."""
    return np.concatenate([ft] + [rng.uniform(lo, hi, ft.shape).astype(np.float32) for _ in range(C // 3 - 1)], -1)


def long_list(spread=0.08, big_face=True):
    """2500 faces in the centre of the image: the tiles there meet more faces than one LDS list holds (1024 / 2048 entries)."""
    rng = np.random.default_rng(7)
    F = 2500
    c = rng.uniform(-0.15, 0.15, (2, F, 1, 2))
    tri = c + rng.uniform(-spread, spread, (2, F, 3, 2))
    z = rng.uniform(2, 4, (2, F, 3, 1))
    fv = np.concatenate([tri, z], -1).astype(np.float32)
    if big_face:
        fv[0, 0] = [[-1.5, -1.2, 3], [1.4, -1.1, 3.5], [0.1, 1.6, 2.5]]
    ft = rng.uniform(0, 1, fv.shape).astype(np.float32)
    return fv, ft, 1.0, 5.0


def tri(xy, z=(2.5, 3.0, 3.5)):
    return [[x, y, zz] for (x, y), zz in zip(xy, z)]


def rot(t, k):                                   # vertex j of the result = vertex (j - k) % 3 of t: the first vertex moves to index k
    return [t[(j - k) % 3] for j in range(3)]


OBTUSE = [(0.02, 0.17), (-0.6, -0.15), (0.6, -0.1)]                # a triangle that is obtuse at its FIRST vertex


def constants_mesh(IS, n_faces=20):
    """face_vertices [2, 20, 3, 3] (the second frame: the first moved a little), float32, read-only: the mesh of
    tests/test_face_constants_gpu.py, whose docstring says what each face is there for."""
    return cached(('constants mesh', IS, n_faces), lambda: _constants_mesh(IS, n_faces))


def _constants_mesh(IS, n_faces):
    ax = 1. / IS + 2e-4                          # 2e-4 beside the pixel-centre column right of the image centre
    faces = [tri([(-0.5 + ax, -0.4), (0.5 + ax, -0.4), (ax, 0.55)], (2.5, 3.0, 3.5))]
    for k in range(3):
        t = rot(tri(OBTUSE, (2.2, 2.8, 3.1)), k)
        faces.append([[x + 0.1 * (k - 1), y + 0.25 * (k - 1), z + 0.1 * k] for x, y, z in t])
    # the sliver, around a pixel centre: its apex 0.008 NDC over the long edge -- below the 0.01 of flag 16 -- at an aspect of 7
    p = (2 * round(0.8 * IS) + 1 - IS) / IS
    faces.append(tri([(p - 0.03, p - 0.004), (p + 0.03, p - 0.003), (p + 0.004, p + 0.0045)], (3.2, 3.3, 3.4)))
    faces.append(tri([(2.0, -0.2), (2.4, -0.1), (2.1, 0.3)], (3.0, 3.0, 3.0)))                 # outside the image
    rng = np.random.default_rng(20)
    while len(faces) < n_faces:
        c = rng.uniform(-0.75, 0.75, 2)
        a0 = rng.uniform(0, 2 * math.pi)
        r = rng.uniform(0.12, 0.25, 3)
        ang = a0 + np.array([0., 2.1, 4.2]) + rng.uniform(-0.3, 0.3, 3)
        if rng.uniform() < 0.5:
            ang = ang[::-1]                                                                        # both windings
        faces.append(tri([(c[0] + r[j] * math.cos(ang[j]), c[1] + r[j] * math.sin(ang[j])) for j in range(3)], rng.uniform(2., 4., 3)))
    f = np.asarray(faces, np.float32)
    fv = np.stack([f, f])
    fv[1, :, :, 0] += 0.013
    fv[1, :, :, 1] -= 0.007
    fv.setflags(write=False)
    return fv
