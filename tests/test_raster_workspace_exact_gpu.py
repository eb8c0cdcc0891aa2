"""The raster through the C ABI with a workspace of EXACTLY lasr_sr_workspace_bytes(N, F, T, IS) bytes and every output the
kernels write carved out of guard-banded, poisoned buffers (tests/guarded.py): through the operator the workspace is at least
1 MiB and usually left over from a larger call, so nothing there shows a kernel that steps past the layout's end.

Per (N, F, IS) and channel count every forward kernel is forced in turn (lasr_sr_options and the forward flags; the plan
lasr_sr_plan_forward reports is asserted, so `forced` is not a hope), at N = 8 in both tile orders; the backward then runs on
the forward's records (LASR_SR_RECORDS_VALID) and with a rebuild, both with LASR_SR_GRADS_OVERWRITE.  Asserted: no band of any
buffer touched, and the same bits in every output under the fills 0xFF and 0x7F.  The float64 entry points run at the first two
sizes with their gradients at the 1e-9 bar of tests/test_raster_fp64_gpu.py (double atomics), once with a faces_info tensor and
once without one: then the forward and the backward each build the per-face data in the workspace, the only code that can step
past lasr_sr_workspace_bytes_f64.  The backward-only workspace size (IS = 0, tests/test_raster_parity_gpu.py) has a case of its
own.

Every output starts as poison: faces_info and aggrs_info are pure outputs in both precisions.  Only what include/lasr_sr.h has
the caller pre-fill is pre-filled, for the float64 entry points: soft_colors with the background, the gradients with zeros.
The generic 16x16 kernel runs at three channels only: six and nine channels exist in LASR's mode combination alone."""
import numpy as np
import pytest
import torch

import guarded
import raster_harness as rh
from lasr_amd import _lib
from raster_harness import BIG

pytestmark = pytest.mark.gpu

SIZES = [(1, 1, 8), (3, 65, 24), (2, 257, 33), (8, 65, 64)]
LASR, HARD = {}, dict(dist_func='hard', aggr_func_rgb='hard', aggr_func_alpha='hard')       # LASR's modes and the all-hard combination
#             name: (coop8_max, coop_max, choose_max, pair_min_tiles), forward flags, modes, plan forms accepted
KERNELS = {'one wave': ((0, 0, 0, BIG), 0, LASR, (_lib.SR_FORM_ONE_WAVE,)),
           'four waves': ((0, BIG, BIG, BIG), 0, LASR, (_lib.SR_FORM_FOUR_WAVES,)),
           'eight waves': ((BIG, BIG, BIG, BIG), 0, LASR, (_lib.SR_FORM_EIGHT_WAVES,)),
           'generic, hard modes': ((0, 0, 0, BIG), 0, HARD, (_lib.SR_FORM_GENERIC,)),
           'pair walk, one team': ((0, 0, 0, 0), _lib.SR_PAIR_ONE_TEAM, LASR, (_lib.SR_FORM_PAIRS_ONE_TEAM,)),
           'pair walk, two teams': ((0, 0, 0, 0), _lib.SR_PAIR_TWO_TEAMS, LASR, (_lib.SR_FORM_PAIRS_TWO_TEAMS,))}
FP64_GRAD_REL = 1e-9                                         # tests/test_raster_fp64_gpu.py


def inputs(dev, N, F, IS, C, dtype=torch.float32):
    fv, near, far = rh.raster_batch(N, F)
    g = torch.Generator().manual_seed(60 + C)
    tfv = torch.from_numpy(fv).reshape(N, F, 9).to(dtype).to(dev).contiguous()
    tft = torch.rand(N, F, 3 * C, generator=g).to(dtype).to(dev)
    up = (torch.randn(N, C + 1, IS, IS, generator=g) / (IS * IS)).to(dtype).to(dev)
    return tfv, tft, up, float(near), float(far)


def run_fp32(dev, fill, N, F, IS, C, options, flags, modes, ws_is=None, with_faces_info=False):
    """One forward and the two backwards under one fill -> (named outputs, band violations)."""
    h = _lib.lib()
    g = guarded.Guard(fill)
    tfv, tft, up, near, far = inputs(dev, N, F, IS, C)
    new = lambda *s: g.allocate(s, torch.float32, dev)                                            # noqa: E731
    nbytes = h.lasr_sr_workspace_bytes(N, F, 3, IS)
    bufs = dict(ws=g.allocate((nbytes,), torch.uint8, dev), colors=new(N, C + 1, IS, IS), aggrs=new(N, 2, IS, IS))
    if with_faces_info:
        bufs['faces_info'] = new(N, F, 27)
    t = rh.tail(**modes)
    rec = rh.forward(dev, tfv, tft.view(N, F, 3, C), near, far, IS, options=options, flags=flags, background=[1.] * C, out=bufs, scalars=t)
    out = {'soft_colors': rec.colors, 'aggrs_info': rec.aggrs}
    if rec.faces_info is not None:
        out['faces_info'] = rec.faces_info
    bws = None
    if ws_is is not None:                                     # the backward-only size: records and rects, no tile-order table
        bbytes = h.lasr_sr_workspace_bytes(N, F, 3, ws_is)
        assert bbytes < nbytes
        bws = g.allocate((bbytes,), torch.uint8, dev)
    for name, bflags in (('records', _lib.SR_RECORDS_VALID | _lib.SR_GRADS_OVERWRITE), ('rebuild', _lib.SR_GRADS_OVERWRITE)):
        if ws_is is not None and name == 'records':
            continue                                          # (the small workspace holds no forward's records)
        gf, gt = rh.backward(dev, rec, up, near, far, IS, flags=bflags, into=(new(N, F, 9), new(N, F, 3 * C)), scalars=t, ws=bws)
        out['grad_faces, ' + name], out['grad_textures, ' + name] = gf, gt
    return out, g.violations(), len(g.allocations)


def same_outputs(what, a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        x, y = guarded._bits(a[k]), guarded._bits(b[k])
        assert torch.equal(x, y), '%s: %s differs between the fills in %d bytes' % (what, k, int((x != y).sum()))


def check_fp32(dev, N, F, IS, C, name, order_max, **kw):
    th, flags, modes, forms = KERNELS[name]
    options = _lib.SrOptions(th[0], th[1], th[2], order_max, th[3])
    p = rh.plan(N, F, C, IS, options, flags, rh.tail(**modes))
    what = 'N=%d F=%d IS=%d C=%d, %s, order_max_tiles=%d' % (N, F, IS, C, name, order_max)
    assert p.form in forms, '%s: planned form %d' % (what, p.form)
    runs = []
    for fill in guarded.FILLS:
        out, bad, n_alloc = run_fp32(dev, fill, N, F, IS, C, options, flags, modes, **kw)
        assert n_alloc >= 6 and not bad, '%s, fill 0x%02X: guard band touched: %s' % (what, fill, bad)
        runs.append(out)
    same_outputs(what, runs[0], runs[1])
    assert bool((runs[0]['soft_colors'] != runs[0]['soft_colors'].reshape(-1)[0]).any())
    return p


@pytest.mark.parametrize('C', [3, 9])
@pytest.mark.parametrize('N,F,IS', SIZES)
def test_every_forward_kernel_and_both_backwards_inside_an_exact_workspace(cuda, N, F, IS, C):
    orders = (0, BIG) if N == 8 else (-1,)
    ordered = set()
    for name in KERNELS:
        if C != 3 and KERNELS[name][2] != LASR:
            continue                                          # (six and nine channels exist in LASR's modes only: the library refuses others)
        for order_max in orders:
            p = check_fp32(cuda, N, F, IS, C, name, order_max, with_faces_info=(C == 3 and name == 'one wave'))
            if KERNELS[name][2] == LASR:
                ordered.add((order_max, p.ordered))
    if N == 8:                                                # both tile orders ran: the fixed one and the launch's own
        assert (0, 0) in ordered and (BIG, 1) in ordered, ordered


def test_the_backward_alone_inside_the_records_only_workspace(cuda):
    check_fp32(cuda, 3, 65, 24, 3, 'one wave', -1, ws_is=0)


def run_fp64(dev, fill, N, F, IS, modes, with_faces_info):
    h = _lib.lib()
    g = guarded.Guard(fill)
    dt = torch.float64
    tfv, tft, up, near, far = inputs(dev, N, F, IS, 3, dt)
    new = lambda *s: g.allocate(s, dt, dev)                                                        # noqa: E731
    nbytes = h.lasr_sr_workspace_bytes_f64(N, F)
    ws = g.allocate((nbytes,), torch.uint8, dev)
    colors, aggrs = new(N, 4, IS, IS).fill_(1.), new(N, 2, IS, IS)
    finfo = new(N, F, 27) if with_faces_info else None          # None: the per-face data goes into the workspace, in both passes
    info_ptr = finfo.data_ptr() if finfo is not None else None
    gf, gt = new(N, F, 9).zero_(), new(N, F, 9).zero_()
    st = torch.cuda.current_stream(dev).cuda_stream
    t = rh.tail(**modes)
    _lib.check(h.lasr_sr_forward_f64(tfv.data_ptr(), tft.data_ptr(), info_ptr, aggrs.data_ptr(), colors.data_ptr(), ws.data_ptr(),
                                     nbytes, N, F, 3, IS, near, far, *t, st), 'lasr_sr_forward_f64')
    _lib.check(h.lasr_sr_backward_f64(tfv.data_ptr(), tft.data_ptr(), colors.data_ptr(), info_ptr, aggrs.data_ptr(), gf.data_ptr(),
                                      gt.data_ptr(), up.data_ptr(), ws.data_ptr(), nbytes, N, F, 3, IS, near, far, *t, st),
               'lasr_sr_backward_f64')
    exact = {'soft_colors': colors, 'aggrs_info': aggrs}
    if finfo is not None:
        exact['faces_info'] = finfo
    else:                                                     # what the two passes left in the workspace: the 256-byte aligned records
        at = (-ws.data_ptr()) % 256
        exact['records in the workspace'] = ws[at:at + N * F * 27 * 8]
    return exact, {'grad_faces': gf, 'grad_textures': gt}, g.violations()


@pytest.mark.parametrize('with_faces_info', [False, True], ids=['records-in-workspace', 'faces_info'])
@pytest.mark.parametrize('modes', [LASR, HARD], ids=['lasr', 'hard'])
@pytest.mark.parametrize('N,F,IS', SIZES[:2])
def test_the_float64_entry_points_inside_an_exact_workspace(cuda, N, F, IS, modes, with_faces_info):
    assert _lib.lib().lasr_sr_workspace_bytes_f64(N, F) >= N * F * 27 * 8
    runs = []
    for fill in guarded.FILLS:
        exact, grads, bad = run_fp64(cuda, fill, N, F, IS, modes, with_faces_info)
        assert not bad, 'fill 0x%02X: guard band touched: %s' % (fill, bad)
        runs.append((exact, grads))
    same_outputs('float64 N=%d F=%d IS=%d' % (N, F, IS), runs[0][0], runs[1][0])
    for k in runs[0][1]:                                      # double atomics: another order of the same sums
        a, b = runs[0][1][k].cpu().numpy(), runs[1][1][k].cpu().numpy()
        assert np.isfinite(a).all() and np.isfinite(b).all()
        scale = max(float(np.abs(b).max()), 1e-300)
        assert float(np.abs(a - b).max()) <= FP64_GRAD_REL * scale, (k, float(np.abs(a - b).max()), scale)
