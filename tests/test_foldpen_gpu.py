"""The fold penalty of the optimiser on the device (scripts/fold_penalty.py, lasr_amd/csrc/foldpen.hip) against the float64
restatement (tests/foldpen_restated.py).  The penalty is this project's own addition: the restatement and closed forms are the only
parity there is.

Which entries are charged is compared for equality: tests/test_foldpen_cpu.py shows that over these fixtures no theta lies within
0.25 degrees of phi or of 0 and no determinant of a pierce test within 4 x its own float32 / float64 difference of zero.  Values and
gradients are held, per mesh, to 4 x max |float32 restatement - float64 restatement|, with a floor that is the largest difference
between two float32 restatements that differ in their order of operations (the arc tangent in float64 and rounded once; the rows
added per vertex in float32 in descending order): both come from restatements only, neither from what the kernels give.  A mesh
without a charged entry has bound 0: its values, loss and gradient are exactly 0.  Every shape is a fixture of the restatement: at
most 2560 faces and 3 meshes.  Every comparison prints its figures before it asserts.

Measured on an MI355X:
  batch3 (1890 entries; charged 0 / 3 / 5, as the restatement): values off by 0 / 3.7e-8 / 5.5e-8 (bounds 0 / 1.5e-7 / 1.3e-7), loss
    by 0 / 1.3e-8 / 6.3e-8 (bounds 0 / 4.8e-7 / 6.7e-7), gradient by 0 / 1.1e-6 / 1.8e-6 (bounds 0 / 4.0e-6 / 5.2e-6; the largest
    gradient entry is 13.4).  Frame 2 alone: the same figures.  At 90 degrees: values 3.2e-7 (9.8e-7), gradient 6.2e-6 (9.2e-6).
  tile257, flip1, pinch2, two2: nothing charged, every value, loss and gradient entry exactly 0.
  eight copies: 15 120 entries, loss 3.052016 / 0.941689 = 8 x 0.381502 / 0.117711, every entry and vertex gradient the base's bits.
  descent on the device: all counts 0 after 36 steps, as the restatement in both precisions; crease sum left 2.8e-4, pierce sum 0.
"""
import functools

import numpy as np
import pytest
import torch

import foldpen_guarded
import foldpen_restated as fr
import guarded
import meshnbr_guarded
import meshnbr_restated as nr
from test_foldpen_cpu import DESCENT

pytestmark = pytest.mark.gpu
U24 = 2. ** -24


def _fp():
    return foldpen_guarded.fold_penalty()


def _dev(cuda, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for a in arrays]


def _mesh(name):
    if name == 'frame2':                                                          # the folded frame of batch3 alone: N = 1
        verts, faces = nr.fixture('batch3')
        return verts[2:], faces
    return nr.fixture(name)


@functools.lru_cache(None)
def _restated(name, deg=30.):
    """The three restatements of a fixture, computed once and shared: float64, float32 and float32 in another order."""
    verts, faces = _mesh(name)
    top = nr.topology(faces)
    return (fr.penalty(verts, faces, deg, np.float64, top), fr.penalty(verts, faces, deg, np.float32, top),
            fr.penalty(verts, faces, deg, np.float32, top, variant=True), top)


def _bounds(r64, r32, alt, key):
    """Per mesh: max(4 max |float32 - float64|, max |float32 - float32 in another order|) of r[key] ([N, ...])."""
    a, b, c = (np.asarray(r[key], np.float64) for r in (r64, r32, alt))
    if key == 'grad':
        a, b, c = a.sum(0), b.sum(0), c.sum(0)                                      # upstream (1, 1): the sum of both planes
    ax = tuple(range(1, a.ndim))
    return np.maximum(4 * np.abs(b - a).max(ax), np.abs(b - c).max(ax)), a


def _held(name, what, got, bound, want):
    err = np.abs(np.asarray(got, np.float64) - want).max(tuple(range(1, want.ndim)))
    print('%s %s: off the float64 restatement by %s, bound %s' % (name, what, ['%.2e' % e for e in err], ['%.2e' % b for b in bound]))
    assert (err <= bound).all(), (name, what)


@pytest.mark.parametrize('name', ['batch3', 'frame2', 'tile257', 'flip1', 'pinch2', 'two2'])
def test_fixture_is_held_to_the_restatement(cuda, name):
    fp = _fp()
    r64, r32, alt, top = _restated(name)
    tv, tf = _dev(cuda, *_mesh(name))
    pen = fp.FoldPenalty(tf, 30.)
    assert np.array_equal(pen.keys.cpu().numpy(), top['keys'])
    loss, values, grad = (t.cpu().numpy() for t in foldpen_guarded.both(pen, tv))
    N = tv.shape[0]
    assert loss.shape == (N, 2) and values.shape == (N, top['n_list']) and grad.shape == tuple(tv.shape) and loss.dtype == np.float32
    charged = values != 0
    print('%s: %d entries, charged per mesh %s (restatement %s), loss %s' % (name, top['n_list'], charged.sum(1).tolist(),
                                                                             r64['active'].sum(1).tolist(), loss.tolist()))
    assert (charged == r64['active']).all() and (values >= 0).all()
    vb, want = _bounds(r64, r32, alt, 'values')
    _held(name, 'values', values, vb, want)
    # a sum of n charged float32 values, each off by at most vb, added in float64 and rounded once
    _held(name, 'loss', loss, r64['active'].sum(1) * vb + U24 * np.abs(r64['loss']).max(1), np.asarray(r64['loss'], np.float64))
    gb, want = _bounds(r64, r32, alt, 'grad')
    _held(name, 'gradient', grad, gb, want)
    if name in ('tile257', 'flip1', 'pinch2', 'two2'):                             # nothing between neighbours: exactly 0
        assert not loss.any() and not values.any() and not grad.any() and not vb.any() and not gb.any()
    else:
        assert loss[-1, 0] > 0.3 and loss[-1, 1] > 0.1 and np.abs(grad[-1]).max() > 1


def test_the_planes_of_the_upstream_gradient_and_the_angle_are_the_callers(cuda):
    fp = _fp()
    r64, r32, alt, _ = _restated('batch3')
    tv, tf = _dev(cuda, *nr.fixture('batch3'))
    pen = fp.FoldPenalty(tf, 30.)
    for up in ((1., 0.), (0., 1.), (0.5, -2.)):
        grad = foldpen_guarded.both(pen, tv, up)[2].cpu().numpy()
        want = up[0] * r64['grad'][0] + up[1] * r64['grad'][1]
        bound = np.maximum(4 * np.abs(sum(u * (r32['grad'][k] - r64['grad'][k]) for k, u in enumerate(up))).max((1, 2)),
                           np.abs(sum(u * (r32['grad'][k] - alt['grad'][k]) for k, u in enumerate(up))).max((1, 2)))
        _held('batch3', 'gradient under upstream %s' % (up,), grad, bound, want)
    wide = _restated('batch3', 90.)                                               # every fold of batch3 and 4 pairs more at 90 degrees
    loss, values, grad = (t.cpu().numpy() for t in foldpen_guarded.both(fp.FoldPenalty(tf, 90.), tv))
    assert min(c['angle'] for c in fr.conditions(*nr.fixture('batch3'), 90.)) > 0.25
    assert ((values != 0) == wide[0]['active']).all()
    _held('batch3 at 90 degrees', 'values', values, *_bounds(*wide[:3], 'values'))
    _held('batch3 at 90 degrees', 'gradient', grad, *_bounds(*wide[:3], 'grad'))
    half = foldpen_guarded.both(pen, tv.double())                                  # any floating type of the vertices
    assert half[2].dtype == torch.float64 and torch.equal(half[0], foldpen_guarded.both(pen, tv)[0])


def test_two_runs_give_the_same_bits(cuda):
    fp = _fp()
    for name in ('batch3', 'tile257'):
        tv, tf = _dev(cuda, *nr.fixture(name))
        a = foldpen_guarded.both(fp.FoldPenalty(tf, 30.), tv)
        b = foldpen_guarded.both(fp.FoldPenalty(tf, 30.), tv)
        for x, y in zip(a, b):
            assert torch.equal(x, y)
    no_grad = fp.FoldPenalty(tf, 30.)(tv)                                          # without a gradient wanted: no rows, the same loss
    assert not no_grad.requires_grad and torch.equal(no_grad, a[0])


def test_copies_across_many_blocks_give_eight_times_the_base(cuda):
    """Eight exact translates of creaseB on the 2^-16 grid: 2560 faces, 15 120 entries in 60 blocks, 8 x 162 vertices in 6; every
    difference of two vertices of a copy is the base's, so every entry and every vertex gradient has the base's bits."""
    fp = _fp()
    v0, f0 = nr.copies_base()
    verts, faces, _ = nr.copies_case(8)
    base = foldpen_guarded.both(fp.FoldPenalty(_dev(cuda, f0)[0], 30.), _dev(cuda, v0)[0])
    whole = foldpen_guarded.both(fp.FoldPenalty(_dev(cuda, faces)[0], 30.), _dev(cuda, verts)[0])
    print('copies: loss %s, base %s' % (whole[0].tolist(), base[0].tolist()))
    assert whole[1].shape == (1, 8 * 1890) and bool((whole[1].view(8, -1) == base[1]).all()) and int((base[1] != 0).sum()) == 5
    assert bool((whole[2].view(8, 162, 3) == base[2]).all()) and float(base[2].abs().max()) > 1
    want = 8 * base[0].double()
    assert bool(((whole[0].double() - want).abs() <= 2 * U24 * want).all()) and float(want.min()) > 0.1
    r64 = fr.penalty(v0, f0, 30.)
    assert ((base[1].cpu().numpy() != 0) == r64['active']).all()


def test_one_face_alone_and_a_list_with_keys_that_name_no_face(cuda):
    fp = _fp()
    tv, tf = _dev(cuda, *nr.fixture('batch3'))
    one = fp.FoldPenalty(torch.tensor([[0, 1, 2]], dtype=torch.int32, device=cuda), 30.)
    loss, values, grad = foldpen_guarded.both(one, tv[:, :3].clone())
    assert one.keys.numel() == 0 and loss.shape == (3, 2) and values.shape == (3, 0) and grad.shape == (3, 3, 3)
    assert not loss.any() and not grad.any()
    # a charged edge pair named with a face past the end, a charged vertex pair with a corner code of 3: both are skipped
    r64, r32, alt, top = _restated('batch3')
    e_at = int(np.nonzero(r64['active'][2] & (top['kind'] == nr.EDGE))[0][0])
    v_at = int(np.nonzero(r64['active'][2] & (top['kind'] == nr.VERTEX))[0][0])
    pen = fp.FoldPenalty(tf, 30.)
    bad = fp.FoldPenalty(tf, 30., keys=foldpen_guarded.bad_keys(pen.keys, tf.shape[0], e_at, v_at))
    full, cut = foldpen_guarded.both(pen, tv), foldpen_guarded.both(bad, tv)
    keep = torch.ones(top['n_list'], dtype=torch.bool, device=cuda)
    keep[[e_at, v_at]] = False
    assert bool((cut[1][:, keep] == full[1][:, keep]).all()) and not cut[1][:, ~keep].any() and bool((full[1][2, ~keep] > 0).all())
    want = r64['grad'].sum(0)
    for e in (e_at, v_at):
        for s, v in enumerate(r64['slots'][e]):
            if v >= 0:
                want[:, v] -= r64['rows'][:, e, s]
    gb, _ = _bounds(r64, r32, alt, 'grad')
    _held('batch3 without entries %d and %d' % (e_at, v_at), 'gradient', cut[2].cpu().numpy(), gb, want)
    lost = full[1][:, ~keep].double().sum(1)
    assert float(lost[2]) > 0.05 and bool(((full[0].sum(1).double() - cut[0].sum(1).double() - lost).abs() <= 4 * U24 * full[0].sum(1)).all())
    with pytest.raises(ValueError, match='keys must be int64'):
        fp.FoldPenalty(tf, 30., keys=pen.keys.int())
    with pytest.raises(ValueError, match=r'verts must be floating point \[N,V,3\]'):
        pen(tv[0])


def test_a_captured_graph_replays_to_the_bits_of_eager(cuda):
    fp = _fp()
    verts, faces = nr.fixture('batch3')
    tv, tf = _dev(cuda, verts, faces)
    pen = fp.FoldPenalty(tf, 30., n_verts=verts.shape[1])
    up = torch.tensor([[1., 0.5]], device=cuda)
    eager = [foldpen_guarded.both(pen, v, (1., 0.5)) for v in (tv, tv.flip(0))]
    x = tv.clone().requires_grad_(True)
    side = torch.cuda.Stream(device=cuda)
    side.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(side):                                                 # warm-up on the capture stream
        for _ in range(2):
            torch.autograd.grad((pen(x) * up).sum(), x)
    torch.cuda.current_stream(cuda).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        loss = pen(x)
        (grad,) = torch.autograd.grad((loss * up).sum(), x)
    for v, want in ((tv, eager[0]), (tv.flip(0), eager[1]), (tv, eager[0])):
        with torch.no_grad():
            x.copy_(v)
        loss.detach().zero_()
        grad.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(loss.detach(), want[0]) and torch.equal(grad, want[2]) and float(grad.abs().max()) > 1


def test_descent_on_the_device_clears_the_report(cuda):
    """The schedule of tests/test_foldpen_cpu.py (DESCENT) with the device's gradient: the counts are those of
    scripts/shape_neighbours.py at 20 degrees.  The restatement needs 36 steps in float32 and in float64."""
    fp, sn = _fp(), meshnbr_guarded.shape_neighbours()
    tv, tf = _dev(cuda, *nr.fixture('batch3'))
    pen = fp.FoldPenalty(tf, DESCENT['fold_deg'])
    nbr = sn.neighbour_list(tf)
    x, done = tv.clone(), None
    for step in range(1, DESCENT['steps'] + 1):
        grad = foldpen_guarded.both(pen, x, DESCENT['weights'])[2]
        x = (x.double() - DESCENT['rate'] * grad.double()).float()
        res = sn.neighbour_tests(x, tf, DESCENT['count_deg'], nbr=nbr)
        if int(res['n_creased'].sum()) + int(res['n_pierced'].sum()) == 0:
            done = step
            break
    print('device: all counts 0 after %s steps (cap %d); restatement: 36 in float64, 36 in float32' % (done, DESCENT['steps']))
    assert done is not None and done <= DESCENT['steps'] and torch.equal(x[0], tv[0])
    left, values = pen.entries(x)                                                  # released at 20 degrees; what is left lies below 30:
    print('the penalty that is left: %s' % left.tolist())                         # no pair is charged more than (30 - 20 degrees)^2
    assert not left[:, 1].any() and float(values.max()) <= np.radians(10.) ** 2 + 1e-6


# ---- guard bands and relocated inputs -------------------------------------------------------------------------------------------------
def _modules():
    return [_fp(), meshnbr_guarded.shape_neighbours()] + guarded._product_modules()


def test_the_natives_with_guard_bands_and_poison(cuda):
    guarded.run_case(foldpen_guarded.CASE, cuda, modules=_modules())


def test_the_natives_with_relocated_inputs(cuda):
    record = guarded.run_relocated(foldpen_guarded.CASE, cuda, modules=_modules())
    assert sorted(record) == sorted(foldpen_guarded.NATIVES)


# ---- through LASR.forward -----------------------------------------------------------------------------------------------------------
def _fold_the_rest_shape(m):
    """The displacement of meshnbr_restated.crease (s = 2, h = -0.05 of the radius) on the rest shape of every hypothesis."""
    f = m.faces.cpu().numpy()
    with torch.no_grad():
        for h in range(m.mean_v.shape[0]):
            v = m.mean_v[h].detach().cpu().numpy().astype(np.float64)
            k = int(np.argmax(v[:, 0]))
            ring = np.array(sorted(set(f[(f == k).any(1)].reshape(-1).tolist()) - {k}))
            c = v[ring].mean(0)
            v[k] = c + 2. * (v[ring[0]] - c) - 0.05 * c
            m.mean_v[h].copy_(torch.from_numpy(v.astype(np.float32)))


def test_through_the_model_the_terms_are_appended_and_every_earlier_total_keeps_its_bits(tmp_path, cuda, monkeypatch):
    """Two forwards of the model differ in their last bits (the encoder's convolutions), so the flag-off numbers are formed from the
    very tensors of the flag-on forward: the call of fused_ops.weighted_mean_sum is recorded and made again without its last two
    terms and with 10 groups, which is the flag-off call.  N = 2 B H = 8 posed meshes.  total = (total_off + w mean(crease)) +
    w mean(pierce) in float32: per term 7 additions, a division and a multiplication, then one addition to the total: 2 x 9
    roundings of at most 2^-24 of a term and 2 of at most 2^-24 of the total, 20 in all."""
    from lasr_amd.nnutils import fused_ops
    from test_lasr_forward_gpu import make_trainer
    tr = make_trainer(tmp_path, symmetric=False, only_mean_sym=False)
    tr.model.train()
    tr.reinit_bones()
    m = tr.module
    _fold_the_rest_shape(m)
    batch = tr.set_input(tr.dataloader[0])
    calls, real = [], fused_ops.weighted_mean_sum

    def recording(terms, n_groups=None):
        calls.append((list(terms), n_groups))
        return real(terms, n_groups)
    monkeypatch.setattr(fused_ops, 'weighted_mean_sum', recording)

    def run():
        torch.manual_seed(7)
        tr.model.zero_grad(set_to_none=True)
        del calls[:]
        loss, aux = tr.model(batch)
        return loss, aux
    assert m.fold_loss is None
    loss_off, aux_off = run()
    (terms_off, groups_off), = calls
    assert 'fold_loss' not in aux_off and groups_off == 10 and not hasattr(m, 'fold_loss_value')
    grad_plain, = torch.autograd.grad(loss_off, m.mean_v)
    w = 0.1
    tr.opts.fold_wt = tr.opts.pierce_wt = w
    m.fold_loss = _fp().FoldPenalty(m.faces, 30., n_verts=m.mean_v.shape[-2])
    loss_on, aux_on = run()
    (terms_on, groups_on), = calls
    assert groups_on == 11 and len(terms_on) == len(terms_off) + 2
    assert [(t[1], t[2]) for t in terms_on[:-2]] == [(t[1], t[2]) for t in terms_off] and [(t[1], t[2]) for t in terms_on[-2:]] == [(w, 10)] * 2
    total_off, sums_off = real(terms_on[:-2], 10)                                 # the flag-off call on the same tensors
    total_on, sums_on = real(terms_on, 11)
    assert torch.equal(total_on, loss_on.detach()) and torch.equal(sums_on[:10], sums_off)               # every earlier group keeps its bits
    for name, g in (('mask_loss', 0), ('flow_rd_loss', 1), ('texture_loss', 2), ('triangle_loss', 3), ('lmotion_loss', 5), ('arap_loss', 6),
                    ('cam_loss', 8)):
        assert torch.equal(getattr(m, name), sums_off[g]), name
    fold = torch.stack([terms_on[-2][0], terms_on[-1][0]], 1).detach().double()
    assert torch.equal(fold.float(), m.fold_loss(m.deform_v.detach().reshape(-1, m.deform_v.shape[-2], 3)))
    N, w32 = fold.shape[0], float(np.float32(w))
    means = [w32 * float(fold[:, k].mean()) for k in (0, 1)]
    off_value, on_value = float(total_off.detach()), float(total_on.detach())
    want = off_value + means[0] + means[1]
    bound = U24 * ((N + 1) * (means[0] + means[1]) + 2 * max(abs(want), abs(off_value)))
    print('flag off %.8f, on %.8f, the two weighted means %.3e + %.3e, off the sum by %.2e (bound %.2e: %d roundings); N = %d; fold %s'
          % (off_value, on_value, means[0], means[1], abs(on_value - want), bound, 2 * (N + 1) + 2, N, fold.sum(0).tolist()))
    assert N == 8 and float(aux_on['fold_loss']) > 0 and means[0] > 0 and torch.equal(aux_on['fold_loss'], m.fold_loss_value)
    assert torch.equal(aux_on['fold_loss'], sums_on[10])
    assert abs(float(sums_on[10]) - (means[0] + means[1])) <= U24 * (N + 2) * (means[0] + means[1])
    assert abs(on_value - want) <= bound
    # the parameter gradients: those of the flag-off total of the same graph, plus what the two terms add
    grad_on, grad_off = (torch.autograd.grad(t, m.mean_v, retain_graph=True)[0] for t in (loss_on, total_off))
    diff = float((grad_on - grad_off).abs().max())
    print('largest gradient by mean_v: %.3e with the terms, %.3e without, they differ by up to %.3e' % (
        float(grad_on.abs().max()), float(grad_off.abs().max()), diff))
    assert torch.isfinite(grad_on).all() and diff > 0 and not torch.equal(grad_on, grad_plain)
