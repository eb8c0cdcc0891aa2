"""The intersection penalty of the optimiser on the device (scripts/isect_penalty.py, lasr_amd/csrc/isectpen.hip) against the
restatement (tests/isectpen_restated.py).  The penalty is this project's own addition: the restatement and closed forms are the only
parity there is.

Counts are compared for equality, with the restatement and with lasr_meshcheck_pairs on the same tensors:
tests/test_isectpen_cpu.py shows that on these fixtures the float32 and float64 restatements agree on which tests hold and which end
is the shallower.  Loss and gradient are held, per mesh, to 4 x max |float32 restatement - float64 restatement| with, as the floor,
the largest difference between two float32 restatements that differ in their order of operations (the unit normal by a reciprocal,
the foot's weights over |n| twice, l_a = 1 - (l_b + l_c)); both are taken on the accumulators before the last rounding, and the
rounding of the result to float32 (2^-24 of the largest magnitude) is added.  All of it comes from restatements only, nothing from
what the kernel gives.  A mesh without an intersecting pair has bound 0: its loss and gradient are exactly 0.  Every shape is a
fixture of the restatements: at most 5120 faces and 3 meshes.  Every comparison prints its figures before it asserts.

Measured on an MI355X:
  pinch2 (10 pairs): loss off the float64 restatement by 3.2e-7 (bound 9.9e-7), gradient by 6.4e-7 (bound 3.1e-6; the largest entry
    is 15.9); the bits of the float32 restatement.  tile257 (82 pairs): 2.6e-7 (7.7e-7), 8.6e-7 (4.0e-6).  two2 (0 / 83 / 94 pairs):
    loss 0 / 4.7e-8 / 1.5e-7 (0 / 7.5e-7 / 9.1e-7), gradient 0 / 8.6e-7 / 8.8e-7 (0 / 4.0e-6 / 3.2e-6).  batch3 (0 / 0 / 4): 5.8e-8
    (2.1e-7), 3.7e-7 (1.7e-6).  ico2: every output exactly 0.  tile257, two2 and batch3 do not have the bits of the float32
    restatement.
  eight copies: n_pairs 664 = 8 x 83, loss 51.727058 = 8 x 6.4658823, every copy's gradient block the base's bits.
  descent on the device: pinch2 clear after 6 steps at rate 0.003 and 2 at 0.01, batch3 after 4, n_pairs after every step as restated.
  through LASR.forward: total 0.98130232 without, 1.37195611 with the weight at 0.1, off the sum by 4.2e-8 (bound 1.6e-6).
"""
import functools

import numpy as np
import pytest
import torch

import guarded
import isectpen_guarded
import isectpen_restated as ir
import meshcheck_restated as mr
from test_isectpen_cpu import DESCENT, STEPS, fixture, restated

pytestmark = pytest.mark.gpu
U24 = 2. ** -24


def _ip():
    return isectpen_guarded.isect_penalty()


def _dev(cuda, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for a in arrays]


@functools.lru_cache(None)
def _bounds(name):
    """Per mesh, from the three restatements: (loss bound [N], gradient bound [N])."""
    a, b, c = restated(name), restated(name, np.float32), restated(name, np.float32, True)
    la, lb, lc = (r['acc_loss'] / ir.Q for r in (a, b, c))
    ga, gb, gc = (r['acc_grad'] / ir.Q for r in (a, b, c))
    loss = np.maximum(4 * np.abs(lb - la), np.abs(lb - lc)) + U24 * np.abs(la)
    grad = np.maximum(4 * np.abs(gb - ga).max((1, 2)), np.abs(gb - gc).max((1, 2))) + U24 * np.abs(ga).max((1, 2))
    return loss, grad


def _run(cuda, name):
    tv, tf = _dev(cuda, *fixture(name))
    return [t.cpu().numpy() for t in isectpen_guarded.both(_ip().IsectPenalty(tf, n_verts=tv.shape[1]), tv)]


@pytest.mark.parametrize('name', ['pinch2', 'tile257', 'two2', 'batch3', 'ico2'])
def test_fixture_is_held_to_the_restatement(cuda, name):
    from lasr_amd.nnutils import meshcheck
    loss, grad, n_pairs, n_dropped = _run(cuda, name)
    r64, r32 = restated(name), restated(name, np.float32)
    N = len(r64['loss'])
    assert loss.shape == (N,) and loss.dtype == np.float32 and grad.shape == r64['gunit'].shape and grad.dtype == np.float32
    assert n_pairs.dtype == np.int64 and n_pairs.tolist() == r64['n_pairs'].tolist() and not n_dropped.any()
    tv, tf = _dev(cuda, *fixture(name))
    assert torch.equal(meshcheck.self_intersections(tv, tf)[0].cpu(), torch.from_numpy(n_pairs))            # integer for integer
    lb, gb = _bounds(name)
    le = np.abs(loss.astype(np.float64) - r64['acc_loss'] / ir.Q)
    ge = np.abs(grad.astype(np.float64) - r64['acc_grad'] / ir.Q).max((1, 2))
    bits = bool((loss == r32['loss']).all() and (grad == r32['gunit']).all())
    print('%s: n_pairs %s, loss %s off the float64 restatement by %s (bound %s), gradient by %s (bound %s; largest entry %.3f); '
          'the bits of the float32 restatement: %s' % (name, n_pairs.tolist(), loss.tolist(), ['%.2e' % e for e in le], ['%.2e' % b for b in lb],
                                                       ['%.2e' % e for e in ge], ['%.2e' % b for b in gb], np.abs(grad).max(), bits))
    assert (le <= lb).all() and (ge <= gb).all()
    clean = r64['n_pairs'] == 0
    assert not loss[clean].any() and not grad[clean].any() and not lb[clean].any() and not gb[clean].any()  # exactly 0 where nothing is charged
    assert (loss[~clean] > 0.1).all() and (np.abs(grad[~clean]).max((1, 2)) > 1).all()
    if name == 'ico2':
        assert clean.all()
    if name == 'two2':
        assert clean.tolist() == [True, False, False]


def test_copies_across_many_tile_pairs_give_eight_times_the_base(cuda):
    """Eight exact translates of the overlapping frame of two2 on the 2^-16 grid: 5120 faces, 20 tiles, 210 tile pairs; every
    difference of two vertices of a copy is the base's, so every contribution has the base's bits and the integer sums are 8 x."""
    verts, faces, exp = mr.copies_case(8)
    base = _run(cuda, 'copies_base')
    tv, tf = _dev(cuda, verts, faces)
    whole = [t.cpu().numpy() for t in isectpen_guarded.both(_ip().IsectPenalty(tf), tv)]
    print('copies: loss %s, base %s, n_pairs %s' % (whole[0].tolist(), base[0].tolist(), whole[2].tolist()))
    assert whole[2].tolist() == [exp['n_pairs']] == [8 * int(base[2][0])] and base[2].tolist() == restated('copies_base')['n_pairs'].tolist()
    assert (whole[1].reshape(8, 324, 3) == base[1][0]).all() and np.abs(base[1]).max() > 1
    assert whole[0].tolist() == [8 * float(base[0][0])] and base[0][0] > 1 and not whole[3].any()


def test_two_runs_and_a_permutation_of_the_faces_give_the_same_bits(cuda):
    ip = _ip()
    for name in ('pinch2', 'two2'):
        tv, tf = _dev(cuda, *fixture(name))
        a = isectpen_guarded.both(ip.IsectPenalty(tf), tv)
        b = isectpen_guarded.both(ip.IsectPenalty(tf), tv)
        perm = torch.from_numpy(np.random.default_rng(5).permutation(tf.shape[0])).to(cuda)
        c = isectpen_guarded.both(ip.IsectPenalty(tf[perm].contiguous()), tv)
        for x, y, z in zip(a, b, c):
            assert torch.equal(x, y) and torch.equal(x, z)
        assert float(a[0].max()) > 1
    plain = ip.IsectPenalty(tf)(tv)                                                # no gradient wanted: gunit NULL, the same loss and counts
    assert not plain.requires_grad and torch.equal(plain, a[0])
    n_pairs, n_dropped = ip.IsectPenalty(tf).counts(tv)
    assert torch.equal(n_pairs, a[2]) and torch.equal(n_dropped, a[3]) and n_pairs.tolist() == [0, 83, 94]
    with_grad = ip.IsectPenalty(tf).launch(tv, True)                               # and the counts of the call with a gradient
    assert torch.equal(with_grad[2], n_pairs) and torch.equal(with_grad[3], n_dropped) and torch.equal(with_grad[0], plain)
    half = isectpen_guarded.both(ip.IsectPenalty(tf), tv.double())                 # any floating type of the vertices
    assert half[1].dtype == torch.float64 and torch.equal(half[0], a[0]) and torch.equal(half[1].float(), a[1])
    with pytest.raises(ValueError, match=r'verts must be floating point \[N,V,3\]'):
        ip.IsectPenalty(tf)(tv[0])
    with pytest.raises(ValueError, match='built for meshes of 7 vertices'):
        ip.IsectPenalty(tf, n_verts=7)(tv)
    with pytest.raises(ValueError, match=r'faces must be integers \[F,3\]'):
        ip.IsectPenalty(tf.float())
    empty = ip.IsectPenalty(tf[:0])
    assert not isectpen_guarded.both(empty, tv)[1].any() and empty.counts(tv)[0].tolist() == [0, 0, 0]


@pytest.mark.parametrize('how', ['outside', 'negative', 'repeated'])
def test_a_face_that_names_no_vertex_or_one_twice_equals_the_mesh_without_it(cuda, how):
    ip = _ip()
    verts, faces = fixture('pinch2')
    frame = restated('pinch2')['frames'][0]
    at = int(frame['pairs'][frame['hit']][0, 1])                                   # a face of an intersecting pair: leaving it out shows
    bad = faces.copy()
    bad[at, 1] = {'outside': verts.shape[1], 'negative': -1, 'repeated': bad[at, 0]}[how]
    tv, tb, tw = _dev(cuda, verts, bad, np.delete(faces, at, 0))
    got, want, full = (isectpen_guarded.both(ip.IsectPenalty(f), tv) for f in (tb, tw, _dev(cuda, faces)[0]))
    for x, y in zip(got, want):
        assert torch.equal(x, y)
    assert int(full[2]) > int(got[2]) > 0 and float(full[0]) > float(got[0]) > 0


def test_a_captured_graph_replays_to_the_bits_of_eager(cuda):
    ip = _ip()
    verts, faces = fixture('two2')
    tv, tf = _dev(cuda, verts, faces)
    pen = ip.IsectPenalty(tf, n_verts=verts.shape[1])
    up = torch.tensor([1., 0.5, -2.], device=cuda)
    eager = [isectpen_guarded.both(pen, v, (1., 0.5, -2.)) for v in (tv, tv.flip(0))]
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
        assert torch.equal(loss.detach(), want[0]) and torch.equal(grad, want[1]) and float(grad.abs().max()) > 1


@pytest.mark.parametrize('name, rate', sorted(DESCENT))
def test_descent_on_the_device_takes_the_restatements_steps(cuda, name, rate):
    """The schedule of tests/test_isectpen_cpu.py (DESCENT) with the device's gradient and the device's count."""
    tv, tf = _dev(cuda, *fixture(name))
    pen = _ip().IsectPenalty(tf, n_verts=tv.shape[1])
    mesh = int(np.argmax(restated(name)['n_pairs']))
    x, done, history = tv.clone(), None, []
    for step in range(1, STEPS + 1):
        grad = isectpen_guarded.both(pen, x)[1]
        x = (x.double() - rate * grad.double()).float()
        n_pairs = pen.counts(x)[0].cpu()
        history.append(int(n_pairs[mesh]))
        if not n_pairs.any():
            done = step
            break
    print('device: %s at rate %g clear after %s steps, n_pairs %s; restatement: %s' % (name, rate, done, history, DESCENT[(name, rate)]))
    assert (done, history) == DESCENT[(name, rate)]
    assert not float(pen(x).abs().max()) and all(torch.equal(x[t], tv[t]) for t in range(len(tv)) if t != mesh)


# ---- guard bands and relocated inputs -------------------------------------------------------------------------------------------------
def _modules():
    return [_ip()] + guarded._product_modules()


def test_the_native_with_guard_bands_and_poison(cuda):
    guarded.run_case(isectpen_guarded.CASE, cuda, modules=_modules())


def test_the_native_with_relocated_inputs(cuda):
    record = guarded.run_relocated(isectpen_guarded.CASE, cuda, modules=_modules())
    assert sorted(record) == sorted(isectpen_guarded.NATIVES)


# ---- through LASR.forward -----------------------------------------------------------------------------------------------------------
def _pinch_the_rest_shape(m):
    """The displacement of meshcheck_restated.pinch2 on the rest shape of every hypothesis: the topmost vertex through the opposite
    side, seen from the centre of the shape."""
    with torch.no_grad():
        for h in range(m.mean_v.shape[0]):
            v = m.mean_v[h].detach().cpu().numpy().astype(np.float64)
            c = v.mean(0)
            k = int(np.argmax(v[:, 2]))
            v[k] = c - 1.3 * (v[k] - c) + np.array([0.013, -0.021, 0.]) * np.abs(v - c).max()
            m.mean_v[h].copy_(torch.from_numpy(v.astype(np.float32)))


def test_through_the_model_the_term_is_appended_and_every_earlier_total_keeps_its_bits(tmp_path, cuda, monkeypatch):
    """The set-up of tests/test_foldpen_gpu.py: two forwards of the model differ in their last bits, so the flag-off numbers are
    formed from the very tensors of the flag-on forward: the recorded call of fused_ops.weighted_mean_sum is made again without
    its last term and with 10 groups, which is the flag-off call.  N = 2 B H = 8 posed meshes.  total = total_off + w mean(isect) in
    float32 is held to 20 roundings of 2^-24 of the largest of the three magnitudes."""
    from lasr_amd.nnutils import fused_ops
    from test_lasr_forward_gpu import make_trainer
    tr = make_trainer(tmp_path, symmetric=False, only_mean_sym=False)
    tr.model.train()
    tr.reinit_bones()
    m = tr.module
    _pinch_the_rest_shape(m)
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
    assert m.isect_loss is None and m.fold_loss is None
    loss_off, aux_off = run()
    (terms_off, groups_off), = calls
    assert 'isect_loss' not in aux_off and groups_off == 10 and not hasattr(m, 'isect_loss_value')
    w = 0.1
    tr.opts.isect_wt = w
    m.isect_loss = _ip().IsectPenalty(m.faces, n_verts=m.mean_v.shape[-2])
    loss_on, aux_on = run()
    (terms_on, groups_on), = calls
    assert groups_on == 11 and len(terms_on) == len(terms_off) + 1
    assert [(t[1], t[2]) for t in terms_on[:-1]] == [(t[1], t[2]) for t in terms_off] and (terms_on[-1][1], terms_on[-1][2]) == (w, 10)
    total_off, sums_off = real(terms_on[:-1], 10)                                  # the flag-off call on the same tensors
    total_on, sums_on = real(terms_on, 11)
    assert torch.equal(total_on, loss_on.detach()) and torch.equal(sums_on[:10], sums_off)               # every earlier group keeps its bits
    for name, g in (('mask_loss', 0), ('flow_rd_loss', 1), ('texture_loss', 2), ('triangle_loss', 3), ('lmotion_loss', 5), ('arap_loss', 6),
                    ('cam_loss', 8)):
        assert torch.equal(getattr(m, name), sums_off[g]), name
    isect = terms_on[-1][0].detach().double()
    posed = m.deform_v.detach().reshape(-1, m.deform_v.shape[-2], 3)
    assert torch.equal(isect.float(), m.isect_loss(posed)) and isect.shape == (8,)
    term = float(np.float32(w)) * float(isect.mean())
    off_value, on_value = float(total_off.detach()), float(total_on.detach())
    want = off_value + term
    bound = 20 * U24 * max(abs(want), abs(off_value), term)
    print('flag off %.8f, on %.8f, the weighted mean %.3e, off the sum by %.2e (bound %.2e: 20 roundings); isect %s, n_pairs %s'
          % (off_value, on_value, term, abs(on_value - want), bound, isect.tolist(), m.isect_loss.counts(posed)[0].tolist()))
    assert term > 0 and torch.equal(aux_on['isect_loss'], m.isect_loss_value) and torch.equal(aux_on['isect_loss'], sums_on[10])
    assert abs(float(sums_on[10]) - term) <= 10 * U24 * term and abs(on_value - want) <= bound
    grad_on, grad_off = (torch.autograd.grad(t, m.mean_v, retain_graph=True)[0] for t in (loss_on, total_off))
    assert torch.isfinite(grad_on).all() and float((grad_on - grad_off).abs().max()) > 0
    # with the fold penalty on as well: 12 groups, the fold terms in group 10, this term in group 11, last
    import foldpen_guarded
    tr.opts.fold_wt = tr.opts.pierce_wt = w
    m.fold_loss = foldpen_guarded.fold_penalty().FoldPenalty(m.faces, 30., n_verts=m.mean_v.shape[-2])
    _, aux_both = run()
    (terms_both, groups_both), = calls
    assert groups_both == 12 and len(terms_both) == len(terms_off) + 3
    assert [(t[1], t[2]) for t in terms_both[:-3]] == [(t[1], t[2]) for t in terms_off]
    assert [(t[1], t[2]) for t in terms_both[-3:]] == [(w, 10), (w, 10), (w, 11)]
    _, sums_both = real(terms_both, 12)
    assert torch.equal(aux_both['fold_loss'], sums_both[10]) and torch.equal(aux_both['isect_loss'], sums_both[11])
    assert torch.equal(real(terms_both[:-3], 10)[1], sums_both[:10]) and float(aux_both['isect_loss']) > 0
