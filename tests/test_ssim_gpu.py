"""The SSIM kernels (lasr_amd/csrc/ssim.hip) on the GPU against the restatement (tests/ssim_restated.py, the definition), closed
forms, determinism and graph capture, the multi-scale module against the torch composition, and the term inside LASR.forward.

Bars: value and gradient against the float64 restatement within 4 x max |float32 restatement - float64 restatement| (at least one
float32 ulp of the largest magnitude), computed from the restatement alone (ssim_cases.bounds).  Nothing is left out of a
comparison.  Every figure is printed before it is asserted."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import optimize                                                    # noqa: E402
import ssim_cases                                                  # noqa: E402
import ssim_restated as sr                                         # noqa: E402
from lasr_amd import _lib                                          # noqa: E402
from lasr_amd.nnutils import fused_ops, mesh_net, train_utils      # noqa: E402

CASES = ssim_cases.cases(_lib.SSIM_TILE_W, _lib.SSIM_TILE_H)
BIG = (2, 3, 64, 80, 1.)


def run(case, cuda, save_planes=None, gd=None):
    ref = ssim_cases.reference(case)
    M, rep, H, W, L = case
    a = torch.tensor(ref['a']).to(cuda)
    b = torch.tensor(ref['b']).to(cuda).requires_grad_(True)
    d = fused_ops.ssim_distance(a, b, rep, L, save_planes=save_planes)
    d.backward(torch.tensor(ref['gd'] if gd is None else gd).to(cuda))
    return d.detach().cpu().numpy(), b.grad.cpu().numpy()


# ---- 1. value and gradient against the restatement -----------------------------------------------------------------------------
@pytest.mark.parametrize('case', CASES, ids=lambda c: 'M%d-rep%d-%dx%d-L%g' % c)
def test_value_and_gradient_match_the_restatement(case, cuda, capsys):
    ref = ssim_cases.reference(case)
    bv, bg = ssim_cases.bounds(ref)
    d, g = run(case, cuda)
    assert d.dtype == np.float32 and d.shape == ref['d64'].shape and g.shape == ref['g64'].shape
    ev, eg = np.abs(d.astype(np.float64) - ref['d64']).max(), np.abs(g.astype(np.float64) - ref['g64']).max()
    same = bool(np.array_equal(d, ref['d32']) and np.array_equal(g, ref['g32']))
    rv = np.abs(d.astype(np.float64) - ref['d32']).max() / max(np.abs(ref['d32'].astype(np.float64) - ref['d64']).max(), 1e-300)
    rg = np.abs(g.astype(np.float64) - ref['g32']).max() / max(np.abs(ref['g32'].astype(np.float64) - ref['g64']).max(), 1e-300)
    with capsys.disabled():
        print('\nssim %s: value err %.3e (bar %.3e), gradient err %.3e (bar %.3e); distance to the float32 restatement / its '
              'spread: value %.3g, gradient %.3g; bit-identical to it: %s' % (case, ev, bv, eg, bg, rv, rg, same))
    assert np.isfinite(d).all() and np.isfinite(g).all()
    assert ev <= bv and eg <= bg, (case, ev, bv, eg, bg)


@pytest.mark.parametrize('case', [(1, 1, 11, 11, 1.), (2, 3, 43, 33, 2.), BIG], ids=str)
def test_saved_planes_and_recomputed_moments_give_the_same_bits(case, cuda):
    d0, g0 = run(case, cuda, save_planes=False)
    d1, g1 = run(case, cuda, save_planes=True)
    assert np.array_equal(d0, d1) and np.array_equal(g0, g1)


# ---- 2. closed forms -----------------------------------------------------------------------------------------------------------
def test_distance_of_an_image_to_itself_is_exactly_zero(cuda):
    for case in [(1, 1, 11, 11, 1.), (2, 1, 43, 33, 2.), (2, 1, 64, 80, 1.)]:
        a = torch.tensor(ssim_cases.reference(case)['a']).to(cuda)
        d = fused_ops.ssim_distance(a, a.clone(), 1, case[4])
        assert d.shape == (case[0],) and bool((d == 0).all()), d
        d3 = fused_ops.ssim_distance(a, a.repeat_interleave(3, 0), 3, case[4])
        assert bool((d3 == 0).all())


@pytest.mark.parametrize('L', [1., 2.])
def test_constant_images_give_the_closed_form(cuda, L, capsys):
    c1, c2 = float(np.float32(0.3)), 0.75                         # the values the float32 images hold
    a, b = np.full((1, 3, 43, 57), c1, np.float32), np.full((2, 3, 43, 57), c2, np.float32)
    C1 = (0.01 * L) ** 2
    want = 1. - (2. * c1 * c2 + C1) / (c1 * c1 + c2 * c2 + C1)
    d32, d64 = sr.distance(a, b, 2, L, np.float32), sr.distance(a, b, 2, L, np.float64)
    bar = max(4. * np.abs(d32.astype(np.float64) - d64).max(), float(np.finfo(np.float32).eps) * abs(want))
    d = fused_ops.ssim_distance(torch.from_numpy(a).to(cuda), torch.from_numpy(b).to(cuda), 2, L).cpu().numpy()
    with capsys.disabled():
        print('\nssim constants L=%g: kernel %r, closed form %.9g, float64 restatement %r, bar %.3e' % (L, d, want, d64, bar))
    assert np.abs(d64 - want).max() <= 1e-12
    assert np.abs(d.astype(np.float64) - want).max() <= bar


def test_repeat_equals_separate_calls_on_repeated_observations(cuda):
    case = (2, 3, 43, 33, 1.)
    ref = ssim_cases.reference(case)
    a, b = torch.tensor(ref['a']).to(cuda), torch.tensor(ref['b']).to(cuda)
    gd = torch.tensor(ref['gd']).to(cuda)
    b3 = b.clone().requires_grad_(True)
    d3 = fused_ops.ssim_distance(a, b3, 3, 1.)
    d3.backward(gd)
    for r in range(3):                                             # hypothesis r of every observation, one call with rep = 1
        br = b[r::3].clone().requires_grad_(True)
        dr = fused_ops.ssim_distance(a, br, 1, 1.)
        dr.backward(gd[r::3].contiguous())
        assert torch.equal(dr, d3[r::3]) and torch.equal(br.grad, b3.grad[r::3])
    ar = a.repeat_interleave(3, 0)                                 # and the observations repeated in memory
    b1 = b.clone().requires_grad_(True)
    d1 = fused_ops.ssim_distance(ar, b1, 1, 1.)
    d1.backward(gd)
    assert torch.equal(d1, d3.detach()) and torch.equal(b1.grad, b3.grad)


# ---- 3. determinism and capture ------------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bits_and_a_captured_graph_replays_them(cuda):
    ref = ssim_cases.reference(BIG)
    M, rep, H, W, L = BIG
    d0, g0 = run(BIG, cuda)
    d1, g1 = run(BIG, cuda)
    assert np.array_equal(d0, d1) and np.array_equal(g0, g1)
    a = torch.tensor(ref['a']).to(cuda)
    b = torch.tensor(ref['b']).to(cuda).requires_grad_(True)
    gd = torch.tensor(ref['gd']).to(cuda)
    side = torch.cuda.Stream(device=cuda)
    side.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(side):                                  # warm-up on the capture stream
        for _ in range(2):
            (gw,) = torch.autograd.grad(fused_ops.ssim_distance(a, b, rep, L), b, gd)
    torch.cuda.current_stream(cuda).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        d_out = fused_ops.ssim_distance(a, b, rep, L)
        (g_out,) = torch.autograd.grad(d_out, b, gd)
    for _ in range(2):
        d_out.detach().zero_()
        g_out.zero_()
        graph.replay()
        torch.cuda.synchronize(cuda)
        assert np.array_equal(d_out.detach().cpu().numpy(), d0) and np.array_equal(g_out.cpu().numpy(), g0)


# ---- 4. the multi-scale module -------------------------------------------------------------------------------------------------
def test_structural_distance_kernel_equals_the_torch_composition(cuda, capsys):
    ref = ssim_cases.reference(BIG)
    M, rep, H, W, L = BIG
    a = torch.tensor(ref['a']).to(cuda)
    bar = 0.
    for xa, xb in zip(sr.pyramid(ref['a'], 3), sr.pyramid(ref['b'], 3)):            # the per-scale bar of check 1, the largest
        d32, d64 = sr.distance(xa, xb, rep, L, np.float32), sr.distance(xa, xb, rep, L, np.float64)
        bar = max(bar, 4. * np.abs(d32.astype(np.float64) - d64).max(), float(np.finfo(np.float32).eps) * np.abs(d64).max())
    out = []
    for use_kernel in (True, False):
        net = mesh_net.StructuralDistance(scales=3, use_kernel=use_kernel).to(cuda)
        b = torch.tensor(ref['b']).to(cuda).requires_grad_(True)
        d = net.forward_pair(a, b, repeat=rep, unit_range=True)
        d.backward(torch.tensor(ref['gd']).to(cuda))
        assert d.shape == (M * rep,) and torch.isfinite(b.grad).all() and float(b.grad.abs().max()) > 0
        out.append((d.detach().cpu().numpy().astype(np.float64), b.grad.cpu().numpy().astype(np.float64)))
    ev = np.abs(out[0][0] - out[1][0]).max()
    want = sr.multiscale_distance(ref['a'], ref['b'], rep, L, 3, np.float64)
    with capsys.disabled():
        print('\nssim three scales: kernel against torch composition %.3e (bar %.3e); kernel against the float64 restatement %.3e, '
              'torch composition against it %.3e; gradients differ by %.3e of the largest entry'
              % (ev, bar, np.abs(out[0][0] - want).max(), np.abs(out[1][0] - want).max(),
                 np.abs(out[0][1] - out[1][1]).max() / np.abs(out[1][1]).max()))
    assert ev <= bar


# ---- 5. in the model -----------------------------------------------------------------------------------------------------------
def make(tmp_path, cuda, *extra, graph=False):
    """The trainer of tests/test_step_tail_gpu.py with the texture term switched on.  That test never runs LASR.forward; with its
    flags alone the forward stops before it reaches the texture term, because the ground-truth-pose path (--use_gtpose, the
    default) does not take two hypotheses (project_points refuses its focal lengths).  --nouse_gtpose, which every forward test of
    tests/test_lasr_forward_gpu.py passes, is therefore added; sizes and everything else stay."""
    flags = ['--name', 't', '--checkpoint_dir', str(tmp_path), '--img_size', '64', '--subdivide', '1', '--n_bones', '3',
             '--n_hypo', '2', '--batch_size', '1', '--opt_tex', 'yes', '--iters_per_epoch', '4', '--nouse_gtpose',
             '--use_graph' if graph else '--nouse_graph', '--dataname', 'synthetic'] + list(extra)
    opts = optimize.parse_flags(flags)
    opts.local_rank = cuda.index or 0
    torch.manual_seed(0)
    return train_utils.LASRTrainer(opts).init_training()


def one_forward(tr):
    tr.model.train()
    tr.reinit_bones()
    loss, _ = tr.model(tr.set_input(tr.dataloader[0]))
    return loss


def test_term_inside_the_model(tmp_path, cuda, capsys):
    tr = make(tmp_path / 'a', cuda, '--ptex_method', 'ssim')
    m = tr.module
    assert type(m.ptex_loss) is mesh_net.StructuralDistance and m.ptex_loss.scales == 3 and m.ptex_loss.use_kernel
    seen = []
    inner = m.ptex_loss.forward_pair

    def recording(a, b, repeat=1, unit_range=False):
        out = inner(a, b, repeat=repeat, unit_range=unit_range)
        seen.append((a.detach().cpu().numpy(), b.detach().cpu().numpy(), repeat, unit_range, out.detach().cpu().numpy()))
        return out
    m.ptex_loss.forward_pair = recording
    loss = one_forward(tr)
    assert len(seen) == 1 and torch.isfinite(loss)
    a, b, rep, unit, out = seen[0]
    assert unit is True and rep == 2 and a.shape[1:] == (3, 64, 64) and b.shape[0] == a.shape[0] * rep and out.shape == (b.shape[0],)
    want = sr.multiscale_distance(a, b, rep, 1., 3, np.float64)
    bar = 0.
    for xa, xb in zip(sr.pyramid(a, 3), sr.pyramid(b, 3)):
        d32, d64 = sr.distance(xa, xb, rep, 1., np.float32), sr.distance(xa, xb, rep, 1., np.float64)
        bar = max(bar, 4. * np.abs(d32.astype(np.float64) - d64).max(), float(np.finfo(np.float32).eps) * np.abs(d64).max())
    err = np.abs(out.astype(np.float64) - want).max()
    with capsys.disabled():
        print('\nssim in LASR.forward: distances %s, err %.3e against the restatement (bar %.3e)' % (out, err, bar))
    assert err <= bar
    loss.backward()
    g_ssim = m.tex.grad.detach().clone()
    assert torch.isfinite(g_ssim).all() and float(g_ssim.abs().max()) > 0
    tr0 = make(tmp_path / 'b', cuda, '--ptex_method', 'ssim', '--noperceptual')
    assert tr0.module.ptex_loss is None
    loss0 = one_forward(tr0)
    loss0.backward()
    g_none = tr0.module.tex.grad
    assert float(loss0.detach()) != float(loss.detach()) and float((g_ssim - g_none).abs().max()) > 1e-3 * float(g_none.abs().max())


def test_graph_replay_matches_the_eager_step(tmp_path, cuda):
    tr = make(tmp_path, cuda, '--ptex_method', 'ssim', graph=True)
    tr.model.train()
    tr.reinit_bones()
    m = tr.module
    try:
        for i in range(3):                                         # iteration 0 eager (part render), then capture + replay
            m.iters = i
            tr.train_step(tr.set_input(tr.dataloader[i]))
        assert hasattr(tr, '_graphs') and len(tr._graphs) == 1
        m.iters = 3
        batch = tr.set_input(tr.dataloader[3])
        eager_loss, _ = tr.model({k: v.clone() for k, v in batch.items()})
        eager_loss = float(eager_loss.detach())
        graph_loss, _ = tr._graphed_forward_backward(batch, tr._graph_key())
        # the bar of tests/test_lasr_forward_gpu.py::test_graph_replay_matches_eager_forward
        assert abs(float(graph_loss.detach()) - eager_loss) <= 1e-4 * max(1.0, abs(eager_loss))
        assert torch.isfinite(m.tex.grad).all() and float(m.tex.grad.abs().max()) > 0
    finally:
        torch.cuda.set_stream(torch.cuda.default_stream())        # the trainer switched the current stream; restore for other tests
