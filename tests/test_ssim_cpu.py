"""The SSIM texture term (optimize.py --ptex_method ssim) without a GPU: closed forms and the hand-derived
gradient of the restatement (tests/ssim_restated.py, the definition), the torch composition against it, the header against the
binding, the refusals of the entry points and of the Python layer, the flags, and the conditioning of the GPU test's fixtures."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import optimize                                                    # noqa: E402
import ssim_restated as sr                                         # noqa: E402
import ssim_cases                                                  # noqa: E402
from lasr_amd import _lib, synth_data                              # noqa: E402
from lasr_amd.nnutils import fused_ops, mesh_net, train_utils      # noqa: E402


# ---- 1. closed forms on the restatement ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('L', [1., 2.])
def test_constant_images_give_the_closed_form(dtype, L):
    c1, c2 = 0.3, 0.75
    a, b = np.full((1, 3, 20, 45), c1, dtype), np.full((2, 3, 20, 45), c2, dtype)
    C1 = (0.01 * L) ** 2
    want = (2 * c1 * c2 + C1) / (c1 * c1 + c2 * c2 + C1)
    s = sr.ssim_map(a, b, 2, L, dtype)
    tol = 1e-12 if dtype is np.float64 else 2e-5        # the variances of a constant are rounding noise against C2 = 9e-4 L^2
    assert s.shape == (2, 3, 10, 35) and np.abs(s - want).max() <= tol
    assert np.abs(sr.distance(a, b, 2, L, dtype) - (1 - want)).max() <= tol
    # multi-scale of constants equals single-scale: pooling a constant gives the constant
    a, b = np.full((1, 3, 48, 52), c1, dtype), np.full((1, 3, 48, 52), c2, dtype)
    assert np.abs(sr.multiscale_distance(a, b, 1, L, 3, dtype) - sr.distance(a, b, 1, L, dtype)).max() <= tol


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_distance_of_an_image_to_itself_is_exactly_zero(dtype):
    # a b == a a bit for bit, 2 x == x + x, so numerator and denominator of s are the same number and s == 1; sums of ones are
    # exact in the block order and in the float64 fold
    a, _ = sr.texture_pair(2, 1, 43, 57, seed=3)
    assert np.all(sr.ssim_map(a, a, 1, 1., dtype) == 1)
    assert np.all(sr.distance(a, a, 1, 1., dtype) == 0) and np.all(sr.distance(a, np.repeat(a, 3, 0), 3, 2., dtype) == 0)


def test_window_sums_to_one_within_an_ulp_and_is_the_kernel_s():
    assert abs(sr.window(np.float64).sum() - 1) <= np.finfo(np.float64).eps
    g32 = sr.window(np.float32)
    assert abs(g32.astype(np.float64).sum() - 1) <= np.finfo(np.float32).eps and np.all(g32 == g32[::-1])
    src = open(os.path.join(ROOT, 'lasr_amd', 'csrc', 'ssim.hip')).read()
    body = re.search(r'SS_WINDOW = \{\{(.*?)\}\}', src, re.S).group(1)
    lits = [np.float32(x.strip().rstrip('f')) for x in body.split(',')]
    assert len(lits) == 11 and np.all(np.array(lits, np.float32) == g32)


# ---- 2. gradient ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('M,rep,H,W,L', [(1, 1, 11, 11, 1.), (2, 3, 26, 27, 2.), (1, 2, 43, 33, 1.)])
def test_hand_derived_gradient_equals_autograd_of_the_restated_forward(M, rep, H, W, L):
    a, b = sr.texture_pair(M, rep, H, W, seed=H + W, unit_range=L == 1.)
    gd = np.random.RandomState(1).standard_normal(M * rep)
    tb = torch.from_numpy(b).double().requires_grad_(True)
    d = sr.distance_torch64(torch.from_numpy(a), tb, rep, L)
    assert np.abs(d.detach().numpy() - sr.distance(a, b, rep, L)).max() <= 1e-12
    d.backward(torch.from_numpy(gd))
    mine = sr.grad_b(a, b, gd, rep, L)
    assert np.abs(mine - tb.grad.numpy()).max() <= 1e-12 * np.abs(tb.grad.numpy()).max()


@pytest.mark.parametrize('M,rep,H,W,L', [(1, 1, 12, 11, 2.), (2, 3, 27, 26, 1.), (2, 1, 64, 80, 1.)])
def test_torch_composition_in_float64_equals_the_restatement(M, rep, H, W, L):
    a, b = sr.texture_pair(M, rep, H, W, seed=7 * H + W, unit_range=L == 1.)
    gd = np.random.RandomState(2).standard_normal(M * rep)
    tb = torch.from_numpy(b).double().requires_grad_(True)
    d = fused_ops.ssim_distance_torch(torch.from_numpy(a).double(), tb, rep, L)
    assert d.shape == (M * rep,) and np.abs(d.detach().numpy() - sr.distance(a, b, rep, L)).max() <= 1e-12
    d.backward(torch.from_numpy(gd))
    want = sr.grad_b(a, b, gd, rep, L)
    assert np.abs(tb.grad.numpy() - want).max() <= 1e-12 * np.abs(want).max()
    # the observed side gets a gradient too in this form
    ta = torch.from_numpy(a).double().requires_grad_(True)
    fused_ops.ssim_distance_torch(ta, torch.from_numpy(b).double(), rep, L).sum().backward()
    assert ta.grad is not None and float(ta.grad.abs().max()) > 0


# ---- 3. header against binding -------------------------------------------------------------------------------------------------
def test_header_prototypes_constants_and_signatures_agree():
    hdr = open(os.path.join(ROOT, 'include', 'lasr_ops.h')).read()
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    protos = dict((m.group(2), (m.group(1), m.group(3))) for m in re.finditer(r'(\w+)\s+(lasr_ssim_\w+)\s*\(([^)]*)\)\s*;', code))
    assert sorted(protos) == sorted(k for k in _lib.SIGNATURES if k.startswith('lasr_ssim_')) == \
        ['lasr_ssim_backward', 'lasr_ssim_forward', 'lasr_ssim_scratch_floats']

    def kind(decl):
        decl = decl.strip()
        if '*' in decl:
            return ctypes.c_void_p
        return {'int': ctypes.c_int, 'float': ctypes.c_float, 'size_t': ctypes.c_size_t}[decl.split()[0]]
    for name, (res, args) in protos.items():
        assert _lib.SIGNATURES[name] == (kind(res), [kind(x) for x in args.split(',')]), name
    assert protos['lasr_ssim_forward'][1].split(',')[-1].strip() == 'void* hip_stream'
    assert protos['lasr_ssim_backward'][1].split(',')[-1].strip() == 'void* hip_stream'
    for name, mine in (('MIN_SIZE', _lib.SSIM_MIN_SIZE), ('MAX_SIZE', _lib.SSIM_MAX_SIZE), ('TILE_W', _lib.SSIM_TILE_W),
                       ('TILE_H', _lib.SSIM_TILE_H)):
        assert int(re.search(r'#define\s+LASR_SSIM_%s\s+(\d+)' % name, hdr).group(1)) == mine == getattr(sr, name)
    assert (_lib.SSIM_MIN_SIZE, _lib.SSIM_MAX_SIZE) == (11, 4096)
    assert _lib.ABI_VERSION == 13 and _lib.lib().lasr_abi_version() == 13
    assert 'the reference has no counterpart' in re.search(r'/\*(?:(?!\*/).)*lasr_ssim_forward:.*?\*/', hdr, re.S).group(0)


# ---- 4. refusals of the entry points (on the host, before any launch: the addresses are never dereferenced) ----------------------
def test_entry_points_refuse_bad_arguments_on_the_host():
    h = _lib.lib()
    A, B, D, P, S, G, GB = (ctypes.c_void_p(0x1000 * i) for i in range(1, 8))
    ok = (2, 3, 64, 80, 1.0)

    def fwd(a=A, b=B, d=D, p=P, s=S, dims=ok):
        return h.lasr_ssim_forward(a, b, d, p, s, *dims, None)

    def bwd(a=A, b=B, p=P, g=G, gb=GB, dims=ok):
        return h.lasr_ssim_backward(a, b, p, g, gb, *dims, None)
    for which in 'abds':
        assert fwd(**{which: None}) == -1, which
    for which in ('a', 'b', 'g', 'gb'):
        assert bwd(**{which: None}) == -1, which
    bad = [(2, 3, 10, 80, 1.0), (2, 3, 64, 10, 1.0), (2, 3, 4097, 80, 1.0), (2, 3, 64, 4097, 1.0), (2, 0, 64, 80, 1.0),
           (2, -1, 64, 80, 1.0), (0, 3, 64, 80, 1.0), (-2, 3, 64, 80, 1.0), (2, 3, 64, 80, 0.0), (2, 3, 64, 80, -1.0),
           (2, 3, 64, 80, float('nan')), (2, 3, 64, 80, float('inf')), (21846, 1, 64, 80, 1.0)]
    for dims in bad:
        assert fwd(dims=dims) == -1 and bwd(dims=dims) == -1 and fwd(p=None, dims=dims) == -1 and bwd(p=None, dims=dims) == -1, dims
        assert h.lasr_ssim_scratch_floats(*dims[:4]) == 0 or dims[4] != 1.0
    assert fwd(d=A) == -1 and fwd(s=D) == -1 and fwd(p=B) == -1 and bwd(gb=B) == -1 and bwd(gb=G) == -1      # aliased outputs
    # one block sum per tile of the output map, channel and image
    tiles = lambda n, t: -(-(n - 10) // t)                                                                  # noqa: E731
    assert h.lasr_ssim_scratch_floats(2, 3, 64, 80) == 6 * 3 * tiles(80, _lib.SSIM_TILE_W) * tiles(64, _lib.SSIM_TILE_H)
    assert h.lasr_ssim_scratch_floats(1, 1, 11, 11) == 3 and h.lasr_ssim_scratch_floats(1, 1, 4096, 4096) == 3 * 128 * 256


# ---- 5. refusals of the Python layer -------------------------------------------------------------------------------------------
def test_python_layer_refusals():
    a, b = torch.zeros(2, 3, 16, 16), torch.zeros(6, 3, 16, 16)
    with pytest.raises(TypeError, match='only cuda'):
        fused_ops.ssim_distance(a, b, 3)
    for fn in (fused_ops.ssim_distance_torch,):
        with pytest.raises(ValueError, match='repeat'):
            fn(a, b, 2)                                             # N is not a multiple of repeat
        with pytest.raises(ValueError, match='3,H,W'):
            fn(torch.zeros(2, 4, 16, 16), torch.zeros(2, 4, 16, 16))
        with pytest.raises(ValueError, match='11'):
            fn(torch.zeros(1, 3, 10, 16), torch.zeros(1, 3, 10, 16))
        with pytest.raises(ValueError, match='data_range'):
            fn(a, b, 3, 0.)
    net = mesh_net.StructuralDistance(scales=3, use_kernel=False)
    assert not list(net.parameters()) and not list(net.buffers()) and not net.state_dict()
    with pytest.raises(ValueError, match=r'scale 2 of 3 is 10 x 10'):
        net.forward_pair(torch.zeros(1, 3, 40, 40), torch.zeros(1, 3, 40, 40))
    with pytest.raises(ValueError, match=r'scale 2 is 10 x 11'):
        sr.multiscale_distance(np.zeros((1, 3, 40, 44)), np.zeros((1, 3, 40, 44)))
    with pytest.raises(ValueError):
        mesh_net.StructuralDistance(scales=0)
    # the module on CPU tensors is the torch composition and agrees with the restated multi-scale form
    xa, xb = sr.texture_pair(1, 2, 48, 52, seed=5)
    d = net.forward_pair(torch.from_numpy(xa).double(), torch.from_numpy(xb).double(), repeat=2, unit_range=True)
    assert np.abs(d.numpy() - sr.multiscale_distance(xa, xb, 2, 1., 3)).max() <= 1e-12
    d2 = net.forward_pair(torch.from_numpy(2 * xa - 1).double(), torch.from_numpy(2 * xb - 1).double(), repeat=2)
    assert np.abs(d2.numpy() - sr.multiscale_distance(2. * xa - 1, 2. * xb - 1, 2, 2., 3)).max() <= 1e-12     # unit_range False: L = 2


# ---- 6. flags ------------------------------------------------------------------------------------------------------------------
class _NoSequence:
    def __init__(self, *a, **k):
        pass

    def pairs(self):
        return [(0, 1), (1, 2)]


def _trainer(tmp_path, monkeypatch, *extra):
    monkeypatch.setattr(synth_data, 'SyntheticSequence', _NoSequence)
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    opts = optimize.parse_flags(['--name', 't', '--checkpoint_dir', str(tmp_path), '--img_size', '64', '--subdivide', '1',
                                 '--n_bones', '3', '--n_hypo', '2', '--batch_size', '1', '--opt_tex', 'yes',
                                 '--iters_per_epoch', '4', '--nouse_graph'] + list(extra))
    torch.manual_seed(0)
    return train_utils.LASRTrainer(opts).init_training()


def test_flag_defaults_and_parsing():
    d = optimize.DEFAULTS
    assert (d['ptex_method'], d['ssim_wt'], d['ssim_scales']) == ('alexnet', 0.125, 3)
    assert type(d['ssim_wt']) is float and type(d['ssim_scales']) is int
    o = optimize.parse_flags('--ptex_method ssim --ssim_wt 0.25 --ssim_scales=2'.split())
    assert (o.ptex_method, o.ssim_wt, o.ssim_scales, o.perceptual) == ('ssim', 0.25, 2, True)
    o = optimize.parse_flags('--ptex_method ssim --noperceptual'.split())
    assert o.ptex_method == 'ssim' and o.perceptual is False
    demo = open(os.path.join(ROOT, 'scripts', 'reconstruct_demo.py')).read()
    assert "'--ptex_method', args.ptex_method" in demo


def test_trainer_builds_the_chosen_term(tmp_path, monkeypatch, capsys):
    tr = _trainer(tmp_path / 'a', monkeypatch, '--ptex_method', 'ssim', '--ssim_scales', '2')
    assert type(tr.module.ptex_loss) is mesh_net.StructuralDistance and tr.module.ptex_loss.scales == 2
    assert 'AlexNet' not in capsys.readouterr().err
    tr = _trainer(tmp_path / 'b', monkeypatch)
    assert type(tr.module.ptex_loss) is mesh_net.PerceptualDistance
    assert '--ptex_method ssim' in capsys.readouterr().err          # the notice about random AlexNet features names the way out
    for method in ('ssim', 'alexnet'):
        tr = _trainer(tmp_path / ('c' + method), monkeypatch, '--ptex_method', method, '--noperceptual')
        assert tr.module.ptex_loss is None


def test_trainer_refuses_an_unknown_method_and_ignored_weights(tmp_path, monkeypatch):
    with pytest.raises(ValueError, match="ptex_method 'lpips'"):
        _trainer(tmp_path, monkeypatch, '--ptex_method', 'lpips')
    with pytest.raises(ValueError, match="ptex_method 'lpips'"):
        _trainer(tmp_path, monkeypatch, '--ptex_method', 'lpips', '--noperceptual')
    with pytest.raises(ValueError, match='alexnet_weights .* with --ptex_method ssim'):
        _trainer(tmp_path, monkeypatch, '--ptex_method', 'ssim', '--alexnet_weights', str(tmp_path / 'w.pth'))
    with pytest.raises(ValueError, match='ssim_scales 4 at --img_size 64'):
        _trainer(tmp_path, monkeypatch, '--ptex_method', 'ssim', '--ssim_scales', '4')


@pytest.mark.parametrize('first,second', [('alexnet', 'ssim'), ('ssim', 'alexnet')])
def test_checkpoints_move_between_the_methods(tmp_path, monkeypatch, first, second):
    a = _trainer(tmp_path / 'a', monkeypatch, '--ptex_method', first)
    with torch.no_grad():
        a.module.mean_v.add_(0.01 * torch.randn(a.module.mean_v.shape, generator=torch.Generator().manual_seed(1)))
        a.module.tex.add_(0.1)
    a.epoch_nscore = torch.zeros(2)
    a.save('latest')
    path = os.path.join(a.save_dir, 'pred_net_latest.pth')
    keys = set(torch.load(path, map_location='cpu'))
    assert any(k.startswith('ptex_loss.') for k in keys) == (first == 'alexnet')      # the structural term adds no keys
    b = _trainer(tmp_path / 'b', monkeypatch, '--ptex_method', second, '--model_path', path)
    assert type(b.module.ptex_loss) is (mesh_net.StructuralDistance if second == 'ssim' else mesh_net.PerceptualDistance)
    assert torch.equal(b.module.mean_v.data, a.module.mean_v.data) and torch.equal(b.module.tex.data, a.module.tex.data)
    sa, sb = a.module.state_dict(), b.module.state_dict()
    for k in sa:
        if not k.startswith('ptex_loss.'):
            assert torch.equal(sa[k], sb[k]), k


# ---- 7. conditioning of the fixtures of tests/test_ssim_gpu.py -------------------------------------------------------------------
def test_fixtures_are_well_conditioned(capsys):
    worst_v = worst_g = 0.
    cases = ssim_cases.cases(_lib.SSIM_TILE_W, _lib.SSIM_TILE_H)
    assert len(cases) >= 40
    for case in cases:
        r = ssim_cases.reference(case)
        sv = np.abs(r['d32'].astype(np.float64) - r['d64']).max() / np.abs(r['d64']).max()
        sg = np.abs(r['g32'].astype(np.float64) - r['g64']).max() / np.abs(r['g64']).max()
        worst_v, worst_g = max(worst_v, sv), max(worst_g, sg)
        with capsys.disabled():
            print('ssim fixture %-34s value spread %.2e  gradient spread %.2e' % (case, sv, sg))
        assert sv < 1e-3 and sg < 1e-3, (case, sv, sg)
    with capsys.disabled():
        print('ssim fixtures: worst relative float32 / float64 spread, value %.2e, gradient %.2e' % (worst_v, worst_g))
