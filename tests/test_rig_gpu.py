"""Rigged glTF export on the device: the four kernels of lasr_amd/csrc/rig.hip against the restatement of tests/rig_restated.py,
the script end to end against the independent GLB reader, and extract.py --rig against the meshes the same export writes.

Wherever float32 device output meets a float64 reference the bound is rig_restated.bound: 4 x the error of the same restatement
run in float32 on the same inputs, at least one float32 ulp.  Measured on an MI355X, kernel error / float32-restatement error:
pack exact (bit-identical), quats 1.00, skin 1.00, stats 1.00 -- the kernels round exactly as the restatement does.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import rig_restated as rr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rig():
    from lasr_amd.nnutils import rig
    return rig


def _dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


@pytest.mark.parametrize('k', [4, 8])
@pytest.mark.parametrize('J', [1, 3, 4, 5, 36, 64])
def test_pack_is_the_restatement_bit_for_bit(cuda, J, k):
    for V in (1, 63, 64, 65, 130):
        skin = rr.softmax_skin(J, V, seed=1000 * J + V)
        assert rr.no_ties(skin, k)                                            # the order is decided; the tie rule has its own test
        joints, weights, dropped = (t.cpu().numpy() for t in _rig().pack_influences(_dev(skin, cuda), k))
        j32, w32, d32 = rr.pack(skin, k, np.float32)
        assert joints.dtype == np.uint8 and joints.shape == (V, k) and (joints == j32).all(), (V, J, k)
        assert weights.tobytes() == w32.tobytes() and dropped.tobytes() == d32.tobytes(), (V, J, k)
        j64, w64, d64 = rr.pack(skin, k)
        assert (j64 == j32).all() and np.abs(w32 - w64).max() <= 4 * 2. ** -24 and np.abs(d32 - d64).max() <= J * 2. ** -24


def test_pack_tie_rule_and_all_zero_column(cuda):
    col = np.array([[0.2, 0., 0.5], [0.3, 0., 0.5], [0.2, 0., 0.], [0.1, 0., 0.], [0.2, 0., 0.], [0., 0., 0.]], np.float32)
    for k in (4, 8):
        joints, weights, dropped = (t.cpu().numpy() for t in _rig().pack_influences(_dev(col, cuda), k))
        j32, w32, d32 = rr.pack(col, k, np.float32)
        assert (joints == j32).all() and weights.tobytes() == w32.tobytes() and dropped.tobytes() == d32.tobytes()
        assert joints[0, :4].tolist() == [1, 0, 2, 4]                         # 0.3, then the three 0.2 by bone index
        assert joints[1].tolist() == [0] * k and weights[1].tolist() == [1] + [0] * (k - 1) and dropped[1] == 0
        assert joints[2].tolist() == [0, 1] + [0] * (k - 2) and weights[2].tolist() == [0.5, 0.5] + [0] * (k - 2)
    assert dropped[0] == 0 and joints[0].tolist() == [1, 0, 2, 4, 3, 0, 0, 0]   # k = 8: bone 5 weighs 0, so its slot holds joint 0


@pytest.mark.parametrize('K', [1, 5])
@pytest.mark.parametrize('T', [1, 2, 7])
def test_quats_are_unit_continuous_and_rebuild_the_rotation(cuda, T, K):
    R = rr.rotations(T, K, seed=7)
    if K > 1:
        assert np.array_equal(R[0, 0], np.eye(3, dtype=np.float32))           # the identity is among the inputs
    q = _rig().rotation_keys(_dev(R, cuda)).cpu().numpy()
    q32, q64 = rr.quats(R, np.float32), rr.quats(R)
    assert ((q64[1:] * q64[:-1]).sum(-1) > 0.1).all()                         # the sign is decided
    want = R.astype(np.float64).transpose(0, 1, 3, 2)
    err, tol = np.abs(rr.quat_matrix(q) - want).max(), rr.bound(rr.quat_matrix(q32), want)
    nerr, ntol = np.abs(np.linalg.norm(q.astype(np.float64), axis=-1) - 1).max(), rr.bound(np.linalg.norm(q32.astype(np.float64), axis=-1), np.ones((T, K)))
    print('quats T %d K %d: R(q) error %.3g (bound %.3g, ratio %.2f), norm error %.3g (bound %.3g), q ratio %.2f'
          % (T, K, err, tol, rr.ratio(rr.quat_matrix(q), rr.quat_matrix(q32), want), nerr, ntol, rr.ratio(q, q32, q64)))
    assert err <= tol and nerr <= ntol
    assert np.abs(q - q64).max() <= rr.bound(q32, q64)
    assert (q[0, :, 3] >= 0).all() and ((q[1:] * q[:-1]).sum(-1) >= 0).all()


def _skin_case(V, T, J, k, seed):
    rs = np.random.RandomState(seed)
    rest = rs.uniform(-1, 1, (V, 3)).astype(np.float32)
    K = J + 1
    R = rr.rotations(T, K, seed)
    trans = (0.3 * rs.randn(T, K, 3)).astype(np.float32)
    trans[:, 0, 2] += 4
    skin = rr.softmax_skin(J, V, seed) if J else None
    joints = weights = None
    if J:
        joints, weights, _ = rr.pack(skin, k, np.float32)
    return rest, skin, R, trans, joints, weights, rr.quats(R, np.float32)


@pytest.mark.parametrize('T', [1, 3])
@pytest.mark.parametrize('V', [1, 65, 1025])
@pytest.mark.parametrize('J,k', [(0, 0), (3, 4), (6, 4), (6, 8)])
def test_skin_is_the_float64_evaluator_and_the_projects_own_lbs(cuda, J, k, V, T):
    from lasr_amd.nnutils import geom_utils
    rest, skin, R, trans, joints, weights, quat = _skin_case(V, T, J, k, seed=V + 10 * T + J)
    dev = [None if a is None else _dev(a, cuda) for a in (rest, joints, weights, quat, trans)]
    got = _rig().skin_packed(*dev).cpu().numpy()
    want, s32 = rr.skin(rest, joints, weights, quat, trans), rr.skin(rest, joints, weights, quat, trans, np.float32)
    err, tol = np.abs(got - want).max(), rr.bound(s32, want)
    print('skin J %d k %d V %d T %d: error %.3g, bound %.3g, ratio %.2f' % (J, k, V, T, err, tol, rr.ratio(got, s32, want)))
    assert got.shape == (T, V, 3) and err <= tol
    if k >= J:                                                                # every weight kept: the full blend on the device
        K = J + 1
        lbs = geom_utils.obj_to_cam(_dev(rest, cuda)[None].expand(T, V, 3).contiguous(), _dev(R, cuda).reshape(T * K, 3, 3),
                                    _dev(trans, cuda).reshape(T * K, 1, 3), K, 1, _dev(skin, cuda)[None, :, :, None] if J else None)
        full = rr.lbs_rows(rest, skin, R, trans)
        err, tol = np.abs(got - lbs.cpu().numpy()).max(), rr.bound(s32, full)
        print('    against obj_to_cam: difference %.3g, bound %.3g' % (err, tol))
        assert err <= tol


@pytest.mark.parametrize('T', [1, 3])
@pytest.mark.parametrize('V', [1, 65, 1025])
def test_stats_bounds_are_exact_sums_within_the_bound_and_runs_identical(cuda, V, T):
    rs = np.random.RandomState(V + T)
    posed = rs.uniform(-2, 2, (T, V, 3)).astype(np.float32)
    ref = (posed + 1e-2 * rs.randn(T, V, 3)).astype(np.float32)
    a, b = _dev(posed, cuda), _dev(ref, cuda)
    got = _rig().deviation(a, b).cpu().numpy()
    again = _rig().deviation(a, b).cpu().numpy()
    assert got.tobytes() == again.tobytes()
    want, s32 = rr.stats(posed, ref), rr.stats(posed, ref, np.float32)
    assert np.array_equal(got[:, 2:5], posed.min(1)) and np.array_equal(got[:, 5:8], posed.max(1))
    for c, name in ((0, 'max'), (1, 'sum of squares')):
        err, tol = np.abs(got[:, c] - want[:, c]).max(), rr.bound(s32[:, c], want[:, c])
        print('stats V %d T %d %s: error %.3g, bound %.3g, ratio %.2f' % (V, T, name, err, tol, rr.ratio(got[:, c], s32[:, c], want[:, c])))
        assert err <= tol


def _export(tmp_path, npz, capsys, *flags):
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    import export_gltf
    d = str(tmp_path)
    np.savez(os.path.join(d, 'rig.npz'), **npz)
    out = os.path.join(d, 'out.glb')
    capsys.readouterr()
    arrays, report = export_gltf.main(['--testdir', d, '--outpath', out] + list(flags))
    printed = capsys.readouterr().out.splitlines()
    gltf, binary = rr.read_glb(open(out, 'rb').read())
    rr.check_rules(gltf, binary)
    return export_gltf, arrays, report, printed, rr.evaluate(gltf, binary)[0]


def _restated_report(eg, npz, arrays, k):
    """The line the script prints, from the float64 restatement alone."""
    a64, posed64 = rr.restated_arrays(npz, k, np.float64)
    full = rr.lbs_rows(npz['rest_verts'], npz['skin'], npz['R'], npz['T'])
    mx, rms, mo, frame, ro = rr.report(posed64, full, npz['rest_verts'])
    return eg.report_line(arrays, dict(influences=k, max_overall=mo, frame=frame, rms_overall=ro)), mx, rms, posed64, full


def test_end_to_end_the_written_file_poses_as_the_kernel_does(cuda, tmp_path, capsys):
    npz = rr.handmade_rig(J=3, T=4)
    eg, arrays, report, printed, got = _export(tmp_path, npz, capsys)         # --influences auto
    file64 = rr.skin(arrays['positions'], arrays['joints'], arrays['weights'], arrays['quat'], arrays['trans'])
    file32 = rr.skin(arrays['positions'], arrays['joints'], arrays['weights'], arrays['quat'], arrays['trans'], np.float32)
    assert np.abs(got - arrays['posed']).max() <= rr.bound(file32, file64)
    assert np.abs(got - file64).max() <= rr.bound(file32, file64)
    line, mx, rms, posed64, full = _restated_report(eg, npz, arrays, 4)
    print(printed[0])
    frameless = lambda text: re.sub(r' \(frame \d+\)', '', text)              # noqa: E731  (rounding alone picks the frame here)
    assert frameless(printed[0]) == frameless(line) and '(frame ' in printed[0] and report['influences'] == 4   # auto stays at 4
    assert report['max_overall'] <= rr.bound(file32, full) / report['diag']  # zero, within the bound
    assert np.array_equal(arrays['frame_ids'], npz['frame_ids']) and printed[1].startswith('wrote ')


def test_end_to_end_truncation_shows_in_the_report_and_eight_influences_remove_it(cuda, tmp_path, capsys):
    npz = rr.handmade_rig(J=5, T=4, seed=2)
    assert rr.no_ties(npz['skin'], 4)
    eg, arrays, report, printed, got = _export(tmp_path, npz, capsys, '--influences', '4')
    line, mx, rms, posed64, full = _restated_report(eg, npz, arrays, 4)
    _, posed32 = rr.restated_arrays(npz, 4, np.float32)
    tol = rr.bound(posed32, posed64) / report['diag']
    print(printed[0], '| restated max %s' % mx)
    assert np.sort(mx)[-1] - np.sort(mx)[-2] > 2 * tol                        # the worst frame is decided
    assert printed[0] == line
    assert report['max_overall'] > 100 * tol                                  # the truncation, not rounding
    assert np.abs(report['max'] - mx).max() <= tol and np.abs(report['rms'] - rms).max() <= tol
    assert np.abs(got - posed64).max() <= rr.bound(posed32, posed64)
    eg, arrays, report, printed, got = _export(tmp_path, npz, capsys, '--influences', '8')
    _, posed32 = rr.restated_arrays(npz, 8, np.float32)
    assert report['max_overall'] <= rr.bound(posed32, full) / report['diag'] and np.abs(got - full).max() <= rr.bound(posed32, full)
    # auto: 4 influences exceed a bar below their deviation, so the script goes to 8
    eg, arrays, report, printed, got = _export(tmp_path, npz, capsys, '--max_dev', repr(0.5 * float(mx.max())))
    assert report['influences'] == 8 and arrays['joints'].shape[1] == 8


class _Replay:
    """Stands in for the trainer's model: records what export() reads of every forward (the camera-space vertices and the
    camera sources, per batch) and, once `play` is set, puts the recording back in place of a new forward.  Two forwards of the
    same batch differ in the last digits (the forward's library kernels are not bitwise reproducible, as
    tests/test_phong_gpu.py documents), so byte identity of two exports can only be asked of the same forwards."""

    def __init__(self, model, module):
        self.model, self.module, self.tape, self.play = model, module, [], None

    def train(self):
        self.model.train()

    def __call__(self, bi):
        m = self.module
        if self.play is None:
            out = self.model(bi)
            self.tape.append((bi['frameid'].clone(), m.verts_cam.clone(), tuple(t.clone() if torch.is_tensor(t) else t for t in m._cam_src)))
            return out
        ids, m.verts_cam, m._cam_src = self.tape[self.play]
        assert torch.equal(ids, bi['frameid'])                                # the loader serves the batches in the same order
        self.play += 1


def test_extract_rig_reproduces_the_exported_meshes_and_changes_no_other_file(cuda, tmp_path, monkeypatch):
    # the fresh five-bone, two-hypothesis model of a three-frame 64 x 64 rendered sequence of tests/test_vis_gpu.py
    sys.path.insert(0, ROOT)
    import extract
    import optimize
    from lasr_amd.ext_utils.ply import read_ply
    from lasr_amd.nnutils import train_utils
    root = str(tmp_path / 'data')
    rc = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'render_syn.py'), '--outdir', 'rig3', '--nframes', '3',
                         '--img_size', '64', '--root', root], cwd=ROOT, timeout=600, capture_output=True, text=True)
    assert rc.returncode == 0, rc.stderr[-2000:]
    opts = optimize.parse_flags(['--name', 't', '--checkpoint_dir', str(tmp_path), '--img_size', '64', '--subdivide', '2',
                                 '--n_bones', '5', '--n_hypo', '2', '--batch_size', '1', '--opt_tex', 'yes', '--nouse_gtpose',
                                 '--only_mean_sym', '--noperceptual', '--nouse_graph', '--dataname', 'rig3', '--data_root', root])
    torch.manual_seed(0)
    tr = train_utils.LASRTrainer(opts).init_training()
    tr.reinit_bones()
    m = tr.module
    with torch.no_grad():                                          # distinct bone shapes and orientations
        m.ctl_rs.add_(0.3 * torch.randn_like(m.ctl_rs))
        m.log_ctl.copy_(torch.randn_like(m.log_ctl))
    tr.epoch_nscore = torch.tensor([1., 0.], device=cuda)          # the second hypothesis scores best
    plain, rigged = os.path.join(str(tmp_path), 'plain'), os.path.join(str(tmp_path), 'rigged')
    tr.model = _Replay(tr.model, m)
    assert tr.module is m
    assert sorted(extract.export(tr, plain)) == [0, 1, 2]
    tr.model.play = 0                                              # the same forwards again, now with rig=True
    assert sorted(extract.export(tr, rigged, rig=True)) == [0, 1, 2]
    assert tr.model.play == len(tr.model.tape) >= 2
    assert sorted(os.listdir(rigged)) == sorted(os.listdir(plain) + ['rig.npz'])
    for name in os.listdir(plain):
        assert open(os.path.join(plain, name), 'rb').read() == open(os.path.join(rigged, name), 'rb').read(), name
    npz = dict(np.load(os.path.join(rigged, 'rig.npz')))
    V, F = npz['rest_verts'].shape[0], m.faces.shape[0]
    assert npz['rest_verts'].shape == (V, 3) and npz['faces'].shape == (F, 3) and npz['colors'].shape == (V, 3)
    assert npz['skin'].shape == (4, V) and npz['R'].shape == (3, 5, 3, 3) and npz['T'].shape == (3, 5, 3) and npz['intrinsics'].shape == (3, 4)
    assert npz['frame_ids'].tolist() == [0, 1, 2] and 0 <= npz['colors'].min() and npz['colors'].max() <= 1
    assert np.abs(npz['skin'].sum(0) - 1).max() < 1e-5
    posed = rr.lbs_rows(npz['rest_verts'], npz['skin'], npz['R'], npz['T'])
    for i, fid in enumerate(npz['frame_ids']):
        ply = read_ply(os.path.join(rigged, 'pred%d.ply' % fid))
        extent = np.ptp(ply['verts'], axis=0).max()
        err = np.abs(posed[i] - ply['verts']).max()
        print('frame %d: re-skinned rig against pred%d.ply %.3g of the extent' % (fid, fid, err / extent))
        assert ply['verts'].shape == (V, 3) and (ply['faces'] == npz['faces']).all() and err <= 1e-5 * extent
        rtk = np.loadtxt(os.path.join(rigged, 'cam%d.txt' % fid))
        assert np.array_equal(rtk[:3, :3].astype(np.float32), npz['R'][i, 0]) and np.array_equal(rtk[:3, 3].astype(np.float32), npz['T'][i, 0])
        assert np.array_equal(rtk[3].astype(np.float32), npz['intrinsics'][i])
    # and the rig goes through the exporter: five bones, four joints, every weight kept
    arrays, report = _rig().build_rig(npz, 4)
    tol = rr.bound(rr.restated_arrays(npz, 4, np.float32)[1], posed) / report['diag']
    print('build_rig on the extracted rig: max deviation %.3g of the diagonal, bound %.3g' % (report['max_overall'], tol))
    assert arrays['joints'].shape == (V, 4) and report['max_overall'] <= tol
    # one rig holds one rest shape and one skin: a batch that brings another is refused
    real, calls = extract.rig_batch, []

    def drifting(tr_, n, best):
        rest, skin, R, T = real(tr_, n, best)
        calls.append(n)
        return (rest if len(calls) == 1 else rest + 1e-3), skin, R, T
    monkeypatch.setattr(extract, 'rig_batch', drifting)
    tr.model.play = 0
    with pytest.raises(ValueError, match='differs between batches'):
        extract.export(tr, os.path.join(str(tmp_path), 'refused'), rig=True)
    assert len(calls) == 2 and not os.path.exists(os.path.join(str(tmp_path), 'refused', 'rig.npz'))
