"""tests/guarded.py catches what it claims to catch: deliberately wrong operators (tests/guarded_fakes.py) on CPU tensors, and
the table of tests/guarded_cases.py names every native the package launches."""
import glob
import os
import re

import pytest
import torch

import guarded
import guarded_fakes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device('cpu')


def _run(name):
    mod, lib = guarded_fakes.make()
    guarded.run_case(guarded_fakes.cases(mod)[name], CPU, modules=[mod], lib=lib, guard_cpu=True)


def test_a_clean_operator_passes():
    _run('clean')


@pytest.mark.parametrize('name', sorted(guarded_fakes.EXPECTED))
def test_a_wrong_operator_is_caught_by_its_rule(name):
    with pytest.raises(AssertionError) as e:
        _run(name)
    assert guarded_fakes.EXPECTED[name] in str(e.value), str(e.value)


def test_the_interior_is_tight_aligned_and_poisoned():
    mod, lib = guarded_fakes.make()
    with guarded.guarded(0x7F, modules=[mod], lib=lib, guard_cpu=True) as g:
        t = mod.torch.empty(3, 5, dtype=torch.float32)
        i = mod.torch.empty((7,), dtype=torch.int32, device='cpu')
        like = mod.torch.empty_like(torch.zeros(4, 6).t())
        z = mod.torch.empty(0, dtype=torch.float64)
        pinned = mod.torch.empty(4, requires_grad=False)                   # any other keyword: the real function
        assert mod.torch.zeros is torch.zeros and mod.torch.float32 is torch.float32
    assert [a.nbytes for a in g.allocations] == [60, 28, 96, 0] and pinned.untyped_storage().nbytes() == 16
    assert t.shape == (3, 5) and t.is_contiguous() and like.shape == (6, 4) and like.is_contiguous() and z.numel() == 0
    for a, x in zip(g.allocations, (t, i, like, z)):
        assert a.backing.numel() == 2 * guarded.BAND + a.nbytes and x.storage_offset() * x.element_size() == guarded.BAND
        assert x.numel() == 0 or x.data_ptr() - a.backing.data_ptr() == guarded.BAND          # (an empty tensor has no address)
        assert bool((a.backing == 0x7F).all())
    assert float(t[0, 0]) > 3e38 and int(i[0]) == 2139062143 and not g.violations()
    i.as_strided((1,), (1,), i.storage_offset() + 7).fill_(0)
    assert g.violations() == [{'ordinal': 1, 'shape': (7,), 'dtype': torch.int32, 'side': 'after'}]
    assert guarded.BAND == 65536 and guarded.FILLS == (0xFF, 0x7F)


def test_the_proxy_is_gone_after_an_exception():
    mod, lib = guarded_fakes.make()
    real_call = lib.call
    with pytest.raises(KeyError):
        with guarded.guarded(0xFF, modules=[mod], lib=lib, guard_cpu=True):
            assert mod.torch is not torch and lib.call is not real_call
            mod._lib.call('no_such_kernel')
    assert mod.torch is torch and lib.call is real_call


# ---- completeness: every native the package launches is in the table ---------------------------------------------------------------
CORE = ('lasr_amd/nnutils/fused_ops.py', 'lasr_amd/nnutils/geom_utils.py', 'lasr_amd/nnutils/image_losses.py',
        'lasr_amd/nnutils/loss_utils.py', 'lasr_amd/soft_renderer/functional/', 'lasr_amd/chamfer3D/')


def first_argument(text, at):
    """The source of the first argument of the call whose '(' is text[at - 1]: up to the first comma (or the closing bracket) that
    is inside no bracket and no string."""
    depth, quote, i = 0, None, at
    while i < len(text):
        c = text[i]
        if quote:
            if c == '\\':
                i += 1
            elif c == quote:
                quote = None
        elif c in '\'"':
            quote = c
        elif c in '([{':
            depth += 1
        elif c in ')]}':
            if depth == 0:
                break
            depth -= 1
        elif c == ',' and depth == 0:
            break
        i += 1
    return text[at:i]


def launched_in(text):
    """Every 'lasr_...' literal in the first argument of a call(...) site (`call('a' if x else 'b', ...)` names two), and the
    sites whose first argument holds none: a name kept in a variable, which the scan cannot follow."""
    names, opaque = [], []
    for m in re.finditer(r"(?<!def )\bcall\(", text):                # (not the helper's own definition)
        arg = first_argument(text, m.end())
        found = re.findall(r"['\"](lasr_\w+)['\"]", arg)
        names += found
        if not found:
            opaque.append(arg.strip())
    return names, opaque


def launched():
    """name -> the files (relative, with '/') that launch it."""
    out = {}
    for path in glob.glob(os.path.join(ROOT, 'lasr_amd', '**', '*.py'), recursive=True):
        rel = os.path.relpath(path, ROOT).replace(os.sep, '/')
        with open(path) as fh:
            names, opaque = launched_in(fh.read())
        assert not opaque, '%s: a launch whose native is no literal: %s (name it in the call)' % (rel, opaque)
        for name in names:
            out.setdefault(name, set()).add(rel)
    return out


def test_the_scan_sees_both_names_of_a_conditional_and_flags_a_variable():
    names, opaque = launched_in("_lib.call('lasr_a_f64' if d else 'lasr_a', x, f('lasr_no', 1))\ncall(\"lasr_b\", y)\n_lib.call(fn, z)")
    assert names == ['lasr_a_f64', 'lasr_a', 'lasr_b'] and opaque == ['fn']


def test_every_launched_native_is_in_a_case_or_named_as_not_covered():
    import guarded_cases
    names = launched()
    assert len(names) > 100 and 'lasr_sr_forward_opt' in names and 'lasr_lbs_forward' in names      # (the scan still finds the sites)
    covered = set().union(*(c.natives for c in guarded_cases.CASES))
    skipped = guarded_cases.NOT_COVERED
    missing = sorted(set(names) - covered - set(skipped))
    assert not missing, 'launched, but in no case of tests/guarded_cases.py and not in NOT_COVERED: %s' % missing
    assert not set(skipped) & covered and set(skipped) <= set(names), 'NOT_COVERED names a covered or an unknown native'
    assert all(isinstance(r, str) and r.strip() for r in skipped.values())
    assert len(skipped) <= len(names) // 10, '%d of %d natives are not covered: at most one tenth' % (len(skipped), len(names))
    core = sorted(n for n in skipped if any(f.startswith(CORE) for f in names[n]))
    assert not core, 'natives of the training path may not be left out: %s' % core
    assert len({c.name for c in guarded_cases.CASES}) == len(guarded_cases.CASES)


def test_the_product_modules_get_the_proxy_and_get_torch_back():
    from lasr_amd import _lib
    from lasr_amd.nnutils import fused_ops, image_losses
    real_call = _lib.call
    with guarded.guarded(0xFF) as g:
        assert fused_ops.torch is not torch and image_losses.torch is not torch and _lib.call is not real_call
        assert fused_ops.torch.empty(3).untyped_storage().nbytes() == 12 and not g.allocations      # a CPU tensor: not guarded
    assert fused_ops.torch is torch and image_losses.torch is torch and _lib.torch is torch and _lib.call is real_call
