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


def _run(name, relocated=None):
    """The fake under run_case, or under run_relocated (default: where only that mode can see what is wrong)."""
    mod, lib = guarded_fakes.make()
    if name in guarded_fakes.RELOCATED_MODE if relocated is None else relocated:
        return guarded.run_relocated(guarded_fakes.cases(mod)[name], CPU, modules=[mod], lib=lib, guard_cpu=True)
    guarded.run_case(guarded_fakes.cases(mod)[name], CPU, modules=[mod], lib=lib, guard_cpu=True)


def test_a_clean_operator_passes():
    _run('clean')


@pytest.mark.parametrize('name', guarded_fakes.CLEAN)
def test_a_clean_operator_passes_with_relocated_inputs(name):
    record = _run(name, relocated=True)
    natives = {'clean': 'fake_copy', 'inout': 'fake_accumulate', 'alias': 'fake_add'}
    n = 33 * 4
    assert record == {natives[name]: {'clean': {'args': 1, 'bytes': n}, 'inout': {'args': 2, 'bytes': 2 * n},
                                      'alias': {'args': 2, 'bytes': n}}[name]}       # alias: x and x[5:] are one block


@pytest.mark.parametrize('name', sorted(set(guarded_fakes.EXPECTED) - set(guarded_fakes.RELOCATED_MODE)))
def test_what_the_plain_guard_catches_the_relocated_mode_catches_too(name):
    with pytest.raises(AssertionError) as e:
        _run(name, relocated=True)
    assert guarded_fakes.EXPECTED[name] in str(e.value), str(e.value)


@pytest.mark.parametrize('name', [n for n in guarded_fakes.RELOCATED_MODE if n != 'raw_pointer'])
def test_the_gap_is_real_the_plain_guard_passes_a_stray_read_or_a_write_beside_an_input(name):
    _run(name, relocated=False)


def test_the_caller_s_buffer_holds_the_increment_after_a_relocated_call():
    mod, lib = guarded_fakes.make()
    x, acc = torch.arange(33.), torch.full((33,), 0.5)
    keep = acc.clone()
    with guarded.guarded(0xFF, modules=[mod], lib=lib, guard_cpu=True, relocate=True) as g:
        version = acc._version
        out = mod.inout(x, acc)
        assert acc._version == version                       # written through an alias of the storage, not through acc
        again = mod.inout(x, acc)                            # the same spans: the same two blocks, refreshed from the originals
        assert len(g.blocks) == 2 and not g.violations()
    assert torch.equal(out, keep + x) and torch.equal(again, keep + 2 * x) and torch.equal(acc, keep + 2 * x)
    assert g.relocated == {'fake_accumulate': {'args': 4, 'bytes': 4 * 33 * 4}}


def test_a_relocated_block_is_tight_keeps_the_address_residue_and_is_poisoned():
    mod, lib = guarded_fakes.make()
    seen = {}
    lib_call = lib.call
    lib.call = lambda name, *args: seen.setdefault(name, []).append(args) or lib_call(name, *args)
    parent = torch.arange(7 * 12, dtype=torch.float32).reshape(7, 12)
    view = parent[1:6, 3:9:2]                                # [5, 3], strides (12, 2), 15 floats into the storage
    formula = (1 + 4 * 12 + 2 * 2) * 4
    assert guarded.span_bytes(view) == formula == 212 and guarded.span_bytes(parent) == parent.numel() * 4
    assert guarded.span_bytes(torch.zeros(3).expand(4, 3)) == 12 and guarded.span_bytes(torch.zeros(())) == 4
    with guarded.guarded(0x7F, modules=[mod], lib=lib, guard_cpu=True, relocate=True) as g:
        out = mod.clean(view)
        (b,) = g.blocks.values()
        got = seen['fake_copy'][0][1]
        assert got.shape == view.shape and got.stride() == view.stride() and got.dtype == view.dtype and torch.equal(got, view)
        assert got.data_ptr() != view.data_ptr() and got.data_ptr() % 64 == view.data_ptr() % 64 == (15 * 4 + parent.data_ptr()) % 64
        assert b.backing.data_ptr() % 64 == 0 and got.data_ptr() == b.backing.data_ptr() + b.lead
        assert (b.start, b.nbytes) == (view.data_ptr(), formula) and b.lead == guarded.BAND + view.data_ptr() % 64
        assert b.backing.numel() == b.lead + formula + guarded.BAND
        assert bool((b.backing[:b.lead] == 0x7F).all()) and bool((b.backing[b.lead + formula:] == 0x7F).all())
        assert torch.equal(b.span(), guarded._alias(parent.untyped_storage(), CPU, 15 * 4, formula))
        mod.clean(view)
        assert len(g.blocks) == 1 and seen['fake_copy'][1][1].data_ptr() == got.data_ptr()     # the same span: the same block
        mod.clean(parent[1:6])                               # another span of the same storage: a block of its own
        assert len(g.blocks) == 2 and not g.violations()
        assert seen['fake_copy'][0][0].data_ptr() == out.data_ptr()                             # the guard's own allocation: not moved
        b.backing[b.lead - 1] = 0
        assert g.violations() == [{'input': 'fake_copy', 'arg': 1, 'side': 'before'}]
    assert torch.equal(out, view) and g.relocated == {'fake_copy': {'args': 3, 'bytes': 2 * formula + 5 * 12 * 4}}


def test_tensors_behind_a_pointer_array_are_relocated_and_a_bare_pointer_array_is_refused():
    import ctypes
    from lasr_amd import _lib
    mod, lib = guarded_fakes.make()
    seen = []
    lib.call = lambda name, *args: seen.append(args)
    x, y = torch.arange(5.), torch.arange(3.)
    with guarded.guarded(0xFF, modules=[mod], lib=lib, guard_cpu=True, relocate=True) as g:
        arr = _lib.pointers([x, y])
        assert list(arr) == [x.data_ptr(), y.data_ptr()] and arr.tensors == (x, y)
        lib.call('fake_many', arr, 2)
        (got, two), = seen
        assert two == 2 and type(got) is type(arr) and len(g.blocks) == 2 and g.relocated == {'fake_many': {'args': 2, 'bytes': 32}}
        assert [torch.equal(a, b) for a, b in zip(got.tensors, (x, y))] == [True, True]
        assert list(got) == [t.data_ptr() for t in got.tensors] and not set(got) & set(arr)
        with pytest.raises(guarded.RelocationError) as e:
            lib.call('fake_many', (ctypes.c_void_p * 1)(x.data_ptr() + 8), 1)
        assert 'fake_many: argument 0 holds the integer' in str(e.value)
        lib.call('fake_many', (ctypes.c_int * 2)(5, 3), 2 ** 40, None, 1.5)                     # sizes, a host address: as they are


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


@pytest.mark.parametrize('how', ['unknown kernel', 'raw pointer'])
def test_the_proxy_is_gone_after_an_exception_in_relocate_mode(how):
    mod, lib = guarded_fakes.make()
    real_call = lib.call
    x = torch.arange(4.)
    with pytest.raises(KeyError if how == 'unknown kernel' else guarded.RelocationError):
        with guarded.guarded(0xFF, modules=[mod], lib=lib, guard_cpu=True, relocate=True):
            assert mod.torch is not torch and lib.call is not real_call
            if how == 'unknown kernel':
                mod._lib.call('no_such_kernel', x)
            mod.raw_pointer(x)
    assert mod.torch is torch and lib.call is real_call and torch.equal(x, torch.arange(4.))


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


def test_not_relocated_is_short_declared_and_off_the_training_path():
    import guarded_cases
    names = launched()
    declared = set().union(*(c.natives for c in guarded_cases.CASES))
    left = guarded_cases.NOT_RELOCATED
    assert len(left) <= len(declared) // 10, '%d of %d natives are not relocated: at most one tenth' % (len(left), len(declared))
    assert set(left) <= declared, 'NOT_RELOCATED names a native no case declares: %s' % sorted(set(left) - declared)
    assert all(isinstance(r, str) and r.strip() for r in left.values())
    core = sorted(n for n in left if any(f.startswith(CORE) for f in names.get(n, ())))
    assert not core, 'natives of the training path must be relocatable (pass the view, not an address): %s' % core


def test_the_training_path_hands_over_no_bare_pointer_array():
    """A ctypes array of addresses hides its tensors from the relocation; lasr_amd._lib.pointers keeps them beside it."""
    for path in glob.glob(os.path.join(ROOT, 'lasr_amd', '**', '*.py'), recursive=True):
        rel = os.path.relpath(path, ROOT).replace(os.sep, '/')
        if rel.startswith(CORE):
            with open(path) as fh:
                assert not re.search(r'c_void_p\s*\*', fh.read()), '%s builds a pointer array by hand: use _lib.pointers' % rel


def test_the_product_modules_get_the_proxy_and_get_torch_back():
    from lasr_amd import _lib
    from lasr_amd.nnutils import fused_ops, image_losses
    real_call = _lib.call
    with guarded.guarded(0xFF) as g:
        assert fused_ops.torch is not torch and image_losses.torch is not torch and _lib.call is not real_call
        assert fused_ops.torch.empty(3).untyped_storage().nbytes() == 12 and not g.allocations      # a CPU tensor: not guarded
    assert fused_ops.torch is torch and image_losses.torch is torch and _lib.torch is torch and _lib.call is real_call
