"""_lib.call / _lib.f32, the one way from an operator into liblasr_hip.so, without a GPU: the real library loads without a device
and its entry points validate on the host before any launch (as tests/test_abi.py relies on); the stream is a null one."""
import contextlib
import os
import re

import pytest
import torch

from lasr_amd import _lib

DEV0 = torch.device('cuda', 0)
QUAT = 'lasr_quat_to_rotmat_forward'                               # (quat, rotmat, M, stream)


@pytest.fixture(autouse=True)
def null_stream(monkeypatch):
    monkeypatch.setattr(_lib, 'stream_of', lambda t: (contextlib.nullcontext(), None))


class _Stub:
    """A handle whose one entry point records that it was entered."""

    def __init__(self, n_args):
        self.entered = []

        def fn(*args):
            self.entered.append(args)
            return 0
        fn.argtypes = [None] * n_args
        setattr(self, QUAT, fn)


@pytest.fixture
def stub(monkeypatch):
    h = _Stub(len(_lib.SIGNATURES[QUAT][1]))
    monkeypatch.setattr(_lib, '_lib', h)
    return h


def test_empty_problem_returns_and_bad_argument_names_the_entry_point():
    assert _lib.call(QUAT, None, None, 0, on=DEV0) is None
    with pytest.raises(_lib.LasrNativeError) as e:
        _lib.call(QUAT, None, None, 3, on=DEV0)                   # NULL pointers with M = 3: refused on the host
    assert QUAT in str(e.value)


def test_stub_sees_the_arguments_and_the_stream_last(stub):
    _lib.call(QUAT, None, 7, 0, on=DEV0)
    assert stub.entered == [(None, 7, 0, None)]


@pytest.mark.parametrize('args', [(None, None, 0, 0), (None, None)], ids=['one too many', 'one too few'])
def test_wrong_argument_count_is_refused_before_the_call(stub, args):
    with pytest.raises(TypeError) as e:
        _lib.call(QUAT, *args, on=DEV0)
    assert QUAT in str(e.value) and '3' in str(e.value) and str(len(args)) in str(e.value)
    assert stub.entered == []


def test_cpu_tensor_is_refused_before_the_call(stub):
    with pytest.raises(TypeError) as e:
        _lib.call(QUAT, torch.zeros(1, 4), None, 1, on=DEV0)
    with pytest.raises(TypeError) as need:
        _lib.need_cuda(torch.zeros(1))
    assert str(e.value) == str(need.value)
    with pytest.raises(TypeError):
        _lib.call(QUAT, None, None, 0, on=torch.zeros(1))
    assert stub.entered == []


def test_no_tensor_and_no_device_is_refused(stub):
    with pytest.raises(TypeError) as e:
        _lib.call(QUAT, None, None, 0)
    assert QUAT in str(e.value) and stub.entered == []


def test_unknown_entry_point():
    with pytest.raises(AttributeError):
        _lib.call('lasr_no_such_entry_point', None, on=DEV0)


def test_every_entry_point_the_package_names_takes_the_stream_last():
    # what call() relies on, for every entry point an operator names in a string (that is: hands to call())
    pkg = os.path.dirname(os.path.abspath(_lib.__file__))
    inc = os.path.join(os.path.dirname(pkg), 'include')
    text = ' '.join(open(os.path.join(inc, f)).read() for f in ('lasr_sr.h', 'lasr_ops.h'))
    text = re.sub(r'/\*.*?\*/|//[^\n]*', ' ', text, flags=re.S)
    last = {m.group(1): m.group(2).split(',')[-1].strip() for m in re.finditer(r'\bint\s+(lasr_\w+)\s*\(([^()]*)\)\s*;', text)}
    named = set()
    for d, _, files in os.walk(pkg):
        for f in files:
            if f.endswith('.py') and os.path.join(d, f) != os.path.abspath(_lib.__file__):
                named |= set(re.findall(r"'(lasr_\w+)'", open(os.path.join(d, f)).read()))
    named &= set(_lib.SIGNATURES)
    assert len(named) > 100 and named <= set(last)
    assert {n: last[n] for n in named if not re.fullmatch(r'void\s*\*\s*(hip_)?stream', last[n])} == {}


def test_f32():
    assert _lib.f32(None) is None
    x = torch.arange(12, dtype=torch.float64).reshape(3, 4).t()
    y = _lib.f32(x)
    assert not x.is_contiguous() and y.is_contiguous() and y.dtype == torch.float32 and torch.equal(y.double(), x)
    z = torch.ones(2, 3)
    assert _lib.f32(z) is z
    pair = _lib.f32(x, None)
    assert isinstance(pair, tuple) and len(pair) == 2 and pair[1] is None and torch.equal(pair[0], y)
