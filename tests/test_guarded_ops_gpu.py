"""Every operator of tests/guarded_cases.py with guard-banded, poisoned outputs and scratch (tests/guarded.py): nothing is written
outside an allocation, no result depends on what memory held before the call, and the natives reached are the declared ones.
The deliberately wrong operators of tests/guarded_fakes.py run on the device too; their stray writes stay inside the guarded
buffer's own bands.  Every operator runs once more with its INPUTS in tight, poisoned copies (guarded.run_relocated): no read
past a tensor it is given reaches a result, no write lands beside one."""
import pytest

import guarded
import guarded_cases
import guarded_fakes

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('case', guarded_cases.CASES, ids=[c.name for c in guarded_cases.CASES])
def test_operator_under_guard_bands_and_two_poisons(cuda, case):
    guarded.run_case(case, cuda)


@pytest.mark.parametrize('case', guarded_cases.CASES, ids=[c.name for c in guarded_cases.CASES])
def test_operator_with_relocated_inputs(cuda, case):
    guarded.run_relocated(case, cuda, not_relocated=guarded_cases.NOT_RELOCATED)


def _fake(cuda, name, relocated=None):
    mod, lib = guarded_fakes.make()
    if name in guarded_fakes.RELOCATED_MODE if relocated is None else relocated:
        return guarded.run_relocated(guarded_fakes.cases(mod)[name], cuda, modules=[mod], lib=lib)
    guarded.run_case(guarded_fakes.cases(mod)[name], cuda, modules=[mod], lib=lib)


def test_a_clean_fake_operator_passes_on_the_device(cuda):
    _fake(cuda, 'clean')


@pytest.mark.parametrize('name', sorted(guarded_fakes.EXPECTED))
def test_a_wrong_fake_operator_is_caught_on_the_device(cuda, name):
    with pytest.raises(AssertionError) as e:
        _fake(cuda, name)
    assert guarded_fakes.EXPECTED[name] in str(e.value), str(e.value)


@pytest.mark.parametrize('name', guarded_fakes.CLEAN)
def test_a_clean_fake_operator_passes_with_relocated_inputs_on_the_device(cuda, name):
    record = _fake(cuda, name, relocated=True)
    assert sum(r['args'] for r in record.values()) == {'clean': 1, 'inout': 2, 'alias': 2}[name]
    assert sum(r['bytes'] for r in record.values()) == 33 * 4 * {'clean': 1, 'inout': 2, 'alias': 1}[name]
