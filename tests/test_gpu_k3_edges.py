"""-m gpu: K3, the end-of-file coverage stage, on the device at its class, depth and window edges.  Every case of tests/k3_cases.py runs
through the C ABI with the library's own launch plan (rsqc_k3_plan.h) against the oracle: once as one batch, once cut into three unequal
batches, so that the difference array is built by several launches of the per-record kernel, with the pad slots and the exon-end decrements
of a gene landing across batches.  The cases that end in the reference's range_error end in ERR_EMPTY_MEDIAN here."""
import functools

import pytest

from rnaseqc_amd import abi, engine
from tests import k3_cases
from tests.compare import assert_results_match

pytestmark = pytest.mark.gpu

CASE_NAMES = [c.name for c in k3_cases.CASES]


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """The oracle's results of a case, computed once for both batchings and left unchanged; ERR_EMPTY_MEDIAN for the error cases."""
    from oracle import binding
    case = k3_cases.CASE_BY_NAME[name]
    try:
        return binding.run_oracle(case.params(), case.input.ann, [case.input.batch])
    except binding.OracleError as e:
        return e.code


def _run(name, batches):
    case = k3_cases.CASE_BY_NAME[name]
    want = _oracle(name)
    if case.error:
        assert want == abi.ERR_EMPTY_MEDIAN
        with pytest.raises(engine.EngineError) as err:
            engine.run_engine(case.params(), case.input.ann, batches)
        assert err.value.code == abi.ERR_EMPTY_MEDIAN
        return
    assert not isinstance(want, int), want
    assert_results_match(engine.run_engine(case.params(), case.input.ann, batches), want)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_one_batch(oracle_lib, name):
    _run(name, [k3_cases.CASE_BY_NAME[name].input.batch])


@pytest.mark.parametrize("name", CASE_NAMES)
def test_three_unequal_batches(oracle_lib, name):
    parts = k3_cases.three_batches(k3_cases.CASE_BY_NAME[name].input.batch)
    assert len(parts) == 3 and len({b.n for b in parts}) == 3 and sum(b.n for b in parts) == k3_cases.CASE_BY_NAME[name].input.batch.n
    _run(name, parts)
