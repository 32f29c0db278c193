"""-m gpu: the fragment-size stage K5 (rsqc_k5.h, host side rsqc_fragsize.hip) on the device at its bucket, select and table edges.
Every case of tests/k5_cases.py with a records form runs through the C ABI with a BED -- one contig, one exon over everything, a
coordinate-sorted hash-only batch in which record f is candidate f -- and is compared with the oracle and with walk(): once as one batch,
once as three unequal batches, so that file indices run across batches.  tests/test_k5_edges_host.py proves under the emulation, from the
exported plan, fills and paths, that each case sits on the edge it is named for; here the same candidates meet the real barriers, atomics,
launch rules and the host's read-back (the second read-back of more than 2 048 distinct sizes exists on the device only).

The RSQC_ERR_CAPACITY case (1 025 listed buckets) is a clean return: pair_bucket_scan_kernel stores a listed bucket only below PB_BIG_MAX,
and both *_replay_big_kernel clamp big[0] to it (read in rsqc_k5.h; the emulation checks the guard entry behind the list)."""
import functools

import numpy as np
import pytest

from rnaseqc_amd import abi, engine
from tests import k5_cases
from tests.compare import assert_results_match

pytestmark = pytest.mark.gpu

CASES = {c.name: c for c in k5_cases.cases() if c.device}


@functools.lru_cache(maxsize=None)
def _input(name):
    case = CASES[name]
    return k5_cases.annotation(case), k5_cases.bed(case), k5_cases.batch(case)


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """the oracle's results of a case, computed once for both batchings and left unchanged"""
    from oracle import binding
    ann, bed, b = _input(name)
    return binding.run_oracle(k5_cases.params(CASES[name]), ann, [b], bed=bed)


def _run(name, batches):
    case = CASES[name]
    ann, bed, _ = _input(name)
    p = k5_cases.params(case)
    if case.expect.get("error", 0):
        assert case.expect["error"] == abi.ERR_CAPACITY
        with pytest.raises(engine.EngineError) as err:                   # no partial result: the run ends with the error
            engine.run_engine(p, ann, batches, bed=bed)
        assert err.value.code == abi.ERR_CAPACITY
        return
    got = engine.run_engine(p, ann, batches, bed=bed)
    samples, kept, pairs = case.reference()
    np.testing.assert_array_equal(got.fragment_size, np.array([s for s, _ in pairs], np.int64))
    np.testing.assert_array_equal(got.fragment_count.astype(np.int64), np.array([c for _, c in pairs], np.int64))
    assert got.fragment_samples_remaining == case.max_samples - len(kept)
    assert len(kept) == case.expect.get("kept", len(kept)) and len(pairs) == case.expect.get("distinct", len(pairs))
    want = _oracle(name)
    assert_results_match(got, want)
    assert got.fragment_samples_remaining == want.fragment_samples_remaining


@pytest.mark.parametrize("name", list(CASES))
def test_one_batch(oracle_lib, name):
    _run(name, [_input(name)[2]])


@pytest.mark.parametrize("name", list(CASES))
def test_three_unequal_batches(oracle_lib, name):
    parts = k5_cases.three_batches(_input(name)[2])
    assert len(parts) == 3 and sum(b.n for b in parts) == CASES[name].n
    _run(name, parts)
