"""-m gpu: the register path of K3, the end-of-file coverage stage, on the device: the cases of tests/test_k3_register_passes_host.py that
records can express -- round edges (coding lengths of exactly k rounds of T x 16 bases and one more, the maximum in the last lane of the
last round, or in base 0 with an equal one behind it), cancellation at 60 000x (180 k one-block reads), the trim against the sums folded
into the scan, exons cut by the mask, the window medians -- as ONE annotation of a dozen genes through the C ABI against the
oracle, once as one batch and once cut into three unequal batches."""
import functools

import numpy as np
import pytest

from rnaseqc_amd import abi, engine
from tests import k3_cases
from tests import test_k3_register_passes_host as host
from tests.compare import assert_results_match

pytestmark = pytest.mark.gpu

# mask 50, the default window of 100 at offset 0; 127 (odd) takes the other branch of computeMedian in the windows
PARAMS = (dict(coverage_mask=50), dict(coverage_mask=50, bias_window=127))


def _genes():
    rounds = [g for g in host._round_edges() if g[0] in ("r1024l", "r1025f", "r2048f", "r2049l", "r4096l", "r4097f", "r8192f", "r8193l")]
    return rounds + host._bump() + host._trim(300) + host._trim(101) + host._exon_mask() + host._exon_rounds(65) + host._median_genes()[:2]


@functools.lru_cache(maxsize=None)
def _input():
    inp = k3_cases.build_input([k3_cases.Gene(n, ex, st, profile=prof) for n, ex, st, prof in _genes()])
    assert len(inp.genes) == 15 and 180_000 <= inp.n_reads <= 230_000
    return inp


@functools.lru_cache(maxsize=None)
def _oracle(k):
    """The oracle's results, computed once for both batchings and left unchanged."""
    from oracle import binding
    return binding.run_oracle(abi.default_params(unpaired=1, **PARAMS[k]), _input().ann, [_input().batch])


def _check(k, batches):
    p = abi.default_params(unpaired=1, **PARAMS[k])
    got, want = engine.run_engine(p, _input().ann, batches), _oracle(k)
    assert_results_match(got, want)
    np.testing.assert_array_equal(got.bias_three, want.bias_three)
    np.testing.assert_array_equal(got.bias_five, want.bias_five)
    np.testing.assert_array_equal(got.exon_cv_valid, want.exon_cv_valid)
    # the expectations of the CPU file, from exact integer sums, on the device's results too
    case = host.Case("device", _genes(), PARAMS[k])
    want_m = [host.model(prof, ex, st, p) for _, ex, st, prof in case.genes]
    assert sum(m["three"] > 0 for m in want_m) == 11                           # the bias path ran where it is meant to
    host.check_against_model(case, lambda f, g: getattr(got, f)[g], lambda f, r: getattr(got, f)[r], want_m)
    bump = [g[0] for g in case.genes].index("bump")
    row = sum(len(g[1]) for g in case.genes[:bump])
    np.testing.assert_allclose(got.exon_cv[row + 1], np.sqrt(1949.0) / 1950.0 / (host.DEEP + 1 / 1950.0), rtol=1e-9, atol=0)   # (the mask leaves 1 950 of its bases)
    assert got.exon_cv[row] == 0.0                                              # a flat exon at 60 000x: exactly 0


@pytest.mark.parametrize("k", range(len(PARAMS)))
def test_one_batch(oracle_lib, k):
    _check(k, [_input().batch])


@pytest.mark.parametrize("k", range(len(PARAMS)))
def test_three_unequal_batches(oracle_lib, k):
    parts = k3_cases.three_batches(_input().batch)
    assert len(parts) == 3 and sum(b.n for b in parts) == _input().batch.n
    _check(k, parts)
