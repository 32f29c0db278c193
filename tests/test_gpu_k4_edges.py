"""-m gpu: the fragment count (rsqc_k4.h: frag_layout / frag_local / frag_count) on the device at its partition, set and window edges.
Every case of tests/k4_cases.py that can be said as records runs through the C ABI -- one single-exon gene per gene index, one unpaired
one-block read per (gene, key, h2) pair, the hashes written directly (a hash-only batch) -- and is compared with the oracle and with the
Python sets: once as one batch (the chunks of the per-record kernel + its dense region), once as three unequal batches (retired into the
dense arena).  tests/test_k4_edges_host.py proves under the emulation, from the exported plan and fills, that each case sits on the edge
it is named for; here the same pairs meet the real barriers, atomics and launch rules.

The RSQC_ERR_CAPACITY cases are clean returns: frag_local_kernel stores only below a list's capacity, frag_count_kernel clamps a fill to
it and the set-aside list to its 32 entries (read in rsqc_k4.h; the emulation checks that no list entry outside a partition's clamped fill
is written).  The case of 65 537 genes stays with the emulation (k4_cases.py says why)."""
import functools

import numpy as np
import pytest

from rnaseqc_amd import abi, engine
from tests import k4_cases
from tests.compare import assert_results_match

pytestmark = pytest.mark.gpu

CASES = {c.name: c for c in k4_cases.cases() if c.device}
CHUNK_SHAPED = [(c.name, g) for c in CASES.values() for g in c.k1_grids]
LEGACY_CASE = "instance_partitions_of_1_32_33_64_1024_1025_2047_2048_keys"


@functools.lru_cache(maxsize=None)
def _input(name):
    case = CASES[name]
    return k4_cases.annotation(case), k4_cases.batch(case)


@functools.lru_cache(maxsize=None)
def _oracle(name, legacy=0):
    """the oracle's results of a case, computed once for every batching and grid and left unchanged"""
    from oracle import binding
    ann, b = _input(name)
    return binding.run_oracle(k4_cases.params(legacy=legacy), ann, [b])


def _run(name, batches, legacy=0):
    case = CASES[name]
    ann, b = _input(name)
    p = k4_cases.params(legacy=legacy)
    if case.expect.get("error", 0):
        assert case.expect["error"] == abi.ERR_CAPACITY
        with pytest.raises(engine.EngineError) as err:
            engine.run_engine(p, ann, batches)
        assert err.value.code == abi.ERR_CAPACITY
        return
    want = _oracle(name, legacy)
    got = engine.run_engine(p, ann, batches)
    np.testing.assert_array_equal(got.gene_reads.astype(np.int64), case.reads)
    np.testing.assert_array_equal(got.gene_fragments.astype(np.int64), case.reference())
    assert_results_match(got, want)


@pytest.mark.parametrize("name", list(CASES))
def test_one_batch(oracle_lib, name):
    _run(name, [_input(name)[1]])


@pytest.mark.parametrize("name", list(CASES))
def test_three_unequal_batches(oracle_lib, name):
    parts = k4_cases.three_batches(_input(name)[1])
    assert len(parts) == 3 and sum(b.n for b in parts) == len(CASES[name].gene)
    _run(name, parts)


@pytest.mark.parametrize("name,grid", CHUNK_SHAPED)
def test_chunk_shaped_case_with_few_workgroups(oracle_lib, monkeypatch, name, grid):
    """RSQC_K1_GRID = 1, 2, 3 (read by rsqc_create): the per-record kernel leaves one to three long chunks, so that a workgroup of
    frag_local_kernel runs several passes over a two-chunk run and the window carries across the seam."""
    monkeypatch.setenv("RSQC_K1_GRID", str(grid))
    _run(name, [_input(name)[1]])


def test_multi_partition_case_under_legacy_rules(oracle_lib):
    """--legacy: all pairs of a batch sit in its dense region, whose sharers follow another launch rule (rsqc_finalize.cpp)"""
    _run(LEGACY_CASE, [_input(LEGACY_CASE)[1]], legacy=1)
    _run(LEGACY_CASE, k4_cases.three_batches(_input(LEGACY_CASE)[1]), legacy=1)
