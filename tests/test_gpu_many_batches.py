"""-m gpu: the end of a --bed / --fasta file with MANY batches in flight (bench.py's resident batches, a host that enqueues faster than
the device runs).  rsqc_finalize then retires all of them into the arenas first -- device-to-device copies of the fragment-size
candidates queued on the main stream BEHIND the fork event -- and the fragment-size stage runs beside the other end-of-file kernels on
a side stream: it has to wait for those copies (rsqc_finalize.cpp: ev_retired).  32 ragged batches, submitted back to back
with no wait in between, host-fed and in the resident form of bench.py; everything equals the oracle on the whole input.

(The other order -- the stage BEHIND the end-of-file kernels, taken when the candidate arena must grow while it holds retired batches --
is out of a quick test's reach: an arena starts at 2^24 entries, rsqc_submit.cpp:arena_reserve.  Every case here runs `beside`.)"""
import numpy as np
import pytest

from rnaseqc_amd import abi, engine, synth
from tests.compare import assert_results_match

pytestmark = pytest.mark.gpu

N_BATCHES = 32
LENGTHS = np.array([600_000, 300_000])


@pytest.fixture(scope="module")
def inputs():
    ann = synth.make_annotation(seed=8, contigs=[("chrA", 600_000, 60), ("chrB", 300_000, 30)])
    bed = synth.make_bed(ann, min_len=250)
    assert len(bed.contig) >= 10
    batch = synth.make_reads(ann, 60000, seed=10, frac=(0.9, 0.04, 0.03, 0.03), expr_sigma=1.0, contig_lengths=LENGTHS)
    rng = np.random.default_rng(3)
    cuts = np.unique(np.concatenate([rng.integers(1, batch.n, N_BATCHES - 3), [7, 64 * 900 + 1]]))      # ragged: a 7-record batch, 200 to 9 000
    cuts = [0] + [int(x) for x in cuts if x % 64] + [batch.n]
    parts = [batch.slice(lo, hi) for lo, hi in zip(cuts[:-1], cuts[1:])]
    assert 28 <= len(parts) <= N_BATCHES and sum(b.n for b in parts) == batch.n
    ref = synth.make_reference(LENGTHS, seed=11)
    return ann, bed, ref, batch, parts


@pytest.fixture(scope="module")
def wants(oracle_lib, inputs):
    ann, bed, ref, batch, _ = inputs
    cache = {}

    def want(samples, with_bed, with_ref):
        key = (samples, with_bed, with_ref)
        if key not in cache:
            cache[key] = oracle_lib.run_oracle(abi.default_params(fragment_samples=samples), ann, [batch], bed=bed if with_bed else None,
                                               reference=ref if with_ref else None)
        return cache[key]
    return want


def _check(got, want):
    assert_results_match(got, want)
    assert got.fragment_samples_remaining == want.fragment_samples_remaining


@pytest.mark.parametrize("samples,with_bed,with_ref", [(1000000, True, False), (100, True, False), (1000000, True, True),
                                                       (100, True, True), (1000000, False, True)])
def test_many_batches_submitted_back_to_back(inputs, wants, samples, with_bed, with_ref):
    ann, bed, ref, batch, parts = inputs
    want = wants(samples, with_bed, with_ref)
    if with_bed:
        assert int(want.fragment_count.sum()) == (100 if samples == 100 else int(want.fragment_count.sum())) and int(want.fragment_count.sum()) >= 100
    if with_ref:
        assert int(np.asarray(want.gc_bins).sum()) > 1000
    e = engine.Engine(abi.default_params(fragment_samples=samples))
    try:
        e.set_annotation(ann)
        if with_bed:
            e.set_bed(bed)
        if with_ref:
            e.set_reference(ref)
        for b in parts:
            e.submit(b)                       # (no wait: the batches are in flight when finalize begins)
        _check(e.finalize(), want)
        assert e.timing()["classify_records"] == batch.n
    finally:
        e.close()


@pytest.mark.parametrize("samples", [1000000, 100])
def test_resident_batches_three_passes(inputs, wants, samples):
    """bench.py's form: every batch uploaded once, then reset / submit_resident x 32 / finalize, three times over."""
    ann, bed, ref, batch, parts = inputs
    want = wants(samples, True, True)
    e = engine.Engine(abi.default_params(fragment_samples=samples))
    try:
        e.set_annotation(ann); e.set_bed(bed); e.set_reference(ref)
        handles = [e.upload(b) for b in parts]
        for _ in range(3):
            e.reset()
            for h in handles:
                e.submit_resident(h)
            _check(e.finalize(), want)
    finally:
        e.close()
