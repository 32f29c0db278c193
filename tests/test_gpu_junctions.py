"""-m gpu: --junctions through the C ABI (rsqc_junctions_begin / rsqc_junctions_end, rnaseqc_amd/csrc/rsqc_junction.hip).  The table
of every pass is compared, row for row, with the Python restatement of the contract (tests/junction_ref.py); rsqc_results of a pass
with the calls equal those of the same pass without them."""
import numpy as np
import pytest

from rnaseqc_amd import abi, engine, synth
from rnaseqc_amd.model import Batch
from tests import junction_cases as jc
from tests import junction_ref as ref
from tests.compare import assert_results_match

pytestmark = pytest.mark.gpu


def _pass(p, ann, batches, junctions=True, sort=None, bed=None, resident=False):
    """One pass; sort: None, "sort_first" or "junctions_first" (the order of the two begins).  Returns (results, table or None)."""
    e = engine.Engine(p)
    try:
        e.set_annotation(ann)
        if bed is not None:
            e.set_bed(bed)
        if sort == "sort_first":
            e.sort_begin()
        if junctions:
            e.junctions_begin()
        if sort == "junctions_first":
            e.sort_begin()
        for b in batches:
            if resident:
                e.submit_resident(e.upload(b))
            else:
                e.submit(b)
        if sort:
            e.sort_end()
        res = e.finalize()
        return res, (e.junctions_end() if junctions else None)
    finally:
        e.close()


@pytest.fixture(scope="module")
def fix():
    class F:
        pass
    f = F()
    f.ann, f.reads = jc.fixture_a()
    f.parts = jc.cut(f.reads)
    f.want = jc.fixture_a_table()
    f.p = abi.default_params()
    f.plain, _ = _pass(f.p, f.ann, f.parts, junctions=False)
    return f


def test_fixture_a_in_five_batches(fix):
    res, got = _pass(fix.p, fix.ann, fix.parts)
    ref.assert_tables_equal(got, fix.want)
    assert got["extract_ms"] > 0 and got["sort_ms"] > 0 and got["reduce_ms"] > 0
    assert_results_match(res, fix.plain)                  # the calls change no other output


def test_growth_of_the_collection(fix, monkeypatch):
    """RSQC_JUNCTION_CAP0 = 1024: four growth steps for these five batches (tests/junction_cases.py), each with instances to carry over."""
    monkeypatch.setenv("RSQC_JUNCTION_CAP0", "1024")
    res, got = _pass(fix.p, fix.ann, fix.parts)
    ref.assert_tables_equal(got, fix.want)
    assert_results_match(res, fix.plain)


@pytest.mark.parametrize("order", ["sort_first", "junctions_first"])
def test_shuffled_records_under_sort(fix, order):
    """The instances are taken from the sorted output batches; the table is that of the records in any order."""
    srt = fix.reads.coordinate_sorted()
    shuffled = srt.take(np.random.default_rng(54).permutation(srt.n))
    want_res, _ = _pass(fix.p, fix.ann, [srt], junctions=False)
    res, got = _pass(fix.p, fix.ann, jc.cut(shuffled, seed=3, parts=4), sort=order)
    ref.assert_tables_equal(got, fix.want)
    assert_results_match(res, want_res)


def test_resident_batch(fix):
    res, got = _pass(fix.p, fix.ann, [fix.reads], resident=True)
    ref.assert_tables_equal(got, fix.want)
    assert_results_match(res, fix.plain)


def test_one_batch_of_several_file_ranges(fix):
    s = fix.reads.coordinate_sorted()
    parts = [s.slice(int(s.seg_start[k]), int(s.seg_start[k + 1])) for k in range(len(s.seg_tid))]
    one = Batch.concat_ranges(parts)
    assert one.seg_file_index is not None and len(one.seg_file_index) >= 3
    _, got = _pass(fix.p, fix.ann, [one])
    ref.assert_tables_equal(got, fix.want)


def test_bed_and_legacy_do_not_change_the_table(fix):
    bed = synth.make_bed(fix.ann, min_len=250)
    p_bed = abi.default_params(fragment_samples=150)
    res, got = _pass(p_bed, fix.ann, fix.parts, bed=bed)
    ref.assert_tables_equal(got, fix.want)
    assert_results_match(res, _pass(p_bed, fix.ann, fix.parts, junctions=False, bed=bed)[0])
    p_leg = abi.default_params(legacy=1)
    res, got = _pass(p_leg, fix.ann, fix.parts)
    ref.assert_tables_equal(got, fix.want)
    assert_results_match(res, _pass(p_leg, fix.ann, fix.parts, junctions=False)[0])


@pytest.fixture(scope="module")
def engines(fix):
    """One context per mapping-quality threshold, reset between the crafted cases."""
    es = {}
    for q in (255, 4):
        es[q] = engine.Engine(abi.default_params(mapq_threshold=q))
        es[q].set_annotation(fix.ann)
    yield es
    for e in es.values():
        e.close()


@pytest.mark.parametrize("name", jc.CRAFTED_NAMES)
def test_crafted(engines, name):
    b, q, want = jc.crafted_case(name)
    e = engines[q]
    e.reset()
    e.junctions_begin()
    e.submit(b)
    e.finalize()
    ref.assert_tables_equal(e.junctions_end(), want)


def test_reset_then_a_second_pass_over_other_records(fix):
    b, _, want = jc.crafted_case("run_across_workgroups")
    e = engine.Engine(fix.p)
    try:
        e.set_annotation(fix.ann)
        e.junctions_begin()
        for part in fix.parts:
            e.submit(part)
        e.finalize()
        first = e.junctions_end()
        ref.assert_tables_equal(first, fix.want)
        e.reset()
        e.junctions_begin()
        e.submit(b)
        e.finalize()
        second = e.junctions_end()
        ref.assert_tables_equal(second, want)              # the second pass's alone
        again = e.junctions_end()                          # a second call: the same table
        ref.assert_tables_equal(again, want)
        assert (again["extract_ms"], again["sort_ms"], again["reduce_ms"]) == (second["extract_ms"], second["sort_ms"], second["reduce_ms"])
        e.reset()                                          # a pass without the calls behind one with them: the mode has ended
        for part in fix.parts:
            e.submit(part)
        assert_results_match(e.finalize(), fix.plain)
        with pytest.raises(engine.EngineError) as err:
            e.junctions_end()
        assert err.value.code == abi.ERR_ARG
    finally:
        e.close()


def test_call_order_errors(fix):
    def refused(call, text):
        with pytest.raises(engine.EngineError) as err:
            call()
        assert err.value.code == abi.ERR_ARG and text in str(err.value), str(err.value)

    e = engine.Engine(fix.p)
    try:
        refused(e.junctions_begin, "rsqc_set_annotation")              # no annotation
        e.set_annotation(fix.ann)
        refused(e.junctions_end, "rsqc_junctions_begin must precede")  # not begun
        e.submit(fix.parts[0])
        refused(e.junctions_begin, "first submit")                     # behind a submit of the same pass
        e.reset()
        e.junctions_begin()
        refused(e.junctions_begin, "already")                          # twice
        e.submit(fix.parts[0])
        refused(e.junctions_end, "rsqc_finalize")                      # the pass is not finalized
        e.finalize()
        refused(e.junctions_begin, "rsqc_reset")                       # behind rsqc_finalize
        t = e.junctions_end()
        ref.assert_tables_equal(t, ref.junction_table([fix.parts[0]], jc.N_CONTIGS, 255))
    finally:
        e.close()
