"""-m gpu: --mark-duplicates through the C ABI (rsqc_markdup_begin / rsqc_markdup_end / rsqc_markdup_verdicts,
rnaseqc_amd/csrc/rsqc_markdup.hip).  Verdicts and figures of every collection are compared, bit for bit, with the Python restatement
of the contract (tests/markdup_ref.py); rsqc_results of a marked pass equal those of a plain sorted pass over the same records with
their flags rewritten by the reference."""
import numpy as np
import pytest

from rnaseqc_amd import abi, engine, synth
from tests import markdup_cases as mc
from tests import markdup_ref as ref
from tests.compare import assert_results_match

pytestmark = pytest.mark.gpu

CONTIGS = [("chrA", 900_000, 70), ("chrB", 500_000, 40), ("chrC", 300_000, 15)]


@pytest.fixture(scope="module")
def ann():
    return synth.make_annotation(seed=51, contigs=CONTIGS)


@pytest.fixture(scope="module")
def eng(ann):
    """One context, reset between the collections."""
    e = engine.Engine(abi.default_params())
    e.set_annotation(ann)
    yield e
    e.close()


def _mark(e, batches, extra=None):
    """sort_begin, markdup_begin, the batches, sort_end: (verdicts, info, sort info).  The pass is left open (not finalized)."""
    e.reset()
    e.sort_begin()
    if extra == "junctions_first":
        e.junctions_begin()
    e.markdup_begin()
    if extra == "junctions_last":
        e.junctions_begin()
    for b in batches:
        e.submit(b)
    sinfo = e.sort_end()
    info = e.markdup_end()
    n = int(info["records"])
    v = np.concatenate([e.markdup_verdicts(0, n // 3), e.markdup_verdicts(n // 3, n - n // 3)]) if n else e.markdup_verdicts(0, 0)
    return v, info, sinfo


def _check(e, batches, want_v, want_info, **kw):
    v, info, sinfo = _mark(e, batches, **kw)
    ref.assert_info_equal(info, want_info)
    np.testing.assert_array_equal(v, want_v)
    assert sinfo["records"] == want_info["records"]
    return info


@pytest.mark.parametrize("name", mc.CRAFTED_NAMES)
def test_crafted(eng, name):
    b, v, info = mc.crafted_case(name)
    _check(eng, [b], v, info)


def test_crafted_all_in_one_pass(eng):
    batches = [mc.crafted_case(n)[0] for n in mc.CRAFTED_NAMES if n != "names_collide_without_qhash2"]
    v, info, _ = ref.mark_duplicates(batches)
    _check(eng, batches, v, info)


def test_fixture_cuts_and_order(eng):
    """One batch, five unequal batches, a shuffle in three: each against the reference on that arrival order; the order-independent
    figures agree across the three."""
    v, info, _ = mc.fixture_expected()
    one = _check(eng, [mc.fixture()], v, info)
    five = _check(eng, mc.cut(mc.fixture(), mc.FIXTURE_CUTS), v, info, extra="junctions_first")
    parts, (v2, info2, _) = mc.fixture_shuffled()
    three = _check(eng, parts, v2, info2, extra="junctions_last")
    for f in ref.ORDER_FREE_FIELDS:
        assert one[f] == five[f] == three[f], f
    assert one["sig_ms"] > 0 and one["sort_ms"] > 0 and one["mark_ms"] > 0
    again = eng.markdup_end()                              # a second call: the same figures
    assert again == three


def _sorted_results(ann, batches, mark):
    e = engine.Engine(abi.default_params())
    try:
        e.set_annotation(ann)
        e.sort_begin()
        if mark:
            e.markdup_begin()
        for b in batches:
            e.submit(b)
        e.sort_end()
        return e.finalize()
    finally:
        e.close()


def test_results_equal_a_sorted_pass_over_rewritten_flags(ann):
    """Every counter and every gene vector: the marked pass against a plain --sort pass over the records as the reference flags them;
    and the plain pass over the records as they arrive says something else (the flags the input carries are random)."""
    parts = mc.cut(mc.fixture(), mc.FIXTURE_CUTS)
    v, info, _ = mc.fixture_expected()
    got = _sorted_results(ann, parts, mark=True)
    want = _sorted_results(ann, ref.rewrite_flags(parts, v), mark=False)
    assert_results_match(got, want)
    plain = _sorted_results(ann, parts, mark=False)
    k = abi.COUNTER_NAMES.index("Mapped Duplicate Reads")
    assert int(got.counters[k]) == int(want.counters[k]) > 0 and int(plain.counters[k]) != int(got.counters[k])


def test_call_order_errors(ann):
    def refused(call, text):
        with pytest.raises(engine.EngineError) as err:
            call()
        assert err.value.code == abi.ERR_ARG and text in str(err.value), str(err.value)

    b, v, info = mc.crafted_case("survivor_set_of_3")
    e = engine.Engine(abi.default_params())
    try:
        e.set_annotation(ann)
        refused(e.markdup_begin, "rsqc_sort_begin must precede")           # no collection
        refused(e.markdup_end, "rsqc_markdup_begin must precede")          # not begun
        refused(lambda: e.markdup_verdicts(0, 0), "must precede")
        e.sort_begin()
        e.submit(b)
        refused(e.markdup_begin, "first submit")                          # behind a submit of the same pass
        e.reset()
        e.sort_begin()
        e.markdup_begin()
        refused(e.markdup_begin, "already")                                # twice
        e.submit(b)
        refused(e.markdup_end, "rsqc_sort_end must precede")               # the stage has not run
        refused(lambda: e.markdup_verdicts(0, 1), "must precede")
        e.sort_end()
        ref.assert_info_equal(e.markdup_end(), info)
        np.testing.assert_array_equal(e.markdup_verdicts(0, b.n), v)
        np.testing.assert_array_equal(e.markdup_verdicts(2, 3), v[2:5])
        refused(lambda: e.markdup_verdicts(1, b.n), "rows")                # past the collection
        e.finalize()
        ref.assert_info_equal(e.markdup_end(), info)                       # still there behind rsqc_finalize
        e.reset()                                                          # the mode has ended
        refused(e.markdup_end, "rsqc_markdup_begin must precede")
        e.sort_begin()                                                     # a plain sorted pass behind a marked one
        e.submit(b)
        e.sort_end()
        refused(e.markdup_end, "rsqc_markdup_begin must precede")
        e.finalize()
    finally:
        e.close()


def test_empty_collection(eng):
    v, info, _ = _mark(eng, [])
    assert len(v) == 0 and all(int(info[f]) == 0 for f in ref.INFO_FIELDS)
