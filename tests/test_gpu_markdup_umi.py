"""-m gpu: UMI-aware duplicate marking through the C ABI (rsqc_markdup_use_umi / rsqc_markdup_umi_end, rsqc_batch.umi;
rnaseqc_amd/csrc/rsqc_markdup.hip).  Verdicts and figures of every collection are compared, bit for bit, with the Python restatement
of the contract (tests/markdup_umi_ref.py); rsqc_results of a UMI-marked pass equal those of a plain sorted pass over the same records
with their flags rewritten by the reference; without rsqc_markdup_use_umi the column is ignored."""
import copy

import numpy as np
import pytest

from rnaseqc_amd import abi, engine, synth
from tests import markdup_cases as mc
from tests import markdup_ref as ref
from tests import markdup_umi_cases as uc
from tests import markdup_umi_ref as uref
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


def _mark(e, batches, use_umi=True):
    """(verdicts, info, umi info or None).  The pass is left open (not finalized)."""
    e.reset()
    e.sort_begin()
    e.markdup_begin()
    if use_umi:
        e.markdup_use_umi()
    for b in batches:
        e.submit(b)
    e.sort_end()
    info = e.markdup_end()
    n = int(info["records"])
    v = np.concatenate([e.markdup_verdicts(0, n // 3), e.markdup_verdicts(n // 3, n - n // 3)]) if n else e.markdup_verdicts(0, 0)
    return v, info, (e.markdup_umi_end() if use_umi else None)


def _check(e, batches, want_v, want_info, want_umi):
    v, info, uinfo = _mark(e, batches)
    ref.assert_info_equal(info, want_info)
    uref.assert_umi_info_equal(uinfo, want_umi)
    np.testing.assert_array_equal(v, want_v)
    return info, uinfo


def test_library_exports_the_abi_7_symbols():
    assert abi.ABI_VERSION == 7
    for sym in ("rsqc_markdup_use_umi", "rsqc_markdup_umi_end", "rsqc_umi_pack"):
        assert sym in engine.EXPORTED_SYMBOLS and getattr(engine.load_library(), sym)


@pytest.mark.parametrize("name", uc.CRAFTED_NAMES)
def test_crafted(eng, name):
    batches, v, info, uinfo = uc.crafted_case(name)
    _check(eng, batches, v, info, uinfo)


def test_crafted_all_in_one_pass(eng):
    batches = [b for n in uc.CRAFTED_NAMES for b in uc.crafted_case(n)[0]]
    v, info, uinfo, _ = uref.mark_duplicates_umi(batches)
    _check(eng, batches, v, info, uinfo)


def test_fixture_cuts_and_order(eng):
    """One batch, five unequal batches, a shuffle in three: each against the reference on that arrival order; the order-free figures
    agree across the three; a second rsqc_markdup_umi_end returns the same figures."""
    v, info, uinfo, _ = uc.fixture_expected()
    one, u1 = _check(eng, [uc.fixture()], v, info, uinfo)
    five, u5 = _check(eng, mc.cut(uc.fixture(), uc.FIXTURE_CUTS), v, info, uinfo)
    parts, (v2, info2, uinfo2, _) = uc.fixture_shuffled()
    three, u3 = _check(eng, parts, v2, info2, uinfo2)
    for f in ref.ORDER_FREE_FIELDS:
        assert one[f] == five[f] == three[f], f
    assert u1 == u5 == u3
    assert eng.markdup_umi_end() == u3 and eng.markdup_end() == three


def _sorted_results(ann, batches, mark, use_umi=False):
    e = engine.Engine(abi.default_params())
    try:
        e.set_annotation(ann)
        e.sort_begin()
        if mark:
            e.markdup_begin()
        if use_umi:
            e.markdup_use_umi()
        for b in batches:
            e.submit(b)
        e.sort_end()
        return e.finalize()
    finally:
        e.close()


def test_results_equal_a_sorted_pass_over_rewritten_flags(ann):
    parts = mc.cut(uc.fixture(), uc.FIXTURE_CUTS)
    v, info, uinfo, _ = uc.fixture_expected()
    got = _sorted_results(ann, parts, mark=True, use_umi=True)
    want = _sorted_results(ann, ref.rewrite_flags(parts, v), mark=False)
    assert_results_match(got, want)
    # ... and the position-only marking of the same records says something else
    position = _sorted_results(ann, parts, mark=True)
    k = abi.COUNTER_NAMES.index("Mapped Duplicate Reads")
    assert 0 < int(got.counters[k]) == int(want.counters[k]) < int(position.counters[k])


def test_without_use_umi_the_column_is_ignored(eng):
    """The umi column present, rsqc_markdup_use_umi not called: plain --mark-duplicates, bit for bit -- the same as without the column."""
    parts = mc.cut(uc.fixture(), uc.FIXTURE_CUTS)
    bare = []
    for p in parts:
        q = copy.copy(p); q.umi = None
        bare.append(q)
    want_v, want_info, _ = ref.mark_duplicates(parts)
    v1, info1, _ = _mark(eng, parts, use_umi=False)
    v0, info0, _ = _mark(eng, bare, use_umi=False)
    ref.assert_info_equal(info1, want_info)
    np.testing.assert_array_equal(v1, want_v)
    np.testing.assert_array_equal(v0, v1)
    ref.assert_info_equal(info0, info1)
    with pytest.raises(engine.EngineError) as err:                  # ... and no UMI figures exist for such a pass
        eng.markdup_umi_end()
    assert err.value.code == abi.ERR_ARG


def test_a_batch_without_the_column_is_refused_and_changes_nothing(eng):
    parts = mc.cut(uc.fixture(), uc.FIXTURE_CUTS)
    v, info, uinfo, _ = uc.fixture_expected()
    bare = copy.copy(parts[2]); bare.umi = None
    eng.reset()
    eng.sort_begin(); eng.markdup_begin(); eng.markdup_use_umi()
    with pytest.raises(engine.EngineError) as err:                  # as the pass's FIRST batch: nothing of it stays behind either
        eng.submit(bare)
    assert err.value.code == abi.ERR_ARG and "rsqc_batch.umi" in str(err.value)
    for k, p in enumerate(parts):
        if k == 2:
            with pytest.raises(engine.EngineError) as err:
                eng.submit(bare)
            assert err.value.code == abi.ERR_ARG
        eng.submit(p)
    eng.sort_end()
    ref.assert_info_equal(eng.markdup_end(), info)                  # the refused batches left the collection as it was
    uref.assert_umi_info_equal(eng.markdup_umi_end(), uinfo)
    np.testing.assert_array_equal(eng.markdup_verdicts(0, info["records"]), v)
    # a later complete pass on the same context is correct
    _check(eng, parts, v, info, uinfo)


def test_call_order_errors(ann):
    def refused(call, text):
        with pytest.raises(engine.EngineError) as err:
            call()
        assert err.value.code == abi.ERR_ARG and text in str(err.value), str(err.value)

    batches, v, info, uinfo = uc.crafted_case("mapq_interleaved_with_other_umi")
    e = engine.Engine(abi.default_params())
    try:
        e.set_annotation(ann)
        refused(e.markdup_use_umi, "rsqc_markdup_begin must precede")     # no collection, no marking
        e.sort_begin()
        refused(e.markdup_use_umi, "rsqc_markdup_begin must precede")     # collecting, not marking
        e.markdup_begin()
        e.submit(batches[0])
        refused(e.markdup_use_umi, "first submit")                        # behind the pass's first submit
        e.reset()
        e.sort_begin(); e.markdup_begin(); e.markdup_use_umi()
        e.submit(batches[0])
        refused(e.markdup_umi_end, "rsqc_sort_end must precede")
        e.sort_end()
        uref.assert_umi_info_equal(e.markdup_umi_end(), uinfo)
        ref.assert_info_equal(e.markdup_end(), info)
        e.finalize()
        uref.assert_umi_info_equal(e.markdup_umi_end(), uinfo)            # still there behind rsqc_finalize
        e.reset()                                                         # the mode has ended
        refused(e.markdup_umi_end, "rsqc_markdup_use_umi must precede")
        e.sort_begin(); e.markdup_begin()                                 # a plain marked pass behind a UMI one: the column is not asked for
        bare = copy.copy(batches[0]); bare.umi = None
        e.submit(bare)
        e.sort_end()
        assert e.markdup_end()["duplicate_fragments"] == uinfo["position_duplicate_fragments"]
        e.finalize()
    finally:
        e.close()
