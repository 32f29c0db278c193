"""-m gpu: UMIs one substitution apart grouped before duplicate marking, through the C ABI (rsqc_markdup_umi_edits /
rsqc_markdup_umi_group_end; rnaseqc_amd/csrc/rsqc_markdup.hip).  Verdicts and figures of every collection are compared, bit for bit, with
the Python restatement of the contract (tests/markdup_umi_group_ref.py); with max_edits 0, or without the call, the pass is
markdup_umi_ref's; rsqc_results of a grouped pass equal those of a plain sorted pass over the same records with their flags rewritten by
the reference."""
import numpy as np
import pytest

from rnaseqc_amd import abi, engine, synth
from tests import markdup_cases as mc
from tests import markdup_ref as ref
from tests import markdup_umi_cases as uc
from tests import markdup_umi_group_cases as gc
from tests import markdup_umi_group_ref as gref
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


def _mark(e, batches, edits=1):
    """(verdicts, info, umi info, group info or None).  edits None: rsqc_markdup_umi_edits is not called.  The pass is left open."""
    e.reset()
    e.sort_begin()
    e.markdup_begin()
    e.markdup_use_umi()
    if edits is not None:
        e.markdup_umi_edits(edits)
    for b in batches:
        e.submit(b)
    e.sort_end()
    info = e.markdup_end()
    n = int(info["records"])
    v = np.concatenate([e.markdup_verdicts(0, n // 3), e.markdup_verdicts(n // 3, n - n // 3)]) if n else e.markdup_verdicts(0, 0)
    return v, info, e.markdup_umi_end(), (e.markdup_umi_group_end() if edits == 1 else None)


def _check(e, batches, want):
    want_v, want_info, want_umi, want_group = want[:4]
    v, info, uinfo, ginfo = _mark(e, batches)
    ref.assert_info_equal(info, want_info)
    uref.assert_umi_info_equal(uinfo, want_umi)
    gref.assert_group_info_equal(ginfo, want_group)
    np.testing.assert_array_equal(v, want_v)
    assert ginfo["group_ms"] >= 0.0
    return info, uinfo, ginfo


def test_library_exports_the_new_symbols_and_the_abi_is_still_7():
    assert abi.ABI_VERSION == 7
    for sym in ("rsqc_markdup_umi_edits", "rsqc_markdup_umi_group_end"):
        assert sym in engine.EXPORTED_SYMBOLS and getattr(engine.load_library(), sym)


@pytest.mark.parametrize("name", gc.CRAFTED_NAMES)
def test_crafted(eng, name):
    batches, *want = gc.crafted_case(name)
    _check(eng, batches, want)


def test_crafted_all_in_one_pass(eng):
    batches = [b for n in gc.CRAFTED_NAMES for b in gc.crafted_case(n)[0]]
    _check(eng, batches, gref.mark_duplicates_umi_group(batches))


def test_fixture_cuts_and_order(eng):
    """One batch, five unequal batches, a shuffle in three: each against the reference on that arrival order; the order-free figures
    agree across the three; a second rsqc_markdup_umi_group_end returns the same figures."""
    want = gc.fixture_expected()
    one = _check(eng, [gc.fixture()], want)
    five = _check(eng, mc.cut(gc.fixture(), gc.FIXTURE_CUTS), want)
    parts, shuffled = gc.fixture_shuffled()
    three = _check(eng, parts, shuffled)
    for f in ref.ORDER_FREE_FIELDS:
        assert one[0][f] == five[0][f] == three[0][f], f
    assert one[1] == five[1] == three[1]
    for f in gref.GROUP_FIELDS:
        assert one[2][f] == five[2][f] == three[2][f], f
    assert one[2]["merged_nodes"] > 0 and one[0]["duplicate_fragments"] < one[1]["position_duplicate_fragments"]
    assert eng.markdup_umi_group_end() == three[2] and eng.markdup_umi_end() == three[1] and eng.markdup_end() == three[0]


@pytest.mark.parametrize("edits", [0, None], ids=["edits_0", "no_call"])
def test_without_the_mode_the_pass_is_exact(eng, edits):
    """rsqc_markdup_umi_edits(0) and no call at all: exactly markdup_umi_ref's result, on the grouping fixture (where grouping would
    merge) and on a crafted case; no group figures exist for such a pass."""
    for batches in (mc.cut(gc.fixture(), gc.FIXTURE_CUTS), gc.crafted_case("chain_9_5_3")[0]):
        want_v, want_info, want_umi, _ = uref.mark_duplicates_umi(batches)
        v, info, uinfo, _ = _mark(eng, batches, edits=edits)
        ref.assert_info_equal(info, want_info)
        uref.assert_umi_info_equal(uinfo, want_umi)
        np.testing.assert_array_equal(v, want_v)
        with pytest.raises(engine.EngineError) as err:
            eng.markdup_umi_group_end()
        assert err.value.code == abi.ERR_ARG
        assert gref.mark_duplicates_umi_group(batches)[1]["duplicate_fragments"] > want_info["duplicate_fragments"]      # grouping WOULD have changed it


def _sorted_results(ann, batches, mark, edits=None):
    e = engine.Engine(abi.default_params())
    try:
        e.set_annotation(ann)
        e.sort_begin()
        if mark:
            e.markdup_begin(); e.markdup_use_umi()
            if edits is not None:
                e.markdup_umi_edits(edits)
        for b in batches:
            e.submit(b)
        e.sort_end()
        return e.finalize()
    finally:
        e.close()


def test_results_equal_a_sorted_pass_over_rewritten_flags(ann):
    parts = mc.cut(gc.fixture(), gc.FIXTURE_CUTS)
    v = gc.fixture_expected()[0]
    got = _sorted_results(ann, parts, mark=True, edits=1)
    want = _sorted_results(ann, ref.rewrite_flags(parts, v), mark=False)
    assert_results_match(got, want)
    # ... and exact matching of the same records flags fewer
    exact = _sorted_results(ann, parts, mark=True)
    k = abi.COUNTER_NAMES.index("Mapped Duplicate Reads")
    assert int(got.counters[k]) == int(want.counters[k]) > int(exact.counters[k]) > 0


def test_call_order_errors(ann):
    def refused(call, text):
        with pytest.raises(engine.EngineError) as err:
            call()
        assert err.value.code == abi.ERR_ARG and text in str(err.value), str(err.value)

    batches, v, info, uinfo, ginfo, _roots = gc.crafted_case("threshold_3_2")
    ev, einfo, euinfo, _ = uref.mark_duplicates_umi(batches)
    e = engine.Engine(abi.default_params())
    try:
        e.set_annotation(ann)
        refused(lambda: e.markdup_umi_edits(1), "rsqc_markdup_use_umi must precede")      # no collection, no marking
        e.sort_begin(); e.markdup_begin()
        refused(lambda: e.markdup_umi_edits(1), "rsqc_markdup_use_umi must precede")      # marking, without the UMI
        e.markdup_use_umi()
        refused(lambda: e.markdup_umi_edits(2), "0 or 1")
        refused(lambda: e.markdup_umi_edits(0xFFFFFFFF), "0 or 1")
        e.submit(batches[0])
        refused(lambda: e.markdup_umi_edits(1), "first submit")                           # behind the pass's first submit
        e.sort_end()                                                                      # ... so this pass is exact
        refused(e.markdup_umi_group_end, "rsqc_markdup_umi_edits(1) must precede")
        ref.assert_info_equal(e.markdup_end(), einfo)
        e.reset()
        e.sort_begin(); e.markdup_begin(); e.markdup_use_umi(); e.markdup_umi_edits(1)
        e.submit(batches[0])
        refused(e.markdup_umi_group_end, "rsqc_sort_end must precede")
        e.sort_end()
        first = e.markdup_umi_group_end()
        gref.assert_group_info_equal(first, ginfo)
        ref.assert_info_equal(e.markdup_end(), info)
        e.finalize()
        assert e.markdup_umi_group_end() == first                                         # a second call, behind rsqc_finalize: the same figures
        e.reset()                                                                         # the mode has ended ...
        refused(e.markdup_umi_group_end, "rsqc_markdup_umi_edits(1) must precede")
        e.sort_begin(); e.markdup_begin(); e.markdup_use_umi()                            # ... and the next pass is exact again
        e.submit(batches[0])
        e.sort_end()
        ref.assert_info_equal(e.markdup_end(), einfo)
        uref.assert_umi_info_equal(e.markdup_umi_end(), euinfo)
        np.testing.assert_array_equal(e.markdup_verdicts(0, einfo["records"]), ev)
        assert einfo["sets"] == 2 and info["sets"] == 1
        e.finalize()
    finally:
        e.close()
