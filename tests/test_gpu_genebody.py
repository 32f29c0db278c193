"""-m gpu: --gene-body through the C ABI (rsqc_genebody_begin / rsqc_genebody_end / rsqc_genebody_sums, rnaseqc_amd/csrc/rsqc_genebody.hip).
The edge catalogue of tests/genebody_cases.py in one batch, in many small batches, with the later track events merged and lane by
lane, and under rsqc_sort_begin on shuffled records: sums and figures are compared, bit for bit, with the numpy restatement of the
contract (tests/genebody_ref.py)."""
import numpy as np
import pytest

from rnaseqc_amd import abi, engine
from rnaseqc_amd.model import Annotation
from tests import genebody_cases as gc
from tests import genebody_ref as ref
from tests import junction_cases as jc

pytestmark = pytest.mark.gpu

# an annotation the records of the catalogue do not touch: the per-read kernels see intergenic reads (this file is about the track)
ANN_ROWS = [dict(contig="c2", type="gene", start=2900, end=2999, strand="+", gene_id="g"), dict(contig="c2", type="exon", start=2900, end=2999, strand="+", gene_id="g")]
MODES = ["one_batch", "many_batches_lane_by_lane", "many_batches_merged", "shuffled_under_sort"]


@pytest.fixture(scope="module")
def one():
    """One context, reset between the passes."""
    e = engine.Engine(abi.default_params())
    e.set_annotation(Annotation.from_rows(["c0", "c1", "c2"], ANN_ROWS))
    yield e
    e.close()


def _batches(batches, mode):
    if mode == "one_batch" or not batches:
        return batches
    b = batches[0]
    if mode == "shuffled_under_sort":
        b = b.take(np.random.default_rng(77).permutation(b.n))
    cuts = jc.unequal_cuts(b.n, 11, min(7, b.n))
    return [b.slice(lo, hi) for lo, hi in zip(cuts[:-1], cuts[1:])]


def _pass(e, lengths, batches, model, sort=False, window=None):
    e.reset()
    if sort:
        e.sort_begin()
    e.track_begin(lengths)
    e.genebody_begin(**model)
    for b in batches:
        e.submit(b)
    if sort:
        e.sort_end()
    e.finalize()
    e.track_end()
    info = e.genebody_end()
    n = len(model["reverse"])
    step = window or max(n, 1)
    parts = [e.genebody_sums(k, min(step, n - k)) for k in range(0, n, step)]
    return (np.concatenate(parts) if parts else np.zeros((0, 100), np.uint64)), info


def _run_case(e, name, mode, monkeypatch):
    lengths, batches, model, _, want, want_info = gc.case(name)
    monkeypatch.setenv("RSQC_TRACK_MERGE", "0" if mode == "many_batches_lane_by_lane" else "1")
    got, info = _pass(e, lengths, _batches(batches, mode), model, sort=mode == "shuffled_under_sort", window=3 if mode == "many_batches_merged" else None)
    ref.assert_equal(got, info, want, want_info)
    assert (info["bins_ms"] > 0) == (want_info["n_measured"] > 0)          # (no measured gene: no launch)
    return got, info


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", gc.SMALL)
def test_catalogue(one, name, mode, monkeypatch):
    _run_case(one, name, mode, monkeypatch)


@pytest.mark.parametrize("mode", ["one_batch", "many_batches_lane_by_lane"])
def test_70000_genes_of_100(one, mode, monkeypatch):
    _run_case(one, "many_genes_of_100", mode, monkeypatch)


@pytest.mark.parametrize("mode", ["one_batch", "many_batches_merged"])
def test_bin_above_2_pow_32(one, mode, monkeypatch):
    """70 000 records 7000000M over one gene of 7 000 000 bases (a 28 MB array): every bin 4.9e9."""
    got, info = _run_case(one, "bin_above_2_pow_32", mode, monkeypatch)
    assert int(got[0].min()) == int(got[0].max()) == gc.BIG_RECORDS * (gc.BIG_L // 100) > 1 << 32


def test_second_end_reset_and_a_new_pass(one, monkeypatch):
    """A second rsqc_genebody_end returns the same figures (the event time included: no device work); after rsqc_reset the context
    takes another model over another track."""
    e = one
    got, info = _run_case(e, "item_edges", "one_batch", monkeypatch)
    assert e.genebody_end() == info
    assert (e.genebody_sums(0, len(got)) == got).all() and (e.genebody_sums(3, 1) == got[3:4]).all() and e.genebody_sums(len(got), 0).shape == (0, 100)
    with pytest.raises(engine.EngineError) as err:
        e.genebody_sums(len(got) - 1, 2)
    assert err.value.code == abi.ERR_ARG
    _run_case(e, "starts_at_zero_of_a_later_contig", "one_batch", monkeypatch)
    _run_case(e, "item_edges", "many_batches_merged", monkeypatch)
    e.reset()                                                              # a pass without the calls behind one with them: the mode has ended
    e.track_begin(gc.LENGTHS)
    e.finalize()
    e.track_end()
    with pytest.raises(engine.EngineError) as err:
        e.genebody_end()
    assert err.value.code == abi.ERR_ARG and "rsqc_genebody_begin must precede" in str(err.value)


@pytest.mark.parametrize("name", list(gc.BROKEN))
def test_every_model_rule_violated_once(one, name):
    model, word, gene = gc.broken_model(name)
    e = one
    e.reset()
    e.track_begin(gc.LENGTHS)
    with pytest.raises(engine.EngineError) as err:
        e.genebody_begin(**model)
    assert err.value.code == abi.ERR_ARG and word in str(err.value) and gene in str(err.value), str(err.value)
    _, _, good, _, _, _ = gc.case("no_records")                            # the refusal leaves the pass usable
    e.genebody_begin(**good)
    e.finalize()
    e.track_end()
    assert e.genebody_end()["n_measured"] == 2


def test_call_order():
    def refused(call, text, code=abi.ERR_ARG):
        with pytest.raises(engine.EngineError) as err:
            call()
        assert err.value.code == code and text in str(err.value), str(err.value)

    lengths, batches, model, _, want, want_info = gc.case("lengths_99_100_101_199")
    begin = lambda: e.genebody_begin(**model)
    e = engine.Engine(abi.default_params())
    try:
        e.set_annotation(Annotation.from_rows(["c0", "c1", "c2"], ANN_ROWS))
        refused(begin, "rsqc_track_begin")                                 # no track
        refused(e.genebody_end, "rsqc_genebody_begin must precede")
        e.track_begin(lengths)
        e.submit(batches[0])
        refused(begin, "first submit")                                     # behind a submit of the same pass
        e.reset()
        refused(begin, "rsqc_track_begin")                                 # the track of the pass before does not count
        e.track_begin(lengths)
        begin()
        refused(begin, "already")                                          # twice
        e.submit(batches[0])
        refused(e.genebody_end, "rsqc_track_end must precede")             # the pass is not finalized, the track not ended
        refused(lambda: e.genebody_sums(0, 1), "rsqc_genebody_end must precede")
        e.finalize()
        refused(e.genebody_end, "rsqc_track_end must precede")
        e.track_end()
        refused(begin, "rsqc_track_begin")                                 # behind rsqc_track_end
        info = e.genebody_end()
        ref.assert_equal(e.genebody_sums(0, 4), info, want, want_info)
    finally:
        e.close()
