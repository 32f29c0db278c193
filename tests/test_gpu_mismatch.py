"""-m gpu: rsqc_mismatch_* through the C ABI.  The catalogue (tests/mismatch_cases.py) goes through rsqc_decode_submit -- in one call, one
BGZF block per call, pipelined, with calls that end inside SEQ, QUAL and the CIGAR -- through rsqc_decode_submit_text and as BGZF SAM:
every route gives the tables of the Python restatement of the contract (tests/mismatch_ref.py), bit for bit, and so the same tables as
every other."""
import numpy as np
import pytest

from rnaseqc_amd import abi, bamio, engine, synth
from tests import mismatch_cases as mc
from tests import mismatch_ref as ref

pytestmark = pytest.mark.gpu

NAMES = [c[0] for c in mc.CONTIGS]
LENGTHS = [r[1] for r in mc.REFERENCE]
SEQS = [None if r[2] is None else r[2].encode() for r in mc.REFERENCE]


@pytest.fixture(scope="module")
def ann():
    # (genes on chrD only: the catalogue's records lie elsewhere, so no other stage's capacity is in the way of 140 000 reads of one name)
    return synth.make_annotation(seed=61, contigs=[("chrA", 21001, 0), ("chrB", 1003, 0), ("chrC", 500, 0), ("chrD", 500_000, 30)])


class Want:
    def __init__(self, tables):
        cyc, subst, byq, self.info = tables
        self.cyc, self.subst, self.byq = np.array(cyc, np.uint64), np.array(subst, np.uint64), np.array(byq, np.uint64)


@pytest.fixture(scope="module")
def want_bam():
    return Want(mc.catalogue_tables(True))


@pytest.fixture(scope="module")
def want_both():
    return Want(mc.catalogue_tables(False))


def _calls(pieces, per_call=None):
    """[(compressed bytes, block table)]: the pieces as BGZF payloads, per_call of them in every rsqc_decode_submit (None: all in one)."""
    blocks = [mc.bgzf_block(p)[1] for p in pieces]
    per_call = per_call or max(len(blocks), 1)
    out = []
    for a in range(0, len(blocks), per_call):
        comp, tab, at = b"", np.zeros(len(blocks[a:a + per_call]), bamio.BGZF_BLOCK), 0
        for k, (payload, isize, crc) in enumerate(blocks[a:a + per_call]):
            tab[k] = (at, len(payload), isize, crc, 0)
            comp += payload; at += len(payload)
        out.append((comp, tab))
    return out


def _engine(ann):
    e = engine.Engine(abi.default_params())
    e.set_annotation(ann)
    return e


def _bam_pass(e, calls, pipelined=False, seqs=SEQS, min_mapq=mc.MIN_MAPQ, cycles=False):
    e.mismatch_begin(LENGTHS, seqs, min_mapq)
    if cycles:
        e.cycles_begin()
    e.decode_begin(len(mc.CONTIGS), pipelined=pipelined)
    for comp, tab in calls:
        e.decode_submit(comp, tab)
    return e.decode_end()


def _sam_pass(e, feed, pipelined=False):
    e.mismatch_begin(LENGTHS, SEQS, mc.MIN_MAPQ)
    e.decode_begin(len(mc.CONTIGS), ref_names=NAMES, pipelined=pipelined)
    feed(e)
    return e.decode_end()


def _check(e, want, decode_info, n_records, timed=True):
    info, cyc, subst, byq = e.mismatch_end()
    assert decode_info[0] == n_records == info["seen_records"]
    assert {f: info[f] for f in ref.INFO_FIELDS} == want.info
    np.testing.assert_array_equal(cyc, want.cyc)
    np.testing.assert_array_equal(subst, want.subst)
    np.testing.assert_array_equal(byq, want.byq)
    assert not timed or info["mismatch_ms"] > 0
    again = e.mismatch_end()                                          # a second call: the same figures
    assert again[0] == info and all((a == b).all() for a, b in zip(again[1:], (cyc, subst, byq)))


@pytest.mark.parametrize("route", ["one_call", "one_block_per_call", "pipelined", "cut_in_seq_qual_and_cigar"])
def test_catalogue_as_bam(ann, want_bam, route):
    records = mc.catalogue(bam_only=True)
    stream, where = mc.bam_body(records)
    if route == "one_call":
        calls = _calls(mc.cut(stream))
    elif route == "one_block_per_call":
        calls = _calls(mc.cut(stream, block=613), 1)                  # (every record longer than 613 bytes straddles calls)
    elif route == "pipelined":
        calls = _calls(mc.cut(stream, block=4099), 3)
    else:
        # calls that end 2 bytes into the operations, 3 into SEQ and 5 into QUAL of records of several lengths and CIGARs (the record is
        # carried over and counted once, by the window that completes it), and one byte in front of a record's end
        cuts = []
        picks = [k for k, r in enumerate(records) if r[1] in ("len63_0", "len129_10", "len700_81", "len20000_91", "wide_0", "cgtag", "d_behind_i_10", "at64")]
        assert len(picks) == 8
        for k in picks:
            cuts += [where[k][1] + 2, where[k][2] + 3, where[k][3] + 5, where[k][4] - 1]
        calls = _calls(mc.cut(stream, cuts), 1)
        assert len(calls) > 30
    e = _engine(ann)
    try:
        _check(e, want_bam, _bam_pass(e, calls, pipelined=(route == "pipelined")), len(records))
    finally:
        e.close()


@pytest.mark.parametrize("route", ["text_one_call", "text_100_bytes", "text_pipelined", "bgzf", "bgzf_cut_in_seq"])
def test_catalogue_as_sam(ann, want_both, route):
    records = mc.catalogue()
    text = mc.sam_header() + mc.sam_body(records)
    if route.startswith("text"):
        step = {"text_one_call": len(text), "text_100_bytes": 100, "text_pipelined": 7001}[route]
        feed = lambda e: [e.decode_submit_text(text[a:a + step]) for a in range(0, len(text), step)]
    else:
        at = text.index(b"len700_0\t") + 200                          # inside the SEQ of a 700-base record
        pieces = mc.cut(text, [at, at + 700] if route == "bgzf_cut_in_seq" else (), block=0xFF00 if route == "bgzf" else 5003)
        calls = _calls(pieces, None if route == "bgzf" else 2)
        feed = lambda e: [e.decode_submit(comp, tab) for comp, tab in calls]
    e = _engine(ann)
    try:
        _check(e, want_both, _sam_pass(e, feed, pipelined=(route == "text_pipelined")), len(records))
    finally:
        e.close()


def test_both_spellings_agree_and_cycles_in_the_same_pass(ann, want_both):
    """The same alignments as BAM give what the SAM routes gave; --cycles in the same pass leaves both stages' tables as they are alone."""
    records = mc.catalogue()
    calls = _calls(mc.cut(mc.bam_body(records)[0], block=2999), 4)
    e = _engine(ann)
    try:
        _check(e, want_both, _bam_pass(e, calls), len(records))
        e.finalize(); e.reset()
        e.cycles_begin()
        e.decode_begin(len(mc.CONTIGS))
        for comp, tab in calls:
            e.decode_submit(comp, tab)
        e.decode_end()
        alone = e.cycles_end()
        e.finalize(); e.reset()
        _check(e, want_both, _bam_pass(e, calls, seqs=None, cycles=True), len(records))
        both = e.cycles_end()
        assert {k: v for k, v in both[0].items() if k != "cycles_ms"} == {k: v for k, v in alone[0].items() if k != "cycles_ms"}
        assert (both[1] == alone[1]).all() and (both[2] == alone[2]).all() and alone[0]["bases"] > 0
    finally:
        e.close()


def test_pile_up_and_empty_inputs(ann):
    """More than 65 535 in one cell inside one window, several workgroups flushing into one cell; then, after rsqc_reset, passes over
    nothing and over excluded records only start from zero, on the reference the context kept."""
    e = _engine(ann)
    try:
        records = mc.pileup()
        want = Want(ref.tables(records, mc.REFERENCE, 0))
        n0 = 70000 + 35000
        assert want.cyc[0, 1, ref.COMPARED] == n0 > 65535 and want.byq[30, 0] > 65535
        _check(e, want, _bam_pass(e, _calls(mc.cut(mc.bam_body(records)[0])), min_mapq=0), len(records))
        excluded = [(f,) + records[0][1:] for f in (0x4, 0x100, 0x200, 0x800)]
        for records in ([], excluded):
            e.finalize(); e.reset()
            info = _bam_pass(e, _calls(mc.cut(mc.bam_body(records)[0])), seqs=None)
            got, cyc, subst, byq = e.mismatch_end()
            assert info[0] == len(records) == got["seen_records"] and all(got[f] == 0 for f in ref.INFO_FIELDS if f != "seen_records")
            assert not cyc.any() and not subst.any() and not byq.any()
    finally:
        e.close()


def test_mixed_stream_a_second_pass_and_add(ann):
    """About 20 000 random records in windows of a few blocks; a second pass after rsqc_reset with sequence = NULL starts from zero on the
    kept reference; rsqc_mismatch_add of host tables adds exactly; NULL with other lengths is RSQC_ERR_ARG."""
    records, first_half, second_half, whole = mc.mixed_tables()
    want = Want(whole)
    assert want.info["records"] > 10000 and want.info["low_mapq_records"] > 1000 and want.info["no_reference_records"] > 1000
    stream, _ = mc.bam_body(records)
    e = _engine(ann)
    try:
        with pytest.raises(engine.EngineError) as err:               # nothing is kept yet
            e.mismatch_begin(LENGTHS, None)
        assert err.value.code == abi.ERR_ARG
        _check(e, want, _bam_pass(e, _calls(mc.cut(stream), 7)), len(records))
        e.finalize(); e.reset()
        for lengths in (LENGTHS[:2], LENGTHS[:2] + [501], LENGTHS + [7]):
            with pytest.raises(engine.EngineError) as err:
                e.mismatch_begin(lengths, None)
            assert err.value.code == abi.ERR_ARG and "differ" in str(err.value)
        half = len(records) // 2
        second = Want(second_half)
        info = _bam_pass(e, _calls(mc.cut(mc.bam_body(records[:half])[0]), 5), pipelined=True, seqs=None)
        assert info[0] == half
        e.mismatch_add(second.cyc, second.subst, second.byq, second.info)          # the other half, counted on the host
        e.mismatch_add(None, None, None, dict(seen_records=3, no_seq_records=3))
        got, cyc, subst, byq = e.mismatch_end()
        assert got["seen_records"] == len(records) + 3 and got["no_seq_records"] == want.info["no_seq_records"] + 3
        for f in ref.INFO_FIELDS:
            if f not in ("seen_records", "no_seq_records"):
                assert got[f] == want.info[f] == first_half[3][f] + second_half[3][f], f
        np.testing.assert_array_equal(cyc, want.cyc); np.testing.assert_array_equal(subst, want.subst); np.testing.assert_array_equal(byq, want.byq)
        with pytest.raises(engine.EngineError) as err:               # behind rsqc_mismatch_end nothing is added
            e.mismatch_add(second.cyc, second.subst, second.byq, second.info)
        assert err.value.code == abi.ERR_ARG
        # rsqc_clear_inputs frees the packed reference
        e.finalize(); e.clear_inputs(); e.set_annotation(ann)
        with pytest.raises(engine.EngineError) as err:
            e.mismatch_begin(LENGTHS, None)
        assert err.value.code == abi.ERR_ARG and "keeps no packed reference" in str(err.value)
    finally:
        e.close()


def test_call_order_and_min_mapq_zero(ann):
    records = mc.catalogue()
    calls = _calls(mc.cut(mc.bam_body(records)[0]))
    e = _engine(ann)
    try:
        # without rsqc_mismatch_begin: rsqc_mismatch_end and rsqc_mismatch_add are RSQC_ERR_ARG
        for call in (e.mismatch_end, lambda: e.mismatch_add(None, None, None, {})):
            with pytest.raises(engine.EngineError) as err:
                call()
            assert err.value.code == abi.ERR_ARG
        with pytest.raises(engine.EngineError) as err:
            e.mismatch_begin(LENGTHS, SEQS, 256)
        assert err.value.code == abi.ERR_ARG
        e.mismatch_begin(LENGTHS, SEQS, 0)
        with pytest.raises(engine.EngineError) as err:               # twice
            e.mismatch_begin(LENGTHS, SEQS, 0)
        assert err.value.code == abi.ERR_ARG
        e.decode_begin(len(mc.CONTIGS))
        with pytest.raises(engine.EngineError) as err:               # while the stream is open
            e.mismatch_end()
        assert err.value.code == abi.ERR_ARG and "rsqc_decode_end" in str(err.value)
        one = np.zeros((2, 512, 6), np.uint64); one[0, 0, 0] = 1
        with pytest.raises(engine.EngineError) as err:               # a table whose column sums are not partial's
            e.mismatch_add(one, None, None, dict(compared=2))
        assert err.value.code == abi.ERR_ARG
        for comp, tab in calls:
            e.decode_submit(comp, tab)
        e.decode_end()
        want = Want(ref.tables(records, mc.REFERENCE, 0))
        assert want.info["low_mapq_records"] == 0
        _check(e, want, (len(records),), len(records))
        e.finalize(); e.reset()
        e.decode_begin(len(mc.CONTIGS))
        with pytest.raises(engine.EngineError) as err:               # behind rsqc_decode_begin
            e.mismatch_begin(LENGTHS, None, 0)
        assert err.value.code == abi.ERR_ARG
        for comp, tab in calls:
            e.decode_submit(comp, tab)
        e.decode_end()
        with pytest.raises(engine.EngineError) as err:               # behind the pass's submits
            e.mismatch_begin(LENGTHS, None, 0)
        assert err.value.code == abi.ERR_ARG
    finally:
        e.close()
