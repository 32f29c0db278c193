"""-m gpu: rsqc_cycles_* through the C ABI.  The catalogue (tests/cycle_cases.py) goes through rsqc_decode_submit -- in one call, in many
small calls that cut records inside SEQ and inside QUAL, pipelined -- through rsqc_decode_submit_text and as BGZF SAM: every route gives
the tables of the Python restatement of the contract (tests/cycle_ref.py), bit for bit, and so the same tables as every other."""
import numpy as np
import pytest

from rnaseqc_amd import abi, bamio, engine, synth
from tests import cycle_cases as cc
from tests import cycle_ref as ref
from tests.compare import assert_results_match

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ann():
    # (genes on chrB only: the catalogue's records all lie on chrA, so no other stage's capacity is in the way of 140 000 reads of one name)
    return synth.make_annotation(seed=61, contigs=[("chrA", 1_000_000, 0), ("chrB", 500_000, 30)])


class Want:
    def __init__(self, records, tables=None):
        base, qual, self.info = tables or ref.tables(records)
        self.base, self.qual = np.array(base, np.uint64), np.array(qual, np.uint64)


@pytest.fixture(scope="module")
def want_bam():
    return Want(cc.catalogue(bam_only=True))


@pytest.fixture(scope="module")
def want_both():
    return Want(cc.catalogue())


def _calls(pieces, per_call=None):
    """[(compressed bytes, block table)]: the pieces as BGZF payloads, per_call of them in every rsqc_decode_submit (None: all in one)."""
    blocks = [cc.bgzf_block(p)[1] for p in pieces]
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


def _bam_pass(e, calls, pipelined=False, cycles=True):
    if cycles:
        e.cycles_begin()
    e.decode_begin(len(cc.CONTIGS), pipelined=pipelined)
    for comp, tab in calls:
        e.decode_submit(comp, tab)
    return e.decode_end()


def _sam_pass(e, feed, pipelined=False):
    e.cycles_begin()
    e.decode_begin(len(cc.CONTIGS), ref_names=[c[0] for c in cc.CONTIGS], pipelined=pipelined)
    feed(e)
    return e.decode_end()


def _check(e, want, decode_info, n_records):
    info, base, qual = e.cycles_end()
    assert decode_info[0] == n_records == info["seen_records"]
    assert {f: info[f] for f in ref.INFO_FIELDS} == want.info
    np.testing.assert_array_equal(base, want.base)
    np.testing.assert_array_equal(qual, want.qual)
    assert info["cycles_ms"] > 0
    again = e.cycles_end()                                            # a second call: the same figures
    assert again[0] == info and (again[1] == base).all() and (again[2] == qual).all()


@pytest.mark.parametrize("route", ["one_call", "one_block_per_call", "pipelined", "cut_in_seq_and_qual"])
def test_catalogue_as_bam(ann, want_bam, route):
    records = cc.catalogue(bam_only=True)
    stream, where = cc.bam_body(records)
    if route == "one_call":
        calls = _calls(cc.cut(stream))
    elif route == "one_block_per_call":
        calls = _calls(cc.cut(stream, block=613), 1)                  # (every record longer than 613 bytes straddles calls; so do SEQ and QUAL of many)
    elif route == "pipelined":
        calls = _calls(cc.cut(stream, block=4099), 3)
    else:
        # calls that end 3 bytes into SEQ and 5 bytes into QUAL of records of several lengths (the record is carried over and counted
        # once, by the window that completes it), and one byte in front of a record's end
        cuts = []
        for k in (17, 30, 45, 61, 69, len(records) - 2):            # L = 63, 127, 256, 513, 20 000, 16
            cuts += [where[k][1] + 3, where[k][2] + 5, where[k][3] - 1]
        calls = _calls(cc.cut(stream, cuts), 1)
        assert len(calls) > 18
    e = _engine(ann)
    try:
        _check(e, want_bam, _bam_pass(e, calls, pipelined=(route == "pipelined")), len(records))
    finally:
        e.close()


@pytest.mark.parametrize("route", ["text_one_call", "text_100_bytes", "text_pipelined", "bgzf", "bgzf_cut_in_seq"])
def test_catalogue_as_sam(ann, want_both, want_bam, route):
    records = cc.catalogue()
    text = cc.sam_header() + cc.sam_body(records)
    if route.startswith("text"):
        step = {"text_one_call": len(text), "text_100_bytes": 100, "text_pipelined": 7001}[route]
        feed = lambda e: [e.decode_submit_text(text[a:a + step]) for a in range(0, len(text), step)]
    else:
        at = text.index(b"len700_0\t") + 200                          # inside the SEQ of a 700-base record
        pieces = cc.cut(text, [at, at + 700] if route == "bgzf_cut_in_seq" else (), block=0xFF00 if route == "bgzf" else 5003)
        calls = _calls(pieces, None if route == "bgzf" else 2)
        feed = lambda e: [e.decode_submit(comp, tab) for comp, tab in calls]
    e = _engine(ann)
    try:
        _check(e, want_both, _sam_pass(e, feed, pipelined=(route == "text_pipelined")), len(records))
    finally:
        e.close()


def test_both_spellings_agree_on_the_device(ann, want_both):
    """The same alignments as BAM give what the SAM routes gave (the reference's tables of the catalogue without its BAM-only records)."""
    records = cc.catalogue()
    e = _engine(ann)
    try:
        _check(e, want_both, _bam_pass(e, _calls(cc.cut(cc.bam_body(records)[0], block=2999), 4)), len(records))
    finally:
        e.close()


def test_pile_up_and_empty_inputs(ann):
    """More than 65 535 in one cell inside one window; then, after rsqc_reset, passes over nothing and over excluded records only start
    from zero."""
    e = _engine(ann)
    try:
        records = cc.pileup()
        _check(e, Want(records), _bam_pass(e, _calls(cc.cut(cc.bam_body(records)[0]))), len(records))
        for records in ([], cc.excluded_only()):
            e.finalize(); e.reset()
            want = Want(records)
            assert want.info["bases"] == 0
            info = _bam_pass(e, _calls(cc.cut(cc.bam_body(records)[0])))
            got, base, qual = e.cycles_end()
            assert info[0] == len(records) == got["seen_records"] and {f: got[f] for f in ref.INFO_FIELDS} == want.info
            assert not base.any() and not qual.any()
    finally:
        e.close()


def test_mixed_stream_totals_and_a_second_pass(ann):
    """About 20 000 random records in windows of a few blocks; a second pass after rsqc_reset + rsqc_cycles_begin starts from zero;
    rsqc_cycles_add of a host table adds exactly."""
    records, first_half, second_half, whole = cc.mixed_tables()
    want = Want(records, whole)
    stream, _ = cc.bam_body(records)
    calls = _calls(cc.cut(stream), 7)
    e = _engine(ann)
    try:
        _check(e, want, _bam_pass(e, calls), len(records))
        e.finalize(); e.reset()
        half = len(records) // 2
        first, second = Want(None, first_half), Want(None, second_half)
        info = _bam_pass(e, _calls(cc.cut(cc.bam_body(records[:half])[0]), 5), pipelined=True)
        assert info[0] == half
        e.cycles_add(second.base, second.qual, second.info)          # the other half, counted on the host
        e.cycles_add(None, None, dict(seen_records=3, no_seq_records=3))
        got, base, qual = e.cycles_end()
        assert got["seen_records"] == len(records) + 3 and got["no_seq_records"] == want.info["no_seq_records"] + 3
        for f in ("records", "no_qual_records", "bases", "beyond_bases", "clamped_quals"):
            assert got[f] == want.info[f] == first.info[f] + second.info[f], f
        np.testing.assert_array_equal(base, want.base)
        np.testing.assert_array_equal(qual, want.qual)
        with pytest.raises(engine.EngineError) as err:               # behind rsqc_cycles_end nothing is added
            e.cycles_add(second.base, second.qual, second.info)
        assert err.value.code == abi.ERR_ARG
    finally:
        e.close()


def test_without_the_mode_and_call_order(ann, want_both):
    records = cc.catalogue()
    calls = _calls(cc.cut(cc.bam_body(records)[0]))
    plain, counted = _engine(ann), _engine(ann)
    try:
        # a pass without rsqc_cycles_begin: rsqc_cycles_end and rsqc_cycles_add are RSQC_ERR_ARG, and the pass is what it is with the mode on
        _bam_pass(plain, calls, cycles=False)
        for call in (plain.cycles_end, lambda: plain.cycles_add(None, None, {})):
            with pytest.raises(engine.EngineError) as err:
                call()
            assert err.value.code == abi.ERR_ARG
        _check(counted, want_both, _bam_pass(counted, calls), len(records))
        assert_results_match(plain.finalize(), counted.finalize())
        # call order: twice; behind rsqc_decode_begin; behind the pass's first submit; rsqc_cycles_end while the stream is open;
        # rsqc_cycles_add of a table whose sum is not partial->bases
        e = plain
        e.reset()
        e.cycles_begin()
        with pytest.raises(engine.EngineError) as err:
            e.cycles_begin()
        assert err.value.code == abi.ERR_ARG
        e.decode_begin(len(cc.CONTIGS))
        with pytest.raises(engine.EngineError) as err:
            e.cycles_end()
        assert err.value.code == abi.ERR_ARG and "rsqc_decode_end" in str(err.value)
        one = np.zeros((2, 512, 5), np.uint64); one[0, 0, 0] = 1
        with pytest.raises(engine.EngineError) as err:
            e.cycles_add(one, None, dict(bases=2))
        assert err.value.code == abi.ERR_ARG
        for comp, tab in calls:
            e.decode_submit(comp, tab)
        e.decode_end()
        _check(e, want_both, (len(records),), len(records))
        e.finalize(); e.reset()
        e.decode_begin(len(cc.CONTIGS))
        with pytest.raises(engine.EngineError) as err:
            e.cycles_begin()
        assert err.value.code == abi.ERR_ARG
        for comp, tab in calls:
            e.decode_submit(comp, tab)
        e.decode_end()
        with pytest.raises(engine.EngineError) as err:               # behind the pass's submits
            e.cycles_begin()
        assert err.value.code == abi.ERR_ARG
    finally:
        plain.close(); counted.close()
