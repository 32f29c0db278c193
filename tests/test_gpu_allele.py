"""-m gpu: rsqc_alleles_* through the C ABI.  The catalogue (tests/allele_cases.py) goes through rsqc_decode_submit -- in one call, one BGZF
block per call, pipelined, with calls that end inside SEQ, QUAL and the CIGAR -- through rsqc_decode_submit_text and as BGZF SAM: every
route gives the table of the Python restatement of the contract (tests/allele_ref.py), bit for bit, and so the same table as every other."""
import numpy as np
import pytest

from rnaseqc_amd import abi, bamio, engine, synth
from tests import allele_cases as ac
from tests import allele_ref as ref
from tests import mismatch_cases as mc

pytestmark = pytest.mark.gpu

Q, BQ = ac.MIN_MAPQ, ac.MIN_BASEQ


@pytest.fixture(autouse=True, params=["0", "1"], ids=["plain", "merge"])
def form(request, monkeypatch):
    """Both forms of the kernel: an atomic per observation, and merged across the wave first (read at rsqc_alleles_begin)."""
    monkeypatch.setenv("RSQC_ALLELE_MERGE", request.param)


@pytest.fixture(scope="module")
def ann():
    # (genes on chrD only: the pile-up's records lie elsewhere, so no other stage's capacity is in the way of 140 000 reads of one name)
    return synth.make_annotation(seed=61, contigs=[("chrA", 21001, 0), ("chrB", 1003, 0), ("chrC", 500, 0), ("chrD", 500_000, 30)])


class Want:
    def __init__(self, tables):
        counts, self.info = tables
        self.counts = np.array(counts, np.uint64).reshape(len(counts), ref.COLS)


def _calls(pieces, per_call=None):
    """[(compressed bytes, block table)]: the pieces as BGZF payloads, per_call of them in every rsqc_decode_submit (None: all in one)."""
    blocks = [ac.bgzf_block(p)[1] for p in pieces]
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


def _begin(e, sites, min_mapq=Q, min_baseq=BQ):
    e.alleles_begin(ac.N_CONTIGS, [s[0] for s in sites], [s[1] for s in sites], min_mapq, min_baseq)


def _bam_pass(e, calls, sites=ac.SITES, pipelined=False, min_mapq=Q, min_baseq=BQ, others=False):
    _begin(e, sites, min_mapq, min_baseq)
    if others:
        e.cycles_begin()
        e.mismatch_begin([r[1] for r in mc.REFERENCE], [None if r[2] is None else r[2].encode() for r in mc.REFERENCE], Q)
    e.decode_begin(ac.N_CONTIGS, pipelined=pipelined)
    for comp, tab in calls:
        e.decode_submit(comp, tab)
    return e.decode_end()


def _sam_pass(e, feed, pipelined=False):
    _begin(e, ac.SITES)
    e.decode_begin(ac.N_CONTIGS, ref_names=ac.NAMES, pipelined=pipelined)
    feed(e)
    return e.decode_end()


def _check(e, want, decode_info, n_records, timed=True):
    info, counts = e.alleles_end()
    assert decode_info[0] == n_records == info["seen_records"]
    assert {f: info[f] for f in ref.INFO_FIELDS} == dict(want.info, seen_records=n_records)
    np.testing.assert_array_equal(counts, want.counts)
    assert not timed or info["alleles_ms"] > 0
    again = e.alleles_end()                                           # a second call: the same figures
    assert again[0] == info and (again[1] == counts).all()


@pytest.mark.parametrize("route", ["one_call", "one_block_per_call", "pipelined", "cut_in_seq_qual_and_cigar"])
def test_catalogue_as_bam(ann, route):
    records = ac.catalogue(bam_only=True)
    stream, where = ac.bam_body(records)
    if route == "one_call":
        calls = _calls(ac.cut(stream))
    elif route == "one_block_per_call":
        calls = _calls(ac.cut(stream, block=613), 1)                  # (every record longer than 613 bytes straddles calls)
    elif route == "pipelined":
        calls = _calls(ac.cut(stream, block=4099), 3)
    else:
        # calls that end 2 bytes into the operations, 3 into SEQ and 5 into QUAL of chosen records (the record is carried over and counted
        # once, by the window that completes it), and one byte in front of a record's end
        cuts = []
        picks = [k for k, r in enumerate(records) if r[1] in ("edge_M_0", "long_20000", "wide_0", "cgtag", "d_mid", "adjacent_65", "n_skips_1000", "far")]
        assert len(picks) == 8
        for k in picks:
            cuts += [where[k][1] + 2, where[k][2] + 3, where[k][3] + 5, where[k][4] - 1]
        calls = _calls(ac.cut(stream, cuts), 1)
        assert len(calls) > 30
    e = _engine(ann)
    try:
        _check(e, Want(ac.catalogue_tables(True)), _bam_pass(e, calls, pipelined=(route == "pipelined")), len(records))
    finally:
        e.close()


@pytest.mark.parametrize("route", ["text_100_bytes", "text_7001_bytes_pipelined", "bgzf"])
def test_catalogue_as_sam(ann, route):
    records = ac.catalogue() + ac.sam_only_qualities()
    want = Want(ref.tables(records, ac.N_CONTIGS, ac.SITES, Q, BQ))
    text = ac.sam_header() + ac.sam_body(records)
    if route.startswith("text"):
        step = 100 if route == "text_100_bytes" else 7001
        feed = lambda e: [e.decode_submit_text(text[a:a + step]) for a in range(0, len(text), step)]
    else:
        calls = _calls(ac.cut(text, block=5003), 2)
        feed = lambda e: [e.decode_submit(comp, tab) for comp, tab in calls]
    e = _engine(ann)
    try:
        _check(e, want, _sam_pass(e, feed, pipelined=route.endswith("pipelined")), len(records))
    finally:
        e.close()


def test_both_spellings_agree_and_the_other_stages_in_the_same_pass(ann):
    """The same alignments as BAM give what the SAM routes gave; --cycles and --mismatches in the same pass leave all three stages' tables
    as they are alone."""
    records = ac.catalogue()
    want = Want(ac.catalogue_tables(False))
    calls = _calls(ac.cut(ac.bam_body(records)[0], block=2999), 4)
    lengths, seqs = [r[1] for r in mc.REFERENCE], [None if r[2] is None else r[2].encode() for r in mc.REFERENCE]
    e = _engine(ann)
    try:
        _check(e, want, _bam_pass(e, calls), len(records))
        e.finalize(); e.reset()
        e.cycles_begin(); e.mismatch_begin(lengths, seqs, Q)
        e.decode_begin(ac.N_CONTIGS)
        for comp, tab in calls:
            e.decode_submit(comp, tab)
        e.decode_end()
        cyc_alone, mm_alone = e.cycles_end(), e.mismatch_end()
        e.finalize(); e.reset()
        _check(e, want, _bam_pass(e, calls, others=True), len(records))
        cyc_both, mm_both = e.cycles_end(), e.mismatch_end()
        for both, alone, ms in ((cyc_both, cyc_alone, "cycles_ms"), (mm_both, mm_alone, "mismatch_ms")):
            assert {k: v for k, v in both[0].items() if k != ms} == {k: v for k, v in alone[0].items() if k != ms}
            assert all((a == b).all() for a, b in zip(both[1:], alone[1:]))
        assert cyc_alone[0]["bases"] > 0 and mm_alone[0]["compared"] > 0
    finally:
        e.close()


@pytest.mark.parametrize("sites", ["empty", "one", "two", "no_first", "no_middle"])
def test_the_tables_edges(ann, sites):
    records = ac.catalogue(bam_only=True)
    e = _engine(ann)
    try:
        info = _bam_pass(e, _calls(ac.cut(ac.bam_body(records)[0])), sites=ac.site_lists()[sites])
        _check(e, Want(ac.catalogue_tables(True, sites)), info, len(records))
    finally:
        e.close()


def test_pile_up_and_empty_inputs(ann):
    """More than 65 535 in one cell inside one window, several workgroups adding to it; then, after rsqc_reset, passes over nothing and
    over excluded records only start from zero."""
    e = _engine(ann)
    try:
        records = ac.pileup()
        want = Want(ref.tables(records, ac.N_CONTIGS, ac.PILE_SITES, 0, 0))
        assert want.counts[0].tolist() == [0, 70000, 0, 70000, 0, 0, 0] and want.counts[3, ref.DELETED] == 140000 == want.counts[1, ref.G]
        _check(e, want, _bam_pass(e, _calls(ac.cut(ac.bam_body(records)[0])), sites=ac.PILE_SITES, min_mapq=0, min_baseq=0), len(records))
        excluded = [(f,) + records[0][1:] for f in (0x4, 0x100, 0x200, 0x800)]
        for records in ([], excluded):
            e.finalize(); e.reset()
            info = _bam_pass(e, _calls(ac.cut(ac.bam_body(records)[0])), sites=ac.PILE_SITES)
            got, counts = e.alleles_end()
            assert info[0] == len(records) == got["seen_records"] and got["n_sites"] == 5 and all(got[f] == 0 for f in ref.INFO_FIELDS[1:-1])
            assert counts.shape == (5, 7) and not counts.any()
    finally:
        e.close()


def test_mixed_stream_a_second_pass_and_add(ann):
    """20 000 random records in windows of a few blocks; a second pass after rsqc_reset with another site list starts from zero;
    rsqc_alleles_add of a host-counted half adds exactly."""
    records, first_half, second_half, whole = ac.mixed_tables()
    want = Want(whole)
    assert want.info["hit_records"] > 3000 and want.info["low_mapq_records"] > 1000 and want.info["records"] > want.info["hit_records"]
    stream, _ = ac.bam_body(records)
    e = _engine(ann)
    try:
        _check(e, want, _bam_pass(e, _calls(ac.cut(stream), 7), sites=ac.MIXED_SITES), len(records))
        e.finalize(); e.reset()
        with pytest.raises(engine.EngineError) as err:               # rsqc_reset ended the mode
            e.alleles_end()
        assert err.value.code == abi.ERR_ARG
        other = ac.MIXED_SITES[::3]
        _check(e, Want(ref.tables(records, ac.N_CONTIGS, other, Q, BQ)), _bam_pass(e, _calls(ac.cut(stream), 9), sites=other, pipelined=True), len(records))
        e.finalize(); e.reset()
        half = len(records) // 2
        second = Want(second_half)
        info = _bam_pass(e, _calls(ac.cut(ac.bam_body(records[:half])[0]), 5), sites=ac.MIXED_SITES, pipelined=True)
        assert info[0] == half
        e.alleles_add(second.counts, second.info)                      # the other half, counted on the host
        e.alleles_add(None, dict(seen_records=3, no_seq_records=3))
        got, counts = e.alleles_end()
        assert got["seen_records"] == len(records) + 3 and got["no_seq_records"] == want.info["no_seq_records"] + 3
        for f in ref.INFO_FIELDS[1:-1]:
            if f != "no_seq_records":
                assert got[f] == want.info[f] == first_half[1][f] + second_half[1][f], f
        np.testing.assert_array_equal(counts, want.counts)
        with pytest.raises(engine.EngineError) as err:               # behind rsqc_alleles_end nothing is added
            e.alleles_add(second.counts, second.info)
        assert err.value.code == abi.ERR_ARG
    finally:
        e.close()


def test_call_order_and_arguments(ann):
    records = ac.catalogue()
    calls = _calls(ac.cut(ac.bam_body(records)[0]))
    e = _engine(ann)
    try:
        # without rsqc_alleles_begin: rsqc_alleles_end and rsqc_alleles_add are RSQC_ERR_ARG
        for call in (e.alleles_end, lambda: e.alleles_add(None, {})):
            with pytest.raises(engine.EngineError) as err:
                call()
            assert err.value.code == abi.ERR_ARG
        # the argument rules: each message names the first offending index
        for sites, kw, text in (([(0, 5), (0, 5)], {}, "site 1 "), ([(0, 5), (0, 9), (0, 7), (0, 6)], {}, "site 2 "), ([(1, 5), (0, 9)], {}, "site 1 "),
                                ([(0, 1), (4, 5)], {}, "site 1 "), ([(-1, 5)], {}, "site 0 "), ([(0, 1), (0, 2), (0, -1)], {}, "site 2 "), ([(0, 2 ** 31 - 1)], {}, "site 0 "),
                                ([(0, 5)], dict(min_mapq=256), "min_mapq"), ([(0, 5)], dict(min_baseq=94), "min_baseq")):
            with pytest.raises(engine.EngineError) as err:
                _begin(e, sites, **kw)
            assert err.value.code == abi.ERR_ARG and text in str(err.value), (sites, str(err.value))
        _begin(e, ac.SITES, 255, 93)
        e.reset()
        _begin(e, ac.SITES, 0, 0)
        with pytest.raises(engine.EngineError) as err:               # twice
            _begin(e, ac.SITES, 0, 0)
        assert err.value.code == abi.ERR_ARG
        e.decode_begin(ac.N_CONTIGS)
        with pytest.raises(engine.EngineError) as err:               # while the stream is open
            e.alleles_end()
        assert err.value.code == abi.ERR_ARG and "rsqc_decode_end" in str(err.value)
        one = np.zeros((len(ac.SITES), 7), np.uint64); one[3, 2] = 1
        with pytest.raises(engine.EngineError) as err:               # a table whose sum is not partial's
            e.alleles_add(one, dict(observations=2))
        assert err.value.code == abi.ERR_ARG
        for comp, tab in calls:
            e.decode_submit(comp, tab)
        e.decode_end()
        want = Want(ref.tables(records, ac.N_CONTIGS, ac.SITES, 0, 0))
        assert want.info["low_mapq_records"] == 0 and not want.counts[:, ref.LOW_BASEQ].any()
        _check(e, want, (len(records),), len(records))
        e.finalize(); e.reset()
        e.decode_begin(ac.N_CONTIGS)
        with pytest.raises(engine.EngineError) as err:               # behind rsqc_decode_begin
            _begin(e, ac.SITES)
        assert err.value.code == abi.ERR_ARG
        for comp, tab in calls:
            e.decode_submit(comp, tab)
        e.decode_end()
        with pytest.raises(engine.EngineError) as err:               # behind the pass's submits
            _begin(e, ac.SITES)
        assert err.value.code == abi.ERR_ARG
    finally:
        e.close()
