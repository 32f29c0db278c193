"""-m gpu: --bedgraph through the C ABI (rsqc_track_begin / rsqc_track_end / rsqc_track_rows / rsqc_track_text,
rnaseqc_amd/csrc/rsqc_track.hip).  The rows and the text of every pass are compared, row for row and byte for byte, with the numpy
restatement of the contract (tests/track_ref.py); rsqc_results of a pass with the calls equal those of the same pass without them."""
import numpy as np
import pytest

from rnaseqc_amd import abi, engine, synth
from rnaseqc_amd.model import Batch
from tests import junction_cases as jc
from tests import junction_ref
from tests import track_cases as tc
from tests import track_ref as ref
from tests.compare import assert_results_match

pytestmark = pytest.mark.gpu


def _pull(e, info, window=None, text=True):
    """The whole table (and its text) in windows of `window` rows."""
    n = int(info["n_rows"])
    step = window or max(n, 1)
    parts = [e.track_rows(k, min(step, n - k)) for k in range(0, n, step)]
    out = {f: (np.concatenate([p[f] for p in parts]) if parts else np.zeros(0, np.int64)) for f in ref.COLUMNS}
    out.update(info)
    if text:
        out["text"] = b"".join(e.track_text(k, min(step, n - k)) for k in range(0, n, step))
    return out


def _pass(p, ann, batches, lengths, names, track=True, sort=None, junctions=None, bed=None, resident=False):
    """One pass; sort / junctions: None, "first" (begun in front of the track) or "last".  Returns (results, track, junction table)."""
    e = engine.Engine(p)
    try:
        e.set_annotation(ann)
        if bed is not None:
            e.set_bed(bed)
        if sort == "first":
            e.sort_begin()
        if junctions == "first":
            e.junctions_begin()
        if track:
            e.track_begin(lengths, names)
        if junctions == "last":
            e.junctions_begin()
        if sort == "last":
            e.sort_begin()
        for b in batches:
            if resident:
                e.submit_resident(e.upload(b))
            else:
                e.submit(b)
        if sort:
            e.sort_end()
        res = e.finalize()
        t = _pull(e, e.track_end()) if track else None
        return res, t, (e.junctions_end() if junctions else None)
    finally:
        e.close()


def _check(got, want, names):
    ref.assert_tracks_equal(got, want)
    assert ref.covered(got) == int(got["aligned_bases"])
    assert got["text"] == ref.render(want, names)


@pytest.fixture(scope="module")
def fix():
    class F:
        pass
    f = F()
    f.ann, f.reads = jc.fixture_a()
    f.parts = tc.cut(f.reads)
    f.want = tc.fixture_a_track()
    f.p = abi.default_params()
    f.plain, _, _ = _pass(f.p, f.ann, f.parts, None, None, track=False)
    return f


def test_fixture_a_in_five_batches(fix):
    res, got, _ = _pass(fix.p, fix.ann, fix.parts, tc.A_LENGTHS, tc.A_NAMES)
    _check(got, fix.want, tc.A_NAMES)
    assert got["events_ms"] > 0 and got["scan_ms"] > 0 and got["rows_ms"] > 0
    assert_results_match(res, fix.plain)                  # the calls change no other output


def test_fixture_a_in_one_batch_with_clipped_records(fix):
    reads, extra = tc.fixture_a_clipped()
    _, got, _ = _pass(fix.p, fix.ann, [reads, extra], tc.A_LENGTHS, tc.A_NAMES)
    _check(got, tc.fixture_a_track(clipped=True), tc.A_NAMES)
    assert got["clipped_bases"] > 0


def test_resident_batch(fix):
    res, got, _ = _pass(fix.p, fix.ann, [fix.reads], tc.A_LENGTHS, tc.A_NAMES, resident=True)
    _check(got, fix.want, tc.A_NAMES)
    assert_results_match(res, fix.plain)


def test_one_batch_of_several_file_ranges(fix):
    s = fix.reads.coordinate_sorted()
    parts = [s.slice(int(s.seg_start[k]), int(s.seg_start[k + 1])) for k in range(len(s.seg_tid))]
    one = Batch.concat_ranges(parts)
    assert one.seg_file_index is not None and len(one.seg_file_index) >= 3
    _, got, _ = _pass(fix.p, fix.ann, [one], tc.A_LENGTHS, tc.A_NAMES)
    _check(got, fix.want, tc.A_NAMES)


@pytest.mark.parametrize("order", ["first", "last"])
def test_shuffled_records_under_sort(fix, order):
    """The events are taken from the sorted output batches; the track is that of the records in any order."""
    srt = fix.reads.coordinate_sorted()
    shuffled = srt.take(np.random.default_rng(54).permutation(srt.n))
    want_res, _, _ = _pass(fix.p, fix.ann, [srt], None, None, track=False)
    res, got, _ = _pass(fix.p, fix.ann, tc.cut(shuffled, seed=3, parts=4), tc.A_LENGTHS, tc.A_NAMES, sort=order)
    _check(got, fix.want, tc.A_NAMES)
    assert_results_match(res, want_res)


@pytest.mark.parametrize("order", ["first", "last"])
def test_with_junctions(fix, order):
    """Both modes in one pass: the two populations are equal and the junction table is the one of a pass without the track."""
    res, got, table = _pass(fix.p, fix.ann, fix.parts, tc.A_LENGTHS, tc.A_NAMES, junctions=order)
    _check(got, fix.want, tc.A_NAMES)
    junction_ref.assert_tables_equal(table, jc.fixture_a_table())
    assert table["population"] == got["population"] == 40_000
    assert_results_match(res, fix.plain)


def test_bed_and_legacy_do_not_change_the_track(fix):
    bed = synth.make_bed(fix.ann, min_len=250)
    p_bed = abi.default_params(fragment_samples=150)
    res, got, _ = _pass(p_bed, fix.ann, fix.parts, tc.A_LENGTHS, tc.A_NAMES, bed=bed)
    _check(got, fix.want, tc.A_NAMES)
    assert_results_match(res, _pass(p_bed, fix.ann, fix.parts, None, None, track=False, bed=bed)[0])
    p_leg = abi.default_params(legacy=1)
    res, got, _ = _pass(p_leg, fix.ann, fix.parts, tc.A_LENGTHS, tc.A_NAMES)
    _check(got, fix.want, tc.A_NAMES)
    assert_results_match(res, _pass(p_leg, fix.ann, fix.parts, None, None, track=False)[0])


@pytest.mark.parametrize("merge", ["0", "1"])
def test_later_events_merged_or_lane_by_lane(fix, merge, monkeypatch):
    """RSQC_TRACK_MERGE picks how the events behind a record's first are added: the track is the same."""
    monkeypatch.setenv("RSQC_TRACK_MERGE", merge)
    _, got, _ = _pass(fix.p, fix.ann, [fix.reads.coordinate_sorted()], tc.A_LENGTHS, tc.A_NAMES)
    _check(got, fix.want, tc.A_NAMES)


@pytest.fixture(scope="module")
def one(fix):
    """One context, reset between the cases that need nothing else."""
    e = engine.Engine(fix.p)
    e.set_annotation(fix.ann)
    yield e
    e.close()


def test_windows_concatenate_to_the_whole(fix, one):
    e = one
    e.reset()
    e.track_begin(tc.A_LENGTHS, tc.A_NAMES)
    e.submit(fix.reads)
    e.finalize()
    info = e.track_end()
    assert info["n_rows"] > 4097
    whole = _pull(e, info)
    _check(whole, fix.want, tc.A_NAMES)
    for window in (64, 4096, 4097):
        got = _pull(e, info, window=window)
        _check(got, fix.want, tc.A_NAMES)
    head = _pull(e, dict(info, n_rows=130), window=1)          # (windows of one row: the first 130)
    for f in ref.COLUMNS:
        assert np.array_equal(head[f], whole[f][:130])
    assert head["text"] == ref.render(fix.want, tc.A_NAMES, 0, 130)
    again = e.track_end()                                      # a second call: the same figures, no device work
    assert again == info
    assert e.track_text(0, 0) == b"" and e.track_text(info["n_rows"], 0) == b""
    with pytest.raises(engine.EngineError) as err:
        e.track_rows(info["n_rows"] - 1, 2)
    assert err.value.code == abi.ERR_ARG


def test_windows_of_one_row_concatenate_to_the_whole(one):
    """A whole table pulled one row at a time, rows and text: the 4 096 rows of the chunk that is all heads."""
    batches, want = tc.crafted_case("chunk_of_heads_only")
    e = one
    e.reset()
    e.track_begin(tc.LENGTHS, tc.NAMES)
    e.submit(batches[0])
    e.finalize()
    info = e.track_end()
    assert info["n_rows"] == tc.CHUNK
    _check(_pull(e, info, window=1), want, tc.NAMES)


@pytest.mark.parametrize("merge", ["0", "1"])
@pytest.mark.parametrize("name", tc.CRAFTED_NAMES)
def test_crafted(one, name, merge, monkeypatch):
    monkeypatch.setenv("RSQC_TRACK_MERGE", merge)
    batches, want = tc.crafted_case(name)
    e = one
    e.reset()
    e.track_begin(tc.LENGTHS, tc.NAMES)
    for b in batches:
        e.submit(b)
    e.finalize()
    got = _pull(e, e.track_end(), window=64)
    _check(got, want, tc.NAMES)
    if want["n_rows"] == 0:
        assert got["text"] == b""


def test_eight_digit_coordinates(one):
    """One contig of 10 000 100 positions (a 40 MB array): starts and ends of 7 and 8 digits."""
    L = 10_000_100
    recs = [dict(tid=0, pos=p, cigar=[(tc.M, 60)]) for p in (999_990, 9_999_950, 9_999_990, 10_000_000, 10_000_000, L - 30)]
    b = Batch.from_records(recs)
    want = ref.track([b], [L])
    assert want["n_rows"] == 7 and want["clipped_bases"] == 30 and int(want["start"][-1]) == L - 30 and int(want["end"][-1]) == L
    e = one
    e.reset()
    e.track_begin([L], ["chr1"])
    e.submit(b)
    e.finalize()
    got = _pull(e, e.track_end())
    _check(got, want, ["chr1"])
    assert b"chr1\t9999990\t10000000\t2\nchr1\t10000000\t10000010\t4\n" in got["text"]


def test_capacity_refusal_then_reset(fix, one, monkeypatch):
    """RSQC_TRACK_MAX_BYTES = 1024: rsqc_track_begin refuses the array with the sizes in its message; the context works after a reset."""
    e = one
    e.reset()
    monkeypatch.setenv("RSQC_TRACK_MAX_BYTES", "1024")
    with pytest.raises(engine.EngineError) as err:
        e.track_begin(tc.A_LENGTHS, tc.A_NAMES)
    assert err.value.code == abi.ERR_CAPACITY and "1700000 positions" in str(err.value) and "1024" in str(err.value)
    monkeypatch.delenv("RSQC_TRACK_MAX_BYTES")
    e.reset()
    e.track_begin(tc.A_LENGTHS, tc.A_NAMES)
    for part in fix.parts:
        e.submit(part)
    assert_results_match(e.finalize(), fix.plain)
    _check(_pull(e, e.track_end()), fix.want, tc.A_NAMES)
    monkeypatch.setenv("RSQC_TRACK_MAX_BYTES", str(4 * (1_700_003 + 1) + 64))       # exactly the array: allowed
    e.reset()
    e.track_begin(tc.A_LENGTHS, tc.A_NAMES)


def test_call_order_and_arguments(fix):
    def refused(call, text, code=abi.ERR_ARG):
        with pytest.raises(engine.EngineError) as err:
            call()
        assert err.value.code == code and text in str(err.value), str(err.value)

    e = engine.Engine(fix.p)
    try:
        refused(lambda: e.track_begin(tc.A_LENGTHS), "rsqc_set_annotation")            # no annotation
        e.set_annotation(fix.ann)
        refused(e.track_end, "rsqc_track_begin must precede")                          # not begun
        refused(lambda: e.track_begin([1 << 31]), "2^31 - 1")
        refused(lambda: e.track_begin([100], ["x" * 256]), "255")
        e.submit(fix.parts[0])
        refused(lambda: e.track_begin(tc.A_LENGTHS), "first submit")                   # behind a submit of the same pass
        e.reset()
        e.track_begin(tc.A_LENGTHS)                                                    # (no names: rows only)
        refused(lambda: e.track_begin(tc.A_LENGTHS), "already")                        # twice
        e.submit(fix.parts[0])
        refused(e.track_end, "rsqc_finalize")                                          # the pass is not finalized
        refused(lambda: e.track_rows(0, 0), "rsqc_track_end must precede")
        e.finalize()
        refused(lambda: e.track_begin(tc.A_LENGTHS), "rsqc_reset")                     # behind rsqc_finalize
        info = e.track_end()
        want = ref.track([fix.parts[0]], tc.A_LENGTHS)
        ref.assert_tracks_equal(_pull(e, info, text=False), want)
        refused(lambda: e.track_text(0, 1), "no contig names")
        e.reset()                                                                      # a pass without the calls behind one with them: the mode has ended
        for part in fix.parts:
            e.submit(part)
        assert_results_match(e.finalize(), fix.plain)
        refused(e.track_end, "rsqc_track_begin must precede")
    finally:
        e.close()
