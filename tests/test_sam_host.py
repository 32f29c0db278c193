"""SAM text input on the host (no GPU): the device stages' per-lane bodies (rnaseqc_amd/csrc/rsqc_sam.h, rsqc_samrec.h) run
as a wave of one lane (tests/hostemu/sam_emu.cpp) -- SAM line against BAM record of the same alignment, field by field; the
stream's columns against the written batch at many window cuts; the malformed-line rules with their line numbers; the
htslib-derived rules on hand-written lines; and the host side's header parsing."""
import numpy as np
import pytest

from rnaseqc_amd import abi, bamio, synth
from rnaseqc_amd.model import Batch
from tests.hostemu import sam

CONTIGS = [("chrA", 3_000_000), ("chrB", 1_000_000), ("chrC", 500_000)]
NAMES = [c[0] for c in CONTIGS]


def _wide_and_odd_records():
    """Records every BAM decode corner has: a CIGAR of more than 65 535 operations, l_seq >= 65 535, NM >= 255, names of 1 and
    254 bytes, duplicates, unplaced records, mates on other contigs."""
    M, I, D, N, S = abi.CIG_M, abi.CIG_I, abi.CIG_D, abi.CIG_N, abi.CIG_S
    recs = []
    recs.append(dict(tid=0, pos=100, mpos=300, isize=250, flag=99, mapq=255, cigar=[(M, 1), (D, 1)] * 35000 + [(M, 10)], nm=3, qname="w" * 254))
    recs.append(dict(tid=0, pos=200, mpos=100, isize=-250, flag=147, mapq=60, cigar=[(S, 5), (M, 70000)], nm=400, qname="x"))
    recs.append(dict(tid=0, pos=200, mpos=100, isize=-250, flag=1171, mapq=60, cigar=[(M, 50), (N, 1000), (M, 25)], nm=None, qname="x", ch=True))
    recs.append(dict(tid=1, pos=5, mpos=900, mtid=2, isize=0, flag=65, mapq=3, cigar=[(M, 20), (I, 2), (M, 28)], nm=-3, qname="mate:elsewhere", tags=[True]))
    recs.append(dict(tid=1, pos=7, mpos=-1, mtid=-1, isize=0, flag=9, mapq=0, cigar=[(M, 30)], nm=0, qname="m_unm"))
    recs.append(dict(tid=-1, pos=-1, mpos=-1, mtid=-1, isize=0, flag=4, mapq=0, cigar=[], l_qseq=76, nm=None, qname="unplaced"))
    recs.append(dict(tid=-1, pos=-1, mpos=-1, mtid=-1, isize=0, flag=0, mapq=0, cigar=[], l_qseq=0, nm=None, qname="unplaced_mapped"))
    return Batch.from_records(recs)


def _batch(n_pairs=3000, seed=36):
    ann = synth.make_annotation(seed=35, contigs=[("chrA", 3_000_000, 120), ("chrB", 1_000_000, 40), ("chrC", 500_000, 10)])
    b = synth.make_reads(ann, n_pairs, seed=seed, keep_qnames=True, chimeric_tag_frac=0.02, filter_tag_frac=0.03, dup_frac=0.05,
                         contig_lengths=np.array([3_000_000, 1_000_000, 500_000]))
    return ann, b


def _check_stream(p, batch):
    """The emulated stream's columns against the batch (tests/test_gpu_decode.py's check_columns on one part)."""
    n = batch.n
    assert len(p["core"]) == n
    np.testing.assert_array_equal(p["core"]["cigar_off"], batch.cigar_off)
    for f in ("pos", "mpos", "isize"):
        np.testing.assert_array_equal(p["core"][f], getattr(batch, f), err_msg=f)
    for f in ("qhash", "flag", "l_qseq", "mapq", "nm", "tagbits", "n_cigar"):
        np.testing.assert_array_equal(p["aux"][f], getattr(batch, f), err_msg=f)
    if batch.qhash2 is not None:
        np.testing.assert_array_equal(p["qhash2"], batch.qhash2)
    np.testing.assert_array_equal(p["cigar"], batch.cigar)
    assert [int(t) for t in p["seg_tid"]] == [int(t) for t in batch.seg_tid]
    assert [int(x) for x in p["seg_start"][:-1]] == [int(x) for x in batch.seg_start[:-1]]
    np.testing.assert_array_equal(p["wide_index"], batch.wide_index)
    np.testing.assert_array_equal(p["wide_nm"], batch.wide_nm)
    np.testing.assert_array_equal(p["wide_lq"], batch.wide_l_qseq)
    np.testing.assert_array_equal(p["wide_nc"], batch.wide_n_cigar)


@pytest.fixture(scope="module")
def written(tmp_path_factory):
    d = tmp_path_factory.mktemp("sam")
    _, b = _batch()
    batch = bamio.sam_consistent(Batch.concat([b, _wide_and_odd_records()]))
    assert batch.n >= 5000 and len(batch.wide_index) >= 3
    bam, samp = str(d / "x.bam"), str(d / "x.sam")
    # (bamio.write_bam stores at most 65 535 operations per record: the longer CIGAR is in the SAM only)
    nc = batch.n_cigar.astype(np.int64)
    nc[batch.wide_index.astype(np.int64)] = batch.wide_n_cigar
    keep = np.flatnonzero(nc < 65536)
    bamio.write_bam(bam, CONTIGS, batch.take(keep))
    bamio.write_sam(samp, CONTIGS, batch)
    return batch, bam, samp, keep


def test_sam_line_equals_bam_record(written):
    """sam_parse_line on every written SAM line == bam_parse_record on the BAM record of the same alignment."""
    batch, bam, samp, keep = written
    sam.begin(NAMES, "ch", ("XF",))
    lines, recs = sam.bam_records(bam), [sam.sam_lines(samp)[k] for k in keep]
    assert len(lines) == len(recs) == batch.n - 1
    for i, (rec, line) in enumerate(zip(lines, recs)):
        a, b = sam.parse_bam_record(rec), sam.parse_line(line)
        assert b["code"] == 0, (i, line[:80])
        for f in sam.FIELDS[1:]:
            assert a[f] == b[f], (i, f, a[f], b[f])
        np.testing.assert_array_equal(a["ops"], b["ops"])


@pytest.mark.parametrize("cut", ["one", "name", "seq", "tab", "newline", "crlf", "tiny", "random"])
def test_window_cuts_give_the_same_columns(written, cut):
    """Windows cut inside a name, inside SEQ, on a tab, on '\\n', inside '\\r\\n', in calls shorter than one line: the carried
    bytes give the columns of one window, equal to the batch."""
    batch, _, samp, _ = written
    text = open(samp, "rb").read()
    if cut == "crlf":
        text = text.replace(b"\n", b"\r\n")
    rng = np.random.default_rng(7)
    if cut == "one":
        cuts = []
    elif cut == "tiny":                                       # far smaller than a line (the wide lines are 70-280 KB)
        cuts = list(range(0, len(text), 4099))
    elif cut == "random":
        cuts = sorted(set(rng.integers(0, len(text), 40).tolist()))
    else:
        want = {"name": lambda t, p: t[p - 1:p] == b"\n", "seq": lambda t, p: t[p - 1:p] == b"A" and t[p:p + 1] == b"A",
                "tab": lambda t, p: t[p:p + 1] == b"\t", "newline": lambda t, p: t[p:p + 1] == b"\n",
                "crlf": lambda t, p: t[p - 1:p] == b"\r"}[cut]
        cuts, p = [], 1
        while p < len(text):
            q = p + int(rng.integers(30_000, 90_000))
            while q < len(text) and not want(text, q if cut != "name" else q):
                q += 1
            if cut == "name":
                q += 2
            if q < len(text):
                cuts.append(q)
            p = q + 1
    sam.begin(NAMES, "ch", ("XF",))
    edges = [0] + cuts + [len(text)]
    for a, b in zip(edges[:-1], edges[1:]):
        if b > a:
            sam.submit(text[a:b], per_thread=int(rng.integers(1, 64)))
    sam.end()
    p = sam.result()
    assert p["carry"] == 0
    _check_stream(p, batch)
    assert not p["unsorted"] and p["n_bad"] == 1 and p["bad_names"] == ["unplaced_mapped"]


def test_missing_final_newline_and_blank_lines(written):
    batch, _, samp, _ = written
    text = open(samp, "rb").read()
    head, body = text.split(b"\n", 1)
    text2 = head + b"\n\n\r\n" + body.replace(b"\n", b"\n\n", 50).rstrip(b"\n")
    sam.begin(NAMES, "ch", ("XF",))
    sam.submit(text2[:len(text2) // 2])
    sam.submit(text2[len(text2) // 2:])
    assert sam.result()["carry"] > 0
    sam.end()
    _check_stream(sam.result(), batch)


GOOD = b"r1\t99\tchrA\t101\t60\t10M\t=\t201\t110\tAAAAAAAAAA\tIIIIIIIIII\tNM:i:2"
HDR = b"@HD\tVN:1.6\n@SQ\tSN:chrA\tLN:1000\n"


@pytest.mark.parametrize("bad,code", [
    (b"r1\t99\tchrA\t101\t60\t10M\t=\t201\t110\tAAAAAAAAAA", 1),                              # 10 fields
    (b"r1\t9x\tchrA\t101\t60\t10M\t=\t201\t110\tAAAAAAAAAA\t*", 2),                          # FLAG
    (b"r1\t99\tchrA\t-5\t60\t10M\t=\t201\t110\tAAAAAAAAAA\t*", 2),                           # POS
    (b"r1\t99\tchrA\t2147483649\t60\t10M\t=\t201\t110\tAAAAAAAAAA\t*", 2),                   # POS overflow
    (b"r1\t99\tchrA\t101\t256\t10M\t=\t201\t110\tAAAAAAAAAA\t*", 2),                         # MAPQ overflow
    (b"r1\t99\tchrA\t101\t60\t10M\t=\t201\t99999999999\tAAAAAAAAAA\t*", 2),                  # TLEN overflow
    (b"r1\t99\tchrA\t101\t60\t10Q\t=\t201\t110\tAAAAAAAAAA\t*", 3),                          # unknown operator
    (b"r1\t99\tchrA\t101\t60\tM\t=\t201\t110\tAAAAAAAAAA\t*", 3),                            # no length
    (b"r1\t99\tchrA\t101\t60\t9M\t=\t201\t110\tAAAAAAAAAA\t*", 4),                           # SEQ / CIGAR
    (b"r1\t99\tchrA\t101\t60\t10M\t=\t201\t110\tAAAAAAAAAA\tIII", 5),                        # SEQ / QUAL
    (b"@CO\tlate header line", 6),
    (b"r1\t99\tchrA\t101\t60\t10M\t=\t201\t110\tAAAAAAAAAA\t*\tNM:i:x", 2),                  # NM value
])
def test_malformed_line_and_its_number(bad, code):
    """Each rule gives the error code and the 1-based line number (header lines counted), wherever the window is cut."""
    text = HDR + GOOD + b"\n" + GOOD + b"\n\n" + bad + b"\n" + GOOD + b"\n"
    for cut in (len(text), 40, len(HDR) + len(GOOD) + 3):
        sam.begin(["chrA"])
        with pytest.raises(sam.SamError) as e:
            sam.submit(text[:cut])
            if cut < len(text):
                sam.submit(text[cut:])
            sam.end()
        assert (e.value.code, e.value.line) == (code, 6), cut


def _one(line, names=("chrA", "chrB"), ch="ch", filt=("XF",)):
    sam.begin(list(names), ch, filt)
    return sam.parse_line(line)


def test_htslib_derived_rules():
    # unknown RNAME: tid -1 and the unmapped bit; its mate field resolves the same way
    r = _one(b"q\t0\tchrZ\t5\t60\t4M\tchrZ\t9\t0\tAAAA\t*")
    assert (r["code"], r["tid"], r["flag"] & 4, r["pos"], r["tagbits"] & abi.TB_MTID_SAME) == (0, -1, 4, 4, abi.TB_MTID_SAME)
    # POS 0 on a named reference: tid -1 + unmapped; RNAME '*' keeps the flag
    r = _one(b"q\t0\tchrB\t0\t60\t4M\t*\t0\t0\tAAAA\t*")
    assert (r["tid"], r["flag"], r["pos"], r["mpos"]) == (-1, 4, -1, -1)
    r = _one(b"q\t0\t*\t0\t0\t*\t*\t0\t0\tAAAA\tIIII")
    assert (r["tid"], r["flag"], r["n_ops"], r["l_seq"]) == (-1, 0, 0, 4)
    # '=' and '*' RNEXT, a named mate
    assert _one(b"q\t1\tchrB\t3\t1\t2M\t=\t7\t6\tAA\t*")["tagbits"] & abi.TB_MTID_SAME
    assert not _one(b"q\t1\tchrB\t3\t1\t2M\t*\t7\t6\tAA\t*")["tagbits"] & abi.TB_MTID_SAME
    assert _one(b"q\t1\tchrB\t3\t1\t2M\tchrB\t7\t6\tAA\t*")["tagbits"] & abi.TB_MTID_SAME
    assert not _one(b"q\t1\tchrB\t3\t1\t2M\tchrA\t7\t6\tAA\t*")["tagbits"] & abi.TB_MTID_SAME
    # hexadecimal FLAG
    assert _one(b"q\t0x93\tchrA\t3\t1\t2M\t=\t7\t6\tAA\t*")["flag"] == 0x93
    # NM:f / NM:Z are not integer tags; NM:i is; the last NM decides
    assert not _one(b"q\t0\tchrA\t3\t1\t2M\t=\t7\t6\tAA\t*\tNM:f:2.0")["tagbits"] & abi.TB_HAS_NM
    r = _one(b"q\t0\tchrA\t3\t1\t2M\t=\t7\t6\tAA\t*\tNM:i:2\tNM:i:300")
    assert (r["nm"], r["wide"], r["tagbits"] & abi.TB_HAS_NM) == (300, 1, abi.TB_HAS_NM)
    # chimeric tag: Z or A; filter tags: Z, f or i count, A / H / B do not
    assert _one(b"q\t0\tchrA\t3\t1\t2M\t=\t7\t6\tAA\t*\tch:A:1")["tagbits"] & abi.TB_HAS_CH
    assert not _one(b"q\t0\tchrA\t3\t1\t2M\t=\t7\t6\tAA\t*\tch:i:1")["tagbits"] & abi.TB_HAS_CH
    for t, want in ((b"XF:Z:a", True), (b"XF:f:1.5", True), (b"XF:i:-4", True), (b"XF:A:c", False), (b"XF:H:1A", False), (b"XF:B:c,1", False)):
        assert bool(_one(b"q\t0\tchrA\t3\t1\t2M\t=\t7\t6\tAA\t*\t" + t)["tagbits"] & abi.TB_FILTER0) == want, t
    # a trailing '\r' is not part of QUAL; '*' SEQ with a CIGAR is allowed
    assert _one(b"q\t0\tchrA\t3\t1\t2M\t=\t7\t6\tAA\tII\r")["code"] == 0
    assert _one(b"q\t0\tchrA\t3\t1\t2M\t=\t7\t6\t*\t*")["code"] == 0


def test_header_lines_and_blank_lines_in_front():
    """'@' lines in front of the first record are the header's (any number of windows); blank lines are skipped."""
    body = b"r\t0\tchrA\t5\t60\t4M\t*\t0\t0\tAAAA\t*\n"
    text = b"@HD\tVN:1.6\n\n" + b"".join(b"@SQ\tSN:c%d\tLN:10\n" % k for k in range(500)) + b"@SQ\tSN:chrA\tLN:100\n" + body * 3
    sam.begin(["chrA"], buf_bytes=1 << 16)                    # (header lines are shorter than a record line: the ABI's buffer has room)
    for k in range(0, len(text), 1000):
        sam.submit(text[k:k + 1000])
    sam.end()
    p = sam.result()
    assert len(p["core"]) == 3 and list(p["seg_tid"]) == [0] and list(p["core"]["pos"]) == [4, 4, 4]


def test_unsorted_and_bad_refid():
    """The sort test and the unrecognised-RefID names, judged on primary, mapped, QC-passed records as in the BAM path."""
    l = lambda n, f, r, p: b"%s\t%d\t%s\t%d\t60\t4M\t*\t0\t0\tAAAA\t*\n" % (n, f, r, p)
    text = l(b"a", 0, b"chrA", 50) + l(b"b", 0, b"chrA", 40) + l(b"c", 0, b"*", 0) + l(b"d", 256, b"*", 0) + l(b"e", 0, b"chrQ", 3)
    sam.begin(["chrA"])
    sam.submit(text[:60])
    sam.submit(text[60:])
    sam.end()
    p = sam.result()
    assert p["unsorted"] and p["n_bad"] == 1 and p["bad_names"] == ["c"]


def test_header_parsing(tmp_path):
    """The command line's SAM header reader (host/sam_feed.cpp): @SQ order, extra fields, no @SQ, BGZF or plain."""
    import ctypes as C
    import os
    so = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rnaseqc_amd", "lib", "librsqc_host.so")
    l = C.CDLL(so)
    l.host_sam_header.argtypes = [C.c_char_p, C.c_char_p, C.c_int]
    l.host_sam_header.restype = C.c_int
    out = C.create_string_buffer(1 << 16)
    cases = [(b"@HD\tVN:1.6\n@SQ\tSN:b\tLN:5\tAS:x\n@SQ\tLN:7\tSN:a\n@PG\tID:x\nq\t4\t*\t0\t0\t*\t*\t0\t0\t*\t*\n", "b:5,a:7"),
             (b"@HD\tVN:1.6\nq\t4\t*\t0\t0\t*\t*\t0\t0\t*\t*\n", ""),
             (b"q\t4\t*\t0\t0\t*\t*\t0\t0\t*\t*\n", "")]
    for k, (text, want) in enumerate(cases):
        for bgzf in (False, True):
            path = str(tmp_path / ("h%d%s" % (k, ".sam.gz" if bgzf else ".sam")))
            if bgzf:
                with open(path, "wb") as f:
                    f.write(bamio._bgzf_block(text) + bamio._EOF)
            else:
                open(path, "wb").write(text)
            kind = l.host_sam_header(path.encode(), out, len(out))
            assert kind == (2 if bgzf else 1), (k, bgzf, kind)
            assert out.value.decode() == want, (k, bgzf)
    bam = str(tmp_path / "x.bam")
    bamio.write_bam(bam, CONTIGS, Batch.from_records([dict(tid=0, pos=1, cigar=[(0, 5)])]))
    assert l.host_sam_header(bam.encode(), out, len(out)) == 3
    gz = str(tmp_path / "x.sam.gz")
    import gzip
    open(gz, "wb").write(gzip.compress(cases[0][0]))
    assert l.host_sam_header(gz.encode(), out, len(out)) == -2


def test_operations_at_two_bytes_each_fit_the_columns():
    """The densest valid CIGARs ("1M1D..." with SEQ '*': an operation per 2 bytes of text) in a window whose buffers are exactly
    as large as the ABI makes them for that window: every operation lands, none outside the column.  Malformed lines whose
    operator counts are larger than the text can hold are refused with their line number."""
    M, D = abi.CIG_M, abi.CIG_D
    n_ops = 4000
    line = b"q\t0\tchrA\t1\t0\t" + b"1M1D" * (n_ops // 2) + b"\t*\t0\t0\t*\t*\n"
    text = line * 40
    sam.begin(["chrA"])
    sam.submit(text)
    sam.end()
    p = sam.result()
    assert len(p["core"]) == 40 and len(p["cigar"]) == 40 * n_ops
    np.testing.assert_array_equal(p["cigar"][:4], [(1 << 4) | M, (1 << 4) | D, (1 << 4) | M, (1 << 4) | D])
    assert list(p["wide_nc"]) == [n_ops] * 40
    bad = b"q\t0\tchrA\t1\t0\t" + b"M" * 30000 + b"\t*\t0\t0\t*\t*\n"
    sam.begin(["chrA"])
    with pytest.raises(sam.SamError) as e:
        sam.submit(line * 3 + bad + line * 20)
    assert (e.value.code, e.value.line) == (3, 4)


def test_sam_stages_on_mutated_text_under_sanitizers(tmp_path):
    """50 000 mutated SAM texts (tests/hostemu/sam_fuzz.cpp) through the stage bodies with every buffer exactly as large as the
    C ABI makes it, under the address / undefined-behaviour sanitizers: records or a refused line, never an access outside."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "sam_fuzz")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(root, "tests", "hostemu", "sam_fuzz.cpp"), "-o", exe])
    r = subprocess.run([exe, "50000", "17"], capture_output=True, text=True, timeout=900, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and "50000 cases" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    import re
    refused, records = (int(x) for x in re.search(r"(\d+) refused, (\d+) records", r.stdout).groups())
    assert refused > 1000 and records > 100_000                  # both outcomes are exercised


def test_inputs_that_are_no_sam(tmp_path):
    """An empty file and bytes that are neither BGZF nor SAM text stay "Unable to open" inputs (not SAM without @SQ lines)."""
    import ctypes as C
    import os
    so = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rnaseqc_amd", "lib", "librsqc_host.so")
    l = C.CDLL(so)
    l.host_sam_header.argtypes = [C.c_char_p, C.c_char_p, C.c_int]
    out = C.create_string_buffer(256)
    for k, data in enumerate([b"", b"\x00\x01garbage\n", b"hello world\nthis is text\n", b"\x1f"]):
        path = str(tmp_path / ("n%d" % k))
        open(path, "wb").write(data)
        assert l.host_sam_header(path.encode(), out, len(out)) == 0, data
    path = str(tmp_path / "ok.sam")
    open(path, "wb").write(b"r\t0\t*\t0\t0\t*\t*\t0\t0\t*\t*\n")
    assert l.host_sam_header(path.encode(), out, len(out)) == 1


def test_threaded_sam_writer_equals_python_writer(written, tmp_path):
    """bamio.write_sam_fast (the C++ writer beside the BAM one) writes the bytes bamio.write_sam writes, plain and BGZF."""
    import gzip
    batch, _, samp, _ = written
    a, b = str(tmp_path / "a.sam"), str(tmp_path / "b.sam.gz")
    bamio.write_sam_fast(a, CONTIGS, batch, threads=3)
    bamio.write_sam_fast(b, CONTIGS, batch, threads=2, bgzf=True)
    want = open(samp, "rb").read()
    assert open(a, "rb").read() == want
    assert gzip.decompress(open(b, "rb").read()) == want
