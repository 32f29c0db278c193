"""CPU suite of --mismatches.  The kernel body (rnaseqc_amd/csrc/rsqc_mismatch.h) runs on the fiber emulation at several schedules, grid
sizes and window cuts over the catalogue (tests/mismatch_cases.py), for BAM windows and SAM windows; the one-thread form runs over the
same bytes, and through the host reader of librsqc_host.so on the catalogue's BAM file; all are compared bit for bit with the Python
restatement of the contract (tests/mismatch_ref.py).  The three report writers are compared byte for byte with the reference's formatting.
A stand-alone sanitizer program hands the one-thread form damaged records."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from rnaseqc_amd import abi
from tests import mismatch_cases as mc
from tests import mismatch_ref as ref
from tests.hostemu import mismatch as emu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = mc.MIN_MAPQ


class Want:
    """The reference's tables of a list of records, as arrays."""

    def __init__(self, tables):
        cyc, subst, byq, self.info = tables
        self.cyc, self.subst, self.byq = np.array(cyc, np.uint64), np.array(subst, np.uint64), np.array(byq, np.uint64)
        i = self.info
        self.len_sum = i["compared"] + i["uncompared"] + i["inserted"] + i["clipped"] + i["beyond_bases"]


@pytest.fixture(scope="module", autouse=True)
def reference():
    emu.set_reference(mc.REFERENCE, [c[0] for c in mc.CONTIGS])


@pytest.fixture(scope="module")
def want_catalogue():
    return Want(mc.catalogue_tables(True))


@pytest.fixture(scope="module")
def want_both_spellings():
    return Want(mc.catalogue_tables(False))


@pytest.fixture(scope="module")
def mixed():
    records = mc.mixed(3000)                                                                 # (the whole stream is the GPU suite's)
    return records, Want(ref.tables(records, mc.REFERENCE, Q))


def assert_tables(got, want, seen):
    info, len_sum = got.info()
    assert info == dict(want.info, seen_records=seen)
    assert len_sum == want.len_sum
    np.testing.assert_array_equal(got.cyc, want.cyc)
    np.testing.assert_array_equal(got.subst, want.subst)
    np.testing.assert_array_equal(got.byq, want.byq)


def test_the_catalogue_reaches_what_it_is_for():
    """The reference reads nibbles and text alike, and every class, column and edge of the contract has a record."""
    records = mc.catalogue(bam_only=True)
    cyc, subst, byq, info = mc.catalogue_tables(True)
    assert ref.tables(records, mc.REFERENCE, Q, nibbles=True) == (cyc, subst, byq, info)
    for f in ref.INFO_FIELDS:
        assert info[f] > 0, f
    assert info["records"] + info["no_reference_records"] + info["low_mapq_records"] + info["no_seq_records"] + info["inconsistent_records"] < info["seen_records"]
    for e in (0, 1):
        assert all(subst[e][r][b] > 0 for r in range(4) for b in range(4))                   # all 12 substitution types, both ends
        assert all(cyc[e][511][k] > 0 for k in (ref.COMPARED, ref.MISMATCH)) and any(cyc[e][c][ref.DELETIONS] for c in range(512))
    assert byq[63][0] > 0 and byq[62][1] > 0 and byq[30][0] >= 64
    at_zero = ref.tables(records, mc.REFERENCE, 0)[3]
    assert at_zero["low_mapq_records"] == 0 and at_zero["records"] > info["records"]


def test_pack_code_of_every_byte():
    codes = emu.pack_codes()
    for v in range(256):
        assert codes[v] == ref.ref_code(chr(v)), v
    assert sorted(set(codes.tolist())) == [0, 1, 2, 3, 4]


def _windows(stream, where, n):
    """The record stream in n windows cut at record boundaries."""
    if n == 1:
        return [stream]
    edges = [0] + [where[(k * len(where)) // n][0] for k in range(1, n)] + [len(stream)]
    return [stream[a:b] for a, b in zip(edges, edges[1:]) if b > a]


@pytest.mark.parametrize("front,n_blocks,n_windows,seed", [(0, 1, 1, 0), (1, 3, 1, 5), (3, 2, 7, 11), (6, 5, 2, 23), (61, 1, 3, 0)])
def test_emulated_kernel_on_bam_windows(want_catalogue, front, n_blocks, n_windows, seed):
    records = mc.catalogue(bam_only=True)
    stream, where = mc.bam_body(records)
    got = emu.run_bam(_windows(stream, where, n_windows), Q, front=front, n_blocks=n_blocks, seed=seed)
    assert_tables(got, want_catalogue, len(records))


@pytest.mark.parametrize("front,n_blocks,n_windows,seed", [(0, 1, 1, 0), (5, 3, 1, 7), (63, 2, 6, 13), (64, 1, 2, 0)])
def test_emulated_kernel_on_sam_windows(want_both_spellings, front, n_blocks, n_windows, seed):
    records = mc.catalogue()
    lines = [mc.sam_line(r) for r in records]
    cuts = [0] + [(k * len(lines)) // n_windows for k in range(1, n_windows)] + [len(lines)]
    windows = [b"".join(lines[a:b]) for a, b in zip(cuts, cuts[1:])]
    windows[0] = mc.sam_header() + windows[0]                                                # (the header lines are skipped, not counted)
    got = emu.run_sam(windows, Q, front=front, n_blocks=n_blocks, seed=seed)
    assert_tables(got, want_both_spellings, len(records))


def test_emulated_kernel_on_the_pile_up():
    """More than 65 535 in one cell of one launch, on one end and split over both."""
    records = mc.pileup()
    want = Want(ref.tables(records, mc.REFERENCE, 0))
    assert want.cyc[0, 1, ref.COMPARED] == 70000 + 35000 and want.cyc[1, 3, ref.MISMATCH] == 0 and want.cyc[1, 2, ref.MISMATCH] == 35000
    got = emu.run_bam([mc.bam_body(records)[0]], 0, n_blocks=2)
    assert_tables(got, want, len(records))


def test_emulated_kernel_on_the_mixed_stream(mixed):
    records, want = mixed
    stream, where = mc.bam_body(records)
    assert_tables(emu.run_bam(_windows(stream, where, 3), Q, front=2, n_blocks=4, seed=3), want, len(records))
    text = [mc.sam_header() + mc.sam_body(records[:1300]), mc.sam_body(records[1300:])]
    assert_tables(emu.run_sam(text, Q, front=7, n_blocks=3, seed=9), want, len(records))


def test_empty_and_excluded_only():
    zero = Want(ref.tables([], mc.REFERENCE))
    assert_tables(emu.run_bam([b""]), zero, 0)
    assert_tables(emu.run_sam([mc.sam_header()]), zero, 0)
    records = [(f,) + mc.pileup()[0][1:] for f in (0x4, 0x100, 0x200, 0x800)]
    assert_tables(emu.run_bam([mc.bam_body(records)[0]]), zero, len(records))


def test_one_thread_form(want_catalogue, want_both_spellings, mixed):
    records = mc.catalogue(bam_only=True)
    assert_tables(emu.run_host(mc.bam_body(records)[0], Q), want_catalogue, len(records))
    records = mc.catalogue()
    assert_tables(emu.run_host(mc.sam_body(records), Q, sam=True), want_both_spellings, len(records))
    assert_tables(emu.run_host(mc.bam_body(mixed[0])[0], Q), mixed[1], len(mixed[0]))


# ---- the host reader and the report writers, through librsqc_host.so ---------------------------------------------------------------
@pytest.fixture(scope="module")
def host():
    path = os.path.join(ROOT, "rnaseqc_amd", "lib", "librsqc_host.so")
    if not os.path.exists(path):
        pytest.fail("rnaseqc_amd/lib/librsqc_host.so is missing: run build()")
    lib = C.CDLL(path)
    lib.host_bam_mismatches.restype = C.c_longlong
    lib.host_bam_mismatches.argtypes = [C.c_char_p, C.c_int, C.c_size_t, C.c_int32, C.c_void_p, C.POINTER(C.c_char_p), C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.POINTER(abi.MismatchInfo)]
    lib.host_mismatch_files.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_char_p, C.c_char_p]
    return lib


@pytest.mark.parametrize("threads,batch,block", [(1, 0, 0xFF00), (3, 37, 4099), (4, 1000, 997)])
def test_host_reader_counts_the_catalogue(host, tmp_path, want_catalogue, threads, batch, block):
    """Small batches end inside a chunk (its tail is parsed again by the next call: counted once); small BGZF blocks cut records."""
    records = mc.catalogue(bam_only=True)
    path = str(tmp_path / "c.bam")
    mc.write_bam(path, records, block=block)
    cyc, subst, byq, info = np.zeros(emu.CYC_SHAPE, np.uint64), np.zeros(emu.SUBST_SHAPE, np.uint64), np.zeros(emu.BYQ_SHAPE, np.uint64), abi.MismatchInfo()
    lengths = np.array([r[1] for r in mc.REFERENCE], np.uint64)
    seqs = (C.c_char_p * 3)(*[None if r[2] is None else r[2].encode() for r in mc.REFERENCE])
    n = host.host_bam_mismatches(path.encode(), threads, batch, 3, lengths.ctypes.data, seqs, Q, cyc.ctypes.data, subst.ctypes.data, byq.ctypes.data, C.byref(info))
    assert n == len(records)
    assert {f: getattr(info, f) for f in ref.INFO_FIELDS} == want_catalogue.info
    np.testing.assert_array_equal(cyc, want_catalogue.cyc)
    np.testing.assert_array_equal(subst, want_catalogue.subst)
    np.testing.assert_array_equal(byq, want_catalogue.byq)


def _files(host, tmp_path, cyc, subst, byq):
    t = [np.ascontiguousarray(a, np.uint64) for a in (cyc, subst, byq)]
    paths = [str(tmp_path / n) for n in ("c.tsv", "t.tsv", "q.tsv")]
    assert host.host_mismatch_files(*[a.ctypes.data for a in t], *[p.encode() for p in paths]) == 0
    return [open(p, "rb").read().decode() for p in paths]


def _formatted(cyc, subst, byq):
    return [ref.format_cycles(cyc.tolist()), ref.format_types(subst.tolist()), ref.format_quality(byq.tolist())]


def test_writers_on_the_catalogue_and_the_mixed_stream(host, tmp_path, want_catalogue, mixed):
    for w in (want_catalogue, mixed[1]):
        got = _files(host, tmp_path, w.cyc, w.subst, w.byq)
        assert got == _formatted(w.cyc, w.subst, w.byq)
    assert got[1].count("\n") == 1 + 32 and got[2].count("\n") == 1 + 5                     # (the mixed stream: both ends, five quality bins)


def test_writers_at_their_edges(host, tmp_path):
    """Rows with compared = 0 (rate 0), a row that only a deletion makes, rows with nothing in the middle, an empty end 2 (no rows of it
    in either file), an end 2 without a compared base (rows by cycle, none by type), large counts, empty tables (the headers alone)."""
    cyc, subst, byq = np.zeros(emu.CYC_SHAPE, np.uint64), np.zeros(emu.SUBST_SHAPE, np.uint64), np.zeros(emu.BYQ_SHAPE, np.uint64)
    cyc[0, 0] = [3, 1, 0, 0, 0, 0]; cyc[0, 1] = [0, 0, 2, 1, 1, 0]; cyc[0, 2] = [7, 7, 0, 0, 0, 0]; cyc[0, 9] = [0, 0, 0, 0, 0, 1]
    cyc[0, 511] = [2 ** 40, 2 ** 40 // 3, 0, 0, 0, 0]
    subst[0, 0, 0] = 2; subst[0, 2, 3] = 8; subst[0, 3, 3] = 2 ** 40
    byq[0] = [1, 1]; byq[40] = [2 ** 40, 12345]; byq[63] = [3, 0]; byq[17] = [0, 0]
    got = _files(host, tmp_path, cyc, subst, byq)
    assert got == _formatted(cyc, subst, byq)
    rows = got[0].splitlines()
    assert len(rows) == 1 + 512 and rows[1] == "1\t1\t3\t1\t0\t0\t0\t0\t0.333333" and rows[2] == "1\t2\t0\t0\t2\t1\t1\t0\t0.000000" and rows[3].endswith("\t1.000000")
    assert rows[5] == "1\t5\t0\t0\t0\t0\t0\t0\t0.000000" and rows[10] == "1\t10\t0\t0\t0\t0\t0\t1\t0.000000"
    assert got[1].count("\n") == 1 + 16 and got[1].splitlines()[1:3] == ["1\tA\tA\t2", "1\tA\tC\t0"] and "1\tG\tT\t8" in got[1]
    assert got[2].splitlines() == ["quality\tcompared\tmismatches\tmismatch_rate", "0\t1\t1\t1.000000", "40\t%d\t12345\t0.000000" % 2 ** 40, "63\t3\t0\t0.000000"]
    cyc[1, 3] = [0, 0, 0, 0, 4, 0]                                                           # end 2: clipped bases only
    got = _files(host, tmp_path, cyc, subst, byq)
    assert got == _formatted(cyc, subst, byq)
    assert got[0].splitlines()[-4:] == ["2\t%d\t0\t0\t0\t0\t%d\t0\t0.000000" % (c, 4 if c == 4 else 0) for c in (1, 2, 3, 4)] and "\n2\t" not in got[1]
    zero = [np.zeros(s, np.uint64) for s in (emu.CYC_SHAPE, emu.SUBST_SHAPE, emu.BYQ_SHAPE)]
    assert _files(host, tmp_path, *zero) == ["end\tcycle\tcompared\tmismatches\tuncompared\tinserted\tclipped\tdeletions\tmismatch_rate\n", "end\tref\tread\tcount\n",
                                             "quality\tcompared\tmismatches\tmismatch_rate\n"]


def test_damaged_records_under_sanitizers(tmp_path):
    """tests/hostemu/mismatch_fuzz.cpp as a program of its own under the address / undefined-behaviour sanitizers: records with a short
    block_size, an impossible l_seq, no read name, the largest n_cigar count nothing; operations that run past L make the record
    inconsistent; pos near 2^31 and at the contig's edges reads nothing outside a reference of exactly its length; random damage reads
    nothing outside its record."""
    exe = emu.build_fuzz(str(tmp_path / "mismatch_fuzz"))
    r = subprocess.run([exe, "6000", "29"], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    cases, refused = (int(x) for x in re.search(r"mismatch_fuzz: (\d+) cases, (\d+) of 6000 random ones refused", r.stdout).groups())
    assert cases > 16000 and 100 < refused < 6000


def test_cli_refusals_before_any_gpu_work(tmp_path):
    """Exit 6 with the message, before any input is opened; the usage text names the flags."""
    exe = os.path.join(ROOT, "rnaseqc_amd", "bin", "rnaseqc")
    if not os.path.exists(exe):
        pytest.fail("rnaseqc_amd/bin/rnaseqc is missing: run build()")
    out = str(tmp_path / "o")
    for extra, env in ((["--gpus", "2"], {}), ([], dict(RSQC_GPUS="3")), ([], dict(RSQC_GPU_LIST="0,1"))):
        p = subprocess.run([exe, "--mismatches", "--fasta", "r.fa", "a.gtf", "b.bam", out, *extra], capture_output=True, text=True, env=dict(os.environ, **env))
        assert p.returncode == 6 and "--mismatches runs on one GPU" in p.stderr and not os.path.exists(out), (p.returncode, p.stderr)
    for args, text in ((["--mismatches"], "--fasta"), (["--mismatches-mapq=3", "--fasta", "r.fa"], "--mismatches"), (["--mismatches", "--fasta", "r.fa", "--mismatches-mapq=256"], "0..255"),
                       (["--mismatches", "--fasta", "r.fa", "--mismatches-mapq", "-1"], "0..255")):
        p = subprocess.run([exe, *args, "a.gtf", "b.bam", out], capture_output=True, text=True)
        assert p.returncode == 6 and text in p.stderr and not os.path.exists(out), (args, p.returncode, p.stderr)
    p = subprocess.run([exe, "--help"], capture_output=True, text=True)
    assert "--mismatches-mapq" in p.stdout + p.stderr and "mismatch_quality.tsv" in p.stdout + p.stderr
