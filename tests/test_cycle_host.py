"""CPU suite of --cycles.  The kernel body (rnaseqc_amd/csrc/rsqc_cycle.h) runs on the fiber emulation at several schedules, grid sizes
and window cuts over the catalogue (tests/cycle_cases.py), for BAM windows and SAM windows; the host reader runs through
librsqc_host.so on the catalogue's BAM file; both are compared bit for bit with the Python restatement of the contract
(tests/cycle_ref.py).  The two report writers are compared byte for byte with the reference's formatting.  A stand-alone sanitizer
program hands the layout helper and the per-record body damaged records."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from rnaseqc_amd import abi
from tests import cycle_cases as cc
from tests import cycle_ref as ref
from tests.hostemu import cycle as emu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Want:
    """The reference's tables of a list of records, as arrays."""

    def __init__(self, records):
        base, qual, self.info = ref.tables(records)
        self.base, self.qual = np.array(base, np.uint64), np.array(qual, np.uint64)
        self.len_sum = self.info["bases"] + self.info["beyond_bases"]


@pytest.fixture(scope="module")
def want_catalogue():
    return Want(cc.catalogue(bam_only=True))


@pytest.fixture(scope="module")
def want_both_spellings():
    return Want(cc.catalogue())


@pytest.fixture(scope="module")
def mixed():
    records = cc.mixed(3000)                                                                 # (the whole stream is the GPU suite's)
    return records, Want(records)


def assert_tables(got, want, seen):
    info, len_sum = got.info()
    assert info == dict(want.info, seen_records=seen)
    assert len_sum == want.len_sum
    np.testing.assert_array_equal(got.base, want.base)
    np.testing.assert_array_equal(got.qual, want.qual)


def test_reference_reads_nibbles_and_text_alike():
    """The catalogue is the same alignments in both spellings only if the base of a character does not depend on the spelling."""
    records = cc.catalogue(bam_only=True)
    assert ref.tables(records) == ref.tables(records, nibbles=True)
    base, qual, info = ref.tables(records)
    assert info["beyond_bases"] > 0 and info["clamped_quals"] > 0 and info["no_seq_records"] == 4 and info["no_qual_records"] == 2
    assert info["records"] + info["no_seq_records"] < info["seen_records"]                  # excluded flags
    assert sum(base[1][511]) > 0 and sum(base[0][511]) > 0                                   # both ends reach the last cycle


def _windows(stream, where, n):
    """The record stream in n windows cut at record boundaries."""
    if n == 1:
        return [stream]
    edges = [0] + [where[(k * len(where)) // n][0] for k in range(1, n)] + [len(stream)]
    return [stream[a:b] for a, b in zip(edges, edges[1:]) if b > a]


@pytest.mark.parametrize("front,n_blocks,n_windows,seed", [(0, 1, 1, 0), (1, 3, 1, 5), (3, 2, 7, 11), (6, 5, 2, 23), (61, 1, 3, 0)])
def test_emulated_kernel_on_bam_windows(want_catalogue, front, n_blocks, n_windows, seed):
    records = cc.catalogue(bam_only=True)
    stream, where = cc.bam_body(records)
    got = emu.run_bam(_windows(stream, where, n_windows), front=front, n_blocks=n_blocks, seed=seed)
    assert_tables(got, want_catalogue, len(records))


@pytest.mark.parametrize("front,n_blocks,n_windows,seed", [(0, 1, 1, 0), (5, 3, 1, 7), (63, 2, 6, 13), (64, 1, 2, 0)])
def test_emulated_kernel_on_sam_windows(want_both_spellings, front, n_blocks, n_windows, seed):
    records = cc.catalogue()
    lines = [cc.sam_line(r) for r in records]
    cuts = [0] + [(k * len(lines)) // n_windows for k in range(1, n_windows)] + [len(lines)]
    windows = [b"".join(lines[a:b]) for a, b in zip(cuts, cuts[1:])]
    windows[0] = cc.sam_header() + windows[0]                                                # (the header lines are skipped, not counted)
    got = emu.run_sam(windows, front=front, n_blocks=n_blocks, seed=seed)
    assert_tables(got, want_both_spellings, len(records))


def test_emulated_kernel_on_the_pile_up():
    """More than 65 535 in one cell of one launch, on one end and split over both."""
    records = cc.pileup()
    want = Want(records)
    assert want.qual[0, 0, 30] == 70000 + 35000 and want.qual[1, 3, 33] == 35000
    got = emu.run_bam([cc.bam_body(records)[0]])
    assert_tables(got, want, len(records))


def test_emulated_kernel_on_the_mixed_stream(mixed):
    records, want = mixed
    stream, where = cc.bam_body(records)
    assert_tables(emu.run_bam(_windows(stream, where, 3), front=2, n_blocks=4, seed=3), want, len(records))
    text = [cc.sam_header() + cc.sam_body(records[:1300]), cc.sam_body(records[1300:])]
    assert_tables(emu.run_sam(text, front=7, n_blocks=3, seed=9), want, len(records))


def test_empty_and_excluded_only():
    zero = Want([])
    assert_tables(emu.run_bam([b""]), zero, 0)
    assert_tables(emu.run_sam([cc.sam_header()]), zero, 0)
    records = cc.excluded_only()
    assert_tables(emu.run_bam([cc.bam_body(records)[0]]), Want(records), len(records))
    assert Want(records).info["bases"] == 0


def test_one_thread_form(want_catalogue):
    records = cc.catalogue(bam_only=True)
    assert_tables(emu.run_host_bam(cc.bam_body(records)[0]), want_catalogue, len(records))


# ---- the host reader and the report writers, through librsqc_host.so ---------------------------------------------------------------
@pytest.fixture(scope="module")
def host():
    path = os.path.join(ROOT, "rnaseqc_amd", "lib", "librsqc_host.so")
    if not os.path.exists(path):
        pytest.fail("rnaseqc_amd/lib/librsqc_host.so is missing: run build()")
    lib = C.CDLL(path)
    lib.host_bam_cycles.restype = C.c_longlong
    lib.host_bam_cycles.argtypes = [C.c_char_p, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.POINTER(abi.CycleInfo)]
    lib.host_cycle_files.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, C.c_char_p]
    return lib


@pytest.mark.parametrize("threads,batch,block", [(1, 0, 0xFF00), (3, 37, 4099), (4, 1000, 997)])
def test_host_reader_counts_the_catalogue(host, tmp_path, want_catalogue, threads, batch, block):
    """Small batches end inside a chunk (its tail is parsed again by the next call: counted once); small BGZF blocks cut SEQ and QUAL."""
    records = cc.catalogue(bam_only=True)
    path = str(tmp_path / "c.bam")
    cc.write_bam(path, records, block=block)
    base, qual, info = np.zeros(emu.BASE_SHAPE, np.uint64), np.zeros(emu.QUAL_SHAPE, np.uint64), abi.CycleInfo()
    n = host.host_bam_cycles(path.encode(), threads, batch, base.ctypes.data, qual.ctypes.data, C.byref(info))
    assert n == len(records)
    assert {f: getattr(info, f) for f in ref.INFO_FIELDS} == want_catalogue.info
    np.testing.assert_array_equal(base, want_catalogue.base)
    np.testing.assert_array_equal(qual, want_catalogue.qual)


def _files(host, tmp_path, base, qual):
    b, q = np.ascontiguousarray(base, np.uint64), np.ascontiguousarray(qual, np.uint64)
    pb, pq = str(tmp_path / "b.tsv"), str(tmp_path / "q.tsv")
    assert host.host_cycle_files(b.ctypes.data, q.ctypes.data, pb.encode(), pq.encode()) == 0
    return open(pb, "rb").read().decode(), open(pq, "rb").read().decode()


def test_writers_on_the_catalogue_and_the_mixed_stream(host, tmp_path, want_catalogue, mixed):
    for w in (want_catalogue, mixed[1]):
        got_b, got_q = _files(host, tmp_path, w.base, w.qual)
        assert got_b == ref.format_bases(w.base.tolist()) and got_q == ref.format_quality(w.base.tolist(), w.qual.tolist())
    assert got_b.count("\n") == 1 + 512 + 512                                                # (the mixed stream: both ends reach 512 cycles)


def test_writers_at_the_quantile_edges(host, tmp_path):
    """n = 1, 2, 3, 4 and more, ties at the quantile's edge, a row with bases and no quality, rows with nothing in the middle, a
    single-end table (no rows of end 2), an empty table (the headers alone)."""
    base, qual = np.zeros(emu.BASE_SHAPE, np.uint64), np.zeros(emu.QUAL_SHAPE, np.uint64)
    cells = [{5: 1}, {5: 1, 40: 1}, {0: 1, 20: 1, 63: 1}, {1: 1, 2: 1, 3: 1, 4: 1}, {10: 2, 30: 2}, {7: 3, 8: 1}, {}, {63: 5}, {0: 4, 1: 4, 2: 4, 3: 4, 4: 1}]
    for c, cell in enumerate(cells):
        n = sum(cell.values())
        base[0, c, c % 5] = max(n, 2)                                                        # (more bases than qualities: records without QUAL)
        for q, v in cell.items():
            qual[0, c, q] = v
    base[0, 20, 4] = 3                                                                       # rows 10..20 are printed, all zero
    base[0, 511, 0] = 2 ** 40
    qual[0, 511, 37] = 2 ** 40 - 1
    qual[0, 511, 2] = 1
    got_b, got_q = _files(host, tmp_path, base, qual)
    assert got_b == ref.format_bases(base.tolist()) and got_q == ref.format_quality(base.tolist(), qual.tolist())
    rows = got_q.splitlines()
    assert len(rows) == 1 + 512 and rows[1] == "1\t1\t1\t5.000000\t5\t5\t5" and rows[2] == "1\t2\t2\t22.500000\t5\t5\t40"
    assert rows[3] == "1\t3\t3\t27.666667\t0\t20\t63" and rows[4] == "1\t4\t4\t2.500000\t1\t2\t3" and rows[7] == "1\t7\t0\t0.000000\t0\t0\t0"
    assert all(r.startswith("1\t") for r in rows[1:])
    base[1, 2, 1] = 9
    got_b, got_q = _files(host, tmp_path, base, qual)
    assert got_b == ref.format_bases(base.tolist()) and got_q == ref.format_quality(base.tolist(), qual.tolist())
    assert got_b.splitlines()[-3:] == ["2\t1\t0\t0\t0\t0\t0\t0", "2\t2\t0\t0\t0\t0\t0\t0", "2\t3\t0\t9\t0\t0\t0\t9"]
    got_b, got_q = _files(host, tmp_path, np.zeros(emu.BASE_SHAPE, np.uint64), np.zeros(emu.QUAL_SHAPE, np.uint64))
    assert got_b == "end\tcycle\tA\tC\tG\tT\tN\ttotal\n" and got_q == "end\tcycle\tbases\tmean\tq25\tmedian\tq75\n"


def test_damaged_records_under_sanitizers(tmp_path):
    """tests/hostemu/cycle_fuzz.cpp as a program of its own under the address / undefined-behaviour sanitizers: records with a short
    block_size, an impossible l_seq, no read name, the largest n_cigar, and SAM lines cut in front of the end of QUAL, each in a heap
    buffer of exactly its size, count nothing; random damage reads nothing outside its record."""
    exe = emu.build_fuzz(str(tmp_path / "cycle_fuzz"))
    r = subprocess.run([exe, "6000", "29"], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    cases, refused = (int(x) for x in re.search(r"cycle_fuzz: (\d+) cases, (\d+) of 6000 random ones refused", r.stdout).groups())
    assert cases > 19000 and 300 < refused < 6000


def test_cli_refuses_more_than_one_gpu(tmp_path):
    """Exit 6 with the message, before any input is opened or any GPU work; the usage text names the flag."""
    exe = os.path.join(ROOT, "rnaseqc_amd", "bin", "rnaseqc")
    if not os.path.exists(exe):
        pytest.fail("rnaseqc_amd/bin/rnaseqc is missing: run build()")
    out = str(tmp_path / "o")
    for extra, env in ((["--gpus", "2"], {}), ([], dict(RSQC_GPUS="3")), ([], dict(RSQC_GPU_LIST="0,1"))):
        p = subprocess.run([exe, "--cycles", "a.gtf", "b.bam", out, *extra], capture_output=True, text=True, env=dict(os.environ, **env))
        assert p.returncode == 6 and "--cycles runs on one GPU" in p.stderr and not os.path.exists(out), (p.returncode, p.stderr)
    p = subprocess.run([exe, "--help"], capture_output=True, text=True)
    assert "--cycles" in p.stdout + p.stderr and "cycle_quality.tsv" in p.stdout + p.stderr
