"""CPU suite of --alleles.  The kernel body (rnaseqc_amd/csrc/rsqc_allele.h) runs on the fiber emulation at several schedules, grid sizes
and window cuts over the catalogue (tests/allele_cases.py), for BAM windows and SAM windows; the one-thread form runs over the same bytes;
and through the host reader of librsqc_host.so, whose workers share one table; all are compared bit for bit with the Python restatement
of the contract (tests/allele_ref.py).  The site-file reader and the report writer are compared with that restatement's rules and
formatting.  A stand-alone sanitizer program hands the one-thread form damaged records and site tables of exactly their length."""
import ctypes as C
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

from rnaseqc_amd import abi
from tests import allele_cases as ac
from tests import allele_ref as ref
from tests.hostemu import allele as emu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q, BQ = ac.MIN_MAPQ, ac.MIN_BASEQ


class Want:
    """The reference's table of a list of records, as an array."""

    def __init__(self, tables):
        counts, self.info = tables
        self.counts = np.array(counts, np.uint64).reshape(len(counts), ref.COLS)


def assert_table(got, want, seen):
    assert got.info() == dict(want.info, seen_records=seen)
    np.testing.assert_array_equal(got.counts, want.counts)


@pytest.fixture(params=[False, True], ids=["plain", "merge"])
def form(request):
    """Both forms of the kernel body: an atomic per observation, and merged across the wave first (RSQC_ALLELE_MERGE)."""
    emu.set_merge(request.param)
    yield request.param
    emu.set_merge(False)


@pytest.fixture()
def main_sites():
    emu.set_sites(ac.N_CONTIGS, ac.SITES, ac.NAMES)


def test_the_catalogue_reaches_what_it_is_for():
    """The reference reads nibbles and text alike; every class, every column and every rule of the walk has a record."""
    records = ac.catalogue(bam_only=True)
    counts, info = ac.catalogue_tables(True)
    assert ref.tables(records, ac.N_CONTIGS, ac.SITES, Q, BQ, nibbles=True) == (counts, info)
    for f in ref.INFO_FIELDS:
        assert info[f] > 0, f
    assert info["records"] + info["off_contig_records"] + info["low_mapq_records"] + info["no_seq_records"] + info["inconsistent_records"] < info["seen_records"]
    assert info["hit_records"] < info["records"]
    for col in range(ref.COLS):
        assert sum(row[col] for row in counts) > 0, ref.COLUMN_NAMES[col]
    both, info_both = ac.catalogue_tables(False)
    for f in ref.INFO_FIELDS:
        assert info_both[f] > 0 or f in ("off_contig_records", "inconsistent_records"), f      # (the two classes SAM cannot spell)
    at_zero = ref.tables(records, ac.N_CONTIGS, ac.SITES, 0, 0)
    assert at_zero[1]["low_mapq_records"] == 0 and at_zero[1]["records"] > info["records"] and sum(r[ref.LOW_BASEQ] for r in at_zero[0]) == 0
    # the first and the last base of a block count, p - 1 and p + n do not; no strand complement
    for code in "MEX":
        rows, i = ac.one("edge_%s_0" % code)
        assert sorted(rows) == [(0, 1000), (0, 1009)] and i["observations"] == 2
        r = [x for x in records if x[1] == "edge_%s_10" % code][0]
        rows, _ = ac.one("edge_%s_10" % code)
        assert all(rows[(0, 1000 + k)][c] == 1 for k in (0, 9) for c in ((ref.LOW_BASEQ,) if r[3][k] < BQ else (ref.base_code(r[2][k]),)))
    # I and S cover no site and shift the query index; the neighbours count
    rows, i = ac.one("i_and_s")
    assert sorted(rows) == [(0, 1100), (0, 1102), (0, 1103), (0, 1105)] and i["observations"] == 4
    rows, _ = ac.one("d_mid")                                          # every position of a D, and the base right behind it
    assert [rows[(0, p)][ref.DELETED] for p in (1203, 1204, 1205)] == [1, 1, 1] and rows[(0, 1202)][ref.DELETED] == 0 == rows[(0, 1206)][ref.DELETED] and (0, 1206) in rows
    rows, _ = ac.one("n_mid")                                          # under an N nothing; right in front of and right behind it a base
    assert sorted(p for t, p in rows if 1300 <= p < 1320) == [1302, 1313, 1315]
    rows, i = ac.one("n_skips_1000")
    assert sorted(rows) == [(0, 2001), (0, 3004)] and i["hit_records"] == 1
    assert ac.one("zero_h_p")[1]["observations"] == 6 and ac.one("code9")[1]["observations"] == 6 and ac.one("cgtag")[1]["observations"] == 3
    assert ac.one("wide_0")[1]["observations"] > 60 and ac.one("long_20000")[1]["observations"] > 2000
    for L in (63, 64, 65):
        assert ac.one("adjacent_%d" % L)[1]["observations"] == L
    rows, _ = ac.one("nibbles")
    assert sum(r[ref.OTHER] for r in rows.values()) == 12 and ac.one("lower_case")[0][(0, 4100)][ref.A] == 1
    rows, _ = ac.one("q_at_and_below")
    assert [rows[(0, 4000 + k)][ref.LOW_BASEQ] for k in range(6)] == [0, 1, 0, 1, 0, 0]
    assert ac.one("q_missing")[1] == dict(ac.one("q_missing")[1], no_qual_records=1, observations=7) and not any(r[ref.LOW_BASEQ] for r in ac.one("q_missing")[0].values())
    rows, _ = ac.one("q_93_and_above")
    assert [rows[(0, 4003 + k)][ref.LOW_BASEQ] for k in range(5)] == [0, 0, 0, 0, 1]
    rows, _ = ac.one("q_below_33", False, ac.sam_only_qualities())
    assert [rows[(0, 4000 + k)][ref.LOW_BASEQ] for k in range(5)] == [1, 0, 1, 0, 1]
    # the table's edges: a read that runs past the end of chrB does not reach chrC's first sites; positions near 2^31 do not wrap
    assert sorted(ac.one("past_the_end_of_b")[0]) == [(1, 1002)] == sorted(ac.one("d_past_the_end_of_b")[0])
    assert ac.one("in_front_of_the_first")[1]["hit_records"] == 0 == ac.one("up_to_the_first")[1]["hit_records"] == ac.one("behind_the_last")[1]["hit_records"]
    assert sorted(ac.one("onto_the_first")[0]) == [(1, 100)] and ac.one("no_sites_on_d")[1] == dict(ac.one("no_sites_on_d")[1], records=1, hit_records=0)
    assert sorted(ac.one("pos_0")[0]) == [(0, 0)] == sorted(ac.one("pos_minus1")[0])
    assert sorted(ac.one("far")[0]) == [(2, 2 ** 31 - 10), (2, 2 ** 31 - 2)] and ac.one("far_d")[0][(2, 2 ** 31 - 2)][ref.DELETED] == 1 and not ac.one("far_start")[0]
    # the classes in their precedence
    for name, f in (("lowq_over_inconsistent", "low_mapq_records"), ("noseq_over_inconsistent", "no_seq_records"), ("lowq_noseq", "low_mapq_records"), ("tid_n_lowq", "off_contig_records"),
                    ("tid_n", "off_contig_records"), ("short", "inconsistent_records"), ("long", "inconsistent_records"), ("no_ops", "inconsistent_records"), ("flag400", "records"),
                    ("mapq_at", "records"), ("mapq_below", "low_mapq_records")):
        i = ac.one(name)[1]
        assert i[f] == 1 and sum(i[g] for g in ref.INFO_FIELDS[1:6]) == 1, name
    assert all(ac.one(n)[1] == dict.fromkeys(ref.INFO_FIELDS, 0, ) | dict(seen_records=1, n_sites=len(ac.SITES)) for n in ("excl_lowq", "excl_off_contig", "flag4"))


def _windows(stream, where, n):
    """The record stream in n windows cut at record boundaries."""
    if n == 1:
        return [stream]
    edges = [0] + [where[(k * len(where)) // n][0] for k in range(1, n)] + [len(stream)]
    return [stream[a:b] for a, b in zip(edges, edges[1:]) if b > a]


@pytest.mark.parametrize("front,n_blocks,n_windows,seed", [(0, 1, 1, 0), (1, 3, 1, 5), (3, 2, 7, 11), (6, 5, 2, 23), (61, 1, 3, 0)])
def test_emulated_kernel_on_bam_windows(form, main_sites, front, n_blocks, n_windows, seed):
    records = ac.catalogue(bam_only=True)
    stream, where = ac.bam_body(records)
    got = emu.run_bam(_windows(stream, where, n_windows), Q, BQ, front=front, n_blocks=n_blocks, seed=seed)
    assert_table(got, Want(ac.catalogue_tables(True)), len(records))


@pytest.mark.parametrize("front,n_blocks,n_windows,seed", [(0, 1, 1, 0), (5, 3, 1, 7), (63, 2, 6, 13), (64, 1, 2, 0)])
def test_emulated_kernel_on_sam_windows(form, main_sites, front, n_blocks, n_windows, seed):
    records = ac.catalogue() + ac.sam_only_qualities()
    lines = [ac.sam_line(r) for r in records]
    cuts = [0] + [(k * len(lines)) // n_windows for k in range(1, n_windows)] + [len(lines)]
    windows = [b"".join(lines[a:b]) for a, b in zip(cuts, cuts[1:])]
    windows[0] = ac.sam_header() + windows[0]                                                # (the header lines are skipped, not counted)
    got = emu.run_sam(windows, Q, BQ, front=front, n_blocks=n_blocks, seed=seed)
    assert_table(got, Want(ref.tables(records, ac.N_CONTIGS, ac.SITES, Q, BQ)), len(records))


@pytest.mark.parametrize("sites", ["empty", "one", "two", "no_first", "no_middle"])
def test_emulated_kernel_at_the_tables_edges(form, sites):
    """No site, one, two; a first and a middle contig without sites (the last has none in every list but the last one here)."""
    emu.set_sites(ac.N_CONTIGS, ac.site_lists()[sites], ac.NAMES)
    records = ac.catalogue(bam_only=True)
    want = Want(ac.catalogue_tables(True, sites))
    assert want.info["records"] > 50 and (want.info["observations"] > 0) == (sites != "empty")
    assert_table(emu.run_bam([ac.bam_body(records)[0]], Q, BQ, n_blocks=2, seed=3), want, len(records))
    assert_table(emu.run_host(ac.bam_body(records)[0], Q, BQ), want, len(records))
    records = ac.catalogue()
    assert_table(emu.run_sam([ac.sam_header() + ac.sam_body(records)], Q, BQ, front=9), Want(ac.catalogue_tables(False, sites)), len(records))


def test_emulated_kernel_on_the_pile_up(form):
    """More than 65 535 in one cell of one launch, several workgroups adding to it; the lanes of a wave meet on the same cells (what the
    merging form is for), on two cells of one site and with lanes in front of and behind the pile that share nothing."""
    emu.set_sites(ac.N_CONTIGS, ac.PILE_SITES, ac.NAMES)
    records = ac.pileup()
    want = Want(ref.tables(records, ac.N_CONTIGS, ac.PILE_SITES, 0, 0))
    assert want.counts[0].tolist() == [0, 70000, 0, 70000, 0, 0, 0] and want.counts[3, ref.DELETED] == 140000 == want.counts[1, ref.G]
    got = emu.run_bam([ac.bam_body(records)[0]], 0, 0, n_blocks=3)
    assert_table(got, want, len(records))


@pytest.fixture(scope="module")
def mixed():
    records, _, _, whole = ac.mixed_tables(3000)                                             # (the whole stream is the GPU suite's)
    return records, Want(whole)


def test_emulated_kernel_on_the_mixed_stream(form, mixed):
    records, want = mixed
    assert want.info["hit_records"] > 500 and want.info["records"] > want.info["hit_records"] and all(want.counts[:, c].sum() > 0 for c in range(ref.COLS))
    emu.set_sites(ac.N_CONTIGS, ac.MIXED_SITES, ac.NAMES)
    stream, where = ac.bam_body(records)
    assert_table(emu.run_bam(_windows(stream, where, 3), Q, BQ, front=2, n_blocks=4, seed=3), want, len(records))
    text = [ac.sam_header() + ac.sam_body(records[:1300]), ac.sam_body(records[1300:])]
    assert_table(emu.run_sam(text, Q, BQ, front=7, n_blocks=3, seed=9), want, len(records))
    assert_table(emu.run_host(stream, Q, BQ), want, len(records))


def test_empty_and_excluded_only(form, main_sites):
    zero = Want(ref.tables([], ac.N_CONTIGS, ac.SITES))
    assert_table(emu.run_bam([b""]), zero, 0)
    assert_table(emu.run_sam([ac.sam_header()]), zero, 0)
    records = [(f,) + ac.pileup()[0][1:] for f in (0x4, 0x100, 0x200, 0x800)]
    assert_table(emu.run_bam([ac.bam_body(records)[0]]), zero, len(records))


def test_one_thread_form(main_sites):
    records = ac.catalogue(bam_only=True)
    assert_table(emu.run_host(ac.bam_body(records)[0], Q, BQ), Want(ac.catalogue_tables(True)), len(records))
    records = ac.catalogue() + ac.sam_only_qualities()
    assert_table(emu.run_host(ac.sam_body(records), Q, BQ, sam=True), Want(ref.tables(records, ac.N_CONTIGS, ac.SITES, Q, BQ)), len(records))


# ---- the host reader, the site-file reader and the writer, through librsqc_host.so ---------------------------------------------------
@pytest.fixture(scope="module")
def host():
    path = os.path.join(ROOT, "rnaseqc_amd", "lib", "librsqc_host.so")
    if not os.path.exists(path):
        pytest.fail("rnaseqc_amd/lib/librsqc_host.so is missing: run build()")
    lib = C.CDLL(path)
    lib.host_bam_alleles.restype = C.c_longlong
    lib.host_bam_alleles.argtypes = [C.c_char_p, C.c_int, C.c_size_t, C.c_int32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(abi.AlleleInfo)]
    lib.host_sites_parse.restype = C.c_longlong
    lib.host_sites_parse.argtypes = [C.c_char_p, C.c_int32, C.POINTER(C.c_char_p), C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_char_p, C.c_uint64]
    lib.host_allele_file.argtypes = [C.c_char_p, C.c_int32, C.POINTER(C.c_char_p), C.c_void_p, C.c_char_p]
    return lib


@pytest.mark.parametrize("threads,batch,block", [(1, 0, 0xFF00), (3, 37, 4099), (4, 1000, 997)])
def test_host_reader_counts_into_one_shared_table(host, tmp_path, mixed, threads, batch, block):
    """Small batches end inside a chunk (its tail is parsed again by the next call: counted once); small BGZF blocks cut records; several
    workers add to one table."""
    for records, sites, want in ((ac.catalogue(bam_only=True), ac.SITES, Want(ac.catalogue_tables(True))), (mixed[0], ac.MIXED_SITES, mixed[1])):
        path = str(tmp_path / "c.bam")
        ac.write_bam(path, records, block=block)
        _, pos, first = emu.site_arrays(ac.N_CONTIGS, sites)
        counts, info = np.zeros((len(sites), ref.COLS), np.uint64), abi.AlleleInfo()
        n = host.host_bam_alleles(path.encode(), threads, batch, ac.N_CONTIGS, len(sites), pos.ctypes.data, first.ctypes.data, Q, BQ, counts.ctypes.data, C.byref(info))
        assert n == len(records)
        assert {f: getattr(info, f) for f in ref.INFO_FIELDS} == dict(want.info, seen_records=n)
        np.testing.assert_array_equal(counts, want.counts)


def _parse(host, path, names):
    cap = 100000
    tid, pos, lines3, text = np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(3, np.uint64), C.create_string_buffer(1 << 22)
    n = host.host_sites_parse(str(path).encode(), len(names), (C.c_char_p * max(len(names), 1))(*[s.encode() for s in names]), tid.ctypes.data, pos.ctypes.data, cap,
                              lines3.ctypes.data, text, len(text))
    if n < 0:
        return n, text.value.decode()
    meta = [tuple(row.split("\t")) for row in text.value.decode().split("\n")[:-1]]
    return list(zip(tid[:n].tolist(), pos[:n].tolist())), meta, [int(v) for v in lines3]


SITE_TEXT = "\n".join([
    "##fileformat=VCFv4.2", "#CHROM\tPOS\tID\tREF\tALT", "",
    "chrB\t500\trs1\tA\tG\t.\tPASS\t.", "chrA\t7\t.\tc\tT,G", "chrA\t3\trs3\tG\t<DEL>\r", "chrZ\t5\trs4\tA\tC", "chrA\t7\tdup\tA\tC", "chrB\t2147483647\tlast\tT\tA",
    "chrA\t9\tindel\tAC\tA", "chrA\t10\tsym\t<X>\tA", "chrA\t11\tn\tN\tA", "chrA\t12\tdot\t.\tA", "\r", "chrD\t000000000000012\tzeros\tt\t.", "#late comment", "chrA\t1\tfirst\tT\tt"])


def test_site_file_reader(host, tmp_path):
    """Plain and gzip; '#' and blank lines; skipped, off-header and duplicate lines; unsorted input comes out sorted by the header's order;
    lower-case REF; a last line without a line feed."""
    want_lines = ref.parse_sites(SITE_TEXT)
    assert want_lines[1] == 4 and len(want_lines[0]) == 8
    for names in (ac.NAMES, ["chrD", "chrB", "chrA"], ["chrQ"], []):
        want = ref.resolve_sites(want_lines[0], names)
        for k, data in enumerate((SITE_TEXT.encode(), gzip.compress(SITE_TEXT.encode()), (SITE_TEXT + "\n").encode())):
            path = tmp_path / ("s%d.vcf" % k)
            path.write_bytes(data)
            assert ref.read_sites(str(path)) == want_lines
            sites, meta, lines3 = _parse(host, path, names)
            assert (sites, meta) == (want[0], want[1]) and lines3 == [want_lines[1], want[2], want[3]]
    sites, meta, lines3 = _parse(host, path, ac.NAMES)
    assert sites == [(0, 0), (0, 2), (0, 6), (1, 499), (1, 2 ** 31 - 2), (3, 11)] and meta[2] == (".", "c", "T,G") and lines3 == [4, 1, 1]
    assert ref.check_sites(ac.N_CONTIGS, sites) is None
    path = tmp_path / "catalogue.vcf.gz"
    path.write_bytes(gzip.compress(ac.vcf_text(ac.SITES).encode()))
    assert _parse(host, path, ac.NAMES)[0] == ac.SITES
    assert _parse(host, tmp_path / "none.vcf", ac.NAMES)[0] == -10


@pytest.mark.parametrize("line,number", [("chrA\t5\t.\tA", 3), ("chrA", 3), ("chrA\t0\t.\tA\tC", 3), ("chrA\t2147483648\t.\tA\tC", 3), ("chrA\t-4\t.\tA\tC", 3), ("chrA\t5x\t.\tA\tC", 3),
                                         ("chrA\t\t.\tA\tC", 3), ("chrA\t+5\t.\tA\tC", 3), ("chrA\t5.0\t.\tA\tC", 3), ("chrA 5 . A C", 3), ("chrA\t99999999999999999999999\t.\tA\tC", 3), ("chrA\t0000000000000\t.\tAC\tC", 3)])
def test_site_file_malformed_lines(host, tmp_path, line, number):
    text = "#h\nchrA\t1\t.\tA\tC\n" + line + "\nchrA\t9\t.\tA\tC\n"
    with pytest.raises(ref.SitesError) as err:
        ref.parse_sites(text)
    assert err.value.args == (number,)
    path = tmp_path / "bad.vcf"
    path.write_text(text)
    n, message = _parse(host, path, ac.NAMES)
    assert n == -11 and message.startswith("%s:%d: " % (path, number))


def _file(host, tmp_path, vcf, names, counts):
    path, out = tmp_path / "w.vcf", tmp_path / "w.tsv"
    path.write_text(vcf)
    counts = np.ascontiguousarray(counts, np.uint64)
    assert host.host_allele_file(str(path).encode(), len(names), (C.c_char_p * max(len(names), 1))(*[s.encode() for s in names]), counts.ctypes.data, str(out).encode()) == 0
    return out.read_bytes().decode()


def test_writer(host, tmp_path, main_sites):
    """Byte for byte against the reference's formatting: the catalogue's table; multi-allelic ALT, ALT equal to REF, '.', symbolic ALT,
    a repeated ALT entry, lower case, counts of 2^40; an empty table gives the header alone."""
    want = Want(ac.catalogue_tables(True))
    vcf = ac.vcf_text(ac.SITES)
    lines, _ = ref.parse_sites(vcf)
    sites, meta, _, _ = ref.resolve_sites(lines, ac.NAMES)
    assert sites == ac.SITES
    assert _file(host, tmp_path, vcf, ac.NAMES, want.counts) == ref.format_file(ac.NAMES, sites, meta, want.counts.tolist())
    vcf = "\n".join("chrB\t%d\tid%d\t%s\t%s" % (k + 1, k, r, a) for k, (r, a) in enumerate(
        [("A", "C"), ("A", "C,G,T"), ("A", "A"), ("A", "."), ("A", "<DEL>"), ("A", "C,C,c"), ("a", "g"), ("T", "A,TT,G,*"), ("C", ""), ("G", "A,,T"), ("G", "N,R,a")])) + "\n"
    lines, _ = ref.parse_sites(vcf)
    sites, meta, _, _ = ref.resolve_sites(lines, ac.NAMES)
    counts = np.array([[1, 20, 300, 4000, 5, 6, 7]] * len(sites), np.uint64)
    counts[1] = [2 ** 40, 2 ** 40 + 1, 2 ** 40 + 2, 2 ** 40 + 3, 0, 0, 0]
    got = _file(host, tmp_path, vcf, ac.NAMES, counts)
    assert got == ref.format_file(ac.NAMES, sites, meta, counts.tolist())
    rows = [r.split("\t") for r in got.splitlines()]
    assert rows[0] == ref.FILE_HEADER.split("\t") and len(rows) == 12 and rows[1][:5] == ["chrB", "1", "id0", "A", "C"]
    assert [r[-2:] for r in rows[1:]] == [["1", "20"], [str(2 ** 40), str(3 * 2 ** 40 + 6)], ["1", "0"], ["1", "0"], ["1", "0"], ["1", "20"], ["1", "300"], ["4000", "301"], ["20", "0"],
                                          ["300", "4001"], ["300", "1"]]
    assert _file(host, tmp_path, "#nothing\n", ac.NAMES, np.zeros((0, 7), np.uint64)) == ref.FILE_HEADER + "\n"
    assert _file(host, tmp_path, vcf, ["chrQ"], np.zeros((0, 7), np.uint64)) == ref.FILE_HEADER + "\n"


def test_damaged_records_under_sanitizers(tmp_path):
    """tests/hostemu/allele_fuzz.cpp as a program of its own under the address / undefined-behaviour sanitizers: records in heap buffers of
    exactly their size and site tables of exactly their length -- a short block_size, an impossible l_seq, operations that run past L, tid
    at and beyond the table's end, pos at both ends of its range, random damage -- read nothing outside either."""
    exe = emu.build_fuzz(str(tmp_path / "allele_fuzz"))
    r = subprocess.run([exe, "6000", "31"], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    cases, walked = (int(x) for x in re.search(r"allele_fuzz: (\d+) cases, (\d+) of 6000 random ones walked", r.stdout).groups())
    assert cases > 12000 and 100 < walked < 6000


def test_cli_refusals_before_any_gpu_work(tmp_path):
    """Exit 6 with the message, before any input is opened; the usage text names the flags."""
    exe = os.path.join(ROOT, "rnaseqc_amd", "bin", "rnaseqc")
    if not os.path.exists(exe):
        pytest.fail("rnaseqc_amd/bin/rnaseqc is missing: run build()")
    out = str(tmp_path / "o")
    for extra, env in ((["--gpus", "2"], {}), ([], dict(RSQC_GPUS="3")), ([], dict(RSQC_GPU_LIST="0,1"))):
        p = subprocess.run([exe, "--alleles=s.vcf", "a.gtf", "b.bam", out, *extra], capture_output=True, text=True, env=dict(os.environ, **env))
        assert p.returncode == 6 and "--alleles runs on one GPU" in p.stderr and not os.path.exists(out), (p.returncode, p.stderr)
    for args, text in ((["--allele-mapq=3"], "--alleles"), (["--allele-baseq=3"], "--alleles"), (["--alleles", "s.vcf", "--allele-mapq=256"], "0..255"),
                       (["--alleles", "s.vcf", "--allele-mapq", "-1"], "0..255"), (["--alleles=s.vcf", "--allele-baseq=94"], "0..93"), (["--alleles=s.vcf", "--allele-baseq", "-1"], "0..93")):
        p = subprocess.run([exe, *args, "a.gtf", "b.bam", out], capture_output=True, text=True)
        assert p.returncode == 6 and text in p.stderr and not os.path.exists(out), (args, p.returncode, p.stderr)
    p = subprocess.run([exe, "--help"], capture_output=True, text=True)
    assert all(t in p.stdout + p.stderr for t in ("--alleles=", "--allele-mapq", "--allele-baseq", "allele_counts.tsv"))
