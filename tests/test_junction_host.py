"""CPU: --junctions.  The kernels of rnaseqc_amd/csrc/rsqc_junction.h, unmodified, on the 64-lane emulation (extract, both sort
stages with rsqc_sort.h's passes, the segmented reduce) against the Python restatement of the contract (tests/junction_ref.py),
round-robin and under seeded schedules (the kernels use atomics); the `known` rule and the table writer through librsqc_host.so; the
command line's usage text and the refused multi-GPU combination."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from rnaseqc_amd import abi
from rnaseqc_amd.model import Batch
from tests import junction_cases as jc
from tests import junction_ref as ref
from tests.hostemu import junction as emu
from tests.test_cli import cli  # noqa: F401

SEEDS = [0, 7, 1234567]          # 0: round-robin


def _check(batches, want, q=255, cap0=65536, seed=0):
    got = emu.run(batches, jc.N_CONTIGS, mapq_threshold=q, cap0=cap0, seed=seed)
    assert got["error"] == 0
    ref.assert_tables_equal(got, want)
    return got


def test_fixture_a_stays_non_trivial():
    ann, reads = jc.fixture_a()
    w = jc.fixture_a_table()
    assert reads.n == w["records"] == 41_000 and w["population"] == 40_000
    assert w["instances"] > 10_000 and w["n"] > 300 and int(w["reads"].max()) > 1_000 and w["n_ops_excluded"] > 200
    assert (w["instances"], w["n"], int(w["reads"].max()), w["n_ops_excluded"], w["n_ops"] + w["n_ops_excluded"]) == (15_220, 402, 1_380, 246, 15_466)
    assert sorted(set(int(x) for x in reads.mapq)) == [0, 3, 255]
    assert 0 < int(w["hq_reads"].sum()) < w["instances"]


@pytest.mark.parametrize("seed", SEEDS)
def test_fixture_a_in_five_unequal_batches(seed):
    _, reads = jc.fixture_a()
    parts = jc.cut(reads)
    assert len(parts) == 5 and len(set(p.n for p in parts)) == 5
    got = _check(parts, jc.fixture_a_table(), seed=seed)
    assert got["passes"][0] >= 1 and got["passes"][1] >= 2       # both stages ran, dead digit positions were skipped
    assert got["passes"][0] <= 3 and got["passes"][1] <= 4


def test_fixture_a_other_order_other_cut_other_threshold():
    """The table does not depend on the order of the records or on the batches; the threshold moves hq_reads only."""
    _, reads = jc.fixture_a()
    shuffled = reads.take(np.random.default_rng(5).permutation(reads.n))
    _check(jc.cut(shuffled, seed=9, parts=3), jc.fixture_a_table(), seed=3)
    w4 = jc.fixture_a_table(3)                 # (the fixture's mapq values are 0, 3 and 255)
    assert int(w4["hq_reads"].sum()) > int(jc.fixture_a_table()["hq_reads"].sum())
    _check([reads], w4, q=3)


def test_growth_of_the_collection():
    """RSQC_JUNCTION_CAP0 = 1024: the collection grows to the host's bound (half the operations so far) in four steps, and what the
    earlier batches left survives every step."""
    _, reads = jc.fixture_a()
    got = _check(jc.cut(reads), jc.fixture_a_table(), cap0=1024, seed=11)
    assert got["grown"] == 4 and got["cap"] >= got["instances"]


def test_a_full_collection_is_an_error_never_a_partial_table():
    """Records of a single N each: the host's bound is half an operation per record, the instances do not fit, the flag is raised."""
    b = Batch.from_records([dict(tid=0, pos=100 + i, cigar=[(abi.CIG_N, 10)]) for i in range(600)])
    got = emu.run([b], jc.N_CONTIGS, cap0=256)
    assert got["error"] == emu.ERR_CAPACITY and got["n"] == 0
    assert emu.run([b], jc.N_CONTIGS, cap0=600)["error"] == 0


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("name", jc.CRAFTED_NAMES)
def test_crafted(name, seed):
    b, q, want = jc.crafted_case(name)
    _check([b], want, q=q, seed=seed)


def test_crafted_all_in_one_pass():
    """Every crafted case as a batch of ONE pass (threshold 255): rows of different batches merge."""
    batches = [jc.crafted_case(n)[0] for n in jc.CRAFTED_NAMES if n != "mapq_threshold_4"]
    _check(batches, ref.junction_table(batches, jc.N_CONTIGS, 255), seed=5)


# ---- host side: the `known` rule and the writer, through librsqc_host.so -------------------------------------------------------------
GTF = "\n".join([
    'chr1\tt\tgene\t100\t900\t.\t+\t.\tgene_id "G1"; gene_name "g1"; transcript_type "protein_coding";',
    'chr1\tt\texon\t100\t200\t.\t+\t.\tgene_id "G1"; transcript_id "T1"; gene_name "g1"; transcript_type "protein_coding";',
    'chr1\tt\texon\t301\t400\t.\t+\t.\tgene_id "G1"; transcript_id "T1"; gene_name "g1"; transcript_type "protein_coding";',
    'chr1\tt\texon\t701\t900\t.\t+\t.\tgene_id "G1"; transcript_id "T1"; gene_name "g1"; transcript_type "protein_coding";',
    'chr1\tt\tgene\t350\t1500\t.\t-\t.\tgene_id "G2"; gene_name "g2"; transcript_type "protein_coding";',
    'chr1\tt\texon\t350\t500\t.\t-\t.\tgene_id "G2"; transcript_id "T2"; gene_name "g2"; transcript_type "protein_coding";',
    'chr1\tt\texon\t1001\t1500\t.\t-\t.\tgene_id "G2"; transcript_id "T2"; gene_name "g2"; transcript_type "protein_coding";',
    'chr2\tt\tgene\t100\t400\t.\t+\t.\tgene_id "G3"; gene_name "g3"; transcript_type "protein_coding";',
    'chr2\tt\texon\t100\t200\t.\t+\t.\tgene_id "G3"; transcript_id "T3"; gene_name "g3"; transcript_type "protein_coding";',
    'chr2\tt\texon\t301\t400\t.\t+\t.\tgene_id "G3"; transcript_id "T3"; gene_name "g3"; transcript_type "protein_coding";',
]) + "\n"


@pytest.fixture(scope="module")
def host_lib():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call(["make", "-s", "-C", os.path.join(root, "rnaseqc_amd", "csrc"), "../lib/librsqc_host.so"])
    return C.CDLL(os.path.join(root, "rnaseqc_amd", "lib", "librsqc_host.so"))


def test_known_rule_and_writer(host_lib, tmp_path):
    gtf = tmp_path / "k.gtf"
    gtf.write_text(GTF)
    # (tid, start, end): G1's two introns and its exon-skipping one; G2's intron; G1's exon end with G2's exon start (another gene's
    # boundary: not known); a novel junction; G1's intron on the other contig of the header (chr2 has it through G3: known there);
    # a contig the GTF does not name
    rows = [(0, 201, 300, 1), (0, 201, 700, 1), (0, 401, 700, 1), (0, 501, 1000, 1), (0, 401, 1000, 0), (0, 201, 349, 0), (0, 250, 300, 0),
            (1, 201, 300, 1), (1, 401, 700, 0), (2, 201, 300, 0)]
    tid = np.array([r[0] for r in rows], np.int32); start = np.array([r[1] for r in rows], np.int32); end = np.array([r[2] for r in rows], np.int32)
    reads = np.arange(10, 10 + len(rows), dtype=np.uint32); hq = reads - np.uint32(3); ov = np.arange(70, 70 + len(rows), dtype=np.uint32)
    names = (C.c_char_p * 3)(b"chr1", b"chr2", b"chrUn")
    out = tmp_path / "x.junctions.tsv"
    host_lib.host_write_junctions.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_char_p), C.c_int, C.c_uint64] + [C.c_void_p] * 6
    host_lib.host_write_junctions.restype = C.c_int
    rc = host_lib.host_write_junctions(str(gtf).encode(), str(out).encode(), names, 3, len(rows), tid.ctypes.data, start.ctypes.data, end.ctypes.data,
                                            reads.ctypes.data, hq.ctypes.data, ov.ctypes.data)
    assert rc == 0
    table = dict(n=len(rows), tid=tid, start=start, end=end, reads=reads, hq_reads=hq, max_overhang=ov)
    want = ref.render(table, ["chr1", "chr2", "chrUn"], [r[3] for r in rows])
    assert out.read_text() == want
    assert want.splitlines()[0].split("\t") == ["contig", "start", "end", "reads", "hq_reads", "max_overhang", "known"]
    # an empty table: the header line alone
    rc = host_lib.host_write_junctions(str(gtf).encode(), str(out).encode(), names, 3, 0, None, None, None, None, None, None)
    assert rc == 0 and out.read_text() == ref.HEADER


def test_known_flags_of_the_reference_restatement():
    """tests/junction_ref.known_flags (what the GPU command-line test renders with) on fixture A's annotation: the reads are spliced
    at annotated exon boundaries, so most rows are known, and a shifted junction is not."""
    ann, _ = jc.fixture_a()
    w = jc.fixture_a_table()
    k = ref.known_flags(ann, w)
    assert k.sum() > len(k) // 2
    moved = dict(w, start=w["start"] + 1)
    assert ref.known_flags(ann, moved).sum() < k.sum()


# ---- the command line, without a GPU ---------------------------------------------------------------------------------------------------
def _run(cli, args, env=None):
    p = subprocess.run([cli, *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, **(env or {})), timeout=60)
    return p.returncode, p.stdout.decode(), p.stderr.decode()


def test_cli_usage_names_the_flag(cli):
    rc, so, se = _run(cli, ["--help"])
    assert "--junctions" in so + se


def test_cli_refuses_junctions_on_several_gpus(cli, tmp_path):
    """Exit 6 before any GPU work (no device is visible: a run that touched one would end with exit 10); no output directory."""
    gtf = tmp_path / "k.gtf"; gtf.write_text(GTF)
    bam = tmp_path / "none.bam"; bam.write_bytes(b"")
    hidden = dict(HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    for args, env in ((["--gpus=2", "--junctions"], {}), (["--junctions", "--gpus", "2"], {}), (["--junctions"], dict(RSQC_GPUS="2")), (["--junctions"], dict(RSQC_GPU_LIST="0,1"))):
        out = str(tmp_path / "refused")
        rc, _, se = _run(cli, args + [str(gtf), str(bam), out], env=dict(hidden, **env))
        assert rc == 6 and "Argument validation error: --junctions" in se, (args, rc, se)
        assert not os.path.exists(out)
