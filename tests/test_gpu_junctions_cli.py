"""-m gpu: --junctions on the command line.  <sample>.junctions.tsv equals the rendering of the Python restatement of the contract
(tests/junction_ref.py) for BAM and SAM input, the device and the host decode, --sort and --bam-list; every other report file is
byte-identical to a run without the flag."""
import os
import subprocess

import numpy as np
import pytest

from rnaseqc_amd import bamio, synth
from tests import junction_cases as jc
from tests import junction_ref as ref
from tests.test_cli import cli  # noqa: F401

pytestmark = pytest.mark.gpu
NAMES = [c[0] for c in jc.CONTIGS]


def _run(cli, args, env=None, timeout=300):
    p = subprocess.run([cli, *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, **(env or {})), timeout=timeout)
    return p.returncode, p.stdout.decode(), p.stderr.decode()


class Case:
    pass


@pytest.fixture(scope="module")
def files(tmp_path_factory, cli):
    d = tmp_path_factory.mktemp("junctionfiles")
    f = Case()
    f.dir = d
    f.ann, reads = jc.fixture_a()
    f.sorted = bamio.sam_consistent(reads.coordinate_sorted())
    f.shuffled = f.sorted.take(np.random.default_rng(73).permutation(f.sorted.n))
    f.paths = dict(gtf=str(d / "j.gtf"), bam=str(d / "sorted.bam"), shuf=str(d / "shuf.bam"), sam=str(d / "sorted.sam"))
    bamio.write_gtf(f.paths["gtf"], f.ann)
    bamio.write_bam(f.paths["bam"], jc.CS, f.sorted)
    bamio.write_bam(f.paths["shuf"], jc.CS, f.shuffled)
    bamio.write_sam(f.paths["sam"], jc.CS, f.sorted)
    table = ref.junction_table([f.sorted], jc.N_CONTIGS, 255)
    ref.assert_tables_equal(table, jc.fixture_a_table())           # (making the records SAM-consistent moves no junction)
    f.table = table
    f.want = ref.render(table, NAMES, ref.known_flags(f.ann, table))
    assert f.want.count("\n") == 1 + 402 and "\t1\n" in f.want
    # the run every other one is compared with: the sorted BAM without the flag
    f.plain_out = str(d / "plain")
    rc, _, se = _run(cli, [f.paths["gtf"], f.paths["bam"], f.plain_out, "-s", "x", "-v", "--coverage"])
    assert rc == 0, se
    return f


def _reports(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d))}


def _check_run(files, out, so):
    got = _reports(out)
    assert got.pop("x.junctions.tsv").decode() == files.want
    assert got == _reports(files.plain_out)                         # every other report file, byte for byte
    assert "Junctions: population 40000, instances 15220, rows 402, extract_ms" in so, so


def test_bam(cli, files):
    out = str(files.dir / "bam")
    rc, so, se = _run(cli, ["--junctions", files.paths["gtf"], files.paths["bam"], out, "-s", "x", "-v", "--coverage"],
                      env=dict(RSQC_DECODE_CHUNK="65536", RSQC_DECODE_MAX_OUT="262144"))     # (many decode windows)
    assert rc == 0, se
    _check_run(files, out, so)
    assert "x.junctions.tsv" not in os.listdir(files.plain_out)


def test_shuffled_bam_with_sort(cli, files):
    out = str(files.dir / "sort")
    rc, so, se = _run(cli, ["--sort", "--junctions", files.paths["gtf"], files.paths["shuf"], out, "-s", "x", "-v", "--coverage"], env=dict(RSQC_SORT_BATCH="9000"))
    assert rc == 0, se
    assert "Sorted on the GPU: records 41000," in so and "was_sorted 0" in so
    _check_run(files, out, so)


def test_sam_text(cli, files):
    out = str(files.dir / "sam")
    rc, so, se = _run(cli, ["--junctions", files.paths["gtf"], files.paths["sam"], out, "-s", "x", "-v", "--coverage"], env=dict(RSQC_SAM_CHUNK="100000"))
    assert rc == 0, se
    _check_run(files, out, so)


def test_host_decode(cli, files):
    out = str(files.dir / "host")
    rc, so, se = _run(cli, ["--junctions", files.paths["gtf"], files.paths["bam"], out, "-s", "x", "-v", "--coverage"], env=dict(RSQC_DECODE="host", RSQC_BATCH="7000"))
    assert rc == 0, se
    _check_run(files, out, so)


def test_bam_list_of_two_samples(cli, files):
    """Each sample of a cohort gets its own table; a sample that fails gets none."""
    d = files.dir
    other = bamio.sam_consistent(synth.make_reads(files.ann, 3000, seed=91, read_len=100, keep_qnames=True, contig_lengths=jc.LENGTHS).coordinate_sorted())
    other_bam = str(d / "other.bam")
    bamio.write_bam(other_bam, jc.CS, other)
    t2 = ref.junction_table([other], jc.N_CONTIGS, 255)
    assert 0 < t2["n"] != files.table["n"]
    want2 = ref.render(t2, NAMES, ref.known_flags(files.ann, t2))
    lst = str(d / "list.txt")
    open(lst, "w").write("%s\tone\n%s\ttwo\n%s\tbroken\n" % (files.paths["bam"], other_bam, str(d / "missing.bam")))
    out = str(d / "cohort")
    rc, so, se = _run(cli, ["--junctions", "--bam-list=" + lst, files.paths["gtf"], out])
    assert rc != 0                                                     # (the third sample cannot be opened)
    assert open(os.path.join(out, "one.junctions.tsv")).read() == files.want
    assert open(os.path.join(out, "two.junctions.tsv")).read() == want2
    assert not os.path.exists(os.path.join(out, "broken.junctions.tsv"))
