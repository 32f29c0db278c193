"""-m gpu: --bedgraph on the command line.  <sample>.coverage.bedgraph equals, byte for byte, the text of the numpy restatement of
the contract (tests/track_ref.py) for BAM and SAM input, the device and the host decode, --sort, --junctions and --bam-list; every
other report file is byte-identical to a run without the flag."""
import os
import subprocess

import numpy as np
import pytest

from rnaseqc_amd import bamio, synth
from tests import junction_cases as jc
from tests import track_cases as tc
from tests import track_ref as ref
from tests.test_cli import cli  # noqa: F401

pytestmark = pytest.mark.gpu
TRACK = "x.coverage.bedgraph"


def _run(cli, args, env=None, timeout=300):
    p = subprocess.run([cli, *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, **(env or {})), timeout=timeout)
    return p.returncode, p.stdout.decode(), p.stderr.decode()


class Case:
    pass


@pytest.fixture(scope="module")
def files(tmp_path_factory, cli):
    d = tmp_path_factory.mktemp("trackfiles")
    f = Case()
    f.dir = d
    f.ann, reads = jc.fixture_a()
    f.sorted = bamio.sam_consistent(reads.coordinate_sorted())
    f.shuffled = f.sorted.take(np.random.default_rng(73).permutation(f.sorted.n))
    f.paths = dict(gtf=str(d / "t.gtf"), bam=str(d / "sorted.bam"), shuf=str(d / "shuf.bam"), sam=str(d / "sorted.sam"))
    bamio.write_gtf(f.paths["gtf"], f.ann)
    bamio.write_bam(f.paths["bam"], jc.CS, f.sorted)
    bamio.write_bam(f.paths["shuf"], jc.CS, f.shuffled)
    bamio.write_sam(f.paths["sam"], jc.CS, f.sorted)
    f.track = ref.track([f.sorted], tc.A_LENGTHS)
    ref.assert_tracks_equal(f.track, tc.fixture_a_track())           # (making the records SAM-consistent moves no aligned base)
    f.want = ref.render(f.track, tc.A_NAMES)
    assert f.want.count(b"\n") == f.track["n_rows"] > 1000
    # the run every other one is compared with: the sorted BAM without the flag
    f.plain_out = str(d / "plain")
    rc, _, se = _run(cli, [f.paths["gtf"], f.paths["bam"], f.plain_out, "-s", "x", "-v", "--coverage"])
    assert rc == 0, se
    return f


def _reports(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d))}


def _check_run(files, out, so):
    got = _reports(out)
    assert got.pop(TRACK) == files.want
    assert got == _reports(files.plain_out)                         # every other report file, byte for byte
    t = files.track
    assert "Track: population %d, aligned_bases %d, clipped_bases 0, rows %d, events_ms" % (t["population"], t["aligned_bases"], t["n_rows"]) in so, so
    assert "scan_ms" in so and "rows_ms" in so


def test_bam(cli, files):
    out = str(files.dir / "bam")
    rc, so, se = _run(cli, ["--bedgraph", files.paths["gtf"], files.paths["bam"], out, "-s", "x", "-v", "--coverage"],
                      env=dict(RSQC_DECODE_CHUNK="65536", RSQC_DECODE_MAX_OUT="262144"))     # (many decode windows)
    assert rc == 0, se
    _check_run(files, out, so)
    assert TRACK not in os.listdir(files.plain_out)


def test_host_decode(cli, files):
    out = str(files.dir / "host")
    rc, so, se = _run(cli, ["--bedgraph", files.paths["gtf"], files.paths["bam"], out, "-s", "x", "-v", "--coverage"], env=dict(RSQC_DECODE="host", RSQC_BATCH="7000"))
    assert rc == 0, se
    _check_run(files, out, so)


def test_sam_text(cli, files):
    out = str(files.dir / "sam")
    rc, so, se = _run(cli, ["--bedgraph", files.paths["gtf"], files.paths["sam"], out, "-s", "x", "-v", "--coverage"], env=dict(RSQC_SAM_CHUNK="100000"))
    assert rc == 0, se
    _check_run(files, out, so)


def test_shuffled_bam_with_sort(cli, files):
    out = str(files.dir / "sort")
    rc, so, se = _run(cli, ["--sort", "--bedgraph", files.paths["gtf"], files.paths["shuf"], out, "-s", "x", "-v", "--coverage"], env=dict(RSQC_SORT_BATCH="9000"))
    assert rc == 0, se
    assert "Sorted on the GPU: records 41000," in so and "was_sorted 0" in so
    _check_run(files, out, so)


def test_with_junctions(cli, files):
    """Both flags: both files, each equal to its single-flag run."""
    only_j = str(files.dir / "only_j")
    rc, _, se = _run(cli, ["--junctions", files.paths["gtf"], files.paths["bam"], only_j, "-s", "x", "-v", "--coverage"])
    assert rc == 0, se
    out = str(files.dir / "both")
    rc, so, se = _run(cli, ["--bedgraph", "--junctions", files.paths["gtf"], files.paths["bam"], out, "-s", "x", "-v", "--coverage"])
    assert rc == 0, se
    got = _reports(out)
    assert got["x.junctions.tsv"] == _reports(only_j)["x.junctions.tsv"] and len(got.pop("x.junctions.tsv")) > 1000
    assert got.pop(TRACK) == files.want
    assert got == _reports(files.plain_out)
    assert "Junctions: population 40000," in so and "Track: population 40000," in so


def test_bam_list_of_two_samples_with_other_lengths(cli, files):
    """Each sample of a cohort gets its own track over ITS header's lengths (the second header's contigs are longer: the array of the
    first sample does not hold them, and chrB and chrC start at other slots); a sample that fails gets no file."""
    d = files.dir
    cs2 = [("chrA", 900_500), ("chrB", 500_000), ("chrC", 300_010)]
    lengths2 = [c[1] for c in cs2]
    other = bamio.sam_consistent(synth.make_reads(files.ann, 3000, seed=91, read_len=100, keep_qnames=True, contig_lengths=np.array(lengths2)).coordinate_sorted())
    other_bam = str(d / "other.bam")
    bamio.write_bam(other_bam, cs2, other)
    t2 = ref.track([other], lengths2)
    assert 0 < t2["n_rows"] != files.track["n_rows"]
    lst = str(d / "list.txt")
    open(lst, "w").write("%s\tone\n%s\ttwo\n%s\tbroken\n" % (files.paths["bam"], other_bam, str(d / "missing.bam")))
    out = str(d / "cohort")
    rc, so, se = _run(cli, ["--bedgraph", "--bam-list=" + lst, files.paths["gtf"], out])
    assert rc != 0                                                     # (the third sample cannot be opened)
    assert open(os.path.join(out, "one.coverage.bedgraph"), "rb").read() == files.want
    assert open(os.path.join(out, "two.coverage.bedgraph"), "rb").read() == ref.render(t2, tc.A_NAMES)
    assert not os.path.exists(os.path.join(out, "broken.coverage.bedgraph"))


def test_sam_header_without_ln(cli, files):
    """A contig without a length: exit 10 with a message that names it, and no track file."""
    text = open(files.paths["sam"]).read()
    assert "@SQ\tSN:chrB\tLN:500000\n" in text
    bad = str(files.dir / "no_ln.sam")
    open(bad, "w").write(text.replace("@SQ\tSN:chrB\tLN:500000\n", "@SQ\tSN:chrB\n", 1))
    out = str(files.dir / "no_ln")
    rc, so, se = _run(cli, ["--bedgraph", files.paths["gtf"], bad, out, "-s", "x"])
    assert rc == 10 and "--bedgraph" in se and "chrB" in se, (rc, se)
    assert not os.path.exists(os.path.join(out, TRACK))
