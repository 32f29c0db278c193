"""-m gpu: --gene-body on the command line, on fixture A of tests/junction_cases.py with a GTF variant that has overlapping exon rows
and reverse-strand genes.  The integer columns of <sample>.gene_body.tsv equal, byte for byte, those of the numpy restatement of the
contract (tests/genebody_ref.py over tests/track_ref.py) and norm_mean stays within the tolerance of tests/compare.py, for BAM and SAM
input, the device and the host decode, --sort, --bedgraph beside it and --bam-list; every other report file is byte-identical to a
run without the flag."""
import os
import subprocess

import numpy as np
import pytest

from rnaseqc_amd import abi, bamio, synth
from rnaseqc_amd.model import Annotation
from tests import compare
from tests import genebody_ref as ref
from tests import junction_cases as jc
from tests import track_cases as tc
from tests import track_ref
from tests.test_cli import cli  # noqa: F401

pytestmark = pytest.mark.gpu
BODY = "x.gene_body.tsv"
TRACK = "x.coverage.bedgraph"


def _run(cli, args, env=None, timeout=300):
    p = subprocess.run([cli, *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, **(env or {})), timeout=timeout)
    return p.returncode, p.stdout.decode(), p.stderr.decode()


def variant(ann):
    """Fixture A's annotation as GTF rows, every third gene with a second exon row that overlaps its first one and every fifth with
    one that abuts its last one."""
    rows = []
    for g, gid in enumerate(ann.gene_ids):
        i = int(np.flatnonzero(ann.gene_row_id == g)[0])
        strand = {0: "+", 1: "-", 2: "."}[int(ann.gene_row_flags[i]) & 3]
        contig = ann.contig_names[int(ann.gene_row_contig[i])]
        ex = [(int(ann.exon_row_start[r]), int(ann.exon_row_end[r])) for r in ann.gene_exon_row[int(ann.gene_exon_off[g]):int(ann.gene_exon_off[g + 1])]]
        if g % 3 == 0:
            ex.append((ex[0][0] + 10, ex[0][1] + 25))
        if g % 5 == 0:
            ex.append((ex[-1][1] + 1, ex[-1][1] + 40))
        rows.append(dict(contig=contig, type="gene", start=int(ann.gene_row_start[i]), end=max(int(ann.gene_row_end[i]), max(e for _, e in ex)), strand=strand, gene_id=gid, gene_name=ann.gene_names[g]))
        rows += [dict(contig=contig, type="exon", start=s, end=e, strand=strand, gene_id=gid, gene_name=ann.gene_names[g], exon_id="%s_x%d" % (gid, k)) for k, (s, e) in enumerate(ex)]
    return Annotation.from_rows(ann.contig_names[:ann.n_ref], rows)


class Case:
    pass


@pytest.fixture(scope="module")
def files(tmp_path_factory, cli):
    d = tmp_path_factory.mktemp("genebodyfiles")
    f = Case()
    f.dir = d
    ann, reads = jc.fixture_a()
    f.ann = variant(ann)
    assert (f.ann.exon_row_flags & 3 == abi.STRAND_REVERSE).any() and f.ann.n_exons > ann.n_exons + 30
    f.sorted = bamio.sam_consistent(reads.coordinate_sorted())
    f.shuffled = f.sorted.take(np.random.default_rng(73).permutation(f.sorted.n))
    f.paths = dict(gtf=str(d / "t.gtf"), bam=str(d / "sorted.bam"), shuf=str(d / "shuf.bam"), sam=str(d / "sorted.sam"))
    bamio.write_gtf(f.paths["gtf"], f.ann)
    bamio.write_bam(f.paths["bam"], jc.CS, f.sorted)
    bamio.write_bam(f.paths["shuf"], jc.CS, f.shuffled)
    bamio.write_sam(f.paths["sam"], jc.CS, f.sorted)
    f.track = track_ref.track([f.sorted], tc.A_LENGTHS)
    f.model = ref.model_from_annotation(f.ann, tc.A_LENGTHS)
    f.sums, f.info = ref.sums(ref.depth_arrays(f.track, tc.A_LENGTHS), f.model)
    f.want = ref.render(f.model, f.sums)
    n_el = int(ref.eligible(f.model, f.sums).sum())
    assert f.info["n_measured"] > 50 and n_el > 20 and f.info["depth_sum"] > 100_000 and int(f.model["reverse"].sum()) > 10
    assert len(f.model["seg_tid"]) < f.ann.n_exons - 30                 # (the overlapping and abutting rows were merged)
    # the run every other one is compared with: the sorted BAM without the flag
    f.plain_out = str(d / "plain")
    rc, _, se = _run(cli, [f.paths["gtf"], f.paths["bam"], f.plain_out, "-s", "x", "-v", "--coverage"])
    assert rc == 0, se
    return f


def _reports(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d))}


def _check_body(got, want):
    """The integer columns byte for byte; norm_mean as printed (%.6f) within the tolerance of tests/compare.py."""
    g, w = [l.split("\t") for l in got.decode().split("\n")], [l.split("\t") for l in want.split("\n")]
    assert len(g) == len(w) == 102 and g[0] == w[0] and g[-1] == w[-1] == [""]
    for a, b in zip(g[1:-1], w[1:-1]):
        assert a[:3] == b[:3] and len(a) == 4, (a, b)
        assert len(a[3].split(".")[1]) == 6
        assert np.isclose(float(a[3]), float(b[3]), rtol=compare.FLOAT_RTOL, atol=compare.FLOAT_ATOL), (a, b)


def _check_run(files, out, so, also=()):
    got = _reports(out)
    _check_body(got.pop(BODY), files.want)
    for name in also:
        got.pop(name)
    assert got == _reports(files.plain_out)                         # every other report file, byte for byte
    assert ref.verbose_line(files.model, files.sums, files.info) in so, so


def test_bam(cli, files):
    out = str(files.dir / "bam")
    rc, so, se = _run(cli, ["--gene-body", files.paths["gtf"], files.paths["bam"], out, "-s", "x", "-v", "--coverage"],
                      env=dict(RSQC_DECODE_CHUNK="65536", RSQC_DECODE_MAX_OUT="262144"))     # (many decode windows)
    assert rc == 0, se
    _check_run(files, out, so)
    assert TRACK not in os.listdir(out) and "Track:" not in so      # the track is built, its file belongs to --bedgraph
    assert BODY not in os.listdir(files.plain_out)


def test_host_decode(cli, files):
    out = str(files.dir / "host")
    rc, so, se = _run(cli, ["--gene-body", files.paths["gtf"], files.paths["bam"], out, "-s", "x", "-v", "--coverage"], env=dict(RSQC_DECODE="host", RSQC_BATCH="7000"))
    assert rc == 0, se
    _check_run(files, out, so)


def test_sam_text(cli, files):
    out = str(files.dir / "sam")
    rc, so, se = _run(cli, ["--gene-body", files.paths["gtf"], files.paths["sam"], out, "-s", "x", "-v", "--coverage"], env=dict(RSQC_SAM_CHUNK="100000"))
    assert rc == 0, se
    _check_run(files, out, so)


def test_shuffled_bam_with_sort(cli, files):
    out = str(files.dir / "sort")
    rc, so, se = _run(cli, ["--sort", "--gene-body", files.paths["gtf"], files.paths["shuf"], out, "-s", "x", "-v", "--coverage"], env=dict(RSQC_SORT_BATCH="9000"))
    assert rc == 0, se
    assert "was_sorted 0" in so
    _check_run(files, out, so)


def test_with_bedgraph(cli, files):
    """Both flags: both files; the bedgraph is the one of --bedgraph alone."""
    only_b = str(files.dir / "only_b")
    rc, _, se = _run(cli, ["--bedgraph", files.paths["gtf"], files.paths["bam"], only_b, "-s", "x", "-v", "--coverage"])
    assert rc == 0, se
    out = str(files.dir / "both")
    rc, so, se = _run(cli, ["--bedgraph", "--gene-body", files.paths["gtf"], files.paths["bam"], out, "-s", "x", "-v", "--coverage"])
    assert rc == 0, se
    assert _reports(out)[TRACK] == _reports(only_b)[TRACK] == track_ref.render(files.track, tc.A_NAMES)
    _check_run(files, out, so, also=(TRACK,))
    assert "Track: population 40000," in so


def test_bam_list_of_two_samples_with_other_lengths(cli, files):
    """Each sample of a cohort gets the model of ITS header (the second header's contigs have other lengths: the exon rows are clipped
    elsewhere and chrB and chrC start at other slots); a sample that fails gets no file."""
    d = files.dir
    cs2 = [("chrA", 640_000), ("chrB", 500_500), ("chrC", 300_010)]
    lengths2 = [c[1] for c in cs2]
    other = bamio.sam_consistent(synth.make_reads(jc.fixture_a()[0], 3000, seed=91, read_len=100, keep_qnames=True, contig_lengths=np.array(lengths2)).coordinate_sorted())
    other_bam = str(d / "other.bam")
    bamio.write_bam(other_bam, cs2, other)
    model2 = ref.model_from_annotation(files.ann, lengths2)
    assert len(model2["seg_tid"]) < len(files.model["seg_tid"])           # (chrA is shorter there: exon rows beyond it fall away)
    sums2, _ = ref.sums(ref.depth_arrays(track_ref.track([other], lengths2), lengths2), model2)
    lst = str(d / "list.txt")
    open(lst, "w").write("%s\tone\n%s\ttwo\n%s\tbroken\n" % (files.paths["bam"], other_bam, str(d / "missing.bam")))
    out = str(d / "cohort")
    rc, so, se = _run(cli, ["--gene-body", "--bam-list=" + lst, files.paths["gtf"], out])
    assert rc != 0                                                     # (the third sample cannot be opened)
    _check_body(open(os.path.join(out, "one.gene_body.tsv"), "rb").read(), files.want)
    _check_body(open(os.path.join(out, "two.gene_body.tsv"), "rb").read(), ref.render(model2, sums2))
    assert not os.path.exists(os.path.join(out, "broken.gene_body.tsv")) and not os.path.exists(os.path.join(out, "one.coverage.bedgraph"))


def test_refused_on_two_gpus(cli, files):
    out = str(files.dir / "refused")
    rc, _, se = _run(cli, ["--gene-body", "--gpus", "2", files.paths["gtf"], files.paths["bam"], out, "-s", "x"])
    assert rc == 6 and "Argument validation error: --gene-body" in se and not os.path.exists(out)


def test_sam_header_without_ln(cli, files):
    """A contig without a length: exit 10 with a message that names the flag and the contig, and no file."""
    text = open(files.paths["sam"]).read()
    assert "@SQ\tSN:chrB\tLN:500000\n" in text
    bad = str(files.dir / "no_ln.sam")
    open(bad, "w").write(text.replace("@SQ\tSN:chrB\tLN:500000\n", "@SQ\tSN:chrB\n", 1))
    out = str(files.dir / "no_ln")
    rc, so, se = _run(cli, ["--gene-body", files.paths["gtf"], bad, out, "-s", "x"])
    assert rc == 10 and "--gene-body" in se and "chrB" in se, (rc, se)
    assert not os.path.exists(os.path.join(out, BODY))
