"""-m gpu: --tin on the command line, on fixture A of tests/junction_cases.py with the GTF variant of tests/test_gpu_genebody_cli.py
(overlapping and abutting exon rows, reverse-strand genes).  gene_id and the integer columns of <sample>.tin.tsv equal, as text, those
of the restatement of the contract (tests/tin_ref.py over tests/track_ref.py); mean_depth and tin, and the summary's three figures,
stay within 1e-6 of it, for BAM and SAM input, the device and the host decode, --sort, --gene-body and --bedgraph beside it and
--bam-list; every other report file is byte-identical to a run without the flag."""
import os
import subprocess

import numpy as np
import pytest

from rnaseqc_amd import bamio, synth
from tests import compare
from tests import junction_cases as jc
from tests import tin_ref as ref
from tests import track_cases as tc
from tests import track_ref
from tests.test_cli import cli  # noqa: F401
from tests.test_gpu_genebody_cli import variant

pytestmark = pytest.mark.gpu
TIN, SUMMARY = "x.tin.tsv", "x.tin_summary.tsv"
BODY, TRACK = "x.gene_body.tsv", "x.coverage.bedgraph"


def _run(cli, args, env=None, timeout=300):
    p = subprocess.run([cli, *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, **(env or {})), timeout=timeout)
    return p.returncode, p.stdout.decode(), p.stderr.decode()


class Case:
    pass


def _gct_ids(path):
    """The first column of a GCT file's rows (behind its three header lines)."""
    return [l.split("\t")[0] for l in open(path).read().split("\n")[3:] if l]


@pytest.fixture(scope="module")
def files(tmp_path_factory, cli):
    d = tmp_path_factory.mktemp("tinfiles")
    f = Case()
    f.dir = d
    ann, reads = jc.fixture_a()
    f.ann = variant(ann)
    f.sorted = bamio.sam_consistent(reads.coordinate_sorted())
    f.shuffled = f.sorted.take(np.random.default_rng(73).permutation(f.sorted.n))
    f.paths = dict(gtf=str(d / "t.gtf"), bam=str(d / "sorted.bam"), shuf=str(d / "shuf.bam"), sam=str(d / "sorted.sam"))
    bamio.write_gtf(f.paths["gtf"], f.ann)
    bamio.write_bam(f.paths["bam"], jc.CS, f.sorted)
    bamio.write_bam(f.paths["shuf"], jc.CS, f.shuffled)
    bamio.write_sam(f.paths["sam"], jc.CS, f.sorted)
    f.track = track_ref.track([f.sorted], tc.A_LENGTHS)
    f.model = ref.model_from_annotation(f.ann, tc.A_LENGTHS)
    f.L = ref.gene_lengths(f.model)
    f.rows, f.info = ref.rows(ref.depth_arrays(f.track, tc.A_LENGTHS), f.model)
    # the run every other one is compared with: the sorted BAM without the flag
    f.plain_out = str(d / "plain")
    rc, _, se = _run(cli, [f.paths["gtf"], f.paths["bam"], f.plain_out, "-s", "x", "-v", "--coverage"])
    assert rc == 0, se
    f.ids = _gct_ids(os.path.join(f.plain_out, "x.gene_reads.gct"))
    assert len(f.ids) == len(f.L) == f.info["n_genes"]
    f.want, f.want_summary = ref.render(f.ids, f.L, f.rows), ref.render_summary(f.L, f.rows)
    _, tin, el = ref.values(f.L, f.rows)
    assert f.info["n_measured"] > 50 and int(el.sum()) > 20 and f.info["depth_sum"] > 100_000 and 0 < tin[el].min() < tin[el].max() <= 100 + 1e-9
    return f


def _reports(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d))}


def _check_text(got, want, floats):
    """Ids and integer columns as text; the last `floats` columns as printed (%.6f) within the 1e-6 of tests/compare.py, the project's bound for
    floating report values (its relative 1e-9 absorbs a last printed digit that rounds the other way)."""
    g, w = [l.split("\t") for l in got.decode().split("\n")], [l.split("\t") for l in want.split("\n")]
    assert len(g) == len(w) and g[0] == w[0] and g[-1] == w[-1] == [""]
    for a, b in zip(g[1:-1], w[1:-1]):
        assert len(a) == len(b), (a, b)
        for k, (x, y) in enumerate(zip(a, b)):
            if k >= len(a) - floats:
                assert len(x.split(".")[1]) == 6 and np.isclose(float(x), float(y), rtol=compare.FLOAT_RTOL, atol=compare.FLOAT_ATOL), (a, b)
            else:
                assert x == y, (a, b)


def _check_run(files, out, so, also=()):
    got = _reports(out)
    _check_text(got.pop(TIN), files.want, 2)
    _check_text(got.pop(SUMMARY), files.want_summary, 3)
    for name in also:
        got.pop(name)
    assert got == _reports(files.plain_out)                         # every other report file, byte for byte
    assert ref.verbose_line(files.L, files.rows, files.info) in so, so


def test_bam(cli, files):
    out = str(files.dir / "bam")
    rc, so, se = _run(cli, ["--tin", files.paths["gtf"], files.paths["bam"], out, "-s", "x", "-v", "--coverage"],
                      env=dict(RSQC_DECODE_CHUNK="65536", RSQC_DECODE_MAX_OUT="262144"))     # (many decode windows)
    assert rc == 0, se
    _check_run(files, out, so)
    assert TRACK not in os.listdir(out) and "Track:" not in so and BODY not in os.listdir(out) and "Gene body:" not in so
    assert TIN not in os.listdir(files.plain_out) and SUMMARY not in os.listdir(files.plain_out)


def test_host_decode(cli, files):
    out = str(files.dir / "host")
    rc, so, se = _run(cli, ["--tin", files.paths["gtf"], files.paths["bam"], out, "-s", "x", "-v", "--coverage"], env=dict(RSQC_DECODE="host", RSQC_BATCH="7000"))
    assert rc == 0, se
    _check_run(files, out, so)


def test_sam_text(cli, files):
    out = str(files.dir / "sam")
    rc, so, se = _run(cli, ["--tin", files.paths["gtf"], files.paths["sam"], out, "-s", "x", "-v", "--coverage"], env=dict(RSQC_SAM_CHUNK="100000"))
    assert rc == 0, se
    _check_run(files, out, so)


def test_shuffled_bam_with_sort(cli, files):
    out = str(files.dir / "sort")
    rc, so, se = _run(cli, ["--sort", "--tin", files.paths["gtf"], files.paths["shuf"], out, "-s", "x", "-v", "--coverage"], env=dict(RSQC_SORT_BATCH="9000"))
    assert rc == 0, se
    assert "was_sorted 0" in so
    _check_run(files, out, so)


def test_with_gene_body_and_bedgraph(cli, files):
    """All three flags: gene_body.tsv and the bedgraph are those of a run without --tin."""
    without = str(files.dir / "without")
    rc, _, se = _run(cli, ["--gene-body", "--bedgraph", files.paths["gtf"], files.paths["bam"], without, "-s", "x", "-v", "--coverage"])
    assert rc == 0, se
    out = str(files.dir / "all3")
    rc, so, se = _run(cli, ["--tin", "--gene-body", "--bedgraph", files.paths["gtf"], files.paths["bam"], out, "-s", "x", "-v", "--coverage"])
    assert rc == 0, se
    got, base = _reports(out), _reports(without)
    assert got[BODY] == base[BODY] and got[TRACK] == base[TRACK] == track_ref.render(files.track, tc.A_NAMES)
    _check_run(files, out, so, also=(BODY, TRACK))
    assert "Track: population 40000," in so and "Gene body: genes" in so


def test_bam_list_of_two_samples_with_other_lengths(cli, files):
    """Each sample of a cohort gets the model of ITS header (the second header's contigs have other lengths); a sample that fails gets
    no file."""
    d = files.dir
    cs2 = [("chrA", 640_000), ("chrB", 500_500), ("chrC", 300_010)]
    lengths2 = [c[1] for c in cs2]
    other = bamio.sam_consistent(synth.make_reads(jc.fixture_a()[0], 3000, seed=91, read_len=100, keep_qnames=True, contig_lengths=np.array(lengths2)).coordinate_sorted())
    other_bam = str(d / "other.bam")
    bamio.write_bam(other_bam, cs2, other)
    model2 = ref.model_from_annotation(files.ann, lengths2)
    assert len(model2["seg_tid"]) < len(files.model["seg_tid"])           # (chrA is shorter there: exon rows beyond it fall away)
    L2 = ref.gene_lengths(model2)
    rows2, _ = ref.rows(ref.depth_arrays(track_ref.track([other], lengths2), lengths2), model2)
    lst = str(d / "list.txt")
    open(lst, "w").write("%s\tone\n%s\ttwo\n%s\tbroken\n" % (files.paths["bam"], other_bam, str(d / "missing.bam")))
    out = str(d / "cohort")
    rc, so, se = _run(cli, ["--tin", "--bam-list=" + lst, files.paths["gtf"], out])
    assert rc != 0                                                     # (the third sample cannot be opened)
    _check_text(open(os.path.join(out, "one.tin.tsv"), "rb").read(), files.want, 2)
    _check_text(open(os.path.join(out, "one.tin_summary.tsv"), "rb").read(), files.want_summary, 3)
    _check_text(open(os.path.join(out, "two.tin.tsv"), "rb").read(), ref.render(files.ids, L2, rows2), 2)
    _check_text(open(os.path.join(out, "two.tin_summary.tsv"), "rb").read(), ref.render_summary(L2, rows2), 3)
    assert not os.path.exists(os.path.join(out, "broken.tin.tsv")) and not os.path.exists(os.path.join(out, "broken.tin_summary.tsv"))
    assert not os.path.exists(os.path.join(out, "one.coverage.bedgraph")) and not os.path.exists(os.path.join(out, "one.gene_body.tsv"))


def test_refused_on_two_gpus(cli, files):
    out = str(files.dir / "refused")
    rc, _, se = _run(cli, ["--tin", "--gpus", "2", files.paths["gtf"], files.paths["bam"], out, "-s", "x"])
    assert rc == 6 and "--tin runs on one GPU" in se and not os.path.exists(out)


def test_sam_header_without_ln(cli, files):
    """A contig without a length: exit 10 with a message that names the flag and the contig, and no file."""
    text = open(files.paths["sam"]).read()
    assert "@SQ\tSN:chrB\tLN:500000\n" in text
    bad = str(files.dir / "no_ln.sam")
    open(bad, "w").write(text.replace("@SQ\tSN:chrB\tLN:500000\n", "@SQ\tSN:chrB\n", 1))
    out = str(files.dir / "no_ln")
    rc, so, se = _run(cli, ["--tin", files.paths["gtf"], bad, out, "-s", "x"])
    assert rc == 10 and "--tin needs" in se and "chrB" in se, (rc, se)
    assert not os.path.exists(os.path.join(out, TIN)) and not os.path.exists(os.path.join(out, SUMMARY))
