"""`rnaseqc --bam-list=FILE gtf output`: a list of samples through one process and one GPU context.  CPU: the argument and list
checks with the reference's exit-code classes.  GPU: every sample's report files equal those of a run of that sample alone."""
import os
import subprocess

import numpy as np
import pytest

from rnaseqc_amd import bamio, synth
from rnaseqc_amd.model import Batch
from tests import cases
from tests.test_cli import cli, run, _compare_tables  # noqa: F401
from tests.test_host_cli_pieces import read_table

CONTIGS = [("chrA", 900_000, 70), ("chrB", 500_000, 40)]
REPORTS = ["metrics.tsv", "gene_reads.gct", "gene_tpm.gct", "gene_fragments.gct", "exon_reads.gct", "coverage.tsv", "exon_cv.tsv", "fragmentSizes.txt"]
INTEGER_TABLES = ["gene_reads.gct", "gene_fragments.gct", "fragmentSizes.txt"]


def _env(**kw):
    env = {k: v for k, v in os.environ.items() if k not in ("RSQC_GPUS", "RSQC_GPU_LIST")}
    env.update(kw)
    return env


def _run(cli, *args, **env):
    p = subprocess.run([cli, *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=_env(**env))
    return p.returncode, p.stdout.decode(), p.stderr.decode()


def test_bam_list_validation_exit_codes(cli, tmp_path):
    ann, batch = cases.quirk_case()
    gtf, bam, out = str(tmp_path / "q.gtf"), str(tmp_path / "q.bam"), str(tmp_path / "o")
    bamio.write_gtf(gtf, ann)
    bamio.write_bam(bam, [("other1", 1000), ("other2", 1000)], batch.slice(0, 0))
    lst = tmp_path / "ok.list"
    lst.write_text("# a comment\n\nq.bam\n" + bam + "\tsecond\n")            # a relative path, a blank line, a named sample
    ok = "--bam-list=" + str(lst)
    assert "--bam-list" in _run(cli, "-h")[1]                                # in the usage text
    assert _run(cli, ok, gtf, out, "extra")[0] == 5                          # a third positional
    assert _run(cli, ok, gtf)[0] == 6                                        # no output directory
    assert _run(cli, ok, gtf, out, "--sample", "x")[0] == 6
    assert _run(cli, ok, gtf, out, "-s", "x")[0] == 6
    assert _run(cli, ok, gtf, out, "--gpus", "2")[0] == 6
    assert _run(cli, ok, gtf, out, RSQC_GPUS="2")[0] == 6
    assert _run(cli, ok, gtf, out, RSQC_GPU_LIST="0,1")[0] == 6
    empty = tmp_path / "empty.list"; empty.write_text("# nothing\n\n")
    assert _run(cli, "--bam-list", str(empty), gtf, out)[0] == 6
    twice = tmp_path / "twice.list"; twice.write_text(bam + "\n" + str(tmp_path / "elsewhere" / "q.bam") + "\n")
    rc, _, err = _run(cli, "--bam-list", str(twice), gtf, out)
    assert rc == 6 and "q.bam" in err                                        # the same default name (basename) twice
    named = tmp_path / "named.list"; named.write_text(bam + "\tx\n" + bam + "\tx\n")
    assert _run(cli, "--bam-list", str(named), gtf, out)[0] == 6
    assert _run(cli, "--bam-list", str(tmp_path / "missing.list"), gtf, out)[0] == 10
    assert not os.path.exists(out)                                           # all of it before anything is written
    assert _run(cli, ok, str(tmp_path / "missing.gtf"), out)[0] == 10       # a valid list, no GTF


def test_one_sample_exit_codes_are_unchanged(cli, tmp_path):
    """The invocations of test_cli.test_cli_exit_codes_without_gpu_work: three positionals, the same codes."""
    rc, out, _ = run(cli, "--version")
    assert rc == 0 and out.strip() == "RNASeQC 2.4.3"
    assert run(cli, "-h")[0] == 4
    assert run(cli)[0] == 6 and run(cli, "a.gtf", "b.bam")[0] == 6
    assert run(cli, "a", "b", "c", "--stranded", "xx")[0] == 6
    assert run(cli, "a", "b", "c", "--nope")[0] == 5 and run(cli, "a", "b", "c", "-q", "abc")[0] == 5
    assert run(cli, "a", "b", "c", "d")[0] == 5
    assert run(cli, str(tmp_path / "missing.gtf"), "b.bam", str(tmp_path / "o"))[0] == 10
    ann, batch = cases.quirk_case()
    gtf, bam = str(tmp_path / "q.gtf"), str(tmp_path / "q.bam")
    bamio.write_gtf(gtf, ann)
    assert run(cli, gtf, str(tmp_path / "missing.bam"), str(tmp_path / "o"))[0] == 10
    assert os.path.isdir(tmp_path / "o")
    bamio.write_bam(bam, [("other1", 1000), ("other2", 1000)], batch.slice(0, 0))
    assert run(cli, gtf, bam, str(tmp_path / "o"))[0] == 11
    fa = tmp_path / "r.fa"; fa.write_text(">chrA\nACGT\n")
    assert run(cli, gtf, bam, str(tmp_path / "o"), "--fasta", str(tmp_path / "missing.fa"))[0] == 10
    assert run(cli, gtf, bam, str(tmp_path / "o"), "--fasta", str(fa))[0] == 10
    empty = tmp_path / "e.gtf"; empty.write_text('c\tx\ttranscript\t1\t5\t.\t+\t.\tgene_id "A"; transcript_id "T";\n')
    assert run(cli, str(empty), bam, str(tmp_path / "o"))[0] == 11
    assert run(cli, "--bam-list=" + str(tmp_path / "missing.list"), gtf, str(tmp_path / "o"))[0] == 10


def _reads(ann, seed):
    return synth.make_reads(ann, 20000, seed=seed, keep_qnames=True, dup_frac=0.1, frac=(0.85, 0.06, 0.05, 0.04), expr_sigma=1.2,
                            contig_lengths=np.array([c[1] for c in CONTIGS]))


def _other_contig_order(batch):
    """The records of `batch` (header chrA, chrB) as a file whose header is chrB, chrA: chrB's records first, RefIDs swapped."""
    tid = batch.tid_per_record()
    a, b, rest = np.flatnonzero(tid == 0), np.flatnonzero(tid == 1), np.flatnonzero(tid < 0)
    assert len(a) and len(b) and (np.diff(a) == 1).all() and (np.diff(b) == 1).all()
    parts = [batch.slice(int(b[0]), int(b[-1]) + 1), batch.slice(int(a[0]), int(a[-1]) + 1)]
    if len(rest):
        parts.append(batch.slice(int(rest[0]), int(rest[-1]) + 1))
    out = Batch.concat(parts)
    out.seg_tid = np.where(out.seg_tid == 0, 1, np.where(out.seg_tid == 1, 0, out.seg_tid)).astype(np.int32)
    return out


def _same_reports(got_dir, want_dir, name, files):
    for f in files:
        got, want = os.path.join(got_dir, name + "." + f), os.path.join(want_dir, name + "." + f)
        assert os.path.exists(got) and os.path.exists(want), (name, f)
        if f in INTEGER_TABLES or f == "gc_content.tsv":
            assert open(got).read() == open(want).read(), (name, f)
        else:                                                   # (f64 atomics: the last bits depend on the order, run to run)
            _compare_tables(got, want, 3 if f.endswith(".gct") else 1, tol=1e-6)
    rows_got, rows_want = read_table(os.path.join(got_dir, name + ".metrics.tsv")), read_table(os.path.join(want_dir, name + ".metrics.tsv"))
    assert [r[0] for r in rows_got] == [r[0] for r in rows_want]
    n_int = 0
    for g, w in zip(rows_got, rows_want):
        if w[1].lstrip("-").isdigit():
            assert g[1] == w[1], (name, g, w)
            n_int += 1
    assert n_int > 20


@pytest.fixture(scope="module")
def cohort(tmp_path_factory):
    d = tmp_path_factory.mktemp("cohort")
    ann = synth.make_annotation(seed=41, contigs=CONTIGS)
    hdr = [(c[0], c[1]) for c in CONTIGS]
    gtf, bedp = str(d / "s.gtf"), str(d / "s.bed")
    bamio.write_gtf(gtf, ann)
    bamio.write_bed(bedp, ann, synth.make_bed(ann, min_len=250))
    batches = {k: _reads(ann, seed) for k, seed in (("a", 42), ("b", 52), ("c", 62), ("d", 72))}
    paths = {k: str(d / (k + (".sam" if k == "c" else ".bam"))) for k in "abcde"}
    bamio.write_bam(paths["a"], hdr, batches["a"])
    bamio.write_bam(paths["b"], hdr, batches["b"])                               # the same header: the context is only reset
    bamio.write_sam(paths["c"], hdr, batches["c"])                               # another format on the kept context
    batches["d"] = _other_contig_order(batches["d"])                             # another contig order + a contig the GTF lacks
    bamio.write_bam(paths["d"], [hdr[1], hdr[0], ("chrZ", 10_000)], batches["d"])
    bamio.write_bam(paths["e"], [("other1", 1000), ("other2", 1000)], batches["a"].slice(0, 0))   # no contig of the GTF
    return dict(dir=d, gtf=gtf, bed=bedp, paths=paths, n={k: batches[k].n for k in "abcd"})


@pytest.mark.gpu
def test_cohort_reports_equal_the_one_sample_runs(cli, cohort):
    d, paths = cohort["dir"], cohort["paths"]
    lst = d / "all.list"
    lst.write_text("a.bam\n" + paths["b"] + "\n" + paths["c"] + "\tsampleC\nd.bam\n# the one that fails\ne.bam\n")
    flags = ["--coverage", "--bed", cohort["bed"]]
    env = _env(RSQC_BATCH="30000")
    p = subprocess.run([cli, "--bam-list=" + str(lst), cohort["gtf"], str(d / "cohort"), *flags], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    err = p.stderr.decode()
    assert p.returncode == 11, err                                              # the first failing sample's code: (e)
    assert "e.bam: BAM file shares no contigs with GTF" in err
    names = {"a": "a.bam", "b": "b.bam", "c": "sampleC", "d": "d.bam"}
    for k in "abcd":
        extra = ["-s", "sampleC"] if k == "c" else []
        q = subprocess.run([cli, cohort["gtf"], paths[k], str(d / "single"), *flags, *extra], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
        assert q.returncode == 0, q.stderr.decode()
        _same_reports(str(d / "cohort"), str(d / "single"), names[k], REPORTS)
    assert not [f for f in os.listdir(d / "cohort") if f.startswith("e.bam")]
    rows = [l.rstrip("\n").split("\t") for l in open(d / "cohort" / "cohort.tsv")]
    assert rows[0] == ["sample", "input", "format", "records", "seconds", "exit_code"]
    assert [r[0] for r in rows[1:]] == ["a.bam", "b.bam", "sampleC", "d.bam", "e.bam"]
    assert [r[1] for r in rows[1:]] == [paths[k] for k in "abcde"]
    assert [r[2] for r in rows[1:]] == ["BAM", "BAM", "SAM text", "BAM", "BAM"]
    assert [int(r[3]) for r in rows[1:]] == [cohort["n"][k] for k in "abcd"] + [0]
    assert [int(r[5]) for r in rows[1:]] == [0, 0, 0, 0, 11]
    assert all(float(r[4]) > 0 for r in rows[1:5])


@pytest.mark.gpu
def test_cohort_with_fasta_replaces_the_reference_with_the_annotation(cli, cohort):
    d, paths = cohort["dir"], cohort["paths"]
    ref = synth.make_reference([CONTIGS[0][1]], seed=43)                         # chrA only: chrB is not in the FASTA index
    bamio.write_fasta(str(d / "ref.fa"), ["chrA"], ref, index_path=str(d / "ref.fai"))
    lst = d / "fasta.list"
    lst.write_text(paths["a"] + "\n" + paths["d"] + "\n")
    flags = ["--fasta", str(d / "ref.fa")]
    env = _env(RSQC_BATCH="30000")
    p = subprocess.run([cli, "--bam-list", str(lst), cohort["gtf"], str(d / "cohort_fa"), *flags], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    assert p.returncode == 0, p.stderr.decode()
    for k in "ad":
        q = subprocess.run([cli, cohort["gtf"], paths[k], str(d / "single_fa"), *flags], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
        assert q.returncode == 0, q.stderr.decode()
        _same_reports(str(d / "cohort_fa"), str(d / "single_fa"), k + ".bam", ["gc_content.tsv", "gene_reads.gct", "gene_fragments.gct", "metrics.tsv", "exon_cv.tsv"])
        assert sum(int(r[1]) for r in read_table(str(d / "cohort_fa" / (k + ".bam.gc_content.tsv")), 1)) > 500
