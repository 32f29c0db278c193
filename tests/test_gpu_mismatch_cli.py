"""-m gpu: --mismatches on the command line.  The mixed stream of tests/mismatch_cases.py as BAM gives the three files of the Python
restatement of the contract (tests/mismatch_ref.py), byte for byte, and leaves every other report file as a run with the same --fasta and
without the flag writes it; the same three files come out under RSQC_DECODE=host, from the plain-SAM spelling and with --sort on a
shuffled copy; a cohort of two samples with one header gives each its own files; the refusals leave nothing behind."""
import os
import random
import subprocess

import pytest

from rnaseqc_amd import bamio, synth
from tests import mismatch_cases as mc
from tests import mismatch_ref as ref
from tests.test_cli import cli  # noqa: F401

pytestmark = pytest.mark.gpu

NEW = ["x.mismatch_cycles.tsv", "x.mismatch_quality.tsv", "x.mismatch_types.tsv"]


def _run(cli, args, env=None, timeout=300):
    p = subprocess.run([cli, *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, **(env or {})), timeout=timeout)
    return p.returncode, p.stdout.decode(), p.stderr.decode()


def _reports(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d))}


def _texts(tables):
    cyc, subst, byq, _ = tables
    return {"mismatch_cycles.tsv": ref.format_cycles(cyc).encode(), "mismatch_types.tsv": ref.format_types(subst).encode(), "mismatch_quality.tsv": ref.format_quality(byq).encode()}


class Case:
    pass


@pytest.fixture(scope="module")
def files(tmp_path_factory, cli):
    d = tmp_path_factory.mktemp("mismatchfiles")
    f = Case()
    f.dir = d
    ann = synth.make_annotation(seed=63, contigs=[("chrA", 21001, 0), ("chrB", 1003, 0), ("chrC", 500, 0), ("chrD", 500_000, 30)])
    records, _, _, whole = mc.mixed_tables()
    f.records, f.info, f.texts = mc.in_coordinate_order(records), whole[3], _texts(whole)
    f.paths = {k: str(d / v) for k, v in dict(gtf="m.gtf", fasta="ref.fa", bam="mixed.bam", sam="mixed.sam", shuffled="shuffled.bam", small="small.bam", lst="cohort.txt",
                                              other_ln="other_ln.bam").items()}
    bamio.write_gtf(f.paths["gtf"], ann)
    mc.write_fasta(f.paths["fasta"])
    mc.write_bam(f.paths["bam"], f.records)
    mc.write_sam(f.paths["sam"], f.records)
    order = list(range(len(f.records)))
    random.Random(5).shuffle(order)
    mc.write_bam(f.paths["shuffled"], [f.records[k] for k in order])
    # a second, different sample with the same header: the catalogue (without its BAM-only records: an operation code above 8 ends a run,
    # as it ends the reference's)
    f.small = mc.in_coordinate_order(mc.catalogue())
    f.small_texts = _texts(mc.catalogue_tables(False))
    mc.write_bam(f.paths["small"], f.small, block=4099)
    # the header says 1004 bases for chrB, the FASTA has 1003
    mc.write_bam(f.paths["other_ln"], f.small, contigs=[c if c[0] != "chrB" else ("chrB", 1004) for c in mc.CONTIGS])
    f.common = ["--fasta", f.paths["fasta"], "--mismatches-mapq=%d" % mc.MIN_MAPQ]
    f.plain_out = str(d / "plain")
    rc, _, se = _run(cli, ["--fasta", f.paths["fasta"], f.paths["gtf"], f.paths["bam"], f.plain_out, "-s", "x", "--coverage"])
    assert rc == 0, se
    return f


def _assert_files(out, f, sample="x", small=False):
    got = _reports(out)
    for name, text in (f.small_texts if small else f.texts).items():
        assert got[sample + "." + name] == text, name
    return got


def test_mismatches_on_the_mixed_bam(cli, files):
    out = str(files.dir / "bam")
    rc, so, se = _run(cli, ["--mismatches", *files.common, files.paths["gtf"], files.paths["bam"], out, "-s", "x", "-v", "--coverage"],
                      env=dict(RSQC_DECODE_CHUNK="65536", RSQC_DECODE_MAX_OUT="262144"))
    assert rc == 0, se
    got = _assert_files(out, files)
    want = _reports(files.plain_out)
    assert sorted(got) == sorted(list(want) + NEW) and len(want) >= 5
    for name in want:
        assert got[name] == want[name], name                          # every other report file: what a run with --fasta alone writes
    i = files.info
    assert ("Mismatches: records %d, no_reference %d, low_mapq %d, no_seq %d, inconsistent %d, compared %d, mismatched %d, uncompared %d, inserted %d, clipped %d, "
            "deletions %d, beyond %d, mismatch_ms " % (i["records"], i["no_reference_records"], i["low_mapq_records"], i["no_seq_records"], i["inconsistent_records"],
                                                       i["compared"], i["mismatched"], i["uncompared"], i["inserted"], i["clipped"], i["deletions"], i["beyond_bases"])) in so, so


@pytest.mark.parametrize("kind,args,env", [("bam", [], dict(RSQC_DECODE="host", RSQC_BATCH="700")), ("sam", [], dict(RSQC_SAM_CHUNK="50000")),
                                           ("shuffled", ["--sort"], {}), ("bam", ["--cycles", "--junctions", "--bedgraph", "--gene-body", "--tin"], {})],
                         ids=["host_decode", "plain_sam", "sort_shuffled", "with_the_other_extensions"])
def test_the_same_files_on_other_routes(cli, files, kind, args, env):
    out = str(files.dir / ("route_" + kind + "_".join(a.strip("-") for a in args) + ("_host" if env.get("RSQC_DECODE") else "")))
    rc, so, se = _run(cli, ["--mismatches", *files.common, *args, files.paths["gtf"], files.paths[kind], out, "-s", "x", "-v"], env=env)
    assert rc == 0, se
    _assert_files(out, files)
    assert "Mismatches: records %d," % files.info["records"] in so


def test_cohort_of_two_samples_with_one_header(cli, files):
    """Two different samples and a missing one between them: the failing sample gets no files, the others their own (the second on the
    reference the context packed for the first)."""
    with open(files.paths["lst"], "w") as f:
        f.write("%s\tbig\n%s\tgone\n%s\tlittle\n" % (files.paths["bam"], str(files.dir / "missing.bam"), files.paths["small"]))
    out = str(files.dir / "cohort")
    rc, so, se = _run(cli, ["--mismatches", *files.common, "--bam-list", files.paths["lst"], files.paths["gtf"], out, "-v"])
    assert rc == 10, (rc, se)
    got = _assert_files(out, files, sample="big")
    _assert_files(out, files, sample="little", small=True)
    assert not [n for n in got if n.startswith("gone.")]
    assert so.count("Mismatches: records ") == 2


@pytest.mark.parametrize("how", ["flag", "RSQC_GPUS", "RSQC_GPU_LIST", "no_fasta", "mapq_alone", "mapq_range"])
def test_refusals_exit_6(cli, files, how):
    out = str(files.dir / ("refused_" + how))
    args = ["--mismatches", "--fasta", files.paths["fasta"], files.paths["gtf"], files.paths["bam"], out, "-s", "x"]
    env, text = {}, "--mismatches runs on one GPU"
    if how == "flag":
        args += ["--gpus", "2"]
    elif how in ("RSQC_GPUS", "RSQC_GPU_LIST"):
        env = {how: "2" if how == "RSQC_GPUS" else "0,1"}
    elif how == "no_fasta":
        args, text = ["--mismatches"] + args[3:], "--fasta"
    elif how == "mapq_alone":
        args, text = ["--mismatches-mapq=5"] + args[1:], "--mismatches-mapq needs --mismatches"
    else:
        args, text = args + ["--mismatches-mapq=300"], "0..255"
    rc, so, se = _run(cli, args, env=env)
    assert rc == 6 and text in se and not os.path.exists(out), (rc, se)


def test_another_length_than_the_header_exits_10(cli, files):
    out = str(files.dir / "other_ln")
    rc, so, se = _run(cli, ["--mismatches", "--fasta", files.paths["fasta"], files.paths["gtf"], files.paths["other_ln"], out, "-s", "x"])
    assert rc == 10 and "--mismatches" in se and "chrB" in se, (rc, se)
    assert not os.path.exists(out) or not os.listdir(out)
