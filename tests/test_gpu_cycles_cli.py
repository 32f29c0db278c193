"""-m gpu: --cycles on the command line.  The mixed stream of tests/cycle_cases.py as BAM gives the two files of the Python restatement of
the contract (tests/cycle_ref.py), byte for byte, and leaves every other report file as a run without the flag writes it; the same two
files come out under RSQC_DECODE=host, from the plain-SAM spelling, with --sort on a shuffled copy and with --mark-duplicates; a cohort
gives each sample its own files; --gpus 2 is refused before anything is written."""
import os
import random
import subprocess

import pytest

from rnaseqc_amd import bamio, synth
from tests import cycle_cases as cc
from tests import cycle_ref as ref
from tests.test_cli import cli  # noqa: F401

pytestmark = pytest.mark.gpu


def _run(cli, args, env=None, timeout=300):
    p = subprocess.run([cli, *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, **(env or {})), timeout=timeout)
    return p.returncode, p.stdout.decode(), p.stderr.decode()


def _reports(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d))}


class Case:
    pass


@pytest.fixture(scope="module")
def files(tmp_path_factory, cli):
    d = tmp_path_factory.mktemp("cyclefiles")
    f = Case()
    f.dir = d
    ann = synth.make_annotation(seed=63, contigs=[("chrA", 1_000_000, 80), ("chrB", 500_000, 30)])
    f.records, _, _, (base, qual, f.info) = cc.mixed_tables()
    f.positions = [100 + 40 * k for k in range(len(f.records))]
    f.bases_text, f.quality_text = ref.format_bases(base).encode(), ref.format_quality(base, qual).encode()
    f.paths = {k: str(d / v) for k, v in dict(gtf="m.gtf", bam="mixed.bam", sam="mixed.sam", shuffled="shuffled.bam", small="small.bam", lst="cohort.txt").items()}
    bamio.write_gtf(f.paths["gtf"], ann)
    cc.write_bam(f.paths["bam"], f.records, positions=f.positions)
    cc.write_sam(f.paths["sam"], f.records, positions=f.positions)
    order = list(range(len(f.records)))
    random.Random(5).shuffle(order)
    cc.write_bam(f.paths["shuffled"], [f.records[k] for k in order], positions=[f.positions[k] for k in order])
    # a second, different sample: the catalogue (BAM-only records included), all at one position
    f.small = cc.catalogue(bam_only=True)
    sb, sq, _ = ref.tables(f.small)
    f.small_bases_text, f.small_quality_text = ref.format_bases(sb).encode(), ref.format_quality(sb, sq).encode()
    cc.write_bam(f.paths["small"], f.small, block=4099)
    f.plain_out = str(d / "plain")
    rc, _, se = _run(cli, [f.paths["gtf"], f.paths["bam"], f.plain_out, "-s", "x", "--coverage"])
    assert rc == 0, se
    return f


def _assert_cycle_files(out, f, sample="x", small=False):
    got = _reports(out)
    assert got[sample + ".cycle_bases.tsv"] == (f.small_bases_text if small else f.bases_text)
    assert got[sample + ".cycle_quality.tsv"] == (f.small_quality_text if small else f.quality_text)
    return got


def test_cycles_on_the_mixed_bam(cli, files):
    out = str(files.dir / "bam")
    rc, so, se = _run(cli, ["--cycles", files.paths["gtf"], files.paths["bam"], out, "-s", "x", "-v", "--coverage"], env=dict(RSQC_DECODE_CHUNK="65536", RSQC_DECODE_MAX_OUT="262144"))
    assert rc == 0, se
    got = _assert_cycle_files(out, files)
    want = _reports(files.plain_out)
    assert sorted(got) == sorted(list(want) + ["x.cycle_bases.tsv", "x.cycle_quality.tsv"]) and len(want) >= 5
    for name in want:
        assert got[name] == want[name], name                          # every other report file: what a run without the flag writes
    i = files.info
    assert ("Cycles: records %d, no_seq %d, no_qual %d, bases %d, beyond %d, clamped %d, cycles_ms " % (
        i["records"], i["no_seq_records"], i["no_qual_records"], i["bases"], i["beyond_bases"], i["clamped_quals"])) in so, so


@pytest.mark.parametrize("kind,args,env", [("bam", [], dict(RSQC_DECODE="host", RSQC_BATCH="700")), ("sam", [], dict(RSQC_SAM_CHUNK="50000")),
                                           ("shuffled", ["--sort"], {}), ("bam", ["--mark-duplicates"], {}),
                                           ("bam", ["--junctions", "--bedgraph", "--gene-body", "--tin"], {})],
                         ids=["host_decode", "plain_sam", "sort_shuffled", "mark_duplicates", "with_the_other_extensions"])
def test_the_same_files_on_other_routes(cli, files, kind, args, env):
    out = str(files.dir / ("route_" + kind + "_".join(a.strip("-") for a in args) + ("_host" if env.get("RSQC_DECODE") else "")))
    rc, so, se = _run(cli, ["--cycles", *args, files.paths["gtf"], files.paths[kind], out, "-s", "x", "-v"], env=env)
    assert rc == 0, se
    _assert_cycle_files(out, files)
    assert "Cycles: records %d," % files.info["records"] in so


def test_cohort_gives_each_sample_its_own_files(cli, files):
    """Two different samples and a missing one between them: the failing sample gets no files, the others their own."""
    with open(files.paths["lst"], "w") as f:
        f.write("%s\tbig\n%s\tgone\n%s\tlittle\n" % (files.paths["bam"], str(files.dir / "missing.bam"), files.paths["small"]))
    out = str(files.dir / "cohort")
    rc, so, se = _run(cli, ["--cycles", "--bam-list", files.paths["lst"], files.paths["gtf"], out])
    assert rc == 10, (rc, se)
    got = _assert_cycle_files(out, files, sample="big")
    _assert_cycle_files(out, files, sample="little", small=True)
    assert not [n for n in got if n.startswith("gone.")]


@pytest.mark.parametrize("how", ["flag", "RSQC_GPUS", "RSQC_GPU_LIST"])
def test_more_than_one_gpu_is_refused(cli, files, how):
    out = str(files.dir / ("refused_" + how))
    args = ["--cycles", files.paths["gtf"], files.paths["bam"], out, "-s", "x"] + (["--gpus", "2"] if how == "flag" else [])
    env = {} if how == "flag" else {how: "2" if how == "RSQC_GPUS" else "0,1"}
    rc, so, se = _run(cli, args, env=env)
    assert rc == 6 and "--cycles runs on one GPU" in se and not os.path.exists(out), (rc, se)
