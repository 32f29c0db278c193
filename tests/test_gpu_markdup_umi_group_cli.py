"""-m gpu: --umi-edits=1 on the command line.  An unsorted, unflagged input whose records carry UMIs -- an RX:Z tag in BAM and SAM, or a
_UMI suffix of the read name -- gives, file for file, the reports of --sort on a copy whose 0x400 flags the Python restatement of the
contract (tests/markdup_umi_group_ref.py) wrote; -v prints the reference's figures; without --umi-edits the run is the exact-match one."""
import dataclasses
import os
import subprocess

import numpy as np
import pytest

from rnaseqc_amd import abi, bamio, synth
from tests import markdup_ref as ref
from tests import markdup_umi_group_cases as gc
from tests import markdup_umi_group_ref as gref
from tests import markdup_umi_ref as uref
from tests.test_cli import cli  # noqa: F401

pytestmark = pytest.mark.gpu
CONTIGS = [("chrA", 900_000, 70), ("chrB", 500_000, 40), ("chrC", 300_000, 15)]
EXTRA = ["--coverage"]
TRACKS = ["--coverage", "--junctions", "--bedgraph", "--gene-body"]


def _run(cli, args, env=None, timeout=300):
    p = subprocess.run([cli, *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, **(env or {})), timeout=timeout)
    return p.returncode, p.stdout.decode(), p.stderr.decode()


def _reports(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d))}


class Case:
    pass


@pytest.fixture(scope="module")
def files(tmp_path_factory, cli):
    d = tmp_path_factory.mktemp("umigroupfiles")
    f = Case()
    f.dir = d
    f.ann = synth.make_annotation(seed=51, contigs=CONTIGS)
    b = gc.fixture()
    # what an aligner emits: no record carries 0x400
    f.reads = bamio.sam_consistent(dataclasses.replace(b, flag=(np.asarray(b.flag, np.uint16) & np.uint16(~abi.FDUP & 0xFFFF)).astype(np.uint16)))
    f.text = gc.fixture_umi_text()
    f.names = [bytes(b.qname[int(b.qname_off[i]):int(b.qname_off[i + 1])]) for i in range(b.n)]
    f.verdict, f.info, f.umi_info, f.group_info, _ = gref.mark_duplicates_umi_group([f.reads])
    f.exact_verdict, f.exact_info, _, _ = uref.mark_duplicates_umi([f.reads])
    assert f.group_info["merged_nodes"] > 0 and f.exact_info["duplicate_fragments"] < f.info["duplicate_fragments"] < f.umi_info["position_duplicate_fragments"]
    p = f.paths = {k: str(d / v) for k, v in dict(gtf="m.gtf", bam="tagged.bam", sam="tagged.sam", named="named.bam", flagged="flagged.bam", exact_flagged="exact_flagged.bam").items()}
    bamio.write_gtf(p["gtf"], f.ann)
    bam_aux = lambda i: ((b"RXZ" + f.text[i].encode() + b"\x00", b"") if i % 3 == 0 else (b"", b"RXZ" + f.text[i].encode() + b"\x00"))
    sam_aux = lambda i: (("RX:Z:" + f.text[i], "") if i % 3 == 0 else ("", "RX:Z:" + f.text[i]))
    bamio.write_bam(p["bam"], gc.CONTIGS, f.reads, extra_aux=bam_aux)
    bamio.write_sam(p["sam"], gc.CONTIGS, f.reads, extra_aux=sam_aux)
    bamio.write_bam(p["named"], gc.CONTIGS, f.reads, qnames=[n + b"_" + t.encode() for n, t in zip(f.names, f.text)])
    bamio.write_bam(p["flagged"], gc.CONTIGS, ref.rewrite_flags([f.reads], f.verdict)[0])
    bamio.write_bam(p["exact_flagged"], gc.CONTIGS, ref.rewrite_flags([f.reads], f.exact_verdict)[0])
    f.want_out, f.exact_out = str(d / "want"), str(d / "exact")
    rc, _, se = _run(cli, ["--sort", p["gtf"], p["flagged"], f.want_out, "-s", "x", *EXTRA])
    assert rc == 0, se
    rc, _, se = _run(cli, ["--sort", p["gtf"], p["exact_flagged"], f.exact_out, "-s", "x", *EXTRA])
    assert rc == 0, se
    assert _reports(f.want_out)["x.metrics.tsv"] != _reports(f.exact_out)["x.metrics.tsv"]
    return f


def _verbose_lines(f):
    return ("Duplicates marked: records %d, population %d, anchors %d, sets %d, duplicate_fragments %d, flagged_records %d, cleared_records %d, sig_ms" % tuple(f.info[k] for k in ref.INFO_FIELDS),
            "UMIs in the signature: anchors_with_umi %d, anchors_without_umi %d, position_duplicate_fragments %d\n" % tuple(f.umi_info[k] for k in uref.UMI_FIELDS),
            "UMIs grouped: umi_nodes %d, merged_nodes %d, exact_duplicate_fragments %d, group_ms " % tuple(f.group_info[k] for k in gref.GROUP_FIELDS))


def _assert_same_reports(got_dir, want_dir):
    got, want = _reports(got_dir), _reports(want_dir)
    assert sorted(got) == sorted(want) and len(got) >= 5
    for name in want:
        assert got[name] == want[name], name


@pytest.mark.parametrize("kind,env", [("bam", dict(RSQC_DECODE_CHUNK="65536", RSQC_DECODE_MAX_OUT="262144")), ("bam", dict(RSQC_DECODE="host", RSQC_BATCH="700")),
                                      ("sam", dict(RSQC_SAM_CHUNK="50000"))], ids=["bam_device", "bam_host", "sam"])
def test_umi_edits_reports_equal_sort_on_the_flagged_copy(cli, files, kind, env):
    out = str(files.dir / ("edits_" + kind + ("_host" if "RSQC_DECODE" in env else "")))
    rc, so, se = _run(cli, ["--umi-tag=RX", "--umi-edits=1", files.paths["gtf"], files.paths[kind], out, "-s", "x", "-v", *EXTRA], env=env)
    assert rc == 0, se
    _assert_same_reports(out, files.want_out)
    for line in _verbose_lines(files):
        assert line in so, so


def test_umi_qname_with_edits_on_the_named_file(cli, files):
    out = str(files.dir / "qname")
    rc, so, se = _run(cli, ["--umi-qname", "--umi-edits", "1", files.paths["gtf"], files.paths["named"], out, "-s", "x", "-v", *EXTRA])
    assert rc == 0, se
    _assert_same_reports(out, files.want_out)                       # the reports of --umi-tag=RX --umi-edits=1 on the tagged file
    for line in _verbose_lines(files):
        assert line in so, so


def test_with_junctions_bedgraph_and_gene_body(cli, files):
    """The other stages that hang on the collection see the grouped flags: every report of --sort with the three flags on the flagged
    copy, the junction table, the coverage track and the gene-body table included."""
    want, out = str(files.dir / "want_tracks"), str(files.dir / "edits_tracks")
    rc, _, se = _run(cli, ["--sort", files.paths["gtf"], files.paths["flagged"], want, "-s", "x", *TRACKS])
    assert rc == 0, se
    rc, so, se = _run(cli, ["--umi-tag=RX", "--umi-edits=1", files.paths["gtf"], files.paths["bam"], out, "-s", "x", "-v", *TRACKS])
    assert rc == 0, se
    _assert_same_reports(out, want)
    assert len(_reports(out)) > len(_reports(files.want_out)) and _verbose_lines(files)[2] in so


@pytest.mark.parametrize("args", [[], ["--umi-edits=0"]], ids=["absent", "edits_0"])
def test_without_umi_edits_the_run_is_the_exact_one(cli, files, args):
    """--umi-tag=RX alone, and with --umi-edits=0: the reports of --sort on the copy the EXACT reference flagged, and no grouping line."""
    out = str(files.dir / ("exact_run" + "".join(args).strip("-").replace("=", "")))
    rc, so, se = _run(cli, ["--umi-tag=RX", *args, files.paths["gtf"], files.paths["bam"], out, "-s", "x", "-v", *EXTRA])
    assert rc == 0, se
    _assert_same_reports(out, files.exact_out)
    assert "UMIs in the signature: anchors_with_umi" in so and "UMIs grouped" not in so
    assert "duplicate_fragments %d, " % files.exact_info["duplicate_fragments"] in so


@pytest.mark.parametrize("args", [["--umi-tag=RX", "--umi-edits=2"], ["--umi-edits=1"], ["--umi-tag=RX", "--umi-edits=1", "--gpus", "2"]])
def test_refusals_on_real_inputs(cli, files, args):
    """Exit 6 with real inputs as well, and nothing is written."""
    out = str(files.dir / ("refused_" + "_".join(a.strip("-").replace("=", "") for a in args)))
    rc, so, se = _run(cli, [*args, files.paths["gtf"], files.paths["bam"], out, "-s", "x"])
    assert rc == 6 and not os.path.exists(out), (rc, se)
