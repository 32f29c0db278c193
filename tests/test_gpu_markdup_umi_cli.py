"""-m gpu: --umi-tag / --umi-qname on the command line.  An unsorted, unflagged input whose records carry UMIs -- an RX:Z tag in BAM,
plain SAM and BGZF SAM, or a _UMI / :UMI suffix of the read name -- gives, file for file, the reports of --sort on a copy whose 0x400
flags the Python restatement of the contract (tests/markdup_umi_ref.py) wrote, under the device decode and RSQC_DECODE=host; the
device-decoded umi column equals the Python pack; --mark-duplicates alone is what it was."""
import dataclasses
import os
import subprocess

import numpy as np
import pytest

from rnaseqc_amd import abi, bamio, engine, synth
from tests import markdup_ref as ref
from tests import markdup_umi_cases as uc
from tests import markdup_umi_ref as uref
from tests.test_cli import cli  # noqa: F401

pytestmark = pytest.mark.gpu
CONTIGS = [("chrA", 900_000, 70), ("chrB", 500_000, 40), ("chrC", 300_000, 15)]


def _run(cli, args, env=None, timeout=300):
    p = subprocess.run([cli, *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, **(env or {})), timeout=timeout)
    return p.returncode, p.stdout.decode(), p.stderr.decode()


def _reports(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d))}


class Case:
    pass


@pytest.fixture(scope="module")
def files(tmp_path_factory, cli):
    d = tmp_path_factory.mktemp("umifiles")
    f = Case()
    f.dir = d
    f.ann = synth.make_annotation(seed=51, contigs=CONTIGS)
    b = uc.fixture()
    # what an aligner emits: no record carries 0x400
    f.reads = bamio.sam_consistent(dataclasses.replace(b, flag=(np.asarray(b.flag, np.uint16) & np.uint16(~abi.FDUP & 0xFFFF)).astype(np.uint16)))
    f.text = uc.fixture_umi_text()
    f.names = [bytes(b.qname[int(b.qname_off[i]):int(b.qname_off[i + 1])]) for i in range(b.n)]
    f.verdict, f.info, f.umi_info, _ = uref.mark_duplicates_umi([f.reads])
    f.position_verdict, f.position_info, _ = ref.mark_duplicates([f.reads])
    assert 0 < f.info["duplicate_fragments"] < f.position_info["duplicate_fragments"] == f.umi_info["position_duplicate_fragments"]
    p = f.paths = {k: str(d / v) for k, v in dict(gtf="m.gtf", bam="tagged.bam", sam="tagged.sam", samgz="tagged.sam.gz", named="named.bam", colon="colon.bam",
                                                  flagged="flagged.bam", position_flagged="position_flagged.bam").items()}
    bamio.write_gtf(p["gtf"], f.ann)
    # the tag in front of the standard aux fields on every third record, behind them on the others
    bam_aux = lambda i: ((b"RXZ" + f.text[i].encode() + b"\x00", b"") if i % 3 == 0 else (b"", b"RXZ" + f.text[i].encode() + b"\x00"))
    sam_aux = lambda i: (("RX:Z:" + f.text[i], "") if i % 3 == 0 else ("", "RX:Z:" + f.text[i]))
    bamio.write_bam(p["bam"], uc.CONTIGS, f.reads, extra_aux=bam_aux)
    bamio.write_sam(p["sam"], uc.CONTIGS, f.reads, extra_aux=sam_aux)
    bamio.write_sam(p["samgz"], uc.CONTIGS, f.reads, extra_aux=sam_aux, bgzf=True)
    bamio.write_bam(p["named"], uc.CONTIGS, f.reads, qnames=[n + b"_" + t.encode() for n, t in zip(f.names, f.text)])
    bamio.write_bam(p["colon"], uc.CONTIGS, f.reads, qnames=[b"M0:7:" + n + b":" + t.encode() for n, t in zip(f.names, f.text)])
    bamio.write_bam(p["flagged"], uc.CONTIGS, ref.rewrite_flags([f.reads], f.verdict)[0])
    bamio.write_bam(p["position_flagged"], uc.CONTIGS, ref.rewrite_flags([f.reads], f.position_verdict)[0])
    f.want_out, f.position_out = str(d / "want"), str(d / "position")
    rc, _, se = _run(cli, ["--sort", p["gtf"], p["flagged"], f.want_out, "-s", "x", "--coverage"])
    assert rc == 0, se
    rc, _, se = _run(cli, ["--sort", p["gtf"], p["position_flagged"], f.position_out, "-s", "x", "--coverage"])
    assert rc == 0, se
    assert _reports(f.want_out)["x.metrics.tsv"] != _reports(f.position_out)["x.metrics.tsv"]
    return f


def _verbose_lines(f):
    return ("Duplicates marked: records %d, population %d, anchors %d, sets %d, duplicate_fragments %d, flagged_records %d, cleared_records %d, sig_ms" % tuple(f.info[k] for k in ref.INFO_FIELDS),
            "UMIs in the signature: anchors_with_umi %d, anchors_without_umi %d, position_duplicate_fragments %d\n" % tuple(f.umi_info[k] for k in uref.UMI_FIELDS))


def _assert_same_reports(got_dir, want_dir):
    got, want = _reports(got_dir), _reports(want_dir)
    assert sorted(got) == sorted(want) and len(got) >= 5
    for name in want:
        assert got[name] == want[name], name


@pytest.mark.parametrize("kind,env", [("bam", dict(RSQC_DECODE_CHUNK="65536", RSQC_DECODE_MAX_OUT="262144")), ("bam", dict(RSQC_DECODE="host", RSQC_BATCH="700")),
                                      ("sam", dict(RSQC_SAM_CHUNK="50000")), ("samgz", {})], ids=["bam_device", "bam_host", "sam", "sam_bgzf"])
def test_umi_tag_reports_equal_sort_on_the_flagged_copy(cli, files, kind, env):
    out = str(files.dir / ("tag_" + kind + ("_host" if "RSQC_DECODE" in env else "")))
    rc, so, se = _run(cli, ["--umi-tag=RX", files.paths["gtf"], files.paths[kind], out, "-s", "x", "-v", "--coverage"], env=env)
    assert rc == 0, se
    _assert_same_reports(out, files.want_out)
    for line in _verbose_lines(files):
        assert line in so, so


@pytest.mark.parametrize("env", [{}, dict(RSQC_DECODE="host")], ids=["device", "host"])
def test_umi_qname_on_the_named_file(cli, files, env):
    out = str(files.dir / ("qname" + ("_host" if env else "")))
    rc, so, se = _run(cli, ["--umi-qname", files.paths["gtf"], files.paths["named"], out, "-s", "x", "-v", "--coverage"], env=env)
    assert rc == 0, se
    _assert_same_reports(out, files.want_out)                       # the reports of --umi-tag=RX on the tagged file
    for line in _verbose_lines(files):
        assert line in so, so


def test_umi_qname_colon(cli, files):
    out = str(files.dir / "colon")
    rc, so, se = _run(cli, ["--umi-qname=:", files.paths["gtf"], files.paths["colon"], out, "-s", "x", "-v", "--coverage"])
    assert rc == 0, se
    _assert_same_reports(out, files.want_out)
    # ... and with the default separator the names of that file carry no UMI: every anchor has key 0, the marking is position-only
    out = str(files.dir / "colon_default")
    rc, so, se = _run(cli, ["--umi-qname", files.paths["gtf"], files.paths["colon"], out, "-s", "x", "-v", "--coverage"])
    assert rc == 0, se
    _assert_same_reports(out, files.position_out)
    assert "anchors_with_umi 0, anchors_without_umi %d, position_duplicate_fragments %d\n" % (files.info["anchors"], files.position_info["duplicate_fragments"]) in so


def test_mark_duplicates_alone_is_what_it_was(cli, files):
    """--mark-duplicates without the new flags on the tagged file: the position-only reports (what tests/test_gpu_markdup_cli.py pins
    for its fixture: --sort on the copy the position-only reference flagged), and no UMI line."""
    out = str(files.dir / "plain_marked")
    rc, so, se = _run(cli, ["--mark-duplicates", files.paths["gtf"], files.paths["bam"], out, "-s", "x", "-v", "--coverage"])
    assert rc == 0, se
    _assert_same_reports(out, files.position_out)
    assert "Duplicates marked: records %d," % files.info["records"] in so and "UMIs in the signature" not in so


def test_device_decoded_umi_column(files):
    """One non-pipelined stream over the tagged BAM in calls of one BGZF block each (records straddle the calls): the window's umi column,
    read back through rsqc_decode_window.device_batch.umi, is the Python pack of every record's tag; the pass it feeds is marked right."""
    want = np.array([uref.umi_pack(t) for t in files.text], np.uint64)
    for kwargs, path in ((dict(umi_tag="RX"), files.paths["bam"]), (dict(umi_qname="_"), files.paths["named"])):
        e = engine.Engine(abi.default_params())
        try:
            e.set_annotation(files.ann)
            e.sort_begin(); e.markdup_begin(); e.markdup_use_umi()
            e.decode_begin(len(uc.CONTIGS), **kwargs)
            got, calls, carried = [], 0, 0
            for comp, tab, skip, limit, _last in bamio.feed_chunks(path, chunk_bytes=1 << 12, max_out=1 << 16):
                n, _runs = e.decode_submit(comp, tab, skip, limit)
                calls += 1
                if n:
                    assert e.last_decoded().umi and e.last_decoded().n == n
                    got.append(e.last_window_umi())
            info = e.decode_end()
            assert info[0] == len(want) and calls > 5                 # several calls: 60 000-byte blocks of ~200-byte records never end on a record
            np.testing.assert_array_equal(np.concatenate(got), want)
            e.sort_end()
            ref.assert_info_equal(e.markdup_end(), files.info)
            uref.assert_umi_info_equal(e.markdup_umi_end(), files.umi_info)
            np.testing.assert_array_equal(e.markdup_verdicts(0, len(want)), files.verdict)
        finally:
            e.close()
    # without a source the window has no column
    e = engine.Engine(abi.default_params())
    try:
        e.set_annotation(files.ann)
        e.decode_begin(len(uc.CONTIGS))
        for comp, tab, skip, limit, _last in bamio.feed_chunks(files.paths["bam"], chunk_bytes=1 << 20):
            n, _runs = e.decode_submit(comp, tab, skip, limit)
            assert not e.last_decoded().umi
        e.decode_end()
    finally:
        e.close()


@pytest.mark.parametrize("args", [["--umi-tag=RX", "--umi-qname"], ["--umi-tag=R"], ["--umi-qname=__"], ["--umi-tag=RX", "--gpus=2"]])
def test_refusals_on_real_inputs(cli, files, args):
    """Exit 6 with real inputs as well, and nothing is written."""
    out = str(files.dir / ("refused_" + "_".join(a.strip("-").replace("=", "") for a in args)))
    rc, so, se = _run(cli, [*args, files.paths["gtf"], files.paths["bam"], out, "-s", "x"])
    assert rc == 6 and not os.path.exists(out), (rc, se)
