"""-m gpu: SAM input (plain text and BGZF-compressed) through the device SAM stages (rnaseqc_amd/csrc/rsqc_sam.hip) -- the
decoded columns against the written records at several call sizes, and the command line on x.sam / x.sam.gz / a FIFO fed
with x.sam against the command line on x.bam of the same alignments: every report file byte-identical."""
import os
import subprocess
import threading

import numpy as np
import pytest

from rnaseqc_amd import abi, bamio, engine, synth
from tests.compare import assert_results_match
from tests.hostemu.decode import feed_chunks
from tests.test_cli import cli  # noqa: F401
from tests.test_gpu_decode import check_columns

pytestmark = pytest.mark.gpu

CONTIGS = [("chrA", 3_000_000), ("chrB", 1_000_000), ("chrC", 500_000)]


def _batch(n_pairs, seed=36, **kw):
    ann = synth.make_annotation(seed=35, contigs=[("chrA", 3_000_000, 120), ("chrB", 1_000_000, 40), ("chrC", 500_000, 10)])
    b = synth.make_reads(ann, n_pairs, seed=seed, keep_qnames=True, chimeric_tag_frac=0.02, filter_tag_frac=0.03, dup_frac=0.05,
                         contig_lengths=np.array([3_000_000, 1_000_000, 500_000]), **kw)
    return ann, bamio.sam_consistent(b)


def _collect(e, n, parts):
    e.wait()
    s = e.last_decoded()
    assert s.n == n
    rd = e.read_device
    parts.append(dict(core=rd(s.core, n, abi.REC_CORE), aux=rd(s.aux, n, abi.REC_AUX), qhash2=rd(s.qhash2, n, np.uint32), cigar=rd(s.cigar, s.n_cigar_total, np.uint32),
                      seg_tid=rd(s.seg_tid, s.n_seg, np.int32), seg_start=rd(s.seg_start, s.n_seg + 1, np.uint64),
                      wide_index=rd(s.wide_index, s.n_wide, np.uint64), wide_nm=rd(s.wide_nm, s.n_wide, np.int32),
                      wide_lq=rd(s.wide_l_qseq, s.n_wide, np.int32), wide_nc=rd(s.wide_n_cigar, s.n_wide, np.uint32), base=s.file_index_base))


@pytest.mark.parametrize("chunk", [None, 1 << 18, 100])
def test_decode_sam_text_columns(tmp_path, chunk):
    """Plain SAM through rsqc_decode_submit_text, non-pipelined: in one call, in calls that lines straddle, in calls shorter
    than one line -- the device_batch columns equal the written records and the results equal the host-fed run's."""
    ann, batch = _batch(6000 if chunk == 100 else 30000)
    path = str(tmp_path / "x.sam")
    bamio.write_sam(path, CONTIGS, batch)
    text = open(path, "rb").read()
    p = abi.default_params(); p.n_filter_tags = 1
    e = engine.Engine(p)
    e.set_annotation(ann)
    e.decode_begin(3, "ch", ("XF",), ref_names=[c[0] for c in CONTIGS])
    parts, total, step = [], 0, chunk or len(text)
    for a in range(0, len(text), step):
        n, _runs = e.decode_submit_text(text[a:a + step])
        total += n
        if n:
            _collect(e, n, parts)
    info = e.decode_end()
    assert total == batch.n == info[0] and not info[1]
    check_columns(parts, batch)
    got = e.finalize()
    e.close()
    assert_results_match(got, engine.run_engine(p, ann, [batch]))


@pytest.mark.parametrize("chunk_bytes", [48 << 20, 1 << 17])
def test_decode_bgzf_sam_columns(tmp_path, chunk_bytes):
    """BGZF-compressed SAM through rsqc_decode_submit (the header's blocks included: the device skips the '@' lines)."""
    ann, batch = _batch(30000)
    path = str(tmp_path / "x.sam.gz")
    bamio.write_sam(path, CONTIGS, batch, bgzf=True)
    p = abi.default_params(); p.n_filter_tags = 1
    e = engine.Engine(p)
    e.set_annotation(ann)
    e.decode_begin(3, "ch", ("XF",), ref_names=[c[0] for c in CONTIGS])
    parts, total = [], 0
    for comp, tab, skip, limit, _last in feed_chunks(path, 0, 0, chunk_bytes=chunk_bytes, max_out=1 << 40):
        n, _ = e.decode_submit(comp, tab, skip, limit)
        total += n
        if n:
            _collect(e, n, parts)
    info = e.decode_end()
    assert total == batch.n == info[0]
    check_columns(parts, batch)
    got = e.finalize()
    e.close()
    assert_results_match(got, engine.run_engine(p, ann, [batch]))


def _run(cli, args, env=None, timeout=300):
    p = subprocess.run([cli, *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, **(env or {})), timeout=timeout)
    return p.returncode, p.stdout.decode(), p.stderr.decode()


def _same_reports(a, b):
    fa, fb = sorted(os.listdir(a)), sorted(os.listdir(b))
    assert fa == fb and fa
    for f in fa:
        assert open(os.path.join(a, f), "rb").read() == open(os.path.join(b, f), "rb").read(), f


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("samcli")
    contigs = [("chrA", 900_000, 70), ("chrB", 500_000, 40)]
    ann = synth.make_annotation(seed=41, contigs=contigs)
    batch = bamio.sam_consistent(synth.make_reads(ann, 20000, seed=42, keep_qnames=True, dup_frac=0.1, chimeric_tag_frac=0.03, filter_tag_frac=0.03,
                                                  contig_lengths=np.array([c[1] for c in contigs])))
    cs = [(c[0], c[1]) for c in contigs]
    paths = dict(gtf=str(d / "s.gtf"), bam=str(d / "s.bam"), sam=str(d / "s.sam"), samgz=str(d / "s.sam.gz"), bed=str(d / "s.bed"), fa=str(d / "ref.fa"))
    bamio.write_gtf(paths["gtf"], ann)
    bamio.write_bam(paths["bam"], cs, batch)
    bamio.write_sam(paths["sam"], cs, batch)
    bamio.write_sam(paths["samgz"], cs, batch, bgzf=True)
    bamio.write_bed(paths["bed"], ann, synth.make_bed(ann, min_len=250))
    bamio.write_fasta(paths["fa"], ["chrA"], synth.make_reference([contigs[0][1]], seed=43), index_path=str(d / "ref.fai"))
    return d, paths


MODES = {"plain": [], "bed": ["--bed", "{bed}"], "legacy": ["--legacy"], "fasta": ["--fasta", "{fa}"], "stranded": ["--stranded=RF", "-u"],
         "tags": ["-t", "XF", "--chimeric-tag", "ch", "--exclude-chimeric"]}


@pytest.mark.parametrize("mode", list(MODES))
def test_cli_sam_reports_equal_bam_reports(cli, inputs, mode):
    d, P = inputs
    extra = [a.format(**P) for a in MODES[mode]]
    env = dict(RSQC_SAM_CHUNK="300000")                       # lines straddle many calls
    outs = {}
    for kind in ("bam", "sam", "samgz", "fifo"):
        out = str(d / ("%s_%s" % (mode, kind)))
        src = P[kind] if kind != "fifo" else str(d / ("%s.fifo" % mode))
        t = None
        if kind == "fifo":
            os.mkfifo(src)
            def writer():
                with open(src, "wb") as w, open(P["sam"], "rb") as r:
                    w.write(r.read())
            t = threading.Thread(target=writer); t.start()
        rc, so, se = _run(cli, [P["gtf"], src, out, "-s", "x", "-vv", "--coverage"] + extra, env=env)
        if t:
            t.join()
        assert rc == 0, (kind, se)
        if kind != "bam":
            assert "SAM" in so, so
        outs[kind] = (out, se)
    for kind in ("sam", "samgz", "fifo"):
        _same_reports(outs["bam"][0], outs[kind][0])


def test_cli_sam_stderr_and_errors(cli, inputs, tmp_path):
    d, P = inputs
    # unsorted input and an unrecognised reference: the same stderr as the BAM run of the same records
    ann, batch = _batch(3000, seed=44)
    idx = np.arange(batch.n)
    idx[100], idx[200] = 200, 100
    b2 = batch.take(idx)
    bam, sam = str(tmp_path / "u.bam"), str(tmp_path / "u.sam")
    bamio.write_bam(bam, CONTIGS, b2)
    bamio.write_sam(sam, CONTIGS, b2)
    gtf = str(tmp_path / "u.gtf")
    bamio.write_gtf(gtf, ann)
    ra = _run(cli, [gtf, bam, str(tmp_path / "ua"), "-s", "x", "-v"])
    rb = _run(cli, [gtf, sam, str(tmp_path / "ub"), "-s", "x", "-v"])
    assert ra[0] == rb[0] == 0
    assert "does not appear to be sorted" in ra[2]
    assert [l for l in ra[2].splitlines() if "sorted" in l or "RefID" in l] == [l for l in rb[2].splitlines() if "sorted" in l or "RefID" in l]
    _same_reports(str(tmp_path / "ua"), str(tmp_path / "ub"))
    # a malformed line: the input-error exit and its line number
    lines = open(P["sam"], "rb").read().split(b"\n")
    n_hdr = sum(1 for l in lines if l.startswith(b"@"))
    k = next(k for k in range(n_hdr + 1000, len(lines)) if b"M\t" in lines[k])
    lines[k] = lines[k].replace(b"M\t", b"Q\t", 1)
    bad = str(tmp_path / "bad.sam")
    open(bad, "wb").write(b"\n".join(lines))
    rc, _, se = _run(cli, [P["gtf"], bad, str(tmp_path / "bad")], env=dict(RSQC_SAM_CHUNK="65536"))
    assert rc == 10 and ("line %d:" % (k + 1)) in se, se
    # plain gzip (not BGZF): exit 10 with the advice
    import gzip
    gz = str(tmp_path / "plain.sam.gz")
    open(gz, "wb").write(gzip.compress(open(P["sam"], "rb").read()))
    rc, _, se = _run(cli, [P["gtf"], gz, str(tmp_path / "gz")])
    assert rc == 10 and "Unable to open" in se and "bgzip" in se
    # --gpus 2 on SAM: the warning, one GPU, the same reports
    rc, _, se = _run(cli, [P["gtf"], P["sam"], str(tmp_path / "g2"), "-s", "x", "--gpus", "2", "--coverage"])
    assert rc == 0 and "running on one GPU" in se
    rc, _, _ = _run(cli, [P["gtf"], P["bam"], str(tmp_path / "g1"), "-s", "x", "--coverage"])
    _same_reports(str(tmp_path / "g1"), str(tmp_path / "g2"))


def test_cli_sam_two_million_records(cli, tmp_path):
    """~2 M records: parity with the BAM run, and the SAM stages' kernels show up in the decode profile."""
    ann, batch = _batch(1_000_000, seed=47)
    gtf, bam, sam = str(tmp_path / "m.gtf"), str(tmp_path / "m.bam"), str(tmp_path / "m.sam")
    bamio.write_gtf(gtf, ann)
    bamio.write_bam_fast(bam, CONTIGS, batch, threads=8)
    bamio.write_sam(sam, CONTIGS, batch)
    ra = _run(cli, [gtf, bam, str(tmp_path / "a"), "-s", "x"])
    rb = _run(cli, [gtf, sam, str(tmp_path / "b"), "-s", "x", "-vv"], env=dict(RSQC_DECODE_PROFILE="1"))
    assert ra[0] == 0 and rb[0] == 0, rb[2]
    assert "frame+parse" in rb[2] and "SAM text on the GPU" in rb[1]
    _same_reports(str(tmp_path / "a"), str(tmp_path / "b"))
