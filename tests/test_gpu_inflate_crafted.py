"""-m gpu: the device-side BGZF inflate on blocks no zlib writes.  One BAM's record bytes (and the same records as SAM text) are cut
into BGZF blocks of mixed sizes -- one of ISIZE 65536, one of a single byte, an empty block in the middle of the file -- and every
block is encoded by another policy of the hand-built catalogue (tests/hostemu/inflate_cases.py: far-only matches, distances pinned
at the edge of the LDS ring's reach, 15-bit codes, one-bit codes over a run, many tiny blocks, stored and dynamic mixed, all-literal,
fixed).  The reference is gzip.decompress on the CPU; on the device every block's CRC-32 is checked against the trailer, so a wrong
byte anywhere is a decode error, and the decoded columns, the results and the report files are compared as in tests/test_gpu_decode.py.
Only valid streams go to the GPU."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from rnaseqc_amd import abi, bamio, engine, synth
from tests.compare import assert_results_match
from tests.hostemu import inflate_cases as ic
from tests.hostemu.decode import feed_chunks
from tests.test_cli import cli  # noqa: F401
from tests.test_gpu_decode import check_columns, decode_file
from tests.test_gpu_sam import _collect, _same_reports

pytestmark = pytest.mark.gpu

CONTIGS = [("chrA", 3_000_000), ("chrB", 1_000_000), ("chrC", 500_000)]


@pytest.fixture(scope="module")
def crafted(tmp_path_factory):
    d = tmp_path_factory.mktemp("crafted")
    ann = synth.make_annotation(seed=35, contigs=[("chrA", 3_000_000, 120), ("chrB", 1_000_000, 40), ("chrC", 500_000, 10)])
    batch = bamio.sam_consistent(synth.make_reads(ann, 10_000, seed=36, keep_qnames=True, chimeric_tag_frac=0.02, filter_tag_frac=0.03,
                                                  contig_lengths=np.array([3_000_000, 1_000_000, 500_000])))
    assert 19_000 <= batch.n <= 21_000
    P = dict(dir=d, ann=ann, batch=batch, plain=str(d / "plain.bam"), bam=str(d / "crafted.bam"), sam=str(d / "crafted.sam.gz"), gtf=str(d / "s.gtf"))
    bamio.write_gtf(P["gtf"], ann)
    bamio.write_bam(P["plain"], CONTIGS, batch)                            # zlib level 1: the baseline of the report files
    raw = gzip.decompress(open(P["plain"], "rb").read())
    data, log = ic.crafted_bgzf_file(raw)
    assert gzip.decompress(data) == raw                                    # the reference: concatenated members give concatenated bytes
    sizes = [n for _s, n in log]
    assert 65536 in sizes and 1 in sizes and 0 in sizes[1:-1] and 100 <= len(log) <= 600
    assert {s for s, _n in log} >= set(ic.BLOCK_STYLES) | {"one_bit_run", "empty"}
    open(P["bam"], "wb").write(data)
    plain_sam = str(d / "plain.sam")
    bamio.write_sam(plain_sam, CONTIGS, batch)
    text = open(plain_sam, "rb").read()
    data, log = ic.crafted_bgzf_file(text)
    assert gzip.decompress(data) == text and 65536 in [n for _s, n in log]
    open(P["sam"], "wb").write(data)
    return P


@pytest.mark.parametrize("chunk_bytes,max_out", [(48 << 20, 768 << 20), (1 << 17, 400_000)])
def test_crafted_bam_columns_and_results(crafted, chunk_bytes, max_out):
    batch, ann = crafted["batch"], crafted["ann"]
    p = abi.default_params(); p.n_filter_tags = 1
    e = engine.Engine(p)
    e.set_annotation(ann)
    parts, runs, total, info, n_calls = decode_file(e, crafted["bam"], 3, "ch", ("XF",), chunk_bytes, max_out)
    assert total == batch.n and info[0] == batch.n and not info[1] and info[2] == 0
    if chunk_bytes < (1 << 20):
        assert n_calls > 3
    check_columns(parts, batch)
    got = e.finalize()
    e.close()
    assert_results_match(got, engine.run_engine(p, ann, [batch]))


def test_crafted_bgzf_sam_columns_and_results(crafted):
    """The same records as BGZF-compressed SAM: crafted blocks in front of the SAM stages."""
    batch, ann = crafted["batch"], crafted["ann"]
    p = abi.default_params(); p.n_filter_tags = 1
    e = engine.Engine(p)
    e.set_annotation(ann)
    e.decode_begin(3, "ch", ("XF",), ref_names=[c[0] for c in CONTIGS])
    parts, total = [], 0
    for comp, tab, skip, limit, _last in feed_chunks(crafted["sam"], 0, 0, chunk_bytes=1 << 18, max_out=1 << 40):
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


def test_cli_on_crafted_bam_in_both_kernel_forms_and_host_decode(cli, crafted):
    """RSQC_INFLATE_ONE_PASS=0 / =1 force the two forms of the inflate kernel (the variable is read once per process: one child
    each), RSQC_DECODE=host is htslib's path of the CLI: every report file byte-equal to the run on the zlib level-1 file."""
    d = crafted["dir"]

    def run(name, path, env):
        out = str(d / name)
        r = subprocess.run([cli, crafted["gtf"], path, out, "-s", "x", "-t", "XF", "--chimeric-tag", "ch", "--coverage"], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           env=dict(os.environ, **env), timeout=120)
        assert r.returncode == 0, (name, r.stderr.decode()[-2000:])
        return out

    base = run("plain", crafted["plain"], dict(RSQC_DECODE="device"))
    for name, env in (("one_pass_0", dict(RSQC_DECODE="device", RSQC_INFLATE_ONE_PASS="0")), ("one_pass_1", dict(RSQC_DECODE="device", RSQC_INFLATE_ONE_PASS="1")),
                      ("host", dict(RSQC_DECODE="host"))):
        _same_reports(base, run(name, crafted["bam"], env))
