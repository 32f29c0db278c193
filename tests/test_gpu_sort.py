"""-m gpu: --sort (rsqc_sort_begin / rsqc_sort_end, rnaseqc_amd/csrc/rsqc_sort.hip).  A pass over unsorted records with the sort on
must give the results of an ordinary pass over the same records put in order beforehand: compared with the oracle on the stably
sorted records and with an ordinary GPU pass over them -- through the C ABI (host-fed batches, the BAM and the SAM decode) and
through the command line."""
import os
import subprocess
import threading

import numpy as np
import pytest

from rnaseqc_amd import abi, bamio, engine, synth
from rnaseqc_amd.model import Batch
from tests.compare import assert_results_match
from tests.hostemu.decode import feed_chunks
from tests.test_cli import cli  # noqa: F401

pytestmark = pytest.mark.gpu

CONTIGS = [("chrA", 900_000, 70), ("chrB", 500_000, 40), ("chrC", 300_000, 15)]
LENGTHS = np.array([c[1] for c in CONTIGS])
CS = [(c[0], c[1]) for c in CONTIGS]


class Case:
    pass


@pytest.fixture(scope="module")
def case(oracle_lib):
    """~60 k records of two read lengths (Read Length depends on the order), spliced reads, mates, duplicates; the references are
    computed once: the oracle and an ordinary GPU pass over the sorted records, with and without a BED whose fragment-sample
    cut-off lies below the number of candidates (the file index decides which are kept)."""
    c = Case()
    c.ann = synth.make_annotation(seed=51, contigs=CONTIGS)
    a = synth.make_reads(c.ann, 20000, seed=52, read_len=150, dup_frac=0.08, keep_qnames=True, contig_lengths=LENGTHS)
    b = synth.make_reads(c.ann, 10000, seed=53, read_len=100, dup_frac=0.08, keep_qnames=True, contig_lengths=LENGTHS, fid_base=1_000_000)
    c.sorted = Batch.concat([a, b]).coordinate_sorted()
    n = c.sorted.n
    c.shuffled = c.sorted.take(np.random.default_rng(54).permutation(n))
    c.collated = c.sorted.take(np.argsort(c.sorted.qhash, kind="stable"))          # mates next to each other, names in hash order
    c.bed = synth.make_bed(c.ann, min_len=250)
    c.p = abi.default_params()
    c.p_bed = abi.default_params(fragment_samples=150)
    c.want, c.gpu, c.ordered = {}, {}, {}
    for name, u in (("shuffled", c.shuffled), ("collated", c.collated)):
        s = u.coordinate_sorted()                                                # the stable sort of what arrives
        c.ordered[name] = s
        for bed in (False, True):
            p, kw = (c.p_bed, dict(bed=c.bed)) if bed else (c.p, {})
            c.want[name, bed] = oracle_lib.run_oracle(p, c.ann, [s], **kw)
            c.gpu[name, bed] = engine.run_engine(p, c.ann, [s], **kw)
    w = c.want["shuffled", True]
    assert w.fragment_samples_remaining == 0 and int(w.fragment_count.sum()) == 150       # the cut-off is in force
    return c


def _unequal_cuts(n, seed, parts):
    cuts = np.sort(np.random.default_rng(seed).choice(np.arange(1, n), parts - 1, replace=False))
    return [0] + [int(x) for x in cuts] + [n]


def _sorted_pass(p, ann, u, bed=None, parts=5, seed=1):
    e = engine.Engine(p)
    try:
        e.set_annotation(ann)
        if bed is not None:
            e.set_bed(bed)
        e.sort_begin()
        cuts = _unequal_cuts(u.n, seed, parts)
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            e.submit(u.slice(lo, hi))
        info = e.sort_end()
        return e.finalize(), info
    finally:
        e.close()


@pytest.mark.parametrize("bed", [False, True])
@pytest.mark.parametrize("order", ["shuffled", "collated"])
def test_core_parity(case, order, bed):
    u = getattr(case, order)
    got, info = _sorted_pass(case.p_bed if bed else case.p, case.ann, u, bed=case.bed if bed else None)
    assert info["records"] == u.n and info["batches_in"] == 5 and info["batches_out"] == 1 and info["was_sorted"] == 0
    assert 0 < info["moved"] <= u.n
    assert_results_match(got, case.want[order, bed])
    assert_results_match(got, case.gpu[order, bed])


def test_fixture_is_order_dependent(case, oracle_lib):
    """The fixture's point: the same records counted in arrival order give other order-dependent outputs (the fragment sample
    kept below the cut-off, Read Length, the gene counts of the static index) than in sorted order -- the parity above is not vacuous."""
    arrival = oracle_lib.run_oracle(case.p_bed, case.ann, [case.shuffled], bed=case.bed)
    want = case.want["shuffled", True]
    assert (arrival.read_length != want.read_length or not np.array_equal(arrival.fragment_size, want.fragment_size)
            or not np.array_equal(arrival.fragment_count, want.fragment_count) or not np.array_equal(arrival.gene_reads, want.gene_reads))


@pytest.mark.parametrize("bed", [False, True])
def test_output_batch_boundaries(case, bed, monkeypatch):
    """RSQC_SORT_BATCH small: seven output batches -- the pool rebase, the segment tables and the file indices at batch boundaries."""
    monkeypatch.setenv("RSQC_SORT_BATCH", str(case.shuffled.n // 7 + 1))
    got, info = _sorted_pass(case.p_bed if bed else case.p, case.ann, case.shuffled, bed=case.bed if bed else None, parts=3, seed=2)
    assert info["batches_out"] == 7
    assert_results_match(got, case.want["shuffled", bed])
    assert_results_match(got, case.gpu["shuffled", bed])


def _odd_records(ann):
    """A record of 300 CIGAR operations, one with NM 300, one without operations, unplaced records and an unrecognised RefID."""
    M, D = abi.CIG_M, abi.CIG_D
    row = int(np.flatnonzero(ann.exon_row_contig == 0)[0])
    start = int(ann.exon_row_start[row]) - 1
    recs = [dict(tid=0, pos=start, mpos=start + 200, isize=400, flag=abi.FPAIRED | abi.FPROPER | abi.FREAD1, cigar=[(M, 1), (D, 1)] * 150, nm=2, qname="odd:long"),
            dict(tid=0, pos=start + 5, mpos=start + 300, isize=400, flag=abi.FPAIRED | abi.FPROPER | abi.FREAD1, cigar=[(M, 76)], nm=300, qname="odd:nm"),
            dict(tid=1, pos=1000, mpos=1000, flag=0, cigar=[], l_qseq=76, qname="odd:noops"),
            dict(tid=len(CONTIGS) + 2, pos=77, mpos=77, flag=0, cigar=[(M, 76)], qname="odd:refid"),
            dict(tid=-1, pos=-1, mpos=-1, flag=abi.FPAIRED | abi.FUNMAP | abi.FMUNMAP | abi.FREAD1, mapq=0, cigar=[], l_qseq=76, qname="odd:un"),
            dict(tid=-1, pos=-1, mpos=-1, flag=abi.FPAIRED | abi.FUNMAP | abi.FMUNMAP | abi.FREAD2, mapq=0, cigar=[], l_qseq=76, qname="odd:un")]
    return Batch.from_records(recs)


@pytest.mark.parametrize("sort_batch", [None, 1500])
def test_wide_records_and_odd_tids(oracle_lib, sort_batch, monkeypatch):
    ann = synth.make_annotation(seed=51, contigs=CONTIGS)
    base = synth.make_reads(ann, 4000, seed=61, dup_frac=0.05, keep_qnames=True, contig_lengths=LENGTHS)
    odd = _odd_records(ann)
    assert len(odd.wide_index) == 2
    # the odd records three times over (other arrival places, several wide entries per output batch)
    allr = Batch.concat([base.slice(0, 3000), odd, base.slice(3000, 6000), odd, base.slice(6000, base.n), odd])
    u = allr.take(np.random.default_rng(62).permutation(allr.n))
    s = u.coordinate_sorted()
    assert len(s.wide_index) == 6
    if sort_batch:
        monkeypatch.setenv("RSQC_SORT_BATCH", str(sort_batch))
    p = abi.default_params()
    got, info = _sorted_pass(p, ann, u, parts=4, seed=3)
    assert info["batches_out"] == ((u.n + sort_batch - 1) // sort_batch if sort_batch else 1)
    assert_results_match(got, oracle_lib.run_oracle(p, ann, [s]))
    assert_results_match(got, engine.run_engine(p, ann, [s]))


def test_already_sorted_input(case):
    got, info = _sorted_pass(case.p_bed, case.ann, case.sorted, bed=case.bed, parts=4, seed=4)
    assert info["was_sorted"] == 1 and info["moved"] == 0 and info["records"] == case.sorted.n
    assert_results_match(got, engine.run_engine(case.p_bed, case.ann, [case.sorted], bed=case.bed))


def test_call_order_and_errors(case):
    e = engine.Engine(case.p)
    try:
        e.set_annotation(case.ann)
        with pytest.raises(engine.EngineError) as err:                     # no collection open
            e.sort_end()
        assert err.value.code == abi.ERR_ARG
        e.submit(case.sorted.slice(0, 1000))
        with pytest.raises(engine.EngineError) as err:                     # behind a submit of the same pass
            e.sort_begin()
        assert err.value.code == abi.ERR_ARG and "first submit" in str(err.value)
        e.reset()
        e.sort_begin()
        ranges = Batch.concat_ranges([case.sorted.slice(0, 500)])
        assert ranges.seg_file_index is not None
        with pytest.raises(engine.EngineError) as err:                     # file ranges cannot be collected
            e.submit(ranges)
        assert err.value.code == abi.ERR_ARG and "seg_file_index" in str(err.value)
        import copy
        no_h2 = copy.copy(case.shuffled.slice(0, 800)); no_h2.qhash2 = None
        e.submit(case.shuffled.slice(800, 1600))
        with pytest.raises(engine.EngineError) as err:                     # qhash2: all batches of a pass or none, as ever
            e.submit(no_h2)
        assert err.value.code == abi.ERR_ARG and "qhash2" in str(err.value)
    finally:
        e.close()


def test_finalize_is_refused_while_a_collection_is_open(case):
    """rsqc_finalize between rsqc_sort_begin and rsqc_sort_end would report a pass without records: it is RSQC_ERR_ARG, the
    collection stays, and rsqc_sort_end + rsqc_finalize behind it give the pass's results."""
    e = engine.Engine(case.p)
    try:
        e.set_annotation(case.ann)
        e.sort_begin()
        e.submit(case.shuffled)
        with pytest.raises(engine.EngineError) as err:
            e.finalize()
        assert err.value.code == abi.ERR_ARG and "rsqc_sort_end" in str(err.value)
        assert e.sort_end()["records"] == case.shuffled.n
        assert_results_match(e.finalize(), case.gpu["shuffled", False])
    finally:
        e.close()


def test_reset_in_the_middle_of_a_collection(case):
    """rsqc_reset leaves the collecting mode and frees the collection; the ordinary pass behind it gives its own results, and so
    does a sorted pass behind that one (tests/test_gpu_reuse.py's pattern)."""
    e = engine.Engine(case.p)
    try:
        e.set_annotation(case.ann)
        e.sort_begin()
        e.submit(case.shuffled.slice(0, 20000))
        e.submit(case.shuffled.slice(20000, 33333))
        e.reset()
        step = case.sorted.n // 3 + 1
        for lo in range(0, case.sorted.n, step):
            e.submit(case.sorted.slice(lo, min(case.sorted.n, lo + step)))
        assert_results_match(e.finalize(), case.gpu["shuffled", False])
        e.reset()
        e.sort_begin()
        e.submit(case.shuffled)
        info = e.sort_end()
        assert info["records"] == case.shuffled.n
        assert_results_match(e.finalize(), case.gpu["shuffled", False])
    finally:
        e.close()


# ---- the decode paths: a shuffled BAM and a shuffled SAM, many small calls (the copy-out of the reused window buffers) ----------
@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("sortfiles")
    f = Case()
    f.dir = d
    f.ann = synth.make_annotation(seed=71, contigs=CONTIGS)
    srt = bamio.sam_consistent(synth.make_reads(f.ann, 15000, seed=72, keep_qnames=True, dup_frac=0.1, chimeric_tag_frac=0.03, filter_tag_frac=0.03, contig_lengths=LENGTHS))
    f.shuffled = srt.take(np.random.default_rng(73).permutation(srt.n))
    f.sorted = f.shuffled.coordinate_sorted()
    f.paths = dict(gtf=str(d / "s.gtf"), bed=str(d / "s.bed"), sorted_bam=str(d / "sorted.bam"), bam=str(d / "shuf.bam"), sam=str(d / "shuf.sam"))
    bamio.write_gtf(f.paths["gtf"], f.ann)
    bamio.write_bed(f.paths["bed"], f.ann, synth.make_bed(f.ann, min_len=250))
    bamio.write_bam(f.paths["sorted_bam"], CS, f.sorted)
    bamio.write_bam(f.paths["bam"], CS, f.shuffled)
    bamio.write_sam(f.paths["sam"], CS, f.shuffled)
    f.p = abi.default_params(); f.p.n_filter_tags = 1
    f.want = engine.run_engine(f.p, f.ann, [f.sorted])
    return f


@pytest.mark.parametrize("pipelined", [False, True])
def test_decode_bam_collects_out_of_reused_windows(files, pipelined):
    e = engine.Engine(files.p)
    try:
        e.set_annotation(files.ann)
        e.sort_begin()
        e.decode_begin(3, "ch", ("XF",), pipelined=pipelined)
        calls = total = 0
        # (from the first record's virtual offset, the default: the header is not record data)
        for comp, tab, skip, limit, _last in feed_chunks(files.paths["bam"], chunk_bytes=1 << 16, max_out=1 << 18):
            total += e.decode_submit(comp, tab, skip, limit)[0]
            calls += 1
        records, unsorted, _, _ = e.decode_end()
        total += e.decode_last[0] if pipelined else 0
        assert calls >= 8 and total == records == files.shuffled.n
        assert unsorted                                                    # still reported; rsqc_sort_end settles it
        info = e.sort_end()
        assert info["records"] == records and info["batches_in"] >= 8 and info["was_sorted"] == 0
        assert_results_match(e.finalize(), files.want)
    finally:
        e.close()


def test_decode_sam_text_collects_out_of_reused_windows(files):
    text = open(files.paths["sam"], "rb").read()
    e = engine.Engine(files.p)
    try:
        e.set_annotation(files.ann)
        e.sort_begin()
        e.decode_begin(3, "ch", ("XF",), pipelined=True, ref_names=[c[0] for c in CONTIGS])
        step = len(text) // 23 + 1
        total = sum(e.decode_submit_text(text[a:a + step])[0] for a in range(0, len(text), step))
        records, _unsorted, _, _ = e.decode_end()
        assert total + e.decode_last[0] == records == files.shuffled.n
        info = e.sort_end()
        assert info["batches_in"] >= 20
        assert_results_match(e.finalize(), files.want)
    finally:
        e.close()


# ---- the command line ------------------------------------------------------------------------------------------------------------
def _run(cli, args, env=None, timeout=300):
    p = subprocess.run([cli, *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, **(env or {})), timeout=timeout)
    return p.returncode, p.stdout.decode(), p.stderr.decode()


def _same_reports(a, b):                                     # (the comparison of tests/test_gpu_sam.py)
    fa, fb = sorted(os.listdir(a)), sorted(os.listdir(b))
    assert fa == fb and fa
    for f in fa:
        assert open(os.path.join(a, f), "rb").read() == open(os.path.join(b, f), "rb").read(), f


@pytest.mark.parametrize("mode", ["plain", "bed"])
def test_cli_sort_reports_equal_sorted_file_reports(cli, files, mode):
    d, P = files.dir, files.paths
    extra = ["--bed", P["bed"], "--fragment-samples", "100"] if mode == "bed" else []
    common = ["-s", "x", "-v", "--coverage"] + extra
    small = dict(RSQC_DECODE_CHUNK="65536", RSQC_DECODE_MAX_OUT="262144", RSQC_SAM_CHUNK="100000", RSQC_SORT_BATCH="7000")
    ref_out = str(d / (mode + "_sorted"))
    rc, _, se = _run(cli, [P["gtf"], P["sorted_bam"], ref_out] + common)
    assert rc == 0 and "sorted" not in se, se
    rc, _, se = _run(cli, [P["gtf"], P["bam"], str(d / (mode + "_plain_shuf"))] + common)
    assert rc == 0 and "does not appear to be sorted" in se                      # without --sort: the reference's warning
    for kind in ("bam", "bam_host", "fifo"):
        out = str(d / ("%s_%s" % (mode, kind)))
        src, t = P["bam"], None
        env = dict(small)
        if kind == "bam_host":
            env["RSQC_DECODE"] = "host"
        if kind == "fifo":
            src = str(d / (mode + ".fifo"))
            os.mkfifo(src)

            def writer():
                with open(src, "wb") as w, open(P["sam"], "rb") as r:
                    w.write(r.read())
            t = threading.Thread(target=writer); t.start()
        rc, so, se = _run(cli, ["--sort", P["gtf"], src, out] + common, env=env)
        if t:
            t.join()
        assert rc == 0, (kind, se)
        assert "does not appear to be sorted" not in se, se
        assert "Sorted on the GPU: records %d," % files.shuffled.n in so and "was_sorted 0" in so, so
        _same_reports(ref_out, out)


def test_cli_sort_refused_combinations(cli, files, tmp_path):
    """Refused before any GPU work (exit 6, like the --bam-list combinations): no output directory is made."""
    P = files.paths
    lst = str(tmp_path / "list.txt")
    open(lst, "w").write(P["bam"] + "\n")
    hidden = dict(HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")              # (a run that touched the GPU would end with exit 10)
    for args, env in ((["--sort", "--gpus", "2", P["gtf"], P["bam"]], {}), (["--sort", P["gtf"], P["bam"]], dict(RSQC_GPUS="2")),
                      (["--sort", P["gtf"], P["bam"]], dict(RSQC_GPU_LIST="0,1")), (["--sort", "--bam-list=" + lst, P["gtf"]], {})):
        out = str(tmp_path / "refused")
        rc, _, se = _run(cli, args + [out], env=dict(hidden, **env))
        assert rc == 6 and "Argument validation error: --sort" in se, (args, rc, se)
        assert not os.path.exists(out)
