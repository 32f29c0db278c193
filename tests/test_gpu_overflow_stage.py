"""-m gpu: classify_long_kernel with a FULL LDS stage (rsqc_k1.h: k1e_overflow, k1e_stage_flush) on the device, and the partition edges
of the device's fragment count.

RSQC_K1_GRID = 1, 2, 3 (read by rsqc_create) gives the per-record kernel, and with it classify_long_kernel, one to three workgroups of
four waves: on tests/cases.py:full_stage_case each of them hands thousands of records to the general kernel through its 1024-entry
stage, in calls of 1 to 64 lanes from four waves at once.  At the default grid the same input leaves a few entries per workgroup
(the control).  tests/test_k1_overflow_stage.py runs the same code under the host emulation's seeded schedules."""
import numpy as np
import pytest

from rnaseqc_amd import abi, engine, synth
from rnaseqc_amd.model import Annotation, Batch
from tests import cases
from tests.compare import assert_results_match

pytestmark = pytest.mark.gpu

CUT = 5_003           # the two-batch split: not a multiple of 64, and between the mates of a pair


@pytest.fixture(scope="module")
def full_stage(oracle_lib):
    ann, batch = cases.full_stage_case()
    wants = {}

    def want(bed=None, reference=None, **kw):
        key = (tuple(sorted(kw.items())), bed is not None, reference is not None)
        if key not in wants:
            wants[key] = oracle_lib.run_oracle(abi.default_params(**kw), ann, [batch], bed=bed, reference=reference)
        return wants[key]
    return ann, batch, want


def _set_grid(monkeypatch, grid):
    if grid is None:
        monkeypatch.delenv("RSQC_K1_GRID", raising=False)
    else:
        monkeypatch.setenv("RSQC_K1_GRID", str(grid))          # (before the Engine is made: rsqc_create reads it)


@pytest.mark.parametrize("variant", ["default", "stranded_forward", "two_batches"])
@pytest.mark.parametrize("grid", [None, 1, 2, 3])
def test_full_stage_vs_oracle(full_stage, monkeypatch, grid, variant):
    ann, batch, want = full_stage
    kw = dict(stranded=abi.STRAND_FORWARD) if variant == "stranded_forward" else {}
    w = want(**kw)
    assert int(w.gene_reads[0]) + int(w.gene_reads[1]) >= batch.n           # every record reaches the feature stage
    parts = [batch.slice(0, CUT), batch.slice(CUT, batch.n)] if variant == "two_batches" else [batch]
    _set_grid(monkeypatch, grid)
    got = engine.run_engine(abi.default_params(**kw), ann, parts)
    assert_results_match(got, w)
    assert got.counter("Total Alignments") == batch.n


def test_full_stage_with_bed(full_stage, monkeypatch):
    """the --bed instances of the kernels, one workgroup"""
    ann, batch, want = full_stage
    bed = cases.full_stage_bed()
    w = want(bed=bed)
    assert int(w.fragment_count.sum()) > 200
    _set_grid(monkeypatch, 1)
    got = engine.run_engine(abi.default_params(), ann, [batch], bed=bed)
    assert_results_match(got, w)
    assert got.fragment_samples_remaining == w.fragment_samples_remaining


def test_full_stage_with_reference(full_stage, monkeypatch):
    """the --fasta instances of the kernels, one workgroup"""
    ann, batch, want = full_stage
    ref = synth.make_reference([cases.FULL_STAGE_CONTIG_LENGTH], seed=5)
    w = want(reference=ref)
    assert w.have_reference            # (no GC candidates here: every record lies under two exons or more; the kernels' --fasta instances run all the same)
    _set_grid(monkeypatch, 1)
    assert_results_match(engine.run_engine(abi.default_params(), ann, [batch], reference=ref), w)


# RSQC_K4_PART_READS = 1024, RSQC_K4_SUB_CAP = 2048, RSQC_K4_PART_SLOTS = 4096 (rsqc_k4.h): one partition / two, a partition's key
# list full / one beyond, more names than the larger counting instance has slots
@pytest.mark.parametrize("n", [1023, 1024, 1025, 2047, 2049, 4097])
def test_fragment_count_partition_edges(oracle_lib, n):
    """One gene, unpaired reads, n distinct names: geneFragmentCounts = n exactly at the edges of the device's partitioning."""
    rows = [dict(contig="c", type="gene", start=1000, end=60000, strand="+", gene_id="G"),
            dict(contig="c", type="exon", start=1000, end=60000, strand="+", gene_id="G", exon_id="E")]
    ann = Annotation.from_rows(["c"], rows)
    recs = [dict(qname="name%05d" % i, tid=0, pos=1500 + 10 * i, cigar=[(abi.CIG_M, 50)], flag=0, mapq=255, nm=0, mpos=-1, mtid=-1)
            for i in range(n)]
    batch = Batch.from_records(recs)
    p = abi.default_params(unpaired=1)
    want = oracle_lib.run_oracle(p, ann, [batch])
    assert int(want.gene_fragments[0]) == n and int(want.gene_reads[0]) == n
    got = engine.run_engine(p, ann, [batch])
    assert int(got.gene_fragments[0]) == n
    assert_results_match(got, want)
