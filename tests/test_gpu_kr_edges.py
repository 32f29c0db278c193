"""-m gpu: the Read Length stage KR on the device at its walk, gate and range edges.  Every case of tests/kr_cases.py goes through the C
ABI -- plain batches, one batch per range, ONE batch of ranges (Batch.concat_ranges), the ranges of a case dealt to two shards -- and is
compared with tests/kr_ref.py: `read_length` after rsqc_finalize, and the shard summary's batch_file_index / rl_offset / rl_span / rl_state
entry by entry; the cases without an error also with the oracle's own walk.  tests/test_kr_edges_host.py proves the same cases under the
emulation, where the kernel's inputs and raw summary slots are visible; here they meet the real wave, the state carried on the device
from batch to batch, the host's read-back and composition, and the --legacy producer (rsqc_kernels.hip), which the emulation leaves out.

One context per parameter set (default, --legacy), reset between cases.  The case with 129 prefix maxima ends its pass with
RSQC_ERR_CAPACITY and a message that names the limit: a clean return (read_length_kernel stores a walk only below RSQC_RL_MAXP; the emulation
checks the words behind the slot), after which the same context must be right again."""
import functools
import os
import subprocess

import numpy as np
import pytest

from rnaseqc_amd import abi, bamio, distributed, engine
from tests import kr_cases, kr_ref

pytestmark = pytest.mark.gpu

CASES = {c.name: c for c in kr_cases.cases()}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def contexts():
    """one context per parameter set, made on first use, holding the catalogue's one annotation"""
    made = {}

    def get(case):
        if case.legacy not in made:
            e = engine.Engine(kr_cases.params(case))
            e.set_annotation(kr_cases.annotation())
            made[case.legacy] = e
        return made[case.legacy]
    yield get
    for e in made.values():
        e.close()


@functools.lru_cache(maxsize=None)
def _oracle_read_length(name):
    """the oracle's walk over the file's batches in file order, computed once per case"""
    from oracle import binding
    case = CASES[name]
    return int(binding.run_oracle(kr_cases.params(case), kr_cases.annotation(), kr_cases.part_batches(case)).read_length)


def _run(e, batches):
    e.reset()
    for b in batches:
        e.submit(b)
    r = e.finalize()
    return int(r.read_length), e.shard_summary()


def _check_summary(case, si, ks):
    """the shard summary against the parts `ks` of the case, entry by entry"""
    np.testing.assert_array_equal(si.batch_file_index, np.array([case.file_index[k] for k in ks], np.uint64), err_msg=case.name)
    np.testing.assert_array_equal(si.batch_records, np.array([len(case.parts[k]) for k in ks], np.uint64), err_msg=case.name)
    tables = [case.device_tables[k] for k in ks]
    np.testing.assert_array_equal(si.rl_offset, np.concatenate([[0], np.cumsum([len(t[0]) for t in tables])]), err_msg=case.name)
    np.testing.assert_array_equal(si.rl_span, np.array([x for t in tables for x in t[0]], np.int64), err_msg=case.name)
    np.testing.assert_array_equal(si.rl_state, np.array([x for t in tables for x in t[1]], np.int64), err_msg=case.name)


def _expect_capacity(e, batches):
    with pytest.raises(engine.EngineError) as err:                       # no value: the pass ends with the error
        _run(e, batches)
    assert err.value.code == abi.ERR_CAPACITY
    assert "Read Length" in str(err.value) and "128" in str(err.value), str(err.value)
    assert "Read Length" in e.last_error() and "128" in e.last_error()


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if not c.error])
def test_named_case(oracle_lib, contexts, name):
    case = CASES[name]
    e = contexts(case)
    every = list(range(len(case.parts)))
    got, si = _run(e, kr_cases.part_batches(case))                       # plain batches / one batch per range: the state is carried on the device
    assert got == case.final == kr_ref.state_machine(case.records, 0, case.legacy), (case, got, case.final)
    _check_summary(case, si, every)
    assert got == _oracle_read_length(name)
    if case.mode == "ranges":
        got, si = _run(e, [kr_cases.range_batch(case)])                   # ONE batch of ranges: a wave per segment, composed on the host
        assert got == case.final, (case, got, case.final)
        _check_summary(case, si, every)
    if case.shards:
        infos = []
        for which in case.shards:
            got, si = _run(e, [kr_cases.range_batch(case, which)])
            assert got == kr_ref.compose([case.tables[k] for k in which])
            _check_summary(case, si, which)
            infos.append(si)
        assert distributed.compose_read_length(infos) == distributed.compose_read_length(infos[::-1]) == case.final


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c.error])
def test_more_than_128_prefix_maxima_end_the_pass_and_a_reset_recovers(oracle_lib, contexts, name):
    case = CASES[name]
    e = contexts(case)
    _expect_capacity(e, kr_cases.part_batches(case))
    small = CASES["value_l_qseq_0_on_an_eligible_record"]
    got, si = _run(e, kr_cases.part_batches(small))                      # the same context, reset
    assert got == small.final
    _check_summary(small, si, [0])
    if case.mode == "ranges":
        _expect_capacity(e, [kr_cases.range_batch(case)])
        full = CASES["walks_128_prefix_maxima"]                           # ... and a pass at the limit itself
        got, si = _run(e, kr_cases.part_batches(full))
        assert got == full.final == _oracle_read_length(full.name)
        _check_summary(full, si, [0])


def test_command_line_one_gpu_and_two_shards(tmp_path):
    """A ranges case as a BAM file through the command line, on one GPU and sharded by contig over two contexts (both on the one GPU): the
    "Read Length" line of both metrics files is the reference's -- the two-shard run is the one that composes the shards' tables in
    merge_shards (host/main.cpp)."""
    from tests.test_host_cli_pieces import read_table
    cli = os.path.join(ROOT, "rnaseqc_amd", "bin", "rnaseqc")
    if not os.path.exists(cli):                                           # (the build makes it; a second make would compile the library again here)
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "rnaseqc_amd", "csrc"), "cli"])
    case = CASES["ranges_two_shards_whose_order_is_not_file_order"]
    # (the case's own check: the command line's packing deals contigs 1, 2 and 0, 3 to the two shards, and their tables composed shard
    #  after shard, in either order, give another value than in file order -- the sort in merge_shards decides)
    for order in (case.shards[0] + case.shards[1], case.shards[1] + case.shards[0]):
        assert kr_ref.compose([case.tables[k] for k in order]) != case.final
    gtf, bam = str(tmp_path / "kr.gtf"), str(tmp_path / "kr.bam")
    bamio.write_gtf(gtf, kr_cases.annotation())
    bamio.write_bam_fast(bam, kr_cases.contigs(), kr_cases.file_batch(case), threads=2, bai=True)     # (the file of bamio.write_bam, and its index: --gpus needs it)
    one = subprocess.run([cli, gtf, bam, str(tmp_path / "one"), "-vv"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert one.returncode == 0, one.stderr.decode()
    two = subprocess.run([cli, gtf, bam, str(tmp_path / "two"), "-vv", "--gpus", "2"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, RSQC_GPU_LIST="0,0"))
    assert two.returncode == 0, two.stderr.decode()
    assert "on 2 GPUs" in two.stdout.decode()
    for d in ("one", "two"):
        m = dict(read_table(str(tmp_path / d / "kr.bam.metrics.tsv")))
        assert m["Read Length"] == str(case.final), (d, m["Read Length"], case.final)
        assert m["Total Alignments"] == str(case.n)
