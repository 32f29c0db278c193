"""No GPU needed: the named cases of tests/k4_cases.py through the unmodified fragment-count kernels (rnaseqc_amd/csrc/rsqc_k4.h) on the
64-lane emulation (tests/hostemu/k4_emu.cpp: k4emu_run_pairs, poisoned arrays sized as rsqc_finalize.cpp sizes them).

Per case and schedule: the error word; every gene's count against a Python set; the PLAN (partition counts, capacities, offsets,
part_first[n_genes]) against a plain restatement of the layout rule; the fills frag_local left and the counting instance that takes each
partition against the numbers the case states -- a case cannot drift off the edge it is named for.

Schedules: every case runs round-robin and under three seeded schedules (SEEDS: random wave order, a yield after every atomic), the
set-aside and window cases under six (MORE_SEEDS) -- they are the cheap ones.  Measured on the build container: 65 s for the emulation
tests of this file beside 52 s for tests/test_k4_wave_emulation.py; 27 s of it are the two layouts of more than 65 536 genes (66 layout
workgroups of 1 024 lanes, twice, per schedule), 6 s the 2 048 keys probing from one slot."""
import functools

import numpy as np
import pytest

from tests import hostemu, k4_cases

SEEDS = (0, 1, 2, 3)
MORE_SEEDS = SEEDS + (4, 5, 6)

CASES = [c for c in k4_cases.cases() if c.emulate]
DEVICE_CASES = [c for c in k4_cases.cases() if c.device]


def _schedules(case):
    return MORE_SEEDS if case.tags else SEEDS


@functools.lru_cache(maxsize=4)
def _layout(name):
    return k4_cases.layout(next(c for c in CASES if c.name == name).reads)


def _check(case, o, seed):
    e = case.expect
    assert o.rc == 0, (case, seed, o.rc)
    # ---- the plan, whatever the pairs do
    pf, gi, pi = _layout(case.name)
    np.testing.assert_array_equal(o.part_first, pf)
    np.testing.assert_array_equal(o.ginfo, gi)
    np.testing.assert_array_equal(o.part_info, pi)
    assert o.n_parts == len(pi) == e.get("n_parts", len(pi))
    for g, parts in e.get("parts", {}).items():
        assert int(o.ginfo[g, 1]) == parts, (case, g)
    # ---- the fills and who counts them
    cap = o.part_info[:, 1] if len(pi) else np.zeros(0, np.int64)
    held = np.minimum(o.cursor, cap)
    first = o.part_first
    for (g, k), want in e.get("fill", {}).items():
        got = int(o.cursor[first[g] + k])
        lo, hi = want if isinstance(want, tuple) else (want, want)
        assert lo <= got <= hi, (case, seed, (g, k), got, want)
    listed = np.flatnonzero(held > k4_cases.PART_SLOTS // 4)
    np.testing.assert_array_equal(o.full_list, listed)
    assert o.full_n == len(listed) == e.get("full_n", len(listed))
    for g, k in e.get("large", ()):
        assert first[g] + k in listed, (case, (g, k))
    for g, k in e.get("small", ()):
        assert 0 < held[first[g] + k] <= k4_cases.PART_SLOTS // 4, (case, (g, k))
    # ---- the result
    assert o.error == e.get("error", 0), (case, seed, o.error)
    if o.error == 0:
        assert int(o.cursor.sum()) <= len(case.gene) and (o.cursor <= cap).all()
        np.testing.assert_array_equal(o.gene_frag.astype(np.int64), case.reference(), err_msg="%s seed %d" % (case, seed))


def run(case, seed):
    return hostemu.run_k4_pairs(case.gene, case.key, case.h2, case.n_genes, case.counts, case.chunk_cap, case.slow_cap, case.sharers,
                                case.grids[0], case.grids[1], seed)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_named_case_under_the_emulation(case):
    for seed in _schedules(case):
        _check(case, run(case, seed), seed)


@pytest.mark.parametrize("case", DEVICE_CASES, ids=lambda c: c.name)
def test_named_case_as_records_through_the_oracle(oracle_lib, case):
    """What tests/test_gpu_k4_edges.py submits (k4_cases.annotation / batch: one unpaired read per pair inside its gene, hashes written
    directly): the oracle counts every pair to the gene the case names and agrees with the Python sets -- key 0 merged with the key it
    is counted as included."""
    want = oracle_lib.run_oracle(k4_cases.params(), k4_cases.annotation(case), [k4_cases.batch(case)])
    np.testing.assert_array_equal(want.gene_reads.astype(np.int64), case.reads)
    np.testing.assert_array_equal(want.gene_fragments.astype(np.int64), case.reference())


def test_the_record_builder_against_from_records():
    from rnaseqc_amd.model import Batch
    case = next(c for c in CASES if c.name == "window_key_0_beside_the_key_it_is_counted_as")
    b = k4_cases.batch(case)
    recs = [dict(qname="q%d" % i, tid=0, pos=int(b.pos[i]), cigar=[(k4_cases.abi.CIG_M, k4_cases.READ_LENGTH)], flag=0, mapq=255, nm=0, mpos=-1, mtid=-1)
            for i in range(b.n)]
    r = Batch.from_records(recs)
    for f in ("pos", "mpos", "isize", "cigar_off", "flag", "l_qseq", "mapq", "nm", "tagbits", "n_cigar", "cigar", "seg_tid", "seg_start"):
        np.testing.assert_array_equal(np.asarray(getattr(b, f)).astype(np.int64), np.asarray(getattr(r, f)).astype(np.int64), err_msg=f)
    assert (np.diff(b.pos) >= 0).all() and len(k4_cases.three_batches(b)) == 3


def test_the_catalogue_covers_what_it_names():
    """the sizes the constants call for do appear (a renamed or dropped case shows here, not as silence)"""
    names = {c.name for c in CASES}
    reads = set()
    for c in CASES:
        reads |= set(int(x) for x in c.reads)
    assert {0, 1, 15, 16, 17, 1023, 1024, 1025, 2048, 2049} <= reads
    assert {c.n_genes for c in CASES} >= {1, 63, 64, 65, 1023, 1024, 1025, 65537, 66562}
    assert max(int(c.reads.max()) for c in CASES) == 128 * k4_cases.PART_READS + 1
    for c in CASES:
        if c.expect.get("error", 0):
            assert c.expect["error"] == k4_cases.abi.ERR_CAPACITY
    assert sum(1 for c in CASES if c.expect.get("error", 0)) == 4
    assert any(not c.device for c in CASES) and "layout_65537_genes_counted_gene_in_the_last_workgroup" in names


def test_hash_restatements_against_known_values():
    """k4_cases.part_hash / set_slot / win_slot are the kernels' three lines: pinned by hand-computed values, and by the emulation placing
    steered keys where the helper says (the capacity cases above)."""
    assert int(k4_cases.part_hash(np.uint64(0))) == 0
    h = 0x12345678
    h ^= h >> 15; h = h * 0x2C1B3C6D & 0xFFFFFFFF; h ^= h >> 12
    assert int(k4_cases.part_hash(np.uint64(0x12345678 << 32 | 99))) == h
    assert k4_cases.set_slot(0xABCD00000000, 4096) == 0
    assert k4_cases.gene_mix(0) == 0 and k4_cases.win_slot(0, 1) == ((0x9E3779B1 >> 12) & 2047)
