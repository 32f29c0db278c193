"""No GPU needed: the named cases of tests/k5_cases.py through the unmodified fragment-size kernels (rnaseqc_amd/csrc/rsqc_k5.h) on the
64-lane emulation (tests/hostemu/k5_emu.cpp: k5emu_run_cands / k5emu_partition; launched by the library's own plan, rsqc_k5_plan.h;
arrays of the size a stage needs, each with a guard entry behind it).

Per case and schedule: the error word; the offsets against numpy's bincount / cumsum and the scatter against the buckets; the listed buckets
and the PATH every non-empty bucket took (the set, the LDS sort, listed) against what the case states; raw samples, kept samples, the
select's final state, `top`, the sizes beyond the table and the (size, count) pairs against walk() -- a case cannot drift off the edge it
is named for.

Schedules: every case runs round-robin; the cases tagged "set" also under 20 seeded schedules (the order of the set's atomicCAS decides
which member of a slot is 0 and which 1), the other small ones under two.

The cases tagged "sanitize" also run through the stand-alone form of k5_emu.cpp (-DK5EMU_MAIN) built with the address and
undefined-behaviour sanitizers, as a child process: __shared__ is static storage under wavemu.h, so a store one entry past s_stash, part,
h or the size table's LDS copy is a global-buffer-overflow there."""
import os
import subprocess

import numpy as np
import pytest

from rnaseqc_amd import abi
from tests import hostemu, k5_cases

SET_SEEDS = tuple(range(1, 21))
FEW_SEEDS = (1, 2)
SMALL = 20000                                       # candidates up to which a case takes the seeded schedules and the per-record emulation

ALL = k5_cases.cases()
FULL = [c for c in ALL if c.emulate == "full"]
PARTITION = [c for c in ALL if c.emulate is not None]
WITH_RECORDS = [c for c in ALL if c.rec is not None and c.n <= SMALL]
SANITIZE = [c for c in ALL if "sanitize" in c.tags]


def _check_partition(case, o):
    e = case.expect
    assert o.rc == 0, (case, o.rc)
    nb = k5_cases.n_buckets(case.n)
    assert o.n == case.n and o.n_buckets == nb == e.get("n_buckets", nb)
    fills = case.fills()
    np.testing.assert_array_equal(o.count, fills)
    np.testing.assert_array_equal(o.off, np.concatenate([[0], np.cumsum(fills)]))
    np.testing.assert_array_equal(np.sort(o.perm), np.arange(case.n))
    np.testing.assert_array_equal(k5_cases.bucket_of(case.cols["qhash"][o.perm], nb), np.repeat(np.arange(nb), fills))
    for b, m in e.get("fill", {}).items():
        assert int(fills[b]) == m, (case, b)
    if "empty" in e:
        assert int((fills == 0).sum()) == e["empty"]
    listed = np.flatnonzero(fills > k5_cases.PB_CAP)
    assert o.big0 == len(listed)                                         # (counted beyond the list's capacity too)
    assert o.error == e.get("error", 0) == (abi.ERR_CAPACITY if len(listed) > k5_cases.PB_BIG_MAX else 0)
    if not o.error:
        np.testing.assert_array_equal(o.listed, listed)
    else:
        assert len(o.listed) == k5_cases.PB_BIG_MAX and set(o.listed.tolist()) < set(listed.tolist())
    if "listed" in e:
        assert listed.tolist() == sorted(e["listed"])
    assert len(listed) >= e.get("listed_min", 0)
    return fills, listed


def _check(case, o, seed):
    e = case.expect
    fills, listed = _check_partition(case, o)
    # ---- the path of every bucket
    want_path = np.where(fills == 0, 0, np.where(fills > k5_cases.PB_CAP, 3, -1))
    known = o.path.copy()
    np.testing.assert_array_equal(known[want_path >= 0], want_path[want_path >= 0])
    stated = e.get("path", {})
    for b, p in stated.items():
        assert hostemu.K5_PATHS[int(o.path[b])] == p, (case, seed, b, hostemu.K5_PATHS[int(o.path[b])])
    if stated:
        assert set(np.flatnonzero(fills).tolist()) == set(stated), "a case that states paths states the path of every non-empty bucket"
    assert ((o.path[(fills > 0) & (fills <= k5_cases.PH_SLOTS // 2)] == 1) | (o.path[(fills > 0) & (fills <= k5_cases.PH_SLOTS // 2)] == 2)).all()
    assert (o.path[(fills > k5_cases.PH_SLOTS // 2) & (fills <= k5_cases.PB_CAP)] == 2).all()
    # ---- samples, selection, sizes against the walk
    samples, kept, pairs = case.reference()
    assert o.raw == samples, (case, seed)
    assert o.n_samples == len(samples) == e.get("samples", len(samples))
    if "raw" in e:
        assert samples == e["raw"]
    if case.max_samples == 0 or not samples:                             # (run_fragment_sizes returns before the select / with nothing)
        assert o.n_kept == 0 and o.pairs == [] and e.get("kept", 0) == 0
        return
    assert o.kept == kept and o.n_kept == len(kept) == e.get("kept", len(kept)), (case, seed)
    assert o.state == (kept[-1][0], 1) and kept[-1][0] == e.get("last_kept", kept[-1][0])      # the prefix: the last kept file index, itself the one sample still wanted
    in_table = [s for _, s in kept if s < k5_cases.SIZE_TABLE]
    assert o.top == (max(in_table) if in_table else 0) == e.get("top", o.top)
    assert o.beyond == sorted(s for _, s in kept if s >= k5_cases.SIZE_TABLE) == e.get("beyond", o.beyond)
    assert o.n_table_pairs == len(set(in_table)) == e.get("table_pairs", len(set(in_table)))
    assert o.pairs == pairs == e.get("pairs", pairs), (case, seed)
    assert len(pairs) == e.get("distinct", len(pairs))


def _seeds(case):
    if "set" in case.tags:
        return (0,) + SET_SEEDS
    return (0,) + (FEW_SEEDS if case.n <= SMALL else ())


@pytest.mark.parametrize("case", FULL, ids=lambda c: c.name)
def test_named_case_under_the_emulation(case):
    for seed in _seeds(case):
        _check(case, hostemu.run_k5_cands(case.cols, case.max_samples, seed), seed)


@pytest.mark.parametrize("case", [c for c in PARTITION if c.emulate == "partition"], ids=lambda c: c.name)
def test_partition_kernels_alone(case):
    """the bucket counts whose replay the emulation leaves to the device: count / scan / scatter against numpy"""
    _check_partition(case, hostemu.run_k5_partition(case.cols["qhash"]))


@pytest.mark.parametrize("case", WITH_RECORDS, ids=lambda c: c.name)
def test_records_give_back_the_candidate_columns(case):
    """What tests/test_gpu_k5_edges.py submits (k5_cases.annotation / bed / batch): under the per-record kernel's emulation every record is a
    candidate, and the candidates' columns are the case's."""
    b = k5_cases.batch(case)
    assert (np.diff(b.pos) > 0).all() and len(k5_cases.three_batches(b)) == 3
    o = hostemu.run_k1(k5_cases.params(case), k5_cases.annotation(case), b, bed=k5_cases.bed(case))
    assert o.n_candidates == case.n
    order = np.argsort(case.cols["file_index"])
    for f in k5_cases.COLUMNS:
        np.testing.assert_array_equal(np.asarray(o.candidates[f]).astype(np.int64), case.cols[f][order].astype(np.int64), err_msg=f)


@pytest.mark.parametrize("case", [c for c in ALL if c.device and not c.slow_device], ids=lambda c: c.name)
def test_named_case_as_records_through_the_oracle(oracle_lib, case):
    """the records form through the oracle's own QNAME-keyed walk: sizes, counts and the samples left equal walk()'s"""
    want = oracle_lib.run_oracle(k5_cases.params(case), k5_cases.annotation(case), [k5_cases.batch(case)], bed=k5_cases.bed(case))
    _, kept, pairs = case.reference()
    np.testing.assert_array_equal(want.fragment_size, np.array([s for s, _ in pairs], np.int64))
    np.testing.assert_array_equal(want.fragment_count.astype(np.int64), np.array([c for _, c in pairs], np.int64))
    assert want.fragment_samples_remaining == case.max_samples - len(kept)


def test_large_cases_restate_their_columns():
    """the cases too long for the per-record emulation: the records form against the rule of rsqc_device.h, restated (bit 31 of flag_size
    = !MateReverse && Reverse && pos != mpos; endpos = pos + the block's length; the interval that holds the block)"""
    for case in (c for c in ALL if c.rec is not None and c.n > SMALL):
        b, bd = k5_cases.batch(case), k5_cases.bed(case)
        pos = b.pos.astype(np.int64)
        order = np.argsort(case.cols["file_index"])
        ok = ((b.flag & 0x20) == 0) & ((b.flag & 0x10) != 0) & (b.pos != b.mpos)
        np.testing.assert_array_equal(case.cols["flag_size"][order], np.abs(b.isize.astype(np.int64)).astype(np.uint32) | (ok.astype(np.uint32) << np.uint32(31)))
        np.testing.assert_array_equal(case.cols["endpos"][order], pos + (b.cigar >> 4))
        iv = np.searchsorted(bd.start.astype(np.int64), pos + 1, side="right") - 1
        assert (iv >= 0).all() and (bd.end.astype(np.int64)[iv] >= pos + 1 + (b.cigar >> 4)).all() and (np.diff(bd.start) > 0).all()
        np.testing.assert_array_equal(case.cols["interval"][order], iv)
        np.testing.assert_array_equal(case.cols["qhash"][order], b.qhash)
        assert (b.flag & 0x3 == 0x3).all() and (np.diff(pos) > 0).all()


def test_the_catalogue_covers_what_it_names():
    """the sizes the constants call for do appear (a renamed or dropped case shows here, not as silence)"""
    names = {c.name for c in ALL}
    assert {c.n for c in ALL} >= {383, 384, 767, 768, 1024 * 384, 1025 * 384, 2049 * 384, 1024 * 2049, 1025 * 2049}
    fills = set()
    for c in ALL:
        if c.n < 500000:
            fills |= set(int(x) for x in c.fills())
    assert {32, 33, 256, 257, 512, 513, 2047, 2048, 2049, 4096, 4097} <= fills
    assert sum(1 for c in ALL if c.expect.get("error", 0)) == 1
    assert {c.max_samples for c in ALL if c.name.startswith("select_max_samples")} >= {0, 1}
    tops = {c.expect.get("top") for c in ALL}
    assert {0, 1023, 1024, k5_cases.SIZE_TABLE - 1} <= tops
    assert {c.expect.get("distinct") for c in ALL} >= {k5_cases.PAIRS_FIRST, k5_cases.PAIRS_FIRST + 1}
    assert any(len(c.expect.get("listed", ())) == 65 for c in ALL) and "select_file_indices_differ_in_the_top_byte_only" in names
    assert all(c.rec is not None or not c.device for c in ALL)


def test_rule_restatements_against_known_values():
    assert k5_cases.n_buckets(0) == 1 and k5_cases.n_buckets(767) == 1 and k5_cases.n_buckets(768) == 2
    assert int(k5_cases.bucket_of(np.uint64(0xFFFFFFFFFFFFFFFF), 5)) == 4 and int(k5_cases.bucket_of(np.uint64(0x80000000 << 32), 3)) == 1
    lo, hi = k5_cases.high_word_range(3, 1)
    assert int(k5_cases.bucket_of(np.uint64(lo << 32), 3)) == 1 and int(k5_cases.bucket_of(np.uint64((lo - 1) << 32), 3)) == 0
    assert int(k5_cases.bucket_of(np.uint64((hi - 1) << 32), 3)) == 1 and int(k5_cases.bucket_of(np.uint64(hi << 32), 3)) == 2
    assert k5_cases.mix(0, 0) == 1 and k5_cases.mix(k5_cases.K, 1) == 1 and k5_cases.mix(5, 0) == 5


def test_the_emulation_compiles_the_product_headers():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    harness = open(os.path.join(root, "tests", "hostemu", "k5_emu.cpp")).read()
    host = open(os.path.join(root, "rnaseqc_amd", "csrc", "rsqc_fragsize.hip")).read()
    for h in ("rsqc_k5.h", "rsqc_k5_plan.h"):
        assert '#include "../../rnaseqc_amd/csrc/%s"' % h in harness and '#include "%s"' % h in host
    for rule in ("k5_plan(", "k5_bucket_count(", "k5_part_grid("):
        assert rule in harness and rule in host, rule
    assert "n / PB_MEAN" not in harness and "n / PB_MEAN)" not in host           # the rule lives in the plan header alone


def test_named_cases_under_sanitizers(tmp_path):
    """Every set, LDS-sort, listed and size-table case through the stand-alone program.  The program prints what the stages left; the
    numbers must be the walk's."""
    exe = str(tmp_path / "k5_emu")
    # (32 KB of stack per lane: the sanitizer clears a stack's shadow at every switch, and these kernels' frames are small)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-DK5EMU_MAIN", "-DWAVEMU_STACK_BYTES=32768", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wno-unused-function", "-Wno-unused-variable", hostemu.K5_PROGRAM_SOURCE, "-o", exe])
    assert len(SANITIZE) >= 20
    for case in SANITIZE:
        for seed in ((0, 3) if "set" in case.tags else (0,)):
            path = str(tmp_path / "case.bin")
            hostemu.write_k5_case_file(path, case.cols, case.max_samples, seed)
            r = subprocess.run([exe, path], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
            assert r.returncode == 0, (case, seed, r.stdout[-2000:] + r.stderr[-4000:])
            samples, kept, pairs = case.reference()
            got = dict(kv.split("=") for kv in r.stdout.split()[1:])
            assert int(got["rc"]) == 0 and int(got["n"]) == case.n and int(got["samples"]) == len(samples), (case, r.stdout)
            if case.max_samples and samples:
                assert int(got["kept"]) == len(kept) and int(got["pairs"]) == len(pairs), (case, r.stdout)
