"""No GPU needed: the named cases of tests/kr_cases.py through the unmodified per-record kernels (rsqc_k1.h) and read_length_kernel
(rsqc_kr.h) on the 64-lane emulation (tests/hostemu/k1_emu.cpp: k1emu_run_kr), at grids of 1, 2 and 5 workgroups, against tests/kr_ref.py.

Per batch or range: the kernel's inputs (tile_span; the extremes rl_stats, or rl_seg armed as rsqc_submit.cpp arms it), P, the flag word
and every table entry of the raw summary slot, the words behind entry P (the slot holds 128 pairs exactly: a 129th would land in the next
batch's slot), the state; and the composition by rsqc_rl_compose.h -- the loop rsqc_finalize.cpp and the command line's shard merge run --
and by distributed.compose_read_length.  The --legacy cases are device code (rsqc_kernels.hip) and run in tests/test_gpu_kr_edges.py only.

The cases tagged "sanitize" also run through the stand-alone form of k1_emu.cpp (-DK1EMU_MAIN) built with the address and
undefined-behaviour sanitizers, as a child process; nothing sanitized is loaded into Python."""
import os
import subprocess

import numpy as np
import pytest

from rnaseqc_amd import abi, distributed
from tests import hostemu, kr_cases, kr_ref

GRIDS = (1, 2, 5)
ALL = kr_cases.cases()
EMULATED = [c for c in ALL if c.emulate]
SANITIZE = [c for c in EMULATED if "sanitize" in c.tags]


def _check_slot(case, k, o, slot, what):
    """entry `slot` of a run against part k of the case; returns False when the part ends the pass (more than 128 prefix maxima)"""
    assert tuple(int(x) for x in o.extremes[slot]) == case.extremes[k], (case, what, k, o.extremes[slot], case.extremes[k])
    assert o.untouched, (case, what, k)
    if case.P[k] > kr_cases.MAXP:
        assert o.P[slot] == kr_cases.MAXP and o.flags[slot] == 1, (case, what, k, o.P, o.flags)         # the cause, for rsqc_last_error
        # ... and the text it becomes (rsqc_rl_compose.h: rl_limit_message, what rsqc_submit.cpp hands to rsqc_last_error)
        assert "Read Length" in o.message and "128" in o.message and "file index %d (%d records)" % (case.file_index[k], len(case.parts[k])) in o.message, o.message
        assert o.tables[slot][0] == case.tables[k][0][:kr_cases.MAXP]
        return False
    assert o.message == "" or any(f for f in o.flags), (case, what, o.message)
    assert o.flags[slot] == 0 and o.P[slot] == len(case.device_tables[k][0]), (case, what, k, o.P, o.flags)
    assert o.tables[slot] == case.device_tables[k], (case, what, k, o.tables[slot], case.device_tables[k])
    return True


def _run_parts_one_by_one(case, grid):
    """plain batches in file order, the state carried as the device carries it; returns [(file index, keys, states)]"""
    p, ann = kr_cases.params(case), kr_cases.annotation(case)
    r, items = 0, []
    for k, b in enumerate(kr_cases.part_batches(case)):
        o = hostemu.run_kr(p, ann, b, grid=grid, r_in=r)
        np.testing.assert_array_equal(o.tile_span, kr_ref.tile_spans(case.parts[k]), err_msg="%s part %d" % (case.name, k))
        if not _check_slot(case, k, o, 0, "batch"):
            assert o.rc == abi.ERR_CAPACITY == o.error, (case, o.rc, o.error)
            return None
        assert o.rc == 0 and o.error == 0, (case, k, o.rc, o.error)
        want = kr_ref.compose(case.tables[:k + 1])
        assert o.state == want == kr_ref.apply_table(case.tables[k], r), (case, k, o.state, want)
        r = o.state
        items.append((case.file_index[k], o.tables[0][0], o.tables[0][1]))
    assert r == case.final
    return items


def _run_as_ranges(case, grid, which=None):
    p, ann = kr_cases.params(case), kr_cases.annotation(case)
    ks = list(range(len(case.parts))) if which is None else list(which)
    b = kr_cases.range_batch(case, ks)
    assert b.seg_file_index is not None and [int(x) for x in b.seg_file_index] == [case.file_index[k] for k in ks]
    o = hostemu.run_kr(p, ann, b, grid=grid, ranges=True)
    np.testing.assert_array_equal(o.tile_span, kr_ref.tile_spans([r for k in ks for r in case.parts[k]]), err_msg=case.name)
    ok = all([_check_slot(case, k, o, slot, "ranges") for slot, k in enumerate(ks)])
    if not ok:
        assert o.rc == abi.ERR_CAPACITY == o.error, (case, o.rc, o.error)
        return None
    assert o.rc == 0 and o.error == 0, (case, o.rc, o.error)
    assert o.state == kr_ref.compose([case.tables[k] for k in ks]), (case, o.state)
    return [(case.file_index[k], o.tables[slot][0], o.tables[slot][1]) for slot, k in enumerate(ks)]


def _shard_info(items):
    off = np.concatenate([[0], np.cumsum([len(t[1]) for t in items])]).astype(np.uint32)
    return distributed.ShardInfo(np.array([t[0] for t in items], np.uint64), np.zeros(len(items), np.uint64), off, np.array([x for t in items for x in t[1]], np.uint32),
                                 np.array([x for t in items for x in t[2]], np.int32), np.zeros(0, np.uint64), np.zeros(0, np.uint32))


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("case", EMULATED, ids=lambda c: c.name)
def test_named_case_under_the_emulation(case, grid):
    one_by_one = _run_parts_one_by_one(case, grid)
    assert (one_by_one is None) == case.error
    runs = [one_by_one]
    if case.mode == "ranges":
        as_ranges = _run_as_ranges(case, grid)
        assert (as_ranges is None) == case.error
        assert as_ranges == one_by_one                                    # the two submissions leave the same tables
        runs.append(as_ranges)
    if case.shards:
        shards = [_run_as_ranges(case, grid, which) for which in case.shards]
        assert sorted(t for s in shards for t in s) == sorted(one_by_one)
        assert distributed.compose_read_length([_shard_info(s) for s in shards]) == case.final
        assert distributed.compose_read_length([_shard_info(s) for s in shards[::-1]]) == case.final
        runs.append([t for s in shards for t in s])                       # (shard by shard: not in file order)
    for items in runs:
        if items is not None:
            assert hostemu.rl_compose(items) == hostemu.rl_compose(items[::-1]) == case.final == distributed.compose_read_length([_shard_info(items)]), (case, items)


@pytest.mark.parametrize("case", ALL, ids=lambda c: c.name)
def test_distributed_restates_the_reference(case):
    """distributed.read_length_transfer / compose_read_length against kr_ref on the parts of every case, the --legacy ones included"""
    parts = list(zip(case.file_index, case.parts))
    assert kr_ref.check_distributed(parts, case.legacy) == case.final
    assert kr_ref.check_distributed(parts[::-1], case.legacy) == case.final


@pytest.mark.parametrize("case", ALL, ids=lambda c: c.name)
def test_named_case_through_the_oracle(oracle_lib, case):
    """the project's oracle walks the same batches record by record (it knows no limit of 128): the value tests/test_gpu_kr_edges.py compares with"""
    got = oracle_lib.run_oracle(kr_cases.params(case), kr_cases.annotation(), kr_cases.part_batches(case))
    assert int(got.read_length) == case.final, (case, int(got.read_length), case.final)


@pytest.mark.parametrize("case", [c for c in EMULATED if "producers" in c.tags], ids=lambda c: c.name)
def test_producer_cases_hand_their_record_on(case):
    """the record that holds the largest span does leave the fast path: classify_ei_kernel defers records, or lists them for the general kernel"""
    b = kr_cases.range_batch(case) if case.mode == "ranges" else kr_cases.file_batch(case)
    o = hostemu.run_k1(kr_cases.params(case), kr_cases.annotation(case), b, grid=1 if "ring" in case.tags else 2)
    assert o.n_deferred + o.n_overflow >= 1, (case, o.n_deferred, o.n_overflow)
    if "ring" in case.tags:
        assert 0 < o.n_deferred < case.n
    assert o.read_length == case.final


def test_the_catalogue_covers_what_it_names():
    names = {c.name for c in ALL}
    plain_P = {c.P[0] for c in ALL if "walks" in c.tags and c.mode == "plain" and "entered" not in c.tags}
    entered = {c.name for c in ALL if "entered" in c.tags}
    assert len(entered) == 5 + 7 + 7 and {"walks_128_keys_entered_%s" % w for w in ("below_key_0", "equal_to_key_63", "between_keys_63_and_64", "equal_to_key_64",
                                                                                   "equal_to_key_100", "equal_to_the_last_key", "above_the_last_key")} <= entered
    assert plain_P == {1, 2, 63, 64, 65, 127, 128, 129}
    assert sum(1 for c in ALL if c.error) == 2 and {c.mode for c in ALL if c.error} == {"plain", "ranges"}
    assert sum(1 for c in ALL if "lowered" in c.tags) >= 7 and sum(1 for c in ALL if "gate" in c.tags) == 5
    for cut in (1, 63, 64, 65):
        entries = {c.name.split("entry_state_")[1] for c in ALL if c.name.startswith("carry_cut_at_%d_" % cut)}
        assert entries == {"below_every_key", "equal_to_a_key", "between_two_keys", "equal_to_the_largest_key", "above_all_keys"}
    assert {c.n for c in ALL if c.name.startswith("value_")} <= {3, 4} and max(c.n for c in ALL) <= 8400 < 2 * kr_cases.GROUP + 64 * 4
    assert any(c.n > 2 * kr_cases.GROUP for c in ALL) and sum(1 for c in ALL if c.legacy) == 2 and sum(1 for c in ALL if c.shards) == 2
    assert {"ranges_four_inside_one_tile", "ranges_boundary_on_a_tile_edge", "ranges_one_starts_in_tile_63_of_a_group", "nothing_eligible_in_the_only_range"} <= names
    assert len(SANITIZE) >= 40 and {t for c in SANITIZE for t in c.tags} >= {"walks", "entered", "lowered", "carry", "ranges", "shards", "producers", "ring"}


def test_reference_against_known_values():
    M, N, S, I = abi.CIG_M, abi.CIG_N, abi.CIG_S, abi.CIG_I
    r = lambda cig, **kw: dict(cigar=cig, flag=kw.pop("flag", 0), **kw)
    assert kr_ref.span(r([(M, 10), (N, 5), (M, 3)])) == 18 and kr_ref.span(r([(S, 4), (I, 2)])) == 1 and kr_ref.span(r([])) == 1
    assert kr_ref.l_qseq(r([(S, 4), (M, 10), (I, 2), (N, 9)])) == 16 and kr_ref.l_qseq(r([(M, 5)], l_qseq=0)) == 0
    assert not kr_ref.eligible(r([(M, 5)], flag=abi.FUNMAP)) and not kr_ref.eligible(r([(M, 5)], flag=abi.FSUPP)) and kr_ref.eligible(r([(M, 5)], flag=abi.FDUP | abi.FPAIRED))
    assert kr_ref.eligible(r([(M, 100001)])) and not kr_ref.eligible(r([(M, 100001)]), legacy=True) and kr_ref.eligible(r([(M, 100000)]), legacy=True)
    recs = [kr_cases.rec(50, 50), kr_cases.rec(5000, 30), kr_cases.rec(40, 45)]
    assert kr_ref.state_machine(recs) == 45 and kr_ref.monotone(recs) == 50 and kr_ref.state_machine(recs, 5000) == 5000 and kr_ref.state_machine(recs, 60) == 45
    assert kr_ref.transfer_table(recs) == ([50, 5000], [45, 45]) and kr_ref.apply_table(([50, 5000], [45, 46]), 50) == 46
    assert kr_ref.extremes(recs) == (5000, 30, 50) and kr_ref.extremes([]) == (0, kr_ref.NO_LENGTH, 0) and kr_ref.tile_spans(recs) == [5000]


def test_the_shared_composition_against_known_values():
    """rsqc_rl_compose.h through the emulation library: the loop rsqc_finalize.cpp and the command line's shard merge call, and the limits
    the wrapper restates"""
    assert hostemu.RL_SUMMARY_WORDS == 2 + 2 * hostemu.RL_MAXP == 258
    assert hostemu.rl_compose([]) == 0 and hostemu.rl_compose([(9, [5], [7]), (3, [4, 8], [6, 2])]) == 6
    assert hostemu.rl_compose([(3, [4, 8], [6, 2]), (9, [5], [7])]) == 6 and hostemu.rl_compose([(3, [5], [7]), (9, [4, 8], [6, 2])]) == 2
    assert hostemu.rl_compose([(1, [5], [5]), (2, [5, 6], [9, 3])]) == 3                   # strict: a key equal to the state does not fire


def test_named_cases_under_sanitizers(tmp_path):
    """Every tagged case through the stand-alone program, plain parts from their entry states and range cases as one batch of ranges.  The
    program prints what the kernel left; the numbers must be the reference's."""
    exe = str(tmp_path / "k1_emu")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-DK1EMU_MAIN", "-DK1E_COARSE", "-DK1E_UNIFORM2=1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wno-unused-function", "-Wno-unused-variable", hostemu.K1_PROGRAM_SOURCE, "-o", exe])
    runs = []                                                              # (path, case, the parts of the run, entry state, ranges)
    for case in SANITIZE:
        p, ann = kr_cases.params(case), kr_cases.annotation(case)
        if case.mode == "ranges":
            path = str(tmp_path / ("%d.bin" % len(runs)))
            hostemu.write_kr_case_file(path, p, ann, kr_cases.range_batch(case), grid=2, ranges=True)
            runs.append((path, case, list(range(len(case.parts))), 0, True))
        else:
            for k, b in enumerate(kr_cases.part_batches(case)):
                path = str(tmp_path / ("%d.bin" % len(runs)))
                hostemu.write_kr_case_file(path, p, ann, b, grid=2, r_in=case.entry[k])
                runs.append((path, case, [k], case.entry[k], False))
    r = subprocess.run([exe] + [x[0] for x in runs], capture_output=True, text=True, timeout=1200, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("k1emu_kr ")]
    assert len(lines) == len(runs)
    for ln, (_, case, ks, r_in, ranges) in zip(lines, runs):
        got = dict(kv.split("=") for kv in ln.split()[1:])
        assert int(got["guard"]) == 0 and int(got["entries"]) == len(ks), (case, ln)
        over = any(case.P[k] > kr_cases.MAXP for k in ks)
        assert int(got["rc"]) == int(got["error"]) == (abi.ERR_CAPACITY if over else 0), (case, ln)
        for slot, k in enumerate(ks):
            want = "%d:%d" % (min(case.P[k], kr_cases.MAXP), 1) if case.P[k] > kr_cases.MAXP else "%d:0" % len(case.device_tables[k][0])
            assert got["P%d" % slot] == want, (case, ln)
        if not over:
            assert int(got["state"]) == kr_ref.compose([case.tables[k] for k in ks], r_in), (case, ln)
