"""CPU: the kernels of --sort (rnaseqc_amd/csrc/rsqc_sort.h), unmodified, on the 64-lane emulation against std::stable_sort
(tests/hostemu/sort_emu.cpp compares permutation for permutation; numpy's stable argsort is checked here as well)."""
import numpy as np
import pytest

from tests.hostemu import sort as emu

TILE = emu.TILE


def _check(keys, want_passes=None, seed=0):
    keys = np.asarray(keys, np.uint64)
    rc, perm, passes, key_or, key_and = emu.run_sort(keys, seed=seed)
    assert rc == 0, rc
    assert (perm == np.argsort(keys, kind="stable").astype(np.uint32)).all()
    if len(keys):
        assert key_or == int(np.bitwise_or.reduce(keys)) and key_and == int(np.bitwise_and.reduce(keys))
    in_order = len(keys) < 2 or bool((keys[1:] >= keys[:-1]).all())
    if in_order:
        assert passes == -1                      # nothing to do: no radix pass runs
    elif want_passes is not None:
        assert passes == want_passes
    return passes


def _random_keys(n, seed, n_tid=3, max_pos=200_000_000):
    r = np.random.default_rng(seed)
    return emu.make_keys(r.integers(0, n_tid, n), r.integers(0, max_pos, n))


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 1])
def test_record_counts(n):
    _check(_random_keys(n, 100 + n))


def test_all_keys_equal_is_pure_stability():
    assert _check(np.full(TILE + 77, emu.make_keys([3], [12345])[0], np.uint64)) == -1
    # ... and equal keys behind one smaller key at the end: every pass moves the whole run, its order must survive all of them
    keys = np.full(2 * TILE + 5, emu.make_keys([3], [12345])[0], np.uint64)
    keys[-1] = emu.make_keys([0], [7])[0]
    _check(keys)


def test_sorted_and_reversed():
    keys = np.sort(_random_keys(2 * TILE + 300, 5))
    assert _check(keys) == -1
    _check(keys[::-1].copy())


def test_two_contigs_interleaved_record_by_record():
    n = 2 * TILE + 131
    pos = np.repeat(np.arange(n // 2 + 1) * 10, 2)[:n]
    _check(emu.make_keys(np.arange(n) % 2, pos))


def test_odd_tids_and_negative_pos():
    r = np.random.default_rng(9)
    n = TILE + 700
    tid = r.choice(np.array([0, 1, 2, -1, 25, 1 << 20]), n)           # unplaced, and RefIDs a header of 3 contigs does not define
    pos = r.integers(-1, 5000, n)
    keys = emu.make_keys(tid, pos)
    rc, perm, _, _, _ = emu.run_sort(keys)
    assert rc == 0
    st, sp = tid[perm], pos[perm]
    assert (st[-(tid == -1).sum():] == -1).all()                     # tid as unsigned: the unplaced records go last
    u = st.astype(np.int32).view(np.uint32).astype(np.int64)
    assert ((u[1:] > u[:-1]) | ((u[1:] == u[:-1]) & (sp[1:] >= sp[:-1]))).all()    # pos as signed: -1 in front of 0


def test_keys_that_differ_only_in_their_highest_used_digit():
    r = np.random.default_rng(11)
    n = TILE + 9
    keys = emu.make_keys(np.zeros(n), 0x00ABCDEF + (r.integers(0, 100, n) << 24))   # one live digit: bits 24..31 of pos
    assert _check(keys, want_passes=1) == 1


def test_pass_skipping_one_and_eight_live_digits():
    r = np.random.default_rng(12)
    n = TILE + 100
    low = (r.integers(0, 256, n)).astype(np.uint64) | np.uint64(0x0123456789ABCD00)
    assert _check(low, want_passes=1) == 1
    full = r.integers(0, 1 << 63, n, dtype=np.int64).astype(np.uint64) * np.uint64(2) + r.integers(0, 2, n).astype(np.uint64)
    assert _check(full, want_passes=8) == 8
    # human-sized input: 25 contigs (one digit of tid), positions below 2^28 (four digits of pos)
    human = emu.make_keys(r.integers(0, 25, n), r.integers(0, 250_000_000, n))
    assert _check(human, want_passes=5) == 5


def test_runs_of_equal_keys_straddle_tiles_and_workgroups():
    # runs of 300 equal keys laid so that tile ends (2048, 4096) and wave ends (512, 1024, ...) fall inside runs, shuffled run by run
    r = np.random.default_rng(13)
    runs = [np.full(300, emu.make_keys([k % 3], [1000 * (k // 3)])[0], np.uint64) for k in range(21)]
    order = r.permutation(len(runs))
    keys = np.concatenate([runs[k] for k in order])
    assert len(keys) > 3 * TILE
    _check(keys)
    _check(keys, seed=7)                         # the emulation's seeded schedule: another order of the waves


def test_key_build_from_segment_table():
    pos = np.array([5, -1, 7, 7, 0, 3, 2], np.int32)
    seg_tid = np.array([1, 4, -1, 0], np.int32)                      # (segment 1 is empty)
    seg_start = np.array([0, 3, 3, 5, 7], np.uint64)
    tid = np.array([1, 1, 1, -1, -1, 0, 0])
    assert (emu.run_keys(pos, seg_tid, seg_start) == emu.make_keys(tid, pos)).all()


@pytest.mark.parametrize("n,n_in,out_batch", [(1, 1, 4), (700, 3, 1 << 20), (2 * TILE + 50, 5, 777), (1500, 4, 256)])
def test_collect_sort_gather(n, n_in, out_batch):
    rc, batches, moved, passes = emu.run_gather(21 + n, n, n_in, out_batch)
    assert rc == 0, rc
    assert batches == (n + out_batch - 1) // out_batch
    assert n == 1 or (moved > 0 and passes > 0)


def test_collect_gather_of_ordered_input_runs_no_pass():
    rc, batches, moved, passes = emu.run_gather(5, 1200, 3, 500, in_order=True)
    assert rc == 0, rc
    assert (batches, moved, passes) == (3, 0, -1)
