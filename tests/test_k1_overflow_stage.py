"""classify_long_kernel's LDS stage in front of the general kernel's list (rnaseqc_amd/csrc/rsqc_k1.h: k1e_overflow, k1e_stage_flush) when
it FILLS: four waves reserve slots on one LDS counter, a reservation that no longer fits goes straight to the list in memory, and the
workgroup's flush moves the staged entries behind it.  What the general kernel receives must be exactly the records handed over -- each
once, none invented.

The unit test runs k1e_overflow itself over prescribed calls under the emulation's SEEDED schedule (tests/hostemu/wavemu.h: the next wave
is drawn from the seed and a lane yields after every atomic), because the default round-robin passes the four waves through their
atomics in one fixed order and a race between them cannot show.  (The version that took an overshooting reservation back from the
counter passes every script under round-robin and fails 91 of the 2 600 seeded runs below: 54 of the 200 seeds of end_minus_34, 7 and 8
of end_minus_63 / _64, 4, 8 and 10 of the three ragged scripts -- a slot range handed out twice, another never written and flushed as
poison.  The scripts in which no smaller call can fit behind an overshoot -- far_below, end_minus_0 / _1 / _5, whole waves, one wave --
pass there too, as they must.)
The second test runs the whole kernels on an input that fills the stage several times over, under both schedules."""
import numpy as np
import pytest

from rnaseqc_amd import abi
from tests import cases, hostemu

SEEDS = range(1, 201)
FULL = (1 << 64) - 1


def _low(n):
    return (1 << n) - 1


def _ragged(rng, n_calls, lo=1, hi=64):
    """n_calls masks of lo..hi lanes each, the lanes anywhere in the wave"""
    out = []
    for _ in range(n_calls):
        lanes = rng.choice(64, size=int(rng.integers(lo, hi + 1)), replace=False)
        out.append(int(sum(1 << int(l) for l in lanes)))
    return out


def _scripts():
    rng = np.random.default_rng(31)
    s = {}
    # far below the end: every call is staged
    s["far_below"] = (100, [_ragged(rng, 5, 1, 40) for _ in range(4)])
    # the counter 1024 - k: one wave's 40 lanes overshoot while the others' 5 still fit (ADVICE r6's example is k = 34), more calls behind
    for k in (0, 1, 5, 34, 63, 64):
        s["end_minus_%d" % k] = (1024 - k, [[_low(40)] + [_low(5)] * 3 + _ragged(rng, 3, 1, 12), [_low(5)] * 4 + _ragged(rng, 3, 1, 12),
                                            [_low(5)] * 7, _ragged(rng, 7, 1, 8)])
    # whole waves only: the bases stay multiples of 64 and the stage ends exactly full
    s["whole_waves"] = (0, [[FULL] * 6 for _ in range(4)])
    s["whole_waves_from_832"] = (832, [[FULL] * 3 for _ in range(4)])
    # ragged calls of 1-64 lanes, from an empty stage (passes the end after ~30 calls) and from close to the end
    s["ragged_from_0"] = (0, [_ragged(rng, 14) for _ in range(4)])
    s["ragged_from_900"] = (900, [_ragged(rng, 8) for _ in range(4)])
    s["small_ragged_from_1000"] = (1000, [_ragged(rng, 12, 1, 9) for _ in range(4)])
    # one wave alone (no other wave to race with: the flush bound itself)
    s["one_wave"] = (1000, [[_low(20), _low(7), _low(3), _low(64)], [], [], []])
    return s


SCRIPTS = _scripts()


def _check(got, want, ctl, what):
    assert len(got) == len(want), (what, len(got), len(want), ctl)              # ovf_count = the entries handed over
    assert not np.any(got == np.uint64(hostemu.STAGE_POISON)), (what, "an unwritten stage slot reached the list", ctl)
    srt = np.sort(got)
    assert not np.any(srt[1:] == srt[:-1]), (what, "an entry is listed twice", ctl)
    missing = np.setdiff1d(want, srt)
    assert missing.size == 0, (what, "entries lost", [hex(int(x)) for x in missing[:8]], ctl)
    np.testing.assert_array_equal(srt, want, err_msg=str(what))


@pytest.mark.parametrize("name", list(SCRIPTS))
def test_overflow_stage_under_seeded_schedules(name):
    start, calls = SCRIPTS[name]
    total = start + sum(bin(m).count("1") for w in calls for m in w)
    ends = set()
    for seed in [0] + list(SEEDS):
        got, want, ctl = hostemu.run_overflow_script(start, calls, seed=seed)
        assert len(want) == total
        _check(got, want, ctl, (name, seed))
        # the stage counter is monotone: it ends at everything ever reserved
        assert ctl[0] == total, (name, seed, ctl)
        if total <= hostemu.STAGE_SLOTS:
            assert ctl[1] == hostemu.STAGE_SLOTS                                 # nothing overshot
        else:
            assert start <= ctl[1] <= hostemu.STAGE_SLOTS and ctl[1] > hostemu.STAGE_SLOTS - 64, (name, seed, ctl)
        ends.add(ctl[1])
    if name.startswith("ragged") or name.startswith("small_ragged"):
        assert len(ends) > 3, (name, ends)            # the seeds do order the waves' atomics differently (first failing base moves)


def test_seeded_schedule_is_reproducible_and_off_by_default():
    start, calls = SCRIPTS["ragged_from_900"]
    a = hostemu.run_overflow_script(start, calls, seed=7)
    b = hostemu.run_overflow_script(start, calls, seed=7)
    np.testing.assert_array_equal(a[0], b[0]); assert a[2] == b[2]
    r0 = hostemu.run_overflow_script(start, calls, seed=0)
    r1 = hostemu.run_overflow_script(start, calls)                                # (after seeded runs: the default schedule is back)
    np.testing.assert_array_equal(r0[0], r1[0]); assert r0[2] == r1[2]
    orders = {hostemu.run_overflow_script(start, calls, seed=s)[0].tobytes() for s in range(1, 9)}
    assert len(orders) > 1


def _compare(o, r):
    for i, n in enumerate(abi.COUNTER_NAMES):
        assert int(o.counters[i]) == int(r.counters[i]), n
    np.testing.assert_array_equal(o.gene_reads, r.gene_reads)
    np.testing.assert_array_equal(o.gene_unique, r.gene_unique)
    np.testing.assert_array_equal(o.gene_fragments, r.gene_fragments)
    np.testing.assert_allclose(o.exon_reads, r.exon_reads, rtol=0, atol=1e-9)
    assert o.read_length == r.read_length


@pytest.fixture(scope="module")
def full_stage(oracle_lib):
    ann, batch = cases.full_stage_case()
    p = abi.default_params()
    return p, ann, batch, oracle_lib.run_oracle(p, ann, [batch])


@pytest.mark.parametrize("grid", [1, 2, 3])
def test_whole_kernels_with_a_full_stage(full_stage, grid):
    """12 000 four-block records on four stacked genes: all deferred to classify_long_kernel, whose one to three workgroups each push
    thousands of them through a 1024-entry stage; the general kernel (which the emulation also checks for out-of-range and repeated
    list entries) must count exactly the oracle's numbers -- under round-robin and under a seeded schedule."""
    p, ann, batch, want = full_stage
    n = batch.n
    assert int(want.gene_reads[0]) == n and int(want.gene_reads[1]) == n
    for seed in (0, 1000 + grid):
        o = hostemu.run_k1(p, ann, batch, grid=grid, seed=seed)
        _compare(o, want)
        assert o.n_deferred == n
        assert o.n_overflow > 4 * 1024
