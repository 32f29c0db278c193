"""Inputs shared by the track tests (CPU emulation, C ABI on the GPU, command line): fixture A of tests/junction_cases.py and the
crafted one-batch cases.  Expected tracks always come from tests/track_ref.py."""
import functools

import numpy as np

from rnaseqc_amd import abi
from rnaseqc_amd.model import Batch
from tests import junction_cases as jc
from tests import track_ref

M, I, D, N, S, H, P, EQ, X = abi.CIG_M, abi.CIG_I, abi.CIG_D, abi.CIG_N, abi.CIG_S, abi.CIG_H, abi.CIG_P, abi.CIG_EQ, abi.CIG_X

# fixture A: the contigs of tests/junction_cases.py with their lengths
A_NAMES = [c[0] for c in jc.CONTIGS]
A_LENGTHS = [int(x) for x in jc.LENGTHS]
cut = jc.cut

# the crafted cases: three short contigs.  The row kernels own chunks of 4 096 slots and a wave of them 1 024; chrA starts at slot
# 0, so a position of chrA is its slot
NAMES = ["chrA", "chrB", "chrC"]
LENGTHS = [20_000, 9_000, 3_000]
N_CONTIGS = 3
CHUNK = 4096
PILE = [(M, 50), (N, 100), (M, 30)]


@functools.lru_cache(maxsize=None)
def fixture_a_clipped():
    """Fixture A and three records that hang over the end of chrC (fixture A itself stays inside its contigs)."""
    _, reads = jc.fixture_a()
    extra = Batch.from_records([dict(tid=2, pos=A_LENGTHS[2] - 40, cigar=[(M, 100)]), dict(tid=2, pos=A_LENGTHS[2] - 1, cigar=[(M, 10), (N, 50), (M, 10)]),
                                dict(tid=2, pos=A_LENGTHS[2] + 7, cigar=[(M, 30)])])
    extra.file_index_base = reads.n                 # (batches are submitted in file order)
    return [reads, extra]


@functools.lru_cache(maxsize=None)
def fixture_a_track(clipped=False):
    return track_ref.track(fixture_a_clipped() if clipped else [jc.fixture_a()[1]], A_LENGTHS)


def _pile(k, pos=1000):
    return [dict(tid=0, pos=pos, cigar=PILE) for _ in range(k)]


def crafted():
    """name -> records of one batch (None: no batch at all)"""
    c = {}
    c["no_record"] = None
    c["none_in_population"] = [dict(tid=0, pos=100, flag=f, cigar=[(M, 20)]) for f in (abi.FUNMAP, abi.FSECONDARY, abi.FQCFAIL, abi.FSUPP)] + [dict(tid=-1, pos=100, cigar=[(M, 20)])]
    c["one_base_at_zero"] = [dict(tid=0, pos=0, cigar=[(M, 1)])]
    c["last_base_of_a_contig"] = [dict(tid=1, pos=LENGTHS[1] - 1, cigar=[(M, 1)])]
    c["straddles_the_end"] = [dict(tid=0, pos=LENGTHS[0] - 10, cigar=[(M, 30)])]
    c["at_and_beyond_the_end"] = [dict(tid=0, pos=LENGTHS[0], cigar=[(M, 10)]), dict(tid=0, pos=1_000_000, cigar=[(M, 10)]), dict(tid=2, pos=(1 << 31) - 5, cigar=[(M, 100)])]
    c["last_of_a_and_first_of_b"] = [dict(tid=0, pos=LENGTHS[0] - 1, cigar=[(M, 1)]), dict(tid=1, pos=0, cigar=[(M, 1)])]
    c["run_ends_on_a_chunks_last"] = [dict(tid=0, pos=CHUNK - 96, cigar=[(M, 96)])]
    c["run_starts_on_a_chunks_first"] = [dict(tid=0, pos=CHUNK, cigar=[(M, 50)])]
    c["run_spans_three_chunks"] = [dict(tid=0, pos=CHUNK - 6, cigar=[(M, CHUNK + 110)])]
    c["single_bases_63_64_65"] = [dict(tid=0, pos=2 * CHUNK + 63, cigar=[(M, 3)]), dict(tid=0, pos=2 * CHUNK + 64, cigar=[(M, 2)]), dict(tid=0, pos=2 * CHUNK + 65, cigar=[(M, 1)])]
    c["chunk_of_heads_only"] = [dict(tid=0, pos=CHUNK, cigar=[(M, CHUNK)])] + [dict(tid=0, pos=CHUNK + k, cigar=[(M, 1)]) for k in range(1, CHUNK, 2)]
    c["chunk_without_a_head"] = [dict(tid=0, pos=100, cigar=[(M, 50)]), dict(tid=0, pos=2 * CHUNK + 100, cigar=[(M, 50)])]
    for k in (64, 65, 256, 257, 5000):
        c["pile_of_%d" % k] = _pile(k)
    c["alternating_lanes"] = [dict(tid=0, pos=1000 + (k & 1), cigar=PILE) for k in range(300)]
    c["stranger_in_a_pile"] = _pile(100) + [dict(tid=0, pos=1020, cigar=[(M, 7)])] + _pile(100)
    c["d_and_n_do_not_cover"] = [dict(tid=0, pos=100, cigar=[(M, 10), (D, 5), (M, 10), (N, 20), (M, 10)])]
    c["i_s_h_p_do_nothing"] = [dict(tid=0, pos=100, cigar=[(H, 4), (S, 5), (M, 10), (I, 3), (P, 2), (M, 10), (S, 4)])]
    c["eq_and_x_cover"] = [dict(tid=0, pos=100, cigar=[(EQ, 10), (X, 5)])]
    c["empty_operations"] = [dict(tid=0, pos=100, cigar=[(M, 10), (M, 0), (M, 10)]), dict(tid=0, pos=200, cigar=[(M, 10), (N, 0), (D, 0), (M, 10)]), dict(tid=0, pos=300, cigar=[(M, 0)])]
    c["insertion_between_blocks"] = [dict(tid=0, pos=100, cigar=[(M, 20), (I, 3), (M, 20)]), dict(tid=0, pos=100, cigar=[(M, 40)])]
    c["deletion_leaves_a_hole"] = [dict(tid=0, pos=100, cigar=[(M, 10), (D, 5), (M, 10)])]
    c["wide_300_operations"] = [dict(tid=0, pos=50, cigar=[(M, 30)]), dict(tid=2, pos=100, cigar=[(M, 5), (N, 10), (I, 1)] * 100), dict(tid=2, pos=100, cigar=[(M, 5)])]
    c["flags"] = [dict(tid=0, pos=100, flag=f, cigar=[(M, 20)]) for f in (0, abi.FUNMAP, abi.FSECONDARY, abi.FQCFAIL, abi.FSUPP, abi.FDUP, abi.FDUP | abi.FPAIRED | abi.FREVERSE)]
    c["foreign_tids"] = [dict(tid=t, pos=100, cigar=[(M, 20)]) for t in (0, -1, N_CONTIGS, N_CONTIGS + 4)]
    c["depths_9_10_99_100"] = sum(([dict(tid=1, pos=p, cigar=[(M, 10)])] * k for p, k in ((100, 9), (200, 10), (300, 99), (400, 100))), [])
    return c


CRAFTED_NAMES = list(crafted())
# Under the emulation only: a position below 0 (clipped in front of the contig), and a record whose CIGAR offset points past the
# batch's pool -- the events kernel clamps it, but a batch on the GPU is also read by the per-read kernels, which trust the offset
EMU_ONLY = {"starts_in_front_of_the_contig": [dict(tid=0, pos=-3, cigar=[(M, 10)]), dict(tid=1, pos=-20, cigar=[(M, 10)])],
            "cigar_offset_past_the_pool": [dict(tid=0, pos=100, cigar=[(M, 30)]), dict(tid=0, pos=200, cigar=[(M, 30)]), dict(tid=0, pos=300, cigar=[(M, 30)])]}


@functools.lru_cache(maxsize=None)
def crafted_case(name):
    """(batches, expected track); the expectations every reader of the contract can check by hand are asserted here."""
    recs = EMU_ONLY[name] if name in EMU_ONLY else crafted()[name]
    batches = [] if recs is None else [Batch.from_records(recs)]
    if name == "cigar_offset_past_the_pool":       # the second record's operations lie outside the pool, the third's last one too
        b = batches[0]
        b.cigar = np.concatenate((b.cigar[:2], np.array([(20 << 4) | M, (9 << 4) | M], np.uint32)))
        b.n_cigar = b.n_cigar.copy(); b.n_cigar[2] = 3
        b.cigar_off = np.array([0, 77, 2], np.uint32)
    want = track_ref.track(batches, LENGTHS)
    rows = [tuple(int(want[f][k]) for f in track_ref.COLUMNS) for k in range(want["n_rows"])]
    sums = (want["population"], want["aligned_bases"], want["clipped_bases"])
    assert track_ref.covered(want) == want["aligned_bases"]
    La, Lb = LENGTHS[0], LENGTHS[1]
    expect = {
        "no_record": ([], (0, 0, 0)), "none_in_population": ([], (0, 0, 0)),
        "one_base_at_zero": ([(0, 0, 1, 1)], (1, 1, 0)), "last_base_of_a_contig": ([(1, Lb - 1, Lb, 1)], (1, 1, 0)),
        "straddles_the_end": ([(0, La - 10, La, 1)], (1, 10, 20)), "at_and_beyond_the_end": ([], (3, 0, 120)),
        "last_of_a_and_first_of_b": ([(0, La - 1, La, 1), (1, 0, 1, 1)], (2, 2, 0)),
        "run_ends_on_a_chunks_last": ([(0, CHUNK - 96, CHUNK, 1)], (1, 96, 0)), "run_starts_on_a_chunks_first": ([(0, CHUNK, CHUNK + 50, 1)], (1, 50, 0)),
        "run_spans_three_chunks": ([(0, CHUNK - 6, 2 * CHUNK + 104, 1)], (1, CHUNK + 110, 0)),
        "single_bases_63_64_65": ([(0, 2 * CHUNK + 63, 2 * CHUNK + 64, 1), (0, 2 * CHUNK + 64, 2 * CHUNK + 65, 2), (0, 2 * CHUNK + 65, 2 * CHUNK + 66, 3)], (3, 6, 0)),
        "chunk_without_a_head": ([(0, 100, 150, 1), (0, 2 * CHUNK + 100, 2 * CHUNK + 150, 1)], (2, 100, 0)),
        "alternating_lanes": ([(0, 1000, 1001, 150), (0, 1001, 1050, 300), (0, 1050, 1051, 150), (0, 1150, 1151, 150), (0, 1151, 1180, 300), (0, 1180, 1181, 150)], (300, 300 * 80, 0)),
        "stranger_in_a_pile": ([(0, 1000, 1020, 200), (0, 1020, 1027, 201), (0, 1027, 1050, 200), (0, 1150, 1180, 200)], (201, 200 * 80 + 7, 0)),
        "d_and_n_do_not_cover": ([(0, 100, 110, 1), (0, 115, 125, 1), (0, 145, 155, 1)], (1, 30, 0)),
        "i_s_h_p_do_nothing": ([(0, 100, 120, 1)], (1, 20, 0)), "eq_and_x_cover": ([(0, 100, 115, 1)], (1, 15, 0)),
        "empty_operations": ([(0, 100, 120, 1), (0, 200, 220, 1)], (3, 40, 0)),
        "insertion_between_blocks": ([(0, 100, 140, 2)], (2, 80, 0)), "deletion_leaves_a_hole": ([(0, 100, 110, 1), (0, 115, 125, 1)], (1, 20, 0)),
        "cigar_offset_past_the_pool": ([(0, 100, 130, 1), (0, 300, 329, 1)], (3, 59, 0)),
        "flags": ([(0, 100, 120, 3)], (3, 60, 0)), "foreign_tids": ([(0, 100, 120, 1)], (1, 20, 0)),
        "depths_9_10_99_100": ([(1, 100, 110, 9), (1, 200, 210, 10), (1, 300, 310, 99), (1, 400, 410, 100)], (218, 2180, 0)),
        "starts_in_front_of_the_contig": ([(0, 0, 7, 1)], (2, 7, 13)),
    }
    if name in expect:
        assert (rows, sums) == expect[name], (name, rows[:8], sums)
    if name.startswith("pile_of_"):
        k = int(name.split("_")[2])
        assert rows == [(0, 1000, 1050, k), (0, 1150, 1180, k)] and sums == (k, 80 * k, 0)
    if name == "chunk_of_heads_only":
        assert want["n_rows"] == CHUNK and rows[0] == (0, CHUNK, CHUNK + 1, 1) and rows[1] == (0, CHUNK + 1, CHUNK + 2, 2) and rows[-1] == (0, 2 * CHUNK - 1, 2 * CHUNK, 2)
    if name == "wide_300_operations":
        assert len(batches[0].wide_index) == 1 and want["n_rows"] == 101 and rows[1] == (2, 100, 105, 2) and rows[2] == (2, 115, 120, 1) and sums == (3, 535, 0)
    return batches, want
