"""The edge catalogue of --tin, shared by the CPU emulation (tests/test_tin_host.py) and the C ABI on the GPU (tests/test_gpu_tin.py):
explicit models over the small tracks of tests/genebody_cases.py, records from its writers or piled by hand.  Expected rows always come
from tests/tin_ref.py over the depth of tests/track_ref.py; every case also carries what a reader can check without the reference."""
import functools
import math

import numpy as np

from rnaseqc_amd import abi
from rnaseqc_amd.model import Batch
from tests import genebody_cases as gc
from tests import tin_ref as ref
from tests import track_ref

M = abi.CIG_M
ITEM = ref.ITEM
LENGTHS = gc.LENGTHS                                # [40 000, 9 000, 3 000]
BIG_L = 70_000                                      # one gene of 70 000 bases under depth 70 000: S = 4.9e9 > 2^32, 18 items
BIG_RECORDS = 70_000
MANY = 70_000                                       # genes of one base
MANY_EMU = 3_000                                    # ... under the emulation (a fiber per lane)


def _pile(tid, pos, length, times):
    return [dict(tid=tid, pos=pos, cigar=[(M, length)])] * times


# the quiet case: nothing but piles, so that every depth is known by hand
UNIFORM = (0, [(1000, 1300)])                       # depth 7 everywhere
UNIFORM_TWO_SEGMENTS = (0, [(1000, 1100), (1200, 1300)])
ONE_BASE = (0, [(2000, 2100)])                      # depth 100 on base 2050, nothing else
EVERY_SECOND_1 = (0, [(3000, 3200)])                # depth 1 on 3000, 3002, ..
EVERY_SECOND_2 = (0, [(4000, 4200)])                # depth 2 on 4000, 4002, ..
DEPTH_ONE = (0, [(5000, 5150)])                     # depth 1 everywhere
LAST_LANE = (0, [(10_000, 10_000 + ITEM + 70)])     # two items; the second one's last round has 6 live lanes: the peak is on u = L - 1
LANE_ZERO = (0, [(20_000, 20_300)])                 # the peak is on u = 0


def _quiet_records():
    return (_pile(0, 1000, 300, 7) + _pile(0, 2050, 1, 100) + [r for p in range(3000, 3200, 2) for r in _pile(0, p, 1, 1)] +
            [r for p in range(4000, 4200, 2) for r in _pile(0, p, 1, 2)] + _pile(0, 5000, 150, 1))


def _catalogue():
    """name -> (lengths, records or None, [(tid, segments)])"""
    c = {}
    ev = gc._everywhere()
    L0, L1, L2 = LENGTHS
    c["lengths_1_63_64_65_99_100"] = (LENGTHS, ev, [(0, [(500, 501)]), (0, [(600, 663)]), (0, [(700, 764)]), (0, [(800, 865)]), (0, [(900, 999)]), (0, [(1100, 1200)])])
    c["item_edges"] = (LENGTHS, ev, [(0, [(100, 100 + ITEM - 1)]), (0, [(100, 100 + ITEM)]), (0, [(100, 100 + ITEM + 1)]),
                                     # three items and five bases; a segment that ends exactly where the second item starts, one that straddles the third
                                     (0, [(1000, 1000 + ITEM), (6000, 6000 + ITEM + 700), (12000, 12000 + ITEM - 695)]),
                                     (0, [(20_000 + 50 * k, 20_000 + 50 * k + 43) for k in range(300)])])
    c["known_depths"] = (LENGTHS, _quiet_records(), [UNIFORM, UNIFORM_TWO_SEGMENTS, ONE_BASE, EVERY_SECOND_1, EVERY_SECOND_2, DEPTH_ONE])
    c["zero_segments_and_zero_depth"] = (LENGTHS, gc._reads(5, 0, 0, 5000, 500), [(0, []), (0, [(100, 400)]), (0, []), (1, [(100, 400)]), (0, [(30_000, 30_200)])])
    c["peak_on_the_last_live_lane_and_on_lane_0"] = (LENGTHS, ev + _pile(0, LAST_LANE[1][0][1] - 1, 1, 500) + _pile(0, 20_000, 1, 400), [LAST_LANE, LANE_ZERO])
    c["overlapping_genes"] = (LENGTHS, ev, [(0, [(3000, 3400), (3600, 3900)]), (0, [(3200, 3700), (3800, 4100)])])
    c["contig_starts_and_ends"] = (LENGTHS, ev + _pile(1, 0, 40, 3) + _pile(0, L0 - 30, 30, 7) + [dict(tid=t, pos=LENGTHS[t] - 20, cigar=[(M, 20)]) for t in (0, 1, 2, 2)],
                                   [(1, [(0, 120)]), (2, [(0, 100)]), (0, [(L0 - 130, L0)]), (1, [(L1 - 100, L1)]), (2, [(0, 100), (L2 - 1, L2)])])
    c["no_genes"] = (LENGTHS, ev, [])
    c["no_records"] = (LENGTHS, None, [(0, [(100, 400)]), (1, [(0, 100)])])
    return c


SMALL = list(_catalogue())
LARGE = ["many_genes_of_one_base", "sum_above_2_pow_32"]


def _many(n):
    return [(0, [((7 * g) % LENGTHS[0], (7 * g) % LENGTHS[0] + 1)]) for g in range(n)]


def model_of(genes):
    """[(tid, segments)] -> the columns of rsqc_tin_begin (the `reverse` of tests/genebody_ref.make_model stays behind)."""
    m = ref.make_model([(t, segs, 0) for t, segs in genes])
    m.pop("reverse")
    return m


@functools.lru_cache(maxsize=None)
def case(name, emu=False):
    """(lengths, batches, model, depth arrays, expected rows, expected info, L per gene)."""
    if name == "many_genes_of_one_base":
        lengths, recs, genes = LENGTHS, gc._everywhere(), _many(MANY_EMU if emu else MANY)
    elif name == "sum_above_2_pow_32":
        lengths, recs, genes = [BIG_L + 3, 500], None, [(0, [(2, BIG_L + 2)]), (1, [(0, 500)])]
    else:
        lengths, recs, genes = _catalogue()[name]
    model = model_of(genes)
    if name == "sum_above_2_pow_32":
        b = Batch.from_records([dict(tid=0, pos=2, cigar=[(M, BIG_L)])])
        batches = [b.take(np.zeros(BIG_RECORDS, np.int64))]             # the same record 70 000 times
        depth = [np.zeros(lengths[0], np.int64), np.zeros(lengths[1], np.int64)]
        depth[0][2:BIG_L + 2] = BIG_RECORDS
    else:
        batches = [] if recs is None else [Batch.from_records(recs)]
        depth = ref.depth_arrays(track_ref.track(batches, lengths), lengths)
    want, info = ref.rows(depth, model)
    L = ref.gene_lengths(model)
    _by_hand(name, emu, depth, want, info, L)
    return lengths, batches, model, depth, want, info, L


def _close(a, b, L):
    return abs(a - b) <= ref.bound(L) * abs(b)


def _by_hand(name, emu, depth, want, info, L):
    """What a reader of the contract can check without the reference."""
    S, C, X, E = (want[f] for f in ("depth_sum", "covered", "max_depth", "dlog2d"))
    mean, tin, el = ref.values(L, want)
    if name == "lengths_1_63_64_65_99_100":
        assert L.tolist() == [1, 63, 64, 65, 99, 100] and info["n_measured"] == 6 and info["model_bases"] == 392
        assert not el[:5].any() and not tin[:5].any() and S[5] == depth[0][1100:1200].sum() and (S > 0).all()      # L < 100: measured, not eligible
        assert S[0] == X[0] == depth[0][500] and C[0] == 1
    if name == "item_edges":
        assert L.tolist() == [ITEM - 1, ITEM, ITEM + 1, 3 * ITEM + 5, 300 * 43] and 3 * ITEM < 300 * 43 < 4 * ITEM
        assert [ref.items_of(x) for x in L] == [1, 1, 2, 4, 4]
    if name == "known_depths":
        assert L.tolist() == [300, 200, 100, 200, 200, 150]
        # uniform depth d: E = S log2(d) and tin = 100 (one segment or two)
        assert (S[0], C[0], X[0]) == (2100, 300, 7) and _close(E[0], 2100 * math.log2(7), 300) and el[0] and abs(tin[0] - 100) < 1e-9
        assert (S[1], C[1], X[1]) == (1400, 200, 7) and _close(E[1], 1400 * math.log2(7), 200) and el[1] and abs(tin[1] - 100) < 1e-9
        # exactly one covered base: E from that base alone, tin = 100 / L
        assert (S[2], C[2], X[2]) == (100, 1, 100) and E[2] == 100 * math.log2(100) and el[2] and abs(tin[2] - 100 / 100) < 1e-9
        # depth 1 on every second base: E = 0 exactly and 100 exp(H) / L = 50; its mean depth is 0.5, so the FILE prints 0 for it ...
        assert (S[3], C[3], X[3]) == (100, 100, 1) and E[3] == 0.0 and abs(ref.tin_formula(200, 100, 0.0) - 50) < 1e-9 and not el[3] and tin[3] == 0 and mean[3] == 0.5
        # ... depth 2 on every second base is the eligible gene with the same evenness: E = S, tin = 50
        assert (S[4], C[4], X[4]) == (200, 100, 2) and E[4] == 200.0 and el[4] and abs(tin[4] - 50) < 1e-9
        # depth 1 on C = L positions: 100 C / L = 100
        assert (S[5], C[5], X[5]) == (150, 150, 1) and E[5] == 0.0 and el[5] and abs(tin[5] - 100) < 1e-9
    if name == "zero_segments_and_zero_depth":
        zero = np.zeros(1, ref.ROW)[0]
        assert info["n_genes"] == 5 and info["n_measured"] == 3 and S[1] > 0 and all(want[g] == zero for g in (0, 2, 3, 4)) and L.tolist() == [0, 300, 0, 300, 200]
    if name == "peak_on_the_last_live_lane_and_on_lane_0":
        last = LAST_LANE[1][0][1] - 1
        assert L.tolist() == [ITEM + 70, 300] and (L[0] - ITEM) % 64 == 6                      # the last round of the second item: lanes 0 .. 5
        assert X[0] == depth[0][last] >= 500 and depth[0][10_000:last].max() < 500 and X[1] == depth[0][20_000] >= 400 and depth[0][20_001:20_300].max() < 400
    if name == "overlapping_genes":
        assert S[0] == depth[0][3000:3400].sum() + depth[0][3600:3900].sum() and S[1] == depth[0][3200:3700].sum() + depth[0][3800:4100].sum()
        assert info["depth_sum"] == S[0] + S[1] and depth[0][3200:3400].sum() > 0               # (the shared bases count in both)
    if name == "contig_starts_and_ends":
        assert depth[1][0] >= 3 and X[0] >= 3 and depth[2][LENGTHS[2] - 1] == 2 and C[4] >= 1 and depth[0][LENGTHS[0] - 1] >= 8 and X[2] >= 8
    if name == "no_genes":
        assert info == dict(n_genes=0, n_measured=0, model_bases=0, depth_sum=0, covered_bases=0) and want.shape == (0,)
    if name == "no_records":
        assert info["n_measured"] == 2 and info["depth_sum"] == 0 and info["covered_bases"] == 0 and not E.any()
    if name == "many_genes_of_one_base":
        n = MANY_EMU if emu else MANY
        assert info["n_measured"] == n == info["model_bases"] and (C <= 1).all() and (S == X).all() and info["depth_sum"] > 0
    if name == "sum_above_2_pow_32":
        assert int(S[0]) == BIG_RECORDS * BIG_L > 1 << 32 and C[0] == BIG_L and X[0] == BIG_RECORDS and ref.items_of(L[0]) == 18
        assert _close(E[0], BIG_RECORDS * BIG_L * math.log2(BIG_RECORDS), BIG_L) and abs(tin[0] - 100) < 1e-9 and want[1] == np.zeros(1, ref.ROW)[0]


BROKEN = gc.BROKEN


def broken_model(name):
    """The tuples of tests/genebody_cases.BROKEN without their strands: (model, a word of the message, the gene it names)."""
    m, word, gene = gc.broken_model(name)
    m = dict(m)
    m.pop("reverse")
    return m, word, gene
