"""The edge catalogue of --gene-body, shared by the CPU emulation (tests/test_genebody_host.py) and the C ABI on the GPU
(tests/test_gpu_genebody.py): explicit models over small tracks, records from the synthetic writers.  Expected sums always come from
tests/genebody_ref.py over the depth of tests/track_ref.py."""
import functools

import numpy as np

from rnaseqc_amd import abi
from rnaseqc_amd.model import Batch
from tests import genebody_ref as ref
from tests import track_ref

M, N = abi.CIG_M, abi.CIG_N
ITEM = 4096                                         # RSQC_GENEBODY_ITEM: most model bases of one wave's item
NAMES = ["chrA", "chrB", "chrC"]
LENGTHS = [40_000, 9_000, 3_000]
BIG_L = 7_000_000                                   # the bin above 2^32: 70 000 records over one gene of 7 000 000 bases
BIG_RECORDS = 70_000
MANY = 70_000                                       # genes of L = 100
MANY_EMU = 3_000                                    # ... under the emulation (a fiber per lane: 70 000 items are 4.5 M fibers)


def _reads(seed, tid, lo, hi, n):
    """n records inside [lo, hi) of contig tid: plain and spliced, piled unevenly so that a profile and its mirror differ."""
    r = np.random.default_rng(seed)
    recs = []
    for k in range(n):
        span = hi - lo - 80
        p = lo + int(span * r.random() ** 2)        # denser towards lo
        recs.append(dict(tid=tid, pos=p, cigar=[(M, 30), (N, 15), (M, 25)] if k % 3 == 0 else [(M, 50)]))
    return recs


def _everywhere(seed=1):
    return _reads(seed, 0, 0, LENGTHS[0], 4000) + _reads(seed + 1, 1, 0, LENGTHS[1], 900) + _reads(seed + 2, 2, 0, LENGTHS[2], 300)


def _catalogue():
    """name -> (lengths, records or None, [(tid, segments, reverse)])"""
    c = {}
    ev = _everywhere()
    c["lengths_99_100_101_199"] = (LENGTHS, ev, [(0, [(500, 599)], 0), (0, [(700, 800)], 0), (0, [(900, 1001)], 1), (0, [(1100, 1299)], 0)])
    segs = [(2000, 2100), (2400, 2500), (3000, 3100)]
    c["same_reads_forward_and_reverse"] = (LENGTHS, ev, [(0, segs, 0), (0, segs, 1)])
    c["hundred_one_base_segments"] = (LENGTHS, ev, [(0, [(1000 + 3 * k, 1001 + 3 * k) for k in range(100)], 0), (0, [(1000 + 3 * k, 1001 + 3 * k) for k in range(100)], 1)])
    c["segments_of_63_64_65"] = (LENGTHS, ev, [(0, [(100, 163), (200, 264), (300, 365)], 0), (0, [(100, 165), (200, 264), (300, 363)], 1), (1, [(10, 74), (74, 138)], 0)])
    # L = 1000: a bin edge every 10 bases; the first segment ends at u = 37, inside the first round of 64 lanes, three bases into bin 3
    c["bin_edge_and_segment_edge_in_one_round"] = (LENGTHS, ev, [(0, [(100, 137), (200, 1163)], 0), (0, [(100, 137), (200, 1163)], 1), (0, [(5000, 5005), (5010, 5129)], 0)])
    c["item_edges"] = (LENGTHS, ev, [(0, [(100, 100 + ITEM - 1)], 0), (0, [(100, 100 + ITEM)], 1), (0, [(100, 100 + ITEM + 1)], 0),
                                     # three items and five bases; a segment that ends exactly where the second item starts, one that straddles the third
                                     (0, [(1000, 1000 + ITEM), (6000, 6000 + ITEM + 700), (12000, 12000 + ITEM - 695)], 1),
                                     (0, [(20_000 + 50 * k, 20_000 + 50 * k + 43) for k in range(300)], 0)])
    c["overlapping_genes_on_opposite_strands"] = (LENGTHS, ev, [(0, [(3000, 3400), (3600, 3900)], 0), (0, [(3200, 3700), (3800, 4100)], 1)])
    c["starts_at_zero_of_contig_0"] = (LENGTHS, ev + [dict(tid=0, pos=0, cigar=[(M, 40)])] * 5, [(0, [(0, 150)], 0), (0, [(0, 1), (2, 101)], 1)])
    c["starts_at_zero_of_a_later_contig"] = (LENGTHS, ev + [dict(tid=1, pos=0, cigar=[(M, 40)])] * 3 + [dict(tid=0, pos=LENGTHS[0] - 30, cigar=[(M, 30)])] * 7,
                                             [(1, [(0, 120)], 0), (2, [(0, 100)], 1)])
    c["ends_at_a_contigs_last_base"] = (LENGTHS, ev + [dict(tid=t, pos=LENGTHS[t] - 20, cigar=[(M, 20)]) for t in (0, 1, 2, 2)] + [dict(tid=1, pos=0, cigar=[(M, 9)])] * 4,
                                        [(0, [(LENGTHS[0] - 130, LENGTHS[0])], 0), (1, [(LENGTHS[1] - 100, LENGTHS[1])], 1), (2, [(0, 100), (LENGTHS[2] - 1, LENGTHS[2])], 0)])
    c["zero_segments_and_zero_depth"] = (LENGTHS, _reads(5, 0, 0, 5000, 500), [(0, [], 0), (0, [(100, 400)], 0), (0, [], 1), (1, [(100, 400)], 1), (0, [(30_000, 30_200)], 0)])
    c["no_genes"] = (LENGTHS, ev, [])
    c["no_records"] = (LENGTHS, None, [(0, [(100, 400)], 0), (1, [(0, 100)], 1)])
    c["unmeasured_only"] = (LENGTHS, ev, [(0, [(100, 150)], 0), (0, [(100, 199)], 1), (0, [], 0)])
    return c


SMALL = list(_catalogue())
LARGE = ["many_genes_of_100", "bin_above_2_pow_32"]


def _many(n):
    return [(0, [((7 * g) % (LENGTHS[0] - 100), (7 * g) % (LENGTHS[0] - 100) + 100)], g & 1) for g in range(n)]


@functools.lru_cache(maxsize=None)
def case(name, emu=False):
    """(lengths, batches, model, depth arrays, expected sums, expected info)."""
    if name == "many_genes_of_100":
        lengths, recs, genes = LENGTHS, _everywhere(), _many(MANY_EMU if emu else MANY)
    elif name == "bin_above_2_pow_32":
        lengths, recs, genes = [BIG_L + 3, 500], None, [(0, [(2, BIG_L + 2)], 1), (1, [(0, 500)], 0)]
    else:
        lengths, recs, genes = _catalogue()[name]
    model = ref.make_model(genes)
    if name == "bin_above_2_pow_32":
        b = Batch.from_records([dict(tid=0, pos=2, cigar=[(M, BIG_L)])])
        batches = [b.take(np.zeros(BIG_RECORDS, np.int64))]             # the same record 70 000 times
        depth = [np.zeros(lengths[0], np.int64), np.zeros(lengths[1], np.int64)]
        depth[0][2:BIG_L + 2] = BIG_RECORDS
    else:
        batches = [] if recs is None else [Batch.from_records(recs)]
        depth = ref.depth_arrays(track_ref.track(batches, lengths), lengths)
    want, info = ref.sums(depth, model)
    _by_hand(name, emu, model, depth, want, info)
    return lengths, batches, model, depth, want, info


def _by_hand(name, emu, model, depth, want, info):
    """What a reader of the contract can check without the reference."""
    w = want.astype(np.int64) if name != "bin_above_2_pow_32" else want
    if name == "lengths_99_100_101_199":
        assert info["n_measured"] == 3 and info["model_bases"] == 400 and not w[0].any()
        assert (w[1] == depth[0][700:800]).all() and w[1].sum() > 0              # L = 100: every bin one base
        assert w[2].sum() == depth[0][900:1001].sum() and w[3].sum() == depth[0][1100:1299].sum()
    if name == "same_reads_forward_and_reverse":
        assert (w[1] == w[0][::-1]).all() and (w[0] != w[0][::-1]).any()         # (L = 300: a multiple of 100, so the mirror is exact)
    if name == "hundred_one_base_segments":
        assert (w[0] == depth[0][1000:1300:3]).all() and (w[1] == w[0][::-1]).all() and w[0].sum() > 0
    if name == "item_edges":
        L = ref.gene_lengths(model)
        assert [int(x) for x in L] == [ITEM - 1, ITEM, ITEM + 1, 3 * ITEM + 5, 300 * 43] and 3 * ITEM < 300 * 43 < 4 * ITEM
    if name == "zero_segments_and_zero_depth":
        assert info["n_genes"] == 5 and info["n_measured"] == 3 and w[1].sum() > 0 and not w[3].any() and not w[4].any()
    if name == "no_genes":
        assert info == dict(n_genes=0, n_measured=0, model_bases=0, depth_sum=0) and want.shape == (0, 100)
    if name == "no_records":
        assert info["n_measured"] == 2 and info["depth_sum"] == 0
    if name == "unmeasured_only":
        assert info["n_measured"] == 0 and info["depth_sum"] == 0 and info["n_genes"] == 3
    if name == "ends_at_a_contigs_last_base":
        assert w[0][99] >= 1 and w[1][0] >= 1 and w[2][99] == 2
    if name == "many_genes_of_100":
        assert info["n_measured"] == (MANY_EMU if emu else MANY) and info["depth_sum"] > 0
    if name == "bin_above_2_pow_32":
        assert (want[0] == np.uint64(BIG_RECORDS * (BIG_L // 100))).all() and int(want[0][0]) > 1 << 32 and not want[1].any()
        assert info["depth_sum"] == BIG_RECORDS * BIG_L


# every model rule violated once: (lengths, [(tid, segments, reverse)], a word of the message)
BROKEN = {
    "contig_below_zero": ([(-1, [(0, 100)], 0)], "contig"),
    "contig_beyond_the_track": ([(3, [(0, 100)], 0)], "contig"),
    "two_contigs_in_one_gene": ([(0, [(0, 100)], 0), (0, [(0, 100), (200, 300)], 0)], "another contig"),
    "empty_segment": ([(0, [(0, 100)], 0), (0, [(10, 60), (70, 70), (80, 200)], 0)], "empty"),
    "end_in_front_of_start": ([(0, [(100, 50)], 0)], "empty"),
    "ends_beyond_the_contig": ([(2, [(2950, 3001)], 0)], "beyond"),
    "starts_beyond_the_contig": ([(1, [(9000, 9100)], 0)], "beyond"),
    "descending": ([(0, [(500, 600), (100, 200)], 1)], "ascending"),
    "overlapping": ([(0, [(100, 200), (199, 300)], 0)], "ascending"),
}


def broken_model(name):
    genes, word = BROKEN[name]
    m = ref.make_model(genes)
    if name == "two_contigs_in_one_gene":
        m["seg_tid"][2] = 1
    return m, word, ("gene %d" % (len(genes) - 1))
