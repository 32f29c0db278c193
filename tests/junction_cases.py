"""Inputs shared by the junction tests (CPU emulation, C ABI on the GPU, command line): fixture A and the crafted one-batch cases.
Expected tables always come from tests/junction_ref.py."""
import functools

import numpy as np

from rnaseqc_amd import abi, synth
from rnaseqc_amd.model import Batch
from tests import junction_ref

CONTIGS = [("chrA", 900_000, 70), ("chrB", 500_000, 40), ("chrC", 300_000, 15)]
LENGTHS = np.array([c[1] for c in CONTIGS])
CS = [(c[0], c[1]) for c in CONTIGS]
N_CONTIGS = len(CONTIGS)
M, I, D, N, S, H, P, EQ, X = abi.CIG_M, abi.CIG_I, abi.CIG_D, abi.CIG_N, abi.CIG_S, abi.CIG_H, abi.CIG_P, abi.CIG_EQ, abi.CIG_X
INT_MAX = (1 << 31) - 1


def unequal_cuts(n, seed, parts):
    cuts = np.sort(np.random.default_rng(seed).choice(np.arange(1, n), parts - 1, replace=False))
    return [0] + [int(x) for x in cuts] + [n]


# fixture A in five unequal batches.  Half the operations so far, the host's bound on the instances, is then 4.4 k, 9.7 k, 17.6 k, 29 k
# and 36 k: from RSQC_JUNCTION_CAP0 = 1024 the collection grows in front of the first four batches (doubling covers the fifth)
FIXTURE_A_CUTS = [0, 5000, 11000, 20000, 33000, 41000]


def cut(batch, seed=None, parts=5):
    c = unequal_cuts(batch.n, seed, parts) if seed is not None else FIXTURE_A_CUTS
    assert c[-1] == batch.n
    return [batch.slice(lo, hi) for lo, hi in zip(c[:-1], c[1:])]


@functools.lru_cache(maxsize=None)
def fixture_a():
    """tests/test_gpu_sort.py's annotation and first read set: (annotation, the records in file order)."""
    ann = synth.make_annotation(seed=51, contigs=CONTIGS)
    reads = synth.make_reads(ann, 20000, seed=52, read_len=150, dup_frac=0.08, keep_qnames=True, contig_lengths=LENGTHS)
    return ann, reads


@functools.lru_cache(maxsize=None)
def fixture_a_table(mapq_threshold=255):
    return junction_ref.junction_table([fixture_a()[1]], N_CONTIGS, mapq_threshold)


def _spliced(k, seed, n_junctions=37):
    """k records of one instance each over n_junctions distinct junctions, in no order."""
    r = np.random.default_rng(seed)
    recs = []
    for i in range(k):
        j = int(r.integers(0, n_junctions))
        recs.append(dict(tid=j % 3, pos=1000 + 700 * j - 20 - int(r.integers(0, 15)), cigar=[(M, 20 + 0), (N, 100 + j), (M, 30)], mapq=(255 if i % 3 else 3)))
        recs[-1]["pos"] = 1000 + 700 * j - recs[-1]["cigar"][0][1]          # the junction's start is fixed: the first block ends in front of it
    return recs


def crafted():
    """name -> (records of one batch, mapq_threshold)"""
    c = {}
    c["zero_instances"] = ([dict(tid=0, pos=100 + i, cigar=[(M, 76)]) for i in range(300)], 255)
    for k in (1, 64, 65, 2048, 2049):
        c["exactly_%d" % k] = (_spliced(k, 900 + k), 255)
    big = [dict(tid=1, pos=5000 - 25 - (i % 7), cigar=[(M, 25 + (i % 7)), (N, 400), (M, 10 + (i % 11))], mapq=(255 if i % 5 else 0)) for i in range(5000)]
    other = [dict(tid=1, pos=3000, cigar=[(M, 30), (N, 90), (M, 30)]), dict(tid=1, pos=5000, cigar=[(M, 30), (N, 90), (M, 30)])]
    c["run_across_workgroups"] = (big[:2500] + other + big[2500:], 255)
    c["same_start_other_end"] = ([dict(tid=0, pos=980, cigar=[(M, 20), (N, 100 + 10 * (i % 4)), (M, 20)]) for i in range(40)], 255)
    c["same_start_end_other_tid"] = ([dict(tid=i % 3, pos=980, cigar=[(M, 20), (N, 100), (M, 20)]) for i in range(30)], 255)
    # `end` values that differ only in their highest byte, `start` fixed: 70 000 and 2^27 + 70 000 (an operation's length has 28 bits,
    # so 2^27 is the highest single bit two introns of one start can differ in)
    c["end_high_byte"] = ([dict(tid=0, pos=59_980, cigar=[(M, 20), (N, (1 << 27) + 10_000 if i % 2 else 10_000), (M, 20)]) for i in range(70)], 255)
    c["back_to_back"] = ([dict(tid=0, pos=100, cigar=[(M, 10), (N, 5), (N, 5), (M, 10)])], 255)
    c["n_first_and_last"] = ([dict(tid=0, pos=100, cigar=[(N, 50), (M, 20)]), dict(tid=0, pos=100, cigar=[(M, 20), (N, 50)]), dict(tid=0, pos=300, cigar=[(N, 7)])], 255)
    c["n_of_length_zero"] = ([dict(tid=0, pos=100, cigar=[(M, 10), (N, 0), (M, 10)]), dict(tid=0, pos=100, cigar=[(M, 10), (N, 0), (M, 5), (N, 100), (M, 20)])], 255)
    c["d_and_i_beside_n"] = ([dict(tid=0, pos=100, cigar=[(S, 4), (M, 20), (D, 5), (N, 100), (I, 3), (M, 30), (H, 2)]),
                              dict(tid=0, pos=100, cigar=[(EQ, 12), (X, 1), (P, 2), (N, 100), (X, 9), (D, 2), (EQ, 4)])], 255)
    c["wide_300_operations"] = ([dict(tid=0, pos=50, cigar=[(M, 30)]), dict(tid=2, pos=1000, cigar=[(M, 5), (N, 10), (I, 1)] * 100), dict(tid=2, pos=1000, cigar=[(M, 5), (N, 10), (M, 5)])], 255)
    c["foreign_tids"] = ([dict(tid=0, pos=100, cigar=[(M, 20), (N, 50), (M, 20)]), dict(tid=N_CONTIGS, pos=100, cigar=[(M, 20), (N, 50), (M, 20)]),
                          dict(tid=N_CONTIGS + 4, pos=100, cigar=[(M, 20), (N, 50), (M, 20)]), dict(tid=-1, pos=100, cigar=[(M, 20), (N, 50), (M, 20)])], 255)
    c["end_beyond_int_max"] = ([dict(tid=0, pos=INT_MAX - 100, cigar=[(M, 50), (N, 100), (M, 20)]), dict(tid=0, pos=INT_MAX - 150, cigar=[(M, 50), (N, 100)]),
                                dict(tid=0, pos=INT_MAX - 400, cigar=[(M, 50), (N, 100), (M, 20), (N, 300), (M, 9)])], 255)
    c["excluding_flags"] = ([dict(tid=0, pos=100, flag=f, cigar=[(M, 20), (N, 50), (M, 20)]) for f in (0, abi.FUNMAP, abi.FSECONDARY, abi.FQCFAIL, abi.FSUPP, abi.FDUP, abi.FDUP | abi.FPAIRED | abi.FREVERSE)], 255)
    mq = [dict(tid=0, pos=100, mapq=q, cigar=[(M, 20), (N, 50), (M, 20)]) for q in (0, 3, 4, 5, 254, 255, 255)]
    c["mapq_threshold_255"] = (mq, 255)
    c["mapq_threshold_4"] = (mq, 4)
    return c


CRAFTED_NAMES = ["zero_instances", "exactly_1", "exactly_64", "exactly_65", "exactly_2048", "exactly_2049", "run_across_workgroups", "same_start_other_end",
                 "same_start_end_other_tid", "end_high_byte", "back_to_back", "n_first_and_last", "n_of_length_zero", "d_and_i_beside_n", "wide_300_operations",
                 "foreign_tids", "end_beyond_int_max", "excluding_flags", "mapq_threshold_255", "mapq_threshold_4"]


@functools.lru_cache(maxsize=None)
def crafted_case(name):
    """(batch, mapq_threshold, expected table); the expectations every reader of the contract can check by hand are asserted here."""
    recs, q = crafted()[name]
    b = Batch.from_records(recs)
    want = junction_ref.junction_table([b], N_CONTIGS, q)
    t = lambda f: [int(x) for x in want[f]]
    if name == "zero_instances":
        assert want["n"] == 0 and want["instances"] == 0 and want["population"] == 300
    if name.startswith("exactly_"):
        assert want["instances"] == int(name.split("_")[1])
    if name == "run_across_workgroups":
        assert t("reads") == [1, 5000, 1] and t("hq_reads") == [1, 4000, 1] and t("max_overhang") == [30, 20, 30]
    if name == "same_start_other_end":
        assert want["n"] == 4 and len(set(t("start"))) == 1 and t("reads") == [10] * 4
    if name == "same_start_end_other_tid":
        assert t("tid") == [0, 1, 2] and t("reads") == [10] * 3
    if name == "end_high_byte":
        assert t("end") == [70_000, (1 << 27) + 70_000] and t("start") == [60_001] * 2 and t("reads") == [35, 35]
    if name == "back_to_back":
        assert (t("start"), t("end"), t("max_overhang")) == ([111, 116], [115, 120], [0, 0])
    if name == "n_first_and_last":
        assert (t("start"), t("end"), t("max_overhang")) == ([101, 121, 301], [150, 170, 307], [0, 0, 0])
    if name == "n_of_length_zero":
        assert (t("start"), t("end"), t("reads"), t("max_overhang")) == ([116], [215], [1], [5])
    if name == "d_and_i_beside_n":
        assert (t("start"), t("end"), t("reads"), t("max_overhang")) == ([114, 126], [213, 225], [1, 1], [13, 20])
    if name == "wide_300_operations":
        assert len(b.wide_index) == 1 and want["instances"] == 101 and want["n"] == 100 and t("reads")[0] == 2 and t("max_overhang")[:2] == [5, 5] and t("max_overhang")[-1] == 0
    if name == "foreign_tids":
        assert want["population"] == 1 and want["instances"] == 1 and want["n_ops_excluded"] == 3
    if name == "end_beyond_int_max":
        assert t("end") == [INT_MAX - 250, INT_MAX] and t("max_overhang") == [20, 0] and want["population"] == 3
    if name == "excluding_flags":
        assert want["population"] == 3 and t("reads") == [3] and want["n_ops_excluded"] == 4
    if name == "mapq_threshold_255":
        assert t("reads") == [7] and t("hq_reads") == [2]
    if name == "mapq_threshold_4":
        assert t("reads") == [7] and t("hq_reads") == [5]
    return b, q, want
