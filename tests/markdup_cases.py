"""Inputs shared by the --mark-duplicates tests (CPU emulation, C ABI on the GPU, command line): the catalogue of crafted collections
and the seeded 40 000-record fixture.  Expected verdicts and figures always come from tests/markdup_ref.py; what a reader of the
contract can check by hand is asserted here."""
import copy
import functools
import json
import os

import numpy as np

from rnaseqc_amd import abi
from rnaseqc_amd.model import Batch
from tests import markdup_ref as ref

M, I, D, N, S, H, P, EQ, X = abi.CIG_M, abi.CIG_I, abi.CIG_D, abi.CIG_N, abi.CIG_S, abi.CIG_H, abi.CIG_P, abi.CIG_EQ, abi.CIG_X
PAIRED, MUNMAP, REV, MREV, R1, R2, DUP = abi.FPAIRED, abi.FMUNMAP, abi.FREVERSE, abi.FMREVERSE, abi.FREAD1, abi.FREAD2, abi.FDUP
INT_MAX, INT_MIN = (1 << 31) - 1, -(1 << 31)
CONTIGS = [("chrA", 900_000), ("chrB", 500_000), ("chrC", 300_000)]


def single(name, pos, cigar=((M, 50),), tid=0, flag=0, mapq=255, **kw):
    return dict(qname=name, tid=tid, pos=pos, cigar=list(cigar), flag=flag, mapq=mapq, **kw)


def pair(name, pos1, pos2, tid=0, length=50, mapq=255, first_is_read1=True, isize=None, extra1=0, extra2=0, cigar1=None, mapq2=None):
    """A forward/reverse pair on one contig: the record at pos1 is forward, the one at pos2 reverse.  Returns both, pos1's first."""
    size = (pos2 + length - pos1) if isize is None else isize
    a, b = (R1, R2) if first_is_read1 else (R2, R1)
    return [dict(qname=name, tid=tid, pos=pos1, mpos=pos2, isize=size, cigar=cigar1 or [(M, length)], flag=PAIRED | MREV | a | extra1, mapq=mapq),
            dict(qname=name, tid=tid, pos=pos2, mpos=pos1, isize=-size if size != INT_MIN else size, cigar=[(M, length)], flag=PAIRED | REV | b | extra2, mapq=mapq if mapq2 is None else mapq2)]


def split(name, tid1, pos1, tid2, pos2, mapq=255, extra1=0):
    """A pair with its mates on two contigs: read1 forward on tid1, read2 reverse on tid2."""
    return [dict(qname=name, tid=tid1, pos=pos1, mtid=tid2, mpos=pos2, cigar=[(M, 50)], flag=PAIRED | MREV | R1 | extra1, mapq=mapq),
            dict(qname=name, tid=tid2, pos=pos2, mtid=tid1, mpos=pos1, cigar=[(M, 50)], flag=PAIRED | REV | R2, mapq=mapq)]


def _distinct_singles(n, start=0, step=10, prefix="u"):
    return [single("%s%d" % (prefix, i), 1000 + step * (start + i)) for i in range(n)]


def _names_with_home(slot, count, mask=1023, prefix="h"):
    """`count` different names whose home slot in a table of mask + 1 slots (qhash & mask) is `slot`."""
    out, k = [], 0
    while len(out) < count:
        block = np.frombuffer(("".join("%s%07d" % (prefix, k + j) for j in range(4096))).encode(), np.uint8).reshape(4096, len(prefix) + 7)
        hit = np.flatnonzero((abi.qname_hash_bytes(block) & np.uint64(mask)) == np.uint64(slot))
        out += ["%s%07d" % (prefix, k + int(j)) for j in hit]
        k += 4096
    return out[:count]


def crafted():
    """name -> (records of one batch in arrival order, use_qhash2)"""
    c = {}
    # ---- u5
    c["u5_leading_clips"] = ([single("a", 100), single("b", 110, [(S, 10), (M, 40)]), single("c", 115, [(H, 5), (S, 10), (M, 35)]), single("d", 105, [(H, 5), (M, 45)]),
                              single("e", 100, [(S, 3), (M, 47)])], True)       # e: the same pos as a, another u5
    c["u5_reverse_trailing_clips"] = ([single("a", 100, flag=REV), single("b", 100, [(M, 40), (S, 10)], flag=REV), single("c", 100, [(M, 30), (S, 10), (H, 10)], flag=REV),
                                       single("d", 100, [(S, 10), (M, 50)], flag=REV), single("e", 110, [(M, 30), (S, 10)], flag=REV), single("f", 100, [(M, 47), (S, 9)], flag=REV)], True)
    c["u5_inner_operations"] = ([single("a", 100, [(M, 10), (D, 5), (M, 10), (N, 100), (EQ, 10), (I, 3), (P, 2), (X, 5)], flag=REV), single("b", 100, [(M, 140)], flag=REV),
                                 single("c", 100, [(M, 143)], flag=REV), single("d", 300, [(I, 4), (M, 20)]), single("e", 300, [(M, 24)]), single("f", 300, [(M, 10), (S, 4), (M, 10)])], True)
    c["u5_no_cigar"] = ([single("a", 500, []), single("b", 500, []), single("c", 500, [], flag=REV), single("d", 500, [], flag=REV), single("e", 450, [(M, 50)], flag=REV)], True)
    wide = [(S, 5)] + [(M, 1), (I, 1)] * 150 + [(S, 7)]
    c["u5_wide_300_operations"] = ([single("a", 1005, wide), single("b", 1000, [(M, 100)]), single("c", 2000, wide, flag=REV), single("d", 2057, [(M, 100)], flag=REV), single("e", 2100, [(M, 50)], flag=REV)], True)
    c["u5_wraps_at_int_max"] = ([single("a", INT_MAX - 10, [(M, 5), (S, 20)], flag=REV), single("b", INT_MAX - 10, [(M, 10), (S, 15)], flag=REV), single("c", INT_MAX - 10, [(M, 10), (S, 16)], flag=REV),
                                 single("d", 3, [(S, 10), (M, 10)]), single("e", 0, [(S, 7), (M, 10)]), single("f", 3, [(S, 9), (M, 10)])], True)
    c["u5_operation_code_above_8"] = ([single("a", 100, [(S, 5), (9, 7), (S, 3), (M, 10)]), single("b", 100, [(S, 5), (M, 10)]), single("c", 100, [(S, 8), (M, 10)]),
                                       single("d", 100, [(M, 10), (12, 4), (S, 5)], flag=REV), single("e", 100, [(M, 10), (S, 5)], flag=REV), single("f", 100, [(M, 10), (S, 5), (15, 9)], flag=REV),
                                       single("g", 100, [(M, 10)], flag=REV)], True)
    # ---- signature
    c["sig_opposite_strands"] = ([single("a", 100), single("b", 50, flag=REV), single("c", 100), single("d", 50, flag=REV)], True)
    kinds = []
    for k in range(2):
        kinds += [single("s%d" % k, 100)] + pair("p%d" % k, 100, 300) + split("x%d" % k, 0, 100, 1, 300)
    c["sig_kinds_at_the_same_coordinates"] = (kinds, True)
    recs = []
    for k, size in enumerate((250, 250, -250, -250, INT_MIN, INT_MIN, 0, 0, 251)):
        recs += pair("i%d" % k, 100, 300, isize=size)
    c["sig_pairs_differ_in_isize"] = (recs, True)
    recs = pair("a", 100, 300) + pair("b", 100, 300) + pair("c", 100, 300) + pair("d", 100, 300)
    for r in recs[4:]:
        r["flag"] &= ~(MREV | REV)                  # c and d: both mates forward
    c["sig_pairs_differ_in_mrev"] = (recs, True)
    c["sig_splits_differ_in_mpos"] = (split("a", 0, 100, 1, 300) + split("b", 0, 100, 1, 300) + split("c", 0, 100, 1, 301) + split("d", 0, 100, 2, 300), True)
    c["sig_mate_unmapped_is_single"] = ([single("a", 100), single("b", 100, flag=PAIRED | MUNMAP | R1 | MREV, mpos=100, isize=77), single("c", 100, flag=PAIRED | MUNMAP | R2, mpos=5)], True)
    # ---- anchor
    recs = pair("a", 100, 100) + pair("b", 100, 100, first_is_read1=False) + pair("c", 100, 100) + pair("d", 100, 100, first_is_read1=False)
    c["anchor_tie_is_decided_by_read1"] = (recs, True)
    bad = []
    for k in range(2):                                  # both mates say "my mate lies in front of me": no anchor
        bad += [dict(qname="m%d" % k, tid=0, pos=300, mpos=100, isize=-250, cigar=[(M, 50)], flag=PAIRED | R1 | MREV), dict(qname="m%d" % k, tid=0, pos=400, mpos=100, isize=-250, cigar=[(M, 50)], flag=PAIRED | R2 | REV)]
    bad += split("n0", 0, 100, 1, 300) + split("n1", 0, 100, 1, 300)
    for r in bad[4:]:
        r["flag"] = (r["flag"] & ~R1) | R2              # ... and split pairs without a read 1
    c["anchor_malformed_pairs_have_none"] = (bad, True)
    recs = [single("x", 100), single("dup", 100)]
    for f in (abi.FSECONDARY, abi.FSUPP, abi.FQCFAIL, abi.FUNMAP):
        recs += [single("dup", 700, flag=f), single("other", 100, flag=f), single("other2", 100, flag=f)]
    recs += [single("dup", 5, tid=-1), single("lost", 9, tid=-1), single("lost2", 9, tid=-1)]
    c["anchor_excluded_records_are_flagged_by_name"] = (recs, True)
    # ---- survivor
    c["survivor_later_higher_mapq"] = ([single("a", 100, mapq=3), single("b", 100, mapq=60), single("c", 100, mapq=59)], True)
    c["survivor_equal_mapq_keeps_the_first"] = ([single("a", 100, mapq=30), single("b", 100, mapq=30), single("c", 100, mapq=30), single("d", 100, mapq=0)], True)
    c["survivor_set_of_3"] = (pair("a", 100, 300, mapq=10) + pair("b", 100, 300, mapq=255) + pair("c", 100, 300, mapq=255), True)
    c["survivor_set_of_2049"] = ([single("m%d" % i, 100, mapq=(200 if i == 1500 else i % 7)) for i in range(2049)] + [single("z", 101)], True)
    # ---- flags on input
    c["input_flags_are_replaced"] = ([single("a", 100, flag=DUP), single("b", 100, flag=DUP), single("c", 200, flag=DUP), single("d", 300), single("e", 400, flag=DUP | abi.FSECONDARY)] +
                                     pair("f", 500, 700, extra1=DUP, extra2=DUP), True)
    # ---- name identity: the colliding names of tests/golden/qname_hash_collision.json
    fx = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "qname_hash_collision.json")))
    coll = [single("first", 100), single(fx["a"], 100), single(fx["b"], 900), single("z", 950)]
    c["names_collide_with_qhash2"] = (coll, True)
    c["names_collide_without_qhash2"] = (coll, False)
    # ---- edges of the machinery
    recs = _distinct_singles(2100)
    for k in (64, 256, 2048):                           # sorted order = arrival order here: the runs straddle anchor slots 63/64, 255/256, 2047/2048
        recs[k] = single("u%d" % k, recs[k - 1]["pos"])
    recs[65] = single("u65", recs[63]["pos"])
    c["edge_runs_across_wave_workgroup_tile"] = (recs, True)
    for n in (2047, 2048, 2049):
        recs = _distinct_singles(n)
        for k in range(6, n, 7):
            recs[k] = single("u%d" % k, recs[k - 1]["pos"], mapq=k % 5)
        recs[n - 1] = single("u%d" % (n - 1), recs[n - 2]["pos"])
        c["edge_exactly_%d_anchors" % n] = (recs + [single("sec", 100, flag=abi.FSECONDARY)], True)
    c["edge_no_duplicates"] = (_distinct_singles(300) + pair("p", 100, 300), True)
    c["edge_one_duplicate"] = (_distinct_singles(300) + [single("again", 1000)], True)
    for n in (512, 513):                                # half a table of 1024 slots, and one more: 2048 slots
        c["edge_%d_duplicates" % n] = (_distinct_singles(n) + _distinct_singles(n, prefix="v") + [single("w", 7)], True)
    chain = _names_with_home(37, 9)
    recs = [single("orig", 100)] + [single(nm, 100) for nm in chain[:5]] + [single(nm, 5000 + 10 * k) for k, nm in enumerate(chain[5:])]
    recs += [single(nm, 9000, flag=abi.FSECONDARY) for nm in chain[:7]]
    c["edge_names_share_a_home_slot"] = (recs, True)
    wrap = _names_with_home(1023, 7, prefix="w")
    recs = [single("orig", 100)] + [single(nm, 100) for nm in wrap[:4]] + [single(nm, 5000 + 10 * k) for k, nm in enumerate(wrap[4:])] + [single(_names_with_home(0, 1, prefix="y")[0], 7777)]
    c["edge_home_is_the_last_slot"] = (recs, True)
    c["edge_no_population"] = ([single("a", 100, flag=abi.FUNMAP | DUP), single("b", 100, flag=abi.FSECONDARY), single("c", 100, flag=abi.FSUPP | DUP), single("d", 100, flag=abi.FQCFAIL), single("e", 100, tid=-1), single("f", 100, tid=-1, flag=DUP)], True)
    return c


CRAFTED_NAMES = ["u5_leading_clips", "u5_reverse_trailing_clips", "u5_inner_operations", "u5_no_cigar", "u5_wide_300_operations", "u5_wraps_at_int_max", "u5_operation_code_above_8",
                 "sig_opposite_strands", "sig_kinds_at_the_same_coordinates", "sig_pairs_differ_in_isize", "sig_pairs_differ_in_mrev", "sig_splits_differ_in_mpos", "sig_mate_unmapped_is_single",
                 "anchor_tie_is_decided_by_read1", "anchor_malformed_pairs_have_none", "anchor_excluded_records_are_flagged_by_name",
                 "survivor_later_higher_mapq", "survivor_equal_mapq_keeps_the_first", "survivor_set_of_3", "survivor_set_of_2049", "input_flags_are_replaced",
                 "names_collide_with_qhash2", "names_collide_without_qhash2",
                 "edge_runs_across_wave_workgroup_tile", "edge_exactly_2047_anchors", "edge_exactly_2048_anchors", "edge_exactly_2049_anchors", "edge_no_duplicates", "edge_one_duplicate",
                 "edge_512_duplicates", "edge_513_duplicates", "edge_names_share_a_home_slot", "edge_home_is_the_last_slot", "edge_no_population"]


def without_qhash2(b):
    nb = copy.copy(b)
    nb.qhash2 = None
    return nb


@functools.lru_cache(maxsize=None)
def _crafted_cached():
    return crafted()


@functools.lru_cache(maxsize=None)
def crafted_case(name):
    """(batch, verdicts, info): the batch has no qhash2 column where the case asks for the 64-bit identity."""
    recs, two = _crafted_cached()[name]
    b = Batch.from_records(recs)
    if not two:
        b = without_qhash2(b)
    v, info, detail = ref.mark_duplicates([b], use_qhash2=two)
    flagged = [r["qname"] for r, x in zip(recs, v) if x]
    sigs = detail["signatures"]
    u5_of = lambda i: sigs[i][1]
    if name == "u5_leading_clips":
        assert [u5_of(i) for i in range(5)] == [100, 100, 100, 100, 97] and flagged == ["b", "c", "d"]
    if name == "u5_reverse_trailing_clips":
        assert [u5_of(i) for i in range(6)] == [150, 150, 150, 150, 150, 156] and flagged == ["b", "c", "d", "e"]
    if name == "u5_inner_operations":
        assert [u5_of(i) for i in range(6)] == [240, 240, 243, 300, 300, 300] and flagged == ["b", "e", "f"]
    if name == "u5_no_cigar":
        assert [u5_of(i) for i in range(5)] == [500] * 5 and flagged == ["b", "d", "e"]
    if name == "u5_wide_300_operations":
        assert len(b.wide_index) == 2 and [u5_of(i) for i in range(5)] == [1000, 1000, 2157, 2157, 2150] and flagged == ["b", "d"]
    if name == "u5_wraps_at_int_max":
        assert [u5_of(i) for i in range(6)] == [INT_MIN + 14, INT_MIN + 14, INT_MIN + 15, -7, -7, -6] and flagged == ["b", "e"]
    if name == "u5_operation_code_above_8":
        assert [u5_of(i) for i in range(7)] == [95, 95, 92, 115, 115, 110, 110] and flagged == ["b", "e", "g"]
    if name == "sig_opposite_strands":
        assert [u5_of(i) for i in range(4)] == [100] * 4 and flagged == ["c", "d"] and info["sets"] == 2
    if name == "sig_kinds_at_the_same_coordinates":
        assert info["anchors"] == 6 and info["sets"] == 3 and flagged == ["s1", "p1", "p1", "x1", "x1"]
    if name == "sig_pairs_differ_in_isize":
        assert info["anchors"] == 9 and info["sets"] == 5 and info["duplicate_fragments"] == 4 and info["flagged_records"] == 8
    if name == "sig_pairs_differ_in_mrev":
        assert info["sets"] == 2 and sorted(set(flagged)) == ["b", "d"]
    if name == "sig_splits_differ_in_mpos":
        assert info["anchors"] == 4 and info["sets"] == 2 and sorted(set(flagged)) == ["b", "d"]      # d: the mate's contig is not in the signature
    if name == "sig_mate_unmapped_is_single":
        assert info["anchors"] == 3 and info["sets"] == 1 and flagged == ["b", "c"]
    if name == "anchor_tie_is_decided_by_read1":
        # a, c: read 1 is the forward record; b, d: read 1 is the reverse one.  Two sets of two
        assert info["anchors"] == 4 and info["sets"] == 2 and sorted(set(flagged)) == ["c", "d"]
    if name == "anchor_malformed_pairs_have_none":
        assert info["population"] == 8 and info["anchors"] == 0 and not flagged
    if name == "anchor_excluded_records_are_flagged_by_name":
        assert info["anchors"] == 2 and flagged == ["dup"] * 6 and info["population"] == 2
    if name == "survivor_later_higher_mapq":
        assert flagged == ["a", "c"]
    if name == "survivor_equal_mapq_keeps_the_first":
        assert flagged == ["b", "c", "d"]
    if name == "survivor_set_of_3":
        assert sorted(set(flagged)) == ["a", "c"] and info["flagged_records"] == 4
    if name == "survivor_set_of_2049":
        assert info["sets"] == 2 and info["duplicate_fragments"] == 2048 and "m1500" not in flagged and "m0" in flagged
    if name == "input_flags_are_replaced":
        assert flagged == ["b"] and info["cleared_records"] == 5
    if name == "names_collide_with_qhash2":
        assert len(flagged) == 1 and info["duplicate_fragments"] == 1
    if name == "names_collide_without_qhash2":
        assert len(flagged) == 2 and info["duplicate_fragments"] == 1
    if name == "edge_runs_across_wave_workgroup_tile":
        assert flagged == ["u64", "u65", "u256", "u2048"]
    if name.startswith("edge_exactly_"):
        assert info["anchors"] == int(name.split("_")[2]) and info["duplicate_fragments"] > 290
    if name == "edge_no_duplicates":
        assert info["duplicate_fragments"] == 0 and info["anchors"] == 301
    if name == "edge_one_duplicate":
        assert flagged == ["again"]
    if name in ("edge_512_duplicates", "edge_513_duplicates"):
        assert info["duplicate_fragments"] == int(name.split("_")[1])
    if name == "edge_names_share_a_home_slot":
        assert info["duplicate_fragments"] == 5 and info["flagged_records"] == 10
    if name == "edge_home_is_the_last_slot":
        assert info["duplicate_fragments"] == 4 and info["flagged_records"] == 4
    if name == "edge_no_population":
        assert info["population"] == 0 and info["anchors"] == 0 and info["cleared_records"] == 3
    return b, v, info


# ---- the seeded fixture: 40 000 records in no order, about 30 % duplicate fragments -------------------------------------------------
FIXTURE_CUTS = [0, 3000, 11000, 12500, 31000, 40000]
_MAPQS = np.array([0, 3, 60, 255])


@functools.lru_cache(maxsize=None)
def fixture():
    """14 000 pairs, 2 000 split pairs, 6 000 single reads and 2 000 secondary / supplementary / unmapped records that carry the names
    of other fragments, shuffled; some records arrive with 0x400 set.  30 % of the fragments copy the coordinates of an earlier one
    (sometimes with another clipping of the anchor and the same u5), under a new name and with another mapq."""
    r = np.random.default_rng(20260)
    recs = []

    def template(kind):
        t = dict(kind=kind, tid=int(r.integers(0, 3)), pos=int(r.integers(1000, 250_000)), d=int(r.integers(0, 400)) if r.random() > 0.05 else 0,
                 r1_first=bool(r.integers(0, 2)), ff=r.random() < 0.1, rev=bool(r.integers(0, 2)), tid2=0, pos2=int(r.integers(1000, 250_000)),
                 intron=int(r.integers(1, 40)) * 50 if r.random() < 0.2 else 0)
        t["tid2"] = (t["tid"] + 1 + int(r.integers(0, 2))) % 3
        return t

    def emit(t, name):
        mapq = int(_MAPQS[r.integers(0, 4)])
        clip = int(r.integers(1, 12)) if r.random() < 0.3 else 0
        lead = [(S, clip), (M, 100 - clip)] if clip else [(M, 100)]
        if t["kind"] == ref.SINGLE:
            gap = [(N, t["intron"])] if t["intron"] else []         # (a fifth of the single reads are spliced: the junction table is not empty)
            if t["rev"]:
                return [single(name, t["pos"], [(M, 50)] + gap + [(M, 50 - clip)] + ([(S, clip)] if clip else []), tid=t["tid"], flag=REV, mapq=mapq)]
            return [single(name, t["pos"] + clip, ([(S, clip)] if clip else []) + [(M, 50 - clip)] + gap + [(M, 50)], tid=t["tid"], mapq=mapq)]
        if t["kind"] == ref.PAIR:
            two = pair(name, t["pos"] + clip, t["pos"] + t["d"], tid=t["tid"], length=100, mapq=mapq, first_is_read1=t["r1_first"], mapq2=int(_MAPQS[r.integers(0, 4)]),
                       cigar1=lead, isize=t["d"] + 100)
            if t["ff"]:
                two[0]["flag"] &= ~MREV; two[1]["flag"] &= ~REV
            return two
        return split(name, t["tid"], t["pos"], t["tid2"], t["pos2"], mapq=mapq)

    n_frag = 0
    for kind, count in ((ref.PAIR, 14000), (ref.SPLIT, 2000), (ref.SINGLE, 6000)):
        originals = []
        for _ in range(count):
            if originals and r.random() < 0.3:
                t = originals[int(r.integers(0, len(originals)))]
            else:
                t = template(kind); originals.append(t)
            recs += emit(t, "f%06d" % n_frag)
            n_frag += 1
    for k in range(2000):
        src = recs[int(r.integers(0, 38000))]
        recs.append(single(src["qname"], int(r.integers(1000, 250_000)), tid=int(r.integers(0, 3)), flag=(abi.FSECONDARY, abi.FSUPP, abi.FUNMAP, abi.FQCFAIL | PAIRED)[k % 4], mapq=0))
    for k in r.choice(len(recs), 2000, replace=False):
        recs[int(k)]["flag"] |= DUP
    order = r.permutation(len(recs))
    return Batch.from_records([recs[int(k)] for k in order])


@functools.lru_cache(maxsize=None)
def fixture_expected():
    return ref.mark_duplicates([fixture()])


def cut(batch, cuts=None, seed=None, parts=3):
    if cuts is None:
        cuts = [0] + sorted(int(x) for x in np.random.default_rng(seed).choice(np.arange(1, batch.n), parts - 1, replace=False)) + [batch.n]
    assert cuts[0] == 0 and cuts[-1] == batch.n
    return [batch.slice(lo, hi) for lo, hi in zip(cuts[:-1], cuts[1:])]


@functools.lru_cache(maxsize=None)
def fixture_shuffled():
    """The fixture in another arrival order, in three unequal batches, with what the reference says for THAT order."""
    b = fixture()
    parts = cut(b.take(np.random.default_rng(77).permutation(b.n)), seed=78, parts=3)
    return parts, ref.mark_duplicates(parts)
