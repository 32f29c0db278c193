"""Inputs shared by the --fasta edge tests (CPU emulation: tests/test_gc_host.py; device: tests/test_gpu_gc_edges.py): a named catalogue
of small references, annotations and records aimed at the edge handling of the GC kernels -- word-boundary masks, clipping at the contig
end, rejected ranges, the contig search, the case fold, bin edges of the sequential sum, the pairing state machine and its three paths.
Every case asserts the expectation a reader can check by hand; whole-path expectations otherwise come from the oracle, candidate-level
ones from tests/gc_ref.py."""
import functools

import numpy as np

from rnaseqc_amd import abi
from rnaseqc_amd.model import Annotation, Batch, Reference
from tests import gc_ref

M, N = abi.CIG_M, abi.CIG_N
K = 0x9E3779B97F4A7C15                      # the multiplier of the pairing set's mix (rsqc_k5.h, pair_bucket_hashed)
MASK64 = (1 << 64) - 1


def seq_of(text):
    return np.frombuffer(text if isinstance(text, bytes) else text.encode(), np.uint8).copy()


def irregular(n, salt=0):
    """A fixed base string without a period that divides 64: G g C c at irregular places between A T N a t."""
    alphabet = b"ACGTgcNatGCAcTg"
    return seq_of(bytes(alphabet[((i * i + 3 * i + salt) * 7 + (i >> 3)) % len(alphabet)] for i in range(n)))


def gene_rows(contig, gid, exons, strand="+"):
    """One gene spanning its exons [(start, end), ...] (1-based closed, GTF)."""
    lo, hi = min(s for s, _ in exons), max(e for _, e in exons)
    rows = [dict(contig=contig, type="gene", start=lo, end=hi, strand=strand, gene_id=gid, gene_name=gid, transcript_type="protein_coding")]
    for k, (s, e) in enumerate(exons):
        rows.append(dict(contig=contig, type="exon", start=s, end=e, strand=strand, gene_id=gid, exon_id="%s_e%d" % (gid, k), gene_name=gid,
                         transcript_type="protein_coding"))
    return rows


def rec(q, tid, pos, ln, first, mpos, isize=300, cigar=None):
    """A mate of a proper pair: `first` = the forward mate (flag 99), else the reverse one (147).  One block of `ln` bases unless a CIGAR is given."""
    return dict(qname=q, tid=tid, pos=pos, cigar=cigar or [(M, ln)], flag=99 if first else 147, mapq=255, nm=0, mpos=mpos, mtid=tid,
                isize=isize if first else -isize)


def pair(q, tid, pos1, ln1, pos2, ln2, isize=300):
    """Two records: the first ends at pos1 + ln1, the second at pos2 + ln2; a fragment covers [pos1 + ln1 - ln2, pos2 + ln2)."""
    return [rec(q, tid, pos1, ln1, True, pos2, isize), rec(q, tid, pos2, ln2, False, pos1, isize)]


def by_position(recs):
    """File order of a coordinate-sorted file (stable)."""
    return sorted(recs, key=lambda r: (r["tid"], r["pos"]))


class Case:
    """ann, ref; whole-path cases: batch (+ params); candidate-level cases: candidates (columns of tests/hostemu/gc.CAND_COLUMNS, emission
    order) with expect["cands"] (the same candidates as dicts, for gc_ref.replay).  expect: what the case states by hand."""
    def __init__(self, name, ann, ref, batch=None, params=None, candidates=None, expect=None):
        self.name, self.ann, self.ref, self.batch, self.candidates = name, ann, ref, batch, candidates
        self.params = params if params is not None else abi.default_params(coverage_mask=0)
        self.expect = expect or {}


# ---- bit ranges ----------------------------------------------------------------------------------------------------------------------
def _bit_ranges():
    """963 single-exon genes on one contig of 300 bases: every start & 63, the last base on bits 0, 1, 31, 32, 62, 63 of the start's
    word, of the next and of the one after.  A second contig carries one ordinary gene and a pair, so that a pass has records."""
    seq = irregular(300)
    rows, n = [], 0
    for start in range(1, 65):                                   # start & 63 = 1 .. 63, 0 (GTF coordinates begin at 1)
        for d in (0, 1, 2):
            for bit in (0, 1, 31, 32, 62, 63):
                last = ((start >> 6) + d) * 64 + bit             # 0-based offset of the last base: the exon covers [start, last]
                if last < start:
                    continue
                rows += gene_rows("c", "b%d" % n, [(start, last)]); n += 1
    assert n == 963                                              # 64 x 18 less the 189 ends in front of their start
    rows += gene_rows("d", "plain", [(1, 250)])
    ann = Annotation.from_rows(["c", "d"], rows)
    ref = Reference(contig=[0, 1], sequence=[seq, irregular(260, salt=5)])
    batch = Batch.from_records(pair("p", 1, 20, 30, 120, 30))
    want = gc_ref.exon_gc(ann, ref)
    assert (want >= 0).all() and len(set(want.tolist())) > 100   # every exon lies inside the contig; the pattern tells the ranges apart
    return Case("bit_ranges", ann, ref, batch, expect=dict(n_candidates=2, fragments=1))


# ---- contig lengths ------------------------------------------------------------------------------------------------------------------
CONTIG_LENGTH_NAMES = ["front", "long", "absent", "L1", "L63", "L64", "gap", "L65", "L127", "L128", "L129", "L0"]


def _contig_lengths():
    """FASTA order: a long all-G contig, then lengths 1, 63, 64, 65, 127, 128, 129 and 0, then the two contigs without exons.  The staging
    buffer still holds the long contig's G behind every shorter one; a wrong word_off moves a contig onto its neighbour's bits (each has
    its own period).  Annotation order: `front` (no exons) before all, `absent` (third, exons, not in the FASTA), `gap` (no exons)
    between L64 and L65."""
    names = CONTIG_LENGTH_NAMES
    length = dict(front=70, long=200, L1=1, L63=63, L64=64, gap=40, L65=65, L127=127, L128=128, L129=129, L0=0)
    seqs = {}
    for k, nm in enumerate(names):
        if nm == "absent":
            continue
        L = length[nm]
        seqs[nm] = seq_of(b"G" * L) if nm == "long" else seq_of(bytes(b"GA"[0 if i % (k + 2) == 0 else 1] for i in range(L)))
    rows = gene_rows("long", "gl", [(10, 150)]) + gene_rows("long", "gl2", [(160, 260)]) + gene_rows("absent", "ga", [(5, 50)])
    rows += gene_rows("L1", "g1", [(1, 5)]) + gene_rows("L0", "g0", [(1, 10)])
    for nm in ("L63", "L64", "L65", "L127", "L128", "L129"):
        L = length[nm]
        rows += gene_rows(nm, "g%s" % nm, [(1, L - 1)]) + gene_rows(nm, "h%s" % nm, [(1, L)]) + gene_rows(nm, "i%s" % nm, [(L - 1, L + 3)]) + \
                gene_rows(nm, "j%s" % nm, [(L, L)])
    ann = Annotation.from_rows(names, rows)
    order = ["long", "L1", "L63", "L64", "L65", "L127", "L128", "L129", "L0", "front", "gap"]
    ref = Reference(contig=[names.index(nm) for nm in order], sequence=[seqs[nm] for nm in order])
    batch = Batch.from_records(by_position(pair("p", 1, 19, 30, 60, 30) + pair("z", 2, 5, 20, 25, 20)))     # `z`: on the absent contig
    want = gc_ref.exon_gc(ann, ref)
    e = lambda eid: want[ann.exon_ids.index(eid)]
    assert e("gl_e0") == gc_ref.gc_of(141, 141) and e("gl2_e0") == gc_ref.gc_of(40, 40)         # [160, 261) clipped at 200
    assert e("ga_e0") == -1.0 and e("g1_e0") == -1.0 and e("g0_e0") == -1.0                     # absent; start 1 >= L 1; L 0
    for nm in ("L63", "L64", "L65", "L127", "L128", "L129"):
        L, period = length[nm], names.index(nm) + 2
        g = lambda lo, hi: sum(1 for i in range(lo, hi) if i % period == 0)
        assert e("g%s_e0" % nm) == gc_ref.gc_of(g(1, L), L - 1)                                 # [1, L): ends at the contig end
        assert e("h%s_e0" % nm) == gc_ref.gc_of(g(1, L), L - 1)                                 # [1, L + 1) clipped: the same bases
        assert e("i%s_e0" % nm) == gc_ref.gc_of(g(L - 1, L), 1)                                 # the last base alone
        assert e("j%s_e0" % nm) == -1.0                                                         # start L
    return Case("contig_lengths", ann, ref, batch, expect=dict(n_candidates=2, fragments=1))


def packed_words(ref, n_contigs):
    """The bit array, word_off and length that rsqc_set_reference documents, restated: every contig on a word of its own, FASTA order."""
    off = np.full(n_contigs, MASK64, np.uint64); length = np.zeros(n_contigs, np.uint64)
    words = []
    for k, s in zip(ref.contig, ref.sequence):
        off[k] = len(words); length[k] = len(s)
        s = bytes(np.asarray(s, np.uint8))
        for w in range((len(s) + 63) // 64):
            words.append(sum(1 << i for i, ch in enumerate(s[64 * w:64 * w + 64]) if ch in b"GgCc"))
    return np.array(words, np.uint64), off, length


# ---- alphabet ------------------------------------------------------------------------------------------------------------------------
def _alphabet():
    """All 256 byte values, twice: only G g C c count (S s N, the line feed and 0x00 do not)."""
    seq = seq_of(bytes(range(256)) * 2)
    singles = {"G": 71, "g": 103, "C": 67, "c": 99, "S": 83, "s": 115, "N": 78, "lf": 10, "nul": 256, "E": 69, "W": 87}       # name -> offset of the byte
    rows = gene_rows("a", "whole", [(1, 500)])
    for nm, at in singles.items():
        assert seq[at] == dict(lf=10, nul=0).get(nm, ord(nm[0]))
        rows += gene_rows("a", "s_" + nm, [(at, at)])
    ann = Annotation.from_rows(["a"], rows)
    ref = Reference(contig=[0], sequence=[seq])
    batch = Batch.from_records(pair("p", 0, 4, 30, 200, 30))                                   # [4, 230): the four of the first copy
    want = gc_ref.exon_gc(ann, ref)
    for nm, at in singles.items():
        assert want[ann.exon_ids.index("s_%s_e0" % nm)] == (1.0 if nm in "GgCc" else 0.0)
    assert want[ann.exon_ids.index("whole_e0")] == gc_ref.gc_of(8, 500)
    words, _, _ = packed_words(ref, 1)
    assert [int(w) for w in words] == [0, (1 << 3) | (1 << 7) | (1 << 35) | (1 << 39), 0, 0] * 2
    bins = {gc_ref.bin_of(gc_ref.gc_of(4, 226)): 1}
    return Case("alphabet", ann, ref, batch, expect=dict(n_candidates=2, fragments=1, bins=bins))


# ---- exons against the contig end ----------------------------------------------------------------------------------------------------
def _exon_ends():
    L = 150
    seq = irregular(L, salt=2)
    rows = gene_rows("c", "inside", [(10, 120)]) + gene_rows("c", "at_Lm1", [(L - 1, L + 3)]) + gene_rows("c", "at_L", [(L, L + 9)]) + \
           gene_rows("c", "at_Lp5", [(L + 5, L + 20)]) + gene_rows("c", "ends_L", [(100, L - 1)]) + gene_rows("c", "ends_Lp1", [(100, L)]) + \
           gene_rows("next", "n", [(1, 60)])
    ann = Annotation.from_rows(["c", "next"], rows)
    ref = Reference(contig=[0, 1], sequence=[seq, seq_of(b"G" * 64)])                          # (bases behind the contig that WOULD count)
    batch = Batch.from_records(pair("p", 0, 20, 30, 70, 30))
    want = gc_ref.exon_gc(ann, ref)
    e = lambda eid: want[ann.exon_ids.index(eid + "_e0")]
    gc = lambda lo, hi: gc_ref.gc_fraction(bytes(seq[lo:hi]))
    assert e("at_Lm1") == gc(L - 1, L) and e("at_L") == -1.0 and e("at_Lp5") == -1.0
    assert e("ends_L") == gc(100, L) == e("ends_Lp1")                                          # 50 bases both: the size is the clipped length
    assert e("ends_L") != gc_ref.gc_of(sum(1 for ch in bytes(seq[100:L]) if ch in b"GgCc"), 51)
    return Case("exon_ends", ann, ref, batch, expect=dict(n_candidates=2, fragments=1))


# ---- fragments against the contig ends -----------------------------------------------------------------------------------------------
def _fragment_ends():
    """L = 400: G on [0, 15) and [385, 400), A elsewhere; one exon (1, 500) that reaches past the contig end.
    neg: stored end 22, second mate of 50 bases -> start -28: no fragment.           zero: stored end 30, 30 bases -> [0, 150): 15 of 150.
    past: stored end 320, second ends at 420 -> [280, 400): 15 of 120 (unclipped 15 of 140).   at_L: second ends at 400 -> [310, 400): 15 of 90.
    beyond: both mates behind the contig end, start 410 >= L: no fragment.            equal: second ends where the first did: no fragment."""
    L = 400
    seq = seq_of(b"G" * 15 + b"A" * 370 + b"G" * 15)
    ann = Annotation.from_rows(["c", "next"], gene_rows("c", "g", [(1, 500)]) + gene_rows("next", "n", [(1, 60)]))
    ref = Reference(contig=[0, 1], sequence=[seq, seq_of(b"A" * 64)])
    recs = pair("neg", 0, 2, 20, 100, 50) + pair("zero", 0, 10, 20, 120, 30) + pair("past", 0, 300, 20, 380, 40) + pair("at_L", 0, 330, 20, 360, 40) + \
           pair("beyond", 0, 410, 20, 440, 20) + pair("equal", 0, 200, 40, 210, 30)
    batch = Batch.from_records(by_position(recs))
    b = lambda k, size: gc_ref.bin_of(gc_ref.gc_of(k, size))
    bins = {}
    for k, size in ((15, 150), (15, 120), (15, 90)):
        bins[b(k, size)] = bins.get(b(k, size), 0) + 1
    assert (b(15, 150), b(15, 120), b(15, 90)) == (10, 12, 16) and b(15, 140) == 10            # 10: what an unclipped range would give
    return Case("fragment_ends", ann, ref, batch, expect=dict(n_candidates=12, fragments=3, bins=bins, hashed=1, sorted=0))


# ---- bin edges -----------------------------------------------------------------------------------------------------------------------
BIN_EDGE_PAIRS = [(26, 104), (78, 104), (21, 105), (84, 105), (53, 106)]        # the k-fold sum lands one bin below (100 k) // size
BIN_EDGE_FULL = [102, 104, 107]                                                 # 100 % GC: bin 99, bin 99, out of range


def _bin_edges():
    """G on [0, 1200), A behind: a fragment [1200 - k, 1200 - k + size) has exactly k G/C bases of size (two mates of 30 bases)."""
    seq = seq_of(b"G" * 1200 + b"A" * 1200)
    ann = Annotation.from_rows(["c"], gene_rows("c", "g", [(1, 2399)]))
    ref = Reference(contig=[0], sequence=[seq])
    recs, bins, oob = [], {}, 0
    for n, (k, size) in enumerate(BIN_EDGE_PAIRS):
        s0 = 1200 - k
        recs += pair("e%d" % n, 0, s0, 30, s0 + size - 30, 30, isize=150 + n)     # (isize only gates candidacy)
        b = gc_ref.bin_of(gc_ref.gc_of(k, size))
        assert b != (100 * k) // size and b == (100 * k) // size - 1
        bins[b] = bins.get(b, 0) + 1
    for n, size in enumerate(BIN_EDGE_FULL):
        s0 = 100 + 150 * n
        recs += pair("f%d" % n, 0, s0, 30, s0 + size - 30, 30, isize=999 - n)
        b = gc_ref.bin_of(gc_ref.gc_of(size, size))
        assert b == (99 if size in (102, 104) else gc_ref.GC_BINS)
        if b < gc_ref.GC_BINS:
            bins[b] = bins.get(b, 0) + 1
        else:
            oob += 1
    assert bins == {24: 1, 74: 1, 19: 1, 79: 1, 49: 1, 99: 2} and oob == 1
    return Case("bin_edges", ann, ref, Batch.from_records(by_position(recs)), expect=dict(n_candidates=16, fragments=8, bins=bins, out_of_range=oob, hashed=1, sorted=0))


# ---- the state machine ---------------------------------------------------------------------------------------------------------------
def _state_machine(legacy=False):
    """One exon (1, 3000) over A with G on [1000, 1100); two overlapping exons of other genes behind it.
    i100 / i1000: |isize| outside the open window (100, 1000): no candidates.    i101 / i999: inside: a fragment each ([200, 330), [400, 530): no G).
    same: pos == mpos on both mates: two candidates, no fragment.
    third: second record ends before the stored end 1550 (the entry stays), the third (40 bases) completes: [1510, 1600), no G.
    equal: second ends exactly at the stored end: no fragment.
    back: four records of one name, two fragments: [1000, 1080), 80 of 80; the name returns, [1040, 1150), 60 of 110.
    two_rows: both mates under two exon rows: no candidates.     split: two blocks: no candidates."""
    seq = seq_of(b"A" * 1000 + b"G" * 100 + b"A" * 2500)
    rows = gene_rows("c", "g", [(1, 3000)]) + gene_rows("c", "o1", [(3100, 3400)]) + gene_rows("c", "o2", [(3200, 3500)])
    ann = Annotation.from_rows(["c"], rows)
    ref = Reference(contig=[0], sequence=[seq])
    recs = pair("i100", 0, 100, 30, 180, 30, isize=100) + pair("i101", 0, 200, 30, 300, 30, isize=101) + pair("i999", 0, 400, 30, 500, 30, isize=999) + \
           pair("i1000", 0, 600, 30, 700, 30, isize=1000)
    recs += [rec("same", 0, 800, 30, True, 800), rec("same", 0, 800, 40, False, 800)]
    recs += [rec("third", 0, 1500, 50, True, 1560), rec("third", 0, 1510, 30, False, 1500), rec("third", 0, 1560, 40, False, 1500)]
    recs += pair("equal", 0, 1700, 40, 1710, 30)
    recs += pair("back", 0, 1010, 20, 1050, 30) + pair("back", 0, 1060, 20, 1110, 40)
    recs += pair("two_rows", 0, 3210, 30, 3300, 30)
    recs += [rec("split", 0, 2000, 0, True, 2200, cigar=[(M, 20), (N, 50), (M, 20)]), rec("split", 0, 2200, 0, False, 2000, cigar=[(M, 20), (N, 50), (M, 20)])]
    batch = Batch.from_records(by_position(recs))
    b = lambda k, size: gc_ref.bin_of(gc_ref.gc_of(k, size))
    bins = {0: 3, b(80, 80): 1, b(60, 110): 1}
    assert b(80, 80) == 99 and b(60, 110) == 54
    if legacy:
        return Case("state_machine_legacy", ann, ref, batch, params=abi.default_params(coverage_mask=0, legacy=1), expect=dict(n_candidates=0, fragments=0, bins={}))
    # candidates: i101 2, i999 2, same 2, third 3, equal 2, back 4; the bucket holds a name of three records and one of four: it is sorted
    return Case("state_machine", ann, ref, batch, expect=dict(n_candidates=15, fragments=5, bins=bins, hashed=0, sorted=1))


WHOLE_PATH = ["bit_ranges", "contig_lengths", "alphabet", "exon_ends", "fragment_ends", "bin_edges", "state_machine", "state_machine_legacy"]


# ---- pairing paths, candidate level ---------------------------------------------------------------------------------------------------
def _pairing_reference():
    """Two exon rows on one contig of 2 000 bases; candidates name rows 0 and 1 directly."""
    ann = Annotation.from_rows(["c"], gene_rows("c", "g", [(1, 900), (1001, 1990)]))
    return ann, Reference(contig=[0], sequence=[irregular(2000, salt=9)])


def _columns(cands):
    """cands: dicts with q, h2, file, row, endpos, l_qseq, moved -> (the columns in a shuffled emission order, names in that order)."""
    order = np.random.default_rng(len(cands)).permutation(len(cands))
    cs = [cands[i] for i in order]
    cols = dict(file_index=[c["file"] for c in cs], qhash=[c["q"] for c in cs], h2=[c["h2"] for c in cs], row=[c["row"] for c in cs],
                endpos=[c["endpos"] for c in cs], flag_lq=[c["l_qseq"] | (0x80000000 if c["moved"] else 0) for c in cs], tid=[0] * len(cs))
    return cols, cs


def replay_expectation(case):
    """gc_ref.replay over the case's candidates in FILE order, a name = (64-bit hash, second hash)."""
    cs = sorted(case.expect["cands"], key=lambda c: c["file"])
    return gc_ref.replay([dict(name=(c["q"], c["h2"]), row=c["row"], endpos=c["endpos"], l_qseq=c["l_qseq"], moved=c["moved"], tid=0) for c in cs], case.ref)


def _random_candidate(r, q, h2):
    # ends around both contig ends, lengths up to 200: starts below 0 and ends beyond L = 2000 occur
    return dict(q=q, h2=h2, file=0, row=int(r.integers(0, 2)) if r.integers(0, 6) == 0 else 0, endpos=int(r.integers(20, 2100)),
                l_qseq=int(r.integers(20, 200)), moved=bool(r.integers(0, 5)))


def _number_files(r, cands):
    """File order = a shuffle; indices unique and sparse."""
    at = 1000
    for i in r.permutation(len(cands)):
        at += 1 + int(r.integers(0, 3))
        cands[int(i)]["file"] = at
    return cands


def _pairing_collisions():
    """760 names of one or two candidates -> three buckets, all paired through the set; then 40 more names, each crafted to share the 64-bit mix
    q ^ h2 K (and the bucket) of an earlier name with another second hash: the set must hand those buckets to the sort."""
    ann, ref = _pairing_reference()
    r = np.random.default_rng(2024)
    cands, names = [], []
    for i in range(760):                                         # 1 160 candidates: three buckets of about 387, below the set's limit of 512
        q, h2 = int(r.integers(0, 1 << 63)) * 2 + int(r.integers(0, 2)), int(r.integers(0, 1 << 32))
        names.append((q, h2))
        cands += [_random_candidate(r, q, h2) for _ in range(2 if i < 400 else 1)]
    plain = Case("pairing_plain", ann, ref, candidates=True, expect=dict(cands=_number_files(r, [dict(c) for c in cands]), hashed=3, sorted=0, oversize=0))
    for k in range(40):
        q, h2 = names[int(r.integers(0, len(names)))]
        while True:                                              # h2' with (h2 K) ^ (h2' K) below 2^50: the buckets are cut on the high bits of q
            tries = r.integers(0, 1 << 32, 1 << 16).astype(np.uint64)
            d = (tries * np.uint64(K)) ^ np.uint64((h2 * K) & MASK64)
            hit = np.flatnonzero(((d >> np.uint64(50)) == 0) & (tries != np.uint64(h2)))
            if len(hit):
                h2b, q2 = int(tries[hit[0]]), q ^ int(d[hit[0]])
                break
        assert (q2 ^ (h2b * K)) & MASK64 == (q ^ (h2 * K)) & MASK64 and (q2, h2b) != (q, h2) and q2 >> 50 == q >> 50
        cands += [_random_candidate(r, q2, h2b) for _ in range(1 + int(r.integers(0, 2)))]
    crafted = Case("pairing_collisions", ann, ref, candidates=True, expect=dict(cands=_number_files(r, cands), sorted_min=1))
    return plain, crafted


def _pairing_oversize():
    """One name with 3 000 records (more than the 2 048 slots of the LDS sort) among 300 ordinary names: its bucket is listed as oversize."""
    ann, ref = _pairing_reference()
    r = np.random.default_rng(77)
    cands = []
    for _ in range(300):
        q, h2 = int(r.integers(0, 1 << 63)) * 2 + 1, int(r.integers(0, 1 << 32))
        cands += [_random_candidate(r, q, h2) for _ in range(1 + int(r.integers(0, 2)))]
    q, h2 = int(r.integers(0, 1 << 63)) * 2, int(r.integers(0, 1 << 32))
    for _ in range(3000):                                        # few distinct ends: a record often ends exactly where the stored one did; some behind L
        c = _random_candidate(r, q, h2)
        c["endpos"] = (1990, 2010, 2040)[int(r.integers(0, 3))] if r.integers(0, 10) == 0 else 300 + 25 * int(r.integers(0, 40))
        cands.append(c)
    return Case("pairing_oversize", ann, ref, candidates=True, expect=dict(cands=_number_files(r, cands), oversize=1))


def _pairing_sorted_small():
    """One bucket that must be sorted (a name of three records), holding: the name (~0, 0xFFFFFFFF) -- the LDS sort's padding key -- with a
    usable pair; `clip`, three records whose third ends behind the contig end: [1850, 2000); `rows`, row 0 stored, a record on row 1
    (nothing happens), then a later record on row 0 completes: [1200, 1500) -- a sequence a coordinate-sorted file cannot produce, so only
    this mode reaches it; `neg`: start below 0."""
    ann, ref = _pairing_reference()
    c = lambda q, h2, file, row, endpos, lq, moved=True: dict(q=q, h2=h2, file=file, row=row, endpos=endpos, l_qseq=lq, moved=moved)
    cands = [c(MASK64, 0xFFFFFFFF, 10, 0, 500, 100), c(MASK64, 0xFFFFFFFF, 20, 0, 640, 100),            # [400, 640)
             c(5, 1, 11, 1, 1900, 60), c(5, 1, 12, 1, 1890, 60), c(5, 1, 13, 1, 2030, 50),              # clip: [1850, 2000)
             c(6, 2, 14, 0, 1300, 80), c(6, 2, 15, 1, 1400, 80), c(6, 2, 16, 0, 1500, 100),             # rows: [1200, 1500)
             c(7, 3, 17, 0, 40, 30), c(7, 3, 18, 0, 90, 60),                                            # neg: 40 - 60 < 0
             c(8, 4, 19, 0, 700, 50), c(8, 4, 21, 0, 700, 50)]                                          # equal ends: nothing
    seq = bytes(ref.sequence[0])
    bins = {}
    for lo, hi in ((400, 640), (1850, 2000), (1200, 1500)):
        b = gc_ref.bin_of(gc_ref.gc_fraction(seq[lo:hi]))
        bins[b] = bins.get(b, 0) + 1
    return Case("pairing_sorted_small", ann, ref, candidates=True, expect=dict(cands=cands, hashed=0, sorted=1, oversize=0, bins=bins, fragments=3))


def _pairing_buckets(name, fills, seed):
    """Names of two candidates (one of one where a fill is odd) steered into buckets by the high words of their hashes (tests/k5_cases.py
    restates the bucket rule): fills = {bucket: candidates}.  gc_replay_kernel and gc_replay_big_kernel are copies of the fragment-size
    replay over the same pairing helpers; these are the fills at which those helpers change path."""
    from tests import k5_cases
    ann, ref = _pairing_reference()
    r = np.random.default_rng(seed)
    n = sum(fills.values())
    nb = k5_cases.n_buckets(n)
    cands = []
    for b, m in fills.items():
        qs = k5_cases.names_in_bucket(r, nb, b, (m + 1) // 2)
        for k, q in enumerate(int(x) for x in qs):
            h2 = int(r.integers(0, 1 << 32))
            cands += [_random_candidate(r, q, h2) for _ in range(2 if 2 * k + 1 < m else 1)]
    assert len(cands) == n
    hashed = sum(1 for m in fills.values() if m <= 512)
    return Case(name, ann, ref, candidates=True, expect=dict(cands=_number_files(r, cands), buckets=nb, hashed=hashed, sorted=len(fills) - hashed,
                                                             oversize=sum(1 for m in fills.values() if m > 2048)))


def _pairing_edges():
    """512 / 513: the set at its limit and one beyond (the sort); 2 048 / 2 049: the LDS sort without a padding slot and one beyond (listed);
    two listed buckets that are neighbours (their sorts lie side by side in big_idx); 65 listed buckets: one more than gc_replay_big_kernel
    has workgroups."""
    many = {b: 2049 for b in list(range(0, 320, 5)) + [346]}
    many[171] = 347 * 384 - 65 * 2049
    return [_pairing_buckets("pairing_buckets_of_512_and_513", {0: 512, 1: 513, 2: 127}, 512),
            _pairing_buckets("pairing_buckets_of_2048_and_2049", {2: 2048, 7: 2049, 10: 127}, 2048),
            _pairing_buckets("pairing_two_neighbouring_listed_buckets", {4: 2049, 5: 2049, 9: 126}, 4098),
            _pairing_buckets("pairing_65_listed_buckets", many, 65)]


PAIRING_EDGES = ["pairing_buckets_of_512_and_513", "pairing_buckets_of_2048_and_2049", "pairing_two_neighbouring_listed_buckets", "pairing_65_listed_buckets"]
CANDIDATE_LEVEL = ["pairing_plain", "pairing_collisions", "pairing_oversize", "pairing_sorted_small"] + PAIRING_EDGES


@functools.lru_cache(maxsize=None)
def _all():
    out = {}
    for c in (_bit_ranges(), _contig_lengths(), _alphabet(), _exon_ends(), _fragment_ends(), _bin_edges(), _state_machine(), _state_machine(legacy=True),
              *_pairing_collisions(), _pairing_oversize(), _pairing_sorted_small(), *_pairing_edges()):
        out[c.name] = c
    assert sorted(out) == sorted(WHOLE_PATH + CANDIDATE_LEVEL)
    return out


def case(name):
    c = _all()[name]
    if c.candidates is True:
        c.candidates, _ = _columns(c.expect["cands"])
    return c


def bins_array(d):
    a = np.zeros(gc_ref.GC_BINS, np.uint64)
    for b, n in d.items():
        a[b] += n
    return a


def three_unequal_batches(batch):
    """The batch cut in three unequal parts; a mate pair may straddle a cut."""
    n = batch.n
    cuts = [0, max(1, n // 5), max(2, (3 * n) // 5 + 1), n] if n >= 3 else [0, n]
    return [batch.slice(lo, hi) for lo, hi in zip(cuts[:-1], cuts[1:])]
