"""The catalogue of --mismatches: a small reference (two contigs with sequence, one without, and a fourth header contig the reference does
not reach), explicit records (flag, name, seq, qual, tid, pos, mapq, ops; tests/mismatch_ref.py says what they count as) at the smallest
shapes at which the stage can go wrong, and a builder that writes the same alignments as BAM records, as SAM lines and through BGZF with
chosen block cuts.  Pure Python (struct, zlib, random): no product code is involved in building an input."""
import functools
import random
import struct

from tests import cycle_ref
from tests import mismatch_ref as ref
from tests.cycle_cases import BGZF_EOF, bgzf_block, cut  # noqa: F401  (the BGZF pieces are the same)

M, I, D, N, S, H, P, EQ, X = range(9)
MIN_MAPQ = 10                                                    # what the tests run the catalogue with


def _make_reference():
    rng = random.Random(20)
    a = [rng.choice("ACGT") for _ in range(21001)]               # 21001: the last word holds one base, chrB starts a new one
    a[100:124] = "NnacgtRYKMryswBDHVbdhvXx"                      # N, lower case and IUPAC
    b = [rng.choice("ACGT") for _ in range(1003)]
    return [("chrA", 21001, "".join(a)), ("chrB", 1003, "".join(b)), ("chrC", 500, None)]


REFERENCE = _make_reference()
CONTIGS = [(name, length) for name, length, _ in REFERENCE] + [("chrD", 500_000)]      # tid 3: a header contig beyond the reference's n


def _qual(L, salt=0):
    return [(i * 11 + i // 64 + salt) % 64 for i in range(L)]


def aligned(flag, name, tid, pos, ops, subs=(), qual="auto", mapq=60, fill="TGCA"):
    """A record whose SEQ is the reference under its CIGAR (upper case; N outside the contig), with the query indices of `subs` replaced
    by the next base (A>C>G>T>A), and the bases of I and S taken from `fill`."""
    text, length = REFERENCE[tid][2], REFERENCE[tid][1]
    seq, p = [], pos
    for n, code in ops:
        if code in (M, EQ, X):
            seq += [text[p + k].upper() if 0 <= p + k < length else "N" for k in range(n)]
            p += n
        elif code in (I, S):
            seq += [fill[(len(seq) + k) % len(fill)] for k in range(n)]
        elif code in (D, N):
            p += n
    for i in subs:
        seq[i] = "ACGT"[("ACGT".find(seq[i]) + 1) % 4] if seq[i] in "ACGT" else "A"
    seq = "".join(seq)
    return (flag, name, seq, _qual(len(seq), len(name)) if qual == "auto" else qual, tid, pos, mapq, list(ops))


FLAGS4 = (0x0, 0x10, 0x1 | 0x80, 0x1 | 0x80 | 0x10)


def match_lengths():
    out = []
    for L in (1, 2, 63, 64, 65, 127, 128, 129, 700, 20000):
        for flag in FLAGS4:
            out.append(aligned(flag, "len%d_%x" % (L, flag), 0, 400 + (L & 7), [(L, M)], subs=[s for s in (0, L // 2, L - 1, 511, 512) if s < L]))
    return out


def mismatch_positions():
    """A mismatch at every lane position 0..64 of a 65-base match, forward and reverse."""
    return [aligned(0x10 if i & 1 else 0x0, "at%d" % i, 0, 1000 + i, [(65, M)], subs=[i]) for i in range(65)]


def substitution_types():
    out = []
    text = REFERENCE[1][2]
    for flag in (0x0, 0x10, 0x1 | 0x80 | 0x10):
        for r in "ACGT":
            at = text.index(r, 10)
            for b in "ACGT":
                if b == r:
                    continue
                rec = aligned(flag, "sub%s%s_%x" % (r, b, flag), 1, at - 2, [(5, M)])
                out.append(rec[:2] + (rec[2][:2] + b + rec[2][3:],) + rec[3:])
    return out


def operation_order():
    cigars = {
        "eqx": [(5, EQ), (3, X), (2, EQ)], "i_first": [(3, I), (10, M)], "i_last": [(10, M), (3, I)], "i_mid": [(5, M), (3, I), (5, M)],
        "s_first": [(3, S), (10, M)], "s_last": [(10, M), (3, S)], "s_both": [(70, S), (5, M), (66, S)], "d_mid": [(5, M), (2, D), (5, M)],
        "d_first": [(2, D), (10, M)], "d_last": [(10, M), (2, D)], "d_behind_i": [(5, M), (3, I), (2, D), (5, M)], "two_d": [(5, M), (2, D), (3, D), (5, M)],
        "n_mid": [(5, M), (100, N), (5, M)], "n_first": [(100, N), (10, M)], "n_last": [(10, M), (7, N)], "h_first": [(2, H), (10, M)], "h_last": [(10, M), (2, H)],
        "h_both_s": [(4, H), (2, S), (10, M), (1, S), (3, H)], "p_mid": [(5, M), (1, P), (5, M)], "p_first": [(2, P), (10, M)], "p_last": [(10, M), (2, P)], "s_i_adjacent": [(2, S), (3, I), (8, M), (1, I), (2, S)],
        "n_d_adjacent": [(4, M), (50, N), (2, D), (4, M)], "i_only": [(7, I)], "s_only": [(9, S)],
        "zero_m": [(0, M), (10, M)], "zero_i": [(5, M), (0, I), (5, M)], "zero_d": [(5, M), (0, D), (5, M)], "zero_s_n": [(0, S), (6, M), (0, N), (4, M)],
        "long_i": [(3, M), (130, I), (3, M)], "d_in_long": [(200, M), (1, D), (400, M)], "x_long": [(70, X)],
    }
    out = []
    for name, ops in cigars.items():
        for flag in (0x0, 0x10, 0x1 | 0x80 | 0x10):
            n_query = sum(n for n, c in ops if c in (M, I, S, EQ, X))
            out.append(aligned(flag, "%s_%x" % (name, flag), 0, 2000 + len(name), ops, subs=[n_query // 2]))
    return out


def bam_only_operations():
    """Codes above 8 have no SAM spelling."""
    return [aligned(f, "code9_%x" % f, 0, 3000, [(4, M), (3, 9), (2, 15), (4, M)], subs=[1]) for f in (0x0, 0x10)]


def reference_edges():
    out = []
    for pos in (96, 97, 99, 100, 101):                            # even and odd, over the N / lower case / IUPAC bases at [100, 124)
        out.append(aligned(0x0, "iupac%d" % pos, 0, pos, [(30, M)]))
        out.append(aligned(0x10, "iupac%dr" % pos, 0, pos, [(30, M)], subs=[9]))
    out.append(aligned(0x0, "over_end", 0, 21000, [(4, M)]))      # one base in front of the contig's end
    out.append(aligned(0x10, "last_word", 0, 20992, [(9, M)], subs=[8]))
    out.append(aligned(0x0, "b_start", 1, 0, [(12, M)], subs=[0]))        # a contig whose first base starts a new word
    out.append(aligned(0x10, "b_end", 1, 995, [(12, M)], subs=[7]))
    out.append(aligned(0x0, "behind_end", 1, 1003, [(5, M)]))
    out.append(aligned(0x0, "n_over_end", 1, 990, [(5, M), (5000, N), (5, M)]))
    for flag in (0x0, 0x10):                                      # read N and =, all 16 nibbles, the SAM spellings
        out.append((flag, "nib_%x" % flag, cycle_ref.NIBBLES, _qual(16, 1), 0, 500, 60, [(16, M)]))
        out.append((flag, "nib_odd_%x" % flag, "A" + cycle_ref.NIBBLES, _qual(17, 2), 0, 501, 60, [(17, M)]))
        out.append((flag, "text_%x" % flag, "acgtn=.RYK", _qual(10, 5), 0, 510, 60, [(10, M)]))
    out.append((0x0, "no_seq_contig", "ACGTACGT", _qual(8), 2, 10, 60, [(8, M)]))        # the FASTA lacks chrC
    out.append((0x0, "tid_beyond_n", "ACGTACGT", _qual(8), 3, 10, 60, [(8, M)]))         # the reference has three contigs
    return out


def bam_only_edges():
    """POS 0 makes a SAM record unmapped; a BAM record keeps pos = -1."""
    return [aligned(f, "pos_minus1_%x" % f, 0, -1, [(6, M)], subs=[3]) for f in (0x0, 0x10)]


def class_boundaries():
    out = []
    ok = aligned(0x0, "x", 0, 700, [(9, M)], subs=[4])
    for f in (0x0, 0x1, 0x1 | 0x40, 0x1 | 0x80, 0x1 | 0x40 | 0x80, 0x80, 0x400, 0x1 | 0x80 | 0x400, 0x4, 0x100, 0x200, 0x800, 0x1 | 0x80 | 0x100, 0x4 | 0x10, 0x900):
        out.append((f, "flag%x" % f) + ok[2:])
    out.append((0x100, "excl_noref") + ok[2:4] + (2,) + ok[5:])                          # each reason in front of the next
    out.append((0x0, "noref_lowq") + ok[2:4] + (2, 700, MIN_MAPQ - 1, ok[7]))
    out.append((0x0, "lowq_noseq", "", None, 0, 700, MIN_MAPQ - 1, ok[7]))
    out.append((0x0, "noseq", "", None, 0, 700, 60, ok[7]))
    out.append((0x0, "noseq_q", "", None, 0, 700, MIN_MAPQ, [(9, M), (2, D)]))
    out.append(ok[:1] + ("mapq_below",) + ok[2:6] + (MIN_MAPQ - 1, ok[7]))
    out.append(ok[:1] + ("mapq_at",) + ok[2:6] + (MIN_MAPQ, ok[7]))
    out.append(ok[:1] + ("mapq_0",) + ok[2:6] + (0, ok[7]))
    out.append(ok[:1] + ("mapq_255",) + ok[2:6] + (255, ok[7]))
    return out


def bam_only_inconsistent():
    ok = aligned(0x0, "x", 0, 800, [(3, S), (9, M), (2, I)], subs=[5])
    out = [ok[:1] + ("short",) + ok[2:7] + ([(3, S), (8, M), (2, I)],), ok[:1] + ("long",) + ok[2:7] + ([(3, S), (9, M), (3, I)],),
           ok[:1] + ("long_d",) + ok[2:7] + ([(3, S), (9, M), (5, D), (3, I)],), ok[:1] + ("no_ops",) + ok[2:7] + ([],),
           (0x0, "noseq_over_inconsistent", "", None, 0, 800, 60, [(3, M)]), ok[:1] + ("lowq_over_inconsistent",) + ok[2:6] + (MIN_MAPQ - 1, []),
           ok[:1] + ("huge_op",) + ok[2:7] + ([((1 << 28) - 1, M)],)]
    # a CG:B,I CIGAR of five operations behind the <L>S<n>N placeholder (the builder writes it so: see bam_record)
    out.append(aligned(0x0, "cgtag", 0, 900, [(4, M), (2, I), (30, N), (5, M), (3, S)], subs=[1, 7]))
    out.append(aligned(0x10, "cgtag_r", 0, 901, [(4, M), (2, D), (5, M), (1, I), (3, M)], subs=[0, 12]))
    return out


def wide():
    """300 operations: above what the one-byte operation column holds."""
    return [aligned(f, "wide_%x" % f, 0, 5000, [(1, M), (1, I)] * 100 + [(2, M), (1, D)] * 50, subs=[0, 77, 199]) for f in (0x0, 0x10)]


def qualities(bam_only=False):
    out = []
    for v in (0, 62, 63, 64, 93):
        out.append(aligned(0x0, "q%d" % v, 0, 600, [(4, M)], subs=[1], qual=[v] * 4))
        out.append(aligned(0x1 | 0x80 | 0x10, "q%d_r2" % v, 0, 601, [(5, M)], subs=[4], qual=[v, 1, 2, 3, v]))
    out.append(aligned(0x0, "q_missing", 0, 602, [(7, M)], subs=[2], qual=None))
    out.append(aligned(0x10, "q_missing_L1", 0, 603, [(1, M)], qual=None))
    out.append(aligned(0x0, "q_same_64", 0, 604, [(64, M)], subs=[0, 15, 16, 63], qual=[30] * 64))          # one value on all 64 lanes
    out.append(aligned(0x0, "q_two_values", 0, 605, [(2, S), (128, M)], subs=[5, 100], qual=[37, 12] * 65))
    if bam_only:
        out.append(aligned(0x0, "q254", 0, 606, [(5, M)], subs=[0, 3], qual=[254, 0, 254, 63, 64]))
        out.append(aligned(0x10, "q_late_ff", 0, 607, [(6, M)], subs=[1], qual=[7, 0xFF, 0xFF, 1, 0xFF, 2]))
    return out


def names():
    """Read names of 1..9 bytes: with the NUL, the operations, SEQ and QUAL start at every offset mod 8."""
    out = []
    for n in range(1, 10):
        for L in (15, 16, 130):
            out.append(aligned(0x10 if n % 2 else 0x0, "n" * n, 1, 20 + n, [(2, S), (L - 2, M)], subs=[L - 1, L // 2]))
    return out


def pileup():
    """70 000 identical short records: more than 65 535 in one LDS cell; then the same split over both ends."""
    one = aligned(0x0, "p", 0, 300, [(1, S), (4, M), (1, D), (1, M)], subs=[2], qual=[30, 31, 32, 33, 30, 30])
    two = (0x1 | 0x80,) + one[1:]
    return [one] * 70000 + [one if k % 2 else two for k in range(70000)]


def catalogue(bam_only=False):
    out = match_lengths() + mismatch_positions() + substitution_types() + operation_order() + reference_edges() + class_boundaries() + wide() + qualities(bam_only) + names()
    if bam_only:
        out += bam_only_operations() + bam_only_edges() + bam_only_inconsistent()
    return out


def mixed(n=20000, seed=11):
    """About 20 000 seeded-random records: spliced and indel CIGARs over the reference with 1 % substitutions, binned qualities, a few
    without SEQ or QUAL, of every class, both ends and strands."""
    rng = random.Random(seed)
    bins = [2, 12, 23, 37, 40]
    out = []
    for k in range(n):
        r = rng.random()
        flag = rng.choice((0x0, 0x10, 0x1 | 0x40, 0x1 | 0x40 | 0x10, 0x1 | 0x80, 0x1 | 0x80 | 0x10))
        if r < 0.02:
            flag |= rng.choice((0x4, 0x100, 0x200, 0x800))
        if r > 0.97:
            flag |= 0x400
        tid = 0 if r < 0.8 else rng.choice((0, 1, 1, 2, 3))
        ops = []
        if rng.random() < 0.3:
            ops.append((rng.randint(1, 20), S))
        ops.append((rng.randint(1, 150), M))
        for _ in range(rng.choice((0, 0, 0, 1, 1, 2, 3))):
            ops.append((rng.randint(1, 300) if rng.random() < 0.5 else rng.randint(1, 4), rng.choice((I, D, N, N))))
            ops.append((rng.randint(1, 150), M))
        if rng.random() < 0.2:
            ops.append((rng.randint(1, 20), S))
        span = sum(m for m, c in ops if c in (M, D, N))
        limit = REFERENCE[tid][1] if tid < 3 else 5000
        pos = rng.randint(0, max(limit - span + 3, 0))
        if tid >= 2:
            L = sum(m for m, c in ops if c in (M, I, S))
            rec = (flag, "m%d" % k, "".join(rng.choices("ACGT", k=L)), None, tid, pos, 0, ops)
        else:
            rec = aligned(flag, "m%d" % k, tid, pos, ops, qual=None)
        L = len(rec[2])
        seq = list(rec[2])
        for i in range(L):
            if rng.random() < 0.01:
                seq[i] = rng.choice("ACGTN")
        mapq = rng.choice((3, 9, 10, 60, 60, 60, 60, 255))
        if 0.03 < r < 0.04:
            out.append((flag, "m%d" % k, "", None, tid, pos, mapq, ops))
            continue
        qual = None if 0.04 < r < 0.05 else rng.choices(bins, k=L)
        out.append((flag, "m%d" % k, "".join(seq), qual, tid, pos, mapq, ops))
    return out


def in_coordinate_order(records):
    """The records as a coordinate-sorted file holds them (a stable sort by contig and position)."""
    return sorted(records, key=lambda r: (r[4], r[5]))


@functools.lru_cache(maxsize=None)
def mixed_tables():
    """(records, tables of the first half, of the second half, of all) at MIN_MAPQ, each (cyc, subst, byq, info): computed once per session
    and shared by the tests that need it; nobody changes it."""
    records = mixed()
    half = len(records) // 2
    a, b = ref.tables(records[:half], REFERENCE, MIN_MAPQ), ref.tables(records[half:], REFERENCE, MIN_MAPQ)
    return records, a, b, ref.add(a, b)


@functools.lru_cache(maxsize=None)
def catalogue_tables(bam_only):
    return ref.tables(catalogue(bam_only), REFERENCE, MIN_MAPQ)


# ---- spellings -------------------------------------------------------------------------------------------------------------------
def bam_record(rec):
    """block_size + record, with where the operations, SEQ and QUAL start (offsets from the block_size field)."""
    flag, name, seq, qual, tid, pos, mapq, ops = rec
    L = len(seq)
    nm = name.encode("latin-1") + b"\x00"
    nib = [cycle_ref.nibble_of_text(ch) for ch in seq] + [0]
    packed = bytes((nib[2 * k] << 4) | nib[2 * k + 1] for k in range((L + 1) // 2))
    q = b"\xff" * L if qual is None else bytes(qual)
    assert len(q) == L
    words = [(n << 4) | code for n, code in ops]
    tail = b"NMC\x00"
    if name.startswith("cgtag"):                                     # the real CIGAR in CG:B,I, the placeholder <L>S<reference span>N in its place
        span = sum(n for n, code in ops if code in (M, D, N, EQ, X))
        tail += b"CGBI" + struct.pack("<I", len(words)) + struct.pack("<%dI" % len(words), *words)
        words = [(L << 4) | S, (span << 4) | N]
    body = struct.pack("<iiBBHHHiiii", tid, pos, len(nm), mapq, 4680, len(words), flag, L, -1, -1, 0) + nm
    ops_off = 4 + len(body)
    body += struct.pack("<%dI" % len(words), *words)
    seq_off = 4 + len(body)
    body += packed
    qual_off = 4 + len(body)
    body += q + tail
    return struct.pack("<I", len(body)) + body, ops_off, seq_off, qual_off


def sam_line(rec):
    flag, name, seq, qual, tid, pos, mapq, ops = rec
    assert qual is None or max(qual) <= 93, "a quality above 93 has no SAM spelling"
    assert all(code <= 8 for _, code in ops) and pos >= 0
    q = "*" if qual is None else "".join(chr(v + 33) for v in qual)
    cigar = "".join("%d%s" % (n, ref.OPS[code]) for n, code in ops) or "*"
    f = [name, str(flag), CONTIGS[tid][0], str(pos + 1), str(mapq), cigar, "*", "0", "0", seq or "*", q, "NM:i:0"]
    return "\t".join(f).encode("latin-1") + b"\n"


def _sq(contigs):
    return "@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % c for c in contigs)


def bam_header(contigs=None):
    contigs = contigs or CONTIGS
    text = _sq(contigs).encode()
    out = b"BAM\x01" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(contigs))
    for name, length in contigs:
        out += struct.pack("<i", len(name) + 1) + name.encode() + b"\x00" + struct.pack("<i", length)
    return out


def sam_header():
    return _sq(CONTIGS).encode()


def bam_body(records):
    """The records one behind the other, and per record (start, operations, SEQ, QUAL, end) in that stream."""
    parts, where, at, memo = [], [], 0, {}
    for r in records:
        key = id(r)
        if key not in memo:
            memo[key] = bam_record(r)
        b, oo, so, qo = memo[key]
        parts.append(b); where.append((at, at + oo, at + so, at + qo, at + len(b))); at += len(b)
    return b"".join(parts), where


def sam_body(records):
    memo = {}
    return b"".join(memo.setdefault(id(r), sam_line(r)) for r in records)


def write_fasta(path, width=60):
    """The reference's contigs that have a sequence, and the .fai index beside it."""
    with open(path, "w") as f, open(path + ".fai", "w") as fai:
        at = 0
        for name, length, text in REFERENCE:
            if text is None:
                continue
            head = ">%s\n" % name
            f.write(head); at += len(head)
            fai.write("%s\t%d\t%d\t%d\t%d\n" % (name, length, at, width, width + 1))
            for a in range(0, length, width):
                f.write(text[a:a + width] + "\n")
            at += length + (length + width - 1) // width


def write_bam(path, records, cuts=(), block=0xFF00, contigs=None):
    """A BAM file: the header (contigs: another list of (name, LN) than CONTIGS) in blocks of its own, then the records cut as cut() says."""
    body, _ = bam_body(records)
    with open(path, "wb") as f:
        for piece in cut(bam_header(contigs)) + cut(body, cuts, block):
            f.write(bgzf_block(piece)[0])
        f.write(BGZF_EOF)


def write_sam(path, records, bgzf=False, cuts=(), block=0xFF00):
    text = sam_header() + sam_body(records)
    with open(path, "wb") as f:
        if not bgzf:
            f.write(text)
            return
        for piece in cut(text, cuts, block):
            f.write(bgzf_block(piece)[0])
        f.write(BGZF_EOF)
