"""The catalogue of --alleles: site lists over the four contigs of tests/mismatch_cases.py's header (chrA 21001, chrB 1003, chrC 500, chrD
500000 -- the record builders of that module spell RNAME from its CONTIGS, and the stage needs no lengths), and explicit records (flag,
name, seq, qual, tid, pos, mapq, ops; tests/allele_ref.py says what they count as) at the smallest shapes at which the stage can go wrong.
The builders that write the same alignments as BAM records, as SAM lines and through BGZF are mismatch_cases' own.  Pure Python: no
product code is involved in building an input."""
import functools
import random

from tests import allele_ref as ref
from tests.mismatch_cases import (BGZF_EOF, CONTIGS, bam_body, bam_header, bgzf_block, cut, in_coordinate_order, sam_body, sam_header, sam_line,  # noqa: F401
                                  write_bam, write_sam)

M, I, D, N, S, H, P, EQ, X = range(9)
NAMES = [c[0] for c in CONTIGS]
N_CONTIGS = len(CONTIGS)
MIN_MAPQ, MIN_BASEQ = 10, 20                                     # what the tests run the catalogue with
FAR = 2 ** 31 - 20                                               # where the records near the end of the position range start


def _sites():
    a = set(range(5000, 21001, 7)) | {0}                         # a site every 7 positions under most of the 20 000-base record; POS 0
    a |= {999, 1000, 1009, 1010}                                 # p - 1, the first and the last base of a block, p + n
    a |= {1100, 1102, 1103, 1105, 1106}                          # around I and S
    a |= {1202, 1203, 1204, 1205, 1206}                          # in front of, under every position of, and right behind a D
    a |= {1302, 1303, 1307, 1312, 1313, 1315, 1316}              # in front of, under and behind an N
    a |= set(range(2003, 3003)) | {2001, 3004}                   # an N over 1 000 sites, then a hit
    a |= set(range(3100, 3107)) | set(range(3200, 3501, 3)) | {3601, 3610, 3634, 3636}
    a |= set(range(4000, 4065)) | set(range(4100, 4116))         # 65 adjacent sites; the nibbles
    b = {100, 101, 500, 900, 1002}                               # 1002: the last position of chrB ...
    c = {0, 1, 2, 3, 4, 2 ** 31 - 10, 2 ** 31 - 2}               # ... and chrC from position 0; the two largest positions a site may have
    return [(0, p) for p in sorted(a)] + [(1, p) for p in sorted(b)] + [(2, p) for p in sorted(c)]       # chrD, the last contig: none


SITES = _sites()


def site_lists():
    """The catalogue's table at its edges: no site, one, two; a first, a middle and a last contig without sites."""
    return {"main": SITES, "empty": [], "one": [(0, 1000)], "two": [(0, 1009), (1, 1002)], "no_first": [s for s in SITES if s[0] != 0],
            "no_middle": [s for s in SITES if s[0] != 1] + [(3, 5)]}


def _seq(name, L):
    rng = random.Random(name)
    return "".join(rng.choice("ACGT") for _ in range(L))


def _qual(L, salt=0):
    return [(i * 11 + i // 64 + salt) % 42 for i in range(L)]     # (on both sides of MIN_BASEQ)


def rec(name, tid, pos, ops, flag=0x0, mapq=60, seq=None, qual="auto"):
    L = sum(n for n, code in ops if code in (M, I, S, EQ, X))
    seq = _seq(name, L) if seq is None else seq
    return (flag, name, seq, _qual(len(seq), len(name)) if qual == "auto" else qual, tid, pos, mapq, list(ops))


def operations():
    out = []
    for flag in (0x0, 0x10, 0x1 | 0x80 | 0x10):                   # (a reverse-strand record: no complement)
        for code in (M, EQ, X):
            out.append(rec("edge_%s_%x" % ("MIDNSHPEX"[code], flag), 0, 1000, [(10, code)], flag))
    out.append(rec("i_and_s", 0, 1100, [(2, S), (3, M), (2, I), (3, M), (2, S)]))
    out.append(rec("d_mid", 0, 1200, [(3, M), (3, D), (3, M)]))
    out.append(rec("d_first", 0, 1203, [(3, D), (4, M)], 0x10))
    out.append(rec("n_mid", 0, 1300, [(3, M), (10, N), (3, M)]))
    out.append(rec("n_skips_1000", 0, 2000, [(3, M), (1000, N), (3, M)]))
    out.append(rec("n_d_adjacent", 0, 1299, [(3, M), (2, N), (3, D), (2, M)]))
    out.append(rec("zero_h_p", 0, 3100, [(0, M), (2, H), (3, M), (0, D), (1, P), (0, N), (3, M), (0, I), (0, S), (2, H)]))
    out.append(rec("s_both", 0, 3103, [(70, S), (4, M), (66, S)]))
    for flag in (0x0, 0x10):
        out.append(rec("wide_%x" % flag, 0, 3200, [(1, M), (1, I)] * 100 + [(1, M), (1, D)] * 50, flag))       # 300 one-base operations
    out.append(rec("long_20000", 0, 500, [(20000, M)]))
    out.append(rec("long_spliced", 0, 3, [(5000, M), (5000, N), (4000, M), (3, D), (4000, M)], 0x10))
    for L in (63, 64, 65):
        out.append(rec("adjacent_%d" % L, 0, 4000, [(L, M)]))
        out.append(rec("adjacent_odd_%d" % L, 0, 4001, [(1, S), (L - 1, M)], 0x10))
    return out


def bam_only_operations():
    """Codes above 8 have no SAM spelling; the CG:B,I CIGAR is a BAM device (the builder writes it for names that start with cgtag)."""
    return [rec("code9", 0, 3100, [(3, M), (4, 9), (2, 15), (3, M)]), rec("cgtag", 0, 3600, [(4, M), (2, I), (30, N), (5, M), (3, S)]),
            rec("cgtag_r", 0, 3599, [(4, M), (2, D), (5, M), (1, I), (3, M)], 0x10)]


def bases_and_qualities(bam_only=False):
    out = [rec("nibbles", 0, 4100, [(16, M)], seq=ref.NIBBLES, qual=[40] * 16),
           rec("nibbles_odd", 0, 4099, [(17, M)], 0x10, seq="A" + ref.NIBBLES, qual=[40] * 17),
           rec("lower_case", 0, 4100, [(10, M)], seq="acgtn=.RYk", qual=[40] * 10),
           rec("q_at_and_below", 0, 4000, [(6, M)], qual=[MIN_BASEQ, MIN_BASEQ - 1, MIN_BASEQ + 1, 0, 93, MIN_BASEQ]),
           rec("q_missing", 0, 4002, [(7, M)], qual=None),
           rec("q_missing_L1", 0, 1000, [(1, M)], 0x10, qual=None)]
    if bam_only:
        out.append(rec("q_93_and_above", 0, 4003, [(5, M)], qual=[93, 94, 200, 254, MIN_BASEQ - 1]))
        out.append(rec("q_late_ff", 0, 4004, [(4, M)], qual=[7, 0xFF, 0xFF, 30]))
    return out


def sam_only_qualities():
    """A QUAL byte below 33 (a space): the value is floored at 0, so it lies below MIN_BASEQ."""
    return [rec("q_below_33", 0, 4000, [(5, M)], qual=[-1, 40, -1, MIN_BASEQ, -1])]


def table_edges():
    out = [rec("pos_0", 0, 0, [(5, M)]),
           rec("in_front_of_the_first", 1, 10, [(5, M)]), rec("up_to_the_first", 1, 95, [(5, M)]), rec("onto_the_first", 1, 96, [(5, M)]),
           rec("behind_the_last", 1, 1003, [(5, M)]), rec("past_the_end_of_b", 1, 998, [(10, M)]), rec("d_past_the_end_of_b", 1, 1000, [(2, M), (8, D), (2, M)], 0x10),
           rec("start_of_c", 2, 0, [(3, M), (1, D), (1, M)]), rec("no_sites_on_d", 3, 0, [(30, M)]), rec("no_sites_on_d_5", 3, 5, [(3, N), (30, M)])]
    return out


def bam_only_edges():
    """POS 0 makes a SAM record unmapped; a BAM record keeps pos = -1.  Positions near 2^31 with long N: p is 64 bits wide -- with 32 it
    would come back to 0 under the last block and count chrC's first sites."""
    far = [(19, M)] + [((1 << 28) - 1, N)] * 24 + [(25, N), (5, M)]
    assert FAR + 19 + sum(n for n, c in far[1:-1]) == 2 ** 33
    return [rec("pos_minus1", 0, -1, [(6, M)]), rec("pos_minus1_r", 0, -1, [(2, S), (1, M), (3, D), (2, M)], 0x10),
            rec("far", 2, FAR, far), rec("far_d", 2, 2 ** 31 - 3, [(1, M), (5, D), (1, M)]), rec("far_start", 2, 2 ** 31 - 1, [(4, M)])]


def classes():
    ok = rec("x", 0, 1000, [(10, M)])
    out = []
    for f in (0x0, 0x1, 0x1 | 0x40, 0x1 | 0x80, 0x400, 0x1 | 0x80 | 0x400, 0x4, 0x100, 0x200, 0x800, 0x1 | 0x80 | 0x100, 0x4 | 0x10, 0x900):
        out.append((f, "flag%x" % f) + ok[2:])
    out.append((0x100, "excl_lowq") + ok[2:6] + (MIN_MAPQ - 1, ok[7]))                       # each reason in front of the next
    out.append((0x0, "lowq_noseq", "", None, 0, 1000, MIN_MAPQ - 1, ok[7]))
    out.append((0x0, "noseq", "", None, 0, 1000, 60, ok[7]))
    for name, mapq in (("mapq_below", MIN_MAPQ - 1), ("mapq_at", MIN_MAPQ), ("mapq_0", 0), ("mapq_255", 255)):
        out.append(ok[:1] + (name,) + ok[2:6] + (mapq, ok[7]))
    return out


def bam_only_classes():
    ok = rec("x", 0, 1000, [(3, S), (9, M), (2, I)])
    return [ok[:1] + ("short",) + ok[2:7] + ([(3, S), (8, M), (2, I)],), ok[:1] + ("long",) + ok[2:7] + ([(3, S), (9, M), (3, I)],),
            ok[:1] + ("no_ops",) + ok[2:7] + ([],), (0x0, "noseq_over_inconsistent", "", None, 0, 1000, 60, [(3, M)]),
            ok[:1] + ("lowq_over_inconsistent",) + ok[2:6] + (MIN_MAPQ - 1, []),
            ok[:4] + (-1,) + ok[5:], ok[:1] + ("tid_n",) + ok[2:4] + (N_CONTIGS,) + ok[5:], ok[:1] + ("tid_n_lowq",) + ok[2:4] + (N_CONTIGS, 1000, MIN_MAPQ - 1, ok[7]),
            (0x200, "excl_off_contig") + ok[2:4] + (-1,) + ok[5:]]


def catalogue(bam_only=False):
    out = operations() + bases_and_qualities(bam_only) + table_edges() + classes()
    if bam_only:
        out += bam_only_operations() + bam_only_edges() + bam_only_classes()
    return out


def pileup():
    """140 000 records over one site and its two neighbours, half of them another base there: a cell above 65 535 in one launch."""
    one = rec("p", 0, 998, [(1, S), (4, M), (1, D), (1, M)], seq="TACGTA", qual=[30, 31, 32, 33, 30, 30])
    two = (0x1 | 0x80 | 0x10,) + one[1:2] + ("TATGTA",) + one[3:]
    off = [rec("p_in_front", 0, 900, [(5, M)]), rec("p_one_site", 0, 1003, [(3, M)]), rec("p_behind", 0, 1100, [(5, M)])]
    return [one if k % 2 else two for k in range(70000)] + off + [one if k % 2 else two for k in range(70000, 140000)]


PILE_SITES = [(0, 999), (0, 1000), (0, 1001), (0, 1002), (0, 1003)]


MIXED_SITES = sorted({(0, p) for p in random.Random(5).sample(range(21001), 3000)} | {(3, p) for p in random.Random(6).sample(range(500_000), 1000)})


def mixed(n=20000, seed=12):
    """Seeded random records over MIXED_SITES -- about one site per 7 positions on chrA, one per 500 on chrD --: spliced and indel CIGARs,
    binned qualities, a few without SEQ or QUAL, of every class the two spellings share, both strands."""
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
        tid = 0 if r < 0.6 else rng.choice((0, 1, 2, 3, 3, 3))
        ops = []
        if rng.random() < 0.3:
            ops.append((rng.randint(1, 20), S))
        ops.append((rng.randint(1, 150), M))
        for _ in range(rng.choice((0, 0, 0, 1, 1, 2, 3))):
            ops.append((rng.randint(1, 3000) if rng.random() < 0.5 else rng.randint(1, 4), rng.choice((I, D, N, N))))
            ops.append((rng.randint(1, 150), M))
        if rng.random() < 0.2:
            ops.append((rng.randint(1, 20), S))
        span = sum(m for m, c in ops if c in (M, D, N))
        pos = rng.randint(0, max(CONTIGS[tid][1] - span + 3, 0))
        L = sum(m for m, c in ops if c in (M, I, S))
        mapq = rng.choice((3, 9, 10, 60, 60, 60, 60, 255))
        if 0.03 < r < 0.04:
            out.append((flag, "m%d" % k, "", None, tid, pos, mapq, ops))
            continue
        qual = None if 0.04 < r < 0.05 else rng.choices(bins, k=L)
        out.append((flag, "m%d" % k, "".join(rng.choices("ACGTN", weights=(25, 25, 25, 24, 1), k=L)), qual, tid, pos, mapq, ops))
    return out


@functools.lru_cache(maxsize=None)
def mixed_tables(n=20000):
    """(records, table of the first half, of the second half, of all) at MIN_MAPQ and MIN_BASEQ, each (counts, info): computed once per
    session and shared by the tests that need it; nobody changes it."""
    records = mixed(n)
    half = len(records) // 2
    a, b = (ref.tables(part, N_CONTIGS, MIXED_SITES, MIN_MAPQ, MIN_BASEQ) for part in (records[:half], records[half:]))
    return records, a, b, ref.add(a, b)


@functools.lru_cache(maxsize=None)
def catalogue_tables(bam_only, sites="main"):
    return ref.tables(catalogue(bam_only), N_CONTIGS, site_lists()[sites], MIN_MAPQ, MIN_BASEQ)


def one(name, bam_only=True, extra=()):
    """What the record of that name counts as, alone: (counts by site as a dict of the non-zero rows, info)."""
    records = [r for r in list(catalogue(bam_only)) + list(extra) if r[1] == name]
    assert len(records) == 1, name
    counts, info = ref.tables(records, N_CONTIGS, SITES, MIN_MAPQ, MIN_BASEQ)
    return {SITES[k]: row for k, row in enumerate(counts) if any(row)}, info


# ---- the site file ---------------------------------------------------------------------------------------------------------------------
def vcf_text(sites, names=None, seed=3):
    """A VCF body for the sites (seeded ID, REF and ALT, one multi-allelic and one symbolic ALT among them), behind two '#' lines."""
    names = names or NAMES
    rng = random.Random(seed)
    out = ["##fileformat=VCFv4.2", "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO"]
    for k, (tid, pos) in enumerate(sites):
        r = rng.choice("ACGT")
        alt = rng.choice([b for b in "ACGT" if b != r])
        if k % 50 == 7:
            alt += "," + rng.choice([b for b in "ACGT" if b not in (r, alt)])
        if k % 50 == 9:
            alt = "<DEL>"
        out.append("%s\t%d\t%s\t%s\t%s\t.\tPASS\t." % (names[tid], pos + 1, "rs%d" % k if k % 3 else ".", r, alt))
    return "\n".join(out) + "\n"
