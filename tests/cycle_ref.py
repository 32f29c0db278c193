"""The contract of --cycles / rsqc_cycles_* (include/rnaseqc_amd.h) restated in plain Python: the tables and the info of a list of
records, and the text of the two files.  A record is (flag, name, seq, qual): seq is the SAM text of SEQ ("" stands for *), qual the
list of quality values as BAM stores them (0..255), or None for a missing QUAL.  Nothing here looks at the product's code; the tests
compare with it bit for bit and byte for byte."""

CYCLE_MAX, QBINS, ENDS, BASES = 512, 64, 2, 5
NIBBLES = "=ACMGRSVTWYHKDBN"
INFO_FIELDS = ("seen_records", "records", "no_seq_records", "no_qual_records", "bases", "beyond_bases", "clamped_quals")


def nibble_of_text(ch):
    """The BAM nibble a SAM SEQ character is stored as (what htslib writes: the letter's upper case, anything unknown as N)."""
    k = NIBBLES.find(ch.upper())
    return k if k >= 0 else 15


def base_of_nibble(n):
    return {1: 0, 2: 1, 4: 2, 8: 3}.get(n, 4)


def base_of_text(ch):
    return {"A": 0, "C": 1, "G": 2, "T": 3}.get(ch.upper(), 4) if len(ch) == 1 and ch.isascii() else 4


def end_of(flag):
    return 1 if (flag & 0x1) and (flag & 0x80) and not (flag & 0x40) else 0


def counted(flag):
    return (flag & (0x100 | 0x200 | 0x800)) == 0


def quality_missing(qual):
    return qual is None or (len(qual) > 0 and qual[0] == 0xFF)


def tables(records, nibbles=False):
    """(base, qual, info): base[e][c][b] and qual[e][c][q] as nested lists.  nibbles: take the base of a SEQ character from the nibble
    BAM stores it as (the two readings agree on every character; the tests check that too)."""
    base = [[[0] * BASES for _ in range(CYCLE_MAX)] for _ in range(ENDS)]
    qual = [[[0] * QBINS for _ in range(CYCLE_MAX)] for _ in range(ENDS)]
    info = dict.fromkeys(INFO_FIELDS, 0)
    for flag, _name, seq, q in records:
        info["seen_records"] += 1
        if not counted(flag):
            continue
        L = len(seq)
        if L == 0:
            info["no_seq_records"] += 1
            continue
        info["records"] += 1
        missing = quality_missing(q)
        if missing:
            info["no_qual_records"] += 1
        e, rev = end_of(flag), bool(flag & 0x10)
        be, qe = base[e], qual[e]
        for i in range(L):
            c = L - 1 - i if rev else i
            if c >= CYCLE_MAX:
                info["beyond_bases"] += 1
                continue
            b = base_of_nibble(nibble_of_text(seq[i])) if nibbles else base_of_text(seq[i])
            if rev and b < 4:
                b = 3 - b
            be[c][b] += 1
            info["bases"] += 1
            if missing:
                continue
            v = q[i]
            if v > QBINS - 1:
                v = QBINS - 1
                info["clamped_quals"] += 1
            qe[c][v] += 1
    return base, qual, info


def add_tables(a, b):
    return [[[x + y for x, y in zip(ra, rb)] for ra, rb in zip(ea, eb)] for ea, eb in zip(a, b)]


def rows_of_end(base, e):
    rows = 0
    for c in range(CYCLE_MAX):
        if sum(base[e][c]):
            rows = c + 1
    return rows


def format_bases(base):
    out = ["end\tcycle\tA\tC\tG\tT\tN\ttotal"]
    for e in range(ENDS):
        for c in range(rows_of_end(base, e)):
            out.append("\t".join(str(v) for v in [e + 1, c + 1] + list(base[e][c]) + [sum(base[e][c])]))
    return "\n".join(out) + "\n"


def quantile(cell, k):
    """The smallest q with 4 cum(q) >= k n; 0 for n = 0."""
    n, cum = sum(cell), 0
    if n == 0:
        return 0
    for q, v in enumerate(cell):
        cum += v
        if 4 * cum >= k * n:
            return q
    raise AssertionError("unreachable")


def format_quality(base, qual):
    out = ["end\tcycle\tbases\tmean\tq25\tmedian\tq75"]
    for e in range(ENDS):
        for c in range(rows_of_end(base, e)):
            cell = qual[e][c]
            n = sum(cell)
            mean = float(sum(q * v for q, v in enumerate(cell))) / float(n) if n else 0.0
            out.append("%d\t%d\t%d\t%.6f\t%d\t%d\t%d" % (e + 1, c + 1, n, mean, quantile(cell, 1), quantile(cell, 2), quantile(cell, 3)))
    return "\n".join(out) + "\n"
