"""The contract of --mismatches / rsqc_mismatch_* (include/rnaseqc_amd.h) restated in plain Python: the tables and the info of a list of
records over a reference, and the text of the three files.  A record is (flag, name, seq, qual, tid, pos, mapq, ops): seq is the SAM text
of SEQ ("" stands for *), qual the list of quality values as BAM stores them (0..255) or None for a missing QUAL, pos 0-based, ops the
CIGAR as a list of (length, code) with the BAM codes M I D N S H P = X = 0..8.  A reference is a list of (name, length, sequence or None).
Nothing here looks at the product's code; the tests compare with it bit for bit and byte for byte."""
from tests import cycle_ref

CYCLE_MAX, QBINS, ENDS, COLS = 512, 64, 2, 6
COMPARED, MISMATCH, UNCOMPARED, INSERTED, CLIPPED, DELETIONS = range(6)
INFO_FIELDS = ("seen_records", "records", "no_reference_records", "low_mapq_records", "no_seq_records", "inconsistent_records", "no_qual_records", "compared",
               "mismatched", "uncompared", "inserted", "clipped", "deletions", "insertion_events", "deletion_events", "deleted_bases", "beyond_bases", "clamped_quals")
OPS = "MIDNSHP=X"


def ref_code(ch):
    return {"A": 0, "C": 1, "G": 2, "T": 3, "a": 0, "c": 1, "g": 2, "t": 3}.get(ch, 4)


def empty_tables():
    return ([[[0] * COLS for _ in range(CYCLE_MAX)] for _ in range(ENDS)], [[[0] * 4 for _ in range(4)] for _ in range(ENDS)], [[0, 0] for _ in range(QBINS)])


def tables(records, reference, min_mapq=0, nibbles=False):
    """(cyc, subst, byq, info).  nibbles: take the base of a SEQ character from the nibble BAM stores it as."""
    cyc, subst, byq = empty_tables()
    info = dict.fromkeys(INFO_FIELDS, 0)
    for flag, _name, seq, qual, tid, pos, mapq, ops in records:
        info["seen_records"] += 1
        if flag & (0x4 | 0x100 | 0x200 | 0x800):
            continue
        if not (0 <= tid < len(reference)) or reference[tid][2] is None:
            info["no_reference_records"] += 1
            continue
        if mapq < min_mapq:
            info["low_mapq_records"] += 1
            continue
        L = len(seq)
        if L == 0:
            info["no_seq_records"] += 1
            continue
        if sum(n for n, code in ops if code in (0, 1, 4, 7, 8)) != L:
            info["inconsistent_records"] += 1
            continue
        info["records"] += 1
        missing = cycle_ref.quality_missing(qual)
        if missing:
            info["no_qual_records"] += 1
        length, text = reference[tid][1], reference[tid][2]
        e, rev = cycle_ref.end_of(flag), bool(flag & 0x10)
        q, p = 0, pos

        def cycle(i):
            return L - 1 - i if rev else i

        for n, code in ops:
            if n == 0:
                continue
            if code in (0, 7, 8):
                for k in range(n):
                    c = cycle(q + k)
                    if c >= CYCLE_MAX:
                        info["beyond_bases"] += 1
                        continue
                    ch = seq[q + k]
                    b = cycle_ref.base_of_nibble(cycle_ref.nibble_of_text(ch)) if nibbles else cycle_ref.base_of_text(ch)
                    r = ref_code(text[p + k]) if 0 <= p + k < length else 4
                    if b < 4 and r < 4:
                        cyc[e][c][COMPARED] += 1
                        if rev:
                            subst[e][3 - r][3 - b] += 1
                        else:
                            subst[e][r][b] += 1
                        if b != r:
                            cyc[e][c][MISMATCH] += 1
                        if not missing:
                            v = qual[q + k]
                            if v > QBINS - 1:
                                v = QBINS - 1
                                info["clamped_quals"] += 1
                            byq[v][0] += 1
                            if b != r:
                                byq[v][1] += 1
                    else:
                        cyc[e][c][UNCOMPARED] += 1
                q += n
                p += n
            elif code in (1, 4):
                for k in range(n):
                    c = cycle(q + k)
                    if c >= CYCLE_MAX:
                        info["beyond_bases"] += 1
                    else:
                        cyc[e][c][INSERTED if code == 1 else CLIPPED] += 1
                if code == 1:
                    info["insertion_events"] += 1
                q += n
            elif code == 2:
                c = cycle(min(q, L - 1))
                if c < CYCLE_MAX:
                    cyc[e][c][DELETIONS] += 1
                info["deletion_events"] += 1
                info["deleted_bases"] += n
                p += n
            elif code == 3:
                p += n
    for name, col in (("compared", COMPARED), ("mismatched", MISMATCH), ("uncompared", UNCOMPARED), ("inserted", INSERTED), ("clipped", CLIPPED), ("deletions", DELETIONS)):
        info[name] = sum(cell[col] for end in cyc for cell in end)
    return cyc, subst, byq, info


def add(a, b):
    """Two results of tables() added up."""
    def rec(x, y):
        return [rec(u, v) for u, v in zip(x, y)] if isinstance(x, list) else x + y
    return rec(a[0], b[0]), rec(a[1], b[1]), rec(a[2], b[2]), {f: a[3][f] + b[3][f] for f in INFO_FIELDS}


def rows_of_end(cyc, e):
    rows = 0
    for c in range(CYCLE_MAX):
        if any(cyc[e][c]):
            rows = c + 1
    return rows


def rate(mismatches, compared):
    return float(mismatches) / float(compared) if compared else 0.0


def format_cycles(cyc):
    out = ["end\tcycle\tcompared\tmismatches\tuncompared\tinserted\tclipped\tdeletions\tmismatch_rate"]
    for e in range(ENDS):
        for c in range(rows_of_end(cyc, e)):
            cell = cyc[e][c]
            out.append("\t".join(str(v) for v in [e + 1, c + 1] + list(cell)) + "\t%.6f" % rate(cell[MISMATCH], cell[COMPARED]))
    return "\n".join(out) + "\n"


def format_types(subst):
    out = ["end\tref\tread\tcount"]
    for e in range(ENDS):
        if not sum(sum(row) for row in subst[e]):
            continue
        for r in range(4):
            for b in range(4):
                out.append("%d\t%s\t%s\t%d" % (e + 1, "ACGT"[r], "ACGT"[b], subst[e][r][b]))
    return "\n".join(out) + "\n"


def format_quality(byq):
    out = ["quality\tcompared\tmismatches\tmismatch_rate"]
    for v in range(QBINS):
        if byq[v][0]:
            out.append("%d\t%d\t%d\t%.6f" % (v, byq[v][0], byq[v][1], rate(byq[v][1], byq[v][0])))
    return "\n".join(out) + "\n"
