"""The contract of --alleles / rsqc_alleles_* (include/rnaseqc_amd.h) restated in plain Python: the table and the info of a list of
records over a list of sites, the rules of the site file, and the text of <sample>.allele_counts.tsv.  A record is (flag, name, seq, qual,
tid, pos, mapq, ops) as in tests/mismatch_ref.py: seq is the SAM text of SEQ ("" stands for *), qual the list of quality values (as BAM
stores them, 0..255; a value below 0 stands for a SAM byte below 33) or None for a missing QUAL, pos 0-based, ops the CIGAR as a list of
(length, code) with the BAM codes M I D N S H P = X = 0..8.  A site is (tid, pos), 0-based; the list is strictly ascending.
Nothing here imports or looks at the product's code; the tests compare with it bit for bit and byte for byte."""
import bisect
import gzip

COLS = 7
A, C, G, T, OTHER, DELETED, LOW_BASEQ = range(7)
COLUMN_NAMES = ("A", "C", "G", "T", "other", "deleted", "low_baseq")
INFO_FIELDS = ("seen_records", "records", "off_contig_records", "low_mapq_records", "no_seq_records", "inconsistent_records", "no_qual_records", "hit_records",
               "observations", "n_sites")
OPS = "MIDNSHP=X"
NIBBLES = "=ACMGRSVTWYHKDBN"


def base_code(ch, nibbles=False):
    """0..3 for A C G T in either case, 4 for everything else.  nibbles: through the nibble BAM stores the character as."""
    if nibbles:
        k = NIBBLES.find(ch.upper())
        return {1: 0, 2: 1, 4: 2, 8: 3}.get(k if k >= 0 else 15, 4)
    return {"A": 0, "C": 1, "G": 2, "T": 3, "a": 0, "c": 1, "g": 2, "t": 3}.get(ch, 4)


def check_sites(n_contigs, sites):
    """The index of the first site that breaks a rule, or None."""
    for k, (tid, pos) in enumerate(sites):
        if not (0 <= tid < n_contigs) or not (0 <= pos < 2 ** 31 - 1) or (k and sites[k - 1] >= (tid, pos)):
            return k
    return None


def tables(records, n_contigs, sites, min_mapq=0, min_baseq=0, nibbles=False):
    """(counts, info): counts[site][column] as nested lists."""
    assert check_sites(n_contigs, sites) is None
    counts = [[0] * COLS for _ in sites]
    info = dict.fromkeys(INFO_FIELDS, 0)
    info["n_sites"] = len(sites)
    of_tid = {}                                                       # tid -> (index of its first site, its positions)
    for k, (tid, pos) in enumerate(sites):
        of_tid.setdefault(tid, (k, []))[1].append(pos)
    for flag, _name, seq, qual, tid, pos, mapq, ops in records:
        info["seen_records"] += 1
        if flag & (0x4 | 0x100 | 0x200 | 0x800):
            continue
        if not (0 <= tid < n_contigs):
            info["off_contig_records"] += 1
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
        missing = qual is None or (len(qual) > 0 and qual[0] == 0xFF)
        if missing:
            info["no_qual_records"] += 1
        first, positions = of_tid.get(tid, (0, []))
        q, p, seen = 0, pos, 0
        for n, code in ops:
            if n == 0:
                continue
            if code in (0, 7, 8):
                for k in range(bisect.bisect_left(positions, p), bisect.bisect_left(positions, p + n)):
                    i = q + (positions[k] - p)
                    if not missing and max(qual[i], 0) < min_baseq:
                        counts[first + k][LOW_BASEQ] += 1
                    else:
                        counts[first + k][base_code(seq[i], nibbles)] += 1
                    seen += 1
                q += n
                p += n
            elif code in (1, 4):
                q += n
            elif code == 2:
                for k in range(bisect.bisect_left(positions, p), bisect.bisect_left(positions, p + n)):
                    counts[first + k][DELETED] += 1
                    seen += 1
                p += n
            elif code == 3:
                p += n
        if seen:
            info["hit_records"] += 1
            info["observations"] += seen
    return counts, info


def add(a, b):
    """Two results of tables() over the same sites added up."""
    info = {f: a[1][f] + b[1][f] for f in INFO_FIELDS}
    info["n_sites"] = a[1]["n_sites"]
    return [[x + y for x, y in zip(ra, rb)] for ra, rb in zip(a[0], b[0])], info


# ---- the site file -----------------------------------------------------------------------------------------------------------------------
class SitesError(Exception):
    """A malformed line: (1-based line number)."""


def parse_sites(text):
    """The body lines of a VCF text: ([(chrom, pos1, id, ref, alt)], skipped_lines).  '#' lines and blank lines are skipped; fewer than
    five fields or a POS that is no integer in 1 .. 2^31 - 1 is malformed; a REF that is not exactly one of A C G T in either case skips
    the line."""
    out, skipped = [], 0
    for number, line in enumerate(text.split("\n"), 1):
        line = line.rstrip("\r")
        if not line or line.startswith("#"):
            continue
        f = line.split("\t")
        if len(f) < 5:
            raise SitesError(number)
        if not (f[1].isascii() and f[1].isdigit() and 1 <= int(f[1]) <= 2 ** 31 - 1):       # (digits only; leading zeros are read over)
            raise SitesError(number)
        if f[3] not in ("A", "C", "G", "T", "a", "c", "g", "t"):
            skipped += 1
            continue
        out.append((f[0], int(f[1]), f[2], f[3], f[4]))
    return out, skipped


def read_sites(path):
    with open(path, "rb") as f:
        data = f.read()
    return parse_sites((gzip.decompress(data) if data[:2] == b"\x1f\x8b" else data).decode("latin-1"))


def resolve_sites(lines, names):
    """The lines against a header's contig names: (sites [(tid, pos0)], meta [(id, ref, alt)], off_header_lines, duplicate_lines).  Sorted by
    (contig in header order, POS), stable; of lines with equal position the first is kept."""
    index = {}
    for k, name in enumerate(names):
        index.setdefault(name, k)
    kept, off = [], 0
    for chrom, pos1, ident, ref, alt in lines:
        if chrom not in index:
            off += 1
            continue
        kept.append((index[chrom], pos1 - 1, ident, ref, alt))
    kept.sort(key=lambda r: (r[0], r[1]))
    sites, meta, dup = [], [], 0
    for tid, pos, ident, ref, alt in kept:
        if sites and sites[-1] == (tid, pos):
            dup += 1
            continue
        sites.append((tid, pos)); meta.append((ident, ref, alt))
    return sites, meta, off, dup


# ---- the file --------------------------------------------------------------------------------------------------------------------------
FILE_HEADER = "contig\tposition\tid\tref\talt\tA\tC\tG\tT\tother\tdeleted\tlow_baseq\tref_count\talt_count"


def format_file(names, sites, meta, counts):
    """<sample>.allele_counts.tsv: one row per site in table order, position 1-based; ref_count is the column of REF, alt_count the sum of
    the columns of the distinct single-base A C G T entries of ALT's comma list that differ from REF."""
    out = [FILE_HEADER]
    for (tid, pos), (ident, ref, alt), row in zip(sites, meta, counts):
        r = base_code(ref)
        alts = []
        for a in alt.split(","):
            if len(a) == 1 and base_code(a) < 4 and base_code(a) != r and base_code(a) not in alts:
                alts.append(base_code(a))
        out.append("\t".join([names[tid], str(pos + 1), ident, ref, alt] + [str(v) for v in row] + [str(row[r]), str(sum(row[a] for a in alts))]))
    return "\n".join(out) + "\n"
