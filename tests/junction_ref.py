"""The contract of --junctions (include/rnaseqc_amd.h, rsqc_junction_table) restated as a plain Python loop over Batch columns: the
expected table of every junction test comes from here, never from the code under test.

population   (flag & (0x4 | 0x100 | 0x200 | 0x800)) == 0 and the segment's tid in [0, n_contigs); nothing else gates a record
walk         p = pos; an N of length L >= 1 is the instance (tid, p + 1, p + L) unless p + L > 2^31 - 1; M D N = X advance p
overhang     min(left, right): the M = X lengths between the previous N (of any length, or the record's start) and this N, and from
             this N to the next N (or the record's end)
table        one row per distinct (tid, start, end), ascending: reads, hq_reads (mapq >= mapq_threshold), max_overhang
known        some gene has, on that contig, an exon that ends at start - 1 and an exon that starts at end + 1
"""
import numpy as np

from rnaseqc_amd import abi

EXCLUDED = 0x4 | 0x100 | 0x200 | 0x800
INT_MAX = (1 << 31) - 1
HEADER = "contig\tstart\tend\treads\thq_reads\tmax_overhang\tknown\n"


def record_ops(batch, i):
    """The operations of record i as (op, length) pairs; a wide record's true count comes from the wide table."""
    n = int(batch.n_cigar[i])
    if n == abi.NCIGAR_ESCAPE:
        hit = np.flatnonzero(np.asarray(batch.wide_index) == i)
        n = int(batch.wide_n_cigar[hit[0]]) if len(hit) else 0
    off = int(batch.cigar_off[i])
    return [(int(w) & 15, int(w) >> 4) for w in batch.cigar[off:off + n]]


def record_instances(tid, pos, ops):
    """[(tid, start, end, overhang)] of one contributing record."""
    p, cur = int(pos), 0
    blocks, found = [], []                      # aligned bases of every block between two N; (start, end, index of the block in front)
    for op, ln in ops:
        if op == abi.CIG_N:
            blocks.append(cur); cur = 0
            if ln >= 1 and p + ln <= INT_MAX:
                found.append((p + 1, p + ln, len(blocks) - 1))
            p += ln
        elif op in (abi.CIG_M, abi.CIG_EQ, abi.CIG_X):
            cur += ln; p += ln
        elif op == abi.CIG_D:
            p += ln
    blocks.append(cur)
    return [(tid, s, e, min(blocks[k], blocks[k + 1], INT_MAX)) for s, e, k in found]


def junction_table(batches, n_contigs, mapq_threshold=255):
    """The table of the records of `batches` (any order, any cut) as a dict of numpy arrays + scalars; also what the fixture
    checks ask for: N operations seen in contributing and in excluded records."""
    rows = {}
    population = instances = n_ops = n_ops_excluded = records = 0
    for b in batches:
        tids = b.tid_per_record()
        for i in range(b.n):
            records += 1
            ops = record_ops(b, i)
            n_here = sum(1 for op, _ in ops if op == abi.CIG_N)
            tid = int(tids[i])
            if (int(b.flag[i]) & EXCLUDED) or tid < 0 or tid >= n_contigs:
                n_ops_excluded += n_here
                continue
            population += 1
            n_ops += n_here
            hq = 1 if int(b.mapq[i]) >= mapq_threshold else 0
            for t, s, e, ov in record_instances(tid, int(b.pos[i]), ops):
                instances += 1
                r = rows.setdefault((t, s, e), [0, 0, 0])
                r[0] += 1; r[1] += hq; r[2] = max(r[2], ov)
    keys = sorted(rows)
    col = lambda k, dt: np.array([x[k] for x in keys], dt).reshape(len(keys))
    val = lambda k: np.array([rows[x][k] for x in keys], np.uint32).reshape(len(keys))
    return dict(n=len(keys), instances=instances, population=population, records=records, n_ops=n_ops, n_ops_excluded=n_ops_excluded,
                tid=col(0, np.int32), start=col(1, np.int32), end=col(2, np.int32), reads=val(0), hq_reads=val(1), max_overhang=val(2))


COLUMNS = ("tid", "start", "end", "reads", "hq_reads", "max_overhang")


def assert_tables_equal(got, want):
    assert got["n"] == want["n"], (got["n"], want["n"])
    assert got["instances"] == want["instances"] and got["population"] == want["population"], (got["instances"], want["instances"], got["population"], want["population"])
    for f in COLUMNS:
        assert np.array_equal(np.asarray(got[f]).astype(np.int64), np.asarray(want[f]).astype(np.int64)), f


def known_flags(ann, table):
    """The `known` column from an Annotation (exon rows with their gene ids)."""
    ends, starts = {}, {}
    for k in range(len(ann.exon_row_contig)):
        c, g = int(ann.exon_row_contig[k]), int(ann.exon_row_gene[k])
        ends.setdefault((c, int(ann.exon_row_end[k])), set()).add(g)
        starts.setdefault((c, int(ann.exon_row_start[k])), set()).add(g)
    out = []
    for t, s, e in zip(table["tid"], table["start"], table["end"]):
        out.append(1 if ends.get((int(t), int(s) - 1), set()) & starts.get((int(t), int(e) + 1), set()) else 0)
    return np.array(out, np.uint8)


def render(table, contig_names, known):
    """<sample>.junctions.tsv as the command line writes it."""
    lines = [HEADER]
    for k in range(table["n"]):
        lines.append("%s\t%d\t%d\t%d\t%d\t%d\t%d\n" % (contig_names[int(table["tid"][k])], table["start"][k], table["end"][k], table["reads"][k],
                                                    table["hq_reads"][k], table["max_overhang"][k], known[k]))
    return "".join(lines)
