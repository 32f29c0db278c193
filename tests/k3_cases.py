"""Inputs shared by the edge tests of K3, the end-of-file coverage stage (CPU: tests/test_k3_edges_host.py -- the reference's own
Metrics.cpp, the oracle, the kernel on the wave emulation; device: tests/test_gpu_k3_edges.py): a named catalogue of small annotations
and reads aimed at the stage's class, depth and window edges -- coding lengths on both sides of every launch's LDS capacity, a depth on
both sides of the 16-bit cell, 64 / 65 exon rows per wave and round, the mask against the (trimmed) length, the window behind the peak,
the 5th-percentile trim and the two bias windows.

A gene is given as exon lengths, a strand and its coverage: per exon a list of (offset, length, depth) covers -- `depth` one-block reads
of `length` bases at exon offset `offset` -- or a PROFILE, the wanted depth of every transcript base, which covers_from_profile() turns
into covers (a read opens at every one-base step up and closes at every step down, so a profile that is strictly monotone in one-base
steps is a staircase of reads started, or ended, one base apart).  Every gene whose bias path is meant to run is strictly monotone inside
the windows it exercises: a window off by one base, or a median off by one rank, changes the result.

Expectations come from the oracle and the reference; HAND_* / Case.hand hold the few written down by hand from the reference's
source lines (src/Metrics.cpp:160-235,265-337; computeMedian, src/Metrics.h:147-160)."""
import functools
import math

import numpy as np

from rnaseqc_amd import abi
from rnaseqc_amd.model import Annotation, Batch

MAX_READ = 1000                  # longest read of a cover made from a profile; longer ones are cut into abutting reads
GAP = 10                         # bases between the exons of a gene (a read never touches the next exon)


# ---- builder -----------------------------------------------------------------------------------------------------------------------
def covers_from_profile(exon_lens, profile, max_len=MAX_READ):
    """Per exon the (offset, length, depth) covers whose sum is `profile` (depth per transcript base, exons stitched in order)."""
    profile = np.asarray(profile, np.int64)
    assert len(profile) == sum(exon_lens) and (len(profile) == 0 or profile.min() >= 0)
    out, a = [], 0
    for ln in exon_lens:
        step = np.diff(np.concatenate([[0], profile[a:a + ln], [0]]))
        a += ln
        open_, covers = [], []
        for i in np.flatnonzero(step).tolist():
            x = int(step[i])
            if x > 0:
                open_.append([i, x])
                continue
            need = -x
            while need:
                s, c = open_[-1]
                t = min(c, need)
                covers.append((s, i - s, t))
                need -= t
                if t == c:
                    open_.pop()
                else:
                    open_[-1][1] -= t
        assert not open_
        cut = []
        for s, l, c in covers:
            while l > max_len:
                cut.append((s, max_len, c)); s += max_len; l -= max_len
            cut.append((s, l, c))
        out.append(cut)
    return out


class Gene:
    def __init__(self, name, exons, strand="+", profile=None, covers=None):
        self.name, self.exons, self.strand = name, [int(x) for x in exons], strand
        self.profile = None if profile is None else np.asarray(profile, np.int64)
        if covers is None:
            covers = covers_from_profile(self.exons, self.profile) if profile is not None else [[] for _ in self.exons]
        assert len(covers) == len(self.exons)
        self.covers = covers
        self.coding = sum(self.exons)


class Input:
    """ann; batch: sorted, unpaired, one M block per read (run with unpaired=1); the inputs of binding.ref_coverage_run: geo
    (gene_exon_off), elen, gstrand, commits (exon row, offset, length, read) in file order."""
    pass


def build_input(genes):
    rows, elen, geo, gstrand = [], [], [0], []
    ex_row, ex_off, ex_len, ex_cnt, ex_start = [], [], [], [], []
    pos = 1_000
    for g in genes:
        lo = pos
        spans = []
        for ln in g.exons:
            spans.append((pos, pos + ln - 1))
            pos += ln + GAP
        rows.append(dict(contig="c", type="gene", start=lo, end=spans[-1][1], strand=g.strand, gene_id=g.name, gene_name=g.name))
        for k, (s, e) in enumerate(spans):
            row = len(elen)
            rows.append(dict(contig="c", type="exon", start=s, end=e, strand=g.strand, gene_id=g.name, exon_id="%s_e%d" % (g.name, k)))
            elen.append(e - s + 1)
            ex_start.append(s)
            for off, ln, depth in g.covers[k]:
                assert 0 <= off and ln >= 1 and off + ln <= e - s + 1 and depth >= 1
                ex_row.append(row); ex_off.append(off); ex_len.append(ln); ex_cnt.append(depth)
        geo.append(len(elen))
        gstrand.append({"+": 0, "-": 1, ".": 2}[g.strand])
        pos += 300
    inp = Input()
    inp.genes = genes
    inp.index = {g.name: i for i, g in enumerate(genes)}
    inp.lengths = [g.coding for g in genes]
    inp.ann = Annotation.from_rows(["c"], rows)
    assert inp.ann.coding_length[:len(genes)].tolist() == inp.lengths
    cnt = np.array(ex_cnt, np.int64)
    row = np.repeat(np.array(ex_row, np.int64), cnt); off = np.repeat(np.array(ex_off, np.int64), cnt); ln = np.repeat(np.array(ex_len, np.int64), cnt)
    start = np.array(ex_start, np.int64)[row] + off                          # 1-based
    order = np.lexsort((-ln, start))                                         # file order: by position, the longest of a position first
    row, off, ln, start = row[order], off[order], ln[order], start[order]
    n = len(row)
    assert n > 0 and span_maxima(ln) <= 32
    inp.n_reads = n
    inp.geo, inp.elen, inp.gstrand = geo, elen, gstrand
    inp.commits = np.stack([row, off, ln, np.arange(n, dtype=np.int64)], axis=1)
    qh = abi.qname_hash_bytes(np.frombuffer(b"".join(b"%015d" % i for i in range(n)), np.uint8).reshape(n, 15))
    p0 = (start - 1).astype(np.int32)
    inp.batch = Batch(pos=p0, mpos=p0.copy(), isize=np.zeros(n, np.int32), qhash=qh, cigar_off=np.arange(n, dtype=np.uint32),
                      flag=np.zeros(n, np.uint16), l_qseq=ln.astype(np.uint16), mapq=np.full(n, 255, np.uint8),
                      nm=np.zeros(n, np.uint8), tagbits=np.full(n, abi.TB_HAS_NM | abi.TB_MTID_SAME, np.uint8),
                      n_cigar=np.ones(n, np.uint8), cigar=((ln << 4) | abi.CIG_M).astype(np.uint32),
                      seg_tid=np.array([0], np.int32), seg_start=np.array([0, n], np.uint64),
                      wide_index=np.zeros(0, np.uint64), wide_nm=np.zeros(0, np.int32), wide_l_qseq=np.zeros(0, np.int32),
                      wide_n_cigar=np.zeros(0, np.uint32))
    return inp


def span_maxima(lengths):
    """Records longer than every record in front of them.  The Read-Length stage of a batch of mixed read lengths keeps one walk per such
    record, 128 at the most (RSQC_ERR_CAPACITY): the inputs here stay far below, in every batch they are cut into."""
    lengths = np.asarray(lengths, np.int64)
    return int((lengths > np.concatenate([[0], np.maximum.accumulate(lengths)[:-1]])).sum())


def three_batches(batch):
    """The batch cut into three unequal parts (a seventh, four sevenths, two sevenths of the records)."""
    n = batch.n
    a, b = max(1, n // 7), max(2, (5 * n) // 7)
    parts = [batch.slice(0, a), batch.slice(a, b), batch.slice(b, n)]
    assert all(span_maxima(p.l_qseq) <= 32 for p in parts)
    return parts


# the eight launches of the stage in launch order (rsqc_k3_plan.h), restated by hand: (threads, LDS capacity)
LAUNCHES = ((1024, 73_000), (256, 12_288), (256, 6_144), (1024, 32_768), (64, 4_096), (64, 3_072), (64, 2_048), (64, 1_024))


def launch_of(coding):
    """The launch a gene of `coding` bases belongs to: the smallest capacity of its thread class (one wave up to 4 096 bases, 256
    threads up to 12 288, 1024 threads beyond; the 146 KB instance also takes what no capacity holds)."""
    for k in (7, 6, 5, 4, 2, 1, 3):
        if coding <= LAUNCHES[k][1]:
            return k
    return 0


def launches_of(lengths):
    out = [0] * 8
    for c in lengths:
        out[launch_of(c)] += 1
    return out


# ---- profiles ----------------------------------------------------------------------------------------------------------------------
def up(n, lo, step=1):
    return lo + step * np.arange(n, dtype=np.int64)


def down(n, hi, step=1):
    return hi - step * np.arange(n, dtype=np.int64)


def bias_profile(coding, salt=0, lo=101, hi=300):
    """Two rising staircases, lo .. at the 5' end of the transcript vector and .. hi at its 3' end (150 bases each, or half the gene),
    a low blocky middle (1 .. 5, 64 bases a level): the peak is the last base, the gate behind it opens, the 5th percentile trims
    nothing off a long gene, and both default windows lie inside a staircase with different medians."""
    front = min(150, coding // 2)
    back = min(150, coding - front)
    p = np.zeros(coding, np.int64)
    p[:front] = up(front, lo)
    p[coding - back:] = up(back, hi - back + 1)
    m = coding - front - back
    if m > 0:
        p[front:front + m] = 1 + ((np.arange(m) // 64 + salt) % 5)
    return p


def two_exons(coding):
    return [coding // 3, coding - coding // 3]


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
INPUTS = {}                      # name -> (builder, the genes per launch the input was built for)


def _input(launches):
    def deco(fn):
        INPUTS[fn.__name__.lstrip("_")] = (fn, launches)
        return fn
    return deco


@functools.lru_cache(maxsize=None)
def get_input(name):
    fn, launches = INPUTS[name]
    inp = build_input(fn())
    inp.name = name
    inp.launches = list(launches)
    assert launches_of(inp.lengths) == inp.launches, (name, inp.lengths, launches_of(inp.lengths))
    return inp


CLASS_BOUNDS = (1024, 1025, 2048, 2049, 3072, 3073, 4096, 4097, 6144, 6145, 12288, 12289)


@_input([0, 2, 2, 1, 2, 2, 2, 1])
def _class_bounds():
    return [Gene("b%d" % c, two_exons(c), "+-"[k % 2], profile=bias_profile(c, salt=k)) for k, c in enumerate(CLASS_BOUNDS)]


def _long_exons(coding):
    ex = []
    for ln in (10_000, 9_000, 8_000, 10_000, 7_000, 10_000, 6_000, 10_000):
        if coding - sum(ex) > ln + 4_000:
            ex.append(ln)
    rest = coding - sum(ex)
    return ex + ([rest] if rest <= 10_000 else [rest - 5_000, 5_000])


@_input([3, 0, 0, 1, 0, 0, 0, 0])
def _lds16_bounds():
    genes = [Gene("l%d" % c, _long_exons(c), "-+"[k % 2], profile=bias_profile(c, salt=k)) for k, c in enumerate((32768, 32769, 73000, 73001))]
    assert all(4_000 <= e <= 10_000 for g in genes for e in g.exons)
    return genes


def _depth_genes(peak):
    """20 kb in five exons; on the third exon a staircase 201 .. 600 of 400 bases whose 200th base (depth 400) is raised to `peak`.  The
    gate (the base in front of the peak: 399) opens, the percentile (221) leaves 379 bases, both windows lie on the staircase."""
    p = np.zeros(20_000, np.int64)
    p[8_000:8_400] = up(400, 201)
    p[8_199] = peak
    shallow = np.zeros(20_000, np.int64)
    shallow[:] = 1 + (np.arange(20_000) // 512) % 4
    return [Gene("deep", [4_000] * 5, "+", profile=p), Gene("shallow", [4_000] * 5, "-", profile=shallow)]


@_input([0, 0, 0, 2, 0, 0, 0, 0])
def _depth_65535():
    return _depth_genes(65_535)


@_input([0, 0, 0, 2, 0, 0, 0, 0])
def _depth_65536():
    return _depth_genes(65_536)


@_input([0, 0, 0, 0, 0, 0, 0, 1])
def _plan_one_1024():
    return [Gene("only", two_exons(1024), "+", profile=bias_profile(1024))]


@_input([0, 0, 0, 1, 0, 0, 0, 0])
def _plan_one_12289():
    return [Gene("only", two_exons(12289), "-", profile=bias_profile(12289))]


@_input([0, 0, 0, 0, 0, 20, 0, 0])
def _plan_ties_3072():
    return [Gene("t%d" % k, two_exons(3072), "+-"[k % 2], profile=bias_profile(3072, salt=k, lo=101 + k, hi=300 - 2 * k)) for k in range(20)]


@_input([0, 1, 3, 1, 0, 0, 0, 0])
def _plan_none_small():
    return [Gene("n%d" % c, two_exons(c), "+-"[k % 2], profile=bias_profile(c, salt=k)) for k, c in enumerate((6144, 13000, 4097, 6145, 5000))]


@_input([0, 0, 0, 0, 0, 0, 0, 5])
def _plan_all_small():
    return [Gene("s%d" % k, two_exons(c), "+-"[k % 2], profile=bias_profile(c, salt=k)) for k, c in enumerate((1000, 200, 1024, 600, 1024))]


@_input([3, 3, 3, 3, 3, 3, 3, 3])
def _plan_zero_between():
    """Three genes per launch; the middle one by length has no read (the early exit), its neighbours in the launch are covered.  Laid
    out along the contig in an order that is not the order by length."""
    trio = [(33_000, 32_900, 32_800), (13_000, 12_900, 12_800), (7_000, 6_900, 6_800), (5_000, 4_900, 4_800), (3_500, 3_400, 3_300),
            (2_500, 2_400, 2_300), (1_500, 1_400, 1_300), (900, 800, 700)]
    genes = []
    for j in (1, 2, 0):
        for k, t in enumerate(trio if j != 2 else trio[::-1]):
            c = t[j]
            ex = _long_exons(c) if c > 20_000 else two_exons(c)
            genes.append(Gene("z%d" % c, ex, "+-"[(k + j) % 2], profile=None if j == 1 else bias_profile(c, salt=k + j)))
    return genes


def _exon_pattern(k, ln):
    a = 1 + (k * 7) % 11                     # differs between exon k and k + 1, k + 64, k + 256, k + 1024
    if ln == 5:
        return [a, a + 1, a + 2, a + 1, a]
    if ln == 3:
        return [a, a + 1, a]
    return [a + (j % 3) for j in range(ln)]


@_input([0, 0, 2, 0, 1, 0, 0, 3])
def _exon_rounds():
    genes = []
    for name, nex, ln, strand in (("x63", 63, 5, "+"), ("x64", 64, 5, "-"), ("x65", 65, 5, "+"), ("x256", 256, 20, "-"), ("x257", 257, 20, "+"),
                                  ("x1025", 1025, 3, "-")):
        genes.append(Gene(name, [ln] * nex, strand, profile=np.concatenate([_exon_pattern(k, ln) for k in range(nex)])))
    return genes


@_input([0, 0, 0, 0, 0, 0, 0, 6])
def _mask_edges():
    low = 10 + (np.arange(600) * 7) % 13                                    # the gate stays shut: [v0, v1) is the whole gene
    # `flank`: 100 bases at 5x in front of a staircase 101 .. 700; the 5th percentile (order statistic 35 of 700) is 5, the flank is
    # trimmed and the 600 bases left, not the 700 coding ones, meet 2 x mask
    flank = np.concatenate([np.full(100, 5), up(600, 101)])
    body = 20 + (np.arange(300) * 5) % 17
    return [Gene("m600", [250, 350], "+", profile=low),
            Gene("m600z", [250, 350], "-"),                                # no read: the early exit's own test against 2 x mask
            Gene("flank", [300, 400], "+", profile=flank),
            Gene("short_ends", [5, 300, 4], "-", profile=np.concatenate([[3, 4, 5, 4, 3], body, [2, 3, 4, 5]])),   # mask 7 swallows both end exons
            Gene("one_base", [8, 300, 8], "+", profile=np.concatenate([up(8, 3), body, down(8, 12)])),     # mask 7 leaves one base of each end exon
            Gene("plain", [700], "-", profile=bias_profile(700))]


# the gate, src/Metrics.cpp:164-181: peak_pos = FIRST maximum; the cursor goes W/2 to the right (stops at end()), then W back (stops at
# begin()) counting n entries; the "median" is computeMedian(n, cursor) on the UNSORTED vector: entry cursor + (n-1)/2, averaged with the
# next one when n is odd (n == 1: the cursor's entry; n == 0: range_error)
def gate_reads(pp, window, coding):
    pos = min(pp + window // 2, coding)
    n = min(window, pos)
    cur = pos - n
    if n == 0:
        return []
    if n == 1:
        return [cur]
    mid = (n - 1) // 2
    return [cur + mid, cur + mid + 1] if n % 2 else [cur + mid]


GATE_CODING = 300
GATE_KINDS = ("peak0", "peak_last", "twin", "near_start", "near_end")
GATE_WINDOWS = (1, 2, 3, 100, 101)


def gate_shape(kind):
    """(shape, first peak): one-base steps everywhere the gate can read; the profile is shape + a level.  `twin`: two equal peaks at 80 and
    220, the second with three-base steps in front of it: would the LAST maximum win, the gate would read two lower."""
    i = np.arange(GATE_CODING, dtype=np.int64)
    if kind == "peak0":
        return -i, 0
    if kind == "peak_last":
        return -(GATE_CODING - 1 - i), GATE_CODING - 1
    if kind == "near_start":
        return -np.abs(i - 20), 20
    if kind == "near_end":
        return -np.abs(i - 285), 285
    s = np.where(i <= 185, -np.abs(i - 80), np.where(i < 220, -3 * (220 - i), -(i - 220)))
    return s, 80


def gate_gene(kind, window, opens):
    """The gate of this gene reads exactly 100 (odd n: 100.5) and opens, or 99 (odd n: 99.5: neighbours 99 and 100) and stays shut."""
    shape, pp = gate_shape(kind)
    at = gate_reads(pp, window, GATE_CODING)
    level = (100 if opens else 99) - int(shape[at[0]])          # shape rises by one from at[0] to at[1] or falls by one
    if len(at) == 2 and shape[at[1]] < shape[at[0]]:
        level += 1
    p = np.maximum(shape + level, 3)
    want = (100.5 if opens else 99.5) if len(at) == 2 else (100 if opens else 99)
    assert sum(int(p[j]) for j in at) / len(at) == want and int(np.argmax(p)) == pp
    return Gene("%s_%s" % (kind, "open" if opens else "shut"), [120, 180], "+-"[opens], profile=p)


def _gate_input(window):
    def build():
        kinds = [k for k in GATE_KINDS if not (k == "peak0" and window == 1)]
        return [gate_gene(k, window, o) for k in kinds for o in (True, False)]
    return build


for _w in GATE_WINDOWS:
    INPUTS["gate_w%d" % _w] = (_gate_input(_w), [0, 0, 0, 0, 0, 0, 0, 8 if _w == 1 else 10])


@_input([0, 0, 0, 0, 0, 0, 0, 2])
def _gate_peak0():
    """Peak at base 0 under window 1: the cursor moves 0 to the right and 0 back: computeMedian of nothing, range_error."""
    p = np.maximum(down(GATE_CODING, 400), 3)
    return [Gene("peak0", [120, 180], "+", profile=p), Gene("beside", [300], "-", profile=bias_profile(300))]


def stairs(coding, lo=101):
    return up(coding, lo)


@_input([0, 0, 0, 0, 0, 0, 0, 7])
def _trim_edges():
    return [Gene("flat", [120, 180], "+", profile=np.full(300, 150)),                      # everything <= the percentile: trimmed to nothing
            Gene("nnz300", [120, 180], "-", profile=stairs(300)),                          # 300 x 0.05 = 15
            Gene("nnz310", [130, 180], "+", profile=stairs(310)),                          # 310 x 0.05 = 15.5 -> 15
            Gene("holes", [150, 100, 150], "-", profile=np.concatenate([up(150, 101), np.zeros(100, np.int64), up(150, 251)])),
            Gene("tlen200", [100, 111], "+", profile=stairs(211)),                         # 211 - (10 + 1) = 200 = bias_gene_length
            Gene("tlen199", [100, 110], "+", profile=stairs(210)),                         # 210 - (10 + 1) = 199
            Gene("tlen200r", [100, 111], "-", profile=stairs(211))]


@_input([0, 0, 0, 0, 0, 0, 0, 2])
def _trim_radix3():
    """A one-wave (32-bit) gene whose maximum is 70 000 (top byte: 2) and whose 5th percentile is 291 = 0x0123: three radix passes, a
    non-zero digit in each of the last two."""
    p = up(300, 276)
    p[200] = 70_000
    return [Gene("radix3", [120, 180], "+", profile=p), Gene("beside", [300], "-", profile=bias_profile(300))]


WINDOW_TLEN = 379                # 400 bases 101 .. 500: order statistic 20 is 121, 21 leading bases go


@_input([0, 0, 0, 0, 0, 0, 0, 5])
def _window_edges():
    # pairs of equal depths: ties inside every window.  402 bases: order statistic 20 is 131, 22 bases go, 380 stay (no shorter than WINDOW_TLEN)
    ties = 101 + np.arange(402, dtype=np.int64) // 2 * 3
    return [Gene("fwd", [150, 250], "+", profile=stairs(400)), Gene("rev", [150, 250], "-", profile=stairs(400)),
            Gene("uns", [150, 250], ".", profile=stairs(400)), Gene("ties", [150, 252], "+", profile=ties),
            Gene("ties_r", [252, 150], "-", profile=ties[::-1].copy())]


WIDE_TLEN = 2089                 # 2200 bases 101 .. 2300: order statistic 110 is 211, 111 leading bases go


@_input([0, 0, 0, 0, 0, 2, 0, 0])
def _window_wide():
    """... and, falling, 2300 .. 101 on the reverse strand: the 111 bases go at the back, the peak is base 0."""
    return [Gene("wfwd", [1200, 1000], "+", profile=stairs(2200)), Gene("wrev", [1000, 1200], "-", profile=down(2200, 2300))]


# ---- cases -------------------------------------------------------------------------------------------------------------------------
ALL_FORCES = (1, 2, 3, 4)


class Case:
    """One run: an input under parameters.  error: every leg ends in ERR_EMPTY_MEDIAN.  forces: the forced configurations of the
    emulation the case also runs under (force=0, the library's plan, always runs).  hand: {gene: expected values written by hand}."""
    def __init__(self, name, input_name, kw=None, error=False, forces=ALL_FORCES, hand=None):
        self.name, self.input_name, self.kw, self.error, self.forces, self.hand = name, input_name, dict(kw or {}), error, tuple(forces), hand or {}

    @property
    def input(self):
        return get_input(self.input_name)

    def params(self):
        return abi.default_params(unpaired=1, **self.kw)


def _sd(n):
    """Population standard deviation of n consecutive integers."""
    return math.sqrt((n * n - 1) / 12.0)


# ---- by hand: `fwd` / `rev` of window_edges, depths 101 + i, i < 400, mask 0.  Peak: the last base.  Gate (W = 100): cursor at end(), 100
# back to 300, entry 300 + 49 = 450 >= 100.  400 non-zero depths, 400 x 0.05 = 20: lowerLimit = sorted[20] = 121; the 21 leading bases
# <= 121 go, nothing at the back: 379 bases 122 .. 500, mean 311.  Windows of 100: left 122 .. 221 -> entry 49 = 171, right 401 .. 500 -> 450;
# of 127 (odd): left 122 .. 248 -> (185 + 186) / 2 = 185.5, right 374 .. 500 -> 437.5, truncated when added to the unsigned long sums.
# A forward gene adds the right window to its 3' sum; a reverse or unstranded one the left.
_H_STAT = dict(valid=1, mean=311.0, std=_sd(379))
HAND_WINDOW_100 = {"fwd": dict(three=450, five=171, **_H_STAT), "rev": dict(three=171, five=450, **_H_STAT), "uns": dict(three=171, five=450, **_H_STAT)}
HAND_WINDOW_127 = {"fwd": dict(three=437, five=185, **_H_STAT), "rev": dict(three=185, five=437, **_H_STAT)}
# W + OFF == tlen (100 + 279): the right window starts at 0: 122 .. 221 -> 171; the left is [279, 379): 401 .. 500 -> 450
HAND_WINDOW_FIT = {"fwd": dict(three=171, five=450, **_H_STAT)}
# ---- by hand: trim_edges, mask 0.  `tlen200`: depths 101 + i, i < 211; 211 x 0.05 = 10.55 -> sorted[10] = 111, 11 bases go, 200 stay
# (112 .. 311, mean 211.5): left 112 .. 211 -> 161, right 212 .. 311 -> 261.  `tlen199`: 210 x 0.05 = 10.5 -> 111 again, 199 stay (112 .. 310):
# shorter than bias_gene_length, no bias, but the statistics are those of the trimmed vector.  `flat`: all 300 bases <= 150: nothing stays.
HAND_TRIM = {"tlen200": dict(valid=1, mean=211.5, std=_sd(200), three=261, five=161),
             "tlen200r": dict(valid=1, mean=211.5, std=_sd(200), three=161, five=261),
             "tlen199": dict(valid=1, mean=211.0, std=_sd(199), three=0, five=0),
             "flat": dict(valid=0, three=0, five=0)}
# ---- by hand: gate_w100, `peak_last`.  shape -(299 - i); the gate reads entry 200 + 49 = 249, shape -50.  open: level 150: depths
# max(i - 149, 3): 3 on bases 0 .. 152, then 4 .. 150; gate 100: lowerLimit = sorted[15] = 3, bases 0 .. 152 go, 147 stay (4 .. 150, mean 77):
# shorter than 200, no bias.  shut: level 149: 3 on bases 0 .. 153, then 4 .. 149; gate 99: untrimmed, mean (154 x 3 + 11169) / 300.
_SHUT = np.concatenate([np.full(154, 3), np.arange(4, 150)])
HAND_GATE_100 = {"peak_last_open": dict(valid=1, mean=77.0, std=_sd(147), three=0, five=0),
                 "peak_last_shut": dict(valid=1, mean=11631 / 300.0, std=float(np.sqrt(np.mean((_SHUT - 11631 / 300.0) ** 2))), three=0, five=0)}

CASES = []


def _case(*a, **k):
    CASES.append(Case(*a, **k))


_case("class_bounds-mask0", "class_bounds", dict(coverage_mask=0))
_case("class_bounds-mask500", "class_bounds", dict(coverage_mask=500), forces=())
# the three long inputs run under the library's plan and the ONE forced configuration that changes their mode: the 64 KB instance for
# lds16_bounds (all four genes in memory), the 146 KB instance for the depth cases (the same 16-bit decision in the other instance);
# left out: forces 1, 3, 4 for lds16_bounds, forces 2, 3, 4 for the depth cases
_case("lds16_bounds", "lds16_bounds", dict(coverage_mask=500), forces=(2,))
_case("depth_65535", "depth_65535", dict(coverage_mask=0), forces=(1,))
_case("depth_65536", "depth_65536", dict(coverage_mask=0), forces=(1,))
_case("plan_degenerate-one_1024", "plan_one_1024", dict(coverage_mask=0))
_case("plan_degenerate-one_12289", "plan_one_12289", dict(coverage_mask=500))
_case("plan_degenerate-ties_3072", "plan_ties_3072", dict(coverage_mask=500), forces=(3,))
_case("plan_degenerate-none_small", "plan_none_small", dict(coverage_mask=0))
_case("plan_degenerate-all_small", "plan_all_small", dict(coverage_mask=100))
_case("plan_degenerate-zero_between-mask0", "plan_zero_between", dict(coverage_mask=0), forces=())
_case("plan_degenerate-zero_between-mask500", "plan_zero_between", dict(coverage_mask=500), forces=(2,))
_case("exon_rounds-mask0", "exon_rounds", dict(coverage_mask=0))
_case("exon_rounds-mask7", "exon_rounds", dict(coverage_mask=7))
for _m in (7, 299, 300, 301):
    _case("mask_edges-mask%d" % _m, "mask_edges", dict(coverage_mask=_m), forces=ALL_FORCES if _m in (7, 300) else ())
for _w in GATE_WINDOWS:
    _case("gate_edges-w%d" % _w, "gate_w%d" % _w, dict(coverage_mask=0, bias_window=_w), forces=ALL_FORCES if _w in (1, 101) else (4,),
          hand=HAND_GATE_100 if _w == 100 else None)
_case("gate_edges-peak0-w1", "gate_peak0", dict(coverage_mask=0, bias_window=1), error=True)
_case("gate_edges-peak0-w2", "gate_peak0", dict(coverage_mask=0, bias_window=2), forces=())
_case("trim_edges-mask0", "trim_edges", dict(coverage_mask=0), hand=HAND_TRIM)
_case("trim_edges-mask50", "trim_edges", dict(coverage_mask=50), forces=())
_case("trim_edges-radix3", "trim_radix3", dict(coverage_mask=0))
_case("window_edges-w100", "window_edges", dict(coverage_mask=0), hand=HAND_WINDOW_100)
_case("window_edges-fit", "window_edges", dict(coverage_mask=0, bias_offset=WINDOW_TLEN - 100), hand=HAND_WINDOW_FIT)            # W + OFF == tlen
_case("window_edges-fit_plus1", "window_edges", dict(coverage_mask=0, bias_offset=WINDOW_TLEN - 99), error=True, forces=(4,))   # == tlen + 1
_case("window_edges-short_left", "window_edges", dict(coverage_mask=0, bias_offset=300), error=True, forces=(3,))                # OFF + W > tlen > OFF
_case("window_edges-offset_is_tlen", "window_edges", dict(coverage_mask=0, bias_offset=WINDOW_TLEN), error=True, forces=())
_case("window_edges-w127", "window_edges", dict(coverage_mask=0, bias_window=127), hand=HAND_WINDOW_127)
_case("window_edges-w128", "window_edges", dict(coverage_mask=0, bias_window=128, bias_offset=7), forces=(4,))
_case("window_edges-w129", "window_edges", dict(coverage_mask=0, bias_window=129, bias_offset=7))                # the first wide window
_case("window_edges-w3", "window_edges", dict(coverage_mask=0, bias_window=3, bias_offset=50), forces=())
_case("window_wide-w1023", "window_wide", dict(coverage_mask=500, bias_window=1023))
_case("window_wide-w1024", "window_wide", dict(coverage_mask=0, bias_window=1024), forces=(3,))
_case("window_wide-w1024-fit", "window_wide", dict(coverage_mask=0, bias_window=1024, bias_offset=WIDE_TLEN - 1024), forces=(4,))
_case("window_wide-w1024-fit_plus1", "window_wide", dict(coverage_mask=0, bias_window=1024, bias_offset=WIDE_TLEN - 1023), error=True, forces=())

CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)
