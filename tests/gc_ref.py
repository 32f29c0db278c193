"""The --fasta statistics restated plainly (Python and numpy, none of the project's C): the GC content of a sequence
(src/Fasta.cpp:67-74), the per-exon GC that exon_gc_kernel documents (src/Metrics.cpp:299-303 for EVERY exon row, covered or not)
and the replay of the fragment map of src/Expression.cpp:461-476 over candidates in file order, with the clipping that
oracle/rsqc_oracle.c documents in get_seq.  Whole-path expectations come from the oracle; this module serves where the oracle
cannot: candidate-level tests, and exon_gc of exons without coverage."""
import numpy as np

GC_BINS = 100
_GC = frozenset(b"GgCc")


def gc_fraction(seq_bytes):
    """gc(): 1.0/len added once per G g C c base, in sequence order, with Python floats (IEEE doubles); -1 for an empty sequence."""
    seq = bytes(seq_bytes)
    if not seq:
        return -1.0
    inc = 1.0 / float(len(seq))
    c = 0.0
    for ch in seq:
        if ch in _GC:
            c += inc
    return c


def gc_of(k, size):
    """gc_fraction of any sequence of `size` bases of which k are G/C (the sum does not depend on where they are)."""
    inc = 1.0 / float(size)
    c = 0.0
    for _ in range(k):
        c += inc
    return c


def bin_of(value):
    """src/RNASeQC.cpp:368: the slot of gcBins[100]; GC_BINS = out of range (a sum that reaches 1.0)."""
    b = int(value * 100.0)
    return b if b < GC_BINS else GC_BINS


def sequences(reference):
    """contig id -> bytes, for the contigs the FASTA names."""
    return {int(k): bytes(np.asarray(s, np.uint8)) for k, s in zip(reference.contig, reference.sequence)}


def get_seq(seqs, contig, start, end):
    """Fasta::getSeq for 0-based [start, end): clipped at the contig's end; b"" where the reference leaves its defined paths
    (contig absent, start < 0, start at or behind the end of the contig, an empty range)."""
    s = seqs.get(int(contig))
    if s is None or start < 0 or start >= len(s) or end <= start:
        return b""
    return s[start:min(end, len(s))]


def exon_gc(ann, reference):
    """By exon id: -1 when the FASTA lacks the contig or the start lies outside it (start < 0, start >= L); otherwise the GC of
    the bases [start, min(start + length, L)) -- the 1-based start used as a 0-based offset."""
    seqs = sequences(reference)
    out = np.full(ann.n_exons, -1.0, np.float64)
    for row in range(ann.n_exons):
        start, end = int(ann.exon_row_start[row]), int(ann.exon_row_end[row])
        seq = get_seq(seqs, int(ann.exon_row_contig[row]), start, start + (end - start + 1))
        out[int(ann.exon_row_id[row])] = gc_fraction(seq)
    return out


def replay(candidates_in_file_order, reference):
    """candidates: dicts with name (anything hashable), row, endpos, l_qseq, moved (pos != mpos), tid -- the records that reach
    src/Expression.cpp:459 -- in file order.  Returns (the 100 bins, out_of_range)."""
    seqs = sequences(reference)
    bins = np.zeros(GC_BINS, np.uint64)
    oob = 0
    fragments = {}
    for c in candidates_in_file_order:
        stored = fragments.get(c["name"])
        if stored is None:                                              # :462-466
            fragments[c["name"]] = (c["row"], c["endpos"])
            continue
        if stored[0] != c["row"]:                                       # :467
            continue
        if c["endpos"] <= stored[1] or not c["moved"]:                  # :471 (the entry stays)
            continue
        seq = get_seq(seqs, c["tid"], stored[1] - c["l_qseq"], c["endpos"])   # :473
        del fragments[c["name"]]                                        # :474
        if seq:                                                         # :475
            b = bin_of(gc_fraction(seq))
            if b < GC_BINS:
                bins[b] += 1
            else:
                oob += 1
    return bins, oob
