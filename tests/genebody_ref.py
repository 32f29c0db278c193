"""The contract of --gene-body (include/rnaseqc_amd.h, rsqc_genebody_info; rnaseqc_amd/csrc/rsqc_genebody.h) restated with numpy: the
expected sums, figures and text of every gene-body test come from here, never from the code under test.

model        gene g's segments are rows [seg_off[g], seg_off[g + 1]) of (seg_tid, seg_start, seg_end), 0-based, end exclusive, on one
             contig, inside it, non-empty, ascending and disjoint; one `reverse` byte per gene; L = the sum of the segment lengths
coordinate   u = the model bases in front of a position; t = u, or L - 1 - u for a reverse gene; bin = floor(t * 100 / L)
sums         sum[g][k] = the total depth over the positions of gene g in bin k; genes with L < 100 are not measured (zeroes)
file         bin, depth_sum (over the measured genes), genes (eligible: L >= 100 and total depth >= L), norm_mean (the mean over the
             eligible genes, in gene order, of (sum[g][k] / len_k) / (total_g / L), len_k = ceil((k + 1) L / 100) - ceil(k L / 100))
"""
import numpy as np

from rnaseqc_amd import abi

BINS = 100
INFO = ("n_genes", "n_measured", "model_bases", "depth_sum")


def make_model(genes):
    """genes: [(tid, [(start, end), ...], reverse)] -> the model's columns."""
    off, tid, start, end, rev = [0], [], [], [], []
    for t, segs, r in genes:
        for s, e in segs:
            tid.append(t); start.append(s); end.append(e)
        off.append(len(tid)); rev.append(1 if r else 0)
    return dict(seg_off=np.array(off, np.uint32), seg_tid=np.array(tid, np.int32), seg_start=np.array(start, np.uint32), seg_end=np.array(end, np.uint32),
                reverse=np.array(rev, np.uint8))


def gene_lengths(model):
    ln = (model["seg_end"].astype(np.int64) - model["seg_start"].astype(np.int64))
    c = np.concatenate(([0], np.cumsum(ln)))
    off = model["seg_off"].astype(np.int64)
    return c[off[1:]] - c[off[:-1]]


def model_from_annotation(ann, lengths):
    """The command line's rule: the listed genes' exon rows on the contig of the gene's first exon row (if the header has it), from
    1-based closed to 0-based half-open, clipped to [0, LN), overlapping and abutting rows merged; reverse: that first row's strand."""
    genes = []
    for g in range(ann.n_genes_listed):
        rows = [int(r) for r in ann.gene_exon_row[int(ann.gene_exon_off[g]):int(ann.gene_exon_off[g + 1])]]
        if not rows or int(ann.exon_row_contig[rows[0]]) >= min(ann.n_ref, len(lengths)):
            genes.append((0, [], False)); continue
        tid = int(ann.exon_row_contig[rows[0]])
        ivs = sorted((max(int(ann.exon_row_start[r]) - 1, 0), min(int(ann.exon_row_end[r]), int(lengths[tid]))) for r in rows if int(ann.exon_row_contig[r]) == tid)
        segs = []
        for s, e in ivs:
            if e <= s:
                continue
            if segs and s <= segs[-1][1]:
                segs[-1][1] = max(segs[-1][1], e)
            else:
                segs.append([s, e])
        genes.append((tid, [tuple(x) for x in segs], (int(ann.exon_row_flags[rows[0]]) & 3) == abi.STRAND_REVERSE))
    return make_model(genes)


def depth_arrays(track, lengths):
    """The depth of every position from the rows of tests/track_ref.py's track: one int64 array per contig."""
    depth = [np.zeros(int(n), np.int64) for n in lengths]
    for t, s, e, d in zip(track["tid"], track["start"], track["end"], track["depth"]):
        depth[int(t)][int(s):int(e)] = int(d)
    return depth


def sums(depth, model):
    """(sums [n_genes, 100] as uint64, info)."""
    n = len(model["reverse"])
    out = np.zeros((n, BINS), np.uint64)
    L = gene_lengths(model)
    for g in range(n):
        if L[g] < BINS:
            continue
        lo, hi = int(model["seg_off"][g]), int(model["seg_off"][g + 1])
        d = np.concatenate([depth[int(model["seg_tid"][k])][int(model["seg_start"][k]):int(model["seg_end"][k])] for k in range(lo, hi)])
        if model["reverse"][g]:
            d = d[::-1]                                                # (in the order of t)
        b = np.arange(int(L[g]), dtype=np.int64) * BINS // int(L[g])     # ascending in t
        edge = np.searchsorted(b, np.arange(BINS + 1))
        c = np.concatenate(([0], np.cumsum(d)))
        out[g] = (c[edge[1:]] - c[edge[:-1]]).astype(np.uint64)
    measured = L >= BINS
    info = dict(n_genes=n, n_measured=int(measured.sum()), model_bases=int(L[measured].sum()), depth_sum=int(out.sum(dtype=np.uint64)))
    return out, info


def eligible(model, s):
    L = gene_lengths(model)
    tot = s.sum(axis=1, dtype=np.uint64)
    return (L >= BINS) & (tot >= L.astype(np.uint64))


def profile(model, s):
    """(depth_sum per bin, eligible genes, norm_mean per bin) of the file."""
    L = gene_lengths(model)
    measured = L >= BINS
    el = np.flatnonzero(eligible(model, s))
    depth_sum = [int(s[measured, k].sum(dtype=np.uint64)) for k in range(BINS)]
    norm = np.zeros(BINS)
    if len(el):
        k = np.arange(BINS, dtype=np.int64)
        Le = L[el][:, None]
        len_k = -((-(k[None, :] + 1) * Le) // BINS) + ((-k[None, :] * Le) // BINS)     # ceil((k + 1) L / 100) - ceil(k L / 100)
        tot = s[el].sum(axis=1, dtype=np.uint64).astype(np.float64)[:, None]
        val = (s[el].astype(np.float64) / len_k.astype(np.float64)) / (tot / Le.astype(np.float64))
        norm = np.cumsum(val, axis=0)[-1] / float(len(el))             # (summed in gene order, like the writer)
    return depth_sum, len(el), norm


def render(model, s):
    """The text of <sample>.gene_body.tsv."""
    depth_sum, n_el, norm = profile(model, s)
    return "bin\tdepth_sum\tgenes\tnorm_mean\n" + "".join("%d\t%d\t%d\t%.6f\n" % (k, depth_sum[k], n_el, norm[k]) for k in range(BINS))


def verbose_line(model, s, info):
    """The -v line up to its timing."""
    return "Gene body: genes %d, measured %d, eligible %d, model_bases %d, depth_sum %d, bins_ms" % (
        info["n_genes"], info["n_measured"], int(eligible(model, s).sum()), info["model_bases"], info["depth_sum"])


def assert_equal(got_sums, got_info, want_sums, want_info):
    for f in INFO:
        assert int(got_info[f]) == int(want_info[f]), (f, int(got_info[f]), int(want_info[f]))
    g, w = np.asarray(got_sums, np.uint64), np.asarray(want_sums, np.uint64)
    assert g.shape == w.shape, (g.shape, w.shape)
    bad = np.argwhere(g != w)
    assert not len(bad), (tuple(int(x) for x in bad[0]), int(g[tuple(bad[0])]), int(w[tuple(bad[0])]))
