"""The contract of --tin (include/rnaseqc_amd.h, rsqc_tin_info; rnaseqc_amd/csrc/rsqc_tin.h) restated with numpy and math.fsum: the
expected rows, figures and text of every tin test come from here, never from the code under test.

model        the model of --gene-body (tests/genebody_ref.py) without its `reverse` byte; L = the sum of the segment lengths; a gene
             is measured when L >= 1
row          over the gene's model positions, d = depth(p): depth_sum S = sum d, covered = #{d > 0}, max_depth = max d (exact);
             dlog2d E = math.fsum(d * math.log2(d)) over d >= 2 (the exactly rounded sum; depths 0 and 1 contribute exactly 0)
bound        the device adds E in a fixed order: |E_device - E| <= (items + 80) * 2^-52 * E, items = ceil(L / 4096); E = 0 is exact
file         gene_id, length, covered, depth_sum, max_depth, mean_depth = S / L (%.6f), tin (%.6f): for an eligible gene (L >= 100 and
             S >= L) H = ln(S) - E ln(2) / S, tin = 100 exp(H) / L; 0 for every other gene
summary      genes, eligible, and over the eligible genes' tin: mean (in gene order), median, population standard deviation
"""
import math

import numpy as np

from tests.genebody_ref import depth_arrays, gene_lengths, make_model, model_from_annotation  # noqa: F401  (the model is --gene-body's)

ITEM = 4096                                         # RSQC_TIN_ITEM: most model bases of one plan item
ROW = np.dtype([("depth_sum", np.uint64), ("covered", np.uint32), ("max_depth", np.uint32), ("dlog2d", np.float64)])
INFO = ("n_genes", "n_measured", "model_bases", "depth_sum", "covered_bases")
MIN_LENGTH = 100
HEADER = "gene_id\tlength\tcovered\tdepth_sum\tmax_depth\tmean_depth\ttin\n"
SUMMARY_HEADER = "genes\teligible\tmean\tmedian\tstdev\n"


def items_of(L):
    return -(-int(L) // ITEM)


def bound(L):
    """The relative bound of a gene's E against the exactly rounded sum, by the contract's formula."""
    return (items_of(L) + 80) * 2.0 ** -52


def dlog2d(d):
    """math.fsum(d * math.log2(d)) over the depths >= 2 of an integer array (the terms are made once per distinct depth)."""
    d = np.asarray(d, np.int64)
    d = d[d >= 2]
    if not len(d):
        return 0.0
    values, inverse = np.unique(d, return_inverse=True)
    terms = np.array([int(v) * math.log2(int(v)) for v in values], np.float64)
    return math.fsum(terms[inverse].tolist())


def rows(depth, model):
    """(rows [n_genes] of ROW, info)."""
    n = len(model["seg_off"]) - 1
    out = np.zeros(n, ROW)
    L = gene_lengths(model)
    for g in range(n):
        lo, hi = int(model["seg_off"][g]), int(model["seg_off"][g + 1])
        if not L[g]:
            continue
        d = np.concatenate([depth[int(model["seg_tid"][k])][int(model["seg_start"][k]):int(model["seg_end"][k])] for k in range(lo, hi)]).astype(np.int64)
        out[g] = (int(d.sum()), int((d > 0).sum()), int(d.max()), dlog2d(d))
    info = dict(n_genes=n, n_measured=int((L >= 1).sum()), model_bases=int(L.sum()), depth_sum=int(out["depth_sum"].sum(dtype=np.uint64)),
                covered_bases=int(out["covered"].sum(dtype=np.uint64)))
    return out, info


def tin_formula(L, S, E):
    """100 exp(H) / L of one gene with S >= 1, whatever its eligibility."""
    return 100.0 * math.exp(math.log(float(S)) - float(E) * math.log(2.0) / float(S)) / float(L)


def values(L, r):
    """(mean_depth, tin, eligible) per gene, as the file prints them (before rounding)."""
    n = len(L)
    mean, tin, el = np.zeros(n), np.zeros(n), np.zeros(n, bool)
    for g in range(n):
        Lg, S = int(L[g]), int(r["depth_sum"][g])
        if Lg:
            mean[g] = S / Lg
        if Lg >= MIN_LENGTH and S >= Lg:
            el[g] = True
            tin[g] = tin_formula(Lg, S, r["dlog2d"][g])
    return mean, tin, el


def summary(tin, el):
    """(eligible, mean, median, stdev)."""
    v = [float(x) for x in np.asarray(tin)[np.asarray(el, bool)]]
    if not v:
        return 0, 0.0, 0.0, 0.0
    mean = 0.0
    for x in v:
        mean += x                                                      # (in gene order, like the writer)
    mean /= len(v)
    s = sorted(v)
    median = s[len(s) // 2] if len(s) % 2 else (s[len(s) // 2 - 1] + s[len(s) // 2]) / 2.0
    var = 0.0
    for x in v:
        var += (x - mean) * (x - mean)
    return len(v), mean, median, math.sqrt(var / len(v))


def render(ids, L, r):
    """The text of <sample>.tin.tsv."""
    mean, tin, _ = values(L, r)
    return HEADER + "".join("%s\t%d\t%d\t%d\t%d\t%.6f\t%.6f\n" % (ids[g], int(L[g]), int(r["covered"][g]), int(r["depth_sum"][g]), int(r["max_depth"][g]), mean[g], tin[g])
                            for g in range(len(L)))


def render_summary(L, r):
    """The text of <sample>.tin_summary.tsv."""
    _, tin, el = values(L, r)
    return SUMMARY_HEADER + "%d\t%d\t%.6f\t%.6f\t%.6f\n" % ((len(L),) + summary(tin, el))


def verbose_line(L, r, info):
    """The -v line up to its median."""
    _, _, el = values(L, r)
    return "TIN: genes %d, measured %d, eligible %d, model_bases %d, covered_bases %d, depth_sum %d, median " % (
        info["n_genes"], info["n_measured"], int(el.sum()), info["model_bases"], info["covered_bases"], info["depth_sum"])


def assert_rows(got, got_info, want, want_info, L):
    """The integers bit for bit, E within the bound of the contract (E = 0: equality)."""
    for f in INFO:
        assert int(got_info[f]) == int(want_info[f]), (f, int(got_info[f]), int(want_info[f]))
    assert got.shape == want.shape, (got.shape, want.shape)
    for f in ("depth_sum", "covered", "max_depth"):
        bad = np.flatnonzero(got[f] != want[f])
        assert not len(bad), (f, int(bad[0]), int(got[f][bad[0]]), int(want[f][bad[0]]))
    tol = np.array([bound(x) for x in L]) * want["dlog2d"]
    err = np.abs(got["dlog2d"] - want["dlog2d"])
    bad = np.flatnonzero(~(err <= tol))
    assert not len(bad), ("dlog2d", int(bad[0]), float(got["dlog2d"][bad[0]]), float(want["dlog2d"][bad[0]]), float(err[bad[0]]), float(tol[bad[0]]))
