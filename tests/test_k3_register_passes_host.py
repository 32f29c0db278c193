"""No GPU needed: the register path of K3, the end-of-file coverage stage (rnaseqc_amd/csrc/rsqc_k3.h: a gene that fits its instance keeps
its coverage vector in registers; maximum, non-zero count and the integer sums of x and x^2 are folded into the scan; mean and deviation
come from the two integer sums, the difference formed in 128 bits; the window medians read the LDS copy beside it), on the wave emulation,
at the smallest shapes at which that code can go wrong.

The kernel runs through hostemu.run_k3 on a DIFFERENCE ARRAY built here from the wanted depth of every transcript base, so depths that
no small set of reads reaches can be crafted.  Expected values come from model() below -- the stage restated on Python integers: exact
sums, the deviation as sqrt(n * sum(x^2) - sum(x)^2) / n from an integer square root -- under the project's tolerances (tests/compare.py);
where records can express the input, the difference array is checked against the per-record code's and every result against the oracle
as well, bias sums and validity flags exactly.  Every case runs under the library's plan and under each forced class: the 146 KB instance
(one round in registers, passes from LDS), the 64 KB one, 256 threads and one wave -- a gene beyond a forced instance's capacity takes the
general path from memory, the others go through register rounds of every width."""
import functools
import math
from fractions import Fraction

import numpy as np
import pytest

from rnaseqc_amd import abi
from tests import hostemu, k3_cases
from tests.compare import FLOAT_ATOL, FLOAT_RTOL
from tests.k3_cases import Gene, down, up

FORCES = (0, 1, 2, 3, 4)


# ---- the stage on Python integers ------------------------------------------------------------------------------------------------------
def mean_sd(vals):
    """(mean, population standard deviation) of integers: sums exact, each result rounded once."""
    n, sx, sxx = len(vals), sum(vals), sum(v * v for v in vals)
    d = n * sxx - sx * sx
    return sx / n, float(Fraction(math.isqrt(d << 128), n << 64))


def quirky_median(vals):
    """computeMedian (src/Metrics.h:147-160) of the values in the order given."""
    n = len(vals)
    if n == 1:
        return float(vals[0])
    mid = (n - 1) // 2
    return (vals[mid] + vals[mid + 1]) / 2.0 if n % 2 else float(vals[mid])


def model(profile, exons, strand, p):
    """What the stage writes for one counted gene: dict(valid, mean, std, cv, three, five, error, exon_cv: per exon a CV or None)."""
    x = [int(v) for v in profile]
    C, M, W, OFF, BGL = len(x), p.coverage_mask, p.bias_window, p.bias_offset, p.bias_gene_length
    out = dict(error=False, three=0, five=0, exon_cv=[])
    lo, hi = M, (C - M if C > M else 0)
    a = 0
    for ln in exons:
        s, e = max(a, lo), min(a + ln, hi)
        a += ln
        cv = None
        if e > s:
            mean, sd = mean_sd(x[s:e])
            cv = sd / mean if mean else None
        out["exon_cv"].append(cv)
    v0, v1 = 0, C
    if C >= BGL:
        mx = max(x)
        pp = x.index(mx) if mx else 0
        cur = min(pp + W // 2, C)
        n = min(W, cur)
        cur -= n
        if n == 0:
            out["error"] = True
        elif quirky_median(x[cur:cur + n]) >= 100.0:
            nnz = sum(1 for v in x if v)
            lower = sorted(x)[(C - nnz) + int(nnz * 0.05)]
            above = [j for j, v in enumerate(x) if v > lower]
            v0, v1 = (above[0], above[-1] + 1) if above else (C, C)
            tlen = v1 - v0
            if tlen >= BGL:
                nl = max(min(OFF + W, tlen) - OFF, 0)
                nr, rlo = (W, tlen - W - OFF) if W + OFF <= tlen else (0, 0)
                if nl == 0 or nr == 0:
                    out["error"] = True
                else:
                    ml = quirky_median(sorted(x[v0 + OFF:v0 + OFF + nl]))
                    mr = quirky_median(sorted(x[v0 + rlo:v0 + rlo + nr]))
                    out["three"], out["five"] = (int(mr), int(ml)) if strand == "+" else (int(ml), int(mr))
    a, b = v0, v1
    if M:
        a, b = (v0 + M, v1 - M) if v1 - v0 > 2 * M else (v0, v0)
    out["valid"] = int(b > a)
    if b > a:
        out["mean"], out["std"] = mean_sd(x[a:b])
        out["cv"] = out["std"] / out["mean"] if out["mean"] else float("nan")
    return out


# ---- cases -----------------------------------------------------------------------------------------------------------------------------
class Case:
    """genes: (name, exon lengths, strand, depth per transcript base); kw: parameters; records: can reads express the depths (then the
    oracle runs too); error: the run ends in ERR_EMPTY_MEDIAN."""
    def __init__(self, name, genes, kw, records=True, error=False):
        self.name, self.genes, self.kw, self.records, self.error = name, genes, dict(kw), records, error

    def params(self):
        return abi.default_params(unpaired=1, **self.kw)


CASES = {}


def _case(name, genes, kw, **k):
    assert name not in CASES
    CASES[name] = lambda: Case(name, genes() if callable(genes) else genes, kw, **k)


@functools.lru_cache(maxsize=None)
def get_case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def get_input(name):
    """The annotation (and, for a case records can express, the reads) through the builder of tests/k3_cases.py."""
    case = get_case(name)
    genes = [Gene(n, ex, st, profile=(prof if case.records else np.ones(len(prof), np.int64))) for n, ex, st, prof in case.genes]
    return k3_cases.build_input(genes)


def diff_array(case):
    """The difference array of the case's depths in the library's layout: a gene's exons contiguous in order, one pad slot behind them."""
    parts = []
    for _, ex, _, prof in case.genes:
        prof = np.asarray(prof, np.int64)
        assert len(prof) == sum(ex)
        parts.append(np.concatenate([np.diff(np.concatenate([[0], prof])), [-prof[-1]]]))
    return (np.concatenate(parts) % (1 << 32)).astype(np.uint32)


# (a) round edges.  A round is T x 16 bases: coding length exactly k rounds and one base more, one wave (1 024 .. 4 096) and 256 threads
# (4 096 under force 3, 4 097 .. 8 193).  `last`: the one maximum is the last base -- the last lane of the last round, or the first lane of
# a round of its own.  `first`: the maximum is base 0, an equal one is the last base.  150 bases at 200x lie beside the base that must win
# and 3 .. 6x beside the other, so the gate (the entry 51 in front of the peak, or 24 behind base 0) opens only for the right one.
ROUND_LENGTHS = (1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193)


def round_edge_profile(coding, kind):
    p = 3 + (np.arange(coding, dtype=np.int64) // 64) % 4
    if kind == "last":
        p[coding - 150:] = 200
    else:
        p[:150] = 200
        p[0] = 500
    p[coding - 1] = 500
    return p


def _round_edges():
    return [("r%d%s" % (c, kind[0]), k3_cases.two_exons(c), "+-"[i % 2], round_edge_profile(c, kind))
            for i, c in enumerate(ROUND_LENGTHS) for kind in ("last", "first")]


_case("round_edges-mask0", _round_edges, dict(coverage_mask=0))
_case("round_edges-mask500", _round_edges, dict(coverage_mask=500))

# (c) cancellation: 60 000x over 3 000 bases with one base at 60 001: the deviation is sqrt(2999) / 3000, lost entirely by
# sum(x^2) / n - mean^2 in doubles (60 000^2 x 2^-53 = 4e-7 against a variance of 3e-4).  Gene statistics with the bias path off (the
# gene is shorter than bias_gene_length) and on (the percentile is 60 000: one base stays); the exon that holds the base.
DEEP = 60_000


def _bump():
    p = np.full(3000, DEEP, np.int64)
    p[1700] += 1
    return [("bump", [1000, 2000], "+", p)]


_case("cancel-bump-nobias", _bump, dict(coverage_mask=0, bias_gene_length=5000))
_case("cancel-bump", _bump, dict(coverage_mask=0))
# a flat vector: deviation and CV exactly 0 (gene: 50x, the gate stays shut; exons: also at 60 000x)
_case("cancel-flat", [("flat50", [1000, 2000], "-", np.full(3000, 50, np.int64)), ("flat60k", [1000, 2000], "+", np.full(3000, DEEP, np.int64))],
      dict(coverage_mask=0, bias_gene_length=5000))
# a counted gene whose masked range is all zero: mean 0, deviation 0, CV NaN; its exon CVs stay unwritten
_case("cancel-zero_range", [("edge_only", [300, 400], "+", np.concatenate([np.full(40, 7), np.zeros(660, np.int64)]))], dict(coverage_mask=50))


# the guard of (c): bits(n) + 2 bits(max) is 64 with 4 095 positions (12 bits) below 2^26 (26 bits), 65 with 4 096 (13 bits): integer
# sums on one side, the two-pass form on the other; both agree with the exact value.  (No reads reach 67 million x.)
def _guard(n):
    return [("g%d" % n, [n - 1000, 1000], "+", (1 << 26) - 1 - (np.arange(n, dtype=np.int64) * 5) % 7)]


_case("guard-bits64", lambda: _guard(4095), dict(coverage_mask=0, bias_gene_length=5000), records=False)
_case("guard-bits65", lambda: _guard(4096), dict(coverage_mask=0, bias_gene_length=5000), records=False)
_case("guard-bits64-trim", lambda: _guard(4095), dict(coverage_mask=0), records=False)


# trim against the folded sums: 5x flanks around a staircase 101 .. of `stairs` bases whose last base is the peak; the percentile (order
# statistic 35 of 700) is 5, so the staircase alone stays: [v0, v1) != [0, coding) and the scan's sums over [mask, coding - mask) do not apply
def _trim(stairs):
    return [("t%d" % stairs, [250, 450], "+-"[stairs % 2], np.concatenate([np.full(300, 5), up(stairs, 101), np.full(400 - stairs, 5)]))]


_case("trim-stairs300", lambda: _trim(300), dict(coverage_mask=50))
_case("trim-2mask", lambda: _trim(100), dict(coverage_mask=50))                  # trimmed length 2 x mask: nothing left
_case("trim-2mask_plus1", lambda: _trim(101), dict(coverage_mask=50))            # ... + 1: one base


# exon against mask 50 (coding 340: [50, 290)): an exon wholly in front, one cut on the left, one inside, one cut on the right, one wholly
# behind; and 64 / 65 exons of 5 bases, mask 7 cutting the second and the last but one
def _exon_mask():
    body = 20 + (np.arange(340, dtype=np.int64) * 5) % 17
    return [("cut", [30, 40, 200, 40, 30], "+", body)]


def _exon_rounds(nex):
    return [("x%d" % nex, [5] * nex, "-", np.concatenate([k3_cases._exon_pattern(k, 5) for k in range(nex)]))]


_case("exon_mask-cut", _exon_mask, dict(coverage_mask=50))
_case("exon_mask-x64", lambda: _exon_rounds(64), dict(coverage_mask=7))
_case("exon_mask-x65", lambda: _exon_rounds(65), dict(coverage_mask=7))

# (d) medians.  500 bases: 5x flanks of 50 (the percentile: trimmed), two regions of 150 bases that hold the windows (offset 0: the first
# and the last bias_window bases of the 400 that stay) around 100 bases at 1 000x with the peak.  Window patterns: all equal, strictly
# increasing, strictly decreasing, two values in no regular order.
MEDIAN_WINDOWS = (1, 2, 3, 64, 65, 99, 100, 128)


def _pattern(kind):
    j = np.arange(150, dtype=np.int64)
    return {"equal": np.full(150, 310, np.int64), "up": up(150, 201), "down": down(150, 457), "two": np.where((j * j + j // 3) % 3 == 0, 220, 330)}[kind]


def _median_genes():
    genes = []
    for k, (left, right) in enumerate((("equal", "up"), ("down", "two"), ("two", "equal"), ("up", "down"))):
        mid = np.full(100, 1000, np.int64)
        mid[50] = 2000
        genes.append(("m_%s_%s" % (left, right), [200, 300], "+-"[k % 2], np.concatenate([np.full(50, 5), _pattern(left), mid, _pattern(right), np.full(50, 5)])))
    return genes


for _w in MEDIAN_WINDOWS:
    _case("median-w%d" % _w, _median_genes, dict(coverage_mask=0, bias_window=_w))
# bias_window larger than the trimmed length (100 stairs stay, bias_gene_length 50 lets them in): no right window, ERR_EMPTY_MEDIAN
_case("median-window_beyond_trimmed", lambda: _trim(100), dict(coverage_mask=0, bias_window=128, bias_gene_length=50), error=True)

CASE_NAMES = list(CASES)


# ---- the run ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pass(name):
    """Difference array and gene counts.  Records: from the per-record code on the host, which the array built here must equal."""
    case, inp = get_case(name), get_input(name)
    cov = diff_array(case)
    if not case.records:
        return cov, np.ones(len(case.genes), np.uint64)
    r = hostemu.run(abi.default_params(unpaired=1), inp.ann, inp.batch, mode=1, want_cov=True)
    np.testing.assert_array_equal(np.asarray(r.cov, np.uint32)[:len(cov)], cov)
    return cov, r.gene_reads


@functools.lru_cache(maxsize=None)
def _oracle(name):
    from oracle import binding
    case, inp = get_case(name), get_input(name)
    try:
        return binding.run_oracle(case.params(), inp.ann, [inp.batch])
    except binding.OracleError as e:
        return e.code


@functools.lru_cache(maxsize=None)
def _model(name):
    case = get_case(name)
    return [model(prof, ex, st, case.params()) for _, ex, st, prof in case.genes]


def check_against_model(case, got_gene, got_exon, want):
    """got_gene(field, gene index), got_exon(field, exon row): the results of a run; want: model() per gene."""
    row = 0
    for g, (w, (gname, ex, _, _)) in enumerate(zip(want, case.genes)):
        assert int(got_gene("gene_cov_valid", g)) == w["valid"], gname
        assert (int(got_gene("bias_three", g)), int(got_gene("bias_five", g))) == (w["three"], w["five"]), gname
        if w["valid"]:
            np.testing.assert_allclose(got_gene("gene_cov_mean", g), w["mean"], rtol=FLOAT_RTOL, atol=FLOAT_ATOL, err_msg=gname)
            np.testing.assert_allclose(got_gene("gene_cov_std", g), w["std"], rtol=FLOAT_RTOL, atol=FLOAT_ATOL, err_msg=gname)
            if math.isnan(w["cv"]):
                assert math.isnan(got_gene("gene_cov_cv", g)), gname
            else:
                np.testing.assert_allclose(got_gene("gene_cov_cv", g), w["cv"], rtol=1e-8, atol=FLOAT_ATOL, err_msg=gname)
        for k, cv in enumerate(w["exon_cv"]):
            assert int(got_exon("exon_cv_valid", row + k)) == int(cv is not None), (gname, k)
            if cv is not None:
                np.testing.assert_allclose(got_exon("exon_cv", row + k), cv, rtol=1e-8, atol=FLOAT_ATOL, err_msg="%s exon %d" % (gname, k))
        row += len(ex)


def check_exact_claims(name, got):
    """What the integer sums promise beyond the project's tolerances."""
    if name == "cancel-flat":
        assert got.gene_cov_std[0] == 0.0 and got.gene_cov_cv[0] == 0.0 and got.gene_cov_mean[0] == 50.0
        assert got.gene_cov_mean[1] == float(DEEP) and got.gene_cov_std[1] == 0.0 and got.gene_cov_cv[1] == 0.0
        assert got.exon_cv_valid.tolist() == [1, 1, 1, 1] and (got.exon_cv == 0.0).all()
    if name == "cancel-bump-nobias":
        # no absolute slack: sqrt(2999) / 3000 to 1e-9, by the integer sums and by the two-pass form of the general path alike (there the
        # mean's rounding, 60 000 x 2^-53, enters the 2 999 small deviations of 1 / 3000 at 2e-8 of each: 1e-11 of the sum of squares)
        np.testing.assert_allclose(got.gene_cov_std[0], math.sqrt(2999.0) / 3000.0, rtol=1e-9, atol=0)
        np.testing.assert_allclose(got.exon_cv[1], math.sqrt(1999.0) / 2000.0 / (DEEP + 1 / 2000.0), rtol=1e-9, atol=0)
        assert got.exon_cv[0] == 0.0
    if name == "cancel-zero_range":
        assert got.gene_cov_valid[0] == 1 and got.gene_cov_mean[0] == 0.0 and got.gene_cov_std[0] == 0.0 and math.isnan(got.gene_cov_cv[0])
        assert got.exon_cv_valid.tolist() == [0, 0]


@pytest.mark.parametrize("force", FORCES)
@pytest.mark.parametrize("name", CASE_NAMES)
def test_emulated_kernel(oracle_lib, name, force):
    case, inp = get_case(name), get_input(name)
    cov, gr = _pass(name)
    got = hostemu.run_k3(case.params(), inp.ann, cov, gr, force=force)
    want = _model(name)
    if case.error:
        assert any(w["error"] for w in want) and got.rc == abi.ERR_EMPTY_MEDIAN
        if case.records:
            assert _oracle(name) == abi.ERR_EMPTY_MEDIAN
        return
    assert got.rc == 0 and not any(w["error"] for w in want)
    check_against_model(case, lambda f, g: getattr(got, f)[g], lambda f, r: getattr(got, f)[r], want)
    check_exact_claims(name, got)
    if case.records:
        ora = _oracle(name)
        assert not isinstance(ora, int), ora
        np.testing.assert_array_equal(gr, ora.gene_reads)
        np.testing.assert_array_equal(got.gene_cov_valid, ora.gene_cov_valid)
        np.testing.assert_array_equal(got.exon_cv_valid, ora.exon_cv_valid)
        np.testing.assert_array_equal(got.bias_three, ora.bias_three)
        np.testing.assert_array_equal(got.bias_five, ora.bias_five)
        check_against_model(case, lambda f, g: getattr(ora, f)[g], lambda f, r: getattr(ora, f)[r], want)    # (the model itself)


def test_the_cases_reach_what_they_name():
    """The paths the cases are aimed at are the ones their inputs take (from the model: no kernel involved)."""
    p0 = abi.default_params(unpaired=1, coverage_mask=0)
    for _, ex, st, prof in _round_edges():                                      # the gate opens: bias sums appear
        m = model(prof, ex, st, p0)
        assert m["three"] > 0 and m["five"] > 0
        if prof[0] == 500:                                                      # ... and would stay shut behind the later, equal maximum
            wrong = np.array(prof).copy()
            wrong[0] -= 1
            assert model(wrong, ex, st, p0)["three"] == 0
    for n, bits in ((4095, 64), (4096, 65)):
        (_, _, _, prof), = _guard(n)
        assert n.bit_length() + 2 * int(prof.max()).bit_length() == bits
    for s, valid in ((100, 0), (101, 1), (300, 1)):
        (_, ex, st, prof), = _trim(s)
        m = model(prof, ex, st, abi.default_params(unpaired=1, coverage_mask=50))
        assert m["valid"] == valid and (not valid or m["mean"] == 101 + (s - 1) / 2.0)
    (_, ex, st, prof), = _exon_mask()
    assert [cv is not None for cv in model(prof, ex, st, abi.default_params(unpaired=1, coverage_mask=50))["exon_cv"]] == [False, True, True, True, False]
    for w in MEDIAN_WINDOWS:
        ms = [model(prof, ex, st, abi.default_params(unpaired=1, coverage_mask=0, bias_window=w)) for _, ex, st, prof in _median_genes()]
        assert all(m["three"] > 0 and m["five"] > 0 for m in ms) and len({(m["three"], m["five"]) for m in ms}) == 4
