"""No GPU needed: K3, the end-of-file coverage stage, at its class, depth and window edges (the case table: tests/k3_cases.py).

 * the launch plan the library uses (rnaseqc_amd/csrc/rsqc_k3_plan.h, reached through the emulation library) covers every gene exactly
   once, with the smallest instance that holds it -- for every multiset of boundary lengths, for random length vectors, with class counts
   that do not fit the lengths, and under every forced configuration;
 * every case through the reference's own Metrics.cpp (oracle/_ref/libref_metrics.so): the oracle agrees bit for bit;
 * every case through the kernel itself on the wave emulation (tests/hostemu/k3_emu.cpp), launched by the library's plan, against the oracle;
 * the expectations written down by hand in the table against both.

Configurations left out to keep the file to minutes: lds16_bounds runs under force 0 and 2 only (not 1, 3, 4), the two depth cases
under force 0 and 1 only (not 2, 3, 4); the other cases name the forced configurations they run under in the table (Case.forces)."""
import functools
import itertools

import numpy as np
import pytest

from rnaseqc_amd import abi
from tests import hostemu, k3_cases
from tests.compare import FLOAT_ATOL, FLOAT_RTOL
from tests.test_k3_wave_emulation import _compare

CASE_NAMES = [c.name for c in k3_cases.CASES]


# ---- the plan ----------------------------------------------------------------------------------------------------------------------
CAPS = np.array([cap for _, cap in k3_cases.LAUNCHES], np.int64)
THREADS = np.array([t for t, _ in k3_cases.LAUNCHES], np.int64)
BOUNDARY = sorted({b + d for b in (1024, 1025, 2048, 2049, 3072, 3073, 4096, 4097, 6144, 6145, 12288, 12289, 32768, 32769, 73000, 73001)
                   for d in (-1, 0, 1)})
COUNT, FIRST = 3, 4              # columns of a plan row (hostemu.K3_PLAN_COLUMNS)


def _multisets(max_size):
    """Every multiset of 1 .. max_size boundary lengths: (m x max_size lengths, m sizes)."""
    rows, ns = [], []
    for size in range(1, max_size + 1):
        idx = np.fromiter(itertools.chain.from_iterable(itertools.combinations_with_replacement(range(len(BOUNDARY)), size)), np.int64).reshape(-1, size)
        block = np.zeros((len(idx), max_size), np.uint32)
        block[:, :size] = np.array(BOUNDARY, np.uint32)[idx]
        rows.append(block); ns.append(np.full(len(idx), size, np.uint32))
    return np.concatenate(rows), np.concatenate(ns)


def _random_vectors(count=400, width=200, seed=31):
    rng = np.random.default_rng(seed)
    lengths = np.zeros((count, width), np.uint32)
    ns = rng.integers(1, width + 1, count).astype(np.uint32)
    for r in range(count):
        n = int(ns[r])
        near = rng.choice(BOUNDARY, n)
        free = np.exp(rng.uniform(0, np.log(120_000), n)).astype(np.int64) + 1
        lengths[r, :n] = np.where(rng.random(n) < (0.0, 0.3, 0.7, 1.0)[r % 4], near, free)
    return lengths, ns


def _assignment(plans, ns, width):
    """The launch of every position of gene_order, after checking that the eight ranges are disjoint and cover [0, n) exactly."""
    count, first = plans[:, :, COUNT], plans[:, :, FIRST]                   # (m, 8)
    n = ns.astype(np.int64)[:, None]
    assert (count.sum(axis=1) == n[:, 0]).all()
    assert (first + count <= n).all()
    j = np.arange(width, dtype=np.int64)[None, None, :]
    inside = (first[:, :, None] <= j) & (j < (first + count)[:, :, None])  # (m, 8, width)
    assert (inside.sum(axis=1) == (j[0] < n)).all()
    return np.where(j[0] < n, inside.argmax(axis=1), -1)


def _check_plan(lengths, ns, force=0, delta=None, chunk=200_000):
    width = lengths.shape[1]
    for lo in range(0, len(ns), chunk):
        ln, nn = lengths[lo:lo + chunk], ns[lo:lo + chunk]
        _, plans, srt = hostemu.k3_plan_many(ln, nn, force=force, delta=None if delta is None else delta[lo:lo + chunk])
        np.testing.assert_array_equal(plans[:, :, 0], np.broadcast_to(THREADS, plans[:, :, 0].shape))
        np.testing.assert_array_equal(plans[:, :, 2], np.broadcast_to(CAPS, plans[:, :, 2].shape))
        assign = _assignment(plans, nn, width)
        live = assign >= 0
        if force == 0 and delta is None:
            holds = (CAPS[np.maximum(assign, 0)] >= srt) | (assign == 0)
            assert holds[live].all()                                         # a launch whose capacity holds the gene, or the 146 KB one
            want = np.select([srt <= c for c in (1024, 2048, 3072, 4096, 6144, 12288, 32768)], [7, 6, 5, 4, 2, 1, 3], 0)
            np.testing.assert_array_equal(assign[live], want[live])         # ... the smallest of its thread class
        elif force:
            want_threads = {1: 1024, 2: 1024, 3: 256, 4: 64}[force]
            assert (THREADS[np.maximum(assign, 0)][live] == want_threads).all()
            if force == 1:
                assert (assign[live] == 0).all()
            if force == 2:
                assert (assign[live] == 3).all()


def test_plan_every_multiset_of_boundary_lengths():
    lengths, ns = _multisets(6)
    assert len(ns) > 2_000_000 and len(BOUNDARY) == 32
    _check_plan(lengths, ns)


def test_plan_random_length_vectors():
    lengths, ns = _random_vectors()
    _check_plan(lengths, ns)
    for force in (1, 2, 3, 4):
        _check_plan(lengths, ns, force=force)


def test_plan_forced_configurations_on_boundary_multisets():
    lengths, ns = _multisets(4)
    for force in (1, 2, 3, 4):
        _check_plan(lengths, ns, force=force)


@pytest.mark.parametrize("which", ["n_le6144", "n_le3072", "n_le2048", "n_le1024"])
@pytest.mark.parametrize("by", [1, -1])
def test_plan_with_inconsistent_counts_still_covers_every_gene_once(which, by):
    """A count of short genes that is one too large or one too small (0 - 1 wraps, as it would in the library's uint32_t): the fallback
    and the two clamps of k3_plan keep the eight ranges a partition of [0, n).  (A gene may then sit in an instance too small for it:
    that instance runs it in its in-memory mode.)"""
    col = hostemu.K3_COUNT_NAMES.index(which)
    for lengths, ns in (_multisets(4), _random_vectors(count=200)):
        delta = np.zeros((len(ns), 7), np.int32)
        delta[:, col] = by
        _check_plan(lengths, ns, delta=delta)


def test_plan_of_the_single_call_export_matches():
    counts, plans, _ = hostemu.k3_plan_many(np.array([k3_cases.CLASS_BOUNDS], np.uint32), [12])
    rows = hostemu.k3_plan(12, *[int(x) for x in counts[0]])
    assert [[r[c] for c in hostemu.K3_PLAN_COLUMNS] for r in rows] == plans[0].tolist()
    assert [r["count"] for r in rows] == [0, 2, 2, 1, 2, 2, 2, 1]
    assert [r["first"] for r in rows] == [0, 1, 3, 0, 5, 7, 9, 11]
    assert [r["stream"] for r in rows] == [0, 1, 1, 2, 1, 1, 1, 1] and [r["cov_bits"] for r in rows] == [16, 32, 32, 16, 32, 32, 32, 32]


# ---- the legs ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ref(oracle_lib):
    if oracle_lib.ref_lib() is None:
        try:
            oracle_lib.build_ref()
        except Exception:
            pass
    if oracle_lib.ref_lib() is None:
        pytest.skip("oracle/_ref/libref_metrics.so cannot be built here (it is compiled from the reference's source tree)")
    return oracle_lib


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """The oracle's results of a case (shared by the legs, left unchanged), or ERR_EMPTY_MEDIAN."""
    from oracle import binding
    case = k3_cases.CASE_BY_NAME[name]
    try:
        return binding.run_oracle(case.params(), case.input.ann, [case.input.batch])
    except binding.OracleError as e:
        assert e.code == abi.ERR_EMPTY_MEDIAN
        return abi.ERR_EMPTY_MEDIAN


@functools.lru_cache(maxsize=None)
def _pass(input_name):
    """The difference array and the gene counts of the input's reads (the per-record code on the host; no K3 parameter enters)."""
    inp = k3_cases.get_input(input_name)
    r = hostemu.run(abi.default_params(unpaired=1), inp.ann, inp.batch, mode=1, want_cov=True)
    return r.cov, r.gene_reads


def test_the_table_covers_what_it_names():
    groups = {n.split("-")[0] for n in CASE_NAMES}
    assert groups == {"class_bounds", "lds16_bounds", "depth_65535", "depth_65536", "plan_degenerate", "exon_rounds", "mask_edges",
                      "gate_edges", "trim_edges", "window_edges", "window_wide"}
    for name, (_, launches) in k3_cases.INPUTS.items():
        inp = k3_cases.get_input(name)
        assert inp.n_reads <= 12_000 or name in ("depth_65535", "depth_65536", "trim_radix3", "exon_rounds"), (name, inp.n_reads)
    deep = {n: k3_cases.get_input(n).genes[0].profile for n in ("depth_65535", "depth_65536")}
    assert int(deep["depth_65535"].max()) == 65_535 and int(deep["depth_65536"].max()) == 65_536


@pytest.mark.parametrize("name", CASE_NAMES)
def test_oracle_vs_reference_metrics_cpp(ref, oracle_lib, name):
    """Bit for bit, as tests/test_reference_metrics.py compares its seeded inputs."""
    case = k3_cases.CASE_BY_NAME[name]
    inp, p = case.input, case.params()
    got = _oracle(name)
    c = inp.commits
    args = (inp.geo, inp.elen, inp.gstrand, c[:, 0], c[:, 1], c[:, 2], c[:, 3])
    kw = dict(mask=p.coverage_mask, bias_offset=p.bias_offset, bias_window=p.bias_window, bias_gene_length=p.bias_gene_length)
    if case.error:
        assert got == abi.ERR_EMPTY_MEDIAN
        with pytest.raises(ref.OracleError) as ei:
            ref.ref_coverage_run(*args, **kw)
        assert ei.value.code == abi.ERR_EMPTY_MEDIAN
        return
    assert got != abi.ERR_EMPTY_MEDIAN
    want = ref.ref_coverage_run(*args, **kw)
    np.testing.assert_array_equal(got.gene_cov_valid, want["gene_valid"])
    v = want["gene_valid"].astype(bool)
    np.testing.assert_array_equal(got.gene_cov_mean[v], want["gene_mean"][v])
    np.testing.assert_array_equal(got.gene_cov_std[v], want["gene_std"][v])
    np.testing.assert_array_equal(got.gene_cov_cv[v], want["gene_cv"][v])
    np.testing.assert_array_equal(got.exon_cv_valid, want["exon_cv_valid"])     # (exon ids are exon rows in these annotations)
    ev = want["exon_cv_valid"].astype(bool)
    np.testing.assert_array_equal(got.exon_cv[ev], want["exon_cv"][ev])
    tot = (got.bias_three + got.bias_five).astype(np.float64)
    ratio = np.where(tot > 0, got.bias_three / np.where(tot > 0, tot, 1), -1.0)
    np.testing.assert_array_equal(ratio, want["bias_ratio"])
    assert int((tot > 0).sum()) == want["counted_genes"]
    np.testing.assert_array_equal(got.gene_reads > 0, [g.profile is not None for g in inp.genes])


def _emulate(name, force):
    case = k3_cases.CASE_BY_NAME[name]
    inp, want = case.input, _oracle(name)
    cov, gr = _pass(case.input_name)
    got = hostemu.run_k3(case.params(), inp.ann, cov, gr, force=force)
    if force == 0:
        assert got.launches == inp.launches                                   # the per-launch counts the input was built for
    if case.error:
        assert want == abi.ERR_EMPTY_MEDIAN and got.rc == abi.ERR_EMPTY_MEDIAN
        return None
    np.testing.assert_array_equal(gr, want.gene_reads)
    _compare(got, want)
    return got


@pytest.mark.parametrize("name", CASE_NAMES)
def test_emulated_kernel_vs_oracle_under_the_library_plan(name):
    _emulate(name, 0)


FORCED = [(c.name, f) for c in k3_cases.CASES for f in c.forces]


@pytest.mark.parametrize("name,force", FORCED)
def test_emulated_kernel_vs_oracle_forced(name, force):
    _emulate(name, force)


def test_bias_path_runs_where_it_is_meant_to():
    """What the cases rest on: the gate opens and both bias sums come out different where a case exercises the windows."""
    r = _oracle("class_bounds-mask0")
    assert (r.bias_three > 0).all() and (r.bias_five > 0).all() and (r.bias_three != r.bias_five).all()
    r = _oracle("lds16_bounds")
    assert (r.bias_three > 0).all() and (r.bias_three != r.bias_five).all()
    for name in ("depth_65535", "depth_65536"):
        r = _oracle(name)
        assert r.bias_three[0] > 0 and r.bias_five[0] > 0
    for w in k3_cases.GATE_WINDOWS:
        case = k3_cases.CASE_BY_NAME["gate_edges-w%d" % w]
        r, inp = _oracle(case.name), case.input
        for g in inp.genes:                         # an open gate shows: the trim moves the mean off that of the profile, or a bias sum appears
            i = inp.index[g.name]
            moved = abs(float(r.gene_cov_mean[i]) - float(np.mean(g.profile))) > 1e-9 or int(r.bias_three[i]) + int(r.bias_five[i]) > 0
            assert moved == g.name.endswith("_open"), (w, g.name)
    r = _oracle("trim_edges-radix3")
    assert r.bias_three[0] > 0
    r, inp = _oracle("exon_rounds-mask0"), k3_cases.get_input("exon_rounds")
    assert r.exon_cv_valid.all() and len(np.unique(np.round(r.exon_cv, 12))) >= 20
    r = _oracle("mask_edges-mask7")
    inp = k3_cases.get_input("mask_edges")
    ex = {g.name: list(range(inp.geo[i], inp.geo[i + 1])) for i, g in enumerate(inp.genes)}
    assert r.exon_cv_valid[ex["short_ends"]].tolist() == [0, 1, 0]
    assert r.exon_cv_valid[ex["one_base"]].tolist() == [1, 1, 1] and r.exon_cv[ex["one_base"][0]] == 0.0 and r.exon_cv[ex["one_base"][2]] == 0.0
    valid = {m: _oracle("mask_edges-mask%d" % m).gene_cov_valid for m in (299, 300, 301)}
    for g in ("m600", "m600z", "flank"):                                      # valid, swallowed, swallowed
        assert [int(valid[m][inp.index[g]]) for m in (299, 300, 301)] == [1, 0, 0], g


HAND = [(c.name, g) for c in k3_cases.CASES for g in sorted(c.hand)]


@pytest.mark.parametrize("name,gene", HAND)
def test_hand_derived_numbers(name, gene):
    """Oracle and emulated kernel equal the numbers written in the table, which come from the reference's source lines alone."""
    case = k3_cases.CASE_BY_NAME[name]
    want = case.hand[gene]
    i = case.input.index[gene]
    cov, gr = _pass(case.input_name)
    for got in (_oracle(name), hostemu.run_k3(case.params(), case.input.ann, cov, gr, force=0)):
        assert int(got.gene_cov_valid[i]) == want["valid"]
        assert int(got.bias_three[i]) == want["three"] and int(got.bias_five[i]) == want["five"]
        if want["valid"]:
            np.testing.assert_allclose(got.gene_cov_mean[i], want["mean"], rtol=FLOAT_RTOL, atol=FLOAT_ATOL)
            np.testing.assert_allclose(got.gene_cov_std[i], want["std"], rtol=FLOAT_RTOL, atol=FLOAT_ATOL)
