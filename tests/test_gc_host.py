"""CPU: --fasta.  The kernels of rnaseqc_amd/csrc/rsqc_gc.h (G/C bit mask, per-exon GC, candidates), the bit helpers of rsqc_device.h
and the pairing / GC replay of rsqc_k5.h, unmodified, on the 64-lane emulation (tests/hostemu/gc_emu.cpp) over the catalogue of
tests/gc_cases.py: round-robin and under two seeded schedules, as one batch and cut in three.  Whole-path expectations come from the
oracle, and from tests/gc_ref.py where the oracle is silent (exon_gc of exons without coverage, candidate-level runs); where both speak
they must agree."""
import os
import re

import numpy as np
import pytest

from rnaseqc_amd import abi, synth
from tests import gc_cases, gc_ref
from tests.hostemu import gc as emu

SEEDS = [0, 7, 1234567]          # 0: round-robin


def _check_expectation(case, got):
    """What the case states by hand."""
    e = case.expect
    if "n_candidates" in e:
        assert got["n_candidates"] == e["n_candidates"]
    if "bins" in e:
        np.testing.assert_array_equal(got["bins"], gc_cases.bins_array(e["bins"]))
        assert got["out_of_range"] == e.get("out_of_range", 0)
    if "fragments" in e:
        assert int(got["bins"].sum()) + got["out_of_range"] == e["fragments"]
    for path in ("hashed", "sorted", "oversize"):
        if path in e:
            assert got[path] == e[path], (path, got[path])


@pytest.fixture(scope="module")
def oracle_results(oracle_lib):
    """name -> the oracle's results for the whole-path case (one batch: the oracle streams, the cut does not matter to it)."""
    cache = {}

    def get(name):
        if name not in cache:
            c = gc_cases.case(name)
            cache[name] = oracle_lib.run_oracle(c.params, c.ann, [c.batch], reference=c.ref)
        return cache[name]
    return get


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("name", gc_cases.WHOLE_PATH)
def test_whole_path_case(name, seed, oracle_results):
    c = gc_cases.case(name)
    want = oracle_results(name)
    want_gc = gc_ref.exon_gc(c.ann, c.ref)
    covered = want.exon_cv_valid.astype(bool)
    assert want.have_reference == 1 and covered.any()
    np.testing.assert_array_equal(want.exon_gc[covered], want_gc[covered])            # the oracle and the restatement agree where both speak
    w_words, w_off, w_len = gc_cases.packed_words(c.ref, c.ann.n_contigs)
    for batches in ([c.batch], gc_cases.three_unequal_batches(c.batch)):
        got = emu.run(c.ann, c.ref, batches=batches, params=c.params, seed=seed)
        assert got["error"] == 0
        np.testing.assert_array_equal(got["words"], w_words)
        np.testing.assert_array_equal(got["word_off"], w_off)
        np.testing.assert_array_equal(got["length"], w_len)
        np.testing.assert_array_equal(got["exon_gc"], want_gc)                        # every exon, as doubles
        np.testing.assert_array_equal(got["bins"], want.gc_bins)
        assert got["out_of_range"] == want.gc_out_of_range
        _check_expectation(c, got)


def test_whole_path_cases_are_cut_in_three_unequal_batches():
    for name in gc_cases.WHOLE_PATH:
        b = gc_cases.case(name).batch
        parts = gc_cases.three_unequal_batches(b)
        assert sum(p.n for p in parts) == b.n and (b.n < 3 or (len(parts) == 3 and all(p.n for p in parts)))


def test_candidate_columns_of_the_state_machine():
    """The candidates kernel's columns for a case whose candidates are listed by hand: file index, row, end, length, the pos != mpos bit."""
    c = gc_cases.case("state_machine")
    got = emu.run(c.ann, c.ref, batches=gc_cases.three_unequal_batches(c.batch), params=c.params, seed=3)
    cols = got["candidates"]
    order = np.argsort(cols["file_index"])
    b = c.batch
    names = [bytes(b.qname[b.qname_off[i]:b.qname_off[i + 1]]).decode() for i in range(b.n)]
    is_cand = [nm in ("i101", "i999", "same", "third", "equal", "back") for nm in names]
    idx = np.flatnonzero(is_cand)
    np.testing.assert_array_equal(cols["file_index"][order], idx.astype(np.uint64))
    np.testing.assert_array_equal(cols["qhash"][order], b.qhash[idx])
    np.testing.assert_array_equal(cols["h2"][order], b.qhash2[idx])
    ref_len = np.array([int(b.cigar[b.cigar_off[i]]) >> 4 for i in idx])
    np.testing.assert_array_equal(cols["endpos"][order], b.pos[idx] + ref_len)
    moved = (b.pos[idx] != b.mpos[idx]).astype(np.uint32) << np.uint32(31)
    np.testing.assert_array_equal(cols["flag_lq"][order], b.l_qseq[idx].astype(np.uint32) | moved)
    assert set(int(x) for x in cols["row"]) == {0} and set(int(x) for x in cols["tid"]) == {0}
    assert int((moved == 0).sum()) == 2                                               # `same`


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("name", gc_cases.CANDIDATE_LEVEL)
def test_candidate_level_case(name, seed):
    c = gc_cases.case(name)
    want_bins, want_oob = gc_cases.replay_expectation(c)
    got = emu.run(c.ann, c.ref, candidates=c.candidates, params=c.params, seed=seed)
    assert got["error"] == 0 and got["n_candidates"] == len(c.expect["cands"])
    np.testing.assert_array_equal(got["bins"], want_bins)
    assert got["out_of_range"] == want_oob
    assert int(want_bins.sum()) + want_oob > 0
    assert 1 <= got["hashed"] + got["sorted"] <= got["buckets"]                       # (an empty bucket takes neither path)
    _check_expectation(c, got)
    if "buckets" in c.expect:
        assert got["buckets"] == c.expect["buckets"]
    if "sorted_min" in c.expect:
        assert got["sorted"] >= c.expect["sorted_min"] and got["oversize"] == 0


def test_random_workload_against_the_oracle(oracle_lib):
    """4 000 pairs over three contigs, two of them in the FASTA: bins, out_of_range and exon_gc of the covered exons against the oracle,
    exon_gc of all exons against the restatement; in three batches under a seeded schedule."""
    contigs = [("chrA", 300_000, 40), ("chrB", 200_000, 25), ("chrC", 100_000, 10)]
    lengths = np.array([c[1] for c in contigs])
    ann = synth.make_annotation(seed=31, contigs=contigs)
    batch = synth.make_reads(ann, 4000, seed=32, dup_frac=0.05, contig_lengths=lengths)
    ref = synth.make_reference(lengths[:2], seed=33, gc_wave=5_000)                    # chrC is not in the FASTA index
    p = abi.default_params()
    want = oracle_lib.run_oracle(p, ann, [batch], reference=ref)
    assert int(want.gc_bins.sum()) > 300 and int((want.gc_bins > 0).sum()) > 15
    got = emu.run(ann, ref, batches=gc_cases.three_unequal_batches(batch), params=p, seed=5)
    assert got["error"] == 0
    np.testing.assert_array_equal(got["bins"], want.gc_bins)
    assert got["out_of_range"] == want.gc_out_of_range
    covered = want.exon_cv_valid.astype(bool)
    assert covered.sum() > 20
    np.testing.assert_array_equal(got["exon_gc"][covered], want.exon_gc[covered])
    np.testing.assert_array_equal(got["exon_gc"], gc_ref.exon_gc(ann, ref))
    assert (got["exon_gc"] == -1.0).any() and got["hashed"] >= 1


def test_bin_edge_premise():
    """What the bin-edge case rests on, with Python floats over the sizes 101-1199: 2 745 (k, size) pairs whose k-fold sum of 1/size lands
    in another bin than (100 k) // size, and 635 sizes below 1 200 whose 100 % sum stays below 1.0 (bin 99, not out of range)."""
    off = 0
    for size in range(101, 1200):
        c, inc = 0.0, 1.0 / float(size)
        for k in range(1, size + 1):
            c += inc
            if gc_ref.bin_of(c) != (100 * k) // size:                 # (k = size: bin 99 against 100)
                off += 1
    below = [size for size in range(1, 1200) if gc_ref.gc_of(size, size) < 1.0]
    assert off == 2745 and len(below) == 635
    assert below[:4] == [6, 7, 10, 13] and all(s in below for s in (102, 103, 104)) and 107 not in below


def test_the_emulation_compiles_the_product_headers():
    """No copy of the kernels' text under tests/: the harness includes the product headers, and the names are defined there."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    harness = open(os.path.join(root, "tests", "hostemu", "gc_emu.cpp")).read()
    for h in ("rsqc_gc.h", "rsqc_k5.h", "rsqc_device.h"):
        assert '#include "../../rnaseqc_amd/csrc/%s"' % h in harness
    defined = {"gc_pack_kernel": "rsqc_gc.h", "exon_gc_kernel": "rsqc_gc.h", "gc_candidates_kernel": "rsqc_gc.h", "gc_replay_kernel": "rsqc_k5.h",
               "gc_replay_big_kernel": "rsqc_k5.h", "gc_count": "rsqc_device.h", "gc_value": "rsqc_device.h"}
    for fn, h in defined.items():
        body = re.compile(r"\b%s\([^;{}]*\)\s*\{" % fn)                                  # a definition: the name, its parameters, a body
        assert body.search(open(os.path.join(root, "rnaseqc_amd", "csrc", h)).read()), fn
        assert not body.search(harness), fn                                            # called, never defined, in the harness


def test_gc_kernels_on_seeded_references_under_sanitizers(tmp_path):
    """tests/hostemu/gc_fuzz.cpp: a stand-alone program around the harness, built with the address and undefined-behaviour sanitizers --
    references with contigs of 0, 1, 63-65 and a few hundred bases, exons and candidate ends on both sides of the contig ends, now and
    then a name with more records than the LDS sort holds.  Every array is a heap block of the size the product allocates: a read of
    gc_count outside its words or a shift by the word size ends the run."""
    import subprocess
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "gc_fuzz")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wno-unused-function",
                           os.path.join(here, "hostemu", "gc_fuzz.cpp"), "-o", exe])
    r = subprocess.run([exe, "8", "1"], capture_output=True, text=True, timeout=900, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "gc_fuzz: 8 cases" in r.stdout
