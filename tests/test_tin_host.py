"""CPU: --tin.  The two kernels of rnaseqc_amd/csrc/rsqc_tin.h, unmodified, with the header's launch plan and the model check and the
walk of rsqc_genemodel.h, on the 64-lane emulation over the edge catalogue (tests/tin_cases.py) against the restatement of the contract
(tests/tin_ref.py), round-robin and under seeded schedules: the integers bit for bit, the double within the contract's bound and
bit-identical across the schedules; the exported plan; every model rule violated once; the same catalogue through a stand-alone
sanitizer build of the harness; the host arithmetic (TIN, summary, the text of both files) through librsqc_host.so; the command
line's usage text and the refused multi-GPU combination."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from tests import compare
from tests import tin_cases as tc
from tests import tin_ref as ref
from tests.hostemu import tin as emu
from tests.test_cli import cli  # noqa: F401
from tests.test_junction_host import GTF, host_lib  # noqa: F401

SEEDS = [0, 7, 1234567, 99]      # 0: round-robin, and three seeded schedules


def _check_plan(model, items, item_off, info):
    """The items tile every measured gene's [0, L) exactly once, each at most ITEM bases, with the segment that holds its first base;
    item_off names every gene's first item and, with its successor, its count."""
    L = ref.gene_lengths(model)
    seg_len = model["seg_end"].astype(np.int64) - model["seg_start"].astype(np.int64)
    at = {}
    for k, (gene, u0, u1, seg, seg_u) in enumerate(items.tolist()):
        assert L[gene] >= 1
        assert u0 == at.get(gene, 0) and u0 < u1 <= L[gene] and u1 - u0 <= tc.ITEM and (u1 - u0 == tc.ITEM or u1 == L[gene])
        assert int(item_off[gene]) <= k < int(item_off[gene + 1])
        at[gene] = u1
        lo, hi = int(model["seg_off"][gene]), int(model["seg_off"][gene + 1])
        assert lo <= seg < hi
        assert seg_u == int(seg_len[lo:seg].sum()) and seg_u <= u0 < seg_u + int(seg_len[seg])
    assert at == {g: int(L[g]) for g in range(len(L)) if L[g] >= 1}
    assert info["items"] == len(items) == sum(ref.items_of(x) for x in L)
    assert info["workgroups"] == -(-len(items) // 4)
    assert [int(g) for g in items[:, 0]] == sorted(int(g) for g in items[:, 0])                # a gene's items are contiguous, in u order
    assert int(item_off[0]) == 0 and np.diff(item_off.astype(np.int64)).tolist() == [ref.items_of(x) for x in L]
    assert info["n_measured"] == int((L >= 1).sum()) and info["model_bases"] == int(L.sum())


@pytest.mark.parametrize("name", tc.SMALL)
def test_catalogue(name):
    """Every schedule: integers bit for bit, E within the bound; E bit-identical across the schedules (the reproducibility rule)."""
    lengths, _, model, depth, want, want_info, L = tc.case(name)
    first = None
    for seed in SEEDS:
        got, info, items, item_off = emu.run(lengths, depth, model, seed=seed)
        ref.assert_rows(got, info, want, want_info, L)
        _check_plan(model, items, item_off, info)
        if first is None:
            first = got
        assert got.tobytes() == first.tobytes(), (name, seed)


def test_item_edges_take_the_items_they_are_named_for():
    lengths, _, model, depth, _, _, _ = tc.case("item_edges")
    _, _, items, item_off = emu.run(lengths, depth, model)
    assert np.bincount(items[:, 0], minlength=5).tolist() == [1, 1, 2, 4, 4] and item_off.tolist() == [0, 1, 2, 4, 8, 12]
    g3 = items[items[:, 0] == 3]
    assert g3[:, 1].tolist() == [0, tc.ITEM, 2 * tc.ITEM, 3 * tc.ITEM] and g3[:, 3].tolist() == [3, 4, 4, 5] and g3[:, 4].tolist() == [0, tc.ITEM, tc.ITEM, 2 * tc.ITEM + 700]


@pytest.mark.parametrize("seed", [0, 3])
def test_many_genes_of_one_base(seed):
    """3 000 genes of one base through the kernels (a fiber per lane: the 70 000 of the GPU test would be 4.5 M fibers): items with one
    live lane ..."""
    lengths, _, model, depth, want, want_info, L = tc.case("many_genes_of_one_base", emu=True)
    got, info, items, item_off = emu.run(lengths, depth, model, seed=seed)
    ref.assert_rows(got, info, want, want_info, L)
    _check_plan(model, items, item_off, info)
    assert info["workgroups"] == tc.MANY_EMU // 4


def test_plan_of_70000_genes():
    """... and the plan of all 70 000, without the kernels: one item a gene, 17 500 workgroups."""
    model = tc.model_of(tc._many(tc.MANY))
    info, items, item_off = emu.plan(model)
    _check_plan(model, items, item_off, info)
    assert info["items"] == tc.MANY and info["workgroups"] == tc.MANY // 4 and info["model_bases"] == tc.MANY


def test_the_two_plans_tile_alike():
    """--tin and --gene-body cut a gene with one function (gene_tile of rsqc_genemodel.h): on one contig of 10 000, genes of 99 bases
    (measured by --tin alone), 100 (the least --gene-body measures), 4 096 in one segment (one full item) and 4 097 in two (the least
    with two items; base 4 096 is the second segment's first) -- the tin items of every gene with L >= 100 are words 0..4 of its
    gene-body items, item_off is contiguous."""
    from tests.hostemu import genebody as gb_emu
    model = dict(seg_off=np.array([0, 1, 2, 3, 5], np.uint32), seg_tid=np.zeros(5, np.int32), seg_start=np.array([0, 100, 300, 4500, 8600], np.uint32),
                 seg_end=np.array([99, 200, 300 + tc.ITEM, 4500 + tc.ITEM, 8601], np.uint32), reverse=np.array([0, 1, 0, 1], np.uint8))
    assert int(model["seg_end"].max()) <= 10_000
    L = ref.gene_lengths(model)
    assert L.tolist() == [99, 100, tc.ITEM, tc.ITEM + 1]
    info, items, item_off = emu.plan(model)
    gb_info, gb_items = gb_emu.plan(model)
    _check_plan(model, items, item_off, info)
    assert item_off.tolist() == [0, 1, 2, 3, 5] and int(item_off[-1]) == len(items)
    for g in range(4):
        mine, theirs = items[items[:, 0] == g], gb_items[gb_items[:, 0] == g]
        if L[g] >= 100:
            assert len(mine) and mine.tolist() == theirs[:, :5].tolist(), g
            assert (theirs[:, 5] == (int(L[g]) | int(model["reverse"][g]) << 31)).all()
        else:
            assert mine.tolist() == [[g, 0, 99, 0, 0]] and len(theirs) == 0
    assert items[1:].tolist() == gb_items[:, :5].tolist()
    assert items[3:].tolist() == [[3, 0, tc.ITEM, 3, 0], [3, tc.ITEM, tc.ITEM + 1, 4, tc.ITEM]]
    assert (info["n_measured"], info["model_bases"]) == (4, int(L.sum())) and (gb_info["n_measured"], gb_info["model_bases"]) == (3, int(L[1:].sum()))


def test_sum_above_2_pow_32():
    """One gene of 70 000 bases under depth 70 000: 18 items added in item order, S = 4.9e9; the same bits under another schedule."""
    lengths, _, model, depth, want, want_info, L = tc.case("sum_above_2_pow_32")
    got, info, items, item_off = emu.run(lengths, depth, model)
    ref.assert_rows(got, info, want, want_info, L)
    _check_plan(model, items, item_off, info)
    assert info["items"] == 18 + 1 and int(got["depth_sum"][0]) == tc.BIG_RECORDS * tc.BIG_L > 1 << 32
    again, _, _, _ = emu.run(lengths, depth, model, seed=11)
    assert again.tobytes() == got.tobytes()


@pytest.mark.parametrize("name", list(tc.BROKEN))
def test_every_model_rule_violated_once(name):
    model, word, gene = tc.broken_model(name)
    with pytest.raises(emu.ModelError) as err:
        emu.run(tc.LENGTHS, [np.zeros(n, np.uint32) for n in tc.LENGTHS], model)
    assert word in str(err.value) and gene in str(err.value), str(err.value)


def test_catalogue_under_sanitizers(tmp_path):
    """The stand-alone form of the harness built with the address and undefined-behaviour sanitizers, as a child process: the scanned
    array, the model's columns, the plan, the item slots and the rows have exactly their size there."""
    exe = str(tmp_path / "tin_emu")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-DTINEMU_MAIN", "-DWAVEMU_STACK_BYTES=32768", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wno-unused-function", "-Wno-unused-variable", emu.PROGRAM_SOURCE, "-o", exe])
    for name in tc.SMALL:
        lengths, _, model, depth, want, info, L = tc.case(name)
        got_rows, _, _, _ = emu.run(lengths, depth, model)                 # (its doubles were compared with the reference above)
        bits = 0
        for b in got_rows["dlog2d"].view(np.uint64).tolist():
            bits = ((bits * 1000003) & 0xFFFFFFFFFFFFFFFF) ^ b
        for seed in (0, 5):
            path = str(tmp_path / "case.bin")
            emu.write_case_file(path, lengths, depth, model, seed)
            r = subprocess.run([exe, path], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
            assert r.returncode == 0, (name, seed, r.stdout[-2000:] + r.stderr[-4000:])
            got = dict(kv.split("=") for kv in r.stdout.split()[1:])
            assert (int(got["rc"]), int(got["genes"]), int(got["measured"]), int(got["bases"]), int(got["items"]), int(got["depth_sum"]), int(got["covered"]), int(got["peaks"]), int(got["bits"])) == \
                (0, info["n_genes"], info["n_measured"], info["model_bases"], sum(ref.items_of(x) for x in L), info["depth_sum"], info["covered_bases"],
                 int(want["max_depth"].sum(dtype=np.uint64)), bits), (name, seed, r.stdout)


# ---- the host arithmetic, through librsqc_host.so ------------------------------------------------------------------------------------
def _host(host_lib, L, rows, tmp_path=None, ids=None):
    """tin_profile (and, with tmp_path, write_tin / write_tin_summary) of the command line on lengths and rows given as columns."""
    vp = C.c_void_p
    host_lib.host_tin_profile.argtypes = [C.c_uint64] + [vp] * 8
    n = len(L)
    L32, r = np.ascontiguousarray(L, np.uint32), np.ascontiguousarray(rows, ref.ROW)
    tin, mean, stats = np.zeros(max(n, 1)), np.zeros(max(n, 1)), np.zeros(4)
    paths = [None, None, None]
    if tmp_path is not None:
        arr = (C.c_char_p * max(n, 1))(*[s.encode() for s in ids])
        paths = [C.cast(arr, vp), str(tmp_path / "x.tin.tsv").encode(), str(tmp_path / "x.tin_summary.tsv").encode()]
    rc = host_lib.host_tin_profile(n, L32.ctypes.data, r.ctypes.data, tin.ctypes.data, mean.ctypes.data, stats.ctypes.data, *paths)
    assert rc == 0
    text = None if tmp_path is None else (open(paths[1].decode()).read(), open(paths[2].decode()).read())
    return tin[:n], mean[:n], stats, text


def _same_text(got, want, floats):
    """Integer columns and ids as text; the last `floats` columns as printed (%.6f) within the 1e-6 of tests/compare.py."""
    g, w = [l.split("\t") for l in got.split("\n")], [l.split("\t") for l in want.split("\n")]
    assert len(g) == len(w) and g[0] == w[0] and g[-1] == w[-1] == [""]
    for a, b in zip(g[1:-1], w[1:-1]):
        assert len(a) == len(b)
        for k, (x, y) in enumerate(zip(a, b)):
            if k >= len(a) - floats:
                assert len(x.split(".")[1]) == 6 and np.isclose(float(x), float(y), rtol=compare.FLOAT_RTOL, atol=compare.FLOAT_ATOL), (a, b)
            else:
                assert x == y, (a, b)


def _row(S, covered, peak, E):
    return (S, covered, peak, E)


def test_host_arithmetic_by_hand_and_against_the_reference(host_lib, tmp_path):
    """The by-hand values of the contract -- uniform coverage 100, one covered base 100 / L, depth 2 on every second base 50; depth 1
    on every second base has a mean depth of 0.5, is not eligible and prints 0 (its 100 exp(H) / L would be 50) --, genes that are too
    short or too thin, an empty one, and the rows of a catalogue case; an odd number of eligible genes."""
    L = [300, 100, 200, 200, 99, 100, 0, 4000]
    rows = np.array([_row(2100, 300, 7, 2100 * math.log2(7)), _row(100, 1, 100, 100 * math.log2(100)), _row(200, 100, 2, 200.0), _row(100, 100, 1, 0.0),
                     _row(990, 99, 10, 990 * math.log2(10)), _row(99, 99, 1, 0.0), _row(0, 0, 0, 0.0), _row(9000, 3000, 5, 9000 * 1.7)], ref.ROW)
    ids = ["G%d" % k for k in range(len(L))]
    tin, mean, stats, text = _host(host_lib, L, rows, tmp_path, ids)
    assert abs(tin[0] - 100) < 1e-9 and abs(tin[1] - 1.0) < 1e-9 and abs(tin[2] - 50) < 1e-9 and tin[3] == tin[4] == tin[5] == tin[6] == 0
    assert abs(ref.tin_formula(200, 100, 0.0) - 50) < 1e-12
    assert mean.tolist() == [7.0, 1.0, 1.0, 0.5, 10.0, 0.99, 0.0, 2.25]
    want_mean, want_tin, el = ref.values(L, rows)
    assert el.tolist() == [True, True, True, False, False, False, False, True] and np.allclose(tin, want_tin, rtol=1e-12, atol=0) and (mean == want_mean).all()
    n, m, med, sd = ref.summary(want_tin, el)
    assert n == 4 == int(stats[0]) and np.allclose(stats[1:], [m, med, sd], rtol=1e-12, atol=0)
    assert abs(med - (want_tin[2] + want_tin[7]) / 2) < 1e-12                      # even: the mean of the two middle ones (1, 50, tin[7], 100)
    _same_text(text[0], ref.render(ids, L, rows), 2)
    _same_text(text[1], ref.render_summary(L, rows), 3)
    assert text[0].split("\n")[1] == "G0\t300\t300\t2100\t7\t7.000000\t100.000000" and text[0].split("\n")[4] == "G3\t200\t100\t100\t1\t0.500000\t0.000000"
    assert text[1].split("\n")[0] == "genes\teligible\tmean\tmedian\tstdev" and text[1].split("\n")[1].split("\t")[:2] == ["8", "4"]
    # an odd count: the middle one
    tin3, _, stats3, _ = _host(host_lib, L[:3], rows[:3])
    assert int(stats3[0]) == 3 and abs(stats3[2] - 50) < 1e-9 and abs(stats3[1] - 151 / 3) < 1e-9
    assert abs(stats3[3] - math.sqrt(((100 - 151 / 3) ** 2 + (1 - 151 / 3) ** 2 + (50 - 151 / 3) ** 2) / 3)) < 1e-9


def test_host_arithmetic_without_an_eligible_gene_and_without_a_gene(host_lib, tmp_path):
    L = [99, 200, 0]
    rows = np.array([_row(990, 99, 10, 990 * math.log2(10)), _row(199, 199, 1, 0.0), _row(0, 0, 0, 0.0)], ref.ROW)
    tin, mean, stats, text = _host(host_lib, L, rows, tmp_path, ["a", "b", "c"])
    assert not tin.any() and stats.tolist() == [0, 0, 0, 0]
    assert text[1] == "genes\teligible\tmean\tmedian\tstdev\n3\t0\t0.000000\t0.000000\t0.000000\n" == ref.render_summary(L, rows)
    _same_text(text[0], ref.render(["a", "b", "c"], L, rows), 2)
    (tmp_path / "none").mkdir()
    _, _, stats0, text0 = _host(host_lib, [], np.zeros(0, ref.ROW), tmp_path / "none", [])
    assert stats0.tolist() == [0, 0, 0, 0] and text0[0] == ref.HEADER and text0[1] == ref.SUMMARY_HEADER + "0\t0\t0.000000\t0.000000\t0.000000\n"


def test_host_arithmetic_on_the_catalogue(host_lib, tmp_path):
    """The rows of the catalogue's cases through the writer: the text of both files against the reference."""
    for name in ("known_depths", "lengths_1_63_64_65_99_100", "item_edges", "zero_segments_and_zero_depth"):
        _, _, _, _, want, _, L = tc.case(name)
        ids = ["gene%d" % g for g in range(len(L))]
        d = tmp_path / name
        d.mkdir()
        _, _, _, text = _host(host_lib, L, want, d, ids)
        _same_text(text[0], ref.render(ids, L, want), 2)
        _same_text(text[1], ref.render_summary(L, want), 3)


# ---- the command line, without a GPU ---------------------------------------------------------------------------------------------------
def _run(cli, args, env=None):
    p = subprocess.run([cli, *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, **(env or {})), timeout=60)
    return p.returncode, p.stdout.decode(), p.stderr.decode()


def test_cli_usage_names_the_flag(cli):
    rc, so, se = _run(cli, ["--help"])
    assert "--tin " in so + se and ".tin.tsv" in so + se and ".tin_summary.tsv" in so + se


def test_cli_refuses_tin_on_several_gpus(cli, tmp_path):
    """Exit 6 before any GPU work (no device is visible: a run that touched one would end with exit 10); no output directory."""
    gtf = tmp_path / "k.gtf"; gtf.write_text(GTF)
    bam = tmp_path / "none.bam"; bam.write_bytes(b"")
    hidden = dict(HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    for args, env in ((["--gpus=2", "--tin"], {}), (["--tin", "--gpus", "2"], {}), (["--tin"], dict(RSQC_GPUS="2")), (["--tin"], dict(RSQC_GPU_LIST="0,1"))):
        out = str(tmp_path / "refused")
        rc, _, se = _run(cli, args + [str(gtf), str(bam), out], env=dict(hidden, **env))
        assert rc == 6 and "--tin runs on one GPU" in se, (args, rc, se)
        assert not os.path.exists(out)
