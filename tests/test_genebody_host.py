"""CPU: --gene-body.  The kernel of rnaseqc_amd/csrc/rsqc_genebody.h, unmodified, with the header's model check and launch plan, on the
64-lane emulation over the edge catalogue (tests/genebody_cases.py) against the numpy restatement of the contract
(tests/genebody_ref.py), round-robin and under seeded schedules (the items of one gene meet in atomics); the exported plan; every model
rule violated once; the same catalogue through a stand-alone sanitizer build of the harness; the command line's usage text and the
refused multi-GPU combination."""
import os
import subprocess

import numpy as np
import pytest

from tests import genebody_cases as gc
from tests import genebody_ref as ref
from tests.hostemu import genebody as emu
from tests.test_cli import cli  # noqa: F401
from tests.test_junction_host import GTF

SEEDS = [0, 7, 1234567]          # 0: round-robin


def _check_plan(model, items, info):
    """The items tile every measured gene's [0, L) exactly once, each at most ITEM bases, with the segment that holds its first base."""
    L = ref.gene_lengths(model)
    seg_len = model["seg_end"].astype(np.int64) - model["seg_start"].astype(np.int64)
    at = {}
    for gene, u0, u1, seg, seg_u, len_rev in items.tolist():
        assert L[gene] >= 100 and (len_rev & 0x7FFFFFFF) == L[gene] and (len_rev >> 31) == int(model["reverse"][gene])
        assert u0 == at.get(gene, 0) and u0 < u1 <= L[gene] and u1 - u0 <= gc.ITEM and (u1 - u0 == gc.ITEM or u1 == L[gene])
        at[gene] = u1
        lo, hi = int(model["seg_off"][gene]), int(model["seg_off"][gene + 1])
        assert lo <= seg < hi
        assert seg_u == int(seg_len[lo:seg].sum()) and seg_u <= u0 < seg_u + int(seg_len[seg])
    assert at == {g: int(L[g]) for g in range(len(L)) if L[g] >= 100}
    assert info["items"] == len(items) == sum(-(-int(x) // gc.ITEM) for x in L if x >= 100)
    assert info["workgroups"] == -(-len(items) // 4)
    assert [int(g) for g in items[:, 0]] == sorted(int(g) for g in items[:, 0])


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("name", gc.SMALL)
def test_catalogue(name, seed):
    lengths, _, model, depth, want, want_info = gc.case(name)
    got, info, items = emu.run(lengths, depth, model, seed=seed)
    ref.assert_equal(got, info, want, want_info)
    _check_plan(model, items, info)


def test_item_edges_take_the_items_they_are_named_for():
    lengths, _, model, depth, _, _ = gc.case("item_edges")
    _, _, items = emu.run(lengths, depth, model)
    per_gene = np.bincount(items[:, 0], minlength=5).tolist()
    assert per_gene == [1, 1, 2, 4, 4]
    g3 = items[items[:, 0] == 3]
    assert g3[:, 1].tolist() == [0, gc.ITEM, 2 * gc.ITEM, 3 * gc.ITEM] and g3[:, 3].tolist() == [3, 4, 4, 5] and g3[:, 4].tolist() == [0, gc.ITEM, gc.ITEM, 2 * gc.ITEM + 700]


@pytest.mark.parametrize("seed", [0, 3])
def test_many_genes(seed):
    """3 000 genes of L = 100 through the kernel (a fiber per lane: the 70 000 of the GPU test would be 4.5 M fibers) ..."""
    lengths, _, model, depth, want, want_info = gc.case("many_genes_of_100", emu=True)
    got, info, items = emu.run(lengths, depth, model, seed=seed)
    ref.assert_equal(got, info, want, want_info)
    _check_plan(model, items, info)
    assert info["workgroups"] == gc.MANY_EMU // 4


def test_plan_of_70000_genes():
    """... and the plan of all 70 000, without the kernel: one item a gene, 17 500 workgroups."""
    model = ref.make_model(gc._many(gc.MANY))
    info, items = emu.plan(model)
    _check_plan(model, items, info)
    assert info["items"] == gc.MANY and info["workgroups"] == gc.MANY // 4 and info["model_bases"] == 100 * gc.MANY


def test_bin_above_2_pow_32():
    """One gene of 7 000 000 bases under depth 70 000 (1 709 items that meet in one row; round-robin only): every bin 4.9e9."""
    lengths, _, model, depth, want, want_info = gc.case("bin_above_2_pow_32")
    got, info, items = emu.run(lengths, depth, model)
    ref.assert_equal(got, info, want, want_info)
    _check_plan(model, items, info)
    assert info["items"] == -(-gc.BIG_L // gc.ITEM) + 1 and info["depth_sum"] == gc.BIG_RECORDS * gc.BIG_L
    assert (got[0] == np.uint64(gc.BIG_RECORDS * (gc.BIG_L // 100))).all() and int(got[0][0]) > 1 << 32


@pytest.mark.parametrize("name", list(gc.BROKEN))
def test_every_model_rule_violated_once(name):
    model, word, gene = gc.broken_model(name)
    with pytest.raises(emu.ModelError) as err:
        emu.run(gc.LENGTHS, [np.zeros(n, np.uint32) for n in gc.LENGTHS], model)
    assert word in str(err.value) and gene in str(err.value), str(err.value)


def test_render_and_model_from_annotation_by_hand():
    """The reference's own pieces on a case small enough to do by hand."""
    from rnaseqc_amd.model import Annotation
    rows = [dict(contig="c1", type="gene", start=101, end=400, strand="-", gene_id="g1"),
            dict(contig="c1", type="exon", start=101, end=200, strand="-", gene_id="g1"), dict(contig="c1", type="exon", start=151, end=250, strand="-", gene_id="g1"),
            dict(contig="c1", type="exon", start=251, end=260, strand="-", gene_id="g1"), dict(contig="c1", type="exon", start=391, end=450, strand="-", gene_id="g1"),
            dict(contig="c2", type="gene", start=1, end=50, strand="+", gene_id="g2"), dict(contig="c2", type="exon", start=1, end=50, strand="+", gene_id="g2"),
            dict(contig="zz", type="gene", start=1, end=500, strand="+", gene_id="g3"), dict(contig="zz", type="exon", start=1, end=500, strand="+", gene_id="g3")]
    ann = Annotation.from_rows(["c1", "c2"], rows)
    m = ref.model_from_annotation(ann, [420, 1000])
    assert m["seg_off"].tolist() == [0, 2, 3, 3] and m["reverse"].tolist() == [1, 0, 0]
    assert list(zip(m["seg_tid"].tolist(), m["seg_start"].tolist(), m["seg_end"].tolist())) == [(0, 100, 260), (0, 390, 420), (1, 0, 50)]
    depth = [np.full(420, 2, np.int64), np.zeros(1000, np.int64)]
    s, info = ref.sums(depth, m)
    assert info == dict(n_genes=3, n_measured=1, model_bases=190, depth_sum=380)
    assert s[0].tolist() == [2 * (-(-(k + 1) * 190 // 100) + (-k * 190 // 100)) for k in range(100)]     # 2 * len_k: one or two bases a bin
    text = ref.render(m, s).split("\n")
    assert text[0] == "bin\tdepth_sum\tgenes\tnorm_mean" and len(text) == 102 and text[-1] == ""
    assert text[1].split("\t")[:3] == ["0", str(int(s[0][0])), "1"] and text[1].split("\t")[3] == "1.000000"      # (uniform depth: every bin at the mean)


def test_catalogue_under_sanitizers(tmp_path):
    """The stand-alone form of the harness built with the address and undefined-behaviour sanitizers, as a child process: the scanned
    array, the model's columns, the plan and the sums have exactly their size there, and __shared__ is static storage."""
    exe = str(tmp_path / "genebody_emu")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-DGBEMU_MAIN", "-DWAVEMU_STACK_BYTES=32768", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wno-unused-function", "-Wno-unused-variable", emu.PROGRAM_SOURCE, "-o", exe])
    for name in gc.SMALL:
        lengths, _, model, depth, want, info = gc.case(name)
        for seed in (0, 5):
            path = str(tmp_path / "case.bin")
            emu.write_case_file(path, lengths, depth, model, seed)
            r = subprocess.run([exe, path], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
            assert r.returncode == 0, (name, seed, r.stdout[-2000:] + r.stderr[-4000:])
            got = dict(kv.split("=") for kv in r.stdout.split()[1:])
            weighted = int((want * np.arange(1, 101, dtype=np.uint64)[None, :]).sum(dtype=np.uint64)) if want.size else 0
            assert (int(got["rc"]), int(got["genes"]), int(got["measured"]), int(got["bases"]), int(got["depth_sum"]), int(got["weighted"])) == \
                (0, info["n_genes"], info["n_measured"], info["model_bases"], info["depth_sum"], weighted), (name, seed, r.stdout)


# ---- the command line, without a GPU ---------------------------------------------------------------------------------------------------
def _run(cli, args, env=None):
    p = subprocess.run([cli, *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, **(env or {})), timeout=60)
    return p.returncode, p.stdout.decode(), p.stderr.decode()


def test_cli_usage_names_the_flag(cli):
    rc, so, se = _run(cli, ["--help"])
    assert "--gene-body" in so + se and ".gene_body.tsv" in so + se


def test_cli_refuses_gene_body_on_several_gpus(cli, tmp_path):
    """Exit 6 before any GPU work (no device is visible: a run that touched one would end with exit 10); no output directory."""
    gtf = tmp_path / "k.gtf"; gtf.write_text(GTF)
    bam = tmp_path / "none.bam"; bam.write_bytes(b"")
    hidden = dict(HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    for args, env in ((["--gpus=2", "--gene-body"], {}), (["--gene-body", "--gpus", "2"], {}), (["--gene-body"], dict(RSQC_GPUS="2")), (["--gene-body"], dict(RSQC_GPU_LIST="0,1"))):
        out = str(tmp_path / "refused")
        rc, _, se = _run(cli, args + [str(gtf), str(bam), out], env=dict(hidden, **env))
        assert rc == 6 and "Argument validation error: --gene-body" in se, (args, rc, se)
        assert not os.path.exists(out)
