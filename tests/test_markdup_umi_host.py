"""CPU: UMI-aware duplicate marking.  rsqc_umi_pack of the library against the Python definition; the stage's kernels in the UMI mode
(rnaseqc_amd/csrc/rsqc_markdup.h: umi_keys, heads_umi and the four sort stages), unmodified, on the 64-lane emulation against the Python
restatement of the contract (tests/markdup_umi_ref.py), round-robin and under seeded schedules; the command line's usage text and the
refused combinations."""
import os
import subprocess

import numpy as np
import pytest

from rnaseqc_amd import abi, engine, synth
from tests import markdup_ref as ref
from tests import markdup_umi_cases as uc
from tests import markdup_umi_ref as uref
from tests.hostemu import markdup_umi as emu
from tests.test_cli import cli  # noqa: F401

SEEDS = [0, 7, 1234567]          # 0: round-robin

PACK_INPUTS = ["", "A", "AA", "AAA", "ACGT" * 7 + "ACG", "ACGT" * 8, "acgtacgt", "AcGtaCgT", "NCGTACGT", "ACGTACGN", "ACGT-TGCA", "ACGT+TGCA", "ACGTTGCA", "-", "+", "-+-",
                "ACGT TGCA", "ACGU", "T" * 31, "T" * 32, "A-" * 31, "A-" * 32, "ACGT\x00", "\xc1CGT", "!CGT", "aCgT-"]


@pytest.mark.parametrize("text", PACK_INPUTS)
def test_pack_matches_the_python_definition(text):
    got = engine.umi_pack(text.encode("latin-1"))
    assert got == uref.umi_pack(text) == abi.umi_pack(text.encode("latin-1"))


def test_pack_by_hand():
    p = lambda t: engine.umi_pack(t.encode("latin-1"))
    assert p("") == 0 and p("-") == 0 and p("N") == 0
    assert (p("A"), p("AA"), p("AAA")) == (4, 16, 64)                      # the length is part of the key
    assert p("ACGT") == (1 << 8) | 0b00011011 and p("T") == 7 and p("acgt") == p("ACGT")
    assert p("ACGT-TGCA") == p("ACGT+TGCA") == p("ACGTTGCA") != 0
    assert p("T" * 31) == (1 << 63) - 1 and p("A" * 31) == 1 << 62 and p("T" * 32) == 0
    assert p("NCGTACGT") == 0 and p("ACGTACGN") == 0
    keys = {p(uc._text(k, 5)) for k in range(1 << 10)}
    assert len(keys) == 1 << 10 and 0 not in keys                          # exact: no two UMIs share a key
    for k in (0, 1, 12345, (1 << 20) - 1):
        assert abi.umi_text(p(uc._text(k, 10))).decode() == uc._text(k, 10)


def _check(batches, want_verdict, want_info, want_umi, seed=0):
    got = emu.run(batches, seed=seed)
    ref.assert_info_equal(got, want_info)
    uref.assert_umi_info_equal(got, want_umi)
    np.testing.assert_array_equal(got["verdict"], want_verdict)
    before = np.concatenate([np.asarray(b.flag, np.uint16) for b in batches if b.n] or [np.zeros(0, np.uint16)])
    np.testing.assert_array_equal(got["flag"], (before & np.uint16(~abi.FDUP & 0xFFFF)) | (want_verdict.astype(np.uint16) * np.uint16(abi.FDUP)))
    return got


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("name", uc.CRAFTED_NAMES)
def test_crafted(name, seed):
    batches, v, info, uinfo = uc.crafted_case(name)
    got = _check(batches, v, info, uinfo, seed=seed)
    if info["duplicate_fragments"] == 0:
        assert got["table_slots"] == 0
    if name == "all_umis_equal":
        assert got["passes_umi"] == 0                   # dead digit positions are skipped: equal keys need no pass at all
    if name == "same_signature_other_umi":
        assert got["passes_umi"] == 1 and got["passes_mapq"] == 0 and got["passes_lo"] == 0 and got["passes_hi"] == 0
    if name == "all_umis_distinct":
        assert got["passes_umi"] == 1                   # 40 UMIs of 8 bases that differ in their last three: one live digit of 8


def test_catalogue_is_complete():
    assert sorted(uc.CRAFTED_NAMES) == sorted(uc.crafted())


def test_position_duplicates_are_plain_markdups_on_every_case():
    for name in uc.CRAFTED_NAMES:
        batches, _v, _info, uinfo = uc.crafted_case(name)
        assert uinfo["position_duplicate_fragments"] == ref.mark_duplicates(batches)[1]["duplicate_fragments"], name


def test_the_catalogue_tells_the_sort_orders_apart():
    """With the UMI ranked BELOW the mapq byte, equal signature-plus-UMI anchors of different mapq are not adjacent: the harness's
    wrong order miscounts the case made for it, the right one does not."""
    batches, v, info, _uinfo = uc.crafted_case("mapq_interleaved_with_other_umi")
    wrong = emu.run(batches, umi_below_mapq=True)
    assert wrong["duplicate_fragments"] != info["duplicate_fragments"] or not np.array_equal(wrong["verdict"], v)
    right = emu.run(batches)
    assert right["duplicate_fragments"] == info["duplicate_fragments"] == 2


def test_crafted_all_in_one_pass():
    batches = [b for n in uc.CRAFTED_NAMES for b in uc.crafted_case(n)[0]]
    v, info, uinfo, _ = uref.mark_duplicates_umi(batches)
    _check(batches, v, info, uinfo, seed=5)


def test_ten_base_umis_have_three_live_digits():
    """A 10-base UMI is 21 bits: 3 live digit positions of 8, the other five are skipped."""
    r = np.random.default_rng(9)
    recs = []
    for i in range(600):
        recs += uc.with_umi(uc.single("r%d" % i, 100 + int(r.integers(0, 5)), mapq=int(r.integers(0, 3))), uc._text(int(r.integers(0, 1 << 20)), 10))
    batches = [uc.to_batch(recs)]
    v, info, uinfo, _ = uref.mark_duplicates_umi(batches)
    got = _check(batches, v, info, uinfo)
    assert got["passes_umi"] == 3 and got["passes_mapq"] == 1


@pytest.mark.parametrize("seed", [0, 99])
def test_fixture(seed):
    v, info, uinfo, _ = uc.fixture_expected()
    _check([uc.fixture()], v, info, uinfo, seed=seed)


def test_fixture_in_batches_and_shuffled():
    v, info, uinfo, _ = uc.fixture_expected()
    from tests import markdup_cases as mc
    _check(mc.cut(uc.fixture(), uc.FIXTURE_CUTS), v, info, uinfo)
    parts, (sv, sinfo, suinfo, _) = uc.fixture_shuffled()
    _check(parts, sv, sinfo, suinfo)
    for f in ref.ORDER_FREE_FIELDS:
        assert sinfo[f] == info[f]
    assert suinfo == uinfo


def test_synth_umi_option_leaves_the_other_columns_alone():
    ann = synth.make_annotation(seed=5, contigs=[("chrA", 400_000, 40)])
    a = synth.make_reads(ann, 500, seed=6, contig_lengths=np.array([400_000]))
    b = synth.make_reads(ann, 500, seed=6, contig_lengths=np.array([400_000]), umi_bases=10)
    assert a.umi is None and b.umi is not None and len(b.umi) == b.n
    for f in ("pos", "mpos", "isize", "qhash", "flag", "mapq", "cigar", "qhash2"):
        np.testing.assert_array_equal(getattr(a, f), getattr(b, f))
    assert ((b.umi >> np.uint64(20)) == 1).all()        # ten bases each
    by_name = {}
    for h, u in zip(b.qhash, b.umi):
        assert by_name.setdefault(int(h), int(u)) == int(u)       # one UMI per fragment
    assert len(set(by_name.values())) > len(by_name) // 2
    assert b.slice(10, 20).umi.tolist() == b.umi[10:20].tolist() and b.take([3, 1]).umi.tolist() == [int(b.umi[3]), int(b.umi[1])]


def test_fast_writer_turns_the_umi_column_into_rx_tags(tmp_path):
    """bamio.write_bam_fast (the input of tools/markdup_umi_bench.py): every record's key comes back from its RX:Z tag through the
    product's own bam_parse_record; a batch without the column gets the bytes it always got."""
    import struct
    from rnaseqc_amd import bamio
    from tests.hostemu import decode, umi as parse
    b = uc.fixture()
    for with_column in (True, False):
        batch = b
        if not with_column:
            import copy
            batch = copy.copy(b); batch.umi = None
        path = str(tmp_path / ("rx%d.bam" % with_column))
        bamio.write_bam_fast(path, uc.CONTIGS, batch, threads=2)
        s, pos, _n_ref = decode.inflate_bam(path, use_emu=False)
        parse.setup(parse.TAG, "RX")
        keys = []
        while pos < len(s):
            bs = struct.unpack_from("<I", s, pos)[0]
            keys.append(parse.parse_bam(s[pos:pos + 4 + bs])["umi"])
            pos += 4 + bs
        assert keys == ([int(k) for k in b.umi] if with_column else [0] * b.n)
        assert (b"RXZ" in s) == with_column


# ---- the command line: usage and refusals need no GPU -------------------------------------------------------------------------------
def test_usage_lists_the_flags(cli):
    out = subprocess.run([cli, "--help"], capture_output=True, text=True)
    assert "--umi-tag=[XX]" in out.stdout + out.stderr and "--umi-qname=[C]" in out.stdout + out.stderr


@pytest.mark.parametrize("args,env", [
    (["--umi-tag=RX", "--umi-qname"], {}),
    (["--umi-tag=R"], {}), (["--umi-tag=RXX"], {}), (["--umi-tag="], {}),
    (["--umi-qname=__"], {}), (["--umi-qname="], {}),
    (["--umi-tag=RX", "--gpus", "2"], {}), (["--umi-qname", "--gpus=2"], {}),
    (["--umi-tag=RX"], {"RSQC_GPUS": "2"}), (["--umi-qname=:"], {"RSQC_GPU_LIST": "0,1"}),
])
def test_refusals_exit_6_before_any_gpu_work(cli, tmp_path, args, env):
    """Refused at validation: exit 6, nothing read, no context made (the inputs do not even exist)."""
    e = dict(os.environ, **env)
    e["HIP_VISIBLE_DEVICES"] = ""                       # a context could not be made: reaching that point would not be exit 6
    out = subprocess.run([cli, *args, str(tmp_path / "no.gtf"), str(tmp_path / "no.bam"), str(tmp_path / "out")], capture_output=True, text=True, env=e)
    assert out.returncode == 6, (out.returncode, out.stderr)
    assert not (tmp_path / "out").exists()


def test_refused_with_a_bam_list(cli, tmp_path):
    out = subprocess.run([cli, "--umi-tag=RX", "--bam-list", str(tmp_path / "list.txt"), str(tmp_path / "no.gtf"), str(tmp_path / "out")], capture_output=True, text=True,
                         env=dict(os.environ, HIP_VISIBLE_DEVICES=""))
    assert out.returncode == 6, (out.returncode, out.stderr)
