"""CPU: --mark-duplicates.  The kernels of rnaseqc_amd/csrc/rsqc_markdup.h, unmodified, on the 64-lane emulation (mark, signature, both
sort stages with rsqc_sort.h's passes, heads, the name table, apply) against the Python restatement of the contract
(tests/markdup_ref.py), round-robin and under seeded schedules (the table is filled with atomicCAS, the counters with atomicAdd); the
command line's usage text and the refused combinations."""
import os
import subprocess

import numpy as np
import pytest

from rnaseqc_amd import abi
from tests import markdup_cases as mc
from tests import markdup_ref as ref
from tests.hostemu import markdup as emu
from tests.test_cli import cli  # noqa: F401

SEEDS = [0, 7, 1234567]          # 0: round-robin


def _check(batches, want_verdict, want_info, seed=0):
    got = emu.run(batches, seed=seed)
    ref.assert_info_equal(got, want_info)
    np.testing.assert_array_equal(got["verdict"], want_verdict)
    before = np.concatenate([np.asarray(b.flag, np.uint16) for b in batches if b.n] or [np.zeros(0, np.uint16)])
    np.testing.assert_array_equal(got["flag"], (before & np.uint16(~abi.FDUP & 0xFFFF)) | (want_verdict.astype(np.uint16) * np.uint16(abi.FDUP)))
    return got


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("name", mc.CRAFTED_NAMES)
def test_crafted(name, seed):
    b, v, info = mc.crafted_case(name)
    got = _check([b], v, info, seed=seed)
    if info["duplicate_fragments"] == 0:
        assert got["table_slots"] == 0                  # |D| = 0: no name table
    if name == "edge_512_duplicates":
        assert got["table_slots"] == 1024
    if name == "edge_513_duplicates":
        assert got["table_slots"] == 2048
    if name in ("edge_no_population", "anchor_malformed_pairs_have_none"):
        assert got["passes"] == (0, 0)


def test_catalogue_is_complete():
    assert sorted(mc.CRAFTED_NAMES) == sorted(mc.crafted())


def test_crafted_all_in_one_pass():
    """Every case with a qhash2 column as a batch of ONE pass: names and coordinates of different cases meet."""
    batches = [mc.crafted_case(n)[0] for n in mc.CRAFTED_NAMES if n != "names_collide_without_qhash2"]
    v, info, _ = ref.mark_duplicates(batches)
    _check(batches, v, info, seed=5)


def test_fixture_stays_non_trivial():
    b = mc.fixture()
    v, info, detail = mc.fixture_expected()
    assert b.n == info["records"] == 40_000
    kinds = [s[4] for s in detail["signatures"].values()]
    assert kinds.count(ref.PAIR) > 10_000 and kinds.count(ref.SPLIT) > 1_500 and kinds.count(ref.SINGLE) > 5_000
    assert 0.25 < info["duplicate_fragments"] / info["anchors"] < 0.35
    sizes = {}
    for s in detail["signatures"].values():
        sizes[s] = sizes.get(s, 0) + 1
    assert max(sizes.values()) > 2 and sum(1 for x in sizes.values() if x > 2) > 500
    # survivors decided by mapq: sets whose survivor is not their earliest arrival
    first = {}
    for idx in sorted(detail["signatures"]):
        first.setdefault(detail["signatures"][idx], idx)
    assert sum(1 for s, idx in detail["survivors"].items() if first[s] != idx) > 500
    assert info["cleared_records"] > 1_000 and info["flagged_records"] > info["duplicate_fragments"]
    assert info["population"] < 40_000 - 1_400 and info["anchors"] == 22_000


@pytest.mark.parametrize("seed", SEEDS)
def test_fixture_in_five_unequal_batches(seed):
    parts = mc.cut(mc.fixture(), mc.FIXTURE_CUTS)
    assert len(parts) == 5 and len(set(p.n for p in parts)) == 5
    v, info, _ = mc.fixture_expected()
    got = _check(parts, v, info, seed=seed)
    assert 1 <= got["passes"][0] <= 6 and 2 <= got["passes"][1] <= 5       # both stages ran, dead digit positions were skipped


def test_fixture_as_one_batch():
    v, info, _ = mc.fixture_expected()
    _check([mc.fixture()], v, info, seed=3)


def test_fixture_shuffled_in_three_batches():
    """The verdicts follow the arrival order (the tie rule); anchors, sets and duplicate fragments do not depend on it."""
    _, info, _ = mc.fixture_expected()
    parts, (v2, info2, _) = mc.fixture_shuffled()
    assert len(parts) == 3
    _check(parts, v2, info2, seed=11)
    for f in ref.ORDER_FREE_FIELDS:
        assert info[f] == info2[f], f


# ---- the command line, without a GPU ---------------------------------------------------------------------------------------------------
GTF = 'chr1\tt\tgene\t100\t900\t.\t+\t.\tgene_id "G1"; gene_name "g1"; transcript_type "protein_coding";\n' \
      'chr1\tt\texon\t100\t200\t.\t+\t.\tgene_id "G1"; transcript_id "T1"; gene_name "g1"; transcript_type "protein_coding";\n'


def _run(cli, args, env=None):
    p = subprocess.run([cli, *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, **(env or {})), timeout=60)
    return p.returncode, p.stdout.decode(), p.stderr.decode()


def test_cli_usage_names_the_flag(cli):
    rc, so, se = _run(cli, ["--help"])
    text = so + se
    assert "--mark-duplicates" in text and text.index("--sort ") < text.index("--mark-duplicates") < text.index("--junctions")


def test_cli_refuses_the_combinations_sort_refuses(cli, tmp_path):
    """Exit 6 before any GPU work (no device is visible: a run that touched one would end with exit 10); no output directory."""
    gtf = tmp_path / "k.gtf"; gtf.write_text(GTF)
    bam = tmp_path / "none.bam"; bam.write_bytes(b"")
    lst = tmp_path / "two.list"; lst.write_text("%s\n" % bam)
    hidden = dict(HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    out = str(tmp_path / "refused")
    for args, env in ((["--gpus=2", "--mark-duplicates"], {}), (["--mark-duplicates", "--gpus", "2"], {}), (["--mark-duplicates"], dict(RSQC_GPUS="2")),
                      (["--mark-duplicates"], dict(RSQC_GPU_LIST="0,1")), (["--mark-duplicates", "--sort"], dict(RSQC_GPUS="2"))):
        rc, _, se = _run(cli, args + [str(gtf), str(bam), out], env=dict(hidden, **env))
        assert rc == 6 and "Argument validation error: --mark-duplicates" in se, (args, rc, se)
        assert not os.path.exists(out)
    rc, _, se = _run(cli, ["--mark-duplicates", "--bam-list=" + str(lst), str(gtf), out], env=hidden)
    assert rc == 6 and "Argument validation error: --mark-duplicates" in se, (rc, se)
    assert not os.path.exists(out)
