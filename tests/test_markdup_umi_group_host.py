"""CPU: UMIs one substitution apart grouped before duplicate marking (rsqc_markdup_umi_edits(1), --umi-edits=1).  The stage's kernels
(rnaseqc_amd/csrc/rsqc_markdup.h: heads_pos, group_nodes, group_parents, group_roots, group_marks between the UMI mode's sort and the
list), unmodified, on the 64-lane emulation against the Python restatement of the contract (tests/markdup_umi_group_ref.py), round-robin
and under seeded schedules: verdicts, the three info structs and the root of every anchor; the command line's usage text and the
refused combinations."""
import os
import subprocess

import numpy as np
import pytest

from rnaseqc_amd import abi
from tests import markdup_cases as mc
from tests import markdup_ref as ref
from tests import markdup_umi_group_cases as gc
from tests import markdup_umi_group_ref as gref
from tests import markdup_umi_ref as uref
from tests.hostemu import markdup_umi_group as emu
from tests.test_cli import cli  # noqa: F401

SEEDS = [0, 7, 1234567]          # 0: round-robin


def _check(batches, want, seed=0):
    want_verdict, want_info, want_umi, want_group, want_roots = want
    got = emu.run(batches, seed=seed)
    ref.assert_info_equal(got, want_info)
    uref.assert_umi_info_equal(got, want_umi)
    gref.assert_group_info_equal(got, want_group)
    np.testing.assert_array_equal(got["verdict"], want_verdict)
    assert got["roots"] == want_roots
    before = np.concatenate([np.asarray(b.flag, np.uint16) for b in batches if b.n] or [np.zeros(0, np.uint16)])
    np.testing.assert_array_equal(got["flag"], (before & np.uint16(~abi.FDUP & 0xFFFF)) | (want_verdict.astype(np.uint16) * np.uint16(abi.FDUP)))
    assert got["duplicate_fragments"] == got["exact_duplicate_fragments"] + got["merged_nodes"]
    assert got["position_duplicate_fragments"] >= got["duplicate_fragments"] >= got["exact_duplicate_fragments"]
    assert got["position_sets"] == got["anchors"] - got["position_duplicate_fragments"]
    return got


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("name", gc.CRAFTED_NAMES)
def test_crafted(name, seed):
    batches, *want = gc.crafted_case(name)
    got = _check(batches, want, seed=seed)
    if name == "threshold_2_2":
        assert got["probes"] == 2 * 3 * 8               # every node of a set with company looks up its 3 L neighbours
    if name == "lengths_never_merge":
        assert got["probes"] == 3 * (4 + 3 + 5)
    if name == "key_0_never_merges":
        assert got["probes"] == 2 * 3                   # the key-0 node looks nothing up
    if name == "neighbour_in_the_next_position_set":
        assert got["probes"] == 6 * 3 * 4               # a set of one node looks nothing up either


def test_catalogue_is_complete():
    assert sorted(gc.CRAFTED_NAMES) == sorted(gc.crafted())


def test_the_catalogue_tells_the_parent_rules_apart():
    """With parent = the eligible neighbour of the smallest key (instead of the highest count) the case made for it comes out wrong, its
    twin with equal counts -- where both rules agree -- does not."""
    batches, v, info, _uinfo, _ginfo, roots = gc.crafted_case("two_parents_count_wins")
    wrong = emu.run(batches, smallest_key_parent=True)
    assert wrong["roots"] != roots and not np.array_equal(wrong["verdict"], v)
    assert wrong["duplicate_fragments"] == info["duplicate_fragments"]         # the figures alone would not have told
    right = emu.run(batches)
    assert right["roots"] == roots and np.array_equal(right["verdict"], v)
    batches, v, _info, _uinfo, _ginfo, roots = gc.crafted_case("two_parents_key_breaks_tie")
    same = emu.run(batches, smallest_key_parent=True)
    assert same["roots"] == roots and np.array_equal(same["verdict"], v)
    told = [n for n in gc.CRAFTED_NAMES if emu.run(gc.crafted_case(n)[0], smallest_key_parent=True)["roots"] != gc.crafted_case(n)[5]]
    assert "two_parents_count_wins" in told


def test_crafted_all_in_one_pass():
    batches = [b for n in gc.CRAFTED_NAMES for b in gc.crafted_case(n)[0]]
    _check(batches, gref.mark_duplicates_umi_group(batches), seed=5)


def test_exact_matching_is_the_grouping_without_merges():
    """On the cases where nothing merges the grouped result IS markdup_umi_ref's."""
    for name in ("threshold_2_2", "threshold_4_3", "lengths_never_merge", "neighbour_in_the_next_position_set"):
        batches, v, info, uinfo, _g, _r = gc.crafted_case(name)
        ev, einfo, euinfo, _ = uref.mark_duplicates_umi(batches)
        np.testing.assert_array_equal(v, ev)
        assert info == einfo and uinfo == euinfo


@pytest.mark.parametrize("seed", [0, 99])
def test_fixture(seed):
    _check([gc.fixture()], gc.fixture_expected(), seed=seed)


def test_fixture_in_batches_and_shuffled():
    want = gc.fixture_expected()
    _check(mc.cut(gc.fixture(), gc.FIXTURE_CUTS), want)
    parts, shuffled = gc.fixture_shuffled()
    _check(parts, shuffled)
    for f in ref.ORDER_FREE_FIELDS:
        assert shuffled[1][f] == want[1][f]
    assert shuffled[2] == want[2] and shuffled[3] == want[3]
    assert sorted(shuffled[4].values()) == sorted(want[4].values())


# ---- the command line: usage and refusals need no GPU -------------------------------------------------------------------------------
def test_usage_lists_the_flag(cli):
    out = subprocess.run([cli, "--help"], capture_output=True, text=True)
    assert "--umi-edits=[N]" in out.stdout + out.stderr


@pytest.mark.parametrize("args,env", [
    (["--umi-tag=RX", "--umi-edits=2"], {}), (["--umi-qname", "--umi-edits=-1"], {}), (["--umi-tag=RX", "--umi-edits="], {}), (["--umi-tag=RX", "--umi-edits=one"], {}),
    (["--umi-edits=1"], {}), (["--umi-edits=0"], {}), (["--mark-duplicates", "--umi-edits=1"], {}),
    (["--umi-tag=RX", "--umi-edits=1", "--gpus", "2"], {}), (["--umi-qname", "--umi-edits=1"], {"RSQC_GPUS": "2"}),
    (["--umi-tag=RX", "--umi-qname", "--umi-edits=1"], {}), (["--umi-tag=R", "--umi-edits=1"], {}),
])
def test_refusals_exit_6_before_any_gpu_work(cli, tmp_path, args, env):
    """Refused at validation: exit 6, nothing read, no context made (the inputs do not even exist)."""
    e = dict(os.environ, **env)
    e["HIP_VISIBLE_DEVICES"] = ""                       # a context could not be made: reaching that point would not be exit 6
    out = subprocess.run([cli, *args, str(tmp_path / "no.gtf"), str(tmp_path / "no.bam"), str(tmp_path / "out")], capture_output=True, text=True, env=e)
    assert out.returncode == 6, (out.returncode, out.stderr)
    assert not (tmp_path / "out").exists()


def test_refused_with_a_bam_list(cli, tmp_path):
    out = subprocess.run([cli, "--umi-tag=RX", "--umi-edits=1", "--bam-list", str(tmp_path / "list.txt"), str(tmp_path / "no.gtf"), str(tmp_path / "out")], capture_output=True, text=True,
                         env=dict(os.environ, HIP_VISIBLE_DEVICES=""))
    assert out.returncode == 6, (out.returncode, out.stderr)
