"""CPU: --bedgraph.  The kernels of rnaseqc_amd/csrc/rsqc_track.h, unmodified, on the 64-lane emulation (events, the scan of
rsqc_sort.h, head count, rows, line lengths, format) against the numpy restatement of the contract (tests/track_ref.py), round-robin
and under seeded schedules (the kernels use atomics), with the later events merged and lane by lane; the text kernels on injected
rows with 10-digit coordinates; the command line's usage text and the refused multi-GPU combination."""
import os
import subprocess

import numpy as np
import pytest

from tests import junction_cases as jc
from tests import track_cases as tc
from tests import track_ref as ref
from tests.hostemu import track as emu
from tests.test_cli import cli  # noqa: F401
from tests.test_junction_host import GTF

SEEDS = [0, 7, 1234567]          # 0: round-robin


def _check(batches, want, lengths, names, seed=0, merge_later=False, windows=None):
    got = emu.run(batches, lengths, names, merge_later=merge_later, seed=seed, windows=windows)
    ref.assert_tracks_equal(got, want)
    assert ref.covered(got) == got["aligned_bases"]
    assert got["text"] == ref.render(want, names)
    return got


def test_fixture_a_stays_non_trivial():
    _, reads = jc.fixture_a()
    w = tc.fixture_a_track()
    assert reads.n == 41_000 and w["population"] == jc.fixture_a_table()["population"] == 40_000
    assert w["n_rows"] > 1_000 and w["max_depth"] > 100 and w["positions"] == 1_700_000
    assert ref.covered(w) == w["aligned_bases"] > 1_000_000
    c = tc.fixture_a_track(clipped=True)            # fixture A stays inside its contigs: three records are added that do not
    assert w["clipped_bases"] == 0 and c["clipped_bases"] == 60 + 19 + 30 and c["population"] == w["population"] + 3


@pytest.mark.parametrize("seed", SEEDS)
def test_fixture_a_in_five_unequal_batches(seed):
    _, reads = jc.fixture_a()
    parts = tc.cut(reads)
    assert len(parts) == 5 and len(set(p.n for p in parts)) == 5
    got = _check(parts, tc.fixture_a_track(), tc.A_LENGTHS, tc.A_NAMES, seed=seed, merge_later=bool(seed == 7))
    assert got["chunks"] == -(-(1_700_000 + 3) // tc.CHUNK)


def test_fixture_a_other_order_other_cut_with_clipped_records():
    """The table does not depend on the order of the records or on the batches; text in windows of 4 097 rows joins to the whole."""
    reads, extra = tc.fixture_a_clipped()
    shuffled = reads.take(np.random.default_rng(5).permutation(reads.n))
    _check(tc.cut(shuffled, seed=9, parts=3) + [extra], tc.fixture_a_track(clipped=True), tc.A_LENGTHS, tc.A_NAMES, seed=3, merge_later=True, windows=4097)


@pytest.mark.parametrize("merge_later", [False, True])
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("name", tc.CRAFTED_NAMES + list(tc.EMU_ONLY))
def test_crafted(name, seed, merge_later):
    batches, want = tc.crafted_case(name)
    got = _check(batches, want, tc.LENGTHS, tc.NAMES, seed=seed, merge_later=merge_later, windows=64)
    if want["n_rows"] == 0:
        assert got["text"] == b""


def test_crafted_all_in_one_pass():
    """Every crafted case as a batch of ONE pass: the depths of different batches add up."""
    batches = [b for n in tc.CRAFTED_NAMES for b in tc.crafted_case(n)[0]]
    _check(batches, ref.track(batches, tc.LENGTHS), tc.LENGTHS, tc.NAMES, seed=5)


def test_ten_digit_coordinates_on_injected_rows():
    """Starts, ends and depths at every digit-count edge up to 2^31 - 1 and 2^32 - 1: the line-length and format kernels on rows the
    suite cannot reach through a difference array (a contig of 10^9 positions is a 4 GB array), against Python's %d."""
    edges = [0, 9, 10, 99, 100, 999, 1000, 99_999, 100_000, 9_999_999, 10_000_000, 99_999_999, 100_000_000, 999_999_999, 1_000_000_000, 2_147_483_647]
    depths = [1, 9, 10, 99, 100, 999_999_999, 1_000_000_000, 4_294_967_295]
    names = ["c", "chr_with_a_longer_name.1", "x" * 255]
    rows = [(k % 3, s, e, depths[(k + j) % len(depths)]) for k, s in enumerate(edges) for j, e in enumerate(edges)]
    assert len(rows) == 256
    rows += [(2, 2_147_483_646, 2_147_483_647, 4_294_967_295)]       # (a second workgroup)
    tid, start, end, depth = (np.array([r[k] for r in rows], np.int64) for k in range(4))
    want = "".join("%s\t%d\t%d\t%d\n" % (names[t], s, e, d) for t, s, e, d in rows).encode()
    assert emu.format_rows(names, tid, start, end, depth) == want
    assert emu.format_rows(names, tid[:1], start[:1], end[:1], depth[:1]) == b"c\t0\t0\t1\n"
    assert emu.format_rows(names, tid[:0], start[:0], end[:0], depth[:0]) == b""


# ---- the command line, without a GPU ---------------------------------------------------------------------------------------------------
def _run(cli, args, env=None):
    p = subprocess.run([cli, *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, **(env or {})), timeout=60)
    return p.returncode, p.stdout.decode(), p.stderr.decode()


def test_cli_usage_names_the_flag(cli):
    rc, so, se = _run(cli, ["--help"])
    assert "--bedgraph" in so + se and ".coverage.bedgraph" in so + se


def test_cli_refuses_bedgraph_on_several_gpus(cli, tmp_path):
    """Exit 6 before any GPU work (no device is visible: a run that touched one would end with exit 10); no output directory."""
    gtf = tmp_path / "k.gtf"; gtf.write_text(GTF)
    bam = tmp_path / "none.bam"; bam.write_bytes(b"")
    hidden = dict(HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    for args, env in ((["--gpus=2", "--bedgraph"], {}), (["--bedgraph", "--gpus", "2"], {}), (["--bedgraph"], dict(RSQC_GPUS="2")), (["--bedgraph"], dict(RSQC_GPU_LIST="0,1"))):
        out = str(tmp_path / "refused")
        rc, _, se = _run(cli, args + [str(gtf), str(bam), out], env=dict(hidden, **env))
        assert rc == 6 and "Argument validation error: --bedgraph" in se, (args, rc, se)
        assert not os.path.exists(out)
