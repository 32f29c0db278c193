"""-m gpu: --mark-duplicates on the command line.  An unsorted, unflagged BAM / SAM with the flag gives, file for file, the reports of
--sort on a copy whose 0x400 flags the Python restatement of the contract (tests/markdup_ref.py) wrote; without the flag the same
input reports no duplicates at all; --junctions and --bedgraph files do not depend on the flag."""
import dataclasses
import os
import re
import subprocess

import numpy as np
import pytest

from rnaseqc_amd import abi, bamio, synth
from tests import markdup_cases as mc
from tests import markdup_ref as ref
from tests.test_cli import cli  # noqa: F401

pytestmark = pytest.mark.gpu
CONTIGS = [("chrA", 900_000, 70), ("chrB", 500_000, 40), ("chrC", 300_000, 15)]


def _run(cli, args, env=None, timeout=300):
    p = subprocess.run([cli, *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, **(env or {})), timeout=timeout)
    return p.returncode, p.stdout.decode(), p.stderr.decode()


def _reports(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d))}


def _metric(reports, key):
    for line in reports["x.metrics.tsv"].decode().splitlines():
        k, _, v = line.partition("\t")
        if k == key:
            return v
    raise KeyError(key)


class Case:
    pass


@pytest.fixture(scope="module")
def files(tmp_path_factory, cli):
    d = tmp_path_factory.mktemp("markdupfiles")
    f = Case()
    f.dir = d
    f.ann = synth.make_annotation(seed=51, contigs=CONTIGS)
    b = mc.fixture()
    # what an aligner emits: no record carries 0x400
    f.reads = bamio.sam_consistent(dataclasses.replace(b, flag=(np.asarray(b.flag, np.uint16) & np.uint16(~abi.FDUP & 0xFFFF)).astype(np.uint16)))
    f.verdict, f.info, _ = ref.mark_duplicates([f.reads])
    v0, info0, _ = mc.fixture_expected()
    np.testing.assert_array_equal(f.verdict, v0)                    # (the flags on input decide cleared_records only)
    assert f.info["cleared_records"] == 0 and f.info["duplicate_fragments"] == info0["duplicate_fragments"] > 5_000
    f.flagged = ref.rewrite_flags([f.reads], f.verdict)[0]
    f.paths = dict(gtf=str(d / "m.gtf"), bam=str(d / "in.bam"), sam=str(d / "in.sam"), flagged=str(d / "flagged.bam"))
    bamio.write_gtf(f.paths["gtf"], f.ann)
    bamio.write_bam(f.paths["bam"], mc.CONTIGS, f.reads)
    bamio.write_sam(f.paths["sam"], mc.CONTIGS, f.reads)
    bamio.write_bam(f.paths["flagged"], mc.CONTIGS, f.flagged)
    # the runs every other one is compared with: --sort on the copy the reference flagged, and --sort on the input as it is
    f.want_out, f.plain_out = str(d / "want"), str(d / "plain")
    rc, _, se = _run(cli, ["--sort", f.paths["gtf"], f.paths["flagged"], f.want_out, "-s", "x", "--coverage"])
    assert rc == 0, se
    rc, _, se = _run(cli, ["--sort", f.paths["gtf"], f.paths["bam"], f.plain_out, "-s", "x", "--coverage"])
    assert rc == 0, se
    return f


def _verbose_line(info):
    return ("Duplicates marked: records %d, population %d, anchors %d, sets %d, duplicate_fragments %d, flagged_records %d, cleared_records %d, sig_ms"
            % tuple(info[k] for k in ref.INFO_FIELDS))


@pytest.mark.parametrize("kind", ["bam", "sam"])
def test_reports_equal_sort_on_the_flagged_copy(cli, files, kind):
    out = str(files.dir / ("marked_" + kind))
    env = dict(RSQC_DECODE_CHUNK="65536", RSQC_DECODE_MAX_OUT="262144") if kind == "bam" else dict(RSQC_SAM_CHUNK="100000")     # (many decode windows)
    rc, so, se = _run(cli, ["--mark-duplicates", files.paths["gtf"], files.paths[kind], out, "-s", "x", "-v", "--coverage"], env=env)
    assert rc == 0, se
    got, want = _reports(out), _reports(files.want_out)
    assert sorted(got) == sorted(want) and len(got) >= 5
    for name in want:
        assert got[name] == want[name], name
    assert "Sorted on the GPU: records 40000," in so and _verbose_line(files.info) in so, so


def test_device_memory_of_the_stage_is_what_the_readme_states(cli, files):
    """RSQC_MARKDUP_PROFILE: the bytes the stage holds at its end (nothing is freed before) against the README's statement -- 44 bytes
    per anchor, 4 per 256 records, 4 per table slot, one per record -- plus the sort's digit histograms (4 x 256 per tile of 2048
    anchors: half a byte per anchor, rounded up to a tile) and the small tables -- 48 bytes per workgroup of the key reduction (at most
    86 here), the scans' chunk sums, the batch table, 64 bytes of slack per allocation: under 16 KiB together."""
    out = str(files.dir / "memory")
    rc, _, se = _run(cli, ["--mark-duplicates", files.paths["gtf"], files.paths["bam"], out, "-s", "x"], env=dict(RSQC_MARKDUP_PROFILE="1"))
    assert rc == 0, se
    m = re.search(r"markdup: anchors (\d+), passes_lo (\d+), passes_hi (\d+), radix_bytes (\d+), table_slots (\d+), device_bytes (\d+)", se)
    assert m, se
    anchors, p_lo, p_hi, radix, slots, held = (int(x) for x in m.groups())
    n, dups = files.info["records"], files.info["duplicate_fragments"]
    assert anchors == files.info["anchors"] and slots == 16384 and 2 * dups <= slots < 4 * dups
    assert 1 <= p_lo <= 6 and 2 <= p_hi <= 5 and radix == (p_lo + p_hi) * 24 * anchors      # dead digit positions were skipped in both stages
    stated = 44 * anchors + 4 * ((n + 255) // 256) + 4 * slots + n
    assert stated <= held <= stated + anchors // 2 + 16384, (stated, held)


def test_without_the_flag_the_duplicate_rows_are_zero(files):
    """The behaviour being fixed: --sort alone on the unflagged input reports no duplicates."""
    plain, want = _reports(files.plain_out), _reports(files.want_out)
    assert int(_metric(plain, "Mapped Duplicate Reads")) == 0 and float(_metric(plain, "Duplicate Rate of Mapped")) == 0
    assert int(_metric(want, "Mapped Duplicate Reads")) > 5_000 and float(_metric(want, "Duplicate Rate of Mapped")) > 0.1
    assert int(_metric(plain, "Mapped Unique Reads")) > int(_metric(want, "Mapped Unique Reads"))
    assert plain["x.metrics.tsv"] != want["x.metrics.tsv"]


def test_junctions_and_bedgraph_do_not_depend_on_the_flag(cli, files):
    outs = {}
    for flag in ("--sort", "--mark-duplicates"):
        out = str(files.dir / ("jb_" + flag.strip("-")))
        rc, so, se = _run(cli, [flag, "--junctions", "--bedgraph", files.paths["gtf"], files.paths["bam"], out, "-s", "x", "--coverage"], env=dict(RSQC_SORT_BATCH="9000"))
        assert rc == 0, se
        outs[flag] = _reports(out)
    extra = sorted(set(outs["--sort"]) - set(_reports(files.plain_out)))
    assert len(extra) == 2, extra
    for name in extra:
        assert len(outs["--sort"][name]) > 100 and outs["--mark-duplicates"][name] == outs["--sort"][name], name
    want = _reports(files.want_out)
    for name in want:                                               # ... and the other reports are the marked ones
        assert outs["--mark-duplicates"][name] == want[name], name
