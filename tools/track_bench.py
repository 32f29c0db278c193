"""What --bedgraph costs: the synthetic records of tools/sam_bench.py (seq_mode 1) as one BAM, and the command line on it in three
configurations, interleaved, `--reps` rounds, by the reference's `Average Reads/Sec` window:

    (a) parent        the binary of the commit before the feature (--parent-bin), without the flag
    (b) plain         this tree's binary without the flag
    (c) bedgraph      this tree's binary with --bedgraph

(b) against (a) is the check that the feature costs nothing when it is off: it passes when the difference of the medians lies
within the spread (max - min) of (a)'s own runs.  (c) against (b) is the price of the feature, reported as measured, with the
fields of the two -v lines: population, bases, rows, events_ms, scan_ms, rows_ms, and the text stage's rows, bytes, seconds and
GB/s (formatting on the device, the copy and the file write together).  The reports of (b) and (c) are compared (every file but
the track must be byte-identical).

Then the deep pile: the same records with a tenth of them moved into one exon-sized region of chr1 (2 000 positions, the file sorted
again), --bedgraph with the events behind a record's first added lane by lane (RSQC_TRACK_MERGE=0) and merged like the first
(RSQC_TRACK_MERGE=1), interleaved; events_ms of each is the basis for the default.

    python tools/track_bench.py --parent-bin PATH/rnaseqc [--records 10000000] [--reps 3] [--out profiles] [--tmp DIR]

Without --parent-bin configuration (a) is left out.  --genome-scale adds one pass through the C ABI with a track of 3.1 G positions
(a 12.4 GB array) and a thousand reads: scan_ms and rows_ms at the size of a human genome, where the scan's one-workgroup top stage
sees 757 k chunk sums.  Writes <out>/track_rates.json."""
import argparse
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from rnaseqc_amd import bamio, synth  # noqa: E402

CLI = os.path.join(ROOT, "rnaseqc_amd", "bin", "rnaseqc")
NUM = r"([0-9.e+-]+)"
TRACK_LINE = re.compile(r"Track: population (\d+), aligned_bases (\d+), clipped_bases (\d+), rows (\d+), events_ms %s, scan_ms %s, rows_ms %s" % (NUM, NUM, NUM))
TEXT_LINE = re.compile(r"Track text: rows (\d+), bytes (\d+), seconds %s" % NUM)
PILE_WIDTH = 2000


def run_cli(binary, gtf, path, out, bedgraph, env=None, timeout=1200):
    t0 = time.time()
    p = subprocess.run([binary] + (["--bedgraph"] if bedgraph else []) + [gtf, path, out, "-s", "x", "-vv"], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       env=dict(os.environ, **(env or {})), timeout=timeout)
    wall = time.time() - t0
    so, se = p.stdout.decode(), p.stderr.decode()
    if p.returncode:
        raise RuntimeError("%s %s: exit %d\n%s" % (binary, path, p.returncode, se[-2000:]))
    m = re.search(r"Average Reads/Sec: ([0-9.e+]+)", so)
    r = dict(reads_per_s_window=float(m.group(1)) if m else None, wall_s=wall)
    t = TRACK_LINE.search(so)
    if t:
        r["track"] = dict(population=int(t.group(1)), aligned_bases=int(t.group(2)), clipped_bases=int(t.group(3)), rows=int(t.group(4)), events_ms=float(t.group(5)),
                          scan_ms=float(t.group(6)), rows_ms=float(t.group(7)))
    x = TEXT_LINE.search(so)
    if x:
        secs = float(x.group(3))
        r["text"] = dict(rows=int(x.group(1)), bytes=int(x.group(2)), seconds=secs, gb_per_s=int(x.group(2)) / secs / 1e9 if secs else None)
    return r


def other_reports_equal(a, b):
    fa = sorted(f for f in os.listdir(a) if not f.endswith(".coverage.bedgraph"))
    fb = sorted(f for f in os.listdir(b) if not f.endswith(".coverage.bedgraph"))
    return fa == fb and all(open(os.path.join(a, f), "rb").read() == open(os.path.join(b, f), "rb").read() for f in fa)


def deep_pile(batch, seed=63):
    """A tenth of the records, taken from the first contig, moved into PILE_WIDTH positions of it; coordinate order restored."""
    tid = batch.tid_per_record()
    on_first = np.flatnonzero(tid == 0)
    r = np.random.default_rng(seed)
    moved = r.choice(on_first, min(batch.n // 10, len(on_first)), replace=False)
    pos = np.array(batch.pos, copy=True)
    pos[moved] = 20_000_000 + r.integers(0, PILE_WIDTH, len(moved))
    batch.pos = pos
    return batch.coordinate_sorted(), len(moved)


def genome_scale():
    """scan_ms and rows_ms of rsqc_track_end over 3.1 G positions (two contigs), nearly empty."""
    from rnaseqc_amd import abi, engine
    lengths = [2_000_000_000, 1_100_000_000]
    ann = synth.make_annotation(seed=61, contigs=[("chr1", 1_000_000, 20), ("chr2", 1_000_000, 20)])
    reads = synth.make_reads(ann, 1000, seed=62, contig_lengths=np.array([1_000_000, 1_000_000]))
    e = engine.Engine(abi.default_params())
    try:
        e.set_annotation(ann)
        t0 = time.time()
        e.track_begin(lengths, ["chr1", "chr2"])
        begin_s = time.time() - t0
        e.submit(reads)
        e.finalize()
        info = e.track_end()
        t0 = time.time()
        text = e.track_text(0, min(info["n_rows"], 4194304))
        return dict(info, array_bytes=4 * (sum(lengths) + 3), begin_s=begin_s, text_s=time.time() - t0, text_bytes=len(text))
    finally:
        e.close()


def median_of(runs, section, keys):
    return {k: statistics.median(r[section][k] for r in runs) for k in keys}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-bin", default=None, help="the rnaseqc binary of the commit before the feature (its library beside it, as `make variant` lays them out)")
    ap.add_argument("--records", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--tmp", default=None)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--genome-scale", action="store_true")
    a = ap.parse_args()
    tmp = tempfile.mkdtemp(dir=a.tmp)
    try:
        contigs = [("chr%d" % k, 50_000_000, 600) for k in range(1, 5)]
        ann = synth.make_annotation(seed=61, contigs=contigs)
        t0 = time.time()
        batch = bamio.sam_consistent(synth.make_reads(ann, a.records // 2, seed=62, contig_lengths=np.array([c[1] for c in contigs])))
        cs = [(c[0], c[1]) for c in contigs]
        bam, deep_bam, gtf = os.path.join(tmp, "x.bam"), os.path.join(tmp, "deep.bam"), os.path.join(tmp, "x.gtf")
        bamio.write_gtf(gtf, ann)
        bamio.write_bam_fast(bam, cs, batch, threads=a.threads, seq_mode=1)
        res = dict(records=int(batch.n), positions=sum(c[1] for c in contigs), input_s=time.time() - t0, bam_bytes=os.path.getsize(bam), reps=a.reps, runs={})
        configs = ([("parent", a.parent_bin, False)] if a.parent_bin else []) + [("plain", CLI, False), ("bedgraph", CLI, True)]
        for rep in range(a.reps):                               # interleaved: drift of the box lands on every configuration alike
            for name, binary, flag in configs:
                out = os.path.join(tmp, "out_" + name)
                shutil.rmtree(out, ignore_errors=True)
                r = run_cli(binary, gtf, bam, out, flag)
                res["runs"].setdefault(name, []).append(r)
                print(rep, name, json.dumps(r), flush=True)
        rates = {n: [r["reads_per_s_window"] for r in rs] for n, rs in res["runs"].items()}
        med = {n: statistics.median(v) for n, v in rates.items()}
        res["median_reads_per_s_window"] = med
        res["other_reports_equal_plain"] = other_reports_equal(os.path.join(tmp, "out_plain"), os.path.join(tmp, "out_bedgraph"))
        res["track_file_bytes"] = os.path.getsize(os.path.join(tmp, "out_bedgraph", "x.coverage.bedgraph"))
        if a.parent_bin:
            spread = max(rates["parent"]) - min(rates["parent"])
            res["off_check"] = dict(parent_median=med["parent"], plain_median=med["plain"], difference=med["plain"] - med["parent"], parent_spread=spread,
                                    within_parent_spread=abs(med["plain"] - med["parent"]) <= spread)
            res["reports_equal_parent"] = other_reports_equal(os.path.join(tmp, "out_parent"), os.path.join(tmp, "out_plain"))
        res["price"] = dict(plain_median=med["plain"], bedgraph_median=med["bedgraph"], ratio=med["bedgraph"] / med["plain"])
        on = res["runs"]["bedgraph"]
        res["track_median"] = median_of(on, "track", ("population", "aligned_bases", "clipped_bases", "rows", "events_ms", "scan_ms", "rows_ms"))
        res["text_median"] = median_of(on, "text", ("rows", "bytes", "seconds", "gb_per_s"))
        # ---- the deep pile: later events lane by lane against merged
        t0 = time.time()
        deep, moved = deep_pile(batch)
        bamio.write_bam_fast(deep_bam, cs, deep, threads=a.threads, seq_mode=1)
        res["deep_pile"] = dict(moved_records=int(moved), width=PILE_WIDTH, input_s=time.time() - t0, runs={})
        for rep in range(a.reps):
            for name, merge in (("lane_by_lane", "0"), ("merged", "1")):
                out = os.path.join(tmp, "out_deep_" + name)
                shutil.rmtree(out, ignore_errors=True)
                r = run_cli(CLI, gtf, deep_bam, out, True, env=dict(RSQC_TRACK_MERGE=merge))
                res["deep_pile"]["runs"].setdefault(name, []).append(r)
                print(rep, "deep", name, json.dumps(r), flush=True)
        same = open(os.path.join(tmp, "out_deep_lane_by_lane", "x.coverage.bedgraph"), "rb").read() == open(os.path.join(tmp, "out_deep_merged", "x.coverage.bedgraph"), "rb").read()
        res["deep_pile"]["tracks_equal"] = same
        res["deep_pile"]["events_ms_median"] = {n: statistics.median(r["track"]["events_ms"] for r in rs) for n, rs in res["deep_pile"]["runs"].items()}
        res["deep_pile"]["reads_per_s_median"] = {n: statistics.median(r["reads_per_s_window"] for r in rs) for n, rs in res["deep_pile"]["runs"].items()}
        if a.genome_scale:
            try:
                res["genome_scale"] = genome_scale()
            except Exception as err:                           # (a device without 12.4 GB to spare: the rest of the figures stand)
                res["genome_scale"] = dict(error=str(err))
            print("genome", json.dumps(res["genome_scale"]), flush=True)
        os.makedirs(a.out, exist_ok=True)
        json.dump(res, open(os.path.join(a.out, "track_rates.json"), "w"), indent=1)
        print(json.dumps({k: v for k, v in res.items() if k != "runs"}))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
