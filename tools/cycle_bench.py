"""What --cycles costs: the input of tools/sam_bench.py (its synthetic records written with write_bam_fast(seq_mode=1): random bases and
binned qualities, 10.25 M records) and the command line on it in three configurations, interleaved and rotated (every round starts
with another one), `--reps` rounds, by the reference's `Average Reads/Sec` window:

    (a) parent   the binary of the commit before the feature (--parent-bin), without the flag
    (b) plain    this tree's binary without the flag
    (c) cycles   this tree's binary with --cycles

(b) against (a): every report file must be equal -- that is the condition; the difference of the median rates is reported beside the
spread (max - min) of (a)'s own runs.  (c) against (b) is the price of the feature, reported as measured: the ratio of the medians,
cycles_ms (HIP events around the stage's kernels, summed over the windows), the SEQ + QUAL bytes the stage reads and the TB/s that
makes, beside the 6.3 TB/s of the project's bandwidth model.  Every report file of (c) but its own two must equal (b)'s.

    python tools/cycle_bench.py --parent-bin PATH/rnaseqc [--records 10000000] [--reps 5] [--out profiles] [--tmp DIR]

Without --parent-bin configuration (a) is left out.  Writes <out>/cycle_rates.json."""
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
CYCLES_LINE = re.compile(r"Cycles: records (\d+), no_seq (\d+), no_qual (\d+), bases (\d+), beyond (\d+), clamped (\d+), cycles_ms ([0-9.e+-]+)")
FIELDS = ("records", "no_seq", "no_qual", "bases", "beyond", "clamped", "cycles_ms")
MODEL_TB_PER_S = 6.3
OWN_FILES = (".cycle_bases.tsv", ".cycle_quality.tsv")


def run_cli(binary, gtf, path, out, flags, timeout=1200):
    t0 = time.time()
    p = subprocess.run([binary] + flags + [gtf, path, out, "-s", "x", "-vv"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)
    wall = time.time() - t0
    so, se = p.stdout.decode(), p.stderr.decode()
    if p.returncode:
        raise RuntimeError("%s %s: exit %d\n%s" % (binary, path, p.returncode, se[-2000:]))
    m = re.search(r"Average Reads/Sec: ([0-9.e+]+)", so)
    r = dict(reads_per_s_window=float(m.group(1)) if m else None, wall_s=wall)
    c = CYCLES_LINE.search(so)
    if c:
        r["cycles"] = {f: (float(c.group(k + 1)) if f == "cycles_ms" else int(c.group(k + 1))) for k, f in enumerate(FIELDS)}
    return r


def other_reports_equal(a, b):
    fa = sorted(f for f in os.listdir(a) if not f.endswith(OWN_FILES))
    fb = sorted(f for f in os.listdir(b) if not f.endswith(OWN_FILES))
    return fa == fb and all(open(os.path.join(a, f), "rb").read() == open(os.path.join(b, f), "rb").read() for f in fa)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-bin", default=None, help="the rnaseqc binary of the commit before the feature (its library beside it, as `make variant` lays them out)")
    ap.add_argument("--records", type=int, default=10_250_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--tmp", default=None)
    ap.add_argument("--threads", type=int, default=16)
    a = ap.parse_args()
    tmp = tempfile.mkdtemp(dir=a.tmp)
    try:
        # the records of tools/sam_bench.py
        contigs = [("chr%d" % k, 50_000_000, 600) for k in range(1, 5)]
        ann = synth.make_annotation(seed=61, contigs=contigs)
        t0 = time.time()
        batch = bamio.sam_consistent(synth.make_reads(ann, a.records // 2, seed=62, contig_lengths=np.array([c[1] for c in contigs])))
        cs = [(c[0], c[1]) for c in contigs]
        bam, gtf = os.path.join(tmp, "x.bam"), os.path.join(tmp, "x.gtf")
        bamio.write_gtf(gtf, ann)
        bamio.write_bam_fast(bam, cs, batch, threads=a.threads, seq_mode=1)
        res = dict(records=int(batch.n), input_s=time.time() - t0, bam_bytes=os.path.getsize(bam), reps=a.reps, runs={})
        configs = ([("parent", a.parent_bin, [])] if a.parent_bin else []) + [("plain", CLI, []), ("cycles", CLI, ["--cycles"])]
        for rep in range(a.reps):                               # interleaved and rotated: drift of the box and the place in the round land on every configuration alike
            k = rep % len(configs)
            for name, binary, flags in configs[k:] + configs[:k]:
                out = os.path.join(tmp, "out_" + name)
                shutil.rmtree(out, ignore_errors=True)
                r = run_cli(binary, gtf, bam, out, flags)
                res["runs"].setdefault(name, []).append(r)
                print(rep, name, json.dumps(r), flush=True)
        rates = {n: [r["reads_per_s_window"] for r in rs] for n, rs in res["runs"].items()}
        med = {n: statistics.median(v) for n, v in rates.items()}
        res["median_reads_per_s_window"] = med
        res["other_reports_equal_plain"] = other_reports_equal(os.path.join(tmp, "out_plain"), os.path.join(tmp, "out_cycles"))
        if a.parent_bin:
            spread = max(rates["parent"]) - min(rates["parent"])
            res["off"] = dict(reports_equal_parent=other_reports_equal(os.path.join(tmp, "out_parent"), os.path.join(tmp, "out_plain")), parent_median=med["parent"],
                              plain_median=med["plain"], difference=med["plain"] - med["parent"], parent_spread=spread)
        cyc = {f: statistics.median(r["cycles"][f] for r in res["runs"]["cycles"]) for f in FIELDS}
        # SEQ is (L + 1) / 2 bytes and QUAL L bytes of a record: with the sum of L and the records, the bytes to within half a byte per record
        length_sum = cyc["bases"] + cyc["beyond"]
        read_bytes = length_sum + (length_sum + cyc["records"]) // 2
        res["on"] = dict(plain_median=med["plain"], cycles_median=med["cycles"], ratio=med["cycles"] / med["plain"], cycles_ms=cyc["cycles_ms"],
                         cycles_ms_runs=[r["cycles"]["cycles_ms"] for r in res["runs"]["cycles"]], figures=cyc, seq_qual_bytes=read_bytes,
                         implied_tb_per_s=read_bytes / (cyc["cycles_ms"] * 1e-3) / 1e12 if cyc["cycles_ms"] else None,
                         model_tb_per_s=MODEL_TB_PER_S, model_ms=read_bytes / (MODEL_TB_PER_S * 1e12) * 1e3)
        os.makedirs(a.out, exist_ok=True)
        json.dump(res, open(os.path.join(a.out, "cycle_rates.json"), "w"), indent=1)
        print(json.dumps({k: v for k, v in res.items() if k != "runs"}))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
