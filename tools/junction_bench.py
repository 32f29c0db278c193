"""What --junctions costs: the synthetic records of tools/sam_bench.py (seq_mode 1) as one BAM, and the command line on it in three
configurations, interleaved, `--reps` rounds, by the reference's `Average Reads/Sec` window:

    (a) parent        the binary of the commit before the feature (--parent-bin), without the flag
    (b) plain         this tree's binary without the flag
    (c) junctions     this tree's binary with --junctions

(b) against (a) is the check that the feature costs nothing when it is off: it passes when the difference of the medians lies
within the spread (max - min) of (a)'s own runs.  (c) against (b) is the price of the feature, reported as measured, with the
fields of the -v line (population, instances, rows, extract_ms, sort_ms, reduce_ms) and the bytes the two sort stages move -- live
passes x 2 x 12 B x instances -- over sort_ms, beside the project's 6.3 TB/s model figure.  The reports of (b) and (c) are compared
(every file but the junction table must be byte-identical).

    python tools/junction_bench.py --parent-bin PATH/rnaseqc [--records 10000000] [--reps 3] [--out profiles] [--tmp DIR]

Without --parent-bin configuration (a) is left out.  Writes <out>/junction_rates.json."""
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
MODEL_TB_PER_S = 6.3
JUNCTION_LINE = re.compile(r"Junctions: population (\d+), instances (\d+), rows (\d+), extract_ms ([0-9.e+-]+), sort_ms ([0-9.e+-]+), reduce_ms ([0-9.e+-]+)")


def run_cli(binary, gtf, path, out, junctions, timeout=1200):
    t0 = time.time()
    p = subprocess.run([binary] + (["--junctions"] if junctions else []) + [gtf, path, out, "-s", "x", "-vv"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)
    wall = time.time() - t0
    so, se = p.stdout.decode(), p.stderr.decode()
    if p.returncode:
        raise RuntimeError("%s %s: exit %d\n%s" % (binary, path, p.returncode, se[-2000:]))
    m = re.search(r"Average Reads/Sec: ([0-9.e+]+)", so)
    r = dict(reads_per_s_window=float(m.group(1)) if m else None, wall_s=wall)
    j = JUNCTION_LINE.search(so)
    if j:
        r["junctions"] = dict(population=int(j.group(1)), instances=int(j.group(2)), rows=int(j.group(3)), extract_ms=float(j.group(4)), sort_ms=float(j.group(5)),
                              reduce_ms=float(j.group(6)))
    return r


def live_passes(path):
    """Digit positions in which the two key parts differ over the rows of a junction table (the instances have the same OR and AND as
    the rows): stage 1 over `end`, stage 2 over (tid << 32) | start."""
    tid_of, ends, his = {}, [], []
    for line in open(path).read().splitlines()[1:]:
        f = line.split("\t")
        t = tid_of.setdefault(f[0], len(tid_of))
        ends.append(int(f[2])); his.append((t << 32) | int(f[1]))

    def live(keys):
        if not keys:
            return 0
        o = a = keys[0]
        for k in keys:
            o |= k; a &= k
        return sum(1 for d in range(8) if ((o ^ a) >> (8 * d)) & 0xFF)
    return live(ends), live(his)


def other_reports_equal(a, b):
    fa = sorted(f for f in os.listdir(a) if not f.endswith(".junctions.tsv"))
    fb = sorted(f for f in os.listdir(b) if not f.endswith(".junctions.tsv"))
    return fa == fb and all(open(os.path.join(a, f), "rb").read() == open(os.path.join(b, f), "rb").read() for f in fa)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-bin", default=None, help="the rnaseqc binary of the commit before the feature (its library beside it, as `make variant` lays them out)")
    ap.add_argument("--records", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--tmp", default=None)
    ap.add_argument("--threads", type=int, default=16)
    a = ap.parse_args()
    tmp = tempfile.mkdtemp(dir=a.tmp)
    try:
        contigs = [("chr%d" % k, 50_000_000, 600) for k in range(1, 5)]
        ann = synth.make_annotation(seed=61, contigs=contigs)
        t0 = time.time()
        batch = bamio.sam_consistent(synth.make_reads(ann, a.records // 2, seed=62, contig_lengths=np.array([c[1] for c in contigs])))
        cs = [(c[0], c[1]) for c in contigs]
        bam, gtf = os.path.join(tmp, "x.bam"), os.path.join(tmp, "x.gtf")
        bamio.write_gtf(gtf, ann)
        bamio.write_bam_fast(bam, cs, batch, threads=a.threads, seq_mode=1)
        res = dict(records=int(batch.n), cigar_operations=int(len(batch.cigar)), input_s=time.time() - t0, bam_bytes=os.path.getsize(bam), reps=a.reps, runs={})
        configs = ([("parent", a.parent_bin, False)] if a.parent_bin else []) + [("plain", CLI, False), ("junctions", CLI, True)]
        for rep in range(a.reps):                               # interleaved: drift of the box lands on every configuration alike
            for name, binary, junctions in configs:
                out = os.path.join(tmp, "out_" + name)
                shutil.rmtree(out, ignore_errors=True)
                r = run_cli(binary, gtf, bam, out, junctions)
                res["runs"].setdefault(name, []).append(r)
                print(rep, name, json.dumps(r), flush=True)
        rates = {n: [r["reads_per_s_window"] for r in rs] for n, rs in res["runs"].items()}
        med = {n: statistics.median(v) for n, v in rates.items()}
        res["median_reads_per_s_window"] = med
        res["other_reports_equal_plain"] = other_reports_equal(os.path.join(tmp, "out_plain"), os.path.join(tmp, "out_junctions"))
        if a.parent_bin:
            spread = max(rates["parent"]) - min(rates["parent"])
            res["off_check"] = dict(parent_median=med["parent"], plain_median=med["plain"], difference=med["plain"] - med["parent"], parent_spread=spread,
                                    within_parent_spread=abs(med["plain"] - med["parent"]) <= spread)
            res["reports_equal_parent"] = other_reports_equal(os.path.join(tmp, "out_parent"), os.path.join(tmp, "out_plain"))
        res["price"] = dict(plain_median=med["plain"], junctions_median=med["junctions"], ratio=med["junctions"] / med["plain"])
        js = [r["junctions"] for r in res["runs"]["junctions"]]
        res["junctions_median"] = {k: statistics.median(j[k] for j in js) for k in ("population", "instances", "rows", "extract_ms", "sort_ms", "reduce_ms")}
        p_end, p_hi = live_passes(os.path.join(tmp, "out_junctions", "x.junctions.tsv"))
        inst, sort_ms = res["junctions_median"]["instances"], res["junctions_median"]["sort_ms"]
        res["sort_stages"] = dict(live_passes_end=p_end, live_passes_tid_start=p_hi, bytes_moved=(p_end + p_hi) * 2 * 12 * int(inst),
                                  gb_per_s=((p_end + p_hi) * 2 * 12 * inst / (sort_ms / 1e3) / 1e9 if sort_ms else None), model_tb_per_s=MODEL_TB_PER_S,
                                  note="sort_ms is a host clock around both stages, their key reduction and its read-back")
        os.makedirs(a.out, exist_ok=True)
        json.dump(res, open(os.path.join(a.out, "junction_rates.json"), "w"), indent=1)
        print(json.dumps({k: v for k, v in res.items() if k != "runs"}))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
