#!/usr/bin/env python
"""Cohort mode against N one-sample runs: N synthetic BAMs (one annotation, different seeds) through `rnaseqc --bam-list` and, on
the same box and interleaved with it, through N runs of the one-sample command line.  Writes both per-sample wall clocks and their
ratio to profiles/cohort_rates.json and prints the same JSON line.
Usage: python tools/cohort_bench.py [--samples N] [--pairs P] [--reps R] [--genome] [--single-bin PATH] [--keep DIR]
--single-bin: the binary of the one-sample runs (default: this tree's; a parent commit's build compares against that)."""
import argparse, json, os, shutil, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rnaseqc_amd import bamio, synth

BIN = os.path.join(ROOT, "rnaseqc_amd", "bin", "rnaseqc")
ap = argparse.ArgumentParser()
ap.add_argument("--samples", type=int, default=8)
ap.add_argument("--pairs", type=int, default=1_000_000)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--genome", action="store_true", help="all human contigs (the 775 MB rank table) instead of chr1")
ap.add_argument("--single-bin", default=BIN)
ap.add_argument("--keep", default="")
ap.add_argument("--run-timeout", type=float, default=600.0, help="seconds one run of the binary may take")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cohort_rates.json"))
args = ap.parse_args()

contigs = synth.human_contigs() if args.genome else [synth.HUMAN_CONTIGS[0]]
ann = synth.make_annotation(seed=1, contigs=contigs)
d = args.keep or tempfile.mkdtemp(prefix="rsqc_cohort_")
os.makedirs(d, exist_ok=True)
gtf = os.path.join(d, "s.gtf")
bamio.write_gtf(gtf, ann)
bams, records = [], 0
for k in range(args.samples):
    batch = synth.make_reads(ann, args.pairs, seed=100 + k)
    bams.append(os.path.join(d, "s%02d.bam" % k))
    bamio.write_bam_fast(bams[-1], [(c[0], c[1]) for c in contigs], batch, threads=16)
    records += int(batch.n)
lst = os.path.join(d, "cohort.list")
open(lst, "w").write("".join(b + "\n" for b in bams))


def timed(cmd):
    t = time.time()
    try:
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=args.run_timeout)
    except subprocess.TimeoutExpired:
        sys.exit("%s did not end within %g s" % (" ".join(cmd), args.run_timeout))
    if p.returncode:
        sys.exit("%s failed (%d): %s" % (" ".join(cmd), p.returncode, p.stderr.decode()[-2000:]))
    return time.time() - t


cohort_s, singles_s = [], []
for rep in range(args.reps + 1):                       # (the first round warms the page cache and the driver: dropped)
    out_c, out_s = os.path.join(d, "out_cohort"), os.path.join(d, "out_single")
    shutil.rmtree(out_c, ignore_errors=True); shutil.rmtree(out_s, ignore_errors=True)
    c = timed([BIN, "--bam-list=" + lst, gtf, out_c])
    s = sum(timed([args.single_bin, gtf, b, out_s]) for b in bams)
    if rep:
        cohort_s.append(c); singles_s.append(s)
rows = [l.rstrip("\n").split("\t") for l in open(os.path.join(d, "out_cohort", "cohort.tsv"))][1:]
best_c, best_s = min(cohort_s), min(singles_s)
res = {"samples": args.samples, "records_per_sample": records // args.samples, "genes": int(ann.n_genes), "contigs": len(contigs),
       "reps": args.reps, "cohort_wall_s": [round(x, 3) for x in cohort_s], "one_sample_runs_wall_s": [round(x, 3) for x in singles_s],
       "cohort_per_sample_s": round(best_c / args.samples, 4), "one_sample_per_sample_s": round(best_s / args.samples, 4),
       "ratio_one_sample_over_cohort": round(best_s / best_c, 3),
       "cohort_tsv_seconds": [float(r[4]) for r in rows], "single_bin": os.path.relpath(args.single_bin, ROOT)}
os.makedirs(os.path.dirname(args.out), exist_ok=True)
open(args.out, "w").write(json.dumps(res, indent=1) + "\n")
print(json.dumps(res))
if not args.keep:
    shutil.rmtree(d, ignore_errors=True)
