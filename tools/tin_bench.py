"""What --tin costs, and what its stage says about --gene-body's: the input of tools/genebody_bench.py (the synthetic records of
tools/sam_bench.py, seq_mode 1, as one BAM of 10.25 M records over a synthetic annotation of 60 000 genes) and the command line on it
in four configurations, interleaved and rotated (every round starts with another one), `--reps` rounds, by the reference's
`Average Reads/Sec` window:

    (a) parent        the binary of the commit before the feature (--parent-bin), without the flag
    (b) plain         this tree's binary without the flag
    (c) gene_body     this tree's binary with --gene-body
    (d) tin           this tree's binary with --tin

(b) against (a) is the check that the feature costs nothing when it is off: it passes when the difference of the medians lies within
the spread (max - min) of (a)'s own runs; both figures are reported, and every report file of (a) and (b) must be equal.  (d) against
(b) is the price of the feature, reported as measured: the ratio of the medians, and tin_ms of (d) beside bins_ms of (c) -- both
stages walk the same model positions of the same array with the same cursor; --tin's has no LDS bins and no atomics.  The reports of
(b) and (d) are compared (every file but the two of --tin must be byte-identical).

    python tools/tin_bench.py --parent-bin PATH/rnaseqc [--records 10000000] [--reps 5] [--out profiles] [--tmp DIR]

Without --parent-bin configuration (a) is left out.  Writes <out>/tin_rates.json."""
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
BODY_LINE = re.compile(r"Gene body: genes (\d+), measured (\d+), eligible (\d+), model_bases (\d+), depth_sum (\d+), bins_ms %s" % NUM)
BODY_FIELDS = ("genes", "measured", "eligible", "model_bases", "depth_sum", "bins_ms")
TIN_LINE = re.compile(r"TIN: genes (\d+), measured (\d+), eligible (\d+), model_bases (\d+), covered_bases (\d+), depth_sum (\d+), median %s, tin_ms %s" % (NUM, NUM))
TIN_FIELDS = ("genes", "measured", "eligible", "model_bases", "covered_bases", "depth_sum", "median", "tin_ms")
MODEL_TB_PER_S = 6.3
OWN_FILES = (".gene_body.tsv", ".tin.tsv", ".tin_summary.tsv")


def run_cli(binary, gtf, path, out, flags, timeout=1200):
    t0 = time.time()
    p = subprocess.run([binary] + flags + [gtf, path, out, "-s", "x", "-vv"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)
    wall = time.time() - t0
    so, se = p.stdout.decode(), p.stderr.decode()
    if p.returncode:
        raise RuntimeError("%s %s: exit %d\n%s" % (binary, path, p.returncode, se[-2000:]))
    m = re.search(r"Average Reads/Sec: ([0-9.e+]+)", so)
    r = dict(reads_per_s_window=float(m.group(1)) if m else None, wall_s=wall)
    b, t = BODY_LINE.search(so), TIN_LINE.search(so)
    if b:
        r["gene_body"] = {f: (float(b.group(k + 1)) if f == "bins_ms" else int(b.group(k + 1))) for k, f in enumerate(BODY_FIELDS)}
    if t:
        r["tin"] = {f: (float(t.group(k + 1)) if f in ("median", "tin_ms") else int(t.group(k + 1))) for k, f in enumerate(TIN_FIELDS)}
    return r


def other_reports_equal(a, b):
    fa = sorted(f for f in os.listdir(a) if not f.endswith(OWN_FILES))
    fb = sorted(f for f in os.listdir(b) if not f.endswith(OWN_FILES))
    return fa == fb and all(open(os.path.join(a, f), "rb").read() == open(os.path.join(b, f), "rb").read() for f in fa)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-bin", default=None, help="the rnaseqc binary of the commit before the feature (its library beside it, as `make variant` lays them out)")
    ap.add_argument("--records", type=int, default=10_000_000)
    ap.add_argument("--genes-per-contig", type=int, default=15_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--tmp", default=None)
    ap.add_argument("--threads", type=int, default=16)
    a = ap.parse_args()
    tmp = tempfile.mkdtemp(dir=a.tmp)
    try:
        contigs = [("chr%d" % k, 50_000_000, a.genes_per_contig) for k in range(1, 5)]
        ann = synth.make_annotation(seed=61, contigs=contigs)
        t0 = time.time()
        batch = bamio.sam_consistent(synth.make_reads(ann, a.records // 2, seed=62, contig_lengths=np.array([c[1] for c in contigs])))
        cs = [(c[0], c[1]) for c in contigs]
        bam, gtf = os.path.join(tmp, "x.bam"), os.path.join(tmp, "x.gtf")
        bamio.write_gtf(gtf, ann)
        bamio.write_bam_fast(bam, cs, batch, threads=a.threads, seq_mode=1)
        res = dict(records=int(batch.n), positions=sum(c[1] for c in contigs), genes=int(ann.n_genes_listed), exon_rows=int(ann.n_exons), input_s=time.time() - t0,
                   bam_bytes=os.path.getsize(bam), reps=a.reps, runs={})
        configs = ([("parent", a.parent_bin, [])] if a.parent_bin else []) + [("plain", CLI, []), ("gene_body", CLI, ["--gene-body"]), ("tin", CLI, ["--tin"])]
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
        res["other_reports_equal_plain"] = dict(tin=other_reports_equal(os.path.join(tmp, "out_plain"), os.path.join(tmp, "out_tin")),
                                                gene_body=other_reports_equal(os.path.join(tmp, "out_plain"), os.path.join(tmp, "out_gene_body")))
        if a.parent_bin:
            spread = max(rates["parent"]) - min(rates["parent"])
            res["off_check"] = dict(parent_median=med["parent"], plain_median=med["plain"], difference=med["plain"] - med["parent"], parent_spread=spread,
                                    within_parent_spread=abs(med["plain"] - med["parent"]) <= spread)
            res["reports_equal_parent"] = other_reports_equal(os.path.join(tmp, "out_parent"), os.path.join(tmp, "out_plain"))
        body = {f: statistics.median(r["gene_body"][f] for r in res["runs"]["gene_body"]) for f in BODY_FIELDS}
        tin = {f: statistics.median(r["tin"][f] for r in res["runs"]["tin"]) for f in TIN_FIELDS}
        res["price"] = dict(plain_median=med["plain"], tin_median=med["tin"], ratio=med["tin"] / med["plain"], gene_body_median=med["gene_body"], gene_body_ratio=med["gene_body"] / med["plain"])
        res["gene_body_median"], res["tin_median"] = body, tin
        read_bytes = 4 * tin["model_bases"]
        res["stage"] = dict(tin_ms=tin["tin_ms"], tin_ms_runs=[r["tin"]["tin_ms"] for r in res["runs"]["tin"]], tin_model_bases=tin["model_bases"],
                            bins_ms=body["bins_ms"], bins_ms_runs=[r["gene_body"]["bins_ms"] for r in res["runs"]["gene_body"]], bins_model_bases=body["model_bases"],
                            tin_over_bins=tin["tin_ms"] / body["bins_ms"] if body["bins_ms"] else None,
                            bytes_read=read_bytes, implied_tb_per_s=read_bytes / (tin["tin_ms"] * 1e-3) / 1e12 if tin["tin_ms"] else None,
                            model_tb_per_s=MODEL_TB_PER_S, model_ms=read_bytes / (MODEL_TB_PER_S * 1e12) * 1e3)
        os.makedirs(a.out, exist_ok=True)
        json.dump(res, open(os.path.join(a.out, "tin_rates.json"), "w"), indent=1)
        print(json.dumps({k: v for k, v in res.items() if k != "runs"}))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
