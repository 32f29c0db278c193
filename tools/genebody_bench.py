"""What --gene-body costs: the synthetic records of tools/sam_bench.py (seq_mode 1) as one BAM over a GENCODE-sized synthetic
annotation (60 000 genes, some 10^8 model bases), and the command line on it in three configurations, interleaved, `--reps` rounds, by
the reference's `Average Reads/Sec` window:

    (a) parent        the binary of the commit before the feature (--parent-bin), without the flag
    (b) plain         this tree's binary without the flag
    (c) gene_body     this tree's binary with --gene-body

(b) against (a) is the check that the feature costs nothing when it is off: it passes when the difference of the medians lies within
the spread (max - min) of (a)'s own runs; both figures are reported.  (c) against (b) is the price of the feature, reported as
measured: the ratio of the medians, and from the -v line bins_ms, the model bases and the bandwidth they imply (4 bytes a model base
over bins_ms) beside the 6.3 TB/s of the project's model.  The reports of (b) and (c) are compared (every file but the profile must
be byte-identical).

    python tools/genebody_bench.py --parent-bin PATH/rnaseqc [--records 10000000] [--reps 3] [--out profiles] [--tmp DIR]

Without --parent-bin configuration (a) is left out.  Writes <out>/genebody_rates.json."""
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
MODEL_TB_PER_S = 6.3
FIELDS = ("genes", "measured", "eligible", "model_bases", "depth_sum", "bins_ms")


def run_cli(binary, gtf, path, out, flag, timeout=1200):
    t0 = time.time()
    p = subprocess.run([binary] + (["--gene-body"] if flag else []) + [gtf, path, out, "-s", "x", "-vv"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)
    wall = time.time() - t0
    so, se = p.stdout.decode(), p.stderr.decode()
    if p.returncode:
        raise RuntimeError("%s %s: exit %d\n%s" % (binary, path, p.returncode, se[-2000:]))
    m = re.search(r"Average Reads/Sec: ([0-9.e+]+)", so)
    r = dict(reads_per_s_window=float(m.group(1)) if m else None, wall_s=wall)
    b = BODY_LINE.search(so)
    if b:
        r["gene_body"] = {f: (float(b.group(k + 1)) if f == "bins_ms" else int(b.group(k + 1))) for k, f in enumerate(FIELDS)}
    return r


def other_reports_equal(a, b):
    fa = sorted(f for f in os.listdir(a) if not f.endswith(".gene_body.tsv"))
    fb = sorted(f for f in os.listdir(b) if not f.endswith(".gene_body.tsv"))
    return fa == fb and all(open(os.path.join(a, f), "rb").read() == open(os.path.join(b, f), "rb").read() for f in fa)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-bin", default=None, help="the rnaseqc binary of the commit before the feature (its library beside it, as `make variant` lays them out)")
    ap.add_argument("--records", type=int, default=10_000_000)
    ap.add_argument("--genes-per-contig", type=int, default=15_000)
    ap.add_argument("--reps", type=int, default=3)
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
        configs = ([("parent", a.parent_bin, False)] if a.parent_bin else []) + [("plain", CLI, False), ("gene_body", CLI, True)]
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
        res["other_reports_equal_plain"] = other_reports_equal(os.path.join(tmp, "out_plain"), os.path.join(tmp, "out_gene_body"))
        if a.parent_bin:
            spread = max(rates["parent"]) - min(rates["parent"])
            res["off_check"] = dict(parent_median=med["parent"], plain_median=med["plain"], difference=med["plain"] - med["parent"], parent_spread=spread,
                                    within_parent_spread=abs(med["plain"] - med["parent"]) <= spread)
            res["reports_equal_parent"] = other_reports_equal(os.path.join(tmp, "out_parent"), os.path.join(tmp, "out_plain"))
        on = res["runs"]["gene_body"]
        body = {f: statistics.median(r["gene_body"][f] for r in on) for f in FIELDS}
        read_bytes = 4 * body["model_bases"]
        res["price"] = dict(plain_median=med["plain"], gene_body_median=med["gene_body"], ratio=med["gene_body"] / med["plain"])
        res["gene_body_median"] = body
        res["stage"] = dict(bins_ms=body["bins_ms"], model_bases=body["model_bases"], bytes_read=read_bytes, implied_tb_per_s=read_bytes / (body["bins_ms"] * 1e-3) / 1e12 if body["bins_ms"] else None,
                            model_tb_per_s=MODEL_TB_PER_S, model_ms=read_bytes / (MODEL_TB_PER_S * 1e12) * 1e3)
        os.makedirs(a.out, exist_ok=True)
        json.dump(res, open(os.path.join(a.out, "genebody_rates.json"), "w"), indent=1)
        print(json.dumps({k: v for k, v in res.items() if k != "runs"}))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
