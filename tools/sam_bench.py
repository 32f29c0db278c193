"""SAM input rates of the command line: the same synthetic records as BAM, plain SAM and BGZF SAM (seq_mode 1: the entropy of a
real file), the CLI on each (reads/s by the reference's `Average Reads/Sec` window and by wall clock; every report file
compared with the BAM run's), then the SAM run once more under `rocprofv3 --kernel-trace --stats` for the kernel table.

    python tools/sam_bench.py [--records 20000000] [--out profiles] [--tmp DIR] [--no-rocprof]

Writes <out>/sam_rates.json and <out>/sam_kernel_table.csv (the kernel table of the plain-SAM run)."""
import argparse
import csv
import glob
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from rnaseqc_amd import bamio, synth  # noqa: E402

CLI = os.path.join(ROOT, "rnaseqc_amd", "bin", "rnaseqc")
SAM_KERNELS = ("sam_", "rsqc::sam_")


def run_cli(gtf, path, out, env=None, timeout=1200):
    e = dict(os.environ, **(env or {}))
    t0 = time.time()
    p = subprocess.run([CLI, gtf, path, out, "-s", "x", "-vv"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e, timeout=timeout)
    wall = time.time() - t0
    so, se = p.stdout.decode(), p.stderr.decode()
    if p.returncode:
        raise RuntimeError("%s: exit %d\n%s" % (path, p.returncode, se[-2000:]))
    m = re.search(r"Average Reads/Sec: ([0-9.e+]+)", so)
    n = re.search(r"Alignments processed: (\d+)\s*$", so.split("Time Elapsed")[1]) if "Time Elapsed" in so else None
    return dict(reads_per_s_window=float(m.group(1)) if m else None, wall_s=wall,
                records=int(n.group(1)) if n else None, decode_profile=[l for l in se.splitlines() if l.startswith("[decode]")])


def same_reports(a, b):
    fa, fb = sorted(os.listdir(a)), sorted(os.listdir(b))
    return fa == fb and all(open(os.path.join(a, f), "rb").read() == open(os.path.join(b, f), "rb").read() for f in fa)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=20_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--tmp", default=None)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--no-rocprof", action="store_true")
    a = ap.parse_args()
    tmp = tempfile.mkdtemp(dir=a.tmp)
    try:
        contigs = [("chr%d" % k, 50_000_000, 600) for k in range(1, 5)]
        ann = synth.make_annotation(seed=61, contigs=contigs)
        t0 = time.time()
        batch = bamio.sam_consistent(synth.make_reads(ann, a.records // 2, seed=62, contig_lengths=np.array([c[1] for c in contigs])))
        cs = [(c[0], c[1]) for c in contigs]
        files = dict(bam=os.path.join(tmp, "x.bam"), sam=os.path.join(tmp, "x.sam"), samgz=os.path.join(tmp, "x.sam.gz"))
        gtf = os.path.join(tmp, "x.gtf")
        bamio.write_gtf(gtf, ann)
        st = batch.to_struct()
        bamio.write_bam_fast(files["bam"], cs, batch, threads=a.threads, seq_mode=1, struct=st)
        bamio.write_sam_fast(files["sam"], cs, batch, threads=a.threads, seq_mode=1, struct=st)
        bamio.write_sam_fast(files["samgz"], cs, batch, threads=a.threads, seq_mode=1, bgzf=True, struct=st)
        res = dict(records=int(batch.n), input_s=time.time() - t0, bytes={k: os.path.getsize(v) for k, v in files.items()}, runs={})
        for k, path in files.items():
            out = os.path.join(tmp, "out_" + k)
            res["runs"][k] = run_cli(gtf, path, out, env=dict(RSQC_DECODE_PROFILE="1"))
            if k != "bam":
                res["runs"][k]["reports_equal_bam"] = same_reports(os.path.join(tmp, "out_bam"), out)
            print(k, json.dumps(res["runs"][k]), flush=True)
        os.makedirs(a.out, exist_ok=True)
        if not a.no_rocprof:
            d = os.path.join(tmp, "prof")
            subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "k", "--",
                            CLI, gtf, files["sam"], os.path.join(tmp, "out_prof"), "-s", "x"], check=True, timeout=1200,
                           stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            stats = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
            if stats:
                shutil.copy(stats[0], os.path.join(a.out, "sam_kernel_table.csv"))
                rows = list(csv.DictReader(open(stats[0])))
                sam_ns = sum(float(r["TotalDurationNs"]) for r in rows if r["Name"].startswith(SAM_KERNELS))
                res["sam_stage_kernel_ms"] = sam_ns / 1e6
                res["sam_stage_records_per_s"] = batch.n / (sam_ns / 1e9) if sam_ns else None
                res["sam_stage_split_ms"] = {r["Name"].split("(")[0]: float(r["TotalDurationNs"]) / 1e6 for r in rows if r["Name"].startswith(SAM_KERNELS)}
        json.dump(res, open(os.path.join(a.out, "sam_rates.json"), "w"), indent=1)
        print(json.dumps({k: v for k, v in res.items() if k != "runs"}))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
