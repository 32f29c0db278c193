"""What --mismatches costs: the records of tools/sam_bench.py (10.25 M) over a synthetic FASTA (bamio.synthetic_reference), written twice --
`reference`: write_bam_fast(seq_mode=2), SEQ copied from the reference under each record's CIGAR with a seeded 0.5 % of substitutions;
`random`: seq_mode=1, random bases, three quarters of which mismatch: the dense worst case of the rare path -- and the command line on each
in three configurations, interleaved and rotated (every round starts with another one), `--reps` rounds, by the reference's
`Average Reads/Sec` window:

    (a) parent      the binary of the commit before the feature (--parent-bin), with --fasta
    (b) fasta       this tree's binary with --fasta alone
    (c) mismatches  this tree's binary with --fasta --mismatches

(b) against (a): every report file must be equal -- that is the condition; the difference of the median rates is reported beside the
spread (max - min) of (a)'s own runs, not judged against a ratio.  (c) against (b) is the price of the feature, reported as measured: the
ratio of the medians, mismatch_ms (HIP events around the stage's kernels, summed over the windows), the bytes of SEQ + QUAL + reference
the stage reads and the TB/s that makes, beside the 6.3 TB/s of the project's bandwidth model.  Every report file of (c) but its own three
must equal (b)'s.

    python tools/mismatch_bench.py --parent-bin PATH/rnaseqc [--records 10250000] [--reps 5] [--out profiles] [--tmp DIR]

Without --parent-bin configuration (a) is left out.  Writes <out>/mismatch_rates.json."""
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
FIELDS = ("records", "no_reference", "low_mapq", "no_seq", "inconsistent", "compared", "mismatched", "uncompared", "inserted", "clipped", "deletions", "beyond", "mismatch_ms")
LINE = re.compile("Mismatches: " + ", ".join(f + r" ([0-9.e+-]+)" for f in FIELDS))
MODEL_TB_PER_S = 6.3
OWN_FILES = (".mismatch_cycles.tsv", ".mismatch_types.tsv", ".mismatch_quality.tsv")


def run_cli(binary, gtf, path, out, flags, timeout=1200):
    t0 = time.time()
    p = subprocess.run([binary] + flags + [gtf, path, out, "-s", "x", "-vv"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)
    wall = time.time() - t0
    so, se = p.stdout.decode(), p.stderr.decode()
    if p.returncode:
        raise RuntimeError("%s %s: exit %d\n%s" % (binary, path, p.returncode, se[-2000:]))
    m = re.search(r"Average Reads/Sec: ([0-9.e+]+)", so)
    r = dict(reads_per_s_window=float(m.group(1)) if m else None, wall_s=wall)
    c = LINE.search(so)
    if c:
        r["mismatches"] = {f: (float(c.group(k + 1)) if f == "mismatch_ms" else int(c.group(k + 1))) for k, f in enumerate(FIELDS)}
    return r


def other_reports_equal(a, b):
    fa = sorted(f for f in os.listdir(a) if not f.endswith(OWN_FILES))
    fb = sorted(f for f in os.listdir(b) if not f.endswith(OWN_FILES))
    return fa == fb and all(open(os.path.join(a, f), "rb").read() == open(os.path.join(b, f), "rb").read() for f in fa)


def write_reference(path, contigs, line_bases=60):
    """The synthetic reference as FASTA + .fai, a contig at a time."""
    with open(path, "wb") as f, open(path + ".fai", "w") as fai:
        for tid, (name, length) in enumerate(contigs):
            f.write(b">" + name.encode() + b"\n")
            off = f.tell()
            seq = bamio.synthetic_reference(tid, length)
            full = length // line_bases
            lines = np.full((full, line_bases + 1), 10, np.uint8)
            lines[:, :line_bases] = seq[:full * line_bases].reshape(full, line_bases)
            f.write(lines.tobytes())
            if length % line_bases:
                f.write(seq[full * line_bases:].tobytes() + b"\n")
            fai.write("%s\t%d\t%d\t%d\t%d\n" % (name, length, off, line_bases, line_bases + 1))


def measure(name, bam, gtf, fasta, tmp, parent_bin, reps):
    res = dict(bam_bytes=os.path.getsize(bam), runs={})
    ref = ["--fasta", fasta]
    configs = ([("parent", parent_bin, ref)] if parent_bin else []) + [("fasta", CLI, ref), ("mismatches", CLI, ref + ["--mismatches"])]
    outs = {n: os.path.join(tmp, "out_%s_%s" % (name, n)) for n, _, _ in configs}
    for rep in range(reps):                               # interleaved and rotated: drift of the box and the place in the round land on every configuration alike
        k = rep % len(configs)
        for cfg, binary, flags in configs[k:] + configs[:k]:
            shutil.rmtree(outs[cfg], ignore_errors=True)
            r = run_cli(binary, gtf, bam, outs[cfg], flags)
            res["runs"].setdefault(cfg, []).append(r)
            print(name, rep, cfg, json.dumps(r), flush=True)
    rates = {n: [r["reads_per_s_window"] for r in rs] for n, rs in res["runs"].items()}
    med = {n: statistics.median(v) for n, v in rates.items()}
    res["median_reads_per_s_window"] = med
    res["other_reports_equal_fasta"] = other_reports_equal(outs["fasta"], outs["mismatches"])
    if parent_bin:
        res["off"] = dict(reports_equal_parent=other_reports_equal(outs["parent"], outs["fasta"]), parent_median=med["parent"], fasta_median=med["fasta"],
                          difference=med["fasta"] - med["parent"], parent_spread=max(rates["parent"]) - min(rates["parent"]), parent_runs=rates["parent"], fasta_runs=rates["fasta"])
    mm = {f: statistics.median(r["mismatches"][f] for r in res["runs"]["mismatches"]) for f in FIELDS}
    # SEQ is (L + 1) / 2 bytes and QUAL L bytes of a record; the reference half a byte per compared or uncompared base
    length_sum = mm["compared"] + mm["uncompared"] + mm["inserted"] + mm["clipped"] + mm["beyond"]
    read_bytes = length_sum + (length_sum + mm["records"]) // 2 + (mm["compared"] + mm["uncompared"]) // 2
    res["on"] = dict(fasta_median=med["fasta"], mismatches_median=med["mismatches"], ratio=med["mismatches"] / med["fasta"], mismatch_ms=mm["mismatch_ms"],
                     mismatch_ms_runs=[r["mismatches"]["mismatch_ms"] for r in res["runs"]["mismatches"]], figures=mm, seq_qual_reference_bytes=read_bytes,
                     implied_tb_per_s=read_bytes / (mm["mismatch_ms"] * 1e-3) / 1e12 if mm["mismatch_ms"] else None,
                     model_tb_per_s=MODEL_TB_PER_S, model_ms=read_bytes / (MODEL_TB_PER_S * 1e12) * 1e3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-bin", default=None, help="the rnaseqc binary of the commit before the feature (its library beside it, as `make variant` lays them out)")
    ap.add_argument("--records", type=int, default=10_250_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--tmp", default=None)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--inputs", default="reference,random")
    ap.add_argument("--variant", default=None, help="a name for this build (a by-quality layout, a workgroup size): its figures go under variants/<name> of the file that is there")
    a = ap.parse_args()
    tmp = tempfile.mkdtemp(dir=a.tmp)
    try:
        # the records of tools/sam_bench.py
        contigs = [("chr%d" % k, 50_000_000, 600) for k in range(1, 5)]
        ann = synth.make_annotation(seed=61, contigs=contigs)
        t0 = time.time()
        batch = bamio.sam_consistent(synth.make_reads(ann, a.records // 2, seed=62, contig_lengths=np.array([c[1] for c in contigs])))
        cs = [(c[0], c[1]) for c in contigs]
        gtf, fasta = os.path.join(tmp, "x.gtf"), os.path.join(tmp, "x.fa")
        bamio.write_gtf(gtf, ann)
        write_reference(fasta, cs)
        res = dict(records=int(batch.n), reps=a.reps, inputs={})
        for name in a.inputs.split(","):
            bam = os.path.join(tmp, name + ".bam")
            bamio.write_bam_fast(bam, cs, batch, threads=a.threads, seq_mode=2 if name == "reference" else 1)
            res["inputs"][name] = measure(name, bam, gtf, fasta, tmp, a.parent_bin, a.reps)
            os.remove(bam)
        res["input_s"] = time.time() - t0
        os.makedirs(a.out, exist_ok=True)
        path = os.path.join(a.out, "mismatch_rates.json")
        if a.variant:
            whole = json.load(open(path)) if os.path.exists(path) else {}
            whole.setdefault("variants", {})[a.variant] = {n: dict(mismatch_ms=r["on"]["mismatch_ms"], mismatch_ms_runs=r["on"]["mismatch_ms_runs"], ratio=r["on"]["ratio"])
                                                           for n, r in res["inputs"].items()}
            res = whole
        json.dump(res, open(path, "w"), indent=1)
        print(json.dumps({n: {k: v for k, v in r.items() if k != "runs"} for n, r in res.get("inputs", {}).items()}))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
