"""What --alleles costs: the records of tools/sam_bench.py (10.25 M, random bases and binned qualities: write_bam_fast(seq_mode=1)) against
two seeded site panels over its four 50 M-base contigs --

    sparse   one site per 1 000 positions (200 000 sites)
    dense    one site per 10 positions (20 M sites)

-- and a `pile` input: as many records drawn over an annotation of 25 genes per contig instead of 600, about 10^5 records per gene, so
that the sites under those hundred genes are each seen by thousands to tens of thousands of records, against the dense panel.  The command line runs on each in three configurations, interleaved and rotated
(every round starts with another one), `--reps` rounds, by the reference's `Average Reads/Sec` window:

    (a) parent   the binary of the commit before the feature (--parent-bin)
    (b) plain    this tree's binary without the flag
    (c) alleles  this tree's binary with --alleles=<panel> and RSQC_ALLELE_MERGE=0: an atomic per observation
    (d) merge    the same with RSQC_ALLELE_MERGE=1: the lanes of a wave that meet on one cell are added up first

(b) against (a): every report file must be equal -- that is the condition; the difference of the median rates is reported beside the
spread (max - min) of (a)'s own runs.  (c) against (b) is the price of the feature, reported as measured: the ratio of the medians,
alleles_ms (HIP events around the stage's kernels, summed over the windows), the observations and the nanoseconds of kernel time per
record and per observation.  (d) is reported the same way beside it.  Every report file of (c) and (d) but their own must equal (b)'s, and
their own must be equal.

    python tools/allele_bench.py [--parent-bin PATH/rnaseqc] [--records 10250000] [--reps 5] [--out profiles] [--tmp DIR] [--variant NAME]

Without --parent-bin configuration (a) is left out.  Writes <out>/allele_rates.json (--variant NAME: that build's figures go under
variants/<NAME> of the file that is there)."""
import argparse
import gzip
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
FIELDS = ("sites", "skipped_lines", "off_header_lines", "duplicate_lines", "records", "hit_records", "observations", "off_contig", "low_mapq", "no_seq", "inconsistent", "no_qual",
          "alleles_ms")
LINE = re.compile("Alleles: " + ", ".join(f + r" ([0-9.e+-]+)" for f in FIELDS))
OWN_FILES = (".allele_counts.tsv",)


def run_cli(binary, gtf, path, out, flags, env=None, timeout=1200):
    t0 = time.time()
    p = subprocess.run([binary] + flags + [gtf, path, out, "-s", "x", "-vv"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout, env=dict(os.environ, **(env or {})))
    wall = time.time() - t0
    so, se = p.stdout.decode(), p.stderr.decode()
    if p.returncode:
        raise RuntimeError("%s %s: exit %d\n%s" % (binary, path, p.returncode, se[-2000:]))
    m = re.search(r"Average Reads/Sec: ([0-9.e+]+)", so)
    r = dict(reads_per_s_window=float(m.group(1)) if m else None, wall_s=wall)
    c = LINE.search(so)
    if c:
        r["alleles"] = {f: (float(c.group(k + 1)) if f == "alleles_ms" else int(c.group(k + 1))) for k, f in enumerate(FIELDS)}
    return r


def other_reports_equal(a, b):
    fa = sorted(f for f in os.listdir(a) if not f.endswith(OWN_FILES))
    fb = sorted(f for f in os.listdir(b) if not f.endswith(OWN_FILES))
    return fa == fb and all(open(os.path.join(a, f), "rb").read() == open(os.path.join(b, f), "rb").read() for f in fa)


def write_panel(path, contigs, every, seed):
    """A seeded panel as a gzip VCF: on every contig length / every distinct positions, REF and ALT two different seeded bases."""
    rng = np.random.default_rng(seed)
    n_sites = 0
    with gzip.open(path, "wb", compresslevel=1) as f:
        f.write(b"##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n")
        for name, length in contigs:
            pos = np.unique(rng.integers(1, length + 1, size=length // every))
            ref = rng.integers(0, 4, size=pos.size)
            alt = (ref + rng.integers(1, 4, size=pos.size)) % 4
            bases = np.array(list("ACGT"))
            rows = np.char.add(np.char.add(np.char.add(name + "\t", pos.astype(str)), "\t.\t"), np.char.add(np.char.add(bases[ref], "\t"), bases[alt]))
            f.write(("\n".join(rows.tolist()) + "\n").encode())
            n_sites += int(pos.size)
    return n_sites


def measure(name, bam, gtf, panel, tmp, parent_bin, reps):
    res = dict(bam_bytes=os.path.getsize(bam), panel_bytes=os.path.getsize(panel), runs={})
    configs = ([("parent", parent_bin, [], {})] if parent_bin else []) + [("plain", CLI, [], {}), ("alleles", CLI, ["--alleles=" + panel], dict(RSQC_ALLELE_MERGE="0")),
                                                                             ("merge", CLI, ["--alleles=" + panel], dict(RSQC_ALLELE_MERGE="1"))]
    outs = {n: os.path.join(tmp, "out_%s_%s" % (name, n)) for n, _, _, _ in configs}
    for rep in range(reps):                               # interleaved and rotated: drift of the box and the place in the round land on every configuration alike
        k = rep % len(configs)
        for cfg, binary, flags, env in configs[k:] + configs[:k]:
            shutil.rmtree(outs[cfg], ignore_errors=True)
            r = run_cli(binary, gtf, bam, outs[cfg], flags, env)
            res["runs"].setdefault(cfg, []).append(r)
            print(name, rep, cfg, json.dumps(r), flush=True)
    rates = {n: [r["reads_per_s_window"] for r in rs] for n, rs in res["runs"].items()}
    med = {n: statistics.median(v) for n, v in rates.items()}
    res["median_reads_per_s_window"] = med
    res["other_reports_equal_plain"] = other_reports_equal(outs["plain"], outs["alleles"]) and other_reports_equal(outs["plain"], outs["merge"])
    res["merge_file_equal"] = open(os.path.join(outs["alleles"], "x.allele_counts.tsv"), "rb").read() == open(os.path.join(outs["merge"], "x.allele_counts.tsv"), "rb").read()
    if parent_bin:
        res["off"] = dict(reports_equal_parent=other_reports_equal(outs["parent"], outs["plain"]), parent_median=med["parent"], plain_median=med["plain"],
                          difference=med["plain"] - med["parent"], parent_spread=max(rates["parent"]) - min(rates["parent"]), parent_runs=rates["parent"], plain_runs=rates["plain"])
    al = {f: statistics.median(r["alleles"][f] for r in res["runs"]["alleles"]) for f in FIELDS}
    res["on"] = dict(plain_median=med["plain"], alleles_median=med["alleles"], ratio=med["alleles"] / med["plain"], alleles_ms=al["alleles_ms"],
                     alleles_ms_runs=[r["alleles"]["alleles_ms"] for r in res["runs"]["alleles"]], wall_s_runs=[r["wall_s"] for r in res["runs"]["alleles"]],
                     plain_wall_s_runs=[r["wall_s"] for r in res["runs"]["plain"]], figures=al,
                     ns_per_record=al["alleles_ms"] * 1e6 / al["records"] if al["records"] else None,
                     ns_per_observation=al["alleles_ms"] * 1e6 / al["observations"] if al["observations"] else None)
    mg = {f: statistics.median(r["alleles"][f] for r in res["runs"]["merge"]) for f in FIELDS}
    res["merge"] = dict(merge_median=med["merge"], ratio=med["merge"] / med["plain"], alleles_ms=mg["alleles_ms"], alleles_ms_runs=[r["alleles"]["alleles_ms"] for r in res["runs"]["merge"]],
                        ns_per_record=mg["alleles_ms"] * 1e6 / mg["records"] if mg["records"] else None,
                        ns_per_observation=mg["alleles_ms"] * 1e6 / mg["observations"] if mg["observations"] else None)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-bin", default=None, help="the rnaseqc binary of the commit before the feature (its library beside it, as `make variant` lays them out)")
    ap.add_argument("--records", type=int, default=10_250_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--tmp", default=None)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--inputs", default="sparse,dense,pile")
    ap.add_argument("--variant", default=None, help="a name for this build (RSQC_ALLELE_MERGE, a workgroup size): its figures go under variants/<name> of the file that is there")
    a = ap.parse_args()
    tmp = tempfile.mkdtemp(dir=a.tmp)
    try:
        t0 = time.time()
        lengths = [50_000_000] * 4
        cs = [("chr%d" % k, n) for k, n in enumerate(lengths, 1)]
        panels = {}
        for every, name in ((1000, "sparse"), (10, "dense")):
            if name in a.inputs.split(",") or (name == "dense" and "pile" in a.inputs.split(",")):
                panels[name] = os.path.join(tmp, name + ".vcf.gz")
                print(name, "panel:", write_panel(panels[name], cs, every, 71 + every), "sites", flush=True)
        res = dict(records=0, reps=a.reps, inputs={})
        kept = os.path.join(a.out, "allele_rates.json")
        if not a.variant and os.path.exists(kept):                        # (--inputs with a part of them: the others' figures stay)
            res["inputs"] = json.load(open(kept)).get("inputs", {})
        batches = {}
        for name in a.inputs.split(","):
            genes = 25 if name == "pile" else 600                         # the records of tools/sam_bench.py; the pile: a hundred genes share them
            if genes not in batches:
                ann = synth.make_annotation(seed=61, contigs=[(c[0], c[1], genes) for c in cs])
                batch = bamio.sam_consistent(synth.make_reads(ann, a.records // 2, seed=62, contig_lengths=np.array(lengths)))
                gtf, bam = os.path.join(tmp, "g%d.gtf" % genes), os.path.join(tmp, "g%d.bam" % genes)
                bamio.write_gtf(gtf, ann)
                bamio.write_bam_fast(bam, cs, batch, threads=a.threads, seq_mode=1)
                batches[genes] = (gtf, bam, int(batch.n))
            gtf, bam, n = batches[genes]
            res["records"] = n
            res["inputs"][name] = measure(name, bam, gtf, panels["dense" if name == "pile" else name], tmp, a.parent_bin, a.reps)
            if not a.variant:                                             # (kept after every input: a run that is cut short leaves what it measured)
                os.makedirs(a.out, exist_ok=True)
                json.dump(res, open(os.path.join(a.out, "allele_rates.json"), "w"), indent=1)
        res["input_s"] = time.time() - t0
        os.makedirs(a.out, exist_ok=True)
        path = os.path.join(a.out, "allele_rates.json")
        if a.variant:
            whole = json.load(open(path)) if os.path.exists(path) else {}
            whole.setdefault("variants", {})[a.variant] = {n: dict(alleles_ms=r["on"]["alleles_ms"], alleles_ms_runs=r["on"]["alleles_ms_runs"], ratio=r["on"]["ratio"],
                                                                   ns_per_observation=r["on"]["ns_per_observation"]) for n, r in res["inputs"].items()}
            res = whole
        json.dump(res, open(path, "w"), indent=1)
        print(json.dumps({n: {k: v for k, v in r.items() if k != "runs"} for n, r in res.get("inputs", {}).items()}))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
