"""What --sort costs: the synthetic records of tools/sam_bench.py (seq_mode 1) as a coordinate-sorted BAM and as a seeded shuffle of
the same records, the CLI on the sorted file without --sort, on the sorted file with --sort and on the shuffle with --sort --
interleaved, `--reps` rounds -- by the reference's `Average Reads/Sec` window, with the fields of rsqc_sort_info the -v line prints.
The comparison is against the plain run on the sorted file of the same invocation; the reports of the three runs are compared.

    python tools/sort_bench.py [--records 10000000] [--reps 3] [--out profiles] [--tmp DIR]

Writes <out>/sort_rates.json.  radix_gb_per_s = live passes x 2 x 12 B x records / sort_ms: the bytes the radix passes have to
move (key + index, read and written once per pass) over the time they took."""
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
SORT_LINE = re.compile(r"Sorted on the GPU: records (\d+), batches in (\d+), batches out (\d+), moved (\d+), key_ms ([0-9.e+-]+), sort_ms ([0-9.e+-]+), "
                       r"gather_ms ([0-9.e+-]+), was_sorted (\d)")


def run_cli(gtf, path, out, sort, timeout=1200):
    t0 = time.time()
    p = subprocess.run([CLI] + (["--sort"] if sort else []) + [gtf, path, out, "-s", "x", "-vv"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)
    wall = time.time() - t0
    so, se = p.stdout.decode(), p.stderr.decode()
    if p.returncode:
        raise RuntimeError("%s: exit %d\n%s" % (path, p.returncode, se[-2000:]))
    m = re.search(r"Average Reads/Sec: ([0-9.e+]+)", so)
    r = dict(reads_per_s_window=float(m.group(1)) if m else None, wall_s=wall, warned_unsorted="does not appear to be sorted" in se)
    s = SORT_LINE.search(so)
    if s:
        r["sort_info"] = dict(records=int(s.group(1)), batches_in=int(s.group(2)), batches_out=int(s.group(3)), moved=int(s.group(4)),
                              key_ms=float(s.group(5)), sort_ms=float(s.group(6)), gather_ms=float(s.group(7)), was_sorted=int(s.group(8)))
    return r


def same_reports(a, b):
    fa, fb = sorted(os.listdir(a)), sorted(os.listdir(b))
    return fa == fb and all(open(os.path.join(a, f), "rb").read() == open(os.path.join(b, f), "rb").read() for f in fa)


def live_passes(batch):
    """Digit positions in which the keys of the batch differ (rsqc_sort.h, sort_live_digits)."""
    tid = batch.tid_per_record().view(np.uint32).astype(np.uint64)
    key = (tid << np.uint64(32)) | (batch.pos.view(np.uint32) ^ np.uint32(0x80000000)).astype(np.uint64)
    differ = int(np.bitwise_or.reduce(key)) ^ int(np.bitwise_and.reduce(key))
    return sum(1 for d in range(8) if (differ >> (8 * d)) & 0xFF)


def main():
    ap = argparse.ArgumentParser()
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
        base = bamio.sam_consistent(synth.make_reads(ann, a.records // 2, seed=62, contig_lengths=np.array([c[1] for c in contigs])))
        shuffled = base.take(np.random.default_rng(63).permutation(base.n))
        ordered = shuffled.coordinate_sorted()                  # the stable sort of the shuffle: what --sort has to reproduce
        cs = [(c[0], c[1]) for c in contigs]
        files = dict(sorted=os.path.join(tmp, "sorted.bam"), shuffled=os.path.join(tmp, "shuffled.bam"))
        gtf = os.path.join(tmp, "x.gtf")
        bamio.write_gtf(gtf, ann)
        bamio.write_bam_fast(files["sorted"], cs, ordered, threads=a.threads, seq_mode=1)
        bamio.write_bam_fast(files["shuffled"], cs, shuffled, threads=a.threads, seq_mode=1)
        passes = live_passes(shuffled)
        res = dict(records=int(base.n), input_s=time.time() - t0, bytes={k: os.path.getsize(v) for k, v in files.items()}, live_passes=passes, reps=a.reps, runs={})
        configs = (("sorted_plain", "sorted", False), ("sorted_sort", "sorted", True), ("shuffled_sort", "shuffled", True))
        for rep in range(a.reps):                               # interleaved: drift of the box lands on every configuration alike
            for name, f, sort in configs:
                out = os.path.join(tmp, "out_" + name)
                shutil.rmtree(out, ignore_errors=True)
                r = run_cli(gtf, files[f], out, sort)
                res["runs"].setdefault(name, []).append(r)
                print(rep, name, json.dumps(r), flush=True)
        res["reports_equal_sorted_plain"] = {n: same_reports(os.path.join(tmp, "out_sorted_plain"), os.path.join(tmp, "out_" + n)) for n in ("sorted_sort", "shuffled_sort")}
        med = {n: statistics.median(r["reads_per_s_window"] for r in rs) for n, rs in res["runs"].items()}
        res["median_reads_per_s_window"] = med
        res["ratio_to_sorted_plain"] = {n: med[n] / med["sorted_plain"] for n in med}
        sort_ms = statistics.median(r["sort_info"]["sort_ms"] for r in res["runs"]["shuffled_sort"])
        res["shuffled_sort_median_ms"] = {k: statistics.median(r["sort_info"][k] for r in res["runs"]["shuffled_sort"]) for k in ("key_ms", "sort_ms", "gather_ms")}
        res["radix_bytes"] = passes * 2 * 12 * int(base.n)
        res["radix_gb_per_s"] = res["radix_bytes"] / (sort_ms / 1e3) / 1e9 if sort_ms else None
        os.makedirs(a.out, exist_ok=True)
        json.dump(res, open(os.path.join(a.out, "sort_rates.json"), "w"), indent=1)
        print(json.dumps({k: v for k, v in res.items() if k != "runs"}))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
