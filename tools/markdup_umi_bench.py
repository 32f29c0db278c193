"""What --umi-tag costs: the input of tools/markdup_bench.py -- the synthetic records of tools/sort_bench.py (seq_mode 1), a seeded
share of their fragments duplicated under new names, shuffled, one unsorted BAM -- with a 10-base RX:Z tag on every record: one UMI
per fragment, a copied fragment keeps its original's UMI with probability one half.  Three configurations, interleaved and rotated,
`--reps` rounds, by the reference's `Average Reads/Sec` window: the parent commit's binary with --mark-duplicates (--parent-cli), this
binary with --mark-duplicates, this binary with --umi-tag=RX.  Two questions: do the new flags cost anything while they are off (this
--mark-duplicates against the parent's, inside the spread of the parent's own runs, every report file equal), and what do they cost
while they are on (the ratio to --mark-duplicates, the stage's three clocks, the live radix passes of the four sort stages and the
bytes they moved).

    python tools/markdup_umi_bench.py [--records 10000000] [--dup-share 0.15] [--reps 9] [--parent-cli PATH] [--out profiles] [--tmp DIR]

Writes <out>/markdup_umi_rates.json.  Without --parent-cli the first question is left open (parent: false)."""
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

from rnaseqc_amd import abi, bamio, synth  # noqa: E402
from rnaseqc_amd.model import Batch  # noqa: E402

CLI = os.path.join(ROOT, "rnaseqc_amd", "bin", "rnaseqc")
NUM = r"([0-9.e+-]+)"
MARK_LINE = re.compile(r"Duplicates marked: records (\d+), population (\d+), anchors (\d+), sets (\d+), duplicate_fragments (\d+), flagged_records (\d+), cleared_records (\d+), "
                       r"sig_ms " + NUM + ", sort_ms " + NUM + ", mark_ms " + NUM)
UMI_LINE = re.compile(r"UMIs in the signature: anchors_with_umi (\d+), anchors_without_umi (\d+), position_duplicate_fragments (\d+)")
SORT_LINE = re.compile(r"Sorted on the GPU: records (\d+), .* key_ms " + NUM + ", sort_ms " + NUM + ", gather_ms " + NUM)
PROFILE_LINE = re.compile(r"markdup: anchors (\d+), passes_lo (\d+), passes_hi (\d+), radix_bytes (\d+), table_slots (\d+), device_bytes (\d+)(?:, passes_mapq (\d+), passes_umi (\d+), umi_column_bytes (\d+))?")
UMI_BASES = 10


def run_cli(cli, flag, gtf, path, out, timeout=1200):
    t0 = time.time()
    p = subprocess.run([cli, flag, gtf, path, out, "-s", "x", "-vv"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout,
                       env=dict(os.environ, RSQC_MARKDUP_PROFILE="1"))
    wall = time.time() - t0
    so, se = p.stdout.decode(), p.stderr.decode()
    if p.returncode:
        raise RuntimeError("%s %s: exit %d\n%s" % (cli, flag, p.returncode, se[-2000:]))
    m = re.search(r"Average Reads/Sec: ([0-9.e+]+)", so)
    r = dict(reads_per_s_window=float(m.group(1)) if m else None, wall_s=wall)
    s = SORT_LINE.search(so)
    if s:
        r["sort_info"] = dict(records=int(s.group(1)), key_ms=float(s.group(2)), sort_ms=float(s.group(3)), gather_ms=float(s.group(4)))
    d = MARK_LINE.search(so)
    if d:
        keys = ("records", "population", "anchors", "sets", "duplicate_fragments", "flagged_records", "cleared_records")
        r["markdup_info"] = dict({k: int(d.group(i + 1)) for i, k in enumerate(keys)}, sig_ms=float(d.group(8)), sort_ms=float(d.group(9)), mark_ms=float(d.group(10)))
    u = UMI_LINE.search(so)
    if u:
        r["umi_info"] = dict(anchors_with_umi=int(u.group(1)), anchors_without_umi=int(u.group(2)), position_duplicate_fragments=int(u.group(3)))
    q = PROFILE_LINE.search(se)
    if q:
        r["markdup_profile"] = dict(anchors=int(q.group(1)), passes_lo=int(q.group(2)), passes_hi=int(q.group(3)), radix_bytes=int(q.group(4)), table_slots=int(q.group(5)), device_bytes=int(q.group(6)))
        if q.group(7) is not None:
            r["markdup_profile"].update(passes_mapq=int(q.group(7)), passes_umi=int(q.group(8)), umi_column_bytes=int(q.group(9)))
    return r


def same_reports(a, b):
    fa, fb = sorted(os.listdir(a)), sorted(os.listdir(b))
    return fa == fb and all(open(os.path.join(a, f), "rb").read() == open(os.path.join(b, f), "rb").read() for f in fa)


def with_duplicates(base, share, seed):
    """The batch plus copies of a seeded share of its fragments (all records of a name) under new names, nobody flagged.  Half of
    the copied fragments keep their original's UMI, the other half get a fresh one (one per copied fragment)."""
    r = np.random.default_rng(seed)
    names = np.unique(base.qhash)
    chosen = names[r.random(len(names)) < share]
    dup = base.take(np.flatnonzero(np.isin(base.qhash, chosen)))
    fresh_of = (np.uint64(1 << (2 * UMI_BASES)) | r.integers(0, 1 << (2 * UMI_BASES), len(chosen), dtype=np.uint64)).astype(np.uint64)
    keeps = r.random(len(chosen)) < 0.5
    k = np.searchsorted(chosen, dup.qhash)
    dup.umi = np.where(keeps[k], dup.umi, fresh_of[k]).astype(np.uint64)
    dup.qhash = dup.qhash ^ np.uint64(0x5DEECE66D1234567)
    both = Batch.concat([base, dup])
    both.flag = (both.flag & np.uint16(~abi.FDUP & 0xFFFF)).astype(np.uint16)
    return both, int(len(chosen)), int(keeps.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=10_000_000)
    ap.add_argument("--dup-share", type=float, default=0.15)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--parent-cli", default=None, help="the rnaseqc binary of the parent commit (built beside its own library)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--tmp", default=None)
    ap.add_argument("--threads", type=int, default=16)
    a = ap.parse_args()
    tmp = tempfile.mkdtemp(dir=a.tmp)
    try:
        contigs = [("chr%d" % k, 50_000_000, 600) for k in range(1, 5)]
        ann = synth.make_annotation(seed=61, contigs=contigs)
        t0 = time.time()
        base = bamio.sam_consistent(synth.make_reads(ann, a.records // 2, seed=62, contig_lengths=np.array([c[1] for c in contigs]), umi_bases=UMI_BASES))
        both, n_copied, n_kept = with_duplicates(base, a.dup_share, 64)
        shuffled = both.take(np.random.default_rng(63).permutation(both.n))
        cs = [(c[0], c[1]) for c in contigs]
        bam, gtf = os.path.join(tmp, "shuffled_rx.bam"), os.path.join(tmp, "x.gtf")
        bamio.write_gtf(gtf, ann)
        bamio.write_bam_fast(bam, cs, shuffled, threads=a.threads, seq_mode=1)         # (the umi column becomes RX:Z on every record)
        res = dict(base_records=int(base.n), records=int(shuffled.n), fragments_copied=n_copied, copies_with_the_originals_umi=n_kept, umi_bases=UMI_BASES, dup_share=a.dup_share,
                   input_s=time.time() - t0, bytes=os.path.getsize(bam), reps=a.reps, parent=a.parent_cli is not None, runs={})
        configs = [("this_markdup", CLI, "--mark-duplicates"), ("this_umi", CLI, "--umi-tag=RX")]
        if a.parent_cli:
            configs.insert(0, ("parent_markdup", a.parent_cli, "--mark-duplicates"))
        for rep in range(a.reps):                               # interleaved and rotated: drift of the box, and what a run leaves behind for the next, land on every configuration alike
            for name, cli, flag in configs[rep % len(configs):] + configs[:rep % len(configs)]:
                out = os.path.join(tmp, "out_" + name)
                shutil.rmtree(out, ignore_errors=True)
                r = run_cli(cli, flag, gtf, bam, out)
                res["runs"].setdefault(name, []).append(r)
                print(rep, name, json.dumps(r), flush=True)
        med = {n: statistics.median(r["reads_per_s_window"] for r in rs) for n, rs in res["runs"].items()}
        res["median_reads_per_s_window"] = med
        res["on_ratio_to_this_markdup"] = med["this_umi"] / med["this_markdup"]
        if a.parent_cli:
            rates = [r["reads_per_s_window"] for r in res["runs"]["parent_markdup"]]
            res["off"] = dict(parent_min=min(rates), parent_max=max(rates), parent_median=med["parent_markdup"], this_median=med["this_markdup"],
                              ratio=med["this_markdup"] / med["parent_markdup"],
                              inside_parent_spread=min(rates) <= med["this_markdup"] <= max(rates) or med["this_markdup"] >= med["parent_markdup"],
                              reports_equal=same_reports(os.path.join(tmp, "out_parent_markdup"), os.path.join(tmp, "out_this_markdup")))
        for name in ("this_markdup", "this_umi"):
            md = res["runs"][name]
            part = dict(median_ms={k: statistics.median(r["markdup_info"][k] for r in md) for k in ("sig_ms", "sort_ms", "mark_ms")},
                        info={k: v for k, v in md[0]["markdup_info"].items() if not k.endswith("_ms")})
            if "umi_info" in md[0]:
                part["umi_info"] = md[0]["umi_info"]
            if "markdup_profile" in md[0]:
                part["profile"] = md[0]["markdup_profile"]
                ms = part["median_ms"]["sort_ms"]
                part["radix_gb_per_s"] = md[0]["markdup_profile"]["radix_bytes"] / (ms / 1e3) / 1e9 if ms else None
            res[name] = part
        os.makedirs(a.out, exist_ok=True)
        json.dump(res, open(os.path.join(a.out, "markdup_umi_rates.json"), "w"), indent=1)
        print(json.dumps({k: v for k, v in res.items() if k != "runs"}))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
