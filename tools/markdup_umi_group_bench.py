"""What --umi-edits=1 costs and recovers: the input of tools/markdup_umi_bench.py -- 11.79 M shuffled records, a 10-base RX:Z tag on
every record, one UMI per fragment, a copied fragment keeping its original's UMI with probability one half -- with sequencing errors
in the copies' UMIs: each base of a copied fragment's UMI is substituted with probability --error (0.01), so a known share of the copies
sit one substitution from their original.  Three configurations, interleaved and rotated, `--reps` rounds, by the reference's
`Average Reads/Sec` window: the parent commit's binary with --umi-tag=RX (--parent-cli), this binary with --umi-tag=RX, this binary
with --umi-tag=RX --umi-edits=1.  Off: this --umi-tag=RX against the parent's, inside the spread of the parent's own runs, every report
file equal.  On: reads/s, group_ms and its split by kernel (RSQC_MARKDUP_PROFILE synchronises behind each), nodes, merged nodes, the
fragments recovered over exact matching, and the keys the parents kernel looks up per second.

    python tools/markdup_umi_group_bench.py [--records 10000000] [--dup-share 0.15] [--error 0.01] [--reps 9] [--parent-cli PATH] [--out profiles] [--tmp DIR]

Writes <out>/markdup_umi_group_rates.json.  Without --parent-cli the first question is left open (parent: false).

That input's position sets are small (2.3 nodes where a node has company at all).  --dense-only adds what the parents kernel does on
LARGE sets to an existing <out>/markdup_umi_group_rates.json ("dense"): about a million nodes in position sets of 16, 256 and 4 096
distinct 10-base UMIs -- a quarter of them molecules with 2 to 6 anchors, each with three single-anchor copies one substitution away
-- submitted through the C ABI, three passes each, the kernel clocks of RSQC_MARKDUP_PROFILE."""
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402

import markdup_umi_bench as ub  # noqa: E402
from rnaseqc_amd import bamio, synth  # noqa: E402

CLI = ub.CLI
NUM = ub.NUM
GROUP_LINE = re.compile(r"UMIs grouped: umi_nodes (\d+), merged_nodes (\d+), exact_duplicate_fragments (\d+), group_ms " + NUM)
GROUP_PROFILE = re.compile(r"markdup group: nodes (\d+), sets (\d+), heads_scans_ms " + NUM + ", nodes_ms " + NUM + ", parents_ms " + NUM + ", roots_ms " + NUM + ", marks_ms " + NUM + r", device_bytes (\d+)")
GROUP_PROBES = re.compile(r"markdup group: merged_nodes (\d+), probes (\d+)")
KERNEL_MS = ("heads_scans_ms", "nodes_ms", "parents_ms", "roots_ms", "marks_ms")


def run_cli(cli, flags, gtf, path, out, timeout=1200):
    t0 = time.time()
    p = subprocess.run([cli, *flags, gtf, path, out, "-s", "x", "-vv"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout, env=dict(os.environ, RSQC_MARKDUP_PROFILE="1"))
    wall = time.time() - t0
    so, se = p.stdout.decode(), p.stderr.decode()
    if p.returncode:
        raise RuntimeError("%s %s: exit %d\n%s" % (cli, flags, p.returncode, se[-2000:]))
    m = re.search(r"Average Reads/Sec: ([0-9.e+]+)", so)
    r = dict(reads_per_s_window=float(m.group(1)) if m else None, wall_s=wall)
    d = ub.MARK_LINE.search(so)
    if d:
        keys = ("records", "population", "anchors", "sets", "duplicate_fragments", "flagged_records", "cleared_records")
        r["markdup_info"] = dict({k: int(d.group(i + 1)) for i, k in enumerate(keys)}, sig_ms=float(d.group(8)), sort_ms=float(d.group(9)), mark_ms=float(d.group(10)))
    u = ub.UMI_LINE.search(so)
    if u:
        r["umi_info"] = dict(anchors_with_umi=int(u.group(1)), anchors_without_umi=int(u.group(2)), position_duplicate_fragments=int(u.group(3)))
    q = ub.PROFILE_LINE.search(se)
    if q:
        r["device_bytes"] = int(q.group(6))
    g = GROUP_LINE.search(so)
    if g:
        r["group_info"] = dict(umi_nodes=int(g.group(1)), merged_nodes=int(g.group(2)), exact_duplicate_fragments=int(g.group(3)), group_ms=float(g.group(4)))
    k = GROUP_PROFILE.search(se)
    if k:
        r["group_profile"] = dict(nodes=int(k.group(1)), sets=int(k.group(2)), device_bytes=int(k.group(8)), **{n: float(k.group(3 + i)) for i, n in enumerate(KERNEL_MS)})
    b = GROUP_PROBES.search(se)
    if b:
        r["probes"] = int(b.group(2))
    return r


def with_umi_errors(base, both, error, seed):
    """Each base of the UMI of a COPIED fragment (the records behind the base's) substituted with probability `error`: one draw per
    fragment name, so mates share it.  Returns how many copied fragments got 0, 1 and more substitutions."""
    r = np.random.default_rng(seed)
    names, k = np.unique(both.qhash[base.n:], return_inverse=True)
    hit = r.random((len(names), ub.UMI_BASES)) < error
    x = r.integers(1, 4, (len(names), ub.UMI_BASES), dtype=np.uint64)
    delta = np.zeros(len(names), np.uint64)
    for j in range(ub.UMI_BASES):
        delta |= np.where(hit[:, j], x[:, j] << np.uint64(2 * j), np.uint64(0)).astype(np.uint64)
    both.umi[base.n:] = both.umi[base.n:] ^ delta[k]
    n_sub = hit.sum(axis=1)
    return int((n_sub == 0).sum()), int((n_sub == 1).sum()), int((n_sub > 1).sum())


DENSE_SETS = ((65536, 16), (4096, 256), (256, 4096))         # (position sets, nodes per set): 2^20 nodes each


def dense_batch(n_sets, per_set):
    """n_sets position sets (single reads, 100 bases apart), in each per_set // 4 distinct 10-base UMIs with 2 to 6 anchors (a random start
    and an odd stride: distinct modulo 4^10) and three single-anchor copies one substitution away each; shuffled, names unique."""
    from rnaseqc_amd.model import Batch
    r = np.random.default_rng(per_set)
    molecules = per_set // 4
    start, stride = r.integers(0, 1 << 20, n_sets, dtype=np.uint64), (r.integers(0, 1 << 19, n_sets, dtype=np.uint64) * np.uint64(2) + np.uint64(1))
    true = (start[:, None] + stride[:, None] * np.arange(molecules, dtype=np.uint64)[None, :]) & np.uint64((1 << 20) - 1)
    count = r.integers(2, 7, true.shape)
    j = r.integers(0, ub.UMI_BASES, true.shape + (3,)).astype(np.uint64)
    x = r.integers(1, 4, true.shape + (3,)).astype(np.uint64)
    child = true[:, :, None] ^ (x << (np.uint64(2) * j))
    set_of_true = np.repeat(np.arange(n_sets), molecules)
    umi = np.concatenate([np.repeat(true.ravel(), count.ravel()), child.ravel()]) | np.uint64(1 << 20)
    pos = np.concatenate([np.repeat(set_of_true, count.ravel()), np.repeat(set_of_true, 3)]).astype(np.int64) * 100 + 1000
    order = r.permutation(len(umi))
    b = Batch.from_records([dict(qname="r", tid=0, pos=1000, cigar=[(0, 50)], flag=0, mapq=60)]).take(np.zeros(len(umi), np.int64))
    b.qname = b.qname_off = b.qhash2 = None
    b.pos = pos[order].astype(b.pos.dtype); b.umi = umi[order].astype(np.uint64)
    b.qhash = np.arange(len(umi), dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(1)
    return b


def dense_child():
    """Runs in a process of its own (the library's profile lines go to ITS stderr): for every shape of DENSE_SETS three grouped passes."""
    os.environ["RSQC_MARKDUP_PROFILE"] = "1"
    from rnaseqc_amd import abi, engine
    ann = synth.make_annotation(seed=61, contigs=[("chr1", 50_000_000, 600)])
    e = engine.Engine(abi.default_params())
    e.set_annotation(ann)
    for n_sets, per_set in DENSE_SETS:
        b = dense_batch(n_sets, per_set)
        for _rep in range(3):
            e.reset()
            e.sort_begin(); e.markdup_begin(); e.markdup_use_umi(); e.markdup_umi_edits(1)
            e.submit(b)
            e.sort_end()
            info, g = e.markdup_end(), e.markdup_umi_group_end()
            print("dense", json.dumps(dict(position_sets=n_sets, nodes_per_set_at_most=per_set, anchors=info["anchors"], duplicate_fragments=info["duplicate_fragments"], **g)), flush=True)
    e.close()


def dense(out_dir):
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--dense-child"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    so, se = p.stdout.decode(), p.stderr.decode()
    if p.returncode:
        raise RuntimeError("dense child: exit %d\n%s" % (p.returncode, se[-3000:]))
    infos = [json.loads(l[6:]) for l in so.splitlines() if l.startswith("dense ")]
    kernels, probes = GROUP_PROFILE.findall(se), GROUP_PROBES.findall(se)
    assert len(infos) == len(kernels) == len(probes) == 3 * len(DENSE_SETS), (len(infos), len(kernels), len(probes))
    shapes = []
    for s in range(len(DENSE_SETS)):
        rows = range(3 * s, 3 * s + 3)
        ms = {n: statistics.median(float(kernels[k][2 + i]) for k in rows) for i, n in enumerate(KERNEL_MS)}
        shapes.append(dict(infos[3 * s], group_ms=statistics.median(infos[k]["group_ms"] for k in rows), nodes=int(kernels[3 * s][0]), sets=int(kernels[3 * s][1]),
                           median_kernel_ms=ms, probes=int(probes[3 * s][1]), probes_per_s=int(probes[3 * s][1]) / (ms["parents_ms"] / 1e3)))
        print(json.dumps(shapes[-1]), flush=True)
    path = os.path.join(out_dir, "markdup_umi_group_rates.json")
    res = json.load(open(path))
    res["dense"] = shapes
    json.dump(res, open(path, "w"), indent=1)


def main():
    if "--dense-child" in sys.argv:
        return dense_child()
    ap = argparse.ArgumentParser()
    ap.add_argument("--dense-only", action="store_true", help="add the large-set measurement to an existing <out>/markdup_umi_group_rates.json and stop")
    ap.add_argument("--records", type=int, default=10_000_000)
    ap.add_argument("--dup-share", type=float, default=0.15)
    ap.add_argument("--error", type=float, default=0.01)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--parent-cli", default=None, help="the rnaseqc binary of the parent commit (built beside its own library)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--tmp", default=None)
    ap.add_argument("--threads", type=int, default=16)
    a = ap.parse_args()
    if a.dense_only:
        return dense(a.out)
    tmp = tempfile.mkdtemp(dir=a.tmp)
    try:
        contigs = [("chr%d" % k, 50_000_000, 600) for k in range(1, 5)]
        ann = synth.make_annotation(seed=61, contigs=contigs)
        t0 = time.time()
        base = bamio.sam_consistent(synth.make_reads(ann, a.records // 2, seed=62, contig_lengths=np.array([c[1] for c in contigs]), umi_bases=ub.UMI_BASES))
        both, n_copied, n_kept = ub.with_duplicates(base, a.dup_share, 64)
        subs = with_umi_errors(base, both, a.error, 65)
        shuffled = both.take(np.random.default_rng(63).permutation(both.n))
        cs = [(c[0], c[1]) for c in contigs]
        bam, gtf = os.path.join(tmp, "shuffled_rx.bam"), os.path.join(tmp, "x.gtf")
        bamio.write_gtf(gtf, ann)
        bamio.write_bam_fast(bam, cs, shuffled, threads=a.threads, seq_mode=1)
        res = dict(base_records=int(base.n), records=int(shuffled.n), fragments_copied=n_copied, copies_with_the_originals_umi=n_kept, umi_bases=ub.UMI_BASES, dup_share=a.dup_share,
                   error_per_base=a.error, copied_fragments_with_0_1_more_substitutions=subs, input_s=time.time() - t0, bytes=os.path.getsize(bam), reps=a.reps,
                   parent=a.parent_cli is not None, runs={})
        configs = [("this_umi", CLI, ["--umi-tag=RX"]), ("this_umi_edits", CLI, ["--umi-tag=RX", "--umi-edits=1"])]
        if a.parent_cli:
            configs.insert(0, ("parent_umi", a.parent_cli, ["--umi-tag=RX"]))
        for rep in range(a.reps):                               # interleaved and rotated: drift of the box lands on every configuration alike
            for name, cli, flags in configs[rep % len(configs):] + configs[:rep % len(configs)]:
                out = os.path.join(tmp, "out_" + name)
                shutil.rmtree(out, ignore_errors=True)
                r = run_cli(cli, flags, gtf, bam, out)
                res["runs"].setdefault(name, []).append(r)
                print(rep, name, json.dumps(r), flush=True)
        med = {n: statistics.median(r["reads_per_s_window"] for r in rs) for n, rs in res["runs"].items()}
        res["median_reads_per_s_window"] = med
        res["spread_reads_per_s_window"] = {n: [min(r["reads_per_s_window"] for r in rs), max(r["reads_per_s_window"] for r in rs)] for n, rs in res["runs"].items()}
        res["on_ratio_to_this_umi"] = med["this_umi_edits"] / med["this_umi"]
        if a.parent_cli:
            rates = [r["reads_per_s_window"] for r in res["runs"]["parent_umi"]]
            res["off"] = dict(parent_min=min(rates), parent_max=max(rates), parent_median=med["parent_umi"], this_median=med["this_umi"], ratio=med["this_umi"] / med["parent_umi"],
                              inside_parent_spread=min(rates) <= med["this_umi"] <= max(rates) or med["this_umi"] >= med["parent_umi"],
                              reports_equal=ub.same_reports(os.path.join(tmp, "out_parent_umi"), os.path.join(tmp, "out_this_umi")),
                              device_bytes_equal=res["runs"]["parent_umi"][0].get("device_bytes") == res["runs"]["this_umi"][0].get("device_bytes"))
        for name in ("this_umi", "this_umi_edits"):
            md = res["runs"][name]
            res[name] = dict(median_ms={k: statistics.median(r["markdup_info"][k] for r in md) for k in ("sig_ms", "sort_ms", "mark_ms")},
                             info={k: v for k, v in md[0]["markdup_info"].items() if not k.endswith("_ms")}, umi_info=md[0]["umi_info"], device_bytes=md[0].get("device_bytes"))
        on, runs = res["this_umi_edits"], res["runs"]["this_umi_edits"]
        on["group_info"] = {k: v for k, v in runs[0]["group_info"].items() if k != "group_ms"}
        on["median_group_ms"] = statistics.median(r["group_info"]["group_ms"] for r in runs)
        on["median_kernel_ms"] = {k: statistics.median(r["group_profile"][k] for r in runs) for k in KERNEL_MS}
        on["nodes"], on["position_sets"], on["probes"] = runs[0]["group_profile"]["nodes"], runs[0]["group_profile"]["sets"], runs[0]["probes"]
        on["probes_per_s"] = on["probes"] / (on["median_kernel_ms"]["parents_ms"] / 1e3) if on["median_kernel_ms"]["parents_ms"] else None
        on["fragments_recovered_over_exact_matching"] = on["info"]["duplicate_fragments"] - on["group_info"]["exact_duplicate_fragments"]
        assert on["group_info"]["exact_duplicate_fragments"] == res["this_umi"]["info"]["duplicate_fragments"]
        os.makedirs(a.out, exist_ok=True)
        json.dump(res, open(os.path.join(a.out, "markdup_umi_group_rates.json"), "w"), indent=1)
        print(json.dumps({k: v for k, v in res.items() if k != "runs"}))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    dense(a.out)


if __name__ == "__main__":
    main()
