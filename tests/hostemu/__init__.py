"""TEST HARNESS: the product's per-record core compiled for the host (see hostemu.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np

from rnaseqc_amd import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "libhostemu.so")
_ROOT = os.path.dirname(os.path.dirname(_HERE))


def build():
    srcs = [os.path.join(_HERE, "hostemu.cpp"), os.path.join(_ROOT, "rnaseqc_amd", "csrc", "rsqc_read.h"),
            os.path.join(_ROOT, "rnaseqc_amd", "csrc", "rsqc_index.h"), os.path.join(_ROOT, "include", "rnaseqc_amd.h")]
    if not os.path.exists(_SO) or any(os.path.getmtime(_SO) < os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-fvisibility=hidden", srcs[0], "-o", _SO])
    return _SO


class Out:
    pass


def run(params, ann, batch, mode=1, want_cov=False):
    """mode 1: the elementary-interval feature stage (what the per-record kernel runs), 0: the row-table one."""
    lib = C.CDLL(build())
    lib.hostemu_set_mode(int(mode))
    a, b = ann.to_struct(), batch.to_struct()
    o = Out()
    G, E = ann.n_genes_listed, ann.n_exons
    o.counters = np.zeros(abi.N_COUNTERS, np.uint64)
    o.gene_reads = np.zeros(G, np.uint64); o.gene_unique = np.zeros(G, np.uint64); o.gene_fragments = np.zeros(G, np.uint64)
    o.exon_reads = np.zeros(E, np.float64)
    rl, nov = C.c_int32(), C.c_uint64()
    o.cov = None
    if want_cov:
        total = int(sum(int(ann.exon_row_end[i]) - int(ann.exon_row_start[i]) + 1 for i in range(E))) + ann.n_genes + 8
        o.cov = np.zeros(total, np.uint32)
    rc = lib.hostemu_run(C.byref(params), C.byref(a), C.byref(b), abi.ptr(o.counters), abi.ptr(o.gene_reads),
                         abi.ptr(o.gene_unique), abi.ptr(o.gene_fragments), abi.ptr(o.exon_reads), C.byref(rl),
                         abi.ptr(o.cov) if want_cov else None, C.byref(nov))
    if rc:
        raise RuntimeError("hostemu rc=%d" % rc)
    o.read_length = rl.value
    o.n_overflow = nov.value
    return o


_K1SO = os.path.join(_HERE, "libk1emu.so")
_K1SO_DEFAULT = os.path.join(_HERE, "libk1emu_default.so")


def build_k1(coarse=True):
    """coarse=True: the kernel with its opt-in paths compiled in (-DK1E_COARSE, the coarse table; -DK1E_UNIFORM2=1, the wave-uniform
    two-block path: a superset of the default code, so the suite exercises all look-up paths); coarse=False: the product's default configuration."""
    csrc = os.path.join(_ROOT, "rnaseqc_amd", "csrc")
    so = _K1SO if coarse else _K1SO_DEFAULT
    srcs = [os.path.join(_HERE, "k1_emu.cpp"), os.path.join(_HERE, "wavemu.h")] + \
           [os.path.join(csrc, f) for f in ("rsqc_read.h", "rsqc_index.h", "rsqc_k1.h", "rsqc_k1s.h", "rsqc_kr.h", "rsqc_rl_compose.h", "rsqc_k4.h", "rsqc_wave.h", "rsqc_device.h")] + \
           [os.path.join(_ROOT, "include", "rnaseqc_amd.h")]
    # (RSQC_EMU_DEFS="-DK1E_..." : the emulation of an A/B build of the kernel; remove the .so files before and after)
    if not os.path.exists(so) or any(os.path.getmtime(so) < os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-fvisibility=hidden", "-Wno-unused-function",
                               "-Wno-unused-variable"] + (["-DK1E_COARSE", "-DK1E_UNIFORM2=1"] if coarse else []) + os.environ.get("RSQC_EMU_DEFS", "").split() + [srcs[0], "-o", so])
    return so


STAGE_POISON = 0xDEADDEADDEADDEAD
STAGE_SLOTS = 1024                     # K1E_OVF_STAGE (rsqc_k1.h)


def run_overflow_script(start, calls, seed=0, cap=1 << 16):
    """k1e_overflow + the flush of classify_long_kernel's tail (rsqc_k1.h), one workgroup of four waves under the emulation.
    start: entries already staged; calls: four lists (one per wave) of 64-bit lane masks, one k1e_overflow call each;
    seed: wavemu.h's seeded schedule (0: round-robin).  Returns (list entries as a uint64 array, expected entries, (counter, end))."""
    lib = C.CDLL(build_k1(True))
    assert len(calls) == 4
    flat = np.array([m for w in calls for m in w] + [0], np.uint64)
    n_calls = np.array([len(w) for w in calls], np.uint32)
    first = np.concatenate([[0], np.cumsum(n_calls)[:-1]]).astype(np.uint32)
    out = np.zeros(cap, np.uint64); count = C.c_uint32(0); ctl = np.zeros(2, np.uint32)
    lib.k1emu_set_schedule_seed.argtypes = [C.c_ulonglong]
    lib.k1emu_overflow_script.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    lib.k1emu_set_schedule_seed(int(seed))
    try:
        rc = lib.k1emu_overflow_script(int(start), flat.ctypes.data, first.ctypes.data, n_calls.ctypes.data, STAGE_POISON, out.ctypes.data, cap,
                                       C.addressof(count), ctl.ctypes.data)
    finally:
        lib.k1emu_set_schedule_seed(0)
    if rc:
        raise RuntimeError("k1emu_overflow_script rc=%d" % rc)
    want = [(1 << 48) | j for j in range(start)]
    for w, masks in enumerate(calls):
        for c, m in enumerate(masks):
            want += [(w << 40) | (c << 8) | l for l in range(64) if (int(m) >> l) & 1]
    return out[:count.value].copy(), np.array(sorted(want), np.uint64), (int(ctl[0]), int(ctl[1]))


def run_k1(params, ann, batch, grid=2, want_cov=False, slow_kernel=True, coarse=True, bed=None, seed=0):
    """The per-record KERNELS (rsqc_k1.h) on the 64-lane fiber emulation of wavemu.h, `grid` workgroups of 256 lanes.
    seed != 0: wavemu.h's seeded schedule (random wave order, a yield after every atomic) instead of round-robin."""
    lib = C.CDLL(build_k1(coarse))
    lib.k1emu_set_schedule_seed.argtypes = [C.c_ulonglong]
    lib.k1emu_set_schedule_seed(int(seed))
    a, b = ann.to_struct(), batch.to_struct()
    o = Out()
    G, E = ann.n_genes_listed, ann.n_exons
    o.counters = np.zeros(abi.N_COUNTERS, np.uint64)
    o.gene_reads = np.zeros(G, np.uint64); o.gene_unique = np.zeros(G, np.uint64); o.gene_fragments = np.zeros(G, np.uint64)
    o.exon_reads = np.zeros(E, np.float64)
    rl = C.c_int32(); stats = np.zeros(4, np.uint64)
    o.cov = None
    if want_cov:
        total = int(sum(int(ann.exon_row_end[i]) - int(ann.exon_row_start[i]) + 1 for i in range(E))) + ann.n_genes + 8
        o.cov = np.zeros(total, np.uint32)
    bs = bed.to_struct() if bed is not None else None           # (with a BED: the --bed instance classify_ei_kernel<true>, candidates checked)
    rc = lib.k1emu_run_bed(C.byref(params), C.byref(a), C.byref(b), C.byref(bs) if bs is not None else None, C.c_int(grid), C.c_int(1 if slow_kernel else 0),
                           abi.ptr(o.counters), abi.ptr(o.gene_reads), abi.ptr(o.gene_unique), abi.ptr(o.gene_fragments), abi.ptr(o.exon_reads), C.byref(rl),
                           abi.ptr(o.cov) if want_cov else None, abi.ptr(stats))
    lib.k1emu_set_schedule_seed(0)
    if rc:
        raise RuntimeError("k1emu rc=%d" % rc)
    o.read_length = rl.value
    o.n_overflow = int(stats[0]); o.n_listed = int(stats[1]) & 0xFFFFFFFF; o.n_deferred = int(stats[1]) >> 32; o.n_pairs = int(stats[2]); o.n_coarse = int(stats[3]) if bed is None else 0; o.n_candidates = int(stats[3]) if bed is not None else 0
    if bed is not None:                                         # the candidates the kernel left, in file order (columns as K5_COLUMNS)
        cols = [np.zeros(max(o.n_candidates, 1), dt) for dt in (np.uint64, np.uint64, np.uint32, np.int32, np.int32, np.uint32)]
        lib.k1emu_last_candidates.argtypes = [C.c_void_p] * 6
        lib.k1emu_last_candidates(*[c.ctypes.data for c in cols])
        o.candidates = dict(zip(("file_index", "qhash", "h2", "interval", "endpos", "flag_size"), (c[:o.n_candidates] for c in cols)))
    lib.k1emu_uniform_calls.restype = C.c_ulonglong
    o.n_uniform = int(lib.k1emu_uniform_calls())
    lib.k1emu_ucache_hits.restype = C.c_ulonglong
    o.n_ucache_hits = int(lib.k1emu_ucache_hits())
    lib.k1emu_uniform2_calls.restype = C.c_ulonglong
    o.n_uniform2 = int(lib.k1emu_uniform2_calls())
    return o


_K4SO = os.path.join(_HERE, "libk4emu.so")


def build_k4():
    csrc = os.path.join(_ROOT, "rnaseqc_amd", "csrc")
    srcs = [os.path.join(_HERE, "k4_emu.cpp"), os.path.join(_HERE, "wavemu.h")] + \
           [os.path.join(csrc, f) for f in ("rsqc_k4.h", "rsqc_wave.h", "rsqc_device.h", "rsqc_read.h")]
    if not os.path.exists(_K4SO) or any(os.path.getmtime(_K4SO) < os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-fvisibility=hidden", "-Wno-unused-function",
                               "-Wno-unused-variable", srcs[0], "-o", _K4SO])
    return _K4SO


def run_k4(seed, n_genes, n_chunks, n_names, hot_reads, arena=False, wide=False):
    """The fragment-counting KERNELS (rsqc_k4.h) on the 64-lane fiber emulation against a std::set per gene.
    Returns (rc, stats): rc 0 = every gene's count equals its name set; stats = pairs, keys kept by frag_local, partitions,
    partitions left to the second counting instance, distinct (gene, name) pairs, chunk capacity."""
    lib = C.CDLL(build_k4())
    lib.k4emu_run.argtypes = [C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    st = np.zeros(6, np.uint64)
    rc = lib.k4emu_run(seed, n_genes, n_chunks, n_names, hot_reads, (1 if arena else 0) | (2 if wide else 0), st.ctypes.data)
    return rc, dict(zip(("pairs", "kept", "partitions", "fuller", "distinct", "chunk_cap"), (int(x) for x in st)))


K4_PART_READS, K4_SUB_CAP, K4_PART_SLOTS = 1024, 2048, 4096       # rsqc_device.h


def k4_bounds(n_pairs, n_genes):
    """(parts_bound, keys_bound) of rsqc_finalize.cpp from the host's pair bound."""
    parts = n_pairs // K4_PART_READS + n_genes + 1
    keys = 2 * n_pairs + K4_SUB_CAP * min(parts, n_pairs // K4_PART_READS + 1) + 16 * n_genes + 16
    return parts, keys


def run_k4_pairs(gene, key, h2, n_genes, counts, chunk_cap, slow_cap, sharers, grid_small, grid_large, seed=0):
    """The fragment-counting KERNELS (rsqc_k4.h) over pairs laid out by the caller (k4_emu.cpp: k4emu_run_pairs).  counts: pairs per
    chunk, then the pairs of the dense region (one entry alone: the dense form); seed: wavemu.h's seeded schedule (0: round-robin).
    Returns an Out: rc, error, gene_frag[G], part_first[G + 1], ginfo[G, 4], part_info[n_parts, 4], cursor[n_parts] (the fills
    frag_local left), full_list[full_n] sorted, full_n."""
    lib = C.CDLL(build_k4())
    lib.k4emu_run_pairs.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32,
                                    C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64] + [C.c_void_p] * 8
    gene = np.ascontiguousarray(gene, np.uint32); key = np.ascontiguousarray(key, np.uint64); h2 = np.ascontiguousarray(h2, np.uint32)
    cnt = np.ascontiguousarray(counts, np.uint32)
    n = len(gene)
    assert len(key) == n and len(h2) == n and len(cnt) >= 1
    pb, kb = k4_bounds(n, n_genes)
    o = Out()
    err = C.c_int(0); full_n = C.c_uint32(0)
    o.gene_frag = np.zeros(n_genes, np.uint64); part_first = np.zeros(n_genes + 1, np.uint32); ginfo = np.zeros((n_genes, 4), np.uint32)
    part_info = np.zeros((pb, 4), np.uint32); cursor = np.zeros(pb, np.uint32); full_list = np.zeros(pb, np.uint32)
    o.rc = lib.k4emu_run_pairs(gene.ctypes.data, key.ctypes.data, h2.ctypes.data, n, n_genes, len(cnt) - 1, chunk_cap, cnt.ctypes.data, slow_cap,
                               sharers, grid_small, grid_large, int(seed), pb, kb, C.addressof(err), o.gene_frag.ctypes.data, part_first.ctypes.data,
                               ginfo.ctypes.data, part_info.ctypes.data, cursor.ctypes.data, full_list.ctypes.data, C.addressof(full_n))
    o.error = err.value; o.full_n = full_n.value
    o.part_first = part_first.astype(np.int64); o.ginfo = ginfo.astype(np.int64)
    o.n_parts = int(part_first[n_genes]) if o.rc != -1004 else 0
    np_ = min(o.n_parts, pb)
    o.part_info = part_info[:np_].astype(np.int64); o.cursor = cursor[:np_].astype(np.int64)
    o.full_list = np.sort(full_list[:min(o.full_n, pb)].astype(np.int64))
    return o


_K3SO = os.path.join(_HERE, "libk3emu.so")


def build_k3():
    csrc = os.path.join(_ROOT, "rnaseqc_amd", "csrc")
    srcs = [os.path.join(_HERE, "k3_emu.cpp"), os.path.join(_HERE, "wavemu.h")] + \
           [os.path.join(csrc, f) for f in ("rsqc_k3.h", "rsqc_k3_plan.h", "rsqc_wave.h", "rsqc_device.h", "rsqc_read.h", "rsqc_index.h")]
    if not os.path.exists(_K3SO) or any(os.path.getmtime(_K3SO) < os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-fvisibility=hidden", "-Wno-unused-function",
                               "-Wno-unused-variable", srcs[0], "-o", _K3SO])
    return _K3SO


def run_k3(params, ann, cov_diff, gene_reads, force=0):
    """The end-of-file coverage KERNEL (rsqc_k3.h) on the 64-lane fiber emulation: from the difference array and the gene counts
    of a pass (hostemu.run(..., want_cov=True)) to per-gene mean / std / CV, per-exon CV and the bias accumulators.  The launches are
    the library's own plan (rsqc_k3_plan.h); `launches`: genes per launch, in launch order; `classes`: genes per workgroup class
    (1024 threads / 146 KB, 1024 / 64 KB, 256, one wave)."""
    lib = C.CDLL(build_k3())
    a = ann.to_struct()
    o = Out()
    G, E = ann.n_genes_listed, ann.n_exons
    o.gene_cov_mean = np.zeros(G, np.float64); o.gene_cov_std = np.zeros(G, np.float64); o.gene_cov_cv = np.zeros(G, np.float64)
    o.gene_cov_valid = np.zeros(G, np.uint8); o.exon_cv = np.zeros(E, np.float64); o.exon_cv_valid = np.zeros(E, np.uint8)
    o.bias_three = np.zeros(G, np.uint64); o.bias_five = np.zeros(G, np.uint64)
    stats = np.zeros(K3_LAUNCHES, np.uint64)
    cov = np.ascontiguousarray(cov_diff, np.uint32); gr = np.ascontiguousarray(gene_reads, np.uint64)
    rc = lib.k3emu_run(C.byref(params), C.byref(a), abi.ptr(cov), abi.ptr(gr), C.c_int(force), abi.ptr(o.gene_cov_mean), abi.ptr(o.gene_cov_std),
                       abi.ptr(o.gene_cov_cv), abi.ptr(o.gene_cov_valid), abi.ptr(o.exon_cv), abi.ptr(o.exon_cv_valid),
                       abi.ptr(o.bias_three), abi.ptr(o.bias_five), abi.ptr(stats))
    o.rc = rc
    o.launches = [int(x) for x in stats]
    o.classes = [o.launches[0], o.launches[3], o.launches[1] + o.launches[2], sum(o.launches[4:])]
    return o


K3_LAUNCHES = 8
K3_PLAN_COLUMNS = ("threads", "cov_bits", "cap", "count", "first", "stream")
K3_COUNT_NAMES = ("n_large", "n_medium", "n_xlarge", "n_le6144", "n_le3072", "n_le2048", "n_le1024")


def _plan_rows(out):
    return [dict(zip(K3_PLAN_COLUMNS, (int(x) for x in out[k * 6:k * 6 + 6]))) for k in range(K3_LAUNCHES)]


def k3_plan(n, n_large, n_medium, n_xlarge, n_le6144, n_le3072, n_le2048, n_le1024):
    """The library's launch plan of the coverage stage (rsqc_k3_plan.h: k3_plan) from class counts as given, no kernel run: eight dicts
    of K3_PLAN_COLUMNS in launch order."""
    lib = C.CDLL(build_k3())
    lib.k3emu_plan.argtypes = [C.c_uint32] * 8 + [C.c_void_p]
    lib.k3emu_plan.restype = None
    out = np.zeros(K3_LAUNCHES * 6, np.uint32)
    lib.k3emu_plan(n, n_large, n_medium, n_xlarge, n_le6144, n_le3072, n_le2048, n_le1024, out.ctypes.data)
    return _plan_rows(out)


def k3_plan_many(lengths, ns, force=0, delta=None):
    """... from coding lengths, the way the emulation (and, for force=0, the library) gets there, for many length vectors at once: row r
    of `lengths` (m x width) holds ns[r] lengths; they are sorted longest first, the classes counted by k3_count_classes, `force` applied,
    `delta` (m x 7, K3_COUNT_NAMES order) added to the counts, then k3_plan.  Returns (counts m x 7, plans m x 8 x 6 in K3_PLAN_COLUMNS
    order, sorted lengths m x width), all int64."""
    lib = C.CDLL(build_k3())
    lib.k3emu_plan_many.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.k3emu_plan_many.restype = None
    ln = np.ascontiguousarray(lengths, np.uint32)
    m, width = ln.shape
    nn = np.ascontiguousarray(ns, np.uint32)
    assert nn.shape == (m,) and (m == 0 or int(nn.max()) <= width)
    dl = None if delta is None else np.ascontiguousarray(delta, np.int32)
    assert dl is None or dl.shape == (m, 7)
    counts = np.zeros((m, 7), np.uint32); out = np.zeros((m, K3_LAUNCHES, 6), np.uint32); srt = np.zeros((m, width), np.uint32)
    lib.k3emu_plan_many(ln.ctypes.data, nn.ctypes.data, m, width, int(force), None if dl is None else dl.ctypes.data, counts.ctypes.data,
                        out.ctypes.data, srt.ctypes.data)
    return counts.astype(np.int64), out.astype(np.int64), srt.astype(np.int64)


_K5SO = os.path.join(_HERE, "libk5emu.so")


def build_k5():
    csrc = os.path.join(_ROOT, "rnaseqc_amd", "csrc")
    srcs = [os.path.join(_HERE, "k5_emu.cpp"), os.path.join(_HERE, "wavemu.h")] + [os.path.join(csrc, f) for f in ("rsqc_k5.h", "rsqc_k5_plan.h", "rsqc_device.h", "rsqc_read.h")]
    if not os.path.exists(_K5SO) or any(os.path.getmtime(_K5SO) < os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-fvisibility=hidden", "-Wno-unused-function",
                               "-Wno-unused-variable", srcs[0], "-o", _K5SO])
    return _K5SO


def run_k5(seed, n_names, max_samples, hot=0):
    """The fragment-size KERNELS (rsqc_k5.h) on the 64-lane fiber emulation against a literal std::map walk in file order.
    hot: records of one extra name (a bucket beyond the LDS sort); -1: one or two candidates per name + crafted collisions of the set's mix.  Returns (rc, candidates, samples, kept, distinct sizes, listed buckets)."""
    lib = C.CDLL(build_k5())
    lib.k5emu_run.argtypes = [C.c_uint64, C.c_int, C.c_uint32, C.c_int, C.c_void_p]
    stats = np.zeros(7, np.uint64)
    rc = lib.k5emu_run(seed, n_names, max_samples, hot, stats.ctypes.data)
    run_k5.last_paths = (int(stats[5]), int(stats[6]))          # buckets paired through the LDS set / handed to the sort (pair_bucket_hashed)
    return (rc,) + tuple(int(x) for x in stats[:5])


K5_COLUMNS = ("file_index", "qhash", "h2", "interval", "endpos", "flag_size")
_K5_DTYPES = (np.uint64, np.uint64, np.uint32, np.int32, np.int32, np.uint32)
K5_PATHS = ("empty", "set", "sort", "listed")                  # the path codes of k5_emu.cpp, per bucket


def _k5_lib():
    lib = C.CDLL(build_k5())
    lib.k5emu_run_cands.argtypes = [C.c_void_p] * 6 + [C.c_uint32, C.c_uint32, C.c_uint64]
    lib.k5emu_partition.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64]
    lib.k5emu_info.argtypes = [C.c_void_p]; lib.k5emu_info.restype = None
    lib.k5emu_fetch.argtypes = [C.c_int, C.c_void_p]; lib.k5emu_fetch.restype = None
    return lib


def _k5_collect(lib, rc, full):
    o = Out()
    info = np.zeros(12, np.uint64)
    lib.k5emu_info(info.ctypes.data)
    o.rc = rc
    o.n, o.n_buckets, o.n_samples, o.n_kept, o.top, o.n_beyond, o.n_pairs = (int(x) for x in info[:7])
    o.error = int(info[7].astype(np.int64)); o.big0 = int(info[8]); o.state = (int(info[9]), int(info[10])); o.n_table_pairs = int(info[11])

    def fetch(what, count, dt):
        a = np.zeros(max(count, 1), dt)
        lib.k5emu_fetch(what, a.ctypes.data)
        return a[:count]
    if rc == 0 and o.n:
        o.count = fetch(0, o.n_buckets, np.uint32).astype(np.int64); o.off = fetch(1, o.n_buckets + 1, np.uint32).astype(np.int64)
        o.listed = np.sort(fetch(2, min(o.big0, 1024), np.uint32).astype(np.int64)); o.perm = fetch(11, o.n, np.uint32).astype(np.int64)
        if full:
            o.path = fetch(3, o.n_buckets, np.uint8).astype(np.int64)
            o.raw = sorted(zip(fetch(4, o.n_samples, np.uint64).tolist(), fetch(5, o.n_samples, np.uint32).tolist()))
            o.kept = sorted(zip(fetch(6, o.n_kept, np.uint64).tolist(), fetch(7, o.n_kept, np.uint32).tolist()))
            o.beyond = fetch(8, o.n_beyond, np.uint32).tolist()
            o.pairs = list(zip(fetch(9, o.n_pairs, np.uint32).tolist(), fetch(10, o.n_pairs, np.uint32).tolist()))
    return o


def run_k5_cands(columns, max_samples, seed=0):
    """The fragment-size KERNELS (rsqc_k5.h) over candidate columns given by the caller (K5_COLUMNS, emission order), launched by the
    library's own plan (rsqc_k5_plan.h); seed: wavemu.h's seeded schedule (0: round-robin).  Returns an Out: rc (0, or 1100 + k: a guard
    entry behind an array was written), error (the device error word), count / off per bucket, listed (bucket numbers, sorted), path per
    bucket (index into K5_PATHS), raw and kept samples as sorted (file index, size) lists, state (the select's prefix and remaining rank),
    top, beyond (the sizes of 2^20 and more, ascending), pairs [(size, count)] as the host merges them, n_table_pairs, perm."""
    lib = _k5_lib()
    cols = [np.ascontiguousarray(columns[f], dt) for f, dt in zip(K5_COLUMNS, _K5_DTYPES)]
    n = len(cols[0])
    assert all(len(c) == n for c in cols)
    rc = lib.k5emu_run_cands(*[c.ctypes.data for c in cols], n, int(max_samples), int(seed))
    return _k5_collect(lib, rc, True)


def run_k5_partition(qhash, seed=0):
    """pair_bucket_count / scan / scatter alone: rc, error, count, off, listed, big0 (the scan's own count of listed buckets), perm."""
    lib = _k5_lib()
    q = np.ascontiguousarray(qhash, np.uint64)
    rc = lib.k5emu_partition(q.ctypes.data, len(q), int(seed))
    return _k5_collect(lib, rc, False)


K5_PROGRAM_SOURCE = os.path.join(_HERE, "k5_emu.cpp")          # with -DK5EMU_MAIN: a stand-alone program over a case file


def write_k5_case_file(path, columns, max_samples, seed=0, partition_only=False):
    """the case file the stand-alone program reads (k5_emu.cpp: main)"""
    cols = [np.ascontiguousarray(columns[f], dt) for f, dt in zip(K5_COLUMNS, _K5_DTYPES)]
    with open(path, "wb") as f:
        f.write(np.array([len(cols[0]), max_samples, seed, 1 if partition_only else 0], np.uint64).tobytes())
        for c in cols:
            f.write(c.tobytes())


RL_SUMMARY_WORDS, RL_MAXP = 2 + 2 * 128, 128                   # RSQC_RL_SUMMARY_WORDS (rsqc_device.h), RSQC_RL_MAXP (rsqc_kr.h)
RL_POISON = 0xA5A5A5A5
K1_PROGRAM_SOURCE = os.path.join(_HERE, "k1_emu.cpp")          # with -DK1EMU_MAIN: a stand-alone program over KR case files


def run_kr(params, ann, batch, grid=2, r_in=0, ranges=False, coarse=True):
    """The Read-Length stage under the emulation (k1_emu.cpp: k1emu_run_kr): the per-record kernels produce tile_span and the extremes, then
    read_length_kernel (rsqc_kr.h) runs from the entry state `r_in`, or -- ranges=True, a batch of Batch.concat_ranges -- with rl_seg armed
    as the library arms it and one block per segment.  Returns an Out: rc (0, an RSQC_ERR_* code, 1000 + k: an internal check of the
    harness), error (the device error word), tile_span, extremes [entries, 3] (max span, min l_qseq, max l_qseq), per entry P, flags and
    the table (keys, states), untouched (True when every summary word behind entry P, and the guard slot behind the last entry, still holds
    the poison), state (the kernel's final state; for ranges: the slots composed in file order from 0 by rsqc_rl_compose.h)."""
    lib = C.CDLL(build_k1(coarse))
    lib.k1emu_run_kr.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    a, b = ann.to_struct(), batch.to_struct()
    entries = len(batch.seg_tid) if ranges else 1
    tile_span = np.zeros(max((batch.n + 63) // 64, 1), np.uint32); extremes = np.zeros(3 * max(entries, 1), np.uint32)
    summary = np.full((entries + 1) * RL_SUMMARY_WORDS, RL_POISON, np.uint32); info = np.zeros(2, np.int32)
    o = Out()
    o.rc = lib.k1emu_run_kr(C.addressof(params), C.addressof(a), C.addressof(b), int(grid), int(r_in), 1 if ranges else 0, tile_span.ctypes.data,
                            extremes.ctypes.data, summary.ctypes.data, info.ctypes.data)
    o.state, o.error = int(info[0]), int(info[1])
    o.tile_span = tile_span[:(batch.n + 63) // 64].astype(np.int64); o.extremes = extremes[:3 * entries].reshape(entries, 3).astype(np.int64)
    slots = summary.reshape(entries + 1, RL_SUMMARY_WORDS)
    o.P = [int(s[0]) for s in slots[:entries]]; o.flags = [int(s[1]) for s in slots[:entries]]
    o.tables = [([int(x) for x in s[2:2 + 2 * min(P, RL_MAXP):2]], [int(x) for x in s[3:3 + 2 * min(P, RL_MAXP):2].astype(np.int32)]) for s, P in zip(slots, o.P)]
    # what rsqc_last_error says of these slots (rsqc_rl_compose.h: rl_limit_message, the text rsqc_submit.cpp hands on); "": none is flagged
    lib.k1emu_rl_limit_message.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_char_p, C.c_uint32]
    lib.k1emu_rl_limit_message.restype = C.c_uint32
    fi = np.ascontiguousarray(batch.seg_file_index if ranges else [batch.file_index_base], np.uint64)
    nrec = np.ascontiguousarray(np.diff(batch.seg_start.astype(np.int64)) if ranges else [batch.n], np.uint64)
    buf = C.create_string_buffer(1024)
    lib.k1emu_rl_limit_message(summary.ctypes.data, entries, fi.ctypes.data, nrec.ctypes.data, buf, 1024)
    o.message = buf.value.decode()
    o.untouched = bool((slots[entries] == RL_POISON).all()) and all(bool((s[2 + 2 * min(P, RL_MAXP):] == RL_POISON).all()) for s, P in zip(slots, o.P))
    return o


def rl_compose(items):
    """rsqc_rl_compose.h, the loop rsqc_finalize.cpp and the command line's shard merge run: items = [(file index, keys, states)], any order."""
    lib = C.CDLL(build_k1(True))
    lib.k1emu_rl_compose.argtypes = [C.c_void_p] * 4 + [C.c_uint32]
    lib.k1emu_rl_compose.restype = C.c_int32
    fi = np.array([t[0] for t in items] + [0], np.uint64)
    off = np.concatenate([[0], np.cumsum([len(t[1]) for t in items])]).astype(np.uint32)
    span = np.array([x for t in items for x in t[1]] + [0], np.uint32); state = np.array([x for t in items for x in t[2]] + [0], np.int32)
    return int(lib.k1emu_rl_compose(fi.ctypes.data, off.ctypes.data, span.ctypes.data, state.ctypes.data, len(items)))


def write_kr_case_file(path, params, ann, batch, grid=2, r_in=0, ranges=False):
    """the case file the stand-alone program reads (k1_emu.cpp: main): a header, then length-prefixed arrays in the order of the structs"""
    ann.to_struct(); batch.to_struct()                          # (leave the contiguous arrays of the boundary on the objects)
    blobs = [bytes(params), np.array([ann.n_ref, ann.n_contigs, ann.n_genes, ann.n_genes_listed, ann.n_exons], np.int32).tobytes()]
    for f in ("gene_row_contig", "gene_row_start", "gene_row_end", "gene_row_flags", "gene_row_id", "exon_row_contig", "exon_row_start", "exon_row_end",
              "exon_row_flags", "exon_row_id", "exon_row_gene", "gene_is_globin", "gene_exon_off", "gene_exon_row", "gene_row_order", "exon_row_order"):
        v = getattr(ann, f)
        blobs.append(b"" if v is None else np.ascontiguousarray(v).tobytes())
    blobs.append(np.array([batch.n, batch.file_index_base, len(batch.cigar), len(batch.seg_tid), len(batch.wide_index)], np.uint64).tobytes())
    blobs += [batch._core.tobytes(), batch._aux.tobytes()]
    blobs += [getattr(batch, f).tobytes() for f in ("cigar", "seg_tid", "seg_start", "wide_index", "wide_nm", "wide_l_qseq", "wide_n_cigar")]
    blobs.append(b"" if batch.qhash2 is None else batch.qhash2.tobytes())
    blobs.append(b"" if batch.seg_file_index is None else batch.seg_file_index.tobytes())
    assert len(blobs) == 30
    with open(path, "wb") as f:
        f.write(np.array([grid, r_in, 1 if ranges else 0], np.uint64).tobytes())
        for bl in blobs:
            f.write(np.array([len(bl)], np.uint64).tobytes()); f.write(bl)
