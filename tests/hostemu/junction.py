"""TEST HARNESS: the kernels of --junctions (rnaseqc_amd/csrc/rsqc_junction.h) and the radix passes they are ordered with
(rsqc_sort.h) on the 64-lane fiber emulation (see junction_emu.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(os.path.dirname(_HERE))
_SO = os.path.join(_HERE, "libjunctionemu.so")

ERR_CAPACITY = -4


def build():
    srcs = [os.path.join(_HERE, "junction_emu.cpp"), os.path.join(_HERE, "wavemu.h"), os.path.join(_ROOT, "rnaseqc_amd", "csrc", "rsqc_junction.h"),
            os.path.join(_ROOT, "rnaseqc_amd", "csrc", "rsqc_sort.h"), os.path.join(_ROOT, "include", "rnaseqc_amd.h")]
    if not os.path.exists(_SO) or any(os.path.getmtime(_SO) < os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-fvisibility=hidden", "-Wno-unused-function",
                               "-Wno-unused-variable", srcs[0], "-o", _SO])
    return _SO


def run(batches, n_contigs, mapq_threshold=255, cap0=65536, seed=0):
    """Extract every batch, order and reduce.  Returns a dict: the table's columns, n, instances, population, error (0 or the
    device error flag), passes (stage 1, stage 2), grown (growth steps of the collection), cap."""
    lib = C.CDLL(build())
    vp = C.c_void_p
    lib.juncemu_set_schedule_seed.argtypes = [C.c_ulonglong]
    lib.juncemu_begin.argtypes = [C.c_uint64, C.c_int32, C.c_uint32]
    lib.juncemu_add_batch.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint64, vp, vp, C.c_uint32, vp, vp, C.c_uint32]
    lib.juncemu_end.argtypes = [vp]
    lib.juncemu_rows.argtypes = [vp] * 6
    lib.juncemu_set_schedule_seed(int(seed))
    try:
        lib.juncemu_begin(cap0, n_contigs, mapq_threshold)
        for b in batches:
            s = b.to_struct()
            rc = lib.juncemu_add_batch(s.core, s.aux, s.n, s.cigar, s.n_cigar_total, s.seg_tid, s.seg_start, s.n_seg, s.wide_index, s.wide_n_cigar, s.n_wide)
            assert rc == 0, "a write past the collection"
        stats = np.zeros(8, np.uint64)
        rc = lib.juncemu_end(stats.ctypes.data)
        assert rc == 0, rc
    finally:
        lib.juncemu_set_schedule_seed(0)
    n = int(stats[0])
    cols = [np.zeros(max(n, 1), np.int32) for _ in range(3)] + [np.zeros(max(n, 1), np.uint32) for _ in range(3)]
    lib.juncemu_rows(*[c.ctypes.data for c in cols])
    out = {f: c[:n].copy() for f, c in zip(("tid", "start", "end", "reads", "hq_reads", "max_overhang"), cols)}
    out.update(n=n, instances=int(stats[1]), population=int(stats[2]), error=int(stats[3].astype(np.int64)), passes=(int(stats[4]), int(stats[5])),
               grown=int(stats[6]), cap=int(stats[7]))
    return out
