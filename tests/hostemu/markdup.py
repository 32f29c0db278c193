"""TEST HARNESS: the kernels of --mark-duplicates (rnaseqc_amd/csrc/rsqc_markdup.h) with the collecting kernel, radix passes and scan
of rsqc_sort.h on the 64-lane fiber emulation (see markdup_emu.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(os.path.dirname(_HERE))
_SO = os.path.join(_HERE, "libmarkdupemu.so")


def build():
    srcs = [os.path.join(_HERE, "markdup_emu.cpp"), os.path.join(_HERE, "wavemu.h"), os.path.join(_ROOT, "rnaseqc_amd", "csrc", "rsqc_markdup.h"),
            os.path.join(_ROOT, "rnaseqc_amd", "csrc", "rsqc_sort.h"), os.path.join(_ROOT, "include", "rnaseqc_amd.h")]
    if not os.path.exists(_SO) or any(os.path.getmtime(_SO) < os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-fvisibility=hidden", "-Wno-unused-function",
                               "-Wno-unused-variable", srcs[0], "-o", _SO])
    return _SO


def run(batches, seed=0):
    """Collect every batch, run the stage.  Returns a dict: verdict (uint8 per record in arrival order), flag (uint16, what the records
    leave with), the figures of rsqc_markdup_info, passes (stage 1, stage 2) and table_slots."""
    lib = C.CDLL(build())
    vp = C.c_void_p
    lib.mdemu_set_schedule_seed.argtypes = [C.c_ulonglong]
    lib.mdemu_add_batch.argtypes = [vp, vp, vp, C.c_uint64, vp, C.c_uint64, vp, vp, C.c_uint32, vp, vp, vp, vp, C.c_uint32]
    lib.mdemu_end.argtypes = [vp]
    lib.mdemu_rows.argtypes = [vp, vp]
    lib.mdemu_set_schedule_seed(int(seed))
    try:
        lib.mdemu_begin()
        for b in batches:
            s = b.to_struct()
            rc = lib.mdemu_add_batch(s.core, s.aux, s.qhash2, s.n, s.cigar, s.n_cigar_total, s.seg_tid, s.seg_start, s.n_seg, s.wide_index, s.wide_nm, s.wide_l_qseq, s.wide_n_cigar, s.n_wide)
            assert rc == 0, "batches with and without qhash2 in one pass"
        stats = np.zeros(10, np.uint64)
        rc = lib.mdemu_end(stats.ctypes.data)
        assert rc == 0, rc
    finally:
        lib.mdemu_set_schedule_seed(0)
    n = int(stats[0])
    verdict, flag = np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.uint16)
    lib.mdemu_rows(verdict.ctypes.data, flag.ctypes.data)
    out = dict(verdict=verdict[:n].copy(), flag=flag[:n].copy(), passes=(int(stats[7]), int(stats[8])), table_slots=int(stats[9]))
    for k, f in enumerate(("records", "population", "anchors", "sets", "duplicate_fragments", "flagged_records", "cleared_records")):
        out[f] = int(stats[k])
    return out
