"""TEST HARNESS: the stage of --mark-duplicates with UMIs one substitution apart grouped (rsqc_markdup_umi_edits(1);
rnaseqc_amd/csrc/rsqc_markdup.h with rsqc_sort.h's passes) on the 64-lane fiber emulation (see markdup_umi_group_emu.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(os.path.dirname(_HERE))
_SO = os.path.join(_HERE, "libmarkdupumigroupemu.so")


def build():
    srcs = [os.path.join(_HERE, "markdup_umi_group_emu.cpp"), os.path.join(_HERE, "wavemu.h"), os.path.join(_ROOT, "rnaseqc_amd", "csrc", "rsqc_markdup.h"),
            os.path.join(_ROOT, "rnaseqc_amd", "csrc", "rsqc_sort.h"), os.path.join(_ROOT, "include", "rnaseqc_amd.h")]
    if not os.path.exists(_SO) or any(os.path.getmtime(_SO) < os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-fvisibility=hidden", "-Wno-unused-function",
                               "-Wno-unused-variable", srcs[0], "-o", _SO])
    return _SO


STATS = ("records", "population", "anchors", "sets", "duplicate_fragments", "flagged_records", "cleared_records", "anchors_with_umi",
         "position_duplicate_fragments", "table_slots", "umi_nodes", "merged_nodes", "exact_duplicate_fragments", "probes", "position_sets")
NO_ANCHOR = (1 << 64) - 1


def run(batches, seed=0, smallest_key_parent=False):
    """Collect every batch (each with its umi column), run the stage.  Returns a dict: verdict (uint8 per record in arrival order), flag
    (uint16, what the records leave with), roots (arrival index of an anchor -> the root key of its UMI) and the entries of STATS +
    anchors_without_umi.  smallest_key_parent: the harness's WRONG parent rule, for showing that a catalogue tells it from the right
    one."""
    lib = C.CDLL(build())
    vp = C.c_void_p
    lib.mdgemu_set_schedule_seed.argtypes = [C.c_ulonglong]
    lib.mdgemu_add_batch.argtypes = [vp, vp, vp, vp, C.c_uint64, vp, C.c_uint64, vp, vp, C.c_uint32, vp, vp, vp, vp, C.c_uint32]
    lib.mdgemu_end.argtypes = [vp, C.c_int]
    lib.mdgemu_rows.argtypes = [vp, vp, vp]
    lib.mdgemu_set_schedule_seed(int(seed))
    try:
        lib.mdgemu_begin()
        for b in batches:
            s = b.to_struct()
            rc = lib.mdgemu_add_batch(s.core, s.aux, s.qhash2, s.umi, s.n, s.cigar, s.n_cigar_total, s.seg_tid, s.seg_start, s.n_seg, s.wide_index, s.wide_nm, s.wide_l_qseq,
                                      s.wide_n_cigar, s.n_wide)
            assert rc == 0, rc
        stats = np.zeros(len(STATS), np.uint64)
        rc = lib.mdgemu_end(stats.ctypes.data, 1 if smallest_key_parent else 0)
        assert rc == 0, rc
    finally:
        lib.mdgemu_set_schedule_seed(0)
    n = int(stats[0])
    verdict, flag, root = np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.uint16), np.zeros(max(n, 1), np.uint64)
    lib.mdgemu_rows(verdict.ctypes.data, flag.ctypes.data, root.ctypes.data)
    out = dict(verdict=verdict[:n].copy(), flag=flag[:n].copy(), roots={i: int(r) for i, r in enumerate(root[:n]) if int(r) != NO_ANCHOR})
    for k, f in enumerate(STATS):
        out[f] = int(stats[k])
    out["anchors_without_umi"] = out["anchors"] - out["anchors_with_umi"]
    return out
