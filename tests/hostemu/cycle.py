"""TEST HARNESS: the kernel body of --cycles (rnaseqc_amd/csrc/rsqc_cycle.h) on the 64-lane fiber emulation (see cycle_emu.cpp), window by
window into one set of tables, and the stand-alone sanitizer program over damaged records (cycle_fuzz.cpp)."""
import ctypes as C

import numpy as np

from . import window_stage

BASE_SHAPE, QUAL_SHAPE, SCALARS = (2, 512, 5), (2, 512, 64), 8
S_RECORDS, S_NO_SEQ, S_NO_QUAL, S_BEYOND, S_CLAMPED, S_LEN_SUM = range(6)


def build_fuzz(exe):
    return window_stage.build_fuzz("cycle", exe)


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(window_stage.build("cycle"))
        vp = C.c_void_p
        _lib.cycemu_set_schedule_seed.argtypes = [C.c_ulonglong]
        _lib.cycemu_bam.restype = C.c_longlong
        _lib.cycemu_bam.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, C.c_uint32, vp, vp, vp]
        _lib.cycemu_sam.restype = C.c_longlong
        _lib.cycemu_sam.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, C.c_int, C.c_uint32, vp, vp, vp]
        _lib.cycemu_host_bam.restype = C.c_longlong
        _lib.cycemu_host_bam.argtypes = [C.c_char_p, C.c_uint64, vp, vp, vp]
    return _lib


class Tables:
    def __init__(self):
        self.base, self.qual, self.scal = np.zeros(BASE_SHAPE, np.uint64), np.zeros(QUAL_SHAPE, np.uint64), np.zeros(SCALARS, np.uint64)
        self.records = 0

    def ptrs(self):
        return self.base.ctypes.data, self.qual.ctypes.data, self.scal.ctypes.data

    def info(self):
        s = [int(v) for v in self.scal]
        return dict(seen_records=self.records, records=s[S_RECORDS], no_seq_records=s[S_NO_SEQ], no_qual_records=s[S_NO_QUAL], bases=int(self.base.sum()),
                    beyond_bases=s[S_BEYOND], clamped_quals=s[S_CLAMPED]), s[S_LEN_SUM]


def run_bam(windows, front=0, n_blocks=1, seed=0):
    """windows: byte strings of complete BAM records; every one is a launch (four tiles x n_blocks workgroups) into the same tables."""
    t, l = Tables(), lib()
    return window_stage.run_windows(l.cycemu_set_schedule_seed, seed, t, windows, lambda w: l.cycemu_bam(w, len(w), front, n_blocks, *t.ptrs()))


def run_sam(windows, front=0, n_blocks=1, seed=0):
    """windows: texts of complete lines; the first may start with header lines."""
    t, l = Tables(), lib()
    return window_stage.run_windows(l.cycemu_set_schedule_seed, seed, t, windows, lambda w: l.cycemu_sam(w, len(w), front, 1 if t.records else 0, n_blocks, *t.ptrs()))


def run_host_bam(stream):
    t = Tables()
    n = lib().cycemu_host_bam(stream, len(stream), *t.ptrs())
    assert n >= 0
    t.records = n
    return t
