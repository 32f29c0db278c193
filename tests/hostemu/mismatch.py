"""TEST HARNESS: the kernel body of --mismatches (rnaseqc_amd/csrc/rsqc_mismatch.h) on the 64-lane fiber emulation (see mismatch_emu.cpp),
window by window into one set of tables, the one-thread form over the same bytes, and the stand-alone sanitizer program over damaged
records (mismatch_fuzz.cpp)."""
import ctypes as C

import numpy as np

from . import window_stage

CYC_SHAPE, SUBST_SHAPE, BYQ_SHAPE, SCALARS = (2, 512, 6), (2, 4, 4), (64, 2), 16
S_NO_REF, S_LOW_MAPQ, S_NO_SEQ, S_INCONSISTENT, S_RECORDS, S_NO_QUAL, S_BEYOND, S_CLAMPED, S_INS_EVENTS, S_DEL_EVENTS, S_DEL_BASES, S_LEN_SUM = range(1, 13)


def build_fuzz(exe):
    return window_stage.build_fuzz("mismatch", exe)


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(window_stage.build("mismatch", ("rsqc_mismatch.h",)))
        vp = C.c_void_p
        tabs = [vp, vp, vp, vp]
        _lib.mmemu_set_schedule_seed.argtypes = [C.c_ulonglong]
        _lib.mmemu_set_reference.argtypes = [C.c_int32, vp, C.POINTER(C.c_char_p)]
        _lib.mmemu_set_names.argtypes = [C.c_int32, C.POINTER(C.c_char_p)]
        _lib.mmemu_pack_codes.argtypes = [vp]
        _lib.mmemu_bam.restype = C.c_longlong
        _lib.mmemu_bam.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32] + tabs
        _lib.mmemu_sam.restype = C.c_longlong
        _lib.mmemu_sam.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32] + tabs
        _lib.mmemu_host_bam.restype = C.c_longlong
        _lib.mmemu_host_bam.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32] + tabs
        _lib.mmemu_host_sam.restype = C.c_longlong
        _lib.mmemu_host_sam.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32] + tabs
    return _lib


def set_reference(reference, names):
    """reference: [(name, length, text or None)]; names: the @SQ names of the stream, in order."""
    l = lib()
    n = len(reference)
    lengths = np.array([r[1] for r in reference], np.uint64)
    seqs = (C.c_char_p * max(n, 1))(*[None if r[2] is None else r[2].encode("latin-1") for r in reference])
    l.mmemu_set_reference(n, lengths.ctypes.data, seqs)
    l.mmemu_set_names(len(names), (C.c_char_p * max(len(names), 1))(*[s.encode() for s in names]))


def pack_codes():
    out = np.zeros(256, np.uint32)
    lib().mmemu_pack_codes(out.ctypes.data)
    return out


class Tables:
    def __init__(self):
        self.cyc, self.subst, self.byq = np.zeros(CYC_SHAPE, np.uint64), np.zeros(SUBST_SHAPE, np.uint64), np.zeros(BYQ_SHAPE, np.uint64)
        self.scal = np.zeros(SCALARS, np.uint64)
        self.records = 0

    def ptrs(self):
        return self.cyc.ctypes.data, self.subst.ctypes.data, self.byq.ctypes.data, self.scal.ctypes.data

    def info(self):
        """(the count fields of rsqc_mismatch_info, the device's sum of L)."""
        s = [int(v) for v in self.scal]
        col = [int(self.cyc[:, :, k].sum()) for k in range(6)]
        return dict(seen_records=self.records, records=s[S_RECORDS], no_reference_records=s[S_NO_REF], low_mapq_records=s[S_LOW_MAPQ], no_seq_records=s[S_NO_SEQ],
                    inconsistent_records=s[S_INCONSISTENT], no_qual_records=s[S_NO_QUAL], compared=col[0], mismatched=col[1], uncompared=col[2], inserted=col[3],
                    clipped=col[4], deletions=col[5], insertion_events=s[S_INS_EVENTS], deletion_events=s[S_DEL_EVENTS], deleted_bases=s[S_DEL_BASES],
                    beyond_bases=s[S_BEYOND], clamped_quals=s[S_CLAMPED]), s[S_LEN_SUM]


def run_bam(windows, min_mapq=0, front=0, n_blocks=1, seed=0):
    """windows: byte strings of complete BAM records; every one is a launch of n_blocks workgroups into the same tables."""
    t, l = Tables(), lib()
    return window_stage.run_windows(l.mmemu_set_schedule_seed, seed, t, windows, lambda w: l.mmemu_bam(w, len(w), front, n_blocks, min_mapq, *t.ptrs()))


def run_sam(windows, min_mapq=0, front=0, n_blocks=1, seed=0):
    """windows: texts of complete lines; the first may start with header lines."""
    t, l = Tables(), lib()
    return window_stage.run_windows(l.mmemu_set_schedule_seed, seed, t, windows, lambda w: l.mmemu_sam(w, len(w), front, 1 if t.records else 0, n_blocks, min_mapq, *t.ptrs()))


def run_host(stream, min_mapq=0, sam=False):
    t = Tables()
    n = (lib().mmemu_host_sam if sam else lib().mmemu_host_bam)(stream, len(stream), min_mapq, *t.ptrs())
    assert n >= 0
    t.records = n
    return t
