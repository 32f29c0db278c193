"""TEST HARNESS: the kernel body of --alleles (rnaseqc_amd/csrc/rsqc_allele.h) on the 64-lane fiber emulation (see allele_emu.cpp), window
by window into one table, the one-thread form over the same bytes, and the stand-alone sanitizer program over damaged records and site
tables (allele_fuzz.cpp)."""
import ctypes as C

import numpy as np

from . import window_stage

COLS, STRIDE, SCALARS = 7, 8, 16
S_OFF_CONTIG, S_LOW_MAPQ, S_NO_SEQ, S_INCONSISTENT, S_RECORDS, S_NO_QUAL, S_HIT, S_OBS = range(1, 9)


def build_fuzz(exe):
    return window_stage.build_fuzz("allele", exe)


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(window_stage.build("allele", ("rsqc_allele.h", "rsqc_mismatch.h")))
        vp = C.c_void_p
        _lib.alemu_set_schedule_seed.argtypes = [C.c_ulonglong]
        _lib.alemu_set_merge.argtypes = [C.c_int]
        _lib.alemu_set_sites.argtypes = [C.c_int32, C.c_uint32, vp, vp]
        _lib.alemu_set_names.argtypes = [C.c_int32, C.POINTER(C.c_char_p)]
        _lib.alemu_bam.restype = C.c_longlong
        _lib.alemu_bam.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp]
        _lib.alemu_sam.restype = C.c_longlong
        _lib.alemu_sam.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp]
        _lib.alemu_host_bam.restype = C.c_longlong
        _lib.alemu_host_bam.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, C.c_uint32, vp, vp]
        _lib.alemu_host_sam.restype = C.c_longlong
        _lib.alemu_host_sam.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, C.c_uint32, vp, vp]
    return _lib


_n_sites = 0


def site_arrays(n_contigs, sites):
    """(tid, pos, first) of a site list, as the stage holds them."""
    tid = np.array([s[0] for s in sites], np.int32)
    pos = np.array([s[1] for s in sites], np.int32)
    first = np.zeros(n_contigs + 1, np.uint32)
    for t in tid:
        first[t + 1] += 1
    return tid, pos, np.cumsum(first, dtype=np.uint64).astype(np.uint32)


def set_sites(n_contigs, sites, names):
    """sites: [(tid, pos)] strictly ascending; names: the @SQ names of the stream, in order."""
    global _n_sites
    l = lib()
    _, pos, first = site_arrays(n_contigs, sites)
    l.alemu_set_sites(n_contigs, len(sites), pos.ctypes.data, first.ctypes.data)
    l.alemu_set_names(len(names), (C.c_char_p * max(len(names), 1))(*[s.encode() for s in names]))
    _n_sites = len(sites)


def set_merge(on):
    """Which form of allele_block the launches run: an atomic per observation, or merged across the wave first."""
    lib().alemu_set_merge(1 if on else 0)


class Table:
    def __init__(self, stride):
        self.cells = np.zeros((_n_sites, stride), np.uint64)
        self.scal = np.zeros(SCALARS, np.uint64)
        self.records = 0

    @property
    def counts(self):
        return self.cells[:, :COLS]

    def info(self):
        s = [int(v) for v in self.scal]
        return dict(seen_records=self.records, records=s[S_RECORDS], off_contig_records=s[S_OFF_CONTIG], low_mapq_records=s[S_LOW_MAPQ], no_seq_records=s[S_NO_SEQ],
                    inconsistent_records=s[S_INCONSISTENT], no_qual_records=s[S_NO_QUAL], hit_records=s[S_HIT], observations=s[S_OBS], n_sites=_n_sites)


def _run(call, windows, seed):
    t, l = Table(STRIDE), lib()
    window_stage.run_windows(l.alemu_set_schedule_seed, seed, t, windows, lambda w: call(l, t, w))
    assert not t.cells[:, COLS:].any()                              # (the eighth cell of a line is never touched)
    return t


def run_bam(windows, min_mapq=0, min_baseq=0, front=0, n_blocks=1, seed=0):
    """windows: byte strings of complete BAM records; every one is a launch of n_blocks workgroups into the same table."""
    return _run(lambda l, t, w: l.alemu_bam(w, len(w), front, n_blocks, min_mapq, min_baseq, t.scal.ctypes.data, t.cells.ctypes.data), windows, seed)


def run_sam(windows, min_mapq=0, min_baseq=0, front=0, n_blocks=1, seed=0):
    """windows: texts of complete lines; the first may start with header lines."""
    return _run(lambda l, t, w: l.alemu_sam(w, len(w), front, 1 if t.records else 0, n_blocks, min_mapq, min_baseq, t.scal.ctypes.data, t.cells.ctypes.data), windows, seed)


def run_host(stream, min_mapq=0, min_baseq=0, sam=False):
    t = Table(COLS)
    n = (lib().alemu_host_sam if sam else lib().alemu_host_bam)(stream, len(stream), min_mapq, min_baseq, t.scal.ctypes.data, t.cells.ctypes.data)
    assert n >= 0
    t.records = n
    return t
