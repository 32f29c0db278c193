"""TEST HARNESS: the kernels of --fasta (rnaseqc_amd/csrc/rsqc_gc.h, the G/C helpers of rsqc_device.h, the pairing and the GC replay
of rsqc_k5.h) on the 64-lane fiber emulation (see gc_emu.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np

from rnaseqc_amd import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(os.path.dirname(_HERE))
_SO = os.path.join(_HERE, "libgcemu.so")
_HEADERS = ("rsqc_gc.h", "rsqc_k5.h", "rsqc_k5_plan.h", "rsqc_device.h", "rsqc_read.h", "rsqc_index.h", "rsqc_wave.h", "rsqc_k1s.h")

GC_BINS = 100
CAND_COLUMNS = ("file_index", "qhash", "h2", "row", "endpos", "flag_lq", "tid")
_CAND_DTYPES = (np.uint64, np.uint64, np.uint32, np.uint32, np.int32, np.uint32, np.int32)


def sources():
    csrc = os.path.join(_ROOT, "rnaseqc_amd", "csrc")
    return [os.path.join(_HERE, "gc_emu.cpp"), os.path.join(_HERE, "wavemu.h")] + [os.path.join(csrc, f) for f in _HEADERS] + \
           [os.path.join(_ROOT, "include", "rnaseqc_amd.h")]


def build():
    srcs = sources()
    if not os.path.exists(_SO) or any(os.path.getmtime(_SO) < os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-fvisibility=hidden", "-Wno-unused-function",
                               "-Wno-unused-variable", srcs[0], "-o", _SO])
    return _SO


def _lib():
    lib = C.CDLL(build())
    vp = C.c_void_p
    lib.gcemu_set_schedule_seed.argtypes = [C.c_ulonglong]
    lib.gcemu_reference_words.argtypes = [vp]
    lib.gcemu_reference_words.restype = C.c_uint64
    lib.gcemu_reference.argtypes = [vp] * 6
    lib.gcemu_run.argtypes = [vp, vp, vp, C.c_int, C.c_uint32] + [vp] * 9
    lib.gcemu_candidates.argtypes = [vp] * 7
    return lib


def _reference(lib, ann, reference):
    a, r = ann.to_struct(), reference.to_struct()
    n_words = int(lib.gcemu_reference_words(C.addressof(r)))
    words = np.zeros(max(n_words, 1), np.uint64)
    off = np.zeros(max(ann.n_contigs, 1), np.uint64); length = np.zeros(max(ann.n_contigs, 1), np.uint64)
    exon_gc = np.zeros(max(ann.n_exons, 1), np.float64)
    rc = lib.gcemu_reference(C.addressof(a), C.addressof(r), words.ctypes.data, off.ctypes.data, length.ctypes.data, exon_gc.ctypes.data)
    assert rc == 0, "gcemu_reference rc=%d" % rc
    return dict(words=words[:n_words], word_off=off[:ann.n_contigs], length=length[:ann.n_contigs], exon_gc=exon_gc[:ann.n_exons])


def reference(ann, reference, seed=0):
    """rsqc_set_reference under the emulation: dict(words, word_off, length, exon_gc by exon id)."""
    lib = _lib()
    lib.gcemu_set_schedule_seed(int(seed))
    try:
        return _reference(lib, ann, reference)
    finally:
        lib.gcemu_set_schedule_seed(0)


def run(ann, reference, batches=None, candidates=None, params=None, seed=0):
    """The whole chain.  batches: a list of model.Batch (the candidates kernel runs per batch); or candidates: a dict of the columns
    CAND_COLUMNS, handed to the pairing as they are.  Returns a dict: bins (100), out_of_range, exon_gc, words / word_off / length,
    candidates (dict of columns, list order), n_candidates, hashed / sorted / oversize (buckets by pairing path), buckets, error."""
    lib = _lib()
    params = params if params is not None else abi.default_params()
    lib.gcemu_set_schedule_seed(int(seed))
    try:
        out = _reference(lib, ann, reference)
        a = ann.to_struct()
        bins = np.zeros(GC_BINS + 1, np.uint64); stats = np.zeros(6, np.uint64)
        if candidates is None:
            structs = [b.to_struct() for b in batches]
            ptrs = (C.c_void_p * max(len(structs), 1))(*[C.addressof(s) for s in structs])
            rc = lib.gcemu_run(C.addressof(params), C.addressof(a), ptrs, len(structs), 0, *([None] * 7), bins.ctypes.data, stats.ctypes.data)
        else:
            cols = [np.ascontiguousarray(candidates[f], dt) for f, dt in zip(CAND_COLUMNS, _CAND_DTYPES)]
            n = len(cols[0])
            assert all(len(c) == n for c in cols)
            rc = lib.gcemu_run(C.addressof(params), C.addressof(a), None, 0, n, *[c.ctypes.data for c in cols], bins.ctypes.data, stats.ctypes.data)
        assert rc == 0, "gcemu_run rc=%d" % rc
        n = int(stats[0])
        got = [np.zeros(max(n, 1), dt) for dt in _CAND_DTYPES]
        lib.gcemu_candidates(*[g.ctypes.data for g in got])
    finally:
        lib.gcemu_set_schedule_seed(0)
    out.update(bins=bins[:GC_BINS].copy(), out_of_range=int(bins[GC_BINS]), n_candidates=n,
               candidates={f: g[:n].copy() for f, g in zip(CAND_COLUMNS, got)},
               hashed=int(stats[1]), sorted=int(stats[2]), oversize=int(stats[3]), error=int(stats[4].astype(np.int64)), buckets=int(stats[5]))
    return out
