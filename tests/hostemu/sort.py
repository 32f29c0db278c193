"""TEST HARNESS: the kernels of --sort (rnaseqc_amd/csrc/rsqc_sort.h) on the 64-lane fiber emulation (see sort_emu.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(os.path.dirname(_HERE))
_SO = os.path.join(_HERE, "libsortemu.so")

THREADS, ROUNDS = 256, 8
TILE = THREADS * ROUNDS                 # RSQC_SORT_TILE: the keys of one scatter workgroup


def build():
    srcs = [os.path.join(_HERE, "sort_emu.cpp"), os.path.join(_HERE, "wavemu.h"), os.path.join(_ROOT, "rnaseqc_amd", "csrc", "rsqc_sort.h"),
            os.path.join(_ROOT, "include", "rnaseqc_amd.h")]
    if not os.path.exists(_SO) or any(os.path.getmtime(_SO) < os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-fvisibility=hidden", "-Wno-unused-function",
                               "-Wno-unused-variable", srcs[0], "-o", _SO])
    return _SO


def make_keys(tid, pos):
    """The order of --sort: tid as unsigned 32 bits, then pos as signed (sort_key, rsqc_sort.h)."""
    tid = np.asarray(tid, np.int64).astype(np.int32).view(np.uint32).astype(np.uint64)
    pos = (np.asarray(pos, np.int64).astype(np.int32).view(np.uint32) ^ np.uint32(0x80000000)).astype(np.uint64)
    return (tid << np.uint64(32)) | pos


def run_sort(keys, prep_grid=3, seed=0):
    """Returns (rc, permutation, passes run or -1 for input in order, OR of the keys, AND of the keys); rc 0 = the permutation is
    std::stable_sort's."""
    lib = C.CDLL(build())
    keys = np.ascontiguousarray(keys, np.uint64)
    perm = np.zeros(max(len(keys), 1), np.uint32); stats = np.zeros(3, np.uint64)
    lib.sortemu_set_schedule_seed.argtypes = [C.c_ulonglong]
    lib.sortemu_sort.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p]
    lib.sortemu_set_schedule_seed(int(seed))
    try:
        rc = lib.sortemu_sort(keys.ctypes.data, len(keys), prep_grid, perm.ctypes.data, stats.ctypes.data)
    finally:
        lib.sortemu_set_schedule_seed(0)
    return rc, perm[:len(keys)].copy(), int(stats[0].astype(np.int64)), int(stats[1]), int(stats[2])


def run_keys(pos, seg_tid, seg_start):
    """sort_append_kernel's keys of one batch."""
    lib = C.CDLL(build())
    pos = np.ascontiguousarray(pos, np.int32); seg_tid = np.ascontiguousarray(seg_tid, np.int32); seg_start = np.ascontiguousarray(seg_start, np.uint64)
    out = np.zeros(max(len(pos), 1), np.uint64)
    lib.sortemu_keys.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    lib.sortemu_keys(pos.ctypes.data, len(pos), seg_tid.ctypes.data, seg_start.ctypes.data, len(seg_tid), out.ctypes.data)
    return out[:len(pos)].copy()


def run_gather(seed, n, n_in, out_batch, in_order=False):
    """Collect, sort and gather `n` seeded records (sort_emu.cpp, sortemu_gather).  Returns (rc, output batches, moved, passes)."""
    lib = C.CDLL(build())
    stats = np.zeros(3, np.uint64)
    lib.sortemu_gather.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p]
    rc = lib.sortemu_gather(seed, n, n_in, out_batch, 1 if in_order else 0, stats.ctypes.data)
    return rc, int(stats[0]), int(stats[1]), int(stats[2].astype(np.int64))
