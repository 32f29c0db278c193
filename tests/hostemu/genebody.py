"""TEST HARNESS: the kernel and the launch plan of --gene-body (rnaseqc_amd/csrc/rsqc_genebody.h) with the model check and the walk of
rsqc_genemodel.h on the 64-lane fiber emulation (see genebody_emu.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(os.path.dirname(_HERE))
_SO = os.path.join(_HERE, "libgenebodyemu.so")
PROGRAM_SOURCE = os.path.join(_HERE, "genebody_emu.cpp")
_lib = None


class ModelError(Exception):
    pass


def build():
    csrc = os.path.join(_ROOT, "rnaseqc_amd", "csrc")
    srcs = [PROGRAM_SOURCE, os.path.join(_HERE, "wavemu.h"), os.path.join(_HERE, "genemodel_emu.h"), os.path.join(csrc, "rsqc_genebody.h"), os.path.join(csrc, "rsqc_genemodel.h"),
            os.path.join(_ROOT, "include", "rnaseqc_amd.h")]
    if not os.path.exists(_SO) or any(os.path.getmtime(_SO) < os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-fvisibility=hidden", "-Wno-unused-function", "-Wno-unused-variable", srcs[0], "-o", _SO])
    return _SO


def _load():
    global _lib
    if _lib is None:
        lib = C.CDLL(build())
        vp = C.c_void_p
        lib.gbemu_set_schedule_seed.argtypes = [C.c_ulonglong]
        lib.gbemu_run.argtypes = [C.c_int32, vp, vp, C.c_int32] + [vp] * 6
        lib.gbemu_plan.argtypes = [C.c_int32] + [vp] * 5
        lib.gbemu_error.restype = C.c_char_p
        lib.gbemu_sums.argtypes = [vp]
        lib.gbemu_items.argtypes = [vp]
        _lib = lib
    return _lib


def _columns(lengths, depth, model):
    lens = np.array([int(x) for x in lengths], np.uint64)
    flat = (np.concatenate([np.asarray(d) for d in depth]) if len(depth) else np.zeros(0)).astype(np.uint32)
    assert len(flat) == int(lens.sum())
    cols = [np.ascontiguousarray(model["seg_off"], np.uint32), np.ascontiguousarray(model["seg_tid"], np.int32), np.ascontiguousarray(model["seg_start"], np.uint32),
            np.ascontiguousarray(model["seg_end"], np.uint32), np.ascontiguousarray(model["reverse"], np.uint8)]
    return lens, flat, cols


def run(lengths, depth, model, seed=0):
    """The stage over `depth` (one array per contig).  Returns (sums [n_genes, 100], info with items and workgroups, the plan's items
    [n, 6]: gene, u0, u1, seg, seg_u, L | reverse << 31); ModelError when the model breaks a rule."""
    lib = _load()
    lens, flat, cols = _columns(lengths, depth, model)
    n_genes = len(cols[4])
    stats = np.zeros(6, np.uint64)
    lib.gbemu_set_schedule_seed(int(seed))
    try:
        rc = lib.gbemu_run(len(lens), lens.ctypes.data, flat.ctypes.data, n_genes, *[c.ctypes.data for c in cols], stats.ctypes.data)
    finally:
        lib.gbemu_set_schedule_seed(0)
    if rc == 1:
        raise ModelError(lib.gbemu_error().decode())
    assert rc == 0, "check %d of the harness" % rc
    sums = np.zeros(max(n_genes * 100, 1), np.uint64)
    lib.gbemu_sums(sums.ctypes.data)
    items = np.zeros((max(int(stats[4]), 1), 6), np.uint32)
    lib.gbemu_items(items.ctypes.data)
    info = dict(n_genes=int(stats[0]), n_measured=int(stats[1]), model_bases=int(stats[2]), depth_sum=int(stats[3]), items=int(stats[4]), workgroups=int(stats[5]))
    return sums[:n_genes * 100].reshape(n_genes, 100), info, items[:int(stats[4])]


def plan(model):
    """The launch plan alone of a model that keeps the rules: (info, items)."""
    lib = _load()
    cols = [np.ascontiguousarray(model[f], np.uint32) for f in ("seg_off", "seg_start", "seg_end")] + [np.ascontiguousarray(model["reverse"], np.uint8)]
    stats = np.zeros(6, np.uint64)
    lib.gbemu_plan(len(cols[3]), *[c.ctypes.data for c in cols], stats.ctypes.data)
    items = np.zeros((max(int(stats[4]), 1), 6), np.uint32)
    lib.gbemu_items(items.ctypes.data)
    info = dict(n_genes=int(stats[0]), n_measured=int(stats[1]), model_bases=int(stats[2]), depth_sum=0, items=int(stats[4]), workgroups=int(stats[5]))
    return info, items[:int(stats[4])]


def write_case_file(path, lengths, depth, model, seed):
    lens, flat, cols = _columns(lengths, depth, model)
    with open(path, "wb") as f:
        f.write(np.array([len(lens), len(cols[4]), len(cols[1]), seed], np.uint64).tobytes())
        for a in [lens, flat] + cols:
            f.write(a.tobytes())
