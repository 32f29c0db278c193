"""TEST HARNESS: the kernels and the launch plan of --tin (rnaseqc_amd/csrc/rsqc_tin.h) with the model check and the walk of
rsqc_genemodel.h on the 64-lane fiber emulation (see tin_emu.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np

from tests import tin_ref as ref

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(os.path.dirname(_HERE))
_SO = os.path.join(_HERE, "libtinemu.so")
PROGRAM_SOURCE = os.path.join(_HERE, "tin_emu.cpp")
_lib = None


class ModelError(Exception):
    pass


def build():
    csrc = os.path.join(_ROOT, "rnaseqc_amd", "csrc")
    srcs = [PROGRAM_SOURCE, os.path.join(_HERE, "wavemu.h"), os.path.join(_HERE, "genemodel_emu.h"), os.path.join(csrc, "rsqc_tin.h"), os.path.join(csrc, "rsqc_genemodel.h"),
            os.path.join(_ROOT, "include", "rnaseqc_amd.h")]
    if not os.path.exists(_SO) or any(os.path.getmtime(_SO) < os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-fvisibility=hidden", "-Wno-unused-function", "-Wno-unused-variable", srcs[0], "-o", _SO])
    return _SO


def _load():
    global _lib
    if _lib is None:
        lib = C.CDLL(build())
        vp = C.c_void_p
        lib.tinemu_set_schedule_seed.argtypes = [C.c_ulonglong]
        lib.tinemu_run.argtypes = [C.c_int32, vp, vp, C.c_int32] + [vp] * 5
        lib.tinemu_plan.argtypes = [C.c_int32] + [vp] * 4
        lib.tinemu_error.restype = C.c_char_p
        lib.tinemu_rows.argtypes = [vp]
        lib.tinemu_items.argtypes = [vp]
        lib.tinemu_item_off.argtypes = [vp]
        _lib = lib
    return _lib


def _columns(lengths, depth, model):
    lens = np.array([int(x) for x in lengths], np.uint64)
    flat = (np.concatenate([np.asarray(d) for d in depth]) if len(depth) else np.zeros(0)).astype(np.uint32)
    assert len(flat) == int(lens.sum())
    cols = [np.ascontiguousarray(model["seg_off"], np.uint32), np.ascontiguousarray(model["seg_tid"], np.int32), np.ascontiguousarray(model["seg_start"], np.uint32),
            np.ascontiguousarray(model["seg_end"], np.uint32)]
    return lens, flat, cols


def _plan_out(lib, stats, n_genes):
    items = np.zeros((max(int(stats[3]), 1), 5), np.uint32)
    lib.tinemu_items(items.ctypes.data)
    item_off = np.zeros(n_genes + 1, np.uint64)
    lib.tinemu_item_off(item_off.ctypes.data)
    info = dict(n_genes=int(stats[0]), n_measured=int(stats[1]), model_bases=int(stats[2]), items=int(stats[3]), workgroups=int(stats[4]))
    return info, items[:int(stats[3])], item_off


def run(lengths, depth, model, seed=0):
    """The stage over `depth` (one array per contig).  Returns (rows [n_genes] of ref.ROW, info with items and workgroups -- depth_sum
    and covered_bases added from the rows, as the library's host side does --, the plan's items [n, 5]: gene, u0, u1, seg, seg_u, and
    item_off [n_genes + 1]); ModelError when the model breaks a rule."""
    lib = _load()
    lens, flat, cols = _columns(lengths, depth, model)
    n_genes = len(cols[0]) - 1
    stats = np.zeros(5, np.uint64)
    lib.tinemu_set_schedule_seed(int(seed))
    try:
        rc = lib.tinemu_run(len(lens), lens.ctypes.data, flat.ctypes.data, n_genes, *[c.ctypes.data for c in cols], stats.ctypes.data)
    finally:
        lib.tinemu_set_schedule_seed(0)
    if rc == 1:
        raise ModelError(lib.tinemu_error().decode())
    assert rc == 0
    rows = np.zeros(max(n_genes, 1), ref.ROW)
    lib.tinemu_rows(rows.ctypes.data)
    rows = rows[:n_genes]
    info, items, item_off = _plan_out(lib, stats, n_genes)
    info.update(depth_sum=int(rows["depth_sum"].sum(dtype=np.uint64)), covered_bases=int(rows["covered"].sum(dtype=np.uint64)))
    return rows, info, items, item_off


def plan(model):
    """The launch plan alone of a model that keeps the rules: (info, items, item_off)."""
    lib = _load()
    cols = [np.ascontiguousarray(model[f], np.uint32) for f in ("seg_off", "seg_start", "seg_end")]
    stats = np.zeros(5, np.uint64)
    n_genes = len(cols[0]) - 1
    lib.tinemu_plan(n_genes, *[c.ctypes.data for c in cols], stats.ctypes.data)
    return _plan_out(lib, stats, n_genes)


def write_case_file(path, lengths, depth, model, seed):
    lens, flat, cols = _columns(lengths, depth, model)
    with open(path, "wb") as f:
        f.write(np.array([len(lens), len(cols[0]) - 1, len(cols[1]), seed], np.uint64).tobytes())
        for a in [lens, flat] + cols:
            f.write(a.tobytes())
