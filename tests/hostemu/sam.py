"""TEST HARNESS: the product's SAM text decode (rsqc_samrec.h / rsqc_sam.h) compiled for the host as a wave of one lane
(see sam_emu.cpp)."""
import ctypes as C
import gzip
import os
import struct
import subprocess

import numpy as np

from rnaseqc_amd import abi
from tests.hostemu.decode import tag_spec

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "libsam_emu.so")
_ROOT = os.path.dirname(os.path.dirname(_HERE))


def build(so=_SO, extra=()):
    csrc = os.path.join(_ROOT, "rnaseqc_amd", "csrc")
    srcs = [os.path.join(_HERE, "sam_emu.cpp")] + [os.path.join(csrc, h) for h in ("rsqc_samrec.h", "rsqc_sam.h", "rsqc_bamrec.h", "rsqc_decode.h")] + \
           [os.path.join(_ROOT, "include", "rnaseqc_amd.h")]
    if not os.path.exists(so) or any(os.path.getmtime(so) < os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-fvisibility=hidden", *extra, srcs[0], "-o", so])
    return so


_lib = None


def lib():
    global _lib
    if _lib is None:
        l = C.CDLL(build())
        l.emu_sam_begin.argtypes = [C.c_int32, C.POINTER(C.c_char_p), C.c_void_p, C.c_uint64]
        l.emu_sam_submit.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32]
        l.emu_sam_error.argtypes = [C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
        l.emu_sam_counts.argtypes = [C.c_void_p]
        l.emu_sam_fetch.argtypes = [C.c_void_p] * 10
        l.emu_sam_bad_name.restype = C.c_char_p
        l.emu_sam_parse_line.argtypes = [C.c_char_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32]
        l.emu_bam_parse_record.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p, C.c_uint32]
        _lib = l
    return _lib


FIELDS = ("code", "tid", "pos", "mpos", "isize", "flag", "mapq", "l_seq", "nm", "n_ops", "tagbits", "wide", "qname_len", "qhash2", "qhash_lo", "qhash_hi")


class SamError(Exception):
    def __init__(self, code, line):
        super().__init__("malformed SAM line %d (code %d)" % (line, code))
        self.code, self.line = code, line


def begin(names, ch_tag="ch", filter_tags=(), buf_bytes=0):
    """buf_bytes: the window buffer the C ABI would have (its capacities follow from it); 0 = each window's own size, the
    tightest the ABI's buffers ever are"""
    t = tag_spec(len(names), ch_tag, filter_tags)
    arr = (C.c_char_p * max(1, len(names)))(*[n.encode() for n in names])
    lib().emu_sam_begin(len(names), arr, C.byref(t), buf_bytes)
    return t


def submit(text, per_thread=32):
    rc = lib().emu_sam_submit(bytes(text), len(text), per_thread)
    if rc:
        line, code = C.c_uint64(), C.c_uint32()
        lib().emu_sam_error(C.byref(line), C.byref(code))
        raise SamError(code.value, line.value)


def end():
    rc = lib().emu_sam_end()
    if rc:
        line, code = C.c_uint64(), C.c_uint32()
        lib().emu_sam_error(C.byref(line), C.byref(code))
        raise SamError(code.value, line.value)


def result():
    """The stream's columns, in the layout of tests/test_gpu_decode.py's parts (one part: whole-stream numbering)."""
    cnt = np.zeros(8, np.uint64)
    lib().emu_sam_counts(cnt.ctypes.data)
    n, nops, nseg, nw = (int(x) for x in cnt[:4])
    p = dict(core=np.zeros(n, abi.REC_CORE), aux=np.zeros(n, abi.REC_AUX), qhash2=np.zeros(n, np.uint32), cigar=np.zeros(nops, np.uint32),
             seg_tid=np.zeros(nseg, np.int32), seg_start=np.zeros(nseg + 1, np.uint64), wide_index=np.zeros(nw, np.uint64),
             wide_nm=np.zeros(nw, np.int32), wide_lq=np.zeros(nw, np.int32), wide_nc=np.zeros(nw, np.uint32), base=0)
    lib().emu_sam_fetch(*[p[k].ctypes.data for k in ("core", "aux", "qhash2", "cigar", "seg_tid", "seg_start", "wide_index", "wide_nm", "wide_lq", "wide_nc")])
    p["seg_start"][-1] = n
    p["unsorted"], p["n_bad"], p["windows"], p["carry"] = bool(cnt[4]), int(cnt[5]), int(cnt[6]), int(cnt[7])
    p["bad_names"] = [lib().emu_sam_bad_name(k).decode() for k in range(min(p["n_bad"], 64))]
    return p


def parse_line(line, max_ops=1 << 20):
    out = np.zeros(16, np.int64)
    ops = np.zeros(max_ops, np.uint32)
    lib().emu_sam_parse_line(line, len(line), out.ctypes.data, ops.ctypes.data, max_ops)
    d = dict(zip(FIELDS, (int(x) for x in out)))
    d["ops"] = ops[:d["n_ops"]].copy() if d["code"] == 0 else None
    return d


def parse_bam_record(rec, max_ops=1 << 20):
    out = np.zeros(16, np.int64)
    ops = np.zeros(max_ops, np.uint32)
    lib().emu_bam_parse_record(rec, out.ctypes.data, ops.ctypes.data, max_ops)
    d = dict(zip(FIELDS, (int(x) for x in out)))
    d["ops"] = ops[:d["n_ops"]].copy()
    return d


def bam_records(path):
    """The raw records (block_size included) of a BAM file written by bamio.write_bam."""
    data = gzip.decompress(open(path, "rb").read())
    l_text = struct.unpack_from("<I", data, 4)[0]
    p = 8 + l_text
    n_ref = struct.unpack_from("<I", data, p)[0]
    p += 4
    for _ in range(n_ref):
        p += 8 + struct.unpack_from("<I", data, p)[0]
    out = []
    while p < len(data):
        bs = struct.unpack_from("<I", data, p)[0]
        out.append(data[p:p + 4 + bs])
        p += 4 + bs
    return out


def sam_lines(path):
    return [l for l in open(path, "rb").read().split(b"\n") if l and not l.startswith(b"@")]
