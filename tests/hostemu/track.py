"""TEST HARNESS: the kernels of --bedgraph (rnaseqc_amd/csrc/rsqc_track.h) and the scan they use (rsqc_sort.h) on the 64-lane fiber
emulation (see track_emu.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(os.path.dirname(_HERE))
_SO = os.path.join(_HERE, "libtrackemu.so")
_lib = None


def build():
    srcs = [os.path.join(_HERE, "track_emu.cpp"), os.path.join(_HERE, "wavemu.h"), os.path.join(_ROOT, "rnaseqc_amd", "csrc", "rsqc_track.h"),
            os.path.join(_ROOT, "rnaseqc_amd", "csrc", "rsqc_sort.h"), os.path.join(_ROOT, "include", "rnaseqc_amd.h")]
    if not os.path.exists(_SO) or any(os.path.getmtime(_SO) < os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-fvisibility=hidden", "-Wno-unused-function",
                               "-Wno-unused-variable", srcs[0], "-o", _SO])
    return _SO


def _load():
    global _lib
    if _lib is None:
        lib = C.CDLL(build())
        vp = C.c_void_p
        lib.trackemu_set_schedule_seed.argtypes = [C.c_ulonglong]
        lib.trackemu_begin.argtypes = [C.c_int32, vp, C.c_char_p, vp, C.c_int]
        lib.trackemu_add_batch.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint64, vp, vp, C.c_uint32, vp, vp, C.c_uint32]
        lib.trackemu_end.argtypes = [vp]
        lib.trackemu_rows.argtypes = [vp] * 4
        lib.trackemu_text.argtypes = [C.c_uint64, C.c_uint32]; lib.trackemu_text.restype = C.c_longlong
        lib.trackemu_text_injected.argtypes = [C.c_uint32] + [vp] * 4; lib.trackemu_text_injected.restype = C.c_longlong
        lib.trackemu_text_copy.argtypes = [vp]
        _lib = lib
    return _lib


def _begin(lib, lengths, names, merge_later):
    lens = np.array([int(x) for x in lengths], np.uint64)
    raw = [n.encode() for n in names]
    name_len = np.array([len(r) for r in raw], np.uint32)
    lib.trackemu_begin(len(lens), lens.ctypes.data, b"".join(raw), name_len.ctypes.data, 1 if merge_later else 0)


def _text(lib, nbytes):
    assert nbytes >= 0, "check %d of the harness" % -nbytes
    buf = C.create_string_buffer(max(int(nbytes), 1))
    lib.trackemu_text_copy(buf)
    return buf.raw[:nbytes]


def run(batches, lengths, names, merge_later=False, seed=0, windows=None):
    """Events of every batch, scan, rows, text.  Returns a dict: the row columns, the scalars of rsqc_track_info, chunks (workgroups
    of the row kernels) and text (all rows; `windows`: formatted that many rows at a time and joined)."""
    lib = _load()
    lib.trackemu_set_schedule_seed(int(seed))
    try:
        _begin(lib, lengths, names, merge_later)
        for b in batches:
            s = b.to_struct()
            rc = lib.trackemu_add_batch(s.core, s.aux, s.n, s.cigar, s.n_cigar_total, s.seg_tid, s.seg_start, s.n_seg, s.wide_index, s.wide_n_cigar, s.n_wide)
            assert rc == 0, "a write past the difference array"
        stats = np.zeros(6, np.uint64)
        rc = lib.trackemu_end(stats.ctypes.data)
        assert rc == 0, rc
        n = int(stats[0])
        cols = [np.zeros(max(n, 1), np.int32)] + [np.zeros(max(n, 1), np.uint32) for _ in range(3)]
        lib.trackemu_rows(*[c.ctypes.data for c in cols])
        step = windows or max(n, 1)
        text = b"".join(_text(lib, lib.trackemu_text(k, min(step, n - k))) for k in range(0, n, step))
    finally:
        lib.trackemu_set_schedule_seed(0)
    out = {f: c[:n].copy() for f, c in zip(("tid", "start", "end", "depth"), cols)}
    out.update(n_rows=n, population=int(stats[1]), aligned_bases=int(stats[2]), clipped_bases=int(stats[3]), positions=int(stats[4]), chunks=int(stats[5]), text=text)
    return out


def format_rows(names, tid, start, end, depth):
    """The line-length and format kernels on INJECTED rows."""
    lib = _load()
    _begin(lib, [1] * len(names), names, False)
    cols = [np.ascontiguousarray(tid, np.int32)] + [np.ascontiguousarray(x, np.uint32) for x in (start, end, depth)]
    return _text(lib, lib.trackemu_text_injected(len(cols[0]), *[c.ctypes.data for c in cols]))
