"""TEST HARNESS: what cycle.py, mismatch.py and allele.py have in common: the build of a stage's emulation library (stale when its source or
one of its headers is newer) and of its stand-alone sanitizer program, and the loop over a stream's windows under a schedule seed."""
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(os.path.dirname(_HERE))
_CSRC = os.path.join(_ROOT, "rnaseqc_amd", "csrc")
# what every stage's emulation includes, behind its own headers
_SHARED = [os.path.join(_CSRC, h) for h in ("rsqc_cycle.h", "rsqc_bamrec.h", "rsqc_samrec.h", "rsqc_sam.h", "rsqc_decode.h", "rsqc_umi.h")] + \
          [os.path.join(_ROOT, "include", "rnaseqc_amd.h"), os.path.join(_HERE, "wavemu.h"), os.path.join(_HERE, "window_emu.h")]


def _stale(out, srcs):
    return not os.path.exists(out) or any(os.path.getmtime(out) < os.path.getmtime(s) for s in srcs)


def build(stage, own_headers=()):
    """<stage>_emu.cpp -> lib<stage>emu.so; own_headers: the headers of csrc/ only this stage includes."""
    src, so = os.path.join(_HERE, stage + "_emu.cpp"), os.path.join(_HERE, "lib%semu.so" % stage)
    if _stale(so, [src] + [os.path.join(_CSRC, h) for h in own_headers] + _SHARED):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-fvisibility=hidden", "-Wno-unused-function", "-Wno-unused-variable", src, "-o", so])
    return so


def build_fuzz(stage, exe):
    """<stage>_fuzz.cpp as a program of its own under AddressSanitizer and UBSan (nothing is preloaded: it is run as a child process)."""
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", os.path.join(_HERE, stage + "_fuzz.cpp"), "-o", exe])
    return exe


def run_windows(set_seed, seed, t, windows, call):
    """call(w) -> the records of window w, launched into the tables t; every window under the schedule seed, which is put back."""
    set_seed(int(seed))
    try:
        for w in windows:
            n = call(w)
            assert n >= 0
            t.records += n
    finally:
        set_seed(0)
    return t
