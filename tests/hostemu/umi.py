"""TEST HARNESS: bam_parse_record / sam_parse_fields of the product on one record or one line with a chosen UMI source (see
umi_emu.cpp), and a small builder that writes the SAME alignment as a BAM record and as a SAM line."""
import ctypes as C
import os
import struct
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(os.path.dirname(_HERE))
_SO = os.path.join(_HERE, "libumiemu.so")
NAMES = ["chrA", "chrB"]
FIELDS = ("code", "tid", "pos", "mpos", "isize", "flag", "mapq", "l_seq", "nm", "n_ops", "tagbits", "wide", "qname_len", "qhash2", "qhash_lo", "qhash_hi")
NONE, TAG, QNAME = 0, 1, 2


def build():
    csrc = os.path.join(_ROOT, "rnaseqc_amd", "csrc")
    srcs = [os.path.join(_HERE, "umi_emu.cpp")] + [os.path.join(csrc, h) for h in ("rsqc_umi.h", "rsqc_bamrec.h", "rsqc_samrec.h")] + [os.path.join(_ROOT, "include", "rnaseqc_amd.h")]
    if not os.path.exists(_SO) or any(os.path.getmtime(_SO) < os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-fvisibility=hidden", srcs[0], "-o", _SO])
    return _SO


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.umiemu_setup.argtypes = [C.c_int32, C.POINTER(C.c_char_p), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]
        _lib.umiemu_bam_record.argtypes = [C.c_char_p, C.c_uint32, C.POINTER(C.c_int64)]
        _lib.umiemu_sam_line.argtypes = [C.c_char_p, C.c_uint32, C.POINTER(C.c_int64)]
    return _lib


def setup(source=NONE, tag="RX", sep="_"):
    names = (C.c_char_p * len(NAMES))(*[n.encode() for n in NAMES])
    lib().umiemu_setup(len(NAMES), names, source, ord(tag[0]), ord(tag[1]), ord(sep))


def _out(v):
    d = {f: int(v[k]) for k, f in enumerate(FIELDS)}
    d["umi"] = (int(v[16]) & 0xFFFFFFFF) | ((int(v[17]) & 0xFFFFFFFF) << 32)
    return d


def parse_bam(rec: bytes):
    v = (C.c_int64 * 18)()
    lib().umiemu_bam_record(rec, len(rec), v)
    return _out(v)


def parse_sam(line: bytes):
    v = (C.c_int64 * 18)()
    lib().umiemu_sam_line(line, len(line), v)
    return _out(v)


# ---- one alignment, two spellings --------------------------------------------------------------------------------------------
# aux: a list of (tag, type, value): 'Z' text, 'A' one character, 'i' an integer (BAM: int32), 'B' a list of int8 ('c')
def bam_aux(aux):
    out = b""
    for tag, typ, val in aux:
        out += tag.encode()
        if typ == "Z":
            out += b"Z" + val.encode("latin-1") + b"\x00"
        elif typ == "A":
            out += b"A" + val.encode("latin-1")
        elif typ == "i":
            out += b"i" + struct.pack("<i", val)
        elif typ == "B":
            out += b"Bc" + struct.pack("<I", len(val)) + bytes(v & 0xFF for v in val)
        else:
            raise ValueError(typ)
    return out


def sam_aux(aux):
    out = []
    for tag, typ, val in aux:
        out.append("%s:%s:%s" % (tag, typ, ("c," + ",".join(str(v) for v in val)) if typ == "B" else val))
    return out


def bam_record(name, aux=(), raw_aux=None, flag=0, tid=0, pos=100, mapq=60, length=20):
    """block_size + record: `length` M, SEQ of that many bases; raw_aux: the aux bytes as given (malformed tails)."""
    nm = name.encode("latin-1")
    rec = struct.pack("<iiBBHHHiiii", tid, pos, len(nm) + 1, mapq, 4680, 1, flag, length, -1, -1, 0)
    rec += nm + b"\x00" + struct.pack("<I", (length << 4) | 0) + b"\x11" * ((length + 1) // 2) + b"\xff" * length
    rec += bam_aux(aux) if raw_aux is None else raw_aux
    return struct.pack("<I", len(rec)) + rec


def sam_line(name, aux=(), flag=0, tid=0, pos=100, mapq=60, length=20):
    f = [name, str(flag), NAMES[tid], str(pos + 1), str(mapq), "%dM" % length, "*", "0", "0", "A" * length, "*"] + sam_aux(aux)
    return "\t".join(f).encode("latin-1")
