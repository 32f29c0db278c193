"""The catalogue of --cycles: explicit records (flag, name, seq, qual-or-None; tests/cycle_ref.py says what they count as) at the smallest
shapes at which the stage can go wrong, and a builder that writes the same alignments as BAM records, as SAM lines and through BGZF
with chosen block cuts.  Pure Python (struct, zlib): no product code is involved in building an input."""
import functools
import random
import struct
import zlib

from tests import cycle_ref as ref

CONTIGS = [("chrA", 1_000_000), ("chrB", 500_000)]
LENGTHS = [0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 700, 20000]


def _seq(L, salt=0):
    return "".join("ACGTN"[(i * 7 + i // 5 + salt) % 5] for i in range(L))


def _qual(L, salt=0):
    """A quality per index that differs from its neighbours' far and near: a cycle that is off by one, or mirrored, shows."""
    return [(i * 11 + i // 64 + salt) % 64 for i in range(L)]


def lengths():
    """Every length forward and reverse, single-end and as a second mate, with per-index distinct qualities."""
    out = []
    for L in LENGTHS:
        for flag in (0x0, 0x10, 0x1 | 0x80, 0x1 | 0x80 | 0x10):
            out.append((flag, "len%d_%x" % (L, flag), _seq(L, L), _qual(L, L) if L else None))
    return out


def flags():
    s, q = _seq(9), _qual(9, 3)
    fl = [0x0, 0x1, 0x1 | 0x40, 0x1 | 0x80, 0x1 | 0x40 | 0x80, 0x80, 0x40, 0x100, 0x200, 0x800, 0x1 | 0x80 | 0x100, 0x4, 0x1 | 0x4 | 0x80, 0x400, 0x1 | 0x80 | 0x400,
          0x1 | 0x2 | 0x20 | 0x80, 0x10 | 0x400]
    return [(f, "flag%x" % f, s, q) for f in fl]


def letters():
    """All 16 nibbles at even and at odd index, the SAM spellings that are no upper-case ACGT, forward and reverse."""
    out = []
    for flag in (0x0, 0x10):
        out.append((flag, "nib_even_%x" % flag, ref.NIBBLES, _qual(16, 1)))
        out.append((flag, "nib_odd_%x" % flag, "A" + ref.NIBBLES, _qual(17, 2)))
        out.append((flag, "text_%x" % flag, "acgtn=.RYK", _qual(10, 5)))
        out.append((flag, "text_odd_%x" % flag, "Tacgtn=.RYK", _qual(11, 6)))
    return out


def qualities(bam_only=False):
    out = []
    for v in (0, 62, 63, 64, 93):
        out.append((0x0, "q%d" % v, "ACGT", [v] * 4))
        out.append((0x1 | 0x80 | 0x10, "q%d_r2" % v, "ACGTA", [v, 1, 2, 3, v]))
    out.append((0x0, "q_missing", "ACGTACG", None))                 # BAM: all 0xFF; SAM: *
    out.append((0x10, "q_missing_L1", "G", None))                   # SAM: QUAL * with L = 1 is a missing quality, not the value 9
    out.append((0x0, "q_bang_tilde", "ACGTAC", [0, 93, 0, 93, 93, 0]))     # SAM bytes ! and ~
    if bam_only:
        out.append((0x0, "q254", "ACGTA", [254, 0, 254, 63, 64]))
        out.append((0x10, "q_late_ff", "ACGTAC", [7, 0xFF, 0xFF, 1, 0xFF, 2]))     # first byte valid: the later 0xFF are values (clamped)
    return out


def alignments():
    """Read names of 1..9 bytes: with the NUL, SEQ starts at every offset mod 8 (and so does QUAL, with L = 15 and 16)."""
    out = []
    for n in range(1, 10):
        for L in (15, 16, 130):
            out.append((0x10 if n % 2 else 0x0, "n" * n, _seq(L, n), _qual(L, n)))
    return out


def pileup():
    """70 000 identical 4-base records: more than 65 535 in one (end, cycle, quality) cell; then the same split over both ends."""
    one = (0x0, "p", "ACGT", [30, 31, 32, 33])
    two = (0x1 | 0x80, "p", "ACGT", [30, 31, 32, 33])
    return [one] * 70000 + [one if k % 2 else two for k in range(70000)]


def catalogue(bam_only=False):
    return lengths() + flags() + letters() + qualities(bam_only) + alignments()


def excluded_only():
    return [(f, "x%x" % f, "ACGT", [1, 2, 3, 4]) for f in (0x100, 0x200, 0x800, 0x900)]


def mixed(n=20000, seed=7):
    """About 20 000 seeded-random records, L 1..600, binned qualities, a few without SEQ or QUAL, both ends and strands."""
    rng = random.Random(seed)
    bins = [2, 12, 23, 37, 40]
    out = []
    for k in range(n):
        L = rng.randint(1, 600)
        r = rng.random()
        flag = rng.choice((0x0, 0x10, 0x1 | 0x40, 0x1 | 0x40 | 0x10, 0x1 | 0x80, 0x1 | 0x80 | 0x10))
        if r < 0.02:
            flag |= rng.choice((0x100, 0x200, 0x800))
        if r > 0.97:
            flag |= 0x400
        seq = "".join(rng.choices("ACGTN", weights=(30, 20, 20, 29, 1), k=L)) if r > 0.01 else ""
        qual = None if (not seq or 0.01 < r < 0.015) else rng.choices(bins, k=L)
        out.append((flag, "m%d" % k, seq, qual))
    return out


@functools.lru_cache(maxsize=None)
def mixed_tables():
    """(records, reference of the first half, of the second half, of all), each (base, qual, info): computed once per session and
    shared by the tests that need it; nobody changes it."""
    records = mixed()
    half = len(records) // 2
    a, b = ref.tables(records[:half]), ref.tables(records[half:])
    whole = (ref.add_tables(a[0], b[0]), ref.add_tables(a[1], b[1]), {f: a[2][f] + b[2][f] for f in ref.INFO_FIELDS})
    return records, a, b, whole


# ---- spellings -------------------------------------------------------------------------------------------------------------------
def bam_record(rec, tid=0, pos=100, mapq=60):
    """block_size + record, with where SEQ and QUAL start (offsets from the block_size field)."""
    flag, name, seq, qual = rec
    L = len(seq)
    nm = name.encode("latin-1") + b"\x00"
    nib = [ref.nibble_of_text(ch) for ch in seq] + [0]
    packed = bytes((nib[2 * k] << 4) | nib[2 * k + 1] for k in range((L + 1) // 2))
    q = b"\xff" * L if qual is None else bytes(qual)
    assert len(q) == L
    body = struct.pack("<iiBBHHHiiii", tid, pos, len(nm), mapq, 4680, 1, flag, L, -1, -1, 0) + nm + struct.pack("<I", max(L, 1) << 4)
    seq_off = 4 + len(body)
    body += packed
    qual_off = 4 + len(body)
    body += q + b"NMC\x00"
    return struct.pack("<I", len(body)) + body, seq_off, qual_off


def sam_line(rec, tid=0, pos=100, mapq=60):
    flag, name, seq, qual = rec
    assert qual is None or max(qual) <= 93, "a quality above 93 has no SAM spelling"
    q = "*" if qual is None else "".join(chr(v + 33) for v in qual)
    f = [name, str(flag), CONTIGS[tid][0], str(pos + 1), str(mapq), "%dM" % max(len(seq), 1), "*", "0", "0", seq or "*", q, "NM:i:0"]
    return "\t".join(f).encode("latin-1") + b"\n"


def bam_header():
    text = ("@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % c for c in CONTIGS)).encode()
    out = b"BAM\x01" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(CONTIGS))
    for name, length in CONTIGS:
        out += struct.pack("<i", len(name) + 1) + name.encode() + b"\x00" + struct.pack("<i", length)
    return out


def sam_header():
    return ("@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % c for c in CONTIGS)).encode()


def bam_body(records, positions=None):
    """The records one behind the other, and per record (start, SEQ start, QUAL start, end) in that stream.  positions: every record's
    0-based position (default: all at 100)."""
    parts, where, at = [], [], 0
    for k, r in enumerate(records):
        b, so, qo = bam_record(r, pos=positions[k] if positions else 100)
        parts.append(b); where.append((at, at + so, at + qo, at + len(b))); at += len(b)
    return b"".join(parts), where


def sam_body(records, positions=None):
    return b"".join(sam_line(r, pos=positions[k] if positions else 100) for k, r in enumerate(records))


def bgzf_block(data):
    """One BGZF block of `data` (at most 64 KiB), and its (payload, isize, crc) as rsqc_decode_submit's block table wants them."""
    assert len(data) <= 65536
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    payload = c.compress(data) + c.flush()
    if len(payload) > 65000:                                         # (random bytes: stored)
        c = zlib.compressobj(0, zlib.DEFLATED, -15)
        payload = c.compress(data) + c.flush()
    crc = zlib.crc32(data) & 0xFFFFFFFF
    block = b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", len(payload) + 25) + payload + struct.pack("<II", crc, len(data))
    return block, (payload, len(data), crc)


def cut(data, cuts=(), block=0xFF00):
    """data in pieces: cut at every offset of `cuts` and wherever a piece would exceed `block` bytes."""
    edges = sorted(set([0, len(data)] + [c for c in cuts if 0 < c < len(data)]))
    out = []
    for a, b in zip(edges, edges[1:]):
        out += [data[p:min(b, p + block)] for p in range(a, b, block)]
    return out


BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def write_bam(path, records, cuts=(), block=0xFF00, positions=None):
    """A BAM file: the header in blocks of its own, then the records cut as cut() says (offsets into the record stream)."""
    body, _ = bam_body(records, positions)
    with open(path, "wb") as f:
        for piece in cut(bam_header()) + cut(body, cuts, block):
            f.write(bgzf_block(piece)[0])
        f.write(BGZF_EOF)


def write_sam(path, records, bgzf=False, cuts=(), block=0xFF00, positions=None):
    text = sam_header() + sam_body(records, positions)
    with open(path, "wb") as f:
        if not bgzf:
            f.write(text)
            return
        for piece in cut(text, cuts, block):
            f.write(bgzf_block(piece)[0])
        f.write(BGZF_EOF)
