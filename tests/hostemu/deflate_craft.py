"""TEST HARNESS: a DEFLATE (RFC 1951) *writer* that does what it is told.

zlib's deflate decides block types, code lengths and matches on its own, so the streams it writes reach the limits of the
decoder under test (rnaseqc_amd/csrc/rsqc_inflate.h) only by accident.  Here the caller decides: stored, fixed and dynamic
blocks from an explicit token list, the code lengths of both alphabets, every field of the dynamic header (HLIT, HDIST, HCLEN,
the code-length code's own lengths, where the repeat codes 16 / 17 / 18 are used), and -- for real data -- a greedy tokeniser
whose matches are placed by a policy.  Nothing here is fast or compresses well; every stream is checked against zlib's
inflate (checked()) before a test hands it to the decoder.

Tokens: an int 0..255 is a literal, a tuple (length, distance) a match; the end-of-block symbol is written by the block.
"""
import heapq
import struct
import zlib

# RFC 1951 3.2.5
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
             16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


def len_symbol(length):
    """(symbol, extra bits, extra value) of a match length 3..258.  258 is symbol 285; 257 is symbol 284 with extra 30."""
    assert 3 <= length <= 258
    if length == 258:
        return 285, 0, 0
    k = max(i for i in range(28) if LEN_BASE[i] <= length)
    return 257 + k, LEN_EXTRA[k], length - LEN_BASE[k]


def dist_symbol(dist):
    assert 1 <= dist <= 32768
    k = max(i for i in range(30) if DIST_BASE[i] <= dist)
    return k, DIST_EXTRA[k], dist - DIST_BASE[k]


class BitWriter:
    """Bits least significant first (RFC 1951 3.1.1); Huffman codes most significant bit first."""

    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def bits(self, value, n):
        assert 0 <= value < (1 << n) or n == 0
        self.acc |= value << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, n):
        rev = 0
        for b in range(n):
            rev |= ((code >> b) & 1) << (n - 1 - b)
        self.bits(rev, n)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    @property
    def bit_length(self):
        return len(self.out) * 8 + self.n

    def getvalue(self):
        return bytes(self.out) + (bytes([self.acc & 0xFF]) if self.n else b"")


def kraft(lengths, maxbits=15):
    """Sum of 2^(maxbits - l) over the codes; a complete set gives 2^maxbits."""
    return sum(1 << (maxbits - l) for l in lengths if l)


def canonical_codes(lengths):
    """{symbol: (code, length)} of RFC 1951 3.2.2."""
    count = [0] * 17
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for b in range(1, 17):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = {}
    for s, l in enumerate(lengths):
        if l:
            out[s] = (nxt[l], l)
            nxt[l] += 1
    return out


def lengths_from_freqs(freqs, maxbits):
    """Code lengths of at most maxbits for the symbols with freq > 0: a Huffman code, pushed under the limit and made complete
    again.  At least two symbols get a code (a lone symbol gets a neighbour), so the set is always Kraft-complete."""
    n = len(freqs)
    used = [s for s in range(n) if freqs[s] > 0]
    freqs = list(freqs)
    while len(used) < 2:
        s = next(s for s in range(n) if s not in used)
        used.append(s); freqs[s] = 1
    heap = [(freqs[s], s, (s,)) for s in used]
    heapq.heapify(heap)
    lens = [0] * n
    tie = n
    while len(heap) > 1:
        fa, _ta, a = heapq.heappop(heap)
        fb, _tb, b = heapq.heappop(heap)
        for s in a + b:
            lens[s] += 1
        heapq.heappush(heap, (fa + fb, tie, a + b)); tie += 1
    for s in used:
        lens[s] = min(lens[s], maxbits)
    target = 1 << maxbits
    k = kraft(lens, maxbits)
    while k > target:                                   # over-subscribed by the clamp: lengthen the deepest code that can grow
        s = max((s for s in used if lens[s] < maxbits), key=lambda s: (lens[s], -freqs[s]))
        k -= 1 << (maxbits - lens[s] - 1)
        lens[s] += 1
    while k < target:                                   # room left: shorten the most frequent code that fits
        s = max((s for s in used if lens[s] > 1 and k + (1 << (maxbits - lens[s])) <= target), key=lambda s: (lens[s], freqs[s]))
        k += 1 << (maxbits - lens[s])
        lens[s] -= 1
    assert kraft(lens, maxbits) == target
    return lens


def rle_code_lengths(seq, use16=True, use17=True, use18=True):
    """The code-length sequence (literal/length lengths followed by the distance lengths, as ONE run: repeats cross the border)
    as [(symbol, extra value)] of the code-length alphabet."""
    ops, i, n = [], 0, len(seq)
    while i < n:
        v = seq[i]
        run = 1
        while i + run < n and seq[i + run] == v:
            run += 1
        if v == 0 and run >= 3 and (use17 or use18):
            if use18 and run >= 11:
                r = min(run, 138); ops.append((18, r - 11))
            elif use17:
                r = min(run, 10); ops.append((17, r - 3))
            else:
                r = 1; ops.append((0, 0))
            i += r
            continue
        if v != 0 and use16 and run >= 4:
            ops.append((v, 0)); i += 1; run -= 1
            while run >= 3:
                r = min(run, 6); ops.append((16, r - 3)); i += r; run -= r
            continue
        ops.append((v, 0)); i += 1
    return ops


def expand_cl_ops(ops):
    out = []
    for s, x in ops:
        if s < 16:
            out.append(s)
        elif s == 16:
            out += [out[-1]] * (3 + x)
        elif s == 17:
            out += [0] * (3 + x)
        else:
            out += [0] * (11 + x)
    return out


_CL_EXTRA = {16: 2, 17: 3, 18: 7}


def token_freqs(tokens):
    ll, dd = [0] * 286, [0] * 30
    for t in tokens:
        if isinstance(t, tuple):
            ll[len_symbol(t[0])[0]] += 1
            dd[dist_symbol(t[1])[0]] += 1
        else:
            ll[t] += 1
    ll[256] += 1
    return ll, dd


_LEN_SYM = [None] * 3 + [len_symbol(n) for n in range(3, 259)]
_DIST_SYM = [None] + [s for k in range(30) for s in [(k, DIST_EXTRA[k], x) for x in range(min(1 << DIST_EXTRA[k], 32769 - DIST_BASE[k]))]]


def _reversed(codes):
    """{symbol: (the code as the bit writer takes it -- first bit lowest --, length)}"""
    out = {}
    for s, (code, n) in codes.items():
        out[s] = (int(format(code, "0%db" % n)[::-1], 2), n)
    return out


def _write_tokens(w, tokens, lcodes, dcodes, eob=True):
    lrev, drev = _reversed(lcodes), _reversed(dcodes)
    acc, n, out = w.acc, w.n, w.out                      # (the bit writer's loop, inlined: this is where a crafted file's time goes)
    for t in tokens:
        if t.__class__ is tuple:
            s, xb, xv = _LEN_SYM[t[0]]
            c, l = lrev[s]
            acc |= (c | (xv << l)) << n; n += l + xb
            d, db, dv = _DIST_SYM[t[1]]
            c, l = drev[d]
            acc |= (c | (dv << l)) << n; n += l + db
        else:
            c, l = lrev[t]
            acc |= c << n; n += l
        while n >= 8:
            out.append(acc & 0xFF); acc >>= 8; n -= 8
    w.acc, w.n = acc, n
    if eob:
        w.code(*lcodes[256])


def stored_block(w, data, final=False):
    assert len(data) <= 65535
    w.bits(1 if final else 0, 1); w.bits(0, 2)
    w.align()
    w.bits(len(data), 16); w.bits(len(data) ^ 0xFFFF, 16)
    assert w.n == 0
    w.out += data


_FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
_FIXED_D = [5] * 32


def fixed_block(w, tokens, final=False):
    w.bits(1 if final else 0, 1); w.bits(1, 2)
    _write_tokens(w, tokens, canonical_codes(_FIXED_LL), canonical_codes(_FIXED_D))


def dynamic_block(w, tokens, ll_lengths=None, d_lengths=None, final=False, hlit=None, hdist=None, hclen=None, cl_lengths=None, cl_ops=None,
                  use16=True, use17=True, use18=True, max_ll_bits=15, max_d_bits=15):
    """One dynamic block.  ll_lengths / d_lengths: code lengths by symbol (shorter lists are padded with zeros); None = a Huffman
    code for the tokens.  d_lengths may be all zero (no distance code) or hold a single code.  hlit / hdist: how many lengths of
    each alphabet the header carries (default: up to the last non-zero one, at least 257 / 1).  cl_ops: the run-length coded
    lengths as [(symbol of the code-length alphabet, extra value)] (default: rle_code_lengths over both alphabets as one
    sequence, with the repeat codes the use16/17/18 switches allow).  cl_lengths: the 19 lengths (<= 7) of the code-length code
    by symbol (default: a Huffman code for cl_ops).  hclen: how many of them the header carries, in CL_ORDER (default: up to the
    last non-zero one, at least 4)."""
    fl, fd = token_freqs(tokens)
    if ll_lengths is None:
        ll_lengths = lengths_from_freqs(fl, max_ll_bits)
    if d_lengths is None:
        d_lengths = lengths_from_freqs(fd, max_d_bits) if any(fd) else [0]
    ll = list(ll_lengths) + [0] * (286 - len(ll_lengths))
    dl = list(d_lengths) + [0] * (30 - len(d_lengths))
    assert len(ll) == 286 and len(dl) == 30 and max(ll) <= 15 and max(dl) <= 15 and ll[256]
    assert kraft(ll) == 1 << 15, "literal/length lengths are not Kraft-complete"
    assert kraft(dl) == 1 << 15 or sum(1 for l in dl if l) <= 1, "distance lengths: complete, a single code, or none"
    if hlit is None:
        hlit = max(257, max(s for s in range(286) if ll[s]) + 1)
    if hdist is None:
        hdist = max([1] + [s + 1 for s in range(30) if dl[s]])
    assert 257 <= hlit <= 286 and 1 <= hdist <= 30 and not any(ll[hlit:]) and not any(dl[hdist:])
    seq = ll[:hlit] + dl[:hdist]
    if cl_ops is None:
        cl_ops = rle_code_lengths(seq, use16, use17, use18)
    assert expand_cl_ops(cl_ops) == seq, "cl_ops do not spell the code lengths"
    if cl_lengths is None:
        f = [0] * 19
        for s, _x in cl_ops:
            f[s] += 1
        cl_lengths = lengths_from_freqs(f, 7)
    assert len(cl_lengths) == 19 and max(cl_lengths) <= 7 and kraft(cl_lengths, 7) == 1 << 7 and all(cl_lengths[s] for s, _x in cl_ops)
    if hclen is None:
        hclen = max(4, max(k + 1 for k in range(19) if cl_lengths[CL_ORDER[k]]))
    assert 4 <= hclen <= 19 and not any(cl_lengths[CL_ORDER[k]] for k in range(hclen, 19))
    w.bits(1 if final else 0, 1); w.bits(2, 2)
    w.bits(hlit - 257, 5); w.bits(hdist - 1, 5); w.bits(hclen - 4, 4)
    for k in range(hclen):
        w.bits(cl_lengths[CL_ORDER[k]], 3)
    clc = canonical_codes(cl_lengths)
    for s, x in cl_ops:
        w.code(*clc[s])
        if s >= 16:
            w.bits(x, _CL_EXTRA[s])
    _write_tokens(w, tokens, canonical_codes(ll), canonical_codes(dl))


def expand(tokens, history=b""):
    """The bytes a token list stands for (behind `history`)."""
    out = bytearray(history)
    for t in tokens:
        if isinstance(t, tuple):
            n, d = t
            assert 1 <= d <= len(out), "distance %d reaches before the start (at %d)" % (d, len(out))
            if d >= n:
                out += out[len(out) - d:len(out) - d + n]
            else:
                for _ in range(n):
                    out.append(out[-d])
        else:
            out.append(t)
    return bytes(out[len(history):])


def checked(stream, expected):
    """The reference is zlib's inflate: the stream must give exactly `expected`, use every byte, and end.  Returns
    (stream, expected) for the decoder under test."""
    d = zlib.decompressobj(-15)
    got = d.decompress(stream)
    assert got == expected, "zlib inflates the crafted stream to other bytes (%d, wanted %d)" % (len(got), len(expected))
    assert d.unused_data == b"" and d.eof, "the crafted stream does not end where its bytes end"
    return stream, expected


# ---- a greedy tokeniser whose matches are placed by a policy ----------------------------------------------------------------
class Policy:
    """min_dist / max_dist: the distances a match may use.  prefer: distances tried first, in this order (exact values).
    only_preferred: no other distance is tried.  min_len / max_len: match lengths.  force_at: output offsets at which a match MUST start (the match in front of it is cut
    short; an error if the data has no match there).  chain: candidates looked at per position."""

    def __init__(self, min_dist=1, max_dist=32768, prefer=(), min_len=3, max_len=258, force_at=(), chain=24, matches=True, only_preferred=False):
        self.min_dist, self.max_dist, self.prefer, self.only_preferred = min_dist, max_dist, tuple(prefer), only_preferred
        self.min_len, self.max_len, self.force_at, self.chain, self.matches = max(3, min_len), min(258, max_len), frozenset(force_at), chain, matches


def _match_len(data, src, at, limit):
    n = 0
    step = 32
    while n + step <= limit and data[src + n:src + n + step] == data[at + n:at + n + step]:
        n += step
    while n < limit and data[src + n] == data[at + n]:
        n += 1
    return n


def tokenize(data, policy=None, start=0):
    """Greedy tokens for data[start:] (data[:start] is history that matches may reach into)."""
    p = policy or Policy()
    n = len(data)
    tokens, table = [], {}
    forced = sorted(x for x in p.force_at if start <= x < n)
    i = 0
    def insert(k):
        if k + 3 <= n:
            table.setdefault(data[k:k + 3], []).append(k)
    for k in range(0, start):
        insert(k)
    i = start
    while i < n:
        nxt = next((x for x in forced if x > i), n)                 # a match may not cross the next forced start
        limit = min(p.max_len, n - i, nxt - i)
        best_len, best_dist = 0, 0
        if p.matches and limit >= p.min_len:
            for d in p.prefer:
                if p.min_dist <= d <= min(p.max_dist, i):
                    m = _match_len(data, i - d, i, limit)
                    if m >= p.min_len and m > best_len:
                        best_len, best_dist = m, d
            if not best_len and not p.only_preferred:
                cand = table.get(data[i:i + 3], ())
                seen = looked = 0
                for src in reversed(cand):
                    d = i - src
                    looked += 1
                    if looked > 16 * p.chain:
                        break
                    if d < p.min_dist:
                        continue
                    if d > p.max_dist:
                        break
                    m = _match_len(data, src, i, limit)
                    if m >= p.min_len and m > best_len:
                        best_len, best_dist = m, d
                        if m == limit:
                            break
                    seen += 1
                    if seen >= p.chain:
                        break
        if i in p.force_at:
            assert best_len, "no match can start at forced offset %d" % i
        if best_len:
            tokens.append((best_len, best_dist))
            for k in range(i, min(i + best_len, i + 4)):
                insert(k)
            if best_len > 8:
                insert(i + best_len - 3); insert(i + best_len - 2); insert(i + best_len - 1)
            i += best_len
        else:
            tokens.append(data[i]); insert(i); i += 1
    return tokens


def deflate_tokens(data, policy=None, block_tokens=None, kind="dynamic", **header):
    """A whole raw DEFLATE stream for `data`: tokenised by the policy, written as blocks of at most `block_tokens` tokens of the
    given kind ("dynamic", "fixed"); `header` goes to dynamic_block."""
    w = BitWriter()
    toks = tokenize(data, policy)
    step = block_tokens or max(1, len(toks))
    parts = [toks[o:o + step] for o in range(0, len(toks), step)] or [[]]
    for k, part in enumerate(parts):
        final = k == len(parts) - 1
        if kind == "fixed":
            fixed_block(w, part, final)
        else:
            dynamic_block(w, part, final=final, **header)
    return w.getvalue()


def stored_stream(data):
    w = BitWriter()
    parts = [data[o:o + 65535] for o in range(0, len(data), 65535)] or [b""]
    for k, part in enumerate(parts):
        stored_block(w, part, k == len(parts) - 1)
    return w.getvalue()


# ---- BGZF (SAM spec 4.1) -------------------------------------------------------------------------------------------------
def bgzf_block(data, stream):
    """The BGZF block (a gzip member with the BC extra field) that holds `data` as the raw DEFLATE `stream`."""
    bsize = len(stream) + 26
    assert len(data) <= 65536 and bsize <= 65536, "a BGZF block is at most 64 KiB on either side"
    return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", bsize - 1) + stream +
            struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data)))


BGZF_EOF = bgzf_block(b"", b"\x03\x00")
