"""TEST HARNESS: the catalogue of hand-built DEFLATE streams aimed at the limits of rnaseqc_amd/csrc/rsqc_inflate.h.

Every case is a named function that returns (stream, expected bytes); CASES maps the name to (function, reached), where
reached(stats) asserts -- on the counters of the -DINF_STATS host build (tests/hostemu/decode.py: inflate_with_stats) -- that
the stream went down the path it is named for.  The limits are read from the header's #defines (K), so a retune moves the
cases with it.  Every stream passed zlib's inflate (deflate_craft.checked) before it is returned.
"""
import os
import random
import re

from . import deflate_craft as dc

_HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "rnaseqc_amd", "csrc", "rsqc_inflate.h")


class Limits:
    def __init__(self, path=_HEADER):
        text = open(path).read()

        def define(name):
            m = re.search(r"^#define\s+%s\s+(\d+)\s*$" % name, text, re.M)
            assert m, "rsqc_inflate.h no longer defines %s" % name
            return int(m.group(1))
        self.RING = 1 << define("INF_RING_BITS_CFG")
        self.FLUSH = define("INF_FLUSH_CFG")
        self.ROUND = define("INF_ROUND_BYTES_CFG")
        self.LBITS = define("INF_LBITS_CFG")
        self.DBITS = define("INF_DBITS_CFG")
        m = re.search(r"INF_NEAR\s*=\s*INF_RING\s*-\s*(\d+)u?\s*;", text)
        assert m, "rsqc_inflate.h no longer defines INF_NEAR as INF_RING minus a constant"
        self.NEAR = self.RING - int(m.group(1))


K = Limits()
CASES = {}


def need(pred):
    """reached(stats) from a predicate."""
    def reached(st):
        assert pred(st), {k: v for k, v in st.items() if v}
    return reached


def case(reached):
    def deco(fn):
        CASES[fn.__name__] = (fn, reached)
        return fn
    return deco


def rnd_bytes(n, seed, alphabet=None):
    r = random.Random(seed)
    if alphabet:
        return bytes(r.choice(alphabet) for _ in range(n))
    return bytes(r.getrandbits(8) for _ in range(n))


def complete_lengths(counts):
    """{length: how many codes} made Kraft-complete: what is left of the code space is handed out as one code per set bit."""
    counts = dict(counts)
    left = (1 << 15) - sum(c << (15 - l) for l, c in counts.items())
    assert left >= 0
    for l in range(1, 16):
        if left & (1 << (15 - l)):
            counts[l] = counts.get(l, 0) + 1
    return counts


def assign_lengths(n, order, counts):
    """Lengths for an alphabet of n symbols: the symbols of `order` get the codes of `counts`, shortest first."""
    lens = [0] * n
    todo = [l for l in sorted(counts) for _ in range(counts[l])]
    assert len(todo) <= len(order), (len(todo), len(order))
    for s, l in zip(order, todo):
        lens[s] = l
    return lens


def finish(w, expected):
    return dc.checked(w.getvalue(), expected)


def _history(w, n, seed, final=False):
    """n bytes of noise as stored blocks: what later matches reach back into."""
    data = rnd_bytes(n, seed)
    for o in range(0, n, 65535):
        dc.stored_block(w, data[o:o + 65535], final and o + 65535 >= n)
    return data


# ---- code shapes ---------------------------------------------------------------------------------------------------------
def _deep_codes():
    # 200 literal/length codes of 9..15 bits, 16 distance codes of 8..15 bits; the rest of each code space as short codes
    lc = complete_lengths({9: 10, 10: 10, 11: 20, 12: 20, 13: 40, 14: 40, 15: 60})
    n_short = sum(c for l, c in lc.items()) - 200
    # short codes: end of block, a few literals and lengths; deep ones: literals and every length symbol
    short = [256, 65, 257, 67, 285, 71, 84, 78][:n_short]
    assert len(short) == n_short
    lsyms = list(range(258, 285))
    deep = [s for s in lsyms] + [s for s in range(0, 256) if s not in short][:200 - len(lsyms)]
    r = random.Random(11); r.shuffle(deep)
    ll = assign_lengths(286, short + deep, lc)
    dcnt = complete_lengths({8: 1, 9: 2, 10: 2, 11: 2, 12: 2, 13: 2, 14: 3, 15: 2})
    n_dshort = sum(dcnt.values()) - 16
    dorder = list(range(0, n_dshort)) + list(range(29, 29 - 16, -1))
    dl = assign_lengths(30, dorder, dcnt)
    return ll, dl


def _reached_deep(st):
    assert all(st["long_ll"][l] > 0 for l in range(max(9, K.LBITS + 1), 16)), st["long_ll"]
    assert all(st["long_d"][l] > 0 for l in range(K.DBITS + 1, 16)), st["long_d"]


@case(_reached_deep)
def deep_codes_both_alphabets():
    """Literal/length codes of every length 9..15 and distance codes of every length 8..15 in one block, every symbol used; HCLEN 19."""
    ll, dl = _deep_codes()
    w = dc.BitWriter()
    hist = _history(w, 32768, 1)
    r = random.Random(2)
    toks = []
    lits = [s for s in range(256) if ll[s]]
    lens = [s for s in range(257, 286) if ll[s]]
    dists = [s for s in range(30) if dl[s]]
    for rep in range(2):
        for k, s in enumerate(lens):
            d = dists[(k + rep * 7) % len(dists)]
            length = dc.LEN_BASE[s - 257] + r.randrange(1 << dc.LEN_EXTRA[s - 257]) if s != 285 else 258
            if s == 284:
                length = min(length, 257)
            toks.append((length, min(32768, dc.DIST_BASE[d] + r.randrange(1 << dc.DIST_EXTRA[d]))))
            toks.append(lits[(k * 5 + rep) % len(lits)])
        for d in dists:
            toks.append((3 + r.randrange(20), dc.DIST_BASE[d]))
        toks += lits
    dc.dynamic_block(w, toks, ll, dl, final=True, hclen=19)
    return finish(w, hist + dc.expand(toks, hist))


def _codes_48():
    # literal 'a' 1 bit, end of block 2 bits, 'b'..'m' 3..14 bits, length symbols 281 / 282 (5 extra bits) 15 bits;
    # distance symbols 0..13 1..14 bits, 28 / 29 (13 extra bits) 15 bits
    ll = [0] * 286
    ll[97] = 1; ll[256] = 2
    for k in range(12):
        ll[98 + k] = 3 + k
    ll[281] = ll[282] = 15
    dl = [0] * 30
    for k in range(14):
        dl[k] = 1 + k
    dl[28] = dl[29] = 15                              # (only 28 is used: 16 KiB of history are enough for it)
    return ll, dl


def _symbols_48(lit_runs):
    ll, dl = _codes_48()
    w = dc.BitWriter()
    hist = _history(w, 24577, 3)
    r = random.Random(4)
    toks = []
    for k in lit_runs:
        toks += [97] * k
        s = 281 if r.random() < 0.8 else 282
        toks.append((dc.LEN_BASE[s - 257] + r.randrange(32), 16385 + r.randrange(8192)))
    dc.dynamic_block(w, toks, ll, dl, final=True)
    return finish(w, hist + dc.expand(toks, hist))


def _reached_48(st):
    assert st["max_symbol_bits"] == 48 and st["long_ll"][15] > 0 and st["long_d"][15] > 0, st


@case(_reached_48)
def symbols_of_48_bits_back_to_back():
    """15-bit length code + 5 extra bits + 15-bit distance code + 13 extra bits, one behind the other; a 1-bit literal every
    third symbol moves the phase, so that rounds start at every bit of a dword."""
    return _symbols_48([1 if k % 3 == 0 else 0 for k in range(160)])


SEED48 = 5


def _reached_48_lanes(st):
    _reached_48(st)
    assert st["long_here_lanes"] == (1 << 64) - 1, hex(st["long_here_lanes"])          # the walk stood on a long code at every lane 0..63
    assert st["stops_other"] > 0 and st["stop_lanes"] >> 49, hex(st["stop_lanes"])          # ... and some ran past the buffered bits (a 48-bit symbol can only do so from lane 50 on)


@case(_reached_48_lanes)
def symbols_of_48_bits_between_one_bit_literals():
    """The same symbols behind runs of 0..70 one-bit literals: the walk meets the long code (INF_K_OTHER in the lanes' own decode) at
    lane 0, at lane 63 and at every lane between them, and the ones that start late run past the buffered bits and end the round."""
    r = random.Random(SEED48)
    runs = list(range(0, 71)) * 3
    r.shuffle(runs)
    return _symbols_48(runs)


@case(need(lambda st: st["max_round_symbols"] == 64 and st["round_symbols"] >= 60 * st["rounds"]))
def one_bit_literal_code():
    """A 1-bit literal: 64 symbols in every round."""
    ll = [0] * 286
    ll[65] = 1; ll[66] = 2; ll[256] = 2
    toks = [65] * 5000 + [66] + [65] * 100
    w = dc.BitWriter()
    dc.dynamic_block(w, toks, ll, [0], final=True)
    return finish(w, dc.expand(toks))


def _one_bit_matches(lengths_cycle, n):
    # length 258 (285) 1 bit, length symbol 284 (227..257) 2 bits, end of block and 'x' 3 bits; the single distance code: distance 1
    ll = [0] * 286
    ll[285] = 1; ll[284] = 2; ll[256] = 3; ll[120] = 3
    w = dc.BitWriter()
    dc.stored_block(w, b"x")
    toks = [(lengths_cycle[k % len(lengths_cycle)], 1) for k in range(n)]
    dc.dynamic_block(w, toks, ll, [1], final=True)
    return finish(w, b"x" + dc.expand(toks, b"x"))


def _reached_cut(st):
    assert st["cuts"] > 0 and st["cut_lanes"], st


@case(need(lambda st: st["cuts"] > 0 and st["max_round_matches"] >= 3 and st["dist_hist"][1] > 0))
def one_bit_length_and_distance_codes():
    """Length 258 as a 1-bit code with the single distance code (distance 1): 32 matches buffered per round, 8 KiB of output, cut at
    the symbol that crosses INF_ROUND_BYTES."""
    return _one_bit_matches([258], 250)


def _round_sum(total):
    # three matches of 258 and one that brings the group to `total`
    last = total - 3 * 258
    assert 227 <= last <= 257
    return [258, 258, 258, last]


@case(_reached_cut)
def round_output_exactly_round_bytes():
    """Groups of matches whose lengths sum to exactly INF_ROUND_BYTES: the cut falls behind the group, the round puts out the limit."""
    return _one_bit_matches(_round_sum(K.ROUND), 60)


@case(_reached_cut)
def round_output_one_below_round_bytes():
    return _one_bit_matches(_round_sum(K.ROUND - 1), 60)


@case(_reached_cut)
def round_output_one_above_round_bytes():
    return _one_bit_matches(_round_sum(K.ROUND + 1), 60)


@case(need(lambda st: st["cuts"] > 0 and bin(st["cut_lanes"]).count("1") >= 8))
def round_cut_at_many_lanes():
    """Matches of random lengths at distance 1: the symbol that crosses INF_ROUND_BYTES stands at many different lanes."""
    r = random.Random(6)
    toks = [120] + [(258, 1) if r.random() < 0.6 else (r.randrange(3, 12), 1) if r.random() < 0.7 else 120 for _ in range(400)]
    w = dc.BitWriter()
    dc.dynamic_block(w, toks, None, [1], final=True)
    return finish(w, dc.expand(toks))


@case(need(lambda st: st["match_bytes"] == 3 + 257 + 258 + 257 + 3 + 258))
def lengths_3_257_258_fixed_and_dynamic():
    """Length 3, length 257 (symbol 284 with extra bits 30 -- not 258) and length 258 by its own symbol 285, in a fixed and in a
    dynamic block."""
    assert dc.len_symbol(257) == (284, 5, 30) and dc.len_symbol(258) == (285, 0, 0) and dc.len_symbol(3) == (257, 0, 0)
    w = dc.BitWriter()
    a = [1, 2, 3, (3, 3), (257, 2), (258, 5)]
    b = [9, (257, 1), (3, 700), (258, 259)]
    dc.fixed_block(w, a)
    dc.dynamic_block(w, b, final=True)
    exp = dc.expand(a)
    return finish(w, exp + dc.expand(b, exp))


# ---- header shapes -------------------------------------------------------------------------------------------------------
@case(need(lambda st: (st["blocks"][2] == 1 and st["near_matches"] + st["far_matches"] == 0)))
def header_all_literal_hlit_257_hdist_1_zero():
    """HLIT = 257, HDIST = 1 and that one distance length zero: an all-literal block."""
    data = rnd_bytes(3000, 7, b"ACGTN\xff\x11")
    w = dc.BitWriter()
    dc.dynamic_block(w, list(data), None, [0], final=True, hlit=257, hdist=1)
    return finish(w, data)


@case(need(lambda st: st["blocks"][2] == 1))
def header_hlit_286_hdist_30():
    toks = list(b"hello") + [(258, 5), (4, 2)]
    w = dc.BitWriter()
    dc.dynamic_block(w, toks, final=True, hlit=286, hdist=30)
    return finish(w, dc.expand(toks))


@case(need(lambda st: st["near_matches"] == 2))
def header_repeat_16_crosses_into_distance_lengths():
    """Code 16 (repeat the previous length) whose run starts in the literal/length lengths and ends in the distance lengths."""
    ll = [0] * 286
    ll[97] = 1; ll[256] = 2; ll[284] = 3; ll[285] = 3
    dl = [3] * 8
    ops = dc.rle_code_lengths(ll + dl)
    at, crossing = 0, False
    for s, x in ops:
        n = 1 if s < 16 else (3 + x if s <= 17 else 11 + x)
        crossing |= s == 16 and at < 286 < at + n
        at += n
    assert crossing
    toks = [97] * 40 + [(258, 7), (250, 13)]
    w = dc.BitWriter()
    dc.dynamic_block(w, toks, ll, dl, final=True, cl_ops=ops)
    return finish(w, dc.expand(toks))


@case(need(lambda st: st["blocks"][2] == 1))
def header_code_18_runs_of_138():
    data = rnd_bytes(500, 8, b"\x00\xff")
    ll = [0] * 286
    ll[0] = 1; ll[255] = 2; ll[256] = 2
    ops = dc.rle_code_lengths(ll[:257] + [0])
    assert (18, 127) in ops
    w = dc.BitWriter()
    dc.dynamic_block(w, list(data), ll, [0], final=True, cl_ops=ops)
    return finish(w, data)


@case(need(lambda st: st["blocks"][2] == 1))
def header_code_length_code_of_7_bits():
    """The code-length code itself with lengths 1..7, the 7-bit ones in use."""
    ll = [0] * 286
    for k, s in enumerate((101, 256, 116, 97, 111, 105, 110, 115, 104)):       # lengths 1..8, 8
        ll[s] = min(k + 1, 8)
    toks = list(b"etaoinshetaoinsh" * 20)
    seq = ll[:257] + [0]
    ops = dc.rle_code_lengths(seq, use16=False, use17=False)
    used = sorted({s for s, _x in ops})
    cl = [0] * 19
    for rank, s in enumerate(used):
        cl[s] = 1 << (len(used) - rank)                 # (as frequencies: a comb, pushed under 7 bits)
    cl = dc.lengths_from_freqs(cl, 7)
    assert max(cl) == 7 and sum(1 for l in cl if l == 7) >= 2
    w = dc.BitWriter()
    dc.dynamic_block(w, toks, ll, [0], final=True, cl_ops=ops, cl_lengths=cl)
    return finish(w, bytes(toks))


@case(need(lambda st: st["blocks"][2] == 1))
def header_hclen_smallest():
    """The shortest header a valid block can have.  HCLEN = 4 carries lengths for 16, 17, 18 and 0 only -- no length above zero can
    be spelled, so no end-of-block code: zlib rejects every such block (test_inflate_crafted.py checks that the decoder does too).
    HCLEN = 5 adds symbol 8: 256 codes of 8 bits and no distance code."""
    ll = [8] * 255 + [0, 8]
    data = rnd_bytes(700, 9)
    data = bytes(b if b != 255 else 0 for b in data)
    w = dc.BitWriter()
    cl = [0] * 19
    cl[8] = 1; cl[0] = 2; cl[16] = 2
    dc.dynamic_block(w, list(data), ll, [0], final=True, hclen=5, cl_lengths=cl, use17=False, use18=False)
    return finish(w, data)


def hclen_4_stream():
    """Not a case (zlib rejects it): HCLEN = 4, every length zero."""
    w = dc.BitWriter()
    w.bits(1, 1); w.bits(2, 2); w.bits(0, 5); w.bits(0, 5); w.bits(0, 4)
    for l in (0, 0, 1, 1):                              # 16, 17, 18, 0: codes for 18 and 0
        w.bits(l, 3)
    w.code(1, 1); w.bits(127, 7); w.code(1, 1); w.bits(120 - 11, 7)          # symbol 18 (canonical code 1) twice: 138 + 120 = 258 zeros
    w.bits(0, 16)
    return w.getvalue()


# ---- block sequencing -----------------------------------------------------------------------------------------------------
@case(need(lambda st: st["blocks"] == [1, 0, 2]))
def empty_stored_block_between_dynamic_blocks_unaligned():
    for extra in range(8):
        w = dc.BitWriter()
        a = list(b"left side ") + [(5, 5)] + [33] * extra
        dc.dynamic_block(w, a)
        if w.bit_length % 8 in (0, 5):
            continue
        dc.stored_block(w, b"")
        b = [(4, 3)] + list(b" right side")
        dc.dynamic_block(w, b, final=True)
        exp = dc.expand(a)
        return finish(w, exp + dc.expand(b, exp))
    raise AssertionError("no unaligned variant")


@case(need(lambda st: st["blocks"] == [1, 1, 0]))
def stored_block_of_len_1():
    w = dc.BitWriter()
    dc.fixed_block(w, list(b"abc"))
    dc.stored_block(w, b"Z", final=True)
    return finish(w, b"abcZ")


@case(need(lambda st: (st["blocks"][0] == 1 and st["full_flushes"] == 65536 // K.FLUSH)))
def stored_block_fills_a_65536_byte_output():
    w = dc.BitWriter()
    dc.dynamic_block(w, [7])
    rest = rnd_bytes(65535, 10)
    dc.stored_block(w, rest, final=True)
    return finish(w, b"\x07" + rest)


@case(need(lambda st: st["blocks"] == [0, 3, 0]))
def empty_fixed_blocks_in_front_and_final_behind_data():
    w = dc.BitWriter()
    dc.fixed_block(w, [])
    dc.fixed_block(w, list(b"data") + [(8, 4)])
    dc.fixed_block(w, [], final=True)
    return finish(w, b"data" * 3)


@case(need(lambda st: (st["blocks"][2] == 200 and st["empty_dist_after_full"] > 0)))
def two_hundred_tiny_dynamic_blocks():
    """The tables are rebuilt 200 times; a block without any distance code follows one whose distance code was complete, and
    blocks with a single distance code follow both."""
    r = random.Random(12)
    w = dc.BitWriter()
    out = bytearray()
    for k in range(200):
        if k % 3 == 0:
            toks = [r.randrange(256) for _ in range(4)] + [(3 + r.randrange(6), 1 + r.randrange(2)) for _ in range(3)] + [(4, 3)]
            if len(out) > 600:
                toks.append((9, 513 + r.randrange(50)))
            dl = None
        elif k % 3 == 1:
            toks = [r.randrange(256) for _ in range(1 + r.randrange(6))]
            dl = [0]
        else:
            toks = [r.randrange(256), (5 + r.randrange(30), 1)]
            dl = [1]
        if k % 3 == 0:
            f = dc.token_freqs(toks)[1]
            dl = dc.lengths_from_freqs(f, 15)
        dc.dynamic_block(w, toks, None, dl, final=k == 199)
        out += dc.expand(toks, bytes(out))
    return finish(w, bytes(out))


@case(need(lambda st: (st["near_matches"] >= 2 and st["far_matches"] >= 2 and st["blocks"][0] == 1)))
def dynamic_block_reaches_into_stored_block_near_and_far():
    w = dc.BitWriter()
    hist = _history(w, 9000, 13)
    toks = [(100, 50), 1, (100, K.NEAR + 500), 2, (258, 9000 + 100 + 1 + 100 + 1), 3, (30, K.NEAR - 100)]
    dc.dynamic_block(w, toks, final=True)
    return finish(w, hist + dc.expand(toks, hist))


# ---- distances and the ring ------------------------------------------------------------------------------------------------
def ring_distances():
    return [1, 2, 63, 64, 65, 257, 258, 259, K.NEAR - 1, K.NEAR, K.NEAR + 1, K.RING - 1, K.RING, K.RING + 1, 32767, 32768]


_MATCH_LENGTHS = (3, 64, 65, 128, 129, 258)


def _reached_distances(st):
    ds = ring_distances()
    want_far = sum(1 for d in ds if d > K.NEAR) * len(_MATCH_LENGTHS)
    want_near = sum(1 for d in ds if d <= K.NEAR) * len(_MATCH_LENGTHS)
    far = st["far_matches"] + st["one_pass_far_matches"]
    near = st["near_matches"] + st["one_pass_matches"] - st["one_pass_far_matches"]
    assert far == want_far and near == want_near, (far, want_far, near, want_near)
    assert st["overlap_recip"] > 0 and st["overlap_sub"] > 0


@case(_reached_distances)
def every_edge_distance_at_every_edge_length():
    """Distances 1, 2, 63..65, 257..259, INF_NEAR - 1 .. + 1, 4095..4097, 32767, 32768 at lengths 3, 64, 65, 128, 129 and 258."""
    w = dc.BitWriter()
    hist = _history(w, 32768, 14)
    r = random.Random(15)
    toks = []
    for n in _MATCH_LENGTHS:
        for d in ring_distances():
            toks += [(n, d), r.randrange(256)]
    dc.dynamic_block(w, toks, final=True)
    return finish(w, hist + dc.expand(toks, hist))


@case(need(lambda st: (st["overlap_recip"] == 63 and st["overlap_sub"] == 7)))
def overlapping_matches_distance_1_to_70_length_258():
    toks = list(rnd_bytes(70, 16))
    for d in range(1, 71):
        toks += [(258, d), d]
    w = dc.BitWriter()
    dc.dynamic_block(w, toks, final=True)
    return finish(w, dc.expand(toks))


@case(need(lambda st: (st["far_matches"] >= 3 and st["near_matches"] >= 6 and st["full_flushes"] >= 8)))
def match_destination_straddles_flush_line_ring_wrap_and_output_end():
    """Matches (run, near, far) whose destination lies across every multiple of INF_FLUSH up to 9 (every other one the ring's wrap);
    the last match ends on the last byte of the output."""
    r = random.Random(17)
    toks, pos = [], 0
    dists = [1, 300, K.NEAR + 1]
    for k in range(1, 10):
        line = k * K.FLUSH
        start = line - (1 + r.randrange(257))
        while pos < start:
            toks.append(r.randrange(256)); pos += 1
        d = dists[k % 3]
        if d > pos:
            d = 1
        toks.append((258, d)); pos += 258
    toks.append((258, K.NEAR + 7))
    w = dc.BitWriter()
    dc.dynamic_block(w, toks, final=True)
    return finish(w, dc.expand(toks))


def _tight_far_slack():
    return K.NEAR + 1 - K.ROUND - (K.FLUSH - 1)


@case(need(lambda st: (st["far_matches"] == 1 and st["far_min_slack"] == _tight_far_slack())))
def far_match_source_ends_at_the_last_byte_the_flush_argument_allows():
    """The tightest far match the header's argument allows: a round that starts with INF_FLUSH - 1 unflushed bytes, puts out exactly
    INF_ROUND_BYTES, and ends in a match of length 258 at distance INF_NEAR + 1.  Its source ends
    INF_NEAR + 1 - INF_ROUND_BYTES - (INF_FLUSH - 1) bytes before the last flushed byte -- the slack the static_assert of
    rsqc_inflate.h keeps above zero."""
    w = dc.BitWriter()
    hist = _history(w, 2 * K.FLUSH + K.FLUSH - 1, 18)
    ll = [0] * 286
    ll[285] = 1; ll[284] = 2; ll[256] = 3; ll[120] = 3
    dl = [0] * 30
    dl[0] = 1; dl[dc.dist_symbol(K.NEAR + 1)[0]] = 1
    toks = [(258, 1), (258, 1), (K.ROUND - 3 * 258, 1), (258, K.NEAR + 1)]
    dc.dynamic_block(w, toks, ll, dl, final=True)
    return finish(w, hist + dc.expand(toks, hist))


@case(need(lambda st: (st["rounds"] == 1 and st["one_pass"] == 1 and st["one_pass_far"] == 1)))
def far_match_near_match_and_literals_in_a_one_pass_round():
    w = dc.BitWriter()
    hist = _history(w, 5000, 19)
    toks = [1, (10, 20), 2, (8, K.NEAR + 600), 3]
    dc.dynamic_block(w, toks, final=True)
    return finish(w, hist + dc.expand(toks, hist))


@case(need(lambda st: (st["rounds"] == 1 and st["one_pass"] == 0 and st["far_matches"] == 1 and st["near_matches"] == 1)))
def far_match_near_match_and_literals_in_one_round():
    w = dc.BitWriter()
    hist = _history(w, 5000, 20)
    toks = [1, (100, 20), 2, (100, K.NEAR + 600), 3]
    dc.dynamic_block(w, toks, final=True)
    return finish(w, hist + dc.expand(toks, hist))


@case(need(lambda st: (st["one_pass_dep"] == 1 and st["one_pass"] == 1 and st["rounds"] == 2)))
def match_reads_a_literal_of_its_own_round_beside_a_round_that_qualifies():
    """Block 1: a match at distance 3 behind three literals of the same round -- not a one-pass round.  Block 2: literals and a match
    that copies from before the round -- a one-pass round."""
    w = dc.BitWriter()
    hist = _history(w, 200, 21)
    a = [97, 98, 99, (3, 3)]
    b = [100, (10, 50), 101]
    dc.dynamic_block(w, a)
    dc.dynamic_block(w, b, final=True)
    e1 = dc.expand(a, hist)
    return finish(w, hist + e1 + dc.expand(b, hist + e1))


# ---- sizes -------------------------------------------------------------------------------------------------------------
def _sized(n):
    def reached(st):
        assert st["full_flushes"] == n // K.FLUSH and st["last_flush"] == n % K.FLUSH, (n, st["full_flushes"], st["last_flush"])

    def build():
        r = random.Random(n)
        words = [rnd_bytes(r.randrange(3, 40), n + k) for k in range(30)]
        data = b"".join(r.choice(words) for _ in range(n // 10 + 2))[:n]
        return dc.checked(dc.deflate_tokens(data, dc.Policy(chain=4)), data)
    build.__name__ = "output_of_%d_bytes" % n
    build.__doc__ = "An output of %d bytes: %d full flushes and a last piece of %d." % (n, n // K.FLUSH, n % K.FLUSH)
    CASES[build.__name__] = (build, reached)


for _n in (0, 1, K.FLUSH - 1, K.FLUSH, K.FLUSH + 1, K.RING, 65535, 65536):
    _sized(_n)


# ---- policies for whole BGZF blocks of real record bytes (tests/test_gpu_inflate_crafted.py) ---------------------------------
def _deepened(freqs, maxbits=15):
    """Code lengths for the used symbols with as many deep codes as the alphabet allows: frequencies replaced by powers of two in
    rank order (a comb), pushed under maxbits."""
    used = sorted((s for s in range(len(freqs)) if freqs[s]), key=lambda s: -freqs[s])
    f = [0] * len(freqs)
    for rank, s in enumerate(used):
        f[s] = 1 << max(0, 40 - rank)
    return dc.lengths_from_freqs(f, maxbits)


def encode_block(data, style):
    """One raw DEFLATE stream for `data` in one of BLOCK_STYLES, checked against zlib."""
    w = dc.BitWriter()
    if style == "stored" or not data:
        return dc.checked(dc.stored_stream(data), data)[0]
    if style == "far_only":
        toks = dc.tokenize(data, dc.Policy(min_dist=K.NEAR + 1, chain=6))
        dc.dynamic_block(w, toks, final=True)
    elif style == "near_edge":
        toks = dc.tokenize(data, dc.Policy(prefer=(K.NEAR, K.NEAR + 1, K.NEAR - 1), only_preferred=True))
        dc.dynamic_block(w, toks, final=True)
    elif style == "deep_codes":
        toks = dc.tokenize(data)
        fl, fd = dc.token_freqs(toks)
        dc.dynamic_block(w, toks, _deepened(fl), _deepened(fd) if sum(1 for x in fd if x) > 1 else ([1] if any(fd) else [0]), final=True, hclen=19)
    elif style == "tiny_blocks":
        toks = dc.tokenize(data)
        parts = [toks[o:o + 24] for o in range(0, len(toks), 24)]
        for k, part in enumerate(parts):
            dc.dynamic_block(w, part, final=k == len(parts) - 1)
    elif style == "stored_and_dynamic":
        half = len(data) // 2
        dc.stored_block(w, data[:half])
        dc.dynamic_block(w, dc.tokenize(data, start=half), final=True)
    elif style == "all_literal":
        dc.dynamic_block(w, list(data), None, [0], final=True, hlit=257, hdist=1)
    elif style == "fixed":
        dc.fixed_block(w, dc.tokenize(data), final=True)
    elif style == "long_matches":
        dc.dynamic_block(w, dc.tokenize(data, dc.Policy(min_len=20, chain=8)), final=True)
    elif style == "distance_64_up":
        dc.dynamic_block(w, dc.tokenize(data, dc.Policy(min_dist=64, prefer=(64, 65, 70, 100, 129, 200))), final=True)
    elif style == "one_bit_run":
        # a run of one byte: the byte, then matches at distance 1 with a 1-bit length code and the single distance code
        assert len(set(data)) == 1 and len(data) >= 4
        toks = [data[0]]
        left = len(data) - 1
        while left:
            n = min(258, left) if left - min(258, left) not in (1, 2) else min(258, left) - 3
            toks.append((n, 1)); left -= n
        fl, _fd = dc.token_freqs(toks)
        dc.dynamic_block(w, toks, None, [1], final=True)
    else:
        raise ValueError(style)
    return dc.checked(w.getvalue(), data)[0]


BLOCK_STYLES = ("far_only", "near_edge", "deep_codes", "tiny_blocks", "stored_and_dynamic", "all_literal", "fixed", "long_matches", "distance_64_up", "stored")

# inflated sizes of the blocks of a crafted file, in turn (11 sizes against 10 styles: every style meets every size)
BLOCK_SIZES = (65536, 1, 30000, K.RING + 1, 61000, K.FLUSH, 2 * K.FLUSH + 1, 12345, 50000, 777, 65535)
_RUN = re.compile(rb"(.)\1{59,}", re.S)


def crafted_bgzf_file(raw):
    """`raw` (the inflated bytes of a BAM or SAM file) as a BGZF file whose blocks have the sizes of BLOCK_SIZES and are each encoded
    in another of BLOCK_STYLES; every tenth block is followed by one that holds nothing but the next run of one byte (SEQ or QUAL of
    a synthetic record) under one-bit codes; the 28-byte empty block stands in the middle of the file (as `cat a.bam b.bam` leaves
    one) and at its end.  Returns (file bytes, [(style, inflated size)])."""
    out, log, p, k, eof_done = [], [], 0, 0, False

    def emit(data, style):
        stream = encode_block(data, style)
        if len(stream) + 26 > 65536:                    # does not fit a BGZF block this way: in two halves
            half = len(data) // 2
            emit(data[:half], style); emit(data[half:], style)
            return
        out.append(dc.bgzf_block(data, stream)); log.append((style, len(data)))

    while p < len(raw):
        size = min(BLOCK_SIZES[k % len(BLOCK_SIZES)], len(raw) - p)
        emit(raw[p:p + size], BLOCK_STYLES[k % len(BLOCK_STYLES)])
        p += size; k += 1
        if k % 10 == 5:
            m = _RUN.search(raw, p, p + 60000)
            if m:
                if m.start() > p:
                    emit(raw[p:m.start()], BLOCK_STYLES[k % len(BLOCK_STYLES)])
                emit(raw[m.start():m.end()], "one_bit_run")
                p = m.end()
        if not eof_done and p >= len(raw) // 2:
            out.append(dc.BGZF_EOF); log.append(("empty", 0)); eof_done = True
    out.append(dc.BGZF_EOF)
    return b"".join(out), log
