"""CPU tests of the wave's DEFLATE decoder (rnaseqc_amd/csrc/rsqc_inflate.h, host build) on hand-built streams aimed at its
limits: the catalogue of tests/hostemu/inflate_cases.py, written by tests/hostemu/deflate_craft.py.  The reference is zlib's
inflate -- every stream passed it before the decoder sees it -- and every case proves, on the counters of the -DINF_STATS
build, that it reached the path it is named for.  The streams also run, clean and damaged, through the sanitized stand-alone
harness (tests/hostemu/inflate_fuzz.cpp --corpus)."""
import os
import struct
import subprocess
import zlib

import pytest

from rnaseqc_amd import bamio
from tests.hostemu import decode as emu
from tests.hostemu import deflate_craft as dc
from tests.hostemu import inflate_cases as ic
from tests.test_device_decode_host import _sanitized

_BUILT = {}


def _case(name):
    if name not in _BUILT:
        stream, expected = ic.CASES[name][0]()
        d = zlib.decompressobj(-15)                       # (deflate_craft.checked did this already; the reference is stated here once more)
        assert d.decompress(stream) == expected and d.unused_data == b"" and d.eof
        _BUILT[name] = (stream, expected)
    return _BUILT[name]


def test_limits_are_read_from_the_header():
    k = ic.K
    assert k.NEAR == k.RING - 258 and k.RING >= k.FLUSH + k.ROUND + 774
    assert len(ic.CASES) >= 35


@pytest.mark.parametrize("name", list(ic.CASES))
def test_crafted_stream_inflates_like_zlib_in_every_variant(name):
    stream, expected = _case(name)
    for variant in emu.VARIANTS:
        rc, out = emu.inflate(stream, len(expected), zlib.crc32(expected), variant)
        assert rc == 0 and out == expected, (name, variant, rc)


@pytest.mark.parametrize("name", list(ic.CASES))
def test_crafted_stream_reaches_its_path(name):
    """The counters of the stats build (the product's configuration): a case that did not go where it is named for fails."""
    stream, expected = _case(name)
    rc, out, st = emu.inflate_with_stats(stream, len(expected), zlib.crc32(expected))
    assert rc == 0 and out == expected
    ic.CASES[name][1](st)


def test_header_without_any_length_symbol_is_rejected():
    """HCLEN = 4 (lengths for 16, 17, 18 and 0 only) cannot spell a length above zero, so there is no valid block of that shape:
    zlib rejects it, and so does the decoder, in every variant."""
    stream = ic.hclen_4_stream()
    with pytest.raises(zlib.error):
        zlib.decompressobj(-15).decompress(stream)
    for variant in emu.VARIANTS:
        assert emu.inflate(stream, 0, 0, variant)[0] != 0, variant


def test_tokeniser_policies_and_block_styles():
    """The greedy tokeniser places matches where its policy says, and every block style of the GPU test's file inflates like zlib
    (encode_block checks that) and through the decoder."""
    r = ic.rnd_bytes(300, 1)
    data = (r + ic.rnd_bytes(40, 2, b"AC") + b"\xff" * 90 + b"\x11" * 40) * 30
    edge = [t for k, d in enumerate((ic.K.NEAR, ic.K.NEAR + 1, ic.K.NEAR - 1) * 3) for t in [(60, d)] + list(ic.rnd_bytes(10, 50 + k))]
    data += dc.expand(edge, data)                          # ... and repeats at the edge of the ring's reach
    toks = dc.tokenize(data, dc.Policy(min_dist=ic.K.NEAR + 1))
    assert dc.expand(toks) == data and any(isinstance(t, tuple) for t in toks) and all(t[1] > ic.K.NEAR for t in toks if isinstance(t, tuple))
    toks = dc.tokenize(data, dc.Policy(min_len=10, max_len=40, max_dist=500))
    assert dc.expand(toks) == data and all(10 <= t[0] <= 40 and t[1] <= 500 for t in toks if isinstance(t, tuple))
    toks = dc.tokenize(data, dc.Policy(prefer=(470,), force_at=(1000, 1003)))
    assert dc.expand(toks) == data
    at, starts = 0, {}
    for t in toks:
        starts[at] = t
        at += t[0] if isinstance(t, tuple) else 1
    assert isinstance(starts[1000], tuple) and starts[1000][0] == 3 and isinstance(starts[1003], tuple) and starts[1003][1] == 470
    for style in ic.BLOCK_STYLES:
        stream = ic.encode_block(data, style)
        rc, out, st = emu.inflate_with_stats(stream, len(data), zlib.crc32(data))
        assert rc == 0 and out == data, style
        if style == "far_only":
            assert st["far_matches"] + st["one_pass_far_matches"] > 0 and st["near_matches"] == 0 and st["one_pass_matches"] == st["one_pass_far_matches"]
        if style == "near_edge":
            assert st["near_matches"] + st["one_pass_matches"] > 0 and st["far_matches"] + st["one_pass_far_matches"] > 0
        if style == "deep_codes":
            assert st["long_ll"][15] > 0
        if style == "tiny_blocks":
            assert st["blocks"][2] >= 10
    run = b"\xff" * 3000
    rc, out, st = emu.inflate_with_stats(ic.encode_block(run, "one_bit_run"), len(run), zlib.crc32(run))
    assert rc == 0 and out == run and st["cuts"] > 0


def test_bgzf_writers_take_a_compress_callable(tmp_path):
    """bamio's BGZF writers with compress=: the same file bytes after gzip.decompress, and the default is unchanged."""
    import gzip
    data = b"some record bytes " * 500
    assert bamio._bgzf_block(data) == bamio._bgzf_block(data, 1, None)
    blk = bamio._bgzf_block(data, compress=lambda d: ic.encode_block(d, "tiny_blocks"))
    assert blk == dc.bgzf_block(data, ic.encode_block(data, "tiny_blocks")) and gzip.decompress(blk) == data
    assert dc.BGZF_EOF == bamio._EOF


def test_crafted_corpus_under_sanitizers(tmp_path):
    """Every stream of the catalogue, clean and under the harness's mutations, through the decoder built with the address and
    undefined-behaviour sanitizers as a stand-alone program: accesses to the ring, the tables and the output stay in bounds on
    these shapes too, and the verdicts are zlib's."""
    corpus = str(tmp_path / "crafted.corpus")
    with open(corpus, "wb") as f:
        for name in ic.CASES:
            stream, expected = _case(name)
            assert len(expected) <= 65536
            f.write(struct.pack("<III", len(stream), len(expected), zlib.crc32(expected)) + stream)
    for variant in ("", "all"):
        exe = _sanitized(tmp_path, "inflate_fuzz", ["-lz"], emu.VARIANTS[variant])
        r = subprocess.run([exe, "--corpus", corpus, "24", "3"], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        assert "corpus of %d streams" % len(ic.CASES) in r.stdout
