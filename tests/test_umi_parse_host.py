"""CPU: where a record's UMI comes from.  bam_parse_record and sam_parse_fields of the product (tests/hostemu/umi_emu.cpp) with the
tag source and the read-name source against the Python definition of the key (tests/markdup_umi_ref.py): the tag's place among the
aux fields, its types, a malformed aux tail, the separator's places in the name; the same alignments as SAM lines; no source
selected changes no other field; damaged records and lines under the sanitizers (tests/hostemu/umi_fuzz.cpp)."""
import os
import re
import struct
import subprocess

import pytest

from tests import markdup_umi_ref as uref
from tests.hostemu import umi as emu

U = "ACGTTGCAAC"
KEY = uref.umi_pack(U)
NM, CH, MD = ("NM", "i", 3), ("ch", "Z", "1"), ("MD", "Z", "10A9")

# name -> (aux list, expected key under --umi-tag=RX); every one is written as a BAM record AND as a SAM line
TAG_CASES = {
    "first": ([("RX", "Z", U), NM, CH], KEY),
    "middle": ([NM, ("RX", "Z", U), MD], KEY),
    "last": ([NM, MD, ("RX", "Z", U)], KEY),                        # (BAM: the value's NUL is the record's last byte)
    "only": ([("RX", "Z", U)], KEY),
    "absent": ([NM, MD], 0),
    "type_A": ([("RX", "A", "A"), NM], 0),
    "type_i": ([NM, ("RX", "i", 7)], 0),
    "type_B": ([("RX", "B", [1, 2, 3]), NM], 0),
    "twice_the_first_counts": ([("RX", "Z", U), NM, ("RX", "Z", "TTTT")], KEY),
    "first_of_two_is_no_Z": ([("RX", "i", 5), ("RX", "Z", U)], 0),   # the first field of that name counts, whatever its type
    "dual_umi": ([("RX", "Z", "ACGT-TGCA")], uref.umi_pack("ACGTTGCA")),
    "with_an_N": ([("RX", "Z", "ACGTNGCA")], 0),
    "lower_case": ([("RX", "Z", U.lower())], KEY),
    "31_bases": ([("RX", "Z", "ACGT" * 7 + "ACG")], uref.umi_pack("ACGT" * 7 + "ACG")),
    "32_bases": ([("RX", "Z", "ACGT" * 8)], 0),
    "another_tag_with_that_value": ([("RY", "Z", U), ("XR", "Z", U)], 0),
}


@pytest.mark.parametrize("name", sorted(TAG_CASES))
def test_tag_source_in_bam_and_sam(name):
    aux, want = TAG_CASES[name]
    emu.setup(emu.TAG, "RX")
    b = emu.parse_bam(emu.bam_record("read1", aux))
    s = emu.parse_sam(emu.sam_line("read1", aux))
    assert b["code"] == 0 and s["code"] == 0
    assert b["umi"] == want and s["umi"] == want
    for f in emu.FIELDS:
        assert b[f] == s[f], f                          # the same alignment: the same BamRecOut


def test_tag_is_empty_text():
    emu.setup(emu.TAG, "RX")
    assert emu.parse_bam(emu.bam_record("r", [("RX", "Z", "")]))["umi"] == 0
    assert emu.parse_bam(emu.bam_record("r", [("RX", "Z", "-")]))["umi"] == 0


def test_bam_malformed_aux_tails():
    emu.setup(emu.TAG, "RX")
    ok = emu.bam_aux([("RX", "Z", U)])
    # the tag's value ends exactly at the record end
    assert emu.parse_bam(emu.bam_record("r", raw_aux=ok))["umi"] == KEY
    # a Z value with no NUL before the record end: the field is cut off, no key -- and no byte behind the record is read
    r = emu.parse_bam(emu.bam_record("r", raw_aux=ok[:-1]))
    assert r["code"] == 0 and r["umi"] == 0
    assert emu.parse_bam(emu.bam_record("r", raw_aux=emu.bam_aux([emu_nm()]) + ok[:-1]))["umi"] == 0
    # a malformed field IN FRONT of the tag: the loop stops scanning there, as it does for NM
    broken_b = b"XBBc" + struct.pack("<I", 1000) + b"\x01\x02"                  # a B array that claims 1000 elements
    r = emu.parse_bam(emu.bam_record("r", raw_aux=broken_b + ok))
    assert r["code"] == 0 and r["umi"] == 0
    r = emu.parse_bam(emu.bam_record("r", raw_aux=b"XQ?" + ok))                 # an unknown type swallows the tail
    assert r["umi"] == 0
    r = emu.parse_bam(emu.bam_record("r", raw_aux=b"XZZnever ends " + ok.replace(b"\x00", b"")))
    assert r["umi"] == 0
    # two bytes of a third field behind the tag: the tag still counts
    assert emu.parse_bam(emu.bam_record("r", raw_aux=ok + b"NM"))["umi"] == KEY


def emu_nm():
    return NM


QNAME_CASES = [
    ("no_separator", "read1", "_", 0),
    ("separator_first", "_" + U, "_", KEY),
    ("separator_last", "read1_", "_", 0),
    ("several", "run_7_lane_" + U, "_", KEY),
    ("several_the_last_counts", "a_" + U + "_TTTT", "_", uref.umi_pack("TTTT")),
    ("two_in_a_row", "a__" + U, "_", KEY),
    ("colon_names", "M0:12:FC:1:1101:1000:2000:" + U, ":", KEY),
    ("colon_names_dual", "M0:12:FC:1:1101:1000:2000:ACGT+TGCA", ":", uref.umi_pack("ACGTTGCA")),
    ("other_separator_in_the_name", "a:b_" + U, ":", 0),                        # behind the last ':' comes "b_ACG...": no UMI
    ("254_bytes", "n" * (253 - len(U)) + "_" + U, "_", KEY),
    ("254_bytes_no_separator", "n" * 254, "_", 0),
    ("254_bytes_separator_first", "_" + "A" * 253, "_", 0),                     # 253 bases: too long
    ("separator_is_a_base", "xxA" + "CGTCGT", "A", uref.umi_pack("CGTCGT")),
    ("separator_is_a_base_inside_the_umi", "xx_ACGACG", "A", uref.umi_pack("CG")),
    ("one_byte_name_is_the_separator", "_", "_", 0),
    ("with_an_N", "r_ACGN", "_", 0),
]


@pytest.mark.parametrize("name,qname,sep,want", QNAME_CASES, ids=[c[0] for c in QNAME_CASES])
def test_qname_source_in_bam_and_sam(name, qname, sep, want):
    assert want == uref.qname_umi(qname, sep)
    emu.setup(emu.QNAME, sep=sep)
    for aux in ([], [NM, ("RX", "Z", "GGGG")]):          # (the tag is not the source: it changes nothing)
        b = emu.parse_bam(emu.bam_record(qname, aux))
        s = emu.parse_sam(emu.sam_line(qname, aux))
        assert b["code"] == 0 and s["code"] == 0 and b["qname_len"] == len(qname)
        assert b["umi"] == want and s["umi"] == want
        for f in emu.FIELDS:
            assert b[f] == s[f], f


def test_off_is_off():
    """With no source selected the key is 0 and every OTHER field is what it is with a source selected."""
    records = [(q, a) for q in ("read1", "run_7_" + U, "M0:1:" + U) for a, _ in TAG_CASES.values()]
    got = {}
    for source, sep in ((emu.NONE, "_"), (emu.TAG, "_"), (emu.QNAME, "_"), (emu.QNAME, ":")):
        emu.setup(source, "RX", sep)
        got[(source, sep)] = [(emu.parse_bam(emu.bam_record(q, a)), emu.parse_sam(emu.sam_line(q, a))) for q, a in records]
    off = got[(emu.NONE, "_")]
    assert all(b["umi"] == 0 and s["umi"] == 0 for b, s in off)
    keyed = 0
    for key, rows in got.items():
        for (b, s), (b0, s0) in zip(rows, off):
            for f in emu.FIELDS:
                assert b[f] == b0[f] and s[f] == s0[f], (key, f)
            keyed += 1 if b["umi"] else 0
    assert keyed > 20


def test_parsers_on_damaged_input_under_sanitizers(tmp_path):
    """60 000 damaged BAM records and SAM lines (tests/hostemu/umi_fuzz.cpp), each parsed from a buffer of exactly its size with each
    source selected, under the address / undefined-behaviour sanitizers.  A stand-alone program: nothing is loaded into Python."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "umi_fuzz")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(root, "tests", "hostemu", "umi_fuzz.cpp"), "-o", exe])
    r = subprocess.run([exe, "60000", "23"], capture_output=True, text=True, timeout=900, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and "60000 cases" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    parsed, refused, keyed = (int(x) for x in re.search(r"(\d+) parsed, (\d+) refused, (\d+) keyed", r.stdout).groups())
    assert parsed > 50_000 and refused > 5_000 and keyed > 10_000            # every outcome is exercised
