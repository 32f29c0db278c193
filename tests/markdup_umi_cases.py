"""Inputs shared by the tests of UMI-aware duplicate marking (CPU emulation, C ABI on the GPU, command line): the catalogue of crafted
collections and the seeded fixture, on top of tests/markdup_cases.py's builders.  A record carries its UMI as text under "umi" (absent
= no UMI: key 0).  Expected verdicts and figures come from tests/markdup_umi_ref.py; what a reader can check by hand is asserted here."""
import copy
import functools

import numpy as np

from rnaseqc_amd import abi
from rnaseqc_amd.model import Batch
from tests import markdup_cases as mc
from tests import markdup_ref as ref
from tests import markdup_umi_ref as uref
from tests.markdup_cases import single, pair, split

CONTIGS = mc.CONTIGS


def with_umi(recs, umi):
    """The records (one dict or a list) with the UMI text `umi` (a list: one per record)."""
    recs = [recs] if isinstance(recs, dict) else list(recs)
    umis = umi if isinstance(umi, (list, tuple)) else [umi] * len(recs)
    assert len(umis) == len(recs)
    return [dict(r, umi=u) for r, u in zip(recs, umis)]


def to_batch(recs):
    b = Batch.from_records(recs)
    b.umi = np.array([uref.umi_pack(r.get("umi", "")) for r in recs], np.uint64)
    return b


def _text(k, length=8):
    """UMI number k as `length` bases (k in base 4, the first base most significant)."""
    return "".join("ACGT"[(k >> (2 * (length - 1 - j))) & 3] for j in range(length))


def crafted():
    """name -> list of batches, each a list of records in arrival order"""
    c = {}
    c["same_signature_other_umi"] = [with_umi(single("a", 100), "ACGTACGT") + with_umi(single("b", 100), "ACGTACGA")]
    # the same signature and UMI with mapq 10, 30, 20, and an anchor of another UMI (mapq 25) between them: with the UMI sorted BELOW
    # the mapq byte the order would be b(30) x(25) c(20) a(10) -- the set of a, b, c is torn apart
    c["mapq_interleaved_with_other_umi"] = [with_umi(single("a", 100, mapq=10), "AAAA") + with_umi(single("b", 100, mapq=30), "AAAA") + with_umi(single("x", 100, mapq=25), "CCCC") +
                                            with_umi(single("c", 100, mapq=20), "AAAA")]
    c["umis_differ_in_the_top_base"] = [with_umi(single("a", 100), "ACGTACGTAC") + with_umi(single("b", 100), "CCGTACGTAC") + with_umi(single("c", 100), "ACGTACGTAC")]
    c["umis_differ_in_the_last_base"] = [with_umi(single("a", 100), "ACGTACGTAC") + with_umi(single("b", 100), "ACGTACGTAG") + with_umi(single("c", 100), "ACGTACGTAG")]
    long_umi = "ACGT" * 7 + "ACG"
    c["lengths_1_and_31_in_one_set"] = [with_umi(single("a", 100), "A") + with_umi(single("b", 100), long_umi) + with_umi(single("c", 100), "A") + with_umi(single("d", 100), long_umi) +
                                        with_umi(single("e", 100), "AA") + with_umi(single("f", 100), long_umi[:30])]
    c["key_0_mixed_with_keyed"] = [[single("a", 100)] + with_umi(single("b", 100), "ACGT") + [single("c", 100)] + with_umi(single("d", 100), "ACNT") + with_umi(single("e", 100), "ACGT") +
                                   with_umi(single("f", 100), "ACGT" * 8)]
    # pairs at one position: p0 and p1 agree in the ANCHOR's UMI (the forward record at pos1) and differ in the mate's; p2's anchor differs
    c["anchor_umi_counts_not_the_mates"] = [with_umi(pair("p0", 100, 300), ["AAAA", "CCCC"]) + with_umi(pair("p1", 100, 300), ["AAAA", "GGGG"]) + with_umi(pair("p2", 100, 300), ["TTTT", "CCCC"])]
    kinds = []
    for k in range(2):
        kinds += with_umi(single("s%d" % k, 100), "ACGT") + with_umi(pair("p%d" % k, 100, 300), "ACGT") + with_umi(split("x%d" % k, 0, 100, 1, 300), "ACGT")
    c["kinds_share_position_and_umi"] = [kinds]
    c["no_anchors"] = [with_umi(single("a", 100, flag=abi.FSECONDARY), "ACGT") + with_umi(single("b", 100, flag=abi.FUNMAP), "ACGT") + with_umi(single("c", 100, tid=-1), "ACGT")]
    c["no_records"] = [[]]
    for n in (255, 256, 257):
        c["one_signature_%d_anchors_3_umis" % n] = [[r for i in range(n) for r in with_umi(single("m%d" % i, 100, mapq=(i * 7) % 61), ("ACGTAC", "ACGTAG", "TCGTAC")[i % 3])] +
                                                    with_umi(single("z", 5000), "ACGTAC")]
    recs = [r for i in range(12) for r in with_umi(single("t%d" % i, 100, mapq=(40, 10, 60, 20)[i % 4]), ("GATTACA", "GATTACC")[i % 2])]
    c["one_signature_across_three_batches"] = [recs[:5], recs[5:6], recs[6:]]
    recs = []
    for i in range(40):
        recs += with_umi(single("e%d" % i, 100 + 10 * (i % 7), mapq=i % 5), "ACGTACGT")
    c["all_umis_equal"] = [recs]
    recs = []
    for i in range(40):
        recs += with_umi(single("d%d" % i, 100 + 10 * (i % 7), mapq=i % 5), _text(i))
    c["all_umis_distinct"] = [recs]
    return c


CRAFTED_NAMES = ["same_signature_other_umi", "mapq_interleaved_with_other_umi", "umis_differ_in_the_top_base", "umis_differ_in_the_last_base", "lengths_1_and_31_in_one_set",
                 "key_0_mixed_with_keyed", "anchor_umi_counts_not_the_mates", "kinds_share_position_and_umi", "no_anchors", "no_records",
                 "one_signature_255_anchors_3_umis", "one_signature_256_anchors_3_umis", "one_signature_257_anchors_3_umis", "one_signature_across_three_batches",
                 "all_umis_equal", "all_umis_distinct"]


@functools.lru_cache(maxsize=None)
def _crafted_cached():
    return crafted()


@functools.lru_cache(maxsize=None)
def crafted_case(name):
    """(batches, verdicts, info, umi_info)"""
    parts = _crafted_cached()[name]
    batches = [to_batch(p) for p in parts]
    v, info, uinfo, _detail = uref.mark_duplicates_umi(batches)
    recs = [r for p in parts for r in p]
    flagged = [r["qname"] for r, x in zip(recs, v) if x]
    # what plain --mark-duplicates calls on the same collection
    assert uinfo["position_duplicate_fragments"] == ref.mark_duplicates(batches)[1]["duplicate_fragments"]
    assert uinfo["anchors_with_umi"] + uinfo["anchors_without_umi"] == info["anchors"]
    if name == "same_signature_other_umi":
        assert not flagged and info["sets"] == 2 and uinfo["position_duplicate_fragments"] == 1
    if name == "mapq_interleaved_with_other_umi":
        assert flagged == ["a", "c"] and info["sets"] == 2
    if name == "umis_differ_in_the_top_base":
        assert flagged == ["c"]
    if name == "umis_differ_in_the_last_base":
        assert flagged == ["c"]
    if name == "lengths_1_and_31_in_one_set":
        assert flagged == ["c", "d"] and info["sets"] == 4
    if name == "key_0_mixed_with_keyed":
        # a, c, d (an N) and f (32 bases) have key 0 and form ONE set; b and e another
        assert flagged == ["c", "d", "e", "f"] and info["sets"] == 2 and uinfo["anchors_with_umi"] == 2 and uinfo["anchors_without_umi"] == 4
    if name == "anchor_umi_counts_not_the_mates":
        assert flagged == ["p1", "p1"] and info["sets"] == 2
    if name == "kinds_share_position_and_umi":
        assert info["anchors"] == 6 and info["sets"] == 3 and flagged == ["s1", "p1", "p1", "x1", "x1"]
    if name == "no_anchors":
        assert info["anchors"] == 0 and info["records"] == 3 and not flagged
    if name == "no_records":
        assert info["records"] == 0
    if name.startswith("one_signature_2"):
        n = int(name.split("_")[2])
        assert info["anchors"] == n + 1 and info["sets"] == 4 and info["duplicate_fragments"] == n - 3 and uinfo["position_duplicate_fragments"] == n - 1
    if name == "one_signature_across_three_batches":
        assert info["sets"] == 2 and info["duplicate_fragments"] == 10 and "t2" not in flagged and "t0" in flagged      # t2: the first mapq 60 of GATTACA
    if name == "all_umis_equal":
        assert info["duplicate_fragments"] == uinfo["position_duplicate_fragments"] == 33
    if name == "all_umis_distinct":
        assert info["duplicate_fragments"] == 0 and uinfo["position_duplicate_fragments"] == 33
    return batches, v, info, uinfo


# ---- the seeded fixture: the first FIXTURE_N records of markdup_cases.fixture() with seeded UMIs ----------------------------------------
FIXTURE_N = 3200
FIXTURE_CUTS = [0, 300, 1100, 1250, 2900, FIXTURE_N]
UMI_POOL = 4                                           # UMIs per position signature: small, so that equal UMIs meet at one position


@functools.lru_cache(maxsize=None)
def fixture_umi_text():
    """One 10-base UMI per FRAGMENT NAME of the fixture (mates and the secondary records that carry the name share it): drawn from
    UMI_POOL texts, a few names without a usable UMI (an N)."""
    b = mc.fixture().slice(0, FIXTURE_N)
    r = np.random.default_rng(4242)
    pool = [_text(int(r.integers(0, 1 << 20)), 10) for _ in range(UMI_POOL)]
    by_name, out = {}, []
    for i in range(b.n):
        nm = bytes(b.qname[int(b.qname_off[i]):int(b.qname_off[i + 1])]).decode()
        if nm not in by_name:
            by_name[nm] = "ACGTNACGTA" if r.random() < 0.03 else pool[int(r.integers(0, UMI_POOL))]
        out.append(by_name[nm])
    return out


@functools.lru_cache(maxsize=None)
def fixture():
    b = copy.copy(mc.fixture().slice(0, FIXTURE_N))
    b.umi = np.array([uref.umi_pack(t) for t in fixture_umi_text()], np.uint64)
    return b


@functools.lru_cache(maxsize=None)
def fixture_expected():
    out = uref.mark_duplicates_umi([fixture()])
    v, info, uinfo, _ = out
    # the fixture exercises what it is for: some position duplicates are rescued by their UMI, some stay, some anchors have no UMI
    assert 0 < info["duplicate_fragments"] < uinfo["position_duplicate_fragments"] and uinfo["anchors_without_umi"] > 0
    return out


@functools.lru_cache(maxsize=None)
def fixture_shuffled():
    """The fixture in another arrival order, in three unequal batches, with what the reference says for THAT order."""
    b = fixture()
    parts = mc.cut(b.take(np.random.default_rng(177).permutation(b.n)), seed=178, parts=3)
    return parts, uref.mark_duplicates_umi(parts)
