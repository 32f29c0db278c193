"""Inputs shared by the tests of UMI grouping (rsqc_markdup_umi_edits(1), --umi-edits=1; CPU emulation, C ABI on the GPU, command
line): crafted collections aimed at the rules of the contract -- the count threshold, the choice among several parents, chains, the
edges of the key, the bounds of a position set's node range -- and a seeded fixture whose UMI pool holds neighbours.  Built with
tests/markdup_umi_cases.py's helpers; expected values come from tests/markdup_umi_group_ref.py, and what a reader can check by hand is
asserted here.  All anchors of a case are single reads at one position with equal mapq unless the case says otherwise."""
import copy
import functools

import numpy as np

from tests import markdup_cases as mc
from tests import markdup_umi_cases as uc
from tests import markdup_umi_group_ref as gref
from tests import markdup_umi_ref as uref
from tests.markdup_cases import single, pair
from tests.markdup_umi_cases import with_umi, to_batch, _text

CONTIGS = mc.CONTIGS


def many(prefix, umi, n, pos=100, **kw):
    """n single reads prefix0 .. at one position with one UMI."""
    return [r for i in range(n) for r in with_umi(single("%s%d" % (prefix, i), pos, **kw), umi)]


def _reverse_at(name, u5, umi):
    """A reverse-strand single read of 50 M whose unclipped 5' end is u5."""
    return with_umi(single(name, u5 - 50, flag=mc.REV), umi)


LONG = "ACGT" * 7 + "ACG"                               # 31 bases: the key's top base sits in bits 60 and 61


def crafted():
    """name -> list of batches, each a list of records in arrival order"""
    c = {}
    c["threshold_3_2"] = [many("a", "ACGTACGT", 3) + many("b", "ACGTACGA", 2)]
    c["threshold_2_2"] = [many("a", "ACGTACGT", 2) + many("b", "ACGTACGA", 2)]
    c["threshold_4_3"] = [many("a", "ACGTACGT", 4) + many("b", "ACGTACGA", 3)]
    c["threshold_2_1"] = [many("a", "ACGTACGT", 2) + many("b", "ACGTACGA", 1)]
    # the larger key arrives first: the root is the smaller key, the survivor the earlier arrival -- an anchor of the CHILD
    c["ones_merge_to_smaller_key"] = [many("a", "AAAC", 1) + many("b", "AAAA", 1)]
    c["child_holds_the_survivor"] = [many("x", "GATTACA", 3, mapq=10) + many("y", "GATTACC", 1, mapq=60)]
    c["chain_9_5_3"] = [many("c", "AACC", 3) + many("a", "AAAA", 9) + many("b", "AAAC", 5)]
    c["two_parents_count_wins"] = [many("k", "AAAA", 1, mapq=60) + many("c", "CAAA", 5, mapq=10) + many("a", "AAAC", 3, mapq=10)]
    c["two_parents_key_breaks_tie"] = [many("k", "AAAA", 1, mapq=60) + many("c", "CAAA", 3, mapq=10) + many("a", "AAAC", 3, mapq=10)]
    # AAAC (257) - TAAC (449) - TAAA (448): the middle key is the largest.  TAAC takes the smaller of its two parents, TAAA (whose only
    # neighbour is the larger TAAC) stays a root
    c["count_one_chain_by_key"] = [many("y", "TAAA", 1) + many("m", "TAAC", 1) + many("x", "AAAC", 1)]
    c["top_base"] = [many("a", "ACGTACGT", 2) + many("b", "TCGTACGT", 1)]
    c["last_base"] = [many("a", "ACGTACGT", 2) + many("b", "ACGTACGA", 1)]
    c["length_1"] = [many("c", "C", 1) + many("a", "A", 2) + many("g", "G", 1) + many("t", "T", 1)]
    c["length_31"] = [many("a", LONG, 2) + many("b", "T" + LONG[1:], 1) + many("c", LONG[:-1] + "T", 1) + many("d", "TT" + LONG[2:], 1, pos=300) + many("e", LONG, 1, pos=300)]
    c["lengths_never_merge"] = [many("a", "ACGT", 3) + many("b", "ACG", 1) + many("c", "ACGTA", 1)]
    c["key_0_never_merges"] = [[single("n0", 100)] + many("a", "A", 1) + with_umi(single("n1", 100), "ACNT") + many("c", "C", 1) + with_umi(single("n2", 100), "ACGT" * 8) +
                               [single("n3", 100), single("n4", 100)]]
    # behind the set at (100, forward, SINGLE) come, in the sorted order, the sets of the other strand and the other kind at 100 and then
    # position 101; in front of it position 99.  Each holds a key one base from AAAA and AAAC, and none of them is in THEIR set
    c["neighbour_in_the_next_position_set"] = [many("a", "AAAA", 3) + many("c", "AAAC", 3) + many("g", "AAAG", 1, pos=101) + many("t", "AAAT", 1, pos=99) +
                                               many("d", "AAAA", 3, pos=500) + many("e", "AAAC", 3, pos=500) + _reverse_at("r", 500, "AAAG") + with_umi(pair("p", 500, 700), "AAAT") +
                                               many("h", "AAAA", 3, pos=900) + many("i", "AAAC", 3, pos=900) + many("j", "AAAG", 1, pos=901)]
    c["first_and_last_node_of_a_set"] = [many("a", "AAAA", 3) + many("b", "AAAC", 1) + many("c", "CCCC", 1) +
                                         many("d", "TTTT", 3, pos=300) + many("e", "TTTG", 1, pos=300) + many("f", "CCCC", 1, pos=300)]
    for n in (63, 64, 65, 255, 256, 257):
        c["set_of_%d_nodes" % n] = [[r for i in range(n) for r in many("m%d_" % i, _text((i * 37) % n if n % 37 else i, 5), 1)] + many("z", "ACGTA", 1, pos=5000)]
    recs = []
    for i in range(300):
        u = (i * 2654435761) % (1 << 16)
        recs += many("s%da" % i, _text(u, 8), 2 - i % 2, pos=1000 + 10 * i) + many("s%db" % i, _text(u ^ (1 + i % 3) << 2 * (i % 8), 8), 1, pos=1000 + 10 * i)
        if i % 3 == 0:
            recs += many("s%dc" % i, _text(u ^ 0x0505, 8), 2, pos=1000 + 10 * i)
    c["sets_straddle_workgroups"] = [recs]
    recs = [r for i in range(12) for r in with_umi(single("t%d" % i, 100, mapq=(40, 10, 60, 20)[i % 4]), ("GATTACA", "GATTACA", "GATTACC")[i % 3])]
    c["one_signature_across_three_batches"] = [recs[:5], recs[5:6], recs[6:]]
    return c


CRAFTED_NAMES = ["threshold_3_2", "threshold_2_2", "threshold_4_3", "threshold_2_1", "ones_merge_to_smaller_key", "child_holds_the_survivor", "chain_9_5_3", "two_parents_count_wins",
                 "two_parents_key_breaks_tie", "count_one_chain_by_key", "top_base", "last_base", "length_1", "length_31", "lengths_never_merge", "key_0_never_merges",
                 "neighbour_in_the_next_position_set", "first_and_last_node_of_a_set", "set_of_63_nodes", "set_of_64_nodes", "set_of_65_nodes", "set_of_255_nodes",
                 "set_of_256_nodes", "set_of_257_nodes", "sets_straddle_workgroups", "one_signature_across_three_batches"]


@functools.lru_cache(maxsize=None)
def _crafted_cached():
    return crafted()


@functools.lru_cache(maxsize=None)
def crafted_case(name):
    """(batches, verdicts, info, umi_info, group_info, roots)"""
    parts = _crafted_cached()[name]
    batches = [to_batch(p) for p in parts]
    v, info, uinfo, ginfo, roots = gref.mark_duplicates_umi_group(batches)
    _ev, exact, exact_uinfo, _ = uref.mark_duplicates_umi(batches)
    recs = [r for p in parts for r in p]
    flagged = [r["qname"] for r, x in zip(recs, v) if x]
    root_of = {recs[i]["qname"]: r for i, r in roots.items()}
    key = uref.umi_pack
    assert uinfo == exact_uinfo and ginfo["exact_duplicate_fragments"] == exact["duplicate_fragments"]
    assert info["duplicate_fragments"] == ginfo["exact_duplicate_fragments"] + ginfo["merged_nodes"]
    assert info["sets"] == exact["sets"] - ginfo["merged_nodes"]
    if name == "threshold_3_2":
        assert info["sets"] == 1 and info["duplicate_fragments"] == 4 and exact["sets"] == 2 and exact["duplicate_fragments"] == 3
        assert flagged == ["a1", "a2", "b0", "b1"]
    if name in ("threshold_2_2", "threshold_4_3"):
        assert ginfo["merged_nodes"] == 0 and info["sets"] == 2 and info == exact          # 2 < 3, 4 < 5
    if name == "threshold_2_1":
        assert ginfo["merged_nodes"] == 1 and flagged == ["a1", "b0"]
    if name == "ones_merge_to_smaller_key":
        assert root_of["a0"] == root_of["b0"] == key("AAAA") and flagged == ["b0"]           # a0, of the child AAAC, arrived first
    if name == "child_holds_the_survivor":
        assert flagged == ["x0", "x1", "x2"] and root_of["y0"] == key("GATTACA")
    if name == "chain_9_5_3":
        assert set(root_of.values()) == {key("AAAA")} and info["sets"] == 1 and ginfo["merged_nodes"] == 2 and info["duplicate_fragments"] == 16
    if name == "two_parents_count_wins":
        assert root_of["k0"] == key("CAAA") and flagged == ["c0", "c1", "c2", "c3", "c4", "a1", "a2"]
    if name == "two_parents_key_breaks_tie":
        assert key("AAAC") & 0xFF == 1 and key("CAAA") & 0xFF == 64
        assert root_of["k0"] == key("AAAC") and flagged == ["c1", "c2", "a0", "a1", "a2"]
    if name == "count_one_chain_by_key":
        assert key("TAAC") > key("TAAA") > key("AAAC")
        assert info["sets"] == 2 and root_of["m0"] == root_of["x0"] == key("AAAC") and root_of["y0"] == key("TAAA") and flagged == ["x0"]      # m0 arrived before x0
    if name in ("top_base", "last_base"):
        assert ginfo["merged_nodes"] == 1 and info["sets"] == 1 and flagged == ["a1", "b0"]
    if name == "length_1":
        assert set(root_of.values()) == {key("A")} and ginfo["merged_nodes"] == 3 and info["sets"] == 1
    if name == "length_31":
        assert key(LONG) >> 62 == 1 and key("T" + LONG[1:]) >> 60 == 7
        assert ginfo["merged_nodes"] == 2 and info["sets"] == 3 and root_of["b0"] == root_of["c0"] == key(LONG) and root_of["d0"] != root_of["e0"]
    if name == "lengths_never_merge":
        assert ginfo["merged_nodes"] == 0 and info["sets"] == 3
    if name == "key_0_never_merges":
        assert ginfo["umi_nodes"] == 3 and ginfo["merged_nodes"] == 1 and info["sets"] == 2 and uinfo["anchors_without_umi"] == 5
        assert [root_of[n] for n in ("n0", "n1", "n2", "n3", "n4")] == [0] * 5 and root_of["c0"] == key("A") and flagged == ["n1", "c0", "n2", "n3", "n4"]
    if name == "neighbour_in_the_next_position_set":
        assert ginfo["merged_nodes"] == 0 and ginfo["umi_nodes"] == 11 and info == exact
    if name == "first_and_last_node_of_a_set":
        assert root_of["b0"] == key("AAAA") and root_of["e0"] == key("TTTT") and ginfo["merged_nodes"] == 2 and info["sets"] == 4
    if name.startswith("set_of_"):
        n = int(name.split("_")[2])
        assert ginfo["umi_nodes"] == n + 1 and ginfo["exact_duplicate_fragments"] == 0 and 0 < ginfo["merged_nodes"] < n
    if name == "sets_straddle_workgroups":
        assert ginfo["umi_nodes"] == 700 and 0 < ginfo["merged_nodes"] <= 300
    if name == "one_signature_across_three_batches":
        # 8 GATTACA and 4 GATTACC (8 >= 7): one set; its survivor t2, the first mapq 60, is an anchor of the child
        assert info["sets"] == 1 and info["duplicate_fragments"] == 11 and "t2" not in flagged and exact["sets"] == 2
    return batches, v, info, uinfo, ginfo, roots


# ---- the seeded fixture: markdup_umi_cases' records with a UMI pool of two neighbour pairs, drawn unevenly -----------------------------
FIXTURE_N = uc.FIXTURE_N
FIXTURE_CUTS = uc.FIXTURE_CUTS
UMI_POOL = ("ACGTTGCAAC", "ACGTTGCAAT", "GGATCCTTAG", "GGTTCCTTAG")      # 0 - 1 and 2 - 3 are one base apart
UMI_SHARE = (0.45, 0.15, 0.3, 0.1)


@functools.lru_cache(maxsize=None)
def fixture_umi_text():
    """One UMI per FRAGMENT NAME of the fixture, a few names without a usable one (an N)."""
    b = mc.fixture().slice(0, FIXTURE_N)
    r = np.random.default_rng(2424)
    by_name, out = {}, []
    for i in range(b.n):
        nm = bytes(b.qname[int(b.qname_off[i]):int(b.qname_off[i + 1])]).decode()
        if nm not in by_name:
            by_name[nm] = "ACGTNACGTA" if r.random() < 0.03 else UMI_POOL[int(r.choice(4, p=UMI_SHARE))]
        out.append(by_name[nm])
    return out


@functools.lru_cache(maxsize=None)
def fixture():
    b = copy.copy(mc.fixture().slice(0, FIXTURE_N))
    b.umi = np.array([uref.umi_pack(t) for t in fixture_umi_text()], np.uint64)
    return b


@functools.lru_cache(maxsize=None)
def fixture_expected():
    out = gref.mark_duplicates_umi_group([fixture()])
    _v, info, uinfo, ginfo, _roots = out
    assert ginfo["merged_nodes"] > 0 and info["duplicate_fragments"] < uinfo["position_duplicate_fragments"] and uinfo["anchors_without_umi"] > 0
    return out


@functools.lru_cache(maxsize=None)
def fixture_shuffled():
    """The fixture in another arrival order, in three unequal batches, with what the reference says for THAT order."""
    b = fixture()
    parts = mc.cut(b.take(np.random.default_rng(277).permutation(b.n)), seed=278, parts=3)
    return parts, gref.mark_duplicates_umi_group(parts)
