"""The contract of UMI-aware duplicate marking (include/rnaseqc_amd.h, rsqc_markdup_use_umi / rsqc_umi_pack) in plain Python: the
contract of tests/markdup_ref.py with ONE change -- the anchor record's own UMI key is the last component of the signature -- and the
three figures of rsqc_markdup_umi_info.  Nothing of the kernels' machinery is restated here."""
import numpy as np

from rnaseqc_amd import abi
from tests.markdup_ref import EXCLUDED, PAIR, SINGLE, SPLIT, INFO_FIELDS, ORDER_FREE_FIELDS, _operations, assert_info_equal, classify, rewrite_flags, u5  # noqa: F401

UMI_FIELDS = ("anchors_with_umi", "anchors_without_umi", "position_duplicate_fragments")
_CODE = {ord("A"): 0, ord("C"): 1, ord("G"): 2, ord("T"): 3, ord("a"): 0, ord("c"): 1, ord("g"): 2, ord("t"): 3}


def umi_pack(umi) -> int:
    """The key of a UMI (str or bytes): 2 bits per base, the first base most significant, '-' and '+' skipped, (1 << 2L) | bits;
    0 when nothing is left, on any other byte, or on more than 31 bases."""
    s = umi.encode("latin-1") if isinstance(umi, str) else bytes(umi)
    bits, n = 0, 0
    for b in s:
        if b in (0x2D, 0x2B):
            continue
        if b not in _CODE:
            return 0
        n += 1
        if n > 31:
            return 0
        bits = bits * 4 + _CODE[b]
    return (1 << (2 * n)) + bits if n else 0


def qname_umi(name, sep="_") -> int:
    """The key of the UMI behind the last `sep` of a read name; 0 without a separator or with nothing behind it."""
    s = name.encode("latin-1") if isinstance(name, str) else bytes(name)
    k = s.rfind(sep.encode("latin-1") if isinstance(sep, str) else sep)
    return umi_pack(s[k + 1:]) if k >= 0 else 0


def mark_duplicates_umi(batches, use_qhash2=True):
    """batches: the collection in arrival order, every batch with a `umi` column.  Returns (verdicts, info, umi_info, detail):
    verdicts / info / detail as markdup_ref.mark_duplicates, umi_info the dict of UMI_FIELDS."""
    names, flags = [], []
    sets, position_sets = {}, {}                       # signature (with / without the UMI) -> [(arrival index, mapq)]
    signatures = {}
    population = with_umi = 0
    at = 0
    for b in batches:
        if b.n == 0:
            continue
        assert b.umi is not None and len(b.umi) == b.n
        tid = b.tid_per_record() if len(b.seg_tid) else np.full(b.n, -1, np.int32)
        two = use_qhash2 and b.qhash2 is not None
        for i in range(b.n):
            flag = int(b.flag[i])
            names.append((int(b.qhash[i]), int(b.qhash2[i]) if two else 0))
            flags.append(flag)
            if flag & EXCLUDED or int(tid[i]) < 0:
                continue
            population += 1
            kind, anchor = classify(flag, int(b.tagbits[i]), int(b.pos[i]), int(b.mpos[i]))
            if not anchor:
                continue
            w = int(b.isize[i]) if kind == PAIR else int(b.mpos[i]) if kind == SPLIT else 0
            position = (int(tid[i]), u5(int(b.pos[i]), flag, _operations(b, i)), 1 if flag & abi.FREVERSE else 0,
                        1 if (kind != SINGLE and flag & abi.FMREVERSE) else 0, kind, w)
            key = int(b.umi[i])                        # the anchor's own key; the mate's is never consulted
            with_umi += 1 if key else 0
            sig = position + (key,)
            sets.setdefault(sig, []).append((at + i, int(b.mapq[i])))
            position_sets.setdefault(position, []).append(at + i)
            signatures[at + i] = sig
        at += b.n
    dup_names, survivors, n_dup = set(), {}, 0
    for sig, members in sets.items():
        best = max(members, key=lambda m: (m[1], -m[0]))            # the highest mapq; ties keep the earliest arrival
        survivors[sig] = best[0]
        for idx, _ in members:
            if idx != best[0]:
                dup_names.add(names[idx]); n_dup += 1
    verdict = np.array([1 if nm in dup_names else 0 for nm in names], np.uint8)
    fl = np.array(flags, np.int64)
    info = dict(records=len(names), population=population, anchors=len(signatures), sets=len(sets), duplicate_fragments=n_dup,
                flagged_records=int(verdict.sum()), cleared_records=int((((fl & abi.FDUP) != 0) & (verdict == 0)).sum()))
    umi_info = dict(anchors_with_umi=with_umi, anchors_without_umi=len(signatures) - with_umi,
                    position_duplicate_fragments=len(signatures) - len(position_sets))
    return verdict, info, umi_info, dict(signatures=signatures, survivors=survivors)


def assert_umi_info_equal(got, want):
    for f in UMI_FIELDS:
        assert int(got[f]) == int(want[f]), (f, int(got[f]), int(want[f]))
