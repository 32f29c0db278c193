"""The contract of rsqc_markdup_umi_edits(1) (include/rnaseqc_amd.h; --umi-edits=1) in plain Python: the contract of
tests/markdup_umi_ref.py with ONE change -- the last component of an anchor's signature is the ROOT of its UMI inside its position set,
not the UMI itself -- and the figures of rsqc_markdup_umi_group_info.  Dicts per position set; nothing of the kernels is restated."""
import numpy as np

from rnaseqc_amd import abi
from tests import markdup_umi_ref as uref
from tests.markdup_umi_ref import assert_info_equal, assert_umi_info_equal  # noqa: F401

GROUP_FIELDS = ("umi_nodes", "merged_nodes", "exact_duplicate_fragments")


def bases(key: int) -> int:
    """The number of bases of a non-zero key: (1 << 2L) | bits."""
    return (key.bit_length() - 1) // 2


def neighbours(key: int):
    """The keys one substitution from a non-zero key: the same length, one base changed."""
    return [key ^ (x << (2 * j)) for j in range(bases(key)) for x in (1, 2, 3)] if key else []


def parents(count: dict) -> dict:
    """count: key -> anchors of ONE position set.  Returns key -> parent key for every node that has one."""
    out = {}
    for k, c in count.items():
        eligible = [p for p in neighbours(k) if p in count and count[p] >= 2 * c - 1 and (count[p] > c or (count[p] == c and p < k))]
        if eligible:
            out[k] = min(eligible, key=lambda p: (-count[p], p))        # the highest count; ties go to the smallest key
    return out


def mark_duplicates_umi_group(batches, use_qhash2=True):
    """batches: the collection in arrival order, every batch with a `umi` column.  Returns (verdicts, info, umi_info, group_info, roots):
    verdicts / info / umi_info as markdup_umi_ref.mark_duplicates_umi with the grouped signature, group_info the dict of GROUP_FIELDS,
    roots the dict arrival index of an anchor -> the root key of its UMI."""
    _v, exact_info, umi_info, detail = uref.mark_duplicates_umi(batches, use_qhash2)
    names, flags, mapq = [], [], []
    for b in batches:
        two = use_qhash2 and b.qhash2 is not None
        for i in range(b.n):
            names.append((int(b.qhash[i]), int(b.qhash2[i]) if two else 0))
            flags.append(int(b.flag[i])); mapq.append(int(b.mapq[i]))
    position_sets = {}                                  # position signature -> {key: [arrival index]}
    for idx, sig in detail["signatures"].items():
        position_sets.setdefault(sig[:-1], {}).setdefault(sig[-1], []).append(idx)
    roots, sets, nodes, merged = {}, {}, 0, 0
    for position, by_key in position_sets.items():
        up = parents({k: len(m) for k, m in by_key.items()})
        assert 0 not in up and 0 not in up.values()
        nodes += len(by_key); merged += len(up)
        for k, members in by_key.items():
            r, steps = k, 0
            while r in up:
                r = up[r]; steps += 1
                assert steps < len(by_key)              # the relation is acyclic
            for idx in members:
                roots[idx] = r
                sets.setdefault(position + (r,), []).append(idx)
    dup_names, n_dup = set(), 0
    for members in sets.values():
        best = max(members, key=lambda i: (mapq[i], -i))             # the highest mapq; ties keep the earliest arrival
        for idx in members:
            if idx != best:
                dup_names.add(names[idx]); n_dup += 1
    verdict = np.array([1 if nm in dup_names else 0 for nm in names], np.uint8)
    fl = np.array(flags, np.int64)
    info = dict(exact_info, sets=len(sets), duplicate_fragments=n_dup, flagged_records=int(verdict.sum()),
                cleared_records=int((((fl & abi.FDUP) != 0) & (verdict == 0)).sum()))
    group = dict(umi_nodes=nodes, merged_nodes=merged, exact_duplicate_fragments=info["anchors"] - nodes)
    assert group["exact_duplicate_fragments"] == exact_info["duplicate_fragments"]
    assert n_dup == group["exact_duplicate_fragments"] + merged
    assert umi_info["position_duplicate_fragments"] >= n_dup >= group["exact_duplicate_fragments"]
    return verdict, info, umi_info, group, roots


def assert_group_info_equal(got, want):
    for f in GROUP_FIELDS:
        assert int(got[f]) == int(want[f]), (f, int(got[f]), int(want[f]))
