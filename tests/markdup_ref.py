"""The contract of --mark-duplicates (include/rnaseqc_amd.h, rsqc_markdup_*) in plain numpy / Python over rnaseqc_amd.model.Batch
lists: the executable form the tests compare against, bit for bit.  Nothing of the kernels' machinery is restated here (no slots,
no sort, no table): anchors, signatures, sets, survivors, names."""
import copy

import numpy as np

from rnaseqc_amd import abi

M32 = 0xFFFFFFFF
EXCLUDED = abi.FUNMAP | abi.FSECONDARY | abi.FQCFAIL | abi.FSUPP
SINGLE, PAIR, SPLIT = 0, 1, 2
INFO_FIELDS = ("records", "population", "anchors", "sets", "duplicate_fragments", "flagged_records", "cleared_records")
ORDER_FREE_FIELDS = ("anchors", "sets", "duplicate_fragments")


def _to_i32(u):
    u &= M32
    return u - (1 << 32) if u & 0x80000000 else u


def u5(pos, flag, ops):
    """The unclipped 5' coordinate (signed 32 bits, wrapped) of a record with the packed operations `ops`."""
    u = int(pos) & M32
    if not flag & abi.FREVERSE:
        for op in ops:
            if (int(op) & 15) not in (abi.CIG_S, abi.CIG_H):
                break
            u = (u - (int(op) >> 4)) & M32
        return _to_i32(u)
    k = len(ops)
    while k > 0 and (int(ops[k - 1]) & 15) in (abi.CIG_S, abi.CIG_H):
        u += int(ops[k - 1]) >> 4
        k -= 1
    for op in ops[:k]:
        if (int(op) & 15) in (abi.CIG_M, abi.CIG_D, abi.CIG_N, abi.CIG_EQ, abi.CIG_X):
            u += int(op) >> 4
    return _to_i32(u)


def _operations(b, i):
    n = int(b.n_cigar[i])
    if n == abi.NCIGAR_ESCAPE:
        k = np.flatnonzero(np.asarray(b.wide_index) == i)
        n = int(b.wide_n_cigar[k[0]]) if len(k) else 0
    off = int(b.cigar_off[i])
    return b.cigar[off:min(off + n, len(b.cigar))]


def classify(flag, tagbits, pos, mpos):
    """(kind, is_anchor) of a population record."""
    if not flag & abi.FPAIRED or flag & abi.FMUNMAP:
        return SINGLE, True
    if tagbits & abi.TB_MTID_SAME:
        return PAIR, pos < mpos or (pos == mpos and bool(flag & abi.FREAD1))
    return SPLIT, bool(flag & abi.FREAD1)


def mark_duplicates(batches, use_qhash2=True):
    """batches: the collection in arrival order.  Returns (verdicts: uint8 per record in arrival order, info: dict of INFO_FIELDS,
    detail: dict with `signatures` (arrival index of every anchor -> signature) and `survivors` (signature -> arrival index))."""
    names, flags = [], []
    sets = {}                                          # signature -> [(arrival index, mapq)]
    signatures = {}
    population = 0
    at = 0
    for b in batches:
        if b.n == 0:
            continue
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
            sig = (int(tid[i]), u5(int(b.pos[i]), flag, _operations(b, i)), 1 if flag & abi.FREVERSE else 0,
                   1 if (kind != SINGLE and flag & abi.FMREVERSE) else 0, kind, w)
            sets.setdefault(sig, []).append((at + i, int(b.mapq[i])))
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
    return verdict, info, dict(signatures=signatures, survivors=survivors)


def rewrite_flags(batches, verdict):
    """Copies of the batches with flag 0x400 of every record replaced by its verdict."""
    out, at = [], 0
    for b in batches:
        nb = copy.copy(b)
        v = verdict[at:at + b.n].astype(np.uint16)
        nb.flag = ((np.asarray(b.flag, np.uint16) & np.uint16(~abi.FDUP & 0xFFFF)) | (v * np.uint16(abi.FDUP))).astype(np.uint16)
        out.append(nb); at += b.n
    assert at == len(verdict)
    return out


def assert_info_equal(got, want):
    for f in INFO_FIELDS:
        assert int(got[f]) == int(want[f]), (f, int(got[f]), int(want[f]))
