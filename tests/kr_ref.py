"""Reference of the Read Length stage KR (src/RNASeQC.cpp:275-278): a literal restatement, record by record, no cleverness.

    for each record in FILE order that reaches :275:
        if span(record) > readLength: readLength = l_qseq(record)

Records are the dicts of model.Batch.from_records.  `span` is the CIGAR's reference length (M, D, N, =, X), or 1 when that is 0 -- a record
without operations, or one of only S and I: the bam_endpos rule.  A record reaches :275 when it is not secondary, not QC-fail, not
supplementary and mapped; under --legacy its span must also be at most 100 000 (:276, LEGACY_MAX_READ_LENGTH).

The library keeps, per batch or file range, the TRANSFER FUNCTION of that walk (include/rnaseqc_amd.h, rsqc_shard_info): keys = the prefix
maxima of span over the eligible records, one final state per key; entered with state r the batch leaves the state of the first key above r,
and r itself when there is none."""
import numpy as np

from rnaseqc_amd import abi

REF_OPS = (abi.CIG_M, abi.CIG_D, abi.CIG_N, abi.CIG_EQ, abi.CIG_X)
QUERY_OPS = (abi.CIG_M, abi.CIG_I, abi.CIG_S, abi.CIG_EQ, abi.CIG_X)
LEGACY_MAX_READ_LENGTH = 100000
NO_LENGTH = 0xFFFFFFFF                                   # the armed minimum: no eligible record


def span(rec):
    n = sum(int(ln) for op, ln in rec.get("cigar", []) if op in REF_OPS)
    return n if n else 1


def l_qseq(rec):
    if "l_qseq" in rec:
        return int(rec["l_qseq"])
    return sum(int(ln) for op, ln in rec.get("cigar", []) if op in QUERY_OPS)


def eligible(rec, legacy=False):
    fl = int(rec.get("flag", 0))
    if fl & (abi.FSECONDARY | abi.FQCFAIL | abi.FSUPP | abi.FUNMAP):
        return False
    return not (legacy and span(rec) > LEGACY_MAX_READ_LENGTH)


def inputs(records, legacy=False):
    """(span, l_qseq) of the eligible records, file order"""
    return [(span(r), l_qseq(r)) for r in records if eligible(r, legacy)]


def state_machine(records, r0=0, legacy=False):
    r = int(r0)
    for s, q in inputs(records, legacy):
        if s > r:
            r = q
    return r


def monotone(records, r0=0, legacy=False):
    """the same walk with a state that never goes down: what an implementation that forgets the lowering computes"""
    r = int(r0)
    for s, q in inputs(records, legacy):
        if s > r:
            r = max(r, q)
    return r


def transfer_table(records, legacy=False):
    """(keys, states): the prefix maxima of span, and for each the final state of the walk that starts by firing it"""
    sq = inputs(records, legacy)
    keys, states, cur = [], [], 0
    for i, (s, q) in enumerate(sq):
        if s > cur:
            cur = s
            r = q
            for s2, q2 in sq[i + 1:]:
                if s2 > r:
                    r = q2
            keys.append(s); states.append(r)
    return keys, states


def apply_table(table, r):
    keys, states = table
    for k, v in zip(keys, states):
        if k > r:
            return v
    return r


def compose(tables, r0=0):
    """tables in FILE order, from state r0"""
    r = int(r0)
    for t in tables:
        r = apply_table(t, r)
    return r


def extremes(records, legacy=False):
    """(max span, min l_qseq, max l_qseq) of the eligible records; (0, NO_LENGTH, 0) when there is none"""
    sq = inputs(records, legacy)
    if not sq:
        return (0, NO_LENGTH, 0)
    return (max(s for s, _ in sq), min(q for _, q in sq), max(q for _, q in sq))


def tile_spans(records, legacy=False):
    """the largest eligible span of every tile of 64 records (0: none)"""
    return [max([span(r) for r in records[t:t + 64] if eligible(r, legacy)] + [0]) for t in range(0, len(records), 64)]


def check_distributed(parts, legacy=False):
    """rnaseqc_amd.distributed's restatement (read_length_transfer, compose_read_length) against the functions above.
    parts: [(file index, records)] in any order -- the batches or ranges of a file.  Returns the composed value."""
    from rnaseqc_amd import distributed
    infos, tables = [], []
    for k, (fi, recs) in enumerate(parts):
        sq = inputs(recs, legacy)
        keys, states = distributed.read_length_transfer([s for s, _ in sq], [q for _, q in sq])
        want = transfer_table(recs, legacy)
        assert [int(x) for x in keys] == want[0] and [int(x) for x in states] == want[1], (k, fi)
        tables.append((fi, want))
        infos.append(distributed.ShardInfo(np.array([fi], np.uint64), np.array([len(recs)], np.uint64), np.array([0, len(keys)], np.uint32), keys, states,
                                           np.zeros(0, np.uint64), np.zeros(0, np.uint32)))
    want = compose([t for _, t in sorted(tables, key=lambda x: x[0])])
    assert distributed.compose_read_length(infos) == want == distributed.compose_read_length(infos[::-1])
    in_order = [r for _, recs in sorted(parts, key=lambda x: x[0]) for r in recs]
    assert want == state_machine(in_order, 0, legacy)
    return want
