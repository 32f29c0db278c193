"""Named edge cases of the Read Length stage KR (rnaseqc_amd/csrc/rsqc_kr.h: read_length_kernel; its inputs from rsqc_k1.h and, under
--legacy, rsqc_kernels.hip; the compositions of rsqc_rl_compose.h and distributed.compose_read_length), after the pattern of k4_cases.py
and k5_cases.py.

A case is a FILE: segments of records (segment k lies on contig k of a small annotation, one gene per contig), and how the file reaches the
library -- `plain`: cut into batches at `cuts`; `ranges`: every segment is a file range (its first file index in `file_index`), submitted
once as one batch per range and once as ONE batch of ranges (Batch.concat_ranges); `shards`: the ranges dealt to several contexts.
Everything expected comes from tests/kr_ref.py.  Every case states the property it is named for as a `check` over the reference alone, run
when the catalogue is built: a case that drifts off its edge fails at import, not silently.

The constants the cases aim at: tiles of 64 records; groups of 64 tiles (one ballot of read_length_kernel: 4 096 records); 128 walks
(RSQC_RL_MAXP), lanes 0..63 twice (s0 / v0, then s1 / v1)."""
import numpy as np

from rnaseqc_amd import abi
from tests import kr_ref

M, I, D, N, S, H = abi.CIG_M, abi.CIG_I, abi.CIG_D, abi.CIG_N, abi.CIG_S, abi.CIG_H
TILE, GROUP, MAXP = 64, 64 * 64, 128
GENE_END = 100000
UNMAPPED, SECONDARY, QCFAIL, SUPPLEMENTARY = abi.FUNMAP, abi.FSECONDARY, abi.FQCFAIL, abi.FSUPP


def rec(span, lq, flag=0, **kw):
    """a record of reference span `span` and read length `lq` with a CIGAR that says both: spliced when the read is shorter than its span,
    soft-clipped when it is longer; lq == 0: the sequence is absent ('*')"""
    if lq == 0:
        cig, kw = [(M, span)], dict(kw, l_qseq=0)
    elif lq == span:
        cig = [(M, span)]
    elif lq > span:
        cig = [(S, lq - span), (M, span)]
    elif lq == 1:
        cig = [(M, 1), (N, span - 1)]
    else:
        cig = [(M, lq // 2), (N, span - lq), (M, lq - lq // 2)]
    r = dict(cigar=cig, flag=flag, mapq=255, nm=0)
    r.update(kw)
    assert kr_ref.span(r) == span and kr_ref.l_qseq(r) == lq
    return r


def ineligible(k, lq):
    """the four ways not to reach src/RNASeQC.cpp:275, by turns"""
    fl = (UNMAPPED, SECONDARY, SUPPLEMENTARY, QCFAIL)[k % 4]
    return dict(cigar=[] if fl == UNMAPPED else [(M, lq)], l_qseq=lq, flag=fl, mapq=255, nm=0)


def fillers(n, span=20, k0=0):
    """eligible records that never fire behind a state of `span` or more, of three lengths (so that the batch takes the general path)"""
    return [rec(span, span + 1 + (k0 + i) % 3) for i in range(n)]


def mixed(rng, n, lo=20, hi=60, bad=0.15):
    """spans and lengths from small overlapping ranges, the spans reaching a little higher (no length ends the walk): states go up and down;
    some records do not count"""
    out = []
    for i in range(n):
        if rng.random() < bad:
            out.append(ineligible(int(rng.integers(0, 4)), int(rng.integers(lo, hi + 1))))
        else:
            out.append(rec(int(rng.integers(lo, hi + 11)), int(rng.integers(lo, hi + 1))))
    return out


def _rng(name):
    return np.random.default_rng(int.from_bytes(name.encode(), "little") % (1 << 63))


class Case:
    def __init__(self, name, segs, mode="plain", cuts=(), legacy=False, file_index=None, shards=None, error=False, check=None, tags=(), emulate=True):
        assert mode in ("plain", "ranges") and 1 <= len(segs) <= 9                 # (N_CONTIGS below)
        self.name, self.mode, self.legacy, self.error, self.tags, self.shards = name, mode, bool(legacy), bool(error), tuple(tags), shards
        self.emulate = emulate and not legacy                  # (the --legacy producer is device code in rsqc_kernels.hip: device only)
        self.segs = [list(s) for s in segs]
        self.records = []
        for t, s in enumerate(self.segs):
            for i, r in enumerate(s):
                r = dict(r); r["tid"] = t; r.setdefault("pos", 10 + 2 * i); r["qname"] = "r%d" % len(self.records)
                self.records.append(r)
        self.n = len(self.records)
        assert self.n <= 8400, name
        at = np.concatenate([[0], np.cumsum([len(s) for s in self.segs])]).astype(int)
        if mode == "plain":
            assert file_index is None and shards is None
            edges = [0] + [int(c) for c in cuts] + [self.n]
            assert all(a < b for a, b in zip(edges, edges[1:])), name
            self.bounds = list(zip(edges, edges[1:]))
            self.file_index = [a for a, _ in self.bounds]
        else:
            assert not cuts and not legacy and all(len(s) for s in self.segs)
            self.bounds = [(int(at[k]), int(at[k + 1])) for k in range(len(self.segs))]
            self.file_index = [int(x) for x in (file_index if file_index is not None else at[:-1])]
            assert len(self.file_index) == len(self.segs)
            assert all(self.file_index[k] + len(self.segs[k]) <= self.file_index[k + 1] for k in range(len(self.segs) - 1))
        # ---- what kr_ref expects: per part (a batch, or a range) and for the file
        L = self.legacy
        self.parts = [self.records[a:b] for a, b in self.bounds]
        self.tables = [kr_ref.transfer_table(p, L) for p in self.parts]
        self.extremes = [kr_ref.extremes(p, L) for p in self.parts]
        self.entry = [kr_ref.state_machine(self.records[:a], 0, L) for a, _ in self.bounds]      # (plain: the state a batch is entered with)
        self.final = kr_ref.state_machine(self.records, 0, L)
        self.P = [len(t[0]) for t in self.tables]
        # the table as the library keeps it: the literal one, but a part whose eligible records all have ONE length L is the single entry
        # (largest span, L) -- the same function (every state of the literal table is L), which is what "equal" is checked as below
        self.device_tables = [([e[0]], [e[1]]) if e[1] == e[2] else t for t, e in zip(self.tables, self.extremes)]
        for t, d in zip(self.tables, self.device_tables):
            assert all(kr_ref.apply_table(t, r) == kr_ref.apply_table(d, r) for k in t[0] for r in (0, k - 1, k, k + 1)), name
        assert self.final == kr_ref.compose(self.tables), name
        assert self.error == any(p > MAXP for p in self.P), name
        if check is not None:
            check(self)

    def __repr__(self):
        return "Case(%s)" % self.name


# ---------------------------------------------------------------- walks: the number of prefix maxima
def _walk_records(P):
    """P prefix maxima (spans 200, 201, ...), each followed by an eligible record that fires the low walks only and one that does not count.
    Every fourth maximum is a soft-clipped read longer than every span: it ends the walks that reach it, each in its own state."""
    out = []
    for k in range(P):
        out.append(rec(200 + k, 1000 + (k // 4) % 5) if k % 4 == 3 else rec(200 + k, 50 + k % 7))
        out.append(rec(60, 40 + k % 3))
        out.append(ineligible(k, 90))
    return out


def _walks_check(P):
    def check(c):
        part = max(range(len(c.P)), key=lambda k: c.P[k])
        assert c.P[part] == P, (c, c.P)
        keys, states = c.tables[part]
        assert P < 3 or len(set(states)) >= 3, c
        assert P < 3 or len({kr_ref.apply_table((keys, states), r) for r in [0] + keys}) >= 3, c
        assert c.extremes[part][1] != c.extremes[part][2] or P <= 1, c
    return check


def _entered_walk_records(P):
    """P prefix maxima two apart (spans 200, 202, ...: an entry state fits between two keys), nearly all of them soft-clipped reads longer
    than every span, of eleven lengths by turns: neighbouring keys, and keys 64 apart, leave different states.  Every eighth is a short
    read, whose walk goes on to the next key."""
    out = []
    for k in range(P):
        out.append(rec(200 + 2 * k, 50 + k % 7) if k % 8 == 5 else rec(200 + 2 * k, 1000 + k % 11))
        out.append(rec(60, 40 + k % 3))
        out.append(ineligible(k, 90))
    return out


def _entered_walk_cases():
    """A batch of more than 64 keys entered with a state that the batch before left: the application of the table to `r_in`, where the
    keys of walks 64 and above live in s1 / v1 (`m1` decides only when no key of s0 exceeds the entry state)."""
    out = []
    for P in (65, 127, 128):
        key = lambda k: 200 + 2 * k
        where = [("below_key_0", 50, 0), ("equal_to_key_63", key(63), 64), ("between_keys_63_and_64", key(63) + 1, 64)]
        if P > 65:                                                        # (of 65 keys, key 64 is the last)
            where += [("equal_to_key_64", key(64), 65)]
        if P > 101:
            where += [("equal_to_key_100", key(100), 101)]
        where += [("equal_to_the_last_key", key(P - 1), P), ("above_the_last_key", key(P - 1) + 40, P)]
        for name, r1, first_above in where:
            first = [rec(600, r1)] + fillers(9, 5)

            def check(c, r1=r1, k=first_above, P=P):
                keys, states = c.tables[1]
                assert c.entry == [0, r1] and c.P[1] == P and keys == [200 + 2 * j for j in range(P)], (c, c.entry, c.P)
                assert [j for j in range(P) if keys[j] > r1][:1] == ([k] if k < P else []), c
                want = states[k] if k < P else r1
                assert c.final == want, (c, c.final, want)
                if 64 <= k < P:
                    assert want != states[k - 64] and want != r1, c          # neither lane k - 64's first walk, nor the state left alone
                if r1 in keys:                                                # entered AT a key: that key's own state is another answer
                    assert states[keys.index(r1)] != want, c
            out.append(Case("walks_%d_keys_entered_%s" % (P, name), [first + _entered_walk_records(P)], cuts=[10], check=check,
                            tags=("walks", "entered") + (("sanitize",) if P == 65 else ())))
    return out


def _walk_cases():
    out = _entered_walk_cases()
    for P in (1, 2, 63, 64, 65, 127, 128, 129):
        recs = _walk_records(P) if P > 1 else [rec(200, 50), ineligible(0, 90), rec(60, 40), rec(150, 41)]
        out.append(Case("walks_%d_prefix_maxima" % P, [recs], error=P > MAXP, check=_walks_check(P), tags=("walks", "sanitize")))
    rng = _rng("walks_ranges")
    out.append(Case("walks_ranges_65_and_128", [_walk_records(65), mixed(rng, 30), _walk_records(128)], mode="ranges", check=_walks_check(128), tags=("walks", "sanitize")))
    out.append(Case("walks_ranges_129_in_the_second_range", [mixed(rng, 50), _walk_records(129), mixed(rng, 20)], mode="ranges", error=True, check=_walks_check(129),
                    tags=("walks", "sanitize")))
    return out


# ---------------------------------------------------------------- values
def _value_cases():
    def has(**kw):
        def check(c):
            el = [r for r in c.records if kr_ref.eligible(r)]
            if "lq" in kw:
                assert any(kr_ref.l_qseq(r) == kw["lq"] for r in el), c
            if "span" in kw:
                assert any(kr_ref.span(r) == kw["span"] for r in el) and kw["span"] in c.tables[0][0], c
            if "final" in kw:
                assert c.final == kw["final"], (c, c.final)
            assert c.extremes[0][1] != c.extremes[0][2], c             # the general path
        return check
    tail = [rec(30, 35), rec(25, 31)]
    out = [
        Case("value_l_qseq_0_on_an_eligible_record", [[rec(40, 44), rec(50, 0), rec(30, 35), rec(25, 31)]], check=has(lq=0, final=35), tags=("sanitize",)),
        Case("value_l_qseq_0_is_the_final_state", [[rec(40, 44), rec(30, 35), rec(50, 0)]], check=has(lq=0, final=0), tags=("sanitize",)),
        Case("value_l_qseq_65534", [[rec(40, 44), rec(100, 65534)] + tail], check=has(lq=65534, final=65534), tags=("sanitize",)),
        Case("value_l_qseq_65535_the_escape_value", [[rec(40, 44), rec(100, 65535)] + tail], check=has(lq=65535, final=65535), tags=("sanitize",)),
        Case("value_l_qseq_70000_through_the_wide_table", [[rec(40, 44), rec(100, 70000)] + tail], check=has(lq=70000, final=70000), tags=("sanitize",)),
        Case("value_span_1_from_a_cigar_without_reference_bases", [[dict(cigar=[(S, 10), (I, 5)], flag=0, mapq=255, nm=0), rec(30, 35), rec(25, 31)]], check=has(span=1, lq=15),
             tags=("sanitize",)),
        Case("value_span_1_from_a_record_without_operations", [[dict(cigar=[], l_qseq=25, flag=0, mapq=255, nm=0), rec(20, 19), rec(30, 35)]], check=has(span=1, lq=25),
             tags=("sanitize",)),
        Case("value_span_above_65536_through_one_long_N", [[rec(40, 44), rec(70020, 40), rec(50, 47), rec(45, 48)]], check=has(span=70020), tags=("sanitize",)),
        Case("value_position_0", [[rec(40, 44, pos=0), rec(60, 35, pos=0), rec(50, 47, pos=1)]], check=has(span=60), tags=("sanitize",)),
    ]
    return out


def _eq(a, b):
    assert a == b, (a, b)


# ---------------------------------------------------------------- the equal-length shortcut, nothing eligible
def _shortcut_cases():
    def body(n, other=None):
        out = []
        for i in range(n):
            out.append(rec(30 + (i * 7) % 40, 76))
            out.append(ineligible(i, (50, 30, 20, 100)[i % 4]))
        if other is not None:
            out[2 * other] = rec(33, 75)
        return out

    def same(c):
        assert c.extremes[0][1] == c.extremes[0][2] == 76 and set(c.tables[0][1]) == {76} and c.device_tables[0] == ([c.extremes[0][0]], [76]), c
        assert {kr_ref.l_qseq(r) for r in c.records if not kr_ref.eligible(r)} == {50, 30, 20, 100}

    def general(c):
        assert c.extremes[0][1:] == (75, 76) and c.P[0] > 1, c
    return [Case("shortcut_one_length_between_ineligible_records_of_others", [body(100)], check=same, tags=("sanitize",)),
            Case("shortcut_broken_by_one_eligible_record_of_another_length", [body(100, other=60)], check=general, tags=("sanitize",))]


def _nothing_cases():
    none = [ineligible(i, 40 + i % 9) for i in range(70)]

    def identity(part):
        def check(c):
            assert c.P[part] == 0 and c.extremes[part] == (0, kr_ref.NO_LENGTH, 0) and c.tables[part] == ([], []), c
        return check
    rng = _rng("nothing")
    head = mixed(rng, 90)
    return [Case("nothing_eligible_in_the_only_batch", [none], check=lambda c: (identity(0)(c), _eq(c.final, 0)), tags=("sanitize",)),
            Case("nothing_eligible_in_the_only_range", [none], mode="ranges", file_index=[500], check=lambda c: (identity(0)(c), _eq(c.final, 0)), tags=("sanitize",)),
            Case("nothing_eligible_behind_a_batch_that_set_the_state", [head + none], cuts=[90], check=lambda c: (identity(1)(c), _eq(c.final, c.entry[1]), _eq(c.final > 0, True)),
                 tags=("sanitize",))]


# ---------------------------------------------------------------- the state goes down
def _lowered(name, n, at_low, at_again, first=0, tags=()):
    """fillers of span 20; `first` fires from 0 and leaves 50; the spliced record at `at_low` (span 5000) fires and leaves 30; the record at
    `at_again` (span 40, between the two) counts again and leaves 45"""
    recs = fillers(n)
    recs[first] = rec(50, 50); recs[at_low] = rec(5000, 30); recs[at_again] = rec(40, 45)

    def check(c):
        assert first < at_low < at_again < c.n
        assert c.final == 45 and kr_ref.monotone(c.records) == 50 != c.final, c
        assert c.tables[0] == ([50, 5000], [45, 45]), c
    return Case(name, [recs], check=check, tags=("lowered",) + tuple(tags))


def _lowered_cases():
    g = GROUP
    out = [
        _lowered("lowered_within_fewer_than_64_tiles", 600, 200, 500, tags=("sanitize",)),
        _lowered("lowered_in_lane_0_reopens_a_tile_of_the_same_group", g + TILE * 12, g + TILE * 5, g + TILE * 9 + 7),
        _lowered("lowered_in_lane_63_reopens_a_tile_of_the_same_group", g + TILE * 12, g + TILE * 5 + 63, g + TILE * 9 + 7),
        _lowered("lowered_reopens_tile_63_of_the_group", 2 * g + 10, g + TILE * 62 + 10, g + TILE * 63 + 3),
        _lowered("lowered_in_tile_63_reopens_a_tile_of_the_second_group", g + TILE * 3, TILE * 63 + 5, g + 2),
        _lowered("lowered_reopens_a_tile_of_the_third_group", 2 * g + 200, g + 100, 2 * g + 70),
        _lowered("lowered_reopens_the_last_partial_tile", g + TILE * 3 + 10, g + 20, g + TILE * 3 + 7),
    ]
    names = {c.name: c for c in out}
    c = names["lowered_in_lane_0_reopens_a_tile_of_the_same_group"]
    assert kr_ref.span(c.records[g + TILE * 5]) == 5000 and (g + TILE * 5) % TILE == 0
    c = names["lowered_in_lane_63_reopens_a_tile_of_the_same_group"]
    assert kr_ref.span(c.records[g + TILE * 5 + 63]) == 5000 and (g + TILE * 5 + 63) % TILE == 63
    c = names["lowered_reopens_tile_63_of_the_group"]
    assert ((g + TILE * 63 + 3) // TILE) % 64 == 63 and kr_ref.span(c.records[g + TILE * 63 + 3]) == 40
    assert names["lowered_reopens_a_tile_of_the_third_group"].n > 2 * g + 64 and names["lowered_reopens_the_last_partial_tile"].n % TILE != 0
    return out


# ---------------------------------------------------------------- the gate's comparisons are strict
def _gate_cases():
    def build(name, head, at, probe, final, keys):
        recs = fillers(TILE * 4)
        for i, r in head:
            recs[i] = r
        recs[at] = probe

        def check(c):
            assert c.final == final and c.tables[0][0] == keys, (c, c.final, c.tables)
        return Case(name, [recs], check=check, tags=("gate",))
    hi, low = [(0, rec(50, 1000))], [(0, rec(50, 50)), (70, rec(5000, 30))]
    return [build("gate_tile_max_equals_the_largest_span_so_far", hi, TILE * 2 + 9, rec(50, 77), 1000, [50]),
            build("gate_tile_max_is_the_largest_span_so_far_plus_1", hi, TILE * 2 + 9, rec(51, 77), 1000, [50, 51]),
            build("gate_tile_max_equals_the_smallest_live_state", low, TILE * 3 + 9, rec(30, 99), 30, [50, 5000]),
            build("gate_tile_max_is_the_smallest_live_state_plus_1", low, TILE * 3 + 9, rec(31, 99), 99, [50, 5000]),
            build("gate_span_equals_the_largest_so_far_above_the_live_states", low, TILE * 3 + 9, rec(5000, 33), 33, [50, 5000])]


# ---------------------------------------------------------------- the state carried from batch to batch
def _carry_cases():
    second = [rec(100, 300)] + fillers(20, 5) + [rec(110, 105)] + fillers(20, 5, 1) + [rec(120, 115)] + fillers(27, 5, 2)
    assert kr_ref.transfer_table(second) == ([100, 110, 120], [300, 115, 115])
    out = []
    for cut in (1, 63, 64, 65):
        for where, r1, want in (("below_every_key", 50, 300), ("equal_to_a_key", 100, 115), ("between_two_keys", 105, 115), ("equal_to_the_largest_key", 120, 120),
                                ("above_all_keys", 200, 200)):
            first = [rec(600, r1)] + fillers(cut - 1, 5)

            def check(c, r1=r1, want=want, cut=cut):
                assert c.bounds[0] == (0, cut) and c.entry == [0, r1] and c.tables[1] == ([100, 110, 120], [300, 115, 115]) and c.final == want, (c, c.entry, c.final)
            out.append(Case("carry_cut_at_%d_entry_state_%s" % (cut, where), [first + second], cuts=[cut], check=check, tags=("carry",) + (("sanitize",) if cut == 65 and r1 in (100, 120) else ())))
    rng = _rng("carry_random")
    recs = mixed(rng, 700)
    out.append(Case("carry_batches_of_1_63_64_65_records", [recs], cuts=[1, 64, 128, 193], check=lambda c: _eq([b - a for a, b in c.bounds][:4], [1, 63, 64, 65]), tags=("carry", "sanitize")))
    for k in range(3):
        cuts = sorted(set(int(x) for x in rng.integers(1, 700, 4)))
        out.append(Case("carry_random_cuts_%d" % k, [recs], cuts=cuts, check=lambda c: _eq(len(set(c.entry)) >= 3, True), tags=("carry",)))
    return out


# ---------------------------------------------------------------- batches of file ranges
def _range_cases():
    rng = _rng("ranges")

    def gaps(sizes, gap=1000):
        """file indices with the records of other shards between the ranges"""
        out, at = [], 7
        for s in sizes:
            out.append(at); at += s + gap
        return out

    def mk(name, segs, check=None, **kw):
        return Case(name, segs, mode="ranges", file_index=gaps([len(s) for s in segs]), check=check, tags=("ranges", "sanitize"), **kw)

    def general_everywhere(c):
        assert all(e[1] != e[2] for e in c.extremes), (c, c.extremes)
    same = [rec(30 + (i * 7) % 40, 76) for i in range(50)]
    none = [ineligible(i, 40 + i % 9) for i in range(45)]
    out = [
        mk("ranges_of_1_63_64_and_65_records", [[rec(41, 44)], mixed(rng, 63), mixed(rng, 64), mixed(rng, 65)], check=lambda c: _eq([len(s) for s in c.segs], [1, 63, 64, 65])),
        mk("ranges_four_inside_one_tile", [mixed(rng, 3, bad=0), [rec(58, 21)], mixed(rng, 20), mixed(rng, 40)], check=lambda c: _eq(c.n, 64)),
        mk("ranges_boundary_on_a_tile_edge", [mixed(rng, 64), mixed(rng, 128), mixed(rng, 30)], check=general_everywhere),
        mk("ranges_one_without_an_eligible_record_between_two_with_some", [mixed(rng, 80), none, mixed(rng, 70)],
           check=lambda c: _eq((c.P[1], c.extremes[1], c.P[0] > 1, c.P[2] > 1), (0, (0, kr_ref.NO_LENGTH, 0), True, True))),
        mk("ranges_same_length_beside_mixed", [mixed(rng, 70), same, mixed(rng, 40)], check=lambda c: _eq((len(c.device_tables[1][0]), c.extremes[1][1], c.extremes[1][2], c.P[0] > 1), (1, 76, 76, True))),
        mk("ranges_one_starts_in_tile_63_of_a_group", [fillers(TILE * 63 + 10) + [], mixed(rng, 200)], check=lambda c: _eq((c.bounds[1][0] // TILE) % 64, 63)),
    ]
    segs = [mixed(rng, 90), mixed(rng, 40), mixed(rng, 130), mixed(rng, 75)]
    at = np.concatenate([[0], np.cumsum([len(s) for s in segs])])
    out.append(Case("ranges_two_shards_interleaved", segs, mode="ranges", file_index=[int(x) for x in at[:-1]], shards=[[0, 2], [1, 3]],
                    check=lambda c: (general_everywhere(c), _eq(len({kr_ref.compose(c.tables[:k]) for k in range(1, 5)}) >= 2, True)), tags=("ranges", "shards", "sanitize")))
    # four contigs whose record counts send contigs 1 and 2 to one shard and 0 and 3 to the other (longest-processing-time packing, the
    # command line's rule and distributed.assign_contigs); the tables are such that composing shard after shard, in either order of the
    # shards, gives another value than composing in file order
    segs = [[rec(40, 29)] + fillers(89), [rec(30, 300)] + fillers(39), [rec(600, 26)] + fillers(129), [rec(28, 77)] + fillers(74)]
    at = np.concatenate([[0], np.cumsum([len(s) for s in segs])])

    def order_matters(c):
        from rnaseqc_amd import distributed
        rank = distributed.assign_contigs([len(s) for s in c.segs], 2)
        assert sorted([k for k in range(4) if rank[k] == g] for g in (0, 1)) == sorted(c.shards) == [[0, 3], [1, 2]], (c, rank)
        assert c.tables == [([40], [29]), ([30], [300]), ([600], [26]), ([28], [77])] and c.final == 77, (c, c.tables)
        for order in ([1, 2, 0, 3], [0, 3, 1, 2]):
            assert kr_ref.compose([c.tables[k] for k in order]) != c.final, (c, order)
        general_everywhere(c)
    out.append(Case("ranges_two_shards_whose_order_is_not_file_order", segs, mode="ranges", file_index=[int(x) for x in at[:-1]], shards=[[1, 2], [0, 3]], check=order_matters,
                    tags=("ranges", "shards", "sanitize")))
    return out


# ---------------------------------------------------------------- the producers: who hands the largest span on
LONG_OPS = [(H, 5), (S, 3), (M, 30), (I, 2), (D, 3), (N, 400), (M, 30), (I, 1), (M, 10), (S, 2)]         # 10 operations, three blocks: span 473
FOUR_BLOCKS = [(M, 20), (N, 100), (M, 20), (N, 100), (M, 20), (N, 100), (M, 20)]                         # span 380
WIDE_OPS = [(M, 2), (I, 1)] * 130                                                                        # 260 operations (the wide table): span 260
THREE = [(M, 30), (N, 5), (M, 30), (N, 7), (M, 30)]                                                      # span 102
THREE_LONGEST = [(M, 30), (N, 5), (M, 30), (N, 50), (M, 30)]                                             # span 145


def _producer_cases():
    rng = _rng("producers")

    def holds_the_maximum(part, i, span):
        def check(c):
            a, _ = c.bounds[part]
            assert kr_ref.span(c.records[a + i]) == span == c.extremes[part][0] == c.tables[part][0][-1], c
            assert sum(1 for r in c.parts[part] if kr_ref.eligible(r) and kr_ref.span(r) == span) == 1 and c.extremes[part][1] != c.extremes[part][2], c
        return check
    out = []
    for name, cig in (("more_than_8_operations", LONG_OPS), ("four_blocks", FOUR_BLOCKS), ("255_or_more_operations", WIDE_OPS)):
        r = dict(cigar=cig, flag=0, mapq=255, nm=0)
        sp = kr_ref.span(r)
        recs = mixed(rng, 150); recs[100] = r
        out.append(Case("producer_largest_span_has_%s" % name, [recs], check=holds_the_maximum(0, 100, sp), tags=("producers", "sanitize")))
        a, b = mixed(rng, 40), mixed(rng, 60); b[10] = r                       # record 50 of the batch: behind the boundary inside tile 0
        out.append(Case("producer_largest_span_has_%s_in_a_boundary_tile" % name, [a, b], mode="ranges", file_index=[3, 900], check=holds_the_maximum(1, 10, sp),
                        tags=("producers", "sanitize")))

    def ring(n):
        """the second input of test_every_record_deferred_fills_the_long_kernels_chunks (tests/test_k1_wave_emulation.py): a wave's ring holds 63
        three-block records when a tile of 64 more arrives; one of the records it cannot take holds the largest span"""
        recs = []
        for i in range(n):
            three = i >= 192 or (i < 189 and i % 3 == 0)
            recs.append(dict(cigar=THREE if three else [(M, 90)], flag=0, mapq=255, nm=0, **({} if i % 5 else dict(l_qseq=95))))
        recs[192 + 60] = dict(cigar=THREE_LONGEST, flag=0, mapq=255, nm=0)
        return recs
    out.append(Case("producer_largest_span_in_the_three_block_rings_surplus", [ring(400)], check=holds_the_maximum(0, 252, 145), tags=("producers", "ring", "sanitize")))
    out.append(Case("producer_largest_span_in_the_three_block_rings_surplus_in_a_boundary_tile", [ring(400)[:255], mixed(rng, 30)], mode="ranges", file_index=[0, 5000],
                    check=lambda c: (holds_the_maximum(0, 252, 145)(c), _eq(c.bounds[1][0] // TILE, 252 // TILE)), tags=("producers", "ring", "sanitize")))
    # --legacy (plain batches; device only): a span of 100 000 counts, 100 001 does not
    for sp, counts in ((100000, True), (100001, False)):
        recs = mixed(rng, 150); recs[149] = rec(sp, 99)                 # the file's last record: it decides when it counts

        def check(c, sp=sp, counts=counts):
            assert c.bounds[1] == (70, 150) and (c.extremes[1][0] == sp) == counts and (sp in c.tables[1][0]) == counts, c
            assert c.legacy and kr_ref.eligible(c.records[149], True) == counts and kr_ref.eligible(c.records[149], False)
            assert (c.final == 99) == counts and kr_ref.state_machine(c.records, 0, False) == 99, c
        out.append(Case("producer_legacy_span_%d" % sp, [recs], cuts=[70], legacy=True, check=check, tags=("producers", "legacy")))
    return out


def all_cases():
    return _walk_cases() + _value_cases() + _shortcut_cases() + _nothing_cases() + _lowered_cases() + _gate_cases() + _carry_cases() + _range_cases() + _producer_cases()


_CASES = None


def cases():
    """the catalogue, built once"""
    global _CASES
    if _CASES is None:
        _CASES = all_cases()
        assert len({c.name for c in _CASES}) == len(_CASES)
    return _CASES


# ---------------------------------------------------------------- a case as input of the C ABI (device, oracle, emulation)
_MEMO = {}


N_CONTIGS = 9


def annotation(case=None):
    """one gene with one exon per contig, nine contigs: the same annotation for every case (a context keeps it across the catalogue)"""
    from rnaseqc_amd.model import Annotation
    if "ann" not in _MEMO:
        rows = []
        for t in range(N_CONTIGS):
            rows.append(dict(contig="c%d" % t, type="gene", start=1, end=GENE_END, strand="+", gene_id="G%d" % t))
            rows.append(dict(contig="c%d" % t, type="exon", start=1, end=GENE_END, strand="+", gene_id="G%d" % t, exon_id="E%d" % t))
        _MEMO["ann"] = Annotation.from_rows(["c%d" % t for t in range(N_CONTIGS)], rows)
    return _MEMO["ann"]


def contigs():
    return [("c%d" % t, GENE_END + 200000) for t in range(N_CONTIGS)]


def file_batch(case):
    """the whole file as one batch, file order (left unchanged: the batches below are slices of it)"""
    from rnaseqc_amd.model import Batch
    if ("file", case.name) not in _MEMO:
        _MEMO[("file", case.name)] = Batch.from_records(case.records)
    return _MEMO[("file", case.name)]


def part_batches(case, which=None):
    """one batch per part -- the plain batches, or the ranges one by one -- with its file index"""
    import copy
    full = file_batch(case)
    out = []
    for k, (a, b) in enumerate(case.bounds):
        if which is not None and k not in which:
            continue
        p = copy.copy(full.slice(a, b))
        p.file_index_base = case.file_index[k]
        out.append(p)
    return out


def range_batch(case, which=None):
    """the ranges (all, or those of one shard) as ONE batch"""
    from rnaseqc_amd.model import Batch
    assert case.mode == "ranges"
    return Batch.concat_ranges(part_batches(case, which))


def params(case):
    return abi.default_params(legacy=1, mapq_threshold=4) if case.legacy else abi.default_params()
