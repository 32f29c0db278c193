"""Named cases for the fragment-size stage K5 (rnaseqc_amd/csrc/rsqc_k5.h, host side rsqc_fragsize.hip) in one-step neighbours of its
constants, and a plain reference.  tests/test_k5_edges_host.py runs them under the 64-lane emulation (tests/hostemu/k5_emu.cpp:
k5emu_run_cands / k5emu_partition) and asserts the numbers each case states against the exported plan, fills and paths;
tests/test_gpu_k5_edges.py runs them as records through the C ABI on the device.

A case is a list of candidates in emission order -- the columns (file_index, qhash, h2, interval, endpos, flag_size: |isize| with bit 31 =
the record may complete a pair) -- plus max_samples and `expect`, what the case is named for:
    n_buckets        fill {bucket: candidates}        path {bucket: "set" | "sort" | "listed"} (every non-empty bucket unless `path_rest`)
    samples / kept / last_kept / top / beyond / distinct: stated where the case is about them (the rest comes from walk())
    error: the error word (0, or abi.ERR_CAPACITY)
Most cases also have a RECORDS form (Case.rec: file-order arrays): record f of a coordinate-sorted hash-only batch is candidate f.

The reference is walk(): a dict keyed by (qhash, h2) walked in file-index order with the rule of src/Expression.cpp:509-538, the first
max_samples samples by file index, a Counter of their sizes.  No buckets, sets, sorts or tables."""
import collections

import numpy as np

from rnaseqc_amd import abi

PB_MEAN, PB_CAP, PB_THREADS, PB_BIG_MAX, PH_SLOTS, BIG_GRID = 384, 2048, 256, 1024, 1024, 64      # rsqc_k5.h / rsqc_k5_plan.h
SIZE_LDS, SIZE_TABLE, PAIRS_FIRST = 4096, 1 << 20, 2048
K = 0x9E3779B97F4A7C15                                  # the multiplier of the pairing set's mix (pair_bucket_hashed)
M64, M32 = (1 << 64) - 1, 0xFFFFFFFF
OK = 0x80000000
COLUMNS = ("file_index", "qhash", "h2", "interval", "endpos", "flag_size")
DTYPES = (np.uint64, np.uint64, np.uint32, np.int32, np.int32, np.uint32)
READ, SHORT = 50, 20                                    # read lengths of the records form


# ---------------------------------------------------------------- the host rules, restated
def n_buckets(n):
    return max(1, n // PB_MEAN)


def bucket_of(qhash, nb):
    """pair_bucket_of (numpy, any shape)"""
    return (((np.asarray(qhash, np.uint64) >> np.uint64(32)) * np.uint64(nb)) >> np.uint64(32)).astype(np.int64)


def high_word_range(nb, b):
    """the high words [lo, hi) that pair_bucket_of sends to bucket b of nb"""
    return -(-(b << 32) // nb), -(-((b + 1) << 32) // nb)


def mix(q, h2):
    """the 64-bit key of a 96-bit name in the pairing set (0 is stored as 1)"""
    return ((q ^ (h2 * K)) & M64) or 1


# ---------------------------------------------------------------- the reference
def walk(cols, max_samples):
    """-> (samples, kept, pairs): all samples [(file index, size)] in file order, the first max_samples of them, [(size, count)] ascending"""
    order = np.argsort(cols["file_index"], kind="stable")
    q, h2, iv, end, fs = (np.asarray(cols[f])[order].tolist() for f in COLUMNS[1:])
    files = np.asarray(cols["file_index"])[order].tolist()
    open_names, samples = {}, []
    for i in range(len(files)):
        key = (q[i], h2[i])
        e = open_names.get(key)
        if e is None:
            open_names[key] = (iv[i], end[i])                       # :512-516
        elif e[0] == iv[i]:                                         # :517
            if not (fs[i] >> 31) or end[i] <= e[1]:                 # :528 (the entry stays)
                continue
            samples.append((files[i], fs[i] & 0x7FFFFFFF))          # :530
            del open_names[key]                                     # :531
    kept = samples[:max_samples]
    return samples, kept, sorted(collections.Counter(s for _, s in kept).items())


class Case:
    def __init__(self, name, cols, max_samples, expect, rec=None, emulate="full", device=None, tags=(), slow_device=False):
        self.name, self.max_samples, self.expect = name, int(max_samples), dict(expect)
        self.cols = {f: np.ascontiguousarray(cols[f], dt) for f, dt in zip(COLUMNS, DTYPES)}
        self.n = len(self.cols["qhash"])
        assert all(len(c) == self.n for c in self.cols.values())
        self.rec = rec                                      # file-order arrays of the records form (None: the case says why)
        self.emulate = emulate                              # "full", "partition" (the three partition kernels alone) or None
        self.device = (rec is not None) if device is None else device
        self.tags = frozenset(tags)                         # "set": more schedules; "sanitize": through the stand-alone sanitizer program
        self.slow_device = slow_device                      # the two cases of 2.1 M records
        self._walk = None

    def reference(self):
        if self._walk is None:
            self._walk = walk(self.cols, self.max_samples)
        return self._walk

    def fills(self):
        return np.bincount(bucket_of(self.cols["qhash"], n_buckets(self.n)), minlength=n_buckets(self.n))

    def __repr__(self):
        return self.name


def _rng(name):
    return np.random.default_rng(int.from_bytes(name.encode(), "little") % (1 << 63))


# ---------------------------------------------------------------- building candidates
def names_in_bucket(rng, nb, b, k):
    """k distinct 64-bit name hashes that bucket b of nb receives (high words drawn inside the bucket's range)"""
    lo, hi = high_word_range(nb, b)
    assert hi - lo >= 1
    out = np.zeros(0, np.uint64)
    while len(out) < k:
        w = rng.integers(lo, hi, 2 * (k - len(out)) + 8, dtype=np.uint64)
        out = np.unique(np.concatenate([out, (w << np.uint64(32)) | rng.integers(0, 1 << 32, len(w), dtype=np.uint64)]))
    out = rng.permutation(out)[:k]
    assert (bucket_of(out, nb) == b).all()
    return out


class Builder:
    """Candidates by bucket and name; build() numbers them as the records of a coordinate-sorted file: file index f = 0 .. n - 1 in a
    seeded shuffle that keeps a name's records in the order given, position 2000 + f (+ 1000 per BED interval in front), one block of
    `len` bases, so endpos = pos + len.  Unless `sure`, a record is short (20 instead of 50 bases) one time in four and lacks the
    completing flags one time in four; the last eighth of the file lies in a second BED interval (a name across the cut yields nothing)."""
    def __init__(self, name, n, one_interval=False):
        self.name, self.n, self.nb, self.rng, self.one_interval = name, n, n_buckets(n), _rng(name), one_interval
        self.q, self.h2, self.nid, self.rank, self.sure, self.size = [], [], [], [], [], []
        self.names = 0

    def add(self, bucket, group, sure=False, q=None, h2=None, size=None):
        """names of group[i] records each into `bucket`; sure: 50 bases and the completing flags on every record (each pair of records
        in one interval yields a sample); q / h2 / size: given instead of drawn (size per record, 0 = drawn)"""
        group = np.asarray(group, np.int64)
        k, m = len(group), int(group.sum())
        q = names_in_bucket(self.rng, self.nb, bucket, k) if q is None else np.asarray(q, np.uint64)
        assert (bucket_of(q, self.nb) == bucket).all()
        h2 = self.rng.integers(0, 1 << 32, k, dtype=np.uint64).astype(np.uint32) if h2 is None else np.asarray(h2, np.uint32)
        first = np.concatenate([[0], np.cumsum(group)[:-1]])
        self.q.append(np.repeat(q, group)); self.h2.append(np.repeat(h2, group))
        self.nid.append(np.repeat(np.arange(k) + self.names, group)); self.rank.append(np.arange(m) - np.repeat(first, group))
        self.sure.append(np.full(m, sure, bool)); self.size.append(np.zeros(m, np.int64) if size is None else np.asarray(size, np.int64))
        self.names += k
        return self

    def pairs(self, bucket, m, **kw):
        """m candidates as m // 2 names of two records and, for an odd m, one of one"""
        return self.add(bucket, [2] * (m // 2) + [1] * (m % 2), **kw)

    def mixed(self, bucket, m, **kw):
        """m candidates in names of one or two records, about one name in three a single"""
        g = []
        while sum(g) < m:
            g.append(1 if (m - sum(g) == 1 or self.rng.integers(0, 3) == 0) else 2)
        return self.add(bucket, g, **kw)

    def build(self, max_samples, expect, file_of=None, emission=None, **kw):
        q, h2, nid, rank, sure, size = (np.concatenate(x) for x in (self.q, self.h2, self.nid, self.rank, self.sure, self.size))
        n, rng = len(q), self.rng
        assert n == self.n, (self.name, n, self.n)
        file = rng.permutation(n).astype(np.int64) if file_of is None else np.asarray(file_of, np.int64)
        by_rank, by_file = np.lexsort((rank, nid)), np.lexsort((file, nid))          # a name's records take its file indices in the order given
        f2 = np.empty(n, np.int64); f2[by_rank] = file[by_file]
        o = np.argsort(f2)
        q, h2, sure, size = q[o], h2[o], sure[o], size[o]                             # file order from here on
        ln = np.where(sure | (rng.integers(0, 4, n) > 0), READ, SHORT)
        ok = sure | (rng.integers(0, 4, n) > 0)
        size = np.where(size > 0, size, 80 + rng.integers(0, 700, n))
        interval = np.zeros(n, np.int64) if self.one_interval else (np.arange(n) >= (7 * n) // 8).astype(np.int64)
        rec = dict(qhash=q.astype(np.uint64), h2=h2.astype(np.uint32), len=ln.astype(np.int64), size=size.astype(np.int64), ok=ok, interval=interval)
        expect = dict(expect); expect.setdefault("n_buckets", self.nb)
        return case_of_records(self.name, rec, max_samples, expect, rng=rng, emission=emission, **kw)


def positions(rec):
    return 2000 + np.arange(len(rec["qhash"]), dtype=np.int64) + 1000 * np.asarray(rec["interval"], np.int64)


def columns_of_records(rec):
    """the candidates the per-record kernel leaves for the records form, in file order"""
    n = len(rec["qhash"])
    return dict(file_index=np.arange(n, dtype=np.uint64), qhash=rec["qhash"], h2=rec["h2"], interval=rec["interval"].astype(np.int32),
                endpos=(positions(rec) + rec["len"]).astype(np.int32), flag_size=(rec["size"].astype(np.uint32) | np.where(rec["ok"], OK, 0).astype(np.uint32)))


def case_of_records(name, rec, max_samples, expect, rng=None, emission=None, **kw):
    cols = columns_of_records(rec)
    order = (rng or _rng(name)).permutation(len(rec["qhash"])) if emission is None else np.asarray(emission, np.int64)
    return Case(name, {f: np.asarray(c)[order] for f, c in cols.items()}, max_samples, expect, rec=rec, **kw)


def explicit(name, recs, max_samples=1_000_000, expect=None, emission=None, **kw):
    """recs in file order: (qhash, h2, len, size, ok[, interval])"""
    rec = dict(qhash=np.array([r[0] for r in recs], np.uint64), h2=np.array([r[1] for r in recs], np.uint32), len=np.array([r[2] for r in recs], np.int64),
               size=np.array([r[3] for r in recs], np.int64), ok=np.array([bool(r[4]) for r in recs]), interval=np.array([r[5] if len(r) > 5 else 0 for r in recs], np.int64))
    expect = dict(expect or {}); expect.setdefault("n_buckets", n_buckets(len(recs)))
    return case_of_records(name, rec, max_samples, expect, emission=emission, **kw)


def _filler(rng, k, size0=300):
    """k ordinary pairs (two records each, both complete) with distinct names, as explicit records"""
    out = []
    for i in range(k):
        q, h = int(rng.integers(1, 1 << 63)), int(rng.integers(0, 1 << 32))
        out += [(q, h, READ, size0 + i, 1), (q, h, READ, size0 + i, 1)]
    return out


# ---------------------------------------------------------------- the catalogue
def _bucket_count_cases():
    out = []
    for n in (383, 384, 767, 768):
        b = Builder("buckets_n_%d" % n, n)
        if n == 768:                                        # two buckets, 384 each: both through the set
            b.mixed(0, 384).mixed(1, 384)
            e = dict(n_buckets=2, fill={0: 384, 1: 384}, path={0: "set", 1: "set"})
        else:                                               # one bucket: 383 / 384 through the set, 767 beyond its 512
            b.mixed(0, n)
            e = dict(n_buckets=1, fill={0: n}, path={0: "set" if n < 512 else "sort"})
        out.append(b.build(1_000_000, e, tags=("set", "sanitize")))
    return out


def _scan_cases():
    """1 024 buckets: pair_bucket_scan_kernel's threads own one bucket each; 1 025: two each, the last bucket alone in thread 512's pair
    (the `hi` clamp), threads 513 .. 1 023 none.  First and last bucket full (2 048: the LDS sort), 760 (761) buckets of 512 between them
    at an even stride, the rest -- a quarter -- empty."""
    out = []
    for nb in (1024, 1025):
        n = nb * PB_MEAN
        b = Builder("scan_%d_buckets" % nb, n)
        rest = n - 2 * PB_CAP
        mid = np.unique(np.linspace(1, nb - 2, rest // 512 + (1 if rest % 512 else 0)).astype(np.int64))
        assert len(mid) == -(-rest // 512)
        fill, path = {0: PB_CAP, nb - 1: PB_CAP}, {0: "sort", nb - 1: "sort"}
        b.pairs(0, PB_CAP)
        for i, bk in enumerate(mid.tolist()):
            m = 512 if (i + 1) * 512 <= rest else rest - i * 512
            b.pairs(bk, m); fill[bk] = m; path[bk] = "set"
        b.pairs(nb - 1, PB_CAP)
        empty = nb - len(fill)
        assert empty > 250 and n_buckets(n) == nb
        out.append(b.build(5000, dict(n_buckets=nb, fill=fill, path=path, empty=empty)))
    # 2 049 buckets: three per thread, thread 682 owns the last three, thread 683 the bucket behind the last.  The partition kernels alone
    # (786 816 candidates: the replay adds nothing to what the two cases above run)
    nb = 2049
    n = nb * PB_MEAN
    rng = _rng("scan_2049")
    q = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    q[:3000] = names_in_bucket(rng, nb, 0, 3000); q[3000:6000] = names_in_bucket(rng, nb, nb - 1, 3000)
    z = np.zeros(n, np.int64)
    cols = dict(file_index=np.arange(n), qhash=q, h2=z, interval=z, endpos=z, flag_size=z)
    out.append(Case("scan_2049_buckets_partition_only", cols, 0, dict(n_buckets=nb, listed_min=2), emulate="partition", device=False))
    return out


def _set_cases():
    out = []
    # buckets of 32 / 33 (64 / 128 slots), 256 / 257 (512 / 1 024 slots), 512 (all of PairHash; 256 complete pairs that all yield: s_stash to
    # its last entry) and 513 (the sort); the seventh bucket takes the rest
    n = 7 * PB_MEAN
    b = Builder("set_buckets_of_32_33_256_257_512_513", n, one_interval=True)
    sizes = [32, 33, 256, 257, 512, 513]
    for bk, m in enumerate(sizes):
        b.pairs(bk, m, sure=(m == 512)) if m in (512, 513) else b.mixed(bk, m)
    b.mixed(6, n - sum(sizes))
    fill = dict(enumerate(sizes)); fill[6] = n - sum(sizes)
    path = {0: "set", 1: "set", 2: "set", 3: "set", 4: "set", 5: "sort", 6: "sort"}
    c = b.build(1_000_000, dict(fill=fill, path=path), tags=("set", "sanitize"))
    in4 = bucket_of(c.cols["qhash"], 7) == 4
    assert len(walk({f: v[in4] for f, v in c.cols.items()}, 1 << 30)[0]) == PH_SLOTS // 4          # 256 samples from the bucket of 512
    out.append(c)
    # 512 singletons: every slot count is 1, no sample
    out.append(Builder("set_512_singletons", 512).add(0, [1] * 512).build(1_000_000, dict(fill={0: 512}, path={0: "set"}, samples=0, kept=0), tags=("set", "sanitize")))
    # file order decides, not emission order.  A: the second mate is EMITTED first and completes (its size, 777, is the sample's); B: emitted
    # in file order; C: the later record is short and ends before the stored end -- no sample, though the pair read backwards would yield one
    # (the earlier record ends later and carries the flags)
    rng = _rng("order")
    a, b_, c_ = (int(x) for x in rng.integers(1, 1 << 63, 3))
    recs = [(a, 1, READ, 111, 1), (b_, 2, READ, 222, 1), (c_, 3, READ, 333, 1), (a, 1, READ, 777, 1), (b_, 2, READ, 888, 1), (c_, 3, SHORT, 999, 1)]
    out.append(explicit("set_second_mate_emitted_first", recs, emission=[3, 0, 1, 4, 5, 2],
                        expect=dict(path={0: "set"}, samples=2, raw=[(3, 777), (4, 888)]), tags=("set", "sanitize")))
    return out


def _handover_cases():
    """the set declines before anything is written; the sort gives the reference's answer"""
    out = []
    rng = _rng("handover")
    T = ("set", "sanitize")
    q = int(rng.integers(1, 1 << 63))
    # three records of one name: the second is short (ends before the stored end, the entry stays), the third completes
    recs = _filler(rng, 4) + [(q, 9, READ, 400, 1), (q, 9, SHORT, 401, 1), (q, 9, READ, 402, 1)] + _filler(rng, 3, 500)
    out.append(explicit("handover_a_name_of_three_candidates", recs, expect=dict(path={0: "sort"}, samples=8), tags=T))
    # two names on one mix, second hashes differ: q2 ^ h2b K == q ^ h2 K
    h2, h2b = 1234567, 7654321
    q2 = q ^ ((h2 * K) & M64) ^ ((h2b * K) & M64)
    assert mix(q, h2) == mix(q2, h2b) and (q, h2) != (q2, h2b)
    recs = _filler(rng, 3) + [(q, h2, READ, 410, 1), (q2, h2b, READ, 411, 1)] + _filler(rng, 3, 500) + [(q, h2, READ, 412, 1)]
    out.append(explicit("handover_two_names_on_one_mix", recs, expect=dict(path={0: "sort"}, samples=7), tags=T))
    # a name whose mix is 0 (stored as 1) beside a name whose mix is 1
    ha, hb = 5, 6
    qa, qb = (ha * K) & M64, ((hb * K) & M64) ^ 1
    assert (qa ^ (ha * K)) & M64 == 0 and (qb ^ (hb * K)) & M64 == 1 and mix(qa, ha) == mix(qb, hb) == 1
    recs = _filler(rng, 2) + [(qa, ha, READ, 420, 1), (qb, hb, READ, 421, 1), (qa, ha, READ, 422, 1), (qb, hb, READ, 423, 1)] + _filler(rng, 2, 500)
    out.append(explicit("handover_mix_0_beside_mix_1", recs, expect=dict(path={0: "sort"}, samples=6), tags=T))
    return out


def _sort_cases():
    out = []
    T = ("sanitize",)
    # 16 buckets: 2 047 (one padding slot), 2 048 (none), 2 049 (listed); names of one to four records
    n = 2047 + 2048 + 2049
    b = Builder("sort_buckets_of_2047_2048_2049", n)
    for bk, m in ((0, 2047), (5, 2048), (15, 2049)):
        g = []
        while sum(g) < m:
            g.append(min(m - sum(g), int(b.rng.integers(1, 5))))
        b.add(bk, g)
    out.append(b.build(1_000_000, dict(n_buckets=16, fill={0: 2047, 5: 2048, 15: 2049}, path={0: "sort", 5: "sort", 15: "listed"}), tags=T))
    # the padding key (~0, 0xFFFFFFFF) as a real name inside a bucket without padding slots: the last of five buckets holds all 2 048
    b = Builder("sort_padding_key_as_a_name_in_a_full_bucket", 2048, one_interval=True)
    b.add(4, [2], sure=True, q=[M64], h2=[M32], size=[0, 987]).mixed(4, 2046)
    c = b.build(1_000_000, dict(n_buckets=5, fill={4: 2048}, path={4: "sort"}), tags=T)
    assert 987 in [s for _, s in c.reference()[0]]
    out.append(c)
    # one name of eight records that yields four samples (a thread owns more than two samples: the third and fourth go straight to the list)
    rng = _rng("eight")
    q = int(rng.integers(1, 1 << 63))
    recs = _filler(rng, 3) + [(q, 3, READ, 600 + i, 1) for i in range(8)] + _filler(rng, 3, 500)
    out.append(explicit("sort_one_name_of_eight_records_yields_four_samples", recs, expect=dict(path={0: "sort"}, samples=10), tags=T))
    # a thread owns the names that start at its slots j, j + 256, j + 512: 300 sure pairs sort to slots 0, 2, 4 ... 598 (even threads own three
    # names, three samples each), a name of three records at the end hands the bucket to the sort
    b = Builder("sort_one_thread_owns_names_at_slots_j_and_j_plus_256", 603, one_interval=True)
    b.add(0, [2] * 300, sure=True).add(0, [3], sure=True, q=[M64 - 15])
    c = b.build(1_000_000, dict(n_buckets=1, fill={0: 603}, path={0: "sort"}, samples=301), tags=T)
    o = np.lexsort((c.cols["file_index"], c.cols["h2"], c.cols["qhash"]))            # the slots after the sort
    starts = np.flatnonzero(np.concatenate([[True], (c.cols["qhash"][o][1:] != c.cols["qhash"][o][:-1]) | (c.cols["h2"][o][1:] != c.cols["h2"][o][:-1])]))
    assert sum(1 for j in starts.tolist() if j < 256 and j + 256 in starts and j + 512 in starts) > 30
    out.append(c)
    return out


def _listed_cases():
    out = []
    # two listed buckets that are neighbours in bucket order (big_idx: 2 * lo, slots <= 2 m)
    n = 11 * PB_MEAN
    b = Builder("listed_two_neighbouring_buckets", n)
    b.pairs(4, 2049).mixed(5, 2049).mixed(9, n - 4098)
    out.append(b.build(1_000_000, dict(fill={4: 2049, 5: 2049, 9: n - 4098}, path={4: "listed", 5: "listed", 9: "set"}, listed=[4, 5]), tags=("sanitize",)))
    # m = 4 096 (a power of two: no padding) and 4 097 (8 192 slots of its 8 194)
    n = 22 * PB_MEAN
    b = Builder("listed_buckets_of_4096_and_4097", n)
    b.mixed(3, 4096).mixed(10, 4097).mixed(21, n - 8193)
    out.append(b.build(3000, dict(fill={3: 4096, 10: 4097, 21: n - 8193}, path={3: "listed", 10: "listed", 21: "set"}, listed=[3, 10]), tags=("sanitize",)))
    # 65 listed buckets of 2 049: more than frag_replay_big_kernel has workgroups (workgroup 0 takes the first and the 65th)
    n = 347 * PB_MEAN
    b = Builder("listed_65_buckets", n)
    which = list(range(0, 320, 5)) + [346]
    assert len(which) == BIG_GRID + 1
    for bk in which:
        b.pairs(bk, 2049)
    b.mixed(171, n - 65 * 2049)
    fill = {bk: 2049 for bk in which}; fill[171] = n - 65 * 2049
    path = {bk: "listed" for bk in which}; path[171] = "set"
    out.append(b.build(1_000_000, dict(fill=fill, path=path, listed=which)))
    return out


def _limit_case(n_listed):
    """PB_BIG_MAX on either side: 1 024 listed buckets of 2 049 candidates (results equal the reference), 1 025 (RSQC_ERR_CAPACITY, no partial
    result).  About 2.1 M candidates: the smallest input that reaches the limit.  Built from arrays; on the host the partition kernels alone
    (the replay of a thousand in-memory sorts is the device's part)."""
    n = n_listed * 2049
    nb = n_buckets(n)
    name = "listed_limit_%d_buckets" % n_listed
    b = Builder(name, n)
    which = np.unique(np.linspace(0, nb - 1, n_listed).astype(np.int64))
    assert len(which) == n_listed
    for bk in which.tolist():
        b.pairs(bk, 2049)
    e = dict(n_buckets=nb, listed=which.tolist(), error=0 if n_listed <= PB_BIG_MAX else abi.ERR_CAPACITY)
    return b.build(5000, e, emulate="partition", slow_device=True)


def _select_cases():
    out = []
    n = 2 * PB_MEAN + 40
    base = Builder("select_base", n, one_interval=True).pairs(0, 410, sure=True).mixed(1, n - 410).build(1_000_000, {})
    ns = len(base.reference()[0])
    assert ns > 300
    for label, ms in (("0", 0), ("1", 1), ("ns_minus_1", ns - 1), ("ns", ns), ("ns_plus_1", ns + 1)):
        e = dict(n_buckets=2, samples=ns, kept=min(ns, ms))
        if ms:
            e["last_kept"] = base.reference()[0][min(ns, ms) - 1][0]
        out.append(Case("select_max_samples_%s" % label, base.cols, ms, e, rec=base.rec, tags=("sanitize",) if ms in (0, 1, ns) else ()))
    # the wanted rank exactly on a digit's cumulative count: as many samples as complete below file index 512 (digits 0 and 1 at shift 8
    # together: the pick must stop AT digit 1 with its whole count still wanted)
    n = 4 * PB_MEAN
    big = Builder("select_rank", n, one_interval=True)
    for bk in range(4):
        big.pairs(bk, PB_MEAN, sure=True)
    c0 = big.build(1_000_000, {})
    files = [f for f, _ in c0.reference()[0]]
    below = sum(1 for f in files if f < 512)
    assert 0 < below < len(files) and any(f >= 512 for f in files)
    out.append(Case("select_rank_on_a_digits_cumulative_count", c0.cols, below, dict(samples=len(files), kept=below, last_kept=files[below - 1]), rec=c0.rec))
    assert files[below - 1] >> 8 == 1
    at255 = [i for i, f in enumerate(files) if f & 255 == 255]
    assert at255, "no sample completes at a file index whose low byte is 255"
    r = at255[len(at255) // 2]
    out.append(Case("select_digit_255_is_the_answer", c0.cols, r + 1, dict(samples=len(files), kept=r + 1, last_kept=files[r]), rec=c0.rec))
    # file indices of 2^56 and more that differ only in their top byte (the first pass: shift 56, no higher digits to compare).  Emulation
    # only: on the device a file index is a record's rank in the file
    m = 200
    c = Builder("select_top_byte", m, one_interval=True).pairs(0, m, sure=True).build(37, {})
    cols = dict(c.cols)
    cols["file_index"] = ((cols["file_index"] + np.uint64(1)) << np.uint64(56)) | np.uint64(0x00ABCDEF01234567)
    top = Case("select_file_indices_differ_in_the_top_byte_only", cols, 37, dict(n_buckets=1, samples=100, kept=37), emulate="full", device=False)
    assert top.reference()[1][-1][0] >> 56 > 37
    top.expect["last_kept"] = top.reference()[1][-1][0]
    out.append(top)
    return out


def _pairs_with_sizes(name, sizes, extra=0, **kw):
    """one sure pair per size (the completing record carries it), `extra` ordinary candidates beside them"""
    n = 2 * len(sizes) + extra
    b = Builder(name, n, one_interval=True)
    per = np.zeros(2 * len(sizes), np.int64); per[1::2] = sizes; per[0::2] = 55
    nb = b.nb
    cut = [(len(sizes) * k) // nb for k in range(nb + 1)]
    for bk in range(nb):
        k = cut[bk + 1] - cut[bk]
        if k:
            b.add(bk, [2] * k, sure=True, size=per[2 * cut[bk]:2 * cut[bk + 1]])
    if extra:
        b.add(0, [1] * extra)
    return b


def _size_cases():
    out = []
    T = ("sanitize",)
    top31 = (1 << 31) - 1
    sizes = [1, 4095, 4096, SIZE_TABLE - 1, SIZE_TABLE, top31, SIZE_TABLE, 300, 300, 4095]
    out.append(_pairs_with_sizes("size_values_at_the_lds_and_table_edges", sizes).build(
        1_000_000, dict(samples=10, top=SIZE_TABLE - 1, beyond=[SIZE_TABLE, SIZE_TABLE, top31], distinct=7,
                        pairs=[(1, 1), (300, 2), (4095, 2), (4096, 1), (SIZE_TABLE - 1, 1), (SIZE_TABLE, 2), (top31, 1)]), tags=T))
    sizes = [SIZE_TABLE, SIZE_TABLE + 1, top31, SIZE_TABLE, 1 << 30]
    out.append(_pairs_with_sizes("size_every_kept_size_beyond_the_table", sizes).build(
        1_000_000, dict(samples=5, top=0, table_pairs=0, beyond=sorted(sizes), distinct=4), tags=T))
    for top in (1023, 1024):                                # used = top + 1 = 1 024 / 1 025 cells: one / two per thread of the compaction
        sizes = [top, 1, 2, top - 1, 512, 513, 1000, top] + list(range(3, 400, 7))
        out.append(_pairs_with_sizes("size_largest_%d" % top, sizes).build(1_000_000, dict(samples=len(sizes), top=top, distinct=len(set(sizes))), tags=T))
    for nd in (PAIRS_FIRST, PAIRS_FIRST + 1):               # the second read-back of run_fragment_sizes: the device's part
        sizes = list(range(100, 100 + nd))
        sizes[5] = SIZE_LDS + 7 if nd > PAIRS_FIRST else sizes[5]
        out.append(_pairs_with_sizes("size_%d_distinct" % nd, sizes + [150, 151]).build(1_000_000, dict(samples=nd + 2, distinct=nd), tags=T if nd > PAIRS_FIRST else ()))
    return out


def all_cases():
    return (_bucket_count_cases() + _scan_cases() + _set_cases() + _handover_cases() + _sort_cases() + _listed_cases() +
            [_limit_case(PB_BIG_MAX), _limit_case(PB_BIG_MAX + 1)] + _select_cases() + _size_cases())


_CASES = None


def cases():
    """the catalogue, built once"""
    global _CASES
    if _CASES is None:
        _CASES = all_cases()
        assert len({c.name for c in _CASES}) == len(_CASES)
    return _CASES


# ---------------------------------------------------------------- a case as records for the C ABI (device, oracle, the per-record emulation)
def annotation(case):
    """one contig, one gene with one exon over everything"""
    from rnaseqc_amd.model import Annotation
    hi = int(positions(case.rec)[-1]) + 2000
    return Annotation.from_rows(["c"], [dict(contig="c", type="gene", start=1, end=hi, strand="+", gene_id="G"),
                                         dict(contig="c", type="exon", start=1, end=hi, strand="+", gene_id="G", exon_id="E")])


def bed(case):
    """one BED interval per interval of the case: from 100 bases in front of its first record to 200 behind its last"""
    from rnaseqc_amd.model import Bed
    pos, iv = positions(case.rec), case.rec["interval"]
    ks = sorted(set(iv.tolist()))
    return Bed.from_intervals([0] * len(ks), [int(pos[iv == k][0]) - 100 for k in ks], [int(pos[iv == k][-1]) + 200 for k in ks])


def batch(case):
    """A coordinate-sorted hash-only batch: record f is candidate f -- HQ, paired, its one block inside its interval.  A record that may
    complete a pair is the reverse mate of a forward one (flag 147), the others are forward mates of a reverse one (99); pos != mpos on all."""
    from rnaseqc_amd.model import Batch
    r = case.rec
    n = len(r["qhash"])
    pos = positions(r)
    z = np.zeros(n, np.int64)
    return Batch(pos=pos.astype(np.int32), mpos=(pos + 1).astype(np.int32), isize=np.where(r["ok"], -r["size"], r["size"]).astype(np.int32), qhash=r["qhash"].copy(),
                 cigar_off=np.arange(n, dtype=np.uint32), flag=np.where(r["ok"], 147, 99).astype(np.uint16), l_qseq=r["len"].astype(np.uint16),
                 mapq=(z + 255).astype(np.uint8), nm=z.astype(np.uint8), tagbits=(z + (abi.TB_HAS_NM | abi.TB_MTID_SAME)).astype(np.uint8),
                 n_cigar=(z + 1).astype(np.uint8), cigar=((r["len"] << 4) | abi.CIG_M).astype(np.uint32), seg_tid=np.zeros(1, np.int32),
                 seg_start=np.array([0, n], np.uint64), qhash2=r["h2"].copy())


def three_batches(b):
    """the batch cut into three unequal parts (a seventh, four sevenths, two sevenths of the records): file indices run across them"""
    n = b.n
    x, y = n // 7, (5 * n) // 7
    return [b.slice(0, x), b.slice(x, y), b.slice(y, n)]


def params(case):
    return abi.default_params(fragment_samples=case.max_samples)
