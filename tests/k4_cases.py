"""Named cases for the fragment count (rnaseqc_amd/csrc/rsqc_k4.h: frag_layout / frag_local / frag_count) in one-step neighbours of its
constants, and a plain reference.  tests/test_k4_edges_host.py runs them under the 64-lane emulation (tests/hostemu/k4_emu.cpp:
k4emu_run_pairs) and asserts the numbers each case states against the exported plan and fills; tests/test_gpu_k4_edges.py runs them as
records through the C ABI on the device.

A case is a stream of (gene, key, h2) pairs plus the shape K1 would have left it in (chunks + the dense region, or the dense form alone),
the sharers of the dense region and the two count grids.  `expect` holds what the case is named for:
    parts {gene: partitions}     fill {(gene, k): keys in partition k of the gene after frag_local; an int, or (lo, hi) where the window's
    outcome depends on the order in which two waves reach one slot}     small / large [(gene, k)]: the counting instance that takes it
    full_n: partitions listed for the larger instance     error: the error word (0, or abi.ERR_CAPACITY)

The reference is a set per gene of (key or GOLD, h2): no partitions, windows or tables."""
import numpy as np

from rnaseqc_amd import abi

PART_READS, SUB_CAP, PART_SLOTS = 1024, 2048, 4096        # rsqc_device.h: RSQC_K4_*
COUNT_THREADS, WIN, PASS, LANES, LAYOUT_GENES = 256, 2048, 2048, 64, 1024
GOLD = 0x9e3779b97f4a7c15                                 # what a key of 0 is counted as (frag_local_kernel; the oracle does the same)
M32 = 0xFFFFFFFF
MUL = 0x9E3779B1


# ---------------------------------------------------------------- the kernels' hashes, restated
def part_hash(key):
    """frag_part_hash: from the key's HIGH word (numpy, any shape)."""
    h = (np.asarray(key, np.uint64) >> np.uint64(32)).astype(np.uint64)
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(0x2C1B3C6D)) & np.uint64(M32)
    h ^= h >> np.uint64(12)
    return h


def part_of(key, parts):
    """partition of a key inside a gene of `parts` partitions"""
    key = np.asarray(key, np.uint64)
    return ((part_hash(key) * np.uint64(parts)) >> np.uint64(32)).astype(np.int64) if parts > 1 else np.zeros(key.shape, np.int64)


def set_slot(key, slots):
    """first slot of a key in a counting set of `slots` slots (frag_count_kernel: insert)"""
    return (((int(key) & M32) * MUL & M32) >> 16) & (slots - 1)


def gene_mix(g):
    return ((g << 32) | (g * MUL & M32)) & 0xFFFFFFFFFFFFFFFF


def win_slot(g, key):
    """slot of the pair in frag_local_kernel's direct-mapped window"""
    lk = (int(key) or GOLD) ^ gene_mix(int(g))
    lk = lk or 1
    return ((((lk ^ (lk >> 32)) & M32) * MUL & M32) >> 12) & (WIN - 1)


def layout(reads):
    """The plan of the header comment of rsqc_k4.h from the genes' counted reads: a gene of n reads owns ceil(n / PART_READS) partitions,
    each of capacity n (one partition) or SUB_CAP; its lists start at a multiple of 16 entries, genes in order.
    Returns (part_first[G + 1], ginfo[G, 4] = {first, parts, cap, offset / 16}, part_info[P, 4] = {gene, cap, offset lo, offset hi})."""
    pf, gi, pi = [], [], []
    off = 0
    for g, n in enumerate(int(x) for x in reads):
        parts = -(-n // PART_READS)
        cap = n if parts == 1 else SUB_CAP                  # (a gene without reads: no partition, no space; its row still says SUB_CAP)
        pf.append(len(pi)); gi.append((len(pi), parts, cap, off >> 4))
        for k in range(parts):
            o = off + k * cap
            pi.append((g, cap, o & M32, o >> 32))
        off += (parts * cap + 15) & ~15
    pf.append(len(pi))
    return np.array(pf, np.int64), np.array(gi, np.int64).reshape(-1, 4), np.array(pi, np.int64).reshape(-1, 4)


class Case:
    def __init__(self, name, n_genes, gene, key, h2=None, counts=None, chunk_cap=None, slow_cap=None, sharers=2, grids=(3, 2), expect=None,
                 tags=(), device=True, emulate=True, k1_grids=()):
        self.name, self.n_genes = name, int(n_genes)
        self.gene = np.asarray(gene, np.uint32); self.key = np.asarray(key, np.uint64)
        self.h2 = np.zeros(len(self.gene), np.uint32) if h2 is None else np.asarray(h2, np.uint32)
        self.has_h2 = h2 is not None
        n = len(self.gene)
        assert len(self.key) == n and len(self.h2) == n and (n == 0 or int(self.gene.max()) < n_genes)
        if counts is None:                                  # three unequal chunks and a dense region of an eighth
            s = n // 8; a = n // 2
            counts = [a, n - a - s, 0, s]
        assert sum(counts) == n
        self.counts = [int(c) for c in counts]
        self.chunk_cap = int(chunk_cap if chunk_cap is not None else (max(self.counts[:-1]) + 3 if len(self.counts) > 1 else 0))
        self.slow_cap = int(slow_cap if slow_cap is not None else self.counts[-1] + (5 if len(self.counts) > 1 else 0))
        self.sharers, self.grids = int(sharers), (int(grids[0]), int(grids[1]))
        self.expect = dict(expect or {})
        self.tags = frozenset(tags)                         # "setaside" / "window": run under more schedules
        self.device = device                                # False: emulation only (the case says why)
        self._reference = None
        self.emulate = emulate                              # False: device only (the case says why)
        self.k1_grids = tuple(k1_grids)                     # chunk-shaped: also with RSQC_K1_GRID = these on the device

    @property
    def reads(self):
        return np.bincount(self.gene, minlength=self.n_genes).astype(np.int64)

    def reference(self):
        """distinct (key or GOLD, h2) per gene"""
        if self._reference is None:
            self._reference = self._count_sets()
            self._reference.setflags(write=False)
        return self._reference

    def _count_sets(self):
        sets = [set() for _ in range(self.n_genes)]
        for g, k, h in zip(self.gene.tolist(), self.key.tolist(), self.h2.tolist()):
            sets[g].add((k or GOLD, h))
        return np.array([len(s) for s in sets], np.int64)

    def __repr__(self):
        return self.name


# ---------------------------------------------------------------- key makers (every case has its own seeded generator)
def _rng(name):
    return np.random.default_rng(int.from_bytes(name.encode(), "little") % (1 << 63))


def keys(rng, n, parts=1, part=None, lo=None, avoid=()):
    """n distinct non-zero keys; with `part`: all in that partition of a gene of `parts` partitions (rejection sampling of high words);
    lo: the low word of every key (the high words then differ); avoid: (gene, window slot) pairs no key may land on."""
    out = np.zeros(0, np.uint64)
    while len(out) < n:
        m = max(64, (n - len(out)) * (2 * parts if part is not None else 1) * 2)
        hi = rng.integers(1, 1 << 32, m, dtype=np.uint64)
        low = rng.integers(1, 1 << 32, m, dtype=np.uint64) if lo is None else np.full(m, lo, np.uint64)
        k = (hi << np.uint64(32)) | low
        if part is not None:
            k = k[part_of(k, parts) == part]
        for g, ws in avoid:
            k = k[np.array([win_slot(g, x) != ws for x in k.tolist()], bool)] if len(k) else k
        out = np.unique(np.concatenate([out, k]))
    return rng.permutation(out)[:n]


def _cat(blocks):
    """[(gene, keys[, h2])...] in stream order -> gene, key, h2 arrays"""
    g = np.concatenate([np.full(len(b[1]), b[0], np.uint32) for b in blocks]) if blocks else np.zeros(0, np.uint32)
    k = np.concatenate([np.asarray(b[1], np.uint64) for b in blocks]) if blocks else np.zeros(0, np.uint64)
    h = np.concatenate([np.asarray(b[2], np.uint32) if len(b) > 2 else np.zeros(len(b[1]), np.uint32) for b in blocks]) if blocks else np.zeros(0, np.uint32)
    return g, k, h


def _shuffled(rng, g, k, h):
    o = rng.permutation(len(g))
    return g[o], k[o], h[o]


def _genes_of_reads(name, reads, **kw):
    """genes with the given numbers of reads, all names distinct, stream shuffled"""
    rng = _rng(name)
    g, k, h = _cat([(i, keys(rng, n)) for i, n in enumerate(reads) if n])
    g, k, h = _shuffled(rng, g, k, h)
    return Case(name, len(reads), g, k, **kw)


# ---------------------------------------------------------------- the catalogue
def _layout_cases():
    out = []
    reads = [1, 0, 15, 16, 17, 0, 0, 1023, 1024, 1025, 2048, 2049, 0, 3]
    out.append(_genes_of_reads("layout_gene_reads_at_the_16_1024_2048_edges", reads,
                               expect=dict(parts={0: 1, 1: 0, 2: 1, 3: 1, 4: 1, 7: 1, 8: 1, 9: 2, 10: 2, 11: 3, 12: 0, 13: 1}, n_parts=14)))
    for ng in (1, 63, 64, 65, 1023, 1024, 1025):            # a two-partition gene at n_genes - 1, single reads before it
        reads = [0] * ng
        reads[ng - 1] = 1025
        for i in range(0, ng - 1, max(1, ng // 7)):
            reads[i] = 1 + i % 3
        out.append(_genes_of_reads("layout_n_genes_%d" % ng, reads, expect=dict(parts={ng - 1: 2})))
    reads = [0] * 1100
    for i in (63, 64, 1023, 1024):
        reads[i] = 1025
    for i in (0, 62, 65, 1022, 1025):
        reads[i] = 1
    reads[1099] = 1030
    out.append(_genes_of_reads("layout_multi_partition_genes_at_the_wave_and_workgroup_seams", reads,
                               expect=dict(parts={63: 2, 64: 2, 1023: 2, 1024: 2, 1099: 2}, n_parts=15)))
    # more than 64 partitions: the wave's walk over a gene's partitions takes a second (third) round.  Most of the reads repeat a few
    # hundred names (the plan depends on the reads alone), so that the emulation spends its time on the layout, not on the sets
    for parts in (65, 66, 129):
        name = "layout_gene_of_%d_partitions" % parts
        rng = _rng(name)
        n = (parts - 1) * PART_READS + 1
        pool = keys(rng, 300)
        g, k, h = _cat([(0, keys(rng, 5)), (1, pool[rng.integers(0, 300, n)]), (2, keys(rng, 17)), (3, keys(rng, 1025))])
        out.append(Case(name, 4, g, k, counts=[n // 2, len(g) - n // 2 - 1000, 1000], sharers=3, grids=(7, 2), expect=dict(parts={1: parts, 3: 2}, n_parts=parts + 4)))
    # more than 64 layout workgroups: the sum of the earlier workgroups' totals takes a second round.  Emulation only: 65 537 single-exon
    # genes are a 20 MB annotation and seconds of host set-up per run on the device for a loop the emulation runs line for line
    reads = [0] * 65537
    reads[0] = 1; reads[40000] = 2; reads[65535] = 1; reads[65536] = 1025
    for i in range(1, 65, 7):
        reads[i * 1024 - 1] = 1 + i % 2                     # a counted gene at the end of earlier workgroups
    out.append(_genes_of_reads("layout_65537_genes_counted_gene_in_the_last_workgroup", reads, expect=dict(parts={65536: 2, 65535: 1, 0: 1}), device=False))
    # ... and that second round is taken from workgroup 65 on (lane 0 then adds the totals of workgroups 0 AND 64): 66 562 genes, counted
    # genes in workgroups 64 and 65
    reads = [0] * 66562
    reads[3] = 2; reads[64 * 1024 + 5] = 1025; reads[65 * 1024 - 1] = 17; reads[65 * 1024] = 1; reads[66561] = 1030
    out.append(_genes_of_reads("layout_66562_genes_counted_genes_in_workgroups_64_and_65", reads, expect=dict(parts={64 * 1024 + 5: 2, 66561: 2}, n_parts=7), device=False))
    return out


def _capacity_cases():
    out = []
    E = abi.ERR_CAPACITY
    rng = _rng("cap")
    g, k, h = _cat([(0, keys(rng, 3)), (1, keys(rng, 2048, 2, 0))])
    out.append(Case("capacity_2048_names_in_partition_0_of_2", 2, g, k, expect=dict(parts={1: 2}, fill={(1, 0): 2048, (1, 1): 0}, large=[(1, 0)], full_n=1)))
    g, k, h = _cat([(0, keys(rng, 3)), (1, keys(rng, 2049, 3, 1)), (2, keys(rng, 4))])
    out.append(Case("capacity_2049_names_in_partition_1_of_3", 3, g, k, expect=dict(parts={1: 3}, fill={(1, 1): 2049}, error=E)))
    g, k, h = _cat([(0, keys(rng, 3)), (1, keys(rng, 4)), (2, keys(rng, 2049, 3, 2))])
    out.append(Case("capacity_2049_names_in_the_last_list_of_the_table", 3, g, k, expect=dict(parts={2: 3}, fill={(2, 2): 2049}, error=E)))
    for n in (2048, 2049):                                  # a caller's weak hash: 1..n, the high word constant -> one partition
        g, k, h = _cat([(0, keys(rng, 3)), (1, np.arange(1, n + 1, dtype=np.uint64))])
        p = int(part_of(np.uint64(1), -(-n // PART_READS)))
        out.append(Case("capacity_weak_hash_1_to_%d" % n, 2, g, k,
                        expect=dict(fill={(1, p): n}, error=0 if n == 2048 else E, **(dict(large=[(1, p)], full_n=1) if n == 2048 else {}))))
    # the low word constant: every key starts at ONE slot of the set, the linear probe runs the whole partition
    g, k, h = _cat([(0, keys(rng, 1024, lo=0x1234)), (1, keys(rng, 2))])
    out.append(Case("probe_1024_keys_from_one_slot_small_instance", 2, g, k, expect=dict(parts={0: 1}, fill={(0, 0): 1024}, small=[(0, 0)], full_n=0)))
    g, k, h = _cat([(0, keys(rng, 2)), (1, keys(rng, 2048, 2, 1, lo=0xBEEF0001))])
    out.append(Case("probe_2048_keys_from_one_slot_large_instance", 2, g, k, expect=dict(parts={1: 2}, fill={(1, 0): 0, (1, 1): 2048}, large=[(1, 1)], full_n=1)))
    return out


def _instance_cases():
    rng = _rng("instance")
    # partitions of multi-partition genes with exactly 1, 32, 33, 64 keys (sets of 64, 64, 128, 128 slots), 1024 (the small instance at
    # KPT x 256 keys exactly), 1025 (listed), 2047 and 2048 (the large instance at half load exactly)
    spec = {1: [(0, 1), (1, 1024)], 2: [(0, 32), (1, 1024)], 3: [(0, 33), (1, 1024)], 4: [(0, 64), (1, 1024)], 5: [(0, 1), (1, 1025)],
            6: [(0, 2047), (1, 1), (2, 1)], 7: [(0, 2048), (1, 1), (2, 1)]}
    blocks = [(0, keys(rng, 2))]
    fill, small, large = {}, [(0, 0)], []
    for g, ps in spec.items():
        for p, n in ps:
            blocks.append((g, keys(rng, n, len(ps), p)))
            fill[(g, p)] = n
            (large if n > 1024 else small).append((g, p))
    g, k, h = _shuffled(rng, *_cat(blocks))
    return [Case("instance_partitions_of_1_32_33_64_1024_1025_2047_2048_keys", 8, g, k, grids=(4, 2),
                 expect=dict(parts={g: len(ps) for g, ps in spec.items()}, fill=fill, small=small, large=large, full_n=3))]


def _pair_key(rng, n=1, **kw):
    return [int(x) for x in keys(rng, n, **kw)]


def _setaside_cases():
    out = []
    E = abi.ERR_CAPACITY
    rng = _rng("setaside")
    T = ("setaside",)
    X, Y = _pair_key(rng, 2)
    g, k, h = _cat([(0, keys(rng, 2)), (1, [X, X, Y, Y, X, Y], [5, 7, 5, 7, 9, 9]), (2, keys(rng, 3))])
    out.append(Case("setaside_two_keys_under_the_same_second_hashes", 3, g, k, h, counts=[len(g), 0], tags=T, expect=dict(fill={(1, 0): 6})))
    # the duplicates of a set-aside name in another workgroup's chunk (no window between them): the list holds the entry twice
    fill_a, fill_b = keys(rng, 2100), keys(rng, 2100)
    g, k, h = _cat([(1, [X, X], [1, 2]), (0, fill_a), (0, fill_b), (1, [X, X, X], [2, 2, 1])])
    out.append(Case("setaside_duplicates_further_apart_than_the_window", 2, g, k, h, counts=[2102, 0, 2103, 0], tags=T,
                    expect=dict(fill={(1, 0): (4, 5)}, parts={0: 5})))
    Z = (_pair_key(rng)[0] & ~M32)                          # low word 0: the owner sits in slot 0 of the set
    assert set_slot(Z, 64) == 0
    g, k, h = _cat([(0, keys(rng, 2)), (1, [Z, Z, Z], [3, 4, 4]), (1, keys(rng, 9))])
    out.append(Case("setaside_owner_in_slot_0", 2, g, k, h, counts=[len(g), 0], tags=T, expect=dict(fill={(1, 0): (11, 12)})))

    def names(gene, key, n, base=0):
        return (gene, [key] * n, [base + 11 * i + 1 for i in range(n)])
    # two count workgroups over eight single-partition genes: workgroup 0 takes partitions 0 2 4 6, workgroup 1 takes 1 3 5 7.
    # set-aside entries in two consecutive partitions of workgroup 0 (0, 2) and in workgroup 1's last (7)
    ks = _pair_key(rng, 8)
    blocks = [names(0, ks[0], 3), names(2, ks[2], 4), names(7, ks[7], 2)] + [(i, keys(rng, 2 + i)) for i in range(8)]
    g, k, h = _shuffled(rng, *_cat(blocks))
    out.append(Case("setaside_in_consecutive_partitions_and_in_the_last_of_a_workgroup", 8, g, k, h, grids=(2, 1), tags=T,
                    expect=dict(n_parts=8, fill={(0, 0): 5, (2, 0): 8, (7, 0): 11})))
    # one count workgroup: set-aside entries, then an EMPTY partition and the other instance's partition (gene 1: 1025 names all in its
    # partition 1), then set-aside entries again, then the other instance's again and an empty partition at the end (gene 4)
    blocks = [names(0, ks[0], 5), (1, keys(rng, 1025, 2, 1)), names(2, ks[2], 3), (3, keys(rng, 4)), names(3, ks[3], 2), (4, keys(rng, 1025, 2, 0))]
    g, k, h = _shuffled(rng, *_cat(blocks))
    out.append(Case("setaside_followed_by_empty_and_listed_partitions_in_one_workgroup", 5, g, k, h, grids=(1, 1), tags=T,
                    expect=dict(n_parts=7, fill={(0, 0): 5, (1, 0): 0, (1, 1): 1025, (2, 0): 3, (3, 0): 6, (4, 0): 1025, (4, 1): 0},
                                large=[(1, 1), (4, 0)], full_n=2)))
    # the 33 / 34 edge in a partition that is not the first of its workgroup (partition 2 of workgroup 0 of 2)
    for n in (33, 34):
        blocks = [(0, keys(rng, 3)), names(0, ks[0], 2), (1, keys(rng, 2)), names(2, ks[2], n), (3, keys(rng, 2))]
        g, k, h = _shuffled(rng, *_cat(blocks))
        out.append(Case("setaside_%d_names_of_one_key_in_a_workgroups_second_partition" % n, 4, g, k, h, grids=(2, 1), tags=T,
                        expect=dict(fill={(2, 0): n}, error=0 if n == 33 else E)))
    # the deferred settle with the count's grid smaller than the partitions: 40 genes of one read (a few of two names under one key),
    # 16 workgroups: set-aside names in partitions i and i + 16 of one workgroup (3 and 19), and in a workgroup's last (39)
    blocks = [(i, keys(rng, 1)) for i in range(40)] + [names(3, ks[3], 3), names(19, ks[1], 2), names(39, ks[5], 4)]
    g, k, h = _shuffled(rng, *_cat(blocks))
    out.append(Case("setaside_in_partitions_i_and_i_plus_grid", 40, g, k, h, grids=(16, 1), tags=T, expect=dict(n_parts=40, fill={(3, 0): 4, (19, 0): 3, (39, 0): 5})))
    return out


def _window_cases():
    out = []
    rng = _rng("window")
    T = ("window",)
    # key ^ mix(gene) == 0, no second hashes: the word is stored as 1, or the first occurrence would be dropped against the cleared window.
    # gene 3's one name: the first pair of chunk 0, its mate later in the run (dropped), and again in the middle of chunk 2 (another
    # workgroup's cleared window: kept).  (One gene only: the window word is 64 bits of key ^ mix(gene), so a second gene's pair whose
    # word is 0 too is the same word -- DESIGN.md section 5.)
    s1 = win_slot(3, gene_mix(3))                           # (the slot of the word 1; a word of 0 would go to slot 0)
    assert s1 != 0
    a, b = keys(rng, 700, avoid=[(0, 0), (0, s1)]), keys(rng, 900, avoid=[(0, 0), (0, s1)])
    g, k, h = _cat([(3, [gene_mix(3)]), (0, a), (3, [gene_mix(3)]), (0, b[:400]), (3, [gene_mix(3)]), (0, b[400:])])
    out.append(Case("window_word_zero_first_of_a_chunk_and_later", 6, g, k, counts=[702, 0, 901, 0], tags=T, k1_grids=(1, 2, 3),
                    expect=dict(fill={(3, 0): 2})))
    g, k, h = _cat([(0, keys(rng, 5)), (2, [0, GOLD, 0, GOLD]), (1, keys(rng, 5))])
    out.append(Case("window_key_0_beside_the_key_it_is_counted_as", 3, g, k, counts=[len(g), 0], tags=T, expect=dict(fill={(2, 0): 1})))
    K = _pair_key(rng)[0]
    g, k, h = _cat([(0, keys(rng, 3)), (1, [K]), (2, [K]), (1, [K]), (2, [K]), (3, [K, K])])
    out.append(Case("window_one_name_counted_to_two_genes_back_to_back", 4, g, k, counts=[len(g), 0], tags=T, expect=dict(fill={(1, 0): 1, (2, 0): 1, (3, 0): 1})))
    # mates d pairs apart in one workgroup's window: gene 1 with nothing on their slot between them (the second is dropped), gene 2 with
    # a pair of gene 3 landing on their slot between them (the second survives unless it reaches the slot first; the count is exact)
    for d in (1, 2047, 2048, 2049):
        A, B = _pair_key(rng, 2)
        sa, sb = win_slot(1, A), win_slot(2, B)
        while sb == sa:
            B = _pair_key(rng)[0]; sb = win_slot(2, B)
        I = next(x for x in _pair_key(rng, 40000) if win_slot(3, x) == sb)
        n = d + 40
        fk = keys(rng, n, avoid=[(0, sa), (0, sb)])
        gene = np.zeros(n, np.uint32); key = fk.copy()
        gene[5] = 1; key[5] = A; gene[5 + d] = 1; key[5 + d] = A
        fill = {(1, 0): 1}
        if d > 1:
            gene[7] = 2; key[7] = B; gene[7 + d] = 2; key[7 + d] = B
            gene[7 + d // 2] = 3; key[7 + d // 2] = I
            fill[(2, 0)] = (1, 2)
        out.append(Case("window_mates_%d_pairs_apart" % d, 4, gene, key, counts=[n, 0], tags=T, k1_grids=(1,), expect=dict(fill=fill)))
    # mates on either side of a chunk boundary inside one workgroup's two-chunk run (gene 1: dropped) and across two workgroups (gene 2: kept)
    A, B = _pair_key(rng, 2)
    f = keys(rng, 90, avoid=[(0, win_slot(1, A)), (0, win_slot(2, B))])
    g, k, h = _cat([(0, f[:30]), (1, [A]), (1, [A]), (0, f[30:60]), (2, [B]), (2, [B]), (0, f[60:])])
    out.append(Case("window_mates_across_a_chunk_boundary_inside_and_between_workgroups", 3, g, k, counts=[31, 32, 31, 0], chunk_cap=40, tags=T,
                    k1_grids=(1, 2, 3), expect=dict(fill={(1, 0): 1, (2, 0): 2})))
    return out


def _chunk_cases():
    out = []
    reads = [5, 0, 300, 1025, 17, 1024, 2049, 1]            # every gene's names distinct: a pair read twice overflows a list of exact capacity
    n = sum(reads)
    for nc in (1, 2, 3):                                    # (3: the odd tail of a two-chunk run)
        cnt = [n // nc + (1 if c < n % nc else 0) for c in range(nc)]
        cnt[-1] -= 333
        out.append(_genes_of_reads("chunks_%d_and_a_dense_region" % nc, reads, counts=cnt + [333], k1_grids=(1, 2, 3)))
    out.append(_genes_of_reads("chunks_empty_first", reads, counts=[0, n - 100, 100], k1_grids=(2,)))
    out.append(_genes_of_reads("chunks_empty_second", reads, counts=[n - 100, 0, 50, 50]))
    out.append(_genes_of_reads("chunks_all_empty_pairs_in_the_dense_region_only", reads, counts=[0, 0, 0, n], sharers=3))
    for run in (2047, 2048, 2049):
        out.append(_genes_of_reads("chunks_run_of_%d" % run, [run - 1030, 1025, 5], counts=[run, 0], k1_grids=(1,)))
    out.append(_genes_of_reads("chunks_1024_and_1024_the_seam_of_a_run", [1000, 1040, 8], counts=[1024, 1024, 0], chunk_cap=1031, k1_grids=(2,)))
    out.append(_genes_of_reads("chunks_filled_to_their_capacity", [700, 1030, 70], counts=[600, 600, 600, 0], chunk_cap=600, slow_cap=0))
    nd = 3 * PASS + 5                                       # four passes of the dense form
    for sh in (7, 4, 1):
        out.append(_genes_of_reads("dense_form_4_passes_%d_sharers" % sh, [nd - 1100, 1030, 70], counts=[nd], sharers=sh))
    return out


def _device_only_cases():
    # about 17 000 genes of one read: the device's count grid stops at 16 384 workgroups, so workgroups 0 .. n - 16 385 take TWO partitions
    # each, i and i + 16 384 -- the deferred settle on real barriers.  Set-aside names (one key, several second hashes) in both partitions
    # of a workgroup, in its first only and in its second only.  (Under the emulation the same walk is setaside_in_partitions_i_and_i_plus_grid:
    # 16 384 emulated workgroups would take minutes.)
    rng = _rng("grid")
    G, step = 17000, 16384
    ks = _pair_key(rng, 6)
    blocks = [(i, keys(rng, 1)) for i in range(G)]
    for j, (gene, n) in enumerate([(5, 3), (5 + step, 2), (100, 4), (300 + step, 3), (G - 1 - step, 2), (G - 1, 5)]):
        blocks.append((gene, [ks[j]] * n, [7 * i + 3 for i in range(n)]))
    g, k, h = _shuffled(rng, *_cat(blocks))
    return [Case("grid_of_16384_workgroups_over_17000_partitions_with_set_aside_names", G, g, k, h, tags=("setaside",), emulate=False, expect=dict(n_parts=G))]


def all_cases():
    return _layout_cases() + _capacity_cases() + _instance_cases() + _setaside_cases() + _window_cases() + _chunk_cases() + _device_only_cases()


_CASES = None


def cases():
    """the catalogue, built once"""
    global _CASES
    if _CASES is None:
        _CASES = all_cases()
        assert len({c.name for c in _CASES}) == len(_CASES)
    return _CASES


# ---------------------------------------------------------------- a case as records for the C ABI (device and oracle)
GENE_STEP, GENE_LENGTH, READ_LENGTH = 200, 160, 50


def annotation(case):
    """one single-exon gene per gene index, in index order, non-overlapping"""
    from rnaseqc_amd.model import Annotation
    rows = []
    for g in range(case.n_genes):
        lo = 1001 + g * GENE_STEP
        rows.append(dict(contig="c", type="gene", start=lo, end=lo + GENE_LENGTH - 1, strand="+", gene_id="G%05d" % g))
        rows.append(dict(contig="c", type="exon", start=lo, end=lo + GENE_LENGTH - 1, strand="+", gene_id="G%05d" % g, exon_id="E%05d" % g))
    return Annotation.from_rows(["c"], rows)


def batch(case):
    """One unpaired one-block read per pair, inside its gene, coordinate-sorted (a gene's reads keep their stream order); a hash-only batch:
    qhash = key, qhash2 = h2 where the case has second hashes."""
    from rnaseqc_amd.model import Batch
    n = len(case.gene)
    order = np.argsort(case.gene, kind="stable")
    gene = case.gene[order].astype(np.int64)
    first = np.searchsorted(gene, gene, side="left"); size = case.reads[gene]
    pos = 1000 + gene * GENE_STEP + ((np.arange(n) - first) * (GENE_LENGTH - READ_LENGTH)) // np.maximum(size, 1)
    z = np.zeros(n, np.int64)
    return Batch(pos=pos.astype(np.int32), mpos=(z - 1).astype(np.int32), isize=z.astype(np.int32), qhash=case.key[order], cigar_off=np.arange(n, dtype=np.uint32),
                 flag=z.astype(np.uint16), l_qseq=(z + READ_LENGTH).astype(np.uint16), mapq=(z + 255).astype(np.uint8), nm=z.astype(np.uint8),
                 tagbits=(z + abi.TB_HAS_NM).astype(np.uint8), n_cigar=(z + 1).astype(np.uint8), cigar=(z + ((READ_LENGTH << 4) | abi.CIG_M)).astype(np.uint32),
                 seg_tid=np.zeros(1, np.int32), seg_start=np.array([0, n], np.uint64), qhash2=case.h2[order].copy() if case.has_h2 else None)


def three_batches(b):
    """the batch cut into three unequal parts (a seventh, four sevenths, two sevenths of the records)"""
    n = b.n
    x, y = n // 7, (5 * n) // 7
    return [b.slice(0, x), b.slice(x, y), b.slice(y, n)]


def params(**kw):
    return abi.default_params(unpaired=1, **kw)
