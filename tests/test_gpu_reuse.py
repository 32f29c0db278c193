"""rsqc_clear_inputs through engine.py: one context, one annotation after another (other contigs, another gene count, a BED),
each result equal to the oracle's and to a fresh context's; nothing of the annotation before is left on the device."""
import numpy as np
import pytest

from rnaseqc_amd import abi, engine, synth
from tests.compare import assert_results_match

pytestmark = pytest.mark.gpu

CONTIGS_A = [("chrA", 900_000, 70), ("chrB", 500_000, 40)]
CONTIGS_B = [("c1", 1_200_000, 90), ("c2", 700_000, 55), ("c3", 400_000, 25)]


def _make_inputs():
    ann_a = synth.make_annotation(seed=11, contigs=CONTIGS_A)
    ann_b = synth.make_annotation(seed=12, contigs=CONTIGS_B)
    assert ann_a.to_struct().n_genes != ann_b.to_struct().n_genes
    batch_a = synth.make_reads(ann_a, 20000, seed=13, dup_frac=0.05, contig_lengths=np.array([c[1] for c in CONTIGS_A]))
    batch_b = synth.make_reads(ann_b, 24000, seed=14, dup_frac=0.05, contig_lengths=np.array([c[1] for c in CONTIGS_B]))
    return ann_a, batch_a, ann_b, batch_b, synth.make_bed(ann_b, min_len=250)


@pytest.fixture(scope="module")
def inputs():
    return _make_inputs()


def _pass(e, batch, parts=3):
    step = (batch.n + parts - 1) // parts
    for lo in range(0, batch.n, step):
        e.submit(batch.slice(lo, min(batch.n, lo + step)))
    return e.finalize()


def test_clear_then_another_annotation_matches_oracle_and_a_fresh_context(oracle_lib, inputs):
    ann_a, batch_a, ann_b, batch_b, bed_b = inputs
    p = abi.default_params()
    want_a = oracle_lib.run_oracle(p, ann_a, [batch_a])
    want_b = oracle_lib.run_oracle(p, ann_b, [batch_b], bed=bed_b)
    assert want_b.fragment_count.sum() > 50
    fresh_b = engine.run_engine(p, ann_b, [batch_b], bed=bed_b)
    e = engine.Engine(p)
    try:
        e.set_annotation(ann_a)
        assert_results_match(_pass(e, batch_a), want_a)
        e.clear_inputs()
        e.set_annotation(ann_b)
        e.set_bed(bed_b)
        got_b = _pass(e, batch_b)
        assert_results_match(got_b, want_b)
        assert_results_match(got_b, fresh_b)
        e.clear_inputs()                                         # ... and back: no BED this time
        e.set_annotation(ann_a)
        got_a = _pass(e, batch_a)
        assert_results_match(got_a, want_a)
        assert got_a.fragment_count.sum() == 0
    finally:
        e.close()


def test_second_annotation_without_a_clear_is_refused(inputs):
    ann_a, _, ann_b, _, _ = inputs
    e = engine.Engine(abi.default_params())
    try:
        e.set_annotation(ann_a)
        with pytest.raises(engine.EngineError) as err:
            e.set_annotation(ann_b)
        assert err.value.code == abi.ERR_ARG and "already set" in str(err.value)
    finally:
        e.close()


def test_clear_waits_for_the_batches_in_flight(oracle_lib, inputs):
    ann_a, batch_a, ann_b, batch_b, bed_b = inputs
    p = abi.default_params()
    want_b = oracle_lib.run_oracle(p, ann_b, [batch_b], bed=bed_b)
    e = engine.Engine(p)
    try:
        e.set_annotation(ann_a)
        step = batch_a.n // 3
        for k in range(3):                                       # asynchronous: uploads and kernels are queued when clear is called
            e.submit(batch_a.slice(k * step, (k + 1) * step))
        e.clear_inputs()
        e.set_annotation(ann_b)
        e.set_bed(bed_b)
        assert_results_match(_pass(e, batch_b), want_b)
    finally:
        e.close()


def _memory_cycles():
    """Runs in a process of its own (below): PyTorch's HIP runtime has to come up before the library's for mem_get_info to see
    the device."""
    import os
    import torch
    torch.cuda.init()
    torch.cuda.synchronize()
    ann_a, batch_a, ann_b, batch_b, bed_b = _make_inputs()
    MB = 1 << 20

    def in_use():
        free, total = torch.cuda.mem_get_info()
        return total - free

    # The HIP runtime reserves scratch memory for a hardware queue at the first launch of a kernel that needs it (the general
    # classify kernel: 624 B a lane, 327 MB for the chip's wave slots) and holds it for the life of the process, whatever the
    # library frees.  So that it is part of the reading after rsqc_create and not of what the clear is charged with, every
    # hardware queue of the process runs a pass first: as many contexts as there are queues, alive together so that their
    # streams spread over the queues, each run and then destroyed -- with no rsqc_clear_inputs anywhere.
    start = in_use()
    warm = [engine.Engine(abi.default_params()) for _ in range(int(os.environ.get("GPU_MAX_HW_QUEUES", "4")))]
    for w in warm:
        w.set_annotation(ann_b)
        w.set_bed(bed_b)
        _pass(w, batch_b)
        print("warm-up pass: %.1f MB in use above the start" % ((in_use() - start) / 1e6), flush=True)
    for w in warm:
        w.close()
    print("the HIP runtime keeps %.1f MB after %d contexts that ran a pass have been destroyed" % ((in_use() - start) / 1e6, len(warm)), flush=True)

    e = engine.Engine(abi.default_params())
    try:
        base = in_use()                                          # after rsqc_create, before any annotation
        held = 0
        left = []
        for k in range(8):
            ann, batch, bed = (ann_a, batch_a, None) if k % 2 == 0 else (ann_b, batch_b, bed_b)
            e.set_annotation(ann)
            if bed is not None:
                e.set_bed(bed)
            _pass(e, batch)
            held = in_use() - base
            e.clear_inputs()
            left.append(in_use() - base)
            print("cycle %d: %.1f MB held with the inputs set, %.1f MB after the clear" % (k, held / 1e6, left[-1] / 1e6), flush=True)
    finally:
        e.close()
    kept = base + left[-1] - in_use()                            # what rsqc_destroy still found to free after the last clear
    print("the cleared context still owned %.1f MB (freed by rsqc_destroy)" % (kept / 1e6), flush=True)
    assert left[-1] <= 64 * MB, left
    assert kept <= 64 * MB, kept                                 # kept but reusable (an arena, a rank table) counts like a leak
    # both kinds of input have been seen once after cycle 1: from there on a cycle allocates nothing that the pools do not
    # already hold, so six more cycles add nothing (2 MB: one page of the device allocator)
    assert left[-1] - left[1] <= 2 * MB, left
    assert held > left[-1]                                       # the clear released something


def test_clear_gives_the_device_memory_back():
    """Device memory in use after 8 clear/set cycles is within 64 MB of what it was after rsqc_create (read in the same process,
    before the first annotation): the 64 MB cover the per-batch buffer pools that the clear keeps on purpose; a leaked or kept
    annotation, rank table, coverage array, arena or stream set is far above it (the pair arena alone is 268 MB, the fragment
    arena 537 MB) or adds up cycle after cycle.

    The reading after rsqc_create is taken once the process's hardware queues have their scratch memory (see _memory_cycles):
    on an MI355X the runtime holds 327 MB a queue from the first general classify kernel on, rsqc_destroy or not, and a context
    measured without that kept 406.8 MB "in use" after every clear, 337.6 MB of them after its rsqc_destroy too.  The context's
    own part is two pair buffers of 17.7 MB, 3.3 MB of upload buffers, 1 MB of fragment buffers, the deferred list and the
    streams' own memory, about 52 MB (the 16.9 MB of Read-Length summaries go with the clear)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, "-c", "from tests.test_gpu_reuse import _memory_cycles; _memory_cycles()"], cwd=root,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    print(p.stdout.decode())
    assert p.returncode == 0, p.stdout.decode()
