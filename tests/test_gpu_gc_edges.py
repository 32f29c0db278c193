"""GPU: the whole-path cases of tests/gc_cases.py through the device (rsqc_set_reference, the candidates pass of every batch, the pairing and
the GC replay at the end of the file), as one batch and cut in three.  The same expectations as on the emulation (tests/test_gc_host.py):
bins and out_of_range against the oracle, exon_gc of EVERY exon -- covered or not -- against tests/gc_ref.py, bit for bit."""
import numpy as np
import pytest

from rnaseqc_amd import engine
from tests import gc_cases, gc_ref
from tests.compare import assert_results_match

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", gc_cases.WHOLE_PATH)
def test_whole_path_case_on_the_device(name, oracle_lib):
    c = gc_cases.case(name)
    want = oracle_lib.run_oracle(c.params, c.ann, [c.batch], reference=c.ref)
    want_gc = gc_ref.exon_gc(c.ann, c.ref)
    covered = want.exon_cv_valid.astype(bool)
    assert covered.any()
    np.testing.assert_array_equal(want.exon_gc[covered], want_gc[covered])
    e = c.expect
    for batches in ([c.batch], gc_cases.three_unequal_batches(c.batch)):
        got = engine.run_engine(c.params, c.ann, batches, reference=c.ref)
        assert got.have_reference == 1
        np.testing.assert_array_equal(got.gc_bins, want.gc_bins)
        assert got.gc_out_of_range == want.gc_out_of_range
        np.testing.assert_array_equal(got.exon_gc, want_gc)                           # every exon, as doubles
        if "bins" in e:
            np.testing.assert_array_equal(got.gc_bins, gc_cases.bins_array(e["bins"]))
            assert got.gc_out_of_range == e.get("out_of_range", 0)
        assert int(got.gc_bins.sum()) + int(got.gc_out_of_range) == e["fragments"]
        assert_results_match(got, want)
