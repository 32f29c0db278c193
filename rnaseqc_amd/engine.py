"""Host-side driver of the HIP hot path through the C ABI (include/rnaseqc_amd.h).

This is plumbing: it loads rnaseqc_amd/lib/librnaseqc_amd.so (built by
__graft_entry__.build() / rnaseqc_amd/csrc/Makefile) and forwards calls.  There is no
fallback of any kind: a missing library or a missing GPU raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RSQC_LIB") or os.path.join(_HERE, "lib", "librnaseqc_amd.so")   # RSQC_LIB: a diagnostic build (make prof)
_lib = None
_hip = None


class EngineError(RuntimeError):
    def __init__(self, code, msg=""):
        super().__init__("rnaseqc_amd error %d: %s" % (code, msg))
        self.code = code


def load_library():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise EngineError(abi.ERR_NO_DEVICE, "HIP library %s is missing; run __graft_entry__.build()" % LIB_PATH)
        lib = C.CDLL(LIB_PATH)
        vp = C.c_void_p
        lib.rsqc_create.argtypes = [C.POINTER(abi.Params), C.POINTER(vp)]
        lib.rsqc_destroy.argtypes = [vp]; lib.rsqc_destroy.restype = None
        lib.rsqc_set_annotation.argtypes = [vp, C.POINTER(abi.AnnotationStruct), vp]
        lib.rsqc_set_bed.argtypes = [vp, C.POINTER(abi.BedStruct)]
        lib.rsqc_set_reference.argtypes = [vp, C.POINTER(abi.ReferenceStruct)]
        lib.rsqc_submit.argtypes = [vp, C.POINTER(abi.BatchStruct)]
        lib.rsqc_wait.argtypes = [vp]
        lib.rsqc_upload.argtypes = [vp, C.POINTER(abi.BatchStruct), C.POINTER(C.c_int)]
        lib.rsqc_submit_resident.argtypes = [vp, C.c_int]
        lib.rsqc_release.argtypes = [vp, C.c_int]
        lib.rsqc_finalize.argtypes = [vp, C.POINTER(abi.ResultsStruct)]
        lib.rsqc_reset.argtypes = [vp]
        lib.rsqc_clear_inputs.argtypes = [vp]
        lib.rsqc_get_timing.argtypes = [vp, C.POINTER(abi.TimingStruct)]
        lib.rsqc_reset_timing.argtypes = [vp]
        lib.rsqc_device_accumulators.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_uint64), C.POINTER(vp), C.POINTER(C.c_uint64)]
        lib.rsqc_device_vectors.argtypes = [vp, C.POINTER(abi.DeviceRange * 3)]
        lib.rsqc_shard_summary.argtypes = [vp, C.POINTER(abi.ShardInfoStruct)]
        lib.rsqc_reduce_peer.argtypes = [vp, vp]
        lib.rsqc_reduce_group.argtypes = [C.POINTER(vp), C.c_int, C.POINTER(C.c_int)]
        lib.rsqc_group_create.argtypes = [C.POINTER(vp), C.c_int, C.POINTER(vp)]
        lib.rsqc_group_reduce.argtypes = [vp, C.POINTER(C.c_int)]
        lib.rsqc_group_info.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_char_p)]
        lib.rsqc_group_destroy.argtypes = [vp]; lib.rsqc_group_destroy.restype = None
        lib.rsqc_refresh_results.argtypes = [vp, C.POINTER(abi.ResultsStruct)]
        lib.rsqc_finalize_device.argtypes = [vp]
        lib.rsqc_host_alloc.argtypes = [C.c_size_t]; lib.rsqc_host_alloc.restype = vp
        lib.rsqc_host_free.argtypes = [vp]; lib.rsqc_host_free.restype = None
        lib.rsqc_strerror.argtypes = [C.c_int]; lib.rsqc_strerror.restype = C.c_char_p
        lib.rsqc_last_error.argtypes = [vp]; lib.rsqc_last_error.restype = C.c_char_p
        lib.rsqc_counter_name.argtypes = [C.c_int]; lib.rsqc_counter_name.restype = C.c_char_p
        lib.rsqc_version.restype = C.c_char_p
        lib.rsqc_qname_hash.argtypes = [C.c_char_p, C.c_size_t]; lib.rsqc_qname_hash.restype = C.c_uint64
        lib.rsqc_qname_hash2.argtypes = [C.c_char_p, C.c_size_t]; lib.rsqc_qname_hash2.restype = C.c_uint32
        lib.rsqc_decode_begin.argtypes = [vp, C.POINTER(abi.DecodeParams)]
        lib.rsqc_decode_submit.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint32, C.c_uint32, C.c_uint64, C.POINTER(abi.DecodeWindow)]
        lib.rsqc_decode_end.argtypes = [vp, C.POINTER(abi.DecodeInfo)]
        lib.rsqc_decode_begin_sam.argtypes = [vp, C.POINTER(abi.DecodeParams), C.POINTER(C.c_char_p)]
        lib.rsqc_decode_submit_text.argtypes = [vp, vp, C.c_uint64, C.POINTER(abi.DecodeWindow)]
        lib.rsqc_sort_begin.argtypes = [vp]
        lib.rsqc_sort_end.argtypes = [vp, C.POINTER(abi.SortInfo)]
        lib.rsqc_markdup_begin.argtypes = [vp]
        lib.rsqc_markdup_end.argtypes = [vp, C.POINTER(abi.MarkdupInfo)]
        lib.rsqc_markdup_verdicts.argtypes = [vp, C.c_uint64, C.c_uint64, C.POINTER(vp)]
        lib.rsqc_markdup_use_umi.argtypes = [vp]
        lib.rsqc_markdup_umi_end.argtypes = [vp, C.POINTER(abi.MarkdupUmiInfo)]
        lib.rsqc_markdup_umi_edits.argtypes = [vp, C.c_uint32]
        lib.rsqc_markdup_umi_group_end.argtypes = [vp, C.POINTER(abi.MarkdupUmiGroupInfo)]
        lib.rsqc_umi_pack.restype = C.c_uint64
        lib.rsqc_umi_pack.argtypes = [C.c_char_p, C.c_uint32]
        lib.rsqc_junctions_begin.argtypes = [vp]
        lib.rsqc_junctions_end.argtypes = [vp, C.POINTER(abi.JunctionTable)]
        lib.rsqc_track_begin.argtypes = [vp, C.c_int32, vp, C.POINTER(C.c_char_p)]
        lib.rsqc_track_end.argtypes = [vp, C.POINTER(abi.TrackInfo)]
        lib.rsqc_track_rows.argtypes = [vp, C.c_uint64, C.c_uint64] + [C.POINTER(vp)] * 4
        lib.rsqc_track_text.argtypes = [vp, C.c_uint64, C.c_uint64, C.POINTER(vp), C.POINTER(C.c_uint64)]
        lib.rsqc_genebody_begin.argtypes = [vp, C.c_int32] + [vp] * 5
        lib.rsqc_genebody_end.argtypes = [vp, C.POINTER(abi.GenebodyInfo)]
        lib.rsqc_genebody_sums.argtypes = [vp, C.c_uint32, C.c_uint32, C.POINTER(vp)]
        lib.rsqc_tin_begin.argtypes = [vp, C.c_int32] + [vp] * 4
        lib.rsqc_tin_end.argtypes = [vp, C.POINTER(abi.TinInfo)]
        lib.rsqc_tin_rows.argtypes = [vp, C.c_uint32, C.c_uint32, C.POINTER(vp)]
        lib.rsqc_cycles_begin.argtypes = [vp]
        lib.rsqc_cycles_add.argtypes = [vp, vp, vp, C.POINTER(abi.CycleInfo)]
        lib.rsqc_cycles_end.argtypes = [vp, C.POINTER(abi.CycleInfo), C.POINTER(vp), C.POINTER(vp)]
        lib.rsqc_mismatch_begin.argtypes = [vp, C.c_int32, vp, C.POINTER(C.c_char_p), C.c_uint32]
        lib.rsqc_mismatch_add.argtypes = [vp, vp, vp, vp, C.POINTER(abi.MismatchInfo)]
        lib.rsqc_mismatch_end.argtypes = [vp, C.POINTER(abi.MismatchInfo), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
        lib.rsqc_alleles_begin.argtypes = [vp, C.c_int32, C.c_uint32, vp, vp, C.c_uint32, C.c_uint32]
        lib.rsqc_alleles_add.argtypes = [vp, vp, C.POINTER(abi.AlleleInfo)]
        lib.rsqc_alleles_end.argtypes = [vp, C.POINTER(abi.AlleleInfo), C.POINTER(vp)]
        _lib = lib
    return _lib


EXPORTED_SYMBOLS = [
    "rsqc_create", "rsqc_destroy", "rsqc_set_annotation", "rsqc_set_bed", "rsqc_set_reference", "rsqc_submit", "rsqc_wait",
    "rsqc_upload", "rsqc_submit_resident", "rsqc_release", "rsqc_finalize", "rsqc_reset", "rsqc_clear_inputs", "rsqc_get_timing",
    "rsqc_reset_timing", "rsqc_device_accumulators", "rsqc_device_vectors", "rsqc_shard_summary", "rsqc_reduce_peer", "rsqc_reduce_group",
    "rsqc_group_create", "rsqc_group_reduce", "rsqc_group_info", "rsqc_group_destroy", "rsqc_refresh_results", "rsqc_finalize_device", "rsqc_host_alloc", "rsqc_host_free", "rsqc_strerror",
    "rsqc_last_error", "rsqc_counter_name", "rsqc_version", "rsqc_qname_hash", "rsqc_qname_hash2",
    "rsqc_decode_begin", "rsqc_decode_submit", "rsqc_decode_end", "rsqc_decode_begin_sam", "rsqc_decode_submit_text",
    "rsqc_sort_begin", "rsqc_sort_end", "rsqc_markdup_begin", "rsqc_markdup_end", "rsqc_markdup_verdicts", "rsqc_markdup_use_umi", "rsqc_markdup_umi_end", "rsqc_markdup_umi_edits", "rsqc_markdup_umi_group_end", "rsqc_umi_pack", "rsqc_junctions_begin", "rsqc_junctions_end",
    "rsqc_track_begin", "rsqc_track_end", "rsqc_track_rows", "rsqc_track_text",
    "rsqc_genebody_begin", "rsqc_genebody_end", "rsqc_genebody_sums",
    "rsqc_tin_begin", "rsqc_tin_end", "rsqc_tin_rows",
    "rsqc_cycles_begin", "rsqc_cycles_add", "rsqc_cycles_end",
    "rsqc_mismatch_begin", "rsqc_mismatch_add", "rsqc_mismatch_end",
    "rsqc_alleles_begin", "rsqc_alleles_add", "rsqc_alleles_end",
]


class DeviceArray:
    """A raw HIP device pointer exposed through __cuda_array_interface__ so that
    torch.as_tensor(..., device='cuda') wraps it zero-copy (used for the RCCL reduction)."""

    def __init__(self, ptr, count, typestr):
        self.__cuda_array_interface__ = {"shape": (int(count),), "typestr": typestr, "data": (int(ptr), False),
                                         "version": 2, "strides": None}


class Engine:
    def __init__(self, params: abi.Params):
        self._l = load_library()
        self._h = C.c_void_p()
        self._keep = []
        self._pinned = []
        rc = self._l.rsqc_create(C.byref(params), C.byref(self._h))
        if rc:
            raise EngineError(rc, self._l.rsqc_strerror(rc).decode())

    def _check(self, rc):
        if rc:
            raise EngineError(rc, "%s (%s)" % (self._l.rsqc_strerror(rc).decode(),
                                               self._l.rsqc_last_error(self._h).decode()))

    def last_error(self) -> str:
        """rsqc_last_error: the message of the last failure -- or the WARNING an accepted annotation left (an exon outside its gene's row)."""
        return self._l.rsqc_last_error(self._h).decode()

    def set_annotation(self, ann, owned=None):
        s = ann.to_struct()
        o = None if owned is None else np.ascontiguousarray(owned, dtype=np.uint8)
        self._keep += [ann, s, o]
        self._check(self._l.rsqc_set_annotation(self._h, C.byref(s), abi.ptr(o)))
        # RSQC_OK may come with a warning (an exon row outside the row of its gene: DESIGN.md 5): returned, kept and logged here,
        # because rsqc_last_error is overwritten by any later failure; the results carry the count (exons_outside_gene_row)
        self.annotation_warning = self.last_error() or None
        if self.annotation_warning:
            import warnings
            warnings.warn("rsqc_set_annotation: " + self.annotation_warning, RuntimeWarning, stacklevel=2)
        return self.annotation_warning

    def set_bed(self, bed):
        s = bed.to_struct()
        self._keep += [bed, s]
        self._check(self._l.rsqc_set_bed(self._h, C.byref(s)))

    def set_reference(self, ref):
        s = ref.to_struct()
        self._check(self._l.rsqc_set_reference(self._h, C.byref(s)))     # (copied: nothing of `ref` is kept)

    def submit(self, batch):
        s = batch.to_struct()
        self._keep += [batch, s]
        self._check(self._l.rsqc_submit(self._h, C.byref(s)))

    def submit_struct(self, s):
        """rsqc_submit of an already packed abi.BatchStruct (the caller keeps its arrays alive until wait())."""
        self._check(self._l.rsqc_submit(self._h, C.byref(s)))

    def pinned_copy(self, a: np.ndarray) -> np.ndarray:
        """A copy of `a` in page-locked host memory (rsqc_host_alloc); freed with the engine."""
        a = np.ascontiguousarray(a)
        nbytes = max(a.nbytes, 16)
        p = self._l.rsqc_host_alloc(nbytes)
        if not p:
            raise EngineError(abi.ERR_HIP, "rsqc_host_alloc failed")
        self._pinned.append(p)
        out = np.frombuffer((C.c_char * nbytes).from_address(p), dtype=a.dtype, count=a.size).reshape(a.shape)
        out[...] = a
        return out

    def wait(self):
        self._check(self._l.rsqc_wait(self._h))

    # ---- device-side BAM decode (rsqc_decode_*) -----------------------------------------------------------------
    def decode_begin(self, n_ref, ch_tag="ch", filter_tags=(), file_index_base=0, pipelined=False, reserve=0, ref_names=None, umi_tag=None, umi_qname=None):
        """ref_names (the SAM header's @SQ names, n_ref of them): a SAM text stream (rsqc_decode_begin_sam), fed with
        decode_submit_text (plain SAM) or decode_submit (BGZF-compressed SAM); None: a BAM stream.
        umi_tag ("RX") or umi_qname (the separator, "_"): the windows get a umi column (rsqc_decode_params.umi_source)."""
        p = abi.DecodeParams()
        if umi_tag is not None and umi_qname is not None:
            raise ValueError("one UMI source: umi_tag or umi_qname")
        if umi_tag is not None:
            if len(umi_tag) != 2:
                raise ValueError("umi_tag is two characters")
            p.umi_source = abi.UMI_SOURCE_TAG; p.umi_tag = umi_tag.encode()
        if umi_qname is not None:
            if len(umi_qname) != 1:
                raise ValueError("umi_qname is one character")
            p.umi_source = abi.UMI_SOURCE_QNAME; p.umi_sep = umi_qname.encode()
        p.pipelined = 1 if pipelined else 0
        p.reserve_inflated_bytes = reserve
        p.n_ref = n_ref
        if ch_tag and len(ch_tag) == 2:
            p.has_chimeric_tag = 1; p.chimeric_tag = ch_tag.encode()
        for k, f in enumerate(filter_tags):
            if len(f) == 2:
                p.filter_tag[k].value = f.encode()
        p.file_index_base = file_index_base
        if ref_names is not None:
            if len(ref_names) != n_ref:
                raise ValueError("ref_names must hold n_ref names")
            names = (C.c_char_p * max(1, n_ref))(*[n.encode() if isinstance(n, str) else bytes(n) for n in ref_names])
            self._check(self._l.rsqc_decode_begin_sam(self._h, C.byref(p), names))
            return
        self._check(self._l.rsqc_decode_begin(self._h, C.byref(p)))

    def decode_submit_text(self, text):
        """Plain SAM text of a stream begun with ref_names (any cut: a line may straddle calls).  Returns (records, [RefID of
        every run of records]) as decode_submit."""
        buf = np.frombuffer(bytes(text), np.uint8) if not isinstance(text, np.ndarray) else text
        self._keep_decode = buf
        w = abi.DecodeWindow()
        self._check(self._l.rsqc_decode_submit_text(self._h, buf.ctypes.data if buf.size else None, buf.size, C.byref(w)))
        self._last_window = w
        runs = list(np.ctypeslib.as_array(C.cast(w.run_tid, C.POINTER(C.c_int32)), (w.n_runs,))) if w.n_runs else []
        return int(w.n_records), [int(t) for t in runs]

    def decode_submit(self, compressed, blocks, skip=0, limit=0):
        """compressed: bytes-like or (address, nbytes); blocks: numpy array of abi BGZF block records (or (address, n)).
        Returns (records, [RefID of every run of records])."""
        if isinstance(compressed, tuple):
            caddr, cbytes = compressed
        else:
            buf = np.frombuffer(compressed, np.uint8)
            self._keep_decode = buf
            caddr, cbytes = buf.ctypes.data, buf.size
        if isinstance(blocks, tuple):
            baddr, nb = blocks
        else:
            blocks = np.ascontiguousarray(blocks)
            baddr, nb = blocks.ctypes.data, len(blocks)
        w = abi.DecodeWindow()
        self._check(self._l.rsqc_decode_submit(self._h, caddr, cbytes, baddr, nb, skip, limit, C.byref(w)))
        self._last_window = w
        runs = list(np.ctypeslib.as_array(C.cast(w.run_tid, C.POINTER(C.c_int32)), (w.n_runs,))) if w.n_runs else []
        return int(w.n_records), [int(t) for t in runs]

    def decode_end(self):
        """(records, unsorted, number of records with an unrecognised RefID, first names of those); .decode_last = (records,
        runs) of the call that rsqc_decode_end completed (pipelined streams)"""
        info = abi.DecodeInfo()
        rc = self._l.rsqc_decode_end(self._h, C.byref(info))
        lw = info.last
        self.decode_last = (int(lw.n_records), [int(t) for t in np.ctypeslib.as_array(C.cast(lw.run_tid, C.POINTER(C.c_int32)), (lw.n_runs,))] if lw.n_runs else [])
        names = []
        if info.n_bad_refid and info.bad_refid:
            arr = C.cast(info.bad_refid, C.POINTER(C.c_char_p))
            names = [arr[k].decode() for k in range(min(info.n_bad_refid, 64))]
        self._check(rc)
        return int(info.records), bool(info.unsorted), int(info.n_bad_refid), names

    # ---- input in any order (rsqc_sort_*) ------------------------------------------------------------------------
    def sort_begin(self):
        """Collecting mode: every submit / decode_submit from here on appends to a device-resident collection."""
        self._check(self._l.rsqc_sort_begin(self._h))

    def sort_end(self) -> dict:
        """Orders the collection on the device and runs it as ordinary batches; the fields of rsqc_sort_info."""
        info = abi.SortInfo()
        self._check(self._l.rsqc_sort_end(self._h, C.byref(info)))
        return {f: getattr(info, f) for f, _ in abi.SortInfo._fields_}

    # ---- duplicate fragments flagged on the collection (rsqc_markdup_*) ------------------------------------------
    def markdup_begin(self):
        """Behind sort_begin(), before the first submit: sort_end() first rewrites flag 0x400 of every collected record."""
        self._check(self._l.rsqc_markdup_begin(self._h))

    def markdup_end(self) -> dict:
        """Behind sort_end(): the fields of rsqc_markdup_info."""
        info = abi.MarkdupInfo()
        self._check(self._l.rsqc_markdup_end(self._h, C.byref(info)))
        return {f: getattr(info, f) for f, _ in abi.MarkdupInfo._fields_}

    def markdup_verdicts(self, first, n) -> np.ndarray:
        """One byte (0 or 1) per record of the collection in arrival order, rows [first, first + n) (a copy)."""
        p = C.c_void_p()
        self._check(self._l.rsqc_markdup_verdicts(self._h, int(first), int(n), C.byref(p)))
        return abi._view(p.value, int(n), np.uint8)

    def markdup_use_umi(self):
        """Behind markdup_begin(), before the first submit: the UMI key (Batch.umi / the decode stream's umi column) joins the signature."""
        self._check(self._l.rsqc_markdup_use_umi(self._h))

    def markdup_umi_end(self) -> dict:
        """Behind sort_end() of a pass with markdup_use_umi(): the fields of rsqc_markdup_umi_info."""
        info = abi.MarkdupUmiInfo()
        self._check(self._l.rsqc_markdup_umi_end(self._h, C.byref(info)))
        return {f: int(getattr(info, f)) for f, _ in abi.MarkdupUmiInfo._fields_}

    def markdup_umi_edits(self, max_edits: int):
        """Behind markdup_use_umi(), before the first submit: 1 groups UMIs of one position set that are one substitution apart
        (rsqc_markdup_umi_edits); 0 is exact matching."""
        self._check(self._l.rsqc_markdup_umi_edits(self._h, int(max_edits)))

    def markdup_umi_group_end(self) -> dict:
        """Behind sort_end() of a pass with markdup_umi_edits(1): the fields of rsqc_markdup_umi_group_info (group_ms a float)."""
        info = abi.MarkdupUmiGroupInfo()
        self._check(self._l.rsqc_markdup_umi_group_end(self._h, C.byref(info)))
        return {f: (float if f == "group_ms" else int)(getattr(info, f)) for f, _ in abi.MarkdupUmiGroupInfo._fields_}

    def last_window_umi(self) -> np.ndarray:
        """The umi column of the window the last decode_submit / decode_submit_text decoded (a non-pipelined stream with a UMI
        source), copied from the device through rsqc_decode_window.device_batch.umi."""
        w = self._last_window
        n = int(w.n_records)
        if n and not w.device_batch.umi:
            raise EngineError(abi.ERR_ARG, "the window has no umi column")
        return self.read_device(w.device_batch.umi, n, np.uint64)

    # ---- reads per splice junction (rsqc_junctions_*) -------------------------------------------------------------
    def junctions_begin(self):
        """From here to the end of the pass every batch that is run also leaves its splice-junction instances on the device."""
        self._check(self._l.rsqc_junctions_begin(self._h))

    def junctions_end(self) -> dict:
        """After finalize() / finalize_device(): the junction table as numpy arrays (copies) -- tid, start, end (int32), reads,
        hq_reads, max_overhang (uint32), one entry per row in (tid, start, end) order -- and the scalars of rsqc_junction_table."""
        t = abi.JunctionTable()
        self._check(self._l.rsqc_junctions_end(self._h, C.byref(t)))
        n = int(t.n)
        out = {f: abi._view(getattr(t, f), n, np.int32) for f in ("tid", "start", "end")}
        out.update({f: abi._view(getattr(t, f), n, np.uint32) for f in ("reads", "hq_reads", "max_overhang")})
        out.update(n=n, instances=int(t.instances), population=int(t.population), extract_ms=t.extract_ms, sort_ms=t.sort_ms, reduce_ms=t.reduce_ms)
        return out

    # ---- per-base coverage track (rsqc_track_*) ---------------------------------------------------------------------
    def track_begin(self, lengths, names=None):
        """From here to the end of the pass every batch that is run also adds its coverage events to a difference array over the
        contigs of `lengths`; `names` (needed for track_text only) are the contigs' names."""
        lens = np.ascontiguousarray([int(x) for x in lengths], dtype=np.uint64)
        arr = None
        if names is not None:
            assert len(names) == len(lens)
            arr = (C.c_char_p * max(len(lens), 1))(*[n.encode() if isinstance(n, str) else n for n in names])
        self._check(self._l.rsqc_track_begin(self._h, len(lens), abi.ptr(lens), arr))

    def track_end(self) -> dict:
        """After finalize() / finalize_device(): the rows are built on the device; the fields of rsqc_track_info."""
        info = abi.TrackInfo()
        self._check(self._l.rsqc_track_end(self._h, C.byref(info)))
        return {f: getattr(info, f) for f, _ in abi.TrackInfo._fields_}

    def track_rows(self, first, n) -> dict:
        """Rows [first, first + n) as numpy arrays (copies): tid (int32), start, end, depth (uint32)."""
        p = [C.c_void_p() for _ in range(4)]
        self._check(self._l.rsqc_track_rows(self._h, int(first), int(n), *[C.byref(x) for x in p]))
        return {f: abi._view(x.value, int(n), dt).copy() for f, x, dt in zip(("tid", "start", "end", "depth"), p, (np.int32, np.uint32, np.uint32, np.uint32))}

    def track_text(self, first, n) -> bytes:
        """Rows [first, first + n) as bedGraph text, formatted on the device."""
        p, nbytes = C.c_void_p(), C.c_uint64()
        self._check(self._l.rsqc_track_text(self._h, int(first), int(n), C.byref(p), C.byref(nbytes)))
        return C.string_at(p.value, nbytes.value) if nbytes.value else b""

    # ---- coverage along the gene body (rsqc_genebody_*) ---------------------------------------------------------------
    def genebody_begin(self, seg_off, seg_tid, seg_start, seg_end, reverse):
        """Behind track_begin and before the first submit: the model of the pass -- gene g's segments are rows [seg_off[g],
        seg_off[g + 1]) of (seg_tid, seg_start, seg_end), 0-based with the end exclusive; `reverse` has one byte per gene."""
        off = np.ascontiguousarray(seg_off, dtype=np.uint32)
        tid = np.ascontiguousarray(seg_tid, dtype=np.int32)
        start, end = np.ascontiguousarray(seg_start, dtype=np.uint32), np.ascontiguousarray(seg_end, dtype=np.uint32)
        rev = np.ascontiguousarray(reverse, dtype=np.uint8)
        assert len(off) == len(rev) + 1 and len(tid) == len(start) == len(end)
        self._check(self._l.rsqc_genebody_begin(self._h, len(rev), abi.ptr(off), abi.ptr(tid), abi.ptr(start), abi.ptr(end), abi.ptr(rev)))

    def genebody_end(self) -> dict:
        """After track_end(): the sums are built on the device; the fields of rsqc_genebody_info."""
        info = abi.GenebodyInfo()
        self._check(self._l.rsqc_genebody_end(self._h, C.byref(info)))
        return {f: getattr(info, f) for f, _ in abi.GenebodyInfo._fields_}

    def genebody_sums(self, first_gene, n) -> np.ndarray:
        """The sums of genes [first_gene, first_gene + n) as a (n, 100) uint64 array (a copy)."""
        p = C.c_void_p()
        self._check(self._l.rsqc_genebody_sums(self._h, int(first_gene), int(n), C.byref(p)))
        return abi._view(p.value, int(n) * abi.GENEBODY_BINS, np.uint64).copy().reshape(int(n), abi.GENEBODY_BINS)

    # ---- per-gene transcript integrity (rsqc_tin_*) -------------------------------------------------------------------
    def tin_begin(self, seg_off, seg_tid, seg_start, seg_end):
        """Behind track_begin and before the first submit: the model of the pass, as for genebody_begin without `reverse` (the
        figures are symmetric in the strand)."""
        off = np.ascontiguousarray(seg_off, dtype=np.uint32)
        tid = np.ascontiguousarray(seg_tid, dtype=np.int32)
        start, end = np.ascontiguousarray(seg_start, dtype=np.uint32), np.ascontiguousarray(seg_end, dtype=np.uint32)
        assert len(off) >= 1 and len(tid) == len(start) == len(end)
        self._check(self._l.rsqc_tin_begin(self._h, len(off) - 1, abi.ptr(off), abi.ptr(tid), abi.ptr(start), abi.ptr(end)))

    def tin_end(self) -> dict:
        """After track_end(): the rows are built on the device and copied to the host; the fields of rsqc_tin_info."""
        info = abi.TinInfo()
        self._check(self._l.rsqc_tin_end(self._h, C.byref(info)))
        return {f: getattr(info, f) for f, _ in abi.TinInfo._fields_}

    def tin_rows(self, first_gene, n) -> np.ndarray:
        """The rows of genes [first_gene, first_gene + n) as a structured array of abi.TIN_ROW (a copy)."""
        p = C.c_void_p()
        self._check(self._l.rsqc_tin_rows(self._h, int(first_gene), int(n), C.byref(p)))
        if not int(n):
            return np.zeros(0, abi.TIN_ROW)
        return abi._view(p.value, int(n) * abi.TIN_ROW.itemsize, np.uint8).copy().view(abi.TIN_ROW)

    # ---- base quality and composition by read cycle (rsqc_cycles_*) -------------------------------------------------------
    def cycles_begin(self):
        """Before the pass's first submit or decode_begin: every decode window from here on is counted by read cycle."""
        self._check(self._l.rsqc_cycles_begin(self._h))

    def cycles_add(self, base, qual, info: dict):
        """Host-computed counts: base [2][512][5] and qual [2][512][64] (uint64, either may be None) and the fields of rsqc_cycle_info."""
        b = None if base is None else np.ascontiguousarray(base, dtype=np.uint64).reshape(-1)
        q = None if qual is None else np.ascontiguousarray(qual, dtype=np.uint64).reshape(-1)
        assert b is None or b.size == abi.CYCLE_ENDS * abi.CYCLE_MAX * abi.CYCLE_BASES
        assert q is None or q.size == abi.CYCLE_ENDS * abi.CYCLE_MAX * abi.CYCLE_QBINS
        part = abi.CycleInfo()
        for f, _ in abi.CycleInfo._fields_:
            setattr(part, f, info.get(f, 0))
        self._check(self._l.rsqc_cycles_add(self._h, abi.ptr(b), abi.ptr(q), C.byref(part)))

    def cycles_end(self):
        """Behind decode_end(): (the fields of rsqc_cycle_info, base [2, 512, 5], qual [2, 512, 64]); the tables are copies."""
        info = abi.CycleInfo()
        pb, pq = C.c_void_p(), C.c_void_p()
        self._check(self._l.rsqc_cycles_end(self._h, C.byref(info), C.byref(pb), C.byref(pq)))
        base = abi._view(pb.value, abi.CYCLE_ENDS * abi.CYCLE_MAX * abi.CYCLE_BASES, np.uint64).copy().reshape(abi.CYCLE_ENDS, abi.CYCLE_MAX, abi.CYCLE_BASES)
        qual = abi._view(pq.value, abi.CYCLE_ENDS * abi.CYCLE_MAX * abi.CYCLE_QBINS, np.uint64).copy().reshape(abi.CYCLE_ENDS, abi.CYCLE_MAX, abi.CYCLE_QBINS)
        return {f: getattr(info, f) for f, _ in abi.CycleInfo._fields_}, base, qual

    # ---- errors by read cycle against the reference (rsqc_mismatch_*) -----------------------------------------------------
    _MM_SHAPES = ((abi.CYCLE_ENDS, abi.CYCLE_MAX, abi.MISMATCH_COLS), (abi.CYCLE_ENDS, 4, 4), (abi.CYCLE_QBINS, 2))

    def mismatch_begin(self, lengths, sequences, min_mapq=0):
        """Before the pass's first submit or decode_begin.  lengths: one per @SQ contig; sequences: per contig bytes or None (the FASTA
        lacks it), or None altogether: the packed reference of an earlier pass of this context is used again."""
        ln = np.ascontiguousarray(lengths, dtype=np.uint64)
        seqs = None
        if sequences is not None:
            assert len(sequences) == ln.size
            seqs = (C.c_char_p * max(ln.size, 1))(*[None if s is None else bytes(s) for s in sequences])
        self._check(self._l.rsqc_mismatch_begin(self._h, int(ln.size), abi.ptr(ln), seqs, int(min_mapq)))

    def mismatch_add(self, cyc, subst, byq, info: dict):
        """Host-computed counts: cyc [2][512][6], subst [2][4][4], byq [64][2] (uint64, any may be None) and the fields of rsqc_mismatch_info."""
        t = [None if a is None else np.ascontiguousarray(a, dtype=np.uint64).reshape(-1) for a in (cyc, subst, byq)]
        for a, shape in zip(t, self._MM_SHAPES):
            assert a is None or a.size == int(np.prod(shape))
        part = abi.MismatchInfo()
        for f, _ in abi.MismatchInfo._fields_:
            setattr(part, f, info.get(f, 0))
        self._check(self._l.rsqc_mismatch_add(self._h, abi.ptr(t[0]), abi.ptr(t[1]), abi.ptr(t[2]), C.byref(part)))

    def mismatch_end(self):
        """Behind decode_end(): (the fields of rsqc_mismatch_info, cyc [2, 512, 6], subst [2, 4, 4], byq [64, 2]); the tables are copies."""
        info = abi.MismatchInfo()
        p = [C.c_void_p(), C.c_void_p(), C.c_void_p()]
        self._check(self._l.rsqc_mismatch_end(self._h, C.byref(info), C.byref(p[0]), C.byref(p[1]), C.byref(p[2])))
        tabs = [abi._view(q.value, int(np.prod(shape)), np.uint64).copy().reshape(shape) for q, shape in zip(p, self._MM_SHAPES)]
        return ({f: getattr(info, f) for f, _ in abi.MismatchInfo._fields_}, *tabs)

    # ---- base counts at known variant sites (rsqc_alleles_*) ---------------------------------------------------------------
    def alleles_begin(self, n_contigs, tid, pos, min_mapq=0, min_baseq=0):
        """Before the pass's first submit or decode_begin.  tid, pos: the sites, 0-based, strictly ascending by (tid, pos)."""
        t, p = np.ascontiguousarray(tid, dtype=np.int32), np.ascontiguousarray(pos, dtype=np.int32)
        assert t.ndim == 1 and t.shape == p.shape
        self._check(self._l.rsqc_alleles_begin(self._h, int(n_contigs), int(t.size), abi.ptr(t), abi.ptr(p), int(min_mapq), int(min_baseq)))
        self._allele_sites = int(t.size)

    def alleles_add(self, counts, info: dict):
        """Host-computed counts: counts [n_sites][7] (uint64, or None) and the fields of rsqc_allele_info."""
        a = None if counts is None else np.ascontiguousarray(counts, dtype=np.uint64).reshape(-1)
        assert a is None or a.size == getattr(self, "_allele_sites", 0) * abi.ALLELE_COLS
        part = abi.AlleleInfo()
        for f, _ in abi.AlleleInfo._fields_:
            setattr(part, f, info.get(f, 0))
        self._check(self._l.rsqc_alleles_add(self._h, abi.ptr(a), C.byref(part)))

    def alleles_end(self):
        """Behind decode_end(): (the fields of rsqc_allele_info, counts [n_sites, 7]); the table is a copy."""
        info = abi.AlleleInfo()
        p = C.c_void_p()
        self._check(self._l.rsqc_alleles_end(self._h, C.byref(info), C.byref(p)))
        n = int(info.n_sites)
        counts = abi._view(p.value, n * abi.ALLELE_COLS, np.uint64).copy().reshape(n, abi.ALLELE_COLS) if n else np.zeros((0, abi.ALLELE_COLS), np.uint64)
        return {f: getattr(info, f) for f, _ in abi.AlleleInfo._fields_}, counts

    def read_device(self, ptr, count, dtype):
        """count items of dtype from a device pointer of this context (tests): hipMemcpy of the HIP runtime the library itself is
        linked against, after rsqc_wait."""
        out = np.zeros(count, dtype)
        if count:
            global _hip
            if _hip is None:
                # the very copy of the HIP runtime the product library is running on (a process may hold a second one, e.g.
                # PyTorch's bundled runtime, which knows nothing of this context's allocations)
                path = "libamdhip64.so"
                for line in open("/proc/self/maps"):
                    if "libamdhip64" in line and "/torch/" not in line:
                        path = line.split()[-1]; break
                _hip = C.CDLL(path)
                _hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
            self.wait()
            rc = _hip.hipMemcpy(out.ctypes.data, ptr, out.nbytes, 2)     # hipMemcpyDeviceToHost
            if rc:
                raise EngineError(abi.ERR_HIP if hasattr(abi, "ERR_HIP") else -1, "hipMemcpy(device -> host) failed: %d" % rc)
        return out

    def last_decoded(self):
        """abi.BatchStruct of DEVICE pointers: rsqc_decode_window.device_batch of the last decode_submit."""
        return self._last_window.device_batch

    def upload(self, batch) -> int:
        s = batch.to_struct()
        h = C.c_int()
        self._check(self._l.rsqc_upload(self._h, C.byref(s), C.byref(h)))
        return h.value

    def upload_struct(self, s) -> int:
        """rsqc_upload of an already packed abi.BatchStruct."""
        h = C.c_int()
        self._check(self._l.rsqc_upload(self._h, C.byref(s), C.byref(h)))
        return h.value

    def submit_resident(self, handle: int):
        self._check(self._l.rsqc_submit_resident(self._h, handle))

    def release(self, handle: int):
        self._check(self._l.rsqc_release(self._h, handle))

    def finalize(self, lazy: bool = False) -> abi.Results:
        """Runs the end-of-file stage and reads every result vector back to the host (inside the library).
        lazy=True returns views that are copied out of the library's host buffers on first access and are only
        valid until the next finalize/reset of this engine."""
        rs = abi.ResultsStruct()
        self._check(self._l.rsqc_finalize(self._h, C.byref(rs)))
        r = abi.Results(rs)
        return r if lazy else r.materialise()

    def finalize_device(self):
        """End-of-file stage without the read-back (the distributed path reduces first, then refresh_results())."""
        self._check(self._l.rsqc_finalize_device(self._h))

    @staticmethod
    def reduce_group(engines) -> bool:
        """rsqc_reduce_group over the contexts of `engines` (all past finalize_device): results summed onto engines[0].
        Returns True when the RCCL path was taken (False: peer copies)."""
        arr = (C.c_void_p * len(engines))(*[e._h for e in engines])
        used = C.c_int(0)
        engines[0]._check(engines[0]._l.rsqc_reduce_group(arr, len(engines), C.byref(used)))
        return bool(used.value)

    class Group:
        """rsqc_group_*: the exchange group of a sharded run, its RCCL communicators made once (any time after the contexts
        exist) and reused by every reduce()."""

        def __init__(self, engines):
            self._engines = list(engines)
            self._l = engines[0]._l
            arr = (C.c_void_p * len(engines))(*[e._h for e in engines])
            h = C.c_void_p()
            engines[0]._check(self._l.rsqc_group_create(arr, len(engines), C.byref(h)))
            self._g = h

        def info(self):
            uses, init_ms, red_ms, note = C.c_int(), C.c_double(), C.c_double(), C.c_char_p()
            self._l.rsqc_group_info(self._g, C.byref(uses), C.byref(init_ms), C.byref(red_ms), C.byref(note))
            return dict(uses_rccl=bool(uses.value), init_ms=init_ms.value, last_reduce_ms=red_ms.value, note=(note.value or b"").decode())

        def reduce(self) -> bool:
            used = C.c_int(0)
            self._engines[0]._check(self._l.rsqc_group_reduce(self._g, C.byref(used)))
            return bool(used.value)

        def close(self):
            if self._g:
                self._l.rsqc_group_destroy(self._g); self._g = None

    def refresh_results(self, lazy: bool = False) -> abi.Results:
        rs = abi.ResultsStruct()
        self._check(self._l.rsqc_refresh_results(self._h, C.byref(rs)))
        r = abi.Results(rs)
        return r if lazy else r.materialise()

    def reset(self):
        self._check(self._l.rsqc_reset(self._h))

    def clear_inputs(self):
        """rsqc_clear_inputs: waits for what is in flight, then drops annotation, BED and reference (and the open pass): the
        engine is as after its creation, set_annotation / set_bed / set_reference may be called again."""
        self._check(self._l.rsqc_clear_inputs(self._h))
        self._keep = []

    def timing(self) -> dict:
        t = abi.TimingStruct()
        self._check(self._l.rsqc_get_timing(self._h, C.byref(t)))
        return {f: getattr(t, f) for f, _ in abi.TimingStruct._fields_}

    def reset_timing(self):
        self._check(self._l.rsqc_reset_timing(self._h))

    def device_accumulators(self):
        u, f = C.c_void_p(), C.c_void_p()
        nu, nf = C.c_uint64(), C.c_uint64()
        self._check(self._l.rsqc_device_accumulators(self._h, C.byref(u), C.byref(nu), C.byref(f), C.byref(nf)))
        # int64 view: torch has no uint64 arithmetic; counts are far below 2^63
        return DeviceArray(u.value, nu.value, "<i8"), DeviceArray(f.value, nf.value, "<f8")

    def device_vectors(self):
        """The three device ranges a sharded run sum-reduces (rsqc_device_vectors): int64 counts, f64 sums and
        owner-only statistics, u8 validity flags."""
        r = (abi.DeviceRange * 3)()
        self._check(self._l.rsqc_device_vectors(self._h, C.byref(r)))
        return (DeviceArray(r[0].base, r[0].count, "<i8"), DeviceArray(r[1].base, r[1].count, "<f8"),
                DeviceArray(r[2].base, r[2].count, "|u1"))

    def shard_summary(self):
        """The order-dependent outputs of this shard (rsqc_shard_summary) as a distributed.ShardInfo (copies)."""
        from .distributed import ShardInfo
        si = abi.ShardInfoStruct()
        self._check(self._l.rsqc_shard_summary(self._h, C.byref(si)))
        nb, ns = si.n_batches, si.n_samples
        off = abi._view(si.rl_offset, nb + 1, np.uint32).copy() if nb else np.zeros(1, np.uint32)
        ne = int(off[-1])
        return ShardInfo(batch_file_index=abi._view(si.batch_file_index, nb, np.uint64).copy(),
                         batch_records=abi._view(si.batch_records, nb, np.uint64).copy(), rl_offset=off,
                         rl_span=abi._view(si.rl_span, ne, np.uint32).copy(), rl_state=abi._view(si.rl_state, ne, np.int32).copy(),
                         sample_file_index=abi._view(si.sample_file_index, ns, np.uint64).copy(),
                         sample_size=abi._view(si.sample_size, ns, np.uint32).copy())

    def close(self):
        if self._h:
            self._l.rsqc_destroy(self._h)
            self._h = C.c_void_p()
            for p in self._pinned:
                self._l.rsqc_host_free(p)
            self._pinned = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def run_engine(params, ann, batches, bed=None, owned=None, reference=None) -> abi.Results:
    e = Engine(params)
    try:
        e.set_annotation(ann, owned)
        if bed is not None:
            e.set_bed(bed)
        if reference is not None:
            e.set_reference(reference)
        for b in batches:
            e.submit(b)
        return e.finalize()
    finally:
        e.close()


def umi_pack(umi) -> int:
    """The product's own rsqc_umi_pack (abi.umi_pack is the same definition in Python)."""
    b = umi.encode() if isinstance(umi, str) else bytes(umi)
    return int(load_library().rsqc_umi_pack(b, len(b)))
