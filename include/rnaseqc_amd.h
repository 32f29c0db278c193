/*
 * rnaseqc_amd.h -- C ABI of the MI355X-native RNA-SeQC per-read hot path.
 *
 * The reference (getzlab/rnaseqc 2.4.3) has no plugin / FFI interface: its hot
 * path is five C++ free functions called from the BAM loop of main()
 * (src/RNASeQC.cpp:242-382, signatures in src/Expression.h:19-37) that mutate
 * namespace-scope globals (src/Metrics.cpp:20-22, src/GTF.cpp:22-27).  This
 * header is the batch-oriented C boundary that replaces that seam:
 *
 *   reference call site / state                         replaced by
 *   --------------------------------------------------  -------------------------
 *   GTF load into features/geneList/exonList/           rsqc_set_annotation()
 *     exonsForGene/exonLengths  (src/RNASeQC.cpp:108-156,
 *     src/GTF.cpp:30-131)
 *   BED load (src/RNASeQC.cpp:172-187, src/BED.cpp:18)  rsqc_set_bed()
 *   Fasta::open / getSeq (src/Fasta.cpp:77-140,          rsqc_set_reference()
 *     src/RNASeQC.cpp:118-121)
 *   while (bam.next(alignment)) { gate cascade;         rsqc_submit() /
 *     extractBlocks; trimFeatures;                      rsqc_submit_resident()
 *     exonAlignmentMetrics; fragmentSizeMetrics }       (one call per SoA batch
 *     (src/RNASeQC.cpp:242-382)                          of records, file order)
 *   dropFeatures at EOF -> BaseCoverage::compute ->     rsqc_finalize()
 *     computeCoverage/computeBias
 *     (src/RNASeQC.cpp:385-388, src/Metrics.cpp:132-337)
 *   geneCounts/uniqueGeneCounts/geneFragmentCounts/     rsqc_results
 *     exonCounts/Metrics/BiasCounter/BaseCoverage
 *     lists/fragmentSizes/readLength read by the
 *     report writer (src/RNASeQC.cpp:397-676)
 *
 * Conventions: plain C, caller-owned inputs, library-owned outputs (valid
 * until the next rsqc_finalize()/rsqc_destroy()), 0 = success, negative =
 * error (no exceptions cross the boundary).  One context drives one GPU (one
 * shard of contigs); contexts are independent, so a node runs one per GPU.
 * All coordinates are as in the reference: features 1-based closed
 * (src/GTF.h:29-37), record pos/mpos 0-based as in BAM (htslib core.pos).
 */
#ifndef RNASEQC_AMD_H
#define RNASEQC_AMD_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RSQC_ABI_VERSION 7

#if defined(__GNUC__)
#define RSQC_API __attribute__((visibility("default")))
#else
#define RSQC_API
#endif

/* ---- error codes ------------------------------------------------------- */
#define RSQC_OK              0
#define RSQC_ERR_ARG        -1   /* bad argument / call order                           */
#define RSQC_ERR_HIP        -2   /* HIP runtime failure (maps to exit code 10)          */
#define RSQC_ERR_BAD_CIGAR  -3   /* CIGAR op outside MIDNSHP=X: the reference throws
                                    std::invalid_argument (src/Expression.cpp:61-63),
                                    exit code 7                                         */
#define RSQC_ERR_CAPACITY   -4   /* a fixed device-side capacity was exceeded            */
#define RSQC_ERR_NO_DEVICE  -5   /* no HIP device: there is NO CPU fallback              */
#define RSQC_ERR_EMPTY_MEDIAN -6 /* std::range_error of computeMedian (src/Metrics.h:149) */
#define RSQC_ERR_INPUT      -7   /* rsqc_decode_*: corrupt BGZF block / malformed or truncated BAM record (the reference
                                    ends with htslib's read error)                       */

/* ---- BAM flag bits (SAM spec; accessors used at src/RNASeQC.cpp:254-330) */
#define RSQC_FPAIRED   0x1
#define RSQC_FPROPER   0x2
#define RSQC_FUNMAP    0x4
#define RSQC_FMUNMAP   0x8
#define RSQC_FREVERSE  0x10
#define RSQC_FMREVERSE 0x20
#define RSQC_FREAD1    0x40
#define RSQC_FREAD2    0x80
#define RSQC_FSECONDARY 0x100
#define RSQC_FQCFAIL   0x200
#define RSQC_FDUP      0x400
#define RSQC_FSUPP     0x800

/* ---- tagbits byte of a record ------------------------------------------ */
#define RSQC_TB_HAS_NM     0x01  /* GetIntTag("NM") succeeded (src/RNASeQC.cpp:295)      */
#define RSQC_TB_HAS_CH     0x02  /* readStringTag(chimeric_tag): Z tag, or A tag with a
                                    non-NUL char (src/RNASeQC.cpp:780-800)              */
#define RSQC_TB_MTID_SAME  0x04  /* ChrID() == MateChrID() (src/RNASeQC.cpp:287)         */
#define RSQC_TB_FILTER0    0x08  /* --tag k present (GetTag: Z, int or float type,
                                    src/RNASeQC.cpp:320-327); k = 0..4 -> bits 3..7     */
#define RSQC_MAX_FILTER_TAGS 5

/* saturating narrow fields: a record whose nm/l_qseq/n_cigar does not fit is
 * stored with the escape value and listed (index-sorted) in the wide table   */
#define RSQC_NM_ESCAPE     0xFF
#define RSQC_LQSEQ_ESCAPE  0xFFFF
#define RSQC_NCIGAR_ESCAPE 0xFF

/* ---- strandedness (reference enum Strand {Forward, Reverse, Unknown},
 *      src/Fasta.h:41; --stranded FR -> Forward, RF -> Reverse,
 *      src/RNASeQC.cpp:78-85) ------------------------------------------------ */
#define RSQC_STRAND_FORWARD 0
#define RSQC_STRAND_REVERSE 1
#define RSQC_STRAND_UNKNOWN 2

/* ---- feature flag byte --------------------------------------------------- */
#define RSQC_FF_STRAND_MASK 0x03 /* RSQC_STRAND_*                                        */
#define RSQC_FF_RIBOSOMAL   0x04 /* transcript_type contains "rRNA" (src/GTF.cpp:113)    */

/* ---- scalar counters (Metrics keys, src/Metrics.cpp:344-384 and
 *      src/RNASeQC.cpp:254-360, src/Expression.cpp:402-455) ------------------ */
enum rsqc_counter {
    RSQC_C_ALTERNATIVE_ALIGNMENTS = 0,
    RSQC_C_SUPPLEMENTARY_ALIGNMENTS,
    RSQC_C_FAILED_VENDOR_QC,
    RSQC_C_LOW_MAPPING_QUALITY,
    RSQC_C_CHIMERIC_AUTO,
    RSQC_C_CHIMERIC_TAG,
    RSQC_C_UNIQUE_VENDOR_PASSED,
    RSQC_C_UNPAIRED_READS,
    RSQC_C_MAPPED_READS,
    RSQC_C_MAPPED_DUPLICATE_READS,
    RSQC_C_MAPPED_UNIQUE_READS,
    RSQC_C_TOTAL_MAPPED_PAIRS,
    RSQC_C_END1_MAPPED_READS,
    RSQC_C_END1_MISMATCHES,
    RSQC_C_END1_BASES,
    RSQC_C_DUPLICATE_PAIRS,
    RSQC_C_UNIQUE_FRAGMENTS,
    RSQC_C_END2_MAPPED_READS,
    RSQC_C_END2_MISMATCHES,
    RSQC_C_END2_BASES,
    RSQC_C_MISMATCHED_BASES,
    RSQC_C_TOTAL_BASES,
    RSQC_C_HIGH_QUALITY_READS,
    RSQC_C_LOW_QUALITY_READS,
    RSQC_C_READS_USED,
    RSQC_C_ALIGNMENT_BLOCKS,
    RSQC_C_NON_GLOBIN_READS,
    RSQC_C_NON_GLOBIN_DUPLICATE_READS,
    RSQC_C_INTRONIC_READS,
    RSQC_C_INTRAGENIC_READS,
    RSQC_C_HQ_INTRONIC_READS,
    RSQC_C_HQ_INTRAGENIC_READS,
    RSQC_C_INTERGENIC_READS,
    RSQC_C_HQ_INTERGENIC_READS,
    RSQC_C_EXONIC_READS,
    RSQC_C_HQ_EXONIC_READS,
    RSQC_C_AMBIGUOUS_READS,
    RSQC_C_HQ_AMBIGUOUS_READS,
    RSQC_C_RRNA_READS,
    RSQC_C_END1_SENSE,
    RSQC_C_END1_ANTISENSE,
    RSQC_C_END2_SENSE,
    RSQC_C_END2_ANTISENSE,
    RSQC_C_TOTAL_ALIGNMENTS,
    RSQC_C_FILTERED_TAG0,          /* "Filtered by tag: X", one per --tag        */
    RSQC_C_FILTERED_TAG1,
    RSQC_C_FILTERED_TAG2,
    RSQC_C_FILTERED_TAG3,
    RSQC_C_FILTERED_TAG4,
    RSQC_C_SPLIT_READS,            /* --legacy only (src/Expression.cpp:274); printed when non-zero
                                      (src/Metrics.cpp:398)                                          */
    RSQC_N_COUNTERS
};

/* ---- run parameters (flag table src/RNASeQC.cpp:39-65, defaults :87-100) - */
typedef struct rsqc_params {
    uint32_t abi_version;          /* RSQC_ABI_VERSION                                   */
    int32_t  device;               /* HIP device ordinal                                 */
    uint32_t mapq_threshold;       /* -q, 255                                            */
    uint32_t base_mismatch;        /* --base-mismatch, 6                                 */
    int32_t  chimeric_distance;    /* --chimeric-distance, 2000000                       */
    uint32_t fragment_samples;     /* --fragment-samples, 1000000 (used iff BED is set)  */
    int32_t  bias_offset;          /* --offset, 0                                        */
    int32_t  bias_window;          /* --window-size, 100                                 */
    uint64_t bias_gene_length;     /* --gene-length, 200                                 */
    uint32_t coverage_mask;        /* --coverage-mask, 500                               */
    int32_t  stranded;             /* RSQC_STRAND_*; UNKNOWN = unstranded                */
    int32_t  unpaired;             /* -u                                                 */
    int32_t  exclude_chimeric;     /* --exclude-chimeric                                 */
    int32_t  n_filter_tags;        /* number of --tag filters carried in tagbits (<=5)   */
    int32_t  legacy;               /* --legacy: RNA-SeQC 1.1.9 counting rules
                                      (legacyExonAlignmentMetrics, src/Expression.cpp:129-304, and the
                                      LegacyMode tests of src/RNASeQC.cpp:258-287).  The caller applies
                                      the two host-side parts: -q defaults to 4 (src/RNASeQC.cpp:90) and
                                      1-base features are left out of the annotation (:129-135)        */
    int32_t  reserved[6];
} rsqc_params;

/* ---- annotation: the flattened form of the reference's GTF state ----------
 * Contig ids: [0, n_ref) are the BAM @SQ entries in header order (a record's
 * tid); [n_ref, n_contigs) are contigs that only the GTF names (their genes
 * still produce coverage rows at EOF, src/RNASeQC.cpp:385-386).
 * Gene ids: [0, n_genes_listed) = geneList order (GTF order of `gene` rows,
 * src/GTF.cpp:87); [n_genes_listed, n_genes) = gene_ids that only exon rows
 * name (they are counted but never reported).  Exon ids = exonList order.
 * Interval rows are sorted by (contig, start), ties in GTF order -- the
 * reference's per-contig std::list::sort(compIntervalStart), stable
 * (src/RNASeQC.cpp:150-152).  start <= end is required.                      */
typedef struct rsqc_annotation {
    int32_t n_ref, n_contigs;
    int32_t n_genes, n_genes_listed, n_exons;

    /* `gene` rows, sorted; n_gene_rows == n_genes_listed                      */
    const int32_t  *gene_row_contig;   /* [n_genes_listed]                     */
    const int32_t  *gene_row_start;    /* 1-based                              */
    const int32_t  *gene_row_end;      /* 1-based closed                       */
    const uint8_t  *gene_row_flags;    /* RSQC_FF_*                            */
    const uint32_t *gene_row_id;       /* gene id of the row                   */

    /* `exon` rows, sorted                                                      */
    const int32_t  *exon_row_contig;   /* [n_exons]                            */
    const int32_t  *exon_row_start;
    const int32_t  *exon_row_end;
    const uint8_t  *exon_row_flags;
    const uint32_t *exon_row_id;       /* exon id (exonList index)             */
    const uint32_t *exon_row_gene;     /* gene id named by the row's gene_id   */

    /* per gene id                                                              */
    const uint8_t  *gene_is_globin;    /* [n_genes] geneNames[gene] in the 12-name
                                          blacklist (src/Expression.cpp:24,396-398) */
    /* exonsForGene (src/RNASeQC.cpp:153-154): CSR over gene id -> sorted exon ROW
       indices, in sorted order                                                 */
    const uint32_t *gene_exon_off;     /* [n_genes + 1]                        */
    const uint32_t *gene_exon_row;     /* [n_exons]                            */

    /* optional (may both be NULL), read only under rsqc_params.legacy: the position of each kept row in the
       GTF (any strictly increasing key, e.g. the line number).  The legacy rules depend on the order of the
       reference's ONE start-sorted list of genes and exons (stable sort, src/RNASeQC.cpp:150-152), i.e. on how
       a gene row and an exon row with the same start are ordered.  When NULL, gene rows are taken to precede
       exon rows of the same start (a GTF whose gene lines precede their exon lines).                        */
    const uint32_t *gene_row_order;    /* [n_genes_listed]                     */
    const uint32_t *exon_row_order;    /* [n_exons]                            */
} rsqc_annotation;

/* ---- BED intervals for the fragment-size sampler (src/BED.cpp:18-45):
 * stored +1/+1 like the reference (start = bed_start+1, end = bed_end+1),
 * per contig in file order, which must be ascending by start               */
typedef struct rsqc_bed {
    int32_t n_intervals;
    const int32_t *contig;             /* contig id (same id space as above)   */
    const int32_t *start;
    const int32_t *end;
} rsqc_bed;

/* ---- reference sequence for the GC statistics of --fasta (src/Fasta.cpp, bioio.hpp): what the reference reads
 * through its .fai index, handed over as plain per-contig base strings (FASTA text without line ends, any case;
 * G/g/C/c count, everything else does not -- gc(), src/Fasta.cpp:67-74).  Contigs the FASTA index does not name
 * are simply absent (Fasta::hasContig).  The library keeps one bit per base in HBM.                             */
typedef struct rsqc_reference {
    int32_t n;                         /* contigs named by the FASTA index     */
    const int32_t  *contig;            /* [n] boundary contig id               */
    const uint64_t *length;            /* [n] bases                            */
    const uint8_t *const *sequence;    /* [n] `length[i]` ASCII bases each     */
} rsqc_reference;
#define RSQC_GC_BINS 100               /* unsigned long gcBins[100], src/RNASeQC.cpp:106 */

/* ---- one batch of alignment records, file order ----------------------------
 * 32 bytes per record + 4 bytes per CIGAR op, stored as two
 * arrays of 16-byte half-records so that a wavefront reads each with one
 * 16-byte-per-lane vector load (1 KiB per wave instruction).  Records of one
 * contig form a segment; tid itself is not stored per record.               */
typedef struct rsqc_rec_core {         /* 16 bytes                             */
    int32_t  pos;                      /* core.pos (0-based)                   */
    int32_t  mpos;                     /* core.mpos                            */
    int32_t  isize;                    /* core.isize                           */
    uint32_t cigar_off;                /* first op of the record in `cigar`    */
} rsqc_rec_core;

typedef struct rsqc_rec_aux {          /* 16 bytes                             */
    uint64_t qhash;                    /* rsqc_qname_hash(QNAME)               */
    uint16_t flag;
    uint16_t l_qseq;                   /* core.l_qseq, RSQC_LQSEQ_ESCAPE = wide */
    uint8_t  mapq;
    uint8_t  nm;                       /* NM value, RSQC_NM_ESCAPE = wide      */
    uint8_t  tagbits;                  /* RSQC_TB_*                            */
    uint8_t  n_cigar;                  /* RSQC_NCIGAR_ESCAPE = wide            */
} rsqc_rec_aux;

/* Limits of one batch: n < 2^32 - 16 records, n_cigar_total < 2^30 ops (split larger inputs into several
 * batches; 1-4 M records per batch is the intended granularity).                                          */
typedef struct rsqc_batch {
    uint64_t n;                        /* records                              */
    uint64_t file_index_base;          /* index of record 0 in the whole file: a batch is a contiguous range of the
                                          file, batches are submitted in ascending order (gaps allowed: the records
                                          of other shards); decides the fragment-size cut-off and the shard merge */
    const rsqc_rec_core *core;         /* [n]                                  */
    const rsqc_rec_aux  *aux;          /* [n]                                  */
    const uint32_t *cigar;             /* BAM packed ops: len<<4 | op          */
    uint64_t n_cigar_total;

    /* contig segments: records [seg_start[s], seg_start[s+1]) have tid seg_tid[s];
       tid may be -1 (unplaced) or >= n_ref (unrecognised RefID)                */
    uint32_t n_seg;
    const int32_t  *seg_tid;           /* [n_seg]                              */
    const uint64_t *seg_start;         /* [n_seg + 1]                          */

    /* wide table for records carrying an escape value, ascending by index     */
    uint32_t n_wide;
    const uint64_t *wide_index;        /* record index within the batch        */
    const int32_t  *wide_nm;
    const int32_t  *wide_l_qseq;
    const uint32_t *wide_n_cigar;

    /* optional (may be NULL): exact QNAMEs, used only by the oracle to check
       that hashing does not change the fragment de-duplication               */
    const uint32_t *qname_off;         /* [n + 1]                              */
    const char     *qname;

    /* optional (may be NULL): a SECOND, independent hash of every record's QNAME (rsqc_qname_hash2).  With it the hot path
       identifies a read name by 96 bits -- (qhash, qhash2) compared exactly in the fragment de-duplication (src/Expression.cpp:
       383-387 compares the strings): two different names are merged only if BOTH hashes collide.  Without it the identity is the
       64-bit qhash alone.  The 32-byte record itself has no room for it (its layout is the contract's: 32 + 4 n_cigar bytes per
       record); the column is read only for records that are counted to a gene.  Both ingest paths of the library (the device
       decode and the host reader) fill it.  Every QNAME-keyed stage uses the same identity: geneFragmentCounts, the fragment-size
       sampler (src/Expression.cpp:511-531) and the fragment GC pairing (:461-474).  ALL OR NONE: the batches of one pass (between
       two rsqc_reset) either all carry the column or none does -- a submit that disagrees with the pass's first batch fails with
       RSQC_ERR_ARG (the two mates of a fragment would otherwise carry (qhash, h2) and (qhash, 0): two names).
       LIMIT: names that share their 64-bit qhash and differ in qhash2 are counted exactly up to 33 of them per fragment partition
       (a gene's names of one hash stripe, ~1 000 records); more is RSQC_ERR_CAPACITY, never a miscount.  rsqc_qname_hash values of
       real read names do not collide at all at these sizes; a crafted 64-bit collision costs ~5e9 hash evaluations each.     */
    const uint32_t *qhash2;            /* [n]                                  */

    /* optional (may be NULL): the batch is SEVERAL ranges of the file, one per contig segment -- seg_file_index[s] is the file index of
       segment s's first record (ascending, every range behind the one before and behind everything submitted earlier); the
       file index of record i of segment s is seg_file_index[s] + (i - seg_start[s]) and file_index_base is ignored.  A GPU
       that owns a set of NON-ADJACENT contigs of a sorted file (a contig-sharded run) submits them as ONE batch and
       one kernel launch; the order-dependent outputs are then kept per segment (rsqc_shard_summary lists one entry per segment
       instead of one per batch) and the context's own "Read Length" is composed from them in file order.  Since ABI version 4.  */
    const uint64_t *seg_file_index;    /* [n_seg]                              */

    /* optional (may be NULL): the UMI key of every record (rsqc_umi_pack of its UMI; 0 = no usable UMI).  Since ABI version 7.  Read ONLY
       in a pass that collects for UMI-aware duplicate marking (rsqc_markdup_use_umi, below): everywhere else the column is ignored
       and never dereferenced.  In such a pass it is ALL OR NONE like qhash2, with the difference that it must be there: a batch
       without the column is RSQC_ERR_ARG and leaves the collection as it was.  Both ingest paths of the library fill it when
       rsqc_decode_params.umi_source selects a source (the host reader: --umi-tag / --umi-qname); rsqc_decode_window.device_batch.umi
       then points at the window's column.  It stays in the collection (8 bytes per record): the sorted output batches do not
       carry it.                                                                                                              */
    const uint64_t *umi;               /* [n]                                  */
} rsqc_batch;

/* ---- results ---------------------------------------------------------------- */
typedef struct rsqc_results {
    int32_t  n_genes_listed, n_exons;
    /* geneCounts / uniqueGeneCounts / geneFragmentCounts (src/Metrics.cpp:20) */
    const uint64_t *gene_reads;        /* [n_genes_listed], geneList order     */
    const uint64_t *gene_unique;
    const uint64_t *gene_fragments;
    /* exonCounts: sum of intersection/alignedLength (src/Expression.cpp:345,
       src/Metrics.cpp:63); exon_hit != 0 iff the exon has a map entry (Q7)    */
    const double   *exon_reads;        /* [n_exons], exonList order            */
    const uint8_t  *exon_hit;
    uint64_t counters[RSQC_N_COUNTERS];
    int32_t  read_length;              /* "Read Length" (src/RNASeQC.cpp:275-278) */

    /* BaseCoverage::compute per listed gene (src/Metrics.cpp:132-151,265-337):
       coverage.tsv row (mean, std, cv); cov_valid == 0 -> row "0 0 nan" and the
       gene is absent from geneMeans/Stds/CVs                                  */
    const double   *gene_cov_mean;     /* [n_genes_listed]                     */
    const double   *gene_cov_std;
    const double   *gene_cov_cv;
    const uint8_t  *gene_cov_valid;
    /* per-exon CV (exon_cv.tsv): exon_cv_valid != 0 iff finite CV was stored  */
    const double   *exon_cv;           /* [n_exons]                            */
    const uint8_t  *exon_cv_valid;
    /* BiasCounter accumulators (src/Metrics.h:76-77)                          */
    const uint64_t *bias_three;        /* [n_genes_listed]                     */
    const uint64_t *bias_five;

    /* fragment size histogram (map<long long, unsigned long>), ascending size */
    uint32_t n_fragment_sizes;
    const int64_t  *fragment_size;
    const uint64_t *fragment_count;
    uint32_t fragment_samples_remaining;

    /* --fasta (valid when have_reference != 0): fragment GC histogram gcBins (src/RNASeQC.cpp:366-369, bin =
       unsigned(gc * 100)); a fragment of 100 % GC indexes past the reference's array (undefined there) and is
       counted in gc_out_of_range instead.  exon_gc = gc() of the exon's sequence as fetched at
       src/Metrics.cpp:301 (-1 when the FASTA lacks the contig); meaningful where exon_cv_valid != 0.              */
    int32_t  have_reference;
    const uint64_t *gc_bins;           /* [RSQC_GC_BINS]                       */
    uint64_t gc_out_of_range;
    const double   *exon_gc;           /* [n_exons], exonList order            */
    /* ABI 5: exon rows of the annotation that lie outside the row of their gene (0 for a well-formed GTF).  Non-zero means that
       gene_fragments and the coverage / bias statistics of THOSE genes are computed "as if the gene stayed in the window" and can
       differ from the reference's streamed result (rsqc_set_annotation's warning): the divergence is flagged in the
       results themselves, not only in rsqc_last_error, which any later failure overwrites.                                    */
    uint32_t exons_outside_gene_row;
} rsqc_results;

/* ---- timing of the device work (HIP events on the context's own stream) --- */
typedef struct rsqc_timing {
    double   classify_ms;              /* sum of K1 classify_count launches since reset */
    uint64_t classify_launches;
    uint64_t classify_records;
    uint64_t classify_bytes;           /* algorithmic bytes: 32*n + 4*n_cigar_total     */
    double   finalize_ms;              /* de-dup + coverage scan/stats + bias           */
    double   h2d_ms;                   /* rsqc_submit host->device copies               */
    uint64_t slow_records;             /* records the general (slow-path) kernel took in the last finalized pass */
    double   fragment_sizes_ms;        /* --bed runs: the fragment-size stage of the end-of-file passes (host clock around its kernels and its
                                          two read-backs; src/Expression.cpp:482-540), summed since reset                              */
    double   classify_long_ms;         /* ABI 5: the launches of classify_long_kernel (the ~1 % of the records the per-record kernel defers: more than
                                          eight CIGAR operations or more than three blocks) since reset; NOT part of classify_ms             */
} rsqc_timing;

typedef struct rsqc_ctx rsqc_ctx;

/* Creates a context on params->device.  Fails with RSQC_ERR_NO_DEVICE when no
 * HIP device is usable -- the product has no CPU path.                        */
RSQC_API int rsqc_create(const rsqc_params *params, rsqc_ctx **out);
RSQC_API void rsqc_destroy(rsqc_ctx *ctx);

/* Copies the annotation into HBM and builds the device index.  `owned_contig`
 * (n_contigs bytes, may be NULL = all) marks the contigs of this shard: only
 * their genes get coverage/bias results (multi-GPU by contig).
 * RSQC_OK may come WITH A WARNING in rsqc_last_error (empty otherwise): an exon row outside the row of its gene.  The
 * reference runs such a GTF and prints "Gene encountered after computing coverage" (src/Metrics.cpp:108-112) when a read
 * reaches the exon after the gene row has left its window; here every record is answered from the rows as given: counters,
 * gene reads / unique reads and exon reads are the reference's, fragment counts and coverage statistics of THAT gene are
 * computed as if the gene had stayed in the window.                                                        */
RSQC_API int rsqc_set_annotation(rsqc_ctx *ctx, const rsqc_annotation *ann,
                        const uint8_t *owned_contig);
RSQC_API int rsqc_set_bed(rsqc_ctx *ctx, const rsqc_bed *bed);
/* --fasta: after rsqc_set_annotation.  Copies the bases to the device, packs them to one G/C bit per base and
 * computes the per-exon GC values; the caller's strings are not referenced afterwards.                          */
RSQC_API int rsqc_set_reference(rsqc_ctx *ctx, const rsqc_reference *ref);

/* Asynchronous: copies the batch H2D on the context's stream and launches the
 * per-read kernels; returns without waiting for either.  The batch memory must
 * stay valid and unmodified until rsqc_wait() (page-locked arrays from
 * rsqc_host_alloc are copied by DMA).  Batches must be submitted in file order. */
RSQC_API int rsqc_submit(rsqc_ctx *ctx, const rsqc_batch *batch);
RSQC_API int rsqc_wait(rsqc_ctx *ctx);

/* Resident variant (what bench.py times): upload once, run many times.       */
RSQC_API int rsqc_upload(rsqc_ctx *ctx, const rsqc_batch *batch, int *handle_out);
RSQC_API int rsqc_submit_resident(rsqc_ctx *ctx, int handle);
RSQC_API int rsqc_release(rsqc_ctx *ctx, int handle);

/* End of file: fragment de-dup, coverage scan, per-gene coverage statistics and
 * bias windows, fragment-size pairing; fills `out`, whose vectors point into a
 * page-locked host mirror owned by the context (valid until the next
 * rsqc_finalize / rsqc_refresh_results / rsqc_destroy).                       */
RSQC_API int rsqc_finalize(rsqc_ctx *ctx, rsqc_results *out);

/* Zeroes every accumulator (keeps annotation/BED and uploaded batches).       */
RSQC_API int rsqc_reset(rsqc_ctx *ctx);

/* Replaces a context's inputs (additive to ABI 5): waits for everything in flight, then returns the context to its state
 * after rsqc_create -- rsqc_set_annotation, rsqc_set_bed and rsqc_set_reference are legal again, for an annotation with other
 * contigs, genes and exons.  Released: the annotation, BED and reference tables, the accumulators and their host mirror, the
 * coverage array, the interval index's rank table, whatever the open pass had emitted (a pass that was not finalized is
 * dropped, an open rsqc_decode_* stream with it) and the sticky error.  Kept: the streams, the event pools, the per-batch
 * buffer pools, the decode window buffers, the timing sums and the resident batches (rsqc_upload) -- whose contig ids then
 * have to mean something in the next annotation.  The vectors of an earlier rsqc_results are invalid afterwards.  Not for a
 * context that is a member of a live rsqc_group.                                                                        */
RSQC_API int rsqc_clear_inputs(rsqc_ctx *ctx);

RSQC_API int rsqc_get_timing(rsqc_ctx *ctx, rsqc_timing *out);
RSQC_API int rsqc_reset_timing(rsqc_ctx *ctx);

/* Device-resident raw accumulators for an in-place RCCL reduction by the host
 * (torch.distributed).  Pointers are HIP device pointers owned by the ctx.
 * Layout: u64 gene_reads[n_genes] | gene_unique[n_genes] | gene_fragments[n_genes]
 * | counters[RSQC_N_COUNTERS] in one allocation; f64 exon_reads[n_exons] (row
 * order) in another.  Valid after rsqc_finalize().                            */
RSQC_API int rsqc_device_accumulators(rsqc_ctx *ctx, void **u64_base, uint64_t *u64_count,
                             void **f64_base, uint64_t *f64_count);
/* Everything a contig-sharded run exchanges, as three device ranges of one element type each, to
 * be sum-reduced in place across the ranks (RCCL all_reduce, SUM) between rsqc_finalize_device and
 * rsqc_refresh_results:
 *   [0] u64: gene_reads | gene_unique | gene_fragments | counters | bias_three | bias_five
 *   [1] f64: exon_reads | gene_cov_mean | gene_cov_std | gene_cov_cv | exon_cv
 *   [2] u8 : gene_cov_valid | exon_cv_valid (padded to 8 bytes each)
 * Counts and exon sums are additive; the per-gene / per-exon statistics are written by the owner of the gene's
 * contig only and stay zero elsewhere, so the same sum is their merge (a NaN CV stays NaN).  rsqc_device_accumulators
 * exposes the additive prefixes of [0] and [1] only.                                                              */
typedef struct rsqc_device_range { void *base; uint64_t count; } rsqc_device_range;
RSQC_API int rsqc_device_vectors(rsqc_ctx *ctx, rsqc_device_range out[3]);
/* The order-dependent outputs of a shard, for the host-side merge of a contig-sharded run; valid
 * after rsqc_finalize / rsqc_finalize_device until the next reset.  Pointers are owned by the context.
 *   Read Length (src/RNASeQC.cpp:275-278) is a state machine over the file.  Per submitted batch the library keeps
 *   the batch's transfer function as a short table: entered with state r, the batch leaves rl_state[k] for the first k
 *   in [rl_offset[b], rl_offset[b+1]) with rl_span[k] > r, and r itself when no entry qualifies.  Composing the
 *   batches of ALL shards in ascending batch_file_index from state 0 gives the reference's value.
 *   LIMIT: the keys of a table are the prefix maxima of the alignment span over the batch's (the range's) records that reach :275, and
 *   one batch or range holds at most 128 of them (RSQC_RL_MAXP).  Reads of ONE length need a single entry whatever their spans; with
 *   mixed lengths every record whose span exceeds all spans before it in the batch adds one.  A batch or range beyond the limit sets
 *   the device error word: the pass ends with RSQC_ERR_CAPACITY at the next rsqc_wait / rsqc_finalize (never with a value), and
 *   rsqc_last_error names Read Length, the batch or range by its file index and the number 128.  rsqc_reset starts a new pass;
 *   smaller batches (the limit is per batch, not per file) avoid it.
 *   Fragment sizes (src/Expression.cpp:482-540): mates pair inside one BED interval, hence inside one shard; the
 *   cut-off --fragment-samples applies in FILE order.  The shard hands over the samples it kept (its first N by the file
 *   index of the completing record, in no particular order); the merged histogram holds the N smallest file indices
 *   of the union.                                                                                                   */
typedef struct rsqc_shard_info {
    uint32_t n_batches;
    const uint64_t *batch_file_index;  /* [n_batches] file_index_base of the batch (of the SEGMENT for a batch with seg_file_index: one entry per segment) */
    const uint64_t *batch_records;     /* [n_batches]                               */
    const uint32_t *rl_offset;         /* [n_batches + 1]                           */
    const uint32_t *rl_span;           /* ascending inside a batch                  */
    const int32_t  *rl_state;
    uint32_t n_samples;
    const uint64_t *sample_file_index; /* [n_samples] unordered                     */
    const uint32_t *sample_size;       /* [n_samples] abs(InsertSize)               */
} rsqc_shard_info;
RSQC_API int rsqc_shard_summary(rsqc_ctx *ctx, rsqc_shard_info *out);
/* dst += src over those three ranges, for ONE process that drives several GPUs (the command line with --gpus): the
 * peer's ranges cross xGMI by hipMemcpyPeerAsync and are added on dst's device.  Both contexts must hold the same
 * annotation and be past rsqc_finalize_device.  A process-per-GPU host uses an RCCL all_reduce on the ranges instead.  */
RSQC_API int rsqc_reduce_peer(rsqc_ctx *dst, rsqc_ctx *src);
/* The exchange step of ONE process that drives n GPUs (the command line with --gpus): the three ranges of every context
 * are sum-reduced onto ctxs[0] with one RCCL ncclReduce per range inside one group call, each GPU's part on its context's
 * stream, over communicators made with ncclCommInitAll on the contexts' devices (src/RNASeQC.cpp:385-394 is the reference's
 * end-of-file window).  librccl is bound at run time; without it, or when two contexts share a device
 * (a communicator cannot), the peer-copy path of rsqc_reduce_peer is taken instead.  *used_rccl (may be NULL) says which. */
RSQC_API int rsqc_reduce_group(rsqc_ctx **ctxs, int n, int *used_rccl);
/* The same exchange with the communicators made ONCE, outside the caller's timed region: rsqc_group_create brings RCCL up on
 * the contexts' devices (any time after rsqc_create; ncclCommInitAll over eight GPUs takes longer than the BAM loop of a
 * 100 M-record file, so the command line calls it beside the GTF parse, before the reference's `Average Reads/Sec` window
 * opens); rsqc_group_reduce = what rsqc_reduce_group does at end of file, on the group's communicators.  A group whose
 * communicators cannot be made (no librccl, RSQC_NO_RCCL, two contexts on one device, ncclCommInitAll failing for lack of
 * P2P or shared memory) is still a valid group: it sums the shards by peer copies, and rsqc_group_info says why.  An RCCL
 * failure AFTER reductions were issued is fatal (ctxs[0] may hold partial sums); one before takes the peer path.          */
typedef struct rsqc_group rsqc_group;
RSQC_API int rsqc_group_create(rsqc_ctx **ctxs, int n, rsqc_group **out);
RSQC_API int rsqc_group_reduce(rsqc_group *group, int *used_rccl);
RSQC_API int rsqc_group_info(const rsqc_group *group, int *uses_rccl, double *init_ms, double *last_reduce_ms, const char **note);
RSQC_API void rsqc_group_destroy(rsqc_group *group);
/* Re-reads the (reduced) device accumulators into the results struct.         */
RSQC_API int rsqc_refresh_results(rsqc_ctx *ctx, rsqc_results *out);
/* Page-locked host memory for the arrays of an rsqc_batch: rsqc_submit then copies by DMA and returns without
 * waiting for the transfer (arrays from ordinary memory work too, through the driver's staging copy).
 * NULL when no device is available.                                                                       */
RSQC_API void *rsqc_host_alloc(size_t bytes);
RSQC_API void rsqc_host_free(void *p);
/* rsqc_finalize without the read-back: runs the end-of-file stage and leaves every result on the device
 * (multi-GPU runs reduce the accumulators first and read back once with rsqc_refresh_results).            */
RSQC_API int rsqc_finalize_device(rsqc_ctx *ctx);

/* ---- device-side BAM decode --------------------------------------------------------------
 * The input side of the per-read path, moved to the GPU: the caller reads the file and hops over the BGZF block
 * headers (src/BamReader.cpp:12-20 does this through htslib's bgzf.c, one thread, inflate included); inflating
 * (one wavefront per block), finding the records and parsing them into an rsqc_batch run on the device, and the
 * batch is submitted as by rsqc_submit.  One stream of consecutive blocks between rsqc_decode_begin and
 * rsqc_decode_end; a record that straddles two calls is carried over on the device.                              */
typedef struct rsqc_bgzf_block {
    uint64_t in_offset;                /* first DEFLATE byte of the block, from `compressed`                   */
    uint32_t in_bytes;                 /* DEFLATE bytes (BSIZE + 1 - XLEN - 20)                                */
    uint32_t out_bytes;                /* ISIZE (<= 65536)                                                     */
    uint32_t crc32;                    /* of the inflated bytes (the gzip trailer)                             */
    uint32_t flags;                    /* RSQC_BGZF_*                                                          */
} rsqc_bgzf_block;
/* The block has been inflated by the caller (spare CPU threads sharing the work with the GPU): in_offset locates its
 * INFLATED bytes in `compressed`, in_bytes == out_bytes, the CRC-32 has been checked.  Such blocks form one run at the
 * END of a call's table, their bytes one after the other in `compressed`.                                          */
#define RSQC_BGZF_INFLATED 1u
#define RSQC_UMI_SOURCE_NONE  0
#define RSQC_UMI_SOURCE_TAG   1
#define RSQC_UMI_SOURCE_QNAME 2
typedef struct rsqc_decode_params {
    int32_t n_ref;                     /* reference sequences in the BAM header                                */
    int32_t has_chimeric_tag;          /* --chimeric-tag (readStringTag, src/RNASeQC.cpp:780-800)              */
    char    chimeric_tag[2];
    char    filter_tag[RSQC_MAX_FILTER_TAGS][2];   /* params.n_filter_tags names; {0,0} never matches          */
    uint64_t file_index_base;          /* index of the stream's first record in the whole file                 */
    int32_t  pipelined;                /* 1: a call returns once its kernels are enqueued; the NEXT call (or rsqc_decode_end)
                                          completes it, so `out` then describes the call before -- the next chunk of the
                                          file crosses PCIe beside this call's kernels                            */
    /* ABI 7 (the four bytes that were `reserved`): where a record's UMI comes from.  RSQC_UMI_SOURCE_NONE: the windows get no umi
       column -- it is neither allocated nor written, no kernel changes.  _TAG: the FIRST aux field named umi_tag of type Z (BAM: the
       bytes up to its NUL; SAM: the text behind XX:Z:); another type, no such field, or one cut off by a malformed aux tail is key 0.
       _QNAME: the bytes of QNAME behind its last umi_sep; no separator, or nothing behind it, is key 0.                         */
    uint8_t  umi_source;
    char     umi_tag[2];
    char     umi_sep;
    uint64_t reserve_inflated_bytes;   /* 0, or: size the device buffers at rsqc_decode_begin for calls of up to this many
                                          inflated bytes (they grow on demand otherwise, which costs a re-allocation
                                          of every window buffer each time a larger call arrives)                 */
} rsqc_decode_params;
typedef struct rsqc_decode_window {    /* what one rsqc_decode_submit decoded (arrays owned by the context, valid until its next decode call) */
    uint64_t n_records;
    uint32_t n_runs;                   /* runs of consecutive records on one reference sequence ...            */
    const int32_t *run_tid;            /* ... their RefIDs, in file order (the batch's contig segments)        */
    rsqc_batch device_batch;           /* NON-PIPELINED streams only (all zero otherwise): the decoded records as the boundary's SoA
                                          batch, every pointer a DEVICE pointer into the context's window buffers (valid until its
                                          next decode call; n == n_records): what the per-read kernels were given -- a host that
                                          wants the columns copies them out with hipMemcpy after rsqc_wait.  A pipelined stream
                                          returns window n from submit n + 1, which has already queued window n + 1's kernels
                                          into the same buffers: there is no moment at which the pointers could be read          */
} rsqc_decode_window;
typedef struct rsqc_decode_info {
    rsqc_decode_window last;           /* pipelined streams: what the last rsqc_decode_submit decoded            */
    uint64_t records;                  /* records decoded and submitted since rsqc_decode_begin                */
    int32_t  unsorted;                 /* a record starts before its predecessor on the same contig, judged on primary,
                                          mapped, QC-passed records: the reference's sort warning (src/RNASeQC.cpp:354) */
    int32_t  n_bad_refid;              /* records whose RefID the header does not define (:333-337) ...        */
    const char *const *bad_refid;      /* ... and the first 64 of their names (owned by the context)           */
} rsqc_decode_info;
RSQC_API int rsqc_decode_begin(rsqc_ctx *ctx, const rsqc_decode_params *p);
/* Inflates n_blocks consecutive blocks behind what the stream already holds, decodes every complete record and submits
 * them as one batch (asynchronous like rsqc_submit; `compressed` may be reused when the call returns).
 * skip_bytes: inflated bytes at the start of the first block that precede the first record (the BAM header, or the
 * in-block part of a virtual file offset) -- only in a call that starts on a record boundary.
 * limit_bytes: 0, or the inflated offset (counted from the first block of THIS call) at which the wanted range ends:
 * records that start there or later are left out.  out (may be NULL): what the call decoded.
 * Limits per call: 1.9 GiB of inflated data.  Size the calls by their BLOCKS, not by their file bytes: one wavefront inflates one
 * block and an MI355X holds 5 120 of them, so a call should carry several times that many (the command line: 1 GiB of inflated
 * data, about 16 000 blocks); a call with about as many blocks as wave slots takes as long as one block takes one wave.       */
RSQC_API int rsqc_decode_submit(rsqc_ctx *ctx, const void *compressed, uint64_t compressed_bytes,
                                const rsqc_bgzf_block *blocks, uint32_t n_blocks,
                                uint32_t skip_bytes, uint64_t limit_bytes, rsqc_decode_window *out);
/* End of the stream: RSQC_ERR_INPUT if an incomplete record is left over ("truncated BAM record").             */
RSQC_API int rsqc_decode_end(rsqc_ctx *ctx, rsqc_decode_info *out);

/* ---- device-side SAM text decode ------------------------------------------------------------------------------
 * The same stream for SAM input (the reference opens SAM, BGZF-compressed SAM and BAM alike through htslib, src/BamReader.h):
 * plain text through rsqc_decode_submit_text, BGZF-compressed SAM through rsqc_decode_submit (blocks as for BAM; skip_bytes
 * may cover the header text).  ref_names: the header's @SQ SN values in order, p->n_ref of them (copied).  Lines starting with
 * '@' in front of the stream's first alignment are header lines and are skipped; any other malformed line (fewer than 11
 * fields, a number that does not parse or overflows its column, an unknown CIGAR operator, SEQ / CIGAR or SEQ / QUAL
 * lengths that differ, a '@' line after the first alignment) is RSQC_ERR_INPUT, and rsqc_last_error names its 1-based line
 * number, counted from the first byte of the stream.  An RNAME the names do not hold, and POS 0 on a named reference, give
 * RefID -1 and the unmapped flag bit.  The bytes after a call's last '\n' are carried to the next call on the device; a last
 * line without '\n' is ended by rsqc_decode_end.  rsqc_decode_end / rsqc_decode_info as for BAM (bad_refid: the names
 * of judged records with RefID -1).                                                                                         */
RSQC_API int rsqc_decode_begin_sam(rsqc_ctx *ctx, const rsqc_decode_params *p, const char *const *ref_names);
RSQC_API int rsqc_decode_submit_text(rsqc_ctx *ctx, const void *text, uint64_t bytes, rsqc_decode_window *out);

/* ---- input in any order (ABI 6) ----------------------------------------------------------------------------------
 * Every rule of the per-read path assumes a coordinate-sorted file.  Between rsqc_sort_begin and rsqc_sort_end the context COLLECTS
 * instead: every record that reaches it -- through rsqc_submit, rsqc_submit_resident, rsqc_decode_submit or
 * rsqc_decode_submit_text -- is appended to a device-resident collection (a stream-ordered device copy: the decode paths' window
 * buffers and the caller's arrays are free again under the usual rules) and no per-read kernel runs.  Batches may arrive in any
 * order, file_index_base is ignored, a batch with seg_file_index is RSQC_ERR_ARG, the qhash2 all-or-none rule holds as ever.
 * rsqc_sort_begin: after the inputs are set and before the pass's first submit (RSQC_ERR_ARG behind one).
 * rsqc_sort_end (behind rsqc_decode_end, if a decode stream fed the collection): orders the collection STABLY by (tid as unsigned 32
 * bits, pos as signed) -- unplaced records (tid -1) last, ties in arrival order -- with a radix sort on the device, forms ordinary
 * batches of at most RSQC_SORT_BATCH records (environment; default 2 097 152) and runs them in order as rsqc_submit_resident would;
 * a record's file index is its rank in that order.  The context is then in the state those submits leave: rsqc_finalize,
 * rsqc_reset, rsqc_shard_summary and rsqc_get_timing behave as ever.  rsqc_reset and rsqc_clear_inputs also leave the collecting
 * mode and free the collection.  The whole input is resident: 44 bytes per record and 4 per CIGAR operation collected -- in columns
 * that grow by doubling, so up to twice that is allocated, and three times what has been collected while a column is being grown
 * (the old one goes as soon as its copy is through) -- and 16 more per record while sorting; batches uploaded by rsqc_submit stay
 * on the device until rsqc_wait, as ever.  A collection the device cannot hold (or of 2^32 - 16 records and more) is
 * RSQC_ERR_CAPACITY with the sizes in rsqc_last_error -- never a partial result: a batch lost while collecting (capacity, a HIP
 * error) and any failure of rsqc_sort_end void the pass, every later call returns that code until rsqc_reset; a batch REFUSED with
 * RSQC_ERR_ARG leaves the collection as it was.  rsqc_finalize between the two calls is RSQC_ERR_ARG.                              */
typedef struct rsqc_sort_info {
    uint64_t records;                  /* collected and run                                                          */
    uint64_t batches_in, batches_out;  /* non-empty batches collected; batches the per-read kernels were given       */
    uint64_t moved;                    /* records whose rank differs from their arrival index                         */
    double   key_ms, sort_ms, gather_ms;   /* the reduction over the keys with its read-back; the radix passes; forming the output batches */
    int32_t  was_sorted;               /* the collection was in order already: no radix pass ran                      */
} rsqc_sort_info;
RSQC_API int rsqc_sort_begin(rsqc_ctx *ctx);
RSQC_API int rsqc_sort_end(rsqc_ctx *ctx, rsqc_sort_info *out);

/* ---- duplicate fragments flagged on the collection (additive to ABI 6) -----------------------------------------------------
 * Behind rsqc_markdup_begin, rsqc_sort_end first runs one block of device work on the complete collection that REWRITES flag 0x400
 * of every record; the per-read kernels then see those flags.  No per-read kernel, no other launch and no other output changes.
 * The contract, in integers (tests/markdup_ref.py is its executable form; no equality with Picard or samtools is claimed):
 *   population   a record is in it iff (flag & (0x4 | 0x100 | 0x200 | 0x800)) == 0 and its contig id (the tid of its segment, as the
 *                collection's key column holds it) is >= 0 as a signed number.  Only population records can anchor a fragment.
 *   u5           the unclipped 5' coordinate, in 32-bit two's-complement arithmetic (wrap-around is part of the contract).  Forward
 *                strand (0x10 clear): pos - the lengths of the leading run of S / H operations.  Reverse strand: pos + the reference
 *                length (M D N = X) + the lengths of the trailing run of S / H.  I and P contribute nothing, nor does an operation
 *                code above 8 (the per-read kernels report that record later).  A record without CIGAR has u5 = pos; a record
 *                stored with the n_cigar escape takes its length from the wide table; no read passes the collected operations.
 *   kind, anchor SINGLE (0): not paired (0x1 clear) or mate unmapped (0x8) -- the record itself anchors.  PAIR (1): paired, mate
 *                mapped, RSQC_TB_MTID_SAME -- the mate with pos < mpos, or pos == mpos and 0x40 set, anchors.  SPLIT (2): paired, mate
 *                mapped, mate on another contig -- the record with 0x40 anchors.  A fragment without an anchor is never judged.
 *   signature    of an anchor: (tid, u5, rev = 0x10, mrev = 0x20 (0 for SINGLE), kind, w) with w = isize for PAIR, mpos for SPLIT,
 *                0 for SINGLE.
 *   sets         anchors with equal signatures form a set; its survivor is the anchor with the highest mapq, ties keep the earliest
 *                in arrival order; every other anchor of the set is a duplicate fragment.
 *   verdicts     a record leaves with 0x400 set iff its name equals the name of a duplicate anchor -- every record of the
 *                collection, whatever its flags or placement.  The name is (qhash, qhash2), or qhash alone in a pass without the
 *                qhash2 column.  Every other record leaves with 0x400 clear: flags the input carried are replaced.
 *   limits       the mate's own clipping is seen only through isize (the key UMI-tools uses, not Picard's); a SPLIT signature does
 *                not know the mate's contig; no rule makes a SINGLE read a duplicate of a pair's end; base qualities are not in
 *                the record, so mapq picks the survivor; an input whose names are not unique per fragment gets every record of a
 *                flagged name flagged.
 * rsqc_markdup_begin: behind rsqc_sort_begin and before the pass's first submit (RSQC_ERR_ARG otherwise); in any order relative to
 * rsqc_junctions_begin and rsqc_track_begin.  rsqc_markdup_end: behind rsqc_sort_end (RSQC_ERR_ARG otherwise); a second call returns
 * the same figures without device work.  rsqc_markdup_verdicts: one byte (0 or 1) per record of the collection in ARRIVAL order, rows
 * [first, first + n); the host array is owned by the context and valid until its next call.  Memory during the stage: 44 bytes per
 * anchor (two key columns and the sort's two key buffers, the record index and the sort's two payload buffers), half a byte per anchor
 * for the digit histograms, 4 bytes per 256 records, 4 bytes per slot of the name table (a power of two >= twice the duplicate fragments, >= 1024) and one byte per record; all but the last is released before the
 * coordinate sort allocates.  An allocation the device refuses is RSQC_ERR_CAPACITY with the sizes in rsqc_last_error and voids the
 * pass as a failing rsqc_sort_end does: never a partly marked run.  rsqc_reset, rsqc_clear_inputs and rsqc_destroy end the mode.     */
typedef struct rsqc_markdup_info {
    uint64_t records, population, anchors, sets, duplicate_fragments;
    uint64_t flagged_records;          /* records that leave with 0x400 set                                           */
    uint64_t cleared_records;          /* records that arrived with 0x400 and leave without                           */
    double   sig_ms, sort_ms, mark_ms; /* anchors and signatures; the two sort stages; heads, name set and apply (host clocks, as rsqc_sort_info's) */
} rsqc_markdup_info;
RSQC_API int rsqc_markdup_begin(rsqc_ctx *ctx);
RSQC_API int rsqc_markdup_end(rsqc_ctx *ctx, rsqc_markdup_info *out);
RSQC_API int rsqc_markdup_verdicts(rsqc_ctx *ctx, uint64_t first, uint64_t n, const uint8_t **dup);

/* ---- UMI-aware duplicate marking (ABI 7) --------------------------------------------------------------------------------------
 * rsqc_markdup_use_umi makes the pass's marking UMI-aware.  The contract is the one above with ONE change: the signature of an anchor
 * becomes (tid, u5, rev, mrev, kind, w, umi), umi being the anchor RECORD's own key in rsqc_batch.umi (rsqc_umi_pack); the mate's key is
 * never consulted.  Anchors with key 0 (no usable UMI) form sets among themselves: an anchor without a UMI is never a duplicate of one
 * that has one.  Survivor, verdicts and the name rule are unchanged.  tests/markdup_umi_ref.py is the executable form.
 *   limits       UMIs match exactly (unless rsqc_markdup_umi_edits, below, groups UMIs one substitution apart); only the anchor's UMI counts; a UMI has at most 31 bases;
 *                an N (any byte other than A C G T in either case and the joiners - and +) voids the UMI: key 0.
 * rsqc_markdup_use_umi: behind rsqc_markdup_begin and before the pass's first submit (RSQC_ERR_ARG otherwise).  Every batch of the
 * pass must then carry rsqc_batch.umi (see there).  rsqc_markdup_umi_end: behind rsqc_sort_end of such a pass (RSQC_ERR_ARG otherwise);
 * a second call returns the same figures.  position_duplicate_fragments is what the marking WITHOUT the UMI would have called on
 * the same collection (anchors minus distinct position signatures): beside rsqc_markdup_info.duplicate_fragments it says how many
 * fragments the UMIs rescued.  rsqc_markdup_info and rsqc_markdup_end are as without the mode.
 * Order and memory: the anchors are sorted by (K_hi, K_lo >> 8, umi, 255 - mapq, arrival) -- LSD in four stages: the mapq byte, the
 * live digits of the UMI keys, K_lo above its mapq byte, K_hi; dead digit positions are skipped in all of them.  The collection holds
 * 8 more bytes per record (the umi column: 52 instead of 44), the stage 8 more bytes per anchor (the anchors' keys: 52 instead of 44);
 * both go with the stage's other buffers before the coordinate sort allocates, and the sorted output batches never see the column.
 * rsqc_reset, rsqc_clear_inputs and rsqc_destroy end the mode.                                                                   */
typedef struct rsqc_markdup_umi_info {
    uint64_t anchors_with_umi;         /* anchors whose key is not 0                                                  */
    uint64_t anchors_without_umi;
    uint64_t position_duplicate_fragments;
} rsqc_markdup_umi_info;
RSQC_API int rsqc_markdup_use_umi(rsqc_ctx *ctx);
RSQC_API int rsqc_markdup_umi_end(rsqc_ctx *ctx, rsqc_markdup_umi_info *out);

/* ---- UMIs one substitution apart grouped before marking (additive to ABI 7: two functions and one struct) -----------------------
 * rsqc_markdup_umi_edits(ctx, 1) changes the contract of rsqc_markdup_use_umi in ONE point: the signature's last component is the ROOT
 * of the anchor's UMI, not the UMI itself.  In integers (tests/markdup_umi_group_ref.py is the executable form; no equality with
 * UMI-tools, fgbio or samtools markdup --barcode-* is claimed):
 *   nodes        a position set P is the set of anchors with equal (tid, u5, rev, mrev, kind, w).  Inside P a node is one distinct UMI
 *                key k; its count c(k) is the number of ANCHORS (not records) of P that carry k.  Key 0 is a node too: it has no
 *                neighbours, never gets a parent and is never one.
 *   neighbours   two non-zero keys of the same number of bases L that differ in exactly one base: k' = k ^ (x << 2j), x in {1, 2, 3},
 *                0 <= j < L.  Keys of different L are never neighbours: no insertions or deletions.  The joiners are gone from the
 *                key: ACGT-TGCA is 8 bases, one substitution allowed anywhere in them.
 *   eligible     a neighbour p of k in the SAME P is an eligible parent when c(p) >= 2 c(k) - 1 (the `directional` threshold, in 64
 *                bits) AND (c(p) > c(k), or c(p) == c(k) and p < k as integers).  Equal counts pass the first test only at c = 1; the
 *                second test makes the relation acyclic.
 *   parent       the eligible neighbour with the highest count, ties to the smallest key; without one, k is a root.
 *   root         root(k) follows parents to a root; the signature is P + (root(k),).  Survivor (the highest mapq, the earliest arrival
 *                on ties, over ALL anchors of the grouped set, whichever node they came from), verdicts by name, population, anchors,
 *                flag rewriting and cleared_records are unchanged.
 *   figures      rsqc_markdup_info.sets and .duplicate_fragments are those of the grouped signature; rsqc_markdup_umi_info is
 *                unchanged (position_duplicate_fragments does not depend on grouping).  umi_nodes: nodes over all position sets;
 *                merged_nodes: nodes with a parent; exact_duplicate_fragments = anchors - umi_nodes: what exact matching would have
 *                called; group_ms: host clock around the grouping kernels.  duplicate_fragments == exact_duplicate_fragments +
 *                merged_nodes and position_duplicate_fragments >= duplicate_fragments >= exact_duplicate_fragments are checked after
 *                read-back (RSQC_ERR_HIP otherwise).
 *   limits       edit distance 1 only, substitutions only; the anchor's UMI only; one parent per node, chosen locally (UMI-tools'
 *                directional method searches from the highest count down and may assign a node otherwise).
 * rsqc_markdup_umi_edits: behind rsqc_markdup_use_umi and before the pass's first submit; max_edits is 0 (exact matching: no launch,
 * allocation or output differs from a pass without the call) or 1; RSQC_ERR_ARG otherwise.  rsqc_markdup_umi_group_end: behind
 * rsqc_sort_end of a pass with max_edits 1 (RSQC_ERR_ARG otherwise); a second call returns the same figures without device work.
 * Memory with max_edits 1: 16 more bytes per anchor during the stage (68 instead of 52: the position marks, which become the final
 * marks, and three node columns sized by the anchor count); the other node columns -- 28 bytes per node: key, best anchor, group's
 * best anchor, parent, root -- live in buffers the sort is done with.  All of it goes with the stage's other buffers.  rsqc_reset,
 * rsqc_clear_inputs and rsqc_destroy end the mode.                                                                                  */
typedef struct rsqc_markdup_umi_group_info {
    uint64_t umi_nodes, merged_nodes, exact_duplicate_fragments;
    double   group_ms;
} rsqc_markdup_umi_group_info;
RSQC_API int rsqc_markdup_umi_edits(rsqc_ctx *ctx, uint32_t max_edits);
RSQC_API int rsqc_markdup_umi_group_end(rsqc_ctx *ctx, rsqc_markdup_umi_group_info *out);

/* ---- reads per splice junction (additive to ABI 6) ---------------------------------------------------------------------
 * Between rsqc_junctions_begin and the end of the pass every batch that the per-read kernels run also leaves its splice-junction
 * INSTANCES on the device (one extra kernel per batch; no other kernel, output or launch changes), and rsqc_junctions_end orders
 * and reduces them to one row per junction.  The contract, in integers:
 *   population   a record contributes iff (flag & (0x4 | 0x100 | 0x200 | 0x800)) == 0 and its segment's tid is in [0, n_contigs).
 *                Nothing else gates it: not -q, the tag filters, --exclude-chimeric, --legacy, --unpaired, --stranded, nor the
 *                duplicate flag.
 *   walk         p = pos (64 bits); the operations in order (a wide record: its true count): an N of length L >= 1 is one instance
 *                (tid, start = p + 1, end = p + L) -- 1-based closed, the intron's first and last base, STAR's SJ.out.tab
 *                convention; M D N = X advance p.  An N of length 0 yields nothing; an instance whose end exceeds 2^31 - 1 is dropped;
 *                an N without an aligned block on one side still counts.
 *   overhang     of an instance: min(left, right), the sums of the M = X lengths between the previous N (of any length; or the
 *                record's start) and this N, and from this N to the next N (or the record's end).  D I S H P add nothing.
 *   table        one row per distinct (tid, start, end), ascending in that order: reads = instances, hq_reads = instances of records
 *                with mapq >= params.mapq_threshold (the complement of the "Low Mapping Quality" test), max_overhang = the largest
 *                overhang among them.  It does not depend on the order of the records or on how they are cut into batches.
 * rsqc_junctions_begin: after rsqc_set_annotation and before the pass's first submit (RSQC_ERR_ARG otherwise); with rsqc_sort_begin in
 * either order -- the instances are then taken from the sorted output batches.  rsqc_junctions_end: behind rsqc_finalize or
 * rsqc_finalize_device of that pass (RSQC_ERR_ARG otherwise); a second call returns the same table without new device work.  The
 * arrays are owned by the context and stay valid until its next rsqc_reset, rsqc_clear_inputs or rsqc_destroy, which also end the
 * mode and forget the instances.  The collection (16 bytes per instance) grows by doubling from 65 536 instances (environment:
 * RSQC_JUNCTION_CAP0) to a bound the host computes without the device -- half the CIGAR operations submitted so far; an instance
 * beyond it, or 2^32 - 16 instances and more, is RSQC_ERR_CAPACITY, never a partial table.  Not exchanged by rsqc_reduce_* /
 * rsqc_group_*: a sharded run keeps one table per context.                                                                        */
typedef struct rsqc_junction_table {
    uint64_t n, instances, population; /* rows; instances; contributing records                                       */
    const int32_t *tid, *start, *end;  /* [n] contig id, first and last base of the intron (1-based closed)           */
    const uint32_t *reads, *hq_reads, *max_overhang;   /* [n]                                                         */
    double extract_ms, sort_ms, reduce_ms;   /* the per-batch kernels (HIP events); the two sort stages; heads, scan and rows (host clocks) */
} rsqc_junction_table;
RSQC_API int rsqc_junctions_begin(rsqc_ctx *ctx);
RSQC_API int rsqc_junctions_end(rsqc_ctx *ctx, rsqc_junction_table *out);

/* ---- per-base coverage track as bedGraph rows (additive to ABI 6) --------------------------------------------------------
 * Between rsqc_track_begin and the end of the pass every batch that the per-read kernels run also adds its coverage events to a
 * device-resident difference array (one extra kernel per batch; no other kernel, output or launch changes); rsqc_track_end turns
 * it into rows on the device, rsqc_track_rows / rsqc_track_text bring windows of them to the host.  The contract, in integers:
 *   contigs      the n contigs handed to rsqc_track_begin (the header's @SQ entries in order) with their lengths, each at most
 *                2^31 - 1; names may be NULL (they are needed for text only), at most 255 bytes each.
 *   population   a record contributes iff (flag & (0x4 | 0x100 | 0x200 | 0x800)) == 0 and its segment's tid is in [0, n): the
 *                population of rsqc_junctions_*.  Nothing else gates it, the duplicate flag included; two mates are two records.
 *   walk         p = pos, in 64 bits.  M = X of length L >= 1 cover [p, p + L) and advance p; D and N advance p and cover nothing;
 *                I S H P do neither; an operation of length 0 does nothing; a wide record's true count is used, clamped to the
 *                batch's pool.  What lies outside [0, length[tid]) is counted in no depth: its bases are clipped_bases, the
 *                bases inside are aligned_bases.
 *   depth        of a position: the number of covering intervals, exact up to 2^32 - 1.
 *   rows         maximal runs of positions of ONE contig with equal, non-zero depth: (tid, start, end, depth), start 0-based, end
 *                exclusive, ascending by (tid, start).  The sum of (end - start) * depth is aligned_bases.  The table does not
 *                depend on the order of the records or on how they are cut into batches.
 *   text         name<TAB>start<TAB>end<TAB>depth<LF> per row, in decimal; no header or track line; no rows, no bytes.
 * rsqc_track_begin: after rsqc_set_annotation and before the pass's first submit (RSQC_ERR_ARG otherwise); with rsqc_sort_begin and
 * rsqc_junctions_begin in any order (under rsqc_sort_begin the events come from the sorted output batches).  It allocates the
 * array -- 4 bytes per position and contig pad -- or keeps the one of an earlier pass that is large enough, and zeroes it on the
 * stream; the environment's RSQC_TRACK_MAX_BYTES (default: no bound) makes it return RSQC_ERR_CAPACITY for a larger array.
 * rsqc_track_end: behind rsqc_finalize or rsqc_finalize_device of that pass; a second call returns the same figures without device
 * work.  2^32 - 16 rows or more, or an allocation the device refuses, is RSQC_ERR_CAPACITY with the sizes in rsqc_last_error, never
 * a partial table.  rsqc_track_rows / rsqc_track_text: rows [first, first + n) behind rsqc_track_end; the host arrays are owned by
 * the context and valid until the next of these two calls; text takes at most 4 194 304 rows a call and needs the names
 * (RSQC_ERR_ARG without).  rsqc_reset, rsqc_clear_inputs and rsqc_destroy end the mode; rsqc_reset keeps the array's allocation.
 * Not exchanged by rsqc_reduce_* / rsqc_group_*.                                                                                  */
typedef struct rsqc_track_info {
    uint64_t n_rows, population, aligned_bases, clipped_bases, positions;   /* positions: the sum of the lengths            */
    double events_ms, scan_ms, rows_ms;   /* the per-batch kernels (HIP events); the prefix sum; count + rows (host clocks) */
} rsqc_track_info;
RSQC_API int rsqc_track_begin(rsqc_ctx *ctx, int32_t n, const uint64_t *length, const char *const *name /* may be NULL */);
RSQC_API int rsqc_track_end(rsqc_ctx *ctx, rsqc_track_info *out);
RSQC_API int rsqc_track_rows(rsqc_ctx *ctx, uint64_t first, uint64_t n, const int32_t **tid, const uint32_t **start, const uint32_t **end, const uint32_t **depth);
RSQC_API int rsqc_track_text(rsqc_ctx *ctx, uint64_t first, uint64_t n, const char **text, uint64_t *bytes);

/* ---- coverage along the gene body, 5' to 3' (additive to ABI 6) ----------------------------------------------------------
 * Behind rsqc_track_end the track's array holds the depth of every reference position; rsqc_genebody_end walks every gene's
 * model positions in transcript order and sums the depth into RSQC_GENEBODY_BINS bins per gene, in one kernel at the end of the
 * pass (no per-read kernel and no launch of a pass without the calls changes).  The contract, in integers:
 *   model        a gene's model is a list of segments (tid, start, end), 0-based with end exclusive.  All segments of one gene
 *                lie on one contig of the track and inside [0, length[tid]).  They are non-empty, ascending and disjoint;
 *                abutting segments are allowed.  Each gene carries one `reverse` byte.  A gene may have zero segments.  L is
 *                the sum of the segment lengths.
 *   coordinate   for a model position p, u is the number of model bases in front of it in genomic order; t = u for a forward
 *                gene, t = L - 1 - u for a `reverse` gene; bin(p) = floor(t * 100 / L), computed with a 64-bit product.
 *   sums         sum[g][k] is the total of depth(p) over the positions of gene g with bin(p) = k: uint64_t and exact.  depth is
 *                the track's: population and CIGAR rules are those of rsqc_track_*, nothing here re-defines them.  Genes with
 *                L < 100 are not measured: their 100 sums are 0.  Genes that share positions each see the full depth.
 *   info         n_genes; n_measured: genes with L >= 100; model_bases: the sum of L over measured genes; depth_sum: the sum
 *                of all bins; bins_ms: HIP events around the stage.
 * The sums do not depend on record order, on how the input is cut into batches, or on RSQC_TRACK_MERGE.
 * rsqc_genebody_begin: behind rsqc_track_begin of the same pass and before the pass's first submit (RSQC_ERR_ARG otherwise).  It
 * validates the model rules (a violation is RSQC_ERR_ARG with a message that names the gene and the rule), builds the launch plan
 * on the host -- every measured gene's [0, L) cut into items of at most 4096 model bases, so that the work is balanced by bases --
 * and uploads model and plan; a device refusal is RSQC_ERR_CAPACITY with the sizes.  Memory beyond the track's: 800 bytes per
 * gene, 12 bytes per segment, 24 bytes per item of the plan.  rsqc_genebody_end: behind rsqc_track_end (RSQC_ERR_ARG otherwise);
 * a second call returns the same figures without device work; a failure voids the pass until rsqc_reset, as with
 * rsqc_track_end.  rsqc_genebody_sums: the n * 100 values of genes [first_gene, first_gene + n), behind rsqc_genebody_end; the
 * host array is owned by the context and valid until its next call.  rsqc_reset, rsqc_clear_inputs and rsqc_destroy end the
 * mode; rsqc_reset keeps the allocations.  Not exchanged by rsqc_reduce_* / rsqc_group_*.                                       */
#define RSQC_GENEBODY_BINS 100
typedef struct rsqc_genebody_info {
    uint64_t n_genes, n_measured, model_bases, depth_sum;
    double bins_ms;
} rsqc_genebody_info;
RSQC_API int rsqc_genebody_begin(rsqc_ctx *ctx, int32_t n_genes, const uint32_t *seg_off /*[n_genes+1]*/,
                                 const int32_t *seg_tid, const uint32_t *seg_start, const uint32_t *seg_end,
                                 const uint8_t *reverse /*[n_genes]*/);
RSQC_API int rsqc_genebody_end(rsqc_ctx *ctx, rsqc_genebody_info *out);
RSQC_API int rsqc_genebody_sums(rsqc_ctx *ctx, uint32_t first_gene, uint32_t n, const uint64_t **sums);

/* ---- per-gene transcript integrity from the coverage track (additive to ABI 7) ----------------------------------------------
 * Behind rsqc_track_end the track's array holds the depth of every reference position; rsqc_tin_end walks every gene's model
 * positions and leaves, per gene, the four figures that the evenness of its coverage (TIN = 100 * exp(H) / L, H the Shannon
 * entropy of the depth along the gene) is made of -- two kernels at the end of the pass, no per-read kernel and no launch of a
 * pass without the calls changes.  No equality with RSeQC's tin.py is claimed: every model position counts here.  The contract:
 *   model        the model of rsqc_genebody_begin without the `reverse` byte (the figures are symmetric in the strand): gene g
 *                owns rows [seg_off[g], seg_off[g + 1]) of (seg_tid, seg_start, seg_end), 0-based with end exclusive, all on one
 *                contig of the track and inside [0, length[tid]), non-empty, ascending and disjoint; abutting rows are allowed; a
 *                gene may have no row.  L is the sum of the segment lengths.  A gene is measured when L >= 1.
 *   depth        depth(p) is the track's: population, CIGAR rules and clipping are those of rsqc_track_*.
 *   row          rsqc_tin_row of every gene (all zero for L = 0), over its model positions p:
 *                depth_sum = S = sum of depth(p); covered = the positions with depth(p) > 0; max_depth = the largest depth(p) --
 *                all three exact; dlog2d = E = sum of depth(p) * log2(depth(p)) over the positions with depth(p) >= 2 (depths 0
 *                and 1 contribute exactly 0).  Genes that share positions each see the full depth.
 *   the double   E is reproducible: the order of its additions is fixed (a lane adds its positions in order, the wave combines its
 *                lanes with a fixed butterfly, every plan item writes its partial to a slot of its own, a gene's items are added
 *                in item order; no floating atomic), so on one device two passes over the same records give bit-identical E in
 *                any record order, with any batch cuts, under rsqc_sort_begin and with RSQC_TRACK_MERGE 0 or 1.  Against the
 *                exactly rounded sum its relative error is at most (items_g + 80) * 2^-52, items_g = ceil(L / 4096); E = 0 is
 *                exact.
 *   info         n_genes; n_measured: genes with L >= 1; model_bases: the sum of L; depth_sum: the sum of S; covered_bases: the
 *                sum of covered (both added on the host from the rows); tin_ms: HIP events around the stage's kernels.
 *   TIN          with H = ln(S) - E * ln(2) / S:  tin = 100 * exp(H) / L.  Uniform coverage gives 100, one covered base 100 / L,
 *                depth 1 on C positions 100 * C / L.  (The command line prints it for genes with L >= 100 and S >= L.)
 * rsqc_tin_begin: behind rsqc_track_begin of the same pass and before the pass's first submit (RSQC_ERR_ARG otherwise), in any
 * order relative to rsqc_genebody_begin: both may be active in one pass, each with model buffers of its own.  It validates the
 * model rules (a violation is RSQC_ERR_ARG with a message that names the gene and the rule; the pass goes on without the mode),
 * builds the launch plan on the host -- every measured gene's [0, L) cut into items of at most 4096 model bases -- and uploads
 * model and plan; a device refusal is RSQC_ERR_CAPACITY with the sizes.  Memory beyond the track's, on the device: 24 bytes per
 * gene (the rows), 24 bytes per item (the partials), 12 bytes per segment (the model), and the plan's 20 bytes per item and 8 bytes
 * per gene; on the host 24 page-locked bytes per gene.  rsqc_tin_end: behind rsqc_track_end (RSQC_ERR_ARG otherwise); a second
 * call returns the same figures without device work; a failure voids the pass until rsqc_reset and never leaves partial rows.
 * rsqc_tin_rows: the rows of genes [first_gene, first_gene + n), behind rsqc_tin_end: a window into page-locked memory that the
 * context owns, valid until the mode ends; a window out of range is RSQC_ERR_ARG.  rsqc_reset, rsqc_clear_inputs and
 * rsqc_destroy end the mode; rsqc_reset keeps the allocations.  Not exchanged by rsqc_reduce_* / rsqc_group_*.                   */
typedef struct rsqc_tin_row {
    uint64_t depth_sum;
    uint32_t covered, max_depth;
    double dlog2d;
} rsqc_tin_row;
typedef struct rsqc_tin_info {
    uint64_t n_genes, n_measured, model_bases, depth_sum, covered_bases;
    double tin_ms;
} rsqc_tin_info;
RSQC_API int rsqc_tin_begin(rsqc_ctx *ctx, int32_t n_genes, const uint32_t *seg_off /*[n_genes+1]*/,
                            const int32_t *seg_tid, const uint32_t *seg_start, const uint32_t *seg_end);
RSQC_API int rsqc_tin_end(rsqc_ctx *ctx, rsqc_tin_info *out);
RSQC_API int rsqc_tin_rows(rsqc_ctx *ctx, uint32_t first_gene, uint32_t n, const rsqc_tin_row **rows);

/* ---- base quality and composition by read cycle (additive to ABI 7) -----------------------------------------------------------
 * The device decode (rsqc_decode_*) inflates SEQ and QUAL of every record into device memory; with the mode on, one more kernel per
 * window counts them by read cycle.  No launch, allocation or output of a pass without the calls changes.  No equality with FastQC,
 * Picard or RSeQC is claimed; tests/cycle_ref.py is the contract's executable form.  The contract, in integers:
 *   population   records with flag & (0x100 | 0x200 | 0x800) == 0; nothing else gates a record (not the mapping quality, the tag
 *                filters, rsqc_params.legacy / unpaired, 0x4 or 0x400): every read counts once, unmapped ones included.
 *   end          e = 1 when flag & 0x1, flag & 0x80 and not flag & 0x40; otherwise e = 0.
 *   length       L = l_seq (BAM); the length of SEQ, 0 when SEQ is * (SAM).  L = 0 adds 1 to no_seq_records and nothing else.  A BAM
 *                record whose fixed part does not fit its block_size (32 + l_read_name + 4 n_cigar + (L + 1) / 2 + L), whose l_seq
 *                is negative or whose l_read_name is 0 contributes nothing (what the decode makes of such a record is unchanged).
 *   cycle        query index i of [0, L) is cycle c = i when flag & 0x10 == 0 and c = L - 1 - i otherwise (hard clips are not part of
 *                SEQ and shift nothing).  A base with c >= RSQC_CYCLE_MAX adds 1 to beyond_bases and to nothing else.
 *   base         columns A C G T other = 0..4.  BAM nibbles 1, 2, 4, 8 are 0, 1, 2, 3, every other nibble 4; SAM bytes A C G T in
 *                either case are 0, 1, 2, 3, every other byte 4.  Under flag & 0x10 a base b < 4 becomes 3 - b.  base[e][c][b] += 1.
 *   quality      missing when BAM qual[0] == 0xFF or SAM QUAL is exactly * (also for L = 1): no_qual_records += 1, the bases still
 *                count.  Otherwise q = the BAM byte, or the SAM byte - 33 with a floor of 0; q > 63 is stored as 63 and adds 1 to
 *                clamped_quals.  qual[e][c][q] += 1.
 *   tables       base[RSQC_CYCLE_ENDS][RSQC_CYCLE_MAX][5] and qual[RSQC_CYCLE_ENDS][RSQC_CYCLE_MAX][RSQC_CYCLE_QBINS], uint64_t.
 *   info         seen_records: every record the pass's windows submitted (== rsqc_decode_info.records) plus those of rsqc_cycles_add;
 *                records: the population with L > 0; bases: the sum of base; cycles_ms: HIP events around the stage's kernels.
 *   checks       behind the read-back: bases + beyond_bases equals the sum of L over the population (the device adds it up in one
 *                more word); for every (e, c) the sum of qual is at most the sum of base.  A violation is RSQC_ERR_HIP.
 * The tables do not depend on the order of the records, on how the input is cut into calls and windows, on pipelining, or on the
 * spelling of the input: the same alignments as BAM, plain SAM and BGZF SAM give identical tables.
 * rsqc_cycles_begin: behind rsqc_create and before the pass's first submit or rsqc_decode_begin* (RSQC_ERR_ARG behind either).  It
 * allocates the tables -- 2 * 512 * (5 + 64) * 8 bytes and a few words on the device, the same in page-locked host memory; a refusal
 * is RSQC_ERR_CAPACITY with the sizes.  Only windows of rsqc_decode_submit / rsqc_decode_submit_text are counted: batches that arrive
 * through rsqc_submit / rsqc_submit_resident carry no SEQ and contribute nothing.  rsqc_cycles_add adds host-computed counts (input whose
 * bytes never reach the device as bytes: a host reader): base and qual in the layout above (either may be NULL), of `partial` the
 * fields seen_records, records, no_seq_records, no_qual_records, bases (which must be the sum of `base`), beyond_bases, clamped_quals;
 * between rsqc_cycles_begin and rsqc_cycles_end.  rsqc_cycles_end: behind the pass's rsqc_decode_end, or behind the last submit of a
 * pass the host read (RSQC_ERR_ARG while a stream is open); the tables are the context's, in page-locked memory, valid until the mode
 * ends; a second call returns the same figures without device work.  rsqc_reset, rsqc_clear_inputs and rsqc_destroy end the mode;
 * rsqc_reset keeps the allocation.  Not exchanged by rsqc_reduce_* / rsqc_group_*.                                                  */
#define RSQC_CYCLE_MAX 512
#define RSQC_CYCLE_QBINS 64
#define RSQC_CYCLE_ENDS 2
#define RSQC_CYCLE_BASES 5
typedef struct rsqc_cycle_info {
    uint64_t seen_records, records, no_seq_records, no_qual_records, bases, beyond_bases, clamped_quals;
    double cycles_ms;
} rsqc_cycle_info;
RSQC_API int rsqc_cycles_begin(rsqc_ctx *ctx);
RSQC_API int rsqc_cycles_add(rsqc_ctx *ctx, const uint64_t *base, const uint64_t *qual, const rsqc_cycle_info *partial);
RSQC_API int rsqc_cycles_end(rsqc_ctx *ctx, rsqc_cycle_info *out, const uint64_t **base, const uint64_t **qual);

/* ---- errors by read cycle against the reference (additive to ABI 7) ------------------------------------------------------------
 * With the mode on, one more kernel per decode window walks every record's CIGAR over its SEQ, its QUAL and the reference, which the
 * device keeps at four bits per base.  No launch, allocation or output of a pass without the calls changes.  No equality with Picard,
 * RSeQC or samtools stats is claimed; tests/mismatch_ref.py is the contract's executable form.  The contract, in integers (end, cycle,
 * the base codes of BAM nibbles and SAM bytes, the quality value, its clamp and a missing quality are those of the section above):
 *   reference    n contigs, the header's @SQ entries in order (the tid space of rsqc_track_begin), each with length[i] and sequence[i]:
 *                ASCII, or NULL when the FASTA lacks the contig.  Reference code r: A C G T in either case 0..3, every other byte 4.
 *                On the device: 4 bits per base, 8 bases per 32-bit word (base 8 w + k in bits [4 k, 4 k + 4)), a word offset per contig.
 *   classes      every record the windows submit is in exactly one, tested in this order:
 *                1. flag & (0x4 | 0x100 | 0x200 | 0x800) != 0: counted nowhere but in seen_records;
 *                2. tid outside [0, n) or no sequence for it: no_reference_records;  3. mapq < min_mapq: low_mapq_records;
 *                4. L = 0: no_seq_records;  5. the lengths of the M I S = X operations do not add up to L (a record without operations
 *                included): inconsistent_records;  6. otherwise records -- only these touch the tables.
 *                Nothing else gates a record (not the mapping quality of rsqc_params, the tag filters, legacy, 0x400).  A BAM record whose
 *                fixed part does not fit its block_size or whose l_read_name is 0 contributes nothing, as in the section above.  A missing
 *                quality adds 1 to no_qual_records; the bases still count.
 *   walk         e = the end of flag; query index q = 0; reference position p = pos (64 bits).  The operations in order (a wide record's
 *                true count; the real CIGAR of a record that keeps it in CG:B,I).  Length 0 does nothing; H, P and codes above 8 do
 *                nothing.  For a query index i, c = its cycle; a query base with c >= 512 adds 1 to beyond_bases and to nothing else.
 *                M = X of length n, k in [0, n): b = the raw base code of index q + k (no strand rule), r = the reference code at p + k,
 *                  4 when p + k < 0 or p + k >= length[tid].  b < 4 and r < 4: compared[e][c] += 1, subst[e][R][B] += 1 with (R, B) =
 *                  (r, b), or (3 - r, 3 - b) under flag & 0x10 (the matrix reads in the orientation of the sequenced read); b != r:
 *                  mismatch[e][c] += 1; with qualities, v = the clamped quality (a clamp counts in clamped_quals): byq[v].compared += 1,
 *                  byq[v].mismatched += 1 on a mismatch.  Otherwise uncompared[e][c] += 1.  Then q += n, p += n.
 *                I: inserted[e][c] += 1 per base, insertion_events += 1, q += n.      S: clipped[e][c] += 1 per base, q += n.
 *                D: one event at i = min(q, L - 1): deletions[e][c] += 1 when c < 512; deletion_events += 1, deleted_bases += n, p += n.
 *                N: p += n.
 *   tables       uint64_t: cyc[2][512][RSQC_MISMATCH_COLS] with the columns compared, mismatch, uncompared, inserted, clipped,
 *                deletions; subst[2][4][4] ([end][reference][read]); byq[64][2] ([quality][compared, mismatched]).
 *   info         seen_records: every record the pass's windows submitted plus those of rsqc_mismatch_add; the class counts; compared ..
 *                deletions: the sums of the columns; mismatch_ms: HIP events around the stage's kernels.
 *   checks       behind the read-back (the device sums L over `records` in one more word): compared + uncompared + inserted + clipped +
 *                beyond_bases equals that sum; mismatch <= compared in every cell; the sum of subst[e] equals the sum of compared[e][.],
 *                its off-diagonal the sum of mismatch[e][.]; the sum of byq.compared is at most compared.  A violation is RSQC_ERR_HIP
 *                and voids the pass until rsqc_reset.
 * The tables do not depend on the order of the records, on how the input is cut into calls and windows, on pipelining, or on the
 * spelling of the input: the same alignments as BAM, plain SAM and BGZF SAM give identical tables.
 * rsqc_mismatch_begin: behind rsqc_create and before the pass's first submit or rsqc_decode_begin* (RSQC_ERR_ARG behind either).  It
 * stages each contig's bases through one buffer (the longest contig, once), packs them on the device (half a byte per base) and allocates
 * and zeroes the tables (under 60 KB on the device, as much page-locked); a refusal of memory is RSQC_ERR_CAPACITY with the sizes.
 * sequence == NULL reuses the packed reference of an earlier pass of this context with the same n and length -- it survives rsqc_reset;
 * RSQC_ERR_ARG when none is kept or n / length differ.  min_mapq: 0..255.  Only windows of rsqc_decode_submit / rsqc_decode_submit_text
 * are counted: batches through rsqc_submit / rsqc_submit_resident carry no SEQ and contribute nothing.  rsqc_mismatch_add adds
 * host-computed counts: the tables in the layout above (any may be NULL) and of `partial` every count field; compared .. deletions must
 * be the sums of the columns of `cyc`.  rsqc_mismatch_end: behind the pass's rsqc_decode_end (RSQC_ERR_ARG while a stream is open); the
 * tables are the context's, in page-locked memory, valid until the mode ends; a second call returns the same figures without device
 * work.  rsqc_reset, rsqc_clear_inputs and rsqc_destroy end the mode; rsqc_clear_inputs and rsqc_destroy also free the packed reference.
 * Not exchanged by rsqc_reduce_* / rsqc_group_*.                                                                                      */
#define RSQC_MISMATCH_COLS 6
typedef struct rsqc_mismatch_info {
    uint64_t seen_records, records, no_reference_records, low_mapq_records, no_seq_records, inconsistent_records, no_qual_records;
    uint64_t compared, mismatched, uncompared, inserted, clipped, deletions;
    uint64_t insertion_events, deletion_events, deleted_bases, beyond_bases, clamped_quals;
    double mismatch_ms;
} rsqc_mismatch_info;
RSQC_API int rsqc_mismatch_begin(rsqc_ctx *ctx, int32_t n, const uint64_t *length, const char *const *sequence, uint32_t min_mapq);
RSQC_API int rsqc_mismatch_add(rsqc_ctx *ctx, const uint64_t *cyc, const uint64_t *subst, const uint64_t *byq, const rsqc_mismatch_info *partial);
RSQC_API int rsqc_mismatch_end(rsqc_ctx *ctx, rsqc_mismatch_info *out, const uint64_t **cyc, const uint64_t **subst, const uint64_t **byq);

/* ---- base counts at known variant sites (additive to ABI 7) ----------------------------------------------------------------------
 * With the mode on, one more kernel per decode window takes a lane per record and counts which base the record shows at every site of a
 * sorted list that lies under one of its aligned blocks.  No launch, allocation or output of a pass without the calls changes.  No
 * equality with GATK ASEReadCounter, samtools mpileup or bcftools is claimed; tests/allele_ref.py is the contract's executable form.
 * The contract, in integers (the base codes of BAM nibbles and SAM bytes, the quality value and a missing quality are those of the
 * --cycles section above):
 *   sites        n_sites pairs (tid[k], pos[k]), 0-based, strictly ascending by (tid, pos) -- so without duplicates --, 0 <= tid <
 *                n_contigs (the header's @SQ entries in order), 0 <= pos < 2^31 - 1.  n_sites may be 0.  No contig length and no FASTA
 *                are needed.  On the device: pos[n_sites] and first[n_contigs + 1] (the sites of tid are [first[tid], first[tid + 1])).
 *   classes      every record the windows submit is in exactly one, tested in this order:
 *                1. flag & (0x4 | 0x100 | 0x200 | 0x800) != 0: counted nowhere but in seen_records;
 *                2. tid outside [0, n_contigs): off_contig_records;  3. mapq < min_mapq: low_mapq_records;  4. L = 0: no_seq_records;
 *                5. the lengths of the M I S = X operations do not add up to L (a record without operations included):
 *                inconsistent_records;  6. otherwise records -- only these are walked.
 *                Nothing else gates a record (not the mapping quality of rsqc_params, the tag filters, legacy, 0x400: flagged duplicates
 *                count; under duplicate marking the stage sees the input's flags).  A BAM record whose fixed part does not fit its
 *                block_size or whose l_read_name is 0 contributes nothing.  A record of class `records` without qualities adds 1 to
 *                no_qual_records.
 *   walk         query index q = 0; reference position p = pos (64 bits).  The operations in order (a wide record's true count; the
 *                real CIGAR of a record that keeps it in CG:B,I).  Length 0, H, P and codes above 8 do nothing.
 *                M = X of length n: for every site s of tid with p <= s.pos < p + n: i = q + (s.pos - p), b = the raw base code of
 *                  index i (no strand complement: SEQ and the alleles of a site are both in reference orientation); with qualities
 *                  and the quality value of i (the BAM byte, or the SAM byte - 33 floored at 0; no clamp) below min_baseq:
 *                  low_baseq[s] += 1; otherwise column b of s += 1 for b < 4, other[s] += 1 for b = 4.  A record without qualities
 *                  passes the quality test.  Then q += n, p += n.
 *                I, S: q += n; they cover no site.      D: deleted[s] += 1 for every site in [p, p + n); p += n.
 *                N: p += n; the sites under it get nothing.
 *   table        uint64_t counts[n_sites][RSQC_ALLELE_COLS] with the columns A C G T other deleted low_baseq.  One observation is one
 *                increment: the two mates of a pair are two records, and where they overlap a site it is observed twice.
 *   info         seen_records: every record the pass's windows submitted plus those of rsqc_alleles_add; the class counts;
 *                hit_records: records of class `records` with at least one observation; observations: the sum of the table;
 *                alleles_ms: HIP events around the stage's kernels, summed over the windows.
 *   checks       behind the read-back (the device adds its observations up in one more word, per lane in registers and one sum per
 *                workgroup): the sum of all cells equals that word plus what rsqc_alleles_add brought; hit_records <= records.  A
 *                violation is RSQC_ERR_HIP and voids the pass until rsqc_reset.
 * The table does not depend on the order of the records, on how the input is cut into calls and windows, on pipelining, or on the
 * spelling of the input: the same alignments as BAM, plain SAM and BGZF SAM give identical tables.
 * rsqc_alleles_begin: behind rsqc_create and before the pass's first submit or rsqc_decode_begin* (RSQC_ERR_ARG behind either).  A list
 * that is not strictly ascending, a tid or pos out of range (each message names the first offending index), min_mapq > 255 or
 * min_baseq > 93 is RSQC_ERR_ARG.  The sites go to the device at every call (4 bytes per site, 4 per contig); the cells are 64 bytes per
 * site on the device and as much page-locked; a refusal of memory is RSQC_ERR_CAPACITY with the sizes.  Only windows of
 * rsqc_decode_submit / rsqc_decode_submit_text are counted.  rsqc_alleles_add adds host-computed counts: `counts` in the layout above
 * (NULL: none) and every count field of `partial`; the sum of `counts` must equal partial->observations (RSQC_ERR_ARG otherwise, and
 * behind rsqc_alleles_end).  rsqc_alleles_end: behind the pass's rsqc_decode_end (RSQC_ERR_ARG while a stream is open); the table is the
 * context's, in page-locked memory, valid until the mode ends; a second call returns the same figures without device work.  rsqc_reset
 * ends the mode and forgets the counts; rsqc_clear_inputs and rsqc_destroy also free the buffers.  Not exchanged by rsqc_reduce_* /
 * rsqc_group_*.                                                                                                                        */
#define RSQC_ALLELE_COLS 7
typedef struct rsqc_allele_info {
    uint64_t seen_records, records, off_contig_records, low_mapq_records, no_seq_records, inconsistent_records, no_qual_records;
    uint64_t hit_records, observations, n_sites;
    double alleles_ms;
} rsqc_allele_info;
RSQC_API int rsqc_alleles_begin(rsqc_ctx *ctx, int32_t n_contigs, uint32_t n_sites, const int32_t *tid, const int32_t *pos, uint32_t min_mapq, uint32_t min_baseq);
RSQC_API int rsqc_alleles_add(rsqc_ctx *ctx, const uint64_t *counts /* [n_sites][RSQC_ALLELE_COLS] or NULL */, const rsqc_allele_info *partial);
RSQC_API int rsqc_alleles_end(rsqc_ctx *ctx, rsqc_allele_info *out, const uint64_t **counts);

RSQC_API const char *rsqc_strerror(int code);
RSQC_API const char *rsqc_last_error(rsqc_ctx *ctx);
RSQC_API const char *rsqc_counter_name(int counter);   /* the reference's Metrics key  */
RSQC_API const char *rsqc_version(void);               /* "RNASeQC 2.4.3 ..." prefix kept for
                                                 python/rnaseqc/run.py:25     */

/* QNAME hash used at the boundary (host decoders must use exactly this).     */
RSQC_API uint64_t rsqc_qname_hash(const char *name, size_t len);
/* the second hash of a name (rsqc_batch.qhash2): a multiply-xorshift recurrence with its own constants + the murmur3 fmix32
 * finaliser over (state ^ length); it shares no structure with the FNV-1a of rsqc_qname_hash                                  */
RSQC_API uint32_t rsqc_qname_hash2(const char *name, size_t len);
/* the UMI key (rsqc_batch.umi): A C G T in either case are 2 bits each, the first base most significant; - and + are skipped; the
 * key is (1 << 2L) | bits for L bases, so A, AA and AAA differ and no usable UMI gives 0; 0 = no usable UMI: nothing left, any
 * other byte (N included) or more than 31 bases.  Exact, not a hash.                                                          */
RSQC_API uint64_t rsqc_umi_pack(const char *umi, uint32_t len);

#ifdef __cplusplus
}
#endif
#endif /* RNASEQC_AMD_H */
