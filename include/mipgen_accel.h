/*
 * mipgen_accel.h — C-ABI drop-in boundary for the candidate-MIP enumeration + scoring hot path of MIPgen,
 * implemented as hand-written HIP kernels for gfx950 (MI355X).
 *
 * The reference (shendurelab/MIPGEN, C++03, single-threaded) has no FFI; the seam this library sits behind
 * is the body of mipgen::tile_regions' innermost loop and the mixed-mode re-scores
 * (file:line citations are into /root/reference):
 *
 *   reference call site / callee                                   replaced by
 *   -------------------------------------------------------------  -------------------------------------------
 *   mipgen.cpp:446-497  new Plus/MinusSVMipv4 + design_mip()        mipgen_accel_score_regions()  (dense grid)
 *                       + get_score() | get_parameters()+predict_value()
 *   mipgen.cpp:599-762  design_mip(Featurev5*, shared_ptr<SVMipv4>)  (same call; copies / masked / flags / SNP ints)
 *   SVMipv4.h:60        double SVMipv4::get_score()                  MIPGEN_SCORE_LOGISTIC
 *   SVMipv4.h:59        void SVMipv4::get_parameters(vector<double>&, double[])   mipgen_accel_score_candidates(.., features_out)
 *   mipgen.cpp:1948     double predict_value(vector<double>&, svm_model*)         MIPGEN_SCORE_SVR
 *   svm.h:78            svm_model* svm_load_model(const char*)      mipgen_accel_load_model_file()
 *   svm.h:88            double svm_predict(const svm_model*, const svm_node*)     (inside the SVR kernels)
 *   Featurev5.h:25      void Featurev5::get_long_range_content(string, string[])  mipgen_accel_long_range_content()
 *   mipgen.cpp:1525-1526,1535-1536,1548-1549,1875-1876  mixed-mode re-score        mipgen_accel_score_candidates()
 *   mipgen.cpp:426-437,494-497  score-dependent early exits (replay)               mipgen_accel_replay_condense()
 *   mipgen.cpp:1670-1746 condense_mips                                             mipgen_accel_replay_condense()
 *   mipgen.cpp:1616-1649 collapse_mips                                             mipgen_accel_collapse()
 *   mipgen.cpp:765-794   print_details (all_mips records)                          mipgen_accel_format_all_mips()
 *   mipgen.cpp:558-596,825-835 arm-oligo copy numbers through bwa                  mipgen_accel_count_oligo_copies()  (opt-in, exact matches)
 *   mipgen.cpp:412-524   tile_regions in -silent_mode (enumerate + score + condense of    mipgen_accel_score_condense_all()
 *                        every region, nothing kept per candidate)
 *
 * Conventions
 *   - plain C, plain pointers and sizes; no C++/torch types cross this boundary.
 *   - every entry point returns 0 on success, a negative MIPGEN_E_* code otherwise;
 *     mipgen_accel_last_error() returns a human-readable message for the calling thread's last failure.
 *     (reference: C++ `throw <int>` caught in main → exit 1, mipgen.cpp:2029-2035; svm_load_model → NULL, svm.cpp:2762.)
 *   - a handle is single-owner and not thread-safe (the reference is not re-entrant either: SURVEY.md section 5);
 *     one handle per GPU.  The library owns device buffers and the densified model; the caller owns every
 *     host array it passes in or receives results into.  Nothing is transferred across the boundary.
 *   - there is NO CPU fallback: if no HIP device is usable every call fails with MIPGEN_E_NODEVICE.
 *   - coordinates are 1-based inclusive chromosome positions, as in the reference.
 */
#ifndef MIPGEN_ACCEL_H
#define MIPGEN_ACCEL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI version.  Struct layouts are unchanged since 1; 2 marks BEHAVIOUR changes of existing entry points that a caller written against 1
 * must know about (result windows): mipgen_accel_score_resident fails with MIPGEN_E_STATE on a batch of several result windows;
 * mipgen_accel_download_replay's emitted counts / survivors and mipgen_accel_download_results' range are those of the window scored last;
 * copy fields saturated at 65535 mean "look the count up"; survivor / collapse downloads are validated per result window.
 * 3: SVR requests on parameter sets outside the tiled kernel's limits succeed (list route) instead of failing with MIPGEN_E_INVALID; a download may fail
 * with MIPGEN_E_STATE when a print-exact re-score list overflowed; new entry points (mipgen_accel_window_uniqueness_begin / _flags_region / _end,
 * mipgen_accel_set_dynamic_skip / _skipped_candidates / _skip_state).
 * 4: new entry points only (mipgen_accel_rescore_survivors / _download_survivor_scores, mipgen_accel_window_views, mipgen_accel_synchronize).
 * 5: new entry point only (mipgen_accel_set_window_breaks: the multi-device front end deals its regions in blocks, a window never spans two). */
#define MIPGEN_ACCEL_ABI_VERSION 6

#define MIPGEN_MAX_ARM_PAIRS 256     /* flattened (ext,lig) list, enumeration order */
#define MIPGEN_N_FEATURES 192        /* SVMipv4.cpp:14 TOTAL_FEATURES */
#define MIPGEN_N_LRC 44              /* Featurev5.h:4 MER_NUM */
#define MIPGEN_MIN_OLIGO 1
#define MIPGEN_MAX_OLIGO 64          /* arm lengths accepted by this library (reference default 16..30) */

/* error codes */
#define MIPGEN_OK 0
#define MIPGEN_E_INVALID (-1)        /* bad argument / inconsistent sizes */
#define MIPGEN_E_NODEVICE (-2)       /* no usable HIP device: this library has no CPU path */
#define MIPGEN_E_HIP (-3)            /* a HIP runtime call or kernel failed */
#define MIPGEN_E_MODEL (-4)          /* libsvm model missing / unparsable / unsupported kernel type */
#define MIPGEN_E_NOMEM (-5)
#define MIPGEN_E_STATE (-6)          /* call sequence error (e.g. scoring before regions are resident) */

/* score_method (mipgen.cpp:182,217; "-score_method") */
#define MIPGEN_SCORE_LOGISTIC 0
#define MIPGEN_SCORE_SVR 1
#define MIPGEN_SCORE_MIXED 2         /* logistic during enumeration, SVR on picked/tested MIPs */

/*
 * Run-wide parameters, parsed once on the host (the reference re-reads map<string,string> args inside the
 * hot loop: mipgen.cpp:467,469,476,494,619,626).
 */
typedef struct mipgen_params {
    int32_t abi_version;             /* MIPGEN_ACCEL_ABI_VERSION */
    int32_t score_method;            /* MIPGEN_SCORE_* */
    int32_t min_capture_size;        /* -min_capture_size  (mipgen.cpp:272) */
    int32_t max_capture_size;        /* -max_capture_size  (mipgen.cpp:271) */
    int32_t capture_increment;       /* -capture_increment (mipgen.cpp:273-274; 0 is coerced to 1) */
    int32_t max_mip_overlap;         /* -max_mip_overlap   (static size skip, mipgen.cpp:429) */
    /* flattened arm-length pairs in enumeration order: arm sum descending, then list order within the sum
     * (mipgen.cpp:431-442; lists built at :222-261).  arm_sum_of[i] = arm_ext[i] + arm_lig[i]. */
    int32_t n_arm_pairs;
    int32_t arm_ext[MIPGEN_MAX_ARM_PAIRS];
    int32_t arm_lig[MIPGEN_MAX_ARM_PAIRS];
    int32_t check_copy_number;       /* 0 iff "-check_copy_number off" (mipgen.cpp:619) */
    int32_t logistic_heuristic;      /* 0 iff "-logistic_heuristic off" (mipgen.cpp:494) */
    double masked_arm_threshold;     /* -masked_arm_threshold (mipgen.cpp:626) */
    /* enumeration / condense thresholds in force while scanning (mipgen.cpp:264-265):
     * logistic and mixed use the logistic pair, svr the svr pair. */
    double upper_score_limit;
    double lower_score_limit;
    int32_t max_arm_copy_product;    /* -max_arm_copy_product (mipgen.cpp:197) */
    int32_t target_arm_copy;         /* -target_arm_copy (mipgen.cpp:198) */
    /* The reference keys its arm-length lists by sum and keeps a key whose list is EMPTY (-arm_length_sums 30,41,62 with the default minimum arm
     * lengths: 30 < 16 + 18 and 62 > 30 + 30 hold no pair, mipgen.cpp:245-258); the first scan position uses the LARGEST key (:421) and the one list
     * :434 never switches off is that of the SMALLEST key.  0 = the largest / smallest sum of the pairs above (every list non-empty). */
    int32_t arm_sum_key_max;
    int32_t arm_sum_key_min;
    int32_t reserved[4];
} mipgen_params;

/*
 * One merged BED interval +/- flank: the hot-path view of Featurev5 (Featurev5.h:7-28) plus the per-region
 * slices of the global lookup tables design_mip consults (mipgen.cpp:612-618,634-760).
 * All per-base arrays cover [seq_start, seq_stop] (index = position - seq_start), length seq_len.
 */
typedef struct mipgen_region {
    int32_t start_flanked;           /* Featurev5::start_position_flanked */
    int32_t stop_flanked;            /* Featurev5::stop_position_flanked */
    int32_t seq_start;               /* Featurev5::chromosomal_sequence_start_position */
    int32_t seq_stop;                /* Featurev5::chromosomal_sequence_stop_position */
    int32_t seq_len;                 /* strlen(seq); normally seq_stop - seq_start + 1 */
    int32_t reserved0;
    const char* seq;                 /* Featurev5::chromosomal_sequence (upper case) */
    const char* masked_seq;          /* Featurev5::masked_chromosomal_sequence, or NULL = same as seq */
    /* copy_chr_start_stop[chr][start][start+len-1] for oligo length len (mipgen.cpp:612-613):
     * copy[len] points to int32[seq_len] indexed by (start - seq_start); absent keys are 0, as
     * std::map::operator[] yields.  copy[len] may be NULL for lengths no arm pair uses, and the whole
     * pointer table may be NULL = "every oligo has copy 1".  MIPGEN_COPY_RESIDENT = the counts the handle itself
     * produced with mipgen_accel_count_oligo_copies_resident() for exactly this batch (they never left the device). */
    const int32_t* const* copy;      /* table of MIPGEN_MAX_OLIGO+1 pointers, indexed by oligo length */
    /* unmappable_positions[capture_size][chr] (mipgen.cpp:615-618): byte [k * seq_len + (pos - seq_start)] != 0
     * iff a MIP of capture size (max_capture_size - k*capture_increment) starting at pos is ambiguous.
     * NULL = none. */
    const uint8_t* unmappable;
    /* chr_snp_positions[chr] restricted to the region (mipgen.cpp:634-760): per base 0 = no SNP,
     * 1 = SNP for which an alternate-allele arm can be generated, 2 = SNP for which it cannot.  NULL = none. */
    const uint8_t* snp_class;
    double long_range_content[MIPGEN_N_LRC];   /* Featurev5::long_range_content (features 22..65) */
} mipgen_region;

/* Geometry of a region's dense candidate grid, as laid out in the result arrays. */
typedef struct mipgen_grid {
    int64_t offset;                  /* index of the region's first candidate in the batch-wide result arrays */
    int64_t count;                   /* n_pos * n_sizes * n_arm_pairs * 2 */
    int32_t first_pos;               /* first scan-start position p (mipgen.cpp:421-425) */
    int32_t n_pos;                   /* positions p = first_pos .. stop_flanked */
    int32_t first_size_index;        /* k0: capture sizes with k < k0 are removed by the static skip (mipgen.cpp:429) */
    int32_t n_sizes;                 /* surviving sizes C = max_capture - k*inc, k = k0 .. k0+n_sizes-1 */
} mipgen_grid;

/*
 * Dense-grid candidate index within a region (strand-major inside a (position, size) row, so that each strand's scores of a
 * row are contiguous in memory and every result store of the kernels is a full, coalesced segment):
 *     idx = ((((p - first_pos) * n_sizes + (k - k0)) * 2 + strand) * n_arm_pairs + a         strand 0 = '+', 1 = '-'
 * The reference's generation order (p asc, C desc, arm sum desc, ext asc, plus then minus: mipgen.cpp:421-491) is recovered by
 * visiting, for a = 0 .. n_arm_pairs-1, the pair (idx_plus(a), idx_plus(a) + n_arm_pairs); MIPGEN_PLUS_INDEX / MIPGEN_MINUS_INDEX.
 *
 * Integer record per candidate (uint64), the fields design_mip() produces:
 */
#define MIPGEN_PLUS_INDEX(pi, n_sizes, ki, n_pairs, a)  (((((int64_t)(pi) * (n_sizes)) + (ki)) * 2 + 0) * (n_pairs) + (a))
#define MIPGEN_MINUS_INDEX(pi, n_sizes, ki, n_pairs, a) (((((int64_t)(pi) * (n_sizes)) + (ki)) * 2 + 1) * (n_pairs) + (a))
#define MIPGEN_REC_EXT_COPY(r)   ((uint32_t)((r) & 0xFFFFu))            /* ext_probe_copy, saturated at 65535: a field that reads 65535 */
#define MIPGEN_REC_LIG_COPY(r)   ((uint32_t)(((r) >> 16) & 0xFFFFu))    /* lig_probe_copy,  means "look the count up in mipgen_region.copy" */
#define MIPGEN_REC_MASKED_N(r)   ((uint32_t)(((r) >> 32) & 0xFFu))      /* #N in masked ext + masked lig (mipgen.cpp:606-610) */
#define MIPGEN_REC_SNP_COUNT(r)  ((uint32_t)(((r) >> 40) & 0xFFu))      /* snp_count, saturated at 255 */
#define MIPGEN_REC_FLAGS(r)      ((uint32_t)(((r) >> 48) & 0xFFu))
#define MIPGEN_REC_JUNCTION(r)   ((uint32_t)(((r) >> 56) & 0xFFu))      /* 4*code(lj[0])+code(lj[1]), A<C<G<T; 255 if not ACGT */
#define MIPGEN_FLAG_VALID        0x01u   /* passes the bounds skips of mipgen.cpp:443-444 (a candidate the reference could emit) */
#define MIPGEN_FLAG_GUARD        0x02u   /* N in either arm or '-' in mip_seq: score -1000 / all-zero vector (SVMipv4.cpp:63,116) */
#define MIPGEN_FLAG_MAPPING      0x04u   /* mapping_failed == '1' (mipgen.cpp:615-625) */
#define MIPGEN_FLAG_MASKING      0x08u   /* masking_failed == '1' (mipgen.cpp:626-633) */
#define MIPGEN_FLAG_SNP          0x10u   /* snp_failed == '1'     (mipgen.cpp:690-693,753-760) */
#define MIPGEN_FLAG_HAS_SNP_MIP  0x20u   /* has_snp_mip           (mipgen.cpp:685,747) */

/* A single candidate addressed by coordinates, for sparse (mixed-mode) re-scoring and inspection. */
typedef struct mipgen_candidate {
    int32_t region;                  /* index into the resident region batch */
    int32_t scan_start;              /* p */
    int32_t capture_size;            /* C */
    int32_t ext_len;
    int32_t lig_len;
    int32_t strand;                  /* 0 '+', 1 '-' */
} mipgen_candidate;

/* Integer features of one candidate as the two scorers see them (strand-oriented sequences). */
typedef struct mipgen_candidate_ints {
    int32_t ext_a, ext_c, ext_g, ext_t;        /* base counts of the extension arm */
    int32_t lig_a, lig_c, lig_g, lig_t;
    int32_t ins_a, ins_c, ins_g, ins_t;        /* base counts of the insert (scan target) */
    int32_t run_count;                         /* GC/AT run counter incl. the final ++ (SVMipv4.cpp:118-142) */
    int32_t junction;                          /* as MIPGEN_REC_JUNCTION */
    int32_t ext_copy, lig_copy;                /* unsaturated */
    int32_t masked_n;
    int32_t snp_count;
    int32_t flags;
    int32_t scan_size;
} mipgen_candidate_ints;

/* Per (scan-start, strand) survivor of the reference's replay + condense_mips fold (mipgen.cpp:1670-1746). */
typedef struct mipgen_survivor {
    int64_t cand_index;              /* dense-grid index within the batch (mipgen_grid.offset + index in the region), or -1 if none survived */
    double score;
    uint64_t record;
} mipgen_survivor;

typedef struct mipgen_accel mipgen_accel;   /* opaque */

/* ---- lifecycle ------------------------------------------------------------------------------------ */
int mipgen_accel_abi_version(void);
const char* mipgen_accel_last_error(void);
/* number of usable HIP devices (0 if none); never fails */
int mipgen_accel_device_count(void);
/* device: HIP ordinal.  stream: a hipStream_t the caller owns (e.g. torch's current stream) or NULL for a private one. */
int mipgen_accel_create(const mipgen_params* params, int device, void* stream, mipgen_accel** out);
void mipgen_accel_destroy(mipgen_accel* h);

/* ---- model (svm.h:78 svm_load_model) -------------------------------------------------------------- */
/* Parses a libsvm 3.17 text model (grammar svm.cpp:2779-2962).  Only epsilon_svr/nu_svr + rbf are accepted;
 * anything else, or a missing file, is MIPGEN_E_MODEL (the reference dereferences NULL instead, svm.cpp:2507). */
int mipgen_accel_load_model_file(mipgen_accel* h, const char* path);
/* Same from memory: sv is row-major [n_sv][192] (absent libsvm indices = 0), coef[n_sv]. */
int mipgen_accel_set_model(mipgen_accel* h, int32_t n_sv, double gamma, double rho, const double* coef, const double* sv);
int mipgen_accel_model_info(const mipgen_accel* h, int32_t* n_sv, double* gamma, double* rho);

/* ---- region batch: host -> HBM -------------------------------------------------------------------- */
/* Copies the batch into device memory (sequence bytes, masked bytes, copy tables, SNP / mappability maps,
 * long-range content) and lays out the dense grids.  grids_out (n entries, caller-allocated) may be NULL.
 * Replaces any previously resident batch.
 *
 * Result windows.  The inputs of EVERY region of the batch stay resident (they are small: ~16-70 bytes per base of region).
 * The dense results (8 B score + 8 B record + 1 B emitted flag per candidate) are what fills HBM, so the batch is cut into
 * windows of consecutive regions whose dense results fit the result arrays; windows are scored one after the other into the
 * same arrays.  A batch that fits is one window (the usual case: 288 GB hold ~1.4e10 candidates).  mipgen_grid.offset stays
 * batch-wide; a region is never split. */
int mipgen_accel_upload_regions(mipgen_accel* h, const mipgen_region* regions, int32_t n, mipgen_grid* grids_out);
/* total dense-grid candidates of the resident batch */
int64_t mipgen_accel_batch_candidates(const mipgen_accel* h);
/* upper bound on the candidates of one result window for the following uploads (0 = automatic: what fits in free device memory, at most
 * 2^30 candidates unless a single region is larger) */
int mipgen_accel_set_window_candidates(mipgen_accel* h, int64_t max_candidates);
/* regions of the following uploads at which a new result window must start whatever the candidate bound says (ascending batch indices; n = 0
 * clears them): a front end that deals consecutive region blocks of one design to several devices in turn (the selection stage consumes the
 * blocks in design order, /root/reference/mipgen.cpp:503-515) uploads its blocks as ONE batch and never gets a window that spans two of them */
int mipgen_accel_set_window_breaks(mipgen_accel* h, const int32_t* first_regions, int32_t n);
int32_t mipgen_accel_window_count(const mipgen_accel* h);
/* regions [first_region, +n_regions), candidates [first_candidate, +n_candidates) and scan positions of window w; any output may be NULL */
int mipgen_accel_window_info(const mipgen_accel* h, int32_t w, int32_t* first_region, int32_t* n_regions, int64_t* first_candidate,
                             int64_t* n_candidates, int64_t* first_position, int64_t* n_positions);

/* ---- the hot path --------------------------------------------------------------------------------- */
/* Scores the resident batch's dense grid with `method` (MIPGEN_SCORE_LOGISTIC or MIPGEN_SCORE_SVR) into
 * library-owned device arrays (double scores[], uint64 records[], both batch_candidates long).
 * Asynchronous on the handle's stream.
 * Every parameter set the reference accepts is scored (mipgen.cpp:222-261, 427-444: any -arm_lengths / -capture_increment / range): SVR
 * requests outside the tiled kernel's limits (scan sizes below 3, more than 240 arm pairs, a tile beyond 160 KiB of LDS) take the
 * list scorer over the window's dense index range - same results, a lower rate (any scan size: the list kernels pass an insert through LDS in
 * pieces of 1,024 bases). */
int mipgen_accel_score_resident(mipgen_accel* h, int32_t method);       /* single-window batches; else MIPGEN_E_STATE */
/* the same for result window w of a larger batch; the window's results replace the previous window's */
int mipgen_accel_score_window(mipgen_accel* h, int32_t w, int32_t method);
/* device pointers of the result arrays (element 0 = first candidate of the window scored last; valid until the next upload) */
int mipgen_accel_result_device_ptrs(const mipgen_accel* h, void** scores_dev, void** records_dev);
/* blocks until the stream is idle, then copies results to host arrays (either may be NULL); [first, first+count) are batch-wide
 * candidate indices and must lie inside the window scored last */
int mipgen_accel_download_results(mipgen_accel* h, double* scores, uint64_t* records, int64_t first, int64_t count);
/* The whole batch the way a -silent_mode design needs it (mipgen.cpp:412-524 without the all_mips / collapsed files): every window is
 * scored, replayed, condensed and collapsed back to back on the stream; only the survivors (2 per scan position), the per-base
 * collapse result and the per-region emitted counts are kept.  Asynchronous; fetch with mipgen_accel_download_survivors /
 * mipgen_accel_download_collapsed. */
int mipgen_accel_score_condense_all(mipgen_accel* h, int32_t method);
/* ONE window that way (ABI 6): scored, replayed and condensed; what mipgen_accel_score_window + mipgen_accel_replay_condense leave for a caller that will
 * never read the window's dense results (a -silent_mode front end that downloads window w while window w + 1 is scored): the print-exact re-score of
 * mipgen_accel_set_print_exact then tests the 2 survivors per scan position - the only scores such a design prints, mipgen.cpp:1917 - instead of every
 * dense candidate.  Follow with mipgen_accel_collapse / mipgen_accel_download_replay / mipgen_accel_download_collapsed as after mipgen_accel_replay_condense. */
int mipgen_accel_score_condense_window(mipgen_accel* h, int32_t w, int32_t method);
/* upload + score + download in one call: the literal replacement for the loop body of mipgen.cpp:446-497 */
int mipgen_accel_score_regions(mipgen_accel* h, const mipgen_region* regions, int32_t n, int32_t method,
                               mipgen_grid* grids_out, double* scores, uint64_t* records, int64_t capacity);

/* Sparse list against the resident batch (mixed-mode re-scores, mipgen.cpp:1525-1526,1875-1876; inspection).
 * Any output pointer may be NULL.  features: [n][192] as SVMipv4::get_parameters fills it. */
int mipgen_accel_score_candidates(mipgen_accel* h, const mipgen_candidate* cands, int32_t n, int32_t method,
                                  double* scores, uint64_t* records, double* features, mipgen_candidate_ints* ints);

/* Probes given by their SEQUENCES instead of coordinates in a resident batch (new entry point only: the ABI number does not change): what a MIP table
 * (all_mips / collapsed_mips / picked_mips / snp_mips, print_details mipgen.cpp:765-794) holds of a probe is everything the two scorers read, so a
 * design that exists only as such a file - this front end's, the reference's, one years old - can be featurized (training rows for
 * mipgen_accel_train_svr) and scored with the model in hand.
 *   - the sequences are STRAND-ORIENTED, as the reference's objects hold them and its files print them; nothing is reverse-complemented here.
 *   - bytes are compared as the reference compares characters (std::string::find of "A", "AC", ..., SVMipv4.cpp:31-57; find("N") / find("-"), :63, :116;
 *     current_base == "G", :123-134): only upper-case A C G T count in a mer, only 'N' in an arm and '-' in mip_seq raise the guard; a lower-case
 *     letter or any other byte is in no mer, is no guard base and is "neither G/C nor A/T" in the run walk of get_score.
 *   - guard (N in an arm, '-' anywhere in mip_seq): the all-zero feature vector; logistic score -1000, SVR the model's value at that vector.
 *   - any insert length (the device stages an insert in pieces); arms of 1..MIPGEN_MAX_OLIGO bases.
 *   - scores: MIPGEN_SCORE_LOGISTIC in the reference's term order with the correctly rounded power; MIPGEN_SCORE_SVR through the matrix-core list
 *     scorer for n >= 256 and the per-probe model walk below - the scorers and the choice of mipgen_accel_score_candidates.
 *   - ints: base counts, run_count, junction, copies, scan_size and flags (MIPGEN_FLAG_VALID, MIPGEN_FLAG_GUARD); masked_n and snp_count are 0 - the
 *     tables they come from are not part of a probe.
 * Any output pointer may be NULL.  A NULL sequence, an empty arm, an lrc_index outside [-1, n_lrc) are MIPGEN_E_INVALID, SVR without a model
 * MIPGEN_E_MODEL, all before anything is allocated.  No resident batch is needed, and the handle's batch, result windows and result arrays are
 * exactly as they were when the call returns. */
typedef struct mipgen_probe {
    const char* ext_seq; const char* lig_seq; const char* ins_seq;   /* oriented, NUL-terminated, upper or lower case as the files hold them */
    const char* mip_seq;             /* may be NULL: then the '-' guard looks at the two arms only */
    int32_t ext_copy, lig_copy;      /* unsaturated */
    int32_t lrc_index;               /* row of the long-range table, or -1 = 44 zeros */
    int32_t reserved;
} mipgen_probe;
int mipgen_accel_score_probes(mipgen_accel* h, const mipgen_probe* probes, int32_t n,
                              const double* lrc, int32_t n_lrc,   /* [n_lrc][44], e.g. from mipgen_accel_long_range_content_batch */
                              int32_t method, double* scores, double* features, mipgen_candidate_ints* ints);

/* ---- measured counts: reads and unique molecular tags per probe from smMIP read pairs (new entry points only: the ABI number does not change) ----
 * The capture model: with E = ext_seq, L = lig_seq as a MIP table prints them and tag sizes (ext_tag, lig_tag), the extension read of a
 * captured molecule is tag + E + target ..., the ligation read is tag + revcomp(L) + ....  A pair is a CANDIDATE of a probe if the S bases behind
 * the tag of its extension read are the first S bases of E, or those of its ligation read the first S of revcomp(L), exactly (S = the shortest arm
 * of the table, at most 32); it PASSES if all of E and all of revcomp(L) match with at most max_mismatches substitutions each (any byte of a read
 * or an arm that is not upper-case A C G T is a mismatch; a read shorter than tag + arm fails).  The pair goes to the passing probe with the
 * fewest mismatches in total; an exact tie for fewest is ambiguous (no probe; two rows with the same arms always tie), no passing probe is
 * unassigned.  reads[p] = pairs assigned to probe p; unique_tags[p] = distinct tags among them, a tag being the ext_tag + lig_tag bases packed at 2
 * bits each; a tag holding a byte that is not A C G T adds to reads, joins no group and is counted in tag_n.  With no tag bases unique_tags = reads.
 * A pair whose two seed ranges hold more than 1,024 probes together is counted in overflow and assigned to nothing.
 *   open:   packs the arms and builds the seed tables (ins_seq, mip_seq and the other members of mipgen_probe are not read).  MIPGEN_E_INVALID: NULL
 *           pointers, n < 1, an empty arm or one beyond MIPGEN_MAX_OLIGO, a shortest arm below 12 bases, negative tag sizes or ext_tag + lig_tag > 16,
 *           max_mismatches outside 0..2; MIPGEN_E_STATE: a session is open; MIPGEN_E_NOMEM: the tables and buffers against free device memory.
 *           Every check comes before any allocation.
 *   feed:   n_pairs read pairs, any number of times: the bytes of read i of a file are bytes[offsets[i] - offsets[0] ... offsets[i + 1] - offsets[0])
 *           (offsets: n_pairs + 1 ascending entries, so a slice of a larger offset array can be passed with the bytes it starts at).  The call
 *           returns when the device is done with the arrays.  MIPGEN_E_STATE without an open session.
 *   finish: reads and unique_tags (n entries each, either may be NULL), the totals (may be NULL), and the session is closed whichever way the call
 *           ends.  The result does not depend on how the pairs were cut into feed calls.
 * The handle's resident batch, result windows, result arrays and model are exactly as they were after each of the calls; mipgen_accel_destroy
 * releases an open session. */
typedef struct mipgen_read_totals { int64_t pairs, assigned, ambiguous, unassigned, tag_n, overflow; } mipgen_read_totals;
int mipgen_accel_reads_open(mipgen_accel* h, const mipgen_probe* probes, int32_t n, int32_t ext_tag, int32_t lig_tag, int32_t max_mismatches);
int mipgen_accel_reads_feed(mipgen_accel* h, int64_t n_pairs, const char* ext_bytes, const int64_t* ext_offsets, const char* lig_bytes, const int64_t* lig_offsets);
int mipgen_accel_reads_finish(mipgen_accel* h, int64_t* reads, int64_t* unique_tags, mipgen_read_totals* totals);
/* Capacity, in keys, of the (probe, tag) key buffer of the sessions opened after the call (0: the default, 2^26 or what free memory allows).  The
 * buffer is sorted and made duplicate-free whenever it fills and grows only when more than half of it is distinct keys: a small value makes that
 * happen often (tests); the counts do not depend on it. */
int mipgen_accel_reads_set_key_buffer(mipgen_accel* h, int64_t n_keys);
/* The probe index of every pair of the LAST feed call (capacity >= its n_pairs): >= 0 assigned, -1 unassigned, -2 ambiguous, -3 overflow. */
int mipgen_accel_reads_last_assignment(mipgen_accel* h, int32_t* probe_index, int64_t capacity);

/* ---- the same per SAMPLE of a multiplexed lane (new entry points only: the ABI number does not change) ----
 * The sample model: n_samples >= 1 barcodes of one length J (1..32), upper-case A C G T only, pairwise distinct.  The index of a pair is
 * the first J bytes of its index read (bytes beyond J are ignored; a shorter read has no sample).  Distance is the Hamming distance over the J
 * positions, a byte that is not upper-case A C G T being a mismatch; the sample of a pair is the barcode at the smallest distance <=
 * barcode_mismatches (0 or 1); two barcodes at that smallest distance: ambiguous; none within it: none.  Row s of the outputs is sample s, row n_samples
 * is `undetermined` (none + ambiguous).  The probe of a pair and the six totals are what a plain session gives, whatever the sample.
 * reads[row * n + p]: pairs of that row assigned to probe p; unique_tags[row * n + p]: distinct clean tags among them (the same tag in two samples
 * is two molecules; = reads with no tag bases); row_pairs[row]: all pairs of the row, assigned to a probe or not.
 *   open_samples:   everything mipgen_accel_reads_open refuses, and MIPGEN_E_INVALID for NULL / no barcodes, barcodes of unequal length or of more than
 *                   32 bases, a byte that is not A C G T, a barcode twice, barcode_mismatches outside 0..1, (n_samples + 1) * n > 2^32.  The count matrices
 *                   (2 x 8 bytes per cell) and the barcode table are part of the MIPGEN_E_NOMEM budget.
 *   feed_samples:   as feed, with the index read of every pair (its offsets checked like the others).
 *   finish_samples: reads and unique_tags hold (n_samples + 1) * n entries each, row-major; row_pairs n_samples + 1; every output may be NULL.
 *   last_samples:   the sample index of every pair of the LAST feed_samples call: >= 0, -1 none, -2 ambiguous (last_assignment gives the probes).
 * feed / finish of one kind on a session of the other kind: MIPGEN_E_STATE, the session is left as it was and a later correct call works. */
typedef struct mipgen_sample_totals { int64_t sample_none, sample_ambiguous; } mipgen_sample_totals;
int mipgen_accel_reads_open_samples(mipgen_accel* h, const mipgen_probe* probes, int32_t n, int32_t ext_tag, int32_t lig_tag, int32_t max_mismatches,
                                    const char* const* barcodes, int32_t n_samples, int32_t barcode_mismatches);
int mipgen_accel_reads_feed_samples(mipgen_accel* h, int64_t n_pairs, const char* ext_bytes, const int64_t* ext_offsets, const char* lig_bytes, const int64_t* lig_offsets,
                                    const char* index_bytes, const int64_t* index_offsets);
int mipgen_accel_reads_finish_samples(mipgen_accel* h, int64_t* reads, int64_t* unique_tags, mipgen_read_totals* totals, mipgen_sample_totals* sample_totals,
                                      int64_t* row_pairs);
int mipgen_accel_reads_last_samples(mipgen_accel* h, int32_t* sample_index, int64_t capacity);

/* ---- one consensus read per molecule (new entry points only: the ABI number does not change) ----
 * The consensus model.  Probe, sample and tag rules are exactly those above: reads, unique_tags, the totals, row_pairs and the per-pair
 * probe / sample indices of a consensus session EQUAL those of a plain or samples session on the same pairs.  A GROUP is all assigned pairs with a
 * clean tag that share (row, probe, tag), row = 0 without barcodes; its FAMILY is their number.  The extension reads and the ligation reads of a group
 * are collapsed separately, each behind its tag (the arms stay); the consensus of a side is as long as the shortest member of that side behind the tag.
 * Per position, with q = clamp(quality byte - 33, 0, 93) and S[b] the sum of q over the members showing base b (a byte that is not upper-case A C G T
 * casts no vote): the base is the b with the strictly largest S[b], or N when the largest is shared or every S is 0; v = S[best] - the sum of the other
 * three, v = - the sum of all for N; the quality byte is 'I' for v > 40, '#' for v < 2, else v + 33.  Sums are exact (no overflow for any family).
 * Groups come in ascending (row, probe, tag code) order - independent of feed order and of how the pairs were cut into feed calls.
 *   open_consensus:   barcodes = NULL with n_samples = 0: one row; otherwise as open_samples.  arena_bytes: the device memory the session may use for
 *                     retained reads (per feed call: twice its read bytes + 44 bytes per pair + at most 48 of alignment); 0 = half of the device memory that is
 *                     free at open beside the tables.  Everything open / open_samples refuses, and MIPGEN_E_INVALID for ext_tag + lig_tag = 0, a negative
 *                     arena_bytes, barcodes and n_samples that disagree, more than 2^31 cells.  Every check comes before any allocation.
 *   feed_consensus:   as feed / feed_samples, with the quality bytes of both reads (they share the offsets of their bases); index_bytes / index_offsets
 *                     are NULL for a session without barcodes.  The chunk stays on the device.  MIPGEN_E_NOMEM when the chunk does not fit what is left
 *                     of the arena (or the device): the session is exactly as it was before the call, and finish_consensus works on what was fed.
 *                     MIPGEN_E_INVALID beyond 2^31 - 1 pairs in a session.  last_assignment / last_samples work as in the other kinds.
 *   finish_consensus: the outputs of finish_samples (sample_totals and row_pairs are left alone without barcodes) and sizes: groups and the bytes of
 *                     all extension / ligation consensus reads; every output may be NULL.  sizes.n_groups is the sum of unique_tags.  The session is
 *                     closed whichever way the call ends; the consensus reads stay on the handle until the next mipgen_accel_reads_open* call or
 *                     mipgen_accel_destroy.
 *   consensus_fetch:  per group cell (row * n + probe), tag (2 bits a base, the first tag base highest) and family; ext_off / lig_off: n_groups + 1
 *                     offsets into the sequence and quality bytes of a side (ext_seq, ext_qual: sizes.ext_bytes each; no terminators).  Every pointer may
 *                     be NULL.  MIPGEN_E_STATE when the handle holds no consensus reads (before a finish_consensus, after the next open).
 * Feed, finish or last_samples of one kind on a session of another: MIPGEN_E_STATE, the session is left as it was and a later correct call works. */
typedef struct mipgen_consensus_sizes { int64_t n_groups, ext_bytes, lig_bytes; } mipgen_consensus_sizes;
int mipgen_accel_reads_open_consensus(mipgen_accel* h, const mipgen_probe* probes, int32_t n, int32_t ext_tag, int32_t lig_tag, int32_t max_mismatches,
                                      const char* const* barcodes, int32_t n_samples, int32_t barcode_mismatches, int64_t arena_bytes);
int mipgen_accel_reads_feed_consensus(mipgen_accel* h, int64_t n_pairs, const char* ext_bytes, const char* ext_qual, const int64_t* ext_offsets, const char* lig_bytes,
                                      const char* lig_qual, const int64_t* lig_offsets, const char* index_bytes, const int64_t* index_offsets);
int mipgen_accel_reads_finish_consensus(mipgen_accel* h, int64_t* reads, int64_t* unique_tags, mipgen_read_totals* totals, mipgen_sample_totals* sample_totals,
                                        int64_t* row_pairs, mipgen_consensus_sizes* sizes);
int mipgen_accel_reads_consensus_fetch(mipgen_accel* h, int32_t* cell, uint32_t* tag, int32_t* family, int64_t* ext_off, char* ext_seq, char* ext_qual, int64_t* lig_off,
                                       char* lig_seq, char* lig_qual);

/* ---- sequencing errors in molecular tags, corrected before the consensus (new entry points only: the ABI number does not change) ----
 * The tag merge model.  A RAW group is a group of the model above; its count c is its family size.  A NEIGHBOUR of a raw group is another raw group of the SAME cell
 * whose tag code differs in exactly one base (one 2-bit field).  Neighbour a is an ELIGIBLE PARENT of b when c_a >= 2 c_b - 1 and c_a > c_b; the PARENT of b is its
 * eligible parent of the largest count, of the smaller tag code among equals; a group without one is a root.  A CORRECTED group is a root with all its descendants:
 * its tag is the root's, its family the sum of the raw families, its consensus the vote of the model above over all those members.  reads, the totals, row_pairs and
 * the per-pair indices are unchanged; unique_tags counts corrected groups.  Dirty tags join nothing, and tags of different cells never meet.
 *   set_tag_mismatches: d = 0 (the default of every open: tags are compared exactly, and the session allocates and launches what it always did) or 1 (the merge
 *                       above at finish_consensus); valid on an open consensus session at any time before its finish.  MIPGEN_E_STATE with no session open or
 *                       with a session that keeps no reads (it stays usable); MIPGEN_E_INVALID for any other d.
 *   last_tag_merge:     the totals of the last finish_consensus: raw_groups, groups (corrected), absorbed = raw_groups - groups, moved_pairs (the pairs of the
 *                       absorbed groups) and max_depth (the parent links of the longest chain).  At d = 0: raw_groups = groups, the rest 0.
 *   tag_map_fetch:      one entry per RAW group in raw group order (ascending cell, raw tag code): cell, raw tag, raw family and the tag of the corrected group
 *                       it went to (at d = 0: the identity map).  Every pointer may be NULL.
 * last_tag_merge and tag_map_fetch: MIPGEN_E_STATE when the handle holds no consensus reads (before a finish_consensus, after the next open).  A parent walk that
 * does not end within 31 links - a state the rule cannot build - fails the finish with MIPGEN_E_STATE. */
typedef struct mipgen_tag_merge_totals { int64_t raw_groups, groups, absorbed, moved_pairs, max_depth; } mipgen_tag_merge_totals;
int mipgen_accel_reads_set_tag_mismatches(mipgen_accel* h, int32_t d);
int mipgen_accel_reads_last_tag_merge(mipgen_accel* h, mipgen_tag_merge_totals* totals);
int mipgen_accel_reads_tag_map_fetch(mipgen_accel* h, int32_t* cell, uint32_t* raw_tag, int32_t* raw_family, uint32_t* tag);

/* ---- allele counts per captured base from the consensus reads (new entry point only: the ABI number does not change) ----
 * The pileup model.  The call reads the consensus reads the handle holds since the last finish_consensus and nothing else.  Probe p has a molecule
 * length mol_len[p] >= 1: the bytes of M = ext arm + scan target + lig arm.  Every read of a probe starts at the same template base, so position t of the extension
 * consensus of any molecule (group) of p is base t of M, and position j of its ligation consensus is the complement of base mol_len[p] - 1 - j; consensus positions
 * at or beyond mol_len[p] (a read that ran through into the backbone) are ignored.  An observation is usable if its base is one of A C G T (the ligation base after
 * A<->T, C<->G) and its quality byte - 33 is >= min_quality (the consensus writes 2..40).  One vote per molecule and position: no usable observation counts nothing,
 * one counts its base, two of the same base count it once, two of different bases count `discordant` and no base.  Groups of fewer than min_family pairs are
 * skipped.  counts[pos_off[p] + t][5] (int32: A, C, G, T, discordant; the bases in the orientation of M; pos_off = the exclusive sum of mol_len) for the groups
 * of ONE row (the sample row; 0 without barcodes; the last row is `undetermined`); sum(mol_len) * 5 entries, may be NULL.  totals (may be NULL): groups = the groups
 * of the row, used = those of at least min_family pairs, bases = the sum of columns A..T, discordant = the sum of the fifth.
 * MIPGEN_E_STATE: the handle holds no consensus reads.  MIPGEN_E_INVALID: NULL mol_len, n different from the session's, a mol_len < 1, row outside [0, rows),
 * min_family < 1, min_quality outside 0..40, more than 2^31 - 1 rounds of 64 positions.  MIPGEN_E_NOMEM: the count buffer (20 bytes per position) and the
 * temporaries against free device memory.  Every check comes before any allocation or launch.  The consensus reads, the resident batch, its windows and results
 * and the model are left as they were; the call may be repeated, for any row in any order.  A handle with zero groups gives zeros. */
typedef struct mipgen_pileup_totals { int64_t groups, used, bases, discordant; } mipgen_pileup_totals;
int mipgen_accel_reads_consensus_pileup(mipgen_accel* h, const int32_t* mol_len, int32_t n, int32_t row, int32_t min_family, int32_t min_quality, int32_t* counts,
                                        mipgen_pileup_totals* totals);

/* ---- the pileup with indels (new entry point only: the ABI number does not change) ----
 * The gapped pileup model.  As the call above, but every consensus read is first PLACED on its template by a banded alignment anchored at its arm,
 * so that the bases behind an insertion or deletion are counted against the template position they came from.  mol_seq: the template bases of every probe, M_p
 * upper-cased, mol_len[p] bytes each, concatenated in probe order (sum(mol_len) bytes; any byte other than A C G T matches nothing).  Per side: the extension
 * consensus against M, the ligation consensus against revcomp(M); score +1 / -1 / 0 (either byte not A C G T), linear gap -2, cells |i - j| <= max_indel, start
 * fixed at (0, 0), end free on the last row of the read or the last column of the template (largest score, then smallest |j - i|, then larger j); traceback
 * preferring diagonal, deletion, insertion on the extension side and deletion, insertion, diagonal on the ligation side.  Quality plays no part in the placement.
 * A diagonal step observes its read base at its template position, a deletion step observes `del` (always usable); per molecule and position the two sides vote as
 * above with `del` as a fifth class.  Insertions are recorded at the anchor t (between t and t + 1, orientation of M) by length only: a side covers t if its path
 * consumes t and t + 1; one covering side counts `ins` if its length is > 0, two with equal length > 0 count it once, two with different lengths count
 * `ins_discordant`.  counts[pos_off[p] + t][8] (int32: A, C, G, T, discordant, del, ins, ins_discordant), sum(mol_len) * 8 entries, may be NULL.  totals (may be
 * NULL): groups, used as above; bases, discordant, deletions, insertions, ins_discordant = the column sums; gapped_sides = the sides of used groups whose path holds
 * at least one gap step.
 * MIPGEN_E_STATE: the handle holds no consensus reads.  MIPGEN_E_INVALID: every case of the call above, NULL mol_seq, max_indel outside 1..15, a mol_len above
 * MIPGEN_GAPPED_MAX_MOL.  MIPGEN_E_NOMEM: the count buffer (32 bytes per position), the projections (at most 3 mol_len bytes per side of the session) and the
 * temporaries against free device memory.  Every check comes before any allocation or launch.  mipgen_accel_reads_consensus_pileup and everything else on the
 * handle are untouched by the call; it may be repeated, for any row in any order.  A handle with zero groups gives zeros. */
#define MIPGEN_GAPPED_MAX_MOL 2048
typedef struct mipgen_gapped_totals { int64_t groups, used, bases, discordant, deletions, insertions, ins_discordant, gapped_sides; } mipgen_gapped_totals;
int mipgen_accel_reads_consensus_pileup_gapped(mipgen_accel* h, const char* mol_seq, const int32_t* mol_len, int32_t n, int32_t row, int32_t min_family, int32_t min_quality,
                                               int32_t max_indel, int32_t* counts, mipgen_gapped_totals* totals);

/* ---- variant calls from the pileup against a background of the other samples (new entry points only: the ABI number does not change) ----
 * The model.  Allele classes: A, C, G, T (0..3) and, in the gapped table, del (4).  At position x with ref = upper(template byte) one of A C G T,
 * an alt allele a is any class but ref (insertions are not called); depth n = A + C + G + T (+ del), alt count k = counts[x][a].  The POOL holds per (x, a) the sums
 * K, N of k', n' over the sample rows that qualify there (n' > 0 and k' 10^6 <= bg_max_ppm n'); sample rows are all rows of the session but the last
 * (undetermined) when it has barcodes, the one row otherwise.  For the row being called K_o = K - k, N_o = N - n when it is itself a qualifying sample row, else K, N.
 * Error rate e = (K_o + a0) / (N_o + n0).  A cell is a CANDIDATE iff min_depth <= n <= MIPGEN_CALL_MAX_DEPTH, k >= min_alt, k 10^6 >= min_ppm n and
 * k (N_o + n0) > n (K_o + a0); its score is Q = min(9999, floor(-10 log10 P)), P the binomial tail sum_{i >= k} C(n,i) e^i (1-e)^(n-i); it is a CALL iff Q >= min_q.
 * Records come in ascending (pos, allele); two calls on the same input return the same bytes.  totals: tested = positions with a usable ref and
 * min_depth <= n <= the cap; too_deep = those above the cap (not tested); candidates; calls.
 *   call_tables:          from host arrays, no read session needed: counts[n_pos][columns] (columns 5: the pileup's table, 8: the gapped one), pool[n_pos][10] int32
 *                         (K[5] then N[5] per position), ref[n_pos] bytes; own_row_is_sample != 0: the row is part of the pool (leave-one-out applies).
 *   consensus_call_pool:  the pileup of every sample row of the session (max_indel 0: mipgen_accel_reads_consensus_pileup's table; 1..15: the gapped one) into a
 *                         scratch of its own, pooled on the device.  The pool stays with the consensus reads and remembers these arguments.  mol_seq is required
 *                         (it supplies the ref bytes; for max_indel > 0 it is the gapped call's mol_seq, upper case).
 *   consensus_call:       recomputes the pileup of `row` (any row, undetermined included) with the pool's arguments - counts (may be NULL) is what the matching
 *                         pileup call returns - then flags, scores and orders its calls.
 *   call_fetch:           the records of the last call of either kind; n must equal its totals.calls.
 *   call_pileup_totals:   the pileup totals of the row consensus_call counted last.
 * MIPGEN_E_INVALID: every refusal of the underlying pileup call; NULL counts / pool / ref / params; columns not 5 or 8; n_pos outside 1..2^29 - 1; max_indel
 * outside 0..15; min_depth < 1; min_alt < 1; min_ppm or bg_max_ppm outside 0..10^6; min_q outside 0..9999; a prior outside 0 < a0 < n0 <= 2^30; fetch with n
 * different from the last totals.calls.  MIPGEN_E_STATE: no consensus reads; consensus_call without a pool, or with params.bg_max_ppm different from the pool's;
 * fetch before any call.  MIPGEN_E_NOMEM: the pool (40 bytes per position), the counts, the ref bytes and the candidate list at its worst case (4 per position)
 * against free device memory.  Every check comes before any allocation or launch. */
#define MIPGEN_CALL_MAX_DEPTH (1 << 20)
typedef struct mipgen_call_params { int32_t min_depth, min_alt, min_ppm, min_q, a0, n0, bg_max_ppm; } mipgen_call_params;
typedef struct mipgen_call_record { int64_t pos; int32_t allele, depth, alt, bg_alt, bg_depth, q; } mipgen_call_record;
typedef struct mipgen_call_totals { int64_t tested, too_deep, candidates, calls; } mipgen_call_totals;
int mipgen_accel_call_tables(mipgen_accel* h, const int32_t* counts, int32_t columns, const int32_t* pool, const uint8_t* ref, int64_t n_pos, int32_t own_row_is_sample,
                             const mipgen_call_params* params, mipgen_call_totals* totals);
int mipgen_accel_reads_consensus_call_pool(mipgen_accel* h, const char* mol_seq, const int32_t* mol_len, int32_t n, int32_t min_family, int32_t min_quality,
                                           int32_t max_indel, int32_t bg_max_ppm);
int mipgen_accel_reads_consensus_call(mipgen_accel* h, int32_t row, const mipgen_call_params* params, int32_t* counts, mipgen_call_totals* totals);
int mipgen_accel_call_fetch(mipgen_accel* h, mipgen_call_record* records, int64_t n);
/* The totals the matching pileup call would have returned for the row of the last mipgen_accel_reads_consensus_call (the ungapped table fills groups, used, bases,
 * discordant and leaves the rest 0): a caller that writes the pileup from that call's counts needs no second count.  MIPGEN_E_STATE before such a call. */
int mipgen_accel_reads_consensus_call_pileup_totals(mipgen_accel* h, mipgen_gapped_totals* totals);

/* ---- pileup and calls per genome locus, merged over the probes that cover it (new entry points only: the ABI number does not change) ----
 * A LOCUS is one genome base; a session has n_pos template positions x (the rows of the pileup tables) and n_loci loci, both 1..2^29 - 1.  The PLAN holds one int64
 * per template position: -1 - the position contributes to no locus - or locus * 4 + flags with 0 <= locus < n_loci; flag bit 0: the probe is on the minus strand;
 * flag bit 1: the insertion columns of this source are those of row x - 1 (it needs x >= 1).  The library does not know what an arm is: the caller decides what is
 * left out.  The MERGED row of a locus is the sum over its sources, in the column layout of the source table: a plus source adds its row as it is, a minus source
 * adds A <-> T and C <-> G swapped (columns 0 <-> 3, 1 <-> 2), discordant and del as they are; the insertion columns (6, 7) are the source's own on a plus source and
 * 0 on a minus one, and those of row x - 1 under bit 1 on either strand.  A locus without a source has a zero row.  totals: covered = loci with a non-zero counter,
 * bases = the sum of A + C + G + T, then the column sums (the last three stay 0 with 5 columns).  A merged counter is a 32-bit sum: the sources of one locus must
 * add up to fewer than 2^31 per column (they do whenever a locus takes at most one position per probe: a counter is then at most the groups of the session).
 * Calls are the calls above with x := locus on the merged tables against locus_ref, the upper-case plus-strand base of every locus; mipgen_call_record.pos is the
 * locus index; records are fetched with mipgen_accel_call_fetch.
 *   locus_tables:      from host arrays, no read session needed: counts[n_pos][columns] -> merged[n_loci][columns] (may be NULL), which mipgen_accel_call_tables takes.
 *   locus_plan:        installs plan and locus_ref for the consensus reads the handle holds; a second plan replaces the first and drops a locus pool
 *                      (a plan refused with MIPGEN_E_INVALID or for its budget leaves the first and its pool as they were).
 *   locus_pileup:      the pileup of `row` (max_indel 0: the 5-column table, mol_seq may be NULL; 1..15: the gapped one) counted into scratch of its own, then merged:
 *                      probe_counts (may be NULL) is what the matching pileup call returns, locus_counts (may be NULL) n_loci x columns; pileup_totals as the gapped
 *                      pileup's (the ungapped table fills groups, used, bases, discordant).
 *   locus_call_pool:   consensus_call_pool with the merge between every row's count and the pool, over n_loci.
 *   locus_call:        consensus_call likewise: probe_counts and locus_counts (either may be NULL) are those of locus_pileup with the pool's arguments.
 * MIPGEN_E_INVALID: every refusal of the underlying pileup or call; NULL plan or ref; n_loci or n_pos outside 1..2^29 - 1; a plan entry below -1, or whose locus is
 * >= n_loci; bit 1 at x = 0; a sum of mol_len different from the plan's n_pos; columns not 5 or 8.  MIPGEN_E_STATE: no consensus reads; no plan; locus_call without a
 * locus pool or with params.bg_max_ppm different from the pool's.  MIPGEN_E_NOMEM: the plan (24 bytes per position, the sort's scratch and sorted pairs, 4 bytes per
 * locus), the merged table, the pool and the candidate list over n_loci do not fit free memory; refused before anything is allocated.  The existing pileup and call
 * entry points, their scratch and timing indices 11-13 are untouched by these calls. */
typedef struct mipgen_locus_totals { int64_t covered, bases, discordant, deletions, insertions, ins_discordant; } mipgen_locus_totals;
int mipgen_accel_locus_tables(mipgen_accel* h, const int32_t* counts, int32_t columns, const int64_t* plan, int64_t n_pos, int64_t n_loci, int32_t* merged,
                              mipgen_locus_totals* totals);
int mipgen_accel_reads_consensus_locus_plan(mipgen_accel* h, const int64_t* plan, int64_t n_pos, const uint8_t* locus_ref, int64_t n_loci);
int mipgen_accel_reads_consensus_locus_pileup(mipgen_accel* h, const char* mol_seq, const int32_t* mol_len, int32_t n, int32_t row, int32_t min_family, int32_t min_quality,
                                              int32_t max_indel, int32_t* probe_counts, int32_t* locus_counts, mipgen_gapped_totals* pileup_totals, mipgen_locus_totals* totals);
int mipgen_accel_reads_consensus_locus_call_pool(mipgen_accel* h, const char* mol_seq, const int32_t* mol_len, int32_t n, int32_t min_family, int32_t min_quality,
                                                 int32_t max_indel, int32_t bg_max_ppm);
int mipgen_accel_reads_consensus_locus_call(mipgen_accel* h, int32_t row, const mipgen_call_params* params, int32_t* probe_counts, int32_t* locus_counts,
                                            mipgen_call_totals* totals);
/* The totals locus_pileup would have returned as pileup_totals for the row of the last mipgen_accel_reads_consensus_locus_call: a caller that writes the pileup from
 * that call's probe_counts needs no second count.  MIPGEN_E_STATE before such a call. */
int mipgen_accel_reads_consensus_locus_call_pileup_totals(mipgen_accel* h, mipgen_gapped_totals* totals);

/* ---- insertion alleles: the inserted bases per anchor, counted per sample (new entry points only: the ABI number does not change) ----
 * Everything up to the vote at an anchor is the gapped pileup above, unchanged.  A used molecule at anchor t (0 <= t <= mol_len - 2) that no side covers counts
 * nothing; two covering sides with different lengths count `ins_discordant`; every other molecule SPANS the anchor with an agreed length l >= 0 (`span`), and with
 * l > 0 it is one EVENT (`ins`: exactly the molecules column 6 of the gapped table counts).  The inserted string of an event, in the orientation of M: a covering
 * side's run is the l read bases q[i .. i + l - 1], i the read index its path holds when it consumes the column in front of the run; base j is q[i + j] on the
 * extension side and complement(q[i + l - 1 - j]) on the ligation side, each with its quality; a base is usable as in the pileup (A C G T, quality - 33 >=
 * min_quality); base j of the molecule is the one usable base, or the common base of two usable ones that agree, else AMBIGUOUS, and so is the event then.  A run of
 * more than 15 bases (up to 2 max_indel, behind deletions) is always ambiguous.  An ALLELE is (pos = pos_off[p] + t, length, ambiguous, bases): bases holds 2 bits
 * per base (A C G T = 0..3), base 0 in the most significant of the 2 length used bits, and is 0 for an ambiguous event; all ambiguous events of one (pos, length) are
 * one allele.  Records come in ascending order of the key pos << 35 | length << 31 | ambiguous << 30 | bases (an allele longer than 15 bases: length field 0, its
 * length in the low bits - it comes first at its position), distinct, the same bytes from call to call.
 *   consensus_insertions: counts (n_pos x 8, may be NULL) is what mipgen_accel_reads_consensus_pileup_gapped returns for the same arguments; anchors (n_pos x 4 int32,
 *                         may be NULL): span, ins, ins_discordant, ambiguous (= the ambiguous events) per anchor, the row of t = mol_len - 1 zero.
 *                         anchors[:, 1] == counts[:, 6] and anchors[:, 2] == counts[:, 7]; per position the counts of the records add up to anchors[:, 1], those
 *                         of the ambiguous ones to anchors[:, 3].  totals (may be NULL): groups, used, gapped_sides as the gapped pileup's; span, insertions,
 *                         ins_discordant, ambiguous = the column sums; alleles = the records left on the handle.
 *   insertions_fetch:     the records of the last consensus_insertions; n must equal its totals.alleles.
 * MIPGEN_E_INVALID: every refusal of the gapped pileup; more than 2^29 - 1 template positions; more than 2^31 - 1 events in the row; fetch with another n.
 * MIPGEN_E_STATE: no consensus reads; fetch before any call (or after one that failed).  MIPGEN_E_NOMEM: the gapped pileup's bytes with 5 bytes per projected
 * position, 16 bytes per position of anchors, and - once the count has given the events - 48 bytes per event and the sort's scratch, against free device memory; each
 * check comes before the allocations it covers.  The call counts into scratch of its own (released with the reads): the pileup, call and locus entry points, their
 * scratch and timing indices 11-14 are untouched by it; it may be repeated, for any row in any order.  A handle with zero groups gives zeros. */
typedef struct mipgen_insertion_record { int64_t pos; int32_t length, count; uint32_t bases; int32_t ambiguous; } mipgen_insertion_record;
typedef struct mipgen_insertion_totals { int64_t groups, used, span, insertions, ins_discordant, ambiguous, alleles, gapped_sides; } mipgen_insertion_totals;
int mipgen_accel_reads_consensus_insertions(mipgen_accel* h, const char* mol_seq, const int32_t* mol_len, int32_t n, int32_t row, int32_t min_family, int32_t min_quality,
                                            int32_t max_indel, int32_t* counts, int32_t* anchors, mipgen_insertion_totals* totals);
int mipgen_accel_insertions_fetch(mipgen_accel* h, mipgen_insertion_record* records, int64_t n);

/* ---- insertion alleles called against a background of the other samples (new entry points only: the ABI number does not change) ----
 * Everything up to a row's allele records and its anchor table is the insertions call above, unchanged.  A record is TESTED material iff it is not ambiguous (so
 * 1 <= length <= 15); ambiguous records are never tested and never pooled as an alt, but their molecules stay in `span`, so in every denominator.  For a tested
 * record k = count and n = span of its anchor (n >= k >= 1).  Sample rows, qualification, leave-one-out, the filters, the score and the totals are those of the
 * variant calls above with (k, n) so defined: sample row s' qualifies at allele a = (pos, length, bases) iff n' > 0 and k' 10^6 <= bg_max_ppm n', k' its count of
 * exactly that allele (0 without such a record), n' its span at pos.  The POOL is sparse: S[pos] = the span summed over ALL sample rows, and per distinct
 * non-ambiguous allele of any sample row one record with bg_alt = K = the k' of the qualifying rows and bg_excluded = X = the n' of the rows whose record does not
 * qualify; N = S - X, and an allele no sample row carries has K = 0, N = S.  totals: tested = non-ambiguous records with min_depth <= n <= MIPGEN_CALL_MAX_DEPTH;
 * too_deep = those above the cap; candidates; calls.  Call records come in ascending order of the allele key, the same bytes from call to call; bg_alt, bg_depth =
 * K_o, N_o, the background without the row; reserved = 0.
 *   insertion_call_tables:     from host arrays, no read session needed: records[n_records] as insertions_fetch returns them (strictly ascending key order; ambiguous
 *                              ones are skipped), span[n_pos] the row's span per anchor, pool_records[n_pool] in strictly ascending key order, pool_span[n_pos] = S.
 *   consensus_insertion_pool:  the insertions route of every sample row of the session, appended, sorted and reduced on the device.  The pool stays with the consensus
 *                              reads and remembers these arguments; totals (may be NULL): rows = the sample rows, entries = their non-ambiguous records, alleles = the
 *                              distinct ones.  The allele records the insertions call left on the handle are gone afterwards.
 *   insertion_pool_fetch:      the distinct pool records (n must equal totals.alleles) and S (n_pos int32; either may be NULL).
 *   consensus_insertion_call:  recomputes the insertions of `row` (any row, undetermined included) with the pool's arguments - counts, anchors, ins_totals (each may
 *                              be NULL) are what mipgen_accel_reads_consensus_insertions returns for them, and mipgen_accel_insertions_fetch finds the row's
 *                              records - then flags, scores, orders and joins its calls.
 *   insertion_call_fetch:      the records of the last insertion call of either kind; n must equal its totals.calls.
 * MIPGEN_E_INVALID: every refusal of the insertions call and of the call parameters; n_pos outside 1..2^29 - 1; n_records or n_pool negative or above 2^29 - 1; a
 * record or pool position outside 0..n_pos - 1; records or pool not strictly ascending; a pool record with length outside 1..15; NULL arrays; a row of more than
 * 2^29 - 1 allele records; a fetch with another n.  MIPGEN_E_STATE: no consensus reads; pool_fetch or consensus_insertion_call without a pool, or with
 * params.bg_max_ppm different from the pool's; call_fetch before any insertion call.  MIPGEN_E_NOMEM: the bytes of the insertions call, 20 bytes per entry twice over and
 * the sort's scratch, 4 bytes per position, and the candidate list of a call (one per record) against free device memory; each check comes before the allocations it
 * covers.  The pileup, call, locus and insertions entry points, their records and timing indices 11-15 are untouched by these calls, except that the pool and the
 * call count into the scratch of mipgen_accel_reads_consensus_insertions. */
typedef struct mipgen_insertion_pool_record { int64_t pos; int32_t length; uint32_t bases; int32_t bg_alt, bg_excluded; } mipgen_insertion_pool_record;
typedef struct mipgen_insertion_call_record { int64_t pos; int32_t length; uint32_t bases; int32_t depth, alt, bg_alt, bg_depth, q, reserved; } mipgen_insertion_call_record;
typedef struct mipgen_insertion_pool_totals { int64_t rows, entries, alleles; } mipgen_insertion_pool_totals;
int mipgen_accel_insertion_call_tables(mipgen_accel* h, const mipgen_insertion_record* records, int64_t n_records, const int32_t* span, int64_t n_pos,
                                       const mipgen_insertion_pool_record* pool_records, int64_t n_pool, const int32_t* pool_span, int32_t own_row_is_sample,
                                       const mipgen_call_params* params, mipgen_call_totals* totals);
int mipgen_accel_reads_consensus_insertion_pool(mipgen_accel* h, const char* mol_seq, const int32_t* mol_len, int32_t n, int32_t min_family, int32_t min_quality,
                                                int32_t max_indel, int32_t bg_max_ppm, mipgen_insertion_pool_totals* totals);
int mipgen_accel_insertion_pool_fetch(mipgen_accel* h, mipgen_insertion_pool_record* pool_records, int64_t n, int32_t* pool_span);
int mipgen_accel_reads_consensus_insertion_call(mipgen_accel* h, int32_t row, const mipgen_call_params* params, int32_t* counts, int32_t* anchors,
                                                mipgen_insertion_totals* ins_totals, mipgen_call_totals* call_totals);
int mipgen_accel_insertion_call_fetch(mipgen_accel* h, mipgen_insertion_call_record* records, int64_t n);

/* ---- insertion alleles per genome locus: folded over the probes that cover it, pooled and called (new entry points only: the ABI number does not change) ----
 * Inputs of one row: its allele records (4.16: ascending key, pos = template position x, bases in the orientation of M), its anchor table anchors[n_pos][4] (span, ins,
 * ins_discordant, ambiguous) and a locus plan (4.15).  A source (x, flags) of locus l PULLS one anchor row: row x - 1 under bit 1, row x with flags 0, none on a minus
 * source without bit 1 - the rule by which the merged table takes its columns 6 and 7; the plan is obeyed as given, so an anchor row is pulled by at most two sources.
 * locus_anchors[n_loci][4] is the sum of the pulled rows, all four columns together.  Every record of a pulled row becomes a locus allele: pos = l; length and
 * ambiguous unchanged; bases unchanged on a source with bit 0 clear, and under bit 0 the reverse complement of a non-ambiguous record (base j becomes
 * 3 - base(length - 1 - j), base 0 still in the most significant used bits); an ambiguous record - a run above 15 bases included - stays bit for bit what it is.
 * Records of equal key add their counts; the locus records come as mipgen_insertion_record in ascending key order, distinct, the same bytes from call to call.
 * locus_anchors[:, 1] and [:, 2] equal columns 6 and 7 of the merged 8-column table of the same row; per locus the record counts add up to locus_anchors[:, 1], those
 * of the ambiguous ones to [:, 3].  totals: loci = loci with a non-zero anchor row; span, insertions, ins_discordant, ambiguous = the column sums; alleles = the locus
 * records; folded = the (record, source) pairs; dropped = the records no source pulls.  Pool and calls are those of 4.17 with x := l, span := locus_anchors[:, 0] and
 * n_pos := n_loci on the locus records of every row; a plus and a minus probe place an insertion inside a repeat at opposite ends of it, and those stay two alleles.
 *   locus_insertion_tables:            from host arrays, no read session needed; locus_anchors and totals may be NULL.
 *   locus_insertions_fetch:            the locus records of the last fold of the handle (tables, locus_insertions or locus_insertion_call); n must equal totals.alleles.
 *   consensus_locus_insertions:        the insertions call of `row` - counts, anchors, ins_totals and mipgen_accel_insertions_fetch are its results - folded under the
 *                                      installed plan.
 *   consensus_locus_insertion_pool:    4.17's pool over the sample rows with the fold between every row's insertions and the append; it stays with the consensus
 *                                      reads until the next locus plan.  locus_insertion_pool_fetch: its records and S[n_loci].
 *   consensus_locus_insertion_call:    recomputes and folds `row` with the pool's arguments, then flags, scores, orders and joins its calls into a run of its own:
 *                                      mipgen_accel_insertion_call_fetch and mipgen_accel_call_fetch keep finding what they found.  locus_insertion_call_fetch: the
 *                                      records, pos = the locus; n must equal call_totals.calls.
 * MIPGEN_E_INVALID: every refusal of the insertions call, of the call parameters and of the plan check; records not strictly ascending; a record position outside
 * 0..n_pos - 1; a sum of mol_len different from the plan's n_pos; more than 2^29 - 1 locus records in a row; a fetch with another n.  MIPGEN_E_STATE: no consensus
 * reads; no plan; a call without a locus insertion pool or with another bg_max_ppm than the pool's; a fetch before any call.  MIPGEN_E_NOMEM: the anchor map (8 bytes
 * per position), the 2 n_records pairs with their sorted copies, scratch and runs, the locus records and locus_anchors against held + free device memory, each before
 * the allocations it covers.  Timing index 17; indices 11-16 and every other entry point's records are untouched, except that the session calls count into the scratch
 * of mipgen_accel_reads_consensus_insertions. */
typedef struct mipgen_locus_insertion_totals { int64_t loci, span, insertions, ins_discordant, ambiguous, alleles, folded, dropped; } mipgen_locus_insertion_totals;
int mipgen_accel_locus_insertion_tables(mipgen_accel* h, const mipgen_insertion_record* records, int64_t n_records, const int32_t* anchors, const int64_t* plan, int64_t n_pos,
                                        int64_t n_loci, int32_t* locus_anchors, mipgen_locus_insertion_totals* totals);
int mipgen_accel_locus_insertions_fetch(mipgen_accel* h, mipgen_insertion_record* records, int64_t n);
int mipgen_accel_reads_consensus_locus_insertions(mipgen_accel* h, const char* mol_seq, const int32_t* mol_len, int32_t n, int32_t row, int32_t min_family, int32_t min_quality,
                                                  int32_t max_indel, int32_t* counts, int32_t* anchors, int32_t* locus_anchors, mipgen_insertion_totals* ins_totals,
                                                  mipgen_locus_insertion_totals* totals);
int mipgen_accel_reads_consensus_locus_insertion_pool(mipgen_accel* h, const char* mol_seq, const int32_t* mol_len, int32_t n, int32_t min_family, int32_t min_quality,
                                                      int32_t max_indel, int32_t bg_max_ppm, mipgen_insertion_pool_totals* totals);
int mipgen_accel_locus_insertion_pool_fetch(mipgen_accel* h, mipgen_insertion_pool_record* pool_records, int64_t n, int32_t* pool_span);
int mipgen_accel_reads_consensus_locus_insertion_call(mipgen_accel* h, int32_t row, const mipgen_call_params* params, int32_t* counts, int32_t* anchors, int32_t* locus_anchors,
                                                      mipgen_insertion_totals* ins_totals, mipgen_locus_insertion_totals* locus_totals, mipgen_call_totals* call_totals);
int mipgen_accel_locus_insertion_call_fetch(mipgen_accel* h, mipgen_insertion_call_record* records, int64_t n);

/* Featurev5::get_long_range_content on the device: extended_seq covers the region +/- 1000 bases
 * (mipgen.cpp:1125-1128,1225); denominator = chrom_seq_stop - chrom_seq_start + 2001 (Featurev5.cpp:49,53). */
int mipgen_accel_long_range_content(mipgen_accel* h, const char* extended_seq, int32_t len,
                                    int32_t chrom_seq_start, int32_t chrom_seq_stop, double* out44);
/* the same for n regions in one launch (one workgroup per region); out is [n][44] */
int mipgen_accel_long_range_content_batch(mipgen_accel* h, int32_t n, const char* const* extended_seqs, const int32_t* lens,
                                          const int32_t* chrom_seq_starts, const int32_t* chrom_seq_stops, double* out);

/* Replays the reference's score-dependent enumeration control flow (mipgen.cpp:426-437,494-497) over the
 * scored dense grid on the device and folds condense_mips (mipgen.cpp:1670-1746) per (scan start, strand).
 * emitted_dev/ survivors are library-owned device arrays; results are fetched with the calls below. */
int mipgen_accel_replay_condense(mipgen_accel* h);
/* results of the window replayed last: per-region emitted-candidate counts (int64[regions of the window]), survivors (2 per scan
 * position of the window: '+','-') and the emitted mask (one byte per candidate of the window).  Any pointer may be NULL. */
int mipgen_accel_download_replay(mipgen_accel* h, int64_t* emitted_per_region, mipgen_survivor* survivors,
                                 int64_t survivor_capacity, uint8_t* emitted_mask, int64_t mask_capacity);
/* after mipgen_accel_score_condense_all: emitted counts of every region (int64[n_regions]) and the survivors of every scan position
 * of the batch (2 per position, region order) */
int mipgen_accel_download_survivors(mipgen_accel* h, int64_t* emitted_per_region, mipgen_survivor* survivors, int64_t survivor_capacity);
/* device pointer of that survivor array (mipgen_survivor[n_survivors], batch order): the send buffer of the multi-GPU gather */
int mipgen_accel_survivors_device_ptr(const mipgen_accel* h, void** survivors_dev, int64_t* n_survivors);

/* collapse_mips (mipgen.cpp:1616-1649) on the device, over the survivors of the window replayed last: for every base a survivor's
 * scan target can cover (bases first_pos .. first_pos + n_bases - 1 of each region, n_bases = n_pos + largest scan size - 1) and each
 * strand, the scan-start index (0-based from the region's first_pos) of the survivor the reference's fold keeps, or -1.
 * mipgen_accel_score_condense_all runs it for every window. */
int mipgen_accel_collapse(mipgen_accel* h);
/* entries [first_entry, first_entry + 2 * n_bases) of the batch-wide collapsed array belong to `region`: [base][strand] */
int mipgen_accel_region_bases(const mipgen_accel* h, int32_t region, int64_t* first_entry, int32_t* n_bases);
/* window >= 0: the entries of that window's regions; window < 0: the whole batch (after mipgen_accel_score_condense_all) */
int mipgen_accel_download_collapsed(mipgen_accel* h, int32_t window, int32_t* best_scan_index, int64_t capacity);

/* ---- mixed designs: the SVR score of every condensed survivor, computed where the survivors are --------------------------------------
 * The reference re-scores the MIPs its pick stage tests one at a time (mipgen.cpp:1523-1527, 1533-1537, 1546-1550, 1873-1877: get_parameters +
 * predict_value, score overwritten in place).  mipgen_accel_rescore_survivors scores EVERY condensed survivor of the window scored + replayed
 * last in one list call on the device (the same kernels and values as mipgen_accel_score_candidates on that list) and keeps the values in the
 * handle, slot for slot beside the survivors (NaN where a slot holds no survivor); the selection stage looks them up. */
int mipgen_accel_rescore_survivors(mipgen_accel* h);
int mipgen_accel_download_survivor_scores(mipgen_accel* h, int32_t window, double* svr, int64_t capacity /* >= 2 * n_positions of the window */);

/* ---- device-side views of a result window ---------------------------------------------------------------------------------------------
 * For a caller that moves results between devices itself - the multi-GPU front end posts these arrays to GPU 0 with one grouped RCCL
 * send / receive per window instead of taking them down each device's own PCIe link.  Pointers into the handle's own device arrays, valid
 * until the next mipgen_accel_upload_regions / mipgen_accel_destroy (text: until the next mipgen_accel_format_all_mips); a field is NULL
 * when the window does not hold it.  mipgen_accel_synchronize waits for everything the handle has enqueued, so that another stream may read
 * them.  cand_index of the survivors is batch-wide: subtract first_candidate for the window-relative index of mipgen_accel_window_info. */
typedef struct mipgen_window_views {
    const void* emitted;             /* int64 [n_emitted]: emitted candidates per region of the window */
    const void* survivors;           /* mipgen_survivor [n_survivors] = 2 per scan position */
    const void* collapsed;           /* int32 [n_collapsed] = 2 per base, region after region (mipgen_accel_collapse) */
    const void* survivor_svr;        /* double [n_survivors] (mipgen_accel_rescore_survivors) */
    const void* text;                /* all_mips text of the last mipgen_accel_format_all_mips, if this is the window it ran on */
    int64_t n_emitted, n_survivors, n_collapsed, n_text_bytes;
    int64_t first_candidate;
} mipgen_window_views;
int mipgen_accel_window_views(mipgen_accel* h, int32_t window, mipgen_window_views* out);
int mipgen_accel_synchronize(mipgen_accel* h);

/* ---- section 8f-4: the all_mips records of a window, formatted on the device -----------------------------------------------------
 * print_details (mipgen.cpp:765-794) for every candidate the replay marked as constructed, in the reference's generation order
 * (position, capture size, arm pair, plus then minus), numbered from first_index + 1 (the running all_mip_counter, mipgen.cpp:474,488):
 * 20 tab-separated columns, scores as printf("%g"), copy numbers from the copy table, mip_sequence = lig + middle + ext.
 * Call after mipgen_accel_replay_condense on the scored window; names[i] describes region i of that window. */
typedef struct mipgen_record_names {
    const char* chr;                 /* Featurev5::chr */
    const char* label;               /* Featurev5::label */
    int32_t feature_start;           /* start_position - 1 (mipgen.cpp:788) */
    int32_t feature_stop;            /* stop_position (:789) */
} mipgen_record_names;
int mipgen_accel_format_all_mips(mipgen_accel* h, const mipgen_record_names* names, const char* middle, int64_t first_index,
                                 int64_t* n_records, int64_t* n_bytes);
/* the text of the last mipgen_accel_format_all_mips (n_bytes bytes, no terminator) */
int mipgen_accel_download_text(mipgen_accel* h, char* dst, int64_t capacity);

/* ---- section 8f-3 (opt-in): arm-oligo copy numbers without the bwa round trip ----------------------------------------------------
 * Replaces check_copy_numbers / find_copy's oligo half (mipgen.cpp:825-835 writes every arm oligo to a FASTQ file, :558-596 reads bwa's
 * X0:i best-hit count back): an oligo always matches itself, so its best hits are its exact occurrences on either strand, counted here in
 * ONE streaming pass over the genome (1 byte per base; canonical 2-bit k-mer keys, exact for lengths <= 31).
 *   chrom_seqs / chrom_lens   the genome the oligos are counted against (ASCII, any case; non-ACGT bytes break k-mers)
 *   region_seqs / region_lens the region strings (Featurev5::chromosomal_sequence)
 *   lengths                   the design's distinct oligo lengths, ascending
 *   copy_out[r]               int32 [n_lengths][region_lens[r]]: exactly the mipgen_region.copy slices (copy[len][start - seq_start]);
 *                             oligos with a non-ACGT byte get 100 (a read without an X0 tag, :589-592), oligos that would run past the
 *                             region string 0 (never written, :829)
 * The uniqueness test of whole capture windows (:841-868) is mipgen_accel_window_uniqueness() below. */
int mipgen_accel_count_oligo_copies(mipgen_accel* h, int32_t n_chrom, const char* const* chrom_seqs, const int64_t* chrom_lens,
                                    int32_t n_regions, const char* const* region_seqs, const int32_t* region_lens,
                                    int32_t n_lengths, const int32_t* lengths, int32_t* const* copy_out);

/* The capture-window half of check_copy_numbers (mipgen.cpp:806-823 writes every capture window to a FASTQ file, :841-868 marks a window start
 * "unmappable" unless bwa's SAM line contains "X0:i:1" and "X1:i:0"; design_mip sets mapping_failed there, :615-625).  Model: a window taken from
 * the genome matches itself exactly, so X0 = its exact occurrences on either strand and X1 = its occurrences with exactly ONE SUBSTITUTION
 * (Hamming distance 1); bwa aln's gapped one-difference hits are not searched.  The substring tests of :852 are kept (X0 printed with a leading
 * '1' passes: 1, 10-19, ...).  Seed-and-extend from the k-mer table: a window within distance 1 of a locus contains its first or its second
 * seed_len-mer exactly, so only the loci of repeated seeds are extended (two streaming passes over the genome).
 *   sizes                     capture sizes (any order), each >= 2 * seed_len
 *   seed_len                  12..31; the design's longest arm oligo (30) is the natural choice
 *   unmap_out[r]              uint8 [n_sizes][region_lens[r]]: 1 = the window of sizes[c] starting at index i of the region string is not unique
 *                             (or holds a non-ACGT byte); 0 = unique, or the window does not fit into the region string.  The caller keeps
 *                             the starts the reference enumerates ([start_flanked - C, stop_flanked), :808-812) - exactly mipgen_region.unmappable. */
int mipgen_accel_window_uniqueness(mipgen_accel* h, int32_t n_chrom, const char* const* chrom_seqs, const int64_t* chrom_lens,
                                   int32_t n_regions, const char* const* region_seqs, const int32_t* region_lens,
                                   int32_t n_sizes, const int32_t* sizes, int32_t seed_len, uint8_t* const* unmap_out);

/* The same test for a caller that wants exactly mipgen_region.unmappable: `bounds` gives, per region, the coordinates the reference's lookup is limited
 * by (mipgen.cpp:808-813: a window start is written only for current_mip_start in [start_flanked - C, stop_flanked), > 0, with the window inside the
 * region string [seq_start, seq_stop]); the flags of every other start are cleared ON THE DEVICE, the flag image stays in the handle, and any_out[r]
 * (one byte per region) says whether region r has a flagged start at all.  Only those regions need mipgen_accel_window_flags_region (out: uint8
 * [n_sizes][region_lens[r]]); mipgen_accel_window_uniqueness_end releases the image (so do the next _begin and mipgen_accel_destroy).  An exome design
 * has a flagged start in a few percent of its regions: 560 MB of flags stay where they were computed. */
typedef struct mipgen_window_bounds { int32_t start_flanked, stop_flanked, seq_start, seq_stop; } mipgen_window_bounds;
int mipgen_accel_window_uniqueness_begin(mipgen_accel* h, int32_t n_chrom, const char* const* chrom_seqs, const int64_t* chrom_lens,
                                         int32_t n_regions, const char* const* region_seqs, const int32_t* region_lens, const mipgen_window_bounds* bounds,
                                         int32_t n_sizes, const int32_t* sizes, int32_t seed_len, uint8_t* any_out);
int mipgen_accel_window_flags_region(mipgen_accel* h, int32_t region, uint8_t* out);
int mipgen_accel_window_uniqueness_end(mipgen_accel* h);

/* The same counts, kept in the handle's device memory in the layout the scoring kernels read (288 GB of HBM: the tables of a whole exome
 * are 6.7 GB and would otherwise cross PCIe twice).  The oligo lengths are the ones the handle's arm pairs use.  The next
 * mipgen_accel_upload_regions must pass the SAME regions (count, order, seq_len) with copy = MIPGEN_COPY_RESIDENT in every one of them;
 * any other upload discards the resident tables.  Counts of 65535 and more - which the 16-bit record fields cannot carry and the host looks
 * up instead (MIPGEN_REC_EXT_COPY) - are returned as a list owned by the handle, valid until the next call on it
 * (start = 0-based offset of the oligo in the region string). */
#define MIPGEN_COPY_RESIDENT ((const int32_t* const*)(uintptr_t)1)
typedef struct mipgen_big_copy { int32_t region, length, start, copies; } mipgen_big_copy;
int mipgen_accel_count_oligo_copies_resident(mipgen_accel* h, int32_t n_chrom, const char* const* chrom_seqs, const int64_t* chrom_lens,
                                             int32_t n_regions, const char* const* region_seqs, const int32_t* region_lens,
                                             int64_t* n_big, const mipgen_big_copy** big);

/* ---- tuning ---------------------------------------------------------------------------------------- */
/* A dense SVR launch with few tiles is split along the support-vector list so that it still fills the chip (partial sums are added
 * in a fixed order: results are deterministic for a given split).  0 = chosen per launch from the tile count (default), n >= 1 forces
 * n parts - e.g. to compare two differently sized batches bit for bit. */
int mipgen_accel_set_sv_split(mipgen_accel* h, int32_t n_split);
/* SVR scores that sit within the device kernels' error (~1e-12) of a midpoint between two 6-significant-digit numbers - the precision the
 * front end prints scores with (mipgen.cpp:774) - are re-scored in the reference's own operation order (svm.cpp:329-368, 2511-2515: index-order
 * sums, every operation rounded on its own) and overwritten, so that the printed digit is the reference's.  On by default; 0 switches it off
 * (measurements, tests of the mechanism).  Dense windows and candidate lists (mixed designs) alike.  Should a window hold more such scores
 * than the re-score list (1/1024 of its candidates + 4096), the next download of its results fails with MIPGEN_E_STATE instead of handing
 * out digits that are not guaranteed. */
/* (ABI 4: logistic scores take the same route - within 1e-11 of a midpoint they are re-scored with the 69 terms in the reference's order, SVMipv4.cpp:176-247.) */
int mipgen_accel_set_print_exact(mipgen_accel* h, int32_t on);
/* The reference stops constructing candidates at a scan position for good once a capture size starts with previous_best_score above the upper
 * score limit (mipgen.cpp:430).  A region of more than nine capture sizes is scored in runs of <= 9 sizes; with this switch on the runs are scored in
 * order and a tile of a later run is left out when every one of its positions has stopped before it - exactly the candidates the reference never
 * constructs.  Emitted masks, emitted counts, survivors, collapse results and all_mips records are unchanged (the replay never consults the rows
 * behind a position's exit); the DENSE scores of skipped tiles read NaN, which is why the switch is off by default for callers that fetch the dense
 * grid.  SVR scoring through the tiled kernel only.  How much it saves is a property of the model (how early the arm-sum lists' last pairs score above
 * the limit); mipgen_accel_skipped_candidates returns - and resets - the dense candidates left out since the last call. */
int mipgen_accel_set_dynamic_skip(mipgen_accel* h, int32_t on);
int mipgen_accel_skipped_candidates(mipgen_accel* h, int64_t* n);
/* inspection: per scan position of the window scored last with the switch on, the state after its last-but-one run (0 still constructing, 1 stopped,
 * 2 too close to the limit to call) and previous_best_score there; either output may be NULL */
int mipgen_accel_skip_state(mipgen_accel* h, uint8_t* state, double* previous_best, int64_t capacity);
/* The dense logistic kernel gives a workgroup `n` consecutive runs of scan positions (it stages the bases once and slides its downstream-arm
 * table from run to run).  0 = chosen from the batch size (1 for small batches, which need every workgroup they can get; 2 or 3 for large ones),
 * 1..8 forced.  Results do not depend on it. */
int mipgen_accel_set_logistic_subruns(mipgen_accel* h, int32_t n);

/* ---- training (svm.cpp:2095 svm_train, epsilon-SVR with an RBF kernel) ------------------------------ */
/* libsvm's svm-train -s 3 -t 2 -h 1 on the device: the same model file, byte for byte (svm_save_model, svm.cpp:2644-2757).  The whole n x n float
 * kernel matrix stays resident in HBM, so n is limited to MIPGEN_SVR_TRAIN_MAX_ROWS (64 GiB of matrix); a larger n is MIPGEN_E_NOMEM before anything
 * is allocated. */
#define MIPGEN_SVR_TRAIN_MAX_ROWS 131072
typedef struct mipgen_svr_train_params {
    double gamma, cost, epsilon_p, eps;   /* -g, -c, -p, -e: gamma >= 0, cost > 0, epsilon_p >= 0, eps > 0 (svm_check_parameter, svm.cpp:3026) */
    int32_t shrinking, reserved;          /* shrinking must be 1 (-h 1) */
} mipgen_svr_train_params;
typedef struct mipgen_svr_train_info {
    int64_t iterations;                   /* the solver's #iter */
    int32_t n_sv, n_bsv;                  /* nSV, nBSV as svm_train_one counts them (svm.cpp:1677-1694) */
    double rho, obj;
    int32_t n_shrink, n_reconstruct;      /* do_shrinking calls; reconstruct_gradient calls that rebuilt an inactive gradient */
    double gram_ms, solve_ms;             /* HIP-event time of the kernel-matrix build; wall time of the solver loop */
} mipgen_svr_train_info;
/* x: row-major [n][192] features (absent libsvm indices = 0), y: n targets; all finite.  Trains, writes model_path as svm_save_model would, then
 * installs it through mipgen_accel_load_model_file.  Invalid arguments are MIPGEN_E_INVALID and leave the handle's model as it was.  info may be NULL. */
int mipgen_accel_train_svr(mipgen_accel* h, int32_t n, const double* x, const double* y, const mipgen_svr_train_params* p, const char* model_path,
                           mipgen_svr_train_info* info);

/* ---- model selection (svm.cpp:2342 svm_cross_validation; svm-train -v n, and a grid of parameter sets around it) --------- */
/* New entry points only: the ABI number does not change.  Every (parameter set, fold) is one problem of a batch that the device solves at once, one
 * workgroup per problem, over ONE kernel matrix per distinct gamma (a fold's matrix is a gather of it); every fold model is the one svm_train gives
 * svm_cross_validation, byte for byte when saved, and target is svm_predict's value within 1e-5. */
typedef struct mipgen_svr_cv_point  { double gamma, cost, epsilon_p; } mipgen_svr_cv_point;
typedef struct mipgen_svr_cv_result {
    double mse, r2;                       /* svm-train's "Cross Validation Mean squared error" / "Squared correlation coefficient", over target and y */
    int64_t iterations;                   /* #iter summed over the folds */
    int32_t n_sv_total, reserved;         /* nSV summed over the folds */
} mipgen_svr_cv_result;
/* host only, no device needed: libsvm's fold assignment for a regression problem (svm.cpp:2408-2415) from glibc's rand() stream as srand(seed)
 * leaves it (seed 1 = what svm-train, which never seeds, gets; the library keeps its own copy of the generator and never calls rand()).
 * perm[n], fold_start[nr_fold + 1]: fold i holds out rows perm[fold_start[i] .. fold_start[i + 1]).  nr_fold > n is clipped to n as libsvm does;
 * nr_fold_used (may be NULL) receives the count in use. */
int mipgen_accel_svr_cv_folds(int32_t n, int32_t nr_fold, uint32_t seed, int32_t* perm, int32_t* fold_start, int32_t* nr_fold_used);
/* n_points parameter sets x nr_fold folds in one call; x, y, eps as mipgen_accel_train_svr takes them (same checks, same messages), nr_fold >= 2,
 * n_points >= 1, n >= 2.  target: [n_points][n] held-out predictions in original row order (may be NULL); results: [n_points];
 * fold_model_prefix (may be NULL): writes "<prefix>.<point>.<fold>.model" as svm_save_model would.  The handle's model is untouched.
 * Points are processed gamma by gamma, one n x n float matrix resident at a time (n <= MIPGEN_SVR_TRAIN_MAX_ROWS); MIPGEN_E_NOMEM before any
 * allocation when the matrix plus the solver state of the largest gamma group's points x folds problems does not fit the device's free memory. */
int mipgen_accel_cross_validate_svr(mipgen_accel* h, int32_t n, const double* x, const double* y, int32_t nr_fold, uint32_t seed, double eps,
                                    int32_t n_points, const mipgen_svr_cv_point* points, double* target, mipgen_svr_cv_result* results,
                                    const char* fold_model_prefix);

/* ---- deletion alleles: start and length per molecule, counted per sample --------------- */
/* Everything up to the vote of a molecule at a template position is the gapped pileup's (4.13), `del` as fifth class.  Let c[t], 0 <= t < L, be the voted class of a
 * used molecule of probe p at position t: A C G T, discordant, del, or nothing.  A deletion EVENT of the molecule is a maximal run [a, a + l) of positions with
 * c[t] == del, so every del the gapped pileup counts belongs to exactly one event; l is bounded by L, not by max_indel.  The event is RAGGED when the molecule is
 * discordant at a - 1 or at a + l with one of its two usable observations there a del: the two sides disagree on its extent (a flank outside [0, L) is never ragged).
 * An ALLELE is (pos = pos_off[p] + a, length, ragged); records come in ascending order of the key pos << 35 | length << 1 | ragged, distinct, the same bytes from
 * call to call.  The depth of a record is the depth at its FIRST deleted base: the used molecules whose class there is one of A C G T del - what the per-base caller
 * of 4.14 takes as depth there -, so count <= depth and depth >= 1.
 *   consensus_deletions: counts (n_pos x 8, may be NULL) is what mipgen_accel_reads_consensus_pileup_gapped returns for the same arguments; sites (n_pos x 4 int32, may
 *                        be NULL): depth, starts (events whose first base is here), ragged (those of them that are ragged), del (molecules that vote del here) per
 *                        position.  sites[:, 3] == counts[:, 5]; sites[:, 0] == counts[:, 0:4].sum(1) + counts[:, 5]; per position the counts of the records add up to
 *                        sites[:, 1], those of the ragged ones to sites[:, 2]; for every position t the counts of the records with pos <= t < pos + length add up to
 *                        counts[t][5].  totals (may be NULL): groups, used, gapped_sides as the gapped pileup's; depth = the sum of sites[:, 0]; deleted_bases = the sum
 *                        of length x count = the gapped pileup's deletions; events, ragged = the sums of sites[:, 1] and [:, 2]; alleles = the records left on the handle.
 *   deletions_fetch:     the records of the last consensus_deletions; n must equal its totals.alleles.
 * MIPGEN_E_INVALID: every refusal of the gapped pileup; more than 2^29 - 1 template positions; more than 2^31 - 1 deleted bases (the bound of the events) in the row;
 * fetch with another n.  MIPGEN_E_STATE: no consensus reads; fetch before any call (or after one that failed behind its refusals).  MIPGEN_E_NOMEM: the gapped pileup's
 * bytes, 16 bytes per position of sites, and - once the count has given the deleted bases - 48 bytes per possible event and the sort's scratch, against held + free
 * device memory; each check comes before the allocations it covers.  The call counts into scratch of its own (released with the reads): every other entry point, its
 * scratch, its records and timing indices 0-18 are untouched by it; it may be repeated, for any row in any order.  A handle with zero groups gives zeros. */
typedef struct mipgen_deletion_record { int64_t pos; int32_t length, count, ragged, depth; } mipgen_deletion_record;
typedef struct mipgen_deletion_totals { int64_t groups, used, depth, deleted_bases, events, ragged, alleles, gapped_sides; } mipgen_deletion_totals;
int mipgen_accel_reads_consensus_deletions(mipgen_accel* h, const char* mol_seq, const int32_t* mol_len, int32_t n, int32_t row, int32_t min_family, int32_t min_quality,
                                           int32_t max_indel, int32_t* counts, int32_t* sites, mipgen_deletion_totals* totals);
int mipgen_accel_deletions_fetch(mipgen_accel* h, mipgen_deletion_record* records, int64_t n);

/* ---- instrumentation ------------------------------------------------------------------------------ */
/* HIP-event time (ms) of the kernels of the last scoring call (summed over its windows), measured on the handle's stream;
 * negative if unavailable.  which: 0 = dense SVR kernel, 1 = records + scoring kernels, 2 = records / logistic kernel,
 * 3 = replay + condense; 4 = genome pass of the last mipgen_accel_count_oligo_copies (always recorded);
 * 5 / 6 = the matrix-core SVR kernel / the feature kernel of the last mipgen_accel_score_candidates or mipgen_accel_score_probes call on a list
 * (>= 256 SVR candidates); 7 = k_read_assign summed over the feed calls since the last mipgen_accel_reads_open (timing enabled);
 * 8 = k_sample_assign summed over the feed calls since the last mipgen_accel_reads_open_samples (timing enabled);
 * 9 = the two k_consensus_vote kernels of the last mipgen_accel_reads_finish_consensus, 10 = its sort of (key, pair id) and the run boundaries
 * (timing enabled); 11 = the pileup kernels of the last mipgen_accel_reads_consensus_pileup (timing enabled); 12 = the kernels of the last
 * mipgen_accel_reads_consensus_pileup_gapped (timing enabled); 13 = the kernels of the last mipgen_accel_call_tables, mipgen_accel_reads_consensus_call (its pileup
 * included) or mipgen_accel_reads_consensus_call_pool (timing enabled); 14 = the kernels of the last locus call of any kind (mipgen_accel_locus_tables,
 * mipgen_accel_reads_consensus_locus_*), its pileup included (timing enabled); 15 = the kernels of the last mipgen_accel_reads_consensus_insertions, its
 * placement and count included (timing enabled); 16 = the kernels of the last insertion pool or insertion call of either kind (mipgen_accel_insertion_call_tables,
 * mipgen_accel_reads_consensus_insertion_pool, mipgen_accel_reads_consensus_insertion_call), the insertions route of its rows included (timing enabled);
 * 17 = the kernels of the last locus insertions call of any kind (mipgen_accel_locus_insertion_tables, mipgen_accel_reads_consensus_locus_insertions, _locus_insertion_pool,
 * _locus_insertion_call), the insertions route of its rows included (timing enabled); 18 = k_tag_parent, k_tag_root and k_tag_rewrite of the last
 * mipgen_accel_reads_finish_consensus of a session with tag mismatches 1 (timing enabled; its second sort and run boundaries are part of 10); 19 = the kernels of
 * the last mipgen_accel_reads_consensus_deletions, its placement and count included (timing enabled). */
double mipgen_accel_last_kernel_ms(mipgen_accel* h, int32_t which);
/* enable/disable per-call event timing (it inserts two hipEventRecord per call) */
int mipgen_accel_set_timing(mipgen_accel* h, int32_t enabled);

#ifdef __cplusplus
}
#endif
#endif /* MIPGEN_ACCEL_H */
