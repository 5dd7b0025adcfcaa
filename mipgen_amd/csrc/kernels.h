// kernels.h — the boundary between the kernel files (kernels_*.hip) and the host side of libmipgen_accel.so (accel*.hip): the structs that
// cross it and every launcher / LDS-sizing function, declared once.  Each kernels_*.hip includes it, so a definition that drifts from its
// declaration fails to compile instead of linking (the symbols are extern "C").  The SVR trainer keeps its own boundary in svr_train.h.
#pragma once
#include <hip/hip_runtime.h>
#include "common.h"
#include "reads_common.h"
#include "call_model.h"
#include "insertion_call_model.h"

struct HostConsts;                   // logistic_device.h: crosses the boundary by pointer only
struct LrcMers { int8_t k[MIPGEN_N_LRC], code[MIPGEN_N_LRC], rc[MIPGEN_N_LRC]; };   // per mer: length, base-4 code, code of its reverse complement (-1: palindrome)
struct FmtRegion {                    // per region of the window: what print_details reads from Featurev5
    int32_t chr_off, chr_len;         // into the string pool
    int32_t label_off, label_len;
    int32_t feature_start, feature_stop;   // start_position - 1, stop_position (mipgen.cpp:788-789)
    int64_t rb0;                      // first row block of the region in the window
};
struct FmtConst {
    char middle[96];                  // universal_middle_mip_seq (mipgen.cpp:199-200)
    int32_t middle_len;
    int32_t n_regions;
    int64_t first_index;              // all_mip_counter before this window
};

struct KmerParams {
    int32_t n_k;                       // requested oligo lengths, ascending
    int32_t k[MIPGEN_MAX_OLIGO];
    int32_t kmax;
    int32_t filter_bits;               // log2 of the Bloom bitmap size in bits (>= KMER_LDS_BITS, kmer_common.h)
    uint64_t cap_mask;                 // partition capacity - 1 (power of two)
};

// the consensus reads a handle holds, as the pileup kernels see them
struct ConsensusView {
    const uint64_t* __restrict__ keys;        // (cell << 32) | tag of every group, ascending
    const int32_t* __restrict__ family;
    const int64_t* __restrict__ ext_off;      // n_groups + 1
    const int64_t* __restrict__ lig_off;
    const uint8_t* __restrict__ ext_seq;
    const uint8_t* __restrict__ ext_qual;
    const uint8_t* __restrict__ lig_seq;
    const uint8_t* __restrict__ lig_qual;
    int64_t n_groups;
};

// the plan of one row of a pileup: units[0, n_small) are the (probe, round) units of the one-wavefront kernel, units[n_small, n_small + n_big) of
// the workgroup kernel; the groups of probe p are [start[p], start[p + 1]); its positions lie at pos_off[p] of the n_pos positions of the table
struct PileRow {
    const uint2* __restrict__ units;
    int64_t n_small, n_big;
    const uint32_t* __restrict__ start;       // n + 1
    const int32_t* __restrict__ mol_len;      // n
    const int64_t* __restrict__ pos_off;      // n
    int32_t n;
    int64_t n_pos;
    uint32_t cell0;                           // the row's first cell
    int min_family, min_quality;
};

// variant calls: what k_call_flag and k_call_tail count; the positions one call takes: 4 candidates per position stay below the 2^31 - 1 pairs of the sort
struct CallCounters { unsigned long long tested, too_deep, candidates, calls; };
#define MIPGEN_CALL_MAX_POSITIONS (((int64_t)1 << 29) - 1)

// insertion calls: the entries appended to the sparse pool so far, its distinct alleles
struct InsPoolCounters { unsigned long long entries, alleles; };

// loci: the totals of a merged table, as k_locus_sum counts them
struct LocusCounters { unsigned long long covered, bases, discordant, deletions, insertions, ins_discordant; };

// insertion alleles per locus: the totals of a locus anchor table, the runs of the sorted pairs, the (record, source) pairs and the records no source pulls
struct LocusInsCounters { unsigned long long loci, span, insertions, ins_discordant, ambiguous, alleles, folded, dropped; };

extern "C" {
// kernels_logistic.hip, kernels_logistic_dense.hip: the two producers of the dense grid's records, bit-identical - both stage the tile's bases and take
// every window count from prefix_words.h, the record rules from mip_record.h and the bounds skips from mip_bounds.h.  k_records_logistic (one candidate per
// lane; span = bases a tile can touch) scores where the window tables of k_logistic_dense do not fit, and writes the records alone for the SVR kernels
size_t mipgen_logistic_lds_bytes(int span);
hipError_t mipgen_launch_records_logistic(hipStream_t, int score, int n_tiles, int span_max, const DevParams*, const DevRegion*, const LogTile*, const uint8_t*, const int32_t*,
                                          const uint8_t*, const HostConsts*, double*, uint64_t*, int64_t* sat_idx, unsigned int* sat_count, unsigned int sat_cap);
// k_logistic_dense (tables per arm / insert window, a (position, size) row per wavefront pass); lds_bytes: the host's tile sizing
size_t mipgen_logistic_dense_lds_bytes(int np_all, int np, int ssr, int ssmax, int Lmax, int n_up, int n_dn);
hipError_t mipgen_launch_logistic_dense(hipStream_t, int n_tiles, size_t lds_bytes, const DevParams*, const DevRegion*, const SvrTile*, const uint8_t*, const int32_t*,
                                        const uint8_t*, const HostConsts*, double*, uint64_t*, int64_t* sat_idx, unsigned int* sat_count, unsigned int sat_cap);
// kernels_svr.hip
size_t mipgen_svr_lds_bytes_tile(int np, int ss_range, int ssmax, int Lmax, int n_arm, int group, int n_e, int n_l, int n_threads, int it_pitch);
int mipgen_svr_scores_fit_lds(int np, int kc, int n_pairs, int ss_range, int ssmax, int Lmax, int n_arm, int group, int n_e, int n_l, int n_threads, int it_pitch);
hipError_t mipgen_launch_svr_dense(hipStream_t, int n_tiles, int n_tiles_few, size_t lds_bytes, const DevParams*, const SvrGeom*, const SvrGeom* geom_few, const DevRegion*,
                                   const SvrTile*, const uint8_t*, const int32_t*, const double* log10_tab, const double* model, int n_sv, double gamma_l2e, double rho,
                                   double s_guard, const uint64_t* records, double* scores, int64_t n_cand, int n_split, double* partials);
// kernels_skip.hip
hipError_t mipgen_launch_svr_run_state(hipStream_t s, int64_t n_pos, const DevParams* P, const DevRegion* regions, const int32_t* pos_region, const int32_t* pos_local,
                                       const uint32_t* run_bounds, int max_levels, int level, double margin, const double* scores, const uint64_t* records, double* pbs,
                                       uint8_t* state);
hipError_t mipgen_launch_svr_tile_keep(hipStream_t s, int n_tiles, const SvrTile* tiles, const int64_t* region_pos0, int64_t win_pos0, const uint8_t* state, int64_t* keep);
hipError_t mipgen_launch_svr_tile_compact(hipStream_t s, int n_tiles, const SvrTile* tiles, const int64_t* keep, const int64_t* offs, SvrTile* out, const DevParams* P,
                                          const DevRegion* regions, double* scores, unsigned long long* skipped);
// kernels_svr_gemm.hip
hipError_t mipgen_launch_svr_gemm(hipStream_t, int n, const double* feats, const uint64_t* records, const double* model_t, const double* sv_norm, const double* sv_coef,
                                  const double* center, int n_sv_pad, double gamma, double rho, double* scores);
// kernels_misc.hip: the list scorers over either source of a list (candidates by coordinates / probes by sequence: ListSrc, common.h) ...
hipError_t mipgen_launch_features_batch(hipStream_t, int n, const ListSrc&, const HostConsts*, uint64_t* records, double* features);
hipError_t mipgen_launch_candidates(hipStream_t, int n, const ListSrc&, const HostConsts*, const double* model, int n_sv, double gamma, double rho, int method, double* scores,
                                    uint64_t* records, double* features, mipgen_candidate_ints*, int literal, const unsigned int* n_dev);
// ... the dense grid as a list, the print-exact scan and its scatter, survivors as a list, long-range content
hipError_t mipgen_launch_dense_candidates(hipStream_t, const DevParams* P, const DevRegion* regions, int r0, int r1, int64_t c0, int n, mipgen_candidate* out);
hipError_t mipgen_launch_dense_list_fix(hipStream_t, int n, const uint64_t* records, double rho, double s_guard, double* scores);
hipError_t mipgen_launch_print_boundary_scan(hipStream_t, const DevParams*, const DevRegion*, const RescoreSrc*, double tol_rel, double tol_abs, mipgen_candidate* out,
                                             int64_t* out_idx, unsigned int* count, unsigned int cap, int n_cu);
hipError_t mipgen_launch_index_candidates(hipStream_t, const DevParams*, const DevRegion*, int r0, int r1, const int64_t* idx, const unsigned int* count, unsigned int cap,
                                          mipgen_candidate* out);
hipError_t mipgen_launch_scatter_scores(hipStream_t, const double* src, const int64_t* idx, int64_t cap, const unsigned int* n_dev, double* dst, mipgen_survivor* dst_surv,
                                        unsigned int* over);
hipError_t mipgen_launch_surv_keep(hipStream_t, const mipgen_survivor* surv, int64_t n, int64_t* keep, double* svr);
hipError_t mipgen_launch_surv_candidates(hipStream_t, const DevParams*, const DevRegion*, int r0, int r1, const mipgen_survivor* surv, int64_t n, int64_t cand0,
                                         const int64_t* offs, mipgen_candidate* out, int64_t* out_idx);
hipError_t mipgen_launch_long_range(hipStream_t, int n, const char* seqs, const int64_t* offs, const int32_t* lens, const int32_t* denoms, const LrcMers*, double* out);
// kernels_replay.hip: the consumers of the dense grid.  Replay + condense fold, one wavefront per scan position of the window's position map; the launcher picks
// k_replay_condense_carry<3|5|8> (<= 64 pairs, <= 8 sizes), _narrow<wide> (<= 64 pairs) or the chunked k_replay_condense from n_pairs and n_sizes_max
hipError_t mipgen_launch_replay_condense(hipStream_t, int total_pos, const DevParams*, int n_pairs, int n_sizes_max, const DevRegion*, const int32_t* pos_region,
                                         const int32_t* pos_local, const double* scores, const uint64_t* records, const int32_t* copy, int64_t cand_base, uint8_t* emitted,
                                         mipgen_survivor* survivors, unsigned long long* emitted_per_region);
hipError_t mipgen_launch_collapse(hipStream_t, int n_tiles, const CollapseTile* tiles, const DevParams*, const DevRegion*, const int64_t* region_pos0,
                                  const int64_t* region_base0, const mipgen_survivor* survivors, const int32_t* copy, int64_t cand_base, int32_t* collapsed, int max_scan_all);
hipError_t mipgen_launch_fill_pos_map(hipStream_t, const int64_t* region_pos0, int n_regions, int64_t total, int32_t* pos_region, int32_t* pos_local);
// kernels_format.hip
hipError_t mipgen_launch_fmt_count(hipStream_t, int64_t n_rb, int r0, const FmtConst*, const FmtRegion*, const DevParams*, const DevRegion*, const uint8_t* emitted,
                                   int64_t* cnt);
hipError_t mipgen_launch_fmt_records(hipStream_t, int write, int64_t n_rb, int r0, const FmtConst*, const FmtRegion*, const char* pool, const DevParams*, const DevRegion*,
                                     const char* letters, const int32_t* copy, const double* scores, const uint64_t* records, const uint8_t* emitted, const int64_t* rank0,
                                     const int64_t* off, int64_t* len_out, char* text);
hipError_t mipgen_scan_i64(hipStream_t, void* temp, size_t* temp_bytes, const int64_t* in, int64_t* out, int64_t n);   // exclusive sum; temp == nullptr: size query
// kernels_kmer.hip
hipError_t mipgen_launch_kmer_insert(hipStream_t, const char* seq, int64_t len, const KmerParams*, uint64_t* keys, uint32_t* filter);
hipError_t mipgen_launch_kmer_fold(hipStream_t, const uint32_t* filter, int filter_bits, uint32_t* folded);
hipError_t mipgen_launch_kmer_count(hipStream_t, const char* genome, int64_t len, const KmerParams*, const uint64_t* keys, const uint32_t* filter, const uint32_t* folded,
                                    unsigned int* counts, int n_cu);
hipError_t mipgen_launch_kmer_lookup(hipStream_t, const char* seq, int64_t len, const KmerParams*, const uint64_t* keys, const unsigned int* counts, int32_t* out);
hipError_t mipgen_launch_kmer_place(hipStream_t, const int32_t* src, int64_t len, const KmerParams*, const int64_t* roff, int n_regions, int32_t* dst, void* big,
                                    unsigned int* n_big, unsigned int big_cap);
// kernels_window.hip
hipError_t mipgen_launch_window_spans(hipStream_t st, const char* q, const int64_t* roff, int n_regions, uint16_t* dist_bad, uint16_t* dist_end, uint16_t* dist_start);
hipError_t mipgen_launch_seed_index(hipStream_t st, const char* q, int64_t total, int k, const uint64_t* keys, uint64_t cap_mask, unsigned int* rmult, unsigned int* rstart,
                                    unsigned int* rfill, uint32_t* rlist, unsigned int* alloc, int phase);
hipError_t mipgen_launch_window_verify(hipStream_t st, const char* G, int64_t glen, const char* q, int64_t total, const int32_t* sizes, int n_sizes, int k,
                                       const uint64_t* keys, uint64_t cap_mask, const unsigned int* counts, const uint32_t* filter, int filter_bits, const unsigned int* rmult,
                                       const unsigned int* rstart, const uint32_t* rlist, const uint16_t* dist_start, unsigned int* ctr);
hipError_t mipgen_launch_window_flags(hipStream_t st, const char* q, int64_t total, const int32_t* sizes, int n_sizes, int k, const uint64_t* keys, uint64_t cap_mask,
                                      const unsigned int* counts, const uint16_t* dist_bad, const uint16_t* dist_end, const unsigned int* ctr, uint8_t* unmap,
                                      const int64_t* roff, int n_regions, const int32_t* bounds, uint8_t* any);
// kernels_reads.hip (pairs [pair0, pair0 + n_pairs) of the uploaded chunk; assign is indexed by the pair's position in the chunk)
hipError_t mipgen_launch_read_assign(hipStream_t, const ReadsParams*, const ReadProbe* probes, const SeedTable* ext_seeds, const SeedTable* lig_seeds, int64_t pair0,
                                     int64_t n_pairs, const uint8_t* ext_bytes, const int64_t* ext_off, int64_t ext_base, const uint8_t* lig_bytes, const int64_t* lig_off,
                                     int64_t lig_base, int32_t* assign, unsigned long long* reads, uint64_t* keys, int64_t key_cap, ReadsCounters* ctr,
                                     const int32_t* row);        // row: nullptr, or the sample row of every pair of the chunk (counts and keys go to the cell row * n_probes + probe)
hipError_t mipgen_launch_sample_assign(hipStream_t, const SampleTable*, int64_t n_pairs, const uint8_t* idx_bytes, const int64_t* idx_off, int64_t idx_base, int32_t* row,
                                       int32_t* sample_index, unsigned long long* row_pairs, SampleCounters* sctr);
hipError_t mipgen_launch_reads_histogram(hipStream_t, const uint64_t* keys, int64_t n, unsigned long long* unique);
hipError_t mipgen_reads_sort_unique(hipStream_t, void* temp, size_t* temp_bytes, uint64_t* keys, uint64_t* alt, int64_t n, int end_bit, unsigned long long* n_out);
// kernels_consensus.hip (the hipCUB steps: temp == nullptr asks for the scratch size)
hipError_t mipgen_launch_member_keys(hipStream_t, const ReadsParams*, int64_t n_pairs, uint32_t pair0, const int32_t* assign, const int32_t* row, const uint8_t* ext_bytes,
                                     const int64_t* ext_off, int64_t ext_base, const uint8_t* lig_bytes, const int64_t* lig_off, int64_t lig_base, int64_t qdelta,
                                     uint64_t sentinel, uint64_t* keys, uint32_t* ids, ConsensusPair* recs, ConsensusCounters* cctr);
hipError_t mipgen_consensus_sort(hipStream_t, void* temp, size_t* temp_bytes, const uint64_t* keys_in, uint64_t* keys_out, const uint32_t* ids_in, uint32_t* ids_out, int64_t n,
                                 int end_bit);
hipError_t mipgen_consensus_runs(hipStream_t, void* temp, size_t* temp_bytes, const uint64_t* keys, int64_t n, uint64_t* group_keys, int32_t* family,
                                 unsigned long long* n_groups);
hipError_t mipgen_consensus_scan_u32(hipStream_t, void* temp, size_t* temp_bytes, const int32_t* family, uint32_t* group_start, int64_t n);
hipError_t mipgen_consensus_scan_i64(hipStream_t, void* temp, size_t* temp_bytes, const int64_t* len, int64_t* off, int64_t n);
hipError_t mipgen_launch_consensus_partition(hipStream_t, const int32_t* family, int64_t n_groups, uint32_t* order, ConsensusCounters* cctr);
hipError_t mipgen_launch_consensus_len(hipStream_t, int te, int tl, int64_t n_groups, const uint32_t* order, int64_t n_big, const uint32_t* group_start, const int32_t* family,
                                       const uint32_t* ids, const ConsensusPair* recs, int64_t* ext_len, int64_t* lig_len);
hipError_t mipgen_launch_consensus_vote(hipStream_t, int te, int tl, int64_t n_groups, const uint32_t* order, int64_t n_small, int64_t n_big, const uint32_t* group_start,
                                        const int32_t* family, const uint32_t* ids, const ConsensusPair* recs, const int64_t* ext_off, const int64_t* lig_off, uint8_t* ext_seq,
                                        uint8_t* ext_qual, uint8_t* lig_seq, uint8_t* lig_qual);
// kernels_tag_merge.hip (the rule and TagMergeCounters: tag_merge.h): the parent of every raw group, its root and the totals (ctr zero on entry), and the
// sorted pairs back into the unsorted arrays with every member key replaced by its root's
struct TagMergeCounters;
hipError_t mipgen_launch_tag_parent(hipStream_t, const uint64_t* keys, const int32_t* family, int64_t n_groups, int tag_bases, int32_t* parent);
hipError_t mipgen_launch_tag_root(hipStream_t, const int32_t* parent, const int32_t* family, int64_t n_groups, int32_t* root, TagMergeCounters* ctr);
hipError_t mipgen_launch_tag_rewrite(hipStream_t, const uint64_t* keys_sorted, const uint32_t* ids_sorted, int64_t n_pairs, int64_t n_members, const uint64_t* group_keys,
                                     int64_t n_groups, const int32_t* root, uint64_t* keys, uint32_t* ids);
// kernels_pileup.hip: the cell boundaries of one row, its (cell, round) units and its used groups (R: cell0, n, mol_len and min_family are read; start, units
// and ctr are written, ctr zero on entry); then the counts and their sums
hipError_t mipgen_launch_pileup_prepare(hipStream_t, const ConsensusView& C, const PileRow& R, int64_t n_units, uint32_t* start, uint2* units, PileupCounters* ctr);
hipError_t mipgen_launch_pileup(hipStream_t, const ConsensusView& C, const PileRow& R, int64_t n_units, int32_t* counts, PileupCounters* ctr);
// kernels_gapped.hip: the sides of one row that need the banded alignment; then the alignment, the counts with indels and their sums
size_t mipgen_gap_align_lds_bytes(int max_len, int W);
// (planes: 3 bytes per projected position, or 5 - the projection that also holds the run indices of DESIGN 4.16)
hipError_t mipgen_launch_gap_list(hipStream_t, const ConsensusView& C, const PileRow& R, const uint8_t* mol_seq, uint32_t g_first, int64_t n_row_groups, int max_indel,
                                  int planes, uint8_t* need, uint32_t* list, int64_t* proj_off, GappedCounters* ctr);
hipError_t mipgen_launch_gapped(hipStream_t, const ConsensusView& C, const PileRow& R, int64_t n_units, const uint8_t* mol_seq, uint32_t g_first, int max_indel, int max_len,
                                int planes, const uint32_t* list, int64_t n_sides, const int64_t* proj_off, uint8_t* proj, int32_t* counts, GappedCounters* ctr);
// insertion alleles: the anchor table and the events of a row from its five-plane projections; the runs of the sorted keys as records
hipError_t mipgen_launch_insertions(hipStream_t, const ConsensusView& C, const PileRow& R, int64_t n_units, uint32_t g_first, const int64_t* proj_off, const uint8_t* proj,
                                    int32_t* anchors, uint64_t* keys, int64_t cap, InsCounters* ctr);
hipError_t mipgen_launch_insertion_records(hipStream_t, const uint64_t* run_keys, const int32_t* run_counts, const unsigned long long* n_runs, int64_t cap,
                                           mipgen_insertion_record* records);
// deletion alleles: the sites table and the events of a row from its three-plane projections; the runs of the sorted keys as records
hipError_t mipgen_launch_deletions(hipStream_t, const ConsensusView& C, const PileRow& R, int64_t n_units, uint32_t g_first, const int64_t* proj_off, const uint8_t* proj,
                                   int32_t* sites, uint64_t* keys, int64_t cap, DelCounters* ctr);
hipError_t mipgen_launch_deletion_records(hipStream_t, const uint64_t* run_keys, const int32_t* run_counts, const unsigned long long* n_runs, int64_t cap, const int32_t* sites,
                                          int64_t n_pos, mipgen_deletion_record* records);
// kernels_call.hip: one row's table added into the pool (K[5], N[5] per position); the candidates of a table against the pool (cand: 4 n_pos records, ctr
// zero on entry); their scores, sort keys and ctr->calls; the calls in key order
hipError_t mipgen_launch_call_pool(hipStream_t, const int32_t* counts, int columns, int64_t n_pos, int32_t bg_max_ppm, int32_t* pool);
hipError_t mipgen_launch_call_flag(hipStream_t, const int32_t* counts, int columns, const int32_t* pool, const uint8_t* ref, int64_t n_pos, int own_row_is_sample,
                                   const CallModel& P, mipgen_call_record* cand, CallCounters* ctr);
hipError_t mipgen_launch_call_tail(hipStream_t, mipgen_call_record* cand, int64_t n_cand, int64_t n_pos, const CallModel& P, uint64_t* keys, uint32_t* ids, CallCounters* ctr);
hipError_t mipgen_launch_call_gather(hipStream_t, const mipgen_call_record* cand, const uint32_t* ids, int64_t n_cand, const CallCounters* ctr, mipgen_call_record* records);
// kernels_insertion_call.hip: one sample row's spans and non-ambiguous alleles into the sparse pool (S zero before the first row, ctr zero on entry; at most
// cap entries are written); the sums of the runs of the sorted entries; the candidates of a row's allele records against the pool (cand: n_records records, ctr zero
// on entry; a candidate's pos is its record's index); the calls joined with their allele records
hipError_t mipgen_launch_ins_pool_append(hipStream_t, const int32_t* anchors, int64_t n_pos, const mipgen_insertion_record* records, int64_t n_records, int32_t bg_max_ppm,
                                         int32_t* S, uint64_t* keys, InsPoolSums* sums, uint32_t* ids, int64_t cap, InsPoolCounters* ctr);
hipError_t mipgen_launch_ins_pool_reduce(hipStream_t, const int32_t* run_counts, const uint32_t* run_start, const unsigned long long* n_runs, int64_t n_entries,
                                         const uint32_t* ids_sorted, const InsPoolSums* entry_sums, InsPoolSums* pool_sums);
hipError_t mipgen_launch_ins_call_flag(hipStream_t, const mipgen_insertion_record* records, int64_t n_records, const int32_t* span, int span_stride, int64_t n_pos,
                                       const uint64_t* pool_keys, const InsPoolSums* pool_sums, int64_t n_pool, const int32_t* pool_span, int own_row_is_sample,
                                       const CallModel& P, mipgen_call_record* cand, CallCounters* ctr);
hipError_t mipgen_launch_ins_call_records(hipStream_t, const mipgen_call_record* calls, int64_t n_calls, const mipgen_insertion_record* records, int64_t n_records,
                                          mipgen_insertion_call_record* out);
// kernels_locus.hip: the (locus, x) pairs of a plan for the sort; src[n_pos] and first[n_loci + 1] from the sorted pairs; a count table folded into
// merged[n_loci][columns] and its totals (ctr zero on entry)
hipError_t mipgen_launch_locus_keys(hipStream_t, const int64_t* plan, int64_t n_pos, int64_t n_loci, uint64_t* keys, uint32_t* ids);
hipError_t mipgen_launch_locus_index(hipStream_t, const uint64_t* keys_sorted, const uint32_t* ids_sorted, const int64_t* plan, int64_t n_pos, int64_t n_loci, uint32_t* src,
                                     uint32_t* first);
hipError_t mipgen_launch_locus_merge(hipStream_t, const int32_t* counts, int columns, const uint32_t* src, const uint32_t* first, int64_t n_pos, int64_t n_loci,
                                     int32_t* merged, LocusCounters* ctr);
// kernels_locus_insertions.hip: own / prev of every anchor row from the sources of a plan (both GAP_LOCUS_NONE on entry); the (locus key, record index)
// pairs of a row's allele records (at most cap = 2 n_records; ctr zero on entry); the locus records of the runs of the sorted pairs; the anchor table folded into
// locus_anchors[n_loci][4] and its totals
hipError_t mipgen_launch_locus_anchor_map(hipStream_t, const uint32_t* src, const uint32_t* first, int64_t n_pos, int64_t n_loci, uint32_t* own, uint32_t* prev);
hipError_t mipgen_launch_locus_ins_fold(hipStream_t, const mipgen_insertion_record* records, int64_t n_records, const uint32_t* own, const uint32_t* prev, int64_t n_pos,
                                        uint64_t* keys, uint32_t* ids, int64_t cap, LocusInsCounters* ctr);
hipError_t mipgen_launch_locus_ins_reduce(hipStream_t, const uint64_t* run_keys, const int32_t* run_counts, const uint32_t* run_start, const unsigned long long* n_runs,
                                          int64_t n_pairs, const uint32_t* ids_sorted, const mipgen_insertion_record* records, int64_t n_records, mipgen_insertion_record* out);
hipError_t mipgen_launch_locus_anchor_merge(hipStream_t, const int32_t* anchors, const uint32_t* src, const uint32_t* first, int64_t n_pos, int64_t n_loci,
                                            int32_t* locus_anchors, LocusInsCounters* ctr);
}
