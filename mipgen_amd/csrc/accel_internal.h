// accel_internal.h — what the host-side translation units of libmipgen_accel.so share (the kernel launchers are in kernels.h): the error convention,
// device buffers, the handle (struct mipgen_accel) and the helpers that cross files.  accel.hip: lifecycle, model, region batch; accel_tiles.hip:
// tile lists of the scoring kernels; accel_score.hip: scoring / replay / collapse / record text / downloads; accel_kmer.hip: section 8f-3;
// accel_reads.hip: read sessions; accel_pileup.hip: the pileups read off the consensus reads a session leaves.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "kernels.h"
#include "logistic_device.h"

// ---- errors ----------------------------------------------------------------------------------------------
// (one buffer per calling thread, shared by the translation units of the library: accel.hip defines it)
extern thread_local char g_mipgen_accel_err[512];
#define g_err g_mipgen_accel_err
static inline int fail(int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}
#define HIP_TRY(expr)                                                                             \
    do {                                                                                          \
        hipError_t e__ = (expr);                                                                  \
        if (e__ != hipSuccess) return fail(MIPGEN_E_HIP, "%s: %s", #expr, hipGetErrorString(e__)); \
    } while (0)

// consecutive regions whose dense results share the result arrays at one time
struct Window {
    int r0 = 0, r1 = 0;              // regions [r0, r1)
    int64_t cand0 = 0, n_cand = 0;   // batch-wide candidate index of the first candidate; candidates
    int64_t pos0 = 0, n_pos = 0;     // batch-wide scan-position index; positions
    int log_tile0 = 0, n_log_tiles = 0, svr_tile0 = 0, n_svr_tiles = 0, col_tile0 = 0, n_col_tiles = 0, ld_tile0 = 0, n_ld_tiles = 0;
    int n_svr_few = 0;               // the LAST n_svr_few of the window's dense SVR tiles run with the few-sizes thread geometry (regions of one capture size)
    std::vector<int> lvl_tile0;      // dense SVR tiles by capture-size run: run l = svr_tiles_lvl[lvl_tile0[l], lvl_tile0[l + 1])
    int lvl0_few = 0;                // ... the last lvl0_few tiles of run 0 with the few-sizes geometry (such regions have one run)
    int64_t base0 = 0, n_base_entries = 0;   // collapsed entries (2 per base) of the window inside the batch-wide array
};

// Device buffers a handle has let go of, kept for its next allocations.  hipFree of tens of GB returns at once but the release is paid by
// a later hipMalloc (~60 ms per GB, tools/microbench/alloc_cost.hip: seconds for the k-mer tables of an exome); handing the blocks on -
// the counter's tables become the result arrays of the scoring calls - costs nothing.  Whole blocks only, best fit, at most 4x the request.
struct DevPool {
    struct Block { void* p; size_t bytes; };
    std::vector<Block> blocks;
    size_t held() const { size_t n = 0; for (const Block& b : blocks) n += b.bytes; return n; }
    void* take(size_t bytes, size_t* got)
    {
        int best = -1;
        for (int i = 0; i < (int)blocks.size(); i++)
            if (blocks[(size_t)i].bytes >= bytes && blocks[(size_t)i].bytes / 4 <= bytes && (best < 0 || blocks[(size_t)i].bytes < blocks[(size_t)best].bytes)) best = i;
        if (best < 0) return nullptr;
        void* p = blocks[(size_t)best].p;
        *got = blocks[(size_t)best].bytes;
        blocks.erase(blocks.begin() + best);
        return p;
    }
    void give(void* p, size_t bytes) { if (bytes >= ((size_t)1 << 20)) blocks.push_back({p, bytes}); else (void)hipFree(p); }   // small ones are not worth keeping
    void clear() { for (const Block& b : blocks) (void)hipFree(b.p); blocks.clear(); }
};

template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;
    DevPool* pool = nullptr;                 // where the buffer comes from / goes to (nullptr: hipMalloc / hipFree)
    int reserve(size_t n)
    {
        if (n <= cap) return 0;
        release();
        size_t want = n + std::min<size_t>(n / 8, (size_t)1 << 20) + 64;
        if (pool) {
            size_t got = 0;
            if (void* q = pool->take(want * sizeof(T), &got)) { p = (T*)q; cap = got / sizeof(T); return 0; }
        }
        hipError_t e = hipMalloc((void**)&p, want * sizeof(T));
        if (e != hipSuccess && pool && !pool->blocks.empty()) {        // out of memory with blocks in hand: give them back and try again
            (void)hipGetLastError();
            pool->clear();
            e = hipMalloc((void**)&p, want * sizeof(T));
        }
        if (e != hipSuccess) { p = nullptr; return fail(MIPGEN_E_NOMEM, "hipMalloc(%zu bytes): %s", want * sizeof(T), hipGetErrorString(e)); }
        cap = want;
        return 0;
    }
    void release()
    {
        if (p) { if (pool) pool->give(p, cap * sizeof(T)); else (void)hipFree(p); }
        p = nullptr; cap = 0;
    }
};
static inline size_t padded(size_t count, size_t size) { return (count + count / 8 + 64) * size; }      // (what DevBuf::reserve asks for at most)

// (key, id) pairs and their sorted copies, with the ONE scratch of mipgen_consensus_sort and of the runs and scans that follow it on the same pairs (kernels_consensus.hip).
// Whoever orders something on the device holds one of these: a budget takes bytes(), and every use is told the whole scratch, so no caller sees a temp_bytes.
struct SortedPairs {
    DevBuf<uint64_t> keys, keys_sorted;
    DevBuf<uint32_t> ids, ids_sorted;
    DevBuf<char> temp;
    size_t held() const { return (keys.cap + keys_sorted.cap) * 8 + (ids.cap + ids_sorted.cap) * 4 + temp.cap; }
    void release() { keys.release(); keys_sorted.release(); ids.release(); ids_sorted.release(); temp.release(); }
    static size_t bytes(size_t n, size_t scratch) { return 2 * padded(n, 8) + 2 * padded(n, 4) + padded(scratch, 1); }     // what reserve(n, scratch) asks for at most
    // *scratch: what a sort of n pairs over end_bit key bits takes and, on the same scratch, the runs of n_runs keys and a u32 scan over n_scan (0: not asked for); 1 at least
    static hipError_t scratch_bytes(hipStream_t st, int64_t n, int end_bit, int64_t n_runs, int64_t n_scan, size_t* scratch)
    {
        size_t t_sort = 0, t_runs = 0, t_scan = 0;
        hipError_t e = mipgen_consensus_sort(st, nullptr, &t_sort, nullptr, nullptr, nullptr, nullptr, n, end_bit);
        if (e == hipSuccess && n_runs) e = mipgen_consensus_runs(st, nullptr, &t_runs, nullptr, n_runs, nullptr, nullptr, nullptr);
        if (e == hipSuccess && n_scan) e = mipgen_consensus_scan_u32(st, nullptr, &t_scan, nullptr, nullptr, n_scan);
        *scratch = std::max<size_t>(std::max(t_sort, std::max(t_runs, t_scan)), 1);
        return e;
    }
    int reserve(size_t n, size_t scratch) { return keys.reserve(n) || keys_sorted.reserve(n) || ids.reserve(n) || ids_sorted.reserve(n) || temp.reserve(scratch) ? MIPGEN_E_NOMEM : MIPGEN_OK; }
    // keys / ids [0, n) into keys_sorted / ids_sorted, ascending by the low end_bit bits of the key; the runs of keys_sorted[0, n): the key and the length of each and their
    // number (keys and ids are free once sorted, and may take the first two); exclusive sums.  Each is told the whole scratch.
    hipError_t sort(hipStream_t st, int64_t n, int end_bit) { size_t all = temp.cap; return mipgen_consensus_sort(st, temp.p, &all, keys.p, keys_sorted.p, ids.p, ids_sorted.p, n, end_bit); }
    hipError_t runs(hipStream_t st, int64_t n, uint64_t* run_keys, int32_t* run_counts, unsigned long long* n_runs) { size_t all = temp.cap; return mipgen_consensus_runs(st, temp.p, &all, keys_sorted.p, n, run_keys, run_counts, n_runs); }
    hipError_t scan_u32(hipStream_t st, const int32_t* in, uint32_t* out, int64_t n) { size_t all = temp.cap; return mipgen_consensus_scan_u32(st, temp.p, &all, in, out, n); }
    hipError_t scan_i64(hipStream_t st, const int64_t* in, int64_t* out, int64_t n) { size_t all = temp.cap; return mipgen_consensus_scan_i64(st, temp.p, &all, in, out, n); }
};

// two pinned host chunks + their "copy finished" events: large tables cross PCIe as they are packed / unpacked, chunk by chunk
template <typename T>
struct PinnedPair {
    T* buf[2] = {nullptr, nullptr};
    hipEvent_t done[2] = {nullptr, nullptr};
    bool busy[2] = {false, false};
    hipError_t alloc(size_t n)
    {
        for (int b = 0; b < 2; b++) {
            hipError_t e = hipHostMalloc((void**)&buf[b], std::max<size_t>(n, 1) * sizeof(T), hipHostMallocDefault);
            if (e != hipSuccess) return e;
            e = hipEventCreateWithFlags(&done[b], hipEventDisableTiming);
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    }
    hipError_t wait(int b) { hipError_t e = busy[b] ? hipEventSynchronize(done[b]) : hipSuccess; busy[b] = false; return e; }
    ~PinnedPair() { for (int b = 0; b < 2; b++) { if (done[b]) { if (busy[b]) (void)hipEventSynchronize(done[b]); (void)hipEventDestroy(done[b]); } if (buf[b]) (void)hipHostFree(buf[b]); } }
};

// What of a result window is current (mipgen_accel::win_state, one byte per window).  The result arrays, the emitted mask and the record text
// hold one window at a time (cur_window); survivors, collapsed entries and survivor SVR scores are batch-wide and keep every window's slice.
enum : uint8_t {
    WIN_SURVIVORS = 1,               // survivors / emitted counts are of the scores the window got last (replay + condense ran on them)
    WIN_MASK = 2,                    // ... and that replay kept the per-candidate emitted mask
    WIN_COLLAPSED = 4,               // the collapsed entries are of those survivors
    WIN_SURV_SVR = 8,                // surv_svr holds the SVR scores of those survivors
    WIN_TEXT = 16,                   // fmt_text / fmt_bytes are the all_mips records of those scores
};

// scores picked out of the fast kernels' results for a second computation: the candidates, where each came from, the new values, how many
struct RescoreList {
    DevBuf<mipgen_candidate> cands; DevBuf<int64_t> idx; DevBuf<double> vals; DevBuf<unsigned int> count;
    void release() { cands.release(); idx.release(); vals.release(); count.release(); }
};

struct ReadsSession;                  // accel_reads.hip

// ---- the consensus reads a session leaves on the handle and the scratch of the two pileups read off them (accel_pileup.hip) ----
// what every count holds of one row: kept with the consensus reads between calls - a call per row would otherwise pay the allocations every time
struct RowScratch {
    DevBuf<int32_t> mol_len;                                 // n
    DevBuf<int64_t> pos_off;                                 // n
    DevBuf<uint32_t> start;                                  // n + 1
    DevBuf<uint2> units;                                     // the rounds of all probes
    DevBuf<PileupCounters> pctr;
    size_t held() const { return mol_len.cap * 4 + pos_off.cap * 8 + start.cap * 4 + units.cap * 8 + pctr.cap * sizeof(PileupCounters); }
    void release() { mol_len.release(); pos_off.release(); start.release(); units.release(); pctr.release(); }
};
// One counted row: the row's buffers and its table.  A count with indels reserves the alignment buffers too; the plain count leaves them unreserved.
// Every instance has its own buffers throughout, so that no entry point touches what another holds.
struct CountScratch {
    RowScratch row;
    DevBuf<int32_t> counts;                                  // positions x PILEUP_COLUMNS or GAPPED_COLUMNS
    DevBuf<int64_t> proj_off;                                // 2 x the row's groups
    DevBuf<uint32_t> list;                                   // the listed sides
    DevBuf<uint8_t> mol_seq, need, proj;                     // positions; 2 x the row's groups; the projections of the listed sides
    DevBuf<GappedCounters> ctr;
    size_t held() const { return row.held() + counts.cap * 4 + proj_off.cap * 8 + list.cap * 4 + mol_seq.cap + need.cap + proj.cap + ctr.cap * sizeof(GappedCounters); }
    void release() { row.release(); counts.release(); proj_off.release(); list.release(); mol_seq.release(); need.release(); proj.release(); ctr.release(); }
};
// The arguments a pool over the sample rows was built with: a call recomputes its row with them.  remember() is what a builder ends with (accel_pileup.hip, beside RowArgs)
struct RowArgs;
struct PoolArgs {
    bool have = false;                                       // a pool is held
    std::vector<int32_t> mol_len;
    std::string mol_seq;                                     // (empty: the pool was built without template bases)
    int32_t min_family = 1, min_quality = 0, max_indel = 0, bg_max_ppm = 0;
    void remember(const RowArgs& A, int64_t n_pos, int32_t bg_max_ppm_);
};
// A dense background pool, its arguments and the pileup totals of the row called last
struct PoolState : PoolArgs {
    DevBuf<int32_t> pool;                                    // positions or loci x (K[5], N[5])
    mipgen_gapped_totals last{0, 0, 0, 0, 0, 0, 0, 0};        // the pileup totals of the row called last
    bool have_last = false;
    void drop() { have = have_last = false; }
    void release() { drop(); pool.release(); }
};
// mipgen_accel_reads_consensus_call_pool / _consensus_call: the pool over the sample rows, the ref bytes and a count scratch of each kind of its own -
// the calls share nothing with `pile` / `gapped` of the two pileup entry points
struct CallScratch {
    CountScratch pile, gapped;
    PoolState state;
    DevBuf<uint8_t> ref;                                     // positions
    size_t held() const { return pile.held() + gapped.held() + state.pool.cap * 4 + ref.cap; }
    void release() { state.release(); pile.release(); gapped.release(); ref.release(); }
};
// what a call of either kind (mipgen_accel_call_tables too) leaves on the HANDLE: the candidate list, the sort's buffers and the ordered records of the last call
struct CallRun {
    DevBuf<mipgen_call_record> cand, records;                // 4 per position at most; the candidates of the call
    SortedPairs pairs;                                       // (key, slot) of every candidate
    DevBuf<CallCounters> ctr;
    DevBuf<int32_t> counts, pool;                            // the uploaded arrays of mipgen_accel_call_tables
    DevBuf<uint8_t> ref;
    int64_t n_calls = -1;                                    // the records of the last call (-1: none yet)
    size_t held() const { return (cand.cap + records.cap) * sizeof(mipgen_call_record) + pairs.held() + ctr.cap * sizeof(CallCounters) + (counts.cap + pool.cap) * 4 + ref.cap; }
    void release() { cand.release(); records.release(); pairs.release(); ctr.release(); counts.release(); pool.release(); ref.release(); n_calls = -1; }
};
// loci.  A plan on the device: src and first are what a merge reads; the rest is held only while the plan is built
struct LocusPlan {
    DevBuf<int64_t> plan;                                    // positions (transient)
    SortedPairs pairs;                                       // (locus, position) of every position (transient)
    DevBuf<uint32_t> src, first;                             // positions: x << 2 | flags in locus order; loci + 1
    int64_t n_pos = 0, n_loci = 0;
    bool have = false;
    size_t held() const { return plan.cap * 8 + pairs.held() + (src.cap + first.cap) * 4; }
    void release_transient() { plan.release(); pairs.release(); }
    void release() { release_transient(); src.release(); first.release(); have = false; n_pos = n_loci = 0; }
};
// what mipgen_accel_locus_tables leaves on the HANDLE: its plan and the uploaded and merged tables
struct LocusRun {
    LocusPlan plan;
    DevBuf<int32_t> counts, merged;
    DevBuf<LocusCounters> ctr;
    size_t held() const { return plan.held() + (counts.cap + merged.cap) * 4 + ctr.cap * sizeof(LocusCounters); }
    void release() { plan.release(); counts.release(); merged.release(); ctr.release(); }
};
// mipgen_accel_reads_consensus_locus_* : the installed plan and locus_ref, a count scratch of each kind of its own (no locus call touches what the pileup or call
// entry points hold), the merged table and the pool over the loci; released with the reads, as CallScratch
struct LocusScratch {
    LocusPlan plan;
    DevBuf<uint8_t> ref;                                     // loci
    CountScratch pile, gapped;
    DevBuf<int32_t> merged;                                  // loci x columns
    DevBuf<LocusCounters> ctr;
    PoolState state;
    size_t held() const { return plan.held() + ref.cap + pile.held() + gapped.held() + (merged.cap + state.pool.cap) * 4 + ctr.cap * sizeof(LocusCounters); }
    void release() { plan.release(); ref.release(); pile.release(); gapped.release(); merged.release(); ctr.release(); state.release(); }
};
// mipgen_accel_reads_consensus_insertions: a count scratch of its own - its projections have five planes -, the anchor table, the events and what
// orders them; released with the reads.  run keys and run counts take the place of pairs.keys and pairs.ids once the sort has read them.
struct InsScratch {
    CountScratch count;
    DevBuf<int32_t> anchors;                                 // positions x INSERTION_COLUMNS
    DevBuf<InsCounters> ctr;
    SortedPairs pairs;                                       // events (the sort moves pairs; nothing reads the ids)
    DevBuf<mipgen_insertion_record> records;                 // events at most
    int64_t n_alleles = -1;                                  // the records of the last call (-1: none, or it failed)
    size_t event_held() const { return pairs.held() + records.cap * sizeof(mipgen_insertion_record); }
    size_t table_held() const { return anchors.cap * 4 + ctr.cap * sizeof(InsCounters); }
    void release() { count.release(); anchors.release(); ctr.release(); pairs.release(); records.release(); n_alleles = -1; }
};
// mipgen_accel_reads_consensus_deletions: a count scratch of its own, the sites table, the events and what orders them; released with the reads.
// run keys and run counts take the place of pairs.keys and pairs.ids once the sort has read them.
struct DelScratch {
    CountScratch count;
    DevBuf<int32_t> sites;                                   // positions x DELETION_COLUMNS
    DevBuf<DelCounters> ctr;
    SortedPairs pairs;                                       // the deleted bases of the row: the events at most (the sort moves pairs; nothing reads the ids)
    DevBuf<mipgen_deletion_record> records;
    int64_t n_alleles = -1;                                  // the records of the last call (-1: none, or it failed)
    size_t event_held() const { return pairs.held() + records.cap * sizeof(mipgen_deletion_record); }
    size_t table_held() const { return sites.cap * 4 + ctr.cap * sizeof(DelCounters); }
    void release() { count.release(); sites.release(); ctr.release(); pairs.release(); records.release(); n_alleles = -1; }
};
// mipgen_accel_reads_consensus_insertion_pool: the sparse pool over the sample rows - S per position, keys and sums per distinct allele - and the
// arguments it was built with; the entries and what orders them are held only while the pool is built.  Released with the reads.
struct InsPool {
    PoolArgs args;
    DevBuf<int32_t> S;                                       // positions
    DevBuf<uint64_t> pool_keys;                              // distinct alleles, ascending
    DevBuf<InsPoolSums> pool_sums;
    DevBuf<InsPoolCounters> ctr;
    SortedPairs pairs;                                       // (key, index) of every entry (transient, as everything below)
    DevBuf<InsPoolSums> sums;
    DevBuf<uint32_t> run_start;
    DevBuf<int32_t> run_counts;
    int64_t n_pos = 0, rows = 0, n_entries = 0, n_alleles = 0;
    size_t entry_held() const { return pairs.held() + pool_keys.cap * 8 + (sums.cap + pool_sums.cap) * sizeof(InsPoolSums) + (run_start.cap + run_counts.cap) * 4; }
    size_t table_held() const { return S.cap * 4 + ctr.cap * sizeof(InsPoolCounters); }
    void release_transient() { pairs.release(); sums.release(); run_start.release(); run_counts.release(); }
    void release() { args.have = false; release_transient(); S.release(); pool_keys.release(); pool_sums.release(); ctr.release(); n_pos = rows = n_entries = n_alleles = 0; }
};
// what an insertion call of either kind (mipgen_accel_insertion_call_tables too) leaves on the HANDLE: a CallRun of its own - mipgen_accel_call_fetch keeps finding the
// last variant call -, the joined records, and the uploaded arrays of the tables call
struct InsCallRun {
    CallRun run;
    DevBuf<mipgen_insertion_call_record> out;
    DevBuf<mipgen_insertion_record> records;
    DevBuf<int32_t> span, pool_span;
    DevBuf<uint64_t> pool_keys;
    DevBuf<InsPoolSums> pool_sums;
    int64_t n_calls = -1;                                    // the records of the last insertion call (-1: none yet)
    size_t call_held() const { return run.held() + out.cap * sizeof(mipgen_insertion_call_record); }          // what run_ins_call fills
    size_t upload_held() const { return records.cap * sizeof(mipgen_insertion_record) + (span.cap + pool_span.cap) * 4 + pool_keys.cap * 8 + pool_sums.cap * sizeof(InsPoolSums); }
    void release() { run.release(); out.release(); records.release(); span.release(); pool_span.release(); pool_keys.release(); pool_sums.release(); n_calls = -1; }
};
// insertion alleles per locus.  What k_locus_anchor_map leaves of a plan: built on the first fold under it, dropped with it
struct LocusInsMap {
    DevBuf<uint32_t> own, prev;                              // positions each: locus << 2 | flags of the source that pulls the anchor row, or GAP_LOCUS_NONE
    bool have = false;
    size_t held() const { return (own.cap + prev.cap) * 4; }
    void release() { own.release(); prev.release(); have = false; }
};
// One folded row, on the HANDLE (the tables call and the session calls share it, as the calls share a CallRun): the (locus key, record index) pairs and what orders
// them - run keys and run counts take the place of pairs.keys and pairs.ids once the sort has read them -, the locus records and the locus anchor table
struct LocusInsFold {
    SortedPairs pairs;                                       // 2 x the row's records at most
    DevBuf<uint32_t> run_start;
    DevBuf<mipgen_insertion_record> records;                 // the locus records of the last fold
    DevBuf<int32_t> anchors;                                 // loci x INSERTION_COLUMNS
    DevBuf<LocusInsCounters> ctr;
    int64_t n_alleles = -1;                                  // the locus records of the last fold (-1: none, or it failed)
    size_t pair_held() const { return pairs.held() + run_start.cap * 4 + records.cap * sizeof(mipgen_insertion_record); }
    size_t table_held() const { return anchors.cap * 4 + ctr.cap * sizeof(LocusInsCounters); }
    void release() { pairs.release(); run_start.release(); records.release(); anchors.release(); ctr.release(); n_alleles = -1; }
};
// what mipgen_accel_locus_insertion_tables leaves on the HANDLE beside the fold: its plan, its map and the uploaded arrays
struct LocusInsRun {
    LocusPlan plan;
    LocusInsMap map;
    DevBuf<mipgen_insertion_record> records;
    DevBuf<int32_t> anchors;
    LocusInsFold fold;
    size_t upload_held() const { return records.cap * sizeof(mipgen_insertion_record) + anchors.cap * 4; }
    void release() { plan.release(); map.release(); records.release(); anchors.release(); fold.release(); }
};
// mipgen_accel_reads_consensus_locus_insertion*: the map of the installed plan and the sparse pool over the loci; released with the reads, dropped with the plan
struct LocusInsScratch {
    LocusInsMap map;
    InsPool pool;
    void drop() { map.have = false; pool.args.have = false; }
    void release() { map.release(); pool.release(); }
};
struct ConsensusResult {
    int64_t n_groups = 0, ext_bytes = 0, lig_bytes = 0;
    int64_t n = 0, rows = 0;                                 // probes and rows of the session that left the reads: a cell is row * n + probe
    CountScratch pile, gapped;                               // of mipgen_accel_reads_consensus_pileup and _pileup_gapped
    CallScratch call;
    LocusScratch locus;
    InsScratch ins;
    InsPool ins_pool;
    LocusInsScratch locus_ins;
    DelScratch del;
    DevBuf<uint64_t> keys;                              // (cell << 32) | tag of every group, ascending
    DevBuf<int32_t> family;
    DevBuf<int64_t> ext_off, lig_off;                        // n_groups + 1
    DevBuf<uint8_t> ext_seq, ext_qual, lig_seq, lig_qual;
    // the tag merge of the session that left the reads.  merged: the raw groups and the root of each are held; otherwise the map is the identity on `keys`
    // and `family` and nothing below is reserved
    mipgen_tag_merge_totals tag_totals{0, 0, 0, 0, 0};
    bool merged = false;
    DevBuf<uint64_t> raw_keys;                               // raw_groups
    DevBuf<int32_t> raw_family, raw_root;                    // ... the family of each and the raw group that is its root
    ConsensusView view() const { return {keys.p, family.p, ext_off.p, lig_off.p, ext_seq.p, ext_qual.p, lig_seq.p, lig_qual.p, n_groups}; }
    void release() { keys.release(); family.release(); ext_off.release(); lig_off.release(); ext_seq.release(); ext_qual.release(); lig_seq.release(); lig_qual.release(); raw_keys.release(); raw_family.release(); raw_root.release(); pile.release(); gapped.release(); call.release(); locus.release(); ins.release(); ins_pool.release(); locus_ins.release(); del.release(); }
};

struct mipgen_accel {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    mipgen_params params;
    DevParams hp;                    // host copy
    DevParams* dp = nullptr;
    HostConsts* dconsts = nullptr;
    HostConsts hconsts;
    SvrGeom geom;
    SvrGeom geom_few;                // thread geometry of the tiles of regions that keep one capture size: more, shorter arm-pair chunks
    bool have_few = false;           // (twice the chunks, half the lanes per chunk: such a tile fills a quarter of the main geometry's lanes)
    // model
    int n_sv = 0;
    double gamma = 0, rho = 0, s_guard = 0;
    DevBuf<double> model;
    std::string svr_geometry_error;  // why the dense SVR kernel cannot run this parameter set ("" = it can); reported when SVR is requested
    std::string svr_batch_error;     // same, for the resident batch (tile does not fit LDS)
    bool record_tiles_ready = false, logistic_tiles_ready = false, svr_tiles_ready = false;   // tile lists of the resident batch, laid out on first use
    int sv_split = 0;                // 0 = chosen per launch from the tile count; > 0 forced
    int ld_subruns = 0;              // position sub-runs per tile of the dense logistic kernel: 0 = from the batch size; 1..8 forced
    int n_cu = 256;
    // batch
    int n_regions = 0;
    int64_t n_cand = 0;
    int64_t total_pos = 0;
    std::vector<DevRegion> hregions;
    std::vector<mipgen_grid> grids;
    DevBuf<DevRegion> regions;
    DevBuf<uint8_t> bases, unmap;
    DevBuf<char> letters;                     // the region strings as given (record formatting prints them; `bases` keeps only classes)
    // device-side all_mips formatting (section 8f-4)
    DevBuf<FmtRegion> fmt_regions;
    DevBuf<char> fmt_pool, fmt_text, scan_temp;   // (scan_temp: scratch of device_scan_i64, whoever scans)
    DevBuf<int64_t> fmt_a, fmt_b, fmt_c, fmt_d;
    int64_t fmt_bytes = 0;                    // bytes in fmt_text (current while a window has WIN_TEXT)
    DevPool pool;                             // large buffers the handle let go of (see DevPool)
    DevBuf<int32_t> copy;
    std::vector<int32_t> resident_lens;      // seq_len of the regions whose copy tables mipgen_accel_count_oligo_copies_resident left in `copy`
    std::vector<mipgen_big_copy> big_copies; // ... and their counts >= 65535
    DevBuf<LogTile> log_tiles;
    DevBuf<SvrTile> svr_tiles, ld_tiles;      // dense SVR tiles; tiles of the table-based dense logistic kernel (same shape, own sizes)
    size_t ld_lds = 0;                        // 0: some region does not fit that kernel's LDS -> the per-candidate kernel scores the batch
    int log_span_max = 0;
    size_t svr_lds = 0;
    // result windows: the inputs of every region stay resident; the dense result arrays (16 B per candidate) hold one window of
    // consecutive regions at a time
    int64_t window_cap = 0;          // max candidates per window; 0 = as many as fit in free device memory
    std::vector<int32_t> window_breaks;   // batch indices at which a window must start (mipgen_accel_set_window_breaks), ascending
    std::vector<Window> windows;
    int cur_window = -1;             // the window whose scores / records are in the result arrays (-1: none scored since the upload)
    std::vector<uint8_t> win_state;  // WIN_* per window, sized with `windows`
    DevBuf<double> scores, partials;
    DevBuf<uint64_t> records;
    // replay
    DevBuf<uint8_t> emitted;
    DevBuf<mipgen_survivor> survivors;
    DevBuf<unsigned long long> emitted_per_region;
    DevBuf<int32_t> pos_region, pos_local;
    // collapse: per base and strand the scan-start index of the best survivor covering it
    std::vector<int64_t> h_region_base0;     // first collapsed entry of every region (batch-wide), + total at the end
    DevBuf<int64_t> region_pos0, region_base0;
    DevBuf<CollapseTile> col_tiles;
    DevBuf<int32_t> collapsed;
    // scores on a rounding boundary of the 6 printed digits are re-scored in the reference's operation order (rescore)
    bool print_exact = true;
    double sum_abs_coef = 0.0;
    RescoreList pb;
    // mixed designs: SVR score of every condensed survivor of the batch (mipgen_accel_rescore_survivors), slot for slot beside `survivors`
    DevBuf<double> surv_svr;
    DevBuf<int64_t> rs_keep, rs_offs, rs_idx;
    // logistic candidates whose b^x lies in [2^53, 2^54) - their score turns on the last bit of the reference's pow (kernels_logistic_dense.hip) - listed by the
    // dense kernel and re-scored in the reference's term order with the correctly rounded power before anything is replayed (rescore)
    RescoreList sat;
    // flag image of the last mipgen_accel_window_uniqueness_begin: uint8 [win_sizes][win_total], region r at column win_roff[r]
    DevBuf<uint8_t> win_img;
    std::vector<int64_t> win_roff;
    std::vector<int32_t> win_lens;
    int win_sizes = 0;
    int64_t win_total = 0;
    // dynamic skip between capture-size runs (kernels_skip.hip; mipgen_accel_set_dynamic_skip)
    bool dyn_skip = false;
    int svr_levels = 1;                      // capture-size runs of the region with the most of them (1: nothing to skip between)
    DevBuf<SvrTile> svr_tiles_lvl, svr_tiles_kept;
    DevBuf<uint32_t> run_bounds;             // [region][level]: first size index | sizes << 16
    DevBuf<double> run_pbs;                  // per scan position of the window: previous_best_score after the runs scored so far
    DevBuf<uint8_t> run_state;               // 0 still constructing, 1 stopped (mipgen.cpp:430), 2 too close to the limit to call
    DevBuf<int64_t> run_keep, run_offs;
    DevBuf<unsigned long long> skip_count;   // dense candidates of the tiles skipped since the last read
    unsigned long long skipped_total = 0;
    bool skip_count_valid = false;
    unsigned int* pb_over = nullptr;         // host-mapped word: entries a re-score list could not hold (checked at the next download: pb_check)
    DevBuf<double> model_t, sv_norm, sv_coef, sv_center;   // the model centred and transposed for the survivor-list scorer (kernels_svr_gemm.hip)
    int n_sv_pad = 0;
    double kmer_count_ms = -1.0;             // genome pass of the last mipgen_accel_count_oligo_copies
    double list_feat_ms = -1.0, list_svr_ms = -1.0;   // k_features_batch / k_svr_gemm of the last list call (timing enabled)
    int64_t kmer_genome_bytes = 0;
    // sparse scratch
    DevBuf<mipgen_candidate> cand_in;
    DevBuf<double> cand_scores, cand_feats;
    DevBuf<uint64_t> cand_records;
    DevBuf<mipgen_candidate_ints> cand_ints;
    // probes given by sequence (mipgen_accel_score_probes): descriptors, packed bytes, long-range rows, launch order
    DevBuf<ProbeRec> probe_recs;
    DevBuf<uint8_t> probe_bytes;
    DevBuf<double> probe_lrc;
    DevBuf<int32_t> probe_order;
    DevBuf<char> lrc_seq;
    DevBuf<double> lrc_out;
    DevBuf<int64_t> lrc_offs;
    DevBuf<int32_t> lrc_lens, lrc_denoms;
    // reads and unique tags per probe (accel_reads.hip): the open session owns its buffers; nothing else of the handle is touched by it
    ReadsSession* reads = nullptr;
    int64_t reads_key_cap = 0;       // mipgen_accel_reads_set_key_buffer (0: default)
    double reads_assign_ms = -1.0;   // k_read_assign over the feed calls of the last session (timing enabled)
    double sample_assign_ms = -1.0;  // k_sample_assign over the feed calls of the last samples session (timing enabled)
    ConsensusResult* consensus = nullptr;   // held from mipgen_accel_reads_finish_consensus until the next mipgen_accel_reads_open* or mipgen_accel_destroy
    double consensus_vote_ms = -1.0; // k_consensus_vote_wave + k_consensus_vote_wg of the last mipgen_accel_reads_finish_consensus (timing enabled)
    double consensus_sort_ms = -1.0; // ... its radix sort of (key, pair id) and the run boundaries (both sorts of a session that merges tags)
    double tag_merge_ms = -1.0;      // ... its k_tag_parent, k_tag_root and k_tag_rewrite (a session with tag mismatches 1, timing enabled)
    double pileup_ms = -1.0;         // the kernels_pileup.hip kernels of the last mipgen_accel_reads_consensus_pileup (timing enabled)
    double gapped_ms = -1.0;         // the kernels of the last mipgen_accel_reads_consensus_pileup_gapped (timing enabled)
    CallRun call_run;                // the last call's candidates and records (accel_pileup.hip)
    double call_ms = -1.0;           // the kernels of the last mipgen_accel_call_tables / _reads_consensus_call / _reads_consensus_call_pool (timing enabled)
    LocusRun locus_run;              // the plan and tables of the last mipgen_accel_locus_tables (accel_pileup.hip)
    double locus_ms = -1.0;          // the kernels of the last locus call of any kind, its pileup included (timing enabled)
    double insertions_ms = -1.0;     // the kernels of the last mipgen_accel_reads_consensus_insertions (timing enabled)
    InsCallRun ins_call;             // the last insertion call's candidates and records (accel_pileup.hip)
    double ins_call_ms = -1.0;       // the kernels of the last insertion pool or insertion call of either kind (timing enabled)
    LocusInsRun locus_ins;           // the last fold of insertion alleles to loci, its records and locus anchor table (accel_pileup.hip)
    InsCallRun locus_ins_call;       // the last insertion call per locus: a run of its own, so that mipgen_accel_insertion_call_fetch keeps finding the last call per probe
    double locus_ins_ms = -1.0;      // the kernels of the last locus insertions call of any kind, the insertions route of its rows included (timing enabled)
    double deletions_ms = -1.0;      // the kernels of the last mipgen_accel_reads_consensus_deletions (timing enabled)
    // timing: four events per window (records | svr | replay), summed over the windows of the last call
    bool timing = false;
    std::vector<hipEvent_t> ev;
    std::vector<uint8_t> ev_used;    // per window: bit 0 scored, bit 1 replayed in the last call
};

// ---- small helpers ----------------------------------------------------------------------------------------
static inline int n_sizes_all(const mipgen_params& P)
{
    if (P.max_capture_size < P.min_capture_size) return 0;
    return (P.max_capture_size - P.min_capture_size) / P.capture_increment + 1;
}

static inline void grid_of(const mipgen_params& P, const DevParams& D, const mipgen_region& R, mipgen_grid* g)
{
    // positions: mipgen.cpp:421-425; static size skip: mipgen.cpp:429
    int cur = R.start_flanked - P.max_capture_size + (P.arm_sum_key_max > 0 ? P.arm_sum_key_max : D.max_sum);   // (:421 uses the largest KEY of the arm-sum map)
    if (cur < 0) cur = 0;
    g->first_pos = cur + 1;
    g->n_pos = std::max(0, R.stop_flanked - cur);
    int K = D.n_sizes_all, k0 = 0;
    while (k0 < K) {
        int C = P.max_capture_size - k0 * P.capture_increment;
        if (C > R.stop_flanked - R.start_flanked + P.max_mip_overlap && C - P.capture_increment >= P.min_capture_size) k0++;
        else break;
    }
    g->first_size_index = k0;
    g->n_sizes = K - k0;
    g->count = (int64_t)g->n_pos * g->n_sizes * P.n_arm_pairs * 2;
    g->offset = 0;
}

static inline bool win_has(const mipgen_accel* h, int w, uint8_t bits) { return w >= 0 && (h->win_state[(size_t)w] & bits) == bits; }   // (w = cur_window may be -1)
static inline void win_set(mipgen_accel* h, int w, uint8_t bits) { h->win_state[(size_t)w] |= bits; }

static inline uint8_t base_code(char c)
{
    switch (c) {
        case 'A': return BASE_A; case 'C': return BASE_C; case 'G': return BASE_G; case 'T': return BASE_T;
        case 'N': return BASE_N; case '-': return BASE_DASH; default: return BASE_OTHER;
    }
}

#ifdef MIPGEN_DIAG
struct DiagClock {                           // host seconds per stage of a call, on stderr (diagnostic builds only)
    const char* what; std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    explicit DiagClock(const char* w) : what(w) {}
    void lap(const char* stage) { const auto n_ = std::chrono::steady_clock::now(); fprintf(stderr, "[mipgen_accel] %s: %s %.3f s\n", what, stage, std::chrono::duration<double>(n_ - t).count()); t = n_; }
};
#define DIAG_CLOCK(name) DiagClock diag_clock(name)
#define DIAG_LAP(stage) diag_clock.lap(stage)
#else
#define DIAG_CLOCK(name) do { } while (0)
#define DIAG_LAP(stage) do { } while (0)
#endif

// ---- what the read sessions and the pileups share of a call's plumbing ----
static inline int free_device_bytes(size_t* free_b)
{
    size_t total_b = 0;
    HIP_TRY(hipMemGetInfo(free_b, &total_b));
    return MIPGEN_OK;
}
// the stream is idle when the scope ends, however it ends: the caller's arrays and the host tables behind an asynchronous copy are free from then on
struct IdleOnExit { hipStream_t s; bool idle = false; hipError_t wait() { idle = true; return hipStreamSynchronize(s); } ~IdleOnExit() { if (!idle) (void)hipStreamSynchronize(s); } };

// HIP-event time of spans of the stream when timing is on (off: no event is ever created).  mark() before and after a span; add_to(), called once the stream is idle and the
// call has succeeded, adds the ms of every span to *sum and says how many it added; the destructor destroys the events.
struct SpanTimer {
    bool on;
    hipStream_t st;
    std::vector<hipEvent_t> ev;                              // (before, after) of every span
    ~SpanTimer() { for (hipEvent_t e : ev) (void)hipEventDestroy(e); }
    void mark() { hipEvent_t e = nullptr; if (on && (on = hipEventCreate(&e) == hipSuccess)) { ev.push_back(e); (void)hipEventRecord(e, st); } }
    int add_to(double* sum) const
    {
        int n = 0;
        float ms = 0.f;
        for (size_t k = 0; on && k + 1 < ev.size(); k += 2)
            if (hipEventElapsedTime(&ms, ev[k], ev[k + 1]) == hipSuccess) { *sum += ms; n++; }
        return n;
    }
};

// ---- helpers that cross translation units ----------------------------------------------------------------------
extern "C" {
int mipgen_pick_sv_split(int n_tiles, int n_sv, int n_cu);       // accel_tiles.hip
int mipgen_ensure_events(mipgen_accel* h);
int mipgen_ensure_tiles(mipgen_accel* h, int32_t method);
int mipgen_pb_check(mipgen_accel* h);                            // accel_score.hip
void mipgen_reads_release(mipgen_accel* h);                      // accel_reads.hip: closes an open read-counting session
void mipgen_consensus_release(mipgen_accel* h);                  // accel_reads.hip: lets go of the consensus reads the handle holds
}
