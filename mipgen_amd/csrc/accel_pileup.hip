// accel_pileup.hip — the two pileups read off the consensus reads a session left on the handle: allele counts per template position of one row (DESIGN 4.12:
// mipgen_accel_reads_consensus_pileup) and the same with indels (4.13: _consensus_pileup_gapped), the variant calls made from them (4.14: mipgen_accel_call_tables,
// _reads_consensus_call_pool, _reads_consensus_call, _call_fetch) and the same per genome locus (4.15: mipgen_accel_locus_tables, _reads_consensus_locus_plan /
// _locus_pileup / _locus_call_pool / _locus_call), and the insertion alleles of a row (4.16: mipgen_accel_reads_consensus_insertions, mipgen_accel_insertions_fetch) and their calls against a sparse pool over the sample rows (4.17: mipgen_accel_insertion_call_tables,
// _reads_consensus_insertion_pool, _insertion_pool_fetch, _reads_consensus_insertion_call, _insertion_call_fetch) and, folded to genome loci by the installed plan between
// the insertions of a row and its pool or call (4.19: mipgen_accel_locus_insertion_tables, _locus_insertions_fetch, _reads_consensus_locus_insertions / _locus_insertion_pool /
// _locus_insertion_call, _locus_insertion_pool_fetch, _locus_insertion_call_fetch: fold_insertions is the one fold), and the deletion alleles of a row (4.21:
// mipgen_accel_reads_consensus_deletions, mipgen_accel_deletions_fetch, counting into the DelScratch of the ConsensusResult).  The arguments of a row travel as one RowArgs.  plan_row makes every check of them (nothing allocated or launched);
// count_row is the ONE count: the budget, prepare_row (the row's buffers, the cell boundaries and the (cell, round) units: a filled PileRow), the launches of the plain
// or the gapped table, download and totals of one row into the CountScratch it is given.  Every entry point gives a scratch of its own - `pile` / `gapped` of the
// ConsensusResult, of its CallScratch, of its LocusScratch, of its InsScratch - so no call touches what another holds.  A pool and a call are one route each (build_pool, call_row) over
// a Target: per template position, or per locus, where count_target folds the row's table by the installed plan (kernels_locus.hip) between the count and the pool
// or run_call.  An entry point is its own refusals, its budget and one call of the shared route.  Whatever is ordered on the device - candidates, plan positions, insertion
// events, pool entries - lies in the SortedPairs of its struct, and what a pool was built with in a PoolArgs (both accel_internal.h).
#include "accel_internal.h"
#include "gapped_align.h"

// The arguments of a row, as every level takes them.  need_seq: the call refuses a NULL mol_seq; must_place: it places with indels whatever max_indel says (the gapped
// pileup, which so refuses max_indel 0); otherwise a row is placed when max_indel is not 0.  runs: the projections take five planes, the run indices of DESIGN 4.16 in the
// last two.
struct RowArgs {
    const char* mol_seq; const int32_t* mol_len; int32_t n, min_family, min_quality, max_indel;
    bool need_seq = false, must_place = false, runs = false;
    bool placed() const { return must_place || max_indel != 0; }
    int planes() const { return runs ? 5 : 3; }
};

void PoolArgs::remember(const RowArgs& A, int64_t n_pos, int32_t bg_max_ppm_)
{
    mol_len.assign(A.mol_len, A.mol_len + A.n);
    if (A.mol_seq) mol_seq.assign(A.mol_seq, (size_t)n_pos); else mol_seq.clear();     // (the dense pool without indels may be built without template bases)
    min_family = A.min_family; min_quality = A.min_quality; max_indel = A.max_indel; bg_max_ppm = bg_max_ppm_;
    have = true;
}

struct RowPlan {
    ConsensusResult* R = nullptr;
    int64_t n_pos = 0, n_units = 0;                                      // template positions; rounds of 64 of them
    int32_t max_len = 0;
    size_t bytes = 0;                                                    // the device memory RowScratch takes at most
};

// what a call may take: the bytes it holds already and the free ones
static int room_beside(size_t held, size_t* room)
{
    size_t free_b = 0;
    if (int rc = free_device_bytes(&free_b)) return rc;
    *room = held + free_b;
    return MIPGEN_OK;
}

// the end of a call that succeeded, its stream idle: the spans of `timer` into *ms when timing is on
static int booked(const SpanTimer& timer, double* ms)
{
    double sum = 0.0;
    if (timer.add_to(&sum)) *ms = sum;
    return MIPGEN_OK;
}

// the two refusals every call that reads the session begins with
static int check_reads(const mipgen_accel* h)
{
    if (!h) return fail(MIPGEN_E_INVALID, "null handle");
    if (!h->consensus) return fail(MIPGEN_E_STATE, "the handle holds no consensus reads: mipgen_accel_reads_finish_consensus leaves them, the next mipgen_accel_reads_open* drops them");
    return MIPGEN_OK;
}

// Every refusal of a row, in one order for all callers; placed molecules are bounded by MIPGEN_GAPPED_MAX_MOL.
static int plan_row(mipgen_accel* h, const RowArgs& A, int32_t row, RowPlan* P)
{
    if (int rc = check_reads(h)) return rc;
    const ConsensusResult* R = P->R = h->consensus;
    if (!A.mol_len) return fail(MIPGEN_E_INVALID, "bad arguments: no molecule lengths");
    if (A.need_seq && !A.mol_seq) return fail(MIPGEN_E_INVALID, "bad arguments: no template bases");
    if ((int64_t)A.n != R->n) return fail(MIPGEN_E_INVALID, "%d molecule lengths: the session that left the consensus reads had %lld probes", A.n, (long long)R->n);
    for (int32_t p = 0; p < A.n; p++) {
        if (A.mol_len[p] < 1) return fail(MIPGEN_E_INVALID, "molecule length %d of probe %d: a length is 1 or more", A.mol_len[p], p);
        if (A.placed() && A.mol_len[p] > MIPGEN_GAPPED_MAX_MOL)
            return fail(MIPGEN_E_INVALID, "molecule length %d of probe %d: the gapped pileup places molecules of at most %d bases", A.mol_len[p], p, MIPGEN_GAPPED_MAX_MOL);
        P->n_pos += A.mol_len[p]; P->n_units += ((int64_t)A.mol_len[p] + 63) / 64; P->max_len = std::max(P->max_len, A.mol_len[p]);
    }
    if (row < 0 || (int64_t)row >= R->rows) return fail(MIPGEN_E_INVALID, "row %d: the session had %lld row%s", row, (long long)R->rows, R->rows == 1 ? "" : "s");
    if (A.min_family < 1) return fail(MIPGEN_E_INVALID, "min_family %d: 1 or more", A.min_family);
    if (A.min_quality < 0 || A.min_quality > 40) return fail(MIPGEN_E_INVALID, "min_quality %d: 0 to 40 (the consensus writes 2 to 40)", A.min_quality);
    if (A.placed() && (A.max_indel < 1 || A.max_indel > GAP_MAX_INDEL)) return fail(MIPGEN_E_INVALID, "max_indel %d: 1 to %d", A.max_indel, GAP_MAX_INDEL);
    if (P->n_units > 0x7fffffff) return fail(MIPGEN_E_INVALID, "%lld template positions: more than 2^31 - 1 rounds of 64", (long long)P->n_pos);
    const size_t n = (size_t)A.n;
    P->bytes = padded(n, 4) + padded(n, 8) + padded(n + 1, 4) + padded((size_t)P->n_units, 8) + padded(1, sizeof(PileupCounters));
    HIP_TRY(hipSetDevice(h->device));
    return MIPGEN_OK;
}

// The row's buffers filled and its kernels run (timed as one span of `timer`): *row is complete, *pc holds `used`, [*first, *last) are the row's groups.
// what: the call's name in a message.
static int prepare_row(mipgen_accel* h, const RowPlan& P, RowScratch& W, const char* what, const RowArgs& A, int32_t row, SpanTimer& timer, PileRow* out,
                       PileupCounters* pc, uint32_t* first, uint32_t* last)
{
    const ConsensusResult* R = P.R;
    const size_t n = (size_t)A.n;
    if (W.mol_len.reserve(n) || W.pos_off.reserve(n) || W.start.reserve(n + 1) || W.units.reserve((size_t)P.n_units) || W.pctr.reserve(1)) return MIPGEN_E_NOMEM;
    std::vector<int64_t> pos_off(n);
    for (int64_t p = 0, at = 0; p < A.n; at += A.mol_len[p], p++) pos_off[(size_t)p] = at;
    hipStream_t st = h->stream;
    IdleOnExit idle{st};                                                 // (pos_off outlives its copy)
    HIP_TRY(hipMemcpyAsync(W.mol_len.p, A.mol_len, n * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(W.pos_off.p, pos_off.data(), n * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(W.pctr.p, 0, sizeof(PileupCounters), st));
    *out = {W.units.p, 0, 0, W.start.p, W.mol_len.p, W.pos_off.p, A.n, P.n_pos, (uint32_t)((int64_t)row * R->n), A.min_family, A.min_quality};
    timer.mark();
    HIP_TRY(mipgen_launch_pileup_prepare(st, R->view(), *out, P.n_units, W.start.p, W.units.p, W.pctr.p));
    timer.mark();
    HIP_TRY(hipMemcpyAsync(pc, W.pctr.p, sizeof *pc, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(first, W.start.p, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(last, W.start.p + A.n, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(idle.wait());
    out->n_small = (int64_t)pc->n_small; out->n_big = (int64_t)pc->n_big;
    if (out->n_small + out->n_big != P.n_units)
        return fail(MIPGEN_E_STATE, "%s: %lld + %lld rounds listed of %lld", what, (long long)out->n_small, (long long)out->n_big, (long long)P.n_units);
    return MIPGEN_OK;
}

// What a call adds to the budget of the row it counts: the bytes it will still allocate beside the row's, and what it already holds of them.  what: the call's name.
struct Budget { const char* what; size_t more_need = 0, more_held = 0; bool keep_on_device = false; };   // keep_on_device: a session without groups still leaves a zeroed table in W.counts
// a counted table on the device and its columns; of a row that launched (have_row), its plan and its first group: what a further pass over the row's projections needs
struct Counted { const int32_t* table = nullptr; int columns = 0; bool have_row = false; PileRow row{}; uint32_t g_first = 0; };

// One row counted into W: the plain table at max_indel 0, else the one with indels (4.13).  W.counts holds it afterwards - *out says so -, `counts` (may
// be NULL) a copy, *totals (may be NULL) its sums, the gapped-only ones 0 for the plain table; the kernels are spans of `timer`.
static int count_row(mipgen_accel* h, const RowPlan& P, CountScratch& W, const Budget& B, const RowArgs& A, int32_t row, SpanTimer& timer, int32_t* counts,
                     mipgen_gapped_totals* totals, Counted* out)
{
    const ConsensusResult* R = P.R;
    hipStream_t st = h->stream;
    const bool gapped = A.max_indel != 0;
    const int columns = gapped ? GAPPED_COLUMNS : PILEUP_COLUMNS;
    const size_t n_pos = (size_t)P.n_pos, cells = n_pos * (size_t)columns;
    GappedCounters gc;
    memset(&gc, 0, sizeof gc);
    if (R->n_groups == 0) {                                              // (no buffer exists: nothing to read, nothing to launch)
        if (counts) memset(counts, 0, cells * sizeof(int32_t));
        if (totals) *totals = mipgen_gapped_totals{};
        if (B.keep_on_device) {
            if (W.counts.reserve(cells)) return MIPGEN_E_NOMEM;
            HIP_TRY(hipMemsetAsync(W.counts.p, 0, cells * sizeof(int32_t), st));
            HIP_TRY(hipStreamSynchronize(st));
        }
        *out = {W.counts.p, columns};
        return MIPGEN_OK;
    }
    // the budget, before anything is allocated: the row's groups are not known yet, so every gapped buffer that grows with them is taken at the session's groups, and a
    // projection at the longest template
    const size_t G = (size_t)R->n_groups;
    size_t need = P.bytes + padded(cells, 4) + B.more_need, room = 0;
    if (gapped)
        need += padded(n_pos, 1) + padded(2 * G, 8) + padded(2 * G, 4) + padded(2 * G, 1) + padded(2 * G * (size_t)A.planes() * (size_t)P.max_len, 1) + padded(1, sizeof(GappedCounters));
    if (int rc = room_beside(W.held() + B.more_held, &room)) return rc;
    if (need > room && gapped)
        return fail(MIPGEN_E_NOMEM, "%s: %lld template positions and %lld groups need up to %zu MiB of device memory, %zu MiB are free", B.what, (long long)P.n_pos,
                    (long long)R->n_groups, need >> 20, room >> 20);
    if (need > room)
        return fail(MIPGEN_E_NOMEM, "%s: %lld template positions need %zu MiB of device memory, %zu MiB are free", B.what, (long long)P.n_pos, need >> 20, room >> 20);
    if (W.counts.reserve(cells) || (gapped && (W.mol_seq.reserve(n_pos) || W.ctr.reserve(1)))) return MIPGEN_E_NOMEM;
    IdleOnExit idle{st};
    if (gapped) {
        HIP_TRY(hipMemcpyAsync(W.mol_seq.p, A.mol_seq, n_pos, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemsetAsync(W.ctr.p, 0, sizeof(GappedCounters), st));
    }
    PileRow Row;
    PileupCounters pc;
    uint32_t first = 0, last = 0;                                        // the row's groups: [first, last)
    if (int rc = prepare_row(h, P, W.row, B.what, A, row, timer, &Row, &pc, &first, &last)) return rc;
    const ConsensusView C = R->view();
    const int64_t n_row = (int64_t)last - (int64_t)first;
    if (!gapped) {
        timer.mark();
        HIP_TRY(mipgen_launch_pileup(st, C, Row, P.n_units, W.counts.p, W.row.pctr.p));
        timer.mark();
        HIP_TRY(hipMemcpyAsync(&pc, W.row.pctr.p, sizeof pc, hipMemcpyDeviceToHost, st));
    } else {
        if (n_row < 0 || n_row > R->n_groups) return fail(MIPGEN_E_STATE, "%s: groups [%u, %u) of %lld", B.what, first, last, (long long)R->n_groups);
        if (n_row > 0) {
            if (W.need.reserve(2 * (size_t)n_row) || W.list.reserve(2 * (size_t)n_row) || W.proj_off.reserve(2 * (size_t)n_row)) return MIPGEN_E_NOMEM;
            timer.mark();
            HIP_TRY(mipgen_launch_gap_list(st, C, Row, W.mol_seq.p, first, n_row, A.max_indel, A.planes(), W.need.p, W.list.p, W.proj_off.p, W.ctr.p));
            timer.mark();
            HIP_TRY(hipMemcpyAsync(&gc, W.ctr.p, sizeof gc, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            if ((int64_t)gc.n_sides > 2 * n_row || gc.proj_bytes > (unsigned long long)gc.n_sides * (unsigned long long)A.planes() * (unsigned long long)P.max_len)
                return fail(MIPGEN_E_STATE, "%s: %llu sides listed of %lld, %llu projection bytes", B.what, gc.n_sides, (long long)(2 * n_row), gc.proj_bytes);
            if (gc.proj_bytes && W.proj.reserve((size_t)gc.proj_bytes)) return MIPGEN_E_NOMEM;
        }
        timer.mark();
        HIP_TRY(mipgen_launch_gapped(st, C, Row, P.n_units, W.mol_seq.p, first, A.max_indel, P.max_len, A.planes(), W.list.p, (int64_t)gc.n_sides, W.proj_off.p, W.proj.p, W.counts.p, W.ctr.p));
        timer.mark();
        HIP_TRY(hipMemcpyAsync(&gc, W.ctr.p, sizeof gc, hipMemcpyDeviceToHost, st));
    }
    if (counts) HIP_TRY(hipMemcpyAsync(counts, W.counts.p, cells * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(idle.wait());
    if (!gapped) { gc.bases = pc.bases; gc.discordant = pc.discordant; } // (the plain kernels sum into the row's own counters; every other sum stays 0)
    if (totals)
        *totals = {n_row, (int64_t)pc.used, (int64_t)gc.bases, (int64_t)gc.discordant, (int64_t)gc.deletions, (int64_t)gc.insertions, (int64_t)gc.ins_discordant,
                   (int64_t)gc.gapped_sides};
    *out = {W.counts.p, columns, true, Row, first};
    return MIPGEN_OK;
}

// ---- variant calls ---------------------------------------------------------------------------------------------------------------------------
static int check_bg_max_ppm(int32_t bg_max_ppm)
{
    if (bg_max_ppm < 0 || bg_max_ppm > 1000000) return fail(MIPGEN_E_INVALID, "bg_max_ppm %d: 0 to 1000000", bg_max_ppm);
    return MIPGEN_OK;
}

static int check_call_params(const mipgen_call_params* p)
{
    if (!p) return fail(MIPGEN_E_INVALID, "bad arguments: no call parameters");
    if (p->min_depth < 1) return fail(MIPGEN_E_INVALID, "min_depth %d: 1 or more", p->min_depth);
    if (p->min_alt < 1) return fail(MIPGEN_E_INVALID, "min_alt %d: 1 or more", p->min_alt);
    if (p->min_ppm < 0 || p->min_ppm > 1000000) return fail(MIPGEN_E_INVALID, "min_ppm %d: 0 to 1000000", p->min_ppm);
    if (p->min_q < 0 || p->min_q > CALL_Q_CAP) return fail(MIPGEN_E_INVALID, "min_q %d: 0 to %d", p->min_q, CALL_Q_CAP);
    if (!(p->a0 > 0 && p->a0 < p->n0 && p->n0 <= (1 << 30))) return fail(MIPGEN_E_INVALID, "prior %d / %d: 0 < a0 < n0 <= 2^30", p->a0, p->n0);
    return check_bg_max_ppm(p->bg_max_ppm);
}

// what flag, tail, sort and gather of at most max_cand candidates (4 per position; every record of an insertion call) take at the worst: the list, the ordered
// records, two (key, slot) pairs per candidate and the sort's own scratch (measured at 1/16 of the sort's bytes, taken at 1/4)
static size_t call_run_bytes(int64_t max_cand)
{
    const size_t c = (size_t)max_cand;
    return 2 * padded(c, sizeof(mipgen_call_record)) + SortedPairs::bytes(c, c * 6) + padded(1, sizeof(CallCounters));
}

// What every call shares from its flag kernel to its ordered records, in the CallRun U it is given: `flag` lists the candidates (at most max_cand; their pos below
// n_keys) into U.cand and counts them in U.ctr, then one read of the candidate count, tail, sort, gather.  The stream is idle and U.n_calls set on success.
template <typename Flag>
static int run_flagged(mipgen_accel* h, CallRun& U, int64_t n_keys, int64_t max_cand, const CallModel& M, SpanTimer& timer, mipgen_call_totals* totals, Flag flag)
{
    U.n_calls = -1;
    if (U.cand.reserve((size_t)max_cand) || U.ctr.reserve(1)) return MIPGEN_E_NOMEM;
    hipStream_t st = h->stream;
    IdleOnExit idle{st};
    CallCounters cc;
    HIP_TRY(hipMemsetAsync(U.ctr.p, 0, sizeof cc, st));
    timer.mark();
    HIP_TRY(flag(U.cand.p, U.ctr.p));
    timer.mark();
    HIP_TRY(hipMemcpyAsync(&cc, U.ctr.p, sizeof cc, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const int64_t n_cand = (int64_t)cc.candidates;
    if (n_cand < 0 || n_cand > max_cand) return fail(MIPGEN_E_STATE, "call: %lld candidates listed of %lld positions", (long long)n_cand, (long long)n_keys);
    if (n_cand > 0) {
        int end_bit = 4;                                                 // the bits of the sentinel n_keys << 3, the largest key
        while (end_bit < 64 && (((uint64_t)n_keys << 3) >> end_bit)) end_bit++;
        size_t scratch = 0;
        HIP_TRY(SortedPairs::scratch_bytes(st, n_cand, end_bit, 0, 0, &scratch));
        if (U.pairs.reserve((size_t)n_cand, scratch) || U.records.reserve((size_t)n_cand)) return MIPGEN_E_NOMEM;
        timer.mark();
        HIP_TRY(mipgen_launch_call_tail(st, U.cand.p, n_cand, n_keys, M, U.pairs.keys.p, U.pairs.ids.p, U.ctr.p));
        HIP_TRY(U.pairs.sort(st, n_cand, end_bit));
        HIP_TRY(mipgen_launch_call_gather(st, U.cand.p, U.pairs.ids_sorted.p, n_cand, U.ctr.p, U.records.p));
        timer.mark();
        HIP_TRY(hipMemcpyAsync(&cc, U.ctr.p, sizeof cc, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(idle.wait());
    if ((int64_t)cc.calls > n_cand) return fail(MIPGEN_E_STATE, "call: %llu calls of %lld candidates", cc.calls, (long long)n_cand);
    U.n_calls = (int64_t)cc.calls;
    if (totals) *totals = {(int64_t)cc.tested, (int64_t)cc.too_deep, n_cand, (int64_t)cc.calls};
    return MIPGEN_OK;
}

static CallModel model_of(const mipgen_call_params& prm) { return {prm.min_depth, prm.min_alt, prm.min_ppm, prm.min_q, prm.a0, prm.n0, prm.bg_max_ppm}; }

// The calls of one finished table on the device against pool and ref there, into h->call_run: k_call_flag, then the shared tail.
static int run_call(mipgen_accel* h, const int32_t* counts, int columns, const int32_t* pool, const uint8_t* ref, int64_t n_pos, bool own_row_is_sample,
                    const mipgen_call_params& prm, SpanTimer& timer, mipgen_call_totals* totals)
{
    const CallModel M = model_of(prm);
    hipStream_t st = h->stream;
    return run_flagged(h, h->call_run, n_pos, 4 * n_pos, M, timer, totals, [&](mipgen_call_record* cand, CallCounters* ctr) {
        return mipgen_launch_call_flag(st, counts, columns, pool, ref, n_pos, own_row_is_sample ? 1 : 0, M, cand, ctr);
    });
}

// the sample rows of a session: all but the last (undetermined) when it had barcodes, the one row otherwise
static int64_t sample_rows(const ConsensusResult* R) { return R->rows > 1 ? R->rows - 1 : 1; }

// ---- loci ------------------------------------------------------------------------------------------------------------------------------------
// every refusal of a plan
static int check_locus_plan(const int64_t* plan, int64_t n_pos, int64_t n_loci)
{
    if (!plan) return fail(MIPGEN_E_INVALID, "bad arguments: no locus plan");
    if (n_loci < 1 || n_loci > MIPGEN_CALL_MAX_POSITIONS) return fail(MIPGEN_E_INVALID, "%lld loci: 1 to 2^29 - 1", (long long)n_loci);
    if (n_pos < 1 || n_pos > MIPGEN_CALL_MAX_POSITIONS) return fail(MIPGEN_E_INVALID, "%lld positions: 1 to 2^29 - 1", (long long)n_pos);
    for (int64_t x = 0; x < n_pos; x++) {
        const int64_t e = plan[x];
        if (e < -1) return fail(MIPGEN_E_INVALID, "locus plan entry %lld of position %lld: -1 or locus * 4 + flags", (long long)e, (long long)x);
        if (e >= 0 && (e >> 2) >= n_loci) return fail(MIPGEN_E_INVALID, "locus %lld of position %lld: the plan has %lld loci", (long long)(e >> 2), (long long)x, (long long)n_loci);
        if (e >= 0 && (e & 2) && x == 0) return fail(MIPGEN_E_INVALID, "locus plan entry %lld of position 0: bit 1 takes the insertion columns of row x - 1", (long long)e);
    }
    return MIPGEN_OK;
}

static int locus_end_bit(int64_t n_loci)                                 // the bits of the sentinel n_loci, the largest key
{
    int end_bit = 1;
    while (end_bit < 64 && ((uint64_t)n_loci >> end_bit)) end_bit++;
    return end_bit;
}

// A checked plan onto the device (timed as one span of `timer`): the budget - the plan, the pairs with the sort's scratch, src and first, and
// `more_need` bytes the caller allocates next, against what is held and free - before anything is allocated; then keys, sort, sources and first.  The stream is idle
// and only src and first are still held on success.  what: the call's name.
static int build_locus_plan(mipgen_accel* h, LocusPlan& L, const int64_t* plan, int64_t n_pos, int64_t n_loci, size_t more_need, size_t more_held, const char* what,
                            SpanTimer& timer)
{
    hipStream_t st = h->stream;
    const size_t np = (size_t)n_pos, nl = (size_t)n_loci;
    const int end_bit = locus_end_bit(n_loci);
    size_t scratch = 0, room = 0;
    HIP_TRY(SortedPairs::scratch_bytes(st, n_pos, end_bit, 0, 0, &scratch));
    const size_t need = padded(np, 8) + SortedPairs::bytes(np, scratch) + padded(np, 4) + padded(nl + 1, 4) + more_need;
    if (int rc = room_beside(L.held() + more_held, &room)) return rc;
    if (need > room)
        return fail(MIPGEN_E_NOMEM, "%s: a plan of %lld positions and %lld loci needs up to %zu MiB of device memory, %zu MiB are free", what, (long long)n_pos,
                    (long long)n_loci, need >> 20, room >> 20);
    L.have = false;
    if (L.plan.reserve(np) || L.pairs.reserve(np, scratch) || L.src.reserve(np) || L.first.reserve(nl + 1)) return MIPGEN_E_NOMEM;
    IdleOnExit idle{st};                                                 // (the caller's plan outlives its copy)
    HIP_TRY(hipMemcpyAsync(L.plan.p, plan, np * 8, hipMemcpyHostToDevice, st));
    timer.mark();
    HIP_TRY(mipgen_launch_locus_keys(st, L.plan.p, n_pos, n_loci, L.pairs.keys.p, L.pairs.ids.p));
    HIP_TRY(L.pairs.sort(st, n_pos, end_bit));
    HIP_TRY(mipgen_launch_locus_index(st, L.pairs.keys_sorted.p, L.pairs.ids_sorted.p, L.plan.p, n_pos, n_loci, L.src.p, L.first.p));
    timer.mark();
    HIP_TRY(idle.wait());
    L.release_transient();
    L.n_pos = n_pos; L.n_loci = n_loci; L.have = true;
    return MIPGEN_OK;
}

// One table on the device folded into merged[n_loci][columns] there (reserved by the caller, as ctr) and summed: a span of `timer`; out (may be NULL) a copy, totals
// (may be NULL) the sums.  The stream is idle on return.
static int merge_loci(mipgen_accel* h, const LocusPlan& L, const int32_t* counts, int columns, int32_t* merged, LocusCounters* ctr, SpanTimer& timer, int32_t* out,
                      mipgen_locus_totals* totals)
{
    hipStream_t st = h->stream;
    IdleOnExit idle{st};
    LocusCounters lc;
    HIP_TRY(hipMemsetAsync(ctr, 0, sizeof lc, st));
    timer.mark();
    HIP_TRY(mipgen_launch_locus_merge(st, counts, columns, L.src.p, L.first.p, L.n_pos, L.n_loci, merged, ctr));
    timer.mark();
    HIP_TRY(hipMemcpyAsync(&lc, ctr, sizeof lc, hipMemcpyDeviceToHost, st));
    if (out) HIP_TRY(hipMemcpyAsync(out, merged, (size_t)L.n_loci * (size_t)columns * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(idle.wait());
    if (totals)
        *totals = {(int64_t)lc.covered, (int64_t)lc.bases, (int64_t)lc.discordant, (int64_t)lc.deletions, (int64_t)lc.insertions, (int64_t)lc.ins_discordant};
    return MIPGEN_OK;
}

// what the locus calls of a session share after plan_row: a plan is installed and is of this table
static int check_locus_session(const LocusScratch& L, const RowPlan& P)
{
    if (!L.plan.have) return fail(MIPGEN_E_STATE, "the consensus reads have no locus plan: mipgen_accel_reads_consensus_locus_plan installs it");
    if (P.n_pos != L.plan.n_pos)
        return fail(MIPGEN_E_INVALID, "%lld template positions: the locus plan was installed for %lld", (long long)P.n_pos, (long long)L.plan.n_pos);
    return MIPGEN_OK;
}

// Where a pool or a call puts the rows it counts: per template position - the scratch, pool and ref bytes of the CallScratch - or, with L set, per locus: every
// counted table is folded by L->plan into L->merged, and pool, ref bytes and run_call are over the loci.  ms: the timing index the route writes.
struct Target {
    CountScratch &pile, &gapped;
    PoolState& S;
    LocusScratch* L;
    const DevBuf<uint8_t>& ref;
    double* ms;
    int64_t n_out(const RowPlan& P) const { return L ? L->plan.n_loci : P.n_pos; }      // the rows of the table a pool adds up and a call tests
};
static Target probe_target(mipgen_accel* h, ConsensusResult* R) { return {R->call.pile, R->call.gapped, R->call.state, nullptr, R->call.ref, &h->call_ms}; }
static Target locus_target(mipgen_accel* h, ConsensusResult* R) { return {R->locus.pile, R->locus.gapped, R->locus.state, &R->locus, R->locus.ref, &h->locus_ms}; }

// One row counted into the target's scratch of the kind A asks for (probe_counts: a copy, may be NULL; pt: the pileup's totals, may be NULL) and, per locus, folded
// into L->merged (locus_counts, lt likewise).  *out: the table the pool or the call reads.
static int count_target(mipgen_accel* h, const RowPlan& P, const Target& T, const Budget& B, const RowArgs& A, int32_t row, SpanTimer& timer, int32_t* probe_counts,
                        int32_t* locus_counts, mipgen_gapped_totals* pt, mipgen_locus_totals* lt, Counted* out)
{
    if (int rc = count_row(h, P, A.max_indel ? T.gapped : T.pile, B, A, row, timer, probe_counts, pt, out)) return rc;
    if (!T.L) return MIPGEN_OK;
    const int32_t* counted = out->table;
    out->table = T.L->merged.p;
    return merge_loci(h, T.L->plan, counted, out->columns, T.L->merged.p, T.L->ctr.p, timer, locus_counts, lt);
}

// The pool of a target over the sample rows of the session: every row counted (and folded) and added on the device, then the arguments remembered for the calls.
// The caller has made its refusals, dropped the pool that was held, taken the budget B and reserved and filled what is its own.
static int build_pool(mipgen_accel* h, const RowPlan& P, const Target& T, const Budget& B, const RowArgs& A, int32_t bg_max_ppm)
{
    PoolState& S = T.S;
    const int64_t n_out = T.n_out(P);
    hipStream_t st = h->stream;
    IdleOnExit idle{st};
    HIP_TRY(hipMemsetAsync(S.pool.p, 0, (size_t)n_out * 40, st));
    SpanTimer timer{h->timing, st};
    for (int64_t r = 0; r < sample_rows(P.R); r++) {
        Counted row;
        if (int rc = count_target(h, P, T, B, A, (int32_t)r, timer, nullptr, nullptr, nullptr, nullptr, &row)) return rc;
        timer.mark();
        HIP_TRY(mipgen_launch_call_pool(st, row.table, row.columns, n_out, bg_max_ppm, S.pool.p));
        timer.mark();
    }
    HIP_TRY(idle.wait());
    S.remember(A, P.n_pos, bg_max_ppm);
    return booked(timer, T.ms);
}

// What a call of one row against the pool of a target shares up to its refusals of the row and the parameters: the row planned with the pool's arguments.
// pool_name: "pool" or "locus pool", as the message names it.
static int plan_call(mipgen_accel* h, const PoolArgs& S, int32_t row, const mipgen_call_params* params, const char* pool_name, RowArgs* A, RowPlan* P)
{
    *A = {S.mol_seq.data(), S.mol_len.data(), (int32_t)S.mol_len.size(), S.min_family, S.min_quality, S.max_indel};
    if (int rc = plan_row(h, *A, row, P)) return rc;
    if (int rc = check_call_params(params)) return rc;
    if (params->bg_max_ppm != S.bg_max_ppm) return fail(MIPGEN_E_STATE, "bg_max_ppm %d: the %s was built with %d", params->bg_max_ppm, pool_name, S.bg_max_ppm);
    return MIPGEN_OK;
}

// The calls of one row against the pool of a target: the row recomputed with the pool's arguments (and folded), then flag, tail and order.  what: the call's name.
static int call_row(mipgen_accel* h, const RowPlan& P, const Target& T, const RowArgs& A, const char* what, int32_t row, const mipgen_call_params& prm,
                    int32_t* probe_counts, int32_t* locus_counts, mipgen_call_totals* totals)
{
    PoolState& S = T.S;
    const int64_t n_out = T.n_out(P);
    *T.ms = -1.0;
    h->call_run.n_calls = -1;
    const Budget B{what, call_run_bytes(4 * n_out), h->call_run.held(), true};
    SpanTimer timer{h->timing, h->stream};
    S.have_last = false;
    Counted counted;
    if (int rc = count_target(h, P, T, B, A, row, timer, probe_counts, locus_counts, &S.last, nullptr, &counted)) return rc;
    S.have_last = true;
    if (int rc = run_call(h, counted.table, counted.columns, S.pool.p, T.ref.p, n_out, (int64_t)row < sample_rows(P.R), prm, timer, totals)) return rc;
    return booked(timer, T.ms);
}

// the pileup totals of the row a target's call counted last; none: the refusal's text
static int last_pileup_totals(mipgen_accel* h, bool locus, const char* none, mipgen_gapped_totals* totals)
{
    if (!h) return fail(MIPGEN_E_INVALID, "null handle");
    const PoolState* S = !h->consensus ? nullptr : locus ? &h->consensus->locus.state : &h->consensus->call.state;
    if (!S || !S->have_last) return fail(MIPGEN_E_STATE, "%s", none);
    if (totals) *totals = S->last;
    return MIPGEN_OK;
}


// ---- insertion alleles and their calls (4.17) ---------------------------------------------------------------------------------------------------
// every refusal of a row whose insertions are asked for: A has need_seq, must_place and runs set
static int plan_insertions(mipgen_accel* h, const RowArgs& A, int32_t row, RowPlan* P)
{
    if (int rc = plan_row(h, A, row, P)) return rc;
    if (P->n_pos > MIPGEN_CALL_MAX_POSITIONS) return fail(MIPGEN_E_INVALID, "%lld template positions: the insertion alleles take 2^29 - 1 at most", (long long)P->n_pos);
    return MIPGEN_OK;
}

// The insertion alleles of one planned row into R->ins, the kernels spans of `timer`: the gapped count with five-plane projections, then - the events being its
// `insertions` total - the anchor table and the events in one pass of the count frame, the keys sorted, their runs, and a record per run.  The anchor table and the
// S.n_alleles records stay on the device (a session without groups leaves neither, and 0 records).  Reads R's groups and reads; writes R->ins only.
static int insertions_row(mipgen_accel* h, const RowPlan& P, const RowArgs& A, int32_t row, SpanTimer& timer, int32_t* counts, int32_t* anchors,
                          mipgen_insertion_totals* totals)
{
    InsScratch& S = P.R->ins;
    S.n_alleles = -1;
    const size_t np = (size_t)P.n_pos, cells = np * INSERTION_COLUMNS;
    hipStream_t st = h->stream;
    mipgen_gapped_totals gt;
    Counted counted;
    const Budget B{"insertions", padded(cells, 4) + padded(1, sizeof(InsCounters)), S.table_held()};
    if (int rc = count_row(h, P, S.count, B, A, row, timer, counts, &gt, &counted)) return rc;
    if (!counted.have_row) {                                             // (a session without groups: nothing was launched)
        if (anchors) memset(anchors, 0, cells * sizeof(int32_t));
        if (totals) *totals = mipgen_insertion_totals{};
        S.n_alleles = 0;
        return MIPGEN_OK;
    }
    const int64_t events = gt.insertions;
    if (events < 0 || events > 0x7fffffff) return fail(MIPGEN_E_INVALID, "insertions: %lld events in row %d: 2^31 - 1 at most", (long long)events, row);
    // the events' bytes, known only now: checked before they are allocated
    const size_t ne = (size_t)events;
    if (events > 0) {
        size_t scratch = 0, room = 0;
        HIP_TRY(SortedPairs::scratch_bytes(st, events, 64, events, 0, &scratch));
        const size_t need = SortedPairs::bytes(ne, scratch) + padded(ne, sizeof(mipgen_insertion_record));
        if (int rc = room_beside(S.event_held(), &room)) return rc;
        if (need > room)
            return fail(MIPGEN_E_NOMEM, "insertions: %lld events need %zu MiB of device memory, %zu MiB are free", (long long)events, need >> 20, room >> 20);
        if (S.pairs.reserve(ne, scratch) || S.records.reserve(ne)) return MIPGEN_E_NOMEM;
    }
    if (S.anchors.reserve(cells) || S.ctr.reserve(1)) return MIPGEN_E_NOMEM;
    IdleOnExit idle{st};
    InsCounters ic;
    HIP_TRY(hipMemsetAsync(S.ctr.p, 0, sizeof ic, st));
    if (events > 0) HIP_TRY(hipMemsetAsync(S.pairs.ids.p, 0, ne * 4, st));
    const CountScratch& W = S.count;
    timer.mark();
    HIP_TRY(mipgen_launch_insertions(st, P.R->view(), counted.row, P.n_units, counted.g_first, W.proj_off.p, W.proj.p, S.anchors.p, S.pairs.keys.p, events, S.ctr.p));
    timer.mark();
    HIP_TRY(hipMemcpyAsync(&ic, S.ctr.p, sizeof ic, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if ((int64_t)ic.events != events || (int64_t)ic.insertions != events || (int64_t)ic.ins_discordant != gt.ins_discordant)
        return fail(MIPGEN_E_STATE, "insertions: %llu events emitted and %llu counted of %lld, %llu discordant of %lld", ic.events, ic.insertions, (long long)events,
                    ic.ins_discordant, (long long)gt.ins_discordant);
    if (events > 0) {
        timer.mark();
        int32_t* run_counts = reinterpret_cast<int32_t*>(S.pairs.ids.p);
        HIP_TRY(S.pairs.sort(st, events, 64));
        HIP_TRY(S.pairs.runs(st, events, S.pairs.keys.p, run_counts, &S.ctr.p->alleles));
        HIP_TRY(mipgen_launch_insertion_records(st, S.pairs.keys.p, run_counts, &S.ctr.p->alleles, events, S.records.p));
        timer.mark();
        HIP_TRY(hipMemcpyAsync(&ic, S.ctr.p, sizeof ic, hipMemcpyDeviceToHost, st));
    }
    if (anchors) HIP_TRY(hipMemcpyAsync(anchors, S.anchors.p, cells * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(idle.wait());
    if ((int64_t)ic.alleles > events || (events > 0 && ic.alleles == 0)) return fail(MIPGEN_E_STATE, "insertions: %llu alleles of %lld events", ic.alleles, (long long)events);
    S.n_alleles = (int64_t)ic.alleles;
    if (totals) *totals = {gt.groups, gt.used, (int64_t)ic.span, events, (int64_t)ic.ins_discordant, (int64_t)ic.ambiguous, S.n_alleles, gt.gapped_sides};
    return MIPGEN_OK;
}

// ---- deletion alleles ------------------------------------------------------------------------------------------------------------------------------
// The deletion alleles of one planned row into R->del, the kernels spans of `timer`: the gapped count with three-plane projections, then - the events being bounded by
// its `deletions` total, the deleted bases - the sites table and the events in one pass of the count frame, the keys sorted, their runs, and a record per run.  The
// sites table and the S.n_alleles records stay on the device (a session without groups leaves neither, and 0 records).  Reads R's groups and reads; writes R->del only.
static int deletions_row(mipgen_accel* h, const RowPlan& P, const RowArgs& A, int32_t row, SpanTimer& timer, int32_t* counts, int32_t* sites, mipgen_deletion_totals* totals)
{
    DelScratch& S = P.R->del;
    S.n_alleles = -1;
    const size_t np = (size_t)P.n_pos, cells = np * DELETION_COLUMNS;
    hipStream_t st = h->stream;
    mipgen_gapped_totals gt;
    Counted counted;
    const Budget B{"deletions", padded(cells, 4) + padded(1, sizeof(DelCounters)), S.table_held()};
    if (int rc = count_row(h, P, S.count, B, A, row, timer, counts, &gt, &counted)) return rc;
    if (!counted.have_row) {                                             // (a session without groups: nothing was launched)
        if (sites) memset(sites, 0, cells * sizeof(int32_t));
        if (totals) *totals = mipgen_deletion_totals{};
        S.n_alleles = 0;
        return MIPGEN_OK;
    }
    const int64_t cap = gt.deletions;                                    // every event holds one deleted base at least
    if (cap < 0 || cap > 0x7fffffff) return fail(MIPGEN_E_INVALID, "deletions: %lld deleted bases in row %d bound its events: 2^31 - 1 at most", (long long)cap, row);
    // the events' bytes, known only now: checked before they are allocated
    const size_t ne = (size_t)cap;
    if (cap > 0) {
        size_t scratch = 0, room = 0;
        HIP_TRY(SortedPairs::scratch_bytes(st, cap, 64, cap, 0, &scratch));
        const size_t need = SortedPairs::bytes(ne, scratch) + padded(ne, sizeof(mipgen_deletion_record));
        if (int rc = room_beside(S.event_held(), &room)) return rc;
        if (need > room)
            return fail(MIPGEN_E_NOMEM, "deletions: up to %lld events need %zu MiB of device memory, %zu MiB are free", (long long)cap, need >> 20, room >> 20);
        if (S.pairs.reserve(ne, scratch) || S.records.reserve(ne)) return MIPGEN_E_NOMEM;
    }
    if (S.sites.reserve(cells) || S.ctr.reserve(1)) return MIPGEN_E_NOMEM;
    IdleOnExit idle{st};
    DelCounters dc;
    HIP_TRY(hipMemsetAsync(S.ctr.p, 0, sizeof dc, st));
    if (cap > 0) HIP_TRY(hipMemsetAsync(S.pairs.ids.p, 0, ne * 4, st));
    const CountScratch& W = S.count;
    timer.mark();
    HIP_TRY(mipgen_launch_deletions(st, P.R->view(), counted.row, P.n_units, counted.g_first, W.proj_off.p, W.proj.p, S.sites.p, S.pairs.keys.p, cap, S.ctr.p));
    timer.mark();
    HIP_TRY(hipMemcpyAsync(&dc, S.ctr.p, sizeof dc, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const int64_t events = (int64_t)dc.events;
    if (dc.events > (unsigned long long)cap || (int64_t)dc.length_sum != cap || (int64_t)dc.deleted != cap || dc.starts != dc.events)
        return fail(MIPGEN_E_STATE, "deletions: %llu events emitted and %llu counted, %llu bases in them and %llu counted of %lld", dc.events, dc.starts, dc.length_sum,
                    dc.deleted, (long long)cap);
    if (events > 0) {
        timer.mark();
        int32_t* run_counts = reinterpret_cast<int32_t*>(S.pairs.ids.p);
        HIP_TRY(S.pairs.sort(st, events, 64));
        HIP_TRY(S.pairs.runs(st, events, S.pairs.keys.p, run_counts, &S.ctr.p->alleles));
        HIP_TRY(mipgen_launch_deletion_records(st, S.pairs.keys.p, run_counts, &S.ctr.p->alleles, events, S.sites.p, P.n_pos, S.records.p));
        timer.mark();
        HIP_TRY(hipMemcpyAsync(&dc, S.ctr.p, sizeof dc, hipMemcpyDeviceToHost, st));
    }
    if (sites) HIP_TRY(hipMemcpyAsync(sites, S.sites.p, cells * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(idle.wait());
    if ((int64_t)dc.alleles > events || (events > 0 && dc.alleles == 0)) return fail(MIPGEN_E_STATE, "deletions: %llu alleles of %lld events", dc.alleles, (long long)events);
    S.n_alleles = (int64_t)dc.alleles;
    if (totals) *totals = {gt.groups, gt.used, (int64_t)dc.depth, cap, events, (int64_t)dc.ragged, S.n_alleles, gt.gapped_sides};
    return MIPGEN_OK;
}

// the first `used` elements of b kept while it grows to `want` (DevBuf::reserve lets go of what it held)
template <typename T>
static int grow_keeping(DevBuf<T>& b, size_t used, size_t want, hipStream_t st)
{
    if (want <= b.cap) return MIPGEN_OK;
    DevBuf<T> bigger;
    bigger.pool = b.pool;
    if (bigger.reserve(want)) return MIPGEN_E_NOMEM;
    if (used) {
        const hipError_t e = hipMemcpyAsync(bigger.p, b.p, used * sizeof(T), hipMemcpyDeviceToDevice, st);
        const hipError_t w = hipStreamSynchronize(st);
        if (e != hipSuccess || w != hipSuccess) { bigger.release(); return fail(MIPGEN_E_HIP, "hipMemcpyAsync of %zu pool entries: %s", used, hipGetErrorString(e != hipSuccess ? e : w)); }
    }
    b.release();
    b = bigger;
    return MIPGEN_OK;
}

// what one entry of the pool takes while the pool is built beside its sorted pairs: its sums, and of its run the key, the sums, the length and the start
static const size_t INS_POOL_ENTRY_BYTES = 8 + 2 * sizeof(InsPoolSums) + 2 * 4;

// The sparse pool over the sample rows: the insertions route of every sample row, its spans added into S and its non-ambiguous records appended as entries;
// then the entries sorted by key, their runs - the distinct alleles - and the sums of every run.  The caller has made its refusals and dropped the pool that was held.
// The pool Q is over n_out anchor rows: the template positions, or the loci, where row_of - which runs the insertions route of sample row r and says
// where its anchor table and its n_rec records lie on the device - folds the row too.  what: the pool as a message names it.
template <typename RowOf>
static int build_ins_pool(mipgen_accel* h, const RowPlan& P, const RowArgs& A, int32_t bg_max_ppm, SpanTimer& timer, InsPool& Q, int64_t n_out, const char* what, RowOf row_of)
{
    InsScratch& I = P.R->ins;
    hipStream_t st = h->stream;
    const size_t np = (size_t)n_out;
    size_t room = 0;
    if (int rc = room_beside(Q.table_held(), &room)) return rc;
    if (padded(np, 4) + padded(1, sizeof(InsPoolCounters)) > room)
        return fail(MIPGEN_E_NOMEM, "%s: %lld template positions need %zu MiB of device memory beside the insertions', %zu MiB are free", what, (long long)n_out,
                    (padded(np, 4) + padded(1, sizeof(InsPoolCounters))) >> 20, room >> 20);
    if (Q.S.reserve(np) || Q.ctr.reserve(1)) return MIPGEN_E_NOMEM;
    IdleOnExit idle{st};
    HIP_TRY(hipMemsetAsync(Q.S.p, 0, np * 4, st));
    HIP_TRY(hipMemsetAsync(Q.ctr.p, 0, sizeof(InsPoolCounters), st));
    InsPoolCounters pc{0, 0};
    int64_t used = 0;
    const int64_t rows = sample_rows(P.R);
    for (int64_t r = 0; r < rows; r++) {
        const int32_t* row_anchors = nullptr;
        const mipgen_insertion_record* row_records = nullptr;
        int64_t n_rec = 0;
        if (int rc = row_of((int32_t)r, &row_anchors, &row_records, &n_rec)) return rc;
        if (P.R->n_groups == 0) continue;                                // (nothing is on the device: S stays zero and there is no entry)
        if (used + n_rec > 0x7fffffff) return fail(MIPGEN_E_INVALID, "%s: more than 2^31 - 1 allele records over the sample rows", what);
        const size_t want = (size_t)(used + n_rec);
        if (want > Q.pairs.keys.cap) {                                         // the entries' bytes, known only now: checked before they are allocated
            const size_t need = padded(want, 8) + padded(want, sizeof(InsPoolSums)) + padded(want, 4);
            if (int rc = room_beside(0, &room)) return rc;
            if (need > room)
                return fail(MIPGEN_E_NOMEM, "%s: %zu entries need %zu MiB of device memory, %zu MiB are free", what, want, need >> 20, room >> 20);
            if (int rc = grow_keeping(Q.pairs.keys, (size_t)used, want, st)) return rc;
            if (int rc = grow_keeping(Q.sums, (size_t)used, want, st)) return rc;
            if (int rc = grow_keeping(Q.pairs.ids, (size_t)used, want, st)) return rc;
        }
        timer.mark();
        HIP_TRY(mipgen_launch_ins_pool_append(st, row_anchors, n_out, row_records, n_rec, bg_max_ppm, Q.S.p, Q.pairs.keys.p, Q.sums.p, Q.pairs.ids.p, (int64_t)want, Q.ctr.p));
        timer.mark();
        HIP_TRY(hipMemcpyAsync(&pc, Q.ctr.p, sizeof pc, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if ((int64_t)pc.entries < used || (int64_t)pc.entries > used + n_rec)
            return fail(MIPGEN_E_STATE, "%s: %llu entries after row %lld, %lld before it and %lld records", what, pc.entries, (long long)r, (long long)used, (long long)n_rec);
        used = (int64_t)pc.entries;
    }
    I.n_alleles = -1;                                                    // (the records of the last sample row are no call's result)
    if (used > 0) {
        const size_t ne = (size_t)used;
        size_t scratch = 0;
        HIP_TRY(SortedPairs::scratch_bytes(st, used, 64, used, used, &scratch));
        const size_t need = SortedPairs::bytes(ne, scratch) + padded(ne, INS_POOL_ENTRY_BYTES);
        if (int rc = room_beside(Q.entry_held(), &room)) return rc;
        if (need > room)
            return fail(MIPGEN_E_NOMEM, "%s: %lld entries need %zu MiB of device memory, %zu MiB are free", what, (long long)used, need >> 20, room >> 20);
        // (keys and ids hold the entries and are large enough: the reserve adds their sorted copies and the scratch)
        if (Q.pairs.reserve(ne, scratch) || Q.pool_keys.reserve(ne) || Q.pool_sums.reserve(ne) || Q.run_counts.reserve(ne) || Q.run_start.reserve(ne)) return MIPGEN_E_NOMEM;
        timer.mark();
        HIP_TRY(Q.pairs.sort(st, used, 64));
        HIP_TRY(Q.pairs.runs(st, used, Q.pool_keys.p, Q.run_counts.p, &Q.ctr.p->alleles));
        HIP_TRY(Q.pairs.scan_u32(st, Q.run_counts.p, Q.run_start.p, used));      // (beyond the runs the lengths are unwritten and the starts unread)
        HIP_TRY(mipgen_launch_ins_pool_reduce(st, Q.run_counts.p, Q.run_start.p, &Q.ctr.p->alleles, used, Q.pairs.ids_sorted.p, Q.sums.p, Q.pool_sums.p));
        timer.mark();
        HIP_TRY(hipMemcpyAsync(&pc, Q.ctr.p, sizeof pc, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(idle.wait());
    if ((int64_t)pc.alleles > used || (used > 0 && pc.alleles == 0)) return fail(MIPGEN_E_STATE, "%s: %llu alleles of %lld entries", what, pc.alleles, (long long)used);
    Q.release_transient();
    Q.n_pos = n_out; Q.rows = rows; Q.n_entries = used; Q.n_alleles = (int64_t)pc.alleles;
    Q.args.remember(A, P.n_pos, bg_max_ppm);
    return MIPGEN_OK;
}

// The insertion calls of n_rec allele records on the device (ascending; span[x * span_stride] the row's span of anchor x) against a sparse pool there, into
// V (h->ins_call; h->locus_ins_call for the calls per locus of DESIGN 4.19): k_ins_call_flag, the tail every call shares, and the join of the calls with their allele
// records.  The stream is idle and V.n_calls set on success.
static int run_ins_call(mipgen_accel* h, InsCallRun& V, const mipgen_insertion_record* records, int64_t n_rec, const int32_t* span, int span_stride, int64_t n_pos, const uint64_t* pool_keys,
                        const InsPoolSums* pool_sums, int64_t n_pool, const int32_t* pool_span, bool own_row_is_sample, const mipgen_call_params& prm, SpanTimer& timer,
                        mipgen_call_totals* totals)
{
    V.n_calls = -1;
    if (n_rec > MIPGEN_CALL_MAX_POSITIONS) return fail(MIPGEN_E_INVALID, "insertion call: %lld allele records in the row: 2^29 - 1 at most", (long long)n_rec);
    if (n_rec == 0) {
        if (totals) *totals = mipgen_call_totals{};
        V.n_calls = 0;
        return MIPGEN_OK;
    }
    // flag, tail, sort, gather and join at the worst (every record a call): the shared tail over n_rec candidates and the joined records
    const size_t need = call_run_bytes(n_rec) + padded((size_t)n_rec, sizeof(mipgen_insertion_call_record));
    size_t room = 0;
    if (int rc = room_beside(V.call_held(), &room)) return rc;
    if (need > room)
        return fail(MIPGEN_E_NOMEM, "insertion call: %lld allele records need up to %zu MiB of device memory, %zu MiB are free", (long long)n_rec, need >> 20, room >> 20);
    const CallModel M = model_of(prm);
    hipStream_t st = h->stream;
    if (int rc = run_flagged(h, V.run, n_rec, n_rec, M, timer, totals, [&](mipgen_call_record* cand, CallCounters* ctr) {
            return mipgen_launch_ins_call_flag(st, records, n_rec, span, span_stride, n_pos, pool_keys, pool_sums, n_pool, pool_span, own_row_is_sample ? 1 : 0, M, cand, ctr);
        })) return rc;
    const int64_t n_calls = V.run.n_calls;
    if (n_calls > 0) {
        if (V.out.reserve((size_t)n_calls)) return MIPGEN_E_NOMEM;
        IdleOnExit idle{st};
        timer.mark();
        HIP_TRY(mipgen_launch_ins_call_records(st, V.run.records.p, n_calls, records, n_rec, V.out.p));
        timer.mark();
        HIP_TRY(idle.wait());
    }
    V.n_calls = n_calls;
    return MIPGEN_OK;
}

// the distinct records of a sparse pool that is held, in ascending key order, and S over its anchor rows
static int fetch_ins_pool(mipgen_accel* h, const InsPool& Q, mipgen_insertion_pool_record* pool_records, int64_t n, int32_t* pool_span)
{
    if (n != Q.n_alleles) return fail(MIPGEN_E_INVALID, "%lld pool records asked: the insertion pool holds %lld", (long long)n, (long long)Q.n_alleles);
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = h->stream;
    std::vector<uint64_t> keys((size_t)n);
    std::vector<InsPoolSums> sums((size_t)n);
    {
        IdleOnExit idle{st};
        if (n && pool_records) {
            HIP_TRY(hipMemcpyAsync(keys.data(), Q.pool_keys.p, (size_t)n * 8, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(sums.data(), Q.pool_sums.p, (size_t)n * sizeof(InsPoolSums), hipMemcpyDeviceToHost, st));
        }
        if (pool_span) HIP_TRY(hipMemcpyAsync(pool_span, Q.S.p, (size_t)Q.n_pos * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(idle.wait());
    }
    for (int64_t i = 0; pool_records && i < n; i++) {
        const uint64_t key = keys[(size_t)i];
        pool_records[i] = {gap_allele_pos(key), gap_allele_length(key), gap_allele_bases(key), sums[(size_t)i].K, sums[(size_t)i].X};
    }
    return MIPGEN_OK;
}

template <typename Record>
static int fetch_records(mipgen_accel* h, const DevBuf<Record>& from, int64_t held, const char* none, const char* what, Record* records, int64_t n)
{
    if (held < 0) return fail(MIPGEN_E_STATE, "%s", none);
    if (n != held) return fail(MIPGEN_E_INVALID, "%lld records asked: the last %s left %lld", (long long)n, what, (long long)held);
    if (n == 0) return MIPGEN_OK;
    if (!records) return fail(MIPGEN_E_INVALID, "bad arguments: no records array");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipMemcpyAsync(records, from.p, (size_t)n * sizeof(Record), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return MIPGEN_OK;
}

// ---- insertion alleles per locus -----------------------------------------------------------------------------------------------------------------
// every refusal of allele records given from the host: positions inside the table, lengths that a key can hold, strictly ascending keys
static int check_insertion_records(const mipgen_insertion_record* records, int64_t n_records, int64_t n_pos)
{
    uint64_t before = 0;
    for (int64_t i = 0; i < n_records; i++) {
        const mipgen_insertion_record& r = records[i];
        if (r.pos < 0 || r.pos >= n_pos) return fail(MIPGEN_E_INVALID, "allele record %lld: position %lld of %lld", (long long)i, (long long)r.pos, (long long)n_pos);
        if (r.length < 1 || (!r.ambiguous && r.length > GAP_ALLELE_MAX_LEN))
            return fail(MIPGEN_E_INVALID, "allele record %lld: length %d (1 to %d bases are spelt out; a longer allele is ambiguous)", (long long)i, r.length, GAP_ALLELE_MAX_LEN);
        const uint64_t key = gap_allele_key(r.pos, r.length, r.ambiguous != 0, r.bases);
        if (i && key <= before) return fail(MIPGEN_E_INVALID, "allele record %lld: the records are not in strictly ascending key order", (long long)i);
        before = key;
    }
    return MIPGEN_OK;
}

// The allele records of one row on the device (ascending; n_rec of them, 0 with records NULL) and its anchor table there (NULL: a session without groups left none,
// and the row is all zero) folded under the plan L into F: the map of the plan built first when M does not hold it; then the (locus key, record index) pairs, their
// sort, runs and scan, a locus record per run, and the locus anchor table with its totals - spans of `timer`.  Each budget is checked before the allocations it
// covers.  F.n_alleles locus records and F.anchors stay on the device; locus_anchors (may be NULL) a copy, totals (may be NULL) the sums.  The stream is idle on return.
static int fold_insertions(mipgen_accel* h, const LocusPlan& L, LocusInsMap& M, LocusInsFold& F, const mipgen_insertion_record* records, int64_t n_rec, const int32_t* anchors,
                           SpanTimer& timer, int32_t* locus_anchors, mipgen_locus_insertion_totals* totals)
{
    F.n_alleles = -1;
    hipStream_t st = h->stream;
    const size_t np = (size_t)L.n_pos, nl = (size_t)L.n_loci, cells = nl * INSERTION_COLUMNS;
    if (n_rec > 0x3fffffff) return fail(MIPGEN_E_INVALID, "locus insertions: %lld allele records in the row: twice as many pairs do not fit the sort", (long long)n_rec);
    size_t room = 0;
    if (!M.have) {
        if (int rc = room_beside(M.held(), &room)) return rc;
        if (2 * padded(np, 4) > room)
            return fail(MIPGEN_E_NOMEM, "locus insertions: the anchor map of %lld positions needs %zu MiB of device memory, %zu MiB are free", (long long)L.n_pos,
                        (2 * padded(np, 4)) >> 20, room >> 20);
        if (M.own.reserve(np) || M.prev.reserve(np)) return MIPGEN_E_NOMEM;
    }
    if (int rc = room_beside(F.table_held(), &room)) return rc;
    if (padded(cells, 4) + padded(1, sizeof(LocusInsCounters)) > room)
        return fail(MIPGEN_E_NOMEM, "locus insertions: %lld loci need %zu MiB of device memory, %zu MiB are free", (long long)L.n_loci,
                    (padded(cells, 4) + padded(1, sizeof(LocusInsCounters))) >> 20, room >> 20);
    if (F.anchors.reserve(cells) || F.ctr.reserve(1)) return MIPGEN_E_NOMEM;
    const int64_t cap = 2 * n_rec;
    if (n_rec > 0) {
        size_t scratch = 0;
        HIP_TRY(SortedPairs::scratch_bytes(st, cap, 64, cap, cap, &scratch));
        const size_t need = SortedPairs::bytes((size_t)cap, scratch) + padded((size_t)cap, 4) + padded((size_t)cap, sizeof(mipgen_insertion_record));
        if (int rc = room_beside(F.pair_held(), &room)) return rc;
        if (need > room)
            return fail(MIPGEN_E_NOMEM, "locus insertions: %lld allele records need up to %zu MiB of device memory, %zu MiB are free", (long long)n_rec, need >> 20, room >> 20);
        if (F.pairs.reserve((size_t)cap, scratch) || F.run_start.reserve((size_t)cap) || F.records.reserve((size_t)cap)) return MIPGEN_E_NOMEM;
    }
    IdleOnExit idle{st};
    LocusInsCounters lc;
    memset(&lc, 0, sizeof lc);
    HIP_TRY(hipMemsetAsync(F.ctr.p, 0, sizeof lc, st));
    timer.mark();
    if (!M.have) {
        HIP_TRY(hipMemsetAsync(M.own.p, 0xff, np * 4, st));
        HIP_TRY(hipMemsetAsync(M.prev.p, 0xff, np * 4, st));
        HIP_TRY(mipgen_launch_locus_anchor_map(st, L.src.p, L.first.p, L.n_pos, L.n_loci, M.own.p, M.prev.p));
        M.have = true;
    }
    if (anchors) HIP_TRY(mipgen_launch_locus_anchor_merge(st, anchors, L.src.p, L.first.p, L.n_pos, L.n_loci, F.anchors.p, F.ctr.p));
    else HIP_TRY(hipMemsetAsync(F.anchors.p, 0, cells * sizeof(int32_t), st));
    if (n_rec > 0) HIP_TRY(mipgen_launch_locus_ins_fold(st, records, n_rec, M.own.p, M.prev.p, L.n_pos, F.pairs.keys.p, F.pairs.ids.p, cap, F.ctr.p));
    timer.mark();
    HIP_TRY(hipMemcpyAsync(&lc, F.ctr.p, sizeof lc, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const int64_t folded = (int64_t)lc.folded;
    if (folded < 0 || folded > cap || (int64_t)lc.dropped > n_rec)
        return fail(MIPGEN_E_STATE, "locus insertions: %llu pairs and %llu records without a source of %lld records", lc.folded, lc.dropped, (long long)n_rec);
    if (folded > 0) {
        timer.mark();
        int32_t* run_counts = reinterpret_cast<int32_t*>(F.pairs.ids.p);
        HIP_TRY(F.pairs.sort(st, folded, 64));
        HIP_TRY(F.pairs.runs(st, folded, F.pairs.keys.p, run_counts, &F.ctr.p->alleles));
        HIP_TRY(F.pairs.scan_u32(st, run_counts, F.run_start.p, folded));          // (beyond the runs the lengths are stale and the starts unread)
        HIP_TRY(mipgen_launch_locus_ins_reduce(st, F.pairs.keys.p, run_counts, F.run_start.p, &F.ctr.p->alleles, folded, F.pairs.ids_sorted.p, records, n_rec, F.records.p));
        timer.mark();
        HIP_TRY(hipMemcpyAsync(&lc, F.ctr.p, sizeof lc, hipMemcpyDeviceToHost, st));
    }
    if (locus_anchors) HIP_TRY(hipMemcpyAsync(locus_anchors, F.anchors.p, cells * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(idle.wait());
    if ((int64_t)lc.alleles > folded || (folded > 0 && lc.alleles == 0)) return fail(MIPGEN_E_STATE, "locus insertions: %llu locus records of %lld pairs", lc.alleles, (long long)folded);
    if ((int64_t)lc.alleles > MIPGEN_CALL_MAX_POSITIONS) return fail(MIPGEN_E_INVALID, "locus insertions: %llu locus records in the row: 2^29 - 1 at most", lc.alleles);
    F.n_alleles = (int64_t)lc.alleles;
    if (totals)
        *totals = {(int64_t)lc.loci, (int64_t)lc.span, (int64_t)lc.insertions, (int64_t)lc.ins_discordant, (int64_t)lc.ambiguous, F.n_alleles, folded, (int64_t)lc.dropped};
    return MIPGEN_OK;
}

// One planned row of the session through the insertions route (into R->ins, as the insertion pool and call of 4.17 count) and folded under the installed plan into
// the handle's fold.  counts, anchors, ins_totals: what the plain insertions call returns (each may be NULL).
static int locus_insertions_row(mipgen_accel* h, const RowPlan& P, const RowArgs& A, int32_t row, SpanTimer& timer, int32_t* counts, int32_t* anchors, int32_t* locus_anchors,
                                mipgen_insertion_totals* ins_totals, mipgen_locus_insertion_totals* totals)
{
    h->locus_ins.fold.n_alleles = -1;
    if (int rc = insertions_row(h, P, A, row, timer, counts, anchors, ins_totals)) return rc;
    const InsScratch& I = P.R->ins;
    const bool on_device = P.R->n_groups != 0;
    return fold_insertions(h, P.R->locus.plan, P.R->locus_ins.map, h->locus_ins.fold, on_device ? I.records.p : nullptr, on_device ? I.n_alleles : 0,
                           on_device ? I.anchors.p : nullptr, timer, locus_anchors, totals);
}

extern "C" {

// Allele counts per template position of one row from the consensus reads the handle holds.  Reads R's groups and reads; writes R->pile only.
int mipgen_accel_reads_consensus_pileup(mipgen_accel* h, const int32_t* mol_len, int32_t n, int32_t row, int32_t min_family, int32_t min_quality, int32_t* counts,
                                        mipgen_pileup_totals* totals)
{
    RowPlan P;
    const RowArgs A{nullptr, mol_len, n, min_family, min_quality, 0};
    if (int rc = plan_row(h, A, row, &P)) return rc;
    h->pileup_ms = -1.0;
    SpanTimer pile_time{h->timing, h->stream};
    mipgen_gapped_totals t;
    Counted counted;
    if (int rc = count_row(h, P, P.R->pile, Budget{"pileup"}, A, row, pile_time, counts, &t, &counted)) return rc;
    if (totals) *totals = {t.groups, t.used, t.bases, t.discordant};
    return booked(pile_time, &h->pileup_ms);
}

// The pileup with indels of one row.  Reads R's groups and reads; writes R->gapped only.
int mipgen_accel_reads_consensus_pileup_gapped(mipgen_accel* h, const char* mol_seq, const int32_t* mol_len, int32_t n, int32_t row, int32_t min_family, int32_t min_quality,
                                               int32_t max_indel, int32_t* counts, mipgen_gapped_totals* totals)
{
    RowPlan P;
    const RowArgs A{mol_seq, mol_len, n, min_family, min_quality, max_indel, true, true};
    if (int rc = plan_row(h, A, row, &P)) return rc;
    h->gapped_ms = -1.0;
    SpanTimer gap_time{h->timing, h->stream};
    Counted counted;
    if (int rc = count_row(h, P, P.R->gapped, Budget{"gapped pileup"}, A, row, gap_time, counts, totals, &counted)) return rc;
    return booked(gap_time, &h->gapped_ms);
}

// Insertion alleles of one row: insertions_row with a timer of its own.  Reads R's groups and reads; writes R->ins only.
int mipgen_accel_reads_consensus_insertions(mipgen_accel* h, const char* mol_seq, const int32_t* mol_len, int32_t n, int32_t row, int32_t min_family, int32_t min_quality,
                                            int32_t max_indel, int32_t* counts, int32_t* anchors, mipgen_insertion_totals* totals)
{
    RowPlan P;
    const RowArgs A{mol_seq, mol_len, n, min_family, min_quality, max_indel, true, true, true};
    if (int rc = plan_insertions(h, A, row, &P)) return rc;
    h->insertions_ms = -1.0;
    SpanTimer timer{h->timing, h->stream};
    if (int rc = insertions_row(h, P, A, row, timer, counts, anchors, totals)) return rc;
    return booked(timer, &h->insertions_ms);
}

// The records of the last insertions call, in ascending key order.
int mipgen_accel_insertions_fetch(mipgen_accel* h, mipgen_insertion_record* records, int64_t n)
{
    if (int rc = check_reads(h)) return rc;
    const InsScratch& S = h->consensus->ins;
    return fetch_records(h, S.records, S.n_alleles, "the consensus reads hold no insertion alleles: mipgen_accel_reads_consensus_insertions leaves them", "insertions call",
                         records, n);
}

// Deletion alleles of one row: deletions_row with a timer of its own.  Reads R's groups and reads; writes R->del only.
int mipgen_accel_reads_consensus_deletions(mipgen_accel* h, const char* mol_seq, const int32_t* mol_len, int32_t n, int32_t row, int32_t min_family, int32_t min_quality,
                                           int32_t max_indel, int32_t* counts, int32_t* sites, mipgen_deletion_totals* totals)
{
    RowPlan P;
    const RowArgs A{mol_seq, mol_len, n, min_family, min_quality, max_indel, true, true};
    if (int rc = plan_row(h, A, row, &P)) return rc;
    if (P.n_pos > MIPGEN_CALL_MAX_POSITIONS) return fail(MIPGEN_E_INVALID, "%lld template positions: the deletion alleles take 2^29 - 1 at most", (long long)P.n_pos);
    h->deletions_ms = -1.0;
    SpanTimer timer{h->timing, h->stream};
    if (int rc = deletions_row(h, P, A, row, timer, counts, sites, totals)) return rc;
    return booked(timer, &h->deletions_ms);
}

// The records of the last deletions call, in ascending key order.
int mipgen_accel_deletions_fetch(mipgen_accel* h, mipgen_deletion_record* records, int64_t n)
{
    if (int rc = check_reads(h)) return rc;
    const DelScratch& S = h->consensus->del;
    return fetch_records(h, S.records, S.n_alleles, "the consensus reads hold no deletion alleles: mipgen_accel_reads_consensus_deletions leaves them", "deletions call",
                         records, n);
}

// Insertion calls from host arrays: no read session is needed; the arrays are uploaded into the handle's InsCallRun, the pool records as keys and sums.
int mipgen_accel_insertion_call_tables(mipgen_accel* h, const mipgen_insertion_record* records, int64_t n_records, const int32_t* span, int64_t n_pos,
                                       const mipgen_insertion_pool_record* pool_records, int64_t n_pool, const int32_t* pool_span, int32_t own_row_is_sample,
                                       const mipgen_call_params* params, mipgen_call_totals* totals)
{
    if (!h) return fail(MIPGEN_E_INVALID, "null handle");
    if (int rc = check_call_params(params)) return rc;
    if (n_pos < 1 || n_pos > MIPGEN_CALL_MAX_POSITIONS) return fail(MIPGEN_E_INVALID, "%lld positions: 1 to 2^29 - 1", (long long)n_pos);
    if (n_records < 0 || n_records > MIPGEN_CALL_MAX_POSITIONS) return fail(MIPGEN_E_INVALID, "%lld allele records: 0 to 2^29 - 1", (long long)n_records);
    if (n_pool < 0 || n_pool > MIPGEN_CALL_MAX_POSITIONS) return fail(MIPGEN_E_INVALID, "%lld pool records: 0 to 2^29 - 1", (long long)n_pool);
    if (!span || !pool_span || (n_records && !records) || (n_pool && !pool_records)) return fail(MIPGEN_E_INVALID, "bad arguments: no records, no span, no pool records or no pool span");
    uint64_t before = 0;
    for (int64_t i = 0; i < n_records; i++) {
        const mipgen_insertion_record& r = records[i];
        if (r.pos < 0 || r.pos >= n_pos) return fail(MIPGEN_E_INVALID, "allele record %lld: position %lld of %lld", (long long)i, (long long)r.pos, (long long)n_pos);
        if (r.length < 1 || (!r.ambiguous && r.length > GAP_ALLELE_MAX_LEN))
            return fail(MIPGEN_E_INVALID, "allele record %lld: length %d (1 to %d bases are spelt out; a longer allele is ambiguous)", (long long)i, r.length, GAP_ALLELE_MAX_LEN);
        const uint64_t key = gap_allele_key(r.pos, r.length, r.ambiguous != 0, r.bases);
        if (i && key <= before) return fail(MIPGEN_E_INVALID, "allele record %lld: the records are not in strictly ascending key order", (long long)i);
        before = key;
    }
    std::vector<uint64_t> keys((size_t)n_pool);
    std::vector<InsPoolSums> sums((size_t)n_pool);
    for (int64_t i = 0; i < n_pool; i++) {
        const mipgen_insertion_pool_record& r = pool_records[i];
        if (r.pos < 0 || r.pos >= n_pos) return fail(MIPGEN_E_INVALID, "pool record %lld: position %lld of %lld", (long long)i, (long long)r.pos, (long long)n_pos);
        if (r.length < 1 || r.length > GAP_ALLELE_MAX_LEN) return fail(MIPGEN_E_INVALID, "pool record %lld: length %d: 1 to %d", (long long)i, r.length, GAP_ALLELE_MAX_LEN);
        keys[(size_t)i] = ins_call_key(r.pos, r.length, r.bases);
        if (i && keys[(size_t)i] <= keys[(size_t)i - 1]) return fail(MIPGEN_E_INVALID, "pool record %lld: the pool is not in strictly ascending key order", (long long)i);
        sums[(size_t)i] = {r.bg_alt, r.bg_excluded};
    }
    HIP_TRY(hipSetDevice(h->device));
    InsCallRun& V = h->ins_call;
    V.n_calls = -1;
    h->ins_call_ms = -1.0;
    const size_t np = (size_t)n_pos, nr = (size_t)n_records, nq = (size_t)n_pool;
    const size_t need = 2 * padded(np, 4) + padded(nr, sizeof(mipgen_insertion_record)) + padded(nq, 8) + padded(nq, sizeof(InsPoolSums));
    size_t room = 0;
    if (int rc = room_beside(V.upload_held(), &room)) return rc;
    if (need > room)
        return fail(MIPGEN_E_NOMEM, "insertion call: %lld positions, %lld allele records and %lld pool records need %zu MiB of device memory, %zu MiB are free", (long long)n_pos,
                    (long long)n_records, (long long)n_pool, need >> 20, room >> 20);
    if (V.span.reserve(np) || V.pool_span.reserve(np) || V.records.reserve(std::max<size_t>(nr, 1)) || V.pool_keys.reserve(std::max<size_t>(nq, 1)) ||
        V.pool_sums.reserve(std::max<size_t>(nq, 1)))
        return MIPGEN_E_NOMEM;
    hipStream_t st = h->stream;
    IdleOnExit idle{st};                                                 // (keys and sums outlive their copies)
    HIP_TRY(hipMemcpyAsync(V.span.p, span, np * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(V.pool_span.p, pool_span, np * 4, hipMemcpyHostToDevice, st));
    if (nr) HIP_TRY(hipMemcpyAsync(V.records.p, records, nr * sizeof(mipgen_insertion_record), hipMemcpyHostToDevice, st));
    if (nq) HIP_TRY(hipMemcpyAsync(V.pool_keys.p, keys.data(), nq * 8, hipMemcpyHostToDevice, st));
    if (nq) HIP_TRY(hipMemcpyAsync(V.pool_sums.p, sums.data(), nq * sizeof(InsPoolSums), hipMemcpyHostToDevice, st));
    SpanTimer timer{h->timing, st};
    if (int rc = run_ins_call(h, V, V.records.p, n_records, V.span.p, 1, n_pos, V.pool_keys.p, V.pool_sums.p, n_pool, V.pool_span.p, own_row_is_sample != 0, *params, timer, totals))
        return rc;
    return booked(timer, &h->ins_call_ms);
}

// The sparse pool over the sample rows of the session.  Writes R->ins_pool and, through the insertions route of every row, R->ins.
int mipgen_accel_reads_consensus_insertion_pool(mipgen_accel* h, const char* mol_seq, const int32_t* mol_len, int32_t n, int32_t min_family, int32_t min_quality,
                                                int32_t max_indel, int32_t bg_max_ppm, mipgen_insertion_pool_totals* totals)
{
    RowPlan P;
    const RowArgs A{mol_seq, mol_len, n, min_family, min_quality, max_indel, true, true, true};
    if (int rc = plan_insertions(h, A, 0, &P)) return rc;
    if (int rc = check_bg_max_ppm(bg_max_ppm)) return rc;
    InsPool& Q = P.R->ins_pool;
    Q.args.have = false;                                                 // (a pool that fails leaves none)
    h->ins_call_ms = -1.0;
    SpanTimer timer{h->timing, h->stream};
    const InsScratch& I = P.R->ins;
    if (int rc = build_ins_pool(h, P, A, bg_max_ppm, timer, Q, P.n_pos, "insertion pool", [&](int32_t r, const int32_t** anchors, const mipgen_insertion_record** records, int64_t* n_rec) {
            if (int rc = insertions_row(h, P, A, r, timer, nullptr, nullptr, nullptr)) return rc;
            *anchors = I.anchors.p; *records = I.records.p; *n_rec = I.n_alleles;
            return (int)MIPGEN_OK;
        })) return rc;
    if (totals) *totals = {Q.rows, Q.n_entries, Q.n_alleles};
    return booked(timer, &h->ins_call_ms);
}

// The distinct records of the pool, in ascending key order, and S.
int mipgen_accel_insertion_pool_fetch(mipgen_accel* h, mipgen_insertion_pool_record* pool_records, int64_t n, int32_t* pool_span)
{
    if (int rc = check_reads(h)) return rc;
    const InsPool& Q = h->consensus->ins_pool;
    if (!Q.args.have) return fail(MIPGEN_E_STATE, "the consensus reads have no insertion pool: mipgen_accel_reads_consensus_insertion_pool builds it");
    return fetch_ins_pool(h, Q, pool_records, n, pool_span);
}

// The insertion calls of one row against the sparse pool: the row's insertions recomputed with the pool's arguments into R->ins, where
// mipgen_accel_insertions_fetch finds its records, then flag, tail, order and join.
int mipgen_accel_reads_consensus_insertion_call(mipgen_accel* h, int32_t row, const mipgen_call_params* params, int32_t* counts, int32_t* anchors,
                                                mipgen_insertion_totals* ins_totals, mipgen_call_totals* call_totals)
{
    if (int rc = check_reads(h)) return rc;
    const InsPool& Q = h->consensus->ins_pool;
    if (!Q.args.have) return fail(MIPGEN_E_STATE, "the consensus reads have no insertion pool: mipgen_accel_reads_consensus_insertion_pool builds it");
    RowPlan P;
    RowArgs A;
    if (int rc = plan_call(h, Q.args, row, params, "insertion pool", &A, &P)) return rc;
    A.need_seq = A.must_place = A.runs = true;
    h->ins_call_ms = -1.0;
    h->ins_call.n_calls = -1;
    SpanTimer timer{h->timing, h->stream};
    if (int rc = insertions_row(h, P, A, row, timer, counts, anchors, ins_totals)) return rc;
    const InsScratch& I = P.R->ins;
    if (int rc = run_ins_call(h, h->ins_call, I.records.p, I.n_alleles, I.anchors.p, INSERTION_COLUMNS, P.n_pos, Q.pool_keys.p, Q.pool_sums.p, Q.n_alleles, Q.S.p,
                              (int64_t)row < sample_rows(P.R), *params, timer, call_totals)) return rc;
    return booked(timer, &h->ins_call_ms);
}

// The records of the last insertion call of either kind, in ascending allele-key order.
int mipgen_accel_insertion_call_fetch(mipgen_accel* h, mipgen_insertion_call_record* records, int64_t n)
{
    if (!h) return fail(MIPGEN_E_INVALID, "null handle");
    return fetch_records(h, h->ins_call.out, h->ins_call.n_calls,
                         "the handle holds no insertion calls: mipgen_accel_insertion_call_tables or mipgen_accel_reads_consensus_insertion_call leaves them", "insertion call",
                         records, n);
}

// Calls from host arrays: no read session is needed; the arrays are uploaded into the handle's CallRun.
int mipgen_accel_call_tables(mipgen_accel* h, const int32_t* counts, int32_t columns, const int32_t* pool, const uint8_t* ref, int64_t n_pos, int32_t own_row_is_sample,
                             const mipgen_call_params* params, mipgen_call_totals* totals)
{
    if (!h) return fail(MIPGEN_E_INVALID, "null handle");
    if (!counts || !pool || !ref) return fail(MIPGEN_E_INVALID, "bad arguments: no counts, no pool or no ref bytes");
    if (columns != PILEUP_COLUMNS && columns != GAPPED_COLUMNS) return fail(MIPGEN_E_INVALID, "%d columns: %d (the pileup's table) or %d (the gapped one)", columns, PILEUP_COLUMNS, GAPPED_COLUMNS);
    if (n_pos < 1 || n_pos > MIPGEN_CALL_MAX_POSITIONS) return fail(MIPGEN_E_INVALID, "%lld positions: 1 to 2^29 - 1", (long long)n_pos);
    if (int rc = check_call_params(params)) return rc;
    HIP_TRY(hipSetDevice(h->device));
    CallRun& U = h->call_run;
    h->call_ms = -1.0;
    const size_t np = (size_t)n_pos, need = padded(np * (size_t)columns, 4) + padded(np * 10, 4) + padded(np, 1) + call_run_bytes(4 * n_pos);
    size_t room = 0;
    if (int rc = room_beside(U.held(), &room)) return rc;
    if (need > room) return fail(MIPGEN_E_NOMEM, "call: %lld positions need up to %zu MiB of device memory, %zu MiB are free", (long long)n_pos, need >> 20, room >> 20);
    if (U.counts.reserve(np * (size_t)columns) || U.pool.reserve(np * 10) || U.ref.reserve(np)) return MIPGEN_E_NOMEM;
    hipStream_t st = h->stream;
    IdleOnExit idle{st};
    HIP_TRY(hipMemcpyAsync(U.counts.p, counts, np * (size_t)columns * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(U.pool.p, pool, np * 40, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(U.ref.p, ref, np, hipMemcpyHostToDevice, st));
    SpanTimer timer{h->timing, st};
    if (int rc = run_call(h, U.counts.p, columns, U.pool.p, U.ref.p, n_pos, own_row_is_sample != 0, *params, timer, totals)) return rc;
    return booked(timer, &h->call_ms);
}

// The pool over the sample rows of the session: every row's pileup into R->call's own scratch, added on the device.  Writes R->call only.
int mipgen_accel_reads_consensus_call_pool(mipgen_accel* h, const char* mol_seq, const int32_t* mol_len, int32_t n, int32_t min_family, int32_t min_quality,
                                           int32_t max_indel, int32_t bg_max_ppm)
{
    RowPlan P;
    const RowArgs A{mol_seq, mol_len, n, min_family, min_quality, max_indel, true};      // the template bases are the ref bytes: needed without indels too
    if (int rc = plan_row(h, A, 0, &P)) return rc;
    if (int rc = check_bg_max_ppm(bg_max_ppm)) return rc;
    if (P.n_pos > MIPGEN_CALL_MAX_POSITIONS) return fail(MIPGEN_E_INVALID, "%lld template positions: a call takes 2^29 - 1 at most", (long long)P.n_pos);
    CallScratch& C = P.R->call;
    C.state.drop();                                                      // (a pool that fails leaves none)
    h->call_ms = -1.0;
    const size_t np = (size_t)P.n_pos;
    // the budget of the pool AND of the calls that follow, before anything is allocated; the row's own terms are count_row's
    const size_t more = padded(np * 10, 4) + padded(np, 1) + call_run_bytes(4 * P.n_pos), held = C.state.pool.cap * 4 + C.ref.cap + h->call_run.held();
    size_t room = 0;
    if (int rc = room_beside(held, &room)) return rc;
    if (more > room)
        return fail(MIPGEN_E_NOMEM, "call pool: %lld template positions need up to %zu MiB of device memory beside the pileup's, %zu MiB are free", (long long)P.n_pos,
                    more >> 20, room >> 20);
    const Budget B{"call pool", more, held, true};                       // held BEFORE the reserves, as it always was here (the locus route below takes it after)
    if (C.state.pool.reserve(np * 10) || C.ref.reserve(np)) return MIPGEN_E_NOMEM;
    HIP_TRY(hipMemcpyAsync(C.ref.p, mol_seq, np, hipMemcpyHostToDevice, h->stream));      // (build_pool leaves the stream idle however it ends)
    return build_pool(h, P, probe_target(h, P.R), B, A, bg_max_ppm);
}

// The calls of one row against the pool: the row's pileup recomputed with the pool's arguments into R->call's scratch, then flag, tail and order.
int mipgen_accel_reads_consensus_call(mipgen_accel* h, int32_t row, const mipgen_call_params* params, int32_t* counts, mipgen_call_totals* totals)
{
    if (int rc = check_reads(h)) return rc;
    const PoolState& S = h->consensus->call.state;
    if (!S.have) return fail(MIPGEN_E_STATE, "the consensus reads have no pool: mipgen_accel_reads_consensus_call_pool builds it");
    RowPlan P;
    RowArgs A;
    if (int rc = plan_call(h, S, row, params, "pool", &A, &P)) return rc;
    return call_row(h, P, probe_target(h, P.R), A, "call", row, *params, counts, nullptr, totals);
}

int mipgen_accel_reads_consensus_call_pileup_totals(mipgen_accel* h, mipgen_gapped_totals* totals)
{
    return last_pileup_totals(h, false, "no row was called: mipgen_accel_reads_consensus_call counts one", totals);
}

// A table from host arrays folded by a plan from host arrays: no read session is needed; everything is uploaded into the handle's LocusRun.
int mipgen_accel_locus_tables(mipgen_accel* h, const int32_t* counts, int32_t columns, const int64_t* plan, int64_t n_pos, int64_t n_loci, int32_t* merged,
                              mipgen_locus_totals* totals)
{
    if (!h) return fail(MIPGEN_E_INVALID, "null handle");
    if (!counts) return fail(MIPGEN_E_INVALID, "bad arguments: no counts");
    if (columns != PILEUP_COLUMNS && columns != GAPPED_COLUMNS) return fail(MIPGEN_E_INVALID, "%d columns: %d (the pileup's table) or %d (the gapped one)", columns, PILEUP_COLUMNS, GAPPED_COLUMNS);
    if (int rc = check_locus_plan(plan, n_pos, n_loci)) return rc;
    HIP_TRY(hipSetDevice(h->device));
    LocusRun& U = h->locus_run;
    h->locus_ms = -1.0;
    const size_t np = (size_t)n_pos, nl = (size_t)n_loci, cols = (size_t)columns;
    SpanTimer timer{h->timing, h->stream};
    if (int rc = build_locus_plan(h, U.plan, plan, n_pos, n_loci, padded(np * cols, 4) + padded(nl * cols, 4) + padded(1, sizeof(LocusCounters)),
                                  (U.counts.cap + U.merged.cap) * 4 + U.ctr.cap * sizeof(LocusCounters), "locus tables", timer)) return rc;
    if (U.counts.reserve(np * cols) || U.merged.reserve(nl * cols) || U.ctr.reserve(1)) return MIPGEN_E_NOMEM;
    {
        IdleOnExit idle{h->stream};
        HIP_TRY(hipMemcpyAsync(U.counts.p, counts, np * cols * 4, hipMemcpyHostToDevice, h->stream));
    }
    if (int rc = merge_loci(h, U.plan, U.counts.p, columns, U.merged.p, U.ctr.p, timer, merged, totals)) return rc;
    return booked(timer, &h->locus_ms);
}

// The plan and the ref bytes of the loci for the consensus reads the handle holds.  Writes R->locus only; a pool over an earlier plan is dropped.
int mipgen_accel_reads_consensus_locus_plan(mipgen_accel* h, const int64_t* plan, int64_t n_pos, const uint8_t* locus_ref, int64_t n_loci)
{
    if (int rc = check_reads(h)) return rc;
    if (!locus_ref) return fail(MIPGEN_E_INVALID, "bad arguments: no ref bytes of the loci");
    if (int rc = check_locus_plan(plan, n_pos, n_loci)) return rc;
    HIP_TRY(hipSetDevice(h->device));
    LocusScratch& L = h->consensus->locus;
    h->locus_ms = -1.0;
    SpanTimer timer{h->timing, h->stream};
    const int built = build_locus_plan(h, L.plan, plan, n_pos, n_loci, padded((size_t)n_loci, 1), L.ref.cap, "locus plan", timer);
    if (!L.plan.have || built == MIPGEN_OK) { L.state.drop(); h->consensus->locus_ins.drop(); }      // the pools and the anchor map go with their plan: a plan refused for its budget leaves them as they were
    if (built) return built;
    L.plan.have = false;                                                 // (until the ref bytes are there too)
    if (L.ref.reserve((size_t)n_loci)) return MIPGEN_E_NOMEM;
    HIP_TRY(hipMemcpyAsync(L.ref.p, locus_ref, (size_t)n_loci, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    L.plan.have = true;
    return booked(timer, &h->locus_ms);
}

// One row counted per template position and folded per locus.  Reads R's groups and reads and the installed plan; writes R->locus only.
int mipgen_accel_reads_consensus_locus_pileup(mipgen_accel* h, const char* mol_seq, const int32_t* mol_len, int32_t n, int32_t row, int32_t min_family, int32_t min_quality,
                                              int32_t max_indel, int32_t* probe_counts, int32_t* locus_counts, mipgen_gapped_totals* pileup_totals, mipgen_locus_totals* totals)
{
    RowPlan P;
    const RowArgs A{mol_seq, mol_len, n, min_family, min_quality, max_indel, max_indel != 0};
    if (int rc = plan_row(h, A, row, &P)) return rc;
    LocusScratch& L = P.R->locus;
    if (int rc = check_locus_session(L, P)) return rc;
    h->locus_ms = -1.0;
    const size_t nl = (size_t)L.plan.n_loci, cols = max_indel ? GAPPED_COLUMNS : PILEUP_COLUMNS;
    const size_t more = padded(nl * cols, 4) + padded(1, sizeof(LocusCounters));
    const auto held = [&] { return L.merged.cap * 4 + L.ctr.cap * sizeof(LocusCounters); };
    size_t room = 0;
    if (int rc = room_beside(held(), &room)) return rc;
    if (more > room)
        return fail(MIPGEN_E_NOMEM, "locus pileup: %lld loci need %zu MiB of device memory beside the pileup's, %zu MiB are free", (long long)L.plan.n_loci, more >> 20,
                    room >> 20);
    if (L.merged.reserve(nl * cols) || L.ctr.reserve(1)) return MIPGEN_E_NOMEM;
    const Budget B{"locus pileup", more, held(), true};                  // held AFTER the reserves: what they took is no longer free, and the count tests need <= held + free
    SpanTimer timer{h->timing, h->stream};
    Counted counted;
    if (int rc = count_target(h, P, locus_target(h, P.R), B, A, row, timer, probe_counts, locus_counts, pileup_totals, totals, &counted)) return rc;
    return booked(timer, &h->locus_ms);
}

// The pool over the sample rows of the session, per locus: every row counted, folded and added on the device.  Writes R->locus only.
int mipgen_accel_reads_consensus_locus_call_pool(mipgen_accel* h, const char* mol_seq, const int32_t* mol_len, int32_t n, int32_t min_family, int32_t min_quality,
                                                 int32_t max_indel, int32_t bg_max_ppm)
{
    RowPlan P;
    const RowArgs A{mol_seq, mol_len, n, min_family, min_quality, max_indel, max_indel != 0};      // (the ref bytes came with the plan, which also bounded the loci)
    if (int rc = plan_row(h, A, 0, &P)) return rc;
    if (int rc = check_bg_max_ppm(bg_max_ppm)) return rc;
    LocusScratch& L = P.R->locus;
    if (int rc = check_locus_session(L, P)) return rc;
    L.state.drop();                                                      // (a pool that fails leaves none)
    h->locus_ms = -1.0;
    const int64_t n_loci = L.plan.n_loci;
    const size_t nl = (size_t)n_loci, cols = max_indel ? GAPPED_COLUMNS : PILEUP_COLUMNS;
    // the budget of the pool AND of the calls that follow, before anything is allocated; the row's own terms are count_row's
    const size_t more = padded(nl * cols, 4) + padded(nl * 10, 4) + padded(1, sizeof(LocusCounters)) + call_run_bytes(4 * n_loci);
    const auto held = [&] { return (L.merged.cap + L.state.pool.cap) * 4 + L.ctr.cap * sizeof(LocusCounters) + h->call_run.held(); };
    size_t room = 0;
    if (int rc = room_beside(held(), &room)) return rc;
    if (more > room)
        return fail(MIPGEN_E_NOMEM, "locus call pool: %lld loci need up to %zu MiB of device memory beside the pileup's, %zu MiB are free", (long long)n_loci, more >> 20,
                    room >> 20);
    if (L.merged.reserve(nl * cols) || L.state.pool.reserve(nl * 10) || L.ctr.reserve(1)) return MIPGEN_E_NOMEM;
    const Budget B{"locus call pool", more, held(), true};               // held AFTER the reserves, as in the locus pileup
    return build_pool(h, P, locus_target(h, P.R), B, A, bg_max_ppm);
}

// The calls of one row per locus against the locus pool: the row counted with the pool's arguments and folded, then run_call over the loci.
int mipgen_accel_reads_consensus_locus_call(mipgen_accel* h, int32_t row, const mipgen_call_params* params, int32_t* probe_counts, int32_t* locus_counts,
                                            mipgen_call_totals* totals)
{
    if (int rc = check_reads(h)) return rc;
    const LocusScratch& L = h->consensus->locus;
    if (!L.plan.have) return fail(MIPGEN_E_STATE, "the consensus reads have no locus plan: mipgen_accel_reads_consensus_locus_plan installs it");
    if (!L.state.have) return fail(MIPGEN_E_STATE, "the consensus reads have no locus pool: mipgen_accel_reads_consensus_locus_call_pool builds it");
    RowPlan P;
    RowArgs A;
    if (int rc = plan_call(h, L.state, row, params, "locus pool", &A, &P)) return rc;
    return call_row(h, P, locus_target(h, P.R), A, "locus call", row, *params, probe_counts, locus_counts, totals);
}

int mipgen_accel_reads_consensus_locus_call_pileup_totals(mipgen_accel* h, mipgen_gapped_totals* totals)
{
    return last_pileup_totals(h, true, "no row was called per locus: mipgen_accel_reads_consensus_locus_call counts one", totals);
}

// The records of the last call of either kind, in ascending (pos, allele).
int mipgen_accel_call_fetch(mipgen_accel* h, mipgen_call_record* records, int64_t n)
{
    if (!h) return fail(MIPGEN_E_INVALID, "null handle");
    return fetch_records(h, h->call_run.records, h->call_run.n_calls, "the handle holds no calls: mipgen_accel_call_tables or mipgen_accel_reads_consensus_call leaves them", "call",
                         records, n);
}

// ---- insertion alleles per locus ----
// Allele records and an anchor table from host arrays folded by a plan from host arrays: no read session is needed; everything is uploaded into the handle's LocusInsRun.
int mipgen_accel_locus_insertion_tables(mipgen_accel* h, const mipgen_insertion_record* records, int64_t n_records, const int32_t* anchors, const int64_t* plan, int64_t n_pos,
                                        int64_t n_loci, int32_t* locus_anchors, mipgen_locus_insertion_totals* totals)
{
    if (!h) return fail(MIPGEN_E_INVALID, "null handle");
    if (!anchors || (n_records && !records)) return fail(MIPGEN_E_INVALID, "bad arguments: no anchor table or no allele records");
    if (int rc = check_locus_plan(plan, n_pos, n_loci)) return rc;
    if (n_records < 0 || n_records > MIPGEN_CALL_MAX_POSITIONS) return fail(MIPGEN_E_INVALID, "%lld allele records: 0 to 2^29 - 1", (long long)n_records);
    if (int rc = check_insertion_records(records, n_records, n_pos)) return rc;
    HIP_TRY(hipSetDevice(h->device));
    LocusInsRun& U = h->locus_ins;
    U.fold.n_alleles = -1;
    U.map.have = false;                                                  // (the map is of the plan of this call)
    h->locus_ins_ms = -1.0;
    const size_t np = (size_t)n_pos, nr = (size_t)n_records;
    SpanTimer timer{h->timing, h->stream};
    if (int rc = build_locus_plan(h, U.plan, plan, n_pos, n_loci, padded(np * INSERTION_COLUMNS, 4) + padded(nr, sizeof(mipgen_insertion_record)), U.upload_held(),
                                  "locus insertion tables", timer)) return rc;
    if (U.anchors.reserve(np * INSERTION_COLUMNS) || U.records.reserve(std::max<size_t>(nr, 1))) return MIPGEN_E_NOMEM;
    {
        IdleOnExit idle{h->stream};
        HIP_TRY(hipMemcpyAsync(U.anchors.p, anchors, np * INSERTION_COLUMNS * 4, hipMemcpyHostToDevice, h->stream));
        if (nr) HIP_TRY(hipMemcpyAsync(U.records.p, records, nr * sizeof(mipgen_insertion_record), hipMemcpyHostToDevice, h->stream));
    }
    if (int rc = fold_insertions(h, U.plan, U.map, U.fold, U.records.p, n_records, U.anchors.p, timer, locus_anchors, totals)) return rc;
    return booked(timer, &h->locus_ins_ms);
}

// The locus records of the last fold the handle made - the tables call, the locus insertions call or the locus insertion call -, in ascending key order.
int mipgen_accel_locus_insertions_fetch(mipgen_accel* h, mipgen_insertion_record* records, int64_t n)
{
    if (!h) return fail(MIPGEN_E_INVALID, "null handle");
    return fetch_records(h, h->locus_ins.fold.records, h->locus_ins.fold.n_alleles,
                         "the handle holds no locus insertion alleles: mipgen_accel_locus_insertion_tables or mipgen_accel_reads_consensus_locus_insertions leaves them",
                         "locus insertions call", records, n);
}

// The insertion alleles of one row (4.16, into R->ins) folded under the installed plan.  Writes R->ins, R->locus_ins.map and the handle's fold.
int mipgen_accel_reads_consensus_locus_insertions(mipgen_accel* h, const char* mol_seq, const int32_t* mol_len, int32_t n, int32_t row, int32_t min_family, int32_t min_quality,
                                                  int32_t max_indel, int32_t* counts, int32_t* anchors, int32_t* locus_anchors, mipgen_insertion_totals* ins_totals,
                                                  mipgen_locus_insertion_totals* totals)
{
    RowPlan P;
    const RowArgs A{mol_seq, mol_len, n, min_family, min_quality, max_indel, true, true, true};
    if (int rc = plan_insertions(h, A, row, &P)) return rc;
    if (int rc = check_locus_session(P.R->locus, P)) return rc;
    h->locus_ins_ms = -1.0;
    SpanTimer timer{h->timing, h->stream};
    if (int rc = locus_insertions_row(h, P, A, row, timer, counts, anchors, locus_anchors, ins_totals, totals)) return rc;
    return booked(timer, &h->locus_ins_ms);
}

// The sparse pool over the sample rows, per locus: 4.17's pool with every row folded between its insertions and the append.  Writes R->locus_ins and, through the
// insertions route of every row, R->ins.
int mipgen_accel_reads_consensus_locus_insertion_pool(mipgen_accel* h, const char* mol_seq, const int32_t* mol_len, int32_t n, int32_t min_family, int32_t min_quality,
                                                      int32_t max_indel, int32_t bg_max_ppm, mipgen_insertion_pool_totals* totals)
{
    RowPlan P;
    const RowArgs A{mol_seq, mol_len, n, min_family, min_quality, max_indel, true, true, true};
    if (int rc = plan_insertions(h, A, 0, &P)) return rc;
    if (int rc = check_bg_max_ppm(bg_max_ppm)) return rc;
    if (int rc = check_locus_session(P.R->locus, P)) return rc;
    InsPool& Q = P.R->locus_ins.pool;
    Q.args.have = false;                                                 // (a pool that fails leaves none)
    h->locus_ins_ms = -1.0;
    LocusInsFold& F = h->locus_ins.fold;
    SpanTimer timer{h->timing, h->stream};
    const int built = build_ins_pool(h, P, A, bg_max_ppm, timer, Q, P.R->locus.plan.n_loci, "locus insertion pool",
                                     [&](int32_t r, const int32_t** anchors, const mipgen_insertion_record** records, int64_t* n_rec) {
            if (int rc = locus_insertions_row(h, P, A, r, timer, nullptr, nullptr, nullptr, nullptr, nullptr)) return rc;
            *anchors = F.anchors.p; *records = F.records.p; *n_rec = F.n_alleles;
            return (int)MIPGEN_OK;
        });
    F.n_alleles = -1;                                                    // (the locus records of the last sample row are no call's result)
    if (built) return built;
    if (totals) *totals = {Q.rows, Q.n_entries, Q.n_alleles};
    return booked(timer, &h->locus_ins_ms);
}

// The distinct records of the locus insertion pool, in ascending key order, and S over the loci.
int mipgen_accel_locus_insertion_pool_fetch(mipgen_accel* h, mipgen_insertion_pool_record* pool_records, int64_t n, int32_t* pool_span)
{
    if (int rc = check_reads(h)) return rc;
    const InsPool& Q = h->consensus->locus_ins.pool;
    if (!Q.args.have) return fail(MIPGEN_E_STATE, "the consensus reads have no locus insertion pool: mipgen_accel_reads_consensus_locus_insertion_pool builds it");
    return fetch_ins_pool(h, Q, pool_records, n, pool_span);
}

// The insertion calls of one row per locus against the locus insertion pool: the row's insertions recomputed with the pool's arguments and folded, then 4.17's
// flag, tail, order and join over the locus records and the locus anchor table, into a run of its own.
int mipgen_accel_reads_consensus_locus_insertion_call(mipgen_accel* h, int32_t row, const mipgen_call_params* params, int32_t* counts, int32_t* anchors, int32_t* locus_anchors,
                                                      mipgen_insertion_totals* ins_totals, mipgen_locus_insertion_totals* locus_totals, mipgen_call_totals* call_totals)
{
    if (int rc = check_reads(h)) return rc;
    const LocusScratch& L = h->consensus->locus;
    const InsPool& Q = h->consensus->locus_ins.pool;
    if (!L.plan.have) return fail(MIPGEN_E_STATE, "the consensus reads have no locus plan: mipgen_accel_reads_consensus_locus_plan installs it");
    if (!Q.args.have) return fail(MIPGEN_E_STATE, "the consensus reads have no locus insertion pool: mipgen_accel_reads_consensus_locus_insertion_pool builds it");
    RowPlan P;
    RowArgs A;
    if (int rc = plan_call(h, Q.args, row, params, "locus insertion pool", &A, &P)) return rc;
    A.need_seq = A.must_place = A.runs = true;
    h->locus_ins_ms = -1.0;
    h->locus_ins_call.n_calls = -1;
    SpanTimer timer{h->timing, h->stream};
    if (int rc = locus_insertions_row(h, P, A, row, timer, counts, anchors, locus_anchors, ins_totals, locus_totals)) return rc;
    const LocusInsFold& F = h->locus_ins.fold;
    if (int rc = run_ins_call(h, h->locus_ins_call, F.records.p, F.n_alleles, F.anchors.p, INSERTION_COLUMNS, L.plan.n_loci, Q.pool_keys.p, Q.pool_sums.p, Q.n_alleles, Q.S.p,
                              (int64_t)row < sample_rows(P.R), *params, timer, call_totals)) return rc;
    return booked(timer, &h->locus_ins_ms);
}

// The records of the last insertion call per locus, in ascending allele-key order; pos is the locus.
int mipgen_accel_locus_insertion_call_fetch(mipgen_accel* h, mipgen_insertion_call_record* records, int64_t n)
{
    if (!h) return fail(MIPGEN_E_INVALID, "null handle");
    return fetch_records(h, h->locus_ins_call.out, h->locus_ins_call.n_calls,
                         "the handle holds no locus insertion calls: mipgen_accel_reads_consensus_locus_insertion_call leaves them", "locus insertion call", records, n);
}

}  // extern "C"
