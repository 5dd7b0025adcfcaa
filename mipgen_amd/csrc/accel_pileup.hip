// accel_pileup.hip — the two pileups read off the consensus reads a session left on the handle: allele counts per template position of one row (DESIGN 4.12:
// mipgen_accel_reads_consensus_pileup) and the same with indels (4.13: _consensus_pileup_gapped).  Both are plan_row (every check, nothing allocated or launched),
// the call's own budget term, prepare_row (the row's buffers, the cell boundaries and the (cell, round) units: a filled PileRow), then the call's own launches,
// download and totals.  Each call writes its own scratch of the ConsensusResult only (pile / gapped), so neither touches what the other holds.
#include "accel_internal.h"
#include "gapped_align.h"

struct GappedArgs { const char* mol_seq; int32_t max_indel; };         // what the gapped call adds to the arguments of a row

struct RowPlan {
    ConsensusResult* R = nullptr;
    int64_t n_pos = 0, n_units = 0;                                      // template positions; rounds of 64 of them
    int32_t max_len = 0;
    size_t bytes = 0;                                                    // the device memory RowScratch takes at most
};

static size_t padded(size_t count, size_t size) { return (count + count / 8 + 64) * size; }      // (what DevBuf::reserve asks for at most)

// Every refusal of a pileup call, in one order for both; G: the gapped call's arguments (molecules are then bounded by MIPGEN_GAPPED_MAX_MOL), or nullptr.
static int plan_row(mipgen_accel* h, const int32_t* mol_len, int32_t n, int32_t row, int32_t min_family, int32_t min_quality, const GappedArgs* G, RowPlan* P)
{
    if (!h) return fail(MIPGEN_E_INVALID, "null handle");
    if (!h->consensus) return fail(MIPGEN_E_STATE, "the handle holds no consensus reads: mipgen_accel_reads_finish_consensus leaves them, the next mipgen_accel_reads_open* drops them");
    const ConsensusResult* R = P->R = h->consensus;
    if (!mol_len) return fail(MIPGEN_E_INVALID, "bad arguments: no molecule lengths");
    if (G && !G->mol_seq) return fail(MIPGEN_E_INVALID, "bad arguments: no template bases");
    if ((int64_t)n != R->n) return fail(MIPGEN_E_INVALID, "%d molecule lengths: the session that left the consensus reads had %lld probes", n, (long long)R->n);
    for (int32_t p = 0; p < n; p++) {
        if (mol_len[p] < 1) return fail(MIPGEN_E_INVALID, "molecule length %d of probe %d: a length is 1 or more", mol_len[p], p);
        if (G && mol_len[p] > MIPGEN_GAPPED_MAX_MOL)
            return fail(MIPGEN_E_INVALID, "molecule length %d of probe %d: the gapped pileup places molecules of at most %d bases", mol_len[p], p, MIPGEN_GAPPED_MAX_MOL);
        P->n_pos += mol_len[p]; P->n_units += ((int64_t)mol_len[p] + 63) / 64; P->max_len = std::max(P->max_len, mol_len[p]);
    }
    if (row < 0 || (int64_t)row >= R->rows) return fail(MIPGEN_E_INVALID, "row %d: the session had %lld row%s", row, (long long)R->rows, R->rows == 1 ? "" : "s");
    if (min_family < 1) return fail(MIPGEN_E_INVALID, "min_family %d: 1 or more", min_family);
    if (min_quality < 0 || min_quality > 40) return fail(MIPGEN_E_INVALID, "min_quality %d: 0 to 40 (the consensus writes 2 to 40)", min_quality);
    if (G && (G->max_indel < 1 || G->max_indel > GAP_MAX_INDEL)) return fail(MIPGEN_E_INVALID, "max_indel %d: 1 to %d", G->max_indel, GAP_MAX_INDEL);
    if (P->n_units > 0x7fffffff) return fail(MIPGEN_E_INVALID, "%lld template positions: more than 2^31 - 1 rounds of 64", (long long)P->n_pos);
    P->bytes = padded((size_t)n, 4) + padded((size_t)n, 8) + padded((size_t)n + 1, 4) + padded((size_t)P->n_units, 8) + padded(1, sizeof(PileupCounters));
    HIP_TRY(hipSetDevice(h->device));
    return MIPGEN_OK;
}

// The row's buffers filled and its kernels run (timed as one span of `timer`): *row is complete, *pc holds `used`, [*first, *last) are the row's groups.
// what: the call's name in a message.
static int prepare_row(mipgen_accel* h, const RowPlan& P, RowScratch& W, const char* what, const int32_t* mol_len, int32_t n, int32_t row, int32_t min_family,
                       int32_t min_quality, SpanTimer& timer, PileRow* out, PileupCounters* pc, uint32_t* first, uint32_t* last)
{
    const ConsensusResult* R = P.R;
    if (W.mol_len.reserve((size_t)n) || W.pos_off.reserve((size_t)n) || W.start.reserve((size_t)n + 1) || W.units.reserve((size_t)P.n_units) || W.pctr.reserve(1))
        return MIPGEN_E_NOMEM;
    std::vector<int64_t> pos_off((size_t)n);
    for (int64_t p = 0, at = 0; p < n; at += mol_len[p], p++) pos_off[(size_t)p] = at;
    hipStream_t st = h->stream;
    IdleOnExit idle{st};                                                 // (pos_off outlives its copy)
    HIP_TRY(hipMemcpyAsync(W.mol_len.p, mol_len, (size_t)n * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(W.pos_off.p, pos_off.data(), (size_t)n * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(W.pctr.p, 0, sizeof(PileupCounters), st));
    *out = {W.units.p, 0, 0, W.start.p, W.mol_len.p, W.pos_off.p, n, P.n_pos, (uint32_t)((int64_t)row * R->n), min_family, min_quality};
    timer.mark();
    HIP_TRY(mipgen_launch_pileup_prepare(st, R->view(), *out, P.n_units, W.start.p, W.units.p, W.pctr.p));
    timer.mark();
    HIP_TRY(hipMemcpyAsync(pc, W.pctr.p, sizeof *pc, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(first, W.start.p, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(last, W.start.p + n, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(idle.wait());
    out->n_small = (int64_t)pc->n_small; out->n_big = (int64_t)pc->n_big;
    if (out->n_small + out->n_big != P.n_units)
        return fail(MIPGEN_E_STATE, "%s: %lld + %lld rounds listed of %lld", what, (long long)out->n_small, (long long)out->n_big, (long long)P.n_units);
    return MIPGEN_OK;
}

extern "C" {

// Allele counts per template position of one row from the consensus reads the handle holds.  Reads R's groups and reads; writes R->pile only.
int mipgen_accel_reads_consensus_pileup(mipgen_accel* h, const int32_t* mol_len, int32_t n, int32_t row, int32_t min_family, int32_t min_quality, int32_t* counts,
                                        mipgen_pileup_totals* totals)
{
    RowPlan P;
    if (int rc = plan_row(h, mol_len, n, row, min_family, min_quality, nullptr, &P)) return rc;
    const ConsensusResult* R = P.R;
    h->pileup_ms = -1.0;
    if (R->n_groups == 0) {                                              // (no buffer exists: nothing to read, nothing to launch)
        if (counts) memset(counts, 0, (size_t)P.n_pos * PILEUP_COLUMNS * sizeof(int32_t));
        if (totals) *totals = {0, 0, 0, 0};
        return MIPGEN_OK;
    }
    PileupScratch& W = P.R->pile;
    const size_t need = P.bytes + padded((size_t)P.n_pos * PILEUP_COLUMNS, 4);
    size_t free_b = 0;
    if (int rc = free_device_bytes(&free_b)) return rc;
    if (need > W.held() + free_b)
        return fail(MIPGEN_E_NOMEM, "pileup: %lld template positions need %zu MiB of device memory, %zu MiB are free", (long long)P.n_pos, need >> 20, (W.held() + free_b) >> 20);
    if (W.counts.reserve((size_t)P.n_pos * PILEUP_COLUMNS)) return MIPGEN_E_NOMEM;
    hipStream_t st = h->stream;
    IdleOnExit idle{st};
    SpanTimer pile_time{h->timing, st};
    PileRow Row;
    PileupCounters pc;
    uint32_t first = 0, last = 0;                                        // the row's groups: [first, last)
    if (int rc = prepare_row(h, P, W.row, "pileup", mol_len, n, row, min_family, min_quality, pile_time, &Row, &pc, &first, &last)) return rc;
    pile_time.mark();
    HIP_TRY(mipgen_launch_pileup(st, R->view(), Row, P.n_units, W.counts.p, W.row.pctr.p));
    pile_time.mark();
    HIP_TRY(hipMemcpyAsync(&pc, W.row.pctr.p, sizeof pc, hipMemcpyDeviceToHost, st));
    if (counts) HIP_TRY(hipMemcpyAsync(counts, W.counts.p, (size_t)P.n_pos * PILEUP_COLUMNS * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(idle.wait());
    double ms = 0.0;
    if (pile_time.add_to(&ms)) h->pileup_ms = ms;
    if (totals) *totals = {(int64_t)last - (int64_t)first, (int64_t)pc.used, (int64_t)pc.bases, (int64_t)pc.discordant};
    return MIPGEN_OK;
}

// The pileup with indels of one row.  Reads R's groups and reads; writes R->gapped only.
int mipgen_accel_reads_consensus_pileup_gapped(mipgen_accel* h, const char* mol_seq, const int32_t* mol_len, int32_t n, int32_t row, int32_t min_family, int32_t min_quality,
                                               int32_t max_indel, int32_t* counts, mipgen_gapped_totals* totals)
{
    RowPlan P;
    const GappedArgs args{mol_seq, max_indel};
    if (int rc = plan_row(h, mol_len, n, row, min_family, min_quality, &args, &P)) return rc;
    const ConsensusResult* R = P.R;
    h->gapped_ms = -1.0;
    if (R->n_groups == 0) {
        if (counts) memset(counts, 0, (size_t)P.n_pos * GAPPED_COLUMNS * sizeof(int32_t));
        if (totals) *totals = {0, 0, 0, 0, 0, 0, 0, 0};
        return MIPGEN_OK;
    }
    GappedScratch& W = P.R->gapped;
    // the budget, before anything is allocated: the row's groups are not known yet, so every buffer that grows with them is taken at the session's groups, and a
    // projection at the longest template
    const size_t G = (size_t)R->n_groups, n_pos = (size_t)P.n_pos;
    const size_t need = P.bytes + padded(n_pos * GAPPED_COLUMNS, 4) + padded(n_pos, 1) + padded(2 * G, 8) + padded(2 * G, 4) + padded(2 * G, 1) +
                        padded(2 * G * 3 * (size_t)P.max_len, 1) + padded(1, sizeof(GappedCounters));
    size_t free_b = 0;
    if (int rc = free_device_bytes(&free_b)) return rc;
    if (need > W.held() + free_b)
        return fail(MIPGEN_E_NOMEM, "gapped pileup: %lld template positions and %lld groups need up to %zu MiB of device memory, %zu MiB are free", (long long)P.n_pos,
                    (long long)R->n_groups, need >> 20, (W.held() + free_b) >> 20);
    if (W.counts.reserve(n_pos * GAPPED_COLUMNS) || W.mol_seq.reserve(n_pos) || W.ctr.reserve(1)) return MIPGEN_E_NOMEM;
    hipStream_t st = h->stream;
    IdleOnExit idle{st};
    HIP_TRY(hipMemcpyAsync(W.mol_seq.p, mol_seq, n_pos, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(W.ctr.p, 0, sizeof(GappedCounters), st));
    SpanTimer gap_time{h->timing, st};
    PileRow Row;
    PileupCounters pc;
    GappedCounters gc;
    memset(&gc, 0, sizeof gc);
    uint32_t first = 0, last = 0;                                        // the row's groups: [first, last)
    if (int rc = prepare_row(h, P, W.row, "gapped pileup", mol_len, n, row, min_family, min_quality, gap_time, &Row, &pc, &first, &last)) return rc;
    const ConsensusView C = R->view();
    const int64_t n_row = (int64_t)last - (int64_t)first;
    if (n_row < 0 || n_row > R->n_groups) return fail(MIPGEN_E_STATE, "gapped pileup: groups [%u, %u) of %lld", first, last, (long long)R->n_groups);
    if (n_row > 0) {
        if (W.need.reserve(2 * (size_t)n_row) || W.list.reserve(2 * (size_t)n_row) || W.proj_off.reserve(2 * (size_t)n_row)) return MIPGEN_E_NOMEM;
        gap_time.mark();
        HIP_TRY(mipgen_launch_gap_list(st, C, Row, W.mol_seq.p, first, n_row, max_indel, W.need.p, W.list.p, W.proj_off.p, W.ctr.p));
        gap_time.mark();
        HIP_TRY(hipMemcpyAsync(&gc, W.ctr.p, sizeof gc, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if ((int64_t)gc.n_sides > 2 * n_row || gc.proj_bytes > (unsigned long long)gc.n_sides * 3ull * (unsigned long long)P.max_len)
            return fail(MIPGEN_E_STATE, "gapped pileup: %llu sides listed of %lld, %llu projection bytes", gc.n_sides, (long long)(2 * n_row), gc.proj_bytes);
        if (gc.proj_bytes && W.proj.reserve((size_t)gc.proj_bytes)) return MIPGEN_E_NOMEM;
    }
    gap_time.mark();
    HIP_TRY(mipgen_launch_gapped(st, C, Row, P.n_units, W.mol_seq.p, first, max_indel, P.max_len, W.list.p, (int64_t)gc.n_sides, W.proj_off.p, W.proj.p, W.counts.p, W.ctr.p));
    gap_time.mark();
    HIP_TRY(hipMemcpyAsync(&gc, W.ctr.p, sizeof gc, hipMemcpyDeviceToHost, st));
    if (counts) HIP_TRY(hipMemcpyAsync(counts, W.counts.p, n_pos * GAPPED_COLUMNS * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(idle.wait());
    double ms = 0.0;
    if (gap_time.add_to(&ms)) h->gapped_ms = ms;
    if (totals)
        *totals = {n_row, (int64_t)pc.used, (int64_t)gc.bases, (int64_t)gc.discordant, (int64_t)gc.deletions, (int64_t)gc.insertions, (int64_t)gc.ins_discordant,
                   (int64_t)gc.gapped_sides};
    return MIPGEN_OK;
}

}  // extern "C"
