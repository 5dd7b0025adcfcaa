// accel_reads.hip — read sessions behind the C ABI: reads and unique tags per probe from smMIP read pairs (mipgen_accel_reads_open / _feed / _finish), per sample of
// a multiplexed lane (4.10: _open_samples / _feed_samples / _finish_samples / _last_samples), with one consensus read pair per molecule (4.11: _open_consensus / _feed_consensus /
// _finish_consensus / _consensus_fetch; the pileups read off the ConsensusResult a finish leaves on the handle are accel_pileup.hip's).  The three families of entry points name ONE path.  ReadsSession is what every session has plus a KeyList, a SamplesPart and a
// ConsensusPart; its flags `samples` and `consensus` say which parts are set up, and session_for() alone matches a call to the open session.  open_impl: check_open
// (probe table, then barcodes), build_host_tables, the budget, upload_tables.  feed_impl: eleven stages, the kinds differing in data only - where the bases of the call live and where
// k_read_assign's keys go.  finish_session: consensus_finish where reads were kept - with merge_tags between its runs and its partition when the session was told to correct its
// tags (4.20: mipgen_accel_reads_set_tag_mismatches / _last_tag_merge / _tag_map_fetch) -, finish_impl, release.  Errors are HIP_TRY returns; IdleOnExit and FreeOnExit put the
// stream and a chunk's block right on every way out, SpanTimer books HIP-event times.  A session owns every buffer it uses; of the handle it takes the device and the stream.
#include "accel_internal.h"
#include "tag_merge.h"

struct SeedTableBufs {
    DevBuf<uint32_t> slots, start;
    DevBuf<uint64_t> keys;
    DevBuf<int32_t> probes;
    SeedTable view{};
    void release() { slots.release(); start.release(); keys.release(); probes.release(); }
};

// one feed call of a consensus session, retained: ONE device block (ChunkLayout) with the records, keys and pair ids of its pairs and their bases and qualities
struct ArenaChunk { uint8_t* block; size_t bytes; int64_t pair0, n; };

// the parts of a chunk's block, each at a multiple of 8 bytes: the quality of a base lies `qdelta` bytes behind it on both sides
struct ChunkLayout {
    size_t recs, keys, ids, ext, lig, ext_qual, lig_qual, total;
    int64_t qdelta;
    ChunkLayout(int64_t n, size_t eb, size_t lb)
    {
        auto pad8 = [](size_t b) { return (b + 7) & ~(size_t)7; };
        recs = 0; keys = recs + (size_t)n * sizeof(ConsensusPair); ids = keys + (size_t)n * 8; ext = ids + pad8((size_t)n * 4);
        lig = ext + pad8(eb); ext_qual = lig + pad8(lb); lig_qual = ext_qual + pad8(eb);
        total = lig_qual + pad8(lb) + 8;                     // (+ 8: k_read_assign fetches aligned 32-bit words, up to 5 bytes beyond the last read)
        qdelta = (int64_t)(pad8(eb) + pad8(lb));
    }
};

static const int64_t READS_KEY_CAP_DEFAULT = (int64_t)1 << 26, READS_KEY_CAP_MAX = (int64_t)1 << 30;

// an arm as bit planes (reads_common.h); rc: of its reverse complement
static void pack_arm(const char* s, int len, bool rc, uint64_t* p0, uint64_t* p1, uint64_t* bad)
{
    *p0 = *p1 = *bad = 0;
    for (int i = 0; i < len; i++) {
        uint32_t c = reads_base_code((uint8_t)(rc ? s[len - 1 - i] : s[i]));
        if (rc && c < 4u) c = 3u - c;
        *p0 |= (uint64_t)(c & 1u) << i; *p1 |= (uint64_t)((c >> 1) & 1u) << i; *bad |= (uint64_t)(c >> 2) << i;
    }
}

struct HostSeedTable { std::vector<uint32_t> slots, start; std::vector<uint64_t> keys; std::vector<int32_t> probes; };

// (key, probe) of every probe whose seed holds A C G T only -> distinct keys ascending, the probes of each ascending, the hash in front
static void build_seed_table(std::vector<std::pair<uint64_t, int32_t>>& kp, HostSeedTable& T)
{
    std::sort(kp.begin(), kp.end());
    T.start.push_back(0);
    for (size_t i = 0; i < kp.size(); i++) {
        if (i == 0 || kp[i].first != kp[i - 1].first) { if (i) T.start.push_back((uint32_t)i); T.keys.push_back(kp[i].first); }
        T.probes.push_back(kp[i].second);
    }
    if (!kp.empty()) T.start.push_back((uint32_t)kp.size());
    size_t n_slots = 16;
    while (n_slots < 2 * T.keys.size()) n_slots *= 2;
    T.slots.assign(n_slots, 0u);
    for (size_t k = 0; k < T.keys.size(); k++) {
        uint32_t s = reads_hash(T.keys[k]) & (uint32_t)(n_slots - 1);
        while (T.slots[s]) s = (s + 1) & (uint32_t)(n_slots - 1);
        T.slots[s] = (uint32_t)k + 1;
    }
    if (T.keys.empty()) { T.keys.push_back(0); T.probes.push_back(0); T.start.push_back(0); }      // (never read: every slot is empty)
}

static int upload_seed_table(mipgen_accel* h, const HostSeedTable& T, SeedTableBufs& B)
{
    if (B.slots.reserve(T.slots.size()) || B.start.reserve(T.start.size()) || B.keys.reserve(T.keys.size()) || B.probes.reserve(T.probes.size())) return MIPGEN_E_NOMEM;
    HIP_TRY(hipMemcpyAsync(B.slots.p, T.slots.data(), T.slots.size() * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(B.start.p, T.start.data(), T.start.size() * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(B.keys.p, T.keys.data(), T.keys.size() * sizeof(uint64_t), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(B.probes.p, T.probes.data(), T.probes.size() * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    B.view = {B.slots.p, B.keys.p, B.start.p, B.probes.p, (uint32_t)(T.slots.size() - 1)};
    return MIPGEN_OK;
}

// the barcode hash of a samples session: every barcode, and at d = 1 every one-substitution neighbour of every barcode.  A neighbour
// that IS another barcode belongs to that barcode (distance 0 wins); one claimed by two barcodes is ambiguous.  (key, kind, sample) sorted: the
// entries of a key are adjacent, an exact one first.
static void build_sample_table(const char* const* barcodes, int n_samples, int J, int d, std::vector<SampleSlot>& slots)
{
    struct Entry { uint64_t key; uint32_t kind; int32_t sample; };
    std::vector<Entry> all;
    all.reserve((size_t)n_samples * (d ? 1 + 3 * (size_t)J : 1));
    const uint64_t jmask = reads_len_mask(J);
    for (int s = 0; s < n_samples; s++) {
        uint64_t p0, p1, bad;
        pack_arm(barcodes[s], J, false, &p0, &p1, &bad);
        all.push_back({reads_seed_key(p0, p1, jmask), SAMPLE_SLOT_EXACT, s});
        if (!d) continue;
        for (int j = 0; j < J; j++) {
            const uint64_t bit = 1ull << j;
            const uint32_t own = (uint32_t)((p0 >> j) & 1u) | ((uint32_t)((p1 >> j) & 1u) << 1);
            for (uint32_t c = 0; c < 4; c++) {
                if (c == own) continue;
                const uint64_t q0 = (p0 & ~bit) | ((c & 1u) ? bit : 0ull), q1 = (p1 & ~bit) | ((c & 2u) ? bit : 0ull);
                all.push_back({reads_seed_key(q0, q1, jmask), SAMPLE_SLOT_NEIGHBOUR, s});
            }
        }
    }
    std::sort(all.begin(), all.end(), [](const Entry& a, const Entry& b) { return a.key != b.key ? a.key < b.key : a.kind != b.kind ? a.kind < b.kind : a.sample < b.sample; });
    std::vector<SampleSlot> distinct;
    for (size_t i = 0; i < all.size();) {
        size_t j = i + 1;
        while (j < all.size() && all[j].key == all[i].key) j++;
        SampleSlot e{all[i].key, all[i].sample, all[i].kind};
        if (all[i].kind == SAMPLE_SLOT_NEIGHBOUR && j - i > 1) e.sample = SAMPLE_AMBIGUOUS;
        distinct.push_back(e);
        i = j;
    }
    size_t n_slots = 16;
    while (n_slots < 2 * distinct.size()) n_slots *= 2;
    slots.assign(n_slots, SampleSlot{0, 0, SAMPLE_SLOT_EMPTY});
    for (const SampleSlot& e : distinct) {
        uint32_t s = reads_hash(e.key) & (uint32_t)(n_slots - 1);
        while (slots[s].kind != SAMPLE_SLOT_EMPTY) s = (s + 1) & (uint32_t)(n_slots - 1);
        slots[s] = e;
    }
}

struct FreeOnExit { void* p; ~FreeOnExit() { if (p) (void)hipFree(p); } };

// The (cell, tag) keys of a plain or samples session, sorted and duplicate-free between feed calls.  A consensus session keeps no list: its `keys` is the scratch
// k_read_assign writes a chunk's keys to (cap stays 0), and `end_bit` serves the sort of its finish; `sort_temp` stays unreserved, as sort_unique is never reached.
struct KeyList {
    DevBuf<uint64_t> keys, keys_alt;
    DevBuf<char> sort_temp;
    int64_t cap = 0;                                         // entries of `keys` in use as capacity
    int64_t ub = 0;                                          // no more keys than this are in the buffer (every pair fed since the last sort-unique counted)
    int end_bit = 64;                                        // key bits that can be set
    void release() { keys.release(); keys_alt.release(); sort_temp.release(); }

    // keys[0, n) sorted and made duplicate-free; ub becomes their exact number (n_keys: the session's device counter of keys written)
    int sort_unique(mipgen_accel* h, unsigned long long* n_keys)
    {
        unsigned long long n = 0;
        HIP_TRY(hipMemcpyAsync(&n, n_keys, sizeof n, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        if ((int64_t)n > cap) return fail(MIPGEN_E_STATE, "read counter: %llu keys in a buffer of %lld", n, (long long)cap);
        if (n > 0) {
            size_t temp_bytes = 0;
            HIP_TRY(mipgen_reads_sort_unique(h->stream, nullptr, &temp_bytes, keys.p, keys_alt.p, (int64_t)n, end_bit, n_keys));
            if (sort_temp.reserve(temp_bytes + 16)) return MIPGEN_E_NOMEM;
            temp_bytes = sort_temp.cap;
            HIP_TRY(mipgen_reads_sort_unique(h->stream, sort_temp.p, &temp_bytes, keys.p, keys_alt.p, (int64_t)n, end_bit, n_keys));
            HIP_TRY(hipMemcpyAsync(&n, n_keys, sizeof n, hipMemcpyDeviceToHost, h->stream));
            HIP_TRY(hipStreamSynchronize(h->stream));
        }
        ub = (int64_t)n;
        return MIPGEN_OK;
    }

    // room for `want` more keys (at least 1): sort-unique what is there, and double the buffer while more than half of it is distinct keys
    int make_room(mipgen_accel* h, unsigned long long* n_keys, int64_t want, int64_t* room)
    {
        if (cap - ub < std::min(want, std::max<int64_t>(cap / 2, 1))) {
            if (int rc = sort_unique(h, n_keys)) return rc;
            while (cap - ub < std::max<int64_t>(cap / 2, 1)) {
                const int64_t grown_cap = cap * 2;
                size_t free_b = 0;
                if (int rc = free_device_bytes(&free_b)) return rc;
                if (grown_cap > READS_KEY_CAP_MAX || (size_t)grown_cap * 16 + ((size_t)64 << 20) > free_b)
                    return fail(MIPGEN_E_NOMEM, "read counter: %lld distinct (probe, tag) keys do not fit device memory (%zu MiB free)", (long long)ub, free_b >> 20);
                DevBuf<uint64_t> grown;
                if (grown.reserve((size_t)grown_cap)) return MIPGEN_E_NOMEM;
                if (ub) HIP_TRY(hipMemcpyAsync(grown.p, keys.p, (size_t)ub * sizeof(uint64_t), hipMemcpyDeviceToDevice, h->stream));
                HIP_TRY(hipStreamSynchronize(h->stream));
                keys.release(); keys_alt.release();
                keys = grown;
                if (keys_alt.reserve((size_t)grown_cap)) return MIPGEN_E_NOMEM;
                cap = grown_cap;
            }
        }
        *room = cap - ub;
        return MIPGEN_OK;
    }
};

// a session with samples: the barcode table, the index reads of the current feed call and what k_sample_assign makes of them
struct SamplesPart {
    SampleTable table{};
    DevBuf<SampleSlot> slots;
    DevBuf<uint8_t> idx_bytes; DevBuf<int64_t> idx_off;      // the index reads of the current feed call
    DevBuf<int32_t> row, sample_index;                       // ... and the row and sample of each of its pairs
    DevBuf<unsigned long long> row_pairs;
    DevBuf<SampleCounters> ctr;
    void release() { slots.release(); idx_bytes.release(); idx_off.release(); row.release(); sample_index.release(); row_pairs.release(); ctr.release(); }
};

// a session that keeps its reads: every feed call's chunk stays resident, within a budget of arena_cap bytes; c_*: the scratch of finish
struct ConsensusPart {
    std::vector<ArenaChunk> chunks;
    size_t arena_cap = 0, arena_used = 0; int64_t total_pairs = 0;
    DevBuf<ConsensusCounters> ctr;
    SortedPairs pairs;                                       // the (key, pair id) of every pair, as fed and sorted; its scratch serves every scan of finish too
    DevBuf<uint32_t> c_start, c_order;
    DevBuf<ConsensusPair> c_recs;
    DevBuf<int64_t> c_ext_len, c_lig_len;
    int32_t tag_mismatches = 0;                              // mipgen_accel_reads_set_tag_mismatches; at 0 nothing below is reserved
    DevBuf<int32_t> t_parent;                                // the parent of every raw group
    DevBuf<TagMergeCounters> t_ctr;
    void release()
    {
        for (const ArenaChunk& c : chunks) (void)hipFree(c.block);
        chunks.clear();
        ctr.release(); pairs.release(); c_start.release(); c_order.release(); c_recs.release();
        c_ext_len.release(); c_lig_len.release(); t_parent.release(); t_ctr.release();
    }
};

struct ReadsSession {
    ReadsParams P{};
    bool samples = false, consensus = false;                 // which parts are set up: smp / cons (and no key list: see KeyList)
    int64_t rows = 1;                                        // n_samples + 1 with samples; the count matrices hold rows * n_probes cells
    DevBuf<ReadProbe> probes;
    SeedTableBufs ext_seeds, lig_seeds;
    DevBuf<unsigned long long> reads, unique;
    DevBuf<ReadsCounters> ctr;
    DevBuf<uint8_t> ext_bytes, lig_bytes;                    // the pairs of the current feed call (a consensus session: in the chunk's block instead)
    DevBuf<int64_t> ext_off, lig_off;
    DevBuf<int32_t> assign;
    int64_t last_pairs = 0;
    KeyList keys;
    SamplesPart smp;
    ConsensusPart cons;
    void release()
    {
        cons.release(); smp.release(); keys.release();
        probes.release(); ext_seeds.release(); lig_seeds.release(); reads.release(); unique.release(); ctr.release();
        ext_bytes.release(); lig_bytes.release(); ext_off.release(); lig_off.release(); assign.release();
    }
};

enum { KIND_PLAIN = 0, KIND_SAMPLES = 1, KIND_CONSENSUS = 2 };      // the three families of entry points

// The open session in *S when a call of `kind` (feed: a feed call; otherwise a finish) is the one that serves it.  If not, the refusal names the entry point that does.
static int session_for(mipgen_accel* h, int kind, bool feed, ReadsSession** S)
{
    ReadsSession* s = h->reads;
    if (!s) return fail(MIPGEN_E_STATE, "no read-counting session is open");
    const char *verb = feed ? "feed" : "finish", *does = feed ? "feeds" : "closes";
    if (s->consensus && kind != KIND_CONSENSUS) return fail(MIPGEN_E_STATE, "the open session is a consensus session: mipgen_accel_reads_%s_consensus %s it", verb, does);
    if (!s->consensus && kind == KIND_CONSENSUS)
        return feed ? fail(MIPGEN_E_STATE, "the open session keeps no reads: it was not opened by mipgen_accel_reads_open_consensus")
                    : fail(MIPGEN_E_STATE, "the open session keeps no reads: mipgen_accel_reads_finish%s closes it", s->samples ? "_samples" : "");
    if (!s->consensus && s->samples != (kind == KIND_SAMPLES))
        return fail(MIPGEN_E_STATE, "the open session has %s: mipgen_accel_reads_%s%s %s it", s->samples ? "samples" : "no samples", verb, s->samples ? "_samples" : "", does);
    *S = s;
    return MIPGEN_OK;
}

// Every check of an open, in the order in which the refusals win, before anything is built or allocated.  *shortest: the shortest arm; *J: the length of the barcodes.
static int check_open(mipgen_accel* h, const mipgen_probe* probes, int32_t n, int32_t ext_tag, int32_t lig_tag, int32_t max_mismatches, const char* const* barcodes, int32_t n_samples,
                      int32_t barcode_mismatches, bool consensus, int64_t arena_bytes, size_t* shortest, int* J)
{
    // the probe table and the session's numbers
    if (!h || !probes || n < 1) return fail(MIPGEN_E_INVALID, "bad arguments");
    if (ext_tag < 0 || lig_tag < 0 || ext_tag + lig_tag > READS_MAX_TAG) return fail(MIPGEN_E_INVALID, "tag sizes %d,%d: at most %d tag bases in all", ext_tag, lig_tag, READS_MAX_TAG);
    if (consensus && ext_tag + lig_tag == 0) return fail(MIPGEN_E_INVALID, "tag sizes 0,0: without tag bases there are no molecules to collapse");
    if (consensus && arena_bytes < 0) return fail(MIPGEN_E_INVALID, "arena_bytes %lld is negative", (long long)arena_bytes);
    if (max_mismatches < 0 || max_mismatches > 2) return fail(MIPGEN_E_INVALID, "max_mismatches %d outside 0..2", max_mismatches);
    *shortest = MIPGEN_MAX_OLIGO;
    for (int i = 0; i < n; i++) {
        const mipgen_probe& q = probes[i];
        if (!q.ext_seq || !q.lig_seq) return fail(MIPGEN_E_INVALID, "probe %d: %s sequence is NULL", i, !q.ext_seq ? "extension arm" : "ligation arm");
        const size_t e = strlen(q.ext_seq), l = strlen(q.lig_seq);
        if (e < MIPGEN_MIN_OLIGO || l < MIPGEN_MIN_OLIGO) return fail(MIPGEN_E_INVALID, "probe %d: empty %s arm", i, e < MIPGEN_MIN_OLIGO ? "extension" : "ligation");
        if (e > MIPGEN_MAX_OLIGO || l > MIPGEN_MAX_OLIGO) return fail(MIPGEN_E_INVALID, "probe %d: arm of %zu bases (at most %d)", i, std::max(e, l), MIPGEN_MAX_OLIGO);
        *shortest = std::min(*shortest, std::min(e, l));
    }
    if (*shortest < 12) return fail(MIPGEN_E_INVALID, "the shortest arm of the table has %zu bases: a seed of fewer than 12 bases is refused", *shortest);
    // the barcodes, and the cells they make with the probes
    const uint64_t cells = (uint64_t)(barcodes ? (int64_t)n_samples + 1 : 1) * (uint64_t)n;
    if (barcodes) {
        if (barcode_mismatches < 0 || barcode_mismatches > 1) return fail(MIPGEN_E_INVALID, "barcode_mismatches %d outside 0..1", barcode_mismatches);
        for (int s = 0; s < n_samples; s++) {
            if (!barcodes[s]) return fail(MIPGEN_E_INVALID, "barcode %d is NULL", s);
            const size_t len = strlen(barcodes[s]);
            if (s == 0) {
                if (len < 1 || len > SAMPLES_MAX_BARCODE) return fail(MIPGEN_E_INVALID, "barcode 0 has %zu bases (1 to %d)", len, SAMPLES_MAX_BARCODE);
                *J = (int)len;
            } else if ((int)len != *J) return fail(MIPGEN_E_INVALID, "barcode %d has %zu bases, barcode 0 has %d: barcodes of unequal length", s, len, *J);
            for (int j = 0; j < *J; j++)
                if (reads_base_code((uint8_t)barcodes[s][j]) > 3u) return fail(MIPGEN_E_INVALID, "barcode %d: byte %d is not one of upper-case A C G T", s, j);
        }
        std::vector<std::string> seen(barcodes, barcodes + n_samples);
        std::sort(seen.begin(), seen.end());
        for (size_t s = 1; s < seen.size(); s++)
            if (seen[s] == seen[s - 1]) return fail(MIPGEN_E_INVALID, "barcode %s is there twice", seen[s].c_str());
        if (cells > ((uint64_t)1 << 32)) return fail(MIPGEN_E_INVALID, "%d samples + undetermined x %d probes: more than 2^32 cells", n_samples, n);
    }
    // (the sentinel key of a pair in no group is the key bit above the cell index: DESIGN 4.11)
    if (consensus && cells > ((uint64_t)1 << 31)) return fail(MIPGEN_E_INVALID, "%lld rows x %d probes: more than 2^31 cells in a consensus session", (long long)(cells / (uint64_t)n), n);
    if (h->reads) return fail(MIPGEN_E_STATE, "a read-counting session is open: mipgen_accel_reads_finish closes it");
    return MIPGEN_OK;
}

struct HostTables { std::vector<ReadProbe> packed; HostSeedTable ext, lig; std::vector<SampleSlot> sample_slots; };      // (no slots without barcodes)

static void build_host_tables(const mipgen_probe* probes, int32_t n, uint64_t seed_mask, const char* const* barcodes, int32_t n_samples, int J, int32_t barcode_mismatches, HostTables& T)
{
    T.packed.resize((size_t)n);
    std::vector<std::pair<uint64_t, int32_t>> ekp, lkp;
    for (int i = 0; i < n; i++) {
        ReadProbe& r = T.packed[(size_t)i];
        memset(&r, 0, sizeof r);
        r.e_len = (int32_t)strlen(probes[i].ext_seq); r.l_len = (int32_t)strlen(probes[i].lig_seq);
        pack_arm(probes[i].ext_seq, r.e_len, false, &r.e0, &r.e1, &r.ebad);
        pack_arm(probes[i].lig_seq, r.l_len, true, &r.l0, &r.l1, &r.lbad);
        if ((r.ebad & seed_mask) == 0) ekp.emplace_back(reads_seed_key(r.e0, r.e1, seed_mask), i);
        if ((r.lbad & seed_mask) == 0) lkp.emplace_back(reads_seed_key(r.l0, r.l1, seed_mask), i);
    }
    build_seed_table(ekp, T.ext);
    build_seed_table(lkp, T.lig);
    if (barcodes) build_sample_table(barcodes, n_samples, J, barcode_mismatches, T.sample_slots);
}

// the buffers of a new session (its flags, rows, P and key capacity are set) and the tables into them; the host tables are free when this returns
static int upload_tables(mipgen_accel* h, ReadsSession* S, const HostTables& T, int J, int32_t barcode_mismatches)
{
    const size_t n = (size_t)S->P.n_probes, cells = (size_t)S->rows * n;
    if (S->probes.reserve(n) || S->reads.reserve(cells) || S->unique.reserve(cells) || S->ctr.reserve(1)) return MIPGEN_E_NOMEM;
    if (S->keys.cap && (S->keys.keys.reserve((size_t)S->keys.cap) || S->keys.keys_alt.reserve((size_t)S->keys.cap))) return MIPGEN_E_NOMEM;
    if (S->samples && (S->smp.slots.reserve(T.sample_slots.size()) || S->smp.row_pairs.reserve((size_t)S->rows) || S->smp.ctr.reserve(1))) return MIPGEN_E_NOMEM;
    if (S->consensus && S->cons.ctr.reserve(1)) return MIPGEN_E_NOMEM;
    IdleOnExit idle{h->stream};
    if (int rc = upload_seed_table(h, T.ext, S->ext_seeds)) return rc;
    if (int rc = upload_seed_table(h, T.lig, S->lig_seeds)) return rc;
    HIP_TRY(hipMemcpyAsync(S->probes.p, T.packed.data(), n * sizeof(ReadProbe), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemsetAsync(S->reads.p, 0, cells * sizeof(unsigned long long), h->stream));
    HIP_TRY(hipMemsetAsync(S->unique.p, 0, cells * sizeof(unsigned long long), h->stream));
    HIP_TRY(hipMemsetAsync(S->ctr.p, 0, sizeof(ReadsCounters), h->stream));
    if (S->consensus) HIP_TRY(hipMemsetAsync(S->cons.ctr.p, 0, sizeof(ConsensusCounters), h->stream));
    if (S->samples) {
        HIP_TRY(hipMemcpyAsync(S->smp.slots.p, T.sample_slots.data(), T.sample_slots.size() * sizeof(SampleSlot), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(hipMemsetAsync(S->smp.row_pairs.p, 0, (size_t)S->rows * sizeof(unsigned long long), h->stream));
        HIP_TRY(hipMemsetAsync(S->smp.ctr.p, 0, sizeof(SampleCounters), h->stream));
        S->smp.table = {S->smp.slots.p, (uint32_t)(T.sample_slots.size() - 1), J, barcode_mismatches, (int32_t)(S->rows - 1)};
    }
    HIP_TRY(idle.wait());
    return MIPGEN_OK;
}

// a session, or the consensus reads a finished one left: the stream is idle before its buffers go
template <typename T> static void release_owned(mipgen_accel* h, T*& owned)
{
    if (!owned) return;
    (void)hipStreamSynchronize(h->stream);
    owned->release(); delete owned; owned = nullptr;
}

extern "C" {

void mipgen_reads_release(mipgen_accel* h) { release_owned(h, h->reads); }
void mipgen_consensus_release(mipgen_accel* h) { release_owned(h, h->consensus); }

int mipgen_accel_reads_set_key_buffer(mipgen_accel* h, int64_t n_keys)
{
    if (!h || n_keys < 0 || n_keys > READS_KEY_CAP_MAX) return fail(MIPGEN_E_INVALID, "bad arguments");
    h->reads_key_cap = n_keys;
    return MIPGEN_OK;
}

// barcodes == nullptr: a session without samples; consensus: the reads stay resident within arena_bytes (0: the default)
static int open_impl(mipgen_accel* h, const mipgen_probe* probes, int32_t n, int32_t ext_tag, int32_t lig_tag, int32_t max_mismatches, const char* const* barcodes,
                     int32_t n_samples, int32_t barcode_mismatches, bool consensus = false, int64_t arena_bytes = 0)
{
    size_t shortest = 0; int J = 0;
    if (int rc = check_open(h, probes, n, ext_tag, lig_tag, max_mismatches, barcodes, n_samples, barcode_mismatches, consensus, arena_bytes, &shortest, &J)) return rc;
    const int64_t rows = barcodes ? (int64_t)n_samples + 1 : 1;
    // the tables, on the host
    const int seed = (int)std::min<size_t>(shortest, READS_MAX_SEED);
    const uint64_t seed_mask = reads_len_mask(seed);
    HostTables T;
    build_host_tables(probes, n, seed_mask, barcodes, n_samples, J, barcode_mismatches, T);
    const size_t cells = (size_t)rows * (size_t)n;
    // the budget: tables + counters + two key buffers, against free device memory
    HIP_TRY(hipSetDevice(h->device));
    size_t free_b = 0;
    if (int rc = free_device_bytes(&free_b)) return rc;
    const bool tags = ext_tag + lig_tag > 0;
    // (a consensus session keeps no key list across feed calls: its groups come from the sort of finish)
    int64_t key_cap = !tags || consensus ? 0 : h->reads_key_cap > 0 ? h->reads_key_cap : READS_KEY_CAP_DEFAULT;
    const size_t fixed = (size_t)n * (sizeof(ReadProbe) + 2 * 4) + cells * 16 + T.sample_slots.size() * sizeof(SampleSlot) + (size_t)rows * 8 + (T.ext.slots.size() + T.lig.slots.size()) * 4 + (T.ext.keys.size() + T.lig.keys.size()) * 12 + ((size_t)64 << 20);
    if (tags && !consensus && h->reads_key_cap <= 0)
        while (key_cap > 1024 && fixed + (size_t)key_cap * 16 > free_b / 2) key_cap /= 2;      // the default gives way to what is free; half is left for the reads
    if (fixed + (size_t)key_cap * 16 > free_b)
        return fail(MIPGEN_E_NOMEM, "read counter: tables of %d probes x %lld rows and %lld keys need %zu MiB of device memory, %zu MiB are free", n, (long long)rows,
                    (long long)key_cap, (fixed + (size_t)key_cap * 16) >> 20, free_b >> 20);
    // the session: from here on it is certain to be attempted, and the consensus reads of an earlier session end here
    mipgen_consensus_release(h);
    ReadsSession* S = new ReadsSession;
    h->reads = S;
    S->P = {ext_tag, lig_tag, max_mismatches, seed, seed_mask, n, 0};
    S->samples = barcodes != nullptr; S->consensus = consensus; S->rows = rows;
    // the arena's default: half of what is free beside the tables; the other half is left to finish (56 bytes per pair of sort buffers and records, and the
    // consensus reads, which are no longer than the reads retained)
    if (consensus) S->cons.arena_cap = arena_bytes > 0 ? (size_t)arena_bytes : (free_b - fixed) / 2;
    S->keys.cap = key_cap;
    int probe_bits = 1;                                                    // (of the cell index rows * n - 1 at most: 32 bits when there are 2^32 cells)
    while (probe_bits < 32 && ((int64_t)1 << probe_bits) < (int64_t)cells) probe_bits++;
    S->keys.end_bit = 32 + probe_bits;
    if (int rc = upload_tables(h, S, T, J, barcode_mismatches)) { mipgen_reads_release(h); return rc; }
    h->reads_assign_ms = 0.0;
    h->sample_assign_ms = barcodes ? 0.0 : -1.0;
    return MIPGEN_OK;
}

// One feed call (kind: of the entry point; a consensus call carries the qualities, and the index reads if its session has samples).  A session that keeps its reads puts the
// chunk's bases and qualities straight into a block of its own (ChunkLayout), where the kernels read them and where they stay.  Everything that can refuse such a chunk - the
// arena's budget, free device memory, every allocation - comes before the first copy or launch: a refused chunk leaves the session as it was.
static int feed_impl(mipgen_accel* h, int kind, int64_t n_pairs, const char* ext_bytes, const char* ext_qual, const int64_t* ext_offsets, const char* lig_bytes,
                     const char* lig_qual, const int64_t* lig_offsets, const char* index_bytes, const int64_t* index_offsets)
{
    // 1. arguments and state
    if (!h || n_pairs < 0 || (n_pairs > 0 && (!ext_bytes || !ext_offsets || !lig_bytes || !lig_offsets || (kind == KIND_SAMPLES && (!index_bytes || !index_offsets)))))
        return fail(MIPGEN_E_INVALID, "bad arguments");
    if (kind == KIND_CONSENSUS && n_pairs > 0 && (!ext_qual || !lig_qual)) return fail(MIPGEN_E_INVALID, "bad arguments: no qualities");
    ReadsSession* S = nullptr;
    if (int rc = session_for(h, kind, true, &S)) return rc;
    const bool with_index = S->samples, keep = S->consensus;
    if (keep && with_index && n_pairs > 0 && (!index_bytes || !index_offsets)) return fail(MIPGEN_E_INVALID, "bad arguments: the session has samples and the call no index reads");
    if (n_pairs > 0x7fffffff) return fail(MIPGEN_E_INVALID, "%lld pairs in one call (at most 2^31 - 1)", (long long)n_pairs);
    if (keep && S->cons.total_pairs + n_pairs > 0x7fffffff)
        return fail(MIPGEN_E_INVALID, "%lld + %lld pairs: a consensus session holds at most 2^31 - 1 (pair ids are 32-bit)", (long long)S->cons.total_pairs, (long long)n_pairs);
    if (!keep || n_pairs == 0) S->last_pairs = 0;                           // (a refused chunk leaves a consensus session as it was, its last assignment included)
    if (n_pairs == 0) return MIPGEN_OK;

    // 2. the kernels trust the offsets: they are checked here
    for (int f = 0; f < (with_index ? 3 : 2); f++) {
        const int64_t* off = f == 2 ? index_offsets : f ? lig_offsets : ext_offsets;
        const char* what = f == 2 ? "index" : f ? "ligation" : "extension";
        if (off[0] < 0) return fail(MIPGEN_E_INVALID, "%s offsets: negative", what);
        for (int64_t i = 0; i < n_pairs; i++)
            if (off[i + 1] < off[i]) return fail(MIPGEN_E_INVALID, "%s offsets: entry %lld below entry %lld", what, (long long)(i + 1), (long long)i);
    }
    const size_t eb = (size_t)(ext_offsets[n_pairs] - ext_offsets[0]), lb = (size_t)(lig_offsets[n_pairs] - lig_offsets[0]);
    const size_t ib = with_index ? (size_t)(index_offsets[n_pairs] - index_offsets[0]) : 0;
    const size_t np = (size_t)n_pairs;
    HIP_TRY(hipSetDevice(h->device));

    // 3. the budget: the arena's, then what the call allocates against free device memory (`have`: what its buffers hold already); a kept chunk has 8 bytes per pair of scratch keys
    const ChunkLayout L(n_pairs, eb, lb);
    const size_t block_bytes = keep ? L.total : 0;
    if (keep && L.total > S->cons.arena_cap - S->cons.arena_used)
        return fail(MIPGEN_E_NOMEM, "consensus reads: a chunk of %lld pairs needs %zu bytes of the arena, %zu of %zu are left (open the session with a larger arena_bytes)",
                    (long long)n_pairs, L.total, S->cons.arena_cap - S->cons.arena_used, S->cons.arena_cap);
    size_t free_b = 0;
    if (int rc = free_device_bytes(&free_b)) return rc;
    const size_t have = (keep ? S->keys.keys.cap * 8 : S->ext_bytes.cap + S->lig_bytes.cap) + (S->ext_off.cap + S->lig_off.cap) * 8 + S->assign.cap * 4 + S->smp.idx_bytes.cap +
                        S->smp.idx_off.cap * 8 + (S->smp.row.cap + S->smp.sample_index.cap) * 4;
    const size_t need = (keep ? np * 8 : eb + lb) + 2 * (np + 1) * 8 + np * 4 + (with_index ? ib + (np + 1) * 8 + np * 8 : 0);
    if (block_bytes + need + need / 8 + ((size_t)64 << 20) > free_b + have)
        return fail(MIPGEN_E_NOMEM, "%s: a chunk of %lld pairs needs %zu MiB of device memory, %zu MiB are free%s", keep ? "consensus reads" : "read counter", (long long)n_pairs,
                    (block_bytes + need) >> 20, (free_b + have) >> 20, keep ? "" : " (feed fewer pairs per call)");

    // 4. reservations (+ 8: k_read_assign fetches the bases as aligned 32-bit words, up to 5 bytes beyond the last read; ChunkLayout has the same tail), and the chunk's block
    if (!keep && (S->ext_bytes.reserve(eb + 8) || S->lig_bytes.reserve(lb + 8))) return MIPGEN_E_NOMEM;
    if (S->ext_off.reserve(np + 1) || S->lig_off.reserve(np + 1) || S->assign.reserve(np)) return MIPGEN_E_NOMEM;
    // (keys of a kept chunk: k_read_assign's, written and never read - a consensus session counts its unique tags from its groups)
    if (keep && S->keys.keys.reserve(np)) return MIPGEN_E_NOMEM;
    if (with_index && (S->smp.idx_bytes.reserve(ib + 8) || S->smp.idx_off.reserve(np + 1) || S->smp.row.reserve(np) || S->smp.sample_index.reserve(np))) return MIPGEN_E_NOMEM;
    uint8_t* block = nullptr;
    if (keep && hipMalloc((void**)&block, L.total) != hipSuccess) { (void)hipGetLastError(); return fail(MIPGEN_E_NOMEM, "consensus reads: hipMalloc of a chunk of %zu bytes failed", L.total); }
    FreeOnExit free_block{block};                                           // (until the chunk is the session's: stage 11)
    hipStream_t st = h->stream;
    SpanTimer sample_time{h->timing, st}, assign_time{h->timing, st};
    IdleOnExit idle{st};                                                    // (ends before free_block and the timers do: events go once the stream is idle)

    // 5. uploads
    uint8_t *ext_dev = keep ? block + L.ext : S->ext_bytes.p, *lig_dev = keep ? block + L.lig : S->lig_bytes.p;
    if (eb) HIP_TRY(hipMemcpyAsync(ext_dev, ext_bytes, eb, hipMemcpyHostToDevice, st));
    if (eb && keep) HIP_TRY(hipMemcpyAsync(block + L.ext_qual, ext_qual, eb, hipMemcpyHostToDevice, st));
    if (lb) HIP_TRY(hipMemcpyAsync(lig_dev, lig_bytes, lb, hipMemcpyHostToDevice, st));
    if (lb && keep) HIP_TRY(hipMemcpyAsync(block + L.lig_qual, lig_qual, lb, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(S->ext_off.p, ext_offsets, (np + 1) * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(S->lig_off.p, lig_offsets, (np + 1) * 8, hipMemcpyHostToDevice, st));
    if (keep) HIP_TRY(hipMemsetAsync(&S->ctr.p->n_keys, 0, sizeof(unsigned long long), st));

    // 6. the sample row of every pair of the chunk, before the launches that count into its cells
    if (with_index) {
        if (ib) HIP_TRY(hipMemcpyAsync(S->smp.idx_bytes.p, index_bytes, ib, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(S->smp.idx_off.p, index_offsets, (np + 1) * 8, hipMemcpyHostToDevice, st));
        sample_time.mark();
        HIP_TRY(mipgen_launch_sample_assign(st, &S->smp.table, n_pairs, S->smp.idx_bytes.p, S->smp.idx_off.p, index_offsets[0], S->smp.row.p, S->smp.sample_index.p,
                                            S->smp.row_pairs.p, S->smp.ctr.p));
        sample_time.mark();
    }
    const int32_t* row = with_index ? S->smp.row.p : nullptr;

    // 7. k_read_assign: a key list takes as many pairs per launch as it has room for; a kept chunk goes in one launch, its keys into the scratch list
    const bool listed = !keep && S->P.te + S->P.tl > 0;
    for (int64_t p0 = 0; p0 < n_pairs;) {
        int64_t c = n_pairs - p0;
        if (listed) {
            if (int rc = S->keys.make_room(h, &S->ctr.p->n_keys, c, &c)) return rc;
            c = std::min(c, n_pairs - p0);
        }
        assign_time.mark();
        HIP_TRY(mipgen_launch_read_assign(st, &S->P, S->probes.p, &S->ext_seeds.view, &S->lig_seeds.view, p0, c, ext_dev, S->ext_off.p, ext_offsets[0], lig_dev, S->lig_off.p,
                                          lig_offsets[0], S->assign.p, S->reads.p, S->keys.keys.p, keep ? (int64_t)S->keys.keys.cap : S->keys.cap, S->ctr.p, row));
        assign_time.mark();
        if (listed) S->keys.ub += c;
        p0 += c;
    }

    // 8. the (key, pair id) and record of every pair of a kept chunk
    if (keep)
        HIP_TRY(mipgen_launch_member_keys(st, &S->P, n_pairs, (uint32_t)S->cons.total_pairs, S->assign.p, row, ext_dev, S->ext_off.p, ext_offsets[0], lig_dev, S->lig_off.p,
                                          lig_offsets[0], L.qdelta, 1ull << S->keys.end_bit, reinterpret_cast<uint64_t*>(block + L.keys), reinterpret_cast<uint32_t*>(block + L.ids),
                                          reinterpret_cast<ConsensusPair*>(block + L.recs), S->cons.ctr.p));

    // 9. - 11. synchronise, book the times, commit
    HIP_TRY(idle.wait());
    sample_time.add_to(&h->sample_assign_ms); assign_time.add_to(&h->reads_assign_ms);
    if (keep) {
        S->cons.chunks.push_back({block, L.total, S->cons.total_pairs, n_pairs});
        free_block.p = nullptr;
        S->cons.total_pairs += n_pairs;
        S->cons.arena_used += L.total;
    }
    S->last_pairs = n_pairs;
    return MIPGEN_OK;
}

// the sample index (sample: true) or the probe index of every pair of the last feed call
static int download_last(mipgen_accel* h, bool sample, int32_t* out, int64_t capacity)
{
    if (!h || !out) return fail(MIPGEN_E_INVALID, "bad arguments");
    const ReadsSession* S = h->reads;
    if (!S) return fail(MIPGEN_E_STATE, "no read-counting session is open");
    if (sample && !S->samples) return fail(MIPGEN_E_STATE, "the open session has no samples");
    if (capacity < S->last_pairs) return fail(MIPGEN_E_INVALID, "capacity %lld < %lld pairs", (long long)capacity, (long long)S->last_pairs);
    HIP_TRY(hipSetDevice(h->device));
    if (S->last_pairs) HIP_TRY(hipMemcpyAsync(out, sample ? S->smp.sample_index.p : S->assign.p, (size_t)S->last_pairs * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return MIPGEN_OK;
}

// The tag merge of a session with tag mismatches 1, between the runs of the sorted member keys and the partition.  On entry the *G raw groups lie in
// Q.keys / Q.ids (group key, family); they are copied to R, every raw group gets its parent and its root, and - when a group was absorbed at all - every member key is
// rewritten to its root's key, back into the unsorted arrays, which are sorted and run-length encoded once more: Q.keys / Q.ids then hold the *G corrected groups.
// The G-sized arrays are checked against free device memory before the first launch.
static int merge_tags(mipgen_accel* h, ReadsSession* S, ConsensusResult* R, int64_t N, int64_t M, int sort_bits, int64_t* G, SpanTimer& sort_time, SpanTimer& merge_time)
{
    hipStream_t st = h->stream;
    ConsensusPart& C = S->cons;
    SortedPairs& Q = C.pairs;
    const int64_t G0 = *G;
    size_t free_b = 0;
    if (int rc = free_device_bytes(&free_b)) return rc;
    const size_t need = padded((size_t)G0, 8) + 3 * padded((size_t)G0, 4) + padded(1, sizeof(TagMergeCounters));      // raw keys; raw families, roots, parents
    if (need + ((size_t)64 << 20) > free_b)
        return fail(MIPGEN_E_NOMEM, "tag merge: the parent, root and raw copy of %lld groups need %zu MiB of device memory, %zu MiB are free", (long long)G0, need >> 20, free_b >> 20);
    if (R->raw_keys.reserve((size_t)G0) || R->raw_family.reserve((size_t)G0) || R->raw_root.reserve((size_t)G0) || C.t_parent.reserve((size_t)G0) || C.t_ctr.reserve(1))
        return MIPGEN_E_NOMEM;
    HIP_TRY(hipMemcpyAsync(R->raw_keys.p, Q.keys.p, (size_t)G0 * 8, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(R->raw_family.p, Q.ids.p, (size_t)G0 * 4, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemsetAsync(C.t_ctr.p, 0, sizeof(TagMergeCounters), st));
    merge_time.mark();
    HIP_TRY(mipgen_launch_tag_parent(st, R->raw_keys.p, R->raw_family.p, G0, S->P.te + S->P.tl, C.t_parent.p));
    HIP_TRY(mipgen_launch_tag_root(st, C.t_parent.p, R->raw_family.p, G0, R->raw_root.p, C.t_ctr.p));
    merge_time.mark();
    TagMergeCounters tc;
    HIP_TRY(hipMemcpyAsync(&tc, C.t_ctr.p, sizeof tc, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (tc.unended) return fail(MIPGEN_E_STATE, "tag merge: the parent walk of %llu groups did not end within %d links", tc.unended, TAG_MERGE_MAX_LINKS);
    if ((int64_t)tc.absorbed >= G0 || (int64_t)tc.moved_pairs >= M)
        return fail(MIPGEN_E_STATE, "tag merge: %llu groups of %lld absorbed, %llu pairs of %lld moved", tc.absorbed, (long long)G0, tc.moved_pairs, (long long)M);
    R->merged = true;
    if (tc.absorbed) {                                                       // (nothing absorbed: the raw groups are the corrected ones, and the second sort is skipped)
        merge_time.mark();
        HIP_TRY(mipgen_launch_tag_rewrite(st, Q.keys_sorted.p, Q.ids_sorted.p, N, M, R->raw_keys.p, G0, R->raw_root.p, Q.keys.p, Q.ids.p));
        merge_time.mark();
        sort_time.mark();
        HIP_TRY(Q.sort(st, N, sort_bits));
        HIP_TRY(Q.runs(st, M, Q.keys.p, reinterpret_cast<int32_t*>(Q.ids.p), &C.ctr.p->groups));
        sort_time.mark();
        ConsensusCounters cc;
        HIP_TRY(hipMemcpyAsync(&cc, C.ctr.p, sizeof cc, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if ((int64_t)cc.groups != G0 - (int64_t)tc.absorbed)
            return fail(MIPGEN_E_STATE, "tag merge: %llu groups after %llu of %lld were absorbed", cc.groups, tc.absorbed, (long long)G0);
        *G = (int64_t)cc.groups;
    }
    R->tag_totals = {G0, *G, (int64_t)tc.absorbed, (int64_t)tc.moved_pairs, (int64_t)tc.max_depth};
    return MIPGEN_OK;
}

// The groups of a consensus session and their consensus reads into R; unique tags per cell - the groups of the cell - into S->unique.
static int consensus_finish(mipgen_accel* h, ReadsSession* S, ConsensusResult* R)
{
    hipStream_t st = h->stream;
    ConsensusPart& C = S->cons;
    SortedPairs& Q = C.pairs;
    const int64_t N = C.total_pairs;
    h->consensus_vote_ms = h->consensus_sort_ms = h->tag_merge_ms = -1.0;
    ConsensusCounters cc;
    HIP_TRY(hipMemcpyAsync(&cc, C.ctr.p, sizeof cc, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const int64_t M = (int64_t)cc.members;                                   // pairs in a group: the keys below the sentinel
    if (M == 0) return MIPGEN_OK;
    // one scratch buffer for the sort, the run boundaries and the three scans (sized for the most entries any of them sees)
    size_t scratch = 0, t_i64 = 0;
    const int sort_bits = S->keys.end_bit + 1;                               // the cell and tag bits that can be set, and the sentinel's
    HIP_TRY(SortedPairs::scratch_bytes(st, N, sort_bits, M, M + 1, &scratch));
    HIP_TRY(mipgen_consensus_scan_i64(st, nullptr, &t_i64, nullptr, nullptr, M + 1));
    // every pair's (key, id) and record, chunk after chunk, in feed order
    if (Q.reserve((size_t)N, std::max(scratch, t_i64) + 16) || C.c_recs.reserve((size_t)N)) return MIPGEN_E_NOMEM;
    for (const ArenaChunk& c : C.chunks) {
        const ChunkLayout L(c.n, 0, 0);                                      // (the per-pair parts lie in front of the bytes)
        HIP_TRY(hipMemcpyAsync(C.c_recs.p + c.pair0, c.block + L.recs, (size_t)c.n * sizeof(ConsensusPair), hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipMemcpyAsync(Q.keys.p + c.pair0, c.block + L.keys, (size_t)c.n * 8, hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipMemcpyAsync(Q.ids.p + c.pair0, c.block + L.ids, (size_t)c.n * 4, hipMemcpyDeviceToDevice, st));
    }
    SpanTimer sort_time{h->timing, st}, vote_time{h->timing, st}, merge_time{h->timing, st};
    // sort; the runs of the member keys: group key and family size (the fed arrays are free once sorted, and take them)
    sort_time.mark();
    HIP_TRY(Q.sort(st, N, sort_bits));
    uint64_t* group_keys = Q.keys.p;
    int32_t* family = reinterpret_cast<int32_t*>(Q.ids.p);
    HIP_TRY(Q.runs(st, M, group_keys, family, &C.ctr.p->groups));
    sort_time.mark();
    HIP_TRY(hipMemcpyAsync(&cc, C.ctr.p, sizeof cc, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    int64_t G = (int64_t)cc.groups;
    if (G < 1 || G > M) return fail(MIPGEN_E_STATE, "consensus reads: %lld groups of %lld members", (long long)G, (long long)M);
    R->tag_totals = {G, G, 0, 0, 0};
    if (C.tag_mismatches)                                                    // (group_keys and family then hold the corrected groups)
        if (int rc = merge_tags(h, S, R, N, M, sort_bits, &G, sort_time, merge_time)) return rc;
    if (R->keys.reserve((size_t)G) || R->family.reserve((size_t)G) || R->ext_off.reserve((size_t)G + 1) || R->lig_off.reserve((size_t)G + 1) || C.c_start.reserve((size_t)G) ||
        C.c_order.reserve((size_t)G) || C.c_ext_len.reserve((size_t)G + 1) || C.c_lig_len.reserve((size_t)G + 1))
        return MIPGEN_E_NOMEM;
    HIP_TRY(hipMemcpyAsync(R->keys.p, group_keys, (size_t)G * 8, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(R->family.p, family, (size_t)G * 4, hipMemcpyDeviceToDevice, st));
    HIP_TRY(Q.scan_u32(st, R->family.p, C.c_start.p, G));
    HIP_TRY(mipgen_launch_consensus_partition(st, R->family.p, G, C.c_order.p, C.ctr.p));
    HIP_TRY(hipMemcpyAsync(&cc, C.ctr.p, sizeof cc, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const int64_t n_small = (int64_t)cc.n_small, n_big = (int64_t)cc.n_big;
    if (n_small + n_big != G) return fail(MIPGEN_E_STATE, "consensus reads: %lld + %lld groups listed of %lld", (long long)n_small, (long long)n_big, (long long)G);
    // the length of every group's two consensus reads (entry G stays 0), and from their exclusive sums where each is written
    HIP_TRY(hipMemsetAsync(C.c_ext_len.p, 0, (size_t)(G + 1) * 8, st));
    HIP_TRY(hipMemsetAsync(C.c_lig_len.p, 0, (size_t)(G + 1) * 8, st));
    HIP_TRY(mipgen_launch_consensus_len(st, S->P.te, S->P.tl, G, C.c_order.p, n_big, C.c_start.p, R->family.p, Q.ids_sorted.p, C.c_recs.p, C.c_ext_len.p, C.c_lig_len.p));
    HIP_TRY(Q.scan_i64(st, C.c_ext_len.p, R->ext_off.p, G + 1));
    HIP_TRY(Q.scan_i64(st, C.c_lig_len.p, R->lig_off.p, G + 1));
    int64_t totals[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(&totals[0], R->ext_off.p + G, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&totals[1], R->lig_off.p + G, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (R->ext_seq.reserve((size_t)totals[0] + 1) || R->ext_qual.reserve((size_t)totals[0] + 1) || R->lig_seq.reserve((size_t)totals[1] + 1) ||
        R->lig_qual.reserve((size_t)totals[1] + 1))
        return MIPGEN_E_NOMEM;
    vote_time.mark();
    HIP_TRY(mipgen_launch_consensus_vote(st, S->P.te, S->P.tl, G, C.c_order.p, n_small, n_big, C.c_start.p, R->family.p, Q.ids_sorted.p, C.c_recs.p, R->ext_off.p,
                                         R->lig_off.p, R->ext_seq.p, R->ext_qual.p, R->lig_seq.p, R->lig_qual.p));
    vote_time.mark();
    // unique tags of a cell = its groups: the group keys ARE the sorted, duplicate-free key list of a plain session
    HIP_TRY(mipgen_launch_reads_histogram(st, R->keys.p, G, S->unique.p));
    HIP_TRY(hipStreamSynchronize(st));
    double sort_ms = 0.0, vote_ms = 0.0, merge_ms = 0.0;
    if (merge_time.add_to(&merge_ms)) h->tag_merge_ms = merge_ms;
    if (sort_time.add_to(&sort_ms)) h->consensus_sort_ms = sort_ms;
    if (vote_time.add_to(&vote_ms)) h->consensus_vote_ms = vote_ms;
    R->n_groups = G; R->ext_bytes = totals[0]; R->lig_bytes = totals[1];
    return MIPGEN_OK;
}

static int finish_impl(mipgen_accel* h, ReadsSession* S, int64_t* reads, int64_t* unique_tags, mipgen_read_totals* totals, mipgen_sample_totals* sample_totals,
                       int64_t* row_pairs)
{
    HIP_TRY(hipSetDevice(h->device));
    const size_t n = (size_t)S->P.n_probes * (size_t)S->rows;                // cells
    const bool tags = S->P.te + S->P.tl > 0;
    if (tags && !S->consensus) {                                             // (a consensus session: consensus_finish counted its groups into `unique`)
        if (int rc = S->keys.sort_unique(h, &S->ctr.p->n_keys)) return rc;
        HIP_TRY(mipgen_launch_reads_histogram(h->stream, S->keys.keys.p, S->keys.ub, S->unique.p));
    }
    ReadsCounters c;
    HIP_TRY(hipMemcpyAsync(&c, S->ctr.p, sizeof c, hipMemcpyDeviceToHost, h->stream));
    static_assert(sizeof(unsigned long long) == sizeof(int64_t), "counts are downloaded in place");
    if (reads) HIP_TRY(hipMemcpyAsync(reads, S->reads.p, n * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
    if (unique_tags) HIP_TRY(hipMemcpyAsync(unique_tags, tags ? S->unique.p : S->reads.p, n * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
    SampleCounters sc{0, 0};
    if (S->samples) {
        HIP_TRY(hipMemcpyAsync(&sc, S->smp.ctr.p, sizeof sc, hipMemcpyDeviceToHost, h->stream));
        if (row_pairs) HIP_TRY(hipMemcpyAsync(row_pairs, S->smp.row_pairs.p, (size_t)S->rows * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
    }
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (c.keys_lost) return fail(MIPGEN_E_STATE, "read counter: %llu keys did not fit the key buffer", c.keys_lost);
    if (sample_totals) *sample_totals = {(int64_t)sc.none, (int64_t)sc.ambiguous};
    if (totals) *totals = {(int64_t)c.pairs, (int64_t)c.assigned, (int64_t)c.ambiguous, (int64_t)c.unassigned, (int64_t)c.tag_n, (int64_t)c.overflow};
    return MIPGEN_OK;
}

// A finish call of any kind: the session is released whatever comes of it; the consensus reads of a session that kept its reads stay on the handle.
static int finish_session(mipgen_accel* h, int kind, int64_t* reads, int64_t* unique_tags, mipgen_read_totals* totals, mipgen_sample_totals* sample_totals, int64_t* row_pairs,
                          mipgen_consensus_sizes* sizes)
{
    if (!h) return fail(MIPGEN_E_INVALID, "null handle");
    ReadsSession* S = nullptr;
    if (int rc = session_for(h, kind, false, &S)) return rc;
    ConsensusResult* R = nullptr;
    int rc = MIPGEN_OK;
    if (S->consensus) {
        HIP_TRY(hipSetDevice(h->device));
        R = new ConsensusResult;
        R->n = S->P.n_probes; R->rows = S->rows;
        rc = consensus_finish(h, S, R);
    }
    if (rc == MIPGEN_OK) rc = finish_impl(h, S, reads, unique_tags, totals, sample_totals, row_pairs);
    mipgen_reads_release(h);
    if (R && rc != MIPGEN_OK) { R->release(); delete R; }
    if (R && rc == MIPGEN_OK) {
        h->consensus = R;
        if (sizes) *sizes = {R->n_groups, R->ext_bytes, R->lig_bytes};
    }
    return rc;
}

int mipgen_accel_reads_open(mipgen_accel* h, const mipgen_probe* probes, int32_t n, int32_t ext_tag, int32_t lig_tag, int32_t max_mismatches)
{
    return open_impl(h, probes, n, ext_tag, lig_tag, max_mismatches, nullptr, 0, 0);
}

int mipgen_accel_reads_open_samples(mipgen_accel* h, const mipgen_probe* probes, int32_t n, int32_t ext_tag, int32_t lig_tag, int32_t max_mismatches,
                                    const char* const* barcodes, int32_t n_samples, int32_t barcode_mismatches)
{
    if (!barcodes || n_samples < 1) return fail(MIPGEN_E_INVALID, "bad arguments: no barcodes");
    return open_impl(h, probes, n, ext_tag, lig_tag, max_mismatches, barcodes, n_samples, barcode_mismatches);
}

int mipgen_accel_reads_open_consensus(mipgen_accel* h, const mipgen_probe* probes, int32_t n, int32_t ext_tag, int32_t lig_tag, int32_t max_mismatches,
                                      const char* const* barcodes, int32_t n_samples, int32_t barcode_mismatches, int64_t arena_bytes)
{
    if ((barcodes == nullptr) != (n_samples == 0) || n_samples < 0) return fail(MIPGEN_E_INVALID, "bad arguments: barcodes and n_samples disagree");
    return open_impl(h, probes, n, ext_tag, lig_tag, max_mismatches, barcodes, n_samples, barcode_mismatches, true, arena_bytes);
}

int mipgen_accel_reads_feed(mipgen_accel* h, int64_t n_pairs, const char* ext_bytes, const int64_t* ext_offsets, const char* lig_bytes, const int64_t* lig_offsets)
{
    return feed_impl(h, KIND_PLAIN, n_pairs, ext_bytes, nullptr, ext_offsets, lig_bytes, nullptr, lig_offsets, nullptr, nullptr);
}

int mipgen_accel_reads_feed_samples(mipgen_accel* h, int64_t n_pairs, const char* ext_bytes, const int64_t* ext_offsets, const char* lig_bytes, const int64_t* lig_offsets,
                                    const char* index_bytes, const int64_t* index_offsets)
{
    return feed_impl(h, KIND_SAMPLES, n_pairs, ext_bytes, nullptr, ext_offsets, lig_bytes, nullptr, lig_offsets, index_bytes, index_offsets);
}

int mipgen_accel_reads_feed_consensus(mipgen_accel* h, int64_t n_pairs, const char* ext_bytes, const char* ext_qual, const int64_t* ext_offsets, const char* lig_bytes,
                                      const char* lig_qual, const int64_t* lig_offsets, const char* index_bytes, const int64_t* index_offsets)
{
    return feed_impl(h, KIND_CONSENSUS, n_pairs, ext_bytes, ext_qual, ext_offsets, lig_bytes, lig_qual, lig_offsets, index_bytes, index_offsets);
}

int mipgen_accel_reads_set_tag_mismatches(mipgen_accel* h, int32_t d)
{
    if (!h) return fail(MIPGEN_E_INVALID, "null handle");
    ReadsSession* S = h->reads;
    if (!S) return fail(MIPGEN_E_STATE, "no read-counting session is open");
    if (!S->consensus) return fail(MIPGEN_E_STATE, "the open session keeps no reads: tags are merged by family size, in a session opened by mipgen_accel_reads_open_consensus");
    if (d != 0 && d != 1) return fail(MIPGEN_E_INVALID, "tag_mismatches %d outside 0..1", d);
    S->cons.tag_mismatches = d;
    return MIPGEN_OK;
}

int mipgen_accel_reads_last_tag_merge(mipgen_accel* h, mipgen_tag_merge_totals* totals)
{
    if (!h || !totals) return fail(MIPGEN_E_INVALID, "bad arguments");
    if (!h->consensus) return fail(MIPGEN_E_STATE, "the handle holds no consensus reads: mipgen_accel_reads_finish_consensus leaves them, the next mipgen_accel_reads_open* drops them");
    *totals = h->consensus->tag_totals;
    return MIPGEN_OK;
}

int mipgen_accel_reads_tag_map_fetch(mipgen_accel* h, int32_t* cell, uint32_t* raw_tag, int32_t* raw_family, uint32_t* tag)
{
    if (!h) return fail(MIPGEN_E_INVALID, "null handle");
    if (!h->consensus) return fail(MIPGEN_E_STATE, "the handle holds no consensus reads: mipgen_accel_reads_finish_consensus leaves them, the next mipgen_accel_reads_open* drops them");
    HIP_TRY(hipSetDevice(h->device));
    const ConsensusResult* R = h->consensus;
    const size_t G0 = (size_t)R->tag_totals.raw_groups;
    if (G0 == 0) return MIPGEN_OK;
    hipStream_t st = h->stream;
    std::vector<uint64_t> keys;
    std::vector<int32_t> root;
    if (cell || raw_tag || tag) {
        keys.resize(G0);
        HIP_TRY(hipMemcpyAsync(keys.data(), R->merged ? R->raw_keys.p : R->keys.p, G0 * 8, hipMemcpyDeviceToHost, st));
    }
    if (tag && R->merged) {
        root.resize(G0);
        HIP_TRY(hipMemcpyAsync(root.data(), R->raw_root.p, G0 * 4, hipMemcpyDeviceToHost, st));
    }
    if (raw_family) HIP_TRY(hipMemcpyAsync(raw_family, R->merged ? R->raw_family.p : R->family.p, G0 * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (size_t g = 0; g < keys.size(); g++) {
        if (cell) cell[g] = (int32_t)(keys[g] >> 32);
        if (raw_tag) raw_tag[g] = (uint32_t)keys[g];
        if (tag) {
            const size_t r = R->merged ? (size_t)root[g] : g;
            if (r >= G0) return fail(MIPGEN_E_STATE, "tag merge: raw group %zu has root %zu of %zu", g, r, G0);
            tag[g] = (uint32_t)keys[r];
        }
    }
    return MIPGEN_OK;
}

int mipgen_accel_reads_last_samples(mipgen_accel* h, int32_t* sample_index, int64_t capacity) { return download_last(h, true, sample_index, capacity); }
int mipgen_accel_reads_last_assignment(mipgen_accel* h, int32_t* probe_index, int64_t capacity) { return download_last(h, false, probe_index, capacity); }

int mipgen_accel_reads_finish(mipgen_accel* h, int64_t* reads, int64_t* unique_tags, mipgen_read_totals* totals)
{
    return finish_session(h, KIND_PLAIN, reads, unique_tags, totals, nullptr, nullptr, nullptr);
}

int mipgen_accel_reads_finish_samples(mipgen_accel* h, int64_t* reads, int64_t* unique_tags, mipgen_read_totals* totals, mipgen_sample_totals* sample_totals, int64_t* row_pairs)
{
    return finish_session(h, KIND_SAMPLES, reads, unique_tags, totals, sample_totals, row_pairs, nullptr);
}

int mipgen_accel_reads_finish_consensus(mipgen_accel* h, int64_t* reads, int64_t* unique_tags, mipgen_read_totals* totals, mipgen_sample_totals* sample_totals,
                                        int64_t* row_pairs, mipgen_consensus_sizes* sizes)
{
    return finish_session(h, KIND_CONSENSUS, reads, unique_tags, totals, sample_totals, row_pairs, sizes);
}

int mipgen_accel_reads_consensus_fetch(mipgen_accel* h, int32_t* cell, uint32_t* tag, int32_t* family, int64_t* ext_off, char* ext_seq, char* ext_qual, int64_t* lig_off,
                                       char* lig_seq, char* lig_qual)
{
    if (!h) return fail(MIPGEN_E_INVALID, "null handle");
    if (!h->consensus) return fail(MIPGEN_E_STATE, "the handle holds no consensus reads: mipgen_accel_reads_finish_consensus leaves them, the next mipgen_accel_reads_open* drops them");
    HIP_TRY(hipSetDevice(h->device));
    const ConsensusResult* R = h->consensus;
    const size_t G = (size_t)R->n_groups;
    if (G == 0) {
        if (ext_off) ext_off[0] = 0;
        if (lig_off) lig_off[0] = 0;
        return MIPGEN_OK;
    }
    hipStream_t st = h->stream;
    std::vector<uint64_t> keys;
    if (cell || tag) {
        keys.resize(G);
        HIP_TRY(hipMemcpyAsync(keys.data(), R->keys.p, G * 8, hipMemcpyDeviceToHost, st));
    }
    if (family) HIP_TRY(hipMemcpyAsync(family, R->family.p, G * 4, hipMemcpyDeviceToHost, st));
    if (ext_off) HIP_TRY(hipMemcpyAsync(ext_off, R->ext_off.p, (G + 1) * 8, hipMemcpyDeviceToHost, st));
    if (lig_off) HIP_TRY(hipMemcpyAsync(lig_off, R->lig_off.p, (G + 1) * 8, hipMemcpyDeviceToHost, st));
    if (ext_seq && R->ext_bytes) HIP_TRY(hipMemcpyAsync(ext_seq, R->ext_seq.p, (size_t)R->ext_bytes, hipMemcpyDeviceToHost, st));
    if (ext_qual && R->ext_bytes) HIP_TRY(hipMemcpyAsync(ext_qual, R->ext_qual.p, (size_t)R->ext_bytes, hipMemcpyDeviceToHost, st));
    if (lig_seq && R->lig_bytes) HIP_TRY(hipMemcpyAsync(lig_seq, R->lig_seq.p, (size_t)R->lig_bytes, hipMemcpyDeviceToHost, st));
    if (lig_qual && R->lig_bytes) HIP_TRY(hipMemcpyAsync(lig_qual, R->lig_qual.p, (size_t)R->lig_bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (size_t g = 0; g < keys.size(); g++) {
        if (cell) cell[g] = (int32_t)(keys[g] >> 32);
        if (tag) tag[g] = (uint32_t)keys[g];
    }
    return MIPGEN_OK;
}

}  // extern "C"
