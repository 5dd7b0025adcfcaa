// reads_common.h — what kernels_reads.hip, kernels_consensus.hip and accel_reads.hip share of the read counter: the packed probe arms,
// the seed tables, the base code, the hash of a seed key and the packing of a tag.  The host packs the arms and builds the tables with the same functions
// the kernel reads them with.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define READS_MAX_SEED 32            // bases of a seed: 2 bits each in a 64-bit key
#define READS_MAX_CAND 1024          // probes compared per pair (both seed ranges together); a pair above it is counted in `overflow`
#define READS_MAX_TAG 16             // tag bases of a pair: 2 bits each in the low word of a 64-bit key

#define READS_UNASSIGNED (-1)
#define READS_AMBIGUOUS (-2)
#define READS_OVERFLOW (-3)

// An arm of up to 64 bases as three bit planes, base i at bit i: low and high bit of its code (A 0, C 1, G 2, T 3) and "not one of upper-case A C G T".
// A mismatch count is then one popcount: ((x0 ^ a0) | (x1 ^ a1) | xbad | abad) & length mask.
struct ReadProbe {                    // 64 bytes: one cache line per probe
    uint64_t e0, e1, ebad;            // E = ext_probe_sequence
    uint64_t l0, l1, lbad;            // revcomp(L), L = lig_probe_sequence
    int32_t e_len, l_len;
    uint64_t pad;
};

// key -> range of probe indices: an open-addressing hash of the DISTINCT seed keys (slot = index of the key + 1, 0 = empty; linear probing, load <= 1/2)
// in front of the sorted keys; probes[start[k], start[k + 1]) are the probes (ascending) whose seed is keys[k]
struct SeedTable {
    const uint32_t* slots;
    const uint64_t* keys;
    const uint32_t* start;
    const int32_t* probes;
    uint32_t mask;                    // slots - 1 (a power of two)
};

struct ReadsParams {
    int32_t te, tl;                   // tag bases at the head of the extension / ligation read
    int32_t m;                        // mismatches allowed per arm
    int32_t S;                        // seed length
    uint64_t seed_mask;               // low S bits
    int32_t n_probes, pad;
};

// index key -> sample: an open-addressing hash (linear probing, load <= 1/2, reads_hash) keyed by the first J index bases packed like a seed
// key.  One 16-byte slot per entry.  At barcode_mismatches = 1 it also holds every one-substitution neighbour of every barcode.
#define SAMPLES_MAX_BARCODE 32       // bases of a barcode: 2 bits each in a 64-bit key
#define SAMPLES_LDS_ROWS 4096        // k_sample_assign counts the pairs of up to this many samples in LDS (16 KiB); beyond it by one atomic per pair, spread over that many rows
#define SAMPLE_NONE (-1)
#define SAMPLE_AMBIGUOUS (-2)
#define SAMPLE_SLOT_EMPTY 0u
#define SAMPLE_SLOT_EXACT 1u         // the key is a barcode
#define SAMPLE_SLOT_NEIGHBOUR 2u     // the key is one substitution from the barcode `sample`, or from several (sample = SAMPLE_AMBIGUOUS)

struct alignas(16) SampleSlot { uint64_t key; int32_t sample; uint32_t kind; };

struct SampleTable {
    const SampleSlot* slots;
    uint32_t mask;                    // slots - 1 (a power of two)
    int32_t J;                        // barcode length
    int32_t d;                        // barcode_mismatches
    int32_t n_samples;
};

struct SampleCounters { unsigned long long none, ambiguous; };

struct ReadsCounters { unsigned long long pairs, assigned, ambiguous, unassigned, tag_n, overflow, n_keys, keys_lost; };

__host__ __device__ static inline uint32_t reads_base_code(uint32_t c)     // 0..3, or 4 for every other byte (lower case included)
{
    return c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : 4u;
}

__host__ __device__ static inline uint64_t reads_len_mask(int n) { return n >= 64 ? ~0ull : ((1ull << n) - 1ull); }

__host__ __device__ static inline uint64_t reads_seed_key(uint64_t p0, uint64_t p1, uint64_t seed_mask) { return (p0 & seed_mask) | ((p1 & seed_mask) << 32); }

__host__ __device__ static inline uint32_t reads_hash(uint64_t k)           // splitmix64's finaliser
{
    k ^= k >> 30; k *= 0xbf58476d1ce4e5b9ull;
    k ^= k >> 27; k *= 0x94d049bb133111ebull;
    k ^= k >> 31;
    return (uint32_t)k;
}

// `n` tag bases from the head of a read into *tag (2 bits each, appended below what is there); false if one of them is not A C G T.  The one packing of a
// tag: k_read_assign's sort-unique keys and k_member_keys' group keys are built with it.
__device__ static inline bool pack_tag(const uint8_t* __restrict__ b, int64_t from, int n, uint32_t* tag)
{
    bool clean = true;
    for (int i = 0; i < n; i++) {
        const uint32_t c = reads_base_code(b[from + i]);
        clean = clean && c < 4u;
        *tag = (*tag << 2) | (c & 3u);
    }
    return clean;
}

// ---- consensus reads per tag group ----
#define CONSENSUS_WG_FAMILY 256      // a family of more members than this is voted by a whole 256-thread workgroup (its four wavefronts stride over the members); up
                                     // to it by one wavefront.  Below 64 members per wavefront the LDS combine and its two barriers per round cost more than they save.
#define CONSENSUS_MAX_Q 93           // q = clamp(byte - 33, 0, 93)

// where the two reads of a retained pair lie in the arena: the first byte of each read (tag included), its length, and the distance from a base to its quality
struct alignas(16) ConsensusPair { const uint8_t* ext; const uint8_t* lig; int64_t qdelta; int32_t ext_len, lig_len; };      // 32 bytes

struct ConsensusCounters { unsigned long long members, groups, n_small, n_big; };

// ---- allele counts per template position from the consensus reads ----
#define PILEUP_WG_CELL 256           // a (row, probe) cell of more molecules than this takes a 256-thread workgroup per round of 64 positions (its four wavefronts stride
                                     // over the molecules); up to it one wavefront.  The trade is CONSENSUS_WG_FAMILY's: two barriers and an LDS combine per round.
#define PILEUP_COLUMNS 5             // A, C, G, T, discordant

// n_small / n_big: the (cell, round) units listed for the one-wavefront / the workgroup kernel; used: the row's groups of at least min_family pairs; bases / discordant:
// the sums of columns 0..3 / of column 4
struct PileupCounters { unsigned long long n_small, n_big, used, bases, discordant; };

// ---- the pileup with indels ----
#define GAPPED_COLUMNS 8             // A, C, G, T, discordant, del, ins, ins_discordant

// n_sides / proj_bytes: the (group, side) pairs listed for k_gap_align and the bytes of their projections; gapped_sides: those whose path holds a gap step; the others:
// the sums of columns 0..3, 4, 5, 6 and 7
struct GappedCounters { unsigned long long n_sides, proj_bytes, gapped_sides, bases, discordant, deletions, insertions, ins_discordant; };
// insertion alleles: the columns of the anchor table; what InsPile sums and emits, and the runs of the sorted keys
#define INSERTION_COLUMNS 4          // span, ins, ins_discordant, ambiguous
struct InsCounters { unsigned long long span, insertions, ins_discordant, ambiguous, events, alleles; };
// deletion alleles: the columns of the sites table; what DelPile sums and emits - the events and the sum of their lengths -, and the runs of the sorted keys
#define DELETION_COLUMNS 4           // depth, starts, ragged, del
struct DelCounters { unsigned long long depth, starts, ragged, deleted, events, length_sum, alleles; };
