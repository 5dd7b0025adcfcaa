// insertion_locus_host.cpp — gap_allele_revcomp and gap_locus_allele_key of mipgen_amd/csrc/gapped_align.h as a plain C++ program, for the sanitizers:
// TEST INFRASTRUCTURE ONLY.  tests/test_insertion_locus_cpu.py builds it with -fsanitize=address,undefined and reads the one line it prints.  The reference is the
// reverse complement done on strings; every string and every key array sits in a heap block of its exact size.
//   - every allele of lengths 1..6, and 2,000 generated alleles of each length 7..15: the packed reverse complement equals the string's, twice applied it is the
//     identity, and the locus key under a plus and under a minus plan word decodes to (locus, length, not ambiguous, the expected bases);
//   - x and l at 0 and at 2^29 - 2;
//   - ambiguous records and runs above 15 bases: the key under a minus word is bit for bit the key under a plus word, and decodes to what it was made of.
//   stdout: "<alleles> alleles and <keys> keys checked; <failures> failures"
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>

#include "../mipgen_amd/csrc/gapped_align.h"

static long long g_keys = 0, g_fail = 0;

static void expect(bool ok, const char* what, uint32_t bases, int l, int64_t x)
{
    if (!ok && g_fail++ < 20) fprintf(stderr, "FAIL %s: bases %08x length %d position %lld\n", what, bases, l, (long long)x);
}

// the l letters of a packed allele in a block of exactly l bytes
static std::unique_ptr<char[]> letters_of(uint32_t bases, int l)
{
    std::unique_ptr<char[]> s(new char[(size_t)l]);
    for (int j = 0; j < l; j++) s[(size_t)j] = "ACGT"[(bases >> (2 * (l - 1 - j))) & 3u];
    return s;
}

static uint32_t pack(const char* s, int l)
{
    uint32_t v = 0;
    for (int j = 0; j < l; j++) v = v * 4 + (uint32_t)(strchr("ACGT", s[j]) - "ACGT");
    return v;
}

// the reverse complement on the string, into a block of exactly l bytes
static std::unique_ptr<char[]> string_revcomp(const char* s, int l)
{
    std::unique_ptr<char[]> r(new char[(size_t)l]);
    for (int j = 0; j < l; j++) {
        const char c = s[l - 1 - j];
        r[(size_t)j] = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : 'A';
    }
    return r;
}

static void check_key(uint64_t key, int64_t pos, int l, bool ambiguous, uint32_t bases, const char* what)
{
    g_keys++;
    expect(gap_allele_pos(key) == pos && gap_allele_length(key) == l && gap_allele_ambiguous(key) == ambiguous && gap_allele_bases(key) == bases, what, bases, l, pos);
}

static void check_allele(uint32_t bases, int l)
{
    const std::unique_ptr<char[]> s = letters_of(bases, l), r = string_revcomp(s.get(), l);
    const uint32_t want = pack(r.get(), l), got = gap_allele_revcomp(bases, l);
    expect(got == want, "revcomp", bases, l, 0);
    expect(gap_allele_revcomp(got, l) == bases, "revcomp twice", bases, l, 0);
    const int64_t ends[2] = {0, ((int64_t)1 << 29) - 2};
    std::unique_ptr<uint64_t[]> keys(new uint64_t[4]);
    for (int e = 0; e < 2; e++) {
        const uint32_t word = (uint32_t)ends[e] << 2;
        keys[(size_t)(2 * e)] = gap_locus_allele_key(word | 0u, l, false, bases);
        keys[(size_t)(2 * e + 1)] = gap_locus_allele_key(word | 3u, l, false, bases);
        check_key(keys[(size_t)(2 * e)], ends[e], l, false, bases, "plus key");
        check_key(keys[(size_t)(2 * e + 1)], ends[e], l, false, want, "minus key");
        expect(gap_locus_allele_key(word | 2u, l, false, bases) == gap_allele_key(ends[e], l, false, bases), "bit 1 alone turns nothing", bases, l, ends[e]);
        expect(gap_locus_allele_key(word | 1u, l, false, bases) == gap_allele_key(ends[e], l, false, want), "bit 0 alone turns", bases, l, ends[e]);
        g_keys += 2;
    }
}

int main()
{
    long long alleles = 0;
    for (int l = 1; l <= 6; l++)
        for (uint32_t b = 0; b < (1u << (2 * l)); b++, alleles++) check_allele(b, l);
    uint64_t state = 0x9e3779b97f4a7c15ull;                                     // (xorshift64: the alleles are the same from run to run)
    for (int l = 7; l <= GAP_ALLELE_MAX_LEN; l++)
        for (int k = 0; k < 2000; k++, alleles++) {
            state ^= state << 13; state ^= state >> 7; state ^= state << 17;
            check_allele((uint32_t)(state >> 20) & ((1u << (2 * l)) - 1u), l);
        }
    check_allele((1u << 30) - 1u, 15);
    check_allele(0u, 15);
    alleles += 2;
    // ambiguous records of every spelt length and runs above 15 bases (up to 2 W = 30): a minus source leaves them bit for bit what a plus source makes of them
    const int64_t ends[2] = {0, ((int64_t)1 << 29) - 2};
    for (int e = 0; e < 2; e++)
        for (int l = 1; l <= 30; l++) {
            const uint32_t word = (uint32_t)ends[e] << 2;
            const uint64_t plus = gap_locus_allele_key(word, l, true, 0u), minus = gap_locus_allele_key(word | 3u, l, true, 0u);
            expect(plus == minus && plus == gap_allele_key(ends[e], l, true, 0u), "ambiguous key", 0u, l, ends[e]);
            check_key(minus, ends[e], l, true, 0u, "ambiguous key decoded");
        }
    printf("%lld alleles and %lld keys checked; %lld failures\n", alleles, g_keys, g_fail);
    return g_fail ? 1 : 0;
}
