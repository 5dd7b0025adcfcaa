// count_row.h — one row of a finished count table through wide loads and stores: what kernels_call.hip and kernels_locus.hip (4.15) share.  A gapped row
// is 32 bytes and 32-byte aligned: two 16-byte accesses.  An ungapped row is 20 bytes and only 4-byte aligned: a 16-byte access the compiler is told not to assume
// aligned, and a 4-byte one.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef int call_v4i __attribute__((ext_vector_type(4)));
struct CallRow4 { call_v4i v; } __attribute__((packed, aligned(4)));       // four counters of a row that is only 4-byte aligned

// the 5 or 8 counters of position x into c[8] (the columns a 5-column row lacks stay 0)
__device__ static inline void call_load_row(const int32_t* __restrict__ counts, int columns, int64_t x, int32_t c[8])
{
    if (columns == 8) {
        const call_v4i a = *(const call_v4i*)(counts + x * 8), b = *(const call_v4i*)(counts + x * 8 + 4);
        c[0] = a.x; c[1] = a.y; c[2] = a.z; c[3] = a.w; c[4] = b.x; c[5] = b.y; c[6] = b.z; c[7] = b.w;
    } else {
        const call_v4i a = ((const CallRow4*)(counts + x * 5))->v;
        c[0] = a.x; c[1] = a.y; c[2] = a.z; c[3] = a.w; c[4] = counts[x * 5 + 4]; c[5] = 0; c[6] = 0; c[7] = 0;
    }
}

// c[0, columns) to position x, with the same accesses
__device__ static inline void call_store_row(int32_t* __restrict__ counts, int columns, int64_t x, const int32_t c[8])
{
    call_v4i a;
    a.x = c[0]; a.y = c[1]; a.z = c[2]; a.w = c[3];
    if (columns == 8) {
        call_v4i b;
        b.x = c[4]; b.y = c[5]; b.z = c[6]; b.w = c[7];
        *(call_v4i*)(counts + x * 8) = a; *(call_v4i*)(counts + x * 8 + 4) = b;
    } else {
        ((CallRow4*)(counts + x * 5))->v = a;
        counts[x * 5 + 4] = c[4];
    }
}
