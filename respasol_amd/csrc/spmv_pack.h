// spmv_pack.h — the packed record of a staged SpMV tile (spmv_plan.cpp
// pack_staged_tiles writes it, spmv.hip stream_products_staged / spmv_tile
// read it, rsp_plan::plan_verify decodes it). Plain C++: no HIP dependency, so the
// arithmetic also builds into the stand-alone sanitizer check
// (drivers/spmv_pack_check.cpp, make asan-pack).
//
// A staged tile's per-entry index is an LDS slot below kStageSlots <= 2048:
// 12 bits. The record of a tile over entries [k0, k1), kb = k0 rounded down
// to the vector width VW, is, in 32-bit words:
//   [0, NTH * NW)  slot fields: thread tid owns the IT * VW consecutive
//                  12-bit fields of words [tid * NW, (tid + 1) * NW), least
//                  significant first; field it * VW + j is the slot of entry
//                  kb + (it * NTH + tid) * VW + j, 0 outside [k0, k1);
//   then           (rows mode) nrows + 1 uint16 row offsets rowptr[r0 + i] -
//                  kb, two per word (low half first), padded to a whole word.
// NW = IT * VW * 12 / 32: 3 words per thread for fp64, 6 for fp32.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define RSP_PK_HD __host__ __device__ __forceinline__
#else
#define RSP_PK_HD inline
#endif

namespace rsp_pack {

constexpr int kBits = 12;
constexpr uint32_t kMask = (1u << kBits) - 1;

// words per thread for `fields` 12-bit fields (whole words only)
constexpr int words_per_thread(int fields) { return fields * kBits / 32; }
static_assert(words_per_thread(8) == 3 && words_per_thread(16) == 6, "fp64 / fp32 geometry");

// slot-field words of a record
constexpr int index_words(int nth, int fields) { return nth * words_per_thread(fields); }
// row-offset words of a record with `nrows` rows
RSP_PK_HD int row_words(int nrows) { return (nrows + 2) >> 1; }

// index bytes of a packed tile against the 2 B per entry of an unpacked one:
// packed only when strictly fewer
RSP_PK_HD bool eligible(int nth, int fields, int len) {
    return (long long)index_words(nth, fields) * 4 < 2LL * len;
}

// field f of a thread's words w[0 .. NW)
RSP_PK_HD uint32_t get_field(const uint32_t *w, int f) {
    const int b = f * kBits, i = b >> 5, s = b & 31;
    uint32_t v = w[i] >> s;
    if (s > 32 - kBits) v |= w[i + 1] << (32 - s);
    return v & kMask;
}

// OR field f into a thread's zeroed words
RSP_PK_HD void put_field(uint32_t *w, int f, uint32_t slot) {
    const int b = f * kBits, i = b >> 5, s = b & 31;
    slot &= kMask;
    w[i] |= slot << s;
    if (s > 32 - kBits) w[i + 1] |= slot >> (32 - s);
}

// Slot fields of one tile: c16[e] is entry e's slot (the plan's 16-bit array,
// indexed by entry). out: index_words(NTH, IT * VW) words.
inline void pack_slots(const uint16_t *c16, int k0, int k1, int vw, int it_n, int nth, uint32_t *out) {
    const int fields = it_n * vw, nw = words_per_thread(fields);
    const int kb = k0 & ~(vw - 1);
    for (int i = 0; i < nth * nw; i++) out[i] = 0;
    for (int tid = 0; tid < nth; tid++)
        for (int it = 0; it < it_n; it++)
            for (int j = 0; j < vw; j++) {
                const long long e = (long long)kb + (long long)(it * nth + tid) * vw + j;
                if (e >= k0 && e < k1) put_field(out + (size_t)tid * nw, it * vw + j, c16[e]);
            }
}

// The slot of entry e (k0 <= e < k1) read back from a tile's fields.
inline uint32_t unpack_slot(const uint32_t *rec, int k0, int e, int vw, int it_n, int nth) {
    const int fields = it_n * vw, nw = words_per_thread(fields);
    const int kb = k0 & ~(vw - 1);
    const int v = (e - kb) / vw, j = (e - kb) % vw;
    const int it = v / nth, tid = v % nth;
    return get_field(rec + (size_t)tid * nw, it * vw + j);
}

// Row offsets rp[r0 + i] - kb, i in [0, nrows]. out: row_words(nrows) words.
inline void pack_rows(const int *rp, int r0, int nrows, int kb, uint32_t *out) {
    const int n = row_words(nrows);
    for (int i = 0; i < n; i++) out[i] = 0;
    for (int i = 0; i <= nrows; i++) out[i >> 1] |= (uint32_t)(uint16_t)(rp[r0 + i] - kb) << (16 * (i & 1));
}

inline int unpack_row(const uint32_t *rows, int i) { return (int)((rows[i >> 1] >> (16 * (i & 1))) & 0xffffu); }

}  // namespace rsp_pack
