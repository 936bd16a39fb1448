// spmv_pack_check.cpp — stand-alone check of the packed SpMV tile record
// (csrc/spmv_pack.h), built with AddressSanitizer + UndefinedBehaviorSanitizer
// by `make asan-pack` (never shipped). Packs and decodes tiles of the shapes
// the GPU tests run — full tiles, tiles that start or end inside a 16-byte
// vector, the eligibility edge (1536 / 1537 entries fp64, 3072 / 3073 fp32),
// one-row and many-row tiles — in heap buffers of the exact record size, and
// exits non-zero on the first mismatch.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "spmv_pack.h"

namespace {

constexpr int kThreads = 256, kIter = 4;

uint32_t rng_state = 12345u;
uint32_t rnd() {
    rng_state = rng_state * 1664525u + 1013904223u;
    return rng_state >> 8;
}

// One tile: entries [k0, k1) of an entry space of `total`, rows of length
// 1 .. maxrow cycling; slots random below `nslots`.
int check_tile(int vw, int k0, int len, int maxrow, int nslots) {
    const int fields = kIter * vw, k1 = k0 + len, kb = k0 & ~(vw - 1);
    const int total = k1 + 7;
    std::vector<uint16_t> c16((size_t)total);
    for (int e = 0; e < total; e++) c16[(size_t)e] = (uint16_t)(rnd() % (uint32_t)nslots);
    if (kb + kThreads * fields < k1) {
        printf("FAIL: tile of %d entries at %d does not fit %d slots\n", len, k0, kThreads * fields);
        return 1;
    }
    // row offsets: row 0 starts at k0
    std::vector<int> rp(1, k0);
    for (int l = 1; rp.back() < k1; l = l % maxrow + 1) rp.push_back(rp.back() + l < k1 ? rp.back() + l : k1);
    const int nrows = (int)rp.size() - 1;
    const int iw = rsp_pack::index_words(kThreads, fields);
    std::vector<uint32_t> rec((size_t)iw + (size_t)rsp_pack::row_words(nrows));  // exact size: the sanitizer sees any overrun
    rsp_pack::pack_slots(c16.data(), k0, k1, vw, kIter, kThreads, rec.data());
    rsp_pack::pack_rows(rp.data(), 0, nrows, kb, rec.data() + iw);
    for (int e = k0; e < k1; e++)
        if (rsp_pack::unpack_slot(rec.data(), k0, e, vw, kIter, kThreads) != c16[(size_t)e]) {
            printf("FAIL: vw %d k0 %d len %d: slot of entry %d\n", vw, k0, len, e);
            return 1;
        }
    const int nw = rsp_pack::words_per_thread(fields);
    for (int tid = 0; tid < kThreads; tid++)
        for (int f = 0; f < fields; f++) {
            const int e = kb + ((f / vw) * kThreads + tid) * vw + f % vw;
            const uint32_t got = rsp_pack::get_field(rec.data() + (size_t)tid * nw, f);
            const uint32_t want = e >= k0 && e < k1 ? c16[(size_t)e] : 0u;
            if (got != want) {
                printf("FAIL: vw %d k0 %d len %d: thread %d field %d = %u, want %u\n", vw, k0, len, tid, f, got, want);
                return 1;
            }
        }
    for (int i = 0; i <= nrows; i++)
        if (rsp_pack::unpack_row(rec.data() + iw, i) + kb != rp[(size_t)i]) {
            printf("FAIL: vw %d k0 %d len %d: row offset %d\n", vw, k0, len, i);
            return 1;
        }
    return 0;
}

}  // namespace

int main() {
    int bad = 0, n = 0;
    // eligibility: strictly fewer index bytes than 2 B per entry
    bad += rsp_pack::eligible(kThreads, 8, 1536) || !rsp_pack::eligible(kThreads, 8, 1537);
    bad += rsp_pack::eligible(kThreads, 16, 3072) || !rsp_pack::eligible(kThreads, 16, 3073);
    if (bad) printf("FAIL: eligibility edge\n");
    struct Geo { int vw, cap, nslots; } geos[2] = {{2, 2047, 1536}, {4, 4093, 2048}};
    for (const Geo &g : geos) {
        const int lens[] = {1, g.vw, g.cap / 2, g.cap / 2 + 1, 3 * g.cap / 4, 3 * g.cap / 4 + 1, g.cap - 1, g.cap};
        for (int len : lens)
            for (int k0 = 0; k0 < 2 * g.vw; k0++)      // every start inside a vector
                for (int maxrow : {1, 9, 256}) {         // 1-entry rows (most row offsets), mixed, long
                    bad += check_tile(g.vw, k0 + 4096 * (len & 3), len, maxrow, g.nslots);
                    n++;
                }
    }
    // slots at the field limit
    bad += check_tile(2, 5, 2047, 9, 4096);
    bad += check_tile(4, 7, 4093, 9, 4096);
    printf("%s: %d tiles\n", bad ? "FAILED" : "ok", n + 2);
    return bad ? 1 : 0;
}
