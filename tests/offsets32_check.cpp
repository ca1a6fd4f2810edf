// tests/offsets32_check.cpp -- TEST INFRASTRUCTURE (tests/test_offsets32.py): a stand-alone host program over the headers the kernels and
// pack_scene share.  It checks the 32-bit byte offsets of the per-lane tables (pt_layout.h pair_offset / rec48_offset, pt_device.h table_at /
// const_table_at) against the 64-bit address `base + index` they replace, and the size rule that keeps them exact (table_limit_error).
// One line per check: "ok <what>" or "FAIL <what> ...", and "limit <table> <last accepted> <message of the first refused count>".
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "pt_device.h"

using namespace prt;

static int failures = 0;

static void check(bool ok, const char* what, uint64_t got, uint64_t want) {
    if (ok) std::printf("ok %s\n", what);
    else { std::printf("FAIL %s: got %" PRIu64 ", want %" PRIu64 "\n", what, got, want); ++failures; }
}

// the address the kernels form for record i of a table at `base` against &base[i], both as integers (nothing is dereferenced)
template <typename T>
static void check_address(const char* table, uint64_t base, uint32_t i) {
    char what[160];
    const T* b = reinterpret_cast<const T*>(static_cast<uintptr_t>(base));
    const uint64_t want = base + (uint64_t)i * sizeof(T);
    std::snprintf(what, sizeof(what), "%s[%" PRIu32 "] table_at at base 0x%" PRIx64, table, i, base);
    const uint64_t got = reinterpret_cast<uintptr_t>(dev::table_at(b, i));
    check(got == want, what, got, want);
    std::snprintf(what, sizeof(what), "%s[%" PRIu32 "] const_table_at at base 0x%" PRIx64, table, i, base);
    const uint64_t gotc = reinterpret_cast<uintptr_t>(dev::const_table_at(b, i));
    check(gotc == want, what, gotc, want);
    std::snprintf(what, sizeof(what), "%s[%" PRIu32 "] last byte below 4 GiB", table, i);
    check((uint64_t)i * sizeof(T) + sizeof(T) - 1 <= 0xFFFFFFFFull, what, (uint64_t)i * sizeof(T) + sizeof(T) - 1, 0xFFFFFFFFull);
}

static void check_limit(const char* table, uint64_t last, int which) {
    char what[96];
    uint64_t n[3] = {1, 1, 1};
    n[which] = last;
    std::snprintf(what, sizeof(what), "%s: %" PRIu64 " accepted", table, last);
    check(table_limit_error(n[0], n[1], n[2]) == nullptr, what, 1, 0);
    n[which] = last + 1;
    const char* m = table_limit_error(n[0], n[1], n[2]);
    std::snprintf(what, sizeof(what), "%s: %" PRIu64 " refused", table, last + 1);
    check(m != nullptr, what, 0, 1);
    std::printf("limit %s %" PRIu64 " %s\n", table, last, m ? m : "(none)");
}

int main() {
    // a base with every bit of the low word set but the alignment's, and a high word: a carry out of the low 32 bits must reach it
    const uint64_t bases[2] = {0x00007f3a00000000ull, 0x00007f3afffffff0ull};
    for (uint64_t base : bases) {
        for (uint32_t i : {0u, 1u, PT_MAX_PAIRS - 1u}) check_address<NodePair>("pairs", base, i);
        for (uint32_t i : {0u, 1u, (uint32_t)((1ull << 32) / 48) - 1u, PT_MAX_SLOTS - 1u}) {
            check_address<TriGeom>("tri_geom", base, i);
            check_address<TriNrm>("tri_nrm", base, i);
        }
        for (uint32_t i : {0u, 1u, PT_MAX_MATS - 1u}) check_address<DevMaterial>("mats", base, i);
    }
    check(rec48_offset((uint32_t)((1ull << 32) / 48) - 1u) == 4294967232ull, "slot * 48 at 2^32 / 48 - 1", rec48_offset((uint32_t)((1ull << 32) / 48) - 1u), 4294967232ull);
    check(pair_offset(PT_MAX_PAIRS - 1u) == 4294967168ull, "pair * 64 at the last pair", pair_offset(PT_MAX_PAIRS - 1u), 4294967168ull);
    check_limit("slots", PT_MAX_SLOTS, 0);
    check_limit("pairs", PT_MAX_PAIRS, 1);
    check_limit("materials", PT_MAX_MATS, 2);
    std::printf("%s\n", failures ? "FAILED" : "all ok");
    return failures ? 1 : 0;
}
