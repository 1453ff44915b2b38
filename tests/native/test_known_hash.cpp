// Driver for pbs_plus_amd/csrc/known_hash.h (the hash of the known-chunk set), host only: the functions the kernels of
// known.hip call, compiled as plain C++.
// Reads one digest per line from stdin (64 hex characters, byte 0 first) and answers each with
//   "<home> <key> <tag>"   (known_home as 16 hex digits, known_key as 8, known_tag as 16)
// The words are loaded by known_load from a 48-byte record, so its little-endian reading of the bytes is part of what is
// printed. tests/test_known_inputs.py compares the answers with the Python port of tests/known_inputs.py.
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "../../pbs_plus_amd/csrc/known_hash.h"

static int hexval(int c) {
    if (c >= '0' && c <= '9') return c - '0';
    if (c >= 'a' && c <= 'f') return c - 'a' + 10;
    if (c >= 'A' && c <= 'F') return c - 'A' + 10;
    return -1;
}

int main() {
    char line[128];
    while (std::scanf("%127s", line) == 1) {
        if (std::strlen(line) != 64) return 2;
        alignas(8) uint8_t rec[2 * 48] = {};  // record 1 of two: known_load's stride is used as well
        for (int b = 0; b < 32; ++b) {
            const int hi = hexval(line[2 * b]), lo = hexval(line[2 * b + 1]);
            if (hi < 0 || lo < 0) return 3;
            rec[48 + 8 + b] = (uint8_t)(hi * 16 + lo);
        }
        uint64_t w[4];
        pbsk::known_load(rec, 48, 1, w);
        const uint64_t h = pbsk::known_home(w);
        std::printf("%016" PRIx64 " %08" PRIx32 " %016" PRIx64 "\n", h, pbsk::known_key(h, w), pbsk::known_tag(w[0]));
    }
    std::printf("known-hash-ok\n");
    return 0;
}
