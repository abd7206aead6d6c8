// Host harness over juicefs_amd/csrc/jfsx_md5.h (tests/test_md5_host.py):
// a shared library for ctypes, and with -DMD5_HOST_MAIN a stand-alone program
// (built with the address and undefined-behaviour sanitizers) that prints the
// digests of a length sweep over a data file for the test to compare with
// hashlib.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../juicefs_amd/csrc/jfsx_md5.h"

extern "C" {
// one-shot digest of n bytes
void md5_digest(const uint8_t *data, uint64_t n, uint8_t out[16]) { jfsx_md5::digest(data, n, out); }

// the same through update() calls of `step` bytes (the buffering branches)
void md5_stream(const uint8_t *data, uint64_t n, uint64_t step, uint8_t out[16]) {
    jfsx_md5::Ctx c;
    jfsx_md5::init(&c);
    for (uint64_t o = 0; o < n; o += step) jfsx_md5::update(&c, data + o, n - o < step ? n - o : step);
    jfsx_md5::final(&c, out);
}

// the message as nw little-endian words through hash_words / finish_words,
// the path md5_blocks_k takes on the GPU (padding for any multiple of 4 bytes)
void md5_words(const uint8_t *data, uint64_t nw, uint8_t out[16]) {
    uint32_t st[4];
    jfsx_md5::hash_words(st, nw, [&](uint64_t i) {
        const uint8_t *p = data + 4 * i;
        return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
    });
    for (int i = 0; i < 16; i++) out[i] = (uint8_t)(st[i >> 2] >> (8 * (i & 3)));
}
}

#ifdef MD5_HOST_MAIN
static void put(const char *tag, uint64_t n, const uint8_t d[16]) {
    printf("%s %llu ", tag, (unsigned long long)n);
    for (int i = 0; i < 16; i++) printf("%02x", d[i]);
    printf("\n");
}

// md5_host_main FILE: digests of FILE's first n bytes for n = 0..130 (one-shot
// "d", streamed in 7-byte updates "s") and of its first 4 * w bytes for
// w = 1..40 through the word path ("w").  Every buffer is an exact-size heap
// copy, so a read past the message is a sanitizer report.
int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<uint8_t> all(256);
    if (fread(all.data(), 1, all.size(), f) != all.size()) return 2;
    fclose(f);
    uint8_t d[16];
    for (uint64_t n = 0; n <= 130; n++) {
        std::vector<uint8_t> m(all.begin(), all.begin() + n);
        md5_digest(m.data(), n, d);
        put("d", n, d);
        md5_stream(m.data(), n, 7, d);
        put("s", n, d);
    }
    for (uint64_t w = 1; w <= 40; w++) {
        std::vector<uint8_t> m(all.begin(), all.begin() + 4 * w);
        md5_words(m.data(), w, d);
        put("w", 4 * w, d);
    }
    return 0;
}
#endif
