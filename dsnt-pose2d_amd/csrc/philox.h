// Philox4x32-10, counter-based: no generator state is carried between calls.  Shared by the augmentation draw and the epoch
// order (augment.hip) and the bootstrap weights (pckh.hip); the counter's last word is the domain that keeps their streams
// of one seed apart.  Restated in numpy by tests/loader_ref.py.
#pragma once
#include <stdint.h>

struct Philox {
    __device__ static void round(uint32_t ctr[4], const uint32_t key[2]) {
        const uint32_t lo0 = 0xD2511F53u * ctr[0], hi0 = __umulhi(0xD2511F53u, ctr[0]);
        const uint32_t lo1 = 0xCD9E8D57u * ctr[2], hi1 = __umulhi(0xCD9E8D57u, ctr[2]);
        const uint32_t c0 = hi1 ^ ctr[1] ^ key[0], c2 = hi0 ^ ctr[3] ^ key[1];
        ctr[0] = c0; ctr[1] = lo1; ctr[2] = c2; ctr[3] = lo0;
    }
    // Philox4x32-10
    __device__ static void gen(uint32_t out[4], uint64_t seed, uint64_t step, uint32_t sample, uint32_t k) {
        uint32_t ctr[4] = {sample, (uint32_t)step, (uint32_t)(step >> 32), k};
        uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
        for (int r = 0; r < 10; ++r) {
            round(ctr, key);
            key[0] += 0x9E3779B9u;
            key[1] += 0xBB67AE85u;
        }
        for (int i = 0; i < 4; ++i) out[i] = ctr[i];
    }
};
