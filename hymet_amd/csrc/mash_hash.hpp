// Mash's k-mer hashing on the device, shared by the screen (screen.hip) and the sketch
// builder (sketch.hip): MurmurHash3_x64_128 word 0 / MurmurHash3_x86_32 of a k-mer held as
// little-endian ASCII words, and the rolling forward / reverse-complement state that feeds
// them one 2-bit base at a time.
#pragma once
#include "common.hpp"

namespace hymet {
namespace mash {

__device__ __forceinline__ uint64_t rotl64(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }
__device__ __forceinline__ uint64_t fmix64(uint64_t k) {
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdULL;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ULL;
    k ^= k >> 33;
    return k;
}

// MurmurHash3_x64_128 word 0 of a K-byte key held little-endian in w[0..3].
template <int K>
__device__ __forceinline__ uint64_t murmur3_h0(const uint64_t (&w)[4], uint32_t seed) {
    constexpr uint64_t c1 = 0x87c37b91114253d5ULL, c2 = 0x4cf5ad432745937fULL;
    constexpr int NB = K / 16, TAIL = K & 15;
    uint64_t h1 = seed, h2 = seed;
#pragma unroll
    for (int b = 0; b < NB; b++) {
        uint64_t k1 = w[2 * b], k2 = w[2 * b + 1];
        k1 *= c1; k1 = rotl64(k1, 31); k1 *= c2; h1 ^= k1;
        h1 = rotl64(h1, 27); h1 += h2; h1 = h1 * 5 + 0x52dce729;
        k2 *= c2; k2 = rotl64(k2, 33); k2 *= c1; h2 ^= k2;
        h2 = rotl64(h2, 31); h2 += h1; h2 = h2 * 5 + 0x38495ab5;
    }
    if constexpr (TAIL > 8) {
        uint64_t k2 = w[2 * NB + 1];
        k2 *= c2; k2 = rotl64(k2, 33); k2 *= c1; h2 ^= k2;
    }
    if constexpr (TAIL > 0) {
        uint64_t k1 = w[2 * NB];
        k1 *= c1; k1 = rotl64(k1, 31); k1 *= c2; h1 ^= k1;
    }
    h1 ^= (uint64_t)K;
    h2 ^= (uint64_t)K;
    h1 += h2;
    h2 += h1;
    h1 = fmix64(h1);
    h2 = fmix64(h2);
    return h1 + h2;
}

__device__ __forceinline__ uint32_t rotl32(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }

// MurmurHash3_x86_32 of a K-byte key (K <= 16) held little-endian in w[0..1], bytes past K zero.
template <int K>
__device__ __forceinline__ uint32_t murmur3_x86_32(const uint64_t (&w)[4], uint32_t seed) {
    constexpr uint32_t c1 = 0xcc9e2d51u, c2 = 0x1b873593u;
    constexpr int NB = K / 4, TAIL = K & 3;
    uint32_t h1 = seed;
#pragma unroll
    for (int b = 0; b < NB; b++) {
        uint32_t k1 = (uint32_t)(w[b >> 1] >> (32 * (b & 1)));
        k1 *= c1; k1 = rotl32(k1, 15); k1 *= c2;
        h1 ^= k1; h1 = rotl32(h1, 13); h1 = h1 * 5 + 0xe6546b64u;
    }
    if constexpr (TAIL > 0) {
        uint32_t k1 = (uint32_t)(w[NB >> 1] >> (32 * (NB & 1)));  // the K & 3 tail bytes, zero above
        k1 *= c1; k1 = rotl32(k1, 15); k1 *= c2; h1 ^= k1;
    }
    h1 ^= (uint32_t)K;
    h1 ^= h1 >> 16; h1 *= 0x85ebca6bu;
    h1 ^= h1 >> 13; h1 *= 0xc2b2ae35u;
    h1 ^= h1 >> 16;
    return h1;
}

template <int K>
__device__ __forceinline__ uint64_t mash_hash(const uint64_t (&w)[4], uint32_t seed) {
    if constexpr (K <= 16) return (uint64_t)murmur3_x86_32<K>(w, seed);
    else return murmur3_h0<K>(w, seed);
}

__device__ __forceinline__ uint32_t ascii_of(uint32_t c) { return (0x54474341u >> (8 * c)) & 0xFFu; }

// Rolling state of the k-mer ending at the last pushed base: 2-bit forward and
// reverse-complement words (the canonical strand is decided by integer compare, == Mash's
// memcmp on ASCII since A<C<G<T) and the two strands' ASCII byte windows (what is hashed).
template <int K>
struct KmerRoll {
    static constexpr int NW = (K + 7) / 8;
    static constexpr int TOPB = K - 8 * (NW - 1);
    static constexpr uint64_t TOPMASK = TOPB == 8 ? ~0ull : ((1ull << (8 * TOPB)) - 1);
    static constexpr uint64_t KMASK = K == 32 ? ~0ull : ((1ull << (2 * K)) - 1);
    uint64_t fwd = 0, rc = 0;
    uint64_t F[4] = {0, 0, 0, 0}, R[4] = {0, 0, 0, 0};

    __device__ __forceinline__ void push(uint32_t c) {
        fwd = ((fwd << 2) | c) & KMASK;
        rc = (rc >> 2) | ((uint64_t)(3u - c) << (2 * (K - 1)));
#pragma unroll
        for (int j = 0; j < NW - 1; j++) F[j] = (F[j] >> 8) | (F[j + 1] << 56);
        F[NW - 1] = (F[NW - 1] >> 8) | ((uint64_t)ascii_of(c) << (8 * (TOPB - 1)));
#pragma unroll
        for (int j = NW - 1; j > 0; j--) R[j] = (R[j] << 8) | (R[j - 1] >> 56);
        R[0] = (R[0] << 8) | ascii_of(3u - c);
        R[NW - 1] &= TOPMASK;
    }
    // the canonical k-mer's hash
    __device__ __forceinline__ uint64_t hash(uint32_t seed) const {
        return (rc < fwd) ? mash_hash<K>(R, seed) : mash_hash<K>(F, seed);
    }
};

}  // namespace mash
}  // namespace hymet
