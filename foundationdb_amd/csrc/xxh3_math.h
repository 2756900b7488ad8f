// XXH3-64 / XXH64 algorithm constants and scalar helpers shared by the device
// code that hashes (xxh3_kernels.hip, xxh3_split.hip, redwood.hip).  Device
// translation units only; each gets its own copy of the secret table.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fdbxxh {

constexpr uint64_t P32_1 = 0x9E3779B1u, P32_2 = 0x85EBCA77u, P32_3 = 0xC2B2AE3Du;
constexpr uint64_t P64_1 = 0x9E3779B185EBCA87ull, P64_2 = 0xC2B2AE3D27D4EB4Full, P64_3 = 0x165667B19E3779F9ull;
constexpr uint64_t P64_4 = 0x85EBCA77C2B2AE63ull, P64_5 = 0x27D4EB2F165667C5ull;

// The default secret as 24 little-endian words (xxhash.h:2500-2511).  Internal
// linkage, so that every translation unit can hold its instance -- except
// where the includer asks otherwise: with an internal table the compiler folds
// the words into immediates, which moves the registers of the kernels in
// xxh3_kernels.hip (k_xxh3: 92 -> 90 VGPRs); that file keeps the external
// instance its kernels were tuned with.
#ifndef FDBXXH_SECRET_LINKAGE
#define FDBXXH_SECRET_LINKAGE static
#endif
FDBXXH_SECRET_LINKAGE __constant__ uint64_t kSec[24] = {
    0xbe4ba423396cfeb8ull, 0x1cad21f72c81017cull, 0xdb979083e96dd4deull, 0x1f67b3b7a4a44072ull,
    0x78e5c0cc4ee679cbull, 0x2172ffcc7dd05a82ull, 0x8e2443f7744608b8ull, 0x4c263a81e69035e0ull,
    0xcb00c391bb52283cull, 0xa32e531b8b65d088ull, 0x4ef90da297486471ull, 0xd8acdea946ef1938ull,
    0x3f349ce33f76faa8ull, 0x1d4f0bc7c7bbdcf9ull, 0x3159b4cd4be0518aull, 0x647378d9c97e9fc8ull,
    0xc3ebd33483acc5eaull, 0xeb6313faffa081c5ull, 0x49daf0b751dd0d17ull, 0x9e68d429265516d3ull,
    0xfca1477d58be162bull, 0xce31d07ad1b8f88full, 0x280416958f3acb45ull, 0x7e404bbbcafbd7afull,
};

// Word j of the secret for `seed` (custom secret, xxhash.h:3550-3566; the
// seed-0 secret is the default one).
__device__ __forceinline__ uint64_t sec_word(int j, uint64_t seed) {
	const uint64_t w = kSec[j];
	return (j & 1) ? w - seed : w + seed;
}
// Secret bytes [8j + r, 8j + r + 8), 0 < r < 8.
__device__ __forceinline__ uint64_t sec_at(int j, int r, uint64_t seed) {
	return (sec_word(j, seed) >> (8 * r)) | (sec_word(j + 1, seed) << (64 - 8 * r));
}
// Default-secret bytes at any offset (short paths never use a custom secret).
__device__ __forceinline__ uint64_t ksec(int off) {
	const int j = off >> 3, r = off & 7;
	return r ? (kSec[j] >> (8 * r)) | (kSec[j + 1] << (64 - 8 * r)) : kSec[j];
}
__device__ __forceinline__ uint32_t ksec32(int off) { return (uint32_t)ksec(off); }

__device__ __forceinline__ uint64_t mulfold(uint64_t a, uint64_t b) { return a * b ^ __umul64hi(a, b); }
__device__ __forceinline__ uint64_t rotl64(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }
__device__ __forceinline__ uint64_t xxh64_aval(uint64_t h) {  // xxhash.h:1711-1718
	h ^= h >> 33;
	h *= P64_2;
	h ^= h >> 29;
	h *= P64_3;
	return h ^ (h >> 32);
}
__device__ __forceinline__ uint64_t xxh3_aval(uint64_t h) {  // xxhash.h:2680-2685
	h ^= h >> 37;
	h *= 0x165667919E3779F9ull;
	return h ^ (h >> 32);
}

}  // namespace fdbxxh
