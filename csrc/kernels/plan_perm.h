// Keyed Feistel permutations of [0, n): the integer math shared by the visit plans (plan.hip) and the DnC column
// sub-sampling (agg.hip k_dnc_gram).  6-round balanced Feistel network on the smallest even bit-width domain covering
// n, with cycle walking back into [0, n).  __host__ __device__, so csrc/host/host_check.hip runs the same code under
// ASan/UBSan on the CPU; mirrored bit-for-bit by attackfl_amd/fl/trainers.py (_mix_i, _perm_t, _half_bits) and
// attackfl_amd/ops/composite.py (dnc_keys, dnc_columns, signguard_mix).
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

__host__ __device__ __forceinline__ uint32_t pl_mix(uint32_t x) {
  x ^= x >> 16;
  x *= 0x85EBCA6Bu;
  x ^= x >> 13;
  x *= 0xC2B2AE35u;
  x ^= x >> 16;
  return x;
}

__host__ __device__ __forceinline__ uint32_t pl_feistel(uint32_t x, int half, uint32_t mask, uint32_t k0, uint32_t k1) {
  uint32_t L = x >> half, R = x & mask;
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    const uint32_t F = pl_mix(R ^ k0 ^ (k1 + 0x9E3779B9u * (uint32_t)(r + 1))) & mask;
    const uint32_t nL = R;
    R = L ^ F;
    L = nL;
  }
  return (L << half) | R;
}

__host__ __device__ __forceinline__ uint32_t pl_perm(uint32_t x, uint32_t n, int half, uint32_t k0, uint32_t k1) {
  const uint32_t mask = (1u << half) - 1u;
  do {
    x = pl_feistel(x, half, mask, k0, k1);
  } while (x >= n);
  return x;
}

__host__ __device__ __forceinline__ int pl_half_bits(uint32_t n) {
  int k = 2;
  while ((1ull << k) < (unsigned long long)n) k += 2;
  return k / 2;
}

// DnC (docs/PARITY.md): the two keys of iteration t's column permutation pi_t from the round's 64-bit seed — the one
// place the derivation is written down on the native side.  Column i of iteration t is
// pl_perm(i, P, pl_half_bits(P), k0, k1) for i < b when b < P, and i itself when b >= P.
struct DncKeys {
  uint32_t k0, k1;
};
__host__ __device__ __forceinline__ DncKeys pl_dnc_keys(uint64_t seed, int t) {
  const uint32_t a = pl_mix((uint32_t)seed ^ 0x2545F491u), b = pl_mix((uint32_t)(seed >> 32) ^ 0x7F4A7C15u);
  DncKeys k;
  k.k0 = pl_mix(a ^ (0x165667B1u * (uint32_t)(t + 1)));
  k.k1 = pl_mix(b + 0xD3A2646Cu * (uint32_t)(t + 1));
  return k;
}

// SignGuard (docs/PARITY.md): the first column s of the round's contiguous sampled window {s, ..., s + b - 1 mod P}
// from the round's 64-bit seed, s = mix(seed) mod P (the caller takes s = 0 when the window is all P columns) — the one
// place the derivation is written down on the native side.
__host__ __device__ __forceinline__ uint32_t pl_signguard_mix(uint64_t seed) {
  const uint32_t a = pl_mix((uint32_t)seed ^ 0x5347D1A3u), b = pl_mix((uint32_t)(seed >> 32) ^ 0x6A09E667u);
  return pl_mix(a + 0x9E3779B9u * b);
}
__host__ __device__ __forceinline__ uint32_t pl_signguard_start(uint64_t seed, uint32_t P) {
  return pl_signguard_mix(seed) % P;
}
