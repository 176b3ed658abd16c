// The counter-based hash of the seeded generators, shared by the probe library (sgl_synth.hip: the synthetic graphs) and the product
// library (sgl_edge_split.hip: the candidate stream of the negative edges; sgl_csr_select.hip: the random edge drop).  Integer arithmetic only, so a device and its numpy mirror
// (sgl_amd/synthetic.py: _mix64, _hash4, _mulhi64) agree bit for bit.
//
//   h(seed, stream, a, b) = mix(mix(mix(seed * GOLD + stream) ^ a) + b),  mix = the splitmix64 finaliser
//   mulhi64(h, n)         = floor(h * n / 2^64): h scaled into [0, n) without a division
//
// Streams in use: 0 degree, 1 column, 2 value, 3 feature (sgl_synth.hip); 101 edge shuffle, 102 negative-edge candidates (the split);
// 103 edge drop (sgl_csr_select.hip: a = row, b = column of the entry, or the pair's (min, max)), 104 node drop (sgl_amd/transforms.py:
// a = node, b = 0).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace {

__host__ __device__ __forceinline__ uint64_t mix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__host__ __device__ __forceinline__ uint64_t hash4(uint64_t seed, uint64_t stream, uint64_t a, uint64_t b) {
    return mix64(mix64(mix64(seed * 0x9E3779B97F4A7C15ull + stream) ^ a) + b);
}

__device__ __forceinline__ uint64_t mulhi64(uint64_t a, uint64_t b) { return __umul64hi(a, b); }

}  // namespace
