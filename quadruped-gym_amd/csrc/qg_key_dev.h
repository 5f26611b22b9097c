// qg_key_dev.h -- the keyed 24-bit draw k(s) of include/quadgym.h (qg_perturb_*, qg_sched_*, qg_cmdcur_*): a pure function of (salted
// seed, global env index, episode, stream), on both sides of a launch.  Shared by qg_perturb.hip, qg_sched.hip and qg_cmdcur.hip;
// each adds its own salt to the seed, so their key spaces are apart.  Internal: not installed, nothing in here is exported.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// the simulator's stream hash (qg_device.h: uniform24s) as the integer behind it
__host__ __device__ static inline uint64_t qgp_mix64(uint64_t x) {
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}
// what (seed_p, env, episode) contribute to every stream of the key
__host__ __device__ static inline uint64_t qgp_key(uint64_t seed_p, uint64_t env_index, uint64_t episode) {
    return seed_p + 0x9E3779B97F4A7C15ull * (env_index + 1) + 0xD1B54A32D192ED03ull * (episode + 1);
}
__host__ __device__ static inline uint32_t qgp_k(uint64_t key, uint64_t stream) {
    return (uint32_t)(qgp_mix64(qgp_mix64(key + 0xA0761D6478BD642Full * stream)) >> 40);
}
