// dsn_philox.h - Philox4x32-10, the project's counter-based generator: four 32-bit words per (counter, key), no state.  Its users fix
// what the counter words mean: dsn_train_draws (dsn_rng.hip) and dsn_mesh_sample_surface (dsn_meshdist.hip), rules in include/dsnerf.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct DsnPhiloxOut { uint32_t x[4]; };

__device__ __forceinline__ DsnPhiloxOut dsn_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
    for (int i = 0; i < 10; ++i) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c0 = n0;
        c1 = (uint32_t)p1;
        c2 = n2;
        c3 = (uint32_t)p0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return {{c0, c1, c2, c3}};
}
