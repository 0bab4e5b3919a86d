// philox.h -- the counter-based generator host and device share: CoreSLAM's candidate jitters (coreslam.hip, k_jitter), the device
// known-answer call slamhip_ctx_philox4x32_10, and the particle filter's noise and resampling offset (hs_mcl.h).  Integer
// arithmetic only: the same words everywhere.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3")
__host__ __device__ static inline void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1)
{
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1, n3 = (uint32_t)p0;
        c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}
