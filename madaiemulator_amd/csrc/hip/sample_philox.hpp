// sample_philox.hpp -- the random numbers of the ensemble sampler (gpemu.h): Philox4x32-10 (Salmon et al.
// 2011) and the uniform made of two of its words.  One body for the kernels of kernels_sample.hip and for the host entries
// gpemu_philox4x32 / gpemu_sample_uniforms: integer arithmetic and one exact fp64 product, the same bits everywhere.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace gpemu {

__host__ __device__ inline void philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4])
{
	uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3], k0 = key[0], k1 = key[1];
	for (int r = 0; r < 10; r++) {
		const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
		const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
		c1 = (uint32_t)p1; c3 = (uint32_t)p0;
		c0 = n0; c2 = n2;
		k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
	}
	out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// U(a, b) = ((a << 20 | b >> 12) + 0.5) 2^-52: 52 bits, strictly inside (0, 1), exact in fp64 (2 n + 1 < 2^53)
__host__ __device__ inline double philox_uniform(uint32_t a, uint32_t b)
{
	const uint64_t n = ((uint64_t)a << 20) | (uint64_t)(b >> 12);
	return (double)(2 * n + 1) * 0x1p-53;
}

// the words of counter (c0, lo, hi, c3) under the key of `seed`
__host__ __device__ inline void sample_words(unsigned long long seed, uint32_t c0, unsigned long long c12, uint32_t c3, uint32_t w[4])
{
	const uint32_t ctr[4] = {c0, (uint32_t)(c12 & 0xffffffffull), (uint32_t)(c12 >> 32), c3};
	const uint32_t key[2] = {(uint32_t)(seed & 0xffffffffull), (uint32_t)(seed >> 32)};
	philox4x32_10(ctr, key, w);
}

// walker k at global step t: u1 (the partner), u2 (the stretch) from counter (k, t, 0), u3 (the accept step) from (k, t, 1)
__host__ __device__ inline void sample_u12(unsigned long long seed, uint32_t walker, unsigned long long step, double *u1, double *u2)
{
	uint32_t w[4];
	sample_words(seed, walker, step, 0u, w);
	*u1 = philox_uniform(w[0], w[1]);
	*u2 = philox_uniform(w[2], w[3]);
}
__host__ __device__ inline double sample_u3(unsigned long long seed, uint32_t walker, unsigned long long step)
{
	uint32_t w[4];
	sample_words(seed, walker, step, 1u, w);
	return philox_uniform(w[0], w[1]);
}

} // namespace gpemu
