// rc_rates_bin.inc — the binning block of k_rates_render (rc_sample_kernels.hip, where the scheme
// is described), as program text: included inside a kernel body that has run nothing yet, on
// launch_rates_render's 2-D grid of kBlock threads, with these names in scope: rates, W, H,
// list2up, list4, list8down, cnt, and the two LDS arrays
//   __shared__ unsigned wsum[kBlock / 64][5];   per wave: the chunk's pixels per counter of cnt
//   __shared__ unsigned wbase[3];               the chunk's first slot in each list
// As a __forceinline__ function the block compiled to other instructions inside k_rates_render
// (commuted operands, other registers), so it stays text; the test harness
// (tests/tools/list_check.hip) includes the same file.  kRateChunk and the two hooks
// (RC_RATES_LAST_CHUNK, RC_RATES_WAVE_BASE) are rc_lists.hpp's.
  {
    const int lin = (int)blockIdx.y * (int)gridDim.x + (int)blockIdx.x;
    const int nwg = (int)gridDim.x * (int)gridDim.y;
    const int chunk = lin / kRateChunk;
    int duty = chunk % kRateChunk;   // which workgroup of the chunk's kRateChunk bins it
    RC_RATES_LAST_CHUNK(chunk, duty, nwg);
    if (lin % kRateChunk == duty) {   // uniform over the workgroup: the barriers below are too
      const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
      const unsigned long long below = (1ull << lane) - 1ull;
      const size_t n = (size_t)W * H;   // < 2^32; the grid's workgroups * 256 >= n
      const size_t first = (size_t)chunk * (kRateChunk * kBlock) + threadIdx.x;
      unsigned tot[5] = {0u, 0u, 0u, 0u, 0u};
#pragma unroll
      for (int it = 0; it < kRateChunk; ++it) {
        const size_t i = first + (size_t)it * kBlock;
        const unsigned rate = i < n ? (unsigned)rates[i] : 0u;
#pragma unroll
        for (int k = 0; k < 3; ++k) tot[k] += (unsigned)__popcll(__ballot(rate == (2u << k)));
        tot[3] += (unsigned)__popcll(__ballot(rate == 1u));
        tot[4] += (unsigned)__popcll(__ballot(!(rate <= 2u || rate == 4u || rate == 8u)));
      }
      if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 5; ++k) wsum[wave][k] = tot[k];
      }
      __syncthreads();
      if (threadIdx.x < 5) {
        unsigned sum = 0u;
        for (int w = 0; w < kBlock / 64; ++w) sum += wsum[w][threadIdx.x];
        unsigned base = 0u;
        if (sum) base = atomicAdd(cnt + threadIdx.x, sum);
        if (threadIdx.x < 3) wbase[threadIdx.x] = base;
      }
      __syncthreads();
      unsigned base[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        base[k] = wbase[k];
        for (int w = 0; w < wave; ++w) RC_RATES_WAVE_BASE(base[k], wsum[w][k]);
      }
      if (tot[0] | tot[1] | tot[2]) {   // uniform over the wave
#pragma unroll
        for (int it = 0; it < kRateChunk; ++it) {
          const size_t i = first + (size_t)it * kBlock;
          const unsigned rate = i < n ? (unsigned)rates[i] : 0u;
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            const unsigned long long m = __ballot(rate == (2u << k));
            if ((m >> lane) & 1ull) {   // i < n: a pixel index below 2^32
              const size_t at = (size_t)base[k] + (unsigned)__popcll(m & below);
              if (k == 0) list2up[at] = (uint32_t)i;
              else if (k == 1) list4[at] = (uint32_t)i;
              else *(list8down - at) = (uint32_t)i;
            }
            base[k] += (unsigned)__popcll(m);
          }
        }
      }
    }
  }
