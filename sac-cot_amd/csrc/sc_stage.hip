// sc_stage.hip — input staging: the user's layout into the padded planes, with the finiteness check, the coordinate statistics and
// the two buffers cleared on the way.  Stage A's tiles are sc_compat.hip, the row statistics and the shard split sc_rows.hip, the
// exclusive scan sc_scan.hip; the host driver of all of it is sc_capi_compat.hip.
#include "sc_arith.hpp"
#include "sc_block.hpp"
#include "sc_kernels.hpp"

namespace sc {

// ------------------------------------------------------------------------------------------------
// input staging: user layout -> 6 zero-padded planes, plus a finiteness check
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void stage_points_kernel(const float* __restrict__ src,
                                                           const float* __restrict__ tgt, int n, int ld,
                                                           int layout, float* __restrict__ planes,
                                                           uint32_t* __restrict__ bad_flag,
                                                           uint32_t* __restrict__ zero, uint32_t zero_words,
                                                           uint32_t* __restrict__ coord_max,
                                                           uint32_t* __restrict__ coord_part,
                                                           uint32_t* __restrict__ mx_ticket,
                                                           uint64_t* __restrict__ host_max,
                                                           uint64_t* __restrict__ host_box,
                                                           uint32_t* __restrict__ zero2, uint32_t zero2_words) {
  int m = blockIdx.x * 256 + threadIdx.x;
  for (uint32_t z = (uint32_t)m; z < zero_words; z += gridDim.x * 256) zero[z] = 0u;  // the per-call control block
  for (uint32_t z = (uint32_t)m; z < zero2_words; z += gridDim.x * 256) zero2[z] = 0u;  // (stage A's deg+ accumulators)
  float v[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (m < n) {
#pragma unroll
    for (int c = 0; c < 3; c++) {
      size_t idx = layout ? ((size_t)c * n + m) : ((size_t)m * 3 + c);
      v[c] = src[idx];
      v[3 + c] = tgt[idx];
    }
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 6; c++) ok = ok && (fabsf(v[c]) < __builtin_inff());
    if (!ok) atomicOr(bad_flag, 1u);
  }
  if (coord_max) {  // largest |coordinate| of either cloud and the two bounding boxes (C2's filters scale and centre by them)
    // coord_max: FX_MX_WORDS words — [0] max |p|, [1] max |q| (non-negative floats order as integers), [2 + c] key(max of
    // coordinate c), [8 + c] key(max of MINUS coordinate c), c = px py pz qx qy qz (float_key orders all floats as
    // unsigned integers, key 0 = "nothing yet").  Pad lanes (m >= n) contribute nothing to the boxes.
    // No same-address atomics (14 words of one cache line from every wave: 15 us): every block leaves its 14 maxima in
    // its own row of coord_part; the block that takes the last ticket reduces the rows.
    __shared__ uint32_t red[4][14];
    uint32_t k14[14];
    k14[0] = __float_as_uint(fmaxf(fabsf(v[0]), fmaxf(fabsf(v[1]), fabsf(v[2]))));
    k14[1] = __float_as_uint(fmaxf(fabsf(v[3]), fmaxf(fabsf(v[4]), fabsf(v[5]))));
#pragma unroll
    for (int c = 0; c < 6; c++) { k14[2 + c] = m < n ? float_key(v[c]) : 0u; k14[8 + c] = m < n ? float_key(-v[c]) : 0u; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
#pragma unroll
      for (int c = 0; c < 14; c++) k14[c] = max(k14[c], (uint32_t)__shfl_xor(k14[c], o));
    if ((threadIdx.x & 63) == 0)
#pragma unroll
      for (int c = 0; c < 14; c++) red[threadIdx.x >> 6][c] = k14[c];
    __syncthreads();
    if (threadIdx.x < 14)
      coord_part[(size_t)blockIdx.x * 16 + threadIdx.x] = max(max(red[0][threadIdx.x], red[1][threadIdx.x]), max(red[2][threadIdx.x], red[3][threadIdx.x]));
    // mx_ticket == nullptr (a host-free call): no workgroup stays behind — stage A's first workgroup reduces the rows (stats_reduce_wave)
    __shared__ uint32_t s_last;
    if (mx_ticket == nullptr) {
      if (threadIdx.x == 0) s_last = 0u;
    } else {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      const uint32_t t = __hip_atomic_fetch_add(mx_ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      s_last = (t == gridDim.x - 1) ? 1u : 0u;
      if (s_last) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    }
    }
    __syncthreads();
    if (s_last) {  // (block-uniform) the last block: reduce the rows, publish
      __shared__ uint32_t fin[16][16];
      const uint32_t c = threadIdx.x & 15, r0 = threadIdx.x >> 4;  // 16 row groups x 16 words
      uint32_t best = 0;
      if (c < 14)
        for (uint32_t r = r0; r < gridDim.x; r += 16)
          best = max(best, __hip_atomic_load(&coord_part[(size_t)r * 16 + c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
      fin[r0][c] = best;
      __syncthreads();
      if (threadIdx.x < 14) {
        uint32_t b2 = 0;
        for (int r = 0; r < 16; r++) b2 = max(b2, fin[r][threadIdx.x]);
        coord_max[threadIdx.x] = b2;   // (plain stores: the next kernels of the stream read them)
        fin[0][threadIdx.x] = b2;
      }
      __syncthreads();
      if (threadIdx.x == 0) {
        // the host gets the two maxima (max |q| << 32 | max |p|, bit patterns) and the boxes: it decides from them which C2
        // kernel can work at this tau (sc_capi.hip decide_filter); nothing waits for it
        if (host_box && host_max)
          for (int k = 0; k < 6; k++)  // (relaxed system-scope stores: the release of host_max below orders them)
            __hip_atomic_store(&host_box[k], ((uint64_t)fin[0][8 + k] << 32) | fin[0][2 + k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(mx_ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // ready for the next call
        // (host_max == nullptr: a host-free call — nothing on the host looks at these words before the call's last kernel, which
        // hands them over with the winner: launch_finalize's DeferredPub.  A system-scope release here costs the staging kernel ~1 us
        // and the launch behind it another: measured, profiles/r05_ab_deferred_publish.txt)
        if (host_max) publish_host(host_max, ((uint64_t)fin[0][1] << 32) | fin[0][0]);  // last: the host takes this word as "the boxes are there too"
      }
    }
  }
  if (m >= ld) return;
#pragma unroll
  for (int c = 0; c < 6; c++) planes[(size_t)c * ld + m] = v[c];
  // AoS copy behind the planes (8 floats per correspondence, 32-byte aligned): stage A fetches a ROW operand with one
  // s_load_dwordx8 instead of six scalar loads and their address arithmetic
  float4* aos = reinterpret_cast<float4*>(planes + 6 * (size_t)ld);
  aos[2 * (size_t)m] = make_float4(v[0], v[1], v[2], v[3]);
  aos[2 * (size_t)m + 1] = make_float4(v[4], v[5], 0.0f, 0.0f);
}

void launch_stage_points(const CoordStatsOut& cs, const ZeroSpan (&zero)[2], const float* d_src, const float* d_tgt, int n, int ld,
                         int layout, float* planes, uint32_t* bad_flag, hipStream_t st) {
  hipLaunchKernelGGL(stage_points_kernel, dim3((ld + 255) / 256), dim3(256), 0, st, d_src, d_tgt, n, ld, layout,
                     planes, bad_flag, zero[0].p, zero[0].words, cs.coord_max, cs.coord_part, cs.mx_ticket, cs.host_max, cs.host_box,
                     zero[1].p, zero[1].words);
}

}  // namespace sc
