// sc_chunks.hpp — the chunk scratch of the frame kernels that sum over a pose's inliers in chunks of 64 consecutive correspondences
// (polish_kernel, polish_poses_kernel, pose_info_frame_kernel, settle_frame_kernel), said once: per pose ceil(n / 64) chunks of
// CHUNK_DOUBLES doubles in global memory, a chunk's sums first and its 64 inlier bits in slot BITS_SLOT.  The accessors are the
// storage policy `Chunks` of refit_iterate (sc_refit.hpp) and, pose-major, of settle_run (sc_settle.hpp); the host sizes a buffer with
// chunk_scratch_bytes.  One definition, so a buffer that serves two entries (ppose_tmp: sc_polish_poses and sc_settle_poses_frame,
// stream-ordered) holds one layout by construction.
#pragma once
#include <cstddef>
#include <cstdint>

#include <hip/hip_runtime.h>

namespace sc {

constexpr int CHUNK_DOUBLES = 16, BITS_SLOT = 15;
constexpr int REFIT_NSUM = 9;  // the sums a refit keeps per chunk (its second pass; the first keeps 7); the information matrix: INFO_NSUM
// bytes of one pose's chunks for n correspondences
inline size_t chunk_scratch_bytes(int n) { return (size_t)((n + 63) / 64) * CHUNK_DOUBLES * sizeof(double); }

// One pose's chunks, NSUM sums each.  Global memory: a block fence publishes a lane's stores before the barrier behind which other
// lanes read them.
template <int NSUM>
struct ChunkScratch {
  static_assert(NSUM <= BITS_SLOT, "the sums and the bit word do not overlap");
  double* base;
  // pose k's block of a buffer that holds the poses one behind the other
  __device__ __forceinline__ static ChunkScratch of_pose(double* all, uint32_t k, int n) { return ChunkScratch{all + (size_t)k * (size_t)((n + 63) / 64) * CHUNK_DOUBLES}; }
  __device__ __forceinline__ double& sum(int ch, int k) const { return base[(size_t)ch * CHUNK_DOUBLES + k]; }
  __device__ __forceinline__ uint64_t& bits(int ch) const {
    return reinterpret_cast<uint64_t*>(base)[(size_t)ch * CHUNK_DOUBLES + BITS_SLOT];
  }
  __device__ __forceinline__ void publish() const { __threadfence_block(); }
};

// The same buffer seen by ONE workgroup that owns every pose: pose k's block, then chunk ch in it.
template <int NSUM>
struct PoseChunks {
  static_assert(NSUM <= BITS_SLOT, "the sums and the bit word do not overlap");
  double* base;
  int nch;
  __device__ __forceinline__ size_t at(int k, int ch) const { return ((size_t)k * nch + ch) * CHUNK_DOUBLES; }
  __device__ __forceinline__ double& sum(int k, int ch, int slot) const { return base[at(k, ch) + slot]; }
  __device__ __forceinline__ uint64_t& bits(int k, int ch) const { return reinterpret_cast<uint64_t*>(base)[at(k, ch) + BITS_SLOT]; }
  __device__ __forceinline__ void publish() const { __threadfence_block(); }
};

}  // namespace sc
