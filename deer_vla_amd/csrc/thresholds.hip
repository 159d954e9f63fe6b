// Exit thresholds of k operating points from one calibration matrix, on the device: the solver of ExitController.set_threshold
// (robot_flamingo/models/value_net.py:242-262) for many points per launch.
//
// values [n_stage][ld] holds the deltas of every calibration sample at every exit.  For point p and exit e (all but the last) the
// reference sorts row e, walks it until out_n[p][e] not-yet-exited samples have passed, takes that value as the threshold and marks every
// sample with v <= T as exited.  Here
//   solve_thresholds_kernel   one workgroup per point, exits in order inside it.  The c-th order statistic over the alive samples is a
//                             radix SELECT: four passes over the row, each a 256-bin histogram (LDS, integer atomics) of one byte of an
//                             order-preserving 32-bit key among the samples that match the bytes chosen so far, then a scan of the bins.
//                             A fifth pass applies the threshold and rewrites the alive bytes (alive_scratch, one byte per sample and point).
// Integer counting only: the result does not depend on the order in which threads arrive.  No float atomics, no grid barrier; every
// store to device memory is a vector-memory store.  A thread visits the same samples in every pass, so it reads back only alive bytes
// it wrote itself.
#include "common.h"
#include "../../include/deer_hip.h"

namespace {

// f32 bits -> unsigned key with the same order as the floats (-inf lowest; -0.0 just below +0.0; NaNs beyond the infinities), and back
__device__ __forceinline__ unsigned key_of(float v) {
  const unsigned u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float value_of(unsigned key) {
  return __uint_as_float((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key);
}

// f(i, row[i]) for the samples of this thread: 16-byte loads where the rows allow them (vec: base 16-byte aligned, ld % 4 == 0), the
// tail and unaligned rows one by one.  The sample -> thread assignment depends on (n, vec) only.
template <class F>
__device__ __forceinline__ void for_each_sample(const float* __restrict__ row, int n, int vec, F f) {
  const int n4 = vec ? n >> 2 : 0;
  for (int j = threadIdx.x; j < n4; j += 256) {
    const float4 v = *reinterpret_cast<const float4*>(row + 4 * j);
    f(4 * j, v.x);
    f(4 * j + 1, v.y);
    f(4 * j + 2, v.z);
    f(4 * j + 3, v.w);
  }
  for (int i = 4 * n4 + threadIdx.x; i < n; i += 256) f(i, row[i]);
}

__global__ __launch_bounds__(256) void solve_thresholds_kernel(const float* __restrict__ values, int n_sample, long ld,
                                                               const int* __restrict__ out_n, int n_exit, int leq,
                                                               unsigned char* __restrict__ alive_all, float* __restrict__ thresholds,
                                                               int* __restrict__ exit_counts, int* __restrict__ status, int vec) {
  __shared__ unsigned hist[256];
  __shared__ unsigned wave_sum[4];
  __shared__ unsigned sel[2];        // the bin that holds the k-th key, and k inside that bin
  __shared__ int tally[2];           // samples that left at this exit; NaNs met so far
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const long p = blockIdx.x;
  unsigned char* alive = alive_all + p * n_sample;
  const unsigned flip = leq ? 0u : 0xffffffffu;      // descending order = ascending order of the complemented key
  const float sentinel = leq ? -1e8f : 1e8f;
  int a = n_sample;                                  // alive count, the same in every thread
  if (t == 0) tally[1] = 0;
  for (int e = 0; e + 1 < n_exit; ++e) {
    const float* row = values + (long)e * ld;
    const int c = out_n[p * n_exit + e];
    const bool all_alive = e == 0;                   // nobody has left yet: the alive bytes are first written by this exit's last pass
    float T = sentinel;
    if (c >= 1 && c <= a) {                          // the same in every thread: the barriers below are reached by all or none
      unsigned prefix = 0, mask = 0, k = (unsigned)c;
      for (int shift = 24; shift >= 0; shift -= 8) {
        hist[t] = 0;
        __syncthreads();
        for_each_sample(row, n_sample, vec, [&](int i, float v) {
          if (all_alive || alive[i]) {
            const unsigned key = key_of(v) ^ flip;
            if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
          }
        });
        __syncthreads();
        const unsigned h = hist[t];
        unsigned inc = h;                            // inclusive scan of the 256 bins: inside the wave, then across the 4 waves
        for (int off = 1; off < 64; off <<= 1) {
          const unsigned u = __shfl_up(inc, off);
          if (lane >= off) inc += u;
        }
        if (lane == 63) wave_sum[wave] = inc;
        __syncthreads();
        for (int w = 0; w < wave; ++w) inc += wave_sum[w];
        if (inc - h < k && k <= inc) {               // exactly one bin: the matching samples number at least k
          sel[0] = (unsigned)t;
          sel[1] = k - (inc - h);
        }
        __syncthreads();
        prefix |= sel[0] << shift;
        mask |= 0xffu << shift;
        k = sel[1];
      }
      T = value_of(prefix ^ flip);
    }
    if (t == 0) tally[0] = 0;
    __syncthreads();
    int left = 0, nans = 0;
    for_each_sample(row, n_sample, vec, [&](int i, float v) {
      nans += v != v;
      if (all_alive || alive[i]) {
        const bool out = leq ? v <= T : v >= T;
        left += out;
        alive[i] = out ? 0 : 1;
      }
    });
    for (int off = 32; off > 0; off >>= 1) {
      left += __shfl_xor(left, off);
      nans += __shfl_xor(nans, off);
    }
    if (lane == 0) {
      atomicAdd(&tally[0], left);
      atomicAdd(&tally[1], nans);
    }
    __syncthreads();
    left = tally[0];
    a -= left;
    if (t == 0) {
      thresholds[p * n_exit + e] = T;
      exit_counts[p * n_exit + e] = left;
    }
    __syncthreads();                                 // tally[0] is cleared again at the next exit
  }
  if (t == 0) {
    thresholds[p * n_exit + n_exit - 1] = -sentinel;
    exit_counts[p * n_exit + n_exit - 1] = a;
    status[p] = tally[1];
  }
}

}  // namespace

extern "C" int deer_solve_thresholds(const float* values, int n_stage, int n_sample, int ld, const int* out_n, int n_points, int n_exit, int leq,
                                     unsigned char* alive_scratch, float* thresholds, int* exit_counts, int* status, void* stream) {
  if (values == nullptr || out_n == nullptr || alive_scratch == nullptr || thresholds == nullptr || exit_counts == nullptr || status == nullptr ||
      n_exit < 1 || n_exit > 16 || n_exit > n_stage || n_sample < 1 || ld < n_sample || n_points < 1)
    return DEER_ERR_SHAPE;
  const int vec = (reinterpret_cast<uintptr_t>(values) % 16 == 0 && ld % 4 == 0) ? 1 : 0;
  hipLaunchKernelGGL(solve_thresholds_kernel, dim3((unsigned)n_points), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), values, n_sample,
                     (long)ld, out_n, n_exit, leq ? 1 : 0, alive_scratch, thresholds, exit_counts, status, vec);
  DEER_LAUNCH_CHECK();
  return DEER_OK;
}
