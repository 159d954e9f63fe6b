// On-policy exit values: the deltas a SHADOW step left in the control blocks, appended to a device-resident value matrix.
//
// A shadow step (DEER_CTL_SHADOW) evaluates every exit, records its delta (ActionValueNet.forward(mode='infer'), robot_flamingo/models/
// value_net.py:120-133) in ctl[b][DEER_CTL_DELTAS + e], commits the LSTM state at the first exit whose criterion fires and never stops
// early: its history is the one a rollout has, its deltas are complete.  One append copies them, for the environments of active_mask,
// into the next free columns of values [n_exit][ld] - the (n_exit, n_sample) matrix deer_solve_thresholds reads - and the exit layer each
// environment took into taken[]: the sample of the "average exit layer" that bayesian_optimization.py:75-79 takes as its budget.
//   value_log_append_kernel   ONE workgroup of 256 threads = one thread per (environment, exit) of DEER_MAX_ENVS x 16.  Every thread reads
//                             the column count at entry; after the barrier thread 0 alone writes the three state words.  Successive appends
//                             are ordered by their stream, so no atomics; every store to device memory is a vector-memory store.
// The kernel runs after the step's verdict and does not consult ALL_EXITED.
#include "common.h"
#include "../../include/deer_hip.h"

namespace {

__global__ __launch_bounds__(256) void value_log_append_kernel(const int* __restrict__ ctl, int n_envs, int n_exit, unsigned active_mask,
                                                               unsigned* __restrict__ values, long ld, int capacity, int* __restrict__ taken,
                                                               int* __restrict__ state) {
  __shared__ int wave_nf[4];
  const int t = threadIdx.x, b = t >> 4, e = t & 15;
  const int count = state[0], dropped = state[1], nonfinite = state[2];
  const bool active = b < n_envs && ((active_mask >> b) & 1u);
  const int slot = count + __popc(active_mask & ((1u << b) - 1u));          // columns in ascending environment order
  const bool col = active && slot >= 0 && slot < capacity;
  bool nf = false;
  if (col && e < n_exit) {
    const unsigned u = (unsigned)ctl[b * DEER_CTL_WORDS + DEER_CTL_DELTAS + e];   // bit for bit: NaN payloads survive
    values[(long)e * ld + slot] = u;
    nf = (u & 0x7f800000u) == 0x7f800000u;
  }
  if (col && e == 0) taken[slot] = ctl[b * DEER_CTL_WORDS + DEER_CTL_EXIT_LAYER];
  const int n = __popcll(__ballot(nf));
  if ((t & 63) == 0) wave_nf[t >> 6] = n;
  __syncthreads();                                                         // every thread has read the state words
  if (t == 0) {
    const int n_active = __popc(active_mask);
    const int room = capacity - count;
    const int written = count < 0 ? 0 : (n_active < room ? n_active : (room > 0 ? room : 0));
    state[0] = count + written;
    state[1] = dropped + (n_active - written);
    state[2] = nonfinite + wave_nf[0] + wave_nf[1] + wave_nf[2] + wave_nf[3];
  }
}

}  // namespace

extern "C" int deer_value_log_append(const int* ctl, int n_envs, int n_exit, int active_mask, float* values, int ld, int capacity, int* taken,
                                     int* state, void* stream) {
  if (ctl == nullptr || values == nullptr || taken == nullptr || state == nullptr || n_envs < 1 || n_envs > DEER_MAX_ENVS || n_exit < 1 ||
      n_exit > 16 || capacity < 1 || ld < capacity || ((unsigned)active_mask >> n_envs) != 0u)
    return DEER_ERR_SHAPE;
  hipLaunchKernelGGL(value_log_append_kernel, dim3(1), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), ctl, n_envs, n_exit,
                     (unsigned)active_mask, reinterpret_cast<unsigned*>(values), (long)ld, capacity, taken, state);
  DEER_LAUNCH_CHECK();
  return DEER_OK;
}
