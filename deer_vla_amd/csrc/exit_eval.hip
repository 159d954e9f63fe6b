// Per-exit demonstration loss: the device pieces of the all-exits window forward (robot_flamingo/models/flamingo_mpt.py:463-517) and of
// the forward half of the multi-exit training step (robot_flamingo/train/train_utils.py:487-543) that csrc/head_seq.hip and
// csrc/calib.hip do not already have.
//
// Pooling (action_head.py:519-520) commutes with the per-(window, step) layer choice of the two sampling strategies (flamingo_mpt.py:
// 485-512), so the hidden states are pooled ONCE per (frame, layer) by deer_calib_pool_layers (csrc/calib.hip, any host list of layers - no
// twin here) and everything below works on pooled [d] rows:
//   window_gather_layers_kernel   X[s][(b, t)] = P[(b, t)][slot_of_layer[sel[s][b][t]]], all S selections in one launch
//   exit_loss_rows_kernel         per (head, row): Huber(delta = 1) mean over the 6 A pose values, BCE-with-logits mean over the A logits;
//                                 optionally their gradient (deer_head_grad_loss, the loss of exit-only fine-tuning: one head)
//   exit_loss_reduce_kernel       per head: mean over the rows of num + w_bin bin, one workgroup, fixed summation order
// No atomics, every sum has a fixed order (identical inputs give identical bits), every store is a vector-memory store.
#include "common.h"
#include "../../include/deer_hip.h"

namespace {

struct GatherSlots { int n; int slot[DEER_CALIB_MAX_LAYERS]; };

// One workgroup per (row r = (b, t), selection s, block of 1024 columns): 16-byte loads / stores, lanes along d.  A selected layer
// without a slot gives a NaN row (deer_calib_gather's contract): the actions of that window are NaN instead of another layer's.
__global__ __launch_bounds__(256) void window_gather_layers_kernel(const float* __restrict__ P, const int* __restrict__ sel, GatherSlots tab,
                                                                   float* __restrict__ X, long R, int NL, int d) {
  const long r = blockIdx.x;
  const int s = blockIdx.y;
  const int i = (blockIdx.z * 256 + threadIdx.x) * 4;
  if (i >= d) return;
  const int lay = sel[(long)s * R + r];
  const int slot = (lay >= 0 && lay < tab.n) ? tab.slot[lay] : -1;
  float4 v = float4{NAN, NAN, NAN, NAN};
  if (slot >= 0) v = *reinterpret_cast<const float4*>(P + (r * NL + slot) * d + i);
  *reinterpret_cast<float4*>(X + ((long)s * R + r) * d + i) = v;
}

// One thread per (head h, row r).  num: F.huber_loss(pose, label, reduction='none').mean(-1) (train_utils.py:520; torch's form
// |e| < 1 ? 0.5 e^2 : |e| - 0.5), bin: F.binary_cross_entropy_with_logits(logit, target, reduction='none').mean(-1) (:529) in the
// overflow-safe form max(x, 0) - x y + log1p(exp(-|x|)); both summed in index order.  dz (nullable; train_utils.py:519-543 backward):
// dz[i] = d (scale mean_rows(num + w_bin bin)) / d [pre-tanh pose 6A | gripper logit A], g_pose / g_bin the two scale factors; the last A
// slots of the 8 A wide row are zeroed.  torch's Huber backward: |e| < 1 ? e : sign(e).
__global__ __launch_bounds__(256) void exit_loss_rows_kernel(const float* __restrict__ actions, const float* __restrict__ pose,
                                                             const float* __restrict__ grip01, float* __restrict__ num, float* __restrict__ bin,
                                                             float* __restrict__ dz, int Hn, long R, int A, float g_pose, float g_bin) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)Hn * R) return;
  const long r = i % R;
  const float* a = actions + i * 8 * A;
  const float* p = pose + r * 6 * A;
  const float* g = grip01 + r * A;
  float* d = dz != nullptr ? dz + i * 8 * A : nullptr;
  float sn = 0.f;
  for (int k = 0; k < 6 * A; ++k) {
    const float df = a[k] - p[k];
    const float e = fabsf(df);
    sn += e < 1.f ? 0.5f * e * e : e - 0.5f;
    if (d != nullptr) d[k] = g_pose * (e < 1.f ? df : copysignf(1.f, df)) * (1.f - a[k] * a[k]);
  }
  float sb = 0.f;
  for (int k = 0; k < A; ++k) {
    const float x = a[7 * A + k];
    sb += (fmaxf(x, 0.f) - x * g[k]) + log1pf(expf(-fabsf(x)));
    if (d != nullptr) {
      d[6 * A + k] = g_bin * (a[6 * A + k] - g[k]);
      d[7 * A + k] = 0.f;
    }
  }
  num[i] = sn / (float)(6 * A);
  bin[i] = sb / (float)A;
}

// One workgroup per head: thread t sums rows t, t + 256, .. in that order, then a fixed tree over the 256 partial sums.
__global__ __launch_bounds__(256) void exit_loss_reduce_kernel(const float* __restrict__ num, const float* __restrict__ bin,
                                                               float* __restrict__ loss, long R, float w_bin) {
  __shared__ float part[256];
  const int h = blockIdx.x;
  float s = 0.f;
  for (long r = threadIdx.x; r < R; r += 256) s += num[h * R + r] + w_bin * bin[h * R + r];
  part[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[h] = part[0] / (float)R;
}

}  // namespace

extern "C" int deer_window_gather_layers(const float* P, const int* sel, const int* slot_of_layer, int n_layers, float* X, int S, int bs, int W,
                                         int NL, int d, void* stream) {
  if (P == nullptr || sel == nullptr || slot_of_layer == nullptr || X == nullptr || n_layers <= 0 || n_layers > DEER_CALIB_MAX_LAYERS || S <= 0 ||
      S > 65535 || bs <= 0 || W <= 0 || NL <= 0 || NL > DEER_CALIB_MAX_NL || d <= 0 || (d & 3) || (d + 1023) / 1024 > 65535)
    return DEER_ERR_SHAPE;
  GatherSlots tab{};
  tab.n = n_layers;
  for (int l = 0; l < n_layers; ++l) {
    if (slot_of_layer[l] >= NL) return DEER_ERR_SHAPE;
    tab.slot[l] = slot_of_layer[l];
  }
  const long R = (long)bs * W;
  if (R > 0x7fffffffL) return DEER_ERR_SHAPE;
  hipLaunchKernelGGL(window_gather_layers_kernel, dim3((unsigned)R, S, (d + 1023) / 1024), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), P,
                     sel, tab, X, R, NL, d);
  DEER_LAUNCH_CHECK();
  return DEER_OK;
}

extern "C" int deer_exit_losses(const float* actions, const float* pose, const float* grip01, int Hn, long R, int A, float w_bin, float* num,
                                float* bin, float* loss, void* stream) {
  if (actions == nullptr || pose == nullptr || grip01 == nullptr || num == nullptr || bin == nullptr || loss == nullptr || Hn <= 0 || Hn > 65535 ||
      R <= 0 || A <= 0 || A > 8 || (long)Hn * R > 0x7fffffffL / (8 * A))
    return DEER_ERR_SHAPE;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const long n = (long)Hn * R;
  hipLaunchKernelGGL(exit_loss_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, actions, pose, grip01, num, bin,
                     static_cast<float*>(nullptr), Hn, R, A, 0.f, 0.f);
  DEER_LAUNCH_CHECK();
  hipLaunchKernelGGL(exit_loss_reduce_kernel, dim3(Hn), dim3(256), 0, st, num, bin, loss, R, w_bin);
  DEER_LAUNCH_CHECK();
  return DEER_OK;
}

// deer_exit_losses for one head, plus dz = d (scale loss) / d (pre-tanh pose, gripper logit) of every row
extern "C" int deer_head_grad_loss(const float* actions, const float* pose, const float* grip01, long R, int A, float w_bin, float scale, float* dz,
                                   float* num, float* bin, float* loss, void* stream) {
  if (actions == nullptr || pose == nullptr || grip01 == nullptr || dz == nullptr || num == nullptr || bin == nullptr || loss == nullptr || R <= 0 ||
      A <= 0 || A > 8 || R > 0x7fffffffL / (8 * A))
    return DEER_ERR_SHAPE;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const float g_pose = scale / ((float)R * (float)(6 * A)), g_bin = scale * w_bin / ((float)R * (float)A);
  hipLaunchKernelGGL(exit_loss_rows_kernel, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, st, actions, pose, grip01, num, bin, dz, 1, R, A, g_pose,
                     g_bin);
  DEER_LAUNCH_CHECK();
  hipLaunchKernelGGL(exit_loss_reduce_kernel, dim3(1), dim3(256), 0, st, num, bin, loss, R, w_bin);
  DEER_LAUNCH_CHECK();
  return DEER_OK;
}
