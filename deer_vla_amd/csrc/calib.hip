// Threshold calibration as one device pass: ActionValueNet.forward(mode='generate') (robot_flamingo/models/value_net.py:134-160) on a
// batch of calibration windows, the head side of generate_action_values (value_net.py:301-397).
//
// For seq_id in [W/2 - 1, W - 1) and every layer i of [0] + exit_list the reference runs the LSTM from zero over
// [features of the random exit layers at steps 0 .. seq_id - 1 ; layer i's feature at seq_id] and keeps the last action.  That factors:
//   history     ONE sequence per window over the random-layer features of steps 0 .. W - 2, (h, c) of every step kept
//   candidates  for every (window, seq_id, layer) ONE LSTM step from the history state after step seq_id - 1 (zero state: seq_id = 0)
//   deltas      of consecutive candidate layers (get_delta, value_net.py:105-117)
// and is layer-major like csrc/head_seq.hip: at LSTM layer l a candidate row needs the history state (l, window, seq_id - 1) and its own
// output of layer l - 1, so history rows and candidate rows share one W_ih projection GEMM per layer, and all candidate rows of a layer
// are one recurrent launch.  The GEMMs, LayerNorms and recurrent steps (deer_calib_lstm_step: the previous state read-only and per row
// through an index) are head_seq.hip's kernels on more rows; this file holds
//   calib_pool_layers_kernel   hidden[layer][row][d] of an env-batch engine -> P[frame][k][d], k over [0] + exit ids, pooled over the T
//                              rows of a frame (AdaptiveMax/AvgPool1d, action_head.py:519-520; all T rows: no key mask reaches the head)
//   calib_gather_kernel        P -> the history rows (the random layer's slot per (window, step)) and the candidate rows, + the
//                              candidate row -> history row index
//   calib_delta_kernel         actions [NL][rows][8 A] -> values [n_exit][rows]
// No atomics, fixed summation order, every store a vector-memory store.
#include "common.h"
#include "../../include/deer_hip.h"

namespace {

struct CalibLayers { int id[DEER_CALIB_MAX_NL]; };
struct CalibSlots { int n; int slot[DEER_CALIB_MAX_LAYERS]; };

// One workgroup per (frame, layer slot, block of 1024 columns): 16-byte loads, lanes along d (coalesced), T rows in order.
__global__ __launch_bounds__(256) void calib_pool_layers_kernel(const float* __restrict__ hidden, long layer_stride, CalibLayers lay,
                                                                float* __restrict__ P, int T, int d, int avg) {
  const int frame = blockIdx.x, k = blockIdx.y, NL = gridDim.y;
  const int i = (blockIdx.z * 256 + threadIdx.x) * 4;
  if (i >= d) return;
  const float* x = hidden + (long)lay.id[k] * layer_stride + (long)frame * T * d + i;
  float4 a = avg ? float4{0.f, 0.f, 0.f, 0.f} : float4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
  for (int t = 0; t < T; ++t) {
    const float4 v = *reinterpret_cast<const float4*>(x + (long)t * d);
    if (avg) { a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w; }
    else { a.x = fmaxf(a.x, v.x); a.y = fmaxf(a.y, v.y); a.z = fmaxf(a.z, v.z); a.w = fmaxf(a.w, v.w); }
  }
  if (avg) { a.x /= (float)T; a.y /= (float)T; a.z /= (float)T; a.w /= (float)T; }
  *reinterpret_cast<float4*>(P + ((long)frame * NL + k) * d + i) = a;
}

// Rows of one chunk of bc windows: r < bc (W - 1): history row (b, t) = P[b][t][slot(rand_layers[b][t])]; then the candidate rows in
// (k, b, s) order = P[b][W/2 - 1 + s][k], with idx[(k, b, s)] = history row (b, W/2 - 2 + s) or -1 (zero state).  A random layer without a
// slot (not layer 0 / an exit) gives a NaN row: the values of that window are NaN instead of silently another layer's.
__global__ __launch_bounds__(256) void calib_gather_kernel(const float* __restrict__ P, const int* __restrict__ rand_layers, CalibSlots tab,
                                                           float* __restrict__ X, int* __restrict__ idx, int bc, int W, int NL, int d) {
  const long r = blockIdx.x;
  const int i = (blockIdx.y * 256 + threadIdx.x) * 4;
  const long Rh = (long)bc * (W - 1);
  const int S = W - W / 2;
  long b, t;
  int slot;
  if (r < Rh) {
    b = r / (W - 1);
    t = r % (W - 1);
    const int lay = rand_layers[b * W + t];
    slot = (lay >= 0 && lay < tab.n) ? tab.slot[lay] : -1;
  } else {
    const long q = r - Rh;
    slot = (int)(q / ((long)bc * S));
    b = (q / S) % bc;
    t = W / 2 - 1 + q % S;
    if (blockIdx.y == 0 && threadIdx.x == 0) idx[q] = t > 0 ? (int)(b * (W - 1) + t - 1) : -1;
  }
  if (i >= d) return;
  float4 v = float4{NAN, NAN, NAN, NAN};
  if (slot >= 0) v = *reinterpret_cast<const float4*>(P + ((b * W + t) * NL + slot) * d + i);
  *reinterpret_cast<float4*>(X + r * d + i) = v;
}

// get_delta (value_net.py:105-117) of consecutive candidate layers: values[e][r] = delta(actions[e][r], actions[e + 1][r]) over the NP
// pose values, summed in index order.  max propagates a NaN like torch's (the form of head_final, csrc/head.hip); cosine = 1 - cos with
// each norm clamped at eps = 1e-5 (torch.nn.functional.cosine_similarity).
__global__ __launch_bounds__(256) void calib_delta_kernel(const float* __restrict__ act, long ld_act, float* __restrict__ values, long ld_val,
                                                          int n_exit, int rows, int NP, int thr_type) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)n_exit * rows) return;
  const long e = i / rows, r = i % rows;
  const float* a = act + (e * rows + r) * ld_act;
  const float* b = act + ((e + 1) * rows + r) * ld_act;
  float delta;
  if (thr_type == 3) {
    float na = 0.f, nb = 0.f, ab = 0.f;
    for (int k = 0; k < NP; ++k) { na += a[k] * a[k]; nb += b[k] * b[k]; }
    na = fmaxf(sqrtf(na), 1e-5f); nb = fmaxf(sqrtf(nb), 1e-5f);
    for (int k = 0; k < NP; ++k) ab += (a[k] / na) * (b[k] / nb);
    delta = 1.f - ab;
  } else {
    float acc = 0.f;
    for (int k = 0; k < NP; ++k) {
      const float dd = fabsf(a[k] - b[k]);
      if (thr_type == 0) acc += dd * dd;
      else if (thr_type == 1) acc += dd;
      else acc = (dd > acc || dd != dd) ? dd : acc;
    }
    delta = thr_type == 0 ? sqrtf(acc / NP) : (thr_type == 1 ? acc / NP : acc);
  }
  values[e * ld_val + r] = delta;
}

}  // namespace

extern "C" int deer_calib_pool_layers(const float* hidden, long layer_stride, const int* layers, int NL, float* P, int n_frames, int T, int d,
                                      int avg, void* stream) {
  if (hidden == nullptr || layers == nullptr || P == nullptr || NL <= 0 || NL > DEER_CALIB_MAX_NL || n_frames <= 0 || T <= 0 || d <= 0 ||
      (d & 3) || layer_stride < (long)n_frames * T * d || (d + 1023) / 1024 > 65535)
    return DEER_ERR_SHAPE;
  CalibLayers lay{};
  for (int k = 0; k < NL; ++k) {
    if (layers[k] < 0) return DEER_ERR_SHAPE;
    lay.id[k] = layers[k];
  }
  hipLaunchKernelGGL(calib_pool_layers_kernel, dim3(n_frames, NL, (d + 1023) / 1024), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), hidden,
                     layer_stride, lay, P, T, d, avg);
  DEER_LAUNCH_CHECK();
  return DEER_OK;
}

extern "C" int deer_calib_gather(const float* P, const int* rand_layers, const int* slot_of_layer, int n_layers, float* X, int* idx, int bc,
                                 int W, int NL, int d, void* stream) {
  if (P == nullptr || rand_layers == nullptr || slot_of_layer == nullptr || X == nullptr || idx == nullptr || n_layers <= 0 ||
      n_layers > DEER_CALIB_MAX_LAYERS || bc <= 0 || W < 2 || NL < 2 || NL > DEER_CALIB_MAX_NL || d <= 0 || (d & 3) || (d + 1023) / 1024 > 65535)
    return DEER_ERR_SHAPE;
  CalibSlots tab{};
  tab.n = n_layers;
  for (int l = 0; l < n_layers; ++l) {
    if (slot_of_layer[l] >= NL) return DEER_ERR_SHAPE;
    tab.slot[l] = slot_of_layer[l];
  }
  const long R = (long)bc * (W - 1) + (long)NL * bc * (W - W / 2);
  if (R > 0x7fffffffL) return DEER_ERR_SHAPE;
  hipLaunchKernelGGL(calib_gather_kernel, dim3((unsigned)R, (d + 1023) / 1024), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), P, rand_layers,
                     tab, X, idx, bc, W, NL, d);
  DEER_LAUNCH_CHECK();
  return DEER_OK;
}

extern "C" int deer_calib_delta(const float* actions, long ld_act, int NL, int rows, int NP, int thr_type, float* values, long ld_val, void* stream) {
  if (actions == nullptr || values == nullptr || NL < 2 || rows <= 0 || NP <= 0 || ld_act < NP || ld_val < rows || thr_type < 0 || thr_type > 3)
    return DEER_ERR_SHAPE;
  const long n = (long)(NL - 1) * rows;
  hipLaunchKernelGGL(calib_delta_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), actions, ld_act,
                     values, ld_val, NL - 1, rows, NP, thr_type);
  DEER_LAUNCH_CHECK();
  return DEER_OK;
}
