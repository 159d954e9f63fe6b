// Window-mode (sequence) evaluation of the action head: DeterministicDecoder.forward on N sequences of L time steps
// (robot_flamingo/models/action_head.py:499-611, the `input_feature.shape[1] > 1` branch :588-595).
//
// The step kernels of csrc/head.hip evaluate ONE time step of up to 16 environments per launch and stream every weight once per
// step.  Here the schedule is layer-major (the cuDNN form of a stacked LSTM):
//   pool      every (sequence, step) row max / mean-pooled over its T feature rows (+ the robot-state embedding, use_state)
//   project   X_l W_ih,l^T + b_ih,l for ALL N L rows of a layer as one MFMA GEMM - W_ih,l is read once per call, not L times
//   recur     per time step: pre[:, t] + h_{t-1} W_hh,l^T + b_hh,l -> gates -> c, h, one launch over all N rows
//   MLP       the hidden Linears (+ LayerNorm) + ReLU and the output Linears (tanh / sigmoid) as GEMMs over all rows
// Operand arithmetic (the step head's): weights bf16 / fp16 (product arithmetic) or f32 (precision = 1); activations f32.  A 16-bit
// weight meets its f32 activation as two MFMAs on the activation's hi + lo planes (common.h split2, with the fp16 saturation of
// |v| > 65504; fp16 outliers of the GEMM inputs go through a 2^-16-scaled second accumulator, seq_frag_mac_wide), so the products keep
// ~16 (bf16) / ~22 (fp16) significand bits of the activation; f32 weights use the exact-f32 MFMA
// (v_mfma_f32_16x16x4_f32, as csrc/precise.hip).  No atomics: every sum has a fixed order, identical inputs give identical bits.
// Every store is a vector-memory store; reads past a matrix edge are clamped to its last row / column and never stored.
// The recurrent step and the LayerNorm serve three chains through nullable arguments: the sequence head (deer_head_seq_lstm_step,
// deer_head_seq_ln), threshold calibration (deer_calib_lstm_step: previous state read-only and per row through an index) and the taped
// forward of exit-only fine-tuning (deer_head_grad_lstm_step: activated gates kept; deer_head_grad_ln: (mean, rstd) kept).
#include "common.h"
#include "../../include/deer_hip.h"

namespace {

// weight formats of the head (deer_model.wkind): 0 bf16, 1 f32, 2 fp16
enum { SEQ_W_BF16 = 0, SEQ_W_F32 = 1, SEQ_W_F16 = 2 };

// acc += W[n0 + c][k .. k+7] . X[m][k .. k+7] for one 16 x 16 tile, k = k0 + 8 g (lane = 16 g + c).  W fragment = MFMA "A" operand,
// activation = "B": the lane ends with acc[r] = sum over k of W[n0 + 4 g + r] X[m0 + c].  kval: this lane's k slice lies inside K.
template <int WK>
__device__ __forceinline__ void seq_frag_mac(const void* __restrict__ wrow, const float* __restrict__ xrow, bool kval, f32x4& acc) {
  float4 x0 = float4{0.f, 0.f, 0.f, 0.f}, x1 = x0;
  if (kval) {
    x0 = *reinterpret_cast<const float4*>(xrow);
    x1 = *reinterpret_cast<const float4*>(xrow + 4);
  }
  if constexpr (WK == SEQ_W_F32) {
    float4 w0 = float4{0.f, 0.f, 0.f, 0.f}, w1 = w0;
    if (kval) {
      w0 = *reinterpret_cast<const float4*>(wrow);
      w1 = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(wrow) + 4);
    }
    // the eight k of the lane's slice go through eight 16x16x4 steps (both operands use the same k permutation)
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w0.x, x0.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w0.y, x0.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w0.z, x0.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w0.w, x0.w, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w1.x, x1.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w1.y, x1.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w1.z, x1.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w1.w, x1.w, acc, 0, 0, 0);
  } else {
    constexpr bool F16 = WK == SEQ_W_F16;
    uint4 w = uint4{0u, 0u, 0u, 0u};
    if (kval) w = *reinterpret_cast<const uint4*>(wrow);
    uint32_t h[4], l[4];
    split2<F16>(x0.x, x0.y, h[0], l[0]);
    split2<F16>(x0.z, x0.w, h[1], l[1]);
    split2<F16>(x1.x, x1.y, h[2], l[2]);
    split2<F16>(x1.z, x1.w, h[3], l[3]);
    const bf16x8 wf = __builtin_bit_cast(bf16x8, w);
    acc = mfma16<F16>(wf, __builtin_bit_cast(bf16x8, uint4{h[0], h[1], h[2], h[3]}), acc);
    acc = mfma16<F16>(wf, __builtin_bit_cast(bf16x8, uint4{l[0], l[1], l[2], l[3]}), acc);
  }
}

// seq_frag_mac for an activation side that may hold fp16 outliers (the pooled features; the LSTM's recurrent input is |h| < 1): an
// |x| > 65504 has no fp16 hi + lo pair (split2 saturates hi and lo overflows), so when any lane of the wave meets one, the k-step splits
// its values into x_s (the ordinary ones) into `acc` and x_b = x / 2^16 (the outliers) into `accb`; the caller adds 2^16 accb.  The
// f32 product of the step head is kept up to |x| ~ 4e9; a k-step without outliers runs the ordinary pair of MFMAs (accb stays 0).
template <int WK>
__device__ __forceinline__ void seq_frag_mac_wide(const void* __restrict__ wrow, const float* __restrict__ xrow, bool kval, f32x4& acc, f32x4& accb) {
  if constexpr (WK == SEQ_W_F16) {
    float x[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (kval) {
      const float4 x0 = *reinterpret_cast<const float4*>(xrow), x1 = *reinterpret_cast<const float4*>(xrow + 4);
      x[0] = x0.x; x[1] = x0.y; x[2] = x0.z; x[3] = x0.w; x[4] = x1.x; x[5] = x1.y; x[6] = x1.z; x[7] = x1.w;
    }
    bool big = false;
#pragma unroll
    for (int e = 0; e < 8; ++e) big |= fabsf(x[e]) > 65504.f;
    if (__any(big)) {                                        // wave-uniform
      uint4 w = uint4{0u, 0u, 0u, 0u};
      if (kval) w = *reinterpret_cast<const uint4*>(wrow);
      const bf16x8 wf = __builtin_bit_cast(bf16x8, w);
      float xs[8], xb[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const bool o = fabsf(x[e]) > 65504.f;
        xs[e] = o ? 0.f : x[e];
        xb[e] = o ? x[e] * (1.f / 65536.f) : 0.f;
      }
      uint32_t h[4], l[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) split2<true>(xs[2 * e], xs[2 * e + 1], h[e], l[e]);
      acc = mfma16<true>(wf, __builtin_bit_cast(bf16x8, uint4{h[0], h[1], h[2], h[3]}), acc);
      acc = mfma16<true>(wf, __builtin_bit_cast(bf16x8, uint4{l[0], l[1], l[2], l[3]}), acc);
#pragma unroll
      for (int e = 0; e < 4; ++e) split2<true>(xb[2 * e], xb[2 * e + 1], h[e], l[e]);
      accb = mfma16<true>(wf, __builtin_bit_cast(bf16x8, uint4{h[0], h[1], h[2], h[3]}), accb);
      accb = mfma16<true>(wf, __builtin_bit_cast(bf16x8, uint4{l[0], l[1], l[2], l[3]}), accb);
      return;
    }
  }
  seq_frag_mac<WK>(wrow, xrow, kval, acc);
}

template <int WK> __device__ __forceinline__ const void* seq_wrow(const void* W, long row, int K, int k) {
  if constexpr (WK == SEQ_W_F32) return reinterpret_cast<const float*>(W) + row * K + k;
  else return reinterpret_cast<const bf16_t*>(W) + row * K + k;
}

// ---- pool: X[r] = max / mean over t < T of feats[r][t] (+ emb[r]) ---------------------------------------------------------------
__global__ __launch_bounds__(256) void seq_pool_kernel(const float* __restrict__ feats, const float* __restrict__ emb, float* __restrict__ X,
                                                       int T, int d, int avg) {
  const long r = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= d) return;
  const float* x = feats + r * T * d + i;
  float a = avg ? 0.f : -INFINITY;
  for (int t = 0; t < T; ++t) {
    const float v = x[(long)t * d];
    a = avg ? a + v : fmaxf(a, v);
  }
  if (avg) a /= (float)T;
  if (emb != nullptr) a += emb[r * d + i];
  X[r * d + i] = a;
}

// ---- robot state -> u = [relu(W_arm arm + b_arm) ; relu(E_grip[(g + 1) / 2 truncated])] (2 d per row; action_head.py:526-532) ------
__global__ __launch_bounds__(256) void seq_state_u_kernel(const float* __restrict__ state, const float* __restrict__ w_arm,
                                                          const float* __restrict__ b_arm, const float* __restrict__ e_grip,
                                                          float* __restrict__ u, int d) {
  const long r = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= d) return;
  const float* st = state + r * 8;
  const int gi = min(1, max(0, (int)((st[6] + 1.0f) * 0.5f)));
  float a = b_arm[i];
#pragma unroll
  for (int k = 0; k < 6; ++k) a += w_arm[i * 6 + k] * st[k];
  u[r * 2 * d + i] = fmaxf(a, 0.f);
  u[r * 2 * d + d + i] = fmaxf(e_grip[(long)gi * d + i], 0.f);
}

// ---- GEMM: out[m][n] = epi(X[m] . W[n] + bias[n]) for m < M, n < N ---------------------------------------------------------------
// Workgroup = 4 waves = 64 weight rows x 64 activation rows; wave w owns weight rows n0 + 16 w .. +15 and the four 16-row tiles.
// DEER_SEQ_EPI_SIGMOID_LOGIT: out[m][n] = sigmoid(v), out[m][N + n] = v (the gripper head's probability and logit, action_head.py:128-134).
template <int WK>
__global__ __launch_bounds__(256) void seq_gemm_kernel(const float* __restrict__ X, long ldx, const void* __restrict__ W,
                                                       const float* __restrict__ bias, float* __restrict__ out, long ldo, int M, int N,
                                                       int K, int epi) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * 64 + wave * 16, m0 = blockIdx.y * 64;
  if (n0 >= N) return;                                      // wave-uniform
  const long wr = min(n0 + c, N - 1);
  long xr[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) xr[j] = min(m0 + j * 16 + c, M - 1);
  f32x4 acc[4], accb[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = accb[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
  for (int k0 = 0; k0 < K; k0 += 32) {
    const int k = k0 + g * 8;
    const bool kval = k < K;
    const int kc = kval ? k : 0;
    const void* wp = seq_wrow<WK>(W, wr, K, kc);
#pragma unroll
    for (int j = 0; j < 4; ++j) seq_frag_mac_wide<WK>(wp, X + xr[j] * ldx + kc, kval, acc[j], accb[j]);
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int m = m0 + j * 16 + c;
    if (m >= M) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int n = n0 + g * 4 + r;
      if (n >= N) continue;
      float v = acc[j][r];
      if constexpr (WK == SEQ_W_F16) v += 65536.f * accb[j][r];
      v += bias != nullptr ? bias[n] : 0.f;
      float* o = out + (long)m * ldo + n;
      if (epi == DEER_SEQ_EPI_RELU) v = fmaxf(v, 0.f);
      else if (epi == DEER_SEQ_EPI_TANH) v = tanhf(v);
      else if (epi == DEER_SEQ_EPI_SIGMOID_LOGIT) {
        o[N] = v;
        v = sigmoidf_(v);
      }
      *o = v;
    }
  }
}

// ---- one LSTM time step of one layer over N rows (torch.nn.LSTM gate order i, f, g, o) ------------------------------------------
// gates = pre[m] + h_prev[p] W_hh^T + b_hh; c' = s(f) c_prev[p] + s(i) tanh(g); h' = s(o) tanh(c').  Row m continues from row p = idx[m]
// (idx NULL: p = m) of h_prev / c_prev; p < 0 is the zero state (zero_row: H zeros, the h operand of such a row); h_prev NULL: no
// recurrent term at all, c_prev NULL: c = 0.  Workgroup = 16 hidden units x SEQ_RT rows; its four waves split K = H (k-steps w, w + 4,
// ...), the partial tiles of the four gates meet in LDS and are summed in wave order: a row's result does not depend on which other rows
// share the launch.  Outputs: h_out row m at h_out + m * ld_out; optional c_out (pitch ld_co), dense h_n / c_n [N][H] and gates_out
// (pitch ld_g): the activated gates s(i), s(f), tanh(g), s(o).  c_out may be c_prev (idx NULL) and gates_out may be pre: every element
// is then read and written by the same thread, so those four pointers carry no __restrict__.  IDX / TAPE: idx / gates_out are in use
// (compile-time, so the sequence head's form pays for neither).  A thread owns 16 SEQ_RT / 256 (unit, row) elements: it loads the inputs
// of all of them before it stores any, so the loads of the second do not wait behind the stores of the first.
template <int WK, bool IDX, bool TAPE>
__global__ __launch_bounds__(256) void seq_lstm_step_kernel(const float* pre, long ld_pre, const float* __restrict__ h_prev, long ld_h,
                                                            const float* c_prev, long ld_c, const int* __restrict__ idx,
                                                            const float* __restrict__ zero_row, const void* __restrict__ w_hh,
                                                            const float* __restrict__ b_hh, float* c_out, long ld_co,
                                                            float* __restrict__ h_out, long ld_out, float* __restrict__ h_n,
                                                            float* __restrict__ c_n, float* gates_out, long ld_g, int N, int H) {
  __shared__ float part[4][4][SEQ_RT / 16][64][4];             // [wave][gate][row tile][lane][r]: 32 KB
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = lane & 15, g = lane >> 4;
  const int u0 = blockIdx.x * 16, m0 = blockIdx.y * SEQ_RT;
  f32x4 acc[4][SEQ_RT / 16];
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int j = 0; j < SEQ_RT / 16; ++j) acc[q][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (h_prev != nullptr) {
    const float* xp[SEQ_RT / 16];
#pragma unroll
    for (int j = 0; j < SEQ_RT / 16; ++j) {
      const int m = min(m0 + j * 16 + c, N - 1);
      const long p = IDX ? idx[m] : m;
      xp[j] = p < 0 ? zero_row : h_prev + p * ld_h;
    }
#pragma unroll 2
    for (int k0 = wave * 32; k0 < H; k0 += 128) {
      const int k = k0 + g * 8;
      const bool kval = k < H;
      const int kc = kval ? k : 0;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const void* wp = seq_wrow<WK>(w_hh, (long)q * H + u0 + c, H, kc);
#pragma unroll
        for (int j = 0; j < SEQ_RT / 16; ++j) seq_frag_mac<WK>(wp, xp[j] + kc, kval, acc[q][j]);
      }
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int j = 0; j < SEQ_RT / 16; ++j)
      *reinterpret_cast<float4*>(&part[wave][q][j][lane][0]) = float4{acc[q][j][0], acc[q][j][1], acc[q][j][2], acc[q][j][3]};
  __syncthreads();
  constexpr int EP = 16 * SEQ_RT / 256;
  float gq[EP][4], cp[EP];
#pragma unroll
  for (int e = 0; e < EP; ++e) {
    const int p = threadIdx.x + e * 256;
    const int ul = p & 15, rl = p >> 4;
    const int m = m0 + rl, u = u0 + ul;
    if (m >= N) continue;
    const int j = rl >> 4, pl = ((ul >> 2) << 4) | (rl & 15), r = ul & 3;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float s = ((part[0][q][j][pl][r] + part[1][q][j][pl][r]) + part[2][q][j][pl][r]) + part[3][q][j][pl][r];
      gq[e][q] = (pre[(long)m * ld_pre + q * H + u] + s) + b_hh[q * H + u];
    }
    const long pr = IDX ? idx[m] : m;
    cp[e] = (c_prev != nullptr && pr >= 0) ? c_prev[pr * ld_c + u] : 0.f;
  }
#pragma unroll
  for (int e = 0; e < EP; ++e) {
    const int p = threadIdx.x + e * 256;
    const int m = m0 + (p >> 4), u = u0 + (p & 15);
    if (m >= N) continue;
    const float gi = sigmoidf_(gq[e][0]), gf = sigmoidf_(gq[e][1]), gg = tanhf(gq[e][2]), go = sigmoidf_(gq[e][3]);
    const float c2 = gf * cp[e] + gi * gg;
    const float h2 = go * tanhf(c2);
    if constexpr (TAPE) {
      float* go_row = gates_out + (long)m * ld_g;
      go_row[u] = gi;
      go_row[H + u] = gf;
      go_row[2 * H + u] = gg;
      go_row[3 * H + u] = go;
    }
    if (c_out != nullptr) c_out[(long)m * ld_co + u] = c2;
    h_out[(long)m * ld_out + u] = h2;
    if (h_n != nullptr) {
      h_n[(long)m * H + u] = h2;
      c_n[(long)m * H + u] = c2;
    }
  }
}

// ---- LayerNorm of rows (one wave per row), optional ReLU: dst[m] = LN(src[m]); stats (nullable): stats[m] = (mean, rstd) ----------
__global__ __launch_bounds__(256) void seq_ln_kernel(const float* src, long ld_src, float* dst, long ld_dst,
                                                     const float* __restrict__ w, const float* __restrict__ b, float* __restrict__ stats,
                                                     int M, int n, float eps, int relu) {
  const int lane = threadIdx.x & 63;
  const long m = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m >= M) return;
  const float* s = src + m * ld_src;
  float sum = 0.f;
  for (int i = lane; i < n; i += 64) sum += s[i];
  const float mean = wave_sum(sum) / n;
  float var = 0.f;
  for (int i = lane; i < n; i += 64) {
    const float dv = s[i] - mean;
    var += dv * dv;
  }
  const float rstd = rsqrtf(wave_sum(var) / n + eps);
  if (stats != nullptr && lane == 0) {
    stats[2 * m] = mean;
    stats[2 * m + 1] = rstd;
  }
  for (int i = lane; i < n; i += 64) {
    const float y = (s[i] - mean) * rstd * w[i] + b[i];
    dst[m * ld_dst + i] = relu ? fmaxf(y, 0.f) : y;
  }
}

// The one launch of seq_lstm_step_kernel: the three exported forms below are their own argument checks plus this call.
static int seq_lstm_step_launch(const float* pre, long ld_pre, const float* h_prev, long ld_h, const float* c_prev, long ld_c, const int* idx,
                                const float* zero_row, const void* w_hh, int w_kind, const float* b_hh, float* c_out, long ld_co, float* h_out,
                                long ld_out, float* h_n, float* c_n, float* gates_out, long ld_g, int N, int H, void* stream) {
  // in-place c is legal only where every thread reads the element it writes: not through an index.  Exact equality is what is tested;
  // a c_out that merely overlaps c_prev is the caller's error.
  // The tape exists on f32 rows without an index only.
  const bool tape = gates_out != nullptr;
  if (w_kind < 0 || w_kind > 2 || (N + SEQ_RT - 1) / SEQ_RT > 65535 || (idx != nullptr && c_out != nullptr && c_out == c_prev) ||
      (tape && (w_kind != SEQ_W_F32 || idx != nullptr)))
    return DEER_ERR_SHAPE;
  dim3 grid(H / 16, (N + SEQ_RT - 1) / SEQ_RT);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
#define SEQ_STEP_LAUNCH(WK, IDX, TAPE)                                                                                                       \
  hipLaunchKernelGGL((seq_lstm_step_kernel<WK, IDX, TAPE>), grid, dim3(256), 0, st, pre, ld_pre, h_prev, ld_h, c_prev, ld_c, idx, zero_row, w_hh, b_hh, c_out, \
                     ld_co, h_out, ld_out, h_n, c_n, gates_out, ld_g, N, H)
#define SEQ_STEP_IDX(WK)                      \
  do {                                        \
    if (idx != nullptr) SEQ_STEP_LAUNCH(WK, true, false); \
    else SEQ_STEP_LAUNCH(WK, false, false);   \
  } while (0)
  if (tape) SEQ_STEP_LAUNCH(SEQ_W_F32, false, true);
  else if (w_kind == SEQ_W_F32) SEQ_STEP_IDX(SEQ_W_F32);
  else if (w_kind == SEQ_W_F16) SEQ_STEP_IDX(SEQ_W_F16);
  else SEQ_STEP_IDX(SEQ_W_BF16);
#undef SEQ_STEP_IDX
#undef SEQ_STEP_LAUNCH
  DEER_LAUNCH_CHECK();
  return DEER_OK;
}

}  // namespace

extern "C" int deer_head_seq_pool(const float* feats, const float* emb, float* X, int M, int T, int d, int avg, void* stream) {
  if (feats == nullptr || X == nullptr || M <= 0 || M > 65535 || T <= 0 || d <= 0) return DEER_ERR_SHAPE;
  hipLaunchKernelGGL(seq_pool_kernel, dim3((d + 255) / 256, M), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), feats, emb, X, T, d, avg);
  DEER_LAUNCH_CHECK();
  return DEER_OK;
}

extern "C" int deer_head_seq_state_u(const float* state, const float* w_arm, const float* b_arm, const float* e_grip, float* u, int M, int d,
                                     void* stream) {
  if (state == nullptr || u == nullptr || M <= 0 || M > 65535 || d <= 0) return DEER_ERR_SHAPE;
  hipLaunchKernelGGL(seq_state_u_kernel, dim3((d + 255) / 256, M), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), state, w_arm, b_arm,
                     e_grip, u, d);
  DEER_LAUNCH_CHECK();
  return DEER_OK;
}

extern "C" int deer_head_seq_gemm(const float* X, long ldx, const void* W, int w_kind, const float* bias, float* out, long ldo, int M, int N,
                                  int K, int epi, void* stream) {
  // 16-byte activation / weight slices: K, ldx % 8 == 0 (rows of 16-bit weights: 16 bytes per lane and k-step)
  if (X == nullptr || W == nullptr || out == nullptr || M <= 0 || N <= 0 || K <= 0 || (K & 7) || (ldx & 7) || ldx < K || ldo < N ||
      (epi == DEER_SEQ_EPI_SIGMOID_LOGIT && ldo < 2 * N) || epi < 0 || epi > 3 || w_kind < 0 || w_kind > 2 || (M + 63) / 64 > 65535)
    return DEER_ERR_SHAPE;
  dim3 grid((N + 63) / 64, (M + 63) / 64);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (w_kind == SEQ_W_F32) hipLaunchKernelGGL(seq_gemm_kernel<SEQ_W_F32>, grid, dim3(256), 0, st, X, ldx, W, bias, out, ldo, M, N, K, epi);
  else if (w_kind == SEQ_W_F16) hipLaunchKernelGGL(seq_gemm_kernel<SEQ_W_F16>, grid, dim3(256), 0, st, X, ldx, W, bias, out, ldo, M, N, K, epi);
  else hipLaunchKernelGGL(seq_gemm_kernel<SEQ_W_BF16>, grid, dim3(256), 0, st, X, ldx, W, bias, out, ldo, M, N, K, epi);
  DEER_LAUNCH_CHECK();
  return DEER_OK;
}

// c_state [N][H] is read and written in place (each element by one thread).  Unlike the two forms below this one does not ask for
// ld_h >= H: the rule is inherited as it was, and the refusal tests pin it.
extern "C" int deer_head_seq_lstm_step(const float* pre, long ld_pre, const float* h_prev, long ld_h, const void* w_hh, int w_kind,
                                       const float* b_hh, float* c_state, float* h_out, long ld_out, float* h_n, float* c_n, int N, int H,
                                       void* stream) {
  if (pre == nullptr || w_hh == nullptr || b_hh == nullptr || c_state == nullptr || h_out == nullptr || N <= 0 || H <= 0 || (H & 15) ||
      (h_prev != nullptr && (ld_h & 7)) || ld_pre < 4L * H || ld_out < H || (h_n == nullptr) != (c_n == nullptr))
    return DEER_ERR_SHAPE;
  return seq_lstm_step_launch(pre, ld_pre, h_prev, ld_h, c_state, H, nullptr, nullptr, w_hh, w_kind, b_hh, c_state, H, h_out, ld_out, h_n, c_n,
                              nullptr, 0, N, H, stream);
}

// the previous state read-only and per row through an index (csrc/calib.hip: history and candidate rows)
extern "C" int deer_calib_lstm_step(const float* pre, long ld_pre, const float* h_prev, long ld_h, const float* c_prev, long ld_c, const int* idx,
                                    const float* zero_row, const void* w_hh, int w_kind, const float* b_hh, float* c_out, long ld_co,
                                    float* h_out, long ld_out, int N, int H, void* stream) {
  if (pre == nullptr || w_hh == nullptr || b_hh == nullptr || h_out == nullptr || N <= 0 || H <= 0 || (H & 15) ||
      (h_prev != nullptr && ((ld_h & 7) || ld_h < H)) || (c_prev != nullptr && (h_prev == nullptr || ld_c < H)) ||
      (idx != nullptr && h_prev != nullptr && zero_row == nullptr) || ld_pre < 4L * H || ld_out < H || (c_out != nullptr && ld_co < H))
    return DEER_ERR_SHAPE;
  return seq_lstm_step_launch(pre, ld_pre, h_prev, ld_h, c_prev, ld_c, idx, zero_row, w_hh, w_kind, b_hh, c_out, ld_co, h_out, ld_out, nullptr,
                              nullptr, nullptr, 0, N, H, stream);
}

// the taped step of csrc/head_grad.hip on f32 weight rows: gates [m][4H] holds pre = x W_ih^T + b_ih on entry and the ACTIVATED gates on
// return; c_prev / h_prev NULL at t = 0 (zero state); c_out, h_out: this step's c_t and raw h_t
extern "C" int deer_head_grad_lstm_step(float* gates, long ld_g, const float* h_prev, long ld_h, const float* w_hh, const float* b_hh,
                                        const float* c_prev, float* c_out, long ld_c, float* h_out, long ld_out, int N, int H, void* stream) {
  if (gates == nullptr || w_hh == nullptr || b_hh == nullptr || c_out == nullptr || h_out == nullptr || N <= 0 || H <= 0 || (H & 15) ||
      (h_prev == nullptr) != (c_prev == nullptr) || (h_prev != nullptr && ((ld_h & 7) || ld_h < H)) || ld_g < 4L * H || ld_c < H || ld_out < H)
    return DEER_ERR_SHAPE;
  return seq_lstm_step_launch(gates, ld_g, h_prev, ld_h, c_prev, ld_c, nullptr, nullptr, w_hh, SEQ_W_F32, b_hh, c_out, ld_c, h_out, ld_out, nullptr,
                              nullptr, gates, ld_g, N, H, stream);
}

extern "C" int deer_head_seq_ln(const float* src, long ld_src, float* dst, long ld_dst, const float* w, const float* b, int M, int n, float eps,
                                int relu, void* stream) {
  if (src == nullptr || dst == nullptr || w == nullptr || b == nullptr || M <= 0 || n <= 0 || ld_src < n || ld_dst < n)
    return DEER_ERR_SHAPE;
  hipLaunchKernelGGL(seq_ln_kernel, dim3((M + 3) / 4), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), src, ld_src, dst, ld_dst, w, b,
                     static_cast<float*>(nullptr), M, n, eps, relu);
  DEER_LAUNCH_CHECK();
  return DEER_OK;
}

// deer_head_seq_ln that keeps the statistics of every row for the backward: stats[m] = (mean, rstd)
extern "C" int deer_head_grad_ln(const float* src, long ld_src, float* dst, long ld_dst, const float* w, const float* b, float* stats, int M, int n,
                                 float eps, int relu, void* stream) {
  if (src == nullptr || dst == nullptr || w == nullptr || b == nullptr || stats == nullptr || M <= 0 || n <= 0 || ld_src < n || ld_dst < n)
    return DEER_ERR_SHAPE;
  hipLaunchKernelGGL(seq_ln_kernel, dim3((M + 3) / 4), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), src, ld_src, dst, ld_dst, w, b, stats, M,
                     n, eps, relu);
  DEER_LAUNCH_CHECK();
  return DEER_OK;
}
