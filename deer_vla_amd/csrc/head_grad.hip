// Exit-only fine-tuning of one action head: the device pieces of the reference's second training stage (only_train_head /
// no_backbone_grad, robot_flamingo/train/train_utils.py:487-543 backward half; AdamW of train_calvin_post_strategy.py:466-535) that
// csrc/head_seq.hip and csrc/exit_eval.hip do not already have.  The head is DeterministicDecoder in window mode (action_head.py:588-595)
// on pooled rows X [N][L][d] from a zero state, no dropout, evaluated from a FLAT f32 parameter buffer (deer_head_param_entry).
//
// The taped forward and the loss with its gradient are the kernels of those two files (deer_head_seq_gemm, deer_head_grad_lstm_step,
// deer_head_grad_ln: csrc/head_seq.hip; deer_head_grad_loss: csrc/exit_eval.hip).  This file holds
//   backward          a strided exact-f32 MFMA GEMM (dX = dY W, dW = dY^T X: either operand may be stored k-major), column sums
//                     (db, LayerNorm d gamma / d beta), the ReLU mask, LayerNorm backward, one recurrent launch per time step
//   deer_adamw_step   torch.optim.AdamW over flat (param, grad, m, v) buffers, decoupled decay per segment
// All arithmetic is f32; every sum has a fixed order and there are no atomics (identical inputs give identical bits); every store is a
// vector-memory store; reads past a matrix edge are masked to zero and never stored.
#include "common.h"
#include "../../include/deer_hip.h"

namespace {

// ---- strided exact-f32 GEMM: C[m][n] (+)= sum_k opA(m, k) opB(n, k) --------------------------------------------------------------------
// TA = 0: A stored [M][K] (row pitch lda), TA = 1: stored [K][M]; TB likewise for B ([N][K] is nn.Linear's layout).  The tile of
// csrc/precise.hip::gemm_f32_kernel (64 x 64 x 32, two LDS stages, v_mfma_f32_16x16x4_f32), with loaders for either storage order.  A
// k-major operand is read in 16-byte pieces along its contiguous index and scattered into the [row][k] LDS image.  vec bit 0 / 1 / 2:
// A / B / C may be accessed as aligned float4 (pointer, pitch and contiguous extent multiples of 4 floats); otherwise element by element.
#define HG_BK 32
#define HG_PITCH 36

template <bool T>
__device__ __forceinline__ void hg_gload(const float* __restrict__ P, long ld, int r0, int k0, int R, int K, bool vec, int tid, float4 (&v)[2]) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int id = tid + i * 256;
    // !T: row = id / 8, 4 k at (id % 8) * 4.  T: k = id / 16, 4 rows at (id % 16) * 4.
    const int row = T ? (id & 15) * 4 : id >> 3;
    const int k = T ? id >> 4 : (id & 7) * 4;
    const int cont0 = T ? r0 + row : k0 + k;          // first index along the contiguous direction
    const int cont_n = T ? R : K;
    const int other = T ? k0 + k : r0 + row;
    const int other_n = T ? K : R;
    float4 t = float4{0.f, 0.f, 0.f, 0.f};
    if (other < other_n && cont0 < cont_n) {
      const float* p = P + (long)other * ld + cont0;
      if (vec) t = *reinterpret_cast<const float4*>(p);
      else {
        t.x = p[0];
        if (cont0 + 1 < cont_n) t.y = p[1];
        if (cont0 + 2 < cont_n) t.z = p[2];
        if (cont0 + 3 < cont_n) t.w = p[3];
      }
    }
    v[i] = t;
  }
}

template <bool T>
__device__ __forceinline__ void hg_swrite(float (*S)[HG_PITCH], int tid, const float4 (&v)[2]) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int id = tid + i * 256;
    if constexpr (T) {
      const int row = (id & 15) * 4, k = id >> 4;
      S[row][k] = v[i].x;
      S[row + 1][k] = v[i].y;
      S[row + 2][k] = v[i].z;
      S[row + 3][k] = v[i].w;
    } else {
      *reinterpret_cast<float4*>(&S[id >> 3][(id & 7) * 4]) = v[i];
    }
  }
}

template <bool TA, bool TB>
__global__ __launch_bounds__(256) void hg_gemm_kernel(const float* __restrict__ A, long lda, const float* __restrict__ B, long ldb, float* C,
                                                      long ldc, int M, int N, int K, int accumulate, int vec) {
  __shared__ __attribute__((aligned(16))) float As[2][64][HG_PITCH];
  __shared__ __attribute__((aligned(16))) float Bs[2][64][HG_PITCH];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int c = lane & 15, g = lane >> 4;
  const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
  const bool va = vec & 1, vb = vec & 2, vc = vec & 4;

  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  float4 ra[2], rb[2];
  const int nk = (K + HG_BK - 1) / HG_BK;
  hg_gload<TA>(A, lda, m0, 0, M, K, va, tid, ra);
  hg_gload<TB>(B, ldb, n0, 0, N, K, vb, tid, rb);
  hg_swrite<TA>(As[0], tid, ra);
  hg_swrite<TB>(Bs[0], tid, rb);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int buf = kt & 1;
    if (kt + 1 < nk) {
      hg_gload<TA>(A, lda, m0, (kt + 1) * HG_BK, M, K, va, tid, ra);
      hg_gload<TB>(B, ldb, n0, (kt + 1) * HG_BK, N, K, vb, tid, rb);
    }
#pragma unroll
    for (int kk = 0; kk < HG_BK / 4; ++kk) {
      float af[2], bf[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) af[j] = As[buf][wm * 32 + j * 16 + c][kk * 4 + g];
#pragma unroll
      for (int i = 0; i < 2; ++i) bf[i] = Bs[buf][wn * 32 + i * 16 + c][kk * 4 + g];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(bf[i], af[j], acc[i][j], 0, 0, 0);
    }
    if (kt + 1 < nk) {
      hg_swrite<TA>(As[buf ^ 1], tid, ra);
      hg_swrite<TB>(Bs[buf ^ 1], tid, rb);
    }
    __syncthreads();
  }

  // lane holds C[m = .. + c][n = .. + 4 g .. + 3] (the B fragment is the MFMA's first operand, like the weight fragment of gemm_f32_kernel)
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int n = n0 + wn * 32 + i * 16 + g * 4;
    if (n >= N) continue;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int m = m0 + wm * 32 + j * 16 + c;
      if (m >= M) continue;
      float* p = C + (long)m * ldc + n;
      if (vc) {
        float4 r = float4{acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]};
        if (accumulate) {
          const float4 o = *reinterpret_cast<const float4*>(p);
          r.x += o.x; r.y += o.y; r.z += o.z; r.w += o.w;
        }
        *reinterpret_cast<float4*>(p) = r;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (n + e < N) p[e] = accumulate ? p[e] + acc[i][j][e] : acc[i][j][e];
      }
    }
  }
}

// ---- column sums over M rows: out_sum[col] (+)= sum_m dy[m][col]; out_xhat[col] (+)= sum_m dy[m][col] (x[m][col] - mean_m) rstd_m -------
// (bias gradients; LayerNorm d beta and d gamma).  Workgroup = 64 columns; wave w sums rows w, w + 4, .. in that order, the four partial
// sums meet in LDS and are added in wave order.
__global__ __launch_bounds__(256) void hg_colsum_kernel(const float* __restrict__ dy, long ld, const float* __restrict__ x, long ldx,
                                                        const float* __restrict__ stats, float* out_sum, float* out_sum2, float* out_xhat, int M,
                                                        int n, int accumulate) {
  __shared__ float part[2][4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = blockIdx.x * 64 + lane;
  float s = 0.f, sx = 0.f;
  if (col < n) {
    for (int m = wave; m < M; m += 4) {
      const float v = dy[(long)m * ld + col];
      s += v;
      if (x != nullptr) sx += v * ((x[(long)m * ldx + col] - stats[2 * m]) * stats[2 * m + 1]);
    }
  }
  part[0][wave][lane] = s;
  part[1][wave][lane] = sx;
  __syncthreads();
  if (wave == 0 && col < n) {
    const float t = ((part[0][0][lane] + part[0][1][lane]) + part[0][2][lane]) + part[0][3][lane];
    if (out_sum != nullptr) out_sum[col] = accumulate ? out_sum[col] + t : t;
    if (out_sum2 != nullptr) out_sum2[col] = accumulate ? out_sum2[col] + t : t;
    if (out_xhat != nullptr) {
      const float tx = ((part[1][0][lane] + part[1][1][lane]) + part[1][2][lane]) + part[1][3][lane];
      out_xhat[col] = accumulate ? out_xhat[col] + tx : tx;
    }
  }
}

// ---- ReLU mask: dz[i] = act[i] > 0 ? dz[i] : 0 over n (multiple of 4) contiguous values ---------------------------------------------
__global__ __launch_bounds__(256) void hg_relu_mask_kernel(float* __restrict__ dz, const float* __restrict__ act, long n4) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  float4 d = reinterpret_cast<float4*>(dz)[i];
  const float4 a = reinterpret_cast<const float4*>(act)[i];
  d.x = a.x > 0.f ? d.x : 0.f;
  d.y = a.y > 0.f ? d.y : 0.f;
  d.z = a.z > 0.f ? d.z : 0.f;
  d.w = a.w > 0.f ? d.w : 0.f;
  reinterpret_cast<float4*>(dz)[i] = d;
}

// ---- LayerNorm backward of rows (one wave per row): dx = rstd (g - mean(g) - xhat mean(g xhat)), g = dy gamma; dx may be dy ---------------
__global__ __launch_bounds__(256) void hg_ln_bwd_kernel(const float* dy, long ld_dy, const float* __restrict__ x, long ld_x,
                                                        const float* __restrict__ stats, const float* __restrict__ gamma, float* dx, long ld_dx,
                                                        int M, int n) {
  const int lane = threadIdx.x & 63;
  const long m = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m >= M) return;
  const float mean = stats[2 * m], rstd = stats[2 * m + 1];
  const float* dyr = dy + m * ld_dy;
  const float* xr = x + m * ld_x;
  float s1 = 0.f, s2 = 0.f;
  for (int i = lane; i < n; i += 64) {
    const float g = dyr[i] * gamma[i];
    s1 += g;
    s2 += g * ((xr[i] - mean) * rstd);
  }
  s1 = wave_sum(s1) / n;
  s2 = wave_sum(s2) / n;
  for (int i = lane; i < n; i += 64) {
    const float g = dyr[i] * gamma[i];
    dx[m * ld_dx + i] = rstd * ((g - s1) - ((xr[i] - mean) * rstd) * s2);
  }
}

// ---- one time step of the LSTM's backward through time over N rows --------------------------------------------------------------------
// dh_t = dh_ext[m] + dG_{t+1}[m] W_hh (the recurrent term; dg_next NULL at t = L - 1), then per unit u
//   do = dh tanh(c_t), dc = dc_in + dh o (1 - tanh^2(c_t)), di = dc g, df = dc c_{t-1}, dg = dc i, dc_{t-1} = dc f
//   dG_t = [di i (1 - i) | df f (1 - f) | dg (1 - g^2) | do o (1 - o)]  (pre-activation gate gradients, torch order i, f, g, o)
// Workgroup = 16 hidden units x 32 rows, the mirror of the forward step: its four waves split K = 4H in chunks of 16, W_hh[k][u] is read
// along u (its contiguous index), the partial tiles meet in LDS and are summed in wave order.  dc [N][H] is read (unless dg_next is NULL:
// zero) and written in place, each element by one thread.
__global__ __launch_bounds__(256) void hg_lstm_bwd_step_kernel(const float* __restrict__ dh_ext, long ld_dh, const float* __restrict__ dg_next,
                                                               const float* __restrict__ gates, float* __restrict__ dg, long ld_g,
                                                               const float* __restrict__ w_hh, const float* __restrict__ c_t,
                                                               const float* __restrict__ c_prev, long ld_c, float* __restrict__ dc, int N, int H) {
  __shared__ float part[4][SEQ_RT / 16][64][4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = lane & 15, g = lane >> 4;
  const int u0 = blockIdx.x * 16, m0 = blockIdx.y * SEQ_RT;
  f32x4 acc[SEQ_RT / 16];
#pragma unroll
  for (int j = 0; j < SEQ_RT / 16; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (dg_next != nullptr) {
    long xr[SEQ_RT / 16];
#pragma unroll
    for (int j = 0; j < SEQ_RT / 16; ++j) xr[j] = min(m0 + j * 16 + c, N - 1);
    const int K = 4 * H;                                     // multiple of 64
    for (int k0 = wave * 16; k0 < K; k0 += 64) {
      const int k = k0 + g * 4;
      // the four k of this lane's slice go through four 16x16x4 steps (both operands use the same k permutation)
      const float* wp = w_hh + (long)k * H + u0 + c;
      const float w0 = wp[0], w1 = wp[H], w2 = wp[2L * H], w3 = wp[3L * H];
#pragma unroll
      for (int j = 0; j < SEQ_RT / 16; ++j) {
        const float4 x = *reinterpret_cast<const float4*>(dg_next + xr[j] * ld_g + k);
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(w0, x.x, acc[j], 0, 0, 0);
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(w1, x.y, acc[j], 0, 0, 0);
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(w2, x.z, acc[j], 0, 0, 0);
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(w3, x.w, acc[j], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < SEQ_RT / 16; ++j)
    *reinterpret_cast<float4*>(&part[wave][j][lane][0]) = float4{acc[j][0], acc[j][1], acc[j][2], acc[j][3]};
  __syncthreads();
  for (int p = threadIdx.x; p < 16 * SEQ_RT; p += 256) {
    const int ul = p & 15, rl = p >> 4;
    const int m = m0 + rl, u = u0 + ul;
    if (m >= N) continue;
    const int j = rl >> 4, pl = ((ul >> 2) << 4) | (rl & 15), r = ul & 3;
    const float rec = ((part[0][j][pl][r] + part[1][j][pl][r]) + part[2][j][pl][r]) + part[3][j][pl][r];
    const float dh = dh_ext[(long)m * ld_dh + u] + rec;
    const float* gr = gates + (long)m * ld_g;
    const float gi = gr[u], gf = gr[H + u], gg = gr[2 * H + u], go = gr[3 * H + u];
    const float tc = tanhf(c_t[(long)m * ld_c + u]);
    const float cp = c_prev != nullptr ? c_prev[(long)m * ld_c + u] : 0.f;
    const float dcn = dg_next != nullptr ? dc[(long)m * H + u] : 0.f;
    const float dcv = dcn + dh * go * (1.f - tc * tc);
    float* d = dg + (long)m * ld_g;
    d[u] = (dcv * gg) * gi * (1.f - gi);
    d[H + u] = (dcv * cp) * gf * (1.f - gf);
    d[2 * H + u] = (dcv * gi) * (1.f - gg * gg);
    d[3 * H + u] = (dh * tc) * go * (1.f - go);
    dc[(long)m * H + u] = dcv * gf;
  }
}

// ---- torch.optim.AdamW, one element per thread ------------------------------------------------------------------------------------------
// p <- p (1 - lr wd) on the elements of a decaying segment; m <- m + (g - m)(1 - b1); v <- b2 v + (1 - b2) g g;
// p <- p - (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps)   (torch/optim/adamw.py _single_tensor_adamw).  seg_end: ascending exclusive ends of
// the n_seg segments, seg_decay: 1 = decays; an element past the last end (padding) takes no decay.
__global__ __launch_bounds__(256) void hg_adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                       float* __restrict__ v, long n, const int* __restrict__ seg_end,
                                                       const int* __restrict__ seg_decay, int n_seg, float decay_mul, float one_minus_b1, float b2,
                                                       float one_minus_b2, float step_size, float bc2_sqrt, float eps) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  bool decays = n_seg == 0;
  if (n_seg > 0) {
    int lo = 0, hi = n_seg;                                // first segment whose end is > i
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if ((long)seg_end[mid] > i) hi = mid;
      else lo = mid + 1;
    }
    decays = lo < n_seg && seg_decay[lo] != 0;
  }
  float pv = p[i];
  const float gv = g[i];
  if (decays) pv *= decay_mul;
  const float mv = m[i] + (gv - m[i]) * one_minus_b1;
  const float vv = v[i] * b2 + one_minus_b2 * gv * gv;
  const float denom = sqrtf(vv) / bc2_sqrt + eps;
  m[i] = mv;
  v[i] = vv;
  p[i] = pv - step_size * (mv / denom);
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int deer_head_grad_gemm(const float* A, long lda, int ta, const float* B, long ldb, int tb, float* C, long ldc, int M, int N, int K,
                                   int accumulate, void* stream) {
  if (A == nullptr || B == nullptr || C == nullptr || M <= 0 || N <= 0 || K <= 0 || lda < (ta ? M : K) || ldb < (tb ? N : K) || ldc < N ||
      (M + 63) / 64 > 65535)
    return DEER_ERR_SHAPE;
  const int vec = ((al16(A) && !(lda & 3) && !((ta ? M : K) & 3)) ? 1 : 0) | ((al16(B) && !(ldb & 3) && !((tb ? N : K) & 3)) ? 2 : 0) |
                  ((al16(C) && !(ldc & 3) && !(N & 3)) ? 4 : 0);
  dim3 grid((N + 63) / 64, (M + 63) / 64);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (ta && tb) hipLaunchKernelGGL((hg_gemm_kernel<true, true>), grid, dim3(256), 0, st, A, lda, B, ldb, C, ldc, M, N, K, accumulate, vec);
  else if (ta) hipLaunchKernelGGL((hg_gemm_kernel<true, false>), grid, dim3(256), 0, st, A, lda, B, ldb, C, ldc, M, N, K, accumulate, vec);
  else if (tb) hipLaunchKernelGGL((hg_gemm_kernel<false, true>), grid, dim3(256), 0, st, A, lda, B, ldb, C, ldc, M, N, K, accumulate, vec);
  else hipLaunchKernelGGL((hg_gemm_kernel<false, false>), grid, dim3(256), 0, st, A, lda, B, ldb, C, ldc, M, N, K, accumulate, vec);
  DEER_LAUNCH_CHECK();
  return DEER_OK;
}

extern "C" int deer_head_grad_colsum(const float* dy, long ld, const float* x, long ldx, const float* stats, float* out_sum, float* out_sum2,
                                     float* out_xhat, int M, int n, int accumulate, void* stream) {
  if (dy == nullptr || (out_sum == nullptr && out_xhat == nullptr) || M <= 0 || n <= 0 || ld < n ||
      (out_xhat != nullptr && (x == nullptr || stats == nullptr || ldx < n)) || (out_xhat == nullptr && x != nullptr))
    return DEER_ERR_SHAPE;
  hipLaunchKernelGGL(hg_colsum_kernel, dim3((n + 63) / 64), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), dy, ld, x, ldx, stats, out_sum,
                     out_sum2, out_xhat, M, n, accumulate);
  DEER_LAUNCH_CHECK();
  return DEER_OK;
}

extern "C" int deer_head_grad_relu_mask(float* dz, const float* act, long n, void* stream) {
  if (dz == nullptr || act == nullptr || n <= 0 || (n & 3) || !al16(dz) || !al16(act) || (n / 4 + 255) / 256 > 0x7fffffffL) return DEER_ERR_SHAPE;
  hipLaunchKernelGGL(hg_relu_mask_kernel, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), dz, act, n / 4);
  DEER_LAUNCH_CHECK();
  return DEER_OK;
}

extern "C" int deer_head_grad_ln_bwd(const float* dy, long ld_dy, const float* x, long ld_x, const float* stats, const float* gamma, float* dx,
                                     long ld_dx, int M, int n, void* stream) {
  if (dy == nullptr || x == nullptr || stats == nullptr || gamma == nullptr || dx == nullptr || M <= 0 || n <= 0 || ld_dy < n || ld_x < n || ld_dx < n)
    return DEER_ERR_SHAPE;
  hipLaunchKernelGGL(hg_ln_bwd_kernel, dim3((M + 3) / 4), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), dy, ld_dy, x, ld_x, stats, gamma, dx,
                     ld_dx, M, n);
  DEER_LAUNCH_CHECK();
  return DEER_OK;
}

extern "C" int deer_head_grad_lstm_bwd_step(const float* dh_ext, long ld_dh, const float* dg_next, const float* gates, float* dg, long ld_g,
                                            const float* w_hh, const float* c_t, const float* c_prev, long ld_c, float* dc, int N, int H,
                                            void* stream) {
  if (dh_ext == nullptr || gates == nullptr || dg == nullptr || w_hh == nullptr || c_t == nullptr || dc == nullptr || N <= 0 || H <= 0 || (H & 15) ||
      ld_dh < H || ld_g < 4L * H || (ld_g & 3) || ld_c < H || (dg_next != nullptr && !al16(dg_next)) || (N + SEQ_RT - 1) / SEQ_RT > 65535)
    return DEER_ERR_SHAPE;
  hipLaunchKernelGGL(hg_lstm_bwd_step_kernel, dim3(H / 16, (N + SEQ_RT - 1) / SEQ_RT), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), dh_ext,
                     ld_dh, dg_next, gates, dg, ld_g, w_hh, c_t, c_prev, ld_c, dc, N, H);
  DEER_LAUNCH_CHECK();
  return DEER_OK;
}

extern "C" int deer_adamw_step(float* param, const float* grad, float* m, float* v, long numel, const int* seg_end, const int* seg_decay, int n_seg,
                               const double* hyper, int step, void* stream) {
  if (param == nullptr || grad == nullptr || m == nullptr || v == nullptr || hyper == nullptr || numel <= 0 || numel > 0x7fffffffL || n_seg < 0 ||
      (n_seg > 0 && (seg_end == nullptr || seg_decay == nullptr)) || step < 1)
    return DEER_ERR_SHAPE;
  const double lr = hyper[0], beta1 = hyper[1], beta2 = hyper[2], eps = hyper[3], weight_decay = hyper[4];
  if (!(lr >= 0.0) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0) || !(weight_decay >= 0.0)) return DEER_ERR_SHAPE;
  // the scalars torch computes in Python floats (doubles) and hands to its f32 kernels: 1 - beta, the bias corrections by step count
  const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
  hipLaunchKernelGGL(hg_adamw_kernel, dim3((unsigned)((numel + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), param, grad, m, v,
                     numel, seg_end, seg_decay, n_seg, (float)(1.0 - lr * weight_decay), (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2),
                     (float)(lr / bc1), (float)sqrt(bc2), (float)eps);
  DEER_LAUNCH_CHECK();
  return DEER_OK;
}
