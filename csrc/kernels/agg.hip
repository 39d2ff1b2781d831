// Aggregation / attack kernels on the gathered client-update matrix U[N, P] (fp32, row-major).
//
//   colstats        column mean / unbiased std (+ LIE candidate mean + z*std)      K-G2/K-G3
//   weighted_rows   out = sum_i w_i U_i (fp64 weights, fp64 accumulate)            K-G1 FedAvg
//   mix_rows        Y = W U, W [R][N] fp64, one pass over U (pre-aggregation: NNM, bucketing; beyond the reference)
//   nnm_weights     nearest-neighbour mixing's W from the distance matrix, one wave (the row sort of krum_select)
//   pair_sqdist     D2[i][j] = ||U_i - U_j||^2 (fp64 difference form, no cancellation) K-G4b / Krum (K > 64)
//   gram_f64        the same from the Gram matrix of the rows centred on a robustly  K-G4b / Krum (K <= 64)
//                   chosen row, on fp64 MFMA
//   noise_philox    own + sigma * N(0,1) from Philox4x32-10 + Box-Muller             K-G10
//   seg_reduce      per-(row, state_dict tensor) partial sums over tiles             K-G4a / K-G5
//   coord_select    coordinate-wise lower median / trimmed mean (register sort)      K-G6
//   row_dots        <u,u>, <u,r>, <r,r> per row                                      K-G8
//   stoch_quant     ScionFL 1-bit stochastic quantisation                            K-G9
//   adam_flat       Adam over a flat arena (optional grad scale = clip coefficient)  K-O1
//   krum_select     Multi-Krum ranking / Bulyan iterated selection on the distance matrix (beyond the reference)
//   bulyan_coord    Bulyan's mean of the beta values closest to the column median, over selected rows
//   geomed_weights  smoothed Weiszfeld (geometric median, RFA) in Gram space
//   cclip_weights   centred clipping in Gram space (anchored Gram: gram_f64 about the previous global model)
//   anchored_rows   out = g + sum_i c_i (U_i - g) (fp64 weights, fp64 accumulate): centred clipping's row pass
//   hist_gram       FoolsGold: H_new = H_old + (U - g) and the fp64-MFMA Gram of H_new in one sweep (gram_f64's tile body)
//   foolsgold_weights  FoolsGold: cosines, pardoning and the logit weights from that Gram, one wave
//   dnc_gram        DnC: fp64-MFMA Grams over keyed random column subsets, all iterations in one launch
//   dnc_select      DnC: top eigenpair, scores, ranked drop, mask intersection and weights, one wave
//   sign_stats      SignGuard: squared norms about the centre and sign counts on a column window, one pass
//   signguard_select  SignGuard: norm filter, mean-shift clustering of the sign features and clipped weights, one wave
//   flame_select    FLAME: majority cluster of the cosine distances (spanning tree + unions), clipped weights, one wave
//   flame_rows      FLAME: anchored_rows' sum plus sigma * N(0, 1) (Philox), sigma read from the device
// Shared: gram_for_tiles (the host's one T = 1 .. 4 launch of gram_f64, hist_gram and dnc_gram), gram_tile_mfma and
// gram_block_partials (the tile body of gram_f64 and hist_gram, whose Grams must agree bit for bit) and lds_load_square
// (the matrix load of geomed_weights, cclip_weights and foolsgold_weights).  The device code of gram_f64 and dnc_gram
// and of the one-wave kernels is otherwise kept per kernel: folding it cost 0.2 - 3 % in single-call timings
// (profiles/ab_agg_refactor.md).
//
// Every reduction is two-pass with a fixed summation order (no float atomics), so results are
// bit-identical across ranks: the replicated server state on each rank stays in lock-step.
#include "common.h"
#include "kernels.h"
#include "plan_perm.h"
#include <type_traits>

// A [n][ld] in LDS <- the n x n fp64 matrix G (the one-wave n <= 64 kernels: 64-thread blocks)
__device__ __forceinline__ void lds_load_square(double* __restrict__ A, int ld, const double* __restrict__ G, int n) {
  for (int e = threadIdx.x; e < n * n; e += 64) A[e / n * ld + e % n] = G[e];
}

// ============================================================================ colstats
__global__ void __launch_bounds__(256) k_colstats(const float* __restrict__ G, int K, long P, float* __restrict__ mean,
                                                  float* __restrict__ stdv, float* __restrict__ out, float z, int mode) {
  long c = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= P) return;
  double s = 0.0;
  for (int k = 0; k < K; ++k) s += (double)G[(long)k * P + c];
  double m = s / K;
  double ss = 0.0;
  for (int k = 0; k < K; ++k) {
    double d = (double)G[(long)k * P + c] - m;
    ss += d * d;
  }
  float mf = (float)m;
  float sf = K > 1 ? (float)sqrt(ss / (K - 1)) : __int_as_float(0x7fc00000);
  mean[c] = mf;
  stdv[c] = sf;
  if (mode == 1) out[c] = mf + z * sf;
}

void afl_colstats(const float* G, int K, long P, float* mean, float* stdv, float* out, float z, int mode,
                  hipStream_t s) {
  hipLaunchKernelGGL(k_colstats, dim3(afl_cdiv(P, 256)), dim3(256), 0, s, G, K, P, mean, stdv, out, z, mode);
}

// ============================================================================ weighted rows
// The accumulate step of weighted_rows and mix_rows, stated once (an explicit fma, which is what the contracted
// acc += w * u compiled to): a mixed row carries the bits of the weighted_rows call with that row of weights.
__device__ __forceinline__ double row_acc(double acc, double w, double u) { return fma(w, u, acc); }

// ok (optional, int32 [N]): every entry > 0 -> the weighted sum, else out = fallback (FedAvg keeps the previous global
// model when a client failed: the early-launch aggregate, decided on the device in the same pass)
__global__ void __launch_bounds__(256) k_weighted_rows(const float* __restrict__ U, const double* __restrict__ w, int N,
                                                       long P, float* __restrict__ out, const int* __restrict__ ok,
                                                       const float* __restrict__ fallback) {
  long c = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= P) return;
  bool all_ok = true;
  if (ok != nullptr)
    for (int i = 0; i < N; ++i) all_ok = all_ok && ok[i] > 0;
  if (!all_ok) {
    out[c] = fallback[c];
    return;
  }
  double acc = 0.0;
  for (int i = 0; i < N; ++i) acc = row_acc(acc, w[i], (double)U[(long)i * P + c]);
  out[c] = (float)acc;
}

void afl_weighted_rows(const float* U, const double* w, int N, long P, float* out, hipStream_t s, const int* ok,
                       const float* fallback) {
  hipLaunchKernelGGL(k_weighted_rows, dim3(afl_cdiv(P, 256)), dim3(256), 0, s, U, w, N, P, out, ok, fallback);
}

// ============================================================================ mix rows
// Y = W U for a small dense W [R][N] (fp64) in ONE pass over U [N][P]: the row mix of pre-aggregation (nearest-neighbour
// mixing, bucketing; docs/PARITY.md).  Thread per column: the column's N values sit in registers (as the doubles the
// accumulate step takes: the conversion is exact and is paid once, not once per mixed row), then for every r an fp64
// dot in ascending j over every j (zero weights included, as weighted_rows does) and a coalesced store of Y[r][c].
// W is staged once per block in LDS (R * NMAX doubles, at most 32 KB); every lane reads the same entry, a broadcast.
// N <= NMAX <= 64, R <= 64.  The dot is unrolled over all NMAX terms without a branch: a term j >= N is W = -0.0 times
// value +0.0, and adding that -0.0 returns every accumulator unchanged, a zero of either sign included, so Y[r] is the
// bits of weighted_rows(U, W[r]) for every N.
template <int NMAX>
__global__ void __launch_bounds__(256) k_mix_rows(const float* __restrict__ U, const double* __restrict__ W, int N, int R,
                                                  long P, float* __restrict__ Y) {
  extern __shared__ double mix_w[];  // [R][NMAX]
  for (int e = threadIdx.x; e < R * NMAX; e += 256) {
    const int r = e / NMAX, j = e - r * NMAX;
    mix_w[e] = j < N ? W[r * N + j] : -0.0;
  }
  __syncthreads();
  const long c = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long cc = c < P ? c : P - 1;  // (a thread past the last column mixes that column again and stores nothing)
  double v[NMAX];
#pragma unroll
  for (int j = 0; j < NMAX; ++j) {
    const float u = U[(long)(j < N ? j : N - 1) * P + cc];
    v[j] = j < N ? (double)u : 0.0;
  }
  for (int r = 0; r < R; ++r) {
    const double* w = mix_w + r * NMAX;
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < NMAX; ++j) acc = row_acc(acc, w[j], v[j]);
    if (c < P) Y[(long)r * P + c] = (float)acc;
  }
}

int afl_mix_rows(const float* U, const double* W, int N, int R, long P, float* Y, hipStream_t s) {
  if (N < 1 || N > 64 || R < 1 || R > 64 || P < 1) return (int)hipErrorInvalidValue;
  dim3 g(afl_cdiv(P, 256)), b(256);
  const size_t lds = sizeof(double) * (size_t)R;  // x NMAX
  if (N <= 8) hipLaunchKernelGGL(k_mix_rows<8>, g, b, lds * 8, s, U, W, N, R, P, Y);
  else if (N <= 16) hipLaunchKernelGGL(k_mix_rows<16>, g, b, lds * 16, s, U, W, N, R, P, Y);
  else if (N <= 32) hipLaunchKernelGGL(k_mix_rows<32>, g, b, lds * 32, s, U, W, N, R, P, Y);
  else hipLaunchKernelGGL(k_mix_rows<64>, g, b, lds * 64, s, U, W, N, R, P, Y);
  return (int)hipGetLastError();
}

// ============================================================================ pairwise sq-dist
// Block b stages a [K][CH] column chunk in LDS (row stride CH+1: conflict-free column reads),
// then threads loop over pairs; partial[b][pair] (fp64) is reduced by k_pair_reduce.  The difference and its
// square are formed in fp64 (the difference of two fp32 values is exact there), so a distance carries only the
// rounding of its fp64 sum: at most P * 2^-53 relative.  K <= 128: K * 257 * 4 bytes of LDS, above the 64 KB
// default from K = 64 on (the launcher raises the kernel's dynamic-LDS limit).
constexpr int PD_CH = 256;
__global__ void __launch_bounds__(256) k_pair_sqdist(const float* __restrict__ G, int K, long P,
                                                     double* __restrict__ partial) {
  extern __shared__ float lds[];  // K * (PD_CH + 1)
  const long c0 = (long)blockIdx.x * PD_CH;
  const int ncol = (int)min((long)PD_CH, P - c0);
  for (int k = 0; k < K; ++k)
    for (int j = threadIdx.x; j < PD_CH; j += blockDim.x)
      lds[k * (PD_CH + 1) + j] = j < ncol ? G[(long)k * P + c0 + j] : 0.f;
  __syncthreads();
  const int M = K * (K - 1) / 2;
  for (int pr = threadIdx.x; pr < M; pr += blockDim.x) {
    // pair index -> (i, j), i < j
    int i = 0, rem = pr;
    while (rem >= K - 1 - i) { rem -= K - 1 - i; ++i; }
    int j = i + 1 + rem;
    const float* a = lds + i * (PD_CH + 1);
    const float* b = lds + j * (PD_CH + 1);
    double acc = 0.0;
    for (int t = 0; t < ncol; ++t) {
      const double d = (double)a[t] - (double)b[t];
      acc += d * d;
    }
    partial[(long)blockIdx.x * M + pr] = acc;
  }
}

__global__ void k_pair_reduce(const double* __restrict__ partial, int nb, int K, double* __restrict__ D) {
  const int M = K * (K - 1) / 2;
  int pr = blockIdx.x * blockDim.x + threadIdx.x;
  if (pr >= M) return;
  double acc = 0.0;
  for (int b = 0; b < nb; ++b) acc += partial[(long)b * M + pr];
  int i = 0, rem = pr;
  while (rem >= K - 1 - i) { rem -= K - 1 - i; ++i; }
  int j = i + 1 + rem;
  D[i * K + j] = acc;
  D[j * K + i] = acc;
}

int afl_pair_sqdist_nblocks(long P) { return afl_cdiv(P, PD_CH); }

int afl_pair_sqdist(const float* G, int K, long P, double* partial, double* D, hipStream_t s) {
  if (K < 2 || K > 128 || P < 1) return (int)hipErrorInvalidValue;
  int nb = afl_cdiv(P, PD_CH);
  size_t lds = (size_t)K * (PD_CH + 1) * sizeof(float);
  if (lds > 64 * 1024 &&
      hipFuncSetAttribute((const void*)k_pair_sqdist, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return -2;
  hipLaunchKernelGGL(k_pair_sqdist, dim3(nb), dim3(256), lds, s, G, K, P, partial);
  int M = K * (K - 1) / 2;
  hipLaunchKernelGGL(k_pair_reduce, dim3(afl_cdiv(M, 256)), dim3(256), 0, s, partial, nb, K, D);
  return (int)hipGetLastError();
}

// ============================================================================ pairwise via Gram (MFMA)
// D2[i][j] = ||G_i - G_j||^2 = g_ii + g_jj - 2 g_ij from the Gram matrix g of the CENTRED rows X_i = G_i - G_c: the
// difference-form correction — model updates are close to each other, so the Gram form of the raw rows would
// cancel catastrophically, while rows centred on one of their own have norms of the order of the distances.
// The centring is done in fp64 (the difference of two fp32 values: exact), the products run on
// v_mfma_f64_16x16x4_f64 with fp64 accumulation.  Error model:
//     err(D_ij) <~ eps64 * (|x_i|^2 + |x_j|^2),  x centred on the chosen row c
// so D_ij is exact to fp64 rounding while x_i, x_j are not much longer than the distance itself, and loses
// log2((|x_i|^2 + |x_j|^2) / D_ij) bits otherwise.  Two passes choose c:
//   pass 1  c = 0.  Good when row 0 is a typical row; when client 0 is an outlier (a Random or scaled attack
//           row) every benign x_i is huge and a benign-pair distance keeps only a few digits.
//   pick    gram_pick_centre (the block of pass 1's reduction, at its end): c* = argmin_i lowermedian_{j != i}
//           D1[i][j], ties to the lowest index — the row closest to the bulk, an outlier only when outliers are
//           the majority; row 0 is kept while it is itself such a row.  Written to a device word: no host read,
//           and a function of D1 alone, so the result stays bit-identical run to run.
//   pass 2  the same kernels centred on c*, read from that word; its blocks return at once when c* == 0 and
//           leave D and the Gram as pass 1 wrote them.
// With a minority of outliers the result is exact to fp64 rounding for every pair.  It is NOT for two distant
// tight clusters: whichever row is the centre, the other cluster's rows have |x|^2 of the order of the squared
// cluster gap, and its within-cluster distances carry an absolute error of eps64 times that.
// K <= 64 (T <= 4 row tiles of 16).  Block b covers GR_CH columns; each of its 4 waves a quarter of them,
// 16 columns per step: lane l loads 4 consecutive columns of row (tile*16 + (l & 15)), column group l >> 4,
// and issues 4 MFMAs per tile pair (element q of the 4 = MFMA q's k = l >> 4: the 16 columns are summed in a
// fixed, data-independent order).  f64 C/D layout: acc[r] = C[(l >> 4) + 4r][l & 15].
// An external centre (``anchor`` [P], afl_gram_anchored: centred clipping's previous global model) replaces the
// centre row: y_i = G_i - anchor, one pass, and k_gram_reduce's ``gram`` is then the raw Gram Y Y^T about it.  Error
// model of that form:
//     err(G_ij) <~ eps64 * |y_i| |y_j|
// and a distance formed from it, d_i^2 = G_ii - 2 (G c)_i + c^T G c to a point v = anchor + sum_j c_j y_j, loses
// log2(G_ii / d_i^2) bits when v comes close to x_i.  A non-finite row poisons its own row and column of the Gram
// only (an MFMA output element reads one row of each operand).
constexpr int GR_CH = 1024;
typedef double d4v __attribute__((ext_vector_type(4)));

// The tile body that k_gram_f64 and k_hist_gram share, stated once.  gram_tile_mfma: one 16-column step of a wave, the
// T (T + 1) / 2 tile pairs in (ti, tj >= ti) order, 4 MFMAs each (q = the k index).  gram_block_partials: the fixed-order
// reduction over the block's 4 waves into its row of ``partial`` (red: the block's [4][NP * 256] LDS buffer).
template <int T>
__device__ __forceinline__ void gram_tile_mfma(const double (&x)[T][4], d4v (&acc)[T * (T + 1) / 2]) {
  int p = 0;
#pragma unroll
  for (int ti = 0; ti < T; ++ti)
#pragma unroll
    for (int tj = ti; tj < T; ++tj, ++p)
#pragma unroll
      for (int q = 0; q < 4; ++q)
        acc[p] = __builtin_amdgcn_mfma_f64_16x16x4f64(x[ti][q], x[tj][q], acc[p], 0, 0, 0);
}

template <int NP>
__device__ __forceinline__ void gram_block_partials(const d4v (&acc)[NP], double (&red)[4][NP * 256],
                                                    double* __restrict__ partial) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r16 = lane & 15, grp = lane >> 4;
#pragma unroll
  for (int p = 0; p < NP; ++p)
#pragma unroll
    for (int r = 0; r < 4; ++r) red[wave][p * 256 + (grp + 4 * r) * 16 + r16] = acc[p][r];
  __syncthreads();
  for (int e = threadIdx.x; e < NP * 256; e += 256)
    partial[(long)blockIdx.x * NP * 256 + e] = ((red[0][e] + red[1][e]) + red[2][e]) + red[3][e];
}

template <int T>
__global__ void __launch_bounds__(256) k_gram_f64(const float* __restrict__ G, int K, long P,
                                                  const int* __restrict__ centre, double* __restrict__ partial,
                                                  const float* __restrict__ anchor) {
  constexpr int NP = T * (T + 1) / 2;
  int crow = 0;  // pass 1 (centre == nullptr): row 0; pass 2: the picked row, nothing to do when that is row 0
  if (centre != nullptr) {
    crow = *centre;
    if (crow <= 0 || crow >= K) return;  // (block-uniform)
  }
  const float* Gc = anchor != nullptr ? anchor : G + (long)crow * P;  // (an anchor comes with centre == nullptr)
  __shared__ double red[4][NP * 256];  // NP <= 10 tile pairs x 16 x 16
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r16 = lane & 15, grp = lane >> 4;
  d4v acc[NP];
#pragma unroll
  for (int p = 0; p < NP; ++p) acc[p] = d4v{0.0, 0.0, 0.0, 0.0};
  const long c_begin = (long)blockIdx.x * GR_CH + wave * (GR_CH / 4);
  for (int st = 0; st < GR_CH / 4 / 16; ++st) {
    const long c0 = c_begin + st * 16 + grp * 4;
    double x[T][4];
    double ctr[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) ctr[q] = c0 + q < P ? (double)Gc[c0 + q] : 0.0;  // the centre row
#pragma unroll
    for (int t = 0; t < T; ++t) {
      const int row = t * 16 + r16;
#pragma unroll
      for (int q = 0; q < 4; ++q)
        x[t][q] = (row < K && c0 + q < P) ? (double)G[(long)row * P + c0 + q] - ctr[q] : 0.0;
    }
    gram_tile_mfma<T>(x, acc);
  }
  gram_block_partials<NP>(acc, red, partial);
}

// FoolsGold's history pass (rule text in docs/PARITY.md): H_new = H_old + (U - g) in fp32, the difference rounded
// first and the sum second (no multiply, so nothing to contract: the bits of torch's H + (U - g[None])), written to a
// second buffer, and the Gram partials of H_new in the same sweep.  The walk is k_gram_f64's with an anchor: every
// (row, column) is loaded by exactly one lane of one block, which is also its one writer, and the MFMA operand is
// (double)H_new, what k_gram_f64 forms from H_new about a zero anchor, so after k_gram_reduce the Gram is bit-equal to
// afl_gram_anchored(H_new, zeros).  *enable == 0 (a failed round, decided on the device): H_new takes the bits of H_old,
// selected, not added to zero, and a faulted row's NaN never reaches the history.
template <int T>
__global__ void __launch_bounds__(256) k_hist_gram(const float* __restrict__ U, const float* __restrict__ g,
                                                   const float* __restrict__ Hold, float* __restrict__ Hnew, int K,
                                                   long P, const int* __restrict__ enable,
                                                   double* __restrict__ partial) {
  constexpr int NP = T * (T + 1) / 2;
  __shared__ double red[4][NP * 256];
  const bool en = enable == nullptr || *enable != 0;  // (block-uniform)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r16 = lane & 15, grp = lane >> 4;
  d4v acc[NP];
#pragma unroll
  for (int p = 0; p < NP; ++p) acc[p] = d4v{0.0, 0.0, 0.0, 0.0};
  const long c_begin = (long)blockIdx.x * GR_CH + wave * (GR_CH / 4);
  for (int st = 0; st < GR_CH / 4 / 16; ++st) {
    const long c0 = c_begin + st * 16 + grp * 4;
    double x[T][4];
    float ctr[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) ctr[q] = c0 + q < P ? g[c0 + q] : 0.f;
#pragma unroll
    for (int t = 0; t < T; ++t) {
      const int row = t * 16 + r16;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        x[t][q] = 0.0;
        if (row < K && c0 + q < P) {
          const long e = (long)row * P + c0 + q;
          const float h = Hold[e];
          const float d = U[e] - ctr[q];
          const float hn = en ? h + d : h;
          Hnew[e] = hn;
          x[t][q] = (double)hn;
        }
      }
    }
    gram_tile_mfma<T>(x, acc);
  }
  gram_block_partials<NP>(acc, red, partial);
}

// The centre of pass 2 from pass 1's distances (the end of pass 1's k_gram_reduce, after D1 is formed): the row closest to
// the bulk, c* = argmin_i lowermedian_{j != i} D1[i][j] (sorted position (K - 2) / 2 of the K - 1 values), ties to the
// lowest index — except that row 0 stays the centre while its own median is within GR_KEEP0 times the smallest one:
// it is then a typical row and pass 2 has nothing to do.  Why pass 1 is good enough then: with m0, mc the medians of
// row 0 and of c*, each row has more than (K - 2) / 2 others within its median, so the two sets share a row j (or one
// of 0, c* lies in the other's set) and sqrt(D_0c) <= sqrt(m0) + sqrt(mc) <= (sqrt(GR_KEEP0) + 1) sqrt(mc) = 3 sqrt(mc).
// By the triangle inequality every row's length centred on row 0 is |x_i| <= sqrt(D_ci) + 3 sqrt(mc): the error
// model's |x_i|^2 grow from D_ci to at most 2 D_ci + 18 mc, a constant factor for rows of the bulk and less for far
// ones.  Row i of D1 sits in LDS (row stride K_max + 1); its median is found by rank counting (ties ranked by
// column, so exactly one column has the wanted rank), the K columns of a row split over the block's four waves:
// K^2 / 4 LDS reads per thread, about 1 k at K = 64, on every call (timings: profiles/bench_agg_edges.md); the argmin
// is a butterfly on (median, index) in the first wave, read from lane 0.
// NaN / inf rows (a faulted client).  Pass 1 always centres on row 0: if that row is not finite every Gram entry is
// NaN, the clamp below turns all of D into zeros, no row is eligible, the word stays 0 and the result is what a
// one-pass run gives (all zeros).  A non-finite row k != 0 has D[k][*] = 0 after the clamp in either pass; it is never
// picked as PASS 2's centre (its own Gram entry is not finite) and its column is left out of the medians (+inf), so
// the other rows' distances stay as accurate as without it.  The word is always in [0, K), and a function of D1 alone.
constexpr int GR_MAXK = 64, GR_LD = GR_MAXK + 1;
constexpr double GR_KEEP0 = 4.0;
__device__ __forceinline__ bool gram_finite(double g) { return g == g && fabs(g) < INFINITY; }

// every thread of the 256-thread block: row i = thread & 63 ranks the columns j = thread >> 6, + 4, ... (exactly one
// column of a row has the wanted rank, so medv[i] has one writer); the first wave then takes the argmin
__device__ void gram_pick_centre(const double* __restrict__ V, double* __restrict__ medv,
                                 const double* __restrict__ gram, int K, int* __restrict__ centre) {
  const int i = threadIdx.x & 63;
  const bool mine = i < K && gram_finite(gram[i * K + i]);
  if (mine) {
    const double* v = V + i * GR_LD;
    const int target = (K - 2) / 2;
    for (int j = threadIdx.x >> 6; j < K; j += 4) {
      if (j == i) continue;
      const double x = v[j];
      int rank = 0;
#pragma unroll 8
      for (int l = 0; l < K; ++l) rank += (l != i && (v[l] < x || (v[l] == x && l < j))) ? 1 : 0;
      if (rank == target) medv[i] = x;
    }
  }
  __syncthreads();
  if (threadIdx.x >= 64) return;
  const double med = mine ? medv[i] : INFINITY;
  const double med0 = __shfl(med, 0, 64);
  int bi = mine ? i : 64;
  double bs = med;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double os = __shfl_xor(bs, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    const bool take = oi < 64 && (bi >= 64 || os < bs || (os == bs && oi < bi));
    bs = take ? os : bs;
    bi = take ? oi : bi;
  }
  bi = __shfl(bi, 0, 64);
  bs = __shfl(bs, 0, 64);
  if (i == 0) *centre = (bi > 0 && bi < K && !(med0 <= GR_KEEP0 * bs)) ? bi : 0;
}

// sum the block partials in block order, then D2 = g_ii + g_jj - 2 g_ij (clamped at 0), symmetric, zero diagonal.
// Pass 1 (centre == nullptr) then picks pass 2's centre into *pick (when given); pass 2 (centre as in k_gram_f64)
// returns at once when the picked row is row 0.  D == nullptr (the anchored Gram): the Gram alone.
__global__ void __launch_bounds__(256) k_gram_reduce(const double* __restrict__ partial, int nb, int K, int T,
                                                     const int* __restrict__ centre, double* __restrict__ gram,
                                                     double* __restrict__ D, int* __restrict__ pick) {
  __shared__ double V[GR_MAXK * GR_LD], medv[GR_MAXK];
  if (centre != nullptr) {
    const int crow = *centre;
    if (crow <= 0 || crow >= K) return;
  }
  const int NP = T * (T + 1) / 2;
  for (int e = threadIdx.x; e < NP * 256; e += 256) {
    double a = 0.0;
    for (int b = 0; b < nb; ++b) a += partial[(long)b * NP * 256 + e];
    // tile pair index -> (ti, tj)
    int p = e >> 8, ti = 0;
    while (p >= T - ti) { p -= T - ti; ++ti; }
    const int tj = ti + p;
    const int i = ti * 16 + ((e & 255) >> 4), j = tj * 16 + (e & 15);
    if (i < K && j < K) {
      gram[i * K + j] = a;
      gram[j * K + i] = a;
    }
  }
  if (D == nullptr) return;  // (uniform)
  __syncthreads();
  for (int e = threadIdx.x; e < K * K; e += 256) {
    const int i = e / K, j = e % K;
    const double gjj = gram[j * K + j];
    double d = i == j ? 0.0 : gram[i * K + i] + gjj - 2.0 * gram[i * K + j];
    d = d > 0.0 ? d : 0.0;
    D[e] = d;
    V[i * GR_LD + j] = gram_finite(gjj) ? d : INFINITY;
  }
  if (pick == nullptr) return;
  if (threadIdx.x < GR_MAXK) medv[threadIdx.x] = INFINITY;
  __syncthreads();
  gram_pick_centre(V, medv, gram, K, pick);
}

// scratch (doubles): the block partials, one word for the picked centre, the K x K Gram of the final centre (tail)
int afl_gram_partials(int K, long P) {
  const int T = (K + 15) / 16;
  return afl_cdiv(P, GR_CH) * T * (T + 1) / 2 * 256 + 1 + K * K;
}

// launch(std::integral_constant<int, T>) for the K <= GR_MAXK rows' tile count T: where a Gram kernel's variant is chosen
template <class Launch>
static void gram_for_tiles(int K, Launch&& launch) {
  switch ((K + 15) / 16) {
    case 1: launch(std::integral_constant<int, 1>{}); break;
    case 2: launch(std::integral_constant<int, 2>{}); break;
    case 3: launch(std::integral_constant<int, 3>{}); break;
    default: launch(std::integral_constant<int, 4>{}); break;
  }
}

static void gram_pass(const float* G, int K, long P, const int* centre, double* partial, double* gram, double* D,
                      int* pick, hipStream_t s, const float* anchor = nullptr) {
  const int nb = afl_cdiv(P, GR_CH);
  gram_for_tiles(K, [&](auto t) {
    hipLaunchKernelGGL(k_gram_f64<decltype(t)::value>, dim3(nb), dim3(256), 0, s, G, K, P, centre, partial, anchor);
  });
  hipLaunchKernelGGL(k_gram_reduce, dim3(1), dim3(256), 0, s, partial, nb, K, (K + 15) / 16, centre, gram, D, pick);
}

int afl_pair_sqdist_gram(const float* G, int K, long P, double* partial, double* D, hipStream_t s) {
  if (K < 1 || K > GR_MAXK || P < 1) return (int)hipErrorInvalidValue;
  double* gram = partial + afl_gram_partials(K, P) - K * K;  // (the scratch: partials, the centre word, the Gram)
  int* centre = (int*)(gram - 1);
  // (K <= 2: every row is as central as row 0, one pass)
  gram_pass(G, K, P, nullptr, partial, gram, D, K > 2 ? centre : nullptr, s);
  if (K > 2) gram_pass(G, K, P, centre, partial, gram, D, nullptr, s);
  return (int)hipGetLastError();
}

// the raw Gram of the rows about an external centre: gram[i][j] = <U_i - anchor, U_j - anchor>, one pass; ``partial``
// as for afl_pair_sqdist_gram (afl_gram_partials doubles cover it)
int afl_gram_anchored(const float* U, int K, long P, const float* anchor, double* partial, double* gram,
                      hipStream_t s) {
  if (K < 1 || K > GR_MAXK || P < 1 || anchor == nullptr) return (int)hipErrorInvalidValue;
  gram_pass(U, K, P, nullptr, partial, gram, nullptr, nullptr, s, anchor);
  return (int)hipGetLastError();
}

// FoolsGold's history update and the Gram of the new history: k_hist_gram, then the Gram pass's own k_gram_reduce.
// Hnew is a second buffer ([K][P], not Hold: the caller keeps the old history until the round is known to have
// succeeded); ``partial``: afl_gram_partials(K, P) doubles; ``enable``: a device word or nullptr (= 1).
int afl_hist_gram(const float* U, const float* g, const float* Hold, float* Hnew, int K, long P, const int* enable,
                  double* partial, double* gram, hipStream_t s) {
  if (K < 1 || K > GR_MAXK || P < 1 || U == nullptr || g == nullptr || Hold == nullptr || Hnew == nullptr ||
      Hold == Hnew)
    return (int)hipErrorInvalidValue;
  const int nb = afl_cdiv(P, GR_CH);
  gram_for_tiles(K, [&](auto t) {
    hipLaunchKernelGGL(k_hist_gram<decltype(t)::value>, dim3(nb), dim3(256), 0, s, U, g, Hold, Hnew, K, P, enable,
                       partial);
  });
  hipLaunchKernelGGL(k_gram_reduce, dim3(1), dim3(256), 0, s, partial, nb, K, (K + 15) / 16, nullptr, gram, nullptr,
                     nullptr);
  return (int)hipGetLastError();
}

// ============================================================================ Philox noise (Random attack)
// out = own + sigma * N(0, 1) (reference create_random_base_model, src/Utils.py:52-57).  Philox4x32-10
// (Salmon et al., SC'11) keyed by the 64-bit seed, counter = (element group, 0, 0, 0): one call gives 4
// uniforms for 4 consecutive elements, turned into normals by Box-Muller (2 pairs).  Stateless and
// deterministic: the same (seed, P) always yields the same noise, on any rank.  The Python mirror
// (ops/composite.py:philox_normal) reproduces the uniforms bit for bit.
__device__ __forceinline__ void philox_round(uint32_t& c0, uint32_t& c1, uint32_t& c2, uint32_t& c3, uint32_t k0,
                                             uint32_t k1) {
  const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
  const uint32_t h0 = (uint32_t)(p0 >> 32), l0 = (uint32_t)p0, h1 = (uint32_t)(p1 >> 32), l1 = (uint32_t)p1;
  const uint32_t n0 = h1 ^ c1 ^ k0, n2 = h0 ^ c3 ^ k1;
  c0 = n0;
  c1 = l1;
  c2 = n2;
  c3 = l0;
}

__global__ void __launch_bounds__(256) k_noise_philox(const float* __restrict__ own, float* __restrict__ out, long P,
                                                      float sigma, uint32_t k0, uint32_t k1) {
  const long g = (long)blockIdx.x * blockDim.x + threadIdx.x;  // element group of 4
  if (g * 4 >= P) return;
  uint32_t c0 = (uint32_t)g, c1 = (uint32_t)(g >> 32), c2 = 0, c3 = 0, a = k0, b = k1;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    philox_round(c0, c1, c2, c3, a, b);
    a += 0x9E3779B9u;
    b += 0xBB67AE85u;
  }
  // uniforms in (0, 1]: (x + 1) * 2^-32 in fp64 then Box-Muller in fp64 (no log(0); one rounding at the end)
  const double u0 = ((double)c0 + 1.0) * 2.3283064365386963e-10, u1 = ((double)c1 + 1.0) * 2.3283064365386963e-10;
  const double u2 = ((double)c2 + 1.0) * 2.3283064365386963e-10, u3 = ((double)c3 + 1.0) * 2.3283064365386963e-10;
  const double r0 = sqrt(-2.0 * log(u0)), r1 = sqrt(-2.0 * log(u2));
  const double t0 = 6.283185307179586 * u1, t1 = 6.283185307179586 * u3;
  const double z[4] = {r0 * cos(t0), r0 * sin(t0), r1 * cos(t1), r1 * sin(t1)};
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const long i = g * 4 + q;
    if (i < P) out[i] = own[i] + sigma * (float)z[q];
  }
}

void afl_noise_philox(const float* own, float* out, long P, float sigma, uint64_t seed, hipStream_t s) {
  hipLaunchKernelGGL(k_noise_philox, dim3(afl_cdiv(afl_cdiv(P, 4), 256)), dim3(256), 0, s, own, out, P, sigma,
                     (uint32_t)seed, (uint32_t)(seed >> 32));
}

// ============================================================================ segmented reductions
// tiles[t] = (segment, start, end).  Pass 1: block (t, row) -> partial[t][row][q].  Pass 2:
// per (row, segment) sum of its tiles in order.
//   mode 0 (sqsum):   q0 = sum x^2                       X = diffs [M, P]
//   mode 1 (coeffs):  row < K: q0 = sum (m-g)^2, q1 = sum (m-g)*d ; row == K: q0 = sum d^2
__global__ void __launch_bounds__(256) k_seg_pass1(int mode, const float* __restrict__ X, long P, int rows,
                                                   const float* __restrict__ mean, const float* __restrict__ dev,
                                                   const int* __restrict__ tiles, double* __restrict__ partial) {
  __shared__ double scratch[8];
  const int t = blockIdx.x, r = blockIdx.y;
  const int st = tiles[3 * t + 1], en = tiles[3 * t + 2];
  double q0 = 0.0, q1 = 0.0;
  if (mode == 0) {
    const float* x = X + (long)r * P;
    for (int c = st + threadIdx.x; c < en; c += blockDim.x) {
      float v = x[c];
      q0 += (double)v * v;
    }
  } else if (r < rows - 1) {
    const float* g = X + (long)r * P;
    for (int c = st + threadIdx.x; c < en; c += blockDim.x) {
      double a = (double)mean[c] - (double)g[c];
      q0 += a * a;
      q1 += a * (double)dev[c];
    }
  } else {
    for (int c = st + threadIdx.x; c < en; c += blockDim.x) {
      double d = dev[c];
      q0 += d * d;
    }
  }
  q0 = block_sum(q0, scratch);
  q1 = block_sum(q1, scratch);
  if (threadIdx.x == 0) {
    partial[((long)t * rows + r) * 2 + 0] = q0;
    partial[((long)t * rows + r) * 2 + 1] = q1;
  }
}

__global__ void k_seg_pass2(const double* __restrict__ partial, const int* __restrict__ segf, int rows, int S,
                            double* __restrict__ out0, double* __restrict__ out1) {
  int id = blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= rows * S) return;
  int r = id / S, sg = id % S;
  double a = 0.0, b = 0.0;
  for (int t = segf[sg]; t < segf[sg + 1]; ++t) {
    a += partial[((long)t * rows + r) * 2 + 0];
    b += partial[((long)t * rows + r) * 2 + 1];
  }
  out0[(long)r * S + sg] = a;
  if (out1) out1[(long)r * S + sg] = b;
}

void afl_seg_reduce(int mode, const float* X, long P, int rows, const float* mean, const float* dev, const int* tiles,
                    int T, const int* segf, int S, double* partial, double* out0, double* out1, hipStream_t s) {
  hipLaunchKernelGGL(k_seg_pass1, dim3(T, rows), dim3(256), 0, s, mode, X, P, rows, mean, dev, tiles, partial);
  hipLaunchKernelGGL(k_seg_pass2, dim3(afl_cdiv((long)rows * S, 256)), dim3(256), 0, s, partial, segf, rows, S, out0,
                     out1);
}

// ============================================================================ coordinate select
// Each thread owns one column: N values in registers, odd-even transposition sort network with
// compile-time indices (NMAX template; padding +inf), then lower-median or trimmed mean.
// NaN (the engine marks a faulted client's row with it) follows the composites: torch.median returns NaN for a
// column that holds one; torch.sort places NaN last, so the trimmed mean is NaN when the column holds more NaNs
// than ``trim`` and the mean of the real values at [trim, N - trim) otherwise.  The column's NaNs are counted
// while loading; the sort moves them behind everything, the +inf padding included, so with at most ``trim`` of
// them the summed positions hold real values.
template <int NMAX>
__global__ void __launch_bounds__(256) k_coord_select(const float* __restrict__ U, int N, long P, int mode, int trim,
                                                      float* __restrict__ out) {
  long c = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= P) return;
  float v[NMAX];
  int nnan = 0;
#pragma unroll
  for (int i = 0; i < NMAX; ++i) {
    v[i] = i < N ? U[(long)i * P + c] : __int_as_float(0x7f800000);
    nnan += v[i] != v[i] ? 1 : 0;
  }
#pragma unroll
  for (int r = 0; r < NMAX; ++r) {
#pragma unroll
    for (int i = (r & 1); i + 1 < NMAX; i += 2) {
      float a = v[i], b = v[i + 1];
      // NaN-aware: a NaN is treated as the largest value (behind the +inf padding)
      bool sw = (a > b) || (a != a && b == b);
      v[i] = sw ? b : a;
      v[i + 1] = sw ? a : b;
    }
  }
  float r = 0.f;
  if (mode == 0) {
    const int mid = (N - 1) / 2;
#pragma unroll
    for (int i = 0; i < NMAX; ++i) r = (i == mid) ? v[i] : r;
    if (nnan > 0) r = __int_as_float(0x7fc00000);
  } else {
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < NMAX; ++i) acc += (i >= trim && i < N - trim) ? v[i] : 0.f;
    r = nnan > trim ? __int_as_float(0x7fc00000) : acc / (float)(N - 2 * trim);
  }
  out[c] = r;
}

void afl_coord_select(const float* U, int N, long P, int mode, int trim, float* out, hipStream_t s) {
  dim3 g(afl_cdiv(P, 256)), b(256);
  if (N <= 8) hipLaunchKernelGGL(k_coord_select<8>, g, b, 0, s, U, N, P, mode, trim, out);
  else if (N <= 16) hipLaunchKernelGGL(k_coord_select<16>, g, b, 0, s, U, N, P, mode, trim, out);
  else if (N <= 32) hipLaunchKernelGGL(k_coord_select<32>, g, b, 0, s, U, N, P, mode, trim, out);
  else hipLaunchKernelGGL(k_coord_select<64>, g, b, 0, s, U, N, P, mode, trim, out);
}

// ============================================================================ row dots
constexpr int RD_CH = 8192;
__global__ void __launch_bounds__(256) k_row_dots(const float* __restrict__ U, const float* __restrict__ ref, long P,
                                                  int mode, double* __restrict__ partial) {
  __shared__ double scratch[8];
  const int ch = blockIdx.x, r = blockIdx.y;
  const long st = (long)ch * RD_CH, en = min(P, st + RD_CH);
  const float* u = U + (long)r * P;
  double uu = 0, ur = 0, rr = 0;
  for (long c = st + threadIdx.x; c < en; c += blockDim.x) {
    double a = u[c];
    uu += a * a;
    if (mode) {
      double b = ref[c];
      ur += a * b;
      rr += b * b;
    }
  }
  uu = block_sum(uu, scratch);
  ur = block_sum(ur, scratch);
  rr = block_sum(rr, scratch);
  if (threadIdx.x == 0) {
    double* p = partial + ((long)r * gridDim.x + ch) * 3;
    p[0] = uu;
    p[1] = ur;
    p[2] = rr;
  }
}

__global__ void k_row_dots_reduce(const double* __restrict__ partial, int N, int nch, double* __restrict__ out) {
  int id = blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= N * 3) return;
  int r = id / 3, q = id % 3;
  double a = 0;
  for (int c = 0; c < nch; ++c) a += partial[((long)r * nch + c) * 3 + q];
  out[r * 3 + q] = a;
}

int afl_row_dots_nchunks(long P) { return afl_cdiv(P, RD_CH); }

void afl_row_dots(const float* U, const float* ref, int N, long P, int mode, double* partial, double* out,
                  hipStream_t s) {
  int nch = afl_cdiv(P, RD_CH);
  hipLaunchKernelGGL(k_row_dots, dim3(nch, N), dim3(256), 0, s, U, ref, P, mode, partial);
  hipLaunchKernelGGL(k_row_dots_reduce, dim3(afl_cdiv(N * 3, 256)), dim3(256), 0, s, partial, N, nch, out);
}

// ============================================================================ ScionFL quantisation
// Row min / max over SQ_NB chunks per row (one workgroup per row kept 8 CUs busy for 49 us at 8 x 47.7 k), the
// chunk partials reduced by the quantisation kernel's blocks themselves (min / max: any order gives the same
// values, so the bits are those of the one-pass form).
constexpr int SQ_NB = 32;
__global__ void __launch_bounds__(256) k_row_minmax(const float* __restrict__ U, long P, float* __restrict__ part) {
  __shared__ float smn[4], smx[4];
  const int r = blockIdx.y, b = blockIdx.x;
  const long c0 = P * b / SQ_NB, c1 = P * (b + 1) / SQ_NB;
  const float* u = U + (long)r * P;
  float mn = __int_as_float(0x7f800000), mx = -mn;
  for (long c = c0 + threadIdx.x; c < c1; c += blockDim.x) {
    const float a = u[c];
    mn = fminf(mn, a);
    mx = fmaxf(mx, a);
  }
  mn = wave_min(mn);
  mx = wave_max(mx);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) {
    smn[w] = mn;
    smx[w] = mx;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < 4; ++i) {
      mn = fminf(mn, smn[i]);
      mx = fmaxf(mx, smx[i]);
    }
    part[((long)r * SQ_NB + b) * 2] = mn;
    part[((long)r * SQ_NB + b) * 2 + 1] = mx;
  }
}

__global__ void __launch_bounds__(256) k_stoch_quant(const float* __restrict__ U, long P, long total,
                                                     const float* __restrict__ part, float* __restrict__ smin,
                                                     float* __restrict__ smax, uint64_t seed,
                                                     float* __restrict__ sigma) {
  __shared__ float lo_s[2], hi_s[2];
  const long id0 = (long)blockIdx.x * blockDim.x;
  const long r0 = id0 / P;  // a block spans at most two rows (P >= 256) or several (P < 256: handled per row)
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (w < 2) {  // wave w reduces the partials of row r0 + w
    const long r = r0 + w;
    const long nrows = total / P;
    float mn = __int_as_float(0x7f800000), mx = -mn;
    if (r < nrows && lane < SQ_NB) {
      mn = part[(r * SQ_NB + lane) * 2];
      mx = part[(r * SQ_NB + lane) * 2 + 1];
    }
    mn = wave_min(mn);
    mx = wave_max(mx);
    if (lane == 0) {
      lo_s[w] = mn;
      hi_s[w] = mx;
    }
  }
  __syncthreads();
  const long id = id0 + threadIdx.x;
  if (id >= total) return;
  const long r = id / P;
  float lo, hi;
  if (r - r0 < 2) {
    lo = lo_s[r - r0];
    hi = hi_s[r - r0];
  } else {  // (rows shorter than a block: reduce this row's partials directly)
    lo = __int_as_float(0x7f800000);
    hi = -lo;
    for (int b = 0; b < SQ_NB; ++b) {
      lo = fminf(lo, part[(r * SQ_NB + b) * 2]);
      hi = fmaxf(hi, part[(r * SQ_NB + b) * 2 + 1]);
    }
  }
  if (id == r * P) {  // the row's first element publishes its min / max
    smin[r] = lo;
    smax[r] = hi;
  }
  const float p = (U[id] - lo) / (hi - lo + 1e-6f);
  sigma[id] = afl_uniform(seed, (uint64_t)id) < p ? 1.f : 0.f;
}

long afl_stoch_quant_ws(int N) { return (long)N * SQ_NB * 2; }

void afl_stoch_quant(const float* U, int N, long P, uint64_t seed, float* sigma, float* smin, float* smax,
                     float* ws, hipStream_t s) {
  hipLaunchKernelGGL(k_row_minmax, dim3(SQ_NB, N), dim3(256), 0, s, U, P, ws);
  const long total = (long)N * P;
  hipLaunchKernelGGL(k_stoch_quant, dim3(afl_cdiv(total, 256)), dim3(256), 0, s, U, P, total, ws, smin, smax, seed,
                     sigma);
}

// ============================================================================ Adam (flat)
// torch.optim.Adam (foreach=False) math: m <- m + (1-b1)(g-m); v <- b2 v + (1-b2) g^2;
// p <- p - (lr/bc1) * m / (sqrt(v)/sqrt(bc2) + eps).  `gscale` folds in a clip coefficient.
__global__ void __launch_bounds__(256) k_adam_flat(float* __restrict__ p, const float* __restrict__ g,
                                                   float* __restrict__ m, float* __restrict__ v, long n, float lr_bc1,
                                                   float rsqrt_bc2, float b1, float b2, float eps, float gscale) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float gi = g[i] * gscale;
  float mi = m[i] + (1.f - b1) * (gi - m[i]);
  float vi = b2 * v[i] + (1.f - b2) * gi * gi;
  m[i] = mi;
  v[i] = vi;
  p[i] -= lr_bc1 * mi / (sqrtf(vi) * rsqrt_bc2 + eps);
}

void afl_adam_flat(float* p, const float* g, float* m, float* v, long n, int step, float lr, float b1, float b2,
                   float eps, float gscale, hipStream_t s) {
  double bc1 = 1.0 - pow((double)b1, step), bc2 = 1.0 - pow((double)b2, step);
  hipLaunchKernelGGL(k_adam_flat, dim3(afl_cdiv(n, 256)), dim3(256), 0, s, p, g, m, v, n, (float)(lr / bc1),
                     (float)(1.0 / sqrt(bc2)), b1, b2, eps, gscale);
}

// ============================================================================ gmm_filter
// GMM gradient filter (reference server.py:352-370, src/Utils.py:257-323), all decisions on the device so the
// round needs no host round trip: input the centred Gram matrix G = Xc Xc^T [n][n] (fp64) of the client updates.
//   1. PCA scores in r dims (rank > 0: min(rank, 4, n); 0: max(1, min(4, n/2 - 1))): cyclic Jacobi eigen-decomposition of G (12 sweeps),
//      eigenvalues in descending order, Z = V_r sqrt(lambda_r), scaled by 1 / max |Z|;
//   2. rows ordered benign then malicious (train_gmm_model's vstack), a 2-component full-covariance GMM
//      (reg_covar 1e-6, tol 1e-3, <= 100 EM iterations, sklearn's M / E steps) initialised by a deterministic
//      k-means (centres: row 0 and the row farthest from it, 10 Lloyd iterations) — sklearn's k-means++ init
//      draws from an unseeded RNG in the reference, so any fixed init is one of its possible runs;
//   3. threshold = 3 x population std of the benign rows' Mahalanobis distances to component 0; a row is kept
//      when its distance to its most probable component is <= threshold.
// One wave: the Jacobi rotations are applied by lane k to row / column k, the E-step and the decisions run one lane
// per row, every sum stays on lane 0 in row order; agg.gmm_filter_ref in Python is the bit-level mirror.
constexpr int GMM_MAXN = 64, GMM_R = 4;

__device__ __host__ inline bool gmm_chol(const double (&S)[GMM_R][GMM_R], int r, double (&Lc)[GMM_R][GMM_R]) {
  for (int i = 0; i < r; ++i)
    for (int j = 0; j <= i; ++j) {
      double s = S[i][j];
      for (int k = 0; k < j; ++k) s -= Lc[i][k] * Lc[j][k];
      if (i == j) {
        if (!(s > 0.0)) return false;
        Lc[i][i] = sqrt(s);
      } else {
        Lc[i][j] = s / Lc[j][j];
      }
    }
  return true;
}
// squared Mahalanobis distance through the Cholesky factor (forward substitution)
__device__ __host__ inline double gmm_md2(const double (&Lc)[GMM_R][GMM_R], int r, const double* x, const double* mu) {
  double y[GMM_R], s = 0.0;
  for (int i = 0; i < r; ++i) {
    double v = x[i] - mu[i];
    for (int k = 0; k < i; ++k) v -= Lc[i][k] * y[k];
    y[i] = v / Lc[i][i];
    s += y[i] * y[i];
  }
  return s;
}

__global__ void __launch_bounds__(64) k_gmm_filter(const double* __restrict__ G, int n, const unsigned char* __restrict__ att,
                                                   unsigned char* __restrict__ keep, double* __restrict__ info, int rank) {
  __shared__ double A[GMM_MAXN * GMM_MAXN], V[GMM_MAXN * GMM_MAXN], Z[GMM_MAXN * GMM_R], X[GMM_MAXN * GMM_R];
  __shared__ double resp[GMM_MAXN * 2], ev[GMM_MAXN];
  __shared__ int ord[GMM_MAXN], evi[GMM_MAXN];
  for (int e = threadIdx.x; e < n * n; e += blockDim.x) {
    A[e] = G[e];
    V[e] = (e / n == e % n) ? 1.0 : 0.0;
  }
  __syncthreads();
  // ---- 1. Jacobi eigen-decomposition (cyclic sweeps, fixed count): every lane derives the rotation, lane k applies
  //      it to row / column k (the same element operations in the same order as the single-lane form and the host
  //      mirror; one lane walking the n^2 updates serially through LDS took ~0.6 ms for n = 8)
  const int k = threadIdx.x;
  for (int sweep = 0; sweep < 12; ++sweep)
    for (int p = 0; p < n - 1; ++p)
      for (int q = p + 1; q < n; ++q) {
        const double apq = A[p * n + q];
        if (fabs(apq) < 1e-300) continue;  // (uniform: every lane read the same word)
        const double th = (A[q * n + q] - A[p * n + p]) / (2.0 * apq);
        const double t = (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        __syncthreads();  // every lane has read A[p][p], A[q][q], A[p][q] before they change
        if (k < n) {  // columns p, q
          const double akp = A[k * n + p], akq = A[k * n + q];
          A[k * n + p] = c * akp - s * akq;
          A[k * n + q] = s * akp + c * akq;
        }
        __syncthreads();
        if (k < n) {  // rows p, q; eigenvectors
          const double apk = A[p * n + k], aqk = A[q * n + k];
          A[p * n + k] = c * apk - s * aqk;
          A[q * n + k] = s * apk + c * aqk;
          const double vkp = V[k * n + p], vkq = V[k * n + q];
          V[k * n + p] = c * vkp - s * vkq;
          V[k * n + q] = s * vkp + c * vkq;
        }
        __syncthreads();
      }
  // ---- the rest: one lane, except the E-step and the decisions (lane i = row i; the sums stay on lane 0 in row
  //      order, so every value equals the single-lane form's and the host mirror's)
  __shared__ double mu[2][GMM_R], w[2], cov[2][GMM_R][GMM_R], Lc[2][GMM_R][GMM_R], logdet[2], lse_row[GMM_MAXN];
  __shared__ int sh_r, sh_m, sh_nb, sh_K, sh_okc, sh_stop;
  __shared__ double sh_thr;
  if (k == 0) {
    for (int i = 0; i < n; ++i) {
      ev[i] = A[i * n + i];
      evi[i] = i;
    }
    for (int i = 1; i < n; ++i) {  // stable insertion sort, descending
      const double v = ev[i];
      const int ix = evi[i];
      int j = i - 1;
      while (j >= 0 && ev[j] < v) {
        ev[j + 1] = ev[j];
        evi[j + 1] = evi[j];
        --j;
      }
      ev[j + 1] = v;
      evi[j + 1] = ix;
    }
    const int r = rank > 0 ? min(min(rank, GMM_R), n) : max(1, min(GMM_R, n / 2 - 1));
    double zmax = 0.0;
    for (int i = 0; i < n; ++i)
      for (int kk = 0; kk < r; ++kk) {
        const double z = V[i * n + evi[kk]] * sqrt(fmax(ev[kk], 1e-30));
        Z[i * GMM_R + kk] = z;
        zmax = fmax(zmax, fabs(z));
      }
    zmax = fmax(zmax, 1e-30);
    int m = 0;
    for (int i = 0; i < n; ++i)
      if (!att[i]) ord[m++] = i;
    const int nb = m;
    for (int i = 0; i < n; ++i)
      if (att[i]) ord[m++] = i;
    for (int i = 0; i < n; ++i)
      for (int kk = 0; kk < r; ++kk) Z[i * GMM_R + kk] /= zmax;
    for (int i = 0; i < m; ++i)
      for (int kk = 0; kk < r; ++kk) X[i * GMM_R + kk] = Z[ord[i] * GMM_R + kk];
    const int K = m >= 2 ? 2 : 1;
    // ---- 2a. deterministic k-means initialisation
    for (int kk = 0; kk < r; ++kk) mu[0][kk] = mu[1][kk] = X[kk];
    if (K == 2) {
      int far = 0;
      double best = -1.0;
      for (int i = 0; i < m; ++i) {
        double d = 0.0;
        for (int kk = 0; kk < r; ++kk) d += (X[i * GMM_R + kk] - X[kk]) * (X[i * GMM_R + kk] - X[kk]);
        if (d > best) {
          best = d;
          far = i;
        }
      }
      for (int kk = 0; kk < r; ++kk) mu[1][kk] = X[far * GMM_R + kk];
      for (int it = 0; it < 10; ++it) {
        double sm[2][GMM_R] = {}, cnt[2] = {0.0, 0.0};
        for (int i = 0; i < m; ++i) {
          double d0 = 0.0, d1 = 0.0;
          for (int kk = 0; kk < r; ++kk) {
            d0 += (X[i * GMM_R + kk] - mu[0][kk]) * (X[i * GMM_R + kk] - mu[0][kk]);
            d1 += (X[i * GMM_R + kk] - mu[1][kk]) * (X[i * GMM_R + kk] - mu[1][kk]);
          }
          const int l = d1 < d0 ? 1 : 0;
          resp[i * 2 + 0] = l == 0 ? 1.0 : 0.0;
          resp[i * 2 + 1] = l == 1 ? 1.0 : 0.0;
          cnt[l] += 1.0;
          for (int kk = 0; kk < r; ++kk) sm[l][kk] += X[i * GMM_R + kk];
        }
        for (int c = 0; c < 2; ++c)
          if (cnt[c] > 0.0)
            for (int kk = 0; kk < r; ++kk) mu[c][kk] = sm[c][kk] / cnt[c];
      }
    } else {
      for (int i = 0; i < m; ++i) {
        resp[i * 2] = 1.0;
        resp[i * 2 + 1] = 0.0;
      }
    }
    sh_r = r;
    sh_m = m;
    sh_nb = nb;
    sh_K = K;
    sh_okc = 1;
  }
  __syncthreads();
  const int r = sh_r, m = sh_m, nb = sh_nb, K = sh_K;
  // ---- 2b. EM (sklearn GaussianMixture, covariance_type "full")
  const double eps10 = 10.0 * 2.220446049250313e-16, reg = 1e-6, LOG2PI = 1.8378770664093453;
  auto mstep = [&]() {  // (lane 0)
    double nks = 0.0;
    for (int c = 0; c < K; ++c) {
      double nk = eps10;
      for (int i = 0; i < m; ++i) nk += resp[i * 2 + c];
      for (int kk = 0; kk < r; ++kk) {
        double sv = 0.0;
        for (int i = 0; i < m; ++i) sv += resp[i * 2 + c] * X[i * GMM_R + kk];
        mu[c][kk] = sv / nk;
      }
      for (int a = 0; a < r; ++a)
        for (int b = 0; b < r; ++b) {
          double sv = 0.0;
          for (int i = 0; i < m; ++i)
            sv += resp[i * 2 + c] * (X[i * GMM_R + a] - mu[c][a]) * (X[i * GMM_R + b] - mu[c][b]);
          cov[c][a][b] = sv / nk + (a == b ? reg : 0.0);
        }
      w[c] = nk;
      nks += nk;
      sh_okc = sh_okc && gmm_chol(cov[c], r, Lc[c]);
      double ld = 0.0;
      for (int kk = 0; kk < r; ++kk) ld += log(Lc[c][kk][kk]);
      logdet[c] = 2.0 * ld;
    }
    for (int c = 0; c < K; ++c) w[c] /= nks;
  };
  auto wlogp = [&](const double* x, int c) {
    return log(w[c]) - 0.5 * (r * LOG2PI + gmm_md2(Lc[c], r, x, mu[c]) + logdet[c]);
  };
  if (k == 0) {
    mstep();
    sh_stop = sh_okc ? 0 : 1;
  }
  __syncthreads();
  double lb = -INFINITY;  // (lane 0's copy is the one that decides)
  for (int it = 0; it < 100 && !sh_stop; ++it) {
    if (k < m) {  // E-step, lane k = row k
      const double* x = X + k * GMM_R;
      double lp[2] = {wlogp(x, 0), K == 2 ? wlogp(x, 1) : -INFINITY};
      const double mx = fmax(lp[0], lp[1]);
      const double lse = mx + log(exp(lp[0] - mx) + exp(lp[1] - mx));
      lse_row[k] = lse;
      resp[k * 2] = exp(lp[0] - lse);
      resp[k * 2 + 1] = K == 2 ? exp(lp[1] - lse) : 0.0;
    }
    __syncthreads();
    if (k == 0) {
      const double prev = lb;
      double tot = 0.0;
      for (int i = 0; i < m; ++i) tot += lse_row[i];
      mstep();
      lb = tot / m;
      sh_stop = (!sh_okc || fabs(lb - prev) < 1e-3) ? 1 : 0;
    }
    __syncthreads();
  }
  // ---- 3. threshold and decisions
  if (k == 0) {
    double s1 = 0.0, s2 = 0.0;
    for (int i = 0; i < nb; ++i) s1 += sqrt(gmm_md2(Lc[0], r, X + i * GMM_R, mu[0]));
    const double meanb = nb ? s1 / nb : 0.0;
    for (int i = 0; i < nb; ++i) {
      const double d = sqrt(gmm_md2(Lc[0], r, X + i * GMM_R, mu[0])) - meanb;
      s2 += d * d;
    }
    sh_thr = nb ? 3.0 * sqrt(s2 / nb) : INFINITY;
  }
  __syncthreads();
  const double thr = sh_thr;
  const bool okc = sh_okc != 0;
  if (k < n) {  // lane k = client k
    const double* x = Z + k * GMM_R;
    const int c = (K == 2 && wlogp(x, 1) > wlogp(x, 0)) ? 1 : 0;
    const bool kp = okc && sqrt(gmm_md2(Lc[c], r, x, mu[c])) <= thr;
    keep[k] = kp ? 1 : 0;
    lse_row[k] = kp ? 1.0 : 0.0;
  }
  __syncthreads();
  if (k == 0) {
    int kept = 0;
    for (int i = 0; i < n; ++i) kept += lse_row[i] > 0.5 ? 1 : 0;
    info[0] = thr;
    info[1] = (double)kept;
    info[2] = okc ? 1.0 : 0.0;
  }
}

int afl_gmm_filter(const double* G, int n, const unsigned char* att, unsigned char* keep, double* info, int rank,
                   hipStream_t s) {
  if (n < 1 || n > GMM_MAXN || rank < 0) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_gmm_filter, dim3(1), dim3(64), 0, s, G, n, att, keep, info, rank);
  return (int)hipGetLastError();
}

// ============================================================================ top_pc
// First principal-component scores of n <= 64 rows from their centred Gram G = Xc Xc^T (fp64 [n][n]), the
// FLTracer PCA(1) (reference src/Utils.py:359-369): Jacobi eigen-decomposition on one wave (at most ``sweeps``
// sweeps, fewer once the off-diagonal mass is at fp64 rounding); z = v_max sqrt(lambda_max).  Parallel (round-robin) ordering: each step rotates m / 2 DISJOINT pairs at
// once (m = n rounded up to even; m - 1 steps cover every pair once per sweep), their (c, s) computed by one lane
// each, then one lane per (pair, row / column) applies them — 7 dependent steps per sweep at n = 8 instead of 28
// sequential rotations (the rotation's fp64 divide / square-root chain and three barriers were the kernel's whole
// time: 158 us per call).  (Repeated squaring of G, the round-4 form, let the second eigenvector leak in at
// (lambda_2 / lambda_1)^(2^squarings): 2 % at a 0.999 ratio, 66 % at 0.9999 — nearly iid updates.)
// The Jacobi body, shared by k_top_pc and k_dnc_select (one 64-lane block): A [n][n] symmetric and V = I in LDS, filled
// and synchronised by the caller; on return A's diagonal holds the eigenvalues, V's columns the eigenvectors, and the
// result is the index of the largest eigenvalue (first maximum; every lane returns the same).
__device__ __forceinline__ int jacobi_top(double* __restrict__ A, double* __restrict__ V, double* __restrict__ cs_c,
                                          double* __restrict__ cs_s, int* __restrict__ cs_p, int* __restrict__ cs_q,
                                          int n, int sweeps) {
  const int k = threadIdx.x;
  const int m = n + (n & 1);  // (an odd n pairs one index with the dummy index n each step: skipped)
  const int half = m / 2;
  for (int sweep = 0; sweep < sweeps; ++sweep) {
    {  // converged to fp64 precision (off-diagonal mass <= 1e-32 of the diagonal's): the remaining rotations
       // would be identities up to rounding, so the sweep count is an upper bound (uniform decision)
      double off = 0.0, dia = 0.0;
      if (k < n) {
        dia = A[k * n + k] * A[k * n + k];
        for (int j = k + 1; j < n; ++j) off += A[k * n + j] * A[k * n + j];
      }
      for (int o = 32; o > 0; o >>= 1) {
        off += __shfl_xor(off, o, 64);
        dia += __shfl_xor(dia, o, 64);
      }
      if (off <= 1e-32 * dia) break;
    }
    for (int r = 0; r < m - 1; ++r) {
      if (k < half) {  // pair k of step r: (r, m - 1) and ((r + k) % (m - 1), (r - k + m - 1) % (m - 1))
        int p = k == 0 ? r : (r + k) % (m - 1);
        int q = k == 0 ? m - 1 : (r - k + m - 1) % (m - 1);
        if (p > q) {
          const int t = p;
          p = q;
          q = t;
        }
        double c = 1.0, sn = 0.0;
        if (q < n) {
          const double apq = A[p * n + q];
          if (fabs(apq) >= 1e-300) {
            const double th = (A[q * n + q] - A[p * n + p]) / (2.0 * apq);
            const double t = (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
            c = 1.0 / sqrt(t * t + 1.0);
            sn = t * c;
          }
        }
        cs_p[k] = p;
        cs_q[k] = q < n ? q : p;  // (identity on the dummy pair: c = 1, s = 0 on column p alone)
        cs_c[k] = c;
        cs_s[k] = sn;
      }
      __syncthreads();
      // one lane per (pair t, row / column i): every pair's rotation applied at once (disjoint pairs)
      for (int e = k; e < half * n; e += 64) {  // columns p, q
        const int t = e / n, i = e - t * n;
        const int p = cs_p[t], q = cs_q[t];
        if (p == q) continue;
        const double c = cs_c[t], sn = cs_s[t];
        const double aip = A[i * n + p], aiq = A[i * n + q];
        const double vip = V[i * n + p], viq = V[i * n + q];
        A[i * n + p] = c * aip - sn * aiq;
        A[i * n + q] = sn * aip + c * aiq;
        V[i * n + p] = c * vip - sn * viq;
        V[i * n + q] = sn * vip + c * viq;
      }
      __syncthreads();
      for (int e = k; e < half * n; e += 64) {  // rows p, q
        const int t = e / n, i = e - t * n;
        const int p = cs_p[t], q = cs_q[t];
        if (p == q) continue;
        const double c = cs_c[t], sn = cs_s[t];
        const double api = A[p * n + i], aqi = A[q * n + i];
        A[p * n + i] = c * api - sn * aqi;
        A[q * n + i] = sn * api + c * aqi;
      }
      __syncthreads();
    }
  }
  int top = 0;
  for (int i = 1; i < n; ++i)
    if (A[i * n + i] > A[top * n + top]) top = i;
  return top;
}

__global__ void __launch_bounds__(64) k_top_pc(const double* __restrict__ G, int n, int sweeps, double* __restrict__ z) {
  __shared__ double A[GMM_MAXN * GMM_MAXN], V[GMM_MAXN * GMM_MAXN];
  __shared__ double cs_c[GMM_MAXN / 2], cs_s[GMM_MAXN / 2];
  __shared__ int cs_p[GMM_MAXN / 2], cs_q[GMM_MAXN / 2];
  const int k = threadIdx.x;
  for (int e = k; e < n * n; e += blockDim.x) {
    A[e] = G[e];
    V[e] = (e / n == e % n) ? 1.0 : 0.0;
  }
  __syncthreads();
  const int top = jacobi_top(A, V, cs_c, cs_s, cs_p, cs_q, n, sweeps);
  if (k < n) z[k] = V[k * n + top] * sqrt(fmax(A[top * n + top], 0.0));
}

int afl_top_pc(const double* G, int n, int sweeps, double* z, hipStream_t s) {
  if (n < 1 || n > GMM_MAXN || sweeps < 1) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_top_pc, dim3(1), dim3(64), 0, s, G, n, sweeps, z);
  return (int)hipGetLastError();
}

// ============================================================================ DnC
// Divide-and-Conquer (Shejwalkar & Houmansadr, NDSS 2021; beyond the reference, rule text in docs/PARITY.md): for each
// of ``iters`` iterations a spectral filter on b keyed random columns.  Two launches for all iterations together.
//
// k_dnc_gram: grid (position chunks of GR_CH, iters).  Position i of iteration t is column pi_t(i) (plan_perm.h
// pl_perm with pl_dnc_keys(seed, t)), or i itself when b >= P (``natural``); positions >= nv = min(b, P) contribute
// zeros.  Each step of a wave covers 16 positions: lane l derives the column of position (l & 15) once, the four
// columns of its group come over by __shfl, and the rest is k_gram_f64 (rows centred on row 0 in fp64, the same
// MFMA / C-D layout / fixed-order cross-wave reduction) with gathered 4-byte loads.  A column index is < P by
// construction (the cycle walk ends in [0, P); nv <= P), a row index is checked against K.
template <int T>
__global__ void __launch_bounds__(256) k_dnc_gram(const float* __restrict__ G, int K, long P, long nv, int natural,
                                                  uint64_t seed, double* __restrict__ partial) {
  constexpr int NP = T * (T + 1) / 2;
  __shared__ double red[4][NP * 256];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r16 = lane & 15, grp = lane >> 4;
  const DncKeys key = pl_dnc_keys(seed, (int)blockIdx.y);
  const int half = pl_half_bits((uint32_t)P);
  d4v acc[NP];
#pragma unroll
  for (int p = 0; p < NP; ++p) acc[p] = d4v{0.0, 0.0, 0.0, 0.0};
  const long c_begin = (long)blockIdx.x * GR_CH + wave * (GR_CH / 4);
  for (int st = 0; st < GR_CH / 4 / 16; ++st) {
    if (c_begin + st * 16 >= nv) break;  // (wave-uniform: the remaining positions are all past b)
    const long pos = c_begin + st * 16 + r16;
    int mycol = -1;
    if (pos < nv) mycol = natural ? (int)pos : (int)pl_perm((uint32_t)pos, (uint32_t)P, half, key.k0, key.k1);
    int col[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) col[q] = __shfl(mycol, grp * 4 + q, 64);
    double x[T][4];
    double ctr[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) ctr[q] = col[q] >= 0 ? (double)G[col[q]] : 0.0;  // the centre row (row 0)
#pragma unroll
    for (int t = 0; t < T; ++t) {
      const int row = t * 16 + r16;
#pragma unroll
      for (int q = 0; q < 4; ++q)
        x[t][q] = (row < K && col[q] >= 0) ? (double)G[(long)row * P + col[q]] - ctr[q] : 0.0;
    }
    int p = 0;
#pragma unroll
    for (int ti = 0; ti < T; ++ti)
#pragma unroll
      for (int tj = ti; tj < T; ++tj, ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q)
          acc[p] = __builtin_amdgcn_mfma_f64_16x16x4f64(x[ti][q], x[tj][q], acc[p], 0, 0, 0);
  }
  // fixed-order reduction over the 4 waves
#pragma unroll
  for (int p = 0; p < NP; ++p)
#pragma unroll
    for (int r = 0; r < 4; ++r) red[wave][p * 256 + (grp + 4 * r) * 16 + r16] = acc[p][r];
  __syncthreads();
  double* out = partial + ((long)blockIdx.y * gridDim.x + blockIdx.x) * NP * 256;
  for (int e = threadIdx.x; e < NP * 256; e += 256) out[e] = ((red[0][e] + red[1][e]) + red[2][e]) + red[3][e];
}

int afl_dnc_nblocks(long P, long b) { return (int)afl_cdiv(b < P ? b : P, GR_CH); }

long afl_dnc_partials(int K, long P, long b, int iters) {
  const int T = (K + 15) / 16;
  return (long)iters * afl_dnc_nblocks(P, b) * (T * (T + 1) / 2) * 256;
}

int afl_dnc_gram(const float* U, int K, long P, long b, int iters, uint64_t seed, double* partial, hipStream_t s) {
  // (P < 2^31: a column index is a uint32 of the permutation's domain and an int in the kernel)
  if (K < 1 || K > GR_MAXK || P < 1 || P > 0x7FFFFFFFl || b < 1 || iters < 1 || iters > 65535)
    return (int)hipErrorInvalidValue;
  const long nv = b < P ? b : P;
  const int natural = b >= P ? 1 : 0;
  const dim3 grid((unsigned)afl_cdiv(nv, GR_CH), (unsigned)iters);
  gram_for_tiles(K, [&](auto t) {
    hipLaunchKernelGGL(k_dnc_gram<decltype(t)::value>, grid, dim3(256), 0, s, U, K, P, nv, natural, seed, partial);
  });
  return (int)hipGetLastError();
}

// k_dnc_select: one wave, looping over the iterations (the masks are ANDed in registers: lane i owns row i).  Per
// iteration: the Gram H of the rows centred on row 0 — the block partials summed in block order (nb > 0), or read as
// it is (nb = 0) —, double-centred C = H - rowmean - colmean + mean (each mean a sum in index order; skipped when
// nb = 0 and !centre) and written to gout; jacobi_top; score_i = lambda_1 u_i^2 (lambda_1 floored at 0); row i is
// dropped when fewer than ``drop`` rows have a larger (score, index), a NaN score counting as +inf — exactly ``drop``
// rows whatever the scores hold, and on an exact tie the higher index.  After the last iteration: no row kept -> every
// row kept; weights = w keep / sum (summed in index order).  Every loop has a fixed trip count (Jacobi: <= DNC_SWEEPS).
constexpr int DNC_SWEEPS = 16;

__global__ void __launch_bounds__(64) k_dnc_select(const double* __restrict__ src, int nb, int n, int iters, int centre,
                                                   int drop, const double* __restrict__ w,
                                                   unsigned char* __restrict__ keep, double* __restrict__ scores,
                                                   double* __restrict__ weights, double* __restrict__ gout) {
  __shared__ double A[GMM_MAXN * GMM_MAXN], V[GMM_MAXN * GMM_MAXN];
  __shared__ double cs_c[GMM_MAXN / 2], cs_s[GMM_MAXN / 2];
  __shared__ int cs_p[GMM_MAXN / 2], cs_q[GMM_MAXN / 2];
  __shared__ double vec[GMM_MAXN];
  const int k = threadIdx.x;
  const int T = (n + 15) / 16, NP = T * (T + 1) / 2;
  bool kept = k < n;
  for (int t = 0; t < iters; ++t) {
    if (nb > 0) {
      const double* part = src + (long)t * nb * NP * 256;
      for (int e = k; e < NP * 256; e += 64) {
        int p = e >> 8, ti = 0;  // tile pair index -> (ti, tj)
        while (p >= T - ti) { p -= T - ti; ++ti; }
        const int tj = ti + p;
        const int i = ti * 16 + ((e & 255) >> 4), j = tj * 16 + (e & 15);
        if (i > j || j >= n) continue;  // (the upper triangle stands for both halves: one writer per entry)
        double a = 0.0;
        for (int b = 0; b < nb; ++b) a += part[(long)b * NP * 256 + e];
        A[i * n + j] = a;
        A[j * n + i] = a;
      }
    } else {
      for (int e = k; e < n * n; e += 64) A[e] = src[(long)t * n * n + e];
    }
    __syncthreads();
    if (nb > 0 || centre) {
      double rm = 0.0;
      if (k < n) {
        for (int j = 0; j < n; ++j) rm += A[k * n + j];
        rm /= (double)n;
        vec[k] = rm;
      }
      __syncthreads();
      double mean = 0.0;
      for (int j = 0; j < n; ++j) mean += vec[j];
      mean /= (double)n;
      // H is symmetric, so column j's mean is row j's; the two means are added first so that C stays symmetric
      for (int e = k; e < n * n; e += 64) A[e] = A[e] - (vec[e / n] + vec[e % n]) + mean;
      __syncthreads();
    }
    for (int e = k; e < n * n; e += 64) {
      gout[(long)t * n * n + e] = A[e];
      V[e] = (e / n == e % n) ? 1.0 : 0.0;
    }
    __syncthreads();
    const int top = jacobi_top(A, V, cs_c, cs_s, cs_p, cs_q, n, DNC_SWEEPS);
    const double lam = A[top * n + top];
    double sc = 0.0;
    if (k < n) {
      const double u = V[k * n + top];
      sc = (lam < 0.0 ? 0.0 : lam) * (u * u);
      scores[(long)t * n + k] = sc;
      vec[k] = sc != sc ? INFINITY : sc;
    }
    __syncthreads();
    if (k < n) {
      const double mine = vec[k];
      int above = 0;
      for (int j = 0; j < n; ++j) above += (vec[j] > mine || (vec[j] == mine && j > k)) ? 1 : 0;
      kept = kept && above >= drop;
    }
    __syncthreads();
  }
  if (__ballot(kept) == 0ull) kept = k < n;  // the empty intersection keeps every row
  if (k < n) vec[k] = kept ? w[k] : 0.0;
  __syncthreads();
  double sum = 0.0;
  for (int j = 0; j < n; ++j) sum += vec[j];
  if (k < n) {
    keep[k] = kept ? 1 : 0;
    weights[k] = vec[k] / sum;
  }
}

int afl_dnc_select(const double* src, int nb, int n, int iters, int centre, int drop, const double* w,
                   unsigned char* keep, double* scores, double* weights, double* gout, hipStream_t s) {
  if (n < 1 || n > GMM_MAXN || iters < 1 || nb < 0 || drop < 0 || drop > n - 1) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_dnc_select, dim3(1), dim3(64), 0, s, src, nb, n, iters, centre, drop, w, keep, scores, weights,
                     gout);
  return (int)hipGetLastError();
}

// ============================================================================ krum_select
// Krum's selection on the squared-distance matrix D [n][n] (fp64, n <= 64), the shared step of Multi-Krum (Blanchard
// et al.) and Bulyan (El Mhamdi et al.).  score(i) on an active set of m rows = the sum, in ascending order of value,
// of the k = max(m - f - 2, 1) smallest D[i][j] over the active j != i (0 when m = 1); a pick is the active row with the
// smallest (score, index).  iterated = 0: the rows are scored once on the full set and ``rounds`` picks follow that
// ranking; iterated = 1: every pick re-scores the rows still active and deactivates the winner.
// One wave, lane i owns row i: it sorts its row once (stable insertion sort of (value, column) in LDS, row stride
// n_max + 1 words so that the lanes' rows fall into different banks), after which a score is one walk along the sorted
// row that skips the inactive columns.  The active set is a 64-bit mask every lane holds; the pick is a butterfly
// reduction on (score, index) whose result is taken from lane 0, so the mask stays wave-uniform whatever the scores
// hold (a NaN compares as a tie and falls to the lower index; an active row always wins over an inactive one, so
// sel[] only ever holds indices in [0, n)).
// D is read as a symmetric matrix, its upper triangle standing for both halves: with k = 1 (Bulyan's last picks) two
// rows that are each other's nearest neighbour tie EXACTLY, and the tie rule only means something if D[i][j] and
// D[j][i] are the same bits (a Gram product computed as a full matrix product may differ in the last bit).
constexpr int KS_LD = GMM_MAXN + 1;
constexpr int BSA_TRIED = 4, BSA_ACC = 20;  // (the st[40] layout of linalg.hip bisect_decide)

// The rule on a matrix already laid out in LDS (V the values, J the column of every entry, row stride KS_LD; the
// caller has synchronised after filling them): sort, score, pick.  Every trip count is fixed by (n, rounds): no
// loop depends on a value.  -> the active mask after ``rounds`` picks (wave-uniform), ``first`` = the first pick.
// ``sel`` / ``scores`` may be null (k_agr_bisect only wants the mask).
// Lane i sorts row i of (V, J) by (value, column): a stable insertion sort in LDS, the columns being in ascending order
// on entry (krum_select_wave, k_nnm_weights).
__device__ __forceinline__ void sort_rows_wave(double* V, unsigned char* J, int n) {
  const int i = threadIdx.x;
  if (i < n) {
    double* v = V + i * KS_LD;
    unsigned char* jx = J + i * KS_LD;
    for (int p = 1; p < n; ++p) {
      const double x = v[p];
      const unsigned char jp = jx[p];
      int q = p - 1;
      while (q >= 0 && v[q] > x) {
        v[q + 1] = v[q];
        jx[q + 1] = jx[q];
        --q;
      }
      v[q + 1] = x;
      jx[q + 1] = jp;
    }
  }
}

__device__ __forceinline__ unsigned long long krum_select_wave(double* V, unsigned char* J, int n, int f, int rounds,
                                                               int iterated, int* __restrict__ sel,
                                                               double* __restrict__ scores, int& first) {
  const int i = threadIdx.x;
  sort_rows_wave(V, J, n);
  unsigned long long act = n >= 64 ? ~0ull : ((1ull << n) - 1ull);
  double sc = 0.0;
  first = 0;
  for (int t = 0; t < rounds; ++t) {
    const bool mine = i < n && ((act >> i) & 1ull);
    if (t == 0 || iterated) {
      const int m = iterated ? n - t : n;
      const int k = max(m - f - 2, 1);
      sc = 0.0;
      if (mine) {
        int cnt = 0;
        for (int p = 0; p < n && cnt < k; ++p) {
          const int j = J[i * KS_LD + p];
          if (j != i && ((act >> j) & 1ull)) {
            sc += V[i * KS_LD + p];
            ++cnt;
          }
        }
      }
      if (t == 0 && i < n && scores) scores[i] = sc;
    }
    int bi = mine ? i : 64;
    double bs = sc;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double os = __shfl_xor(bs, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      const bool take = oi < 64 && (bi >= 64 || os < bs || (!(bs < os) && oi < bi));
      bs = take ? os : bs;
      bi = take ? oi : bi;
    }
    bi = __shfl(bi, 0, 64) & 63;  // (rounds <= n: an active row exists, so the index is one of [0, n))
    if (i == 0 && sel) sel[t] = bi;
    if (t == 0) first = bi;
    act &= ~(1ull << bi);
  }
  return act;
}

__global__ void __launch_bounds__(64) k_krum_select(const double* __restrict__ D, int n, int f, int rounds, int iterated,
                                                    int* __restrict__ sel, unsigned char* __restrict__ mask,
                                                    double* __restrict__ scores) {
  __shared__ double V[GMM_MAXN * KS_LD];
  __shared__ unsigned char J[GMM_MAXN * KS_LD];
  const int i = threadIdx.x;
  for (int e = i; e < n * n; e += 64) {
    const int r = e / n, c = e - r * n;
    V[r * KS_LD + c] = r <= c ? D[e] : D[c * n + r];  // (the upper triangle, see above)
    J[r * KS_LD + c] = (unsigned char)c;
  }
  __syncthreads();
  int first;
  const unsigned long long act = krum_select_wave(V, J, n, f, rounds, iterated, sel, scores, first);
  if (i < n) mask[i] = ((act >> i) & 1ull) ? 0 : 1;
}

int afl_krum_select(const double* D, int n, int f, int rounds, int iterated, int* sel, unsigned char* mask,
                    double* scores, hipStream_t s) {
  if (n < 1 || n > GMM_MAXN || f < 0 || f > n || rounds < 1 || rounds > n || (iterated != 0 && iterated != 1))
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_krum_select, dim3(1), dim3(64), 0, s, D, n, f, rounds, iterated, sel, mask, scores);
  return (int)hipGetLastError();
}

// ============================================================================ nnm_weights
// Nearest-neighbour mixing (Allouah et al., AISTATS 2023; docs/PARITY.md): the mixing matrix W [n][n] from the squared
// distances D [n][n] (fp64, n <= 64, read as symmetric from the upper triangle like k_krum_select).  Row i mixes itself
// and the first k = n - f - 1 other rows by (D_ij, j) ascending, a NaN distance counting as +inf; W_ij = inv =
// 1 / (n - f) (formed on the host in fp64) on that set N_i, 0 elsewhere; nbr[i] = N_i as a 64-bit mask.
// One wave, lane i owns row i and sorts it with the sort of krum_select; the walk along the sorted row has a fixed trip
// count (f = 0 is no special case).  W is written with coalesced stores from the masks in LDS.
__global__ void __launch_bounds__(64) k_nnm_weights(const double* __restrict__ D, int n, int k, double inv,
                                                    double* __restrict__ W, unsigned long long* __restrict__ nbr) {
  __shared__ double V[GMM_MAXN * KS_LD];
  __shared__ unsigned char J[GMM_MAXN * KS_LD];
  __shared__ unsigned long long M[GMM_MAXN];
  const int i = threadIdx.x;
  for (int e = i; e < n * n; e += 64) {
    const int r = e / n, c = e - r * n;
    const double d = r <= c ? D[e] : D[c * n + r];
    V[r * KS_LD + c] = d != d ? INFINITY : d;
    J[r * KS_LD + c] = (unsigned char)c;
  }
  __syncthreads();
  sort_rows_wave(V, J, n);
  unsigned long long m = 0ull;
  if (i < n) {
    m = 1ull << i;
    int cnt = 0;
    for (int p = 0; p < n; ++p) {
      const int j = J[i * KS_LD + p];
      const bool take = j != i && cnt < k;
      m |= take ? (1ull << j) : 0ull;
      cnt += take ? 1 : 0;
    }
    M[i] = m;
    nbr[i] = m;
  }
  __syncthreads();
  for (int e = i; e < n * n; e += 64) {
    const int r = e / n, c = e - r * n;
    W[e] = ((M[r] >> c) & 1ull) ? inv : 0.0;
  }
}

int afl_nnm_weights(const double* D, int n, int f, double* W, unsigned long long* nbr, hipStream_t s) {
  if (n < 1 || n > GMM_MAXN || f < 0 || f > n - 1) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_nnm_weights, dim3(1), dim3(64), 0, s, D, n, n - f - 1, 1.0 / (double)(n - f), W, nbr);
  return (int)hipGetLastError();
}

// ============================================================================ agr_bisect
// The AGR-tailored attacks on Krum / Multi-Krum / Bulyan (Shejwalkar & Houmansadr, NDSS 2021; docs/PARITY.md): the
// whole bisection on gamma in ONE launch of one wave.  The modelled system has n' = K + m rows: the K genuine rows
// (indices 0 .. K - 1, squared distances Dg [K][K] fp64, read as symmetric from the upper triangle) and m identical
// copies of the candidate c(gamma) = mean - gamma dev (indices K .. n' - 1: last, so that every index tie goes against
// the attacker), whose squared distance to genuine row j is d_j = max(A_j - 2 gamma B_j + gamma^2 C, 0) and to each
// other 0.  Per gamma the wave rebuilds that n' x n' matrix in LDS and runs krum_select_wave on it:
//   target 0 (Krum):       1 pick,            accepted when the pick is a copy;
//   target 1 (Multi-Krum): n' - f picks,      scored once,            accepted when all m copies are picked;
//   target 2 (Bulyan):     n' - 2 f picks,    re-scored every pick,   accepted when all m copies are picked.
// A NaN in A, B or C rejects.  An accept moves gamma up by step / 2, a reject down; the state is bisect_decide's
// (linalg.hip): st[0] the next gamma, st[1] the last accepted, st[2] the last tried, st[4 + i] the gamma tried at
// iteration i, st[20 + i] 1.0 if it was accepted.  d_j is formed with individually rounded products and sums (no
// contraction), the operation order of the composite, so that both sides see the same bits.
// Every trip count is fixed by (n', f, target, n_iter); lane 0 writes the state with ordinary stores.
__global__ void __launch_bounds__(64) k_agr_bisect(const double* __restrict__ Dg, const double* __restrict__ A,
                                                   const double* __restrict__ B, const double* __restrict__ C, int K,
                                                   int m, int f, int target, int n_iter, double step0,
                                                   double* __restrict__ st) {
  __shared__ double V[GMM_MAXN * KS_LD];
  __shared__ unsigned char J[GMM_MAXN * KS_LD];
  __shared__ double dj[GMM_MAXN];
  const int i = threadIdx.x;
  const int n = K + m;
  const int rounds = target == 0 ? 1 : (target == 1 ? n - f : n - 2 * f);
  const int iterated = target == 2 ? 1 : 0;
  const unsigned long long copies = (n >= 64 ? ~0ull : ((1ull << n) - 1ull)) & ~((1ull << K) - 1ull);  // (K < 64)
  const double a = i < K ? A[i] : 0.0, b = i < K ? B[i] : 0.0, c = C[0];
  const bool bad = __any((a != a) || (b != b) || (c != c));
  double g = st[0], step = step0;
  for (int it = 0; it < n_iter; ++it) {
    if (i < K) {
      const double q = __dadd_rn(__dsub_rn(a, __dmul_rn(__dmul_rn(2.0, g), b)), __dmul_rn(__dmul_rn(g, g), c));
      dj[i] = q > 0.0 ? q : 0.0;
    }
    __syncthreads();
    for (int e = i; e < n * n; e += 64) {
      const int r = e / n, cc = e - r * n;
      const int lo = min(r, cc), hi = max(r, cc);
      V[r * KS_LD + cc] = hi < K ? Dg[lo * K + hi] : (lo < K ? dj[lo] : 0.0);
      J[r * KS_LD + cc] = (unsigned char)cc;
    }
    __syncthreads();
    int first;
    const unsigned long long act = krum_select_wave(V, J, n, f, rounds, iterated, nullptr, nullptr, first);
    const bool acc = !bad && (target == 0 ? first >= K : (act & copies) == 0ull);
    if (i == 0) {
      st[BSA_TRIED + it] = g;
      st[BSA_ACC + it] = acc ? 1.0 : 0.0;
      st[2] = g;
      if (acc) st[1] = g;
      st[0] = acc ? g + step / 2.0 : g - step / 2.0;
    }
    g = acc ? g + step / 2.0 : g - step / 2.0;
    step *= 0.5;
    __syncthreads();  // (the next iteration overwrites the rows this one's lanes still walked)
  }
}

int afl_agr_bisect(const double* Dg, const double* A, const double* B, const double* C, int K, int m, int f, int target,
                   int n_iter, double gamma0, double* st, hipStream_t s) {
  const long n = (long)K + m;
  if (K < 1 || m < 1 || n > GMM_MAXN || n_iter < 1 || n_iter > 16 || !afl_agr_admissible(n, f, target))
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_agr_bisect, dim3(1), dim3(64), 0, s, Dg, A, B, C, K, m, f, target, n_iter, gamma0, st);
  return (int)hipGetLastError();
}

// ============================================================================ bulyan_coord
// Bulyan's coordinate step: per column, over the theta rows sel[0 .. theta) of U (a device index list: no gathered
// copy of the rows), the mean of the beta values closest to the lower median (sorted position (theta - 1) / 2, as
// coord_select's median).  One thread per column, the k_coord_select register sort (NaN last, counted), then a two-pointer
// expansion from the median position: the beta smallest keys (|x - med| in fp32, x) are contiguous in sorted order, and
// on an equal distance the left neighbour, the smaller value, is taken.  Registers are only indexed by compile-time
// constants (the neighbours come out of predicated sweeps), the window is summed in fp64 in sorted order.
// A row index is clamped into [0, N) before it is used as an address.
template <int NMAX>
__global__ void __launch_bounds__(256) k_bulyan_coord(const float* __restrict__ U, int N, long P,
                                                      const int* __restrict__ sel, int theta, int beta,
                                                      float* __restrict__ out) {
  long c = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= P) return;
  float v[NMAX];
  int nnan = 0;
#pragma unroll
  for (int i = 0; i < NMAX; ++i) {
    float x = __int_as_float(0x7f800000);
    if (i < theta) {
      const int r = min(max(sel[i], 0), N - 1);
      x = U[(long)r * P + c];
    }
    v[i] = x;
    nnan += x != x ? 1 : 0;
  }
#pragma unroll
  for (int r = 0; r < NMAX; ++r) {
#pragma unroll
    for (int i = (r & 1); i + 1 < NMAX; i += 2) {
      float a = v[i], b = v[i + 1];
      bool sw = (a > b) || (a != a && b == b);
      v[i] = sw ? b : a;
      v[i + 1] = sw ? a : b;
    }
  }
  const int mid = (theta - 1) / 2;
  float med = 0.f;
#pragma unroll
  for (int i = 0; i < NMAX; ++i) med = (i == mid) ? v[i] : med;
  // NaN as composite.bulyan_coord (torch.sort: NaN last, a NaN distance last): the window runs over the ``real``
  // non-NaN values only; beta > real gives NaN; a NaN median (mid >= real) makes every distance NaN, and the stable
  // sort of those keeps the beta smallest values
  const int real = theta - nnan;
  int lo = mid, hi = mid;
  for (int s = 1; s < beta; ++s) {
    float a = 0.f, b = 0.f;  // the neighbours v[lo - 1], v[hi + 1]
#pragma unroll
    for (int i = 0; i < NMAX; ++i) {
      a = (i == lo - 1) ? v[i] : a;
      b = (i == hi + 1) ? v[i] : b;
    }
    const bool left = lo > 0 && (hi + 1 >= real || fabsf(a - med) <= fabsf(b - med));
    // (beta <= real: one side is inside the list while the window is short)
    if (left || hi + 1 >= real) lo = max(lo - 1, 0);
    else ++hi;
  }
  if (mid >= real) {
    lo = 0;
    hi = beta - 1;
  }
  double acc = 0.0;
#pragma unroll
  for (int i = 0; i < NMAX; ++i) acc += (i >= lo && i <= hi) ? (double)v[i] : 0.0;
  out[c] = beta > real ? __int_as_float(0x7fc00000) : (float)(acc / (double)beta);
}

int afl_bulyan_coord(const float* U, int N, long P, const int* sel, int theta, int beta, float* out, hipStream_t s) {
  if (N < 1 || P < 1 || theta < 1 || theta > N || theta > 64 || beta < 1 || beta > theta)
    return (int)hipErrorInvalidValue;
  dim3 g(afl_cdiv(P, 256)), b(256);
  if (theta <= 8) hipLaunchKernelGGL(k_bulyan_coord<8>, g, b, 0, s, U, N, P, sel, theta, beta, out);
  else if (theta <= 16) hipLaunchKernelGGL(k_bulyan_coord<16>, g, b, 0, s, U, N, P, sel, theta, beta, out);
  else if (theta <= 32) hipLaunchKernelGGL(k_bulyan_coord<32>, g, b, 0, s, U, N, P, sel, theta, beta, out);
  else hipLaunchKernelGGL(k_bulyan_coord<64>, g, b, 0, s, U, N, P, sel, theta, beta, out);
  return (int)hipGetLastError();
}

// ============================================================================ geomed_weights
// Geometric median (RFA, Pillutla et al.: smoothed Weiszfeld) of n <= 64 rows in Gram space: with w on the simplex and
// z = sum_j w_j u_j, ||u_i - z||^2 = G_ii - 2 (G w)_i + w^T G w for the centred Gram G, so the iteration needs the rows
// only for the final weighted sum.  Start w = alpha; an iteration computes d_i = sqrt(max(0, .)), the objective
// sum_i alpha_i d_i and w_i <- alpha_i / max(nu, d_i), normalised; it stops after ``iters`` iterations or once
// |objective - previous| <= 1e-9 objective.  One wave, lane i owns row i of G in LDS (row stride n_max + 1): G w is a
// per-lane dot product in column order, w^T G w, the objective and the normaliser are xor-butterfly sums, which leave
// the same bits on every lane (each step adds the same two operands on both partners), so the stop is wave-uniform.
__global__ void __launch_bounds__(64) k_geomed_weights(const double* __restrict__ G, const double* __restrict__ alpha,
                                                       int n, int iters, double nu, double* __restrict__ w,
                                                       double* __restrict__ info) {
  __shared__ double A[GMM_MAXN * KS_LD], wb[GMM_MAXN];
  const int i = threadIdx.x;
  lds_load_square(A, KS_LD, G, n);
  const double al = i < n ? alpha[i] : 0.0;
  double wi = al, prev = INFINITY, obj = 0.0;
  int it = 0;
  __syncthreads();
  const double gii = i < n ? A[i * KS_LD + i] : 0.0;
  while (it < iters) {
    wb[i] = wi;
    __syncthreads();
    double gw = 0.0;
    if (i < n)
      for (int j = 0; j < n; ++j) gw += A[i * KS_LD + j] * wb[j];
    __syncthreads();  // (wb is rewritten by the next iteration)
    const double q = wave_sum(wi * gw);
    const double d2 = gii - 2.0 * gw + q;
    const double d = i < n ? sqrt(d2 > 0.0 ? d2 : 0.0) : 0.0;
    obj = wave_sum(al * d);
    const double u = i < n ? al / (d > nu ? d : nu) : 0.0;
    wi = u / wave_sum(u);
    ++it;
    if (fabs(obj - prev) <= 1e-9 * obj) break;  // (uniform: every lane holds the same obj and prev)
    prev = obj;
  }
  if (i < n) w[i] = wi;
  if (i == 0) {
    info[0] = (double)it;
    info[1] = obj;
  }
}

int afl_geomed_weights(const double* G, const double* alpha, int n, int iters, double nu, double* w, double* info,
                       hipStream_t s) {
  if (n < 1 || n > GMM_MAXN || iters < 1 || !(nu > 0.0)) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_geomed_weights, dim3(1), dim3(64), 0, s, G, alpha, n, iters, nu, w, info);
  return (int)hipGetLastError();
}

// ============================================================================ cclip_weights
// Centred clipping (Karimireddy, He & Jaggi, ICML 2021; rule text in docs/PARITY.md) of n <= 64 rows in Gram space.
// The iterate is v = g + sum_j c_j y_j (G the Gram of y_i = x_i - g about the centre g, c0 = 0) or v = sum_j c_j x_j
// (G the mean-centred Gram, c0 = alpha, sum c = 1 kept by the update); either way
//     d_i^2 = max(0, G_ii - 2 (G c)_i + c^T G c),  s_i = d_i <= tau ? 1 : tau / d_i,  c <- (1 - S) c + alpha s,
// S = sum_i alpha_i s_i, exactly ``iters`` times.  tau <= 0 on entry means auto: the lower median (sorted position
// (m - 1) / 2) of the m finite rows' d_i of iteration 0, by rank counting with ties ranked by row (exactly one row
// has the wanted rank), kept for every iteration and never read back.  A row whose G_ii is not finite (a faulted
// client's NaN row) has s = 0 and c = 0 exactly and is skipped, not multiplied by zero, in G c, c^T G c, S and the
// median; alpha is not renormalised.  One wave, lane i owns row i of G in LDS (row stride n_max + 1): G c is a per-lane
// dot product in column order, the sums are xor butterflies that leave the same bits on every lane.
// info = {tau, rows with s < 1 in the last iteration, finite rows}.
__global__ void __launch_bounds__(64) k_cclip_weights(const double* __restrict__ G, const double* __restrict__ alpha,
                                                      const double* __restrict__ c0, int n, int iters, double tau_in,
                                                      double* __restrict__ c, double* __restrict__ info) {
  __shared__ double A[GMM_MAXN * KS_LD], cb[GMM_MAXN], db[GMM_MAXN], tau_s;
  const int i = threadIdx.x;
  lds_load_square(A, KS_LD, G, n);
  __syncthreads();
  const double gii = i < n ? A[i * KS_LD + i] : 0.0;
  const bool fin = i < n && gram_finite(gii);
  const unsigned long long fm = __ballot(fin);
  const int m = __popcll(fm);
  const double al = fin ? alpha[i] : 0.0;
  double ci = fin ? c0[i] : 0.0, tau = tau_in;
  int clipped = 0;
  for (int it = 0; it < iters; ++it) {
    cb[i] = ci;
    __syncthreads();
    double gc = 0.0;
    if (fin)
      for (int j = 0; j < n; ++j)
        if ((fm >> j) & 1ull) gc += A[i * KS_LD + j] * cb[j];
    const double q = wave_sum(fin ? ci * gc : 0.0);
    const double d2 = gii - 2.0 * gc + q;
    const double d = fin ? sqrt(d2 > 0.0 ? d2 : 0.0) : INFINITY;
    if (it == 0 && !(tau_in > 0.0)) {  // auto (uniform)
      db[i] = d;
      if (i == 0) tau_s = 0.0;  // (no finite row)
      __syncthreads();
      int rank = 0;
      if (fin)
        for (int l = 0; l < n; ++l)
          rank += (((fm >> l) & 1ull) && (db[l] < d || (db[l] == d && l < i))) ? 1 : 0;
      if (fin && rank == (m - 1) / 2) tau_s = d;
      __syncthreads();
      tau = tau_s;
    }
    const double s = fin ? (d <= tau ? 1.0 : tau / d) : 0.0;  // (d > tau >= 0: no division by zero)
    const double S = wave_sum(al * s);
    ci = fin ? (1.0 - S) * ci + al * s : 0.0;
    clipped = __popcll(__ballot(fin && s < 1.0));
    __syncthreads();  // (cb is rewritten by the next iteration)
  }
  if (i < n) c[i] = ci;
  if (i == 0) {
    info[0] = tau;
    info[1] = (double)clipped;
    info[2] = (double)m;
  }
}

int afl_cclip_weights(const double* G, const double* alpha, const double* c0, int n, int iters, double tau, double* c,
                      double* info, hipStream_t s) {
  if (n < 1 || n > GMM_MAXN || iters < 1 || tau != tau) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_cclip_weights, dim3(1), dim3(64), 0, s, G, alpha, c0, n, iters, tau, c, info);
  return (int)hipGetLastError();
}

// ============================================================================ anchored rows
// out = (float)(g + sum_{j: c_j != 0} c_j (U_j - g)): centred clipping's result about the centre g, the weights read
// from the device; one column per thread, rows in ascending order, differences and sum in fp64.  A row with c_j == 0
// (a non-finite row's weight) is not read into the sum.
__global__ void __launch_bounds__(256) k_anchored_rows(const float* __restrict__ U, const double* __restrict__ c, int N,
                                                       long P, const float* __restrict__ g, float* __restrict__ out) {
  long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  const double gp = (double)g[p];
  double acc = 0.0;
  for (int j = 0; j < N; ++j) {
    const double cj = c[j];
    if (cj != 0.0) acc += cj * ((double)U[(long)j * P + p] - gp);
  }
  out[p] = (float)(gp + acc);
}

int afl_anchored_rows(const float* U, const double* c, int N, long P, const float* g, float* out, hipStream_t s) {
  if (N < 1 || P < 1) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_anchored_rows, dim3(afl_cdiv(P, 256)), dim3(256), 0, s, U, c, N, P, g, out);
  return (int)hipGetLastError();
}

// ============================================================================ foolsgold_weights
// FoolsGold (Fung, Yoon & Beschastnikh, RAID 2020; rule text in docs/PARITY.md) from the Gram G = H H^T of the n <= 64
// clients' histories:
//     cs_ij = clamp(G_ij / (sqrt(G_ii) sqrt(G_jj)), -1, 1) for i != j, 0 for a pair with a zero or non-finite norm
//     v_i = max_{j != i} cs_ij;  cs'_ij = cs_ij v_i / v_j where v_j > v_i (and v_j != 0), else cs_ij
//     a_i = clamp(1 - max_{j != i} cs'_ij, 0, 1), M = max_i a_i;  M <= 0: every alpha_i = 0, otherwise a_i <- a_i / M,
//     an a_i of exactly 1 becomes 0.99, alpha_i = clamp(kappa (ln(a_i / (1 - a_i)) + 0.5), 0, 1);  n = 1: alpha = 1, v = 0
// One wave, lane i owns row i of G in LDS (row stride n_max + 1): the two row maxima are per-lane loops over the n
// columns, M is an xor butterfly, which leaves the same bits on every lane; every trip count is fixed by n.
// out [3][n] = {alpha, v, c = alpha0 * alpha (the weights of anchored_rows)}.
__global__ void __launch_bounds__(64) k_foolsgold_weights(const double* __restrict__ G, const double* __restrict__ alpha0,
                                                          int n, double kappa, double* __restrict__ out) {
  __shared__ double A[GMM_MAXN * KS_LD], nb[GMM_MAXN], vb[GMM_MAXN];
  const int i = threadIdx.x;
  lds_load_square(A, KS_LD, G, n);
  __syncthreads();
  const double gii = i < n ? A[i * KS_LD + i] : 0.0;
  nb[i] = gram_finite(gii) && gii > 0.0 ? sqrt(gii) : 0.0;  // (0: the row's pairs get cs = 0)
  __syncthreads();
  const double* row = A + (i < n ? i : 0) * KS_LD;
  const double mi = nb[i];
  double v = -INFINITY;
  for (int j = 0; j < n; ++j) {
    const double nj = nb[j];
    double cs = mi > 0.0 && nj > 0.0 ? row[j] / (mi * nj) : 0.0;
    cs = cs > 1.0 ? 1.0 : (cs < -1.0 ? -1.0 : cs);
    v = j != i && cs > v ? cs : v;
  }
  v = i < n && n > 1 ? v : 0.0;
  vb[i] = v;
  __syncthreads();
  double m = -INFINITY;
  for (int j = 0; j < n; ++j) {
    const double nj = nb[j], vj = vb[j];
    double cs = mi > 0.0 && nj > 0.0 ? row[j] / (mi * nj) : 0.0;
    cs = cs > 1.0 ? 1.0 : (cs < -1.0 ? -1.0 : cs);
    cs = vj > v && vj != 0.0 ? cs * v / vj : cs;
    m = j != i && cs > m ? cs : m;
  }
  double a = 1.0 - m;
  a = a > 1.0 ? 1.0 : (a > 0.0 ? a : 0.0);  // (a NaN, which no finite Gram gives, counts as 0)
  a = i < n ? a : 0.0;
  const double M = wave_max(a);
  double al = 0.0;
  if (M > 0.0) {  // (uniform)
    a = a / M;
    a = a == 1.0 ? 0.99 : a;
    al = kappa * (log(a / (1.0 - a)) + 0.5);
    al = al > 1.0 ? 1.0 : (al > 0.0 ? al : 0.0);
  }
  al = n == 1 ? 1.0 : al;
  if (i < n) {
    out[i] = al;
    out[n + i] = v;
    out[2 * n + i] = alpha0[i] * al;
  }
}

int afl_foolsgold_weights(const double* G, const double* alpha0, int n, double kappa, double* out, hipStream_t s) {
  if (n < 1 || n > GMM_MAXN || !(kappa > 0.0)) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_foolsgold_weights, dim3(1), dim3(64), 0, s, G, alpha0, n, kappa, out);
  return (int)hipGetLastError();
}

// ============================================================================ signguard
// SignGuard (Xu, Huang, Qu & Song, ICDCS 2022; rule text in docs/PARITY.md) of n <= 64 rows about the centre g.
// k_sign_stats: one pass over U and g.  Block (x, y) owns the columns [x SS_CH, (x + 1) SS_CH) of the rows
// [y SS_ROWS, (y + 1) SS_ROWS); column p is in the sampled window {s, ..., s + b - 1 mod P} when p >= s ? p < e1 :
// p < wrap (e1 = s + b, wrap = s + b - P: two integer compares).  The loads of the block's rows are issued together,
// then per (block, row): qpart [x][row] = sum (U - g)^2 over the chunk in fp64 — every thread its SS_CH / 256 strided
// columns in ascending order, an xor butterfly over the wave, the four waves in wave order — and cpart [x][row] =
// {#(d > 0), #(d < 0)} over the chunk's window columns (a NaN difference is neither).  No atomics; k_signguard_select
// sums the blocks in block order.
constexpr int SS_CH = 1024, SS_ROWS = 8;

__global__ void __launch_bounds__(256) k_sign_stats(const float* __restrict__ U, const float* __restrict__ g, int K,
                                                    long P, long s, long e1, long wrap, double* __restrict__ qpart,
                                                    int* __restrict__ cpart) {
  __shared__ double sq[SS_ROWS][4];
  __shared__ int sc[SS_ROWS][4];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int r0 = blockIdx.y * SS_ROWS, nr = K - r0 < SS_ROWS ? K - r0 : SS_ROWS;
  constexpr int M = SS_CH / 256;
  double gv[M];
  bool ok[M], win[M];
#pragma unroll
  for (int m = 0; m < M; ++m) {
    const long p = (long)blockIdx.x * SS_CH + t + 256 * m;
    ok[m] = p < P;
    gv[m] = ok[m] ? (double)g[p] : 0.0;
    win[m] = ok[m] && (p >= s ? p < e1 : p < wrap);
  }
  float uv[SS_ROWS][M];
#pragma unroll
  for (int r = 0; r < SS_ROWS; ++r) {
    const float* u = U + (long)(r0 + r) * P + (long)blockIdx.x * SS_CH + t;
#pragma unroll
    for (int m = 0; m < M; ++m) uv[r][m] = r < nr && ok[m] ? u[256 * m] : 0.0f;
  }
#pragma unroll
  for (int r = 0; r < SS_ROWS; ++r) {
    double q = 0.0;
    int cnt = 0;  // pos in the low half, neg in the high half (<= SS_CH each)
#pragma unroll
    for (int m = 0; m < M; ++m) {
      if (r < nr && ok[m]) {
        const double d = (double)uv[r][m] - gv[m];
        q += d * d;
        if (win[m]) cnt += (d > 0.0 ? 1 : 0) + (d < 0.0 ? 1 << 16 : 0);
      }
    }
    for (int o = 32; o; o >>= 1) {
      q += __shfl_xor(q, o, 64);
      cnt += __shfl_xor(cnt, o, 64);
    }
    if (lane == 0) {
      sq[r][w] = q;
      sc[r][w] = cnt;
    }
  }
  __syncthreads();
  if (t < nr) {
    const long e = (long)blockIdx.x * K + r0 + t;
    qpart[e] = ((sq[t][0] + sq[t][1]) + sq[t][2]) + sq[t][3];
    const int cnt = sc[t][0] + sc[t][1] + sc[t][2] + sc[t][3];
    cpart[2 * e] = cnt & 0xFFFF;
    cpart[2 * e + 1] = cnt >> 16;
  }
}

int afl_sign_stats_chunk() { return SS_CH; }
int afl_sign_stats_nblocks(long P) { return (int)afl_cdiv(P, SS_CH); }
uint32_t afl_signguard_start(uint64_t seed, long P) { return pl_signguard_start(seed, (uint32_t)P); }

// partial: 2 nb K doubles = qpart [nb][K] fp64, then cpart [nb][K][2] int32
int afl_sign_stats(const float* U, const float* g, int K, long P, long s, long b, double* partial, hipStream_t st) {
  if (K < 1 || K > GMM_MAXN || P < 1 || b < 1 || b > P || s < 0 || s >= P) return (int)hipErrorInvalidValue;
  const int nb = afl_sign_stats_nblocks(P);
  hipLaunchKernelGGL(k_sign_stats, dim3(nb, afl_cdiv(K, SS_ROWS)), dim3(256), 0, st, U, g, K, P, s, s + b, s + b - P,
                     partial, (int*)(partial + (long)nb * K));
  return (int)hipGetLastError();
}

// k_signguard_select: one wave, lane i owns row i; steps 2 to 5 of the rule.  part = the nb blocks' partials of
// k_sign_stats (summed in block order; nb = 1: the statistics themselves).  Every comparison that decides something is
// on fp64 values of the host mirror's expression shape (``composite.signguard_select``): contraction is off in this
// kernel, distances are compared squared ((dx dx + dy dy) + dz dz against h h), sums run in index order.
//   norms: q not finite -> +inf; M = the norm of rank (n - 1) / 2 by (norm, row); pass = finite and lo M <= norm <= hi M;
//   scale = norm <= M ? 1 : M / norm.  F_i = (pos, b - pos - neg, neg) / b in LDS.
//   h = max(mean_i sqrt(k-th smallest squared distance from F_i, itself counted), 1 / b), k = max(1, n / 2).
//   mean shift from every row, flat kernel of radius h, <= SG_MAXIT moves, stop after a move of <= 1e-3 h (diverges per
//   lane); cnt = points within h of the final centre; seeds ordered by (cnt descending, row); an alive seed removes the
//   later seeds whose centres lie within h (one ballot per position); label = the nearest alive centre, the earlier one
//   on a tie; the largest cluster, the earlier one on a tie; keep = pass and in it; c = keep alpha scale / sum kept alpha.
// out: keep, norm_ok [n] 0/1, label [n], feat [n][3], c [n], info = {M, h}, qout [n], cout [n][2] = {pos, neg}.
constexpr int SG_MAXIT = 300;

__device__ __forceinline__ double sg_d2(double a0, double a1, double a2, double c0, double c1, double c2) {
#pragma clang fp contract(off)
  const double dx = a0 - c0, dy = a1 - c1, dz = a2 - c2;
  return (dx * dx + dy * dy) + dz * dz;
}

__global__ void __launch_bounds__(64) k_signguard_select(const double* __restrict__ part, int nb, int n, long b,
                                                         const double* __restrict__ alpha, double lo, double hi,
                                                         unsigned char* __restrict__ keep,
                                                         unsigned char* __restrict__ norm_ok, int* __restrict__ label,
                                                         double* __restrict__ feat, double* __restrict__ c,
                                                         double* __restrict__ info, double* __restrict__ qout,
                                                         int* __restrict__ cout) {
#pragma clang fp contract(off)
  __shared__ double F[3][GMM_MAXN], C[3][GMM_MAXN], vec[GMM_MAXN], D[GMM_MAXN * KS_LD], Ms;
  __shared__ int ord[GMM_MAXN], cn[GMM_MAXN];
  const int i = threadIdx.x;
  const bool act = i < n;
  // ---- 2. statistics: the blocks in block order
  double q = 0.0;
  int pos = 0, neg = 0;
  if (act) {
    const int* cp = (const int*)(part + (long)nb * n);
    for (int x = 0; x < nb; ++x) {
      const long e = (long)x * n + i;
      q += part[e];
      pos += cp[2 * e];
      neg += cp[2 * e + 1];
    }
  }
  // ---- 3. norm filter
  const double norm = act && gram_finite(q) ? sqrt(q) : INFINITY;
  vec[i] = norm;
  __syncthreads();
  int rank = 0;
  for (int l = 0; l < n; ++l) rank += (vec[l] < norm || (vec[l] == norm && l < i)) ? 1 : 0;
  if (act && rank == (n - 1) / 2) Ms = norm;
  __syncthreads();
  const double M = Ms;
  const bool pass = act && norm < INFINITY && lo * M <= norm && norm <= hi * M;
  const double scale = norm <= M ? 1.0 : M / norm;
  // ---- 4. features, bandwidth
  const double bd = (double)b;
  const double f0 = (double)pos / bd, f1 = (double)(b - pos - neg) / bd, f2 = (double)neg / bd;
  F[0][i] = f0;
  F[1][i] = f1;
  F[2][i] = f2;
  __syncthreads();
  const int kth = n / 2 > 1 ? n / 2 : 1;
  double r2 = 0.0;
  if (act) {
    double* row = D + i * KS_LD;
    for (int j = 0; j < n; ++j) row[j] = sg_d2(F[0][j], F[1][j], F[2][j], f0, f1, f2);
    for (int j = 0; j < n; ++j) {
      const double dj = row[j];
      int rk = 0;
      for (int l = 0; l < n; ++l) rk += (row[l] < dj || (row[l] == dj && l < j)) ? 1 : 0;
      if (rk == kth - 1) r2 = dj;
    }
  }
  __syncthreads();  // (vec: every lane has read the norms)
  vec[i] = sqrt(r2);
  __syncthreads();
  double rsum = 0.0;
  for (int j = 0; j < n; ++j) rsum += vec[j];
  const double rmean = rsum / (double)n, floor_h = 1.0 / bd;
  const double h = rmean > floor_h ? rmean : floor_h;
  const double h2 = h * h, tol = 1e-3 * h, conv2 = tol * tol;
  // ---- mean shift: every row a seed
  double c0 = f0, c1 = f1, c2 = f2;
  int cnt = 0;
  if (act) {
    for (int it = 0; it < SG_MAXIT; ++it) {
      double s0 = 0.0, s1 = 0.0, s2 = 0.0;
      int m = 0;
      for (int j = 0; j < n; ++j) {
        if (sg_d2(F[0][j], F[1][j], F[2][j], c0, c1, c2) <= h2) {
          s0 += F[0][j];
          s1 += F[1][j];
          s2 += F[2][j];
          ++m;
        }
      }
      if (m == 0) break;
      const double n0 = s0 / (double)m, n1 = s1 / (double)m, n2 = s2 / (double)m;
      const double mv2 = sg_d2(n0, n1, n2, c0, c1, c2);
      c0 = n0;
      c1 = n1;
      c2 = n2;
      if (mv2 <= conv2) break;
    }
    for (int j = 0; j < n; ++j) cnt += sg_d2(F[0][j], F[1][j], F[2][j], c0, c1, c2) <= h2 ? 1 : 0;
  }
  C[0][i] = c0;
  C[1][i] = c1;
  C[2][i] = c2;
  cn[i] = cnt;
  __syncthreads();
  // ---- dedup in the order (cnt descending, row ascending)
  int mypos = 0;
  for (int j = 0; j < n; ++j) mypos += (cn[j] > cnt || (cn[j] == cnt && j < i)) ? 1 : 0;
  if (act) ord[mypos] = i;
  __syncthreads();
  unsigned long long alive = n == 64 ? ~0ull : (1ull << n) - 1ull;
  for (int p = 0; p < n; ++p) {
    const int sp = ord[p];
    if ((alive >> sp) & 1ull) {  // (uniform)
      const bool kill = act && mypos > p && ((alive >> i) & 1ull) &&
                        sg_d2(c0, c1, c2, C[0][sp], C[1][sp], C[2][sp]) <= h2;
      alive &= ~__ballot(kill);
    }
  }
  // ---- labels: the nearest alive centre, the earlier one on a tie; the largest cluster
  int lab = -1, ncl = 0;
  double best = INFINITY;
  for (int p = 0; p < n; ++p) {
    const int sp = ord[p];
    if ((alive >> sp) & 1ull) {
      const double d2 = sg_d2(f0, f1, f2, C[0][sp], C[1][sp], C[2][sp]);
      if (d2 < best) {
        best = d2;
        lab = ncl;
      }
      ++ncl;
    }
  }
  __syncthreads();  // (cn: every lane has its position)
  cn[i] = act ? lab : -1;
  __syncthreads();
  int top = 0, topsz = -1;
  for (int cl = 0; cl < ncl; ++cl) {
    int sz = 0;
    for (int j = 0; j < n; ++j) sz += cn[j] == cl ? 1 : 0;
    if (sz > topsz) {
      topsz = sz;
      top = cl;
    }
  }
  // ---- 5. weights
  const bool kp = pass && lab == top;
  const double al = act ? alpha[i] : 0.0;
  __syncthreads();  // (vec: every lane has summed the radii)
  vec[i] = kp ? al : 0.0;
  __syncthreads();
  double den = 0.0;
  for (int j = 0; j < n; ++j) den += vec[j];
  if (act) {
    keep[i] = kp ? 1 : 0;
    norm_ok[i] = pass ? 1 : 0;
    label[i] = lab;
    feat[3 * i] = f0;
    feat[3 * i + 1] = f1;
    feat[3 * i + 2] = f2;
    c[i] = kp ? (al * scale) / den : 0.0;
    qout[i] = q;
    cout[2 * i] = pos;
    cout[2 * i + 1] = neg;
  }
  if (i == 0) {
    info[0] = M;
    info[1] = h;
  }
}

int afl_signguard_select(const double* part, int nb, int n, long b, const double* alpha, double lo, double hi,
                         unsigned char* keep, unsigned char* norm_ok, int* label, double* feat, double* c, double* info,
                         double* qout, int* cout, hipStream_t s) {
  if (n < 1 || n > GMM_MAXN || nb < 1 || b < 1 || !(lo > 0.0) || !(hi >= lo)) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_signguard_select, dim3(1), dim3(64), 0, s, part, nb, n, b, alpha, lo, hi, keep, norm_ok, label,
                     feat, c, info, qout, cout);
  return (int)hipGetLastError();
}

// ============================================================================ flame
// FLAME (Nguyen et al., USENIX Security 2022; rule text in docs/PARITY.md) of n <= 64 rows from the Gram G of the
// updates about the centre.  k_flame_select: one wave, lane i owns row i; contraction off, the host mirror's expression
// shapes (``composite.flame_select``), correctly rounded sqrt and division.
//   finite rows: G_ii finite (n' of them, m = n' / 2 + 1); e_i = sqrt(G_ii) (0 when G_ii <= 0).
//   D_ij = 1 - G_ij / (e_i e_j) from the upper triangle of G (i < j; the lower one is its copy, so D is symmetric to
//   the bit), 1 when e_i or e_j is 0, +inf when the quotient is NaN, D_ii = 0; D overwrites G in LDS.
//   Prim's minimum spanning tree of the finite rows from the lowest one: n' - 1 wave-wide argmins by (key, lane); step
//   s leaves edge s = (weight, lower row, higher row).  The edges are rank-sorted by (weight, lower, higher), then
//   united in that order on 64-bit membership masks (lane i holds its component's) until a union holds >= m rows:
//   its weight is d*.  Every further edge of weight d* is united too (the components of the graph D <= d* are those of
//   any spanning tree's edges <= d*), and the component that reached m is kept.
//   S = the lower median (rank (n' - 1) / 2 by (e, row)) of the finite rows' e; for a kept row c_i = (alpha_i scale_i) /
//   sum_kept alpha, scale_i = e_i <= S ? 1 : S / e_i, the sum in index order; else c_i = 0.
// out: keep [n] 0/1, c [n], info = {S, sigma = lam S, d*, m, n'}.
__global__ void __launch_bounds__(64) k_flame_select(const double* __restrict__ G, const double* __restrict__ alpha,
                                                     int n, double lam, unsigned char* __restrict__ keep,
                                                     double* __restrict__ c, double* __restrict__ info) {
#pragma clang fp contract(off)
  __shared__ double A[GMM_MAXN * KS_LD], eb[GMM_MAXN], ew[GMM_MAXN], sw[GMM_MAXN], S_s;
  __shared__ unsigned char ea[GMM_MAXN], eh[GMM_MAXN], sa[GMM_MAXN], sh[GMM_MAXN];
  const int i = threadIdx.x;
  lds_load_square(A, KS_LD, G, n);
  __syncthreads();
  const double gii = i < n ? A[i * KS_LD + i] : 0.0;
  const bool fin = i < n && gram_finite(gii);
  const unsigned long long fm = __ballot(fin);
  const int nf = __popcll(fm), m = nf / 2 + 1;
  const double e = fin && gii > 0.0 ? sqrt(gii) : 0.0;
  eb[i] = e;
  __syncthreads();
  // ---- cosine distances: the upper triangle first (lane i reads and writes its own row only), then its copy
  if (i < n) {
    for (int j = i + 1; j < n; ++j) {
      const double ej = eb[j];
      double d = 1.0;
      if (e != 0.0 && ej != 0.0) {
        d = 1.0 - A[i * KS_LD + j] / (e * ej);
        d = d == d ? d : INFINITY;
      }
      A[i * KS_LD + j] = d;
    }
    A[i * KS_LD + i] = 0.0;
  }
  __syncthreads();
  if (i < n)
    for (int j = 0; j < i; ++j) A[i * KS_LD + j] = A[j * KS_LD + i];
  __syncthreads();
  // ---- Prim from the lowest finite row
  const int r0 = nf ? __ffsll((long long)fm) - 1 : 0;
  unsigned long long tree = nf ? 1ull << r0 : 0ull;
  double key = fin ? A[i * KS_LD + r0] : INFINITY;
  int par = r0;
  const int ne = nf > 0 ? nf - 1 : 0;
  for (int s = 0; s < ne; ++s) {
    const bool cand = fin && !((tree >> i) & 1ull);
    double bk = cand ? key : INFINITY;
    int bi = cand ? i : 64;
    for (int o = 32; o; o >>= 1) {
      const double ok = __shfl_xor(bk, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (ok < bk || (ok == bk && oi < bi)) {
        bk = ok;
        bi = oi;
      }
    }
    const int u = bi & 63;  // (the same on every lane; bi < 64: a finite row is outside the tree while s < n' - 1)
    const int pu = __shfl(par, u, 64);
    if (i == 0) {
      ew[s] = bk;
      ea[s] = (unsigned char)(u < pu ? u : pu);
      eh[s] = (unsigned char)(u < pu ? pu : u);
    }
    tree |= 1ull << u;
    const double d = A[i * KS_LD + u];
    if (cand && i != u && d < key) {
      key = d;
      par = u;
    }
  }
  __syncthreads();
  // ---- the edges in the order (weight, lower row, higher row)
  if (i < ne) {
    const double w = ew[i];
    const int a = ea[i], h = eh[i];
    int rank = 0;
    for (int t = 0; t < ne; ++t) {
      const double wt = ew[t];
      const int at = ea[t], ht = eh[t];
      rank += (wt < w || (wt == w && (at < a || (at == a && ht < h)))) ? 1 : 0;
    }
    sw[rank] = w;
    sa[rank] = (unsigned char)a;
    sh[rank] = (unsigned char)h;
  }
  __syncthreads();
  // ---- unions until a component holds m rows, then the ties of d*
  unsigned long long mask = fin ? 1ull << i : 0ull;
  bool found = false;
  double dstar = 0.0;
  int arow = r0;
  for (int k = 0; k < ne; ++k) {  // (uniform)
    const double w = sw[k];
    if (found && w != dstar) break;
    const int a = sa[k], h = sh[k];
    const unsigned long long mg = __shfl(mask, a, 64) | __shfl(mask, h, 64);
    if ((mg >> i) & 1ull) mask = mg;
    if (!found && __popcll(mg) >= m) {
      found = true;
      dstar = w;
      arow = a;
    }
  }
  const unsigned long long kept = nf ? __shfl(mask, arow, 64) : 0ull;  // (n' = 1: the row's own bit)
  const bool kp = (kept >> i) & 1ull;
  // ---- the lower median norm, the weights
  if (i == 0) S_s = 0.0;  // (no finite row)
  __syncthreads();
  int rank = 0;
  if (fin)
    for (int l = 0; l < n; ++l) rank += (((fm >> l) & 1ull) && (eb[l] < e || (eb[l] == e && l < i))) ? 1 : 0;
  if (fin && rank == (nf - 1) / 2) S_s = e;
  const double al = i < n ? alpha[i] : 0.0;
  ew[i] = kp ? al : 0.0;  // (ew: the edges are in sw)
  __syncthreads();
  const double S = S_s;
  double den = 0.0;
  for (int j = 0; j < n; ++j) den += ew[j];
  const double scale = e <= S ? 1.0 : S / e;
  if (i < n) {
    keep[i] = kp ? 1 : 0;
    c[i] = kp ? (al * scale) / den : 0.0;
  }
  if (i == 0) {
    info[0] = S;
    info[1] = lam * S;
    info[2] = dstar;
    info[3] = (double)m;
    info[4] = (double)nf;
  }
}

int afl_flame_select(const double* G, const double* alpha, int n, double lam, unsigned char* keep, double* c,
                     double* info, hipStream_t s) {
  if (n < 1 || n > GMM_MAXN || !(lam >= 0.0) || !(lam < INFINITY)) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_flame_select, dim3(1), dim3(64), 0, s, G, alpha, n, lam, keep, c, info);
  return (int)hipGetLastError();
}

// k_flame_rows: out = (float)(g + sum_{j: c_j != 0} c_j (U_j - g) + sigma z), FLAME's row pass.  The sum is
// k_anchored_rows' (rows in ascending order, differences and sum in fp64, a row with c_j == 0 not read); sigma is read
// from the device (k_flame_select's info[1]) and z are the N(0, 1) draws of k_noise_philox's scheme under the key
// (k0, k1): the counter is the column group p / 4, one call gives the normals of 4 consecutive columns, so a thread
// owns one group (the last one may hold fewer than four columns).  sigma == 0: no draw, the term is left out and the
// bits are k_anchored_rows'.
__global__ void __launch_bounds__(256) k_flame_rows(const float* __restrict__ U, const double* __restrict__ c, int N,
                                                    long P, const float* __restrict__ g,
                                                    const double* __restrict__ sigma_p, uint32_t k0, uint32_t k1,
                                                    float* __restrict__ out) {
  const long grp = (long)blockIdx.x * blockDim.x + threadIdx.x;  // column group of 4
  const long p0 = grp * 4;
  if (p0 >= P) return;
  const int nq = P - p0 < 4 ? (int)(P - p0) : 4;
  double gp[4], acc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int q = 0; q < 4; ++q) gp[q] = q < nq ? (double)g[p0 + q] : 0.0;
  for (int j = 0; j < N; ++j) {
    const double cj = c[j];
    if (cj != 0.0) {
      const float* u = U + (long)j * P + p0;
      float uv[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) uv[q] = q < nq ? u[q] : 0.0f;
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[q] += cj * ((double)uv[q] - gp[q]);
    }
  }
  double r[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) r[q] = gp[q] + acc[q];
  const double sigma = *sigma_p;
  if (sigma != 0.0) {
    uint32_t c0 = (uint32_t)grp, c1 = (uint32_t)(grp >> 32), c2 = 0, c3 = 0, a = k0, b = k1;
#pragma unroll
    for (int t = 0; t < 10; ++t) {
      philox_round(c0, c1, c2, c3, a, b);
      a += 0x9E3779B9u;
      b += 0xBB67AE85u;
    }
    const double u0 = ((double)c0 + 1.0) * 2.3283064365386963e-10, u1 = ((double)c1 + 1.0) * 2.3283064365386963e-10;
    const double u2 = ((double)c2 + 1.0) * 2.3283064365386963e-10, u3 = ((double)c3 + 1.0) * 2.3283064365386963e-10;
    const double r0 = sqrt(-2.0 * log(u0)), r1 = sqrt(-2.0 * log(u2));
    const double t0 = 6.283185307179586 * u1, t1 = 6.283185307179586 * u3;
    r[0] += sigma * (r0 * cos(t0));
    r[1] += sigma * (r0 * sin(t0));
    r[2] += sigma * (r1 * cos(t1));
    r[3] += sigma * (r1 * sin(t1));
  }
#pragma unroll
  for (int q = 0; q < 4; ++q)
    if (q < nq) out[p0 + q] = (float)r[q];
}

int afl_flame_rows(const float* U, const double* c, int N, long P, const float* g, const double* sigma, uint64_t key,
                   float* out, hipStream_t s) {
  if (N < 1 || P < 1 || sigma == nullptr) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_flame_rows, dim3(afl_cdiv(afl_cdiv(P, 4), 256)), dim3(256), 0, s, U, c, N, P, g, sigma,
                     (uint32_t)key, (uint32_t)(key >> 32), out);
  return (int)hipGetLastError();
}
