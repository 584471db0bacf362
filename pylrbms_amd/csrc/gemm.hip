// Batched fp64 Gram / projection GEMM on the CDNA4 matrix cores:
//   G[b] (Mx x My) = alpha * X[b]^T diag(rowscale) Y[b],   X [K][ldx], Y [K][ldy] row-major ("K-major" operands).
//
// This is the dense half of the projections P1 / P2: V^T (A V), Wt^T (E Wt), Rt^T (B Rt), ...
// with K = n (DG DoFs), n_rt or n_T of ONE subdomain, so every problem is small (K <= a few hundred) and the batch
// (number of subdomains) supplies the parallelism.
//
// Mapping: v_mfma_f64_16x16x4_f64.  A operand lane l holds A[i = l&15][k = l>>4] = X[k][i], B operand lane l holds
// B[k = l>>4][j = l&15] = Y[k][j]: both are read from K-major LDS tiles with 16 consecutive lanes on 16 consecutive
// doubles.  The tile rows are padded to BM+16 doubles so that the four k-rows a wave reads at once fall into
// different halves of the 64 LDS banks (ds_read_b64 services 32 lanes per cycle).  C/D: lane l holds rows
// (l>>4) + 4 r, r = 0..3, of column l&15.
//
// Workgroup = 256 threads = 4 waves, output tile 64 x 64 (wave tile 32 x 32 = 2 x 2 MFMA tiles),
// K staged in chunks of 16 rows.  fp64 MFMA peak on gfx950 = 78.6 TFLOP/s (= one 16x16x4 per 64 cycles per SIMD).
#include "lrbms_dev.h"

namespace {

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int BM = 64, BN = 64, BK = 16, PAD = 16;

__global__ __launch_bounds__(256) void k_gemm_tn(int K, int Mx, int My, const double* __restrict__ X, long sx, int ldx,
                                                 const double* __restrict__ Y, long sy, int ldy, double* __restrict__ G,
                                                 long sg, int ldg, const double* __restrict__ rowscale, double alpha) {
  __shared__ double Xs[BK][BM + PAD];
  __shared__ double Ys[BK][BN + PAD];
  const int bz = blockIdx.z;
  const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
  X += (long)bz * sx;
  Y += (long)bz * sy;
  G += (long)bz * sg;
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int wr = wave >> 1, wc = wave & 1;
  const int li = lane & 15, lk = lane >> 4;

  d4 acc[2][2];
  for (int a = 0; a < 2; ++a)
    for (int b = 0; b < 2; ++b) acc[a][b] = (d4){0.0, 0.0, 0.0, 0.0};

  // staging: thread -> (row = tid / 16, 4 consecutive columns)
  const int srow = tid >> 4, scol = (tid & 15) * 4;
  for (int k0 = 0; k0 < K; k0 += BK) {
    const int kr = k0 + srow;
    double xv[4] = {0, 0, 0, 0}, yv[4] = {0, 0, 0, 0};
    if (kr < K) {
      const double sc = rowscale ? rowscale[kr] : 1.0;
      const double* xp = X + (long)kr * ldx + m0 + scol;
      const double* yp = Y + (long)kr * ldy + n0 + scol;
      for (int c = 0; c < 4; ++c) {
        if (m0 + scol + c < Mx) xv[c] = xp[c];
        if (n0 + scol + c < My) yv[c] = sc * yp[c];
      }
    }
    __syncthreads();  // previous chunk fully consumed
    for (int c = 0; c < 4; ++c) {
      Xs[srow][scol + c] = xv[c];
      Ys[srow][scol + c] = yv[c];
    }
    __syncthreads();
    for (int kk = 0; kk < BK; kk += 4) {
      double a[2], b[2];
      for (int mi = 0; mi < 2; ++mi) a[mi] = Xs[kk + lk][wr * 32 + mi * 16 + li];
      for (int ni = 0; ni < 2; ++ni) b[ni] = Ys[kk + lk][wc * 32 + ni * 16 + li];
      for (int mi = 0; mi < 2; ++mi)
        for (int ni = 0; ni < 2; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[mi], b[ni], acc[mi][ni], 0, 0, 0);
    }
  }
  for (int mi = 0; mi < 2; ++mi)
    for (int ni = 0; ni < 2; ++ni) {
      const int col = n0 + wc * 32 + ni * 16 + li;
      for (int r = 0; r < 4; ++r) {
        const int row = m0 + wr * 32 + mi * 16 + lk + 4 * r;
        if (row < Mx && col < My) G[(long)row * ldg + col] = alpha * acc[mi][ni][r];
      }
    }
}

// Projection of K source load vectors (lrbms_project_sources), one launch on the matrix cores.  Per subdomain s the output
// [K][N + C] is X^T Y with two column ranges of different reduction length:
//   columns [0, N):  X[k][j] = bK[j][s][k] (k < n DoFs),             Y = V[s]    [n][N]     -> rhs_red_K[j][s][.]
//   columns [N, N+C): X[k][j] = sum of bK[j][s] over the 3 DoFs of T (k = T < n_T), Y = D[s] [n_T][C] -> r_fd_K[j][s][.]
// (b0 + b1 + b2 in the order the fused pass forms it).  Workgroup = (64-column tile, s): 4 waves, one 16-column MFMA tile each,
// all ceil(K / 16) <= 4 row tiles of the K sources, so every tile of V and D is read once for all K.
__global__ __launch_bounds__(256) void k_project_sources(int S, int n, int nT, int N, int C, int K, int tilesV,
                                                         const double* __restrict__ bK, const double* __restrict__ V,
                                                         const double* __restrict__ D, double* __restrict__ rhs_K,
                                                         double* __restrict__ rfd_K) {
  __shared__ double Xs[BK][BM + PAD];
  __shared__ double Ys[BK][BN + PAD];
  const int s = blockIdx.y;
  const bool dpart = (int)blockIdx.x >= tilesV;
  const int n0 = (dpart ? (int)blockIdx.x - tilesV : (int)blockIdx.x) * BN;
  const int Kred = dpart ? nT : n, ncol = dpart ? C : N;
  const double* Y = dpart ? D + (long)s * nT * C : V + (long)s * n * N;
  const long bstride = (long)S * n;                  // between the sources in bK [K][S][n]
  const double* bs = bK + (long)s * n;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int li = lane & 15, lk = lane >> 4;
  const int KT = (K + 15) >> 4;
  d4 acc[4];
#pragma unroll
  for (int m = 0; m < 4; ++m) acc[m] = (d4){0.0, 0.0, 0.0, 0.0};
  const int srow = tid >> 4, scol = (tid & 15) * 4;
  double xv[4], yv[4];
  // thread -> (row srow of the chunk, 4 consecutive columns); the loads of chunk k0 + BK are issued before the MFMAs of
  // chunk k0, so their latency hides behind the matrix work (one chunk in flight per thread)
  auto load = [&](int k0) {
    const int kr = k0 + srow;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      xv[c] = 0.0;
      yv[c] = 0.0;
    }
    if (kr < Kred) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int j = scol + c;
        if (j < K) {
          const double* bj = bs + j * bstride;
          xv[c] = dpart ? bj[3 * kr] + bj[3 * kr + 1] + bj[3 * kr + 2] : bj[kr];
        }
        if (n0 + scol + c < ncol) yv[c] = Y[(long)kr * ncol + n0 + scol + c];
      }
    }
  };
  load(0);
  for (int k0 = 0; k0 < Kred; k0 += BK) {
    __syncthreads();  // previous chunk fully consumed
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      Xs[srow][scol + c] = xv[c];
      Ys[srow][scol + c] = yv[c];
    }
    __syncthreads();
    if (k0 + BK < Kred) load(k0 + BK);
    for (int kk = 0; kk < BK; kk += 4) {
      const double b = Ys[kk + lk][wave * 16 + li];
#pragma unroll
      for (int m = 0; m < 4; ++m)
        if (m < KT) acc[m] = __builtin_amdgcn_mfma_f64_16x16x4f64(Xs[kk + lk][m * 16 + li], b, acc[m], 0, 0, 0);
    }
  }
  const int col = n0 + wave * 16 + li;
  if (col >= ncol) return;
  double* out = dpart ? rfd_K : rhs_K;
#pragma unroll
  for (int m = 0; m < 4; ++m)
    if (m < KT)
      for (int r = 0; r < 4; ++r) {
        const int j = m * 16 + lk + 4 * r;
        if (j < K) out[((long)j * S + s) * ncol + col] = acc[m][r];
      }
}

}  // namespace

int launch_project_sources(lrbms_ctx* ctx, int N, int C, int K, const double* bK, const double* V, const double* D, double* rhs_K,
                           double* rfd_K, hipStream_t st) {
  if (K < 1 || K > BM) return lrbms_fail(ctx, LRBMS_E_INVALID, "project_sources: K must be in [1, 64]");
  if (N < 1 || C < 1) return lrbms_fail(ctx, LRBMS_E_INVALID, "project_sources: empty basis");
  if (ctx->S > 65535) return lrbms_fail(ctx, LRBMS_E_INVALID, "project_sources: more than 65535 subdomains");
  const int tilesV = (N + BN - 1) / BN, tilesD = (C + BN - 1) / BN;
  hipLaunchKernelGGL(k_project_sources, dim3(tilesV + tilesD, ctx->S), dim3(256), 0, st, ctx->S, ctx->t.n, ctx->t.nT, N, C, K, tilesV,
                     bK, V, D, rhs_K, rfd_K);
  LRBMS_LAUNCH_CHECK(ctx);
  return LRBMS_OK;
}

int launch_gemm_tn(lrbms_ctx* ctx, int batch, int K, int Mx, int My, const double* X, long sx, int ldx, const double* Y,
                   long sy, int ldy, double* G, long sg, int ldg, const double* rowscale, double alpha, hipStream_t st) {
  if (batch <= 0 || K <= 0 || Mx <= 0 || My <= 0) return lrbms_fail(ctx, LRBMS_E_INVALID, "gemm_tn: empty problem");
  if (ldx < Mx || ldy < My || ldg < My) return lrbms_fail(ctx, LRBMS_E_INVALID, "gemm_tn: leading dimension too small");
  dim3 grid((My + BN - 1) / BN, (Mx + BM - 1) / BM, batch);
  if (grid.z > 65535) return lrbms_fail(ctx, LRBMS_E_INVALID, "gemm_tn: batch > 65535");
  hipLaunchKernelGGL(k_gemm_tn, grid, dim3(256), 0, st, K, Mx, My, X, sx, ldx, Y, sy, ldy, G, sg, ldg, rowscale, alpha);
  LRBMS_LAUNCH_CHECK(ctx);
  return LRBMS_OK;
}
