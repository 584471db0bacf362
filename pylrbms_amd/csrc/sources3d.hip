// 3D / P2 path: affine sources -- k3_source_gram, k3_project_sources, k3_source_terms and lrbms3_combine_sources, which launches
// the shape-agnostic kernel of online.hip through launch_combine_sources_base.  online3d.hip (the batched parabolic estimate)
// reaches k3_source_terms through launch_source_terms.
// (lrbms3_reduced_solve_batch_src and the _src forms of the implicit Euler live with their solvers in online3d.hip and lrbms3d.hip.)
#include "lrbms3d_dev.h"

using namespace lrbms3;

// ================================================================================================= affine sources
// f(mu) or f(t, mu) = sum_j phi_j f_j with K components: the Grams of the components, the projections of their
// load vectors and element integrals, and the f terms of the residual indicator for columns with coefficients of their own.
int launch_combine_sources_base(lrbms_ctx_base* ctx, int* num_cus, int K, long M, const double* phi, const double* x_K, double* y,
                                hipStream_t st);      // online.hip: the 2D export's kernel, shape-agnostic

namespace {

// F2 [S][K][K]: one workgroup per (subdomain, pair j <= l), the expression and the fixed-order tree of k3_scalars' f2 with one factor
// from each component -- K = 1 gives that f2 bit for bit.  comp = S n_T f_stride, the stride between two components' samples.
__global__ __launch_bounds__(256) void k3_source_gram(T3 t, int K, long comp, const double* __restrict__ f_smp_K, double* __restrict__ F2) {
  __shared__ double sa[256];
  const int s = blockIdx.x, tid = threadIdx.x;
  int j = 0, l = blockIdx.y;                 // pair index -> (j, l), row-wise over the upper triangle
  while (l >= K - j) {
    l -= K - j;
    ++j;
  }
  l += j;
  const double* fj = f_smp_K + (long)j * comp;
  const double* fl = f_smp_K + (long)l * comp;
  double acc = 0.0;
  for (int e = tid; e < t.nT; e += 256) {
    const double* rj = fj + ((long)s * t.nT + e) * t.f_stride;
    const double* rl = fl + ((long)s * t.nT + e) * t.f_stride;
    for (int k = 0; k < t.nB; ++k) acc += t.WB[k] * rj[k] * rl[k];
  }
  sa[tid] = acc;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) sa[tid] += sa[tid + w];
    __syncthreads();
  }
  if (tid == 0) {
    F2[((long)s * K + j) * K + l] = sa[0];
    F2[((long)s * K + l) * K + j] = sa[0];
  }
}

// Both projections of lrbms3_project_sources in one launch on the fp64 matrix cores, one workgroup of 8 waves per (subdomain, role):
//   role 0   rhs_red_K [K][S][N]  = b_K[j][s]^T V_s                       rows = the n DoFs, row operand = the rows of V_s
//   role 1   r_fd_K    [K][S][QN] = sum_e bdiv_K[j][s][e] div(R_self)_e    rows = the n_T elements, row operand = the divergence of the
//            element's four RT0 rows of the flux image R_self [S][n_rt][QN], formed in the lane (orientation and |f| / |T| as k3_estimate)
// A wave takes four rows per step: the A operand holds the K components' weights of these rows (lane: component l & 15, row l >> 4),
// the B operand the row operand (lane: column l & 15, row l >> 4); V and R_self are read once, whatever K.  KT = 16-component tiles;
// up to four 16-column tiles.  The waves' tiles are summed in a fixed order through the LDS.
template <int KT>
__global__ __launch_bounds__(512) void k3_project_sources(T3 t, int N, int QN, int K, const int* __restrict__ list,
                                                          const double* __restrict__ b_K, const double* __restrict__ bdiv_K,
                                                          const double* __restrict__ V,
                                                          const double* __restrict__ Rs, double* __restrict__ rhs_K,
                                                          double* __restrict__ rfd_K) {
  __shared__ double red[8][256];
  const int s = list ? list[blockIdx.x] : blockIdx.x, mode = blockIdx.y, tid = threadIdx.x, lane = tid & 63, li = lane & 15, lk = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int cols = mode ? QN : N, rows = mode ? t.nT : t.n, nct = (cols + 15) / 16;
  const long xs = (long)t.S * rows;
  const double* X = (mode ? bdiv_K : b_K) + (long)s * rows;
  d4 acc[KT][4];
#pragma unroll
  for (int rt = 0; rt < KT; ++rt)
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) acc[rt][ct] = d4{0.0, 0.0, 0.0, 0.0};
  for (int r0 = wave * 4; r0 < rows; r0 += 32) {
    const int r = r0 + lk;
    const bool rin = r < rows;
    double a[KT], v[4];
#pragma unroll
    for (int rt = 0; rt < KT; ++rt) {
      const int j = 16 * rt + li;
      a[rt] = (rin && j < K) ? X[(long)j * xs + r] : 0.0;
    }
    if (mode == 0) {
      const double* row = V + ((long)s * t.n + (rin ? r : 0)) * N;
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        const int c = 16 * ct + li;
        v[ct] = (rin && c < cols) ? row[c] : 0.0;
      }
    } else {
      const int e = rin ? r : 0, ty = t.elem_type[e];
      double dd[4];
      const double* rr[4];
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        dd[f] = rin ? sgn3(t, s, e, f) * t.divc[ty * 4 + f] : 0.0;
        rr[f] = Rs + ((long)s * t.nrt + t.elem_rt[e * 4 + f]) * QN;
      }
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        const int c = 16 * ct + li;
        double dv = 0.0;
        if (c < cols) {
#pragma unroll
          for (int f = 0; f < 4; ++f) dv += dd[f] * rr[f][c];
        }
        v[ct] = dv;
      }
    }
#pragma unroll
    for (int rt = 0; rt < KT; ++rt)
#pragma unroll
      for (int ct = 0; ct < 4; ++ct)
        if (ct < nct) acc[rt][ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[rt], v[ct], acc[rt][ct], 0, 0, 0);
  }
  double* out = mode ? rfd_K : rhs_K;
#pragma unroll
  for (int rt = 0; rt < KT; ++rt)
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
      if (ct >= nct) continue;               // (uniform over the workgroup)
      __syncthreads();
#pragma unroll
      for (int r = 0; r < 4; ++r) red[wave][r * 64 + lane] = acc[rt][ct][r];
      __syncthreads();
      if (tid < 256) {
        const int r = tid >> 6, l = tid & 63;
        double sum = 0.0;
        for (int w = 0; w < 8; ++w) sum += red[w][tid];
        const int j = 16 * rt + (l >> 4) + 4 * r, c = 16 * ct + (l & 15);
        if (j < K && c < cols) out[((long)j * t.S + s) * cols + c] = sum;
      }
    }
}

// Sum over the workers (tid >> 3) of the values of column tid & 7, fixed order; red [256].  The result is valid in every thread.
__device__ inline double column_sum8(double v, double* red) {
  const int tid = threadIdx.x;
  __syncthreads();
  red[tid] = v;
  __syncthreads();
  for (int w = 128; w >= 8; w >>= 1) {
    if (tid < w) red[tid] += red[tid + w];
    __syncthreads();
  }
  return red[tid & 7];
}

// The f terms of the residual indicator (lrbms3_reduced_source_terms) for eight columns per workgroup: threads = (worker tid >> 3,
// column tid & 7) as in k3_estimate_batch, so the eight columns share every factor row.  ur, zf = Rb ur_a and the divergence of zf on
// the side elements are those of k3_estimate; theta [L][Q] and phi [L][K] are per column.  out [S][L].
__global__ __launch_bounds__(256) void k3_source_terms(T3 t, int Q, int N, int K, int L, const double* __restrict__ theta,
                                                       const double* __restrict__ phi, const double* __restrict__ F2,
                                                       const double* __restrict__ r_fd_K, const double* __restrict__ bdiv_K,
                                                       const double* __restrict__ Rb, const double* __restrict__ u,
                                                       const double* __restrict__ ceps, double hdiam, double* __restrict__ out) {
  extern __shared__ double lds[];
  const int s = blockIdx.x, tid = threadIdx.x, w = tid >> 3, m = tid & 7, QN = Q * N;
  double* us = lds;                    // [7][N][8] coefficients on the neighbourhood (0 where no neighbour)
  double* zf = us + 7 * N * 8;         // [nbf][8]  flux of the neighbours on the side faces
  double* ths = zf + t.nbf * 8;        // [8][8]    theta_q of the columns
  double* red = ths + 64;              // [256]
  const int l0 = blockIdx.y * 8;
  const int l = l0 + m < L ? l0 + m : L - 1;          // columns behind L repeat the last one and are not stored
  for (int k = tid; k < 7 * N * 8; k += 256) {
    const int slot = k / (N * 8), j = (k >> 3) % N, mm = k & 7;
    const int ll = l0 + mm < L ? l0 + mm : L - 1;
    const int s2 = t.nbr[s * 7 + slot];
    us[k] = s2 >= 0 ? u[((long)s2 * N + j) * L + ll] : 0.0;
  }
  if (tid < 64) {
    const int q = tid >> 3, ll = l0 + (tid & 7) < L ? l0 + (tid & 7) : L - 1;
    ths[tid] = q < Q ? theta[(long)ll * Q + q] : 0.0;
  }
  __syncthreads();
  for (int sf = w; sf < t.nbf; sf += 32) {
    const double* ua = us + side_slot(sf / t.ncf) * N * 8 + m;
    const double* r = Rb + ((long)s * t.nbf + sf) * QN;
    double acc = 0.0;
    for (int q = 0; q < Q; ++q) {
      double aq = 0.0;
      for (int j = 0; j < N; ++j) aq += r[q * N + j] * ua[j * 8];
      acc += ths[q * 8 + m] * aq;
    }
    zf[sf * 8 + m] = acc;
  }
  __syncthreads();
  const double* ph = phi + (long)l * K;
  const double* u0 = us + 3 * N * 8 + m;
  double p_fd = 0.0, p_ff = 0.0;
  for (int r = w; r < QN; r += 32) {
    double rp = 0.0;
    for (int j = 0; j < K; ++j) rp += ph[j] * r_fd_K[((long)j * t.S + s) * QN + r];
    p_fd += rp * (ths[(r / N) * 8 + m] * u0[(r % N) * 8]);
  }
  for (int k = w; k < t.nsel; k += 32) {
    const int e = t.sel_elem[k], ty = t.elem_type[e];
    double dv = 0.0;
    for (int f = 0; f < 4; ++f) {
      const int sf = t.sel_sf[k * 4 + f];
      const double ze = sf >= 0 ? zf[sf * 8 + m] : 0.0;
      dv += sgn3(t, s, e, f) * t.divc[ty * 4 + f] * ze;
    }
    double bp = 0.0;
    for (int j = 0; j < K; ++j) bp += ph[j] * bdiv_K[((long)j * t.S + s) * t.nT + e];
    p_fd += bp * dv;
  }
  for (int k = w; k < K * K; k += 32) p_ff += ph[k / K] * F2[(long)s * K * K + k] * ph[k % K];
  const double fd = column_sum8(p_fd, red);
  const double ff = column_sum8(p_ff, red);
  if (w == 0 && l0 + m < L) {
    const double pi = 3.14159265358979323846;
    out[(long)s * L + l] = (ff - 2.0 * fd) * (1.0 / (pi * pi)) / ceps[s] * hdiam * hdiam;
  }
}

}  // namespace

namespace lrbms3 {

static size_t source_terms_lds(const T3& t, int N) { return sizeof(double) * (7 * (size_t)N * 8 + (size_t)t.nbf * 8 + 64 + 256); }
bool source_terms_fits(const lrbms3_ctx* ctx, int N) { return source_terms_lds(ctx->t, N) <= 64 * 1024; }
void launch_source_terms(hipStream_t st, const T3& t, int Q, int N, int K, int L, const double* theta, const double* phi, const double* F2,
                         const double* r_fd_K, const double* bdiv_K, const double* Rb, const double* u, const double* ceps, double hdiam,
                         double* out) {
  hipLaunchKernelGGL(k3_source_terms, dim3(t.S, (L + 7) / 8), dim3(256), source_terms_lds(t, N), st, t, Q, N, K, L, theta, phi, F2, r_fd_K,
                     bdiv_K, Rb, u, ceps, hdiam, out);
}

}  // namespace lrbms3

extern "C" {

int lrbms3_assemble_source_gram(lrbms3_ctx* ctx, int32_t K, const double* f_smp_K, double* F2, void* stream) {
  LRBMS_REQUIRE_MESH(ctx);
  const T3& t = ctx->t;
  if (t.S_ext != t.S) return lrbms_fail(ctx, LRBMS_E_INVALID, "assemble_source_gram: needs all subdomains on this rank");
  if (K < 1 || K > 64) return lrbms_fail(ctx, LRBMS_E_INVALID, "assemble_source_gram: K must be in [1, 64]");
  if (!f_smp_K || !F2) return lrbms_fail(ctx, LRBMS_E_INVALID, "assemble_source_gram: null argument");
  hipLaunchKernelGGL(k3_source_gram, dim3(t.S, K * (K + 1) / 2), dim3(256), 0, (hipStream_t)stream, t, K, (long)t.S * t.nT * t.f_stride,
                     f_smp_K, F2);
  LRBMS_LAUNCH_CHECK(ctx);
  return LRBMS_OK;
}

int lrbms3_project_sources(lrbms3_ctx* ctx, int32_t Q, int32_t N, int32_t K, const double* b_K, const double* bdiv_K, const double* V,
                           const double* R_self, double* rhs_red_K, double* r_fd_K, void* stream) {
  LRBMS_REQUIRE_MESH(ctx);
  const T3& t = ctx->t;
  if (t.S_ext != t.S) return lrbms_fail(ctx, LRBMS_E_INVALID, "project_sources: needs all subdomains on this rank");
  if (K < 1 || K > 64) return lrbms_fail(ctx, LRBMS_E_INVALID, "project_sources: K must be in [1, 64]");
  if (Q < 1 || Q > 8 || N < 1 || N > 64 || Q * N > 64) return lrbms_fail(ctx, LRBMS_E_INVALID, "project_sources: needs N <= 64 and Q N <= 64");
  if (!b_K || !bdiv_K || !V || !R_self || !rhs_red_K || !r_fd_K) return lrbms_fail(ctx, LRBMS_E_INVALID, "project_sources: null argument");
  hipStream_t st = (hipStream_t)stream;
  const int* list = ctx->sub_active ? ctx->sub_own : nullptr;      // lrbms3_pass_set_subset: the rows of the own list only
  const int cnt = ctx->sub_active ? ctx->sub_own_n : t.S;
  if (cnt <= 0) return LRBMS_OK;
  const dim3 grid(cnt, 2);
#define PSCASE(T)                                                                                                                  \
  case T:                                                                                                                          \
    hipLaunchKernelGGL(k3_project_sources<T>, grid, dim3(512), 0, st, t, N, Q * N, K, list, b_K, bdiv_K, V, R_self, rhs_red_K, r_fd_K); \
    break
  switch ((K + 15) / 16) {
    PSCASE(1);
    PSCASE(2);
    PSCASE(3);
    PSCASE(4);
  }
#undef PSCASE
  LRBMS_LAUNCH_CHECK(ctx);
  return LRBMS_OK;
}

int lrbms3_reduced_source_terms(lrbms3_ctx* ctx, int32_t Q, int32_t N, int32_t K, int32_t L, const double* theta, const double* phi,
                                const double* F2, const double* r_fd_K, const double* bdiv_K, const double* Rb, const double* u,
                                const double* ceps, double hdiam, double* out, void* stream) {
  LRBMS_REQUIRE_MESH(ctx);
  const T3& t = ctx->t;
  if (t.S_ext != t.S) return lrbms_fail(ctx, LRBMS_E_INVALID, "reduced_source_terms: needs all subdomains on this rank");
  if (Q < 1 || Q > 8 || N < 1 || N > 64 || K < 1 || K > 64 || L < 1 || (L + 7) / 8 > 65535)
    return lrbms_fail(ctx, LRBMS_E_INVALID, "reduced_source_terms: bad N / L / K / Q");
  if (!theta || !phi || !F2 || !r_fd_K || !bdiv_K || !Rb || !u || !ceps || !out)
    return lrbms_fail(ctx, LRBMS_E_INVALID, "reduced_source_terms: null argument");
  if (!source_terms_fits(ctx, N)) return lrbms_fail(ctx, LRBMS_E_INVALID, "reduced_source_terms: the side faces of this template do not fit the LDS");
  launch_source_terms((hipStream_t)stream, t, Q, N, K, L, theta, phi, F2, r_fd_K, bdiv_K, Rb, u, ceps, hdiam, out);
  LRBMS_LAUNCH_CHECK(ctx);
  return LRBMS_OK;
}

int lrbms3_combine_sources(lrbms3_ctx* ctx, int32_t K, int64_t M, const double* phi, const double* x_K, double* y, void* stream) {
  if (!ctx) return LRBMS_E_INVALID;
  if (!phi || !x_K || !y) return lrbms_fail(ctx, LRBMS_E_INVALID, "combine_sources: null argument");
  return launch_combine_sources_base(ctx, &ctx->num_cus, K, (long)M, phi, x_K, y, (hipStream_t)stream);
}

}  // extern "C"
