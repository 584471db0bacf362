// Local POD basis extension: the batched method of snapshots per subdomain.
//
// Per subdomain s, independently: snapshots U [n][L], basis slab V [n][Nw] with nloc[s] product-orthonormal columns and zero
// columns behind them, local product P (applied by the path's own launcher, PodProduct).
//   1  norm0 = max_j sqrt(u_j^T P u_j)
//   2  R = U, twice: R -= V (V^T P R)                                   k_pod_xty<false> + k_pod_xt
//   3  G = sym(R^T P R)                                                 k_pod_xty<true>: upper 16 x 16 tiles, mirrored
//   4  G = Z diag(lam) Z^T, lam descending                              k_pod_eigh mode 0
//   5  k = min(#{sigma_j > max(atol, rtol norm0)}, modes, Nw - nloc)    k_pod_select
//   6  W = R Z_k Sigma_k^-1                                             k_pod_xt
//   7  W -= V (V^T P W)
//   8  G2 = sym(W^T P W), W <- W G2^{-1/2} (Loewdin)                    k_pod_eigh mode 1
//   9  V[:, nloc .. nloc + k) = W, nloc += k                            k_pod_xt (writes k columns, nothing else) + k_pod_finish
// Everything runs on the caller's stream, without host synchronisation and without atomics; every sum has a fixed order (the
// reduction over n runs chunk by chunk, a split over n is summed split by split), so repeat calls give the same bits.
//
// MFMA mapping (v_mfma_f64_16x16x4_f64) as in gemm.hip: A operand lane l holds X[k = l>>4][i = l&15], B operand lane l holds
// Y[k = l>>4][j = l&15], both read from K-major LDS chunks whose rows are padded by 16 doubles; C/D lane l holds rows
// (l>>4) + 4 r of column l&15.  One workgroup works on ALL tiles of a subdomain: a staged chunk of X and Y is read from HBM once.
#include <math.h>

#include "lrbms_pod.h"

namespace {

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int XK = 16;            // rows of a staged chunk
constexpr int XW = 128;           // columns of a staged chunk (>= L, Nw)
constexpr int XPAD = 16;
constexpr int XT = 9;             // tiles per wave: 36 upper tiles of 8 x 8 (symmetric), 32 of 4 x 8 (V^T P R)
constexpr int SPLIT_ROWS = 512;   // the reduction over n is split into pieces of this many rows ...
constexpr int SPLIT_MAX = 8;      // ... at most this many (3D: n = 3840 -> 8 pieces of 480 rows)

__host__ __device__ inline int pod_nsplit(int n) {
  if (n <= SPLIT_ROWS) return 1;
  const int p = (n + SPLIT_ROWS - 1) / SPLIT_ROWS;
  return p < SPLIT_MAX ? p : SPLIT_MAX;
}

// G[s] (Mx x My) = X[s]^T Y[s] over the rows of piece blockIdx.y; X [S][n][Mx], Y [S][n][My].
// SYM (Mx == My): only the tiles ti <= tj are computed; with one piece the epilogue writes G[i][j] = G[j][i] = x_i^T y_j (i <= j).
// With nsplit > 1 the raw tiles go to part [S][nsplit][Mx][My] (SYM: the upper tiles only) and k_pod_xty_sum adds them.
template <bool SYM>
__global__ __launch_bounds__(256) void k_pod_xty(int n, int Mx, int My, int nsplit, const double* __restrict__ X,
                                                 const double* __restrict__ Y, double* __restrict__ G) {
  __shared__ double Xs[XK][XW + XPAD];
  __shared__ double Ys[XK][XW + XPAD];
  const int s = blockIdx.x, sp = blockIdx.y;
  X += (long)s * n * Mx;
  Y += (long)s * n * My;
  G += ((long)s * nsplit + sp) * Mx * My;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int li = lane & 15, lk = lane >> 4;
  const int TX = (Mx + 15) >> 4, TY = (My + 15) >> 4;
  const int ntile = SYM ? TX * (TX + 1) / 2 : TX * TY;
  // rows of this piece: whole chunks of XK rows, the same plan for every call with this n
  const int chunks = (n + XK - 1) / XK, per = (chunks + nsplit - 1) / nsplit;
  const int k_begin = sp * per * XK, k_end = min(n, (sp + 1) * per * XK);

  int ti[XT], tj[XT];
  d4 acc[XT];
#pragma unroll
  for (int t = 0; t < XT; ++t) {
    const int id = wave + 4 * t;
    acc[t] = (d4){0.0, 0.0, 0.0, 0.0};
    ti[t] = tj[t] = -1;
    if (id < ntile) {
      if (SYM) {
        int a = 0, rem = id;
        while (rem >= TX - a) {
          rem -= TX - a;
          ++a;
        }
        ti[t] = a;
        tj[t] = a + rem;
      } else {
        ti[t] = id / TY;
        tj[t] = id - ti[t] * TY;
      }
    }
  }

  const int srow = tid >> 4, scol = tid & 15;      // staging: thread -> row srow, columns scol + 16 c
  for (int k0 = k_begin; k0 < k_end; k0 += XK) {
    const int kr = k0 + srow;
    double xv[8], yv[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const int col = scol + 16 * c;
      xv[c] = (kr < k_end && col < Mx) ? X[(long)kr * Mx + col] : 0.0;
      yv[c] = (kr < k_end && col < My) ? Y[(long)kr * My + col] : 0.0;
    }
    __syncthreads();      // previous chunk fully consumed
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      Xs[srow][scol + 16 * c] = xv[c];
      Ys[srow][scol + 16 * c] = yv[c];
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < XK; kk += 4) {
#pragma unroll
      for (int t = 0; t < XT; ++t)
        if (ti[t] >= 0)      // wave-uniform
          acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(Xs[kk + lk][ti[t] * 16 + li], Ys[kk + lk][tj[t] * 16 + li], acc[t], 0, 0, 0);
    }
  }

#pragma unroll
  for (int t = 0; t < XT; ++t) {
    if (ti[t] < 0) continue;
    const int col = tj[t] * 16 + li;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = ti[t] * 16 + lk + 4 * r;
      if (row >= Mx || col >= My) continue;
      if (!SYM || nsplit > 1) {
        G[(long)row * My + col] = acc[t][r];
      } else if (row <= col) {
        G[(long)row * My + col] = acc[t][r];
        G[(long)col * My + row] = acc[t][r];
      }
    }
  }
}

// G[s][i][j] = sum over the pieces, in their order, of part[s][piece][i][j]; SYM: of the entry (min(i,j), max(i,j))
__global__ __launch_bounds__(256) void k_pod_xty_sum(int Mx, int My, int nsplit, int sym, const double* __restrict__ part,
                                                     double* __restrict__ G) {
  const int s = blockIdx.y;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= Mx * My) return;
  int i = idx / My, j = idx - i * My;
  if (sym && i > j) {
    const int h = i;
    i = j;
    j = h;
  }
  const double* p = part + (long)s * nsplit * Mx * My + (long)i * My + j;
  double acc = 0.0;
  for (int q = 0; q < nsplit; ++q) acc += p[(long)q * Mx * My];
  G[(long)s * Mx * My + idx] = acc;
}

// out[s][i][off_s + j] (+)= alpha sum_k X[s][i][k] T[s][k][j],  j < cnt_s.   X [S][n][ldx] (columns < Kin), T [S][Kin][ldt],
// out [S][n][ldo]; off (nullptr: 0) and cnt (nullptr: J) per subdomain, on the device.  Columns outside [off_s, off_s + cnt_s)
// are not touched.  Workgroup = 32 rows of one subdomain; the sum over k runs in index order.
constexpr int TR = 32;
__global__ __launch_bounds__(256) void k_pod_xt(int n, int Kin, int J, const double* __restrict__ X, int ldx, const double* __restrict__ T,
                                                int ldt, double* out, int ldo, const int32_t* __restrict__ off,
                                                const int32_t* __restrict__ cnt, double alpha, int accumulate) {
  __shared__ double Xs[TR][XW + 1];
  const int s = blockIdx.y, r0 = blockIdx.x * TR;
  const int tid = threadIdx.x;
  int o = off ? off[s] : 0, c = cnt ? cnt[s] : J;
  if (c > J) c = J;
  if (o < 0 || o + c > ldo) c = 0;           // never past the row
  if (c <= 0) return;                         // (uniform over the workgroup)
  X += (long)s * n * ldx;
  T += (long)s * Kin * ldt;
  out += (long)s * n * ldo;
  for (int idx = tid; idx < TR * Kin; idx += 256) {
    const int r = idx / Kin, k = idx - r * Kin;
    Xs[r][k] = r0 + r < n ? X[(long)(r0 + r) * ldx + k] : 0.0;
  }
  __syncthreads();
  const int jl = tid & 63, rg = (tid >> 6) * 8;
  for (int j = jl; j < c; j += 64) {
    double acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int k = 0; k < Kin; ++k) {
      const double t = T[(long)k * ldt + j];
#pragma unroll
      for (int r = 0; r < 8; ++r) acc[r] = fma(Xs[rg + r][k], t, acc[r]);
    }
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int row = r0 + rg + r;
      if (row < n) {
        double* p = out + (long)row * ldo + o + j;
        *p = accumulate ? *p + alpha * acc[r] : alpha * acc[r];
      }
    }
  }
}

// norm0sq[s] = max_j max(u_j^T (P u)_j, 0)
__global__ __launch_bounds__(256) void k_pod_norm0(int n, int L, const double* __restrict__ U, const double* __restrict__ PU,
                                                   double* __restrict__ norm0sq) {
  __shared__ double part[2][XW];
  const int s = blockIdx.x, j = threadIdx.x & 127, h = threadIdx.x >> 7;
  U += (long)s * n * L;
  PU += (long)s * n * L;
  double acc = 0.0;
  if (j < L)
    for (int i = h; i < n; i += 2) acc = fma(U[(long)i * L + j], PU[(long)i * L + j], acc);
  part[h][j] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double m = 0.0;
    for (int q = 0; q < L; ++q) {
      const double v = part[0][q] + part[1][q];
      if (v > m) m = v;
    }
    norm0sq[s] = m;
  }
}

__device__ inline double block_sum(double* red, double v) {
  const int tid = threadIdx.x;
  __syncthreads();
  red[tid] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  return red[0];
}

// Batched symmetric eigen-solver: one workgroup per matrix, two-sided cyclic Jacobi in the round-robin ("tournament") ordering:
// Lp - 1 rounds of Lp / 2 disjoint rotations per sweep, Lp = L rounded up to even (the padded row / column is zero, every rotation
// with it is the identity and it stays exactly zero; so does the row / column of a zero snapshot).  G sits in LDS with rows of
// Lp + 1 doubles.  Z^T (eigenvector of column j in row j, so that a rotation works on two contiguous rows) sits in LDS behind it
// when both fit (ZLDS: Lp <= 96), otherwise in `Zw` in global memory, where the workgroup's 128 KB stay in L2.
// A rotation zeroes its (p, q) entry exactly and updates the two diagonal entries by the t-formulas, so the off-diagonal norm
// falls below eps |G|_F; that is the convergence test, once per sweep, at most `max_sweeps` sweeps (info bit 0 otherwise).
// Entries of at most eps |G|_F / Lp are not rotated (zero entries among them: the identity, exactly).
template <bool ZLDS>
__global__ __launch_bounds__(256) void k_pod_eigh(int L, int mode, int max_sweeps, const double* __restrict__ Gin,
                                                  const int32_t* __restrict__ kcount, double* __restrict__ lam_out,
                                                  double* __restrict__ Zout, int32_t* __restrict__ info, double* Zw) {
  extern __shared__ double lds[];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int Lp = L + (L & 1), ld = Lp + 1, half = Lp >> 1;
  double* Gs = lds;                                    // [Lp][ld]
  double* Zt = ZLDS ? Gs + Lp * ld : Zw + (long)b * Lp * Lp;
  const int ldz = ZLDS ? ld : Lp;
  double* tail = Gs + (ZLDS ? 2 : 1) * Lp * ld;
  double* red = tail;                                  // [256]
  double* rc = red + 256;                              // [64] cosines
  double* rs = rc + 64;                                // [64] sines
  double* dp = rs + 64;                                // [64] new G[p][p]
  double* dq = dp + 64;                                // [64] new G[q][q]
  double* lam = dq + 64;                               // [128]
  int* rp = (int*)(lam + 128);                         // [64]
  int* rq = rp + 64;                                   // [64]
  int* rank = rq + 64;                                 // [128]
  Gin += (long)b * L * L;

  for (int idx = tid; idx < Lp * Lp; idx += 256) {
    const int i = idx / Lp, j = idx - i * Lp;
    Gs[i * ld + j] = (i < L && j < L) ? 0.5 * (Gin[i * L + j] + Gin[j * L + i]) : 0.0;
    Zt[i * ldz + j] = i == j ? 1.0 : 0.0;
  }
  __syncthreads();
  double fro2 = 0.0;
  for (int idx = tid; idx < Lp * Lp; idx += 256) {
    const double g = Gs[(idx / Lp) * ld + idx % Lp];
    fro2 = fma(g, g, fro2);
  }
  fro2 = block_sum(red, fro2);
  const double eps = 2.220446049250313e-16;
  const double tol2 = eps * eps * fro2;
  const double small = eps * sqrt(fro2) / Lp;      // entries up to it are left alone: rotating rounding noise inside a cluster of
                                                   // equal eigenvalues stalls the iteration; all of them that small = converged

  int converged = 0;
  for (int sweep = 0; sweep <= max_sweeps; ++sweep) {
    double off2 = 0.0;
    for (int idx = tid; idx < Lp * Lp; idx += 256) {
      const int i = idx / Lp, j = idx - i * Lp;
      const double g = Gs[i * ld + j];
      if (i != j) off2 = fma(g, g, off2);
    }
    off2 = block_sum(red, off2);
    if (off2 <= tol2) {          // also NaN-free exit: a NaN never compares true, the cap ends the loop
      converged = 1;
      break;
    }
    if (sweep == max_sweeps) break;
    for (int round = 0; round < Lp - 1; ++round) {
      if (tid < half) {
        const int m = Lp - 1;
        int a = tid == 0 ? m : (round + tid) % m;
        int c = tid == 0 ? round : (round - tid + m) % m;
        const int p = a < c ? a : c, q = a < c ? c : a;
        const double app = Gs[p * ld + p], aqq = Gs[q * ld + q], apq = Gs[p * ld + q];
        double cs = 1.0, sn = 0.0, t = 0.0;
        if (fabs(apq) > small) {
          const double tau = (aqq - app) / (2.0 * apq);
          t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
          cs = 1.0 / sqrt(1.0 + t * t);
          sn = t * cs;
        }
        rp[tid] = p;
        rq[tid] = q;
        rc[tid] = cs;
        rs[tid] = sn;
        dp[tid] = app - t * apq;
        dq[tid] = aqq + t * apq;
      }
      __syncthreads();
      // columns: G <- G J (every row i), and the rows of Z^T
      for (int idx = tid; idx < half * Lp; idx += 256) {
        const int k = idx / Lp, i = idx - k * Lp;
        const double cs = rc[k], sn = rs[k];
        if (sn == 0.0) continue;
        const int p = rp[k], q = rq[k];
        const double gp = Gs[i * ld + p], gq = Gs[i * ld + q];
        Gs[i * ld + p] = cs * gp - sn * gq;
        Gs[i * ld + q] = sn * gp + cs * gq;
        const double zp = Zt[p * ldz + i], zq = Zt[q * ldz + i];
        Zt[p * ldz + i] = cs * zp - sn * zq;
        Zt[q * ldz + i] = sn * zp + cs * zq;
      }
      __syncthreads();
      // rows: G <- J^T G (every column j); the 2 x 2 block of the pair gets its exact values
      for (int idx = tid; idx < half * Lp; idx += 256) {
        const int k = idx / Lp, j = idx - k * Lp;
        const double cs = rc[k], sn = rs[k];
        if (sn == 0.0) continue;
        const int p = rp[k], q = rq[k];
        const double gp = Gs[p * ld + j], gq = Gs[q * ld + j];
        double np_ = cs * gp - sn * gq, nq_ = sn * gp + cs * gq;
        if (j == p) {
          np_ = dp[k];
          nq_ = 0.0;
        } else if (j == q) {
          np_ = 0.0;
          nq_ = dq[k];
        }
        Gs[p * ld + j] = np_;
        Gs[q * ld + j] = nq_;
      }
      __syncthreads();
    }
  }

  // descending order, ties by index: rank[j] = position of column j
  if (tid < XW) lam[tid] = tid < L ? Gs[tid * ld + tid] : 0.0;
  __syncthreads();
  if (tid < L) {
    const double v = lam[tid];
    int r = 0;
    for (int i = 0; i < L; ++i) {
      const double w = lam[i];
      r += (w > v || (w == v && i < tid) || (v != v && w == w)) ? 1 : 0;      // (a NaN sorts last)
    }
    rank[tid] = r;
    lam_out[(long)b * L + r] = v;
  }
  __syncthreads();
  int flags = converged ? 0 : 1;
  Zout += (long)b * L * L;
  if (mode == 0) {
    for (int idx = tid; idx < L * L; idx += 256) {
      const int j = idx / L, i = idx - j * L;
      Zout[rank[j] * L + i] = Zt[j * ldz + i];
    }
  } else {
    // Loewdin factor over the kc largest eigenpairs: H = sum_j z_j z_j^T / sqrt(lam_j), the sum in column order, upper part mirrored
    int kc = kcount ? kcount[b] : L;
    if (kc > L) kc = L;
    double w = 0.0;
    if (tid < L && rank[tid] < kc) {
      if (lam[tid] > 0.0) w = 1.0 / sqrt(lam[tid]);
      else flags |= 2;
    }
    if (tid < XW) rc[tid] = w;      // (rc and rs are free now: 128 doubles in a row hold the weights)
    __syncthreads();
    for (int idx = tid; idx < L * L; idx += 256) {
      const int a = idx / L, c = idx - a * L;
      if (a > c) continue;
      double h = 0.0;
      for (int j = 0; j < L; ++j) h = fma(Zt[j * ldz + a] * rc[j], Zt[j * ldz + c], h);
      Zout[a * L + c] = h;
      Zout[c * L + a] = h;
    }
  }
  // info: OR over the workgroup in a fixed order
  const double f = block_sum(red, (double)(flags & 2));
  if (tid == 0) info[b] = (converged ? 0 : 1) | (f > 0.0 ? 2 : 0);
}

// sigma, the retained count and the coefficients of the modes: T [L][K], column j = z_j / sigma_j for j < k, 0 behind
__global__ __launch_bounds__(128) void k_pod_select(int L, int Nw, int modes, int K, double rtol, double atol,
                                                    const double* __restrict__ lam, const double* __restrict__ Zs,
                                                    const double* __restrict__ norm0sq, const int32_t* __restrict__ nloc,
                                                    double* __restrict__ sv, int32_t* __restrict__ ks, int32_t* __restrict__ added,
                                                    double* __restrict__ T) {
  __shared__ double sig[XW];
  __shared__ int kk;
  const int s = blockIdx.x, tid = threadIdx.x;
  lam += (long)s * L;
  Zs += (long)s * L * L;
  T += (long)s * L * K;
  const double thr = fmax(atol, rtol * sqrt(fmax(norm0sq[s], 0.0)));
  if (tid < L) {
    const double l = lam[tid];
    const double sg = l > 0.0 ? sqrt(l) : 0.0;
    sig[tid] = sg;
    sv[(long)s * L + tid] = sg;
  }
  __syncthreads();
  if (tid == 0) {
    int cnt = 0;
    while (cnt < L && sig[cnt] > thr) ++cnt;          // descending: the retained values come first
    const int nl = nloc[s];
    const int room = (nl >= 0 && nl <= Nw) ? Nw - nl : 0;
    int k = cnt < modes ? cnt : modes;
    k = k < room ? k : room;
    k = k < K ? k : K;
    kk = k;
    ks[s] = k;
    added[s] = k;
  }
  __syncthreads();
  const int k = kk;
  for (int idx = tid; idx < L * K; idx += 128) {
    const int i = idx / K, j = idx - i * K;
    T[idx] = j < k ? Zs[j * L + i] / sig[j] : 0.0;
  }
}

__global__ void k_pod_finish(int S, const int32_t* __restrict__ ks, const int32_t* __restrict__ ia, const int32_t* __restrict__ ib,
                             int32_t* __restrict__ nloc, int32_t* __restrict__ info) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  nloc[s] += ks[s];
  info[s] = ia[s] | (ib[s] << 2);
}

constexpr int EIGH_TAIL = 256 + 4 * 64 + 128 + (64 + 64 + 128) / 2;      // doubles behind the matrices
constexpr int EIGH_ZLDS_MAX = 96;
constexpr int EIGH_SWEEPS = 40;

size_t eigh_lds_bytes(int L, bool zlds) {
  const int Lp = L + (L & 1);
  return sizeof(double) * ((size_t)(zlds ? 2 : 1) * Lp * (Lp + 1) + EIGH_TAIL);
}

int xty(lrbms_ctx_base* ctx, bool sym, int S, int n, int Mx, int My, const double* X, const double* Y, double* G, double* part,
        hipStream_t st) {
  const int ns = pod_nsplit(n);
  double* dst = ns > 1 ? part : G;
  KScope ks(ctx, sym ? "k_pod_xty<sym>" : "k_pod_xty", st);
  if (sym) hipLaunchKernelGGL((k_pod_xty<true>), dim3(S, ns), dim3(256), 0, st, n, Mx, My, ns, X, Y, dst);
  else hipLaunchKernelGGL((k_pod_xty<false>), dim3(S, ns), dim3(256), 0, st, n, Mx, My, ns, X, Y, dst);
  if (ns > 1)
    hipLaunchKernelGGL(k_pod_xty_sum, dim3((Mx * My + 255) / 256, S), dim3(256), 0, st, Mx, My, ns, sym ? 1 : 0, (const double*)part, G);
  LRBMS_LAUNCH_CHECK(ctx);
  return LRBMS_OK;
}

int xt(lrbms_ctx_base* ctx, int S, int n, int Kin, int J, const double* X, int ldx, const double* T, int ldt, double* out, int ldo,
       const int32_t* off, const int32_t* cnt, double alpha, int accumulate, hipStream_t st) {
  KScope ks(ctx, "k_pod_xt", st);
  hipLaunchKernelGGL(k_pod_xt, dim3((n + TR - 1) / TR, S), dim3(256), 0, st, n, Kin, J, X, ldx, T, ldt, out, ldo, off, cnt, alpha,
                     accumulate);
  LRBMS_LAUNCH_CHECK(ctx);
  return LRBMS_OK;
}

// Steps 7 - 9 of the local POD, shared by launch_local_pod and the stream's finish: W [S][n][K] (ks[s] columns in use) is deflated
// once more against V, re-orthonormalised (Loewdin) and written into the columns nloc[s] .. nloc[s] + ks[s] - 1 of V; nloc += ks,
// info = ia | ib << 2.  PR [S][n][K], C [S][Nw][K], G, Zs [S][K][K], Zw (pod_eigh_work_size(S, K)), lam [S][K] are scratch.
int pod_tail(lrbms_ctx_base* ctx, int S, int n, int Nw, int K, PodProduct P, double* V, int32_t* nloc, double* Wb, double* PR, double* C,
             double* G, double* Zs, double* Zw, double* lam, const int32_t* ks, const int32_t* ia, int32_t* ib, double* part,
             int32_t* info, hipStream_t st) {
  int rc;
  // 7: once more against V
  if ((rc = P.apply(P.self, K, Wb, PR, st)) != LRBMS_OK) return rc;
  if ((rc = xty(ctx, false, S, n, Nw, K, V, PR, C, part, st)) != LRBMS_OK) return rc;
  if ((rc = xt(ctx, S, n, Nw, K, V, Nw, C, K, Wb, K, nullptr, nullptr, -1.0, 1, st)) != LRBMS_OK) return rc;
  // 8: symmetric re-orthonormalisation
  if ((rc = P.apply(P.self, K, Wb, PR, st)) != LRBMS_OK) return rc;
  if ((rc = xty(ctx, true, S, n, K, K, Wb, PR, G, part, st)) != LRBMS_OK) return rc;
  if ((rc = launch_pod_eigh(ctx, S, K, 1, G, ks, lam, Zs, ib, Zw, st)) != LRBMS_OK) return rc;
  // 9: into the free columns of V
  if ((rc = xt(ctx, S, n, K, K, Wb, K, Zs, K, V, Nw, nloc, ks, 1.0, 0, st)) != LRBMS_OK) return rc;
  hipLaunchKernelGGL(k_pod_finish, dim3((S + 255) / 256), dim3(256), 0, st, S, (const int32_t*)ks, (const int32_t*)ia,
                     (const int32_t*)ib, nloc, info);
  LRBMS_LAUNCH_CHECK(ctx);
  return LRBMS_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Streamed local POD (incremental HAPOD).  Per subdomain the state carries the panels X = [B | R] and
// PX = [PB | PR], both [n][Lx], Lx = keep + cmax: columns < kb hold the carried modes scaled by their singular values, the columns
// from keep on the deflated chunk of the current push; everything else is zero.
constexpr int RS_ROWS = 32;       // rows of a staged tile of the rotate kernel
constexpr int RS_LDX = 130;       // its row length in LDS: 2 mod 32 doubles, the A operand's 16 rows x 4 k then hit every bank pair twice
constexpr int RS_NK = POD_MAX_L / 4;      // k-steps of the MFMA at most

// In place: X[s][:, :keep] = X[s] T[s], PX[s][:, :keep] = PX[s] T[s] with T [S][Lx][keep]; the columns j >= kb[s] get exact zeros.
// A workgroup owns the rows [blockIdx.y rows_per_wg, ...) of subdomain blockIdx.x in both panels.  Wave w owns the 16 columns
// 16 w .. 16 w + 15 of the result (keep <= 64: four waves) and keeps its slice of T, the B operand of every k-step, in registers
// for the whole kernel; tile by tile, RS_ROWS whole rows are staged in LDS (row-major, the A operand of both row tiles), and the
// tile's columns < keep are written only after the barrier behind its staging -- nobody else reads these rows.  33 KB of static
// LDS: four workgroups per CU.  The sum over k runs in index order, four at a time.
__global__ __launch_bounds__(256) void k_pod_stream_rotate(int n, int Lx, int keep, int rows_per_wg, double* X, double* PX,
                                                           const double* __restrict__ T, const int32_t* __restrict__ kb) {
  __shared__ double Xs[RS_ROWS * RS_LDX];
  const int s = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int li = lane & 15, lk = lane >> 4;
  const int K4 = (Lx + 3) & ~3, nk = K4 >> 2;
  const int col = wave * 16 + li;
  const bool active = wave * 16 < keep;      // wave-uniform
  T += (long)s * Lx * keep;
  double b[RS_NK];
#pragma unroll
  for (int q = 0; q < RS_NK; ++q) {
    const int k = 4 * q + lk;
    b[q] = (q < nk && k < Lx && col < keep) ? T[(long)k * keep + col] : 0.0;
  }
  int kbs = kb[s];
  kbs = kbs < 0 ? 0 : (kbs > keep ? keep : kbs);
  const int row_begin = blockIdx.y * rows_per_wg, row_end = min(n, row_begin + rows_per_wg);
  const double* xa0 = Xs + li * RS_LDX + lk;
  const double* xa1 = xa0 + 16 * RS_LDX;
  for (int panel = 0; panel < 2; ++panel) {
    double* A = (panel ? PX : X) + (long)s * n * Lx;
    for (int r0 = row_begin; r0 < row_end; r0 += RS_ROWS) {
      __syncthreads();      // the previous tile is consumed
      for (int idx = tid; idx < RS_ROWS * K4; idx += 256) {
        const int r = idx / K4, c = idx - r * K4;
        Xs[r * RS_LDX + c] = (r0 + r < row_end && c < Lx) ? A[(long)(r0 + r) * Lx + c] : 0.0;
      }
      __syncthreads();      // every read of these rows is done: from here on they may be written
      if (!active) continue;
      d4 acc0 = (d4){0.0, 0.0, 0.0, 0.0}, acc1 = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int q = 0; q < RS_NK; ++q) {
        if (q < nk) {      // uniform
          acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(xa0[4 * q], b[q], acc0, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(xa1[4 * q], b[q], acc1, 0, 0, 0);
        }
      }
      if (col < keep) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = r0 + lk + 4 * r;
          if (row < row_end) A[(long)row * Lx + col] = col < kbs ? acc0[r] : 0.0;
          if (row + 16 < row_end) A[(long)(row + 16) * Lx + col] = col < kbs ? acc1[r] : 0.0;
        }
      }
    }
  }
}

// X[s][i][keep + j] = R[s][i][j], PX likewise from PR (R, PR [S][n][C]) for j < C, zero for C <= j < Lx - keep
__global__ __launch_bounds__(256) void k_pod_stream_pack(int n, int C, int Lx, int keep, const double* __restrict__ R,
                                                         const double* __restrict__ PR, double* __restrict__ X, double* __restrict__ PX) {
  const int s = blockIdx.y, W = Lx - keep;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)n * W) return;
  const int i = (int)(idx / W), j = (int)(idx - (long)i * W);
  const long src = ((long)s * n + i) * C + j, dst = ((long)s * n + i) * Lx + keep + j;
  X[dst] = j < C ? R[src] : 0.0;
  PX[dst] = j < C ? PR[src] : 0.0;
}

// dst0[s][i][j] = src0[s][i][j], dst1 from src1, j < W: the leading columns between two row lengths
__global__ __launch_bounds__(256) void k_pod_stream_copy(int n, int W, const double* __restrict__ src0, const double* __restrict__ src1,
                                                         int lds_, double* __restrict__ dst0, double* __restrict__ dst1, int ldd) {
  const int s = blockIdx.y;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)n * W) return;
  const int i = (int)(idx / W), j = (int)(idx - (long)i * W);
  const long a = ((long)s * n + i) * lds_ + j, b = ((long)s * n + i) * ldd + j;
  dst0[b] = src0[a];
  dst1[b] = src1[a];
}

// Node truncation of a push: kb = min(#{lam_j > (1e-7)^2 lam_1}, keep), lost += sum_{j >= kb} max(lam_j, 0) in index order,
// norm0sq = max(norm0sq, that of the chunk), flags |= the eigen-solver's; T [Lx][keep]: column j = z_j for j < kb, 0 behind.
__global__ __launch_bounds__(128) void k_pod_stream_select(int Lx, int keep, const double* __restrict__ lam, const double* __restrict__ Zs,
                                                           const double* __restrict__ nrm, const int32_t* __restrict__ ia,
                                                           double* __restrict__ norm0sq, double* __restrict__ lost,
                                                           int32_t* __restrict__ kb, int32_t* __restrict__ flags, double* __restrict__ T) {
  __shared__ int kk;
  const int s = blockIdx.x, tid = threadIdx.x;
  lam += (long)s * Lx;
  Zs += (long)s * Lx * Lx;
  T += (long)s * Lx * keep;
  if (tid == 0) {
    const double floor_ = POD_MIN_RTOL * POD_MIN_RTOL * lam[0];
    int cnt = 0;
    while (cnt < Lx && cnt < keep && lam[cnt] > 0.0 && lam[cnt] > floor_) ++cnt;      // descending; a NaN ends the count
    double acc = 0.0;
    for (int j = cnt; j < Lx; ++j) acc += lam[j] > 0.0 ? lam[j] : 0.0;
    lost[s] += acc;
    const double m = nrm[s];
    if (m > norm0sq[s]) norm0sq[s] = m;
    flags[s] |= ia[s];
    kb[s] = cnt;
    kk = cnt;
  }
  __syncthreads();
  const int k = kk;
  for (int idx = tid; idx < Lx * keep; idx += 128) {
    const int i = idx / keep, j = idx - i * keep;
    T[idx] = j < k ? Zs[(long)j * Lx + i] : 0.0;
  }
}

// finish: lost_out = lost + sum_{ks <= j < keep} max(lam_j, 0), ia = flags of the pushes | that of the last eigen-solve
__global__ void k_pod_stream_final(int S, int keep, const double* __restrict__ lam, const int32_t* __restrict__ ks,
                                   const double* __restrict__ lost, const int32_t* __restrict__ flags, const int32_t* __restrict__ ia2,
                                   double* __restrict__ lost_out, int32_t* __restrict__ ia) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  double acc = 0.0;
  for (int j = ks[s] < 0 ? 0 : ks[s]; j < keep; ++j) {
    const double l = lam[(long)s * keep + j];
    acc += l > 0.0 ? l : 0.0;
  }
  lost_out[s] = lost[s] + acc;
  ia[s] = (flags[s] | ia2[s]) & 1;
}

struct StreamBuffers {
  // state
  double *X, *PX, *norm0sq, *lost;
  int32_t *kb, *flags;
  // work
  double *R, *PR, *X2, *X2b, *C, *G, *Zs, *Zw, *lam, *T, *nrm, *part;
  int32_t *ks, *ia, *ib, *ia2;
};

StreamBuffers stream_buffers(int S, int n, int keep, int cmax, int Nw, double* state, double* work) {
  const long Lx = keep + cmax, Lp = Lx + (Lx & 1), M1 = cmax > keep ? cmax : keep;
  StreamBuffers b;
  b.X = state;
  b.PX = b.X + (long)S * n * Lx;
  b.norm0sq = b.PX + (long)S * n * Lx;
  b.lost = b.norm0sq + S;
  b.kb = (int32_t*)(b.lost + S);
  b.flags = b.kb + S;
  b.R = work;
  b.PR = b.R + (long)S * n * M1;
  b.X2 = b.PR + (long)S * n * M1;
  b.X2b = b.X2 + (long)S * n * keep;
  b.C = b.X2b + (long)S * n * keep;
  b.G = b.C + (long)S * Nw * M1;
  b.Zs = b.G + (long)S * Lx * Lx;
  b.Zw = b.Zs + (long)S * Lx * Lx;
  b.lam = b.Zw + (long)S * Lp * Lp;
  b.T = b.lam + (long)S * Lx;
  b.nrm = b.T + (long)S * Lx * keep;
  b.ks = (int32_t*)(b.nrm + S);      // 3 doubles = 6 int32 per subdomain, four in use
  b.ia = b.ks + S;
  b.ib = b.ia + S;
  b.ia2 = b.ib + S;
  b.part = b.nrm + 4L * S;
  return b;
}

int stream_check(lrbms_ctx_base* ctx, int S, int n, int keep, int cmax) {
  if (S < 1 || S > 65535 || n < 1) return lrbms_fail(ctx, LRBMS_E_INVALID, "local_pod_stream: S in [1, 65535], n >= 1");
  if (keep < 1 || keep > POD_MAX_NW) return lrbms_fail(ctx, LRBMS_E_INVALID, "local_pod_stream: keep must be in [1, 64]");
  if (cmax < 1) return lrbms_fail(ctx, LRBMS_E_INVALID, "local_pod_stream: cmax must be >= 1");
  if (keep + cmax > POD_MAX_L) return lrbms_fail(ctx, LRBMS_E_INVALID, "local_pod_stream: keep + cmax must be <= 128");
  return LRBMS_OK;
}

}  // namespace

int64_t pod_stream_state_size(int S, int n, int keep, int cmax) {
  const int64_t Lx = keep + cmax;
  return (int64_t)S * (2 * (int64_t)n * Lx + 3);
}

int64_t pod_stream_work_size(int S, int n, int keep, int cmax, int Nw) {
  const int64_t Lx = keep + cmax, Lp = Lx + (Lx & 1), M1 = cmax > keep ? cmax : keep, M = Lx > Nw ? Lx : Nw;
  const int ns = pod_nsplit(n);
  return (int64_t)S * (2 * (int64_t)n * M1 + 2 * (int64_t)n * keep + Nw * M1 + 2 * Lx * Lx + Lp * Lp + Lx + Lx * keep + 4 +
                       (ns > 1 ? (int64_t)ns * M * Lx : 0));
}

int launch_pod_stream_begin(lrbms_ctx_base* ctx, int S, int n, int keep, int cmax, double* state, hipStream_t st) {
  int rc;
  if ((rc = stream_check(ctx, S, n, keep, cmax)) != LRBMS_OK) return rc;
  if (!state) return lrbms_fail(ctx, LRBMS_E_INVALID, "local_pod_stream_begin: null pointer");
  LRBMS_HIP_CHECK(ctx, hipMemsetAsync(state, 0, sizeof(double) * (size_t)pod_stream_state_size(S, n, keep, cmax), st));
  return LRBMS_OK;
}

int launch_pod_stream_push(lrbms_ctx_base* ctx, int S, int n, int keep, int cmax, int C, int Nw, int rotate_valu, PodProduct P,
                           const double* U, const double* V, const int32_t* nloc, double* state, double* work, hipStream_t st) {
  int rc;
  if ((rc = stream_check(ctx, S, n, keep, cmax)) != LRBMS_OK) return rc;
  if (C < 1 || C > cmax) return lrbms_fail(ctx, LRBMS_E_INVALID, "local_pod_stream_push: the chunk width C must be in [1, cmax]");
  if (Nw < 1 || Nw > POD_MAX_NW) return lrbms_fail(ctx, LRBMS_E_INVALID, "local_pod_stream_push: the slab width Nw must be in [1, 64]");
  if (!U || !V || !nloc || !state || !work) return lrbms_fail(ctx, LRBMS_E_INVALID, "local_pod_stream_push: null pointer");
  const int Lx = keep + cmax;
  const StreamBuffers b = stream_buffers(S, n, keep, cmax, Nw, state, work);

  // 1: the largest snapshot norm, of the undeflated chunk
  if ((rc = P.apply(P.self, C, U, b.PR, st)) != LRBMS_OK) return rc;
  hipLaunchKernelGGL(k_pod_norm0, dim3(S), dim3(256), 0, st, n, C, U, (const double*)b.PR, b.nrm);
  LRBMS_LAUNCH_CHECK(ctx);
  // 2: R = U, deflated twice against V
  LRBMS_HIP_CHECK(ctx, hipMemcpyAsync(b.R, U, sizeof(double) * (size_t)S * n * C, hipMemcpyDeviceToDevice, st));
  for (int pass = 0; pass < 2; ++pass) {
    if ((rc = P.apply(P.self, C, b.R, b.PR, st)) != LRBMS_OK) return rc;
    if ((rc = xty(ctx, false, S, n, Nw, C, V, b.PR, b.C, b.part, st)) != LRBMS_OK) return rc;
    if ((rc = xt(ctx, S, n, Nw, C, V, Nw, b.C, C, b.R, C, nullptr, nullptr, -1.0, 1, st)) != LRBMS_OK) return rc;
  }
  if ((rc = P.apply(P.self, C, b.R, b.PR, st)) != LRBMS_OK) return rc;
  // 3: X = [B | R], PX = [PB | PR], their Gram matrix and its eigenpairs
  {
    KScope ks(ctx, "k_pod_stream_pack", st);
    hipLaunchKernelGGL(k_pod_stream_pack, dim3((unsigned)(((long)n * cmax + 255) / 256), S), dim3(256), 0, st, n, C, Lx, keep,
                       (const double*)b.R, (const double*)b.PR, b.X, b.PX);
    LRBMS_LAUNCH_CHECK(ctx);
  }
  if ((rc = xty(ctx, true, S, n, Lx, Lx, b.X, b.PX, b.G, b.part, st)) != LRBMS_OK) return rc;
  if ((rc = launch_pod_eigh(ctx, S, Lx, 0, b.G, nullptr, b.lam, b.Zs, b.ia, b.Zw, st)) != LRBMS_OK) return rc;
  // 4: the node's truncation
  hipLaunchKernelGGL(k_pod_stream_select, dim3(S), dim3(128), 0, st, Lx, keep, (const double*)b.lam, (const double*)b.Zs,
                     (const double*)b.nrm, (const int32_t*)b.ia, b.norm0sq, b.lost, b.kb, b.flags, b.T);
  LRBMS_LAUNCH_CHECK(ctx);
  // 5: B <- X T, PB <- PX T
  if (!rotate_valu) {
    const int tiles = (n + RS_ROWS - 1) / RS_ROWS;
    int split = (2048 + S - 1) / S;                        // enough workgroups for the device, as few loads of T as that allows
    split = split < tiles ? split : tiles;
    const int rows_per_wg = ((tiles + split - 1) / split) * RS_ROWS;
    KScope ks(ctx, "k_pod_stream_rotate", st);
    hipLaunchKernelGGL(k_pod_stream_rotate, dim3(S, (n + rows_per_wg - 1) / rows_per_wg), dim3(256), 0, st, n, Lx, keep, rows_per_wg,
                       b.X, b.PX, (const double*)b.T, (const int32_t*)b.kb);
    LRBMS_LAUNCH_CHECK(ctx);
  } else {      // the VALU route: two k_pod_xt launches into a second buffer and the copy back
    if ((rc = xt(ctx, S, n, Lx, keep, b.X, Lx, b.T, keep, b.X2, keep, nullptr, nullptr, 1.0, 0, st)) != LRBMS_OK) return rc;
    if ((rc = xt(ctx, S, n, Lx, keep, b.PX, Lx, b.T, keep, b.X2b, keep, nullptr, nullptr, 1.0, 0, st)) != LRBMS_OK) return rc;
    KScope ks(ctx, "k_pod_stream_copy", st);
    hipLaunchKernelGGL(k_pod_stream_copy, dim3((unsigned)(((long)n * keep + 255) / 256), S), dim3(256), 0, st, n, keep,
                       (const double*)b.X2, (const double*)b.X2b, keep, b.X, b.PX, Lx);
    LRBMS_LAUNCH_CHECK(ctx);
  }
  return LRBMS_OK;
}

int launch_pod_stream_finish(lrbms_ctx_base* ctx, int S, int n, int keep, int cmax, int Nw, int modes, double rtol, double atol,
                             PodProduct P, double* V, int32_t* nloc, double* state, double* sv, int32_t* added, int32_t* info,
                             double* lost, double* work, hipStream_t st) {
  int rc;
  if ((rc = stream_check(ctx, S, n, keep, cmax)) != LRBMS_OK) return rc;
  if (Nw < 1 || Nw > POD_MAX_NW) return lrbms_fail(ctx, LRBMS_E_INVALID, "local_pod_stream_finish: the slab width Nw must be in [1, 64]");
  if (modes < 1) return lrbms_fail(ctx, LRBMS_E_INVALID, "local_pod_stream_finish: modes must be >= 1");
  if (!(rtol >= POD_MIN_RTOL))
    return lrbms_fail(ctx, LRBMS_E_INVALID, "local_pod_stream_finish: rtol < 1e-7: the Gram matrix squares the singular values, below 1e-7 relative they are rounding noise");
  if (!(atol >= 0.0)) return lrbms_fail(ctx, LRBMS_E_INVALID, "local_pod_stream_finish: atol must be >= 0");
  if (!V || !nloc || !state || !sv || !added || !info || !lost || !work)
    return lrbms_fail(ctx, LRBMS_E_INVALID, "local_pod_stream_finish: null pointer");
  const int Lx = keep + cmax;
  int K = modes < keep ? modes : keep;
  K = K < Nw ? K : Nw;
  const StreamBuffers b = stream_buffers(S, n, keep, cmax, Nw, state, work);

  // 1: B and PB side by side, their Gram matrix (diagonal up to rounding: the last push left B = X Z_k) and its eigenpairs
  {
    KScope ks(ctx, "k_pod_stream_copy", st);
    hipLaunchKernelGGL(k_pod_stream_copy, dim3((unsigned)(((long)n * keep + 255) / 256), S), dim3(256), 0, st, n, keep,
                       (const double*)b.X, (const double*)b.PX, Lx, b.R, b.PR, keep);
    LRBMS_LAUNCH_CHECK(ctx);
  }
  if ((rc = xty(ctx, true, S, n, keep, keep, b.R, b.PR, b.G, b.part, st)) != LRBMS_OK) return rc;
  if ((rc = launch_pod_eigh(ctx, S, keep, 0, b.G, nullptr, b.lam, b.Zs, b.ia2, b.Zw, st)) != LRBMS_OK) return rc;
  // 2, 3: selection, the energy it leaves behind
  hipLaunchKernelGGL(k_pod_select, dim3(S), dim3(128), 0, st, keep, Nw, modes, K, rtol, atol, (const double*)b.lam, (const double*)b.Zs,
                     (const double*)b.norm0sq, (const int32_t*)nloc, sv, b.ks, added, b.T);
  LRBMS_LAUNCH_CHECK(ctx);
  hipLaunchKernelGGL(k_pod_stream_final, dim3((S + 255) / 256), dim3(256), 0, st, S, keep, (const double*)b.lam, (const int32_t*)b.ks,
                     (const double*)b.lost, (const int32_t*)b.flags, (const int32_t*)b.ia2, lost, b.ia);
  LRBMS_LAUNCH_CHECK(ctx);
  // 4: W = B Z_k Sigma_k^-1 and the tail of the local POD
  if ((rc = xt(ctx, S, n, keep, K, b.R, keep, b.T, K, b.X2, K, nullptr, nullptr, 1.0, 0, st)) != LRBMS_OK) return rc;
  return pod_tail(ctx, S, n, Nw, K, P, V, nloc, b.X2, b.X2b, b.C, b.G, b.Zs, b.Zw, b.lam, b.ks, b.ia, b.ib, b.part, info, st);
}

int64_t pod_eigh_work_size(int batch, int L) {
  const int64_t Lp = L + (L & 1);
  return (int64_t)batch * Lp * Lp;
}

int64_t pod_work_size(int S, int n, int L, int Nw) {
  const int64_t Kc = L < Nw ? L : Nw, Lp = L + (L & 1), M = L > Nw ? L : Nw;
  const int ns = pod_nsplit(n);
  return (int64_t)S * (2 * (int64_t)n * L + n * Kc + (int64_t)Nw * L + 2 * (int64_t)L * L + Lp * Lp + L + L * Kc + 4 +
                       (ns > 1 ? (int64_t)ns * M * L : 0));
}

int launch_pod_gram(lrbms_ctx_base* ctx, int batch, int K, int L, const double* X, const double* Y, double* G, hipStream_t st) {
  if (batch < 1 || batch > 65535 || K < 1 || L < 1 || L > POD_MAX_L) return lrbms_fail(ctx, LRBMS_E_INVALID, "pod_gram: batch in [1, 65535], K >= 1, L in [1, 128]");
  if (!X || !Y || !G) return lrbms_fail(ctx, LRBMS_E_INVALID, "pod_gram: null pointer");
  hipLaunchKernelGGL((k_pod_xty<true>), dim3(batch, 1), dim3(256), 0, st, K, L, L, 1, X, Y, G);
  LRBMS_LAUNCH_CHECK(ctx);
  return LRBMS_OK;
}

int launch_pod_eigh(lrbms_ctx_base* ctx, int batch, int L, int mode, const double* G, const int32_t* kcount, double* lam, double* Z,
                    int32_t* info, double* work, hipStream_t st) {
  if (batch < 1 || L < 1 || L > POD_MAX_L) return lrbms_fail(ctx, LRBMS_E_INVALID, "pod_eigh: batch >= 1, L in [1, 128]");
  if (mode != 0 && mode != 1) return lrbms_fail(ctx, LRBMS_E_INVALID, "pod_eigh: mode is 0 (eigenpairs) or 1 (inverse square root)");
  if (!G || !lam || !Z || !info || !work) return lrbms_fail(ctx, LRBMS_E_INVALID, "pod_eigh: null pointer");
  const bool zlds = L <= EIGH_ZLDS_MAX;
  const size_t bytes = eigh_lds_bytes(L, zlds);
  KScope ks(ctx, mode ? "k_pod_eigh<invsqrt>" : "k_pod_eigh", st);
  if (zlds) {
    LRBMS_HIP_CHECK(ctx, hipFuncSetAttribute((const void*)k_pod_eigh<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    hipLaunchKernelGGL((k_pod_eigh<true>), dim3(batch), dim3(256), bytes, st, L, mode, EIGH_SWEEPS, G, kcount, lam, Z, info, work);
  } else {
    LRBMS_HIP_CHECK(ctx, hipFuncSetAttribute((const void*)k_pod_eigh<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    hipLaunchKernelGGL((k_pod_eigh<false>), dim3(batch), dim3(256), bytes, st, L, mode, EIGH_SWEEPS, G, kcount, lam, Z, info, work);
  }
  LRBMS_LAUNCH_CHECK(ctx);
  return LRBMS_OK;
}

int launch_local_pod(lrbms_ctx_base* ctx, int S, int n, int L, int Nw, int modes, double rtol, double atol, PodProduct P,
                     const double* U, double* V, int32_t* nloc, double* sv, int32_t* added, int32_t* info, double* work,
                     hipStream_t st) {
  if (S < 1 || S > 65535 || n < 1) return lrbms_fail(ctx, LRBMS_E_INVALID, "local_pod: S in [1, 65535], n >= 1");
  if (L < 1 || L > POD_MAX_L) return lrbms_fail(ctx, LRBMS_E_INVALID, "local_pod: L must be in [1, 128] (more snapshots: consecutive calls)");
  if (Nw < 1 || Nw > POD_MAX_NW) return lrbms_fail(ctx, LRBMS_E_INVALID, "local_pod: the slab width Nw must be in [1, 64]");
  if (modes < 1) return lrbms_fail(ctx, LRBMS_E_INVALID, "local_pod: modes must be >= 1");
  if (!(rtol >= POD_MIN_RTOL))
    return lrbms_fail(ctx, LRBMS_E_INVALID, "local_pod: rtol < 1e-7: the Gram matrix squares the singular values, below 1e-7 relative they are rounding noise");
  if (!(atol >= 0.0)) return lrbms_fail(ctx, LRBMS_E_INVALID, "local_pod: atol must be >= 0");
  if (!work) return lrbms_fail(ctx, LRBMS_E_INVALID, "local_pod: null work (lrbms_local_pod_work_size doubles)");
  if (!U || !V || !nloc || !sv || !added || !info) return lrbms_fail(ctx, LRBMS_E_INVALID, "local_pod: null pointer");

  int K = modes < L ? modes : L;
  K = K < Nw ? K : Nw;
  const long Kc = L < Nw ? L : Nw, Lp = L + (L & 1);
  double* R = work;
  double* PR = R + (long)S * n * L;
  double* Wb = PR + (long)S * n * L;
  double* C = Wb + (long)S * n * Kc;
  double* G = C + (long)S * Nw * L;
  double* Zs = G + (long)S * L * L;
  double* Zw = Zs + (long)S * L * L;
  double* lam = Zw + (long)S * Lp * Lp;
  double* T = lam + (long)S * L;
  double* norm0 = T + (long)S * L * Kc;
  int32_t* ks = (int32_t*)(norm0 + S);                 // 3 doubles = 6 int32 per subdomain: ks, ia, ib
  int32_t* ia = ks + S;
  int32_t* ib = ia + S;
  double* part = norm0 + 4L * S;
  int rc;

  // 1: norm0
  if ((rc = P.apply(P.self, L, U, PR, st)) != LRBMS_OK) return rc;
  hipLaunchKernelGGL(k_pod_norm0, dim3(S), dim3(256), 0, st, n, L, U, (const double*)PR, norm0);
  LRBMS_LAUNCH_CHECK(ctx);
  // 2: R = U, deflated twice
  LRBMS_HIP_CHECK(ctx, hipMemcpyAsync(R, U, sizeof(double) * (size_t)S * n * L, hipMemcpyDeviceToDevice, st));
  for (int pass = 0; pass < 2; ++pass) {
    if ((rc = P.apply(P.self, L, R, PR, st)) != LRBMS_OK) return rc;
    if ((rc = xty(ctx, false, S, n, Nw, L, V, PR, C, part, st)) != LRBMS_OK) return rc;
    if ((rc = xt(ctx, S, n, Nw, L, V, Nw, C, L, R, L, nullptr, nullptr, -1.0, 1, st)) != LRBMS_OK) return rc;
  }
  // 3, 4: Gram matrix and its eigenpairs
  if ((rc = P.apply(P.self, L, R, PR, st)) != LRBMS_OK) return rc;
  if ((rc = xty(ctx, true, S, n, L, L, R, PR, G, part, st)) != LRBMS_OK) return rc;
  if ((rc = launch_pod_eigh(ctx, S, L, 0, G, nullptr, lam, Zs, ia, Zw, st)) != LRBMS_OK) return rc;
  // 5, 6: selection on the device, modes
  hipLaunchKernelGGL(k_pod_select, dim3(S), dim3(128), 0, st, L, Nw, modes, K, rtol, atol, (const double*)lam, (const double*)Zs,
                     (const double*)norm0, (const int32_t*)nloc, sv, ks, added, T);
  LRBMS_LAUNCH_CHECK(ctx);
  if ((rc = xt(ctx, S, n, L, K, R, L, T, K, Wb, K, nullptr, nullptr, 1.0, 0, st)) != LRBMS_OK) return rc;
  return pod_tail(ctx, S, n, Nw, K, P, V, nloc, Wb, PR, C, G, Zs, Zw, lam, ks, ia, ib, part, info, st);
}
