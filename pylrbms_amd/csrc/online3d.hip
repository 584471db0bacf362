// Reduced (online) solvers of the 3D / P2 path: the block-Jacobi PCG of lrbms3_reduced_solve, the batched solve in groups of
// <= 16 parameters with its coarse level and the installable preconditioner, and the reduced side of the parabolic path
// (implicit Euler single and batched, the time residual, the batched parabolic estimate).  Cut out of lrbms3d.hip as text; the
// estimator kernels stay there and are reached through launch_reduced_estimate_batch / launch_estimate_nc_batch, the source terms
// of sources3d.hip through launch_source_terms.
// Home of k3_combine and k3p_axpy, which other files reach through launch_combine and launch_axpy; k3_reduce1 lives in
// lrbms3d.hip with fom_cg (which launches it three times per iteration, red_cg once per residual check) and is reached
// through launch_reduce1.  The dense coarse inverses go through dense_spd_inverse of lrbms3d.hip.
#include "lrbms3d_dev.h"

using namespace lrbms3;

namespace {

// ------------------------------------------------------------------------------------------------- online: reduced solve
__global__ __launch_bounds__(256) void k3_combine(long per_q, int Q, QV th, const double* __restrict__ B, double* __restrict__ Amu) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= per_q) return;
  double acc = 0.0;
  for (int q = 0; q < Q; ++q) acc += th.v[q] * B[q * per_q + i];
  Amu[i] = acc;
}

// inverse of the SPD diagonal blocks by Gauss-Jordan elimination in LDS (no pivoting)
__global__ __launch_bounds__(256) void k3_block_inverse(int N, const double* __restrict__ Amu, double* __restrict__ Dinv) {
  extern __shared__ double lds[];   // [N][2N + 1]
  const int s = blockIdx.x, tid = threadIdx.x, ld = 2 * N + 1;
  const double* A = Amu + ((long)s * 7 + 3) * N * N;
  for (int i = tid; i < N * 2 * N; i += 256) {
    const int r = i / (2 * N), c = i - r * 2 * N;
    // a zero diagonal entry = a zero-padded basis column (ragged local bases: its whole row and column are zero): identity there,
    // the padded unknown stays exactly 0 (2D: k_block_inverse)
    lds[r * ld + c] = c < N ? ((c == r && A[r * N + c] == 0.0) ? 1.0 : A[r * N + c]) : (c - N == r ? 1.0 : 0.0);
  }
  __syncthreads();
  for (int p = 0; p < N; ++p) {
    const double ip = 1.0 / lds[p * ld + p];
    __syncthreads();
    for (int c = tid; c < 2 * N; c += 256) lds[p * ld + c] *= ip;
    __syncthreads();
    for (int i = tid; i < N * 2 * N; i += 256) {
      const int r = i / (2 * N), c = i - r * 2 * N;
      if (r != p && c != p) lds[r * ld + c] -= lds[r * ld + p] * lds[p * ld + c];
    }
    __syncthreads();
    for (int r = tid; r < N; r += 256)
      if (r != p) lds[r * ld + p] = 0.0;
    __syncthreads();
  }
  for (int i = tid; i < N * N; i += 256) Dinv[(long)s * N * N + i] = lds[(i / N) * ld + N + i % N];
}

// scal: [0] rz_old, [1] rz_new, [2] pAp, [3] rr, [4] bb;  partial arrays [S]
// init: x = 0, r = b, z = Dinv r, partial rz, rr
__global__ __launch_bounds__(64) void k3_pcg_init(int N, const double* __restrict__ rhs, const double* __restrict__ Dinv,
                                                  double* __restrict__ x, double* __restrict__ r, double* __restrict__ z,
                                                  double* __restrict__ p, double* __restrict__ prz, double* __restrict__ prr) {
  __shared__ double rs[64], red[64];
  const int s = blockIdx.x, i = threadIdx.x;
  const double ri = i < N ? rhs[(long)s * N + i] : 0.0;
  rs[i] = ri;
  __syncthreads();
  double zi = 0.0;
  if (i < N) {
    const double* D = Dinv + ((long)s * N + i) * N;
    for (int j = 0; j < N; ++j) zi += D[j] * rs[j];
    x[(long)s * N + i] = 0.0;
    r[(long)s * N + i] = ri;
    z[(long)s * N + i] = zi;
    p[(long)s * N + i] = 0.0;
  }
  red[i] = ri * zi;
  __syncthreads();
  for (int w = 32; w > 0; w >>= 1) {
    if (i < w) red[i] += red[i + w];
    __syncthreads();
  }
  if (i == 0) prz[s] = red[0];
  __syncthreads();
  red[i] = ri * ri;
  __syncthreads();
  for (int w = 32; w > 0; w >>= 1) {
    if (i < w) red[i] += red[i + w];
    __syncthreads();
  }
  if (i == 0) prr[s] = red[0];
}

__device__ inline double sum_partials(const double* __restrict__ part, int S, double* red) {   // 64 threads, fixed order
  const int i = threadIdx.x;
  double a[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};      // eight loads in flight per thread
  int k = i;
  for (; k + 7 * 64 < S; k += 8 * 64) {
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = part[k + u * 64];
#pragma unroll
    for (int u = 0; u < 8; ++u) a[u] += v[u];
  }
  for (; k < S; k += 64) a[0] += part[k];
  const double acc = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
  __syncthreads();
  red[i] = acc;
  __syncthreads();
  for (int w = 32; w > 0; w >>= 1) {
    if (i < w) red[i] += red[i + w];
    __syncthreads();
  }
  const double v = red[0];
  __syncthreads();
  return v;
}

// direction + matvec: p_new = z + beta p_old on the neighbourhood (own part stored), Ap = sum_slot A[s][slot] p_new[slot]
__global__ __launch_bounds__(64) void k3_pcg_matvec(T3 t, int N, int first, const double* __restrict__ Amu,
                                                    const double* __restrict__ z, const double* __restrict__ p_old,
                                                    double* __restrict__ p_new, double* __restrict__ Ap,
                                                    const double* __restrict__ prz_new, const double* __restrict__ prz_old,
                                                    double* __restrict__ ppap) {
  extern __shared__ double lds[];   // [7][N] + 64
  double* red = lds + 7 * N;
  const int s = blockIdx.x, i = threadIdx.x, S = t.S;
  double beta = 0.0;
  if (!first) {
    const double a = sum_partials(prz_new, S, red), b = sum_partials(prz_old, S, red);
    beta = a / b;
  }
  for (int k = i; k < 7 * N; k += 64) {
    const int s2 = t.nbr[s * 7 + k / N];
    lds[k] = s2 >= 0 ? z[(long)s2 * N + k % N] + beta * p_old[(long)s2 * N + k % N] : 0.0;
  }
  __syncthreads();
  double acc = 0.0;
  if (i < N) {
    p_new[(long)s * N + i] = lds[3 * N + i];
    for (int slot = 0; slot < 7; ++slot) {
      if (t.nbr[s * 7 + slot] < 0) continue;
      const double* row = Amu + (((long)s * 7 + slot) * N + i) * N;
      const double* ps = lds + slot * N;
      for (int j = 0; j < N; ++j) acc += row[j] * ps[j];
    }
    Ap[(long)s * N + i] = acc;
  }
  __syncthreads();
  red[i] = i < N ? acc * lds[3 * N + i] : 0.0;
  __syncthreads();
  for (int w = 32; w > 0; w >>= 1) {
    if (i < w) red[i] += red[i + w];
    __syncthreads();
  }
  if (i == 0) ppap[s] = red[0];
}

// x += alpha p, r -= alpha Ap, z = Dinv r; partial r.z and r.r
__global__ __launch_bounds__(64) void k3_pcg_update(int S, int N, const double* __restrict__ Dinv, const double* __restrict__ p,
                                                    const double* __restrict__ Ap, double* __restrict__ x, double* __restrict__ r,
                                                    double* __restrict__ z, const double* __restrict__ prz_cur,
                                                    const double* __restrict__ ppap, double* __restrict__ prz_out,
                                                    double* __restrict__ prr) {
  __shared__ double rs[64], red[64];
  const int s = blockIdx.x, i = threadIdx.x;
  const double rz = sum_partials(prz_cur, S, red), pap = sum_partials(ppap, S, red);
  const double alpha = rz / pap;
  double ri = 0.0;
  if (i < N) {
    x[(long)s * N + i] += alpha * p[(long)s * N + i];
    ri = r[(long)s * N + i] - alpha * Ap[(long)s * N + i];
    r[(long)s * N + i] = ri;
  }
  rs[i] = ri;
  __syncthreads();
  double zi = 0.0;
  if (i < N) {
    const double* D = Dinv + ((long)s * N + i) * N;
    for (int j = 0; j < N; ++j) zi += D[j] * rs[j];
    z[(long)s * N + i] = zi;
  }
  red[i] = ri * zi;
  __syncthreads();
  for (int w = 32; w > 0; w >>= 1) {
    if (i < w) red[i] += red[i + w];
    __syncthreads();
  }
  if (i == 0) prz_out[s] = red[0];
  __syncthreads();
  red[i] = ri * ri;
  __syncthreads();
  for (int w = 32; w > 0; w >>= 1) {
    if (i < w) red[i] += red[i + w];
    __syncthreads();
  }
  if (i == 0) prr[s] = red[0];
}

// ------------------------------------------------------------------------------------------------- online: batched reduced solve
// nmu <= 16 parameters at once: every projected block is read once per iteration for the whole batch, one block-Jacobi
// preconditioner at the batch-mean theta (any SPD preconditioner is admissible), independent CG scalars per parameter.
// Vectors [S][N][nmu] (parameter fastest).  Threads (i = row, m = parameter).

// scal [5][16]: rz_old, rz_new, pAp, rr, bb per parameter;  partial arrays [S][16]
__global__ __launch_bounds__(256) void k3b_reduce(int S, int nmu, const double* __restrict__ part, double* __restrict__ out) {
  __shared__ double red[256];
  const int tid = threadIdx.x, m = tid & 15, g = tid >> 4;
  double acc = 0.0;
  if (m < nmu)
    for (int k = g; k < S; k += 16) acc += part[(long)k * 16 + m];
  red[tid] = acc;
  __syncthreads();
  for (int w = 128; w >= 16; w >>= 1) {
    if (tid < w) red[tid] += red[tid + w];
    __syncthreads();
  }
  if (tid < 16) out[tid] = red[tid];
}

//   x: this group's columns of the caller's solution array, x[(s N + i) ldx + m]
__global__ __launch_bounds__(512) void k3b_init(int N, int nmu, int ldx, const double* __restrict__ rhs, const double* __restrict__ Dinv,
                                                double* __restrict__ x, double* __restrict__ r, double* __restrict__ z,
                                                double* __restrict__ p, double* __restrict__ prz, double* __restrict__ prr) {
  extern __shared__ double lds[];      // [N] rhs + [N][16] products
  const int s = blockIdx.x, tid = threadIdx.x, i = tid >> 4, m = tid & 15;
  for (int k = tid; k < N; k += 512) lds[k] = rhs[(long)s * N + k];
  __syncthreads();
  double ri = 0.0, zi = 0.0;
  const bool on = i < N && m < nmu;
  if (on) {
    ri = lds[i];
    const double* D = Dinv + ((long)s * N + i) * N;
    for (int j = 0; j < N; ++j) zi += D[j] * lds[j];
    const long d = ((long)s * N + i) * nmu + m;
    x[((long)s * N + i) * ldx + m] = 0.0;
    r[d] = ri; z[d] = zi; p[d] = 0.0;
  }
  double* pr = lds + N;
  for (int pass = 0; pass < 2; ++pass) {
    __syncthreads();
    if (i < 32) pr[i * 16 + m] = on ? (pass ? ri * ri : ri * zi) : 0.0;
    __syncthreads();
    if (tid < 16) {
      double a = 0.0;
      for (int k = 0; k < N; ++k) a += pr[k * 16 + tid];
      (pass ? prr : prz)[(long)s * 16 + tid] = a;
    }
  }
}

// k3b_init with a right-hand side of its own per column (lrbms3_reduced_solve_batch_src): column m starts from
// sum_j phi[m][j] rhs_K[j][s], spelled out with fma from the first product; phi = this group's rows [nmu][K] of the device table,
// rhs_K [K][S][N] (SN = S N).  K = 1 with phi = 1 gives the bits of k3b_init: 1 * x is exact and the rest is its arithmetic.
__global__ __launch_bounds__(512) void k3b_init_src(int N, int nmu, int ldx, int K, long SN, const double* __restrict__ phi,
                                                    const double* __restrict__ rhs_K, const double* __restrict__ Dinv,
                                                    double* __restrict__ x, double* __restrict__ r, double* __restrict__ z,
                                                    double* __restrict__ p, double* __restrict__ prz, double* __restrict__ prr) {
  extern __shared__ double lds[];      // [N][16] rhs per column + [32][16] products
  const int s = blockIdx.x, tid = threadIdx.x, i = tid >> 4, m = tid & 15;
  for (int k = tid; k < N * 16; k += 512) {
    const int kk = k >> 4, mm = k & 15;
    double acc = 0.0;
    if (mm < nmu) {
      const double* ph = phi + (long)mm * K;
      const double* src = rhs_K + (long)s * N + kk;
      acc = ph[0] * src[0];
      for (int j = 1; j < K; ++j) acc = __fma_rn(ph[j], src[(long)j * SN], acc);
    }
    lds[k] = acc;
  }
  __syncthreads();
  double ri = 0.0, zi = 0.0;
  const bool on = i < N && m < nmu;
  if (on) {
    ri = lds[i * 16 + m];
    const double* D = Dinv + ((long)s * N + i) * N;
    for (int j = 0; j < N; ++j) zi += D[j] * lds[j * 16 + m];
    const long d = ((long)s * N + i) * nmu + m;
    x[((long)s * N + i) * ldx + m] = 0.0;
    r[d] = ri; z[d] = zi; p[d] = 0.0;
  }
  double* pr = lds + N * 16;
  for (int pass = 0; pass < 2; ++pass) {
    __syncthreads();
    if (i < 32) pr[i * 16 + m] = on ? (pass ? ri * ri : ri * zi) : 0.0;
    __syncthreads();
    if (tid < 16) {
      double a = 0.0;
      for (int k = 0; k < N; ++k) a += pr[k * 16 + tid];
      (pass ? prr : prz)[(long)s * 16 + tid] = a;
    }
  }
}

// dst [rows][nm] = this group's columns src[row ldx + m] of a panel with leading dimension ldx
__global__ __launch_bounds__(256) void k3b_gather(long rows, int nm, int ldx, const double* __restrict__ src, double* __restrict__ dst) {
  const long total = rows * nm;
  for (long k = (long)blockIdx.x * 256 + threadIdx.x; k < total; k += (long)gridDim.x * 256) dst[k] = src[(k / nm) * ldx + k % nm];
}

// Step start of the batched reduced implicit Euler (lrbms3_reduced_implicit_euler_batch(_src)) for one group: given
// y = (M + dt A_m) u_k from the MASS matvec, f_m = M_red u_k + dt b_m in the operation order of k3p_red_rhs(_src) -- the mass row
// sum first, then + dt * b, b_m = rhs_K[s][i] (K == 0) or sum_j phi[m][j] rhs_K[j][s][i] spelled out with fma from the first
// product (phi: this group's rows of step k + 1, row stride ldphi) -- and the CG start of k3b_init from x = u_k: r = f - y,
// z = Dinv r, p = 0, x written into the group's columns of U[k+1]; partials of r.z, r.r and |f_m|^2.
__global__ __launch_bounds__(512) void k3b_step_init(int N, int nmu, int ldx, double dt, const double* __restrict__ Mred,
                                                     const double* __restrict__ uk, int K, long SN, long ldphi,
                                                     const double* __restrict__ phi, const double* __restrict__ rhs_K,
                                                     const double* __restrict__ y, const double* __restrict__ Dinv,
                                                     double* __restrict__ x, double* __restrict__ r, double* __restrict__ z,
                                                     double* __restrict__ p, double* __restrict__ prz, double* __restrict__ prr,
                                                     double* __restrict__ pff) {
  extern __shared__ double lds[];      // [N][16] u_k + [N][16] residual + [32][16] products
  const int s = blockIdx.x, tid = threadIdx.x, i = tid >> 4, m = tid & 15;
  double* us = lds;
  double* rs = lds + N * 16;
  for (int k = tid; k < N * 16; k += 512) {
    const int kk = k >> 4, mm = k & 15;
    us[k] = mm < nmu ? uk[((long)s * N + kk) * ldx + mm] : 0.0;
  }
  __syncthreads();
  double fi = 0.0, ri = 0.0, zi = 0.0;
  const bool on = i < N && m < nmu;
  const long d = ((long)s * N + i) * nmu + m;
  if (on) {
    const double* M = Mred + ((long)s * N + i) * N;
    double acc = 0.0;
    for (int j = 0; j < N; ++j) acc += M[j] * us[j * 16 + m];
    const double* src = rhs_K + (long)s * N + i;
    double bs = src[0];
    if (K > 0) {
      const double* ph = phi + (long)m * ldphi;
      bs = ph[0] * src[0];
      for (int j = 1; j < K; ++j) bs = __fma_rn(ph[j], src[(long)j * SN], bs);
    }
    fi = acc + dt * bs;
    ri = fi - y[d];
  }
  if (i < N) rs[i * 16 + m] = ri;
  __syncthreads();
  if (on) {
    const double* D = Dinv + ((long)s * N + i) * N;
    for (int j = 0; j < N; ++j) zi += D[j] * rs[j * 16 + m];
    x[((long)s * N + i) * ldx + m] = us[i * 16 + m];
    r[d] = ri; z[d] = zi; p[d] = 0.0;
  }
  double* pr = lds + 2 * N * 16;
  for (int pass = 0; pass < 3; ++pass) {
    __syncthreads();
    if (i < 32) pr[i * 16 + m] = on ? (pass == 0 ? ri * zi : pass == 1 ? ri * ri : fi * fi) : 0.0;
    __syncthreads();
    if (tid < 16) {
      double a = 0.0;
      for (int k = 0; k < N; ++k) a += pr[k * 16 + tid];
      (pass == 0 ? prz : pass == 1 ? prr : pff)[(long)s * 16 + tid] = a;
    }
  }
}

// Coarse level of the batched reduced solve (nullptr members: block-Jacobi alone): y0 [S][16] = A0^-1 r0 of the last residual,
// prc_* [S][16] its contributions r0 . y0 to r.z -- summed with the fine partials wherever r.z is needed.
struct CoarseB {
  const double* y0;
  const double* prc_new;
  const double* prc_old;
};

// The CG scalars of an iteration are sums over the workgroups' partials [S][16] of the previous kernel; every workgroup (512
// threads) forms them itself, in the same fixed order, so an iteration is two launches (no reduction kernels in between).
// Returns the sum for parameter tid & 15 in every thread; buf [32][16] doubles of LDS.
__device__ inline double sum_partials16(const double* __restrict__ part, int S, double* buf, int tid) {
  const int m = tid & 15, g = tid >> 4, ng = blockDim.x >> 4;     // 16 or 32 groups (256 / 512 threads)
  double a[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};      // eight loads in flight (a plain loop waits one L2 round trip per entry)
  int k = g;
  for (; k + 7 * ng < S; k += 8 * ng) {
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = part[(long)(k + u * ng) * 16 + m];
#pragma unroll
    for (int u = 0; u < 8; ++u) a[u] += v[u];
  }
  for (; k < S; k += ng) a[0] += part[(long)k * 16 + m];
  const double acc = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
  __syncthreads();
  buf[g * 16 + m] = acc;
  __syncthreads();
  double v = 0.0;
  for (int k = 0; k < ng; ++k) v += buf[k * 16 + m];
  __syncthreads();
  return v;
}

// The same direction + matvec on the matrix cores (N <= 32): Ap [rows i][16 parameters] = sum_q sum_slot B_q[slot] (theta_q . p[slot])
// -- the A operand is a 16-row strip of a projected block straight from global memory (lane: row l & 15, columns 2 (l >> 4) and
// + 1 of the wave's 8-column band: one 16-byte load for two k-steps), the B operand the direction of the slot from the LDS with the
// parameter weight theta_qm folded in (a lane owns ONE parameter, l & 15).  Four waves, wave w owns the column band [8 w, 8 w + 8) of
// every block, so the A_mu strips are read exactly once; the waves' tiles meet in the LDS in a fixed order.
// MASS (lrbms3_reduced_implicit_euler_batch): the step operator M_red + dt A_m -- M_red [S][N][N] is one more A-operand block on
// the self slot with coefficient 1, dt is folded into th by the host; no augmented copy of B is written anywhere.
template <bool MASS> struct MassOp3 {};
template <> struct MassOp3<true> { const double* M; };
template <int RT, bool MASS = false>
__global__ __launch_bounds__(256) void k3b_matvec_mfma(T3 t, int Q, int N, int nmu, int first, TB th, const double* __restrict__ B,
                                                       const double* __restrict__ z, const double* __restrict__ p_old,
                                                       double* __restrict__ p_new, double* __restrict__ Ap,
                                                       const double* __restrict__ prz_new, const double* __restrict__ prz_old,
                                                       double* __restrict__ ppap, CoarseB cl, MassOp3<MASS> mass = MassOp3<MASS>()) {
  extern __shared__ double lds[];      // [7][32][16] direction (rows >= N zero) + [4][RT][256] partial tiles + [32][16] sums
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, li = lane & 15, lk = lane >> 4, S = t.S;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  double* dir = lds;
  double* part = lds + 7 * 32 * 16;
  double* buf = part + 4 * RT * 256;
  double bm = 0.0;
  if (!first) {
    double rz_new = sum_partials16(prz_new, S, buf, tid), rz_old = sum_partials16(prz_old, S, buf, tid);
    if (cl.y0) {
      rz_new += sum_partials16(cl.prc_new, S, buf, tid);
      rz_old += sum_partials16(cl.prc_old, S, buf, tid);
    }
    bm = rz_old == 0.0 ? 0.0 : rz_new / rz_old;
  }
  for (int k = tid; k < 7 * 32 * 16; k += 256) {
    const int slot = k >> 9, j = (k >> 4) & 31, mm = k & 15;
    const int s2 = t.nbr[s * 7 + slot];
    double v = 0.0;
    if (s2 >= 0 && mm < nmu && j < N) {
      const long d = ((long)s2 * N + j) * nmu + mm;
      double zt = z[d];
      if (cl.y0 && j == 0) zt += cl.y0[s2 * 16 + mm];              // z = Dinv r + e_0 y0: the coarse correction
      v = first ? zt : zt + bm * p_old[d];
    }
    dir[k] = v;
  }
  __syncthreads();
  for (int k = tid; k < N * 16; k += 256) {
    const int i = k >> 4, mm = k & 15;
    if (mm < nmu) p_new[((long)s * N + i) * nmu + mm] = dir[(3 * 32 + i) * 16 + mm];
  }
  d4 acc[RT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) acc[rt] = (d4){0.0, 0.0, 0.0, 0.0};
  const int c0 = 8 * wave + 2 * lk;                  // this lane's two columns of the band (clamped into the matrix: the matching
  const bool even = (N & 1) == 0;                    // direction rows are zero beyond N)
  const int ca = c0 < N ? c0 : N - 1, cb = c0 + 1 < N ? c0 + 1 : N - 1, cpair = c0 + 1 < N ? c0 : N - 2;
  if (8 * wave < N) {
    double thq[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) thq[q] = q < Q ? th.v[li][q] : 0.0;
    for (int slot = 0; slot < 7; ++slot) {
      if (t.nbr[s * 7 + slot] < 0) continue;         // wave-uniform
      const double p0 = dir[(slot * 32 + c0) * 16 + li], p1 = dir[(slot * 32 + c0 + 1) * 16 + li];
      for (int q = 0; q < Q; ++q) {
        const double b0 = thq[q] * p0, b1 = thq[q] * p1;
        const double* blk = B + (((long)q * S + s) * 7 + slot) * N * N;
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
          const int row = rt * 16 + li < N ? rt * 16 + li : N - 1;
          double a0, a1;
          if (even) {
            const double2 v = *reinterpret_cast<const double2*>(blk + row * N + cpair);
            a0 = v.x; a1 = v.y;
          } else {
            a0 = blk[row * N + ca]; a1 = blk[row * N + cb];
          }
          acc[rt] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[rt], 0, 0, 0);
          acc[rt] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[rt], 0, 0, 0);
        }
      }
    }
    if constexpr (MASS) {                            // + M_red[s] p_self: the same strip loads and MFMA chain, coefficient 1
      const double b0 = dir[(3 * 32 + c0) * 16 + li], b1 = dir[(3 * 32 + c0 + 1) * 16 + li];
      const double* blk = mass.M + (long)s * N * N;
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
        const int row = rt * 16 + li < N ? rt * 16 + li : N - 1;
        double a0, a1;
        if (even) {
          const double2 v = *reinterpret_cast<const double2*>(blk + row * N + cpair);
          a0 = v.x; a1 = v.y;
        } else {
          a0 = blk[row * N + ca]; a1 = blk[row * N + cb];
        }
        acc[rt] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[rt], 0, 0, 0);
        acc[rt] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[rt], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int r = 0; r < 4; ++r) part[((wave * RT + rt) * 4 + r) * 64 + lane] = acc[rt][r];
  __syncthreads();
  double pp = 0.0;
  if (wave < RT) {                                   // wave rt finishes tile rt: rows rt * 16 + lk + 4 r, parameter li
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      double v = 0.0;
      for (int w = 0; w < 4; ++w) v += part[((w * RT + wave) * 4 + r) * 64 + lane];
      const int row = wave * 16 + lk + 4 * r;
      if (row < N && li < nmu) {
        Ap[((long)s * N + row) * nmu + li] = v;
        pp += v * dir[(3 * 32 + row) * 16 + li];
      }
    }
    pp += __shfl_xor(pp, 16);
    pp += __shfl_xor(pp, 32);
    if (lk == 0) buf[wave * 16 + li] = pp;
  }
  __syncthreads();
  if (tid < 16) {
    double a = 0.0;
    for (int rt = 0; rt < RT; ++rt) a += buf[rt * 16 + tid];
    ppap[(long)s * 16 + tid] = a;
  }
}

// direction + matvec: p_new = z + beta_m p_old on the neighbourhood (own part stored), Ap = sum_q theta_qm sum_slot B_q p_new;
// beta_m = r.z (prz_new) / previous r.z (prz_old)
template <bool MASS = false>
__global__ __launch_bounds__(512) void k3b_matvec(T3 t, int Q, int N, int nmu, int first, TB th, const double* __restrict__ B,
                                                  const double* __restrict__ z, const double* __restrict__ p_old,
                                                  double* __restrict__ p_new, double* __restrict__ Ap, const double* __restrict__ prz_new,
                                                  const double* __restrict__ prz_old, double* __restrict__ ppap, CoarseB cl,
                                                  MassOp3<MASS> mass = MassOp3<MASS>()) {
  extern __shared__ double lds[];      // [7][N][16] direction + [32][16] products
  const int s = blockIdx.x, tid = threadIdx.x, i = tid >> 4, m = tid & 15, S = t.S;
  double bm = 0.0;                     // (512 % 16 == 0: a thread fills entries of its own parameter only)
  if (!first) {
    double* buf = lds + 7 * N * 16;
    double rz_new = sum_partials16(prz_new, S, buf, tid), rz_old = sum_partials16(prz_old, S, buf, tid);
    if (cl.y0) {
      rz_new += sum_partials16(cl.prc_new, S, buf, tid);
      rz_old += sum_partials16(cl.prc_old, S, buf, tid);
    }
    bm = rz_old == 0.0 ? 0.0 : rz_new / rz_old;                    // a converged parameter (r = 0) stays put
  }
  for (int k = tid; k < 7 * N * 16; k += 512) {
    const int slot = k / (N * 16), j = (k >> 4) % N, mm = k & 15;
    const int s2 = t.nbr[s * 7 + slot];
    double v = 0.0;
    if (s2 >= 0 && mm < nmu) {
      const long d = ((long)s2 * N + j) * nmu + mm;
      double zt = z[d];
      if (cl.y0 && j == 0) zt += cl.y0[s2 * 16 + mm];
      v = first ? zt : zt + bm * p_old[d];
    }
    lds[k] = v;
  }
  __syncthreads();
  double acc = 0.0;
  const bool on = i < N && m < nmu;
  if (on) {
    p_new[((long)s * N + i) * nmu + m] = lds[(3 * N + i) * 16 + m];
    for (int q = 0; q < Q; ++q) {
      double aq = 0.0;
      for (int slot = 0; slot < 7; ++slot) {
        if (t.nbr[s * 7 + slot] < 0) continue;
        const double* row = B + ((((long)q * S + s) * 7 + slot) * N + i) * N;
        const double* ps = lds + slot * N * 16 + m;
        for (int j = 0; j < N; ++j) aq += row[j] * ps[j * 16];
      }
      acc += th.v[m][q] * aq;
    }
    if constexpr (MASS) {
      const double* row = mass.M + ((long)s * N + i) * N;
      const double* ps = lds + 3 * N * 16 + m;
      double am = 0.0;
      for (int j = 0; j < N; ++j) am += row[j] * ps[j * 16];
      acc += am;
    }
    Ap[((long)s * N + i) * nmu + m] = acc;
  }
  double* pr = lds + 7 * N * 16;
  __syncthreads();
  if (i < 32) pr[i * 16 + m] = on ? acc * lds[(3 * N + i) * 16 + m] : 0.0;
  __syncthreads();
  if (tid < 16) {
    double a = 0.0;
    for (int k = 0; k < N && k < 32; ++k) a += pr[k * 16 + tid];
    ppap[(long)s * 16 + tid] = a;
  }
}

__global__ __launch_bounds__(512) void k3b_update(int N, int nmu, int ldx, const double* __restrict__ Dinv, const double* __restrict__ p,
                                                  const double* __restrict__ Ap, double* __restrict__ x, double* __restrict__ r,
                                                  double* __restrict__ z, int S, const double* __restrict__ prz_cur,
                                                  const double* __restrict__ prc_cur, const double* __restrict__ ppap,
                                                  double* __restrict__ prz, double* __restrict__ prr) {
  extern __shared__ double lds[];      // [N][16] residual + [32][16] products
  const int s = blockIdx.x, tid = threadIdx.x, i = tid >> 4, m = tid & 15;
  const bool on = i < N && m < nmu;
  double ri = 0.0, zi = 0.0;
  double rz = sum_partials16(prz_cur, S, lds + N * 16, tid);
  if (prc_cur) rz += sum_partials16(prc_cur, S, lds + N * 16, tid);
  const double pap = sum_partials16(ppap, S, lds + N * 16, tid);
  if (on) {
    const double alpha = pap != 0.0 ? rz / pap : 0.0;               // a converged parameter (r = 0) stays put
    const long d = ((long)s * N + i) * nmu + m;
    x[((long)s * N + i) * ldx + m] += alpha * p[d];
    ri = r[d] - alpha * Ap[d];
    r[d] = ri;
  }
  if (i < N) lds[i * 16 + m] = ri;
  __syncthreads();
  if (on) {
    const double* D = Dinv + ((long)s * N + i) * N;
    for (int j = 0; j < N; ++j) zi += D[j] * lds[j * 16 + m];
    z[((long)s * N + i) * nmu + m] = zi;
  }
  double* pr = lds + N * 16;
  for (int pass = 0; pass < 2; ++pass) {
    __syncthreads();
    if (i < 32) pr[i * 16 + m] = on ? (pass ? ri * ri : ri * zi) : 0.0;
    __syncthreads();
    if (tid < 16) {
      double a = 0.0;
      for (int k = 0; k < N && k < 32; ++k) a += pr[k * 16 + tid];
      (pass ? prr : prz)[(long)s * 16 + tid] = a;
    }
  }
}

// ---- coarse level of the reduced solvers: the Galerkin problem on the FIRST local basis vector of every subdomain (the constant the
// reductor starts every basis with), A0[s][t] = A_mu[s][slot of t][0][0] -- a 7-point S x S matrix, inverted densely once per
// reduced model at a reference parameter (lrbms3_reduced_precond_build; any SPD preconditioner is admissible for the other mu).
__global__ __launch_bounds__(256) void k3r_coarse_fill(T3 t, int Q, int N, QV th, const double* __restrict__ B, double* __restrict__ A0,
                                                       double* __restrict__ Id) {
  const int idx = blockIdx.x * 256 + threadIdx.x, S = t.S;
  if (idx >= S * 7) return;
  const int s = idx / 7, slot = idx - s * 7;
  if (slot == 3) Id[(long)s * S + s] = 1.0;
  const int tt = slot == 3 ? s : t.nbr[s * 7 + slot];
  if (tt < 0) return;
  double v = 0.0;
  for (int q = 0; q < Q; ++q) v += th.v[q] * B[(((long)q * S + s) * 7 + slot) * N * N];
  A0[(long)s * S + tt] = v;
}

// y0 [S][16] = A0inv r0, r0[t][m] = r[t][0][m], on the matrix cores: one 16-row tile of A0inv per workgroup, sixteen waves split
// K = S and keep eight k-steps of operands in flight (a load -> MFMA chain per k-step is one L2 round trip each: 25 us);
// prc [S][16] = r0 . y0 (the coarse part of r.z)
__global__ __launch_bounds__(1024) void k3b_coarse_apply(int S, int N, int nmu, const double* __restrict__ A0inv, const double* __restrict__ r,
                                                         double* __restrict__ y0, double* __restrict__ prc) {
  __shared__ double part[16][4][64];
  const int tid = threadIdx.x, lane = tid & 63, li = lane & 15, lk = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int row0 = blockIdx.x * 16, row = row0 + li < S ? row0 + li : S - 1;
  const double* arow = A0inv + (long)row * S;
  d4 acc = (d4){0.0, 0.0, 0.0, 0.0};
  const int ksteps = (S + 3) / 4;
  for (int k0 = wave; k0 < ksteps; k0 += 16 * 8) {
    double a[8], b[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int c = 4 * (k0 + 16 * u) + lk, cc = c < S ? c : S - 1;
      a[u] = arow[cc];
      b[u] = r[((long)cc * N) * nmu + (li < nmu ? li : 0)];
      if (c >= S || li >= nmu) b[u] = 0.0;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], b[u], acc, 0, 0, 0);
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) part[wave][q][lane] = acc[q];
  __syncthreads();
  if (wave < 4) {                                     // wave q finishes accumulator register q: rows lk + 4 q, column li
    double v = 0.0;
    for (int w = 0; w < 16; ++w) v += part[w][wave][lane];
    const int rr = row0 + lk + 4 * wave;
    if (rr < S) {
      const double r0 = li < nmu ? r[((long)rr * N) * nmu + li] : 0.0;
      y0[rr * 16 + li] = li < nmu ? v : 0.0;
      prc[rr * 16 + li] = li < nmu ? v * r0 : 0.0;
    }
  }
}

// ------------------------------------------------------------------------------------------------- parabolic path: reduced side
// (the description of the path and its full-order side: lrbms3d.hip)
__global__ __launch_bounds__(256) void k3p_axpy(long total, const double* __restrict__ x, double* __restrict__ y) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < total) y[i] += x[i];
}

// Amu [S][7][N][N] slot 3 (self) += M_red [S][N][N]
__global__ __launch_bounds__(256) void k3p_red_add_mass(long total, int N, const double* __restrict__ Mred, double* __restrict__ Amu) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const long NN = (long)N * N, s = i / NN;
  Amu[(s * 7 + 3) * NN + (i - s * NN)] += Mred[i];
}

// reduced step right-hand side: f = M_red u_k + dt rhs_red, rhs = f - Ku; partial |f|^2 per subdomain
__global__ __launch_bounds__(64) void k3p_red_rhs(int N, double dt, const double* __restrict__ Mred, const double* __restrict__ u,
                                                  const double* __restrict__ rhs_red, const double* __restrict__ Ku,
                                                  double* __restrict__ rhs, double* __restrict__ part) {
  __shared__ double us[64], red[64];
  const int s = blockIdx.x, i = threadIdx.x;
  us[i] = i < N ? u[(long)s * N + i] : 0.0;
  __syncthreads();
  double f = 0.0;
  if (i < N) {
    const double* M = Mred + ((long)s * N + i) * N;
    double acc = 0.0;
    for (int j = 0; j < N; ++j) acc += M[j] * us[j];
    f = acc + dt * rhs_red[(long)s * N + i];
    rhs[(long)s * N + i] = f - Ku[(long)s * N + i];
  }
  red[i] = f * f;
  __syncthreads();
  for (int w = 32; w > 0; w >>= 1) {
    if (i < w) red[i] += red[i + w];
    __syncthreads();
  }
  if (i == 0) part[s] = red[0];
}

// k3p_red_rhs with the load sum_j phi[j] rhs_red_K[j] (rhs_red_K [K][S][N], SN = S N).  K = 1, phi = 1: the bits of k3p_red_rhs.
__global__ __launch_bounds__(64) void k3p_red_rhs_src(int N, double dt, const double* __restrict__ Mred, const double* __restrict__ u,
                                                      int K, long SN, const double* __restrict__ phi,
                                                      const double* __restrict__ rhs_red_K, const double* __restrict__ Ku,
                                                      double* __restrict__ rhs, double* __restrict__ part) {
  __shared__ double us[64], red[64];
  const int s = blockIdx.x, i = threadIdx.x;
  us[i] = i < N ? u[(long)s * N + i] : 0.0;
  __syncthreads();
  double f = 0.0;
  if (i < N) {
    const double* M = Mred + ((long)s * N + i) * N;
    double acc = 0.0;
    for (int j = 0; j < N; ++j) acc += M[j] * us[j];
    double bs = phi[0] * rhs_red_K[(long)s * N + i];
    for (int j = 1; j < K; ++j) bs = __fma_rn(phi[j], rhs_red_K[(long)j * SN + (long)s * N + i], bs);
    f = acc + dt * bs;
    rhs[(long)s * N + i] = f - Ku[(long)s * N + i];
  }
  red[i] = f * f;
  __syncthreads();
  for (int w = 32; w > 0; w >>= 1) {
    if (i < w) red[i] += red[i + w];
    __syncthreads();
  }
  if (i == 0) part[s] = red[0];
}

// out [L][S] = y^T Minv_s y, y = (Amu dU_l)_s on the 7-slot operator; one workgroup per (subdomain, vector)
__global__ __launch_bounds__(64) void k3p_time_residual(T3 t, int N, const double* __restrict__ Amu, const double* __restrict__ Minv,
                                                        const double* __restrict__ dU, double* __restrict__ out) {
  extern __shared__ double lds[];   // [7][N] | y [N] | 64
  double* ys = lds + 7 * N;
  double* red = ys + N;
  const int s = blockIdx.x, l = blockIdx.y, i = threadIdx.x, S = t.S;
  const double* x = dU + (long)l * S * N;
  for (int k = i; k < 7 * N; k += 64) {
    const int s2 = t.nbr[s * 7 + k / N];
    lds[k] = s2 >= 0 ? x[(long)s2 * N + k % N] : 0.0;
  }
  __syncthreads();
  double y = 0.0;
  if (i < N) {
    for (int slot = 0; slot < 7; ++slot) {
      if (t.nbr[s * 7 + slot] < 0) continue;
      const double* row = Amu + (((long)s * 7 + slot) * N + i) * N;
      const double* ps = lds + slot * N;
      for (int j = 0; j < N; ++j) y += row[j] * ps[j];
    }
    ys[i] = y;
  }
  __syncthreads();
  double w = 0.0;
  if (i < N) {
    const double* D = Minv + ((long)s * N + i) * N;
    for (int j = 0; j < N; ++j) w += D[j] * ys[j];
  }
  red[i] = i < N ? y * w : 0.0;
  __syncthreads();
  for (int k = 32; k > 0; k >>= 1) {
    if (i < k) red[i] += red[i + k];
    __syncthreads();
  }
  if (i == 0) out[(long)l * S + s] = red[0];
}

}  // namespace

namespace lrbms3 {

// the kernels of this file that other files launch: grid and block as at the launches below
void launch_combine(hipStream_t st, long per_q, int Q, const QV& th, const double* B, double* Amu) {
  hipLaunchKernelGGL(k3_combine, dim3((unsigned)((per_q + 255) / 256)), dim3(256), 0, st, per_q, Q, th, B, Amu);
}
void launch_axpy(hipStream_t st, long total, const double* x, double* y) {
  hipLaunchKernelGGL(k3p_axpy, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, total, x, y);
}

}  // namespace lrbms3

extern "C" {

int64_t lrbms3_reduced_solve_work_size(lrbms3_ctx* ctx, int32_t N) {
  if (!ctx || !ctx->has_mesh) return -1;
  const int64_t S = ctx->t.S;
  return S * 7 * N * N + S * N * N + 6 * S * N + 5 * S + 16;
}

}  // extern "C"

namespace {

// work layout of the single-parameter reduced PCG (lrbms3_reduced_solve_work_size doubles)
struct RedWork {
  double *Amu, *Dinv, *r, *z, *p0, *p1, *Ap, *prz0, *prz1, *ppap, *prr, *scal;
};

RedWork red_work(long S, int N, double* work) {
  RedWork w;
  w.Amu = work;
  w.Dinv = w.Amu + S * 7 * N * N;
  w.r = w.Dinv + S * N * N;
  w.z = w.r + S * N;
  w.p0 = w.z + S * N;
  w.p1 = w.p0 + S * N;
  w.Ap = w.p1 + S * N;
  w.prz0 = w.Ap + S * N;     // partial sums, ping-pong
  w.prz1 = w.prz0 + S;
  w.ppap = w.prz1 + S;
  w.prr = w.ppap + S;
  w.scal = w.prr + S;        // [0] rr, [1] bb
  return w;
}

// Block-Jacobi PCG on the 7-slot operator w.Amu (inverse diagonal blocks in w.Dinv) from u = 0; the relative residual is taken
// against |rhs|, or against the device scalar bref (squared norm) when it is given and non-zero (warm starts, as fom_cg).
int red_cg(lrbms3_ctx* ctx, hipStream_t st, int N, RedWork& w, const double* rhs, double* u, double rtol, int max_iter, double* info,
           const double* bref, const char* name) {
  const T3& t = ctx->t;
  const long S = t.S;
  hipLaunchKernelGGL(k3_pcg_init, dim3(S), dim3(64), 0, st, N, rhs, w.Dinv, u, w.r, w.z, w.p0, w.prz0, w.prr);
  launch_reduce1(st, (int)S, w.prr, w.scal + 1);
  LRBMS_LAUNCH_CHECK(ctx);
  double bb = 0.0, bn = 0.0;
  LRBMS_HIP_CHECK(ctx, hipMemcpyAsync(&bb, w.scal + 1, sizeof(double), hipMemcpyDeviceToHost, st));
  if (bref) LRBMS_HIP_CHECK(ctx, hipMemcpyAsync(&bn, bref, sizeof(double), hipMemcpyDeviceToHost, st));
  LRBMS_HIP_CHECK(ctx, hipStreamSynchronize(st));
  if (info) info[0] = 0, info[1] = 0;
  if (bb == 0.0) return LRBMS_OK;
  const double den = bn > 0.0 ? bn : bb;
  const size_t lds = sizeof(double) * (7 * N + 64);
  double *po = w.p0, *pn = w.p1, *rz_old = w.prz1, *rz_cur = w.prz0;
  int it = 0;
  double rel = 1.0;
  const int check = 8;
  while (it < max_iter) {
    for (int k = 0; k < check && it < max_iter; ++k, ++it) {
      hipLaunchKernelGGL(k3_pcg_matvec, dim3(S), dim3(64), lds, st, t, N, it == 0 ? 1 : 0, w.Amu, w.z, po, pn, w.Ap, rz_cur, rz_old, w.ppap);
      hipLaunchKernelGGL(k3_pcg_update, dim3(S), dim3(64), 0, st, (int)S, N, w.Dinv, pn, w.Ap, u, w.r, w.z, rz_cur, w.ppap, rz_old, w.prr);
      std::swap(po, pn);
      std::swap(rz_old, rz_cur);
    }
    launch_reduce1(st, (int)S, w.prr, w.scal);
    LRBMS_LAUNCH_CHECK(ctx);
    double rr = 0.0;
    LRBMS_HIP_CHECK(ctx, hipMemcpyAsync(&rr, w.scal, sizeof(double), hipMemcpyDeviceToHost, st));
    LRBMS_HIP_CHECK(ctx, hipStreamSynchronize(st));
    rel = sqrt(rr / den);
    if (!(rel == rel)) return lrbms_fail(ctx, LRBMS_E_NOT_CONVERGED, std::string(name) + ": NaN residual");
    if (rel <= rtol) break;
  }
  if (info) info[0] = it, info[1] = rel;
  if (rel > rtol) return lrbms_fail(ctx, LRBMS_E_NOT_CONVERGED, std::string(name) + ": not converged");
  return LRBMS_OK;
}

}  // namespace

extern "C" {

int lrbms3_reduced_solve(lrbms3_ctx* ctx, int32_t Q, int32_t N, const double* theta, const double* B_sys, const double* rhs_red,
                         double* work, double* u, double rtol, int32_t max_iter, double* info, void* stream) {
  LRBMS_REQUIRE_MESH(ctx);
  const T3& t = ctx->t;
  if (t.S_ext != t.S) return lrbms_fail(ctx, LRBMS_E_INVALID, "reduced_solve: needs all subdomains on this rank");
  if (Q < 1 || Q > 8 || N < 1 || N > 64 || !theta || !B_sys || !rhs_red || !work || !u)
    return lrbms_fail(ctx, LRBMS_E_INVALID, "reduced_solve: bad argument");
  hipStream_t st = (hipStream_t)stream;
  const long S = t.S, per_q = S * 7 * N * N;
  RedWork w = red_work(S, N, work);
  hipLaunchKernelGGL(k3_combine, dim3((unsigned)((per_q + 255) / 256)), dim3(256), 0, st, per_q, Q, make_theta(Q, theta), B_sys, w.Amu);
  hipLaunchKernelGGL(k3_block_inverse, dim3(S), dim3(256), sizeof(double) * N * (2 * N + 1), st, N, w.Amu, w.Dinv);
  return red_cg(ctx, st, N, w, rhs_red, u, rtol, max_iter, info, nullptr, "reduced_solve");
}

// doubles of work per group of <= 16 parameters of the batched reduced solve
static long reduced_batch_group_size(long S, int N) {
  return S * 7 * N * N + S * N * N + 5 * S * N * 16 + 4 * S * 16 + 5 * 16 + 16 + 3 * S * 16;      // (+ y0, prc [2] of the coarse level)
}

int64_t lrbms3_reduced_solve_batch_work_size(lrbms3_ctx* ctx, int32_t N, int32_t nmu) {
  if (!ctx || !ctx->has_mesh || nmu < 1) return -1;
  return (int64_t)((nmu + 15) / 16) * reduced_batch_group_size(ctx->t.S, N);
}

}  // extern "C"

namespace {

// One group of <= 16 columns of the batched reduced solvers: its slice of the work array, its theta table, its stream and state.
struct RbGroup {
  int nm, m0;
  TB th;
  double *Amu, *Dinv, *r, *z, *po, *pn, *Ap, *prz, *ppap, *prr, *scal, *y0, *prc;
  hipStream_t st;
  bool done;
  double rel;
  int it, last_it;
  double look[32];                  // host: scal [3] (residuals) and [4] (|b|^2) as the last look at the group copied them
};

// the vectors, partials and scalars of a group from w on (5 S N 16 + 4 S 16 + 96 + 3 S 16 doubles)
void rb_group_vectors(RbGroup& G, double* w, long S, int N) {
  const long nv = S * N * 16;
  G.r = w;
  G.z = G.r + nv;
  G.po = G.z + nv;
  G.pn = G.po + nv;
  G.Ap = G.pn + nv;
  G.prz = G.Ap + nv;                // [2][S][16]: r.z partials of the last two updates (beta needs both)
  G.ppap = G.prz + 2 * S * 16;
  G.prr = G.ppap + S * 16;
  G.scal = G.prr + S * 16;          // [5][16]: only the residual norms ([3], [4]) are reduced by a kernel of their own
  G.y0 = G.scal + 5 * 16 + 16;      // coarse level: correction and its r.z contributions [2][S][16]
  G.prc = G.y0 + S * 16;
}

// What the iteration loop applies: sum_q th_qm B_q on the 7 slots, plus M_red on the self slot when it is given (the step operator
// of the implicit Euler, dt folded into th); A0inv: the coarse inverse [S][S] or nullptr; u: the panel the solve iterates in, ldx = nmu.
struct RbOp {
  int Q, N, nmu;
  const double *B_sys, *M_red, *A0inv;
  double* u;
};

// The panel matvec of one group: p_new = z + beta p_old (first: p_new = z), Ap = A p_new, in the matrix-core form with one or two
// row tiles or in the VALU form (LRBMS3_OPT_SOLVE_VALU); MASS adds M_red on the self slot.
template <bool MASS>
void launch_matvec3(lrbms3_ctx* ctx, const RbOp& op, RbGroup& G, int first, const double* rz_cur, const double* rz_nxt, const CoarseB& cb) {
  const T3& t = ctx->t;
  const long S = t.S;
  const int Q = op.Q, N = op.N;
  const size_t lds_mv = sizeof(double) * (7 * N * 16 + 32 * 16);
  const size_t lds_mm = sizeof(double) * (7 * 32 * 16 + 4 * (N <= 16 ? 1 : 2) * 256 + 32 * 16);
  const bool mfma_mv = ctx->opt_solve_valu == 0;
  MassOp3<MASS> mo;
  if constexpr (MASS) mo.M = op.M_red;
  if (mfma_mv && N <= 16)
    hipLaunchKernelGGL((k3b_matvec_mfma<1, MASS>), dim3(S), dim3(256), lds_mm, G.st, t, Q, N, G.nm, first, G.th, op.B_sys, G.z, G.po, G.pn,
                       G.Ap, rz_cur, rz_nxt, G.ppap, cb, mo);
  else if (mfma_mv)
    hipLaunchKernelGGL((k3b_matvec_mfma<2, MASS>), dim3(S), dim3(256), lds_mm, G.st, t, Q, N, G.nm, first, G.th, op.B_sys, G.z, G.po, G.pn,
                       G.Ap, rz_cur, rz_nxt, G.ppap, cb, mo);
  else
    hipLaunchKernelGGL(k3b_matvec<MASS>, dim3(S), dim3(512), lds_mv, G.st, t, Q, N, G.nm, first, G.th, op.B_sys, G.z, G.po, G.pn, G.Ap,
                       rz_cur, rz_nxt, G.ppap, cb, mo);
}

// The iteration loop of the batched reduced solvers from the state the start kernels left (G.it = 0, G.done = false): matvec /
// update / coarse apply per group, launches interleaved iteration by iteration over the groups' streams, a look at the residuals
// after first_block and then after every check iterations.  A group leaves at rel <= rtol, at max_iter (honoured exactly) or on a
// NaN (nan set).  The residual norms sit in scal [3], their references in scal [4].
int red_batch_iterate(lrbms3_ctx* ctx, const RbOp& op, RbGroup* g, int ng, int first_block, int check, double rtol, int max_iter,
                      bool& nan) {
  const long S = ctx->t.S;
  const int N = op.N, nmu = op.nmu;
  const double* A0inv = op.A0inv;
  double* u = op.u;
  const size_t lds_up = sizeof(double) * (N * 16 + 32 * 16);
  const bool mfma_mv = ctx->opt_solve_valu == 0;
  bool all_done = false;
  int block = first_block;
  while (!all_done) {
    for (int c = 0; c < block; ++c)
      for (int k = 0; k < ng; ++k) {
        RbGroup& G = g[k];
        if (G.done || G.it >= max_iter) continue;
        const int it = G.it;
        double* rz_cur = G.prz + (it & 1) * S * 16;          // written by the previous update (or the start kernel)
        double* rz_nxt = G.prz + ((it + 1) & 1) * S * 16;    // holds the r.z of the update before that until this update overwrites it
        double* rc_cur = G.prc + (it & 1) * S * 16;
        double* rc_nxt = G.prc + ((it + 1) & 1) * S * 16;
        const CoarseB cb{A0inv ? G.y0 : nullptr, rc_cur, rc_nxt};
        if (op.M_red) {
          KScope ks(ctx, mfma_mv ? "k3b_matvec_mfma<mass>" : "k3b_matvec<mass>", G.st);
          launch_matvec3<true>(ctx, op, G, it == 0 ? 1 : 0, rz_cur, rz_nxt, cb);
        } else {
          KScope ks(ctx, mfma_mv ? "k3b_matvec_mfma" : "k3b_matvec", G.st);
          launch_matvec3<false>(ctx, op, G, it == 0 ? 1 : 0, rz_cur, rz_nxt, cb);
        }
        hipLaunchKernelGGL(k3b_update, dim3(S), dim3(512), lds_up, G.st, N, G.nm, nmu, G.Dinv, G.pn, G.Ap, u + G.m0, G.r, G.z, (int)S,
                           rz_cur, A0inv ? rc_cur : nullptr, G.ppap, rz_nxt, G.prr);
        if (A0inv)    // the coarse correction of the new residual: read by the next matvec (direction) and by the next update (r.z)
          hipLaunchKernelGGL(k3b_coarse_apply, dim3((unsigned)((S + 15) / 16)), dim3(1024), 0, G.st, (int)S, N, G.nm, A0inv, G.r, G.y0,
                             rc_nxt);
        std::swap(G.po, G.pn);
        ++G.it;
      }
    block = check;
    for (int k = 0; k < ng; ++k) {
      RbGroup& G = g[k];
      if (G.done) continue;
      hipLaunchKernelGGL(k3b_reduce, dim3(1), dim3(256), 0, G.st, (int)S, G.nm, G.prr, G.scal + 48);
      LRBMS_HIP_CHECK(ctx, hipMemcpyAsync(G.look, G.scal + 48, sizeof(double) * 32, hipMemcpyDeviceToHost, G.st));   // [3] residuals, [4] |b|^2
    }
    LRBMS_LAUNCH_CHECK(ctx);
    all_done = true;
    for (int k = 0; k < ng; ++k) {
      RbGroup& G = g[k];
      if (G.done) continue;
      LRBMS_HIP_CHECK(ctx, hipStreamSynchronize(G.st));
      G.rel = 0.0;
      for (int m = 0; m < G.nm; ++m) {
        const double bbm = G.look[16 + m], rm = bbm > 0.0 ? sqrt(G.look[m] / bbm) : 0.0;
        if (!(rm == rm)) nan = true;
        G.rel = rm > G.rel ? rm : G.rel;
      }
      if (G.rel <= rtol || G.it >= max_iter || nan) G.done = true;
      if (!G.done) all_done = false;
    }
  }
  return LRBMS_OK;
}

// The group driver shared by lrbms3_reduced_solve_batch and lrbms3_reduced_solve_batch_src: K == 0 broadcasts
// rhs_red [S][N] to every column (k3b_init); K >= 1 gives column m the right-hand side sum_j phi[m][j] rhs_red[j] of
// rhs_red [K][S][N] (k3b_init_src, phi [nmu][K] on the device).  Everything behind the start kernel is the same launch sequence.
int red_batch_run(lrbms3_ctx* ctx, const std::string& name, int Q, int N, int nmu, const double* theta, const double* B_sys,
                  const double* rhs_red, int K, const double* phi, double* work, double* u, double rtol, int max_iter, double* info,
                  hipStream_t st) {
  const T3& t = ctx->t;
  const long S = t.S, per_q = S * 7 * N * N;
  // Up to four groups of <= 16 parameters, each an independent CG on its own stream (the caller's and the library's three side
  // streams): a group's kernels are 512 small workgroups that wait on memory most of the time, so two or three groups share the
  // chip at little cost to each other.  Launches are interleaved iteration by iteration; residuals are looked at together.
  const int ng = (nmu + 15) / 16;
  const long gsize = reduced_batch_group_size(S, N);
  RbGroup g[4];                       // (ahead of the fork: the groups' copies target it until the fork has left)
  StreamFork fork(ctx);
  if (int rc = fork.fork(st, ng)) return rc;
  const double* A0inv = ctx->user_pc_N == N ? ctx->user_pc : nullptr;
  for (int k = 0; k < ng; ++k) {
    RbGroup& G = g[k];
    G.m0 = 16 * k;
    G.nm = nmu - G.m0 < 16 ? nmu - G.m0 : 16;
    G.st = fork.stream(k);
    G.done = false;
    G.rel = 0.0;
    G.it = G.last_it = 0;
    double* w = work + k * gsize;
    G.Amu = w;                        // blocks at the group-mean theta: only its diagonal blocks are used (preconditioner)
    G.Dinv = G.Amu + per_q;
    rb_group_vectors(G, G.Dinv + S * N * N, S, N);
    G.th = TB{};
  }
  for (int k = 0; k < ng; ++k) {
    RbGroup& G = g[k];
    QV mean{};
    for (int m = 0; m < G.nm; ++m)
      for (int q = 0; q < Q; ++q) {
        G.th.v[m][q] = theta[(G.m0 + m) * Q + q];
        mean.v[q] += theta[(G.m0 + m) * Q + q] / G.nm;
      }
    if (A0inv) {
      G.Dinv = const_cast<double*>(A0inv) + S * S;      // the prebuilt preconditioner carries its inverse diagonal blocks (read only)
    } else {
      hipLaunchKernelGGL(k3_combine, dim3((unsigned)((per_q + 255) / 256)), dim3(256), 0, G.st, per_q, Q, mean, B_sys, G.Amu);
      hipLaunchKernelGGL(k3_block_inverse, dim3(S), dim3(256), sizeof(double) * N * (2 * N + 1), G.st, N, G.Amu, G.Dinv);
    }
    LRBMS_HIP_CHECK(ctx, hipMemsetAsync(G.scal, 0, sizeof(double) * 80, G.st));
    if (K == 0)
      hipLaunchKernelGGL(k3b_init, dim3(S), dim3(512), sizeof(double) * (N + 32 * 16), G.st, N, G.nm, nmu, rhs_red, G.Dinv, u + G.m0, G.r,
                         G.z, G.po, G.prz, G.prr);
    else
      hipLaunchKernelGGL(k3b_init_src, dim3(S), dim3(512), sizeof(double) * (N * 16 + 32 * 16), G.st, N, G.nm, nmu, K, S * N,
                         phi + (long)G.m0 * K, rhs_red, G.Dinv, u + G.m0, G.r, G.z, G.po, G.prz, G.prr);
    if (A0inv)
      hipLaunchKernelGGL(k3b_coarse_apply, dim3((unsigned)((S + 15) / 16)), dim3(1024), 0, G.st, (int)S, N, G.nm, A0inv, G.r, G.y0, G.prc);
    hipLaunchKernelGGL(k3b_reduce, dim3(1), dim3(256), 0, G.st, (int)S, G.nm, G.prr, G.scal + 64);
  }
  LRBMS_LAUNCH_CHECK(ctx);
  if (info) info[0] = 0, info[1] = 0;
  const int check = A0inv ? 12 : 8;    // iterations between two looks at the residuals (a host synchronisation each)
  bool nan = false;
  const RbOp op{Q, N, nmu, B_sys, nullptr, A0inv, u};
  if (int irc = red_batch_iterate(ctx, op, g, ng, check, check, rtol, max_iter, nan)) return irc;
  if (int jrc = fork.join()) return jrc;
  int it = 0;
  double rel = 0.0;
  for (int k = 0; k < ng; ++k) {
    it = g[k].it > it ? g[k].it : it;
    rel = g[k].rel > rel ? g[k].rel : rel;
  }
  if (info) info[0] = it, info[1] = rel;
  if (nan) return lrbms_fail(ctx, LRBMS_E_NOT_CONVERGED, name + ": NaN residual");
  if (rel > rtol) return lrbms_fail(ctx, LRBMS_E_NOT_CONVERGED, name + ": not converged");
  return LRBMS_OK;
}

}  // namespace

extern "C" {

int lrbms3_reduced_solve_batch(lrbms3_ctx* ctx, int32_t Q, int32_t N, int32_t nmu, const double* theta, const double* B_sys,
                               const double* rhs_red, double* work, double* u, double rtol, int32_t max_iter, double* info,
                               void* stream) {
  LRBMS_REQUIRE_MESH(ctx);
  if (ctx->t.S_ext != ctx->t.S) return lrbms_fail(ctx, LRBMS_E_INVALID, "reduced_solve_batch: needs all subdomains on this rank");
  if (Q < 1 || Q > 8 || N < 1 || N > 32 || nmu < 1 || nmu > 64 || !theta || !B_sys || !rhs_red || !work || !u)
    return lrbms_fail(ctx, LRBMS_E_INVALID, "reduced_solve_batch: needs N <= 32 and nmu <= 64");
  return red_batch_run(ctx, "reduced_solve_batch", Q, N, nmu, theta, B_sys, rhs_red, 0, nullptr, work, u, rtol, max_iter, info,
                       (hipStream_t)stream);
}

// phi [nmu][K] arrives on the host and goes to a ctx-owned device table (64 x 64 doubles, allocated on first use) on the caller's
// stream ahead of the fork, so the work size is that of lrbms3_reduced_solve_batch.  Only k3b_init_src reads the table, and every
// group has synchronised behind it before the call returns: the next call may overwrite it.
int lrbms3_reduced_solve_batch_src(lrbms3_ctx* ctx, int32_t Q, int32_t N, int32_t K, int32_t nmu, const double* theta,
                                   const double* phi, const double* B_sys, const double* rhs_red_K, double* work, double* u,
                                   double rtol, int32_t max_iter, double* info, void* stream) {
  LRBMS_REQUIRE_MESH(ctx);
  if (ctx->t.S_ext != ctx->t.S) return lrbms_fail(ctx, LRBMS_E_INVALID, "reduced_solve_batch_src: needs all subdomains on this rank");
  if (Q < 1 || Q > 8 || N < 1 || N > 32 || nmu < 1 || nmu > 64 || !theta || !phi || !B_sys || !rhs_red_K || !work || !u)
    return lrbms_fail(ctx, LRBMS_E_INVALID, "reduced_solve_batch_src: needs N <= 32 and nmu <= 64");
  if (K < 1 || K > 64) return lrbms_fail(ctx, LRBMS_E_INVALID, "reduced_solve_batch_src: need 1 <= K <= 64");
  hipStream_t st = (hipStream_t)stream;
  if (!ctx->src_phi) {
    void* p = nullptr;
    LRBMS_HIP_CHECK(ctx, hipMalloc(&p, sizeof(double) * 64 * 64));
    ctx->owned.push_back(p);
    ctx->src_phi = static_cast<double*>(p);
  }
  LRBMS_HIP_CHECK(ctx, hipMemcpyAsync(ctx->src_phi, phi, sizeof(double) * nmu * K, hipMemcpyHostToDevice, st));
  return red_batch_run(ctx, "reduced_solve_batch_src", Q, N, nmu, theta, B_sys, rhs_red_K, K, ctx->src_phi, work, u, rtol, max_iter,
                       info, st);
}

int64_t lrbms3_reduced_precond_size(lrbms3_ctx* ctx, int32_t N) {
  if (!ctx || !ctx->has_mesh || N < 1) return -1;
  return (int64_t)ctx->t.S * ctx->t.S + (int64_t)ctx->t.S * N * N;          // coarse inverse | inverse diagonal blocks
}

int64_t lrbms3_reduced_precond_work_size(lrbms3_ctx* ctx, int32_t N) {
  if (!ctx || !ctx->has_mesh || N < 1) return -1;
  const int64_t S = ctx->t.S;
  return std::max<int64_t>(2 * S * S + 2, S * 7 * N * N);
}

int lrbms3_reduced_precond_build(lrbms3_ctx* ctx, int32_t Q, int32_t N, const double* theta, const double* B_sys, double* work,
                                 double* pc, void* stream) {
  LRBMS_REQUIRE_MESH(ctx);
  const T3& t = ctx->t;
  if (t.S_ext != t.S) return lrbms_fail(ctx, LRBMS_E_INVALID, "reduced_precond_build: needs all subdomains on this rank");
  if (Q < 1 || Q > 8 || N < 1 || N > 32 || !theta || !B_sys || !work || !pc)
    return lrbms_fail(ctx, LRBMS_E_INVALID, "reduced_precond_build: bad argument (the batched solve it serves takes N <= 32)");
  hipStream_t st = (hipStream_t)stream;
  const long S = t.S;
  double* A0 = work;
  double* Id = A0 + S * S;
  rocblas_int* pinfo = (rocblas_int*)(Id + S * S);
  LRBMS_HIP_CHECK(ctx, hipMemsetAsync(A0, 0, sizeof(double) * 2 * S * S, st));
  hipLaunchKernelGGL(k3r_coarse_fill, dim3((unsigned)((S * 7 + 255) / 256)), dim3(256), 0, st, t, Q, N, make_theta(Q, theta), B_sys, A0, Id);
  LRBMS_LAUNCH_CHECK(ctx);
  rocblas_int hinfo = 0;
  if (int rc = dense_spd_inverse(ctx, st, S, A0, Id, pinfo, hinfo)) return rc;
  if (hinfo != 0) return lrbms_fail(ctx, LRBMS_E_INVALID, "reduced_precond_build: the coarse matrix is not positive definite (first basis vectors)");
  LRBMS_HIP_CHECK(ctx, hipMemcpyAsync(pc, Id, sizeof(double) * S * S, hipMemcpyDeviceToDevice, st));
  // the inverse diagonal blocks at the same reference parameter (the dense work is done: its space holds the combined blocks)
  const long per_q = S * 7 * N * N;
  hipLaunchKernelGGL(k3_combine, dim3((unsigned)((per_q + 255) / 256)), dim3(256), 0, st, per_q, Q, make_theta(Q, theta), B_sys, work);
  hipLaunchKernelGGL(k3_block_inverse, dim3(S), dim3(256), sizeof(double) * N * (2 * N + 1), st, N, work, pc + S * S);
  LRBMS_LAUNCH_CHECK(ctx);
  return LRBMS_OK;
}

int lrbms3_reduced_precond_use(lrbms3_ctx* ctx, int32_t N, const double* pc) {
  LRBMS_REQUIRE_MESH(ctx);
  ctx->user_pc = pc;
  ctx->user_pc_N = pc ? N : 0;
  return LRBMS_OK;
}

}  // extern "C"

namespace {

// The reduced counterpart, shared by lrbms3_reduced_implicit_euler and lrbms3_reduced_implicit_euler_src.
template <class F>
int red_euler_run(lrbms3_ctx* ctx, const char* name, int Q, int N, const double* theta, double dt, int nt, const double* B_sys,
                  const double* M_red, double* work, double* U, double rtol, int max_iter, double* info, hipStream_t st, F rhs_launch) {
  const T3& t = ctx->t;
  const long S = t.S, per_q = S * 7 * N * N, total = S * N;
  RedWork w = red_work(S, N, work);
  double* rhs = work + lrbms3_reduced_solve_work_size(ctx, N);
  double* part = rhs + total;
  double* ff = part + S;
  QV th = make_theta(Q, theta);
  for (int q = 0; q < Q; ++q) th.v[q] *= dt;
  // M_red + dt sum_q theta_q B_sys_q, the mass on the self slot; zero-padded columns keep a zero diagonal there, so the block
  // inverse puts the identity on them and the padded unknowns stay exactly 0
  hipLaunchKernelGGL(k3_combine, dim3((unsigned)((per_q + 255) / 256)), dim3(256), 0, st, per_q, Q, th, B_sys, w.Amu);
  hipLaunchKernelGGL(k3p_red_add_mass, dim3((unsigned)((S * N * N + 255) / 256)), dim3(256), 0, st, S * N * N, N, M_red, w.Amu);
  hipLaunchKernelGGL(k3_block_inverse, dim3(S), dim3(256), sizeof(double) * N * (2 * N + 1), st, N, w.Amu, w.Dinv);
  LRBMS_LAUNCH_CHECK(ctx);
  const size_t lds = sizeof(double) * (7 * N + 64);
  double iters = 0.0, worst = 0.0;
  if (info) info[0] = 0, info[1] = 0;
  for (int k = 0; k < nt; ++k) {
    const double* uk = U + (long)k * total;
    double* un = U + (long)(k + 1) * total;
    // K u_k by the CG's matvec (first iteration: p = z = u_k), into Ap
    hipLaunchKernelGGL(k3_pcg_matvec, dim3(S), dim3(64), lds, st, t, N, 1, w.Amu, uk, uk, w.p1, w.Ap, w.prz0, w.prz1, w.ppap);
    rhs_launch(k, uk, w.Ap, rhs, part);
    launch_reduce1(st, (int)S, part, ff);
    LRBMS_LAUNCH_CHECK(ctx);
    double inf[2] = {0.0, 0.0};
    int rc = red_cg(ctx, st, N, w, rhs, un, rtol, max_iter, inf, ff, name);
    iters += inf[0];
    worst = std::max(worst, inf[1]);
    if (info) info[0] = iters, info[1] = worst;
    if (rc != LRBMS_OK && rc != LRBMS_E_NOT_CONVERGED) return rc;
    // (also behind a step that missed rtol: U[k + 1] holds the iterate u_k + d, as the batched exports leave it, not the bare correction)
    hipLaunchKernelGGL(k3p_axpy, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, total, uk, un);
    LRBMS_LAUNCH_CHECK(ctx);
    if (rc != LRBMS_OK) return rc;
  }
  return LRBMS_OK;
}

}  // namespace

extern "C" {

int64_t lrbms3_reduced_implicit_euler_work_size(lrbms3_ctx* ctx, int32_t N) {
  const int64_t base = lrbms3_reduced_solve_work_size(ctx, N);
  if (base < 0) return -1;
  return base + (int64_t)ctx->t.S * N + ctx->t.S + 16;    // + right-hand side of the correction, partial |f|^2, |f|^2
}

int lrbms3_reduced_implicit_euler(lrbms3_ctx* ctx, int32_t Q, int32_t N, const double* theta, double dt, int32_t nt,
                                  const double* B_sys, const double* M_red, const double* rhs_red, double* work, double* U,
                                  double rtol, int32_t max_iter, double* info, void* stream) {
  LRBMS_REQUIRE_MESH(ctx);
  const T3& t = ctx->t;
  if (t.S_ext != t.S) return lrbms_fail(ctx, LRBMS_E_INVALID, "reduced_implicit_euler: needs all subdomains on this rank");
  if (Q < 1 || Q > 8 || N < 1 || N > 64 || !theta || !B_sys || !M_red || !rhs_red || !work || !U)
    return lrbms_fail(ctx, LRBMS_E_INVALID, "reduced_implicit_euler: bad argument");
  if (!(dt > 0.0) || nt < 1) return lrbms_fail(ctx, LRBMS_E_INVALID, "reduced_implicit_euler: dt > 0 and nt >= 1 required");
  hipStream_t st = (hipStream_t)stream;
  return red_euler_run(ctx, "reduced_implicit_euler", Q, N, theta, dt, nt, B_sys, M_red, work, U, rtol, max_iter, info, st,
                       [&](int, const double* uk, const double* Ku, double* rhs, double* part) {
                         hipLaunchKernelGGL(k3p_red_rhs, dim3(t.S), dim3(64), 0, st, N, dt, M_red, uk, rhs_red, Ku, rhs, part);
                       });
}

int lrbms3_reduced_implicit_euler_src(lrbms3_ctx* ctx, int32_t Q, int32_t N, int32_t K, const double* theta, double dt, int32_t nt,
                                      const double* B_sys, const double* M_red, const double* rhs_red_K, const double* phi,
                                      double* work, double* U, double rtol, int32_t max_iter, double* info, void* stream) {
  LRBMS_REQUIRE_MESH(ctx);
  const T3& t = ctx->t;
  if (t.S_ext != t.S) return lrbms_fail(ctx, LRBMS_E_INVALID, "reduced_implicit_euler_src: needs all subdomains on this rank");
  if (Q < 1 || Q > 8 || N < 1 || N > 64 || !theta || !B_sys || !M_red || !rhs_red_K || !phi || !work || !U)
    return lrbms_fail(ctx, LRBMS_E_INVALID, "reduced_implicit_euler_src: bad argument");
  if (K < 1 || K > 64) return lrbms_fail(ctx, LRBMS_E_INVALID, "reduced_implicit_euler_src: need 1 <= K <= 64");
  if (!(dt > 0.0) || nt < 1) return lrbms_fail(ctx, LRBMS_E_INVALID, "reduced_implicit_euler_src: dt > 0 and nt >= 1 required");
  hipStream_t st = (hipStream_t)stream;
  return red_euler_run(ctx, "reduced_implicit_euler_src", Q, N, theta, dt, nt, B_sys, M_red, work, U, rtol, max_iter, info, st,
                       [&](int step, const double* uk, const double* Ku, double* rhs, double* part) {
                         hipLaunchKernelGGL(k3p_red_rhs_src, dim3(t.S), dim3(64), 0, st, N, dt, M_red, uk, K, (long)t.S * N,
                                            phi + (long)(step + 1) * K, rhs_red_K, Ku, rhs, part);
                       });
}

}  // extern "C"

namespace {

// doubles ahead of the groups in the work array of the batched trajectories: the step operator at the call-mean theta, its inverse
// diagonal blocks, the coarse matrix and its inverse, the info word of the factorisation
long red_euler_batch_shared_size(long S, int N) { return S * 7 * N * N + S * N * N + 2 * S * S + 2; }
// a group without blocks of its own (reduced_batch_group_size carries a group-mean operator and its block inverse)
long red_euler_batch_group_size(long S, int N) { return reduced_batch_group_size(S, N) - S * 7 * N * N - S * N * N; }

// The driver of lrbms3_reduced_implicit_euler_batch(_src): a loop over the steps around red_batch_iterate.  K == 0: rhs [S][N] for
// every column and step; K >= 1: rhs [K][S][N], phi_dev [nmu][nt+1][K] (device), step k takes row k + 1.  tv == false: theta [nmu][Q],
// the groups' tables are filled once; tv == true (lrbms3_reduced_implicit_euler_batch_tv): theta_t [nmu][nt+1][Q],
// the tables are refilled with dt x row k + 1 ahead of the step k -> k + 1, the preconditioner sits at the time mean (ThetaRows::bar).
int red_euler_batch_run(lrbms3_ctx* ctx, const std::string& name, bool tv, int Q, int N, int nmu, const double* theta, double dt, int nt,
                        const double* B_sys, const double* M_red, const double* rhs, int K, const double* phi_dev, double* work,
                        double* U, double rtol, int max_iter, double* info, hipStream_t st) {
  const T3& t = ctx->t;
  const long S = t.S, per_q = S * 7 * N * N, rows = S * N;
  const int ng = (nmu + 15) / 16;
  if (info) info[0] = 0, info[1] = 0;
  // ---- the preconditioner of the call, on the caller's stream ahead of the fork, shared by all groups: inverse diagonal blocks
  // of M_red + dt sum_q mean(theta)_q B_q (zero-padded basis columns keep a zero diagonal: the identity there, they stay exactly 0)
  // and the coarse level on the first local basis vectors of that operator.  A preconditioner installed with
  // lrbms3_reduced_precond_use belongs to A and is neither read nor replaced.
  double* Amu = work;
  double* Dinv = Amu + per_q;
  double* A0 = Dinv + S * N * N;
  double* Id = A0 + S * S;
  rocblas_int* pinfo = (rocblas_int*)(Id + S * S);
  double* gwork = Id + S * S + 2;
  const ThetaRows tr{theta, Q, tv ? nt + 1 : 0};
  QV mean{}, one{};
  for (int m = 0; m < nmu; ++m)
    for (int q = 0; q < Q; ++q) mean.v[q] += tr.bar(m, q) / nmu;
  for (int q = 0; q < Q; ++q) mean.v[q] *= dt;
  one.v[0] = 1.0;
  hipLaunchKernelGGL(k3_combine, dim3((unsigned)((per_q + 255) / 256)), dim3(256), 0, st, per_q, Q, mean, B_sys, Amu);
  hipLaunchKernelGGL(k3p_red_add_mass, dim3((unsigned)((S * N * N + 255) / 256)), dim3(256), 0, st, S * N * N, N, M_red, Amu);
  hipLaunchKernelGGL(k3_block_inverse, dim3(S), dim3(256), sizeof(double) * N * (2 * N + 1), st, N, Amu, Dinv);
  LRBMS_HIP_CHECK(ctx, hipMemsetAsync(A0, 0, sizeof(double) * 2 * S * S, st));
  hipLaunchKernelGGL(k3r_coarse_fill, dim3((unsigned)((S * 7 + 255) / 256)), dim3(256), 0, st, t, 1, N, one, Amu, A0, Id);
  LRBMS_LAUNCH_CHECK(ctx);
  rocblas_int hinfo = 0;
  if (int rc = dense_spd_inverse(ctx, st, S, A0, Id, pinfo, hinfo)) return rc;
  const double* A0inv = nullptr;       // not positive definite (a zeroed first basis vector): block-Jacobi alone
  if (hinfo == 0) A0inv = Id;
  RbGroup g[4];                        // (ahead of the fork: the groups' copies target it until the fork has left)
  StreamFork fork(ctx);
  if (int frc = fork.fork(st, ng)) return frc;
  const long gsize = red_euler_batch_group_size(S, N);
  for (int k = 0; k < ng; ++k) {
    RbGroup& G = g[k];
    G.m0 = 16 * k;
    G.nm = nmu - G.m0 < 16 ? nmu - G.m0 : 16;
    G.st = fork.stream(k);
    G.done = false;
    G.rel = 0.0;
    G.it = G.last_it = 0;
    G.Amu = Amu;
    G.Dinv = Dinv;
    rb_group_vectors(G, gwork + k * gsize, S, N);
    G.th = TB{};
    for (int m = 0; m < G.nm; ++m)
      for (int q = 0; q < Q; ++q) G.th.v[m][q] = dt * tr.at(G.m0 + m, 0, q);          // dt folded into the table (tv: refilled per step)
  }
  for (int k = 0; k < ng; ++k) LRBMS_HIP_CHECK(ctx, hipMemsetAsync(g[k].scal, 0, sizeof(double) * 80, g[k].st));
  const int check = A0inv ? 12 : 8;
  const size_t lds_si = sizeof(double) * (2 * N * 16 + 32 * 16);
  const CoarseB none{nullptr, nullptr, nullptr};
  bool nan = false, capped = false;
  long total_it = 0;
  double worst = 0.0;
  for (int step = 0; step < nt && !nan && !capped; ++step) {
    const double* uk = U + (long)step * rows * nmu;
    double* un = U + (long)(step + 1) * rows * nmu;
    const RbOp op{Q, N, nmu, B_sys, M_red, A0inv, un};
    // ---- step start of every group, no look at the host: y = (M + dt A_m) u_k by the MASS matvec (first = 1, direction u_k
    // gathered into the group's z, no coarse correction), then k3b_step_init
    for (int k = 0; k < ng; ++k) {
      RbGroup& G = g[k];
      const long vec = rows * G.nm;
      for (int m = 0; tv && m < G.nm; ++m)      // the operator of the step k -> k + 1: row k + 1
        for (int q = 0; q < Q; ++q) G.th.v[m][q] = dt * tr.at(G.m0 + m, step + 1, q);
      hipLaunchKernelGGL(k3b_gather, dim3((unsigned)((vec + 255) / 256 > 4096 ? 4096 : (vec + 255) / 256)), dim3(256), 0, G.st, rows, G.nm,
                         nmu, uk + G.m0, G.z);
      launch_matvec3<true>(ctx, op, G, 1, G.prz, G.prz, none);
      hipLaunchKernelGGL(k3b_step_init, dim3(S), dim3(512), lds_si, G.st, N, G.nm, nmu, dt, M_red, uk + G.m0, K, rows, (long)(nt + 1) * K,
                         K ? phi_dev + ((long)G.m0 * (nt + 1) + step + 1) * K : nullptr, rhs, G.Ap, Dinv, un + G.m0, G.r, G.z, G.po,
                         G.prz, G.prr, G.ppap);
      if (A0inv)
        hipLaunchKernelGGL(k3b_coarse_apply, dim3((unsigned)((S + 15) / 16)), dim3(1024), 0, G.st, (int)S, N, G.nm, A0inv, G.r, G.y0, G.prc);
      hipLaunchKernelGGL(k3b_reduce, dim3(1), dim3(256), 0, G.st, (int)S, G.nm, G.ppap, G.scal + 64);      // |f_m|^2: the step's reference
      G.it = 0;
      G.done = false;
    }
    LRBMS_LAUNCH_CHECK(ctx);
    // the first block goes out with the start kernels, a little short of what the previous step took
    int block = check;
    for (int k = 0; k < ng; ++k) {
      const int guess = (int)(0.8 * g[k].last_it);
      if (guess > block) block = guess;
    }
    if (int rc = red_batch_iterate(ctx, op, g, ng, block, check, rtol, max_iter, nan)) return rc;
    int it = 0;
    for (int k = 0; k < ng; ++k) {
      RbGroup& G = g[k];
      G.last_it = G.it;
      it = G.it > it ? G.it : it;
      worst = G.rel > worst ? G.rel : worst;
      if (G.rel > rtol) capped = true;
    }
    total_it += it;                    // the iterations of the slowest group, summed over the steps
  }
  if (int jrc = fork.join()) return jrc;
  if (info) info[0] = (double)total_it, info[1] = worst;
  if (nan) return lrbms_fail(ctx, LRBMS_E_NOT_CONVERGED, name + ": NaN residual");
  if (capped) return lrbms_fail(ctx, LRBMS_E_NOT_CONVERGED, name + ": not converged");
  return LRBMS_OK;
}

}  // namespace

extern "C" {

int64_t lrbms3_reduced_implicit_euler_batch_work_size(lrbms3_ctx* ctx, int32_t N, int32_t nmu) {
  if (!ctx || !ctx->has_mesh || N < 1 || nmu < 1) return -1;
  const long S = ctx->t.S;
  return red_euler_batch_shared_size(S, N) + (int64_t)((nmu + 15) / 16) * red_euler_batch_group_size(S, N);
}

int lrbms3_reduced_implicit_euler_batch(lrbms3_ctx* ctx, int32_t Q, int32_t N, int32_t nmu, const double* theta, double dt, int32_t nt,
                                        const double* B_sys, const double* M_red, const double* rhs_red, double* work, double* U,
                                        double rtol, int32_t max_iter, double* info, void* stream) {
  LRBMS_REQUIRE_MESH(ctx);
  if (ctx->t.S_ext != ctx->t.S) return lrbms_fail(ctx, LRBMS_E_INVALID, "reduced_implicit_euler_batch: needs all subdomains on this rank");
  if (Q < 1 || Q > 8 || N < 1 || N > 32 || nmu < 1 || nmu > 64 || !theta || !B_sys || !M_red || !rhs_red || !work || !U)
    return lrbms_fail(ctx, LRBMS_E_INVALID, "reduced_implicit_euler_batch: needs N <= 32 and nmu <= 64");
  if (!(dt > 0.0) || nt < 1) return lrbms_fail(ctx, LRBMS_E_INVALID, "reduced_implicit_euler_batch: dt > 0 and nt >= 1 required");
  return red_euler_batch_run(ctx, "reduced_implicit_euler_batch", false, Q, N, nmu, theta, dt, nt, B_sys, M_red, rhs_red, 0, nullptr, work, U,
                             rtol, max_iter, info, (hipStream_t)stream);
}

int lrbms3_reduced_implicit_euler_batch_src(lrbms3_ctx* ctx, int32_t Q, int32_t N, int32_t K, int32_t nmu, const double* theta, double dt,
                                            int32_t nt, const double* B_sys, const double* M_red, const double* rhs_red_K,
                                            const double* phi, double* work, double* U, double rtol, int32_t max_iter, double* info,
                                            void* stream) {
  LRBMS_REQUIRE_MESH(ctx);
  if (ctx->t.S_ext != ctx->t.S)
    return lrbms_fail(ctx, LRBMS_E_INVALID, "reduced_implicit_euler_batch_src: needs all subdomains on this rank");
  if (Q < 1 || Q > 8 || N < 1 || N > 32 || nmu < 1 || nmu > 64 || !theta || !B_sys || !M_red || !rhs_red_K || !phi || !work || !U)
    return lrbms_fail(ctx, LRBMS_E_INVALID, "reduced_implicit_euler_batch_src: needs N <= 32 and nmu <= 64");
  if (K < 1 || K > 64) return lrbms_fail(ctx, LRBMS_E_INVALID, "reduced_implicit_euler_batch_src: need 1 <= K <= 64");
  if (!(dt > 0.0) || nt < 1) return lrbms_fail(ctx, LRBMS_E_INVALID, "reduced_implicit_euler_batch_src: dt > 0 and nt >= 1 required");
  return red_euler_batch_run(ctx, "reduced_implicit_euler_batch_src", false, Q, N, nmu, theta, dt, nt, B_sys, M_red, rhs_red_K, K, phi, work, U,
                             rtol, max_iter, info, (hipStream_t)stream);
}

// theta_t [nmu][nt+1][Q] host; K == 0: rhs_red_K is rhs_red [S][N] and phi is null, K >= 1: rhs_red_K [K][S][N] and phi (device)
int lrbms3_reduced_implicit_euler_batch_tv(lrbms3_ctx* ctx, int32_t Q, int32_t N, int32_t K, int32_t nmu, const double* theta_t, double dt,
                                           int32_t nt, const double* B_sys, const double* M_red, const double* rhs_red_K,
                                           const double* phi, double* work, double* U, double rtol, int32_t max_iter, double* info,
                                           void* stream) {
  LRBMS_REQUIRE_MESH(ctx);
  if (ctx->t.S_ext != ctx->t.S)
    return lrbms_fail(ctx, LRBMS_E_INVALID, "reduced_implicit_euler_batch_tv: needs all subdomains on this rank");
  if (Q < 1 || Q > 8 || N < 1 || N > 32 || nmu < 1 || nmu > 64 || !theta_t || !B_sys || !M_red || !rhs_red_K || !work || !U)
    return lrbms_fail(ctx, LRBMS_E_INVALID, "reduced_implicit_euler_batch_tv: needs N <= 32 and nmu <= 64");
  if (K < 0 || K > 64 || (K > 0) != (phi != nullptr))
    return lrbms_fail(ctx, LRBMS_E_INVALID, "reduced_implicit_euler_batch_tv: need 0 <= K <= 64, phi with K >= 1 and null with K = 0");
  if (!(dt > 0.0) || nt < 1) return lrbms_fail(ctx, LRBMS_E_INVALID, "reduced_implicit_euler_batch_tv: dt > 0 and nt >= 1 required");
  return red_euler_batch_run(ctx, "reduced_implicit_euler_batch_tv", true, Q, N, nmu, theta_t, dt, nt, B_sys, M_red, rhs_red_K, K, phi, work,
                             U, rtol, max_iter, info, (hipStream_t)stream);
}

int64_t lrbms3_reduced_time_residual_work_size(lrbms3_ctx* ctx, int32_t N) {
  if (!ctx || !ctx->has_mesh) return -1;
  const int64_t S = ctx->t.S;
  return S * 7 * N * N + S * N * N;
}

int lrbms3_reduced_time_residual(lrbms3_ctx* ctx, int32_t Q, int32_t N, int32_t L, const double* theta, const double* B_sys,
                                 const double* M_red, const double* dU, double* work, double* out, void* stream) {
  LRBMS_REQUIRE_MESH(ctx);
  const T3& t = ctx->t;
  if (t.S_ext != t.S) return lrbms_fail(ctx, LRBMS_E_INVALID, "reduced_time_residual: needs all subdomains on this rank");
  if (Q < 1 || Q > 8 || N < 1 || N > 64 || L < 1 || L > 65535 || !theta || !B_sys || !M_red || !dU || !work || !out)
    return lrbms_fail(ctx, LRBMS_E_INVALID, "reduced_time_residual: bad argument");
  hipStream_t st = (hipStream_t)stream;
  const long S = t.S, per_q = S * 7 * N * N, NN = (long)N * N;
  double* Amu = work;
  double* Minv = Amu + per_q;
  // M_red^-1 by the reduced solver's block inverse, which reads the self slot of a 7-slot operator: M_red goes to slot 3 of Amu
  // first (its zero-diagonal rule: the identity on padded columns), then Amu receives the combined operator
  LRBMS_HIP_CHECK(ctx, hipMemcpy2DAsync(Amu + 3 * NN, sizeof(double) * 7 * NN, M_red, sizeof(double) * NN, sizeof(double) * NN, S,
                             hipMemcpyDeviceToDevice, st));
  hipLaunchKernelGGL(k3_block_inverse, dim3(S), dim3(256), sizeof(double) * N * (2 * N + 1), st, N, Amu, Minv);
  hipLaunchKernelGGL(k3_combine, dim3((unsigned)((per_q + 255) / 256)), dim3(256), 0, st, per_q, Q, make_theta(Q, theta), B_sys, Amu);
  hipLaunchKernelGGL(k3p_time_residual, dim3(S, L), dim3(64), sizeof(double) * (8 * N + 64), st, t, N, Amu, Minv, dU, out);
  LRBMS_LAUNCH_CHECK(ctx);
  return LRBMS_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------- batched parabolic estimate
// lrbms3_reduced_parabolic_estimate_batch: the parabolic estimate of the nmu <= 64 trajectories of one panel
// U [nt+1][S][N][nmu].  The elliptic rows come from the batched estimate on every slab (launch_reduced_estimate_batch), the nc form of
// the differences from k3_estimate_nc_batch16, the time residual from the panel matvec on gathered columns; the kernels below are the
// glue: differences, the per-column tables of the source terms, M_red^-1 y . y per panel, and the combination into the five outputs.
namespace {

__global__ __launch_bounds__(256) void k3pe_diff(long total, const double* __restrict__ U, double* __restrict__ dU, long slab) {
  for (long k = (long)blockIdx.x * 256 + threadIdx.x; k < total; k += (long)gridDim.x * 256) dU[k] = U[k + slab] - U[k];
}

// theta of the group's columns into thd [nmu][Q], and its rows of phi [nmu][nt+1][K] into phid [nt+1][nmu][K] (the layout
// k3_source_terms takes per step: one coefficient row per column)
__global__ __launch_bounds__(256) void k3pe_tables(int Q, int K, int nmu, int nt, int m0, int nm, TB th, const double* __restrict__ phi,
                                                   double* __restrict__ thd, double* __restrict__ phid) {
  const int tid = threadIdx.x;
  for (int i = tid; i < nm * Q; i += 256) thd[(long)m0 * Q + i] = th.v[i / Q][i % Q];
  const long per = (long)(nt + 1) * K;
  for (long i = tid; i < nm * per; i += 256) {
    const long m = m0 + i / per, r = i % per, k = r / K, j = r % K;
    phid[(k * nmu + m) * K + j] = phi[m * per + r];
  }
}

// The per-step variant of k3pe_tables (lrbms3_reduced_parabolic_estimate_batch_tv): row k of the group's columns, theta from the
// kernel argument into thd_t [nt+1][nmu][Q], phi [nmu][nt+1][K] into phid [nt+1][nmu][K]
__global__ __launch_bounds__(256) void k3pe_tables_tv(int Q, int K, int nmu, int nt, int k, int m0, int nm, TB th,
                                                      const double* __restrict__ phi, double* __restrict__ thd_t,
                                                      double* __restrict__ phid) {
  const int tid = threadIdx.x;
  for (int i = tid; i < nm * Q; i += 256) thd_t[((long)k * nmu + m0) * Q + i] = th.v[i / Q][i % Q];
  for (int i = tid; i < nm * K; i += 256) {
    const long m = m0 + i / K, j = i % K;
    phid[((long)k * nmu + m) * K + j] = phi[(m * (nt + 1) + k) * K + j];
  }
}

// A chunk of a host table into the work array in stream order: the chunk is the kernel argument (2 KB), so no copy from pageable
// host memory and no host synchronisation (2D: k_pe_put)
struct PeChunk { double v[256]; };
__global__ __launch_bounds__(256) void k3pe_put(int n, PeChunk c, double* __restrict__ dst) {
  if ((int)threadIdx.x < n) dst[threadIdx.x] = c.v[threadIdx.x];
}

// out[s ldo + m] = y^T Minv[s] y for the columns m < nm of the compact panel y [S][N][nm] (N <= 32): one workgroup per subdomain,
// the panel in the LDS, thread = (row group tid >> 4, column tid & 15) -- the 16 lanes of a row group share the row of the inverse --
// and the products y_i (Minv y)_i summed over the rows in ascending order
__global__ __launch_bounds__(256) void k3pe_inv_norm2_panel(int N, int nm, int ldo, const double* __restrict__ Minv,
                                                            const double* __restrict__ y, double* __restrict__ out) {
  __shared__ double ys[32 * 16], pr[32 * 16];
  const int s = blockIdx.x, tid = threadIdx.x, g = tid >> 4, m = tid & 15;
  for (int k = tid; k < N * 16; k += 256) {
    const int i = k >> 4, mm = k & 15;
    ys[k] = mm < nm ? y[((long)s * N + i) * nm + mm] : 0.0;
  }
  __syncthreads();
  for (int i = g; i < N; i += 16) {
    const double* D = Minv + ((long)s * N + i) * N;
    double z = 0.0;
    for (int j = 0; j < N; ++j) z += D[j] * ys[j * 16 + m];
    pr[i * 16 + m] = ys[i * 16 + m] * z;
  }
  __syncthreads();
  if (tid < nm) {
    double a = 0.0;
    for (int i = 0; i < N; ++i) a += pr[i * 16 + tid];
    out[(long)s * ldo + tid] = a;
  }
}

struct PeCoef { double v[64][2]; };      // coef [nmu][2]: one kernel argument (1 KB)
// the two coefficients of (column m, step k): from the kernel argument (k3pe_combine), from the table [nmu][nt+1][2] (k3pe_combine_tv)
struct PeCoefArg {
  const PeCoef& cf;
  __device__ double get(int m, int, int i) const { return cf.v[m][i]; }
};
struct PeCoefTable {
  const double* __restrict__ coef;
  int nt;
  __device__ double get(int m, int k, int i) const { return coef[((long)m * (nt + 1) + k) * 2 + i]; }
};

// The five outputs from the raw rows: one workgroup per 16 columns, thread = (part tid >> 4, column tid & 15).  Sums over the
// subdomains: part g takes s = g, g + 16, ... in ascending order, the 16 parts are then added in their order.
//   raw [nt+1][3][S][nmu] (nc, r, df of U[k]), src [nt+1][S][nmu] or nullptr (the f terms of the r row), ncd [nt][3][S][nmu] (row 0:
//   nc of the differences), tr2 [nt][S][nmu] (y^T M_red^-1 y)
template <class CF>
__device__ __forceinline__ void pe_combine_body(int S, int nmu, int nt, double dt, const CF& cf, const double* __restrict__ raw,
                                                const double* __restrict__ src, const double* __restrict__ ncd,
                                                const double* __restrict__ tr2, double* __restrict__ eta_loc,
                                                double* __restrict__ tdnc, double* __restrict__ tres, double* __restrict__ eta,
                                                double* __restrict__ est) {
  __shared__ double buf[2][16 * 16];
  const int tid = threadIdx.x, g = tid >> 4, mm = tid & 15, m = blockIdx.x * 16 + mm;
  const bool on = m < nmu;
  const double sc = 2.0 * sqrt(dt / 3.0);
  const long SM = (long)S * nmu, row = (long)(nt + 1) * SM;
  double e2 = 0.0, r2 = 0.0, d2 = 0.0;      // squares of eta, time_residual, time_deriv_nc (meaningful in part 0)
  for (int k = 0; k <= nt; ++k) {
    double a_nc = 0.0, a_rd = 0.0;
    if (on)
      for (int s = g; s < S; s += 16) {
        const long o = (long)s * nmu + m;
        const double nc = raw[(k * 3L + 0) * SM + o], df = raw[(k * 3L + 2) * SM + o];
        double r = raw[(k * 3L + 1) * SM + o];
        if (src) r += src[k * SM + o];
        eta_loc[k * SM + o] = nc * sc;
        eta_loc[row + k * SM + o] = r * sc;
        eta_loc[2 * row + k * SM + o] = df * sc;
        a_nc += nc * nc;
        a_rd += (r + df) * (r + df);
      }
    __syncthreads();
    buf[0][tid] = a_nc;
    buf[1][tid] = a_rd;
    __syncthreads();
    if (g == 0 && on) {
      double s_nc = 0.0, s_rd = 0.0;
      for (int p = 0; p < 16; ++p) {
        s_nc += buf[0][p * 16 + mm];
        s_rd += buf[1][p * 16 + mm];
      }
      const double ek = sc * (cf.get(m, k, 0) * sqrt(s_nc) + cf.get(m, k, 1) * sqrt(s_rd));
      eta[(long)k * nmu + m] = ek;
      e2 += ek * ek;
    }
  }
  for (int k = 0; k < nt; ++k) {
    double a_tr = 0.0, a_td = 0.0;
    if (on)
      for (int s = g; s < S; s += 16) {
        const long o = (long)s * nmu + m;
        const double v = ncd[k * 3L * SM + o], q = (v > 0.0 ? v : 0.0) / dt;
        tdnc[k * SM + o] = sqrt(q);
        a_td += q;
        a_tr += tr2[k * SM + o];
      }
    __syncthreads();
    buf[0][tid] = a_tr;
    buf[1][tid] = a_td;
    __syncthreads();
    if (g == 0 && on) {
      double s_tr = 0.0, s_td = 0.0;
      for (int p = 0; p < 16; ++p) {
        s_tr += buf[0][p * 16 + mm];
        s_td += buf[1][p * 16 + mm];
      }
      const double tk = sqrt(dt / 3.0 * s_tr);
      tres[(long)k * nmu + m] = tk;
      r2 += tk * tk;
      d2 += s_td;
    }
  }
  if (g == 0 && on) est[m] = sqrt(e2) + sqrt(r2) + sqrt(d2);
}

__global__ __launch_bounds__(256) void k3pe_combine(int S, int nmu, int nt, double dt, PeCoef cf, const double* __restrict__ raw,
                                                    const double* __restrict__ src, const double* __restrict__ ncd,
                                                    const double* __restrict__ tr2, double* __restrict__ eta_loc,
                                                    double* __restrict__ tdnc, double* __restrict__ tres, double* __restrict__ eta,
                                                    double* __restrict__ est) {
  pe_combine_body(S, nmu, nt, dt, PeCoefArg{cf}, raw, src, ncd, tr2, eta_loc, tdnc, tres, eta, est);
}

// k3pe_combine with the coefficients per (column, step) from coef [nmu][nt+1][2] on the device: the same thread mapping and summation
// order, so a table that is constant in time gives the bits of k3pe_combine
__global__ __launch_bounds__(256) void k3pe_combine_tv(int S, int nmu, int nt, double dt, const double* __restrict__ coef,
                                                       const double* __restrict__ raw, const double* __restrict__ src,
                                                       const double* __restrict__ ncd, const double* __restrict__ tr2,
                                                       double* __restrict__ eta_loc, double* __restrict__ tdnc,
                                                       double* __restrict__ tres, double* __restrict__ eta, double* __restrict__ est) {
  pe_combine_body(S, nmu, nt, dt, PeCoefTable{coef, nt}, raw, src, ncd, tr2, eta_loc, tdnc, tres, eta, est);
}

// doubles of work: raw, dU, ncd, tr2, src | thd [64][8], phid [nt+1][nmu][64] | Minv, the 7-slot copy of M_red the block inverse
// reads | one group's panel vectors z, p, y [S][N][16] and partials [S][16]
long pe_batch3_work_size(long S, long N, long nmu, long nt) {
  return (nt + 1) * 3 * S * nmu + nt * S * N * nmu + nt * 3 * S * nmu + nt * S * nmu + (nt + 1) * S * nmu + 64 * 8 + (nt + 1) * nmu * 64 +
         S * N * N + 7 * S * N * N + 3 * S * N * 16 + S * 16;
}
// behind the work of the twin, the tables of the _tv form: thd_t [nt+1][nmu][8], coef [nmu][nt+1][2]
long pe_batch3_tv_extra(long nmu, long nt) { return (nt + 1) * nmu * 8 + ((nmu * (nt + 1) * 2 + 15) & ~15L); }

}  // namespace

extern "C" {

int64_t lrbms3_reduced_parabolic_estimate_batch_work_size(lrbms3_ctx* ctx, int32_t N, int32_t nmu, int32_t nt) {
  if (!ctx || !ctx->has_mesh || N < 1 || N > 32 || nmu < 1 || nmu > 64 || nt < 1) return -1;
  return pe_batch3_work_size(ctx->t.S, N, nmu, nt);
}

int64_t lrbms3_reduced_parabolic_estimate_batch_tv_work_size(lrbms3_ctx* ctx, int32_t N, int32_t nmu, int32_t nt) {
  const int64_t base = lrbms3_reduced_parabolic_estimate_batch_work_size(ctx, N, nmu, nt);
  return base < 0 ? -1 : base + pe_batch3_tv_extra(nmu, nt);
}

}  // extern "C"

namespace {

#define LRBMS3_PE_PARAMS                                                                                                                \
  lrbms3_ctx *ctx, int32_t Q, int32_t N, int32_t K, int32_t nmu, int32_t nt, double dt, const double *theta, const double *coef,        \
      const double *U, const double *B_sys, const double *M_red, const double *G_nc, const double *G_bb, const double *G_rdd,           \
      const double *G_ab, const double *G_aa, const double *r_fd, const double *Rb, const double *Yb, const double *Dp,                 \
      const double *Xab, const double *As, const double *Cn, const double *ebar, const double *Bbb, const double *bdiv,                 \
      const double *f2, const double *ceps, double hdiam, const double *phi, const double *F2, const double *r_fd_K,                    \
      const double *bdiv_K, double *work, double *eta_loc, double *time_deriv_nc, double *time_residual, double *eta, double *est,      \
      void *stream
#define LRBMS3_PE_ARGS                                                                                                                  \
  ctx, Q, N, K, nmu, nt, dt, theta, coef, U, B_sys, M_red, G_nc, G_bb, G_rdd, G_ab, G_aa, r_fd, Rb, Yb, Dp, Xab, As, Cn, ebar, Bbb, bdiv, \
      f2, ceps, hdiam, phi, F2, r_fd_K, bdiv_K, work, eta_loc, time_deriv_nc, time_residual, eta, est, stream

// The driver of lrbms3_reduced_parabolic_estimate_batch (tv == false: theta [nmu][Q], coef [nmu][2]) and of its _tv twin (tv == true:
// theta_t [nmu][nt+1][Q], coef [nmu][nt+1][2]): the elliptic rows and the source terms of U[k] use row k, as does
// coef in eta[k]; the time residual of U[k+1] - U[k] uses row k + 1 (the operator that produced U[k+1]); the nc form of the
// differences reads no theta.
int pe_batch3_drive(const char* name, bool tv, LRBMS3_PE_PARAMS) {
  LRBMS_REQUIRE_MESH(ctx);
  const T3& t = ctx->t;
  if (t.S_ext != t.S) return lrbms_fail(ctx, LRBMS_E_INVALID, std::string(name) + ": needs all subdomains on this rank");
  if (Q < 1 || Q > 8 || N < 1 || N > 32 || Q * N > 64 || nmu < 1 || nmu > 64 || K < 0 || K > 64)
    return lrbms_fail(ctx, LRBMS_E_INVALID, std::string(name) + ": needs N <= 32, Q N <= 64, 1 <= nmu <= 64 and 0 <= K <= 64");
  if (!(dt > 0.0) || nt < 1) return lrbms_fail(ctx, LRBMS_E_INVALID, std::string(name) + ": dt > 0 and nt >= 1 required");
  if (!theta || !coef || !U || !B_sys || !M_red || !G_nc || !G_bb || !G_rdd || !G_ab || !G_aa || !r_fd || !Rb || !Yb || !Dp || !Xab || !As ||
      !Cn || !ebar || !Bbb || !bdiv || !f2 || !ceps || !work || !eta_loc || !time_deriv_nc || !time_residual || !eta || !est)
    return lrbms_fail(ctx, LRBMS_E_INVALID, std::string(name) + ": null argument");
  const int nsrc = (phi != nullptr) + (F2 != nullptr) + (r_fd_K != nullptr) + (bdiv_K != nullptr);
  if (nsrc != (K > 0 ? 4 : 0))
    return lrbms_fail(ctx, LRBMS_E_INVALID, std::string(name) + ": phi, F2, r_fd_K, bdiv_K are all set with K >= 1 and all null with K = 0");
  if (estimate_batch_form(ctx, Q, N) == 0 || (K > 0 && !source_terms_fits(ctx, N)))
    return lrbms_fail(ctx, LRBMS_E_INVALID, std::string(name) + ": template too large for the LDS");
  hipStream_t st = (hipStream_t)stream;
  const long S = t.S, SM = S * nmu, slab = S * N * nmu, NN = (long)N * N;
  double* raw = work;
  double* dU = raw + (nt + 1) * 3 * SM;
  double* ncd = dU + nt * slab;
  double* tr2 = ncd + nt * 3 * SM;
  double* src = tr2 + nt * SM;
  double* thd = src + (nt + 1) * SM;
  double* phid = thd + 64 * 8;
  double* Minv = phid + (long)(nt + 1) * nmu * 64;
  double* Mslot = Minv + S * NN;
  double* gw = Mslot + 7 * S * NN;
  double* thd_t = work + pe_batch3_work_size(S, N, nmu, nt);      // tv only: theta rows [nt+1][nmu][Q], then coef [nmu][nt+1][2]
  double* coef_t = thd_t + (long)(nt + 1) * nmu * 8;
  const ThetaRows tr{theta, Q, tv ? nt + 1 : 0};
  std::vector<double> th_row((size_t)nmu * Q);                    // tv: row k of every column, contiguous
  auto row_of = [&](int k) {
    if (!tv) return theta;
    for (int m = 0; m < nmu; ++m)
      for (int q = 0; q < Q; ++q) th_row[(size_t)m * Q + q] = tr.at(m, k, q);
    return (const double*)th_row.data();
  };
  EA a{U, G_nc, G_bb, G_rdd, G_ab, G_aa, r_fd, Rb, Yb, Dp, Xab, As, Cn, ebar, Bbb, bdiv, f2, ceps, hdiam, raw};
  // ---- 1. the elliptic rows of every slab
  for (int k = 0; k <= nt; ++k) {
    a.u = U + k * slab;
    a.eta = raw + k * 3 * SM;
    if (int rc = launch_reduced_estimate_batch(ctx, st, Q, N, nmu, row_of(k), a)) return rc;
  }
  // ---- 2. the differences
  {
    const long total = nt * slab, blocks = (total + 255) / 256;
    hipLaunchKernelGGL(k3pe_diff, dim3((unsigned)(blocks > 8192 ? 8192 : blocks)), dim3(256), 0, st, total, U, dU, slab);
  }
  // ---- 3. their nc form: the nc-only matrix-core kernel, or row 0 of the full estimate where that form is not the one in use
  const bool nc16 = estimate_batch_form(ctx, Q, N) == 16 && estimate_nc16_fits(ctx, N);
  const double* th_nc = row_of(0);                               // (row 0 of the full estimate reads no theta)
  for (int k = 0; k < nt; ++k) {
    a.u = dU + k * slab;
    a.eta = ncd + k * 3 * SM;
    if (int rc = nc16 ? launch_estimate_nc_batch(ctx, st, N, nmu, a) : launch_reduced_estimate_batch(ctx, st, Q, N, nmu, th_nc, a)) return rc;
  }
  // ---- 4. the time residual: M_red^-1 once (the block inverse reads the self slot of a 7-slot operator, with its identity rule on
  // zero-padded basis columns), then per step and group y = sum_q theta_qm B_q dU by the panel matvec and y^T M_red^-1 y
  LRBMS_HIP_CHECK(ctx, hipMemcpy2DAsync(Mslot + 3 * NN, sizeof(double) * 7 * NN, M_red, sizeof(double) * NN, sizeof(double) * NN, S,
                                        hipMemcpyDeviceToDevice, st));
  hipLaunchKernelGGL(k3_block_inverse, dim3(S), dim3(256), sizeof(double) * N * (2 * N + 1), st, N, Mslot, Minv);
  const CoarseB none{nullptr, nullptr, nullptr};
  const long rows = S * N;
  for (int m0 = 0; m0 < nmu; m0 += 16) {
    RbGroup G{};
    G.m0 = m0;
    G.nm = nmu - m0 < 16 ? nmu - m0 : 16;
    G.st = st;
    G.z = gw;
    G.po = gw;                         // (first = 1: not read)
    G.pn = gw + rows * 16;
    G.Ap = G.pn + rows * 16;
    G.ppap = G.Ap + rows * 16;
    G.th = TB{};
    auto fill = [&](int row) {
      for (int m = 0; m < G.nm; ++m)
        for (int q = 0; q < Q; ++q) G.th.v[m][q] = tr.at(m0 + m, row, q);
    };
    fill(0);
    if (K > 0 && !tv) hipLaunchKernelGGL(k3pe_tables, dim3(1), dim3(256), 0, st, Q, K, nmu, nt, m0, G.nm, G.th, phi, thd, phid);
    if (K > 0 && tv) hipLaunchKernelGGL(k3pe_tables_tv, dim3(1), dim3(256), 0, st, Q, K, nmu, nt, 0, m0, G.nm, G.th, phi, thd_t, phid);
    const RbOp op{Q, N, nmu, B_sys, nullptr, nullptr, nullptr};
    const long vec = rows * G.nm;
    for (int k = 0; k < nt; ++k) {
      if (tv) {                        // the operator that produced U[k + 1]: row k + 1, for the matvec and for the source terms of U[k + 1]
        fill(k + 1);
        if (K > 0) hipLaunchKernelGGL(k3pe_tables_tv, dim3(1), dim3(256), 0, st, Q, K, nmu, nt, k + 1, m0, G.nm, G.th, phi, thd_t, phid);
      }
      hipLaunchKernelGGL(k3b_gather, dim3((unsigned)((vec + 255) / 256 > 4096 ? 4096 : (vec + 255) / 256)), dim3(256), 0, st, rows, G.nm, nmu,
                         dU + k * slab + m0, G.z);
      launch_matvec3<false>(ctx, op, G, 1, G.ppap, G.ppap, none);
      hipLaunchKernelGGL(k3pe_inv_norm2_panel, dim3(S), dim3(256), 0, st, N, G.nm, nmu, Minv, G.Ap, tr2 + k * SM + m0);
    }
  }
  // ---- 5. the f terms of the r rows (K >= 1: the caller's f2, r_fd and bdiv are zero)
  if (K > 0)
    for (int k = 0; k <= nt; ++k)
      launch_source_terms(st, t, Q, N, K, nmu, tv ? thd_t + (long)k * nmu * Q : thd, phid + (long)k * nmu * K, F2, r_fd_K, bdiv_K, Rb,
                          U + k * slab, ceps, hdiam, src + k * SM);
  // ---- 6. the five outputs
  if (!tv) {
    PeCoef cf{};
    for (int m = 0; m < nmu; ++m) cf.v[m][0] = coef[m * 2], cf.v[m][1] = coef[m * 2 + 1];
    hipLaunchKernelGGL(k3pe_combine, dim3((nmu + 15) / 16), dim3(256), 0, st, (int)S, nmu, nt, dt, cf, raw, K > 0 ? src : nullptr, ncd, tr2,
                       eta_loc, time_deriv_nc, time_residual, eta, est);
  } else {                             // coef [nmu][nt+1][2] has no bound in nt: into the work array in chunks, in stream order
    const long nc = (long)nmu * (nt + 1) * 2;
    for (long c0 = 0; c0 < nc; c0 += 256) {
      PeChunk c;
      const int n = nc - c0 < 256 ? (int)(nc - c0) : 256;
      for (int i = 0; i < 256; ++i) c.v[i] = i < n ? coef[c0 + i] : 0.0;
      hipLaunchKernelGGL(k3pe_put, dim3(1), dim3(256), 0, st, n, c, coef_t + c0);
    }
    hipLaunchKernelGGL(k3pe_combine_tv, dim3((nmu + 15) / 16), dim3(256), 0, st, (int)S, nmu, nt, dt, coef_t, raw, K > 0 ? src : nullptr, ncd,
                       tr2, eta_loc, time_deriv_nc, time_residual, eta, est);
  }
  LRBMS_LAUNCH_CHECK(ctx);
  return LRBMS_OK;
}

}  // namespace

extern "C" {

int lrbms3_reduced_parabolic_estimate_batch(LRBMS3_PE_PARAMS) {
  return pe_batch3_drive("reduced_parabolic_estimate_batch", false, LRBMS3_PE_ARGS);
}

// theta = theta_t [nmu][nt+1][Q], coef [nmu][nt+1][2] (host); work: lrbms3_reduced_parabolic_estimate_batch_tv_work_size doubles
int lrbms3_reduced_parabolic_estimate_batch_tv(LRBMS3_PE_PARAMS) {
  return pe_batch3_drive("reduced_parabolic_estimate_batch_tv", true, LRBMS3_PE_ARGS);
}
#undef LRBMS3_PE_ARGS
#undef LRBMS3_PE_PARAMS

}  // extern "C"
