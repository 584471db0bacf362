// Full-order solve (SURVEY.md section 8f "next" #2: snapshot generation).
//
// Reference: DuneDiscretization._solve (discretize_elliptic_block_swipdg.py:219-225) hands the assembled global matrix
// to ISTL (bicgstab.ilut, python/scripts/online_adaptive_lrbms.py:71).  Here the block operator is never assembled:
// the matvec works on the block-ELL data of the discretization (A_diag: diagonal blocks of every subdomain, A_cpl:
// coupling blocks on the side faces) and the solver is a preconditioned CG -- the SWIPDG operator is symmetric positive
// definite -- with the 3x3 element blocks as block-Jacobi preconditioner.  Per iteration: two launches
//   k_fom_cg_matvec   beta = rz' / rz, p = z + beta p (own and neighbouring elements, on the fly), y = A(mu) p, partial p.y
//   k_fom_cg_update   alpha = rz / pAp, x += alpha p, r -= alpha y, z = M^-1 r, partial r.z and r.r
// A dependent kernel costs ~6 us on this part whatever it does, so the scalar reductions are no kernels of their own:
// every workgroup sums the per-workgroup partials of the previous kernel itself (a few KB from L2, the same fixed
// order everywhere, so every workgroup gets the same bits; 4 launches per iteration: 31.8 us, 2 launches: see DESIGN.md).
// The host looks at |r| where the observed convergence rate predicts the tolerance, at most 100 iterations apart.
// The theta-weighted blocks are combined once per solve.
//
// Batched snapshots (lrbms_fom_solve_batch): up to 64 parameters per call in panels of 16 columns.
// The panel kernels k_fomb_* further down read the Q uncombined blocks once per iteration for all 16 columns and weight
// them per lane with the column's own theta; the kernels above are untouched by it.
//
// Batched trajectories (lrbms_fom_implicit_euler_batch): the same panels on the step operator
// M + dt A(theta_m) of the implicit Euler (the _mass instantiations of the two panel kernels), every step of a panel a
// warm-started PCG relative to the step's full right-hand side.
#include <type_traits>
#include "lrbms_dev.h"

namespace {

struct QVecF { double v[8]; };

// sum over the 64 lanes of a wave, returned to every lane: DPP moves inside the rows of 16 lanes, then the four row sums
// through scalar registers (fixed order; no LDS crossbar traffic as with __shfl_xor)
__device__ inline double wave_sum_dpp(double v) {
  auto dpp = [](double x, auto ctrl_c) {
    constexpr int CTRL = decltype(ctrl_c)::value;
    int lo = __double2loint(x), hi = __double2hiint(x);
    lo = __builtin_amdgcn_update_dpp(lo, lo, CTRL, 0xF, 0xF, true);
    hi = __builtin_amdgcn_update_dpp(hi, hi, CTRL, 0xF, 0xF, true);
    return __hiloint2double(hi, lo);
  };
  v += dpp(v, std::integral_constant<int, 0xB1>{});    // quad_perm [1,0,3,2]
  v += dpp(v, std::integral_constant<int, 0x4E>{});    // quad_perm [2,3,0,1]
  v += dpp(v, std::integral_constant<int, 0x141>{});   // row_half_mirror
  v += dpp(v, std::integral_constant<int, 0x140>{});   // row_mirror
  double rows[4];
#pragma unroll
  for (int k = 0; k < 4; ++k)
    rows[k] = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), 16 * k), __builtin_amdgcn_readlane(__double2loint(v), 16 * k));
  return (rows[0] + rows[1]) + (rows[2] + rows[3]);
}

__device__ inline double block_sum_256(double v, double* red) {
  const int tid = threadIdx.x;
  red[tid] = v;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off) red[tid] += red[tid + off];
    __syncthreads();
  }
  const double out = red[0];
  __syncthreads();
  return out;
}

// sums of a[0..na) and b[0..nb) by a 256-thread workgroup: thread-strided partial sums (all loads of a 2048-entry chunk
// issued before the first add: a plain `acc += a[i]` loop waits one L2 round trip per entry), then one fixed-order tree
// for both (same bits in every workgroup).  red: 512 doubles.
__device__ inline void block_sum_arrays_256(const double* __restrict__ a, int na, const double* __restrict__ b, int nb, double* red,
                                            double& sa, double& sb) {
  const int tid = threadIdx.x;
  double acc_a = 0.0, acc_b = 0.0;
  const int n = na > nb ? na : nb;
  for (int base = 0; base < n; base += 2048) {
    double va[8], vb[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int i = base + tid + 256 * k;
      va[k] = i < na ? a[i] : 0.0;
      vb[k] = i < nb ? b[i] : 0.0;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      acc_a += va[k];
      acc_b += vb[k];
    }
  }
  red[tid] = acc_a;
  red[256 + tid] = acc_b;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off) {
      red[tid] += red[tid + off];
      red[256 + tid] += red[256 + tid + off];
    }
    __syncthreads();
  }
  sa = red[0];
  sb = red[256];
  __syncthreads();
}

// Amu_d [S][nT][4][9] = sum_q theta_q A_diag_q (+ mass * |T|/12 (1 + delta_ij) on the diagonal block),
// Amu_c [S][4][ncf][9] = sum_q theta_q A_cpl_q, Minv [S][nT][9] = inverse of the diagonal 3x3 block
__global__ __launch_bounds__(256) void k_fom_combine(Tmpl t, int S, int Q, QVecF th, double mass, const double* __restrict__ A_diag,
                                                     const double* __restrict__ A_cpl, double* __restrict__ Amu_d,
                                                     double* __restrict__ Amu_c, double* __restrict__ Minv) {
  const long nd = (long)S * t.nT * 36, nc = (long)S * 4 * t.ncf * 9;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nd + nc; i += (long)gridDim.x * blockDim.x) {
    double acc = 0.0;
    if (i < nd) {
      for (int q = 0; q < Q; ++q) acc += th.v[q] * A_diag[(long)q * nd + i];
      const int k = (int)(i % 36);
      if (mass != 0.0 && k < 9) acc += mass * t.area[(i / 36) % t.nT] / 12.0 * (k % 4 == 0 ? 2.0 : 1.0);
      Amu_d[i] = acc;
    } else {
      for (int q = 0; q < Q; ++q) acc += th.v[q] * A_cpl[(long)q * nc + (i - nd)];
      Amu_c[i - nd] = acc;
    }
  }
  const long ne = (long)S * t.nT;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < ne; e += (long)gridDim.x * blockDim.x) {
    double a[9];
    for (int k = 0; k < 9; ++k) {
      a[k] = 0.0;
      for (int q = 0; q < Q; ++q) a[k] += th.v[q] * A_diag[(long)q * nd + e * 36 + k];
      if (mass != 0.0) a[k] += mass * t.area[e % t.nT] / 12.0 * (k % 4 == 0 ? 2.0 : 1.0);
    }
    const double c0 = a[4] * a[8] - a[5] * a[7], c1 = a[5] * a[6] - a[3] * a[8], c2 = a[3] * a[7] - a[4] * a[6];
    const double id = 1.0 / (a[0] * c0 + a[1] * c1 + a[2] * c2);
    double* o = Minv + e * 9;
    o[0] = c0 * id;
    o[1] = (a[2] * a[7] - a[1] * a[8]) * id;
    o[2] = (a[1] * a[5] - a[2] * a[4]) * id;
    o[3] = c1 * id;
    o[4] = (a[0] * a[8] - a[2] * a[6]) * id;
    o[5] = (a[2] * a[3] - a[0] * a[5]) * id;
    o[6] = c2 * id;
    o[7] = (a[1] * a[6] - a[0] * a[7]) * id;
    o[8] = (a[0] * a[4] - a[1] * a[3]) * id;
  }
}

// Four lanes per (subdomain, element): lane b applies block b of the element's block row (its own 3x3 block and the
// three face neighbours'), so a wave reads 16 x 288 contiguous bytes of the block-ELL data; the three row sums are
// combined by two butterflies.  beta = rz_new / rz_old from the partials prz_new / prz_old [npart] (first: 0).
// 64 elements per workgroup; partial[blockIdx.x] = sum over its elements of p . y.
__global__ __launch_bounds__(256) void k_fom_cg_matvec(Tmpl t, int S, const int* __restrict__ nbr, const double* __restrict__ Amu_d,
                                                       const double* __restrict__ Amu_c, const double* __restrict__ z,
                                                       const double* __restrict__ p_old, const double* __restrict__ prz_new,
                                                       const double* __restrict__ prz_old, int npart, int first,
                                                       const double* __restrict__ c0, double* __restrict__ p_new,
                                                       double* __restrict__ y, double* __restrict__ partial) {
  __shared__ double red[512];
  const long ne = (long)S * t.nT;
  const long idx = (long)blockIdx.x * 64 + (threadIdx.x >> 2);
  const int b = threadIdx.x & 3;
  // all loads first (block, neighbour values): none of them depends on beta, and the reduction below synchronises
  double blk[9], zv[3] = {0.0, 0.0, 0.0}, po[3] = {0.0, 0.0, 0.0};
  bool live = false;
#pragma unroll
  for (int k = 0; k < 9; ++k) blk[k] = 0.0;
  if (idx < ne) {
    const int e = (int)(idx % t.nT), s = (int)(idx / t.nT);
    int e2 = e, s2 = s;
    const double* bp = Amu_d + idx * 36 + b * 9;
    if (b > 0) {
      const int nb = t.nb_elem[e * 3 + b - 1];
      if (nb >= 0) {
        e2 = nb;
      } else {
        const int side = -1 - nb;
        s2 = nbr[s * 5 + side_to_slot(side)];
        e2 = t.nb_elem_out[e * 3 + b - 1];
        bp = Amu_c + (((long)s * 4 + side) * t.ncf + t.elem_side_pos[e * 3 + b - 1]) * 9;
      }
    }
    if (s2 >= 0) {
      live = true;
      const long g = ((long)s2 * t.nT + e2) * 3;
#pragma unroll
      for (int k = 0; k < 9; ++k) blk[k] = bp[k];
      const double cz = c0 ? c0[s2] : 0.0;                // coarse part of the preconditioned residual (constant per subdomain)
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        zv[i] = z[g + i] + cz;
        if (!first) po[i] = p_old[g + i];
      }
    }
  }
  double beta = 0.0;
  if (!first) {
    double rz_new, rz_old;
    block_sum_arrays_256(prz_new, npart, prz_old, npart, red, rz_new, rz_old);
    beta = rz_old != 0.0 ? rz_new / rz_old : 0.0;
  }
  double dot = 0.0;
  if (idx < ne) {
    double acc[3] = {0.0, 0.0, 0.0}, pv[3] = {0.0, 0.0, 0.0};
    if (live) {
      for (int i = 0; i < 3; ++i) pv[i] = zv[i] + beta * po[i];
      for (int i = 0; i < 3; ++i) acc[i] = blk[i * 3] * pv[0] + blk[i * 3 + 1] * pv[1] + blk[i * 3 + 2] * pv[2];
    }
    for (int i = 0; i < 3; ++i) {
      acc[i] += __shfl_xor(acc[i], 1, 64);
      acc[i] += __shfl_xor(acc[i], 2, 64);
    }
    if (b == 0)
      for (int i = 0; i < 3; ++i) {
        p_new[idx * 3 + i] = pv[i];
        y[idx * 3 + i] = acc[i];
        dot += pv[i] * acc[i];
      }
  }
  const double sum = block_sum_256(dot, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = sum;
}

// alpha = rz / pAp from the partials prz_in [npart] / ppap [npap] (first: 0 -- only z and the partials of the start residual)
__global__ __launch_bounds__(256) void k_fom_cg_update(long ne, const double* __restrict__ Minv, const double* __restrict__ prz_in,
                                                       const double* __restrict__ ppap, int npart, int npap, int first,
                                                       double* __restrict__ x, double* __restrict__ r, const double* __restrict__ p,
                                                       const double* __restrict__ y, double* __restrict__ z,
                                                       double* __restrict__ prz_out, double* __restrict__ prr,
                                                       double* __restrict__ r0w) {
  __shared__ double red[512];
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  // all loads first: none of them depends on alpha, and the reduction below synchronises
  double xv[3] = {0.0, 0.0, 0.0}, rv[3] = {0.0, 0.0, 0.0}, pv[3] = {0.0, 0.0, 0.0}, yv[3] = {0.0, 0.0, 0.0}, M[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) M[k] = 0.0;
  if (idx < ne) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const long g = idx * 3 + i;
      rv[i] = r[g];
      if (!first) {
        xv[i] = x[g];
        pv[i] = p[g];
        yv[i] = y[g];
      }
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) M[k] = Minv[idx * 9 + k];
  }
  double alpha = 0.0;
  if (!first) {
    double rz, pap;
    block_sum_arrays_256(prz_in, npart, ppap, npap, red, rz, pap);
    alpha = pap != 0.0 ? rz / pap : 0.0;
  }
  double rz = 0.0, rr = 0.0, rsum = 0.0;
  if (idx < ne) {
    for (int i = 0; i < 3; ++i) {
      const long g = idx * 3 + i;
      if (!first) {
        x[g] = xv[i] + alpha * pv[i];
        rv[i] -= alpha * yv[i];
        r[g] = rv[i];
      }
    }
    rsum = rv[0] + rv[1] + rv[2];
    for (int i = 0; i < 3; ++i) {
      const double zi = M[i * 3] * rv[0] + M[i * 3 + 1] * rv[1] + M[i * 3 + 2] * rv[2];
      z[idx * 3 + i] = zi;
      rz += rv[i] * zi;
      rr += rv[i] * rv[i];
    }
  }
  if (r0w) {
    // restriction to the coarse space on the way: the sum of the new residual over this wave's 64 elements (waves do not
    // straddle subdomains when 64 divides the elements per subdomain); k_fom_coarse1 adds the waves of a subdomain
    const double ws = wave_sum_dpp(rsum);
    if ((threadIdx.x & 63) == 0) r0w[idx >> 6] = ws;
  }
  const double s1 = block_sum_256(rz, red);
  const double s2 = block_sum_256(rr, red);
  if (threadIdx.x == 0) {
    prz_out[blockIdx.x] = s1;
    prr[blockIdx.x] = s2;
  }
}

// implicit Euler step, warm start x = u_k:  r = M u_k + dt b - y  with y = (M + dt A) u_k;  partial = |M u_k + dt b|^2
__global__ __launch_bounds__(256) void k_fom_step_residual(Tmpl t, long ne, double dt, const double* __restrict__ uk,
                                                           const double* __restrict__ b, const double* __restrict__ y,
                                                           double* __restrict__ r, double* __restrict__ partial) {
  __shared__ double red[256];
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  double acc = 0.0;
  if (idx < ne) {
    const double m = t.area[idx % t.nT] / 12.0;
    const double u0 = uk[idx * 3], u1 = uk[idx * 3 + 1], u2 = uk[idx * 3 + 2];
    const double sum = u0 + u1 + u2;
    const double uv[3] = {u0, u1, u2};
    for (int i = 0; i < 3; ++i) {
      const double rhs = m * (sum + uv[i]) + dt * b[idx * 3 + i];
      r[idx * 3 + i] = rhs - y[idx * 3 + i];
      acc += rhs * rhs;
    }
  }
  const double s = block_sum_256(acc, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// the same with a time-dependent affine source:  r = M u_k + dt sum_j phi_j b_j - y,  b_j = bK + j nv (bK [K][S][n]),
// phi = the coefficient row of the step (device, K entries).  With K = 1 and phi = 1 the expressions are those of
// k_fom_step_residual (1.0 * b == b), so the two agree bit for bit.
__global__ __launch_bounds__(256) void k_fom_step_residual_src(Tmpl t, long ne, double dt, const double* __restrict__ uk, int K,
                                                               const double* __restrict__ phi, const double* __restrict__ bK,
                                                               const double* __restrict__ y, double* __restrict__ r,
                                                               double* __restrict__ partial) {
  __shared__ double red[256];
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long nv = ne * 3;
  double acc = 0.0;
  if (idx < ne) {
    const double m = t.area[idx % t.nT] / 12.0;
    const double u0 = uk[idx * 3], u1 = uk[idx * 3 + 1], u2 = uk[idx * 3 + 2];
    const double sum = u0 + u1 + u2;
    const double uv[3] = {u0, u1, u2};
    double bk[3] = {0.0, 0.0, 0.0};
    for (int j = 0; j < K; ++j) {
      const double pj = phi[j];
      const double* bj = bK + (long)j * nv + idx * 3;
      for (int i = 0; i < 3; ++i) bk[i] += pj * bj[i];
    }
    for (int i = 0; i < 3; ++i) {
      // the contraction k_fom_step_residual compiles to (fma of the mass term onto dt b), spelled out: the compiler would
      // otherwise fuse dt * bk instead and the two kernels would differ in the last bit
      const double dtb = dt * bk[i];
      const double rhs = __fma_rn(m, sum + uv[i], dtb);
      r[idx * 3 + i] = rhs - y[idx * 3 + i];
      acc += rhs * rhs;
    }
  }
  const double s = block_sum_256(acc, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// Coarse level (see online.hip): the span of the subdomain indicator functions.  A0[s][t] = 1^T A_st 1: the sum of all
// entries of the combined blocks between subdomains s and t.  One workgroup per subdomain.
__global__ __launch_bounds__(256) void k_fom_coarse_entries(Tmpl t, int S, const int* __restrict__ nbr, const double* __restrict__ Amu_d,
                                                            const double* __restrict__ Amu_c, double* __restrict__ A0) {
  __shared__ double red[256];
  const int s = blockIdx.x;
  double acc = 0.0;
  for (int i = threadIdx.x; i < t.nT * 4; i += 256) {
    const int e = i >> 2, b = i & 3;
    if (b > 0 && t.nb_elem[e * 3 + b - 1] < 0) continue;             // that neighbour lives in another subdomain (Amu_c)
    const double* blk = Amu_d + ((long)s * t.nT * 4 + i) * 9;
    for (int k = 0; k < 9; ++k) acc += blk[k];
  }
  const double diag = block_sum_256(acc, red);
  if (threadIdx.x == 0) A0[(long)s * S + s] = diag;
  for (int side = 0; side < 4; ++side) {
    const int s2 = nbr[s * 5 + side_to_slot(side)];
    if (s2 < 0) continue;
    double a = 0.0;
    for (int i = threadIdx.x; i < t.side_count[side] * 9; i += 256) a += Amu_c[((long)s * 4 + side) * t.ncf * 9 + i];
    const double off = block_sum_256(a, red);
    if (threadIdx.x == 0) A0[(long)s * S + s2] = off;
  }
}

// Coarse part of the preconditioned residual with the restriction folded in: r0[t] = sum of the wps wave sums of
// subdomain t (written by k_fom_cg_update), c0[s] = (A0^-1 r0)_s, prz_c[s] = r0[s] c0[s].  One wave per coarse row.
__global__ __launch_bounds__(256) void k_fom_coarse1(int S, int wps, const double* __restrict__ A0inv, const double* __restrict__ r0w,
                                                     double* __restrict__ c0, double* __restrict__ prz_c) {
  const int lane = threadIdx.x & 63, s = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (s >= S) return;
  const double* row = A0inv + (long)s * S;
  double acc = 0.0;
  for (int base = 0; base < S; base += 512) {
    double a[8], b[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int i = base + lane + 64 * k;
      a[k] = i < S ? row[i] : 0.0;
      b[k] = 0.0;
    }
    for (int w = 0; w < wps; ++w) {
      double t[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int i = base + lane + 64 * k;
        t[k] = i < S ? r0w[(long)i * wps + w] : 0.0;
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) b[k] += t[k];
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) acc += a[k] * b[k];
  }
  const double sum = wave_sum_dpp(acc);
  if (lane == 0) {
    double own = 0.0;
    for (int w = 0; w < wps; ++w) own += r0w[(long)s * wps + w];
    c0[s] = sum;
    prz_c[s] = own * sum;
  }
}

// r0[s] = sum of the residual over subdomain s (restriction to the coarse space); zeroes the coarse solution and the
// coarse part of the r.z partials, which k_coarse_apply accumulates into.  One workgroup per subdomain.
__global__ __launch_bounds__(256) void k_fom_restrict(int n, const double* __restrict__ r, double* __restrict__ r0,
                                                      double* __restrict__ c0, double* __restrict__ prz_c) {
  __shared__ double red[256];
  const int s = blockIdx.x;
  double v[8];
  double acc = 0.0;
  for (int base = 0; base < n; base += 2048) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int i = base + threadIdx.x + 256 * k;
      v[k] = i < n ? r[(long)s * n + i] : 0.0;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) acc += v[k];
  }
  const double sum = block_sum_256(acc, red);
  if (threadIdx.x == 0) {
    r0[s] = sum;
    c0[s] = 0.0;
    prz_c[s] = 0.0;
  }
}

}  // namespace

int64_t fom_solve_work_size(lrbms_ctx* ctx) {
  const Tmpl& t = ctx->t;
  const int64_t S = ctx->S, ne = S * t.nT;
  const int64_t nblk = (ne + 255) / 256, nmv = (ne + 63) / 64;
  return ne * 36 + S * 4 * t.ncf * 9 + ne * 9 + 5 * ne * 3 + 3 * nblk + 2 * nmv + 4 * S + 16;
}

namespace {

struct FomCg {
  double *Amu_d, *Amu_c, *Minv, *r, *z, *p[2], *y, *prz[2], *ppap, *prr, *r0, *c0, *r0w;
  int wps = 0;        // waves per subdomain of the update kernel if 64 divides the elements per subdomain (fused restriction), else 0
  const double* A0inv = nullptr;   // coarse level, or nullptr
  long ne, nv;
  int nblk, nmv;      // workgroups (= partial sums) of the update kernel (256 elements each) / the matvec kernel (64 each)
  void carve(lrbms_ctx* ctx, double* work) {
    const Tmpl& t = ctx->t;
    const long S = ctx->S;
    ne = S * t.nT;
    nv = ne * 3;
    nblk = (int)((ne + 255) / 256);
    nmv = (int)((ne + 63) / 64);
    Amu_d = work;
    Amu_c = Amu_d + ne * 36;
    Minv = Amu_c + S * 4 * t.ncf * 9;
    r = Minv + ne * 9;
    z = r + nv;
    p[0] = z + nv;
    p[1] = p[0] + nv;
    y = p[1] + nv;
    prz[0] = y + nv;              // [nblk + S]: r.z partials of the update kernel, then the coarse parts per subdomain
    prz[1] = prz[0] + nblk + S;
    prr = prz[1] + nblk + S;
    ppap = prr + nblk;   // [nmv]
    r0 = ppap + nmv;
    c0 = r0 + S;
    r0w = c0 + S;                 // [nmv] residual sums per wave of the update kernel (ends at fom_solve_work_size - 16)
    wps = t.nT % 64 == 0 ? t.nT / 64 : 0;
  }
};

int fom_host_sum(lrbms_ctx* ctx, const double* dev, std::vector<double>& host, double* out, hipStream_t st) {
  LRBMS_HIP_CHECK(ctx, hipMemcpyAsync(host.data(), dev, sizeof(double) * host.size(), hipMemcpyDeviceToHost, st));
  LRBMS_HIP_CHECK(ctx, hipStreamSynchronize(st));
  double acc = 0.0;
  for (double v : host) acc += v;
  *out = acc;
  return LRBMS_OK;
}

// PCG on the combined operator: on entry x holds the start value and b.r the start residual; iterates until
// |r| <= rtol * sqrt(ref2) (ref2 < 0: relative to the start residual).
// the coarse part of z = M^-1 r for the residual just written by k_fom_cg_update: restriction, dense coarse solve
// (k_coarse_apply of online.hip with one column and one unknown per subdomain); c0 is added to z by the next matvec
int fom_coarse_step(lrbms_ctx* ctx, FomCg& b, double* prz, hipStream_t st) {
  if (!b.A0inv) return LRBMS_OK;
  if (b.wps) {                                           // the update kernel left the residual sums per wave
    hipLaunchKernelGGL(k_fom_coarse1, dim3((ctx->S + 3) / 4), dim3(256), 0, st, ctx->S, b.wps, b.A0inv, b.r0w, b.c0, prz + b.nblk);
    LRBMS_LAUNCH_CHECK(ctx);
    return LRBMS_OK;
  }
  hipLaunchKernelGGL(k_fom_restrict, dim3(ctx->S), dim3(256), 0, st, ctx->t.n, b.r, b.r0, b.c0, prz + b.nblk);
  LRBMS_LAUNCH_CHECK(ctx);
  return launch_coarse_apply(ctx, 1, 1, b.A0inv, b.r0, b.c0, prz + b.nblk, st);
}

// Builds the coarse level for the combined blocks of `b` (b.A0inv stays nullptr if it is not available)
int fom_coarse_setup(lrbms_ctx* ctx, FomCg& b, hipStream_t st) {
  b.A0inv = nullptr;
  LRBMS_HIP_CHECK(ctx, hipMemsetAsync(b.prz[0], 0, sizeof(double) * 2 * (b.nblk + ctx->S), st));
  double* A0 = nullptr;
  if (int rc = coarse_begin(ctx, &A0, st)) return rc;
  if (!A0) return LRBMS_OK;
  hipLaunchKernelGGL(k_fom_coarse_entries, dim3(ctx->S), dim3(256), 0, st, ctx->t, ctx->S, ctx->nbr, b.Amu_d, b.Amu_c, A0);
  LRBMS_LAUNCH_CHECK(ctx);
  return coarse_finish(ctx, &b.A0inv, st);
}

// PCG on the combined operator: on entry x holds the start value and b.r the start residual; iterates until
// |r| <= rtol * sqrt(ref2) (ref2 < 0: relative to the start residual).  Preconditioner: inverse 3x3 element blocks plus
// the coarse level on the subdomain indicator functions (element-block Jacobi alone needs 3 800 iterations at config 3,
// doubling with the number of subdomains per direction; with the coarse level ~450).
int fom_cg_run(lrbms_ctx* ctx, FomCg& b, double* x, double ref2, double rtol, int max_iter, int* its, double* rel_out, hipStream_t st) {
  const Tmpl& t = ctx->t;
  const int S = ctx->S, nblk = b.nblk;
  const int npart = b.A0inv ? nblk + S : nblk;          // r.z partials: per update workgroup (+ the coarse parts per subdomain)
  const double* c0 = b.A0inv ? b.c0 : nullptr;
  std::vector<double> host(nblk);
  hipLaunchKernelGGL(k_fom_cg_update, dim3(nblk), dim3(256), 0, st, b.ne, b.Minv, b.prz[0], b.ppap, npart, b.nmv, 1, x, b.r, b.p[0], b.y, b.z,
                     b.prz[0], b.prr, b.A0inv && b.wps ? b.r0w : nullptr);
  LRBMS_LAUNCH_CHECK(ctx);
  if (int rc = fom_coarse_step(ctx, b, b.prz[0], st)) return rc;
  double rr = 0.0;
  if (int rc = fom_host_sum(ctx, b.prr, host, &rr, st)) return rc;
  if (ref2 < 0.0) ref2 = rr;
  *its = 0;
  *rel_out = 0.0;
  if (rr == 0.0 || ref2 == 0.0) return LRBMS_OK;
  double rel = sqrt(rr / ref2);
  int it = 0, block = 10;
  while (rel > rtol && it < max_iter) {
    if (block > max_iter - it) block = max_iter - it;
    for (int k = 0; k < block; ++k, ++it) {
      const int c = it & 1, o = c ^ 1;
      hipLaunchKernelGGL(k_fom_cg_matvec, dim3(b.nmv), dim3(256), 0, st, t, S, ctx->nbr, b.Amu_d, b.Amu_c, b.z, b.p[o], b.prz[c], b.prz[o],
                         npart, it == 0 ? 1 : 0, c0, b.p[c], b.y, b.ppap);
      hipLaunchKernelGGL(k_fom_cg_update, dim3(nblk), dim3(256), 0, st, b.ne, b.Minv, b.prz[c], b.ppap, npart, b.nmv, 0, x, b.r, b.p[c], b.y, b.z,
                         b.prz[o], b.prr, b.A0inv && b.wps ? b.r0w : nullptr);
      if (int rc = fom_coarse_step(ctx, b, b.prz[o], st)) return rc;
    }
    LRBMS_LAUNCH_CHECK(ctx);
    if (int rc = fom_host_sum(ctx, b.prr, host, &rr, st)) return rc;
    rel = sqrt(rr / ref2);
    if (!(rel == rel)) return lrbms_fail(ctx, LRBMS_E_NOT_CONVERGED, "fom CG: NaN residual (operator not SPD?)");
    const double rate = log(rel) / it;
    block = 25;
    if (rel > rtol && rate < 0.0) {                     // aim a little short: CG converges superlinearly
      const double need = 0.8 * (log(rtol) - log(rel)) / rate;
      block = need < 4.0 ? 4 : need > 100.0 ? 100 : (int)need;
    }
  }
  *its = it;
  *rel_out = rel;
  return LRBMS_OK;
}

}  // namespace

int launch_fom_solve(lrbms_ctx* ctx, int Q, const double* theta, const double* A_diag, const double* A_cpl, const double* b,
                     double* work, double* x, double rtol, int max_iter, double* info, hipStream_t st) {
  if (ctx->S_ext != ctx->S) return lrbms_fail(ctx, LRBMS_E_INVALID, "fom_solve needs all subdomains on one rank");
  if (Q < 1 || Q > 8 || max_iter < 1 || !(rtol > 0.0)) return lrbms_fail(ctx, LRBMS_E_INVALID, "fom_solve: bad Q / max_iter / rtol");
  QVecF th;
  for (int q = 0; q < 8; ++q) th.v[q] = q < Q ? theta[q] : 0.0;
  FomCg c;
  c.carve(ctx, work);
  hipLaunchKernelGGL(k_fom_combine, dim3(4096), dim3(256), 0, st, ctx->t, ctx->S, Q, th, 0.0, A_diag, A_cpl, c.Amu_d, c.Amu_c, c.Minv);
  LRBMS_LAUNCH_CHECK(ctx);
  if (int rc = fom_coarse_setup(ctx, c, st)) return rc;
  LRBMS_HIP_CHECK(ctx, hipMemsetAsync(x, 0, sizeof(double) * c.nv, st));
  LRBMS_HIP_CHECK(ctx, hipMemcpyAsync(c.r, b, sizeof(double) * c.nv, hipMemcpyDeviceToDevice, st));
  int it = 0;
  double rel = 0.0;
  if (int rc = fom_cg_run(ctx, c, x, -1.0, rtol, max_iter, &it, &rel, st)) return rc;
  if (info) { info[0] = it; info[1] = rel; }
  if (rel > rtol) return lrbms_fail(ctx, LRBMS_E_NOT_CONVERGED, "fom_solve: CG did not reach rtol");
  return LRBMS_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// Batched snapshots (lrbms_fom_solve_batch): up to 64 parameters per call, solved in panels of 16 columns.  Column m solves
// (sum_q theta[m][q] A_q) x_m = sum_j phi[m][j] b_K[j] from x = 0; the panel vectors r, z, p, y are [S n][16] (column
// fastest: the 16 lanes of a column group read 128 contiguous bytes), x lives in the caller's X [S][n][nmu].
// No combined operator per column: the kernels read the Q uncombined blocks once per iteration and weight them per lane
// with the column's own theta (the panel's table travels as a kernel argument).  Per iteration
//   k_fomb_matvec    lane = (column, block of the element's block row), one wave per element:  beta = rz' / rz,
//                    p = z + c0 + beta p, y = A(theta_m) p, partial p.y per workgroup and column
//   k_fomb_update    lane = (column, element of four):  alpha = rz / pAp, x += alpha p, r -= alpha y, z = D(theta_m)^-1 r
//                    with the 3x3 diagonal block combined and inverted on the fly, partial r.z and r.r
//   k_fomb_restrict + k_coarse_apply (coarse level only): r0 = R0 r per column, c0 = A0^-1 r0, coarse part of r.z
//   k_fomb_scalars   rz per column = the update kernel's partials + the coarse parts (one workgroup per column)
// Workgroups of 1024 threads loop over the elements, at most 256 of them: a kernel leaves <= 256 x 16 partials, which the
// next kernel's workgroups re-sum themselves (p.y: 4 loads per thread).  The r.z sum also has S coarse parts per column
// (16 S values); re-summing those in every workgroup of two kernels would cost more than the one small dependent launch of
// k_fomb_scalars.  Every sum runs in a fixed order and nothing is accumulated with atomics: repeat calls give the same bits.
// One coarse level per call, built at the mean theta of the call's columns with the kernels of lrbms_fom_solve.
namespace {

struct ThetaP { double v[16][8]; };                  // theta of the panel's columns (1 KB of kernel arguments)

constexpr int FOMB_THREADS = 1024, FOMB_GRID_MAX = 256;

// sum over the G rows of part [G][16] in column (threadIdx.x & 15), returned to every thread of a 1024-thread workgroup
// (64 row groups, then one fixed-order tree: the same bits in every workgroup).  red: 1024 doubles.
__device__ inline double fomb_colsum(const double* __restrict__ part, int G, double* red) {
  const int tid = threadIdx.x, c = tid & 15, j = tid >> 4;
  double acc = 0.0;
  for (int base = 0; base < G; base += 256) {
    double v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int row = base + j + 64 * k;
      v[k] = row < G ? part[(long)row * 16 + c] : 0.0;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) acc += v[k];
  }
  red[tid] = acc;
  __syncthreads();
  for (int off = 512; off >= 16; off >>= 1) {
    if (tid < off) red[tid] += red[tid + off];
    __syncthreads();
  }
  const double out = red[c];
  __syncthreads();
  return out;
}

// the per-wave sums v (lanes 0..15: one per column) of the 16 waves of a workgroup -> out[blockIdx.x][16]; red: 256 doubles
__device__ inline void fomb_store_partial(double v, double* red, double* __restrict__ out) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (lane < 16) red[wave * 16 + lane] = v;
  __syncthreads();
  if (tid < 16) {
    double acc = 0.0;
#pragma unroll
    for (int w = 0; w < 16; ++w) acc += red[w * 16 + tid];
    out[(long)blockIdx.x * 16 + tid] = acc;
  }
  __syncthreads();
}

// r [S n][16] = sum_j phi[m0 + c][j] b_K[j] (fma from the first product: K = 1, phi = 1 gives the bits of b), columns
// c >= P zero;  X[.][m0 + c] = 0
__global__ __launch_bounds__(256) void k_fomb_rhs(long nv, int K, int P, int nmu, int m0, const double* __restrict__ phi,
                                                  const double* __restrict__ bK, double* __restrict__ r, double* __restrict__ X) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nv * 16; i += (long)gridDim.x * blockDim.x) {
    const long g = i >> 4;
    const int c = (int)(i & 15);
    double acc = 0.0;
    if (c < P) {
      const double* ph = phi + (long)(m0 + c) * K;
      acc = ph[0] * bK[g];
      for (int j = 1; j < K; ++j) acc = __fma_rn(ph[j], bK[(long)j * nv + g], acc);
      X[g * nmu + m0 + c] = 0.0;
    }
    r[i] = acc;
  }
}

// One wave per element: lane = (column c = lane & 15, block b = lane >> 4 of the element's block row: its own 3x3 block and
// the three face neighbours').  The 16 lanes of a block share the loads of the Q uncombined blocks and weight them with
// their own theta; the three row sums meet by two butterflies across the blocks.  rz_new / rz_old [16]: r.z per column
// (k_fomb_scalars).  partial [gridDim.x][16] = p . y over the workgroup's elements.
// MASS: the step operator of the implicit Euler, M + A(theta) with theta pre-multiplied by dt: the P1 mass |T|/12 (1 + delta_ij)
// (the expression of k_fom_combine) joins the element's own 3x3 block on the b == 0 lanes.
template <bool MASS>
__device__ __forceinline__ void fomb_matvec_body(const Tmpl& t, int S, int Q, int P, const ThetaP& th, const int* __restrict__ nbr,
                                                 const double* __restrict__ A_diag, const double* __restrict__ A_cpl,
                                                 const double* __restrict__ z, const double* __restrict__ p_old,
                                                 const double* __restrict__ rz_new, const double* __restrict__ rz_old, int first,
                                                 const double* __restrict__ c0, double* __restrict__ p_new,
                                                 double* __restrict__ y, double* __restrict__ partial, double* red) {
  const long ne = (long)S * t.nT, nd = ne * 36, nc = (long)S * 4 * t.ncf * 9;
  const int lane = threadIdx.x & 63, c = lane & 15, b = lane >> 4, wave = threadIdx.x >> 6;
  const bool on = c < P;
  double thq[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) thq[q] = q < Q ? th.v[c][q] : 0.0;
  double beta = 0.0;
  if (!first) {
    const double rn = rz_new[c], ro = rz_old[c];
    beta = ro != 0.0 ? rn / ro : 0.0;
  }
  double dot = 0.0;
  for (long idx = (long)blockIdx.x * 16 + wave; idx < ne; idx += (long)gridDim.x * 16) {
    const int e = (int)(idx % t.nT), s = (int)(idx / t.nT);
    int e2 = e, s2 = s;
    const double* bp = A_diag + idx * 36 + b * 9;
    long qs = nd;
    if (b > 0) {
      const int nb = t.nb_elem[e * 3 + b - 1];
      if (nb >= 0) {
        e2 = nb;
      } else {
        const int side = -1 - nb;
        s2 = nbr[s * 5 + side_to_slot(side)];
        e2 = t.nb_elem_out[e * 3 + b - 1];
        bp = A_cpl + (((long)s * 4 + side) * t.ncf + t.elem_side_pos[e * 3 + b - 1]) * 9;
        qs = nc;
      }
    }
    double acc[3] = {0.0, 0.0, 0.0}, pv[3] = {0.0, 0.0, 0.0};
    if (s2 >= 0 && on) {
      double blk[9];
#pragma unroll
      for (int k = 0; k < 9; ++k) blk[k] = 0.0;
#pragma unroll
      for (int q = 0; q < 8; ++q)
        if (q < Q) {
#pragma unroll
          for (int k = 0; k < 9; ++k) blk[k] += thq[q] * bp[q * qs + k];
        }
      if (MASS && b == 0) {
        const double ma = t.area[e];
#pragma unroll
        for (int k = 0; k < 9; ++k) blk[k] += ma / 12.0 * (k % 4 == 0 ? 2.0 : 1.0);
      }
      const long g = ((long)s2 * t.nT + e2) * 3;
      const double cz = c0 ? c0[(long)s2 * 16 + c] : 0.0;          // coarse part of the preconditioned residual (constant per subdomain)
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const double zv = z[(g + i) * 16 + c] + cz;
        const double po = first ? 0.0 : p_old[(g + i) * 16 + c];
        pv[i] = zv + beta * po;
      }
#pragma unroll
      for (int i = 0; i < 3; ++i) acc[i] = blk[i * 3] * pv[0] + blk[i * 3 + 1] * pv[1] + blk[i * 3 + 2] * pv[2];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      acc[i] += __shfl_xor(acc[i], 16, 64);
      acc[i] += __shfl_xor(acc[i], 32, 64);
    }
    if (b == 0 && on) {
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        p_new[(idx * 3 + i) * 16 + c] = pv[i];
        y[(idx * 3 + i) * 16 + c] = acc[i];
        dot += pv[i] * acc[i];
      }
    }
  }
  fomb_store_partial(dot, red, partial);
}

__global__ __launch_bounds__(1024) void k_fomb_matvec(Tmpl t, int S, int Q, int P, ThetaP th, const int* __restrict__ nbr,
                                                      const double* __restrict__ A_diag, const double* __restrict__ A_cpl,
                                                      const double* __restrict__ z, const double* __restrict__ p_old,
                                                      const double* __restrict__ rz_new, const double* __restrict__ rz_old, int first,
                                                      const double* __restrict__ c0, double* __restrict__ p_new,
                                                      double* __restrict__ y, double* __restrict__ partial) {
  __shared__ double red[256];
  fomb_matvec_body<false>(t, S, Q, P, th, nbr, A_diag, A_cpl, z, p_old, rz_new, rz_old, first, c0, p_new, y, partial, red);
}

// the same on M + A(theta) (lrbms_fom_implicit_euler_batch)
__global__ __launch_bounds__(1024) void k_fomb_matvec_mass(Tmpl t, int S, int Q, int P, ThetaP th, const int* __restrict__ nbr,
                                                           const double* __restrict__ A_diag, const double* __restrict__ A_cpl,
                                                           const double* __restrict__ z, const double* __restrict__ p_old,
                                                           const double* __restrict__ rz_new, const double* __restrict__ rz_old,
                                                           int first, const double* __restrict__ c0, double* __restrict__ p_new,
                                                           double* __restrict__ y, double* __restrict__ partial) {
  __shared__ double red[256];
  fomb_matvec_body<true>(t, S, Q, P, th, nbr, A_diag, A_cpl, z, p_old, rz_new, rz_old, first, c0, p_new, y, partial, red);
}

// lane = (column c = lane & 15, element lane >> 4 of the wave's four).  alpha = rz / pAp per column (rz [16] from
// k_fomb_scalars, pAp re-summed from ppap [npap][16]); the diagonal 3x3 block of A(theta_c) is combined from the Q diagonal
// blocks and inverted on the spot (the expressions of k_fom_combine).  first: only z and the partials of the start residual.
// x is column m0 + c of X [S n][nmu].  prz_out / prr [gridDim.x][16].
// MASS: the mass (area [nT]: the template's element areas) joins the diagonal block before the inverse.
template <bool MASS>
__device__ __forceinline__ void fomb_update_body(long ne, int Q, int P, int nmu, int m0, const ThetaP& th, const double* __restrict__ A_diag,
                                                 const double* __restrict__ rz_in, const double* __restrict__ ppap, int npap,
                                                 int first, double* __restrict__ X, double* __restrict__ r,
                                                 const double* __restrict__ p, const double* __restrict__ y,
                                                 double* __restrict__ z, double* __restrict__ prz_out, double* __restrict__ prr,
                                                 const double* __restrict__ area, int nT, double* red) {
  const long nd = ne * 36;
  const int lane = threadIdx.x & 63, c = lane & 15, sub = lane >> 4, wave = threadIdx.x >> 6;
  const bool on = c < P;
  double thq[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) thq[q] = q < Q ? th.v[c][q] : 0.0;
  double alpha = 0.0;
  if (!first) {
    const double pap = fomb_colsum(ppap, npap, red);
    const double rz = rz_in[c];
    alpha = pap != 0.0 ? rz / pap : 0.0;
  }
  double rz = 0.0, rr = 0.0;
  for (long e0 = ((long)blockIdx.x * 16 + wave) * 4; e0 < ne; e0 += (long)gridDim.x * 64) {
    const long idx = e0 + sub;
    if (idx < ne && on) {
      double a[9], rv[3], xv[3] = {0.0, 0.0, 0.0}, pv[3] = {0.0, 0.0, 0.0}, yv[3] = {0.0, 0.0, 0.0};
#pragma unroll
      for (int k = 0; k < 9; ++k) a[k] = 0.0;
#pragma unroll
      for (int q = 0; q < 8; ++q)
        if (q < Q) {
#pragma unroll
          for (int k = 0; k < 9; ++k) a[k] += thq[q] * A_diag[q * nd + idx * 36 + k];
        }
      if (MASS) {
        const double ma = area[(unsigned)idx % (unsigned)nT];
#pragma unroll
        for (int k = 0; k < 9; ++k) a[k] += ma / 12.0 * (k % 4 == 0 ? 2.0 : 1.0);
      }
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const long g = (idx * 3 + i) * 16 + c;
        rv[i] = r[g];
        if (!first) {
          xv[i] = X[(idx * 3 + i) * nmu + m0 + c];
          pv[i] = p[g];
          yv[i] = y[g];
        }
      }
      const double d0 = a[4] * a[8] - a[5] * a[7], d1 = a[5] * a[6] - a[3] * a[8], d2 = a[3] * a[7] - a[4] * a[6];
      const double id = 1.0 / (a[0] * d0 + a[1] * d1 + a[2] * d2);
      double M[9];
      M[0] = d0 * id;
      M[1] = (a[2] * a[7] - a[1] * a[8]) * id;
      M[2] = (a[1] * a[5] - a[2] * a[4]) * id;
      M[3] = d1 * id;
      M[4] = (a[0] * a[8] - a[2] * a[6]) * id;
      M[5] = (a[2] * a[3] - a[0] * a[5]) * id;
      M[6] = d2 * id;
      M[7] = (a[1] * a[6] - a[0] * a[7]) * id;
      M[8] = (a[0] * a[4] - a[1] * a[3]) * id;
      if (!first) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          X[(idx * 3 + i) * nmu + m0 + c] = xv[i] + alpha * pv[i];
          rv[i] -= alpha * yv[i];
          r[(idx * 3 + i) * 16 + c] = rv[i];
        }
      }
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const double zi = M[i * 3] * rv[0] + M[i * 3 + 1] * rv[1] + M[i * 3 + 2] * rv[2];
        z[(idx * 3 + i) * 16 + c] = zi;
        rz += rv[i] * zi;
        rr += rv[i] * rv[i];
      }
    }
  }
  rz += __shfl_xor(rz, 16, 64);
  rz += __shfl_xor(rz, 32, 64);
  rr += __shfl_xor(rr, 16, 64);
  rr += __shfl_xor(rr, 32, 64);
  fomb_store_partial(rz, red, prz_out);
  fomb_store_partial(rr, red, prr);
}

__global__ __launch_bounds__(1024) void k_fomb_update(long ne, int Q, int P, int nmu, int m0, ThetaP th, const double* __restrict__ A_diag,
                                                      const double* __restrict__ rz_in, const double* __restrict__ ppap, int npap,
                                                      int first, double* __restrict__ X, double* __restrict__ r,
                                                      const double* __restrict__ p, const double* __restrict__ y,
                                                      double* __restrict__ z, double* __restrict__ prz_out, double* __restrict__ prr) {
  __shared__ double red[1024];
  fomb_update_body<false>(ne, Q, P, nmu, m0, th, A_diag, rz_in, ppap, npap, first, X, r, p, y, z, prz_out, prr, nullptr, 1, red);
}

// the same with the inverse diagonal blocks of M + A(theta) (lrbms_fom_implicit_euler_batch)
__global__ __launch_bounds__(1024) void k_fomb_update_mass(long ne, int Q, int P, int nmu, int m0, ThetaP th,
                                                           const double* __restrict__ A_diag, const double* __restrict__ rz_in,
                                                           const double* __restrict__ ppap, int npap, int first, double* __restrict__ X,
                                                           double* __restrict__ r, const double* __restrict__ p,
                                                           const double* __restrict__ y, double* __restrict__ z,
                                                           double* __restrict__ prz_out, double* __restrict__ prr,
                                                           const double* __restrict__ area, int nT) {
  __shared__ double red[1024];
  fomb_update_body<true>(ne, Q, P, nmu, m0, th, A_diag, rz_in, ppap, npap, first, X, r, p, y, z, prz_out, prr, area, nT, red);
}

// Implicit Euler step of a panel (lrbms_fom_implicit_euler_batch), warm start x = u_k: the columns m0 .. m0 + P - 1 of the slab
// Uk [S n][nmu] -> the panel vector uk [S n][16] (columns c >= P zero) and the same columns of the next slab X.
__global__ __launch_bounds__(256) void k_fomb_load(long nv, int P, int nmu, int m0, const double* __restrict__ Uk, double* __restrict__ X,
                                                   double* __restrict__ uk) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nv * 16; i += (long)gridDim.x * blockDim.x) {
    const long g = i >> 4;
    const int c = (int)(i & 15);
    double v = 0.0;
    if (c < P) {
      v = Uk[g * nmu + m0 + c];
      X[g * nmu + m0 + c] = v;
    }
    uk[i] = v;
  }
}

// r = M u_k + dt sum_j phi_c[j] b_j - y per column (y = (M + dt A(theta_c)) u_k from k_fomb_matvec_mass with first = 1), the
// arithmetic of k_fom_step_residual_src; columns c >= P of r zero.  phi: the table [nmu][rows][K] offset to the step's row, so
// column c reads phi + (m0 + c) rows K.  Lanes as in k_fomb_update; partial [gridDim.x][16] = |M u_k + dt sum_j phi b_j|^2.
__global__ __launch_bounds__(1024) void k_fomb_step_residual(Tmpl t, long ne, double dt, int K, int P, int m0, long phi_stride,
                                                             const double* __restrict__ phi, const double* __restrict__ bK,
                                                             const double* __restrict__ uk, const double* __restrict__ y,
                                                             double* __restrict__ r, double* __restrict__ partial) {
  __shared__ double red[256];
  const long nv = ne * 3;
  const int lane = threadIdx.x & 63, c = lane & 15, sub = lane >> 4, wave = threadIdx.x >> 6;
  const bool on = c < P;
  const double* ph = phi + (long)(m0 + (on ? c : 0)) * phi_stride;
  double acc = 0.0;
  for (long e0 = ((long)blockIdx.x * 16 + wave) * 4; e0 < ne; e0 += (long)gridDim.x * 64) {
    const long idx = e0 + sub;
    if (idx >= ne) continue;
    if (!on) {
      for (int i = 0; i < 3; ++i) r[(idx * 3 + i) * 16 + c] = 0.0;
      continue;
    }
    const double m = t.area[(unsigned)idx % (unsigned)t.nT] / 12.0;
    const double u0 = uk[(idx * 3) * 16 + c], u1 = uk[(idx * 3 + 1) * 16 + c], u2 = uk[(idx * 3 + 2) * 16 + c];
    const double sum = u0 + u1 + u2;
    const double uv[3] = {u0, u1, u2};
    double bk[3] = {0.0, 0.0, 0.0};
    for (int j = 0; j < K; ++j) {
      const double pj = ph[j];
      const double* bj = bK + (long)j * nv + idx * 3;
      for (int i = 0; i < 3; ++i) bk[i] += pj * bj[i];
    }
    for (int i = 0; i < 3; ++i) {
      // the spelled-out contraction of k_fom_step_residual_src
      const double dtb = dt * bk[i];
      const double rhs = __fma_rn(m, sum + uv[i], dtb);
      r[(idx * 3 + i) * 16 + c] = rhs - y[(idx * 3 + i) * 16 + c];
      acc += rhs * rhs;
    }
  }
  acc += __shfl_xor(acc, 16, 64);
  acc += __shfl_xor(acc, 32, 64);
  fomb_store_partial(acc, red, partial);
}

// r0 [S][16] = sum of the residual over subdomain s per column (restriction to the coarse space); zeroes the coarse solution
// c0 [S][16] and the coarse parts prz_c [16][S] of r.z, which k_coarse_apply accumulates into.  One workgroup per subdomain.
__global__ __launch_bounds__(256) void k_fomb_restrict(int S, int n, const double* __restrict__ r, double* __restrict__ r0,
                                                       double* __restrict__ c0, double* __restrict__ prz_c) {
  __shared__ double red[256];
  const int s = blockIdx.x, tid = threadIdx.x, c = tid & 15, j = tid >> 4;
  double acc = 0.0;
  for (int base = 0; base < n; base += 128) {
    double v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int i = base + j + 16 * k;
      v[k] = i < n ? r[((long)s * n + i) * 16 + c] : 0.0;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) acc += v[k];
  }
  red[tid] = acc;
  __syncthreads();
  for (int off = 128; off >= 16; off >>= 1) {
    if (tid < off) red[tid] += red[tid + off];
    __syncthreads();
  }
  if (tid < 16) {
    r0[(long)s * 16 + tid] = red[tid];
    c0[(long)s * 16 + tid] = 0.0;
    prz_c[(long)tid * S + s] = 0.0;
  }
}

// rz [16]: column blockIdx.x = the npart partials prz [npart][16] of the update kernel + the ncoarse coarse parts prz_c [16][ncoarse]
__global__ __launch_bounds__(256) void k_fomb_scalars(const double* __restrict__ prz, int npart, const double* __restrict__ prz_c,
                                                      int ncoarse, double* __restrict__ rz) {
  __shared__ double red[256];
  const int c = blockIdx.x;
  double acc = 0.0;
  for (int i = threadIdx.x; i < npart; i += 256) acc += prz[(long)i * 16 + c];
  for (int i = threadIdx.x; i < ncoarse; i += 256) acc += prz_c[(long)c * ncoarse + i];
  const double sum = block_sum_256(acc, red);
  if (threadIdx.x == 0) rz[c] = sum;
}

struct FomB {
  double *Amu_d, *Amu_c, *Minv;     // scratch of the coarse setup: the combined operator at the mean theta
  double *r, *z, *p[2], *y;         // [nv][16]
  double *ppap, *prz, *prr;         // [gm][16], [gu][16], [gu][16]
  double *r0, *c0, *prz_c, *rz[2];  // [S][16], [S][16], [16][S], [16] each
  const double* A0inv = nullptr;
  long ne, nv;
  int gm, gu;                       // workgroups (= partial rows) of the matvec (16 elements per pass) / update kernel (64)
  static long scratch(lrbms_ctx* ctx) {
    const long S = ctx->S, ne = S * ctx->t.nT;
    return ne * 36 + S * 4 * ctx->t.ncf * 9 + ne * 9;
  }
  static long total(lrbms_ctx* ctx) {
    const long S = ctx->S, ne = S * ctx->t.nT;
    return scratch(ctx) + 5 * ne * 3 * 16 + 3 * FOMB_GRID_MAX * 16 + 3 * S * 16 + 32 + 16;
  }
  void carve(lrbms_ctx* ctx, double* work) {
    const Tmpl& t = ctx->t;
    const long S = ctx->S;
    ne = S * t.nT;
    nv = ne * 3;
    gm = (int)((ne + 15) / 16 < FOMB_GRID_MAX ? (ne + 15) / 16 : FOMB_GRID_MAX);
    gu = (int)((ne + 63) / 64 < FOMB_GRID_MAX ? (ne + 63) / 64 : FOMB_GRID_MAX);
    Amu_d = work;
    Amu_c = Amu_d + ne * 36;
    Minv = Amu_c + S * 4 * t.ncf * 9;
    r = work + scratch(ctx);
    z = r + nv * 16;
    p[0] = z + nv * 16;
    p[1] = p[0] + nv * 16;
    y = p[1] + nv * 16;
    ppap = y + nv * 16;
    prz = ppap + FOMB_GRID_MAX * 16;
    prr = prz + FOMB_GRID_MAX * 16;
    r0 = prr + FOMB_GRID_MAX * 16;
    c0 = r0 + S * 16;
    prz_c = c0 + S * 16;
    rz[0] = prz_c + S * 16;
    rz[1] = rz[0] + 16;               // ends at total() - 16
  }
};

// the sum per column of the partials part [b.gu][16] (r.r of the update kernel: b.prr), on the host in a fixed order
int fomb_host_rr(lrbms_ctx* ctx, const FomB& b, const double* part, std::vector<double>& host, double* rr, hipStream_t st) {
  LRBMS_HIP_CHECK(ctx, hipMemcpyAsync(host.data(), part, sizeof(double) * (size_t)b.gu * 16, hipMemcpyDeviceToHost, st));
  LRBMS_HIP_CHECK(ctx, hipStreamSynchronize(st));
  for (int c = 0; c < 16; ++c) {
    double acc = 0.0;
    for (int i = 0; i < b.gu; ++i) acc += host[(size_t)i * 16 + c];
    rr[c] = acc;
  }
  return LRBMS_OK;
}

// z -> coarse part and r.z per column for the residual the update kernel has just written
int fomb_precond_tail(lrbms_ctx* ctx, FomB& b, double* rz_out, hipStream_t st) {
  const int S = ctx->S;
  if (b.A0inv) {
    hipLaunchKernelGGL(k_fomb_restrict, dim3(S), dim3(256), 0, st, S, ctx->t.n, b.r, b.r0, b.c0, b.prz_c);
    LRBMS_LAUNCH_CHECK(ctx);
    if (int rc = launch_coarse_apply(ctx, 1, 16, b.A0inv, b.r0, b.c0, b.prz_c, st)) return rc;
  }
  hipLaunchKernelGGL(k_fomb_scalars, dim3(16), dim3(256), 0, st, b.prz, b.gu, b.prz_c, b.A0inv ? S : 0, rz_out);
  LRBMS_LAUNCH_CHECK(ctx);
  return LRBMS_OK;
}

// The panel's operator: the elliptic one, or (mass) the step operator M + A(theta) with theta pre-multiplied by dt
struct FombOp {
  int Q, P, nmu, m0;
  ThetaP th;
  const double *A_diag, *A_cpl;
  bool mass;
};

void fomb_launch_matvec(lrbms_ctx* ctx, FomB& b, const FombOp& op, const double* z, const double* p_old, const double* rz_new,
                        const double* rz_old, int first, const double* c0, double* p_new, hipStream_t st) {
  if (op.mass)
    hipLaunchKernelGGL(k_fomb_matvec_mass, dim3(b.gm), dim3(FOMB_THREADS), 0, st, ctx->t, ctx->S, op.Q, op.P, op.th, ctx->nbr, op.A_diag,
                       op.A_cpl, z, p_old, rz_new, rz_old, first, c0, p_new, b.y, b.ppap);
  else
    hipLaunchKernelGGL(k_fomb_matvec, dim3(b.gm), dim3(FOMB_THREADS), 0, st, ctx->t, ctx->S, op.Q, op.P, op.th, ctx->nbr, op.A_diag,
                       op.A_cpl, z, p_old, rz_new, rz_old, first, c0, p_new, b.y, b.ppap);
}

void fomb_launch_update(lrbms_ctx* ctx, FomB& b, const FombOp& op, const double* rz_in, int first, double* X, const double* p,
                        hipStream_t st) {
  if (op.mass)
    hipLaunchKernelGGL(k_fomb_update_mass, dim3(b.gu), dim3(FOMB_THREADS), 0, st, b.ne, op.Q, op.P, op.nmu, op.m0, op.th, op.A_diag, rz_in,
                       b.ppap, b.gm, first, X, b.r, p, b.y, b.z, b.prz, b.prr, ctx->t.area, ctx->t.nT);
  else
    hipLaunchKernelGGL(k_fomb_update, dim3(b.gu), dim3(FOMB_THREADS), 0, st, b.ne, op.Q, op.P, op.nmu, op.m0, op.th, op.A_diag, rz_in, b.ppap,
                       b.gm, first, X, b.r, p, b.y, b.z, b.prz, b.prr);
}

// PCG on one panel of P <= 16 columns (columns m0 .. m0 + P - 1 of the call), shared by lrbms_fom_solve_batch and the steps of
// lrbms_fom_implicit_euler_batch: on entry X holds the start values and b.r the start residual.  Iterates until the worst
// column with a nonzero reference is at or below rtol; the host checks follow fom_cg_run.  The reference per column is |r_0|
// (ref_part == nullptr: the right-hand side, the start value being zero) or the sum of the partials ref_part [b.gu][16] (the
// step's full right-hand side, left by k_fomb_step_residual); `what` names the caller in the error text.
int fomb_panel_run(lrbms_ctx* ctx, FomB& b, const FombOp& op, double* X, const double* ref_part, double rtol, int max_iter, int* its,
                   double* rel_out, const char* what, hipStream_t st) {
  const int P = op.P;
  const double* c0 = b.A0inv ? b.c0 : nullptr;
  std::vector<double> host((size_t)b.gu * 16);
  fomb_launch_update(ctx, b, op, b.rz[0], 1, X, b.p[0], st);
  LRBMS_LAUNCH_CHECK(ctx);
  if (int rc = fomb_precond_tail(ctx, b, b.rz[0], st)) return rc;
  double ref2[16], rr[16];
  if (int rc = fomb_host_rr(ctx, b, b.prr, host, rr, st)) return rc;
  if (ref_part) {
    if (int rc = fomb_host_rr(ctx, b, ref_part, host, ref2, st)) return rc;
  } else {
    for (int c = 0; c < 16; ++c) ref2[c] = rr[c];
  }
  auto worst = [&](const double* cur) {
    double w = 0.0;
    for (int c = 0; c < P; ++c)
      if (ref2[c] != 0.0) {
        const double rel = sqrt(cur[c] / ref2[c]);
        if (!(rel == rel)) return rel;                      // NaN
        if (rel > w) w = rel;
      }
    return w;
  };
  *its = 0;
  double rel = worst(rr);                  // 1 from a zero start value, or 0 if every right-hand side of the panel is zero
  *rel_out = 0.0;
  if (rel == 0.0) return LRBMS_OK;
  int it = 0, block = 10;
  while (rel > rtol && it < max_iter) {
    if (block > max_iter - it) block = max_iter - it;
    for (int k = 0; k < block; ++k, ++it) {
      const int c = it & 1, o = c ^ 1;
      fomb_launch_matvec(ctx, b, op, b.z, b.p[o], b.rz[c], b.rz[o], it == 0 ? 1 : 0, c0, b.p[c], st);
      fomb_launch_update(ctx, b, op, b.rz[c], 0, X, b.p[c], st);
      if (int rc = fomb_precond_tail(ctx, b, b.rz[o], st)) return rc;
    }
    LRBMS_LAUNCH_CHECK(ctx);
    if (int rc = fomb_host_rr(ctx, b, b.prr, host, rr, st)) return rc;
    rel = worst(rr);
    if (!(rel == rel)) return lrbms_fail(ctx, LRBMS_E_NOT_CONVERGED, what);
    const double rate = log(rel) / it;
    block = 25;
    if (rel > rtol && rate < 0.0) {                          // aim a little short: CG converges superlinearly
      const double need = 0.8 * (log(rtol) - log(rel)) / rate;
      block = need < 4.0 ? 4 : need > 100.0 ? 100 : (int)need;
    }
  }
  *its = it;
  *rel_out = rel;
  return LRBMS_OK;
}

}  // namespace

int64_t fom_solve_batch_work_size(lrbms_ctx* ctx, int nmu) {
  if (nmu < 1 || nmu > 64) return -1;
  return FomB::total(ctx);
}

int launch_fom_solve_batch(lrbms_ctx* ctx, int Q, int nmu, const double* theta, const double* A_diag, const double* A_cpl, int K,
                           const double* phi, const double* bK, double* work, double* X, double rtol, int max_iter, double* info,
                           hipStream_t st) {
  if (ctx->S_ext != ctx->S) return lrbms_fail(ctx, LRBMS_E_INVALID, "fom_solve_batch needs all subdomains on one rank");
  if (Q < 1 || Q > 8 || nmu < 1 || nmu > 64 || K < 1 || K > 64 || max_iter < 1 || !(rtol > 0.0))
    return lrbms_fail(ctx, LRBMS_E_INVALID, "fom_solve_batch: bad Q / nmu / K / max_iter / rtol");
  FomB b;
  b.carve(ctx, work);
  // one coarse level per call, at the mean theta of its columns (summed in column order)
  double* A0 = nullptr;
  if (int rc = coarse_begin(ctx, &A0, st)) return rc;
  if (A0) {
    QVecF tb;
    for (int q = 0; q < 8; ++q) {
      double acc = 0.0;
      for (int m = 0; q < Q && m < nmu; ++m) acc += theta[(long)m * Q + q];
      tb.v[q] = acc / nmu;
    }
    hipLaunchKernelGGL(k_fom_combine, dim3(4096), dim3(256), 0, st, ctx->t, ctx->S, Q, tb, 0.0, A_diag, A_cpl, b.Amu_d, b.Amu_c, b.Minv);
    hipLaunchKernelGGL(k_fom_coarse_entries, dim3(ctx->S), dim3(256), 0, st, ctx->t, ctx->S, ctx->nbr, b.Amu_d, b.Amu_c, A0);
    LRBMS_LAUNCH_CHECK(ctx);
    if (int rc = coarse_finish(ctx, &b.A0inv, st)) return rc;
  }
  int its_max = 0;
  double worst = 0.0;
  bool missed = false;
  for (int i = 0; i < 8; ++i) ctx->fomb_panels[i] = 0.0;
  for (int m0 = 0; m0 < nmu; m0 += 16) {
    const int P = nmu - m0 < 16 ? nmu - m0 : 16;
    ThetaP th;
    for (int c = 0; c < 16; ++c)
      for (int q = 0; q < 8; ++q) th.v[c][q] = (c < P && q < Q) ? theta[(long)(m0 + c) * Q + q] : 0.0;
    hipLaunchKernelGGL(k_fomb_rhs, dim3(2048), dim3(256), 0, st, b.nv, K, P, nmu, m0, phi, bK, b.r, X);
    LRBMS_LAUNCH_CHECK(ctx);
    int it = 0;
    double rel = 0.0;
    const FombOp op{Q, P, nmu, m0, th, A_diag, A_cpl, false};
    if (int rc = fomb_panel_run(ctx, b, op, X, nullptr, rtol, max_iter, &it, &rel, "fom_solve_batch: NaN residual (operator not SPD?)", st))
      return rc;
    ctx->fomb_panels[m0 / 16 * 2] = it;
    ctx->fomb_panels[m0 / 16 * 2 + 1] = rel;
    if (it > its_max) its_max = it;
    if (rel > worst) worst = rel;
    if (rel > rtol) missed = true;
  }
  if (info) { info[0] = its_max; info[1] = worst; }
  if (missed) return lrbms_fail(ctx, LRBMS_E_NOT_CONVERGED, "fom_solve_batch: CG did not reach rtol");
  return LRBMS_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// Batched full-order trajectories (lrbms_fom_implicit_euler_batch): column m runs the implicit Euler
//   (M + dt A(theta_m)) u_{k+1} = M u_k + dt sum_j phi[m][k+1][j] b_K[j],   k = 0 .. nt-1,
// on U [nt+1][S][n][nmu] (parameter fastest; slab 0 is input).  Panels of <= 16 columns, panels outermost: a panel runs its
// whole trajectory with one theta table (pre-multiplied by dt), every step a warm-started PCG of the panel kernels on the step
// operator (k_fomb_matvec_mass / k_fomb_update_mass), relative to the step's full right-hand side per column.  Per step
//   k_fomb_load            u_k of the panel's columns -> b.z [S n][16] and the next slab (x = u_k)
//   k_fomb_matvec_mass     first = 1, no coarse part: y = (M + dt A(theta_c)) u_k
//   k_fomb_step_residual   r = M u_k + dt sum_j phi b_j - y, partials of |M u_k + dt sum_j phi b_j|^2 into b.ppap
// then fomb_panel_run (its first update kernel overwrites b.z, which the two kernels before it have consumed: no extra work).
// One coarse level per call, A0 = R0 (M + dt A(theta_bar)) R0^T at the call mean, for all panels and steps.
int64_t fom_implicit_euler_batch_work_size(lrbms_ctx* ctx, int nmu) {
  if (nmu < 1 || nmu > 64) return -1;
  return FomB::total(ctx);
}

namespace {

// The driver of lrbms_fom_implicit_euler_batch (tv == false: theta [nmu][Q], one table per panel) and of
// lrbms_fom_implicit_euler_batch_tv (tv == true: theta [nmu][nt+1][Q], the step k -> k+1 fills the panel's table from row k + 1;
// the coarse level sits at the mean over the columns and the rows 1 .. nt).  The launches are the same in both forms.
int fom_euler_batch_drive(lrbms_ctx* ctx, const std::string& name, bool tv, int Q, int K, int nmu, const double* theta, double dt, int nt,
                          const double* A_diag, const double* A_cpl, const double* bK, const double* phi, double* work, double* U,
                          double rtol, int max_iter, double* info, hipStream_t st) {
  if (ctx->S_ext != ctx->S) return lrbms_fail(ctx, LRBMS_E_INVALID, name + " needs all subdomains on one rank");
  if (Q < 1 || Q > 8 || nmu < 1 || nmu > 64 || K < 1 || K > 64 || nt < 1 || max_iter < 1 || !(rtol > 0.0) || !(dt > 0.0))
    return lrbms_fail(ctx, LRBMS_E_INVALID, name + ": bad Q / nmu / K / nt / dt / max_iter / rtol");
  const long th_ld = tv ? (long)(nt + 1) * Q : Q;        // doubles per column of theta
  const std::string nan_text = name + ": NaN residual (operator not SPD?)";
  FomB b;
  b.carve(ctx, work);
  // one coarse level per call, of the step operator at the mean theta of its columns (summed in column order)
  double* A0 = nullptr;
  if (int rc = coarse_begin(ctx, &A0, st)) return rc;
  if (A0) {
    QVecF tb;
    for (int q = 0; q < 8; ++q) {
      double acc = 0.0;
      for (int m = 0; q < Q && m < nmu; ++m) {
        if (!tv) acc += theta[(long)m * Q + q];
        for (int k = 1; tv && k <= nt; ++k) acc += theta[m * th_ld + (long)k * Q + q];
      }
      tb.v[q] = tv ? dt * (acc / ((double)nmu * nt)) : dt * (acc / nmu);
    }
    hipLaunchKernelGGL(k_fom_combine, dim3(4096), dim3(256), 0, st, ctx->t, ctx->S, Q, tb, 1.0, A_diag, A_cpl, b.Amu_d, b.Amu_c, b.Minv);
    hipLaunchKernelGGL(k_fom_coarse_entries, dim3(ctx->S), dim3(256), 0, st, ctx->t, ctx->S, ctx->nbr, b.Amu_d, b.Amu_c, A0);
    LRBMS_LAUNCH_CHECK(ctx);
    if (int rc = coarse_finish(ctx, &b.A0inv, st)) return rc;
  }
  const long slab = b.nv * nmu;
  long its_sum = 0;
  double worst = 0.0;
  bool missed = false;
  for (int i = 0; i < 8; ++i) ctx->fombe_panels[i] = 0.0;
  for (int m0 = 0; m0 < nmu; m0 += 16) {
    FombOp op{Q, nmu - m0 < 16 ? nmu - m0 : 16, nmu, m0, {}, A_diag, A_cpl, true};
    for (int c = 0; c < 16; ++c)
      for (int q = 0; q < 8; ++q) op.th.v[c][q] = (c < op.P && q < Q) ? dt * theta[(m0 + c) * th_ld + q] : 0.0;
    long its_p = 0;
    double worst_p = 0.0;
    for (int step = 0; step < nt; ++step) {
      if (tv)                                                // the operator of this step: row step + 1
        for (int c = 0; c < op.P; ++c)
          for (int q = 0; q < Q; ++q) op.th.v[c][q] = dt * theta[(m0 + c) * th_ld + (long)(step + 1) * Q + q];
      const double* Uk = U + step * slab;
      double* X = U + (step + 1) * slab;
      hipLaunchKernelGGL(k_fomb_load, dim3(2048), dim3(256), 0, st, b.nv, op.P, nmu, m0, Uk, X, b.z);
      fomb_launch_matvec(ctx, b, op, b.z, b.p[1], b.rz[0], b.rz[1], 1, nullptr, b.p[0], st);
      hipLaunchKernelGGL(k_fomb_step_residual, dim3(b.gu), dim3(FOMB_THREADS), 0, st, ctx->t, b.ne, dt, K, op.P, m0, (long)(nt + 1) * K,
                         phi + (long)(step + 1) * K, bK, b.z, b.y, b.r, b.ppap);
      LRBMS_LAUNCH_CHECK(ctx);
      int it = 0;
      double rel = 0.0;
      if (int rc = fomb_panel_run(ctx, b, op, X, b.ppap, rtol, max_iter, &it, &rel, nan_text.c_str(), st))
        return rc;
      its_p += it;
      const bool nan = !(rel == rel);
      if (nan || rel > worst_p) worst_p = rel;
      if (nan || rel > rtol) {                               // this panel stops here; its later slabs are not written
        missed = true;
        break;
      }
    }
    ctx->fombe_panels[m0 / 16 * 2] = (double)its_p;
    ctx->fombe_panels[m0 / 16 * 2 + 1] = worst_p;
    its_sum += its_p;
    if (!(worst_p == worst_p) || worst_p > worst) worst = worst_p;
  }
  if (info) { info[0] = (double)its_sum; info[1] = worst; }
  if (missed) return lrbms_fail(ctx, LRBMS_E_NOT_CONVERGED, name + ": CG did not reach rtol");
  return LRBMS_OK;
}

}  // namespace

int launch_fom_implicit_euler_batch(lrbms_ctx* ctx, int Q, int K, int nmu, const double* theta, double dt, int nt, const double* A_diag,
                                    const double* A_cpl, const double* bK, const double* phi, double* work, double* U, double rtol,
                                    int max_iter, double* info, hipStream_t st) {
  return fom_euler_batch_drive(ctx, "fom_implicit_euler_batch", false, Q, K, nmu, theta, dt, nt, A_diag, A_cpl, bK, phi, work, U, rtol,
                               max_iter, info, st);
}

// lrbms_fom_implicit_euler_batch_tv: theta_t [nmu][nt+1][Q] host, column m steps with (M + dt A(theta_t[m][k+1])) u_{k+1} = ...
int launch_fom_implicit_euler_batch_tv(lrbms_ctx* ctx, int Q, int K, int nmu, const double* theta_t, double dt, int nt,
                                       const double* A_diag, const double* A_cpl, const double* bK, const double* phi, double* work,
                                       double* U, double rtol, int max_iter, double* info, hipStream_t st) {
  return fom_euler_batch_drive(ctx, "fom_implicit_euler_batch_tv", true, Q, K, nmu, theta_t, dt, nt, A_diag, A_cpl, bK, phi, work, U,
                               rtol, max_iter, info, st);
}

namespace {

// The time loop shared by lrbms_fom_implicit_euler and lrbms_fom_implicit_euler_src: combine (M + dt A(mu)) once, then per
// step y = (M + dt A) u_k, the step's right-hand side and residual (`step_rhs(step, uk, c)` launches the kernel that writes
// c.r and the |rhs|^2 partials into c.ppap), and a warm-started CG.
template <typename StepRhs>
int fom_euler_run(lrbms_ctx* ctx, const char* name, int Q, const double* theta, double dt, int nt, const double* A_diag,
                  const double* A_cpl, double* work, double* U, double rtol, int max_iter, double* info, hipStream_t st,
                  StepRhs&& step_rhs) {
  if (ctx->S_ext != ctx->S) return lrbms_fail(ctx, LRBMS_E_INVALID, "fom_implicit_euler needs all subdomains on one rank");
  if (Q < 1 || Q > 8 || max_iter < 1 || !(rtol > 0.0) || nt < 1 || !(dt > 0.0))
    return lrbms_fail(ctx, LRBMS_E_INVALID, "fom_implicit_euler: bad Q / max_iter / rtol / nt / dt");
  QVecF th;
  for (int q = 0; q < 8; ++q) th.v[q] = q < Q ? dt * theta[q] : 0.0;
  FomCg c;
  c.carve(ctx, work);
  const int nblk = c.nblk;
  hipLaunchKernelGGL(k_fom_combine, dim3(4096), dim3(256), 0, st, ctx->t, ctx->S, Q, th, 1.0, A_diag, A_cpl, c.Amu_d, c.Amu_c, c.Minv);
  LRBMS_LAUNCH_CHECK(ctx);
  if (int rc = fom_coarse_setup(ctx, c, st)) return rc;
  std::vector<double> host(nblk);
  long total_it = 0;
  double worst = 0.0;
  for (int step = 0; step < nt; ++step) {
    const double* uk = U + (long)step * c.nv;
    double* x = U + (long)(step + 1) * c.nv;
    LRBMS_HIP_CHECK(ctx, hipMemcpyAsync(x, uk, sizeof(double) * c.nv, hipMemcpyDeviceToDevice, st));
    // y = (M + dt A) u_k  (the matvec kernel with first = 1 takes its direction from `z`)
    hipLaunchKernelGGL(k_fom_cg_matvec, dim3(c.nmv), dim3(256), 0, st, ctx->t, ctx->S, ctx->nbr, c.Amu_d, c.Amu_c, uk, c.p[1], c.prz[0],
                       c.prz[1], nblk, 1, (const double*)nullptr, c.p[0], c.y, c.ppap);
    step_rhs(step, uk, c);
    LRBMS_LAUNCH_CHECK(ctx);
    double ref2 = 0.0;
    if (int rc = fom_host_sum(ctx, c.ppap, host, &ref2, st)) return rc;
    if (ref2 == 0.0) continue;      // zero right-hand side: u_{k+1} = u_k = 0
    int it = 0;
    double rel = 0.0;
    if (int rc = fom_cg_run(ctx, c, x, ref2, rtol, max_iter, &it, &rel, st)) return rc;
    total_it += it;
    if (rel > worst) worst = rel;
    if (rel > rtol) {
      if (info) { info[0] = (double)total_it; info[1] = worst; }
      return lrbms_fail(ctx, LRBMS_E_NOT_CONVERGED, name);
    }
  }
  if (info) { info[0] = (double)total_it; info[1] = worst; }
  return LRBMS_OK;
}

}  // namespace

// Implicit Euler for M u' + A(mu) u = b (pyMOR ImplicitEulerTimeStepper as used at discretize_parabolic_block_swipdg.py:87;
// InstationaryDuneDiscretization._solve :28-40):  (M + dt A(mu)) u_{k+1} = M u_k + dt b,  nt steps in ONE call: the
// theta-weighted blocks (+ the mass on the diagonal 3x3 blocks) are combined once, every step is a warm-started CG with
// the kernels of lrbms_fom_solve.  U [nt+1][S][n]: U[0] is the initial value (input), U[1..nt] are written.
// info[0] = CG iterations over all steps, info[1] = worst final residual relative to |M u_k + dt b|.
int launch_fom_implicit_euler(lrbms_ctx* ctx, int Q, const double* theta, double dt, int nt, const double* A_diag, const double* A_cpl,
                              const double* b, double* work, double* U, double rtol, int max_iter, double* info, hipStream_t st) {
  return fom_euler_run(ctx, "fom_implicit_euler: CG did not reach rtol", Q, theta, dt, nt, A_diag, A_cpl, work, U, rtol, max_iter,
                       info, st, [&](int, const double* uk, FomCg& c) {
    hipLaunchKernelGGL(k_fom_step_residual, dim3(c.nblk), dim3(256), 0, st, ctx->t, c.ne, dt, uk, b, c.y, c.r, c.ppap);
  });
}

// The same with the time-dependent affine source f(t, mu) = sum_j phi_j(t, mu) f_j:
//   (M + dt A(mu)) u_{k+1} = M u_k + dt sum_j phi[k+1][j] b_j,   bK [K][S][n], phi [nt+1][K] (device; row k+1 = step k).
// Only the kernel that forms the step's right-hand side differs from launch_fom_implicit_euler.
int launch_fom_implicit_euler_src(lrbms_ctx* ctx, int Q, int K, const double* theta, double dt, int nt, const double* A_diag,
                                  const double* A_cpl, const double* bK, const double* phi, double* work, double* U, double rtol,
                                  int max_iter, double* info, hipStream_t st) {
  if (K < 1) return lrbms_fail(ctx, LRBMS_E_INVALID, "fom_implicit_euler_src: K < 1");
  return fom_euler_run(ctx, "fom_implicit_euler_src: CG did not reach rtol", Q, theta, dt, nt, A_diag, A_cpl, work, U, rtol,
                       max_iter, info, st, [&](int step, const double* uk, FomCg& c) {
    hipLaunchKernelGGL(k_fom_step_residual_src, dim3(c.nblk), dim3(256), 0, st, ctx->t, c.ne, dt, uk, K, phi + (long)(step + 1) * K,
                       bK, c.y, c.r, c.ppap);
  });
}
