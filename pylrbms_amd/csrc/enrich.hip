// Online enrichment: batched local corrector solves (SURVEY.md section 8f "next" #1).
//
// Reference: DuneDiscretization.solve_for_local_correction (discretize_elliptic_block_swipdg.py:227-316) assembles
// the SWIPDG operator of the neighbourhood N(ii) = {ii and its face neighbours} with an all-Dirichlet local boundary
// (:240-247, :794-795), the L2 functional of f as right-hand side (:263-268), solves with ISTL and keeps the part of
// the solution that lives on subdomain ii (:303-316).  online_enrichment.py:49-50 does this for one marked subdomain
// after the other.
//
// Here every marked subdomain is one workgroup that runs its whole preconditioned CG without leaving the CU:
//  * the neighbourhood operator is never assembled: it is the block-ELL data the discretization already holds
//    (A_diag, A_cpl) plus the Dirichlet correction blocks D_corr on the outer coupling faces;
//  * each thread owns one element (EPT == 1, the 384-DoF subdomains of the benchmark configs): its four theta-weighted
//    3x3 blocks, its inverse diagonal block, x and r stay in registers for all iterations;
//  * the search direction p (5 n doubles) lives in LDS, where the neighbouring elements read it;
//  * the three dot products of an iteration are fixed-order wave + workgroup reductions (deterministic), three
//    barriers per iteration, no global synchronisation and no HBM traffic inside the loop.
// Larger templates fall back to EPT > 1 elements per thread with the blocks re-read (L2) every iteration.
//
// That PCG is written once (HoodPcg: set-up, operator apply, first direction, iteration) and instantiated by two kernels that
// differ in the operator block they hand it and in what surrounds the solve: k_hood_pcg (stationary: hood_block, one solve from
// x = 0) and k_hood_euler (parabolic: euler_block, one warm-started solve per implicit-Euler step).  The host side is shared the
// same way: one internal launch_local_correction holds the refusals, the marked upload, the (EPT, BT) ladder and the verdict.
#include "lrbms_dev.h"

#include <type_traits>

namespace {

struct QVecE { double v[8]; };
struct Vec3 { double v[3]; };

// theta-weighted block `bidx` (0 = diagonal, 1 + f = face f) of element e of neighbourhood member `slot` (subdomain kk)
// of marked subdomain ii.  Returns the LDS offset of the source element's first DoF, or -1 if the block is absent.
__device__ inline int hood_block(const Tmpl& t, int S, const int* __restrict__ nbr, int Q, const QVecE& th,
                                 const double* __restrict__ A_diag, const double* __restrict__ A_cpl,
                                 const double* __restrict__ D_corr, int ii, int slot, int kk, int e, int bidx, double Hb[9]) {
  const int nT = t.nT, n = t.n;
  const double* base;
  long qs;
  int src;
  if (bidx == 0) {
    base = A_diag + ((long)kk * nT + e) * 36;
    qs = (long)S * nT * 36;
    src = slot * n + 3 * e;
  } else {
    const int f = bidx - 1;
    const int nb = t.nb_elem[e * 3 + f];
    if (nb >= 0) {
      base = A_diag + ((long)kk * nT + e) * 36 + bidx * 9;
      qs = (long)S * nT * 36;
      src = slot * n + 3 * nb;
    } else {
      const int side = -1 - nb, sl2 = side_to_slot(side);
      int srcslot;
      if (slot == 2) {
        if (nbr[ii * 5 + sl2] < 0) return -1;   // physical boundary: already in A_diag
        srcslot = sl2;
      } else {
        if (sl2 != 4 - slot) return -1;         // outer boundary of the neighbourhood: Dirichlet, no coupling
        srcslot = 2;
      }
      base = A_cpl + (((long)kk * 4 + side) * t.ncf + t.elem_side_pos[e * 3 + f]) * 9;
      qs = (long)S * 4 * t.ncf * 9;
      src = srcslot * n + 3 * t.nb_elem_out[e * 3 + f];
    }
  }
#pragma unroll
  for (int i = 0; i < 9; ++i) Hb[i] = 0.0;
  for (int q = 0; q < Q; ++q) {
    const double w = th.v[q];
#pragma unroll
    for (int i = 0; i < 9; ++i) Hb[i] += w * base[q * qs + i];
  }
  if (bidx == 0 && slot != 2) {
    const long dqs = (long)S * 4 * t.ncf * 9;
    for (int f = 0; f < 3; ++f) {
      const int nb = t.nb_elem[e * 3 + f];
      if (nb >= 0) continue;
      const int side = -1 - nb, sl2 = side_to_slot(side);
      if (sl2 == 4 - slot || nbr[kk * 5 + sl2] < 0) continue;
      const double* dc = D_corr + (((long)kk * 4 + side) * t.ncf + t.elem_side_pos[e * 3 + f]) * 9;
      for (int q = 0; q < Q; ++q) {
        const double w = th.v[q];
#pragma unroll
        for (int i = 0; i < 9; ++i) Hb[i] += w * dc[q * dqs + i];
      }
    }
  }
  return src;
}

// Inverse of a 3x3 block.  det = a0 c0 + a1 c1 + a2 c2 has its contraction written out: left to the compiler, which of the first two
// products stays unfused follows the operand order of the surrounding code, and every entry of the inverse, hence the last bits of
// every iterate, with it.  A0_PLAIN names that product (a0 c0, else a1 c1); each kernel keeps the form it has always been compiled to.
template <bool A0_PLAIN>
__device__ inline void inv3(const double a[9], double o[9]) {
  const double c0 = a[4] * a[8] - a[5] * a[7], c1 = a[5] * a[6] - a[3] * a[8], c2 = a[3] * a[7] - a[4] * a[6];
  const double id = 1.0 / (A0_PLAIN ? fma(a[2], c2, fma(a[1], c1, a[0] * c0)) : fma(a[2], c2, fma(a[0], c0, a[1] * c1)));
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

template <int NW>
__device__ inline double block_sum(double v, double* red, int lane, int wave) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  if (lane == 0) red[wave] = v;
  __syncthreads();
  double s = 0.0;
#pragma unroll
  for (int w = 0; w < NW; ++w) s += red[w];
  return s;
}

template <int NW>
__device__ inline void block_sum2(double& a, double& b, double* red, int lane, int wave) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    a += __shfl_down(a, off, 64);
    b += __shfl_down(b, off, 64);
  }
  if (lane == 0) {
    red[wave] = a;
    red[NW + wave] = b;
  }
  __syncthreads();
  double sa = 0.0, sb = 0.0;
#pragma unroll
  for (int w = 0; w < NW; ++w) {
    sa += red[w];
    sb += red[NW + w];
  }
  a = sa;
  b = sb;
}

// The block-Jacobi PCG of one neighbourhood, one workgroup of BT threads with EPT elements per thread.  `block(slot, kk, e, bidx, Hb)`
// is the operator: it fills the 3x3 block `bidx` of an element and returns the LDS offset of its source element (-1: absent), as
// hood_block does.  EPT == 1 keeps the four blocks in registers; EPT > 1 asks `block` again in every apply.
template <int EPT, int BT>
struct HoodPcg {
  static constexpr int NW = BT / 64;
  static constexpr bool REG = EPT == 1;
  int n, lane, wave;
  double* P;       // [5][n] the vector the operator is applied to: the search direction (LDS)
  double* redA;    // [NW]
  double* redB;    // [2][NW]
  int slot[EPT], kk[EPT], el[EPT];
  bool act[EPT];
  double x[EPT][3], r[EPT][3], p[EPT][3], Mi[EPT][9];
  double H[REG ? 4 : 1][9];
  int src[REG ? 4 : 1];

  // Indices, blocks and M^-1 = inv3<DET_A0_PLAIN>(diagonal block) of this thread's elements; x = r = p = 0 and P = 0 (the slots of absent
  // neighbours stay zero for good).  No barrier: the caller has one between these zeros and its first write of P.
  template <bool DET_A0_PLAIN, class Block>
  __device__ __forceinline__ void setup(const Tmpl& t, const int* __restrict__ nbr, int ii, double* lds, const Block& block) {
    const int tid = threadIdx.x, nT = t.nT, nel = 5 * nT;
    n = t.n;
    lane = tid & 63;
    wave = tid >> 6;
    P = lds;
    redA = lds + 5 * n;
    redB = redA + NW;
    for (int i = tid; i < 5 * n; i += BT) P[i] = 0.0;
#pragma unroll
    for (int k = 0; k < EPT; ++k) {
      const int j = tid + k * BT;
      slot[k] = j < nel ? j / nT : 0;
      el[k] = j < nel ? j - slot[k] * nT : 0;
      kk[k] = j < nel ? nbr[ii * 5 + slot[k]] : -1;
      act[k] = kk[k] >= 0;
#pragma unroll
      for (int i = 0; i < 3; ++i) x[k][i] = r[k][i] = p[k][i] = 0.0;
#pragma unroll
      for (int i = 0; i < 9; ++i) Mi[k][i] = 0.0;
      if constexpr (REG) {
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          src[b] = -1;
#pragma unroll
          for (int i = 0; i < 9; ++i) H[b][i] = 0.0;
        }
      }
      if (act[k]) {
        double H0[9];
        if constexpr (REG) {
#pragma unroll
          for (int b = 0; b < 4; ++b) {
            double Hb[9];
            const int sb = block(slot[k], kk[k], el[k], b, Hb);
            src[b] = sb;
            if (sb >= 0) {
#pragma unroll
              for (int i = 0; i < 9; ++i) H[b][i] = Hb[i];
            }
          }
#pragma unroll
          for (int i = 0; i < 9; ++i) H0[i] = H[0][i];
        } else {
          block(slot[k], kk[k], el[k], 0, H0);
        }
        inv3<DET_A0_PLAIN>(H0, Mi[k]);
      }
    }
  }

  // P[own DoFs] = v
  __device__ __forceinline__ void publish(const double (&v)[EPT][3]) {
#pragma unroll
    for (int k = 0; k < EPT; ++k) {
      if (act[k]) {
#pragma unroll
        for (int i = 0; i < 3; ++i) P[slot[k] * n + 3 * el[k] + i] = v[k][i];
      }
    }
  }

  // (H v) of this thread's element k for the vector v that is complete in P.  (Returned by value: handing the three sums back
  // through a reference costs the EPT > 1 forms scratch.)
  template <class Block>
  __device__ __forceinline__ Vec3 apply(const Block& block, int k) const {
    Vec3 y = {{0.0, 0.0, 0.0}};
    if constexpr (REG) {
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int sb = src[b] >= 0 ? src[b] : 0;     // absent blocks are zero: read any valid address
        const double p0 = P[sb], p1 = P[sb + 1], p2 = P[sb + 2];
#pragma unroll
        for (int i = 0; i < 3; ++i) y.v[i] += H[b][i * 3] * p0 + H[b][i * 3 + 1] * p1 + H[b][i * 3 + 2] * p2;
      }
    } else if (act[k]) {
      for (int b = 0; b < 4; ++b) {
        double Hb[9];
        const int sb = block(slot[k], kk[k], el[k], b, Hb);
        if (sb < 0) continue;
        const double p0 = P[sb], p1 = P[sb + 1], p2 = P[sb + 2];
#pragma unroll
        for (int i = 0; i < 3; ++i) y.v[i] += Hb[i * 3] * p0 + Hb[i * 3 + 1] * p1 + Hb[i * 3 + 2] * p2;
      }
    }
    return y;
  }

  // First direction from the residual in r: p = z = M^-1 r, and this thread's part of rz = r.z and rr = r.r.  The caller sums them
  // (sum2) and publishes p: after the sum's barrier where P still holds something that is being read, before it otherwise.
  __device__ __forceinline__ void direction(double& rz, double& rr) {
    rz = 0.0;
    rr = 0.0;
#pragma unroll
    for (int k = 0; k < EPT; ++k) {
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        p[k][i] = Mi[k][i * 3] * r[k][0] + Mi[k][i * 3 + 1] * r[k][1] + Mi[k][i * 3 + 2] * r[k][2];   // z = M^-1 r
        rz += r[k][i] * p[k][i];
        rr += r[k][i] * r[k][i];
      }
    }
  }

  __device__ __forceinline__ void sum2(double& a, double& b) { block_sum2<NW>(a, b, redB, lane, wave); }

  // The iterations after the first direction: advances x, r, p and P until rr <= rtol2 * ref2, max_iter or pAp <= 0 (`bad`); rr is
  // the last r.r.  Returns the number of iterations.  Three barriers each: P complete, pAp, (rz, rr).
  template <class Block>
  __device__ __forceinline__ int iterate(const Block& block, double rz, double& rr, double ref2, double rtol2, int max_iter, bool& bad) {
    int iters = 0;
    for (int it = 0; it < max_iter; ++it) {
      __syncthreads();                                   // P complete
      Vec3 Ap[EPT];
      double pAp = 0.0;
#pragma unroll
      for (int k = 0; k < EPT; ++k) {
        Ap[k] = apply(block, k);
#pragma unroll
        for (int i = 0; i < 3; ++i) pAp += p[k][i] * Ap[k].v[i];
      }
      pAp = block_sum<NW>(pAp, redA, lane, wave);
      iters = it + 1;
      if (!(pAp > 0.0)) {
        bad = true;
        break;
      }
      const double alpha = rz / pAp;
      double rz_new = 0.0;
      rr = 0.0;
      double z[EPT][3];
#pragma unroll
      for (int k = 0; k < EPT; ++k) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          x[k][i] += alpha * p[k][i];
          r[k][i] -= alpha * Ap[k].v[i];
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          z[k][i] = Mi[k][i * 3] * r[k][0] + Mi[k][i * 3 + 1] * r[k][1] + Mi[k][i * 3 + 2] * r[k][2];
          rz_new += r[k][i] * z[k][i];
          rr += r[k][i] * r[k][i];
        }
      }
      sum2(rz_new, rr);
      if (rr <= rtol2 * ref2) break;
      const double beta = rz_new / rz;
      rz = rz_new;
#pragma unroll
      for (int k = 0; k < EPT; ++k) {
        if (act[k]) {
#pragma unroll
          for (int i = 0; i < 3; ++i) {
            p[k][i] = z[k][i] + beta * p[k][i];
            P[slot[k] * n + 3 * el[k] + i] = p[k][i];
          }
        }
      }
    }
    return iters;
  }
};

// Stationary corrector: A_N(theta) x = b|_N from x = 0, so r = b and no operator apply in front of the first iteration.
// info [nmark][2] = iterations, |r| / |b| (0 for b = 0; -1: pAp <= 0).
template <int EPT, int BT>
__global__ __launch_bounds__(BT) void k_hood_pcg(Tmpl t, int S, const int* __restrict__ nbr, int Q, QVecE th,
                                                 const int* __restrict__ marked, const double* __restrict__ A_diag,
                                                 const double* __restrict__ A_cpl, const double* __restrict__ D_corr,
                                                 const double* __restrict__ bvec, double* __restrict__ corr,
                                                 double rtol2, int max_iter, double* __restrict__ info) {
  extern __shared__ double lds[];
  const int n = t.n, ii = marked[blockIdx.x];
  const auto block = [&](int slot, int kk, int e, int bidx, double Hb[9]) {
    return hood_block(t, S, nbr, Q, th, A_diag, A_cpl, D_corr, ii, slot, kk, e, bidx, Hb);
  };
  HoodPcg<EPT, BT> c;
  c.template setup<(EPT > 1)>(t, nbr, ii, lds, block);      // (the determinant form of the re-read instantiations: see inv3)
  __syncthreads();      // P is zero before the first direction goes into it
#pragma unroll
  for (int k = 0; k < EPT; ++k) {
    if (c.act[k]) {
      const double* bs = bvec + (long)c.kk[k] * n + 3 * c.el[k];
#pragma unroll
      for (int i = 0; i < 3; ++i) c.r[k][i] = bs[i];
    }
  }
  double rz, rr;
  c.direction(rz, rr);
  c.publish(c.p);
  c.sum2(rz, rr);
  const double rr0 = rr;
  int iters = 0;
  bool bad = false;
  if (rr0 > 0.0) iters = c.iterate(block, rz, rr, rr0, rtol2, max_iter, bad);
#pragma unroll
  for (int k = 0; k < EPT; ++k) {
    if (c.act[k] && c.slot[k] == 2) {
      double* out = corr + (long)blockIdx.x * n + 3 * c.el[k];
#pragma unroll
      for (int i = 0; i < 3; ++i) out[i] = c.x[k][i];
    }
  }
  if (threadIdx.x == 0) {
    info[2 * blockIdx.x] = (double)iters;
    info[2 * blockIdx.x + 1] = bad ? -1.0 : (rr0 > 0.0 ? sqrt(rr / rr0) : 0.0);
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Parabolic counterpart: the corrector TRAJECTORY of every marked neighbourhood,
//   (M_N + dt A_N(theta)) x_{k+1} = M_N x_k + dt sum_j phi[k+1][j] b_j|_N,   x_0 = 0,   k = 0 .. nt-1,
// one workgroup per marked subdomain for all nt steps.  M_N is the P1 element mass (t.mass9, block diagonal: M x_k is thread-local),
// so the step operator H = dt A_N + M_N has the sparsity of A_N and the same four blocks per element.  Every step is a PCG
// warm-started at x_k: x and r stay in registers, the search direction lives in LDS; the first residual of a step stages x
// through that same LDS array (one extra operator apply).  Stop rule |r| <= rtol |rhs| (lrbms_fom_implicit_euler); a step whose
// right-hand side is exactly zero keeps x_{k+1} = x_k.

// step-operator block `bidx` of an element: dt * (theta-weighted block) (+ the element mass on the diagonal block)
__device__ inline int euler_block(const Tmpl& t, int S, const int* __restrict__ nbr, int Q, const QVecE& th,
                                  const double* __restrict__ A_diag, const double* __restrict__ A_cpl,
                                  const double* __restrict__ D_corr, double dt, int ii, int slot, int kk, int e, int bidx, double Hb[9]) {
  const int sb = hood_block(t, S, nbr, Q, th, A_diag, A_cpl, D_corr, ii, slot, kk, e, bidx, Hb);
  if (sb < 0) return sb;
  if (bidx == 0) {
    // dt * block + mass in one rounding, written out: left to the compiler, the product is fused into the sum only where bidx is
    // a compile-time constant, so the rounding of the diagonal blocks would follow the unrolling of the caller's loop over the blocks
    const double* m = t.mass9 + (long)e * 9;
#pragma unroll
    for (int i = 0; i < 9; ++i) Hb[i] = fma(Hb[i], dt, m[i]);
  } else {
#pragma unroll
    for (int i = 0; i < 9; ++i) Hb[i] *= dt;
  }
  return sb;
}

// info [nmark][2] = iterations summed over the steps, worst final |r| / |rhs| of a step (-1: pAp <= 0, the trajectory ended there).
template <int EPT, int BT>
__global__ __launch_bounds__(BT) void k_hood_euler(Tmpl t, int S, const int* __restrict__ nbr, int Q, QVecE th,
                                                   const int* __restrict__ marked, const double* __restrict__ A_diag,
                                                   const double* __restrict__ A_cpl, const double* __restrict__ D_corr,
                                                   const double* __restrict__ bK, int K, const double* __restrict__ phi, double dt,
                                                   int nt, double* __restrict__ corr, double rtol2, int max_iter,
                                                   double* __restrict__ info) {
  extern __shared__ double lds[];
  constexpr int NW = BT / 64;
  const int n = t.n, ii = marked[blockIdx.x];
  const auto block = [&](int slot, int kk, int e, int bidx, double Hb[9]) {
    return euler_block(t, S, nbr, Q, th, A_diag, A_cpl, D_corr, dt, ii, slot, kk, e, bidx, Hb);
  };
  HoodPcg<EPT, BT> c;
  c.template setup<false>(t, nbr, ii, lds, block);

  int iters = 0;
  bool bad = false;
  double worst = 0.0;
  for (int step = 0; step < nt; ++step) {
    if (!bad) {
      // right-hand side M x_k + dt sum_j phi[step + 1][j] b_j, kept in r
      const double* ph = phi + (long)(step + 1) * K;
      double ref2 = 0.0;
#pragma unroll
      for (int k = 0; k < EPT; ++k) {
        if (c.act[k]) {
          const double* m = t.mass9 + (long)c.el[k] * 9;
          double f[3] = {0.0, 0.0, 0.0};
          for (int j = 0; j < K; ++j) {
            const double w = ph[j];
            const double* bs = bK + ((long)j * S + c.kk[k]) * n + 3 * c.el[k];
#pragma unroll
            for (int i = 0; i < 3; ++i) f[i] += w * bs[i];
          }
#pragma unroll
          for (int i = 0; i < 3; ++i) {
            c.r[k][i] = m[i * 3] * c.x[k][0] + m[i * 3 + 1] * c.x[k][1] + m[i * 3 + 2] * c.x[k][2] + dt * f[i];
            ref2 += c.r[k][i] * c.r[k][i];
          }
        }
      }
      ref2 = block_sum<NW>(ref2, c.redA, c.lane, c.wave);
      if (ref2 > 0.0) {
        // first residual of the warm start: r = rhs - H x_k, x_k staged through P
        c.publish(c.x);
        __syncthreads();
#pragma unroll
        for (int k = 0; k < EPT; ++k) {
          const Vec3 Hx = c.apply(block, k);
#pragma unroll
          for (int i = 0; i < 3; ++i) c.r[k][i] -= Hx.v[i];
        }
        double rz, rr;
        c.direction(rz, rr);
        c.sum2(rz, rr);          // (its barrier: every read of x in P is done)
        c.publish(c.p);
        if (rr > rtol2 * ref2) iters += c.iterate(block, rz, rr, ref2, rtol2, max_iter, bad);
        if (!bad) worst = fmax(worst, sqrt(rr / ref2));
      }
      __syncthreads();      // redA / redB are free again and every read of P is done before the next step writes either
    }
    // x_{k+1} restricted to ii: column `step` of corr [nmark][n][nt] (a trajectory that ended on pAp <= 0 repeats its last state)
#pragma unroll
    for (int k = 0; k < EPT; ++k) {
      if (c.act[k] && c.slot[k] == 2) {
        double* out = corr + ((long)blockIdx.x * n + 3 * c.el[k]) * nt + step;
#pragma unroll
        for (int i = 0; i < 3; ++i) out[(long)i * nt] = c.x[k][i];
      }
    }
  }
  if (threadIdx.x == 0) {
    info[2 * blockIdx.x] = (double)iters;
    info[2 * blockIdx.x + 1] = bad ? -1.0 : worst;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Host side.  What both exports hand to a kernel; the right-hand side is a `const double*` b (stationary) or an EulerRhs.
struct HoodCall {
  int Q, nmark;
  const double *A_diag, *A_cpl, *D_corr;
  double* corr;
  double rtol;
  int max_iter;
  double* info_dev;   // work: info [nmark][2], then marked
  int* marked_dev;    // (filled with th by the shared launch_local_correction)
  QVecE th;
};

struct EulerRhs {
  const double *bK, *phi;
  int K, nt;
  double dt;
};

template <int EPT, int BT, class Rhs>
void launch_hood(lrbms_ctx* ctx, const HoodCall& c, const Rhs& rhs, hipStream_t st) {
  const size_t lds = sizeof(double) * (5 * (size_t)ctx->t.n + 3 * (BT / 64));
  if constexpr (std::is_same_v<Rhs, EulerRhs>)
    hipLaunchKernelGGL((k_hood_euler<EPT, BT>), dim3(c.nmark), dim3(BT), lds, st, ctx->t, ctx->S, ctx->nbr, c.Q, c.th, c.marked_dev,
                       c.A_diag, c.A_cpl, c.D_corr, rhs.bK, rhs.K, rhs.phi, rhs.dt, rhs.nt, c.corr, c.rtol * c.rtol, c.max_iter,
                       c.info_dev);
  else
    hipLaunchKernelGGL((k_hood_pcg<EPT, BT>), dim3(c.nmark), dim3(BT), lds, st, ctx->t, ctx->S, ctx->nbr, c.Q, c.th, c.marked_dev,
                       c.A_diag, c.A_cpl, c.D_corr, rhs, c.corr, c.rtol * c.rtol, c.max_iter, c.info_dev);
}

// The arguments both exports range-check alike (each adds its own and its own message).
bool hood_range_ok(int nmark, int Q, int max_iter, double rtol) { return nmark >= 1 && Q >= 1 && Q <= 8 && max_iter >= 1 && rtol > 0.0; }

// What both exports do after their range check: the remaining refusals (nothing is launched or copied before the last of them),
// theta and the upload of `marked`, the one (EPT, BT) ladder of both kernels, the read-back of info [nmark][2] (into `info` if given)
// and the verdict, every ratio in [0, rtol] or `miss`.  The refusals are written once, under the stationary export's name, where
// tests/test_corrector_iterates_host.py reads them and the ladder; the Euler export renames them (as_euler).
template <class Rhs>
int launch_local_correction(lrbms_ctx* ctx, HoodCall& c, const double* theta, const int32_t* marked, const Rhs& rhs, double* info,
                            const char* miss, hipStream_t st) {
  const int nmark = c.nmark, nel = 5 * ctx->t.nT;
  for (int m = 0; m < nmark; ++m) {
    if (marked[m] < 0 || marked[m] >= ctx->S) return lrbms_fail(ctx, LRBMS_E_INVALID, "local_correction_solve: marked index out of range");
    // the operator blocks of the WHOLE neighbourhood must be on this rank (a sharded discretization runs its corrector
    // problems on a context whose local set is its local + halo subdomains)
    for (int slot = 0; slot < 5; ++slot)
      if (ctx->nbr_host[(size_t)marked[m] * 5 + slot] >= ctx->S)
        return lrbms_fail(ctx, LRBMS_E_INVALID, "local_correction_solve: the neighbourhood of a marked subdomain is not assembled on this rank");
  }
  if ((size_t)5 * ctx->t.n * sizeof(double) + 1024 > 160 * 1024)
    return lrbms_fail(ctx, LRBMS_E_INVALID, "local_correction_solve: neighbourhood does not fit in LDS");
  if (nel > 8192) return lrbms_fail(ctx, LRBMS_E_INVALID, "local_correction_solve: template too large");
  for (int q = 0; q < 8; ++q) c.th.v[q] = q < c.Q ? theta[q] : 0.0;
  c.marked_dev = reinterpret_cast<int*>(c.info_dev + 2 * (size_t)nmark);
  LRBMS_HIP_CHECK(ctx, hipMemcpyAsync(c.marked_dev, marked, sizeof(int) * (size_t)nmark, hipMemcpyHostToDevice, st));
  if (nel <= 640)
    launch_hood<1, 640>(ctx, c, rhs, st);
  else if (nel <= 1024)
    launch_hood<1, 1024>(ctx, c, rhs, st);
  else if (nel <= 2048)
    launch_hood<2, 1024>(ctx, c, rhs, st);
  else if (nel <= 4096)
    launch_hood<4, 1024>(ctx, c, rhs, st);
  else if (nel <= 8192)
    launch_hood<8, 1024>(ctx, c, rhs, st);
  LRBMS_LAUNCH_CHECK(ctx);
  std::vector<double> host(2 * (size_t)nmark);
  LRBMS_HIP_CHECK(ctx, hipMemcpyAsync(host.data(), c.info_dev, sizeof(double) * 2 * (size_t)nmark, hipMemcpyDeviceToHost, st));
  LRBMS_HIP_CHECK(ctx, hipStreamSynchronize(st));
  bool ok = true;
  for (int m = 0; m < nmark; ++m) {
    if (info) {
      info[2 * m] = host[2 * m];
      info[2 * m + 1] = host[2 * m + 1];
    }
    const double rel = host[2 * m + 1];
    if (!(rel >= 0.0) || rel > c.rtol) ok = false;
  }
  return ok ? LRBMS_OK : lrbms_fail(ctx, LRBMS_E_NOT_CONVERGED, miss);
}

// A refusal of the shared part under the Euler export's name.
int as_euler(lrbms_ctx* ctx, int rc) {
  const std::string from = "local_correction_solve:";
  if (rc != LRBMS_OK && ctx->err.compare(0, from.size(), from) == 0) ctx->err.replace(0, from.size(), "local_correction_euler:");
  return rc;
}

}  // namespace

int64_t local_correction_work_size(lrbms_ctx* ctx, int nmark) {
  (void)ctx;
  return 3 * (int64_t)nmark + 8;
}

int64_t local_correction_euler_work_size(lrbms_ctx* ctx, int nmark) { return local_correction_work_size(ctx, nmark); }

int launch_local_correction(lrbms_ctx* ctx, int Q, const double* theta, int nmark, const int32_t* marked, const double* A_diag,
                            const double* A_cpl, const double* D_corr, const double* b, double* work, double* corr, double rtol,
                            int max_iter, double* info, hipStream_t st) {
  if (!hood_range_ok(nmark, Q, max_iter, rtol))
    return lrbms_fail(ctx, LRBMS_E_INVALID, "local_correction_solve: bad nmark / Q / max_iter / rtol");
  HoodCall c{Q, nmark, A_diag, A_cpl, D_corr, corr, rtol, max_iter, work, nullptr, {}};
  return launch_local_correction(ctx, c, theta, marked, b, info,
                                 "local_correction_solve: CG did not reach rtol (or the operator is not SPD)", st);
}

// The corrector trajectories of the parabolic enrichment (k_hood_euler).  phi [nt + 1][K] device, row k = time of step k; corr
// [nmark][n][nt], step fastest.
int launch_local_correction_euler(lrbms_ctx* ctx, int Q, int K, const double* theta, double dt, int nt, int nmark,
                                  const int32_t* marked, const double* A_diag, const double* A_cpl, const double* D_corr,
                                  const double* bK, const double* phi, double* work, double* corr, double rtol, int max_iter,
                                  double* info, hipStream_t st) {
  if (!hood_range_ok(nmark, Q, max_iter, rtol) || K < 1 || K > 64 || nt < 1 || !(dt > 0.0))
    return lrbms_fail(ctx, LRBMS_E_INVALID, "local_correction_euler: bad nmark / Q / K / nt / dt / max_iter / rtol");
  HoodCall c{Q, nmark, A_diag, A_cpl, D_corr, corr, rtol, max_iter, work, nullptr, {}};
  return as_euler(ctx, launch_local_correction(ctx, c, theta, marked, EulerRhs{bK, phi, K, nt, dt}, info,
                                               "local_correction_euler: CG did not reach rtol in a step (or the operator is not SPD)", st));
}
