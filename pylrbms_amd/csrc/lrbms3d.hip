// 3D / P2 hot path (BASELINE.json config 5) for gfx950: C ABI of include/lrbms3d_hip.h.  This file holds the context and the
// mesh upload, the offline assembly, the pass, the estimator and the full-order solvers with their parabolic side.  The reduced
// solvers live in online3d.hip, affine sources in sources3d.hip and online enrichment in enrich3d.hip, with lrbms3d_dev.h between
// the four files.  Other files call launch_fom_block_inverse, launch_fom_add_mass and launch_reduce1 of this file, and
// dense_spd_inverse: this file owns the rocBLAS handle of the context.
//
// Kuhn triangulation: every element is a translate of one of six reference tetrahedra, so every local integral is a
// contraction of coefficient samples with a reference table (pylrbms_amd/grid3d.py builds the tables on the host, once):
//     block[e][c] = sum_k sample[e][k] * TABLE[type(e)][k][c].
// The pass (lrbms3_project_estimate) is built from one MFMA kernel template, k3_pg<KIND>: G = sum_items X^T (L Y) with the
// element-local apply L Y and the projection both on the fp64 matrix cores, operands straight from global memory (no LDS
// staging, no VALU arithmetic in the loop), one wave per item, one workgroup per (subdomain, operator).  Images of a NEIGHBOUR's
// basis live on the side faces / side nodes of the target subdomain only: they are returned as factors (Rb, Yb, Dp, Xab, As, Cn)
// and the estimate kernel consumes the factors (header).
#include "lrbms3d_dev.h"
#include "lrbms_pod.h"

using namespace lrbms3;

namespace {

// ------------------------------------------------------------------------------------------------- offline assembly
__device__ inline double contract(const double* __restrict__ smp, const double* __restrict__ tab, int K, int C, int c) {
  double acc = 0.0;
  for (int k = 0; k < K; ++k) acc += smp[k] * tab[(long)k * C + c];
  return acc;
}

// f2 = ||f||^2, ceps = min lambda_hat * kmin per subdomain: one workgroup, fixed-order tree
__global__ __launch_bounds__(256) void k3_scalars(T3 t, const double* __restrict__ f_smp, const double* __restrict__ lhat,
                                                  double* __restrict__ f2, double* __restrict__ ceps) {
  __shared__ double sa[256], sb[256];
  const int s = blockIdx.x, tid = threadIdx.x;
  double acc = 0.0, mn = INFINITY;
  for (int e = tid; e < t.nT; e += 256) {
    const double* rf = f_smp + ((long)s * t.nT + e) * t.f_stride;
    const double* rh = lhat + ((long)s * t.nT + e) * t.hat_stride;
    for (int k = 0; k < t.nB; ++k) {
      acc += t.WB[k] * rf[k] * rf[k];
      mn = fmin(mn, rh[k]);
    }
  }
  sa[tid] = acc;
  sb[tid] = mn;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) {
      sa[tid] += sa[tid + w];
      sb[tid] = fmin(sb[tid], sb[tid + w]);
    }
    __syncthreads();
  }
  if (tid == 0) {
    f2[s] = sa[0];
    ceps[s] = sb[0] * t.kmin;
  }
}

// Products and estimator operators on the matrix cores.  For the elements of ONE type the contraction
//     out[e][c] = sum_k W(e, k) TABLE[type][k][c]
// is a GEMM of the sample rows with the reference table: A operand = W (lane: element li, quadrature point lk), B operand = the
// table chunk staged in LDS once per workgroup (64 elements = 4 waves x 16), accumulators = 16 elements x 16 entries per tile.
// (The first version had one workgroup per element re-read the whole 173 KB table from L2 and divide per term: 15.8 ms at
// config 5.)  OP: 0 ebar (W = lambda_bar), 1 A_aa pair (W = lambda_q lambda_q' / lambda_hat), 2 A_ab (W = lambda_q / lambda_hat,
// orientation sign of column f at the store), 3 B_bb (W = 1 / lambda_hat, signs of row and column).
constexpr int ASM_KC = 32;        // quadrature points per staged table chunk

//   4 rhs b (W = f at rule B, table w |T| phi_i), 5 int_T f (W = f at rule C, table = the weights), 6 diagonal block of the SWIPDG
//   system (K = volume rule + 4 faces x (inner-face table | Dirichlet table), the weight of the table that does not apply to the
//   face set to zero), 7 block towards the neighbour across face `fq2` (inner: A_diag slot 1 + f; coupling face: A_cpl; zero else).
//   8 / 9 the same two for the LOCAL ENERGY PRODUCT (block_swipdg.py:651-677): penalty parts of the face tables only, every face of
//   the subdomain boundary (coupling or physical) a Dirichlet face with the inside coefficient, no coupling blocks; the sample is
//   sum_q theta_bar_q lambda_q (every term is linear in lambda; theta_bar [Q] on the device through `lhat`).
template <int OP, int NCT>
__global__ __launch_bounds__(256) void k3_asm(T3 t, int Q, int q, int q2, const double* __restrict__ lam, const double* __restrict__ lbar,
                                              const double* __restrict__ lhat, double* __restrict__ out, double* __restrict__ out_mirror) {
  __shared__ double Ts[ASM_KC][NCT * 16 + 4];
  constexpr int C = OP == 2 ? 40 : (OP == 3 ? 16 : (OP == 4 ? 10 : (OP == 5 ? 1 : 100)));
  const int ty = blockIdx.x % 6, grp = blockIdx.x / 6, s = blockIdx.y;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, lk = lane >> 4;
  const int ncube = t.nT / 6;
  const int cube = grp * 64 + wave * 16 + li;                        // this lane's element (A operand row)
  const int e = (cube < ncube ? cube : ncube - 1) * 6 + ty;
  const int fq = q2;                                                 // OP 7: the face
  const int K = OP == 0 || OP == 4 ? t.nB : (OP == 6 || OP == 8 ? t.nA + 8 * t.nFs : (OP == 7 || OP == 9 ? t.nFs : t.nC));
  const double* tab;
  if (OP == 0) tab = t.TE + (long)ty * K * C;
  if (OP == 1) tab = t.TAA + (long)ty * K * C;
  if (OP == 2) tab = t.TAB + (long)ty * K * C;
  if (OP == 3) tab = t.TB + (long)ty * K * C;
  if (OP == 4) tab = t.TPH + (long)ty * K * C;
  if (OP == 5) tab = t.WC;
  if (OP == 6) tab = t.TSD + (long)ty * K * C;
  if (OP == 7) tab = t.TFn + ((long)(ty * 4 + fq) * K) * C;
  if (OP == 8) tab = t.TSP + (long)ty * K * C;
  if (OP == 9) tab = t.TPn + ((long)(ty * 4 + fq) * K) * C;
  const long se = (long)s * t.nT + e;
  // OP 0: lambda_bar; 1-3: lambda_hat at rule C; 4 / 5: f at rule B / C (passed as lbar)
  const double* w0 = OP == 0 ? lbar + se * t.nB : (OP == 4 ? lbar + se * t.f_stride : (OP == 5 ? lbar + se * t.f_stride + t.nB
                                                                                        : lhat + se * t.hat_stride + t.nB));
  const double* rec = lam + (((long)q * t.S_ext + s) * t.nT + e) * t.lam_stride;                   // lambda_q record of the element
  const double* w1 = rec + t.o_c;                                                                  // ... at rule C
  const double* w2 = lam + (((long)q2 * t.S_ext + s) * t.nT + e) * t.lam_stride + t.o_c;
  bool bnd[4] = {false, false, false, false};                        // OP 6 / 7: face on the physical boundary
  if (OP == 6 || OP == 7) {
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      const int nb = t.nb_elem[e * 4 + f];
      bnd[f] = nb < 0 && ((t.phys[s] >> (-(nb + 1))) & 1);
    }
  }
  if (OP == 8 || OP == 9) {          // local product: every face of the subdomain boundary is a Dirichlet face
#pragma unroll
    for (int f = 0; f < 4; ++f) bnd[f] = t.nb_elem[e * 4 + f] < 0;
  }
  // OP 8 / 9: lambda at mu_bar = sum_q theta_bar_q lambda_q at point `off` of the element's records
  auto lam_bar = [&](int off) {
    double v = 0.0;
    for (int qq = 0; qq < Q; ++qq) v += lhat[qq] * lam[(((long)qq * t.S_ext + s) * t.nT + e) * t.lam_stride + off];
    return v;
  };
  d4 acc[NCT];
#pragma unroll
  for (int j = 0; j < NCT; ++j) acc[j] = (d4){0.0, 0.0, 0.0, 0.0};
  for (int k0 = 0; k0 < K; k0 += ASM_KC) {
    __syncthreads();
    for (int i = tid; i < ASM_KC * NCT * 16; i += 256) {
      const int kk = i / (NCT * 16), c = i - kk * NCT * 16;
      Ts[kk][c] = (k0 + kk < K && c < C) ? tab[(long)(k0 + kk) * C + c] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < ASM_KC / 4; ++ks) {
      const int k = k0 + 4 * ks + lk;
      double w = 0.0;
      if (k < K) {
        if (OP == 0 || OP == 4 || OP == 5) w = w0[k];
        else if (OP == 1) w = w1[k] * w2[k] / w0[k];
        else if (OP == 2) w = w1[k] / w0[k];
        else if (OP == 3) w = 1.0 / w0[k];
        else if (OP == 6) {
          if (k < t.nA) {
            w = rec[k];
          } else {                       // face f: nFs points against the inner-face table, then the same points against the Dirichlet table
            const int kf = k - t.nA, f = kf / (2 * t.nFs), r2 = kf - f * 2 * t.nFs, dir = r2 >= t.nFs, pt = dir ? r2 - t.nFs : r2;
            const bool bf = f == 0 ? bnd[0] : (f == 1 ? bnd[1] : (f == 2 ? bnd[2] : bnd[3]));
            w = (bf == (dir != 0)) ? rec[t.o_fs + f * t.nFs + pt] : 0.0;
          }
        } else if (OP == 8) {
          if (k < t.nA) {
            w = lam_bar(k);
          } else {
            const int kf = k - t.nA, f = kf / (2 * t.nFs), r2 = kf - f * 2 * t.nFs, dir = r2 >= t.nFs, pt = dir ? r2 - t.nFs : r2;
            const bool bf = f == 0 ? bnd[0] : (f == 1 ? bnd[1] : (f == 2 ? bnd[2] : bnd[3]));
            w = (bf == (dir != 0)) ? lam_bar(t.o_fs + f * t.nFs + pt) : 0.0;
          }
        } else if (OP == 9) {
          const bool bf = fq == 0 ? bnd[0] : (fq == 1 ? bnd[1] : (fq == 2 ? bnd[2] : bnd[3]));
          w = bf ? 0.0 : lam_bar(t.o_fs + fq * t.nFs + k);
        } else {
          const bool bf = fq == 0 ? bnd[0] : (fq == 1 ? bnd[1] : (fq == 2 ? bnd[2] : bnd[3]));
          w = bf ? 0.0 : rec[t.o_fs + fq * t.nFs + k];
        }
      }
#pragma unroll
      for (int j = 0; j < NCT; ++j) acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(w, Ts[4 * ks + lk][j * 16 + li], acc[j], 0, 0, 0);
    }
  }
  // D layout: lane holds elements lk + 4 r of the wave's 16, entry j * 16 + li
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int cb = grp * 64 + wave * 16 + lk + 4 * r;
    if (cb >= ncube) continue;
    const int eo = cb * 6 + ty;
    const long so = (long)s * t.nT + eo;
#pragma unroll
    for (int j = 0; j < NCT; ++j) {
      const int c = j * 16 + li;
      if (c >= C) continue;
      double v = acc[j][r];
      if (OP == 2) v *= (double)sgn3(t, s, eo, c & 3);
      if (OP == 3) v *= (double)(sgn3(t, s, eo, c >> 2) * sgn3(t, s, eo, c & 3));
      if (OP == 6) {
        out[(((long)q * t.S + s) * t.nT + eo) * 500 + c] = v;
      } else if (OP == 8) {
        out[((long)s * t.nT + eo) * 500 + c] = v;
      } else if (OP == 9) {
        out[((long)s * t.nT + eo) * 500 + (1 + fq) * 100 + c] = t.nb_elem[eo * 4 + fq] >= 0 ? v : 0.0;
      } else if (OP == 7) {
        const int nb = t.nb_elem[eo * 4 + fq];
        out[(((long)q * t.S + s) * t.nT + eo) * 500 + (1 + fq) * 100 + c] = nb >= 0 ? v : 0.0;
        if (nb < 0) {
          const int side = -(nb + 1);
          out_mirror[((((long)q * t.S + s) * 6 + side) * t.ncf + t.face_pos[eo * 4 + fq]) * 100 + c] = ((t.phys[s] >> side) & 1) ? 0.0 : v;
        }
      } else {
        out[so * C + c] = v;
        if (OP == 1 && out_mirror) out_mirror[so * C + c] = v;
      }
    }
  }
}

__global__ __launch_bounds__(64) void k3_assemble_flux(T3 t, const double* __restrict__ lam, double* __restrict__ Cf) {
  const int e = blockIdx.x, s = blockIdx.y, q = blockIdx.z, c = threadIdx.x;
  if (c >= 40) return;
  const int f = c / 10, i = c - f * 10;
  const int ty = t.elem_type[e];
  const int nb = t.nb_elem[e * 4 + f];
  const bool bnd = nb < 0 && ((t.phys[s] >> (-(nb + 1))) & 1);
  const double* lf = lam + (((long)q * t.S_ext + s) * t.nT + e) * t.lam_stride + t.o_ff + f * t.nFf;
  const double* tab = (bnd ? t.TCb : t.TC) + ((long)(ty * 4 + f) * t.nFf) * 10;
  Cf[(((long)q * t.S_ext + s) * t.nT + e) * 40 + c] = contract(lf, tab, t.nFf, 10, i);
}

// ------------------------------------------------------------------------------------------------- pass: preparation
// R_self [S][n_rt][QN]: RT0 flux image of the own basis on the own faces;  Rb [S][nbf][QN]: the neighbour's share on the side faces.
// One wave per row: the row's elements, orientation and the ten flux coefficients per (element, q) are wave-uniform and come
// through the scalar cache; the only vector-memory instructions are the loads of the basis rows (the address unit, not the
// HBM, bounds these kernels).
constexpr int FLUX_R = 1;     // rows per wave and step (4 rows with their loads grouped was measured: slower)
// rows a wave handles one after the other (measured at config 5, FLUX_LOOP 1 / 4 / 8 / 16: k3_flux 362 / 381 / 387 / 398 us -- it is bound
// by L2 traffic, every element's rows are read by its four faces; NODE_LOOP 1 / 4 / 8 / 16: k3_node_avg 232 / 192 / 192 / 198 us)
#ifndef FLUX_LOOP
#define FLUX_LOOP 1
#endif
#ifndef NODE_LOOP
#define NODE_LOOP 4
#endif

// The same decode for a pass restricted to a list of subdomains (lrbms3_pass_set_subset): the chunks of 8 are formed over the cnt
// POSITIONS of the list and the subdomain is list[position]; every stride and every neighbour lookup keeps using the subdomain.
// list == nullptr (a kernel argument: the branch is wave-uniform): no restriction, position == subdomain, cnt == t.S.
__device__ inline bool xcd_block_list(int nblk, int cnt, const int* __restrict__ list, int& xblk, int& s) {
  if (!xcd_block(nblk, cnt, xblk, s)) return false;
  if (list) s = list[s];
  return true;
}

__global__ __launch_bounds__(256) void k3_flux(T3 t, int Q, int N, int rbeg, int rend, const int* __restrict__ list, int cnt,
                                               const double* __restrict__ V, const double* __restrict__ Cf, double* __restrict__ Rs,
                                               double* __restrict__ Rb) {
  const int QN = Q * N, nrows = rend;          // rows [rbeg, rend) of [own faces | side faces]
  int s, xblk;
  if (!xcd_block_list((rend - rbeg + 4 * FLUX_R * FLUX_LOOP - 1) / (4 * FLUX_R * FLUX_LOOP), cnt, list, xblk, s)) return;
  const int lane = threadIdx.x & 63, half = lane >> 5, jl = lane & 31;
  for (int rep = 0; rep < FLUX_LOOP; ++rep) {      // a wave lives for FLUX_LOOP rows: these sweeps are bound by the wave launch rate
  const int row0 = __builtin_amdgcn_readfirstlane(rbeg + ((xblk * FLUX_LOOP + rep) * 4 + (threadIdx.x >> 6)) * FLUX_R);
  if (row0 >= nrows) return;
  // The (<= 2) elements of a face are dealt to the two halves of the wave: lanes 0..31 take the first, lanes 32..63 the second,
  // lane = basis column.  Every basis row is loaded once per face (ten instead of twenty vector-memory instructions), both affine
  // components are formed in the lane from wave-uniform coefficients, and the halves meet through one lane exchange.
  const double* c0[FLUX_R];
  const double* c1[FLUX_R];
  double sgh[FLUX_R];
  long vrow[FLUX_R];
  double* dst[FLUX_R];
  bool on[FLUX_R];
#pragma unroll
  for (int r = 0; r < FLUX_R; ++r) {
    const int row = row0 + r < nrows ? row0 + r : nrows - 1;
    on[r] = row0 + r < nrows;
    int es[2], fs[2], ss[2], sg[2];
    if (row < t.nrt) {
      es[0] = t.rt_e0[row]; fs[0] = t.rt_f0[row]; es[1] = t.rt_e1[row]; fs[1] = t.rt_f1[row];
      ss[0] = ss[1] = s;
      sg[0] = sgn3(t, s, es[0], fs[0]);
      sg[1] = es[1] >= 0 ? sgn3(t, s, es[1], fs[1]) : 0;
    } else {
      const int sf = row - t.nrt;
      const int t2 = t.nbr[s * 7 + side_slot(sf / t.ncf)];
      es[0] = t.side_elem_out[sf]; fs[0] = t.side_face_out[sf]; es[1] = -1; fs[1] = 0;
      ss[0] = ss[1] = t2;
      sg[0] = sg[1] = 0;
      if (t2 >= 0 && es[0] >= 0) sg[0] = t.tsign[es[0] * 4 + fs[0]];      // a coupling face of the neighbour: its template orientation
      else es[0] = -1;
    }
    if (es[0] < 0) ss[0] = 0, es[0] = 0, fs[0] = 0;                        // nothing to add: sign 0, any valid address
    if (es[1] < 0) ss[1] = ss[0], es[1] = es[0], fs[1] = fs[0];
    c0[r] = Cf + ((long)ss[0] * t.nT + es[0]) * 40 + fs[0] * 10;
    c1[r] = Cf + ((long)ss[1] * t.nT + es[1]) * 40 + fs[1] * 10;
    sgh[r] = (double)(half ? sg[1] : sg[0]);
    vrow[r] = half ? ((long)ss[1] * t.n + es[1] * 10) : ((long)ss[0] * t.n + es[0] * 10);
    dst[r] = row < t.nrt ? Rs + ((long)s * t.nrt + row) * QN : Rb + ((long)s * t.nbf + row - t.nrt) * QN;
  }
  const long qstride = (long)t.S_ext * t.nT * 40;
  for (int j0 = 0; j0 < N; j0 += 32) {
    const int j = j0 + jl, jc = j < N ? j : N - 1;
    double vv[FLUX_R][10];
#pragma unroll
    for (int r = 0; r < FLUX_R; ++r) {
      const double* v = V + vrow[r] * N + jc;
#pragma unroll
      for (int i = 0; i < 10; ++i) vv[r][i] = v[(long)i * N];
    }
#pragma unroll
    for (int r = 0; r < FLUX_R; ++r)
      for (int q = 0; q < Q; ++q) {
        const double* a0 = c0[r] + q * qstride;
        const double* a1 = c1[r] + q * qstride;
        double s0 = 0.0, s1 = 0.0;          // both coefficient rows are wave-uniform (scalar loads); the lane keeps its half's sum
#pragma unroll
        for (int i = 0; i < 10; ++i) {
          s0 += a0[i] * vv[r][i];
          s1 += a1[i] * vv[r][i];
        }
        const double acc = (half ? s1 : s0) * sgh[r];
        const double other = __shfl_xor(acc, 32);
        if (half == 0 && j < N && on[r]) dst[r][q * N + j] = acc + other;
      }
  }
  }
}

// (Measured and dropped, round 3: the own faces from element chunks staged in LDS -- 24 elements per workgroup, rows and flux
// coefficients loaded once with 16-byte loads, only the faces towards a later chunk read their second element from global memory:
// 268 + 70 us (side faces) against 363 us for this kernel, but the PASS went from 2.19 to 2.29 ms: with 73 KB of LDS and 128 VGPRs
// per workgroup the sweep no longer fits beside the MFMA kernels of the other two chains, and hiding under them is worth more than
// the 25 us.)
// Avg [S][n_nodes][N]: own share of the Oswald node average (0 on the physical boundary: the interpolant vanishes there);
// As [S][6][nvs][N]: the neighbours' shares at the side nodes.  One wave per node, DoF lists through the scalar cache.
__global__ __launch_bounds__(256) void k3_node_avg(T3 t, int N, int rbeg, int rend, const int* __restrict__ list, int cnt,
                                                   const double* __restrict__ V, double* __restrict__ Avg, double* __restrict__ As) {
  int s, xblk;
  if (!xcd_block_list((rend - rbeg + 4 * NODE_LOOP - 1) / (4 * NODE_LOOP), cnt, list, xblk, s)) return;          // rows [rbeg, rend) of [own nodes | side nodes]
  const int j = threadIdx.x & 63;
  const int jc = j < N ? j : N - 1;
  const int phys = t.phys[s];
  for (int rep = 0; rep < NODE_LOOP; ++rep) {
  const int row = __builtin_amdgcn_readfirstlane(rbeg + (xblk * NODE_LOOP + rep) * 4 + (threadIdx.x >> 6));
  if (row >= rend) return;
  int p0 = 0, p1 = 0, node, src = s;
  const int* list;
  if (row < t.nnodes) {
    node = row;
    list = t.node_dofs;
    if (!(t.node_mask[node] & phys)) p0 = t.node_ptr[row], p1 = t.node_ptr[row + 1];
  } else {
    const int sp = row - t.nnodes;
    node = t.side_nodes[sp];
    src = t.nbr[s * 7 + side_slot(sp / t.nvs)];
    list = t.sn_dofs;
    if (node >= 0 && src >= 0 && !(t.node_mask[node] & phys)) p0 = t.sn_ptr[sp], p1 = t.sn_ptr[sp + 1];
  }
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  if (p1 > p0) {
    const double* v = V + (long)src * t.n * N + jc;
    int p = p0;
    for (; p + 3 < p1; p += 4) {
      a0 += v[(long)list[p] * N];
      a1 += v[(long)list[p + 1] * N];
      a2 += v[(long)list[p + 2] * N];
      a3 += v[(long)list[p + 3] * N];
    }
    for (; p < p1; ++p) a0 += v[(long)list[p] * N];
    a0 = ((a0 + a1) + (a2 + a3)) / (double)t.node_count[node];
  }
  if (j < N) {
    if (row < t.nnodes) Avg[((long)s * t.nnodes + row) * N + j] = a0;
    else As[((long)s * 6 * t.nvs + row - t.nnodes) * N + j] = a0;
  }
  }
}

// ------------------------------------------------------------------------------------------------- pass: projections
enum { G_SYS = 0, G_AAA = 1, G_NC = 2, G_AB = 3, G_BB = 4, G_CPL = 6 };

struct GA {
  T3 t;
  int Q, N;
  const double *V, *A_diag, *A_cpl, *ebar, *Aaa, *Aab, *Bbb, *Rs, *Avg;
  double* out;
  double* Zb;   // NC: rows of E W_self at the boundary DoFs [S][nbd][N]
  double *out2, *out3;     // BB: G_rdd [S][QN][QN], r_fd [S][QN] (accumulated beside G_bb: they share every operand)
  const double* bdiv;
  const double* b;        // SYS: right-hand side [S][n]; rhs_red = V^T b rides on the X operands of the q = 0 blocks
  double* out4;           // SYS: rhs_red [S][N]
  double *Yb, *Dp, *Xab;  // BB: rows of B R_self and |T| div div R_self at the side faces; AB: A_ab^T V at the side faces
  int ksplit;             // > 1: the items of a (subdomain, operator) are dealt to ksplit workgroups, partial results go to `part`
  double* part;           //      [batch][ksplit][pg_part_size] and k3_pg_combine sums them in a fixed order
  const int* list;        // restricted pass (lrbms3_pass_set_subset): the nlist subdomains the launch covers; nullptr: all, nlist = t.S
  int nlist;
};

// ------------------------------------------------------------------------------------------------- pass: MFMA pipeline
// G = sum_items X^T (L Y), everything on the matrix cores, operands straight from global memory (L2 / L1 resident):
//   Z  = L Y      L [mz x ky] element block as the A operand (lane: row l&15, k l>>4), Y rows gathered as the B operand
//   G += X^T Z    the accumulator layout of Z (lane: rows (l>>4) + 4 r, column l&15) IS the B-operand layout of k-step r,
//                 so Z never leaves the registers; X rows as the A operand
// One wave per item (element / side face), NW waves per workgroup = one (subdomain, operator); the waves' tiles are summed in a
// fixed order through the LDS at the end.  RT x CT output tiles of 16 x 16 per wave.
template <int KIND> struct PGT {};
template <> struct PGT<G_SYS> { static constexpr int MZ = 10, KY = 50; };
template <> struct PGT<G_AAA> { static constexpr int MZ = 10, KY = 10; };
template <> struct PGT<G_NC> { static constexpr int MZ = 10, KY = 10; };
template <> struct PGT<G_CPL> { static constexpr int MZ = 10, KY = 10; };
template <> struct PGT<G_AB> { static constexpr int MZ = 4, KY = 10; };    // contracted through the 4 faces: W = A_ab^T V_e first
template <> struct PGT<G_BB> { static constexpr int MZ = 4, KY = 4; };

// side-face index (side * ncf + pos) of face f of element e, or -1; `has`: the neighbour across that side exists
__device__ inline int side_face_of(const T3& t, int s, int e, int f, bool& has) {
  const int nb = t.nb_elem[e * 4 + f];
  has = false;
  if (nb >= 0) return -1;
  const int side = -(nb + 1);
  has = t.nbr[s * 7 + side_slot(side)] >= 0;
  return side * t.ncf + t.face_pos[e * 4 + f];
}

constexpr int pg_max_threads(int tiles) { return tiles <= 4 ? 1024 : (tiles <= 8 ? 512 : 256); }   // VGPR budget 128 / 256 / 512

// Block id -> (subdomain, operator, part).  Workgroups are dealt round-robin to the 8 XCDs (each with its own L2); all operator
// blocks (and all parts) of one subdomain read the same basis rows, so they get ids that differ by multiples of 8 inside one chunk
// of 8 subdomains: same XCD, launched together.
template <int KIND>
struct PGBlock {
  int b, pb, s, q, q2, Mx, My, t2, side, part;      // pb: b with the POSITION in the list for the subdomain (partial tiles)
  double* out;
  __device__ bool decode(const GA& a, int x) {
    const T3& t = a.t;
    const int N = a.N, Q = a.Q, QN = Q * N, ks = a.ksplit;
    const int nops = KIND == G_SYS || KIND == G_AB ? Q : (KIND == G_AAA ? Q * (Q + 1) / 2 : (KIND == G_CPL ? 6 * Q : 1));
    const int chunk = x / (8 * nops * ks), within = x - chunk * 8 * nops * ks;
    const int op = (within >> 3) / ks, sx = chunk * 8 + (within & 7);
    part = (within >> 3) - op * ks;
    if (sx >= a.nlist) return false;
    pb = KIND == G_CPL ? ((op / 6) * a.nlist + sx) * 6 + op % 6 : op * a.nlist + sx;
    const int sr = a.list ? a.list[sx] : sx;          // (wave-uniform: a kernel argument)
    b = KIND == G_CPL ? ((op / 6) * t.S + sr) * 6 + op % 6 : op * t.S + sr;
    q = q2 = t2 = side = 0;
    if (KIND == G_SYS) {
      q = b / t.S; s = b - q * t.S; Mx = My = N;
      out = a.out + (((long)q * t.S + s) * 7 + 3) * N * N;
    } else if (KIND == G_CPL) {
      side = b % 6;
      const int qs = b / 6;
      q = qs / t.S; s = qs - q * t.S; Mx = My = N;
      t2 = t.nbr[s * 7 + side_slot(side)];
      out = a.out + (((long)q * t.S + s) * 7 + side_slot(side)) * N * N;
    } else if (KIND == G_AAA) {       // one block per pair q <= q2 (row-major); the block (q2, q) is the transpose
      int p = b / t.S;
      s = b - p * t.S; Mx = My = N;
      while (p >= Q - q) p -= Q - q, ++q;
      q2 = q + p;
      out = a.out + (((long)q * Q + q2) * t.S + s) * N * N;
    } else if (KIND == G_NC) {
      s = b; Mx = My = N;
      out = a.out + (long)b * N * N;
    } else if (KIND == G_AB) {
      q = b / t.S; s = b - q * t.S; Mx = N; My = QN;
      out = a.out + (long)b * N * QN;
    } else {
      s = b; Mx = My = QN;
      out = a.out + (long)b * QN * QN;
    }
    return true;
  }
};

// doubles of one partial result: the output matrix (BB: G_bb and G_rdd) plus one row (SYS: rhs_red, BB: r_fd)
template <int KIND>
__host__ __device__ inline long pg_part_size(int N, int QN) {
  return KIND == G_BB ? 2L * QN * QN + QN : (KIND == G_AB ? (long)N * QN : (KIND == G_SYS ? (long)N * N + N : (long)N * N));
}

__device__ inline double ld8(const double* base, unsigned byte_off) {   // uniform base + 32-bit lane offset: no 64-bit VALU
  return *reinterpret_cast<const double*>(reinterpret_cast<const char*>(base) + byte_off);
}

// On this chip the f64 MFMA stream of one wave and the VALU work of the other waves of the SIMD do not overlap (DESIGN.md
// section 5.1), so the address arithmetic per item is kept minimal: every operand address is (uniform base of the item) +
// (32-bit lane offset), and the lane offsets are (element term: one multiply per neighbour slot and item) + (lane constant
// computed once in front of the loop).  The K index of the apply is scheduled so that a k-step reads ONE neighbour slot:
// rows j = 0..3 and 4..7 of every slot as full steps, the rows 8, 9 of two slots paired into one step.
__device__ inline double2 ld16(const double* base, unsigned byte_off) {
  return *reinterpret_cast<const double2*>(reinterpret_cast<const char*>(base) + byte_off);
}

// WIDE (even tile counts and even N): lane li owns the adjacent output columns li * CT + ct (rows li * RT + rt) instead of
// ct * 16 + li, and the two full k-steps of a slot read the rows j = 2 lk and 2 lk + 1, so a lane's operands of two tiles / two
// k-steps are 16 contiguous bytes: half as many vector-memory instructions per item.  The address unit of a CU serves its four
// SIMDs at a fixed number of cycles per instruction, and with 45 eight-byte loads per 38 MFMAs it, not the matrix pipe, set
// the pace.
template <int KIND, int RT, int CT, bool WIDE>
__global__ __launch_bounds__(pg_max_threads(KIND == G_BB ? (RT > 2 ? 8 : 4) : RT * CT * (KIND == G_NC || KIND == G_SYS ? 2 : 1))) void k3_pg(GA a) {
  extern __shared__ double lds[];   // [RT * CT][256]
  constexpr int MZ = PGT<KIND>::MZ, KY = PGT<KIND>::KY, KR = (MZ + 3) / 4;
  constexpr int NG = KY == 50 ? 5 : 1;                       // neighbour slots whose rows the apply reads
  constexpr int KS = KY == 4 ? 1 : 2 * NG + (NG + 1) / 2;    // k-steps: 13 for SYS, 3 for the 10-row kinds, 1 for the 4-row kinds
  constexpr bool NCK = KIND == G_NC, FACEK = KIND == G_AB || KIND == G_BB;
  const T3& t = a.t;
  const int N = a.N, Q = a.Q, QN = Q * N;
  const int tid = threadIdx.x, lane = tid & 63, li = lane & 15, lk = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int NW = blockDim.x >> 6;
  PGBlock<KIND> B;
  if (!B.decode(a, blockIdx.x)) return;
  const int pb = B.pb, s = B.s, q = B.q, q2 = B.q2, Mx = B.Mx, My = B.My, t2 = B.t2, side = B.side, part = B.part;
  double* out = B.out;
  int nitems = KIND == G_CPL ? t.ncf : t.nT;
  if (KIND == G_CPL && t2 < 0) {        // no neighbour on that side: the block is zero (the combine kernel skips it too)
    if (part == 0)
      for (int i = tid; i < Mx * My; i += blockDim.x) out[i] = 0.0;
    return;
  }
  const double* Vs = a.V + (long)s * t.n * N;
  const double* Yb = KIND == G_CPL ? a.V + (long)t2 * t.n * N : Vs;
  const double* Av = a.Avg + (long)s * t.nnodes * N;
  const double* Rss = a.Rs + (long)s * t.nrt * QN;
  const double* Lall;               // element blocks of this (subdomain, operator): item e at Lall + e * LSTRIDE
  constexpr int LSTRIDE = KIND == G_SYS ? 500 : (KIND == G_AB ? 40 : (KIND == G_BB ? 16 : 100));
  if (KIND == G_SYS) Lall = a.A_diag + ((long)q * t.S + s) * t.nT * 500;
  if (KIND == G_AAA) Lall = a.Aaa + (((long)q * Q + q2) * t.S + s) * t.nT * 100;
  if (KIND == G_NC) Lall = a.ebar + (long)s * t.nT * 100;
  if (KIND == G_AB) Lall = a.Aab + ((long)q * t.S + s) * t.nT * 40;
  if (KIND == G_BB) Lall = a.Bbb + (long)s * t.nT * 16;
  if (KIND == G_CPL) Lall = a.A_cpl + (((long)q * t.S + s) * 6 + side) * t.ncf * 100;

  // ---- lane constants
  const unsigned rowb = (unsigned)N * 8u, erow = 10u * rowb;            // bytes per DoF row / per element of the basis slab
  const int lic = li < MZ ? li : MZ - 1;
  unsigned yc[KS][CT];        // Y: (row j of the step) * rowb + column
  unsigned lc[KS];            // L: offset inside the item's block(s)
  int sA[KS];                 // neighbour slot this lane reads in step k (lane constant)
  bool pad[KS];               // lane is K padding in this step
#pragma unroll
  for (int k = 0; k < KS; ++k) {
    int g, j;
    bool pd = false;
    if (KY == 4) {
      g = 0; j = lk;
    } else if (k < 2 * NG) {
      g = k >> 1; j = WIDE ? 2 * lk + (k & 1) : 4 * (k & 1) + lk;
    } else {                   // rows 8, 9 of slot gA (lanes lk < 2) and of slot gA + 1 (lanes lk >= 2)
      const int gA = 2 * (k - 2 * NG);
      g = lk < 2 ? gA : gA + 1;
      j = 8 + (lk & 1);
      if (g >= NG) g = gA, pd = true;
    }
    sA[k] = g; pad[k] = pd;
    if (KIND == G_SYS) lc[k] = 8u * (g * 100 + lic * 10 + j);
    else if (KIND == G_AB) lc[k] = 8u * (lic * 4 + j);
    else if (KIND == G_BB) lc[k] = 8u * (j * 4 + lic);                                        // symmetric: read transposed
    else lc[k] = 8u * (lic * 10 + j);
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      int col;
      if (WIDE) {              // pairs of columns stay inside the (even) row: the last pair is repeated for the padding lanes
        const int c0 = li * CT + (ct & ~1);
        col = (c0 + 1 < My ? c0 : My - 2) + (ct & 1);
      } else {
        const int col0 = ct * 16 + li;
        col = col0 < My ? col0 : My - 1;
      }
      yc[k][ct] = (FACEK ? 0u : (unsigned)j * rowb) + 8u * col;
    }
  }
  unsigned xc[KR][RT];
  bool xin[KR];
#pragma unroll
  for (int r = 0; r < KR; ++r) {
    const int row0 = 4 * r + lk;
    xin[r] = row0 < MZ;
    const int row = xin[r] ? row0 : MZ - 1;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      int col;
      if (WIDE) {
        const int c0 = li * RT + (rt & ~1);
        col = (c0 + 1 < Mx ? c0 : Mx - 2) + (rt & 1);
      } else {
        const int col0 = rt * 16 + li;
        col = col0 < Mx ? col0 : Mx - 1;
      }
      xc[r][rt] = (KIND == G_BB ? 0u : (unsigned)row * rowb) + 8u * col;
    }
  }
  const double* zero = t.zeros + lane;

  d4 acc[RT][CT];
#pragma unroll
  for (int i = 0; i < RT; ++i)
#pragma unroll
    for (int j = 0; j < CT; ++j) acc[i][j] = (d4){0.0, 0.0, 0.0, 0.0};

  // index tables of an item (fetched one item ahead): element, its neighbours (SYS), node / RT0 numbers of this lane's rows
  struct Idx {
    int e, eo;
    int nb[4], up[4];
    int aux[KR], auy[KR];
  };
  const int last = nitems - 1;
  auto load_idx = [&](int item, Idx& ix) {
    item = item < last ? item : last;
    if (KIND != G_CPL) item = t.order[item];          // element visited at this position of the traversal
    ix.e = item;
    ix.eo = 0;
    if (KIND == G_CPL) {
      const int sp = side * t.ncf + item;
      ix.e = t.side_elem[sp];
      // a padded position (a side with fewer faces than ncf) has zero blocks, but its operand rows are loaded all the same: take them
      // from the neighbour's element at position 0 of the side -- inside the cube layer, the only rows a halo slab is known to hold
      ix.eo = t.side_elem_out[ix.e >= 0 ? sp : side * t.ncf];
    }
    if (KIND == G_SYS) {
      const int4 v = *reinterpret_cast<const int4*>(t.nb_elem + item * 4);
      ix.nb[0] = v.x; ix.nb[1] = v.y; ix.nb[2] = v.z; ix.nb[3] = v.w;
      const int4 u = *reinterpret_cast<const int4*>(t.up_face + item * 4);
      ix.up[0] = u.x; ix.up[1] = u.y; ix.up[2] = u.z; ix.up[3] = u.w;
    }
#pragma unroll
    for (int r = 0; r < KR; ++r) {
      ix.aux[r] = 0;
      ix.auy[r] = 0;
      if (NCK) {
        const int row = 4 * r + lk;
        ix.aux[r] = t.dof_node[item * 10 + (row < 10 ? row : 9)];                      // node of X row 4 r + lk
        const int j = r < 2 ? (WIDE ? 2 * lk + r : 4 * r + lk) : 8 + (lk & 1);          // node of the Y row of k-step r
        ix.auy[r] = t.dof_node[item * 10 + j];
      }
    }
    if (FACEK) ix.aux[0] = t.elem_rt[item * 4 + lk];
  };

  // G_bb: second accumulator set (G_rdd, upper tile triangle like G_bb) and the r_fd row
  constexpr bool BBK = KIND == G_BB;
  d4 accd[BBK ? RT : 1][BBK ? CT : 1];
  double fd[BBK ? CT : 1];
  if constexpr (BBK) {
    static_assert(KIND != G_BB || RT == CT, "G_bb is square");
#pragma unroll
    for (int i = 0; i < RT; ++i)
#pragma unroll
      for (int j = 0; j < CT; ++j) accd[i][j] = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < CT; ++j) fd[j] = 0.0;
  }
  // B_sys: lane constants of the symmetric form (below); rhs_red accumulators of the q = 0 blocks
  double racc[KIND == G_SYS ? RT : 1];
#pragma unroll
  for (int i = 0; i < (KIND == G_SYS ? RT : 1); ++i) racc[i] = 0.0;
  unsigned sl_full, sy_full[2][CT], sl_rem, sy_rem[CT];
  if constexpr (KIND == G_SYS) {
    sl_full = 8u * (lic * 10 + (WIDE ? 2 * lk : lk));                 // rows j = 2 lk, 2 lk + 1 (one 16-byte load) / j = lk, 4 + lk
    sl_rem = 8u * (lic * 10 + 8 + (lk & 1));
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      int col;
      if (WIDE) {
        const int c0 = li * CT + (ct & ~1);
        col = (c0 + 1 < N ? c0 : N - 2) + (ct & 1);
      } else {
        const int col0 = ct * 16 + li;
        col = col0 < N ? col0 : N - 1;
      }
#pragma unroll
      for (int par = 0; par < 2; ++par) sy_full[par][ct] = (unsigned)(WIDE ? 2 * lk + par : 4 * par + lk) * rowb + 8u * col;
      sy_rem[ct] = (unsigned)(8 + (lk & 1)) * rowb + 8u * col;
    }
  }
  // G_ab: lane constants of its own form (below)
  unsigned abl[3], abv[3][RT];
  bool abpad[3];
  if constexpr (KIND == G_AB) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int j = k < 2 ? (WIDE ? 2 * lk + k : 4 * k + lk) : 8 + (lk & 1);
      abpad[k] = k == 2 && lk >= 2;
      abl[k] = 8u * (j * 4 + (li < 4 ? li : 3));            // A_ab[e][j][f = li]: rows f >= 4 of the product are never used
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
        int col;
        if (WIDE) {
          const int c0 = li * RT + (rt & ~1);
          col = (c0 + 1 < N ? c0 : N - 2) + (rt & 1);
        } else {
          const int col0 = rt * 16 + li;
          col = col0 < N ? col0 : N - 1;
        }
        abv[k][rt] = (unsigned)j * rowb + 8u * col;
      }
    }
  }

  // the items of this part: a contiguous range of the traversal
  const int plen = (nitems + a.ksplit - 1) / a.ksplit, pbeg = part * plen;
  const int pend = pbeg + plen < nitems ? pbeg + plen : nitems;
  double* P = a.ksplit > 1 ? a.part + ((long)pb * a.ksplit + part) * pg_part_size<KIND>(N, QN) : nullptr;
  Idx ix1, ix2;
  load_idx(pbeg + wave, ix1);
  for (int item0 = pbeg + wave; item0 < pend; item0 += NW) {
    const int item = item0 < last ? item0 : last;
    if constexpr (KIND == G_SYS) {
      // Symmetric form: A[e', e] = A[e, e']^T, so with H = sum_e V_e^T (1/2 A_ee V_e + sum_{e' > e} A[e, e'] V_e') the projection is
      // B = H + H^T (epilogue).  Per element only the diagonal block and the blocks towards the neighbours with the HIGHER index
      // are read (t.up_face, on average 1.75 of 3.5 inner faces): 55 % of the A_diag bytes and of the neighbour rows, and
      // 2 s + ceil(s / 2) k-steps for s = 1 + #upper slots instead of 13.  Slots are wave-uniform, skipped slots cost nothing.
      const int e = ix1.e;
      const double* Lb = Lall + (long)e * LSTRIDE;
      const unsigned ex = (unsigned)e * erow;
      const int nsl = 1 + (ix1.up[0] >= 0) + (ix1.up[1] >= 0) + (ix1.up[2] >= 0) + (ix1.up[3] >= 0);
      unsigned ebs[5], bos[5];
      ebs[0] = ex;
      bos[0] = 0u;
#pragma unroll
      for (int g = 1; g < 5; ++g) {
        const int f = ix1.up[g - 1], fc = f < 0 ? 0 : f;
        const int ee = fc == 0 ? ix1.nb[0] : (fc == 1 ? ix1.nb[1] : (fc == 2 ? ix1.nb[2] : ix1.nb[3]));
        ebs[g] = (unsigned)(f < 0 ? e : ee) * erow;
        bos[g] = f < 0 ? 0u : 800u * (1 + fc);
      }
      double lop[13], yv[CT][13], xop[RT][KR];
#pragma unroll
      for (int g = 0; g < 5; ++g) {
        if (g < nsl) {                                    // wave-uniform
          if (WIDE) {
            const double2 v = ld16(Lb, bos[g] + sl_full);
            lop[2 * g] = v.x;
            lop[2 * g + 1] = v.y;
          } else {
            lop[2 * g] = ld8(Lb, bos[g] + sl_full);
            lop[2 * g + 1] = ld8(Lb, bos[g] + sl_full + 32u);
          }
#pragma unroll
          for (int par = 0; par < 2; ++par)
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) {
              if (WIDE) {
                if ((ct & 1) == 0) {
                  const double2 v = ld16(Vs, ebs[g] + sy_full[par][ct]);
                  yv[ct][2 * g + par] = v.x;
                  yv[ct + 1 < CT ? ct + 1 : ct][2 * g + par] = v.y;
                }
              } else {
                yv[ct][2 * g + par] = ld8(Vs, ebs[g] + sy_full[par][ct]);
              }
            }
        }
      }
#pragma unroll
      for (int r = 0; r < 3; ++r) {                       // rows 8, 9 of slots 2 r (lanes lk < 2) and 2 r + 1 (lanes lk >= 2)
        if (2 * r < nsl) {
          const int gB = 2 * r + 1 < 5 ? 2 * r + 1 : 2 * r;
          const bool hasB = 2 * r + 1 < nsl;
          const unsigned eo = (lk < 2 || !hasB) ? ebs[2 * r] : ebs[gB];
          const unsigned bo = (lk < 2 || !hasB) ? bos[2 * r] : bos[gB];
          lop[10 + r] = (lk >= 2 && !hasB) ? *zero : ld8(Lb, bo + sl_rem);
#pragma unroll
          for (int ct = 0; ct < CT; ++ct) {
            if (WIDE) {
              if ((ct & 1) == 0) {
                const double2 v = ld16(Vs, eo + sy_rem[ct]);
                yv[ct][10 + r] = v.x;
                yv[ct + 1 < CT ? ct + 1 : ct][10 + r] = v.y;
              }
            } else {
              yv[ct][10 + r] = ld8(Vs, eo + sy_rem[ct]);
            }
          }
        }
      }
#pragma unroll
      for (int r = 0; r < KR; ++r)
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
          if (WIDE) {
            if ((rt & 1) == 0) {
              const double2 v = xin[r] ? ld16(Vs, ex + xc[r][rt]) : *reinterpret_cast<const double2*>(t.zeros);
              xop[rt][r] = v.x;
              xop[rt + 1 < RT ? rt + 1 : rt][r] = v.y;
            }
          } else {
            xop[rt][r] = xin[r] ? ld8(Vs, ex + xc[r][rt]) : *zero;
          }
        }
      double bv[KR];                                      // q = 0 (wave-uniform): the element's entries of b for rhs_red = V^T b
#pragma unroll
      for (int r = 0; r < KR; ++r) bv[r] = (q == 0 && xin[r]) ? a.b[(long)s * t.n + e * 10 + 4 * r + lk] : 0.0;
      load_idx(item0 + NW, ix2);
      ix1 = ix2;
      lop[0] *= 0.5;                                      // the diagonal block enters H with the factor 1/2
      lop[1] *= 0.5;
      lop[10] *= lk < 2 ? 0.5 : 1.0;
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        d4 z = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int g = 0; g < 5; ++g)
          if (g < nsl) {
            z = __builtin_amdgcn_mfma_f64_16x16x4f64(lop[2 * g], yv[ct][2 * g], z, 0, 0, 0);
            z = __builtin_amdgcn_mfma_f64_16x16x4f64(lop[2 * g + 1], yv[ct][2 * g + 1], z, 0, 0, 0);
          }
#pragma unroll
        for (int r = 0; r < 3; ++r)
          if (2 * r < nsl) z = __builtin_amdgcn_mfma_f64_16x16x4f64(lop[10 + r], yv[ct][10 + r], z, 0, 0, 0);
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
          for (int r = 0; r < KR; ++r) acc[rt][ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(xop[rt][r], z[r], acc[rt][ct], 0, 0, 0);
      }
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int r = 0; r < KR; ++r) racc[rt] += xop[rt][r] * bv[r];
      continue;
    }
    if constexpr (KIND == G_BB) {
      // Three operators of the four RT0 rows R_e of an element, one set of loads:
      //   G_bb  += R_e^T (B_bb R_e)                        apply (A operand B_bb, symmetric) + projection, upper tile triangle
      //   G_rdd += |T| (d^T R_e)^T (d^T R_e)               d_f = +-|f| / |T|: z1 = d^T R_e is ONE row, so the projection is a
      //                                                    k = 1 product of z1 with itself (lanes lk = 0 carry it)
      //   r_fd  += (int_T f) z1                            a VALU accumulation of the same row
      const int e = ix1.e;
      const double* Lb = Lall + (long)e * LSTRIDE;
      const unsigned rb = (unsigned)ix1.aux[0] * ((unsigned)QN * 8u);
      const int ty = t.elem_type[e];
      double dd[4];
#pragma unroll
      for (int f = 0; f < 4; ++f) dd[f] = sgn3(t, s, e, f) * t.divc[ty * 4 + f];
      const double bd = a.bdiv[(long)s * t.nT + e];
      const double lopB = ld8(Lb, 8u * (lk * 4 + (li < 4 ? li : 3)));
      double re[CT];
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        if (WIDE) {
          if ((ct & 1) == 0) {
            const double2 v = ld16(Rss, rb + yc[0][ct]);
            re[ct] = v.x;
            re[ct + 1 < CT ? ct + 1 : ct] = v.y;
          }
        } else {
          re[ct] = ld8(Rss, rb + yc[0][ct]);
        }
      }
      load_idx(item0 + NW, ix2);
      ix1 = ix2;
      const double dsel = lk == 0 ? dd[0] : (lk == 1 ? dd[1] : (lk == 2 ? dd[2] : dd[3]));
      const double l1 = li < 4 ? dsel : 0.0;              // A operand of z1: rows 0..3 = d^T (every k lane then holds the row)
      bool shas;
      const int sfi = side_face_of(t, s, e, lk, shas);    // this lane's face f = lk as a side face
      double zb[CT], z1r[CT], z1[CT];
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        const d4 z0 = (d4){0.0, 0.0, 0.0, 0.0};
        zb[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(lopB, re[ct], z0, 0, 0, 0)[0];      // rows f = lk of B_bb R_e
        z1r[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(l1, re[ct], z0, 0, 0, 0)[0];       // d^T R_e, replicated in the four k lanes
        z1[ct] = lk == 0 ? z1r[ct] : 0.0;                                                 // ... as a k = 1 operand
        fd[ct] += bd * z1[ct];
      }
      if (sfi >= 0) {      // side-face factors (read by the estimate): Yb = row of B R_self, Dp = |T| d_f (d^T R_self); 0 if no neighbour
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
          const int col = WIDE ? li * CT + ct : ct * 16 + li;
          if (col < My) {
            a.Yb[((long)s * t.nbf + sfi) * QN + col] = shas ? zb[ct] : 0.0;
            a.Dp[((long)s * t.nbf + sfi) * QN + col] = shas ? t.volume * dsel * z1r[ct] : 0.0;
          }
        }
      }
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
        const double a1 = t.volume * z1[rt];
#pragma unroll
        for (int ct = rt; ct < CT; ++ct) {
          acc[rt][ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(re[rt], zb[ct], acc[rt][ct], 0, 0, 0);
          accd[rt][ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, z1[ct], accd[rt][ct], 0, 0, 0);
        }
      }
      continue;
    }
    if constexpr (KIND == G_AB) {
      // G_ab[q] = sum_e V_e^T A_ab R_e = sum_e (A_ab^T V_e)^T R_e: contracted through the FOUR faces instead of the ten DoFs.
      //   W = A_ab^T V_e   [4 x N]    A operand A_ab^T (rows f), B operand the rows of V_e: 3 k-steps per row tile
      //   G += W^T R_e                 A operand = accumulator element 0 of W (lane: f = lk, i = li), B operand the four RT0 rows
      // 3 RT + RT CT = 14 MFMAs per element at config 5 instead of 28.
      const int e = ix1.e;
      const double* Lb = Lall + (long)e * LSTRIDE;
      const unsigned ex = (unsigned)e * erow, rb = (unsigned)ix1.aux[0] * ((unsigned)QN * 8u);
      bool shas;
      const int sfi = side_face_of(t, s, e, lk, shas);    // this lane's face f = lk as a side face
      double lop[3], vv[RT][3], re[CT];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        lop[k] = abpad[k] ? *zero : ld8(Lb, abl[k]);
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
          if (WIDE) {
            if ((rt & 1) == 0) {
              const double2 v = ld16(Vs, ex + abv[k][rt]);
              vv[rt][k] = v.x;
              vv[rt + 1 < RT ? rt + 1 : rt][k] = v.y;
            }
          } else {
            vv[rt][k] = ld8(Vs, ex + abv[k][rt]);
          }
        }
      }
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        if (WIDE) {
          if ((ct & 1) == 0) {
            const double2 v = ld16(Rss, rb + yc[0][ct]);
            re[ct] = v.x;
            re[ct + 1 < CT ? ct + 1 : ct] = v.y;
          }
        } else {
          re[ct] = ld8(Rss, rb + yc[0][ct]);
        }
      }
      load_idx(item0 + NW, ix2);
      ix1 = ix2;
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
        d4 z = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < 3; ++k) z = __builtin_amdgcn_mfma_f64_16x16x4f64(lop[k], vv[rt][k], z, 0, 0, 0);
        if (sfi >= 0) {        // side-face factor Xab_q = (A_ab^T V_e) at the face (0 if there is no neighbour)
          const int col = WIDE ? li * RT + rt : rt * 16 + li;
          if (col < N) a.Xab[(((long)q * t.S + s) * t.nbf + sfi) * N + col] = shas ? z[0] : 0.0;
        }
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) acc[rt][ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(z[0], re[ct], acc[rt][ct], 0, 0, 0);
      }
      continue;
    }
    // ---- operand loads of the item, all issued before the first MFMA (no arithmetic on loaded values here)
    const bool on = KIND != G_CPL || ix1.e >= 0;
    const int e = on ? ix1.e : 0;
    const double* Lb = Lall + (long)(KIND == G_CPL ? item : e) * LSTRIDE;
    unsigned eb[NG];                          // byte offset of the rows of the slot's element
    if (FACEK) {
      eb[0] = (unsigned)ix1.aux[0] * ((unsigned)QN * 8u);
    } else if (KIND == G_CPL) {
      eb[0] = (unsigned)ix1.eo * erow;
    } else {
      eb[0] = (unsigned)e * erow;
      if (KIND == G_SYS) {
#pragma unroll
        for (int g = 1; g < NG; ++g) {
          const int ee = ix1.nb[g - 1];
          eb[g] = (unsigned)(ee < 0 ? e : ee) * erow;     // side face: no inner neighbour, its block is zero
        }
      }
    }
    const unsigned ex = (unsigned)e * erow;
    double lop[KS], yv[CT][KS], xop[RT][KR];
    int dnode[NCK ? KS : 1];
    if (NCK) {
#pragma unroll
      for (int k = 0; k < KS; ++k) dnode[NCK ? k : 0] = ix1.auy[NCK ? k : 0];
    }
    double yav[NCK ? CT : 1][NCK ? KS : 1], xav[NCK ? RT : 1][NCK ? KR : 1];
    int bslot[NCK ? KR : 1];
#pragma unroll
    for (int k = 0; k < KS; ++k) {
      unsigned eo = eb[0];
      if (NG > 1) {
        if (k < 2 * NG) eo = eb[k >> 1];
        else eo = (lk < 2 || 2 * (k - 2 * NG) + 1 >= NG) ? eb[2 * (k - 2 * NG)] : eb[(2 * (k - 2 * NG) + 1) % NG];
      }
      if (WIDE && KY != 4 && k < 2 * NG) {          // full steps: rows j = 2 lk, 2 lk + 1 of the slot in one 16-byte load
        if ((k & 1) == 0) {
          const double2 v = on ? ld16(Lb, lc[k]) : *reinterpret_cast<const double2*>(t.zeros);
          lop[k] = v.x;
          lop[k + 1 < KS ? k + 1 : k] = v.y;
        }
      } else {
        lop[k] = (pad[k] || !on) ? *zero : ld8(Lb, lc[k]);
      }
      unsigned nd = 0;
      if (NCK) nd = (unsigned)dnode[NCK ? k : 0] * rowb;
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        if (WIDE) {
          if ((ct & 1) == 0) {
            const double2 v = ld16(FACEK ? Rss : Yb, eo + yc[k][ct]);
            yv[ct][k] = v.x;
            yv[ct + 1 < CT ? ct + 1 : ct][k] = v.y;
            if (NCK) {
              const double2 w = ld16(Av, nd + 8u * (yc[k][ct] % rowb / 8u));
              yav[NCK ? ct : 0][NCK ? k : 0] = w.x;
              yav[NCK ? (ct + 1 < CT ? ct + 1 : ct) : 0][NCK ? k : 0] = w.y;
            }
          }
        } else {
          yv[ct][k] = ld8(FACEK ? Rss : Yb, eo + yc[k][ct]);
          if (NCK) yav[NCK ? ct : 0][NCK ? k : 0] = ld8(Av, nd + 8u * (yc[k][ct] % rowb / 8u));
        }
      }
    }
#pragma unroll
    for (int r = 0; r < KR; ++r) {
      unsigned nd = 0;
      if (NCK) {
        nd = (unsigned)ix1.aux[r] * rowb;
        bslot[NCK ? r : 0] = t.dof_bslot[e * 10 + (4 * r + lk < MZ ? 4 * r + lk : MZ - 1)];
      }
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
        const unsigned off = (KIND == G_BB ? eb[0] : ex) + xc[r][rt];
        if (WIDE) {
          if ((rt & 1) == 0) {
            const double2 v = xin[r] ? ld16(KIND == G_BB ? Rss : Vs, off) : *reinterpret_cast<const double2*>(t.zeros);
            xop[rt][r] = v.x;
            xop[rt + 1 < RT ? rt + 1 : rt][r] = v.y;
            if (NCK) {
              const double2 w = xin[r] ? ld16(Av, nd + 8u * (xc[r][rt] % rowb / 8u)) : *reinterpret_cast<const double2*>(t.zeros);
              xav[NCK ? rt : 0][NCK ? r : 0] = w.x;
              xav[NCK ? (rt + 1 < RT ? rt + 1 : rt) : 0][NCK ? r : 0] = w.y;
            }
          }
        } else {
          xop[rt][r] = xin[r] ? ld8(KIND == G_BB ? Rss : Vs, off) : *zero;
          if (NCK) xav[NCK ? rt : 0][NCK ? r : 0] = xin[r] ? ld8(Av, nd + 8u * (xc[r][rt] % rowb / 8u)) : *zero;
        }
      }
    }
    load_idx(item0 + NW, ix2);
    ix1 = ix2;
    if (NCK) {
#pragma unroll
      for (int k = 0; k < KS; ++k)
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) yv[ct][k] -= yav[NCK ? ct : 0][NCK ? k : 0];
#pragma unroll
      for (int r = 0; r < KR; ++r)
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) xop[rt][r] -= xav[NCK ? rt : 0][NCK ? r : 0];
    }
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      d4 z = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int k = 0; k < KS; ++k) z = __builtin_amdgcn_mfma_f64_16x16x4f64(lop[k], yv[ct][k], z, 0, 0, 0);
      if (NCK) {      // rows of E W_self at boundary DoFs: the side-node factors Cn are summed from them (k3_side_nc)
        const int col = WIDE ? li * CT + ct : ct * 16 + li;
#pragma unroll
        for (int r = 0; r < KR; ++r) {
          const int row = 4 * r + lk;
          if (row < MZ && col < My && bslot[NCK ? r : 0] >= 0) a.Zb[((long)s * t.nbd + bslot[NCK ? r : 0]) * N + col] = z[r];
        }
      }
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int r = 0; r < KR; ++r) acc[rt][ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(xop[rt][r], z[r], acc[rt][ct], 0, 0, 0);
    }
  }
  if constexpr (BBK) {
    // fixed-order sum over the waves of both accumulator sets (upper tile triangle) and of the r_fd row, then the stores with the
    // mirrored tiles
    constexpr int NTRI = RT * (RT + 1) / 2;
    double* lfd = lds + 2 * NTRI * 256;
    for (int w = NW - 1; w > 0; --w) {
      __syncthreads();
      if (wave == w) {
        int tix = 0;
#pragma unroll
        for (int i = 0; i < RT; ++i)
#pragma unroll
          for (int j = i; j < CT; ++j, ++tix)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              lds[(tix * 4 + r) * 64 + lane] = acc[i][j][r];
              lds[((NTRI + tix) * 4 + r) * 64 + lane] = accd[i][j][r];
            }
#pragma unroll
        for (int j = 0; j < CT; ++j) lfd[j * 64 + lane] = fd[j];
      }
      __syncthreads();
      if (wave == w - 1) {
        int tix = 0;
#pragma unroll
        for (int i = 0; i < RT; ++i)
#pragma unroll
          for (int j = i; j < CT; ++j, ++tix)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              acc[i][j][r] += lds[(tix * 4 + r) * 64 + lane];
              accd[i][j][r] += lds[((NTRI + tix) * 4 + r) * 64 + lane];
            }
#pragma unroll
        for (int j = 0; j < CT; ++j) fd[j] += lfd[j * 64 + lane];
      }
    }
    if (wave == 0 && P) {                  // K-split: both matrices in full (mirrored) and the r_fd row as a partial result
#pragma unroll
      for (int i = 0; i < RT; ++i)
#pragma unroll
        for (int j = i; j < CT; ++j) {
          const int col = WIDE ? li * CT + j : j * 16 + li;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int row = WIDE ? (lk + 4 * r) * RT + i : i * 16 + lk + 4 * r;
            if (row < Mx && col < My) {
              P[(long)row * My + col] = acc[i][j][r];
              P[(long)QN * QN + (long)row * My + col] = accd[i][j][r];
              if (i != j) {
                P[(long)col * My + row] = acc[i][j][r];
                P[(long)QN * QN + (long)col * My + row] = accd[i][j][r];
              }
            }
          }
        }
      if (lk == 0) {
#pragma unroll
        for (int j = 0; j < CT; ++j) {
          const int col = WIDE ? li * CT + j : j * 16 + li;
          if (col < My) P[2L * QN * QN + col] = fd[j];
        }
      }
      return;
    }
    if (wave == 0) {
      double* o2 = a.out2 + (long)s * QN * QN;
#pragma unroll
      for (int i = 0; i < RT; ++i)
#pragma unroll
        for (int j = i; j < CT; ++j) {
          const int col = WIDE ? li * CT + j : j * 16 + li;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int row = WIDE ? (lk + 4 * r) * RT + i : i * 16 + lk + 4 * r;
            if (row < Mx && col < My) {
              out[(long)row * My + col] = acc[i][j][r];
              o2[(long)row * My + col] = accd[i][j][r];
              if (i != j) {
                out[(long)col * My + row] = acc[i][j][r];
                o2[(long)col * My + row] = accd[i][j][r];
              }
            }
          }
        }
      if (lk == 0) {
#pragma unroll
        for (int j = 0; j < CT; ++j) {
          const int col = WIDE ? li * CT + j : j * 16 + li;
          if (col < My) a.out3[(long)s * QN + col] = fd[j];
        }
      }
    }
    return;
  }
  // ---- fixed-order sum over the waves: acc_0 + (acc_1 + (... + acc_{NW-1}))
  for (int w = NW - 1; w > 0; --w) {
    __syncthreads();
    if (wave == w) {
#pragma unroll
      for (int i = 0; i < RT; ++i)
#pragma unroll
        for (int j = 0; j < CT; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r) lds[((i * CT + j) * 4 + r) * 64 + lane] = acc[i][j][r];
    }
    __syncthreads();
    if (wave == w - 1) {
#pragma unroll
      for (int i = 0; i < RT; ++i)
#pragma unroll
        for (int j = 0; j < CT; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[i][j][r] += lds[((i * CT + j) * 4 + r) * 64 + lane];
    }
  }
  if constexpr (KIND == G_SYS) {       // B = H + H^T through the LDS (Mx My <= RT CT 256 doubles)
    if (q == 0) {                      // rhs_red: sum over the four k lanes, then over the waves in a fixed order
      __shared__ double rsh[16][RT * 16];
      __syncthreads();
#pragma unroll
      for (int i = 0; i < RT; ++i) {
        double v = racc[i];
        v += __shfl_xor(v, 16);
        v += __shfl_xor(v, 32);
        if (lk == 0) rsh[wave][i * 16 + li] = v;
      }
      __syncthreads();
      if (wave == 0 && lk == 0) {
#pragma unroll
        for (int i = 0; i < RT; ++i) {
          double v = 0.0;
          for (int ww = 0; ww < NW; ++ww) v += rsh[ww][i * 16 + li];
          const int col = WIDE ? li * RT + i : i * 16 + li;
          if (col < N) (P ? P[(long)N * N + col] : a.out4[(long)s * N + col]) = v;
        }
      }
    }
    if (P) {                                // K-split: H itself is the partial result, the combine kernel forms H + H^T
      if (wave == 0) {
#pragma unroll
        for (int i = 0; i < RT; ++i)
#pragma unroll
          for (int j = 0; j < CT; ++j) {
            const int col = WIDE ? li * CT + j : j * 16 + li;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int row = WIDE ? (lk + 4 * r) * RT + i : i * 16 + lk + 4 * r;
              if (row < Mx && col < My) P[(long)row * My + col] = acc[i][j][r];
            }
          }
      }
      return;
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int i = 0; i < RT; ++i)
#pragma unroll
        for (int j = 0; j < CT; ++j) {
          const int col = WIDE ? li * CT + j : j * 16 + li;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int row = WIDE ? (lk + 4 * r) * RT + i : i * 16 + lk + 4 * r;
            if (row < Mx && col < My) lds[row * My + col] = acc[i][j][r];
          }
        }
    }
    __syncthreads();
    for (int i = tid; i < Mx * My; i += blockDim.x) {
      const int row = i / My, col = i - row * My;
      out[i] = lds[i] + lds[col * My + row];
    }
    return;
  }
  if (wave == 0 && P) {
#pragma unroll
    for (int i = 0; i < RT; ++i)
#pragma unroll
      for (int j = 0; j < CT; ++j) {
        const int col = WIDE ? li * CT + j : j * 16 + li;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = WIDE ? (lk + 4 * r) * RT + i : i * 16 + lk + 4 * r;
          if (row < Mx && col < My) P[(long)row * My + col] = acc[i][j][r];
        }
      }
    return;
  }
  if (wave == 0) {
    double* mirror = nullptr;       // AAA: block (q2, q) = transpose of block (q, q2)
    if (KIND == G_AAA && q != q2) mirror = a.out + (((long)q2 * Q + q) * t.S + s) * N * N;
#pragma unroll
    for (int i = 0; i < RT; ++i)
#pragma unroll
      for (int j = 0; j < CT; ++j) {
        const int col = WIDE ? li * CT + j : j * 16 + li;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = WIDE ? (lk + 4 * r) * RT + i : i * 16 + lk + 4 * r;
          if (row < Mx && col < My) {
            out[(long)row * My + col] = acc[i][j][r];
            if (mirror) mirror[(long)col * My + row] = acc[i][j][r];
          }
        }
      }
  }
}

// K-split: sum of the partial results of a (subdomain, operator) in the fixed order part = 0 .. ksplit - 1, then the epilogue of
// the kind (B_sys = H + H^T and rhs_red; mirrored A_aa block; G_bb, G_rdd, r_fd)
template <int KIND>
__global__ __launch_bounds__(256) void k3_pg_combine(GA a) {
  PGBlock<KIND> B;
  GA a1 = a;
  a1.ksplit = 1;
  if (!B.decode(a1, blockIdx.x)) return;
  const T3& t = a.t;
  const int N = a.N, Q = a.Q, QN = Q * N, ks = a.ksplit;
  if (KIND == G_CPL && B.t2 < 0) return;
  const long psz = pg_part_size<KIND>(N, QN);
  const double* P = a.part + (long)B.pb * ks * psz;
  const int Mx = B.Mx, My = B.My, nent = Mx * My;
  for (int i = threadIdx.x; i < nent; i += 256) {
    double v = 0.0;
    for (int p = 0; p < ks; ++p) v += P[p * psz + i];
    if (KIND == G_SYS) {
      const int row = i / My, col = i - row * My;
      double vt = 0.0;
      for (int p = 0; p < ks; ++p) vt += P[p * psz + (long)col * My + row];
      B.out[i] = v + vt;
    } else {
      B.out[i] = v;
      if (KIND == G_AAA && B.q != B.q2) {
        const int row = i / My, col = i - row * My;
        a.out[(((long)B.q2 * Q + B.q) * t.S + B.s) * N * N + (long)col * My + row] = v;
      }
      if (KIND == G_BB) {
        double v2 = 0.0;
        for (int p = 0; p < ks; ++p) v2 += P[p * psz + (long)QN * QN + i];
        a.out2[(long)B.s * QN * QN + i] = v2;
      }
    }
  }
  if (KIND == G_SYS && B.q == 0)
    for (int i = threadIdx.x; i < N; i += 256) {
      double v = 0.0;
      for (int p = 0; p < ks; ++p) v += P[p * psz + (long)N * N + i];
      a.out4[(long)B.s * N + i] = v;
    }
  if (KIND == G_BB)
    for (int i = threadIdx.x; i < QN; i += 256) {
      double v = 0.0;
      for (int p = 0; p < ks; ++p) v += P[p * psz + 2L * QN * QN + i];
      a.out3[(long)B.s * QN + i] = v;
    }
}

template <int KIND, int RT, int CT>
void launch_pg(const GA& a, int batch, int nw, hipStream_t st) {
  if (a.nlist <= 0) return;                                    // an empty list of a restricted pass: nothing to launch
  const int batch1 = batch / a.nlist * ((a.nlist + 7) / 8 * 8);     // whole chunks of 8 subdomains (PGBlock: XCD-aware block ids)
  batch = batch1 * a.ksplit;
  constexpr int maxt = pg_max_threads(KIND == G_BB ? (RT > 2 ? 8 : 4) : RT * CT * (KIND == G_NC || KIND == G_SYS ? 2 : 1));   // NC also holds the node averages of its operands; BB: two upper tile triangles
  if (nw * 64 > maxt) nw = maxt / 64;
  constexpr bool EVEN = RT % 2 == 0 && CT % 2 == 0;
  const size_t ldsb = sizeof(double) * (KIND == G_BB ? RT * (RT + 1) * 256 + CT * 64 : RT * CT * 256);   // BB: two upper triangles + r_fd
  if (EVEN && a.N % 2 == 0)
    hipLaunchKernelGGL((k3_pg<KIND, RT, CT, EVEN>), dim3(batch), dim3(64 * nw), ldsb, st, a);
  else
    hipLaunchKernelGGL((k3_pg<KIND, RT, CT, false>), dim3(batch), dim3(64 * nw), ldsb, st, a);
  if (a.ksplit > 1) hipLaunchKernelGGL((k3_pg_combine<KIND>), dim3(batch1), dim3(256), 0, st, a);
}

// tile shapes: square (rt == ct) for everything but AB, where ct = tiles of Q N >= rt = tiles of N (no AB (3, 4): rt = 3 means
// N > 32, so Q = 1 and ct = rt).  tests/test_dispatch_coverage3d.py checks that every listed shape is reachable and tested.
template <int KIND>
int dispatch_pg(const GA& a, int batch, int rt, int ct, int nw, hipStream_t st) {
#define PGCASE(R, C)                                 \
  if (rt == R && ct == C) {                          \
    launch_pg<KIND, R, C>(a, batch, nw, st);         \
    return 0;                                        \
  }
  if constexpr (KIND != G_AB) { PGCASE(1, 1) PGCASE(2, 2) PGCASE(3, 3) PGCASE(4, 4) }
  if constexpr (KIND == G_AB) { PGCASE(1, 1) PGCASE(1, 2) PGCASE(1, 3) PGCASE(1, 4) PGCASE(2, 2) PGCASE(2, 3) PGCASE(2, 4) PGCASE(3, 3) PGCASE(4, 4) }
#undef PGCASE
  return -1;
}

// Cn [S][nb][N] = -(P^T E W_self) at the boundary nodes: sum of the rows k3_pg<NC> left in Zb over the DoFs of the node.
// One wave per node, its slot list through the scalar cache.
__global__ __launch_bounds__(256) void k3_side_nc(T3 t, int N, const int* __restrict__ list, const double* __restrict__ Zb,
                                                  double* __restrict__ Cn) {
  const int s = list ? list[blockIdx.y] : blockIdx.y, c = threadIdx.x & 63;
  const int bn = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
  if (bn >= t.nb) return;
  const int cc = c < N ? c : N - 1;
  const double* z = Zb + (long)s * t.nbd * N + cc;
  const int p0 = t.bn_ptr[bn], p1 = t.bn_ptr[bn + 1];
  double a0 = 0.0, a1 = 0.0;
  int p = p0;
  for (; p + 1 < p1; p += 2) {
    a0 += z[(long)t.bn_slots[p] * N];
    a1 += z[(long)t.bn_slots[p + 1] * N];
  }
  if (p < p1) a0 += z[(long)t.bn_slots[p] * N];
  if (c < N) Cn[((long)s * t.nb + bn) * N + c] = -(a0 + a1);
}

// Restricted pass with padded side tables: the rows of Yb, Dp [S][nbf][QN] and Xab [Q][S][nbf][N] of the listed subdomains set to
// zero (the whole pass clears the three arrays by memset; the padded rows are written by no kernel).  One workgroup per subdomain.
__global__ __launch_bounds__(256) void k3_zero_side_rows(T3 t, int Q, int N, const int* __restrict__ list, double* __restrict__ Yb,
                                                         double* __restrict__ Dp, double* __restrict__ Xab) {
  const int s = list[blockIdx.x];
  const long nq = (long)t.nbf * Q * N, nx = (long)t.nbf * N;
  for (long i = threadIdx.x; i < nq; i += 256) {
    Yb[s * nq + i] = 0.0;
    Dp[s * nq + i] = 0.0;
  }
  for (int q = 0; q < Q; ++q)
    for (long i = threadIdx.x; i < nx; i += 256) Xab[((long)q * t.S + s) * nx + i] = 0.0;
}

// ------------------------------------------------------------------------------------------------- online: estimate
__device__ inline double block_sum(double v, double* red) {   // fixed-order tree over 256 threads; red [256]
  const int tid = threadIdx.x;
  __syncthreads();
  red[tid] = v;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) red[tid] += red[tid + w];
    __syncthreads();
  }
  return red[0];
}

__global__ __launch_bounds__(256) void k3_estimate(T3 t, int Q, int N, QV th, EA a) {
  extern __shared__ double lds[];
  const int s = blockIdx.x, tid = threadIdx.x, QN = Q * N;
  double* us = lds;                 // [7][N] coefficients on the neighbourhood (0 where no neighbour)
  double* ur = us + 7 * N;          // [QN]   theta_q u_self
  double* zf = ur + QN;             // [nbf]  flux of the neighbours on the side faces
  double* z = zf + t.nbf;           // [nb]   neighbours' share of the node averages
  double* red = z + t.nb;           // [256]
  for (int i = tid; i < 7 * N; i += 256) {
    const int s2 = t.nbr[s * 7 + i / N];
    us[i] = s2 >= 0 ? a.u[(long)s2 * N + i % N] : 0.0;
  }
  __syncthreads();
  const double* u0 = us + 3 * N;
  for (int i = tid; i < QN; i += 256) ur[i] = th.v[i / N] * u0[i % N];
  for (int sf = tid; sf < t.nbf; sf += 256) {
    const double* ua = us + side_slot(sf / t.ncf) * N;
    const double* r = a.Rb + ((long)s * t.nbf + sf) * QN;
    double acc = 0.0;
    for (int q = 0; q < Q; ++q) {
      double aq = 0.0;
      for (int j = 0; j < N; ++j) aq += r[q * N + j] * ua[j];
      acc += th.v[q] * aq;
    }
    zf[sf] = acc;
  }
  for (int bn = tid; bn < t.nb; bn += 256) {
    double acc = 0.0;
    for (int k = 0; k < 3; ++k) {
      const int sp = t.bnode_sides[bn * 3 + k];
      if (sp < 0) continue;
      const double* ua = us + side_slot(sp / t.nvs) * N;
      const double* r = a.As + ((long)s * 6 * t.nvs + sp) * N;
      for (int j = 0; j < N; ++j) acc += r[j] * ua[j];
    }
    z[bn] = acc;
  }
  __syncthreads();
  // ---- nonconformity
  double p_nc = 0.0;
  for (int r = tid; r < N; r += 256) {
    const double* g = a.G_nc + ((long)s * N + r) * N;
    double d = 0.0;
    for (int j = 0; j < N; ++j) d += g[j] * u0[j];
    p_nc += u0[r] * d;
  }
  for (int bn = tid; bn < t.nb; bn += 256) {
    const double* g = a.Cn + ((long)s * t.nb + bn) * N;
    double d = 0.0;
    for (int j = 0; j < N; ++j) d += g[j] * u0[j];
    p_nc += 2.0 * z[bn] * d;
  }
  for (int k = tid; k < t.nbel; k += 256) {
    const int e = t.bel_elem[k];
    const double* E = a.ebar + ((long)s * t.nT + e) * 100;
    double ze[10];
    for (int i = 0; i < 10; ++i) {
      const int bn = t.bel_bnode[k * 10 + i];
      ze[i] = bn >= 0 ? z[bn] : 0.0;
    }
    for (int i = 0; i < 10; ++i) {
      if (ze[i] == 0.0) continue;
      double d = 0.0;
      for (int j = 0; j < 10; ++j) d += E[i * 10 + j] * ze[j];
      p_nc += ze[i] * d;
    }
  }
  const double nc = block_sum(p_nc, red);
  // ---- flux terms
  double p_bb = 0.0, p_dd = 0.0, p_fd = 0.0, p_ab = 0.0, p_aa = 0.0;
  for (int r = tid; r < QN; r += 256) {
    const double* gb = a.G_bb + ((long)s * QN + r) * QN;
    const double* gd = a.G_rdd + ((long)s * QN + r) * QN;
    double db = 0.0, dd = 0.0;
    for (int j = 0; j < QN; ++j) {
      db += gb[j] * ur[j];
      dd += gd[j] * ur[j];
    }
    p_bb += ur[r] * db;
    p_dd += ur[r] * dd;
    p_fd += a.r_fd[(long)s * QN + r] * ur[r];
  }
  for (int r = tid; r < N; r += 256) {
    for (int q = 0; q < Q; ++q) {
      const double* g = a.G_ab + (((long)q * t.S + s) * N + r) * QN;
      double d = 0.0;
      for (int j = 0; j < QN; ++j) d += g[j] * ur[j];
      p_ab += th.v[q] * u0[r] * d;
      for (int q2 = 0; q2 < Q; ++q2) {
        const double* ga = a.G_aa + ((((long)q * Q + q2) * t.S + s) * N + r) * N;
        double da = 0.0;
        for (int j = 0; j < N; ++j) da += ga[j] * u0[j];
        p_aa += th.v[q] * th.v[q2] * u0[r] * da;
      }
    }
  }
  for (int sf = tid; sf < t.nbf; sf += 256) {
    const double zz = zf[sf];
    if (zz == 0.0) continue;
    const double* yb = a.Yb + ((long)s * t.nbf + sf) * QN;
    const double* dp = a.Dp + ((long)s * t.nbf + sf) * QN;
    double db = 0.0, dd = 0.0;
    for (int j = 0; j < QN; ++j) {
      db += yb[j] * ur[j];
      dd += dp[j] * ur[j];
    }
    p_bb += 2.0 * zz * db;
    p_dd += 2.0 * zz * dd;
    for (int q = 0; q < Q; ++q) {
      const double* xa = a.Xab + (((long)q * t.S + s) * t.nbf + sf) * N;
      double d = 0.0;
      for (int j = 0; j < N; ++j) d += xa[j] * u0[j];
      p_ab += th.v[q] * zz * d;
    }
  }
  for (int k = tid; k < t.nsel; k += 256) {
    const int e = t.sel_elem[k], ty = t.elem_type[e];
    const double* B = a.Bbb + ((long)s * t.nT + e) * 16;
    double ze[4], dv = 0.0;
    for (int f = 0; f < 4; ++f) {
      const int sf = t.sel_sf[k * 4 + f];
      ze[f] = sf >= 0 ? zf[sf] : 0.0;
      dv += sgn3(t, s, e, f) * t.divc[ty * 4 + f] * ze[f];
    }
    for (int f = 0; f < 4; ++f)
      for (int g = 0; g < 4; ++g) p_bb += ze[f] * B[f * 4 + g] * ze[g];
    p_dd += t.volume * dv * dv;
    p_fd += a.bdiv[(long)s * t.nT + e] * dv;
  }
  const double bb = block_sum(p_bb, red);
  const double dd = block_sum(p_dd, red);
  const double fd = block_sum(p_fd, red);
  const double ab = block_sum(p_ab, red);
  const double aa = block_sum(p_aa, red);
  if (tid == 0) {
    const double pi = 3.14159265358979323846;
    a.eta[s] = nc;
    a.eta[t.S + s] = (a.f2[s] - 2.0 * fd + dd) * (1.0 / (pi * pi)) / a.ceps[s] * a.hdiam * a.hdiam;
    a.eta[2 * t.S + s] = bb + 2.0 * ab + aa;
  }
}

// Batched form: MB = 8 parameters per workgroup pass.  Threads = (worker w = tid >> 3, parameter m = tid & 7): the eight
// parameter lanes of a worker read the same factor row (one address, broadcast) and their own coefficient column from LDS, so
// every projected operator and factor is read once per batch.  u [S_ext][N][nmu] (parameter fastest), eta [3][S][nmu].
constexpr int EST_MB = 8;
struct TB8 { double v[EST_MB][8]; };

// sum_j g[j] * u[j * 8]: a row of a projected operator (global) against a coefficient column in the LDS (parameter-fastest, 8 per
// row), for the eight parameter lanes of a worker (consecutive lanes, same g, same control flow).  The lanes would all load the
// same address -- 8 useful bytes per lane-group and instruction, and the address unit, not the memory, sets the pace -- so lane m
// loads entry j0 + m of every 8-entry chunk (all chunks first: n <= 64) and the group passes the values around by lane shuffles.
__device__ inline double dot_row8(const double* __restrict__ g, const double* u, int n) {
  const int lane = threadIdx.x & 63, m = lane & 7, base = lane & ~7;
  double mine[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) mine[c] = (c * 8 < n && c * 8 + m < n) ? g[c * 8 + m] : 0.0;
  double d = 0.0;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    if (c * 8 >= n) break;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const double gk = __shfl(mine[c], base + k);
      if (c * 8 + k < n) d += gk * u[(c * 8 + k) * 8];
    }
  }
  return d;
}

__global__ __launch_bounds__(256) void k3_estimate_batch(T3 t, int Q, int N, int nmu, int m0, TB8 th, EA a) {
  extern __shared__ double lds[];
  const int s = blockIdx.x, tid = threadIdx.x, w = tid >> 3, m = tid & 7, QN = Q * N, NWK = 32;
  const int mb = nmu - m0 < EST_MB ? nmu - m0 : EST_MB;      // parameters of this pass
  double* us = lds;                       // [7][N][8]
  double* ur = us + 7 * N * 8;            // [QN][8]
  double* zf = ur + QN * 8;               // [nbf][8]
  double* z = zf + t.nbf * 8;             // [nb][8]
  double* red = z + t.nb * 8;             // [256]
  for (int i = tid; i < 7 * N * 8; i += 256) {
    const int mm = i & 7, row = i >> 3, s2 = t.nbr[s * 7 + row / N];
    us[i] = (s2 >= 0 && mm < mb) ? a.u[((long)s2 * N + row % N) * nmu + m0 + mm] : 0.0;
  }
  __syncthreads();
  const double* u0 = us + 3 * N * 8 + m;          // own coefficients of parameter m: u0[j * 8]
  for (int i = tid; i < QN * 8; i += 256) {
    const int mm = i & 7, c = i >> 3;
    ur[i] = th.v[mm][c / N] * us[(3 * N + c % N) * 8 + mm];
  }
  for (int sf = w; sf < t.nbf; sf += NWK) {
    const double* ua = us + side_slot(sf / t.ncf) * N * 8 + m;
    const double* r = a.Rb + ((long)s * t.nbf + sf) * QN;
    double acc = 0.0;
    for (int q = 0; q < Q; ++q) {
      double aq = 0.0;
      aq = dot_row8(r + q * N, ua, N);
      acc += th.v[m][q] * aq;
    }
    zf[sf * 8 + m] = acc;
  }
  for (int bn = w; bn < t.nb; bn += NWK) {
    double acc = 0.0;
    for (int k = 0; k < 3; ++k) {
      const int sp = t.bnode_sides[bn * 3 + k];
      if (sp < 0) continue;
      const double* ua = us + side_slot(sp / t.nvs) * N * 8 + m;
      const double* r = a.As + ((long)s * 6 * t.nvs + sp) * N;
      acc += dot_row8(r, ua, N);
    }
    z[bn * 8 + m] = acc;
  }
  __syncthreads();
  const double* urm = ur + m;
  double p_nc = 0.0, p_bb = 0.0, p_dd = 0.0, p_fd = 0.0, p_ab = 0.0, p_aa = 0.0;
  for (int r = w; r < N; r += NWK) {
    const double* g = a.G_nc + ((long)s * N + r) * N;
    const double d = dot_row8(g, u0, N);
    p_nc += u0[r * 8] * d;
    for (int q = 0; q < Q; ++q) {
      const double* gab = a.G_ab + (((long)q * t.S + s) * N + r) * QN;
      const double dab = dot_row8(gab, urm, QN);
      p_ab += th.v[m][q] * u0[r * 8] * dab;
      for (int q2 = 0; q2 < Q; ++q2) {
        const double* ga = a.G_aa + ((((long)q * Q + q2) * t.S + s) * N + r) * N;
        const double da = dot_row8(ga, u0, N);
        p_aa += th.v[m][q] * th.v[m][q2] * u0[r * 8] * da;
      }
    }
  }
  for (int bn = w; bn < t.nb; bn += NWK) {
    const double* g = a.Cn + ((long)s * t.nb + bn) * N;
    const double d = dot_row8(g, u0, N);
    p_nc += 2.0 * z[bn * 8 + m] * d;
  }
  for (int k = w; k < t.nbel; k += NWK) {
    const int e = t.bel_elem[k];
    const double* E = a.ebar + ((long)s * t.nT + e) * 100;
    double ze[10];
    for (int i = 0; i < 10; ++i) {
      const int bn = t.bel_bnode[k * 10 + i];
      ze[i] = bn >= 0 ? z[bn * 8 + m] : 0.0;
    }
    for (int i = 0; i < 10; ++i) {
      double d = 0.0;
      for (int j = 0; j < 10; ++j) d += E[i * 10 + j] * ze[j];
      p_nc += ze[i] * d;
    }
  }
  for (int r = w; r < QN; r += NWK) {
    const double* gb = a.G_bb + ((long)s * QN + r) * QN;
    const double* gd = a.G_rdd + ((long)s * QN + r) * QN;
    const double db = dot_row8(gb, urm, QN), dd = dot_row8(gd, urm, QN);
    p_bb += urm[r * 8] * db;
    p_dd += urm[r * 8] * dd;
    p_fd += a.r_fd[(long)s * QN + r] * urm[r * 8];
  }
  for (int sf = w; sf < t.nbf; sf += NWK) {
    const double zz = zf[sf * 8 + m];
    const double* yb = a.Yb + ((long)s * t.nbf + sf) * QN;
    const double* dp = a.Dp + ((long)s * t.nbf + sf) * QN;
    const double db = dot_row8(yb, urm, QN), dd = dot_row8(dp, urm, QN);
    p_bb += 2.0 * zz * db;
    p_dd += 2.0 * zz * dd;
    for (int q = 0; q < Q; ++q) {
      const double* xa = a.Xab + (((long)q * t.S + s) * t.nbf + sf) * N;
      const double d = dot_row8(xa, u0, N);
      p_ab += th.v[m][q] * zz * d;
    }
  }
  for (int k = w; k < t.nsel; k += NWK) {
    const int e = t.sel_elem[k], ty = t.elem_type[e];
    const double* B = a.Bbb + ((long)s * t.nT + e) * 16;
    double ze[4], dv = 0.0;
    for (int f = 0; f < 4; ++f) {
      const int sf = t.sel_sf[k * 4 + f];
      ze[f] = sf >= 0 ? zf[sf * 8 + m] : 0.0;
      dv += sgn3(t, s, e, f) * t.divc[ty * 4 + f] * ze[f];
    }
    for (int f = 0; f < 4; ++f)
      for (int g = 0; g < 4; ++g) p_bb += ze[f] * B[f * 4 + g] * ze[g];
    p_dd += t.volume * dv * dv;
    p_fd += a.bdiv[(long)s * t.nT + e] * dv;
  }
  // sums over the 32 workers per parameter, fixed order
  double tot[6];
  const double part[6] = {p_nc, p_bb, p_dd, p_fd, p_ab, p_aa};
  for (int k = 0; k < 6; ++k) {
    __syncthreads();
    red[tid] = part[k];
    __syncthreads();
    double acc = 0.0;
    if (tid < 8)
      for (int ww = 0; ww < NWK; ++ww) acc += red[ww * 8 + tid];
    tot[k] = acc;
  }
  if (tid < mb) {
    const double pi = 3.14159265358979323846;
    const long o = (long)s * nmu + m0 + tid;
    a.eta[o] = tot[0];
    a.eta[(long)t.S * nmu + o] = (a.f2[s] - 2.0 * tot[3] + tot[2]) * (1.0 / (pi * pi)) / a.ceps[s] * a.hdiam * a.hdiam;
    a.eta[2L * t.S * nmu + o] = tot[1] + 2.0 * tot[4] + tot[5];
  }
}

// ---- the same estimate for 16 parameters per pass on the matrix cores.  Every dense term is x^T (G y) with G a projected operator
// or a factor (rows x cols, row-major in global memory) and x, y coefficient panels [.][16] in the LDS (one column per parameter):
// a wave takes 16-row strips of G, T = G y is one accumulator tile (A operand: the strip straight from global memory, lane =
// (row l & 15, k l >> 4), four k-steps of loads in flight; B operand: y rows from the LDS, lane = (parameter l & 15, k)), and the
// lane sums its four rows of x . T for ITS parameter.  G is read once per pass for all 16 parameters with full-width loads (the
// VALU kernel above: eight lanes per loaded entry).  The element-local quadratic terms and the node sums stay on the VALU.
constexpr int EST16 = 16;
struct TB16 { double v[EST16][8]; };

// tile of T = G y for the 16-row strip at row0 (rows clamped into [0, rows)); y [cols][16] in the LDS; cols <= 64.  All loads of
// the strip are issued before the first MFMA (a load -> MFMA chain per k-step exposes one memory round trip each).
__device__ inline d4 est_strip(const double* __restrict__ G, int ld, int row0, int rows, int cols, const double* y, int li, int lk) {
  const int row = row0 + li < rows ? row0 + li : rows - 1;
  const double* g = G + (long)row * ld;
  d4 acc = (d4){0.0, 0.0, 0.0, 0.0};
  for (int c0 = 0; c0 < cols; c0 += 32) {                            // eight k-steps of loads in flight (sixteen spill at 128 VGPRs)
    double av[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int c = c0 + 4 * u + lk;
      av[u] = c0 + 4 * u < cols ? g[c < cols ? c : cols - 1] : 0.0;  // (c0 + 4 u < cols: wave-uniform)
    }
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (c0 + 4 * u < cols) {
        const int c = c0 + 4 * u + lk;
        const double bv = c < cols ? y[c * 16 + li] : 0.0;
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u], bv, acc, 0, 0, 0);
      }
  }
  return acc;
}

// sum_rows x[row][m] T[row][m] over the strip's valid rows for this lane's parameter
__device__ inline double est_dot(const d4& T, const double* x, int row0, int rows, int li, int lk) {
  double v = 0.0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = row0 + lk + 4 * r;
    if (row < rows) v += x[row * 16 + li] * T[r];
  }
  return v;
}

// sum_j g[j] u[j * 16] for the 16 parameter lanes of a worker (consecutive lanes, same g, same control flow; n <= 64): lane m loads
// entry 16 c + m of every chunk, the group passes the values around by lane shuffles (see dot_row8)
__device__ inline double dot_row16(const double* __restrict__ g, const double* u, int n) {
  const int lane = threadIdx.x & 63, m = lane & 15, base = lane & ~15;
  double mine[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) mine[c] = (c * 16 < n && c * 16 + m < n) ? g[c * 16 + m] : 0.0;
  double d = 0.0;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    if (c * 16 >= n) break;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const double gk = __shfl(mine[c], base + k);
      if (c * 16 + k < n) d += gk * u[(c * 16 + k) * 16];
    }
  }
  return d;
}

constexpr int EST_NW = 16;     // waves per workgroup of k3_estimate_batch16 (<= 128 VGPRs: sixteen k-steps of loads per strip would spill)

__global__ __launch_bounds__(64 * EST_NW) void k3_estimate_batch16(T3 t, int Q, int N, int nmu, int m0, TB16 th, EA a) {
  extern __shared__ double lds[];
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, li = lane & 15, lk = lane >> 4, QN = Q * N;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int w = tid >> 4, m = tid & 15, NWK = 4 * EST_NW;     // VALU parts: workers x 16 parameters
  const int mb = nmu - m0 < EST16 ? nmu - m0 : EST16;
  double* us = lds;                        // [7][N][16]  coefficients of the neighbourhood
  double* ur = us + 7 * N * 16;            // [QN][16]    theta_q u_own
  double* zf = ur + QN * 16;               // [nbf][16]   neighbours' flux traces at the side faces
  double* z = zf + t.nbf * 16;             // [nb][16]    neighbours' node averages at the boundary nodes
  double* red = z + t.nb * 16;             // [EST_NW][6][16] parts of the waves + [NWK][16] r_fd parts of the workers
  for (int i = tid; i < 7 * N * 16; i += 64 * EST_NW) {
    const int mm = i & 15, row = i >> 4, s2 = t.nbr[s * 7 + row / N];
    us[i] = (s2 >= 0 && mm < mb) ? a.u[((long)s2 * N + row % N) * nmu + m0 + mm] : 0.0;
  }
  __syncthreads();
  const double* u0p = us + 3 * N * 16;     // own coefficients [N][16]
  for (int i = tid; i < QN * 16; i += 64 * EST_NW) {
    const int mm = i & 15, c = i >> 4;
    ur[i] = th.v[mm][c / N] * u0p[(c % N) * 16 + mm];
  }
  double thq[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) thq[q] = q < Q ? th.v[li][q] : 0.0;
  // the strips of a term are dealt to the waves round-robin, every term starting one wave further (terms have 2 .. 25 strips)
  int rot = 0;
  auto first_strip = [&]() { return 16 * ((wave + EST_NW - (rot++ % EST_NW)) % EST_NW); };
  // zf = sum_q theta_q Rb_q u_a, side by side (the rows of a side read the coefficients of ONE neighbour)
  for (int side = 0; side < 6; ++side) {
    const double* ua = us + side_slot(side) * N * 16;
    for (int row0 = first_strip(); row0 < t.ncf; row0 += 16 * EST_NW) {
      d4 zt = (d4){0.0, 0.0, 0.0, 0.0};
      for (int q = 0; q < Q; ++q) {
        const d4 T = est_strip(a.Rb + ((long)s * t.nbf + side * t.ncf) * QN + q * N, QN, row0, t.ncf, N, ua, li, lk);
#pragma unroll
        for (int r = 0; r < 4; ++r) zt[r] += thq[q] * T[r];
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = row0 + lk + 4 * r;
        if (row < t.ncf) zf[(side * t.ncf + row) * 16 + li] = zt[r];
      }
    }
  }
  // z = sum over the (<= 3) sides of a boundary node of As u_a: side by side as MFMA strips over the side's nodes, each tile added to
  // the rows of its boundary nodes (a side holds a node once: no two lanes meet; the sides follow each other, so the order of the
  // additions is fixed).  (One worker per node with its rows loaded cooperatively: 78 us of 246 -- chains of index -> row -> 30
  // shuffles per node.)
  int* sp2bn = reinterpret_cast<int*>(red + EST_NW * 6 * 16 + 4 * EST_NW * 16);      // [6 nvs] side node -> boundary node
  for (int i = tid; i < 6 * t.nvs; i += 64 * EST_NW) sp2bn[i] = -1;
  for (int i = tid; i < t.nb * 16; i += 64 * EST_NW) z[i] = 0.0;
  __syncthreads();
  for (int i = tid; i < 3 * t.nb; i += 64 * EST_NW) {
    const int sp = t.bnode_sides[i];
    if (sp >= 0) sp2bn[sp] = i / 3;
  }
  __syncthreads();
  for (int side = 0; side < 6; ++side) {
    const double* ua = us + side_slot(side) * N * 16;
    for (int row0 = first_strip(); row0 < t.nvs; row0 += 16 * EST_NW) {
      const d4 T = est_strip(a.As + ((long)s * 6 * t.nvs + side * t.nvs) * N, N, row0, t.nvs, N, ua, li, lk);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = row0 + lk + 4 * r;
        const int bn = row < t.nvs ? sp2bn[side * t.nvs + row] : -1;
        if (bn >= 0) z[bn * 16 + li] += T[r];
      }
    }
    __syncthreads();
  }
  double p_nc = 0.0, p_bb = 0.0, p_dd = 0.0, p_fd = 0.0, p_ab = 0.0, p_aa = 0.0;      // per lane: its parameter, part of the rows
  // ---- dense terms on the matrix cores
  for (int row0 = first_strip(); row0 < N; row0 += 16 * EST_NW) {
    p_nc += est_dot(est_strip(a.G_nc + (long)s * N * N, N, row0, N, N, u0p, li, lk), u0p, row0, N, li, lk);
    for (int q = 0; q < Q; ++q) {
      p_ab += thq[q] * est_dot(est_strip(a.G_ab + ((long)q * t.S + s) * N * QN, QN, row0, N, QN, ur, li, lk), u0p, row0, N, li, lk);
      for (int q2 = 0; q2 < Q; ++q2)
        p_aa += thq[q] * thq[q2] *
                est_dot(est_strip(a.G_aa + (((long)q * Q + q2) * t.S + s) * N * N, N, row0, N, N, u0p, li, lk), u0p, row0, N, li, lk);
    }
  }
  for (int row0 = first_strip(); row0 < t.nb; row0 += 16 * EST_NW)
    p_nc += 2.0 * est_dot(est_strip(a.Cn + (long)s * t.nb * N, N, row0, t.nb, N, u0p, li, lk), z, row0, t.nb, li, lk);
  for (int row0 = first_strip(); row0 < QN; row0 += 16 * EST_NW) {
    p_bb += est_dot(est_strip(a.G_bb + (long)s * QN * QN, QN, row0, QN, QN, ur, li, lk), ur, row0, QN, li, lk);
    p_dd += est_dot(est_strip(a.G_rdd + (long)s * QN * QN, QN, row0, QN, QN, ur, li, lk), ur, row0, QN, li, lk);
  }
  for (int row0 = first_strip(); row0 < t.nbf; row0 += 16 * EST_NW) {
    p_bb += 2.0 * est_dot(est_strip(a.Yb + (long)s * t.nbf * QN, QN, row0, t.nbf, QN, ur, li, lk), zf, row0, t.nbf, li, lk);
    p_dd += 2.0 * est_dot(est_strip(a.Dp + (long)s * t.nbf * QN, QN, row0, t.nbf, QN, ur, li, lk), zf, row0, t.nbf, li, lk);
    for (int q = 0; q < Q; ++q)
      p_ab += thq[q] * est_dot(est_strip(a.Xab + ((long)q * t.S + s) * t.nbf * N, N, row0, t.nbf, N, u0p, li, lk), zf, row0, t.nbf, li, lk);
  }
  // ---- element-local quadratic terms, one element per wave at a time, on the matrix cores as well:
  // boundary elements: ze^T E ze with ze = z at the element's boundary nodes (0 elsewhere); T = E ze is a 10 x 16 tile, K = 10
  // (four elements per wave in flight: one at a time is a chain of memory round trips -- index, block, LDS -- per element)
  constexpr int EU = 4;
  for (int k0 = wave * EU; k0 < t.nbel; k0 += EST_NW * EU) {
    double av[EU][3], bv[EU][3], xr[EU][3];
#pragma unroll
    for (int x = 0; x < EU; ++x) {
      const int k = k0 + x < t.nbel ? k0 + x : t.nbel - 1;
      const int e = t.bel_elem[k];
      const double* E = a.ebar + ((long)s * t.nT + e) * 100 + (li < 10 ? li : 9) * 10;
#pragma unroll
      for (int u = 0; u < 3; ++u) {
        const int c = 4 * u + lk, cc = c < 10 ? c : 9;
        av[x][u] = E[cc];
        const int bn = t.bel_bnode[k * 10 + cc];
        bv[x][u] = (c < 10 && bn >= 0 && k0 + x < t.nbel) ? z[bn * 16 + li] : 0.0;
        xr[x][u] = bv[x][u];                                       // rows lk + 4 u of ze: the same entries as the B operand
      }
    }
#pragma unroll
    for (int x = 0; x < EU; ++x) {
      d4 T = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int u = 0; u < 3; ++u) T = __builtin_amdgcn_mfma_f64_16x16x4f64(av[x][u], bv[x][u], T, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 3; ++r) p_nc += xr[x][r] * T[r];       // (rows >= 10 and missing nodes carry ze = 0)
    }
  }
  // side elements: ze^T B ze, the divergence of the side part and its pairings; ze = zf at the element's side faces (4 x 4 block)
  for (int k0 = wave * EU; k0 < t.nsel; k0 += EST_NW * EU) {
    double av[EU], ze[EU], cf[EU], bd[EU];
#pragma unroll
    for (int x = 0; x < EU; ++x) {
      const bool on = k0 + x < t.nsel;
      const int k = on ? k0 + x : t.nsel - 1;
      const int e = t.sel_elem[k], ty = t.elem_type[e];
      const int sf = t.sel_sf[k * 4 + lk];
      ze[x] = (on && sf >= 0) ? zf[sf * 16 + li] : 0.0;            // face lk, parameter li
      av[x] = a.Bbb[((long)s * t.nT + e) * 16 + (li < 4 ? li : 3) * 4 + lk];
      cf[x] = sgn3(t, s, e, lk) * t.divc[ty * 4 + lk];
      bd[x] = a.bdiv[(long)s * t.nT + e];
    }
#pragma unroll
    for (int x = 0; x < EU; ++x) {
      const d4 T = __builtin_amdgcn_mfma_f64_16x16x4f64(av[x], ze[x], (d4){0.0, 0.0, 0.0, 0.0}, 0, 0, 0);
      p_bb += ze[x] * T[0];                                         // row lk of B ze (rows 0 .. 3 sit in register 0)
      double dv = cf[x] * ze[x];
      dv += __shfl_xor(dv, 16);
      dv += __shfl_xor(dv, 32);
      if (lk == 0) {
        p_dd += t.volume * dv * dv;
        p_fd += bd[x] * dv;
      }
    }
  }
  // sum over the four k lanes of a parameter
  double part[6] = {p_nc, p_bb, p_dd, p_fd, p_ab, p_aa};
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    part[k] += __shfl_xor(part[k], 16);
    part[k] += __shfl_xor(part[k], 32);
  }
  double v_fd = 0.0;                       // r_fd . ur: thread = (worker w, parameter m)
  for (int r = w; r < QN; r += NWK) v_fd += a.r_fd[(long)s * QN + r] * ur[r * 16 + m];
  double* vred = red + EST_NW * 6 * 16;    // [NWK][16]
  vred[w * 16 + m] = v_fd;
  if (lk == 0)
#pragma unroll
    for (int k = 0; k < 6; ++k) red[(wave * 6 + k) * 16 + li] = part[k];
  __syncthreads();
  if (tid < mb) {                          // totals per parameter, fixed order
    double tot[6];
    for (int k = 0; k < 6; ++k) {
      double v = 0.0;
      for (int ww = 0; ww < EST_NW; ++ww) v += red[(ww * 6 + k) * 16 + tid];
      tot[k] = v;
    }
    for (int ww = 0; ww < NWK; ++ww) tot[3] += vred[ww * 16 + tid];
    const double pi = 3.14159265358979323846;
    const long o = (long)s * nmu + m0 + tid;
    a.eta[o] = tot[0];
    a.eta[(long)t.S * nmu + o] = (a.f2[s] - 2.0 * tot[3] + tot[2]) * (1.0 / (pi * pi)) / a.ceps[s] * a.hdiam * a.hdiam;
    a.eta[2L * t.S * nmu + o] = tot[1] + 2.0 * tot[4] + tot[5];
  }
}

// ---- the nonconformity form ALONE for 16 columns per pass (the batched parabolic estimate evaluates it on the differences
// U[k+1] - U[k]): nc = u^T G_nc u + 2 (Cn u) . z + sum_e ze^T E ze with z = sum_sides As u_a, the same panel layout, strips and
// element tiles as k3_estimate_batch16; a.eta [S][nmu].  Of the estimator operators it reads As, G_nc, Cn and ebar only.
// Without zf and the side elements nothing orders the terms but z, so the work is two flat item lists dealt round-robin to the 16
// waves: A = the (side, strip) tiles of As and the strips of G_nc; B (behind z) = the strips of Cn and, starting at the wave where
// those stop, the boundary elements in fours.  The tiles of the sides go to zs [6][nvs][16] (no two lanes meet, no barrier per side
// as in the full kernel) and a node's z is the sum of its (<= 3) memberships in the order of bnode_sides.
__global__ __launch_bounds__(64 * EST_NW) void k3_estimate_nc_batch16(T3 t, int N, int nmu, int m0, EA a) {
  extern __shared__ double lds[];
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, li = lane & 15, lk = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int mb = nmu - m0 < EST16 ? nmu - m0 : EST16;
  double* us = lds;                        // [7][N][16]    coefficients of the neighbourhood
  double* zs = us + 7 * N * 16;            // [6][nvs][16]  As u_a per side node
  double* z = zs + 6 * t.nvs * 16;         // [nb][16]      neighbours' node averages at the boundary nodes
  double* red = z + t.nb * 16;             // [EST_NW][16]  parts of the waves
  for (int i = tid; i < 7 * N * 16; i += 64 * EST_NW) {
    const int mm = i & 15, row = i >> 4, s2 = t.nbr[s * 7 + row / N];
    us[i] = (s2 >= 0 && mm < mb) ? a.u[((long)s2 * N + row % N) * nmu + m0 + mm] : 0.0;
  }
  __syncthreads();
  const double* u0p = us + 3 * N * 16;     // own coefficients [N][16]
  const int nst = (t.nvs + 15) / 16, ngs = (N + 15) / 16, ncs = (t.nb + 15) / 16;
  double p_nc = 0.0;                       // per lane: its column, part of the rows
  for (int it = wave; it < 6 * nst + ngs; it += EST_NW) {
    if (it < 6 * nst) {
      const int side = it / nst, row0 = 16 * (it - side * nst);
      const d4 T = est_strip(a.As + ((long)s * 6 * t.nvs + side * t.nvs) * N, N, row0, t.nvs, N, us + side_slot(side) * N * 16, li, lk);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = row0 + lk + 4 * r;
        if (row < t.nvs) zs[(side * t.nvs + row) * 16 + li] = T[r];
      }
    } else {
      const int row0 = 16 * (it - 6 * nst);
      p_nc += est_dot(est_strip(a.G_nc + (long)s * N * N, N, row0, N, N, u0p, li, lk), u0p, row0, N, li, lk);
    }
  }
  __syncthreads();
  for (int i = tid; i < t.nb * 16; i += 64 * EST_NW) {
    const int bn = i >> 4, mm = i & 15;
    double acc = 0.0;
    for (int k = 0; k < 3; ++k) {
      const int sp = t.bnode_sides[bn * 3 + k];
      if (sp >= 0) acc += zs[sp * 16 + mm];
    }
    z[i] = acc;
  }
  __syncthreads();
  for (int it = wave; it < ncs; it += EST_NW)
    p_nc += 2.0 * est_dot(est_strip(a.Cn + (long)s * t.nb * N, N, 16 * it, t.nb, N, u0p, li, lk), z, 16 * it, t.nb, li, lk);
  // boundary elements: ze^T E ze as in k3_estimate_batch16 (T = E ze a 10 x 16 tile, K = 10, four elements per wave in flight)
  constexpr int EU = 4;
  const int wel = (wave + EST_NW - ncs % EST_NW) % EST_NW;
  for (int k0 = wel * EU; k0 < t.nbel; k0 += EST_NW * EU) {
    double av[EU][3], bv[EU][3];
#pragma unroll
    for (int x = 0; x < EU; ++x) {
      const int k = k0 + x < t.nbel ? k0 + x : t.nbel - 1;
      const int e = t.bel_elem[k];
      const double* E = a.ebar + ((long)s * t.nT + e) * 100 + (li < 10 ? li : 9) * 10;
#pragma unroll
      for (int u = 0; u < 3; ++u) {
        const int c = 4 * u + lk, cc = c < 10 ? c : 9;
        av[x][u] = E[cc];
        const int bn = t.bel_bnode[k * 10 + cc];
        bv[x][u] = (c < 10 && bn >= 0 && k0 + x < t.nbel) ? z[bn * 16 + li] : 0.0;      // also rows lk + 4 u of ze
      }
    }
#pragma unroll
    for (int x = 0; x < EU; ++x) {
      d4 T = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int u = 0; u < 3; ++u) T = __builtin_amdgcn_mfma_f64_16x16x4f64(av[x][u], bv[x][u], T, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 3; ++r) p_nc += bv[x][r] * T[r];       // (rows >= 10 and missing nodes carry ze = 0)
    }
  }
  p_nc += __shfl_xor(p_nc, 16);
  p_nc += __shfl_xor(p_nc, 32);
  if (lk == 0) red[wave * 16 + li] = p_nc;
  __syncthreads();
  if (tid < mb) {                          // totals per column, the waves in their order
    double v = 0.0;
    for (int ww = 0; ww < EST_NW; ++ww) v += red[ww * 16 + tid];
    a.eta[(long)s * nmu + m0 + tid] = v;
  }
}

// ------------------------------------------------------------------------------------------------- one-block sum of partials
// (fom_cg, the Euler drivers and, through launch_reduce1, the reduced PCG of online3d.hip)
__global__ __launch_bounds__(256) void k3_reduce1(int S, const double* __restrict__ part, double* __restrict__ out) {
  __shared__ double red[256];
  const int tid = threadIdx.x;
  // eight loads in flight per thread (a plain `acc += part[k]` loop waits one L2 round trip per entry: 11 us for 10 k entries)
  double a[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  int k = tid;
  for (; k + 7 * 256 < S; k += 8 * 256) {
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = part[k + u * 256];
#pragma unroll
    for (int u = 0; u < 8; ++u) a[u] += v[u];
  }
  for (; k < S; k += 256) a[0] += part[k];
  red[tid] = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) red[tid] += red[tid + w];
    __syncthreads();
  }
  if (tid == 0) out[0] = red[0];
}

// ------------------------------------------------------------------------------------------------- full-order apply
__global__ __launch_bounds__(256) void k3_fom_apply(T3 t, int Q, int M, QV th, const double* __restrict__ A_diag,
                                                    const double* __restrict__ A_cpl, const double* __restrict__ x,
                                                    double* __restrict__ y) {
  const int e = blockIdx.x, s = blockIdx.y;
  for (int w = threadIdx.x; w < 10 * M; w += 256) {
    const int i = w / M, m = w - i * M;
    double acc = 0.0;
    for (int q = 0; q < Q; ++q) {
      double aq = 0.0;
      const double* A = A_diag + ((((long)q * t.S + s) * t.nT + e) * 5) * 100 + i * 10;
      for (int slot = 0; slot < 5; ++slot) {
        int ee = e, ss = s;
        const double* L = A + slot * 100;
        if (slot > 0) {
          ee = t.nb_elem[e * 4 + slot - 1];
          if (ee < 0) {
            if (A_cpl == nullptr) continue;      // local operator (energy product): no coupling blocks
            const int side = -(ee + 1);
            ss = t.nbr[s * 7 + side_slot(side)];
            if (ss < 0) continue;
            L = A_cpl + ((((long)q * t.S + s) * 6 + side) * t.ncf + t.face_pos[e * 4 + slot - 1]) * 100 + i * 10;
            ee = t.nb_out[e * 4 + slot - 1];
          }
        }
        const double* xv = x + ((long)ss * t.n + ee * 10) * M + m;
        for (int j = 0; j < 10; ++j) aq += L[j] * xv[(long)j * M];
      }
      acc += th.v[q] * aq;
    }
    y[((long)s * t.n + e * 10 + i) * M + m] = acc;
  }
}

// ------------------------------------------------------------------------------------------------- full-order solve (snapshots)
// A(mu) x = b on the never-assembled block operator: CG with the 10 x 10 element blocks as block-Jacobi preconditioner.  The
// operator is combined once per solve (Amu = sum_q theta_q A_q); an iteration is three kernels + three one-block reductions,
// all scalars stay on the device.  EPB elements (10 rows each) per workgroup.
constexpr int FOM_MAX_COARSE = 8192;      // largest dense coarse problem of the full-order solver (2 x 0.5 GB of work, ~0.1 s to invert)

// inverse of the diagonal 10 x 10 blocks (SPD): Gauss-Jordan, one thread per element, the block in LDS
__global__ __launch_bounds__(64) void k3f_block_inverse(T3 t, const double* __restrict__ Amu, double* __restrict__ Dinv) {
  __shared__ double a[64][101];
  const int s = blockIdx.y, e = blockIdx.x * 64 + threadIdx.x;
  if (e >= t.nT) return;
  double* m = a[threadIdx.x];
  const double* src = Amu + (((long)s * t.nT + e) * 5) * 100;
  for (int i = 0; i < 100; ++i) m[i] = src[i];
  double inv[100];
  for (int i = 0; i < 100; ++i) inv[i] = (i / 10 == i % 10) ? 1.0 : 0.0;
  for (int p = 0; p < 10; ++p) {
    const double ip = 1.0 / m[p * 10 + p];
    for (int c = 0; c < 10; ++c) {
      m[p * 10 + c] *= ip;
      inv[p * 10 + c] *= ip;
    }
    for (int r = 0; r < 10; ++r) {
      if (r == p) continue;
      const double f = m[r * 10 + p];
      for (int c = 0; c < 10; ++c) {
        m[r * 10 + c] -= f * m[p * 10 + c];
        inv[r * 10 + c] -= f * inv[p * 10 + c];
      }
    }
  }
  // the inverse of an SPD block is symmetric: its upper triangle is stored, packed row by row (56 doubles per block) -- the update
  // kernel of the CG streams these blocks every iteration and is bound by their bytes
  double* dst = Dinv + ((long)s * t.nT + e) * 56;
  int k = 0;
  for (int i = 0; i < 10; ++i)
    for (int j = i; j < 10; ++j) dst[k++] = inv[i * 10 + j];
  dst[55] = 0.0;
}

// scal: [0], [1] r.z of the last two updates (alternating)  [2] pAp  [3] rr  [4] bb
// p = z + beta p  (beta = rz_new / rz_old; p = z in the first iteration)
//   with the coarse level: z + R0^T y0 in the place of z (y0 [S][nc], Phi [n][4])
__global__ __launch_bounds__(256) void k3f_dir(long total, int first, int cur, const double* __restrict__ scal,
                                               const double* __restrict__ z, double* __restrict__ p, int n, int nc,
                                               const double* __restrict__ Phi, const double* __restrict__ y0) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const double beta = first ? 0.0 : scal[cur] / scal[cur ^ 1];       // r.z of the last two updates alternate between slots 0 and 1
  double zi = z[i];
  if (nc > 0) {
    const long s = i / n;
    const int dof = (int)(i - s * n);
    for (int k = 0; k < nc; ++k) zi += Phi[dof * 4 + k] * y0[s * nc + k];
  }
  p[i] = first ? zi : zi + beta * p[i];              // the first direction does not read p: work is uninitialised there
}

// y = Amu p on the block-ELL + coupling data; partial p.y per workgroup.
// Bound by the 0.8 GB of 10 x 10 blocks it streams, so (1) every block is read by ONE 16-byte-per-lane load of 50 lanes (800
// contiguous bytes; lane l holds A[i][2c], A[i][2c + 1], i = l / 5, c = l % 5 -- a thread per row reading 80-byte rows costs a
// cache-line lookup per lane and instruction, which, not the HBM, then sets the pace) and the products are summed across lanes;
// (2) the operator is symmetric, A[e'][e] = A[e][e']^T: inside a subdomain only the blocks towards the neighbour with the HIGHER
// element index are read from their own place (sum over the row: lanes l .. l + 4), the element on the other side reads the same
// block and sums over the columns (lanes l, l + 5, ...).  The two readers are workgroups of the same subdomain, and the 1D grid
// is decoded so that all workgroups of a subdomain run on one XCD (xcd_block): the second read comes from that XCD's L2 and HBM
// delivers 61 % of the block bytes.  One wave per element at a time, four waves per workgroup.
__global__ __launch_bounds__(256) void k3f_matvec(T3 t, int nbx, const double* __restrict__ Amu, const double* __restrict__ Cmu,
                                                  const double* __restrict__ p, double* __restrict__ y, double* __restrict__ part) {
  __shared__ double red[4];
  int s, bx;
  if (!xcd_block(nbx, t.S, bx, s)) return;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const bool act = lane < 50;
  const int li = act ? lane : 49, row = li / 5, c2 = 2 * (li - row * 5);
  const double* As = Amu + (long)s * t.nT * 500;
  const double* ps = p + (long)s * t.n;
  double py = 0.0;
  const int e1 = (bx + 1) * FOM_EPB < t.nT ? (bx + 1) * FOM_EPB : t.nT;
  for (int e = bx * FOM_EPB + wave; e < e1; e += 4) {
    const int4 nb = *reinterpret_cast<const int4*>(t.nb_elem + e * 4);
    const int nbv[4] = {nb.x, nb.y, nb.z, nb.w};
    double yr = 0.0, yc0 = 0.0, yc1 = 0.0;            // row sums (valid in lanes 5 i), column sums (valid in lanes 0 .. 4)
    {                                                 // diagonal block
      const double2 a = *reinterpret_cast<const double2*>(As + (long)e * 500 + li * 2);
      const double2 pv = *reinterpret_cast<const double2*>(ps + e * 10 + c2);
      yr = act ? a.x * pv.x + a.y * pv.y : 0.0;
    }
    // (the faces are wave-uniform branches; making every load unconditional -- faces without a neighbour pointing at the own block
    // with weight zero -- was measured: 136 instead of 126 us, the kernel is within 25 % of its HBM time either way)
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      const int ee = nbv[f];                          // wave-uniform
      if (ee >= 0 && ee < e) {                        // the lower element's block towards e, used transposed
        const int4 nb2 = *reinterpret_cast<const int4*>(t.nb_elem + ee * 4);
        const int fb = nb2.x == e ? 0 : (nb2.y == e ? 1 : (nb2.z == e ? 2 : 3));
        const double2 a = *reinterpret_cast<const double2*>(As + (long)ee * 500 + (1 + fb) * 100 + li * 2);
        const double pr = ps[ee * 10 + row];
        yc0 += act ? a.x * pr : 0.0;
        yc1 += act ? a.y * pr : 0.0;
        continue;
      }
      const double* L;
      const double* pn;
      if (ee >= 0) {
        L = As + (long)e * 500 + (1 + f) * 100;
        pn = ps + ee * 10;
      } else {
        const int side = -(ee + 1), ss = t.nbr[s * 7 + side_slot(side)];
        if (ss < 0) continue;
        L = Cmu + (((long)s * 6 + side) * t.ncf + t.face_pos[e * 4 + f]) * 100;
        pn = p + (long)ss * t.n + t.nb_out[e * 4 + f] * 10;
      }
      const double2 a = *reinterpret_cast<const double2*>(L + li * 2);
      const double2 pv = *reinterpret_cast<const double2*>(pn + c2);
      yr += act ? a.x * pv.x + a.y * pv.y : 0.0;
    }
    // row sums: lanes l .. l + 4 (fixed order), result in lanes 5 i
    double r1 = yr + __shfl_down(yr, 1);
    r1 = r1 + __shfl_down(r1, 2);
    const double rs = r1 + __shfl_down(yr, 4);
    // column sums: lanes l, l + 5, ..., l + 45 (lanes >= 50 contribute zeros), result in lanes 0 .. 4
    double c0 = yc0 + __shfl_down(yc0, 5), c1 = yc1 + __shfl_down(yc1, 5);
    c0 += __shfl_down(c0, 10); c1 += __shfl_down(c1, 10);
    c0 += __shfl_down(c0, 20); c1 += __shfl_down(c1, 20);
    c0 += __shfl_down(yc0 + __shfl_down(yc0, 5), 40); c1 += __shfl_down(yc1 + __shfl_down(yc1, 5), 40);
    // entry t of y_e in lane t < 10: row sum of row t + column sum of column t
    const int tl = lane < 10 ? lane : 0;
    const double ya = __shfl(rs, 5 * tl), yb0 = __shfl(c0, tl >> 1), yb1 = __shfl(c1, tl >> 1);
    if (lane < 10) {
      const double v = ya + ((lane & 1) ? yb1 : yb0);
      y[(long)s * t.n + e * 10 + lane] = v;
      py += v * ps[e * 10 + lane];
    }
  }
  for (int o = 8; o > 0; o >>= 1) py += __shfl_down(py, o);          // lanes 0 .. 9 (others are zero)
  if (lane == 0) red[wave] = py;
  __syncthreads();
  if (threadIdx.x == 0) part[(long)s * nbx + bx] = (red[0] + red[1]) + (red[2] + red[3]);
}

// x += alpha p, r -= alpha y, z = Dinv r; partials r.z and r.r per workgroup (init: x = 0, r = b: alpha = 0 with p = y = any)
__global__ __launch_bounds__(256) void k3f_update(T3 t, int init, int cur, const double* __restrict__ scal, const double* __restrict__ Dinv,
                                                  const double* __restrict__ p, const double* __restrict__ y, const double* __restrict__ b,
                                                  double* __restrict__ x, double* __restrict__ r, double* __restrict__ z,
                                                  double* __restrict__ prz, double* __restrict__ prr, int nc,
                                                  const double* __restrict__ Phi, double* __restrict__ pr0) {
  __shared__ double rs[256], red[256];
  const int s = blockIdx.y, tid = threadIdx.x;
  const int el = tid / 10, i = tid - el * 10, e = blockIdx.x * FOM_EPB + el;
  const bool on = el < FOM_EPB && e < t.nT;
  const long d = (long)s * t.n + e * 10 + i;
  double ri = 0.0;
  if (on) {
    if (init) {
      ri = b[d];
      x[d] = 0.0;
    } else {
      const double alpha = scal[cur] / scal[2];
      x[d] += alpha * p[d];
      ri = r[d] - alpha * y[d];
    }
    r[d] = ri;
  }
  rs[tid] = ri;
  __syncthreads();
  double zi = 0.0;
  if (on) {
    const double* D = Dinv + ((long)s * t.nT + e) * 56;          // packed upper triangle: entry (a, b), a <= b, at a (21 - a) / 2 + b - a
#pragma unroll
    for (int j = 0; j < 10; ++j) {
      const int a = i < j ? i : j, b = i < j ? j : i;
      zi += D[a * (21 - a) / 2 + b - a] * rs[el * 10 + j];
    }
    z[d] = zi;
  }
  red[tid] = ri * zi;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) red[tid] += red[tid + w];
    __syncthreads();
  }
  const long blk = (long)blockIdx.y * gridDim.x + blockIdx.x;
  if (tid == 0) prz[blk] = red[0];
  __syncthreads();
  red[tid] = ri * ri;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) red[tid] += red[tid + w];
    __syncthreads();
  }
  if (tid == 0) prr[blk] = red[0];
  // restriction of the residual to the coarse space: partial sums phi_k . r of this workgroup's rows (fixed-order tree)
  for (int k = 0; k < nc; ++k) {
    __syncthreads();
    red[tid] = on ? ri * Phi[(e * 10 + i) * 4 + k] : 0.0;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
      if (tid < w) red[tid] += red[tid + w];
      __syncthreads();
    }
    if (tid == 0) pr0[blk * 4 + k] = red[0];
  }
}

// ---- coarse level of the full-order preconditioner: M^-1 = blockdiag(A_ee)^-1 + R0^T (R0 A R0^T)^-1 R0 (additive, SPD), the rows
// of R0 = nc functions per subdomain (P1 in the subdomain-local coordinates by default: Phi [n][4], the same table everywhere).
// A1b [S][7][16]: the 4 x 4 blocks phi_{s,k}^T A phi_{t,l} for t = the subdomain itself (slot 3) and its six neighbours.
__global__ __launch_bounds__(256) void k3f_coarse_blocks(T3 t, const double* __restrict__ Phi, const double* __restrict__ Amu,
                                                         const double* __restrict__ Cmu, double* __restrict__ A1b) {
  __shared__ double red[16][256];
  const int s = blockIdx.x, tid = threadIdx.x;
  const int el = tid / 10, i = tid - el * 10;
  for (int t7 = 0; t7 < 7; ++t7) {
    double acc[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) acc[c] = 0.0;
    if (el < 25)
      for (int e = el; e < t.nT; e += 25) {
        const double* A = Amu + (((long)s * t.nT + e) * 5) * 100 + i * 10;
        const double* ph = Phi + (e * 10 + i) * 4;
        for (int slot = 0; slot < 5; ++slot) {
          int ee = e, tgt = 3;
          const double* L = A + slot * 100;
          if (slot > 0) {
            ee = t.nb_elem[e * 4 + slot - 1];
            if (ee < 0) {
              const int side = -(ee + 1);
              tgt = side_slot(side);
              if (t.nbr[s * 7 + tgt] < 0) continue;
              L = Cmu + (((long)s * 6 + side) * t.ncf + t.face_pos[e * 4 + slot - 1]) * 100 + i * 10;
              ee = t.nb_out[e * 4 + slot - 1];
            }
          }
          if (tgt != t7) continue;
          double a[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
          for (int j = 0; j < 10; ++j) {
            const double lj = L[j];
            const double* pj = Phi + (ee * 10 + j) * 4;
#pragma unroll
            for (int l = 0; l < 4; ++l) a[l] += lj * pj[l];
          }
#pragma unroll
          for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int l = 0; l < 4; ++l) acc[k * 4 + l] += ph[k] * a[l];
        }
      }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 16; ++c) red[c][tid] = acc[c];
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
      for (int idx = tid; idx < 16 * w; idx += 256) {
        const int c = idx / w, k = idx - c * w;
        red[c][k] += red[c][k + w];
      }
      __syncthreads();
    }
    if (tid < 16) A1b[((long)s * 7 + t7) * 16 + tid] = red[tid][0];
  }
}

// dense coarse matrix [M][M], M = nc S, from the blocks (zero-filled before); identity for the inverse
__global__ __launch_bounds__(256) void k3f_coarse_dense(T3 t, int nc, const double* __restrict__ A1b, double* __restrict__ A1,
                                                        double* __restrict__ Id) {
  const long M = (long)nc * t.S;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx < M) Id[idx * M + idx] = 1.0;
  if (idx >= (long)t.S * 7 * 16) return;
  const int kl = (int)(idx & 15), t7 = (int)((idx >> 4) % 7), s = (int)(idx / 112);
  const int k = kl >> 2, l = kl & 3;
  const int tt = t7 == 3 ? s : t.nbr[s * 7 + t7];
  if (tt < 0 || k >= nc || l >= nc) return;
  A1[((long)s * nc + k) * M + (long)tt * nc + l] = A1b[idx];
}

// r0 [M] from the workgroups' partial sums (fixed order)
__global__ __launch_bounds__(256) void k3f_coarse_r0(int S, int nbx, int nc, const double* __restrict__ pr0, double* __restrict__ r0) {
  const int m = blockIdx.x * 256 + threadIdx.x;
  if (m >= S * nc) return;
  const int s = m / nc, k = m - s * nc;
  double v = 0.0;
  for (int bx = 0; bx < nbx; ++bx) v += pr0[((long)s * nbx + bx) * 4 + k];
  r0[m] = v;
}

// y0 = A1inv r0, one wave per row; prc [M] = r0 . y0 contributions to r.z
__global__ __launch_bounds__(256) void k3f_coarse_apply(int M, const double* __restrict__ A1inv, const double* __restrict__ r0,
                                                        double* __restrict__ y0, double* __restrict__ prc) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= M) return;
  const double* a = A1inv + (long)row * M;
  double v0 = 0.0, v1 = 0.0, v2 = 0.0, v3 = 0.0;
  int c = lane;
  for (; c + 192 < M; c += 256) {
    v0 += a[c] * r0[c];
    v1 += a[c + 64] * r0[c + 64];
    v2 += a[c + 128] * r0[c + 128];
    v3 += a[c + 192] * r0[c + 192];
  }
  for (; c < M; c += 64) v0 += a[c] * r0[c];
  double v = (v0 + v1) + (v2 + v3);
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  if (lane == 0) {
    y0[row] = v;
    prc[row] = v * r0[row];
  }
}


}  // namespace

namespace lrbms3 {

// the kernels of this file that other files launch: grid and block as at the launches below
void launch_fom_block_inverse(hipStream_t st, const T3& t, const double* Amu, double* Dinv) {
  hipLaunchKernelGGL(k3f_block_inverse, dim3((t.nT + 63) / 64, t.S), dim3(64), 0, st, t, Amu, Dinv);
}
void launch_reduce1(hipStream_t st, int S, const double* part, double* out) {
  hipLaunchKernelGGL(k3_reduce1, dim3(1), dim3(256), 0, st, S, part, out);
}

// Inverse of the dense SPD matrix A [M][M] on the stream: Cholesky factor in place (lower), then the solve against the identity
// the caller has put into Id, which becomes A^-1.  The rocBLAS handle of the context is created on first use.  hinfo receives the
// info word of the factorisation (pinfo: its device word); non-zero: A is not positive definite, the solve is not issued and Id
// stays the identity.  That is no error here: what follows from it is the caller's business.
int dense_spd_inverse(lrbms3_ctx* ctx, hipStream_t st, long M, double* A, double* Id, rocblas_int* pinfo, rocblas_int& hinfo) {
  if (!ctx->blas) {
    rocblas_handle h = nullptr;
    if (rocblas_create_handle(&h) != rocblas_status_success) return lrbms_fail(ctx, LRBMS_E_HIP, "rocblas_create_handle failed");
    ctx->blas = h;
  }
  rocblas_handle h = (rocblas_handle)ctx->blas;
  if (rocblas_set_stream(h, st) != rocblas_status_success) return lrbms_fail(ctx, LRBMS_E_HIP, "rocblas_set_stream failed");
  if (rocsolver_dpotrf(h, rocblas_fill_lower, (rocblas_int)M, A, (rocblas_int)M, pinfo) != rocblas_status_success)
    return lrbms_fail(ctx, LRBMS_E_HIP, "rocsolver_dpotrf failed");
  hinfo = 0;
  LRBMS_HIP_CHECK(ctx, hipMemcpyAsync(&hinfo, pinfo, sizeof(rocblas_int), hipMemcpyDeviceToHost, st));
  LRBMS_HIP_CHECK(ctx, hipStreamSynchronize(st));
  if (hinfo == 0 &&
      rocsolver_dpotrs(h, rocblas_fill_lower, (rocblas_int)M, (rocblas_int)M, A, (rocblas_int)M, Id, (rocblas_int)M) != rocblas_status_success)
    return lrbms_fail(ctx, LRBMS_E_HIP, "rocsolver_dpotrs failed");
  return LRBMS_OK;
}

// ---- the batched estimate as a helper: the launch loop of lrbms3_reduced_estimate_batch, on the columns of one panel
static size_t est16_lds(const T3& t, int Q, int N) {
  return sizeof(double) * ((size_t)(7 * N + Q * N + t.nbf + t.nb) * EST16 + EST_NW * 6 * 16 + 4 * EST_NW * 16 + 3 * t.nvs + 1);
}
static size_t est8_lds(const T3& t, int Q, int N) { return sizeof(double) * ((size_t)(7 * N + Q * N + t.nbf + t.nb) * EST_MB + 256); }
static size_t estnc16_lds(const T3& t, int N) { return sizeof(double) * ((size_t)(7 * N + 6 * t.nvs + t.nb) * EST16 + EST_NW * 16); }

int estimate_batch_form(const lrbms3_ctx* ctx, int Q, int N) {
  if (ctx->opt_estimate_valu == 0 && est16_lds(ctx->t, Q, N) <= 160 * 1024 - 2048) return 16;      // LRBMS3_OPT_ESTIMATE_VALU
  return est8_lds(ctx->t, Q, N) <= 160 * 1024 ? 8 : 0;
}

int launch_reduced_estimate_batch(lrbms3_ctx* ctx, hipStream_t st, int Q, int N, int nmu, const double* theta, const EA& a) {
  const T3& t = ctx->t;
  const int form = estimate_batch_form(ctx, Q, N);
  if (form == 16) {
    const size_t lds16 = est16_lds(t, Q, N);
    if (lds16 > 64 * 1024)
      LRBMS_HIP_CHECK(ctx, hipFuncSetAttribute((const void*)k3_estimate_batch16, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds16));
    for (int m0 = 0; m0 < nmu; m0 += EST16) {
      TB16 th{};
      for (int m = 0; m < EST16 && m0 + m < nmu; ++m)
        for (int q = 0; q < Q; ++q) th.v[m][q] = theta[(m0 + m) * Q + q];
      KScope ks(ctx, "k3_estimate_batch16", st);
      hipLaunchKernelGGL(k3_estimate_batch16, dim3(t.S), dim3(64 * EST_NW), lds16, st, t, Q, N, nmu, m0, th, a);
    }
    LRBMS_LAUNCH_CHECK(ctx);
    return LRBMS_OK;
  }
  if (form == 0) return lrbms_fail(ctx, LRBMS_E_INVALID, "reduced_estimate_batch: template too large for the LDS");
  const size_t lds = est8_lds(t, Q, N);
  if (lds > 64 * 1024)      // k_c = 4 at Q N = 64: 71 808 B
    LRBMS_HIP_CHECK(ctx, hipFuncSetAttribute((const void*)k3_estimate_batch, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  for (int m0 = 0; m0 < nmu; m0 += EST_MB) {
    TB8 th{};
    for (int m = 0; m < EST_MB && m0 + m < nmu; ++m)
      for (int q = 0; q < Q; ++q) th.v[m][q] = theta[(m0 + m) * Q + q];
    hipLaunchKernelGGL(k3_estimate_batch, dim3(t.S), dim3(256), lds, st, t, Q, N, nmu, m0, th, a);
  }
  LRBMS_LAUNCH_CHECK(ctx);
  return LRBMS_OK;
}

bool estimate_nc16_fits(const lrbms3_ctx* ctx, int N) { return estnc16_lds(ctx->t, N) <= 160 * 1024 - 2048; }

int launch_estimate_nc_batch(lrbms3_ctx* ctx, hipStream_t st, int N, int nmu, const EA& a) {
  const T3& t = ctx->t;
  const size_t lds = estnc16_lds(t, N);
  if (lds > 64 * 1024)
    LRBMS_HIP_CHECK(ctx, hipFuncSetAttribute((const void*)k3_estimate_nc_batch16, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  for (int m0 = 0; m0 < nmu; m0 += EST16) {
    KScope ks(ctx, "k3_estimate_nc_batch16", st);
    hipLaunchKernelGGL(k3_estimate_nc_batch16, dim3(t.S), dim3(64 * EST_NW), lds, st, t, N, nmu, m0, a);
  }
  LRBMS_LAUNCH_CHECK(ctx);
  return LRBMS_OK;
}

}  // namespace lrbms3

extern "C" {

int lrbms3_ctx_create(int device, lrbms3_ctx** out) {
  if (!out) return LRBMS_E_INVALID;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count) return LRBMS_E_HIP;
  if (hipSetDevice(device) != hipSuccess) return LRBMS_E_HIP;
  lrbms3_ctx* c = new lrbms3_ctx();
  if (lrbms_ctx_base_init(c, device) != LRBMS_OK) return lrbms3_ctx_destroy(c), LRBMS_E_HIP;
  *out = c;
  return LRBMS_OK;
}

int lrbms3_ctx_destroy(lrbms3_ctx* ctx) {
  if (!ctx) return LRBMS_E_INVALID;
  (void)hipSetDevice(ctx->device);
  for (void* p : ctx->owned) (void)hipFree(p);
  if (ctx->pg_part) (void)hipFree(ctx->pg_part);
  if (ctx->blas) (void)rocblas_destroy_handle((rocblas_handle)ctx->blas);
  if (ctx->fom_pc) (void)hipFree(ctx->fom_pc);
  lrbms_ctx_base_release(ctx);
  delete ctx;
  return LRBMS_OK;
}

const char* lrbms3_last_error(lrbms3_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int lrbms3_ctx_set_option(lrbms3_ctx* ctx, int32_t option, int32_t value) {
  if (!ctx) return LRBMS_E_INVALID;
  int hi = 1;
  if (option == LRBMS3_OPT_KSPLIT) hi = 8;
  if (option == LRBMS3_OPT_WAVES) hi = 16;
  if (value < 0 || value > hi) return lrbms_fail(ctx, LRBMS_E_INVALID, "set_option: value out of range for this option");
  switch (option) {
    case LRBMS3_OPT_KSPLIT: ctx->opt_ksplit = value; break;
    case LRBMS3_OPT_SERIAL: ctx->opt_serial = value; break;
    case LRBMS3_OPT_WAVES: ctx->opt_waves = value; break;
    case LRBMS3_OPT_ESTIMATE_VALU: ctx->opt_estimate_valu = value; break;
    case LRBMS3_OPT_SOLVE_VALU: ctx->opt_solve_valu = value; break;
    case LRBMS3_OPT_FOM_COARSE: ctx->opt_fom_coarse = value; break;
    case LRBMS3_OPT_POD_ROTATE_VALU: ctx->opt_pod_rotate_valu = value; break;
    default: return lrbms_fail(ctx, LRBMS_E_INVALID, "set_option: unknown option");
  }
  return LRBMS_OK;
}

int lrbms3_mesh_upload(lrbms3_ctx* ctx, const lrbms3_mesh_desc* d, int32_t S, int32_t S_ext, const int32_t* nbr,
                       const int32_t* phys) {
  if (!ctx || !d || !nbr || !phys) return LRBMS_E_INVALID;
  if (ctx->has_mesh) return lrbms_fail(ctx, LRBMS_E_STATE, "mesh already uploaded (one template per context)");
  if (S <= 0 || S_ext < S || d->n_T <= 0 || d->ncf <= 0) return lrbms_fail(ctx, LRBMS_E_INVALID, "bad sizes");
  for (int s = 0; s < S; ++s) {
    if (nbr[s * 7 + 3] != s) return lrbms_fail(ctx, LRBMS_E_INVALID, "nbr[s][3] must be s");
    for (int k = 0; k < 7; ++k)
      if (nbr[s * 7 + k] < -1 || nbr[s * 7 + k] >= S_ext) return lrbms_fail(ctx, LRBMS_E_INVALID, "nbr entry out of range");
  }
  LRBMS_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  T3& t = ctx->t;
  t.S = S; t.S_ext = S_ext;
  t.nT = d->n_T; t.n = 10 * d->n_T; t.nrt = d->n_rt; t.ncf = d->ncf; t.nbf = 6 * d->ncf; t.nvs = d->nvs;
  t.nnodes = d->n_nodes; t.nb = d->nb; t.nbel = d->nbel; t.nsel = d->nsel; t.nbd = d->nbd;
  t.nA = d->nA; t.nB = d->nB; t.nC = d->nC; t.nFs = d->nFs; t.nFf = d->nFf;
  t.o_fs = d->o_fs; t.o_ff = d->o_ff; t.o_c = d->o_c; t.lam_stride = d->lam_stride; t.hat_stride = d->hat_stride;
  t.f_stride = d->f_stride;
  t.volume = d->volume; t.kmin = d->kmin;
  const long nT = t.nT, n = t.n;
  int rc;
#define UP(field, count) if ((rc = upload(ctx, d->field, (long)(count), &t.field)) != LRBMS_OK) return rc
  UP(elem_type, nT); UP(up_face, nT * 4); UP(order, nT); UP(nb_elem, nT * 4); UP(nb_out, nT * 4); UP(face_pos, nT * 4); UP(tsign, nT * 4); UP(elem_rt, nT * 4);
  UP(rt_e0, t.nrt); UP(rt_f0, t.nrt); UP(rt_e1, t.nrt); UP(rt_f1, t.nrt);
  UP(side_elem, t.nbf); UP(side_face, t.nbf); UP(side_elem_out, t.nbf); UP(side_face_out, t.nbf);
  UP(dof_node, n); UP(node_ptr, t.nnodes + 1); UP(node_dofs, n); UP(node_mask, t.nnodes); UP(node_count, t.nnodes);
  UP(side_nodes, 6 * t.nvs); UP(sn_ptr, 6 * t.nvs + 1);
  UP(sn_dofs, d->sn_ptr[6 * t.nvs]);
  UP(dof_bslot, n); UP(bn_ptr, t.nb + 1); UP(bn_slots, t.nbd); UP(bnodes, t.nb); UP(bnode_sides, t.nb * 3); UP(bel_elem, t.nbel); UP(bel_bnode, t.nbel * 10); UP(sel_elem, t.nsel);
  UP(sel_sf, t.nsel * 4);
  UP(divc, 24);
  UP(TV, 6L * t.nA * 100); UP(TE, 6L * t.nB * 100); UP(TAA, 6L * t.nC * 100);
  UP(TFo, 24L * t.nFs * 100); UP(TFn, 24L * t.nFs * 100); UP(TFb, 24L * t.nFs * 100);
  UP(TPo, 24L * t.nFs * 100); UP(TPn, 24L * t.nFs * 100); UP(TPb, 24L * t.nFs * 100);
  UP(TC, 24L * t.nFf * 10); UP(TCb, 24L * t.nFf * 10);
  UP(TPH, 6L * t.nB * 10); UP(TM, 600); UP(TB, 6L * t.nC * 16); UP(TAB, 6L * t.nC * 40); UP(WB, t.nB); UP(WC, t.nC);
#undef UP
  if ((rc = upload(ctx, nbr, (long)S * 7, &t.nbr)) != LRBMS_OK) return rc;
  if ((rc = upload(ctx, phys, (long)S_ext, &t.phys)) != LRBMS_OK) return rc;
  {
    const double z[64] = {0.0};
    if ((rc = upload(ctx, z, 64L, &t.zeros)) != LRBMS_OK) return rc;
  }
  {      // concatenated table of the diagonal block: volume rule, then per face the inner-face and the Dirichlet table
    const long KD = t.nA + 8L * t.nFs;
    std::vector<double> tsd((size_t)6 * KD * 100);
    for (int ty = 0; ty < 6; ++ty) {
      double* dst = tsd.data() + (size_t)ty * KD * 100;
      memcpy(dst, d->TV + (size_t)ty * t.nA * 100, sizeof(double) * t.nA * 100);
      for (int f = 0; f < 4; ++f) {
        memcpy(dst + ((size_t)t.nA + (size_t)f * 2 * t.nFs) * 100, d->TFo + ((size_t)(ty * 4 + f) * t.nFs) * 100, sizeof(double) * t.nFs * 100);
        memcpy(dst + ((size_t)t.nA + (size_t)f * 2 * t.nFs + t.nFs) * 100, d->TFb + ((size_t)(ty * 4 + f) * t.nFs) * 100, sizeof(double) * t.nFs * 100);
      }
    }
    if ((rc = upload(ctx, tsd.data(), (long)tsd.size(), &t.TSD)) != LRBMS_OK) return rc;
    for (int ty = 0; ty < 6; ++ty) {      // the same layout with the penalty parts of the face tables: local energy product
      double* dst = tsd.data() + (size_t)ty * KD * 100;
      for (int f = 0; f < 4; ++f) {
        memcpy(dst + ((size_t)t.nA + (size_t)f * 2 * t.nFs) * 100, d->TPo + ((size_t)(ty * 4 + f) * t.nFs) * 100, sizeof(double) * t.nFs * 100);
        memcpy(dst + ((size_t)t.nA + (size_t)f * 2 * t.nFs + t.nFs) * 100, d->TPb + ((size_t)(ty * 4 + f) * t.nFs) * 100, sizeof(double) * t.nFs * 100);
      }
    }
    if ((rc = upload(ctx, tsd.data(), (long)tsd.size(), &t.TSP)) != LRBMS_OK) return rc;
  }
  ctx->nbr_host.assign(nbr, nbr + (long)S * 7);
  ctx->sub_active = false;      // a restriction of the pass belongs to a mesh
  ctx->side_padding = false;
  for (int i = 0; i < t.nbf; ++i) ctx->side_padding = ctx->side_padding || d->side_elem[i] < 0;
  ctx->has_mesh = true;
  return LRBMS_OK;
}

int lrbms3_assemble_system(lrbms3_ctx* ctx, int32_t Q, const double* lam, double* A_diag, double* A_cpl, void* stream) {
  LRBMS_REQUIRE_MESH(ctx);
  if (Q < 1 || Q > 8 || !lam || !A_diag || !A_cpl) return lrbms_fail(ctx, LRBMS_E_INVALID, "assemble_system: bad argument");
  const T3& t = ctx->t;
  if (t.nT % 6) return lrbms_fail(ctx, LRBMS_E_INVALID, "assemble_system: template is not made of whole cubes");
  const dim3 grid(6 * ((t.nT / 6 + 63) / 64), t.S);
  // sides with fewer faces than the padded row length (unequal cubes per direction) leave positions no kernel writes: zero
  LRBMS_HIP_CHECK(ctx, hipMemsetAsync(A_cpl, 0, sizeof(double) * (size_t)Q * t.S * 6 * t.ncf * 100, (hipStream_t)stream));
  for (int q = 0; q < Q; ++q) {
    hipLaunchKernelGGL((k3_asm<6, 7>), grid, dim3(256), 0, (hipStream_t)stream, t, Q, q, 0, lam, (const double*)nullptr,
                       (const double*)nullptr, A_diag, (double*)nullptr);
    for (int f = 0; f < 4; ++f)
      hipLaunchKernelGGL((k3_asm<7, 7>), grid, dim3(256), 0, (hipStream_t)stream, t, Q, q, f, lam, (const double*)nullptr,
                         (const double*)nullptr, A_diag, A_cpl);
  }
  LRBMS_LAUNCH_CHECK(ctx);
  return LRBMS_OK;
}

int lrbms3_assemble_rhs(lrbms3_ctx* ctx, const double* f_smp, const double* lhat, double* b, double* f2, double* ceps,
                        double* bdiv, void* stream) {
  LRBMS_REQUIRE_MESH(ctx);
  if (!f_smp || !lhat || !b || !f2 || !ceps || !bdiv) return lrbms_fail(ctx, LRBMS_E_INVALID, "assemble_rhs: null argument");
  const T3& t = ctx->t;
  if (t.nT % 6) return lrbms_fail(ctx, LRBMS_E_INVALID, "assemble_rhs: template is not made of whole cubes");
  const dim3 grid(6 * ((t.nT / 6 + 63) / 64), t.S);
  hipLaunchKernelGGL((k3_asm<4, 1>), grid, dim3(256), 0, (hipStream_t)stream, t, 1, 0, 0, f_smp, f_smp, lhat, b, (double*)nullptr);
  hipLaunchKernelGGL((k3_asm<5, 1>), grid, dim3(256), 0, (hipStream_t)stream, t, 1, 0, 0, f_smp, f_smp, lhat, bdiv, (double*)nullptr);
  hipLaunchKernelGGL(k3_scalars, dim3(t.S), dim3(256), 0, (hipStream_t)stream, t, f_smp, lhat, f2, ceps);
  LRBMS_LAUNCH_CHECK(ctx);
  return LRBMS_OK;
}

int lrbms3_assemble_products(lrbms3_ctx* ctx, int32_t Q, const double* lam, const double* lbar, const double* lhat, double* ebar,
                             double* Aaa, double* Aab, double* Bbb, void* stream) {
  LRBMS_REQUIRE_MESH(ctx);
  if (Q < 1 || Q > 8 || !lam || !lbar || !lhat || !ebar || !Aaa || !Aab || !Bbb)
    return lrbms_fail(ctx, LRBMS_E_INVALID, "assemble_products: bad argument");
  const T3& t = ctx->t;
  if (t.nT % 6) return lrbms_fail(ctx, LRBMS_E_INVALID, "assemble_products: template is not made of whole cubes");
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(6 * ((t.nT / 6 + 63) / 64), t.S);
  hipLaunchKernelGGL((k3_asm<0, 7>), grid, dim3(256), 0, st, t, Q, 0, 0, lam, lbar, lhat, ebar, (double*)nullptr);
  const long blk = (long)t.S * t.nT * 100;
  for (int q = 0; q < Q; ++q)
    for (int q2 = q; q2 < Q; ++q2)         // A_aa[q][q'] = A_aa[q'][q]: one contraction, two stores
      hipLaunchKernelGGL((k3_asm<1, 7>), grid, dim3(256), 0, st, t, Q, q, q2, lam, lbar, lhat, Aaa + ((long)q * Q + q2) * blk,
                         q2 != q ? Aaa + ((long)q2 * Q + q) * blk : (double*)nullptr);
  for (int q = 0; q < Q; ++q)
    hipLaunchKernelGGL((k3_asm<2, 3>), grid, dim3(256), 0, st, t, Q, q, q, lam, lbar, lhat, Aab + (long)q * t.S * t.nT * 40,
                       (double*)nullptr);
  hipLaunchKernelGGL((k3_asm<3, 1>), grid, dim3(256), 0, st, t, Q, 0, 0, lam, lbar, lhat, Bbb, (double*)nullptr);
  LRBMS_LAUNCH_CHECK(ctx);
  return LRBMS_OK;
}

int lrbms3_assemble_energy_product(lrbms3_ctx* ctx, int32_t Q, const double* theta_bar, const double* lam, double* P_diag,
                                   void* stream) {
  LRBMS_REQUIRE_MESH(ctx);
  if (Q < 1 || Q > 8 || !theta_bar || !lam || !P_diag) return lrbms_fail(ctx, LRBMS_E_INVALID, "assemble_energy_product: bad argument");
  const T3& t = ctx->t;
  if (t.nT % 6) return lrbms_fail(ctx, LRBMS_E_INVALID, "assemble_energy_product: template is not made of whole cubes");
  hipStream_t st = (hipStream_t)stream;
  if (!ctx->thbar) {
    LRBMS_HIP_CHECK(ctx, hipMalloc((void**)&ctx->thbar, sizeof(double) * 8));
    ctx->owned.push_back(ctx->thbar);
  }
  double* thb = ctx->thbar;
  LRBMS_HIP_CHECK(ctx, hipMemcpyAsync(thb, theta_bar, sizeof(double) * Q, hipMemcpyHostToDevice, st));
  const dim3 grid(6 * ((t.nT / 6 + 63) / 64), t.S);
  hipLaunchKernelGGL((k3_asm<8, 7>), grid, dim3(256), 0, st, t, Q, 0, 0, lam, (const double*)nullptr, (const double*)thb, P_diag,
                     (double*)nullptr);
  for (int f = 0; f < 4; ++f)
    hipLaunchKernelGGL((k3_asm<9, 7>), grid, dim3(256), 0, st, t, Q, 0, f, lam, (const double*)nullptr, (const double*)thb, P_diag,
                       (double*)nullptr);
  LRBMS_LAUNCH_CHECK(ctx);
  LRBMS_HIP_CHECK(ctx, hipStreamSynchronize(st));          // theta_bar is a host buffer of the caller
  return LRBMS_OK;
}

int lrbms3_energy_product_apply(lrbms3_ctx* ctx, int32_t M, const double* P_diag, const double* X, double* Y, void* stream) {
  LRBMS_REQUIRE_MESH(ctx);
  if (M < 1 || !P_diag || !X || !Y) return lrbms_fail(ctx, LRBMS_E_INVALID, "energy_product_apply: bad argument");
  const T3& t = ctx->t;
  const double one = 1.0;
  hipLaunchKernelGGL(k3_fom_apply, dim3(t.nT, t.S), dim3(256), 0, (hipStream_t)stream, t, 1, M, make_theta(1, &one), P_diag,
                     (const double*)nullptr, X, Y);
  LRBMS_LAUNCH_CHECK(ctx);
  return LRBMS_OK;
}

// -- local POD basis extension (pod.hip); the product is the local energy product, applied as lrbms3_energy_product_apply does
namespace {
struct Pod3D {
  lrbms3_ctx* ctx;
  const double* P_diag;
};
int pod_product_3d(void* self, int M, const double* X, double* Y, hipStream_t st) {
  const Pod3D* a = static_cast<const Pod3D*>(self);
  return lrbms3_energy_product_apply(a->ctx, M, a->P_diag, X, Y, (void*)st);
}
}  // namespace

int64_t lrbms3_local_pod_work_size(lrbms3_ctx* ctx, int32_t L, int32_t Nw) {
  if (!ctx || !ctx->has_mesh || L < 1 || L > POD_MAX_L || Nw < 1 || Nw > POD_MAX_NW) return -1;
  return pod_work_size(ctx->t.S, ctx->t.n, L, Nw);
}

int lrbms3_local_pod(lrbms3_ctx* ctx, int32_t L, int32_t Nw, int32_t modes, double rtol, double atol, const double* P_diag,
                     const double* U, double* V, int32_t* nloc, double* sv, int32_t* added, int32_t* info, double* work,
                     void* stream) {
  LRBMS_REQUIRE_MESH(ctx);
  if (!P_diag) return lrbms_fail(ctx, LRBMS_E_INVALID, "local_pod: null pointer: P_diag");
  Pod3D self{ctx, P_diag};
  return launch_local_pod(ctx, ctx->t.S, ctx->t.n, L, Nw, modes, rtol, atol, PodProduct{pod_product_3d, &self}, U, V, nloc, sv, added,
                          info, work, (hipStream_t)stream);
}

int64_t lrbms3_local_pod_stream_state_size(lrbms3_ctx* ctx, int32_t keep, int32_t cmax) {
  if (!ctx || !ctx->has_mesh || keep < 1 || keep > POD_MAX_NW || cmax < 1 || keep + cmax > POD_MAX_L) return -1;
  return pod_stream_state_size(ctx->t.S, ctx->t.n, keep, cmax);
}

int64_t lrbms3_local_pod_stream_work_size(lrbms3_ctx* ctx, int32_t keep, int32_t cmax, int32_t Nw) {
  if (lrbms3_local_pod_stream_state_size(ctx, keep, cmax) < 0 || Nw < 1 || Nw > POD_MAX_NW) return -1;
  return pod_stream_work_size(ctx->t.S, ctx->t.n, keep, cmax, Nw);
}

int lrbms3_local_pod_stream_begin(lrbms3_ctx* ctx, int32_t keep, int32_t cmax, double* state, void* stream) {
  LRBMS_REQUIRE_MESH(ctx);
  return launch_pod_stream_begin(ctx, ctx->t.S, ctx->t.n, keep, cmax, state, (hipStream_t)stream);
}

int lrbms3_local_pod_stream_push(lrbms3_ctx* ctx, int32_t keep, int32_t cmax, int32_t C, int32_t Nw, const double* P_diag,
                                 const double* U, const double* V, const int32_t* nloc, double* state, double* work, void* stream) {
  LRBMS_REQUIRE_MESH(ctx);
  if (!P_diag) return lrbms_fail(ctx, LRBMS_E_INVALID, "local_pod_stream_push: null pointer: P_diag");
  Pod3D self{ctx, P_diag};
  return launch_pod_stream_push(ctx, ctx->t.S, ctx->t.n, keep, cmax, C, Nw, ctx->opt_pod_rotate_valu, PodProduct{pod_product_3d, &self},
                                U, V, nloc, state, work, (hipStream_t)stream);
}

int lrbms3_local_pod_stream_finish(lrbms3_ctx* ctx, int32_t keep, int32_t cmax, int32_t Nw, int32_t modes, double rtol, double atol,
                                   const double* P_diag, double* V, int32_t* nloc, double* state, double* sv, int32_t* added,
                                   int32_t* info, double* lost, double* work, void* stream) {
  LRBMS_REQUIRE_MESH(ctx);
  if (!P_diag) return lrbms_fail(ctx, LRBMS_E_INVALID, "local_pod_stream_finish: null pointer: P_diag");
  Pod3D self{ctx, P_diag};
  return launch_pod_stream_finish(ctx, ctx->t.S, ctx->t.n, keep, cmax, Nw, modes, rtol, atol, PodProduct{pod_product_3d, &self}, V, nloc,
                                  state, sv, added, info, lost, work, (hipStream_t)stream);
}

int lrbms3_assemble_flux(lrbms3_ctx* ctx, int32_t Q, const double* lam, double* Cf, void* stream) {
  LRBMS_REQUIRE_MESH(ctx);
  if (Q < 1 || Q > 8 || !lam || !Cf) return lrbms_fail(ctx, LRBMS_E_INVALID, "assemble_flux: bad argument");
  const T3& t = ctx->t;
  hipLaunchKernelGGL(k3_assemble_flux, dim3(t.nT, t.S_ext, Q), dim3(64), 0, (hipStream_t)stream, t, lam, Cf);
  LRBMS_LAUNCH_CHECK(ctx);
  return LRBMS_OK;
}

int64_t lrbms3_work_size(lrbms3_ctx* ctx, int32_t Q, int32_t N) {
  if (!ctx || !ctx->has_mesh) return -1;
  const T3& t = ctx->t;
  return (int64_t)t.S * t.nrt * Q * N + (int64_t)t.S * t.nnodes * N + (int64_t)t.S * t.nbd * N;
}

int lrbms3_project_estimate(lrbms3_ctx* ctx, int32_t Q, int32_t N, const double* V, const double* A_diag, const double* A_cpl,
                            const double* b, const double* ebar, const double* Aaa, const double* Aab, const double* Bbb,
                            const double* bdiv, const double* Cf, double* work, double* B_sys, double* rhs_red, double* G_nc,
                            double* G_bb, double* G_rdd, double* G_ab, double* G_aa, double* r_fd, double* Rb, double* Yb,
                            double* Dp, double* Xab, double* As, double* Cn, void* stream) {
  return lrbms3_project_estimate_phase(ctx, 0, Q, N, V, A_diag, A_cpl, b, ebar, Aaa, Aab, Bbb, bdiv, Cf, work, B_sys, rhs_red, G_nc,
                                       G_bb, G_rdd, G_ab, G_aa, r_fd, Rb, Yb, Dp, Xab, As, Cn, stream);
}

int lrbms3_project_estimate_phase(lrbms3_ctx* ctx, int32_t phase, int32_t Q, int32_t N, const double* V, const double* A_diag,
                                  const double* A_cpl, const double* b, const double* ebar, const double* Aaa, const double* Aab,
                                  const double* Bbb, const double* bdiv, const double* Cf, double* work, double* B_sys,
                                  double* rhs_red, double* G_nc, double* G_bb, double* G_rdd, double* G_ab, double* G_aa,
                                  double* r_fd, double* Rb, double* Yb, double* Dp, double* Xab, double* As, double* Cn, void* stream) {
  LRBMS_REQUIRE_MESH(ctx);
  if (phase < 0 || phase > 2) return lrbms_fail(ctx, LRBMS_E_INVALID, "project_estimate: phase must be 0, 1 or 2");
  const bool own = phase != 2, side = phase != 1;        // 1: everything that reads rank-local slabs only; 2: the rest
  if (Q < 1 || Q > 8 || N < 1 || N > 64 || Q * N > 64)
    return lrbms_fail(ctx, LRBMS_E_INVALID, "project_estimate: needs N <= 64 and Q N <= 64");
  if (!V || !A_diag || !A_cpl || !b || !ebar || !Aaa || !Aab || !Bbb || !bdiv || !Cf || !work || !B_sys || !rhs_red || !G_nc ||
      !G_bb || !G_rdd || !G_ab || !G_aa || !r_fd || !Rb || !Yb || !Dp || !Xab || !As || !Cn)
    return lrbms_fail(ctx, LRBMS_E_INVALID, "project_estimate: null argument");
  const T3& t = ctx->t;
  hipStream_t st = (hipStream_t)stream;
  ctx->ktime_n = ctx->ktime ? ctx->ktime_n : 0;
  double* Rs = work;
  double* Avg = work + (long)t.S * t.nrt * Q * N;
  double* Zb = Avg + (long)t.S * t.nnodes * N;
  // Three independent chains, each on its own stream so that the latency-bound preparation kernels run beside the MFMA kernels:
  //   caller's stream  B_sys (diagonal + coupling blocks), G_aa, rhs_red         -- need nothing but V and the element blocks
  //   aux 0            flux image  ->  G_ab, G_bb, G_rdd, r_fd, side-face factors
  //   aux 1            node averages  ->  G_nc, side-node factors
  // (while per-kernel timing is on, everything runs on the caller's stream: overlapping kernels would stretch each other's
  // event intervals)
  const bool serial = ctx->ktime || ctx->opt_serial != 0;      // LRBMS3_OPT_SERIAL: rocprofv3 kernel statistics of a serial pass
  hipStream_t sf = serial ? st : ctx->aux[0], sn = serial ? st : ctx->aux[1];
  LRBMS_HIP_CHECK(ctx, hipEventRecord(ctx->ev_fork, st));
  LRBMS_HIP_CHECK(ctx, hipStreamWaitEvent(sf, ctx->ev_fork, 0));
  LRBMS_HIP_CHECK(ctx, hipStreamWaitEvent(sn, ctx->ev_fork, 0));
  // Restricted pass (lrbms3_pass_set_subset): everything phase 1 launches runs over the own list, everything phase 2 launches over
  // the side list; a null list is the whole pass, launched exactly as without the feature.
  const bool sub = ctx->sub_active;
  const int* l_own = sub ? ctx->sub_own : nullptr;
  const int* l_side = sub ? ctx->sub_side : nullptr;
  const int n_own = sub ? ctx->sub_own_n : t.S, n_side = sub ? ctx->sub_side_n : t.S;
  GA a{t, Q, N, V, A_diag, A_cpl, ebar, Aaa, Aab, Bbb, Rs, Avg, nullptr, Zb, G_rdd, r_fd, bdiv, b, rhs_red, Yb, Dp, Xab, 1, nullptr, l_own, n_own};
  if (own && ctx->side_padding && !sub) {      // padded side-face rows are written by no kernel: define them (the estimate multiplies them by 0)
    LRBMS_HIP_CHECK(ctx, hipMemsetAsync(Yb, 0, sizeof(double) * (size_t)t.S * t.nbf * Q * N, sf));
    LRBMS_HIP_CHECK(ctx, hipMemsetAsync(Dp, 0, sizeof(double) * (size_t)t.S * t.nbf * Q * N, sf));
    LRBMS_HIP_CHECK(ctx, hipMemsetAsync(Xab, 0, sizeof(double) * (size_t)Q * t.S * t.nbf * N, sf));
  }
  if (own && ctx->side_padding && sub && n_own > 0)      // ... of the listed subdomains only: every other row keeps its bits
    hipLaunchKernelGGL(k3_zero_side_rows, dim3(n_own), dim3(256), 0, sf, t, Q, N, l_own, Yb, Dp, Xab);
  const int tn = (N + 15) / 16, tq = (Q * N + 15) / 16;
  const int nw_env = ctx->opt_waves;      // LRBMS3_OPT_WAVES
  const int nw = nw_env > 0 ? nw_env : 4;
  const int nw_s = nw_env > 0 ? nw_env : 8;      // kernels with one workgroup per subdomain only: more waves each
  int bad = 0;
  // own faces | side faces (the neighbours' share: halo), own nodes | side nodes: one launch over both row ranges for the whole
  // pass, one launch per range and list for a restricted one (unless both lists are the same: all subdomains changed ran 3.5 %
  // behind the whole pass with the split launches)
  auto flux = [&](int r0, int r1, const int* list, int cnt, const char* name) {
    if (cnt <= 0) return;
    KScope k(ctx, name, sf);
    hipLaunchKernelGGL(k3_flux, dim3(xcd_grid((r1 - r0 + 4 * FLUX_R * FLUX_LOOP - 1) / (4 * FLUX_R * FLUX_LOOP), cnt)), dim3(256), 0, sf, t, Q, N, r0, r1, list, cnt, V, Cf, Rs, Rb);
  };
  auto node_avg = [&](int r0, int r1, const int* list, int cnt, const char* name) {
    if (cnt <= 0) return;
    KScope k(ctx, name, sn);
    hipLaunchKernelGGL(k3_node_avg, dim3(xcd_grid((r1 - r0 + 4 * NODE_LOOP - 1) / (4 * NODE_LOOP), cnt)), dim3(256), 0, sn, t, N, r0, r1, list, cnt, V, Avg, As);
  };
  if (!sub || (own && side && n_own == n_side)) {      // (own list within the side list: equal lengths mean equal lists)
    flux(own ? 0 : t.nrt, side ? t.nrt + t.nbf : t.nrt, l_own, n_own, own ? "k3_flux" : "k3_flux<side>");
    node_avg(own ? 0 : t.nnodes, side ? t.nnodes + 6 * t.nvs : t.nnodes, l_own, n_own, own ? "k3_node_avg" : "k3_node_avg<side>");
  } else {
    if (own) flux(0, t.nrt, l_own, n_own, "k3_flux");
    if (side) flux(t.nrt, t.nrt + t.nbf, l_side, n_side, "k3_flux<side>");
    if (own) node_avg(0, t.nnodes, l_own, n_own, "k3_node_avg");
    if (side) node_avg(t.nnodes, t.nnodes + 6 * t.nvs, l_side, n_side, "k3_node_avg<side>");
  }
  const int npair = Q * (Q + 1) / 2;       // A_aa: pairs q <= q', the transposed blocks are written from the same accumulators
  // K-split for small per-rank subdomain counts (the 4 x 4 x 4 tile of an 8-GPU run has 64): one workgroup per (subdomain,
  // operator) would leave most of the 256 CUs idle, so the element range is dealt to ksplit workgroups and k3_pg_combine sums
  // their partial results in a fixed order.  Off (ksplit = 1, no extra launch) from ~400 workgroups per kernel on.  A restricted
  // pass counts the LISTED subdomains: 16 of 512 still fill the chip through the partial tiles, which are indexed by position.
  const int ks_env = ctx->opt_ksplit;      // LRBMS3_OPT_KSPLIT
  // target workgroups per launch, measured on the 4 x 4 x 4 tile of an 8-GPU run (64 subdomains; LRBMS3_OPT_KSPLIT 2 / 4 / 6 / auto):
  // the kernels with ONE workgroup per subdomain and ~240 VGPRs (BB: 4 waves, NC: 8 waves) want one workgroup per CU (k3_pg<BB>
  // 104 us at 256 workgroups, 124 at 512; <NC> 44 vs 51), G_aa three per CU (70 us at 768, 85 at 576), the others two
  auto ksplit_of = [&](int nblocks, int target) {
    if (nblocks <= 0) return 1;      // an empty list: nothing is launched
    if (ks_env > 0) return ks_env < 8 ? ks_env : 8;
    if (nblocks >= 384) return 1;
    const int k = (target + nblocks - 1) / nblocks;
    return k < 1 ? 1 : (k < 8 ? k : 8);
  };
  const int QNl = Q * N;
  const int ks_sys = ksplit_of(Q * n_own, 512), ks_aaa = ksplit_of(npair * n_own, 768), ks_nc = ksplit_of(n_own, 256), ks_ab = ksplit_of(Q * n_own, 512),
            ks_bb = ksplit_of(n_own, 256), ks_cpl = ksplit_of(Q * n_side * 6, 512);
  const long need_sys = ks_sys > 1 ? (long)Q * n_own * ks_sys * pg_part_size<G_SYS>(N, QNl) : 0,
             need_aaa = ks_aaa > 1 ? (long)npair * n_own * ks_aaa * pg_part_size<G_AAA>(N, QNl) : 0,
             need_nc = ks_nc > 1 ? (long)n_own * ks_nc * pg_part_size<G_NC>(N, QNl) : 0,
             need_ab = ks_ab > 1 ? (long)Q * n_own * ks_ab * pg_part_size<G_AB>(N, QNl) : 0,
             need_bb = ks_bb > 1 ? (long)n_own * ks_bb * pg_part_size<G_BB>(N, QNl) : 0,
             need_cpl = ks_cpl > 1 ? (long)Q * n_side * 6 * ks_cpl * pg_part_size<G_CPL>(N, QNl) : 0;
  const long need = need_sys + need_aaa + need_nc + need_ab + need_bb + need_cpl;
  if (need > ctx->pg_part_cap) {
    LRBMS_HIP_CHECK(ctx, hipDeviceSynchronize());
    if (ctx->pg_part) (void)hipFree(ctx->pg_part);
    ctx->pg_part = nullptr;
    ctx->pg_part_cap = 0;
    LRBMS_HIP_CHECK(ctx, hipMalloc((void**)&ctx->pg_part, sizeof(double) * need));
    ctx->pg_part_cap = need;
  }
  double* part_sys = ctx->pg_part;
  double* part_aaa = part_sys + need_sys;
  double* part_nc = part_aaa + need_aaa;
  double* part_ab = part_nc + need_nc;
  double* part_bb = part_ab + need_ab;
  double* part_cpl = part_bb + need_bb;
  // (launch order measured: the MFMA-bound G_aa kernel first on the caller's stream, beside the latency-bound preparation
  // kernels of the other two chains, the HBM-bound system kernel after it: 2.39 -> 2.29 ms; a fourth stream for G_aa: slower)
  if (own && n_own > 0) {
    KScope k(ctx, "k3_pg<AAA>", st);
    a.ksplit = ks_aaa;
    a.part = part_aaa;
    a.out = G_aa;
    bad |= dispatch_pg<G_AAA>(a, npair * n_own, tn, tn, nw, st);
  }
  if (own && n_own > 0) {
    KScope k(ctx, "k3_pg<SYS>", st);
    a.ksplit = ks_sys;
    a.part = part_sys;
    a.out = B_sys;
    bad |= dispatch_pg<G_SYS>(a, Q * n_own, tn, tn, nw, st);
  }
  if (own && n_own > 0) {
    KScope k(ctx, "k3_pg<AB>", sf);
    a.ksplit = ks_ab;
    a.part = part_ab;
    a.out = G_ab;
    bad |= dispatch_pg<G_AB>(a, Q * n_own, tn, tq, nw, sf);
  }
  if (own && n_own > 0) {
    KScope k(ctx, "k3_pg<NC>", sn);
    a.ksplit = ks_nc;
    a.part = part_nc;
    a.out = G_nc;
    bad |= dispatch_pg<G_NC>(a, n_own, tn, tn, nw_s, sn);
  }
  if (own && n_own > 0) {
    KScope k(ctx, "k3_pg<BB>", sf);
    a.ksplit = ks_bb;
    a.part = part_bb;
    a.out = G_bb;
    bad |= dispatch_pg<G_BB>(a, n_own, tq, tq, nw, sf);          // 4 waves: 291 us, 8 waves: 307 us (tools/nw_sweep.sh)
  }
  if (own && n_own > 0) {
    KScope k(ctx, "k3_side_nc", sn);
    hipLaunchKernelGGL(k3_side_nc, dim3((t.nb + 3) / 4, n_own), dim3(256), 0, sn, t, N, l_own, Zb, Cn);
  }
  if (side && n_side > 0) {
    KScope k(ctx, "k3_pg<CPL>", st);
    a.ksplit = ks_cpl;
    a.part = part_cpl;
    a.out = B_sys;
    a.list = l_side;
    a.nlist = n_side;
    bad |= dispatch_pg<G_CPL>(a, Q * n_side * 6, tn, tn, nw, st);
  }
  if (bad) return lrbms_fail(ctx, LRBMS_E_INVALID, "project_estimate: unsupported tile shape");
  LRBMS_HIP_CHECK(ctx, hipEventRecord(ctx->ev_join[0], sf));
  LRBMS_HIP_CHECK(ctx, hipEventRecord(ctx->ev_join[1], sn));
  LRBMS_HIP_CHECK(ctx, hipStreamWaitEvent(st, ctx->ev_join[0], 0));
  LRBMS_HIP_CHECK(ctx, hipStreamWaitEvent(st, ctx->ev_join[1], 0));
  LRBMS_LAUNCH_CHECK(ctx);
  return LRBMS_OK;
}

int lrbms3_pass_set_subset(lrbms3_ctx* ctx, const int32_t* changed, int32_t count) {
  if (!ctx) return LRBMS_E_INVALID;
  if (!ctx->has_mesh) return lrbms_fail(ctx, LRBMS_E_INVALID, "pass_set_subset: mesh not uploaded");
  const T3& t = ctx->t;
  if (count < 0) return lrbms_fail(ctx, LRBMS_E_INVALID, "pass_set_subset: count must not be negative");
  if (count == 0) {
    ctx->sub_active = false;
    return LRBMS_OK;
  }
  if (!changed) return lrbms_fail(ctx, LRBMS_E_INVALID, "pass_set_subset: null list with count > 0");
  for (int i = 0; i < count; ++i) {
    if (changed[i] < 0 || changed[i] >= t.S_ext)
      return lrbms_fail(ctx, LRBMS_E_INVALID, "pass_set_subset: index " + std::to_string(changed[i]) + " out of range [0, S_ext)");
    if (i > 0 && changed[i] <= changed[i - 1])
      return lrbms_fail(ctx, LRBMS_E_INVALID, "pass_set_subset: the list must be strictly ascending");
  }
  // own list: the changed local subdomains; side list: the local subdomains that are changed or see a changed slab (local or
  // halo) through a face -- from the host copy of the neighbour table
  std::vector<char> hit((size_t)t.S_ext, 0);
  for (int i = 0; i < count; ++i) hit[changed[i]] = 1;
  std::vector<int32_t> lown, lside;
  for (int s = 0; s < t.S; ++s) {
    if (hit[s]) lown.push_back(s);
    bool touched = false;
    for (int k = 0; k < 7; ++k) {
      const int s2 = ctx->nbr_host[(size_t)s * 7 + k];
      touched = touched || (s2 >= 0 && hit[s2]);
    }
    if (touched) lside.push_back(s);
  }
  if (!ctx->sub_own) {
    void* p = nullptr;
    LRBMS_HIP_CHECK(ctx, hipMalloc(&p, sizeof(int) * 2 * (size_t)t.S));
    ctx->owned.push_back(p);
    ctx->sub_own = static_cast<int*>(p);
    ctx->sub_side = ctx->sub_own + t.S;
  }
  // synchronous copies: the lists a pass still in flight reads must not change under it, and `changed` may go away after return
  LRBMS_HIP_CHECK(ctx, hipDeviceSynchronize());
  if (!lown.empty()) LRBMS_HIP_CHECK(ctx, hipMemcpy(ctx->sub_own, lown.data(), sizeof(int) * lown.size(), hipMemcpyHostToDevice));
  if (!lside.empty()) LRBMS_HIP_CHECK(ctx, hipMemcpy(ctx->sub_side, lside.data(), sizeof(int) * lside.size(), hipMemcpyHostToDevice));
  ctx->sub_own_n = (int)lown.size();
  ctx->sub_side_n = (int)lside.size();
  ctx->sub_active = true;
  return LRBMS_OK;
}

int lrbms3_kernel_timing(lrbms3_ctx* ctx, int32_t enable) { return lrbms_ctx_kernel_timing(ctx, enable); }

int lrbms3_kernel_timing_read(lrbms3_ctx* ctx, char* names, int64_t names_cap, double* ms, int32_t cap, int32_t* count) {
  return lrbms_ctx_kernel_timing_read(ctx, names, names_cap, ms, cap, count);
}

int lrbms3_reduced_estimate(lrbms3_ctx* ctx, int32_t Q, int32_t N, const double* theta, const double* u, const double* G_nc,
                            const double* G_bb, const double* G_rdd, const double* G_ab, const double* G_aa, const double* r_fd,
                            const double* Rb, const double* Yb, const double* Dp, const double* Xab, const double* As,
                            const double* Cn, const double* ebar, const double* Bbb, const double* bdiv, const double* f2,
                            const double* ceps, double hdiam, double* eta_loc, void* stream) {
  LRBMS_REQUIRE_MESH(ctx);
  if (Q < 1 || Q > 8 || N < 1 || Q * N > 64 || !theta || !u || !eta_loc)
    return lrbms_fail(ctx, LRBMS_E_INVALID, "reduced_estimate: bad argument");
  const T3& t = ctx->t;
  EA a{u, G_nc, G_bb, G_rdd, G_ab, G_aa, r_fd, Rb, Yb, Dp, Xab, As, Cn, ebar, Bbb, bdiv, f2, ceps, hdiam, eta_loc};
  const size_t lds = sizeof(double) * (7 * N + Q * N + t.nbf + t.nb + 256);
  if (lds > 64 * 1024) return lrbms_fail(ctx, LRBMS_E_INVALID, "reduced_estimate: template too large for the LDS");
  hipLaunchKernelGGL(k3_estimate, dim3(t.S), dim3(256), lds, (hipStream_t)stream, t, Q, N, make_theta(Q, theta), a);
  LRBMS_LAUNCH_CHECK(ctx);
  return LRBMS_OK;
}

int lrbms3_reduced_estimate_batch(lrbms3_ctx* ctx, int32_t Q, int32_t N, int32_t nmu, const double* theta, const double* u,
                                  const double* G_nc, const double* G_bb, const double* G_rdd, const double* G_ab, const double* G_aa,
                                  const double* r_fd, const double* Rb, const double* Yb, const double* Dp, const double* Xab,
                                  const double* As, const double* Cn, const double* ebar, const double* Bbb, const double* bdiv,
                                  const double* f2, const double* ceps, double hdiam, double* eta_loc, void* stream) {
  LRBMS_REQUIRE_MESH(ctx);
  if (Q < 1 || Q > 8 || N < 1 || Q * N > 64 || nmu < 1 || !theta || !u || !eta_loc)
    return lrbms_fail(ctx, LRBMS_E_INVALID, "reduced_estimate_batch: bad argument");
  const EA a{u, G_nc, G_bb, G_rdd, G_ab, G_aa, r_fd, Rb, Yb, Dp, Xab, As, Cn, ebar, Bbb, bdiv, f2, ceps, hdiam, eta_loc};
  return launch_reduced_estimate_batch(ctx, (hipStream_t)stream, Q, N, nmu, theta, a);
}

int lrbms3_fom_coarse_space(lrbms3_ctx* ctx, int32_t nc, const double* Phi) {
  LRBMS_REQUIRE_MESH(ctx);
  if (nc < 0 || nc > 4 || (nc > 0 && !Phi)) return lrbms_fail(ctx, LRBMS_E_INVALID, "fom_coarse_space: 0 <= nc <= 4 functions, Phi [n][nc]");
  if (!ctx->has_mesh) return lrbms_fail(ctx, LRBMS_E_STATE, "fom_coarse_space: upload the mesh first");
  const T3& t = ctx->t;
  ctx->fom_nc = 0;
  ctx->fom_pc_M = 0;                     // a kept coarse inverse belongs to the old space
  if (nc == 0) return LRBMS_OK;
  std::vector<double> padded((size_t)t.n * 4, 0.0);
  for (long d = 0; d < t.n; ++d)
    for (int k = 0; k < nc; ++k) padded[d * 4 + k] = Phi[d * nc + k];
  if (!ctx->fom_phi) {
    LRBMS_HIP_CHECK(ctx, hipMalloc((void**)&ctx->fom_phi, sizeof(double) * (size_t)t.n * 4));
    ctx->owned.push_back(ctx->fom_phi);
  }
  LRBMS_HIP_CHECK(ctx, hipMemcpy(ctx->fom_phi, padded.data(), sizeof(double) * padded.size(), hipMemcpyHostToDevice));
  ctx->fom_nc = nc;
  return LRBMS_OK;
}

int lrbms3_fom_precond_keep(lrbms3_ctx* ctx, int32_t keep) {
  LRBMS_REQUIRE_MESH(ctx);
  ctx->fom_keep = keep != 0;
  if (!keep) {
    if (ctx->fom_pc) (void)hipFree(ctx->fom_pc);
    ctx->fom_pc = nullptr;
    ctx->fom_pc_M = 0;
  }
  return LRBMS_OK;
}

int64_t lrbms3_fom_solve_work_size(lrbms3_ctx* ctx) {
  if (!ctx || !ctx->has_mesh) return -1;
  const T3& t = ctx->t;
  const int64_t nblk = (int64_t)t.S * ((t.nT + FOM_EPB - 1) / FOM_EPB), M = std::min<int64_t>(4 * (int64_t)t.S, FOM_MAX_COARSE);
  return (int64_t)t.S * t.nT * 500 + (int64_t)t.S * 6 * t.ncf * 100 + (int64_t)t.S * t.nT * 100 + 4 * (int64_t)t.S * t.n + 3 * nblk + 16 +
         M + 4 * nblk + 2 * M + (int64_t)t.S * 112 + 2 * M * M + 2;       // coarse level: prc, pr0, r0, y0, blocks, A1, A1inv, info
}

}  // extern "C"

namespace {

// work layout of the full-order CG (lrbms3_fom_solve_work_size doubles; lrbms3_fom_implicit_euler appends its own buffers)
struct FomWork {
  int nbx;
  long nblk, Mmax;
  double *Amu, *Cmu, *Dinv, *r, *z, *p, *y, *prz, *prc, *ppy, *prr, *scal, *pr0, *r0, *y0, *A1b, *A1, *A1inv;
  rocblas_int* pinfo;
};

FomWork fom_work(const T3& t, double* work) {
  FomWork w;
  const long S = t.S, nd = S * t.nT * 500, ncp = S * 6 * t.ncf * 100, total = S * t.n;
  w.nbx = (t.nT + FOM_EPB - 1) / FOM_EPB;
  w.nblk = S * w.nbx;
  w.Mmax = std::min<long>(4 * S, FOM_MAX_COARSE);
  w.Amu = work;
  w.Cmu = w.Amu + nd;
  w.Dinv = w.Cmu + ncp;
  w.r = w.Dinv + S * t.nT * 100;
  w.z = w.r + total;
  w.p = w.z + total;
  w.y = w.p + total;
  w.prz = w.y + total;
  w.prc = w.prz + w.nblk;              // coarse contributions to r.z: summed with prz by ONE reduction
  w.ppy = w.prc + w.Mmax;
  w.prr = w.ppy + w.nblk;
  w.scal = w.prr + w.nblk;
  w.pr0 = w.scal + 16;
  w.r0 = w.pr0 + 4 * w.nblk;
  w.y0 = w.r0 + w.Mmax;
  w.A1b = w.y0 + w.Mmax;
  w.A1 = w.A1b + S * 112;
  w.A1inv = w.A1 + w.Mmax * w.Mmax;
  w.pinfo = (rocblas_int*)(w.A1inv + w.Mmax * w.Mmax);
  return w;
}

// Coarse level of the two-level preconditioner on the operator in w.Amu / w.Cmu (LRBMS3_OPT_FOM_COARSE 0 switches it off).
// shared_pc: the elliptic solves' kept inverse (lrbms3_fom_precond_keep) may be used and is refreshed; false: a private one
// in the work buffer, the context's is neither read nor replaced.  Out: nc (0 = block-Jacobi alone) and the dense inverse.
int fom_coarse(lrbms3_ctx* ctx, hipStream_t st, FomWork& w, bool shared_pc, int& nc_out, const double*& A1inv_out) {
  const T3& t = ctx->t;
  const long S = t.S;
  double* A1inv = w.A1inv;
  const bool coarse_env = ctx->opt_fom_coarse != 0;
  int nc = coarse_env ? ctx->fom_nc : 0;
  if (nc > 1 && (long)nc * S > FOM_MAX_COARSE) nc = 1;       // the dense coarse inverse is capped: constants instead of P1, then none
  if ((long)nc * S > FOM_MAX_COARSE) nc = 0;
  const double* Phi = ctx->fom_phi;
  const long M = (long)nc * S;
  const bool kept = shared_pc && nc > 0 && ctx->fom_keep && ctx->fom_pc && ctx->fom_pc_M == M && ctx->fom_pc_nc == nc;
  if (kept) A1inv = ctx->fom_pc;          // built by an earlier solve (another parameter: any SPD preconditioner is admissible)
  if (nc > 0 && !kept) {
    hipLaunchKernelGGL(k3f_coarse_blocks, dim3(S), dim3(256), 0, st, t, Phi, w.Amu, w.Cmu, w.A1b);
    LRBMS_HIP_CHECK(ctx, hipMemsetAsync(w.A1, 0, sizeof(double) * 2 * M * M, st));             // A1 and the identity behind it (A1inv at M * M when nc = 4)
    double* Id = w.A1 + M * M;
    hipLaunchKernelGGL(k3f_coarse_dense, dim3((unsigned)((std::max(M, S * 112) + 255) / 256)), dim3(256), 0, st, t, nc, w.A1b, w.A1, Id);
    LRBMS_LAUNCH_CHECK(ctx);
    rocblas_int hinfo = 0;
    if (int rc = dense_spd_inverse(ctx, st, M, w.A1, Id, w.pinfo, hinfo)) return rc;
    if (hinfo != 0) nc = 0;                                   // not positive definite (dependent functions): block-Jacobi alone
    A1inv = Id;
    if (shared_pc && nc > 0 && ctx->fom_keep) {
      if (ctx->fom_pc && ctx->fom_pc_M != M) {
        LRBMS_HIP_CHECK(ctx, hipFree(ctx->fom_pc));
        ctx->fom_pc = nullptr;
      }
      ctx->fom_pc_M = 0;
      if (!ctx->fom_pc) LRBMS_HIP_CHECK(ctx, hipMalloc((void**)&ctx->fom_pc, sizeof(double) * M * M));
      LRBMS_HIP_CHECK(ctx, hipMemcpyAsync(ctx->fom_pc, Id, sizeof(double) * M * M, hipMemcpyDeviceToDevice, st));
      ctx->fom_pc_M = M;
      ctx->fom_pc_nc = nc;
    }
  }
  nc_out = nc;
  A1inv_out = A1inv;
  return LRBMS_OK;
}

// Preconditioned CG on the operator in w (element-block inverses in w.Dinv, coarse level nc / A1inv of fom_coarse) from x = 0.
// The relative residual is taken against |b|, or against the device scalar bref (squared norm) when it is given and non-zero:
// a warm-started solve hands in the correction's right-hand side b - K x0 and the norm of the full right-hand side.
int fom_cg(lrbms3_ctx* ctx, hipStream_t st, FomWork& w, int nc, const double* A1inv, const double* b, double* x, double rtol,
           int max_iter, double* info, const double* bref, const char* name) {
  const T3& t = ctx->t;
  const long S = t.S, total = S * t.n, nblk = w.nblk, M = (long)nc * S;
  const int nbx = w.nbx;
  const double* Phi = ctx->fom_phi;
  double *Amu = w.Amu, *Cmu = w.Cmu, *Dinv = w.Dinv, *r = w.r, *z = w.z, *p = w.p, *y = w.y, *prz = w.prz, *prc = w.prc;
  double *ppy = w.ppy, *prr = w.prr, *scal = w.scal, *pr0 = w.pr0, *r0 = w.r0, *y0 = w.y0;
  const long nrz = nblk + (nc > 0 ? M : 0);
  auto coarse = [&]() {
    if (nc == 0) return;
    hipLaunchKernelGGL(k3f_coarse_r0, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, st, (int)S, nbx, nc, pr0, r0);
    hipLaunchKernelGGL(k3f_coarse_apply, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, st, (int)M, A1inv, r0, y0, prc);
  };
  const dim3 grid(nbx, S);
  hipLaunchKernelGGL(k3f_update, grid, dim3(256), 0, st, t, 1, 0, scal, Dinv, p, y, b, x, r, z, prz, prr, nc, Phi, pr0);
  coarse();
  hipLaunchKernelGGL(k3_reduce1, dim3(1), dim3(256), 0, st, (int)nrz, prz, scal + 0);
  hipLaunchKernelGGL(k3_reduce1, dim3(1), dim3(256), 0, st, (int)nblk, prr, scal + 4);
  LRBMS_LAUNCH_CHECK(ctx);
  double bb = 0.0, bn = 0.0;
  LRBMS_HIP_CHECK(ctx, hipMemcpyAsync(&bb, scal + 4, sizeof(double), hipMemcpyDeviceToHost, st));
  if (bref) LRBMS_HIP_CHECK(ctx, hipMemcpyAsync(&bn, bref, sizeof(double), hipMemcpyDeviceToHost, st));
  LRBMS_HIP_CHECK(ctx, hipStreamSynchronize(st));
  if (info) info[0] = 0, info[1] = 0;
  if (bb == 0.0) return LRBMS_OK;
  const double den = bn > 0.0 ? bn : bb;
  int it = 0;
  double rel = 1.0;
  const int check = 16;
  while (it < max_iter) {
    for (int k = 0; k < check && it < max_iter; ++k, ++it) {
      const int cur = it & 1;                       // slot of the current r.z (the update of this iteration writes the other one)
      hipLaunchKernelGGL(k3f_dir, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, total, it == 0 ? 1 : 0, cur, scal, z, p, t.n, nc,
                         Phi, y0);
      hipLaunchKernelGGL(k3f_matvec, dim3(xcd_grid(nbx, (int)S)), dim3(256), 0, st, t, nbx, Amu, Cmu, p, y, ppy);
      hipLaunchKernelGGL(k3_reduce1, dim3(1), dim3(256), 0, st, (int)nblk, ppy, scal + 2);
      hipLaunchKernelGGL(k3f_update, grid, dim3(256), 0, st, t, 0, cur, scal, Dinv, p, y, b, x, r, z, prz, prr, nc, Phi, pr0);
      coarse();
      hipLaunchKernelGGL(k3_reduce1, dim3(1), dim3(256), 0, st, (int)nrz, prz, scal + (cur ^ 1));
    }
    hipLaunchKernelGGL(k3_reduce1, dim3(1), dim3(256), 0, st, (int)nblk, prr, scal + 3);
    LRBMS_LAUNCH_CHECK(ctx);
    double rr = 0.0;
    LRBMS_HIP_CHECK(ctx, hipMemcpyAsync(&rr, scal + 3, sizeof(double), hipMemcpyDeviceToHost, st));
    LRBMS_HIP_CHECK(ctx, hipStreamSynchronize(st));
    rel = sqrt(rr / den);
    if (!(rel == rel)) return lrbms_fail(ctx, LRBMS_E_NOT_CONVERGED, std::string(name) + ": NaN residual");
    if (rel <= rtol) break;
  }
  if (info) info[0] = it, info[1] = rel;
  if (rel > rtol) return lrbms_fail(ctx, LRBMS_E_NOT_CONVERGED, std::string(name) + ": not converged");
  return LRBMS_OK;
}

// ------------------------------------------------------------------------------------------------- batched snapshots
// lrbms3_fom_solve_batch: up to 64 parameters per call in panels of 16 columns.  Column m solves
// (sum_q theta[m][q] A_q) x_m = sum_j phi[m][j] b_K[j] from x = 0; the panel vectors r, z, p, y are [S n][16] (column fastest: the
// 16 lanes of a matrix-core operand row read 128 contiguous bytes), x lives in the caller's X [S][n][nmu].  There is no combined
// operator per column: k3fb_matvec reads the Q uncombined blocks once per iteration for all 16 columns and folds the column's
// theta into the direction operand.  ONE preconditioner per call, both levels at the mean theta of the call (k3_combine,
// k3f_block_inverse, fom_coarse with a private inverse).  Per iteration
//   k3fb_dir           p = z + R0^T y0 + beta p                          (beta = rz' / rz per column, 0 when rz = 0)
//   k3fb_matvec        y = A(theta_m) p on the fp64 matrix cores, p.y per workgroup and column
//   k3fb_scalars       pAp per column
//   k3fb_update        alpha = rz / pAp (0 when pAp = 0), x += alpha p, r -= alpha y, z = Dinv r (matrix cores), per workgroup and
//                      column r.z, r.r and the nc restriction sums phi_k . r
//   k3fb_coarse_r0 + k3fb_coarse_apply   r0, y0 = A1inv r0, the coarse parts of r.z          (coarse level only)
//   k3fb_scalars       rz per column
// Every sum has a fixed order that depends on the mesh alone and no atomics are used: repeat calls give the same bits, and a
// column's bits do not depend on its place in the panel (a lane owns one column: li = lane & 15).  Columns >= P of the panel
// vectors are neither loaded nor stored.  scal [5][16]: rz (two alternating slots), pAp, rr, bb.
//
// Matrix-core tiles (v_mfma_f64_16x16x4): A operand lane l = M[row l & 15][k = (l >> 4) + 4 ks], B operand lane l =
// V[k = (l >> 4) + 4 ks][column l & 15], result register r of lane l = (row (l >> 4) + 4 r, column l & 15).  The 10 x 10 blocks
// are padded to 16 x 12 with zeros in the operand, never in memory.

// The five blocks of element e's block row: where the q = 0 block lies, its stride over q, whether it is used transposed, and the
// first entry of the direction it multiplies (nullptr: no block -- a physical boundary face).
struct Fb3Row {
  const double* src[5];
  const double* pb[5];
  long qs[5];
  bool tr[5];
};

// y = A(theta_m) p for the 16 columns of a panel.  One wave per element at a time, four waves per workgroup, FOM_EPB elements per
// workgroup, all workgroups of a subdomain on one XCD (xcd_block).  Per (element, q) the wave moves its five blocks from global
// memory into the LDS with ONE 16-byte load per lane and block (50 lanes, 800 contiguous bytes) and reads the operand order of
// the matrix cores from there; inside a subdomain the block towards the lower-index neighbour is that element's block read
// transposed from the LDS (k3f_matvec's symmetric read: the second reader finds it in the XCD's L2).  The column's theta_q
// multiplies the direction operand, every (block, q) adds three k-steps to the ONE accumulator tile of the element.
// MASS: the step operator of the implicit Euler, M + A(theta) with theta pre-multiplied by dt (lrbms3_fom_implicit_euler_batch).
// The element's mass block TM, unweighted, joins its own block: three more k-steps on the same accumulator tile whose direction
// operand is the plain pv[0][ks].  The TM blocks of all six element types are staged in the LDS once per workgroup.
template <bool MASS>
__global__ __launch_bounds__(256) void k3fb_matvec(T3 t, int nbx, int Q, int P, TB th, const double* __restrict__ A_diag,
                                                   const double* __restrict__ A_cpl, const double* __restrict__ p,
                                                   double* __restrict__ y, double* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) double blk[4][5][104];
  __shared__ double ths[128];
  __shared__ double red[4][16];
  __shared__ double tms[MASS ? 600 : 1];
  int s, bx;
  if (!xcd_block(nbx, t.S, bx, s)) return;
  const int tid = threadIdx.x, lane = tid & 63, li = lane & 15, lk = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  if (tid < 128) ths[tid] = th.v[tid >> 3][tid & 7];
  if (MASS)
    for (int i = tid; i < 600; i += 256) tms[i] = t.TM[i];
  __syncthreads();
  const bool col = li < P;
  const long qd = (long)t.S * t.nT * 500, qc = (long)t.S * 6 * t.ncf * 100;
  const double* Ad = A_diag + (long)s * t.nT * 500;
  const double* ps = p + (long)s * t.n * 16;
  const int ii = li < 10 ? li : 9;
  double py = 0.0;
  const int e1 = (bx + 1) * FOM_EPB < t.nT ? (bx + 1) * FOM_EPB : t.nT;
  for (int e = bx * FOM_EPB + wave; e < e1; e += 4) {
    const int4 nb = *reinterpret_cast<const int4*>(t.nb_elem + e * 4);
    const int nbv[4] = {nb.x, nb.y, nb.z, nb.w};
    Fb3Row row;
    row.src[0] = Ad + (long)e * 500;
    row.pb[0] = ps + (long)e * 160;
    row.qs[0] = qd;
    row.tr[0] = false;
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      const int ee = nbv[f];                          // wave-uniform
      row.src[1 + f] = nullptr;
      row.pb[1 + f] = ps;
      row.qs[1 + f] = qd;
      row.tr[1 + f] = false;
      if (ee >= 0) {
        if (ee < e) {                                 // the lower element's block towards e, used transposed
          const int4 nb2 = *reinterpret_cast<const int4*>(t.nb_elem + ee * 4);
          const int fb = nb2.x == e ? 0 : (nb2.y == e ? 1 : (nb2.z == e ? 2 : 3));
          row.src[1 + f] = Ad + (long)ee * 500 + (1 + fb) * 100;
          row.tr[1 + f] = true;
        } else {
          row.src[1 + f] = Ad + (long)e * 500 + (1 + f) * 100;
        }
        row.pb[1 + f] = ps + (long)ee * 160;
      } else {
        const int side = -(ee + 1), ss = t.nbr[s * 7 + side_slot(side)];
        if (ss >= 0) {
          row.src[1 + f] = A_cpl + (((long)s * 6 + side) * t.ncf + t.face_pos[e * 4 + f]) * 100;
          row.qs[1 + f] = qc;
          row.pb[1 + f] = p + ((long)ss * t.n + t.nb_out[e * 4 + f] * 10) * 16;
        }
      }
    }
    // direction operands: rows lk, lk + 4, lk + 8 of the block's ten, this lane's column
    double pv[5][3];
#pragma unroll
    for (int b = 0; b < 5; ++b)
#pragma unroll
      for (int ks = 0; ks < 3; ++ks) {
        const int k = lk + 4 * ks;
        pv[b][ks] = (row.src[b] && col && k < 10) ? row.pb[b][k * 16 + li] : 0.0;
      }
    d4 acc = (d4){0.0, 0.0, 0.0, 0.0};
    if (MASS) {
      const double* tm = tms + t.elem_type[e] * 100;          // wave-uniform; TM [i][j] as k3p_fom_add_mass adds it to the own block
#pragma unroll
      for (int ks = 0; ks < 3; ++ks) {
        const int k = lk + 4 * ks, kk = k < 10 ? k : 9;
        const double mv = tm[ii * 10 + kk];
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64((li < 10 && k < 10) ? mv : 0.0, pv[0][ks], acc, 0, 0, 0);
      }
    }
    for (int q = 0; q < Q; ++q) {
      double2 a2[5];
#pragma unroll
      for (int b = 0; b < 5; ++b) {
        a2[b] = make_double2(0.0, 0.0);
        if (row.src[b] && lane < 50) a2[b] = *reinterpret_cast<const double2*>(row.src[b] + q * row.qs[b] + 2 * lane);
      }
      __builtin_amdgcn_wave_barrier();               // (the reads of the previous q come first: LDS operations of a wave run in order)
#pragma unroll
      for (int b = 0; b < 5; ++b)
        if (row.src[b] && lane < 50) *reinterpret_cast<double2*>(&blk[wave][b][2 * lane]) = a2[b];
      __builtin_amdgcn_wave_barrier();
      const double tq = ths[li * 8 + q];
#pragma unroll
      for (int b = 0; b < 5; ++b) {
        if (!row.src[b]) continue;                    // wave-uniform
#pragma unroll
        for (int ks = 0; ks < 3; ++ks) {
          const int k = lk + 4 * ks, kk = k < 10 ? k : 9;
          const double av = blk[wave][b][row.tr[b] ? kk * 10 + ii : ii * 10 + kk];
          const double a = (li < 10 && k < 10) ? av : 0.0;
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, tq * pv[b][ks], acc, 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const int i = lk + 4 * r;
      if (i < 10 && col) {
        y[((long)s * t.n + e * 10 + i) * 16 + li] = acc[r];
        py += acc[r] * pv[0][r];
      }
    }
  }
  py += __shfl_xor(py, 16);
  py += __shfl_xor(py, 32);
  if (lk == 0) red[wave][li] = py;
  __syncthreads();
  if (tid < 16) part[((long)s * nbx + bx) * 16 + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}

// r [S n][16] = sum_j phi[m0 + c][j] b_K[j] (fma from the first product: K = 1, phi = 1 gives the bits of b), X[.][m0 + c] = 0
__global__ __launch_bounds__(256) void k3fb_rhs(long nv, int K, int P, int nmu, int m0, const double* __restrict__ phi,
                                                const double* __restrict__ bK, double* __restrict__ r, double* __restrict__ X) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x, g = i >> 4;
  const int c = (int)(i & 15);
  if (g >= nv || c >= P) return;
  const double* ph = phi + (long)(m0 + c) * K;
  double acc = ph[0] * bK[g];
  for (int j = 1; j < K; ++j) acc = __fma_rn(ph[j], bK[(long)j * nv + g], acc);
  r[i] = acc;
  X[g * nmu + m0 + c] = 0.0;
}

// p = z + R0^T y0 + beta p per column (y0 [S nc][16]); the first direction does not read p.  Grid (16 n / 256, S): the subdomain
// is a block index, no division per entry (measured: 281 us at config 5 either way, 2.7 TB/s on 8-byte lane accesses).
__global__ __launch_bounds__(256) void k3fb_dir(int P, int first, int cur, const double* __restrict__ scal,
                                                const double* __restrict__ z, double* __restrict__ p, int n, int nc,
                                                const double* __restrict__ Phi, const double* __restrict__ y0) {
  const int j = blockIdx.x * 256 + threadIdx.x, dof = j >> 4, c = j & 15, s = blockIdx.y;
  if (dof >= n || c >= P) return;
  const long i = ((long)s * n + dof) * 16 + c;
  double zi = z[i];
  for (int k = 0; k < nc; ++k) zi += Phi[dof * 4 + k] * y0[((long)s * nc + k) * 16 + c];
  if (first) {
    p[i] = zi;
    return;
  }
  const double old = scal[(cur ^ 1) * 16 + c];
  const double beta = old != 0.0 ? scal[cur * 16 + c] / old : 0.0;
  p[i] = zi + beta * p[i];
}

// x += alpha p, r -= alpha y, z = Dinv r (init: r is the right-hand side k3fb_rhs wrote, x = 0 already; p and y are not read).
// One wave per element at a time in the lane layout of the matrix-core tile: lane (column li, rows lk + 4 ks).  The packed
// inverse block (56 doubles) goes through the LDS like the blocks of k3fb_matvec, z_e [10 x 16] is one 3 k-step tile.
// prz, prr [S nbx][16], pr0 [S nbx][4][16].
__global__ __launch_bounds__(256) void k3fb_update(T3 t, int P, int nmu, int m0, int init, int cur, const double* __restrict__ scal,
                                                   const double* __restrict__ Dinv, const double* __restrict__ p,
                                                   const double* __restrict__ y, double* __restrict__ X, double* __restrict__ r,
                                                   double* __restrict__ z, double* __restrict__ prz, double* __restrict__ prr, int nc,
                                                   const double* __restrict__ Phi, double* __restrict__ pr0) {
  __shared__ __attribute__((aligned(16))) double dinv[4][56];
  __shared__ double red[4][6][16];
  const int s = blockIdx.y, bx = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, li = lane & 15, lk = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool col = li < P;
  double alpha = 0.0;
  if (!init && col) {
    const double pap = scal[32 + li];
    alpha = pap != 0.0 ? scal[cur * 16 + li] / pap : 0.0;
  }
  double sum[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};      // r.z, r.r, phi_k . r
  const int e1 = (bx + 1) * FOM_EPB < t.nT ? (bx + 1) * FOM_EPB : t.nT;
  for (int e = bx * FOM_EPB + wave; e < e1; e += 4) {
    const double* D = Dinv + ((long)s * t.nT + e) * 56;
    double2 d2 = make_double2(0.0, 0.0);
    if (lane < 28) d2 = *reinterpret_cast<const double2*>(D + 2 * lane);
    __builtin_amdgcn_wave_barrier();
    if (lane < 28) *reinterpret_cast<double2*>(&dinv[wave][2 * lane]) = d2;
    __builtin_amdgcn_wave_barrier();
    double rn[3];
#pragma unroll
    for (int ks = 0; ks < 3; ++ks) {
      const int i = lk + 4 * ks;
      rn[ks] = 0.0;
      if (i < 10 && col) {
        const long g = (long)s * t.n + e * 10 + i, d = g * 16 + li;
        if (init) {
          rn[ks] = r[d];
        } else {
          X[g * nmu + m0 + li] += alpha * p[d];
          rn[ks] = r[d] - alpha * y[d];
          r[d] = rn[ks];
        }
      }
    }
    d4 acc = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int ks = 0; ks < 3; ++ks) {
      const int k = lk + 4 * ks, kk = k < 10 ? k : 9, ii = li < 10 ? li : 9;
      const int a = ii < kk ? ii : kk, b = ii < kk ? kk : ii;          // packed upper triangle: entry (a, b), a <= b
      const double dv = dinv[wave][a * (21 - a) / 2 + b - a];
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64((li < 10 && k < 10) ? dv : 0.0, rn[ks], acc, 0, 0, 0);
    }
#pragma unroll
    for (int ks = 0; ks < 3; ++ks) {
      const int i = lk + 4 * ks;
      if (i < 10 && col) {
        z[((long)s * t.n + e * 10 + i) * 16 + li] = acc[ks];
        sum[0] += rn[ks] * acc[ks];
        sum[1] += rn[ks] * rn[ks];
        for (int k = 0; k < nc; ++k) sum[2 + k] += rn[ks] * Phi[(e * 10 + i) * 4 + k];
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double v = sum[j];
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    if (lk == 0) red[wave][j][li] = v;
  }
  __syncthreads();
  if (tid < 96) {
    const int j = tid >> 4, c = tid & 15;
    const double v = (red[0][j][c] + red[1][j][c]) + (red[2][j][c] + red[3][j][c]);
    const long blkid = (long)s * gridDim.x + bx;
    if (j == 0) prz[blkid * 16 + c] = v;
    else if (j == 1) prr[blkid * 16 + c] = v;
    else if (j - 2 < nc) pr0[(blkid * 4 + (j - 2)) * 16 + c] = v;
  }
}

// r0 [S nc][16] from the workgroups' restriction sums (fixed order)
__global__ __launch_bounds__(256) void k3fb_coarse_r0(int S, int nbx, int nc, const double* __restrict__ pr0, double* __restrict__ r0) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)S * nc * 16) return;
  const int c = (int)(idx & 15), m = (int)(idx >> 4), s = m / nc, k = m - s * nc;
  double v = 0.0;
  for (int bx = 0; bx < nbx; ++bx) v += pr0[(((long)s * nbx + bx) * 4 + k) * 16 + c];
  r0[idx] = v;
}

// y0 = A1inv r0 for 16 columns, one wave per row (k3f_coarse_apply widened): lane (column li, every fourth entry of the row from
// lk on); prc [M][16] = the row's part of r0 . y0
__global__ __launch_bounds__(256) void k3fb_coarse_apply(int M, const double* __restrict__ A1inv, const double* __restrict__ r0,
                                                         double* __restrict__ y0, double* __restrict__ prc) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63, li = lane & 15, lk = lane >> 4;
  if (row >= M) return;
  const double* a = A1inv + (long)row * M;
  double v0 = 0.0, v1 = 0.0, v2 = 0.0, v3 = 0.0;
  int c = lk;
  for (; c + 12 < M; c += 16) {
    v0 += a[c] * r0[(long)c * 16 + li];
    v1 += a[c + 4] * r0[(long)(c + 4) * 16 + li];
    v2 += a[c + 8] * r0[(long)(c + 8) * 16 + li];
    v3 += a[c + 12] * r0[(long)(c + 12) * 16 + li];
  }
  for (; c < M; c += 4) v0 += a[c] * r0[(long)c * 16 + li];
  double v = (v0 + v1) + (v2 + v3);
  v += __shfl_xor(v, 16);
  v += __shfl_xor(v, 32);
  if (lk == 0) {
    y0[(long)row * 16 + li] = v;
    prc[(long)row * 16 + li] = v * r0[(long)row * 16 + li];
  }
}

// out [16]: column blockIdx.x = the sum over the rows of part [np][16] and of part2 [np2][16] (fixed order)
__global__ __launch_bounds__(256) void k3fb_scalars(const double* __restrict__ part, long np, const double* __restrict__ part2, long np2,
                                                    double* __restrict__ out) {
  __shared__ double red[256];
  const int tid = threadIdx.x, c = blockIdx.x;
  double a = 0.0, a2 = 0.0;
#pragma unroll 4
  for (long k = tid; k < np; k += 256) a += part[k * 16 + c];          // (unrolled: the loads of four rounds are in flight together)
#pragma unroll 4
  for (long k = tid; k < np2; k += 256) a2 += part2[k * 16 + c];
  red[tid] = a + a2;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) red[tid] += red[tid + w];
    __syncthreads();
  }
  if (tid == 0) out[c] = red[0];
}

// work of lrbms3_fom_solve_batch: the single solver's layout (the operator at the mean theta, the inverse blocks, the coarse
// matrices) followed by the panel's own buffers
struct FomBatch3 {
  double *r, *z, *p, *y;               // [S n][16]
  double *ppy, *prz, *prr, *pr0;       // [nblk][16] each, pr0 [nblk][4][16]
  double *r0, *y0, *prc;               // [Mmax][16]
  double* scal;                        // [5][16]
  static long extra(const T3& t) {
    const long S = t.S, nblk = S * ((t.nT + FOM_EPB - 1) / FOM_EPB), M = std::min<long>(4 * S, FOM_MAX_COARSE);
    return 4 * S * t.n * 16 + 7 * nblk * 16 + 3 * M * 16 + 80;
  }
  void carve(const T3& t, const FomWork& w, double* at) {
    const long tot = (long)t.S * t.n * 16;
    r = at;
    z = r + tot;
    p = z + tot;
    y = p + tot;
    ppy = y + tot;
    prz = ppy + w.nblk * 16;
    prr = prz + w.nblk * 16;
    pr0 = prr + w.nblk * 16;
    r0 = pr0 + 4 * w.nblk * 16;
    y0 = r0 + w.Mmax * 16;
    prc = y0 + w.Mmax * 16;
    scal = prc + w.Mmax * 16;
  }
};

// The panel's operator: the elliptic one, or (mass) the step operator M + A(theta) with theta pre-multiplied by dt
struct Fb3Op {
  int Q, P, nmu, m0;
  TB th;
  const double *A_diag, *A_cpl;
  bool mass;
};

void fomb3_launch_matvec(lrbms3_ctx* ctx, hipStream_t st, const FomWork& w, const Fb3Op& op, const double* p, double* y, double* part) {
  const T3& t = ctx->t;
  if (op.mass)
    hipLaunchKernelGGL(k3fb_matvec<true>, dim3(xcd_grid(w.nbx, t.S)), dim3(256), 0, st, t, w.nbx, op.Q, op.P, op.th, op.A_diag, op.A_cpl, p, y,
                       part);
  else
    hipLaunchKernelGGL(k3fb_matvec<false>, dim3(xcd_grid(w.nbx, t.S)), dim3(256), 0, st, t, w.nbx, op.Q, op.P, op.th, op.A_diag, op.A_cpl, p, y, part);
}

// PCG on the panel of P <= 16 columns m0 .. m0 + P - 1 of the call, shared by lrbms3_fom_solve_batch and the steps of
// lrbms3_fom_implicit_euler_batch: on entry X holds the start values and b.r the start residual.  The host reads r.r per column
// every 16 iterations (fom_cg) and stops when the worst column with a nonzero reference is at or below rtol.  The reference per
// column is |r_0| (ref_part == nullptr: the right-hand side, the start value being zero) or the sum of the partials
// ref_part [nblk][16] (the step's full right-hand side, left by k3fb_step_residual); `name` is the caller in the error texts.
int fomb3_panel_run(lrbms3_ctx* ctx, hipStream_t st, const FomWork& w, const FomBatch3& b, const Fb3Op& op, int nc, const double* A1inv,
                    double* X, const double* ref_part, double rtol, int max_iter, int* its, double* rel_out, const char* name) {
  const T3& t = ctx->t;
  const long S = t.S, nblk = w.nblk, M = (long)nc * S;
  const int nbx = w.nbx, P = op.P, nmu = op.nmu, m0 = op.m0;
  const double* Phi = ctx->fom_phi;
  const dim3 grid(nbx, S);
  auto tail = [&](double* rz) {                      // coarse step and r.z per column for the residual k3fb_update has just written
    if (nc > 0) {
      hipLaunchKernelGGL(k3fb_coarse_r0, dim3((unsigned)((M * 16 + 255) / 256)), dim3(256), 0, st, (int)S, nbx, nc, b.pr0, b.r0);
      hipLaunchKernelGGL(k3fb_coarse_apply, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, st, (int)M, A1inv, b.r0, b.y0, b.prc);
    }
    hipLaunchKernelGGL(k3fb_scalars, dim3(16), dim3(256), 0, st, b.prz, nblk, b.prc, nc > 0 ? M : 0L, rz);
  };
  hipLaunchKernelGGL(k3fb_update, grid, dim3(256), 0, st, t, P, nmu, m0, 1, 0, b.scal, w.Dinv, b.p, b.y, X, b.r, b.z, b.prz, b.prr, nc,
                     Phi, b.pr0);
  tail(b.scal);
  hipLaunchKernelGGL(k3fb_scalars, dim3(16), dim3(256), 0, st, ref_part ? ref_part : b.prr, nblk, (const double*)nullptr, 0L, b.scal + 64);
  if (ref_part) hipLaunchKernelGGL(k3fb_scalars, dim3(16), dim3(256), 0, st, b.prr, nblk, (const double*)nullptr, 0L, b.scal + 48);
  LRBMS_LAUNCH_CHECK(ctx);
  double bb[16], rr[16];
  LRBMS_HIP_CHECK(ctx, hipMemcpyAsync(bb, b.scal + 64, sizeof(bb), hipMemcpyDeviceToHost, st));
  if (ref_part) LRBMS_HIP_CHECK(ctx, hipMemcpyAsync(rr, b.scal + 48, sizeof(rr), hipMemcpyDeviceToHost, st));
  LRBMS_HIP_CHECK(ctx, hipStreamSynchronize(st));
  auto worst = [&](const double* cur) {
    double wr = 0.0;
    for (int c = 0; c < P; ++c)
      if (bb[c] != 0.0) {
        const double rel = sqrt(cur[c] / bb[c]);
        if (!(rel == rel)) return rel;
        if (rel > wr) wr = rel;
      }
    return wr;
  };
  *its = 0;
  *rel_out = 0.0;
  double rel = worst(ref_part ? rr : bb);            // 1 from a zero start value; 0 if every reference or every start residual is zero
  if (rel == 0.0) return LRBMS_OK;
  if (!(rel == rel)) return lrbms_fail(ctx, LRBMS_E_NOT_CONVERGED, std::string(name) + ": NaN right-hand side");
  int it = 0;
  const int check = 16;
  while (it < max_iter) {
    for (int k = 0; k < check && it < max_iter; ++k, ++it) {
      const int cur = it & 1;                        // slot of the current r.z (the update of this iteration writes the other one)
      hipLaunchKernelGGL(k3fb_dir, dim3((unsigned)((t.n * 16 + 255) / 256), (unsigned)S), dim3(256), 0, st, P, it == 0 ? 1 : 0, cur, b.scal,
                         b.z, b.p, t.n, nc, Phi, b.y0);
      fomb3_launch_matvec(ctx, st, w, op, b.p, b.y, b.ppy);
      hipLaunchKernelGGL(k3fb_scalars, dim3(16), dim3(256), 0, st, b.ppy, nblk, (const double*)nullptr, 0L, b.scal + 32);
      hipLaunchKernelGGL(k3fb_update, grid, dim3(256), 0, st, t, P, nmu, m0, 0, cur, b.scal, w.Dinv, b.p, b.y, X, b.r, b.z, b.prz, b.prr,
                         nc, Phi, b.pr0);
      tail(b.scal + (cur ^ 1) * 16);
    }
    hipLaunchKernelGGL(k3fb_scalars, dim3(16), dim3(256), 0, st, b.prr, nblk, (const double*)nullptr, 0L, b.scal + 48);
    LRBMS_LAUNCH_CHECK(ctx);
    LRBMS_HIP_CHECK(ctx, hipMemcpyAsync(rr, b.scal + 48, sizeof(rr), hipMemcpyDeviceToHost, st));
    LRBMS_HIP_CHECK(ctx, hipStreamSynchronize(st));
    rel = worst(rr);
    if (!(rel == rel)) return lrbms_fail(ctx, LRBMS_E_NOT_CONVERGED, std::string(name) + ": NaN residual");
    if (rel <= rtol) break;
  }
  *its = it;
  *rel_out = rel;
  return LRBMS_OK;
}

// A panel of lrbms3_fom_solve_batch: the right-hand sides, x = 0, then the PCG relative to |b_m|
int fomb3_panel(lrbms3_ctx* ctx, hipStream_t st, const FomWork& w, const FomBatch3& b, const Fb3Op& op, int K, const double* phi,
                const double* b_K, int nc, const double* A1inv, double* X, double rtol, int max_iter, int* its, double* rel_out) {
  const long total = (long)ctx->t.S * ctx->t.n;
  hipLaunchKernelGGL(k3fb_rhs, dim3((unsigned)((total * 16 + 255) / 256)), dim3(256), 0, st, total, K, op.P, op.nmu, op.m0, phi, b_K, b.r,
                     X);
  return fomb3_panel_run(ctx, st, w, b, op, nc, A1inv, X, nullptr, rtol, max_iter, its, rel_out, "fom_solve_batch");
}

}  // namespace

extern "C" {

int64_t lrbms3_fom_solve_batch_work_size(lrbms3_ctx* ctx, int32_t nmu) {
  if (!ctx || !ctx->has_mesh || nmu < 1 || nmu > 64) return -1;
  return lrbms3_fom_solve_work_size(ctx) + FomBatch3::extra(ctx->t);
}

int lrbms3_fom_solve_batch(lrbms3_ctx* ctx, int32_t Q, int32_t nmu, const double* theta, const double* A_diag, const double* A_cpl,
                           int32_t K, const double* phi, const double* b_K, double* work, double* X, double rtol, int32_t max_iter,
                           double* info, void* stream) {
  LRBMS_REQUIRE_MESH(ctx);
  const T3& t = ctx->t;
  if (t.S_ext != t.S) return lrbms_fail(ctx, LRBMS_E_INVALID, "fom_solve_batch: needs all subdomains on this rank");
  if (Q < 1 || Q > 8 || nmu < 1 || nmu > 64 || K < 1 || K > 64 || max_iter < 1 || !(rtol > 0.0))
    return lrbms_fail(ctx, LRBMS_E_INVALID, "fom_solve_batch: bad Q / nmu / K / max_iter / rtol");
  if (!theta || !A_diag || !A_cpl || !phi || !b_K || !work || !X) return lrbms_fail(ctx, LRBMS_E_INVALID, "fom_solve_batch: null argument");
  hipStream_t st = (hipStream_t)stream;
  const long S = t.S, nd = S * t.nT * 500, ncp = S * 6 * t.ncf * 100;
  FomWork w = fom_work(t, work);
  FomBatch3 b;
  b.carve(t, w, work + lrbms3_fom_solve_work_size(ctx));
  // one preconditioner per call, both levels at the mean theta of its columns (summed in column order)
  QV tb{};
  for (int q = 0; q < Q; ++q) {
    double acc = 0.0;
    for (int m = 0; m < nmu; ++m) acc += theta[(long)m * Q + q];
    tb.v[q] = acc / nmu;
  }
  launch_combine(st, nd, Q, tb, A_diag, w.Amu);
  launch_combine(st, ncp, Q, tb, A_cpl, w.Cmu);
  hipLaunchKernelGGL(k3f_block_inverse, dim3((t.nT + 63) / 64, S), dim3(64), 0, st, t, w.Amu, w.Dinv);
  int nc = 0;
  const double* A1inv = nullptr;
  if (int rc = fom_coarse(ctx, st, w, false, nc, A1inv)) return rc;
  int its_max = 0;
  double worst = 0.0;
  bool missed = false;
  for (int i = 0; i < 8; ++i) ctx->fomb_panels[i] = 0.0;
  for (int m0 = 0; m0 < nmu; m0 += 16) {
    const int P = nmu - m0 < 16 ? nmu - m0 : 16;
    Fb3Op op{Q, P, nmu, m0, {}, A_diag, A_cpl, false};
    for (int c = 0; c < 16; ++c)
      for (int q = 0; q < 8; ++q) op.th.v[c][q] = (c < P && q < Q) ? theta[(long)(m0 + c) * Q + q] : 0.0;
    int it = 0;
    double rel = 0.0;
    if (int rc = fomb3_panel(ctx, st, w, b, op, K, phi, b_K, nc, A1inv, X, rtol, max_iter, &it, &rel)) return rc;
    ctx->fomb_panels[m0 / 16 * 2] = it;
    ctx->fomb_panels[m0 / 16 * 2 + 1] = rel;
    if (it > its_max) its_max = it;
    if (rel > worst) worst = rel;
    if (rel > rtol) missed = true;
  }
  if (info) info[0] = its_max, info[1] = worst;
  if (missed) return lrbms_fail(ctx, LRBMS_E_NOT_CONVERGED, "fom_solve_batch: CG did not reach rtol");
  return LRBMS_OK;
}

int lrbms3_fom_solve_batch_panel_info(lrbms3_ctx* ctx, double* out) {
  if (!ctx || !out) return LRBMS_E_INVALID;
  for (int i = 0; i < 8; ++i) out[i] = ctx->fomb_panels[i];
  return LRBMS_OK;
}

int lrbms3_fom_solve(lrbms3_ctx* ctx, int32_t Q, const double* theta, const double* A_diag, const double* A_cpl, const double* b,
                     double* work, double* x, double rtol, int32_t max_iter, double* info, void* stream) {
  LRBMS_REQUIRE_MESH(ctx);
  const T3& t = ctx->t;
  if (t.S_ext != t.S) return lrbms_fail(ctx, LRBMS_E_INVALID, "fom_solve: needs all subdomains on this rank");
  if (Q < 1 || Q > 8 || !theta || !A_diag || !A_cpl || !b || !work || !x) return lrbms_fail(ctx, LRBMS_E_INVALID, "fom_solve: bad argument");
  hipStream_t st = (hipStream_t)stream;
  const long S = t.S, nd = S * t.nT * 500, ncp = S * 6 * t.ncf * 100;
  FomWork w = fom_work(t, work);
  const QV th = make_theta(Q, theta);
  launch_combine(st, nd, Q, th, A_diag, w.Amu);
  launch_combine(st, ncp, Q, th, A_cpl, w.Cmu);
  hipLaunchKernelGGL(k3f_block_inverse, dim3((t.nT + 63) / 64, S), dim3(64), 0, st, t, w.Amu, w.Dinv);
  int nc = 0;
  const double* A1inv = nullptr;
  int rc = fom_coarse(ctx, st, w, true, nc, A1inv);
  if (rc != LRBMS_OK) return rc;
  return fom_cg(ctx, st, w, nc, A1inv, b, x, rtol, max_iter, info, nullptr, "fom_solve");
}

int lrbms3_fom_apply(lrbms3_ctx* ctx, int32_t Q, int32_t M, const double* theta, const double* A_diag, const double* A_cpl,
                     const double* x, double* y, void* stream) {
  LRBMS_REQUIRE_MESH(ctx);
  if (Q < 1 || Q > 8 || M < 1 || !theta || !A_diag || !A_cpl || !x || !y) return lrbms_fail(ctx, LRBMS_E_INVALID, "fom_apply: bad argument");
  const T3& t = ctx->t;
  hipLaunchKernelGGL(k3_fom_apply, dim3(t.nT, t.S), dim3(256), 0, (hipStream_t)stream, t, Q, M, make_theta(Q, theta), A_diag, A_cpl, x, y);
  LRBMS_LAUNCH_CHECK(ctx);
  return LRBMS_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------- parabolic path
// M u' + A(mu) u = f with the block L2 product as mass: implicit Euler on the full-order and on the reduced system, the mass
// norms of the parabolic estimator, the projected mass.  The P2 DG mass matrix is element-block-diagonal, every block the
// table TM of the element's type, so M^-1 is TM^-1 per element (inverted once per context).  The step operators reuse the CG
// machinery of lrbms3_fom_solve / lrbms3_reduced_solve (fom_coarse, fom_cg, red_cg).
namespace {

// inverses of the six element mass tables: one workgroup per type, Gauss-Jordan in LDS (SPD: no pivoting)
__global__ __launch_bounds__(64) void k3p_tm_inverse(const double* __restrict__ TM, double* __restrict__ TMinv) {
  __shared__ double a[10][21];
  const int ty = blockIdx.x, tid = threadIdx.x;
  for (int i = tid; i < 200; i += 64) {
    const int r = i / 20, c = i - r * 20;
    a[r][c] = c < 10 ? TM[ty * 100 + r * 10 + c] : (c - 10 == r ? 1.0 : 0.0);
  }
  __syncthreads();
  for (int p = 0; p < 10; ++p) {
    const double ip = 1.0 / a[p][p];
    __syncthreads();
    if (tid < 20) a[p][tid] *= ip;
    __syncthreads();
    for (int i = tid; i < 200; i += 64) {
      const int r = i / 20, c = i - r * 20;
      if (r != p && c != p) a[r][c] -= a[r][p] * a[p][c];
    }
    __syncthreads();
    if (tid < 10 && tid != p) a[tid][p] = 0.0;
    __syncthreads();
  }
  for (int i = tid; i < 100; i += 64) TMinv[ty * 100 + i] = a[i / 10][10 + i % 10];
}

// out [S][L] = sum_e y_e^T TM_e^-1 y_e, Y [S][n][L]: one workgroup per subdomain streams its slab once.  Threads (g, l) of a
// chunk of Lc <= 256 vectors: vector l0 + l, elements g, g + G, ... (G = 256 / Lc); the G partial sums are added in a fixed order.
__global__ __launch_bounds__(256) void k3p_mass_inv_norm2(T3 t, int L, const double* __restrict__ TMinv, const double* __restrict__ Y,
                                                          double* __restrict__ out) {
  __shared__ double mi[600], red[256];
  const int s = blockIdx.x, tid = threadIdx.x;
  for (int i = tid; i < 600; i += 256) mi[i] = TMinv[i];
  for (int l0 = 0; l0 < L; l0 += 256) {
    const int Lc = L - l0 < 256 ? L - l0 : 256, G = 256 / Lc, g = tid / Lc, l = tid - g * Lc;
    __syncthreads();
    double acc = 0.0;
    if (g < G)
      for (int e = g; e < t.nT; e += G) {
        const double* Mi = mi + t.elem_type[e] * 100;
        const double* y = Y + ((long)s * t.n + e * 10) * L + l0 + l;
        double v[10];
#pragma unroll
        for (int i = 0; i < 10; ++i) v[i] = y[(long)i * L];
#pragma unroll
        for (int i = 0; i < 10; ++i) {
          double a = 0.0;
#pragma unroll
          for (int j = 0; j < 10; ++j) a += Mi[i * 10 + j] * v[j];
          acc += v[i] * a;
        }
      }
    red[tid] = acc;
    __syncthreads();
    if (tid < Lc) {
      double sum = 0.0;
      for (int k = 0; k < G; ++k) sum += red[k * Lc + tid];
      out[(long)s * L + l0 + tid] = sum;
    }
  }
}

// M_red [S][N][N] = sum_e V_e^T TM_e V_e on the fp64 matrix cores, one workgroup of 8 waves per subdomain, one wave per element
// at a time.  Z = TM_e V_e (TM as the A operand: lane row l&15, k l>>4; rows of V_e as the B operand), then G += V_e^T Z: the
// accumulator layout of Z (rows (l>>4) + 4 r, column l&15) is the B operand of k-step r, and the A operand of that step,
// V_e[(l>>4) + 4 r][16 rt + (l&15)], is the B operand of the first product for k-step r -- every lane loads its 3 T values of
// V_e once (rows >= 10 and columns >= N as zeros) and both products read them from registers.  T = 16-column tiles per side.
template <int T>
__global__ __launch_bounds__(512) void k3p_project_mass(T3 t, int N, const double* __restrict__ V, double* __restrict__ Mred) {
  __shared__ double red[8][256];
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, li = lane & 15, lk = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  d4 acc[T][T];
#pragma unroll
  for (int rt = 0; rt < T; ++rt)
#pragma unroll
    for (int ct = 0; ct < T; ++ct) acc[rt][ct] = d4{0.0, 0.0, 0.0, 0.0};
  const double* Vs = V + (long)s * t.n * N;
  for (int e = wave; e < t.nT; e += 8) {
    const double* tm = t.TM + t.elem_type[e] * 100;
    const double* Ve = Vs + (long)e * 10 * N;
    double a[3], v[3][T];
#pragma unroll
    for (int ks = 0; ks < 3; ++ks) {
      const int r = 4 * ks + lk;
      a[ks] = (li < 10 && r < 10) ? tm[li * 10 + r] : 0.0;
#pragma unroll
      for (int ct = 0; ct < T; ++ct) {
        const int c = 16 * ct + li;
        v[ks][ct] = (r < 10 && c < N) ? Ve[r * N + c] : 0.0;
      }
    }
#pragma unroll
    for (int ct = 0; ct < T; ++ct) {
      d4 z = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int ks = 0; ks < 3; ++ks) z = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ks], v[ks][ct], z, 0, 0, 0);
#pragma unroll
      for (int rt = 0; rt < T; ++rt)
#pragma unroll
        for (int r = 0; r < 3; ++r) acc[rt][ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(v[r][rt], z[r], acc[rt][ct], 0, 0, 0);
    }
  }
  // the waves' tiles summed in a fixed order through the LDS
#pragma unroll
  for (int rt = 0; rt < T; ++rt)
#pragma unroll
    for (int ct = 0; ct < T; ++ct) {
      __syncthreads();
#pragma unroll
      for (int r = 0; r < 4; ++r) red[wave][r * 64 + lane] = acc[rt][ct][r];
      __syncthreads();
      if (tid < 256) {
        const int r = tid >> 6, l = tid & 63;
        double sum = 0.0;
        for (int w = 0; w < 8; ++w) sum += red[w][tid];
        const int row = 16 * rt + (l >> 4) + 4 * r, col = 16 * ct + (l & 15);
        if (row < N && col < N) Mred[((long)s * N + row) * N + col] = sum;
      }
    }
}

// Amu [S][n_T][5][100] (slot 0 = the (e, e) block) += TM of the element's type: the mass part of the implicit Euler step operator
__global__ __launch_bounds__(256) void k3p_fom_add_mass(T3 t, long total, double* __restrict__ Amu) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const long se = i / 100;
  const int c = (int)(i - se * 100), e = (int)(se % t.nT);
  Amu[se * 500 + c] += t.TM[t.elem_type[e] * 100 + c];
}

// right-hand side of a warm-started step: f = TM u_k + dt b (per element), rhs = f - Ku (Ku = step operator applied to u_k);
// partial |f|^2 per workgroup (rows as k3f_update)
__global__ __launch_bounds__(256) void k3p_fom_rhs(T3 t, double dt, const double* __restrict__ u, const double* __restrict__ b,
                                                   const double* __restrict__ Ku, double* __restrict__ rhs, double* __restrict__ part) {
  __shared__ double red[256];
  const int s = blockIdx.y, tid = threadIdx.x;
  const int el = tid / 10, i = tid - el * 10, e = blockIdx.x * FOM_EPB + el;
  const bool on = el < FOM_EPB && e < t.nT;
  double f = 0.0;
  if (on) {
    const long d = (long)s * t.n + e * 10 + i;
    const double* tm = t.TM + t.elem_type[e] * 100 + i * 10;
    const double* ue = u + (long)s * t.n + e * 10;
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < 10; ++j) acc += tm[j] * ue[j];
    f = acc + dt * b[d];
    rhs[d] = f - Ku[d];
  }
  const double sum = block_sum(f * f, red);
  if (tid == 0) part[(long)blockIdx.y * gridDim.x + blockIdx.x] = sum;
}

// k3p_fom_rhs with the load sum_j phi[j] b_K[j] (phi: the coefficient row of the step's new time, device; b_K [K][S][n], SN = S n),
// the sum spelled out with fma from the first product.  K = 1, phi = 1: the bits of k3p_fom_rhs.
__global__ __launch_bounds__(256) void k3p_fom_rhs_src(T3 t, double dt, const double* __restrict__ u, int K, long SN,
                                                       const double* __restrict__ phi, const double* __restrict__ b_K,
                                                       const double* __restrict__ Ku, double* __restrict__ rhs, double* __restrict__ part) {
  __shared__ double red[256];
  const int s = blockIdx.y, tid = threadIdx.x;
  const int el = tid / 10, i = tid - el * 10, e = blockIdx.x * FOM_EPB + el;
  const bool on = el < FOM_EPB && e < t.nT;
  double f = 0.0;
  if (on) {
    const long d = (long)s * t.n + e * 10 + i;
    const double* tm = t.TM + t.elem_type[e] * 100 + i * 10;
    const double* ue = u + (long)s * t.n + e * 10;
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < 10; ++j) acc += tm[j] * ue[j];
    double bs = phi[0] * b_K[d];
    for (int j = 1; j < K; ++j) bs = __fma_rn(phi[j], b_K[(long)j * SN + d], bs);
    f = acc + dt * bs;
    rhs[d] = f - Ku[d];
  }
  const double sum = block_sum(f * f, red);
  if (tid == 0) part[(long)blockIdx.y * gridDim.x + blockIdx.x] = sum;
}

int ensure_tm_inverse(lrbms3_ctx* ctx, hipStream_t st) {
  if (ctx->tm_inv && ctx->tm_inv_src == ctx->t.TM) return LRBMS_OK;
  if (!ctx->tm_inv) {
    LRBMS_HIP_CHECK(ctx, hipMalloc((void**)&ctx->tm_inv, sizeof(double) * 600));
    ctx->owned.push_back(ctx->tm_inv);
  }
  hipLaunchKernelGGL(k3p_tm_inverse, dim3(6), dim3(64), 0, st, ctx->t.TM, ctx->tm_inv);
  LRBMS_LAUNCH_CHECK(ctx);
  LRBMS_HIP_CHECK(ctx, hipStreamSynchronize(st));      // later calls may come on other streams
  ctx->tm_inv_src = ctx->t.TM;
  return LRBMS_OK;
}

}  // namespace

namespace lrbms3 {

void launch_fom_add_mass(hipStream_t st, const T3& t, double* Amu) {
  const long total = (long)t.S * t.nT * 100;
  hipLaunchKernelGGL(k3p_fom_add_mass, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, t, total, Amu);
}

}  // namespace lrbms3

extern "C" {

int lrbms3_mass_inverse_norm2(lrbms3_ctx* ctx, int32_t L, const double* Y, double* out, void* stream) {
  LRBMS_REQUIRE_MESH(ctx);
  const T3& t = ctx->t;
  if (t.S_ext != t.S) return lrbms_fail(ctx, LRBMS_E_INVALID, "mass_inverse_norm2: needs all subdomains on this rank");
  if (L < 1 || !Y || !out) return lrbms_fail(ctx, LRBMS_E_INVALID, "mass_inverse_norm2: bad argument");
  hipStream_t st = (hipStream_t)stream;
  int rc = ensure_tm_inverse(ctx, st);
  if (rc != LRBMS_OK) return rc;
  hipLaunchKernelGGL(k3p_mass_inv_norm2, dim3(t.S), dim3(256), 0, st, t, L, ctx->tm_inv, Y, out);
  LRBMS_LAUNCH_CHECK(ctx);
  return LRBMS_OK;
}

int lrbms3_project_mass(lrbms3_ctx* ctx, int32_t N, const double* V, double* M_red, void* stream) {
  LRBMS_REQUIRE_MESH(ctx);
  const T3& t = ctx->t;
  if (t.S_ext != t.S) return lrbms_fail(ctx, LRBMS_E_INVALID, "project_mass: needs all subdomains on this rank");
  if (N < 1 || N > 64 || !V || !M_red) return lrbms_fail(ctx, LRBMS_E_INVALID, "project_mass: bad argument (1 <= N <= 64)");
  hipStream_t st = (hipStream_t)stream;
  const int T = (N + 15) / 16;
  if (T == 1) hipLaunchKernelGGL(k3p_project_mass<1>, dim3(t.S), dim3(512), 0, st, t, N, V, M_red);
  else if (T == 2) hipLaunchKernelGGL(k3p_project_mass<2>, dim3(t.S), dim3(512), 0, st, t, N, V, M_red);
  else if (T == 3) hipLaunchKernelGGL(k3p_project_mass<3>, dim3(t.S), dim3(512), 0, st, t, N, V, M_red);
  else hipLaunchKernelGGL(k3p_project_mass<4>, dim3(t.S), dim3(512), 0, st, t, N, V, M_red);
  LRBMS_LAUNCH_CHECK(ctx);
  return LRBMS_OK;
}

int64_t lrbms3_fom_implicit_euler_work_size(lrbms3_ctx* ctx) {
  const int64_t base = lrbms3_fom_solve_work_size(ctx);
  if (base < 0) return -1;
  const T3& t = ctx->t;
  const int64_t nblk = (int64_t)t.S * ((t.nT + FOM_EPB - 1) / FOM_EPB);
  return base + (int64_t)t.S * t.n + nblk + 16;          // + right-hand side of the correction, partial |f|^2, |f|^2
}

}  // extern "C"

namespace {

// The time loop shared by lrbms3_fom_implicit_euler and lrbms3_fom_implicit_euler_src: the step operator M + dt A(mu), its
// element-block inverses and its coarse level once, then per step K u_k, the right-hand side of the correction (rhs_launch(step, u_k,
// K u_k, rhs, part): the one kernel in which the two exports differ), the warm-started CG and u_{k+1} = u_k + d.
template <class F>
int fom_euler_run(lrbms3_ctx* ctx, const char* name, int Q, const double* theta, double dt, int nt, const double* A_diag,
                  const double* A_cpl, double* work, double* U, double rtol, int max_iter, double* info, hipStream_t st, F rhs_launch) {
  const T3& t = ctx->t;
  const long S = t.S, nd = S * t.nT * 500, ncp = S * 6 * t.ncf * 100, total = S * t.n;
  FomWork w = fom_work(t, work);
  double* rhs = work + lrbms3_fom_solve_work_size(ctx);
  double* part = rhs + total;
  double* ff = part + w.nblk;
  QV th = make_theta(Q, theta);
  for (int q = 0; q < Q; ++q) th.v[q] *= dt;
  // step operator M + dt A(mu): element-block inverses and coarse level once per call, on it (never the elliptic solves' kept one)
  launch_combine(st, nd, Q, th, A_diag, w.Amu);
  launch_combine(st, ncp, Q, th, A_cpl, w.Cmu);
  hipLaunchKernelGGL(k3p_fom_add_mass, dim3((unsigned)((S * t.nT * 100 + 255) / 256)), dim3(256), 0, st, t, S * t.nT * 100, w.Amu);
  hipLaunchKernelGGL(k3f_block_inverse, dim3((t.nT + 63) / 64, S), dim3(64), 0, st, t, w.Amu, w.Dinv);
  LRBMS_LAUNCH_CHECK(ctx);
  int nc = 0;
  const double* A1inv = nullptr;
  int rc = fom_coarse(ctx, st, w, false, nc, A1inv);
  if (rc != LRBMS_OK) return rc;
  double iters = 0.0, worst = 0.0;
  if (info) info[0] = 0, info[1] = 0;
  for (int k = 0; k < nt; ++k) {
    // warm start at u_k: the correction solves K d = (M u_k + dt b) - K u_k, with the residual relative to |M u_k + dt b|
    const double* uk = U + (long)k * total;
    double* un = U + (long)(k + 1) * total;
    hipLaunchKernelGGL(k3f_matvec, dim3(xcd_grid(w.nbx, (int)S)), dim3(256), 0, st, t, w.nbx, w.Amu, w.Cmu, uk, w.y, w.ppy);
    rhs_launch(k, uk, w.y, rhs, part, w.nbx);
    hipLaunchKernelGGL(k3_reduce1, dim3(1), dim3(256), 0, st, (int)w.nblk, part, ff);
    LRBMS_LAUNCH_CHECK(ctx);
    double inf[2] = {0.0, 0.0};
    rc = fom_cg(ctx, st, w, nc, A1inv, rhs, un, rtol, max_iter, inf, ff, name);
    iters += inf[0];
    worst = std::max(worst, inf[1]);
    if (info) info[0] = iters, info[1] = worst;
    if (rc != LRBMS_OK && rc != LRBMS_E_NOT_CONVERGED) return rc;
    // (also behind a step that missed rtol: U[k + 1] holds the iterate u_k + d, as the batched exports leave it, not the bare correction)
    launch_axpy(st, total, uk, un);
    LRBMS_LAUNCH_CHECK(ctx);
    if (rc != LRBMS_OK) return rc;
  }
  return LRBMS_OK;
}

}  // namespace

extern "C" {

int lrbms3_fom_implicit_euler(lrbms3_ctx* ctx, int32_t Q, const double* theta, double dt, int32_t nt, const double* A_diag,
                              const double* A_cpl, const double* b, double* work, double* U, double rtol, int32_t max_iter,
                              double* info, void* stream) {
  LRBMS_REQUIRE_MESH(ctx);
  const T3& t = ctx->t;
  if (t.S_ext != t.S) return lrbms_fail(ctx, LRBMS_E_INVALID, "fom_implicit_euler: needs all subdomains on this rank");
  if (Q < 1 || Q > 8 || !theta || !A_diag || !A_cpl || !b || !work || !U)
    return lrbms_fail(ctx, LRBMS_E_INVALID, "fom_implicit_euler: bad argument");
  if (!(dt > 0.0) || nt < 1) return lrbms_fail(ctx, LRBMS_E_INVALID, "fom_implicit_euler: dt > 0 and nt >= 1 required");
  hipStream_t st = (hipStream_t)stream;
  return fom_euler_run(ctx, "fom_implicit_euler", Q, theta, dt, nt, A_diag, A_cpl, work, U, rtol, max_iter, info, st,
                       [&](int, const double* uk, const double* Ku, double* rhs, double* part, int nbx) {
                         hipLaunchKernelGGL(k3p_fom_rhs, dim3(nbx, t.S), dim3(256), 0, st, t, dt, uk, b, Ku, rhs, part);
                       });
}

int lrbms3_fom_implicit_euler_src(lrbms3_ctx* ctx, int32_t Q, int32_t K, const double* theta, double dt, int32_t nt,
                                  const double* A_diag, const double* A_cpl, const double* b_K, const double* phi, double* work,
                                  double* U, double rtol, int32_t max_iter, double* info, void* stream) {
  LRBMS_REQUIRE_MESH(ctx);
  const T3& t = ctx->t;
  if (t.S_ext != t.S) return lrbms_fail(ctx, LRBMS_E_INVALID, "fom_implicit_euler_src: needs all subdomains on this rank");
  if (Q < 1 || Q > 8 || !theta || !A_diag || !A_cpl || !b_K || !phi || !work || !U)
    return lrbms_fail(ctx, LRBMS_E_INVALID, "fom_implicit_euler_src: bad argument");
  if (K < 1 || K > 64) return lrbms_fail(ctx, LRBMS_E_INVALID, "fom_implicit_euler_src: need 1 <= K <= 64");
  if (!(dt > 0.0) || nt < 1) return lrbms_fail(ctx, LRBMS_E_INVALID, "fom_implicit_euler_src: dt > 0 and nt >= 1 required");
  hipStream_t st = (hipStream_t)stream;
  return fom_euler_run(ctx, "fom_implicit_euler_src", Q, theta, dt, nt, A_diag, A_cpl, work, U, rtol, max_iter, info, st,
                       [&](int step, const double* uk, const double* Ku, double* rhs, double* part, int nbx) {
                         hipLaunchKernelGGL(k3p_fom_rhs_src, dim3(nbx, t.S), dim3(256), 0, st, t, dt, uk, K, (long)t.S * t.n,
                                            phi + (long)(step + 1) * K, b_K, Ku, rhs, part);
                       });
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------- batched trajectories
// lrbms3_fom_implicit_euler_batch (2D: lrbms_fom_implicit_euler_batch): column m runs the implicit Euler
//   (M + dt A(theta_m)) u_{k+1} = M u_k + dt sum_j phi[m][k+1][j] b_K[j],   k = 0 .. nt-1,
// on U [nt+1][S][n][nmu] (parameter fastest; slab 0 is input).  Panels of <= 16 columns, panels outermost: a panel runs its whole
// trajectory with one theta table (pre-multiplied by dt), every step a warm-started PCG of the panel kernels of
// lrbms3_fom_solve_batch on the step operator (k3fb_matvec<true>), relative to the step's full right-hand side per column.  Per step
//   k3fb_load            u_k of the panel's columns -> b.p [S n][16] and the next slab (x = u_k)
//   k3fb_matvec<true>     y = (M + dt A(theta_c)) u_k
//   k3fb_step_residual   r = M u_k + dt sum_j phi b_j - y, partials of |M u_k + dt sum_j phi b_j|^2
// then fomb3_panel_run (its first direction overwrites b.p, which the two kernels before it have consumed).  ONE preconditioner
// per call, both levels on M + dt A(theta_bar) at the call mean, for all panels and steps.
namespace {

// the columns m0 .. m0 + P - 1 of the slab Uk [S n][nmu] -> the panel vector uk [S n][16] and the same columns of the next slab X
__global__ __launch_bounds__(256) void k3fb_load(long nv, int P, int nmu, int m0, const double* __restrict__ Uk, double* __restrict__ X,
                                                 double* __restrict__ uk) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x, g = i >> 4;
  const int c = (int)(i & 15);
  if (g >= nv || c >= P) return;
  const double v = Uk[g * nmu + m0 + c];
  X[g * nmu + m0 + c] = v;
  uk[i] = v;
}

// r = TM u_k + dt sum_j phi_c[j] b_j - y per column (y = (M + dt A(theta_c)) u_k from k3fb_matvec<true>), the arithmetic of
// k3p_fom_rhs_src: the TM row sum in its order, the source sum as fma from the first product.  phi: the table [nmu][rows][K] offset
// to the step's row, so column c reads phi + (m0 + c) phi_stride.  Workgroups and lanes as in k3fb_update: one wave per element at
// a time, lane (column li, rows lk + 4 ks).  part [S nbx][16] = |TM u_k + dt sum_j phi b_j|^2 over the workgroup's elements.
__global__ __launch_bounds__(256) void k3fb_step_residual(T3 t, double dt, int K, int P, int m0, long phi_stride,
                                                          const double* __restrict__ phi, const double* __restrict__ b_K,
                                                          const double* __restrict__ uk, const double* __restrict__ y,
                                                          double* __restrict__ r, double* __restrict__ part) {
  __shared__ double red[4][16];
  const int s = blockIdx.y, bx = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, li = lane & 15, lk = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool col = li < P;
  const long SN = (long)t.S * t.n;
  const double* ph = phi + (long)(m0 + (col ? li : 0)) * phi_stride;
  double ff = 0.0;
  const int e1 = (bx + 1) * FOM_EPB < t.nT ? (bx + 1) * FOM_EPB : t.nT;
  for (int e = bx * FOM_EPB + wave; e < e1; e += 4) {
    if (!col) continue;
    const long g0 = (long)s * t.n + e * 10;
    double ue[10];
#pragma unroll
    for (int j = 0; j < 10; ++j) ue[j] = uk[(g0 + j) * 16 + li];
#pragma unroll
    for (int ks = 0; ks < 3; ++ks) {
      const int i = lk + 4 * ks;
      if (i >= 10) continue;
      const long d = g0 + i;
      const double* tm = t.TM + t.elem_type[e] * 100 + i * 10;
      double acc = 0.0;
#pragma unroll
      for (int j = 0; j < 10; ++j) acc += tm[j] * ue[j];
      double bs = ph[0] * b_K[d];
      for (int j = 1; j < K; ++j) bs = __fma_rn(ph[j], b_K[(long)j * SN + d], bs);
      const double f = acc + dt * bs;
      r[d * 16 + li] = f - y[d * 16 + li];
      ff += f * f;
    }
  }
  ff += __shfl_xor(ff, 16);
  ff += __shfl_xor(ff, 32);
  if (lk == 0) red[wave][li] = ff;
  __syncthreads();
  if (tid < 16) part[((long)s * gridDim.x + bx) * 16 + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}

}  // namespace

extern "C" {

int64_t lrbms3_fom_implicit_euler_batch_work_size(lrbms3_ctx* ctx, int32_t nmu) {
  const int64_t base = lrbms3_fom_solve_batch_work_size(ctx, nmu);
  if (base < 0) return -1;
  const T3& t = ctx->t;
  return base + 16 * (int64_t)t.S * ((t.nT + FOM_EPB - 1) / FOM_EPB);          // + the partials of |M u_k + dt sum_j phi b_j|^2
}

}  // extern "C"

namespace {

// The driver of lrbms3_fom_implicit_euler_batch (tv == false: theta [nmu][Q], one table per panel for all its steps) and of its
// _tv twin (tv == true: theta_t [nmu][nt+1][Q], the panel's table is filled with dt x row k + 1 ahead of the step k -> k + 1;
// DESIGN.md 9.18).  The preconditioner of the call sits at the mean over the columns of ThetaRows::bar.
int fom3_euler_batch_drive(lrbms3_ctx* ctx, const std::string& name, bool tv, int Q, int K, int nmu, const double* theta, double dt,
                           int nt, const double* A_diag, const double* A_cpl, const double* b_K, const double* phi, double* work,
                           double* U, double rtol, int max_iter, double* info, void* stream) {
  LRBMS_REQUIRE_MESH(ctx);
  const T3& t = ctx->t;
  if (t.S_ext != t.S) return lrbms_fail(ctx, LRBMS_E_INVALID, name + ": needs all subdomains on this rank");
  if (Q < 1 || Q > 8 || nmu < 1 || nmu > 64 || K < 1 || K > 64 || nt < 1 || max_iter < 1 || !(rtol > 0.0) || !(dt > 0.0))
    return lrbms_fail(ctx, LRBMS_E_INVALID, name + ": bad Q / nmu / K / nt / dt / max_iter / rtol");
  if (!theta || !A_diag || !A_cpl || !b_K || !phi || !work || !U) return lrbms_fail(ctx, LRBMS_E_INVALID, name + ": null argument");
  const ThetaRows tr{theta, Q, tv ? nt + 1 : 0};
  hipStream_t st = (hipStream_t)stream;
  const long S = t.S, nd = S * t.nT * 500, ncp = S * 6 * t.ncf * 100, total = S * t.n;
  FomWork w = fom_work(t, work);
  FomBatch3 b;
  b.carve(t, w, work + lrbms3_fom_solve_work_size(ctx));
  double* pff = work + lrbms3_fom_solve_batch_work_size(ctx, nmu);
  // one preconditioner per call, both levels on the step operator at the mean theta of its columns (summed in column order);
  // never the elliptic solves' kept inverse
  QV tb{};
  for (int q = 0; q < Q; ++q) {
    double acc = 0.0;
    for (int m = 0; m < nmu; ++m) acc += tr.bar(m, q);
    tb.v[q] = dt * (acc / nmu);
  }
  launch_combine(st, nd, Q, tb, A_diag, w.Amu);
  launch_combine(st, ncp, Q, tb, A_cpl, w.Cmu);
  hipLaunchKernelGGL(k3p_fom_add_mass, dim3((unsigned)((S * t.nT * 100 + 255) / 256)), dim3(256), 0, st, t, S * t.nT * 100, w.Amu);
  hipLaunchKernelGGL(k3f_block_inverse, dim3((t.nT + 63) / 64, S), dim3(64), 0, st, t, w.Amu, w.Dinv);
  LRBMS_LAUNCH_CHECK(ctx);
  int nc = 0;
  const double* A1inv = nullptr;
  if (int rc = fom_coarse(ctx, st, w, false, nc, A1inv)) return rc;
  const long slab = total * nmu;
  const unsigned gv = (unsigned)((total * 16 + 255) / 256);
  double its_sum = 0.0, worst = 0.0;
  bool missed = false;
  for (int i = 0; i < 8; ++i) ctx->fombe_panels[i] = 0.0;
  for (int m0 = 0; m0 < nmu; m0 += 16) {
    const int P = nmu - m0 < 16 ? nmu - m0 : 16;
    Fb3Op op{Q, P, nmu, m0, {}, A_diag, A_cpl, true};
    auto fill = [&](int row) {
      for (int c = 0; c < 16; ++c)
        for (int q = 0; q < 8; ++q) op.th.v[c][q] = (c < P && q < Q) ? dt * tr.at(m0 + c, row, q) : 0.0;
    };
    if (!tv) fill(0);
    double its_p = 0.0, worst_p = 0.0;
    for (int step = 0; step < nt; ++step) {
      if (tv) fill(step + 1);                                // the operator of the step k -> k + 1: row k + 1
      const double* Uk = U + step * slab;
      double* X = U + (step + 1) * slab;
      hipLaunchKernelGGL(k3fb_load, dim3(gv), dim3(256), 0, st, total, P, nmu, m0, Uk, X, b.p);
      fomb3_launch_matvec(ctx, st, w, op, b.p, b.y, b.ppy);
      hipLaunchKernelGGL(k3fb_step_residual, dim3(w.nbx, S), dim3(256), 0, st, t, dt, K, P, m0, (long)(nt + 1) * K,
                         phi + (long)(step + 1) * K, b_K, b.p, b.y, b.r, pff);
      int it = 0;
      double rel = 0.0;
      if (int rc = fomb3_panel_run(ctx, st, w, b, op, nc, A1inv, X, pff, rtol, max_iter, &it, &rel, name.c_str())) return rc;
      its_p += it;
      if (rel > worst_p) worst_p = rel;
      if (rel > rtol) {                                      // this panel stops here; its later slabs are not written
        missed = true;
        break;
      }
    }
    ctx->fombe_panels[m0 / 16 * 2] = its_p;
    ctx->fombe_panels[m0 / 16 * 2 + 1] = worst_p;
    its_sum += its_p;
    if (worst_p > worst) worst = worst_p;
  }
  if (info) info[0] = its_sum, info[1] = worst;
  if (missed) return lrbms_fail(ctx, LRBMS_E_NOT_CONVERGED, name + ": CG did not reach rtol");
  return LRBMS_OK;
}

}  // namespace

extern "C" {

int lrbms3_fom_implicit_euler_batch(lrbms3_ctx* ctx, int32_t Q, int32_t K, int32_t nmu, const double* theta, double dt, int32_t nt,
                                    const double* A_diag, const double* A_cpl, const double* b_K, const double* phi, double* work,
                                    double* U, double rtol, int32_t max_iter, double* info, void* stream) {
  return fom3_euler_batch_drive(ctx, "fom_implicit_euler_batch", false, Q, K, nmu, theta, dt, nt, A_diag, A_cpl, b_K, phi, work, U, rtol,
                                max_iter, info, stream);
}

int lrbms3_fom_implicit_euler_batch_tv(lrbms3_ctx* ctx, int32_t Q, int32_t K, int32_t nmu, const double* theta_t, double dt, int32_t nt,
                                       const double* A_diag, const double* A_cpl, const double* b_K, const double* phi, double* work,
                                       double* U, double rtol, int32_t max_iter, double* info, void* stream) {
  return fom3_euler_batch_drive(ctx, "fom_implicit_euler_batch_tv", true, Q, K, nmu, theta_t, dt, nt, A_diag, A_cpl, b_K, phi, work, U,
                                rtol, max_iter, info, stream);
}

int lrbms3_fom_implicit_euler_batch_panel_info(lrbms3_ctx* ctx, double* out) {
  if (!ctx || !out) return LRBMS_E_INVALID;
  for (int i = 0; i < 8; ++i) out[i] = ctx->fombe_panels[i];
  return LRBMS_OK;
}

}  // extern "C"
