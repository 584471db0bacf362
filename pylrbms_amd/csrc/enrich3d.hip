// 3D / P2 path: online enrichment -- the Dirichlet correction blocks and the batched neighbourhood corrector PCG k3l_* behind
// lrbms3_assemble_dirichlet_correction, lrbms3_local_correction_solve and its implicit Euler form lrbms3_local_correction_euler.
// No other file calls into this one; it combines its operator with launch_combine (online3d.hip), adds the element mass with
// launch_fom_add_mass and inverts the element blocks with launch_fom_block_inverse (lrbms3d.hip).
#include "lrbms3d_dev.h"

using namespace lrbms3;

// ------------------------------------------------------------------------------------------------- online enrichment
// Neighbourhood corrector problems (reference block_swipdg.py:227-316; 2D: csrc/enrich.hip): for a marked subdomain m the SWIPDG
// problem on N(m) = m and its face neighbours with Dirichlet data on the outer boundary, right-hand side the L2 functional of f,
// solution restricted to m.  In the block data: the operator restricted to the members of N(m), the coupling blocks towards
// subdomains outside dropped and the correction block D_corr added to the own element's diagonal block on those faces.
// A 3D neighbourhood does not fit a workgroup (7 x 3 840 unknowns at config 5), so this is a batched multi-kernel PCG in the
// style of lrbms3_fom_solve with a problem dimension: vectors [nmark][7][n] (slot = the slot of nbr[m], absent slots never
// touched), scalars per problem on the device, block-Jacobi from the uncorrected element blocks (SPD, one inverse per element
// for all problems).  The matvec is organised by MEMBER subdomain: a workgroup owns (subdomain, element chunk), reads every
// combined block once and applies it to the vectors of every problem that contains the subdomain.
namespace {

// per problem: [0], [1] r.z of the last two updates (alternating)  [2] p.Ap  [3] r.r  [4] b.b  [5] state: 0 running, 1 converged,
// 2 broken down (p.Ap <= 0 or a NaN)  [6] iterations at the freeze.  A frozen problem is skipped by every kernel: its x stays.
// The Euler form: [4] is |f|^2 of the step, [7] != 0 marks a trajectory that ended (k3l_euler_open), [5] = 3 a step that ran out
// of iterations, kept from then on.
constexpr int LC_SCAL = 8;

// D_corr[q][s][side][pos] = lambda_q at the face points of the own side element . (Dirichlet-face table - inner-face own/own table)
__global__ __launch_bounds__(128) void k3l_dirichlet_correction(T3 t, const double* __restrict__ lam, double* __restrict__ D_corr) {
  const int sf = blockIdx.x, s = blockIdx.y, q = blockIdx.z, c = threadIdx.x;
  if (c >= 100) return;
  const int side = sf / t.ncf, e = t.side_elem[sf], f = t.side_face[sf];
  double acc = 0.0;
  if (e >= 0 && !((t.phys[s] >> side) & 1) && t.nbr[s * 7 + side_slot(side)] >= 0) {
    const double* w = lam + (((long)q * t.S_ext + s) * t.nT + e) * t.lam_stride + t.o_fs + f * t.nFs;
    const long tab = ((long)(t.elem_type[e] * 4 + f) * t.nFs) * 100 + c;
    for (int k = 0; k < t.nFs; ++k) acc += w[k] * (t.TFb[tab + (long)k * 100] - t.TFo[tab + (long)k * 100]);
  }
  D_corr[(((long)q * t.S + s) * t.nbf + sf) * 100 + c] = acc;
}

// p = z + beta p on the present slots of the running problems (the first direction does not read p)
__global__ __launch_bounds__(256) void k3l_dir(T3 t, int first, int cur, const int* __restrict__ marked, const double* __restrict__ scal,
                                               const double* __restrict__ z, double* __restrict__ p) {
  const int slot = blockIdx.y, pm = blockIdx.z;
  const double* sc = scal + (long)pm * LC_SCAL;
  if (sc[5] != 0.0 || t.nbr[marked[pm] * 7 + slot] < 0) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= t.n) return;
  const long d = ((long)pm * 7 + slot) * t.n + i;
  p[d] = first ? z[d] : z[d] + (sc[cur] / sc[cur ^ 1]) * p[d];
}

// y = A_N(m) p for every running problem m that contains the subdomain of this workgroup; partial p.y per (problem, slot, chunk).
// k3f_matvec (block loads of 16 bytes per lane, the symmetric read inside a subdomain, xcd_block) with the blocks of an element
// held in registers over the loop of the <= 7 problems: nbr[s][j] = m marked <=> s sits in slot 6 - j of problem m.  A side
// face with neighbour s' contributes the coupling block times x_m[s'] in problem m = s, times x_m[self] in problem m = s', and
// Dmu times the own element's x in every other problem (s' lies outside that neighbourhood).
__global__ __launch_bounds__(256) void k3l_matvec(T3 t, int nbx, int nmemb, const int* __restrict__ memb, const int* __restrict__ pidx,
                                                  const double* __restrict__ scal, const double* __restrict__ Amu,
                                                  const double* __restrict__ Cmu, const double* __restrict__ Dmu,
                                                  const double* __restrict__ p, double* __restrict__ y, double* __restrict__ part) {
  __shared__ double red[7][4];
  int mi, bx;
  if (!xcd_block(nbx, nmemb, bx, mi)) return;
  const int s = memb[mi];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const bool act = lane < 50;
  const int li = act ? lane : 49, row = li / 5, c2 = 2 * (li - row * 5);
  int pmj[7];
  bool any = false;
#pragma unroll
  for (int j = 0; j < 7; ++j) {
    const int m = t.nbr[s * 7 + j];
    int pm = m >= 0 ? pidx[m] : -1;
    if (pm >= 0 && scal[(long)pm * LC_SCAL + 5] != 0.0) pm = -1;
    pmj[j] = pm;
    any = any || pm >= 0;
  }
  if (!any) return;
  const double* As = Amu + (long)s * t.nT * 500;
  double py[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  const int e1 = (bx + 1) * FOM_EPB < t.nT ? (bx + 1) * FOM_EPB : t.nT;
  for (int e = bx * FOM_EPB + wave; e < e1; e += 4) {
    const int4 nb = *reinterpret_cast<const int4*>(t.nb_elem + e * 4);
    const int nbv[4] = {nb.x, nb.y, nb.z, nb.w};
    const double2 a0 = *reinterpret_cast<const double2*>(As + (long)e * 500 + li * 2);
    double2 af[4], ad[4];
    int kind[4], eo[4], sl[4];        // 0 nothing, 1 the lower element's block (transposed), 2 own block, 3 side face with a neighbour
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      const int ee = nbv[f];          // wave-uniform
      af[f] = ad[f] = make_double2(0.0, 0.0);
      kind[f] = 0, eo[f] = 0, sl[f] = 0;
      if (ee >= 0 && ee < e) {
        const int4 nb2 = *reinterpret_cast<const int4*>(t.nb_elem + ee * 4);
        const int fb = nb2.x == e ? 0 : (nb2.y == e ? 1 : (nb2.z == e ? 2 : 3));
        af[f] = *reinterpret_cast<const double2*>(As + (long)ee * 500 + (1 + fb) * 100 + li * 2);
        kind[f] = 1, eo[f] = ee;
      } else if (ee >= 0) {
        af[f] = *reinterpret_cast<const double2*>(As + (long)e * 500 + (1 + f) * 100 + li * 2);
        kind[f] = 2, eo[f] = ee;
      } else {
        const int side = -(ee + 1);
        sl[f] = side_slot(side);
        if (t.nbr[s * 7 + sl[f]] >= 0) {
          const long off = (((long)s * 6 + side) * t.ncf + t.face_pos[e * 4 + f]) * 100 + li * 2;
          af[f] = *reinterpret_cast<const double2*>(Cmu + off);
          ad[f] = *reinterpret_cast<const double2*>(Dmu + off);
          kind[f] = 3, eo[f] = t.nb_out[e * 4 + f];
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 7; ++j) {
      const int pm = pmj[j];          // wave-uniform
      if (pm < 0) continue;
      const double* P = p + (long)pm * 7 * t.n;
      const double* ps = P + (long)(6 - j) * t.n;
      double yr, yc0 = 0.0, yc1 = 0.0;                // row sums (valid in lanes 5 i), column sums (valid in lanes 0 .. 4)
      {
        const double2 pv = *reinterpret_cast<const double2*>(ps + e * 10 + c2);
        yr = act ? a0.x * pv.x + a0.y * pv.y : 0.0;
      }
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        if (kind[f] == 1) {
          const double pr = ps[eo[f] * 10 + row];
          yc0 += act ? af[f].x * pr : 0.0;
          yc1 += act ? af[f].y * pr : 0.0;
        } else if (kind[f] == 2) {
          const double2 pv = *reinterpret_cast<const double2*>(ps + eo[f] * 10 + c2);
          yr += act ? af[f].x * pv.x + af[f].y * pv.y : 0.0;
        } else if (kind[f] == 3) {
          const bool cpl = j == 3 || j == sl[f];      // the neighbour across this side belongs to the problem
          const double* pn = j == 3 ? P + (long)sl[f] * t.n + eo[f] * 10 : (j == sl[f] ? P + 3L * t.n + eo[f] * 10 : ps + e * 10);
          const double2 a = cpl ? af[f] : ad[f];
          const double2 pv = *reinterpret_cast<const double2*>(pn + c2);
          yr += act ? a.x * pv.x + a.y * pv.y : 0.0;
        }
      }
      // row sums: lanes l .. l + 4 (fixed order), result in lanes 5 i;  column sums: lanes l, l + 5, ..., l + 45, result in lanes 0 .. 4
      double r1 = yr + __shfl_down(yr, 1);
      r1 = r1 + __shfl_down(r1, 2);
      const double rs = r1 + __shfl_down(yr, 4);
      double c0 = yc0 + __shfl_down(yc0, 5), c1 = yc1 + __shfl_down(yc1, 5);
      c0 += __shfl_down(c0, 10); c1 += __shfl_down(c1, 10);
      c0 += __shfl_down(c0, 20); c1 += __shfl_down(c1, 20);
      c0 += __shfl_down(yc0 + __shfl_down(yc0, 5), 40); c1 += __shfl_down(yc1 + __shfl_down(yc1, 5), 40);
      const int tl = lane < 10 ? lane : 0;
      const double ya = __shfl(rs, 5 * tl), yb0 = __shfl(c0, tl >> 1), yb1 = __shfl(c1, tl >> 1);
      if (lane < 10) {
        const double v = ya + ((lane & 1) ? yb1 : yb0);
        y[((long)pm * 7 + (6 - j)) * t.n + e * 10 + lane] = v;
        py[j] += v * ps[e * 10 + lane];
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 7; ++j) {
    double v = py[j];
    for (int o = 8; o > 0; o >>= 1) v += __shfl_down(v, o);          // lanes 0 .. 9 (others are zero)
    if (lane == 0) red[j][wave] = v;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int j = 0; j < 7; ++j)
      if (pmj[j] >= 0) part[((long)pmj[j] * 7 + (6 - j)) * nbx + bx] = (red[j][0] + red[j][1]) + (red[j][2] + red[j][3]);
  }
}

// k3f_update per (chunk, slot, problem): x += alpha p, r -= alpha y, z = Dinv r with the element inverses of the slot's subdomain;
// partial r.z and r.r (init: x = 0, r = b of the member subdomain)
__global__ __launch_bounds__(256) void k3l_update(T3 t, int init, int cur, const int* __restrict__ marked, const double* __restrict__ scal,
                                                  const double* __restrict__ Dinv, const double* __restrict__ p, const double* __restrict__ y,
                                                  const double* __restrict__ b, double* __restrict__ x, double* __restrict__ r,
                                                  double* __restrict__ z, double* __restrict__ prz, double* __restrict__ prr) {
  __shared__ double rs[256], red[256];
  const int slot = blockIdx.y, pm = blockIdx.z, tid = threadIdx.x;
  const double* sc = scal + (long)pm * LC_SCAL;
  const int s = t.nbr[marked[pm] * 7 + slot];
  if (s < 0 || (!init && sc[5] != 0.0)) return;
  const int el = tid / 10, i = tid - el * 10, e = blockIdx.x * FOM_EPB + el;
  const bool on = el < FOM_EPB && e < t.nT;
  const long d = ((long)pm * 7 + slot) * t.n + e * 10 + i;
  double ri = 0.0;
  if (on) {
    if (init) {
      ri = b[(long)s * t.n + e * 10 + i];
      x[d] = 0.0;
    } else {
      const double alpha = sc[cur] / sc[2];
      x[d] += alpha * p[d];
      ri = r[d] - alpha * y[d];
    }
    r[d] = ri;
  }
  rs[tid] = ri;
  __syncthreads();
  double zi = 0.0;
  if (on) {
    const double* D = Dinv + ((long)s * t.nT + e) * 56;          // packed upper triangle (k3f_block_inverse)
#pragma unroll
    for (int j = 0; j < 10; ++j) {
      const int a = i < j ? i : j, bb = i < j ? j : i;
      zi += D[a * (21 - a) / 2 + bb - a] * rs[el * 10 + j];
    }
    z[d] = zi;
  }
  const long blk = ((long)pm * 7 + slot) * gridDim.x + blockIdx.x;
  red[tid] = ri * zi;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) red[tid] += red[tid + w];
    __syncthreads();
  }
  if (tid == 0) prz[blk] = red[0];
  __syncthreads();
  red[tid] = ri * ri;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) red[tid] += red[tid + w];
    __syncthreads();
  }
  if (tid == 0) prr[blk] = red[0];
}

// One workgroup per problem: the partials of its present slots and chunks summed in a fixed order (the same whatever else is in
// the batch), then the problem's scalars and its state.
//   mode 0 (after the init update):  pa -> r.z [0], pb -> r.r [3] and b.b [4];  b = 0: converged at 0 iterations (x = 0)
//   mode 1 (after the matvec):       pa -> p.Ap [2];  p.Ap <= 0 (or NaN): broken down, x stays where it is
//   mode 2 (after the update):       pa -> r.z [nxt], pb -> r.r [3];  sqrt(r.r / b.b) <= rtol: converged after it + 1 iterations
__global__ __launch_bounds__(256) void k3l_reduce(T3 t, int mode, int nbx, int it, int nxt, double rtol, const int* __restrict__ marked,
                                                  const double* __restrict__ pa, const double* __restrict__ pb, double* __restrict__ scal) {
  __shared__ double ra[256], rb[256];
  const int pm = blockIdx.x, tid = threadIdx.x;
  double* sc = scal + (long)pm * LC_SCAL;
  if (mode != 0 && sc[5] != 0.0) return;
  const int m = marked[pm], cnt = 7 * nbx;
  double a = 0.0, b = 0.0;
  for (int k = tid; k < cnt; k += 256) {
    if (t.nbr[m * 7 + k / nbx] < 0) continue;
    a += pa[(long)pm * cnt + k];
    if (pb) b += pb[(long)pm * cnt + k];
  }
  ra[tid] = a;
  rb[tid] = b;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) {
      ra[tid] += ra[tid + w];
      rb[tid] += rb[tid + w];
    }
    __syncthreads();
  }
  if (tid != 0) return;
  a = ra[0], b = rb[0];
  if (mode == 0) {
    sc[0] = a, sc[3] = b, sc[4] = b;
    sc[5] = b == 0.0 ? 1.0 : (b == b ? 0.0 : 2.0);
    sc[6] = 0.0;
  } else if (mode == 1) {
    sc[2] = a;
    if (!(a > 0.0)) sc[5] = 2.0, sc[6] = (double)it;
  } else {
    sc[nxt] = a, sc[3] = b;
    if (!(b == b) || !(a == a)) sc[5] = 2.0, sc[6] = (double)(it + 1);
    else if (sqrt(b / sc[4]) <= rtol) sc[5] = 1.0, sc[6] = (double)(it + 1);
  }
}

// corr [nmark][n] = the self slot of x
__global__ __launch_bounds__(256) void k3l_restrict(int n, const double* __restrict__ x, double* __restrict__ corr) {
  const int i = blockIdx.x * 256 + threadIdx.x, pm = blockIdx.y;
  if (i < n) corr[(long)pm * n + i] = x[((long)pm * 7 + 3) * n + i];
}

// ---- corrector trajectories (lrbms3_local_correction_euler): implicit Euler on the same neighbourhoods.  x is
// the state x_k; a step is the PCG above on M_N + dt A_N, warm-started at x_k, so only its opening differs: y = H x_k by
// k3l_matvec with p := x, then k3l_euler_rhs and k3l_euler_reduce0 in place of the init update and its reduce.

// x_0 = 0 on the present slots
__global__ __launch_bounds__(256) void k3l_euler_zero(T3 t, const int* __restrict__ marked, double* __restrict__ x) {
  const int slot = blockIdx.y, pm = blockIdx.z;
  if (t.nbr[marked[pm] * 7 + slot] < 0) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < t.n) x[((long)pm * 7 + slot) * t.n + i] = 0.0;
}

// Opens a step: a problem whose previous step broke down or ran out of iterations has ended for good ([7] != 0, state != 0: every
// kernel skips it and x keeps its last state); every other problem runs again.
__global__ __launch_bounds__(256) void k3l_euler_open(int nmark, int first, double* __restrict__ scal) {
  const int pm = blockIdx.x * 256 + threadIdx.x;
  if (pm >= nmark) return;
  double* sc = scal + (long)pm * LC_SCAL;
  if (first) {
    sc[5] = 0.0, sc[7] = 0.0;
  } else if (sc[7] != 0.0 || sc[5] != 1.0) {
    sc[7] = 1.0;
    if (sc[5] == 0.0) sc[5] = 3.0;
  } else {
    sc[5] = 0.0;
  }
}

// Per (chunk, slot, problem), rows as k3l_update: f = TM x_k + dt sum_j phi[j] b_K[j] on the elements of the slot's subdomain (the
// sums in the order of k3p_fom_rhs_src), r = f - y with y = H x_k, z = Dinv r; partial r.z, r.r and f.f
__global__ __launch_bounds__(256) void k3l_euler_rhs(T3 t, double dt, int K, long SN, const int* __restrict__ marked,
                                                     const double* __restrict__ scal, const double* __restrict__ Dinv,
                                                     const double* __restrict__ phi, const double* __restrict__ b_K,
                                                     const double* __restrict__ x, const double* __restrict__ y, double* __restrict__ r,
                                                     double* __restrict__ z, double* __restrict__ prz, double* __restrict__ prr,
                                                     double* __restrict__ pff) {
  __shared__ double rs[256], red[256];
  const int slot = blockIdx.y, pm = blockIdx.z, tid = threadIdx.x;
  const int s = t.nbr[marked[pm] * 7 + slot];
  if (s < 0 || scal[(long)pm * LC_SCAL + 5] != 0.0) return;
  const int el = tid / 10, i = tid - el * 10, e = blockIdx.x * FOM_EPB + el;
  const bool on = el < FOM_EPB && e < t.nT;
  const long d = ((long)pm * 7 + slot) * t.n + e * 10 + i;
  double fi = 0.0, ri = 0.0;
  if (on) {
    const double* tm = t.TM + t.elem_type[e] * 100 + i * 10;
    const double* xe = x + ((long)pm * 7 + slot) * t.n + e * 10;
    const long ds = (long)s * t.n + e * 10 + i;
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < 10; ++j) acc += tm[j] * xe[j];
    double bs = phi[0] * b_K[ds];
    for (int j = 1; j < K; ++j) bs = __fma_rn(phi[j], b_K[(long)j * SN + ds], bs);
    fi = acc + dt * bs;
    ri = fi - y[d];
    r[d] = ri;
  }
  rs[tid] = ri;
  __syncthreads();
  double zi = 0.0;
  if (on) {
    const double* D = Dinv + ((long)s * t.nT + e) * 56;          // packed upper triangle (k3f_block_inverse)
#pragma unroll
    for (int j = 0; j < 10; ++j) {
      const int a = i < j ? i : j, bb = i < j ? j : i;
      zi += D[a * (21 - a) / 2 + bb - a] * rs[el * 10 + j];
    }
    z[d] = zi;
  }
  const long blk = ((long)pm * 7 + slot) * gridDim.x + blockIdx.x;
  const double term[3] = {ri * zi, ri * ri, fi * fi};
  double* const out[3] = {prz, prr, pff};
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    red[tid] = term[q];
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
      if (tid < w) red[tid] += red[tid + w];
      __syncthreads();
    }
    if (tid == 0) out[q][blk] = red[0];
    __syncthreads();
  }
}

// k3l_reduce for the opening of a step (one workgroup per running problem, the same summation order): r.z [0], r.r [3], f.f [4].
// f = 0 (the leading steps of a source that starts late) or a first residual within rtol: converged at 0 iterations, x_{k+1} = x_k.
__global__ __launch_bounds__(256) void k3l_euler_reduce0(T3 t, int nbx, double rtol, const int* __restrict__ marked,
                                                         const double* __restrict__ prz, const double* __restrict__ prr,
                                                         const double* __restrict__ pff, double* __restrict__ scal) {
  __shared__ double ra[256], rb[256], rc[256];
  const int pm = blockIdx.x, tid = threadIdx.x;
  double* sc = scal + (long)pm * LC_SCAL;
  if (sc[5] != 0.0) return;
  const int m = marked[pm], cnt = 7 * nbx;
  double a = 0.0, b = 0.0, c = 0.0;
  for (int k = tid; k < cnt; k += 256) {
    if (t.nbr[m * 7 + k / nbx] < 0) continue;
    a += prz[(long)pm * cnt + k];
    b += prr[(long)pm * cnt + k];
    c += pff[(long)pm * cnt + k];
  }
  ra[tid] = a, rb[tid] = b, rc[tid] = c;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) {
      ra[tid] += ra[tid + w];
      rb[tid] += rb[tid + w];
      rc[tid] += rc[tid + w];
    }
    __syncthreads();
  }
  if (tid != 0) return;
  a = ra[0], b = rb[0], c = rc[0];
  sc[0] = a, sc[3] = b, sc[4] = c, sc[6] = 0.0;
  if (!(a == a) || !(b == b) || !(c == c)) sc[5] = 2.0;
  else if (c == 0.0 || sqrt(b / c) <= rtol) sc[5] = 1.0;
}

// corr [M][nt] = traj [nt][M]^T through a 32 x 32 LDS tile.  The reads are coalesced along M (32 consecutive doubles per row of
// threads).  On the write side a row of 32 threads covers one m: min(nt - k0, 32) consecutive doubles, so for the small nt of this
// path (2 .. 10) a wave writes two runs of nt doubles and most of its lanes idle.  Once per call, after the last step.
__global__ __launch_bounds__(256) void k3l_traj_transpose(long M, int nt, const double* __restrict__ traj, double* __restrict__ corr) {
  __shared__ double tile[32][33];
  const long m0 = (long)blockIdx.x * 32;
  const int k0 = blockIdx.y * 32, tx = threadIdx.x, ty = threadIdx.y;
  for (int j = ty; j < 32; j += 8)
    if (k0 + j < nt && m0 + tx < M) tile[j][tx] = traj[(long)(k0 + j) * M + m0 + tx];
  __syncthreads();
  for (int j = ty; j < 32; j += 8)
    if (m0 + j < M && k0 + tx < nt) corr[(m0 + j) * nt + k0 + tx] = tile[tx][j];
}

// work layout of lrbms3_local_correction_solve
struct LcWork {
  int nbx;
  long nvec, npart;
  double *Amu, *Cmu, *Dmu, *Dinv, *x, *r, *z, *p, *y, *ppy, *prz, *prr, *scal;
  int *marked, *pidx, *memb;
};

long lc_work(const T3& t, long nmark, double* work, LcWork* w) {
  const long S = t.S, nd = S * t.nT * 500, ncp = S * 6 * t.ncf * 100;
  const int nbx = (t.nT + FOM_EPB - 1) / FOM_EPB;
  const long nvec = nmark * 7 * t.n, npart = nmark * 7 * nbx;
  if (w) {
    LcWork& l = *w;
    l.nbx = nbx, l.nvec = nvec, l.npart = npart;
    l.Amu = work;                       // every vector below starts at an even offset: the matvec loads 16 bytes per lane
    l.Cmu = l.Amu + nd;
    l.Dmu = l.Cmu + ncp;
    l.Dinv = l.Dmu + ncp;
    l.x = l.Dinv + S * t.nT * 56;
    l.r = l.x + nvec;
    l.z = l.r + nvec;
    l.p = l.z + nvec;
    l.y = l.p + nvec;
    l.ppy = l.y + nvec;
    l.prz = l.ppy + npart;
    l.prr = l.prz + npart;
    l.scal = l.prr + npart;
    l.marked = (int*)(l.scal + nmark * LC_SCAL);      // [nmark] | pidx [S] | memb [S]
    l.pidx = l.marked + nmark;
    l.memb = l.pidx + S;
  }
  return nd + 2 * ncp + S * t.nT * 56 + 5 * nvec + 3 * npart + nmark * LC_SCAL + (nmark + 2 * S + 1) / 2;
}

// The refusals both corrector exports share (args_ok: what the export itself requires of its arguments) and their host tables:
// tab = marked | problem index of a subdomain (-1: not marked) | the subdomains that belong to some problem, ascending
int lc_tables(lrbms3_ctx* ctx, const char* name, int Q, int nmark, const int32_t* marked, bool args_ok, std::vector<int>& tab, int& nmemb) {
  const T3& t = ctx->t;
  const std::string nm(name);
  if (t.S_ext != t.S) return lrbms_fail(ctx, LRBMS_E_INVALID, nm + ": needs all subdomains on this rank");
  if (Q < 1 || Q > 8 || nmark < 1 || nmark > 65535 || !args_ok) return lrbms_fail(ctx, LRBMS_E_INVALID, nm + ": bad argument");
  const long S = t.S;
  tab.assign((size_t)nmark + 2 * S, -1);
  int* pidx = tab.data() + nmark;
  int* memb = pidx + S;
  for (int k = 0; k < nmark; ++k) {
    const int m = marked[k];
    if (m < 0 || m >= S) return lrbms_fail(ctx, LRBMS_E_INVALID, nm + ": marked subdomain " + std::to_string(m) + " out of range");
    if (pidx[m] >= 0) return lrbms_fail(ctx, LRBMS_E_INVALID, nm + ": subdomain " + std::to_string(m) + " marked twice");
    pidx[m] = k;
    tab[k] = m;
  }
  nmemb = 0;
  for (int s = 0; s < S; ++s) {
    bool in = false;
    for (int j = 0; j < 7; ++j) in = in || (ctx->nbr_host[(size_t)s * 7 + j] >= 0 && pidx[ctx->nbr_host[(size_t)s * 7 + j]] >= 0);
    if (in) memb[nmemb++] = s;
  }
  return LRBMS_OK;
}

// The tables onto the device, then the operator of the call: the blocks combined with th, with the element mass on the own blocks
// for the Euler form (th = dt theta), and the element inverses of the uncorrected diagonal blocks
int lc_operator(lrbms3_ctx* ctx, hipStream_t st, const LcWork& w, const std::vector<int>& tab, int Q, const QV& th, const double* A_diag,
                const double* A_cpl, const double* D_corr, bool mass) {
  const T3& t = ctx->t;
  const long S = t.S, nd = S * t.nT * 500, ncp = S * 6 * t.ncf * 100;
  LRBMS_HIP_CHECK(ctx, hipMemcpyAsync(w.marked, tab.data(), sizeof(int) * tab.size(), hipMemcpyHostToDevice, st));
  LRBMS_HIP_CHECK(ctx, hipStreamSynchronize(st));
  launch_combine(st, nd, Q, th, A_diag, w.Amu);
  launch_combine(st, ncp, Q, th, A_cpl, w.Cmu);
  launch_combine(st, ncp, Q, th, D_corr, w.Dmu);
  if (mass) launch_fom_add_mass(st, t, w.Amu);
  launch_fom_block_inverse(st, t, w.Amu, w.Dinv);
  return LRBMS_OK;
}

// The PCG iterations of a batch whose opening (r, z and the scalars [0], [3], [4], [5], [6]) has been launched: the scalars are
// read, then direction, matvec, reduce, update, reduce per iteration with a poll every 16, until every problem is frozen, max_iter,
// or -- stop_on_breakdown -- some problem broke down.  sc: the scalars of the last poll, it: the iterations issued.
int lc_iterate(lrbms3_ctx* ctx, hipStream_t st, const LcWork& w, int nmark, int nmemb, const double* b, double rtol, int max_iter,
               bool stop_on_breakdown, std::vector<double>& sc, int& it) {
  const T3& t = ctx->t;
  const int nbx = w.nbx;
  const dim3 gupd(nbx, 7, nmark), gdir((t.n + 255) / 256, 7, nmark);
  auto poll = [&](bool& all_done, bool& broken) -> int {
    LRBMS_HIP_CHECK(ctx, hipMemcpyAsync(sc.data(), w.scal, sizeof(double) * sc.size(), hipMemcpyDeviceToHost, st));
    LRBMS_HIP_CHECK(ctx, hipStreamSynchronize(st));
    all_done = true, broken = false;
    for (int k = 0; k < nmark; ++k) {
      all_done = all_done && sc[(size_t)k * LC_SCAL + 5] != 0.0;
      broken = broken || (stop_on_breakdown && sc[(size_t)k * LC_SCAL + 5] == 2.0);
    }
    return LRBMS_OK;
  };
  bool all_done = false, broken = false;
  int rc = poll(all_done, broken);
  if (rc != LRBMS_OK) return rc;
  it = 0;
  const int check = 16;
  while (!all_done && !broken && it < max_iter) {
    for (int k = 0; k < check && it < max_iter; ++k, ++it) {
      const int cur = it & 1;
      hipLaunchKernelGGL(k3l_dir, gdir, dim3(256), 0, st, t, it == 0 ? 1 : 0, cur, w.marked, w.scal, w.z, w.p);
      hipLaunchKernelGGL(k3l_matvec, dim3(xcd_grid(nbx, nmemb)), dim3(256), 0, st, t, nbx, nmemb, w.memb, w.pidx, w.scal, w.Amu, w.Cmu,
                         w.Dmu, w.p, w.y, w.ppy);
      hipLaunchKernelGGL(k3l_reduce, dim3(nmark), dim3(256), 0, st, t, 1, nbx, it, 0, rtol, w.marked, w.ppy, (const double*)nullptr, w.scal);
      hipLaunchKernelGGL(k3l_update, gupd, dim3(256), 0, st, t, 0, cur, w.marked, w.scal, w.Dinv, w.p, w.y, b, w.x, w.r, w.z, w.prz, w.prr);
      hipLaunchKernelGGL(k3l_reduce, dim3(nmark), dim3(256), 0, st, t, 2, nbx, it, cur ^ 1, rtol, w.marked, w.prz, w.prr, w.scal);
    }
    LRBMS_LAUNCH_CHECK(ctx);
    if ((rc = poll(all_done, broken)) != LRBMS_OK) return rc;
  }
  return LRBMS_OK;
}

}  // namespace

extern "C" {

int lrbms3_assemble_dirichlet_correction(lrbms3_ctx* ctx, int32_t Q, const double* lam, double* D_corr, void* stream) {
  LRBMS_REQUIRE_MESH(ctx);
  if (Q < 1 || Q > 8 || !lam || !D_corr) return lrbms_fail(ctx, LRBMS_E_INVALID, "assemble_dirichlet_correction: bad argument");
  const T3& t = ctx->t;
  hipLaunchKernelGGL(k3l_dirichlet_correction, dim3(t.nbf, t.S, Q), dim3(128), 0, (hipStream_t)stream, t, lam, D_corr);
  LRBMS_LAUNCH_CHECK(ctx);
  return LRBMS_OK;
}

int64_t lrbms3_local_correction_work_size(lrbms3_ctx* ctx, int32_t nmark) {
  if (!ctx || !ctx->has_mesh || nmark < 1) return -1;
  return (int64_t)lc_work(ctx->t, nmark, nullptr, nullptr);
}

int lrbms3_local_correction_solve(lrbms3_ctx* ctx, int32_t Q, const double* theta, int32_t nmark, const int32_t* marked,
                                  const double* A_diag, const double* A_cpl, const double* D_corr, const double* b, double* work,
                                  double* corr, double rtol, int32_t max_iter, double* info, void* stream) {
  LRBMS_REQUIRE_MESH(ctx);
  const T3& t = ctx->t;
  std::vector<int> tab;
  int nmemb = 0;
  int rc = lc_tables(ctx, "local_correction_solve", Q, nmark, marked,
                     theta && marked && A_diag && A_cpl && D_corr && b && work && corr && rtol > 0.0 && max_iter >= 1, tab, nmemb);
  if (rc != LRBMS_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  LcWork w;
  lc_work(t, nmark, work, &w);
  if ((rc = lc_operator(ctx, st, w, tab, Q, make_theta(Q, theta), A_diag, A_cpl, D_corr, false)) != LRBMS_OK) return rc;
  const int nbx = w.nbx;
  hipLaunchKernelGGL(k3l_update, dim3(nbx, 7, nmark), dim3(256), 0, st, t, 1, 0, w.marked, w.scal, w.Dinv, w.p, w.y, b, w.x, w.r, w.z,
                     w.prz, w.prr);
  hipLaunchKernelGGL(k3l_reduce, dim3(nmark), dim3(256), 0, st, t, 0, nbx, 0, 0, rtol, w.marked, w.prz, w.prr, w.scal);
  LRBMS_LAUNCH_CHECK(ctx);
  std::vector<double> sc((size_t)nmark * LC_SCAL);
  int it = 0;
  if ((rc = lc_iterate(ctx, st, w, nmark, nmemb, b, rtol, max_iter, true, sc, it)) != LRBMS_OK) return rc;
  hipLaunchKernelGGL(k3l_restrict, dim3((t.n + 255) / 256, nmark), dim3(256), 0, st, t.n, w.x, corr);
  LRBMS_LAUNCH_CHECK(ctx);
  int bad = -1, bad_state = 0;
  for (int k = 0; k < nmark; ++k) {
    const double* s8 = sc.data() + (size_t)k * LC_SCAL;
    const int state = (int)s8[5];
    if (info) {
      info[2 * k] = state != 0 ? s8[6] : (double)it;
      info[2 * k + 1] = s8[4] > 0.0 ? sqrt(s8[3] / s8[4]) : 0.0;
    }
    if (state != 1 && bad < 0) bad = k, bad_state = state;
  }
  if (bad >= 0)
    return lrbms_fail(ctx, LRBMS_E_NOT_CONVERGED,
                      "local_correction_solve: subdomain " + std::to_string(marked[bad]) +
                          (bad_state == 2 ? ": p.Ap <= 0 (the neighbourhood operator is not positive definite)" : ": not converged"));
  return LRBMS_OK;
}

int64_t lrbms3_local_correction_euler_work_size(lrbms3_ctx* ctx, int32_t nmark, int32_t nt) {
  if (!ctx || !ctx->has_mesh || nmark < 1 || nt < 1) return -1;
  return (int64_t)(lc_work(ctx->t, nmark, nullptr, nullptr) + (long)nt * nmark * ctx->t.n);      // + traj [nt][nmark][n]
}

int lrbms3_local_correction_euler(lrbms3_ctx* ctx, int32_t Q, int32_t K, const double* theta, double dt, int32_t nt, int32_t nmark,
                                  const int32_t* marked, const double* A_diag, const double* A_cpl, const double* D_corr,
                                  const double* b_K, const double* phi, double* work, double* corr, double rtol, int32_t max_iter,
                                  double* info, void* stream) {
  LRBMS_REQUIRE_MESH(ctx);
  const T3& t = ctx->t;
  std::vector<int> tab;
  int nmemb = 0;
  int rc = lc_tables(ctx, "local_correction_euler", Q, nmark, marked,
                     theta && marked && A_diag && A_cpl && D_corr && b_K && phi && work && corr && rtol > 0.0 && max_iter >= 1, tab, nmemb);
  if (rc != LRBMS_OK) return rc;
  if (K < 1 || K > 64) return lrbms_fail(ctx, LRBMS_E_INVALID, "local_correction_euler: need 1 <= K <= 64");
  if (!(dt > 0.0) || nt < 1) return lrbms_fail(ctx, LRBMS_E_INVALID, "local_correction_euler: dt > 0 and nt >= 1 required");
  hipStream_t st = (hipStream_t)stream;
  LcWork w;
  double* traj = work + lc_work(t, nmark, work, &w);            // [nt][nmark][n]
  QV th = make_theta(Q, theta);
  for (int q = 0; q < Q; ++q) th.v[q] *= dt;
  if ((rc = lc_operator(ctx, st, w, tab, Q, th, A_diag, A_cpl, D_corr, true)) != LRBMS_OK) return rc;
  const int nbx = w.nbx;
  const long M = (long)nmark * t.n, SN = (long)t.S * t.n;
  const dim3 gupd(nbx, 7, nmark), gdir((t.n + 255) / 256, 7, nmark);
  hipLaunchKernelGGL(k3l_euler_zero, gdir, dim3(256), 0, st, t, w.marked, w.x);
  std::vector<double> sc((size_t)nmark * LC_SCAL), iters((size_t)nmark, 0.0), worst((size_t)nmark, 0.0);
  std::vector<int> end_step((size_t)nmark, -1), end_state((size_t)nmark, 0);      // the step at which a trajectory ended, and how
  for (int k = 0; k < nt; ++k) {
    hipLaunchKernelGGL(k3l_euler_open, dim3((nmark + 255) / 256), dim3(256), 0, st, nmark, k == 0 ? 1 : 0, w.scal);
    hipLaunchKernelGGL(k3l_matvec, dim3(xcd_grid(nbx, nmemb)), dim3(256), 0, st, t, nbx, nmemb, w.memb, w.pidx, w.scal, w.Amu, w.Cmu,
                       w.Dmu, w.x, w.y, w.ppy);
    hipLaunchKernelGGL(k3l_euler_rhs, gupd, dim3(256), 0, st, t, dt, K, SN, w.marked, w.scal, w.Dinv, phi + (long)(k + 1) * K, b_K, w.x,
                       w.y, w.r, w.z, w.prz, w.prr, w.ppy);
    hipLaunchKernelGGL(k3l_euler_reduce0, dim3(nmark), dim3(256), 0, st, t, nbx, rtol, w.marked, w.prz, w.prr, w.ppy, w.scal);
    LRBMS_LAUNCH_CHECK(ctx);
    int it = 0;
    if ((rc = lc_iterate(ctx, st, w, nmark, nmemb, nullptr, rtol, max_iter, false, sc, it)) != LRBMS_OK) return rc;
    hipLaunchKernelGGL(k3l_restrict, dim3((t.n + 255) / 256, nmark), dim3(256), 0, st, t.n, w.x, traj + (long)k * M);
    LRBMS_LAUNCH_CHECK(ctx);
    for (int pm = 0; pm < nmark; ++pm) {
      if (end_step[pm] >= 0) continue;
      const double* s8 = sc.data() + (size_t)pm * LC_SCAL;
      const int state = (int)s8[5];
      iters[pm] += state != 0 ? s8[6] : (double)it;
      worst[pm] = std::max(worst[pm], s8[4] > 0.0 ? sqrt(s8[3] / s8[4]) : 0.0);
      if (state != 1) end_step[pm] = k, end_state[pm] = state;
    }
  }
  hipLaunchKernelGGL(k3l_traj_transpose, dim3((unsigned)((M + 31) / 32), (nt + 31) / 32), dim3(32, 8), 0, st, M, nt, traj, corr);
  LRBMS_LAUNCH_CHECK(ctx);
  int bad = -1;
  for (int pm = 0; pm < nmark; ++pm) {
    if (info) info[2 * pm] = iters[pm], info[2 * pm + 1] = worst[pm];
    if (end_step[pm] >= 0 && bad < 0) bad = pm;
  }
  if (bad >= 0)
    return lrbms_fail(ctx, LRBMS_E_NOT_CONVERGED,
                      "local_correction_euler: subdomain " + std::to_string(marked[bad]) + ", step " + std::to_string(end_step[bad] + 1) +
                          (end_state[bad] == 2 ? ": p.Ap <= 0 (the neighbourhood operator is not positive definite)" : ": not converged"));
  return LRBMS_OK;
}

}  // extern "C"
