// Internal definitions shared by the 3D / P2 translation units of liblrbms_hip.so (gfx950 only): the counterpart of
// lrbms_dev.h for lrbms3d.hip (context, assembly, pass, estimator, full-order solvers), online3d.hip (reduced solvers),
// sources3d.hip and enrich3d.hip.  Everything that crosses a file sits in the namespace lrbms3
// (the 2D units keep internals of the same names); no kernel is defined here: a kernel that a second file needs is reached
// through its home file's launch_* function.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>

#include <rocsolver/rocsolver.h>

#include "../../include/lrbms3d_hip.h"
#include "lrbms_ctx_base.h"

namespace lrbms3 {

typedef double d4 __attribute__((ext_vector_type(4)));

struct T3 {
  int S, S_ext, nT, n, nrt, ncf, nbf, nvs, nnodes, nb, nbel, nsel, nbd;
  int nA, nB, nC, nFs, nFf, o_fs, o_ff, o_c, lam_stride, hat_stride, f_stride;
  double volume, kmin;
  const int *nbr, *phys;
  const int *elem_type, *up_face, *order, *nb_elem, *nb_out, *face_pos, *tsign, *elem_rt, *rt_e0, *rt_f0, *rt_e1, *rt_f1;
  const int *side_elem, *side_face, *side_elem_out, *side_face_out;
  const int *dof_node, *node_ptr, *node_dofs, *node_mask, *node_count, *side_nodes, *sn_ptr, *sn_dofs;
  const int *dof_bslot, *bn_ptr, *bn_slots, *bnodes, *bnode_sides, *bel_elem, *bel_bnode, *sel_elem, *sel_sf;
  const double *divc, *TV, *TE, *TAA, *TFo, *TFn, *TFb, *TPo, *TPn, *TPb, *TC, *TCb, *TPH, *TM, *TB, *TAB, *WB, *WC;
  const double* TSP;     // [6][nA + 8 nFs][100] diagonal block of the local energy product: TV | per face (TPo | TPb)
  const double* TSD;     // [6][nA + 8 nFs][100] system diagonal block: TV | per face (TFo | TFb)  (built at mesh upload)
  const double* zeros;   // [64] zeros: target of the loads of padding lanes
};

}  // namespace lrbms3

struct lrbms3_ctx : lrbms_ctx_base {
  lrbms3::T3 t{};
  std::vector<int32_t> nbr_host;
  // coarse space of the full-order solver (lrbms3_fom_coarse_space): nc functions per subdomain, values at the local DoFs
  int fom_nc = 0;
  double* fom_phi = nullptr;      // [n][4] device, zero-padded columns
  bool fom_keep = false;          // lrbms3_fom_precond_keep: the coarse inverse of a solve stays in the context for the next ones
  double* fom_pc = nullptr;       // [M][M] device (owned), valid for fom_pc_M = nc S unknowns of fom_pc_nc functions
  long fom_pc_M = 0;
  int fom_pc_nc = 0;
  double fomb_panels[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // lrbms3_fom_solve_batch: (iterations, final ratio) of the up to four panels of the last call
  double fombe_panels[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // lrbms3_fom_implicit_euler_batch: (iterations over the steps, worst ratio) per panel of the last call
  void* blas = nullptr;           // rocBLAS handle (dense coarse inverses), created on first use
  const double* user_pc = nullptr;   // coarse inverse the batched reduced solve uses (lrbms3_reduced_precond_use), caller-owned
  int user_pc_N = 0;
  double* thbar = nullptr;         // [8] device: theta(mu_bar) of lrbms3_assemble_energy_product
  double* tm_inv = nullptr;        // [6][100] device (owned): inverses of the element mass tables (parabolic path, first use)
  const double* tm_inv_src = nullptr;   // the TM table they were taken from (a new mesh upload invalidates them)
  double* pg_part = nullptr;       // K-split partial results of the k3_pg kernels (library-owned, grown on demand)
  long pg_part_cap = 0;
  // launch policy (lrbms3_ctx_set_option): the library reads no environment variable
  int opt_ksplit = 0, opt_serial = 0, opt_waves = 0, opt_estimate_valu = 0, opt_solve_valu = 0, opt_fom_coarse = 1;
  double* src_phi = nullptr;       // [64][64] device (owned): source coefficients of lrbms3_reduced_solve_batch_src, first use
  int num_cus = 0;                 // compute units of the device (lrbms3_combine_sources sizes its grid by them), first use
  bool side_padding = false;       // some side has fewer faces than ncf (unequal cubes per direction): padded factor rows exist
  // restricted pass (lrbms3_pass_set_subset): device lists [S] each (one ctx-owned allocation, made at the first restriction)
  bool sub_active = false;
  int* sub_own = nullptr;          // changed local subdomains, ascending: phase 1 runs over them
  int* sub_side = nullptr;         // local subdomains that are changed or have a changed face neighbour, ascending: phase 2
  int sub_own_n = 0, sub_side_n = 0;
};

namespace lrbms3 {

__device__ inline int side_slot(int side) { return side < 3 ? side : side + 1; }

// RT0 orientation of (element, face) in subdomain s: +1 = outward from this element
__device__ inline int sgn3(const T3& t, int s, int e, int f) {
  const int nb = t.nb_elem[e * 4 + f];
  if (nb < 0 && ((t.phys[s] >> (-(nb + 1))) & 1)) return 1;
  return t.tsign[e * 4 + f];
}

// Workgroups are dealt round-robin to the 8 XCDs, each with its own L2.  The row blocks of one subdomain read overlapping basis
// rows, so a 1D grid is decoded such that all blocks of a subdomain get ids that are equal modulo 8 (one XCD) and close in time:
// chunks of 8 subdomains, inside a chunk the subdomain is the fast index.  Returns false for the padding of the last chunk.
__device__ inline bool xcd_block(int nblk, int S, int& xblk, int& s) {
  const int L = blockIdx.x, chunk = L / (8 * nblk), in = L - chunk * 8 * nblk;
  s = chunk * 8 + (in & 7);
  xblk = in >> 3;
  return s < S;
}
inline unsigned xcd_grid(int nblk, int S) { return (unsigned)((S + 7) / 8 * 8 * nblk); }

struct QV { double v[8]; };
// theta table of <= 16 columns: a group of the batched reduced solvers (online3d.hip), a panel of the batched full-order ones (lrbms3d.hip)
struct TB { double v[16][8]; };     // theta [nmu][Q]

// elements (10 rows each) per workgroup of the full-order solver kernels and of the kernels that share their partial-sum layout
constexpr int FOM_EPB = 24;

// arguments of the estimate kernels (lrbms3d.hip): the coefficients u, the factored estimator operators of the pass, eta the output
struct EA {
  const double *u, *G_nc, *G_bb, *G_rdd, *G_ab, *G_aa, *r_fd, *Rb, *Yb, *Dp, *Xab, *As, *Cn, *ebar, *Bbb, *bdiv, *f2, *ceps;
  double hdiam;
  double* eta;
};

inline QV make_theta(int Q, const double* theta) {
  QV th{};
  for (int q = 0; q < Q && q < 8; ++q) th.v[q] = theta[q];
  return th;
}

// Host tables of the batched parabolic drivers and their _tv twins: theta [nmu][Q] with rows == 0 (the twin: a row
// stride of zero, every step reads the one row), theta_t [nmu][rows][Q] with rows == nt + 1 (row k: the time of step k).
struct ThetaRows {
  const double* theta;
  int Q, rows;
  double at(int m, int k, int q) const { return rows ? theta[((long)m * rows + k) * Q + q] : theta[(long)m * Q + q]; }
  // what the call's preconditioner takes for column m: the entry itself, or the mean over the rows 1 .. nt summed in ascending
  // order (nt == 1: row 1 exactly)
  double bar(int m, int q) const {
    if (!rows) return theta[(long)m * Q + q];
    double acc = 0.0;
    for (int k = 1; k < rows; ++k) acc += at(m, k, q);
    return acc / (rows - 1);
  }
};

// ---- host functions that cross files.  Kernels that a second file launches (the bodies are one hipLaunchKernelGGL each, grid,
// block and LDS as at the launches of the home file):
// online3d.hip, called by lrbms3d.hip (the full-order solvers) and enrich3d.hip
void launch_combine(hipStream_t st, long per_q, int Q, const QV& th, const double* B, double* Amu);                  // k3_combine
// online3d.hip, called by lrbms3d.hip (fom_euler_run)
void launch_axpy(hipStream_t st, long total, const double* x, double* y);                                            // k3p_axpy
// lrbms3d.hip, called by enrich3d.hip
void launch_fom_block_inverse(hipStream_t st, const T3& t, const double* Amu, double* Dinv);                         // k3f_block_inverse
// lrbms3d.hip, called by enrich3d.hip (the corrector trajectories): slot 0 of Amu [S][n_T][5][100] += the element mass
void launch_fom_add_mass(hipStream_t st, const T3& t, double* Amu);                                                  // k3p_fom_add_mass
// lrbms3d.hip, called by online3d.hip (red_cg, red_euler_run)
void launch_reduce1(hipStream_t st, int S, const double* part, double* out);                                         // k3_reduce1
// lrbms3d.hip (owner of ctx->blas), called there (fom_coarse) and by online3d.hip: A^-1 of a dense SPD matrix into Id (identity on entry) by
// rocSOLVER potrf / potrs on the stream; hinfo != 0 (and LRBMS_OK) when A is not positive definite
int dense_spd_inverse(lrbms3_ctx* ctx, hipStream_t st, long M, double* A, double* Id, rocblas_int* pinfo, rocblas_int& hinfo);
// lrbms3d.hip, called there (lrbms3_reduced_estimate_batch) and by online3d.hip (the batched parabolic estimate): the launches of the
// batched estimate for the nmu columns of the panel a.u [S][N][nmu] into a.eta [3][S][nmu] on st -- the 16-column matrix-core form
// where its LDS fits and LRBMS3_OPT_ESTIMATE_VALU is 0, else the 8-column VALU form.  estimate_batch_form: 16 / 8 = the form the
// helper will launch, 0 = neither fits the LDS (the helper would return LRBMS_E_INVALID): known before any launch.
int estimate_batch_form(const lrbms3_ctx* ctx, int Q, int N);
int launch_reduced_estimate_batch(lrbms3_ctx* ctx, hipStream_t st, int Q, int N, int nmu, const double* theta, const EA& a);      // k3_estimate_batch16 / k3_estimate_batch
// lrbms3d.hip, called by online3d.hip: the nonconformity form alone, a.eta [S][nmu] (a.u, G_nc, As, Cn, ebar are read, nothing else);
// estimate_nc16_fits: its LDS bound
bool estimate_nc16_fits(const lrbms3_ctx* ctx, int N);
int launch_estimate_nc_batch(lrbms3_ctx* ctx, hipStream_t st, int N, int nmu, const EA& a);                                         // k3_estimate_nc_batch16
// sources3d.hip, called there (lrbms3_reduced_source_terms) and by online3d.hip: out [S][L]; source_terms_fits: its LDS bound
bool source_terms_fits(const lrbms3_ctx* ctx, int N);
void launch_source_terms(hipStream_t st, const T3& t, int Q, int N, int K, int L, const double* theta, const double* phi, const double* F2,
                         const double* r_fd_K, const double* bdiv_K, const double* Rb, const double* u, const double* ceps, double hdiam,
                         double* out);                                                                                              // k3_source_terms

}  // namespace lrbms3
