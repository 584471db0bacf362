/*
 * lrbms3d_hip.h -- C ABI of the 3D / P2 hot path in liblrbms_hip.so (BASELINE.json config 5: 3D diffusion, 8x8x8
 * subdomains, SWIPDG p = 2, local basis dim 30).
 *
 * The reference binds the 2D / P1 operators only (python/dune/pylrbms/discretize_elliptic_block_swipdg.py:22-23; :195 uses
 * x[0], x[1]), so these entry points have no reference call site of their own: each one is the 3D / P2 counterpart of the
 * 2D entry point named beside it (include/lrbms_hip.h, which cites the reference line it replaces), with the same rules:
 * caller-allocated device buffers, plain pointers and sizes, int return codes (LRBMS_OK / LRBMS_E_*), explicit hipStream_t.
 *
 * Geometry: Kuhn triangulation (6 tetrahedra per cube), every subdomain a translate of one template of kx x ky x kz cubes,
 * every element a translate of one of 6 reference tetrahedra.  All local integrals are contractions
 *     block[e][c] = sum_k sample[e][k] * TABLE[type(e)][k][c]
 * of coefficient samples (host-evaluated data functions at the quadrature points, as in 2D) with reference tables that the
 * host builds once (pylrbms_amd/grid3d.py) and the context keeps on the device.
 *
 *   S, S_ext     local / local + halo subdomains;  n_T elements, n = 10 n_T DG DoFs, n_rt RT0 DoFs per subdomain
 *   sides        0 = z-, 1 = y-, 2 = x-, 3 = x+, 4 = y+, 5 = z+ ; slots 0..6 = sides 0..2, self (3), sides 3..5
 *   ncf          faces per side, nbf = 6 ncf side faces ("sf" = side * ncf + pos);  nvs nodes per side,  nb boundary nodes
 *   Q, N, QN     affine components, local basis size, Q * N;  columns (q, j) of flux images are q-major
 */
#ifndef LRBMS3D_HIP_H
#define LRBMS3D_HIP_H

#include <stdint.h>

#include "lrbms_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lrbms3_ctx lrbms3_ctx;

typedef struct {
  int32_t n_T, n_rt, ncf, nvs, n_nodes, nb, nbel, nsel, nbd;
  int32_t nA, nB, nC, nFs, nFf;                   /* points of the rules: system volume, product volume, estimator volume,
                                                     system face, flux face */
  int32_t o_fs, o_ff, o_c, lam_stride;            /* lambda_q record: volA | 4 x Fs | 4 x Ff | volC */
  int32_t hat_stride, f_stride;                   /* lambda_hat and f records: volB | volC;  lambda_bar record: volB */
  double volume, kmin;                            /* |T|; smallest eigenvalue of the symmetric part of kappa */
  const int32_t *elem_type;                       /* [n_T] 0..5 */
  const int32_t *up_face;                         /* [n_T][4] faces whose inner neighbour has the higher element index (-1 padded) */
  const int32_t *order;                           /* [n_T] traversal order of the element loops (a permutation; cache locality only) */
  const int32_t *nb_elem, *nb_out, *face_pos, *tsign, *elem_rt;   /* [n_T][4]: inner neighbour or -(1+side); the neighbour's
                                                     element across a side face; position on the side; RT0 orientation; RT0 DoF */
  const int32_t *rt_e0, *rt_f0, *rt_e1, *rt_f1;   /* [n_rt] the (<= 2) own elements of an RT0 face */
  const int32_t *side_elem, *side_face, *side_elem_out, *side_face_out;   /* [6][ncf] */
  const int32_t *dof_node;                        /* [n] Lagrange node of a DG DoF */
  const int32_t *node_ptr, *node_dofs;            /* CSR node -> own DoFs: [n_nodes + 1], [n] */
  const int32_t *node_mask, *node_count;          /* [n_nodes] sides a node lies on (bit a); size of its averaging patch */
  const int32_t *side_nodes;                      /* [6][nvs] node at position p of side a (-1 padded) */
  const int32_t *sn_ptr, *sn_dofs;                /* CSR (side, pos) -> the NEIGHBOUR's DoFs at that node: [6 nvs + 1], [...] */
  const int32_t *dof_bslot;                       /* [n] compact index (0 .. nbd-1) of a DoF on a boundary node, else -1 */
  const int32_t *bn_ptr, *bn_slots;               /* CSR boundary node -> compact indices of its own DoFs: [nb + 1], [nbd] */
  const int32_t *bnodes, *bnode_sides;            /* [nb] boundary nodes; [nb][3] their (side * nvs + pos) memberships, -1 padded */
  const int32_t *bel_elem, *bel_bnode;            /* [nbel] elements with a boundary node; [nbel][10] boundary-node index per DoF or -1 */
  const int32_t *sel_elem, *sel_sf;               /* [nsel] elements with a side face; [nsel][4] side-face index per face or -1 */
  const double *divc;                             /* [6][4] |f| / |T| */
  const double *TV, *TE, *TAA;                    /* [6][nA|nB|nC][100]  w |T| grad phi_i . kappa grad phi_j */
  const double *TFo, *TFn, *TFb;                  /* [6][4][nFs][100]    inner face (own, own) / (own, neighbour); Dirichlet face */
  const double *TPo, *TPn, *TPb;                  /* [6][4][nFs][100]    their penalty parts alone (local energy product) */
  const double *TC, *TCb;                         /* [6][4][nFf][10]     flux coefficients: inner / Dirichlet face */
  const double *TPH, *TM;                         /* [6][nB][10] w |T| phi_i;  [6][100] mass */
  const double *TB, *TAB;                         /* [6][nC][16] w |T| psi_f . kappa^-1 psi_g;  [6][nC][40] w |T| grad phi_i . psi_f */
  const double *WB, *WC;                          /* [nB], [nC] w |T| */
} lrbms3_mesh_desc;

int lrbms3_ctx_create(int device, lrbms3_ctx** out);
int lrbms3_ctx_destroy(lrbms3_ctx* ctx);
const char* lrbms3_last_error(lrbms3_ctx* ctx);

/* Launch policy of the library (no numerical convention).  The library reads no environment variable: these options are the
 * only switches; tests use them to reach every kernel path at small sizes.  2D: lrbms_ctx_set_option.
 *   LRBMS3_OPT_KSPLIT          0 (default): workgroups per (subdomain, operator) of the projection kernels chosen from the launch
 *                              size (1 from ~400 workgroups per kernel on, i.e. at config 5's 512 subdomains); 1 .. 8: forced
 *                              (1 = the in-kernel epilogues, > 1 = partial tiles + k3_pg_combine)
 *   LRBMS3_OPT_SERIAL          1: every kernel of the pass on the caller's stream (kernel statistics of a serial pass)
 *   LRBMS3_OPT_WAVES           0 (default): 4 / 8 waves per workgroup of the projection kernels; else that many
 *   LRBMS3_OPT_ESTIMATE_VALU   1: VALU form of the batched estimate (cross-check of the matrix-core form)
 *   LRBMS3_OPT_SOLVE_VALU      1: VALU form of the batched solver's panel matvec (cross-check)
 *   LRBMS3_OPT_FOM_COARSE      0: full-order solves without the coarse level whatever lrbms3_fom_coarse_space set
 *   LRBMS3_OPT_POD_ROTATE_VALU 1: the rotation of lrbms3_local_pod_stream_push through k_pod_xt and a copy back (cross-check) */
#define LRBMS3_OPT_KSPLIT 1
#define LRBMS3_OPT_SERIAL 2
#define LRBMS3_OPT_WAVES 3
#define LRBMS3_OPT_ESTIMATE_VALU 4
#define LRBMS3_OPT_SOLVE_VALU 5
#define LRBMS3_OPT_FOM_COARSE 6
#define LRBMS3_OPT_POD_ROTATE_VALU 7
int lrbms3_ctx_set_option(lrbms3_ctx* ctx, int32_t option, int32_t value);

/* Template, tables, neighbour table nbr [S][7] (index into the S_ext ordering per slot, -1 = none, nbr[s][3] == s) and
 * phys [S_ext] (bit a set: side a lies on the physical boundary).   2D: lrbms_mesh_upload. */
int lrbms3_mesh_upload(lrbms3_ctx* ctx, const lrbms3_mesh_desc* desc, int32_t S, int32_t S_ext, const int32_t* nbr,
                       const int32_t* phys);

/* -- offline assembly ------------------------------------------------------------------------------------------------- */
/* SWIPDG system (sigma = 20 / 38, beta = 1/2).  lam [Q][S_ext][n_T][lam_stride];
 *   A_diag [Q][S][n_T][5][100]  block-ELL: 0 = (e, e), 1 + f = (e, inner neighbour across face f)
 *   A_cpl  [Q][S][6][ncf][100]  block (own side element, neighbour's element) per coupling face, zero on physical sides
 * 2D: lrbms_assemble_swipdg. */
int lrbms3_assemble_system(lrbms3_ctx* ctx, int32_t Q, const double* lam, double* A_diag, double* A_cpl, void* stream);
/* f_smp [S][n_T][f_stride], lhat [S][n_T][hat_stride] -> b [S][n], f2 [S], ceps [S], bdiv [S][n_T] = int_T f.  2D: lrbms_assemble_rhs. */
int lrbms3_assemble_rhs(lrbms3_ctx* ctx, const double* f_smp, const double* lhat, double* b, double* f2, double* ceps,
                        double* bdiv, void* stream);
/* lbar [S][n_T][nB] -> ebar [S][n_T][100] (E_ii element blocks);  Aaa [Q][Q][S][n_T][100], Aab [Q][S][n_T][10][4],
 * Bbb [S][n_T][4][4] (RT0 orientation signs folded in).  2D: lrbms_assemble_products. */
int lrbms3_assemble_products(lrbms3_ctx* ctx, int32_t Q, const double* lam, const double* lbar, const double* lhat, double* ebar,
                             double* Aaa, double* Aab, double* Bbb, void* stream);
/* Local energy product of every subdomain (reference: local_energy_dg_product_i, discretize_elliptic_block_swipdg.py:651-677, the
 * product the local bases are orthonormalised in, reductor.py:19-31): sum_q theta_bar_q [volume term of lambda_q + the PENALTY
 * terms of the faces inside the subdomain + the Dirichlet penalty, with the inside coefficient, on every face of the subdomain
 * boundary (coupling or physical: all-Dirichlet boundary info on the subdomain layer, :658)].  theta_bar [Q] host;
 * P_diag [S][n_T][5][100] block-ELL like A_diag (no coupling blocks: the product is local).  2D: P_diag of lrbms_assemble_products. */
int lrbms3_assemble_energy_product(lrbms3_ctx* ctx, int32_t Q, const double* theta_bar, const double* lam, double* P_diag,
                                   void* stream);

/* Y [S][n][M] = P_diag X (the local energy product applied to M vectors per subdomain): Gram-Schmidt of the reductor.
 * 2D: lrbms_blockell_apply. */
int lrbms3_energy_product_apply(lrbms3_ctx* ctx, int32_t M, const double* P_diag, const double* X, double* Y, void* stream);

/* Local POD basis extension, the batched method of snapshots per subdomain: lrbms_local_pod of include/lrbms_hip.h (algorithm,
 * arguments, the work formula with this path's S and n, limits and refusals are the same, the kernels are shared) with the local
 * energy product P_diag [S][n_T][5][100] applied as lrbms3_energy_product_apply does.  U [S][n][L] with 1 <= L <= 128,
 * V [S(_ext)][n][Nw] with Nw <= 64, nloc / added / info [S] int32 on the device, sv [S][L].  n > 512: the reductions over n
 * (V^T P R, R^T P R) run in min(8, ceil(n / 512)) pieces that are summed in their order.  rtol < 1e-7 is refused (the Gram
 * matrix squares the singular values). */
int64_t lrbms3_local_pod_work_size(lrbms3_ctx* ctx, int32_t L, int32_t Nw);
int lrbms3_local_pod(lrbms3_ctx* ctx, int32_t L, int32_t Nw, int32_t modes, double rtol, double atol, const double* P_diag,
                     const double* U, double* V, int32_t* nloc, double* sv, int32_t* added, int32_t* info, double* work,
                     void* stream);

/* Streamed local POD over a training set of any size (incremental HAPOD): lrbms_local_pod_stream_* of include/lrbms_hip.h --
 * algorithm, state and work layouts and their size formulas (state: S (2 n Lx + 3) doubles, Lx = keep + cmax; work: the formula
 * stated there, with this path's S and n), limits, refusals and kernels are the same -- with the local energy product P_diag
 * [S][n_T][5][100].  LRBMS3_OPT_POD_ROTATE_VALU 1 selects the k_pod_xt route of the rotation (cross-check). */
int64_t lrbms3_local_pod_stream_state_size(lrbms3_ctx* ctx, int32_t keep, int32_t cmax);
int64_t lrbms3_local_pod_stream_work_size(lrbms3_ctx* ctx, int32_t keep, int32_t cmax, int32_t Nw);
int lrbms3_local_pod_stream_begin(lrbms3_ctx* ctx, int32_t keep, int32_t cmax, double* state, void* stream);
int lrbms3_local_pod_stream_push(lrbms3_ctx* ctx, int32_t keep, int32_t cmax, int32_t C, int32_t Nw, const double* P_diag,
                                 const double* U, const double* V, const int32_t* nloc, double* state, double* work, void* stream);
int lrbms3_local_pod_stream_finish(lrbms3_ctx* ctx, int32_t keep, int32_t cmax, int32_t Nw, int32_t modes, double rtol, double atol,
                                   const double* P_diag, double* V, int32_t* nloc, double* state, double* sv, int32_t* added,
                                   int32_t* info, double* lost, double* work, void* stream);

/* Cf [Q][S_ext][n_T][4][10]: contribution of the element's own DoFs to the RT0 DoF of its face f (unsigned; the kernels
 * apply the orientation).  2D: lrbms_assemble_flux. */
int lrbms3_assemble_flux(lrbms3_ctx* ctx, int32_t Q, const double* lam, double* Cf, void* stream);

/* -- project + estimate-offline (the timed region) ----------------------------------------------------------------------- */
/* One pass over all local subdomains: Oswald interpolation error and RT0 flux reconstruction of the local bases, Galerkin
 * projection of the system and of the estimator operators, in the FACTORED layout (cf. lrbms_project_estimate_fused_factored):
 *   V [S_ext][n][N] (halo filled)
 *   B_sys [Q][S][7][N][N], rhs_red [S][N]
 *   G_nc [S][N][N], G_bb, G_rdd [S][QN][QN], G_ab [Q][S][N][QN], G_aa [Q][Q][S][N][N], r_fd [S][QN]      the [self, self] blocks
 *   Rb, Yb, Dp [S][nbf][QN], Xab [Q][S][nbf][N]     per side face: neighbour's flux image; rows of B R_self, vol div div R_self,
 *                                                   A_ab^T V at the face
 *   As [S][6][nvs][N], Cn [S][nb][N]                per side node: neighbour's share of the vertex average; -P^T E W_self
 * so that for coefficients u (own u_s, neighbours u_a), ur = (theta_q u)_q, zf = Rb ur_a (per side face), z = sum_a As u_a:
 *   nc  = u_s^T G_nc u_s + 2 z^T Cn u_s + sum_e z_e^T ebar_e z_e
 *   df  = ur^T G_bb ur + 2 zf^T Yb ur + sum_e zf_e^T Bbb_e zf_e + 2 sum_q theta_q (u_s^T G_ab_q ur + zf^T Xab_q u_s) + sum theta theta u_s^T G_aa u_s
 *   rdd = ur^T G_rdd ur + 2 zf^T Dp ur + sum_e |T| (div zf_e)^2,   rfd = r_fd^T ur + sum_e bdiv_e div zf_e
 * work >= lrbms3_work_size doubles (flux image R_self [S][n_rt][QN], vertex averages [S][n_nodes][N], rows of E W_self at
 * the boundary DoFs [S][nbd][N]). */
int64_t lrbms3_work_size(lrbms3_ctx* ctx, int32_t Q, int32_t N);
int lrbms3_project_estimate(lrbms3_ctx* ctx, int32_t Q, int32_t N, const double* V, const double* A_diag, const double* A_cpl,
                            const double* b, const double* ebar, const double* Aaa, const double* Aab, const double* Bbb,
                            const double* bdiv, const double* Cf, double* work, double* B_sys, double* rhs_red, double* G_nc,
                            double* G_bb, double* G_rdd, double* G_ab, double* G_aa, double* r_fd, double* Rb, double* Yb,
                            double* Dp, double* Xab, double* As, double* Cn, void* stream);

/* The same pass in two halves for a sharded run that overlaps its halo exchange with compute: phase 1 reads the first S
 * (rank-local) slabs of V only -- everything but the neighbours' shares; phase 2 needs the halo slabs and writes Rb, As and the
 * coupling blocks of B_sys.  phase 0 == lrbms3_project_estimate; 1 followed by 2 is bit-identical to 0 (same buffers, same
 * work).  2D: lrbms_project_estimate_fused_phase. */
int lrbms3_project_estimate_phase(lrbms3_ctx* ctx, int32_t phase, int32_t Q, int32_t N, const double* V, const double* A_diag,
                                  const double* A_cpl, const double* b, const double* ebar, const double* Aaa, const double* Aab,
                                  const double* Bbb, const double* bdiv, const double* Cf, double* work, double* B_sys,
                                  double* rhs_red, double* G_nc, double* G_bb, double* G_rdd, double* G_ab, double* G_aa,
                                  double* r_fd, double* Rb, double* Yb, double* Dp, double* Xab, double* As, double* Cn, void* stream);

/* Incremental re-projection: restrict every following lrbms3_project_estimate, lrbms3_project_estimate_phase and
 * lrbms3_project_sources of this context to the subdomains whose basis changed.  changed [count] is a HOST array of strictly
 * ascending indices in the S_ext ordering, in [0, S_ext) (a changed halo slab re-projects the side arrays of its local neighbours).
 * Everything phase 1 writes depends on the subdomain's own slab only, everything phase 2 writes on the slabs of the subdomain and
 * of its face neighbours (nbr; no diagonal dependence), so the library derives two lists from `changed` and the neighbour table:
 *   own list    the changed indices < S;
 *   side list   the local subdomains that are changed or have a changed face neighbour (ascending).
 * Under the restriction a pass writes
 *   the own arrays of exactly the own list: G_aa, G_ab, G_nc, G_bb, G_rdd, r_fd, rhs_red, the diagonal slot of B_sys, Yb, Dp, Xab,
 *   Cn and the three parts of `work` (with padded side tables the listed rows of Yb, Dp, Xab are cleared first, not the arrays);
 *   the side arrays of exactly the side list: Rb, As and the six coupling slots of B_sys;
 * every other row of every output and of `work` keeps its bits; strides stay those of all S subdomains.  Phase 1 covers the own
 * list and phase 2 the side list; 1 followed by 2 stays bit-identical to 0.  lrbms3_project_sources writes the rows of the own list.
 * Launch sizes, the automatic K-split included, follow the list lengths; an empty list launches nothing.
 * The lists are copied before the call returns (after a device synchronisation: a pass in flight keeps the lists it started with).
 * count == 0 lifts the restriction (changed may be NULL), and so does lrbms3_mesh_upload.  LRBMS_E_INVALID with a message, and
 * nothing changed, for count < 0, an index out of range, a list that is not strictly ascending, and a context without a mesh.
 * 2D: lrbms_fused_set_subset. */
int lrbms3_pass_set_subset(lrbms3_ctx* ctx, const int32_t* changed, int32_t count);

/* Per-kernel device timing of the pass, as lrbms_kernel_timing / lrbms_kernel_timing_read. */
int lrbms3_kernel_timing(lrbms3_ctx* ctx, int32_t enable);
int lrbms3_kernel_timing_read(lrbms3_ctx* ctx, char* names, int64_t names_cap, double* ms, int32_t cap, int32_t* count);

/* -- online ---------------------------------------------------------------------------------------------------------------- */
/* Local estimator terms from the factored operators.  theta [Q] host; u [S_ext][N]; eta_loc [3][S]: nc, r (scaled by
 * (1/pi^2) / c_eps h^2), df -- squared quantities.  2D: lrbms_reduced_estimate_factored. */
int lrbms3_reduced_estimate(lrbms3_ctx* ctx, int32_t Q, int32_t N, const double* theta, const double* u, const double* G_nc,
                            const double* G_bb, const double* G_rdd, const double* G_ab, const double* G_aa, const double* r_fd,
                            const double* Rb, const double* Yb, const double* Dp, const double* Xab, const double* As,
                            const double* Cn, const double* ebar, const double* Bbb, const double* bdiv, const double* f2,
                            const double* ceps, double hdiam, double* eta_loc, void* stream);

/* Throughput form: nmu parameters at once (passes of 8): theta [nmu][Q] host, u [S_ext][N][nmu] (parameter fastest, the layout
 * lrbms3_reduced_solve_batch returns), eta_loc [3][S][nmu].  Every operator and factor is read once per pass of 8.
 * 2D: lrbms_reduced_estimate_batch_factored. */
int lrbms3_reduced_estimate_batch(lrbms3_ctx* ctx, int32_t Q, int32_t N, int32_t nmu, const double* theta, const double* u,
                                  const double* G_nc, const double* G_bb, const double* G_rdd, const double* G_ab, const double* G_aa,
                                  const double* r_fd, const double* Rb, const double* Yb, const double* Dp, const double* Xab,
                                  const double* As, const double* Cn, const double* ebar, const double* Bbb, const double* bdiv,
                                  const double* f2, const double* ceps, double hdiam, double* eta_loc, void* stream);

/* (sum_q theta_q B_sys_q) u = rhs_red by block-Jacobi preconditioned CG on the 7-slot block-sparse reduced system (S_ext == S).
 * info[0] = iterations, info[1] = final relative residual (host, may be NULL).  2D: lrbms_reduced_solve. */
int64_t lrbms3_reduced_solve_work_size(lrbms3_ctx* ctx, int32_t N);
int lrbms3_reduced_solve(lrbms3_ctx* ctx, int32_t Q, int32_t N, const double* theta, const double* B_sys, const double* rhs_red,
                         double* work, double* u, double rtol, int32_t max_iter, double* info, void* stream);

/* Throughput form of the reduced solve: nmu <= 64 parameters at once (N <= 32), in groups of <= 16.  theta [nmu][Q] host;
 * u [S][N][nmu] (parameter fastest).  Inside a group every projected block is read once per CG iteration for all its parameters
 * (panel matvec on the matrix cores), independent CG scalars per parameter; preconditioner: the inverse diagonal blocks at the
 * group-mean theta, or the prebuilt two-level one (lrbms3_reduced_precond_use).  The (<= 4) groups run on the caller's stream and
 * the library's three side streams, launches interleaved: their kernels are latency-bound and share the chip.  info[0] =
 * iterations (of the slowest group), info[1] = worst relative residual.  2D: lrbms_reduced_solve_batch. */
int64_t lrbms3_reduced_solve_batch_work_size(lrbms3_ctx* ctx, int32_t N, int32_t nmu);
int lrbms3_reduced_solve_batch(lrbms3_ctx* ctx, int32_t Q, int32_t N, int32_t nmu, const double* theta, const double* B_sys,
                               const double* rhs_red, double* work, double* u, double rtol, int32_t max_iter, double* info,
                               void* stream);

/* Coarse level of lrbms3_reduced_solve_batch's preconditioner, built once per reduced model (2D: lrbms_reduced_precond_build /
 * _use): the Galerkin problem on the FIRST local basis vector of every subdomain (the constant the reductor starts every basis
 * with, reference reductor.py:29-31), A0[s][t] = sum_q theta_q B_sys_q[s][slot of t][0][0], inverted densely (rocSOLVER) at the
 * reference parameter theta; added to the inverse diagonal blocks it halves the iteration count at 8^3 subdomains.  Any SPD
 * preconditioner is admissible, so one build serves every parameter.
 *   lrbms3_reduced_precond_build   theta [Q] host; work: lrbms3_reduced_precond_work_size doubles; pc: lrbms3_reduced_precond_size
 *                                  doubles, caller-owned, filled ([S][S] coarse inverse, then the inverse diagonal blocks
 *                                  [S][N][N] at the same theta); LRBMS_E_INVALID if the coarse matrix is not positive definite
 *   lrbms3_reduced_precond_use     subsequent lrbms3_reduced_solve_batch calls with basis size N use pc (it must stay alive);
 *                                  NULL: the inverse diagonal blocks alone */
int64_t lrbms3_reduced_precond_size(lrbms3_ctx* ctx, int32_t N);
int64_t lrbms3_reduced_precond_work_size(lrbms3_ctx* ctx, int32_t N);
int lrbms3_reduced_precond_build(lrbms3_ctx* ctx, int32_t Q, int32_t N, const double* theta, const double* B_sys, double* work,
                                 double* pc, void* stream);
int lrbms3_reduced_precond_use(lrbms3_ctx* ctx, int32_t N, const double* pc);

/* Snapshot generation: A(mu) x = b on the never-assembled block operator (S_ext == S), CG with a two-level additive
 * preconditioner: the inverse 10 x 10 element blocks plus, if lrbms3_fom_coarse_space was called, the Galerkin coarse problem on
 * nc functions per subdomain (dense (nc S)^2 inverse by rocSOLVER per solve; the 2D solver's coarse space are the subdomain
 * indicator functions).  b, x [S][n]; work: lrbms3_fom_solve_work_size doubles; info[0] = iterations, info[1] = final relative
 * residual (host, may be NULL); LRBMS_E_NOT_CONVERGED above rtol after max_iter.  2D: lrbms_fom_solve
 * (DuneDiscretization._solve, discretize_elliptic_block_swipdg.py:219-225, has no 3D counterpart in the reference).
 *
 * lrbms3_fom_coarse_space: Phi [n][nc], the values of the nc <= 4 coarse functions at the local DoFs -- functions of the
 * subdomain-local coordinates, hence one table for all subdomains (the host mirror passes 1, x, y, z: P1 per subdomain);
 * nc = 0 switches the coarse level off.  Needs the mesh.  The dense coarse problem is capped at 8 192 unknowns: beyond it only
 * the first function is used, beyond 8 192 subdomains none. */
int lrbms3_fom_coarse_space(lrbms3_ctx* ctx, int32_t nc, const double* Phi);
/* keep != 0: the next lrbms3_fom_solve leaves its dense coarse inverse in the context and the following ones reuse it whatever
 * their parameter (any SPD preconditioner is admissible; saves the ~10 ms factorisation per snapshot at config 5) until keep = 0
 * frees it or the coarse space changes. */
int lrbms3_fom_precond_keep(lrbms3_ctx* ctx, int32_t keep);
int64_t lrbms3_fom_solve_work_size(lrbms3_ctx* ctx);
int lrbms3_fom_solve(lrbms3_ctx* ctx, int32_t Q, const double* theta, const double* A_diag, const double* A_cpl, const double* b,
                     double* work, double* x, double rtol, int32_t max_iter, double* info, void* stream);

/* Batched snapshots (2D: lrbms_fom_solve_batch): column m of X [S][n][nmu] (column fastest) solves
 *     (sum_q theta[m][q] A_q) x_m = sum_j phi[m][j] b_K[j]        theta [nmu][Q] host, phi [nmu][K] device, b_K [K][S][n]
 * from x = 0, 1 <= nmu <= 64 columns per call in panels of at most 16, one after the other on the caller's stream.  The panel
 * kernels read the Q uncombined blocks of A_diag / A_cpl once per iteration for all columns of the panel (fp64 matrix cores) and
 * weight them with the column's own theta; there is no combined operator per column.  ONE preconditioner per call, both levels
 * (inverse 10 x 10 element blocks, coarse level of lrbms3_fom_coarse_space) built at the mean theta of the call's columns, summed
 * in column order; the coarse inverse is private to the call, the one lrbms3_fom_precond_keep keeps is neither read nor replaced.
 * x is updated in place in X; max_iter caps ONE panel and is honoured exactly (a call with max_iter = k leaves the k-th PCG iterate
 * of every column).  info[0] = largest iteration count of a panel, info[1] = worst final |r| / |b_m| (host, may be NULL); the host
 * reads r.r per column every 16 iterations.  LRBMS_E_NOT_CONVERGED after a miss (the remaining panels still run).  A column with a
 * zero right-hand side stays exactly zero and has no say in convergence; all right-hand sides zero: LRBMS_OK, info = (0, 0).
 * Fixed summation orders, no atomics: repeat calls give the same bits, equal columns give equal bits wherever they stand.
 * LRBMS_E_INVALID before any launch (work and X untouched): Q outside [1, 8], nmu outside [1, 64], K outside [1, 64], rtol not
 * > 0, max_iter < 1, a null pointer, S_ext != S.  work: lrbms3_fom_solve_batch_work_size doubles (< 0: no mesh, nmu outside
 * [1, 64]).  lrbms3_fom_solve_batch_panel_info: out [4][2] = (iterations, final ratio) per panel of the last call, zeros for
 * panels it did not have. */
int64_t lrbms3_fom_solve_batch_work_size(lrbms3_ctx* ctx, int32_t nmu);
int lrbms3_fom_solve_batch(lrbms3_ctx* ctx, int32_t Q, int32_t nmu, const double* theta, const double* A_diag, const double* A_cpl,
                           int32_t K, const double* phi, const double* b_K, double* work, double* X, double rtol, int32_t max_iter,
                           double* info, void* stream);
int lrbms3_fom_solve_batch_panel_info(lrbms3_ctx* ctx, double* out);

/* y [S][n][M] = sum_q theta_q (A_diag_q x_s + sum_sides A_cpl_q x_neighbour), x [S_ext][n][M].  2D: lrbms_fom_apply. */
int lrbms3_fom_apply(lrbms3_ctx* ctx, int32_t Q, int32_t M, const double* theta, const double* A_diag, const double* A_cpl,
                     const double* x, double* y, void* stream);

/* -- parabolic LRBMS ------------------------------------------------------------------------------------------------------ */
/* M u' + A(mu) u = f with the block L2 product as mass (the 3D counterpart of the 2D parabolic block, include/lrbms_hip.h;
 * reference discretize_parabolic_block_swipdg.py, estimators.py ParabolicEstimator).  The P2 DG mass matrix is
 * element-block-diagonal: every block is the mesh table TM of the element's type, M_s^-1 is TM^-1 per element.  Every export
 * needs S_ext == S (LRBMS_E_INVALID otherwise).
 *
 * lrbms3_mass_inverse_norm2   Y [S][n][L] -> out [S][L] = y^T M_s^-1 y (time residual of the estimate).  2D: lrbms_mass_inverse_norm2.
 * lrbms3_project_mass         V [S_ext][n][N] (the first S slabs are read), 1 <= N <= 64 -> M_red [S][N][N] = V_s^T M_s V_s on the
 *                             fp64 matrix cores; zero-padded basis columns give exact zero rows and columns. */
int lrbms3_mass_inverse_norm2(lrbms3_ctx* ctx, int32_t L, const double* Y, double* out, void* stream);
int lrbms3_project_mass(lrbms3_ctx* ctx, int32_t N, const double* V, double* M_red, void* stream);

/* Implicit Euler (pyMOR's ImplicitEulerTimeStepper(nt)) on the full-order system, all nt steps in one call:
 *   (M + dt A(mu)) u_{k+1} = M u_k + dt b,  k = 0 .. nt-1.
 * The step operator (dt theta-combined blocks, TM added to the (e, e) blocks), its element-block inverses and its coarse level
 * are built once per call; every step is a CG of lrbms3_fom_solve warm-started at u_k.  The coarse inverse that
 * lrbms3_fom_precond_keep holds for the elliptic solves is neither used nor replaced.
 *   theta [Q] host; U [nt+1][S][n]: U[0] = initial value (input), U[1..nt] written; work: lrbms3_fom_implicit_euler_work_size
 *   doubles; info (host, may be NULL): {total CG iterations, worst final residual relative to |M u_k + dt b|}.
 *   LRBMS_E_INVALID if dt <= 0 or nt < 1; LRBMS_E_NOT_CONVERGED if a step misses rtol within max_iter (U[k+1] then holds
 *   that step's last iterate u_k + d, later slabs are untouched; the reduced counterpart does the same).
 * 2D: lrbms_fom_implicit_euler. */
int64_t lrbms3_fom_implicit_euler_work_size(lrbms3_ctx* ctx);
int lrbms3_fom_implicit_euler(lrbms3_ctx* ctx, int32_t Q, const double* theta, double dt, int32_t nt, const double* A_diag,
                              const double* A_cpl, const double* b, double* work, double* U, double rtol, int32_t max_iter,
                              double* info, void* stream);

/* Batched full-order trajectories (2D: lrbms_fom_implicit_euler_batch): 1 <= nmu <= 64 parameters per call.
 * Column m runs
 *     (M + dt A(theta_m)) u_{k+1} = M u_k + dt sum_j phi[m][k+1][j] b_K[j],   k = 0 .. nt-1     (K = 1, phi = 1, b_K = b: the plain source)
 * in panels of at most 16 columns, panels outermost: a panel runs its whole trajectory, then the next one starts; its theta table,
 * pre-multiplied by dt, is one kernel argument for all steps.  Every step is a CG warm-started in place (x = slab k+1 preset to
 * u_k) with the panel kernels of lrbms3_fom_solve_batch on the step operator (the element's TM joins its own block in the matvec).
 * ONE preconditioner per call, both levels on M + dt A(theta_bar) at the mean theta of the call's columns (summed in column
 * order): the inverse 10 x 10 element blocks and the coarse level of lrbms3_fom_coarse_space, private to the call -- the inverse
 * that lrbms3_fom_precond_keep holds is neither read nor replaced, and the result does not depend on the call history.
 *   theta [nmu][Q] host; phi [nmu][nt+1][K] DEVICE (row k: the time of step k; row 0 is not read); b_K [K][S][n];
 *   U [nt+1][S][n][nmu] (parameter fastest): slab 0 is input (the initial values per column, read and never written), slabs
 *   1..nt are written; nothing outside U and work is written.  work: lrbms3_fom_implicit_euler_batch_work_size doubles (-1 for nmu
 *   outside [1, 64] or without a mesh).
 * A step of a panel iterates until its worst column is at or below rtol relative to |M u_k + dt sum_j phi b_j| of that column (the
 * full right-hand side, as lrbms3_fom_implicit_euler, not the start residual); the host reads r.r per column every 16 iterations.
 * A column whose full right-hand side is exactly zero has no say and keeps u_{k+1} = u_k bit for bit.  max_iter caps ONE step of
 * ONE panel and is honoured exactly (nt = 1, max_iter = k: U[1] - U[0] is the k-th PCG iterate of every column).  After a miss
 * that panel stops at that step (its later slabs are not written), the other panels still run and the call returns
 * LRBMS_E_NOT_CONVERGED.  info (host, may be NULL) = (CG iterations summed over panels and steps, worst final ratio).
 * Fixed summation orders, no atomics: repeat calls give the same bits, equal columns give equal bits wherever they stand.
 * LRBMS_E_INVALID before any launch (U[1..] and work untouched): S_ext != S, Q outside [1, 8], K outside [1, 64], nmu outside
 * [1, 64], nt < 1, dt <= 0, rtol <= 0, max_iter < 1, a null pointer (info excepted).
 * lrbms3_fom_implicit_euler_batch_panel_info: out [4][2] host = (iterations summed over the steps, worst ratio) per panel of the
 * last call on this context, zeros for panels it did not have. */
int64_t lrbms3_fom_implicit_euler_batch_work_size(lrbms3_ctx* ctx, int32_t nmu);
int lrbms3_fom_implicit_euler_batch(lrbms3_ctx* ctx, int32_t Q, int32_t K, int32_t nmu, const double* theta, double dt, int32_t nt,
                                    const double* A_diag, const double* A_cpl, const double* b_K, const double* phi, double* work,
                                    double* U, double rtol, int32_t max_iter, double* info, void* stream);
int lrbms3_fom_implicit_euler_batch_panel_info(lrbms3_ctx* ctx, double* out);

/* The reduced counterpart on the projected operators: (M_red + dt sum_q theta_q B_sys_q) u_{k+1} = M_red u_k + dt rhs_red.
 *   B_sys [Q][S][7][N][N], rhs_red [S][N] as the pass writes them, M_red [S][N][N] (lrbms3_project_mass); U [nt+1][S][N]
 *   (U[0] input); work: lrbms3_reduced_implicit_euler_work_size doubles; info as above.  The step operator and its inverse
 *   diagonal blocks are built once; every step runs the block-Jacobi PCG of lrbms3_reduced_solve warm-started at u_k.
 *   Padded unknowns (zero basis columns) stay exactly at their U[0] value.  N <= 64, Q <= 8.  2D: lrbms_reduced_implicit_euler. */
int64_t lrbms3_reduced_implicit_euler_work_size(lrbms3_ctx* ctx, int32_t N);
int lrbms3_reduced_implicit_euler(lrbms3_ctx* ctx, int32_t Q, int32_t N, const double* theta, double dt, int32_t nt,
                                  const double* B_sys, const double* M_red, const double* rhs_red, double* work, double* U,
                                  double rtol, int32_t max_iter, double* info, void* stream);

/* Time-stepping residual of the reduced model: dU [L][S][N] -> out [L][S] = y^T M_red[s]^-1 y, y = (sum_q theta_q B_sys_q dU_l)_s.
 * On padded columns M_red counts as the identity (they contribute 0).  work: lrbms3_reduced_time_residual_work_size doubles.
 * 2D: lrbms_reduced_time_residual. */
int64_t lrbms3_reduced_time_residual_work_size(lrbms3_ctx* ctx, int32_t N);
int lrbms3_reduced_time_residual(lrbms3_ctx* ctx, int32_t Q, int32_t N, int32_t L, const double* theta, const double* B_sys,
                                 const double* M_red, const double* dU, double* work, double* out, void* stream);

/* -- affine sources: f(mu) = sum_j phi_j(mu) f_j on the stationary path, f(t, mu) = sum_j phi_j(t, mu) f_j on the parabolic one ------
 * The 3D counterparts of the two source blocks of include/lrbms_hip.h, K components, 1 <= K <= 64.  The host
 * evaluates the coefficients phi; the library never evaluates an expression.  Per component j, lrbms3_assemble_rhs on its samples
 * gives the load vector and the element integrals: b_K [K][S][n], bdiv_K [K][S][n_T] (its f2 and ceps outputs are not needed).
 * Every export that reads the mesh needs S_ext == S (LRBMS_E_INVALID otherwise); lrbms3_combine_sources is a plain vector
 * operation and needs no mesh.  LRBMS_E_INVALID also for K outside [1, 64] and for a null argument.
 *
 *   lrbms3_assemble_source_gram     f_smp_K [K][S][n_T][f_stride] (K sample tables as for lrbms3_assemble_rhs) ->
 *                                   F2 [S][K][K] = (f_j, f_l)_{L2(Omega_s)}: per element the expression, and per subdomain the
 *                                   reduction order, of the f2 of lrbms3_assemble_rhs; K = 1: that f2 bit for bit.
 *   lrbms3_project_sources          for the basis V [S][n][N] (N <= 64, Q N <= 64) and R_self [S][n_rt][QN], the RT0 flux image of
 *                                   the SAME V: the first S n_rt Q N doubles of the work buffer of a finished
 *                                   lrbms3_project_estimate pass on V (offset 0; the pass leaves it there, read only here):
 *                                     rhs_red_K [K][S][N]  = V_s^T b_K[j][s]
 *                                     r_fd_K    [K][S][QN] = sum_e bdiv_K[j][s][e] div(R_self)_e
 *                                   K = 1 with the discretization's b / bdiv: the pass's rhs_red and r_fd (other summation order).
 *                                   One launch on the fp64 matrix cores; V and R_self are read once, whatever K.
 *   lrbms3_reduced_source_terms     L >= 1 columns u [S][N][L] (column fastest), each with its own theta [L][Q] and phi [L][K]
 *                                   (both DEVICE arrays: one launch serves any number of parameters or time steps):
 *                                     out [S][L] = (phi_l^T F2_s phi_l - 2 sum_j phi_lj (r_fd_K[j][s]^T ur_l + sum_e bdiv_K[j][s][e] div zf_{l,e}))
 *                                                  (1/pi^2) / ceps[s] hdiam^2
 *                                   with ur, zf = Rb ur_a and the side elements of lrbms3_reduced_estimate (Rb [S][nbf][QN] of the
 *                                   pass).  Added to the r row of lrbms3_reduced_estimate_batch run with f2 = 0, r_fd = 0 and
 *                                   bdiv = 0 it gives the residual indicator of f = sum_j phi_lj f_j (the indicator is affine in
 *                                   (f2, r_fd, bdiv)).  N <= 64, Q <= 8.
 *   lrbms3_reduced_solve_batch_src  lrbms3_reduced_solve_batch where column m solves against sum_j phi[m][j] rhs_red_K[j]:
 *                                   theta [nmu][Q] host, phi [nmu][K] host, rhs_red_K [K][S][N], u [S][N][nmu].  Work size
 *                                   lrbms3_reduced_solve_batch_work_size(N, nmu); same limits (N <= 32, nmu <= 64, groups of 16),
 *                                   preconditioner handling (lrbms3_reduced_precond_use), info and error codes; only the start
 *                                   kernel differs.  K = 1, phi = 1: the bits of lrbms3_reduced_solve_batch.  A column whose
 *                                   right-hand side is exactly zero comes back as zeros.
 *   lrbms3_combine_sources          y [M] = sum_j phi[j] x_K[j] for x_K [K][M] (device), phi [K] host; the sum is spelled out with
 *                                   fma from the first product (the order of lrbms3_reduced_solve_batch_src; the kernel of
 *                                   lrbms_combine_sources).  Forms b(mu) (M = S n), rhs_red(mu) (M = S N), bdiv(mu) (M = S n_T).
 *   lrbms3_fom_implicit_euler_src   lrbms3_fom_implicit_euler with the step right-hand side M u_k + dt sum_j phi[k+1][j] b_K[j];
 *                                   phi [nt+1][K] device (row k: the time of step k).  Same work size, info and errors.
 *   lrbms3_reduced_implicit_euler_src  lrbms3_reduced_implicit_euler with M_red u_k + dt sum_j phi[k+1][j] rhs_red_K[j].  N <= 64.
 *                                   Both: K = 1, phi = 1 gives the bits of the export without _src. */
int lrbms3_assemble_source_gram(lrbms3_ctx* ctx, int32_t K, const double* f_smp_K, double* F2, void* stream);
int lrbms3_project_sources(lrbms3_ctx* ctx, int32_t Q, int32_t N, int32_t K, const double* b_K, const double* bdiv_K, const double* V,
                           const double* R_self, double* rhs_red_K, double* r_fd_K, void* stream);
int lrbms3_reduced_source_terms(lrbms3_ctx* ctx, int32_t Q, int32_t N, int32_t K, int32_t L, const double* theta, const double* phi,
                                const double* F2, const double* r_fd_K, const double* bdiv_K, const double* Rb, const double* u,
                                const double* ceps, double hdiam, double* out, void* stream);
int lrbms3_reduced_solve_batch_src(lrbms3_ctx* ctx, int32_t Q, int32_t N, int32_t K, int32_t nmu, const double* theta,
                                   const double* phi, const double* B_sys, const double* rhs_red_K, double* work, double* u,
                                   double rtol, int32_t max_iter, double* info, void* stream);
int lrbms3_combine_sources(lrbms3_ctx* ctx, int32_t K, int64_t M, const double* phi, const double* x_K, double* y, void* stream);
int lrbms3_fom_implicit_euler_src(lrbms3_ctx* ctx, int32_t Q, int32_t K, const double* theta, double dt, int32_t nt,
                                  const double* A_diag, const double* A_cpl, const double* b_K, const double* phi, double* work,
                                  double* U, double rtol, int32_t max_iter, double* info, void* stream);
int lrbms3_reduced_implicit_euler_src(lrbms3_ctx* ctx, int32_t Q, int32_t N, int32_t K, const double* theta, double dt, int32_t nt,
                                      const double* B_sys, const double* M_red, const double* rhs_red_K, const double* phi,
                                      double* work, double* U, double rtol, int32_t max_iter, double* info, void* stream);

/* -- batched reduced trajectories: nmu <= 64 parameters of the parabolic reduced model in one call ----------------
 *   lrbms3_reduced_implicit_euler_batch      column m of U [nt+1][S][N][nmu] (parameter fastest; U[0] input, [S][N][nmu]) is the
 *                                   trajectory of lrbms3_reduced_implicit_euler at theta[m]: per step and per group of <= 16 columns
 *                                   the PCG of lrbms3_reduced_solve_batch on the step operator M_red + dt sum_q theta_qm B_sys_q
 *                                   (the mass is one more block of the panel matvec's self slot; no combined copy per column is
 *                                   written), started at u_k and iterating in place in U[k+1]; up to four groups on four streams.
 *                                   theta [nmu][Q] host; B_sys, M_red, rhs_red [S][N] as for the single export.  One preconditioner
 *                                   per call, built at the call-mean theta: inverse diagonal blocks (identity on zero-padded basis
 *                                   columns, which stay exactly 0) and a coarse level on the first local basis vectors; if that
 *                                   coarse matrix is not positive definite the call runs block-Jacobi alone.  A preconditioner
 *                                   installed with lrbms3_reduced_precond_use belongs to A: it is neither read nor replaced.
 *                                   max_iter caps ONE step: on a miss LRBMS_E_NOT_CONVERGED, the iterate in U[step+1], later slabs
 *                                   untouched.  info (host, may be NULL): {sum over the steps of the slowest group's iterations,
 *                                   worst final residual relative to |M_red u_k + dt b_m|}.  A column with zero data stays exactly 0.
 *                                   Limits: N <= 32, nmu <= 64, Q <= 8, dt > 0, nt >= 1, S_ext == S; every violation and every null
 *                                   pointer is LRBMS_E_INVALID before any launch.
 *                                   work: lrbms3_reduced_implicit_euler_batch_work_size(N, nmu) doubles.
 *   lrbms3_reduced_implicit_euler_batch_src  the same with b_m of step k = sum_j phi[m][k+1][j] rhs_red_K[j]: rhs_red_K [K][S][N],
 *                                   phi [nmu][nt+1][K] on the DEVICE (row k: the time of step k), 1 <= K <= 64.  K = 1, phi = 1: the
 *                                   bits of lrbms3_reduced_implicit_euler_batch.
 * 2D: lrbms_reduced_implicit_euler_batch(_src). */
int64_t lrbms3_reduced_implicit_euler_batch_work_size(lrbms3_ctx* ctx, int32_t N, int32_t nmu);
int lrbms3_reduced_implicit_euler_batch(lrbms3_ctx* ctx, int32_t Q, int32_t N, int32_t nmu, const double* theta, double dt, int32_t nt,
                                        const double* B_sys, const double* M_red, const double* rhs_red, double* work, double* U,
                                        double rtol, int32_t max_iter, double* info, void* stream);
int lrbms3_reduced_implicit_euler_batch_src(lrbms3_ctx* ctx, int32_t Q, int32_t N, int32_t K, int32_t nmu, const double* theta, double dt,
                                            int32_t nt, const double* B_sys, const double* M_red, const double* rhs_red_K,
                                            const double* phi, double* work, double* U, double rtol, int32_t max_iter, double* info,
                                            void* stream);

/* -- batched parabolic estimates: the estimate of nmu <= 64 reduced trajectories in one call -------------------------
 * The 3D counterpart of lrbms_reduced_parabolic_estimate_batch: for column m of the panel U [nt+1][S][N][nmu] (parameter fastest, as
 * lrbms3_reduced_implicit_euler_batch returns it; read only) with theta[m], term for term what
 * InstationaryReducedDiscretization3D.estimate computes for one trajectory:
 *   eta_loc       [3][nt+1][S][nmu]  nc, r, df: the rows of lrbms3_reduced_estimate_batch on U[k], times 2 sqrt(dt / 3)
 *   time_deriv_nc [nt][S][nmu]       sqrt(max(nc(U[k+1] - U[k]), 0) / dt)
 *   time_residual [nt][nmu]          sqrt(dt / 3 sum_s y^T M_red[s]^-1 y),  y = (sum_q theta_qm B_sys_q (U[k+1] - U[k]))_s
 *   eta           [nt+1][nmu]        2 sqrt(dt / 3) (coef[m][0] |nc[:, k]|_2 + coef[m][1] |(r + df)[:, k]|_2), norms of the raw rows over
 *                                    the subdomains
 *   est           [nmu]              |eta|_2 + |time_residual|_2 + |time_deriv_nc|_F
 * theta [nmu][Q] and coef [nmu][2] = (sqrt(gamma_bar / alpha_bar), 1 / sqrt(alpha_hat alpha_bar)) are HOST arrays, read before the
 * call returns (they travel as kernel arguments).  B_sys, M_red as for lrbms3_reduced_implicit_euler_batch; G_nc .. hdiam as for
 * lrbms3_reduced_estimate_batch.  On zero-padded basis columns M_red counts as the identity (lrbms3_reduced_time_residual).
 * Source f(t, mu) = sum_j phi_j f_j with K >= 1 components: phi [nmu][nt+1][K] (DEVICE; row k: the time of U[k]), F2 [S][K][K],
 * r_fd_K [K][S][QN], bdiv_K [K][S][n_T] as for lrbms3_reduced_source_terms, and the caller passes zeroed f2 / r_fd / bdiv; the f terms
 * of column m at step k are added to its r row.  K = 0: the four pointers are NULL and f2 / r_fd / bdiv are the discretization's.
 * Per slab U[k] the call launches what lrbms3_reduced_estimate_batch launches (either form, LRBMS3_OPT_ESTIMATE_VALU); the nc form of
 * the differences runs in a kernel of its own that reads As, G_nc, Cn and ebar only (row 0 of the full estimate where the 16-column
 * form is not in use); the time residual uses the panel matvec of lrbms3_reduced_solve_batch (LRBMS3_OPT_SOLVE_VALU) on groups of
 * <= 16 columns, no combined operator is written.  Everything runs on `stream`, without a host synchronisation and without atomics:
 * fixed summation orders, repeat calls give the same bits, equal columns give equal bits wherever they stand.  Nothing but work
 * and the five outputs is written; a preconditioner installed with lrbms3_reduced_precond_use is neither read nor replaced.
 * Limits: 1 <= nmu <= 64, N <= 32, Q <= 8, Q N <= 64, nt >= 1, dt > 0, 0 <= K <= 64, S_ext == S; every violation, every null pointer
 * (the K pointers: all set with K >= 1, all NULL with K = 0) and a template whose estimate does not fit the LDS is LRBMS_E_INVALID
 * before any launch, outputs and work untouched.  work: lrbms3_reduced_parabolic_estimate_batch_work_size(N, nmu, nt) doubles (-1 for
 * arguments outside the limits or without a mesh).  2D: lrbms_reduced_parabolic_estimate_batch. */
int64_t lrbms3_reduced_parabolic_estimate_batch_work_size(lrbms3_ctx* ctx, int32_t N, int32_t nmu, int32_t nt);
int lrbms3_reduced_parabolic_estimate_batch(lrbms3_ctx* ctx, int32_t Q, int32_t N, int32_t K, int32_t nmu, int32_t nt, double dt,
                                            const double* theta, const double* coef, const double* U, const double* B_sys,
                                            const double* M_red, const double* G_nc, const double* G_bb, const double* G_rdd,
                                            const double* G_ab, const double* G_aa, const double* r_fd, const double* Rb, const double* Yb,
                                            const double* Dp, const double* Xab, const double* As, const double* Cn, const double* ebar,
                                            const double* Bbb, const double* bdiv, const double* f2, const double* ceps, double hdiam,
                                            const double* phi, const double* F2, const double* r_fd_K, const double* bdiv_K, double* work,
                                            double* eta_loc, double* time_deriv_nc, double* time_residual, double* eta, double* est,
                                            void* stream);

/* -- time-dependent diffusion coefficients theta_q(t, mu) on the three batched parabolic exports -------------------
 * The 3D counterparts of the lrbms_*_tv exports.  Each is its twin above with theta_t [nmu][nt+1][Q] (HOST, the
 * shape of phi; row k belongs to the time of step k, every entry positive) in place of theta [nmu][Q]; theta is never baked into an
 * operator, so a row per step is one table refill per step and nothing is rebuilt.  Everything not named here is the twin's contract:
 * limits, max_iter rules, info, refusals before any launch (outputs and work untouched), no atomics, fixed summation orders (repeat
 * calls give the same bits, equal columns give equal bits wherever they stand), and a preconditioner installed with
 * lrbms3_reduced_precond_use is neither read nor replaced.  The twins launch the same kernels with the same arguments as before
 * (they go through the shared drivers with a row stride of zero).
 *   lrbms3_fom_implicit_euler_batch_tv       column m steps with (M + dt A(theta_t[m][k+1])) u_{k+1} = M u_k + dt sum_j phi[m][k+1][j] b_K[j]:
 *                                   the panel's table is filled with dt x row k+1 ahead of every step.  Row 0 is not read.  Work size
 *                                   and lrbms3_fom_implicit_euler_batch_panel_info are the twin's.
 *   lrbms3_reduced_implicit_euler_batch_tv   the same on the projected operators, one export for both right-hand sides: K = 0 takes
 *                                   rhs_red_K = rhs_red [S][N] and phi = NULL, 1 <= K <= 64 takes rhs_red_K [K][S][N] and phi
 *                                   [nmu][nt+1][K] (DEVICE); LRBMS_E_INVALID for a phi that does not go with K.  The groups' tables are
 *                                   refilled from row k+1 per step.  Work size lrbms3_reduced_implicit_euler_batch_work_size(N, nmu).
 *   lrbms3_reduced_parabolic_estimate_batch_tv  theta_t and coef [nmu][nt+1][2] (HOST, read before the call returns): the elliptic
 *                                   rows and the source terms of U[k] use row k, as does coef in eta[k] (alpha, gamma of row k); the
 *                                   time residual of U[k+1] - U[k] uses row k+1, the operator that produced U[k+1]; the nc form of
 *                                   the differences reads no theta.  The coef table goes to work in stream order in kernel-argument
 *                                   chunks of 256 doubles (no copy from pageable host memory, no host synchronisation); a table
 *                                   that is constant in time gives the bits of the twin.
 *                                   work: lrbms3_reduced_parabolic_estimate_batch_tv_work_size(N, nmu, nt) doubles (-1 outside the
 *                                   twin's limits or without a mesh).
 * The preconditioner of the two solvers: ONE per call, as in the twins, at the time mean of every column,
 *     theta_bar_m[q] = (sum_{k=1..nt} theta_t[m][k][q]) / nt   (ascending k),
 * then the twin's expression over the columns (reduced: sum_m theta_bar_m / nmu accumulated in column order; full order: the column sum
 * divided by nmu), times dt.  With nt = 1 that is the twin's arithmetic on row 1: a _tv call with nt = 1 gives the bits of its twin at
 * theta = row 1.  For d/dt A != 0 the estimate is an indicator, not a proven bound. */
int lrbms3_fom_implicit_euler_batch_tv(lrbms3_ctx* ctx, int32_t Q, int32_t K, int32_t nmu, const double* theta_t, double dt, int32_t nt,
                                       const double* A_diag, const double* A_cpl, const double* b_K, const double* phi, double* work,
                                       double* U, double rtol, int32_t max_iter, double* info, void* stream);
int lrbms3_reduced_implicit_euler_batch_tv(lrbms3_ctx* ctx, int32_t Q, int32_t N, int32_t K, int32_t nmu, const double* theta_t, double dt,
                                           int32_t nt, const double* B_sys, const double* M_red, const double* rhs_red_K,
                                           const double* phi, double* work, double* U, double rtol, int32_t max_iter, double* info,
                                           void* stream);
int64_t lrbms3_reduced_parabolic_estimate_batch_tv_work_size(lrbms3_ctx* ctx, int32_t N, int32_t nmu, int32_t nt);
int lrbms3_reduced_parabolic_estimate_batch_tv(lrbms3_ctx* ctx, int32_t Q, int32_t N, int32_t K, int32_t nmu, int32_t nt, double dt,
                                               const double* theta_t, const double* coef, const double* U, const double* B_sys,
                                               const double* M_red, const double* G_nc, const double* G_bb, const double* G_rdd,
                                               const double* G_ab, const double* G_aa, const double* r_fd, const double* Rb,
                                               const double* Yb, const double* Dp, const double* Xab, const double* As, const double* Cn,
                                               const double* ebar, const double* Bbb, const double* bdiv, const double* f2,
                                               const double* ceps, double hdiam, const double* phi, const double* F2,
                                               const double* r_fd_K, const double* bdiv_K, double* work, double* eta_loc,
                                               double* time_deriv_nc, double* time_residual, double* eta, double* est, void* stream);

/* -- online enrichment ------------------------------------------------------------------------------------------------------ */
/* Dirichlet correction blocks of the neighbourhood problems: on every coupling face of subdomain s, for the own side element,
 * the Dirichlet-face block (inside coefficient) minus the inner-face own / own block already contained in A_diag (mesh tables
 * TFb and TFo contracted with the lambda_q samples at the system face rule, as the diagonal block of lrbms3_assemble_system).
 *   D_corr [Q][S][6][ncf][100], zero on physical sides and on padded positions.  Once per discretization, not hot.
 * 2D: lrbms_assemble_dirichlet_correction. */
int lrbms3_assemble_dirichlet_correction(lrbms3_ctx* ctx, int32_t Q, const double* lam, double* D_corr, void* stream);

/* The corrector problems (reference block_swipdg.py:227-316) of nmark marked subdomains at once: SWIPDG on N(m) = m + face
 * neighbours (<= 7 subdomains, the slots of nbr[m]) with Dirichlet outer boundary, rhs = L2 functional of f, restricted to m.
 *   theta [Q] host, marked [nmark] host (in [0, S), no duplicates: LRBMS_E_INVALID otherwise), b [S][n], corr [nmark][n] out;
 *   work: lrbms3_local_correction_work_size(nmark) doubles -- everything lives there (no allocation in the call), its content on
 *   entry does not matter;  info (host, may be NULL) [nmark][2] = iterations, final relative residual.
 * A batched multi-kernel PCG (vectors [nmark][7][n], block-Jacobi from the uncorrected element blocks, scalars per problem on
 * the device, polled every 16 iterations); the matvec reads every combined block once per iteration for all problems that
 * contain its subdomain.  A problem is frozen at the first iteration at which its own residual meets rtol or p.Ap <= 0: its result
 * and its info row do not depend on what else is in the batch.  LRBMS_E_NOT_CONVERGED (message naming the subdomain) if a
 * problem is above rtol after max_iter or hit p.Ap <= 0 (cells of high aspect ratio can make a neighbourhood operator
 * indefinite).  Needs S_ext == S (LRBMS_E_INVALID).  2D: lrbms_local_correction_work_size / lrbms_local_correction_solve. */
int64_t lrbms3_local_correction_work_size(lrbms3_ctx* ctx, int32_t nmark);
int lrbms3_local_correction_solve(lrbms3_ctx* ctx, int32_t Q, const double* theta, int32_t nmark, const int32_t* marked,
                                  const double* A_diag, const double* A_cpl, const double* D_corr, const double* b, double* work,
                                  double* corr, double rtol, int32_t max_iter, double* info, void* stream);

/* The parabolic counterpart (2D: lrbms_local_correction_euler): the corrector TRAJECTORIES of nmark marked
 * subdomains, implicit Euler with zero initial value on the same neighbourhood problems,
 *   (M_N + dt A_N(theta)) x_{k+1} = M_N x_k + dt sum_j phi[k+1][j] b_j|_N,   k = 0 .. nt-1,   x_0 = 0,
 * M_N the element mass of lrbms3_fom_implicit_euler; x_k restricted to the marked subdomain is kept.
 *   theta [Q] host, marked [nmark] host, b_K [K][S][n], phi [nt + 1][K] device (row k = time of step k; row 0 is not read; K = 1,
 *   phi = 1: the plain load), work: lrbms3_local_correction_euler_work_size(nmark, nt) doubles, its content on entry does not
 *   matter; corr [nmark][n][nt] out, step fastest: column k - 1 = x_k.
 * The step operator, its element inverses and the host tables are built once per call; a step is the batched PCG of
 * lrbms3_local_correction_solve on it, warm-started at x_k, that stops per problem at |r| <= rtol |M x_k + dt sum_j phi b_j| or after
 * max_iter iterations of the step.  A step whose right-hand side is exactly zero, or whose first residual is within rtol, keeps
 * x_{k+1} = x_k at 0 iterations.  Fixed-order reductions and per-problem freezing: a trajectory and its info row do not depend on
 * what else is in the batch, on the order of marked, or on the content of work.
 *   info (host, may be NULL) [nmark][2] = iterations summed over the steps, worst final ratio of a step.
 * LRBMS_E_INVALID (before any launch): the refusals of lrbms3_local_correction_solve, K outside 1..64, nt < 1, dt <= 0, b_K or phi
 * NULL.  LRBMS_E_NOT_CONVERGED (message naming the first such subdomain and its step) if a step of a problem is above rtol after
 * max_iter or hit p.Ap <= 0: that trajectory ends there, the column of the step holds the iterate as it stands and the later
 * columns repeat it; the other problems run on, corr and info are filled. */
int64_t lrbms3_local_correction_euler_work_size(lrbms3_ctx* ctx, int32_t nmark, int32_t nt);
int lrbms3_local_correction_euler(lrbms3_ctx* ctx, int32_t Q, int32_t K, const double* theta, double dt, int32_t nt, int32_t nmark,
                                  const int32_t* marked, const double* A_diag, const double* A_cpl, const double* D_corr,
                                  const double* b_K, const double* phi, double* work, double* corr, double rtol, int32_t max_iter,
                                  double* info, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LRBMS3D_HIP_H */
