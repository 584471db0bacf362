// Local POD basis extension (pod.hip): launchers on lrbms_ctx_base, shared by the 2D and the 3D exports.  The local product is the
// path's own launcher behind a function pointer (2D: launch_blockell_apply on P_diag, 3D: k3_fom_apply without coupling blocks).
#pragma once
#include "lrbms_ctx_base.h"

// Y [S][n][M] = P X [S][n][M] on stream st; returns an LRBMS_* code
typedef int (*pod_product_fn)(void* self, int M, const double* X, double* Y, hipStream_t st);
struct PodProduct {
  pod_product_fn apply;
  void* self;
};

constexpr int POD_MAX_L = 128, POD_MAX_NW = 64;
constexpr double POD_MIN_RTOL = 1e-7;

// doubles of `work` for launch_local_pod (the formula of include/lrbms_hip.h)
int64_t pod_work_size(int S, int n, int L, int Nw);
// doubles of `work` for launch_pod_eigh
int64_t pod_eigh_work_size(int batch, int L);

int launch_local_pod(lrbms_ctx_base* ctx, int S, int n, int L, int Nw, int modes, double rtol, double atol, PodProduct P,
                     const double* U, double* V, int32_t* nloc, double* sv, int32_t* added, int32_t* info, double* work,
                     hipStream_t st);
// Streamed local POD (incremental HAPOD; the contract of lrbms_local_pod_stream_* in include/lrbms_hip.h, which also states the two
// size formulas).  rotate_valu != 0: step 5 of a push through k_pod_xt and a copy back instead of k_pod_stream_rotate.
int64_t pod_stream_state_size(int S, int n, int keep, int cmax);
int64_t pod_stream_work_size(int S, int n, int keep, int cmax, int Nw);
int launch_pod_stream_begin(lrbms_ctx_base* ctx, int S, int n, int keep, int cmax, double* state, hipStream_t st);
int launch_pod_stream_push(lrbms_ctx_base* ctx, int S, int n, int keep, int cmax, int C, int Nw, int rotate_valu, PodProduct P,
                           const double* U, const double* V, const int32_t* nloc, double* state, double* work, hipStream_t st);
int launch_pod_stream_finish(lrbms_ctx_base* ctx, int S, int n, int keep, int cmax, int Nw, int modes, double rtol, double atol,
                             PodProduct P, double* V, int32_t* nloc, double* state, double* sv, int32_t* added, int32_t* info,
                             double* lost, double* work, hipStream_t st);
// G[b] [L][L] = sym(X[b]^T Y[b]), X, Y [batch][K][L]: upper-triangle tiles on the fp64 MFMA, mirrored
int launch_pod_gram(lrbms_ctx_base* ctx, int batch, int K, int L, const double* X, const double* Y, double* G, hipStream_t st);
// cyclic Jacobi on G[b] [L][L].  mode 0: lam [batch][L] descending, Z [batch][L][L] with the eigenvector of lam[b][j] in ROW j;
// mode 1: Z = G^{-1/2} over the kcount[b] (nullptr: L) largest eigenpairs (Loewdin factor), lam as in mode 0.
// info [batch]: bit 0 the sweep cap was reached, bit 1 (mode 1) a retained eigenvalue was not positive.
int launch_pod_eigh(lrbms_ctx_base* ctx, int batch, int L, int mode, const double* G, const int32_t* kcount, double* lam, double* Z,
                    int32_t* info, double* work, hipStream_t st);
