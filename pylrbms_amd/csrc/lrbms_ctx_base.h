// Host-side plumbing shared by the 2D context (lrbms_ctx, lrbms_dev.h) and the 3D context (lrbms3_ctx, lrbms3d_dev.h): the error
// string and the check macros, per-kernel event timing, template uploads and the library-owned side streams.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>

#include "../../include/lrbms_hip.h"

// Library-owned side streams, one set per device, shared by every context of the process (2D and 3D alike).  HIP maps streams
// round-robin onto a few hardware queues (4 by default); a second context with side streams of its own lands on queues the
// first one (or the caller's stream) already uses and its "concurrent" chains then run one after another -- measured: the
// config-5 pass 2.49 ms instead of 2.20 ms when a 2D context with three streams of its own was alive in the process.
// Reference-counted; the stream is destroyed with its last user.  Thread-safe.
hipStream_t lrbms_side_stream_acquire(int device, int i);   // i in [0, 3); nullptr on failure
void lrbms_side_stream_release(int device, int i);

// What both context types hold first; lrbms_ctx and lrbms3_ctx derive from it, the helpers below take either.
struct lrbms_ctx_base {
  int device = 0;
  bool has_mesh = false;
  std::vector<void*> owned;       // device allocations to free
  hipStream_t aux[3] = {nullptr, nullptr, nullptr};   // library-owned side streams: independent kernels run concurrently
  hipEvent_t ev_fork = nullptr, ev_join[3] = {nullptr, nullptr, nullptr};
  // per-kernel device timing (lrbms_kernel_timing / lrbms3_kernel_timing): HIP event pairs on the stream each kernel runs on
  bool ktime = false;
  struct KTimer { const char* name; hipEvent_t e0, e1; bool used; };
  std::vector<KTimer> ktimers;
  int ktime_n = 0;
  int opt_pod_rotate_valu = 0;    // LRBMS_OPT_POD_ROTATE_VALU / LRBMS3_OPT_POD_ROTATE_VALU
  std::string err;
};

// The fork event, the three side streams and their join events (LRBMS_E_HIP on failure; lrbms_ctx_base_release gives back
// what was acquired), and their release together with the timing events.
int lrbms_ctx_base_init(lrbms_ctx_base* ctx, int device);
void lrbms_ctx_base_release(lrbms_ctx_base* ctx);

// Bodies of lrbms[3]_kernel_timing and lrbms[3]_kernel_timing_read: names joined by '\n', no trailing separator.
int lrbms_ctx_kernel_timing(lrbms_ctx_base* ctx, int32_t enable);
int lrbms_ctx_kernel_timing_read(lrbms_ctx_base* ctx, char* names, int64_t names_cap, double* ms, int32_t cap, int32_t* count);

static inline int lrbms_fail(lrbms_ctx_base* ctx, int code, const std::string& msg) {
  if (ctx) ctx->err = msg;
  return code;
}

#define LRBMS_HIP_CHECK(ctx, expr)                                                                  \
  do {                                                                                              \
    hipError_t _e = (expr);                                                                         \
    if (_e != hipSuccess)                                                                           \
      return lrbms_fail(ctx, LRBMS_E_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));       \
  } while (0)

#define LRBMS_REQUIRE_MESH(ctx)                                                      \
  do {                                                                               \
    if (!(ctx)) return LRBMS_E_INVALID;                                              \
    if (!(ctx)->has_mesh) return lrbms_fail(ctx, LRBMS_E_STATE, "mesh not uploaded"); \
  } while (0)

#define LRBMS_LAUNCH_CHECK(ctx) LRBMS_HIP_CHECK(ctx, hipGetLastError())

// RAII scope around one kernel launch: when timing is enabled (lrbms_kernel_timing) records an event pair on the
// kernel's own stream; otherwise costs one branch.
struct KScope {
  lrbms_ctx_base* ctx;
  hipStream_t st;
  int idx;
  KScope(lrbms_ctx_base* c, const char* name, hipStream_t s) : ctx(c), st(s), idx(-1) {
    if (!c->ktime) return;
    if (c->ktime_n == (int)c->ktimers.size()) {
      lrbms_ctx_base::KTimer k{name, nullptr, nullptr, false};
      if (hipEventCreate(&k.e0) != hipSuccess || hipEventCreate(&k.e1) != hipSuccess) return;
      c->ktimers.push_back(k);
    }
    idx = c->ktime_n++;
    c->ktimers[idx].name = name;
    c->ktimers[idx].used = true;
    (void)hipEventRecord(c->ktimers[idx].e0, st);
  }
  ~KScope() {
    if (idx >= 0) (void)hipEventRecord(ctx->ktimers[idx].e1, st);
  }
};

// RAII fork of ng <= 4 independent chains onto the caller's stream and the library's side streams (the batched reduced solvers,
// 2D and 3D: one group of parameters per stream).  fork() makes the side streams wait for what the caller's stream holds, join()
// makes the caller's stream wait for them.  Every EARLY return between the two (a failed HIP call) leaves through the destructor:
// the group streams are drained -- their asynchronous copies target host memory of the frames that are being left -- and joined
// into the caller's stream, which the fused pass and the next call share with them.
struct StreamFork {
  lrbms_ctx_base* ctx;
  hipStream_t st = nullptr;
  int ng = 0;
  bool armed = false;
  explicit StreamFork(lrbms_ctx_base* c) : ctx(c) {}
  StreamFork(const StreamFork&) = delete;
  StreamFork& operator=(const StreamFork&) = delete;
  hipStream_t stream(int k) const { return k == 0 ? st : ctx->aux[k - 1]; }
  int fork(hipStream_t s, int n) {
    st = s;
    ng = n;
    armed = true;
    if (ng > 1) {
      LRBMS_HIP_CHECK(ctx, hipEventRecord(ctx->ev_fork, st));
      for (int k = 1; k < ng; ++k) LRBMS_HIP_CHECK(ctx, hipStreamWaitEvent(stream(k), ctx->ev_fork, 0));
    }
    return LRBMS_OK;
  }
  int join() {
    for (int k = 1; k < ng; ++k) {
      LRBMS_HIP_CHECK(ctx, hipEventRecord(ctx->ev_join[k - 1], stream(k)));
      LRBMS_HIP_CHECK(ctx, hipStreamWaitEvent(st, ctx->ev_join[k - 1], 0));
    }
    armed = false;
    return LRBMS_OK;
  }
  ~StreamFork() {
    if (!armed) return;
    for (int k = 0; k < ng; ++k) (void)hipStreamSynchronize(stream(k));
    for (int k = 1; k < ng; ++k) {
      (void)hipEventRecord(ctx->ev_join[k - 1], stream(k));
      (void)hipStreamWaitEvent(st, ctx->ev_join[k - 1], 0);
    }
  }
};

// A ctx-owned device copy of count (at least one) elements of host; with host == nullptr the allocation is left uninitialised.
template <typename T>
int upload(lrbms_ctx_base* ctx, const T* host, long count, const T** dev) {
  void* p = nullptr;
  LRBMS_HIP_CHECK(ctx, hipMalloc(&p, sizeof(T) * (count > 0 ? count : 1)));
  ctx->owned.push_back(p);
  if (host && count > 0) LRBMS_HIP_CHECK(ctx, hipMemcpy(p, host, sizeof(T) * count, hipMemcpyHostToDevice));
  *dev = static_cast<const T*>(p);
  return LRBMS_OK;
}
