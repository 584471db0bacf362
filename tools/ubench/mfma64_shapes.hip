// Microbenchmark (gfx950): the two f64 MFMA shapes, v_mfma_f64_16x16x4_f64 ("16": 2 048 flop) and v_mfma_f64_4x4x4_4b_f64 ("4": four
// independent 4 x 4 x 4 blocks, 512 flop, one double per lane for each of A, B and D).
//   part 1: the lane layout of the small shape, found with unit patterns: A = 1 on lane La only, B = 1 on lane Lb only, for all
//           64 x 64 pairs; the lane where D is nonzero (if any) says which A lane meets which B lane and where the product lands.
//   part 2: cycles per instruction of a stream of independent / dependent MFMAs of either shape and of a "4" placed between two "16",
//           with one wave per SIMD (waves 4-7 of a 512-thread workgroup, one workgroup per CU) and with two (waves 0-3 stream
//           another shape beside them: serial means both ~ sum, overlap means both ~ max).
// build: hipcc --offload-arch=gfx950 -O3 -o mfma64_shapes mfma64_shapes.hip        run: mfma64_shapes [blocks = 256]
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
typedef double d4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(64) void k_layout(unsigned long long* out) {
  const int lane = threadIdx.x;
  for (int la = 0; la < 64; ++la)
    for (int lb = 0; lb < 64; ++lb) {
      const double d = __builtin_amdgcn_mfma_f64_4x4x4f64(lane == la ? 1.0 : 0.0, lane == lb ? 1.0 : 0.0, 0.0, 0, 0, 0);
      const unsigned long long m = __ballot(d != 0.0);
      if (lane == 0) out[la * 64 + lb] = m;
    }
}

// a numeric check of the map that part 1 prints: D[b][i][j] = sum_k A[b][i][k] B[b][k][j] with the lanes of the hypothesis
__global__ __launch_bounds__(64) void k_value(double* out, const double* A, const double* B) {
  const int lane = threadIdx.x;
  out[lane] = __builtin_amdgcn_mfma_f64_4x4x4f64(A[lane], B[lane], 0.0, 0, 0, 0);
}

enum { NONE = 0, IND16 = 1, DEP16 = 2, IND4 = 3, DEP4 = 4, MIX = 5 };
constexpr int NI = 60;      // instructions of one shape per iteration (MIX: NI of each shape, alternating)

template <int MODE>
__device__ __forceinline__ double stream(int iters, double av, double bv) {
  double res = 0.0;
  if (MODE == IND16) {
    d4 acc[20];
#pragma unroll
    for (int i = 0; i < 20; ++i) acc[i] = (d4){0, 0, 0, 0};
    for (int it = 0; it < iters; ++it)
#pragma unroll
      for (int r = 0; r < NI; ++r) acc[r % 20] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc[r % 20], 0, 0, 0);
    for (int i = 0; i < 20; ++i) res += acc[i][0] + acc[i][3];
  } else if (MODE == DEP16) {
    d4 acc = (d4){0, 0, 0, 0};
    for (int it = 0; it < iters; ++it)
#pragma unroll
      for (int r = 0; r < NI; ++r) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
    res = acc[0] + acc[3];
  } else if (MODE == IND4) {
    double acc[20];
#pragma unroll
    for (int i = 0; i < 20; ++i) acc[i] = 0.0;
    for (int it = 0; it < iters; ++it)
#pragma unroll
      for (int r = 0; r < NI; ++r) acc[r % 20] = __builtin_amdgcn_mfma_f64_4x4x4f64(av, bv, acc[r % 20], 0, 0, 0);
    for (int i = 0; i < 20; ++i) res += acc[i];
  } else if (MODE == DEP4) {
    double acc = 0.0;
    for (int it = 0; it < iters; ++it)
#pragma unroll
      for (int r = 0; r < NI; ++r) acc = __builtin_amdgcn_mfma_f64_4x4x4f64(av, bv, acc, 0, 0, 0);
    res = acc;
  } else if (MODE == MIX) {
    d4 acc[12];
    double sm[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) acc[i] = (d4){0, 0, 0, 0}, sm[i] = 0.0;
    for (int it = 0; it < iters; ++it)
#pragma unroll
      for (int r = 0; r < NI; ++r) {
        acc[r % 12] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc[r % 12], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        sm[r % 12] = __builtin_amdgcn_mfma_f64_4x4x4f64(av, bv, sm[r % 12], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
    for (int i = 0; i < 12; ++i) res += acc[i][0] + acc[i][3] + sm[i];
  }
  return res;
}

// waves 4-7 ("M") run MM, waves 0-3 ("P") run PM; ticks[block * 8 + wave]: the wave's own cycle count of its stream
template <int PM, int MM>
__global__ __launch_bounds__(512) void k(double* out, long long* ticks, int iters, double a, double b) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const double av = a + lane, bv = b;
  const long long t0 = __builtin_readcyclecounter();
  const double res = wave >= 4 ? stream<MM>(iters, av, bv) : stream<PM>(iters, av, bv);
  const long long t1 = __builtin_readcyclecounter();
  out[(size_t)blockIdx.x * 512 + threadIdx.x] = res;
  if (lane == 0) ticks[blockIdx.x * 8 + wave] = t1 - t0;
}

struct Res {
  float ms;
  double tick_p, tick_m;      // mean ticks of the P / M waves
};

template <typename K>
Res run(K kern, int blocks, double* out, long long* ticks, int iters) {
  hipLaunchKernelGGL(kern, dim3(blocks), dim3(512), 0, 0, out, ticks, iters, 1.0000001, 1e-9);
  hipDeviceSynchronize();
  hipEvent_t e0, e1;
  hipEventCreate(&e0);
  hipEventCreate(&e1);
  hipEventRecord(e0);
  for (int r = 0; r < 3; ++r) hipLaunchKernelGGL(kern, dim3(blocks), dim3(512), 0, 0, out, ticks, iters, 1.0000001, 1e-9);
  hipEventRecord(e1);
  hipEventSynchronize(e1);
  Res x;
  hipEventElapsedTime(&x.ms, e0, e1);
  x.ms /= 3;
  hipEventDestroy(e0);
  hipEventDestroy(e1);
  long long* h = (long long*)malloc(sizeof(long long) * 8 * blocks);
  hipMemcpy(h, ticks, sizeof(long long) * 8 * blocks, hipMemcpyDeviceToHost);
  x.tick_p = x.tick_m = 0.0;
  for (int i = 0; i < 8 * blocks; ++i) (i % 8 < 4 ? x.tick_p : x.tick_m) += (double)h[i] / (4.0 * blocks);
  free(h);
  return x;
}

static const char* NAMES[] = {"-", "16 independent", "16 dependent", "4 independent", "4 dependent", "16,4 alternating"};

template <int PM, int MM>
Res report(int blocks, double* out, long long* ticks, int iters) {
  const Res x = run(k<PM, MM>, blocks, out, ticks, iters);
  const double n = (double)iters * NI;       // instructions per shape and wave
  printf("P %-17s M %-17s | %8.3f ms = %7.1f cycles at 2.4 GHz per M step | wave ticks per step: P %7.1f  M %7.1f\n", NAMES[PM], NAMES[MM],
         x.ms, x.ms * 1e-3 * 2.4e9 / n, x.tick_p / n, x.tick_m / n);
  return x;
}

int main(int argc, char** argv) {
  const int blocks = argc > 1 ? atoi(argv[1]) : 256;
  const int iters = 400;
  double *out, *dA, *dB;
  long long* ticks;
  unsigned long long* map;
  hipMalloc(&out, sizeof(double) * 512 * blocks);
  hipMalloc(&dA, sizeof(double) * 64);
  hipMalloc(&dB, sizeof(double) * 64);
  hipMalloc(&ticks, sizeof(long long) * 8 * blocks);
  hipMalloc(&map, sizeof(unsigned long long) * 4096);

  // ---- part 1
  hipLaunchKernelGGL(k_layout, dim3(1), dim3(64), 0, 0, map);
  static unsigned long long h[4096];
  hipMemcpy(h, map, sizeof(h), hipMemcpyDeviceToHost);
  printf("part 1: v_mfma_f64_4x4x4_4b_f64, unit patterns. A lane La: the B lanes it meets -> the lane of D that receives the product\n");
  int pairs = 0, multi = 0, bad = 0;
  for (int la = 0; la < 64; ++la) {
    printf("  A lane %2d:", la);
    for (int lb = 0; lb < 64; ++lb) {
      const unsigned long long m = h[la * 64 + lb];
      if (m == 0) continue;
      ++pairs;
      if (m & (m - 1)) ++multi;
      const int ld = __builtin_ctzll(m);
      printf("  B %2d -> D %2d", lb, ld);
      // hypothesis: lane = 16 k + 4 block + i for A[block][i][k], 16 k + 4 block + j for B[block][k][j], 16 i + 4 block + j for D[block][i][j]
      const int ka = la >> 4, ba = (la >> 2) & 3, i = la & 3, kb = lb >> 4, bb = (lb >> 2) & 3, j = lb & 3;
      if (ka != kb || ba != bb || ld != 16 * i + 4 * ba + j) ++bad;
    }
    printf("\n");
  }
  printf("  %d (La, Lb) pairs meet (expected 4 blocks x 4 i x 4 j x 4 k = 256), %d of them in more than one D lane\n", pairs, multi);
  printf("  hypothesis  A[b][i][k]: lane 16 k + 4 b + i   B[b][k][j]: lane 16 k + 4 b + j   D[b][i][j]: lane 16 i + 4 b + j  -> %s\n",
         pairs == 256 && multi == 0 && bad == 0 ? "HOLDS for every pair" : "DOES NOT HOLD");
  {
    double A[64], B[64], D[64], worst = 0.0;
    for (int l = 0; l < 64; ++l) A[l] = 1.0 + 0.37 * l + 0.01 * l * l, B[l] = 2.0 - 0.11 * l + 0.003 * l * l;
    hipMemcpy(dA, A, sizeof(A), hipMemcpyHostToDevice);
    hipMemcpy(dB, B, sizeof(B), hipMemcpyHostToDevice);
    hipLaunchKernelGGL(k_value, dim3(1), dim3(64), 0, 0, out, dA, dB);
    hipMemcpy(D, out, sizeof(D), hipMemcpyDeviceToHost);
    for (int b = 0; b < 4; ++b)
      for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
          double ref = 0.0;
          for (int kk = 0; kk < 4; ++kk) ref += A[16 * kk + 4 * b + i] * B[16 * kk + 4 * b + j];
          const double err = fabs(D[16 * i + 4 * b + j] - ref) / fabs(ref);
          worst = err > worst ? err : worst;
        }
    printf("  numeric check of the hypothesis with general A, B: largest relative difference %.2e\n", worst);
  }

  // ---- part 2
  printf("part 2: %d blocks of 512 threads, %d x %d instructions per shape and wave; a step is one instruction (16,4 alternating: one pair)\n",
         blocks, iters, NI);
  printf("one wave per SIMD:\n");
  const Res i16 = report<NONE, IND16>(blocks, out, ticks, iters);
  const Res d16 = report<NONE, DEP16>(blocks, out, ticks, iters);
  const Res i4 = report<NONE, IND4>(blocks, out, ticks, iters);
  const Res d4r = report<NONE, DEP4>(blocks, out, ticks, iters);
  const Res mix = report<NONE, MIX>(blocks, out, ticks, iters);
  printf("two waves per SIMD:\n");
  report<IND16, IND16>(blocks, out, ticks, iters);
  report<IND4, IND4>(blocks, out, ticks, iters);
  report<IND4, IND16>(blocks, out, ticks, iters);
  report<DEP4, IND16>(blocks, out, ticks, iters);
  report<IND16, DEP4>(blocks, out, ticks, iters);
  report<MIX, MIX>(blocks, out, ticks, iters);
  const double n = (double)iters * NI;
  const double t16 = i16.tick_m / n, t4 = i4.tick_m / n, t4d = d4r.tick_m / n, t4mix = mix.tick_m / n - t16;
  printf("summary (wave ticks): t16 independent %.1f dependent %.1f | t4 independent %.1f dependent %.1f | a 4 between two 16: %.1f\n", t16,
         d16.tick_m / n, t4, t4d, t4mix);
  printf("gate (>= 140 ticks per chunk): 6 (t16 - t4) = %.0f, 6 t16 - 5 t4 = %.0f with t4 independent; %.0f and %.0f with t4 between two 16\n",
         6 * (t16 - t4), 6 * t16 - 5 * t4, 6 * (t16 - t4mix), 6 * t16 - 5 * t4mix);
  return 0;
}
