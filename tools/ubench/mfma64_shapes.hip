// Microbenchmark (gfx950): the two f64 MFMA shapes, v_mfma_f64_16x16x4_f64 ("16": 2 048 flop) and v_mfma_f64_4x4x4_4b_f64 ("4": four
// independent 4 x 4 x 4 blocks, 512 flop, one double per lane for each of A, B and D).
//   part 1: the lane layout of the small shape, found with unit patterns: A = 1 on lane La only, B = 1 on lane Lb only, for all
//           64 x 64 pairs; the lane where D is nonzero (if any) says which A lane meets which B lane and where the product lands.
//   part 2: cycles per instruction of a stream of independent / dependent MFMAs of either shape and of a "4" placed between two "16",
//           with one wave per SIMD (waves 4-7 of a 512-thread workgroup, one workgroup per CU) and with two (waves 0-3 stream
//           another shape beside them: serial means both ~ sum, overlap means both ~ max).
//   part 3: an ACCUMULATING chain (non-zero running C, 128 k-steps) of the half-empty third row tile of k_f1w: rows 0-7 of one "16"
//           (output registers 0 and 1) against two chains of "4" (rows 0-3 and 4-7, A replicated over the four blocks), same random
//           operands, compared bit for bit; 256 independent trials.
// build: hipcc --offload-arch=gfx950 -O3 -o mfma64_shapes mfma64_shapes.hip        run: mfma64_shapes [blocks = 256] [accumulate]
//   (a second argument runs part 3 alone)
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

// part 3.  X[k][16] (columns 8-15 zero: the rows of the tile beyond N), Y[k][16], C[16][16]; lane = 16 lk + li.  The "16" takes
// A = X[kk + lk][li], B = Y[kk + lk][li] and returns row lk + 4 r of column li in register r; the "4" takes A = X[kk + lk][4 h + (li & 3)]
// (h = 0, 1), the same B, and returns row 4 h + lk of column li.
constexpr int ACC_KSTEPS = 128;
__global__ __launch_bounds__(64) void k_accumulate(double* out16, double* out4, const double* X, const double* Y, const double* C) {
  const int lane = threadIdx.x, li = lane & 15, lk = lane >> 4;
  X += (size_t)blockIdx.x * ACC_KSTEPS * 64, Y += (size_t)blockIdx.x * ACC_KSTEPS * 64, C += (size_t)blockIdx.x * 256;
  d4 acc;
  for (int r = 0; r < 4; ++r) acc[r] = C[(lk + 4 * r) * 16 + li];
  double t0 = acc[0], t1 = acc[1];
  for (int kk = 0; kk < 4 * ACC_KSTEPS; kk += 4) {
    const double bv = Y[(kk + lk) * 16 + li];
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(X[(kk + lk) * 16 + li], bv, acc, 0, 0, 0);
    t0 = __builtin_amdgcn_mfma_f64_4x4x4f64(X[(kk + lk) * 16 + (li & 3)], bv, t0, 0, 0, 0);
    t1 = __builtin_amdgcn_mfma_f64_4x4x4f64(X[(kk + lk) * 16 + 4 + (li & 3)], bv, t1, 0, 0, 0);
  }
  out16[blockIdx.x * 128 + 2 * lane] = acc[0], out16[blockIdx.x * 128 + 2 * lane + 1] = acc[1];
  out4[blockIdx.x * 128 + 2 * lane] = t0, out4[blockIdx.x * 128 + 2 * lane + 1] = t1;
}

static int accumulate_case() {
  const int trials = 256, nk = 4 * ACC_KSTEPS;
  const size_t nx = (size_t)trials * nk * 16, nc = (size_t)trials * 256, no = (size_t)trials * 128;
  double *X = (double*)malloc(8 * nx), *Y = (double*)malloc(8 * nx), *C = (double*)malloc(8 * nc);
  double *h16 = (double*)malloc(8 * no), *h4 = (double*)malloc(8 * no);
  unsigned long long st = 0x9E3779B97F4A7C15ull;
  auto rnd = [&]() {      // signed, magnitudes over eight binades: sums cancel and every rounding position occurs
    st = st * 6364136223846793005ull + 1442695040888963407ull;
    const double m = 1.0 + (double)((st >> 11) & ((1ull << 52) - 1)) / 4503599627370496.0;
    return ((st >> 63) ? -m : m) * ldexp(1.0, (int)((st >> 8) & 7) - 4);
  };
  for (size_t i = 0; i < nx; ++i) X[i] = i % 16 < 8 ? rnd() : 0.0, Y[i] = rnd();
  for (size_t i = 0; i < nc; ++i) C[i] = 16.0 * rnd();
  double *dX, *dY, *dC, *d16, *d4o;
  hipMalloc(&dX, 8 * nx), hipMalloc(&dY, 8 * nx), hipMalloc(&dC, 8 * nc), hipMalloc(&d16, 8 * no), hipMalloc(&d4o, 8 * no);
  hipMemcpy(dX, X, 8 * nx, hipMemcpyHostToDevice), hipMemcpy(dY, Y, 8 * nx, hipMemcpyHostToDevice), hipMemcpy(dC, C, 8 * nc, hipMemcpyHostToDevice);
  hipMemset(d16, 0xff, 8 * no), hipMemset(d4o, 0xff, 8 * no);
  hipLaunchKernelGGL(k_accumulate, dim3(trials), dim3(64), 0, 0, d16, d4o, dX, dY, dC);
  if (hipDeviceSynchronize() != hipSuccess) return printf("part 3: kernel failed\n"), 1;
  hipMemcpy(h16, d16, 8 * no, hipMemcpyDeviceToHost), hipMemcpy(h4, d4o, 8 * no, hipMemcpyDeviceToHost);
  size_t differ = 0;
  double worst16 = 0.0, worst4 = 0.0, worst_pair = 0.0;
  for (int t = 0; t < trials; ++t)
    for (int lane = 0; lane < 64; ++lane)
      for (int r = 0; r < 2; ++r) {
        const int row = (lane >> 4) + 4 * r, col = lane & 15;
        long double ref = C[(size_t)t * 256 + row * 16 + col], mag = fabsl(ref);
        for (int k = 0; k < nk; ++k) {
          const long double pr = (long double)X[((size_t)t * nk + k) * 16 + row] * Y[((size_t)t * nk + k) * 16 + col];
          ref += pr, mag += fabsl(pr);
        }
        const size_t o = (size_t)t * 128 + 2 * lane + r;
        unsigned long long b16, b4;
        memcpy(&b16, h16 + o, 8), memcpy(&b4, h4 + o, 8);
        differ += b16 != b4;
        worst16 = fmax(worst16, (double)(fabsl(h16[o] - ref) / mag)), worst4 = fmax(worst4, (double)(fabsl(h4[o] - ref) / mag));
        worst_pair = fmax(worst_pair, (double)(fabsl((long double)h16[o] - h4[o]) / mag));
      }
  printf("part 3: accumulating chains, %d trials x 128 outputs (rows 0-7 x 16 columns), %d k-steps each, running C non-zero from the start\n", trials,
         ACC_KSTEPS);
  printf("  16x16x4 registers 0, 1 against two 4x4x4_4b chains: %zu of %zu outputs differ bitwise -> %s\n", differ, no,
         differ == 0 ? "BIT-IDENTICAL" : "NOT bit-identical");
  printf("  largest |difference| / sum of |terms|: 16x16x4 against long double %.2e, 4x4x4 against long double %.2e, the two shapes %.2e\n", worst16,
         worst4, worst_pair);
  return 0;
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
  if (argc > 2) return accumulate_case();
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
  return accumulate_case();
}
