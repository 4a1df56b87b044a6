// clamp_forms.hip -- the two ways to write the row projection of the ADMM iteration, run against each other on the device.
//
//   min/max form   fminf(fmaxf(t, lo), hi)               every kernel but the MIXED horizon-10 ones (csrc/mpcqp_leg.h: leg_clip<false>)
//   median form    __builtin_amdgcn_fmed3f(t, lo, hi)    the MIXED horizon-10 kernels (leg_clip<true>): one v_med3_f32
//
// For finite t and lo <= hi the two are the same number.  Where they could part is decided here, by running both over every
// combination of the bound pairs the kernels use and the operands listed below, and printing each combination whose result WORDS
// differ (a zero of the other sign and another NaN payload count as differences).
//
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -o clamp_forms tools/clamp_forms.hip && ./clamp_forms
//
// Output: one line `DIFF <row kind> t=<hex> lo=<hex> hi=<hex> minmax=<hex> med3=<hex>` per differing combination, then
// `clamp_forms: <n> combinations, <d> differ`.  Exit status 0 unless the device could not be used.  tests/test_clamp_forms.py runs
// it and holds the DIFF lines against the set the source tolerates (none: every row kind uses the median).
//
// The bound pairs: the table BOUNDS below, one line per (lo, hi) expression pair that w_admm forms
//   A.lo0 = stance ? s.fmin : 0    A.hi0 = stance ? s.fmax : 0    A.loA = stance ? -BIG : 0    A.hiB = stance ? BIG : 0,   BIG = 1e30
//   row 0: (lo0, hi0)     rows 1, 3: (loA, 0)     rows 2, 4: (0, hiB)
// with s.fmin / s.fmax taken from BOX: the configuration's default box, boxes of model rows, a degenerate box (f_min = f_max), a zero
// lower bound of either sign.  The operands t: +-0, the smallest and the largest denormal, +-FLT_MIN, +-1, +-1e30, +-FLT_MAX, +-inf,
// a quiet NaN of either sign (t is the result of an fma and an add: a signalling NaN cannot occur), every bound value, and the
// neighbours of every bound value one spacing below and above.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

static constexpr float BIG = 1e30f;

struct Box { float fmin, fmax; };
static const Box BOX[] = {
    {3.0f, 100.0f},            // the default configuration
    {1.0f, 40.0f},   {5.0f, 150.0f},   {8.7f, 39.2f},   {12.0f, 25.0f},   // model rows
    {10.0f, 10.0f},            // f_min = f_max
    {0.0f, 100.0f},  {-0.0f, 100.0f},  {0.0f, 0.0f},
};

struct Bounds { const char* kind; const char* lo; const char* hi; };
// BEGIN BOUNDS (tests/test_clamp_forms.py reads these lines against w_admm)
static const Bounds BOUNDS[] = {
    {"row0_stance", "s.fmin", "s.fmax"},
    {"row0_swing", "0", "0"},
    {"rowA_stance", "-BIG", "0"},
    {"rowA_swing", "0", "0"},
    {"rowB_stance", "0", "BIG"},
    {"rowB_swing", "0", "0"},
};
// END BOUNDS

__global__ void clip_minmax(const float* __restrict__ t, const float* __restrict__ lo, const float* __restrict__ hi, float* __restrict__ z, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) z[i] = fminf(fmaxf(t[i], lo[i]), hi[i]);
}

__global__ void clip_med3(const float* __restrict__ t, const float* __restrict__ lo, const float* __restrict__ hi, float* __restrict__ z, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) z[i] = __builtin_amdgcn_fmed3f(t[i], lo[i], hi[i]);
}

static uint32_t word(float v) { uint32_t w; std::memcpy(&w, &v, 4); return w; }
static float from_word(uint32_t w) { float v; std::memcpy(&v, &w, 4); return v; }

#define HIP_OK(call) do { const hipError_t e_ = (call); if (e_ != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #call, hipGetErrorString(e_)); return 2; } } while (0)

int main() {
  std::vector<float> t, lo, hi;
  std::vector<int> kind;
  const int nkind = (int)(sizeof(BOUNDS) / sizeof(BOUNDS[0]));
  auto value = [](const char* e, const Box& b) {
    if (!std::strcmp(e, "s.fmin")) return b.fmin;
    if (!std::strcmp(e, "s.fmax")) return b.fmax;
    if (!std::strcmp(e, "-BIG")) return -BIG;
    if (!std::strcmp(e, "BIG")) return BIG;
    return 0.0f;
  };
  for (int k = 0; k < nkind; ++k) {
    const bool boxed = !std::strcmp(BOUNDS[k].lo, "s.fmin");
    for (const Box& b : BOX) {
      const float l = value(BOUNDS[k].lo, b), h = value(BOUNDS[k].hi, b);
      std::vector<float> ops = {0.0f, -0.0f, from_word(1u), -from_word(1u), from_word(0x007fffffu), -from_word(0x007fffffu), FLT_MIN, -FLT_MIN,
                                1.0f, -1.0f, BIG, -BIG, FLT_MAX, -FLT_MAX, INFINITY, -INFINITY, from_word(0x7fc00000u), from_word(0xffc00000u)};
      for (const float bound : {l, h}) {
        ops.push_back(bound);
        ops.push_back(-bound);
        ops.push_back(std::nextafterf(bound, -INFINITY));
        ops.push_back(std::nextafterf(bound, INFINITY));
      }
      for (const float v : ops) { t.push_back(v); lo.push_back(l); hi.push_back(h); kind.push_back(k); }
      if (!boxed) break;   // (the other row kinds do not depend on the box)
    }
  }
  const int n = (int)t.size();
  float *dt, *dlo, *dhi, *dz;
  HIP_OK(hipMalloc(&dt, n * sizeof(float)));
  HIP_OK(hipMalloc(&dlo, n * sizeof(float)));
  HIP_OK(hipMalloc(&dhi, n * sizeof(float)));
  HIP_OK(hipMalloc(&dz, 2 * n * sizeof(float)));
  HIP_OK(hipMemcpy(dt, t.data(), n * sizeof(float), hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(dlo, lo.data(), n * sizeof(float), hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(dhi, hi.data(), n * sizeof(float), hipMemcpyHostToDevice));
  const int nb = (n + 255) / 256;
  hipLaunchKernelGGL(clip_minmax, dim3(nb), dim3(256), 0, 0, dt, dlo, dhi, dz, n);
  hipLaunchKernelGGL(clip_med3, dim3(nb), dim3(256), 0, 0, dt, dlo, dhi, dz + n, n);
  HIP_OK(hipGetLastError());
  HIP_OK(hipDeviceSynchronize());
  std::vector<float> z(2 * n);
  HIP_OK(hipMemcpy(z.data(), dz, 2 * n * sizeof(float), hipMemcpyDeviceToHost));
  int differ = 0;
  for (int i = 0; i < n; ++i) {
    if (word(z[i]) != word(z[n + i])) {
      ++differ;
      std::printf("DIFF %s t=%08x lo=%08x hi=%08x minmax=%08x med3=%08x\n", BOUNDS[kind[i]].kind, word(t[i]), word(lo[i]), word(hi[i]), word(z[i]), word(z[n + i]));
    }
  }
  std::printf("clamp_forms: %d combinations, %d differ\n", n, differ);
  HIP_OK(hipFree(dt)); HIP_OK(hipFree(dlo)); HIP_OK(hipFree(dhi)); HIP_OK(hipFree(dz));
  return 0;
}
