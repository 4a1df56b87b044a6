// rs8_forms.hip -- the two forms of the mat-vec's reduce-scatter over the 8 lanes of a group, run against each other on the device.
//
//   select form   rs8 (csrc/mpcqp_leg.h): the first step picks what a lane keeps and what it sends with two selects per sum
//   banked form   rs8_banked: the first step as two DPP adds per sum under bank write masks (the MIXED horizon-10 kernels)
//
// The two add the same two operands, in the other order.  One wave -- lane 8 gr + gc, all eight grid rows, so both bank parities --
// runs both forms on each operand set below and the host prints every result word that differs (a zero of the other sign and
// another NaN payload count as differences).
//
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -o rs8_forms tools/rs8_forms.hip && ./rs8_forms
//
// Output: one line `DIFF <set> lane=<l> select=<hex> banked=<hex>` per differing word, then `rs8_forms: <n> words, <d> differ`.
// Exit status 0 unless the device could not be used.  tests/test_rs8_forms.py runs it, holds the DIFF lines against the empty set,
// and holds the two functions between the BEGIN / END marks against the text of csrc/mpcqp_leg.h.
//
// Operand sets (8 values per lane): random values of mixed magnitude and sign; zeros of either sign; denormals; random values
// with +-inf among them; and random values with one NaN in a single lane and element, at sixteen places that cover both banks,
// both row parities and every element.  (Every value reaches the forms as the result of a VALU multiply by one, as the kernels'
// operands are results of the tile product's last adds.)
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

template <int CTRL>
__device__ __forceinline__ float dpp_mov(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}

// BEGIN RS8 (tests/test_rs8_forms.py reads these lines against csrc/mpcqp_leg.h)
template <typename T>
__device__ __forceinline__ T rs8(const T (&v)[8], int gc) {
  const bool hi = (gc & 4) != 0, b1 = (gc & 2) != 0, b0 = (gc & 1) != 0;
  T t[4];
#pragma unroll
  for (int m = 0; m < 4; ++m) { const T keep = hi ? v[4 + m] : v[m], send = hi ? v[m] : v[4 + m]; t[m] = keep + dpp_mov<0x141>(send); }
  T s2[2];
#pragma unroll
  for (int m = 0; m < 2; ++m) { const T keep = b1 ? t[2 + m] : t[m], send = b1 ? t[m] : t[2 + m]; s2[m] = keep + dpp_mov<0x4E>(send); }
  const T keep = b0 ? s2[1] : s2[0], send = b0 ? s2[0] : s2[1];
  return keep + dpp_mov<0xB1>(send);
}
// END RS8
// BEGIN RS8_BANKED
__device__ __forceinline__ float rs8_banked(const float (&v)[8], int gc) {
  const bool b1 = (gc & 2) != 0, b0 = (gc & 1) != 0;
  float t[4];
  asm("s_nop 1\n\t"
      "v_add_f32_dpp %0, %4, %4 row_half_mirror row_mask:0xf bank_mask:0x5\n\t"
      "v_add_f32_dpp %1, %5, %5 row_half_mirror row_mask:0xf bank_mask:0x5\n\t"
      "v_add_f32_dpp %2, %6, %6 row_half_mirror row_mask:0xf bank_mask:0x5\n\t"
      "v_add_f32_dpp %3, %7, %7 row_half_mirror row_mask:0xf bank_mask:0x5\n\t"
      "v_add_f32_dpp %0, %8, %8 row_half_mirror row_mask:0xf bank_mask:0xa\n\t"
      "v_add_f32_dpp %1, %9, %9 row_half_mirror row_mask:0xf bank_mask:0xa\n\t"
      "v_add_f32_dpp %2, %10, %10 row_half_mirror row_mask:0xf bank_mask:0xa\n\t"
      "v_add_f32_dpp %3, %11, %11 row_half_mirror row_mask:0xf bank_mask:0xa"
      : "=&v"(t[0]), "=&v"(t[1]), "=&v"(t[2]), "=&v"(t[3])
      : "v"(v[0]), "v"(v[1]), "v"(v[2]), "v"(v[3]), "v"(v[4]), "v"(v[5]), "v"(v[6]), "v"(v[7]));
  float s2[2];
#pragma unroll
  for (int m = 0; m < 2; ++m) { const float keep = b1 ? t[2 + m] : t[m], send = b1 ? t[m] : t[2 + m]; s2[m] = keep + dpp_mov<0x4E>(send); }
  const float keep = b0 ? s2[1] : s2[0], send = b0 ? s2[0] : s2[1];
  return keep + dpp_mov<0xB1>(send);
}
// END RS8_BANKED

__global__ void run_forms(const float* __restrict__ in, const float* __restrict__ one, float* __restrict__ out, int nsets) {
  const int lane = threadIdx.x;
  const float o = one[0];
  for (int s = 0; s < nsets; ++s) {   // uniform: every lane of the wave is active in both forms
    float v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = in[(s * 64 + lane) * 8 + i] * o;
    out[(2 * s) * 64 + lane] = rs8<float>(v, lane & 7);
    out[(2 * s + 1) * 64 + lane] = rs8_banked(v, lane & 7);
  }
}

static uint32_t word(float v) { uint32_t w; std::memcpy(&w, &v, 4); return w; }
static float from_word(uint32_t w) { float v; std::memcpy(&v, &w, 4); return v; }

#define HIP_OK(call) do { const hipError_t e_ = (call); if (e_ != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #call, hipGetErrorString(e_)); return 2; } } while (0)

int main() {
  uint64_t state = 0x9E3779B97F4A7C15ull;
  auto rnd = [&]() { state = state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(state >> 32); };
  auto value = [&]() {   // a finite normal number, magnitude 2^-20 .. 2^20, either sign
    return from_word((rnd() & 0x80000000u) | ((107u + rnd() % 41u) << 23) | (rnd() & 0x007fffffu));
  };
  std::vector<std::string> names;
  std::vector<float> in;
  auto add_set = [&](const std::string& name, auto&& gen) {
    names.push_back(name);
    for (int l = 0; l < 64; ++l) for (int i = 0; i < 8; ++i) in.push_back(gen(l, i));
  };
  for (int k = 0; k < 4; ++k) add_set("random" + std::to_string(k), [&](int, int) { return value(); });
  add_set("zeros", [&](int, int) { return from_word(rnd() & 0x80000000u); });
  add_set("zeros_and_values", [&](int, int) { return (rnd() & 1u) ? from_word(rnd() & 0x80000000u) : value(); });
  add_set("denormals", [&](int, int) { return from_word((rnd() & 0x80000000u) | (1u + rnd() % 0x007fffffu)); });
  add_set("denormals_and_values", [&](int, int) { return (rnd() & 1u) ? from_word((rnd() & 0x80000000u) | (1u + rnd() % 0x007fffffu)) : value(); });
  add_set("inf_sparse", [&](int, int) { return rnd() % 16u == 0 ? ((rnd() & 1u) ? INFINITY : -INFINITY) : value(); });
  add_set("inf_dense", [&](int, int) { return rnd() % 2u == 0 ? ((rnd() & 1u) ? INFINITY : -INFINITY) : value(); });
  for (int k = 0; k < 16; ++k) {   // one NaN: lane 13 k + 5 (mod 64) reaches every group row parity and both halves of a group
    const int nl = (13 * k + 5) % 64, ni = k % 8;
    const uint32_t nan_word = (k & 1) ? 0xffc00000u : 0x7fc00000u;
    add_set("nan_l" + std::to_string(nl) + "_e" + std::to_string(ni), [&](int l, int i) { return l == nl && i == ni ? from_word(nan_word) : value(); });
  }
  const int nsets = (int)names.size();
  const float one = 1.0f;
  float *din, *done, *dout;
  HIP_OK(hipMalloc(&din, in.size() * sizeof(float)));
  HIP_OK(hipMalloc(&done, sizeof(float)));
  HIP_OK(hipMalloc(&dout, (size_t)nsets * 128 * sizeof(float)));
  HIP_OK(hipMemcpy(din, in.data(), in.size() * sizeof(float), hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(done, &one, sizeof(float), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(run_forms, dim3(1), dim3(64), 0, 0, din, done, dout, nsets);
  HIP_OK(hipGetLastError());
  HIP_OK(hipDeviceSynchronize());
  std::vector<float> out((size_t)nsets * 128);
  HIP_OK(hipMemcpy(out.data(), dout, out.size() * sizeof(float), hipMemcpyDeviceToHost));
  int differ = 0, nans = 0, infs = 0;
  for (int s = 0; s < nsets; ++s) {
    for (int l = 0; l < 64; ++l) {
      const float a = out[(2 * s) * 64 + l], b = out[(2 * s + 1) * 64 + l];
      nans += std::isnan(a); infs += std::isinf(a);
      if (word(a) != word(b)) {
        ++differ;
        std::printf("DIFF %s lane=%d select=%08x banked=%08x\n", names[s].c_str(), l, word(a), word(b));
      }
    }
  }
  std::printf("rs8_forms: %d words, %d differ (%d sets, %d NaN and %d inf results)\n", nsets * 64, differ, nsets, nans, infs);
  HIP_OK(hipFree(din)); HIP_OK(hipFree(done)); HIP_OK(hipFree(dout));
  return 0;
}
