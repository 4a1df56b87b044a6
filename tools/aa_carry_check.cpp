// aa_carry_check.cpp -- host replay of the Anderson step (csrc/mpcqp_leg.h: w_aa_step): the form that sums all nine numbers of the
// least-squares system in every call against the form that carries the Gram entries of the surviving columns from call to call.
// Both run on the same random fp32 histories, with the workgroup sum emulated in the pairing order of wave_sum / block_sum
// (csrc/mpcqp_device.h), and must agree BITWISE in gamma, `ok`, `have_prev`, the returned base point and the filed history.
//
//   c++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all tools/aa_carry_check.cpp -o aa_carry_check
//   ./aa_carry_check            (add -DAA_M=2 for the two-column variant)
//
// 1 000 sequences of 40 calls, one wave (64 lanes) and four waves (256 lanes) alternating; degenerate systems are forced (an image
// equal to its base point, a repeated column, an overflowing entry) so that histories restart.  Exit status 0 = identical.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#ifndef AA_M
#define AA_M 3
#endif
constexpr int M = AA_M, NG = M * (M + 1) / 2, NQ = NG + M, NC = M * (M - 1) / 2;
static_assert(M == 2 || M == 3, "two or three columns");
constexpr int gram_at(int i, int j) { return i * M - i * (i - 1) / 2 + (j - i); }

struct Lane { float rp[5], dX[M][5], dF[M][5], xb[5], fp[5]; };
struct Group {
  std::vector<Lane> lane;
  float gc[NC];          // carried form only
  bool have_prev = false;
  explicit Group(int n) : lane(n) { reset(); for (auto& l : lane) for (int k = 0; k < 5; ++k) l.xb[k] = l.fp[k] = 0.f; }
  void reset() {
    for (auto& l : lane) { std::memset(l.rp, 0, sizeof l.rp); std::memset(l.dX, 0, sizeof l.dX); std::memset(l.dF, 0, sizeof l.dF); }
    for (float& c : gc) c = 0.f;
  }
};

// wave_sum: butterfly inside each row of 16 (xor 1, xor 2, half-row mirror, row mirror), rows folded into row 3, lane 63 read.
static float wave_sum(const float* in) {
  float v[64], t[64];
  std::memcpy(v, in, sizeof v);
  auto stage = [&](auto src) { for (int i = 0; i < 64; ++i) { const int s = src(i); t[i] = s < 0 ? v[i] + 0.f : v[i] + v[s]; } std::memcpy(v, t, sizeof v); };
  stage([](int i) { return i ^ 1; });
  stage([](int i) { return i ^ 2; });
  stage([](int i) { return (i & ~7) | (7 - (i & 7)); });
  stage([](int i) { return (i & ~15) | (15 - (i & 15)); });
  stage([](int i) { return ((i >> 4) & 1) ? (i & ~15) - 1 : -1; });   // row_bcast15 into rows 1, 3 (other rows add zero)
  stage([](int i) { return (i >> 5) ? 31 : -1; });                    // row_bcast31 into rows 2, 3
  return v[63];
}
// block_sum: the waves' sums added in wave order.
static float group_sum(const std::vector<float>& per_lane) {
  const int nw = (int)per_lane.size() / 64;
  float m = wave_sum(per_lane.data());
  for (int w = 1; w < nw; ++w) m += wave_sum(per_lane.data() + 64 * w);
  return m;
}

struct StepOut { float g[M]; bool ok, solved; };

// The regularised normal equations by L D L', as w_aa_step solves them (1 / x stands in for v_rcp_f32 in both forms).
template <int MM>
static void aa_solve(const float* q, StepOut& o, bool& have) {
  if constexpr (MM == 3) {
    const float tr = q[0] + q[3] + q[5];
    have = tr > 0.f;
    const float reg = fmaf(1e-6f, tr, 1e-30f);
    const float a00 = q[0] + reg, a11 = q[3] + reg, a22 = q[5] + reg, a01 = q[1], a02 = q[2], a12 = q[4];
    const float i0 = 1.f / a00, l10 = a01 * i0, l20 = a02 * i0;
    const float d1 = fmaf(-l10, a01, a11), i1 = 1.f / d1, t21 = fmaf(-l20, a01, a12), l21 = t21 * i1;
    const float d2 = fmaf(-l21, t21, fmaf(-l20, a02, a22)), i2 = 1.f / d2;
    const float y0 = q[6], y1 = fmaf(-l10, y0, q[7]), y2 = fmaf(-l21, y1, fmaf(-l20, y0, q[8]));
    o.g[2] = y2 * i2; o.g[1] = fmaf(-l21, o.g[2], y1 * i1); o.g[0] = fmaf(-l20, o.g[2], fmaf(-l10, o.g[1], y0 * i0));
    o.ok = have && d1 > 0.f && d2 > 0.f && fabsf(o.g[0]) + fabsf(o.g[1]) + fabsf(o.g[2]) <= 1e4f;
  } else {
    const float tr = q[0] + q[2];
    have = tr > 0.f;
    const float reg = fmaf(1e-6f, tr, 1e-30f);
    const float a00 = q[0] + reg, a11 = q[2] + reg, a01 = q[1];
    const float i0 = 1.f / a00, l10 = a01 * i0, d1 = fmaf(-l10, a01, a11), i1 = 1.f / d1;
    const float y0 = q[3], y1 = fmaf(-l10, y0, q[4]);
    o.g[1] = y1 * i1; o.g[0] = fmaf(-l10, o.g[1], y0 * i0);
    o.ok = have && d1 > 0.f && fabsf(o.g[0]) + fabsf(o.g[1]) <= 1e4f;
  }
}

// One call, for every lane of the group.  `carry`: the form under test.  fx[lane][5]: the new image.
static StepOut aa_step(Group& G, const std::vector<float>& fx, bool carry) {
  StepOut o{};
  const int n = (int)G.lane.size();
  if (!G.have_prev) {
    for (int l = 0; l < n; ++l) for (int k = 0; k < 5; ++k) { Lane& L = G.lane[l]; L.rp[k] = fx[5 * l + k] - L.xb[k]; L.fp[k] = L.xb[k] = fx[5 * l + k]; }
    G.have_prev = true;
    return o;
  }
  std::vector<float> r(5 * n);
  for (int l = 0; l < n; ++l) {
    Lane& L = G.lane[l];
    for (int k = 0; k < 5; ++k) {
      r[5 * l + k] = fx[5 * l + k] - L.xb[k];
      const float dx = fx[5 * l + k] - L.fp[k], df = r[5 * l + k] - L.rp[k];
      for (int j = 0; j + 1 < M; ++j) { L.dX[j][k] = L.dX[j + 1][k]; L.dF[j][k] = L.dF[j + 1][k]; }
      L.dX[M - 1][k] = dx; L.dF[M - 1][k] = df;
      L.fp[k] = fx[5 * l + k]; L.rp[k] = r[5 * l + k];
    }
  }
  auto dot = [&](int i, int j) {   // j == M: the right-hand side
    std::vector<float> part(n);
    for (int l = 0; l < n; ++l) {
      float a = 0.f;
      for (int k = 0; k < 5; ++k) a = fmaf(G.lane[l].dF[i][k], j == M ? r[5 * l + k] : G.lane[l].dF[j][k], a);
      part[l] = a;
    }
    return group_sum(part);
  };
  float q[NQ];
  {
    int ac = 0;
    for (int i = 0; i < M; ++i) {
      for (int j = i; j < M; ++j) q[gram_at(i, j)] = (carry && j < M - 1) ? G.gc[ac++] : dot(i, j);
      q[NG + i] = dot(i, M);
    }
    ac = 0;
    for (int i = 0; i + 1 < M; ++i) for (int j = i; j + 1 < M; ++j) G.gc[ac++] = q[gram_at(i + 1, j + 1)];
  }
  o.solved = true;
  bool have;
  aa_solve<M>(q, o, have);
  if (have && !o.ok) { G.reset(); G.have_prev = false; }
  for (int l = 0; l < n; ++l) {
    Lane& L = G.lane[l];
    for (int k = 0; k < 5; ++k) {
      float c = 0.f;
      for (int j = 0; j < M; ++j) c = fmaf(o.g[j], L.dX[j][k], c);
      L.xb[k] = o.ok ? fx[5 * l + k] - c : fx[5 * l + k];
    }
  }
  return o;
}

static bool same_bits(const void* a, const void* b, size_t n) { return std::memcmp(a, b, n) == 0; }

int main() {
  std::mt19937 rng(20251018);
  std::normal_distribution<float> nrm(0.f, 1.f);
  std::uniform_int_distribution<int> pick(0, 99);
  long calls = 0, resets = 0, extrap = 0, empty = 0;
  for (int seq = 0; seq < 1000; ++seq) {
    const int n = (seq & 1) ? 256 : 64, legs = (seq & 1) ? 80 * 3 : 40;   // lanes beyond `legs` hold zeros, as in the kernels
    Group A(n), B(n);
    for (int l = 0; l < legs; ++l) for (int k = 0; k < 5; ++k) A.lane[l].xb[k] = A.lane[l].fp[k] = B.lane[l].xb[k] = B.lane[l].fp[k] = nrm(rng);
    std::vector<float> fx(5 * n, 0.f), fixed(5 * n, 0.f), dir(5 * n, 0.f);
    for (int l = 0; l < 5 * legs; ++l) { fixed[l] = nrm(rng); dir[l] = nrm(rng); }
    const float rate = 0.5f + 0.0045f * (float)pick(rng);   // contraction factor 0.5 .. 0.95
    for (int call = 0; call < 40; ++call) {
      const int kind = pick(rng);
      for (int l = 0; l < 5 * legs; ++l) {
        const float xb = A.lane[l / 5].xb[l % 5];
        if (kind < 4) fx[l] = xb;                                   // image = base point: zero residual, a zero or repeated column
        else if (kind < 8) fx[l] = xb + 1e-3f * dir[l];             // the same step again: dependent columns
        else if (kind < 10) fx[l] = (l == 7) ? 3e30f : xb;          // an entry whose square overflows: NaN in the system
        else fx[l] = fixed[l] + rate * (xb - fixed[l]) + 1e-4f * nrm(rng);   // a noisy contraction
      }
      const bool hadA = A.have_prev;
      const StepOut a = aa_step(A, fx, false), b = aa_step(B, fx, true);
      ++calls;
      if (!a.solved) ++empty; else if (a.ok) ++extrap; else if (hadA && !A.have_prev) ++resets;
      bool same = a.ok == b.ok && a.solved == b.solved && A.have_prev == B.have_prev && same_bits(a.g, b.g, sizeof a.g)
                  && same_bits(A.lane.data(), B.lane.data(), n * sizeof(Lane));
      if (!same) {
        std::printf("MISMATCH sequence %d call %d (%d lanes): ok %d/%d have_prev %d/%d gamma", seq, call, n, a.ok, b.ok, A.have_prev, B.have_prev);
        for (int j = 0; j < M; ++j) std::printf(" %a/%a", a.g[j], b.g[j]);
        std::printf("\n");
        return 1;
      }
    }
  }
  std::printf("AA_M = %d: %ld calls bitwise identical (%ld extrapolations, %ld restarts, %ld first images)\n", M, calls, extrap, resets, empty);
  if (resets < 100 || extrap < 10000) { std::printf("the sequences do not exercise restarts / extrapolations enough\n"); return 2; }
  return 0;
}
