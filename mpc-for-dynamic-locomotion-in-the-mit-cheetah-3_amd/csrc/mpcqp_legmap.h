// mpcqp_legmap.h -- the 6 x 3 wrench map of one leg-stage, A[c][q] = wrench component q of reduced variable c, in the two forms the
// engines build, with the arithmetic that knows where its zeros are.  Both engines' *_sys functions fill these types; the dense 3 x 6
// form (LegMapDense at the end of this file) spends a multiplication on every structural zero (no fast-math: fma(0, x, y) is not folded).
//   ADMM kind    A[c][i] = B[i][c] (i < 3: the angular part, general),  A[c][3 + a] = (a == c) cm:  the linear part is cm I
//   polish kind  angular part general; linear part  row 0 = (d0, 0, 0),  row 1 = (0, d1, 0),  row 2 = (t0, t1, t2)
// Three operations per kind, register values to register values, no lane exchange:
//   wrench   b[6]  = sum(A' a)      `sum`: the caller's quad sum, applied to each component as it is formed
//   back     fin(c, (A c6)[c])  c = 0, 1, 2: each component is handed to the caller as it is formed
//   gram     e[21] = upper triangle of A diag(dinv) A', row by row; `sum` is applied to every entry that is not structurally zero,
//                    the structural zeros are +0
// The terms that remain are the dense expressions' terms in their order (c = 0, 1, 2 in the products, q ascending in `back`), so every
// result is the dense result bit for bit, except that a zero may carry the other sign.  Why:
//   a dropped fma(+-0, x, acc) returns acc, unless acc is -0 (then +0 comes back) -- for finite x, which the input check guarantees;
//   after a dropped leading 0 * x = +-0 the next fma(c, y, +-0) rounds c y once, as the plain product does, and differs from it only in
//   the sign of an exact zero.
// Where such a sign could go, and why it goes nowhere:
//   gram    cm >= 0 and dinv >= 0 make the ADMM kind's all-zero entries +0 in the dense form too; any zero of E is then added to the
//           table entry of K^-1, whose zeros are +0:  x + (+-0) = x  and  (+0) + (+-0) = +0.  The tile is bitwise the same.
//   wrench  S^-1 is dense, so a zero's sign in b reaches the mat-vec result only when every entry of the right-hand side is a zero:
//           a QP without a stance leg on any stage, whose forces are written as selected zeros.
//   back    a stance leg's partial sum is -0 only if the wrench it reads is zero; a swing leg's map (polish kind) is all selected
//           zeros / its dinv is zero (ADMM kind), and its force is selected to zero at the output.
// Host check of exactly this: tools/legmap_check.cpp (tests/test_legmap_host.py).  On the device: tests/test_gpu_legmap_identity.py.
// Plain C++: a host compiler can include this file (no device builtin, no lane operation).
#pragma once
#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LEGMAP_FN __host__ __device__ __forceinline__
#else
#define LEGMAP_FN inline
#endif
// No contraction inside the maps: several results END in a plain product where the dense form ended in an fma, and the device
// compiler (fp-contract on by default) would fuse such a product into the first add of the caller's quad sum -- one rounding fewer,
// another bit pattern.  The multiplications written below are multiplications.
#if defined(__clang__)
#define LEGMAP_EXACT _Pragma("clang fp contract(off)")
#else
#define LEGMAP_EXACT
#endif

namespace {

// One correctly rounded fused multiply-add in the element type (never through a wider type), on the host and on the device.
LEGMAP_FN float lm_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
LEGMAP_FN double lm_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }

template <typename TM>
struct LegMapAdmm {
  static constexpr bool dense = false;
  TM B[3][3];    // B[c][i] = A[c][i], i < 3
  TM cm;         // A[c][3 + c]
  TM dinv[3];
  template <typename F>
  LEGMAP_FN void wrench(const TM (&a)[3], TM (&b)[6], F sum) const {
    LEGMAP_EXACT
    for (int q = 0; q < 3; ++q) b[q] = sum(lm_fma(B[2][q], a[2], lm_fma(B[1][q], a[1], B[0][q] * a[0])));
    for (int c = 0; c < 3; ++c) b[3 + c] = sum(cm * a[c]);
  }
  template <typename F>
  LEGMAP_FN void back(const TM (&c6)[6], F fin) const {
    LEGMAP_EXACT
    for (int c = 0; c < 3; ++c) {
      TM t = B[c][0] * c6[0];
      t = lm_fma(B[c][1], c6[1], t);
      t = lm_fma(B[c][2], c6[2], t);
      fin(c, lm_fma(cm, c6[3 + c], t));
    }
  }
  template <typename F>
  LEGMAP_FN void gram(TM (&e)[21], F sum) const {
    LEGMAP_EXACT
    TM dB[3][3];   // dinv[c] B[c][q]: the dense form's first factor
    for (int c = 0; c < 3; ++c)
      for (int q = 0; q < 3; ++q) dB[c][q] = dinv[c] * B[c][q];
    int k = 0;
    for (int q = 0; q < 3; ++q) {
      for (int p = q; p < 3; ++p) e[k++] = sum(lm_fma(dB[2][q], B[2][p], lm_fma(dB[1][q], B[1][p], dB[0][q] * B[0][p])));
      for (int c = 0; c < 3; ++c) e[k++] = sum(dB[c][q] * cm);
    }
    for (int c = 0; c < 3; ++c) {
      e[k++] = sum((dinv[c] * cm) * cm);
      for (int p = c + 1; p < 3; ++p) e[k++] = (TM)0;
    }
  }
};

template <typename TM>
struct LegMapPolish {
  static constexpr bool dense = false;
  TM B[3][3];    // B[c][i] = A[c][i], i < 3
  TM d0, d1;     // A[0][3], A[1][4]
  TM t[3];       // A[2][3 + a]
  TM dinv[3];
  template <typename F>
  LEGMAP_FN void wrench(const TM (&a)[3], TM (&b)[6], F sum) const {
    LEGMAP_EXACT
    for (int q = 0; q < 3; ++q) b[q] = sum(lm_fma(B[2][q], a[2], lm_fma(B[1][q], a[1], B[0][q] * a[0])));
    b[3] = sum(lm_fma(t[0], a[2], d0 * a[0]));
    b[4] = sum(lm_fma(t[1], a[2], d1 * a[1]));
    b[5] = sum(t[2] * a[2]);
  }
  template <typename F>
  LEGMAP_FN void back(const TM (&c6)[6], F fin) const {
    LEGMAP_EXACT
    TM r[3];
    for (int c = 0; c < 3; ++c) {
      r[c] = B[c][0] * c6[0];
      r[c] = lm_fma(B[c][1], c6[1], r[c]);
      r[c] = lm_fma(B[c][2], c6[2], r[c]);
    }
    fin(0, lm_fma(d0, c6[3], r[0]));
    fin(1, lm_fma(d1, c6[4], r[1]));
    fin(2, lm_fma(t[2], c6[5], lm_fma(t[1], c6[4], lm_fma(t[0], c6[3], r[2]))));
  }
  // Row c of the dense 3 x 6 map (what the records of the polish's rank-one updates hold); its structural zeros are +0.
  LEGMAP_FN void row(const int c, TM (&o)[6]) const {
    for (int q = 0; q < 3; ++q) o[q] = B[c][q];
    o[3] = c == 0 ? d0 : (c == 2 ? t[0] : (TM)0);
    o[4] = c == 1 ? d1 : (c == 2 ? t[1] : (TM)0);
    o[5] = c == 2 ? t[2] : (TM)0;
  }
  template <typename F>
  LEGMAP_FN void gram(TM (&e)[21], F sum) const {
    LEGMAP_EXACT
    TM dB[3][3];
    for (int c = 0; c < 3; ++c)
      for (int q = 0; q < 3; ++q) dB[c][q] = dinv[c] * B[c][q];
    const TM dt[3] = {dinv[2] * t[0], dinv[2] * t[1], dinv[2] * t[2]};
    int k = 0;
    for (int q = 0; q < 3; ++q) {
      for (int p = q; p < 3; ++p) e[k++] = sum(lm_fma(dB[2][q], B[2][p], lm_fma(dB[1][q], B[1][p], dB[0][q] * B[0][p])));
      e[k++] = sum(lm_fma(dB[2][q], t[0], dB[0][q] * d0));
      e[k++] = sum(lm_fma(dB[2][q], t[1], dB[1][q] * d1));
      e[k++] = sum(dB[2][q] * t[2]);
    }
    e[k++] = sum(lm_fma(dt[0], t[0], (dinv[0] * d0) * d0));
    e[k++] = sum(dt[0] * t[1]);
    e[k++] = sum(dt[0] * t[2]);
    e[k++] = sum(lm_fma(dt[1], t[1], (dinv[1] * d1) * d1));
    e[k++] = sum(dt[1] * t[2]);
    e[k++] = sum(dt[2] * t[2]);
  }
};

// The dense form the two maps replace: all eighteen entries, the zeros included.  Data only: a kernel instantiation that loses registers
// to the structured form (W_LEGMAP in mpcqp_wrench.h, SG_LEGMAP in mpcqp_stage.h) has its *_sys functions fill this
// type and keeps, in w_solve / w_build_E / sg_leg_solve / sg_build_E, the expressions it always had -- written out there, because the
// same expressions reached through member functions of this type already move those kernels' instruction order and allocation.
template <typename TM>
struct LegMapDense {
  static constexpr bool dense = true;
  TM A[3][6];    // A[c][q]: wrench component q of reduced variable c
  TM dinv[3];
  LEGMAP_FN void row(const int c, TM (&o)[6]) const {
    for (int q = 0; q < 6; ++q) o[q] = A[c][q];
  }
};

// The map type a kernel instantiation computes with: the structured kind, or the dense form (the engines' *_sys functions fill either).
template <bool STRUCTURED, typename MAP, typename TM> struct LegMapPick { using type = MAP; };
template <typename MAP, typename TM> struct LegMapPick<false, MAP, TM> { using type = LegMapDense<TM>; };

}  // namespace
