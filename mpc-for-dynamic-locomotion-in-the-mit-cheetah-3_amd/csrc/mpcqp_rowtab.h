// mpcqp_rowtab.h -- the lane-order row table of the tile build (mpcqp_wrench.h: w_tile_init_rows), horizon 10.
//
// Per tile row, w_tile_init derives from the lane and the row alone -- never from the QP -- where the row's run of E starts and
// which pair slots lie inside it:  R = 8 gr + r,  h = 3 (R / 6) - 4 gc  (64 beyond the 6 N wrench rows),  base = 6 R - 2 h,  pair slot
// p in the run iff h <= p <= h + 2,  quad hq read from E[base + 4 hq], or from E[0] when neither of its pairs is in the run.  This
// header states that rule ONCE as one 32-bit word per (lane, tile row); mpcqp_create files the words in lane order, eight per lane in the lane's
// record (below: two b128 loads), and the MIXED horizon-10 kernels' builds read them in place of the arithmetic.
//   bits  0..11   8 x the offset of quad 0 into E, fallback applied   (the byte offset in an fp64 E; bits 1..11: in an fp32 E)
//   bits 12..15   bit 12 + p: pair slot p lies in the run
//   bits 16..27   8 x the offset of quad 1
// Plain C++ (no device code): tools/tile_row_table.cpp prints the table and the packed records on the host, tests/test_tile_row_table.py
// holds them against a restatement of the rule and of the record layout.
#pragma once
#include <cstring>

namespace mpcqp_rowtab {

constexpr int PAIR_BIT = 12;    // position of the first pair-in-run bit
constexpr int QUAD_STEP = 16;   // bit distance between the two offset fields

// Offset (in elements of E) of quad hq of tile row r of lane (gr, gc), and the four pair-in-run bits of the row.
constexpr int row_h(int N, int gr, int gc, int r) {
  const int R = 8 * gr + r;
  return R < 6 * N ? 3 * (R / 6) - 4 * gc : 64;
}
constexpr unsigned row_pairs(int N, int gr, int gc, int r) {
  const int h = row_h(N, gr, gc, r);
  unsigned bits = 0;
  for (int p = 0; p < 4; ++p) bits |= (unsigned)(h <= p && p <= h + 2) << p;
  return bits;
}
constexpr int row_quad(int N, int gr, int gc, int r, int hq) {
  const int R = 8 * gr + r, base = 6 * R - 2 * row_h(N, gr, gc, r);
  return (row_pairs(N, gr, gc, r) & (3u << (2 * hq))) ? base + 4 * hq : 0;
}
constexpr unsigned row_word(int N, int gr, int gc, int r) {
  return 8u * (unsigned)row_quad(N, gr, gc, r, 0) | row_pairs(N, gr, gc, r) << PAIR_BIT | 8u * (unsigned)row_quad(N, gr, gc, r, 1) << QUAD_STEP;
}

// The table of a G x G lane grid, [G * G][8].  False if an offset does not fit its field or a read would leave E (36 N elements).
inline bool lane_order_rows(int N, int G, unsigned* tab) {
  bool ok = true;
  for (int t = 0; t < G * G; ++t) {
    for (int r = 0; r < 8; ++r) {
      for (int hq = 0; hq < 2; ++hq) {
        const int o = row_quad(N, t / G, t % G, r, hq);
        ok = ok && o >= 0 && o + 4 <= 36 * N && 8 * o < (1 << PAIR_BIT) && o % 2 == 0;
      }
      tab[8 * t + r] = row_word(N, t / G, t % G, r);
    }
  }
  return ok;
}

// The lane record the kernels read the words from (w_kq_rows_load): the lane's LANE_VALUES K^-1 values of element type T, then its
// ROW_WORDS row words -- one address per lane for both.  A multiple of 16 bytes for float and double.
constexpr int LANE_VALUES = 16, ROW_WORDS = 8;
template <typename T> constexpr int record_words_at() { return LANE_VALUES * (int)sizeof(T); }              // byte offset of the words in a record
template <typename T> constexpr int record_bytes() { return record_words_at<T>() + ROW_WORDS * (int)sizeof(unsigned); }
static_assert(record_bytes<float>() % 16 == 0 && record_bytes<double>() % 16 == 0, "b128 loads of a record");

// nlane records from the [nlane][LANE_VALUES] table of values and the [nlane][ROW_WORDS] table of words.
template <typename T>
inline void pack_records(int nlane, const T* values, const unsigned* words, unsigned char* out) {
  for (int t = 0; t < nlane; ++t) {
    unsigned char* rec = out + (std::size_t)t * record_bytes<T>();
    std::memcpy(rec, values + LANE_VALUES * t, LANE_VALUES * sizeof(T));
    std::memcpy(rec + record_words_at<T>(), words + ROW_WORDS * t, ROW_WORDS * sizeof(unsigned));
  }
}

}  // namespace mpcqp_rowtab
