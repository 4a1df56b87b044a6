// tile_row_table.cpp -- prints the row table of the tile build that mpcqp_create files for the horizon-10 kernels
// (csrc/mpcqp_rowtab.h: lane_order_rows, the function build_wrench_tables calls), one line of eight hex words per lane; then the
// lane records as build_wrench_tables packs them (pack_records) from that table and from the values 16 t + i in place of K^-1, read
// back at the offsets the kernels read them at (record_bytes, record_words_at): per element type a line `records <bytes per value>
// <record bytes>` and per lane sixteen values and eight hex words.
//
//   c++ -O1 -std=c++17 -I <csrc> -o tile_row_table tools/tile_row_table.cpp && ./tile_row_table [N G]
//
// Exit status 1 if the builder reports an offset that does not fit its field or a read that leaves E.  tests/test_tile_row_table.py
// holds the output against a numpy restatement of w_tile_init's per-row rule.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mpcqp_rowtab.h"

template <typename T>
static void print_records(int nlane, const unsigned* tab) {
  using namespace mpcqp_rowtab;
  std::vector<T> values((size_t)LANE_VALUES * nlane);
  for (size_t i = 0; i < values.size(); ++i) values[i] = (T)i;
  std::vector<unsigned char> out((size_t)record_bytes<T>() * nlane);
  pack_records<T>(nlane, values.data(), tab, out.data());
  std::printf("records %d %d\n", (int)sizeof(T), record_bytes<T>());
  for (int t = 0; t < nlane; ++t) {
    const unsigned char* rec = out.data() + (size_t)record_bytes<T>() * t;
    for (int i = 0; i < LANE_VALUES; ++i) { T v; std::memcpy(&v, rec + sizeof(T) * i, sizeof(T)); std::printf("%d ", (int)v); }
    for (int r = 0; r < ROW_WORDS; ++r) { unsigned w; std::memcpy(&w, rec + record_words_at<T>() + 4 * r, 4); std::printf("%08x%c", w, r == ROW_WORDS - 1 ? '\n' : ' '); }
  }
}

int main(int argc, char** argv) {
  const int N = argc > 2 ? std::atoi(argv[1]) : 10, G = argc > 2 ? std::atoi(argv[2]) : 8;
  std::vector<unsigned> tab(8 * G * G);
  const bool ok = mpcqp_rowtab::lane_order_rows(N, G, tab.data());
  std::printf("rowtab N %d G %d pair_bit %d quad_step %d fits %d\n", N, G, mpcqp_rowtab::PAIR_BIT, mpcqp_rowtab::QUAD_STEP, (int)ok);
  for (int t = 0; t < G * G; ++t) {
    for (int r = 0; r < 8; ++r) std::printf("%08x%c", tab[8 * t + r], r == 7 ? '\n' : ' ');
  }
  print_records<float>(G * G, tab.data());
  print_records<double>(G * G, tab.data());
  return ok ? 0 : 1;
}
