// Prints the layout contract of csrc/kernels/lenet_layout.h as plain integers, one per line under a
// "# section" header, for tests/test_update_oracle_cpu.py to compare with its Python mirror
// (tests/_update_oracle.py): slab_slot of every conv parameter, slot_param of every slab slot,
// slab_off of every slot at a few rows for a few (grid, batch) pairs, vec16_index at a handful of
// (feature, sample), and the constants.
#include <cstdio>

#include "kernels/lenet_layout.h"

using namespace csed::lenet;

int main() {
  std::printf("# constants\n");
  for (long v : {(long)NP, (long)O_C1W, (long)O_C1B, (long)O_C2W, (long)O_C2B, (long)O_F1W, (long)O_F1B, (long)O_F2W,
                 (long)O_F2B, (long)CNP, (long)C1_CH, (long)S_C2, (long)CNP_PAD, (long)N_CHUNKS, (long)V_P2, (long)V_DZ1,
                 (long)V_H, (long)V_DLOG, (long)VEC, (long)SPLIT_K})
    std::printf("%ld\n", v);
  std::printf("# slab_slot\n");
  for (int p = 0; p < CNP; ++p) std::printf("%d\n", slab_slot(p));
  std::printf("# slot_param\n");
  for (int s = 0; s < CNP_PAD; ++s) std::printf("%d\n", slot_param(s));
  const int gb[5][2] = {{4, 1}, {32, 8}, {7, 100}, {256, 64}, {256, 1000}};
  for (const auto& p : gb) {
    const int G = p[0], B = p[1], R2 = G < B ? G : B;
    std::printf("# slab_off %d %d\n", G, B);
    for (int s = 0; s < CNP_PAD; ++s) {
      const int rows = (s >> 6) < C1_CH ? G : R2;
      for (int row : {0, 1, rows / 2, rows - 1}) std::printf("%d\n", slab_off(s, row < rows ? row : rows - 1, G, R2));
    }
  }
  std::printf("# vec16_index\n");
  for (int f : {0, 1, 319, 320, 383, 384, 448, 463})
    for (int b : {0, 1, 3, 4, 7, 63, 64, 1000, 2050}) std::printf("%lld\n", (long long)vec16_index(f, b));
  std::printf("# vec16_bytes\n");
  for (int B : {1, 63, 64, 65, 1000, 2051}) std::printf("%lld\n", (long long)vec16_bytes(B));
  return 0;
}
