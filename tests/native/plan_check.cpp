// Host-side check of the fused launches' plan (csrc/kernels/lenet_plan.h), built with AddressSanitizer +
// UndefinedBehaviorSanitizer on the host (tests/test_native_host_cpu.py): (a) every plan the resolver calls
// valid keeps the invariants the kernels' instantiations rely on, over every batch / grid / dtype / request /
// staging / train-or-eval combination near the thresholds, and (b) the engine's default geometry at each
// threshold is the hand-written table below.
#include <cstdio>
#include <initializer_list>

#include "kernels/lenet_plan.h"

using namespace csed;

static int bad = 0;
#define EXPECT(cond, ...)                                     \
  do {                                                        \
    if (!(cond) && bad++ < 10) { std::printf(__VA_ARGS__); std::printf(": %s\n", #cond); } \
  } while (0)

static long check_batch(int B) {
  const int tiles = (B + 3) / 4, tgrid = tiles < 256 ? tiles : 256;  // (written out: not the header's function)
  long valid = 0;
  const int top = B < 256 ? B : 256;
  for (int gi = 1; gi <= top + 2; ++gi) {
    const int grid = gi <= top ? gi : (gi == top + 1 ? 4 * B : tgrid);
    for (int dt : {kF32, kBF16, kF16})
      for (int req = 0; req <= 2; ++req)
        for (int staged = 0; staged <= 1; ++staged)
          for (int train = 0; train <= 1; ++train) {
            const LenetPlan p = lenet_plan(B, grid, dt, req, staged, staged, false, true, train);
            if (p.error) continue;
            ++valid;
            const bool split = p.variant == kLenetSplit, tile = p.kernel == kLenetTile;
#define WHERE "B=%d grid=%d dtype=%d request=%d staged=%d train=%d", B, grid, dt, req, staged, train
            EXPECT(p.grid == grid, WHERE);
            EXPECT((p.kernel == kLenetFp32) == (dt == kF32), WHERE);
            EXPECT(!split || (staged && train && grid == 4 * B && grid <= 256), WHERE);
            EXPECT(!tile || (dt != kF32 && grid == tgrid), WHERE);
            EXPECT(!(dt == kF32 && staged) || split, WHERE);
            EXPECT(p.one_tile == (tile && B <= 4 * grid), WHERE);
            EXPECT(p.stage_rows == (!staged ? 0 : tile ? 4 * grid : grid), WHERE);
            EXPECT(p.stage_rows <= kLenetStageMaxB, WHERE);
            EXPECT(grid <= B || split, WHERE);
            EXPECT((p.variant == kLenetStaged) == (staged && !tile && !split), WHERE);
            EXPECT(!staged || train, WHERE);
#undef WHERE
          }
  }
  return valid;
}

struct Row {
  int dtype, B;                                  // default grid, split allowed
  int grid, split, staged, tile_staged, rows;    // the geometry
  int kernel, variant, one_tile;                 // the plan of the step it launches (auto request)
};

int main() {
  long valid = 0;
  for (int B = 1; B <= 1100; ++B) valid += check_batch(B);
  for (int B : {2048, 2051, 4096, 8192}) valid += check_batch(B);
  EXPECT(valid > 1000000, "only %ld valid plans", valid);

  // launches that must stay rejected, each with a message
  EXPECT(lenet_plan(64, 64, kBF16, 2, false, false, false, true, true).error, "kernel 2 off the tile grid");
  EXPECT(lenet_plan(1024, 200, kBF16, 0, false, false, false, true, true).error, "auto at B = 1024 on grid 200");
  EXPECT(lenet_plan(64, 64, kF32, 0, true, true, false, true, true).error, "fp32 staged with grid == B");
  EXPECT(lenet_plan(65, 260, kBF16, 0, true, true, false, true, true).error, "staged B = 65 on grid 260");
  EXPECT(lenet_plan(8, 8, kBF16, 0, true, false, false, true, true).error, "xstage without lstage");
  EXPECT(lenet_plan(8, 32, kBF16, 0, false, false, false, true, true).error, "unstaged grid > B");
  EXPECT(lenet_plan(8, 32, kBF16, 0, true, true, true, false, true).error, "stage_next without a cursor");
  EXPECT(lenet_plan(8, 8, kBF16, 0, false, false, true, true, true).error, "stage_next without a staged batch");
  // evaluation chooses its own grid
  EXPECT(lenet_plan(10000, 0, kBF16, 0, false, false, false, false, false).grid == 256, "eval grid");
  EXPECT(lenet_plan(100, 0, kBF16, 0, false, false, false, false, false).grid == 100, "eval grid");
  EXPECT(lenet_plan(100, 0, kBF16, 2, false, false, false, false, false).grid == 25, "eval grid");

  // the engine's defaults at every threshold, read off FusedLeNetTrainer.__init__ as it was before the resolver
  const Row table[] = {
      {kBF16, 8, 32, 1, 1, 0, 32, kLenetPerSample, kLenetSplit, 0},
      {kBF16, 64, 256, 1, 1, 0, 256, kLenetPerSample, kLenetSplit, 0},
      {kBF16, 65, 65, 0, 1, 0, 65, kLenetPerSample, kLenetStaged, 0},
      {kBF16, 256, 256, 0, 1, 0, 256, kLenetPerSample, kLenetStaged, 0},
      {kBF16, 257, 256, 0, 0, 0, 0, kLenetPerSample, kLenetStrided, 0},
      {kBF16, 1023, 256, 0, 0, 0, 0, kLenetPerSample, kLenetStrided, 0},
      {kBF16, 1024, 256, 0, 0, 1, 1024, kLenetTile, kLenetStrided, 1},
      {kBF16, 8192, 256, 0, 0, 1, 1024, kLenetTile, kLenetStrided, 0},
      {kF32, 64, 256, 1, 1, 0, 256, kLenetFp32, kLenetSplit, 0},
      {kF32, 65, 65, 0, 0, 0, 0, kLenetFp32, kLenetStrided, 0},
      {kF32, 8192, 256, 0, 0, 0, 0, kLenetFp32, kLenetStrided, 0},
  };
  for (const Row& r : table) {
    const LenetGeometry g = lenet_geometry(r.B, r.dtype, 0, true);
    EXPECT(g.grid == r.grid && g.split == r.split && g.staged == r.staged && g.tile_staged == r.tile_staged &&
               g.stage_rows == r.rows,
           "geometry dtype=%d B=%d: grid %d split %d staged %d tile_staged %d rows %d", r.dtype, r.B, g.grid, g.split,
           g.staged, g.tile_staged, g.stage_rows);
    const bool st = g.stage_rows > 0;
    const LenetPlan p = lenet_plan(r.B, g.grid, r.dtype, 0, st, st, st, true, true);
    EXPECT(!p.error && p.kernel == r.kernel && p.variant == r.variant && p.one_tile == r.one_tile &&
               p.stage_rows == r.rows,
           "plan dtype=%d B=%d: kernel %d variant %d one_tile %d rows %d (%s)", r.dtype, r.B, p.kernel, p.variant,
           p.one_tile, p.stage_rows, p.error ? p.error : "valid");
  }
  // the split switch off, and an explicit grid: one workgroup per sample, no split
  EXPECT(!lenet_geometry(8, kBF16, 0, false).split && lenet_geometry(8, kBF16, 0, false).grid == 8, "split off");
  EXPECT(!lenet_geometry(8, kF32, 0, false).staged, "fp32 without the split step does not stage");
  EXPECT(lenet_geometry(600, kBF16, 5, false).stage_rows == 0, "explicit grid");
  if (bad) std::printf("plan check FAILED (%d)\n", bad);
  else std::printf("plan check ok (%ld valid plans)\n", valid);
  return bad ? 1 : 0;
}
