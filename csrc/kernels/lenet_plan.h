// Which training kernel runs a fused LeNet launch, in which instantiation, on what grid and with
// how many staging rows: decided here and nowhere else.  The launchers (lenet_fused.hip,
// lenet_tile.hip, lenet_fused_f32.hip) dispatch on lenet_plan(), the ops (bindings.cpp) report its
// message, and Python asks through csed::lenet_plan / csed::lenet_geometry (engine/fused.py).  A new
// kernel variant is added here.  Plain integer logic: no HIP call, no environment, no allocation
// (tests/native/plan_check.cpp runs it on the host).
#pragma once

namespace csed {

// dtype codes shared with Python (see ops/_dtypes.py)
enum : int { kF32 = 0, kBF16 = 1, kF16 = 2, kU8 = 3 };

namespace lenet {
constexpr int SPLIT_K = 4;  // split step: workgroups per sample (the backward conv stages are divided among them)
}
constexpr int kLenetTileSamples = 4;   // samples per tile of the sample-tile kernel (lenet_tile.hip)
constexpr int kLenetTileMinB = 1024;   // smallest per-rank batch the auto request runs on it
constexpr int kLenetStageMaxB = 1024;  // most staging rows (the tile kernel: 256 workgroups x 4 samples)
constexpr int kLenetWave = 256;        // one wave of workgroups: default / tile / split / fp32 grids end here
constexpr int kLenetMaxGrid = 1024;    // the per-sample 16-bit kernel's largest grid

// workgroups of the sample-tile kernel at per-rank batch B
constexpr int lenet_tile_grid(int B) {
  const int tiles = (B + kLenetTileSamples - 1) / kLenetTileSamples;
  return tiles < kLenetWave ? tiles : kLenetWave;
}

enum : int { kLenetPerSample = 0, kLenetTile = 1, kLenetFp32 = 2 };  // LenetPlan::kernel
enum : int { kLenetStrided = 0, kLenetStaged = 1, kLenetSplit = 2 };  // LenetPlan::variant

struct LenetPlan {
  int kernel;         // lenet_train (per sample), lenet_tile or lenet_train_f32
  int variant;        // workgroups stride over samples (tiles) / one staged sample per workgroup / split step
  int grid;           // the launch's grid (evaluation with grid 0: chosen here)
  bool one_tile;      // tile kernel: every workgroup has exactly one tile
  int stage_rows;     // staging rows the launch reads and (stage_next) writes; 0: it gathers through perm
  const char* error;  // null: a valid launch; else the rule it breaks
};

// request: 0 auto, 1 per-sample kernel, 2 sample-tile kernel (the exact-fp32 kernel ignores it).
inline LenetPlan lenet_plan(int B, int grid, int mfma_dtype, int request, bool xstage, bool lstage, bool stage_next,
                            bool cursor, bool train) {
  LenetPlan p{};
  const bool fp32 = mfma_dtype == kF32, staged = xstage && lstage;
  p.kernel = fp32 ? kLenetFp32
                  : (request == 2 || (request == 0 && B >= kLenetTileMinB)) ? kLenetTile : kLenetPerSample;
  const bool tile = p.kernel == kLenetTile;
  if (!train && grid == 0) grid = tile ? lenet_tile_grid(B) : (B < kLenetWave ? B : kLenetWave);
  p.grid = grid;
  const bool split_grid = staged && !tile && grid == lenet::SPLIT_K * B;
  const bool split = split_grid && train && grid <= kLenetWave;
  p.variant = split ? kLenetSplit : (staged && !tile ? kLenetStaged : kLenetStrided);
  p.one_tile = tile && B <= kLenetTileSamples * grid;
  p.stage_rows = !staged ? 0 : (tile ? grid * kLenetTileSamples : grid);
  p.error = B < 1 || grid < 1                     ? "batch and grid must be positive"
            : request < 0 || request > 2          ? "kernel 0 (auto), 1 (per sample) or 2 (sample tiles)"
            : xstage != lstage                    ? "xstage and lstage go together"
            : staged && !train                    ? "evaluation reads no staged batch"
            : stage_next && !(staged && cursor)   ? "stage_next needs a staged batch and the cursor"
            : tile && grid != lenet_tile_grid(B)  ? "the sample-tile kernel runs grid min(256, ceil(B / 4))"
            : tile || split                       ? nullptr
            : split_grid                          ? "the split step (grid = split_k * B) runs at most 256 workgroups"
            : grid > B                            ? "1 <= grid <= B (or split_k * B for a staged batch)"
            : grid > (fp32 ? kLenetWave : kLenetMaxGrid) ? "grid <= 1024 (fp32: 256)"
            : fp32 && staged ? "fp32 stages its batch only in the split step (grid = split_k * B)"
            : staged && grid != B ? "the per-sample kernel stages one sample per workgroup (grid == B or split_k * B)"
                                  : nullptr;
  return p;
}

// The engine's default launch of a full step (engine/fused.py FusedLeNetTrainer): grid 0 = min(B, 256).
// The split step runs where allowed (allow_split: no explicit grid, CSED_SPLIT / split= not off) and
// split_k * B fits one wave; else a batch of one workgroup per sample is staged (16-bit only), and the
// tile kernel's launch stages every workgroup's first tile.
struct LenetGeometry {
  int grid;
  bool split, staged, tile_staged;
  int stage_rows;
};

inline LenetGeometry lenet_geometry(int B, int mfma_dtype, int grid, bool allow_split) {
  LenetGeometry g{};
  g.grid = grid > 0 ? grid : (B < kLenetWave ? B : kLenetWave);
  const bool can_stage = B <= kLenetStageMaxB && g.grid == B;
  g.split = can_stage && allow_split && lenet::SPLIT_K * B <= kLenetWave;
  g.staged = can_stage && (mfma_dtype != kF32 || g.split);
  if (g.split) g.grid = lenet::SPLIT_K * B;
  const LenetPlan p = lenet_plan(B, g.grid, mfma_dtype, 0, true, true, false, true, true);
  g.tile_staged = !g.staged && p.kernel == kLenetTile && !p.error;
  g.stage_rows = g.staged ? g.grid : (g.tile_staged ? p.stage_rows : 0);
  return g;
}

}  // namespace csed
