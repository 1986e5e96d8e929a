// Which training kernel runs a fused LeNet launch, in which instantiation, on what grid and with
// how many staging rows, and which form, instantiation and grid the step's second launch (lenet_update)
// gets: decided here and nowhere else.  The launchers (lenet_fused.hip, lenet_tile.hip,
// lenet_fused_f32.hip) dispatch on lenet_plan() / lenet_update_plan(), the ops (bindings.cpp) report
// their message, and Python asks through csed::lenet_plan / csed::lenet_geometry /
// csed::lenet_update_plan (engine/fused.py).  lenet_update_rule() holds the rules of lenet_update's optimizer
// options (EMA, Adam / AdamW), for the launcher and the ops alike.  A new kernel variant is added here.  Plain scalar logic:
// no HIP call, no environment, no allocation (tests/native/plan_check.cpp runs it on the host).
#pragma once
#include <stdint.h>

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

// ---------------------------------------------------------------------------
// lenet_update: the step's second launch (kernels/lenet_fused.hip update_role).  Two block roles in one
// grid, the FC blocks first, then NB_CONV CONV blocks.
namespace lenet {
constexpr int UP_WAVES = 8;                         // waves of an update workgroup (UP_NT / 64)
constexpr int NB_CONV = 84;                         // CONV blocks: one 64-slot slab chunk each (N_CHUNKS)
constexpr int FC1_TILES = 4 * 21, FC_TILES = FC1_TILES + 4;
// FC role: wpt waves per tile (K split over them), 8 / wpt tiles per block.  A
// small batch uses one wave per tile (no combine, no barrier: the tile's K is one
// or two 64-sample chunks); a large batch streams K over 8 waves.
constexpr int fc_waves_per_tile(int B) {
  return B <= 128 ? 1 : (B <= 256 ? 2 : (B <= 512 ? 4 : 8));
}
// Update workgroups of UP_NT threads: a CONV workgroup holds one 64-parameter block; an FC
// workgroup UP_NT/64/wpt tiles when the batch splits K over waves, else ONE tile: the FC
// phase is bound by per-CU load / store issue (32 loads and ~12 stores per tile wave), so
// 88 workgroups of one tile beat 11 of eight (16.86 -> 16.38 us/step, round 1).
constexpr int fc_tiles_per_block(int B) {
  return fc_waves_per_tile(B) == 1 ? 1 : UP_WAVES / fc_waves_per_tile(B);
}
constexpr int fc_blocks(int B) {
  return (FC_TILES + fc_tiles_per_block(B) - 1) / fc_tiles_per_block(B);
}
constexpr int update_blocks(int B) { return fc_blocks(B) + NB_CONV; }
// (update_role shifts by log2 of both: they must stay powers of two)
constexpr bool fc_shapes_pow2() {
  for (int B : {1, 32, 64, 128, 129, 256, 257, 512, 513, 1024, 8192}) {
    const int w = fc_waves_per_tile(B), t = fc_tiles_per_block(B);
    if ((w & (w - 1)) || (t & (t - 1))) return false;
  }
  return true;
}
static_assert(fc_shapes_pow2(), "fc waves per tile / tiles per block: powers of two");
constexpr int NB_FC = FC_TILES;                     // FC blocks at most (one tile each)
constexpr int NB_UPDATE = NB_CONV + NB_FC;
// split-K fc gradients: at most FC_MAX_SLICES batch slices of 88 tiles x 256 partial sums, then
// 88 arrival counters (ints, zero between launches) in the same fp32 scratch
constexpr int FC_MAX_SLICES = 8;
constexpr int FC_PART_FLOATS = FC_MAX_SLICES * FC_TILES * 256;
constexpr int FC_SPLIT_MIN_B = 513;                 // smallest batch a (forced) slice count applies to
constexpr int FC_SLICE_B = 1024;                    // automatic slices: one per this many samples
constexpr int EXCH_WORDS = NB_CONV * 64 + FC_TILES * 256;  // 27904 words per sender of the fused exchange
constexpr int SGD_BLOCKS = 86;                      // lenet_sgd_kernel: 256 parameters per block
}  // namespace lenet

enum : int { kUpdateSgd = 0, kUpdateExchange = 1, kUpdateSplitK = 2, kUpdatePlain = 3 };  // LenetUpdatePlan::form

struct LenetUpdatePlan {
  int form;            // SGD from grad_in (lenet_sgd_kernel); else lenet_update_kernel: fused exchange, split-K fc, plain
  int world_bound;     // XW: 0 (no exchange) or the exchange's world rounded up to 2 / 4 / 8
  bool loopback;       // LBC: the looped-back exchange with its invariant check
  bool sched;          // SCHED: the learning rate comes from the device-resident schedule
  int blocks;          // the launch's grid
  int fc_blocks;       // of them the FC role (the first ones); the rest are the NB_CONV CONV blocks
  int waves_per_tile;  // waves that split one FC tile's K (the others of a one-tile block idle)
  int tiles_per_block;
  int slices;          // split-K batch slices per FC tile (1: unsplit)
  int fc_tpb, fc_sl;   // the kernel's trailing arguments: FC tiles per block fixed here (0: it derives them from B), slices
  const char* error;   // null: a valid launch; else the rule it breaks
};

// exch_world: the fused exchange's world (0: no exchange), exch_cap its words per sender.  fc_part_n:
// floats of the split-K scratch (0: none).  forced_slices: CSED_FC_SLICES (0: automatic).
inline LenetUpdatePlan lenet_update_plan(int B, bool apply_sgd, bool grad_in, bool vslab, int exch_world,
                                         bool exch_loopback, int64_t exch_cap, bool exch_timeout, bool lr_table,
                                         bool lr_pos, bool ticket, int lr_len, int64_t fc_part_n, int forced_slices) {
  using namespace lenet;
  LenetUpdatePlan p{};
  const bool exch = exch_world > 0;
  p.sched = lr_table;
  // a device-resident schedule: SGD-applying launches only, with a position and at least one entry
  p.error = !lr_table              ? nullptr
            : !apply_sgd           ? "reduce-only mode applies no SGD step and takes no lr_table"
            : !lr_pos              ? "lr_table and lr_pos come together"
            : lr_len < 1           ? "lr_table needs at least one entry"
            : !ticket              ? "a scheduled launch needs the ticket counter"
                                   : nullptr;
  if (!p.error && exch && grad_in) p.error = "the fused exchange reduces the slabs itself (no grad_in)";
  if (p.error) return p;
  if (apply_sgd && grad_in) {
    p.form = kUpdateSgd;
    p.blocks = SGD_BLOCKS;
    return p;
  }
  p.error = !vslab ? "vslab: the step's fc vectors are missing" : B < 1 ? "batch must be positive" : nullptr;
  if (p.error) return p;
  p.waves_per_tile = fc_waves_per_tile(B);
  p.slices = 1;
  if (exch) {
    // The exchange tag is a per-workgroup call counter, so the workgroup -> exchange-word map
    // must not depend on the batch: one FC tile per workgroup (NB_UPDATE workgroups) for
    // every B, the full steps' and the epoch tail's alike (a batch-dependent layout let
    // the counters of different words drift apart between steps of different batch sizes).
    p.form = kUpdateExchange;
    p.world_bound = exch_world <= 2 ? 2 : (exch_world <= 4 ? 4 : 8);
    p.loopback = exch_loopback;
    p.error = exch_cap < EXCH_WORDS ? "the exchange buffer holds fewer than lenet_exch_words() words per sender"
              : !exch_timeout       ? "the exchange timeout must be positive"
                                    : nullptr;
  } else if (fc_part_n > 0 && !grad_in && B >= FC_SPLIT_MIN_B) {
    // Split-K fc gradients, large batches only (the FC role's K loop then streams B x 32 features per
    // tile on 88 CUs): S = B / 1024 rounded down to a power of two, at most 8, or the forced count
    // likewise; a scratch too small for the partials + the per-tile counters runs unsplit.
    int S = 1;
    if (forced_slices > 0) {
      while (S * 2 <= (forced_slices < FC_MAX_SLICES ? forced_slices : FC_MAX_SLICES)) S *= 2;
    } else {
      while (S * 2 <= FC_MAX_SLICES && S * 2 * FC_SLICE_B <= B) S *= 2;
    }
    if (fc_part_n >= FC_PART_FLOATS + FC_TILES) p.slices = S;
  }
  if (p.form != kUpdateExchange) p.form = p.slices > 1 ? kUpdateSplitK : kUpdatePlain;
  // one tile per workgroup (x S slices, the last one to arrive finishes the tile), or packed by B
  p.fc_tpb = p.form == kUpdatePlain ? 0 : 1;
  p.fc_sl = p.slices;
  p.tiles_per_block = p.fc_tpb ? 1 : fc_tiles_per_block(B);
  p.fc_blocks = p.fc_tpb ? FC_TILES * p.slices : fc_blocks(B);
  p.blocks = p.fc_blocks + NB_CONV;
  return p;
}

// The launch's optimizer options, which are no plan dimension (the kernels' EMA / ADAM template flags): the
// rule they break, or null.  The launcher and the ops (launchers.h lenet_update_rule(LenetUpdateArgs)) both
// ask here, with the float32 values the kernel will see.  ema / adam_v: the buffers' addresses, 0 for none.
inline const char* lenet_update_rule(bool apply_sgd, bool step, bool ticket, float mom, float dampening, bool nesterov,
                                     uintptr_t ema, float ema_decay, uintptr_t adam_v, float beta1, float beta2,
                                     float eps) {
  const auto unit = [](float x) { return x >= 0.f && x < 1.f; };  // (false for a NaN)
  if (ema) {
    if (!apply_sgd) return "ema comes only with apply_sgd (a reduce-only launch changes no parameter)";
    if (!unit(ema_decay)) return "ema_decay must be in [0, 1) in float32";
    if (ema & 15) return "ema must be 16-byte aligned";
  }
  if (!adam_v) return nullptr;
  return !apply_sgd         ? "Adam comes only with apply_sgd (a reduce-only launch changes no parameter)"
         : !step || !ticket ? "Adam reads the step number in every block: it needs step and ticket"
         : adam_v & 15      ? "adam_v must be 16-byte aligned"
         : !unit(beta1)     ? "beta1 must be in [0, 1) in float32"
         : !unit(beta2)     ? "beta2 must be in [0, 1) in float32"
         : !(eps > 0.f)     ? "eps must be positive in float32"
         : mom != 0.f || dampening != 0.f || nesterov
             ? "mom, dampening and nesterov are SGD's and must be 0 under Adam"
             : nullptr;
}

// The engine allocates the split-K scratch from this per-rank batch on: past one automatic slice's worth
// (the automatic count exceeds 1 from 2 * FC_SLICE_B; a forced count applies to every batch that has the scratch).
constexpr int kLenetFcPartMinB = lenet::FC_SLICE_B + 1;

}  // namespace csed
