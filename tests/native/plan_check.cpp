// Host-side check of the fused launches' plan (csrc/kernels/lenet_plan.h), built with AddressSanitizer +
// UndefinedBehaviorSanitizer on the host (tests/test_native_host_cpu.py): (a) every plan the resolver calls
// valid keeps the invariants the kernels' instantiations rely on, over every batch / grid / dtype / request /
// staging / train-or-eval combination near the thresholds, (b) the engine's default geometry at each
// threshold is the hand-written table below, and (c) lenet_update's plan is, case by case, what the launcher
// decided before the plan existed (transcribed below), with the grid invariants update_role relies on, and
// (d) lenet_update_rule accepts and rejects the optimizer options of the table in check_rule, sentence by sentence.
#include <cstdint>
#include <cstdio>
#include <cstring>
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

// ---- lenet_update.  The oracle: a literal transcription of launch_lenet_update, fc_split_slices and
// update_blocks as they stood in lenet_fused.hip before the plan (numbers written out, nothing from the header).
struct OldUpdate {
  bool error;
  int form, xw, loopback, blocks, fc_tpb, fc_sl;  // the kernel launched, its grid and two trailing arguments
};
static int old_waves_per_tile(int B) { return B <= 128 ? 1 : (B <= 256 ? 2 : (B <= 512 ? 4 : 8)); }
static int old_tiles_per_block(int B) { return old_waves_per_tile(B) == 1 ? 1 : 512 / 64 / old_waves_per_tile(B); }
static int old_fc_blocks(int B) { return (88 + old_tiles_per_block(B) - 1) / old_tiles_per_block(B); }
static int old_update_blocks(int B) { return old_fc_blocks(B) + 84; }
static int old_fc_split_slices(bool fc_part, bool exch, bool grad_in, int B, long fc_part_n, int forced) {
  if (!fc_part || exch || grad_in || B <= 512) return 1;
  int S = 1;
  if (forced > 0) {
    while (S * 2 <= (forced < 8 ? forced : 8)) S *= 2;
  } else {
    while (S * 2 <= 8 && S * 2 * 1024 <= B) S *= 2;
  }
  if (fc_part_n < 8 * 88 * 256 + 88) return 1;
  return S;
}
static OldUpdate old_launch_update(int B, bool apply_sgd, bool grad_in, bool vslab, int world, bool loopback, long cap,
                                   double timeout_s, bool lr_table, bool lr_pos, bool ticket, int lr_len,
                                   long fc_part_n, int forced) {
  const OldUpdate invalid{true, 0, 0, 0, 0, 0, 0};
  const bool sched = lr_table, exch = world > 0;
  if (sched && (!apply_sgd || !lr_pos || lr_len < 1 || !ticket)) return invalid;
  if (apply_sgd && grad_in) return {false, kUpdateSgd, 0, 0, (21840 + 255) / 256, 0, 0};
  if (!vslab || B <= 0) return invalid;
  if (exch) {
    if (cap < 27904 || timeout_s <= 0.0) return invalid;
    return {false, kUpdateExchange, world <= 2 ? 2 : (world <= 4 ? 4 : 8), loopback, 84 + 88, 1, 1};
  }
  const int S = old_fc_split_slices(fc_part_n > 0, exch, grad_in, B, fc_part_n, forced);
  if (S > 1) return {false, kUpdateSplitK, 0, 0, 88 * S + 84, 1, S};
  return {false, kUpdatePlain, 0, 0, old_update_blocks(B), 0, 1};
}

static bool pow2(int v) { return v > 0 && !(v & (v - 1)); }

// defect: 0 none; 1 no lr_pos, 2 empty table, 3 no ticket (scheduled launches); 4 no vslab, 5 batch 0;
// 6 exchange buffer one word short, 7 exchange timeout 0
static long check_update(int B, int mode, int world, bool loopback, bool sched, long fc_part_n, int forced, int defect) {
  const bool apply_sgd = mode != 1, grad_in = mode == 2;  // step, reduce, apply
  const bool lr_pos = sched && defect != 1, ticket = defect != 3, vslab = defect != 4;
  const int lr_len = sched ? (defect == 2 ? 0 : 3) : 0, batch = defect == 5 ? 0 : B;
  const long cap = world ? (defect == 6 ? 27903 : 27904) : 0;
  const double timeout_s = defect == 7 ? 0.0 : 2.0;
  const LenetUpdatePlan p = lenet_update_plan(batch, apply_sgd, grad_in, vslab, world, loopback, cap, timeout_s > 0.0,
                                              sched, lr_pos, ticket, lr_len, fc_part_n, forced);
  const OldUpdate o = old_launch_update(batch, apply_sgd, grad_in, vslab, world, loopback, cap, timeout_s, sched,
                                        lr_pos, ticket, lr_len, fc_part_n, forced);
#define WHERE                                                                                                      \
  "update B=%d mode=%d world=%d loopback=%d sched=%d scratch=%ld forced=%d defect=%d", B, mode, world, loopback, sched, \
      fc_part_n, forced, defect
  if (world && grad_in) {  // (the op refused this before it reached the launcher; the plan says so itself)
    EXPECT(p.error && p.error[0], WHERE);
    return 0;
  }
  EXPECT((p.error != nullptr) == o.error, WHERE);
  EXPECT(!p.error || p.error[0], WHERE);  // every rejected launch carries a sentence
  if (p.error || o.error) return 0;
  EXPECT(p.form == o.form && p.world_bound == o.xw && p.loopback == (o.loopback != 0) && p.sched == sched, WHERE);
  EXPECT(p.blocks == o.blocks && p.fc_tpb == o.fc_tpb && p.fc_sl == o.fc_sl, WHERE);
  if (p.form == kUpdateSgd) return 1;
  EXPECT(p.slices == p.fc_sl && (p.slices > 1) == (p.form == kUpdateSplitK), WHERE);
  EXPECT(p.blocks == (p.form == kUpdateSplitK ? 88 * p.slices + 84 : p.fc_blocks + 84), WHERE);
  EXPECT(p.blocks == p.fc_blocks + 84, WHERE);
  EXPECT(pow2(p.waves_per_tile) && pow2(p.tiles_per_block) && pow2(p.slices) && p.slices <= 8, WHERE);
  EXPECT(p.waves_per_tile == old_waves_per_tile(B), WHERE);
  // the kernel packs 8 / waves_per_tile tiles into a block where it derives them from B (fc_tpb 0); where the
  // launcher fixes one tile per block (the exchange's batch-independent map, split-K) the other waves idle
  if (p.fc_tpb == 0) {
    EXPECT(p.waves_per_tile == 1 ? p.tiles_per_block == 1 : p.waves_per_tile * p.tiles_per_block == 8, WHERE);
    EXPECT(p.fc_blocks == (88 + p.tiles_per_block - 1) / p.tiles_per_block, WHERE);
  } else {
    EXPECT(p.tiles_per_block == 1 && p.waves_per_tile * p.tiles_per_block <= 8 && p.fc_blocks == 88 * p.slices, WHERE);
  }
  EXPECT(p.form != kUpdateExchange || (p.blocks == 172 && pow2(p.world_bound) && p.world_bound >= world), WHERE);
  EXPECT(p.form != kUpdateSplitK || (B > 512 && !world && fc_part_n >= 8 * 88 * 256 + 88), WHERE);
#undef WHERE
  return 1;
}

static long check_updates() {
  long valid = 0;
  const long need = 8 * 88 * 256 + 88;
  for (int B : {1, 8, 32, 33, 128, 129, 256, 257, 512, 513, 1024, 1025, 2047, 2048, 2051, 4096, 8192, 16384})
    for (int mode = 0; mode < 3; ++mode)
      for (int world : {0, 2, 3, 4, 8})
        for (int loopback = 0; loopback <= 1; ++loopback)
          for (int sched = 0; sched <= 1; ++sched)
            for (long scratch : {0L, need - 1, need})
              for (int forced : {0, 1, 2, 3, 8, 9})
                for (int defect = 0; defect < 8; ++defect)
                  valid += check_update(B, mode, world, loopback, sched, scratch, forced, defect);
  // the corner cases by hand
  auto slices = [&](int B, long scratch, int forced) {
    return lenet_update_plan(B, true, false, true, 0, false, 0, true, false, false, true, 0, scratch, forced).slices;
  };
  EXPECT(slices(2047, need, 0) == 1 && slices(2048, need, 0) == 2 && slices(4096, need, 0) == 4, "automatic slices");
  EXPECT(slices(8192, need, 0) == 8 && slices(16384, need, 0) == 8, "automatic slices: at most 8");
  EXPECT(slices(512, need, 8) == 1 && slices(513, need, 8) == 8, "a forced count applies past B = 512");
  EXPECT(slices(513, need, 3) == 2 && slices(513, need, 9) == 8 && slices(8192, need, 1) == 1, "forced: pow2, <= 8");
  EXPECT(slices(8192, need - 1, 0) == 1 && slices(8192, 0, 0) == 1, "a short scratch runs unsplit, no error");
  EXPECT(!lenet_update_plan(8192, true, false, true, 0, false, 0, true, false, false, true, 0, need - 1, 0).error,
         "a short scratch is no error");
  const LenetUpdatePlan x = lenet_update_plan(8192, true, false, true, 2, true, 27904, true, false, false, true, 0, need, 0);
  EXPECT(x.blocks == 172 && x.fc_blocks == 88 && x.tiles_per_block == 1 && x.slices == 1 && x.loopback, "exchange at 8192");
  EXPECT(lenet_update_plan(2051, true, false, true, 0, false, 0, true, false, false, true, 0, need, 0).blocks == 260,
         "B = 2051: two slices, 260 blocks");
  return valid;
}

// ---- lenet_update_rule: the optimizer options (EMA, Adam / AdamW).  Four valid launches, then one launch per
// sentence that breaks exactly that rule, then the float32 edge: the rule judges what the kernel will see.
struct Opt {
  const char* what;
  bool apply_sgd, step, ticket;
  float mom, dampening;
  bool nesterov;
  uintptr_t ema;
  double ema_decay;
  uintptr_t adam_v;
  double beta1, beta2, eps;
  const char* says;  // a piece of the sentence; null: a valid launch
};

static void check_rule() {
  const uintptr_t E = 0x7f0000001000, V = 0x7f0000020000;  // (16-byte aligned addresses; never dereferenced)
  const Opt table[] = {
      {"sgd", true, true, true, 0.5f, 0.1f, true, 0, 0.0, 0, 0.0, 0.0, 0.0, nullptr},
      {"sgd, reduce-only", false, false, false, 0.f, 0.f, false, 0, 0.0, 0, 0.0, 0.0, 0.0, nullptr},
      {"ema", true, true, true, 0.5f, 0.f, false, E, 0.999, 0, 0.0, 0.0, 0.0, nullptr},
      {"ema, decay 0", true, false, false, 0.f, 0.f, false, E, 0.0, 0, 0.0, 0.0, 0.0, nullptr},
      {"adam", true, true, true, 0.f, 0.f, false, 0, 0.0, V, 0.9, 0.999, 1e-8, nullptr},
      {"adamw (the rule does not see decoupled) with ema, betas 0", true, true, true, 0.f, 0.f, false, E, 0.99, V, 0.0,
       0.0, 1e-8, nullptr},
      {"ema on a reduce-only launch", false, true, true, 0.f, 0.f, false, E, 0.9, 0, 0.0, 0.0, 0.0,
       "ema comes only with apply_sgd"},
      {"ema_decay 1", true, true, true, 0.f, 0.f, false, E, 1.0, 0, 0.0, 0.0, 0.0, "ema_decay must be in [0, 1)"},
      {"ema_decay < 0", true, true, true, 0.f, 0.f, false, E, -0.1, 0, 0.0, 0.0, 0.0, "ema_decay must be in [0, 1)"},
      {"ema off by 4 bytes", true, true, true, 0.f, 0.f, false, E + 4, 0.9, 0, 0.0, 0.0, 0.0,
       "ema must be 16-byte aligned"},
      {"adam on a reduce-only launch", false, true, true, 0.f, 0.f, false, 0, 0.0, V, 0.9, 0.999, 1e-8,
       "Adam comes only with apply_sgd"},
      {"adam without step", true, false, true, 0.f, 0.f, false, 0, 0.0, V, 0.9, 0.999, 1e-8, "needs step and ticket"},
      {"adam without ticket", true, true, false, 0.f, 0.f, false, 0, 0.0, V, 0.9, 0.999, 1e-8, "needs step and ticket"},
      {"adam_v off by 4 bytes", true, true, true, 0.f, 0.f, false, 0, 0.0, V + 4, 0.9, 0.999, 1e-8,
       "adam_v must be 16-byte aligned"},
      {"beta1 < 0", true, true, true, 0.f, 0.f, false, 0, 0.0, V, -0.1, 0.999, 1e-8, "beta1 must be in [0, 1)"},
      {"beta1 1", true, true, true, 0.f, 0.f, false, 0, 0.0, V, 1.0, 0.999, 1e-8, "beta1 must be in [0, 1)"},
      {"beta2 1", true, true, true, 0.f, 0.f, false, 0, 0.0, V, 0.9, 1.0, 1e-8, "beta2 must be in [0, 1)"},
      {"eps 0", true, true, true, 0.f, 0.f, false, 0, 0.0, V, 0.9, 0.999, 0.0, "eps must be positive"},
      {"adam with mom", true, true, true, 0.5f, 0.f, false, 0, 0.0, V, 0.9, 0.999, 1e-8, "mom, dampening and nesterov"},
      {"adam with dampening", true, true, true, 0.f, 0.1f, false, 0, 0.0, V, 0.9, 0.999, 1e-8,
       "mom, dampening and nesterov"},
      {"adam with nesterov", true, true, true, 0.f, 0.f, true, 0, 0.0, V, 0.9, 0.999, 1e-8, "mom, dampening and nesterov"},
      // below 1 in double, 1.0f in float32 (1 - 2^-30); positive in double, 0.0f in float32
      {"beta1 rounds to 1", true, true, true, 0.f, 0.f, false, 0, 0.0, V, 0.999999999, 0.999, 1e-8,
       "beta1 must be in [0, 1)"},
      {"beta2 rounds to 1", true, true, true, 0.f, 0.f, false, 0, 0.0, V, 0.9, 0.999999999, 1e-8,
       "beta2 must be in [0, 1)"},
      {"ema_decay rounds to 1", true, true, true, 0.f, 0.f, false, E, 0.999999999, 0, 0.0, 0.0, 0.0,
       "ema_decay must be in [0, 1)"},
      {"eps rounds to 0", true, true, true, 0.f, 0.f, false, 0, 0.0, V, 0.9, 0.999, 1e-50, "eps must be positive"},
  };
  int valid = 0;
  for (const Opt& o : table) {
    const char* r = lenet_update_rule(o.apply_sgd, o.step, o.ticket, o.mom, o.dampening, o.nesterov, o.ema,
                                      (float)o.ema_decay, o.adam_v, (float)o.beta1, (float)o.beta2, (float)o.eps);
    valid += !o.says;
    if (!o.says) EXPECT(!r, "rule: %s is valid, got '%s'", o.what, r ? r : "");
    else EXPECT(r && std::strstr(r, o.says), "rule: %s must say '%s', got '%s'", o.what, o.says, r ? r : "(valid)");
  }
  EXPECT(valid == 6, "rule: the valid launches");
  EXPECT(0.999999999 < 1.0 && (float)0.999999999 == 1.0f && 1e-50 > 0.0 && (float)1e-50 == 0.0f, "the float32 edges");
  // the same options break nothing once the buffer is gone
  EXPECT(!lenet_update_rule(false, false, false, 0.5f, 0.1f, true, 0, 7.f, 0, 7.f, 7.f, -1.f), "no buffer, no rule");
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
  const long updates = check_updates();
  EXPECT(updates > 20000, "only %ld valid update plans", updates);
  check_rule();

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
