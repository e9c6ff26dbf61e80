// roialign_plan_check -- host-only check of csrc/roialign_plan.h (no GPU, no HIP): walks the plan over a grid of descriptors
// and checks what the kernels rely on: the tile grid covers every bin row of every RoI exactly once, a workgroup's table
// entries fit the LDS plan, the generic grid is within its cap, the extents are consistent, and the validation refuses
// what it must -- the size limits of the 32-bit byte offsets among them.  Part of `all`; SAN=1 (host/Makefile) builds it
// under AddressSanitizer / UBSan.  Prints "roialign_plan_check: ok" and returns 0, or says what failed and returns 1.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../csrc/roialign_plan.h"

using namespace dfx;

static int g_fail = 0;
#define CHECK(cond, ...)                 \
  do {                                   \
    if (!(cond)) {                       \
      printf("FAIL %s: ", #cond);        \
      printf(__VA_ARGS__);               \
      printf("\n");                      \
      ++g_fail;                          \
    }                                    \
  } while (0)

static dfx_roialign_desc base() {
  dfx_roialign_desc d;
  memset(&d, 0, sizeof(d));
  d.bs = 2; d.n = 5; d.mode = DFX_ROI_BATCHED; d.levels = 2; d.c = 32; d.dt = DFX_U8;
  for (int l = 0; l < 4; ++l) { d.h[l] = 13 >> l ? 13 >> l : 1; d.w[l] = 17 >> l ? 17 >> l : 1; d.src_ld[l] = 32; d.spatial_scale[l] = 1.0f / (1 << l); }
  d.level_area_thr[0] = 100.f; d.level_area_thr[1] = 400.f; d.level_area_thr[2] = 1600.f;
  d.ph = 7; d.pw = 7; d.sampling_ratio = 2; d.aligned = 1; d.dst_ld = 32; d.force_path = -1;
  return d;
}

static int expect(const dfx_roialign_desc &d, int want, const char *what) {
  const char *why = "";
  const int rc = roi_validate(d, &why);
  CHECK(rc == want, "%s: got %d (%s), want %d", what, rc, why, want);
  CHECK(rc == DFX_OK || why[0] != 0, "%s: a refusal without a reason", what);
  return rc != DFX_OK;
}

int main() {
  // ---- the plan over a grid of descriptors ----
  const int Rs[] = {1, 2, 3, 5, 70, 210, 255, 256, 511, 512, 513, 1000, 8000};
  const int bins[] = {1, 2, 3, 7, 14, 63, 64};
  long long plans = 0, groups_walked = 0;
  for (int mode = 0; mode < 2; ++mode)
    for (int R : Rs)
      for (int ph : bins)
        for (int pw : bins)
          for (int S = 1; S <= 4; ++S)
            for (int dt : {DFX_U8, DFX_S8, DFX_F32}) {
              dfx_roialign_desc d = base();
              d.mode = mode; d.ph = ph; d.pw = pw; d.sampling_ratio = S; d.dt = dt;
              if (mode == DFX_ROI_BATCHED) { d.bs = R % 3 == 0 ? 3 : 1; d.n = R / d.bs; } else { d.bs = 2; d.n = R; }
              const unsigned long long rows = roi_rows(d);
              if (expect(d, DFX_OK, "grid point")) continue;
              ++plans;
              CHECK(roi_tile_class(d), "c 32 with ld 32 is in the tile class");
              const int rpg = roi_rows_per_group(d), splits = roi_splits(d);
              CHECK(rpg >= 1 && rpg <= ph, "rows_per_group %d of ph %d", rpg, ph);
              CHECK((splits - 1) * rpg < ph && splits * rpg >= ph, "splits %d x rows %d against ph %d", splits, rpg, ph);
              CHECK(rows < (unsigned)ROI_SPLIT_TARGET || splits == 1, "R %llu fills the device but is split", rows);
              CHECK(roi_tile_grid(d) == rows * splits, "tile grid");
              CHECK(roi_table_entries_y(d) <= ROI_TABLE && roi_table_entries_x(d) <= ROI_TABLE, "table entries %d / %d", roi_table_entries_y(d),
                    roi_table_entries_x(d));
              CHECK((roi_table_entries_y(d) + roi_table_entries_x(d)) * ROI_ENTRY_BYTES <= roi_lds_bytes(DFX_ROIALIGN_TILE), "LDS plan");
              // every bin row of every RoI exactly once, as the kernel derives it from its workgroup index
              std::vector<unsigned char> seen((size_t)rows * ph, 0);
              for (unsigned g = 0; g < roi_tile_grid(d); ++g) {
                const unsigned r = g / (unsigned)splits;
                const int row0 = (int)(g % (unsigned)splits) * rpg, n = rpg < ph - row0 ? rpg : ph - row0;
                CHECK(r < rows && row0 < ph && n >= 1, "workgroup %u owns nothing", g);
                for (int k = 0; k < n; ++k) ++seen[(size_t)r * ph + row0 + k];
                ++groups_walked;
              }
              size_t bad = 0;
              for (unsigned char s : seen) bad += s != 1;
              CHECK(bad == 0, "%zu bin rows not covered exactly once (R %llu, ph %d)", bad, rows, ph);
              const int gg = roi_generic_grid(d);
              CHECK(gg >= 1 && gg <= ROI_MAX_GENERIC_GRID && (unsigned long long)gg * ROI_THREADS >= (roi_elements(d) < (unsigned long long)ROI_MAX_GENERIC_GRID * ROI_THREADS
                                                                                                          ? roi_elements(d)
                                                                                                          : (unsigned long long)ROI_MAX_GENERIC_GRID * ROI_THREADS),
                    "generic grid %d", gg);
              CHECK(roi_dst_extent(d) == (rows * ph * pw - 1) * 32 * roi_esize(dt) + 32ull * roi_esize(dt), "dst extent");
              CHECK(roi_path(d) == DFX_ROIALIGN_GENERIC, "32 bytes of channels are below the measured sizes: generic on auto");
            }
  printf("plan: %lld descriptors, %lld workgroups walked\n", plans, groups_walked);

  // ---- the class ----
  {
    dfx_roialign_desc d = base();
    d.c = 20; d.src_ld[0] = d.src_ld[1] = 32;
    CHECK(!roi_tile_class(d), "c 20 u8");
    d.force_path = DFX_ROIALIGN_TILE;
    expect(d, DFX_ERR_INVALID, "forced tile outside its class");
    d = base(); d.dt = DFX_F32; d.c = 4; d.src_ld[0] = d.src_ld[1] = 4; d.dst_ld = 8;
    CHECK(roi_tile_class(d), "f32 c 4");
    d.c = 6; d.src_ld[0] = d.src_ld[1] = 8;
    CHECK(!roi_tile_class(d), "f32 c 6");
    d = base(); d.src_ld[1] = 40;
    CHECK(!roi_tile_class(d), "u8 ld 40");
    d = base(); d.dst_ld = 36;
    CHECK(!roi_tile_class(d), "u8 dst_ld 36");
    d = base(); d.levels = 1; d.src_ld[1] = 33;  // an unused level does not count
    CHECK(roi_tile_class(d), "unused level");
    // the auto rule: the measured sizes and just below each of them
    d = base(); d.bs = 1; d.n = 100; d.c = 256; d.dst_ld = 256;
    for (int l = 0; l < 4; ++l) d.src_ld[l] = 256;
    CHECK(roi_path(d) == DFX_ROIALIGN_TILE, "u8 c 256, 100 RoIs, 7 x 7");
    d.n = 99;
    CHECK(roi_path(d) == DFX_ROIALIGN_GENERIC, "99 RoIs");
    d.n = 100; d.ph = 6; d.pw = 8;
    CHECK(roi_path(d) == DFX_ROIALIGN_GENERIC, "48 bins");
    d.ph = d.pw = 7; d.c = 240;
    CHECK(roi_path(d) == DFX_ROIALIGN_GENERIC, "240 bytes of channels");
    d.c = 64; d.dt = DFX_F32;
    CHECK(roi_path(d) == DFX_ROIALIGN_TILE, "f32 c 64");
    d.c = 256; d.dt = DFX_U8; d.dst_ld = 260;
    CHECK(roi_path(d) == DFX_ROIALIGN_GENERIC, "outside the class");
    d.force_path = DFX_ROIALIGN_GENERIC; d.dst_ld = 256;
    CHECK(roi_path(d) == DFX_ROIALIGN_GENERIC, "forced");
  }

  // ---- refusals ----
  int refusals = 0;
  const float nan = __builtin_nanf(""), inf = __builtin_inff();
#define REFUSE(code, stmt)                 \
  do {                                     \
    dfx_roialign_desc d = base();          \
    stmt;                                  \
    refusals += expect(d, code, #stmt);    \
  } while (0)
  REFUSE(DFX_ERR_INVALID, d.bs = 0);
  REFUSE(DFX_ERR_INVALID, d.n = 0);
  REFUSE(DFX_ERR_INVALID, d.mode = 2);
  REFUSE(DFX_ERR_INVALID, d.levels = 0);
  REFUSE(DFX_ERR_INVALID, d.levels = 5);
  REFUSE(DFX_ERR_INVALID, d.c = 0);
  REFUSE(DFX_ERR_INVALID, d.dt = DFX_S32);
  REFUSE(DFX_ERR_INVALID, d.h[1] = 0);
  REFUSE(DFX_ERR_INVALID, d.w[0] = 65536);
  REFUSE(DFX_ERR_INVALID, d.src_ld[1] = 31);
  REFUSE(DFX_ERR_INVALID, d.dst_ld = 31);
  REFUSE(DFX_ERR_INVALID, d.spatial_scale[0] = 0.0f);
  REFUSE(DFX_ERR_INVALID, d.spatial_scale[1] = -1.0f);
  REFUSE(DFX_ERR_INVALID, d.spatial_scale[1] = nan);
  REFUSE(DFX_ERR_INVALID, d.spatial_scale[0] = inf);
  REFUSE(DFX_ERR_INVALID, d.level_area_thr[0] = nan);
  REFUSE(DFX_ERR_INVALID, d.level_area_thr[0] = inf);
  REFUSE(DFX_ERR_INVALID, (d.levels = 3, d.level_area_thr[1] = 50.f));
  REFUSE(DFX_ERR_INVALID, d.ph = 0);
  REFUSE(DFX_ERR_INVALID, d.pw = 65);
  REFUSE(DFX_ERR_INVALID, d.sampling_ratio = 5);
  REFUSE(DFX_ERR_INVALID, d.sampling_ratio = -1);
  REFUSE(DFX_ERR_INVALID, d.aligned = 2);
  REFUSE(DFX_ERR_INVALID, d.force_path = 2);
  REFUSE(DFX_ERR_UNSUPPORTED, d.sampling_ratio = 0);
  // the limits of the 32-bit byte offsets
  REFUSE(DFX_ERR_UNSUPPORTED, (d.mode = DFX_ROI_LIST, d.n = 2147483647, d.ph = d.pw = 64));
  REFUSE(DFX_ERR_UNSUPPORTED, (d.bs = 2147483647, d.n = 2147483647));
  REFUSE(DFX_ERR_UNSUPPORTED, (d.mode = DFX_ROI_LIST, d.n = (1 << 27) / 49 + 1));                 // dst: 49 * 32 bytes per row
  REFUSE(DFX_ERR_UNSUPPORTED, (d.levels = 1, d.bs = 1, d.c = 1, d.src_ld[0] = 2, d.dst_ld = 1, d.h[0] = d.w[0] = 65535));
  REFUSE(DFX_ERR_UNSUPPORTED, (d.levels = 1, d.bs = 1, d.c = 1, d.src_ld[0] = 1, d.dst_ld = 1, d.dt = DFX_F32, d.h[0] = d.w[0] = 65535));
  REFUSE(DFX_ERR_UNSUPPORTED, (d.bs = 2147483647, d.n = 1, d.mode = DFX_ROI_LIST, d.h[0] = d.w[0] = 65535, d.src_ld[0] = 2147483647));
  {  // just inside: 65535 * 65535 bytes < 2^32, and the last dst row that fits
    dfx_roialign_desc d = base();
    d.levels = 1; d.bs = 1; d.c = 1; d.src_ld[0] = 1; d.dst_ld = 1; d.h[0] = d.w[0] = 65535;
    expect(d, DFX_OK, "a level of 65535 x 65535 bytes");
    d = base(); d.mode = DFX_ROI_LIST; d.n = (1 << 27) / 49;
    expect(d, DFX_OK, "the largest dst");
    CHECK(roi_dst_extent(d) < ROI_MAX_BYTES, "its extent");
  }
  printf("validation: %d refusals\n", refusals);

  if (g_fail) {
    printf("roialign_plan_check: %d FAILED\n", g_fail);
    return 1;
  }
  printf("roialign_plan_check: ok\n");
  return 0;
}
