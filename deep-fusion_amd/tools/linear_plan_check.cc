// linear_plan_check -- host-only check of csrc/linear_plan.h and csrc/linear_pack.h, what the int8 token linear op
// (dfx_linear_*) decides before a kernel runs: the order of the descriptor's validation (every DFX_ERR_INVALID before the one
// DFX_ERR_UNSUPPORTED) at the last admitted and the first refused value of every bound, the class and auto predicates, the
// tile height, tiles and grids under the cap, the LDS plan, the image's sections, and the packer: every weight at its
// documented place, zero pads, the compensation, the route's proof at its edge.  No HIP: it builds with SAN=1 (ASan + UBSan)
// and runs anywhere.
//   linear_plan_check
//   linear_plan_check plan <rows> <k> <n> <src_ld> <dst_ld> <cus> <forced_bm> <cap> <weights.bin> <image.bin>
//     prints the plan of the descriptor (s8 in and out, forced tile path) as "key value" lines and writes the image that
//     lin_pack makes of the n * k weight bytes in weights.bin (no bias, scale 1): tests/test_linear_cpu.py compares both with
//     its Python mirror
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../csrc/linear_pack.h"
#include "../csrc/linear_plan.h"

using namespace dfx;

static int g_bad = 0;
#define EXPECT(cond)                                                  \
  do {                                                                \
    if (!(cond)) {                                                    \
      printf("linear_plan_check: line %d: %s\n", __LINE__, #cond);    \
      ++g_bad;                                                        \
    }                                                                 \
  } while (0)

static dfx_linear_desc desc(long long rows, int k, int n, long long src_ld, long long dst_ld, int src_dt = DFX_S8, int dst_dt = DFX_S8) {
  dfx_linear_desc d;
  memset(&d, 0, sizeof(d));
  d.rows = rows; d.k = k; d.n = n; d.src_dt = src_dt; d.dst_dt = dst_dt; d.bia_dt = DFX_UNDEF; d.relu = 0; d.round_mode = DFX_ROUND_NEAREST;
  d.nscales = 1; d.lut_in_dt = DFX_UNDEF; d.force_path = -1; d.src_ld = src_ld; d.dst_ld = dst_ld;
  return d;
}
static int rc(const dfx_linear_desc &d) {
  const char *why = nullptr;
  const int r = lin_validate(d, &why);
  EXPECT(why != nullptr && (r == DFX_OK) == (why[0] == 0));
  EXPECT(lin_validate(d, nullptr) == r);
  return r;
}

static int plan_mode(char **v) {
  const long long rows = atoll(v[0]), src_ld = atoll(v[3]), dst_ld = atoll(v[4]), cap = atoll(v[7]);
  const int k = atoi(v[1]), n = atoi(v[2]), cus = atoi(v[5]), forced = atoi(v[6]);
  dfx_linear_desc d = desc(rows, k, n, src_ld, dst_ld);
  d.force_path = DFX_LINEAR_TILE;
  const char *why = "";
  const int r = lin_validate(d, &why);
  printf("validate %d\n", r);
  if (r) return 0;
  const int bm = lin_bm(d, cus, forced);
  const LinImage im = lin_image(n, k);
  printf("path %d\nbm %d\ntiles %lld\ngrid_tile %d\ngrid_generic %d\nlds %d\n", lin_path(d), bm, lin_tiles(d, bm),
         lin_grid(d, DFX_LINEAR_TILE, bm, cus, cap), lin_grid(d, DFX_LINEAR_GENERIC, bm, cus, cap), lin_lds_bytes(DFX_LINEAR_TILE, bm));
  printf("off_comp %zu\noff_bias %zu\noff_scale %zu\noff_table %zu\nbytes %zu\n", im.off_comp, im.off_bias, im.off_scale, im.off_table, im.bytes);
  std::vector<int8_t> w((size_t)n * k);
  FILE *f = fopen(v[8], "rb");
  if (!f || fread(w.data(), 1, w.size(), f) != w.size()) {
    printf("linear_plan_check: cannot read %s\n", v[8]);
    if (f) fclose(f);
    return 1;
  }
  fclose(f);
  std::vector<unsigned char> img(im.bytes, 0xEE);
  const float one = 1.0f;
  printf("fast %d\n", (int)lin_pack(d, w.data(), nullptr, &one, img.data()));
  for (size_t i = im.off_table; i < im.bytes; ++i)
    if (img[i] != 0xEE) {
      printf("linear_plan_check: lin_pack wrote into the table section\n");
      return 1;
    }
  f = fopen(v[9], "wb");
  if (!f || fwrite(img.data(), 1, im.off_table, f) != im.off_table) {
    printf("linear_plan_check: cannot write %s\n", v[9]);
    if (f) fclose(f);
    return 1;
  }
  fclose(f);
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 12 && !strcmp(argv[1], "plan")) return plan_mode(argv + 2);
  if (argc != 1) {
    printf("usage: linear_plan_check | linear_plan_check plan <rows> <k> <n> <src_ld> <dst_ld> <cus> <forced_bm> <cap> <weights.bin> <image.bin>\n");
    return 2;
  }
  // ---- validation, each bound at its last admitted and first refused value
  EXPECT(rc(desc(1, 1, 1, 1, 1)) == DFX_OK);
  EXPECT(rc(desc(0, 1, 1, 1, 1)) == DFX_ERR_INVALID && rc(desc(-1, 1, 1, 1, 1)) == DFX_ERR_INVALID);
  EXPECT(rc(desc(4, 0, 8, 16, 8)) == DFX_ERR_INVALID && rc(desc(4, -1, 8, 16, 8)) == DFX_ERR_INVALID);
  EXPECT(rc(desc(4, LIN_KMAX, 8, LIN_KMAX, 8)) == DFX_OK && rc(desc(4, LIN_KMAX + 1, 8, LIN_KMAX + 1, 8)) == DFX_ERR_INVALID);
  EXPECT(rc(desc(4, 8, 0, 8, 8)) == DFX_ERR_INVALID);
  EXPECT(rc(desc(1, 8, LIN_NMAX, 8, LIN_NMAX)) == DFX_OK && rc(desc(1, 8, LIN_NMAX + 1, 8, (long long)LIN_NMAX + 1)) == DFX_ERR_INVALID);
  EXPECT(rc(desc(4, 96, 40, 95, 40)) == DFX_ERR_INVALID && rc(desc(4, 96, 40, 96, 39)) == DFX_ERR_INVALID && rc(desc(4, 96, 40, 97, 41)) == DFX_OK);
  for (int dt : {(int)DFX_UNDEF, (int)DFX_F32, (int)DFX_S32, 5, -1}) EXPECT(rc(desc(4, 96, 40, 96, 40, dt, DFX_S8)) == DFX_ERR_INVALID);
  for (int dt : {(int)DFX_UNDEF, 5, -1}) EXPECT(rc(desc(4, 96, 40, 96, 40, DFX_S8, dt)) == DFX_ERR_INVALID);
  for (int s : {(int)DFX_S8, (int)DFX_U8})
    for (int o : {(int)DFX_S8, (int)DFX_U8, (int)DFX_S32, (int)DFX_F32}) EXPECT(rc(desc(4, 96, 40, 96, 40, s, o)) == DFX_OK);
  {
    dfx_linear_desc d = desc(4, 96, 40, 96, 40);
    for (int b = -1; b <= 5; ++b) {
      d.bia_dt = b;
      EXPECT(rc(d) == ((b >= 0 && b <= 4) ? DFX_OK : DFX_ERR_INVALID));
    }
    d.bia_dt = DFX_UNDEF;
    for (int m = -1; m <= 2; ++m) {
      d.round_mode = m;
      EXPECT(rc(d) == ((m == 0 || m == 1) ? DFX_OK : DFX_ERR_INVALID));
    }
    d.round_mode = 0;
    for (int s : {0, 1, 2, 39, 40, 41}) {
      d.nscales = s;
      EXPECT(rc(d) == ((s == 1 || s == 40) ? DFX_OK : DFX_ERR_INVALID));
    }
    d.nscales = 1;
    for (int t = -1; t <= 5; ++t) {
      d.lut_in_dt = t;
      EXPECT(rc(d) == ((t == DFX_UNDEF || t == DFX_S8 || t == DFX_U8) ? DFX_OK : DFX_ERR_INVALID));
    }
    d.lut_in_dt = DFX_S8;
    for (int o : {(int)DFX_S32, (int)DFX_F32}) {
      d.dst_dt = o;
      EXPECT(rc(d) == DFX_ERR_INVALID);
    }
    d.dst_dt = DFX_U8;
    EXPECT(rc(d) == DFX_OK);
    d.lut_in_dt = DFX_UNDEF;
    for (int p = -3; p <= 3; ++p) {
      d.force_path = p;
      EXPECT(rc(d) == ((p >= -1 && p <= 1) ? DFX_OK : DFX_ERR_INVALID));
    }
  }
  // the 2^40 limit, on either pitch
  EXPECT(rc(desc((1ll << 40) / 96, 96, 40, 96, 40)) == DFX_OK && rc(desc((1ll << 40) / 96 + 1, 96, 40, 96, 40)) == DFX_ERR_INVALID);
  EXPECT(rc(desc(1ll << 33, 96, 40, 96, 128)) == DFX_OK && rc(desc((1ll << 33) + 1, 96, 40, 96, 128)) == DFX_ERR_INVALID);
  EXPECT(rc(desc(1ll << 40, 1, 1, 1, 1)) == DFX_OK && rc(desc((1ll << 40) + 1, 1, 1, 1, 1)) == DFX_ERR_INVALID);
  EXPECT(rc(desc(2, 8, 8, 1ll << 62, 8)) == DFX_ERR_INVALID);  // (no overflow in the product)
  // the one UNSUPPORTED, and only after everything invalid
  {
    dfx_linear_desc d = desc(4, 96, 40, 100, 40);
    EXPECT(!lin_tile_class(d) && rc(d) == DFX_OK && lin_path(d) == DFX_LINEAR_GENERIC);
    d.force_path = DFX_LINEAR_TILE;
    EXPECT(rc(d) == DFX_ERR_UNSUPPORTED);
    d.nscales = 2;
    EXPECT(rc(d) == DFX_ERR_INVALID);
    d.nscales = 1;
    d.rows = 0;
    EXPECT(rc(d) == DFX_ERR_INVALID);
    d.rows = 4;
    d.dst_ld = 39;
    EXPECT(rc(d) == DFX_ERR_INVALID);
    d.dst_ld = 40;
    d.src_ld = 112;
    EXPECT(rc(d) == DFX_OK && lin_path(d) == DFX_LINEAR_TILE);
    d.force_path = DFX_LINEAR_GENERIC;
    EXPECT(rc(d) == DFX_OK && lin_path(d) == DFX_LINEAR_GENERIC);
  }
  // ---- auto: the tile kernel from the smallest measured rows, n, k, tile count and multiply-adds, on both sides of each bound
  {
    auto path = [](long long rows, int k, int n, long long src_ld) { return lin_path(desc(rows, k, n, src_ld, n)); };
    const int T = DFX_LINEAR_TILE, G = DFX_LINEAR_GENERIC;
    EXPECT(path(1576, 768, 2304, 768) == T && path(12608, 3072, 768, 3072) == T && path(9408, 96, 288, 96) == T && path(1700, 256, 256, 256) == T);
    EXPECT(path(1576, 768, 768, 768) == T && path(1575, 768, 768, 768) == G);          // rows
    EXPECT(path(9408, 256, 96, 256) == T && path(9408, 256, 95, 256) == G);            // n
    EXPECT(path(9408, 96, 288, 96) == T && path(9408, 95, 288, 96) == G);              // k
    EXPECT(path(3393, 512, 128, 512) == T && path(3392, 512, 128, 512) == G);          // 54 tiles of 64 x 128: 54 x 1 against 53 x 1
    EXPECT(path(1700, 256, 256, 256) == T && path(1699, 256, 256, 256) == G);          // 1700 * 256 * 256 multiply-adds
    EXPECT(path(3456, 96, 96, 96) == G && path(3456, 96, 336, 96) == T);               // (54 tiles, 0.29 of the multiply-adds; above them)
    EXPECT(path(1576, 768, 2304, 784) == T && path(1576, 768, 2304, 776) == G);        // the class
    EXPECT(path(1, 16, 1, 16) == G && lin_tile_auto(desc(1ll << 33, 65025, 96, 65040, 96)));
  }
  // ---- requant type and ReLU
  {
    dfx_linear_desc d = desc(4, 96, 40, 96, 40, DFX_S8, DFX_S8);
    EXPECT(lin_requant_dt(d) == DFX_S8 && !lin_relu(d));
    d.dst_dt = DFX_U8;
    EXPECT(lin_requant_dt(d) == DFX_U8 && lin_relu(d));
    d.lut_in_dt = DFX_S8;  // with a table the ReLU follows relu / lut_in_dt, not dst_dt
    EXPECT(lin_requant_dt(d) == DFX_S8 && !lin_relu(d));
    d.relu = 1;
    EXPECT(lin_relu(d));
    d.relu = 0; d.dst_dt = DFX_S8; d.lut_in_dt = DFX_U8;
    EXPECT(lin_requant_dt(d) == DFX_U8 && lin_relu(d));
  }
  // ---- tile height, tiles, grids, LDS
  {
    const dfx_linear_desc vit = desc(1576, 768, 2304, 768, 2304);  // ViT-B bs 8 QKV: 13 x 18 tiles of 128
    EXPECT(lin_tiles(vit, 128) == 13 * 18 && lin_tiles(vit, 64) == 25 * 18);
    EXPECT(lin_bm(vit, 256, 0) == 64 && lin_bm(vit, 234, 0) == 128 && lin_bm(vit, 235, 0) == 64);
    EXPECT(lin_bm(vit, 256, 128) == 128 && lin_bm(vit, 1, 64) == 64 && lin_bm(vit, 1, 96) == 128 && lin_bm(vit, 0, 0) == 128);
    EXPECT(lin_grid(vit, DFX_LINEAR_TILE, 64, 256, 0) == 450 && lin_grid(vit, DFX_LINEAR_TILE, 64, 100, 0) == 200);
    EXPECT(lin_grid(vit, DFX_LINEAR_TILE, 64, 256, 3) == 3 && lin_grid(vit, DFX_LINEAR_TILE, 64, 256, 1) == 1);
    EXPECT(lin_grid(vit, DFX_LINEAR_GENERIC, 64, 256, 0) == 4096 && lin_grid(vit, DFX_LINEAR_GENERIC, 64, 256, 7) == 7);
    EXPECT(lin_grid(desc(1, 1, 1, 1, 1), DFX_LINEAR_GENERIC, 64, 256, 0) == 1 && lin_grid(desc(1, 1, 1, 16, 1), DFX_LINEAR_TILE, 64, 256, 0) == 1);
    EXPECT(lin_tiles(desc(1ll << 33, 1, 1, 16, 1), 64) == (1ll << 27) && lin_grid(desc(1ll << 33, 1, 1, 16, 1), DFX_LINEAR_TILE, 64, 256, 0) == 512);
    EXPECT(lin_lds_bytes(DFX_LINEAR_TILE, 128) == 2 * (8192 + 8192) + 1536 + 256 && lin_lds_bytes(DFX_LINEAR_TILE, 64) == 2 * (4096 + 8192) + 1792);
    EXPECT(lin_lds_bytes(DFX_LINEAR_GENERIC, 128) == 0 && lin_lds_bytes(DFX_LINEAR_TILE, 128) <= 65536);
    EXPECT(lin_algorithmic_ops(vit) == 2ull * 1576 * 768 * 2304);
    EXPECT(lin_algorithmic_bytes(vit) == 1576ull * 768 + 2304ull * 768 + 1576ull * 2304 + 4);
    dfx_linear_desc f = desc(10, 20, 30, 32, 40, DFX_U8, DFX_F32);
    f.bia_dt = DFX_S8; f.nscales = 30;
    EXPECT(lin_algorithmic_bytes(f) == 10 * 20 + 30 * 20 + 10 * 30 * 4 + 4 * 30 + 4 * 30);
    f.dst_dt = DFX_U8; f.lut_in_dt = DFX_U8;
    EXPECT(lin_algorithmic_bytes(f) == 10 * 20 + 30 * 20 + 10 * 30 + 4 * 30 + 4 * 30 + 256);
    EXPECT(plan_extent(10, 32, 20, 1) == 9 * 32 + 20 && plan_extent(10, 40, 30, 4) == (9 * 40 + 30) * 4);
    EXPECT(plan_overlap(100, 10, 109, 1) && !plan_overlap(100, 10, 110, 1) && !plan_overlap(110, 1, 100, 10) && plan_overlap(105, 1, 100, 10));
    // the documented maximum, rows * ld = 2^40: extents (4-byte elements: 2^42 bytes), tiles, items and grids at full range
    EXPECT(plan_extent(1ll << 20, 1ll << 20, 1ll << 20, 4) == 1ull << 42 && plan_extent(1ll << 40, 1, 1, 4) == 1ull << 42);
    EXPECT(plan_extent(2, 1ll << 39, 40, 4) == ((1ull << 39) + 40) * 4 && plan_extent(1ll << 33, 128, 40, 1) == (1ull << 40) - 128 + 40);
    EXPECT(plan_extent(3, (1ll << 31) + 4160, 72, 1) == (1ull << 32) + 8320 + 72);  // (the pitches of tests/far_offsets.py)
    const uintptr_t far = (uintptr_t)1 << 47;  // an operand of 2^42 bytes against a neighbour on either side
    EXPECT(plan_overlap(far, 1ull << 42, far + (1ull << 42) - 1, 1) && !plan_overlap(far, 1ull << 42, far + (1ull << 42), 8) &&
           !plan_overlap(far, 1ull << 42, far - 8, 8) && plan_overlap(far, 1ull << 42, far - 8, 9) && plan_overlap(far + (1ull << 32) + 64, 408, far, (1ull << 32) + 8392));
    const dfx_linear_desc most = desc(1ll << 40, 1, 1, 1, 1), wide = desc(1ll << 33, 96, 128, 96, 128);
    EXPECT(rc(most) == DFX_OK && rc(wide) == DFX_OK);
    EXPECT(lin_mtiles(1ll << 40, 64) == 1ll << 34 && lin_mtiles(1ll << 40, 128) == 1ll << 33 && lin_mtiles((1ll << 40) - 1, 128) == 1ll << 33);
    EXPECT(lin_tiles(most, 64) == 1ll << 34 && lin_tiles(wide, 128) == 1ll << 26 && lin_items(most) == 1ll << 40 && lin_items(wide) == 1ll << 40);
    EXPECT(lin_grid(most, DFX_LINEAR_TILE, 64, 256, 0) == 512 && lin_grid(most, DFX_LINEAR_GENERIC, 64, 256, 0) == 4096 &&
           lin_grid(wide, DFX_LINEAR_GENERIC, 128, 256, 0) == 4096 && lin_grid(most, DFX_LINEAR_TILE, 64, 256, 1ll << 40) == 512);
    EXPECT(lin_algorithmic_ops(wide) == 2ull * 96 << 40 && lin_algorithmic_bytes(wide) == (96ull << 33) + 128 * 96 + (1ull << 40) + 4);
  }
  // ---- the image's sections
  for (int n : {1, 127, 128, 129, 264})
    for (int k : {1, 63, 64, 65, 200}) {
      const LinImage im = lin_image(n, k);
      const size_t nb = (size_t)(n + 127) / 128, ns = (size_t)(k + 63) / 64;
      EXPECT(lin_packed_bytes(n, k) == nb * ns * 8192 && im.off_comp == nb * ns * 8192);
      EXPECT(im.off_bias == im.off_comp + nb * 512 && im.off_scale == im.off_bias + nb * 512 && im.off_table == im.off_scale + nb * 512);
      EXPECT(im.bytes == im.off_table + 256 && im.off_comp % 16 == 0 && im.off_table % 16 == 0);
    }
  // ---- the packer: every weight at its documented place exactly once, zero pads, comp, bias, scale
  for (int n : {1, 3, 127, 129, 264})
    for (int k : {1, 15, 17, 63, 65, 136, 200}) {
      dfx_linear_desc d = desc(4, k, n, (k + 15) / 16 * 16, n, DFX_U8, DFX_S8);
      d.bia_dt = DFX_S8; d.nscales = n;
      std::vector<int8_t> w((size_t)n * k), bia(n);
      std::vector<float> sc(n);
      unsigned s = 12345u + (unsigned)(n * 1000 + k);
      for (auto &x : w) x = (int8_t)((s = s * 1664525u + 1013904223u) >> 24);
      for (int o = 0; o < n; ++o) {
        bia[o] = (int8_t)(o * 37 - 100);
        sc[o] = 0.001f * (float)(o + 1);
      }
      const LinImage im = lin_image(n, k);
      std::vector<unsigned char> img(im.bytes, 0xEE);
      EXPECT(lin_pack(d, w.data(), bia.data(), sc.data(), img.data()));
      std::vector<unsigned char> used(im.off_comp, 0);
      bool ok = true;
      for (int o = 0; o < n && ok; ++o) {
        long long sum = 0;
        for (int c = 0; c < k; ++c) {
          const size_t at = lin_wei_offset(o, c, k);
          ok = ok && at < im.off_comp && !used[at] && (int8_t)img[at] == w[(size_t)o * k + c];
          if (at < im.off_comp) used[at] = 1;
          sum += w[(size_t)o * k + c];
        }
        ok = ok && ((const int32_t *)(img.data() + im.off_comp))[o] == (int32_t)(128 * sum);
        ok = ok && ((const float *)(img.data() + im.off_bias))[o] == (float)bia[o] && ((const float *)(img.data() + im.off_scale))[o] == sc[o];
      }
      for (size_t i = 0; i < im.off_comp; ++i) ok = ok && (used[i] || img[i] == 0);
      const size_t consts = (im.off_bias - im.off_comp) / 4;
      for (size_t o = (size_t)n; o < consts; ++o)
        ok = ok && ((const int32_t *)(img.data() + im.off_comp))[o] == 0 && ((const int32_t *)(img.data() + im.off_bias))[o] == 0 &&
             ((const int32_t *)(img.data() + im.off_scale))[o] == 0;
      for (size_t i = im.off_table; i < im.bytes; ++i) ok = ok && img[i] == 0xEE;
      EXPECT(ok);
      std::vector<uint8_t> lut(256);
      for (int i = 0; i < 256; ++i) lut[i] = (uint8_t)(255 - i);
      lin_pack_table(d, lut.data(), img.data());
      EXPECT(!memcmp(img.data() + im.off_table, lut.data(), 256));
    }
  // the documented place, spelled out once: W[o = 128 nb + 32 f + r][c = 64 ks + 32 j + 16 h + b]
  EXPECT(lin_wei_offset(0, 0, 200) == 0 && lin_wei_offset(1, 0, 200) == 16 && lin_wei_offset(0, 16, 200) == 512 && lin_wei_offset(0, 32, 200) == 1024);
  EXPECT(lin_wei_offset(32, 0, 200) == 2048 && lin_wei_offset(0, 64, 200) == 8192 && lin_wei_offset(128, 0, 200) == 4 * 8192);
  EXPECT(lin_wei_offset(128 + 32 * 3 + 5, 64 * 2 + 32 + 16 + 7, 200) == (size_t)(4 + 2) * 8192 + ((3 * 2 + 1) * 64 + 32 + 5) * 16 + 7);
  // ---- the route's proof at its edge: one row, k = 1, the weight 64: B = 255 * 64 (u8) or 128 * 64 (s8)
  {
    const int8_t w = 64, wn = -64;
    std::vector<unsigned char> img(lin_image(1, 1).bytes);
    dfx_linear_desc d = desc(1, 1, 1, 16, 1, DFX_U8, DFX_S32);
    float s = 65536.0f;  // 2^16 * 2^14 = 2^30
    EXPECT(lin_acc_bound(DFX_U8, 64, 0) == 255.0 * 64 && lin_acc_bound(DFX_S8, 64, 0) == 128.0 * 64 && lin_acc_bound(DFX_S8, 3, 5) == 128.0 * 8);
    EXPECT(lin_acc_bound(DFX_U8, 3, 5) == 255.0 * 5);
    const int8_t w65 = 65;
    EXPECT(lin_pack(d, &w, nullptr, &s, img.data()) && !lin_pack(d, &w65, nullptr, &s, img.data()));  // 255 * 64 * 2^16 < 2^30 < 255 * 65 * 2^16
    d.src_dt = DFX_S8;
    s = 131072.0f;  // 128 * 64 * 2^17 = 2^30: the last scale admitted
    EXPECT(!lin_pack(d, &w65, nullptr, &s, img.data()));
    EXPECT(lin_pack(d, &w, nullptr, &s, img.data()) && lin_pack(d, &wn, nullptr, &s, img.data()));
    s = 131072.0f * 1.0000002f;
    EXPECT(s > 131072.0f && !lin_pack(d, &w, nullptr, &s, img.data()));
    s = 131072.0f;
    d.bia_dt = DFX_F32;
    float b = 1.0f;
    EXPECT(!lin_pack(d, &w, &b, &s, img.data()));
    b = 0.0f;
    EXPECT(lin_pack(d, &w, &b, &s, img.data()));
    for (unsigned bits : {0x7f800000u, 0xff800000u, 0x7fc00000u}) {
      float x;
      memcpy(&x, &bits, 4);
      float one = 1.0f, zero = 0.0f;
      EXPECT(!lin_pack(d, &w, &zero, &x, img.data()) && !lin_pack(d, &w, &x, &one, img.data()));
    }
  }
  if (g_bad) {
    printf("linear_plan_check: %d check(s) FAILED\n", g_bad);
    return 1;
  }
  printf("linear plans: validation order, classes, tile heights, grids, LDS, image sections, the packer and the route's proof hold\n");
  return 0;
}
