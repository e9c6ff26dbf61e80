// patchembed_plan_check -- host-only check of csrc/patchembed_plan.h and csrc/patchembed_pack.h, what the int8 patch-embedding
// op (dfx_patchembed_*) decides before a kernel runs: the order of the descriptor's validation (every DFX_ERR_INVALID before
// the one DFX_ERR_UNSUPPORTED) at the last admitted and the first refused value of every bound, the granule of the tile class,
// the auto rule, the GEMM handed to linear_plan.h, the image's sections, the K offset table against the bytes of an image, the
// weight permutation, the table's scan and padding, and the route's proof at its edge with a bias and with a table.  No HIP: it
// builds with SAN=1 (ASan + UBSan) and runs anywhere.
//   patchembed_plan_check
//   patchembed_plan_check plan <bs> <ih> <iw> <ic> <ph> <pw> <th> <tw> <oc> <table> <t0> <cus> <forced_bm> <cap> <weights.bin> <image.bin>
//     prints the plan of the descriptor (u8 in, s8 out, forced tile path) as "key value" lines and writes the image that
//     pe_pack makes of the oihw weight bytes in weights.bin (no bias, scale 1; with a table: every entry 0.5, and the table
//     section behind it): tests/test_patchembed_cpu.py compares both with its Python mirror
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../csrc/patchembed_pack.h"
#include "../csrc/patchembed_plan.h"

using namespace dfx;

static int g_bad = 0;
#define EXPECT(cond)                                                     \
  do {                                                                   \
    if (!(cond)) {                                                       \
      printf("patchembed_plan_check: line %d: %s\n", __LINE__, #cond);   \
      ++g_bad;                                                           \
    }                                                                    \
  } while (0)

static dfx_patchembed_desc desc(int bs, int ih, int iw, int ic, int ph, int pw, int oc) {
  dfx_patchembed_desc d;
  memset(&d, 0, sizeof(d));
  d.bs = bs; d.ih = ih; d.iw = iw; d.ic = ic; d.ph = ph; d.pw = pw; d.th = ih / (ph > 0 ? ph : 1); d.tw = iw / (pw > 0 ? pw : 1); d.oc = oc;
  d.src_dt = DFX_U8; d.dst_dt = DFX_S8; d.bia_dt = DFX_UNDEF; d.relu = 0; d.round_mode = DFX_ROUND_NEAREST; d.nscales = 1;
  d.table = 0; d.tok_offset = 0; d.force_path = -1;
  d.img_rows = (long long)d.th * d.tw; d.dst_ld = oc;
  return d;
}
static int rc(const dfx_patchembed_desc &d) {
  const char *why = nullptr;
  const int r = pe_validate(d, &why);
  EXPECT(why != nullptr && (r == DFX_OK) == (why[0] == 0));
  EXPECT(pe_validate(d, nullptr) == r);
  return r;
}

static int plan_mode(char **v) {
  dfx_patchembed_desc d = desc(atoi(v[0]), atoi(v[1]), atoi(v[2]), atoi(v[3]), atoi(v[4]), atoi(v[5]), atoi(v[8]));
  d.th = atoi(v[6]); d.tw = atoi(v[7]); d.table = atoi(v[9]); d.tok_offset = atoi(v[10]);
  d.img_rows = d.tok_offset + pe_tokens(d);
  d.force_path = DFX_PATCHEMBED_TILE;
  const int cus = atoi(v[11]), forced = atoi(v[12]);
  const long long cap = atoll(v[13]);
  const int r = pe_validate(d, nullptr);
  printf("validate %d\n", r);
  if (r) return 0;
  const int bm = pe_bm(d, cus, forced);
  const PeImage im = pe_image(d);
  printf("path %d\ngranule %d\nbm %d\ntiles %lld\ngrid_tile %d\ngrid_generic %d\nlds %d\n", pe_path(d), pe_granule(d), bm, lin_tiles(pe_gemm(d, false), bm),
         pe_grid(d, DFX_PATCHEMBED_TILE, bm, cus, cap), pe_grid(d, DFX_PATCHEMBED_GENERIC, bm, cus, cap), pe_lds_bytes(DFX_PATCHEMBED_TILE, bm));
  printf("off_comp %zu\noff_bias %zu\noff_scale %zu\noff_ktab %zu\noff_table %zu\noff_prefix %zu\nbytes %zu\n", im.lin.off_comp, im.lin.off_bias, im.lin.off_scale,
         im.off_ktab, im.off_table, im.off_prefix, im.bytes);
  std::vector<int8_t> w((size_t)d.oc * pe_k(d)), wp(w.size());
  FILE *f = fopen(v[14], "rb");
  if (!f || fread(w.data(), 1, w.size(), f) != w.size()) {
    printf("patchembed_plan_check: cannot read %s\n", v[14]);
    if (f) fclose(f);
    return 1;
  }
  fclose(f);
  pe_permute(d, w.data(), wp.data());
  std::vector<unsigned char> img(im.bytes, 0xEE);
  std::vector<float> table((size_t)pe_tokens(d) * d.oc, 0.5f), tmax((size_t)d.oc);
  const float one = 1.0f;
  if (d.table) {
    if (!pe_scan_table(d, table.data(), d.oc, tmax.data())) return 1;
    pe_pack_table(d, table.data(), d.oc, (float *)(img.data() + im.off_table));
  }
  printf("fast %d\n", (int)pe_pack(d, wp.data(), nullptr, &one, d.table ? tmax.data() : nullptr, img.data()));
  for (size_t i = im.off_prefix; i < im.bytes; ++i)
    if (img[i] != 0xEE) {
      printf("patchembed_plan_check: the packers wrote into the prefix section\n");
      return 1;
    }
  f = fopen(v[15], "wb");
  if (!f || fwrite(img.data(), 1, im.off_prefix, f) != im.off_prefix) {
    printf("patchembed_plan_check: cannot write %s\n", v[15]);
    if (f) fclose(f);
    return 1;
  }
  fclose(f);
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 18 && !strcmp(argv[1], "plan")) return plan_mode(argv + 2);
  if (argc != 1) {
    printf("usage: patchembed_plan_check | patchembed_plan_check plan <bs> <ih> <iw> <ic> <ph> <pw> <th> <tw> <oc> <table> <t0> <cus> <forced_bm> <cap> "
           "<weights.bin> <image.bin>\n");
    return 2;
  }
  // ---- validation, each bound at its last admitted and first refused value
  EXPECT(rc(desc(1, 1, 1, 1, 1, 1, 1)) == DFX_OK);
  EXPECT(rc(desc(0, 8, 8, 3, 4, 4, 8)) == DFX_ERR_INVALID && rc(desc(1, 8, 8, 0, 4, 4, 8)) == DFX_ERR_INVALID);
  EXPECT(rc(desc(1, 0, 8, 3, 4, 4, 8)) == DFX_ERR_INVALID && rc(desc(1, 8, 0, 3, 4, 4, 8)) == DFX_ERR_INVALID);
  EXPECT(rc(desc(1, 255, 8, 1, 255, 4, 8)) == DFX_OK && rc(desc(1, 256, 8, 1, 256, 4, 8)) == DFX_ERR_INVALID && rc(desc(1, 8, 8, 1, 0, 4, 8)) == DFX_ERR_INVALID);
  EXPECT(rc(desc(1, 8, 255, 1, 4, 255, 8)) == DFX_OK && rc(desc(1, 8, 256, 1, 4, 256, 8)) == DFX_ERR_INVALID && rc(desc(1, 8, 8, 1, 4, 0, 8)) == DFX_ERR_INVALID);
  EXPECT(rc(desc(1, 255, 255, 1, 255, 255, 8)) == DFX_OK && pe_k(desc(1, 255, 255, 1, 255, 255, 8)) == LIN_KMAX);
  EXPECT(rc(desc(1, 255, 128, 2, 255, 128, 8)) == DFX_ERR_INVALID && rc(desc(1, 127, 128, 4, 127, 128, 8)) == DFX_OK);
  EXPECT(rc(desc(1, 8, 8, 3, 4, 4, 0)) == DFX_ERR_INVALID && rc(desc(1, 8, 8, 3, 4, 4, LIN_NMAX)) == DFX_OK);
  {
    dfx_patchembed_desc d = desc(2, 9, 11, 3, 4, 4, 8);  // floors: th <= 2, tw <= 2
    EXPECT(d.th == 2 && d.tw == 2 && rc(d) == DFX_OK);
    d.th = 3; EXPECT(rc(d) == DFX_ERR_INVALID);
    d.th = 0; EXPECT(rc(d) == DFX_ERR_INVALID);
    d.th = 1; d.img_rows = 2; EXPECT(rc(d) == DFX_OK);
    d.tw = 3; d.img_rows = 3; EXPECT(rc(d) == DFX_ERR_INVALID);
    d.tw = 0; EXPECT(rc(d) == DFX_ERR_INVALID);
  }
  {
    dfx_patchembed_desc d = desc(2, 8, 8, 4, 4, 4, 40);
    for (int dt = -1; dt <= 5; ++dt) {
      d.src_dt = dt; EXPECT(rc(d) == ((dt == DFX_U8 || dt == DFX_S8) ? DFX_OK : DFX_ERR_INVALID));
    }
    d.src_dt = DFX_S8;
    for (int dt = -1; dt <= 5; ++dt) {
      d.dst_dt = dt; EXPECT(rc(d) == ((dt >= 1 && dt <= 4) ? DFX_OK : DFX_ERR_INVALID));
    }
    d.dst_dt = DFX_F32;
    for (int dt = -1; dt <= 5; ++dt) {
      d.bia_dt = dt; EXPECT(rc(d) == ((dt >= 0 && dt <= 4) ? DFX_OK : DFX_ERR_INVALID));
    }
    d.bia_dt = DFX_UNDEF;
    d.round_mode = 2; EXPECT(rc(d) == DFX_ERR_INVALID); d.round_mode = DFX_ROUND_DOWN; EXPECT(rc(d) == DFX_OK);
    d.nscales = 2; EXPECT(rc(d) == DFX_ERR_INVALID); d.nscales = 40; EXPECT(rc(d) == DFX_OK);
    d.table = 2; EXPECT(rc(d) == DFX_ERR_INVALID); d.table = -1; EXPECT(rc(d) == DFX_ERR_INVALID); d.table = 1; EXPECT(rc(d) == DFX_OK);
    d.bia_dt = DFX_S32; EXPECT(rc(d) == DFX_ERR_INVALID); d.bia_dt = DFX_UNDEF;
    d.tok_offset = -1; EXPECT(rc(d) == DFX_ERR_INVALID);
    d.tok_offset = 2; EXPECT(rc(d) == DFX_ERR_INVALID);  // img_rows is 4
    d.img_rows = 6; EXPECT(rc(d) == DFX_OK); d.img_rows = 5; EXPECT(rc(d) == DFX_ERR_INVALID); d.img_rows = 9; EXPECT(rc(d) == DFX_OK);
    d.dst_ld = 39; EXPECT(rc(d) == DFX_ERR_INVALID); d.dst_ld = 41; EXPECT(rc(d) == DFX_OK);
    d.force_path = 2; EXPECT(rc(d) == DFX_ERR_INVALID); d.force_path = -2; EXPECT(rc(d) == DFX_ERR_INVALID);
    d.force_path = DFX_PATCHEMBED_TILE; EXPECT(rc(d) == DFX_OK); d.force_path = DFX_PATCHEMBED_GENERIC; EXPECT(rc(d) == DFX_OK);
    // the 2^40 limits
    d = desc(1 << 20, 1 << 10, 1 << 8, 4, 4, 4, 8); d.th = d.tw = 1; d.img_rows = 1; EXPECT(rc(d) == DFX_OK);          // 2^40 bytes
    d.ih += 1; EXPECT(rc(d) == DFX_ERR_INVALID);
    d = desc(1 << 20, 8, 8, 4, 4, 4, 8); d.img_rows = 1 << 10; d.dst_ld = 1 << 10; EXPECT(rc(d) == DFX_OK);             // 2^40 elements
    d.dst_ld += 1; EXPECT(rc(d) == DFX_ERR_INVALID);
    // ph * iw * ic below 2^31
    d = desc(1, 128, 1 << 22, 4, 128, 4, 8); d.tw = 1; d.img_rows = 1; EXPECT(rc(d) == DFX_ERR_INVALID);                // 128 * 2^24 = 2^31
    d = desc(1, 127, 1 << 22, 4, 127, 4, 8); d.tw = 1; d.img_rows = 1; EXPECT(rc(d) == DFX_OK);
    // the table image's cap: th * tw * up4(oc) * 4 <= 2^30
    d = desc(1, 1 << 10, 1 << 10, 1, 1, 1, 256); d.table = 1; EXPECT(rc(d) == DFX_OK);
    d.oc = 257; d.dst_ld = 257; EXPECT(rc(d) == DFX_ERR_INVALID); d.table = 0; EXPECT(rc(d) == DFX_OK);
  }
  // ---- the class, and the one unsupported case behind everything invalid
  EXPECT(pe_granule(desc(1, 32, 32, 3, 16, 16, 8)) == 16 && pe_granule(desc(1, 8, 8, 3, 4, 4, 8)) == 4 && pe_granule(desc(1, 28, 28, 3, 14, 14, 8)) == 0);
  EXPECT(pe_granule(desc(1, 8, 8, 4, 1, 4, 8)) == 16 && pe_granule(desc(1, 8, 9, 4, 1, 4, 8)) == 4 && pe_granule(desc(1, 4, 4, 8, 2, 2, 8)) == 16);
  EXPECT(pe_granule(desc(1, 4, 5, 8, 2, 2, 8)) == 4 && pe_granule(desc(1, 4, 5, 3, 2, 4, 8)) == 0 && pe_granule(desc(1, 4, 5, 2, 2, 2, 8)) == 0);
  {
    dfx_patchembed_desc d = desc(1, 28, 28, 3, 14, 14, 8);
    EXPECT(rc(d) == DFX_OK && pe_path(d) == DFX_PATCHEMBED_GENERIC);
    d.force_path = DFX_PATCHEMBED_GENERIC; EXPECT(rc(d) == DFX_OK);
    d.force_path = DFX_PATCHEMBED_TILE; EXPECT(rc(d) == DFX_ERR_UNSUPPORTED);
    d.dst_ld = 7; EXPECT(rc(d) == DFX_ERR_INVALID); d.dst_ld = 8;
    d.nscales = 3; EXPECT(rc(d) == DFX_ERR_INVALID);
  }
  // ---- the auto rule on both sides of each bound: rows 49, oc 96, K 48, 3136 * 96 * 48 multiply-adds, the class
  {
    auto tokens = [](int rows, int ic, int oc) {  // one image of `rows` patches of 1 x 4 x ic: K = 4 * ic, granule 16 where ic % 4 == 0
      dfx_patchembed_desc d = desc(1, 1, 4 * rows, ic, 1, 4, oc);
      return d;
    };
    EXPECT(pe_path(tokens(12544, 12, 96)) == DFX_PATCHEMBED_TILE && pe_path(tokens(12544, 12, 95)) == DFX_PATCHEMBED_GENERIC);   // oc
    EXPECT(pe_path(tokens(12544, 8, 96)) == DFX_PATCHEMBED_GENERIC);                                                              // K 32
    EXPECT(pe_path(tokens(49, 768, 768)) == DFX_PATCHEMBED_TILE && pe_path(tokens(48, 768, 768)) == DFX_PATCHEMBED_GENERIC);      // rows
    EXPECT(pe_path(tokens(3136, 12, 96)) == DFX_PATCHEMBED_TILE && pe_path(tokens(3135, 12, 96)) == DFX_PATCHEMBED_GENERIC);      // multiply-adds
    EXPECT(pe_path(tokens(12544, 13, 768)) == DFX_PATCHEMBED_TILE && pe_granule(tokens(12544, 13, 768)) == 4);                    // K 52, granule 4
    EXPECT(pe_path(desc(8, 224, 224, 3, 14, 14, 768)) == DFX_PATCHEMBED_GENERIC);                                                 // outside the class
  }
  for (int bs : {1, 64}) {
    dfx_patchembed_desc d = desc(bs, 224, 224, 3, 16, 16, 768);
    EXPECT(pe_path(d) == DFX_PATCHEMBED_TILE && pe_tile_auto(d));
    d.force_path = DFX_PATCHEMBED_GENERIC; EXPECT(pe_path(d) == DFX_PATCHEMBED_GENERIC);
  }
  // ---- the GEMM, tile height, grids, LDS
  {
    const dfx_patchembed_desc d = desc(8, 224, 224, 3, 16, 16, 768);
    const dfx_linear_desc g = pe_gemm(d, false);
    EXPECT(g.rows == 8 * 196 && g.k == 768 && g.n == 768 && g.src_ld == 768 && g.dst_ld == 768 && g.lut_in_dt == DFX_UNDEF && g.bia_dt == DFX_UNDEF);
    EXPECT(pe_gemm(d, true).bia_dt == DFX_F32);
    EXPECT(pe_bm(d, 256, 0) == 64 && pe_bm(d, 64, 0) == 128 && pe_bm(d, 256, 128) == 128 && pe_bm(d, 64, 64) == 64);
    EXPECT(pe_grid(d, DFX_PATCHEMBED_TILE, 64, 256, 0) == 25 * 6 && pe_grid(d, DFX_PATCHEMBED_TILE, 64, 256, 3) == 3 && pe_grid(d, DFX_PATCHEMBED_TILE, 64, 8, 0) == 16);
    EXPECT(pe_grid(d, DFX_PATCHEMBED_GENERIC, 64, 256, 0) == 4096);
    EXPECT(pe_lds_bytes(DFX_PATCHEMBED_TILE, 128) == 2 * (128 * 64 + 8192) + 1536 && pe_lds_bytes(DFX_PATCHEMBED_TILE, 64) == 2 * (64 * 64 + 8192) + 1536);
    EXPECT(pe_lds_bytes(DFX_PATCHEMBED_GENERIC, 128) == 0 && pe_lds_bytes(DFX_PATCHEMBED_TILE, 128) <= 65536);
    EXPECT(pe_algorithmic_ops(d) == 2ull * 8 * 196 * 768 * 768);
  }
  // ---- the K offset table against an image's bytes: gathering through it gives the patch in (ky, kx, i) order
  for (int geo = 0; geo < 4; ++geo) {
    const int ph = geo == 0 ? 3 : geo == 1 ? 4 : geo == 2 ? 2 : 5, pw = geo == 0 ? 16 : geo == 1 ? 4 : geo == 2 ? 2 : 4, ic = geo == 0 ? 3 : geo == 1 ? 3 : geo == 2 ? 32 : 4;
    dfx_patchembed_desc d = desc(2, 3 * ph + 1, 4 * pw + (geo == 3 ? 1 : 0), ic, ph, pw, 5);
    const int g = pe_granule(d), k = pe_k(d);
    EXPECT(g == (geo == 1 || geo == 3 ? 4 : 16) && rc(d) == DFX_OK);
    std::vector<int32_t> tab(pe_ktab_entries(d) + 1, -7);
    pe_fill_ktab(d, tab.data());
    EXPECT(tab.back() == -7 && pe_ktab_entries(d) == (size_t)lin_nslabs(k) * (64 / g));
    std::vector<unsigned char> img((size_t)d.bs * d.ih * d.iw * d.ic);
    for (size_t i = 0; i < img.size(); ++i) img[i] = (unsigned char)(i * 131 + i / 253);
    for (int b = 0; b < d.bs; ++b)
      for (int ty = 0; ty < d.th; ++ty)
        for (int tx = 0; tx < d.tw; ++tx) {
          const size_t base = (((size_t)b * d.ih + (size_t)ty * ph) * d.iw + (size_t)tx * pw) * ic;
          for (int c = 0; c < k; ++c) {
            const int ky = c / (pw * ic), kx = c % (pw * ic) / ic, i = c % ic;
            const size_t direct = (((size_t)b * d.ih + ty * ph + ky) * d.iw + tx * pw + kx) * ic + i;
            const size_t via = base + (size_t)tab[c / g] + (size_t)(c % g);
            if (via != direct || via >= img.size()) { EXPECT(via == direct); break; }
          }
        }
    for (size_t e = (size_t)(k + g - 1) / g; e < pe_ktab_entries(d); ++e) EXPECT(tab[e] == 0);
  }
  // ---- the permutation, the image through lin_wei_offset, comp, the table's scan and padding, the proof at its edge
  {
    dfx_patchembed_desc d = desc(1, 8, 8, 3, 4, 4, 130);
    d.table = 1; d.src_dt = DFX_U8;
    const int k = pe_k(d);
    std::vector<int8_t> w((size_t)d.oc * k), wp(w.size());
    for (size_t i = 0; i < w.size(); ++i) w[i] = (int8_t)((i * 37 + i / 101) % 255 - 127);
    pe_permute(d, w.data(), wp.data());
    for (int o = 0; o < d.oc; o += 43)
      for (int i = 0; i < 3; ++i)
        for (int ky = 0; ky < 4; ++ky)
          for (int kx = 0; kx < 4; ++kx) EXPECT(wp[(size_t)o * k + (ky * 4 + kx) * 3 + i] == w[(((size_t)o * 3 + i) * 4 + ky) * 4 + kx]);
    const PeImage im = pe_image(d);
    EXPECT(im.off_ktab == im.lin.off_table && im.off_table == im.off_ktab + 16 * 4 - 16 + 16 && im.off_prefix == im.off_table + 4 * 132 * 4 && im.bytes == im.off_prefix);
    EXPECT(im.off_ktab % 16 == 0 && im.off_table % 16 == 0 && im.off_prefix % 16 == 0);
    std::vector<unsigned char> img(im.bytes, 0xEE);
    std::vector<float> table((size_t)4 * 140), tmax((size_t)d.oc, -1.0f), scales(1, 1.0f);
    for (size_t i = 0; i < table.size(); ++i) table[i] = (float)((int)(i % 17) - 8);
    EXPECT(pe_scan_table(d, table.data(), 140, tmax.data()));
    for (int o = 0; o < d.oc; ++o) {
      float m = 0;
      for (int t = 0; t < 4; ++t) m = fmaxf(m, fabsf(table[(size_t)t * 140 + o]));
      EXPECT(tmax[o] == m);
    }
    pe_pack_table(d, table.data(), 140, (float *)(img.data() + im.off_table));
    const float *tp = (const float *)(img.data() + im.off_table);
    for (int t = 0; t < 4; ++t) {
      for (int o = 0; o < d.oc; ++o) EXPECT(tp[t * 132 + o] == table[(size_t)t * 140 + o]);
      EXPECT(tp[t * 132 + 130] == 0.0f && tp[t * 132 + 131] == 0.0f);
    }
    EXPECT(pe_pack(d, wp.data(), nullptr, scales.data(), tmax.data(), img.data()));
    for (int o = 0; o < d.oc; o += 7)
      for (int c = 0; c < k; c += 5) EXPECT((int8_t)img[lin_wei_offset(o, c, k)] == wp[(size_t)o * k + c]);
    const int32_t *comp = (const int32_t *)(img.data() + im.lin.off_comp);
    const float *bias = (const float *)(img.data() + im.lin.off_bias);
    for (int o = 0; o < d.oc; ++o) {
      long long s = 0;
      for (int c = 0; c < k; ++c) s += wp[(size_t)o * k + c];
      EXPECT(comp[o] == 128 * s && bias[o] == 0.0f);  // the table's maximum served the proof only
    }
    table[3] = std::numeric_limits<float>::infinity();
    EXPECT(!pe_scan_table(d, table.data(), 140, tmax.data()));
    table[3] = std::numeric_limits<float>::quiet_NaN();
    EXPECT(!pe_scan_table(d, table.data(), 140, tmax.data()));
  }
  {
    // one channel of 48 weights of 127: B = 255 * 48 * 127 = 1554480; with scale 512 the proof holds up to |add| = 2^21 - B
    dfx_patchembed_desc d = desc(1, 4, 4, 3, 4, 4, 1);
    std::vector<int8_t> wp(48, 127);
    const PeImage im = pe_image(d);
    std::vector<unsigned char> img(im.bytes);
    const float scale = 512.0f, edge = 2097152.0f - 1554480.0f;
    float b = edge;
    d.bia_dt = DFX_F32;
    EXPECT(pe_pack(d, wp.data(), &b, &scale, nullptr, img.data()));
    b = edge + 1.0f; EXPECT(!pe_pack(d, wp.data(), &b, &scale, nullptr, img.data()));
    b = -edge; EXPECT(pe_pack(d, wp.data(), &b, &scale, nullptr, img.data()));
    d.bia_dt = DFX_UNDEF; d.table = 1;
    const PeImage imt = pe_image(d);
    img.assign(imt.bytes, 0);
    float t = edge;
    EXPECT(pe_pack(d, wp.data(), nullptr, &scale, &t, img.data()));
    t = edge + 1.0f; EXPECT(!pe_pack(d, wp.data(), nullptr, &scale, &t, img.data()));
    EXPECT(pe_pack(d, wp.data(), nullptr, &scale, nullptr, img.data()));  // no table yet: proved as if it were 0
    const float inf = std::numeric_limits<float>::infinity();
    EXPECT(!pe_pack(d, wp.data(), nullptr, &inf, nullptr, img.data()));
    d.src_dt = DFX_S8;  // B = 128 * 48 * 127 = 780288
    t = 2097152.0f - 780288.0f; EXPECT(pe_pack(d, wp.data(), nullptr, &scale, &t, img.data()));
    t += 1.0f; EXPECT(!pe_pack(d, wp.data(), nullptr, &scale, &t, img.data()));
  }
  // ---- extents
  {
    dfx_patchembed_desc d = desc(2, 8, 8, 4, 4, 4, 10);
    d.tok_offset = 1; d.img_rows = 7; d.dst_ld = 12; d.dst_dt = DFX_S32;
    EXPECT(rc(d) == DFX_OK && pe_src_extent(d) == 2 * 8 * 8 * 4 && pe_dst_extent(d) == ((7 + 1 + 4 - 1) * 12 + 10) * 4ull);
    EXPECT(pe_image(d).bytes == pe_image(d).off_prefix + 48);
    // the documented maxima: bs * ih * iw * ic = 2^40 and bs * img_rows * dst_ld = 2^40 with 4-byte elements; rows, tiles and grids
    d = desc(1 << 16, 4096, 4096, 1, 4, 4, 8);
    d.dst_dt = DFX_F32; d.img_rows = 1 << 20; d.dst_ld = 16;
    EXPECT(rc(d) == DFX_OK && pe_src_extent(d) == 1ull << 40 && pe_rows(d) == 1ll << 36);
    EXPECT(pe_dst_extent(d) == ((((1ull << 16) - 1) * (1ull << 20) + (1ull << 20) - 1) * 16 + 8) * 4);
    EXPECT(pe_grid(d, DFX_PATCHEMBED_TILE, 64, 256, 0) == 512 && pe_grid(d, DFX_PATCHEMBED_GENERIC, 64, 256, 0) == 4096);
    EXPECT(lin_tiles(pe_gemm(d, false), 64) == 1ll << 30 && lin_items(pe_gemm(d, false)) == 1ll << 39);
    d.bs += 1; EXPECT(rc(d) == DFX_ERR_INVALID);
    // the shapes of tests/far_offsets.py: 258 images of 2^24 bytes; three images whose rows lie 2^31 + 4160 bytes apart
    d = desc(258, 2048, 2048, 4, 4, 4, 40); d.th = d.tw = 2; d.img_rows = 4; d.dst_ld = 40;
    EXPECT(rc(d) == DFX_OK && pe_src_extent(d) == 258ull << 24 && pe_granule(d) == 16);
    d = desc(3, 8, 8, 4, 4, 4, 40); d.tok_offset = 2; d.dst_ld = 64; d.img_rows = ((1ll << 31) + 4160) / 64;
    EXPECT(rc(d) == DFX_OK && pe_dst_extent(d) == (2 * d.img_rows + 5) * 64ull + 40);
  }
  if (g_bad) {
    printf("patchembed_plan_check: %d check(s) failed\n", g_bad);
    return 1;
  }
  printf("patchembed plans: validation order, granules, the auto rule, tile heights, grids, LDS, image sections, the K offset table, the packer and the route's proof hold\n");
  return 0;
}
