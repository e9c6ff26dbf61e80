// wsum_plan_check -- host-only check of the scaled element-wise sum's plan (csrc/wsum_plan.h): the descriptor validation
// and its codes, the layout of the constants the vec kernel stages in LDS, the aliasing classification and the grid.
// No GPU, no HIP.  Built plainly as part of `all`; `make -B ../tools/wsum_plan_check SAN=1` builds it under
// AddressSanitizer / UBSan.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../csrc/wsum_plan.h"

using namespace dfx;

static int failures = 0;
#define CHECK(cond)                                                \
  do {                                                             \
    if (!(cond)) {                                                 \
      printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);       \
      ++failures;                                                  \
    }                                                              \
  } while (0)

static dfx_wsum_desc base() {
  dfx_wsum_desc d;
  memset(&d, 0, sizeof(d));
  d.bs = 2; d.h = 5; d.w = 7; d.c = 32;
  d.n_inputs = 2;
  d.src_dt[0] = DFX_U8; d.src_dt[1] = DFX_S32;
  d.nscales[0] = 1; d.nscales[1] = 32;
  d.dst_dt = DFX_U8;
  d.force_path = -1;
  return d;
}

static void check_validation() {
  const char *why = nullptr;
  dfx_wsum_desc d = base();
  CHECK(wsum_validate(d, &why) == DFX_OK);
  CHECK(wsum_validate(d, nullptr) == DFX_OK);
  d = base(); d.n_inputs = 0; CHECK(wsum_validate(d, &why) == DFX_ERR_INVALID);
  d = base(); d.n_inputs = 9; CHECK(wsum_validate(d, &why) == DFX_ERR_INVALID);
  d = base(); d.src_dt[1] = DFX_UNDEF; CHECK(wsum_validate(d, &why) == DFX_ERR_INVALID);
  d = base(); d.src_dt[5] = 77; CHECK(wsum_validate(d, &why) == DFX_OK);  // entries from n_inputs on are ignored
  d = base(); d.nscales[1] = 16; CHECK(wsum_validate(d, &why) == DFX_ERR_INVALID);
  d = base(); d.n_bias = 2; CHECK(wsum_validate(d, &why) == DFX_ERR_INVALID);
  d = base(); d.n_bias = 32; CHECK(wsum_validate(d, &why) == DFX_OK);
  d = base(); d.dst_dt = DFX_S32; CHECK(wsum_validate(d, &why) == DFX_ERR_UNSUPPORTED);
  d = base(); d.dst_dt = DFX_S32; d.round_mode = 5; CHECK(wsum_validate(d, &why) == DFX_ERR_INVALID);  // invalid comes first
  d = base(); d.dst_dt = DFX_F32; d.lut_in_dt = DFX_S8; CHECK(wsum_validate(d, &why) == DFX_ERR_INVALID);
  d = base(); d.lut_in_dt = DFX_F32; CHECK(wsum_validate(d, &why) == DFX_ERR_INVALID);
  d = base(); d.force_path = 2; CHECK(wsum_validate(d, &why) == DFX_ERR_INVALID);
  // the caps, at the last admitted and the first refused value; nothing overflows on the way (UBSan watches)
  d = base(); d.bs = 1; d.h = 32768; d.w = 65535; d.c = 1; d.nscales[1] = 1; CHECK(wsum_validate(d, &why) == DFX_OK);
  d.w = 65536; CHECK(wsum_validate(d, &why) == DFX_ERR_INVALID);
  d.w = 65535; d.bs = 512; CHECK(wsum_validate(d, &why) == DFX_OK);
  CHECK(wsum_elems(d) == 512ll * 32768 * 65535);
  d.bs = 513; CHECK(wsum_validate(d, &why) == DFX_ERR_INVALID);
  d = base(); d.bs = d.h = d.w = d.c = 2147483647; d.nscales[1] = d.c; CHECK(wsum_validate(d, &why) == DFX_ERR_INVALID);
  d = base(); d.h = 2147483647; d.w = 2147483647; d.c = 1; d.nscales[1] = 1; CHECK(wsum_validate(d, &why) == DFX_ERR_INVALID);
}

static void check_image() {
  // every slot is read by the kernel as c floats from slot * c: slots must not overlap, must lie inside the image, and
  // the table must follow them
  const int cs[] = {1, 16, 17, 48, 72, 256, 2048};
  for (int c : cs)
    for (int mask = 0; mask < 256; mask += 37)
      for (int nb = 0; nb < 3; ++nb)
        for (int lut = 0; lut < 2; ++lut) {
          dfx_wsum_desc d = base();
          d.c = c; d.n_inputs = 8;
          for (int i = 0; i < 8; ++i) { d.src_dt[i] = DFX_S8; d.nscales[i] = (mask >> i & 1) ? c : 1; }
          d.n_bias = nb == 0 ? 0 : nb == 1 ? 1 : c;
          d.lut_in_dt = lut ? DFX_S8 : DFX_UNDEF;
          CHECK(wsum_validate(d, nullptr) == DFX_OK);
          const WsumImage m = wsum_image(d);
          std::vector<int> owner((size_t)m.bytes, -1);
          int want = 0;
          for (int i = 0; i <= 8; ++i) {
            const int s = i < 8 ? m.slot[i] : m.bias_slot;
            const bool per_channel = c > 1 && (i < 8 ? d.nscales[i] == c : d.n_bias == c);
            CHECK((s >= 0) == per_channel);
            if (s < 0) continue;
            CHECK(s == want);
            ++want;
            for (long long b = (long long)s * c * 4; b < (long long)(s + 1) * c * 4; ++b) {
              CHECK(b < m.bytes && owner[(size_t)b] == -1);
              owner[(size_t)b] = i;
            }
          }
          CHECK(m.slots == want);
          CHECK(m.bytes % 16 == 0);
          if (lut) {
            CHECK(m.lut_off >= (long long)m.slots * c * 4 && m.lut_off % 16 == 0 && m.lut_off + 256 == m.bytes);
          } else {
            CHECK(m.lut_off == -1);
          }
          CHECK(wsum_vec_class(d) == (c % 16 == 0 && m.bytes <= WSUM_MAX_LDS));
        }
  dfx_wsum_desc d = base();
  d.c = 2048; d.n_inputs = 8;
  for (int i = 0; i < 8; ++i) { d.src_dt[i] = DFX_U8; d.nscales[i] = 2048; }
  CHECK(wsum_vec_class(d));                      // 8 * 2048 * 4 = 64 KiB exactly
  d.n_bias = 2048; CHECK(!wsum_vec_class(d));
  d.n_bias = 0; d.lut_in_dt = DFX_U8; CHECK(!wsum_vec_class(d));
}

static void check_alias() {
  const unsigned long long e = 1000;
  const int u8s32[2] = {DFX_U8, DFX_S32};
  uintptr_t src[2] = {0x10000, 0x20000};
  CHECK(wsum_alias(2, src, u8s32, 0x30000, DFX_U8, e) == WSUM_ALIAS_NONE);
  CHECK(wsum_alias(2, src, u8s32, 0x10000, DFX_U8, e) == WSUM_ALIAS_IN_PLACE);      // dst is the u8 input
  CHECK(wsum_alias(2, src, u8s32, 0x20000, DFX_U8, e) == WSUM_ALIAS_REFUSED);       // 1-byte dst at the 4-byte input
  CHECK(wsum_alias(2, src, u8s32, 0x20000, DFX_F32, e) == WSUM_ALIAS_IN_PLACE);     // 4-byte dst at the 4-byte input
  CHECK(wsum_alias(2, src, u8s32, 0x10000, DFX_F32, e) == WSUM_ALIAS_REFUSED);
  CHECK(wsum_alias(2, src, u8s32, 0x10000 + 999, DFX_U8, e) == WSUM_ALIAS_REFUSED); // last byte of the u8 input
  CHECK(wsum_alias(2, src, u8s32, 0x10000 + 1000, DFX_U8, e) == WSUM_ALIAS_NONE);
  CHECK(wsum_alias(2, src, u8s32, 0x10000 - 1000, DFX_U8, e) == WSUM_ALIAS_NONE);
  CHECK(wsum_alias(2, src, u8s32, 0x10000 - 999, DFX_U8, e) == WSUM_ALIAS_REFUSED);
  CHECK(wsum_alias(2, src, u8s32, 0x20000 + 3999, DFX_U8, e) == WSUM_ALIAS_REFUSED);
  CHECK(wsum_alias(2, src, u8s32, 0x20000 + 4000, DFX_U8, e) == WSUM_ALIAS_NONE);
  // one buffer given twice, dst being it; dst being input 0 while overlapping input 1 partially
  const int u8u8[2] = {DFX_U8, DFX_U8};
  uintptr_t same[2] = {0x10000, 0x10000};
  CHECK(wsum_alias(2, same, u8u8, 0x10000, DFX_U8, e) == WSUM_ALIAS_IN_PLACE);
  CHECK(wsum_alias(2, same, u8u8, 0x40000, DFX_S8, e) == WSUM_ALIAS_NONE);
  uintptr_t shifted[2] = {0x10000, 0x10000 + 16};
  CHECK(wsum_alias(2, shifted, u8u8, 0x10000, DFX_U8, e) == WSUM_ALIAS_REFUSED);
  CHECK(wsum_alias(2, shifted, u8u8, 0x10000 + 16, DFX_U8, e) == WSUM_ALIAS_REFUSED);
  // the last input
  uintptr_t three[3] = {0x10000, 0x20000, 0x30000};
  const int dts[3] = {DFX_S8, DFX_U8, DFX_S8};
  CHECK(wsum_alias(3, three, dts, 0x30000, DFX_U8, e) == WSUM_ALIAS_IN_PLACE);
}

static void check_grid() {
  CHECK(wsum_grid(0, 0) == 1 && wsum_grid(1, 0) == 1 && wsum_grid(256, 0) == 1 && wsum_grid(257, 0) == 2);
  CHECK(wsum_grid(1ll << 40, 0) == WSUM_MAX_BLOCKS && wsum_grid(1ll << 40, 2) == 2 && wsum_grid(100, 5) == 1);
  CHECK(wsum_grid(1ll << 40, 1ll << 40) == WSUM_MAX_BLOCKS);
  // every item is visited exactly once by the grid-stride loop, the vec kernel's running channel group equals id % groups
  const long long items[] = {1, 5, 255, 256, 257, 3 * 9 * 11 * 2, 70000};
  const int groups[] = {1, 2, 3, 16, 45, 128};
  for (long long n : items)
    for (int cap = 0; cap < 4; ++cap)
      for (int gr : groups) {
        const int grid = wsum_grid(n, cap);
        const long long stride = (long long)grid * WSUM_THREADS;
        std::vector<char> seen((size_t)n, 0);
        for (long long id0 = 0; id0 < stride; ++id0) {
          int g = (int)(id0 % gr);
          const int gstep = (int)(stride % gr);
          for (long long id = id0; id < n; id += stride) {
            CHECK(!seen[(size_t)id]);
            seen[(size_t)id] = 1;
            CHECK(g == (int)(id % gr));
            g += gstep;
            if (g >= gr) g -= gr;
          }
        }
        for (char s : seen) CHECK(s);
      }
  // the auto rule: the vec kernel in its class from 2^19 elements on; a forced path is taken as it is
  dfx_wsum_desc a = base();
  a.bs = 1; a.h = 64; a.w = 64; a.c = 128; a.nscales[1] = 128;
  CHECK(wsum_elems(a) == WSUM_AUTO_MIN_ELEMS && wsum_path(a) == DFX_WSUM_VEC);
  a.h = 63; CHECK(wsum_path(a) == DFX_WSUM_GENERIC);
  a.force_path = DFX_WSUM_VEC; CHECK(wsum_path(a) == DFX_WSUM_VEC);
  a.h = 64; a.force_path = DFX_WSUM_GENERIC; CHECK(wsum_path(a) == DFX_WSUM_GENERIC);
  a.force_path = -1; a.c = 136; a.nscales[1] = 136; CHECK(wsum_path(a) == DFX_WSUM_GENERIC);  // outside the class
  dfx_wsum_desc d = base();
  CHECK(wsum_items(d, DFX_WSUM_VEC) * 16 == wsum_elems(d) && wsum_items(d, DFX_WSUM_GENERIC) == wsum_elems(d));
}

int main() {
  check_validation();
  check_image();
  check_alias();
  check_grid();
  if (failures) {
    printf("wsum_plan_check: %d failures\n", failures);
    return 1;
  }
  printf("wsum plans: validation, constant image, aliasing and grid hold\n");
  return 0;
}
