// requant_host_check -- host-only check of the requantisation constants and of the fast route's proof
// (csrc/requant_host.h), meant to be built with the host sanitizers; it needs no GPU and no HIP:
//   g++ -std=c++11 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/requant_host_check.cc -o tools/requant_host_check
// Every expected value below is a literal worked out by hand; the two scales at the edge of the 2^30 clause are derived
// with nextafterf and both sides of the edge are asserted.
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../csrc/requant_host.h"

static int failures = 0;
#define CHECK(cond)                                            \
  do {                                                         \
    if (!(cond)) {                                             \
      printf("line %d: %s is false\n", __LINE__, #cond);       \
      ++failures;                                              \
    }                                                          \
  } while (0)

static unsigned bits(float f) {
  unsigned u;
  memcpy(&u, &f, 4);
  return u;
}

int main() {
  using namespace dfx;
  const float inf = INFINITY, nan = NAN;

  // ---- the small helpers
  CHECK(round16(0) == 0 && round16(1) == 16 && round16(16) == 16 && round16(17) == 32);
  CHECK(!strcmp(dt_name(DFX_F32), "f32") && !strcmp(dt_name(DFX_S32), "s32") && !strcmp(dt_name(DFX_S8), "s8") &&
        !strcmp(dt_name(DFX_U8), "u8"));

  // ---- bias conversion (buffers of exactly the indexed size: the sanitizer sees an element too many)
  {
    const std::vector<int8_t> s8 = {0, -128};
    const std::vector<uint8_t> u8 = {0, 255};
    const std::vector<int32_t> s32 = {INT32_MIN, 16777217, 16777219};  // 2^24 + 1 and + 3: ties, to the even neighbour
    CHECK(bias_to_f32(s8.data(), DFX_S8, 1) == -128.0f);
    CHECK(bias_to_f32(u8.data(), DFX_U8, 1) == 255.0f);
    CHECK(bias_to_f32(s32.data(), DFX_S32, 0) == -2147483648.0f);
    CHECK(bias_to_f32(s32.data(), DFX_S32, 1) == 16777216.0f);
    CHECK(bias_to_f32(s32.data(), DFX_S32, 2) == 16777220.0f);
    const unsigned payload = 0x7fc12345u;  // a quiet NaN with a payload
    std::vector<float> f32(2, 0.0f);
    memcpy(&f32[1], &payload, 4);
    CHECK(bits(bias_to_f32(f32.data(), DFX_F32, 1)) == payload);
  }

  // ---- constants of a channel with the taps {127, -128, 0, 5}: P = 127 + 5 = 132, N = 128, comp = 128 * (132 - 128) = 512
  const double amax = 33660.0;  // 255 * max(132, 128)
  {
    const std::vector<int8_t> wei = {127, -128, 0, 5, 127, -128, 0, 5};
    const std::vector<int32_t> bia = {7, -9};
    const float one_scale[1] = {0.5f};
    std::vector<int32_t> comp(2, -1);
    std::vector<float> fb(2, -1.0f), fs(2, -1.0f);
    const int8_t *w = wei.data();
    const bool ok = requant_consts(2, 4, [w](int k, size_t i) { return w[(size_t)k * 4 + i]; }, bia.data(), DFX_S32, one_scale, 1,
                                   comp.data(), fb.data(), fs.data());
    CHECK(ok);
    CHECK(comp[0] == 512 && comp[1] == 512);
    CHECK(fb[0] == 7.0f && fb[1] == -9.0f);
    CHECK(fs[0] == 0.5f && fs[1] == 0.5f);  // nscales == 1: broadcast
    // no bias: zeros, and the bias pointer is not read
    const bool ok2 = requant_consts(2, 4, [w](int k, size_t i) { return w[(size_t)k * 4 + i]; }, nullptr, DFX_UNDEF, one_scale, 1,
                                    comp.data(), fb.data(), fs.data());
    CHECK(ok2 && fb[0] == 0.0f && fb[1] == 0.0f);
  }

  // ---- the clause at its edge: two adjacent floats with 33660 * s_lo <= 2^30 < 33660 * s_hi, products in double
  const double lim = 1073741824.0;
  float s_lo = (float)(lim / amax);
  if (amax * (double)s_lo > lim) s_lo = nextafterf(s_lo, 0.0f);
  const float s_hi = nextafterf(s_lo, inf);
  CHECK(amax * (double)s_lo <= lim && lim < amax * (double)s_hi);
  CHECK(s_lo > 31899.0f && s_hi < 31900.0f);  // 2^30 / 33660 = 31899.6...
  CHECK(fast_ok_2p30(amax, 0.0f, s_lo));
  CHECK(!fast_ok_2p30(amax, 0.0f, s_hi));
  CHECK(fast_ok_2p30(amax, 0.0f, -s_lo) && !fast_ok_2p30(amax, 0.0f, -s_hi));  // |scale|
  // a bias that alone tips it over: (33660 + 1) * s_lo is 31899 beyond what 33660 * s_lo leaves below 2^30
  CHECK(!fast_ok_2p30(amax, 1.0f, s_lo) && !fast_ok_2p30(amax, -1.0f, s_lo));
  // not finite: rejected whatever the other operand is
  CHECK(!fast_ok_2p30(0.0, nan, 1.0f) && !fast_ok_2p30(0.0, inf, 1.0f) && !fast_ok_2p30(0.0, -inf, 1.0f));
  CHECK(!fast_ok_2p30(0.0, 0.0f, nan) && !fast_ok_2p30(0.0, 0.0f, inf) && !fast_ok_2p30(0.0, 0.0f, -inf));
  CHECK(!fast_ok_2p30(0.0, inf, 0.0f) && !fast_ok_2p30(0.0, nan, 0.0f));
  // the all-zero channel: accepted under any finite scale
  CHECK(fast_ok_2p30(0.0, 0.0f, 1.0f) && fast_ok_2p30(0.0, 0.0f, FLT_MAX) && fast_ok_2p30(0.0, 0.0f, 0.0f));

  // ---- all channels: the same edge through requant_consts, which derives amax = 33660 from the taps itself;
  //      exactly one failing channel of three makes it false, and every channel's constants are still written
  {
    const std::vector<int8_t> wei = {127, -128, 0, 5, 0, 0, 0, 0, 127, -128, 0, 5};  // channel 1 is all-zero
    const int8_t *w = wei.data();
    auto tap = [w](int k, size_t i) { return w[(size_t)k * 4 + i]; };
    for (int bad = -1; bad < 3; ++bad) {
      std::vector<float> scales = {s_lo, FLT_MAX, s_lo};
      if (bad == 0 || bad == 2) scales[bad] = s_hi;
      if (bad == 1) scales[bad] = inf;
      std::vector<int32_t> comp(3, -1);
      std::vector<float> fb(3, -1.0f), fs(3, -1.0f);
      const bool ok = requant_consts(3, 4, tap, nullptr, DFX_UNDEF, scales.data(), 3, comp.data(), fb.data(), fs.data());
      CHECK(ok == (bad < 0));
      CHECK(comp[0] == 512 && comp[1] == 0 && comp[2] == 512);
      CHECK(fb[0] == 0.0f && fb[1] == 0.0f && fb[2] == 0.0f);
      CHECK(bits(fs[0]) == bits(scales[0]) && bits(fs[1]) == bits(scales[1]) && bits(fs[2]) == bits(scales[2]));
    }
    // a bias that tips one channel over
    const std::vector<int8_t> bia = {0, 0, 1};
    const std::vector<float> scales = {s_lo, 1.0f, s_lo};
    std::vector<int32_t> comp(3);
    std::vector<float> fb(3), fs(3);
    CHECK(!requant_consts(3, 4, tap, bia.data(), DFX_S8, scales.data(), 3, comp.data(), fb.data(), fs.data()));
    CHECK(fb[2] == 1.0f);
  }

  if (failures) {
    printf("requant_host_check: %d check(s) FAILED\n", failures);
    return 1;
  }
  printf("requant_host_check: bias conversion, constants and the 2^30 clause at its edge (scales %.9g | %.9g) all as worked out by hand\n",
         (double)s_lo, (double)s_hi);
  return 0;
}
