// window_check -- runs deepfusion::window_partition / window_reverse of the drop-in C++ API (include/deepfusion.h) and compares
// every result, byte for byte, with a scalar restatement of include/dfx.h in this file (four nested loops over windows and
// in-window tokens; no row map).  One frame chains partition -> reverse on the device with no host step in between, submitted
// asynchronously, and must give the grid back; another keeps two partitions of one grid in flight at once.  With a directory
// argument it also runs the cases a test wrote there (cases.txt:
//   case <name> <dir> <bs> <grid_C> <h> <w> <c_valid> <win_C> <wh> <ww> <shift_y> <shift_x> <col_major> <dtype> <pad hex> <async>
// with <name>.src / .dst beside it; .dst is the expected storage of dst) against BOTH the file and the scalar restatement.
// Prints one line per case, "ok" or "DIFFERENT"; exits non-zero on a difference.
//   window_check [directory]
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "cli_flags.h"
#include "deepfusion.h"
#include "dfx.h"

using namespace deepfusion;
typedef memory::dtype DT;

static std::unique_ptr<memory> mk(int n, int c, int h, int w, DT dt) {
  return std::unique_ptr<memory>(new memory(memory::nchw_dims{n, c, h, w}, memory::format::nhwc, dt));
}
static size_t esize(DT dt) { return (dt == DT::f32 || dt == DT::s32) ? 4 : 1; }
static const char *dt_name(DT dt) { return dt == DT::f32 ? "f32" : dt == DT::s32 ? "s32" : dt == DT::u8 ? "u8" : "s8"; }

struct Geo {
  int bs, h, w, c, gC, wC;  // c valid of gC (grid side) and wC (window side) channels
  window_shape ws;
  size_t es;
  int hp() const { return (h + ws.wh - 1) / ws.wh * ws.wh; }
  int wp() const { return (w + ws.ww - 1) / ws.ww * ws.ww; }
};

// dir 0: win <- grid (pad tokens <- pad); dir 1: grid <- win.  Only the c valid channels of the destination are touched.
static void ref_window(int dir, const Geo &g, const unsigned char *src, unsigned char *dst, uint32_t pad) {
  const int hp = g.hp(), wp = g.wp(), nwy = hp / g.ws.wh, nwx = wp / g.ws.ww;
  unsigned char padb[4];
  if (g.es == 1) padb[0] = (unsigned char)(pad & 0xff);
  else memcpy(padb, &pad, 4);
  for (int b = 0; b < g.bs; ++b)
    for (int wy = 0; wy < nwy; ++wy)
      for (int wx = 0; wx < nwx; ++wx)
        for (int iy = 0; iy < g.ws.wh; ++iy)
          for (int ix = 0; ix < g.ws.ww; ++ix) {
            const int y = (wy * g.ws.wh + iy + g.ws.shift_y) % hp, x = (wx * g.ws.ww + ix + g.ws.shift_x) % wp;
            const size_t in = g.ws.col_major ? (size_t)ix * g.ws.wh + iy : (size_t)iy * g.ws.ww + ix;
            const size_t wrow = ((size_t)b * nwy * nwx + (size_t)wy * nwx + wx) * g.ws.wh * g.ws.ww + in;
            const size_t grow = ((size_t)b * g.h + y) * g.w + x;
            const bool is_pad = y >= g.h || x >= g.w;
            unsigned char *wp_ = const_cast<unsigned char *>(dir == 0 ? dst : src) + wrow * g.wC * g.es;
            unsigned char *gp_ = const_cast<unsigned char *>(dir == 0 ? src : dst) + grow * g.gC * g.es;
            if (dir == 0) {
              if (is_pad) for (size_t k = 0; k < (size_t)g.c * g.es; ++k) wp_[k] = padb[k % g.es];
              else memcpy(wp_, gp_, (size_t)g.c * g.es);
            } else if (!is_pad) {
              memcpy(gp_, wp_, (size_t)g.c * g.es);
            }
          }
}

static int report(const char *name, const std::string &what, bool bad) {
  printf("window_check %-14s %s: %s\n", name, what.c_str(), bad ? "DIFFERENT from the reference" : "ok");
  return bad ? 1 : 0;
}
// the c valid channels of every row (the op leaves the pad channels of dst's device copy as they are)
static bool rows_differ(const void *got, const void *want, size_t rows, int ld, int c, size_t es) {
  for (size_t r = 0; r < rows; ++r)
    if (memcmp((const unsigned char *)got + r * ld * es, (const unsigned char *)want + r * ld * es, (size_t)c * es) != 0) return true;
  return false;
}
static void fill(memory &m, Lcg &g) {
  for (size_t i = 0; i < m.buffer_size(); ++i) ((uint8_t *)m.data())[i] = (uint8_t)(g.next() & 0xff);
}
static std::string describe(int dir, const Geo &g, DT dt, bool use_async) {
  char what[240];
  snprintf(what, sizeof(what), "%s bs %d %dx%d c %d/%d/%d window %dx%d shift %d,%d %s %s %s", dir ? "reverse" : "partition", g.bs, g.h, g.w, g.c, g.gC, g.wC,
           g.ws.wh, g.ws.ww, g.ws.shift_y, g.ws.shift_x, g.ws.col_major ? "col" : "row", dt_name(dt), use_async ? "async" : "sync");
  return what;
}

// one op on fresh tensors; src: the source's storage or null for random bytes; file: the expected storage of dst or null
static int check_one(const char *name, int dir, Geo g, DT dt, uint32_t pad, bool use_async, Lcg &rng, const unsigned char *src_bytes = nullptr,
                     const unsigned char *file = nullptr) {
  g.es = esize(dt);
  const int hp = g.hp(), wp = g.wp();
  auto grid = mk(g.bs, g.gC, g.h, g.w, dt), win = mk(g.bs, g.wC, hp, wp, dt);
  memory &src = dir == 0 ? *grid : *win, &dst = dir == 0 ? *win : *grid;
  if (src_bytes) memcpy(src.data(), src_bytes, src.buffer_size());
  else fill(src, rng);
  memset(dst.data(), 0xCD, dst.buffer_size());
  std::vector<unsigned char> want(dst.buffer_size(), 0xCD);
  ref_window(dir, g, (const unsigned char *)src.host_data(), want.data(), pad);
  auto op = dir == 0 ? window_partition(grid, win, g.ws, pad, g.c) : window_reverse(win, grid, g.ws, g.c);
  if (use_async) {
    op->submit_async();
    op->wait();
    dst.download();
  } else {
    op->submit();
  }
  const size_t rows = dir == 0 ? (size_t)g.bs * hp * wp : (size_t)g.bs * g.h * g.w;
  const int ld = dir == 0 ? g.wC : g.gC;
  const bool b_ref = rows_differ(dst.host_data(), want.data(), rows, ld, g.c, g.es);
  const bool b_file = file && rows_differ(dst.host_data(), file, rows, ld, g.c, g.es);
  return report(name, describe(dir, g, dt, use_async) + (b_file ? " [file differs]" : "") + (b_ref ? " [scalar reference differs]" : ""), b_ref || b_file);
}

// partition -> reverse, both submitted asynchronously: the windows never leave the device in between, the grid comes back
static int frame_round_trip(Lcg &rng) {
  Geo g = {2, 16, 12, 64, 64, 192, {7, 7, 3, 3, false}, 1};
  auto grid = mk(g.bs, g.gC, g.h, g.w, DT::s8), win = mk(g.bs, g.wC, g.hp(), g.wp(), DT::s8), back = mk(g.bs, g.gC, g.h, g.w, DT::s8);
  fill(*grid, rng);
  memset(back->data(), 0xCD, back->buffer_size());
  auto part = window_partition(grid, win, g.ws, 0x80);
  auto rev = window_reverse(win, back, g.ws, g.c);
  const char *shards = getenv("DEEPFUSION_DEVICES");
  if (shards && *shards) {  // sharded ops work host to host: the chain runs through the host tensors
    part->submit();
    rev->submit();
  } else {
    part->submit_async();
    rev->submit_async();
    rev->wait();
    part->wait();
    win->download();
    back->download();
  }
  std::vector<unsigned char> want(win->buffer_size(), 0);
  ref_window(0, g, (const unsigned char *)grid->host_data(), want.data(), 0x80);
  const bool bad = rows_differ(win->host_data(), want.data(), (size_t)g.bs * g.hp() * g.wp(), g.wC, g.c, 1) ||
                   memcmp(back->host_data(), grid->host_data(), grid->buffer_size()) != 0;
  return report("round trip", "partition -> reverse of bs 2 16x12x64, window 7, shift 3, asynchronous", bad);
}

// two partitions of one grid in flight at once: the W-MSA and the SW-MSA windows
static int frame_two_in_flight(Lcg &rng) {
  Geo a = {3, 10, 13, 24, 24, 24, {7, 7, 0, 0, false}, 4}, b = a;
  b.ws.shift_y = 3; b.ws.shift_x = 3; b.ws.col_major = true;
  auto grid = mk(a.bs, a.gC, a.h, a.w, DT::f32), wa = mk(a.bs, a.wC, a.hp(), a.wp(), DT::f32), wb = mk(a.bs, a.wC, a.hp(), a.wp(), DT::f32);
  fill(*grid, rng);
  auto pa = window_partition(grid, wa, a.ws, 0x3fc01234u), pb = window_partition(grid, wb, b.ws, 0);
  pa->submit_async();
  pb->submit_async();
  pb->wait();
  pa->wait();
  wa->download();
  wb->download();
  std::vector<unsigned char> ra(wa->buffer_size(), 0), rb(wb->buffer_size(), 0);
  ref_window(0, a, (const unsigned char *)grid->host_data(), ra.data(), 0x3fc01234u);
  ref_window(0, b, (const unsigned char *)grid->host_data(), rb.data(), 0);
  const bool bad = memcmp(wa->host_data(), ra.data(), ra.size()) != 0 || memcmp(wb->host_data(), rb.data(), rb.size()) != 0;
  return report("two in flight", "two f32 partitions of one 10x13 grid, submit_async on both", bad);
}

static bool read_file(const std::string &path, std::vector<unsigned char> &out, size_t want) {
  FILE *f = fopen(path.c_str(), "rb");
  if (!f) return false;
  out.resize(want);
  const size_t n = fread(out.data(), 1, want, f);
  const bool more = fgetc(f) != EOF;
  fclose(f);
  return n == want && !more;
}

static int run_directory(const std::string &dir, int *n_out, Lcg &rng) {
  FILE *f = fopen((dir + "/cases.txt").c_str(), "r");
  if (!f) { fprintf(stderr, "window_check: cannot read %s/cases.txt\n", dir.c_str()); return 1; }
  int bad = 0, n = 0;
  char name[64];
  int d, bs, gC, h, w, c, wC, wh, ww, sy, sx, col, dtc, use_async;
  unsigned pad;
  while (fscanf(f, " case %63s %d %d %d %d %d %d %d %d %d %d %d %d %d %x %d", name, &d, &bs, &gC, &h, &w, &c, &wC, &wh, &ww, &sy, &sx, &col, &dtc, &pad,
                &use_async) == 16) {
    const DT dt = dtc == DFX_F32 ? DT::f32 : dtc == DFX_S32 ? DT::s32 : dtc == DFX_U8 ? DT::u8 : DT::s8;
    Geo g = {bs, h, w, c, gC, wC, {wh, ww, sy, sx, col != 0}, esize(dt)};
    const size_t gbytes = (size_t)bs * h * w * gC * g.es, wbytes = (size_t)bs * g.hp() * g.wp() * wC * g.es;
    std::vector<unsigned char> fs, fd;
    const std::string base = dir + "/" + name;
    if (!read_file(base + ".src", fs, d == 0 ? gbytes : wbytes) || !read_file(base + ".dst", fd, d == 0 ? wbytes : gbytes)) {
      fprintf(stderr, "window_check: case %s: a file is missing or has the wrong size\n", name);
      fclose(f);
      return 1;
    }
    bad += check_one(name, d, g, dt, pad, use_async != 0, rng, fs.data(), fd.data());
    ++n;
  }
  fclose(f);
  *n_out = n;
  return bad;
}

int main(int argc, char **argv) {
  Lcg g(1979);
  int bad = 0, n = 0;
  bad += check_one("swin s1", 0, Geo{2, 56, 56, 96, 96, 96, {7, 7, 0, 0, false}, 1}, DT::s8, 0, false, g); ++n;
  bad += check_one("swin s1 shift", 0, Geo{2, 56, 56, 96, 96, 96, {7, 7, 3, 3, false}, 1}, DT::s8, 0, true, g); ++n;
  bad += check_one("swin reverse", 1, Geo{2, 56, 56, 96, 96, 96, {7, 7, 3, 3, false}, 1}, DT::u8, 0, false, g); ++n;
  bad += check_one("padded", 0, Geo{3, 10, 13, 48, 48, 64, {7, 7, 3, 0, false}, 1}, DT::u8, 0x80, false, g); ++n;
  bad += check_one("padded rev", 1, Geo{3, 10, 13, 48, 64, 48, {7, 7, 13, 13, true}, 1}, DT::s8, 0, true, g); ++n;
  bad += check_one("merge", 0, Geo{2, 16, 12, 64, 64, 64, {2, 2, 0, 0, true}, 1}, DT::s8, 0, false, g); ++n;
  bad += check_one("merge odd", 0, Geo{1, 7, 5, 21, 21, 23, {2, 2, 0, 0, true}, 1}, DT::u8, 0x7f, true, g); ++n;
  bad += check_one("expand", 1, Geo{2, 8, 8, 4, 4, 4, {2, 2, 0, 0, false}, 4}, DT::f32, 0, false, g); ++n;
  bad += check_one("big window", 0, Geo{2, 5, 4, 12, 12, 12, {7, 7, 6, 2, false}, 4}, DT::s32, 0xdeadbeefu, false, g); ++n;
  bad += check_one("c_valid", 1, Geo{2, 3, 200, 5, 8, 7, {3, 5, 1, 4, false}, 4}, DT::f32, 0, true, g); ++n;
  bad += check_one("one token", 0, Geo{5, 1, 1, 16, 16, 16, {1, 1, 0, 0, false}, 1}, DT::s8, 0, false, g); ++n;
  bad += frame_round_trip(g); ++n;
  bad += frame_two_in_flight(g); ++n;
  if (argc > 1) {
    int m = 0;
    bad += run_directory(argv[1], &m, g);
    printf("window_check: %d entries from %s\n", m, argv[1]);
    n += m;
  }
  if (bad) {
    printf("window_check: %d of %d cases FAILED\n", bad, n);
    return 1;
  }
  printf("window_check: every case identical to the reference (%d cases)\n", n);
  return 0;
}
