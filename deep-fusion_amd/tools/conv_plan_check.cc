// conv_plan_check -- host-only driver and check of csrc/conv_plan.h, everything dfx_conv_create decides before it allocates.
// No HIP: it builds with SAN=1 (ASan + UBSan) and runs anywhere.
//   conv_plan_check < cases.txt   one case per line: the 25 integers of dfx_conv_desc in the header's order, the device's CU
//                                 count, the workgroups per CU the runtime reports for the chosen stream / direct / pointwise
//                                 kernel, then any number of KEY=VALUE tuning switches.  Prints one line per case: "rc=<code>
//                                 <message>" where dfx_conv_create refuses, otherwise every field of the plan (of the chosen
//                                 geometry all but the pointers and the requant fields dfx_conv_set_weights fills), the
//                                 kernel's name last.  tests/golden/conv_plans.json holds such lines recorded on an MI355X.
//   conv_plan_check < /dev/null   the self-check: over a sweep of small descriptors and switches, what the kernels' decoders
//                                 rely on: unit counts, the magic numbers' exact division over their whole range, LDS size,
//                                 alignment and order of every LDS offset, the half-unit rules of tests/hipref.check_sched.
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../csrc/conv_plan.h"

using namespace dfx;

static int g_bad = 0;
#define EXPECT(cond)                                                                   \
  do {                                                                                 \
    if (!(cond)) {                                                                     \
      if (++g_bad <= 20) printf("conv_plan_check: line %d: %s [%s]\n", __LINE__, #cond, g_case.c_str()); \
    }                                                                                  \
  } while (0)

static std::string g_case;
static std::vector<std::pair<std::string, std::string> > g_tuning;
static int g_per_cu = 1;
static const char *tune_of(const char *key) {
  for (const auto &kv : g_tuning)
    if (kv.first == key) return kv.second.c_str();
  return nullptr;
}

static int plan(const dfx_conv_desc &d, int ncu, ConvPlan *p, const char **why) {
  memset(p, 0, sizeof(*p));
  const int rc = conv_validate(d, why);
  if (rc) return rc;
  ConvEnv env;
  env.ncu = ncu;
  env.tune = tune_of;
  env.wg_per_cu = [](void *, const ConvPlan &) { return g_per_cu; };
  env.ctx = nullptr;
  return conv_plan(d, env, p, why);
}

static bool resident(const ConvPlan &p) { return p.variant == DFX_VARIANT_MFMA_FUSED || p.variant == DFX_VARIANT_MFMA_CONV; }

static void print_plan(const ConvPlan &P) {
  printf("variant=%d direct=%d pw=%d nw=%d wo=%d wo1=%d occ=%d pxb=%d icb=%d ocb=%d G=%d grid=%d block=%d lds=%d roles_ok=%d rows_per_unit=%d units_per_image=%d",
         P.variant, P.direct, P.pw, P.nw, P.wo, P.wo1, P.occ, P.pxb, P.icb, P.ocb, P.G, P.grid, P.block, P.lds, (int)P.roles_ok, P.rows_per_unit, P.units_per_image);
  if (resident(P)) {
    const MfmaGeom &g = P.geom;
    printf(" m.th=%d m.tw=%d m.uy=%d m.ux=%d m.linear=%d m.total_units=%d m.row_chunks=%d m.tile_chunks=%d m.row_magic=%u m.tw_magic=%u m.upi_magic=%u m.ux_magic=%u m.ntu=%d m.ntu_magic=%u m.claim_limit=%d m.tile_stride=%d m.static_rounds=%d m.pool=%d m.lazy_queue=%d m.half_from=%d m.upx=%d",
           g.th, g.tw, g.uy, g.ux, g.linear, g.total_units, g.row_chunks, g.tile_chunks, g.row_magic, g.tw_magic, g.upi_magic, g.ux_magic, g.ntu, g.ntu_magic, g.claim_limit, g.tile_stride, g.static_rounds, g.pool, g.lazy_queue, g.half_from, g.upx);
  } else if (P.variant == DFX_VARIANT_MFMA_STREAM && !P.direct) {
    const StreamGeom &g = P.sgeom;
    printf(" s.ni=%d s.thv=%d s.twv=%d s.uy=%d s.ux=%d s.total_units=%d s.lh=%d s.lw=%d s.npos=%d s.n_icc=%d s.icb=%d s.n_occ=%d s.ocb=%d s.n_g1=%d s.ks2=%d s.s0_steps=%d s.mid_stride=%d s.off_tile=%d s.off_pxoff=%d s.off_mid=%d s.off_cst=%d s.off_stage=%d s.planes=%d s.mg_g4=%u s.mg_lhw=%u s.mg_lw=%u s.occ_par=%d",
           g.ni, g.thv, g.twv, g.uy, g.ux, g.total_units, g.lh, g.lw, g.npos, g.n_icc, g.icb, g.n_occ, g.ocb, g.n_g1, g.ks2, g.s0_steps, g.mid_stride, g.off_tile, g.off_pxoff, g.off_mid, g.off_cst, g.off_stage, g.planes, g.mg_g4, g.mg_lhw, g.mg_lw, g.occ_par);
  } else if (P.variant == DFX_VARIANT_MFMA_STREAM) {
    const DirectGeom &g = P.dgeom;
    printf(" d.ni=%d d.thv=%d d.twv=%d d.uy=%d d.ux=%d d.total_units=%d d.lh=%d d.lw=%d d.npos=%d d.icb=%d d.n_planes=%d d.plane_bytes=%d d.row_pitch=%d d.img_pitch=%d d.unfused=%d d.ocb=%d d.n_g1=%d d.mid_stride=%d d.off_pxoff=%d d.off_mid=%d d.off_cst=%d d.npb=%d",
           g.ni, g.thv, g.twv, g.uy, g.ux, g.total_units, g.lh, g.lw, g.npos, g.icb, g.n_planes, g.plane_bytes, g.row_pitch, g.img_pitch, g.unfused, g.ocb, g.n_g1, g.mid_stride, g.off_pxoff, g.off_mid, g.off_cst, g.npb);
    if (P.pw) {
      const PwGeom &q = P.pwgeom;
      printf(" p.icb=%d p.ocb=%d p.px_total=%d p.n_blocks=%d p.off_cst=%d p.off_stage=%d p.stage_bytes=%d", q.icb, q.ocb, q.px_total, q.n_blocks, q.off_cst, q.off_stage, q.stage_bytes);
    }
  }
  printf(" name=%s\n", P.kernel_name);
}

// n / div == umulhi(n, magic) for every n in [0, range): all of a small range, else the top of it, where a magic number
// that is too coarse fails first (at the last n = k * div - 1 and k * div)
static bool magic_exact(unsigned magic, long long div, long long range) {
  auto ok = [&](long long n) { return n < 0 || (long long)(((unsigned long long)n * magic) >> 32) == n / div; };
  if (range <= (1 << 17)) {
    for (long long n = 0; n < range; ++n)
      if (!ok(n)) return false;
    return true;
  }
  for (long long n = 0; n < (1 << 16); ++n)
    if (!ok(n)) return false;
  const long long top = (range - 1) / div;
  for (long long k = top; k > top - 4096 && k > 0; --k)
    if (!ok(k * div - 1) || !ok(k * div) || !ok(k * div + div - 1 < range ? k * div + div - 1 : range - 1)) return false;
  return ok(range - 1);
}

static void check_plan(const dfx_conv_desc &d, int ncu, const ConvPlan &p) {
  const long long px = (long long)d.bs * d.oh * d.ow;
  EXPECT(p.lds >= 0 && p.lds <= 163840);
  EXPECT(p.grid >= 1 && p.block >= 64 && p.block <= 1024 && p.block % 64 == 0);
  EXPECT(p.kernel_name[0] != 0 && strlen(p.kernel_name) < sizeof(p.kernel_name));
  if (resident(p)) {
    const MfmaGeom &g = p.geom;
    const long long units = (long long)d.bs * g.uy * g.ux;
    const int teams = p.grid * MFMA_TEAMS;
    EXPECT(g.th >= 1 && g.tw >= 1 && g.uy >= 1 && g.ux >= 1 && teams >= 2 && p.grid <= ncu);
    EXPECT(g.linear ? g.tw == d.ow : (g.tw % 32 == 0 && g.tw < d.ow));
    // ---- hand-out: tests/hipref.check_sched
    if (g.half_from >= g.total_units) {
      EXPECT(g.total_units == units && g.half_from == 0x7fffffff);
    } else {
      const long long nh = g.total_units - units;
      EXPECT(!p.roles_ok && !g.pool && g.th % 2 == 0 && g.lazy_queue == 1 && !g.upx);
      EXPECT(nh > 0 && g.half_from == units - nh && g.total_units == units + nh);
      EXPECT(nh <= units - (long long)(g.static_rounds + 1) * teams);
    }
    EXPECT(g.static_rounds >= 0 && (long long)g.static_rounds * teams < g.total_units + teams);
    // ---- the decoders' divisions
    EXPECT(g.row_chunks == (g.tw + 2) * (d.ic / 16) && g.tile_chunks == (g.th + 2) * g.row_chunks);
    EXPECT(magic_exact(g.row_magic, g.row_chunks, g.tile_chunks + 64));
    EXPECT(magic_exact(g.tw_magic, g.tw, g.upx ? (long long)d.oh * d.ow + g.upx : (long long)g.th * g.tw + 32));
    if (g.uy * g.ux > 1) EXPECT(magic_exact(g.upi_magic, (long long)g.uy * g.ux, units));
    else EXPECT(g.upi_magic == 0);
    if (g.ux > 1) EXPECT(magic_exact(g.ux_magic, g.ux, (long long)g.uy * g.ux));
    else EXPECT(g.ux_magic == 0);
    EXPECT(g.ntu >= 1 && g.claim_limit > 0 && g.claim_limit == (int)std::min<long long>(0x7ffffff0LL, (long long)g.ntu * ((long long)g.total_units + 4)));
    if (g.ntu > 1) EXPECT(magic_exact(g.ntu_magic, g.ntu, g.claim_limit));
    if (g.upx) EXPECT(g.upx % 32 == 0 && g.upx < 32768 && g.ux == 1 && g.ntu == g.upx / 32 && (long long)g.uy * g.upx >= (long long)d.oh * d.ow &&
                      (long long)(g.uy - 1) * g.upx < (long long)d.oh * d.ow && g.th == (d.ow - 1 + g.upx + d.ow - 1) / d.ow);
    else EXPECT((long long)g.uy * g.th >= d.oh && (long long)(g.uy - 1) * g.th < d.oh && (long long)g.ux * g.tw >= d.ow && (long long)(g.ux - 1) * g.tw < d.ow);
    if (g.pool) EXPECT(g.th % 2 == 0 && d.oc1x1 == 0);
    // ---- LDS: weights, constants, control block, then MFMA_NB tile slots
    EXPECT(g.tile_stride % 1024 == 0 && g.tile_stride >= g.tile_chunks * 16 + 1024);
    const int fixed = p.lds - MFMA_NB * g.tile_stride;
    EXPECT(fixed > 0 && fixed % 16 == 0);
    EXPECT(p.rows_per_unit == g.th && p.units_per_image == g.uy * g.ux && p.block == MFMA_THREADS);
  } else if (p.variant == DFX_VARIANT_MFMA_STREAM && !p.direct) {
    const StreamGeom &g = p.sgeom;
    const int M = ST_M * p.pxb;
    EXPECT((p.pxb == 1 || p.pxb == 2) && g.ni >= 1 && g.thv >= 1 && g.twv >= 1 && g.ni * g.thv * g.twv <= M);
    EXPECT(g.total_units == (d.bs + g.ni - 1) / g.ni * g.uy * g.ux && g.npos == g.ni * g.lh * g.lw);
    EXPECT((long long)g.uy * g.thv >= d.oh && (long long)g.ux * g.twv >= d.ow);
    const int offs[] = {g.off_tile, g.off_pxoff, g.off_mid, g.off_cst, g.off_stage};
    for (int o : offs) EXPECT(o % 16 == 0 && o >= 0 && o <= p.lds);
    EXPECT(g.off_tile < g.off_pxoff && g.off_pxoff + 4 * M == g.off_mid && g.off_mid <= g.off_cst && g.off_cst <= p.lds);
    EXPECT(g.off_pxoff - g.off_tile >= g.planes * g.npos * ST_POS + 16 && p.lds % 16 == 0);
    EXPECT(g.planes == 1 || g.planes == g.n_icc);
    EXPECT(magic_exact(g.mg_g4, 4 * g.planes, (long long)4 * g.planes * g.npos + 1024));
    EXPECT(magic_exact(g.mg_lhw, (long long)g.lh * g.lw, (long long)g.npos + 1024) && magic_exact(g.mg_lw, g.lw, (long long)g.lh * g.lw + 1024));
    EXPECT(p.grid <= g.total_units * (g.occ_par ? g.n_occ : 1) && p.block == ST_THREADS);
    EXPECT(!g.occ_par || (d.oc1x1 == 0 && g.n_occ > 1));
    EXPECT(px * (d.oc1x1 ? d.oc1x1 : d.oc) * (long long)conv_dt_size(d.dst_dt) < (1LL << 32) - 16);
  } else if (p.variant == DFX_VARIANT_MFMA_STREAM && !p.pw) {
    const DirectGeom &g = p.dgeom;
    const int M = 32 * g.npb;
    EXPECT((g.npb == 1 || g.npb == 2 || g.npb == 4) && g.ni >= 1 && g.ni * g.thv * g.twv <= M && g.n_planes <= 16);
    EXPECT(g.total_units == (d.bs + g.ni - 1) / g.ni * g.uy * g.ux && g.npos == g.ni * g.lh * g.lw);
    EXPECT((long long)g.uy * g.thv >= d.oh && (long long)g.ux * g.twv >= d.ow);
    EXPECT(g.row_pitch % 16 == 0 && g.row_pitch >= g.lw * DK_POS && g.img_pitch % 16 == 0 && g.img_pitch >= g.lh * g.row_pitch &&
           g.plane_bytes == g.ni * g.img_pitch);
    const int offs[] = {g.off_pxoff, g.off_mid, g.off_cst};
    for (int o : offs) EXPECT(o % 16 == 0 && o >= 0 && o <= p.lds);
    EXPECT(g.off_pxoff >= g.n_planes * g.plane_bytes + 16 && g.off_pxoff + 8 * M == g.off_mid && g.off_mid + M * g.mid_stride <= g.off_cst &&
           g.off_cst <= p.lds && p.lds % 16 == 0);
    EXPECT(p.grid <= g.total_units && p.block == 64 * p.nw && (p.nw == 4 || p.nw == 8));
  } else if (p.variant == DFX_VARIANT_MFMA_STREAM) {
    const PwGeom &g = p.pwgeom;
    EXPECT(g.px_total == px && g.n_blocks == (px + 31) / 32 && g.off_cst == d.oc * d.ic && g.off_cst % 16 == 0);
    EXPECT(g.off_stage % 16 == 0 && g.off_stage >= g.off_cst + 3 * d.oc * 4 && g.stage_bytes % 16 == 0 &&
           p.lds == g.off_stage + p.nw * g.stage_bytes);
    EXPECT(p.grid <= p.dgeom.total_units && p.block == PW_THREADS);
  } else {
    EXPECT(p.variant == DFX_VARIANT_GENERIC && (long long)p.grid * GEN_TP >= px && (long long)(p.grid - 1) * GEN_TP < px);
  }
}

static dfx_conv_desc desc(int bs, int ic, int ih, int iw, int oc, int oc1, int k, int s, int pad, int dst, int pool = 0) {
  dfx_conv_desc d;
  memset(&d, 0, sizeof(d));
  d.bs = bs; d.ic = ic; d.ih = ih; d.iw = iw; d.oc = oc; d.kh = d.kw = k; d.sh = d.sw = s; d.pad_t = d.pad_l = pad;
  d.oh = (ih + 2 * pad - k) / s + 1; d.ow = (iw + 2 * pad - k) / s + 1;
  d.oc1x1 = oc1; d.dst_dt = dst; d.conv0_nscales = d.conv1_nscales = 1; d.force_variant = -1; d.fuse_pool = pool;
  return d;
}

static int self_check() {
  int planned = 0, refused = 0, families[5] = {0, 0, 0, 0, 0}, halves = 0, runs = 0;
  auto one = [&](const dfx_conv_desc &d, int ncu, int per_cu) {
    char buf[160];
    snprintf(buf, sizeof(buf), "bs %d ic %d %dx%d oc %d oc1 %d k%d s%d p%d dt%d pool%d ncu %d/%d +%d switches", d.bs, d.ic, d.ih, d.iw, d.oc, d.oc1x1, d.kh,
             d.sh, d.pad_t, d.dst_dt, d.fuse_pool, ncu, per_cu, (int)g_tuning.size());
    g_case = buf;
    g_per_cu = per_cu;
    ConvPlan p;
    const char *why = nullptr;
    const int rc = plan(d, ncu, &p, &why);
    EXPECT(why != nullptr && (rc == DFX_OK) == (why[0] == 0));
    if (rc) {
      ++refused;
      return;
    }
    ++planned;
    check_plan(d, ncu, p);
    families[resident(p) ? 0 : p.variant == DFX_VARIANT_GENERIC ? 4 : p.pw ? 3 : p.direct ? 2 : 1]++;
    if (resident(p)) {
      halves += p.geom.half_from < p.geom.total_units;
      runs += p.geom.upx > 0;
    }
  };
  const int sizes[][2] = {{4, 4}, {9, 7}, {13, 13}, {28, 28}, {56, 56}, {57, 33}, {64, 64}, {30, 100}, {112, 112}, {16, 224}, {224, 224}};
  // ---- the resident kernel's class, every dst type, with and without the 1x1 stage, padding 0 / 1
  for (const auto &hw : sizes)
    for (int bs : {1, 2, 5, 64, 130})
      for (int ic : {32, 64})
        for (int oc : {32, 64})
          for (int oc1 : {0, 32, 96, 128, 256, 512})
            for (int dst : {(int)DFX_F32, (int)DFX_S32, (int)DFX_S8, (int)DFX_U8})
              for (int pad = 0; pad < 2; ++pad) {
                if ((hw[0] >= 112 || hw[1] >= 112) && (bs == 5 || bs == 130 || ic != oc)) continue;  // (keeps the sweep short)
                one(desc(bs, ic, hw[0], hw[1], oc, oc1, 3, 1, pad, dst), 256, 1);
                if (oc1 == 0 && hw[0] % 2 == 0 && hw[1] % 2 == 0 && pad == 1) one(desc(bs, ic, hw[0], hw[1], oc, 0, 3, 1, 1, dst, 2), 256, 1);
              }
  // ---- the hand-out under its switches, on other CU counts
  const char *const sw[][2] = {{"DFX_HALF_UNITS", "64"}, {"DFX_HALF_UNITS", "100000"}, {"DFX_UNIT_PX", "0"}, {"DFX_UNIT_PX", "128"},
                               {"DFX_UNIT_PX", "2048"}, {"DFX_STATIC_ROUNDS", "0"}, {"DFX_STATIC_ROUNDS", "5"}, {"DFX_NO_LAZY", "1"},
                               {"DFX_MAX_TH", "1"}, {"DFX_MAX_TH", "2"}, {"DFX_FORCE_GEOM", "2,32"}, {"DFX_FORCE_GEOM", "4,56"},
                               {"DFX_STORE_BOUND_BYTES", "64"}, {"DFX_NO_ROLES", "1"}};
  for (const auto &kv : sw) {
    g_tuning.assign(1, std::make_pair(std::string(kv[0]), std::string(kv[1])));
    for (int ncu : {8, 64, 256, 304})
      for (int bs : {1, 16, 128})
        for (int dst : {(int)DFX_F32, (int)DFX_S32, (int)DFX_U8}) {
          one(desc(bs, 64, 56, 56, 64, 256, 3, 1, 1, dst), ncu, 1);
          one(desc(bs, 64, 224, 224, 64, 128, 3, 1, 1, dst), ncu, 1);
          one(desc(bs, 32, 28, 28, 32, 0, 3, 1, 1, dst), ncu, 1);
        }
  }
  g_tuning.clear();
  // ---- the streamed, direct, pointwise and scalar kernels
  for (const auto &hw : sizes)
    for (int bs : {1, 8, 128})
      for (int ic : {16, 48, 128, 256, 2048})
        for (int oc : {16, 64, 80, 256, 512})
          for (int oc1 : {0, 64, 512})
            for (int k : {1, 3})
              for (int s : {1, 2})
                for (int dst : {(int)DFX_S32, (int)DFX_U8}) {
                  if (hw[0] * hw[1] > 60 * 60 || (long long)ic * oc > 512 * 256 || (s == 2 && dst == DFX_S32)) continue;  // (keeps the sweep short)
                  one(desc(bs, ic, hw[0], hw[1], oc, oc1, k, s, k / 2, dst), 256, bs == 8 ? 2 : 1);
                }
  for (int fv = 0; fv < 4; ++fv) {
    dfx_conv_desc d = desc(2, 32, 28, 28, 32, 64, 3, 1, 1, DFX_U8);
    d.force_variant = fv;
    one(d, 256, 2);
  }
  EXPECT(planned > 10000 && refused == 0);  // (every descriptor of the sweep is valid and none is forced)
  for (int f = 0; f < 5; ++f) EXPECT(families[f] > 0);
  EXPECT(halves > 0 && runs > 0);
  if (g_bad) {
    printf("conv_plan_check: %d checks FAILED\n", g_bad);
    return 1;
  }
  printf("conv plans: %d plans (resident %d, streamed %d, direct %d, pointwise %d, scalar %d; %d with half units, %d with pixel runs): "
         "unit counts, magic numbers, LDS layouts and the hand-out rules hold\n", planned, families[0], families[1], families[2], families[3],
         families[4], halves, runs);
  return 0;
}

int main() {
  char line[4096];
  int ncases = 0;
  while (fgets(line, sizeof(line), stdin)) {
    int32_t v[27];
    int n = 0;
    char *save = nullptr;
    g_tuning.clear();
    for (char *tok = strtok_r(line, " \t\r\n", &save); tok; tok = strtok_r(nullptr, " \t\r\n", &save)) {
      if (n < 27) {
        v[n++] = (int32_t)strtol(tok, nullptr, 10);
      } else if (char *eq = strchr(tok, '=')) {
        g_tuning.push_back(std::make_pair(std::string(tok, eq - tok), std::string(eq + 1)));
      }
    }
    if (n == 0) continue;
    ++ncases;
    if (n < 27) {
      printf("rc=-1 conv_plan_check: a case needs 25 descriptor integers, the CU count and the workgroups per CU\n");
      continue;
    }
    dfx_conv_desc d;
    static_assert(sizeof(d) == 25 * sizeof(int32_t), "dfx_conv_desc is 25 int32_t");
    memcpy(&d, v, sizeof(d));
    g_per_cu = v[26];
    ConvPlan p;
    const char *why = "";
    const int rc = plan(d, v[25], &p, &why);
    if (rc) printf("rc=%d %s\n", rc, why);
    else print_plan(p);
  }
  return ncases ? 0 : self_check();
}
