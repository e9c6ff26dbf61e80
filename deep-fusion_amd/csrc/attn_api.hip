// attn_api.hip -- host side of the fused int8 attention (dfx_attn_* of include/dfx.h): descriptor validation, the path, the
// LDS plan and the grid (all planned in attn_plan.h), the chain of the three existing ops over scratch the handle owns (made
// at create where it is the plan, at the first fallback submit on a fused handle) and the order of its submits, the device copies of the table and the out scales with both requant routes proved from the
// shape, the overlap check and the choice of the path per submit, launches.  The kernel is in attn.cuh / attn.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#include "path_op.h"
#include "attn.cuh"
#include "attn_plan.h"
#include "bias_plan.h"

namespace dfx {
int launch_attn_fused(const AttnArgs &a, int grid, int lds, hipStream_t s, int mode, bool fast_logits, bool fast_context, bool bias);
}
using namespace dfx;

struct dfx_attn {
  dfx_attn_desc d;
  int device = 0;
  int path = DFX_ATTN_CHAIN;
  bool fused_ok = false;       // the descriptor is in the fused kernel's class and the instances admit its LDS
  int grid = 0, lds = 0;       // of the fused kernel
  AttnArgs args = {};          // everything but q / k / v / o; copied per launch
  unsigned int *d_table = nullptr;
  float *d_oscale = nullptr;   // [dv rounded up to 32]
  int dv_pad = 0;
  std::atomic<int> table_set{0}, scales_set{0};
  int route_l = 0, route_o = 0;  // 0 exact, 1 fast
  // the chain: the three ops the attention is defined by, L and P in one allocation.  Made at create where the chain is the
  // plan; on a fused handle at the first submit that falls back (ensure_chain, under order.mu), from the host copies below
  dfx_bmm_t *bmm_l = nullptr, *bmm_o = nullptr;
  dfx_head_t *head = nullptr;
  unsigned char *scratch = nullptr;
  std::atomic<int> chain_ready{0};
  uint32_t table[256] = {};
  float logit_scale = 0.0f;
  std::vector<float> out_scales;
  // the logit bias (of the logits' product, bias_plan.h): the fused kernel's device image, on handles whose plan is the fused
  // kernel only (the chain's bmm_l owns its own), and, only until the chain exists, the host copy of the caller's table in
  // its own layout, from which ensure_chain gives it to the chain
  float *d_bias = nullptr;
  bool bias_set = false;
  dfx_logit_bias_desc bias = {};
  BiasScan bias_scan;
  std::vector<float> bias_host;
  TwoLaunchOrder order;
  char kernel_name[96] = "";
};

namespace {

// submits since the library was loaded, by the path that ran; process-wide (dfx_debug_attn_launches)
LaunchCounts<2> g_launches;

// (AUTO RULE with a logit bias -- include/dfx.h DFX_ATTN_AUTO_NOTE, DESIGN.md section 4.22, profiles/attn/bench_attn_bias.txt: the
// biased fused kernel beat the biased chain at every point of the unbiased rule's box and lost where the unbiased one loses,
// so the box is the same and a bias does not change the handle's plan, h->path.)
void set_name(dfx_attn *h) {
  const dfx_attn_desc &d = h->d;
  const char *which = h->path == DFX_ATTN_FUSED ? "attn_fused" : "attn_chain";
  const char *bias = h->bias_set ? " +bias" : "";
  if (!h->scales_set.load())
    snprintf(h->kernel_name, sizeof(h->kernel_name), "%s<%s,%s> (no scales)%s", which, dt_name(d.q_dt), dt_name(d.dst_dt), bias);
  else
    snprintf(h->kernel_name, sizeof(h->kernel_name), "%s<%s,%s> %s/%s%s", which, dt_name(d.q_dt), dt_name(d.dst_dt),
             h->route_l ? "fast" : "exact", h->route_o ? "fast" : "exact", bias);
}

// both routes from the shape, the scales and the bias as the handle holds them now: whichever setter came last
void prove_routes(dfx_attn *h) {
  if (!h->scales_set.load()) return;
  const dfx_attn_desc &d = h->d;
  const bool fl = h->bias_set ? bmm_fast_ok_biased(attn_bmm_logits(d), &h->logit_scale, h->bias_scan) : attn_fast_logits(d, h->logit_scale);
  h->route_l = fl && fast_allowed() ? 1 : 0;
  h->route_o = attn_fast_context(d, h->out_scales.data()) && fast_allowed() ? 1 : 0;
}

void drop_chain(dfx_attn *h) {
  (void)dfx_bmm_destroy(h->bmm_l);
  (void)dfx_bmm_destroy(h->bmm_o);
  (void)dfx_head_destroy(h->head);
  (void)hipFree(h->scratch);
  h->bmm_l = h->bmm_o = nullptr;
  h->head = nullptr;
  h->scratch = nullptr;
}

void release(dfx_attn *h) {
  if (!h) return;
  DeviceGuard dg(h->device);
  drop_chain(h);
  (void)hipFree(h->d_table);
  (void)hipFree(h->d_oscale);
  (void)hipFree(h->d_bias);
  h->order.destroy();
  delete h;
}

// the three ops and the scratch for L and P, with the table and the scales the handle has been given so far.  At create, or
// with order.mu held.  (attn_validate has found the three descriptors valid: tools/attn_plan_check holds it to that.)
int ensure_chain(dfx_attn *h) {
  if (h->chain_ready.load()) return DFX_OK;
  const dfx_attn_desc &d = h->d;
  const dfx_bmm_desc bl = attn_bmm_logits(d), bo = attn_bmm_context(d);
  const dfx_head_desc hd = attn_head_softmax(d);
  int rc;
  if ((rc = dfx_bmm_create(&bl, &h->bmm_l)) != DFX_OK || (rc = dfx_head_create(&hd, &h->head)) != DFX_OK ||
      (rc = dfx_bmm_create(&bo, &h->bmm_o)) != DFX_OK) {
    drop_chain(h);
    return rc;  // (the op that failed has recorded why)
  }
  const hipError_t e = hipMalloc((void **)&h->scratch, (size_t)attn_scratch_bytes(d));
  if (e != hipSuccess) {
    drop_chain(h);
    return fail(DFX_ERR_HIP, "attn: scratch for the logits and the probabilities: %s", hipGetErrorString(e));
  }
  if (h->table_set.load()) rc = dfx_head_set_table(h->head, h->table);
  if (rc == DFX_OK && h->scales_set.load()) rc = dfx_bmm_set_scales(h->bmm_l, &h->logit_scale);
  if (rc == DFX_OK && h->scales_set.load()) rc = dfx_bmm_set_scales(h->bmm_o, h->out_scales.data());
  if (rc == DFX_OK && h->bias_set) rc = dfx_bmm_set_bias(h->bmm_l, &h->bias, h->bias_host.data());
  if (rc != DFX_OK) {
    drop_chain(h);
    return rc;
  }
  std::vector<float>().swap(h->bias_host);  // bmm_l has it now; later set_bias calls forward to it
  h->chain_ready.store(1);
  return DFX_OK;
}

}  // namespace

extern "C" {

int dfx_attn_create(const dfx_attn_desc *desc, dfx_attn_t **out) {
  dfx_attn *h = nullptr;
  int cus = 0;
  int rc = open_create("attn", desc, out, &h, [](const dfx_attn_desc &d) { return validated("attn", attn_validate, d); }, &cus, release);
  if (rc) return rc;
  const dfx_attn_desc &d = *desc;
  // AUTO RULE (include/dfx.h DFX_ATTN_AUTO_NOTE)
  h->path = attn_path(d);
  h->fused_ok = attn_fused_class(d);
  h->grid = attn_grid(d, cus, grid_cap("DFX_ATTN_GRID"));
  h->lds = (int)std::min<long long>(attn_lds_bytes(d), ATTN_LDS_MAX);
  h->dv_pad = (int)(((long long)d.dv + 31) / 32 * 32);
  // the chain where it is the plan; a fused handle makes it at the first submit that falls back (a misaligned q, k or v),
  // so that the fused path has no scratch in HBM at all
  if (h->path == DFX_ATTN_CHAIN && (rc = ensure_chain(h)) != DFX_OK) {
    release(h);
    return rc;
  }
  hipError_t e = hipMalloc((void **)&h->d_table, HEAD_TABLE_BYTES);
  if (e == hipSuccess) e = hipMalloc((void **)&h->d_oscale, (size_t)h->dv_pad * sizeof(float));
  if (e == hipSuccess) e = h->order.create();
  if (e != hipSuccess) {
    release(h);
    return fail(DFX_ERR_HIP, "attn_create: table, scales: %s", hipGetErrorString(e));
  }
  AttnArgs &a = h->args;
  a.table = h->d_table;
  a.oscale = h->d_oscale;
  a.prob_scale = d.prob_scale;
  a.q_s0 = d.q_s0; a.q_s1 = d.q_s1; a.ldq = d.ldq;
  a.k_s0 = d.k_s0; a.k_s1 = d.k_s1; a.ldk = d.ldk;
  a.v_s0 = d.v_s0; a.v_s1 = d.v_s1; a.ldv = d.ldv;
  a.o_s0 = d.o_s0; a.o_s1 = d.o_s1; a.ldo = d.ldo;
  a.batch1 = d.batch1; a.tq = d.tq; a.tk = d.tk; a.d = d.d; a.dv = d.dv;
  a.q_u8 = d.q_dt == DFX_U8; a.dst_dt = d.dst_dt;
  a.relu = (d.relu || d.dst_dt == DFX_U8) ? 1 : 0; a.rm = d.round_mode;
  a.mt = (int)(((long long)d.tq + ATTN_STRIP - 1) / ATTN_STRIP);
  a.strips = attn_strips(d);
  a.pitch = (int)attn_pitch(d);
  a.vtiles = (int)attn_vtiles(d);  // (dv <= 2^31 - 32)
  a.kparts = attn_kparts(d);
  if (h->fused_ok) {  // more than 64 KiB of LDS is dynamic and has to be admitted per instance
    for (int r = 0; r < 8; ++r) {
      const int rc2 = launch_attn_fused(a, 0, h->lds, nullptr, 1, (r & 1) != 0, (r & 2) != 0, (r & 4) != 0);
      if (rc2 != 0) {
        (void)hipGetLastError();
        release(h);
        return fail(DFX_ERR_HIP, "attn_create: the fused kernel does not admit %d bytes of LDS", h->lds);
      }
    }
  }
  set_name(h);
  *out = h;
  return DFX_OK;
}

int dfx_attn_set_table(dfx_attn_t *h, const uint32_t *table256) {
  if (!h || !table256) return fail(DFX_ERR_INVALID, "attn_set_table: null argument");
  const char *why = "";
  const int rc = head_table_ok(table256, h->d.tk, &why);
  if (rc) return fail(rc, "attn_set_table: %s", why);
  std::lock_guard<std::mutex> lk(h->order.mu);
  if (h->chain_ready.load()) {
    const int rc2 = dfx_head_set_table(h->head, table256);
    if (rc2) return rc2;
  }
  DeviceGuard dg(h->device);
  HIP_TRY(hipMemcpy(h->d_table, table256, HEAD_TABLE_BYTES, hipMemcpyHostToDevice));
  memcpy(h->table, table256, sizeof(h->table));
  h->table_set.store(1);
  return DFX_OK;
}

int dfx_attn_set_scales(dfx_attn_t *h, float logit_scale, const float *out_scales) {
  if (!h || !out_scales) return fail(DFX_ERR_INVALID, "attn_set_scales: null argument");
  const dfx_attn_desc &d = h->d;
  std::lock_guard<std::mutex> lk(h->order.mu);
  if (h->chain_ready.load()) {
    int rc = dfx_bmm_set_scales(h->bmm_l, &logit_scale);
    if (rc == DFX_OK) rc = dfx_bmm_set_scales(h->bmm_o, out_scales);
    if (rc) return rc;
  }
  std::vector<float> img((size_t)h->dv_pad, 0.0f);  // (the entries dv .. dv_pad - 1 stay 0)
  for (int i = 0; i < d.dv; ++i) img[i] = out_scales[d.nscales == 1 ? 0 : i];
  DeviceGuard dg(h->device);
  HIP_TRY(hipMemcpy(h->d_oscale, img.data(), img.size() * sizeof(float), hipMemcpyHostToDevice));
  h->args.logit_scale = logit_scale;
  h->logit_scale = logit_scale;
  h->out_scales.assign(out_scales, out_scales + d.nscales);
  h->scales_set.store(1);
  prove_routes(h);
  set_name(h);
  return DFX_OK;
}

int dfx_attn_set_bias(dfx_attn_t *h, const dfx_logit_bias_desc *desc, const float *host_table) {
  if (!h) return fail(DFX_ERR_INVALID, "attn_set_bias: null argument");
  std::lock_guard<std::mutex> lk(h->order.mu);
  DeviceGuard dg(h->device);
  if (!desc) {  // clear: the handle gives its former bits
    if (h->chain_ready.load()) {
      const int rc = dfx_bmm_set_bias(h->bmm_l, nullptr, nullptr);
      if (rc) return rc;
    }
    (void)hipFree(h->d_bias);
    h->d_bias = nullptr;
    h->bias_set = false;
    h->args.bias = nullptr;
    std::vector<float>().swap(h->bias_host);
    prove_routes(h);
    set_name(h);
    return DFX_OK;
  }
  if (!host_table) return fail(DFX_ERR_INVALID, "attn_set_bias: null table");
  const dfx_bmm_desc bl = attn_bmm_logits(h->d);
  const char *why = "";
  int rc = bias_validate(bl, *desc, &why);
  if (rc) return fail(rc, "attn_set_bias: %s", why);
  BiasScan scan;
  if (bias_scan(bl, *desc, host_table, &scan) != DFX_OK) return fail(DFX_ERR_INVALID, "attn_set_bias: +inf or NaN in the table (finite values and -inf)");
  const bool fused_plan = h->path == DFX_ATTN_FUSED;  // (then fused_ok: attn_validate; any other handle only ever runs the chain)
  std::vector<float> img, host;
  try {
    if (!h->chain_ready.load()) host.assign(host_table, host_table + bias_host_elems(bl, *desc));
    if (fused_plan) img.resize((size_t)bias_image_elems(bl, *desc));
  } catch (const std::bad_alloc &) {
    return fail(DFX_ERR_HIP, "out of host memory");
  }
  float *fresh = nullptr;  // the handle keeps its former bias if anything below fails
  if (fused_plan) {         // the fused kernel's own image
    bias_fill_image(bl, *desc, host_table, img.data());
    hipError_t e = hipMalloc((void **)&fresh, img.size() * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(fresh, img.data(), img.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      (void)hipFree(fresh);
      return fail(DFX_ERR_HIP, "attn_set_bias: the table's image: %s", hipGetErrorString(e));
    }
  }
  if (h->chain_ready.load() && (rc = dfx_bmm_set_bias(h->bmm_l, desc, host_table)) != DFX_OK) {
    (void)hipFree(fresh);
    return rc;
  }
  (void)hipFree(h->d_bias);
  h->d_bias = fresh;
  h->bias = *desc;
  h->bias_scan = scan;
  h->bias_host.swap(host);
  h->bias_set = true;
  AttnArgs &a = h->args;
  a.bias = h->d_bias;
  a.bias_p0 = desc->period0; a.bias_p1 = desc->period1;
  a.bias_rows = (int)bias_rows(bl, *desc); a.bias_cols = (int)bias_cols(bl);
  prove_routes(h);
  set_name(h);
  return DFX_OK;
}

int dfx_attn_submit(dfx_attn_t *h, const void *q_dev, const void *k_dev, const void *v_dev, void *o_dev, dfx_stream_t s) {
  if (!h || !q_dev || !k_dev || !v_dev || !o_dev) return fail(DFX_ERR_INVALID, "attn_submit: null argument");
  if (!h->table_set.load()) return fail(DFX_ERR_STATE, "attn_submit: dfx_attn_set_table not called");
  if (!h->scales_set.load()) return fail(DFX_ERR_STATE, "attn_submit: dfx_attn_set_scales not called");
  const dfx_attn_desc &d = h->d;
  const unsigned esz = (unsigned)plan_dt_size(d.dst_dt);
  const uintptr_t pq = (uintptr_t)q_dev, pk = (uintptr_t)k_dev, pv = (uintptr_t)v_dev, po = (uintptr_t)o_dev;
  if (po % esz) return fail(DFX_ERR_INVALID, "attn_submit: o is not aligned to its element");
  const dfx_bmm_desc bl = attn_bmm_logits(d), bo = attn_bmm_context(d);
  const unsigned long long qbytes = bmm_a_elems(bl), kbytes = bmm_b_elems(bl), vbytes = bmm_b_elems(bo), obytes = bmm_c_elems(bo) * esz;
  if (plan_overlap(po, obytes, pq, qbytes) || plan_overlap(po, obytes, pk, kbytes) || plan_overlap(po, obytes, pv, vbytes))
    return fail(DFX_ERR_INVALID, "attn_submit: o overlaps q, k or v");
  DeviceGuard dg(h->device);
  // 16-byte loads need aligned operands: others take the chain for this submit
  const int path = h->path == DFX_ATTN_FUSED && h->fused_ok && (pq | pk | pv) % 16 == 0 ? DFX_ATTN_FUSED : DFX_ATTN_CHAIN;
  if (path == DFX_ATTN_FUSED) {
    AttnArgs a = h->args;  // per launch: concurrent submits on several streams are independent
    a.q = (const unsigned char *)q_dev;
    a.k = (const signed char *)k_dev;
    a.v = (const signed char *)v_dev;
    a.o = (unsigned char *)o_dev;
    a.o_vec = po % (4 * esz) == 0 && d.ldo % 4 == 0 && d.o_s0 % 4 == 0 && d.o_s1 % 4 == 0;
    if (launch_attn_fused(a, h->grid, h->lds, (hipStream_t)s, 0, h->route_l != 0, h->route_o != 0, a.bias != nullptr) != 0)
      return fail(DFX_ERR_UNSUPPORTED, "attn_submit: no kernel instance for this op");
    HIP_TRY(hipGetLastError());
  } else {
    // L and P are the handle's: chain submits take turns, on the host (mu) and on the device (TwoLaunchOrder)
    std::lock_guard<std::mutex> lk(h->order.mu);
    int rc = ensure_chain(h);
    if (rc) return rc;
    unsigned char *const l_dev = h->scratch, *const p_dev = h->scratch + attn_scratch_bytes(d) / 2;
    rc = h->order.enter((hipStream_t)s);
    if (rc == DFX_OK) rc = dfx_bmm_submit(h->bmm_l, q_dev, k_dev, l_dev, s);
    if (rc == DFX_OK) rc = dfx_head_submit(h->head, l_dev, p_dev, nullptr, s);
    if (rc == DFX_OK) rc = dfx_bmm_submit(h->bmm_o, p_dev, v_dev, o_dev, s);
    if (rc == DFX_OK) rc = h->order.leave((hipStream_t)s);
    if (rc) return rc;
  }
  g_launches.hit(path);
  return DFX_OK;
}

// test hook: how many submits have run on each path so far (shows the per-submit fallback, which query cannot)
int dfx_debug_attn_launches(int64_t out[2]) { return g_launches.read("attn", out); }

int dfx_attn_query(const dfx_attn_t *h, dfx_attn_info *info) {
  if (const int rc = open_query("attn", h, info)) return rc;
  const bool fused = h->path == DFX_ATTN_FUSED;
  info->grid = fused ? h->grid : 0;
  info->block = fused ? ATTN_THREADS : 0;
  info->lds_bytes = fused ? h->lds : 0;
  info->route_logits = h->scales_set.load() ? h->route_l : -1;
  info->route_context = h->scales_set.load() ? h->route_o : -1;
  info->scratch_bytes = h->chain_ready.load() ? attn_scratch_bytes(h->d) : 0;
  info->algorithmic_ops = attn_algorithmic_ops(h->d);
  info->algorithmic_bytes = attn_algorithmic_bytes(h->d) + (h->bias_set ? bias_distinct_bytes(attn_bmm_logits(h->d), h->bias) : 0);
  return DFX_OK;
}

int dfx_attn_destroy(dfx_attn_t *h) {
  release(h);
  return DFX_OK;
}

}  // extern "C"
