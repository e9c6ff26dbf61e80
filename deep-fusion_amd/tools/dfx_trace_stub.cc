// dfx_trace_stub.cc -- a recording fake of the C ABI (include/dfx.h): every entry point host/deepfusion.cc calls, with
// no GPU, no HIP and no arithmetic behind it.  "Device" buffers are malloc'ed, streams are small records, and every call
// that touches memory or orders streams is appended to an in-process trace (dfx_trace.h) that coherence_check.cc walks
// with vector clocks.  A *_submit records its src / lateral / dst ranges with the byte sizes of the descriptor given at
// create time; copies record both sides and do copy (so that a sanitizer build sees a wrong range); set_weights is a
// host-thread read of the borrowed tensors and a write of the handle's packed copy, which every submit reads.  Every
// other entry point -- dfx_set_device, handle create / destroy, dfx_mem_alloc_* / dfx_mem_free_*, dfx_stream_create, the
// dfx_event_* calls -- leaves a NOTE, so that --dump is the complete call sequence; a NOTE names allocation ids, byte
// counts and creation indices, never an address.
//   DFX_TRACE_DEVICES=<n>   what dfx_device_count reports (default 1), so that DEEPFUSION_DEVICES shards can be traced
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <initializer_list>
#include <string>
#include <vector>

#include "dfx.h"
#include "dfx_trace.h"

namespace {

struct allocation {
  char *base;
  size_t bytes;
  bool host, live;
};
struct stream_rec {  // never freed or reused: a stale handle cannot alias a newer stream
  int id, device;
  bool live;
};
struct handle {  // behind every dfx_*_t
  const char *op;
  std::vector<size_t> src;  // bytes of each source tensor
  size_t lat, dst;          // bytes of the tensor to add (resize) and of dst
  std::vector<size_t> wei;  // bytes of the borrowed host tensors, in set_weights' argument order (scales left out)
  int packed;               // allocation id standing for the handle's own copy of the weights
};

std::vector<allocation> g_allocs;  // index = allocation id
std::deque<stream_rec> g_streams;  // (a deque: addresses stay put)
std::vector<dfx_trace::record> g_trace;
std::vector<std::string> g_errors;
std::string g_last_error;
int g_device = 0;
int g_events = 0;

void note(const std::string &text) { g_trace.push_back({dfx_trace::NOTE, nullptr, nullptr, text, {}}); }
int stream_index(dfx_stream_t s) { return s ? static_cast<stream_rec *>(s)->id : 0; }  // creation index; 0: the default stream

int fail(int rc, const std::string &msg) {
  g_last_error = msg;
  return rc;
}
void stub_error(const std::string &msg) {
  g_errors.push_back(msg);
  g_last_error = msg;
}

size_t dt_size(int dt) { return dt == DFX_F32 || dt == DFX_S32 ? 4 : 1; }

// `what`: the entry point, for the NOTE (null: the caller writes its own)
int new_alloc(void **p, size_t bytes, bool host, const char *what) {
  char *b = static_cast<char *>(malloc(bytes ? bytes : 1));
  if (!b) return fail(DFX_ERR_HIP, "out of memory");
  g_allocs.push_back({b, bytes, host, true});
  *p = b;
  if (what) note(std::string(what) + " #" + std::to_string(g_allocs.size() - 1) + " " + std::to_string(bytes) + " bytes");
  return DFX_OK;
}
int free_alloc(void *p, bool host, const char *what) {
  if (!p) {
    if (what) note(std::string(what) + " null");
    return DFX_OK;
  }
  for (size_t i = 0; i < g_allocs.size(); ++i) {
    allocation &a = g_allocs[i];
    if (a.live && a.base == p && a.host == host) {
      a.live = false;
      free(a.base);
      if (what) note(std::string(what) + " #" + std::to_string(i));
      return DFX_OK;
    }
  }
  stub_error("free of a pointer that is no live allocation");
  return DFX_ERR_INVALID;
}
// [p, p + len) -> range of the live allocation that holds it
bool resolve(const void *p, size_t len, bool write, dfx_trace::range *out) {
  const char *c = static_cast<const char *>(p);
  for (size_t i = 0; i < g_allocs.size(); ++i) {
    const allocation &a = g_allocs[i];
    if (a.live && c >= a.base && c + len <= a.base + a.bytes) {
      *out = {static_cast<int>(i), static_cast<size_t>(c - a.base), len, write};
      return true;
    }
  }
  return false;
}
void add_range(dfx_trace::record &r, const void *p, size_t len, bool write) {
  dfx_trace::range g;
  if (!p || !len) return;
  if (resolve(p, len, write, &g)) r.ranges.push_back(g);
  else stub_error(r.name + ": " + std::to_string(len) + " bytes outside every live allocation");
}
// a stream handle the caller passes in: NULL is the default stream
bool stream_ok(dfx_stream_t s, const char *what) {
  if (!s) return true;
  for (stream_rec &t : g_streams)
    if (&t == s) {
      if (t.live) return true;
      stub_error(std::string(what) + ": stream " + std::to_string(t.id) + " was destroyed");
      return false;
    }
  stub_error(std::string(what) + ": not a stream");
  return false;
}

handle *new_handle(const char *op) {
  handle *h = new handle();
  h->op = op;
  h->lat = h->dst = 0;
  void *p = nullptr;
  new_alloc(&p, 1, false, nullptr);
  h->packed = static_cast<int>(g_allocs.size()) - 1;
  note(std::string("dfx_") + op + "_create #" + std::to_string(h->packed));
  return h;
}
int destroy_handle(void *hv) {
  handle *h = static_cast<handle *>(hv);
  if (!h) {
    note("handle destroy null");
    return DFX_OK;
  }
  note(std::string("dfx_") + h->op + "_destroy #" + std::to_string(h->packed));
  free_alloc(g_allocs[h->packed].base, false, nullptr);
  delete h;
  return DFX_OK;
}
// host-thread read of the borrowed weight / bias tensors, host-thread write of the packed copy
int set_weights(void *hv, const char *name, std::initializer_list<const void *> tensors) {
  handle *h = static_cast<handle *>(hv);
  if (!h) return fail(DFX_ERR_INVALID, "null handle");
  dfx_trace::record r{dfx_trace::HOST, nullptr, nullptr, name, {}};
  size_t i = 0;
  for (const void *t : tensors) {
    if (i < h->wei.size()) add_range(r, t, h->wei[i], false);
    ++i;
  }
  r.ranges.push_back({h->packed, 0, 1, true});
  g_trace.push_back(r);
  return DFX_OK;
}
int submit(void *hv, const char *name, const void *const *srcs, const void *lat, void *dst, dfx_stream_t s) {
  handle *h = static_cast<handle *>(hv);
  if (!h) return fail(DFX_ERR_INVALID, "null handle");
  if (!stream_ok(s, name)) return DFX_ERR_INVALID;
  dfx_trace::record r{dfx_trace::ACCESS, s, nullptr, name, {}};
  for (size_t i = 0; i < h->src.size(); ++i) add_range(r, srcs[i], h->src[i], false);
  if (lat) add_range(r, lat, h->lat, false);
  add_range(r, dst, h->dst, true);
  r.ranges.push_back({h->packed, 0, 1, false});
  g_trace.push_back(r);
  return DFX_OK;
}
int submit1(void *hv, const char *name, const void *src, void *dst, dfx_stream_t s) {
  return submit(hv, name, &src, nullptr, dst, s);
}

}  // namespace

namespace dfx_trace {
const std::vector<record> &records() { return g_trace; }
void host_access(const char *name, const void *p, size_t len, bool write) {
  record r{HOST, nullptr, nullptr, name, {}};
  add_range(r, p, len, write);
  g_trace.push_back(r);
}
const std::vector<std::string> &stub_errors() { return g_errors; }
std::string describe(const range &r) {
  return std::string(g_allocs[r.buf].host ? "host#" : "device#") + std::to_string(r.buf) + "+" + std::to_string(r.off);
}
int buffer_of(const void *p) {
  range g;
  return resolve(p, 1, false, &g) ? g.buf : -1;
}
}  // namespace dfx_trace

extern "C" {

int dfx_version(void) { return DFX_VERSION; }
const char *dfx_last_error(void) { return g_last_error.c_str(); }
int dfx_device_count(int *count) {
  const char *e = getenv("DFX_TRACE_DEVICES");
  const int n = e ? atoi(e) : 1;
  *count = n < 1 ? 1 : n;
  return DFX_OK;
}
int dfx_set_device(int ordinal) {
  note("dfx_set_device " + std::to_string(ordinal));
  int n = 1;
  dfx_device_count(&n);
  if (ordinal < 0 || ordinal >= n) return fail(DFX_ERR_NO_DEVICE, "no such device");
  g_device = ordinal;
  return DFX_OK;
}

int dfx_mem_alloc_host(void **p, size_t bytes) { return new_alloc(p, bytes, true, "dfx_mem_alloc_host"); }
int dfx_mem_free_host(void *p) { return free_alloc(p, true, "dfx_mem_free_host"); }
int dfx_mem_alloc_device(void **p, size_t bytes) { return new_alloc(p, bytes, false, "dfx_mem_alloc_device"); }
int dfx_mem_free_device(void *p) { return free_alloc(p, false, "dfx_mem_free_device"); }
int dfx_memcpy_h2d(void *dst_dev, const void *src_host, size_t bytes, dfx_stream_t s) {
  if (!stream_ok(s, "dfx_memcpy_h2d")) return DFX_ERR_INVALID;
  dfx_trace::record r{dfx_trace::ACCESS, s, nullptr, "dfx_memcpy_h2d", {}};
  add_range(r, src_host, bytes, false);
  add_range(r, dst_dev, bytes, true);
  g_trace.push_back(r);
  if (r.ranges.size() == 2) memcpy(dst_dev, src_host, bytes);
  return DFX_OK;
}
int dfx_memcpy_d2h(void *dst_host, const void *src_dev, size_t bytes, dfx_stream_t s) {
  if (!stream_ok(s, "dfx_memcpy_d2h")) return DFX_ERR_INVALID;
  dfx_trace::record r{dfx_trace::ACCESS, s, nullptr, "dfx_memcpy_d2h", {}};
  add_range(r, src_dev, bytes, false);
  add_range(r, dst_host, bytes, true);
  g_trace.push_back(r);
  if (r.ranges.size() == 2) memcpy(dst_host, src_dev, bytes);
  return DFX_OK;
}
int dfx_stream_create(dfx_stream_t *s) {
  g_streams.push_back({static_cast<int>(g_streams.size()) + 1, g_device, true});
  *s = &g_streams.back();
  note("dfx_stream_create sid " + std::to_string(g_streams.back().id) + " device " + std::to_string(g_device));
  return DFX_OK;
}
int dfx_stream_destroy(dfx_stream_t s) {
  if (!s) return DFX_OK;
  if (!stream_ok(s, "dfx_stream_destroy")) return DFX_ERR_INVALID;
  static_cast<stream_rec *>(s)->live = false;
  g_trace.push_back({dfx_trace::STREAM_DESTROY, s, nullptr, "dfx_stream_destroy", {}});
  return DFX_OK;
}
int dfx_stream_sync(dfx_stream_t s) {
  if (!stream_ok(s, "dfx_stream_sync")) return DFX_ERR_INVALID;
  g_trace.push_back({dfx_trace::SYNC, s, nullptr, "dfx_stream_sync", {}});
  return DFX_OK;
}
int dfx_stream_wait_stream(dfx_stream_t waiter, dfx_stream_t producer) {
  if (!stream_ok(waiter, "dfx_stream_wait_stream (waiter)") || !stream_ok(producer, "dfx_stream_wait_stream (producer)"))
    return DFX_ERR_INVALID;
  g_trace.push_back({dfx_trace::WAIT, waiter, producer, "dfx_stream_wait_stream", {}});
  return DFX_OK;
}
// an event is its creation index
int dfx_event_create(dfx_event_t *e) {
  *e = new int(++g_events);
  note("dfx_event_create event " + std::to_string(g_events));
  return DFX_OK;
}
int dfx_event_record(dfx_event_t e, dfx_stream_t s) {
  if (!stream_ok(s, "dfx_event_record")) return DFX_ERR_INVALID;
  note("dfx_event_record event " + std::to_string(*static_cast<int *>(e)) + " sid " + std::to_string(stream_index(s)));
  return DFX_OK;
}
int dfx_event_elapsed_ms(dfx_event_t a, dfx_event_t b, float *ms) {
  note("dfx_event_elapsed_ms event " + std::to_string(*static_cast<int *>(a)) + " event " + std::to_string(*static_cast<int *>(b)));
  *ms = 0.f;
  return DFX_OK;
}
int dfx_event_destroy(dfx_event_t e) {
  if (e) note("dfx_event_destroy event " + std::to_string(*static_cast<int *>(e)));
  delete static_cast<int *>(e);
  return DFX_OK;
}

// the layout of include/deepfusion.h: [O/16][I/16][kh][kw][(i%16)/4][o%16][i%4]
int dfx_reorder_oihw_to_blocked(const int8_t *oihw, int8_t *blocked, int O, int I, int KH, int KW) {
  if (!oihw || !blocked || O < 1 || I < 1 || O % 16 || I % 16 || KH < 1 || KW < 1) return fail(DFX_ERR_INVALID, "bad reorder");
  for (int o = 0; o < O; ++o)
    for (int i = 0; i < I; ++i)
      for (int y = 0; y < KH; ++y)
        for (int x = 0; x < KW; ++x) {
          const size_t blk = (((size_t)(o / 16) * (I / 16) + i / 16) * KH + y) * KW + x;
          blocked[blk * 256 + ((i % 16) / 4) * 64 + (o % 16) * 4 + i % 4] = oihw[(((size_t)o * I + i) * KH + y) * KW + x];
        }
  return DFX_OK;
}

// ---- conv (+ the pooling fused into it) ----
int dfx_conv_create(const dfx_conv_desc *d, dfx_conv_t **out) {
  if (!d || !out || d->bs < 1) return fail(DFX_ERR_INVALID, "bad conv descriptor");
  handle *h = new_handle("conv");
  const int oc = d->oc1x1 ? d->oc1x1 : d->oc, div = d->fuse_pool == 2 ? 2 : 1;
  h->src = {(size_t)d->bs * d->ih * d->iw * d->ic};
  h->dst = (size_t)d->bs * (d->oh / div) * (d->ow / div) * oc * dt_size(d->dst_dt);
  h->wei = {(size_t)d->oc * d->ic * d->kh * d->kw, d->bia0_dt ? d->oc * dt_size(d->bia0_dt) : 0, (size_t)d->oc1x1 * d->oc,
            d->bia1_dt ? d->oc1x1 * dt_size(d->bia1_dt) : 0};
  *out = reinterpret_cast<dfx_conv_t *>(h);
  return DFX_OK;
}
int dfx_conv_set_weights(dfx_conv_t *h, const int8_t *w0, const void *b0, const float *, const int8_t *w1, const void *b1,
                         const float *) {
  return set_weights(h, "dfx_conv_set_weights", {w0, b0, w1, b1});
}
int dfx_conv_submit(dfx_conv_t *h, const void *src, void *dst, dfx_stream_t s) { return submit1(h, "dfx_conv_submit", src, dst, s); }
int dfx_conv_destroy(dfx_conv_t *h) { return destroy_handle(h); }

int dfx_pool_create(const dfx_pool_desc *d, dfx_pool_t **out) {
  if (!d || !out) return fail(DFX_ERR_INVALID, "bad pool descriptor");
  handle *h = new_handle("pool");
  h->src = {(size_t)d->bs * d->ih * d->iw * d->c * dt_size(d->dt)};
  h->dst = (size_t)d->bs * d->oh * d->ow * d->c * dt_size(d->dt);
  *out = reinterpret_cast<dfx_pool_t *>(h);
  return DFX_OK;
}
int dfx_pool_submit(dfx_pool_t *h, const void *src, void *dst, dfx_stream_t s) { return submit1(h, "dfx_pool_submit", src, dst, s); }
int dfx_pool_destroy(dfx_pool_t *h) { return destroy_handle(h); }

// ---- concat, eltwise sum ----
int dfx_concat_create(const dfx_concat_desc *d, dfx_concat_t **out) {
  if (!d || !out || d->n_inputs < 1) return fail(DFX_ERR_INVALID, "bad concat descriptor");
  handle *h = new_handle("concat");
  const size_t px = (size_t)d->bs * d->h * d->w * dt_size(d->dt);
  for (int i = 0; i < d->n_inputs; ++i) {
    h->src.push_back(px * d->channels[i]);
    h->dst += px * d->channels[i];
  }
  *out = reinterpret_cast<dfx_concat_t *>(h);
  return DFX_OK;
}
int dfx_concat_submit(dfx_concat_t *h, const void *const *srcs, void *dst, dfx_stream_t s) {
  return submit(h, "dfx_concat_submit", srcs, nullptr, dst, s);
}
int dfx_concat_destroy(dfx_concat_t *h) { return destroy_handle(h); }

int dfx_eltwise_create(const dfx_eltwise_desc *d, dfx_eltwise_t **out) {
  if (!d || !out || d->n_inputs < 2) return fail(DFX_ERR_INVALID, "bad eltwise descriptor");
  handle *h = new_handle("eltwise");
  h->src.assign(d->n_inputs, (size_t)d->elems * dt_size(d->dt));
  h->dst = (size_t)d->elems * dt_size(d->dt);
  *out = reinterpret_cast<dfx_eltwise_t *>(h);
  return DFX_OK;
}
int dfx_eltwise_submit(dfx_eltwise_t *h, const void *const *srcs, void *dst, dfx_stream_t s) {
  return submit(h, "dfx_eltwise_submit", srcs, nullptr, dst, s);
}
int dfx_eltwise_destroy(dfx_eltwise_t *h) { return destroy_handle(h); }

// ---- reorder ----
int dfx_reorder_create(const dfx_reorder_desc *d, const float *, dfx_reorder_t **out) {
  if (!d || !out) return fail(DFX_ERR_INVALID, "bad reorder descriptor");
  handle *h = new_handle("reorder");
  const size_t px = (size_t)d->bs * d->h * d->w;
  h->src = {px * d->src_c * dt_size(d->src_dt)};
  h->dst = px * d->dst_c * dt_size(d->dst_dt);
  *out = reinterpret_cast<dfx_reorder_t *>(h);
  return DFX_OK;
}
int dfx_reorder_submit(dfx_reorder_t *h, const void *src, void *dst, dfx_stream_t s) {
  return submit1(h, "dfx_reorder_submit", src, dst, s);
}
int dfx_reorder_destroy(dfx_reorder_t *h) { return destroy_handle(h); }

// ---- concat + pointwise conv ----
int dfx_catconv_create(const dfx_catconv_desc *d, dfx_catconv_t **out) {
  if (!d || !out || d->n_inputs < 2) return fail(DFX_ERR_INVALID, "bad catconv descriptor");
  handle *h = new_handle("catconv");
  const size_t px = (size_t)d->bs * d->h * d->w;
  size_t ic = 0;
  for (int i = 0; i < d->n_inputs; ++i) {
    h->src.push_back(px * d->channels[i]);
    ic += d->channels[i];
  }
  h->dst = px * d->oc * dt_size(d->dst_dt);
  h->wei = {(size_t)d->oc * ic, d->bia_dt ? d->oc * dt_size(d->bia_dt) : 0};
  *out = reinterpret_cast<dfx_catconv_t *>(h);
  return DFX_OK;
}
int dfx_catconv_set_weights(dfx_catconv_t *h, const int8_t *w, const void *b, const float *) {
  return set_weights(h, "dfx_catconv_set_weights", {w, b});
}
int dfx_catconv_submit(dfx_catconv_t *h, const void *const *srcs, void *dst, dfx_stream_t s) {
  return submit(h, "dfx_catconv_submit", srcs, nullptr, dst, s);
}
int dfx_catconv_destroy(dfx_catconv_t *h) { return destroy_handle(h); }

// ---- the single-source conv family: depthwise, grouped, first-layer, transposed, dilated, fully-connected ----
#define DFX_STUB_CONV_FAMILY(NAME, DESC, SRC_BYTES, DST_ELEMS, WEI_BYTES, BIA_N)                                              \
  int dfx_##NAME##_create(const DESC *d, dfx_##NAME##_t **out) {                                                            \
    if (!d || !out || d->bs < 1) return fail(DFX_ERR_INVALID, "bad " #NAME " descriptor");                                  \
    handle *h = new_handle(#NAME);                                                                                           \
    h->src = {(size_t)(SRC_BYTES)};                                                                                          \
    h->dst = (size_t)(DST_ELEMS)*dt_size(d->dst_dt);                                                                         \
    h->wei = {(size_t)(WEI_BYTES), d->bia_dt ? (size_t)(BIA_N)*dt_size(d->bia_dt) : 0};                                      \
    *out = reinterpret_cast<dfx_##NAME##_t *>(h);                                                                            \
    return DFX_OK;                                                                                                           \
  }                                                                                                                          \
  int dfx_##NAME##_set_weights(dfx_##NAME##_t *h, const int8_t *w, const void *b, const float *) {                          \
    return set_weights(h, "dfx_" #NAME "_set_weights", {w, b});                                                              \
  }                                                                                                                          \
  int dfx_##NAME##_submit(dfx_##NAME##_t *h, const void *src, void *dst, dfx_stream_t s) {                                  \
    return submit1(h, "dfx_" #NAME "_submit", src, dst, s);                                                                  \
  }                                                                                                                          \
  int dfx_##NAME##_destroy(dfx_##NAME##_t *h) { return destroy_handle(h); }

DFX_STUB_CONV_FAMILY(dwconv, dfx_dwconv_desc, (size_t)d->bs * d->ih * d->iw * d->c, (size_t)d->bs * d->oh * d->ow * d->c,
                     (size_t)d->c * d->kh * d->kw, d->c)
DFX_STUB_CONV_FAMILY(gconv, dfx_gconv_desc, (size_t)d->bs * d->ih * d->iw * d->ic, (size_t)d->bs * d->oh * d->ow * d->oc,
                     (size_t)d->oc * (d->ic / (d->groups > 0 ? d->groups : 1)) * d->kh * d->kw, d->oc)
DFX_STUB_CONV_FAMILY(imgconv, dfx_imgconv_desc, (size_t)d->bs * d->ih * d->iw * d->ic, (size_t)d->bs * d->oh * d->ow * d->oc,
                     (size_t)d->oc * d->ic * d->kh * d->kw, d->oc)
DFX_STUB_CONV_FAMILY(deconv, dfx_deconv_desc, (size_t)d->bs * d->ih * d->iw * d->ic, (size_t)d->bs * d->oh * d->ow * d->oc,
                     (size_t)d->oc * d->ic * d->kh * d->kw, d->oc)
DFX_STUB_CONV_FAMILY(dilconv, dfx_dilconv_desc, (size_t)d->bs * d->ih * d->iw * d->ic, (size_t)d->bs * d->oh * d->ow * d->oc,
                     (size_t)d->oc * d->ic * d->kh * d->kw, d->oc)
DFX_STUB_CONV_FAMILY(fc, dfx_fc_desc, (size_t)d->bs * d->ih * d->iw * d->ic, (size_t)d->bs * d->oc,
                     (size_t)d->oc * d->ic * d->ih * d->iw, d->oc)
#undef DFX_STUB_CONV_FAMILY

// ---- depthwise + pointwise conv ----
int dfx_dwpw_create(const dfx_dwpw_desc *d, dfx_dwpw_t **out) {
  if (!d || !out || d->bs < 1) return fail(DFX_ERR_INVALID, "bad dwpw descriptor");
  handle *h = new_handle("dwpw");
  h->src = {(size_t)d->bs * d->ih * d->iw * d->c};
  h->dst = (size_t)d->bs * d->oh * d->ow * d->oc * dt_size(d->dst_dt);
  h->wei = {(size_t)d->c * d->kh * d->kw, d->bia0_dt ? d->c * dt_size(d->bia0_dt) : 0, (size_t)d->oc * d->c,
            d->bia1_dt ? d->oc * dt_size(d->bia1_dt) : 0};
  *out = reinterpret_cast<dfx_dwpw_t *>(h);
  return DFX_OK;
}
int dfx_dwpw_set_weights(dfx_dwpw_t *h, const int8_t *w0, const void *b0, const float *, const int8_t *w1, const void *b1,
                         const float *) {
  return set_weights(h, "dfx_dwpw_set_weights", {w0, b0, w1, b1});
}
int dfx_dwpw_submit(dfx_dwpw_t *h, const void *src, void *dst, dfx_stream_t s) { return submit1(h, "dfx_dwpw_submit", src, dst, s); }
int dfx_dwpw_destroy(dfx_dwpw_t *h) { return destroy_handle(h); }

// ---- resize (+ add) ----
int dfx_resize_create(const dfx_resize_desc *d, dfx_resize_t **out) {
  if (!d || !out || d->bs < 1) return fail(DFX_ERR_INVALID, "bad resize descriptor");
  handle *h = new_handle("resize");
  h->src = {(size_t)d->bs * d->ih * d->iw * d->c * dt_size(d->dt)};
  h->dst = (size_t)d->bs * d->oh * d->ow * d->c * dt_size(d->dt);
  h->lat = d->add ? h->dst : 0;
  *out = reinterpret_cast<dfx_resize_t *>(h);
  return DFX_OK;
}
int dfx_resize_submit(dfx_resize_t *h, const void *src, const void *add, void *dst, dfx_stream_t s) {
  return submit(h, "dfx_resize_submit", &src, add, dst, s);
}
int dfx_resize_destroy(dfx_resize_t *h) { return destroy_handle(h); }

// ---- squeeze-and-excitation (dst may be src) ----
int dfx_se_create(const dfx_se_desc *d, dfx_se_t **out) {
  if (!d || !out || d->bs < 1) return fail(DFX_ERR_INVALID, "bad se descriptor");
  handle *h = new_handle("se");
  h->src = {(size_t)d->bs * d->ih * d->iw * d->c};
  h->dst = d->mode == DFX_SE_SCALE ? h->src[0] : (size_t)d->bs * d->c;
  h->wei = {(size_t)d->cr * d->c, d->bia1_dt ? d->cr * dt_size(d->bia1_dt) : 0, (size_t)d->c * d->cr,
            d->bia2_dt ? d->c * dt_size(d->bia2_dt) : 0};
  *out = reinterpret_cast<dfx_se_t *>(h);
  return DFX_OK;
}
int dfx_se_set_weights(dfx_se_t *h, const int8_t *w1, const void *b1, const float *, const int8_t *w2, const void *b2, const float *,
                       const uint8_t *, const float *) {
  return set_weights(h, "dfx_se_set_weights", {w1, b1, w2, b2});
}
int dfx_se_submit(dfx_se_t *h, const void *src, void *dst, dfx_stream_t s) { return submit1(h, "dfx_se_submit", src, dst, s); }
int dfx_se_destroy(dfx_se_t *h) { return destroy_handle(h); }

// ---- scaled element-wise sum (dst may be an input) ----
int dfx_wsum_create(const dfx_wsum_desc *d, dfx_wsum_t **out) {
  if (!d || !out || d->bs < 1 || d->n_inputs < 1 || d->n_inputs > DFX_WSUM_MAX_INPUTS) return fail(DFX_ERR_INVALID, "bad wsum descriptor");
  handle *h = new_handle("wsum");
  const size_t elems = (size_t)d->bs * d->h * d->w * d->c;
  for (int i = 0; i < d->n_inputs; ++i) h->src.push_back(elems * dt_size(d->src_dt[i]));
  h->dst = elems * dt_size(d->dst_dt);
  *out = reinterpret_cast<dfx_wsum_t *>(h);
  return DFX_OK;
}
int dfx_wsum_set_params(dfx_wsum_t *h, const float *const *, const float *, const uint8_t *) {
  return set_weights(h, "dfx_wsum_set_params", {});
}
int dfx_wsum_submit(dfx_wsum_t *h, const void *const *srcs, void *dst, dfx_stream_t s) {
  return submit(h, "dfx_wsum_submit", srcs, nullptr, dst, s);
}
int dfx_wsum_destroy(dfx_wsum_t *h) { return destroy_handle(h); }

// ---- net head: one read (src), one write (idx or dst) and, when given, a second write (val; its bytes are kept in `lat`) ----
int dfx_head_create(const dfx_head_desc *d, dfx_head_t **out) {
  if (!d || !out || d->rows < 1 || d->c < 1 || d->src_ld < d->c) return fail(DFX_ERR_INVALID, "bad head descriptor");
  handle *h = new_handle("head");
  const bool topk = d->mode == DFX_HEAD_TOPK;
  const size_t rows = (size_t)d->rows, ld = (size_t)(topk ? d->idx_ld : d->dst_ld), cols = (size_t)(topk ? d->k : d->c);
  h->src.push_back(((rows - 1) * d->src_ld + d->c) * dt_size(d->src_dt));
  h->dst = ((rows - 1) * ld + cols) * dt_size(d->dst_dt);
  h->lat = topk ? ((rows - 1) * ld + cols) * dt_size(d->src_dt) : 0;
  *out = reinterpret_cast<dfx_head_t *>(h);
  return DFX_OK;
}
int dfx_head_set_table(dfx_head_t *h, const uint32_t *) { return set_weights(h, "dfx_head_set_table", {}); }
int dfx_head_submit(dfx_head_t *hv, const void *src, void *idx_or_dst, void *val_or_null, dfx_stream_t s) {
  handle *h = reinterpret_cast<handle *>(hv);
  if (!h) return fail(DFX_ERR_INVALID, "null handle");
  if (!stream_ok(s, "dfx_head_submit")) return DFX_ERR_INVALID;
  dfx_trace::record r{dfx_trace::ACCESS, s, nullptr, "dfx_head_submit", {}};
  add_range(r, src, h->src[0], false);
  add_range(r, idx_or_dst, h->dst, true);
  if (val_or_null) add_range(r, val_or_null, h->lat, true);
  r.ranges.push_back({h->packed, 0, 1, false});
  g_trace.push_back(r);
  return DFX_OK;
}
int dfx_head_destroy(dfx_head_t *h) { return destroy_handle(h); }

// ---- layer norm / RMS norm: one read (src), one write (dst) ----
int dfx_lnorm_create(const dfx_lnorm_desc *d, dfx_lnorm_t **out) {
  if (!d || !out || d->rows < 1 || d->c < 1 || d->src_ld < d->c || d->dst_ld < d->c) return fail(DFX_ERR_INVALID, "bad lnorm descriptor");
  handle *h = new_handle("lnorm");
  const size_t rows = (size_t)d->rows;
  h->src.push_back(((rows - 1) * d->src_ld + d->c) * dt_size(d->src_dt));
  h->dst = ((rows - 1) * d->dst_ld + d->c) * dt_size(d->dst_dt);
  *out = reinterpret_cast<dfx_lnorm_t *>(h);
  return DFX_OK;
}
int dfx_lnorm_set_params(dfx_lnorm_t *h, const float *, const float *, const uint8_t *) { return set_weights(h, "dfx_lnorm_set_params", {}); }
int dfx_lnorm_submit(dfx_lnorm_t *hv, const void *src, void *dst, dfx_stream_t s) {
  handle *h = reinterpret_cast<handle *>(hv);
  if (!h) return fail(DFX_ERR_INVALID, "null handle");
  if (!stream_ok(s, "dfx_lnorm_submit")) return DFX_ERR_INVALID;
  dfx_trace::record r{dfx_trace::ACCESS, s, nullptr, "dfx_lnorm_submit", {}};
  add_range(r, src, h->src[0], false);
  add_range(r, dst, h->dst, true);
  r.ranges.push_back({h->packed, 0, 1, false});
  g_trace.push_back(r);
  return DFX_OK;
}
int dfx_lnorm_destroy(dfx_lnorm_t *h) { return destroy_handle(h); }

// ---- window partition / reverse: one read (src), one write (dst); the row map is the handle's own ----
int dfx_window_create(const dfx_window_desc *d, dfx_window_t **out) {
  if (!d || !out || d->bs < 1 || d->h < 1 || d->w < 1 || d->c < 1 || d->wh < 1 || d->ww < 1 || d->grid_ld < d->c || d->win_ld < d->c)
    return fail(DFX_ERR_INVALID, "bad window descriptor");
  handle *h = new_handle("window");
  const size_t hp = ((size_t)d->h + d->wh - 1) / d->wh * d->wh, wp = ((size_t)d->w + d->ww - 1) / d->ww * d->ww;
  const size_t grid = (((size_t)d->bs * d->h * d->w - 1) * d->grid_ld + d->c) * dt_size(d->dt);
  const size_t win = (((size_t)d->bs * hp * wp - 1) * d->win_ld + d->c) * dt_size(d->dt);
  h->src.push_back(d->dir == DFX_WINDOW_PARTITION ? grid : win);
  h->dst = d->dir == DFX_WINDOW_PARTITION ? win : grid;
  *out = reinterpret_cast<dfx_window_t *>(h);
  return DFX_OK;
}
int dfx_window_submit(dfx_window_t *h, const void *src, void *dst, dfx_stream_t s) { return submit1(h, "dfx_window_submit", src, dst, s); }
int dfx_window_destroy(dfx_window_t *h) { return destroy_handle(h); }

// ---- token linear layer: one read (src), one write (dst); set_weights reads the borrowed weights and bias ----
int dfx_linear_create(const dfx_linear_desc *d, dfx_linear_t **out) {
  if (!d || !out || d->rows < 1 || d->k < 1 || d->n < 1 || d->src_ld < d->k || d->dst_ld < d->n) return fail(DFX_ERR_INVALID, "bad linear descriptor");
  handle *h = new_handle("linear");
  const size_t rows = (size_t)d->rows;
  h->src.push_back(((rows - 1) * d->src_ld + d->k) * dt_size(d->src_dt));
  h->dst = ((rows - 1) * d->dst_ld + d->n) * dt_size(d->dst_dt);
  h->wei = {(size_t)d->n * d->k, d->bia_dt ? (size_t)d->n * dt_size(d->bia_dt) : 0};
  *out = reinterpret_cast<dfx_linear_t *>(h);
  return DFX_OK;
}
int dfx_linear_set_weights(dfx_linear_t *h, const int8_t *w, const void *b, const float *) { return set_weights(h, "dfx_linear_set_weights", {w, b}); }
int dfx_linear_set_table(dfx_linear_t *h, const uint8_t *) { return set_weights(h, "dfx_linear_set_table", {}); }
int dfx_linear_submit(dfx_linear_t *h, const void *src, void *dst, dfx_stream_t s) { return submit1(h, "dfx_linear_submit", src, dst, s); }
int dfx_linear_destroy(dfx_linear_t *h) { return destroy_handle(h); }

// ---- patch embedding: one read (the images), one write (the token matrix); set_weights reads the borrowed weights and bias ----
int dfx_patchembed_create(const dfx_patchembed_desc *d, dfx_patchembed_t **out) {
  if (!d || !out || d->bs < 1 || d->ih < 1 || d->iw < 1 || d->ic < 1 || d->ph < 1 || d->pw < 1 || d->th < 1 || d->tw < 1 || d->oc < 1 || d->tok_offset < 0 ||
      d->img_rows < d->tok_offset + (long long)d->th * d->tw || d->dst_ld < d->oc)
    return fail(DFX_ERR_INVALID, "bad patchembed descriptor");
  handle *h = new_handle("patchembed");
  h->src.push_back((size_t)d->bs * d->ih * d->iw * d->ic);
  h->dst = (((size_t)d->bs * d->img_rows - 1) * d->dst_ld + d->oc) * dt_size(d->dst_dt);
  h->wei = {(size_t)d->oc * d->ic * d->ph * d->pw, d->bia_dt ? (size_t)d->oc * dt_size(d->bia_dt) : 0};
  *out = reinterpret_cast<dfx_patchembed_t *>(h);
  return DFX_OK;
}
int dfx_patchembed_set_weights(dfx_patchembed_t *h, const int8_t *w, const void *b, const float *) { return set_weights(h, "dfx_patchembed_set_weights", {w, b}); }
int dfx_patchembed_set_table(dfx_patchembed_t *h, const float *, int64_t) { return set_weights(h, "dfx_patchembed_set_table", {}); }
int dfx_patchembed_set_prefix(dfx_patchembed_t *h, const void *) { return set_weights(h, "dfx_patchembed_set_prefix", {}); }
int dfx_patchembed_submit(dfx_patchembed_t *h, const void *src, void *dst, dfx_stream_t s) { return submit1(h, "dfx_patchembed_submit", src, dst, s); }
int dfx_patchembed_destroy(dfx_patchembed_t *h) { return destroy_handle(h); }

// ---- image-wide top-K: reads src and the gather sources (`src`); writes idx (`dst`), val when given (`lat`), count and the
// gather destinations (this op borrows no host tensors: `wei` holds the bytes of count and of each gather destination) ----
int dfx_select_create(const dfx_select_desc *d, dfx_select_t **out) {
  if (!d || !out || d->bs < 1 || d->c < 1 || d->src_ld < d->c || d->k < 1 || d->idx_ld < d->k || d->n_gather < 0 ||
      d->n_gather > DFX_SELECT_MAX_GATHER)
    return fail(DFX_ERR_INVALID, "bad select descriptor");
  handle *h = new_handle("select");
  const size_t px = (size_t)d->bs * d->h * d->w, rows = ((size_t)d->bs - 1) * d->idx_ld + d->k;
  h->src.push_back((px - 1) * d->src_ld + d->c);
  h->dst = rows * 4;
  h->lat = rows;
  h->wei.push_back((size_t)d->bs * 4);
  for (int i = 0; i < d->n_gather; ++i) {
    h->src.push_back((px - 1) * d->pixel_stride_bytes[i] + d->row_bytes[i]);
    h->wei.push_back((size_t)d->bs * d->k * d->row_bytes[i]);
  }
  *out = reinterpret_cast<dfx_select_t *>(h);
  return DFX_OK;
}
int dfx_select_submit(dfx_select_t *hv, const void *src, void *idx, void *val_or_null, void *count, const void *const *gsrc,
                      void *const *gdst, dfx_stream_t s) {
  handle *h = reinterpret_cast<handle *>(hv);
  if (!h) return fail(DFX_ERR_INVALID, "null handle");
  if (!stream_ok(s, "dfx_select_submit")) return DFX_ERR_INVALID;
  dfx_trace::record r{dfx_trace::ACCESS, s, nullptr, "dfx_select_submit", {}};
  add_range(r, src, h->src[0], false);
  add_range(r, idx, h->dst, true);
  if (val_or_null) add_range(r, val_or_null, h->lat, true);
  add_range(r, count, h->wei[0], true);
  for (size_t i = 1; i < h->src.size(); ++i) {
    add_range(r, gsrc[i - 1], h->src[i], false);
    add_range(r, gdst[i - 1], h->wei[i], true);
  }
  r.ranges.push_back({h->packed, 0, 1, false});
  g_trace.push_back(r);
  return DFX_OK;
}
int dfx_select_destroy(dfx_select_t *h) { return destroy_handle(h); }

// ---- box decode + NMS: reads the mode's inputs (`src`, in the order boxes | idx, deltas, anchors, tab_c, tab_s; count_in when
// given: bs * 4 bytes); writes keep (`dst`), count (`wei[0]`) and boxes_out when given (`lat`) ----
int dfx_nms_create(const dfx_nms_desc *d, dfx_nms_t **out) {
  if (!d || !out || d->bs < 1 || d->n < 1 || d->max_out < 1 || d->max_out > d->n || d->keep_ld < d->max_out) return fail(DFX_ERR_INVALID, "bad nms descriptor");
  handle *h = new_handle("nms");
  const size_t e = (size_t)d->bs * d->n;
  h->src.push_back(d->mode == DFX_NMS_DECODE ? 0 : e * 16);                                                      // boxes
  h->src.push_back(d->mode == DFX_NMS_DECODE || d->per_class ? (((size_t)d->bs - 1) * d->idx_ld + d->n) * 4 : 0);  // idx
  h->src.push_back(d->mode == DFX_NMS_DECODE ? (e - 1) * d->row_bytes + 4 * (size_t)d->anchors_per_pixel : 0);    // deltas
  h->src.push_back(d->mode == DFX_NMS_DECODE ? (size_t)d->n_anchors * 16 : 0);                                   // anchors
  h->src.push_back(d->mode == DFX_NMS_DECODE ? 1024 : 0);                                                        // a table
  h->dst = (((size_t)d->bs - 1) * d->keep_ld + d->max_out) * 4;
  h->lat = (size_t)d->bs * d->max_out * 16;
  h->wei.push_back((size_t)d->bs * 4);
  *out = reinterpret_cast<dfx_nms_t *>(h);
  return DFX_OK;
}
int dfx_nms_submit(dfx_nms_t *hv, const dfx_nms_io *io, dfx_stream_t s) {
  handle *h = reinterpret_cast<handle *>(hv);
  if (!h || !io) return fail(DFX_ERR_INVALID, "null handle");
  if (!stream_ok(s, "dfx_nms_submit")) return DFX_ERR_INVALID;
  dfx_trace::record r{dfx_trace::ACCESS, s, nullptr, "dfx_nms_submit", {}};
  const void *in[6] = {io->boxes, io->idx, io->deltas, io->anchors, io->tab_c, io->tab_s};
  for (int i = 0; i < 6; ++i) {
    const size_t bytes = h->src[i < 5 ? i : 4];
    if (bytes && in[i]) add_range(r, in[i], bytes, false);
  }
  if (io->count_in) add_range(r, io->count_in, h->wei[0], false);
  add_range(r, io->keep, h->dst, true);
  add_range(r, io->count, h->wei[0], true);
  if (io->boxes_out) add_range(r, io->boxes_out, h->lat, true);
  r.ranges.push_back({h->packed, 0, 1, false});
  g_trace.push_back(r);
  return DFX_OK;
}
int dfx_nms_destroy(dfx_nms_t *h) { return destroy_handle(h); }

// ---- RoIAlign: reads the levels (`src[0 .. levels-1]`), boxes (`wei[0]`) and count or batch_idx when given (`wei[1]`);
// writes dst (`dst`) ----
int dfx_roialign_create(const dfx_roialign_desc *d, dfx_roialign_t **out) {
  if (!d || !out || d->bs < 1 || d->n < 1 || d->levels < 1 || d->levels > DFX_ROIALIGN_MAX_LEVELS || d->c < 1 || d->dst_ld < d->c || d->ph < 1 ||
      d->pw < 1)
    return fail(DFX_ERR_INVALID, "bad roialign descriptor");
  handle *h = new_handle("roialign");
  const size_t es = d->dt == DFX_F32 ? 4 : 1, rows = d->mode == DFX_ROI_LIST ? (size_t)d->n : (size_t)d->bs * d->n;
  for (int l = 0; l < d->levels; ++l) h->src.push_back((((size_t)d->bs * d->h[l] * d->w[l] - 1) * d->src_ld[l] + d->c) * es);
  h->dst = ((rows * d->ph * d->pw - 1) * d->dst_ld + d->c) * es;
  h->wei.push_back(rows * 16);
  h->wei.push_back(d->mode == DFX_ROI_LIST ? rows * 4 : (size_t)d->bs * 4);
  *out = reinterpret_cast<dfx_roialign_t *>(h);
  return DFX_OK;
}
int dfx_roialign_submit(dfx_roialign_t *hv, const dfx_roialign_io *io, dfx_stream_t s) {
  handle *h = reinterpret_cast<handle *>(hv);
  if (!h || !io) return fail(DFX_ERR_INVALID, "null handle");
  if (!stream_ok(s, "dfx_roialign_submit")) return DFX_ERR_INVALID;
  dfx_trace::record r{dfx_trace::ACCESS, s, nullptr, "dfx_roialign_submit", {}};
  for (size_t l = 0; l < h->src.size(); ++l) add_range(r, io->src[l], h->src[l], false);
  add_range(r, io->boxes, h->wei[0], false);
  if (io->count) add_range(r, io->count, h->wei[1], false);
  if (io->batch_idx) add_range(r, io->batch_idx, h->wei[1], false);
  add_range(r, io->dst, h->dst, true);
  r.ranges.push_back({h->packed, 0, 1, false});
  g_trace.push_back(r);
  return DFX_OK;
}
int dfx_roialign_destroy(dfx_roialign_t *h) { return destroy_handle(h); }

// ---- batched matrix product: reads A (`src[0]`) and B (`src[1]`), writes C (`dst`); byte ranges from the first to behind the
// last valid element of each operand, as dfx_bmm_submit's overlap check takes them ----
int dfx_bmm_create(const dfx_bmm_desc *d, dfx_bmm_t **out) {
  if (!d || !out || d->batch0 < 1 || d->batch1 < 1 || d->m < 1 || d->n < 1 || d->k < 1 || d->lda < d->k || d->ldc < d->n ||
      d->ldb < (d->trans_b ? d->k : d->n))
    return fail(DFX_ERR_INVALID, "bad bmm descriptor");
  handle *h = new_handle("bmm");
  const size_t b0 = (size_t)d->batch0 - 1, b1 = (size_t)d->batch1 - 1;
  const size_t brows = (size_t)(d->trans_b ? d->n : d->k), bcols = (size_t)(d->trans_b ? d->k : d->n);
  h->src.push_back(b0 * d->a_s0 + b1 * d->a_s1 + ((size_t)d->m - 1) * d->lda + d->k);
  h->src.push_back(b0 * d->b_s0 + b1 * d->b_s1 + (brows - 1) * d->ldb + bcols);
  h->dst = (b0 * d->c_s0 + b1 * d->c_s1 + ((size_t)d->m - 1) * d->ldc + d->n) * dt_size(d->dst_dt);
  *out = reinterpret_cast<dfx_bmm_t *>(h);
  return DFX_OK;
}
int dfx_bmm_set_scales(dfx_bmm_t *h, const float *) { return set_weights(h, "dfx_bmm_set_scales", {}); }
int dfx_bmm_set_bias(dfx_bmm_t *h, const dfx_logit_bias_desc *, const float *) { return set_weights(h, "dfx_bmm_set_bias", {}); }
int dfx_bmm_submit(dfx_bmm_t *hv, const void *a, const void *b, void *c, dfx_stream_t s) {
  handle *h = reinterpret_cast<handle *>(hv);
  if (!h) return fail(DFX_ERR_INVALID, "null handle");
  if (!stream_ok(s, "dfx_bmm_submit")) return DFX_ERR_INVALID;
  dfx_trace::record r{dfx_trace::ACCESS, s, nullptr, "dfx_bmm_submit", {}};
  add_range(r, a, h->src[0], false);
  add_range(r, b, h->src[1], false);
  add_range(r, c, h->dst, true);
  r.ranges.push_back({h->packed, 0, 1, false});
  g_trace.push_back(r);
  return DFX_OK;
}
int dfx_bmm_destroy(dfx_bmm_t *h) { return destroy_handle(h); }

// ---- fused attention: reads Q (`src[0]`), K (`src[1]`) and V (`src[2]`), writes O (`dst`); byte ranges from the first to
// behind the last valid element of each operand, as dfx_attn_submit's overlap check takes them ----
int dfx_attn_create(const dfx_attn_desc *d, dfx_attn_t **out) {
  if (!d || !out || d->batch0 < 1 || d->batch1 < 1 || d->tq < 1 || d->tk < 1 || d->d < 1 || d->dv < 1 || d->ldq < d->d || d->ldk < d->d ||
      d->ldv < d->dv || d->ldo < d->dv)
    return fail(DFX_ERR_INVALID, "bad attn descriptor");
  handle *h = new_handle("attn");
  const size_t b0 = (size_t)d->batch0 - 1, b1 = (size_t)d->batch1 - 1;
  h->src.push_back(b0 * d->q_s0 + b1 * d->q_s1 + ((size_t)d->tq - 1) * d->ldq + d->d);
  h->src.push_back(b0 * d->k_s0 + b1 * d->k_s1 + ((size_t)d->tk - 1) * d->ldk + d->d);
  h->src.push_back(b0 * d->v_s0 + b1 * d->v_s1 + ((size_t)d->tk - 1) * d->ldv + d->dv);
  h->dst = (b0 * d->o_s0 + b1 * d->o_s1 + ((size_t)d->tq - 1) * d->ldo + d->dv) * dt_size(d->dst_dt);
  *out = reinterpret_cast<dfx_attn_t *>(h);
  return DFX_OK;
}
int dfx_attn_set_table(dfx_attn_t *h, const uint32_t *) { return set_weights(h, "dfx_attn_set_table", {}); }
int dfx_attn_set_scales(dfx_attn_t *h, float, const float *) { return set_weights(h, "dfx_attn_set_scales", {}); }
int dfx_attn_set_bias(dfx_attn_t *h, const dfx_logit_bias_desc *, const float *) { return set_weights(h, "dfx_attn_set_bias", {}); }
int dfx_attn_submit(dfx_attn_t *hv, const void *q, const void *k, const void *v, void *o, dfx_stream_t s) {
  handle *h = reinterpret_cast<handle *>(hv);
  if (!h) return fail(DFX_ERR_INVALID, "null handle");
  if (!stream_ok(s, "dfx_attn_submit")) return DFX_ERR_INVALID;
  dfx_trace::record r{dfx_trace::ACCESS, s, nullptr, "dfx_attn_submit", {}};
  add_range(r, q, h->src[0], false);
  add_range(r, k, h->src[1], false);
  add_range(r, v, h->src[2], false);
  add_range(r, o, h->dst, true);
  r.ranges.push_back({h->packed, 0, 1, false});
  g_trace.push_back(r);
  return DFX_OK;
}
int dfx_attn_destroy(dfx_attn_t *h) { return destroy_handle(h); }

}  // extern "C"
