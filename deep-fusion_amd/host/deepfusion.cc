// deepfusion.cc -- implementation of include/deepfusion.h on top of the C ABI
// (include/dfx.h, libdfx_hip.so).  Host-side counterpart of the reference's
//   src/deepfusion.cc   memory, op::submit, the dtype-switch factories (:59-185)
//   src/op_conv.h       construction-time checks + buffer capture (:34-96)
//   src/op_concat.h     (:28-61)
//   util/memory.cc      aligned_malloc/free (:21-40)   -> pinned host + device buffers
//   util/log.h          error_and_exit (:38-42)        -> same exit-on-failure behaviour
// One op::submit() is one kernel launch on the op's HIP stream (the reference
// runs OpenMP loops of per-row JIT calls, op_conv.cc:140-260).
#include "deepfusion.h"

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "dfx.h"

namespace deepfusion {

namespace {

[[noreturn]] void error_and_exit(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  fprintf(stderr, "[deepfusion] ");
  vfprintf(stderr, fmt, ap);
  fprintf(stderr, "\n");
  va_end(ap);
  exit(EXIT_FAILURE);  // reference: util/log.h:38-42
}

void check_dfx(int rc, const char *what) {
  if (rc != DFX_OK) error_and_exit("%s failed (%d): %s", what, rc, dfx_last_error());
}

size_t dtype_size(memory::dtype dt) {  // util/memory.cc:42-56
  switch (dt) {
    case memory::dtype::f32:
    case memory::dtype::s32: return 4;
    case memory::dtype::s8:
    case memory::dtype::u8: return 1;
    default: error_and_exit("Unknown data type");
  }
}

int to_dfx_dtype(memory::dtype dt) { return static_cast<int>(dt); }  // same numbering

// logical nchw -> physical dim order (reference deepfusion.cc:25-57)
memory::dims physical_dims(const memory::nchw_dims &dm, memory::format fmt) {
  switch (fmt) {
    case memory::format::nhwc: return {dm[0], dm[2], dm[3], dm[1]};
    case memory::format::nchw:
    case memory::format::OIhw4i16o4i:
    case memory::format::gOIhw4i16o4i: return {dm[0], dm[1], dm[2], dm[3]};
    default: error_and_exit("bad type");
  }
}

}  // namespace

// ---------------------------------------------------------------------------
// memory
// ---------------------------------------------------------------------------

namespace detail {

struct memory_state {
  void *host = nullptr;    // pinned
  void *device = nullptr;  // lazily allocated
  size_t bytes = 0;
  unsigned long long host_version = 1;      // bumped by every data() call
  unsigned long long uploaded_version = 0;  // host_version the device copy reflects
  dfx_stream_t producer = nullptr;          // stream of the op whose launch, possibly still in flight, last wrote the
                                            // device copy; cleared once that stream has been synchronised
  std::vector<dfx_stream_t> readers;        // streams of the ops whose launches, possibly still in flight, have read the
                                            // device copy since that write (the producer's own stream is not listed: a
                                            // stream is in order); a stream leaves when it is synchronised or destroyed
  bool device_ahead = false;                // the device copy is NEWER than the host bytes (written by an op and
                                            // not downloaded yet): an upload would destroy it
};

// FNV-1a over 8-byte words (+ tail): the trigger for re-packing borrowed weight tensors.  The
// reference reads the caller's host buffers on every submit(); here a submit() hashes them
// (~15 us for the headline op's 53 KB) and re-packs only when the bytes really changed.
inline unsigned long long hash_bytes(const void *p, size_t n, unsigned long long h) {
  const unsigned char *b = static_cast<const unsigned char *>(p);
  size_t i = 0;
  for (; i + 8 <= n; i += 8) {
    unsigned long long w;
    memcpy(&w, b + i, 8);
    h = (h ^ w) * 1099511628211ull;
  }
  for (; i < n; ++i) h = (h ^ b[i]) * 1099511628211ull;
  return h;
}

// DEEPFUSION_PROFILE=1 (the env flag the reference reads, util/scaffold.cc:56-82): op::submit()
// prints "<name> infer <ms>" like the reference's timing wrapper (deepfusion.cc:91-102)
inline bool profiling_enabled() {
  static const bool on = [] {
    const char *e = getenv("DEEPFUSION_PROFILE");
    return e && atoi(e) != 0;
  }();
  return on;
}

// Multi-device submit(): DEEPFUSION_DEVICES=<n>|all splits an op's batch into n contiguous shards
// (the split the reference makes over OpenMP threads, op_conv.cc:155-156 balance211), shard i on
// visible device i % device_count with its own handle, stream and device buffers.  n may exceed the
// device count (several shards per device): that is how the sharded path is exercised on a one-GPU
// box.  Unset or 1: the single-device path.
inline int requested_shards() {
  static const int n = [] {
    const char *e = getenv("DEEPFUSION_DEVICES");
    if (!e || !*e) return 1;
    int cnt = 1;
    if (dfx_device_count(&cnt) != DFX_OK || cnt < 1) cnt = 1;
    if (!strcmp(e, "all")) return cnt;
    const int v = atoi(e);
    return v < 1 ? 1 : v;
  }();
  return n;
}
struct shard_range { int device, n0, n; };
inline std::vector<shard_range> plan_shards(int batch) {
  std::vector<shard_range> v;
  int want = requested_shards();
  if (want > batch) want = batch;
  if (want <= 1) return v;  // empty: single-device path
  int cnt = 1;
  if (dfx_device_count(&cnt) != DFX_OK || cnt < 1) cnt = 1;
  const int base = batch / want, rem = batch % want;
  int n0 = 0;
  for (int i = 0; i < want; ++i) {
    const int n = base + (i < rem ? 1 : 0);
    v.push_back({i % cnt, n0, n});
    n0 += n;
  }
  return v;
}

// shared plumbing of the ops (op_base holds one): access to the tensors' private state
struct op_state {
  dfx_stream_t stream = nullptr;

  static memory_state *st(memory &m) { return m.st_; }

  void ensure_stream() {
    if (!stream) check_dfx(dfx_stream_create(&stream), "stream create");
  }
  // The tensors in which this op's stream is registered as producer or reader.  Tensors outlive the ops built from them
  // (deepfusion.h), so the pointers stay valid for the op's life.
  std::vector<memory_state *> touched;
  void touch(memory_state *s) {
    for (memory_state *t : touched)
      if (t == s) return;
    touched.push_back(s);
  }
  // This op's stream is about to WRITE the device copy of s (a kernel's output or an upload): order it behind every launch
  // on another stream that still reads the copy (write after read) or wrote it last (write after write), then own it.
  void before_write(memory_state *s) {
    bool was_reader = false;  // then sync_in() has waited for this producer already (every write clears the list)
    for (dfx_stream_t r : s->readers) {
      if (r != stream) check_dfx(dfx_stream_wait_stream(stream, r), "stream wait");
      else was_reader = true;
    }
    s->readers.clear();
    if (s->producer && s->producer != stream && !was_reader) check_dfx(dfx_stream_wait_stream(stream, s->producer), "stream wait");
    s->producer = stream;
    touch(s);
  }
  // Make the device copy of input `m` current; returns the device pointer.
  // always == true is the reference-compatible submit(): the caller may have refilled the host
  // buffer through a pointer it fetched once (the reference reads host memory on every submit),
  // so the (pinned) host bytes are uploaded every time -- unless the device copy is the NEWER one
  // (an op wrote it with submit_async() and nobody has called data() since: the host bytes are
  // stale, uploading them would overwrite the producer's result).  The asynchronous extension path
  // (submit_async / upload / device_data) skips the copy while no data() call has bumped the
  // version, and orders itself behind the op that produced the device copy on another stream.
  // An upload is a write of the device copy like any other (before_write); a plain read registers
  // this stream in `readers`, so that the next writer on another stream waits for it.
  void *sync_in(memory &m, bool always) {
    memory_state *s = m.st_;
    if (!s->device) check_dfx(dfx_mem_alloc_device(&s->device, s->bytes), "device alloc");
    const bool host_touched = s->uploaded_version != s->host_version;
    if (host_touched || (always && !s->device_ahead)) {
      before_write(s);
      check_dfx(dfx_memcpy_h2d(s->device, s->host, s->bytes, stream), "H2D copy");
      s->uploaded_version = s->host_version;
      s->device_ahead = false;
    } else if (s->producer != stream) {
      if (s->producer) check_dfx(dfx_stream_wait_stream(stream, s->producer), "stream wait");
      bool listed = false;
      for (dfx_stream_t r : s->readers) listed = listed || r == stream;
      if (!listed) s->readers.push_back(stream);
      touch(s);
    }
    return s->device;
  }
  void *device_out(memory &m) {
    memory_state *s = m.st_;
    if (!s->device) check_dfx(dfx_mem_alloc_device(&s->device, s->bytes), "device alloc");
    before_write(s);  // (an op whose input is also its output, resize_add(lateral = dst), does not wait on itself)
    s->uploaded_version = s->host_version;  // the device copy is about to become the newer one
    s->device_ahead = true;
    return s->device;
  }
  // forget this op's stream in every tensor it is registered in
  void unregister() {
    for (memory_state *s : touched) {
      if (s->producer == stream) s->producer = nullptr;
      for (size_t i = 0; i < s->readers.size();)
        if (s->readers[i] == stream) s->readers.erase(s->readers.begin() + i);
        else ++i;
    }
    touched.clear();
  }
  // this op's stream has just been synchronised: nothing it launched is still writing its output or reading its inputs;
  // ops on other streams need not (and, once this op is gone, could not) wait on it
  void settled() { unregister(); }
  // the op is being destroyed while a launch of it may still be writing its output or reading an input (the reference
  // only asks that tensors outlive ops): finish that work, then forget the stream -- it is about to be destroyed
  void retire() {
    if (stream && !touched.empty()) {
      dfx_stream_sync(stream);
      unregister();
    }
  }
  // device-side duration of what infer() enqueued, printed like the reference's profiling wrapper
  dfx_event_t ev0 = nullptr, ev1 = nullptr;
  void profile_begin() {
    if (!profiling_enabled()) return;
    if (!ev0) {
      check_dfx(dfx_event_create(&ev0), "event create");
      check_dfx(dfx_event_create(&ev1), "event create");
    }
    check_dfx(dfx_event_record(ev0, stream), "event record");
  }
  void profile_end(const char *name) {
    if (!profiling_enabled()) return;
    check_dfx(dfx_event_record(ev1, stream), "event record");
    float ms = 0.f;
    check_dfx(dfx_event_elapsed_ms(ev0, ev1, &ms), "event elapsed");
    printf("%s infer %.4f ms\n", name, ms);
  }
  // the op has just (re)written m on the device: the host copy is stale until downloaded
  void fetch_out(memory &m) {
    memory_state *s = m.st_;
    check_dfx(dfx_memcpy_d2h(s->host, s->device, s->bytes, stream), "D2H copy");
    s->uploaded_version = s->host_version;  // host == device after the copy
    s->device_ahead = false;
  }
  // sharded submit wrote m's HOST buffer directly: any device copy is stale
  static void host_is_current(memory &m) {
    m.st_->uploaded_version = 0;
    m.st_->producer = nullptr;
    m.st_->device_ahead = false;
  }
  // the events and the stream go (op_base::teardown, before the tensors a derived class owns)
  void close() {
    if (ev0) dfx_event_destroy(ev0);
    if (ev1) dfx_event_destroy(ev1);
    if (stream) dfx_stream_destroy(stream);
    ev0 = ev1 = nullptr;
    stream = nullptr;
  }
  ~op_state() { close(); }
};

}  // namespace detail

memory::memory(const nchw_dims &dm, const format fmt, const dtype dt, int alignment)
    : st_(nullptr), std_dims_(dm), fmt_(fmt), dt_(dt) {
  dims_ = physical_dims(dm, fmt);
  allocate_buffer(alignment);
}

memory::memory(const dims &dm, const format fmt, const dtype dt, int alignment)
    : st_(nullptr), dims_(dm), fmt_(fmt), dt_(dt) {
  // the reference leaves std_dims_ uninitialised here although bias checks read
  // it; give it the obvious meaning for 1-D tensors
  std_dims_ = {dm.size() > 0 ? dm[0] : 0, dm.size() > 1 ? dm[1] : 1, dm.size() > 2 ? dm[2] : 1,
               dm.size() > 3 ? dm[3] : 1};
  allocate_buffer(alignment);
}

memory::~memory() {
  if (!st_) return;
  dfx_mem_free_host(st_->host);
  dfx_mem_free_device(st_->device);
  delete st_;
}

void memory::allocate_buffer(int /*alignment: pinned allocations are page aligned*/) {
  if (buffer_size() == 0) error_and_exit("memory: empty buffer");
  st_ = new detail::memory_state();
  st_->bytes = buffer_size();
  check_dfx(dfx_mem_alloc_host(&st_->host, st_->bytes), "pinned host alloc");
}

size_t memory::size() {
  size_t n = 1;
  for (int d : dims_) n *= static_cast<size_t>(d);
  return n;
}

size_t memory::buffer_size() { return size() * dtype_size(dt_); }

void *memory::data() {
  ++st_->host_version;  // the caller may write through the pointer
  return st_->host;
}
const void *memory::host_data() const { return st_->host; }
unsigned long long memory::host_version() const { return st_->host_version; }

void *memory::device_data() {
  if (!st_->device) check_dfx(dfx_mem_alloc_device(&st_->device, st_->bytes), "device alloc");
  return st_->device;
}
void memory::upload() {
  // the copy overwrites the device buffer: launches that still read or write it finish first
  for (dfx_stream_t r : st_->readers) check_dfx(dfx_stream_sync(r), "stream sync");
  st_->readers.clear();
  if (st_->producer) {
    check_dfx(dfx_stream_sync(st_->producer), "stream sync");
    st_->producer = nullptr;
  }
  check_dfx(dfx_memcpy_h2d(device_data(), st_->host, st_->bytes, nullptr), "H2D copy");
  check_dfx(dfx_stream_sync(nullptr), "sync");
  st_->uploaded_version = st_->host_version;
  st_->device_ahead = false;
}
void memory::download() {
  if (!st_->device) return;  // no device copy exists (e.g. batch-sharded ops work host to host): the host bytes are current
  if (st_->producer) {  // the op that wrote the device copy may still be running on its own stream
    check_dfx(dfx_stream_sync(st_->producer), "stream sync");
    st_->producer = nullptr;
  }
  check_dfx(dfx_memcpy_d2h(st_->host, device_data(), st_->bytes, nullptr), "D2H copy");
  check_dfx(dfx_stream_sync(nullptr), "sync");
  st_->uploaded_version = st_->host_version;
  st_->device_ahead = false;
}

// ---------------------------------------------------------------------------
// op base
// ---------------------------------------------------------------------------

void op::submit() { infer(); }
void op::submit_async() { infer(); }
void op::wait() {}

namespace {

int to_dfx_round(round_mode rm) { return rm == round_mode::down ? DFX_ROUND_DOWN : DFX_ROUND_NEAREST; }

// a dfx_*_destroy as a function of the opaque handle that op_base keeps
template <class H, int (*Destroy)(H *)>
int destroy_as(void *h) {
  return Destroy(static_cast<H *>(h));
}
// a dfx_*_create that takes (descriptor, handle): `fmt` is the class's "Init ... op failed! (%s)"
template <class H, class D>
void *create_or_exit(int (*create)(const D *, H **), const D &d, const char *fmt) {
  H *h = nullptr;
  if (create(&d, &h) != DFX_OK) error_and_exit(fmt, dfx_last_error());
  return h;
}

// ---- what every op class shares: submit / submit_async / wait / infer, the single-device run, the batch shards of
// DEEPFUSION_DEVICES, the profile brackets and the borrowed-weights protocol.  A derived class validates, fills its
// descriptor and then says, in its constructor:
//   reads(m, bytes per image [, own])   the tensors a launch reads, in the order launch() gets their device pointers.  m may be
//                                       null (an optional tensor: the slot stays, its pointer is null).  own: a tensor of the op
//                                       itself that no caller can refill behind data()'s back -- even submit() trusts its version
//                                       counter and uploads it once
//   writes(m, bytes per image)          the tensors it writes.  The order is at once the order of device_out(), of the copies back
//                                       in submit() and of a shard's downloads
//   borrows(m)                          a host tensor of the caller's that pack() reads (weights, biases); null is skipped.  None
//                                       at all: nothing is ever packed (squeeze_excite's pool-only mode, every op without weights)
//   build(batch, create)                LAST: create(n) makes a handle for n images on the current device, with whatever follows
//                                       a create (set_params, set_table).  batch > 0: the class shards over that many images,
//                                       tensors are batch-major and bytes per image must be given.  0: one handle on one device
// and overrides pack(handle) and launch(handle, pointers, stream): pointers are the reads', then the writes'.  The base
// constructor takes the handle's destroy function (a destructor cannot call down into a derived class). ----
class op_base : public op {
public:
  ~op_base() override { teardown(); }

  void submit() override {
    if (!shards_.empty()) {
      enqueue_shards();
      sync_shards();
      return;
    }
    run(true);
    fetch_outputs();
    check_dfx(dfx_stream_sync(st_.stream), "stream sync");
    st_.settled();
  }
  // (sharded: host in -> host out like submit(), without the final wait; the device-resident
  // chaining extension is single-device)
  void submit_async() override {
    if (!shards_.empty()) {
      enqueue_shards();
      return;
    }
    run(false);
    if (fetch_on_async_ && detail::requested_shards() > 1) fetch_outputs();
  }
  void wait() override {
    if (!shards_.empty()) {
      sync_shards();
    } else {
      check_dfx(dfx_stream_sync(st_.stream), "stream sync");
      st_.settled();
    }
  }

protected:
  explicit op_base(int (*destroy)(void *)) : destroy_(destroy) {}

  void reads(memory *m, size_t img = 0, bool own = false) { reads_.push_back(tensor{m, img, own}); }
  void writes(memory *m, size_t img = 0) { writes_.push_back(tensor{m, img, false}); }
  void borrows(memory *m) {
    if (m) weights_.push_back(m);
  }
  size_t n_reads() const { return reads_.size(); }

  template <class Create>
  void build(int batch, Create create) {
    if (batch > 0) {
      for (const detail::shard_range &r : detail::plan_shards(batch)) {
        shard sh;
        sh.r = r;
        check_dfx(dfx_set_device(r.device), "set device");
        sh.h = create(r.n);
        check_dfx(dfx_stream_create(&sh.stream), "stream create");
        for (const std::vector<tensor> *list : {&reads_, &writes_})
          for (const tensor &t : *list) {
            void *p = nullptr;
            if (t.m) check_dfx(dfx_mem_alloc_device(&p, (size_t)r.n * t.img), "device alloc");
            sh.buf.push_back(p);
          }
        shards_.push_back(sh);
      }
    }
    if (!shards_.empty()) {
      check_dfx(dfx_set_device(shards_[0].r.device), "set device");
      return;
    }
    h_ = create(batch);
    ptr_.resize(reads_.size() + writes_.size());
    st_.ensure_stream();
  }
  // What a destructor does, in the order the C ABI sees it: per shard set device, handle, stream, input buffers, output
  // buffers; back to the first shard's device; wait for a launch that is still in flight (retire); the handle; the events
  // and the stream.  The destructor calls it; a class that owns tensors its launches read (op_nms) calls it from its own
  // destructor, before those tensors go.  The second call does nothing.
  void teardown() {
    if (torn_down_) return;
    torn_down_ = true;
    for (shard &sh : shards_) {
      dfx_set_device(sh.r.device);
      destroy_(sh.h);
      dfx_stream_destroy(sh.stream);
      for (void *p : sh.buf) dfx_mem_free_device(p);
    }
    if (!shards_.empty()) dfx_set_device(shards_[0].r.device);
    st_.retire();
    destroy_(h_);
    st_.close();
  }

  void infer() override {
    if (!shards_.empty()) enqueue_shards();
    else run(true);
  }
  // set_weights (and its like) on `h` from the borrowed tensors; only called when there are any
  virtual void pack(void * /*handle*/) {}
  // enqueue the op on `s`: p[0 .. reads) are the device pointers of the reads, p[reads ..) of the writes, null where absent
  virtual void launch(void *handle, void *const *p, dfx_stream_t s) = 0;

  // OPTION (op_conv_pool, op_eltwise): under DEEPFUSION_DEVICES > 1 submit_async() also copies the result to the host, where
  // a sharded neighbour, which works host to host, finds it after wait().  The other classes that do not shard leave the
  // result on the device; the difference is historical and kept as it is.
  bool fetch_on_async_ = false;

private:
  struct tensor {
    memory *m;
    size_t img;  // bytes per image (sharding classes)
    bool own;
  };
  struct shard {
    detail::shard_range r;
    void *h = nullptr;
    dfx_stream_t stream = nullptr;
    std::vector<void *> buf;  // this shard's images of every read, then of every write; null where the tensor is absent
    unsigned long long wei_seen = 0;  // hash of the weights the handle was packed from
  };

  unsigned long long weights_hash() const {
    unsigned long long v = 1469598103934665603ull;
    for (memory *m : weights_) v = detail::hash_bytes(m->host_data(), m->buffer_size(), v);
    return v | 1ull;  // (never 0 = "nothing packed yet")
  }
  unsigned long long weights_versions() const {
    unsigned long long v = 0;
    for (memory *m : weights_) v += m->host_version();
    return v;
  }
  void fetch_outputs() {
    for (const tensor &t : writes_)
      if (t.m) st_.fetch_out(*t.m);
  }
  // every shard: upload its images from the host tensors, launch, download into the host tensors
  void enqueue_shards() {
    const unsigned long long v = weights_.empty() ? 0 : weights_hash();
    for (shard &sh : shards_) {
      check_dfx(dfx_set_device(sh.r.device), "set device");
      if (!weights_.empty() && v != sh.wei_seen) {
        check_dfx(dfx_stream_sync(sh.stream), "stream sync");
        pack(sh.h);
        sh.wei_seen = v;
      }
      size_t k = 0;
      for (const tensor &t : reads_) {
        if (t.m)
          check_dfx(dfx_memcpy_h2d(sh.buf[k], static_cast<const char *>(t.m->host_data()) + sh.r.n0 * t.img, sh.r.n * t.img, sh.stream),
                    "H2D copy");
        ++k;
      }
      launch(sh.h, sh.buf.data(), sh.stream);
      for (const tensor &t : writes_) {
        if (t.m)
          check_dfx(dfx_memcpy_d2h(static_cast<char *>(const_cast<void *>(t.m->host_data())) + sh.r.n0 * t.img, sh.buf[k], sh.r.n * t.img,
                                   sh.stream),
                    "D2H copy");
        ++k;
      }
    }
    check_dfx(dfx_set_device(shards_[0].r.device), "set device");
    for (const tensor &t : writes_)
      if (t.m) detail::op_state::host_is_current(*t.m);
  }
  void sync_shards() {
    for (shard &sh : shards_) {
      check_dfx(dfx_set_device(sh.r.device), "set device");
      check_dfx(dfx_stream_sync(sh.stream), "stream sync");
    }
    check_dfx(dfx_set_device(shards_[0].r.device), "set device");
  }
  // sync_host == true: reference semantics (host buffers are re-read: inputs uploaded, weights
  // re-packed when their bytes changed).  false: the asynchronous device-resident extension,
  // which trusts the data() version counters.
  void run(bool sync_host) {
    // weights are borrowed host tensors the caller may rewrite between submits (the reference
    // re-reads them on every call).  What the handle holds is described by TWO values taken at pack
    // time: the hash of the packed bytes and the sum of the tensors' data() counters.  submit() re-reads
    // the bytes (hash); submit_async() trusts the counters, and only when they moved looks at the bytes.
    if (!weights_.empty()) {
      const unsigned long long vers = weights_versions();
      if (sync_host || vers != packed_versions_) {
        const unsigned long long hash = weights_hash();
        if (hash != packed_hash_) {
          check_dfx(dfx_stream_sync(st_.stream), "stream sync");  // no launch may still read the old copy
          pack(h_);
          packed_hash_ = hash;
        }
        packed_versions_ = vers;
      }
    }
    // (a tensor may be read and written: resize_add's lateral, scaled_sum's and squeeze_excite's src -- uploaded, then overwritten)
    size_t k = 0;
    for (const tensor &t : reads_) ptr_[k++] = t.m ? st_.sync_in(*t.m, sync_host && !t.own) : nullptr;
    for (const tensor &t : writes_) ptr_[k++] = t.m ? st_.device_out(*t.m) : nullptr;
    st_.profile_begin();
    launch(h_, ptr_.data(), st_.stream);
    st_.profile_end(name());
  }

  int (*destroy_)(void *);
  detail::op_state st_;
  std::vector<tensor> reads_, writes_;
  std::vector<memory *> weights_;
  void *h_ = nullptr;                                         // the single-device handle; null when sharded
  unsigned long long packed_hash_ = 0, packed_versions_ = 0;  // what h_ was packed from (see run())
  std::vector<void *> ptr_;                                   // run()'s device pointers, sized once
  std::vector<shard> shards_;  // DEEPFUSION_DEVICES > 1: one entry per batch shard; empty otherwise
  bool torn_down_ = false;
};

// ---- conv: replaces op_conv<T> ----
class op_conv : public op_base {
public:
  op_conv(const std::unique_ptr<memory> &src, const std::unique_ptr<memory> &wei,
          const std::unique_ptr<memory> &bia, std::array<int, 2> stride, std::array<int, 2> pad,
          std::unique_ptr<memory> &dst, const std::vector<float> &scales0,
          const std::vector<float> &scales1, const std::unique_ptr<memory> &wei1x1,
          const std::unique_ptr<memory> &bia1x1, bool relu0, bool relu1, round_mode rm0,
          round_mode rm1)
      : op_base(destroy_as<dfx_conv_t, dfx_conv_destroy>), src_(src.get()), wei_(wei.get()), bia_(bia.get()), wei1_(wei1x1.get()), bia1_(bia1x1.get()),
        dst_(dst.get()), scales0_(scales0), scales1_(scales1) {
    using fmt = memory::format;
    if (!src_ || !wei_ || !dst_) error_and_exit("Init Conv op failed! (null tensor)");
    // dtype / format gate of jit_conv_kernel::init_conf (jit_conv_kernel.cc:531-564)
    bool ok = src_->data_type() == memory::dtype::u8 && wei_->data_type() == memory::dtype::s8 &&
              (!wei1_ || wei1_->data_type() == memory::dtype::s8) && src_->dim_format() == fmt::nhwc &&
              dst_->dim_format() == fmt::nhwc &&
              (wei_->dim_format() == fmt::OIhw4i16o4i || wei_->dim_format() == fmt::gOIhw4i16o4i) &&
              (!wei1_ || wei1_->dim_format() == fmt::OIhw4i16o4i ||
               wei1_->dim_format() == fmt::gOIhw4i16o4i) &&
              (!bia_ || bia_->dim_format() == fmt::x) && (!bia1_ || bia1_->dim_format() == fmt::x);
    if (!ok) error_and_exit("Init Conv op failed! (data type / format)");
    auto s = src_->std_dims(), w = wei_->std_dims(), o = dst_->std_dims();
    // shape checks of op_conv<T>::init_conf (op_conv.cc:286-346)
    if (s[0] != o[0]) error_and_exit("Init Conv op failed! (Batch size do not equal)");
    if (s[1] != w[1]) error_and_exit("Init Conv op failed! (Input channel do not match)");
    dfx_conv_desc d;
    memset(&d, 0, sizeof(d));
    d.bs = s[0]; d.ic = s[1]; d.ih = s[2]; d.iw = s[3];
    d.oc = w[0]; d.kh = w[2]; d.kw = w[3];
    d.oh = o[2]; d.ow = o[3];
    d.sh = stride[0]; d.sw = stride[1]; d.pad_t = pad[0]; d.pad_l = pad[1];
    if (wei1_) {
      auto w1 = wei1_->std_dims();
      if (w1[1] != w[0]) error_and_exit("Init Conv op failed! (Conv0 output channel do not match)");
      if (o[1] != w1[0]) error_and_exit("Init Conv op failed! (Conv1x1 output channel do not match)");
      if (w1[2] != 1 || w1[3] != 1) error_and_exit("Init Conv op failed! (Fused conv must be 1x1 kernel)");
      if (bia1_ && (int)bia1_->size() != o[1]) error_and_exit("Init Conv op failed! (Bias channel do not match)");
      d.oc1x1 = w1[0];
    } else {
      if (o[1] != w[0]) error_and_exit("Init Conv op failed! (Output channel do not match)");
    }
    if (bia_ && (int)bia_->size() != w[0]) error_and_exit("Init Conv op failed! (Bias channel do not match)");
    d.dst_dt = to_dfx_dtype(dst_->data_type());
    d.bia0_dt = bia_ ? to_dfx_dtype(bia_->data_type()) : DFX_UNDEF;
    d.bia1_dt = bia1_ ? to_dfx_dtype(bia1_->data_type()) : DFX_UNDEF;
    d.conv0_relu = relu0; d.conv1_relu = relu1;
    d.conv0_round_mode = to_dfx_round(rm0);
    d.conv1_round_mode = to_dfx_round(rm1);
    d.conv0_nscales = (int)scales0_.size();
    d.conv1_nscales = wei1_ ? (int)scales1_.size() : 1;
    d.force_variant = -1;
    const size_t src_img = (size_t)d.ih * d.iw * d.ic;
    const size_t dst_img = (size_t)d.oh * d.ow * (d.oc1x1 ? d.oc1x1 : d.oc) * dtype_size(dst_->data_type());
    reads(src_, src_img);
    writes(dst_, dst_img);
    borrows(wei_); borrows(bia_); borrows(wei1_); borrows(bia1_);
    build(d.bs, [&](int n) -> void * {
      dfx_conv_desc ds = d;
      ds.bs = n;
      return create_or_exit(dfx_conv_create, ds, "Init Conv op failed! (%s)");
    });
  }

protected:
  void pack(void *h) override {
    check_dfx(dfx_conv_set_weights(static_cast<dfx_conv_t *>(h), (const int8_t *)wei_->host_data(), bia_ ? bia_->host_data() : nullptr,
                                   scales0_.data(), wei1_ ? (const int8_t *)wei1_->host_data() : nullptr,
                                   bia1_ ? bia1_->host_data() : nullptr, scales1_.data()),
              "conv set_weights");
  }
  void launch(void *h, void *const *p, dfx_stream_t s) override {
    check_dfx(dfx_conv_submit(static_cast<dfx_conv_t *>(h), p[0], p[1], s), "conv submit");
  }
  const char *name() override { return "conv"; }

private:
  memory *src_, *wei_, *bia_, *wei1_, *bia1_, *dst_;
  std::vector<float> scales0_, scales1_;  // owned copies (the reference keeps a dangling pointer)
};

// ---- concat: replaces op_concat<T> ----
class op_concat : public op_base {
public:
  op_concat(const std::vector<std::unique_ptr<memory>> &srcs, std::unique_ptr<memory> &dst, bool relu)
      : op_base(destroy_as<dfx_concat_t, dfx_concat_destroy>), dst_(dst.get()) {
    if (!dst_ || srcs.empty()) error_and_exit("Init Concat op failed!");
    if (dst_->dim_format() != memory::format::nhwc) error_and_exit("Init Concat op failed! (format)");
    auto dm = dst_->actual_dims();  // {n,h,w,c}
    std::vector<int32_t> ch;
    int total = 0;
    for (auto &m : srcs) {
      // jit_concat_kernel::init_conf (jit_concat_kernel.cc:178-191)
      if (!m || m->dim_format() != dst_->dim_format() || m->data_type() != dst_->data_type())
        error_and_exit("Init Concat op failed! (format / data type)");
      auto sd = m->actual_dims();
      if (sd[0] != dm[0] || sd[1] != dm[1] || sd[2] != dm[2]) error_and_exit("Init Concat op failed! (shape)");
      srcs_.push_back(m.get());
      ch.push_back(sd[3]);
      total += sd[3];
    }
    if (total != dm[3]) error_and_exit("Init Concat op failed! (channels)");
    dfx_concat_desc d;
    d.n_inputs = (int)ch.size();
    d.bs = dm[0]; d.h = dm[1]; d.w = dm[2];
    d.dt = to_dfx_dtype(dst_->data_type());
    d.post_relu = relu;
    d.channels = ch.data();
    const size_t esz = dtype_size(dst_->data_type()), px = (size_t)dm[1] * dm[2];
    for (size_t k = 0; k < srcs_.size(); ++k) reads(srcs_[k], px * ch[k] * esz);
    writes(dst_, px * total * esz);
    build(d.bs, [&](int n) -> void * {
      dfx_concat_desc ds = d;
      ds.bs = n;
      return create_or_exit(dfx_concat_create, ds, "Init Concat op failed! (%s)");
    });
  }

protected:
  void launch(void *h, void *const *p, dfx_stream_t s) override {
    check_dfx(dfx_concat_submit(static_cast<dfx_concat_t *>(h), p, p[n_reads()], s), "concat submit");
  }
  const char *name() override { return "concat"; }

private:
  std::vector<memory *> srcs_;
  memory *dst_;
};

// ---- conv + relu + max pooling (reference roadmap, README.md:64): the conv runs as the unfused conv
// op into a device buffer the op owns (the intermediate never visits the host), the pooling kernel
// reads it (from L2 / the Infinity Cache for the sizes of test_conv_relu_pooling.cc) ----
class op_conv_pool : public op_base {
public:
  op_conv_pool(const std::unique_ptr<memory> &src, const std::unique_ptr<memory> &wei,
               const std::unique_ptr<memory> &bia, std::array<int, 2> stride, std::array<int, 2> pad,
               std::array<int, 2> pk, std::array<int, 2> ps, std::array<int, 2> pp, std::unique_ptr<memory> &dst,
               bool relu, const std::vector<float> &scales, round_mode rm, pool_algo algo)
      : op_base(destroy_parts), src_(src.get()), wei_(wei.get()), bia_(bia.get()), dst_(dst.get()), scales_(scales) {
    using fmt = memory::format;
    if (!src_ || !wei_ || !dst_) error_and_exit("Init ConvReluPool op failed! (null tensor)");
    bool ok = src_->data_type() == memory::dtype::u8 && wei_->data_type() == memory::dtype::s8 &&
              src_->dim_format() == fmt::nhwc && dst_->dim_format() == fmt::nhwc &&
              (wei_->dim_format() == fmt::OIhw4i16o4i || wei_->dim_format() == fmt::gOIhw4i16o4i) &&
              (!bia_ || bia_->dim_format() == fmt::x);
    if (!ok) error_and_exit("Init ConvReluPool op failed! (data type / format)");
    auto s = src_->std_dims(), w = wei_->std_dims(), o = dst_->std_dims();
    if (s[0] != o[0]) error_and_exit("Init ConvReluPool op failed! (Batch size do not equal)");
    if (s[1] != w[1]) error_and_exit("Init ConvReluPool op failed! (Input channel do not match)");
    if (o[1] != w[0]) error_and_exit("Init ConvReluPool op failed! (Output channel do not match)");
    if (bia_ && (int)bia_->size() != w[0]) error_and_exit("Init ConvReluPool op failed! (Bias channel do not match)");
    // conv output size: util/math_func.cc:22-24
    const int ch = (s[2] + 2 * pad[0] - w[2]) / stride[0] + 1, cw = (s[3] + 2 * pad[1] - w[3]) / stride[1] + 1;
    if (ch <= 0 || cw <= 0) error_and_exit("Init ConvReluPool op failed! (conv output size)");
    dfx_conv_desc d;
    memset(&d, 0, sizeof(d));
    d.bs = s[0]; d.ic = s[1]; d.ih = s[2]; d.iw = s[3];
    d.oc = w[0]; d.kh = w[2]; d.kw = w[3]; d.oh = ch; d.ow = cw;
    d.sh = stride[0]; d.sw = stride[1]; d.pad_t = pad[0]; d.pad_l = pad[1];
    d.dst_dt = to_dfx_dtype(dst_->data_type());
    d.bia0_dt = bia_ ? to_dfx_dtype(bia_->data_type()) : DFX_UNDEF;
    d.bia1_dt = DFX_UNDEF;
    d.conv0_relu = relu;
    d.conv0_round_mode = to_dfx_round(rm);
    d.conv1_round_mode = DFX_ROUND_NEAREST;
    d.conv0_nscales = (int)scales_.size();
    d.conv1_nscales = 1;
    d.force_variant = -1;
    reads(src_);
    writes(dst_);
    borrows(wei_); borrows(bia_);
    fetch_on_async_ = true;  // (this op is not sharded, its neighbours may be: see op_base)
    build(0, [&](int) -> void * {
      parts *h = new parts();
      // 2x2 stride-2 pooling without padding over an even-sized conv output: fused into the conv kernel's
      // store stage where that kernel covers the conv (dfx.h, dfx_conv_desc::fuse_pool); one launch, the
      // unpooled activation never exists
      if (algo == pool_algo::max && pk[0] == 2 && pk[1] == 2 && ps[0] == 2 && ps[1] == 2 && pp[0] == 0 && pp[1] == 0 && ch % 2 == 0 && cw % 2 == 0 &&
          o[2] == ch / 2 && o[3] == cw / 2) {
        dfx_conv_desc df = d;
        df.fuse_pool = 2;
        if (dfx_conv_create(&df, &h->conv) == DFX_OK) return h;
        h->conv = nullptr;
      }
      if (dfx_conv_create(&d, &h->conv) != DFX_OK) error_and_exit("Init ConvReluPool op failed! (%s)", dfx_last_error());
      dfx_pool_desc p;
      memset(&p, 0, sizeof(p));
      p.bs = s[0]; p.c = w[0]; p.ih = ch; p.iw = cw; p.oh = o[2]; p.ow = o[3];
      p.kh = pk[0]; p.kw = pk[1]; p.sh = ps[0]; p.sw = ps[1]; p.pad_t = pp[0]; p.pad_l = pp[1];
      p.dt = d.dst_dt;
      p.algo = algo == pool_algo::max ? DFX_POOL_MAX
             : algo == pool_algo::avg_include_padding ? DFX_POOL_AVG_INCLUDE_PADDING : DFX_POOL_AVG_EXCLUDE_PADDING;
      if (dfx_pool_create(&p, &h->pool) != DFX_OK) error_and_exit("Init ConvReluPool op failed! (%s)", dfx_last_error());
      check_dfx(dfx_mem_alloc_device(&h->mid, (size_t)s[0] * ch * cw * w[0] * dtype_size(dst_->data_type())), "device alloc");
      return h;
    });
  }

protected:
  void pack(void *h) override {
    check_dfx(dfx_conv_set_weights(static_cast<parts *>(h)->conv, (const int8_t *)wei_->host_data(), bia_ ? bia_->host_data() : nullptr,
                                   scales_.data(), nullptr, nullptr, nullptr),
              "conv set_weights");
  }
  void launch(void *hv, void *const *p, dfx_stream_t s) override {  // (both launches inside the one profile bracket)
    parts *h = static_cast<parts *>(hv);
    if (!h->pool) {  // pooling fused into the conv kernel
      check_dfx(dfx_conv_submit(h->conv, p[0], p[1], s), "conv submit");
    } else {
      check_dfx(dfx_conv_submit(h->conv, p[0], h->mid, s), "conv submit");
      check_dfx(dfx_pool_submit(h->pool, h->mid, p[1], s), "pool submit");
    }
  }
  const char *name() override { return "conv_relu_pool"; }

private:
  // OPTION: this class's handle is two handles and a buffer of its own -- the conv, and where the pooling is not fused
  // into it the pooling op and the unpooled activation between them
  struct parts {
    dfx_conv_t *conv = nullptr;
    dfx_pool_t *pool = nullptr;
    void *mid = nullptr;
  };
  static int destroy_parts(void *hv) {
    parts *h = static_cast<parts *>(hv);
    if (!h) return DFX_OK;
    dfx_conv_destroy(h->conv);
    if (h->pool) dfx_pool_destroy(h->pool);
    if (h->mid) dfx_mem_free_device(h->mid);
    delete h;
    return DFX_OK;
  }
  memory *src_, *wei_, *bia_, *dst_;
  std::vector<float> scales_;
};

// ---- eltwise sum (+relu) (reference roadmap, README.md:65) ----
class op_eltwise : public op_base {
public:
  op_eltwise(const std::vector<std::unique_ptr<memory>> &srcs, std::unique_ptr<memory> &dst, bool relu)
      : op_base(destroy_as<dfx_eltwise_t, dfx_eltwise_destroy>), dst_(dst.get()) {
    if (!dst_ || srcs.size() < 2) error_and_exit("Init EltwiseSum op failed!");
    for (auto &m : srcs) {
      if (!m || m->dim_format() != dst_->dim_format() || m->data_type() != dst_->data_type() ||
          m->actual_dims() != dst_->actual_dims())
        error_and_exit("Init EltwiseSum op failed! (format / data type / shape)");
      srcs_.push_back(m.get());
    }
    dfx_eltwise_desc d;
    d.n_inputs = (int)srcs_.size();
    d.elems = (long long)dst_->size();
    d.dt = to_dfx_dtype(dst_->data_type());
    d.post_relu = relu;
    for (memory *m : srcs_) reads(m);
    writes(dst_);
    fetch_on_async_ = true;  // (not sharded: see op_conv_pool)
    build(0, [&](int) -> void * { return create_or_exit(dfx_eltwise_create, d, "Init EltwiseSum op failed! (%s)"); });
  }

protected:
  void launch(void *h, void *const *p, dfx_stream_t s) override {
    check_dfx(dfx_eltwise_submit(static_cast<dfx_eltwise_t *>(h), p, p[n_reads()], s), "eltwise submit");
  }
  const char *name() override { return "eltwise_sum"; }

private:
  std::vector<memory *> srcs_;
  memory *dst_;
};

// ---- activation reorder (dfx_reorder_*): layout / dtype / scale conversion, channel pad and crop ----
class op_reorder : public op_base {
public:
  op_reorder(const std::unique_ptr<memory> &src, const std::unique_ptr<memory> &dst, const std::vector<float> &scales,
             round_mode rm)
      : op_base(destroy_as<dfx_reorder_t, dfx_reorder_destroy>), src_(src.get()), dst_(dst.get()), scales_(scales) {
    using fmt = memory::format;
    if (!src_ || !dst_) error_and_exit("Init Reorder op failed! (null tensor)");
    for (memory *m : {src_, dst_})
      if (m->dim_format() != fmt::nchw && m->dim_format() != fmt::nhwc) error_and_exit("Init Reorder op failed! (format)");
    auto s = src_->std_dims(), o = dst_->std_dims();
    if (s[0] != o[0]) error_and_exit("Init Reorder op failed! (Batch size do not equal)");
    if (s[2] != o[2] || s[3] != o[3]) error_and_exit("Init Reorder op failed! (shape)");
    dfx_reorder_desc d;
    memset(&d, 0, sizeof(d));
    d.bs = s[0]; d.h = s[2]; d.w = s[3]; d.src_c = s[1]; d.dst_c = o[1];
    d.src_fmt = src_->dim_format() == fmt::nhwc ? DFX_FMT_NHWC : DFX_FMT_NCHW;
    d.dst_fmt = dst_->dim_format() == fmt::nhwc ? DFX_FMT_NHWC : DFX_FMT_NCHW;
    d.src_dt = to_dfx_dtype(src_->data_type());
    d.dst_dt = to_dfx_dtype(dst_->data_type());
    d.round_mode = to_dfx_round(rm);
    d.n_scales = (int)scales_.size();
    // both layouts are batch-major: a batch shard is a contiguous byte range of src and of dst
    const size_t src_img = (size_t)d.h * d.w * d.src_c * dtype_size(src_->data_type());
    const size_t dst_img = (size_t)d.h * d.w * d.dst_c * dtype_size(dst_->data_type());
    reads(src_, src_img);
    writes(dst_, dst_img);
    build(d.bs, [&](int n) -> void * {
      dfx_reorder_desc ds = d;
      ds.bs = n;
      dfx_reorder_t *h = nullptr;
      if (dfx_reorder_create(&ds, scales_.data(), &h) != DFX_OK) error_and_exit("Init Reorder op failed! (%s)", dfx_last_error());
      return h;
    });
  }

protected:
  void launch(void *h, void *const *p, dfx_stream_t s) override {
    check_dfx(dfx_reorder_submit(static_cast<dfx_reorder_t *>(h), p[0], p[1], s), "reorder submit");
  }
  const char *name() override { return "reorder"; }

private:
  memory *src_, *dst_;
  std::vector<float> scales_;
};

// ---- concat + pointwise conv in one launch (dfx_catconv_*): the branches are read in place, the concatenated
// tensor is never written.  Checks are op_concat's for the branches and op_conv's for weights, bias and dst. ----
class op_concat_conv : public op_base {
public:
  op_concat_conv(const std::vector<std::unique_ptr<memory>> &srcs, const std::unique_ptr<memory> &wei,
                 const std::unique_ptr<memory> &bia, std::unique_ptr<memory> &dst, bool relu,
                 const std::vector<float> &scales, round_mode rm)
      : op_base(destroy_as<dfx_catconv_t, dfx_catconv_destroy>), wei_(wei.get()), bia_(bia.get()), dst_(dst.get()), scales_(scales) {
    using fmt = memory::format;
    if (!wei_ || !dst_ || srcs.empty()) error_and_exit("Init ConcatConv op failed! (null tensor)");
    if (wei_->data_type() != memory::dtype::s8 || dst_->dim_format() != fmt::nhwc ||
        (wei_->dim_format() != fmt::OIhw4i16o4i && wei_->dim_format() != fmt::gOIhw4i16o4i) ||
        (bia_ && bia_->dim_format() != fmt::x))
      error_and_exit("Init ConcatConv op failed! (data type / format)");
    auto w = wei_->std_dims(), o = dst_->std_dims();
    std::vector<int32_t> ch;
    int total = 0;
    for (auto &m : srcs) {
      if (!m || m->dim_format() != fmt::nhwc || m->data_type() != memory::dtype::u8)
        error_and_exit("Init ConcatConv op failed! (branches must be nhwc u8)");
      auto sd = m->std_dims();
      if (sd[0] != o[0]) error_and_exit("Init ConcatConv op failed! (Batch size do not equal)");
      if (sd[2] != o[2] || sd[3] != o[3]) error_and_exit("Init ConcatConv op failed! (shape)");
      srcs_.push_back(m.get());
      ch.push_back(sd[1]);
      total += sd[1];
    }
    if (total != w[1]) error_and_exit("Init ConcatConv op failed! (Input channel do not match)");
    if (w[2] != 1 || w[3] != 1) error_and_exit("Init ConcatConv op failed! (conv must be 1x1 kernel)");
    if (o[1] != w[0]) error_and_exit("Init ConcatConv op failed! (Output channel do not match)");
    if (bia_ && (int)bia_->size() != w[0]) error_and_exit("Init ConcatConv op failed! (Bias channel do not match)");
    dfx_catconv_desc d;
    memset(&d, 0, sizeof(d));
    d.n_inputs = (int)ch.size();
    d.bs = o[0]; d.h = o[2]; d.w = o[3]; d.oc = w[0];
    d.dst_dt = to_dfx_dtype(dst_->data_type());
    d.bia_dt = bia_ ? to_dfx_dtype(bia_->data_type()) : DFX_UNDEF;
    d.relu = relu;
    d.round_mode = to_dfx_round(rm);
    d.nscales = (int)scales_.size();
    d.force_path = -1;
    d.channels = ch.data();
    const size_t px = (size_t)d.h * d.w;
    for (size_t k = 0; k < srcs_.size(); ++k) reads(srcs_[k], px * ch[k]);  // (a shard is an offset into every branch)
    writes(dst_, px * d.oc * dtype_size(dst_->data_type()));
    borrows(wei_); borrows(bia_);
    build(d.bs, [&](int n) -> void * {
      dfx_catconv_desc ds = d;
      ds.bs = n;
      return create_or_exit(dfx_catconv_create, ds, "Init ConcatConv op failed! (%s)");
    });
  }

protected:
  void pack(void *h) override {
    check_dfx(dfx_catconv_set_weights(static_cast<dfx_catconv_t *>(h), (const int8_t *)wei_->host_data(), bia_ ? bia_->host_data() : nullptr,
                                      scales_.data()),
              "concat_conv set_weights");
  }
  void launch(void *h, void *const *p, dfx_stream_t s) override {
    check_dfx(dfx_catconv_submit(static_cast<dfx_catconv_t *>(h), p, p[n_reads()], s), "concat_conv submit");
  }
  const char *name() override { return "concat_conv"; }

private:
  std::vector<memory *> srcs_;
  memory *wei_, *bia_, *dst_;
  std::vector<float> scales_;
};

// ---- depthwise conv (dfx_dwconv_*): every channel has its own kh x kw window.  Checks are op_conv's; the weights are
// a plain oihw {c, 1, kh, kw} tensor, and dst's dims give the output size (windows may hang over the bottom / right
// edge). ----
class op_depthwise_conv : public op_base {
public:
  op_depthwise_conv(const std::unique_ptr<memory> &src, const std::unique_ptr<memory> &wei, const std::unique_ptr<memory> &bia,
                    std::array<int, 2> stride, std::array<int, 2> padding, std::unique_ptr<memory> &dst, bool relu,
                    const std::vector<float> &scales, round_mode rm)
      : op_base(destroy_as<dfx_dwconv_t, dfx_dwconv_destroy>), src_(src.get()), wei_(wei.get()), bia_(bia.get()), dst_(dst.get()), scales_(scales) {
    using fmt = memory::format;
    if (!src_ || !wei_ || !dst_) error_and_exit("Init DepthwiseConv op failed! (null tensor)");
    if (src_->data_type() != memory::dtype::u8 || wei_->data_type() != memory::dtype::s8 || src_->dim_format() != fmt::nhwc ||
        dst_->dim_format() != fmt::nhwc || wei_->dim_format() != fmt::oihw || (bia_ && bia_->dim_format() != fmt::x))
      error_and_exit("Init DepthwiseConv op failed! (data type / format)");
    auto i = src_->std_dims(), w = wei_->std_dims(), o = dst_->std_dims();
    if (i[0] != o[0]) error_and_exit("Init DepthwiseConv op failed! (Batch size do not equal)");
    if (w[0] != i[1] || w[1] != 1) error_and_exit("Init DepthwiseConv op failed! (weights must be {c, 1, kh, kw})");
    if (o[1] != i[1]) error_and_exit("Init DepthwiseConv op failed! (Output channel do not match)");
    if (bia_ && (int)bia_->size() != i[1]) error_and_exit("Init DepthwiseConv op failed! (Bias channel do not match)");
    dfx_dwconv_desc d;
    memset(&d, 0, sizeof(d));
    d.bs = i[0]; d.c = i[1]; d.ih = i[2]; d.iw = i[3]; d.oh = o[2]; d.ow = o[3];
    d.kh = w[2]; d.kw = w[3]; d.sh = stride[0]; d.sw = stride[1]; d.pad_t = padding[0]; d.pad_l = padding[1];
    d.dst_dt = to_dfx_dtype(dst_->data_type());
    d.bia_dt = bia_ ? to_dfx_dtype(bia_->data_type()) : DFX_UNDEF;
    d.relu = relu;
    d.round_mode = to_dfx_round(rm);
    d.nscales = (int)scales_.size();
    d.force_path = -1;
    const size_t src_img = (size_t)d.ih * d.iw * d.c;
    const size_t dst_img = (size_t)d.oh * d.ow * d.c * dtype_size(dst_->data_type());
    reads(src_, src_img);
    writes(dst_, dst_img);
    borrows(wei_); borrows(bia_);
    build(d.bs, [&](int n) -> void * {
      dfx_dwconv_desc ds = d;
      ds.bs = n;
      return create_or_exit(dfx_dwconv_create, ds, "Init DepthwiseConv op failed! (%s)");
    });
  }

protected:
  void pack(void *h) override {
    const void *bia = bia_ ? bia_->host_data() : nullptr;
    check_dfx(dfx_dwconv_set_weights(static_cast<dfx_dwconv_t *>(h), (const int8_t *)wei_->host_data(), bia, scales_.data()), "depthwise_conv set_weights");
  }
  void launch(void *h, void *const *p, dfx_stream_t s) override {
    check_dfx(dfx_dwconv_submit(static_cast<dfx_dwconv_t *>(h), p[0], p[1], s), "depthwise_conv submit");
  }
  const char *name() override { return "depthwise_conv"; }

private:
  memory *src_, *wei_, *bia_, *dst_;
  std::vector<float> scales_;
};

// ---- grouped conv (dfx_gconv_*): output channel o reads the ic / groups input channels of its group.  Checks are
// op_depthwise_conv's; the weights are a plain oihw {oc, ic / groups, kh, kw} tensor, and dst's dims give the output size
// (windows may hang over the bottom / right edge).  Weight hashing and batch sharding are op_base's. ----
class op_grouped_conv : public op_base {
public:
  op_grouped_conv(const std::unique_ptr<memory> &src, const std::unique_ptr<memory> &wei, const std::unique_ptr<memory> &bia,
                  int groups, std::array<int, 2> stride, std::array<int, 2> padding, std::unique_ptr<memory> &dst, bool relu,
                    const std::vector<float> &scales, round_mode rm)
      : op_base(destroy_as<dfx_gconv_t, dfx_gconv_destroy>), src_(src.get()), wei_(wei.get()), bia_(bia.get()), dst_(dst.get()), scales_(scales) {
    using fmt = memory::format;
    if (!src_ || !wei_ || !dst_) error_and_exit("Init GroupedConv op failed! (null tensor)");
    if (src_->data_type() != memory::dtype::u8 || wei_->data_type() != memory::dtype::s8 || src_->dim_format() != fmt::nhwc ||
        dst_->dim_format() != fmt::nhwc || wei_->dim_format() != fmt::oihw || (bia_ && bia_->dim_format() != fmt::x))
      error_and_exit("Init GroupedConv op failed! (data type / format)");
    auto i = src_->std_dims(), w = wei_->std_dims(), o = dst_->std_dims();
    if (i[0] != o[0]) error_and_exit("Init GroupedConv op failed! (Batch size do not equal)");
    if (groups < 1 || i[1] % groups || o[1] % groups) error_and_exit("Init GroupedConv op failed! (groups must divide both channel counts)");
    if (w[0] != o[1] || w[1] != i[1] / groups) error_and_exit("Init GroupedConv op failed! (weights must be {oc, ic / groups, kh, kw})");
    if (bia_ && (int)bia_->size() != o[1]) error_and_exit("Init GroupedConv op failed! (Bias channel do not match)");
    dfx_gconv_desc d;
    memset(&d, 0, sizeof(d));
    d.bs = i[0]; d.ic = i[1]; d.ih = i[2]; d.iw = i[3]; d.oc = o[1]; d.oh = o[2]; d.ow = o[3]; d.groups = groups;
    d.kh = w[2]; d.kw = w[3]; d.sh = stride[0]; d.sw = stride[1]; d.pad_t = padding[0]; d.pad_l = padding[1];
    d.dst_dt = to_dfx_dtype(dst_->data_type());
    d.bia_dt = bia_ ? to_dfx_dtype(bia_->data_type()) : DFX_UNDEF;
    d.relu = relu;
    d.round_mode = to_dfx_round(rm);
    d.nscales = (int)scales_.size();
    d.force_path = -1;
    const size_t src_img = (size_t)d.ih * d.iw * d.ic;
    const size_t dst_img = (size_t)d.oh * d.ow * d.oc * dtype_size(dst_->data_type());
    reads(src_, src_img);
    writes(dst_, dst_img);
    borrows(wei_); borrows(bia_);
    build(d.bs, [&](int n) -> void * {
      dfx_gconv_desc ds = d;
      ds.bs = n;
      return create_or_exit(dfx_gconv_create, ds, "Init GroupedConv op failed! (%s)");
    });
  }

protected:
  void pack(void *h) override {
    const void *bia = bia_ ? bia_->host_data() : nullptr;
    check_dfx(dfx_gconv_set_weights(static_cast<dfx_gconv_t *>(h), (const int8_t *)wei_->host_data(), bia, scales_.data()), "grouped_conv set_weights");
  }
  void launch(void *h, void *const *p, dfx_stream_t s) override {
    check_dfx(dfx_gconv_submit(static_cast<dfx_gconv_t *>(h), p[0], p[1], s), "grouped_conv submit");
  }
  const char *name() override { return "grouped_conv"; }

private:
  memory *src_, *wei_, *bia_, *dst_;
  std::vector<float> scales_;
};

// ---- first-layer conv over a 1- to 4-channel image (dfx_imgconv_*).  Checks are op_grouped_conv's; the weights are a
// plain oihw {oc, ic, kh, kw} tensor, and dst's dims give the output size (windows may hang over the bottom / right
// edge).  Weight hashing and batch sharding are op_base's. ----
class op_image_conv : public op_base {
public:
  op_image_conv(const std::unique_ptr<memory> &src, const std::unique_ptr<memory> &wei, const std::unique_ptr<memory> &bia,
                std::array<int, 2> stride, std::array<int, 2> padding, std::unique_ptr<memory> &dst, bool relu,
                const std::vector<float> &scales, round_mode rm)
      : op_base(destroy_as<dfx_imgconv_t, dfx_imgconv_destroy>), src_(src.get()), wei_(wei.get()), bia_(bia.get()), dst_(dst.get()), scales_(scales) {
    using fmt = memory::format;
    if (!src_ || !wei_ || !dst_) error_and_exit("Init ImageConv op failed! (null tensor)");
    if (src_->data_type() != memory::dtype::u8 || wei_->data_type() != memory::dtype::s8 || src_->dim_format() != fmt::nhwc ||
        dst_->dim_format() != fmt::nhwc || wei_->dim_format() != fmt::oihw || (bia_ && bia_->dim_format() != fmt::x))
      error_and_exit("Init ImageConv op failed! (data type / format)");
    auto i = src_->std_dims(), w = wei_->std_dims(), o = dst_->std_dims();
    if (i[0] != o[0]) error_and_exit("Init ImageConv op failed! (Batch size do not equal)");
    if (i[1] > 4) error_and_exit("Init ImageConv op failed! (an image has 1 to 4 channels)");
    if (w[0] != o[1] || w[1] != i[1]) error_and_exit("Init ImageConv op failed! (weights must be {oc, ic, kh, kw})");
    if (bia_ && (int)bia_->size() != o[1]) error_and_exit("Init ImageConv op failed! (Bias channel do not match)");
    dfx_imgconv_desc d;
    memset(&d, 0, sizeof(d));
    d.bs = i[0]; d.ic = i[1]; d.ih = i[2]; d.iw = i[3]; d.oc = o[1]; d.oh = o[2]; d.ow = o[3];
    d.kh = w[2]; d.kw = w[3]; d.sh = stride[0]; d.sw = stride[1]; d.pad_t = padding[0]; d.pad_l = padding[1];
    d.dst_dt = to_dfx_dtype(dst_->data_type());
    d.bia_dt = bia_ ? to_dfx_dtype(bia_->data_type()) : DFX_UNDEF;
    d.relu = relu;
    d.round_mode = to_dfx_round(rm);
    d.nscales = (int)scales_.size();
    d.force_path = -1;
    const size_t src_img = (size_t)d.ih * d.iw * d.ic;
    const size_t dst_img = (size_t)d.oh * d.ow * d.oc * dtype_size(dst_->data_type());
    reads(src_, src_img);
    writes(dst_, dst_img);
    borrows(wei_); borrows(bia_);
    build(d.bs, [&](int n) -> void * {
      dfx_imgconv_desc ds = d;
      ds.bs = n;
      return create_or_exit(dfx_imgconv_create, ds, "Init ImageConv op failed! (%s)");
    });
  }

protected:
  void pack(void *h) override {
    const void *bia = bia_ ? bia_->host_data() : nullptr;
    check_dfx(dfx_imgconv_set_weights(static_cast<dfx_imgconv_t *>(h), (const int8_t *)wei_->host_data(), bia, scales_.data()), "image_conv set_weights");
  }
  void launch(void *h, void *const *p, dfx_stream_t s) override {
    check_dfx(dfx_imgconv_submit(static_cast<dfx_imgconv_t *>(h), p[0], p[1], s), "image_conv submit");
  }
  const char *name() override { return "image_conv"; }

private:
  memory *src_, *wei_, *bia_, *dst_;
  std::vector<float> scales_;
};

// ---- transposed conv (dfx_deconv_*).  Checks are op_grouped_conv's; the weights are a plain oihw {oc, ic, kh, kw} tensor
// (oneDNN's logical order for deconvolution), and dst's dims give the output size (output_padding, cropping).  Weight
// hashing and batch sharding are op_base's. ----
class op_deconvolution : public op_base {
public:
  op_deconvolution(const std::unique_ptr<memory> &src, const std::unique_ptr<memory> &wei, const std::unique_ptr<memory> &bia,
                std::array<int, 2> stride, std::array<int, 2> padding, std::unique_ptr<memory> &dst, bool relu,
                const std::vector<float> &scales, round_mode rm)
      : op_base(destroy_as<dfx_deconv_t, dfx_deconv_destroy>), src_(src.get()), wei_(wei.get()), bia_(bia.get()), dst_(dst.get()), scales_(scales) {
    using fmt = memory::format;
    if (!src_ || !wei_ || !dst_) error_and_exit("Init Deconvolution op failed! (null tensor)");
    if (src_->data_type() != memory::dtype::u8 || wei_->data_type() != memory::dtype::s8 || src_->dim_format() != fmt::nhwc ||
        dst_->dim_format() != fmt::nhwc || wei_->dim_format() != fmt::oihw || (bia_ && bia_->dim_format() != fmt::x))
      error_and_exit("Init Deconvolution op failed! (data type / format)");
    auto i = src_->std_dims(), w = wei_->std_dims(), o = dst_->std_dims();
    if (i[0] != o[0]) error_and_exit("Init Deconvolution op failed! (Batch size do not equal)");
    if (w[0] != o[1] || w[1] != i[1]) error_and_exit("Init Deconvolution op failed! (weights must be {oc, ic, kh, kw})");
    if (bia_ && (int)bia_->size() != o[1]) error_and_exit("Init Deconvolution op failed! (Bias channel do not match)");
    dfx_deconv_desc d;
    memset(&d, 0, sizeof(d));
    d.bs = i[0]; d.ic = i[1]; d.ih = i[2]; d.iw = i[3]; d.oc = o[1]; d.oh = o[2]; d.ow = o[3];
    d.kh = w[2]; d.kw = w[3]; d.sh = stride[0]; d.sw = stride[1]; d.pad_t = padding[0]; d.pad_l = padding[1];
    d.dst_dt = to_dfx_dtype(dst_->data_type());
    d.bia_dt = bia_ ? to_dfx_dtype(bia_->data_type()) : DFX_UNDEF;
    d.relu = relu;
    d.round_mode = to_dfx_round(rm);
    d.nscales = (int)scales_.size();
    d.force_path = -1;
    const size_t src_img = (size_t)d.ih * d.iw * d.ic;
    const size_t dst_img = (size_t)d.oh * d.ow * d.oc * dtype_size(dst_->data_type());
    reads(src_, src_img);
    writes(dst_, dst_img);
    borrows(wei_); borrows(bia_);
    build(d.bs, [&](int n) -> void * {
      dfx_deconv_desc ds = d;
      ds.bs = n;
      return create_or_exit(dfx_deconv_create, ds, "Init Deconvolution op failed! (%s)");
    });
  }

protected:
  void pack(void *h) override {
    const void *bia = bia_ ? bia_->host_data() : nullptr;
    check_dfx(dfx_deconv_set_weights(static_cast<dfx_deconv_t *>(h), (const int8_t *)wei_->host_data(), bia, scales_.data()), "deconvolution set_weights");
  }
  void launch(void *h, void *const *p, dfx_stream_t s) override {
    check_dfx(dfx_deconv_submit(static_cast<dfx_deconv_t *>(h), p[0], p[1], s), "deconvolution submit");
  }
  const char *name() override { return "deconvolution"; }

private:
  memory *src_, *wei_, *bia_, *dst_;
  std::vector<float> scales_;
};

// ---- dilated conv (dfx_dilconv_*).  Checks are op_grouped_conv's; the weights are a plain oihw {oc, ic, kh, kw} tensor and
// dst's dims give the output size.  Weight hashing and batch sharding are op_base's. ----
class op_dilated_conv : public op_base {
public:
  op_dilated_conv(const std::unique_ptr<memory> &src, const std::unique_ptr<memory> &wei, const std::unique_ptr<memory> &bia,
                std::array<int, 2> stride, std::array<int, 2> dilation, std::array<int, 2> padding, std::unique_ptr<memory> &dst, bool relu,
                const std::vector<float> &scales, round_mode rm)
      : op_base(destroy_as<dfx_dilconv_t, dfx_dilconv_destroy>), src_(src.get()), wei_(wei.get()), bia_(bia.get()), dst_(dst.get()), scales_(scales) {
    using fmt = memory::format;
    if (!src_ || !wei_ || !dst_) error_and_exit("Init DilatedConv op failed! (null tensor)");
    if (src_->data_type() != memory::dtype::u8 || wei_->data_type() != memory::dtype::s8 || src_->dim_format() != fmt::nhwc ||
        dst_->dim_format() != fmt::nhwc || wei_->dim_format() != fmt::oihw || (bia_ && bia_->dim_format() != fmt::x))
      error_and_exit("Init DilatedConv op failed! (data type / format)");
    auto i = src_->std_dims(), w = wei_->std_dims(), o = dst_->std_dims();
    if (i[0] != o[0]) error_and_exit("Init DilatedConv op failed! (Batch size do not equal)");
    if (w[0] != o[1] || w[1] != i[1]) error_and_exit("Init DilatedConv op failed! (weights must be {oc, ic, kh, kw})");
    if (bia_ && (int)bia_->size() != o[1]) error_and_exit("Init DilatedConv op failed! (Bias channel do not match)");
    dfx_dilconv_desc d;
    memset(&d, 0, sizeof(d));
    d.bs = i[0]; d.ic = i[1]; d.ih = i[2]; d.iw = i[3]; d.oc = o[1]; d.oh = o[2]; d.ow = o[3];
    d.kh = w[2]; d.kw = w[3]; d.sh = stride[0]; d.sw = stride[1]; d.dh = dilation[0]; d.dw = dilation[1]; d.pad_t = padding[0]; d.pad_l = padding[1];
    d.dst_dt = to_dfx_dtype(dst_->data_type());
    d.bia_dt = bia_ ? to_dfx_dtype(bia_->data_type()) : DFX_UNDEF;
    d.relu = relu;
    d.round_mode = to_dfx_round(rm);
    d.nscales = (int)scales_.size();
    d.force_path = -1;
    const size_t src_img = (size_t)d.ih * d.iw * d.ic;
    const size_t dst_img = (size_t)d.oh * d.ow * d.oc * dtype_size(dst_->data_type());
    reads(src_, src_img);
    writes(dst_, dst_img);
    borrows(wei_); borrows(bia_);
    build(d.bs, [&](int n) -> void * {
      dfx_dilconv_desc ds = d;
      ds.bs = n;
      return create_or_exit(dfx_dilconv_create, ds, "Init DilatedConv op failed! (%s)");
    });
  }

protected:
  void pack(void *h) override {
    const void *bia = bia_ ? bia_->host_data() : nullptr;
    check_dfx(dfx_dilconv_set_weights(static_cast<dfx_dilconv_t *>(h), (const int8_t *)wei_->host_data(), bia, scales_.data()), "dilated_conv set_weights");
  }
  void launch(void *h, void *const *p, dfx_stream_t s) override {
    check_dfx(dfx_dilconv_submit(static_cast<dfx_dilconv_t *>(h), p[0], p[1], s), "dilated_conv submit");
  }
  const char *name() override { return "dilated_conv"; }

private:
  memory *src_, *wei_, *bia_, *dst_;
  std::vector<float> scales_;
};

// ---- fully-connected layer (dfx_fc_*): dst[n][o] = requant(sum over c, y, x of src[n][y][x][c] * wei[o][c][y][x]).  Checks
// are op_grouped_conv's; the weights are a plain oihw {oc, c, h, w} tensor over the whole source image (a flattened-CHW
// classifier), dst is {bs, oc, 1, 1}.  Weight hashing and batch sharding are op_base's. ----
class op_inner_product : public op_base {
public:
  op_inner_product(const std::unique_ptr<memory> &src, const std::unique_ptr<memory> &wei, const std::unique_ptr<memory> &bia,
                   std::unique_ptr<memory> &dst, bool relu, const std::vector<float> &scales, round_mode rm)
      : op_base(destroy_as<dfx_fc_t, dfx_fc_destroy>), src_(src.get()), wei_(wei.get()), bia_(bia.get()), dst_(dst.get()), scales_(scales) {
    using fmt = memory::format;
    if (!src_ || !wei_ || !dst_) error_and_exit("Init InnerProduct op failed! (null tensor)");
    if (src_->data_type() != memory::dtype::u8 || wei_->data_type() != memory::dtype::s8 || src_->dim_format() != fmt::nhwc ||
        dst_->dim_format() != fmt::nhwc || wei_->dim_format() != fmt::oihw || (bia_ && bia_->dim_format() != fmt::x))
      error_and_exit("Init InnerProduct op failed! (data type / format)");
    auto i = src_->std_dims(), w = wei_->std_dims(), o = dst_->std_dims();
    if (i[0] != o[0]) error_and_exit("Init InnerProduct op failed! (Batch size do not equal)");
    if (w[0] != o[1] || w[1] != i[1] || w[2] != i[2] || w[3] != i[3]) error_and_exit("Init InnerProduct op failed! (weights must be {oc, c, h, w} of src)");
    if (o[2] != 1 || o[3] != 1) error_and_exit("Init InnerProduct op failed! (dst must be {bs, oc, 1, 1})");
    if (bia_ && (int)bia_->size() != o[1]) error_and_exit("Init InnerProduct op failed! (Bias channel do not match)");
    dfx_fc_desc d;
    memset(&d, 0, sizeof(d));
    d.bs = i[0]; d.ic = i[1]; d.ih = i[2]; d.iw = i[3]; d.oc = o[1];
    d.dst_dt = to_dfx_dtype(dst_->data_type());
    d.bia_dt = bia_ ? to_dfx_dtype(bia_->data_type()) : DFX_UNDEF;
    d.relu = relu;
    d.round_mode = to_dfx_round(rm);
    d.nscales = (int)scales_.size();
    d.force_path = -1;
    const size_t src_img = (size_t)d.ih * d.iw * d.ic;
    const size_t dst_img = (size_t)d.oc * dtype_size(dst_->data_type());
    reads(src_, src_img);
    writes(dst_, dst_img);
    borrows(wei_); borrows(bia_);
    build(d.bs, [&](int n) -> void * {
      dfx_fc_desc ds = d;
      ds.bs = n;
      return create_or_exit(dfx_fc_create, ds, "Init InnerProduct op failed! (%s)");
    });
  }

protected:
  void pack(void *h) override {
    const void *bia = bia_ ? bia_->host_data() : nullptr;
    check_dfx(dfx_fc_set_weights(static_cast<dfx_fc_t *>(h), (const int8_t *)wei_->host_data(), bia, scales_.data()), "inner_product set_weights");
  }
  void launch(void *h, void *const *p, dfx_stream_t s) override {
    check_dfx(dfx_fc_submit(static_cast<dfx_fc_t *>(h), p[0], p[1], s), "inner_product submit");
  }
  const char *name() override { return "inner_product"; }

private:
  memory *src_, *wei_, *bia_, *dst_;
  std::vector<float> scales_;
};

// ---- activation resize (dfx_resize_*), optionally with a lateral tensor added in the same launch.  No weights: nothing to
// hash or pack.  Batch sharding is op_base's; the lateral is sharded like dst, whose dims it has. ----
class op_resize : public op_base {
public:
  op_resize(const std::unique_ptr<memory> &src, const std::unique_ptr<memory> *lateral, std::unique_ptr<memory> &dst, resize_algo algo,
            resize_coord coord, bool post_relu)
      : op_base(destroy_as<dfx_resize_t, dfx_resize_destroy>), src_(src.get()), lat_(lateral ? lateral->get() : nullptr), dst_(dst.get()) {
    using fmt = memory::format;
    if (!src_ || !dst_ || (lateral && !lat_)) error_and_exit("Init Resize op failed! (null tensor)");
    if (src_->dim_format() != fmt::nhwc || dst_->dim_format() != fmt::nhwc || src_->data_type() != dst_->data_type())
      error_and_exit("Init Resize op failed! (data type / format)");
    auto i = src_->std_dims(), o = dst_->std_dims();
    if (i[0] != o[0]) error_and_exit("Init Resize op failed! (Batch size do not equal)");
    if (i[1] != o[1]) error_and_exit("Init Resize op failed! (Channel do not match)");
    if (lat_ && (lat_->dim_format() != fmt::nhwc || lat_->data_type() != dst_->data_type() || lat_->std_dims() != o))
      error_and_exit("Init Resize op failed! (the lateral must have dst's dims, format and data type)");
    if (src_ == dst_) error_and_exit("Init Resize op failed! (dst must not be src)");
    dfx_resize_desc d;
    memset(&d, 0, sizeof(d));
    d.bs = i[0]; d.c = i[1]; d.ih = i[2]; d.iw = i[3]; d.oh = o[2]; d.ow = o[3];
    d.dt = to_dfx_dtype(dst_->data_type());
    d.algo = algo == resize_algo::nearest ? DFX_RESIZE_NEAREST : DFX_RESIZE_BILINEAR;
    d.coord = coord == resize_coord::half_pixel ? DFX_COORD_HALF_PIXEL
              : coord == resize_coord::align_corners ? DFX_COORD_ALIGN_CORNERS : DFX_COORD_ASYMMETRIC;
    d.add = lat_ ? 1 : 0;
    d.post_relu = post_relu ? 1 : 0;
    d.force_path = -1;
    const size_t src_img = (size_t)d.ih * d.iw * d.c * dtype_size(src_->data_type());
    const size_t dst_img = (size_t)d.oh * d.ow * d.c * dtype_size(dst_->data_type());
    reads(src_, src_img);
    reads(lat_, dst_img);  // (absent for resize(); it may be dst)
    writes(dst_, dst_img);
    build(d.bs, [&](int n) -> void * {
      dfx_resize_desc ds = d;
      ds.bs = n;
      return create_or_exit(dfx_resize_create, ds, "Init Resize op failed! (%s)");
    });
  }

protected:
  void launch(void *h, void *const *p, dfx_stream_t s) override {
    check_dfx(dfx_resize_submit(static_cast<dfx_resize_t *>(h), p[0], p[1], p[2], s), "resize submit");
  }
  const char *name() override { return lat_ ? "resize_add" : "resize"; }

private:
  memory *src_, *lat_, *dst_;
};

// ---- scaled element-wise sum (dfx_wsum_*): 1 to 8 nhwc tensors of mixed dtypes, scales, bias, ReLU, table.  The scales,
// the bias and the table are copied at construction: nothing to hash.  dst may be one of the srcs; every src is registered
// as a read and dst as a write (op_state), so an in-place op waits for earlier readers of that tensor on other streams.
// Batch sharding is op_base's: every tensor is batch-major. ----
class op_scaled_sum : public op_base {
public:
  op_scaled_sum(const std::vector<std::unique_ptr<memory>> &srcs, const std::vector<std::vector<float>> &scales, std::unique_ptr<memory> &dst,
                const std::vector<float> &bias, bool post_relu, const std::vector<u8> &table, memory::dtype table_in, round_mode rm)
      : op_base(destroy_as<dfx_wsum_t, dfx_wsum_destroy>), dst_(dst.get()) {
    using fmt = memory::format;
    if (!dst_ || srcs.empty() || srcs.size() > DFX_WSUM_MAX_INPUTS) error_and_exit("Init ScaledSum op failed! (1 to 8 sources and a dst)");
    if (scales.size() != srcs.size()) error_and_exit("Init ScaledSum op failed! (one vector of scales per source)");
    if (dst_->dim_format() != fmt::nhwc) error_and_exit("Init ScaledSum op failed! (format)");
    if ((table_in != memory::dtype::undef) != !table.empty() || (!table.empty() && table.size() != 256))
      error_and_exit("Init ScaledSum op failed! (a table has 256 entries and needs table_in)");
    auto o = dst_->std_dims();
    dfx_wsum_desc d;
    memset(&d, 0, sizeof(d));
    d.bs = o[0]; d.c = o[1]; d.h = o[2]; d.w = o[3];
    d.n_inputs = (int)srcs.size();
    for (size_t i = 0; i < srcs.size(); ++i) {
      memory *m = srcs[i].get();
      if (!m || m->dim_format() != fmt::nhwc || m->std_dims() != o) error_and_exit("Init ScaledSum op failed! (format / shape of a source)");
      srcs_.push_back(m);
      d.src_dt[i] = to_dfx_dtype(m->data_type());
      d.nscales[i] = (int)scales[i].size();
    }
    d.n_bias = (int)bias.size();
    d.dst_dt = to_dfx_dtype(dst_->data_type());
    d.round_mode = to_dfx_round(rm);
    d.post_relu = post_relu ? 1 : 0;
    d.lut_in_dt = to_dfx_dtype(table_in);
    d.force_path = -1;
    const size_t img = (size_t)d.h * d.w * d.c;
    for (memory *m : srcs_) reads(m, img * dtype_size(m->data_type()));  // (a source may be dst)
    writes(dst_, img * dtype_size(dst_->data_type()));
    std::vector<const float *> sp;
    for (const std::vector<float> &s : scales) sp.push_back(s.data());
    const float *bp = bias.empty() ? nullptr : bias.data();
    const u8 *tp = table.empty() ? nullptr : table.data();
    build(d.bs, [&](int n) -> void * {
      dfx_wsum_desc ds = d;
      ds.bs = n;
      dfx_wsum_t *h = static_cast<dfx_wsum_t *>(create_or_exit(dfx_wsum_create, ds, "Init ScaledSum op failed! (%s)"));
      check_dfx(dfx_wsum_set_params(h, sp.data(), bp, tp), "wsum set_params");
      return h;
    });
  }

protected:
  void launch(void *h, void *const *p, dfx_stream_t s) override {
    check_dfx(dfx_wsum_submit(static_cast<dfx_wsum_t *>(h), p, p[n_reads()], s), "wsum submit");
  }
  const char *name() override { return "scaled_sum"; }

private:
  std::vector<memory *> srcs_;
  memory *dst_;
};

// ---- net head (dfx_head_*): channel top-k / argmax and table softmax over the rows of an nhwc tensor (rows = bs * h * w,
// src_ld = C, c_valid <= C).  TOPK writes idx {bs, k, h, w} and, if given, val of src's dtype; SOFTMAX writes dst
// {bs, C', h, w} with C' >= c_valid; the kernel leaves channels c_valid .. C'-1 of the device copy alone, so after the copy
// back the host's pad channels are undefined (deepfusion.h says so).  The table is copied at construction: nothing to hash.  src is registered as a read,
// idx / dst and val as writes (op_state).  Batch sharding is op_base's: every tensor is batch-major. ----
class op_head : public op_base {
public:
  op_head(const std::unique_ptr<memory> &src, std::unique_ptr<memory> &out, memory *val, int mode, int k, int c_valid,
          const std::array<uint32_t, 256> *table, float out_scale)
      : op_base(destroy_as<dfx_head_t, dfx_head_destroy>), src_(src.get()), out_(out.get()), val_(val) {
    using fmt = memory::format;
    if (!src_ || !out_) error_and_exit("Init Head op failed! (null tensor)");
    if (src_->dim_format() != fmt::nhwc || out_->dim_format() != fmt::nhwc || (val_ && val_->dim_format() != fmt::nhwc))
      error_and_exit("Init Head op failed! (format)");
    auto i = src_->std_dims(), o = out_->std_dims();
    if (i[0] != o[0] || i[2] != o[2] || i[3] != o[3]) error_and_exit("Init Head op failed! (batch size / height / width do not equal)");
    if (val_ && (val_->std_dims() != o || val_->data_type() != src_->data_type())) error_and_exit("Init Head op failed! (val must have idx's dims and src's data type)");
    dfx_head_desc d;
    memset(&d, 0, sizeof(d));
    const long long px = (long long)i[2] * i[3];
    d.rows = (long long)i[0] * px;
    d.mode = mode;
    d.src_dt = to_dfx_dtype(src_->data_type());
    d.dst_dt = to_dfx_dtype(out_->data_type());
    d.c = c_valid > 0 ? c_valid : i[1];
    d.src_ld = i[1];
    d.k = k;
    if (mode == DFX_HEAD_TOPK) {
      if (o[1] != k) error_and_exit("Init Head op failed! (idx must be {bs, k, h, w})");
      d.idx_ld = o[1];
    } else {
      d.dst_ld = o[1];
    }
    d.out_scale = out_scale;
    d.force_path = -1;
    const size_t src_img = (size_t)px * i[1] * dtype_size(src_->data_type());
    const size_t out_img = (size_t)px * o[1] * dtype_size(out_->data_type());
    const size_t val_img = val_ ? (size_t)px * o[1] * dtype_size(val_->data_type()) : 0;
    reads(src_, src_img);
    writes(out_, out_img);
    writes(val_, val_img);  // (absent unless top_k() was given one)
    build(i[0], [&](int n) -> void * {
      dfx_head_desc ds = d;
      ds.rows = (long long)n * px;
      dfx_head_t *h = static_cast<dfx_head_t *>(create_or_exit(dfx_head_create, ds, "Init Head op failed! (%s)"));
      if (table && dfx_head_set_table(h, table->data()) != DFX_OK) error_and_exit("Init Head op failed! (%s)", dfx_last_error());
      return h;
    });
  }

protected:
  void launch(void *h, void *const *p, dfx_stream_t s) override {
    check_dfx(dfx_head_submit(static_cast<dfx_head_t *>(h), p[0], p[1], p[2], s), "head submit");
  }
  const char *name() override { return "head"; }

private:
  memory *src_, *out_, *val_;
};

// ---- int8 layer norm / RMS norm (dfx_lnorm_*) over the rows of an nhwc tensor (rows = bs * h * w, src_ld = C, c_valid <= C);
// dst {bs, C', h, w} with C' >= c_valid, whose pad channels the kernel leaves alone (undefined on the host afterwards, as
// op_head's softmax).  gamma / beta / shifts are copied at construction.  src is registered as a read, dst as a write
// (op_state).  Batch sharding is op_base's: both tensors are batch-major. ----
class op_layer_norm : public op_base {
public:
  op_layer_norm(const std::unique_ptr<memory> &src, const std::vector<float> &gamma, const std::vector<float> &beta,
                std::unique_ptr<memory> &dst, float eps, norm_mode mode, const std::vector<u8> &shifts, int c_valid)
      : op_base(destroy_as<dfx_lnorm_t, dfx_lnorm_destroy>), src_(src.get()), dst_(dst.get()) {
    using fmt = memory::format;
    if (!src_ || !dst_) error_and_exit("Init LayerNorm op failed! (null tensor)");
    if (src_ == dst_) error_and_exit("Init LayerNorm op failed! (in place is not built)");
    if (src_->dim_format() != fmt::nhwc || dst_->dim_format() != fmt::nhwc) error_and_exit("Init LayerNorm op failed! (format)");
    auto i = src_->std_dims(), o = dst_->std_dims();
    if (i[0] != o[0] || i[2] != o[2] || i[3] != o[3]) error_and_exit("Init LayerNorm op failed! (batch size / height / width do not equal)");
    dfx_lnorm_desc d;
    memset(&d, 0, sizeof(d));
    const long long px = (long long)i[2] * i[3];
    d.rows = (long long)i[0] * px;
    d.mode = mode == norm_mode::rms ? DFX_LNORM_RMS : DFX_LNORM_LAYER;
    d.src_dt = to_dfx_dtype(src_->data_type());
    d.dst_dt = to_dfx_dtype(dst_->data_type());
    d.c = c_valid > 0 ? c_valid : i[1];
    d.src_ld = i[1];
    d.dst_ld = o[1];
    d.eps = eps;
    d.force_path = -1;
    if ((long long)gamma.size() != d.c) error_and_exit("Init LayerNorm op failed! (gamma must have c_valid values)");
    if (!beta.empty() && (long long)beta.size() != d.c) error_and_exit("Init LayerNorm op failed! (beta must be empty or have c_valid values)");
    if (!shifts.empty() && (long long)shifts.size() != d.c) error_and_exit("Init LayerNorm op failed! (shifts must be empty or have c_valid values)");
    const float *b = beta.empty() ? nullptr : beta.data();
    const u8 *s = shifts.empty() ? nullptr : shifts.data();
    const size_t src_img = (size_t)px * i[1] * dtype_size(src_->data_type());
    const size_t dst_img = (size_t)px * o[1] * dtype_size(dst_->data_type());
    reads(src_, src_img);
    writes(dst_, dst_img);
    build(i[0], [&](int n) -> void * {
      dfx_lnorm_desc ds = d;
      ds.rows = (long long)n * px;
      dfx_lnorm_t *h = static_cast<dfx_lnorm_t *>(create_or_exit(dfx_lnorm_create, ds, "Init LayerNorm op failed! (%s)"));
      if (dfx_lnorm_set_params(h, gamma.data(), b, s) != DFX_OK) error_and_exit("Init LayerNorm op failed! (%s)", dfx_last_error());
      return h;
    });
  }

protected:
  void launch(void *h, void *const *p, dfx_stream_t s) override {
    check_dfx(dfx_lnorm_submit(static_cast<dfx_lnorm_t *>(h), p[0], p[1], s), "lnorm submit");
  }
  const char *name() override { return "layer_norm"; }

private:
  memory *src_, *dst_;
};

// ---- int8 token linear layer (dfx_linear_*) over the rows of an nhwc tensor (rows = bs * h * w, src_ld = C, k <= C); dst
// {bs, C', h, w} with C' >= n, whose pad channels the kernel leaves alone (undefined on the host afterwards, as op_layer_norm's).
// The weights are a plain oihw {n, k, 1, 1} tensor, hashed and re-packed by op_base; the table is copied at
// construction.  src is registered as a read, dst as a write (op_state).  One device: the op is not sharded. ----
class op_linear : public op_base {
public:
  op_linear(const std::unique_ptr<memory> &src, const std::unique_ptr<memory> &wei, const std::unique_ptr<memory> &bia,
            std::unique_ptr<memory> &dst, bool relu, const std::vector<float> &scales, round_mode rm, int k_valid, const std::vector<u8> &table,
            memory::dtype table_in)
      : op_base(destroy_as<dfx_linear_t, dfx_linear_destroy>), src_(src.get()), wei_(wei.get()), bia_(bia.get()), dst_(dst.get()), scales_(scales) {
    using fmt = memory::format;
    if (!src_ || !wei_ || !dst_) error_and_exit("Init Linear op failed! (null tensor)");
    if (src_ == dst_) error_and_exit("Init Linear op failed! (in place is not built)");
    if (wei_->data_type() != memory::dtype::s8 || src_->dim_format() != fmt::nhwc || dst_->dim_format() != fmt::nhwc ||
        wei_->dim_format() != fmt::oihw || (bia_ && bia_->dim_format() != fmt::x))
      error_and_exit("Init Linear op failed! (data type / format)");
    auto i = src_->std_dims(), w = wei_->std_dims(), o = dst_->std_dims();
    if (i[0] != o[0] || i[2] != o[2] || i[3] != o[3]) error_and_exit("Init Linear op failed! (batch size / height / width do not equal)");
    const int k = k_valid > 0 ? k_valid : i[1];
    if (w[1] != k || w[2] != 1 || w[3] != 1) error_and_exit("Init Linear op failed! (weights must be {n, k, 1, 1})");
    if (bia_ && (int)bia_->size() != w[0]) error_and_exit("Init Linear op failed! (Bias channel do not match)");
    if (!table.empty() && table.size() != 256) error_and_exit("Init Linear op failed! (the table must be empty or have 256 bytes)");
    if (table.empty() != (table_in == memory::dtype::undef)) error_and_exit("Init Linear op failed! (a table needs table_in, and table_in a table)");
    dfx_linear_desc d;
    memset(&d, 0, sizeof(d));
    d.rows = (long long)i[0] * i[2] * i[3];
    d.k = k; d.n = w[0];
    d.src_dt = to_dfx_dtype(src_->data_type());
    d.dst_dt = to_dfx_dtype(dst_->data_type());
    d.bia_dt = bia_ ? to_dfx_dtype(bia_->data_type()) : DFX_UNDEF;
    d.relu = relu;
    d.round_mode = to_dfx_round(rm);
    d.nscales = (int)scales_.size();
    d.lut_in_dt = table.empty() ? DFX_UNDEF : to_dfx_dtype(table_in);
    d.force_path = -1;
    d.src_ld = i[1];
    d.dst_ld = o[1];
    reads(src_);
    writes(dst_);
    borrows(wei_); borrows(bia_);
    build(0, [&](int) -> void * {
      dfx_linear_t *h = static_cast<dfx_linear_t *>(create_or_exit(dfx_linear_create, d, "Init Linear op failed! (%s)"));
      if (!table.empty() && dfx_linear_set_table(h, table.data()) != DFX_OK) error_and_exit("Init Linear op failed! (%s)", dfx_last_error());
      return h;
    });
  }

protected:
  void pack(void *h) override {
    check_dfx(dfx_linear_set_weights(static_cast<dfx_linear_t *>(h), (const int8_t *)wei_->host_data(), bia_ ? bia_->host_data() : nullptr,
                                     scales_.data()),
              "linear set_weights");
  }
  void launch(void *h, void *const *p, dfx_stream_t s) override {
    check_dfx(dfx_linear_submit(static_cast<dfx_linear_t *>(h), p[0], p[1], s), "linear submit");
  }
  const char *name() override { return "linear"; }

private:
  memory *src_, *wei_, *bia_, *dst_;
  std::vector<float> scales_;
};

// ---- int8 patch embedding (dfx_patchembed_*): a non-overlapping conv over an nhwc u8 / s8 image whose dst is a token matrix,
// an nhwc tensor {bs, C', H, W} read as bs * H * W rows of C' channels: H * W >= tok_offset + th * tw rows per image, C' >= oc.
// The kernel leaves alone the pad channels, the rows behind the tokens and, without a prefix, the rows in front of them
// (undefined on the host afterwards, as op_linear's pad channels).  The weights are a plain oihw {oc, ic, ph, pw} tensor, hashed
// and re-packed by op_base; table and prefix are copied at construction, into every shard's handle.  Batch sharding is
// op_base's: both tensors are batch-major and the op is per image. ----
class op_patch_embed : public op_base {
public:
  op_patch_embed(const std::unique_ptr<memory> &src, const std::unique_ptr<memory> &wei, const std::unique_ptr<memory> &bia,
                 std::unique_ptr<memory> &dst, bool relu, const std::vector<float> &scales, round_mode rm, const std::vector<float> &table,
                 int tok_offset, const std::vector<u8> &prefix)
      : op_base(destroy_as<dfx_patchembed_t, dfx_patchembed_destroy>), src_(src.get()), wei_(wei.get()), bia_(bia.get()), dst_(dst.get()), scales_(scales) {
    using fmt = memory::format;
    if (!src_ || !wei_ || !dst_) error_and_exit("Init PatchEmbed op failed! (null tensor)");
    if (src_ == dst_) error_and_exit("Init PatchEmbed op failed! (in place is not built)");
    if (wei_->data_type() != memory::dtype::s8 || src_->dim_format() != fmt::nhwc || dst_->dim_format() != fmt::nhwc ||
        wei_->dim_format() != fmt::oihw || (bia_ && bia_->dim_format() != fmt::x))
      error_and_exit("Init PatchEmbed op failed! (data type / format)");
    auto i = src_->std_dims(), w = wei_->std_dims(), o = dst_->std_dims();
    if (i[0] != o[0]) error_and_exit("Init PatchEmbed op failed! (Batch size do not equal)");
    if (w[1] != i[1] || w[2] < 1 || w[3] < 1) error_and_exit("Init PatchEmbed op failed! (weights must be {oc, ic, ph, pw})");
    if (bia_ && (int)bia_->size() != w[0]) error_and_exit("Init PatchEmbed op failed! (Bias channel do not match)");
    dfx_patchembed_desc d;
    memset(&d, 0, sizeof(d));
    d.bs = i[0]; d.ic = i[1]; d.ih = i[2]; d.iw = i[3];
    d.ph = w[2]; d.pw = w[3]; d.th = d.ih / d.ph; d.tw = d.iw / d.pw; d.oc = w[0];
    d.src_dt = to_dfx_dtype(src_->data_type());
    d.dst_dt = to_dfx_dtype(dst_->data_type());
    d.bia_dt = bia_ ? to_dfx_dtype(bia_->data_type()) : DFX_UNDEF;
    d.relu = relu;
    d.round_mode = to_dfx_round(rm);
    d.nscales = (int)scales_.size();
    d.table = table.empty() ? 0 : 1;
    d.tok_offset = tok_offset;
    d.force_path = -1;
    d.img_rows = (long long)o[2] * o[3];
    d.dst_ld = o[1];
    if (!table.empty() && table.size() != (size_t)d.th * d.tw * d.oc) error_and_exit("Init PatchEmbed op failed! (the table must be empty or hold th * tw * oc floats)");
    if (!prefix.empty() && (tok_offset < 1 || prefix.size() != (size_t)tok_offset * d.oc * dtype_size(dst_->data_type())))
      error_and_exit("Init PatchEmbed op failed! (the prefix must be empty or hold tok_offset * oc elements of dst's type)");
    const size_t src_img = (size_t)d.ih * d.iw * d.ic;
    const size_t dst_img = (size_t)d.img_rows * d.dst_ld * dtype_size(dst_->data_type());
    reads(src_, src_img);
    writes(dst_, dst_img);
    borrows(wei_); borrows(bia_);
    build(d.bs, [&](int n) -> void * {
      dfx_patchembed_desc ds = d;
      ds.bs = n;
      dfx_patchembed_t *h = static_cast<dfx_patchembed_t *>(create_or_exit(dfx_patchembed_create, ds, "Init PatchEmbed op failed! (%s)"));
      if (!table.empty() && dfx_patchembed_set_table(h, table.data(), d.oc) != DFX_OK) error_and_exit("Init PatchEmbed op failed! (%s)", dfx_last_error());
      if (!prefix.empty() && dfx_patchembed_set_prefix(h, prefix.data()) != DFX_OK) error_and_exit("Init PatchEmbed op failed! (%s)", dfx_last_error());
      return h;
    });
  }

protected:
  void pack(void *h) override {
    check_dfx(dfx_patchembed_set_weights(static_cast<dfx_patchembed_t *>(h), (const int8_t *)wei_->host_data(), bia_ ? bia_->host_data() : nullptr,
                                         scales_.data()),
              "patch_embed set_weights");
  }
  void launch(void *h, void *const *p, dfx_stream_t s) override {
    check_dfx(dfx_patchembed_submit(static_cast<dfx_patchembed_t *>(h), p[0], p[1], s), "patch_embed submit");
  }
  const char *name() override { return "patch_embed"; }

private:
  memory *src_, *wei_, *bia_, *dst_;
  std::vector<float> scales_;
};

// ---- window partition / reverse (dfx_window_*): the tokens of an nhwc grid {bs, C, h, w} gathered into the rows of an nhwc
// tensor {bs, C', H, W} with H * W = hp * wp (bs * nW windows of wh * ww rows), or back.  Data movement only: no weights, nothing
// to pack.  Channels from c on are neither read nor written (undefined on the host afterwards, as op_layer_norm's pad channels).
// src is registered as a read, dst as a write (op_state).  Batch sharding is op_base's: both tensors are batch-major and the
// row map is per image. ----
class op_window : public op_base {
public:
  op_window(int dir, memory *grid, memory *windows, const window_shape &ws, uint32_t pad_value, int c_valid)
      : op_base(destroy_as<dfx_window_t, dfx_window_destroy>) {
    using fmt = memory::format;
    const char *who = dir == DFX_WINDOW_PARTITION ? "WindowPartition" : "WindowReverse";
    if (!grid || !windows) error_and_exit("Init %s op failed! (null tensor)", who);
    if (grid == windows) error_and_exit("Init %s op failed! (in place is not built)", who);
    if (grid->dim_format() != fmt::nhwc || windows->dim_format() != fmt::nhwc || grid->data_type() != windows->data_type())
      error_and_exit("Init %s op failed! (data type / format)", who);
    auto g = grid->std_dims(), w = windows->std_dims();
    if (g[0] != w[0]) error_and_exit("Init %s op failed! (Batch size do not equal)", who);
    dfx_window_desc d;
    memset(&d, 0, sizeof(d));
    d.dir = dir;
    d.dt = to_dfx_dtype(grid->data_type());
    d.bs = g[0]; d.h = g[2]; d.w = g[3];
    d.c = c_valid > 0 ? c_valid : (g[1] < w[1] ? g[1] : w[1]);
    d.wh = ws.wh; d.ww = ws.ww; d.shift_y = ws.shift_y; d.shift_x = ws.shift_x;
    d.order = ws.col_major ? DFX_WINDOW_COL_MAJOR : DFX_WINDOW_ROW_MAJOR;
    d.grid_ld = g[1];
    d.win_ld = w[1];
    d.pad_value = pad_value;
    d.force_path = -1;
    if (ws.wh < 1 || ws.ww < 1) error_and_exit("Init %s op failed! (the window must be positive)", who);
    const long long hp = ((long long)d.h + ws.wh - 1) / ws.wh * ws.wh, wp = ((long long)d.w + ws.ww - 1) / ws.ww * ws.ww;
    if ((long long)w[2] * w[3] != hp * wp) error_and_exit("Init %s op failed! (the window side must hold hp * wp rows per image)", who);
    const size_t es = dtype_size(grid->data_type());
    const size_t grid_img = (size_t)d.h * d.w * g[1] * es, win_img = (size_t)(hp * wp) * w[1] * es;
    if (dir == DFX_WINDOW_PARTITION) {
      reads(grid, grid_img);
      writes(windows, win_img);
    } else {
      reads(windows, win_img);
      writes(grid, grid_img);
    }
    build(d.bs, [&](int n) -> void * {
      dfx_window_desc ds = d;
      ds.bs = n;
      return create_or_exit(dfx_window_create, ds, dir == DFX_WINDOW_PARTITION ? "Init WindowPartition op failed! (%s)" : "Init WindowReverse op failed! (%s)");
    });
  }

protected:
  void launch(void *h, void *const *p, dfx_stream_t s) override {
    check_dfx(dfx_window_submit(static_cast<dfx_window_t *>(h), p[0], p[1], s), "window submit");
  }
  const char *name() override { return "window"; }
};

// ---- image-wide top-K with peak filter (dfx_select_*): the k best elements of every image of an nhwc score tensor,
// optionally only 3x3 local maxima and only elements >= min_val, with whole pixel rows of further nhwc tensors gathered
// behind it.  src and the gather sources are registered as reads, idx, count, val and the gather destinations as writes
// (op_state).  One handle on one device: DEEPFUSION_DEVICES does not shard this op (its results are per image, but a
// detector's batch is small). ----
class op_select : public op_base {
public:
  op_select(const std::unique_ptr<memory> &src, std::unique_ptr<memory> &idx, memory *val, std::unique_ptr<memory> &count, int k,
            bool peak3, int min_val, int c_valid, const std::vector<memory *> &gsrc, const std::vector<memory *> &gdst)
      : op_base(destroy_as<dfx_select_t, dfx_select_destroy>), src_(src.get()), idx_(idx.get()), val_(val), count_(count.get()), gsrc_(gsrc), gdst_(gdst) {
    using fmt = memory::format;
    using dt = memory::dtype;
    if (!src_ || !idx_ || !count_) error_and_exit("Init Select op failed! (null tensor)");
    if (src_->dim_format() != fmt::nhwc) error_and_exit("Init Select op failed! (format)");
    auto i = src_->std_dims(), o = idx_->std_dims();
    if (idx_->data_type() != dt::s32 || o[0] != i[0] || o[1] != k || o[2] != 1 || o[3] != 1)
      error_and_exit("Init Select op failed! (idx must be s32 {bs, k, 1, 1})");
    if (val_ && (val_->std_dims() != o || val_->data_type() != src_->data_type()))
      error_and_exit("Init Select op failed! (val must have idx's dims and src's data type)");
    if (count_->data_type() != dt::s32 || count_->size() != (size_t)i[0]) error_and_exit("Init Select op failed! (count must be s32 {bs})");
    if (gsrc_.size() != gdst_.size() || gsrc_.size() > (size_t)DFX_SELECT_MAX_GATHER) error_and_exit("Init Select op failed! (gather lists)");
    dfx_select_desc d;
    memset(&d, 0, sizeof(d));
    d.bs = i[0]; d.h = i[2]; d.w = i[3];
    d.c = c_valid > 0 ? c_valid : i[1];
    d.src_ld = i[1];
    d.src_dt = to_dfx_dtype(src_->data_type());
    d.k = k;
    d.idx_ld = k;
    d.peak = peak3 ? DFX_SELECT_PEAK3 : DFX_SELECT_ALL;
    d.min_val = min_val == select_all_values ? (src_->data_type() == dt::s8 ? -128 : 0) : min_val;
    d.n_gather = (int)gsrc_.size();
    for (size_t g = 0; g < gsrc_.size(); ++g) {
      memory *s = gsrc_[g], *t = gdst_[g];
      if (!s || !t || s->dim_format() != fmt::nhwc || t->dim_format() != fmt::nhwc) error_and_exit("Init Select op failed! (gather tensor)");
      auto sd = s->std_dims(), td = t->std_dims();
      if (sd[0] != i[0] || sd[2] != i[2] || sd[3] != i[3]) error_and_exit("Init Select op failed! (a gather source must share bs, h, w with src)");
      if (t->data_type() != s->data_type() || td[0] != i[0] || td[1] != sd[1] || td[2] != k || td[3] != 1)
        error_and_exit("Init Select op failed! (a gather destination must be {bs, C, k, 1} of its source's type)");
      d.row_bytes[g] = d.pixel_stride_bytes[g] = (int)(sd[1] * dtype_size(s->data_type()));
    }
    d.force_path = -1;
    reads(src_);
    for (memory *m : gsrc_) reads(m);
    writes(idx_);
    writes(count_);
    writes(val_);  // (absent unless given)
    for (memory *m : gdst_) writes(m);
    build(0, [&](int) -> void * { return create_or_exit(dfx_select_create, d, "Init Select op failed! (%s)"); });
  }

protected:
  void launch(void *h, void *const *p, dfx_stream_t s) override {
    const void *gs[DFX_SELECT_MAX_GATHER] = {nullptr, nullptr, nullptr, nullptr};
    void *gd[DFX_SELECT_MAX_GATHER] = {nullptr, nullptr, nullptr, nullptr};
    void *const *w = p + n_reads();  // idx, count, val, the gather destinations
    for (size_t g = 0; g < gsrc_.size(); ++g) {
      gs[g] = p[1 + g];
      gd[g] = w[3 + g];
    }
    check_dfx(dfx_select_submit(static_cast<dfx_select_t *>(h), p[0], w[0], w[2], w[1], gs, gd, s), "select submit");
  }
  const char *name() override { return "select"; }

private:
  memory *src_, *idx_, *val_, *count_;
  std::vector<memory *> gsrc_, gdst_;
};

// ---- box decode + greedy NMS (dfx_nms_*): what a detector does behind select_top_k().  boxes (or idx, deltas and anchors),
// the two tables and count_in are registered as reads, keep, count and boxes_out as writes (op_state).  The tables are two
// small tensors of the op's own.  One handle on one device: DEEPFUSION_DEVICES does not shard this op, as it does not
// shard select_top_k(). ----
class op_nms : public op_base {
public:
  op_nms(memory *boxes, memory *idx, memory *deltas, memory *anchors, const std::array<float, 256> *tab_c, const std::array<float, 256> *tab_s,
         memory *count_in, memory *keep, memory *count, memory *boxes_out, float iou_thr, int classes, bool per_class, int apx, float clip_w,
         float clip_h)
      : op_base(destroy_as<dfx_nms_t, dfx_nms_destroy>), boxes_(boxes), idx_(idx), deltas_(deltas), anchors_(anchors), count_in_(count_in), keep_(keep), count_(count), boxes_out_(boxes_out) {
    using fmt = memory::format;
    using dt = memory::dtype;
    const bool decode = boxes_ == nullptr;
    if (!keep_ || !count_ || (decode && (!idx_ || !deltas_ || !anchors_))) error_and_exit("Init Nms op failed! (null tensor)");
    if (!decode && per_class && !idx_) error_and_exit("Init Nms op failed! (per-class NMS on boxes needs idx)");
    auto o = keep_->std_dims();
    const int bs = o[0], max_out = o[1];
    if (keep_->data_type() != dt::s32 || o[2] != 1 || o[3] != 1) error_and_exit("Init Nms op failed! (keep must be s32 {bs, max_out, 1, 1})");
    if (count_->data_type() != dt::s32 || count_->size() != (size_t)bs) error_and_exit("Init Nms op failed! (count must be s32 {bs})");
    if (count_in_ && (count_in_->data_type() != dt::s32 || count_in_->size() != (size_t)bs)) error_and_exit("Init Nms op failed! (count_in must be s32 {bs})");
    int n = 0;
    dfx_nms_desc d;
    memset(&d, 0, sizeof(d));
    if (decode) {
      auto i = idx_->std_dims(), q = deltas_->std_dims(), a = anchors_->std_dims();
      n = i[1];
      if (idx_->data_type() != dt::s32 || i[0] != bs || i[2] != 1 || i[3] != 1) error_and_exit("Init Nms op failed! (idx must be s32 {bs, n, 1, 1})");
      if (deltas_->dim_format() != fmt::nhwc || dtype_size(deltas_->data_type()) != 1 || q[0] != bs || q[2] != n || q[3] != 1)
        error_and_exit("Init Nms op failed! (deltas must be a 1-byte nhwc tensor {bs, C, n, 1})");
      if (anchors_->dim_format() != fmt::nhwc || anchors_->data_type() != dt::f32 || a[1] != 4 || a[2] != 1 || a[3] != 1)
        error_and_exit("Init Nms op failed! (anchors must be f32 nhwc {n_anchors, 4, 1, 1})");
      d.row_bytes = q[1];
      d.n_anchors = a[0];
      tab_c_.reset(new memory(memory::nchw_dims{1, 256, 1, 1}, fmt::nhwc, dt::f32));
      tab_s_.reset(new memory(memory::nchw_dims{1, 256, 1, 1}, fmt::nhwc, dt::f32));
      memcpy(tab_c_->data(), tab_c->data(), 1024);
      memcpy(tab_s_->data(), tab_s->data(), 1024);
    } else {
      auto b = boxes_->std_dims();
      n = b[2];
      if (boxes_->dim_format() != fmt::nhwc || boxes_->data_type() != dt::f32 || b[0] != bs || b[1] != 4 || b[3] != 1)
        error_and_exit("Init Nms op failed! (boxes must be f32 nhwc {bs, 4, n, 1})");
      if (idx_ && (idx_->data_type() != dt::s32 || idx_->std_dims() != memory::nchw_dims{bs, n, 1, 1}))
        error_and_exit("Init Nms op failed! (idx must be s32 {bs, n, 1, 1})");
      d.n_anchors = classes > 0 ? 2147483647 / classes : 1;
    }
    if (boxes_out_) {
      auto b = boxes_out_->std_dims();
      if (boxes_out_->dim_format() != fmt::nhwc || boxes_out_->data_type() != dt::f32 || b[0] != bs || b[1] != 4 || b[2] != max_out || b[3] != 1)
        error_and_exit("Init Nms op failed! (boxes_out must be f32 nhwc {bs, 4, max_out, 1})");
    }
    d.bs = bs; d.n = n; d.max_out = max_out; d.keep_ld = max_out;
    d.mode = decode ? DFX_NMS_DECODE : DFX_NMS_BOXES;
    d.per_class = per_class ? 1 : 0;
    d.classes = classes; d.anchors_per_pixel = apx; d.idx_ld = n;
    d.iou_thr = iou_thr; d.clip_w = clip_w; d.clip_h = clip_h;
    d.force_path = -1;
    reads(boxes_);
    reads(idx_);
    reads(deltas_);
    reads(anchors_);
    reads(tab_c_.get(), 0, true);  // (the op's own tensors: uploaded once)
    reads(tab_s_.get(), 0, true);
    reads(count_in_);
    writes(keep_);
    writes(count_);
    writes(boxes_out_);
    build(0, [&](int) -> void * { return create_or_exit(dfx_nms_create, d, "Init Nms op failed! (%s)"); });
  }
  ~op_nms() override { teardown(); }  // (before tab_c_ and tab_s_ go: a launch may still read them)

protected:
  void launch(void *h, void *const *p, dfx_stream_t s) override {
    dfx_nms_io io;
    memset(&io, 0, sizeof(io));
    io.boxes = p[0]; io.idx = p[1]; io.deltas = p[2]; io.anchors = p[3]; io.tab_c = p[4]; io.tab_s = p[5]; io.count_in = p[6];
    io.keep = p[7]; io.count = p[8]; io.boxes_out = p[9];
    check_dfx(dfx_nms_submit(static_cast<dfx_nms_t *>(h), &io, s), "nms submit");
  }
  const char *name() override { return "nms"; }

private:
  memory *boxes_, *idx_, *deltas_, *anchors_, *count_in_, *keep_, *count_, *boxes_out_;
  std::unique_ptr<memory> tab_c_, tab_s_;
};

// ---- RoIAlign (dfx_roialign_*): what a two-stage detector does behind box_nms().  The levels, boxes and count / batch_idx
// are registered as reads, dst as a write (op_state).  One handle on one device: DEEPFUSION_DEVICES does not shard this op,
// as it does not shard select_top_k(). ----
class op_roialign : public op_base {
public:
  op_roialign(const std::vector<memory *> &levels, const std::vector<float> &scales, const std::vector<float> &thr, memory *boxes, memory *count,
              memory *batch_idx, memory *dst, int sampling_ratio, bool aligned, int c_valid)
      : op_base(destroy_as<dfx_roialign_t, dfx_roialign_destroy>), levels_(levels), boxes_(boxes), count_(count), batch_idx_(batch_idx), dst_(dst) {
    using fmt = memory::format;
    using dt = memory::dtype;
    if (levels_.empty() || levels_.size() > (size_t)DFX_ROIALIGN_MAX_LEVELS || !levels_[0] || !boxes_ || !dst_)
      error_and_exit("Init RoiAlign op failed! (null tensor, or not 1 .. 4 levels)");
    if (scales.size() != levels_.size() || thr.size() + 1 != levels_.size())
      error_and_exit("Init RoiAlign op failed! (one spatial scale per level and levels - 1 area thresholds)");
    if (batch_idx_ && count_) error_and_exit("Init RoiAlign op failed! (count belongs to the batched form)");
    auto l0 = levels_[0]->std_dims(), o = dst_->std_dims(), b = boxes_->std_dims();
    const int bs = l0[0];
    dfx_roialign_desc d;
    memset(&d, 0, sizeof(d));
    for (size_t l = 0; l < levels_.size(); ++l) {
      memory *m = levels_[l];
      if (!m || m->dim_format() != fmt::nhwc || m->data_type() != levels_[0]->data_type()) error_and_exit("Init RoiAlign op failed! (levels must be nhwc of one dtype)");
      auto i = m->std_dims();
      if (i[0] != bs || i[1] != l0[1]) error_and_exit("Init RoiAlign op failed! (levels must share bs and C)");
      d.h[l] = i[2]; d.w[l] = i[3]; d.src_ld[l] = i[1]; d.spatial_scale[l] = scales[l];
      if (l) d.level_area_thr[l - 1] = thr[l - 1];
    }
    if (boxes_->dim_format() != fmt::nhwc || boxes_->data_type() != dt::f32 || b[1] != 4 || b[3] != 1)
      error_and_exit("Init RoiAlign op failed! (boxes must be f32 nhwc {bs, 4, n, 1} or {R, 4, 1, 1})");
    if (batch_idx_) {
      if (b[2] != 1 || batch_idx_->data_type() != dt::s32 || batch_idx_->size() != (size_t)b[0])
        error_and_exit("Init RoiAlign op failed! (the list form takes boxes {R, 4, 1, 1} and batch_idx s32 {R, 1, 1, 1})");
      d.mode = DFX_ROI_LIST; d.n = b[0];
    } else {
      if (b[0] != bs) error_and_exit("Init RoiAlign op failed! (batched boxes must be {bs, 4, n, 1})");
      if (count_ && (count_->data_type() != dt::s32 || count_->size() != (size_t)bs)) error_and_exit("Init RoiAlign op failed! (count must be s32 {bs})");
      d.mode = DFX_ROI_BATCHED; d.n = b[2];
    }
    const long long rows = d.mode == DFX_ROI_LIST ? d.n : (long long)bs * d.n;
    if (dst_->dim_format() != fmt::nhwc || dst_->data_type() != levels_[0]->data_type() || o[0] != rows || o[1] != l0[1])
      error_and_exit("Init RoiAlign op failed! (dst must be nhwc {R, C, ph, pw} of the levels' dtype)");
    d.bs = bs; d.levels = (int)levels_.size();
    d.c = c_valid > 0 ? c_valid : l0[1];
    d.dt = to_dfx_dtype(dst_->data_type());
    d.ph = o[2]; d.pw = o[3]; d.dst_ld = o[1];
    d.sampling_ratio = sampling_ratio; d.aligned = aligned ? 1 : 0;
    d.force_path = -1;
    for (memory *m : levels_) reads(m);
    reads(boxes_);
    reads(count_);      // (absent in the list form, optional in the batched one)
    reads(batch_idx_);  // (the list form's)
    writes(dst_);
    build(0, [&](int) -> void * { return create_or_exit(dfx_roialign_create, d, "Init RoiAlign op failed! (%s)"); });
  }

protected:
  void launch(void *h, void *const *p, dfx_stream_t s) override {
    dfx_roialign_io io;
    memset(&io, 0, sizeof(io));
    const size_t nl = levels_.size();
    for (size_t l = 0; l < nl; ++l) io.src[l] = p[l];
    io.boxes = p[nl]; io.count = p[nl + 1]; io.batch_idx = p[nl + 2]; io.dst = p[nl + 3];
    check_dfx(dfx_roialign_submit(static_cast<dfx_roialign_t *>(h), &io, s), "roialign submit");
  }
  const char *name() override { return "roialign"; }

private:
  std::vector<memory *> levels_;
  memory *boxes_, *count_, *batch_idx_, *dst_;
};

// ---- batched int8 matrix product (dfx_bmm_*): C[g] = requant(A[g] . B[g](^T)) over matrices that lie in three tensors at the
// strides of matmul_shape.  a and b are registered as reads, c as a write (op_state).  One handle on one device:
// DEEPFUSION_DEVICES does not shard this op (a head-sliced operand is not batch-major). ----
// the dfx_logit_bias_desc of a logit_bias over {rows, cols} products, its table checked against what the layout addresses
// (the library cannot: it only sees a pointer); a layout the library refuses anyway is passed on for it to say why
static dfx_logit_bias_desc logit_bias_desc(const logit_bias &bias, long long rows, long long cols, const char *what) {
  dfx_logit_bias_desc b;
  b.period0 = bias.period0; b.period1 = bias.period1; b.s0 = bias.s0; b.s1 = bias.s1; b.ld = bias.ld;
  if (bias.period0 >= 1 && bias.period1 >= 1 && bias.s0 >= 0 && bias.s1 >= 0 && bias.ld >= 0) {
    const unsigned __int128 need = (unsigned __int128)(bias.period0 - 1) * (unsigned __int128)bias.s0 + (unsigned __int128)(bias.period1 - 1) * (unsigned __int128)bias.s1 +
                                   (unsigned __int128)(bias.ld == 0 ? 0 : rows - 1) * (unsigned __int128)bias.ld + (unsigned __int128)cols;
    if (need > (unsigned __int128)bias.table.size()) error_and_exit("Init %s op failed! (the logit bias's layout reaches beyond its table)", what);
  }
  return b;
}

class op_matmul : public op_base {
public:
  op_matmul(memory *a, memory *b, memory *c, const matmul_shape &sh, const std::vector<float> &scales, bool relu, round_mode rm,
            const logit_bias *bias = nullptr)
      : op_base(destroy_as<dfx_bmm_t, dfx_bmm_destroy>), a_(a), b_(b), c_(c) {
    if (!a_ || !b_ || !c_) error_and_exit("Init MatMul op failed! (null tensor)");
    dfx_bmm_desc d;
    memset(&d, 0, sizeof(d));
    d.batch0 = sh.batch0; d.batch1 = sh.batch1; d.m = sh.m; d.n = sh.n; d.k = sh.k; d.trans_b = sh.trans_b ? 1 : 0;
    d.a_dt = to_dfx_dtype(a_->data_type()); d.b_dt = to_dfx_dtype(b_->data_type()); d.dst_dt = to_dfx_dtype(c_->data_type());
    d.relu = relu ? 1 : 0;
    d.round_mode = to_dfx_round(rm);
    d.nscales = (int)scales.size();
    d.force_path = -1;
    d.a_s0 = sh.a_s0; d.a_s1 = sh.a_s1; d.lda = sh.lda;
    d.b_s0 = sh.b_s0; d.b_s1 = sh.b_s1; d.ldb = sh.ldb;
    d.c_s0 = sh.c_s0; d.c_s1 = sh.c_s1; d.ldc = sh.ldc;
    if (scales.empty()) error_and_exit("Init MatMul op failed! (scales must hold 1 or n floats)");
    reads(a_);
    reads(b_);
    writes(c_);
    build(0, [&](int) -> void * {
      dfx_bmm_t *h = static_cast<dfx_bmm_t *>(create_or_exit(dfx_bmm_create, d, "Init MatMul op failed! (%s)"));
      // every matrix within its tensor: the last row of a and of b up to its valid columns rounded up to 16, which is what
      // the library may read (the create above has found the sizes positive and the strides non-negative)
      const long long brows = sh.trans_b ? sh.n : sh.k, bcols = sh.trans_b ? sh.k : sh.n;
      const long long a_row = std::min<long long>(sh.lda, ((long long)sh.k + 15) / 16 * 16), b_row = std::min<long long>(sh.ldb, (bcols + 15) / 16 * 16);
      const long long a_end = (sh.batch0 - 1) * sh.a_s0 + (sh.batch1 - 1) * sh.a_s1 + (long long)(sh.m - 1) * sh.lda + a_row;
      const long long b_end = (sh.batch0 - 1) * sh.b_s0 + (sh.batch1 - 1) * sh.b_s1 + (brows - 1) * sh.ldb + b_row;
      const long long c_end = (sh.batch0 - 1) * sh.c_s0 + (sh.batch1 - 1) * sh.c_s1 + (long long)(sh.m - 1) * sh.ldc + sh.n;
      if (a_end > (long long)a_->size() || b_end > (long long)b_->size() || c_end > (long long)c_->size())
        error_and_exit("Init MatMul op failed! (a matrix reaches beyond its tensor)");
      if (dfx_bmm_set_scales(h, scales.data()) != DFX_OK) error_and_exit("Init MatMul op failed! (%s)", dfx_last_error());
      if (bias) {
        const dfx_logit_bias_desc bd = logit_bias_desc(*bias, sh.m, sh.n, "MatMul");
        if (dfx_bmm_set_bias(h, &bd, bias->table.data()) != DFX_OK) error_and_exit("Init MatMul op failed! (%s)", dfx_last_error());
      }
      return h;
    });
  }

protected:
  void launch(void *h, void *const *p, dfx_stream_t s) override {
    check_dfx(dfx_bmm_submit(static_cast<dfx_bmm_t *>(h), p[0], p[1], p[2], s), "bmm submit");
  }
  const char *name() override { return "matmul"; }

private:
  memory *a_, *b_, *c_;
};

// ---- fused int8 attention (dfx_attn_*): o[g] = requant(softmax(requant(q[g] . k[g]^T)) . v[g]) over matrices that lie in four
// tensors at the strides of attention_shape.  q, k and v are registered as reads, o as a write (op_state).  One handle on one
// device, like op_matmul. ----
class op_attention : public op_base {
public:
  op_attention(memory *q, memory *k, memory *v, const std::array<uint32_t, 256> &table, memory *o, const attention_shape &sh, float logit_scale,
               const std::vector<float> &out_scales, float prob_scale, bool relu, round_mode rm, const logit_bias *bias = nullptr)
      : op_base(destroy_as<dfx_attn_t, dfx_attn_destroy>), q_(q), k_(k), v_(v), o_(o) {
    if (!q_ || !k_ || !v_ || !o_) error_and_exit("Init Attention op failed! (null tensor)");
    dfx_attn_desc d;
    memset(&d, 0, sizeof(d));
    d.batch0 = sh.batch0; d.batch1 = sh.batch1; d.tq = sh.tq; d.tk = sh.tk; d.d = sh.d; d.dv = sh.dv;
    d.q_dt = to_dfx_dtype(q_->data_type()); d.k_dt = to_dfx_dtype(k_->data_type()); d.v_dt = to_dfx_dtype(v_->data_type());
    d.dst_dt = to_dfx_dtype(o_->data_type());
    d.relu = relu ? 1 : 0;
    d.round_mode = to_dfx_round(rm);
    d.nscales = (int)out_scales.size();
    d.force_path = -1;
    d.prob_scale = prob_scale;
    d.q_s0 = sh.q_s0; d.q_s1 = sh.q_s1; d.ldq = sh.ldq;
    d.k_s0 = sh.k_s0; d.k_s1 = sh.k_s1; d.ldk = sh.ldk;
    d.v_s0 = sh.v_s0; d.v_s1 = sh.v_s1; d.ldv = sh.ldv;
    d.o_s0 = sh.o_s0; d.o_s1 = sh.o_s1; d.ldo = sh.ldo;
    if (out_scales.empty()) error_and_exit("Init Attention op failed! (out_scales must hold 1 or dv floats)");
    reads(q_);
    reads(k_);
    reads(v_);
    writes(o_);
    build(0, [&](int) -> void * {
      dfx_attn_t *h = static_cast<dfx_attn_t *>(create_or_exit(dfx_attn_create, d, "Init Attention op failed! (%s)"));
      // every matrix within its tensor: the last row of q, k and v up to its valid columns rounded up to 16, which is what the
      // library may read (the create above has found the sizes positive and the strides non-negative)
      auto end = [&](long long s0, long long s1, long long ld, long long rows, long long cols, bool read) {
        const long long row = read ? std::min<long long>(ld, (cols + 15) / 16 * 16) : cols;
        return (sh.batch0 - 1) * s0 + (sh.batch1 - 1) * s1 + (rows - 1) * ld + row;
      };
      if (end(sh.q_s0, sh.q_s1, sh.ldq, sh.tq, sh.d, true) > (long long)q_->size() || end(sh.k_s0, sh.k_s1, sh.ldk, sh.tk, sh.d, true) > (long long)k_->size() ||
          end(sh.v_s0, sh.v_s1, sh.ldv, sh.tk, sh.dv, true) > (long long)v_->size() || end(sh.o_s0, sh.o_s1, sh.ldo, sh.tq, sh.dv, false) > (long long)o_->size())
        error_and_exit("Init Attention op failed! (a matrix reaches beyond its tensor)");
      if (dfx_attn_set_table(h, table.data()) != DFX_OK) error_and_exit("Init Attention op failed! (%s)", dfx_last_error());
      if (dfx_attn_set_scales(h, logit_scale, out_scales.data()) != DFX_OK) error_and_exit("Init Attention op failed! (%s)", dfx_last_error());
      if (bias) {
        const dfx_logit_bias_desc bd = logit_bias_desc(*bias, sh.tq, sh.tk, "Attention");
        if (dfx_attn_set_bias(h, &bd, bias->table.data()) != DFX_OK) error_and_exit("Init Attention op failed! (%s)", dfx_last_error());
      }
      return h;
    });
  }

protected:
  void launch(void *h, void *const *p, dfx_stream_t s) override {
    check_dfx(dfx_attn_submit(static_cast<dfx_attn_t *>(h), p[0], p[1], p[2], p[3], s), "attn submit");
  }
  const char *name() override { return "attention"; }

private:
  memory *q_, *k_, *v_, *o_;
};

// ---- squeeze-and-excitation (dfx_se_*) and, with no weights, the global average pooling it starts with.  The two weight
// tensors are plain oihw {cr, c, 1, 1} and {c, cr, 1, 1}; dst may be src.  Weight hashing and batch sharding are
// op_base's: the op is per image, so shards are independent. ----
class op_squeeze_excite : public op_base {
public:
  op_squeeze_excite(const std::unique_ptr<memory> &src, const std::unique_ptr<memory> *wei1, const std::unique_ptr<memory> *bia1,
                    const std::unique_ptr<memory> *wei2, const std::unique_ptr<memory> *bia2, const std::array<u8, 256> *table,
                    std::unique_ptr<memory> &dst, const std::vector<float> &scales1, const std::vector<float> &scales2,
                    const std::vector<float> &out_scales, round_mode rm)
      : op_base(destroy_as<dfx_se_t, dfx_se_destroy>), src_(src.get()), wei1_(wei1 ? wei1->get() : nullptr), bia1_(bia1 ? bia1->get() : nullptr), wei2_(wei2 ? wei2->get() : nullptr),
        bia2_(bia2 ? bia2->get() : nullptr), dst_(dst.get()), pool_only_(!wei1), scales1_(scales1), scales2_(scales2), out_scales_(out_scales) {
    using fmt = memory::format;
    const char *what = pool_only_ ? "GlobalAvgPool" : "SqueezeExcite";
    if (!src_ || !dst_ || (!pool_only_ && (!wei1_ || !wei2_))) error_and_exit("Init %s op failed! (null tensor)", what);
    if (src_->data_type() != memory::dtype::u8 || dst_->data_type() != memory::dtype::u8 || src_->dim_format() != fmt::nhwc ||
        dst_->dim_format() != fmt::nhwc)
      error_and_exit("Init %s op failed! (data type / format)", what);
    auto i = src_->std_dims(), o = dst_->std_dims();
    if (i[0] != o[0]) error_and_exit("Init %s op failed! (Batch size do not equal)", what);
    if (i[1] != o[1]) error_and_exit("Init %s op failed! (Channel do not match)", what);
    dfx_se_desc d;
    memset(&d, 0, sizeof(d));
    d.bs = i[0]; d.c = i[1]; d.ih = i[2]; d.iw = i[3];
    d.cr = 1;
    d.nscales1 = d.nscales2 = d.nscales_out = 1;
    d.bia1_dt = d.bia2_dt = DFX_UNDEF;
    d.round_mode = to_dfx_round(rm);
    d.force_path = -1;
    if (pool_only_) {
      if (o[2] != 1 || o[3] != 1) error_and_exit("Init GlobalAvgPool op failed! (dst must be {bs, c, 1, 1})");
      if (src_ == dst_) error_and_exit("Init GlobalAvgPool op failed! (dst must not be src)");
      d.mode = DFX_SE_SQUEEZE;
    } else {
      if (wei1_->data_type() != memory::dtype::s8 || wei2_->data_type() != memory::dtype::s8 || wei1_->dim_format() != fmt::oihw ||
          wei2_->dim_format() != fmt::oihw || (bia1_ && bia1_->dim_format() != fmt::x) || (bia2_ && bia2_->dim_format() != fmt::x))
        error_and_exit("Init SqueezeExcite op failed! (data type / format)");
      if (o != i) error_and_exit("Init SqueezeExcite op failed! (dst must have src's dims)");
      auto w1 = wei1_->std_dims(), w2 = wei2_->std_dims();
      if (w1[1] != i[1] || w1[2] != 1 || w1[3] != 1 || w2[0] != i[1] || w2[1] != w1[0] || w2[2] != 1 || w2[3] != 1)
        error_and_exit("Init SqueezeExcite op failed! (weights must be {cr, c, 1, 1} and {c, cr, 1, 1})");
      if ((bia1_ && (int)bia1_->size() != w1[0]) || (bia2_ && (int)bia2_->size() != i[1]))
        error_and_exit("Init SqueezeExcite op failed! (Bias channel do not match)");
      table_ = *table;
      d.mode = DFX_SE_SCALE;
      d.cr = w1[0];
      d.bia1_dt = bia1_ ? to_dfx_dtype(bia1_->data_type()) : DFX_UNDEF;
      d.bia2_dt = bia2_ ? to_dfx_dtype(bia2_->data_type()) : DFX_UNDEF;
      d.nscales1 = (int)scales1_.size();
      d.nscales2 = (int)scales2_.size();
      d.nscales_out = (int)out_scales_.size();
    }
    const size_t src_img = (size_t)d.ih * d.iw * d.c, dst_img = pool_only_ ? (size_t)d.c : src_img;
    reads(src_, src_img);
    writes(dst_, dst_img);  // (dst may be src)
    // OPTION: global_avg_pool() borrows nothing, so nothing is hashed and pack() is never called
    if (!pool_only_) {
      borrows(wei1_); borrows(wei2_); borrows(bia1_); borrows(bia2_);
    }
    build(d.bs, [&](int n) -> void * {
      dfx_se_desc ds = d;
      ds.bs = n;
      dfx_se_t *h = nullptr;
      if (dfx_se_create(&ds, &h) != DFX_OK) error_and_exit("Init %s op failed! (%s)", what, dfx_last_error());
      return h;
    });
  }

protected:
  void pack(void *h) override {
    check_dfx(dfx_se_set_weights(static_cast<dfx_se_t *>(h), (const int8_t *)wei1_->host_data(), bia1_ ? bia1_->host_data() : nullptr,
                                 scales1_.data(), (const int8_t *)wei2_->host_data(), bia2_ ? bia2_->host_data() : nullptr, scales2_.data(),
                                 table_.data(), out_scales_.data()),
              "squeeze_excite set_weights");
  }
  void launch(void *h, void *const *p, dfx_stream_t s) override {
    check_dfx(dfx_se_submit(static_cast<dfx_se_t *>(h), p[0], p[1], s), "squeeze_excite submit");
  }
  const char *name() override { return pool_only_ ? "global_avg_pool" : "squeeze_excite"; }

private:
  memory *src_, *wei1_, *bia1_, *wei2_, *bia2_, *dst_;
  bool pool_only_;  // no weights: global_avg_pool()
  std::array<u8, 256> table_;
  std::vector<float> scales1_, scales2_, out_scales_;
};

// ---- depthwise + pointwise conv (dfx_dwpw_*): depthwise_conv() with a u8 result followed by a 1x1 conv(), behind one
// handle.  force_path stays -1 (auto), so the path is the library's choice (dfx.h, AUTO RULE at DFX_DWPW_FUSED).  The depthwise weights are a plain oihw
// {c, 1, kh, kw} tensor, the pointwise weights OIhw4i16o4i {oc, c, 1, 1}; dst's dims give the output size. ----
class op_depthwise_separable_conv : public op_base {
public:
  op_depthwise_separable_conv(const std::unique_ptr<memory> &src, const std::unique_ptr<memory> &wei, const std::unique_ptr<memory> &bia,
                              std::array<int, 2> stride, std::array<int, 2> padding, const std::unique_ptr<memory> &wei_pw,
                              const std::unique_ptr<memory> &bia_pw, std::unique_ptr<memory> &dst, bool relu,
                              const std::vector<float> &scales, const std::vector<float> &scales_pw, round_mode rm,
                              round_mode rm_pw)
      : op_base(destroy_as<dfx_dwpw_t, dfx_dwpw_destroy>), src_(src.get()), wei_(wei.get()), bia_(bia.get()), wei_pw_(wei_pw.get()), bia_pw_(bia_pw.get()), dst_(dst.get()),
        scales_(scales), scales_pw_(scales_pw) {
    using fmt = memory::format;
    if (!src_ || !wei_ || !wei_pw_ || !dst_) error_and_exit("Init DepthwiseSeparableConv op failed! (null tensor)");
    if (src_->data_type() != memory::dtype::u8 || wei_->data_type() != memory::dtype::s8 || src_->dim_format() != fmt::nhwc ||
        dst_->dim_format() != fmt::nhwc || wei_->dim_format() != fmt::oihw || (bia_ && bia_->dim_format() != fmt::x) ||
        wei_pw_->data_type() != memory::dtype::s8 || wei_pw_->dim_format() != fmt::OIhw4i16o4i ||
        (bia_pw_ && bia_pw_->dim_format() != fmt::x))
      error_and_exit("Init DepthwiseSeparableConv op failed! (data type / format)");
    auto i = src_->std_dims(), w = wei_->std_dims(), o = dst_->std_dims(), p = wei_pw_->std_dims();
    if (i[0] != o[0]) error_and_exit("Init DepthwiseSeparableConv op failed! (Batch size do not equal)");
    if (w[0] != i[1] || w[1] != 1) error_and_exit("Init DepthwiseSeparableConv op failed! (weights must be {c, 1, kh, kw})");
    if (p[1] != i[1] || p[2] != 1 || p[3] != 1) error_and_exit("Init DepthwiseSeparableConv op failed! (pointwise weights must be {oc, c, 1, 1})");
    if (o[1] != p[0]) error_and_exit("Init DepthwiseSeparableConv op failed! (Output channel do not match)");
    if (bia_pw_ && (int)bia_pw_->size() != p[0]) error_and_exit("Init DepthwiseSeparableConv op failed! (Bias channel do not match)");
    if (bia_ && (int)bia_->size() != i[1]) error_and_exit("Init DepthwiseSeparableConv op failed! (Bias channel do not match)");
    dfx_dwpw_desc d;
    memset(&d, 0, sizeof(d));
    d.bs = i[0]; d.c = i[1]; d.ih = i[2]; d.iw = i[3]; d.oh = o[2]; d.ow = o[3];
    d.kh = w[2]; d.kw = w[3]; d.sh = stride[0]; d.sw = stride[1]; d.pad_t = padding[0]; d.pad_l = padding[1];
    d.oc = p[0];
    d.dst_dt = to_dfx_dtype(dst_->data_type());
    d.bia0_dt = bia_ ? to_dfx_dtype(bia_->data_type()) : DFX_UNDEF;
    d.bia1_dt = bia_pw_ ? to_dfx_dtype(bia_pw_->data_type()) : DFX_UNDEF;
    d.relu = relu;
    d.round_mode0 = to_dfx_round(rm);
    d.round_mode1 = to_dfx_round(rm_pw);
    d.nscales0 = (int)scales_.size();
    d.nscales1 = (int)scales_pw_.size();
    d.force_path = -1;
    const size_t src_img = (size_t)d.ih * d.iw * d.c;
    const size_t dst_img = (size_t)d.oh * d.ow * d.oc * dtype_size(dst_->data_type());
    reads(src_, src_img);
    writes(dst_, dst_img);
    borrows(wei_); borrows(bia_); borrows(wei_pw_); borrows(bia_pw_);
    build(d.bs, [&](int n) -> void * {
      dfx_dwpw_desc ds = d;
      ds.bs = n;
      return create_or_exit(dfx_dwpw_create, ds, "Init DepthwiseSeparableConv op failed! (%s)");
    });
  }

protected:
  void pack(void *h) override {
    check_dfx(dfx_dwpw_set_weights(static_cast<dfx_dwpw_t *>(h), (const int8_t *)wei_->host_data(), bia_ ? bia_->host_data() : nullptr,
                                   scales_.data(), (const int8_t *)wei_pw_->host_data(), bia_pw_ ? bia_pw_->host_data() : nullptr,
                                   scales_pw_.data()),
              "depthwise_separable_conv set_weights");
  }
  void launch(void *h, void *const *p, dfx_stream_t s) override {
    check_dfx(dfx_dwpw_submit(static_cast<dfx_dwpw_t *>(h), p[0], p[1], s), "depthwise_separable_conv submit");
  }
  const char *name() override { return "depthwise_separable_conv"; }

private:
  memory *src_, *wei_, *bia_, *wei_pw_, *bia_pw_, *dst_;
  std::vector<float> scales_, scales_pw_;
};

}  // namespace

std::unique_ptr<op> depthwise_conv(const std::unique_ptr<memory> &src, const std::unique_ptr<memory> &wei,
                                   const std::unique_ptr<memory> &bia, std::array<int, 2> sz_stride,
                                   std::array<int, 2> sz_padding, std::unique_ptr<memory> &dst, bool relu,
                                   std::vector<float> scales, round_mode rm) {
  return std::unique_ptr<op>(new op_depthwise_conv(src, wei, bia, sz_stride, sz_padding, dst, relu, scales, rm));
}

std::unique_ptr<op> grouped_conv(const std::unique_ptr<memory> &src, const std::unique_ptr<memory> &wei,
                                 const std::unique_ptr<memory> &bia, int groups, std::array<int, 2> sz_stride,
                                 std::array<int, 2> sz_padding, std::unique_ptr<memory> &dst, bool relu,
                                 std::vector<float> scales, round_mode rm) {
  return std::unique_ptr<op>(new op_grouped_conv(src, wei, bia, groups, sz_stride, sz_padding, dst, relu, scales, rm));
}

std::unique_ptr<op> image_conv(const std::unique_ptr<memory> &src, const std::unique_ptr<memory> &wei,
                               const std::unique_ptr<memory> &bia, std::array<int, 2> sz_stride,
                               std::array<int, 2> sz_padding, std::unique_ptr<memory> &dst, bool relu,
                               std::vector<float> scales, round_mode rm) {
  return std::unique_ptr<op>(new op_image_conv(src, wei, bia, sz_stride, sz_padding, dst, relu, scales, rm));
}

std::unique_ptr<op> deconvolution(const std::unique_ptr<memory> &src, const std::unique_ptr<memory> &wei,
                               const std::unique_ptr<memory> &bia, std::array<int, 2> sz_stride,
                               std::array<int, 2> sz_padding, std::unique_ptr<memory> &dst, bool relu,
                               std::vector<float> scales, round_mode rm) {
  return std::unique_ptr<op>(new op_deconvolution(src, wei, bia, sz_stride, sz_padding, dst, relu, scales, rm));
}

std::unique_ptr<op> dilated_conv(const std::unique_ptr<memory> &src, const std::unique_ptr<memory> &wei,
                                 const std::unique_ptr<memory> &bia, std::array<int, 2> sz_stride,
                                 std::array<int, 2> sz_dilation, std::array<int, 2> sz_padding,
                                 std::unique_ptr<memory> &dst, bool relu, std::vector<float> scales, round_mode rm) {
  return std::unique_ptr<op>(new op_dilated_conv(src, wei, bia, sz_stride, sz_dilation, sz_padding, dst, relu, scales, rm));
}

std::unique_ptr<op> resize(const std::unique_ptr<memory> &src, std::unique_ptr<memory> &dst, resize_algo algo, resize_coord coord) {
  return std::unique_ptr<op>(new op_resize(src, nullptr, dst, algo, coord, false));
}

std::unique_ptr<op> resize_add(const std::unique_ptr<memory> &src, const std::unique_ptr<memory> &lateral,
                               std::unique_ptr<memory> &dst, resize_algo algo, resize_coord coord, bool post_relu) {
  return std::unique_ptr<op>(new op_resize(src, &lateral, dst, algo, coord, post_relu));
}

std::unique_ptr<op> inner_product(const std::unique_ptr<memory> &src, const std::unique_ptr<memory> &wei,
                                  const std::unique_ptr<memory> &bia, std::unique_ptr<memory> &dst, bool relu,
                                  std::vector<float> scales, round_mode rm) {
  return std::unique_ptr<op>(new op_inner_product(src, wei, bia, dst, relu, scales, rm));
}

std::unique_ptr<op> squeeze_excite(const std::unique_ptr<memory> &src, const std::unique_ptr<memory> &wei1,
                                   const std::unique_ptr<memory> &bia1, const std::unique_ptr<memory> &wei2,
                                   const std::unique_ptr<memory> &bia2, const std::array<u8, 256> &gate_table,
                                   std::unique_ptr<memory> &dst, std::vector<float> scales1, std::vector<float> scales2,
                                   std::vector<float> out_scales, round_mode rm) {
  return std::unique_ptr<op>(new op_squeeze_excite(src, &wei1, &bia1, &wei2, &bia2, &gate_table, dst, scales1, scales2, out_scales, rm));
}

std::unique_ptr<op> scaled_sum(const std::vector<std::unique_ptr<memory>> &srcs, const std::vector<std::vector<float>> &scales,
                               std::unique_ptr<memory> &dst, const std::vector<float> &bias, bool post_relu, const std::vector<u8> &table,
                               memory::dtype table_in, round_mode rm) {
  return std::unique_ptr<op>(new op_scaled_sum(srcs, scales, dst, bias, post_relu, table, table_in, rm));
}

std::unique_ptr<op> argmax(const std::unique_ptr<memory> &src, std::unique_ptr<memory> &dst_idx, int c_valid) {
  return std::unique_ptr<op>(new op_head(src, dst_idx, nullptr, DFX_HEAD_TOPK, 1, c_valid, nullptr, 0.f));
}

std::unique_ptr<op> top_k(const std::unique_ptr<memory> &src, std::unique_ptr<memory> &dst_idx, memory *dst_val, int k, int c_valid) {
  return std::unique_ptr<op>(new op_head(src, dst_idx, dst_val, DFX_HEAD_TOPK, k, c_valid, nullptr, 0.f));
}

std::unique_ptr<op> softmax(const std::unique_ptr<memory> &src, const std::array<uint32_t, 256> &table, std::unique_ptr<memory> &dst,
                            float out_scale, int c_valid) {
  return std::unique_ptr<op>(new op_head(src, dst, nullptr, DFX_HEAD_SOFTMAX, 0, c_valid, &table, out_scale));
}

std::unique_ptr<op> layer_norm(const std::unique_ptr<memory> &src, const std::vector<float> &gamma, const std::vector<float> &beta,
                               std::unique_ptr<memory> &dst, float eps, norm_mode mode, const std::vector<u8> &shifts, int c_valid) {
  return std::unique_ptr<op>(new op_layer_norm(src, gamma, beta, dst, eps, mode, shifts, c_valid));
}

std::unique_ptr<op> linear(const std::unique_ptr<memory> &src, const std::unique_ptr<memory> &wei, const std::unique_ptr<memory> &bia,
                           std::unique_ptr<memory> &dst, bool relu, std::vector<float> scales, round_mode rm, int k_valid,
                           const std::vector<u8> &table, memory::dtype table_in) {
  return std::unique_ptr<op>(new op_linear(src, wei, bia, dst, relu, scales, rm, k_valid, table, table_in));
}

std::unique_ptr<op> patch_embed(const std::unique_ptr<memory> &src, const std::unique_ptr<memory> &wei, const std::unique_ptr<memory> &bia,
                                std::unique_ptr<memory> &dst, bool relu, std::vector<float> scales, round_mode rm, const std::vector<float> &table,
                                int tok_offset, const std::vector<u8> &prefix) {
  return std::unique_ptr<op>(new op_patch_embed(src, wei, bia, dst, relu, scales, rm, table, tok_offset, prefix));
}

std::unique_ptr<op> window_partition(const std::unique_ptr<memory> &grid, std::unique_ptr<memory> &windows, window_shape shape,
                                     uint32_t pad_value, int c_valid) {
  return std::unique_ptr<op>(new op_window(DFX_WINDOW_PARTITION, grid.get(), windows.get(), shape, pad_value, c_valid));
}

std::unique_ptr<op> window_reverse(const std::unique_ptr<memory> &windows, std::unique_ptr<memory> &grid, window_shape shape, int c_valid) {
  return std::unique_ptr<op>(new op_window(DFX_WINDOW_REVERSE, grid.get(), windows.get(), shape, 0, c_valid));
}

std::array<long long, 3> attention_strides(int bs, int heads, int t, int d, long long ld) {
  if (ld == 0) ld = (long long)heads * d;
  if (bs < 1 || heads < 1 || t < 1 || d < 1 || ld < (long long)heads * d) error_and_exit("attention_strides: bad shape");
  return std::array<long long, 3>{{(long long)t * ld, (long long)d, ld}};
}

std::unique_ptr<op> matmul(const std::unique_ptr<memory> &a, const std::unique_ptr<memory> &b, std::unique_ptr<memory> &c,
                           const matmul_shape &shape, const std::vector<float> &scales, bool relu, round_mode rm) {
  return std::unique_ptr<op>(new op_matmul(a.get(), b.get(), c.get(), shape, scales, relu, rm));
}

std::unique_ptr<op> matmul(const std::unique_ptr<memory> &a, const std::unique_ptr<memory> &b, std::unique_ptr<memory> &c,
                           const matmul_shape &shape, const std::vector<float> &scales, const logit_bias &bias, bool relu, round_mode rm) {
  return std::unique_ptr<op>(new op_matmul(a.get(), b.get(), c.get(), shape, scales, relu, rm, &bias));
}

std::unique_ptr<op> attention(const std::unique_ptr<memory> &q, const std::unique_ptr<memory> &k, const std::unique_ptr<memory> &v,
                              const std::array<uint32_t, 256> &table, std::unique_ptr<memory> &o, const attention_shape &shape,
                              float logit_scale, const std::vector<float> &out_scales, float prob_scale, bool relu, round_mode rm) {
  return std::unique_ptr<op>(new op_attention(q.get(), k.get(), v.get(), table, o.get(), shape, logit_scale, out_scales, prob_scale, relu, rm));
}

std::unique_ptr<op> attention(const std::unique_ptr<memory> &q, const std::unique_ptr<memory> &k, const std::unique_ptr<memory> &v,
                              const std::array<uint32_t, 256> &table, std::unique_ptr<memory> &o, const attention_shape &shape,
                              float logit_scale, const std::vector<float> &out_scales, const logit_bias &bias, float prob_scale, bool relu,
                              round_mode rm) {
  return std::unique_ptr<op>(new op_attention(q.get(), k.get(), v.get(), table, o.get(), shape, logit_scale, out_scales, prob_scale, relu, rm, &bias));
}

std::unique_ptr<op> select_top_k(const std::unique_ptr<memory> &src, std::unique_ptr<memory> &dst_idx, memory *dst_val,
                                 std::unique_ptr<memory> &dst_count, int k, bool peak3, int min_val, int c_valid,
                                 const std::vector<memory *> &gather_src, const std::vector<memory *> &gather_dst) {
  return std::unique_ptr<op>(new op_select(src, dst_idx, dst_val, dst_count, k, peak3, min_val, c_valid, gather_src, gather_dst));
}

std::unique_ptr<op> box_nms(const std::unique_ptr<memory> &boxes, memory *idx, memory *count_in, std::unique_ptr<memory> &dst_keep,
                            std::unique_ptr<memory> &dst_count, memory *dst_boxes, float iou_thr, int classes) {
  return std::unique_ptr<op>(new op_nms(boxes.get(), idx, nullptr, nullptr, nullptr, nullptr, count_in, dst_keep.get(), dst_count.get(), dst_boxes,
                                        iou_thr, classes > 0 ? classes : 1, classes > 0, 1, 0.f, 0.f));
}

std::unique_ptr<op> box_nms(const std::unique_ptr<memory> &idx, const std::unique_ptr<memory> &deltas, const std::unique_ptr<memory> &anchors,
                            const std::array<float, 256> &tab_c, const std::array<float, 256> &tab_s, memory *count_in,
                            std::unique_ptr<memory> &dst_keep, std::unique_ptr<memory> &dst_count, memory *dst_boxes, float iou_thr,
                            int classes, bool per_class, int anchors_per_pixel, float clip_w, float clip_h) {
  return std::unique_ptr<op>(new op_nms(nullptr, idx.get(), deltas.get(), anchors.get(), &tab_c, &tab_s, count_in, dst_keep.get(), dst_count.get(),
                                        dst_boxes, iou_thr, classes, per_class, anchors_per_pixel, clip_w, clip_h));
}

std::unique_ptr<op> roi_align(const std::vector<memory *> &levels, const std::vector<float> &spatial_scales,
                              const std::vector<float> &level_area_thr, memory *boxes, memory *count, memory *batch_idx,
                              std::unique_ptr<memory> &dst, int sampling_ratio, bool aligned, int c_valid) {
  return std::unique_ptr<op>(new op_roialign(levels, spatial_scales, level_area_thr, boxes, count, batch_idx, dst.get(), sampling_ratio, aligned, c_valid));
}

std::unique_ptr<op> global_avg_pool(const std::unique_ptr<memory> &src, std::unique_ptr<memory> &dst) {
  return std::unique_ptr<op>(new op_squeeze_excite(src, nullptr, nullptr, nullptr, nullptr, nullptr, dst, {1.f}, {1.f}, {1.f},
                                                   round_mode::nearest));
}

std::unique_ptr<op> depthwise_separable_conv(const std::unique_ptr<memory> &src, const std::unique_ptr<memory> &wei_dw,
                                             const std::unique_ptr<memory> &bia_dw, std::array<int, 2> sz_stride,
                                             std::array<int, 2> sz_padding, const std::unique_ptr<memory> &wei_pw,
                                             const std::unique_ptr<memory> &bia_pw, std::unique_ptr<memory> &dst, bool relu,
                                             std::vector<float> scales_dw, std::vector<float> scales_pw, round_mode rm_dw,
                                             round_mode rm_pw) {
  return std::unique_ptr<op>(new op_depthwise_separable_conv(src, wei_dw, bia_dw, sz_stride, sz_padding, wei_pw, bia_pw, dst, relu,
                                                             scales_dw, scales_pw, rm_dw, rm_pw));
}

std::unique_ptr<op> concat_conv(const std::vector<std::unique_ptr<memory>> &srcs, const std::unique_ptr<memory> &wei,
                                const std::unique_ptr<memory> &bia, std::unique_ptr<memory> &dst, bool relu,
                                std::vector<float> scales, round_mode rm) {
  return std::unique_ptr<op>(new op_concat_conv(srcs, wei, bia, dst, relu, scales, rm));
}

std::unique_ptr<op> reorder(const std::unique_ptr<memory> &src, const std::unique_ptr<memory> &dst,
                            const std::vector<float> &scales, round_mode rm) {
  return std::unique_ptr<op>(new op_reorder(src, dst, scales, rm));
}

std::unique_ptr<op> conv_relu_pool(const std::unique_ptr<memory> &src, const std::unique_ptr<memory> &wei,
                                   const std::unique_ptr<memory> &bia, std::array<int, 2> conv_stride,
                                   std::array<int, 2> conv_padding, std::array<int, 2> pool_kernel,
                                   std::array<int, 2> pool_stride, std::array<int, 2> pool_padding,
                                   std::unique_ptr<memory> &dst, bool conv_relu, std::vector<float> conv_scales,
                                   round_mode conv_round_mode, pool_algo algo) {
  return std::unique_ptr<op>(new op_conv_pool(src, wei, bia, conv_stride, conv_padding, pool_kernel, pool_stride,
                                              pool_padding, dst, conv_relu, conv_scales, conv_round_mode, algo));
}

std::unique_ptr<op> eltwise_sum(const std::vector<std::unique_ptr<memory>> &srcs, std::unique_ptr<memory> &dst,
                                bool post_relu) {
  return std::unique_ptr<op>(new op_eltwise(srcs, dst, post_relu));
}

// ---------------------------------------------------------------------------
// factories (reference deepfusion.cc:105-185)
// ---------------------------------------------------------------------------

std::unique_ptr<op> concat(const std::vector<std::unique_ptr<memory>> &srcs,
                           std::unique_ptr<memory> &dst, bool post_relu) {
  return std::unique_ptr<op>(new op_concat(srcs, dst, post_relu));
}

std::unique_ptr<op> conv(const std::unique_ptr<memory> &src, const std::unique_ptr<memory> &wei,
                         const std::unique_ptr<memory> &bia, std::array<int, 2> sz_stride,
                         std::array<int, 2> sz_padding, const std::unique_ptr<memory> &wei1x1,
                         const std::unique_ptr<memory> &bia1x1, std::unique_ptr<memory> &dst,
                         bool conv0_relu, std::vector<float> conv0_scales, round_mode conv0_round_mode,
                         bool conv1_relu, std::vector<float> conv1_scales, round_mode conv1_round_mode) {
  return std::unique_ptr<op>(new op_conv(src, wei, bia, sz_stride, sz_padding, dst, conv0_scales,
                                         conv1_scales, wei1x1, bia1x1, conv0_relu, conv1_relu,
                                         conv0_round_mode, conv1_round_mode));
}

std::unique_ptr<op> conv(const std::unique_ptr<memory> &src, const std::unique_ptr<memory> &wei,
                         const std::unique_ptr<memory> &bia, std::array<int, 2> sz_stride,
                         std::array<int, 2> sz_padding, std::unique_ptr<memory> &dst, bool conv0_relu,
                         std::vector<float> conv0_scales, round_mode conv0_round_mode) {
  static const std::unique_ptr<memory> none;
  return conv(src, wei, bia, sz_stride, sz_padding, none, none, dst, conv0_relu, conv0_scales,
              conv0_round_mode);
}

void reorder_weights(const s8 *oihw, const std::unique_ptr<memory> &blocked) {
  if (!oihw || !blocked || blocked->data_type() != memory::dtype::s8 ||
      (blocked->dim_format() != memory::format::OIhw4i16o4i &&
       blocked->dim_format() != memory::format::gOIhw4i16o4i))
    error_and_exit("reorder_weights: destination must be an s8 OIhw4i16o4i memory");
  auto d = blocked->std_dims();
  check_dfx(dfx_reorder_oihw_to_blocked(oihw, static_cast<int8_t *>(blocked->data()), d[0], d[1], d[2],
                                        d[3]),
            "reorder");
}

}  // namespace deepfusion
