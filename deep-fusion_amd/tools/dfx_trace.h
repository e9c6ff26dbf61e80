// dfx_trace.h -- what dfx_trace_stub.cc records, for coherence_check.cc.  The stub is a host-only stand-in for
// libdfx_hip.so: it runs no arithmetic and only writes down, in call order, every entry point of include/dfx.h: those
// that touch memory or order streams with what they touch, the others as a NOTE.  One host thread makes all the calls, so call order is the host's program order.
#pragma once
#include <cstddef>
#include <string>
#include <vector>

namespace dfx_trace {

enum kind {
  ACCESS = 0,      // work enqueued on `stream` (a copy or a *_submit): asynchronous to the host
  HOST,            // the host thread itself reads or writes (set_weights, and the checker's own marks)
  SYNC,            // dfx_stream_sync(stream): the host waits for the stream
  WAIT,            // dfx_stream_wait_stream(stream, other): later work on `stream` waits for what `other` holds now
  STREAM_DESTROY,  // dfx_stream_destroy(stream): no later record may name it
  NOTE,            // any other entry point (set_device, create / destroy of a handle, alloc / free, stream create, events):
                   // `name` is the whole line -- entry point, then the device ordinal, "#<allocation id>" (a handle is the id
                   // of its packed copy), the byte count, "sid <n>" (the n-th stream created; 0 the default stream: not the
                   // checker's clock number) or "event <n>".  No stream, no ranges: it orders nothing and is only printed.
};

struct range {
  int buf;  // allocation id: unique for the process, never reused (an address may be)
  size_t off, len;
  bool write;
};

struct record {
  kind k;
  const void *stream, *other;
  std::string name;  // entry point, e.g. "dfx_gconv_submit"; host marks carry the caller's text
  std::vector<range> ranges;
};

const std::vector<record> &records();
// a host-thread access of [p, p + len) that no dfx_* call sees: a fill through memory::data(), a read of results
void host_access(const char *name, const void *p, size_t len, bool write);
// text of problems the stub itself saw (a destroyed stream used again, a range outside every live allocation)
const std::vector<std::string> &stub_errors();
// "host#3+0" / "device#7+128": kind of allocation, its id, the offset
std::string describe(const range &r);
// id of the live allocation that holds p, -1 if none (to give tensors names in reports)
int buffer_of(const void *p);

}  // namespace dfx_trace
