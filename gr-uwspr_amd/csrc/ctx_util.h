// ctx_util.h -- what the host sides of the kernels share (K7..K10, K13, K14, uwspr_api.hip): the context's error message,
// the checked HIP call, the device preamble, the pointer check of the UWSPR_DEVICE doors, the grown scratch buffer, the
// timing hook of the uwspr_debug_*_time entry points, the upload of scattered item offsets and the batch door of the
// kernels that take [n][162] soft symbols.  Host code only; one copy each.
//
// Not here, on purpose: K8's sub_grow and K7's tx_grow (other minimum, no synchronisation: their callers synchronise
// first), and K11 / K12's rs_fail / bk_fail / bk_grow (another signature: the stream ring reaches them without a context).
#pragma once

#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include "uwspr_internal.h"

#pragma GCC visibility push(hidden)   // the library exports its C ABI, not these
namespace uwspr {

// the context's message (uwspr_last_error) and the status to return
inline int ctx_fail(uwspr_ctx *c, int status, const char *fmt, ...) {
  if (c) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(c->err, sizeof(c->err), fmt, ap);
    va_end(ap);
  }
  return status;
}

#define CTXCHK(c, call)                                                                                 \
  do {                                                                                                  \
    hipError_t e_ = (call);                                                                             \
    if (e_ != hipSuccess)                                                                               \
      return uwspr::ctx_fail((c), UWSPR_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)

// a context whose creation found no device refuses; else its device becomes the calling thread's
inline int ctx_device_ready(uwspr_ctx *c) {
  if (!c->own_stream) return ctx_fail(c, UWSPR_ERR_NODEVICE, "context has no device (creation failed: %s)", c->err);
  CTXCHK(c, hipSetDevice(c->device));
  return UWSPR_OK;
}

// The context's device and [p, p + bytes) inside one device allocation of it: what a kernel may touch with XNACK off.
// Pageable host memory, another device's memory and ranges past an allocation's end are refused here, before any launch.
inline bool ctx_device_range(uwspr_ctx *c, const void *p, size_t bytes) {
  hipPointerAttribute_t a;
  memset(&a, 0, sizeof(a));
  const hipError_t e = hipPointerGetAttributes(&a, p);
  (void)hipGetLastError();   // a refused query leaves no error behind for the calls that follow
  if (e != hipSuccess || a.type != hipMemoryTypeDevice || a.device != c->device) return false;
  hipDeviceptr_t base = nullptr;
  size_t size = 0;
  if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) != hipSuccess) { (void)hipGetLastError(); return false; }
  const char *b = (const char *)base, *q = (const char *)p;
  return q >= b && bytes <= size && (size_t)(q - b) <= size - bytes;
}

// scratch of the context for `elems` elements, at least 256, never shrunk
template <typename T>
inline int ctx_grow(uwspr_ctx *c, T **buf, size_t *cap, size_t elems) {
  if (elems <= *cap && *buf) return UWSPR_OK;
  CTXCHK(c, hipStreamSynchronize(c->stream));   // the old buffer may still be read by the call before
  if (*buf) { CTXCHK(c, hipFree(*buf)); *buf = nullptr; *cap = 0; }
  const size_t n = elems > 256 ? elems : 256;
  const hipError_t e = hipMalloc((void **)buf, n * sizeof(T));
  if (e != hipSuccess) { (void)hipGetLastError(); return ctx_fail(c, UWSPR_ERR_NOMEM, "hipMalloc(%zu bytes): %s", n * sizeof(T), hipGetErrorString(e)); }
  *cap = n;
  return UWSPR_OK;
}

// The measurement hook behind uwspr_debug_{osd,blockdemod,deep,calls}_time (the probes under tools/): HIP events around
// the launches of a call while `timing` is on.
struct launch_timer {
  hipEvent_t ev[2] = {nullptr, nullptr};
  bool timing = false, timed = false;
  int begin(uwspr_ctx *c) {
    if (!timing) return UWSPR_OK;
    for (hipEvent_t &e : ev) if (!e) CTXCHK(c, hipEventCreate(&e));
    CTXCHK(c, hipEventRecord(ev[0], c->stream));
    return UWSPR_OK;
  }
  int end(uwspr_ctx *c) {
    if (!timing) return UWSPR_OK;
    CTXCHK(c, hipEventRecord(ev[1], c->stream));
    timed = true;
    return UWSPR_OK;
  }
  void release() {
    for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
  }
  // enable = 1 / 0 switches the events of the calls that follow on / off (< 0: unchanged); with ms given, waits for the last
  // timed call's launches and returns their time (0 when none was timed)
  int read(uwspr_ctx *c, int enable, double *ms) {
    if (enable >= 0) timing = enable != 0;
    if (ms) {
      *ms = 0.0;
      if (timed) {
        float f = 0.0f;
        CTXCHK(c, hipEventSynchronize(ev[1]));
        CTXCHK(c, hipEventElapsedTime(&f, ev[0], ev[1]));
        *ms = f;
      }
    }
    return UWSPR_OK;
  }
};

// The byte offsets of n scattered items (K9, K13, K14: item i = the 162 symbols at base + off[i]) into the context's
// buffer.  off is the caller's host memory, so the call waits for the copy -- for the whole stream.  K10 deliberately does
// not (page-locked items and an event of its own, k10_blockdemod.hip): an open item of DESIGN.md.
inline int scattered_offsets(uwspr_ctx *c, unsigned long long **d_off, size_t *cap_off, const unsigned long long *off, int n) {
  if (const int rc = ctx_grow(c, d_off, cap_off, (size_t)n)) return rc;
  CTXCHK(c, hipMemcpyAsync(*d_off, off, (size_t)n * sizeof(unsigned long long), hipMemcpyHostToDevice, c->stream));
  CTXCHK(c, hipStreamSynchronize(c->stream));
  return UWSPR_OK;
}

// The door of uwspr_osd_batch, uwspr_deep_batch and uwspr_calls_batch: n items of 162 soft symbols, n results of type R,
// both in host memory or both in memory of the context's device.  `refusal` is the entry point's own precondition, already
// evaluated (null: it holds).  begin(&stage) makes the kernel's state and hands out its staging buffer for host symbols;
// run(d_symbols, d_res, &d_res_out) launches on the context's stream, into d_res or -- d_res null -- into a buffer of the
// context handed back through d_res_out.
struct symbols_stage { uint8_t *d_sym = nullptr; size_t cap_sym = 0; };
template <typename R, typename Begin, typename Run>
inline int symbols_batch(uwspr_ctx *c, const char *name, const uint8_t *symbols, int n, int where, R *res, const char *refusal,
                         Begin begin, Run run) {
  if (n < 0 || (n > 0 && (!symbols || !res)) || (where != UWSPR_HOST && where != UWSPR_DEVICE))
    return ctx_fail(c, UWSPR_ERR_ARG, "%s: symbols %p, n %d, where %d, res %p", name, (const void *)symbols, n, where, (void *)res);
  if (refusal) return ctx_fail(c, UWSPR_ERR_ARG, "%s: %s", name, refusal);
  if (n == 0) return UWSPR_OK;
  int rc = ctx_device_ready(c);
  if (rc) return rc;
  const size_t nsym = (size_t)n * UWSPR_NSYM, nres = (size_t)n * sizeof(R);
  if (where == UWSPR_DEVICE) {
    if (!ctx_device_range(c, symbols, nsym) || !ctx_device_range(c, res, nres))
      return ctx_fail(c, UWSPR_ERR_ARG, "%s: UWSPR_DEVICE needs symbols (%zu bytes) and res (%zu bytes) inside device allocations of device %d",
                      name, nsym, nres, c->device);
    return run(symbols, res, (R **)nullptr);
  }
  symbols_stage *st = nullptr;
  if ((rc = begin(&st))) return rc;
  if ((rc = ctx_grow(c, &st->d_sym, &st->cap_sym, nsym))) return rc;
  CTXCHK(c, hipMemcpyAsync(st->d_sym, symbols, nsym, hipMemcpyHostToDevice, c->stream));
  R *d_res = nullptr;
  if ((rc = run(st->d_sym, (R *)nullptr, &d_res))) return rc;
  CTXCHK(c, hipMemcpyAsync(res, d_res, nres, hipMemcpyDeviceToHost, c->stream));
  CTXCHK(c, hipStreamSynchronize(c->stream));
  return UWSPR_OK;
}

}  // namespace uwspr
#pragma GCC visibility pop
