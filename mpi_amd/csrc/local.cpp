// local.cpp -- entry points of the local and verification kernels, the profile counters and the link probe.
#include <algorithm>
#include <cstring>
#include <mutex>

#include "comm.h"
#include "kernels.h"
#include "sched_steps.h"

using namespace xmpi;

static int timed_launch(xmpi_comm* c, int kind, size_t bytes, hipError_t (*launch)(void*, hipEvent_t, hipEvent_t),
                        void* ctx) {
  hipStream_t s = c->local_stream;
  if (!c->prof_on) {
    XMPI_HIP(launch(ctx, nullptr, nullptr));
    XMPI_HIP(hipStreamSynchronize(s));
    return XMPI_OK;
  }
  // the events ride on the dispatch itself: they carry the kernel's own begin / end timestamps
  hipEvent_t a = ev_get(c, true), b = ev_get(c, true);
  if (!a || !b) return XMPI_ERR_HIP;
  XMPI_HIP(launch(ctx, a, b));
  XMPI_HIP(hipStreamSynchronize(s));
  float ms = 0.f;
  XMPI_HIP(hipEventElapsedTime(&ms, a, b));
  c->prof[kind].add(ms, bytes);
  ev_put(c, a, true);
  ev_put(c, b, true);
  return XMPI_OK;
}

extern "C" {

int xmpi_reduce_local(xmpi_comm* c, void* dst, const void* a, const void* b, size_t count, xmpi_dtype dtype, xmpi_op op) {
  XMPI_ENTER(c);
  const size_t es = xmpi_dtype_size(dtype);
  if (!es || op < 0 || op >= XMPI_OP_COUNT) return XMPI_ERR_ARG;
  if (refuse_bitwise_on_float((int)dtype, (int)op)) return XMPI_ERR_ARG;
  if (op == XMPI_SUM_WIDE) op = XMPI_SUM;  // two operands: the same bits (include/xmpi.h)
  struct Ctx { xmpi_comm* c; void* dst; const void *a, *b; size_t n; int dt, op; } ctx{c, dst, a, b, count, (int)dtype, (int)op};
  return timed_launch(c, PROF_REDUCE2, 3 * count * es,
                      [](void* p, hipEvent_t es, hipEvent_t ee) {
                        Ctx* x = (Ctx*)p;
                        return launch_reduce2(x->dst, x->a, x->b, x->n, x->dt, x->op, x->c->local_stream, es, ee);
                      },
                      &ctx);
}

int xmpi_reduce_local_n(xmpi_comm* c, void* dst, const void* const* srcs, int nsrc, size_t count, xmpi_dtype dtype,
                        xmpi_op op) {
  XMPI_ENTER(c);
  const size_t es = xmpi_dtype_size(dtype);
  if (!es || op < 0 || op >= XMPI_OP_COUNT || nsrc < 1 || nsrc > kMaxReduceSrcs) return XMPI_ERR_ARG;
  if (refuse_bitwise_on_float((int)dtype, (int)op)) return XMPI_ERR_ARG;
  struct Ctx { xmpi_comm* c; void* dst; const void* const* s; int ns; size_t n; int dt, op; } ctx{c, dst, srcs, nsrc, count, (int)dtype, normal_op((int)dtype, (int)op)};
  return timed_launch(c, PROF_REDUCEN, (size_t)(nsrc + 1) * count * es,
                      [](void* p, hipEvent_t es, hipEvent_t ee) {
                        Ctx* x = (Ctx*)p;
                        return launch_reduce_n(x->dst, x->s, x->ns, x->n, x->dt, x->op, x->c->local_stream, es, ee);
                      },
                      &ctx);
}

int xmpi_copy_local(xmpi_comm* c, void* dst, const void* src, size_t bytes) {
  XMPI_ENTER(c);
  struct Ctx { xmpi_comm* c; void* dst; const void* src; size_t n; } ctx{c, dst, src, bytes};
  return timed_launch(c, PROF_COPY, 2 * bytes,
                      [](void* p, hipEvent_t es, hipEvent_t ee) {
                        Ctx* x = (Ctx*)p;
                        return launch_copy(x->dst, x->src, x->n, x->c->local_stream, es, ee);
                      },
                      &ctx);
}

int xmpi_reduce_local_multi(xmpi_comm* c, void* const* dsts, int ndst, const void* const* srcs, int nsrc, size_t count,
                            xmpi_dtype dtype, xmpi_op op) {
  XMPI_ENTER(c);
  const size_t es = xmpi_dtype_size(dtype);
  if (!es || op < 0 || op >= XMPI_OP_COUNT || nsrc < 1 || nsrc > kMaxReduceSrcs || ndst < 1 || ndst > kMaxReduceSrcs)
    return XMPI_ERR_ARG;
  if (refuse_bitwise_on_float((int)dtype, (int)op)) return XMPI_ERR_ARG;
  struct Ctx { xmpi_comm* c; void* const* d; int nd; const void* const* s; int ns; size_t n; int dt, op; }
      ctx{c, dsts, ndst, srcs, nsrc, count, (int)dtype, normal_op((int)dtype, (int)op)};
  return timed_launch(c, PROF_ZCOPY, (size_t)(nsrc + ndst) * count * es,
                      [](void* p, hipEvent_t es, hipEvent_t ee) {
                        Ctx* x = (Ctx*)p;
                        return launch_reduce_n_multi(x->d, x->nd, x->s, x->ns, x->n, x->dt, x->op, x->c->local_stream,
                                                     es, ee);
                      },
                      &ctx);
}

int xmpi_copy_local_pairs(xmpi_comm* c, void* const* dsts, const void* const* srcs, int n, size_t bytes) {
  XMPI_ENTER(c);
  if (n < 1 || n > kMaxReduceSrcs || !dsts || !srcs) return XMPI_ERR_ARG;
  struct Ctx { xmpi_comm* c; void* const* d; const void* const* s; int n; size_t bytes; } ctx{c, dsts, srcs, n, bytes};
  return timed_launch(c, PROF_ZCOPY, (size_t)(2 * n) * bytes,
                      [](void* p, hipEvent_t es, hipEvent_t ee) {
                        Ctx* x = (Ctx*)p;
                        return launch_copy_pairs(x->d, x->s, x->n, x->bytes, x->c->local_stream, es, ee);
                      },
                      &ctx);
}

int xmpi_copy_local_multi(xmpi_comm* c, void* const* dsts, int ndst, const void* src, size_t bytes) {
  XMPI_ENTER(c);
  if (ndst < 1 || ndst > kMaxReduceSrcs) return XMPI_ERR_ARG;
  struct Ctx { xmpi_comm* c; void* const* d; int nd; const void* src; size_t n; } ctx{c, dsts, ndst, src, bytes};
  return timed_launch(c, PROF_ZCOPY, (size_t)(1 + ndst) * bytes,
                      [](void* p, hipEvent_t es, hipEvent_t ee) {
                        Ctx* x = (Ctx*)p;
                        return launch_copy_multi(x->d, x->nd, x->src, x->n, x->c->local_stream, es, ee);
                      },
                      &ctx);
}

int xmpi_reduce_local_batch(xmpi_comm* c, void* const* dst, void* const* dst2, const void* const* a, const void* const* b,
                            const size_t* counts, int n, xmpi_dtype dtype, xmpi_op op) {
  XMPI_ENTER(c);
  const size_t es = xmpi_dtype_size(dtype);
  if (!es || op < 0 || op >= XMPI_OP_COUNT || n < 1 || n > kMaxBatch || !dst || !a || !b || !counts) return XMPI_ERR_ARG;
  if (refuse_bitwise_on_float((int)dtype, (int)op)) return XMPI_ERR_ARG;
  if (op == XMPI_SUM_WIDE) op = XMPI_SUM;  // two operands per segment: the same bits (include/xmpi.h)
  size_t total = 0;
  for (int i = 0; i < n; i++) {
    if (!a[i] || !b[i]) return XMPI_ERR_ARG;  // (dst[i] and dst2[i] may be null: kernels.h)
    total += counts[i];
  }
  struct Ctx { xmpi_comm* c; void* const* d; void* const* d2; const void* const* a; const void* const* b; const size_t* n; int segs, dt, op; }
      ctx{c, dst, dst2, a, b, counts, n, (int)dtype, (int)op};
  return timed_launch(c, PROF_REDUCE2, 3 * total * es,
                      [](void* p, hipEvent_t es, hipEvent_t ee) {
                        Ctx* x = (Ctx*)p;
                        return launch_reduce2_batch(x->d, x->d2, x->a, x->b, x->n, x->segs, x->dt, x->op, x->c->local_stream,
                                                    es, ee);
                      },
                      &ctx);
}

int xmpi_copy_local_batch(xmpi_comm* c, void* const* dst, void* const* dst2, const void* const* src, const size_t* bytes, int n) {
  XMPI_ENTER(c);
  if (n < 1 || n > kMaxBatch || !dst || !src || !bytes) return XMPI_ERR_ARG;
  size_t total = 0;
  for (int i = 0; i < n; i++) {
    if (!dst[i] || !src[i]) return XMPI_ERR_ARG;  // (only dst2[i] may be null: kernels.h)
    total += bytes[i];
  }
  struct Ctx { xmpi_comm* c; void* const* d; void* const* d2; const void* const* s; const size_t* n; int segs; } ctx{c, dst, dst2, src, bytes, n};
  return timed_launch(c, PROF_COPY, 2 * total,
                      [](void* p, hipEvent_t es, hipEvent_t ee) {
                        Ctx* x = (Ctx*)p;
                        return launch_copy_batch(x->d, x->d2, x->s, x->n, x->segs, x->c->local_stream, es, ee);
                      },
                      &ctx);
}

int xmpi_count_mismatch(xmpi_comm* c, const void* a, const void* b, size_t bytes, uint64_t* out) {
  XMPI_ENTER(c);
  if (!out) return XMPI_ERR_ARG;
  std::lock_guard<std::mutex> g(c->coll_mu);
  hipStream_t s = c->local_stream;
  XMPI_HIP(hipMemsetAsync(c->dev_words, 0, 32, s));
  XMPI_HIP(launch_count_mismatch(a, b, bytes, c->dev_words, s));
  XMPI_HIP(hipMemcpyAsync(out, c->dev_words, 8, hipMemcpyDeviceToHost, s));
  XMPI_HIP(hipStreamSynchronize(s));
  return XMPI_OK;
}

int xmpi_checksum(xmpi_comm* c, const void* buf, size_t bytes, uint64_t* out) {
  XMPI_ENTER(c);
  if (!out) return XMPI_ERR_ARG;
  std::lock_guard<std::mutex> g(c->coll_mu);
  hipStream_t s = c->local_stream;
  XMPI_HIP(hipMemsetAsync(c->dev_words, 0, 32, s));
  XMPI_HIP(launch_checksum(buf, bytes, c->dev_words, s));
  XMPI_HIP(hipMemcpyAsync(out, c->dev_words, 8, hipMemcpyDeviceToHost, s));
  XMPI_HIP(hipStreamSynchronize(s));
  return XMPI_OK;
}

int xmpi_diff_stats(xmpi_comm* c, const void* a, const void* b, size_t count, xmpi_dtype dtype, double stats[3]) {
  XMPI_ENTER(c);
  if (!stats) return XMPI_ERR_ARG;
  if (dtype != XMPI_F16 && dtype != XMPI_BF16 && dtype != XMPI_F32 && dtype != XMPI_F64 && !dtype_is_f8(dtype)) return XMPI_ERR_ARG;
  std::lock_guard<std::mutex> g(c->coll_mu);
  hipStream_t s = c->local_stream;
  uint64_t w[4] = {0, 0, 0, 0};
  XMPI_HIP(hipMemsetAsync(c->dev_words, 0, 32, s));
  XMPI_HIP(launch_diff_stats(a, b, count, (int)dtype, c->dev_words, s));
  XMPI_HIP(hipMemcpyAsync(w, c->dev_words, 24, hipMemcpyDeviceToHost, s));
  XMPI_HIP(hipStreamSynchronize(s));
  memcpy(&stats[0], &w[0], 8);
  memcpy(&stats[1], &w[1], 8);
  stats[2] = (double)w[2];
  return XMPI_OK;
}

int xmpi_diff_rel(xmpi_comm* c, const void* a, const void* b, size_t count, xmpi_dtype dtype, double* max_rel) {
  XMPI_ENTER(c);
  if (!max_rel) return XMPI_ERR_ARG;
  if (dtype != XMPI_F16 && dtype != XMPI_BF16 && dtype != XMPI_F32 && dtype != XMPI_F64 && !dtype_is_f8(dtype)) return XMPI_ERR_ARG;
  std::lock_guard<std::mutex> g(c->coll_mu);
  hipStream_t s = c->local_stream;
  uint64_t w[4] = {0, 0, 0, 0};
  XMPI_HIP(hipMemsetAsync(c->dev_words, 0, 32, s));
  XMPI_HIP(launch_diff_stats(a, b, count, (int)dtype, c->dev_words, s));
  XMPI_HIP(hipMemcpyAsync(w, c->dev_words, 32, hipMemcpyDeviceToHost, s));
  XMPI_HIP(hipStreamSynchronize(s));
  memcpy(max_rel, &w[3], 8);
  if (w[2]) *max_rel = 1.0 / 0.0;  // a NaN on one side only
  return XMPI_OK;
}

int xmpi_fill_pattern(xmpi_comm* c, void* buf, size_t count, xmpi_dtype dtype, int pattern, uint64_t seed) {
  XMPI_ENTER(c);
  if (!xmpi_dtype_size(dtype) || pattern < 0 || pattern > 3) return XMPI_ERR_ARG;
  XMPI_HIP(launch_fill(buf, count, (int)dtype, pattern, seed, c->local_stream));
  XMPI_HIP(hipStreamSynchronize(c->local_stream));
  return XMPI_OK;
}

int xmpi_prof_enable(xmpi_comm* c, int on) {
  if (!c || c->finalized) return XMPI_ERR_STATE;
  std::lock_guard<std::mutex> g(c->coll_mu);
  c->prof_on = on != 0;
  return XMPI_OK;
}

int xmpi_prof_reset(xmpi_comm* c) {
  if (!c || c->finalized) return XMPI_ERR_STATE;
  std::lock_guard<std::mutex> g(c->coll_mu);
  for (auto& p : c->prof) p = ProfCounter();
  return XMPI_OK;
}

int xmpi_prof_get(xmpi_comm* c, int kind, uint64_t* launches, double* total_ms, uint64_t* bytes) {
  if (!c || c->finalized) return XMPI_ERR_STATE;
  if (kind < 0 || kind >= PROF_KINDS) return XMPI_ERR_ARG;
  std::lock_guard<std::mutex> g(c->coll_mu);
  if (kind == PROF_ZCOPY && !c->dsync_prof_pending.empty()) {  // launches whose events nobody has read yet
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->local_stream);
    dsync_prof_harvest(c);
  }
  if (launches) *launches = c->prof[kind].launches;
  if (total_ms) *total_ms = c->prof[kind].total_ms;
  if (bytes) *bytes = c->prof[kind].bytes;
  return XMPI_OK;
}

int xmpi_link_probe(xmpi_comm* c, int peer, size_t bytes, int engine, int iters, int direction, double* gbps) {
  XMPI_ENTER(c);
  if (peer < 0 || peer >= c->size || iters < 1 || !gbps) return XMPI_ERR_ARG;
  std::lock_guard<std::mutex> g(c->coll_mu);
  if (!c->windows_ok) {
    set_last_error("link probe: it copies between the HBM windows, which this job could not map (xmpi_degraded)");
    return XMPI_ERR_UNSUPPORTED;
  }
  {
    const int src = ensure_streams(c);
    if (src != XMPI_OK) return src;
  }
  // the FIFO slots this rank owns in the peer's window (idle between collectives) are the remote
  // end; the slots the peer owns in this rank's window are the local end
  const size_t span = (size_t)c->lanes * c->fifo_depth * c->slot_bytes;
  bytes = std::min(bytes, span);
  char* remote = c->peer_window[peer] + c->coll_slot_off(c->rank, 0, 0);
  char* local = c->window + c->coll_slot_off(peer, 0, 0);
  char* dst = direction == 0 ? remote : local;  // 0 = write to the peer, 1 = read from the peer
  char* src = direction == 0 ? local : remote;
  hipStream_t s = c->send_stream[peer] ? c->send_stream[peer] : c->local_stream;
  hipEvent_t a = ev_get(c, true), b = ev_get(c, true);
  if (!a || !b) return XMPI_ERR_HIP;
  // engine 2: the stepped kernels' own accesses -- system-scope loads, written-through stores -- with as many workers as they run
  const int sys_grid = (int)std::max<long>(1, std::min<long>((long)((bytes + kSchedTileBytes - 1) / kSchedTileBytes), 1024 / std::max(1, c->dsync_sharers)));
  auto once = [&]() -> hipError_t {
    if (engine == 2) return launch_sys_copy(dst, src, bytes, sys_grid, s);
    if (engine == 1) return launch_copy(dst, src, bytes, s);
    return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s);
  };
  for (int w = 0; w < 2; w++) XMPI_HIP(once());
  XMPI_HIP(hipStreamSynchronize(s));
  XMPI_HIP(hipEventRecord(a, s));
  for (int i = 0; i < iters; i++) XMPI_HIP(once());
  XMPI_HIP(hipEventRecord(b, s));
  XMPI_HIP(hipStreamSynchronize(s));
  float ms = 0.f;
  XMPI_HIP(hipEventElapsedTime(&ms, a, b));
  ev_put(c, a, true);
  ev_put(c, b, true);
  *gbps = ms > 0 ? (double)bytes * iters / (ms * 1e-3) / 1e9 : 0.0;
  if (bytes >= ((size_t)1 << 20)) c->link_gbps[peer] = std::max(c->link_gbps[peer], *gbps);  // (sizes the pull kernel's grid)
  return XMPI_OK;
}

}  // extern "C"
