// The context: a device, a stream, the illegal-apply counter and the grow-only buffers that the entry points reuse
// from call to call (staging scratch, MCTS node pool, log table, work queue).  File map: osg_batch_internal.h.
#include <memory>

#include "osg_batch_internal.h"

namespace osg {

int check_illegal(osg_ctx* ctx, int64_t* h_illegal) {
  unsigned long long count = 0;
  OSG_HIP(hipMemcpyAsync(&count, ctx->d_illegal, sizeof(count), hipMemcpyDeviceToHost, ctx->stream));
  OSG_HIP(hipStreamSynchronize(ctx->stream));
  if (count) OSG_HIP(hipMemsetAsync(ctx->d_illegal, 0, sizeof(count), ctx->stream));
  if (h_illegal) { *h_illegal = static_cast<int64_t>(count); return OSG_OK; }
  if (count) return set_error(OSG_ERR_ILLEGAL, std::to_string(count) + " illegal action(s) applied (or out-of-range gather indices)");
  return OSG_OK;
}

template <class T>
hipError_t ctx_grow(osg_ctx* ctx, DeviceArray<T>& buf, size_t n) {
  if (n <= buf.size()) return hipSuccess;
  // Grow-only; make sure no queued kernel still reads the old block.
  if (const hipError_t e = hipStreamSynchronize(ctx->stream); e != hipSuccess) return e;
  return buf.alloc(n);
}
template hipError_t ctx_grow(osg_ctx*, DeviceArray<unsigned char>&, size_t);  // d_scratch, d_mcts_pool, d_ismcts
template hipError_t ctx_grow(osg_ctx*, DeviceArray<double>&, size_t);         // d_mcts_logs
template hipError_t ctx_grow(osg_ctx*, DeviceArray<int32_t>&, size_t);        // d_mcts_queue

void ctx_retain(osg_ctx* ctx) { __atomic_add_fetch(&ctx->refs, 1, __ATOMIC_RELAXED); }
void ctx_release(osg_ctx* ctx) {
  if (__atomic_sub_fetch(&ctx->refs, 1, __ATOMIC_ACQ_REL) != 0) return;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  const hipStream_t owned = ctx->own_stream ? ctx->stream : nullptr;
  delete ctx;  // frees the buffers
  if (owned) (void)hipStreamDestroy(owned);
}

}  // namespace osg

int osg_ctx_scratch(osg_ctx* ctx, size_t bytes, void** out) {
  if (bytes > ctx->d_scratch.size()) OSG_HIP(ctx_grow(ctx, ctx->d_scratch, bytes + bytes / 2));
  *out = ctx->d_scratch.get();
  return OSG_OK;
}

// ---------------------------------------------------------------------------
// C-ABI
// ---------------------------------------------------------------------------
extern "C" {

int osg_ctx_create(int device, void* stream, int own_stream, osg_ctx** out) {
  if (!out) return set_error(OSG_ERR_INVALID, "null out");
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count == 0)
    return set_error(OSG_ERR_HIP, "no HIP device visible: the MI355X path has no CPU fallback");
  if (device < 0 || device >= count) return set_error(OSG_ERR_INVALID, "bad device index");
  OSG_HIP(hipSetDevice(device));
  // (released on every failed return below: the buffers, and the stream once it is the context's own)
  std::unique_ptr<osg_ctx, void (*)(osg_ctx*)> ctx(new osg_ctx, osg::ctx_release);
  ctx->device = device;
  if (!own_stream) {
    ctx->stream = static_cast<hipStream_t>(stream);
  } else {
    OSG_HIP(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
    ctx->own_stream = true;
  }
  // [0] illegal-apply counter, [1 ...] the partial counter slots of k_random_steps
  OSG_HIP(ctx->d_illegal.alloc(1 + 2 * kCounterSlots));
  OSG_HIP(hipMemsetAsync(ctx->d_illegal, 0, sizeof(unsigned long long) * (1 + 2 * kCounterSlots), ctx->stream));
  *out = ctx.release();
  return OSG_OK;
}

int osg_ctx_destroy(osg_ctx* ctx) {
  if (!ctx) return OSG_OK;
  if (ctx->closed) return set_error(OSG_ERR_INVALID, "osg_ctx_destroy: context already destroyed");
  ctx->closed = true;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  osg::ctx_release(ctx);
  return OSG_OK;
}

int osg_ctx_synchronize(osg_ctx* ctx) {
  OSG_HIP(hipStreamSynchronize(ctx->stream));
  return check_illegal(ctx, nullptr);
}
void* osg_ctx_stream(osg_ctx* ctx) { return ctx->stream; }

int osg_ctx_set_stream(osg_ctx* ctx, void* stream) {
  if (!ctx || ctx->closed) return set_error(OSG_ERR_INVALID, "osg_ctx_set_stream: bad context");
  if (ctx->own_stream) return set_error(OSG_ERR_INVALID, "osg_ctx_set_stream: the context owns its stream");
  ctx->stream = static_cast<hipStream_t>(stream);
  return OSG_OK;
}

int osg_ctx_trim(osg_ctx* ctx) {
  if (!ctx || ctx->closed) return set_error(OSG_ERR_INVALID, "osg_ctx_trim: bad context");
  OSG_HIP(hipSetDevice(ctx->device));
  OSG_HIP(hipStreamSynchronize(ctx->stream));
  ctx->d_mcts_pool.reset();
  ctx->d_scratch.reset();
  ctx->d_mcts_queue.reset();
  ctx->d_ismcts.reset();
  ctx->ismcts.n = 0;   // the trees of the last information-set search go with their workspace
  return OSG_OK;
}

}  // extern "C"
