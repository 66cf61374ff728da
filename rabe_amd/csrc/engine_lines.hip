// engine_lines.hip -- a prepared-lines handle of fixed capacity that is filled and emptied by ranges of blocks (include/rabe_hip.h:
// rhip_g2_lines_reserve, _prepare_range, _scrub_range, _range_is_zero): what the GHW11 key store that adds and revokes keys in place
// stands on (host/packed.cpp: TkStore).  A block is one point's share of the handle's three flat arrays: 88 line triples of twelve
// 16-byte words, their reduced-radix records of nine, one flag.  The blocks of a range are adjacent in each array, so a range is one
// contiguous stream per array.
//
// Two kernels, both bandwidth-bound streams: every lane moves one 16-byte word per step, a wave one KiB, no LDS; the grid is capped and
// strides over the rest.  The preparation itself is engine.hip's k_g2_prepare_lines and engine_rr.hip's k_lines_to_rr, launched on the
// range's addresses (rhip_launch_g2_prepare_lines, rhip_lines_to_rr_into).
//
// A translation unit of its own, as engine_gtpow.hip is: the other units' instruction streams are what was measured.
#include "engine_internal.h"

#define RB_LINES_STREAM_BLOCK 256
#define RB_LINES_STREAM_MAX_BLOCKS 2048

// blocks back to empty: zero words over a[0 .. na) (line triples) and b[0 .. nb) (their reduced-radix records, nb = 0 where the handle has
// none), flag 1 (the point at infinity: a pair on the block contributes 1) over flags[0 .. nf).  Plain vector stores.
__global__ void __launch_bounds__(RB_LINES_STREAM_BLOCK) k_lines_scrub(uint4* a, size_t na, uint4* b, size_t nb, uint8_t* flags, size_t nf) {
  const size_t stride = (size_t)gridDim.x * blockDim.x, t0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint4 z = make_uint4(0u, 0u, 0u, 0u);
  for (size_t t = t0; t < na; t += stride) a[t] = z;
  for (size_t t = t0; t < nb; t += stride) b[t] = z;
  for (size_t t = t0; t < nf; t += stride) flags[t] = 1;
}
// *nonzero |= 1 when a word of a[0 .. na) or b[0 .. nb) is not zero or a flag of flags[0 .. nf) is not 1.  A lane ORs what it reads and
// reports once; *nonzero is zeroed by the caller in front of the launch.
__global__ void __launch_bounds__(RB_LINES_STREAM_BLOCK) k_lines_is_zero(const uint4* a, size_t na, const uint4* b, size_t nb, const uint8_t* flags, size_t nf,
                                                                         uint32_t* nonzero) {
  const size_t stride = (size_t)gridDim.x * blockDim.x, t0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t acc = 0;
  for (size_t t = t0; t < na; t += stride) { const uint4 v = a[t]; acc |= v.x | v.y | v.z | v.w; }
  for (size_t t = t0; t < nb; t += stride) { const uint4 v = b[t]; acc |= v.x | v.y | v.z | v.w; }
  for (size_t t = t0; t < nf; t += stride) acc |= (uint32_t)(flags[t] ^ 1u);
  if (acc) atomicOr(nonzero, 1u);
}

namespace {
struct Range { uint4* a; size_t na; uint4* b; size_t nb; uint8_t* flags; size_t nf; };
// the three streams of blocks [first, first + n); the caller has checked the range against the capacity
Range range_of(const rhip_g2_lines* p, size_t first, size_t n) {
  const size_t per = RB_MILLER_LINES;
  return Range{(uint4*)p->lines + first * per * RB_LINE_QUADS, n * per * RB_LINE_QUADS,
               p->lines29 ? (uint4*)p->lines29 + first * per * RB_LINE29_QUADS : nullptr, p->lines29 ? n * per * RB_LINE29_QUADS : 0, p->q_inf + first, n};
}
bool in_capacity(const rhip_g2_lines* p, size_t first, size_t n) { return first <= p->n && n <= p->n - first; }
unsigned stream_blocks(const Range& r) {
  const unsigned want = blocks_for(r.na > r.nb ? r.na : r.nb, RB_LINES_STREAM_BLOCK);
  return want < RB_LINES_STREAM_MAX_BLOCKS ? (want ? want : 1u) : RB_LINES_STREAM_MAX_BLOCKS;
}
int32_t launch_scrub(rhip_ctx* ctx, const Range& r) {
  KLAUNCH(ctx, "k_lines_scrub", k_lines_scrub, dim3(stream_blocks(r)), dim3(RB_LINES_STREAM_BLOCK), 0, ctx->stream, r.a, r.na, r.b, r.nb, r.flags, r.nf);
  return RHIP_OK;
}
}  // namespace
static_assert(sizeof(LineM) == RB_LINE_QUADS * sizeof(uint4), "a line triple is twelve 16-byte words");

extern "C" int32_t rhip_g2_lines_reserve(rhip_ctx* ctx, size_t capacity, rhip_g2_lines** out) {
  NEED(ctx);
  if (!out || !capacity) return RHIP_ERR_ARG;
  *out = nullptr;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  rhip_g2_lines* p = new rhip_g2_lines{ctx, capacity, nullptr, nullptr};
  // the allocations of rhip_g2_lines_prepare over `capacity` points (rhip_g2_lines_bytes reports the same size for both)
  hipError_t e = hipMalloc((void**)&p->lines, capacity * RB_MILLER_LINES * sizeof(LineM));
  if (e == hipSuccess) e = hipMalloc((void**)&p->q_inf, capacity);
  if (e == hipSuccess && rhip_want_lines29(ctx)) e = hipMalloc(&p->lines29, capacity * RB_MILLER_LINES * RB_LINE29_QUADS * sizeof(uint4));
  if (e != hipSuccess) { rhip_g2_lines_destroy(p); return fail(ctx, e, "rhip_g2_lines_reserve: hipMalloc"); }
  int32_t rc = launch_scrub(ctx, range_of(p, 0, capacity));
  if (rc == RHIP_OK) {
    const hipError_t es = hipStreamSynchronize(ctx->stream);
    if (es != hipSuccess) rc = fail(ctx, es, "rhip_g2_lines_reserve: sync");
  }
  if (rc) { rhip_g2_lines_destroy(p); return rc; }
  *out = p;
  return RHIP_OK;
}
extern "C" int32_t rhip_g2_lines_scrub_range(rhip_ctx* ctx, rhip_g2_lines* lines, size_t first, size_t n) {
  NEED(ctx);
  if (!lines || !in_capacity(lines, first, n)) return RHIP_ERR_ARG;
  if (!n) return RHIP_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const int32_t rc = launch_scrub(ctx, range_of(lines, first, n));
  if (rc) return rc;
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return RHIP_OK;
}
extern "C" int32_t rhip_g2_lines_prepare_range(rhip_ctx* ctx, rhip_g2_lines* lines, size_t first, size_t n, const rhip_g2* dev_q) {
  NEED(ctx);
  if (!lines || !in_capacity(lines, first, n) || (n && !dev_q)) return RHIP_ERR_ARG;
  if (!n) return RHIP_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const Range r = range_of(lines, first, n);
  // k_g2_prepare_lines writes no line of a point at infinity: the range is emptied first, so that such a block is empty whatever it held
  int32_t rc = launch_scrub(ctx, r);
  if (rc == RHIP_OK) rc = rhip_launch_g2_prepare_lines(ctx, n, dev_q, r.a, r.flags);
  if (rc == RHIP_OK && r.b) rc = rhip_lines_to_rr_into(ctx, n * RB_MILLER_LINES, r.a, r.b);
  if (rc) return rc;
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));          // the handle is read from any context afterwards
  return RHIP_OK;
}
extern "C" int32_t rhip_g2_lines_range_is_zero(rhip_ctx* ctx, const rhip_g2_lines* lines, size_t first, size_t n, int32_t* out_zero) {
  NEED(ctx);
  if (!lines || !out_zero || !in_capacity(lines, first, n)) return RHIP_ERR_ARG;
  *out_zero = 1;
  if (!n) return RHIP_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const int32_t rc = ensure_scratch(ctx, sizeof(uint32_t));
  if (rc) return rc;
  uint32_t* d_flag = (uint32_t*)ctx->scratch;
  HIP_TRY(ctx, hipMemsetAsync(d_flag, 0, sizeof(uint32_t), ctx->stream));
  const Range r = range_of(lines, first, n);
  KLAUNCH(ctx, "k_lines_is_zero", k_lines_is_zero, dim3(stream_blocks(r)), dim3(RB_LINES_STREAM_BLOCK), 0, ctx->stream, (const uint4*)r.a, r.na, (const uint4*)r.b, r.nb,
          (const uint8_t*)r.flags, r.nf, d_flag);
  uint32_t nonzero = 1;
  HIP_TRY(ctx, hipMemcpyAsync(&nonzero, d_flag, sizeof nonzero, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  *out_zero = nonzero ? 0 : 1;
  return RHIP_OK;
}
