// tex_downscale.hip — RGBA8 layers halved, quartered or eighthed on the device (uvol_downscale_rgba_batch_dev): the reduced-resolution
// texture targets of the player manifest (reference src/Interfaces.ts:41-73: every texture target carries its own `resolution`), and the
// building block of KTX2 mip levels (still refused, the filter exists).
//
// The filter is this project's own, exact in integers, so that the device and the NumPy restatement of tests/downscale_cases.py agree bit
// for bit (stock `basisu -mipmap` filters with a Kaiser window in linear light; nothing at hand pins its output).  Factor f in {2, 4, 8}:
// W x H becomes ceil(W / f) x ceil(H / f); output texel (X, Y) is computed in ONE step from the box B of the n input texels with
// f X <= x < min(f X + f, W), f Y <= y < min(f Y + f, H):
//   lin[v]  = floor(65535 L(v / 255) + 0.5), L = the sRGB decoding function, evaluated in double on the host, once;
//   alpha   : A = sum a, out.a = (2 A + n) / (2 n);
//   colour  : alpha-weighted in linear light (a transparent neighbour does not bleed into an opaque texel): N = sum lin[c] a, D = A - or, when
//             A == 0, N = sum lin[c], D = n -, m = (2 N + D) / (2 D) (2 N + D <= 2 139 078 720 at f = 8: uint32), out.c = the v with the smallest
//             |lin[v] - m|, the lower v at a tie.
// The inverse is a search over the table: v = the number of entries of mid[u] = lin[u] + lin[u + 1] (u = 0 .. 254, strictly increasing) that
// are < 2 m - an entry EQUAL to 2 m is the tie, which goes to the lower v.  The search starts from a bucket table instead of the middle:
// neighbouring mid[] differ by at least 38, so among the 16 values of m that share m >> 4 the count changes at most once, and
// v = base[m >> 4] + (mid[base[m >> 4]] < 2 m) with base[k] = the count for m = 16 k: two LDS reads in place of the eight dependent ones of a
// binary search, which took 1.6 of the 5.0 ms of the f = 2 kernel (profiles/r13_downscale.json).  The host checks the short form against the
// plain count for every m when it builds the tables.  lin, mid and base (6 KiB) live in LDS; at f = 8 lin is held once per LDS bank (k_downscale).
//
// Memory-bound: every input byte is read once, 1 / f^2 of them written.  One thread makes four neighbouring output texels of one output row
// from 4 f input texels of each of the f input rows: f 16-byte loads per row and one 16-byte store where the addresses allow it - a layer that
// starts 16-byte aligned with a width (for the loads) / an output width (for the store) that is a multiple of 4 -, 4-byte loads and stores
// otherwise: the layers of an ingest slot start at base + i W H 4, which for odd sizes is only 4-byte aligned, and the last thread of a row
// may hold fewer than four texels.  Every read is bounded by W and H, every write by ow and oh, on both paths.
#include "uvol_common.hpp"
#include <cmath>

#define DOWN_BLOCK 256

// one input texel into the sums of its output texel; lin = the table's copy of this lane (REP words per entry)
template <int REP>
__device__ __forceinline__ void down_acc(uint32_t p, const uint32_t *lin, uint32_t &A, uint32_t *Nw, uint32_t *Nu) {
  const uint32_t a = p >> 24, r = lin[(p & 255u) * REP], g = lin[((p >> 8) & 255u) * REP], b = lin[((p >> 16) & 255u) * REP];
  A += a;
  Nw[0] += r * a; Nw[1] += g * a; Nw[2] += b * a;
  Nu[0] += r; Nu[1] += g; Nu[2] += b;
}
// the v whose lin[v] is nearest to m <= 65535 (the lower one at a tie): how many of the 255 midpoint sums lie below 2 m (mid[255] = 0xffffffff)
__device__ __forceinline__ uint32_t down_inverse(uint32_t m, const uint32_t *mid, const uint8_t *base) {
  const uint32_t v = base[m >> 4];
  return v + (mid[v] < 2u * m ? 1u : 0u);
}

template <int F, int REP>
__global__ void __launch_bounds__(DOWN_BLOCK) k_downscale(const uint8_t *const *layers, uint8_t *out0, uint32_t W, uint32_t H, uint32_t ow, uint32_t oh,
                                                           uint32_t n_layers, const uint32_t *tables) {
  // REP = 32: lin[] once per LDS bank, word v * 32 + (lane & 31) - the three look-ups per input texel go to 64 unrelated entries per wave
  // instruction, and with one copy they took 1.8 of the 4.8 ms of the f = 8 kernel on noise (profiles/r13_downscale.json); a lane that stays
  // on its own bank cannot collide.  32 KiB of LDS per workgroup: four workgroups per CU.  REP = 1: the table once (the host picks per factor)
  __shared__ uint32_t s_lin[256 * REP], s_mid[256], s_base32[DOWN_BUCKETS / 4];
  for (uint32_t k = threadIdx.x; k < 256u * REP; k += DOWN_BLOCK) s_lin[k] = tables[k / REP];
  for (uint32_t k = threadIdx.x; k < 256u; k += DOWN_BLOCK) s_mid[k] = tables[256u + k];
  for (uint32_t k = threadIdx.x; k < DOWN_BUCKETS / 4; k += DOWN_BLOCK) s_base32[k] = tables[512u + k];
  __syncthreads();
  const uint8_t *s_base = reinterpret_cast<const uint8_t *>(s_base32);
  const uint32_t *my_lin = s_lin + (threadIdx.x & (uint32_t)(REP - 1));
  const uint32_t G = (ow + 3u) / 4u;                      // threads per output row
  const unsigned long long items = (unsigned long long)n_layers * oh * G, stride = (unsigned long long)gridDim.x * DOWN_BLOCK;
  const size_t obytes = (size_t)ow * oh * 4;
  for (unsigned long long it = (unsigned long long)blockIdx.x * DOWN_BLOCK + threadIdx.x; it < items; it += stride) {
    const uint32_t gx = (uint32_t)(it % G); const unsigned long long t = it / G;
    const uint32_t Y = (uint32_t)(t % oh), li = (uint32_t)(t / oh);
    const uint8_t *src8 = layers[li]; uint8_t *dst8 = out0 + obytes * li;
    const uint32_t *src = reinterpret_cast<const uint32_t *>(src8); uint32_t *dst = reinterpret_cast<uint32_t *>(dst8);
    const uint32_t x0 = 4u * F * gx, X0 = 4u * gx, y0 = (uint32_t)F * Y;
    const uint32_t y1 = y0 + F < H ? y0 + F : H;            // rows [y0, y1) exist
    const bool wide_in = (((uintptr_t)src8 & 15) == 0) && (W & 3u) == 0 && x0 + 4u * F <= W;
    uint32_t A[4] = { 0, 0, 0, 0 }, Nw[4][3] = { { 0, 0, 0 }, { 0, 0, 0 }, { 0, 0, 0 }, { 0, 0, 0 } }, Nu[4][3] = { { 0, 0, 0 }, { 0, 0, 0 }, { 0, 0, 0 }, { 0, 0, 0 } };
    for (uint32_t y = y0; y < y1; y++) {
      const uint32_t *row = src + (size_t)y * W + x0;
      if (wide_in) {
        const uint4 *row4 = reinterpret_cast<const uint4 *>(row);
#pragma unroll
        for (int k = 0; k < F; k++) {
          const uint4 v = row4[k];
          down_acc<REP>(v.x, my_lin, A[(4 * k + 0) / F], Nw[(4 * k + 0) / F], Nu[(4 * k + 0) / F]);
          down_acc<REP>(v.y, my_lin, A[(4 * k + 1) / F], Nw[(4 * k + 1) / F], Nu[(4 * k + 1) / F]);
          down_acc<REP>(v.z, my_lin, A[(4 * k + 2) / F], Nw[(4 * k + 2) / F], Nu[(4 * k + 2) / F]);
          down_acc<REP>(v.w, my_lin, A[(4 * k + 3) / F], Nw[(4 * k + 3) / F], Nu[(4 * k + 3) / F]);
        }
      } else {
#pragma unroll
        for (int c = 0; c < 4 * F; c++) if (x0 + (uint32_t)c < W) down_acc<REP>(row[c], my_lin, A[c / F], Nw[c / F], Nu[c / F]);
      }
    }
    uint32_t o[4] = { 0, 0, 0, 0 };
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const uint32_t X = X0 + (uint32_t)j;
      if (X >= ow) continue;
      const uint32_t bx = (uint32_t)F * X, bw = bx + F < W ? (uint32_t)F : W - bx, n = bw * (y1 - y0);
      const uint32_t D = A[j] ? A[j] : n;
      uint32_t px = ((2u * A[j] + n) / (2u * n)) << 24;
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const uint32_t N = A[j] ? Nw[j][c] : Nu[j][c];
        px |= down_inverse((2u * N + D) / (2u * D), s_mid, s_base) << (8 * c);
      }
      o[j] = px;
    }
    uint32_t *orow = dst + (size_t)Y * ow + X0;
    if ((((uintptr_t)dst8 & 15) == 0) && (ow & 3u) == 0) *reinterpret_cast<uint4 *>(orow) = make_uint4(o[0], o[1], o[2], o[3]);      // (ow % 4 == 0: the group is whole)
    else {
#pragma unroll
      for (int j = 0; j < 4; j++) if (X0 + (uint32_t)j < ow) orow[j] = o[j];
    }
  }
}

// ================================================================================================
// host side
// ================================================================================================
struct DownState { uvol_devbuf out[2], in, ptrs, tables; bool tables_up = false; std::vector<const uint8_t *> hptrs; uint32_t htab[DOWN_TABLE_WORDS]; };
// lin[], mid[] and base[] (see the head of this file); lin is strictly increasing (smallest step 19) and no value lies closer than 0.0016 to
// a rounding boundary, so the libm in use cannot change an entry.  false: the bucket form of the search disagrees with the plain count for
// some m (it cannot, with this table: the check is what makes that a fact of the build at hand).  Shared with tex_mipchain.hip.
bool down_tables(uint32_t *t) {
  for (int v = 0; v < 256; v++) {
    const double s = v / 255.0, L = s <= 0.04045 ? s / 12.92 : std::pow((s + 0.055) / 1.055, 2.4);
    t[v] = (uint32_t)std::floor(65535.0 * L + 0.5);
  }
  uint32_t *mid = t + 256; uint8_t *base = reinterpret_cast<uint8_t *>(t + 512);
  for (int v = 0; v < 255; v++) mid[v] = t[v] + t[v + 1];
  mid[255] = 0xffffffffu;
  uint32_t c = 0;                                          // the plain count, which only grows with m
  for (uint32_t m = 0; m < 65536u; m++) {
    while (c < 255 && mid[c] < 2u * m) c++;
    if ((m & 15u) == 0) base[m >> 4] = (uint8_t)c;
    const uint32_t v = base[m >> 4];
    if (v + (mid[v] < 2u * m ? 1u : 0u) != c) return false;
  }
  return true;
}
void down_destroy(uvol_ctx *ctx) {
  DownState *S = ctx->down; if (!S) return;
  for (uvol_devbuf *b : { &S->out[0], &S->out[1], &S->in, &S->ptrs, &S->tables }) if (b->p) (void)hipFree(b->p);
  delete S; ctx->down = nullptr;
}
// uvol_trim: the slots (and the staging buffer of host inputs) go back to the device; the next call allocates what it needs
void down_trim(uvol_ctx *ctx) {
  DownState *S = ctx->down; if (!S) return;
  for (uvol_devbuf *b : { &S->out[0], &S->out[1], &S->in, &S->ptrs }) if (b->p) { (void)hipFree(b->p); b->p = nullptr; b->cap = 0; }
}
// n layers of w x h RGBA8 (device pointers, or host memory that is uploaded through the staging buffers) -> rgba_dev_out[i] = the layer
// downscaled by `factor` in the context's downscale slot `slot`.  One launch for the whole batch on the context's stream, behind the
// un-filter of any ingest slot the layers lie in; returns when the layers are complete.
int down_rgba_batch(uvol_ctx *ctx, const uint8_t *const *rgba, int n, uint32_t w, uint32_t h, bool inputs_on_device, int factor, int slot, const uint8_t **rgba_dev_out) {
  if (n <= 0) return UVOL_OK;
  if (factor != 2 && factor != 4 && factor != 8) { ctx->set_error("uvol_downscale_rgba_batch_dev: factor %d (2, 4 or 8)", factor); return UVOL_E_INVALID; }
  if (slot < 0 || slot > 1) { ctx->set_error("uvol_downscale_rgba_batch_dev: slot %d (0 or 1)", slot); return UVOL_E_INVALID; }
  if (!w || !h || w > 8192 || h > 16384) { ctx->set_error("uvol_downscale_rgba_batch_dev: width %u x height %u (1 x 1 up to 8192 x 16384)", w, h); return UVOL_E_INVALID; }
  for (int i = 0; i < n; i++) {
    if (!rgba[i]) { ctx->set_error("uvol_downscale_rgba_batch_dev: rgba[%d] is NULL", i); return UVOL_E_INVALID; }
    if (inputs_on_device && ((uintptr_t)rgba[i] & 3)) { ctx->set_error("uvol_downscale_rgba_batch_dev: rgba[%d] is a device layer that is not 4-byte aligned", i); return UVOL_E_INVALID; }
  }
  if (!ctx->down) ctx->down = new DownState();
  DownState *S = ctx->down;
  const uint32_t f = (uint32_t)factor, ow = (w + f - 1) / f, oh = (h + f - 1) / f;
  const size_t ibytes = (size_t)w * h * 4, obytes = (size_t)ow * oh * 4;
  int rc;
  if ((rc = uvol_ensure(ctx, S->out[slot], obytes * (size_t)n))) return rc;
  if ((rc = uvol_ensure(ctx, S->ptrs, sizeof(uint8_t *) * (size_t)n))) return rc;
  if ((rc = uvol_ensure(ctx, S->tables, sizeof S->htab))) return rc;
  if (!S->tables_up) {
    if (!down_tables(S->htab)) { ctx->set_error("uvol_downscale_rgba_batch_dev: the inverse table's bucket search disagrees with the plain search"); return UVOL_E_HIP; }
    UVOL_HIP_CHECK(ctx, hipMemcpyAsync(S->tables.p, S->htab, sizeof S->htab, hipMemcpyHostToDevice, ctx->stream));
    S->tables_up = true;
  }
  S->hptrs.assign(rgba, rgba + n);
  if (inputs_on_device) {
    if ((rc = png_order_before(ctx, ctx->stream, rgba, (size_t)n))) return rc;
  } else {
    if ((rc = uvol_ensure(ctx, S->in, ibytes * (size_t)n))) return rc;
    std::vector<UvolUpItem> ups; ups.reserve((size_t)n);
    for (int i = 0; i < n; i++) { ups.push_back(UvolUpItem{ ibytes * (size_t)i, rgba[i], ibytes }); S->hptrs[(size_t)i] = (const uint8_t *)S->in.p + ibytes * (size_t)i; }
    uvol_ctx::Scope sc(ctx, "ingest.downscale_upload", (uint64_t)ibytes * n);
    if ((rc = uvol_upload_staged(ctx, (uint8_t *)S->in.p, ups))) return rc;
  }
  UVOL_HIP_CHECK(ctx, hipMemcpyAsync(S->ptrs.p, S->hptrs.data(), sizeof(uint8_t *) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
  const unsigned long long items = (unsigned long long)n * oh * ((ow + 3) / 4);
  const unsigned blocks = (unsigned)std::min<unsigned long long>((items + DOWN_BLOCK - 1) / DOWN_BLOCK, 2048ull);      // grid-stride beyond 8 workgroups per CU
  { uvol_ctx::Scope sc(ctx, "ingest.downscale", (uint64_t)(ibytes + obytes) * n);
    if (uvol_debug()) { fprintf(stderr, "[uvol] launch k_downscale<%d> %d layers %u x %u\n", factor, n, w, h); fflush(stderr); }
    const uint8_t *const *lp = (const uint8_t *const *)S->ptrs.p; uint8_t *op = (uint8_t *)S->out[slot].p; const uint32_t *tp = (const uint32_t *)S->tables.p;
#define DOWN_LAUNCH(F_, R_) hipLaunchKernelGGL((k_downscale<F_, R_>), dim3(blocks), dim3(DOWN_BLOCK), 0, ctx->stream, lp, op, w, h, ow, oh, (uint32_t)n, tp)
    // copies of lin[] in LDS, chosen per factor by measurement (640 layers of 2048^2, noise; profiles/r13_downscale.json): one per bank at
    // f = 8 (3.2 ms against 6.2 with a single copy), a single one at f = 2 and 4 (3.7 against 3.9 ms, 2.3 against 2.45: there the 37 KiB per
    // workgroup cost more, in waves per CU, than the collisions)
    if (factor == 2) DOWN_LAUNCH(2, 1); else if (factor == 4) DOWN_LAUNCH(4, 1); else DOWN_LAUNCH(8, 32);
#undef DOWN_LAUNCH
  }
  UVOL_HIP_CHECK(ctx, hipGetLastError());
  for (int i = 0; i < n; i++) rgba_dev_out[i] = (const uint8_t *)S->out[slot].p + obytes * (size_t)i;
  UVOL_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return UVOL_OK;
}
