// tex_etc2.hip — RGBA8 layers encoded to full ETC1 blocks on the device (uvol_encode_etc2_rgb_batch): the raw `etc2` texture target of the
// player manifest (reference src/Interfaces.ts:19, src/V2/player.ts:338-356 uploads it as RGB_ETC2_Format) made from the SOURCE texels with a
// search, instead of re-packing the ETC1S segments (k_tdec_etc1, tex_decode.hip), whose blocks have one base colour and one table for both
// halves and are snapped to the segment's codebooks although the raw file pays 8 bytes per block whatever is in them.
//
// The rule is this project's own, exact in integers; include/uvol_codec.h states it (the normative text) and tests/etc2_direct_cases.py
// restates it in NumPy, bit for bit.  In short, per 4x4 block (texels fetched as t_load_block does: y_flip, replicated edges, px[4 y + x],
// alpha ignored): for flip 0 (left | right) and flip 1 (top | bottom) each half is searched around its mean colour in 4 bits (individual
// mode) and in 5 bits (differential mode) - step 1: the 8 tables x the base moved by (0, -1, +1) on all channels, step 2: one channel at a
// time by -1 / +1 at the best table -; the differential pair is the refined one when its deltas fit -4 .. 3, else the unrefined q5 pair with
// its best tables when THOSE fit, else there is none; differential wins with E_diff <= E_ind, flip 1 only with a strictly smaller error.
// The second base of a differential block is a 5-bit value by construction, so no block is one of ETC2's T, H or planar modes - which stay
// out of scope: their bit layouts are in nothing at hand, and this project does not restate formats from memory.
//
// Compute-bound: a block costs 2 flips x 2 halves x 2 precisions x (24 + up to 6) evaluations of E over 8 texels, against 64 bytes read and
// 8 written.  E uses the closed form of t_eval_block where no modified colour clamps (the same integers), the per-channel form otherwise.
// Four lanes per block: lane k of a quad searches half k & 1 of flip k >> 1 in both precisions, the halves of a flip meet over
// __shfl_xor(., 1), the flips over __shfl_xor(., 2), every lane then makes the selectors of row k and lane 0 stores the block.  Measured at
// 640 layers of 2048^2 against one lane per block (everything in one lane, as k_tex_fit does it): 319.5 against 351.9 ms per launch, the same
// bytes (profiles/r14_etc2_direct.json); the one-lane form was dropped.
// A fit travels as one 64-bit word: error << 32 | table << 15 | r << 10 | g << 5 | b (errors are at most 16 x 3 x 255^2 < 2^22).
// Every read is bounded by W and H (clamped coordinates), every write by the block count of the layer.
// The ETC1 tables, expansions, pixel-index order, planes and the block's byte layout are those of tex_blocks.hpp.
#include "uvol_common.hpp"
#include "tex_device.hpp"

#define E2_BLOCK 256
#ifdef HIPEMU
#define E2_MAX_GRID 4u                                   /* the emulation build strides after 256 blocks: every test of it runs the loop's later rounds */
#else
#define E2_MAX_GRID 32768u                               /* workgroups; the kernel strides beyond (2 097 152 blocks per round) */
#endif

template <int TOP> __device__ __forceinline__ int e2_expand(int b) { return TOP == 31 ? t_expand5(b) : t_expand4(b); }
__device__ __forceinline__ uint32_t e2_err(unsigned long long w) { return (uint32_t)(w >> 32); }
__device__ __forceinline__ unsigned long long e2_word(uint32_t err, uint32_t code) { return ((unsigned long long)err << 32) | code; }

// 4x4 block fetch of layer `img`: what t_load_block does for colour slices (y_flip, edges replicated, px[4 y + x] = R | G << 8 | B << 16);
// the 16-byte path also asks the layer itself to be 16-byte aligned (device layers of this entry point are 4-byte aligned only)
__device__ inline void e2_load_block(const uint8_t *img, uint32_t W, uint32_t H, int yflip, uint32_t X, uint32_t Y, uint32_t px[16]) {
  const bool wide = (W & 3u) == 0 && ((uintptr_t)img & 15) == 0;      // (then X * 4 + 3 < W for every block)
  for (int y = 0; y < 4; y++) {
    uint32_t py = Y * 4 + (uint32_t)y; if (py >= H) py = H - 1;
    const uint32_t sr = yflip ? H - 1 - py : py;
    const uint32_t *row = reinterpret_cast<const uint32_t *>(img) + (size_t)sr * W;
    if (wide) {
      const uint4 v = *reinterpret_cast<const uint4 *>(row + 4 * (size_t)X);
      px[4 * y + 0] = v.x & 0xffffffu; px[4 * y + 1] = v.y & 0xffffffu; px[4 * y + 2] = v.z & 0xffffffu; px[4 * y + 3] = v.w & 0xffffffu;
    } else {
      for (int x = 0; x < 4; x++) { uint32_t pxx = X * 4 + (uint32_t)x; if (pxx >= W) pxx = W - 1; px[4 * y + x] = row[pxx] & 0xffffffu; }
    }
  }
}
// the 8 texels of half `half` under `flip`
__device__ __forceinline__ void e2_gather(const uint32_t px[16], int flip, int half, uint32_t h[8]) {
#pragma unroll
  for (int j = 0; j < 8; j++) h[j] = flip ? px[8 * half + j] : px[4 * (j >> 1) + 2 * half + (j & 1)];
}
// q5 and q4 of a half: m8 = (sum + 4) >> 3 per channel
__device__ __forceinline__ void e2_means(const uint32_t h[8], int q5[3], int q4[3]) {
#pragma unroll
  for (int c = 0; c < 3; c++) {
    int s = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) s += (int)((h[j] >> (8 * c)) & 255u);
    const int m8 = (s + 4) >> 3;
    q5[c] = (m8 * 31 + 127) / 255; q4[c] = (m8 * 15 + 127) / 255;
  }
}

// E(base, t): sum over the half's texels of the smallest squared error among the four modified colours (each channel clamped to 0 .. 255)
__device__ inline uint32_t e2_half_err(const uint32_t h[8], int br, int bg, int bb, int t) {
  const int S = etc1_mag_s(t), L = etc1_mag_l(t);
  const int lo = br < bg ? (br < bb ? br : bb) : (bg < bb ? bg : bb), hi = br > bg ? (br > bb ? br : bb) : (bg > bb ? bg : bb);
  uint32_t tot = 0;
  if (lo - L >= 0 && hi + L <= 255) {
    // nothing clamps: the error under modifier d is A + 2 d B + 3 d^2 (A = sum_c e_c^2, B = sum_c e_c, e_c = base_c - p_c), so the best of
    // +-M is A + 3 M^2 - M |2 B| - the integers of the per-channel form below
    const int kl = 3 * L * L, ks = 3 * S * S;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const int er = br - (int)(h[j] & 255u), eg = bg - (int)((h[j] >> 8) & 255u), eb = bb - (int)((h[j] >> 16) & 255u);
      const int A = er * er + eg * eg + eb * eb, B2 = 2 * (er + eg + eb), ab = B2 < 0 ? -B2 : B2;
      const int a = kl - L * ab, b = ks - S * ab;
      tot += (uint32_t)(A + (a < b ? a : b));
    }
    return tot;
  }
  for (int j = 0; j < 8; j++) {
    const int r = (int)(h[j] & 255u), g = (int)((h[j] >> 8) & 255u), b = (int)((h[j] >> 16) & 255u);
    uint32_t be = 0xffffffffu;
    for (uint32_t s = 0; s < 4; s++) {
      const int d = etc1_mod(S, L, s);
      const int dr = t_clampi(br + d, 0, 255) - r, dg = t_clampi(bg + d, 0, 255) - g, db = t_clampi(bb + d, 0, 255) - b;
      const uint32_t e = (uint32_t)(dr * dr + dg * dg + db * db);
      if (e < be) be = e;
    }
    tot += be;
  }
  return tot;
}
template <int TOP> __device__ __forceinline__ uint32_t e2_code_err(const uint32_t h[8], uint32_t code) {
  return e2_half_err(h, e2_expand<TOP>((int)((code >> 10) & 31u)), e2_expand<TOP>((int)((code >> 5) & 31u)), e2_expand<TOP>((int)(code & 31u)), (int)(code >> 15));
}

// the half search in precision TOP (31: 5 bits, 15: 4 bits) from q: `refined` after steps 1 and 2, `plain` = the best table at base q
template <int TOP>
__device__ inline void e2_search(const uint32_t h[8], const int q[3], unsigned long long &refined, unsigned long long &plain) {
  uint32_t be = 0xffffffffu, bc = 0, ue = 0xffffffffu, uc = 0;
  for (int t = 0; t < 8; t++) {
    for (int k = 0; k < 3; k++) {
      const int dd = k == 0 ? 0 : (k == 1 ? -1 : 1);
      const uint32_t code = ((uint32_t)t << 15) | ((uint32_t)t_clampi(q[0] + dd, 0, TOP) << 10) | ((uint32_t)t_clampi(q[1] + dd, 0, TOP) << 5) | (uint32_t)t_clampi(q[2] + dd, 0, TOP);
      const uint32_t e = e2_code_err<TOP>(h, code);
      if (e < be) { be = e; bc = code; }
      if (k == 0 && e < ue) { ue = e; uc = code; }
    }
  }
  for (int c = 0; c < 3; c++) {
    const int sh = 10 - 5 * c;
    for (int k = 0; k < 2; k++) {
      const int v = (int)((bc >> sh) & 31u) + (k ? 1 : -1);
      if (v < 0 || v > TOP) continue;
      const uint32_t code = (bc & ~(31u << sh)) | ((uint32_t)v << sh);
      const uint32_t e = e2_code_err<TOP>(h, code);
      if (e < be) { be = e; bc = code; }
    }
  }
  refined = e2_word(be, bc); plain = e2_word(ue, uc);
}

// every delta second - first of two 5-bit fits in -4 .. 3
__device__ __forceinline__ bool e2_fits(unsigned long long a, unsigned long long b) {
  bool ok = true;
#pragma unroll
  for (int sh = 0; sh <= 10; sh += 5) { const int d = (int)((b >> sh) & 31u) - (int)((a >> sh) & 31u); ok = ok && d >= -4 && d <= 3; }
  return ok;
}
// one flip: r5 / u5 / r4 [half] = the refined 5-bit, the unrefined 5-bit and the refined 4-bit fit -> error << 32 | bytes 0 .. 3 of the block
__device__ inline unsigned long long e2_flip_pick(const unsigned long long r5[2], const unsigned long long u5[2], const unsigned long long r4[2], int flip) {
  const uint32_t e_ind = e2_err(r4[0]) + e2_err(r4[1]);
  unsigned long long d0 = 0, d1 = 0; bool have = false;
  if (e2_fits(r5[0], r5[1])) { d0 = r5[0]; d1 = r5[1]; have = true; }
  else if (e2_fits(u5[0], u5[1])) { d0 = u5[0]; d1 = u5[1]; have = true; }
  uint32_t hdr = 0;
  if (have && e2_err(d0) + e2_err(d1) <= e_ind) {
#pragma unroll
    for (int c = 0; c < 3; c++) { const int sh = 10 - 5 * c; const uint32_t b0 = (uint32_t)(d0 >> sh) & 31u, b1 = (uint32_t)(d1 >> sh) & 31u; hdr |= ((b0 << 3) | ((b1 - b0) & 7u)) << (8 * c); }
    hdr |= ((((uint32_t)(d0 >> 15) & 7u) << 5) | (((uint32_t)(d1 >> 15) & 7u) << 2) | 2u | (uint32_t)flip) << 24;
    return e2_word(e2_err(d0) + e2_err(d1), hdr);
  }
#pragma unroll
  for (int c = 0; c < 3; c++) { const int sh = 10 - 5 * c; hdr |= ((((uint32_t)(r4[0] >> sh) & 15u) << 4) | ((uint32_t)(r4[1] >> sh) & 15u)) << (8 * c); }
  hdr |= ((((uint32_t)(r4[0] >> 15) & 7u) << 5) | (((uint32_t)(r4[1] >> 15) & 7u) << 2) | (uint32_t)flip) << 24;
  return e2_word(e_ind, hdr);
}
// pixel indices of rows [y0, y1) under the block header `hdr` (bytes 0 .. 3, read back as a decoder reads them): every texel takes the first
// nearest of the four modified colours in pixel-index order; -> msb plane | lsb plane << 16
__device__ inline uint32_t e2_select(const uint32_t px[16], uint32_t hdr, int y0, int y1) {
  const uint32_t b3 = hdr >> 24; const bool diff = (b3 & 2u) != 0; const int flip = (int)(b3 & 1u);
  int base[2][3];
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const int B = (int)((hdr >> (8 * c)) & 255u);
    if (diff) { const int b0 = B >> 3, d = (B & 7) >= 4 ? (B & 7) - 8 : (B & 7); base[0][c] = e2_expand<31>(b0); base[1][c] = e2_expand<31>(b0 + d); }
    else { base[0][c] = e2_expand<15>(B >> 4); base[1][c] = e2_expand<15>(B & 15); }
  }
  const int tab[2] = { (int)(b3 >> 5), (int)((b3 >> 2) & 7u) };
  uint32_t msb = 0, lsb = 0;
  for (int y = y0; y < y1; y++) for (int x = 0; x < 4; x++) {
    const int hf = flip ? (y >= 2) : (x >= 2), S = etc1_mag_s(tab[hf]), L = etc1_mag_l(tab[hf]);
    const uint32_t p = px[4 * y + x]; const int r = (int)(p & 255u), g = (int)((p >> 8) & 255u), b = (int)((p >> 16) & 255u);
    uint32_t be = 0xffffffffu, bi = 0;
    for (uint32_t s = 0; s < 4; s++) {
      const int d = etc1_mod(S, L, s);
      const int dr = t_clampi(base[hf][0] + d, 0, 255) - r, dg = t_clampi(base[hf][1] + d, 0, 255) - g, db = t_clampi(base[hf][2] + d, 0, 255) - b;
      const uint32_t e = (uint32_t)(dr * dr + dg * dg + db * db);
      if (e < be) { be = e; bi = s; }
    }
    etc1_plane_put(msb, lsb, x, y, bi);
  }
  return msb | (lsb << 16);
}

// Four lanes per block: thread g works on block g / 4 of the batch (layer-major, raster order inside a layer) as lane k = g % 4 of its quad.
// E2_BLOCK and the stride are multiples of 64, so the lanes of a quad are neighbours in one wave.  A wave stays in the loop as long as its
// first lane has work, so that every lane of it takes part in the shuffles; lanes past the end redo the last block and store nothing.
__global__ void __launch_bounds__(E2_BLOCK) k_etc2_encode(const uint8_t *const *layers, uint8_t *const *outs, uint32_t W, uint32_t H, uint32_t bx, uint32_t by,
                                                           uint32_t n_layers, int yflip) {
  const unsigned long long nbk = (unsigned long long)bx * by, items = nbk * n_layers, stride = (unsigned long long)gridDim.x * E2_BLOCK;
  for (unsigned long long g = (unsigned long long)blockIdx.x * E2_BLOCK + threadIdx.x; (g & ~63ull) / 4 < items; g += stride) {
    const bool live = g / 4 < items;
    const unsigned long long it = live ? g / 4 : items - 1; const int k = (int)(g & 3), flip = k >> 1, half = k & 1;
    const uint32_t li = (uint32_t)(it / nbk), b = (uint32_t)(it % nbk);
    uint32_t px[16], h[8];
    e2_load_block(layers[li], W, H, yflip, b % bx, b / bx, px);
    int q5[3], q4[3];
    unsigned long long m5, mu, m4, unused;
    e2_gather(px, flip, half, h); e2_means(h, q5, q4);
    e2_search<31>(h, q5, m5, mu); e2_search<15>(h, q4, m4, unused);
    const unsigned long long o5 = __shfl_xor(m5, 1), ou = __shfl_xor(mu, 1), o4 = __shfl_xor(m4, 1);      // the other half of this flip
    const unsigned long long r5[2] = { half ? o5 : m5, half ? m5 : o5 }, u5[2] = { half ? ou : mu, half ? mu : ou }, r4[2] = { half ? o4 : m4, half ? m4 : o4 };
    const unsigned long long mine = e2_flip_pick(r5, u5, r4, flip), other = __shfl_xor(mine, 2);             // the other flip
    const unsigned long long pick0 = flip ? other : mine, pick1 = flip ? mine : other;
    const uint32_t hdr = (uint32_t)(e2_err(pick1) < e2_err(pick0) ? pick1 : pick0);
    uint32_t sel = e2_select(px, hdr, k, k + 1);
    sel |= __shfl_xor(sel, 1); sel |= __shfl_xor(sel, 2);
    if (k == 0 && live) *reinterpret_cast<uint2 *>(outs[li] + 8 * (size_t)b) = etc1_words(hdr, sel & 0xffffu, sel >> 16);      // blocks[] are 8-byte aligned: one store
  }
}

// ================================================================================================
// host side
// ================================================================================================
struct Etc2State { uvol_devbuf in, out, ptrs; std::vector<const uint8_t *> hptrs; };
void etc2_destroy(uvol_ctx *ctx) {
  Etc2State *S = ctx->etc2; if (!S) return;
  for (uvol_devbuf *b : { &S->in, &S->out, &S->ptrs }) if (b->p) (void)hipFree(b->p);
  delete S; ctx->etc2 = nullptr;
}
// uvol_trim: the staging buffers of host inputs / outputs go back to the device; the next call allocates what it needs
void etc2_trim(uvol_ctx *ctx) {
  Etc2State *S = ctx->etc2; if (!S) return;
  for (uvol_devbuf *b : { &S->in, &S->out, &S->ptrs }) if (b->p) { (void)hipFree(b->p); b->p = nullptr; b->cap = 0; }
}

// n layers of w x h RGBA8 (device pointers, or host memory uploaded through the staging buffers) -> blocks[i] = ceil(w / 4) ceil(h / 4) ETC1
// blocks (device pointers, or host memory).  One launch for the whole batch on the context's stream, behind the un-filter of any ingest slot
// the layers lie in; returns when the blocks are complete.
int etc2_rgb_batch(uvol_ctx *ctx, const uint8_t *const *rgba, int n, uint32_t w, uint32_t h, bool inputs_on_device, uint8_t *const *blocks, size_t layer_cap, bool outputs_on_device) {
  if (n <= 0) return UVOL_OK;
  if (!w || !h || w > 8192 || h > 16384) { ctx->set_error("uvol_encode_etc2_rgb_batch: width %u x height %u (1 x 1 up to 8192 x 16384)", w, h); return UVOL_E_INVALID; }
  for (int i = 0; i < n; i++) {
    if (!rgba[i]) { ctx->set_error("uvol_encode_etc2_rgb_batch: rgba[%d] is NULL", i); return UVOL_E_INVALID; }
    if (!blocks[i]) { ctx->set_error("uvol_encode_etc2_rgb_batch: blocks[%d] is NULL", i); return UVOL_E_INVALID; }
    if (inputs_on_device && ((uintptr_t)rgba[i] & 3)) { ctx->set_error("uvol_encode_etc2_rgb_batch: rgba[%d] is a device layer that is not 4-byte aligned", i); return UVOL_E_INVALID; }
    if (outputs_on_device && ((uintptr_t)blocks[i] & 7)) { ctx->set_error("uvol_encode_etc2_rgb_batch: blocks[%d] is a device buffer that is not 8-byte aligned", i); return UVOL_E_INVALID; }
  }
  const uint32_t bx = (w + 3) / 4, by = (h + 3) / 4;
  const size_t ibytes = (size_t)w * h * 4, obytes = (size_t)bx * by * 8;
  if (layer_cap < obytes) { ctx->set_error("uvol_encode_etc2_rgb_batch: layer_cap %zu < %zu (uvol_etc2_rgb_bound)", layer_cap, obytes); return UVOL_E_NOSPACE; }
  if (!ctx->etc2) ctx->etc2 = new Etc2State();
  Etc2State *S = ctx->etc2;
  int rc;
  if ((rc = uvol_ensure(ctx, S->ptrs, 2 * sizeof(uint8_t *) * (size_t)n))) return rc;
  if (!outputs_on_device && (rc = uvol_ensure(ctx, S->out, obytes * (size_t)n))) return rc;
  S->hptrs.assign((size_t)2 * n, nullptr);                // [0, n): the layers, [n, 2 n): where the kernel writes
  for (int i = 0; i < n; i++) { S->hptrs[(size_t)i] = rgba[i]; S->hptrs[(size_t)n + i] = outputs_on_device ? blocks[i] : (uint8_t *)S->out.p + obytes * (size_t)i; }
  if (inputs_on_device) {
    if ((rc = png_order_before(ctx, ctx->stream, rgba, (size_t)n))) return rc;
  } else {
    if ((rc = uvol_ensure(ctx, S->in, ibytes * (size_t)n))) return rc;
    std::vector<UvolUpItem> ups; ups.reserve((size_t)n);
    for (int i = 0; i < n; i++) { ups.push_back(UvolUpItem{ ibytes * (size_t)i, rgba[i], ibytes }); S->hptrs[(size_t)i] = (const uint8_t *)S->in.p + ibytes * (size_t)i; }
    uvol_ctx::Scope sc(ctx, "etc2.upload", (uint64_t)ibytes * n);
    if ((rc = uvol_upload_staged(ctx, (uint8_t *)S->in.p, ups))) return rc;
  }
  UVOL_HIP_CHECK(ctx, hipMemcpyAsync(S->ptrs.p, S->hptrs.data(), 2 * sizeof(uint8_t *) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
  const unsigned long long threads = (unsigned long long)n * bx * by * 4;
  const unsigned grid = (unsigned)std::min<unsigned long long>((threads + E2_BLOCK - 1) / E2_BLOCK, (unsigned long long)E2_MAX_GRID);
  { uvol_ctx::Scope sc(ctx, "etc2.encode", (uint64_t)(ibytes + obytes) * n);
    if (uvol_debug()) { fprintf(stderr, "[uvol] launch k_etc2_encode %d layers %u x %u\n", n, w, h); fflush(stderr); }
    const uint8_t *const *lp = (const uint8_t *const *)S->ptrs.p; uint8_t *const *op = (uint8_t *const *)S->ptrs.p + n;
    hipLaunchKernelGGL(k_etc2_encode, dim3(grid), dim3(E2_BLOCK), 0, ctx->stream, lp, op, w, h, bx, by, (uint32_t)n, ctx->prm.y_flip ? 1 : 0);
  }
  UVOL_HIP_CHECK(ctx, hipGetLastError());
  if (outputs_on_device) UVOL_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  else {
    std::vector<UvolDnItem> dns; dns.reserve((size_t)n);
    for (int i = 0; i < n; i++) dns.push_back(UvolDnItem{ (const uint8_t *)S->out.p + obytes * (size_t)i, blocks[i], obytes });
    if ((rc = uvol_download_staged(ctx, dns))) return rc;
  }
  ctx->resolve_profile();
  return UVOL_OK;
}
