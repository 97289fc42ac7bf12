// jpeg_ingest.hip — JPEG coefficients to RGBA8 layers on the device (uvol_idct_jpeg_batch_dev; SURVEY §8 f-3, the ingest stage).
//
// The reference's README names a JPEG as its example texture input, and the `basisu` that scripts/Encoder.py:290 spawns reads .jpg as it reads
// .png.  The split is the PNG one (png_ingest.hip): the serial bit stream - marker parse and Huffman decode - stays on the ingest threads
// (host/uvol_host.cpp read_jpeg_raw), the data-parallel part runs here, straight into the RGBA8 layers of an ingest slot that the texture
// encoders read from HBM.  The decoding rule is stated once, in include/uvol_codec.h ("THE DECODING RULE"); it is exact in integers, and this
// file, host/uvol_host.cpp read_jpeg and the NumPy restatement of tests/jpeg_cases.py agree bit for bit.
//
// Two kernels per call, each one launch for the whole batch:
//   k_jpeg_idct   every 8 x 8 block of every component of every image: dequantise, column pass, row pass, level shift -> one byte per
//                 sample in a plane per component (padded to whole MCUs) in a scratch buffer of the state.  EIGHT LANES SHARE A BLOCK: lane r
//                 loads row r of the block (its 16 bytes in one load, the 16 bytes of the quantisation row in another), the 1-D passes
//                 exchange through LDS - the column pass needs a column per lane, the row pass a row per lane.  A block's LDS tile is 36
//                 words (32 + 4 of padding): the column reads of the eight blocks of a wave then fall into eight disjoint groups of four
//                 banks (36 k mod 64 = 0, 36, 8, 44, 16, 52, 24, 60), and a row is still one aligned 16-byte access.  Values are int16 in
//                 LDS (both intermediate results are clamped to that range by the rule).  A 1-D pass is 32 multiply-adds, not 64: K[7 - x][u] =
//                 (-1)^u K[x][u] holds exactly in the integer table, and integer sums do not depend on their order.
//   k_jpeg_rgba   eight neighbouring texels of one row per lane: luma as one 8-byte load, chroma through the 2 x 1 / 2 x 2 filter over the
//                 component's REAL extent (a neighbour outside it is the sample itself), YCbCr -> RGB, two 16-byte stores where the width
//                 allows it (the rule of t_store_row4 in tex_blocks.hpp), 4-byte stores otherwise.
// Planes first and a second pass over texels, instead of one kernel that recomputes the chroma halo of its MCU run: the 2 x 2 filter of a
// texel row needs chroma rows of the MCU row above or below and columns of the MCUs left and right, i.e. for a run of MCUs a halo of whole
// blocks (an IDCT yields 8 x 8 samples or nothing) - at 4:2:0 one extra chroma block row per 16 texel rows on each side, which is twice the
// chroma IDCT work and twice its coefficient reads.  The planes cost 1.5 bytes written and read per texel (4:2:0) against 4 bytes of output
// and stay in L2 between the kernels for batches of the size the drivers issue; both kernels are plain streaming passes.
// Every read is bounded by the padded planes (a lane of the last group of a row reads luma bytes up to the next multiple of 8, the
// planes' pitch), every chroma index is clamped to the real extent, every write by W and H.
#include "uvol_common.hpp"
#include <cmath>

struct JpegGeom {
  uint32_t W, H, ncomp, hs, vs;          // hs / vs: the luma sampling factors (chroma is 1 x 1)
  uint32_t bw[3], bh[3], boff[3], nb;    // per component: block grid, first block within the image; blocks per image
  uint32_t cw[3], ch[3];                 // per component: real extent in samples
};

#define JPEG_IDCT_BLOCK 256
#define JPEG_TILE 36                     /* LDS words per block: 8 rows of 4 words (8 int16) + 4 words of padding */

// one 1-D pass of the rule: out[x] = sum_u K[x][u] in[u], K = floor(8192 s_u cos((2 x + 1) u pi / 16) + 0.5) (jpeg_check_table below)
__device__ __forceinline__ void jpeg_idct8(const int *a, int *o) {
  const int e0 = 2896 * a[0] + 3784 * a[2] + 2896 * a[4] + 1567 * a[6];
  const int e1 = 2896 * a[0] + 1567 * a[2] - 2896 * a[4] - 3784 * a[6];
  const int e2 = 2896 * a[0] - 1567 * a[2] - 2896 * a[4] + 3784 * a[6];
  const int e3 = 2896 * a[0] - 3784 * a[2] + 2896 * a[4] - 1567 * a[6];
  const int o0 = 4017 * a[1] + 3406 * a[3] + 2276 * a[5] + 799 * a[7];
  const int o1 = 3406 * a[1] - 799 * a[3] - 4017 * a[5] - 2276 * a[7];
  const int o2 = 2276 * a[1] - 4017 * a[3] + 799 * a[5] + 3406 * a[7];
  const int o3 = 799 * a[1] - 2276 * a[3] + 3406 * a[5] - 4017 * a[7];
  o[0] = e0 + o0; o[7] = e0 - o0; o[1] = e1 + o1; o[6] = e1 - o1;
  o[2] = e2 + o2; o[5] = e2 - o2; o[3] = e3 + o3; o[4] = e3 - o3;
}
__device__ __forceinline__ int jpeg_clamp16(int v) { return v < -32768 ? -32768 : (v > 32767 ? 32767 : v); }
__device__ __forceinline__ int jpeg_lo16(uint32_t w) { return (int)(int16_t)(w & 0xffffu); }
__device__ __forceinline__ int jpeg_hi16(uint32_t w) { return (int)w >> 16; }

__global__ void __launch_bounds__(JPEG_IDCT_BLOCK) k_jpeg_idct(const int16_t *coef, const uint16_t *qt, uint8_t *planes, JpegGeom G, unsigned long long total) {
  __shared__ __attribute__((aligned(16))) uint32_t tile[(JPEG_IDCT_BLOCK / 8) * JPEG_TILE];
  const uint32_t tid = threadIdx.x, r = tid & 7u, blk = tid >> 3;
  uint32_t *T = tile + blk * JPEG_TILE;                    // this block's tile: only the eight lanes that share the block touch it
  const unsigned long long per = JPEG_IDCT_BLOCK / 8, stride = (unsigned long long)gridDim.x * per;
  for (unsigned long long base = (unsigned long long)blockIdx.x * per; base < total; base += stride) {      // (workgroup-uniform trip count)
    const unsigned long long g = base + blk; const bool on = g < total;
    uint32_t img = 0, c = 0, bx = 0, by = 0;
    int a[8], o[8];
    if (on) {
      img = (uint32_t)(g / G.nb); const uint32_t bi = (uint32_t)(g % G.nb);
      c = (G.ncomp == 3 && bi >= G.boff[1]) ? (bi >= G.boff[2] ? 2u : 1u) : 0u;
      const uint32_t lb = bi - G.boff[c]; bx = lb % G.bw[c]; by = lb / G.bw[c];
      // row r of the block: 8 quantised int16, and row r of the component's table: 8 uint16
      const uint4 cv = *reinterpret_cast<const uint4 *>(coef + g * 64ull + 8u * r);
      const uint4 qv = *reinterpret_cast<const uint4 *>(qt + ((size_t)img * G.ncomp + c) * 64u + 8u * r);
      const uint32_t cw_[4] = { cv.x, cv.y, cv.z, cv.w }, qw_[4] = { qv.x, qv.y, qv.z, qv.w };
      uint32_t pk[4];
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const int f0 = jpeg_clamp16(jpeg_lo16(cw_[j]) * (int)(qw_[j] & 0xffffu)), f1 = jpeg_clamp16(jpeg_hi16(cw_[j]) * (int)(qw_[j] >> 16));
        pk[j] = ((uint32_t)f0 & 0xffffu) | ((uint32_t)f1 << 16);
      }
      *reinterpret_cast<uint4 *>(T + 4u * r) = make_uint4(pk[0], pk[1], pk[2], pk[3]);
    }
    __syncthreads();
    if (on) {                                              // column pass: this lane takes column u = r
#pragma unroll
      for (int v = 0; v < 8; v++) { const uint32_t w = T[4 * v + (r >> 1)]; a[v] = (r & 1u) ? jpeg_hi16(w) : jpeg_lo16(w); }
      jpeg_idct8(a, o);
#pragma unroll
      for (int y = 0; y < 8; y++) o[y] = jpeg_clamp16((o[y] + 1024) >> 11);
    }
    __syncthreads();                                       // (every column is read before any b[][] is written)
    if (on) {
      uint16_t *Th = reinterpret_cast<uint16_t *>(T);
#pragma unroll
      for (int y = 0; y < 8; y++) Th[8 * y + r] = (uint16_t)o[y];
    }
    __syncthreads();
    if (on) {                                              // row pass: this lane takes row y = r
      const uint4 bv = *reinterpret_cast<const uint4 *>(T + 4u * r);
      const uint32_t bw_[4] = { bv.x, bv.y, bv.z, bv.w };
#pragma unroll
      for (int j = 0; j < 4; j++) { a[2 * j] = jpeg_lo16(bw_[j]); a[2 * j + 1] = jpeg_hi16(bw_[j]); }
      jpeg_idct8(a, o);
      uint32_t s[2] = { 0, 0 };
#pragma unroll
      for (int x = 0; x < 8; x++) { int p = ((o[x] + 16384) >> 15) + 128; p = p < 0 ? 0 : (p > 255 ? 255 : p); s[x >> 2] |= (uint32_t)p << (8 * (x & 3)); }
      const size_t pitch = (size_t)G.bw[c] * 8u;
      uint8_t *dst = planes + (size_t)img * G.nb * 64u + (size_t)G.boff[c] * 64u + ((size_t)by * 8u + r) * pitch + (size_t)bx * 8u;
      *reinterpret_cast<uint2 *>(dst) = make_uint2(s[0], s[1]);
    }
    __syncthreads();                                       // (the rows are read before the next trip writes the tile)
  }
}

// a chroma row index's neighbour j over the real extent [0, n): outside it, the row itself
__device__ __forceinline__ uint32_t jpeg_nb(uint32_t i, int j, uint32_t n) { return (j < 0 || j >= (int)n) ? i : (uint32_t)j; }
__device__ __forceinline__ uint32_t jpeg_rgb(int Y, int Cb, int Cr) {
  const int cb = Cb - 128, cr = Cr - 128;
  int R = Y + ((91881 * cr + 32768) >> 16), Gn = Y - ((22554 * cb + 46802 * cr + 32768) >> 16), B = Y + ((116130 * cb + 32768) >> 16);
  R = R < 0 ? 0 : (R > 255 ? 255 : R); Gn = Gn < 0 ? 0 : (Gn > 255 ? 255 : Gn); B = B < 0 ? 0 : (B > 255 ? 255 : B);
  return (uint32_t)R | ((uint32_t)Gn << 8) | ((uint32_t)B << 16) | 0xff000000u;
}

// EIGHT texels of a row per lane: their luma is one aligned 8-byte load; at 4:2:2 / 4:2:0 their four chroma samples are one aligned 4-byte load
// per row and component, and the filter's two outer neighbours one byte each (where they exist: outside the real extent the sample itself
// stands in).  The first form took four texels per lane and fetched every chroma sample and neighbour by a byte load, 25 loads per four
// texels: 1.02 ms for 64 layers of 2048 x 2048 against 0.37 ms for the IDCT kernel.
__global__ void __launch_bounds__(256) k_jpeg_rgba(const uint8_t *planes, uint8_t *out0, JpegGeom G, uint32_t n) {
  const uint32_t G8 = (G.W + 7u) / 8u;
  const unsigned long long items = (unsigned long long)n * G.H * G8, stride = (unsigned long long)gridDim.x * 256ull;
  const size_t pbytes = (size_t)G.nb * 64u, obytes = (size_t)G.W * G.H * 4u;
  for (unsigned long long it = (unsigned long long)blockIdx.x * 256ull + threadIdx.x; it < items; it += stride) {
    const uint32_t gx = (uint32_t)(it % G8); const unsigned long long t = it / G8;
    const uint32_t y = (uint32_t)(t % G.H), img = (uint32_t)(t / G.H);
    const uint8_t *P = planes + pbytes * img;
    const uint2 yv = *reinterpret_cast<const uint2 *>(P + (size_t)y * (G.bw[0] * 8u) + 8u * gx);      // (every plane's pitch is a multiple of 8: aligned, in bounds)
    const uint32_t yw[2] = { yv.x, yv.y };
    uint32_t px[8];
    if (G.ncomp == 1) {
#pragma unroll
      for (int k = 0; k < 8; k++) { const uint32_t v = (yw[k >> 2] >> (8 * (k & 3))) & 255u; px[k] = v | (v << 8) | (v << 16) | 0xff000000u; }
    } else {
      int cc[2][8];                                         // Cb, Cr of the eight texels
#pragma unroll
      for (int c = 1; c <= 2; c++) {
        const uint8_t *C = P + (size_t)G.boff[c] * 64u; const size_t pitch = (size_t)G.bw[c] * 8u; const uint32_t cw = G.cw[c], ch = G.ch[c];
        int *dst = cc[c - 1];
        if (G.hs == 1) {
          const uint2 cv = *reinterpret_cast<const uint2 *>(C + (size_t)y * pitch + 8u * gx);
          const uint32_t w[2] = { cv.x, cv.y };
#pragma unroll
          for (int k = 0; k < 8; k++) dst[k] = (int)((w[k >> 2] >> (8 * (k & 3))) & 255u);
        } else {
          // a[1 .. 4]: the four samples (at 4:2:0 after the vertical step 3 c + above / below, not rounded), a[0] / a[5]: their outer neighbours
          const bool two = G.vs == 2; const uint32_t i0 = 4u * gx;
          const uint32_t cy = two ? (y >> 1) : y, oy = two ? jpeg_nb(cy, (y & 1u) ? (int)cy + 1 : (int)cy - 1, ch) : cy;
          const uint8_t *rc = C + (size_t)cy * pitch, *ro = C + (size_t)oy * pitch;
          const uint32_t wc = *reinterpret_cast<const uint32_t *>(rc + i0), wo = *reinterpret_cast<const uint32_t *>(ro + i0);
          int a[6];
#pragma unroll
          for (int j = 0; j < 4; j++) { const int sc = (int)((wc >> (8 * j)) & 255u), so = (int)((wo >> (8 * j)) & 255u); a[j + 1] = two ? 3 * sc + so : sc; }
          a[0] = i0 > 0 ? (two ? 3 * rc[i0 - 1] + ro[i0 - 1] : (int)rc[i0 - 1]) : a[1];
          a[5] = i0 + 4u < cw ? (two ? 3 * rc[i0 + 4] + ro[i0 + 4] : (int)rc[i0 + 4]) : a[4];
          const int rl = two ? 8 : 1, rr = two ? 7 : 2, sh = two ? 4 : 2;
#pragma unroll
          for (int j = 0; j < 4; j++) {
            const int m = a[j + 1], l = a[j], r = (i0 + (uint32_t)j + 1u < cw) ? a[j + 2] : m;      // (a sample behind the real extent belongs to texels behind W, which are not stored)
            dst[2 * j] = (3 * m + l + rl) >> sh; dst[2 * j + 1] = (3 * m + r + rr) >> sh;
          }
        }
      }
#pragma unroll
      for (int k = 0; k < 8; k++) px[k] = jpeg_rgb((int)((yw[k >> 2] >> (8 * (k & 3))) & 255u), cc[0][k], cc[1][k]);
    }
    // the layer starts at base + img W H 4: 16-byte aligned when W is a multiple of 4, and then a group of four is whole (as t_store_row4 decides)
    uint32_t *orow = reinterpret_cast<uint32_t *>(out0 + obytes * img) + (size_t)y * G.W + 8u * gx;
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const uint32_t x0 = 8u * gx + 4u * (uint32_t)h;
      if ((G.W & 3u) == 0) { if (x0 < G.W) *reinterpret_cast<uint4 *>(orow + 4 * h) = make_uint4(px[4 * h], px[4 * h + 1], px[4 * h + 2], px[4 * h + 3]); }
      else {
#pragma unroll
        for (int k = 0; k < 4; k++) if (x0 + (uint32_t)k < G.W) orow[4 * h + k] = px[4 * h + k];
      }
    }
  }
}

// ================================================================================================
// host side
// ================================================================================================
struct JpegState { uvol_devbuf coef, qt, planes; std::vector<uint16_t> hqt; hipEvent_t up_done = nullptr; int table_ok = -1; };

// the cosine table of the rule, computed as the rule says, against the constants of jpeg_idct8 (the margin to a rounding boundary is far
// above what a libm can differ by; the check makes that a fact of the build at hand)
static bool jpeg_check_table() {
  static const int k0[8] = { 2896, 4017, 3784, 3406, 2896, 2276, 1567, 799 };
  const double pi = 3.14159265358979323846;
  for (int x = 0; x < 8; x++) for (int u = 0; u < 8; u++) {
    const double s = u == 0 ? 1.0 / (2.0 * std::sqrt(2.0)) : 0.5;
    const int k = (int)std::floor(8192.0 * s * std::cos((2 * x + 1) * u * pi / 16.0) + 0.5);
    // K[x][u] = +- K[0][m] with (2 x + 1) u folded into the first quadrant: compare through a direct evaluation of the butterfly's sign rule
    const int q = ((2 * x + 1) * u) % 32, m = q <= 8 ? q : (q <= 16 ? 16 - q : (q <= 24 ? q - 16 : 32 - q)), sign = (q > 8 && q < 24) ? -1 : 1;
    const int want = u == 0 ? 2896 : (m == 8 ? 0 : sign * (m == 4 ? 2896 : k0[m]));
    if (k != want) return false;
  }
  return true;
}

static bool jpeg_geom(const uvol_jpeg_layout *L, JpegGeom &G) {
  if (!L || !L->width || !L->height || L->width > 8192 || L->height > 16384) return false;
  if (L->components == 1) { G.hs = 1; G.vs = 1; }
  else if (L->components == 3 && ((L->luma_h == 1 && L->luma_v == 1) || (L->luma_h == 2 && L->luma_v == 1) || (L->luma_h == 2 && L->luma_v == 2))) { G.hs = (uint32_t)L->luma_h; G.vs = (uint32_t)L->luma_v; }
  else return false;
  G.W = L->width; G.H = L->height; G.ncomp = (uint32_t)L->components;
  const uint32_t mw = (G.W + 8 * G.hs - 1) / (8 * G.hs), mh = (G.H + 8 * G.vs - 1) / (8 * G.vs);
  uint32_t off = 0;
  for (uint32_t c = 0; c < 3; c++) {
    const uint32_t h = c == 0 ? G.hs : 1, v = c == 0 ? G.vs : 1;
    if (c >= G.ncomp) { G.bw[c] = G.bh[c] = G.cw[c] = G.ch[c] = 0; G.boff[c] = off; continue; }
    G.bw[c] = mw * h; G.bh[c] = mh * v; G.boff[c] = off; off += G.bw[c] * G.bh[c];
    G.cw[c] = (G.W * h + G.hs - 1) / G.hs; G.ch[c] = (G.H * v + G.vs - 1) / G.vs;
  }
  G.nb = off;                                              // at most 1024 x 2048 x 3 blocks: fits 32 bits
  return true;
}
size_t jpeg_coeff_count(const uvol_jpeg_layout *L) { JpegGeom G; return jpeg_geom(L, G) ? (size_t)G.nb * 64 : 0; }

void jpeg_destroy(uvol_ctx *ctx) {
  JpegState *S = ctx->jpeg; if (!S) return;
  for (uvol_devbuf *b : { &S->coef, &S->qt, &S->planes }) if (b->p) (void)hipFree(b->p);
  if (S->up_done) (void)hipEventDestroy(S->up_done);
  delete S; ctx->jpeg = nullptr;
}
// uvol_trim: the coefficient and plane buffers go back to the device (the slots themselves: png_trim)
void jpeg_trim(uvol_ctx *ctx) {
  JpegState *S = ctx->jpeg; if (!S) return;
  for (uvol_devbuf *b : { &S->coef, &S->qt, &S->planes }) if (b->p) { (void)hipFree(b->p); b->p = nullptr; b->cap = 0; }
}

int jpeg_idct_batch(uvol_ctx *ctx, const int16_t *const *coeffs, const uint16_t *const *qtables, int n, const uvol_jpeg_layout *layout, int slot, const uint8_t **rgba_dev_out) {
  if (n <= 0) return UVOL_OK;
  if (slot < 0 || slot > 1) { ctx->set_error("uvol_idct_jpeg_batch_dev: slot %d (0 or 1)", slot); return UVOL_E_INVALID; }
  JpegGeom G;
  if (!jpeg_geom(layout, G)) {
    ctx->set_error("uvol_idct_jpeg_batch_dev: layout %u x %u, %d components, luma %d x %d (1 x 1 up to 8192 x 16384; grey, or Y Cb Cr with luma 1 x 1, 2 x 1 or 2 x 2)",
                   layout->width, layout->height, layout->components, layout->luma_h, layout->luma_v);
    return UVOL_E_INVALID;
  }
  for (int i = 0; i < n; i++) {
    if (!coeffs[i]) { ctx->set_error("uvol_idct_jpeg_batch_dev: coeffs[%d] is NULL", i); return UVOL_E_INVALID; }
    if (!qtables[i]) { ctx->set_error("uvol_idct_jpeg_batch_dev: qtables[%d] is NULL", i); return UVOL_E_INVALID; }
  }
  if (!ctx->jpeg) ctx->jpeg = new JpegState();
  JpegState *S = ctx->jpeg;
  if (S->table_ok < 0) S->table_ok = jpeg_check_table() ? 1 : 0;
  if (!S->table_ok) { ctx->set_error("uvol_idct_jpeg_batch_dev: the cosine table computed here differs from the kernel's constants"); return UVOL_E_HIP; }
  const size_t cbytes = (size_t)G.nb * 128, pbytes = (size_t)G.nb * 64, obytes = (size_t)G.W * G.H * 4, qbytes = (size_t)G.ncomp * 128;
  hipStream_t ingest = nullptr; uint8_t *base = nullptr; int rc;
  if ((rc = png_slot_begin(ctx, slot, obytes * (size_t)n, &ingest, &base))) return rc;
  hipStream_t saved = ctx->stream; ctx->stream = ingest;            // (uvol_ensure, uvol_upload_staged, Scope use ctx->stream)
  struct Restore { uvol_ctx *c; hipStream_t s; ~Restore() { c->stream = s; } } restore_{ ctx, saved };
  if ((rc = uvol_ensure(ctx, S->coef, cbytes * (size_t)n))) return rc;
  if ((rc = uvol_ensure(ctx, S->qt, qbytes * (size_t)n))) return rc;
  if ((rc = uvol_ensure(ctx, S->planes, pbytes * (size_t)n + 16))) return rc;
  std::vector<UvolUpItem> ups; ups.reserve((size_t)n);
  S->hqt.resize((size_t)n * G.ncomp * 64);
  for (int i = 0; i < n; i++) {
    ups.push_back(UvolUpItem{ cbytes * (size_t)i, coeffs[i], cbytes });
    std::memcpy(S->hqt.data() + (size_t)i * G.ncomp * 64, qtables[i], qbytes);
    rgba_dev_out[i] = base + obytes * (size_t)i;
  }
  bool direct = true; for (const UvolUpItem &it : ups) if (!uvol_host_pinned(it.src, it.bytes)) { direct = false; break; }
  { uvol_ctx::Scope sc(ctx, "jpeg.upload", (uint64_t)(cbytes + qbytes) * n);
    if ((rc = uvol_upload_staged(ctx, (uint8_t *)S->coef.p, ups))) return rc;
    UVOL_HIP_CHECK(ctx, hipMemcpyAsync(S->qt.p, S->hqt.data(), qbytes * (size_t)n, hipMemcpyHostToDevice, ctx->stream)); }
  // (as in png_ingest_batch: inputs that all lie in uvol_host_alloc memory go by DMA from where they lie, so the call waits for those copies)
  if (direct) {
    if (!S->up_done) UVOL_HIP_CHECK(ctx, hipEventCreateWithFlags(&S->up_done, hipEventDisableTiming));
    UVOL_HIP_CHECK(ctx, hipEventRecord(S->up_done, ctx->stream));
  }
  { uvol_ctx::Scope sc(ctx, "jpeg.idct", (uint64_t)(cbytes + obytes) * n);
    if (uvol_debug()) { fprintf(stderr, "[uvol] launch k_jpeg_idct, k_jpeg_rgba: %d images %u x %u, %u components, luma %u x %u\n", n, G.W, G.H, G.ncomp, G.hs, G.vs); fflush(stderr); }
    const unsigned long long total = (unsigned long long)G.nb * (unsigned long long)n, per = JPEG_IDCT_BLOCK / 8;
    const unsigned ga = (unsigned)std::min<unsigned long long>((total + per - 1) / per, 8192ull);
    hipLaunchKernelGGL(k_jpeg_idct, dim3(ga), dim3(JPEG_IDCT_BLOCK), 0, ctx->stream, (const int16_t *)S->coef.p, (const uint16_t *)S->qt.p, (uint8_t *)S->planes.p, G, total);
    const unsigned long long items = (unsigned long long)n * G.H * ((G.W + 7) / 8);
    const unsigned gb = (unsigned)std::min<unsigned long long>((items + 255) / 256, 8192ull);
    hipLaunchKernelGGL(k_jpeg_rgba, dim3(gb), dim3(256), 0, ctx->stream, (const uint8_t *)S->planes.p, base, G, (uint32_t)n); }
  UVOL_HIP_CHECK(ctx, hipGetLastError());
  if ((rc = png_slot_end(ctx, slot))) return rc;
  if (direct) UVOL_HIP_CHECK(ctx, hipEventSynchronize(S->up_done));      // (the kernels queued behind the copies run on)
  if (uvol_debug()) UVOL_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return UVOL_OK;
}
