// tex_mipchain.hip — the mip chain of RGBA8 layers on the device (uvol_mipchain_rgba_batch_dev): levels 1 .. levels - 1 of every layer in ONE
// pass over level 0, for the mip levels inside one UASTC .ktx2 (uvol_encode_texture_segments_mips; reference src/lib/KTX2Loader.js:279 turns
// trilinear filtering on only for a file that carries more than one level, and :516-570 transcodes every (mip, layer) the file has).
//
// The filter is the one of tex_downscale.hip with a box of any size (include/uvol_codec.h has the normative text): level v is
// lw x lh = max(1, W >> v) x max(1, H >> v), fx = W / lw and fy = H / lh are exact integers (the host refuses the call otherwise), and output
// texel (X, Y) comes in one step from the n = fx fy texels of level 0 in its box: A = sum a, N = sum lin[c] a (or sum lin[c] with D = n when
// A == 0), out.a = (2 A + n) / (2 n), m = (2 N + D) / (2 D), out.c = the v nearest to m in lin[].  A, sum lin a and sum lin are additive over
// boxes, so a level is computed from the sums of any finer level whose boxes tile its own - with the same result as from level 0 - and
// level 0 is read from HBM once, not once per level.
//
// Word sizes: a sum over n texels is at most 16 711 425 n, which fits 32 bits up to n = 256 (a 16 x 16 box); 2 N + D fits 32 bits up to
// n = 128.  So the boxes of levels 1 - 3 (n = 4, 16, 64), which a thread keeps in registers, are summed and divided in 32 bits exactly as
// k_downscale does it; from the 16 x 16 box of level 4 on (n = 256) sums and divisions are 64-bit (n <= 8192 x 16384 = 2^27: N < 2^51).
//
// k_mip_tiles: a workgroup of 16 x 16 threads takes a 128 x 128 tile of level 0, a thread an 8 x 8 box of it, two rows at a time: after two
// rows its four level-1 texels are complete (one 16-byte store), after four rows two level-2 texels, after eight the level-3 texel; the
// level-3 sums go to LDS and 64, 16, 4 and 1 threads make levels 4 - 7 of the tile from them.  Only the DYADIC levels are made here: v <= 7
// with 2^v dividing W and H, so that no box is cut by the image or by a tile.  What is left - levels beyond 7, and the levels of sizes such as
// 96 x 40 whose boxes are 16 x 20 - is made by k_mip_tail, one launch per level, from the sums of level u that k_mip_tiles leaves in a scratch
// array: u = the coarsest dyadic level whose boxes tile the boxes of every remaining level (7 for power-of-two sizes: 56 bytes per tile).
// k_mip_tail leaves its level's sums too, and the next level is made from those where its boxes nest (four entries per texel for powers of two).
// Measured (640 layers of 2048^2, profiles/r17_mipmaps.json): levels 1 - 3 in 4.5 ms where the three k_downscale launches take 9.1, the full
// 12-level chain in 5.5 ms = 2.6 TB/s of the bytes it must move.
// Memory-bound like k_downscale: every input byte once, a third of them written.  Every read is bounded by W and H, every write by the level's
// lw and lh; tiles at the right and bottom edge may be partial.
#include "uvol_common.hpp"
#include <algorithm>

#define MIP_BLOCK 256
#define MIP_TILE 128u
#define MIP_TILE_LEVELS 7u                              /* 2^7 = MIP_TILE */
#define MIP_MAX_LEVELS 15                               /* 16384 = 2^14 */
#define MIP_NO_SCRATCH 0xffffffffu

struct MipGeom {
  uint32_t W, H, n_layers, tiles_x, tiles_y;
  uint32_t la;                                           // k_mip_tiles makes levels 1 .. la
  uint32_t u, sw, sh;                                    // scratch: sums of level u (MIP_NO_SCRATCH: none), sw x sh entries of 7 words per layer
  uint32_t lw[MIP_TILE_LEVELS + 1], lh[MIP_TILE_LEVELS + 1];
  unsigned long long off[MIP_TILE_LEVELS + 1];           // level v of layer i: out + off[v] + i lw[v] lh[v] 4
};

__device__ __forceinline__ uint32_t mip_inverse(uint32_t m, const uint32_t *mid, const uint8_t *base) {      // tex_downscale.hip: down_inverse
  const uint32_t v = base[m >> 4];
  return v + (mid[v] < 2u * m ? 1u : 0u);
}
// s = { A, sum lin a (r, g, b), sum lin (r, g, b) } of a box of n = 2^ln texels -> the texel; 32-bit: n <= 128
__device__ __forceinline__ uint32_t mip_texel32(const uint32_t *s, uint32_t ln, const uint32_t *mid, const uint8_t *base) {
  const uint32_t n = 1u << ln, A = s[0], D = A ? A : n;
  uint32_t px = ((2u * A + n) >> (ln + 1u)) << 24;       // (2 A + n) / (2 n)
#pragma unroll
  for (int c = 0; c < 3; c++) { const uint32_t N = A ? s[1 + c] : s[4 + c]; px |= mip_inverse((2u * N + D) / (2u * D), mid, base) << (8 * c); }
  return px;
}
__device__ __forceinline__ uint32_t mip_texel64(const unsigned long long *s, unsigned long long n, const uint32_t *mid, const uint8_t *base) {
  const unsigned long long A = s[0], D = A ? A : n;
  uint32_t px = (uint32_t)((2ull * A + n) / (2ull * n)) << 24;
  for (int c = 0; c < 3; c++) { const unsigned long long N = A ? s[1 + c] : s[4 + c]; px |= mip_inverse((uint32_t)((2ull * N + D) / (2ull * D)), mid, base) << (8 * c); }
  return px;
}
__device__ __forceinline__ void mip_scratch32(unsigned long long *scratch, const MipGeom &G, uint32_t li, uint32_t X, uint32_t Y, const uint32_t *s) {
  if (X >= G.sw || Y >= G.sh) return;
  unsigned long long *d = scratch + (((size_t)li * G.sh + Y) * G.sw + X) * 7;
#pragma unroll
  for (int k = 0; k < 7; k++) d[k] = s[k];
}

// (one copy of lin[] in LDS: a copy per bank, which k_downscale takes at f = 8, and divisions through f32 / f64 reciprocals were measured
// slower or no faster here - profiles/r17_mipmaps.json)
__global__ void __launch_bounds__(MIP_BLOCK) k_mip_tiles(const uint8_t *const *layers, uint8_t *out, unsigned long long *scratch, const uint32_t *tables, MipGeom G) {
  __shared__ uint32_t s_lin[256], s_mid[256], s_base32[1024];
  __shared__ uint32_t s_3[7][256];                       // the tile's 16 x 16 level-3 sums (n = 64: 32 bits)
  __shared__ unsigned long long s_up[7][64 + 16 + 4];     // its 8 x 8 level-4, 4 x 4 level-5 and 2 x 2 level-6 sums
  for (uint32_t k = threadIdx.x; k < 256u; k += MIP_BLOCK) { s_lin[k] = tables[k]; s_mid[k] = tables[256u + k]; }
  for (uint32_t k = threadIdx.x; k < 1024u; k += MIP_BLOCK) s_base32[k] = tables[512u + k];
  __syncthreads();
  const uint8_t *s_base = reinterpret_cast<const uint8_t *>(s_base32);
  const uint32_t tid = threadIdx.x, tx = tid & 15u, ty = tid >> 4;
  const uint32_t per = G.tiles_x * G.tiles_y, li = blockIdx.x / per, tile = blockIdx.x % per, tX = tile % G.tiles_x, tY = tile / G.tiles_x;
  const uint32_t gx = tX * 16u + tx, gy = tY * 16u + ty, x0 = gx * 8u, y0 = gy * 8u;      // this thread's 8 x 8 box = texel (gx, gy) of level 3
  const uint8_t *src8 = layers[li];
  const uint32_t *src = reinterpret_cast<const uint32_t *>(src8);
  const uint32_t W = G.W, H = G.H;
  uint32_t s3[7] = { 0, 0, 0, 0, 0, 0, 0 };
  if (li < G.n_layers && x0 < W && y0 < H) {
    const bool wide = (((uintptr_t)src8 & 15) == 0) && (W & 3u) == 0 && x0 + 8u <= W;
    uint32_t s2[2][7];
    for (uint32_t rp = 0; rp < 4u; rp++) {                 // two rows of the box: one row of level 1
      uint32_t s1[4][7];
#pragma unroll
      for (int j = 0; j < 4; j++) for (int k = 0; k < 7; k++) s1[j][k] = 0;
      if ((rp & 1u) == 0) { for (int j = 0; j < 2; j++) for (int k = 0; k < 7; k++) s2[j][k] = 0; }
      for (uint32_t r = 0; r < 2u; r++) {
        const uint32_t y = y0 + 2u * rp + r;
        if (y >= H) continue;
        const uint32_t *row = src + (size_t)y * W + x0;
        uint32_t p[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
        if (wide) {
          const uint4 v0 = reinterpret_cast<const uint4 *>(row)[0], v1 = reinterpret_cast<const uint4 *>(row)[1];
          p[0] = v0.x; p[1] = v0.y; p[2] = v0.z; p[3] = v0.w; p[4] = v1.x; p[5] = v1.y; p[6] = v1.z; p[7] = v1.w;
        } else {
#pragma unroll
          for (int c = 0; c < 8; c++) if (x0 + (uint32_t)c < W) p[c] = row[c];
        }
#pragma unroll
        for (int c = 0; c < 8; c++) {
          if (x0 + (uint32_t)c >= W) continue;
          const uint32_t a = p[c] >> 24, lr = s_lin[p[c] & 255u], lg = s_lin[(p[c] >> 8) & 255u], lb = s_lin[(p[c] >> 16) & 255u];
          uint32_t *s = s1[c >> 1];
          s[0] += a; s[1] += lr * a; s[2] += lg * a; s[3] += lb * a; s[4] += lr; s[5] += lg; s[6] += lb;
          if (G.u == 0) { const uint32_t t[7] = { a, lr * a, lg * a, lb * a, lr, lg, lb }; mip_scratch32(scratch, G, li, x0 + (uint32_t)c, y, t); }
        }
      }
      if (G.la >= 1u) {
        const uint32_t X1 = gx * 4u, Y1 = gy * 4u + rp, lw = G.lw[1];
        if (Y1 < G.lh[1] && X1 < lw) {
          uint32_t o[4];
#pragma unroll
          for (int j = 0; j < 4; j++) o[j] = mip_texel32(s1[j], 2u, s_mid, s_base);
          uint32_t *d = reinterpret_cast<uint32_t *>(out + G.off[1] + (size_t)li * lw * G.lh[1] * 4) + (size_t)Y1 * lw + X1;
          if ((((uintptr_t)d & 15) == 0) && X1 + 4u <= lw) *reinterpret_cast<uint4 *>(d) = make_uint4(o[0], o[1], o[2], o[3]);
          else {
#pragma unroll
            for (int j = 0; j < 4; j++) if (X1 + (uint32_t)j < lw) d[j] = o[j];
          }
        }
        if (G.u == 1u) { for (int j = 0; j < 4; j++) mip_scratch32(scratch, G, li, X1 + (uint32_t)j, Y1, s1[j]); }
      }
#pragma unroll
      for (int j = 0; j < 4; j++) for (int k = 0; k < 7; k++) s2[j >> 1][k] += s1[j][k];
      if (rp & 1u) {                                        // four rows: one row of level 2
        if (G.la >= 2u) {
          const uint32_t X2 = gx * 2u, Y2 = gy * 2u + (rp >> 1), lw = G.lw[2];
          uint32_t *d = reinterpret_cast<uint32_t *>(out + G.off[2] + (size_t)li * lw * G.lh[2] * 4) + (size_t)Y2 * lw + X2;
          for (int j = 0; j < 2; j++) if (Y2 < G.lh[2] && X2 + (uint32_t)j < lw) d[j] = mip_texel32(s2[j], 4u, s_mid, s_base);
          if (G.u == 2u) { for (int j = 0; j < 2; j++) mip_scratch32(scratch, G, li, X2 + (uint32_t)j, Y2, s2[j]); }
        }
#pragma unroll
        for (int k = 0; k < 7; k++) s3[k] += s2[0][k] + s2[1][k];
      }
    }
    if (G.la >= 3u) {
      if (gx < G.lw[3] && gy < G.lh[3])
        reinterpret_cast<uint32_t *>(out + G.off[3] + (size_t)li * G.lw[3] * G.lh[3] * 4)[(size_t)gy * G.lw[3] + gx] = mip_texel32(s3, 6u, s_mid, s_base);
      if (G.u == 3u) mip_scratch32(scratch, G, li, gx, gy, s3);
    }
  }
  // levels 4 - 7 of the tile from the 16 x 16 level-3 sums (a box outside the image holds zeros); G.la is the same for every thread
  for (int k = 0; k < 7; k++) s_3[k][tid] = s3[k];
  __syncthreads();
  for (uint32_t lv = 4u; lv <= G.la; lv++) {
    const uint32_t side = 128u >> lv, ps = 2u * side;      // boxes per tile side at this level and at the one before
    const uint32_t in_at = lv == 5u ? 0u : 64u + (lv == 7u ? 16u : 0u), out_at = lv == 4u ? 0u : (lv == 5u ? 64u : 80u);      // places in s_up
    if (tid < side * side) {
      const uint32_t cx = tid % side, cy = tid / side, i0 = (2u * cy) * ps + 2u * cx;
      unsigned long long s[7];
      for (int k = 0; k < 7; k++) {
        if (lv == 4u) s[k] = (unsigned long long)s_3[k][i0] + s_3[k][i0 + 1u] + s_3[k][i0 + ps] + s_3[k][i0 + ps + 1u];
        else { const unsigned long long *pv = s_up[k] + in_at; s[k] = pv[i0] + pv[i0 + 1u] + pv[i0 + ps] + pv[i0 + ps + 1u]; }
      }
      const uint32_t X = tX * side + cx, Y = tY * side + cy;
      if (li < G.n_layers && X < G.lw[lv] && Y < G.lh[lv]) {
        reinterpret_cast<uint32_t *>(out + G.off[lv] + (size_t)li * G.lw[lv] * G.lh[lv] * 4)[(size_t)Y * G.lw[lv] + X] = mip_texel64(s, 1ull << (2u * lv), s_mid, s_base);
        if (G.u == lv && X < G.sw && Y < G.sh) { unsigned long long *d = scratch + (((size_t)li * G.sh + Y) * G.sw + X) * 7; for (int k = 0; k < 7; k++) d[k] = s[k]; }
      }
      if (lv < 7u) for (int k = 0; k < 7; k++) s_up[k][out_at + tid] = s[k];
    }
    __syncthreads();
  }
}

// one level from sums: output texel (X, Y) of layer li = the bx x by entries of its box in an array of sw x sh entries per layer (the scratch
// of k_mip_tiles, or the sums an earlier launch of this kernel left in sums_out), n = fx fy texels of level 0; one thread per texel
__global__ void __launch_bounds__(MIP_BLOCK) k_mip_tail(const unsigned long long *sums, uint32_t sw, uint32_t sh, uint8_t *out_level, unsigned long long *sums_out,
                                                         uint32_t lw, uint32_t lh, uint32_t bx, uint32_t by, unsigned long long n, uint32_t n_layers, const uint32_t *tables) {
  __shared__ uint32_t s_mid[256], s_base32[1024];
  for (uint32_t k = threadIdx.x; k < 256u; k += MIP_BLOCK) s_mid[k] = tables[256u + k];
  for (uint32_t k = threadIdx.x; k < 1024u; k += MIP_BLOCK) s_base32[k] = tables[512u + k];
  __syncthreads();
  const unsigned long long items = (unsigned long long)n_layers * lw * lh, it = (unsigned long long)blockIdx.x * MIP_BLOCK + threadIdx.x;
  if (it >= items) return;                                 // (after the only __syncthreads)
  const uint32_t X = (uint32_t)(it % lw), Y = (uint32_t)((it / lw) % lh), li = (uint32_t)(it / ((unsigned long long)lw * lh));
  unsigned long long s[7] = { 0, 0, 0, 0, 0, 0, 0 };
  for (uint32_t y = Y * by; y < Y * by + by && y < sh; y++)
    for (uint32_t x = X * bx; x < X * bx + bx && x < sw; x++) {
      const unsigned long long *e = sums + (((size_t)li * sh + y) * sw + x) * 7;
      for (int k = 0; k < 7; k++) s[k] += e[k];
    }
  for (int k = 0; k < 7; k++) sums_out[it * 7 + k] = s[k];
  reinterpret_cast<uint32_t *>(out_level)[it] = mip_texel64(s, n, s_mid, reinterpret_cast<const uint8_t *>(s_base32));
}

// ================================================================================================
// host side
// ================================================================================================
// out[0] / out[1]: the chain slots of uvol_mipchain_rgba_batch_dev; out[2]: the slot uvol_encode_texture_segments_mips keeps for itself
struct MipState { uvol_devbuf out[3], in, ptrs, tables, scratch; bool tables_up = false; std::vector<const uint8_t *> hptrs; uint32_t htab[DOWN_TABLE_WORDS]; };

void mip_destroy(uvol_ctx *ctx) {
  MipState *S = ctx->mip; if (!S) return;
  for (uvol_devbuf *b : { &S->out[0], &S->out[1], &S->out[2], &S->in, &S->ptrs, &S->tables, &S->scratch }) if (b->p) (void)hipFree(b->p);
  delete S; ctx->mip = nullptr;
}
void mip_trim(uvol_ctx *ctx) {
  MipState *S = ctx->mip; if (!S) return;
  for (uvol_devbuf *b : { &S->out[0], &S->out[1], &S->out[2], &S->in, &S->ptrs, &S->scratch }) if (b->p) { (void)hipFree(b->p); b->p = nullptr; b->cap = 0; }
}
int mip_level_count(uint32_t w, uint32_t h) {
  uint32_t m = w > h ? w : h; int k = 0;
  while (m) { k++; m >>= 1; }
  return k;                                                // floor(log2(max(w, h))) + 1; 0 for an empty image
}
static inline uint32_t mip_ctz(uint32_t v) { uint32_t k = 0; while (k < 32 && !((v >> k) & 1u)) k++; return k; }

// The arguments of a chain call, checked before anything runs (who: the entry point's name in the messages).  levels: 0 = the full chain;
// *levels_out = the resolved count.
int mip_check(uvol_ctx *ctx, const char *who, uint32_t w, uint32_t h, int levels, int *levels_out) {
  if (!w || !h || w > 8192 || h > 16384) { ctx->set_error("%s: width %u x height %u (1 x 1 up to 8192 x 16384)", who, w, h); return UVOL_E_INVALID; }
  const int full = mip_level_count(w, h);
  if (levels < 0 || levels > full) { ctx->set_error("%s: levels %d (0 = the full chain, or 1 .. %d for %u x %u)", who, levels, full, w, h); return UVOL_E_INVALID; }
  const int nl = levels ? levels : full;
  for (int v = 1; v < nl; v++) {
    const uint32_t lw = std::max(1u, w >> v), lh = std::max(1u, h >> v);
    if (w % lw || h % lh) { ctx->set_error("%s: level %d of %u x %u is %u x %u, and width / level width, height / level height must be integers", who, v, w, h, lw, lh); return UVOL_E_INVALID; }
  }
  *levels_out = nl;
  return UVOL_OK;
}

// n layers of w x h RGBA8 (device pointers, or host memory uploaded through the staging buffers) -> rgba_dev_out[i * (levels - 1) + v - 1] =
// level v of layer i in chain slot `slot`.  Level v of all layers is one contiguous run, layer after layer (what a batch of encoder jobs reads),
// runs start 256-byte aligned.  Enqueued on the context's stream behind the un-filter of any ingest slot the layers lie in; `wait`: returns
// when the levels are complete.
int mip_rgba_batch(uvol_ctx *ctx, const char *who, const uint8_t *const *rgba, int n, uint32_t w, uint32_t h, bool inputs_on_device, int levels, int slot, const uint8_t **rgba_dev_out, bool wait) {
  if (n <= 0) return UVOL_OK;
  int nl = 0, rc;
  if ((rc = mip_check(ctx, who, w, h, levels, &nl))) return rc;
  if (slot < 0 || slot > 2) { ctx->set_error("%s: slot %d (0 or 1)", who, slot); return UVOL_E_INVALID; }
  for (int i = 0; i < n; i++) {
    if (!rgba[i]) { ctx->set_error("%s: rgba[%d] is NULL", who, i); return UVOL_E_INVALID; }
    if (inputs_on_device && ((uintptr_t)rgba[i] & 3)) { ctx->set_error("%s: rgba[%d] is a device layer that is not 4-byte aligned", who, i); return UVOL_E_INVALID; }
  }
  if (nl == 1) return UVOL_OK;
  if (!ctx->mip) ctx->mip = new MipState();
  MipState *S = ctx->mip;
  // geometry of every level; which levels the tile kernel makes (la) and from which level's sums the others are made (u)
  uint32_t lw[MIP_MAX_LEVELS], lh[MIP_MAX_LEVELS]; size_t off[MIP_MAX_LEVELS]; size_t total = 0;
  for (int v = 1; v < nl; v++) { lw[v] = std::max(1u, w >> v); lh[v] = std::max(1u, h >> v); off[v] = total; total += ((size_t)lw[v] * lh[v] * 4 * (size_t)n + 255) & ~(size_t)255; }
  MipGeom G; memset(&G, 0, sizeof G);
  G.W = w; G.H = h; G.n_layers = (uint32_t)n; G.tiles_x = (w + MIP_TILE - 1) / MIP_TILE; G.tiles_y = (h + MIP_TILE - 1) / MIP_TILE;
  G.la = std::min(std::min(mip_ctz(w), mip_ctz(h)), std::min((uint32_t)(nl - 1), MIP_TILE_LEVELS));
  G.u = MIP_NO_SCRATCH;
  if ((int)G.la < nl - 1) {
    uint32_t u = G.la;
    for (int v = (int)G.la + 1; v < nl; v++) u = std::min(u, std::min(mip_ctz(w / lw[v]), mip_ctz(h / lh[v])));
    G.u = u; G.sw = w >> u; G.sh = h >> u;                 // (2^u divides w and h: u <= la)
  }
  for (uint32_t v = 1; v <= G.la; v++) { G.lw[v] = lw[v]; G.lh[v] = lh[v]; G.off[v] = off[v]; }
  const size_t ibytes = (size_t)w * h * 4;
  if ((rc = uvol_ensure(ctx, S->out[slot], total))) return rc;
  if ((rc = uvol_ensure(ctx, S->ptrs, sizeof(uint8_t *) * (size_t)n))) return rc;
  if ((rc = uvol_ensure(ctx, S->tables, sizeof S->htab))) return rc;
  // scratch: the level-u sums of k_mip_tiles, then the sums of every level k_mip_tail makes (56 bytes per entry)
  size_t soff[MIP_MAX_LEVELS], stotal = G.u != MIP_NO_SCRATCH ? (size_t)G.sw * G.sh * 7 * (size_t)n : 0;
  for (int v = (int)G.la + 1; v < nl; v++) { soff[v] = stotal; stotal += (size_t)lw[v] * lh[v] * 7 * (size_t)n; }
  if (stotal && (rc = uvol_ensure(ctx, S->scratch, stotal * 8))) return rc;
  if (!S->tables_up) {
    if (!down_tables(S->htab)) { ctx->set_error("%s: the inverse table's bucket search disagrees with the plain search", who); return UVOL_E_HIP; }
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
    uvol_ctx::Scope sc(ctx, "ingest.mipchain_upload", (uint64_t)ibytes * n);
    if ((rc = uvol_upload_staged(ctx, (uint8_t *)S->in.p, ups))) return rc;
  }
  UVOL_HIP_CHECK(ctx, hipMemcpyAsync(S->ptrs.p, S->hptrs.data(), sizeof(uint8_t *) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
  const uint32_t *tp = (const uint32_t *)S->tables.p; uint8_t *op = (uint8_t *)S->out[slot].p; unsigned long long *sp = (unsigned long long *)S->scratch.p;
  { uvol_ctx::Scope sc(ctx, "ingest.mipchain", (uint64_t)ibytes * n + (uint64_t)total);
    if (uvol_debug()) { fprintf(stderr, "[uvol] launch k_mip_tiles %d layers %u x %u, %d levels (tile levels 1 .. %u, scratch level %d)\n", n, w, h, nl, G.la, G.u == MIP_NO_SCRATCH ? -1 : (int)G.u); fflush(stderr); }
    const unsigned long long wgs = (unsigned long long)G.tiles_x * G.tiles_y * (unsigned long long)n;      // <= 64 x 128 tiles x n
    if (wgs > 0x7fffffffull) { ctx->set_error("%s: %d layers of %u x %u are more tiles than one launch takes", who, n, w, h); return UVOL_E_INVALID; }
    hipLaunchKernelGGL(k_mip_tiles, dim3((unsigned)wgs), dim3(MIP_BLOCK), 0, ctx->stream, (const uint8_t *const *)S->ptrs.p, op, sp, tp, G);
    UVOL_HIP_CHECK(ctx, hipGetLastError());
    // a level is made from the sums of the level before when that level's boxes tile its own (4 entries per texel for powers of two), else from
    // the level-u sums
    uint32_t src_fx = 1u << G.u, src_fy = 1u << G.u, src_w = G.sw, src_h = G.sh; const unsigned long long *srcp = sp;
    for (int v = (int)G.la + 1; v < nl; v++) {
      const uint32_t fx = w / lw[v], fy = h / lh[v];
      if (fx % src_fx || fy % src_fy) { src_fx = src_fy = 1u << G.u; src_w = G.sw; src_h = G.sh; srcp = sp; }
      const unsigned long long items = (unsigned long long)n * lw[v] * lh[v];
      hipLaunchKernelGGL(k_mip_tail, dim3((unsigned)((items + MIP_BLOCK - 1) / MIP_BLOCK)), dim3(MIP_BLOCK), 0, ctx->stream, srcp, src_w, src_h, op + off[v], sp + soff[v],
                         lw[v], lh[v], fx / src_fx, fy / src_fy, (unsigned long long)fx * fy, (uint32_t)n, tp);
      UVOL_HIP_CHECK(ctx, hipGetLastError());
      src_fx = fx; src_fy = fy; src_w = lw[v]; src_h = lh[v]; srcp = sp + soff[v];
    }
  }
  for (int i = 0; i < n; i++) for (int v = 1; v < nl; v++) rgba_dev_out[(size_t)i * (nl - 1) + (v - 1)] = op + off[v] + (size_t)lw[v] * lh[v] * 4 * (size_t)i;
  if (wait) UVOL_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return UVOL_OK;
}
