// tex_blocks.hpp — the block formats of the texture targets, each rule stated once: ETC1 (tables, expansions, pixel indices, planes), the
// ETC1 re-pack of an ETC1S block, EAC alpha, BC4, BC1, the BC7 weights and 128-bit writer, the RGBA row store.  Plain device functions and
// constants: no job structs, no host code.  tests/transcode_ref.py has the same factoring in NumPy (etc1_repack, eac_fit, eac_pack, bc4_fit,
// bc1_fit); K is the number of distinct values a block is fitted to: 4 (the colours / levels of an ETC1S block, texels follow their
// selectors) or 16 (the texels of a decoded UASTC block).
//
// Conventions: a texel is R | G << 8 | B << 16 | A << 24; texels of a block in raster order, i = 4 y + x; an ETC1S selector word holds
// texel (x, y) at bits 8 y + 2 x = 2 i.  Searches run ascending and keep the FIRST best.  Blocks leave through byte stores unless the
// caller knows more about its output's alignment.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

// ---- ETC1 ----
__device__ __forceinline__ int t_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ int t_expand5(int c) { return (c << 3) | (c >> 2); }
__device__ __forceinline__ int t_inten(int t, int s) {
  // g_etc1_inten_tables, linear selector order low -> high
  const int hi_[8] = { 8, 17, 29, 42, 60, 80, 106, 183 }, lo_[8] = { 2, 5, 9, 13, 18, 24, 33, 47 };
  const int m = (s == 0 || s == 3) ? hi_[t] : lo_[t];
  return s < 2 ? -m : m;
}
__device__ __forceinline__ int t_expand4(int c) { return c * 17; }
// The small / large magnitude of table t for everything but the ETC1S encoder (whose t_inten above keeps its text): lo_ / hi_ as the bytes
// of one word each, so that a look-up is a shift and no load - the transcode kernels are latency-bound behind the endpoint they fetched.
__device__ __forceinline__ int etc1_mag_s(int t) { return (int)((0x2F2118120D090502ull >> (8 * t)) & 255u); }      // 2, 5, 9, 13, 18, 24, 33, 47 (lo_)
__device__ __forceinline__ int etc1_mag_l(int t) { return (int)((0xB76A503C2A1D1108ull >> (8 * t)) & 255u); }      // 8, 17, 29, 42, 60, 80, 106, 183 (hi_)
// the four modifiers of table t in ETC1S selector order, dark -> bright: -large, -small, +small, +large
__device__ __forceinline__ void etc1s_mods(int t, int mod[4]) { const int S = etc1_mag_s(t), L = etc1_mag_l(t); mod[0] = -L; mod[1] = -S; mod[2] = S; mod[3] = L; }
// the modifier of ETC1 pixel index 0 .. 3 of a table with magnitudes S, L: +small, +large, -small, -large
__device__ __forceinline__ int etc1_mod(int S, int L, uint32_t idx) { const int m = (idx & 1u) ? L : S; return (idx & 2u) ? -m : m; }
// ETC1S selector 0 .. 3 (dark -> bright) -> ETC1 pixel index
__device__ __forceinline__ uint32_t etc1_sel_index(uint32_t s) { return s == 0 ? 3u : (s == 1 ? 2u : (s == 2 ? 0u : 1u)); }
// the pixel index of texel (x, y) goes to bit 4 x + y of the msb and lsb planes (16 bits each)
__device__ __forceinline__ void etc1_plane_put(uint32_t &msb, uint32_t &lsb, int x, int y, uint32_t idx) { const int i = 4 * x + y; msb |= (idx >> 1) << i; lsb |= (idx & 1u) << i; }
// Block bytes: R, G, B (differential: base5 << 3 | delta3, individual: base4 << 4 | base4), table1 << 5 | table2 << 2 | diff << 1 | flip,
// then the msb and the lsb plane, big-endian.  -> the block's two words in memory order; hdr = bytes 0 .. 3, byte 0 in the low bits
__device__ __forceinline__ uint32_t etc1_header(uint32_t b0, uint32_t b1, uint32_t b2, uint32_t b3) { return (b0 & 255u) | ((b1 & 255u) << 8) | ((b2 & 255u) << 16) | ((b3 & 255u) << 24); }
__device__ __forceinline__ uint2 etc1_words(uint32_t hdr, uint32_t msb, uint32_t lsb) { return make_uint2(hdr, (msb >> 8) | ((msb & 255u) << 8) | ((lsb >> 8) << 16) | ((lsb & 255u) << 24)); }
__device__ __forceinline__ void t_store_le32(uint8_t *out, uint32_t w) { out[0] = (uint8_t)w; out[1] = (uint8_t)(w >> 8); out[2] = (uint8_t)(w >> 16); out[3] = (uint8_t)(w >> 24); }
__device__ __forceinline__ void etc1_store(uint8_t *out, uint2 w) { t_store_le32(out, w.x); t_store_le32(out + 4, w.y); }

// Every ETC1S block IS an ETC1 block - differential mode with a zero delta, both sub-blocks on the same intensity table, no flip - so its
// transcode is a re-pack of (colour5, table, selectors); a differential block with zero deltas is also a valid ETC2 block.  e = r5 g5 b5 table
__device__ __forceinline__ uint2 etc1_repack(const uint8_t *e, uint32_t sel) {
  uint32_t msb = 0, lsb = 0;
  for (int y = 0; y < 4; y++) for (int x = 0; x < 4; x++) etc1_plane_put(msb, lsb, x, y, etc1_sel_index((sel >> (8 * y + 2 * x)) & 3u));
  const uint32_t t = e[3];
  return etc1_words(etc1_header((uint32_t)e[0] << 3, (uint32_t)e[1] << 3, (uint32_t)e[2] << 3, (t << 5) | (t << 2) | 2u), msb, lsb);
}

// ---- EAC alpha (the alpha half of ETC2 RGBA8) ----
// eight levels clamp(base + multiplier * table[j]) out of 16 tables
__device__ const int8_t EAC_MOD[16][8] = {
  { -3, -6, -9, -15, 2, 5, 8, 14 }, { -3, -7, -10, -13, 2, 6, 9, 12 }, { -2, -5, -8, -13, 1, 4, 7, 12 }, { -2, -4, -6, -13, 1, 3, 5, 12 },
  { -3, -6, -8, -12, 2, 5, 7, 11 }, { -3, -7, -9, -11, 2, 6, 8, 10 }, { -4, -7, -8, -11, 3, 6, 7, 10 }, { -3, -5, -8, -11, 2, 4, 7, 10 },
  { -2, -6, -8, -10, 1, 5, 7, 9 }, { -2, -5, -8, -10, 1, 4, 7, 9 }, { -2, -4, -8, -10, 1, 3, 7, 9 }, { -2, -5, -7, -10, 1, 4, 6, 9 },
  { -3, -4, -7, -10, 2, 3, 6, 9 }, { -1, -2, -3, -10, 0, 1, 2, 9 }, { -4, -6, -8, -9, 3, 5, 7, 8 }, { -3, -5, -7, -9, 2, 4, 6, 8 } };
__device__ __forceinline__ int eac_level(int base, int mul, int t, int j) { return t_clampi(base + mul * EAC_MOD[t][j], 0, 255); }
// the first nearest of the eight levels of (base, mul, t)
__device__ __forceinline__ uint32_t eac_nearest(int base, int mul, int t, int a) {
  int be = 1 << 30; uint32_t bj = 0;
  for (int j = 0; j < 8; j++) { const int d = eac_level(base, mul, t, j) - a; if (d * d < be) { be = d * d; bj = (uint32_t)j; } }
  return bj;
}
// The search: level(k), k < K, is carried by weight(k) texels (0: unused; callables, so that a caller's values stay where they are).  Every (table 0 .. 15, multiplier 1 .. 15) is tried with the five
// bases mid - 2 .. mid + 2 inside 0 .. 255, mid = (lowest + highest used level + 1) >> 1; the error is the weighted sum of the squared
// distances to the nearest level; the first best wins and an error of 0 ends the search.  (A sum that has reached the best so far is
// dropped early: it cannot win.)  shortcut: one used value takes (table 13 - it has a zero modifier -, multiplier 1, base = the value)
// without a search.  Not a restatement of the basis transcoder's table-driven path (its tables are not in the reference).
template <int K, typename LV, typename WT>
__device__ inline void eac_fit(LV level, WT weight, bool shortcut, int &bb, int &bm, int &bt) {
  int lo = 255, hi = 0;
  for (int k = 0; k < K; k++) if (weight(k)) { const int v = level(k); lo = v < lo ? v : lo; hi = v > hi ? v : hi; }
  if (shortcut && lo == hi) { bt = 13; bm = 1; bb = hi; return; }
  const int mid = (lo + hi + 1) >> 1;
  uint32_t best = 0xffffffffu; bt = 0; bm = 1; bb = mid;
  for (int t = 0; t < 16 && best; t++) for (int m = 1; m < 16 && best; m++) for (int db = -2; db <= 2; db++) {
    const int base = mid + db; if (base < 0 || base > 255) continue;
    int lv[8]; for (int j = 0; j < 8; j++) lv[j] = eac_level(base, m, t, j);
    uint32_t err = 0;
    for (int k = 0; k < K && err < best; k++) if (weight(k)) {
      int be = 1 << 30;
      for (int j = 0; j < 8; j++) { const int d = lv[j] - level(k); be = d * d < be ? d * d : be; }
      err += weight(k) * (uint32_t)be;
    }
    if (err < best) { best = err; bt = t; bm = m; bb = base; }
  }
}
// Block bytes: base, multiplier << 4 | table, then 16 x 3-bit indices, pixel 4 x + y first, in the top bits.  idx(i): the index of texel i
template <typename F>
__device__ __forceinline__ void eac_pack(uint8_t *out, int bb, int bm, int bt, F idx) {
  unsigned long long bits = 0;
  for (int y = 0; y < 4; y++) for (int x = 0; x < 4; x++) bits |= (unsigned long long)idx(4 * y + x) << (45 - 3 * (4 * x + y));
  out[0] = (uint8_t)bb; out[1] = (uint8_t)((bm << 4) | bt);
  for (int k = 0; k < 6; k++) out[2 + k] = (uint8_t)(bits >> (40 - 8 * k));
}

// ---- BC4 (the alpha half of BC3) ----
// eight-value mode: value j = alpha0, alpha1, then ((8 - j) alpha0 + (j - 1) alpha1) / 7
__device__ __forceinline__ int bc4_value(int a0, int a1, int j) { return j == 0 ? a0 : (j == 1 ? a1 : ((8 - j) * a0 + (j - 1) * a1) / 7); }
// alpha0 = the highest, alpha1 = the lowest of the levels level(k), k < K, the block uses (bit k of used); a level takes its first
// nearest value
template <int K, typename LV>
__device__ inline void bc4_fit(LV level, uint32_t used, int &a0, int &a1) {
  a0 = 0; a1 = 255;
  for (int k = 0; k < K; k++) if ((used >> k) & 1u) { const int v = level(k); a0 = v > a0 ? v : a0; a1 = v < a1 ? v : a1; }
}
__device__ __forceinline__ uint32_t bc4_nearest(int a0, int a1, int v) {
  int be = 1 << 30; uint32_t bj = 0;
  for (int j = 0; j < 8; j++) { const int d = bc4_value(a0, a1, j) - v; if (d * d < be) { be = d * d; bj = (uint32_t)j; } }
  return bj;
}
// Block bytes: alpha0, alpha1, 16 x 3-bit indices in raster order from bit 0; equal endpoints: index 0 everywhere (idx is not asked)
template <typename F>
__device__ __forceinline__ void bc4_pack(uint8_t *out, int a0, int a1, F idx) {
  unsigned long long bits = 0;
  if (a0 > a1) for (int i = 0; i < 16; i++) bits |= (unsigned long long)idx(i) << (3 * i);
  out[0] = (uint8_t)a0; out[1] = (uint8_t)a1;
  for (int k = 0; k < 6; k++) out[2 + k] = (uint8_t)(bits >> (8 * k));
}

// ---- BC1 (and the colour half of BC3, which always reads it in four-colour mode) ----
// an 8-bit colour rounded to RGB565 (R in the top 5 bits), and the 565 colour widened by bit replication
__device__ __forceinline__ uint32_t bc1_round565(const int c[3]) { return (uint32_t)((((c[0] * 31 + 127) / 255) << 11) | (((c[1] * 63 + 127) / 255) << 5) | ((c[2] * 31 + 127) / 255)); }
__device__ __forceinline__ void bc1_widen565(uint32_t q, int e[3]) {
  const int r = (int)(q >> 11), g = (int)((q >> 5) & 63u), b = (int)(q & 31u);
  e[0] = (r << 3) | (r >> 2); e[1] = (g << 2) | (g >> 4); e[2] = (b << 3) | (b >> 2);
}
// four-colour palette: c0, c1, (2 c0 + c1) / 3, (c0 + 2 c1) / 3
__device__ __forceinline__ void bc1_palette(uint32_t c0, uint32_t c1, int pal[4][3]) {
  int e0[3], e1[3]; bc1_widen565(c0, e0); bc1_widen565(c1, e1);
  for (int c = 0; c < 3; c++) { pal[0][c] = e0[c]; pal[1][c] = e1[c]; pal[2][c] = (2 * e0[c] + e1[c]) / 3; pal[3][c] = (e0[c] + 2 * e1[c]) / 3; }
}
// hi / lo: the 8-bit colours that become colour0 / colour1; a colour (alpha byte ignored) takes the first nearest palette entry (squared
// error over R, G, B).  An opaque block needs colour0 > colour1 as 16-bit numbers (otherwise index 3 means transparent black):
// colour0 < colour1 swaps the endpoints, indices 0 <-> 1 and 2 <-> 3.
struct Bc1Fit { uint32_t c0, c1, swap; int pal[4][3]; };      // c0 >= c1 as stored; pal and swap: as fitted, before the swap
__device__ inline void bc1_fit(const int hi[3], const int lo[3], Bc1Fit &F) {
  const uint32_t c0 = bc1_round565(hi), c1 = bc1_round565(lo);
  bc1_palette(c0, c1, F.pal);
  F.swap = c0 < c1 ? 1u : 0u; F.c0 = F.swap ? c1 : c0; F.c1 = F.swap ? c0 : c1;
}
__device__ __forceinline__ uint32_t bc1_nearest(const Bc1Fit &F, int r, int g, int b) {
  int be = 1 << 30; uint32_t bj = 0;
  for (int j = 0; j < 4; j++) { const int dr = F.pal[j][0] - r, dg = F.pal[j][1] - g, db = F.pal[j][2] - b, d = dr * dr + dg * dg + db * db; if (d < be) { be = d; bj = (uint32_t)j; } }
  return bj ^ F.swap;
}
// Block bytes: colour0, colour1 (u16 little-endian), 16 x 2-bit indices in raster order from bit 0; colour0 == colour1 uses index 0 only
// (idx is not asked)
template <typename F>
__device__ __forceinline__ void bc1_pack(uint8_t *out, uint32_t c0, uint32_t c1, F idx) {
  uint32_t bits = 0;
  if (c0 != c1) for (int i = 0; i < 16; i++) bits |= idx(i) << (2 * i);
  t_store_le32(out, c0 | (c1 << 16)); t_store_le32(out + 4, bits);
}

// ---- BC7 ----
// interpolation weights of 2-bit and 4-bit indices, and the interpolation itself
__device__ __forceinline__ int bc7_w2(uint32_t k) { const int W[4] = { 0, 21, 43, 64 }; return W[k]; }      // (local tables: they fold into unrolled loops)
__device__ __forceinline__ int bc7_w4(uint32_t k) { const int W[16] = { 0, 4, 9, 13, 17, 21, 26, 30, 34, 38, 43, 47, 51, 55, 60, 64 }; return W[k]; }
__device__ __forceinline__ int bc7_interp(int l, int h, int w) { return (l * (64 - w) + h * w + 32) >> 6; }
// Bit layouts, LSB first, pixels in raster order.  Mode 5: 6 bits (1 << 5); rotation 2; R0 R1 G0 G1 B0 B1, 7 bits each; A0 A1, 8 bits each;
// colour indices 1 + 15 * 2 bits; alpha indices 1 + 15 * 2 bits.  Mode 6: 7 bits (1 << 6); R0 R1 G0 G1 B0 B1 A0 A1, 7 bits each; P0 P1;
// indices 3 + 15 * 4 bits.  Pixel 0's index has its MSB implied 0: otherwise swap the endpoints and complement the indices.

// 128-bit block under construction, LSB first (BC7, UASTC and ASTC blocks): put_raw places x < 2^n, n > 0, at bit o; put takes the low n
// bits of any v and allows n <= 0
struct TBits128 {
  unsigned long long lo, hi;
  __device__ __forceinline__ void put_raw(int &o, unsigned long long x, int n) {
    if (o < 64) { lo |= x << o; if (o + n > 64) hi |= x >> (64 - o); } else hi |= x << (o - 64);
    o += n;
  }
  __device__ __forceinline__ void put(int &o, uint32_t v, int n) { if (n > 0) put_raw(o, (unsigned long long)v & ((1ull << n) - 1ull), n); }
};

// ---- RGBA8 target: the four texels of block column X in one row of a W-texel image (row = that image row's first byte) ----
// one 16-byte store where every block row is whole and aligned with the image's, else the texels inside the image byte by byte
__device__ __forceinline__ void t_store_row4(uint8_t *row, uint32_t W, uint32_t X, const uint32_t px4[4]) {
  if (X * 4 + 3 < W && (W & 3) == 0) *reinterpret_cast<uint4 *>(row + 16 * (size_t)X) = make_uint4(px4[0], px4[1], px4[2], px4[3]);
  else for (int x = 0; x < 4 && 4 * X + (uint32_t)x < W; x++) t_store_le32(row + 4 * (4 * (size_t)X + x), px4[x]);
}
