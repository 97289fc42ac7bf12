// geo_matseam.hpp - K6b: the material attribute of a frame with interior material seams, as a Draco MESH_CORNER_ATTRIBUTE.
// Part of the geometry encoder translation unit: included by geom_encode.hip, in pipeline order (not a standalone header).
// ------------------------------------------------------------------------------------------------
// uvol_params.material_seams.  The ids arrive per face; where two ids meet at a shared vertex (GeoJob::mat_seam, found by k_mat_vert) the
// attribute cannot live on the base table.  Draco then gives it a corner table of its own: the base table with the edges between faces of
// different ids cut (MeshAttributeCornerTable), one attribute vertex per fan segment between two cuts, a seam-bit stream, a depth-first
// traversal of that table from the decoder-order component starts, and the parallelogram predictor on it.
//
// This is the "third slot" form with storage of its own (GeoJob::ms): the packed two-slot arrays the hot kernels read (fseam, sbpack, the
// record tables) are not widened, and the pass is a short launch sequence of its own BEHIND the main traversals, between k_mat_vert and
// k_stream_setup.  The host launches it only for a group that may need it (ms.on frames whose input ids are not all equal - known from the
// look the host takes at the group anyway, k_coherence); every kernel leaves at once for a frame without a seam, so the material traversal
// of such a frame does not run and its bytes are the vertex-attribute form's.
//
// The traversal runs one lane per frame over 24-byte face records of its own (k_ms_pack): a frame with material seams pays one more
// serial walk of its faces.
// ------------------------------------------------------------------------------------------------
#define MS_LIVE(J) ((J).status == 0 && (J).ms.on && (J).mat_seam)
__device__ __forceinline__ bool ms_fseam_bit(const GeoJob &J, int c) { return (J.ms.fseam[c / 3] >> (c % 3)) & 1u; }
__device__ __forceinline__ int ms_opp(const GeoJob &J, int c) { return (c < 0 || ms_fseam_bit(J, c)) ? GEO_INV : J.opp[c]; }
__device__ __forceinline__ bool ms_touched(const GeoJob &J, uint32_t v) { return (J.ms.vseam[v >> 5] >> (v & 31)) & 1u; }
// vertex of corner c in the material's table: the base vertex unless a material seam touches it
__device__ __forceinline__ int ms_vertex(const GeoJob &J, int c) { const int v = geo_vt(J)[c]; return ms_touched(J, (uint32_t)v) ? J.ms.avert[c] : v; }

// One thread per stored face: the seam flags across its three edges (a boundary counts as a seam; an interior edge is one when the two
// faces carry different ids) and the 'a material seam touches this vertex' bits, as k_seams does for value ids.
__global__ void __launch_bounds__(UVOL_BLOCK) k_ms_flags(GeoJob *jobs) {
  GeoJob &J = jobs[blockIdx.y];
  if (!MS_LIVE(J)) return;
  const uint32_t f = blockIdx.x * UVOL_BLOCK + threadIdx.x;
  if (f >= J.nf) return;
  const uvol_s3 o3 = *reinterpret_cast<const uvol_s3 *>(J.opp + 3 * (size_t)f);
  const int opp_[3] = { o3.x, o3.y, o3.z };
  const uint32_t own = J.fmat[f];
  uint32_t bits = 0;
  for (int k = 0; k < 3; k++) {
    uint32_t sm = 1;
    if (opp_[k] >= 0) {
      sm = J.fmat[opp_[k] / 3] != own ? 1u : 0u;
      if (sm) {                                                           // both ends of the edge get split
        const uint32_t va = (uint32_t)geo_vt(J)[3 * f + (k + 1) % 3], vb = (uint32_t)geo_vt(J)[3 * f + (k + 2) % 3];
        atomicOr(&J.ms.vseam[va >> 5], 1u << (va & 31)); atomicOr(&J.ms.vseam[vb >> 5], 1u << (vb & 31));
      }
    }
    bits |= sm << k;
  }
  J.ms.fseam[f] = (uint8_t)bits;
}
// seam bits, pass 1 (k_sb_count's rule and order): one thread per DECODER-order face, the edges whose neighbour has the higher decoder
// index, in the decoder's corner rotation; one byte per face and the block sums for k_scan_sums(SCAN_ELIG)
__global__ void __launch_bounds__(UVOL_BLOCK) k_ms_sb_count(GeoJob *jobs) {
  GeoJob &J = jobs[blockIdx.y];
  { __shared__ int live_; if (threadIdx.x == 0) live_ = MS_LIVE(J) ? 1 : 0; __syncthreads(); if (!live_) return; }
  const uint32_t f = blockIdx.x * UVOL_BLOCK + threadIdx.x;
  uint32_t cnt = 0;
  if (f < J.nf) {
    const int x0 = J.tstart[f], fo = x0 >> 2, r0 = x0 & 3;
    const uvol_s3 o3 = *reinterpret_cast<const uvol_s3 *>(J.opp + 3 * (size_t)fo);
    const int opp_[3] = { o3.x, o3.y, o3.z };
    const uint32_t fs = J.ms.fseam[fo];
    uint32_t b0 = 0;
    for (int k = 0; k < 3; k++) {
      const int j = (r0 + k) % 3;
      if (opp_[j] < 0) continue;
      const int t = J.face_time[opp_[j] / 3], df = t >= 0 ? J.nsym - 1 - t : J.nsym + (-t - 2);
      if ((uint32_t)df <= f) continue;
      b0 |= ((fs >> j) & 1u) << cnt; cnt++;
    }
    J.ms.sbpack[f] = (uint8_t)(cnt | (b0 << 2));
  }
  const uint32_t tot = block_sum(cnt);
  if (threadIdx.x == 0 && blockIdx.x < uvol_blocks_dev(J.nf)) J.bsum[blockIdx.x] = tot;
}
// pass 2 (after k_scan_sums over SCAN_ELIG): the bits at their places, the zero count for the rabs coder, and the stream's array
__global__ void __launch_bounds__(UVOL_BLOCK) k_ms_sb_write(GeoJob *jobs) {
  GeoJob &J = jobs[blockIdx.y];
  __shared__ int live_; __shared__ uint32_t zc;
  if (threadIdx.x == 0) { live_ = MS_LIVE(J) ? 1 : 0; zc = 0; }
  __syncthreads();
  if (!live_) return;
  const uint32_t nf = J.nf, f = blockIdx.x * UVOL_BLOCK + threadIdx.x;
  const uint32_t pk = f < nf ? J.ms.sbpack[f] : 0u, cnt = pk & 3u;
  uint32_t tot;
  const uint32_t pos = block_excl_scan(cnt, &tot) + (blockIdx.x <= uvol_blocks_dev(nf) ? J.bsum[blockIdx.x] : 0);
  if (cnt) {
    const uint32_t b = pk >> 2; uint32_t z = 0;
    for (uint32_t k = 0; k < cnt; k++) { const uint8_t sb = (uint8_t)((b >> k) & 1u); J.ms.sbits[pos + k] = sb; z += sb ? 0u : 1u; }
    if (z) atomicAdd(&zc, z);
  }
  __syncthreads();
  if (threadIdx.x == 0 && zc) atomicAdd(&J.rb[GEO_RB_MAT].zeros, zc);
  if (blockIdx.x == 0 && threadIdx.x == 0) { J.rb[GEO_RB_MAT].n = J.bsum[uvol_blocks_dev(nf)]; J.rb[GEO_RB_MAT].bits = J.ms.sbits; }
}
// attribute vertices of the touched vertices (k_aseg's rule and its segment walk, aseg_fill).  Pass 0, one thread per stored face: every
// flagged edge whose left end a material seam touches starts a segment - maximal run of fan corners no seam or boundary separates - which
// gets an id nverts_base + k and is walked rightwards.  Pass 1, one thread per frame: the size of the table's vertex id space.
__global__ void __launch_bounds__(UVOL_BLOCK) k_ms_aseg(GeoJob *jobs, int pass) {
  GeoJob &J = jobs[blockIdx.y];
  if (!MS_LIVE(J)) return;
  const uint32_t f = blockIdx.x * UVOL_BLOCK + threadIdx.x;
  if (pass == 1) {
    if (f == 0) { const uint32_t tot = J.nverts_t[0] + J.ms.nseg; J.ms.nverts = tot; if (tot > J.ecap) J.status = GEO_E_WS_OVERFLOW; }
    return;
  }
  if (f >= J.nf) return;
  const uint8_t *const fseam = J.ms.fseam;
  const uint32_t fs = fseam[f];
  if (!fs) return;
  const int32_t *const opp = J.opp, *const vt = geo_vt(J);
  int32_t *const avert = J.ms.avert;
  const uint32_t nc = J.nc, nbase = J.nverts_t[0];
  for (int k = 0; k < 3; k++) {
    if (!((fs >> k) & 1u)) continue;
    const int c = g_prv(3 * (int)f + k);
    if (!ms_touched(J, (uint32_t)vt[c])) continue;
    const int32_t id = (int32_t)(nbase + atomicAdd(&J.ms.nseg, 1u));
    const bool ok = aseg_fill(avert, c, id, nc, [=](int p) {
      const uint32_t fb = fseam[p / 3]; const int o = opp[p];
      return ((fb >> (p % 3)) & 1u) ? GEO_INV : o; });
    if (!ok) { J.status = -22; return; }
  }
}
// Records of the material's table for the serial traverser and what follows it, one thread per stored face: avert[] becomes, for EVERY
// corner, attribute vertex << 1 | open (in place: a thread reads only the entries it writes), ropp[] the opposite corner through the
// seam-cut table.  A vertex of this table is open when a seam touches it (its segments end at seams) or when it is on the mesh boundary.
// The traverser then needs two 12-byte loads per face instead of a chain through opp / seam flags / touched bits / attribute vertices.
__global__ void __launch_bounds__(UVOL_BLOCK) k_ms_pack(GeoJob *jobs) {
  GeoJob &J = jobs[blockIdx.y];
  if (!MS_LIVE(J)) return;
  const uint32_t f = blockIdx.x * UVOL_BLOCK + threadIdx.x;
  if (f >= J.nf) return;
  const uint32_t nbase = J.nverts_t[0], fs = J.ms.fseam[f];
  const uvol_s3 o3 = *reinterpret_cast<const uvol_s3 *>(J.opp + 3 * (size_t)f);
  const int oo[3] = { o3.x, o3.y, o3.z };
  uvol_s3 r, v; int rr[3], vv[3];
  for (int k = 0; k < 3; k++) {
    rr[k] = ((fs >> k) & 1u) ? GEO_INV : oo[k];
    const uint32_t a = (uint32_t)ms_vertex(J, 3 * (int)f + k);
    vv[k] = (int)((a << 1) | ((a >= nbase || J.vopen_d[0][a]) ? 1u : 0u));
  }
  r.x = rr[0]; r.y = rr[1]; r.z = rr[2]; v.x = vv[0]; v.y = vv[1]; v.z = vv[2];
  *reinterpret_cast<uvol_s3 *>(J.ms.ropp + 3 * (size_t)f) = r;
  *reinterpret_cast<uvol_s3 *>(J.ms.avert + 3 * (size_t)f) = v;
}
// DepthFirstTraverser over the material's table, one lane per frame (traverse_lane0's steps on the records of k_ms_pack): components start
// in DECODER order (tstart), a new vertex that is not on a boundary of this table goes right, a fork keeps its left side for later.
__global__ void __launch_bounds__(64) k_ms_traverse(GeoJob *jobs) {
  GeoJob &J = jobs[blockIdx.x];
  if (threadIdx.x != 0 || !MS_LIVE(J)) return;
  const int nf = (int)J.nf;
  const uint32_t ecap = J.ecap, stcap = J.stcap;
  uint32_t *fvis = J.ms.fvis, *vvis = J.ms.vvis;
  int32_t *order = J.ms.order, *stack = J.ms.stack;
  const int32_t *rv = J.ms.avert, *ro = J.ms.ropp;          // (k_ms_pack)
  uint32_t n = 0; int nvis = 0;
#define MS_FVIS(F) ((fvis[(F) >> 5] >> ((F) & 31)) & 1u)
#define MS_VISIT(C, VI) do { const uint32_t v_ = (uint32_t)(VI) >> 1; const uint32_t w_ = vvis[v_ >> 5]; if (!((w_ >> (v_ & 31)) & 1u)) { \
    if (n >= ecap) { J.status = GEO_E_WS_OVERFLOW; return; } vvis[v_ >> 5] = w_ | (1u << (v_ & 31)); order[n++] = (C); fresh = true; } } while (0)
  for (int f = 0; f < nf && nvis < nf; f++) {
    const int x0 = J.tstart[f], c0 = 3 * (x0 >> 2) + (x0 & 3);
    if (MS_FVIS(c0 / 3)) continue;
    uint32_t sp = 0; bool fresh;
    stack[sp++] = c0;
    MS_VISIT(g_nxt(c0), rv[g_nxt(c0)]); MS_VISIT(g_prv(c0), rv[g_prv(c0)]);
    while (sp > 0) {
      int c = stack[sp - 1];
      if (c < 0 || MS_FVIS(c / 3)) { sp--; continue; }
      for (;;) {
        const int face = c / 3, k = c - 3 * face;
        const uvol_s3 v3 = *reinterpret_cast<const uvol_s3 *>(rv + 3 * (size_t)face), o3 = *reinterpret_cast<const uvol_s3 *>(ro + 3 * (size_t)face);
        const int vs[3] = { v3.x, v3.y, v3.z }, os[3] = { o3.x, o3.y, o3.z };
        const int vi = vs[k], rc = os[(k + 1) % 3], lc = os[(k + 2) % 3];
        fvis[face >> 5] |= 1u << (face & 31); nvis++;
        fresh = false;
        MS_VISIT(c, vi);
        if (fresh && !(vi & 1)) { c = rc; if (c < 0) { J.status = -23; return; } continue; }      // (an interior vertex has a right neighbour)
        const bool rvis = rc < 0 || MS_FVIS(rc / 3), lvis = lc < 0 || MS_FVIS(lc / 3);
        if (rvis && lvis) { sp--; break; }
        if (rvis) { c = lc; continue; }
        if (lvis) { c = rc; continue; }
        if (sp + 1 > stcap) { J.status = GEO_E_WS_OVERFLOW; return; }
        stack[sp - 1] = lc; stack[sp++] = rc;
        break;
      }
    }
  }
#undef MS_VISIT
#undef MS_FVIS
  J.ms.ne = n; J.ms.done = 1;
}
// v2d[attribute vertex] = its position in the coding order
__global__ void __launch_bounds__(UVOL_BLOCK) k_ms_v2d(GeoJob *jobs) {
  GeoJob &J = jobs[blockIdx.y];
  if (!MS_LIVE(J)) return;
  const uint32_t i = blockIdx.x * UVOL_BLOCK + threadIdx.x;
  if (i < J.ms.ne) J.ms.v2d[(uint32_t)J.ms.avert[J.ms.order[i]] >> 1] = (int32_t)i;      // (avert: vertex << 1 | open since k_ms_pack)
}
// Residuals (k_pred_mat on the material's own table): the opposite corner is taken through the seam-masked table and the neighbour
// availability test runs against this table's order.  Every corner of a face carries the face's id, so the parallelogram of the face
// across a non-seam edge predicts that face's id; without one, the previous entry (0 for entry 0).  Wrap transform over [min id, max id].
__global__ void __launch_bounds__(UVOL_BLOCK) k_ms_pred(GeoJob *jobs) {
  GeoJob &J = jobs[blockIdx.y];
  if (!MS_LIVE(J)) return;
  const uint32_t p = blockIdx.x * UVOL_BLOCK + threadIdx.x;
  if (p >= J.ms.ne) return;
  const int32_t *v2d = J.ms.v2d;
  const int ci = J.ms.order[p];
  const int own = J.fmat[ci / 3];
  long long pred = 0;
  if (p > 0) {
    bool have = false;
    const int oci = J.ms.ropp[ci];
    if (oci >= 0) {
      const uvol_s3 v3 = *reinterpret_cast<const uvol_s3 *>(J.ms.avert + 3 * (size_t)(oci / 3));      // (order does not matter: all three must be coded before p)
      const uint32_t a = (uint32_t)v2d[(uint32_t)v3.x >> 1], bn = (uint32_t)v2d[(uint32_t)v3.y >> 1], bp = (uint32_t)v2d[(uint32_t)v3.z >> 1];
      if (a < p && bn < p && bp < p) { pred = J.fmat[oci / 3]; have = true; }      // (next + previous - opposite, all three of one face)
    }
    if (!have) pred = J.fmat[J.ms.order[p - 1] / 3];
  }
  J.sym_mat[p] = g_sym_of(g_wrap_corr((int)J.mat_lo, (int)J.mat_hi, own, pred));
}
