// geo_weld.hpp - the decoder's last mile: weld the three per-corner entry streams into ONE index per corner + one value record per point
// (uvol_decode_mesh_batch_points; what the stock player's DRACOLoader hands a BufferGeometry).
// Part of the geometry decoder translation unit: included by geom_decode.hip after k_gdec_finish (not a standalone header).
// ------------------------------------------------------------------------------------------------
// A point is a distinct tuple (idx_pos[c], idx_uv[c], idx_nrm[c]) - on the packed path, for a frame whose material is a corner attribute, with
// the corner's material value as a fourth member (J.w.cmat, k_m3_cornermat) -; points are numbered by first appearance in corner order.  The keys are
// the three index streams k_gdec_finish has just written (12 bytes per corner, never copied).  Route (b) of the two that fit this code base,
// "position fans": a point never spans two position entries, so the corners are grouped by position entry with a counting sort and every
// corner compares itself against its own small fan (~6 corners) - nothing is hashed, the result is exact by construction and independent
// of the order the atomics put the fan in (the representative is a minimum).  One launch per stage for the whole batch (blockIdx.y = frame);
// no thread walks more than one fan.
//   k_weld_clear    zero the per-entry counters
//   k_weld_count    corner -> its rank inside the fan of its position entry (one atomicAdd per corner)
//   k_weld_scan     counters -> block-local exclusive offsets + block sums            } fan start of entry p =
//   k_weld_sums     block sums -> block offsets (one workgroup per frame)             }   bsum_p[p / 256] + cnt[p]
//   k_weld_scatter  fan[start + rank] = corner
//   k_weld_rep      representative = lowest corner of the fan with equal (uv, normal) entries (and corner material); first-appearance flags scanned per block
//   k_weld_sums     again for the flags -> point ids, n_points
//   k_weld_write    index[c] = point of the representative; the first corner of a point gathers its values (bit copies, no arithmetic)
// uvol_decode_mesh_batch_packed runs the same stages up to the point ids, k_weld_packed_check ahead of them and k_weld_write_packed in
// place of k_weld_write: 16-byte records of the integers the file holds (no dequantised float is read: none is written on that path).
// A position entry shared by more than GW_MAXFAN corners fails its frame (GW_E_FAN -> UVOL_E_UNSUPPORTED): the pairwise compare is
// quadratic in the fan, and a longer one would turn one thread into a serial chain.  This is a limit of this entry point alone: such a
// file (a sequential, `-cl 0`, stream can hold one) still decodes through uvol_decode_mesh_batch.  The largest fan of the recorded files
// (every fifth counted) is 62 corners, of the bench's sphere 400 (its poles).  tests/points_cases.py (run_long_fan) pins the code.
// Route (a), the hash-partitioned LDS dedup of geo_dedup.hpp, was NOT built or measured against this one (DESIGN.md section 5 says so).
// ------------------------------------------------------------------------------------------------
#define GW_MAXFAN 4096
#define GW_E_FAN (-41)
#define GW_E_NOPOS (-42)
#define GW_E_PK_POS (-43)      // packed records: the position attribute is not quantised to 1 .. 16 bits (or has not 3 components)
#define GW_E_PK_UV (-44)       //                 the same of the tex-coord attribute (2 components)
#define GW_E_PK_NRM (-45)      //                 a normal attribute that is neither octahedral nor of 3 components

struct GWView { const uint32_t *ip, *iu, *in; uint32_t nc, np, has_uv, has_nrm; };
// np = 0 (every kernel idles) unless the frame decoded, carries positions and its entries fit the counters
__device__ __forceinline__ GWView gw_view(const GeoDecJob &J) {
  GWView V; V.ip = J.o_idx[0]; V.iu = J.o_idx[1]; V.in = J.o_idx[2]; V.nc = 3u * (uint32_t)J.nf;
  V.np = (J.w.on && J.o_n[0] <= J.ecap) ? J.o_n[0] : 0u; V.has_uv = J.o_n[1] != 0; V.has_nrm = J.o_n[2] != 0;
  return V;
}
__device__ __forceinline__ uint32_t gw_blocks(uint32_t n) { return (n + UVOL_BLOCK - 1) / UVOL_BLOCK; }

__global__ void __launch_bounds__(UVOL_BLOCK) k_weld_clear(GeoDecJob *jobs) {
  GeoDecJob &J = jobs[blockIdx.y];
  if (!J.w.on || J.status != 0) return;
  const GWView V = gw_view(J);
  if (blockIdx.x == 0 && threadIdx.x == 0 && V.np == 0) { J.status = GW_E_NOPOS; return; }      // no position attribute (or more entries than the workspace was carved for)
  for (uint32_t i = blockIdx.x * UVOL_BLOCK + threadIdx.x; i <= V.np; i += gridDim.x * UVOL_BLOCK) J.w.cnt[i] = 0;
}

__global__ void __launch_bounds__(UVOL_BLOCK) k_weld_count(GeoDecJob *jobs) {
  GeoDecJob &J = jobs[blockIdx.y];
  const GWView V = gw_view(J);
  const uint32_t c = blockIdx.x * UVOL_BLOCK + threadIdx.x;
  if (J.status != 0 || V.np == 0 || c >= V.nc) return;
  const uint32_t p = V.ip[c];
  if (p >= V.np || (V.has_uv && V.iu[c] >= J.o_n[1]) || (V.has_nrm && V.in[c] >= J.o_n[2])) { J.status = -19; return; }      // an index past its attribute's entries: corrupt tables
  J.w.rep[c] = atomicAdd(&J.w.cnt[p], 1u);                  // (rank inside the fan; rep[] holds it until k_weld_rep)
}

__global__ void __launch_bounds__(UVOL_BLOCK) k_weld_scan(GeoDecJob *jobs) {
  GeoDecJob &J = jobs[blockIdx.y];
  const GWView V = gw_view(J);
  if (blockIdx.x >= gw_blocks(V.np)) return;                // block-uniform (np does not change during the weld)
  const uint32_t i = blockIdx.x * UVOL_BLOCK + threadIdx.x;
  const uint32_t v = i < V.np ? J.w.cnt[i] : 0u; uint32_t tot;
  if (v > GW_MAXFAN) J.status = GW_E_FAN;
  const uint32_t ex = block_excl_scan(v, &tot);
  if (i < V.np) J.w.cnt[i] = ex;
  if (threadIdx.x == 0) J.w.bsum_p[blockIdx.x] = tot;
}

// block sums -> exclusive block offsets, [nblocks] = total.  which 0: the fan counters (per position entry); 1: the first-appearance flags
// (per corner), whose total is the frame's point count
__global__ void __launch_bounds__(UVOL_BLOCK) k_weld_sums(GeoDecJob *jobs, int which) {
  GeoDecJob &J = jobs[blockIdx.y];
  const GWView V = gw_view(J);
  if (V.np == 0) return;
  const uint32_t nblocks = gw_blocks(which == 0 ? V.np : V.nc);
  uint32_t *bsum = which == 0 ? J.w.bsum_p : J.w.bsum_c;
  __shared__ uint32_t carry;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (uint32_t b0 = 0; b0 < nblocks; b0 += UVOL_BLOCK) {
    const uint32_t i = b0 + threadIdx.x;
    const uint32_t v = i < nblocks ? bsum[i] : 0u; uint32_t tot;
    const uint32_t ex = block_excl_scan(v, &tot);
    const uint32_t c = carry;
    if (i < nblocks) bsum[i] = c + ex;
    __syncthreads();
    if (threadIdx.x == 0) carry = c + tot;
    __syncthreads();
  }
  if (threadIdx.x == 0) { bsum[nblocks] = carry; if (which == 1) J.w.np = carry; }
}

__global__ void __launch_bounds__(UVOL_BLOCK) k_weld_scatter(GeoDecJob *jobs) {
  GeoDecJob &J = jobs[blockIdx.y];
  const GWView V = gw_view(J);
  const uint32_t c = blockIdx.x * UVOL_BLOCK + threadIdx.x;
  if (J.status != 0 || V.np == 0 || c >= V.nc) return;
  const uint32_t p = V.ip[c];
  J.w.fan[J.w.bsum_p[p / UVOL_BLOCK] + J.w.cnt[p] + J.w.rep[c]] = c;      // (status 0: every corner was counted, the fans tile [0, nc))
}

__global__ void __launch_bounds__(UVOL_BLOCK) k_weld_rep(GeoDecJob *jobs) {
  GeoDecJob &J = jobs[blockIdx.y];
  const GWView V = gw_view(J);
  if (V.np == 0 || blockIdx.x >= gw_blocks(V.nc)) return;   // block-uniform
  const uint32_t c = blockIdx.x * UVOL_BLOCK + threadIdx.x;
  const bool live = J.status == 0 && c < V.nc;              // (no kernel of this launch writes the status)
  uint32_t best = c;
  if (live) {
    const uint32_t p = V.ip[c], ku = V.has_uv ? V.iu[c] : 0u, kn = V.has_nrm ? V.in[c] : 0u;
    const uint8_t *cm = J.w.mat_corner ? J.w.cmat : nullptr; const uint32_t km = cm ? cm[c] : 0u;
    const uint32_t s = J.w.bsum_p[p / UVOL_BLOCK] + J.w.cnt[p], e = p + 1 < V.np ? J.w.bsum_p[(p + 1) / UVOL_BLOCK] + J.w.cnt[p + 1] : V.nc;
    for (uint32_t j = s; j < e; j++) {                      // <= GW_MAXFAN corners (k_weld_scan)
      const uint32_t c2 = J.w.fan[j];
      if (c2 < best && (!V.has_uv || V.iu[c2] == ku) && (!V.has_nrm || V.in[c2] == kn) && (!cm || cm[c2] == km)) best = c2;
    }
    J.w.rep[c] = best;
  }
  uint32_t tot;
  const uint32_t ex = block_excl_scan((live && best == c) ? 1u : 0u, &tot);
  if (live) J.w.pid[c] = ex;
  if (threadIdx.x == 0) J.w.bsum_c[blockIdx.x] = tot;
}

__global__ void __launch_bounds__(UVOL_BLOCK) k_weld_write(GeoDecJob *jobs) {
  GeoDecJob &J = jobs[blockIdx.y];
  const GWView V = gw_view(J);
  const uint32_t c = blockIdx.x * UVOL_BLOCK + threadIdx.x;
  if (J.status != 0 || V.np == 0 || c >= V.nc || J.w.np > J.w.cap) return;      // a frame whose points do not fit is left alone (UVOL_E_NOSPACE)
  const uint32_t r = J.w.rep[c], id = J.w.bsum_c[r / UVOL_BLOCK] + J.w.pid[r];
  if (J.w.o_index) J.w.o_index[c] = id;
  if (r != c) return;
  // the first corner of point `id` gathers the point's values: bit copies of the entries k_gdec_finish wrote
  const uint32_t *pv = reinterpret_cast<const uint32_t *>(J.o_val[0]) + 3 * (size_t)V.ip[c];
  const uint32_t *uv = V.has_uv ? reinterpret_cast<const uint32_t *>(J.o_val[1]) + 2 * (size_t)V.iu[c] : nullptr;
  const uint32_t *nv = V.has_nrm ? reinterpret_cast<const uint32_t *>(J.o_val[2]) + 3 * (size_t)V.in[c] : nullptr;
  if (J.w.layout == 1) {                                    // 32-byte record pos[3] nrm[3] uv[2]: two 16-byte stores, absent slots zero
    if (!J.w.o_val[0]) return;
    uint4 *rec = reinterpret_cast<uint4 *>(J.w.o_val[0]) + 2 * (size_t)id;
    rec[0] = make_uint4(pv[0], pv[1], pv[2], nv ? nv[0] : 0u);
    rec[1] = make_uint4(nv ? nv[1] : 0u, nv ? nv[2] : 0u, uv ? uv[0] : 0u, uv ? uv[1] : 0u);
    return;
  }
  if (J.w.o_val[0]) { uint32_t *o = reinterpret_cast<uint32_t *>(J.w.o_val[0]) + 3 * (size_t)id; o[0] = pv[0]; o[1] = pv[1]; o[2] = pv[2]; }
  if (J.w.o_val[1] && uv) { uint32_t *o = reinterpret_cast<uint32_t *>(J.w.o_val[1]) + 2 * (size_t)id; o[0] = uv[0]; o[1] = uv[1]; }
  if (J.w.o_val[2] && nv) { uint32_t *o = reinterpret_cast<uint32_t *>(J.w.o_val[2]) + 3 * (size_t)id; o[0] = nv[0]; o[1] = nv[1]; o[2] = nv[2]; }
}

// ---- packed records (uvol_decode_mesh_batch_packed) ----
// One thread per frame, ahead of the weld: can the frame's integers go into uint16 slots?  A frame that fails here is skipped by every
// weld kernel (status != 0) and none of its outputs is written.  Also picks the material decoder (k_gdec_facemat's rule).
__global__ void __launch_bounds__(64) k_weld_packed_check(GeoDecJob *jobs) {
  GeoDecJob &J = jobs[blockIdx.x];
  if (threadIdx.x != 0 || !J.w.on || J.status != 0) return;
  J.w.mat_dec = gd_mat_decoder(J);
  if (J.o_dec[0] < 0) return;                               // (no position attribute: k_weld_clear reports it)
  { const GDAtt &A = J.att[J.o_dec[0]]; if (A.seq_type != 2 || A.ncomp != 3 || A.qbits < 1 || A.qbits > 16) { J.status = GW_E_PK_POS; return; } }
  if (J.o_dec[1] >= 0) { const GDAtt &A = J.att[J.o_dec[1]]; if (A.seq_type != 2 || A.ncomp != 2 || A.qbits < 1 || A.qbits > 16) { J.status = GW_E_PK_UV; return; } }
  if (J.o_dec[2] >= 0) { const GDAtt &A = J.att[J.o_dec[2]]; if (A.seq_type != 3 && A.ncomp != 3) { J.status = GW_E_PK_NRM; return; } }
}

// rintf(v * 127) as the low byte of an int8 (round to nearest even, the default mode); a value past the int8 range - no unit normal has one - saturates
__device__ __forceinline__ uint32_t gw_snorm8(float v) {
  const float r = rintf(v * 127.0f);
  return (uint32_t)(int32_t)fminf(fmaxf(r, -128.0f), 127.0f) & 0xffu;
}

// index[c] = point of the representative; the first corner of a point gathers the point's record:
//   uint16 px py pz | uint16 material | uint16 u v | int8 nx ny nz 0      - one aligned 16-byte store per point, absent slots zero
// The integers come straight from the decoders' vals arrays (kept alive up to this stage on the packed path, gdec_carve); the normal is
// the float of gd_oct_normal / k_gdec_finish's expressions, rounded here.
__global__ void __launch_bounds__(UVOL_BLOCK) k_weld_write_packed(GeoDecJob *jobs, const GeoJob *gj) {
  GeoDecJob &J = jobs[blockIdx.y]; const GeoJob &G = gj[blockIdx.y];
  const GWView V = gw_view(J);
  const uint32_t c = blockIdx.x * UVOL_BLOCK + threadIdx.x;
  if (J.status != 0 || V.np == 0 || c >= V.nc || J.w.np > J.w.cap) return;      // a frame whose points do not fit is left alone (UVOL_E_NOSPACE)
  const uint32_t r = J.w.rep[c], id = J.w.bsum_c[r / UVOL_BLOCK] + J.w.pid[r];
  if (J.w.o_index) J.w.o_index[c] = id;
  if (r != c || !J.w.o_val[0]) return;
  const int32_t *pv = J.att[J.o_dec[0]].vals + 3 * (size_t)V.ip[c];
  const uint32_t mat = J.w.mat_dec >= 0 ? (J.w.mat_corner ? (uint32_t)J.w.cmat[c] : (uint32_t)gd_mat_value(J, G, J.w.mat_dec, c)) : 0u;
  uint4 rec;
  rec.x = ((uint32_t)pv[0] & 0xffffu) | ((uint32_t)pv[1] << 16);
  rec.y = ((uint32_t)pv[2] & 0xffffu) | (mat << 16);
  rec.z = 0; rec.w = 0;
  if (V.has_uv) { const int32_t *uv = J.att[J.o_dec[1]].vals + 2 * (size_t)V.iu[c]; rec.z = ((uint32_t)uv[0] & 0xffffu) | ((uint32_t)uv[1] << 16); }
  if (V.has_nrm) {
    const GDAtt &A = J.att[J.o_dec[2]]; const size_t i = V.in[c];
    float n[3];
    if (A.seq_type == 3) gd_oct_normal(A, i, n[0], n[1], n[2]);
    else if (A.seq_type == 2) { const float delta = gd_delta(A); for (int k = 0; k < 3; k++) n[k] = A.minv[k] + (float)A.vals[3 * i + k] * delta; }
    else for (int k = 0; k < 3; k++) n[k] = (float)A.vals[3 * i + k];
    rec.w = gw_snorm8(n[0]) | (gw_snorm8(n[1]) << 8) | (gw_snorm8(n[2]) << 16);
  }
  reinterpret_cast<uint4 *>(J.w.o_val[0])[id] = rec;        // id < np <= cap <= the caller's cap_points
}
