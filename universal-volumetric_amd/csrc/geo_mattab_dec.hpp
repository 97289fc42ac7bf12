// geo_mattab_dec.hpp - K7b: the material attribute of a file whose material is a Draco MESH_CORNER_ATTRIBUTE on a THIRD seam-cut table
// (attribute-data slot 2: what uvol_params.material_seams writes for a frame with tex-coords and normals; csrc/geo_matseam.hpp is the
// encoder's half).  Part of the geometry decoder translation unit: included by geom_decode.hip behind k_gdec_facemat (not a standalone header).
// ------------------------------------------------------------------------------------------------
// The shared stages already give every attribute-data slot its seam bits, edge flags and attribute vertices (k_gdec_seams, k_gdec_atttab /
// k_gdec_attscan run over GD_MAXAD slots); what stops at two tables is everything from k_gdec_open on, because the traversal kernels the
// decoder shares with the encoder (geo_run_traversals) read a GeoJob with two attribute tables.  Those are the encoder's hot kernels and
// are not widened: the third table has storage of its own (GeoDecJob::m3) and this pass of its own, BEHIND the prediction stage and ahead
// of the outputs, for the calls that return materials (uvol_decode_mesh_batch_mat, uvol_decode_mesh_batch_packed).  The other entry points
// enqueue and carve none of it and skip the values of the slot-2 decoder; neither does a call none of whose files carries such an attribute
// (gdec_corner_material, geom_decode.hip: the host looks at the decoder rows of the files, which lie in host memory).  In a mixed call every
// kernel leaves at once for a frame without a slot-2 corner material (m3.dec < 0).
//   k_m3_setup      1 lane / frame   which decoder sits on table 3; its symbol stream is pointed at the pass's own (small) tables
//   k_m3_open       thread / corner  seam-cut opposite corners (ropp) and the on-boundary flags of the table's vertices
//   k_m3_traverse   1 lane / frame   DepthFirstTraverser over the table from the decoder-order component starts (faces 0, 1, 2 ...) -> order, ne
//   k_m3_v2d        thread / entry   attribute vertex -> entry
//   k_gdec_rans     (mode 4)         the decoder's symbol stream, with the count the traversal gave
//   k_m3_pgram      thread / entry   parallelogram neighbours on this table (k_gdec_pgram's rule)
//   k_m3_pred       1 wave / frame   the wrap-transform recurrence (gd_pgram_chunks, one component) -> att[dec].vals
//   k_m3_cornermat  thread / corner  packed form only, frames whose material is a corner attribute in ANY slot: the value at every corner,
//                                    one byte each - the weld's fourth key and the records' material
// The parallel kernels run a bounded grid per frame (M3_GRID workgroups, grid-stride): most frames of a call carry no such material, and an idle
// frame then costs a few dozen workgroups that leave at once, not one per 256 corners.
// The traversal is one lane per frame, as the encoder's K6b: a frame with a slot-2 material pays one more serial walk of its faces
// (DESIGN.md section 5 has the measurement).
// ------------------------------------------------------------------------------------------------
#define M3_NS 1024           // alphabet of the symbol stream: wrap-corrected residuals of 8-bit values stay below 512
#define M3_PREC_BITS 15      // and its rANS precision: (3 * bit length) / 2 of such an alphabet
#define M3_GRID 48           // workgroups per frame of the pass's parallel kernels
#define M3_LIVE(J) ((J).status == 0 && (J).m3.on && (J).m3.dec >= 0)

__global__ void __launch_bounds__(64) k_m3_setup(GeoDecJob *jobs) {
  GeoDecJob &J = jobs[blockIdx.x];
  if (threadIdx.x != 0 || J.status != 0 || !J.m3.on || J.method != 1) return;
  int d = -1;
  for (int k = J.ndec - 1; k >= 0; k--) if (J.att[k].table == 3) d = k;          // (k_gdec_index let only the material shape onto table 3)
  if (d < 0 || J.nad < 3) return;
  GDRans &S = J.rs[6 + d];
  // an alphabet or a precision past what 8-bit values can need: not this attribute (the plain entry points, which skip the values, still read the file)
  if (!S.present || S.ns > M3_NS || S.prec_bits > M3_PREC_BITS) { J.status = -23; return; }
  S.probs = J.m3.probs; S.cum = J.m3.cum; S.lut = J.m3.lut; S.out = J.m3.syms; S.nvals = 0; S.early = 0; S.redo = 0;
  J.m3.ne = 0; J.m3.dec = d;
}

__global__ void __launch_bounds__(UVOL_BLOCK) k_m3_open(GeoDecJob *jobs) {
  GeoDecJob &J = jobs[blockIdx.y];
  if (!M3_LIVE(J)) return;
  const int nc = 3 * J.nf;
  GTab T; T.opp = J.opp; T.seam = J.edge_seam[2];
  for (int c = (int)(blockIdx.x * UVOL_BLOCK + threadIdx.x); c < nc; c += (int)(gridDim.x * UVOL_BLOCK)) {
    if (c < J.t_nv[2]) J.m3.v2d[c] = 0;                    // (attribute vertices <= corners; a vertex the traversal misses - corrupt tables - maps to entry 0)
    J.m3.ropp[c] = gt_opp(T, c);
    // a vertex of this table is on a boundary when the fan segment it stands for ends: some corner of it has no left neighbour
    if (gt_swl(T, c) < 0) J.m3.vopen[J.t_c2v[2][c]] = 1;   // (k_gdec_validate: every t_c2v entry is below t_nv <= ecap; flags start out zero)
  }
}

// traverse_lane0's steps (geo_traverse_lds.hpp) on this table: a new vertex that is not on a boundary goes right, a fork keeps its left side
__global__ void __launch_bounds__(64) k_m3_traverse(GeoDecJob *jobs) {
  GeoDecJob &J = jobs[blockIdx.x];
  if (threadIdx.x != 0 || !M3_LIVE(J)) return;
  const int nf = J.nf;
  const uint32_t ecap = J.ecap, stcap = (uint32_t)nf + 2;
  UVOL_G(uint32_t) fvis = UVOL_TO_G(uint32_t, J.m3.fvis); UVOL_G(uint32_t) vvis = UVOL_TO_G(uint32_t, J.m3.vvis);
  UVOL_G(int32_t) order = UVOL_TO_G(int32_t, J.m3.order); UVOL_G(int32_t) stack = UVOL_TO_G(int32_t, J.m3.stack);
  UVOL_G(const int32_t) rv = UVOL_TO_G(const int32_t, J.t_c2v[2]); UVOL_G(const int32_t) ro = UVOL_TO_G(const int32_t, J.m3.ropp);
  UVOL_G(const uint8_t) vopen = UVOL_TO_G(const uint8_t, J.m3.vopen);
  uint32_t n = 0; int nvis = 0;
#define M3_FVIS(F) ((fvis[(F) >> 5] >> ((F) & 31)) & 1u)
#define M3_VISIT(C, V) do { const uint32_t v_ = (uint32_t)(V); const uint32_t w_ = vvis[v_ >> 5]; if (!((w_ >> (v_ & 31)) & 1u)) { \
    if (n >= ecap) { J.status = GD_E_WS_OVERFLOW; return; } vvis[v_ >> 5] = w_ | (1u << (v_ & 31)); order[n++] = (C); fresh = true; } } while (0)
  for (int f = 0; f < nf && nvis < nf; f++) {
    if (M3_FVIS(f)) continue;
    const int c0 = 3 * f;
    uint32_t sp = 0; bool fresh;
    stack[sp++] = c0;
    M3_VISIT(c0 + 1, rv[c0 + 1]); M3_VISIT(c0 + 2, rv[c0 + 2]);
    while (sp > 0) {
      int c = stack[sp - 1];
      if (c < 0 || M3_FVIS(c / 3)) { sp--; continue; }
      for (;;) {
        const int face = c / 3, k = c - 3 * face;
        const int vi = rv[c], rc = ro[3 * face + (k + 1) % 3], lc = ro[3 * face + (k + 2) % 3];
        fvis[face >> 5] |= 1u << (face & 31); nvis++;
        fresh = false;
        M3_VISIT(c, vi);
        if (fresh && !vopen[vi]) { c = rc; if (c < 0) { J.status = -19; return; } continue; }      // (an interior vertex has a right neighbour)
        const bool rvis = rc < 0 || M3_FVIS(rc / 3), lvis = lc < 0 || M3_FVIS(lc / 3);
        if (rvis && lvis) { sp--; break; }
        if (rvis) { c = lc; continue; }
        if (lvis) { c = rc; continue; }
        if (sp + 1 > stcap) { J.status = -19; return; }
        stack[sp - 1] = lc; stack[sp++] = rc;
        break;
      }
    }
  }
#undef M3_VISIT
#undef M3_FVIS
  J.m3.ne = n;
  GDRans &S = J.rs[6 + J.m3.dec]; S.nvals = n; S.early = 3;      // one component: k_gdec_rans, mode 4
}

__global__ void __launch_bounds__(UVOL_BLOCK) k_m3_v2d(GeoDecJob *jobs) {
  GeoDecJob &J = jobs[blockIdx.y];
  if (!M3_LIVE(J)) return;
  for (uint32_t i = blockIdx.x * UVOL_BLOCK + threadIdx.x; i < J.m3.ne; i += gridDim.x * UVOL_BLOCK) J.m3.v2d[J.t_c2v[2][J.m3.order[i]]] = (int32_t)i;
}

__global__ void __launch_bounds__(UVOL_BLOCK) k_m3_pgram(GeoDecJob *jobs) {
  GeoDecJob &J = jobs[blockIdx.y];
  if (!M3_LIVE(J)) return;
  const int32_t *v2d = J.m3.v2d, *xc2v = J.t_c2v[2];
  const bool pgram = J.att[J.m3.dec].pred_method == 1;
  for (int p = (int)(blockIdx.x * UVOL_BLOCK + threadIdx.x); p < (int)J.m3.ne; p += (int)(gridDim.x * UVOL_BLOCK)) {
    int32_t *nb = J.m3.nbr + 3 * (size_t)p;
    nb[0] = nb[1] = nb[2] = -1;
    if (p == 0 || !pgram) continue;
    const int oci = J.m3.ropp[J.m3.order[p]];
    if (oci == GEO_INV) continue;
    const int a = v2d[xc2v[oci]], bn = v2d[xc2v[g_nxt(oci)]], bp = v2d[xc2v[g_prv(oci)]];
    if (a < p && bn < p && bp < p) { nb[0] = a; nb[1] = bn; nb[2] = bp; }
  }
}

__global__ void __launch_bounds__(64) k_m3_pred(GeoDecJob *jobs) {
  GeoDecJob &J = jobs[blockIdx.x];
  __shared__ int s_go;
  __shared__ __attribute__((aligned(16))) int32_t s_ring[GDP_R], s_stage[64 * GDP_STAGE], s_tile[64];
  if (threadIdx.x == 0) s_go = M3_LIVE(J) ? 1 : 0;         // (sampled once per workgroup: all lanes take the same path to the barriers)
  __syncthreads();
  if (!s_go) return;
  const GDAtt &A = J.att[J.m3.dec];
  gd_pgram_chunks<1>((int)J.m3.ne, UVOL_TO_G(const int32_t, J.m3.nbr), UVOL_TO_G(const uint32_t, J.m3.syms), UVOL_TO_G(int32_t, A.vals), A.lo, A.hi, s_ring, s_stage, s_tile);
}

__global__ void __launch_bounds__(UVOL_BLOCK) k_m3_cornermat(GeoDecJob *jobs, const GeoJob *gj) {
  GeoDecJob &J = jobs[blockIdx.y]; const GeoJob &G = gj[blockIdx.y];
  if (J.status != 0 || !J.w.on || !J.w.packed) return;
  const int d = gd_mat_decoder(J);
  if (d < 0 || J.att[d].dec_type != 1) return;
  if (blockIdx.x == 0 && threadIdx.x == 0) J.w.mat_corner = 1;
  for (uint32_t c = blockIdx.x * UVOL_BLOCK + threadIdx.x; c < 3u * (uint32_t)J.nf; c += gridDim.x * UVOL_BLOCK) J.w.cmat[c] = gd_mat_value(J, G, d, c);
}
