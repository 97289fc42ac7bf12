/* include/uvol_codec.h — C ABI of the MI355X-native UVOL codec (libuvolcodec.so).
 *
 * This is the drop-in boundary for the ONE hot path of EtherealEngine/Universal-Volumetric:
 * the per-frame geometry + texture encode that scripts/Encoder.py performs by spawning two
 * external processes,
 *     draco_encoder -i f.obj -o f.drc -qp 11 -qt 10 -qn 8 -qg 8 -cl 7      (scripts/Encoder.py:260-262)
 *     basisu -ktx2 -tex_type video -multifile_printf P -multifile_num B -multifile_first i -y_flip
 *            -output_file texture_%07u.ktx2                                  (scripts/Encoder.py:290-292)
 * Every entry point below replaces one of those process boundaries with an in-process call that
 * runs hand-written HIP kernels on gfx950.  Conventions follow the reference's own in-repo C-ABI
 * precedent (deprecated/encoder_legacy/codec/corto_codec.h:41-43): opaque handle, caller-owned
 * buffers, int status, no exceptions, no torch types.
 *
 * Threading: a ctx is bound to one GPU and one HIP stream; it is NOT thread-safe.  Different
 * ctxs may be used from different threads / processes (one process per GPU in bench.py).
 * Every batched encode entry point also has an enqueue form (`*_async`): it returns at once, the work runs in call order on the
 * context, and uvol_sync(ctx) completes it (SURVEY 8b "Threading").
 * There is NO CPU fallback: uvol_ctx_create fails with UVOL_E_NODEVICE when no gfx950 GPU is present.
 */
#ifndef UVOL_CODEC_H
#define UVOL_CODEC_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UVOL_ABI_VERSION 1

enum {
  UVOL_OK = 0,
  UVOL_E_INVALID = -1,     /* bad argument */
  UVOL_E_NODEVICE = -2,    /* no usable HIP device (fails loudly, never falls back to CPU) */
  UVOL_E_HIP = -3,         /* HIP runtime error, see uvol_last_error */
  UVOL_E_NOSPACE = -4,     /* caller output buffer too small (out_len holds the required size) */
  UVOL_E_ENCODE = -5,      /* per-frame encode failure (bad indices, empty mesh, ...) */
  UVOL_E_UNSUPPORTED = -6
};

/* Mirrors the numeric project-config.json fields consumed on the hot path
 * (scripts/Encoder.py:171-179 template, :260 and :290 use sites; defaults identical). */
typedef struct uvol_params {
  int32_t q_position_attr;          /* Q_POSITION_ATTR,         default 11 */
  int32_t q_texture_attr;           /* Q_TEXTURE_ATTR,          default 10 */
  int32_t q_normal_attr;            /* Q_NORMAL_ATTR,           default 8  */
  int32_t q_generic_attr;           /* Q_GENERIC_ATTR,          default 8 (accepted, numerically inert as in stock draco_encoder: the one generic attribute, the
                                       material id of uvol_encode_mesh_batch_mat, is an integer attribute and Draco quantises float attributes only) */
  int32_t draco_compression_level;  /* DRACO_COMPRESSION_LEVEL 0..10, default 7.  0 = sequential connectivity + difference predictor (stock draco_encoder's choice at
                                       this level); 1..10 are encoded with the level-7 tool set (valence edgebreaker; the level itself is not part of the bitstream) */
  int32_t ktx2_batch_size;          /* KTX2_BATCH_SIZE (mandatory in the reference) = layers per .ktx2 */
  int32_t etc1s_quality;            /* basisu -q equivalent, 1..255, default 128 (Encoder.py passes none) */
  int32_t y_flip;                   /* basisu -y_flip (Encoder.py:290 always passes it), default 1 */
  int32_t max_batch;                /* frames in flight per geometry batch, default 32 */
  int32_t cu_mod;                   /* experimental CU partition (hipExtStreamCreateWithCUMask), 0 = all CUs (default).  > 1: mask bits with
                                       (index % cu_mod) in cu_residues; -1: the CUs with ordinal lo .. hi - 1 inside EVERY XCD, cu_residues =
                                       lo << 8 | hi.  Mask bit i is CU i / 8 of XCD i % 8, and a queue cannot be kept off an XCD
                                       (profiles/r05_xcd_census.json) */
  int32_t cu_residues;              /* bit r set = residue r allowed (cu_mod > 1); lo << 8 | hi (cu_mod == -1) */
  int32_t traverse_vbits_l2;        /* 1: the attribute traversers keep only their face bitmap in LDS and the vertex bitmap in L2
                                       (6 instead of 3 per CU): pays off when several contexts keep > 700 frames in flight */
  int32_t stream_priority;          /* 1: create the context's HIP stream with the highest priority (short, LDS-hungry texture
                                       kernels then get free CU slots before the long geometry walkers take them) */
  int32_t uastc;                    /* basisu -uastc: 1 = the texture entry points write UASTC LDR 4x4 .ktx2 files (DFD colour model 166, no
                                       supercompression; every layer an independent image) instead of ETC1S/BasisLZ; default 0 (Encoder.py:290 passes no -uastc) */
  int32_t material_seams;           /* 1: a frame in which two materials meet at shared vertices (an interior material seam) is written with its
                                       material attribute as a Draco MESH_CORNER_ATTRIBUTE (seam-bit stream, corner table and traversal of its own)
                                       instead of being refused; frames without such a seam keep their bytes.  Default 0: such a frame gets
                                       UVOL_E_UNSUPPORTED (see "material ids" below).  Took reserved[0]: struct size and UVOL_ABI_VERSION stay */
  int32_t reserved[1];
} uvol_params;

void uvol_params_default(uvol_params *p);

typedef struct uvol_ctx uvol_ctx;

int  uvol_abi_version(void);
int  uvol_device_count(void);
/* device = HIP ordinal. Returns UVOL_OK and *out on success. */
int  uvol_ctx_create(int device, const uvol_params *params, uvol_ctx **out);
void uvol_ctx_destroy(uvol_ctx *ctx);
const char *uvol_last_error(const uvol_ctx *ctx);
/* completes everything enqueued on ctx (uvol_*_async calls and the stream); returns the first error among the enqueued calls */
int  uvol_sync(uvol_ctx *ctx);

/* Page-locked host memory (SURVEY 8(d) times the path from "inputs resident in pinned host memory").  The entry points that take HOST arrays
 * copy pageable memory through the library's own pinned double buffers (host threads fill them, ~42 GB/s).  A call whose input arrays ALL lie
 * in memory from uvol_host_alloc takes the UPLINK instead (round 6): the uploads of all its groups (meshes) / parts (texture segments) are
 * queued on a copy stream of the context when the call begins, ahead of its kernels, and the encoders' streams wait for them on the device -
 * no host thread touches the data, and with the enqueue forms (`*_async`) the next call's uploads cross the link while this call encodes.
 * The device layout mirrors the caller's: arrays that lie back to back in host memory (256-byte aligned, gaps of <= 4 KiB) go over in ONE
 * copy per run - lay the arrays of a frame, and consecutive frames, next to each other in the arena.
 * One pageable array and the whole call is staged as before.  Input arrays belong to the call until it completes (blocking forms: until they
 * return; enqueue forms: until uvol_sync).  The ring of upload slots holds 8 mesh groups / 4 texture parts at most (a slot of 640
 * 100 k-vertex frames is 6.8 GB; uvol_trim gives them back).  Process-wide registry, thread-safe; NULL when the runtime refuses (no device,
 * out of lockable memory).  What a caller of the reference holds at this boundary are files / host buffers (scripts/Encoder.py:244-302):
 * this is where it would read them into. */
void *uvol_host_alloc(size_t bytes);
void  uvol_host_free(void *p);
/* uvol_sync, then the workspaces of ctx - geometry lanes, texture lanes, upload slots - go back to the device (they only grow: a context that
 * once ran a 2560-frame call as one group keeps ~130 GB until it is destroyed); its streams stay, the next call allocates what it needs.  No counterpart in the reference
 * (its encoders are processes that exit, scripts/Encoder.py:266-302); a long-lived host uses it between jobs of very different sizes. */
int  uvol_trim(uvol_ctx *ctx);

/* One frame of OBJ-shaped geometry: separate value arrays + per-corner index triplets
 * (what draco_encoder parses out of `v/vt/vn/f` lines).  uv / nrm (and their index arrays) may be
 * NULL.  Pointers are HOST pointers for uvol_encode_mesh* and DEVICE pointers for *_dev. */
typedef struct uvol_mesh {
  const float    *pos;      uint32_t n_pos;    /* n_pos * 3 */
  const float    *uv;       uint32_t n_uv;     /* n_uv  * 2 */
  const float    *nrm;      uint32_t n_nrm;    /* n_nrm * 3 */
  const uint32_t *idx_pos;                     /* 3 * n_faces */
  const uint32_t *idx_uv;                      /* 3 * n_faces or NULL */
  const uint32_t *idx_nrm;                     /* 3 * n_faces or NULL */
  uint32_t        n_faces;
} uvol_mesh;

/* Upper bound of the .drc size for a mesh (use to size `out`). */
size_t uvol_mesh_bound(const uvol_mesh *m);

/* Device memory one frame of these dimensions occupies while it is in flight inside uvol_encode_mesh_batch[_dev] (workspace with
 * lifetime-shared arrays + its share of the packed output area): frames in flight per GPU = HBM left / this. */
size_t uvol_mesh_workspace(const uvol_ctx *ctx, const uvol_mesh *m);

/* Replaces one `draco_encoder` process (scripts/Encoder.py:260-262): OBJ arrays -> .drc bytes. */
int uvol_encode_mesh(uvol_ctx *ctx, const uvol_mesh *mesh, uint8_t *out, size_t cap, size_t *out_len);

/* Batched form of HOT LOOP 1 (scripts/Encoder.py:256-267): n independent frames, all in flight on
 * the GPU at once (one serial connectivity walker per frame, parallel kernels batched over frames).
 * status[i] is the per-frame result; a failed frame does not poison the batch. */
int uvol_encode_mesh_batch(uvol_ctx *ctx, const uvol_mesh *meshes, int n,
                           uint8_t *const *outs, const size_t *caps, size_t *out_lens, int *status);
/* Same with inputs already resident in HBM (device pointers inside `meshes`; `meshes` itself is a host array). */
int uvol_encode_mesh_batch_dev(uvol_ctx *ctx, const uvol_mesh *meshes, int n,
                               uint8_t *const *outs, const size_t *caps, size_t *out_lens, int *status);

/* Ingest on the device (`draco_encoder -i frame.obj` parses the OBJ text itself, scripts/Encoder.py:256-262): n OBJ files
 * as TEXT in host memory -> meshes_out[i] with DEVICE pointers (v / vt / vn / f lines, polygons fanned, 1-based and negative indices;
 * bit-identical to the host parser of host/uvol_host.cpp, i.e. to strtof), ready for uvol_encode_mesh_batch_dev[_async].  The arrays
 * live in the context's slot `slot` (0 or 1) until that slot is parsed into again.  To parse batch b + 1 WHILE batch b encodes, parse on a
 * second context of the same device (contexts are independent and device pointers are not tied to one; host/uvolenc.cpp does this) -
 * on one context the call waits for that context's enqueued calls like every other entry point.  status[i]: UVOL_OK; UVOL_E_UNSUPPORTED = the text holds a number or line the device
 * parser leaves to the host (more than 19 significant digits, inf / nan, a value on a float rounding boundary, an incomplete `v` line):
 * parse that file with the host parser; UVOL_E_INVALID = a face references a missing vertex / no faces.  Blocking. */
int uvol_parse_obj_batch_dev(uvol_ctx *ctx, const uint8_t *const *obj_text, const size_t *lens, int n, int slot,
                             uvol_mesh *meshes_out, int *status);

/* The PNG half of the ingest stage (`basisu` reads the PNGs itself, scripts/Encoder.py:274-292): n images of one size as INFLATED
 * scanlines in host memory - what zlib gives for the concatenated IDAT chunks of an 8-bit, non-interlaced RGB (channels 3) or RGBA (4)
 * PNG: height rows of one filter-type byte + width * channels filtered bytes - are un-filtered on the device (Sub / Up / Average /
 * Paeth, bit-identical to the host reader) into RGBA8 layers, top row first, in the context's slot `slot` (0 / 1; valid until that slot
 * is used again): rgba_dev_out[i] is what uvol_encode_texture_segments_dev takes.  The inflate stays with the caller (one serial bit
 * stream per file; the files of a batch inflate in parallel on host threads).  Other PNG variants (16-bit, palette, grey, interlaced,
 * wider than 8192): decode them on the host.  The call returns once the kernel is queued on an ingest stream of the context (the host
 * buffers may be re-used at once: pageable buffers have been staged, buffers in uvol_host_alloc memory have been read - the call waits for
 * those copies, not for the kernels); the context's texture entry points order themselves behind it, a caller that
 * reads the layers itself calls uvol_sync(ctx) first.  So the un-filter of batch k + 1 overlaps the encode of batch k. */
int uvol_unfilter_png_batch_dev(uvol_ctx *ctx, const uint8_t *const *inflated, int n, uint32_t width, uint32_t height, int channels,
                                int slot, const uint8_t **rgba_dev_out);

/* The same with the zlib INFLATE on the device too (what `basisu` does first with every PNG it reads, scripts/Encoder.py:274-292): n images
 * of one size, each as its zlib stream - the concatenated data of the file's IDAT chunks, zlib header and Adler-32 trailer included -
 * in host memory.  One wave per stream inflates it (stored, fixed and dynamic blocks; the 32 KiB window lives in LDS) into the scanline
 * buffer the un-filter kernel then reads, so the host uploads the ~3 MB file instead of inflating it and staging 16.8 MB.  Same slots,
 * ordering and output as uvol_unfilter_png_batch_dev.  A corrupt stream, or one that does not hold height x (1 + width x channels) bytes,
 * or whose Adler-32 trailer does not match, fails ALONE: uvol_png_status reports it, its layer is undefined, the other images are not
 * affected. */
int uvol_inflate_png_batch_dev(uvol_ctx *ctx, const uint8_t *const *zlib_streams, const size_t *lens, int n, uint32_t width, uint32_t height,
                               int channels, int slot, const uint8_t **rgba_dev_out);
/* Per-image statuses of the last uvol_unfilter_png_batch_dev / uvol_inflate_png_batch_dev call on `slot` (waits for its kernels):
 * status[i] = UVOL_OK or UVOL_E_INVALID, n <= the images of that call.  status == NULL: the first failure is the return value. */
int uvol_png_status(uvol_ctx *ctx, int slot, int *status, int n);

/* ---- JPEG textures (additive: uvol_abi_version stays 1) ----
 * The reference's README names a JPEG as its example texture input (`ImagesPath: Eg: /home/3D/export_[#####].jpg`), and the `basisu` that
 * scripts/Encoder.py:290 spawns reads .jpg as it reads .png.  The split is the PNG one: the serial bit stream (marker parse, Huffman decode)
 * stays with the caller (host/uvol_host.cpp read_jpeg_raw; one stream per file, the files of a batch in parallel on host threads), the
 * data-parallel part - dequantisation, 8 x 8 inverse DCT, chroma upsampling, YCbCr -> RGB - runs on the device into the RGBA8 layers of an
 * ingest slot.
 *
 * THE DECODING RULE.  JPEG fixes neither an IDCT nor an upsampling filter bit for bit, so - as with the downscale filter and the direct etc2
 * encode - the rule is this project's own and exact in integers: the device kernel, the host reader (read_jpeg) and the NumPy restatement of
 * tests/jpeg_cases.py agree bit for bit; closeness to libjpeg is measured, not an identity.
 *
 * Accepted: baseline sequential DCT (SOF0), 8-bit samples, Huffman coding, ONE scan that holds all components, restart intervals (DRI /
 * RST0-7) included; one component (grey; its sampling factors are ignored, as the standard says for a single-component scan) or three
 * components Y, Cb, Cr with chroma at 1 x 1 and luma at 1 x 1 (4:4:4), 2 x 1 (4:2:2) or 2 x 2 (4:2:0); width <= 8192, height <= 16384.
 * Refused by name (UVOL_E_UNSUPPORTED from the host reader, never a silent wrong decode): progressive (SOF2), extended or 12-bit (SOF1 with
 * P != 8), lossless or arithmetic-coded (SOF3, SOF9 upwards), four components or any other sampling layout (luma 1 x 2 included), an Adobe
 * APP14 segment with transform 0 (RGB stored as such), 16-bit quantisation tables, several scans.
 *
 * Coefficient layout (what uvol_idct_jpeg_batch_dev takes; also what jpeg_read_coefficients of libjpeg hands a caller): per image, then per
 * component, the component's blocks in raster order over its block grid padded to whole MCUs - with mcu_w = ceil(W / (8 hmax)),
 * mcu_h = ceil(H / (8 vmax)) the grid is mcu_w h_c blocks wide and mcu_h v_c blocks high -, each block 64 int16 in natural order
 * (8 v + u), QUANTISED (not dequantised).  Each image also carries its quantisation tables, one per component: 64 uint16, natural order.
 *
 * Per block (every >> is an arithmetic shift; every sum fits 32 bits because of the two clamps):
 *   dequantise  F[v][u] = clamp(coef[v][u] q[v][u], -32768, 32767)
 *   cosines     K[x][u] = floor(8192 s_u cos((2 x + 1) u pi / 16) + 0.5) in double, s_0 = 1 / (2 sqrt 2), s_u = 1 / 2 otherwise
 *               (K[x][0] = 2896; the largest entry is 4017)
 *   columns     b[y][u] = clamp((sum_v K[y][v] F[v][u] + 1024) >> 11, -32768, 32767)
 *   rows        p[y][x] = (sum_u K[x][u] b[y][u] + 16384) >> 15
 *   sample      clamp(p + 128, 0, 255)
 * Both clamps are inactive on any stream an encoder produced; they keep a hostile stream from overflowing.
 *
 * Chroma upsampling.  A component's real extent is cw = ceil(W h_c / hmax) by ch = ceil(H v_c / vmax); the filter runs over that extent, not
 * over the MCU padding: a neighbour outside it is the sample itself.
 *   2 x 1   with sample c and its left / right neighbours l / r: out[2 i] = (3 c + l + 1) >> 2, out[2 i + 1] = (3 c + r + 2) >> 2
 *   2 x 2   vertical step, not rounded: a_even = 3 c + above, a_odd = 3 c + below; horizontal step on those rows:
 *           out[2 i] = (3 a + a_left + 8) >> 4, out[2 i + 1] = (3 a + a_right + 7) >> 4
 * Crop to W x H after upsampling.
 *
 * Colour, with cb = Cb - 128, cr = Cr - 128: R = Y + ((91881 cr + 32768) >> 16), G = Y - ((22554 cb + 46802 cr + 32768) >> 16),
 * B = Y + ((116130 cb + 32768) >> 16), each clamped to 0 .. 255; grey gives R = G = B = Y.  Alpha is 255, top row first. */
typedef struct {
  uint32_t width, height;
  int components;        /* 1 or 3 */
  int luma_h, luma_v;    /* 1 x 1, 2 x 1 or 2 x 2; 1 x 1 for grey */
} uvol_jpeg_layout;
/* int16 values per image in the layout above; 0 for a layout outside the rule */
size_t uvol_jpeg_coeff_count(const uvol_jpeg_layout *layout);
/* n images of ONE layout, each as its quantised coefficients (coeffs[i]: uvol_jpeg_coeff_count values) and its own quantisation tables
 * (qtables[i]: components x 64 uint16 - a sequence may change quality from frame to frame), in host memory -> rgba_dev_out[i] = DEVICE
 * pointer to width * height * 4 bytes in slot `slot` (0 / 1) of the SAME ingest slots uvol_unfilter_png_batch_dev writes, with its ordering
 * and lifetime: the call returns once the kernels are queued on the ingest stream and the host buffers have been read (pageable memory
 * is staged, uvol_host_alloc memory is copied from where it lies and the call waits for those copies); the texture, downscale and mip-chain
 * entry points order themselves behind it; uvol_sync before the caller reads the layers itself; uvol_trim gives the memory back.
 * n <= 0: UVOL_OK, nothing happens.  UVOL_E_INVALID with a message, before anything runs: a bad slot, a NULL pointer, a layout outside the
 * rule, a size beyond 8192 x 16384.  Profile groups: jpeg.upload, jpeg.idct. */
int uvol_idct_jpeg_batch_dev(uvol_ctx *ctx, const int16_t *const *coeffs, const uint16_t *const *qtables, int n,
                             const uvol_jpeg_layout *layout, int slot, const uint8_t **rgba_dev_out);

/* ---- reduced-resolution texture layers (additive: uvol_abi_version stays 1) ----
 * The player manifest gives every texture target its own `resolution` (reference src/Interfaces.ts:41-73, :113-131), so that one capture is
 * served in several sizes; the raw `etc2` target in particular exists for the devices that cannot afford the transcoder
 * (src/V2/player.ts:207-222) - nor 2048^2 per frame.  This entry point makes the smaller layers on the device, from the full-size layers
 * that lie in HBM after uvol_unfilter_png_batch_dev / uvol_inflate_png_batch_dev anyway: n RGBA8 layers of width x height (rgba[i]: width *
 * height * 4 bytes, top row first) are downscaled by factor = 2, 4 or 8 in ONE kernel launch; rgba_dev_out[i] is a DEVICE pointer to
 * ceil(width / factor) x ceil(height / factor) x 4 bytes in the context's downscale slot `slot` (0 / 1), valid until that slot is written
 * again, and is what uvol_encode_texture_segment[s]_dev[_async] takes.
 * inputs_on_device: rgba[i] are device pointers (4-byte aligned; layers of a PNG ingest slot are ordered behind their un-filter, as the
 * texture entry points do it); otherwise host memory, uploaded through the library's staging buffers.
 * The filter is this project's own, defined exactly in integers (stock `basisu -mipmap` uses a Kaiser window in linear light, which nothing
 * at hand pins): output texel (X, Y) is made in ONE step - never by repeated halving - from the box B of the n input texels with
 * factor X <= x < min(factor X + factor, width), factor Y <= y < min(factor Y + factor, height).
 *   lin[v] = floor(65535 L(v / 255) + 0.5), v = 0 .. 255, L = the sRGB decoding function (s / 12.92 for s <= 0.04045, else
 *            ((s + 0.055) / 1.055)^2.4), in double; strictly increasing, lin[1] = 20, lin[254] = 64952, lin[255] = 65535.
 *   alpha:   A = sum of a over B; out.a = (2 A + n) / (2 n), integer division.
 *   colour:  alpha-weighted in linear light, so that a transparent neighbour does not bleed into an opaque texel.  Per channel c of r, g, b:
 *            N = sum lin[c] a, D = A - or, when A == 0, N = sum lin[c], D = n -; m = (2 N + D) / (2 D), integer division; out.c = the v
 *            with the smallest |lin[v] - m|, the lower v at a tie.
 * A constant image maps to itself; a 2 x 2 black / white opaque checker gives (188, 188, 188, 255), where a byte average would give 128.
 * Blocking: like the other blocking entry points it first waits for the context's enqueued calls - so a slot an enqueued encode still reads
 * is never overwritten - and returns when the layers are complete.  There is NO host-output form (the layers exist to be encoded from HBM)
 * and NO enqueue form (the kernel moves 17 MB per 2048^2 layer once; the encode that follows is what takes time).  uvol_trim gives the slots
 * back, uvol_ctx_destroy frees them.  Mip levels inside one .ktx2 are made by uvol_mipchain_rgba_batch_dev below, with this filter.
 * UVOL_E_INVALID with a message, before anything runs: a factor other than 2 / 4 / 8, a slot other than 0 / 1, a NULL layer (or a device
 * layer that is not 4-byte aligned), width or height zero or beyond the limits of uvol_unfilter_png_batch_dev (8192 x 16384).  n <= 0 is
 * UVOL_OK and does nothing. */
int uvol_downscale_rgba_batch_dev(uvol_ctx *ctx, const uint8_t *const *rgba, int n, uint32_t width, uint32_t height,
                                  int inputs_on_device, int factor, int slot, const uint8_t **rgba_dev_out);

/* ---- mip levels inside one UASTC .ktx2 (additive: uvol_abi_version stays 1) ----
 * A compressed texture cannot get mip levels at load time: the stock loader turns trilinear filtering on only for a file that carries more
 * than one level (reference src/lib/KTX2Loader.js:279) and transcodes every (mip, layer) the file has (:516-570).  The reduced-resolution
 * targets above are separate files a player picks between, not levels of one texture.
 *
 * uvol_mip_level_count: floor(log2(max(width, height))) + 1, the length of the full chain (level 0 included); 0 for an empty image.
 *
 * uvol_mipchain_rgba_batch_dev: n RGBA8 layers of width x height (top row first) become levels 1 .. levels - 1 of each layer in ONE pass over
 * level 0; rgba_dev_out[i * (levels - 1) + (v - 1)] is a DEVICE pointer to level v of layer i, in the context's CHAIN slot `slot` (0 / 1; the
 * chain slots are not the downscale slots: a ladder rung and a chain coexist), valid until that slot is written again.  levels == 0 means the
 * full chain (rgba_dev_out then holds n * (uvol_mip_level_count(width, height) - 1) entries).  inputs_on_device as for the downscale: device
 * pointers (4-byte aligned; layers of a PNG ingest slot are ordered behind their un-filter) or host memory uploaded through the staging buffers.
 * The filter (normative) is the one of uvol_downscale_rgba_batch_dev with a box of any size:
 *   level v is lw x lh with lw = max(1, width >> v), lh = max(1, height >> v);
 *   fx = width / lw and fy = height / lh must be exact integers - always so for powers of two, and for width = 2^a m up to v = a -; otherwise
 *   the call is UVOL_E_INVALID with a message naming the level and the size, before anything runs;
 *   output texel (X, Y) of level v is made in ONE step from the n = fx fy texels of level 0 with fx X <= x < fx X + fx, fy Y <= y < fy Y + fy, by
 *   exactly the lin[], alpha, alpha-weighted colour and nearest-v rules above (A = sum a, out.a = (2 A + n) / (2 n); N = sum lin[c] a, D = A - or,
 *   when A == 0, N = sum lin[c], D = n -, m = (2 N + D) / (2 D), out.c = the v with the smallest |lin[v] - m|, the lower v at a tie).
 * So for v <= 3 the result is bit-identical to uvol_downscale_rgba_batch_dev at factor 2^v.  The sums A, sum lin a and sum lin are additive
 * over boxes, so the device computes a level from the sums of finer levels with the same result as from level 0, and reads level 0 once
 * (sums are 64-bit from the 16 x 16 box on; csrc/tex_mipchain.hip).
 * Blocking: it first waits for the context's enqueued calls and returns when the levels are complete; there is no enqueue form.  uvol_trim
 * gives the slots back, uvol_ctx_destroy frees them.  UVOL_E_INVALID with a message, before anything runs: the refusals of the downscale (a
 * NULL layer, a device layer that is not 4-byte aligned, a slot other than 0 / 1, width or height zero or beyond 8192 x 16384), levels < 0,
 * levels > uvol_mip_level_count(width, height), a level that fails the divisibility rule.  levels == 1 and n <= 0 are UVOL_OK and do nothing.
 * Profile groups: ingest.mipchain (and ingest.mipchain_upload for host inputs). */
int uvol_mip_level_count(uint32_t width, uint32_t height);
int uvol_mipchain_rgba_batch_dev(uvol_ctx *ctx, const uint8_t *const *rgba, int n, uint32_t width, uint32_t height,
                                 int inputs_on_device, int levels, int slot, const uint8_t **rgba_dev_out);

/* uvol_encode_texture_segments_mips: the semantics of uvol_encode_texture_segments_st (per-segment status[], host or device inputs) with mip
 * levels.  In a context created with uvol_params.uastc = 1 every segment becomes ONE .ktx2 with levelCount = levels (0 = the full chain):
 * level 0 as uvol_encode_texture_segments_st encodes it, then the chain above on the context's stream (in a slot of its own, not the caller's
 * two), then the UASTC encode of every level; the context's y_flip applies to each level's own height.  A UASTC level is nothing but its
 * layers' blocks, so level v of the file is byte for byte the level data of a single-level file encoded from the level-v images.  Container:
 * levelCount in the header, one level-index entry of 24 bytes per level from byte 80 on (level 0 first), DFD and key-value offsets moved
 * accordingly, level data stored smallest level first, every level 16-byte aligned, inside a level the layers in order with
 * ceil(lw / 4) ceil(lh / 4) blocks of 16 bytes each, byteLength == uncompressedByteLength, KTXanimData and the DFD as in the single-level file,
 * the alpha channel id set when any level has a block with alpha.  levels == 1 gives the bytes of uvol_encode_texture_segments_st.  The
 * divisibility rule of the chain applies (UVOL_E_INVALID before anything runs).  In an ETC1S context (uastc = 0) levels != 1 is
 * UVOL_E_UNSUPPORTED before anything runs: "mip levels are written in the UASTC mode only" - the ETC1S pipeline has
 * one slice geometry for all slices.  There is NO enqueue form.  uvol_texture_bound_mips: the size that always suffices for outs[s]. */
size_t uvol_texture_bound_mips(uint32_t width, uint32_t height, int n_layers, int levels);
int uvol_encode_texture_segments_mips(uvol_ctx *ctx, const uint8_t *const *rgba, int n_segments, int n_layers,
                                      uint32_t width, uint32_t height, int inputs_on_device, int levels,
                                      uint8_t *const *outs, const size_t *caps, size_t *out_lens, int *status);

/* Reading them.  uvol_ktx2_levels (host-only): the level count of a file uvol_ktx2_info accepts - a UASTC file's levelCount, after every
 * entry of its level index has been checked against the file size and against layers x blocks(level) x 16; 1 for an ETC1S file.
 * uvol_transcode_texture_segments_level: uvol_transcode_texture_segments_st for mip level `level` of every file: outs[s * layers + l] receives
 * that level of layer l at the LEVEL's size (max(1, width >> level) x max(1, height >> level); layer_cap sized for it), for every UVOL_TARGET_*
 * a UASTC source takes - what transcodeImage(dst, mip, layer, ...) gives the stock loader.  A file whose count is <= level is UVOL_E_INVALID in
 * its own status; an ETC1S file has one level: level 0 behaves as uvol_transcode_texture_segments_st, any other is UVOL_E_INVALID for that
 * segment.  The decode / transcode entry points without a level argument and uvol_ktx2_info accept a multi-level UASTC file and mean level 0.
 * Zstandard-supercompressed multi-level UASTC files carry one frame per level; each is inflated under the bounds of the single-level case.
 * Multi-level ETC1S (stock `basisu -mipmap` without -uastc) stays UVOL_E_UNSUPPORTED, with a message that names it. */
int uvol_ktx2_levels(const uint8_t *ktx2, size_t len, uint32_t *levels);
int uvol_transcode_texture_segments_level(uvol_ctx *ctx, const uint8_t *const *ktx2, const size_t *lens, int n_segments, int level,
                                          uint8_t *const *outs, size_t layer_cap, int target, int outputs_on_device, int *status);

/* ---- the raw `etc2` texture target from source texels (additive: uvol_abi_version stays 1) ----
 * The player's raw `etc2` target is uncompressed block data, one file per frame at 8 bytes per 4x4 block, for the devices that cannot afford
 * the transcoder (reference src/Interfaces.ts:19, :165-169, src/V2/player.ts:208-222, :338-356, :454-470).
 * uvol_transcode_texture_segments_etc1 makes it by re-packing ETC1S segments: one base colour and one table per block, snapped to the
 * segment's codebooks, at a file size that is fixed anyway.  This entry point encodes it from the SOURCE texels with a search over all of
 * ETC1: n RGBA8 layers of width x height (rgba[i]: width * height * 4 bytes, top row first) -> blocks[i] = ceil(width / 4) * ceil(height / 4)
 * 8-byte ETC1 blocks (valid ETC2 RGB8), raster order, the byte layout uvol_transcode_texture_segments_etc1 writes; ONE kernel launch for the
 * batch.  Texels are fetched as the texture encoder fetches them: the context's y_flip applies, edges are replicated for partial blocks,
 * px[4 y + x]; alpha is ignored (the player uploads RGB_ETC2_Format).
 *
 * The encoding rule is this project's own, exact in integers (this text is normative; tests/etc2_direct_cases.py restates it in NumPy and
 * is checked bit for bit).
 * Preliminaries.  For flip f in {0, 1}, half h of texel (x, y) is x >= 2 (f = 0) or y >= 2 (f = 1).  Per half and channel:
 *   m8 = (sum over its 8 texels + 4) >> 3, q5 = (m8 * 31 + 127) / 255, q4 = (m8 * 15 + 127) / 255.  A 5-bit base b expands to
 *   (b << 3) | (b >> 2), a 4-bit base to b * 17.  Modifiers are those of ETC1: table t has magnitudes {2,8}, {5,17}, {9,29}, {13,42}, {18,60},
 *   {24,80}, {33,106}, {47,183}; pixel index 0 .. 3 = +small, +large, -small, -large.
 * Half error E(base, t): the sum over the half's 8 texels of the smallest squared RGB error among the four modified colours, each channel
 *   clamped to 0 .. 255 before the difference is taken; each texel takes the first nearest index in the order 0 .. 3.
 * Half search in precision P (5 or 4 bits, top value 31 or 15), starting at q = q5 or q4.
 *   Step 1: for t = 0 .. 7, for dd in the order (0, -1, +1): the candidate is clamp(q[c] + dd, 0, top) on all three channels; a candidate
 *     replaces the best only on strictly smaller E.
 *   Step 2, at the best table of step 1: for c = 0 .. 2, for dd in the order (-1, +1): channel c alone is moved from the current best base;
 *     the move is skipped if it leaves 0 .. top and accepted only on strictly smaller E.
 *   The unrefined result is kept too: the best t at base q with dd = 0, first best.
 * Per flip.  Individual candidate: both halves searched in 4 bits, E_ind = the sum of their errors.  Differential candidate: both halves
 *   searched in 5 bits; if every refined delta (second - first) lies in -4 .. 3 the refined pair is used; otherwise, if the unrefined q5 pair
 *   has all deltas in -4 .. 3, that pair with its best tables; otherwise there is none.  Differential wins when it exists and
 *   E_diff <= E_ind.
 * Block.  Flip 1 wins only with strictly smaller error than flip 0.  Bytes 0 .. 2: base5 << 3 | (delta & 7) (differential) or
 *   base4 of the first half << 4 | base4 of the second (individual), R G B; byte 3: table of the first half << 5 | table of the second << 2 |
 *   diff << 1 | flip; bytes 4 .. 7: the msb plane and the lsb plane of the pixel indices, 16 bits each, big-endian, pixel i = 4 x + y.
 * Two properties follow: every block's squared error against its source texels is <= that of the plain ETC1 fit the UASTC transcode uses
 * (mean colours, best table per half) on the same texels - base q with every table is among the candidates of both modes, and the fallback
 * keeps the plain differential fit reachable -; and a differential block has 0 <= base5 + delta <= 31 in every channel, so no block falls
 * into ETC2's T, H or planar modes.  Those three modes are NOT used: their bit layouts are in nothing this project has at hand, and it does
 * not restate formats from memory.  Neither is there an EAC alpha form or an enqueue form.
 *
 * inputs_on_device: rgba[i] are device pointers (4-byte aligned; layers of a PNG ingest slot or a downscale slot are ordered behind the
 * kernels that produce them, as the texture entry points do it); otherwise host memory, uploaded through the library's staging buffers.
 * outputs_on_device: blocks[i] are device pointers (8-byte aligned); otherwise host memory, pageable or from uvol_host_alloc, on the paths
 * of the transcode entry points.  layer_cap = the size of each output buffer, at least uvol_etc2_rgb_bound(width, height) =
 * 8 * ceil(width / 4) * ceil(height / 4).
 * Blocking: it first waits for the context's enqueued calls and returns when the blocks are complete.  UVOL_E_INVALID with a message,
 * before anything runs: a NULL layer or output, a misaligned device pointer, width or height zero or beyond the limits of
 * uvol_unfilter_png_batch_dev (8192 x 16384).  UVOL_E_NOSPACE: layer_cap below the bound.  n <= 0 is UVOL_OK and does nothing.  Profile
 * groups: etc2.encode (and etc2.upload for host inputs). */
size_t uvol_etc2_rgb_bound(uint32_t width, uint32_t height);
int uvol_encode_etc2_rgb_batch(uvol_ctx *ctx, const uint8_t *const *rgba, int n, uint32_t width, uint32_t height,
                               int inputs_on_device, uint8_t *const *blocks, size_t layer_cap, int outputs_on_device);

/* GPU-resident form (SURVEY 8(b) "variants taking arrays of frames + hipStream_t"; caller-owned buffers as in
 * deprecated/encoder_legacy/codec/corto_codec.h:41-43): inputs are device pointers PRODUCED ON `producer_stream` (a hipStream_t passed
 * as void *, NULL = already complete) - the codec's kernels are ordered after the work queued on that stream so far, without a host
 * wait -, and the .drc bitstreams are LEFT IN HBM: packed into the caller's device buffer `dev_out` (capacity dev_cap bytes; 32768 +
 * 8 bytes per face per frame always suffices for the default quantisation), frame i at dev_out + out_offs[i], out_lens[i] bytes long;
 * offsets, lengths and status come back to the host, the payload never does.  A frame that does not fit gets UVOL_E_NOSPACE.  Blocking. */
int uvol_encode_mesh_batch_dev_out(uvol_ctx *ctx, const uvol_mesh *meshes, int n, void *producer_stream,
                                   uint8_t *dev_out, size_t dev_cap, size_t *out_offs, size_t *out_lens, int *status);

/* Enqueue forms.  The call returns as soon as its arguments are recorded (the `meshes`, `outs` and `caps` ARRAYS are copied);
 * the frames' input arrays, the output buffers and `out_lens` / `status` belong to the call until uvol_sync(ctx) returns, which
 * reports the first failing call (its message through uvol_last_error).  Calls enqueued on one ctx run in order; a blocking entry
 * point on the same ctx waits for them first.  A host driver overlaps its own work - parsing the next batch, writing the previous
 * one - with the GPU this way without owning a thread per context (host/uvolenc.cpp does). */
int uvol_encode_mesh_batch_async(uvol_ctx *ctx, const uvol_mesh *meshes, int n,
                                 uint8_t *const *outs, const size_t *caps, size_t *out_lens, int *status);
int uvol_encode_mesh_batch_dev_async(uvol_ctx *ctx, const uvol_mesh *meshes, int n,
                                     uint8_t *const *outs, const size_t *caps, size_t *out_lens, int *status);

/* ---- material ids: the OBJ `usemtl` attribute (additive: uvol_abi_version stays 1) ----
 * Stock draco_encoder adds a fourth attribute to every OBJ that has a `usemtl` line: GENERIC, uint8, one component, the index of the face's
 * material (every recorded .drc of the reference carries it).  uvol_mesh is passed in arrays, so the ids travel in a parallel array:
 * face_material: NULL, or n entries; face_material[i]: NULL (frame i is encoded exactly as by uvol_encode_mesh_batch*) or meshes[i].n_faces
 * bytes, one material id per INPUT face, in host or device memory like the mesh's own arrays (inputs_on_device).  The attribute is written as
 * Draco writes it while every vertex has ONE material - single-material frames, and frames whose materials follow connected components: a
 * vertex attribute on the base corner table, parallelogram prediction, wrap transform.  A frame in which two materials meet at a shared
 * vertex (an interior material seam, which Draco codes as a corner attribute with a table of its own) gets status[i] = UVOL_E_UNSUPPORTED,
 * uvol_last_error names it, and the other frames of the batch are not affected: encode that frame without materials - or create the
 * context with uvol_params.material_seams = 1.  Such a frame is then written as Draco writes an attribute with interior seams, a
 * MESH_CORNER_ATTRIBUTE: the material's decoder row is the one above with decoder type 1 and the material's own attribute-data slot (the
 * last one); that slot's seam stream carries one bit per interior edge - 1 where the two faces carry different ids - in the order of the
 * other seam streams; the values are one uint8 per attribute vertex of the material's seam-cut corner table, in the depth-first traversal
 * order of THAT table, predicted by the parallelogram rule on it (previous entry where no parallelogram is available), wrap transform over
 * the frame's [min id, max id].  The choice is made per frame on the device: a frame without such a seam - no ids, one id, ids that follow
 * connected components - gives the bytes it gives with material_seams = 0, and a group none of whose frames carries two ids launches
 * nothing new.  No stock file of this shape is at hand (every recorded file of the reference has one material), so this form is not
 * byte-pinned against stock draco_encoder, like alpha slices and -cl 0; the repository's oracle decoder, which is pinned on the recorded
 * files for the tex-coord and normal slots, reads it generically.  A seamed frame holds more device memory while it is in flight
 * (DESIGN.md section 3); uvol_mesh_workspace has no material argument and keeps its meaning.  The DECODE side of this library reads the
 * corner form in every slot (see uvol_decode_mesh_batch_mat and uvol_decode_mesh_batch_packed below), as any Draco decoder does.  With
 * DRACO_COMPRESSION_LEVEL 0 (sequential connectivity) a call that passes any ids is refused as a whole (UVOL_E_UNSUPPORTED).  Host ids are
 * uploaded through the library's staging buffers; uvol_encode_mesh_batch_dev_out has no such form. */
size_t uvol_mesh_bound_mat(const uvol_mesh *m);      /* upper bound of the .drc of a frame with material ids */
int uvol_encode_mesh_batch_mat(uvol_ctx *ctx, const uvol_mesh *meshes, const uint8_t *const *face_material, int n, int inputs_on_device,
                               uint8_t *const *outs, const size_t *caps, size_t *out_lens, int *status);
/* enqueue form: the contract of uvol_encode_mesh_batch_async (the face_material ARRAY is copied, the ids belong to the call until uvol_sync) */
int uvol_encode_mesh_batch_mat_async(uvol_ctx *ctx, const uvol_mesh *meshes, const uint8_t *const *face_material, int n, int inputs_on_device,
                                     uint8_t *const *outs, const size_t *caps, size_t *out_lens, int *status);
/* As uvol_parse_obj_batch_dev, plus face_material_dev_out[i] = device pointer to one byte per fanned triangle (in the context's slot, like the
 * mesh's arrays), or NULL when the file has no `usemtl` line.  Ids are handed out by first appearance of the name, from 0; faces ahead of the
 * first `usemtl` take id 0; `mtllib` files are not read; a file with more than 256 names loses the attribute (stock switches to uint16). */
int uvol_parse_obj_batch_dev_mat(uvol_ctx *ctx, const uint8_t *const *obj_text, const size_t *lens, int n, int slot,
                                 uvol_mesh *meshes_out, const uint8_t **face_material_dev_out, int *status);

/* Replaces one `basisu -ktx2 -tex_type video` process (scripts/Encoder.py:290-292):
 * n_layers RGBA8 images (width*height*4 bytes each, top row first as a PNG decoder yields them)
 * -> one ETC1S/BasisLZ .ktx2 with n_layers array layers (layer 0 I-frame, others P-frames).
 * A segment any of whose images has alpha != 255 gets ALPHA SLICES, as basisu writes them and the stock player reads them
 * (src/lib/KTX2Loader.js:493-497): a second slice per image (the alpha channel as a grey image through the same codebooks), a second
 * DFD sample (channel 15) and the image descs' second offset / length pair; opaque segments are unchanged, and the two kinds may
 * share a batch.  Read back by uvol_decode_texture_segments (RGBA32); the opaque targets (ETC1 / BC7) refuse such a file. */
size_t uvol_texture_bound(uint32_t width, uint32_t height, int n_layers);
int uvol_encode_texture_segment(uvol_ctx *ctx, const uint8_t *const *rgba, int n_layers,
                                uint32_t width, uint32_t height,
                                uint8_t *out, size_t cap, size_t *out_len);
/* Same with the layers already resident in HBM (array of device pointers). */
int uvol_encode_texture_segment_dev(uvol_ctx *ctx, const uint8_t *const *rgba_dev, int n_layers,
                                    uint32_t width, uint32_t height,
                                    uint8_t *out, size_t cap, size_t *out_len);

/* Batched form of HOT LOOP 2 (scripts/Encoder.py:279-298): n_segments independent segments of n_layers layers each
 * (rgba[s * n_layers + l]), all of one size, encoded with ONE kernel launch per pipeline stage. */
int uvol_encode_texture_segments(uvol_ctx *ctx, const uint8_t *const *rgba, int n_segments, int n_layers,
                                 uint32_t width, uint32_t height,
                                 uint8_t *const *outs, const size_t *caps, size_t *out_lens);
int uvol_encode_texture_segments_dev(uvol_ctx *ctx, const uint8_t *const *rgba_dev, int n_segments, int n_layers,
                                     uint32_t width, uint32_t height,
                                     uint8_t *const *outs, const size_t *caps, size_t *out_lens);

/* enqueue forms of the two batched texture entry points (same contract as uvol_encode_mesh_batch_async) */
int uvol_encode_texture_segments_async(uvol_ctx *ctx, const uint8_t *const *rgba, int n_segments, int n_layers,
                                       uint32_t width, uint32_t height,
                                       uint8_t *const *outs, const size_t *caps, size_t *out_lens);
int uvol_encode_texture_segments_dev_async(uvol_ctx *ctx, const uint8_t *const *rgba_dev, int n_segments, int n_layers,
                                           uint32_t width, uint32_t height,
                                           uint8_t *const *outs, const size_t *caps, size_t *out_lens);

/* ---- decode path, texture half ----
 * Replaces, for the RGBA32 target, what the stock player does per .ktx2 segment: KTX2Loader parses the container and
 * hands every array layer to the basis transcoder (reference src/lib/KTX2Loader.js:469-580; src/V2/player.ts:338-356
 * uploads the layers as one sampler2DArray).  Input: BasisLZ/ETC1S .ktx2 files as uvol_encode_texture_segment[s] or
 * `basisu -ktx2 -tex_type video` write them (with or without alpha slices, one mip level), or the UASTC .ktx2 files this codec writes with
 * uvol_params.uastc (told apart by the DFD colour model).  Output: RGBA8, rows in stored order. */
/* host-only: container dimensions of one file (UVOL_E_INVALID if it is not a KTX2/BasisLZ file this decoder handles;
 * a UASTC file whose level data are Zstandard-supercompressed - supercompressionScheme 2, the default of stock `basisu -uastc -ktx2` - is
 * read since round 5 when the system's libzstd.so.1 is installed: the decode / transcode entry points inflate the level on the host
 * (dlopen; this library contains no Zstandard code) and go on as for a scheme-0 file; without libzstd, for another scheme or a corrupt
 * frame the file is UVOL_E_UNSUPPORTED, as every supercompressed UASTC file was before) */
int uvol_ktx2_info(const uint8_t *ktx2, size_t len, uint32_t *width, uint32_t *height, uint32_t *layers);
/* n_segments files of one width / height / layer count; rgba[s * layers + l] receives width*height*4 bytes
 * (layer_cap = size of each buffer).  One kernel launch per stage for the whole batch. */
int uvol_decode_texture_segments(uvol_ctx *ctx, const uint8_t *const *ktx2, const size_t *lens, int n_segments,
                                 uint8_t *const *rgba, size_t layer_cap);
/* Same, writing straight into device buffers (rgba_dev = host array of device pointers). */
int uvol_decode_texture_segments_dev(uvol_ctx *ctx, const uint8_t *const *ktx2, const size_t *lens, int n_segments,
                                     uint8_t *const *rgba_dev, size_t layer_cap);

/* ETC1 target (the player's `etc2` raw-texture family, reference src/Interfaces.ts:19, src/V2/player.ts:338-356; any ETC2 sampler
 * reads ETC1 blocks): blocks[s * layers + l] receives ceil(w/4) * ceil(h/4) 8-byte ETC1 blocks in raster order (layer_cap =
 * size of each buffer); an exact re-pack, every ETC1S block is a valid ETC1 block.  outputs_on_device: blocks are device pointers.
 * UASTC sources (round 5; the loader's etc2Supported / etc1Supported rows for UASTC, src/lib/KTX2Loader.js:619-636): this entry point and
 * uvol_transcode_texture_segments_etc2_rgba take them as well - a plain ETC1 fit of each block's decoded texels (both flips, differential
 * or individual bases, best intensity table per half-block; not the basis transcoder's hint-driven path) and an EAC fit of their alpha,
 * gated by PSNR against the RGBA32 decode. */
int uvol_transcode_texture_segments_etc1(uvol_ctx *ctx, const uint8_t *const *ktx2, const size_t *lens, int n_segments,
                                         uint8_t *const *blocks, size_t layer_cap, int outputs_on_device);

/* BC7 target (KTX2Loader's choice on desktop GPUs, reference src/lib/KTX2Loader.js:591-689): blocks[s * layers + l] receives
 * ceil(w/4) * ceil(h/4) 16-byte BC7 mode-6 blocks in raster order.  Lossy re-fit of the four ETC1S colours to 16 interpolation
 * weights (endpoint error <= 1, inner colours to the nearest weight); gated by PSNR against the RGBA32 decode, not bit parity. */
int uvol_transcode_texture_segments_bc7(uvol_ctx *ctx, const uint8_t *const *ktx2, const size_t *lens, int n_segments,
                                        uint8_t *const *blocks, size_t layer_cap, int outputs_on_device);
/* UASTC sources (round 5): BC7 is what the stock loader asks a UASTC file for wherever ASTC is not supported - every desktop GPU
 * (reference src/lib/KTX2Loader.js:601-609, chosen at :665-676).  Single-plane blocks and solid blocks become mode 6 (each endpoint with
 * the p-bit that represents its four values best, every texel the nearest of the 16 interpolated colours), dual-plane blocks mode 5 with
 * the rotation that puts the second plane's channel into the scalar slot (UASTC's and BC7's 2-bit weights are equal).  A re-fit of the
 * block's own endpoints, gated by PSNR against the RGBA32 decode like the ETC1S case - the basis transcoder's tables are not restated. */
/* Files WITH alpha slices (images whose alpha was not 255; reference src/lib/KTX2Loader.js:493-497 reads them): the stock loader asks
 * such a file for the SECOND format of its table (:672-676) - BC7 with alpha or ETC2 RGBA.  uvol_transcode_texture_segments_bc7 then
 * writes mode-5 blocks whose alpha endpoints are the alpha block's lowest / highest level (exact) with 2-bit alpha indices;
 * uvol_transcode_texture_segments_etc2_rgba writes 16-byte ETC2_EAC RGBA8 blocks (EAC alpha block + the exact ETC1 colour re-pack;
 * opaque files get alpha 255).  Alpha is a re-fit (the basis transcoder's tables are not in the reference): gated by alpha PSNR against
 * the RGBA32 decode, like the BC7 colour.  The ETC1 target stays opaque-only and refuses a file with alpha slices. */
int uvol_transcode_texture_segments_etc2_rgba(uvol_ctx *ctx, const uint8_t *const *ktx2, const size_t *lens, int n_segments,
                                              uint8_t *const *blocks, size_t layer_cap, int outputs_on_device);

/* ASTC 4x4 target for UASTC sources (KTX2Loader's first choice for them, reference src/lib/KTX2Loader.js:591-600, :648-689; BASELINE
 * configs[4] "KTX2 -> ASTC"): blocks[s * layers + l] receives ceil(w/4) * ceil(h/4) 16-byte ASTC blocks in raster order.  A direct
 * re-pack of the UASTC block (same endpoints and weights; the pair is swapped and the weights mirrored where ASTC would apply blue
 * contraction; solid blocks become void-extent blocks): an ASTC decoder reproduces the UASTC texels exactly.  ETC1S sources are
 * rejected with UVOL_E_UNSUPPORTED (the stock player never picks ASTC for them). */
int uvol_transcode_texture_segments_astc(uvol_ctx *ctx, const uint8_t *const *ktx2, const size_t *lens, int n_segments,
                                         uint8_t *const *blocks, size_t layer_cap, int outputs_on_device);

/* ---- per-segment results for the batched texture calls (round 5; additive: uvol_abi_version stays 1) ----
 * The reference fails per `basisu` process (scripts/Encoder.py:293-298): one bad batch does not undo the others.  The batched texture
 * entry points above return ONE code for the call; these forms also fill status[s] per segment, like uvol_encode_mesh_batch does per
 * frame, and return UVOL_OK whenever the call itself ran (bad arguments, device errors and out-of-memory still fail the call).
 *
 * uvol_encode_texture_segments_st: as uvol_encode_texture_segments[_dev] (inputs_on_device selects which); a segment whose output buffer
 * is too small gets UVOL_E_NOSPACE (out_lens[s] = the size it needs), one the device could not encode UVOL_E_ENCODE; the others are written.
 *
 * uvol_transcode_texture_segments_st: every decode / transcode target through one entry point.  Files are judged one by one: an
 * unreadable container (UVOL_E_INVALID / UVOL_E_UNSUPPORTED from uvol_ktx2_info's rules), a shape other than the first readable file's
 * (UVOL_E_INVALID), a source kind the target does not take (UVOL_E_UNSUPPORTED: ASTC wants UASTC sources, ETC1 / ETC2 want ETC1S; RGBA32 and
 * BC7 take both), a payload that turns out corrupt on the device (UVOL_E_ENCODE) fail in their own slot; ETC1S and UASTC files may share a
 * batch.  out[s * layers + l] as in the entry point of the target; slots of failed segments are not read. */
enum { UVOL_TARGET_RGBA32 = 0, UVOL_TARGET_ETC1 = 1, UVOL_TARGET_BC7 = 2, UVOL_TARGET_ASTC = 3, UVOL_TARGET_ETC2_RGBA = 4,
       UVOL_TARGET_BC1 = 5, UVOL_TARGET_BC3 = 6 };
/* UVOL_TARGET_BC1 / UVOL_TARGET_BC3 (round 5, ETC1S sources, through uvol_transcode_texture_segments_st only): the stock loader's
 * `dxtSupported` row (reference src/lib/KTX2Loader.js:610-618: TranscoderFormat.BC1 for an opaque file, BC3 for one with alpha slices).
 * 8-byte BC1 blocks (four-colour mode; a file with alpha slices is UVOL_E_UNSUPPORTED: it is asked for BC3) / 16-byte BC3 blocks (BC4
 * alpha block from the alpha slice - 255 for an opaque file -, then the colour block), raster order.  Re-fits of the four ETC1S colours /
 * alpha levels, gated by PSNR against the RGBA32 decode like the BC7 target.  UASTC sources take both targets as well: the decoded texels of
 * a block are range-fitted (bounding-box corners along the sign of the R-G / B-G covariances, RGB565, nearest palette entry per texel), BC3
 * takes its BC4 alpha block from the texels' alpha, BC1 drops alpha. */
int uvol_encode_texture_segments_st(uvol_ctx *ctx, const uint8_t *const *rgba, int n_segments, int n_layers,
                                    uint32_t width, uint32_t height, int inputs_on_device,
                                    uint8_t *const *outs, const size_t *caps, size_t *out_lens, int *status);
int uvol_transcode_texture_segments_st(uvol_ctx *ctx, const uint8_t *const *ktx2, const size_t *lens, int n_segments,
                                       uint8_t *const *out, size_t layer_cap, int outputs_on_device, int target, int *status);

/* ---- decode path, geometry half ----
 * Replaces what the stock player obtains from the draco WASM decoder per frame (reference src/V2/player.ts:101, :313-336):
 * Draco 2.2 TRIANGULAR_MESH / valence-edgebreaker files with the attribute decoders of the fixtures (position, tex-coord,
 * normal, optional generic) -> de-quantised values per attribute in decoding order + one entry index per corner, i.e. the
 * inverse of uvol_mesh. */
typedef struct uvol_decoded_mesh {
  /* in: capacities of the caller's buffers */
  uint32_t cap_faces;              /* idx_* hold 3 * cap_faces entries */
  size_t cap_values;               /* pos / nrm hold 3 * cap_values floats, uv 2 * cap_values (3 * n_faces always suffices) */
  /* in: caller buffers (any may be NULL to skip that output) */
  float *pos, *uv, *nrm;
  uint32_t *idx_pos, *idx_uv, *idx_nrm;
  /* out */
  uint32_t n_faces, n_pos, n_uv, n_nrm;
} uvol_decoded_mesh;
/* host-only: face count of a .drc and the value count that always suffices (UVOL_E_INVALID for foreign data) */
int uvol_drc_info(const uint8_t *drc, size_t len, uint32_t *n_faces, uint32_t *max_values);
/* n frames, one kernel launch per stage; status[i] per frame (may be NULL).  The arrays of `out` are caller-owned host memory: pageable arrays
 * are filled through the library's pinned double buffers (host threads copy out of them); arrays that ALL lie in uvol_host_alloc memory are
 * written by the DMA engines where they are (round 6: no staging, no host copy of the 10.5 MB a 100 k-vertex frame decodes to). */
int uvol_decode_mesh_batch(uvol_ctx *ctx, const uint8_t *const *drc, const size_t *lens, int n, uvol_decoded_mesh *out, int *status);
/* Same with the buffers of `out` in HBM (device pointers): the decoded arrays stay on the device - what a GPU-resident consumer
 * (a renderer's vertex buffers, or uvol_encode_mesh_batch_dev[_out] re-encoding them) reads without a host round trip.  The .drc
 * files themselves are host memory; counts come back in `out`. */
int uvol_decode_mesh_batch_dev(uvol_ctx *ctx, const uint8_t *const *drc, const size_t *lens, int n, uvol_decoded_mesh *out, int *status);

/* As uvol_decode_mesh_batch (outputs_on_device = 0) / uvol_decode_mesh_batch_dev (1), plus the material ids: face_material (may be NULL)
 * holds n entries, face_material[i] = NULL or out[i].cap_faces bytes (host / device memory like the arrays of `out`) that receive one id per
 * face, in the face order of idx_pos; has_material[i] (may be NULL) = 1 when the file carries a GENERIC uint8 1-component attribute with plain
 * integer values, either as a vertex attribute (decoder type 0, on the base corner table: what stock draco_encoder writes while no two
 * materials meet at a vertex) or in the CORNER form (decoder type 1, on the seam-cut table of its own attribute-data slot: what this encoder
 * writes with uvol_params.material_seams = 1 for a frame with interior material seams); else 0 and the buffer is left alone (a generic
 * attribute of another shape decodes as it always did and reports no material).  face_material[f] is the value at corner 3 f; this encoder
 * writes one id on all three corners of a face.  The corner form in slot 0 or 1 (a frame without tex-coords or without normals) is read off
 * the two seam-cut tables every call builds; in slot 2 (a frame with tex-coords and normals) the material has a third table, which the calls
 * that return materials - this one with face_material or has_material non-NULL, and uvol_decode_mesh_batch_packed - build in a pass of their
 * own, enqueued only when a file of the call carries such an attribute (the decoder rows are looked at on the host).
 * uvol_decode_mesh_batch, _dev and _points decode position, tex-coord and normal of such a file and skip the material's values.  Any other
 * corner attribute in a third slot is refused as before (status UVOL_E_ENCODE). */
int uvol_decode_mesh_batch_mat(uvol_ctx *ctx, const uint8_t *const *drc, const size_t *lens, int n, int outputs_on_device,
                               uvol_decoded_mesh *out, uint8_t *const *face_material, int *has_material, int *status);

/* ---- render-ready form of the geometry decode (additive: uvol_abi_version stays 1) ----
 * What the stock player obtains from its loader (reference src/lib/DRACOLoader.js:470-569: decodeGeometry / decodeIndex / decodeAttribute)
 * is ONE vertex array per attribute, all of num_points entries, plus one uint32 index per corner, which go straight into a BufferGeometry.
 * uvol_decode_mesh_batch hands back the inverse of uvol_mesh instead - a value count and an index stream per attribute -, which no
 * graphics API draws.  This entry point welds the three streams on the device (csrc/geo_weld.hpp):
 *   point    = a distinct tuple (idx_pos[c], idx_uv[c], idx_nrm[c]) over the corners c = 0 .. 3 * n_faces - 1, in exactly the face and corner
 *              order uvol_decode_mesh_batch returns; an attribute the file does not carry is left out of the tuple;
 *   numbering: points are numbered by FIRST APPEARANCE in that corner order - deterministic, and vertex order stays coherent with face
 *              order.  It is not Draco's own point numbering, which nothing at hand pins down (the recorded .drc files carry no point
 *              ids and the reference holds no decoder to run);
 *   values   : index[c] is the point of corner c; the values of point p are the bit-identical floats uvol_decode_mesh_batch produces for the
 *              entries of p's tuple (the weld adds no arithmetic).
 * Layouts: UVOL_POINTS_PLANAR - pos / uv / nrm receive 3 / 2 / 3 floats per point (any may be NULL to skip that output; the array of an
 * absent attribute is left alone); UVOL_POINTS_INTERLEAVED - `pos` is the one buffer, 32 bytes per point = pos[3] nrm[3]
 * uv[2], uv / nrm are ignored, the slot of an absent attribute is written as zeros.  has_uv / has_nrm say which attributes the file carries.
 * A DEVICE interleaved buffer must be 16-byte aligned (the kernels write it with 16-byte stores); host outputs are copied and need no
 * alignment.  An unknown layout or a misaligned device buffer in any frame is a mistake of the caller, not of a file: the whole call returns
 * UVOL_E_INVALID and nothing is decoded.
 * Capacity: n_points <= 3 * n_faces, so uvol_drc_info's max_values always suffices as cap_points.  Frames fail alone, status[i] (may be NULL:
 * the worst code is then the return value): a frame whose points exceed cap_points, or whose faces exceed cap_faces, gets UVOL_E_NOSPACE
 * with n_points / n_faces set to the count it needs and none of its arrays written; a foreign file (uvol_drc_info refuses it) UVOL_E_INVALID;
 * a corrupt one UVOL_E_ENCODE; one with a position entry shared by more than 4096 corners UVOL_E_UNSUPPORTED (every corner compares itself
 * against the corners of its position entry).  Sequential files (`-cl 0`) go through the same entry and come out under the same numbering.
 * Output memory as in the existing decode: device pointers when outputs_on_device (written in place by the weld kernels, no copy);
 * pageable host arrays through the pinned double buffers; arrays that ALL lie in uvol_host_alloc memory written by DMA where they are.
 * Out of scope on this float form: material ids (uvol_decode_mesh_batch_packed below carries them; uvol_decode_mesh_batch_mat returns them
 * per face, in the same face order); half-float vertex formats.  uvol_decode_mesh_batch, _dev and _mat are unchanged: they launch none
 * of the weld kernels and carve none of their scratch. */
enum { UVOL_POINTS_PLANAR = 0, UVOL_POINTS_INTERLEAVED = 1 };
typedef struct uvol_decoded_points {
  /* in */
  uint32_t cap_faces;              /* index holds 3 * cap_faces entries */
  size_t cap_points;               /* planar: pos / nrm hold 3 * cap_points floats, uv 2 * cap_points; interleaved: pos holds 8 * cap_points */
  uint32_t layout;                 /* UVOL_POINTS_PLANAR / UVOL_POINTS_INTERLEAVED */
  float *pos, *uv, *nrm;
  uint32_t *index;                 /* may be NULL */
  /* out */
  uint32_t n_faces, n_points;
  uint32_t has_uv, has_nrm;
} uvol_decoded_points;
int uvol_decode_mesh_batch_points(uvol_ctx *ctx, const uint8_t *const *drc, const size_t *lens, int n, int outputs_on_device,
                                  uvol_decoded_points *out, int *status);

/* ---- packed render-ready form: 16-byte records of the file's own integers, with material ids (additive: uvol_abi_version stays 1) ----
 * A .drc file stores positions and tex-coords as small integers (11 and 10 bits in every recorded file); the float form above turns them
 * into 32-bit floats and has no slot for the material id.  This entry point hands a renderer that feeds normalised-integer vertex formats
 * (KHR_mesh_quantization style) the integers themselves, exactly, in half the bytes.  Points, their numbering and `index` are those of
 * uvol_decode_mesh_batch_points on the same file.  Record of point p, 16 bytes, little endian:
 *   bytes  0 -  5   uint16 px, py, pz   the file's quantised position integers of p's position entry, unchanged
 *   bytes  6 -  7   uint16 material     the material id of p (0 when has_material is 0)
 *   bytes  8 - 11   uint16 u, v         the file's quantised tex-coord integers (zeros when the file has no tex-coords)
 *   bytes 12 - 15   int8 nx, ny, nz, 0  rintf(n[k] * 127.0f), round to nearest even, n = the float normal uvol_decode_mesh_batch_points returns
 *                                       for that entry, bit for bit (zeros when the file has no normals)
 * Dequantisation, all in IEEE binary32 with the product rounded BEFORE the sum (two roundings, no fused multiply-add):
 *   position k = pos_min[k] + (float)q[k] * pos_scale,   pos_scale = range / (float)((1u << pos_bits) - 1)
 *   tex-coord k = uv_min[k] + (float)q[k] * uv_scale,    uv_scale  = range / (float)((1u << uv_bits) - 1)
 * which reproduces the floats of uvol_decode_mesh_batch[_points] bit for bit (the checker's drc_dequant evaluates the same expression, built
 * with floating-point contraction off; tests/test_hipemu_packed.py asserts it against NumPy).  A shader that fuses the two differs by at
 * most one unit in the last place.  pos_min / uv_min are the attribute's minimum values as the file stores them.
 * Material: the attribute uvol_decode_mesh_batch_mat reads (GENERIC uint8, one component, plain integers, of an edgebreaker file), under the
 * same condition for has_material.  As a vertex attribute its entry is a function of the position entry, so it never splits a point.  As
 * a corner attribute (interior material seams) the corner's material value is a fourth member of the point tuple: a (position, tex-coord,
 * normal) tuple used by corners of different ids becomes one point per id, points are still numbered by first appearance in corner order
 * and n_points <= 3 n_faces still holds; where no tuple carries two ids, index and n_points are those of uvol_decode_mesh_batch_points.
 * `material` is the value at the point's first corner.  A generic attribute of any other shape: has_material = 0, slot zero.
 * records == NULL or index == NULL skips that output.  A DEVICE records buffer must be 16-byte aligned (one 16-byte store per point); a
 * misaligned one in any frame fails the whole call with UVOL_E_INVALID before anything runs.  Capacity and per-frame statuses as in the
 * float form: UVOL_E_NOSPACE (points or faces exceed the capacities: n_points / n_faces are the needed counts, nothing of the frame is
 * written), UVOL_E_INVALID (foreign file), UVOL_E_ENCODE (corrupt file), UVOL_E_UNSUPPORTED (a position entry shared by more than 4096
 * corners) and, of this form alone, UVOL_E_UNSUPPORTED for a position or tex-coord attribute that is not quantised or is quantised to more
 * than 16 bits (uvol_last_error names the attribute; nothing of the frame is written).  Sequential (`-cl 0`) files go through the same
 * entry.  Output memory: the three forms of the float entry point.  The float value arrays are neither carved nor written on this path. */
typedef struct uvol_packed_points {
  /* in */
  uint32_t cap_faces;              /* index holds 3 * cap_faces entries */
  size_t cap_points;               /* records holds 16 * cap_points bytes */
  void *records;                   /* 16 bytes per point, layout above; NULL skips it */
  uint32_t *index;                 /* one point id per corner; NULL skips it */
  /* out */
  uint32_t n_faces, n_points;
  uint32_t has_uv, has_nrm, has_material;
  uint32_t pos_bits, uv_bits;      /* quantisation bits of the file; uv_bits 0 when absent */
  float pos_min[3], pos_scale;     /* position k = pos_min[k] + q[k] * pos_scale */
  float uv_min[2], uv_scale;
} uvol_packed_points;
int uvol_decode_mesh_batch_packed(uvol_ctx *ctx, const uint8_t *const *drc, const size_t *lens, int n, int outputs_on_device,
                                  uvol_packed_points *out, int *status);

/* ---- measurement hooks (bench.py / rocprof cross-check) ---- */
/* When enabled, every kernel group is bracketed by hipEvents on the ctx stream. */
int uvol_profile_enable(uvol_ctx *ctx, int on);
int uvol_profile_reset(uvol_ctx *ctx);
/* Number of distinct kernel groups recorded so far. */
int uvol_profile_count(uvol_ctx *ctx);
/* name/launch-count/total-ms/algorithmic-bytes of group i (for the matrix-core sub-group tex.k10_sel_assign the last field
 * counts integer multiply/add operations instead of bytes). */
int uvol_profile_get(uvol_ctx *ctx, int i, char *name, size_t name_cap,
                     uint64_t *launches, double *total_ms, uint64_t *algo_bytes);

#ifdef __cplusplus
}
#endif
#endif /* UVOL_CODEC_H */
