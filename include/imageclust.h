/*
 * imageclust.h -- C-ABI of libimageclust_hip.so, the MI355X (gfx950) engine that stands in for the
 * embed + Ward-cluster hot path of monahand1023/imageclust.
 *
 * This is the drop-in boundary: plain pointers and sizes, int status codes, caller-owned outputs, no C++
 * exceptions, no torch types.  Each entry point names the reference interface it replaces (file:line under
 * /root/reference).  The Go binding a maintainer adds is shown in INTEGRATION.md and go/.
 *
 * Conventions
 *   - every function returns ICL_OK (0) or an ICL_ERR_* code; icl_last_error() gives the text.
 *   - matrices are row-major; "host" pointers are ordinary memory, "_dev" variants take device pointers that
 *     live on the context's GPU and are consumed on the context's stream (icl_stream()).
 *   - all entry points are thread-safe (a context serialises its own calls with a mutex): the reference calls
 *     GetImageEmbedding from N goroutines (internal/workflow/workflow.go:156-175).
 *   - one context drives ONE GPU.  Several GPUs: an icl_group (one process, one context + host thread per GPU, peer copies
 *     over xGMI), or one process per GPU with the icl_ward_* span calls and RCCL as the transport (bench.py).
 */
#ifndef IMAGECLUST_H
#define IMAGECLUST_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct icl_ctx icl_ctx;

enum {
    ICL_OK = 0,
    ICL_ERR_ARG = 1,         /* bad argument (null, negative size, unknown enum) */
    ICL_ERR_CONSTRAINT = 2,  /* clustering.go:204-207,175-177: constraints cannot be met -> (nil,false) */
    ICL_ERR_HIP = 3,         /* a HIP runtime call failed / no usable gfx950 device */
    ICL_ERR_NOMODEL = 4,     /* embed called before a model was loaded */
    ICL_ERR_IO = 5,          /* file missing / unreadable / malformed */
    ICL_ERR_UNSUPPORTED = 6, /* valid request this build cannot serve */
    ICL_ERR_OVERSIZE = 7,    /* a cluster above maxSize was observed (clustering.go:251; unreachable) */
    ICL_ERR_NOMEM = 8        /* out of host memory, or a device allocation (workspace, temporary, device copy of a host argument) does not fit */
};

enum { ICL_HEAD_POOLED = 2048, /* global-average-pool vector (north_star) */
       ICL_HEAD_DENSE0 = 1000  /* "resnetv17_dense0_fwd" (embeddings.go:140) */ };
enum { ICL_PREC_FP32 = 0,  /* f32 MFMA, parity mode (<=1e-4 vs the fp32 restatement) */
       ICL_PREC_BF16 = 1,  /* bf16 MFMA with fp32 accumulate, throughput mode */
       ICL_PREC_BF16X3 = 2 /* split bf16: operands as hi + lo bf16 pairs, three bf16 MFMAs per product (wh.xh + wl.xh + wh.xl) with fp32
                              accumulate; meets the parity bound (<=1e-4 vs the fp32 restatement; ~7e-6 measured).  33.1k img/s at batch 256,
                              2.2x ICL_PREC_FP32 (profiles/r06_embed_prec_rate.json).
                              Holds a third copy of the conv weights (~100 MB more device memory per context); ignores ICL_CONV_SPLIT */ };
enum { ICL_UPDATE_EXACT = 0, /* centroid recompute, bit-identical to clustering.go:76-96 */
       ICL_UPDATE_LW = 1     /* MFMA distance tile + Lance-Williams rows: fast, NOT bit-identical */ };
enum { ICL_SYNTH_NOISE = 0, ICL_SYNTH_STRUCTURED = 1 };

/* ---- context ------------------------------------------------------------------------------------------ */
int icl_create(int device_ordinal, icl_ctx **out);
void icl_destroy(icl_ctx *ctx);
/* Last error text of ctx (or of the calling thread's last failed icl_create when ctx == NULL). */
const char *icl_last_error(icl_ctx *ctx);
/* hipStream_t (as void*) every kernel of this context is launched on. */
void *icl_stream(icl_ctx *ctx);
int icl_sync(icl_ctx *ctx);
int icl_device_info(icl_ctx *ctx, char *name, int name_cap, int *n_cu, int64_t *hbm_bytes);
/* Device memory helpers for hosts that have no allocator of their own (Go shim, ctypes tests). */
int icl_dev_malloc(icl_ctx *ctx, int64_t bytes, void **dptr);
int icl_dev_free(icl_ctx *ctx, void *dptr);
int icl_memcpy_h2d(icl_ctx *ctx, void *dst_dev, const void *src_host, int64_t bytes);
int icl_memcpy_d2h(icl_ctx *ctx, void *dst_host, const void *src_dev, int64_t bytes);

/* ---- model: replaces LoadPretrainedModelONNX (internal/embeddings/embeddings.go:28-43) ------------------- */
/* Parse an ONNX file's initializers (no protobuf dependency) into the context. */
int icl_model_load_onnx(icl_ctx *ctx, const char *path);
/* The conversion step of the above alone (host only, no GPU): ONNX file -> ICLW blob; blob == NULL returns the size. */
int icl_onnx_to_blob_file(const char *path, void *blob, int64_t cap_bytes, int64_t *bytes);
/* Load an "ICLW" blob (include/icl_model_format.h). */
int icl_model_load_blob(icl_ctx *ctx, const void *blob, int64_t bytes);
/* Seeded synthetic ResNet50-v1 weights: generate on the host, then load. */
int icl_model_load_synthetic(icl_ctx *ctx, uint64_t seed);
int64_t icl_synthetic_blob_bytes(void);
int icl_synthetic_blob(uint64_t seed, void *blob, int64_t bytes); /* host only, no GPU needed */

/* ---- embed: replaces PreprocessImage + GetImageEmbedding (embeddings.go:46-116,119-163) ----------------- */
/* n images, each 224*224*3 u8, HWC, RGB (i.e. after the reference's resize + BGR->RGB).  out is n x head fp32.
 * head: ICL_HEAD_POOLED or ICL_HEAD_DENSE0.  prec: ICL_PREC_*.  Batches internally (default 256).
 * Host buffers (pageable memory is fine) are streamed through the GPU in slabs of 4096 images; the upload of the next slab
 * (a helper thread owned by the call) overlaps the forward passes of the current one.  The _dev variant takes device pointers. */
int icl_embed_u8(icl_ctx *ctx, const uint8_t *hwc_rgb, int64_t n, int head, int prec, float *out);
int icl_embed_u8_dev(icl_ctx *ctx, const uint8_t *d_hwc_rgb, int64_t n, int head, int prec, float *d_out);
/* One image file (baseline or progressive Huffman JPEG, PNG (progressive or Adam7-interlaced), or binary PPM "P6"): decode, bilinear resize to 224x224
 * (embeddings.go:69), then as icl_embed_u8 with n = 1, fp32. */
int icl_embed_file(icl_ctx *ctx, const char *path, int head, float *out);
/* icl_embed_file is what GetImageEmbedding(appCtx, path) binds to, and workflow.go:156-175 calls that from one goroutine per
 * image.  The file is read as icl_load_image_224 reads it (JPEG samplings: see icl_decode_image_file).  Concurrent callers are coalesced: each decodes / resizes its own file, then one forward pass serves everything
 * that queued up within window_us (or max_batch images).  prec selects ICL_PREC_FP32 (default: rows equal the one-at-a-time
 * result bit for bit), ICL_PREC_BF16X3 or ICL_PREC_BF16.  window_us = 0 disables waiting (a lone caller runs at once).
 * prec | ICL_FILE_FAIL_NEXT_LEADER: the next batch leader fails with ICL_ERR_NOMEM right after it has taken its queued requests --
 * every caller of that batch gets the error, nobody is left waiting (the recovery path of the queue, exercised by the test suite). */
enum { ICL_FILE_FAIL_NEXT_LEADER = 0x100 };
int icl_set_file_options(icl_ctx *ctx, int prec, int window_us, int max_batch);
int icl_file_batch_stats(icl_ctx *ctx, int64_t *batches, int64_t *images); /* forward passes run / images served by icl_embed_file */
/* Image ingest on the host (embeddings.go:50-82): decode a file (baseline or progressive Huffman JPEG, PNG, or binary PPM) to interleaved RGB.
 * With rgb == NULL only *w / *h are returned.  cap_bytes must be >= w*h*3.
 * JPEG: 8 bit, 1 component, or 3 with 1x1 chroma and luma sampling 1x1 (4:4:4), 2x1 (4:2:2), 2x2 (4:2:0), 1x2 (4:4:0: a 4:2:2 file after a
 * lossless 90-degree rotation), 4x1 or 1x4 (4:1:1, either way up); pixels are libjpeg-turbo's with its default settings.  Any other
 * sampling (4:1:0, subsampled luma, ...), CMYK, arithmetic coding, lossless and 12 bit return ICL_ERR_UNSUPPORTED; for a sampling the
 * message names the factors found.  Every file entry point below reads JPEGs through this decoder's frame header. */
int icl_decode_image_file(const char *path, uint8_t *rgb, int64_t cap_bytes, int32_t *w, int32_t *h);
/* decode + cv::resize(INTER_LINEAR)-compatible resize to 224x224 (embeddings.go:50,69): out is 224*224*3 u8 RGB. */
int icl_load_image_224(const char *path, uint8_t *out);
/* PreprocessImage alone: the 1x3x224x224 fp32 NCHW blob of embeddings.go:96-108 (host). */
int icl_preprocess_u8(const uint8_t *hwc_rgb, float *nchw);
/* PreprocessImage(imagePath) (embeddings.go:46-116) end to end on the host: IMRead (EXIF orientation applied, as cv::imread
 * does) -> cv::resize(224x224, INTER_LINEAR; exact 2x2 decimation takes OpenCV's INTER_AREA path) -> RGB/255 NCHW fp32. */
int icl_preprocess_file(const char *path, float *nchw);
/* The resize step alone (embeddings.go:69) on an interleaved u8 RGB image: cv::resize(src, dst, (dw, dh), 0, 0, INTER_LINEAR). */
int icl_resize_u8(const uint8_t *src_rgb, int32_t sw, int32_t sh, uint8_t *dst_rgb, int32_t dw, int32_t dh);
/* ---- batched file ingest: replaces the per-file decode of GetImageEmbedding (embeddings.go:46-116) as workflow.go:149-185 calls it ----
 * paths[0..n): JPEG / PNG / PPM files, as icl_load_image_224 reads them (every JPEG sampling icl_decode_image_file lists is rebuilt on
 * the GPU: 4:4:4, 4:2:2, 4:2:0, 4:4:0 and 4:1:1 files all count under gpu_jpegs).  threads: host decode threads
 * (0 = min(16, hardware threads)).  status[i] = ICL_OK or the ICL_ERR_* code of file i (may be NULL).
 * Returns ICL_OK when every file was read, else ICL_ERR_IO / _UNSUPPORTED naming the LOWEST failed
 * index in icl_last_error; rows of failed files are NaN.  Row i always belongs to paths[i].
 * Host workers parse each JPEG and run its entropy decoder (stage A); the GPU dequantises, runs the islow IDCT, upsamples the
 * chroma, converts the colour, applies the EXIF orientation and resizes to 224x224, bit-identical to icl_load_image_224.  PNG, PPM
 * and JPEGs too large for one staging slab are decoded and resized on the host.  Output does not depend on threads.
 * icl_load_images_224_dev: d_out (device, on the context's stream) gets n x 224x224x3 u8 RGB rows, each equal to what
 * icl_load_image_224 gives for its file; a failed file's row is left all ZERO (the u8 form of "NaN").  No model needed. */
int icl_load_images_224_dev(icl_ctx *ctx, const char *const *paths, int64_t n, int32_t threads,
                            uint8_t *d_out /* n x 224x224x3 */, int32_t *status);
/* replaces the loop of GetImageEmbedding calls of workflow.go:149-185: out (host) is n x head fp32, each row equal to icl_embed_u8 on
 * the icl_load_image_224 output of its file; rows of failed files are NaN.  The _dev variant writes d_out on the device. */
int icl_embed_files(icl_ctx *ctx, const char *const *paths, int64_t n, int head, int prec,
                    int32_t threads, float *out, int32_t *status);
int icl_embed_files_dev(icl_ctx *ctx, const char *const *paths, int64_t n, int head, int prec,
                        int32_t threads, float *d_out, int32_t *status);
/* what the last files call did: JPEGs rebuilt on the GPU, files decoded on the host (PNG, PPM, fallbacks; with ICL_PNG_GPU a PNG
 * decoded on the GPU is counted by icl_last_png_stats instead),
 * bytes uploaded, host thread-seconds spent in stage A / host decode */
int icl_last_ingest_stats(icl_ctx *ctx, int64_t *gpu_jpegs, int64_t *host_files, int64_t *upload_bytes,
                          double *host_decode_s);
/* ---- entropy decoding on the GPU (opt-in) ----
 * ICL_ENTROPY_HOST (default): host workers run stage A (parsing + Huffman decoding) of every JPEG, as described above.
 * ICL_ENTROPY_GPU: for a sequential Huffman JPEG (SOF0 / SOF1, 8 bit) whose ONE scan carries all components (1, or 3 at 4:4:4 / 4:2:2 /
 * 4:2:0 / 4:4:0 / 4:1:1, i.e. every sampling the host decoder reads: 3, 4 or 6 blocks per MCU; with or without restart interval) a host worker only parses the markers and unstuffs the entropy-coded segment; kernels decode
 * it in fixed-size subsequences and accept the result only when the chain of subsequence states is consistent and the stream is clean,
 * which makes it the sequential decode.  Every other file, and every image the check rejects (damaged, truncated, odd streams), takes the
 * ICL_ENTROPY_HOST route; rows, status codes and messages are identical in both modes.  The environment variable ICL_JPEG_ENTROPY=gpu
 * selects ICL_ENTROPY_GPU when the context is created. */
enum { ICL_ENTROPY_HOST = 0, ICL_ENTROPY_GPU = 1 };
int icl_set_ingest_options(icl_ctx *ctx, int entropy_mode);
/* what the last files call did with its JPEGs: entropy-decoded on the GPU and accepted, entropy-decoded by host stage A because of the
 * routing rule (progressive, one scan per component, too large, or ICL_ENTROPY_HOST), rejected by the GPU check and redone by the host
 * route, bytes of unstuffed stream uploaded */
int icl_last_entropy_stats(icl_ctx *ctx, int64_t *gpu_entropy_jpegs, int64_t *host_entropy_jpegs, int64_t *redone_on_host,
                           int64_t *stream_bytes);
/* Test hooks: the quantised coefficients as stage A leaves them (per component 0, 1, 2: wblocks x hblocks blocks of 64 int16 in natural
 * order, not dequantised).  state[i] / info[0]: 1 = decoded and accepted, 0 = rejected by the chain / cleanliness check (no
 * coefficients), -1 = the file does not qualify for the GPU decoder (no coefficients; never with ICL_ENTROPY_HOST).
 * icl_jpeg_coefs_files: file i's coefficients go to coefs[offsets[i] .. offsets[i + 1]) (host memory, cap elements); entropy_mode
 * chooses host stage A or the GPU decoder.  With coefs == NULL only offsets[0..n] are computed (and with ICL_ENTROPY_GPU nothing is
 * decoded: state is 0 for every qualifying file).  A rejected file keeps its range, unwritten.  A file stage A cannot read fails the call.
 * icl_jpeg_coefs_file_host: no GPU.  sub_bits == 0: host stage A; otherwise stage A0 and the GPU decoder's schedule as a host loop over
 * subsequences of sub_bits bits (a multiple of 32).  *need receives the element count; coefs may be NULL.  info[8]: state, components,
 * blocks of component 0, 1, 2, rounds the slowest workgroup needed, subsequences, restart intervals. */
int icl_jpeg_coefs_files(icl_ctx *ctx, const char *const *paths, int64_t n, int entropy_mode, int16_t *coefs, int64_t cap,
                         int64_t *offsets /* n + 1 */, int32_t *state /* n */);
int icl_jpeg_coefs_file_host(const char *path, int sub_bits, int16_t *coefs, int64_t cap, int64_t *need, int32_t *info /* 8 */);
/* ---- PNG on the GPU (opt-in) ----
 * ICL_PNG_HOST (default): a host worker decodes a PNG whole (icl_decode_image_file's code) and resizes it; only the 224x224 row is
 * uploaded.  ICL_PNG_GPU: for a PNG that QUALIFIES -- its chunks parse (signature, CRCs, IHDR, PLTE, IDAT, IEND, zlib header), it is
 * not Adam7-interlaced, its zlib stream fits one staging slab (128 MiB) and its scanlines, height x (1 + row bytes), are at most 512 MiB
 * -- a host worker only parses the chunks and copies the zlib stream; kernels inflate it (one workgroup per image), check the
 * Adler-32, undo the scanline filters and resize from the scanlines.  All five colour types at every legal depth qualify.  The GPU
 * accepts an image only when the final block ended with exactly the expected byte count from a legal stream (the host decoder's rules),
 * the Adler-32 matches, every filter byte is 0..4 and no palette index is out of range; every image it rejects, and every file that
 * does not qualify, takes the ICL_PNG_HOST route, which also owns every status code and message.  Rows, status codes and messages are
 * identical in both modes.  Counters: a PNG decoded on the GPU is counted in gpu_pngs (icl_last_png_stats) and NOT in host_files
 * (icl_last_ingest_stats); gpu_jpegs stays JPEG-only.  icl_embed_file, the single-file calls and icl_downsize_images keep PNG on the
 * host.  The environment variable ICL_PNG_INFLATE=gpu selects ICL_PNG_GPU when the context is created. */
enum { ICL_PNG_HOST = 0, ICL_PNG_GPU = 1 };
int icl_set_png_options(icl_ctx *ctx, int png_mode);
/* what the last files call did with its PNGs: decoded on the GPU and accepted, decoded by the host because of the routing rule (does
 * not qualify, or ICL_PNG_HOST), rejected by the GPU check and redone by the host route, zlib stream bytes uploaded */
int icl_last_png_stats(icl_ctx *ctx, int64_t *gpu_pngs, int64_t *host_pngs, int64_t *redone_on_host, int64_t *stream_bytes);
/* Test hooks.  stage 0: the inflated stream (filter bytes + filtered scanlines); stage 1: after unfiltering (filter bytes kept); the
 * host hooks also know stage 2: the sample-to-RGB rule on every pixel (w x h x 3).  state[i] / info[0]: 1 accepted, 0 rejected by the
 * GPU check (no bytes), -1 the file does not qualify (no bytes).
 * icl_png_raw_files: file i's bytes go to raw[offsets[i] .. offsets[i + 1]) (host memory, cap bytes); one single-image slab per file
 * through the pipeline's own placement and launch code.  With raw == NULL only offsets[0..n] are computed and nothing is decoded (state
 * is 0 for every qualifying file).  A rejected file keeps its range, unwritten.
 * icl_png_raw_file_host / icl_png_raw_mem_host: no GPU; the kernels' schedule run as a host loop over the same __host__ __device__
 * functions.  *need receives the byte count (0 unless accepted); raw may be NULL.  info[12]: state, w, h, depth, colour type, stored /
 * fixed / dynamic block counts, longest code length seen, largest match distance, matches with distance < length, matches whose
 * destination wraps the 32 KiB ring. */
int icl_png_raw_files(icl_ctx *ctx, const char *const *paths, int64_t n, int stage, uint8_t *raw, int64_t cap, int64_t *offsets /* n + 1 */,
                      int32_t *state /* n */);
int icl_png_raw_file_host(const char *path, int stage, uint8_t *raw, int64_t cap, int64_t *need, int32_t *info /* 12 */);
int icl_png_raw_mem_host(const uint8_t *data, int64_t bytes, int stage, uint8_t *raw, int64_t cap, int64_t *need, int32_t *info /* 12 */);
int icl_set_batch(icl_ctx *ctx, int batch); /* embed batch size, 1..1024 */
/* Which bf16 convolution launches take the deep-pipelined 256 x 256 x 64 kernel (conv_p8_kernel: LDS-DMA kept in flight across raw
 * barriers, counted vmcnt, staggered wave groups) instead of the 128 x 128 two-stage kernels: ICL_CONV_P8_OFF never, ICL_CONV_P8_AUTO
 * (default; the environment variable ICL_CONV_P8 = 0/1/2 overrides the default when the context is created) the layers with K >= 256,
 * ICL_CONV_P8_ALL every shape the kernel supports (Cout % 128 == 0, K % 128 == 0;
 * the per-layer parity tests run small shapes through it this way).  Results are those of the same bf16 arithmetic in a different
 * summation order (fp32 accumulation); the fp32 parity path is not affected. */
/* ICL_CONV_SPLIT (or-ed into p8_mode; environment: ICL_CONV_SK=1; default off): a LATENCY mode for callers with one forward pass in flight or
 * small batches.  The 7 x 7 layers (Ho * Wo <= 49, K % 256 == 0, K >= 2048, Cout % 256 == 0: 0.38 tiles of 256 x 256 per image, 98 per batch of 256 on
 * 256 CUs) then run every tile on TWO workgroups, each over half of K; the second adds the first one's fp32 sums in a fixed order, so results
 * are deterministic and do not depend on the batch (the rule looks at the layer's shape only), but differ from the default's in the last bits
 * (another summation order).  Measured (profiles/r05_conv_split_ab.txt): a single-stream forward pass of 256 images 3 476 -> 3 277 us, the
 * three 3x3 layers of stage 4 321 -> 227 us; with two passes in flight -- the throughput configuration, where the idle CUs are the other
 * pass's -- the embedding is 1.1-1.5 % SLOWER, hence not the default. */
enum { ICL_CONV_P8_OFF = 0, ICL_CONV_P8_AUTO = 1, ICL_CONV_P8_ALL = 2, ICL_CONV_SPLIT = 16 };
int icl_set_conv_options(icl_ctx *ctx, int p8_mode);
/* Dead pixels of the bf16 forward pass (default on; the environment variable ICL_PRUNE = 0/1 overrides the default when the context is
 * created): block 0 of stages 2-4 reads the tensor in front of it through 1x1 / pad 0 / stride 2 convolutions only, i.e. at the pixels
 * (2 oy, 2 ox).  With the option on, the bottleneck in front of such a block runs its 3x3 convolution at that stride and its last 1x1
 * convolution over the quarter of the pixels that is read, written to their places in the full-size tensor; the other pixels of that
 * tensor are not written.  Every value that is computed is computed by the same kernel in the same order: embeddings and the tensors of
 * icl_embed_taps (a tapped tensor is always computed whole) are bit-identical with the option on and off.  ICL_PREC_FP32 and
 * ICL_PREC_BF16X3 are not affected.  icl_forward_prune_stats: bottlenecks run in the pruned form since the context was created. */
int icl_set_forward_prune(icl_ctx *ctx, int on);
int icl_forward_prune_stats(icl_ctx *ctx, int64_t *pruned_blocks);
/* The same rule on a bottleneck that runs as ONE fused launch (stage 1's last block, in front of stage 2's block 0): the launch takes the
 * instantiation that computes the 3x3 and the last 1x1 convolution for the pixels (2 oy, 2 ox) only and stores only those; bit-identical
 * results.  Default on (environment: ICL_PRUNE_FUSED = 0/1); in effect only while icl_set_forward_prune is on, which turns both parts off.
 * icl_forward_prune_fused_stats: such launches of the forward pass since the context was created (icl_forward_prune_stats does not count them). */
int icl_set_forward_prune_fused(icl_ctx *ctx, int on);
int icl_forward_prune_fused_stats(icl_ctx *ctx, int64_t *pruned_launches);
/* For the tests of the stem kernels (stem2_pool_kernel, stem_pool_kernel, stem_conv_kernel): at most max_blocks workgroups in their
 * persistent grid, in icl_stem_pool and in the forward pass alike, so that a workgroup walks several work units -- the unit-to-unit
 * transition, the carried conv row, the prefetch across an image boundary -- at a batch of one to three images.  0 (the default): no cap,
 * every launch is what it is without this call.  Results do not depend on the grid. */
int icl_set_stem_max_blocks(icl_ctx *ctx, int max_blocks);
/* Launches of the split form since the context was created. */
int icl_conv_split_launches(icl_ctx *ctx, int64_t *launches);
/* Convolution launches since the context was created: on conv_p8_kernel / on every other convolution kernel (either pointer may be NULL). */
int icl_conv_stats(icl_ctx *ctx, int64_t *p8_launches, int64_t *other_launches);
/* One fused convolution layer of the engine (the unit every ResNet50 conv is lowered to), host buffers:
 * y = relu?( conv(x, w) * scale[c] + shift[c] (+ residual) ).  x: [B][H][H][Cin] NHWC fp32, w: [Cout][Cin][k][k]
 * (OIHW, as in the ONNX initializer), residual / y: [B][Ho][Ho][Cout] NHWC fp32.  Needs Cin % 64 == 0 and
 * Cout % 64 == 0.  Operands are rounded to bf16 when prec == ICL_PREC_BF16, split into hi + lo bf16 pairs when prec == ICL_PREC_BF16X3. */
int icl_conv2d_fused(icl_ctx *ctx, int prec, const float *x, int B, int H, int Cin, const float *w, int Cout, int k,
                     int stride, int pad, const float *scale, const float *shift, const float *residual, int relu,
                     float *y);

/* The dual-operand launch that computes block 0 of stages 2-4 (a bottleneck's last 1x1 convolution and its downsample branch in one
 * launch), host buffers, for the parity tests: y = relu?( (x . w1 + x2[:, ::stride2, ::stride2] . w2) * scale[c] + shift[c] ).
 * x: [B][Ho][Ho][Cin], w1: [Cout][Cin], x2: [B][H2][H2][Cin2], w2: [Cout][Cin2], y: [B][Ho][Ho][Cout], all fp32, NHWC.  Needs
 * (Ho - 1) * stride2 < H2 (ICL_ERR_ARG otherwise), Cin % 64 == 0, Cin2 % 64 == 0 and Cout % 128 == 0 (ICL_ERR_UNSUPPORTED).  The kernel
 * is chosen as in the forward pass (icl_set_conv_options); operands are stored as icl_conv2d_fused stores them. */
int icl_conv2d_dual(icl_ctx *ctx, int prec, const float *x, int B, int Ho, int Cin, const float *w1, const float *x2, int H2, int Cin2,
                    const float *w2, int stride2, int Cout, const float *scale, const float *shift, int relu, float *y);
/* The mapped launch of a pruned bottleneck's last 1x1 convolution (icl_set_forward_prune), host buffers, bf16 operands, for the per-layer
 * tests: x [B][Ho][Ho][Cin] with Ho = (H - 1) / sub + 1, w [Cout][Cin], residual (or NULL) and y [B][H][H][Cout], all fp32 NHWC.
 * y[b][sub oy][sub ox][c] = relu?( (x[b][oy][ox] . w[c]) * scale[c] + shift[c] (+ residual[b][sub oy][sub ox][c]) ); y is read and written:
 * every other value comes back as it went in, rounded to bf16.  Cin = 128 with Cout % 256 == 0, or Cin = 256 with Cout % 128 == 0
 * (ICL_ERR_UNSUPPORTED otherwise: no other kernel stands behind this entry point). */
int icl_conv1x1_mapped(icl_ctx *ctx, const float *x, int B, int H, int sub, int Cin, const float *w, int Cout, const float *scale,
                       const float *shift, const float *residual, int relu, float *y);
/* The forward pass of the loaded model on ONE batch of B images (B <= icl_set_batch's batch), ended at a tap, for the per-block parity
 * tests: out receives, as fp32 NHWC, the tensor the pass holds after the stem + maxpool (tap 0: [B][56][56][64]) or after bottleneck
 * tap (1..16: [B][56][56][256] x 3, [B][28][28][512] x 4, [B][14][14][1024] x 6, [B][7][7][2048] x 3).  Same kernels, order and
 * buffers as icl_embed_u8. */
int icl_embed_taps(icl_ctx *ctx, int prec, const uint8_t *hwc_rgb, int B, int tap, float *out);

/* The two cross-layer fusions of the forward pass (the reference's OpenCV-DNN fuses layers inside Net.Forward,
 * embeddings.go:141), exposed one at a time for the per-layer parity tests, host buffers:
 * icl_stem_pool: conv0 7x7/2 + BN + ReLU + maxpool 3x3/2 of the LOADED model in one launch.  img: B x 224x224x3 u8 HWC RGB,
 * out: [B][56][56][64] NHWC fp32.
 * icl_bottleneck56: one whole stage-1 bottleneck in one launch (bf16 operands, fp32 accumulate; t1 / t2 rounded to bf16 as the
 * layer-by-layer bf16 path stores them).  wds == NULL (Cin = 256): y = relu(bn3(conv3(relu(bn2(conv2_3x3(relu(bn1(conv1(x)))))))) + x);
 * wds != NULL (Cin = 64): y = relu(bn3(conv3(t2)) + bn_ds(conv_ds(x))).  x: [B][H][W][Cin] NHWC, w1: [64][Cin], w2: [64][64][3][3]
 * (OIHW), w3: [256][64], wds: [256][Cin], sc / sh: folded BatchNorm scale / shift per output channel, y: [B][H][W][256]. */
int icl_stem_pool(icl_ctx *ctx, int prec, const uint8_t *hwc_rgb, int B, float *out);
int icl_bottleneck56(icl_ctx *ctx, const float *x, int B, int H, int W, int Cin, const float *w1, const float *sc1, const float *sh1,
                     const float *w2, const float *sc2, const float *sh2, const float *w3, const float *sc3, const float *sh3,
                     const float *wds, const float *scds, const float *shds, float *y);
/* icl_bottleneck56's identity form (Cin = 256) with the launch's sub: 1 computes every pixel, 2 is the pruned instantiation, which writes the
 * pixels (2 oy, 2 ox) only.  Every 16-bit element of the device tensor y holds `fill` (0 .. 0xffff, a bf16 bit pattern) when the kernel
 * starts, so a pixel the launch does not write comes back as that pattern (widened to fp32). */
int icl_bottleneck56_sub(icl_ctx *ctx, const float *x, int B, int H, int W, const float *w1, const float *sc1, const float *sh1,
                         const float *w2, const float *sc2, const float *sh2, const float *w3, const float *sc3, const float *sh3,
                         int sub, int fill, float *y);

/* ---- several GPUs behind one handle ------------------------------------------------------------------
 * workflow.go:89,161 run in ONE process: a group drives ndev contexts from ndev host threads.  embed shards the images by
 * contiguous index ranges; cluster builds the initial distance matrix (clustering.go:61-73) on GPU 0 alone (matrix-core bounds)
 * or, from 6 GPUs on, on every GPU in area-balanced runs of 128-row tile rows that GPU 0 reads out of its peers' memory over
 * xGMI straight into its matrix (icl_group_set_options), and runs the exact merge loop on GPU 0.  Outputs are bit-identical to
 * the single-GPU calls.  devices[] entries may repeat (tests on a 1-GPU box). */
typedef struct icl_group icl_group;
int icl_group_create(const int32_t *devices, int32_t ndev, icl_group **out);
void icl_group_destroy(icl_group *g);
int32_t icl_group_size(icl_group *g);
icl_ctx *icl_group_ctx(icl_group *g, int32_t i); /* borrowed: context of GPU i for per-device calls */
const char *icl_group_last_error(icl_group *g);
int icl_group_load_onnx(icl_group *g, const char *path);
int icl_group_load_blob(icl_group *g, const void *blob, int64_t bytes);
int icl_group_load_synthetic(icl_group *g, uint64_t seed);
int icl_group_embed_u8(icl_group *g, const uint8_t *hwc_rgb, int64_t n, int head, int prec, float *out);
int icl_group_cluster(icl_group *g, const float *E, int64_t n, int32_t d, int32_t min_size, int32_t max_size, int update,
                      int32_t *cluster_id, int32_t *member_rank, int32_t *n_clusters);
/* workflow.go:84-94 in ONE call -- createEmbeddings (:149-185) then PerformClusteringWithConstraints (:89) -- with the
 * embeddings staying on the GPUs in between: every GPU embeds its shard of the n images (2048-d pooled head) into its own copy
 * of E, the shards are exchanged by peer copies (xGMI), the distance rows are built on all GPUs and the merge loop runs on
 * GPU 0.  Nothing crosses PCIe between embed and cluster.  E_out (host, n x 2048) may be NULL.  Bit-identical to
 * icl_embed_u8 + icl_cluster on one GPU. */
int icl_group_embed_cluster(icl_group *g, const uint8_t *hwc_rgb, int64_t n, int prec, int32_t min_size, int32_t max_size, int update,
                            float *E_out, int32_t *cluster_id, int32_t *member_rank, int32_t *n_clusters);

/* Who builds the initial distance matrix of a group (clustering.go:61-73): ICL_TILES_AUTO (default) lets GPU 0 build all of it
 * wherever it can use the integer GEMM (D <= 2048: 63 ms at n = 100 000, as long as receiving the rows would take) and below 4 GPUs;
 * from 4 GPUs on the f32 bound rows (D > 2048) are dealt out (flagged bounds, computed by every GPU with the same GEMM: 0.15 s / G of
 * compute + 20 GB (G - 1) / G over one xGMI link per sender against 0.15 s locally: DESIGN.md 6); ICL_TILES_LOCAL /
 * ICL_TILES_DISTRIBUTED force either.  Results do not depend on it. */
enum { ICL_TILES_AUTO = 0, ICL_TILES_LOCAL = 1, ICL_TILES_DISTRIBUTED = 2 };
/* Where the exact merge loop (clustering.go:220-246) runs.  ICL_MERGE_GPU0 (default): on GPU 0.  ICL_MERGE_SHARDED: on every GPU at
 * once -- each holds a replica of the whole state (its own 4 n^2-byte distance matrix) and computes only every G-th 64-cluster
 * block of UpdateDistanceMatrix's new rows (clustering.go:76-96); after each update launch the replicas read the other blocks'
 * entries out of each other's matrices (peer access over xGMI) and finish the step identically.  The per-step vector arithmetic
 * divides by the number of GPUs; cluster ids, member order and merge log stay bit-identical.  At most 16 GPUs. */
enum { ICL_MERGE_GPU0 = 0, ICL_MERGE_SHARDED = 1 };
int icl_group_set_options(icl_group *g, int tiles_mode, int merge_mode);

/* The building blocks of the above, for callers that bring their own transport (bench.py: one process per GPU, RCCL
 * send/recv).  TRANSPORT FORMAT of distance rows: rows [row_lo, row_hi) of the packed lower triangle (row r = r floats, padded
 * to 4) are ONE contiguous span of floats.  The clustering GPU lays spans it can READ -- a landing buffer of its own that a
 * transport has just filled (any run of whole rows: bounded pieces), or a peer GPU's memory (hipDeviceEnablePeerAccess: the reads
 * cross xGMI) -- straight into its distance matrix with icl_ward_unpack_spans_dev; nothing is staged, so the clustering GPU holds the
 * matrix (4 n^2 bytes; rows and columns are recycled during the merge loop, ward.hip) plus O(n d) whatever the number of parts.
 * The rows it computes itself are the own_lo / own_hi of icl_cluster_prefilled_dev (matrix-core bounds, as in icl_cluster_dev).
 * Since round 5 the delivered rows hold the same kind of entries: with bounds in use (ICL_DIST_AUTO from n = 4096, ICL_DIST_BOUND / _LWBOUND)
 * icl_ward_distance_rows_dev runs the f32 matrix-core GEMM of the single-GPU path (0.15 s / G at n = 100 000 instead of 0.49 s / G of exact
 * vector arithmetic) and the span carries flagged lower bounds; every context of a job must carry the same icl_set_ward_options (a
 * clustering call that takes foreign rows as values checks them for flagged entries and fails with ICL_ERR_ARG). */
int icl_ward_rows_partition(int64_t n, int32_t parts, int32_t part, int64_t *row_lo, int64_t *row_hi); /* area-balanced, whole 128-row tile rows */
int icl_ward_span(int64_t row_lo, int64_t row_hi, int64_t *float_off, int64_t *float_cnt);             /* where that span sits / how long it is */
int icl_ward_distance_rows_dev(icl_ctx *ctx, const float *d_E, int64_t n, int32_t d, int64_t row_lo, int64_t row_hi, float *d_span);
int icl_ward_rows_hold_bounds(icl_ctx *ctx, int64_t n, int32_t d); /* 1: icl_ward_distance_rows_dev writes flagged matrix-core lower bounds (the clustering call makes them exact on demand), 0: exact values */
int icl_ward_prepare(icl_ctx *ctx, int64_t n, int32_t d);                                              /* allocate the clustering workspace */
int icl_ward_unpack_spans_dev(icl_ctx *ctx, int32_t nspans, const int64_t *row_lo, const int64_t *row_hi, const float *const *d_spans); /* spans -> matrix rows */
int icl_cluster_prefilled_dev(icl_ctx *ctx, const float *d_E, int64_t n, int32_t d, int32_t min_size, int32_t max_size, int update,
                              int64_t own_lo, int64_t own_hi, int32_t *cluster_id, int32_t *member_rank, int32_t *n_clusters);

/* ---- Ward clustering: replaces internal/clustering/clustering.go --------------------------------------- */
/* CalculateOptimalClusters (clustering.go:168-186). ICL_ERR_CONSTRAINT on the reference's error branches. */
int icl_calc_optimal_clusters(int64_t total, int64_t min_size, int64_t max_size, int64_t *k);
/* ComputeInitialDistanceMatrix (clustering.go:61-73) for n clusters with centroids C (n x d) and sizes
 * (NULL = all 1).  D is n x n with leading dimension ld, symmetric, diagonal 0.  Bit-identical. */
int icl_ward_distance_matrix(icl_ctx *ctx, const float *C, const int32_t *sizes, int64_t n, int32_t d, float *D,
                             int64_t ld);
int icl_ward_distance_matrix_dev(icl_ctx *ctx, const float *d_C, const int32_t *d_sizes, int64_t n, int32_t d,
                                 float *d_D, int64_t ld);
/* Centroid of MergeClusters(a,b) (clustering.go:37-40): (float(sa)*Ca + float(sb)*Cb)/float(sa+sb), host pointers. */
int icl_merge_centroid(icl_ctx *ctx, const float *ca, int64_t sa, const float *cb, int64_t sb, int32_t d, float *out);
/* UpdateDistanceMatrix (clustering.go:76-96) incl. RemoveRowsAndColumns (:100-116), host pointers.  D: n x n before the merge
 * (leading dimension ld); r1, r2: positions of the merged clusters; C / sizes: the (n-1) clusters AFTER RemoveClusters +
 * append (:240-241), new cluster last; Dout: (n-1) x (n-1), leading dimension ldout.  Bit-identical. */
int icl_update_distance_matrix(icl_ctx *ctx, const float *D, int64_t n, int64_t ld, const float *C, const int32_t *sizes,
                               int32_t d, int64_t r1, int64_t r2, float *Dout, int64_t ldout);
/* FindClosestClusters (clustering.go:119-133): first strict minimum of the lower triangle in row-major
 * order; (-1,-1) if none is < MaxFloat32. */
int icl_find_closest(icl_ctx *ctx, const float *D, int64_t n, int64_t ld, int64_t *i, int64_t *j);
int icl_find_closest_dev(icl_ctx *ctx, const float *d_D, int64_t n, int64_t ld, int64_t *i, int64_t *j);
/* PerformClusteringWithConstraints (clustering.go:198-284) on E (n x d).  Canonical output:
 * cluster_id[i] = dense id of the kept cluster of image i, or -1 if its cluster was dropped (< min_size);
 * member_rank[i] = position of image i in that cluster's member list.  Returns ICL_ERR_CONSTRAINT for the
 * reference's (nil,false). */
int icl_cluster(icl_ctx *ctx, const float *E, int64_t n, int32_t d, int32_t min_size, int32_t max_size, int update,
                int32_t *cluster_id, int32_t *member_rank, int32_t *n_clusters);
int icl_cluster_dev(icl_ctx *ctx, const float *d_E, int64_t n, int32_t d, int32_t min_size, int32_t max_size,
                    int update, int32_t *cluster_id, int32_t *member_rank, int32_t *n_clusters);
/* Many independent PerformClusteringWithConstraints calls (clustering.go:198-284) in one, exact mode only -- the serving pattern of
 * the reference, where every request clusters its own few hundred images.  Problem p clusters n[p] rows of d[p] floats that start at
 * float offset e_off[p] of E (rows contiguous); E holds e_len floats and every problem's rows must lie inside it.  Problem p's images
 * occupy [img_off(p), img_off(p) + n[p]) of cluster_id / member_rank, where img_off(p) = n[0] + ... + n[p-1].  Per problem, the results
 * are exactly what icl_cluster(E_p, n[p], d[p], min_size[p], max_size[p], ICL_UPDATE_EXACT) gives: cluster_id, member_rank,
 * n_clusters[p] and the merge log, bit for bit.  status[p] = ICL_OK or that problem's error (ICL_ERR_CONSTRAINT for the reference's
 * (nil,false)); a failed problem's rows are -1 and its n_clusters[p] and n_merges[p] are 0.  merges (may be NULL): problem p's merge
 * log, pairs of creation ids as icl_last_merges gives them, at offset 2*img_off(p); n_merges[p] holds its length in pairs.
 * Returns ICL_OK when every problem succeeded; otherwise the code of the LOWEST failed problem, which icl_last_error names.  A bad
 * argument (null pointer, nprob < 0, e_len < 0, negative n or d, rows outside E) returns ICL_ERR_ARG and writes nothing.  Problems of
 * up to 256 rows run together, one workgroup each (ward_many.hip); larger ones, and a lone small one, run one at a time on the whole
 * GPU, as icl_cluster does.
 * The call leaves what icl_last_merges, icl_last_merge_values and icl_last_ward_* report about the last icl_cluster unchanged.
 * The _dev variant takes E (e_len floats) on the context's device; everything else stays in host memory. */
int icl_cluster_many(icl_ctx *ctx, int32_t nprob, const float *E, int64_t e_len, const int64_t *e_off, const int32_t *n, const int32_t *d,
                     const int32_t *min_size, const int32_t *max_size, int32_t *cluster_id, int32_t *member_rank, int32_t *n_clusters,
                     int32_t *n_merges, int32_t *merges, int32_t *status);
int icl_cluster_many_dev(icl_ctx *ctx, int32_t nprob, const float *d_E, int64_t e_len, const int64_t *e_off, const int32_t *n, const int32_t *d,
                         const int32_t *min_size, const int32_t *max_size, int32_t *cluster_id, int32_t *member_rank, int32_t *n_clusters,
                         int32_t *n_merges, int32_t *merges, int32_t *status);
/* Problems of 257 to 2048 rows (above the small route's cap) can also run one workgroup each, in groups whose workspace stays under a
 * budget (the mid-size route of ward_many.hip; the same results, bit for bit).  ICL_MANY_MID_AUTO (default) takes that route when the
 * call holds enough such problems for it to beat the large-N engine (measured crossover counts), ICL_MANY_MID_OFF never, ICL_MANY_MID_ON
 * always, a lone problem included.  The environment variable ICL_MANY_MID=auto|off|on sets the default of new contexts;
 * ICL_MANY_MID_WS_MB overrides the group budget (read once per process).  Returns ICL_ERR_ARG for a null context or an unknown mode. */
#define ICL_MANY_MID_AUTO 0
#define ICL_MANY_MID_OFF 1
#define ICL_MANY_MID_ON 2
int icl_set_many_options(icl_ctx *ctx, int mid_mode);
/* problems of the last icl_cluster_many[_dev] call by route, and the number of mid-route groups it was run in (any pointer may be NULL) */
int icl_last_many_stats(icl_ctx *ctx, int64_t *small, int64_t *mid, int64_t *large, int64_t *mid_groups);
/* ---- seeded clustering: the loop of clustering.go:216-246 started from existing clusters (DESIGN.md "Seeded clustering") ----
 * The icl_cluster_many layout with SEEDS in place of images: problem p holds m[p] seed clusters, seed i given by its centroid (row i of
 * the problem's d[p]-float rows in E) and seed_size[seed_off(p) + i], seed_off(p) = m[0] + ... + m[p-1]: s > 0, a cluster of s items;
 * s < 0, a FROZEN cluster of -s items (every pair with it is banned from the start: it is never merged, but counts as a cluster and
 * its items count in N); s == 0 is ICL_ERR_ARG.  N = the items of all seeds.  k = k_target[p] when k_target is not NULL and the entry
 * is above 0, else CalculateOptimalClusters(N, min_size[p], max_size[p]) (ICL_ERR_CONSTRAINT as the problem's status on its errors);
 * max(0, m[p] - k) merges are asked for.  The loop is the reference's with the clusters' real sizes: the first strict minimum in
 * row-major order, the MaxFloat32 ban where the size sum exceeds max_size[p], fp32 values bit for bit.  Creation ids: seed i has id i,
 * the t-th merge id m[p] + t; merges holds (larger id, smaller id) per merge at offset 2*seed_off(p).  cluster_id / seed_rank
 * (seed_off layout): the final list is the surviving seeds in seed order, then the merged clusters in creation order; a cluster with
 * fewer than min_size[p] ITEMS is dropped (its seeds get -1 in both arrays), kept clusters get dense ids; seed_rank is the seed's place
 * in its cluster's seed sequence (Merge(a, b): a's seeds, then b's, a = the pair's first id).  C_out (may be NULL; the layout of E;
 * host memory, device memory for _dev): the row of each final cluster's rank-0 seed holds that cluster's centroid exactly as the loop
 * holds it, kept and dropped clusters alike (a never-merged seed's row is its input row), every other row is zero; the rows of a failed
 * problem are zero; floats of E between the problems' rows are zero in the host call's C_out and untouched in the _dev call's.
 * status[p]: ICL_OK, ICL_ERR_CONSTRAINT, or ICL_ERR_UNSUPPORTED for a seed above max_size[p] that is not frozen (the reference
 * would split it), more than 2048 seeds, or 2^30 items and more.  Problems of m <= 1 succeed with no merge.  Problems of up to 256 seeds
 * take the small route of ward_many.hip, a lone one included, larger ones the mid-size route whatever icl_set_many_options says.
 * With every seed_size 1 and no k_target the results are icl_cluster_many's, bit for bit.  The return code, "nothing is written on
 * ICL_ERR_ARG" and the icl_last_* guarantees are icl_cluster_many's; icl_last_many_stats reports the call. */
int icl_cluster_many_seeded(icl_ctx *ctx, int32_t nprob, const float *E, int64_t e_len, const int64_t *e_off, const int32_t *m, const int32_t *d,
                            const int32_t *seed_size, const int32_t *min_size, const int32_t *max_size, const int32_t *k_target,
                            int32_t *cluster_id, int32_t *seed_rank, int32_t *n_clusters, int32_t *n_merges, int32_t *merges, int32_t *status,
                            float *C_out);
int icl_cluster_many_seeded_dev(icl_ctx *ctx, int32_t nprob, const float *d_E, int64_t e_len, const int64_t *e_off, const int32_t *m,
                                const int32_t *d, const int32_t *seed_size, const int32_t *min_size, const int32_t *max_size,
                                const int32_t *k_target, int32_t *cluster_id, int32_t *seed_rank, int32_t *n_clusters, int32_t *n_merges,
                                int32_t *merges, int32_t *status, float *d_C_out);
/* ---- constrained seeded clustering: keep-apart pairs and anchored clusters (DESIGN.md "Constrained seeded clustering") ----
 * The seeded problem of icl_cluster_many_seeded, unchanged, plus a symmetric relation B, "apart", over the clusters.  Per problem:
 * apart_class[seed_off(p) + i] (NULL: all 0), one int per seed, 0 meaning none -- two different seeds of one non-zero class are apart; and
 * the pairs [pair_off[p], pair_off[p + 1]) of apart_pairs, two seed indices of the problem each, either order, duplicates allowed (pair_off
 * and apart_pairs both NULL: no pairs).  At the start B holds exactly these pairs; every pair in B holds MaxFloat32 in the matrix and is
 * never evaluated, beside the frozen and the size rule (a pair that names a frozen seed changes nothing).  When a and b merge into c,
 * B(c, x) = B(a, x) or B(b, x) for every other cluster x: a cluster that swallowed image A still refuses image B.  Where B(c, x) holds, x
 * is frozen or the size sum exceeds max_size[p], the new entry is MaxFloat32 and is not evaluated; elsewhere it is WardDistance(x, c) as
 * in the seeded call.  Everything else is the seeded call's: the first strict minimum in row-major order, the merge rule, creation ids,
 * the log, k, the final list, the drop rule, C_out, and the loop ending early for want of pairs, n_merges[p] then below m[p] - k.
 * Consequences: with apart_class all 0 (or NULL) and no pairs the results are icl_cluster_many_seeded's, bit for bit; and a run cut
 * after t merges and resumed -- the surviving clusters as seeds, each one's inherited bans as pairs, k_target as before -- is the same run.
 * The relation lives in the workspace as bit rows, m[p] x ceil(m[p] / 32) words per problem.  ICL_ERR_ARG, nothing written: a pair index
 * outside [0, m[p]), a pair (i, i), a negative class, a negative or decreasing pair offset, apart_pairs NULL where a problem has pairs or
 * given without pair_off.  status[p]: the seeded call's, ICL_ERR_UNSUPPORTED above 2048 seeds included.  The constraint arrays are host
 * memory in both forms.  The return code, "nothing is written on ICL_ERR_ARG" and icl_last_many_stats are icl_cluster_many_seeded's. */
int icl_cluster_many_apart(icl_ctx *ctx, int32_t nprob, const float *E, int64_t e_len, const int64_t *e_off, const int32_t *m, const int32_t *d,
                           const int32_t *seed_size, const int32_t *min_size, const int32_t *max_size, const int32_t *k_target,
                           const int32_t *apart_class, const int64_t *pair_off, const int32_t *apart_pairs, int32_t *cluster_id,
                           int32_t *seed_rank, int32_t *n_clusters, int32_t *n_merges, int32_t *merges, int32_t *status, float *C_out);
int icl_cluster_many_apart_dev(icl_ctx *ctx, int32_t nprob, const float *d_E, int64_t e_len, const int64_t *e_off, const int32_t *m,
                               const int32_t *d, const int32_t *seed_size, const int32_t *min_size, const int32_t *max_size,
                               const int32_t *k_target, const int32_t *apart_class, const int64_t *pair_off, const int32_t *apart_pairs,
                               int32_t *cluster_id, int32_t *seed_rank, int32_t *n_clusters, int32_t *n_merges, int32_t *merges, int32_t *status,
                               float *d_C_out);
/* ONE seeded problem on the large-N engine (ward.hip), with no cap on the number of seeds other than memory: the semantics above for a single
 * problem of m seeds -- C holds the m centroid rows of d floats, seed_size[m] as above, k = k_target when it is above 0 --, the same creation
 * ids, final list, drop rule and C_out (may be NULL; m x d floats, host memory, device memory for _dev).  The call runs the engine's EXACT
 * pipeline only -- every entry of the initial matrix by the exact tile with the seeds' sizes, exact rows for new clusters, batched or one merge
 * per step (ICL_WARD_BATCH=0) -- whatever icl_set_ward_options and m say: the matrix-core bounds and the Lance-Williams bound rows are proven for
 * singletons.  Returns ICL_OK; ICL_ERR_ARG (nothing written) for a null context or array, m < 0, d < 0 or a size of 0; ICL_ERR_CONSTRAINT for the
 * reference's (nil,false); ICL_ERR_UNSUPPORTED for a seed above max_size that is not frozen, 2^30 items or more, or a context that is a replica
 * of a group; ICL_ERR_NOMEM when the workspace (4 m^2 bytes, 8 m^2 where icl_cluster's own layout for m rows is the wider one) does not fit.  On
 * ICL_ERR_CONSTRAINT / _UNSUPPORTED cluster_id and seed_rank are -1, *n_clusters 0 and C_out zero.  A problem of m <= 1 runs no merge.  As after
 * icl_cluster, icl_last_merges (the log: (larger id, smaller id) per merge), icl_last_merge_values, icl_last_ward_mode and
 * icl_last_ward_stats report the call; icl_ward_dump_pairs_dev refuses the workspace a seeded call leaves (ICL_ERR_UNSUPPORTED).  With the
 * same problem the results equal icl_cluster_many_seeded's, and with every size 1 and no k_target icl_cluster's, bit for bit. */
int icl_cluster_seeded(icl_ctx *ctx, const float *C, int64_t m, int32_t d, const int32_t *seed_size, int32_t min_size, int32_t max_size,
                       int32_t k_target, int32_t *cluster_id, int32_t *seed_rank, int32_t *n_clusters, float *C_out);
int icl_cluster_seeded_dev(icl_ctx *ctx, const float *d_C, int64_t m, int32_t d, const int32_t *seed_size, int32_t min_size, int32_t max_size,
                           int32_t k_target, int32_t *cluster_id, int32_t *seed_rank, int32_t *n_clusters, float *d_C_out);
/* The seeded problem above in FAST mode (ICL_UPDATE_LW; DESIGN.md "Seeded clustering in FAST mode"): the same arguments, admission (N, k,
 * frozen seeds, an unfrozen seed above max_size), creation ids, final list, drop rule and seed_rank, on the Lance-Williams loop of
 * icl_cluster(update = ICL_UPDATE_LW).  The initial matrix comes from the matrix cores: entry (i, j), i > j, is
 * clamp0(fl(fl(f32(|s_i| |s_j|) / f32(|s_i| + |s_j|)) * fl(2 D~(i, j)))) with D~ icl_distance_mfma_dev's matrix of the m centroid rows
 * (icl_distance_mfma_seeded_dev is that matrix alone); selection, new rows, clamp and the NaN rule are FAST mode's, on the effective sizes (a
 * frozen seed counts max_size).  The engine keeps no centroids in this mode: C_out (may be NULL) is MergeClusters' centroid evaluated along
 * the call's own log with the real item counts -- what the exact call would hold had it made the same merges -- at the row of each final
 * cluster's rank-0 seed; a never-merged seed keeps its input row, every other row is zero.  NOT an identity: a FAST run cut after t merges
 * and resumed from its clusters rebuilds the matrix from centroids, where the uncut run carried Lance-Williams values forward; only the
 * exact calls have the restart identity.  With every size 1 and no k_target the results equal icl_cluster(update = ICL_UPDATE_LW)'s, bit
 * for bit.  Statuses, "nothing written on ICL_ERR_ARG", the rows of -1 and the zero C_out of a refused problem are icl_cluster_seeded's;
 * ICL_ERR_UNSUPPORTED also on a replica of a group.  icl_last_merges, icl_last_merge_values and icl_last_ward_stats report the call,
 * icl_last_ward_mode gives ICL_ROWS_LW_FAST (ICL_ROWS_SINGLE under ICL_WARD_BATCH=0), icl_ward_dump_pairs_dev refuses the workspace
 * afterwards.  Not covered: keep-apart constraints, the ward_many routes and icl_cluster_requests, distance bounds, group contexts. */
int icl_cluster_seeded_fast(icl_ctx *ctx, const float *C, int64_t m, int32_t d, const int32_t *seed_size, int32_t min_size, int32_t max_size,
                            int32_t k_target, int32_t *cluster_id, int32_t *seed_rank, int32_t *n_clusters, float *C_out);
int icl_cluster_seeded_fast_dev(icl_ctx *ctx, const float *d_C, int64_t m, int32_t d, const int32_t *seed_size, int32_t min_size,
                                int32_t max_size, int32_t k_target, int32_t *cluster_id, int32_t *seed_rank, int32_t *n_clusters,
                                float *d_C_out);
/* ONE constrained seeded problem on the large-N engine (DESIGN.md "Constrained seeded clustering, large N"): icl_cluster_many_apart's semantics
 * for a single problem of m seeds with no cap on m other than memory.  The relation B starts from apart_class[m] (NULL: all 0; two different
 * seeds of one non-zero class are apart) and the n_pairs pairs of apart_pairs (two seed indices each, either order, duplicates allowed; NULL
 * with n_pairs 0), both host memory in both forms; a pair in B holds MaxFloat32 and is never picked; when a and b merge into c,
 * B(c, x) = B(a, x) or B(b, x).  Everything else is icl_cluster_seeded's: selection order, values, ids, the log, k, the final list, the drop
 * rule, C_out, and the loop ending early for want of pairs.  With no constraint the results equal icl_cluster_seeded's, and for m <= 2048
 * icl_cluster_many_apart's, bit for bit.  The relation lives in the engine's workspace as m x ceil(m / 32) words over the matrix's column slots
 * (1.25 GB at m = 100 000), built on the device from the two arrays.  The call runs the ONE-MERGE-PER-STEP exact loop only, whatever
 * ICL_WARD_BATCH says.  Not covered: the batched loops, the distance bounds and FAST mode, group and replica contexts (ICL_ERR_UNSUPPORTED),
 * icl_cluster_requests; the exact fill evaluates banned pairs too before they are masked.
 * ICL_ERR_ARG, nothing written: icl_cluster_seeded's cases, a negative n_pairs, apart_pairs NULL with n_pairs above 0, a negative class, a
 * pair index outside [0, m) or a pair (i, i).  Every other status is icl_cluster_seeded's; ICL_ERR_NOMEM also where the bit rows do not fit.
 * The icl_last_* reports behave as after icl_cluster_seeded, icl_last_ward_mode gives ICL_ROWS_SINGLE_APART, and icl_ward_dump_pairs_dev
 * refuses the workspace afterwards (ICL_ERR_UNSUPPORTED). */
int icl_cluster_apart(icl_ctx *ctx, const float *C, int64_t m, int32_t d, const int32_t *seed_size, int32_t min_size, int32_t max_size,
                      int32_t k_target, const int32_t *apart_class, int64_t n_pairs, const int32_t *apart_pairs, int32_t *cluster_id,
                      int32_t *seed_rank, int32_t *n_clusters, float *C_out);
int icl_cluster_apart_dev(icl_ctx *ctx, const float *d_C, int64_t m, int32_t d, const int32_t *seed_size, int32_t min_size, int32_t max_size,
                          int32_t k_target, const int32_t *apart_class, int64_t n_pairs, const int32_t *apart_pairs, int32_t *cluster_id,
                          int32_t *seed_rank, int32_t *n_clusters, float *d_C_out);
/* The id rule above for one problem, on the host (no GPU, no context): m seeds, their sizes (the sign is ignored), min_size and a merge
 * log of n_merges pairs -> cluster_id[m], seed_rank[m], n_clusters.  ICL_ERR_ARG for a size of 0 or a log that names a cluster that does
 * not exist (any more); nothing is written then. */
int icl_seeded_assign_ids(int32_t m, const int32_t *seed_size, int32_t min_size, const int32_t *merges, int32_t n_merges, int32_t *cluster_id,
                          int32_t *seed_rank, int32_t *n_clusters);
/* ---- nearest clusters: each query's k library clusters of smallest WardDistance, exact, with no distance matrix (DESIGN.md "Nearest clusters") ----
 * Q holds nq query centroids and E n library centroids, rows of d floats; q_size[nq] / e_size[n] are the clusters' item counts (NULL: all 1).
 * VALUE of pair (i, j): WardDistance (clustering.go:136-157) of a cluster of q_size[i] items at Q[i] and one of e_size[j] items at E[j], bit for
 * bit -- differences, products and the sum each rounded, strictly in k order, then (float(sa*sb) / float(sa+sb)) * s.  With both size arrays
 * NULL the values are the entries of ComputeInitialDistanceMatrix (:61-73) over the stacked rows.
 * PAIRS LEFT OUT: j == exclude[i] (exclude may be NULL; -1: none; a self-join -- Q is E -- passes exclude[i] = i), and, when max_size > 0, every
 * pair with q_size[i] + e_size[j] > max_size: the reference's ban (:228).
 * ORDER: row i of idx / val (nq x k each) holds the k smallest remaining pairs, ascending by (value, j): values compare as fp32 with `<`, NaN
 * values sort behind every number, ties (equal numbers, two NaNs) go by j.  The result does not depend on tile order, split count or launch
 * geometry.  SHORT ROWS: if fewer than k pairs remain the tail is idx = -1, val = MaxFloat32 (the reference's ban value).
 * Returns ICL_ERR_ARG, with nothing written, for a null pointer that is needed (the context; Q, idx, val when nq > 0; E when n > 0), k outside
 * 1..64, d < 1, negative nq or n, n >= 2^31, a size <= 0, or an exclude entry outside [-1, n); nq == 0 or n == 0 is ICL_OK, and with n == 0 every
 * entry is the tail; ICL_ERR_UNSUPPORTED on a context that is a replica of a group; ICL_ERR_NOMEM when the workspace does not fit.
 * icl_nearest takes host memory throughout: it uploads, calls the _dev form and downloads.  icl_nearest_dev takes Q, E, idx and val on the
 * context's device (consumed and written on the context's stream; Q and E 16-byte aligned take the wide loads when d % 4 == 0); q_size, e_size
 * and exclude stay in host memory and may be reused at return.  No nq x n array exists anywhere: the workspace is the device copies of the
 * three host arrays plus 8 * nq * k * splits bytes of partial lists when the library's columns are split (splits > 1). */
int icl_nearest(icl_ctx *ctx, const float *Q, const int32_t *q_size, int64_t nq, const float *E, const int32_t *e_size, int64_t n, int32_t d,
                int32_t k, int32_t max_size, const int64_t *exclude, int32_t *idx, float *val);
int icl_nearest_dev(icl_ctx *ctx, const float *d_Q, const int32_t *q_size, int64_t nq, const float *d_E, const int32_t *e_size, int64_t n,
                    int32_t d, int32_t k, int32_t max_size, const int64_t *exclude, int32_t *d_idx, float *d_val);
/* The same leave-out and order rules applied to values the caller already holds (host only: no context, no GPU), e.g. the result of
 * icl_ward_distance_matrix: D[i * ld + j] is pair (i, j)'s value, used as given; the sizes serve the max_size rule alone.  The comparison and
 * the insertion are the code the device runs (nearest_select.h).  ICL_ERR_ARG, with nothing written, as above and for ld < n. */
int icl_nearest_from_matrix(const float *D, int64_t nq, int64_t n, int64_t ld, const int32_t *q_size, const int32_t *e_size, int32_t k,
                            int32_t max_size, const int64_t *exclude, int32_t *idx, float *val);
/* A workgroup owns a band of 128 query rows; with few bands and a large library the library's 128-column tiles are split over column_splits
 * workgroups per band and a second kernel merges their partial lists.  0 (default): the engine decides from nq, n and the CU count; a count
 * above 0 is used as given, up to one tile per split and 1024 splits.  Same results for every count.  ICL_ERR_ARG for a null context or a negative count. */
int icl_set_nearest_options(icl_ctx *ctx, int32_t column_splits);
/* The last icl_nearest[_dev] of the context: info = splits used, tiles run, pairs evaluated, workspace bytes (all 0 after a call with nq == 0). */
int icl_last_nearest_stats(icl_ctx *ctx, int64_t info[4]);
/* ---- cluster fit: each clustered row's exact cost against its own cluster and its nearest alternatives, no distance matrix (DESIGN.md "Cluster fit") ----
 * Q holds nq rows of d floats (images, or seeds at seed granularity) with item counts q_size[nq] (NULL: all 1); C holds K centroid rows with
 * item counts c_size[K] in the seeded calls' sign convention: s > 0 a cluster of s items, s < 0 a FROZEN cluster of -s items, NULL: all 1.
 * cluster_of[nq] names each row's own cluster in C, -1: the row belongs to none.
 * VALUE of pair (i, j): WardDistance (clustering.go:136-157) of q_size[i] items at Q[i] and |c_size[j]| items at C[j], bit for bit, icl_nearest's
 * arithmetic.  The own cost and the alternatives are the same quantity: "closer to another cluster than to its own" is an exact statement.
 * PER ROW: own[i] is the value of pair (i, cluster_of[i]) -- a frozen own cluster included, never subject to the max_size ban --, MaxFloat32 for
 * cluster_of[i] == -1.  Row i of alt_idx / alt_val (nq x k_alt each) is icl_nearest's result over C with three kinds of pair left out: column
 * cluster_of[i]; every frozen column; and, when max_size > 0, pairs with q_size[i] + c_size[j] > max_size.  Order, NaN placement, ties by j and
 * the tails of short rows (-1, MaxFloat32) are icl_nearest's.  k_alt is 0 .. 64; with k_alt == 0 both pointers may be NULL.
 * PER CLUSTER (each pointer may be NULL): listed[j] = the number of rows that name cluster j; rep[j] = the row of smallest own cost among them
 * (values compare with `<`, numbers come before NaN, ties go to the lowest row); worst[j] = the row of largest own cost (NaN counts above every
 * number, ties go to the lowest row); both -1 when no row names the cluster.
 * The results do not depend on tile order, split count or launch geometry; icl_set_nearest_options' column_splits applies as it does to icl_nearest.
 * Returns ICL_ERR_ARG, with nothing written, for a null pointer that is needed (the context; Q, cluster_of, own when nq > 0; alt_idx, alt_val when
 * nq > 0 and k_alt > 0; C when K > 0), k_alt outside 0..64, d < 1, negative nq or K, nq or K >= 2^31, a q_size <= 0, a c_size of 0, or a cluster_of
 * entry outside [-1, K) (so K == 0 takes rows of -1 only); nq == 0 is ICL_OK and leaves listed 0 and rep / worst -1; ICL_ERR_UNSUPPORTED on a
 * context that is a replica of a group; ICL_ERR_NOMEM when the workspace does not fit.
 * icl_cluster_fit takes host memory throughout: it uploads, runs the _dev body and downloads.  icl_cluster_fit_dev takes Q, C, own, alt_idx,
 * alt_val, listed, rep and worst on the context's device (consumed and written on the context's stream; Q and C 16-byte aligned take the wide
 * loads when d % 4 == 0); q_size, cluster_of and c_size stay in host memory and may be reused at return.  With k_alt == 0 no tile is run: the
 * own costs come from icl_ward_values_at's kernel on the pairs (i, cluster_of[i]).  The workspace is the device copies of the three host
 * arrays, 8 * nq * k_alt * splits bytes of partial lists when the columns are split, and 16 * K bytes of keys when rep or worst is asked for. */
int icl_cluster_fit(icl_ctx *ctx, const float *Q, const int32_t *q_size, const int32_t *cluster_of, int64_t nq, const float *C,
                    const int32_t *c_size, int64_t K, int32_t d, int32_t k_alt, int32_t max_size, float *own, int32_t *alt_idx, float *alt_val,
                    int32_t *listed, int32_t *rep, int32_t *worst);
int icl_cluster_fit_dev(icl_ctx *ctx, const float *d_Q, const int32_t *q_size, const int32_t *cluster_of, int64_t nq, const float *d_C,
                        const int32_t *c_size, int64_t K, int32_t d, int32_t k_alt, int32_t max_size, float *d_own, int32_t *d_alt_idx,
                        float *d_alt_val, int32_t *d_listed, int32_t *d_rep, int32_t *d_worst);
/* The same rules applied to values the caller already holds (host only: no context, no GPU): D[i * ld + j] is pair (i, j)'s value, used as
 * given -- own[i] = D[i * ld + cluster_of[i]] --; the sizes serve the frozen and max_size rules alone.  The leave-out rule and the key order
 * are the code the device runs (fit_select.h).  ICL_ERR_ARG, with nothing written, as above (D is needed when nq > 0 and K > 0) and for ld < K. */
int icl_cluster_fit_from_matrix(const float *D, int64_t nq, int64_t K, int64_t ld, const int32_t *q_size, const int32_t *cluster_of,
                                const int32_t *c_size, int32_t k_alt, int32_t max_size, float *own, int32_t *alt_idx, float *alt_val,
                                int32_t *listed, int32_t *rep, int32_t *worst);
/* The last icl_cluster_fit[_dev] of the context: info = column splits used, tiles run (both 0 with k_alt == 0), pairs evaluated, workspace
 * bytes (all 0 after a call with nq == 0 and K == 0). */
int icl_last_fit_stats(icl_ctx *ctx, int64_t info[4]);
/* Exact values of listed pairs: val[p] = WardDistance of q_size[qi[p]] items at row qi[p] of Q (nq x d) and |e_size[ej[p]]| items at row ej[p]
 * of E (n x d), bit for bit, for p < np (size arrays NULL: all 1; a negative e_size is a frozen cluster's item count).  Pairs may repeat.  One
 * lane per pair adds the pair's d rounded products in k order; no tile is run, so np pairs cost np * d operations wherever they lie.
 * Returns ICL_ERR_ARG, with nothing written, for a null pointer that is needed (the context; Q, E, qi, ej, val when np > 0), d < 1, a negative
 * count, nq or n >= 2^31, a q_size <= 0, an e_size of 0 or a pair outside [0, nq) x [0, n); np == 0 is ICL_OK; ICL_ERR_UNSUPPORTED on a replica
 * of a group; ICL_ERR_NOMEM when the device copies do not fit.  icl_ward_values_at_dev takes Q, E and val on the context's device (written on
 * the context's stream); the sizes and the pair list stay in host memory and may be reused at return. */
int icl_ward_values_at(icl_ctx *ctx, const float *Q, const int32_t *q_size, int64_t nq, const float *E, const int32_t *e_size, int64_t n, int32_t d,
                       const int32_t *qi, const int32_t *ej, int64_t np, float *val);
int icl_ward_values_at_dev(icl_ctx *ctx, const float *d_Q, const int32_t *q_size, int64_t nq, const float *d_E, const int32_t *e_size, int64_t n,
                           int32_t d, const int32_t *qi, const int32_t *ej, int64_t np, float *d_val);
/* ---- fold centroids: the centroid of every cluster given as a member list (DESIGN.md "Editing a held clustering") ----
 * E holds n rows of d floats with item counts size[n] (NULL: all 1).  Group g, g < K, is the rows member[row_ptr[g] .. row_ptr[g + 1]) of E, in
 * that order; a row may appear in several groups, several times in one group, or in none.
 * VALUE: what the reference holds after merging the members one at a time in member order (MergeClusters, clustering.go:29-47).  The first
 * member's row is copied; member t then gives, per column k,
 *     c[k] = (float(S) * c[k] + float(s_t) * E[m_t][k]) / float(S + s_t),    S += s_t
 * with S the integer item total so far and each product, the sum and the quotient rounded to fp32 on its own (no contraction).  The fold is
 * not associative: the order is the list's.  Row g of C_out (K x d, no pitch) receives group g's centroid, size_out[g] (may be NULL) its item
 * total; an empty group gives a row of +0.0 and size 0.  The result does not depend on launch geometry.
 * Returns ICL_ERR_ARG, with nothing written, for a null pointer that is needed (the context; row_ptr and C_out when K > 0; member and E when a
 * group has a member), n < 0, d < 1, K < 0 or K >= 2^31, row_ptr[0] != 0, a decreasing row_ptr, a member outside [0, n), a size below 1, or a
 * group whose item total exceeds INT32_MAX; K == 0 is ICL_OK with no launch; ICL_ERR_UNSUPPORTED on a context that is a replica of a group;
 * ICL_ERR_NOMEM when the device copies do not fit.
 * icl_fold_centroids takes host memory throughout: it uploads E, runs the _dev body and downloads C_out.  icl_fold_centroids_dev takes E and
 * C_out on the context's device (read and written on the context's stream; both 16-byte aligned take 16-byte loads and stores when
 * d % 4 == 0); size, row_ptr, member and size_out stay in host memory and may be reused at return. */
int icl_fold_centroids(icl_ctx *ctx, const float *E, const int32_t *size, int64_t n, int32_t d, const int64_t *row_ptr, const int32_t *member,
                       int64_t K, float *C_out, int32_t *size_out);
int icl_fold_centroids_dev(icl_ctx *ctx, const float *d_E, const int32_t *size, int64_t n, int32_t d, const int64_t *row_ptr,
                           const int32_t *member, int64_t K, float *d_C_out, int32_t *size_out);
/* The last icl_fold_centroids[_dev] of the context: info = groups, member rows read, the longest group's length, workspace bytes (all 0 after
 * a call with K == 0). */
int icl_last_fold_stats(icl_ctx *ctx, int64_t info[4]);
/* ---- duplicate pairs: every pair of rows whose WardDistance is at most a threshold, exact and complete, no distance matrix (DESIGN.md "Duplicate pairs") ----
 * E holds n rows of d floats; size[n] are the rows' item counts (NULL: all 1).
 * VALUE of pair (i, j), j < i < n: WardDistance (clustering.go:136-157) of a cluster of size[i] items at E[i] and one of size[j] items at E[j],
 * bit for bit -- differences, products and the sum each rounded, strictly in k order, then (float(sa*sb) / float(sa+sb)) * s.  With size NULL
 * the values are the entries of ComputeInitialDistanceMatrix (:61-73).
 * PAIR SET: every pair with value <= threshold as an fp32 comparison, however many partners a row has.  A NaN value is never listed; a
 * threshold of -0.0f admits zero values; +Inf admits everything that is not NaN.  A NaN threshold is ICL_ERR_ARG.
 * ORDER AND LAYOUT (CSR over the strict lower triangle): col[row_ptr[i] .. row_ptr[i + 1]) are row i's partners j < i in ascending j and val
 * holds their values at the same places; row_ptr[0] = 0 and *total = row_ptr[n].  Each pair appears once.  The result does not depend on
 * tile order, launch geometry or the order in which workgroups finish.
 * CAPACITY: col and val hold cap entries each.  row_ptr (n + 1 entries) and *total are always complete and exact.  If *total > cap the call
 * returns ICL_ERR_ARG with those two filled and col / val unspecified (icl_jpeg_encode_rgb_dev's convention: ask again with a buffer of
 * *total entries; a caller tells this case from a bad argument by *total, which a bad argument leaves untouched).  col == NULL && val == NULL
 * && cap == 0 is the size query and returns ICL_OK.
 * Returns ICL_ERR_ARG, with nothing written, for a null pointer that is needed (the context, row_ptr, total; E when n > 1; one of col / val
 * without the other, or both NULL with cap > 0), d < 1, n < 0, n >= 2^31, a size <= 0, cap < 0, a NaN threshold, or an n whose triangle of
 * 128 x 128 tiles does not fit one launch (2^31 tiles); n <= 1 is ICL_OK with *total = 0; ICL_ERR_UNSUPPORTED on a context that is a
 * replica of a group; ICL_ERR_NOMEM when the workspace, or in the host form the device copies of E, col and val, do not fit.
 * icl_pairs_within takes host memory throughout: it uploads, runs the _dev body and downloads.  icl_pairs_within_dev takes E, col and val on
 * the context's device (col and val are written on the context's stream; E 16-byte aligned with d % 4 == 0 takes the wide loads, anything
 * else the scalar loads, with equal results); size and row_ptr stay in host memory, and row_ptr and *total are final at return.
 * COST: no n x n array exists anywhere.  A count pass evaluates every tile of the triangle once; a fill pass evaluates the tiles that hold
 * a listed pair a second time.  With rare duplicates that is a negligible share; with threshold = +Inf it is the whole triangle twice.
 * The fill pass gives each row of tiles to one workgroup, which walks that row's tiles one after the other: a dense result at large n takes
 * longer than two count passes (the longest row of tiles sets the time; not measured).
 * The workspace is 4 n bytes of sizes, 4 n of counts, 8 (n + 1) of row_ptr, one byte per tile and 4 bytes per tile row. */
int icl_pairs_within(icl_ctx *ctx, const float *E, const int32_t *size, int64_t n, int32_t d, float threshold, int64_t *row_ptr, int32_t *col,
                     float *val, int64_t cap, int64_t *total);
int icl_pairs_within_dev(icl_ctx *ctx, const float *d_E, const int32_t *size, int64_t n, int32_t d, float threshold, int64_t *row_ptr,
                         int32_t *d_col, float *d_val, int64_t cap, int64_t *total);
/* The same pair rule, layout and capacity convention applied to values the caller already holds (host only: no context, no GPU), e.g. the
 * result of icl_ward_distance_matrix: D[i * ld + j], j < i, is pair (i, j)'s value, used as given; nothing else of D is read.  The
 * comparison is the code the device runs (pairs_select.h).  ICL_ERR_ARG, with nothing written, as above (D is needed when n > 1) and for ld < n. */
int icl_pairs_within_from_matrix(const float *D, int64_t n, int64_t ld, float threshold, int64_t *row_ptr, int32_t *col, float *val, int64_t cap,
                                 int64_t *total);
/* The connected components of the pair graph a CSR list describes (host only): group[i] is the smallest index of i's component -- an image
 * with no partner is its own group --, *n_groups the number of components with at least two members.  ICL_ERR_ARG, with nothing written, for
 * a null pointer that is needed, n < 0, n >= 2^31, row_ptr[0] != 0, a row_ptr that decreases or a col entry of row i outside [0, i). */
int icl_pair_groups(int64_t n, const int64_t *row_ptr, const int32_t *col, int32_t *group, int64_t *n_groups);
/* The last icl_pairs_within[_dev] of the context: info = tiles run in the count pass, tiles with a hit, pairs j < i < n evaluated (both
 * passes; the fill pass counts when it ran), workspace bytes (all 0 after a call with n <= 1). */
int icl_last_pairs_stats(icl_ctx *ctx, int64_t info[4]);
/* ---- duplicates against a library: every pair (query row, library row) whose WardDistance is at most a threshold, exact and complete, no
 * distance matrix, no cap on a query's partners (DESIGN.md "Duplicates against a library") ----
 * Q holds nq query rows and L n library rows of d floats; q_size[nq] / l_size[n] are the rows' item counts (NULL: all 1).
 * VALUE of pair (i, j): WardDistance (clustering.go:136-157) of q_size[i] items at Q[i] and l_size[j] items at L[j], icl_nearest's value bit for
 * bit: the exact tile's sum, then (float(sa*sb) / float(sa+sb)) * s.
 * PAIR SET: every pair with j != exclude[i] and value <= threshold as an fp32 comparison, whatever the sizes (there is no max_size ban: a
 * duplicate is a duplicate).  exclude may be NULL, -1 means none; queries that are themselves library rows pass their own row.  A NaN value
 * is never listed; a threshold of -0.0f admits zero values; +Inf admits everything that is not NaN.  A NaN threshold is ICL_ERR_ARG.
 * ORDER AND LAYOUT (CSR over the queries): col[row_ptr[i] .. row_ptr[i + 1]) are query i's library partners in ascending j and val holds their
 * values at the same places; row_ptr has nq + 1 entries, row_ptr[0] = 0 and *total = row_ptr[nq].  The result does not depend on split
 * count, tile order or the order in which workgroups finish.
 * CAPACITY: as icl_pairs_within.  col and val hold cap entries each; row_ptr and *total are always complete and exact; *total > cap returns
 * ICL_ERR_ARG with those two filled and col / val unspecified (a bad argument leaves *total untouched); col == NULL && val == NULL && cap == 0
 * is the size query and returns ICL_OK.
 * Returns ICL_ERR_ARG, with nothing written, for a null pointer that is needed (the context, row_ptr, total; Q and L when nq > 0 and n > 0; one
 * of col / val without the other, or both NULL with cap > 0), d < 1, negative nq or n, n >= 2^31, a size <= 0, an exclude entry outside
 * [-1, n), a NaN threshold, cap < 0, or a grid (bands of 128 queries x column splits) that does not fit one launch; nq == 0 or n == 0 is ICL_OK
 * with *total = 0; ICL_ERR_UNSUPPORTED on a context that is a replica of a group; ICL_ERR_NOMEM when the workspace, or in the host form the
 * device copies of Q, L, col and val, do not fit.
 * icl_pairs_between takes host memory throughout: it uploads, runs the _dev body and downloads.  icl_pairs_between_dev takes Q, L, col and val
 * on the context's device (col and val are written on the context's stream; Q and L 16-byte aligned with d % 4 == 0 take the wide loads,
 * anything else the scalar loads, with equal results); q_size, l_size, exclude and row_ptr stay in host memory, and row_ptr and *total are
 * final at return.
 * GEOMETRY AND COST: icl_nearest's band walk for both passes.  A workgroup owns a band of 128 queries and a contiguous range of the library's
 * 128-column tiles; few bands against a large library are split over several workgroups per band (icl_set_nearest_options' column_splits
 * applies here too; same results for every count).  A count pass evaluates every tile once and stores one count per (query, split) and one
 * flag per tile, each with a single writer (no atomics on global memory); the host takes the prefix; a fill pass, launched for the (band,
 * split) pairs that counted a hit, evaluates the flagged tiles a second time and places each hit by arithmetic alone.  With rare duplicates
 * the second pass is a negligible share; with threshold = +Inf it is the whole rectangle twice.
 * The workspace is the device copies of the three host arrays, 4 nq splits bytes of counts, 8 (nq splits + 1) of segment starts, one byte
 * per tile and 4 bytes per workgroup. */
int icl_pairs_between(icl_ctx *ctx, const float *Q, const int32_t *q_size, int64_t nq, const float *L, const int32_t *l_size, int64_t n, int32_t d,
                      float threshold, const int64_t *exclude, int64_t *row_ptr, int32_t *col, float *val, int64_t cap, int64_t *total);
int icl_pairs_between_dev(icl_ctx *ctx, const float *d_Q, const int32_t *q_size, int64_t nq, const float *d_L, const int32_t *l_size, int64_t n,
                          int32_t d, float threshold, const int64_t *exclude, int64_t *row_ptr, int32_t *d_col, float *d_val, int64_t cap,
                          int64_t *total);
/* The same pair rule, layout and capacity convention applied to values the caller already holds (host only: no context, no GPU), e.g. a block
 * of icl_ward_distance_matrix: D[i * ld + j] is pair (i, j)'s value, used as given.  The comparison is the code the device runs
 * (pairs_select.h).  ICL_ERR_ARG, with nothing written, as above (D is needed when nq > 0 and n > 0) and for ld < n. */
int icl_pairs_between_from_matrix(const float *D, int64_t nq, int64_t n, int64_t ld, float threshold, const int64_t *exclude, int64_t *row_ptr,
                                  int32_t *col, float *val, int64_t cap, int64_t *total);
/* The last icl_pairs_between[_dev] of the context: info = column splits used, tiles run in the count pass, tiles with a hit, pairs evaluated
 * (both passes; the fill pass counts when it ran), workspace bytes (all 0 after a call with nq == 0 or n == 0). */
int icl_last_pairs_between_stats(icl_ctx *ctx, int64_t info[5]);
/* ---- a queue of requests, files to cluster ids: replaces workflow.Run (workflow.go:84-94) for nreq requests in ONE call ----
 * Request r is n[r] image files with labels.  Every image gets its embedding row (GetImageEmbedding; head, prec as icl_embed_files), a one-hot
 * vector over the request's label set is appended (GenerateLabelVector + CombineEmbeddings, embeddings.go:166-183: d[r] = head + n_labels[r]
 * columns) and the combined rows are clustered (PerformClusteringWithConstraints, exact mode).  The combined rows are assembled on the GPU
 * (requests.hip) and stay there between the two halves.
 * icl_requests_layout (host only, no GPU): where request r's rows live in E and how wide they are: d[r] = head + n_labels[r],
 * e_off[r] = sum over q < r of n[q] * d[q] (rows contiguous, requests back to back), *e_len = the total number of floats.  Any output may be NULL.
 * ICL_ERR_ARG (nothing written) for nreq < 0, head < 0, a null input, a negative n / n_labels or a row length beyond int32.
 * icl_cluster_requests: paths lists all images, request after request (sum of n[r] entries).  Image i's labels are
 * label_idx[label_off[i] .. label_off[i + 1]): columns within its request's label set; -1 = "label not in the set" (embeddings.go:169) is
 * ignored, a column listed twice is set once.  Outputs use the icl_cluster_many layout: request r's images occupy [img_off(r), img_off(r) +
 * n[r]) of cluster_id / member_rank, img_off(r) = n[0] + ... + n[r-1], and its merge log (merges may be NULL) starts at 2 * img_off(r) with
 * n_merges[r] pairs.  For every request whose files were all read the results -- ids, ranks, n_clusters[r], merge log, and its rows of E_out --
 * are bit for bit those of icl_embed_files(head, prec) on its paths, CombineEmbeddings on the host, then icl_cluster_many on those rows.
 * status[r] = ICL_OK, ICL_ERR_CONSTRAINT for the reference's (nil,false), or -- a request with a file that cannot be read fails as a whole
 * (workflow.go:162-181) -- the code of its lowest failed file; a failed request's rows are -1 and its n_clusters[r] and n_merges[r] are 0.
 * Requests with a failed file are left out of the clustering launches; the others are unaffected.  file_status (may be NULL): every image's
 * code, as icl_embed_files gives it.  E_out (host, e_len floats of icl_requests_layout, may be NULL): the combined rows of every request,
 * with NaN in the embedding part of failed files.
 * Returns ICL_OK when every request succeeded; otherwise the code of the LOWEST failed request, which icl_last_error names together with
 * the file where there is one.  ICL_ERR_ARG (nothing written): a null pointer, nreq < 0, a negative n / n_labels, label_off decreasing or
 * starting below 0, a label index outside [-1, n_labels[r]), an unknown head / prec, threads < 0.  ICL_ERR_NOMODEL before anything runs.
 * Every ICL_* code is >= 0, and status is written only together with the per-request results: when the call returns a code that is not a
 * request's own failure (ICL_ERR_ARG, ICL_ERR_NOMODEL, a device or memory error that stopped it) status and every other output's per-request
 * meaning are void and status itself is left untouched -- a caller that pre-fills status with -1 finds the -1 still there.
 * The context's mutex is held once for the whole call; icl_set_ingest_options, icl_set_many_options, icl_set_batch and icl_set_conv_options
 * apply as they do to icl_embed_files and icl_cluster_many; icl_last_ingest_stats, icl_last_entropy_stats and icl_last_many_stats report this
 * call afterwards; what icl_last_merges and icl_last_ward_* report about the last icl_cluster stays unchanged.
 * icl_last_requests_ms: wall times (ms, HIP events on the context stream) of the last icl_cluster_requests: files -> embedding rows,
 * assembly of the combined rows, clustering (any pointer may be NULL). */
int icl_requests_layout(int32_t nreq, const int32_t *n, const int32_t *n_labels, int head, int64_t *e_off /* nreq */, int32_t *d /* nreq */,
                        int64_t *e_len);
int icl_cluster_requests(icl_ctx *ctx, int32_t nreq, const char *const *paths, const int32_t *n, const int32_t *n_labels,
                         const int64_t *label_off /* sum n[r] + 1 */, const int32_t *label_idx, const int32_t *min_size, const int32_t *max_size,
                         int head, int prec, int32_t threads, int32_t *cluster_id, int32_t *member_rank, int32_t *n_clusters, int32_t *n_merges,
                         int32_t *merges, int32_t *status /* nreq */, int32_t *file_status /* sum n[r] */, float *E_out);
int icl_last_requests_ms(icl_ctx *ctx, double *embed_ms, double *assemble_ms, double *cluster_ms);
/* ---- images from memory: the twins of the path calls above for callers that hold the encoded bytes (workflow.go:66: workflow.Run receives
 * models.UploadedImage{Filename, Data}; the reference writes them to a temporary directory, :120-127, only because gocv.IMRead wants a name) ----
 * An image is data[0 .. bytes): the bytes of a JPEG / PNG / PPM file, decoded in place by the decoders the path calls use; nothing is copied
 * or written to disk.  THE BUFFERS STAY OWNED BY THE CALLER AND MUST REMAIN VALID AND UNCHANGED UNTIL THE CALL RETURNS (the batched calls may
 * read an image twice: an image the GPU entropy check rejects is decoded again from the same buffer).  Nothing past data[bytes - 1] is read.
 * Outputs, layout, row ownership (row i belongs to image i), status codes, NaN / zero rows of failed images and the statistics calls are
 * those of the path twin; for the same bytes the results are equal bit for bit.  An error message names a memory image as
 * "image <index> (in memory, <bytes> bytes)" where the path call names the path (index 0 for the single-image calls).  data == NULL or
 * bytes <= 0 is that IMAGE's failure (ICL_ERR_IO, "empty image buffer"), as a missing file is for a path call.  ICL_ERR_ARG (nothing written)
 * is for the call's own arguments: a null data or bytes ARRAY with n > 0, n < 0, and whatever the path twin rejects.
 * icl_decode_image_mem / icl_load_image_224_mem / icl_preprocess_mem: icl_decode_image_file / icl_load_image_224 / icl_preprocess_file (host only).
 * icl_embed_image_mem: icl_embed_file; it joins the SAME coalescing queue (a batch may mix path and memory callers; icl_set_file_options,
 * icl_file_batch_stats and ICL_FILE_FAIL_NEXT_LEADER apply alike).
 * icl_load_images_224_mem_dev / icl_embed_images_mem / icl_embed_images_mem_dev: icl_load_images_224_dev / icl_embed_files / icl_embed_files_dev;
 * icl_last_ingest_stats and icl_last_entropy_stats report the call afterwards.
 * icl_cluster_requests_mem: icl_cluster_requests with data / bytes (sum of n[r] entries, request after request) in place of paths.
 * icl_jpeg_coefs_mem: icl_jpeg_coefs_files (test hook). */
int icl_decode_image_mem(const uint8_t *data, int64_t bytes, uint8_t *rgb, int64_t cap_bytes, int32_t *w, int32_t *h);
int icl_load_image_224_mem(const uint8_t *data, int64_t bytes, uint8_t *out);
int icl_preprocess_mem(const uint8_t *data, int64_t bytes, float *nchw);
int icl_embed_image_mem(icl_ctx *ctx, const uint8_t *data, int64_t bytes, int head, float *out);
int icl_load_images_224_mem_dev(icl_ctx *ctx, const uint8_t *const *data, const int64_t *bytes, int64_t n, int32_t threads,
                                uint8_t *d_out /* n x 224x224x3 */, int32_t *status);
int icl_embed_images_mem(icl_ctx *ctx, const uint8_t *const *data, const int64_t *bytes, int64_t n, int head, int prec,
                         int32_t threads, float *out, int32_t *status);
int icl_embed_images_mem_dev(icl_ctx *ctx, const uint8_t *const *data, const int64_t *bytes, int64_t n, int head, int prec,
                             int32_t threads, float *d_out, int32_t *status);
int icl_cluster_requests_mem(icl_ctx *ctx, int32_t nreq, const uint8_t *const *data, const int64_t *bytes, const int32_t *n, const int32_t *n_labels,
                             const int64_t *label_off /* sum n[r] + 1 */, const int32_t *label_idx, const int32_t *min_size, const int32_t *max_size,
                             int head, int prec, int32_t threads, int32_t *cluster_id, int32_t *member_rank, int32_t *n_clusters, int32_t *n_merges,
                             int32_t *merges, int32_t *status /* nreq */, int32_t *file_status /* sum n[r] */, float *E_out);
int icl_jpeg_coefs_mem(icl_ctx *ctx, const uint8_t *const *data, const int64_t *bytes, int64_t n, int entropy_mode, int16_t *coefs, int64_t cap,
                       int64_t *offsets /* n + 1 */, int32_t *state /* n */);
/* ---- the label service's downsizer: resizeImageIfNeeded (internal/rekognition/rekognition.go:173-259) and the JPEG encoder it needs ----
 * icl_jpeg_encode_rgb (host only): interleaved u8 RGB -> a complete JPEG file, the bytes libjpeg(-turbo) writes after jpeg_set_defaults +
 * jpeg_set_quality(quality, TRUE): baseline SOF0, YCbCr 4:2:0, Annex K Huffman tables, islow DCT, JFIF 1.01 (pinned byte for byte to Pillow;
 * cv::imwrite(".jpg") makes the same libjpeg calls).  *bytes receives the file's size; out == NULL asks for the size alone; cap < size is
 * ICL_ERR_ARG with *bytes set.  quality 1..100, 1 <= w, h <= 65535, else ICL_ERR_ARG.
 * icl_jpeg_encode_bound(w, h): an upper bound on that size for every image and quality (0 for a size the encoder rejects): 625 header and
 * EOI bytes + per 8x8 block 64 coefficients of at most 27 bits (a 16-bit code + 11 amplitude bits; ZRL and EOB only replace zeros and cost
 * less), i.e. 216 bytes, doubled for the 0x00 stuffed behind every 0xFF, over the 6 blocks of each 16x16 MCU, + 2 for the padded last byte.
 * icl_jpeg_encode_rgb_dev: the same files for n resident images in one call on the context's stream.  Image i is d_rgb + offsets[i],
 * w[i] x h[i]; file i is out[out_off[i] .. out_off[i + 1]) (out_off: host, n + 1).  out_on_device != 0: out is device memory.  cap too
 * small is ICL_ERR_ARG with out_off filled (out_off[n] is the size needed) and out unspecified.
 * icl_downsize_image_file / _mem (host only): resizeImageIfNeeded with its limits as arguments (the reference: 5 MiB, 2048).  bytes <=
 * max_bytes: the input comes back unchanged, undecoded, image or not.  Otherwise IMRead(IMReadColor) (EXIF orientation applied), and with
 * R rows, C columns: ratio = double(C) / R; R > C ? (newW = max_dim, newH = int(max_dim * ratio)) : (newH = max_dim, newW = int(max_dim /
 * ratio)) -- THE REFERENCE READS gocv's Size() = [rows, cols] AS (width, height), SO A 4000x3000 LANDSCAPE PHOTO BECOMES 1536 WIDE x 2048 HIGH;
 * a drop-in keeps that distortion.  cv::resize INTER_LINEAR, JPEG at quality 95; still above max_bytes: once more at newW / 2 x newH / 2 from
 * the decoded original, returned whatever its size (a halved size of 0 returns the first result).  newW or newH < 1: ICL_ERR_ARG.  A file the
 * decoders reject returns their code and message.  Two-call size query as above.  info (may be NULL): passthrough (0 / 1), decoded W, H
 * (after orientation), final newW, newH, attempts (0 for a passthrough).
 * icl_downsize_images / _mem: the batched form.  Row i belongs to image i: output i is out[out_off[i] .. out_off[i + 1]) and equals
 * icl_downsize_image_mem's on the same bytes, in both entropy modes and for any threads.  A failed image fails alone (status[i], empty range);
 * the call returns the code of the lowest failed index.  Images at or under the limit are copied on the host; JPEGs above it are rebuilt on
 * the GPU from their coefficients (planes -> gather + resize at the new size -> encoder kernels); PNG, PPM and JPEGs too large for a slab
 * are decoded and resized on the host and encoded on the GPU.  cap too small: ICL_ERR_ARG, out_off[n] is the size needed.
 * icl_last_downsize_stats: counts of the last batched call (passthrough + gpu_rebuilt + host_decoded + failed == n) and its stage times. */
int64_t icl_jpeg_encode_bound(int32_t w, int32_t h);
int icl_jpeg_encode_rgb(const uint8_t *rgb, int32_t w, int32_t h, int32_t quality, uint8_t *out, int64_t cap, int64_t *bytes);
int icl_jpeg_encode_rgb_dev(icl_ctx *ctx, const uint8_t *d_rgb, const int64_t *offsets, const int32_t *w, const int32_t *h, int64_t n, int32_t quality,
                            uint8_t *out, int32_t out_on_device, int64_t cap, int64_t *out_off /* n + 1 */);
int icl_downsize_image_file(const char *path, int64_t max_bytes, int32_t max_dim, uint8_t *out, int64_t cap, int64_t *bytes, int32_t *info /* 6 */);
int icl_downsize_image_mem(const uint8_t *data, int64_t in_bytes, int64_t max_bytes, int32_t max_dim, uint8_t *out, int64_t cap, int64_t *bytes,
                           int32_t *info /* 6 */);
int icl_downsize_images(icl_ctx *ctx, const char *const *paths, int64_t n, int64_t max_bytes, int32_t max_dim, int32_t threads, uint8_t *out,
                        int64_t cap, int64_t *out_off /* n + 1 */, int32_t *status /* n */);
int icl_downsize_images_mem(icl_ctx *ctx, const uint8_t *const *data, const int64_t *bytes, int64_t n, int64_t max_bytes, int32_t max_dim,
                            int32_t threads, uint8_t *out, int64_t cap, int64_t *out_off /* n + 1 */, int32_t *status /* n */);
int icl_last_downsize_stats(icl_ctx *ctx, int64_t *passthrough, int64_t *gpu_rebuilt, int64_t *host_decoded, int64_t *second_attempts, int64_t *bytes_in,
                            int64_t *bytes_out, double *stage_ms /* 3: host decode (thread-ms), GPU rebuild + encode, download + copy */);
/* workflow.go:84-94 on one GPU in one call: embed n resident images (2048-d pooled head, into d_E: device, n x 2048) and
 * cluster them.  flags & ICL_FUSE_OVERLAP: the distance rows of already-embedded images are computed on a side stream of the
 * context while later batches embed (same kernels, same results as icl_embed_u8_dev + icl_cluster_dev, bit for bit). */
enum { ICL_FUSE_OVERLAP = 1 };
int icl_embed_cluster_dev(icl_ctx *ctx, const uint8_t *d_hwc_rgb, int64_t n, int prec, int32_t min_size, int32_t max_size, int update, int flags,
                          float *d_E, int32_t *cluster_id, int32_t *member_rank, int32_t *n_clusters);
/* How the exact mode builds ComputeInitialDistanceMatrix (clustering.go:61-73).  ICL_DIST_EXACT: every value by the exact
 * vector-ALU kernel (3 D unfused fp32 ops per pair).  ICL_DIST_BOUND: proven lower bounds from an f32 GEMM on the matrix cores,
 * made exact on demand -- the reference's own sequential fp32 expression -- by the row scans of the merge loop; the same
 * cluster ids, member order, merge log and merge values, bit for bit.  UpdateDistanceMatrix's new rows (clustering.go:75-108) are
 * always values from the exact vector-ALU kernel (round 3 also offered them as bounds: parity-green, slower, retired; the
 * old name ICL_DIST_BOUND_INIT stays as an alias of ICL_DIST_BOUND).  ICL_DIST_AUTO (default): ICL_DIST_LWBOUND for n >= 4096 (with
 * exact rows like ICL_DIST_BOUND where its conditions do not hold: D % 4 != 0, a sharded group call), ICL_DIST_EXACT below. */
enum { ICL_DIST_AUTO = 0, ICL_DIST_EXACT = 1, ICL_DIST_BOUND = 2, ICL_DIST_BOUND_INIT = 3,
       /* ICL_DIST_BOUND plus: the rows UpdateDistanceMatrix (clustering.go:76-96) gives the new clusters are proven lower bounds as well,
        * from the Lance-Williams recurrence on the stored entries (12 bytes instead of 3 D operations per entry), evaluated exactly on
        * demand like the bounds of the initial matrix.  Same results bit for bit. */
       ICL_DIST_LWBOUND = 4 };
int icl_set_ward_options(icl_ctx *ctx, int dist_mode);
/* The merge sequence of the last icl_cluster call on this context: pairs (creation id of the higher-position
 * cluster, creation id of the lower-position one); returns the number of merges performed. */
int64_t icl_last_merges(icl_ctx *ctx, int32_t *pairs, int64_t cap_pairs);
/* Ward distance (clustering.go:84) of the pair joined by each merge of that log, i.e. the dendrogram heights: the
 * value FindClosestClusters found (:123-131).  Returns the number of merges; fills min(cap, merges) values. */
int64_t icl_last_merge_values(icl_ctx *ctx, float *vals, int64_t cap);
/* MFMA distance tile alone (north_star K6): D~[i][j] = 0.5*(|e_i|^2+|e_j|^2-2 e_i.e_j), bf16x3 split operands,
 * fp32 accumulate; lower triangle incl. diagonal written, packed row-major with leading dimension ld.  An estimate that
 * comes out negative or -0 (rounding noise of near-duplicate rows) is stored as +0, a NaN stays a NaN: this is, entry for
 * entry, the matrix ICL_UPDATE_LW clusters.  d_D must be 16-byte aligned (rows are written with 16-byte stores when ld % 4 == 0);
 * cells above the diagonal and in the pad columns n..ld are not written. */
int icl_distance_mfma_dev(icl_ctx *ctx, const float *d_E, int64_t n, int32_t d, float *d_D, int64_t ld);
/* The same tile for m seed clusters of |seed_size[i]| items each (host memory, the sign is ignored): entry (i, j), i > j, is
 * clamp0(fl(fl(f32(s_i s_j) / f32(s_i + s_j)) * fl(2 D~(i, j)))), D~ the entry icl_distance_mfma_dev gives for the same rows -- entry for
 * entry the matrix icl_cluster_seeded_fast clusters; with every size 1 it is D~ itself.  Layout, diagonal (0), alignment and the cells that
 * are not written are icl_distance_mfma_dev's.  ICL_ERR_ARG also for a size of 0 or of 2^30 items and more. */
int icl_distance_mfma_seeded_dev(icl_ctx *ctx, const float *d_C, int64_t m, int32_t d, const int32_t *seed_size, float *d_D, int64_t ld);

/* ---- synthetic inputs ---------------------------------------------------------------------- */
/* Images first..first+n-1 of the seeded synthetic set, u8 HWC RGB 224x224x3. */
int icl_synth_images(uint64_t seed, int64_t first, int64_t n, int mode, uint8_t *out);
int icl_synth_images_dev(icl_ctx *ctx, uint64_t seed, int64_t first, int64_t n, int mode, uint8_t *d_out);

/* ---- in-library HIP-event timing of the kernel classes (bench.py roofline) --------------------------------- */
enum {
    ICL_K_CONV = 0,       /* implicit-GEMM conv launches, 128x128 tile (conv_igemm_kernel<*,128>) */
    ICL_K_DIST_EXACT = 1, /* exact Ward distance tile (K6x) */
    ICL_K_DIST_MFMA = 2,  /* MFMA distance tile (K6) */
    ICL_K_ROWMIN = 3,     /* masked row argmin scans (K7) */
    ICL_K_UPDATE = 4,     /* per-merge exact row update (K8) */
    ICL_K_EMBED_OTHER = 5,/* im2col, pooling, fc */
    ICL_K_CONV64 = 6,     /* implicit-GEMM conv launches, 128x64 tile (Cout == 64 layers) */
    ICL_K_NCLASS = 7
};
/* class_mask: bit k enables HIP-event bracketing of kernel class k (0 = off, -1 = all). */
int icl_prof_enable(icl_ctx *ctx, int class_mask);
int icl_prof_reset(icl_ctx *ctx);
/* Accumulated since reset: device milliseconds, launches, algorithmic flops, algorithmic bytes. */
int icl_prof_query(icl_ctx *ctx, int kclass, double *ms, int64_t *launches, double *flops, double *bytes);
/* Stage wall times (ms, HIP events on the context stream) of the last embed / cluster call. */
int icl_last_stage_ms(icl_ctx *ctx, double *embed_ms, double *dist_ms, double *merge_ms);
/* Shape of the last icl_cluster[_dev] merge loop: merges done, update-kernel launches that carried work ("steps"; the
 * exact mode attempts several independent merges per launch, ICL_UPDATE_LW one), steps that fell back to a single
 * pick, and the sum over steps of the live cluster count (x 4*D bytes = centroid bytes streamed by the update kernel). */
int icl_last_ward_stats(icl_ctx *ctx, int64_t *merges, int64_t *steps, int64_t *single_pick_steps, int64_t *sum_live);
/* Which pipeline the last icl_cluster[_dev] merge loop actually ran -- the options are requests, the engine falls back where a mode's
 * conditions do not hold (D % 4 != 0, a packed size/id word that does not fit, ICL_WARD_BATCH=0, a sharded group call): row_mode = the kernel
 * that made the new clusters' rows, init_bounds = 1 when the initial matrix was filled with matrix-core lower bounds. */
enum { ICL_ROWS_SINGLE = 0,      /* one merge per step, exact rows (ward_update_exact_kernel) */
       ICL_ROWS_EXACT_BATCH = 1, /* batched, exact rows: 3 D unfused operations per entry (ward_update_batch2_kernel) */
       ICL_ROWS_LW_BOUND = 2,    /* batched, Lance-Williams lower bounds + exact evaluation on demand (ward_update_lb_kernel) */
       ICL_ROWS_LW_FAST = 3,     /* ICL_UPDATE_LW: Lance-Williams values, not bit-identical (ward_update_batch_lw_kernel) */
       ICL_ROWS_SINGLE_APART = 4 }; /* icl_cluster_apart: one merge per step, exact rows under a keep-apart relation (ward_update_apart_kernel) */
int icl_last_ward_mode(icl_ctx *ctx, int32_t *row_mode, int32_t *init_bounds);
/* Layout of the distance matrix of the last merge loop.  complete_rows = 1: one column per CREATION ID (row pitch 2 n + 4 floats, 8 n^2 bytes) and
 * every live row holds the pair (x, y) for every live y -- the bound-rows loop (ICL_ROWS_LW_BOUND) then reads two contiguous rows per merge instead
 * of walking a column ("complete rows").  The engine picks it wherever that loop can run and the wider matrix takes at most half of
 * the device memory (n <= ~134 000 on a 288 GB MI355X; environment ICL_WARD_WIDE=0 / 1 overrides the memory rule for tests and A/B runs);
 * complete_rows = 0: recycled columns, row pitch n, 4 n^2 bytes (every other loop, and n = 250 000). */
int icl_last_ward_layout(icl_ctx *ctx, int32_t *complete_rows, int64_t *row_pitch, int32_t *int8_bounds);
/* (int8_bounds = 1: the bounds of the initial matrix came from the integer GEMM of distance_i8.hip -- exact int8 matrix-core arithmetic on a
 * fixed-point image of the rows, what the engine uses when one GPU fills the whole matrix and D <= 2048; 0: from the f32 fmaf-chain GEMM --
 * delivered rows, D > 2048, ICL_DIST_I8=0 -- or no bounds at all.) */
/* Run-time check of the distance bounds' soundness: every flagged entry (a proven lower bound, ward.hip) that the last merge loop's row scans
 * made exact was compared with the value that replaced it; the number of values found BELOW their bound.  0 by the error analysis of DESIGN.md 3;
 * anything else means a wrong bound could have hidden a pair, and the tests assert 0. */
int64_t icl_last_ward_bound_violations(icl_ctx *ctx);

/* Test hook for the distance bounds of the exact mode's initial matrix: ALL n (n - 1) / 2 pairs of E [n][d] -- the bounds by the
 * production kernels (kind 0: what icl_cluster_dev would use for this shape, 1: the f32 fmaf-chain GEMM, 2: the integer GEMM of
 * distance_i8.hip, D <= 2048), the values by the exact kernel -- and counts the pairs whose value lies BELOW its lower bound, ABOVE the upper
 * bound the row scans derive from it, and the entries that came out without the flag; sum_gap / sum_val: sum of (value - bound) and of the
 * values (the bounds' mean tightness).  The merge loop itself only meets the few entries near a row's minimum. */
int icl_distance_bounds_check_dev(icl_ctx *ctx, const float *d_E, int64_t n, int32_t d, int kind, int64_t *below, int64_t *above, int64_t *unflagged,
                                  double *sum_gap, double *sum_val);
/* Test hook for the matrix the merge loop works on ("every entry of the final matrix"): the Ward workspace exactly as the last
 * icl_cluster[_dev] call on this context left it, for the L creation ids the caller names (the test derives the live set from the merge log; the
 * engine's own idea of who is alive is not used).  Nothing in the workspace is changed.  Host outputs:
 *   sizes [L], centroids [L][d]: what the engine holds for the cluster (a singleton's centroid is its embedding row);
 *   row_filled [L]: 1 when the cluster's row of the matrix was written (derived from the loop's step state; every loop ends with all rows filled);
 *   entries [L][L]: the raw 32 bits of the entry of the pair (ids[i], ids[j]), sign bit (= "lower bound, not a value") included, read the way
 *     the kernels read it; 0 on the diagonal;
 *   mirror [L][L]: the second copy the complete-rows layout keeps in the row of the pair's OLDER cluster; all 0 in the recycled-column layout;
 *   lb_g1, lb_delta2: the constants of the Lance-Williams bound the call used (0 unless row mode ICL_ROWS_LW_BOUND);
 *   info [6]: row mode (ICL_ROWS_*), complete_rows, n, d, merges done, max_size of that call.
 * ICL_ROWS_EXACT_BATCH and ICL_ROWS_LW_BOUND (both layouts) are covered and tested; ICL_ROWS_SINGLE takes the same path (no test runs it); ICL_ERR_ARG without a finished call on the workspace
 * (or after anything that re-initialised it, icl_distance_bounds_check_dev for one), for an id outside [0, n + merges) or a d (the row length
 * the centroids buffer was sized for) that is not the last call's; ICL_ERR_UNSUPPORTED
 * after a FAST-mode call or on a context of a sharded group. */
int icl_ward_dump_pairs_dev(icl_ctx *ctx, const int32_t *ids, int64_t L, int32_t d, int32_t *sizes, float *centroids, int32_t *row_filled, uint32_t *entries,
                            uint32_t *mirror, float *lb_g1, float *lb_delta2, int32_t *info);

const char *icl_version(void);

#ifdef __cplusplus
}
#endif
#endif
