/*
 * fdnn.h -- C-ABI of the MI355X-native fast-dnn scorer (libfast-dnn.so).
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++ / torch types.
 * The JNI exports the Java class suskun.nn.QuantizedDnn binds
 * (include/fdnn_jni.h) are thin wrappers over these functions, and each entry
 * point cites the reference interface it replaces (paths relative to the
 * reference repository).
 *
 * Conventions
 *   - every function returns FDNN_OK (0) or a negative fdnn_status; the text of
 *     the last error on the calling thread is in fdnn_last_error().
 *   - "host" pointers are ordinary process memory; "device" pointers (d_*) are
 *     HIP device memory on the model's device.  Inputs are const: unlike the
 *     reference (dnn.cc:175-192) the caller's frames are never modified.
 *   - frames are row-major n x input_dim fp32, input_dim being the padded
 *     (multiple of 4) layer-0 width the reference reports (jni_dnn.cc:20-25);
 *     outputs are row-major n x output_dim fp32 soft-max rows.
 *   - a model handle is immutable after load and may be used from many threads
 *     at once (jni_dnn.cc:49-51 gives every call its own context; here calls
 *     draw a device context from a per-model pool).  A context handle is
 *     single-threaded, like the reference's LazyContext.
 *   - stream ordering on a context: the *_device entry points enqueue on the
 *     caller's stream and do not synchronize; the host-pointer entry points use
 *     the context's own stream and return with their result complete.  Calls on
 *     ONE context are ordered behind each other whatever streams they use (each
 *     waits, on the device, for the context's previously enqueued work), so
 *     forward_hidden_device(stream) followed by lazy_output() / read_hidden()
 *     needs no synchronization by the caller.  Caller-owned buffers (d_x,
 *     d_masks, d_out) are the caller's to order.
 *   - there is no CPU fallback: without a usable HIP device every entry point
 *     that computes returns FDNN_E_DEVICE.
 *
 * Device buffers (every d_* argument; tests/test_gpu_caller_buffers.py holds each line below on guarded buffers)
 *   The kernels read and write the caller's memory directly.  Extent: exactly the array the entry point documents --
 *   d_x [n][input_dim], d_raw [n][raw_dim], d_masks [count][output_dim] bytes, d_bits [count][ceil(output_dim / 64)]
 *   words, d_out [n or count][output_dim] (row 0 of d_out / d_masks / d_bits is frame `first` of the call, not of the
 *   context), d_row_ptr [count + 1], d_nodes [nnz or len], d_probs [nnz], [count][len] or [n][k], d_inactive [count],
 *   d_nodes / d_vals of a top-k call [n][k], d_rows [n][width], d_out of a pool call [n][C], d_ref / d_q [n][output_dim].  Nothing outside an input's
 *   extent reaches a result, NOTHING outside an output's extent is written (no padded row of a partial frame tile, no
 *   padded node of the last node tile), and every element of an output is written.  Inputs are never modified.
 *   Alignment: the natural alignment of the ELEMENT (4 bytes for fp32 / int32, 1 for mask bytes, 8 for bit words) is all
 *   any buffer needs -- a slice of a caller's tensor works as it is -- with one exception: d_x of the quantized net
 *   (fdnn_calculate_device, fdnn_calculate_lazy_bits_device, fdnn_calculate_topk_device, fdnn_calculate_pool_device,
 *   fdnn_ctx_forward_hidden_device, fdnn_server_submit_device) must start on a 16-BYTE boundary, because layer 0 moves the frames into LDS in 16-byte
 *   DMA pieces; input_dim is a multiple of 4, so every row and every sub-range of rows of such a buffer qualifies.  Frames
 *   that do not are FDNN_E_ARG before anything is launched.  (d_raw and the float net's d_x are read element by element:
 *   element alignment.)  Some kernels take a faster path where a buffer happens to sit on a 16-byte boundary; results
 *   are bit-identical wherever it sits.
 *   Masks: a mask BYTE is active when it is non-zero, whatever the value (1, 0x80, 0xff alike); of a row's last bit word
 *   only bits 0 .. output_dim % 64 - 1 are looked at when output_dim is no multiple of 64 -- bits past output_dim are
 *   ignored by every entry point, device or host, and need not be cleared.
 */
#ifndef FDNN_H
#define FDNN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FDNN_API __attribute__((visibility("default")))

typedef enum fdnn_status {
  FDNN_OK = 0,
  FDNN_E_ARG = -1,    /* null / out-of-range argument, dimension mismatch */
  FDNN_E_IO = -2,     /* file cannot be opened / short read */
  FDNN_E_FORMAT = -3, /* .bin is not a net this path can run (see fdnn_model_load) */
  FDNN_E_DEVICE = -4, /* no HIP device, or a HIP call failed */
  FDNN_E_NOMEM = -5,
  FDNN_E_STATE = -6   /* call sequence violated (e.g. lazy output before forward_hidden) */
} fdnn_status;

typedef struct fdnn_model fdnn_model; /* replaces dnn::QuantizedDnn*   (dnn.h:106-142) */
typedef struct fdnn_ctx fdnn_ctx;     /* replaces dnn::CalculationContext* (dnn.h:144-208) */

FDNN_API const char *fdnn_last_error(void);
FDNN_API const char *fdnn_version(void);
FDNN_API int fdnn_device_count(void);

/* ------------------------------------------------------------------ model
 * fdnn_model_load <- Java initialize(String, float) / jni_dnn.cc:7-18:
 *   FloatDnn(path) (float_dnn.cc:18-69) + QuantizedDnn(floatDnn, cutoff)
 *   (dnn.cc:511-531).  Reads the big-endian .bin, pads layer-0 input to x4,
 *   quantizes layers 1.. with the reference's per-layer multiplier rule
 *   (dnn.cc:460-509) and uploads one packed weight blob to `device`.
 *   Accepts what the reference can run: >= 4 affine layers (dnn.cc:199 needs
 *   layers()[1] to be a hidden layer), all hidden widths equal and x16
 *   (README.md:10,:69); otherwise FDNN_E_FORMAT.  cutoff must be > 0
 *   (QuantizedDnn.java:55-57). */
FDNN_API int fdnn_model_load(const char *path, float cutoff, fdnn_model **out);
FDNN_API int fdnn_model_load_on(const char *path, float cutoff, int device, fdnn_model **out);
/* <- Java delete() / jni_dnn.cc:128-133.  Contexts must be freed first. */
FDNN_API void fdnn_model_free(fdnn_model *m);

/* <- inputDimension / outputDimension / layerCount / layerDimension,
 *    jni_dnn.cc:20-33, :135-156.  layer_count = quantized layers + 1;
 *    layer_dim(0) = layer-0 node count, layer_dim(k>=1) = node count of
 *    quantized layer index k as the reference indexes it (layers()[k], i.e.
 *    affine layer k+1); out of range -> -1.  The reference reads one past the
 *    end for k == layer_count-1 (its bound check is off by one); here that
 *    index returns -1. */
FDNN_API int fdnn_model_input_dim(const fdnn_model *m);
FDNN_API int fdnn_model_output_dim(const fdnn_model *m);
FDNN_API int fdnn_model_hidden_dim(const fdnn_model *m);
FDNN_API int fdnn_model_layer_count(const fdnn_model *m);
FDNN_API int fdnn_model_layer_dim(const fdnn_model *m, int index);
FDNN_API int fdnn_model_device(const fdnn_model *m);

/* Numeric flavour of the fp32 input layer.
 *   0 (default) -- unfused multiply then add, four k-mod-4 partial sums
 *                  combined (l0+l1)+(l2+l3): the reference built
 *                  -O2 -msse4 -ffp-contract=off (dnn.cc:219-247, :168-172).
 *   1           -- the same chains with fused multiply-add, i.e. the reference
 *                  built with its own Makefile's -march=native on an FMA host. */
FDNN_API int fdnn_model_set_l0_fma(fdnn_model *m, int on);

/* How the list entry points (fdnn_ctx_lazy_output_lists, _lists_device, fdnn_calculate_lazy_lists and what goes through
 * them; LazyOutputActivations, dnn.cc:355-392) score their entries.
 * 0 (default): the dot-product kernels, exactly as today.  g in 1..8: lists are scored on the int8 MFMA over the union of
 * each group of 32 * g consecutive rows of the call (groups counted from `first`); -1: on, with the library's default g.
 * Results are byte-identical either way.  Like fdnn_model_set_l0_fma: set before the model is used from several threads.
 * A layer the MFMA tile's shape does not apply to (K > 2048, output_dim > 65536) is served by the dot-product kernels.
 * Any other value is FDNN_E_ARG.  The scoring loop, device groups and the JNI shim do not look at the switch. */
FDNN_API int fdnn_model_set_lists_union(fdnn_model *m, int group_tiles);

/* ------------------------------------------------------------------ dense path
 * fdnn_calculate <- Java calculate(long, float[], int, int, int) /
 *   jni_dnn.cc:35-62 -> CalculationContext::Calculate (dnn.cc:162-165).
 *   x: host n x dim, out: host n x output_dim.  dim must equal input_dim
 *   (QuantizedDnn.java:157-161).  n == 0 is a no-op.  batch_hint is the
 *   reference's frame-block size; results never depend on it. */
FDNN_API int fdnn_calculate(fdnn_model *m, const float *x, int n, int dim, int batch_hint, float *out);
/* Same computation on device-resident buffers (the roofline path): d_x and
 * d_out live on the model's device, work is enqueued on `stream` (a
 * hipStream_t; NULL = default stream) and NOT synchronized. */
FDNN_API int fdnn_calculate_device(fdnn_model *m, const float *d_x, int n, float *d_out, void *stream);

/* One-call lazy scoring: CalculateUntilLastHiddenLayer (dnn.cc:402-424) + LazyOutputActivations
 * (dnn.cc:355-392) for every frame of the call, in one call and one stream synchronisation -- what a LazyContext does in
 * two calls per utterance (QuantizedDnn.java:72-107), without the per-frame JNI round trips README.md:45 complains about.
 *   fdnn_calculate_lazy       masks [n][output_dim] bytes, non-zero = active (the JNI contract's byte masks)
 *   fdnn_calculate_lazy_bits  bits [n][ceil(output_dim / 64)] 64-bit words, bit b of word w = node 64 w + b
 * out [n][output_dim]: active nodes their probability, inactive nodes 1 / total (dnn.cc:366-369, :389).  Host callers get
 * their rows back COMPACTED over PCIe (active probabilities + one value per frame) and rebuilt in `out`.
 * The _device form works on device-resident buffers, enqueued on `stream`, not synchronised. */
FDNN_API int fdnn_calculate_lazy(fdnn_model *m, const float *x, int n, int dim, const int8_t *masks, float *out);
FDNN_API int fdnn_calculate_lazy_bits(fdnn_model *m, const float *x, int n, int dim, const uint64_t *bits, float *out);
FDNN_API int fdnn_calculate_lazy_bits_device(fdnn_model *m, const float *d_x, int n, const uint64_t *d_bits, float *d_out, void *stream);

/* ------------------------------------------------------------------ raw feature frames: the <Splice> block on the device
 * Every net this library runs reads SPLICED rows: row t is the raw feature frames t + o_0 .. t + o_{C-1} side by side
 * (a Kaldi nnet1 final.feature_transform starts with <Splice> [ -5 .. 5 ]; the reference's converter reads that block and
 * drops it, FeedForwardNetwork.java:97-100, so its callers splice on the host: 11 copies of every frame over PCIe).
 * With a splice spec set, the entry points below take the RAW frames and build the rows on the device.
 *
 *   spec       offsets o_0 .. o_{C-1} (1 <= C <= 64, each |o| <= 64, any order, duplicates allowed) and the raw frame
 *              width D, with C * D <= input_dim (the padded layer-0 width).
 *   row t      raw[f(t + o_0)] || ... || raw[f(t + o_{C-1})], then zeros up to input_dim (BatchData.alignDimension).
 *   f          whole utterance: the frame index clamped to the utterance's first and last frame (Kaldi's edge rule).
 *              stream: frame 0 of the stream is the left clamp; frame t is complete once raw frame t + max(o, 0) has
 *              arrived; at the end of the stream the rest is flushed, right-clamped to the last frame.
 *   results    the rows are copies, so every result is BIT-IDENTICAL to the same entry point on the host-spliced rows
 *              (convert.splice_frames).
 *
 * Every raw entry point returns FDNN_E_STATE while no spec is set and FDNN_E_ARG when raw_dim is not the spec's D.  Raw
 * frames are row-major [n][D] fp32; one raw frame gives one output row.
 *
 * fdnn_model_set_splice  sets the spec; count == 0 with raw_dim == 0 clears it (count == 0 with a width is FDNN_E_ARG).  Like fdnn_model_set_l0_fma: set it before the model is used
 *   from several threads.  On a group-attached model it applies to every replica (fdnn_group_attach hands the leader's
 *   spec to the replicas, and a sharded call splices every shard by the leader's).  A call in progress, a stream and a
 *   queued server submission keep the spec they started with.  Contexts that never splice do not grow;
 *   a context allocates its raw buffer (and, in the scoring loop, its frame buffer) on its first raw call.
 * fdnn_model_get_splice  copies up to `cap` offsets and D (raw_dim may be NULL); returns the offset count (0: no spec).
 * fdnn_calculate_raw     one utterance, host to host, n output rows; n == 0 is a no-op.  Routed like fdnn_calculate:
 *   sharded over an attached group first, each replica uploading only the raw frames its rows reference (its shard plus
 *   the halo), and through the batcher of the model that scores the rows when one is on (fdnn_model_enable_batcher /
 *   FDNN_BATCHER).  A large utterance's raw frames are uploaded
 *   once and spliced chunk by chunk (fdnn_debug_frame_chunks) before each chunk's hidden layers.
 * fdnn_calculate_raw_device  device buffers d_raw [n][D], d_out [n][output_dim]; seg_starts (host, n_segs entries, first
 *   0, strictly ascending) cuts the n frames into utterances, each with its own edges; NULL = one utterance.  Enqueued on
 *   `stream`, not synchronised.
 * fdnn_calculate_lazy_bits_raw  the one-call lazy contract (fdnn_calculate_lazy_bits) on raw frames, rows back compacted.
 * fdnn_ctx_forward_hidden_raw   calculateUntilOutput on fdnn_ctx_frame_count(c) raw frames of one utterance; then
 *   fdnn_ctx_output*, fdnn_ctx_lazy_output* and fdnn_ctx_read_hidden work unchanged. */
FDNN_API int fdnn_model_set_splice(fdnn_model *m, const int *offsets, int count, int raw_dim);
FDNN_API int fdnn_model_get_splice(const fdnn_model *m, int *offsets, int cap, int *raw_dim);
FDNN_API int fdnn_calculate_raw(fdnn_model *m, const float *raw, int n, int raw_dim, float *out);
FDNN_API int fdnn_calculate_raw_device(fdnn_model *m, const float *d_raw, int n, const int *seg_starts, int n_segs, float *d_out,
                                       void *stream);
FDNN_API int fdnn_calculate_lazy_bits_raw(fdnn_model *m, const float *raw, int n, int raw_dim, const uint64_t *bits, float *out);
FDNN_API int fdnn_ctx_forward_hidden_raw(fdnn_ctx *c, const float *raw);

/* Streams: an utterance scored as it arrives, chunk by chunk (a real-time recogniser's feed).  The stream keeps the spec
 * it was created with, and its last max(-o, 0) + max(o, 0) raw frames on the device (never uploaded twice).
 * fdnn_stream_create     max_chunk: the most raw frames one push may carry.
 * fdnn_stream_reset      the next push starts a new utterance (also after a push with `end`, which closes the stream:
 *                        a further push without a reset is FDNN_E_STATE).
 * fdnn_stream_position   raw frames pushed and rows emitted since the utterance started.
 * fdnn_stream_push       n_raw (0 .. max_chunk) raw frames; scores the frames this push completes, in order, into out
 *   [*n_out][output_dim] (at most n_raw + max(o, 0) rows).  end != 0 flushes the rest (n_raw = 0 is a flush only).  With
 *   out == NULL only the hidden layers run: fdnn_stream_ctx(s) is then a context (owned by the stream; do not free it)
 *   whose frames 0 .. *n_out - 1 are exactly those frames, for the lazy entry points -- the reference's LazyContext
 *   protocol (calculateUntilOutput, then per-frame masks; QuantizedDnn.java:72-107), chunk by chunk.  Host-synchronous. */
typedef struct fdnn_stream fdnn_stream;
FDNN_API int fdnn_stream_create(fdnn_model *m, int max_chunk, fdnn_stream **out);
FDNN_API void fdnn_stream_free(fdnn_stream *s);
FDNN_API int fdnn_stream_reset(fdnn_stream *s);
FDNN_API int fdnn_stream_position(const fdnn_stream *s, int64_t *pushed, int64_t *emitted);
FDNN_API int fdnn_stream_push(fdnn_stream *s, const float *raw, int n_raw, int end, float *out, int *n_out);
FDNN_API fdnn_ctx *fdnn_stream_ctx(fdnn_stream *s);

/* ------------------------------------------------------------------ contexts / lazy path
 * fdnn_ctx_create <- getContext / jni_dnn.cc:64-77 (CalculationContext ctor,
 *   dnn.cc:194-215): device scratch for n frames. */
FDNN_API int fdnn_ctx_create(fdnn_model *m, int n, int batch_hint, fdnn_ctx **out);
/* <- deleteLazyContext / jni_dnn.cc:119-126 */
FDNN_API void fdnn_ctx_free(fdnn_ctx *c);
FDNN_API int fdnn_ctx_frame_count(const fdnn_ctx *c);
FDNN_API int fdnn_ctx_output_dim(const fdnn_ctx *c);
/* <- calculateUntilOutput / jni_dnn.cc:79-95 -> CalculateUntilLastHiddenLayer
 *    (dnn.cc:402-424).  x: host n x input_dim. */
FDNN_API int fdnn_ctx_forward_hidden(fdnn_ctx *c, const float *x);
FDNN_API int fdnn_ctx_forward_hidden_device(fdnn_ctx *c, const float *d_x, void *stream);
/* <- calculateLazy / jni_dnn.cc:97-117 -> LazyOutputActivations
 *    (dnn.cc:355-392): one frame, mask of output_dim bytes (non-zero = active).
 *    Masked-out nodes keep logit 0, contribute exp(0) to the soft-max
 *    denominator and come back as 1/total.  out: host output_dim floats.
 *    frame >= n leaves the reference with a partially written buffer; here it
 *    is FDNN_E_ARG. */
FDNN_API int fdnn_ctx_lazy_output(fdnn_ctx *c, int frame, const int8_t *mask, float *out);
/* Batched form of the same contract: frames
 * [first, first+count) with masks[count][output_dim] -> out[count][output_dim]. */
FDNN_API int fdnn_ctx_lazy_output_batch(fdnn_ctx *c, int first, int count, const int8_t *masks, float *out);
FDNN_API int fdnn_ctx_lazy_output_batch_device(fdnn_ctx *c, int first, int count, const int8_t *d_masks, float *d_out,
                                               void *stream);
/* The same with the masks as BITS: bits[count][ceil(output_dim / 64)] 64-bit words, bit b of word w of a row = node
 * 64 w + b active (bits past output_dim ignored).  A decoder that keeps its active set as a bit set hands it over as it
 * is: an eighth of the bytes over PCIe / HBM and no pack pass (LazyOutputActivations, dnn.cc:355-392: inactive nodes
 * contribute exp(0) to the sum and all read 1 / total). */
FDNN_API int fdnn_ctx_lazy_output_batch_bits(fdnn_ctx *c, int first, int count, const uint64_t *bits, float *out);
FDNN_API int fdnn_ctx_lazy_output_batch_bits_device(fdnn_ctx *c, int first, int count, const uint64_t *d_bits, float *d_out, void *stream);
/* Lazy output by ACTIVE-NODE LISTS: only the listed nodes are scored (LazyOutputActivations, dnn.cc:355-392, exists to skip
 * the nodes a decoder does not ask for; the masked entry points above compute the whole layer and mask).  For narrow
 * active sets -- forced alignment, lattice rescoring, keyword spotting: a few nodes per frame -- and the per-frame protocol.
 * The caller opts in: nothing is routed here by itself (INTEGRATION.md states the measured crossover).
 *   lists   for rows first .. first + count - 1 of a context whose hidden layers have run: row_ptr [count + 1] int32,
 *           row_ptr[0] == 0, non-decreasing, row_ptr[count] == nnz; nodes [nnz] int32, strictly ascending inside a row
 *           and in [0, output_dim).  Such a list is exactly a mask.
 *   probs   [nnz]: entry i's probability under the lazy contract -- listed nodes have the logit f32(f32(acc) / coef) +
 *           bias, every unlisted node the logit 0 and contributes exp(0) = 1 to the total (dnn.cc:366-369).
 *   inactive [count]: the value every unlisted node of that row reads, 1 / total (dnn.cc:389).  An empty row gives
 *           1 / output_dim; a row that lists every node is the dense soft-max.
 * The row total is summed in one fixed order, so a row's bytes do not depend on the batch it was
 * scored in, its position or the entry point.
 * fdnn_ctx_lazy_output_lists         host buffers, host-synchronous; validates the lists: FDNN_E_ARG names the row.
 *   FDNN_E_STATE before the hidden layers, FDNN_E_ARG for rows outside the context (as fdnn_ctx_lazy_output_batch_bits).
 * fdnn_ctx_lazy_output_lists_device  device buffers, enqueued on `stream`, not synchronised, ordered on the context like
 *   the other *_device entries.  The lists are NOT validated: a node outside [0, output_dim) is never used as an address,
 *   its row's entries and inactive value come back NaN; row_ptr values are clamped to [0, nnz].
 * fdnn_calculate_lazy_lists          one call: pooled context, hidden layers + lists; a large n goes chunk by chunk
 *   (fdnn_debug_frame_chunks), each chunk with its slice of the lists rebased.  LazyOutputActivations, dnn.cc:355-392. */
FDNN_API int fdnn_ctx_lazy_output_lists(fdnn_ctx *c, int first, int count, const int32_t *row_ptr, const int32_t *nodes, float *probs,
                                        float *inactive);
FDNN_API int fdnn_ctx_lazy_output_lists_device(fdnn_ctx *c, int first, int count, const int32_t *d_row_ptr, const int32_t *d_nodes,
                                               int nnz, float *d_probs, float *d_inactive, void *stream);
FDNN_API int fdnn_calculate_lazy_lists(fdnn_model *m, const float *x, int n, int dim, const int32_t *row_ptr, const int32_t *nodes,
                                       float *probs, float *inactive);
/* Lazy output for ONE NODE SET shared by a row range: the list contract above with the same list in every row -- forced
 * alignment (the transcript's states), keyword spotting, n-best rescoring.  The set's weight rows are read once per frame
 * tile and scored on the int8 matrix pipe (fdnn_set.hip) instead of once per (row, node).
 *   nodes    [len] int32, strictly ascending, each in [0, output_dim), 0 <= len <= output_dim
 *   probs    [count][len] row-major: probs[r][j] = node nodes[j]'s probability in row first + r under the lazy contract
 *   inactive [count]: the 1 / total every unlisted node of that row reads.  len == 0 gives 1 / output_dim per row and no
 *            probs; len == output_dim is the dense soft-max.  count x len must fit an int32 (FDNN_E_ARG otherwise).
 * The result for (row, set) is byte-identical to fdnn_ctx_lazy_output_lists called with the set as every row's list: a
 * row's bytes depend on the row and the set only, not on first, count or the entry point.  Several utterances in one
 * context: one call per utterance's row range.
 * fdnn_ctx_lazy_output_set         host buffers, host-synchronous; validates the set (FDNN_E_ARG for a malformed set or
 *   rows outside the context, FDNN_E_STATE before the hidden layers).
 * fdnn_ctx_lazy_output_set_device  device buffers, enqueued on `stream`, not synchronised, ordered on the context like the
 *   other *_device entries.  The set is NOT validated: a node outside [0, output_dim) is never used as an address, its
 *   column's e is NaN, so every row's entries and inactive value come back NaN.
 * fdnn_calculate_lazy_set          one call: pooled context, hidden layers + the set; a large n goes chunk by chunk
 *   (fdnn_debug_frame_chunks), every chunk with the same set.  LazyOutputActivations, dnn.cc:355-392. */
FDNN_API int fdnn_ctx_lazy_output_set(fdnn_ctx *c, int first, int count, const int32_t *nodes, int len, float *probs, float *inactive);
FDNN_API int fdnn_ctx_lazy_output_set_device(fdnn_ctx *c, int first, int count, const int32_t *d_nodes, int len, float *d_probs,
                                             float *d_inactive, void *stream);
FDNN_API int fdnn_calculate_lazy_set(fdnn_model *m, const float *x, int n, int dim, const int32_t *nodes, int len, float *probs,
                                     float *inactive);
/* Lazy output for PER-SEGMENT NODE SETS: the set contract above with one set per segment of a row range, all segments in one
 * call -- many utterances in one context, each with its own set (its transcript's states).  Up to 64 segments share one
 * launch of the set kernel's tile (fdnn_sets.hip); LazyOutputActivations, dnn.cc:355-392.
 *   seg_rows [n_segs + 1] int32, HOST memory in every form: non-decreasing; segment s = rows [seg_rows[s], seg_rows[s + 1])
 *            of the context; seg_rows[0] >= 0, seg_rows[n_segs] <= frame count; empty segments allowed
 *   set_ptr  [n_segs + 1] int32, HOST memory in every form: set_ptr[0] == 0, non-decreasing; segment s's set is
 *            nodes[set_ptr[s] .. set_ptr[s + 1])
 *   nodes    [set_ptr[n_segs]] int32, strictly ascending inside each segment's set, each in [0, output_dim)
 *   probs    ragged: segment s's block starts at sum_{t < s} rows_t * len_t and is [rows_s][len_s] row-major
 *   inactive [seg_rows[n_segs] - seg_rows[0]]: one 1 / total per row, in row order
 * The sum of rows_s * len_s must fit an int32 (FDNN_E_ARG otherwise); n_segs == 0 is a no-op; a segment with len == 0 gives
 * 1 / output_dim per row and no probs.  This is the list contract's CSR with row_ptr[r] = block start + r_local * len_s.
 * A row's bytes depend on the row and its set only: they equal fdnn_ctx_lazy_output_set on that segment alone and
 * fdnn_ctx_lazy_output_lists with the sets repeated per row (dnn.cc:355-392 in each).
 * fdnn_ctx_lazy_output_sets         host buffers, host-synchronous; validates tables and sets (FDNN_E_ARG names the first
 *   malformed segment, FDNN_E_STATE before the hidden layers).
 * fdnn_ctx_lazy_output_sets_device  device buffers (d_nodes, d_probs, d_inactive), enqueued on `stream`, not synchronised,
 *   ordered on the context like the other *_device entries; the tables are read before the call returns.  The tables are
 *   checked, the sets are NOT: a node outside [0, output_dim) is never used as an address, it makes ITS segment's rows NaN
 *   (entries and inactive values) and no other's.
 * fdnn_calculate_lazy_sets          one call: pooled context, hidden layers + the sets; seg_rows must cover [0, n); a large n
 *   goes chunk by chunk (fdnn_debug_frame_chunks), a segment cut by a chunk keeps its set. */
FDNN_API int fdnn_ctx_lazy_output_sets(fdnn_ctx *c, const int32_t *seg_rows, const int32_t *set_ptr, int n_segs, const int32_t *nodes,
                                       float *probs, float *inactive);
FDNN_API int fdnn_ctx_lazy_output_sets_device(fdnn_ctx *c, const int32_t *seg_rows, const int32_t *set_ptr, int n_segs,
                                              const int32_t *d_nodes, float *d_probs, float *d_inactive, void *stream);
FDNN_API int fdnn_calculate_lazy_sets(fdnn_model *m, const float *x, int n, int dim, const int32_t *seg_rows, const int32_t *set_ptr,
                                      int n_segs, const int32_t *nodes, float *probs, float *inactive);
/* Dense output layer over the context's hidden activations
 * (CalculateOutput, dnn.cc:428-454). */
FDNN_API int fdnn_ctx_output(fdnn_ctx *c, float *out);
FDNN_API int fdnn_ctx_output_device(fdnn_ctx *c, float *d_out, void *stream);
/* ------------------------------------------------------------------ dense output with a top-k return (fdnn_topk.hip)
 * The dense soft-max with the DEVICE choosing what to return: of every row the k first-ranked nodes and their
 * probabilities, 1 <= k <= min(row width, 256) -- n x k x 8 bytes instead of n x output_dim x 4.  The contract, for a row
 * p[0 .. W) of fp32 values:
 *   key(v) = u ^ (u >> 31 ? 0xffffffff : 0x80000000) for the 32 bits u of v: the usual total order on floats,
 *   -NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN, with no special case (rows of the unstabilised soft-max can hold inf / NaN);
 *   node i ranks before node j when key(p[i]) > key(p[j]), or the keys are equal and i < j;
 *   nodes[0 .. k) / vals[0 .. k) are the k first-ranked nodes in rank order and their values, the row's own 32 bits.
 * The top k is a prefix of the top k + 1.  A result depends on its row and k only: not on n, the row's position, the entry
 * point, the batch it rode in or the kernel form that served it.  Results are [n][k] row-major.  FDNN_E_ARG for k outside
 * its range.  Nothing is routed here: the batcher (fdnn_model_enable_batcher), device groups and the JNI shim neither route
 * to nor look at any of these entry points, and every other entry point keeps its bytes.
 *
 * fdnn_topk_rows_device       the selection alone on any device-resident [n][width] fp32 rows of the CURRENT device (behind
 *   fdnn_calculate_device, fdnn_float_calculate_device or the lazy *_device forms, for instance; extends CalculateOutput,
 *   dnn.cc:428-454).  Enqueued on `stream`, not synchronised; n == 0 is a no-op; FDNN_E_ARG for null pointers or width < 1.
 * fdnn_ctx_output_topk        fdnn_ctx_output's computation (CalculateOutput, dnn.cc:428-454) into the context's own rows,
 *   then the selection; host buffers, host-synchronous.  FDNN_E_STATE before the hidden layers.  Works unchanged on
 *   fdnn_stream_ctx(s) after a hidden-only push.
 * fdnn_ctx_output_topk_device the same with device buffers, enqueued on `stream`, ordered on the context like the other
 *   *_device entries (CalculateOutput, dnn.cc:428-454).
 * fdnn_calculate_topk         host to host on a pooled context, chunk by chunk like fdnn_calculate (Calculate,
 *   dnn.cc:162-165): only n x k x 8 bytes cross PCIe.  Obeys the re-run rules of the dense host forms.
 * fdnn_calculate_topk_raw     the same from raw feature frames, like fdnn_calculate_raw (Calculate, dnn.cc:162-165).
 * fdnn_calculate_topk_device  device buffers, a pooled context for the intermediate rows; enqueued, not synchronised
 *   (Calculate, dnn.cc:162-165). */
FDNN_API int fdnn_topk_rows_device(const float *d_rows, int n, int width, int k, int32_t *d_nodes, float *d_vals, void *stream);
FDNN_API int fdnn_ctx_output_topk(fdnn_ctx *c, int k, int32_t *nodes, float *probs);
FDNN_API int fdnn_ctx_output_topk_device(fdnn_ctx *c, int k, int32_t *d_nodes, float *d_probs, void *stream);
FDNN_API int fdnn_calculate_topk(fdnn_model *m, const float *x, int n, int dim, int k, int32_t *nodes, float *probs);
FDNN_API int fdnn_calculate_topk_raw(fdnn_model *m, const float *raw, int n, int raw_dim, int k, int32_t *nodes, float *probs);
FDNN_API int fdnn_calculate_topk_device(fdnn_model *m, const float *d_x, int n, int k, int32_t *d_nodes, float *d_probs, void *stream);
/* ------------------------------------------------------------------ dense output pooled over a node -> class map (fdnn_pool.hip)
 * The dense soft-max summed on the DEVICE over classes of output nodes -- the silence posterior of a frame, phone posteriors
 * out of senones, coarse pruning by phone class: n x C x 4 bytes instead of n x output_dim x 4 (192 bytes a frame at 48
 * phones against 32 000).  The reference has no such call; this extends CalculateOutput (dnn.cc:428-454), as top-k does.
 *
 * The map: class_of[0 .. W) of int32 with 1 <= C <= W classes; class_of[i] in [0, C) puts node i into that class, -1 leaves it
 * out of every class, anything else is FDNN_E_ARG.  Classes may be empty.  fdnn_pool_create validates on the host, builds the
 * CSR (class_ptr [C + 1], member [nnz], sorted by class, then by node) and uploads it to the device that is CURRENT at that
 * moment.  A handle is immutable; threads, contexts and scoring loops may share it; it must outlive every call and every
 * ticket that uses it.  A call whose pool width differs from the row width (the model's output_dim), whose pool lives on
 * another device than the model, or whose model leads a device group is FDNN_E_ARG before anything is launched.
 *
 * The sum, for a row p[0 .. W) of fp32 values and a class c with members m_0 < m_1 < ... < m_{L-1}:
 *   s_j = +0.0f;  for t = j, j + 16, j + 32, ... (t < L):  s_j = s_j + p[m_t]          j = 0 .. 15
 *   q_c = (((s_0+s_1)+(s_2+s_3)) + ((s_4+s_5)+(s_6+s_7))) + (((s_8+s_9)+(s_10+s_11)) + ((s_12+s_13)+(s_14+s_15)))
 * every + one fp32 addition, round to nearest even, denormals kept.  An empty class gives +0.0f; a singleton returns its
 * value's own bits (-0 becomes +0); a class with a NaN member, or with +inf and -inf together, returns A NaN (payload
 * unspecified).  q[r][c] is a function of row r and the map alone: not of n, the row's position, the entry point, the batch
 * it rode in or the kernel form.  Each member passes through at most d_c = ceil(L_c / 16) + 4 additions, the first exact:
 *   |q_c - sum_{i in c} p_i| <= d_c u / (1 - d_c u) * sum_{i in c} |p_i|,  u = 2^-24.
 * The width of sixteen partials (one DPP row of a gfx950 wave) is frozen: results depend on it.  Results are [n][C]
 * row-major; every element is written, nothing outside is, inputs are never modified.  Nothing is routed here: the batcher,
 * device groups and the JNI shim neither route to nor look at any of these entry points, and every other entry point keeps
 * its bytes.
 *
 * fdnn_pool_create / _free / _width / _classes   the handle (NULL from create: see fdnn_last_error; extends CalculateOutput,
 *   dnn.cc:428-454).
 * fdnn_pool_rows_device       the pooling alone on any device-resident [n][width] fp32 rows of the pool's device (rows 4-byte
 *   aligned; extends CalculateOutput, dnn.cc:428-454).  Enqueued on `stream`, not synchronised; n == 0 is a no-op;
 *   FDNN_E_ARG for null pointers or width != the pool's.
 * fdnn_ctx_output_pool        fdnn_ctx_output's computation (CalculateOutput, dnn.cc:428-454) into the context's own rows,
 *   then the pooling; host buffer, host-synchronous.  FDNN_E_STATE before the hidden layers.  Works unchanged on
 *   fdnn_stream_ctx(s) after a hidden-only push.
 * fdnn_ctx_output_pool_device the same with a device buffer, enqueued on `stream`, ordered on the context like the other
 *   *_device entries (CalculateOutput, dnn.cc:428-454).
 * fdnn_calculate_pool         host to host on a pooled context, chunk by chunk like fdnn_calculate (Calculate,
 *   dnn.cc:162-165): only n x C x 4 bytes cross PCIe.  Obeys the re-run rules of the dense host forms.
 * fdnn_calculate_pool_raw     the same from raw feature frames, like fdnn_calculate_raw (Calculate, dnn.cc:162-165).
 * fdnn_calculate_pool_device  device buffers (d_x 16-byte aligned like its siblings, d_out element-aligned), a pooled context
 *   for the intermediate rows; enqueued, not synchronised (Calculate, dnn.cc:162-165). */
typedef struct fdnn_pool fdnn_pool;
FDNN_API fdnn_pool *fdnn_pool_create(const int32_t *class_of, int width, int n_classes);
FDNN_API void fdnn_pool_free(fdnn_pool *pool);
FDNN_API int fdnn_pool_width(const fdnn_pool *pool);
FDNN_API int fdnn_pool_classes(const fdnn_pool *pool);
FDNN_API int fdnn_pool_rows_device(const fdnn_pool *pool, const float *d_rows, int n, float *d_out, void *stream);
FDNN_API int fdnn_ctx_output_pool(fdnn_ctx *c, const fdnn_pool *pool, float *out);
FDNN_API int fdnn_ctx_output_pool_device(fdnn_ctx *c, const fdnn_pool *pool, float *d_out, void *stream);
FDNN_API int fdnn_calculate_pool(fdnn_model *m, const float *x, int n, int dim, const fdnn_pool *pool, float *out);
FDNN_API int fdnn_calculate_pool_raw(fdnn_model *m, const float *raw, int n, int raw_dim, const fdnn_pool *pool, float *out);
FDNN_API int fdnn_calculate_pool_device(fdnn_model *m, const float *d_x, int n, const fdnn_pool *pool, float *d_out, void *stream);
/* ------------------------------------------------------------------ dense output as decoder scores (fdnn_loglik.hip)
 * What a hybrid decoder consumes is not the posterior but the scaled log-likelihood ln p(s|x) - ln p(s).  These entries
 * compute it on the DEVICE from the dense soft-max and return the whole row, as fp32 or -- scores fit fp16 where
 * probabilities do not: a posterior of 1e-9 is 0 in fp16, its logarithm -20.7 an ordinary number -- as fp16, half the bytes
 * of fdnn_calculate.  The reference has no such call; every entry below extends CalculateOutput (dnn.cc:428-454).
 *
 * The handle: fdnn_loglik_create(log_prior [W], W, floor, type).  Every log_prior[i] is finite; 1 <= W <= 2^19; floor is not
 * a NaN and not +inf, -inf means no floor; type is FDNN_LOGLIK_F32 or FDNN_LOGLIK_F16; an F16 handle with a finite floor
 * below -65504 is refused.  The priors are uploaded to the device that is CURRENT at creation.  A handle is immutable;
 * threads, contexts and scoring loops may share it; it must outlive every call and every ticket that uses it.  A call whose
 * handle width differs from the model's output_dim, whose handle lives on another device than the model, or whose model
 * leads a device group is FDNN_E_ARG before anything is launched.
 *
 * The score of a row p[0 .. W):
 *   s_i = ln(p_i) - log_prior[i]          one fp32 subtraction, round to nearest even
 *   s_i = (s_i < floor) ? floor : s_i     a NaN stays a NaN
 *   F16: the RN-even conversion of s_i    |s_i| >= 65520 becomes +-inf; fp16 denormals are kept
 * ln is neither the hardware's nor the C library's logarithm but ONE fixed sequence of fp32 operations (fdnn_loglik.hpp:
 * fmaf, single multiplications, additions and subtractions, integer operations; the Cephes scheme), the same bits on the
 * host and on the device: NaN -> a NaN; any negative value, negative denormals included -> a NaN; +0 and -0 -> -inf;
 * +inf -> +inf; denormals are not flushed.  Over ALL positive finite floats its worst error against float64 log is 0.8265
 * ulp (bound kLnMaxUlp = 0.85), it is monotone, and ln(1) = +0 (tools/ln_sweep.cpp, profiles/ln_sweep.log).  It differs
 * from the correctly rounded logarithm in 0.6 % of the floats in (0, 1]: compare with fdnn_debug_loglik_ref, not with a
 * library's log.  s is a function of the row and the handle alone: not of n, the row's position, the entry point, the batch
 * or the kernel form.  With a finite floor no -inf leaves the device.  FROZEN: results depend on the sequence.
 * NOTE: the k best probabilities are NOT the k best scores -- subtracting the priors reorders the nodes; a top-k result
 * turned into scores (fdnn_loglik_entries_device) holds the scores of the k most PROBABLE nodes.
 * Results are [n][W] row-major of float (F32) or IEEE binary16 (F16); every element is written, nothing outside is, inputs
 * are never modified.  The batcher, device groups and the JNI shim neither route to nor look at these entry points, and every
 * other entry point keeps its bytes.
 *
 * fdnn_loglik_create / _free / _width / _type   the handle (NULL from create: see fdnn_last_error; dnn.cc:428-454).
 * fdnn_loglik_rows_device     the scores alone of any device-resident [n][W] fp32 rows of the handle's device (rows 4-byte
 *   aligned, d_out aligned to its element; where W % 4 == 0 and both start on a 16-byte boundary a faster form runs, same
 *   bytes; dnn.cc:428-454).  Enqueued on `stream`, not synchronised; n == 0 is a no-op.
 * fdnn_loglik_entries_device  for a flat list (d_nodes[j], d_p[j]), j < count: s_j = ln(p_j) - log_prior[node_j], the same
 *   floor and type; a node outside [0, W) gives a NaN and reads nothing.  Turns the results of the top-k, lists, set and
 *   sets calls into decoder scores on the device (dnn.cc:428-454).
 * fdnn_ctx_output_loglik      fdnn_ctx_output's computation (CalculateOutput, dnn.cc:428-454) into the context's own rows,
 *   then the scores; host buffer, host-synchronous.  FDNN_E_STATE before the hidden layers.  Works unchanged on
 *   fdnn_stream_ctx(s) after a hidden-only push.
 * fdnn_ctx_output_loglik_device  the same with a device buffer, enqueued on `stream` (dnn.cc:428-454).
 * fdnn_calculate_loglik       host to host on a pooled context, chunk by chunk like fdnn_calculate (Calculate,
 *   dnn.cc:162-165; CalculateOutput, dnn.cc:428-454): n x W x 4 or 2 bytes cross PCIe.  Obeys the re-run rules of the dense
 *   host forms.
 * fdnn_calculate_loglik_raw   the same from raw feature frames, like fdnn_calculate_raw (dnn.cc:428-454).
 * fdnn_calculate_loglik_device  device buffers (d_x 16-byte aligned like its siblings, d_out element-aligned), a pooled
 *   context for the intermediate rows; enqueued, not synchronised (dnn.cc:428-454). */
#define FDNN_LOGLIK_F32 0
#define FDNN_LOGLIK_F16 1
typedef struct fdnn_loglik fdnn_loglik;
FDNN_API fdnn_loglik *fdnn_loglik_create(const float *log_prior, int width, float floor, int type);
FDNN_API void fdnn_loglik_free(fdnn_loglik *ll);
FDNN_API int fdnn_loglik_width(const fdnn_loglik *ll);
FDNN_API int fdnn_loglik_type(const fdnn_loglik *ll);
FDNN_API int fdnn_loglik_rows_device(const fdnn_loglik *ll, const float *d_rows, int n, void *d_out, void *stream);
FDNN_API int fdnn_loglik_entries_device(const fdnn_loglik *ll, const int32_t *d_nodes, const float *d_p, long long count, void *d_out, void *stream);
FDNN_API int fdnn_ctx_output_loglik(fdnn_ctx *c, const fdnn_loglik *ll, void *out);
FDNN_API int fdnn_ctx_output_loglik_device(fdnn_ctx *c, const fdnn_loglik *ll, void *d_out, void *stream);
FDNN_API int fdnn_calculate_loglik(fdnn_model *m, const float *x, int n, int dim, const fdnn_loglik *ll, void *out);
FDNN_API int fdnn_calculate_loglik_raw(fdnn_model *m, const float *raw, int n, int raw_dim, const fdnn_loglik *ll, void *out);
FDNN_API int fdnn_calculate_loglik_device(fdnn_model *m, const float *d_x, int n, const fdnn_loglik *ll, void *d_out, void *stream);
/* ------------------------------------------------------------------ forced alignment (fdnn_align.hip)
 * The best monotone path of a transcript's states over an utterance's rows, and its score, on the DEVICE: what the lazy paths
 * for per-utterance node sets were built for.  Instead of rows x len probabilities per utterance, 4 bytes per frame leave
 * the device.  The reference has no such call; every entry below extends LazyOutputActivations (dnn.cc:355-392).
 *
 * A SEGMENT is one utterance: T >= 1 consecutive rows and a transcript states[0 .. S) of output-node numbers, 1 <= S <=
 * 16384, each in [0, output_dim), in any order, repeats allowed.  Optional transition scores self_lp[0 .. S) and
 * next_lp[0 .. S): next_lp[S - 1] is never read, every value that is read is finite, NULL is an array of +0.0f (the same
 * bytes).  The tables of a call are host memory:
 *   seg_rows  [n_segs + 1]  rising strictly; segment s = rows [seg_rows[s], seg_rows[s + 1])
 *   state_ptr [n_segs + 1]  state_ptr[0] == 0; segment s's transcript = states[state_ptr[s] .. state_ptr[s + 1])
 *   states, self_lp, next_lp [state_ptr[n_segs]]
 *   path [seg_rows[n_segs] - seg_rows[0]] int32 in row order, total [n_segs] float
 * The emission of state j in row t is what fdnn_loglik_entries_device returns for (states[j], p), p the lazy-contract
 * probability of that node in that row under the segment's node set -- the transcript's distinct nodes, ascending:
 *   e(t, j) = score(p, log_prior[states[j]], floor); an F16 handle's value is rounded to fp16 and widened exactly.
 * The recursion, in fp32, every + rounded once, nothing contracted (fdnn_align.hpp):
 *   d[0][0] = e(0, 0);   d[0][j] = -inf for j > 0
 *   stay = d[t-1][j] + self_lp[j];   move = d[t-1][j-1] + next_lp[j-1]   (j = 0: -inf)
 *   take = move > stay               (false on a tie and for a NaN on either side: stay)
 *   d[t][j] = (take ? move : stay) + e(t, j);   total = d[T-1][S-1]
 *   path: j = S-1; for t = T-1 .. 1: path[t] = j; if take[t][j]: j -= 1;  path[0] = j
 * Total not finite (-inf: T < S or no path with a finite score; +inf; a NaN): every element of path is -1; a NaN total is
 * 0x7fc00000.  Otherwise path[0] = 0, path[T-1] = S-1 and steps are 0 or 1.  Among paths of equal score the one whose moves
 * come earliest is returned.  Additions and comparisons only: path and total are a function of the scores and the transcript
 * alone -- not of the kernel form, the chunking or the entry point -- and equal fdnn_debug_align_ref byte for byte.
 * FDNN_E_ARG before anything is launched, naming the first bad segment: malformed tables, a node outside [0, output_dim), a
 * transcript without or with more than 16384 states, T < S (host-table forms), a transition score that is read and is not
 * finite, a handle whose width or device is not the model's, a model that leads a device group, back-pointer words of one
 * call above 2^30 bytes.  FDNN_E_STATE before the hidden layers have run.  The batcher, the scoring loop, device groups and
 * the JNI shim neither route to nor look at these entry points, and every other entry point keeps its bytes.
 *
 * fdnn_align_rows_device   the recursion alone on any device-resident fp32 rows (dnn.cc:355-392): segment s has seg_T[s]
 *   rows of stride row_ld[s] elements beginning row_off[s] elements into d_rows (host tables); state j of the call reads
 *   column d_col[j] of its segment's rows.  With ll == NULL the rows are scores already, e(t, j) = rows[t ld + col[j]], and
 *   d_state_node is not read; with a handle they are probabilities and d_state_node[j] names the prior.  A column outside
 *   [0, row_ld) or a node outside [0, W) gives a NaN emission and reads nothing: the total is a NaN (the last state's) or
 *   -inf (the move out of a NaN is never taken), the path -1 everywhere.  T < S is not refused here: -1 everywhere, total -inf.  d_self_lp / d_next_lp may be NULL.  d_scratch: at least the 32-bit words fdnn_align_scratch_words names
 *   for the same tables, on an 8-byte boundary (NULL when 0); its contents mean nothing before or after.  d_path [sum T],
 *   d_total [n_segs].  Enqueued on `stream`, not synchronised.
 * fdnn_align_scratch_words the scratch of that call: the back-pointer words of the segments that do not fit LDS
 *   (dnn.cc:355-392).
 * fdnn_ctx_align           host tables and host results, host-synchronous, over rows of a context whose hidden layers have
 *   run (dnn.cc:355-392): the transcripts' node sets, fdnn_ctx_lazy_output_sets' computation into a context-owned device
 *   buffer, the recursion, then ONE transfer of path and total.  Works unchanged on fdnn_stream_ctx(s) after a hidden-only
 *   push.
 * fdnn_ctx_align_device    the same with device result buffers, enqueued on `stream`; the host tables are read before it
 *   returns (dnn.cc:355-392).
 * fdnn_calculate_align     one call on a pooled context (dnn.cc:355-392): seg_rows must cover [0, n); a large n goes chunk
 *   by chunk (fdnn_debug_frame_chunks) like fdnn_calculate_lazy_sets, a segment cut by a chunk keeps its set, the chunks'
 *   probabilities stay on the device and the recursion runs ONCE behind the last chunk: a cut segment's path is the uncut one.
 * fdnn_calculate_align_raw the same from raw feature frames [n][raw_dim] (dnn.cc:355-392); every segment is an utterance of
 *   its own: its edge rows repeat its own first and last frame. */
FDNN_API int fdnn_align_rows_device(const fdnn_loglik *ll, const float *d_rows, const int32_t *seg_T, const long long *row_off, const int32_t *row_ld,
                                    const int32_t *state_ptr, int n_segs, const int32_t *d_col, const int32_t *d_state_node, const float *d_self_lp,
                                    const float *d_next_lp, void *d_scratch, long long scratch_words, int32_t *d_path, float *d_total, void *stream);
FDNN_API int fdnn_align_scratch_words(const int32_t *seg_T, const int32_t *state_ptr, int n_segs, long long *words);
FDNN_API int fdnn_ctx_align(fdnn_ctx *c, const fdnn_loglik *ll, const int32_t *seg_rows, const int32_t *state_ptr, int n_segs, const int32_t *states,
                            const float *self_lp, const float *next_lp, int32_t *path, float *total);
FDNN_API int fdnn_ctx_align_device(fdnn_ctx *c, const fdnn_loglik *ll, const int32_t *seg_rows, const int32_t *state_ptr, int n_segs,
                                   const int32_t *states, const float *self_lp, const float *next_lp, int32_t *d_path, float *d_total, void *stream);
FDNN_API int fdnn_calculate_align(fdnn_model *m, const float *x, int n, int dim, const fdnn_loglik *ll, const int32_t *seg_rows,
                                  const int32_t *state_ptr, int n_segs, const int32_t *states, const float *self_lp, const float *next_lp,
                                  int32_t *path, float *total);
FDNN_API int fdnn_calculate_align_raw(fdnn_model *m, const float *raw, int n, int raw_dim, const fdnn_loglik *ll, const int32_t *seg_rows,
                                      const int32_t *state_ptr, int n_segs, const int32_t *states, const float *self_lp, const float *next_lp,
                                      int32_t *path, float *total);
/* ------------------------------------------------------------------ alignment graphs (fdnn_align_graph.hip)
 * The best path over ANY arc set of a segment's states, and its score, on the device: optional silence between words,
 * pronunciation variants, absent leading or trailing silence, a keyword looped against a filler -- what the chain above leaves
 * out.  The reference has no such call; every entry below extends LazyOutputActivations (dnn.cc:355-392).  THE CONTRACT IS
 * STATED ONCE, in csrc/fdnn_align_graph.hpp; in short:
 *
 * A segment has T >= 1 rows and a graph of 1 <= S <= 16384 states.  State j has an output node states[j] (repeats are
 * normal) and the incoming arcs arc_ptr[j] .. arc_ptr[j + 1], in the order the caller wrote them; an arc has a source
 * arc_src[a], a state index local to the segment in [0, S) (self-loops, forward, skip and backward arcs alike) and a finite
 * score arc_lp[a].  Every arc consumes a frame.  The tables follow the chain's:
 *   seg_rows [n_segs + 1], state_ptr [n_segs + 1], states [N], N = state_ptr[n_segs]
 *   arc_ptr  [N + 1]   arc_ptr[0] == 0, non-decreasing (a segment's arcs are contiguous); at most 2^17 arcs per segment
 *   arc_src, arc_lp [arc_ptr[N]]
 *   start_lp, final_lp [N] or NULL, each value finite or -inf; NULL start_lp = +0.0f for the segment's state 0 and -inf
 *     elsewhere, NULL final_lp = +0.0f for its state S - 1 and -inf elsewhere
 *   path [seg_rows[n_segs] - seg_rows[0]] int32 in row order, total [n_segs] float
 * The emission e(t, j) is the chain's.  In fp32, every + rounded once, nothing contracted:
 *   d[0][j] = start_lp[j] + e(0, j)
 *   t >= 1: best = -inf, from = -1; for each arc a of j in order: cand = d[t-1][arc_src[a]] + arc_lp[a];
 *           if (cand > best) best = cand, from = arc_src[a];    d[t][j] = best + e(t, j), bp[t][j] = from
 *   total:  the best of d[T-1][j] + final_lp[j] over j ascending, taken only where above the best so far; end = its state
 *   path:   j = end; for t = T-1 .. 1: path[t] = j, j = bp[t][j];  path[0] = j
 * A tie and a NaN are never taken: among equal candidates the EARLIEST arc of a state's list wins, among equal final states
 * the lowest; the total is never a NaN (unlike the chain's).  A total that is not finite (-inf: no path; +inf) gives -1 in
 * every frame.  A state without arcs is reachable at t = 0 only.  With state j's arcs (j with self_lp[j], then j - 1 with
 * next_lp[j - 1]) and NULL start_lp / final_lp the result is fdnn_calculate_align's byte for byte wherever no emission is a
 * NaN or +inf, T < S included.  Path and total are a function of the scores and the graph alone -- not of the kernel form,
 * the chunking or the entry point -- and equal fdnn_debug_align_graph_ref byte for byte.
 * FDNN_E_ARG before anything is launched, naming the first bad segment: the chain's row, state and node reasons (not T < S:
 * a graph may skip), a malformed arc_ptr, more than 2^17 arcs, a source outside [0, S), an arc score that is not finite, a
 * start or final value that is a NaN or +inf, no start or no final state with a finite value, the chain's handle and
 * device-group reasons, back-pointers of one call above 2^30 bytes.  FDNN_E_STATE before the hidden layers have run.  The
 * batcher, the scoring loop, device groups and the JNI shim neither route to nor look at these entry points, and every other
 * entry point keeps its bytes.
 *
 * fdnn_align_graph_rows_device   the recursion alone on any device-resident fp32 rows (dnn.cc:355-392): seg_T, row_off,
 *   row_ld, state_ptr and arc_ptr are host tables (the plan is made from them, and the host arc_ptr bounds every arc index on
 *   the device); d_col, d_state_node [N] as fdnn_align_rows_device; d_arc_ptr [N + 1], d_arc_src, d_arc_lp [arcs] device copies
 *   of the graph; d_start_lp / d_final_lp [N] or NULL.  A source outside [0, S) makes that candidate a NaN and reads nothing;
 *   a column or node out of range makes the emission a NaN.  d_scratch: at least the 32-bit words
 *   fdnn_align_graph_scratch_words names, on a 4-byte boundary (NULL when 0).  d_path [sum T], d_total [n_segs].  Enqueued on
 *   `stream`, not synchronised.
 * fdnn_align_graph_scratch_words the scratch of that call: the back-pointers (16 bits a frame and state) of the segments
 *   whose do not fit LDS (dnn.cc:355-392).
 * fdnn_ctx_align_graph           host tables and host results, host-synchronous, over rows of a context whose hidden layers
 *   have run (dnn.cc:355-392): the graphs' node sets, fdnn_ctx_lazy_output_sets' computation into a context-owned buffer, the
 *   recursion, then ONE transfer of path and total.
 * fdnn_ctx_align_graph_device    the same with device result buffers, enqueued on `stream`; the host tables are read before
 *   it returns (dnn.cc:355-392).
 * fdnn_calculate_align_graph     one call on a pooled context (dnn.cc:355-392): seg_rows must cover [0, n); a large n goes
 *   chunk by chunk like fdnn_calculate_align, and the recursion runs ONCE behind the last chunk: a cut segment's path is the
 *   uncut one.
 * fdnn_calculate_align_graph_raw the same from raw feature frames [n][raw_dim] (dnn.cc:355-392); every segment is an
 *   utterance of its own. */
FDNN_API int fdnn_align_graph_rows_device(const fdnn_loglik *ll, const float *d_rows, const int32_t *seg_T, const long long *row_off,
                                          const int32_t *row_ld, const int32_t *state_ptr, const int32_t *arc_ptr, int n_segs, const int32_t *d_col,
                                          const int32_t *d_state_node, const int32_t *d_arc_ptr, const int32_t *d_arc_src, const float *d_arc_lp,
                                          const float *d_start_lp, const float *d_final_lp, void *d_scratch, long long scratch_words, int32_t *d_path,
                                          float *d_total, void *stream);
FDNN_API int fdnn_align_graph_scratch_words(const int32_t *seg_T, const int32_t *state_ptr, int n_segs, long long *words);
FDNN_API int fdnn_ctx_align_graph(fdnn_ctx *c, const fdnn_loglik *ll, const int32_t *seg_rows, const int32_t *state_ptr, int n_segs,
                                  const int32_t *states, const int32_t *arc_ptr, const int32_t *arc_src, const float *arc_lp, const float *start_lp,
                                  const float *final_lp, int32_t *path, float *total);
FDNN_API int fdnn_ctx_align_graph_device(fdnn_ctx *c, const fdnn_loglik *ll, const int32_t *seg_rows, const int32_t *state_ptr, int n_segs,
                                         const int32_t *states, const int32_t *arc_ptr, const int32_t *arc_src, const float *arc_lp,
                                         const float *start_lp, const float *final_lp, int32_t *d_path, float *d_total, void *stream);
FDNN_API int fdnn_calculate_align_graph(fdnn_model *m, const float *x, int n, int dim, const fdnn_loglik *ll, const int32_t *seg_rows,
                                        const int32_t *state_ptr, int n_segs, const int32_t *states, const int32_t *arc_ptr, const int32_t *arc_src,
                                        const float *arc_lp, const float *start_lp, const float *final_lp, int32_t *path, float *total);
FDNN_API int fdnn_calculate_align_graph_raw(fdnn_model *m, const float *raw, int n, int raw_dim, const fdnn_loglik *ll, const int32_t *seg_rows,
                                            const int32_t *state_ptr, int n_segs, const int32_t *states, const int32_t *arc_ptr,
                                            const int32_t *arc_src, const float *arc_lp, const float *start_lp, const float *final_lp, int32_t *path,
                                            float *total);
/* ------------------------------------------------------------------ alignment graphs, summed (fdnn_fb.hip)
 * The likelihood of a segment's WHOLE graph, ln of the sum over its paths, and the state occupancies gamma[t][j], the
 * posterior of being in state j at frame t, on the device: a keyword graph against a filler graph, an utterance's
 * confidence, a choice between transcripts, soft boundaries, statistics over soft alignments.  The reference has no such
 * call; every entry below extends LazyOutputActivations (dnn.cc:355-392).  THE CONTRACT IS STATED ONCE, in csrc/fdnn_fb.hpp;
 * in short:
 *
 * The inputs are the alignment graphs' above, checked by the same validator.  In fp32, every + and - rounded once, nothing
 * contracted, with two stated functions -- exp_neg(x), exp on (-inf, 0] by one fixed sequence of operations (a NaN and
 * x < -87 give +0, no result is a denormal), and ladd(a, b) = hi + ln(1 + exp_neg(lo - hi)) with the frozen logarithm of the
 * decoder scores (lo == -inf gives hi, hi == +inf gives +inf) --:
 *   alpha[0][j] = start_lp[j] + e(0, j)
 *   t >= 1: acc = -inf; for each arc a of j in order: cand = alpha[t-1][arc_src[a]] + arc_lp[a]; a NaN is never added;
 *           acc = ladd(acc, cand);   alpha[t][j] = acc + e(t, j)
 *   total:  the terms alpha[T-1][j] + final_lp[j], a NaN skipped, state j dealt to partial j mod 256 and added there in
 *           ascending j, then the tree step = 128 .. 1: partial[i] = ladd(partial[i], partial[i + step]); total = partial[0]
 *   bb:     the same recursion on the transposed graph in reversed time from final_lp (fdnn_fb_transpose: a stable counting
 *           sort of a segment's arcs by source), bb[t][i] including i's own emission
 *   gamma[t][j] = exp_neg(min(0, ((alpha[t][j] + bb[t][j]) - e(t, j)) - total)), row-major [t][j] per segment, segment s at
 *           the sum of T S over the segments before it
 *   total [n_segs] float, gamma [sum of T S] float or NULL
 * The total is never a NaN; -inf means no path; a total that is not finite gives gamma = +0 everywhere.  gamma == NULL means
 * forward only: no transposed tables, no backward launch, no lattice, four bytes per segment leave the device.  On any
 * input total >= fdnn_debug_align_graph_ref's best-path total, and on a graph with exactly one path of finite score the two
 * are equal as bits.  The order of a state's arcs is part of the input.  Total and gamma are a function of the scores and
 * the graph alone -- not of the kernel form, the chunking or the entry point -- and equal fdnn_debug_fb_ref byte for byte.
 * FDNN_E_ARG before anything is launched: the alignment graphs' reasons, and a lattice (4 bytes a frame and state, only
 * where gamma is asked) above 2^30 bytes.  FDNN_E_STATE before the hidden layers have run.  The batcher, the scoring loop,
 * device groups and the JNI shim neither route to nor look at these entry points, and every other entry point keeps its
 * bytes.
 *
 * fdnn_fb_rows_device     the sweeps alone on any device-resident fp32 rows (dnn.cc:355-392): seg_T, row_off, row_ld,
 *   state_ptr, arc_ptr and t_ptr are host tables (the plan is made from them; the host arc_ptr / t_ptr bound every arc index
 *   on the device); d_col, d_state_node, the device copies of the graph and d_start_lp / d_final_lp as
 *   fdnn_align_graph_rows_device; d_t_ptr [N + 1], d_t_src, d_t_lp [arcs] device copies of the transposed tables.  A source or
 *   destination outside [0, S) makes that candidate a NaN and reads nothing.  d_gamma may be NULL: t_ptr and the d_t_ tables
 *   are then not read and no scratch is needed.  d_scratch: at least the fp32 words fdnn_fb_scratch_words names (NULL when
 *   0).  d_total [n_segs], d_gamma [sum T S].  Enqueued on `stream`, not synchronised.
 * fdnn_fb_scratch_words   the scratch of that call: T S words a segment where gamma is wanted, else 0 (dnn.cc:355-392);
 *   above 2^30 bytes FDNN_E_ARG.
 * fdnn_fb_transpose       host code: t_ptr [N + 1], t_src [arcs] (the DESTINATION, local to the segment), t_lp [arcs] from a
 *   call's arc tables (dnn.cc:355-392); FDNN_E_ARG for a source outside [0, S).  The one definition of the backward order.
 * fdnn_ctx_fb             host tables and host results, host-synchronous, over rows of a context whose hidden layers have run
 *   (dnn.cc:355-392): the graphs' node sets into a context-owned buffer, the sweeps, then one transfer of total and one of
 *   gamma where it is not NULL.
 * fdnn_ctx_fb_device      the same with device result buffers, enqueued on `stream`; the host tables are read before it
 *   returns (dnn.cc:355-392).
 * fdnn_calculate_fb       one call on a pooled context (dnn.cc:355-392): seg_rows must cover [0, n); a large n goes chunk by
 *   chunk, and the sweeps run ONCE behind the last chunk: a cut segment's results are the uncut ones.
 * fdnn_calculate_fb_raw   the same from raw feature frames [n][raw_dim] (dnn.cc:355-392); every segment is an utterance of
 *   its own. */
FDNN_API int fdnn_fb_rows_device(const fdnn_loglik *ll, const float *d_rows, const int32_t *seg_T, const long long *row_off, const int32_t *row_ld,
                                 const int32_t *state_ptr, const int32_t *arc_ptr, const int32_t *t_ptr, int n_segs, const int32_t *d_col,
                                 const int32_t *d_state_node, const int32_t *d_arc_ptr, const int32_t *d_arc_src, const float *d_arc_lp,
                                 const float *d_start_lp, const float *d_final_lp, const int32_t *d_t_ptr, const int32_t *d_t_src, const float *d_t_lp,
                                 void *d_scratch, long long scratch_words, float *d_total, float *d_gamma, void *stream);
FDNN_API int fdnn_fb_scratch_words(const int32_t *seg_T, const int32_t *state_ptr, int n_segs, int want_gamma, long long *words);
FDNN_API int fdnn_fb_transpose(const int32_t *state_ptr, int n_segs, const int32_t *arc_ptr, const int32_t *arc_src, const float *arc_lp,
                               int32_t *t_ptr, int32_t *t_src, float *t_lp);
FDNN_API int fdnn_ctx_fb(fdnn_ctx *c, const fdnn_loglik *ll, const int32_t *seg_rows, const int32_t *state_ptr, int n_segs, const int32_t *states,
                         const int32_t *arc_ptr, const int32_t *arc_src, const float *arc_lp, const float *start_lp, const float *final_lp,
                         float *total, float *gamma);
FDNN_API int fdnn_ctx_fb_device(fdnn_ctx *c, const fdnn_loglik *ll, const int32_t *seg_rows, const int32_t *state_ptr, int n_segs,
                                const int32_t *states, const int32_t *arc_ptr, const int32_t *arc_src, const float *arc_lp, const float *start_lp,
                                const float *final_lp, float *d_total, float *d_gamma, void *stream);
FDNN_API int fdnn_calculate_fb(fdnn_model *m, const float *x, int n, int dim, const fdnn_loglik *ll, const int32_t *seg_rows, const int32_t *state_ptr,
                               int n_segs, const int32_t *states, const int32_t *arc_ptr, const int32_t *arc_src, const float *arc_lp,
                               const float *start_lp, const float *final_lp, float *total, float *gamma);
FDNN_API int fdnn_calculate_fb_raw(fdnn_model *m, const float *raw, int n, int raw_dim, const fdnn_loglik *ll, const int32_t *seg_rows,
                                   const int32_t *state_ptr, int n_segs, const int32_t *states, const int32_t *arc_ptr, const int32_t *arc_src,
                                   const float *arc_lp, const float *start_lp, const float *final_lp, float *total, float *gamma);
/* Last hidden layer's u8 activations, n x hidden_dim (quantized_activations_). */
FDNN_API int fdnn_ctx_read_hidden(fdnn_ctx *c, uint8_t *out);

/* ------------------------------------------------------------------ multi-stream scoring loop
 * Generalises the reference's serving shape -- caller threads over independent
 * utterances, one context per call (QuantizedDnn.java:72-107,
 * MultiThreadedStressTest.java:48-69) -- to batches in flight on one GPU.
 * A server owns `depth` slots (a context sized for max_frames each) and two
 * shared streams: consecutive large batches are serialised on the compute
 * stream while the HBM-bound soft-max scale of batch i runs on the tail stream
 * under the VALU-bound layer 0 of batch i+1; batches too small to fill the chip
 * run whole on their slot's stream, next to each other.  A submission returns a
 * ticket; fdnn_server_wait(ticket) returns when its results are complete.
 * At most `depth` device submissions are in flight: a further submit first
 * waits for the oldest.  All entry points are thread-safe.
 *
 *   fdnn_server_submit_device  d_x [n][input_dim] and d_out [n][output_dim] live
 *     on the model's device and must stay valid until the ticket completes;
 *     d_masks (may be NULL) [n][output_dim] selects the lazy contract
 *     (dnn.cc:355-392).  n <= max_frames.
 *   fdnn_server_submit         host buffers, any n >= 1.  Submissions from any
 *     number of threads are coalesced: packed into one batch of up to
 *     max_frames frames per slot, scored once, scattered back to each caller's
 *     `out`.  x / masks / out must stay valid until the ticket completes.  A
 *     coalesced utterance is bit-identical to the same utterance scored alone
 *     (frames are independent, kernels are batch-size invariant).
 *   fdnn_server_set_linger_us  how long the packer waits for more host
 *     submissions before launching a batch that is not full (default 0); it
 *     never lingers while the server is idle (no batch in flight).
 *   fdnn_model_enable_batcher  routes fdnn_calculate (= the JNI calculate()) of
 *     this model through an internal server, so that the unmodified Java class
 *     called from many threads is coalesced as well; also switched on at load by
 *     the environment variable FDNN_BATCHER=max_frames[:depth[:linger_us]]. */
typedef struct fdnn_server fdnn_server;
FDNN_API int fdnn_server_create(fdnn_model *m, int max_frames, int depth, fdnn_server **out);
FDNN_API void fdnn_server_free(fdnn_server *s);
FDNN_API int fdnn_server_set_linger_us(fdnn_server *s, int microseconds);
FDNN_API int fdnn_server_submit_device(fdnn_server *s, const float *d_x, int n, const int8_t *d_masks, float *d_out,
                                       uint64_t *ticket);
FDNN_API int fdnn_server_submit(fdnn_server *s, const float *x, int n, const int8_t *masks, float *out, uint64_t *ticket);
/* The lazy contract through the loop with the masks as BITS (bits [n][ceil(output_dim / 64)], bit b of word w = node
 * 64 w + b, as fdnn_calculate_lazy_bits): bit-mask submissions are coalesced with one another, scored once, and come back
 * COMPACTED -- the active nodes' probabilities and one value per frame over PCIe, each caller's rows rebuilt inside its
 * own `out` by the thread that waits for the ticket.  x / bits / out must stay valid until the ticket completes.
 * (LazyContext.calculateUntilOutput + calculateForOutputNodes per frame, QuantizedDnn.java:72-107, for many callers.) */
FDNN_API int fdnn_server_submit_lazy_bits(fdnn_server *s, const float *x, int n, const uint64_t *bits, float *out, uint64_t *ticket);
/* Raw feature frames through the loop (see "raw feature frames" above): raw [n][D]; bits NULL = dense rows, else the
 * compacted lazy return of fdnn_server_submit_lazy_bits.  Raw utterances are coalesced with one another, each keeping its
 * own edges (the batch's segment table); only the raw frames travel.  Bit-identical to the same utterance through
 * fdnn_calculate_raw / fdnn_calculate_lazy_bits_raw.  raw / bits / out must stay valid until the ticket completes.  A
 * submission is spliced by the model's spec at the time it was submitted. */
FDNN_API int fdnn_server_submit_raw(fdnn_server *s, const float *raw, int n, const uint64_t *bits, float *out, uint64_t *ticket);
/* One utterance with ITS OWN node set through the loop (the set contract of fdnn_ctx_lazy_output_set; LazyOutputActivations,
 * dnn.cc:355-392, for many callers): set submissions are coalesced with one another, the hidden layers run once for the
 * batch, and the pieces' sets are scored as the segments of one fdnn_ctx_lazy_output_sets-style call -- the dense output layer
 * does not run at all, and only probs [n][len] and inactive [n] cross PCIe (32 KB for 100 frames x 80 nodes, against 3.2 MB
 * of dense rows).  The results are byte-identical to fdnn_calculate_lazy_set on the same utterance.  The set is validated
 * at submit (FDNN_E_ARG) and COPIED: the caller may release `nodes` at once; x or raw, probs and inactive must stay valid
 * until the ticket completes.  len == 0: every row's inactive value is 1 / output_dim, probs is not written.
 * fdnn_server_submit_raw_set takes raw feature frames [n][D], spliced on the device by the model's spec at submit time. */
FDNN_API int fdnn_server_submit_lazy_set(fdnn_server *s, const float *x, int n, const int32_t *nodes, int len, float *probs,
                                         float *inactive, uint64_t *ticket);
FDNN_API int fdnn_server_submit_raw_set(fdnn_server *s, const float *raw, int n, const int32_t *nodes, int len, float *probs,
                                        float *inactive, uint64_t *ticket);
/* One utterance's k best nodes per frame through the loop (the top-k contract above; CalculateOutput, dnn.cc:428-454, for
 * many callers): top-k submissions are coalesced with one another (same rawness and spec), the batch runs as a dense batch,
 * ONE selection launch with the largest k among its pieces runs over the rows -- which never leave the device --, one
 * transfer brings the pairs to the host, and each caller gets the first k columns of its rows (the prefix property).
 * Byte-identical to fdnn_calculate_topk / fdnn_calculate_topk_raw on the same utterance.  x or raw, nodes [n][k] and probs
 * [n][k] must stay valid until the ticket completes.  fdnn_server_submit_raw_topk takes raw feature frames [n][D], spliced
 * on the device by the model's spec at submit time. */
FDNN_API int fdnn_server_submit_topk(fdnn_server *s, const float *x, int n, int k, int32_t *nodes, float *probs, uint64_t *ticket);
FDNN_API int fdnn_server_submit_raw_topk(fdnn_server *s, const float *raw, int n, int k, int32_t *nodes, float *probs, uint64_t *ticket);
/* One utterance's class posteriors through the loop (the pool contract above; CalculateOutput, dnn.cc:428-454, for many
 * callers): pool submissions share a batch only with pool submissions of the SAME handle, the same rawness and the same
 * spec; the batch runs as a dense batch, ONE pooling launch runs over the rows -- which never leave the device --, one
 * transfer brings [rows][C] to the host, and each caller gets its rows.  Byte-identical to fdnn_calculate_pool /
 * fdnn_calculate_pool_raw on the same utterance.  x or raw, out [n][C] and the handle must stay valid until the ticket
 * completes.  fdnn_server_submit_raw_pool takes raw feature frames [n][D], spliced on the device by the model's spec at
 * submit time. */
FDNN_API int fdnn_server_submit_pool(fdnn_server *s, const float *x, int n, const fdnn_pool *pool, float *out, uint64_t *ticket);
FDNN_API int fdnn_server_submit_raw_pool(fdnn_server *s, const float *raw, int n, const fdnn_pool *pool, float *out, uint64_t *ticket);
/* One utterance's decoder scores through the loop (the loglik contract above; CalculateOutput, dnn.cc:428-454, for many
 * callers): loglik submissions share a batch only with loglik submissions of the SAME handle, the same rawness and the same
 * spec; the batch runs as a dense batch, ONE score launch runs over the rows -- which never leave the device --, one transfer
 * brings [rows][output_dim] scores of the handle's type to the host (half the dense batch's bytes for F16), and each caller
 * gets its rows.  Byte-identical to fdnn_calculate_loglik / fdnn_calculate_loglik_raw on the same utterance.  x or raw, out
 * [n][output_dim] and the handle must stay valid until the ticket completes. */
FDNN_API int fdnn_server_submit_loglik(fdnn_server *s, const float *x, int n, const fdnn_loglik *ll, void *out, uint64_t *ticket);
FDNN_API int fdnn_server_submit_raw_loglik(fdnn_server *s, const float *raw, int n, const fdnn_loglik *ll, void *out, uint64_t *ticket);
/* Live utterances through the loop: many utterances arriving at once, each chunk by chunk (SURVEY 8(f) row 3 as a real-time
 * recogniser meets it; see "Streams" above for one utterance on its own).  A live handle is the stream object of ONE
 * utterance at a time; its pushes are scored by the loop, in batches shared with the other handles' pushes and with whole
 * raw utterances (fdnn_server_submit_raw*) of the same spec, same kind of return and, for pool, same handle.  Over an
 * utterance's pushes the rows are byte for byte those of fdnn_calculate_raw / fdnn_calculate_topk_raw /
 * fdnn_calculate_pool_raw on the whole utterance, and for sets those of fdnn_calculate_lazy_set on the host-spliced rows,
 * whatever the chunking and whatever else shared the batches.
 * fdnn_server_live_open      max_chunk: the most raw frames one push may carry.  The handle keeps the model's spec of this
 *   moment (FDNN_E_STATE when the model has none), as fdnn_stream_create does, and the last max(-o, 0) + max(o, 0) raw frames
 *   on the HOST: a push re-stages them, 156 B per frame of 39 floats.
 * fdnn_server_live_close     frees the handle.  Never waits: queued pushes own their frames, their tickets stay valid.  Close
 *   every handle before fdnn_server_free.
 * fdnn_server_live_reset     the next push starts a new utterance (also after a push with `end`, which closes the utterance:
 *   a further push without a reset is FDNN_E_STATE).  Never waits either.
 * fdnn_server_live_position  raw frames pushed and rows emitted since the utterance started.
 * fdnn_server_live_push      n_raw (0 .. max_chunk) raw frames [n_raw][D].  Returns AT ONCE: *n_out is the number of rows this
 *   push completes -- row t is complete once frame t + max(o, 0) has arrived; end != 0 flushes the rest, right-clamped to the
 *   last frame (n_raw = 0 is a flush only) --, known when the call returns, and the rows themselves are in out
 *   [*n_out][output_dim] once fdnn_server_wait(*ticket) has returned.  out must hold n_raw + max(o, 0) rows and stay valid
 *   until then; `raw` is COPIED by the push, the caller may overwrite it at once (a feed's ring buffer does).  A push that
 *   completes no rows queues nothing and sets *ticket = 0: there is then nothing to wait for (fdnn_server_wait refuses
 *   ticket 0).  The buffers are checked all the same.
 * fdnn_server_live_push_topk / _pool / _set   the same push with the return of fdnn_server_submit_raw_topk (nodes and probs
 *   [*n_out][k]), fdnn_server_submit_raw_pool (out [*n_out][C]: the silence posterior out of a class map, for end-pointing)
 *   and fdnn_server_submit_raw_set (probs [*n_out][len], inactive [*n_out]: one keyword's nodes; the set is copied), with
 *   those entries' argument checks.  There is no bit-mask form: a recogniser does not have the masks of frames it has not
 *   decoded.
 * One handle is used by one thread at a time, like a context; different handles from any threads. */
typedef struct fdnn_live fdnn_live;
FDNN_API int fdnn_server_live_open(fdnn_server *s, int max_chunk, fdnn_live **out);
FDNN_API void fdnn_server_live_close(fdnn_live *l);
FDNN_API int fdnn_server_live_reset(fdnn_live *l);
FDNN_API int fdnn_server_live_position(const fdnn_live *l, int64_t *pushed, int64_t *emitted);
FDNN_API int fdnn_server_live_push(fdnn_live *l, const float *raw, int n_raw, int end, float *out, int *n_out, uint64_t *ticket);
FDNN_API int fdnn_server_live_push_topk(fdnn_live *l, const float *raw, int n_raw, int end, int k, int32_t *nodes, float *probs, int *n_out,
                                        uint64_t *ticket);
FDNN_API int fdnn_server_live_push_pool(fdnn_live *l, const float *raw, int n_raw, int end, const fdnn_pool *pool, float *out, int *n_out,
                                        uint64_t *ticket);
FDNN_API int fdnn_server_live_push_set(fdnn_live *l, const float *raw, int n_raw, int end, const int32_t *nodes, int len, float *probs,
                                       float *inactive, int *n_out, uint64_t *ticket);
/* The same push with the return of fdnn_server_submit_raw_loglik: out [*n_out][output_dim] decoder scores of the handle's
 * type (CalculateOutput, dnn.cc:428-454). */
FDNN_API int fdnn_server_live_push_loglik(fdnn_live *l, const float *raw, int n_raw, int end, const fdnn_loglik *ll, void *out, int *n_out,
                                          uint64_t *ticket);
FDNN_API int fdnn_server_wait(fdnn_server *s, uint64_t ticket);
FDNN_API int fdnn_server_drain(fdnn_server *s);
FDNN_API int fdnn_server_stats(fdnn_server *s, uint64_t *batches, uint64_t *frames, uint64_t *requests,
                               uint64_t *coalesced_requests);
FDNN_API int fdnn_model_enable_batcher(fdnn_model *m, int max_frames, int depth, int linger_us);

/* ------------------------------------------------------------------ one process, N devices of one node
 * BASELINE north_star: frames shard across the node's GPUs, weights broadcast at
 * load only.  fdnn_group_load quantizes on devices[0] and sends the packed blob
 * device-to-device to every other listed device (hipMemcpyPeer over xGMI, or one
 * ncclBroadcast when FDNN_GROUP_BCAST=rccl); fdnn_group_calculate cuts the n
 * frames of ONE call (host buffers, as fdnn_calculate / jni_dnn.cc:35-62) into
 * contiguous shards -- fdnn_group_shard, sizes differ by at most one -- scores
 * them concurrently, one host thread per device, each into its slice of `out`.
 * No collective in steady state.  A device may be listed more than once (two
 * replicas on one GPU: how the protocol is tested on a one-GPU box).
 * fdnn_group_attach makes the group transparent: fdnn_calculate on
 * fdnn_group_model(g, 0) shards over the group and fdnn_model_free on it frees
 * the whole group -- which is what fdnn_model_load does by itself when the
 * environment variable FDNN_DEVICES lists several devices ("0,1,2,3" / "all"),
 * so the unmodified Java class scales with no code change. */
typedef struct fdnn_group fdnn_group;
FDNN_API int fdnn_group_load(const char *path, float cutoff, const int *devices, int n_devices, fdnn_group **out);
FDNN_API void fdnn_group_free(fdnn_group *g);
FDNN_API int fdnn_group_size(const fdnn_group *g);
FDNN_API fdnn_model *fdnn_group_model(const fdnn_group *g, int index);
FDNN_API const char *fdnn_group_weight_transport(const fdnn_group *g); /* "none" | "peer-copy" | "rccl" */
/* CPU list the persistent host thread of replica `index` pinned itself to (its device's NUMA-local CPUs), "" before the
 * first large call or when the list could not be read.  Diagnostics. */
FDNN_API const char *fdnn_group_worker_cpus(fdnn_group *g, int index);
FDNN_API int fdnn_group_calculate(fdnn_group *g, const float *x, int n, int dim, int batch_hint, float *out);
FDNN_API void fdnn_group_shard(int n, int world, int rank, int *start, int *stop);
FDNN_API int fdnn_group_attach(fdnn_group *g);

/* ------------------------------------------------------------------ multi-GPU weight distribution
 * Rank 0 quantizes once; the packed blob (header + fp32 layer 0 + int8 layers +
 * per-node offsets + biases + shift/scale + LUT) is broadcast over RCCL by the
 * caller and imported on every other device, so all ranks hold bit-identical
 * weights.  No reference counterpart (the reference is single-process). */
FDNN_API int fdnn_model_blob_size(const fdnn_model *m, size_t *bytes);
FDNN_API int fdnn_model_export_blob(const fdnn_model *m, void *d_dst, size_t capacity, void *stream);
FDNN_API int fdnn_model_import_blob(const void *d_src, size_t bytes, int device, fdnn_model **out);

/* ------------------------------------------------------------------ parity taps (same kernels, extra stores)
 * Runs the dense path on host buffers and also returns intermediate state;
 * any output pointer may be NULL.
 *   l0_lin   [n][H]              layer-0 activation after bias (fp32)
 *   u8_acts  [n_hidden][n][H]    u8 activations after every hidden layer
 *   acc_hid  [n_hidden-1][n][H]  int32 accumulators of the int8 hidden layers
 *                                (pmaddubsw-saturating semantics, dnn.cc:323-349)
 *   acc_out  [n][O]              same for the output layer
 *   logits   [n][O]              output value after bias, before soft-max
 *   probs    [n][O]
 * masks (may be NULL) switches the output layer to the lazy contract. */
FDNN_API int fdnn_debug_forward_taps(fdnn_model *m, const float *x, int n, const int8_t *masks, float *l0_lin,
                                     uint8_t *u8_acts, int32_t *acc_hid, int32_t *acc_out, float *logits, float *probs);

/* The int32 accumulators of the output layer as the PRODUCTION kernel instances hold them (no tap kernels anywhere on
 * the path: the dense / masked instance a plain call of the same size launches), for every stride-th frame:
 * acc [ceil(n/stride)][O].  probs (may be NULL) receives the call's ordinary result [n][O].  Parity tests only. */
FDNN_API int fdnn_debug_production_acc_out(fdnn_model *m, const float *x, int n, int stride, const int8_t *masks, int32_t *acc,
                                           float *probs);

/* How a pass over n frames is cut into chunks (host logic only, no device needed): chunks[2 i] = first frame,
 * chunks[2 i + 1] = frame count of chunk i; returns the number of chunks, or -1 if `cap` pairs do not hold them.  The
 * reference blocks a call by `batch` frames (dnn.cc:402-454: blocking never changes a result); here a very large batch
 * runs as device-sized chunks for cache locality, results unchanged (tests / diagnostics). */
FDNN_API int fdnn_debug_frame_chunks(int n, int *chunks, int cap);
/* The same for a batch whose hidden layers run (chained != 0) or do not run as one chained launch: without the chain a few
 * frames past a whole round of workgroups (up to 2 048) go as a batch of their own (host logic; fdnn_debug_set_chain(0),
 * FDNN_CHAIN=0, fewer than two int8 hidden layers, a layer without the validated division are such configurations). */
FDNN_API int fdnn_debug_frame_chunks_for(int n, int chained, int *chunks, int cap);

/* Which kernel computes the canonical fp32 input layer (tests / measurements only; results are
 * bit-identical): 0 = by batch size (default), 1 = always the chain-pass kernel (128 x 128
 * tiles over chain-major images), 2 = always the 64 x 64-tile kernel, 3 = the screened matrix-pipe path wherever it is
 * available (batches of 2048 frames and more, no taps). */
FDNN_API int fdnn_debug_set_l0_kernel(fdnn_model *m, int kind);

/* Tests only, process-wide: 0 = large batches scale their soft-max in a separate pass (what FDNN_FUSE_NORM=0 or a second
 * process on the GPU selects), 1 = inside the output kernel wherever the shape allows, -1 = the default rule.  Results are
 * bit-identical (one tree order for the row total everywhere).  SoftMax::apply, dnn.cc:534-544. */
FDNN_API int fdnn_debug_set_fuse(int mode);

/* Tests only, host code, no device needed: the host half of a compacted lazy return (what fdnn_calculate_lazy_bits and
 * the scoring loop run on the caller's thread).  comp [count][stride] = per row its inactive value, then its active nodes'
 * values in node order; bits [count][ceil(O / 64)]; out [count][O].  mode 0: the library's choice (AVX-512 expanding loads
 * where the CPU has them), 1: the scalar form, 2: comp copied into the tail of out first (the in-place form of the
 * one-call entry).  LazyOutputActivations' row layout, dnn.cc:366-369, :389. */
FDNN_API int fdnn_debug_lazy_expand(float *out, const float *comp, int count, int O, int stride, const uint64_t *bits, int mode);

/* Tests only: cap the per-launch list of flagged layer-0 outputs (int8 screening) of contexts created AFTER the call at
 * `cap` entries (0 = the default, 1/16 of the outputs), so that a small batch overflows it: tiles that no longer fit take
 * the whole-tile recomputation, results unchanged.  Drops the model's pooled contexts.  InputActivations, dnn.cc:219-247. */
FDNN_API int fdnn_debug_set_l0_list_cap(fdnn_model *m, int cap);

/* How the int8 hidden layers run (tests / measurements only; results are bit-identical): mode 1 = as ONE persistent
 * launch (fdnn_chain.hip: tasks drawn from per-XCD queues, a task waits only for its own frame tile's node tiles of the
 * layer before) for batches of at least min_frames frames (<= 0: the default threshold), 0 = one launch per layer,
 * -1 = the default (FDNN_CHAIN / FDNN_CHAIN_MIN in the environment, else on).  Process-wide.
 * CalculateUntilLastHiddenLayer's layer loop, src/cpp/dnn.cc:413-423, is what is being computed. */
FDNN_API int fdnn_debug_set_chain(int mode, int min_frames);

/* How a large batch's int8 hidden layers run when they are launched layer by layer: 1 = the role-split kernel (fdnn_pp.hip:
 * one wave of each SIMD in the k-loop, its partner staging that tile's operands and running the previous tile's epilogue)
 * for batches of at least min_frames frames (<= 0: the default threshold), 0 = fdnn_gemm.hip's in-phase tiles, -1 = the
 * default (FDNN_PP / FDNN_PP_MIN in the environment, else: layers without saturating pairs from 16 384 frames).  Process-wide; identical bytes either way.
 * QuantizedLayerActivations + AddBias + QuantizedSigmoid, src/cpp/dnn.cc:250-349, is what is being computed. */
FDNN_API int fdnn_debug_set_pp(int mode, int min_frames);

/* How the OUTPUT layer of a large dense batch runs when its soft-max is fused: 1 = the role-split kernel (fdnn_ppo.hip: the
 * exchange of the 256-node row sums and the scale run beside the next half's k-loop) whenever the shape allows (8 000-node
 * class layer: 32 node tiles, 2 048 inputs, dense, validated division), 0 = fdnn_gemm.hip's in-phase fused tiles, -1 = the
 * default (FDNN_PPO in the environment, else by batch size: a layer without saturating weight pairs from 14 pairs of 160-frame
 * halves = 4 161 frames, one with pairs from 22 = 6 721, in either case only where the launch's last round of frame pairs is
 * at least 3/4 resp. 4/5 full -- fdnn_select.hpp: ppo_ok).  Process-wide; identical bits either way.
 * CalculateOutput + SoftMax::apply, src/cpp/dnn.cc:428-454, :534-544, is what is being computed. */
FDNN_API int fdnn_debug_set_ppo(int mode);

/* The launch recorder (tests and the tools under tools/): every host launch site of a compute kernel has a stable name for the
 * branch it takes ("gemm.out.ft320.fused_masked", "small.hid.nt64.prod", "chain.ft320.nofix", "l0.fixlist.lpo8", "norm.rows", ...),
 * kept in one static table that can be read with no device present.  fdnn_debug_launch_name_count: entries of the table;
 * fdnn_debug_launch_name: the name of entry `index` (null outside the table) and, where `flags` is not null, 1 if the branch
 * exists only in measurement builds (-DFDNN_ABLATION), 2 if the kernel runs at model load.  fdnn_debug_launch_record(1 / 0)
 * switches counting on / off for the whole process (off by default: a launch then pays one relaxed load);
 * fdnn_debug_launch_reset zeroes the counts; fdnn_debug_launch_counts copies the first `cap` of them, in table order, and
 * returns the table's size.  The counts are process-wide relaxed atomics: launches of scoring-loop, group and stream worker
 * threads are counted like the caller's own.  Recording changes no selection rule and no kernel. */
FDNN_API int fdnn_debug_launch_name_count(void);
FDNN_API const char *fdnn_debug_launch_name(int index, int *flags);
FDNN_API int fdnn_debug_launch_record(int on);
FDNN_API int fdnn_debug_launch_reset(void);
FDNN_API int fdnn_debug_launch_counts(unsigned long long *out, int cap);

/* Lazy output by lists (LazyOutputActivations, dnn.cc:355-392), tests and tools.
 * fdnn_debug_lists_check     the validator of the host entry points, host code, no device needed: 0, or -(row + 1) of the
 *   first row whose list is not well formed (row_ptr[0] != 0 answers as row 0).
 * fdnn_debug_ctx_lists_acc   acc [nnz]: the int32 accumulators as the score kernel of a plain call holds them (a
 *   wave-uniform branch of the same kernel, not a second one); otherwise as fdnn_ctx_lazy_output_lists (dnn.cc:355-392).
 * fdnn_debug_lists_launches  process-wide launch counts since load, returns 3: out[0] score kernel without the walk over
 *   saturating pairs, [1] with it, [2] the finish kernel.  (Not in the launch recorder's table: see fdnn_note.hpp;
 *   dnn.cc:355-392 is what the kernels compute.) */
FDNN_API int fdnn_debug_lists_check(const int32_t *row_ptr, const int32_t *nodes, int count, int output_dim);
FDNN_API int fdnn_debug_ctx_lists_acc(fdnn_ctx *c, int first, int count, const int32_t *row_ptr, const int32_t *nodes, int32_t *acc);
FDNN_API int fdnn_debug_lists_launches(unsigned long long *out, int cap);

/* Lazy output by lists over per-frame-group node unions (fdnn_model_set_lists_union; LazyOutputActivations,
 * dnn.cc:355-392), tests and tools.  With the switch on, fdnn_debug_ctx_lists_acc returns the accumulators the MFMA tile
 * holds (a wave-uniform branch of the production kernel).
 * fdnn_debug_lists_union_launches  process-wide counts since load, returns 4: out[0] union-build launches, [1] / [2] score
 *   launches without / with the walk over saturating pairs, [3] calls that had the switch on and were served by the
 *   dot-product kernels.  (Not in the launch recorder's table: see fdnn_note.hpp.)
 * fdnn_debug_ctx_lists_union       host buffers, validated like fdnn_ctx_lazy_output_lists: runs the union-build kernel
 *   alone for rows first .. first + count - 1 with groups of 32 * group_tiles rows (1..8) and copies back what it wrote:
 *   u_len [ceil(count / (32 * group_tiles))] every group's union length; u_nodes [nnz] group q's union, ascending, from
 *   index row_ptr[q * 32 * group_tiles] on, every word no union covers -1; pos [nnz] every entry's rank in its group's union.
 * fdnn_debug_lists_union_ref       the same three arrays from the host restatement (fdnn_lists_union.hpp), no device. */
FDNN_API int fdnn_debug_lists_union_launches(unsigned long long *out, int cap);
FDNN_API int fdnn_debug_ctx_lists_union(fdnn_ctx *c, int first, int count, const int32_t *row_ptr, const int32_t *nodes, int group_tiles,
                                        int32_t *u_len, int32_t *u_nodes, int32_t *pos);
FDNN_API int fdnn_debug_lists_union_ref(const int32_t *row_ptr, const int32_t *nodes, int count, int output_dim, int group_tiles,
                                        int32_t *u_len, int32_t *u_nodes, int32_t *pos);

/* Lazy output for a shared node set (LazyOutputActivations, dnn.cc:355-392), tests and tools.
 * fdnn_debug_set_check     the validator of the host entry points, host code, no device needed: 0, or -1 for a set that is
 *   not strictly ascending inside [0, output_dim).
 * fdnn_debug_ctx_set_acc   acc [count][len]: the int32 accumulators as the set kernel holds them (a wave-uniform branch of
 *   the same kernel, not a second one); otherwise as fdnn_ctx_lazy_output_set (dnn.cc:355-392).
 * fdnn_debug_set_launches  process-wide counts since load, returns 3: out[0] the MFMA set kernel without the walk over
 *   saturating pairs, [1] with it, [2] calls served by the list kernels as fallback.  (Not in the launch recorder's table:
 *   see fdnn_note.hpp.)
 * fdnn_debug_set_kernel    process-wide: 0 the default rule, 1 always the MFMA kernel where its shape applies, 2 always
 *   the fallback (the list kernels over the set as lists: the same bytes; dnn.cc:355-392 either way). */
FDNN_API int fdnn_debug_set_check(const int32_t *nodes, int len, int output_dim);
FDNN_API int fdnn_debug_ctx_set_acc(fdnn_ctx *c, int first, int count, const int32_t *nodes, int len, int32_t *acc);
FDNN_API int fdnn_debug_set_launches(unsigned long long *out, int cap);
FDNN_API int fdnn_debug_set_kernel(int mode);

/* Lazy output for per-segment node sets (LazyOutputActivations, dnn.cc:355-392), tests and tools.
 * fdnn_debug_sets_check     the validator of the host entry points, host code, no device needed: 0, or -(s + 1) for the first
 *   malformed segment s (malformed tables as a whole answer as segment 0); ctx_rows is the context's frame count.
 * fdnn_debug_ctx_sets_acc   acc, ragged like probs: the int32 accumulators as the kernel holds them (a wave-uniform branch of
 *   the same kernel, not a second one); otherwise as fdnn_ctx_lazy_output_sets (dnn.cc:355-392).
 * fdnn_debug_sets_launches  process-wide counts since load, returns 3: out[0] launches of the segmented MFMA kernel without
 *   the walk over saturating pairs, [1] with it, [2] calls served by the list kernels as fallback.  Not counted in
 *   fdnn_debug_set_launches and not in the launch recorder's table (fdnn_note.hpp).  fdnn_debug_set_kernel's mode applies to
 *   these entry points as well (dnn.cc:355-392 either way). */
FDNN_API int fdnn_debug_sets_check(const int32_t *seg_rows, const int32_t *set_ptr, const int32_t *nodes, int n_segs, int output_dim,
                                   int ctx_rows);
FDNN_API int fdnn_debug_ctx_sets_acc(fdnn_ctx *c, const int32_t *seg_rows, const int32_t *set_ptr, int n_segs, const int32_t *nodes,
                                     int32_t *acc);
FDNN_API int fdnn_debug_sets_launches(unsigned long long *out, int cap);

/* Dense output with a top-k return (CalculateOutput, dnn.cc:428-454), tests and tools.
 * fdnn_debug_topk_launches    process-wide counts since load, returns 2: out[0] launches of the resident form (the row kept
 *   in LDS), [1] of the streaming form (the passes re-read the row).  Not in the launch recorder's table (fdnn_note.hpp).
 * fdnn_debug_set_topk_kernel  process-wide: 0 the plan's rule (resident up to the resident width), 1 resident where the
 *   width allows, 2 always streaming -- the same bytes either way (dnn.cc:428-454).
 * fdnn_debug_topk_ref         the selection of fdnn_topk_rows_device from the host restatement (fdnn_topk.hpp) on host
 *   rows, host code, no device needed (dnn.cc:428-454).
 * fdnn_debug_topk_limits      the largest k and the widest resident row, as the kernels were built (dnn.cc:428-454). */
FDNN_API int fdnn_debug_topk_launches(unsigned long long *out, int cap);
FDNN_API int fdnn_debug_set_topk_kernel(int mode);
FDNN_API int fdnn_debug_topk_ref(const float *rows, int n, int width, int k, int32_t *nodes, float *vals);
FDNN_API int fdnn_debug_topk_limits(int *max_k, int *resident_width);

/* Dense output pooled over a node -> class map (CalculateOutput, dnn.cc:428-454), tests and tools.
 * fdnn_debug_pool_launches    process-wide counts since load, returns 2: out[0] launches of the resident form (the row kept
 *   in LDS), [1] of the streaming form (members gathered from memory).  Not in the launch recorder's table (fdnn_note.hpp).
 * fdnn_debug_set_pool_kernel  process-wide: 0 the plan's rule (resident up to the resident width), 1 resident where the
 *   width allows, 2 always streaming -- the same bytes either way (dnn.cc:428-454).
 * fdnn_debug_pool_ref         the pooling of fdnn_pool_rows_device from the host restatement (fdnn_pool.hpp) on host rows
 *   [n][width] under the map class_of [width], out [n][n_classes]; host code, no device needed (dnn.cc:428-454).
 * fdnn_debug_pool_limits      the number of partial sums of a class and the widest resident row, as the kernels were built
 *   (dnn.cc:428-454). */
FDNN_API int fdnn_debug_pool_launches(unsigned long long *out, int cap);
FDNN_API int fdnn_debug_set_pool_kernel(int mode);
FDNN_API int fdnn_debug_pool_ref(const float *rows, int n, const int32_t *class_of, int width, int n_classes, float *out);
FDNN_API int fdnn_debug_pool_limits(int *lanes, int *resident_width);

/* Dense output as decoder scores (CalculateOutput, dnn.cc:428-454), tests and tools.
 * fdnn_debug_loglik_launches    process-wide counts since load, returns 3: out[0] launches of the rows kernel's vector form,
 *   [1] of its scalar-access form, [2] of the entries kernel.  Not in the launch recorder's table (fdnn_note.hpp).
 * fdnn_debug_set_loglik_kernel  process-wide: 0 the plan's rule (vector where width % 4 == 0 and both bases are 16-byte
 *   aligned), 1 vector where allowed, 2 always scalar access -- the same bytes either way (dnn.cc:428-454).
 * fdnn_debug_loglik_ref         the scores of fdnn_loglik_rows_device from the host restatement (fdnn_loglik.hpp) on host rows
 *   [n][width], out [n][width] of the type; host code, no device needed (dnn.cc:428-454).
 * fdnn_debug_loglik_entries_ref the same for fdnn_loglik_entries_device (dnn.cc:428-454).
 * fdnn_debug_ln_ref             loglik::ln of count floats (dnn.cc:428-454). */
FDNN_API int fdnn_debug_loglik_launches(unsigned long long *out, int cap);
FDNN_API int fdnn_debug_set_loglik_kernel(int mode);
FDNN_API int fdnn_debug_loglik_ref(const float *rows, int n, const float *log_prior, int width, float floor, int type, void *out);
FDNN_API int fdnn_debug_loglik_entries_ref(const int32_t *nodes, const float *p, long long count, const float *log_prior, int width, float floor, int type, void *out);
FDNN_API int fdnn_debug_ln_ref(const float *x, long long count, float *out);

/* Forced alignment (LazyOutputActivations, dnn.cc:355-392), tests and tools.
 * fdnn_debug_align_launches    process-wide counts since load, returns 2: out[0] launches of the wave form, [1] of the
 *   workgroup form.  Not in the launch recorder's table (fdnn_note.hpp).
 * fdnn_debug_set_align_kernel  process-wide: 0 the plan's rule (one wave per segment where S <= 1024, else 256 threads), 1 the
 *   wave form where allowed, 2 always the workgroup form -- the same bytes either way (dnn.cc:355-392).
 * fdnn_debug_align_limits      returns 6: out[0] the longest transcript, [1] segments per launch, [2] the wave form's longest
 *   transcript, [3] rows in flight, [4] the back-pointer words of a segment that stay in LDS, [5] the scratch cap of a call
 *   in MiB (dnn.cc:355-392).
 * fdnn_debug_align_ref         fdnn_align_rows_device from the host restatement (fdnn_align.hpp) on host rows and host
 *   col / state_node / transition arrays; type FDNN_LOGLIK_F32 / _F16 with log_prior [width] and floor, or -1: the rows are
 *   scores and state_node, log_prior are not read; host code, no device needed (dnn.cc:355-392).
 * fdnn_debug_align_sets        the transcripts' node sets as the align calls build them: set_ptr [n_segs + 1], nodes (room
 *   for state_ptr[n_segs]) -- each segment's distinct nodes, ascending, the form fdnn_calculate_lazy_sets takes -- and col
 *   [state_ptr[n_segs]], nodes[set_ptr[s] + col[j]] == states[j]; host code (dnn.cc:355-392). */
FDNN_API int fdnn_debug_align_launches(unsigned long long *out, int cap);
FDNN_API int fdnn_debug_set_align_kernel(int mode);
FDNN_API int fdnn_debug_align_limits(int *out, int cap);
FDNN_API int fdnn_debug_align_ref(const float *rows, const int32_t *seg_T, const long long *row_off, const int32_t *row_ld, const int32_t *state_ptr,
                                  int n_segs, const int32_t *col, const int32_t *state_node, const float *log_prior, int width, float floor, int type,
                                  const float *self_lp, const float *next_lp, int32_t *path, float *total);
FDNN_API int fdnn_debug_align_sets(const int32_t *state_ptr, const int32_t *states, int n_segs, int32_t *set_ptr, int32_t *nodes, int32_t *col);

/* Alignment graphs (LazyOutputActivations, dnn.cc:355-392), tests and tools.
 * fdnn_debug_align_graph_launches    process-wide counts since load, returns 2: out[0] launches of the wave form, [1] of the
 *   workgroup form.  A counter of their own: not in the launch recorder's table (fdnn_note.hpp), apart from the chain's.
 * fdnn_debug_set_align_graph_kernel  process-wide: 0 the plan's rule (one wave per segment where S <= 64, else 256
 *   threads), 1 the wave form where allowed (S <= 256), 2 always the workgroup form -- the same bytes either way
 *   (dnn.cc:355-392).
 * fdnn_debug_align_graph_limits      returns 8: out[0] the most states, [1] segments per launch, [2] the wave form's most
 *   states, [3] the most arcs of a segment, [4] the arcs of a segment the wave form stages in LDS, [5] the back-pointer
 *   words of a segment that stay in LDS, [6] the scratch cap of a call in MiB, [7] the most states at which the rule takes
 *   the wave form (dnn.cc:355-392).
 * fdnn_debug_align_graph_ref         fdnn_align_graph_rows_device from the host restatement (fdnn_align_graph.hpp) on host
 *   rows and host arrays; type as fdnn_debug_align_ref; host code, no device needed (dnn.cc:355-392). */
FDNN_API int fdnn_debug_align_graph_launches(unsigned long long *out, int cap);
FDNN_API int fdnn_debug_set_align_graph_kernel(int mode);
FDNN_API int fdnn_debug_align_graph_limits(int *out, int cap);
FDNN_API int fdnn_debug_align_graph_ref(const float *rows, const int32_t *seg_T, const long long *row_off, const int32_t *row_ld,
                                        const int32_t *state_ptr, int n_segs, const int32_t *col, const int32_t *state_node, const float *log_prior,
                                        int width, float floor, int type, const int32_t *arc_ptr, const int32_t *arc_src, const float *arc_lp,
                                        const float *start_lp, const float *final_lp, int32_t *path, float *total);

/* Alignment graphs, summed (LazyOutputActivations, dnn.cc:355-392), tests and tools.
 * fdnn_debug_fb_launches     process-wide counts since load, returns 4: out[0] forward launches of the wave form, [1] forward
 *   of the workgroup form, [2] backward of the wave form, [3] backward of the workgroup form.  A counter of their own: not
 *   in the launch recorder's table (fdnn_note.hpp).
 * fdnn_debug_set_fb_kernel   process-wide: 0 the plan's rule (one wave per segment where S <= 64, else 256 threads), 1 the
 *   wave form where allowed (S <= 256), 2 always the workgroup form -- the same bytes either way (dnn.cc:355-392).
 * fdnn_debug_fb_limits       returns 8: out[0] the most states, [1] segments per launch, [2] the wave form's most states,
 *   [3] the most arcs of a segment, [4] the arcs of a segment the wave form stages in LDS, [5] the total's partial sums,
 *   [6] the scratch cap of a call in MiB, [7] the most states at which the rule takes the wave form (dnn.cc:355-392).
 * fdnn_debug_fb_ref          fdnn_fb_rows_device from the host restatement (fdnn_fb.hpp) on host rows and host arrays; type
 *   as fdnn_debug_align_ref; gamma, and then t_ptr, t_src, t_lp, may be NULL; host code, no device needed (dnn.cc:355-392).
 * fdnn_debug_fb_math_ref     the two stated functions on host arrays: op 0 out[i] = exp_neg(a[i]) (b not read), op 1 out[i] =
 *   ladd(a[i], b[i]); host code (dnn.cc:355-392).
 * fdnn_debug_fb_math_device  the same on device arrays in a trivial kernel, enqueued on `stream` (dnn.cc:355-392). */
FDNN_API int fdnn_debug_fb_launches(unsigned long long *out, int cap);
FDNN_API int fdnn_debug_set_fb_kernel(int mode);
FDNN_API int fdnn_debug_fb_limits(int *out, int cap);
FDNN_API int fdnn_debug_fb_ref(const float *rows, const int32_t *seg_T, const long long *row_off, const int32_t *row_ld, const int32_t *state_ptr,
                               int n_segs, const int32_t *col, const int32_t *state_node, const float *log_prior, int width, float floor, int type,
                               const int32_t *arc_ptr, const int32_t *arc_src, const float *arc_lp, const float *start_lp, const float *final_lp,
                               const int32_t *t_ptr, const int32_t *t_src, const float *t_lp, float *total, float *gamma);
FDNN_API int fdnn_debug_fb_math_ref(int op, const float *a, const float *b, float *out, long long n);
FDNN_API int fdnn_debug_fb_math_device(int op, const float *d_a, const float *d_b, float *d_out, long long n, void *stream);

/* Splicing through a segment table in device memory (the scoring loop's live batches, fdnn_splice.hip), tests and tools.
 * fdnn_debug_splice_table   the splice alone, host in and host out: raw [raw_frames][raw_dim] -> x [rows][input_dim] under the
 *   `count` offsets; segs [n_segs][4] = (row, center, lo, hi), rows ascending from 0: row t of segment g reads the raw frames
 *   clamp(center + (t - row) + o, lo, hi), never outside the buffer.  use_table = 0 runs the launches every other caller has
 *   (the table by value, 96 segments a launch), use_table = 1 the kernel that reads the table from device memory: one launch.
 * fdnn_debug_live_launches  process-wide since load: launches of that kernel, and the longest table it has been given.  Not
 *   in the launch recorder's table (fdnn_note.hpp).
 * fdnn_debug_server_hold    on != 0: the loop's packer plans no batch and host submissions queue up; 0: it wakes and packs
 *   them.  Lets a test decide which submissions share a batch.  (fdnn_server_free packs whatever is still held.) */
FDNN_API int fdnn_debug_splice_table(const int *offsets, int count, int raw_dim, int input_dim, const float *raw, int raw_frames,
                                     const int32_t *segs, int n_segs, int rows, int use_table, float *x, int device);
FDNN_API int fdnn_debug_live_launches(unsigned long long *launches, unsigned long long *max_segs);
FDNN_API int fdnn_debug_server_hold(fdnn_server *s, int on);

/* Tests: write the word a fused soft-max workgroup raises (in host memory) when it gives up waiting for its frame tile's
 * siblings -- 1: as if a launch of this model had just done so (from the next call on the model runs the unfused soft-max
 * and says so once on stderr), 0: forget it.  The production path needs no call: fdnn_gemm.hip / fdnn_ppo.hip raise it. */
FDNN_API int fdnn_debug_raise_fuse_fault(fdnn_model *m, int value);

/* Measurement builds of the chained hidden-layer kernel (-DFDNN_CHAIN_CLK=1; the shipped library records nothing): with
 * out == NULL, give the context a buffer for the phase clocks of cap_tasks tasks; with out != NULL copy the records of the
 * launches since ([0] = tasks recorded, then from [8] ten words per task: block / task id, XCD / layer / frame tile, the
 * wall clock, seven cycle stamps) into out[8 + 10 * cap_tasks] and start over. */
FDNN_API int fdnn_debug_chain_clocks(fdnn_ctx *c, long long *out, int cap_tasks);

/* Layer 0 alone through the PRODUCTION kernels (no taps): u8_out [n][hidden_dim].  Large batches take the
 * screened path (fused chains on the fp32 matrix pipe, a rigorous bound on |fused - unfused|, exact unfused
 * recomputation of the outputs whose table index the difference could change); *recomputed (may be NULL)
 * receives how many outputs of this call were recomputed.  Tests compare u8_out with the oracle bit for bit. */
FDNN_API int fdnn_debug_layer0(fdnn_model *m, const float *x, int n, uint8_t *u8_out, unsigned long long *recomputed);

/* The int8 screening of the input layer, opened up for the parity tests: besides u8_out [n][hidden_dim] (as
 * fdnn_debug_layer0, int8-screened path at any batch size) t_out / dd_out [n][hidden_dim] receive what the screening kernel
 * computed per output -- t~ = 100 lin~ from the exact digit products, and Dd, the half-width its error bound vouches for
 * (fdnn_l0s.hip).  The bound's claim is |100 lin_ref - t~| <= Dd for the reference's lin (dnn.cc:219-264); the tests assert
 * it on every output and report the slack max |100 lin_ref - t~| / Dd.  Needs an input width of 64 .. 496. */
FDNN_API int fdnn_debug_layer0_screen(fdnn_model *m, const float *x, int n, uint8_t *u8_out, float *t_out, float *dd_out,
                                      unsigned long long *recomputed);

/* 1 when ANOTHER process held this GPU's marker (/dev/shm/fdnn-gpu-<pci bus id>, an advisory lock taken by the first process
 * that asks / loads a model there) when this process first looked: this process then scales its soft-max in a separate pass
 * instead of inside the output kernel, whose workgroups wait for one another and must not share the chip with another
 * process's (same results).  0 = this process owns the marker, or none could be created.
 * Negative = error.  The reference's concurrency model is threads of one process (MultiThreadedStressTest.java:48-69). */
FDNN_API int fdnn_device_shared(int device);

/* Fused soft-max health counter.  Large dense / batched-lazy calls scale their soft-max inside the output kernel: the
 * node tiles of a frame tile exchange row sums and wait for one another (bounded).  Within a process the library chains
 * those launches per device, so the wait is microseconds; a workgroup whose wait nevertheless timed out (another PROCESS
 * on the same GPU, see INTEGRATION.md: FDNN_FUSE_NORM=0) leaves its block to the frame tile's last workgroup -- same bits, tens of
 * milliseconds late.  *tiles = how many tiles that has happened to on this model since load (0 in a healthy setup).
 * SoftMax::apply, src/cpp/dnn.cc:534-544, is what is being computed. */
FDNN_API int fdnn_model_fuse_giveups(fdnn_model *m, unsigned long long *tiles);
/* Chained hidden layers health counter (fdnn_chain.hip: the int8 hidden layers of a large batch in one persistent launch,
 * a task waiting -- bounded, seconds -- only for its own frame tile's node tiles of the layer before).  *faults = waits that
 * ran into their bound on this model since load: 0 in a healthy setup; non-zero means a launch computed on rows that may
 * not have been written (counters left dirty by a killed launch, a wedged device).  The context that saw it re-zeroes its
 * counters and stops chaining; fdnn_calculate re-runs the affected pass before it returns; callers of the *_device entry
 * points, which do not synchronise, read this after their own synchronisation.
 * CalculateUntilLastHiddenLayer's layer loop, src/cpp/dnn.cc:413-423, is what is being computed. */
FDNN_API int fdnn_model_chain_faults(fdnn_model *m, unsigned long long *faults);
/* The model's raw device counter words, n <= 32 ([1] layer-0 outputs recomputed, [2] fused soft-max give-ups; kernel clock
 * stamps of timing builds from [4]).  Measurements only. */
FDNN_API int fdnn_debug_device_counters(fdnn_model *m, unsigned long long *out, int n);

/* The scratch audit (tests).  A context carries counter arrays that every launch assumes zero on entry
 * and that only the kernels put back to zero: the table of them is fdnn_debug_scratch_count entries long, entry `index` is
 * called fdnn_debug_scratch_name(index) (null outside the table).  All counts below are in table order, n at least the
 * table's length.
 * fdnn_debug_ctx_scratch        waits for the context's last work, copies every listed buffer to the host -- all of it, not
 *                               only the words a launch reaches -- and writes the number of non-zero words per buffer.  A
 *                               context whose chained launch faulted (fdnn_model_chain_faults) reports its chain counters clean:
 *                               they are dirty by design until the next hidden pass re-zeroes them.  Likewise the fused
 *                               soft-max exchange counters once a role-split fused launch of the model has given up
 *                               (fdnn_model_fuse_giveups): the library zeroes them before every fused launch from then on.
 * fdnn_debug_ctx_scratch_words  the buffers' lengths in 32-bit words.
 * fdnn_debug_ctx_scratch_poke   writes one word (the audit's self-test only: never launch on a context poked non-zero).
 * fdnn_debug_scratch_audit      process-wide, off by default (then nothing changes): while on, every context is counted the
 *                               same way when it goes back to its model's pool and when it is destroyed -- pooled contexts,
 *                               the debug entry points' own, a scoring loop's slots -- and the counts are added up.
 * fdnn_debug_scratch_dirty      reads and resets those totals: out[0 .. count) non-zero words per buffer, out[count] contexts
 *                               audited, out[count + 1] contexts that could not be read, out[count + 2] the nanoseconds
 *                               the audits themselves took, their waits included; n at least count + 3. */
FDNN_API int fdnn_debug_scratch_count(void);
FDNN_API const char *fdnn_debug_scratch_name(int index);
FDNN_API int fdnn_debug_ctx_scratch(fdnn_ctx *c, unsigned long long *out, int n);
FDNN_API int fdnn_debug_ctx_scratch_words(fdnn_ctx *c, unsigned long long *out, int n);
FDNN_API int fdnn_debug_ctx_scratch_poke(fdnn_ctx *c, int which, long long index, unsigned value);
FDNN_API int fdnn_debug_scratch_audit(int on);
FDNN_API int fdnn_debug_scratch_dirty(unsigned long long *out, int n);

/* ------------------------------------------------------------------ per-kernel timing (bench / profiling only)
 * Between begin and end every kernel launch of this model is bracketed by HIP
 * events recorded on the stream it is launched on; end() synchronizes them and
 * returns the summed device time and launch count per kernel kind. */
enum { FDNN_PROF_L0 = 0, FDNN_PROF_FIX = 1, FDNN_PROF_HIDDEN = 2, FDNN_PROF_OUTPUT = 3, FDNN_PROF_NORMALIZE = 4, FDNN_PROF_KINDS = 5 };
FDNN_API int fdnn_profile_begin(fdnn_model *m);
FDNN_API int fdnn_profile_end(fdnn_model *m, double *ms /*[FDNN_PROF_KINDS]*/, int *launches /*[FDNN_PROF_KINDS]*/);

/* ------------------------------------------------------------------ host-only helpers (no device needed)
 * The load-time half of the path, exposed so it can be checked on a machine
 * without a GPU: .bin parsing, the quantizer, the sigmoid table, and the
 * packed-blob sections the kernels read. */
typedef struct fdnn_host_model fdnn_host_model;
FDNN_API int fdnn_host_model_load(const char *path, float cutoff, fdnn_host_model **out);
FDNN_API void fdnn_host_model_free(fdnn_host_model *hm);
FDNN_API int fdnn_host_model_layers(const fdnn_host_model *hm); /* affine layers incl. fp32 layer 0 */
FDNN_API int fdnn_host_model_layer_in(const fdnn_host_model *hm, int j);
FDNN_API int fdnn_host_model_layer_out(const fdnn_host_model *hm, int j);
FDNN_API float fdnn_host_model_multiplier(const fdnn_host_model *hm, int j);            /* j >= 1 */
FDNN_API int fdnn_host_model_weights_q(const fdnn_host_model *hm, int j, int8_t *out);  /* out_dim x in_dim */
FDNN_API int fdnn_host_model_bias(const fdnn_host_model *hm, int j, float *out);
FDNN_API int fdnn_host_model_wsum128(const fdnn_host_model *hm, int j, int32_t *out);   /* 128 * sum_k w[node][k] */
FDNN_API long long fdnn_host_model_risky_pairs(const fdnn_host_model *hm, int j);       /* pairs that can saturate */
FDNN_API size_t fdnn_host_model_blob_size(const fdnn_host_model *hm);
/* The packed weight blob as bytes (what fdnn_model_export_blob hands to RCCL),
 * and the receiver-side validation of such bytes (magic/version/size), with no
 * device involved -- used by the world_size-2 gloo tests of the load protocol. */
FDNN_API int fdnn_host_model_blob(const fdnn_host_model *hm, void *out, size_t capacity);
FDNN_API int fdnn_host_blob_check(const void *bytes, size_t size, int *input_dim, int *hidden_dim, int *output_dim,
                                  int *n_affine);
FDNN_API int fdnn_host_sigmoid_lut(uint8_t *out1280); /* QuantizedSigmoid table, dnn.cc:100-115 */
FDNN_API int fdnn_host_quantize(const float *w, int rows, int cols, float cutoff, int8_t *out, float *multiplier);

/* ------------------------------------------------------------------ the unquantized net and the quantization report
 * The reference's one notion of accuracy is the distance between QuantizedDnn and the fp32 net it was made from
 * (FuncTest.diff, test/java/suskun/nn/FuncTest.java:59-74, against FeedForwardNetwork.calculate,
 * FeedForwardNetwork.java:133-148).  Both halves run on the device here: fp32 GEMMs on the f32-input MFMA
 * (fdnn_float.hip) and a report that accumulates over any number of calls.
 *
 * A layer's sum is, bit for bit, s = 0; for k ascending: s = fmaf(x[k], w[k], s); z = s + bias -- so a row's bytes depend
 * on the row alone (not on n, its position, or the chunk size), and fdnn_debug_float_layer_ref restates it on the host.
 * This is the fused chain, not Java's mul-then-add loop (:360-375): the two differ at the ulp level (DESIGN).
 * Sigmoid (:398-402) and soft-max (:404-414, no max subtraction) are fp32: DESIGN gives their bounds against float64.
 *
 * fdnn_float_model_load / _load_on <- FeedForwardNetwork.loadFromBinary, FeedForwardNetwork.java:209-224: the same .bin, the
 *   same rejections (FDNN_E_FORMAT) as fdnn_model_load; FDNN_E_DEVICE without a HIP device (no CPU path).
 * fdnn_float_model_input_dim      the width of a caller's row: the file's, padded to x4 -- fdnn_model_input_dim's value.
 * fdnn_float_model_layer_count    affine layers (:133-148 runs them all); fdnn_float_model_layer_dim(j) the nodes of layer j.
 * fdnn_float_calculate            <- calculate(float[][]), :133-148.  Host buffers x [n][dim] -> out [n][output_dim],
 *   host-synchronous; n == 0 is a no-op.  FDNN_E_ARG for a wrong dim or a null buffer.
 * fdnn_float_calculate_device     device buffers, enqueued on `stream`, not synchronised.
 * Calls on one float model are thread-safe: they are serialised on a mutex inside the model and, across streams, ordered
 * behind each other on the device (the model owns one set of activation buffers: this is a yardstick, not a serving path).
 * A large n goes through in chunks of fdnn_debug_float_set_chunk frames (0 = default, 4096); results never depend on it.
 *
 * fdnn_debug_float_layer          ONE layer j on a caller's host rows in [n][K_j] (K_0 = input_dim): lin [n][rows_j] receives
 *   z, act [n][rows_j] the sigmoid (the soft-max probabilities for the last layer); either may be NULL.  j == -1 is the input
 *   step (:121-128) on in [n][input_dim]: lin = x + shift, act = (x + shift) * scale.  fdnn_float_calculate is exactly the
 *   composition of these calls.  FDNN_E_ARG for a j outside -1 .. layer_count - 1.
 * fdnn_debug_float_layer_us       measurement only (tools/float_sweep.py), apart from the call the tests use: uploads in
 *   [n][K_j] once, runs layer j (0 .. layer_count - 1) once to warm up and then `reps` times back to back between two
 *   events; *us = device microseconds per run (the output layer's with its scale pass).  Copies nothing back.
 * fdnn_debug_float_layer_ref      the host restatement of a layer's sums, no device: w [rows][K] dense, in [n][K], lin [n][rows].
 * fdnn_debug_float_input_ref      the host restatement of the input step, no device; lin or act may be NULL.
 * fdnn_debug_float_launches       process-wide launch counts since load, returns 8: fgemm sigmoid, exp, sigmoid + tap,
 *   exp + tap, input step, report rows, report nodes, report fold.  (Not in the launch recorder's table: see fdnn_note.hpp.) */
typedef struct fdnn_float_model fdnn_float_model;
FDNN_API int fdnn_float_model_load(const char *path, fdnn_float_model **out);
FDNN_API int fdnn_float_model_load_on(const char *path, int device, fdnn_float_model **out);
FDNN_API void fdnn_float_model_free(fdnn_float_model *fm);
FDNN_API int fdnn_float_model_input_dim(const fdnn_float_model *fm);
FDNN_API int fdnn_float_model_output_dim(const fdnn_float_model *fm);
FDNN_API int fdnn_float_model_layer_count(const fdnn_float_model *fm);
FDNN_API int fdnn_float_model_layer_dim(const fdnn_float_model *fm, int index);
FDNN_API int fdnn_float_model_device(const fdnn_float_model *fm);
FDNN_API int fdnn_float_calculate(fdnn_float_model *fm, const float *x, int n, int dim, float *out);
FDNN_API int fdnn_float_calculate_device(fdnn_float_model *fm, const float *d_x, int n, float *d_out, void *stream);
FDNN_API int fdnn_debug_float_layer(fdnn_float_model *fm, int j, const float *in, int n, float *lin, float *act);
FDNN_API int fdnn_debug_float_layer_us(fdnn_float_model *fm, int j, const float *in, int n, int reps, double *us);
FDNN_API int fdnn_debug_float_layer_ref(const float *w, const float *bias, int rows, int K, const float *in, int n, float *lin);
FDNN_API int fdnn_debug_float_input_ref(const float *shift, const float *scale, int dim, const float *x, int n, float *lin, float *act);
FDNN_API int fdnn_debug_float_set_chunk(fdnn_float_model *fm, int rows);
FDNN_API int fdnn_debug_float_launches(unsigned long long *out, int cap);

/* The report (FuncTest.diff, FuncTest.java:59-74: per output node, |quantized - float| summed over the frames; the harness
 * prints the nodes above 0.1).  Two [n][output_dim] fp32 matrices per call, `ref` and `q`; the accumulators live on the
 * device (doubles and 64-bit counts, added to in a fixed order: the figures are a function of the sequence of calls).
 * A row with a NaN in either matrix counts in nan_rows and is left out of every other figure.
 * fdnn_report_add_device  device buffers, enqueued on `stream`;  fdnn_report_add  host rows, host-synchronous.
 * fdnn_report_read        synchronises the device; nodes_over = nodes whose sum exceeds `threshold`; node_sum [output_dim]
 *   receives the per-node sums unless NULL.  top1_agree counts rows whose arg max (first index on ties) is the same in both.
 * Calls on one report are serialised on a mutex inside it. */
typedef struct fdnn_report fdnn_report;
typedef struct {
  uint64_t frames, nan_rows, top1_agree, nodes_over;
  double sum_abs, max_abs, max_node_sum;
} fdnn_accuracy;
FDNN_API int fdnn_report_create(int device, int output_dim, fdnn_report **out);
FDNN_API void fdnn_report_free(fdnn_report *r);
FDNN_API int fdnn_report_reset(fdnn_report *r);
FDNN_API int fdnn_report_add_device(fdnn_report *r, const float *d_ref, const float *d_q, int n, void *stream);
FDNN_API int fdnn_report_add(fdnn_report *r, const float *ref, const float *q, int n);
FDNN_API int fdnn_report_read(fdnn_report *r, double threshold, fdnn_accuracy *acc, double *node_sum);

#ifdef __cplusplus
}
#endif
#endif /* FDNN_H */
