/*
 * pose_mi355x.h -- C ABI of the MI355X-native OpenPose inference path (libpose_mi355x.so).
 *
 * The reference (DeNA/Chainer_Realtime_Multi-Person_Pose_Estimation) is pure Python and has no FFI of
 * its own: the boundary its hot path sits behind is the Python class `PoseDetector`
 * (pose_detector.py:15-517).  This header is the C ABI a binding for that class would use; each entry
 * point names the reference interface it replaces (file:line relative to the reference repo).
 * The Python mirror of `PoseDetector` in this repo binds exactly these symbols through ctypes
 * (see INTEGRATION.md for the stub).
 *
 * Conventions: plain pointers and sizes only (no torch / HIP types in signatures; a HIP stream is
 * passed as void*).  Every function returns PMX_OK (0) or an error code; no exceptions cross the ABI;
 * pmx_last_error() returns a thread-local message for the last failing call.  One context per host
 * thread / stream; calls on a context are stream-ordered and asynchronous unless stated.  Contexts of different host threads may be created,
 * used and destroyed concurrently (never one context from two threads at once) and give the bits they give alone; every option belongs to
 * the context it was set on.
 * There is NO CPU fallback: pmx_create fails with PMX_ERR_NO_DEVICE when no gfx950 device is present.
 */
#ifndef POSE_MI355X_H
#define POSE_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PMX_ABI_VERSION 2

/* The reference has no limits on peaks, candidate connections, person hypotheses or persons (np.vstack / Python lists,
 * pose_detector.py:104-110,157,243).  The device-side buffers have CAPACITIES instead, owned by the context: they start at
 * the values below and, when an image needs more, are grown and the post-process of that batch is re-run before any result
 * is handed out (pmx_get_results / pmx_results_layout / the parity accessors) -- callers never see a truncated result. */
#define PMX_N_JOINTS 18          /* entity.py:9-45 */
#define PMX_N_LIMBS 19           /* entity.py:85-105 */
#define PMX_N_PAF 38
#define PMX_N_HEAT 19
#define PMX_INIT_PEAKS_PER_JOINT 128   /* initial capacity: peaks of one joint type per image */
#define PMX_INIT_SUBSETS 128           /* initial capacity: live person hypotheses during grouping */
#define PMX_INIT_PEOPLE 64             /* initial capacity: persons per result record */

enum pmx_status {
    PMX_OK = 0,
    PMX_ERR_INVALID = 1,     /* bad argument */
    PMX_ERR_HIP = 2,         /* HIP runtime error (message in pmx_last_error) */
    PMX_ERR_NO_DEVICE = 3,   /* no usable gfx950 GPU */
    PMX_ERR_WEIGHTS = 4,     /* forward called before all 92 layers were set / unknown layer */
    PMX_ERR_CAPACITY = 5,    /* batch / image larger than the context was created for */
    PMX_ERR_STATE = 6        /* call sequence error (e.g. postprocess before forward) */
};

/* per-image status bits (pmx_image_info.status).  The capacity bits are internal: they trigger the grow-and-re-run and are
 * never set in a record that is handed out. */
enum pmx_image_status {
    PMX_IMG_OK = 0,
    PMX_IMG_PEAK_OVERFLOW = 1,      /* more peaks of one joint type than the current capacity */
    PMX_IMG_CAND_OVERFLOW = 2,      /* more accepted candidates for one limb than the current capacity */
    PMX_IMG_SUBSET_OVERFLOW = 4,    /* more live subsets than the current capacity */
    PMX_IMG_TRIPLE_MATCH = 8,       /* third subset matches a connection: the reference raises IndexError
                                       (pose_detector.py:193,197); the binding re-raises it */
    PMX_IMG_PEOPLE_OVERFLOW = 16    /* more persons after the final filter than the record capacity */
};

typedef struct pmx_ctx pmx_ctx;

typedef struct pmx_image_info {
    int32_t n_people;   /* rows of poses/scores (pose_detector.py:515-516) */
    int32_t n_peaks;    /* len(all_peaks) (pose_detector.py:508); 0 => the reference's early return :509-510 */
    int32_t status;     /* pmx_image_status bits */
    int32_t n_subsets_raw; /* subsets alive before the final filter (pose_detector.py:248) */
} pmx_image_info;

/* Result record, one per image, contiguous on the device (what multi-GPU runs gather with RCCL) and in pmx_get_results:
 *     pmx_image_info info;
 *     double scores[people_cap];                  subsets[:, -2]        (pose_detector.py:516)
 *     double poses[people_cap][PMX_N_JOINTS][3];  [x, y, 2] | [0, 0, 0] (pose_detector.py:252-265)
 * people_cap is the context's current person capacity; query it (and the record size) with pmx_results_layout AFTER the
 * post-process and BEFORE sizing the output buffer: it grows when an image needs it. */
#define PMX_RECORD_BYTES(people_cap) (sizeof(pmx_image_info) + (size_t)(people_cap) * (1 + PMX_N_JOINTS * 3) * sizeof(double))

/* ---- library / device ------------------------------------------------------------------------ */
const char* pmx_version(void);
const char* pmx_last_error(void);
int pmx_device_count(int* n);

/* ---- context: PoseDetector.__init__ (pose_detector.py:16-35) ----------------------------------
 * Replaces model construction (`params['archs'][arch]()`, :23), `model.to_gpu()` (:31) and the device
 * selection (:30).  max_h/max_w bound the network input size (multiples of 8), max_batch the batch. */
int pmx_create(pmx_ctx** out, int device, int max_batch, int max_h, int max_w);
/* `params['archs'][arch]()` (entity.py:50-54; pose_detector.py:23, face_detector.py:15, hand_detector.py:15):
 * arch = "posenet" (models/CocoPoseNet.py), "facenet" (models/FaceNet.py, 71 maps) or "handnet" (models/HandNet.py, 22 maps). */
int pmx_create_net(pmx_ctx** out, const char* arch, int device, int max_batch, int max_h, int max_w);
void pmx_destroy(pmx_ctx* ctx);
/* Puts the context on a stream of the caller's (synchronises the stream it leaves).  From then on every launch and copy of the context --
 * the lanes of detect_precise fork from and join that stream -- is ordered after what the caller enqueued on it before the call and before
 * what the caller enqueues after it: device inputs (`on_device`) need no host synchronisation after their producer on that stream, device
 * outputs (pmx_render canvases, pmx_results_snapshot, the prepared samples) none before their consumer on it.  A handle of 0 / NULL selects
 * the context's OWN stream (created non-blocking): the legacy default stream cannot be given.  torch's default stream has the handle 0, so
 * a caller working on it must synchronise around the calls or use a side stream (torch.cuda.Stream()) for them. */
int pmx_set_stream(pmx_ctx* ctx, void* hip_stream);
int pmx_synchronize(pmx_ctx* ctx);                    /* cuda.get_device_from_id().synchronize(), :506 */
/* Test / measurement knobs (defaults are the product configuration):
 *   "kernel_gen" 1 | 5 | 6     conv kernel generation: 1 = LDS-staged weights (v1) everywhere, 5 = v5 for 3x3 / 7x7,
 *                              6 = default (v6 / conv1_1 kernel where they apply, else v5); all compute identical bits
 *   "force_variant_k1|k3|k7"   force one entry of the conv variant table for that kernel size (-1 = automatic)
 *   "conv_algo" 1 | 0 | 2 | 3  fp32 algorithm of the 3x3 / 7x7 layers.  The Winograd F(2x2, 3x3) kernel needs 16 instead of 36 products per
 *                              2x2 output tile and channel pair for a 3x3 layer; a 7x7 layer = four 3x3 sub-kernels summed in the
 *                              transformed domain + four 1-D F(2,3) sub-kernels for row 6 / column 6 + one direct tap: 100 instead
 *                              of 196.  Its blocks are equal and run one per CU, so a launch costs whole CU rounds.
 *                              1 (default): by launch size (pmx_api.hip::wino_mode) -- the Winograd kernel when the blocks fill at
 *                              least half of their rounds (batches); its UNIT mode (a tile's passes / chunk groups as separate
 *                              blocks writing slabs + the split-K combine kernel) when a cost model says the rounds would stay
 *                              mostly empty (the 46x46 layers of 1 - 4 and 8 images); else the direct kernels with split-K.
 *                              0: direct kernels everywhere.  2: the Winograd kernel on every eligible layer; 3: unit mode wherever
 *                              it applies (tests).  All forms are fp32 fused-multiply-add chains in a defined order with a plain-C
 *                              twin (oracle/conv_fma_ref.c); the Winograd forms differ from the direct chain by fp32 rounding (~1e-6
 *                              of the map scale; they are the closer ones to float64)
 *   "wino_min_fill" percent    tuning (default 50): share of the block slots of its CU rounds a launch must fill to take the Winograd kernel
 *   "wino_unit_eff" percent    tuning (default 80): in-round efficiency assumed for unit-mode blocks in the selection cost model
 *   "wino_geom" -1 | 0 | 1     block geometry of the plain Winograd kernel on 46-pixel-wide maps (the 46 x 46 maps of a 368 x 368 input):
 *                              -1 / 1 (default) = runs of 32 consecutive Winograd tiles (529 tiles = 16.5 blocks per map), 0 = the
 *                              8 x 16 pixel rectangles every other map size uses (18 per map).  Same bits either way
 *   "wino_tail" -1 | 0 | 1     run geometry: the part-filled last block of every image as K units + a combine kernel (the 16 full
 *                              blocks of 32 images x 2 branches are exactly 4 rounds of 256 CUs): -1 (default) by the cost model,
 *                              0 never, 1 wherever a unit plan exists.  The tiles of that block (row-major index >= 32 * full blocks)
 *                              are then summed unit by unit (C twin: `unit_from`); profile label "...r/t<chunks per unit>"
 *   "wino_tail_g" n            tuning: chunks per pass-1 unit of those tails (0 = automatic)
 *   "wino_split" 1 | 0 | pct   a batch whose plain launch of a 3x3 / 7x7 layer would end in a part-filled round of the CUs (equal
 *                              one-per-CU blocks: the round costs as much as a full one) is cut in two by images: the images of the
 *                              whole rounds through the plain kernel, the rest through the launch form of THEIR count (unit mode) --
 *                              1 (default) where the cost model gains >= 3 %, 0 never, 50 .. 100 = that threshold in percent.
 *                              Eight 368 x 496 frames: 5 + 3, 14.4 -> 13.4 ms.  Part of the arithmetic (an image's rounding then depends
 *                              on which side of the cut it lies): profile label "...@<first image>+<count>"
 *   "wino_unit_g" n            chunks per pass-1 unit of a launch that runs in unit mode as a whole (single images, small batches):
 *                              0 (default) = the plan a dispatch simulation over the device's CUs finishes first (one 368 x 368 image:
 *                              conv4_2 as 3 units of 6 / 6 / 4 chunks = 216 blocks in one round), n > 0 = n chunks, -1 = as many
 *                              units as 8 slabs allow (the rule until round 6).  Part of the arithmetic: profile label ".../u<n>"
 *   "wino_tail_merge" 1 | 0    batches of 46-wide maps whose tail lies in one tile row (46 x 46: 17 tiles per image): 1 (default) = the
 *                              tails of all images of the launch as one stream of tiles, 32 per block (every MFMA row a real tile);
 *                              0 = one part-filled block per image.  Same units, same bits; profile label "...r/t<g>m"
 *   "batch_chains" 0 | 1 | -1  pmx_detect_batch on a uniform fp32 batch of B images as two independent half-batch chains: images [0, B / 2) on
 *                              the context's stream, the rest on a second stream of the context's own, network and post-process alike,
 *                              forked at entry and joined before the call returns (whatever is enqueued on the context's stream afterwards
 *                              sees all B records; no host synchronisation is added).  Every layer's form and plan is chosen once for the
 *                              whole batch and launched per half, so maps and records are bit for bit those of the one-chain call; the
 *                              profile labels of the halves end in "@<first image>+<count>".  0 = never; 1 = wherever every layer keeps
 *                              its whole-batch plan on a half (no layer cut by "wino_split", the merged tails mergeable per half), else one
 *                              chain; -1 (default) = automatic: under "conv_algo" 1, when in addition the plain launch of every 7x7 layer is whole
 *                              rounds of the CUs for each half (32 or 16 frames of 368 x 368 on 256 CUs) and the per-launch profiler
 *                              (pmx_profile_enable 1) is off: its event pairs would time a launch's wait for the other chain.  Mixed-size batches,
 *                              pmx_detect_precise, "precision" 1 / 2, "keep_smoothed", the loss hook, backward and training contexts
 *                              always run one chain.  The second chain holds slab scratch of its own
 *   "precision" 0 | 1 | 2      0 (default): every convolution is the fp32 FMA chain the parity tests specify.  1: the 3x3 / 7x7
 *                              layers that run on the one-block-per-CU kernels use the bf16 matrix cores with every fp32 value
 *                              split into three bf16 terms (six products, fp32 accumulate): fp32-grade accuracy, 2.67x the
 *                              matrix rate, results equal to the fp32 path only to summation-order-sized noise (opt-in build only).
 *                              2: the f16 inference mode.  Every 3x3 / 7x7 layer (conv1_1 included; FaceNet / HandNet alike) runs on
 *                              the f16 matrix cores: per output y = sum over (16-channel chunk, tap) of f16(x) * f16(w), summed in
 *                              fp32 on v_mfma_f32_32x32x16_f16 in an order fixed per layer (chunk-major, taps row-major, no split-K),
 *                              then the fp32 epilogue (2x2 max-pool, + bias, ReLU).  f16(v) = round-to-nearest-even saturating at
 *                              +-65504 (no inf; f16 subnormals are kept, NaN stays NaN); weights are rounded once, on the device, into the layer's f16 pack; activations stay fp32 in device memory and
 *                              are rounded while a kernel stages them.  The 1x1 layers stay fp32.  The order does not depend on the
 *                              batch, the image's position or the segment layout: an image gives the same maps bit for bit alone,
 *                              anywhere in a uniform batch and inside a mixed-size batch (pmx_detect_images).  Accuracy against
 *                              the fp32 path: INTEGRATION.md section 4.  Any other value: PMX_ERR_INVALID, the option unchanged
 *                              Non-finite values, all three precisions (the forward contract; tests/test_gpu_nonfinite.py): relu(v) is
 *                              NaN if v is NaN, else max(v, +0); the 2x2 max-pool is NaN if any of its four inputs is NaN, else their
 *                              maximum; +-inf follow IEEE arithmetic (f16 mode: saturated to +-65504 first; bf16x3 mode: the split's
 *                              second term x - bf16(x) is inf - inf = NaN).  A direct kernel's output is non-finite exactly where
 *                              the float reference's is (relu, max-pool and convolution of PyTorch / NumPy).  A Winograd kernel's
 *                              output is non-finite at least there, and possibly elsewhere inside the same even-aligned 2x2 output
 *                              tile: the transforms share the tile's 4 x 4 input patch (7x7 layers: 8 x 8) and compute inf - inf = NaN.
 *                              No kernel is non-finite anywhere else.  A NaN weight therefore gives NaN maps and a NaN validation
 *                              loss, never a quietly zeroed channel
 *   "f16_bn" 0 | 64 | 128      f16 mode, a test seam: output channels per block of a 3x3 / 7x7 launch.  0 (default): 128 where the launch
 *                              then still has a block per CU, else 64.  64 | 128: that width whatever the launch size (128 only for
 *                              layers whose padded channel count is a multiple of 128; the others stay at 64).  Same bits either way
 *                              (the order above does not depend on it); per context; profile labels unchanged.  Any other value:
 *                              PMX_ERR_INVALID, the option unchanged
 *   "grad_precision" 0 | 2     pmx_conv2d_backward and pmx_backward_head (the values are named like "precision"): 0 (default) fp32
 *                              gradients; 2: dw and dx of a 3x3 / 7x7 layer with f16 operands and fp32 sums (the f16 paragraphs of
 *                              pmx_conv2d_backward and pmx_backward_head).  z, db, the masks and the 1x1 layers keep their launches, and
 *                              given the same inputs their bits.  pmx_backward_trunk does NOT read it: the trunk chain stays fp32 and
 *                              continues from whatever gradient the head chain left at conv4_2's output.  The train steps take the
 *                              gradient store as it is.  Per context.  Any other value (1, bf16x3, included): PMX_ERR_INVALID, the
 *                              option unchanged
 *   "loss_scale_log2" 0..24    k (default 0): a STATIC loss scale 2^k.  The next hooked forward with the loss gradients on multiplies the
 *                              two constants c of pmx_loss_grad_enable by 2^k on the host (exact); the losses and the maps do not change.
 *                              Everything downstream is linear, so the loss gradients, every g, dx, dw, db and the trunk gradient -- the
 *                              trunk chain's results included -- carry the factor 2^k, and the accessors return the stored, SCALED
 *                              values.  In fp32 the factor is exact bit for bit unless an unscaled intermediate is subnormal.  The value
 *                              in force when a forward ran stays with that forward's gradients (pmx_get_loss_grad_scale); a later change
 *                              relabels nothing.  The caller un-scales: by 2^-k on the host, or in a train step through the per-layer
 *                              scale, scale * 2^-k (pmx_train_set_grad_scale; exact).  Any other value: PMX_ERR_INVALID, the option
 *                              unchanged
 *   "fuse_conv1" 1 | 0         conv1_1 recomputed on conv1_2's halo tiles, one launch instead of two (default 1); identical bits
 *   "precise_lanes" 1..4       detect_precise: inference scales in flight at once, each on its own stream and working set (default 4;
 *                              1: one after the other on the context's stream); same bits
 *   "precise_plain" -1 | 0 | 1  detect_precise's forward passes on the plain Winograd kernels ("conv_algo" 2 for their duration): -1 (default) =
 *                              when all four lanes are in use (scales that share the chip should spend as little CU time as possible),
 *                              0 = the default selection, 1 = always.  Changes the fp32 rounding of the maps like any kernel choice
 *   "precise_lane_priority" 1 | 0   detect_precise: the lanes' streams get priorities, the last lane (the reference's largest scale) the highest
 *                              (default 1; takes effect for lanes created afterwards, i.e. set it before the first detect_precise); same bits
 *   "precise_table_cap" n      detect_precise: cached cubic tables at which the next pmx_precise_begin* starts the cache over (default 208)
 *   "cubic_rows" 1 | 0         detect_precise's float32 cubic resizes: separable through LDS (default) | one thread per element; same bits
 *   "conv1_wino" 1 | 0 | 2     that launch with conv1_2 as Winograd F(2x2, 3x3) on 16 x 16 squares (default 1: where "conv_algo" >= 1
 *                              and the launch has a block per CU; 2: whatever the launch size); 0: the direct 8 x 16 tiles everywhere
 *   "fuse_pairs" 1 | 0         the two 1x1 layers that end every stage as one launch (default) or as two; identical bits
 *   "ksplit" 0 | 1 | n         split-K of the 3x3 / 7x7 launches that cannot fill the chip (single images): 0 = automatic,
 *                              1 = never, n = n K slices wherever split-K applies.  The slices are combined in a fixed
 *                              order, so results stay deterministic; they differ in the last bits from the unsplit sum
 *   "ksplit_plan" digits       tuning: explicit slices, decimal digits = 16-channel chunks per slice (3221 = 3 + 2 + 2 + 1);
 *                              applied to launches whose chunk count equals the digit sum
 *   "keep_smoothed"            keep the smoothed heat maps for pmx_get_smoothed
 *   "stop_stage" 1..6          stop the network after this stage (profiling)
 *   "kp_flip_x" 0 | 1          pmx_keypoints: mirror the resized heat maps left-right before the peaks are taken (the reference's
 *                              `cv2.flip(heatmaps, 1)` for left hands, hand_detector.py:46-47)
 *   "peaks_gpu_branch"         the reference's GPU-branch peak extraction (17 x 17 un-normalised kernel, zero pad, >=)
 *   "pp_limbs_slices" -1 | n   blocks per (limb, image) of the candidate-pair scan: -1 (default) = 8 where the maps come at full
 *                              resolution (detect_precise, pmx_set_maps), one block otherwise; 0 / 1 = one block; same results
 *   "conv_min_lds", "conv_v5_lds", "pp_generic"   ablation switches
 * "pp_generic", "conv_min_lds", "conv_v5_lds" and "cubic_rows" choose between kernel forms that compute the same bits: switches for tests
 * and tuning, not configuration. */
int pmx_set_option(pmx_ctx* ctx, const char* key, int value);

/* ---- weights: serializers.load_npz (pose_detector.py:26) --------------------------------------
 * One call per Chainer-NPZ entry pair `<layer>/W` (float32 OIHW) + `<layer>/b`; names and shapes are the
 * 92 links of models/CocoPoseNet.py:26-129.  Host pointers; packed and uploaded immediately. */
int pmx_set_layer(pmx_ctx* ctx, const char* name, const float* w_oihw, const float* bias,
                  int cout, int cin, int ksize);
int pmx_weights_missing(pmx_ctx* ctx, int* n_missing);

/* ---- network forward: `self.model(x)` (pose_detector.py:499; models/CocoPoseNet.py:132-262) ----
 * pmx_forward_u8 also fuses `preprocess` (pose_detector.py:426-431): uint8 HWC BGR -> float32, /255 - 0.5.
 * pmx_forward_f32 is the reference's inner seam (x = float32 NCHW as produced by preprocess).
 * `on_device` != 0: the pointer is device memory on the context's device. */
int pmx_forward_u8(pmx_ctx* ctx, const uint8_t* bgr_nhwc, int batch, int h, int w, int on_device);
int pmx_forward_f32(pmx_ctx* ctx, const float* x_nchw, int batch, int h, int w, int on_device);
/* `cv2.resize(orig_img, (w, h))` (pose_detector.py:493; INTER_LINEAR uint8, OpenCV's fixed-point algorithm restated) on
 * the device, then pmx_forward_u8.  All images of the batch share one source size; identity when the sizes agree. */
int pmx_forward_u8_resized(pmx_ctx* ctx, const uint8_t* bgr_nhwc, int batch, int src_h, int src_w, int h, int w, int on_device);
int pmx_get_resized(pmx_ctx* ctx, uint8_t* out_nhwc, int batch, int h, int w);   /* parity accessor */
/* last-stage outputs h1s[-1] (PAF, B x 38 x h/8 x w/8) and h2s[-1] (heat, B x 19 x h/8 x w/8), float32 NCHW,
 * copied to host (synchronises).  Either pointer may be NULL. */
int pmx_get_maps(pmx_ctx* ctx, float* paf_nchw, float* heat_nchw);
/* test seam = the reference's `model=` constructor argument (pose_detector.py:19-20): install network
 * outputs directly (host float32 NCHW, B x 38|19 x fh x fw) instead of running the network. */
int pmx_set_maps(pmx_ctx* ctx, const float* paf_nchw, const float* heat_nchw, int batch, int fh, int fw);

/* ---- post-process (pose_detector.py:501-517) --------------------------------------------------
 * F.resize_images to (map_h, map_w) (:501-502) + compute_peaks_from_heatmaps CPU-branch semantics
 * (:75-110) + compute_connections (:135-181) + grouping_key_points (:183-250) + the rescale to original
 * image pixels (:513-514) + subsets_to_pose_array (:252-265), all on the device.
 * img_len: :511 passes map_w (fast path), :478 orig_img_w (precise path).
 * scale_xy: per image (sx, sy) = (orig_w / map_w, orig_h / map_h) as float64, or NULL for (1, 1).
 * gauss_w: the 2*radius+1 float64 taps scipy's gaussian_filter(sigma=2.5) uses (NULL -> computed in C).
 * Radii and sizes: pmx_set_gaussian takes radius 0 .. 16 (sigma up to 4.0 at SciPy's truncate = 4; radius 0 is the identity filter),
 * PMX_ERR_INVALID beyond.  Radius 10 without "pp_generic" runs the fast peak kernel, every other radius the generic one: same bits.
 * map_h x map_w may be any size from 1 x 1 with map_h * map_w < 2^31, whatever the size of the network output: larger (the usual
 * up-sampling), equal (the resize is then the identity, except that a zero weight next to an infinity gives NaN, as in the reference),
 * smaller (down-sampling), narrower than the filter radius on either axis (SciPy's 'reflect' then wraps more than once), one pixel wide.
 * Non-finite maps (pmx_postprocess, pmx_postprocess_images, pmx_detect_batch, pmx_detect_images, detect_precise; the forward's contract
 * is under option "precision"): the resize and the filter follow IEEE arithmetic in the reference's order, so the smoothed maps are
 * non-finite exactly where the reference's are.  Every comparison is the reference's ordered one: a non-finite smoothed value is never a
 * peak (NaN > x is false; -inf exceeds nothing; a filter of radius >= 1 spreads +inf to the neighbours, which it then does not exceed
 * -- only at radius 0 can a lone +inf be a peak, as in the reference), and neither is a pixel with a NaN 4-neighbour; the rest of the
 * channel and the other channels are not affected.  A limb score that is NaN (a NaN sample, or +inf and -inf samples together) is
 * never a candidate; +inf scores are kept, sort first among the candidates (ties by pair index, as the reference's stable sort) and
 * reach the connection, subset and person scores as +inf.  The threshold pruning of the
 * fast peak kernel ignores NaN pixels (fmaxf): no peak can exist where it exits, so the result is the reference's.  status stays 0.
 * tests/test_gpu_postprocess_edges.py; the oracle is pinned to the verbatim reference on the same inputs. */
int pmx_set_gaussian(pmx_ctx* ctx, const double* taps, int radius);
int pmx_postprocess(pmx_ctx* ctx, int batch, int map_h, int map_w, double img_len, const double* scale_xy);

/* ---- detect_precise (pose_detector.py:433-482) accumulated on the device ------------------------------------
 * begin(orig size) -> add_scale(host uint8 orig image, scaled size = ceil(orig * multiplier), :442-443) per inference scale ->
 * finish() (average, :469-470; installs the full-resolution maps as a batch of one) -> pmx_postprocess(ctx, 1, orig_h,
 * orig_w, img_len = orig_w, NULL) (:475-481).  cv2.resize(INTER_CUBIC) is restated (uint8 fixed-point and float32 paths).
 * Every add_scale of one begin / finish sequence resizes the SAME original image(s): the host buffer is uploaded by the first call and
 * a later call that passes the same pointer reuses the device copy, so the pixels must not change between begin and finish, and the
 * buffer must stay allocated until a synchronising call (pmx_get_results, pmx_get_maps, pmx_synchronize) has returned: add_scale only enqueues. */
int pmx_precise_begin(pmx_ctx* ctx, int orig_h, int orig_w);
int pmx_precise_add_scale(pmx_ctx* ctx, const uint8_t* bgr_hwc, int scaled_h, int scaled_w);
int pmx_precise_finish(pmx_ctx* ctx);
/* the same for n images of ONE original size (n <= the context's batch capacity; the reference handles one image per call): every
 * scale runs the n images as one batch through the network; finish() installs a batch of n -> pmx_postprocess(ctx, n, orig_h, orig_w,
 * orig_w, NULL).  bgr_nhwc: n x orig_h x orig_w x 3, contiguous.  Per image the results equal the single-image calls up to the
 * kernel-choice-by-launch-size rounding of the network. */
int pmx_precise_begin_batch(pmx_ctx* ctx, int n_images, int orig_h, int orig_w);      /* (at most 8 scales per sequence) */
int pmx_precise_add_scale_batch(pmx_ctx* ctx, const uint8_t* bgr_nhwc, int scaled_h, int scaled_w);
/* the same with the scale's POSITION in the reference's loop given (slot 0 .. 7, each once per sequence, no gaps at finish): the parts are
 * summed in slot order (:463,467) whatever order the scales are enqueued in, so the caller can enqueue the largest scale -- the longest
 * chain of the sequence -- first.  pmx_precise_add_scale* without a slot take the next free one. */
int pmx_precise_add_scale_at(pmx_ctx* ctx, const uint8_t* bgr_nhwc, int scaled_h, int scaled_w, int slot);
/* the per-axis cubic tables a context caches (~22 per distinct original size) and how often the cache was started over.  That happens
 * only inside pmx_precise_begin*, behind a device synchronisation, once `cached` has reached option "precise_table_cap" (default 208):
 * never while a sequence holds table pointers. */
int pmx_precise_table_stats(pmx_ctx* ctx, int* cached, int* trims);

/* FaceDetector / HandDetector post-process (face_detector.py:37-38,58-68; hand_detector.py:41,68-78) for facenet / handnet
 * contexts: F.resize_images(hs[-1], (out_h, out_w)) + gaussian_filter + per-channel arg-max.  out: batch x (maps - 1) x 4
 * float64 rows (x, y, confidence, valid); valid = 0 where the reference appends None.  Synchronises.
 * Non-finite maps (pmx_keypoints, pmx_keypoints_images, pmx_keypoints_boxes, pmx_keypoints_boxes_images): `heatmap.max()` of a smoothed
 * channel that holds a NaN anywhere is NaN and `max_value > thresh` is false, so such a channel yields no key point: valid = 0, x = y = 0
 * and confidence = NaN, however large its finite values are.  A channel whose maximum is +inf yields the key point of its +inf pixels
 * (the tie rule for equal maxima applies) with confidence +inf; -inf pixels never win.  The other channels are not affected.  Sizes and
 * radii as for pmx_postprocess. */
int pmx_keypoints(pmx_ctx* ctx, int batch, int out_h, int out_w, double thresh, double* out);

/* ---- face / hand key points for many boxes of ONE image (demo.py:30-55: per person a face crop and two hand crops) ------------------
 * The two entries of this form are adapters onto the many-image entries below (one implementation): the image as a list of one, image 0 on
 * every box; same checks, same PMX_ERR_* codes, same bytes.  facenet / handnet contexts.  boxes: n x 5 int32 (left, top, right, bottom, flip) in image pixels; a box may extend past the image (those
 * pixels are 0: PoseDetector.crop_image, pose_detector.py:401-424); flip = 1 mirrors the crop left-right (cv2.flip(img, 1) of a left hand,
 * hand_detector.py:29-30).  Every box must be non-empty with int32 extents, else PMX_ERR_INVALID naming the box, before anything runs.
 * The network input is the context's max_h x max_w (368 x 368 for the detectors): per box crop + mirror + cv2.resize INTER_LINEAR, the same
 * bytes as crop_image (+ [:, ::-1]) followed by pmx_forward_u8_resized.  img: img_h x img_w x 3 uint8 BGR, host (uploaded once per call;
 * read before the call returns) or device memory (on_device != 0).
 * pmx_forward_u8_boxes: gather + resize + forward of n <= max_batch boxes (pmx_get_resized reads the network input back); asynchronous. */
int pmx_forward_u8_boxes(pmx_ctx* ctx, const uint8_t* img, int img_h, int img_w, int on_device, const int* boxes, int n);
/* pmx_keypoints for the B images of the current maps (a forward or pmx_set_maps), each with its own output size and mirror:
 * out_hwf: B x 3 int32 (out_h, out_w, flip); out as pmx_keypoints (B x (maps - 1) x 4 float64).  Bit-identical per image to pmx_keypoints with
 * that size and option "kp_flip_x" = flip.  Synchronises. */
int pmx_keypoints_images(pmx_ctx* ctx, int batch, const int* out_hwf, double thresh, double* out);
/* the one-call form: boxes -> key points in each box's own pixel frame (out: n x (maps - 1) x 4 float64, as pmx_keypoints), in chunks of
 * max_batch enqueued back to back; one image upload, one D2H copy and one stream synchronisation per call.  n == 0: nothing, PMX_OK. */
int pmx_keypoints_boxes(pmx_ctx* ctx, const uint8_t* img, int img_h, int img_w, int on_device, const int* boxes, int n,
                        double thresh, double* out);

/* ---- boxes of MANY images (the people of a batch of frames): the implementation of both forms --------------------------------------------
 * images: n_images images of any, differing sizes; host memory (read before the call returns) or, with on_device != 0, device memory on the
 * context's device.  boxes6: n x 6 int32 (left, top, right, bottom, flip, image): columns 0..4 as above, image = index into `images`.  An
 * image that no box refers to is allowed; it is neither looked at nor uploaded.  Checked before anything is enqueued, PMX_ERR_INVALID with
 * the box or the image named: n_images < 1 with n > 0, an image index outside 0 .. n_images - 1, a null or non-positive-size image that a
 * box refers to, an empty box, a bad flip.  A posenet context: PMX_ERR_STATE.  Per box the network input holds the same bytes, and the key
 * points are those, of a call with that box and its own image alone (same kernels chosen: bit-identical; the f16 mode makes an image's maps
 * independent of batch size and position). */
typedef struct pmx_box_image { const uint8_t* bgr; int h, w; } pmx_box_image;   /* h x w x 3 uint8 BGR */
/* gather + resize + forward of n <= max_batch boxes (1 .. max_batch, else PMX_ERR_CAPACITY); asynchronous. */
int pmx_forward_u8_boxes_images(pmx_ctx* ctx, const pmx_box_image* images, int n_images, int on_device, const int* boxes6, int n);
/* boxes -> key points, out: n x (maps - 1) x 4 float64 rows in box order, each in its box's own pixel frame (as pmx_keypoints).  Chunks of
 * max_batch crops are taken in box order ACROSS image borders: 70 boxes on a batch-32 context are network calls of 32, 32 and 6 crops
 * whatever images they belong to, each with one gather launch.  Per call, however many images: one staging copy (it carries the image
 * table -- address, height, width per image; host images are placed in one device store at 64-bit byte offsets -- next to the crop
 * descriptors and tables), one upload per referenced host image enqueued back to back with no synchronisation between them, one D2H copy
 * and ONE stream synchronisation.  n == 0: nothing, PMX_OK.  Gaussian radii other than 10, "peaks_gpu_branch" and "pp_generic" fall back to
 * a per-crop key-point loop (so does pmx_keypoints_boxes). */
int pmx_keypoints_boxes_images(pmx_ctx* ctx, const pmx_box_image* images, int n_images, int on_device, const int* boxes6, int n,
                               double thresh, double* out);

/* ---- result images: draw_person_pose (pose_detector.py:520-553), cv2.addWeighted(img, 0.6, canvas, 0.4, 0) (:574, demo.py:27) and, per
 * person, draw_face_keypoints / draw_hand_keypoints / cv2.rectangle (demo.py:30-55) for a list of images in ONE launch -----------------------
 * The contract is the package's own host functions, byte for byte (OpenCV's line and circle rasters are not pinned; the stand-ins are):
 *   blend == 0      canvas = pose_detector.draw_person_pose(img, poses)
 *   blend != 0      canvas = demo.add_weighted(img, 0.6, draw_person_pose(img, poses), 0.4, 0), then the image's parts in array order, each
 *                   opaque over the canvas: a face (kind 0, 70 key points) as face_hand_detector.draw_face_keypoints draws it -- every valid
 *                   key point a radius-2 disc, then the `face_line_indices` segments whose two ends are valid, thickness 1, colour
 *                   (255, 255, 0) -- a hand (kind 1, 21 key points) as draw_hand_keypoints does -- per finger and bone the radius-3 discs of
 *                   its valid ends, then the bone's thickness-1 segment if both are -- and last demo.draw_rectangle((left, top), (right,
 *                   bottom), white, 1): the one-pixel outline of the box, clipped.  This is demo.render(img, poses, parts).
 * Every host step assigns its colour to the pixels it covers, one step after the other, so a pixel holds the colour of the LAST step that
 * covers it -- within the pose layer and within the parts layer separately; the blend sits between the two.
 *   Poses    np.round (half to even) of x, y and v first, then int32.  Limbs 9 and 13 are skipped; a limb is drawn when the rounded v of both
 *            joints is non-zero (thickness 2, LIMB_COLORS), all limbs of all people before the joints (radius-3 discs where the rounded v is
 *            non-zero, JOINT_COLORS).
 *   Segment  _draw_line in float64, every operation rounded on its own (no fused multiply-add): r = thickness / 2; the box xa = max(0,
 *            floor(min(x1, x2) - r)) .. xb = min(w - 1, ceil(max(x1, x2) + r)), ya .. yb alike, nothing when it is empty; dx = x2 - x1,
 *            dy = y2 - y1, L2 = dx * dx + dy * dy; for a pixel (x, y) of the box t = ((x - x1) * dx + (y - y1) * dy) / L2 clipped to [0, 1],
 *            or 0 when L2 is not > 0; ex = x - (x1 + t * dx), ey = y - (y1 + t * dy); covered when ex * ex + ey * ey <= r * r + 0.25.
 *   Disc     _draw_disc on the centre truncated toward zero (int()): the pixels of the box max(0, cx - R) .. min(w - 1, cx + R) (y alike)
 *            with (x - cx)^2 + (y - cy)^2 <= R^2 in integers.
 *   Key point  the row's (x, y) + (left, top) of its part in float64 (fractional coordinates stay fractional in the segment test).
 *   Blend    per channel saturate(rint(img * 0.6f + c * 0.4f + 0.0f)): three float32 operations in that order, round half to even; c is the
 *            pose layer's colour, or the image's own pixel where nothing was drawn (also for an image without people, which the host blends
 *            with itself).
 * images: n_images images of any sizes, host memory (read before the call returns) or device memory (on_device != 0).  poses: the people of
 * image 0, then of image 1, ...; n_people: one count per image (NULL: nobody anywhere).  parts: each names its image; keypoints: the parts'
 * rows (x, y, confidence, valid) end to end in part order, 70 per face and 21 per hand, in the box's own pixel frame.  out: the canvases end
 * to end in image order (h x w x 3 bytes each), host memory, or device memory on the context's device (out_on_device != 0; it must not
 * overlap the images).  Works on a context of any architecture and needs no weights; maps, records and retained state stay untouched.
 * Per call: the primitive table (built on the host in drawing order, with each step's clipped box) travels with the per-image table in ONE
 * staging copy; one launch covers the 64 x 16 pixel tiles of all images; host output comes back in one D2H copy behind ONE stream
 * synchronisation, device input and output synchronise nothing (the buffers grow on demand, which synchronises once).
 * PMX_ERR_INVALID, before anything is enqueued and with the offender named: a null image or one of non-positive size, a negative count, a
 * part whose image index or kind is out of range, parts with blend == 0 (the host has no such form), a non-finite v, a non-finite
 * coordinate or one of magnitude >= 2^30 on a joint or key point that would be drawn.  n_images == 0: nothing, PMX_OK. */
typedef struct pmx_render_part { int image, kind /* 0 face: 70 points, 1 hand: 21 */, left, top, right, bottom; } pmx_render_part;
int pmx_render(pmx_ctx* ctx, const pmx_box_image* images, int n_images, int on_device, const double* poses, const int* n_people,
               const pmx_render_part* parts, int n_parts, const double* keypoints, int blend, uint8_t* out, int out_on_device);

/* fused: forward_u8 + postprocess (PoseDetector.__call__, pose_detector.py:484-517, for images already
 * at the network input size; cv2.resize at :493 is the identity for them) */
int pmx_detect_batch(pmx_ctx* ctx, const uint8_t* bgr_nhwc, int batch, int h, int w, int on_device,
                     int map_h, int map_w, double img_len, const double* scale_xy);

/* ---- batches of images of DIFFERENT sizes ------------------------------------------------------------------------
 * The reference takes any image in any call and picks the network size per image (pose_detector.py:490-493, compute_optimal_size
 * :57-73), so a stream of frames has a new size every few images.  pmx_detect_images is `PoseDetector.__call__` (:484-517) for B
 * such images in ONE call: per image the cv2.resize of :493 on the device, the network over all images as one launch per layer
 * (consecutive images of one network size form a segment; the segments lie end to end in the activation buffers and a per-level
 * table tells a block which segment its tile belongs to), the post-process per run of images with equal sizes -- with the image's
 * own map size (:491, :501-502), img_len = map_w (:511) and coordinate rescale orig / map (:513-514).  Records in image order
 * (pmx_get_results as usual).  Capacity: B <= max_batch and the sum of net_h * net_w <= max_batch * max_h * max_w of pmx_create.
 * Per image the maps equal those of a single-image call that runs the plain Winograd kernels (options "conv_algo" 2, "conv1_wino" 2)
 * bit for bit; against the default single-image call (unit-mode / split-K kernels) they differ by fp32 rounding like any two batch
 * sizes do.  Callers sort their images by size to get few segments; any order is valid. */
typedef struct pmx_image {
    const uint8_t* bgr;      /* src_h x src_w x 3 uint8 BGR, host memory; read before the call returns */
    int src_h, src_w;        /* original size */
    int net_h, net_w;        /* network input size: compute_optimal_size(orig, inference_img_size), multiples of 8 */
    int map_h, map_w;        /* size the network maps are up-sampled to: compute_optimal_size(orig, heatmap_size) */
} pmx_image;
int pmx_detect_images(pmx_ctx* ctx, const pmx_image* images, int batch);
/* the two halves apart: the network on uint8 images already at their network sizes, pixels end to end (image i: net_hw[2 i] x
 * net_hw[2 i + 1] x 3; host or device memory), and the post-process of those maps (image i up-sampled to map_hw[2 i] x map_hw[2 i + 1],
 * img_len = that width; scale_xy: batch x 2 doubles or NULL as in pmx_postprocess) */
int pmx_forward_u8_images(pmx_ctx* ctx, const uint8_t* bgr, const int* net_hw, int batch, int on_device);
int pmx_postprocess_images(pmx_ctx* ctx, const int* map_hw, int batch, const double* scale_xy);
/* parity accessor: the network output of ONE image of the current batch (uniform or mixed) as NCHW float32, paf 38 x fh x fw and heat
 * 19 x fh x fw (either may be NULL); fh x fw must be the image's map size (network size / 8).  Synchronises. */
int pmx_get_image_maps(pmx_ctx* ctx, int image, float* paf, float* heat, int fh, int fw);

/* ---- detect_precise for a LIST of images of any sizes (pose_detector.py:433-482 per image) ------------------------------------
 * Per image exactly detect_precise: each scale k does the uint8 cubic resize of the original to scaled_hw[2 k] x scaled_hw[2 k + 1] (a copy
 * when that is the original size), the pad to a multiple of 8 with (104, 117, 123), the forward, the x8 cubic up-sampling, the crop and the
 * cubic resize to the original size; the parts are summed left to right from 0.f in slot order and divided by n_scales; the post-process
 * runs at the original size with img_len = orig_w and no rescale.  Results in image order through pmx_get_results / pmx_get_peaks /
 * pmx_get_connections / pmx_get_subsets (image index = position in `images`).
 * Every (image, scale) pair is a segment of ONE network forward on the context's stream (pairs of equal network size merge; no lanes,
 * no stream priorities): the maps do not depend on GPU_MAX_HW_QUEUES.  In fp32 they equal, bit for bit, the pmx_precise_begin / add_scale /
 * finish sequence of each image alone with options "precise_plain" 1 and "conv1_wino" 2 (the plain Winograd kernels a segmented forward
 * runs); in f16 mode ("precision" 2) the default sequence.  "precision" 1 (bf16x3) is refused with PMX_ERR_INVALID.
 * Capacity, checked before anything is enqueued (PMX_ERR_CAPACITY naming what overflowed): n <= max_batch, the network-input pixels of
 * all pairs (sum of padded h x w) <= max_batch x max_h x max_w, the level-3 pixels (sum of h/8 x w/8) within the cat / branch buffers,
 * 32-bit offsets and buffer extents.  The call's planar temporaries, full-resolution maps and tables live in per-call buffers that grow
 * on demand and are never cached by size; the tables stay valid until the next call (a capacity grow-and-re-run of the post-process
 * inside pmx_get_results uses them).  Synchronises once.  The caller's images are read before the call returns. */
typedef struct pmx_precise_image {
    const uint8_t* bgr;      /* orig_h x orig_w x 3 uint8 BGR, host memory */
    int orig_h, orig_w;
    int n_scales;            /* 1 .. 8 */
    int scaled_hw[16];       /* (h, w) per scale in the reference's loop order (:441-443): ceil(orig * multiplier), computed by the caller */
} pmx_precise_image;
int pmx_detect_precise_images(pmx_ctx* ctx, const pmx_precise_image* images, int n);
/* the averaged maps of image `image` of the last pmx_detect_precise_images call as NCHW float32: paf 38 x h x w, heat 19 x h x w (either
 * may be NULL); h x w must be the image's original size.  Synchronises. */
int pmx_get_precise_image_maps(pmx_ctx* ctx, int image, float* paf, float* heat, int h, int w);
/* bytes of the per-call table buffer the context holds for pmx_detect_precise_images (diagnostics: bounded by the largest call, not by
 * the number of distinct sizes seen) */
int pmx_precise_images_table_bytes(pmx_ctx* ctx, size_t* bytes);

/* ---- validation loss: Validator.evaluate (train_coco_pose_estimation.py:129-159) without the data loader ------------------------
 * The forward under no_backprop_mode (:147-150) followed by compute_loss (:41-73): per stage the mean squared error of the PAF and of the
 * heat-map output against the label maps, ignored pixels excluded by overwriting the target with the output (:62-63).  Forward only: no
 * backward pass, no optimiser.  These entries take images that are already samples (insize x insize, mask resized and dilated); the
 * resizes, the 16 x 16 dilation of the ignore mask (coco_data_loader.py:340) and the augmentation are pmx_samples_prepare, below.  posenet contexts (facenet / handnet: PMX_ERR_STATE), uniform batches, fp32 and f16 mode.  With the hook off
 * (the default) no call of this header launches, allocates or synchronises anything more than before.
 *
 * Targets.  pmx_loss_set_poses evaluates generate_heatmaps + generate_pafs (coco_data_loader.py:208-268) on the device in float64, product
 * by product as NumPy does (no fused multiply-add), and casts to float32 (:229, :268): heat of a joint type = max over the people with v > 0
 * of exp(-0.5 * d2 / heat_sigma**2), channel 18 = 1 - the max over all joints; PAF of a limb = the sum of the unit vectors of the people
 * whose band (0 <= hor <= dist, |ver| <= paf_width, `ver` through the reference's rotation by pi / 2 with its cos = 6.123233995736766e-17,
 * :238-246) covers the pixel, divided by their number (:266); a person whose joint has v <= 0 (:260) or whose joints coincide (:233) is
 * skipped.  The labels are evaluated only at the four corner pixels each map pixel of h/8 x w/8 needs and combined as F.resize_images does
 * (:57-58: float64 weight products cast to float32, four float32 products summed left to right); the batch x 57 x h x w maps never exist.
 *   poses        sum(n_people) x 18 x 3 float64 rows (x, y, v) in network-input pixels, image after image
 *   n_people     batch ints (>= 0)
 *   ignore_mask  batch x h x w uint8, non-zero = ignored, or NULL (nothing ignored); resized with the same float32 weighted sum, a map
 *                pixel is ignored when that sum is > 0 (:59-60)
 *   heat_sigma   params['heatmap_sigma'] (entity.py: 7), paf_width: params['paf_sigma'] (8)
 * Asynchronous; the host arrays are read before the call returns.
 * pmx_loss_set_targets installs label maps the caller made: float32 NCHW host maps (batch x 38 / 19 x th x tw) either at th x tw = h x w
 * (resized on the device as :57-60 do) or already at h/8 x w/8 (taken as they are, :56); ignore_mask: batch x th x tw uint8 or NULL.
 * Errors of both (checked before anything is enqueued; the context stays usable): PMX_ERR_INVALID for null arguments, n_people < 0, a
 * non-finite x or y of a visible joint, heat_sigma <= 0, paf_width < 0, h or w no multiple of 8, th x tw neither of the two sizes;
 * PMX_ERR_CAPACITY for batch > max_batch or h * w > max_h * max_w. */
int pmx_loss_set_poses(pmx_ctx* ctx, const double* poses, const int* n_people, int batch, int h, int w,
                       const uint8_t* ignore_mask, double heat_sigma, double paf_width);
int pmx_loss_set_targets(pmx_ctx* ctx, const float* paf_t, const float* heat_t, const uint8_t* ignore_mask,
                         int batch, int th, int tw, int h, int w);
/* on != 0: every uniform forward (pmx_forward_u8 / _f32 / _u8_resized, pmx_detect_batch) enqueues, right after the last launch of each
 * stage, one launch that reads the stage's output where the network left it and accumulates, per branch, the float64 sum of
 * ((double)d * d) with d = y - t in float32 (F.mean_squared_error's difference), ignored pixels contributing 0 -- a wave-64 reduction, then
 * LDS across the block's waves, one partial per block and branch in a fixed slot -- and after the last stage one launch that adds the
 * partials in slot order and divides by batch * 38 * h/8 * w/8 and batch * 19 * h/8 * w/8 (the mean over ALL elements, :65-66).  No
 * floating-point atomics: the same bits on every run.  No synchronisation and no host copy between the stages; the maps of a hooked
 * forward are bit-identical to an unhooked one (the hook only reads).  With the hook on, PMX_ERR_STATE (before anything is enqueued) for
 * a forward without targets or with targets of another batch, h or w, and for every mixed-size or precise entry (pmx_forward_u8_images,
 * pmx_detect_images, pmx_precise_*, pmx_detect_precise_images). */
int pmx_loss_enable(pmx_ctx* ctx, int on);
/* the losses of the last hooked forward: paf_loss6[s], heat_loss6[s] = paf_loss_log[s], heatmap_loss_log[s] of compute_loss (:70-71) for
 * stage s + 1; n_stages = 6, or option "stop_stage" (the later entries are 0).  PMX_ERR_STATE before any hooked forward.  Synchronises. */
int pmx_loss_get(pmx_ctx* ctx, double* paf_loss6, double* heat_loss6, int* n_stages);
/* one stage of compute_loss for the CURRENT maps (a forward's last stage, or pmx_set_maps) against the targets (PMX_ERR_STATE unless both
 * exist with the same batch and map size).  Synchronises. */
int pmx_loss_current_maps(pmx_ctx* ctx, double* paf_loss, double* heat_loss);
/* Validator.evaluate for one batch (:146-157): pmx_forward_u8 with the hook on (whatever pmx_loss_enable set, which it leaves unchanged) +
 * pmx_loss_get.  out13 = total (`val/loss`: the stages' paf + heat added in stage order), paf[6], heat[6].  Synchronises. */
int pmx_validate_batch(pmx_ctx* ctx, const uint8_t* bgr_nhwc, int batch, int h, int w, int on_device, double* out13);
/* the public label generator / parity accessor: generate_pafs (38 x h x w) and generate_heatmaps (19 x h x w) of image `image` of the
 * poses of the last pmx_loss_set_poses, float32 at full resolution (h x w as set there).  Either pointer may be NULL.  Synchronises. */
int pmx_get_labels(pmx_ctx* ctx, int image, float* paf, float* heat, int h, int w);
/* parity accessor: the current targets as NCHW float32 (batch x 38 | 19 x h/8 x w/8) and the resized ignore mask (batch x h/8 x w/8, 0 | 1);
 * any pointer may be NULL.  Synchronises. */
int pmx_get_loss_targets(pmx_ctx* ctx, float* paf_t, float* heat_t, uint8_t* mask);
/* The gradient of compute_loss at the twelve stage outputs, where loss.backward() starts (train_coco_pose_estimation.py:90-126).  on != 0:
 * while the loss hook is on as well, every hooked uniform forward enqueues, after each stage's loss launch, one more launch that writes
 * d(total_loss)/dy of that stage into a context buffer [stage][image][map pixel][38 | 19].  total_loss is the plain sum over stages and
 * branches (:68), so this is F.mean_squared_error's backward with gy = 1: d = y - t in float32, c = (float)(2.0 / N) with
 * N = batch * 38 * h/8 * w/8 (PAF) or batch * 19 * h/8 * w/8 (heat), gradient = c * d (one float32 product) where the resized ignore mask
 * is 0 and +0.0f where it is set (:62-63 make the difference zero there).  The maps and losses of the forward keep their bits.  Off (the
 * default): nothing more is launched or allocated. */
int pmx_loss_grad_enable(pmx_ctx* ctx, int on);
/* the gradients of stage + 1 (stage 0 .. 5) of the last hooked forward, NCHW float32 (batch x 38 | 19 x h/8 x w/8); either pointer may be
 * NULL.  PMX_ERR_INVALID for a stage outside 0 .. 5; PMX_ERR_STATE before a hooked forward with the gradients on, and for a stage that
 * forward did not run (option "stop_stage").  Synchronises. */
int pmx_get_loss_grads(pmx_ctx* ctx, int stage, float* gpaf_nchw, float* gheat_nchw);
/* k of option "loss_scale_log2" as it was when the last hooked forward with the gradients on ran: the stored loss gradients, and whatever a
 * backward makes of them, are 2^k times the gradients of the loss.  PMX_ERR_STATE before such a forward. */
int pmx_get_loss_grad_scale(pmx_ctx* ctx, int* scale_log2);

/* ---- sample preparation: the pixel side of CocoDataLoader.generate_labels (coco_data_loader.py:72-205, 334-341) ---------------------
 * One call prepares up to max_batch samples from images of different sizes: one launch per step over all samples, every kernel a gather
 * (no atomics: the same bits on every run).  The NUMBERS of a sample (scale, matrix, crop offset, colour offsets, flip) come from the
 * caller; the reference's random policy and its int32 pose arithmetic are host code (samples.py).  Steps, in the reference's order:
 *   resize   (resized_w, resized_h) != (0, 0): cv2.resize (linear, uint8; the contract of pmx_forward_u8_resized) of the image, and of the
 *            mask as 0/1 bytes followed by != 0 (:76-77)
 *   rotate   has_rotate: cv2.warpAffine of the resized image to rot_w x rot_h, cubic with constant border 128 (round-half-even of 127.5),
 *            and of the mask x 255, linear with border 0, followed by > 0 (:115-117).  OUR contract, modelled on OpenCV's fixed-point scheme;
 *            no equality with an OpenCV build is claimed.  `inv` = the INVERSE matrix M0 .. M5 in float64.  For destination (x, y):
 *            X = (rint((M1*y + M2)*1024) + 16 + rint(M0*x*1024)) >> 5 and Y alike from M3, M4, M5, rint = round-half-even in float64 without
 *            fused multiply-add; source pixel X >> 5, fraction X & 31.  Cubic: taps -1 .. +2, per fraction f/32 four float32 coefficients
 *            of the Keys kernel with A = -0.75; linear: taps 0 .. +1 with (1 - f/32, f/32).  2-D weights rint(cy[i]*cx[j]*32768) (float32
 *            product) as int16, their sum corrected to exactly 32768 at the largest weight (the first in row-major order among equals).
 *            Pixel = clamp((sum w*p + 16384) >> 15, 0, 255); a tap outside the source reads the border value.
 *   crop     has_crop: the insize x insize window whose first pixel is (off_x, off_y) of the rotated image; outside it the image is 127
 *            (uint8(127.5), :137) and the mask 0.  Only the window is computed; the rotated image as a whole never exists.  Window pixels
 *            outside the rotated image are 127, rotated-image pixels outside the source 128: the reference's seam, kept.
 *   distort  has_distort: BGR -> HSV in integers (v = max, d = v - min, s = (d*sdiv[v] + 2048) >> 12 with sdiv[v] = rint(255*4096/v);
 *            h = g-b | b-r+2d | r-g+4d tested in the order v == r, v == g, else, then (h*hdiv[d] + 2048) >> 12 with hdiv[d] =
 *            rint(180*4096/(6d)), + 180 if negative; both tables 0 at 0), delta[0..2] added to h, s, v, each clamped to 0 .. 255 (the hue is
 *            clamped, not wrapped, :167; a hue >= 180 then counts modulo 180), HSV -> BGR by the float32 six-sector formula
 *            (h*(6/180), s/255, v/255 as float32 products with the float32 constants), clamp(rint(x*255)).  |delta| <= 10, 40, 30.
 *   flip     the window mirrored left-right (:176-177)
 *   has_crop = 0: a VALIDATION sample -- only resize_data to insize x insize (:336); every other step must be off.
 * Then, for every sample, the 16 x 16 MORPH_DILATE of the mask (:340): out[y, x] = max in[y-8 .. y+7, x-8 .. x+7] inside the image.
 * Results stay on the device: batch x insize x insize x 3 uint8 BGR and the dilated mask batch x insize x insize (0 | 1), which
 * pmx_validate_samples hands to the label, forward and loss entries without a host round trip.
 * bgr: src_h x src_w x 3 uint8; mask: src_h x src_w uint8 (non-zero = ignored) or NULL; host pointers, or device pointers when on_device
 * (they must then stay valid until the stream has run the call).  Asynchronous; host arrays are read before the call returns.
 * The workspace (sources, resized intermediates, results) grows on demand up to PMX_SAMPLES_WORKSPACE_BYTES.
 * Errors (checked before anything is enqueued; the context stays usable): PMX_ERR_INVALID for null pointers, n <= 0, insize no positive
 * multiple of 8, non-positive sizes or sides above 16384, non-finite matrix entries, a singular matrix, colour offsets outside the ranges,
 * a validation sample with another step on; PMX_ERR_CAPACITY for n > max_batch, insize * insize > max_h * max_w, a workspace above the
 * budget; PMX_ERR_STATE on facenet / handnet contexts. */
#define PMX_SAMPLES_WORKSPACE_BYTES ((size_t)1 << 30)
typedef struct pmx_sample {
    const uint8_t* bgr;
    const uint8_t* mask;
    int32_t src_h, src_w;
    int32_t resized_w, resized_h;     /* 0, 0: no resize */
    int32_t has_rotate, rot_w, rot_h;
    int32_t has_crop, off_x, off_y;
    int32_t has_distort, delta[3];
    int32_t flip;
    double inv[6];
} pmx_sample;
int pmx_samples_prepare(pmx_ctx* ctx, const pmx_sample* samples, int n, int insize, int on_device);
/* device pointers of the prepared images and dilated masks (either may be NULL); valid until the next pmx_samples_prepare or pmx_destroy.
 * PMX_ERR_STATE without prepared samples.  Does not synchronise. */
int pmx_samples_device_ptrs(pmx_ctx* ctx, void** bgr_nhwc, void** mask);
/* parity accessor: the prepared images (n x insize x insize x 3) and dilated masks (n x insize x insize) -> host; either may be NULL; n and
 * insize as prepared (else PMX_ERR_INVALID).  Synchronises. */
int pmx_get_samples(pmx_ctx* ctx, uint8_t* bgr, uint8_t* mask, int n, int insize);
/* Validator.evaluate for the prepared samples: pmx_loss_set_poses (heat_sigma 7, paf_width 8: the reference's params) with the prepared
 * device mask, pmx_validate_batch on the prepared device images.  poses / n_people as pmx_loss_set_poses takes them, in the pixels of the
 * prepared samples; out13 as pmx_validate_batch.  PMX_ERR_STATE without prepared samples.  Synchronises. */
int pmx_validate_samples(pmx_ctx* ctx, const double* poses, const int* n_people, double* out13);

/* ---- ignore masks from COCO segmentations (csrc/pmx_masks.hip) ----------------------------------------------------------------------
 * gen_masks of the reference's gen_ignore_mask.py (:23-37) for a batch of images of any sizes in ONE launch: per image `mask_all` (the
 * union of every annotation's mask) and `mask_miss` (what the loss ignores: the PNG the reference saves), h x w bytes of 0 | 1 each,
 * row-major.  The contract is the package's own NumPy functions (coco.py: polygon_mask, rle_mask, masks_numpy), byte for byte.  It
 * restates annToMask of pycocotools' C part (rleFrPoly + rleMerge + rleDecode) from its published source; that library is no dependency,
 * and the restatement has NOT been compared with it.
 *   Polygon part (flat x0, y0, x1, y1, ... of k vertices) -> mask.  C `double` and C `int` arithmetic, every operation rounded on its
 *   own, (int) truncating toward zero:
 *     1. X[j] = (int)(5 * x[j] + .5), Y[j] alike; closed: X[k] = X[0], Y[k] = Y[0].
 *     2. Every edge j -> j + 1 is traced into a dense point list.  dx = |xe - xs|, dy = |ys - ye|, flip = (dx >= dy && xs > xe) ||
 *        (dx < dy && ys > ye); with flip the end points are swapped.  dx >= dy: s = (double)(ye - ys) / dx, and for d = 0 .. dx,
 *        t = flip ? dx - d : d, the point (u, v) = (t + xs, (int)(ys + s * t + .5)).  Else s = (double)(xe - xs) / dy, and for d = 0 .. dy,
 *        t = flip ? dy - d : d, the point ((int)(xs + s * t + .5), t + ys).  The lists of all edges concatenate in order.  A zero-length
 *        edge gives its vertex once (0 / 0 is not evaluated).
 *     3. Every consecutive pair p - 1, p of the list with u[p] != u[p-1] gives a candidate: m = u[p] < u[p-1] ? u[p] : u[p] - 1,
 *        xd = (m + .5) / 5 - .5, kept when xd is an integer with 0 <= xd <= w - 1; yd = (min(v[p], v[p-1]) + .5) / 5 - .5 clamped to
 *        [0, h], then ceil.  The crossing point is (xd, yd).
 *     4. Pixel (x, y) is 1 iff the number of crossing points of column x with yd <= y is odd (points with yd == h close a run at the
 *        column's end; the count of a column is even).
 *   Run-length part: counts of runs of 0 and 1 in turn, starting with 0, over the column-major index x * h + y.
 *   An annotation's mask is the union of its parts.  Per image, in part order and with `all` as it was before the annotation:
 *   class 2 (crowd): miss |= mask & ~all;  class 1 (too few key points / too small): miss |= mask;  class 0: nothing;  then all |= mask.
 * images: per image its size and its range of `parts`; the parts of one annotation (same `ann`) are consecutive and share `cls`; a part's
 * (off, len) index `xy` (kind 0: len doubles) or `counts` (kind 1: len counts).  All tables are host memory, read before the call returns;
 * they travel in ONE staging copy (at most PMX_MASKS_TABLE_BYTES).  mask_miss / mask_all: the masks end to end in image order (h * w bytes
 * each); either may be NULL; host memory (one synchronisation behind the copies), or device memory on the context's device
 * (out_on_device != 0: asynchronous on the context's stream, nothing synchronises).  Works on a context of any architecture and needs no
 * weights; maps, records, samples and retained state stay untouched.
 * Errors, before anything is enqueued (the context stays usable): PMX_ERR_INVALID for a null table, n_images <= 0, both outputs NULL, a
 * side < 1 or > 16384, a part range outside the table, an unknown kind or class, annotation indices that go back or one annotation with
 * two classes, an (off, len) outside its array, a polygon of fewer than 6 numbers or an odd count, a coordinate that is not finite or
 * outside +-65536, counts that do not sum to h * w; PMX_ERR_CAPACITY for tables above the budget. */
#define PMX_MASKS_TABLE_BYTES ((size_t)64 << 20)
typedef struct pmx_mask_image { int32_t h, w, part0, n_parts; } pmx_mask_image;
typedef struct pmx_mask_part { int32_t kind /* 0 polygon, 1 run-length */, ann, cls /* 0 keep, 1 miss, 2 crowd */, off, len, reserved; } pmx_mask_part;
int pmx_coco_masks(pmx_ctx* ctx, const pmx_mask_image* images, int n_images, const pmx_mask_part* parts, int n_parts, const double* xy,
                   size_t n_xy, const uint32_t* counts, size_t n_counts, uint8_t* mask_miss, uint8_t* mask_all, int out_on_device);
/* the columns one block of pmx_coco_masks owns for an image of height h (1 .. 16384, else 0): a launch-geometry fact for tests */
int pmx_coco_masks_strip(int h);

/* ---- COCO key-point evaluation: OKS and matching (csrc/pmx_eval.hip) ------------------------------------------------------------------
 * evaluateImg + computeOks of COCOeval with iouType = 'keypoints', for a batch of images with any mix of detection and ground-truth
 * counts in ONE launch, one block per image; the accumulation over images (precision / recall, AP / AR) stays on the host.  The contract
 * is the package's own NumPy functions (coco.py: oks_matrix, evaluate_image): the tables are equal, the OKS values equal up to the exp
 * of the two sides (about one ulp per term, at most 17 terms <= 1: below 1e-14 absolute).  It restates the published source of
 * pycocotools; that library is no dependency and the restatement has NOT been compared with it.
 *   Detections of an image: n people, each a score and 18 rows (x, y, v).  COCO key point i is row consts->joint[i]; it is (x, y) where
 *   v != 0, else (0, 0).  They are ranked by descending score, equal scores in input order (argsort(-score, kind='mergesort')), and
 *   cut to the first PMX_EVAL_MAX_DETS = 20: D = min(n, 20).  area = (max x - min x) * (max y - min y) over all 17 points, zeros
 *   included (loadRes).
 *   Ground truths of an image: G annotations in file order; ignore = iscrowd == 1 || num_keypoints == 0.
 *   OKS of (detection d, ground truth g), fp64, every operation rounded on its own: k1 = count(vg > 0).  k1 > 0: dx = xd - xg,
 *   dy = yd - yg.  Else, bb = bbox: x0 = bb[0] - bb[2], x1 = bb[0] + bb[2] * 2, y0 = bb[1] - bb[3], y1 = bb[1] + bb[3] * 2,
 *   dx = max(0, x0 - xd) + max(0, xd - x1), dy alike.  e_i = (dx * dx + dy * dy) / vars[i] / (area_g + eps) / 2, left to right.
 *   oks = (exp(-e_i) added in ascending i, over the i with vg > 0 if k1 > 0, else over all 17) / (number of terms).
 *   Matching, independently for each area range a = 0 .. 2 ([lo, hi] = area_rngs[a]) and threshold t = 0 .. 9 (the 30 walks run side
 *   by side): gt_ig[g] = ignore[g] || area_g < lo || area_g > hi; the ground truths are visited kept ones first, file order within
 *   each group.  For each detection in rank order: iou = min(iou_thrs[t], 1 - 1e-10), m = -1; walk the ground truths: one already
 *   matched in this walk that is not crowd (iscrowd != 1) is skipped; if m > -1 && !gt_ig[m] && gt_ig[g] the walk stops; if
 *   oks[d][g] < iou it is skipped; else iou = oks[d][g], m = g (an equal later value replaces an earlier one).  With a match:
 *   dt_match = m (file-order index), dt_ig = gt_ig[m], m is marked.  Afterwards dt_ig |= dt_match == -1 && (area_d < lo || area_d > hi).
 * Inputs, all host memory, read before the call returns; they travel in ONE staging copy of at most PMX_EVAL_TABLE_BYTES:
 *   images[n_images]: per image its range (gt0, n_gt) of gts[n_gts]; consts: the constant tables as the host computed them.
 *   Detections, form 1 (poses != NULL): poses[sum n][18][3] and scores[sum n] end to end in image order, n_people[n_images].
 *   Form 2 (poses == NULL; scores, n_people ignored): the first n_images result records of the last post-process are read WHERE THEY LIE
 *   on the device -- the call finalises them as pmx_results_layout does (synchronises; grows and re-runs if an image overflowed);
 *   PMX_ERR_STATE before any post-process and when n_images exceeds the records' batch.  detect -> evaluate moves no pose to the host.
 * Outputs, host memory, each may be NULL but not all; one synchronisation behind the copies.  Unused slots hold -1 (det_order,
 * dt_match) or 0:
 *   det_count[n_images] = D; det_order[n_images][20]: index of the ranked detection among the image's people; det_scores, det_areas
 *   [n_images][20]; dt_match int32 and dt_ig bytes [n_images][3][10][20]; gt_ig: per image n_gt x 3 bytes (row g, column a); oks:
 *   per image 20 x n_gt doubles (row d, column g, rows from D on are 0); both with the images end to end: image k starts at 3 * s and
 *   20 * s, s = the sum of n_gt of the images before it.
 * PMX_EVAL_MAX_GT bounds the ground truths of ONE image: its working set lives in LDS (160 KB per block).  Per ground truth: 20 OKS
 * doubles (160 bytes), its area (8), its place in the three visiting orders (3 x 2), gt_ig of the three ranges (3), the crowd flag (1) and
 * the matched flags of the 30 walks (30): 208 bytes; per image 20 x 17 detection points, scores, areas, order: about 6 KB.  512 x 208 + 6 K =
 * 110 KB fits, 768 x 208 + 6 K = 162 KB does not; 512 is the largest power of two.
 * Works on a context of any architecture and needs no weights; maps, records, samples and retained state stay untouched; runs on the
 * context's stream.  No atomics: two calls give the same bytes.
 * Errors, before anything is enqueued (the context stays usable): PMX_ERR_INVALID for a null table or consts, n_images <= 0, all outputs
 * NULL, a negative count, a range outside gts, form 1 without scores or n_people, a coordinate, area, box or score that is not finite,
 * consts that are not finite or a joint outside 0 .. 17; PMX_ERR_CAPACITY for an image with more than PMX_EVAL_MAX_GT ground truths and for
 * tables above the budget. */
#define PMX_EVAL_MAX_GT 512
#define PMX_EVAL_MAX_DETS 20
#define PMX_EVAL_KEYPOINTS 17
#define PMX_EVAL_TABLE_BYTES ((size_t)64 << 20)
typedef struct pmx_eval_image { int32_t gt0, n_gt; } pmx_eval_image;
typedef struct pmx_eval_gt { double keypoints[PMX_EVAL_KEYPOINTS][3]; double area; double bbox[4]; int32_t iscrowd, num_keypoints; } pmx_eval_gt;
typedef struct pmx_eval_consts { double vars[PMX_EVAL_KEYPOINTS]; double iou_thrs[10]; double area_rngs[3][2]; double eps; int32_t joint[PMX_EVAL_KEYPOINTS]; int32_t reserved; } pmx_eval_consts;
int pmx_coco_eval(pmx_ctx* ctx, const pmx_eval_image* images, int n_images, const pmx_eval_gt* gts, int n_gts, const pmx_eval_consts* consts,
                  const double* poses, const double* scores, const int32_t* n_people, int32_t* det_count, int32_t* det_order,
                  double* det_scores, double* det_areas, int32_t* dt_match, uint8_t* dt_ig, uint8_t* gt_ig, double* oks);

/* results.  pmx_results_layout synchronises, grows the capacities and re-runs the post-process if an image overflowed them,
 * and returns the layout of the (now final) records; pmx_get_results does the same and copies `batch` records to `out`
 * (out_bytes >= batch * bytes_per_record, else PMX_ERR_CAPACITY). */
int pmx_results_layout(pmx_ctx* ctx, int* people_cap, size_t* bytes_per_record);
int pmx_get_results(pmx_ctx* ctx, int batch, void* out, size_t out_bytes);
/* device pointer of the record array (for RCCL gathers): synchronises and finalises the records like pmx_results_layout (PMX_ERR_STATE
 * before any post-process); valid until the next post-process, capacity change or pmx_destroy */
int pmx_results_device_ptr(pmx_ctx* ctx, void** dev_ptr, size_t* bytes_per_record);
/* pipelined consumers (a multi-GPU gather that runs one step behind the compute): pmx_results_snapshot enqueues, stream-ordered after
 * the last post-process and WITHOUT synchronising, a device-to-device copy of its `batch` records to dst_device (>= batch *
 * bytes_per_record at the context's current layout, else PMX_ERR_CAPACITY) plus a copy of the per-image status words to pinned host
 * memory, and marks the point with the event of `slot` (0 .. PMX_SNAPSHOT_SLOTS - 1: a consumer that runs d steps behind needs d + 1).  The caller
 * may then enqueue the next pmx_detect_batch.
 * pmx_snapshot_wait blocks until slot's copies are done (not until the stream is idle) and returns the layout the snapshot was
 * taken at and the OR of the status words: if it carries a capacity bit (PMX_IMG_*_OVERFLOW) the snapshot is NOT final -- run the
 * step again and fetch it through pmx_results_layout / pmx_get_results, which grow the capacities (docs: INTEGRATION.md). */
#define PMX_SNAPSHOT_SLOTS 4
int pmx_results_snapshot(pmx_ctx* ctx, int slot, void* dst_device, size_t dst_bytes);
int pmx_snapshot_wait(pmx_ctx* ctx, int slot, int* batch, int* people_cap, size_t* bytes_per_record, int* status_or);
/* capacities: pre-size a context for crowds (or shrink them in tests to exercise the growth path); 0 keeps a value.
 * candidates: 0 = accepted candidates of a limb are kept in LDS (4096 slots), > 0 = that many slots in device memory.
 * people <= subsets, every value <= 2^20 (candidates <= 2^24), else PMX_ERR_INVALID; if the device cannot hold the new buffers the
 * call fails with PMX_ERR_HIP and the context keeps its previous buffers and capacities. */
int pmx_set_capacities(pmx_ctx* ctx, int peaks_per_joint, int subsets, int people, int candidates);
int pmx_get_capacities(pmx_ctx* ctx, int* peaks_per_joint, int* subsets, int* people, int* candidates);

/* parity accessors for one image of the last post-process (host copies; synchronise).
 * peaks: rows (type, x, y, score, id) float64 = all_peaks (pose_detector.py:76,110), BEFORE the rescale;
 * conns: rows (limb, id_a, id_b, score) = all_connections (:161-181) flattened in limb order;
 * subsets: rows of 20 float64 after the final filter (:248-249).
 * n_rows is always set; PMX_ERR_CAPACITY if it exceeds cap_rows (call again with a larger buffer). */
int pmx_get_peaks(pmx_ctx* ctx, int image, double* peaks5, int cap_rows, int* n_rows);
int pmx_get_connections(pmx_ctx* ctx, int image, double* conns4, int cap_rows, int* n_rows);
int pmx_get_subsets(pmx_ctx* ctx, int image, double* subsets20, int cap_rows, int* n_rows);
/* smoothed heat map (gaussian_filter output, pose_detector.py:86) of one image/joint: only produced when
 * option "keep_smoothed" is 1; float32 map_h x map_w. */
int pmx_get_smoothed(pmx_ctx* ctx, int image, int joint, float* out, int map_h, int map_w);

/* ---- measurement ------------------------------------------------------------------------------
 * HIP-event timing on the stream the kernels are launched on. */
int pmx_timer_start(pmx_ctx* ctx);
int pmx_timer_stop(pmx_ctx* ctx, double* ms);          /* synchronises */
int pmx_profile_enable(pmx_ctx* ctx, int on);          /* 1: event pairs around every kernel launch; 2: only around the 7x7
                                                          convolutions (the dominant kernel; fewest events inside a timed region) */
int pmx_profile_reset(pmx_ctx* ctx);
int pmx_profile_count(pmx_ctx* ctx, int* n);
int pmx_profile_entry(pmx_ctx* ctx, int i, char* name, int name_cap, double* total_ms,
                      int64_t* launches, double* flop_per_launch, double* bytes_per_launch);
/* FLOP per launch the entry's kernel ISSUES to the matrix cores for real outputs: the algorithmic figure for the direct kernels,
 * 16/36 (3x3) or 100/196 (7x7) of it for the Winograd forms -- the numerator of a roofline fraction that cannot exceed 1 */
int pmx_profile_issued(pmx_ctx* ctx, int i, double* issued_flop_per_launch);

/* ---- kernel unit-test entry (T0): one convolution layer through the product kernels -----------
 * x: float32 NCHW host (B, cin, h, w); w: OIHW; y: NCHW host (B, cout, h', w') with h' = h/2 if pool.
 * Semantics = L.Convolution2D(ksize, stride 1, pad ksize/2) [+ F.relu] [+ F.max_pooling_2d(2, 2)]. */
int pmx_conv2d(pmx_ctx* ctx, const float* x_nchw, const float* w_oihw, const float* bias,
               int batch, int cin, int h, int w, int cout, int ksize, int relu, int pool,
               float* y_nchw, int iters, double* avg_ms);

/* ---- kernel unit-test entry: two layers as the two groups of one launch ---------------------------
 * pmx_conv2d for two layers of equal ksize and cin whose output channels pad to the same count (both <= 64, or the same multiple of 128;
 * cout0 and cout1 themselves may differ), planned as ONE launch of two groups under the context's options -- the form the PAF / heat-map
 * branches of the network run in.  On the device the inputs are channel slices of one NHWC buffer and the outputs channel slices of
 * another, each with a channel stride larger than a group's own channels, as the branches' buffers are; the output buffer is poisoned
 * (all bits set) first.  x1 null: both groups read x0.  Host pointers; x (B, cin, h, w), w OIHW, y0 (B, cout0, h', w'), y1 (B, cout1, h',
 * w'); not timed.  PMX_ERR_INVALID for a null pointer, a ksize outside {1, 3, 7}, a non-positive shape, pool with odd h or w, or output
 * channel counts that pad differently. */
int pmx_conv2d_pair(pmx_ctx* ctx, const float* x0_nchw, const float* x1_nchw, const float* w0_oihw, const float* bias0, int cout0,
                    const float* w1_oihw, const float* bias1, int cout1, int batch, int cin, int h, int w, int ksize, int relu, int pool,
                    float* y0_nchw, float* y1_nchw);

/* ---- the backward twin of pmx_conv2d: the gradients of one convolution layer ---------------------
 * Host pointers, float32, the layouts of pmx_conv2d: x (B, cin, h, w), w OIHW, dy (B, cout, h', w') with h' = h/2, w' = w/2 if pool.
 * Semantics = Chainer's backward of L.Convolution2D(ksize, 1, ksize/2) [+ F.relu] [+ F.max_pooling_2d(2, 2)].  fp32 only.
 *   z    z = conv(x, w) + bias, computed by ONE plan of the dispatcher with relu = 0, pool = 0 under the context's options; returned in
 *        z_nchw (B, cout, h, w) when that pointer is given.  a = relu ? max(z, 0) : z.
 *   g    the gradient at the convolution's output, (B, cout, h, w).  Without pool g = dy.  With pool, dy[n,c,i,j] goes to the FIRST position
 *        of the window (2i+di, 2j+dj), in the order (0,0), (0,1), (1,0), (1,1), whose a equals the window's maximum; the other three get 0
 *        (the first-argmax of Chainer and torch).  With relu, g is then zeroed where z > 0 is false (strict, as in gy * (y > 0)).
 *   dx   (B, cin, h, w): the dispatcher run on g with the packed layer w'[ci][co][ky][kx] = w[co][ci][ks-1-ky][ks-1-kx], no bias, no ReLU,
 *        no pool.  It takes whatever form the options select for that layer shape, as pmx_conv2d would.
 *   dw   OIHW: dw[co][ci][ky][kx] = sum over (n, y, x) of g[n,co,y,x] * x[n,ci,y+ky-p,x+kx-p], p = ksize/2, out-of-image taps as zeros.
 *        One launch of the weight-gradient kernel (csrc/conv_bwd.hip, v_mfma_f32_32x32x2_f32) + one combine launch.  The B*h image rows are
 *        cut into S strips of R = ceil(B*h / S0) consecutive rows (S0 = option "wgrad_strips" if > 0, else as many as fill the device;
 *        S0 <= PMX_WGRAD_MAX_STRIPS and <= B*h; S = ceil(B*h / R)); every strip writes its partial sums to its own slot of a workspace of
 *        S * round_up(cout, 32) * round_up(cin, 32) * ksize^2 floats, i.e. at most PMX_WGRAD_MAX_STRIPS * 4 * round_up(cout, 32) *
 *        round_up(cin, 32) * ksize^2 bytes (302 MB for a 512 -> 512 3x3 layer, 103 MB for 128 -> 128 7x7).  No floating-point atomics.
 *        THE ORDER, per (co, ci, ky, kx), is that of this host twin (tests/conv_wgrad_twin.c), bit for bit, whatever the options:
 *            for strip s = 0 .. S-1:  acc = +0;  for every pixel (n, y, x) of the strip's rows in row-major order:
 *                                         acc = fmaf(g[n,co,y,x], tap inside the image ? x[n,ci,y+ky-p,x+kx-p] : 0, acc);
 *                                     if the strip has an odd number of pixels: acc = fmaf(0, 0, acc);      (the MFMA's second K slot)
 *                                     part[s] = acc;
 *            dw = part[0];  for s = 1 .. S-1: dw = dw + part[s];                                            (float32 adds, left to right)
 *   db   db[co] = sum over (n, y, x) of g[n,co,y,x]: float64 sums in fixed slots added in slot order, cast to float32.
 * Option "grad_precision" = 2 (default 0: everything above): dw and dx of a 3x3 / 7x7 layer with f16 operands and fp32 sums.  z is still
 * computed under the context's own options in fp32, the mask and db do not change: z, g and db keep every bit, and so does all of a 1x1
 * layer.  f16(v) is csrc/f16_round.h::f16_rn_sat: round to nearest even, saturating at +-65504, subnormals and NaN kept.
 *   dw   dw[co][ci][ky][kx] = sum over (n, y, x) of f16(g[n,co,y,x]) * f16(x[n,ci,y+ky-p,x+kx-p]), out-of-image taps as zeros.  Every product
 *        is exact in fp32; the products are summed in fp32 in a fixed order.  One launch of conv_wgrad_f16_kernel
 *        (csrc/conv_wgrad_f16.hip, v_mfma_f32_32x32x16_f16; g and x are rounded while they are staged, no f16 copy of an activation is
 *        written) + the combine launch of the fp32 path.  THE GROUPS: every image row of w pixels is cut into ceil(w / 16) groups of 16
 *        consecutive pixels; the last group of a row is padded with zero operands (a group never crosses a row, so a tap shift is one
 *        uniform pixel offset).  THE STRIPS: the B*h image rows are cut into S strips of R = ceil(B*h / S0) consecutive rows, S0 =
 *        option "wgrad_strips" if > 0, else ceil(4096 / (4 * blocks)) with blocks = ceil(round_up(cout, 32) / 128) * ksize *
 *        ceil(round_up(cin, 32) / (ksize == 7 ? 32 : 64)), the blocks of four waves one strip takes; S0 <= PMX_WGRAD_MAX_STRIPS and
 *        <= B*h; S = ceil(B*h / R) (csrc/wgrad_strips.h: pmx_wgrad_f16_strips; the workspace is the fp32 path's).  THE ORDER, per
 *        (co, ci, ky, kx): within a strip one MFMA per group adds the group's 16 products to the accumulator, the groups of a row left to
 *        right, the rows top to bottom; each strip's accumulator goes to its own workspace slot and the slots are added left to right
 *        in float32.  The order of the 16 products inside one MFMA belongs to the hardware, so there is no bit-exact host twin for
 *        arbitrary inputs: |dw - the float64 sum of the same products| <= (16 + R * ceil(w / 16) + S) * 2^-23 * sum |f16(g) * f16(x)|,
 *        and inputs on which every partial sum is exact give the exact result (tests/f16_grad_emulation.py).  No atomics: the same
 *        bits on every run and under every forward option.
 *        Non-finite operands: f16() saturates, so an infinity in g or x enters the sums as +-65504 and dw stays finite (db, a float64
 *        sum of the unrounded g, does not).  A NaN in g[., co, ., .] (in x[., ci, ., .]) makes NaN every dw[co][.][.][.] (every
 *        dw[.][ci][.][.]) whose sum holds it, and leaves every other co (ci) untouched.  Pad pixels and out-of-image taps are ZERO
 *        OPERANDS, not skipped products, and 0 * NaN = NaN: for a NaN at a pixel closer than p to the image border, or to the pad
 *        pixels of a row's last group, the elements of the same co (ci) whose exact sum pairs it with an out-of-image tap or a pad
 *        pixel are NaN as well.
 *   dx   the f16 form of the dispatcher (the f16 inference contract above, applied to (g, w')): ONE conv_f16_kernel launch on the f16 pack
 *        of the transposed layer, which rounds g while staging; option "f16_bn" applies as to a forward, with the same bits either way.
 * Loss scaling is deliberately not part of any kernel: everything after the mask is linear in dy and the masks do not depend on dy, so a
 * caller whose gradients would fall below the f16 range scales dy by 2^k and un-scales dx, dw and db by 2^-k (exact in fp32).  The chains
 * get their dy from the loss gradients, so there the scale is option "loss_scale_log2": 2^k enters on the host, in the two constants the
 * loss-gradient kernel is handed, and pmx_get_loss_grads, pmx_get_layer_grad, pmx_get_trunk_grad and pmx_get_retained(name, 1) return the
 * stored, scaled values.
 * Each of dx, dw, db, z may be NULL; a NULL output's work is skipped (z is still computed when relu or pool need it).  avg_ms3 may be NULL;
 * with iters > 0 it receives the mean time over `iters` repetitions of [0] the data-gradient plan, [1] the weight-gradient launches
 * (combine included), [2] the mask + bias-gradient launches, each timed on its own between two events (0 for a part that was skipped).
 * Errors, checked before anything is enqueued (the context stays usable): PMX_ERR_INVALID for a null x, w or dy, for all four outputs NULL,
 * for ksize outside {1, 3, 7}, for a non-positive shape or pool with odd h or w; PMX_ERR_STATE when option "precision" is not 0 (the f16
 * and bf16x3 modes are inference modes), whatever "grad_precision" is.  Option "wgrad_strips" (0 = automatic) exists for the tests: it only moves the strip borders. */
#define PMX_WGRAD_MAX_STRIPS 32
int pmx_conv2d_backward(pmx_ctx* ctx, const float* x_nchw, const float* w_oihw, const float* bias, const float* dy_nchw,
                        int batch, int cin, int h, int w, int cout, int ksize, int relu, int pool,
                        float* dx_nchw, float* dw_oihw, float* db, float* z_nchw, int iters, double* avg_ms3);

/* ---- head backward: the gradients of the 82 layers after conv4_2 ------------------------------------
 * conv4_3_CPM, conv4_4_CPM, the ten layers of stage 1 and the seventy of stages 2 - 6: the layers the reference updates while conv1_1 ..
 * conv4_2 are frozen (train_coco_pose_estimation.py:219-225).  All live at h/8 x w/8.  posenet contexts, uniform batches, fp32.
 *
 * pmx_backward_enable(on != 0; on = 2: the trunk as well, see "trunk backward" below) allocates, for max_batch images of max_h x max_w (PMX_ERR_CAPACITY if the device refuses; about 3 GB of
 * activations at 32 x 368 x 368, as much again for the gradients), and from then on a uniform fp32 forward that runs with the loss hook AND
 * the loss gradients on RETAINS what the backward reads: the post-ReLU output of each of the 82 layers and conv4_2's output, NHWC, written
 * by the layers' own launches into the store (never copied afterwards), with two exceptions --
 *   the feature map     conv4_4_CPM's output stays where every stage reads it, in channels 0 .. 127 of the concat buffer;
 *   the stage outputs   every stage overwrites the PAF / heat slices of the concat buffer, so after each stage's loss launch one launch copies
 *                       the 64 channels [38 PAF, 2 zeros | 19 heat, 5 zeros] to the store (the 57 channels per stage; the backward copies
 *                       them back before the weight gradient of Mconv1_stage{s+1} reads the buffer, and the last stage's at its end, so the
 *                       current maps stay those of the forward).
 * The two 1x1 layers that end a stage run as two launches while retaining (the fused launch does not store the middle activation); the
 * maps, the losses and the loss gradients keep their bits.  With retention off nothing more is launched or allocated.  A ReLU gate is read
 * from the stored output: a > 0 exactly when z > 0.
 *
 * pmx_backward_head enqueues the backward of the last retained forward on the context's stream, in reverse layer order, for the stages
 * that forward ran (option "stop_stage").  Per layer, with u the gradient at its output:
 *   g    = u where a > 0, +0.0f elsewhere (Mconv7_* and conv5_5_CPM_*: no ReLU, g = u); kept, one slot per layer
 *   db   as pmx_conv2d_backward
 *   dw   as pmx_conv2d_backward (the same kernel, the same order per element, strips cut from the batch * h/8 image rows; option
 *        "wgrad_strips"), OIHW; for Mconv1_* in the REFERENCE's input order 38 PAF, 19 heat, 128 feature
 *   dx   the dispatcher on g with the transposed, 180-degree-rotated pack (built by the device packers on the first backward, kept per layer, dropped
 *        by pmx_set_layer), two branches per launch where the forward has two; the packs of Mconv1_* write concat-buffer order, zeros in
 *        the pad channels
 * THE SUMS.  Every step is one float32 add, left to right:
 *   stage output   u(stage s PAF | heat) = loss_grad[s] + dx(Mconv1_stage{s+1}_L1) + dx(Mconv1_stage{s+1}_L2); the last stage run: loss_grad alone
 *   feature map    u(conv4_4_CPM) = the contributions in the order the backward produces them: Mconv1_stage6_L1, Mconv1_stage6_L2,
 *                  Mconv1_stage5_L1, ..., Mconv1_stage2_L2, conv5_1_CPM_L1, conv5_1_CPM_L2 (the stages that ran), starting from the first
 *   elsewhere      u = dx of the one layer that reads the output
 * No floating-point atomics: every run gives the same bits.  The chain ends with dx of conv4_3_CPM, the gradient at conv4_2's output,
 * where a trunk backward would start (pmx_get_trunk_grad).  Asynchronous.
 * Option "grad_precision" = 2: the 58 layers of the head with ksize > 1 -- conv4_3_CPM, conv4_4_CPM, conv5_1..3_CPM_*, Mconv1..5_stage*_* --
 * take dw and dx with f16 operands and fp32 sums, by the contract of pmx_conv2d_backward's f16 paragraph:
 *   dw   conv_wgrad_f16_kernel + the combine, on the same slices of the stores the fp32 kernel reads (g and x are rounded while they are
 *        staged; Mconv1_* through the same channel map).  Groups of 16 pixels per map row of w/8 pixels, the batch * h/8 map rows cut into
 *        strips by the f16 rule (option "wgrad_strips"), the bound (16 + R * ceil((w/8) / 16) + S) * 2^-23 * sum |f16(g) * f16(x)|.
 *   dx   the dispatcher's f16 form on the f16 pack of the transposed layer (built with the transposed pack, kept per layer, dropped by
 *        pmx_set_layer): one conv_f16_kernel launch per layer pair, whatever "conv_algo" and the batch are.
 * The 24 1x1 layers (dw and dx), every db, every mask, the sums above and the copies keep their launches and, given the same inputs, their bits;
 * the retained forward, the losses and the loss gradients do not depend on the option.  No atomics here either: the same bits on every
 * run.  Gradients below the f16 range are flushed while staged (f16_rn_sat): option "loss_scale_log2" moves them into it, and
 * pmx_backward_g_census counts what a given scale leaves outside.
 * PMX_ERR_STATE, before anything is enqueued: no retained forward yet, a forward since then that was not retained (any forward without
 * retention, the hook or the loss gradients), option "precision" != 0, a facenet / handnet context. */
int pmx_backward_enable(pmx_ctx* ctx, int on);
int pmx_backward_head(pmx_ctx* ctx);
/* dw (OIHW, the layer's shape as in pmx_set_layer) and db (cout) of one of the 82 layers after the last pmx_backward_head; either pointer
 * may be NULL (both: PMX_ERR_INVALID).  PMX_ERR_INVALID for an unknown name or a trunk layer, PMX_ERR_STATE without a backward and for a
 * layer of a stage that "stop_stage" cut off.  Synchronises. */
int pmx_get_layer_grad(pmx_ctx* ctx, const char* name, float* dw_oihw, float* db);
/* the gradient at conv4_2's output, NCHW float32 batch x 512 x h/8 x w/8.  Synchronises. */
int pmx_get_trunk_grad(pmx_ctx* ctx, float* g_nchw);
/* parity accessor: which = 0: the retained output a of layer `name` (after a retained forward; `name` may be "conv4_2"), which = 1: its
 * masked gradient g (after pmx_backward_head; not for "conv4_2"); NCHW float32 batch x cout x h/8 x w/8.  Errors as pmx_get_layer_grad;
 * which outside {0, 1}: PMX_ERR_INVALID.  Synchronises. */
int pmx_get_retained(pmx_ctx* ctx, const char* name, int which, float* out_nchw);
/* The range census of one head layer's kept g (what pmx_get_retained(name, 1) returns), over the layer's cout channels: with
 * r = f16_rn_sat(g) (csrc/f16_round.h), counts[0] = elements with g != 0, [1] g != 0 and r == 0 (flushed), [2] 0 < |r| < 2^-14 (subnormal),
 * [3] |g| > 65504 (saturated; infinities included), [4] NaN.  One launch of its own on the context's stream -- a block reduction, then one
 * integer atomic add per block and counter, so the counts are the same on every run -- only on request, never inside the chain.  Head layers
 * only: PMX_ERR_INVALID for an unknown name, for "conv4_2" and for every other trunk layer (in mode 2 as well, where
 * pmx_get_retained(name, 1) takes them) and for a NULL counts; PMX_ERR_STATE without a retained forward, before pmx_backward_head has run
 * for it, with option "precision" != 0, and for a layer of a stage that "stop_stage" cut off.  Synchronises. */
int pmx_backward_g_census(pmx_ctx* ctx, const char* name, unsigned long long counts[5]);

/* ---- trunk backward: the gradients of conv1_1 .. conv4_2 -----------------------------------------------------------------------------
 * From iteration 2000 on the reference updates all 92 layers (train_coco_pose_estimation.py:96-101: enable_update on the ten trunk
 * layers).  This chain continues where pmx_backward_head stops: at the gradient at conv4_2's output.  posenet, uniform batches, fp32.
 *
 * RETENTION.  pmx_backward_enable(ctx, 2) allocates what pmx_backward_enable(ctx, 1) allocates plus the trunk's stores; value 1 (and any
 * other non-zero value) is the head alone, exactly as above -- its allocations, launches and bits, and the refusal of trunk names by the
 * accessors; 0 frees everything.  Asking for 2 while 1 is on, or for 1 while 2 is on, is PMX_ERR_STATE: switch retention off first.
 * PMX_ERR_CAPACITY, with the sizes in the message, if the device refuses.  With mode 2 on, under the conditions of the head (hook and loss
 * gradients on, uniform batch, fp32), the stem writes into the trunk store with the layers' own launches, nothing copied afterwards:
 *   conv1_1, conv1_2     two launches (neither fused conv1 kernel stores conv1_1's output); a uint8 input is preprocessed into the
 *                        16-float input buffer first, which nothing overwrites before the backward
 *   conv1_2, conv2_2,    run with pool = 0 and store their post-ReLU, PRE-pool output a; one launch of maxpool_nhwc_kernel each writes the
 *   conv3_4              pooled map the next layer reads.  A maximum of four floats is exact; the gate and the argmax are read from a alone:
 *                        a > 0 exactly when z > 0, and the first maximum of a = relu(z) is the first maximum F.max_pooling_2d(F.relu(z)) sees
 * Retained, NHWC at the layer's own channel count: a of conv1_1 .. conv4_1 (conv4_2's is the head's slot), the three pooled maps, the
 * prepared input (16 floats per pixel, where the forward holds it anyway).  With P = max_batch * max_h * max_w input pixels the store is
 *   (64 + 64 + 128/4 + 128/4 + 4 * 256/16 + 512/64 + 64/4 + 128/16 + 256/64) * P = 292 * P floats      5.06 GB at 32 x 368 x 368,
 * next to it the gradient pair u | g of 2 * 64 * P floats (2.22 GB; the widest layer, conv1_*; every other layer of the chain reuses the
 * pair) and the ten gradient segments (5.9 M floats).  Per-layer g slots are NOT kept: they would cost 272 * P floats (4.71 GB at
 * 32 x 368 x 368) for an accessor only the tests use.  Option "trunk_keep_g" = 1, read by pmx_backward_enable(ctx, 2), allocates them
 * instead of the shared g buffer, so that pmx_get_retained(name, 1) can return a trunk layer's g; it changes no arithmetic.
 * BITS.  A mode-2 forward takes other kernel forms in the stem than a non-retaining forward (unfused conv1, un-pooled launches + the pool
 * kernel), so its maps and losses are not promised to equal those of modes 0 / 1 bit for bit (INTEGRATION.md section 5 records what was
 * found); the backward differentiates the forward that ran.  Modes 0 and 1 keep their bits, launches and allocations.
 *
 * pmx_backward_trunk, asynchronous on the context's stream, after pmx_backward_head for the same retained forward, walks conv4_2 ..
 * conv1_1.  NO SUMS: every trunk output has exactly one consumer, so u of a layer is the dx of the layer after it (conv4_2: the head's
 * trunk gradient).  Per layer, at the layer's own resolution:
 *   g    un-pooled layers: u where a > 0, +0.0f elsewhere (the head's mask launch).  Pooled layers: u has the pooled size; it goes to the
 *        FIRST maximum of its 2 x 2 window of a, strictly greater in the order (0,0), (0,1), (1,0), (1,1) (pmx_conv2d_backward's rule), if
 *        that a > 0, and the other positions get +0.0f.  One thread writes the four elements of a window; no atomics.
 *   db   as pmx_conv2d_backward
 *   dw   conv1_2 .. conv4_2: as pmx_conv2d_backward -- the same kernel and order per element -- with a strip rule of its own: S0 as
 *        there (option "wgrad_strips" if > 0, else ceil(2048 / the layer's units of one wave each)), S0 <= PMX_WGRAD_TRUNK_MAX_STRIPS and
 *        <= batch * h, but R = FLOOR(batch * h / S0) rows per strip, S = ceil(batch * h / R), so that S0 <= S < 2 * S0.  pmx_conv2d_backward's
 *        R = ceil(...) gives S <= S0 and would leave conv1_2 (6 units; S0 = 342) with 335 strips = 2010 waves at 10 x 368 x 368; rounding R
 *        down gives every trunk layer its 2048 waves wherever batch * h >= S0.  The workspace is S * 9 * cout * cin floats: below 57 MB per layer where
 *        S = S0, below 114 MB at any size.  The head chain and pmx_conv2d_backward keep their rule, PMX_WGRAD_MAX_STRIPS and
 *        their bits.
 *        conv1_1: its own kernel (csrc/conv_bwd.hip: conv1_wgrad_kernel), which reads the input at its 16 floats per pixel: the 32 B
 *        columns of v_mfma_f32_32x32x2_f32 are the 27 (ci, ky, kx) of one co and 5 zeros; one wave per strip keeps both 32-co tiles.
 *        Its strip rule is the same with S0 = PMX_WGRAD_CONV1_STRIPS (or option "wgrad_strips"): at least 2048 waves whenever
 *        batch * h >= 2048; workspace S * 64 * 32 floats (< 33.6 MB).
 *        THE ORDER per element is the twin's of pmx_conv2d_backward (tests/conv_wgrad_twin.c with cin = 3 and the same (S, R)): fmaf over
 *        the strip's pixels in row-major order, the odd strip's closing fmaf(0, 0, acc), the strips added left to right.  No atomics.
 *        Option "wgrad_strips" forces S0 for all ten layers.
 *   dx   the dispatcher on g with the transposed, 180-degree-rotated pack, relu = 0, pool = 0 (conv1_1: none, and no pack is built)
 * The ten dw | db segments follow the head's in the gradient store, each padded to 64 floats; every head offset is as in mode 1, so
 * pmx_train_enable / pmx_train_step_head work in mode 2 as in mode 1 and update the 82 head layers only (their stores are as large as
 * the gradient store, so 3 x 23.5 MB larger); pmx_train_step updates all 92 layers (the training steps, below).
 * PMX_ERR_STATE, before anything is enqueued: mode is not 2, no retained forward, pmx_backward_head has not run for it, option "precision"
 * != 0, a facenet / handnet context.
 * With mode 2 on, pmx_get_layer_grad also takes the ten trunk names after pmx_backward_trunk (before: PMX_ERR_STATE; mode 1:
 * PMX_ERR_INVALID as ever), and pmx_get_retained takes them with which = 0: a (pre-pool) at the layer's own resolution; 1: g, after
 * pmx_backward_trunk and with "trunk_keep_g" (else PMX_ERR_STATE); 2: the pooled map of conv1_2 / conv2_2 / conv3_4 (any other layer:
 * PMX_ERR_INVALID); and the name "input" with which = 0: the prepared input, batch x 3 x h x w. */
#define PMX_WGRAD_TRUNK_MAX_STRIPS 512
#define PMX_WGRAD_CONV1_STRIPS 2048
int pmx_backward_trunk(pmx_ctx* ctx);
/* test entry: conv1_1's weight-gradient kernel on the caller's host arrays x (B, 3, h, w) and g (B, 64, h, w) -> dw (64, 3, 3, 3).
 * strips: S0 (0 = the rule); the S and R used come back in strips_out / rows_out (either may be NULL).  Synchronises. */
int pmx_conv1_wgrad(pmx_ctx* ctx, const float* x_nchw, const float* g_nchw, int batch, int h, int w, int strips, float* dw_oihw,
                    int* strips_out, int* rows_out);
/* test entry: the max-pool kernel and the pooled layers' g kernel on host arrays a (B, C, h, w; h, w even) and u (B, C, h/2, w/2) ->
 * pooled (B, C, h/2, w/2) and g (B, C, h, w).  Synchronises. */
int pmx_pool_backward_test(pmx_ctx* ctx, const float* a_nchw, const float* u_nchw, int batch, int channels, int h, int w, float* pooled_out,
                           float* g_out);

/* ---- training steps: Adam on the 82 layers after conv4_2 or on all 92, every weight pack rewritten on the device ----------------------
 * What the reference's optimizer.update() does: during its first 2000 iterations (train_coco_pose_estimation.py:219-225: Adam, conv1_1 ..
 * conv4_2 frozen, GradientScaling(conv4_3_CPM / conv4_4_CPM, 1/4)) pmx_train_step_head, applied to the gradient store pmx_backward_head
 * leaves; from iteration 2000 on (:96-101, enable_update on the ten trunk layers) pmx_train_step, applied to what pmx_backward_head and
 * pmx_backward_trunk leave.  The weights never leave the device.  posenet contexts, fp32 ("precision" 0).
 *
 * STORES.  pmx_train_enable(on != 0) needs pmx_backward_enable on and every layer's weights set (else PMX_ERR_STATE / PMX_ERR_WEIGHTS).  It
 * allocates three stores with the layout of the gradient store (per layer dw | db, every layer padded to a multiple of 64 floats; about
 * 3 x 186 MB): the master weights w (OIHW, the reference's input order), filled by un-pack launches from the layers' current device packs
 * (the context keeps no host copy), and Adam's moments m = v = 0; the step count t of every head layer becomes 0, its gradient scale 1, the
 * hyper-parameters alpha = 1e-4, beta1 = 0.9, beta2 = 0.999, eps = 1e-8 (Chainer's and the reference's).  PMX_ERR_CAPACITY if the device
 * refuses; the context stays usable.  on = 0 frees the stores (so does pmx_backward_enable(0)).  With training off nothing is allocated or
 * launched that was not before.  While training is on, pmx_set_layer on a head layer also rewrites that layer's master weights (m, v, t stay).
 * With pmx_backward_enable(ctx, 2) the ten trunk layers conv1_1 .. conv4_2 have all of this too -- master weights, moments, t, scale, the
 * pmx_set_layer rule -- in the ten segments that follow the head's; pmx_train_set_grad_scale / pmx_train_get_state / pmx_train_set_state
 * then take their names.
 *
 * THE CONTRACT of one parameter, this project's own restatement of Chainer's AdamRule with eta = 1 and weight_decay_rate = 0.  Every line is
 * ONE float32 operation rounded to nearest, sqrt and / correctly rounded, nothing fused:
 *     g = grad * scale
 *     d = g - m;   m = m + omb1 * d                 omb1 = (float)(1 - beta1)
 *     q = g * g;   e = q - v;   v = v + omb2 * e    omb2 = (float)(1 - beta2)
 *     s = sqrtf(v) + eps                            eps  = (float)eps
 *     w = w - (alpha_t * m) / s                     alpha_t = (float)(alpha * sqrt(1 - beta2^t) / (1 - beta1^t)), in double on the host
 * t is the LAYER's own step count after the increment; scale, alpha_t and t are per layer.  A CUDA build of Chainer may contract a multiply
 * and an add into one FMA, so bit equality with Chainer is not claimed; tests/adam_twin.py restates the lines in NumPy and is matched bit
 * for bit.  Pad floats between layers are neither used as parameters nor changed.
 *
 * pmx_train_step_head, asynchronous on the context's stream, after pmx_backward_head for the retained forward:
 *   1. t += 1 for the layers that received a gradient: those of the stages the retained forward ran.  Layers of stages that "stop_stage" cut
 *      off keep their weights, packs, moments and t (this project's rule: a parameter without a gradient is not updated);
 *   2. Adam over all those layers in ONE launch (a per-segment table, sent through pinned memory; the call waits only if the previous
 *      step's table copy has not finished);
 *   3. the packers: every pack of an updated layer that EXISTS is rewritten in place, same pointer, with the bits a one-off build gives
 *      from the same OIHW weights (csrc/pack_index.h defines every float of every pack) -- the direct pack and bias (pmx_set_layer),
 *      the Winograd pack, the f16 and bf16x3 packs, the transposed 180-degree-rotated pack of the data gradient, its Winograd pack
 *      and its f16 pack (pmx_get_transposed_f16_pack; it exists once a head backward ran under "grad_precision" 2).  A pack that
 *      does not exist is not created: its lazy builder makes it on first use from the then-current direct pack, after waiting for
 *      the stream.  ONE launch per kind of pack serves all updated layers (direct + bias, transposed, f16 of both, bf16x3, Winograd
 *      of both, conv1_1's fused-kernel pack, in this order: a derived pack after the pack it reads): six launches at most, driven
 *      by per-layer tables that travel with Adam's in the same pinned copy.
 * Under a loss scale ("loss_scale_log2" = k) the gradient store holds 2^k times the gradients; Adam's kernel and contract do not change:
 * the caller sets every layer's scale to scale * 2^-k, which is exact, and line one of the contract, g = grad * scale, un-scales.
 * No host synchronisation, no host <-> device copy but the table.  The step CONSUMES the gradients: a second step without a new retained
 * forward + pmx_backward_head is PMX_ERR_STATE; pmx_get_layer_grad keeps working until the next forward.
 * Errors, before anything is enqueued: PMX_ERR_INVALID for a null context; PMX_ERR_STATE for a facenet / handnet context, "precision" != 0,
 * training off, no backward for the retained forward, consumed gradients.
 *
 * pmx_train_step, asynchronous on the context's stream, after pmx_backward_head AND pmx_backward_trunk for the retained forward (mode 2):
 * the same three phases over every layer that received a gradient -- the head layers of the stages the forward ran and all ten trunk layers,
 * whatever "stop_stage" is.  t is per layer, so a trunk layer that joins at iteration 2000 takes its first step with t = 1 while the head
 * layers are at t = 2001 (Chainer's per-parameter UpdateRule.t).  Still one Adam launch (92 segments at most).  A trunk layer's packs are
 * re-packed like a head layer's: the direct pack and bias, conv1_2's Winograd pack, the transposed packs and their Winograd packs
 * (conv1_1 has none), and conv1_1's fused-kernel pack (pmx_get_pack which = 2).  Either step consumes the gradients for both:
 * pmx_train_step after pmx_train_step_head for the same backward is PMX_ERR_STATE, and the reverse.  pmx_train_step_head in mode 2 leaves
 * the trunk's weights, packs, moments and t alone.
 * Errors as pmx_train_step_head's, and PMX_ERR_STATE in mode 1 and before pmx_backward_trunk. */
int pmx_train_enable(pmx_ctx* ctx, int on);
/* Adam's hyper-parameters from the next step on (the reference lowers alpha at 100 000 and 200 000 iterations).  alpha, eps > 0 and
 * 0 <= beta < 1, else PMX_ERR_INVALID; PMX_ERR_STATE with training off. */
int pmx_train_set_adam(pmx_ctx* ctx, double alpha, double beta1, double beta2, double eps);
/* the gradient scale of one head layer, in mode 2 also of a trunk layer (GradientScaling; rounded to float32).  PMX_ERR_INVALID for an
 * unknown name, and in mode 1 for a trunk layer. */
int pmx_train_set_grad_scale(pmx_ctx* ctx, const char* name, double scale);
int pmx_train_step_head(pmx_ctx* ctx);
int pmx_train_step(pmx_ctx* ctx);
/* The current weights (OIHW, the layer's shape as in pmx_set_layer, the reference's input order) and bias of ANY layer; either pointer may
 * be NULL (both: PMX_ERR_INVALID).  A head layer with training on is read from the master store, anything else is un-packed from its direct
 * pack on the device -- the same floats, a pack holds them unrounded.  Any context.  PMX_ERR_INVALID for an unknown name, PMX_ERR_WEIGHTS
 * for a layer without weights.  Synchronises. */
int pmx_get_layer(pmx_ctx* ctx, const char* name, float* w_oihw, float* bias);
/* Adam's state of one head layer, in mode 2 also of a trunk layer (the reference's --resume): moments of the weights (OIHW) and of the bias, and the step count.  get: any
 * pointer may be NULL.  set: all four arrays, t >= 0, else PMX_ERR_INVALID.  PMX_ERR_STATE with training off.  Both synchronise. */
int pmx_train_get_state(pmx_ctx* ctx, const char* name, float* m_w, float* v_w, float* m_b, float* v_b, int* t);
int pmx_train_set_state(pmx_ctx* ctx, const char* name, const float* m_w, const float* v_w, const float* m_b, const float* v_b, int t);
/* parity accessor: the raw bytes of one pack of a layer -- which = 0 the direct pack, 1 the padded bias, 2 the Winograd pack (conv1_1: its
 * fused-kernel pack), 3 the transposed pack of the data gradient, 4 its Winograd pack (all float32), 5 the f16 pack, 6 the bf16x3 pack
 * (uint16 words).  *n_bytes is the pack's size whenever it exists; PMX_ERR_STATE if it does not exist now, PMX_ERR_INVALID for another
 * `which`, PMX_ERR_CAPACITY if out is NULL or cap_bytes too small.  Synchronises. */
int pmx_get_pack(pmx_ctx* ctx, const char* name, int which, void* out, size_t cap_bytes, size_t* n_bytes);
/* parity accessor, as pmx_get_pack: the f16 pack of the transposed layer of the data gradient (uint16 words), what dx of a 3x3 / 7x7 head
 * layer reads under "grad_precision" 2 -- pack 7 of the Python binding; an entry of its own because pmx_get_pack's `which` ends at 6.
 * It exists once a head backward ran under "grad_precision" 2 (never for a 1x1 layer) and is rewritten by every train step from then on.
 * PMX_ERR_STATE if it does not exist now, PMX_ERR_INVALID for an unknown layer, PMX_ERR_CAPACITY as pmx_get_pack.  Synchronises. */
int pmx_get_transposed_f16_pack(pmx_ctx* ctx, const char* name, void* out, size_t cap_bytes, size_t* n_bytes);
/* test entry: the Adam launch of the training steps on the caller's host arrays of `total` floats each (w, m, v updated in place).  Segment
 * i covers floats [off[i], off[i] + n[i]); off[i] a multiple of 4, the segments in rising order and not sharing a 16-byte vector, else
 * PMX_ERR_INVALID.  Floats outside the segments keep their bits.  Synchronises. */
int pmx_adam_apply(pmx_ctx* ctx, float* w, float* m, float* v, const float* grad, size_t total, const size_t* off, const unsigned* n,
                   const float* scale, const float* alpha_t, int nseg, float omb1, float omb2, float eps);

#ifdef __cplusplus
}
#endif
#endif /* POSE_MI355X_H */
