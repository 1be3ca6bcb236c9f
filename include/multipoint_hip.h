/*
 * libmultipoint_hip.so -- C ABI of the MI355X (gfx950) implementation of the MultiPoint
 * inference hot path (ethz-asl/multipoint).
 *
 * The reference has no FFI: its boundary is Python (class MultiPoint + three free functions).
 * Each entry point below names the reference interface it replaces (paths relative to the
 * reference repository root); multipoint_amd/ binds them with ctypes (see INTEGRATION.md for the
 * stub a reference maintainer would add).
 *
 * Conventions
 *   - every function returns MP_OK (0) or a negative MP_E* code; mp_last_error() gives the text.
 *   - all tensor arguments are DEVICE pointers owned by the caller unless marked "host".
 *     The library never frees or reallocates caller memory; outputs are fully overwritten.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  Kernels are enqueued on
 *     it; functions do not synchronise unless stated.
 *   - one handle per (process, device); a handle is not thread-safe.  The handle owns the packed
 *     device weights and one grow-only workspace.
 *   - images / probability maps are fp32 [B][H][W] (== NCHW with C = 1), H and W multiples of 8.
 *   - coarse descriptor maps are channels-last fp32 [B][H/8][W/8][D].
 *   - keypoint lists are int32 [B][K][2] as (y, x) in row-major order (torch.nonzero order),
 *     counts int32 [B].
 */
#ifndef MULTIPOINT_HIP_H
#define MULTIPOINT_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define MP_OK 0
#define MP_EINVAL (-1)      /* bad argument / unsupported configuration */
#define MP_EHIP (-2)        /* HIP runtime error */
#define MP_ESTATE (-3)      /* call order (e.g. forward before load_weights) */
#define MP_ENOMEM (-4)

typedef struct mp_handle mp_handle;

/* model: keys of MultiPoint.default_config (multipoint/models/MultiPoint.py:9-23) that change
 * the computation */
typedef struct mp_model_config {
    int multispectral;          /* two encoders routed by is_optical (MultiPoint.py:55-59,107-122) */
    int descriptor_head;
    int descriptor_size;        /* 64 (shipped params.yaml) | 128 | 256 */
    int normalize_descriptors;
    int final_batchnorm;
    int reflection_pad;         /* 1: ReflectionPad2d(1), 0: ZeroPad2d(1)  (MultiPoint.py:33-36) */
    int bn_first;               /* MultiPoint.py:137-141 */
    int double_convolution;     /* 1: two 3x3 convolutions per stage; 0: one (MultiPoint.py:144-148) */
    int channel_version;        /* 0: [1,64,64,128,128], heads 256; 1: [1,32,64,96,128]; 2: [1,8,16,32,64] (heads = descriptor_size) */
    /* model.type 'SuperPointMagicLeap' (multipoint/models/SuperPointMagicLeap.py): same layer shapes, no
     * BatchNorm, zero padding, state_dict keys conv1a..conv4b / convPa,convPb / convDa,convDb, heat map =
     * exp(x) / (sum exp(x) + 1e-5) without max subtraction (generate_heatmap, :68-85). */
    int batchnorm;              /* 1: BatchNorm2d after every 3x3 conv (MultiPoint), 0: none (MagicLeap) */
    int key_layout;             /* 0: MultiPoint nn.Sequential keys, 1: SuperPointMagicLeap keys */
    int softmax_mode;           /* 0: nn.Softmax2d, 1: MagicLeap generate_heatmap arithmetic */
    /* MultiPoint.py:21,99-103: forward under torch.cuda.amp.autocast.  1: fp16 activations and weights on the
     * fp16 MFMA (fp32 accumulate), BatchNorm / softmax / descriptor normalisation in fp32; inputs and outputs
     * of mp_forward stay fp32. */
    int mixed_precision;
    /* Algorithm of the 3x3 convolutions (no reference counterpart: ATen picks its own).  0 auto (= 1), 1 winograd43: Winograd
     * F(4x4,3x3) on the fp32 MFMA -- the fastest; equal to the fp32 reference within 2e-5 (prob) / 2e-6 (desc), which can reorder
     * EXACT ties of the heat map (flat or saturated image regions; a top-k cut inside a plateau of tied scores picks other members of
     * the plateau: parity.structured of bench.py); 2
     * winograd43_general: the same arithmetic on the any-frame-size kernel only; 3 direct: implicit-GEMM convolution, a k-ordered
     * fp32 multiply-add chain per output like the reference's -- keeps exact ties, 2.4x slower.  INTEGRATION.md has the numbers. */
    int conv_algorithm;
    /* 1: a forward's output bits do not depend on how many images it holds.  By default (0) forwards of ONE or TWO images (counted over
     * the whole forward, not per encoder of a multispectral model) --
     * the reference's shipped batchsize 1 -- run launches that are too small to fill the GPU with their input channels cut into
     * ranges (single-pair latency: 0.51 instead of 0.56 ms at 480x640, 0.33 instead of 0.44 ms at 240x320), which sums the same products in another order than the
     * batched launch does: equal within 3e-5 (prob) / 3e-6 (desc), deterministic from run to run, but not bit-identical to the
     * same images inside a larger batch.  Set it when shards of <= 2 images must reproduce a batched run bit for bit. */
    int batch_invariant;
} mp_model_config;

/* one entry of the reference state_dict (torch.save(net.state_dict()), train.py:161-173), host fp32 */
typedef struct mp_tensor {
    const char* name;           /* e.g. "encoder.5.weight", "detector_head_convolutions.5.running_var" */
    const float* data;          /* host pointer, contiguous, reference layout (conv: OIHW) */
    long long numel;
} mp_tensor;

/* lifetime ----------------------------------------------------------------------------------- */
int mp_create(mp_handle** out, int device);
void mp_destroy(mp_handle* h);
const char* mp_last_error(const mp_handle* h);      /* h may be NULL: error of the last mp_create */
const char* mp_version(void);
/* The machine shape the handle's persistent kernels are sized for, derived from the device in mp_create (compute units;
 * XCDs = L2 domains the work items are cut into; workgroups of a one-per-CU persistent launch).  No reference counterpart: the
 * reference leaves scheduling to ATen.  mp_create fails with MP_EINVAL on a shape the kernels cannot be scheduled on. */
int mp_device_shape(const mp_handle* h, int* compute_units, int* xcds, int* persistent_workgroups);

/* replaces MultiPoint.__init__ + load_state_dict (MultiPoint.py:25-91,
 * predict_align_image_pair.py:57-62): validates the key set strictly, repacks conv weights into
 * MFMA fragment order, precomputes eval-mode BatchNorm scale/shift, uploads. */
int mp_load_weights(mp_handle* h, const mp_model_config* cfg, const mp_tensor* tensors, int n_tensors);

/* replaces MultiPoint.forward / forward_impl in eval mode (MultiPoint.py:99-135).
 *   images      [B][H][W] fp32 in [0,1]
 *   is_optical  host uint8[B] or NULL (only read when cfg.multispectral)
 *   prob        [B][H][W] or NULL          (softmax -> drop dustbin -> PixelShuffle(8))
 *   logits      [B][65][H/8][W/8] or NULL  (force_return_logits path, MultiPoint.py:153-154)
 *   desc        [B][H/8][W/8][D] or NULL   (channels-last; L2-normalised if cfg says so) */
int mp_forward(mp_handle* h, const float* images, const unsigned char* is_optical, int B, int H,
               int W, float* prob, float* logits, float* desc, void* stream);

/* The launch plan of mp_forward for a B x H x W forward of the loaded model, read-only: one record per convolution launch the
 * planner decides on -- each encoder's first block (when it is a launch of its own), its 3x3 layers, and the launch of both 3x3 head
 * convolutions -- in launch order (multispectral: the thermal encoder's, then the optical one's).  The 1x1 head layers are not
 * planned: they run in the fused head tail or on the direct / streaming kernels for every shape.  Nothing is launched or allocated;
 * the records come from the functions mp_forward itself plans and sizes its launches with.  No reference counterpart: the
 * reference leaves kernel selection to ATen.  For tests and tools that must know which kernel instantiation a shape reaches. */
#define MP_PLAN_FIRST 0             /* the first block (Cin = 1) as a launch of its own */
#define MP_PLAN_DIRECT 1            /* direct implicit-GEMM fp32 kernel */
#define MP_PLAN_WINO43 2            /* fp32 F(4x4,3x3), frames that are multiples of the 4x4 tile, reflection padding */
#define MP_PLAN_WINO43B 3           /* fp32 F(4x4,3x3), any frame, either padding */
#define MP_PLAN_F16 4               /* fp16 streaming kernel */
#define MP_PLAN_F16_RES 5           /* fp16 kernel with LDS-resident weights */
#define MP_PLAN_F16_RES_SLICES 6    /* ... launched once per 64-channel output slice */
typedef struct mp_plan_launch {
    const char* name;           /* the launch's profile name (mp_profile_read), e.g. "enc.conv1+2", "enc.conv5", "heads.conv3x3" */
    int kernel;                 /* MP_PLAN_* */
    int images, H, W;           /* the launch's input: images of this encoder (heads: of the forward), frame of this layer */
    int pooled;                 /* the launch applies the 2x2 max-pool that follows the layer */
    int tc4;                    /* F(4x4,3x3): tile columns of an item, 8 (16 x 32 pixels) or 4 (32 x 16 pixels); else 0 */
    int ks_shift;               /* F(4x4,3x3): the input channels run as 2^ks_shift ranges (forwards of one or two images) */
    int vin;                    /* F(4x4,3x3): the input is transformed once, by a pass of its own, in front of the launch */
    int fuse_first;             /* the first block is evaluated inside this launch */
    int in_layout, out_layout;  /* 0 NHWC, 1 channel-quad planar, 2 column-interleaved planar */
    int workgroups;             /* F(4x4,3x3): workgroups of the persistent launch; else 0 */
    long long items;            /* F(4x4,3x3): work items (tile block, slice [, range]) the workgroups walk; else 0 */
} mp_plan_launch;
/*   n_optical  images the optical encoder receives (multispectral models; ignored otherwise)
 *   out        capacity records or NULL; *n receives the number of records of the plan (only the first `capacity` are written) */
int mp_forward_plan(mp_handle* h, int B, int H, int W, int n_optical, mp_plan_launch* out, int capacity, int* n);

/* replaces MultiPoint.forward in TRAINING mode, forward only (the reference's train.py never calls net.eval(), so its validation
 * loop, train.py:127-150, runs this): every BatchNorm2d normalises with the mean and biased variance of this batch (eps 1e-5);
 * the detector head returns logits only (MultiPoint.py:150-158).  fp32 models with BatchNorm only: mixed_precision models and
 * models without BatchNorm (SuperPointMagicLeap) are refused with MP_EINVAL, as is a batch in which some BatchNorm layer sees
 * a single value per channel (torch raises ValueError there: e.g. B = 1 at 8x8).  Multispectral: each encoder's statistics
 * cover the images routed to it; an encoder that receives no images does not run and its statistics are left unwritten.
 * Every layer runs on the direct convolution kernels plus three batchnorm_stats.hip passes; the results are bit-identical from
 * run to run.  The running statistics of the model are not touched.
 *   logits [B][65][H/8][W/8] (required), desc [B][H/8][W/8][D] or NULL (channels-last, as mp_forward)
 *   stats  NULL, or fp32: per BatchNorm layer i (mp_batch_stats_layer), in state_dict order, [2][C_i] = the batch mean and the
 *          unbiased variance (what torch blends into running_mean / running_var with momentum 0.1); layer i starts at float
 *          offset 2 * (C_0 + ... + C_{i-1}) */
int mp_forward_batch_stats(mp_handle* h, const float* images, const unsigned char* is_optical, int B, int H, int W,
                           float* logits, float* desc, float* stats, void* stream);
/* the BatchNorm layers of the loaded model in state_dict order: their number (0 without BatchNorm), and layer i's state_dict
 * prefix (e.g. "encoder.2", "detector_head_convolutions.5"; valid until the next mp_load_weights) and channel count C_i */
int mp_batch_stats_count(const mp_handle* h, int* count);
int mp_batch_stats_layer(const mp_handle* h, int i, const char** name, int* channels);

/* replaces utils.box_nms (multipoint/utils/utils.py:78-122) incl. the `prob * valid_mask`
 * multiply of its callers (predict_align_image_pair.py:128,133).
 *   valid_mask  uint8 [B][H][W] or NULL
 *   prob_nms    [B][H][W] dense output (zeros except kept pixels, which keep their score)
 *   max_rounds  0: run until converged (groups of 8 rounds, one 4-byte host read per group: synchronises
 *               `stream`; at most 4096 rounds); >0: enqueue exactly that many (<= 64) fixed-point rounds
 *               asynchronously, check with mp_nms_unresolved() after a sync.
 *   iou         DOUBLE: torchvision's CPU kernel (nms_kernel_impl(dets, scores, double iou_threshold)) compares the fp32 overlap
 *               ratio with the caller's Python float in double, and 0.1 is not 0.1f (they differ where ratio == (float)iou,
 *               e.g. size 11, iou 0.1, offset 9: 22 / 220).
 * Any H x W (the reference takes any 2-D / 4-D map, utils.py:90-91; W need not be a multiple of 4 here either).  Deviation:
 * box sizes above 16 are refused with MP_EINVAL (a footprint row is one 32-bit mask; the reference has no limit, its shipped
 * configs use 4).
 * Tie-break (stated rule): priority = (score descending, row-major index ascending). */
int mp_box_nms(mp_handle* h, const float* prob, const unsigned char* valid_mask, int B, int H, int W,
               float size, float min_prob, double iou, int keep_top_k, float* prob_nms,
               int max_rounds, void* stream);

/* fused box_nms + torch.nonzero(prob_nms > min_prob) (predict_align_image_pair.py:170-171,
 * evaluation.py:262-263): same NMS, but the survivors are returned as lists.
 *   kp_yx [B][K][2], kp_score [B][K] (may be NULL), kp_count [B]; kp_count may exceed K when
 *   keep_top_k == 0 and more than K pixels survive (only the first K are stored). */
int mp_detect_keypoints(mp_handle* h, const float* prob, const unsigned char* valid_mask, int B, int H,
                        int W, float size, float min_prob, double iou, int keep_top_k, int K,
                        int* kp_yx, float* kp_score, int* kp_count, int max_rounds, void* stream);

/* ---- spatially uniform top-k: adaptive non-maximal suppression (an extension; Brown, Szeliski and Winder 2005) ----
 * The reference keeps the keep_top_k highest scores, which all land in one corner when the texture does.  The spread entries
 * keep the keep_top_k candidates with the largest suppression radius instead.  Per image, with the NMS survivors in row-major
 * order (y_i, x_i, s_i), i < n, and c = robust (fp32, 0 < c <= 1):
 *   dominance  j dominates i iff s_i < c * s_j, the product being ONE fp32 multiply; equal scores never dominate each other,
 *              and with c < 1 a score exactly equal to c * s_j is not dominated
 *   radius     R_i = min over the dominators j of (y_i - y_j)^2 + (x_i - x_j)^2 as a uint32 (< 2^25 at 4096 x 4096);
 *              R_i = 0xFFFFFFFF when nothing dominates i
 *   selection  order by (R descending, score bits descending, row-major index ascending) and keep the first min(keep_top_k, n);
 *              n <= keep_top_k keeps every survivor, as the score entries do
 * The output contract is that of mp_box_nms / mp_detect_keypoints: kept keypoints in row-major order, kp_score their scores,
 * kp_count their number, rows at or beyond K not stored, the dense prob_nms the kept scores and zeros elsewhere.
 *   kp_radius2  uint32 [B][K] or NULL: R of every stored keypoint
 * Refused with MP_EINVAL before any launch, outputs untouched: robust outside (0, 1] or not finite, keep_top_k <= 0, and what
 * mp_box_nms / mp_detect_keypoints refuse.
 * Tie guards: of the three conditions behind mp_topk_ambiguous, the plateau at the score cut and the exact-tie split describe
 * a cut on scores and are NOT evaluated by the spread entries; the footprint tie guard is, unchanged.
 * mp_suppression_radii: R alone for any integer keypoint list (mp_detect_keypoints', mp_extract_keypoints', a classic
 * detector's): kp_yx [B][K][2] with 0 <= y, x < 32768, kp_score [B][K] positive, kp_count [B] (a count above K is clamped), 0 < B <= 65535;
 * radius2 uint32 [B][K], rows at or beyond the count are not written.  No result depends on B or on the launch geometry. */
int mp_box_nms_spread(mp_handle* h, const float* prob, const unsigned char* valid_mask, int B, int H, int W,
                      float size, float min_prob, double iou, int keep_top_k, float* prob_nms,
                      int max_rounds, float robust, void* stream);
int mp_detect_keypoints_spread(mp_handle* h, const float* prob, const unsigned char* valid_mask, int B, int H,
                               int W, float size, float min_prob, double iou, int keep_top_k, int K,
                               int* kp_yx, float* kp_score, int* kp_count, int max_rounds, float robust,
                               unsigned* kp_radius2, void* stream);
int mp_suppression_radii(mp_handle* h, const int* kp_yx, const float* kp_score, const int* kp_count, int B, int K,
                         float robust, unsigned* radius2, void* stream);

/* number of still-undecided NMS candidates summed over all mp_box_nms / mp_detect_keypoints calls since
 * the previous mp_nms_unresolved (0 = every result exact); resets the counter.  Synchronises `stream`. */
int mp_nms_unresolved(mp_handle* h, int* unresolved, void* stream);

/* Top-k tie guard (no reference counterpart; it exists because the reference's list is a function of EXACT score order,
 * multipoint/utils/utils.py:97-116: score-ordered indices, per-image [:keep_top_k]).  The default convolution algorithm
 * (Winograd F(4x4,3x3)) equals the fp32 reference within ~1e-5 in prob, which reorders exact ties of the heat map; when the
 * top-k cut of an image falls inside a plateau of (near-)tied scores, WHICH members of the plateau are kept is then decided by
 * that noise.  mp_box_nms / mp_detect_keypoints (keep_top_k > 0) therefore count, per image, the NMS survivors whose score lies
 * within `eps` (default 6e-5: the measured prob noise) of the k-th score -- admitted ones and cut-off ones separately -- and flag
 * the image when BOTH counts reach `min_each_side` (default 4; 0 switches the guard off).  A flagged image is one whose list the
 * caller should recompute from a forward with conv_algorithm 3 (direct), which keeps exact ties; the Python mirror does that in
 * PairPipeline.run_converged / utils.box_nms_tie_robust, the throughput entry only reports the count.
 * Two more conditions raise the same per-image flag:
 *   - the cut splits a run of EXACTLY equal scores (some admitted, some not), whatever their number;
 *   - footprint tie guard (also for keep_top_k == 0, the shipped configs' `topk: 0`): at least `min_pairs` (default 16; 0: off)
 *     of the image's NMS decisions were taken between scores within `eps` -- a candidate suppressed by kept neighbours that are
 *     ALL within eps of its own score, i.e. a suppression the noise could have turned around -- and they are at least 1 % of the
 *     image's survivors.  Heat maps of independent scores hold about one such pair per 1000 survivors (0-5 per 480x640 image at
 *     eps 6e-5, measured on the oracle's maps); a plateau of tied scores inside one footprint holds several per survivor.
 * What the guard does NOT cover (stated residual): fewer than min_each_side / min_pairs near-ties -- a single near-tied pair
 * straddling the cut or inside a footprint flips with the noise; those are the explained fp32 flips the parity tests bound
 * (<= 0.2 % of the keypoints, tests/test_gpu_e2e_parity.py).
 *   mp_topk_ambiguous: flags [B] (host ints, 0/1) of the LATEST mp_box_nms / mp_detect_keypoints call; *total = flagged
 *   images summed over all calls since the previous read (resets).  Synchronises `stream`. */
int mp_topk_tie_guard(mp_handle* h, float eps, int min_each_side);
int mp_nms_tie_guard(mp_handle* h, int min_pairs);
int mp_topk_ambiguous(mp_handle* h, int* flags, int B, int* total, void* stream);

/* replaces torch.nonzero(map > thr) on an arbitrary dense map; with valid_mask (uint8 [B][H][W] or NULL) it is
 * torch.nonzero((map > thr) * valid_mask) (multipoint/utils/evaluation.py:156-157, predict_keypoints.py:176-178).  Any H x W. */
int mp_extract_keypoints(mp_handle* h, const float* map, const unsigned char* valid_mask, int B, int H, int W, float thr,
                         int K, int* kp_yx, float* kp_score, int* kp_count, void* stream);

/* replaces utils.interpolate_descriptors (multipoint/utils/utils.py:159-167).
 *   desc [B][Hc][Wc][D] channels-last, D a multiple of 64 up to 384, out [B][K][D]; rows k >= kp_count[b] are written as
 *   zeros. */
int mp_sample_descriptors(mp_handle* h, const float* desc, int B, int Hc, int Wc, int D, int H, int W,
                          const int* kp_yx, const int* kp_count, int K, float* out, void* stream);

/* ---- sub-pixel keypoints (an extension: the reference keeps torch.nonzero's integer pixels; its interpolate_descriptors and
 * cv2.findHomography take float positions) ----
 * mp_refine_keypoints: a separable log-parabola fit on the detector map around every entry of a keypoint list, one thread per
 * entry.  Any H x W.
 *   prob       fp32 [B][H][W]: the FORWARD's map -- not the NMS output, whose suppressed neighbours are zero
 *   kp_yx, kp_count, K   a list as mp_detect_keypoints / mp_extract_keypoints write it (a count above K is clamped)
 *   kp_sub_yx  fp32 [B][K][2] (y, x); rows k >= min(kp_count[b], K) are written as zeros
 * Per axis, with p0 = prob[y][x], p-, p+ its two neighbours on that axis, l = logf(p) and den = l- - 2 l0 + l+: the axis is
 * refined iff both neighbours lie inside the frame, p-, p0, p+ are all finite and > 0, p0 >= p-, p0 >= p+ and den < 0; then
 * delta = 0.5 (l- - l+) / den (so |delta| <= 0.5), else delta = 0 and the output is exactly (float)y / (float)x.
 * mp_sample_descriptors_f: mp_sample_descriptors at float positions kp_yx_f [B][K][2] (the reference's keypoints.float(),
 * utils.py:159-167): the same kernel body from the normalisation on, zero padding of out-of-range taps as grid_sample's; whole
 * numbers give the bits of mp_sample_descriptors. */
int mp_refine_keypoints(mp_handle* h, const float* prob, int B, int H, int W, const int* kp_yx, const int* kp_count, int K,
                        float* kp_sub_yx, void* stream);
int mp_sample_descriptors_f(mp_handle* h, const float* desc, int B, int Hc, int Wc, int D, int H, int W,
                            const float* kp_yx_f, const int* kp_count, int K, float* out, void* stream);

/* replaces utils.get_matches(..., 'nnmatcher' | 'bfmatcher' crossCheck=True)
 * (multipoint/utils/matching.py:4-33, NNMatcher.match :41-72) for P independent pairs.
 *   descA/descB: first pair's descriptors [K][D]; pair p at + p * pair_stride floats
 *   countA/countB: int32, pair p at [p * count_stride]
 *   threshold < 0 disables the distance test (plain mutual NN == crossCheck)
 *   match_idx [P][K]: train index of query i or -1; match_dist [P][K]; match_count [P]
 *   0 < P <= 65535 (all four matchers: a pair is a row of the launch grid), K > 0, D must be 64, 128, 256 or 384 (LGHD) */
int mp_match_mutual_nn(mp_handle* h, const float* descA, const int* countA, const float* descB,
                       const int* countB, long long pair_stride, int count_stride, int P, int K,
                       int D, float threshold, int* match_idx, float* match_dist, int* match_count,
                       void* stream);

/* replaces the per-sample arithmetic of utils.compute_descriptor_metrics (multipoint/utils/evaluation.py:287-328) on
 * the device-resident lists the calls above produced, for P pairs stored interleaved (image slot 2p = optical,
 * 2p+1 = thermal):
 *   kp_yx [2P][K][2], kp_count [2P]; match_idx [P][K]: thermal index matched to optical keypoint i, or -1
 *   homography  device double [2P][9], row-major 3x3 acting on (x, y, 1): slot 2p = ground-truth optical->thermal
 *               homography h_t * inv(h_o) (evaluation.py:259), slot 2p+1 = its inverse (:288)
 *   metrics [P][8] int32: n_gt_optical, n_gt_thermal (:297-298), num_matched_optical, num_matched_thermal (:301-311),
 *               N_optical, N_thermal (warped keypoints inside the H x W image, :315-316), number of matches, 0
 *   tp [2P][K] uint8: tp[2p][i] = match of optical keypoint i is correct; tp[2p+1][j] = match of thermal keypoint j
 *               (the same mutual pair seen from the other side) is correct; 0 for unmatched keypoints */
int mp_pair_metrics(mp_handle* h, const int* kp_yx, const int* kp_count, const int* match_idx, const double* homography,
                    int P, int K, int H, int W, float threshold_keypoints, int* metrics, unsigned char* tp,
                    void* stream);

/* replaces the per-sample arithmetic of utils.compute_repeatability_multispectral (multipoint/utils/evaluation.py:156-199)
 * for P pairs stored interleaved (slot 2p = optical, 2p+1 = thermal):
 *   homography  device double [2P][2][9]: for slot b first the INVERSE of its own homography, then the other image's
 *               homography (evaluation.py:168-169,173-174); both warps truncate to integers like warp_keypoints' default
 *   counts [P][4] int32: count1 (warped thermal points with an optical keypoint within distance_thresh), count2 (warped
 *               optical points near a thermal keypoint), N_thermal, N_optical (warped points inside the H x W frame);
 *               repeatability = (count1 + count2) / (N_thermal + N_optical)  (:198-199) */
int mp_repeatability(mp_handle* h, const int* kp_yx, const int* kp_count, const double* homography, int P, int K, int H,
                     int W, double distance_thresh, int* counts, void* stream);

/* replaces cv2.findHomography(optical_pts, thermal_pts, cv2.RANSAC, ransacReprojThreshold) on the matched keypoints
 * (predict_align_image_pair.py:205-216, multipoint/utils/evaluation.py:330-349) for P pairs (slot 2p optical, 2p+1
 * thermal).  Not a bit-level restatement of OpenCV (absent third-party code with its own RNG): max_iters hypotheses
 * from 4 random matches each (counter-based RNG on `seed`: reproducible), forward reprojection error test, most
 * inliers wins, normalised-DLT refit over the winner's inliers.  OpenCV's closing Levenberg-Marquardt polish is a call of
 * its own: mp_refine_homography.
 *   homography   device double [P][9], row-major, maps optical (x, y, 1) to thermal; all zeros when < 4 matches or
 *                no hypothesis found 4 inliers (the reference's `H_est is None`)
 *   inlier_mask  uint8 [P][K] per OPTICAL keypoint (1 = its match is an inlier); n_inliers int32 [P] */
int mp_find_homography(mp_handle* h, const int* kp_yx, const int* kp_count, const int* match_idx, int P, int K,
                       double reproj_threshold, int max_iters, unsigned long long seed, double* homography,
                       unsigned char* inlier_mask, int* n_inliers, void* stream);
/* the same on sub-pixel keypoints: kp_sub_yx fp32 [2P][K][2] (y, x) (mp_refine_keypoints) in the place of kp_yx; one kernel
 * template behind both, so a float list of whole numbers gives the bits of mp_find_homography */
int mp_find_homography_f(mp_handle* h, const float* kp_sub_yx, const int* kp_count, const int* match_idx, int P, int K,
                         double reproj_threshold, int max_iters, unsigned long long seed, double* homography,
                         unsigned char* inlier_mask, int* n_inliers, void* stream);

/* the other modes of utils.get_matches (multipoint/utils/matching.py:4-33); same descriptor / count addressing as
 * mp_match_mutual_nn, 1 <= D <= 384.
 * mp_match_knn2 replaces cv2.BFMatcher(cv2.NORM_L2).knnMatch(d1, d2, 2) (:21, followed by Lowe's ratio test :23-27)
 * and .match() without crossCheck (:7,31): nn_idx / nn_dist [P][K][2] = the two nearest train rows of every query
 * row under ||a - b||_2 (ties: lower train index first), idx -1 where the pair has fewer than 1 / 2 train rows.
 * mp_match_threshold replaces ThresholdMatcher.match (:81-99): every (i, j) with sqrt(2 - 2 clip(a.b, -1, 1)) <
 * threshold is appended (arbitrary order) to list_ij [P][capacity][2] / list_dist [P][capacity]; list_count [P] is
 * the number FOUND (may exceed capacity: the caller retries with a larger list). */
int mp_match_knn2(mp_handle* h, const float* descA, const int* countA, const float* descB, const int* countB,
                  long long pair_stride, int count_stride, int P, int K, int D, int* nn_idx, float* nn_dist,
                  void* stream);
int mp_match_threshold(mp_handle* h, const float* descA, const int* countA, const float* descB, const int* countB,
                       long long pair_stride, int count_stride, int P, int K, int D, float threshold, int capacity,
                       int* list_ij, float* list_dist, int* list_count, void* stream);

/* one-directional matching of P pairs at the speed of mp_match_mutual_nn (the same MFMA distance tiles, one direction,
 * the two nearest per query); same descriptor / count addressing and the same [P][K] outputs as mp_match_mutual_nn, so
 * mp_find_homography and the per-pair records take them unchanged.  Rows are taken as UNIT vectors (what
 * mp_sample_descriptors always produces): the metric is sqrt(2 - 2 clip(a.b, -1, 1)), which for unit rows equals the
 * L2 distance; for arbitrary rows use mp_match_knn2.  D must be 64, 128, 256 or 384.
 *   ratio <= 0  replaces cv2.BFMatcher(cv2.NORM_L2).match() without crossCheck (matching.py:7,31): every query row of
 *               a pair with at least one train row is matched to its nearest (ties: the lower train index).
 *   ratio > 0   replaces knnMatch(d1, d2, 2) plus Lowe's ratio test (matching.py:20-27): query i keeps its nearest iff
 *               (double)d1 < ratio * (double)d2, compared in double as Python compares `m.distance < 0.9 * n.distance`
 *               (pass 0.9, not 0.9f).  A pair with fewer than two train rows yields no matches (the reference's
 *               `for m, n in all_matches` raises there).
 *   match_idx [P][K]: train index of query i or -1; match_dist [P][K] (0 where unmatched); match_count [P]
 *   second_idx / second_dist [P][K] or NULL: the second-nearest train row of every query row (-1 / 0 where the pair
 *               has fewer than two train rows or i >= countA), whatever the ratio test decided */
int mp_match_nearest(mp_handle* h, const float* descA, const int* countA, const float* descB, const int* countB,
                     long long pair_stride, int count_stride, int P, int K, int D, double ratio,
                     int* match_idx, float* match_dist, int* match_count,
                     int* second_idx /* [P][K] or NULL */, float* second_dist /* [P][K] or NULL */, void* stream);

/* guided matching: mutual nearest neighbours INSIDE a geometric gate, for re-matching under a first homography estimate
 * (mp_find_homography).  Descriptors, counts, outputs and limits as for mp_match_mutual_nn (unit rows, the same fp32 MFMA
 * distance tiles, D 64 / 128 / 256, 0 < P <= 65535); the list is again one-to-one, so mp_find_homography, mp_pair_metrics and
 * the per-pair records take it unchanged.
 *   kpA_yx / kpB_yx  int32 (y, x) of the optical / thermal rows, addressed like the descriptors: row r of pair p at
 *                kp + (p * (pair_stride / D) + r) * 2 -- for the interleaved lists of a pair batch kp_yx and kp_yx + 2 K
 *                (pair_stride must be a multiple of D)
 *   homography   device double [P][9], row-major, optical (x, y, 1) -> thermal, as mp_find_homography writes it
 *   wa_i       = H_p (x_i, y_i, 1) in double, divided by its third component and rounded once to fp32; optical row i has no
 *                candidates if that component is 0 or the result is not finite -- so a pair whose H_p is all zeros
 *                (mp_find_homography's "no estimate") gets no matches
 *   gate(i, j) = (wa_i.x - x_j)^2 + (wa_i.y - y_j)^2 <= radius^2 in fp32 (radius finite and positive)
 *   i is matched to j iff j minimises d(i, .) over {j : gate(i, j)} and i minimises d(., j) over {i : gate(i, j)} (the
 *                lower index wins exact ties) and, with threshold >= 0, d < threshold
 * Both directions decide the gate from the same fp32 bits, so the mutual test is exact; results are bit-identical from
 * run to run. */
int mp_match_guided(mp_handle* h, const float* descA, const int* countA, const float* descB, const int* countB,
                    long long pair_stride, int count_stride, int P, int K, int D, const int* kpA_yx, const int* kpB_yx,
                    const double* homography /* [P][9] */, float radius, float threshold, int* match_idx, float* match_dist,
                    int* match_count, void* stream);

/* the last step of cv2.findHomography(..., cv2.RANSAC, thr), which mp_find_homography leaves out: a Levenberg-Marquardt
 * polish of the estimate over its inliers (OpenCV 4.2: HomographyRefineCallback + createLMSolver(cb, 10)).  fp64; 8
 * parameters (h22 = 1), residuals (x' - u, y' - v), lambda_0 = 1e-3, at most `iters` iterations (OpenCV: 10) of at most 8
 * trial steps (J^T J + lambda diag(J^T J))^-1 (-J^T r); a step is accepted iff the cost falls (then lambda <- max(0.1
 * lambda, 1e-12), else lambda <- 10 lambda; a singular system is a rejected trial), an iteration without an accepted step
 * ends the polish.  Lists as for mp_find_homography (slot 2p optical, 2p+1 thermal; 0 < K <= 3200); match_idx may come
 * from any of the matchers.
 *   homography   device double [P][9]: in the estimate, out the polished matrix divided by h22.  All zeros out when the
 *                input is all zeros (or has h22 = 0) or fewer than 4 matches are inliers
 *   inlier_mask  uint8 [P][K] per optical keypoint, n_inliers [P]: the matches whose forward reprojection error under the
 *                INPUT estimate is <= reproj_threshold -- the set the polish runs on, recomputed here
 *   cost         double [P][2] or NULL: sum of squared residuals over that set before / after (after <= before) */
int mp_refine_homography(mp_handle* h, const int* kp_yx, const int* kp_count, const int* match_idx, int P, int K,
                         double reproj_threshold, int iters, double* homography, unsigned char* inlier_mask, int* n_inliers,
                         double* cost /* [P][2] or NULL */, void* stream);
/* the same on sub-pixel keypoints (kp_sub_yx fp32 [2P][K][2]); whole numbers give the bits of mp_refine_homography */
int mp_refine_homography_f(mp_handle* h, const float* kp_sub_yx, const int* kp_count, const int* match_idx, int P, int K,
                           double reproj_threshold, int iters, double* homography, unsigned char* inlier_mask, int* n_inliers,
                           double* cost /* [P][2] or NULL */, void* stream);

/* ---- pooled homography: ONE model per group of pairs, from the matches of all of them (an extension; the reference leaves the
 * initial transform of a recording to a hand measurement).  A rig has one optical -> thermal transform for a whole recording; a
 * single cross-spectral pair has few matches and many wrong ones, many pairs together have thousands.  The algorithm is
 * mp_find_homography's and mp_refine_homography's with the group index in the place of the pair index (sampling is
 * sample4(seed, g, t, n_g)), so a group that holds one pair gets that pair's model; the correspondences live in global memory
 * instead of LDS, so there is no 3200 limit.  Results are bit-identical from run to run (integer atomics only).
 *
 * mp_pool_matches compacts the match lists of P pairs (lists as for mp_find_homography: slot 2p optical, 2p+1 thermal; any K):
 *   groups        device int32 [P], the group id of every pair, NON-DECREASING, in [0, G) -- or NULL: one group (G must be 1).
 *                 Unchecked (device data); ids that decrease give group ranges that are wrong but never out of bounds
 *   pts           device fp32 [capacity][4], 16-byte aligned: (x, y) optical, (u, v) thermal of every match with
 *                 0 <= match_idx < thermal count, pair-major, query order inside a pair
 *   query_index   device int32 [capacity]: the optical keypoint (row of match_idx) each row of pts came from
 *   capacity      rows of pts / query_index; rows beyond it are dropped, so it must reach pair_offsets[P] (P * K always does)
 *   pair_offsets  device int32 [P + 1]: pair p owns rows pair_offsets[p] .. pair_offsets[p + 1]; pair_offsets[P] = N
 *   group_offsets device int32 [G + 1]: group g owns rows group_offsets[g] .. group_offsets[g + 1] (empty groups allowed)
 *   workspace     device scratch of mp_pooled_workspace_bytes(P, G, max_iters) bytes (any max_iters >= 1 for this call)
 * mp_find_homography_pooled estimates one model per group of a pts list (from mp_pool_matches or the caller's own fp32 points):
 *   N             rows of pts, 0 <= N < 2^24; 0 < G <= 65535; 0 < max_iters <= 2^20
 *   homography    device double [G][9], optical (x, y, 1) -> thermal; all zeros for a group with fewer than 4 rows or without a
 *                 hypothesis of 4 inliers
 *   inlier_mask   device uint8 [N], one per row of pts (all zeros in a group without a model); n_inliers int32 [G]
 * mp_refine_homography_pooled is mp_refine_homography on the groups: homography [G][9] in / out, inlier_mask [N] / n_inliers [G]
 * of the INPUT estimate, cost [G][2] or NULL.
 * mp_pooled_chunk reports the points per staged chunk of the scoring kernel and the most workgroups that share one group's
 * points (the sizes at which the kernel changes path; for tests). */
int mp_pooled_chunk(int* chunk_points, int* max_splits);
int mp_pooled_workspace_bytes(int P, int G, int max_iters, long long* bytes);
int mp_pool_matches(mp_handle* h, const int* kp_yx, const int* kp_count, const int* match_idx, const int* groups /* [P] or NULL */,
                    int P, int K, int G, float* pts, int* query_index, long long capacity, int* pair_offsets, int* group_offsets,
                    void* workspace, long long workspace_bytes, void* stream);
/* mp_pool_matches on sub-pixel keypoints (kp_sub_yx fp32 [2P][K][2]): pts holds the float positions as they are; the pooled
 * estimators take pts and need no second entry */
int mp_pool_matches_f(mp_handle* h, const float* kp_sub_yx, const int* kp_count, const int* match_idx,
                      const int* groups /* [P] or NULL */, int P, int K, int G, float* pts, int* query_index, long long capacity,
                      int* pair_offsets, int* group_offsets, void* workspace, long long workspace_bytes, void* stream);
int mp_find_homography_pooled(mp_handle* h, const float* pts, const int* group_offsets, long long N, int G,
                              double reproj_threshold, int max_iters, unsigned long long seed, double* homography,
                              unsigned char* inlier_mask, int* n_inliers, void* workspace, long long workspace_bytes, void* stream);
int mp_refine_homography_pooled(mp_handle* h, const float* pts, const int* group_offsets, long long N, int G,
                                double reproj_threshold, int iters, double* homography, unsigned char* inlier_mask, int* n_inliers,
                                double* cost /* [G][2] or NULL */, void* stream);

/* ---- similarity and affine models on the same three routes (an extension; the reference's manual alignment estimates its
 * initial transform both ways, cv2.estimateRigidTransform(ir, opt, False) next to cv2.findHomography,
 * create_dataset/helper_functions/align.py).  A rig's optical -> thermal transform is close to a similarity, and a pair with
 * 6-10 correct matches among dozens of wrong ones determines 4 or 6 parameters where it does not determine 8.  Not OpenCV's
 * estimateAffinePartial2D / estimateAffine2D bit for bit; no adaptive iteration bound.
 *   MP_MODEL_HOMOGRAPHY  the entry forwards to its *_homography* counterpart (`rounds` as `iters`): the same bits
 *   MP_MODEL_SIMILARITY  [[a, -b, tx], [b, a, ty], [0, 0, 1]]; a hypothesis from 2 distinct matches in closed form (refused
 *                        when they lie closer than 1e-5 px: |d|^2 < 1e-10)
 *   MP_MODEL_AFFINE      [[a, b, tx], [c, d, ty], [0, 0, 1]]; a hypothesis from 3 matches by 3x3 elimination with partial
 *                        pivoting (refused when a pivot is below 1e-10: collinear points)
 * Arguments, lists, limits, sampling (sample4's counter scheme on S = 2 / 3 indices), tie-break and determinism are those of the
 * counterparts; the test is forward error^2 <= reproj_threshold^2 (no division).  The refit over the winner's consensus set
 * is the exact least-squares minimiser of the summed squared forward error (closed form on centred points / 3x3 normal
 * equations on centred source points); a winner with fewer than S + 1 inliers -- a model that explains only its own sample --
 * gives a zero matrix, zero count and zero mask.
 * mp_refine_transform* is local optimisation in the place of the Levenberg-Marquardt polish, which the exact refit makes
 * unnecessary: at most `rounds` (0..1000) times { mark the inliers of the current model, refit over them }, ended early by a
 * marking that changes nothing.  In: the estimate (top two rows divided by h22; the last row is taken as (0, 0, h22)).  Out: the
 * last model, inlier_mask / n_inliers of the last set marked (the set that model was fitted to; the input's own for rounds =
 * 0), cost [.][2] or NULL: the summed squared error over that set under the model before / after the last refit
 * (after <= before).  All outputs are zero for an estimate that is all zeros, not finite or has h22 = 0, and when a marked
 * set has fewer than S + 1 members. */
#define MP_MODEL_HOMOGRAPHY 0
#define MP_MODEL_SIMILARITY 1
#define MP_MODEL_AFFINE 2
int mp_find_transform(mp_handle* h, const int* kp_yx, const int* kp_count, const int* match_idx, int P, int K, int model,
                      double reproj_threshold, int max_iters, unsigned long long seed, double* transform,
                      unsigned char* inlier_mask, int* n_inliers, void* stream);
int mp_find_transform_f(mp_handle* h, const float* kp_sub_yx, const int* kp_count, const int* match_idx, int P, int K, int model,
                        double reproj_threshold, int max_iters, unsigned long long seed, double* transform,
                        unsigned char* inlier_mask, int* n_inliers, void* stream);
int mp_refine_transform(mp_handle* h, const int* kp_yx, const int* kp_count, const int* match_idx, int P, int K, int model,
                        double reproj_threshold, int rounds, double* transform, unsigned char* inlier_mask, int* n_inliers,
                        double* cost /* [P][2] or NULL */, void* stream);
int mp_refine_transform_f(mp_handle* h, const float* kp_sub_yx, const int* kp_count, const int* match_idx, int P, int K, int model,
                          double reproj_threshold, int rounds, double* transform, unsigned char* inlier_mask, int* n_inliers,
                          double* cost /* [P][2] or NULL */, void* stream);
int mp_find_transform_pooled(mp_handle* h, const float* pts, const int* group_offsets, long long N, int G, int model,
                             double reproj_threshold, int max_iters, unsigned long long seed, double* transform,
                             unsigned char* inlier_mask, int* n_inliers, void* workspace, long long workspace_bytes, void* stream);
int mp_refine_transform_pooled(mp_handle* h, const float* pts, const int* group_offsets, long long N, int G, int model,
                               double reproj_threshold, int rounds, double* transform, unsigned char* inlier_mask, int* n_inliers,
                               double* cost /* [G][2] or NULL */, void* stream);

/* ---- single-image detector metrics: multipoint/utils/evaluation.py:10-97 (predict_keypoints.py:88-104) ----
 * mp_detector_metrics replaces compute_tp_fp_dist (evaluation.py:56-97) for B heat maps at once:
 *   prob          fp32 [B][H][W]  detector map after valid mask / NMS (evaluation.py:19-25)
 *   keypoint_map  uint8 [B][H][W] ground-truth label map (nonzero = keypoint; ImagePairDataset 'keypoints')
 * predictions = pixels with prob > zero_threshold (reference default 1e-4), ranked by (prob desc, flat index asc);
 * each prediction names the first ground-truth point in row-major order within distance_thresh (reference default
 * 2.0; must be < 3) and is a true positive iff it is the best-ranked prediction naming that point (the closed form
 * of the reference's greedy loop, :84-93).  Outputs, one record per prediction in arbitrary order:
 *   rec_index int32 [B][H*W] flat pixel index y*W+x;  rec_prob fp32 [B][H*W];
 *   rec_bits uint32 [B][H*W]: bit (dy+2)*5+(dx+2) set for every ground-truth point at offset (dy, dx) within
 *             distance_thresh (the entries of `dist[matches]`, :97), bit 31 = true positive;
 *   rec_count int32 [B] predictions per image;  n_gt int32 [B] ground-truth points per image (`len(kp)`);
 *   work uint64 [B][H][W] scratch. */
int mp_detector_metrics(mp_handle* h, const float* prob, const unsigned char* keypoint_map, int B, int H, int W,
                        float zero_threshold, float distance_thresh, unsigned long long* work, int* rec_index,
                        float* rec_prob, unsigned int* rec_bits, int* rec_count, int* n_gt, void* stream);

/* ---- homographic adaptation: multipoint/utils/homographies.py:38-189, export_keypoints.py:64-103 ----
 * Homographies are device double [n][9], row-major 3x3 acting on pixel coordinates (x, y, 1).
 *
 * mp_warp_perspective replaces WarpingModule / warp_perspective_tensor (homographies.py:404-433; kornia's
 * homography_warp = F.grid_sample(align_corners=True) on the homography in normalised coordinates): single-channel
 * maps src [n_src][H][W] -> dst [n_out][Ho][Wo],  dst[n](x, y) = src[n % n_src] sampled at dst_to_src[n] * (x, y, 1)
 * (dst_to_src = inverse of the M the reference passes); mode 0 bilinear / 1 nearest (half to even);
 * padding 0 zeros / 1 reflection (about pixel centres 0 and size-1). */
int mp_warp_perspective(mp_handle* h, const float* src, int n_src, int H, int W, const double* dst_to_src, int n_out,
                        int Ho, int Wo, int mode, int padding, float* dst, void* stream);

/* replaces cv2.warpPerspective(image, M, (W, H), borderMode=...) with the default INTER_LINEAR, as the dataset's
 * homographic augmentation calls it (multipoint/datasets/augmentation/augmentation.py:33-36): source coordinates in
 * 1/32-pixel fixed point (OpenCV's INTER_BITS = 5), float32 bilinear weight table, block-wise float64 coordinate
 * arithmetic.  src/dst fp32 [n][H][W] (dst != src); hom_inv device double [n][9] = inverse of the M the reference
 * passes (cv2 inverts it first); border 0 = BORDER_CONSTANT (0), 1 = BORDER_REFLECT_101. */
int mp_warp_perspective_cv(mp_handle* h, const float* src, int n, int H, int W, const double* hom_inv, int border,
                           float* dst, void* stream);

/* replaces compute_valid_mask (homographies.py:361-389) for G homographies: cv2.warpPerspective(ones, M, INTER_NEAREST)
 * (1 where the rounded source pixel hom_inv * (x, y, 1) lies in the frame) followed by cv2.erode with a
 * (2*erosion_radius+1)^2 box (erosion_radius <= 16); mask_border != 0 also erodes from the image border.
 * mask: uint8 [G][H][W]. */
int mp_ha_valid_mask(mp_handle* h, const double* hom_inv, int G, int H, int W, int erosion_radius, int mask_border,
                     unsigned char* mask, void* stream);

/* aggregation state of homographic_adaptation(_multispectral): prob, count fp32 [B][H][W].
 * aggregation 0: one map (prob_b NULL); 1 'prod' / 2 'sum' of the optical and thermal maps (homographies.py:63-68).
 *   mp_ha_begin       prob = map(s) of the un-warped images, count = 1                            (:60-68, :149-150)
 *   mp_ha_accumulate  for g < G in order: cs = nearest(mask[g], hom[g]); count += cs;
 *                     prob += bilinear(map[g][b], hom[g]) * cs   (zeros padding)                   (:111-113, :178-180)
 *                     prob_a / prob_b: [G][B][H][W] heat maps of the images warped by hom[g]
 *   mp_ha_finalize    out = prob / count; sqrt (prod) or * 0.5 (sum); 0 where count < min_count    (:115-127, :182-187) */
int mp_ha_begin(mp_handle* h, const float* prob_a, const float* prob_b, int B, int H, int W, int aggregation,
                float* prob, float* count, void* stream);
int mp_ha_accumulate(mp_handle* h, const float* prob_a, const float* prob_b, const unsigned char* mask,
                     const double* hom, int G, int B, int H, int W, int aggregation, float* prob, float* count,
                     void* stream);
int mp_ha_finalize(mp_handle* h, const float* prob, const float* count, int B, int H, int W, int aggregation,
                   float min_count, float* out, void* stream);

/* replaces filter(pad(prob)) (homographies.py:55-58: ReflectionPad2d((k-1)/2) + the k x k depthwise filter of
 * utils.get_gaussian_filter, utils.py:124-160): in/out fp32 [B][H][W], weights device fp32 [k][k], k odd, k <= 31. */
int mp_gaussian_filter(mp_handle* h, const float* in, int B, int H, int W, int ksize, const float* weights, float* out,
                       void* stream);

/* ---- SuperPointLoss, evaluation and gradients (multipoint/utils/losses.py:8-272) ----
 * Shapes: logits fp32 [B][65][Hc][Wc] (mp_forward with force_return_logits); keypoint / valid maps uint8 [B][H][W],
 * nonzero = keypoint / valid pixel; desc1 / desc2 channels-last fp32 [B][Hc][Wc][D] like mp_forward's descriptors;
 * homographies fp32 [B][9] row-major, acting on (x, y, 1).  H == 8 Hc and W == 8 Wc are required (MP_EINVAL otherwise, as
 * for D outside {64, 128, 256}).  Both losses write per-image double results; the caller forms the batch means.  The
 * results are bit-identical from run to run (fixed-order reductions, no float atomics).
 *
 * mp_loss_workspace_bytes: bytes of the caller-owned device workspace both losses need for B images of H x W. */
int mp_loss_workspace_bytes(int B, int H, int W, long long* bytes);

/* replaces SuperPointLoss.detector_loss (losses.py:85-122).  A cell is valid when all 64 of its pixels are (valid == NULL:
 * every cell).  use_cross_entropy 1: label = argmax([3 kp_c + noise_c (c < 64), 2.0]), loss = logsumexp - logit[label];
 * noise fp32 [B][64][Hc][Wc] is the reference's torch.rand draw, or NULL for a counter-based hash of
 * (noise_seed, b, c, h, w).  0: BCE on softmax(logits) against the normalised multi-hot labels plus dustbin (:110-119).
 * out double [B][2]: sum over cells of loss * valid, number of valid cells (loss = mean_b(out[b][0] / out[b][1])). */
int mp_detector_loss(mp_handle* h, const float* logits, int B, int Hc, int Wc, const unsigned char* keypoints,
                     const unsigned char* valid_mask, int H, int W, int use_cross_entropy, const float* noise,
                     unsigned long long noise_seed, void* workspace, long long workspace_bytes, double* out, void* stream);

/* replaces the dense branch of SuperPointLoss.descriptor_loss (losses.py:207-272) without its B x (Hc Wc)^2 tensors:
 * cell centres (8h+4, 8w+4) warped by inverse(hom) (hom NULL: identity), corr = |w1[j] - w2[i]| <= threshold,
 * dot = desc2[i] . desc1[j], pos = lambda_d corr max(0, positive_margin - dot), neg = (1 - corr) max(0, dot - negative_margin),
 * with use_mask both times valid2[i] valid1[j] (cell validity as above; valid NULL: every cell).
 * out double [B][4]: sum pos, sum neg, corresponding valid pairs, normalisation (valid1 cells x valid2 cells with the
 * mask, (Hc Wc)^2 without).  warped: optional fp32 [2][B][Hc Wc][2], the warped centres (y, x) of side 1 then side 2. */
int mp_descriptor_loss(mp_handle* h, const float* desc1, const float* desc2, int B, int Hc, int Wc, int D,
                       const float* hom1, const float* hom2, const unsigned char* valid1, const unsigned char* valid2,
                       int H, int W, float threshold, float positive_margin, float negative_margin, float lambda_d,
                       int use_mask, void* workspace, long long workspace_bytes, double* out, float* warped,
                       void* stream);

/* Gradients of the loss (the backward of the above).  Both entry points are stateless: they take the
 * forward's inputs again plus `forward_out`, the out array the matching forward call wrote, and recompute what they need
 * (labels, cell validity, warped centres).  `coef` is device memory (double), the upstream coefficients, so that a
 * backward never synchronises with the host.  With the upstream gradients g_T, g_det1, g_det2, g_desc, g_pos, g_neg of
 * the batch means total, detector_loss1 / 2, descriptor_loss, positive_dist and negative_dist (lambda = the weight of the
 * descriptor loss in total):  gamma_k = g_T + g_det_k,  alpha = lambda g_T + g_desc + g_pos,  beta = lambda g_T + g_desc
 * + g_neg.  h(x) = 1 for x > 0, 1/2 for x == 0 (torch's maximum backward at a tie), 0 for x < 0; every tie is decided on
 * the kernel's own fp32 value (the dot in the forward's k order).  An image whose count / normalisation is 0 gets NaN
 * gradients (as the reference's division); other images are unaffected.  Results are bit-identical from run to run.
 *
 * mp_detector_loss_backward: coef[0] = gamma; grad_logits fp32 [B][65][Hc][Wc] =
 *   gamma valid / (B count_b) (softmax(z) - onehot(label))                       (cross entropy; label as the forward's)
 *   gamma valid / (B count_b) p (gp - sum_c p_c gp_c), gp_c = (p_c - y_c) / max(p_c (1 - p_c), 1e-12)   (BCE, p = softmax)
 * with count_b = forward_out[b][1] (the forward's double [B][2]).  noise / noise_seed as given to the forward. */
int mp_detector_loss_backward(mp_handle* h, const float* logits, int B, int Hc, int Wc, const unsigned char* keypoints,
                              const unsigned char* valid_mask, int H, int W, int use_cross_entropy, const float* noise,
                              unsigned long long noise_seed, const double* forward_out, const double* coef,
                              void* workspace, long long workspace_bytes, float* grad_logits, void* stream);

/* mp_descriptor_loss_backward: coef[0] = alpha, coef[1] = beta; norm_b = forward_out[b][3] (the forward's double [B][4]).
 * With dot[i][j] = desc2[i] . desc1[j], w[i][j] = valid2[i] valid1[j] (1 without the mask), c = w corr(i, j):
 *   G[i][j] = (-alpha lambda_d c h(positive_margin - dot) + beta (w - c) h(dot - negative_margin)) / (B norm_b)
 *   grad1[j] = sum_i G[i][j] desc2[i],   grad2[i] = sum_j G[i][j] desc1[j]
 * grad1 / grad2 channels-last fp32 [B][Hc][Wc][D] like the descriptors; each cell's gradient is written once (no
 * atomics, nothing of size (Hc Wc)^2).  One of grad1 / grad2 may be NULL: that side is not computed (both NULL: MP_EINVAL).
 * The workspace is mp_loss_workspace_bytes as for the forward. */
int mp_descriptor_loss_backward(mp_handle* h, const float* desc1, const float* desc2, int B, int Hc, int Wc, int D,
                                const float* hom1, const float* hom2, const unsigned char* valid1,
                                const unsigned char* valid2, int H, int W, float threshold, float positive_margin,
                                float negative_margin, float lambda_d, int use_mask, const double* forward_out,
                                const double* coef, void* workspace, long long workspace_bytes, float* grad1,
                                float* grad2, void* stream);

/* ---- photometric augmentation (multipoint/datasets/augmentation/augmentation.py:8-22 and
 * photometric_augmentation.py:13-77) ----
 * n images fp32 [n][H][W] (any H, W), one plan per image drawn on the host (multipoint_amd.datasets.augmentation.
 * draw_photometric_plan: the reference's random / np.random draws in the reference's order).  A plan lists its primitives
 * in the order they run; every op carries its own scalar draw.  Plans and ellipses are HOST memory, copied into the
 * workspace on `stream` (the entry points synchronise `stream` once, after that copy, so the caller may free them on
 * return); the per-pixel noise fields are device memory.
 *   MP_PHOTO_GAUSSIAN_NOISE  additive_gaussian_noise (:13-17): x = clip(float(double(x) + n), 0, 1), n = normal[field] (host
 *                            noise) or value * N(0, 1) from a counter-based hash of (key, pixel) (device noise)
 *   MP_PHOTO_GAUSSIAN_ADD    the in-place `image += noise` of :15 alone, without the clip (an aliased pair's shared input)
 *   MP_PHOTO_SPECKLE         additive_speckle_noise (:19-24): u = uniform[field] or hash(key, pixel); x = 0 where
 *                            u < value, x = 1 where u > 1.0 - value (compared in double)
 *   MP_PHOTO_BRIGHTNESS      random_brightness (:26-28): clip(x + float(value), 0, 1)
 *   MP_PHOTO_CONTRAST        random_contrast (:30-34): m = image.mean() (numpy's float32 sum: pairwise sums of chunks of 8192
 *                            pixels accumulated in order), clip((x - m) * float(value) + m, 0, 1)
 *   MP_PHOTO_SHADE           additive_shade (:36-54): mask = cv2.ellipse fill (thickness -1) of ellipses
 *                            [ellipse_offset, +ellipse_count) (x, y, ax, ay, angle in integer degrees), cv2.GaussianBlur(mask,
 *                            (ksize, ksize), 0) with BORDER_REFLECT_101; clip(x * (1 - float(value) * mask), 0, 1)
 *   MP_PHOTO_MOTION_BLUR     motion_blur (:56-77): cv2.filter2D with the ksize non-zero taps `taps` along the line of `mode`
 *                            (0 'h', 1 'v', 2 'diag_down', 3 'diag_up') in row-major order, BORDER_REFLECT_101
 * Every elementwise step is rounded separately (no fused multiply-add), as numpy computes it. */
#define MP_PHOTO_MAX_OPS 16
#define MP_PHOTO_MAX_TAPS 11
#define MP_PHOTO_MAX_BLUR 801
enum { MP_PHOTO_GAUSSIAN_NOISE = 0, MP_PHOTO_SPECKLE = 1, MP_PHOTO_BRIGHTNESS = 2, MP_PHOTO_CONTRAST = 3, MP_PHOTO_SHADE = 4,
       MP_PHOTO_MOTION_BLUR = 5, MP_PHOTO_GAUSSIAN_ADD = 6 };

typedef struct mp_photometric_op {
    int kind;                       /* MP_PHOTO_* */
    int ksize;                      /* shade: blur kernel size (odd, <= MP_PHOTO_MAX_BLUR); motion blur: taps (odd, <= 11) */
    int mode;                       /* motion blur line */
    int ellipse_offset, ellipse_count;   /* shade: rows of the ellipse table */
    int field;                      /* host noise: plane of the normal / uniform field */
    double value;                   /* stddev | prob | delta | strength | transparency */
    unsigned long long key;         /* device noise: key of the counter-based generator */
    float taps[MP_PHOTO_MAX_TAPS];  /* motion blur weights (float32, row-major order of the non-zero kernel entries) */
    int pad;
} mp_photometric_op;

typedef struct mp_photometric_plan {
    int n_ops;                      /* 0 .. MP_PHOTO_MAX_OPS */
    int noise_device;               /* 0: normal / uniform fields given, 1: drawn on the device from op.key */
    mp_photometric_op op[MP_PHOTO_MAX_OPS];
} mp_photometric_plan;

/* mp_photometric_workspace_bytes: bytes of the caller-owned device workspace of mp_photometric_augment /
 * mp_photometric_shade_mask for n images of H x W with n_ellipses rows in the ellipse table. */
int mp_photometric_workspace_bytes(int n, int H, int W, int n_ellipses, long long* bytes);

/* replaces photometric_augmentation (augmentation.py:8-22) for a batch: out[i] = the plan's primitives applied to in[i] in
 * order.  in == out is allowed.  plans host [n]; ellipses host int32 [n_ellipses][5]; normal / uniform device float64
 * [n_normal][H][W] / [n_uniform][H][W], the reference's np.random.normal / np.random.uniform fields (NULL with 0 planes
 * when every plan draws its noise on the device). */
int mp_photometric_augment(mp_handle* h, const float* in, float* out, int n, int H, int W, const mp_photometric_plan* plans,
                           const int* ellipses, int n_ellipses, const double* normal, int n_normal, const double* uniform,
                           int n_uniform, void* workspace, long long workspace_bytes, void* stream);

/* the shade mask of additive_shade (photometric_augmentation.py:39-51) of op `op_index` of every plan: the filled ellipses
 * (blurred 0) or the mask after cv2.GaussianBlur (blurred 1); zeros for a plan whose op there is not a shade.
 * out fp32 [n][H][W]. */
int mp_photometric_shade_mask(mp_handle* h, int n, int H, int W, const mp_photometric_plan* plans, const int* ellipses,
                              int n_ellipses, int op_index, int blurred, float* out, void* workspace,
                              long long workspace_bytes, void* stream);

/* ---- synthetic shapes (multipoint/utils/draw_primitives.py, multipoint/datasets/SyntheticShapes.py) ----
 * The host draws every random number of an image into a list of draw commands (multipoint_amd/utils/draw_primitives.py);
 * mp_shapes_render replays the lists of n images on their fp32 canvases [n][H][W], command s of every image in the same
 * launches, with OpenCV's integer drawing rules (LINE_8, 16.16 fixed point, spans clipped to the frame):
 *   MP_SHAPES_THRESHOLD  canvas = u > t ? 1 : 0, u = fields[a[0]] (double, host noise) or hash(key, pixel) when a[0] < 0
 *   MP_SHAPES_MEAN       mean[img] = the canvas mean, summed in double; stays on the device (colours resolve against it)
 *   MP_SHAPES_BLOBS      circles a[0] .. a[0] + a[1] - 1 of the circle table, cv2.circle(..., -1) each: a pixel takes the
 *                        colour of the highest-index circle that covers it; a[2] != 0: uncovered pixels take the command's
 *                        colour (the fill below the blobs).  Circle i's colour is circle_colors[i] = (a, b).
 *   MP_SHAPES_BOX_BLUR   cv2.blur(img, (a[0], a[0])): anchor a[0] / 2, BORDER_REFLECT_101 repeated, sums in double
 *   MP_SHAPES_LINE       cv2.line((a[0], a[1]), (a[2], a[3]), thickness a[4])
 *   MP_SHAPES_CONVEX     cv2.fillConvexPoly of vertices a[0] .. a[0] + a[1] - 1 of the vertex table
 *   MP_SHAPES_POLY       cv2.fillPoly of one contour (same fields); a[2] != 0: the covered pixels are copied from the
 *                        image's second canvas instead of taking a colour
 *   MP_SHAPES_ELLIPSE    cv2.ellipse(centre (a[0], a[1]), axes (a[2], a[3]), angle a[4] degrees, 0, 360, colour, -1)
 *   MP_SHAPES_RANDU      canvas = hash(key, pixel), uniform in [0, 1)
 * target 0 is the image's canvas, 1 its second canvas (in the workspace; blobs / box blur only).
 * A colour (a, b) with resolve != 0 is b when |u - mean[img]| < min_contrast and a otherwise; resolve == 0: a. */
enum { MP_SHAPES_THRESHOLD = 0, MP_SHAPES_MEAN = 1, MP_SHAPES_BLOBS = 2, MP_SHAPES_BOX_BLUR = 3, MP_SHAPES_LINE = 4,
       MP_SHAPES_CONVEX = 5, MP_SHAPES_POLY = 6, MP_SHAPES_ELLIPSE = 7, MP_SHAPES_RANDU = 8 };
#define MP_SHAPES_MAX_VERTS 64      /* vertices of one polygon */
#define MP_SHAPES_MAX_RADIUS 255    /* circle radius, line thickness */
#define MP_SHAPES_MAX_BLOBS 15000   /* circles of one MP_SHAPES_BLOBS command (a tile's list holds them all) */
#define MP_SHAPES_MAX_COORD 1048576 /* |coordinate| of a vertex, centre or end point */

typedef struct mp_shapes_cmd {
    int kind;                       /* MP_SHAPES_* */
    int target;                     /* 0: canvas, 1: second canvas */
    int a[6];                       /* per kind, see above */
    int resolve;                    /* colour: 0 literal a, 1 resolved against the device mean */
    int pad;
    double u, col_a, col_b, min_contrast;
    double t;                       /* threshold */
    unsigned long long key;         /* device noise key (threshold with a[0] < 0, randu) */
} mp_shapes_cmd;

/* bytes of the caller-owned device workspace of mp_shapes_render / mp_shapes_finish for n images of H x W */
int mp_shapes_workspace_bytes(int n, int H, int W, int n_cmds, int n_verts, int n_circles, long long* bytes);

/* canvas device fp32 [n][H][W], read and written (a render may continue the canvases of an earlier one); mean device
 * float64 [n], read and written likewise.  cmds host [cmd_offset[n]], image i owning cmds[cmd_offset[i] ..
 * cmd_offset[i + 1]); verts host int32 [n_verts][2] (x, y); circles host int32 [n_circles][3] (x, y, radius);
 * circle_colors host float64 [n_circles][2]; fields device float64 [n_fields][H][W]. */
int mp_shapes_render(mp_handle* h, float* canvas, double* mean, int n, int H, int W, const mp_shapes_cmd* cmds,
                     const int* cmd_offset, const int* verts, int n_verts, const int* circles, const double* circle_colors,
                     int n_circles, const double* fields, int n_fields, void* workspace, long long workspace_bytes,
                     void* stream);

/* SyntheticShapes.py:131-144: cv2.GaussianBlur(canvas, (blur1[i], blur1[i]), 0), then with blur2[i] when it is not 0 (host
 * int arrays [n], odd sizes <= MP_PHOTO_MAX_BLUR; the sepFilter2D restatement of the photometric shade, fp32), in place, then
 * cv2.resize(..., (w, h), INTER_LINEAR) into out fp32 [n][h][w] (a plain copy when h x w is H x W). */
int mp_shapes_finish(mp_handle* h, float* canvas, int n, int H, int W, const int* blur1, const int* blur2, float* out, int oh,
                     int ow, void* workspace, long long workspace_bytes, void* stream);

/* ---- mutual-information alignment (create_dataset/helper_functions/align.py:13-215) ----
 * An EVALUATION is (pair p, bin count n, transform T [9] double, mapping thermal pixels to optical ones):
 *   w   = cv2.warpPerspective(optical[p], inv(T), (W, H), borderValue=-1.0), INTER_LINEAR: the arithmetic of
 *         mp_warp_perspective_cv with taps outside the Ho x Wo source reading -1 and the block width taken from the H x W
 *         destination; the matrix applied to destination pixels is cv_invert3(cv_invert3(T)), the closed-form adjugate
 *         inverse both times (the reference's first inverse is LAPACK's: a last-bits deviation)
 *   jh  = np.histogram2d(w.ravel(), thermal[p].ravel(), bins=(n, 2n)) as numpy >= 2 bins float32 samples: per axis
 *         a = min, b = max (a - 0.5, b + 0.5 when equal), float32 edges e[i] = fl(fl(i (b - a) / n) + a), e[n] = b,
 *         bin = (edges <= v) - 1, v == b in the last bin.  Counts are u32 and exact (integer atomics only)
 *   jh  = scipy.ndimage.gaussian_filter(jh, sigma, mode='constant') in double when sigma > 0 (sigma <= 16)
 *   mi  = sum jh log jh - sum s1 log s1 - sum s2 log s2 of jh = (jh + 2^-52) / sum and its marginals, or normalised
 *         (sum s1 log s1 + sum s2 log s2) / sum jh log jh - 1
 *   value = -mi  (+ the Frobenius norm of T_init - T with a regulariser)
 * The value of an evaluation has the same bits alone, inside any batch and from run to run.
 * optical fp32 [n_pairs][Ho][Wo], thermal fp32 [n_pairs][H][W], transforms device double [n_evals][9]; eval_pair / eval_bins
 * are HOST int arrays [n_evals], copied into the workspace on `stream`, which mp_mi_joint_histogram, mp_mi_objective and
 * mp_mi_refine_begin synchronise once behind that copy.
 * MP_EINVAL: a NULL tensor, sizes that are not positive (frames above 32767 x 32767 or 2^30 pixels), bins outside [1, 256], a
 * pair index outside [0, n_pairs), more than 65535 evaluations or pairs, sigma outside [0, 16], a workspace smaller than
 * mp_mi_workspace_bytes says for the call's evaluations.
 *
 * mp_mi_workspace_bytes: n_thermal_maps = distinct (pair, bins) among the evaluations, max_bins their largest bin count,
 * smoothing != 0 when sigma > 0.  A refinement of P problems counts MP_MI_SLOTS evaluations per problem. */
#define MP_MI_SLOTS 10
#define MP_MI_PARAMS_MAX 9      /* parameters of the largest motion model of a refinement (mp_mi_refine_begin_model) */
int mp_mi_workspace_bytes(int n_evals, int n_pairs, int n_thermal_maps, int H, int W, int max_bins, int smoothing,
                          long long* bytes);

/* counts u32: the n x 2n histogram of evaluation e starts at sum over e' < e of 2 n_e'^2; minmax fp32 [n_evals][2]: min and
 * max of the warped frame; warped fp32 [n_evals][H][W] or NULL.  strategy 0: an LDS copy of the histogram per workgroup
 * for n <= 64, global atomics above; 1 / 2 force one of the two (1 needs n <= 64).  The counts do not depend on it. */
int mp_mi_joint_histogram(mp_handle* h, const float* optical, int Ho, int Wo, const float* thermal, int H, int W, int n_pairs,
                          const int* eval_pair, const int* eval_bins, const double* transforms, int n_evals, int strategy,
                          unsigned int* counts, float* minmax, float* warped, void* workspace, long long workspace_bytes,
                          void* stream);

/* values double [n_evals]; init_transforms device double [n_evals][9] adds the regulariser, NULL: none */
int mp_mi_objective(mp_handle* h, const float* optical, int Ho, int Wo, const float* thermal, int H, int W, int n_pairs,
                    const int* eval_pair, const int* eval_bins, const double* transforms, int n_evals, double sigma,
                    int normalized, const double* init_transforms, double* values, void* workspace, long long workspace_bytes,
                    void* stream);

/* Nelder-Mead over the 9 entries of T for a batch of problems, as scipy.optimize.minimize(method='Nelder-Mead', options=
 * {'adaptive': False}) runs it: initial simplex x0 and per coordinate 1.05 x0[k] (0.00025 where x0[k] == 0), reflection,
 * expansion, outside and inside contraction, shrink; iterations and function calls counted as scipy counts them (the
 * reference's call leaves maxiter = maxfun = 1800, xatol = fatol = 1e-6); success = neither limit was reached.  Equal
 * values keep their order when the simplex is sorted.
 *   mp_mi_refine_begin   problems HOST [n_problems], init_transforms device double [n_problems][9]; the workspace (sized
 *                        for MP_MI_SLOTS * n_problems evaluations) holds the whole state until the next begin on this handle
 *   mp_mi_refine_step    enqueues n_iters rounds: one objective launch over the candidate points of every live problem
 *                        (the simplex at first, then the four candidate points of a step, or the nine shrunk vertices),
 *                        then the decision.  Finished problems cost nothing.  *live (device int) = problems still running
 *                        after the last round.  No host synchronisation: the caller reads *live between calls.
 *   mp_mi_refine_result  transforms double [n_problems][9], values double, iterations / function_calls / success int
 *                        [n_problems]; a problem still running reports its best vertex so far and success 0.
 * A handle runs ONE refinement at a time: its record (where the pieces lie in the workspace, and the caller's `optical`
 * pointer) is kept in the handle, and the next mp_mi_refine_begin on the handle replaces it.  `optical` and the workspace
 * must stay allocated and unchanged from begin to the last step / result; a workspace that was freed must not be handed to
 * step / result again, even if a new allocation has its address.
 * MP_ESTATE: step / result on a workspace other than the one of the handle's latest begin. */
typedef struct mp_mi_problem {
    int pair, bins;                 /* bins in [1, 256] */
    int maxiter, maxfun;            /* scipy's limits (200 * 9 each by default) */
    double xatol, fatol;
} mp_mi_problem;
int mp_mi_refine_begin(mp_handle* h, const float* optical, int Ho, int Wo, const float* thermal, int H, int W, int n_pairs,
                       const mp_mi_problem* problems, const double* init_transforms, int n_problems, double sigma,
                       int normalized, int regularize, void* workspace, long long workspace_bytes, void* stream);
int mp_mi_refine_step(mp_handle* h, void* workspace, int n_iters, int* live, void* stream);
int mp_mi_refine_result(mp_handle* h, void* workspace, double* transforms, double* values, int* iterations,
                        int* function_calls, int* success, void* stream);

/* The same refinement over the n parameters of a motion model (MP_MODEL_*) with a simplex of n + 1 vertices;
 * the objective reads the 3x3 matrix of a parameter vector p, through the same perspective warp:
 *   MP_MODEL_HOMOGRAPHY  n = 9  the nine entries
 *   MP_MODEL_SIMILARITY  n = 4  p = (angle, scale, dx, dy): [[s cos a, s sin a, dx], [-s sin a, s cos a, dy], [0, 0, 1]], the
 *                               reference's decomposed form (create_dataset/helper_functions/align.py:137-139)
 *   MP_MODEL_AFFINE      n = 6  the six entries of the top two rows, row-major; last row (0, 0, 1)
 * Parameters are mapped as they are (no clamping).  scipy's rules are those of mp_mi_refine_begin with n in the place of 9:
 * initial vertex k + 1 = 1.05 x0[k] (0.00025 where x0[k] == 0), the centroid summed vertex by vertex and divided by n.  With
 * `regularize` the Frobenius norm of (matrix of the start parameters - matrix of the candidate) over the nine entries is added.
 *   mp_mi_refine_begin_model   mp_mi_refine_begin's arguments, then `model` and init_params device double [n_problems][n], the
 *                              start.  init_transforms is read only when init_params is NULL and the model is the homography
 *                              (whose parameters are the matrix entries); mp_mi_refine_begin is this with model 0.
 *                              MP_EINVAL also for an unknown model (mp_last_error names it)
 *   mp_mi_refine_result_model  mp_mi_refine_result's arguments, then params double [n_problems][n]: the best vertex itself;
 *                              transforms is its matrix
 *   mp_mi_model_transform      the map alone: transforms double [n_rows][9] of params double [n_rows][n], both on the device
 * mp_mi_refine_step serves every model.  A workspace of the size mp_mi_workspace_bytes returns suffices for every model. */
int mp_mi_refine_begin_model(mp_handle* h, const float* optical, int Ho, int Wo, const float* thermal, int H, int W, int n_pairs,
                             const mp_mi_problem* problems, const double* init_transforms, int n_problems, double sigma,
                             int normalized, int regularize, void* workspace, long long workspace_bytes, void* stream, int model,
                             const double* init_params);
int mp_mi_refine_result_model(mp_handle* h, void* workspace, double* transforms, double* values, int* iterations,
                              int* function_calls, int* success, void* stream, double* params);
int mp_mi_model_transform(mp_handle* h, int model, const double* params, int n_rows, double* transforms, void* stream);

/* ---- image pyramid of the staged alignment (create_dataset/align_images.py:163-171, helper_functions/align.py:485-489;
 * DESIGN.md 3.8.3) ----
 * mp_gaussian_blur: cv2.GaussianBlur(frame, (ksize, ksize), 0) of n fp32 frames in [n][H][W], the float path of sepFilter2D:
 *   weights  getGaussianKernel(ksize, 0, CV_32F): for ksize 1, 3, 5, 7 the fixed tables [1], [.25 .5 .25],
 *            [.0625 .25 .375 .25 .0625], [.03125 .109375 .21875 .28125 .21875 .109375 .03125]; above that
 *            sigma = 0.3 ((ksize - 1) / 2 - 1) + 0.8, exp in double, stored as float, normalised by the double sum
 *   rows     sum over the taps from left to right, w[0] x[-r] first
 *   columns  w[r] S[0], then w[r + j] (S[+j] + S[-j]) for j = 1 .. r
 *   border   BORDER_REFLECT_101; every product and sum is rounded to fp32 (no FMA)
 * decimate 0: out [n][H][W].  decimate != 0: out [n][(H + 1) / 2][(W + 1) / 2], the even rows and columns of that result bit
 * for bit (the reference's [::2, ::2]); only those pixels are computed.  No workspace; in and out must not overlap.
 * MP_EINVAL: a NULL tensor, in == out, an even ksize or one outside [1, 31], ksize / 2 >= min(H, W), n outside [1, 65535],
 * H or W outside [1, 32767].
 * mp_gaussian_weights writes the ksize weights (host memory; needs no device); MP_EINVAL for a ksize as above or NULL. */
int mp_gaussian_weights(int ksize, float* weights);
int mp_gaussian_blur(mp_handle* h, const float* in, int n, int H, int W, int ksize, int decimate, float* out, void* stream);

/* 8- and 16-bit frames as the reference turns them into fp32 (align.py:485, align_images.py:161): out fp32 [n][H][W] from
 *   MP_FRAMES_U8    uint8 [n][H][W]:      v / 255.0f
 *   MP_FRAMES_BGR8  uint8 [n][H][W][3]:   each channel / 255.0f, then COLOR_BGR2GRAY (0.114f B + 0.587f G) + 0.299f R
 *   MP_FRAMES_U16   uint16 [n][H][W]:     v / 65535.0f
 * MP_EINVAL: a NULL tensor, another mode, n outside [1, 65535], H or W outside [1, 32767]. */
#define MP_FRAMES_U8 0
#define MP_FRAMES_BGR8 1
#define MP_FRAMES_U16 2
int mp_frames_to_float(mp_handle* h, const void* in, int mode, int n, int H, int W, float* out, void* stream);

/* ---- frame preparation (create_dataset/extract_images.py:167-242, preprocess_images; DESIGN.md 3.13 is the specification) ----
 * Batches of n frames on the caller's stream; K, D and K_new are HOST arrays (K, K_new: 3 x 3 row-major, of which fx, fy, cx, cy
 * are read; D: k1, k2, p1, p2[, k3]).
 *
 * mp_undistort: cv2.undistort(src, K, D, None, K_new) of uint8 [n][H][W][3] (MP_FRAMES_BGR8) or uint16 [n][H][W] (MP_FRAMES_U16).
 * Per destination pixel (u, v), float64, + - * / only, nothing contracted: x = (u - cx') / fx', y = (v - cy') / fy',
 * r2 = x x + y y, kr = 1 + ((k3 r2 + k2) r2 + k1) r2, xd = x kr + p1 (2 x y) + p2 (r2 + 2 x x),
 * yd = y kr + p1 (r2 + 2 y y) + p2 (2 x y), us = fx xd + cx, vs = fy yd + cy; iu = rint(32 us), iv = rint(32 vs) (half to even,
 * saturated to int32), first tap (iv >> 5, iu >> 5), fractions ax = iu & 31, ay = iv & 31.  Taps (sy, sx), (sy, sx + 1),
 * (sy + 1, sx), (sy + 1, sx + 1) with weights (32 - ax)(32 - ay), ax (32 - ay), (32 - ax) ay, ax ay over 1024; a tap outside
 * the frame reads 0.  8 bit: weights x 32, (sum + 16384) >> 15 per channel.  16 bit: float weights w / 1024, products summed in
 * that order in fp32 (no FMA), rint half to even, saturated to [0, 65535].  rotate180 != 0 writes the result rotated by 180
 * degrees ([..., ::-1, ::-1]).
 * MP_EINVAL: a NULL argument, src == dst, another dtype, n_coeffs other than 4 or 5, a non-finite parameter, a zero focal
 * length in K_new, n outside [1, 65535], H or W outside [1, 32767], more than 2^38 pixels, dst not 4-byte aligned. */
int mp_undistort(mp_handle* h, const void* src, int dtype, int n, int H, int W, const double* K, const double* D, int n_coeffs,
                 const double* K_new, int rotate180, void* dst, void* stream);

/* cv2.resize(src, (ow, oh)), INTER_LINEAR, of uint8 [n][H][W][3] into [n][oh][ow][3]: OpenCV's 11-bit fixed-point path.  Per
 * axis: f = (float)((d + 0.5) (in / out) - 0.5) with the product in float64, i = floor(f), f -= i; i < 0: i = 0, f = 0;
 * i >= in - 1: i = in - 1, f = 0; a1 = rint(2048 f), a0 = rint(2048 (1 - f)), both saturated to int16.  S = v[i] a0 + v[i + 1] a1
 * along the row, then (((b0 (S0 >> 4)) >> 16) + ((b1 (S1 >> 4)) >> 16) + 2) >> 2 saturated to uint8.
 * MP_EINVAL: a NULL tensor, src == dst, a size outside the ranges above, dst not 4-byte aligned. */
int mp_resize_bgr8(mp_handle* h, const unsigned char* src, int n, int H, int W, int oh, int ow, unsigned char* dst, void* stream);

/* The thermal frame's rescale, per image of uint16 [n][H][W]:
 *   bounds    lower = np.percentile(x, 1), upper = np.percentile(x, 99) (linear method, float64) from the exact order statistics;
 *             outlier_rejection == 0: no bounds, nothing is clipped
 *   clipped   (may be `in`, may be NULL) x < lower -> trunc(lower), then x > upper -> trunc(upper)
 *   rescaled  fp32: cv2.normalize(clipped, 0, 1, NORM_MINMAX, CV_32F): scale = 1 / (max - min) in float64 (0 when max - min <=
 *             DBL_EPSILON), shift = -min scale, out = (float)v (float)scale + (float)shift, a separate multiply and add
 *   saved     (may be NULL) uint16: (rescaled * 65535).astype(uint16): fp32 product, truncated, the low 16 bits
 * The workspace (mp_thermal_rescale_workspace_bytes, 16-byte aligned) is scratch; it is zeroed on the stream by the call.
 * MP_EINVAL: a NULL in / rescaled / workspace, saved aliasing in or clipped, sizes as above, a small or misaligned workspace. */
int mp_thermal_rescale_workspace_bytes(int n, long long* bytes);
int mp_thermal_rescale(mp_handle* h, const unsigned short* in, int n, int H, int W, int outlier_rejection, unsigned short* clipped,
                       float* rescaled, unsigned short* saved, void* workspace, long long workspace_bytes, void* stream);

/* ---- result views as pictures (show_keypoints.py, show_image_pair_sample.py, the drawing of predict_keypoints.py:159-280 and
 * predict_align_image_pair.py:197-254, create_dataset/check_alignment.py; DESIGN.md 3.14 is the specification) ----
 * Canvases are uint8 [B][Hc][Wc][3], RGB, contiguous, owned by the caller.  Every entry queues its launches on `stream` and
 * returns; list lengths are read on the device.  Every pixel write is checked against the canvas: what falls outside is
 * clipped, what nothing covers keeps its value.  Centre + offset is added in 64 bits.  A result does not depend on the launch
 * shape or on the order in which workgroups run.
 * MP_EINVAL for all four: a NULL tensor (the optional ones excepted), B / P outside [1, 65535], a frame or canvas side outside
 * [1, 32767], K outside [1, 2^20], and what each entry lists.
 *
 * The 8-bit value of a fp32 one, u8(g): NaN -> 0, clamped to [0, 1], (uint8)(c * 255.0f) with one fp32 product, truncated --
 * numpy's (np.clip(g, 0, 1) * 255.0).astype(np.uint8).
 *
 * mp_draw_gray_to_rgb: B fp32 frames [B][H][W] as grey pixels at canvas offset (y0, x0): v = x, or the fp32 product x * m with
 * `mask` (fp32 [B][H][W], may be NULL); g = the fp32 product v * gain; all three channels = u8(g).  Canvas pixels outside the
 * frame are not written. */
int mp_draw_gray_to_rgb(mp_handle* h, const float* images, const float* mask, int B, int H, int W, float gain,
                        unsigned char* canvas, int Hc, int Wc, int y0, int x0, void* stream);

/* mp_draw_marks: one layer of marks.  kp_yx int32 [B][K][2] (y, x), kp_count int32 [B] (a count above K means K, a negative
 * one 0; only that many entries are read).  With half_r[k] the half widths of OpenCV's Circle() walk of radius r (the widest
 * span it draws on the rows cy -+ k):
 *   disc(c, r)     {(x, y): |y - cy| <= r, |x - cx| <= half_r[|y - cy|]}; r = 0 is the centre pixel
 *   MP_DRAW_RING   disc(c, radius + thickness / 2) without disc(c, radius - (thickness + 1) / 2) (empty for a negative radius)
 *   MP_DRAW_DISC   disc(c, radius)
 *   MP_DRAW_CROSS  the centre row and the centre column within +-radius
 * (integer divisions; disc and cross do not read the thickness).  Mark i has its centre at keypoint i + (y0, x0); a pixel takes
 * palette[i mod n_colors] (uint8 [n_colors][3]) of the HIGHEST i covering it.
 * MP_EINVAL: another kind, radius < 0, thickness < 1, outer radius (radius + thickness / 2 for a ring) above
 * MP_DRAW_MAX_RADIUS, n_colors < 1. */
#define MP_DRAW_MAX_RADIUS 64
#define MP_DRAW_RING 0
#define MP_DRAW_DISC 1
#define MP_DRAW_CROSS 2
int mp_draw_marks(mp_handle* h, const int* kp_yx, const int* kp_count, int B, int K, int kind, int radius, int thickness,
                  const unsigned char* palette, int n_colors, unsigned char* canvas, int Hc, int Wc, int y0, int x0, void* stream);

/* mp_draw_matches: one layer of matches per pair on a canvas that shows both images.  kp_a, kp_b int32 [P][K][2] (y, x) with
 * count_a, count_b int32 [P]; match_idx int32 [P][K]: the index into kp_b that kp_a's entry q is matched to, or -1; draw_mask
 * uint8 [P][K] or NULL.  Primitive q exists when q < min(count_a, K), 0 <= match_idx[q] < min(count_b, K) and draw_mask is NULL
 * or non-zero at q; nothing else is read.  With A = kp_a[q] + (ya, xa) and B = kp_b[match_idx[q]] + (yb, xb) it covers the rings
 * (MP_DRAW_RING at radius / thickness) around A and B and the LINE_8 segment A -> B: cv2.line at thickness 1, i.e. clipLine to
 * the canvas and then the LineIterator from the left end, the rule of MP_SHAPES_LINE.  A pixel takes palette[q mod n_colors] of
 * the HIGHEST q covering it.  The order is kept in an owner map (uint32 per canvas pixel, atomicMax(q + 1)) in the handle's
 * grow-only workspace, cleared on `stream` at the start of the call; a buffer it outgrows stays allocated until mp_destroy.
 * One call at a time per handle.
 * MP_EINVAL: radius < 0, thickness < 1, outer radius above MP_DRAW_MAX_RADIUS, n_colors < 1.  MP_ENOMEM: the owner map. */
int mp_draw_matches(mp_handle* h, const int* kp_a, const int* kp_b, const int* count_a, const int* count_b, const int* match_idx,
                    const unsigned char* draw_mask, int P, int K, int ya, int xa, int yb, int xb, int radius, int thickness,
                    const unsigned char* palette, int n_colors, unsigned char* canvas, int Hc, int Wc, void* stream);

/* mp_segments_draw: a list of line segments per canvas (the needle map of the residual field).  segments int32
 * [B][N][MP_DRAW_SEGMENT_INTS] rows of (y0, x0, y1, x1, colour), seg_count int32 [B]: the first min(seg_count[b], N) rows of canvas b
 * exist.  Segment i covers, for every pixel (x, y) of mp_draw_matches' line walk from (x0, y0) to (x1, y1) -- clipLine to the canvas,
 * then the LineIterator from the left end; a zero-length segment is its one pixel -- the box [x - (t - 1) / 2, x + t / 2] x
 * [y - (t - 1) / 2, y + t / 2] for thickness t, clipped to the canvas.  A pixel takes palette[colour mod n_colors] of the HIGHEST i
 * covering it, through the owner map of mp_draw_matches (one call at a time per handle).
 * MP_EINVAL: a NULL tensor, B outside [1, 65535], a canvas side outside [1, 32767], N outside [1, 2^20], thickness outside
 * [1, MP_DRAW_MAX_THICKNESS], n_colors < 1.  MP_ENOMEM: the owner map. */
#define MP_DRAW_SEGMENT_INTS 5
#define MP_DRAW_MAX_THICKNESS 15
int mp_segments_draw(mp_handle* h, const int* segments, const int* seg_count, int B, int N, int thickness,
                     const unsigned char* palette, int n_colors, unsigned char* canvas, int Hc, int Wc, void* stream);

/* mp_draw_compose: alignment views of a warped optical frame and a thermal frame, both fp32 [B][H][W], at canvas offset
 * (y0, x0).  T = u8(thermal); a pixel with warped < 0 (the -1 border of mp_mi_joint_histogram's warp) is outside: A = 0 there,
 * A = u8(warped) elsewhere.
 *   MP_DRAW_BLEND       (A alpha + T (256 - alpha) + 128) >> 8 on all channels
 *   MP_DRAW_CHECKER     A where x / cell + y / cell is even, else T (frame coordinates, integer divisions)
 *   MP_DRAW_ANAGLYPH    (R, G, B) = (A, T, T)
 *   MP_DRAW_DIFFERENCE  |A - T| on all channels
 * In blend, checker and difference an outside pixel shows (T, T, T).
 * MP_EINVAL: another mode, alpha outside [0, 256], cell < 1. */
#define MP_DRAW_BLEND 0
#define MP_DRAW_CHECKER 1
#define MP_DRAW_ANAGLYPH 2
#define MP_DRAW_DIFFERENCE 3
int mp_draw_compose(mp_handle* h, const float* warped, const float* thermal, int B, int H, int W, int mode, int alpha, int cell,
                    unsigned char* canvas, int Hc, int Wc, int y0, int x0, void* stream);

/* ---- 2-D FFT and the LGHD baseline (multipoint/models/ClassicDetectors.py, class LGHD) ----
 * Line lengths are 2^a 3^b 5^c in [8, 4096] (mp_fft_supported); complex arrays are interleaved fp32 (re, im).
 *
 * mp_fft2d: unnormalised DFT of `planes` frames of H x W complex values along the rows (axes 1, length W), the columns
 * (axes 2, length H) or both (3); inverse != 0 conjugates the kernel (no 1 / N).  in == out is allowed.
 * MP_EINVAL: a transformed length outside the supported set, planes outside [1, 65535]. */
int mp_fft_supported(int n);
int mp_fft2d(mp_handle* h, const float* in, float* out, int planes, int H, int W, int inverse, int axes, void* stream);

/* u8[i] = (uint8)(image[i] * 255.0f): the reference's (image * 255.0).astype(np.uint8), one fp32 multiply then truncation */
int mp_lghd_quantize(mp_handle* h, const float* image, unsigned char* u8, long long n, void* stream);

/* FAST-9/16, threshold 10, with non-maximum suppression.  Circle (dx, dy): (0,3) (1,3) (2,2) (3,1) (3,0) (3,-1) (2,-2) (1,-3)
 * (0,-3) (-1,-3) (-2,-2) (-3,-1) (-3,0) (-3,1) (-2,2) (-1,3); only 3 <= y <= H-4, 3 <= x <= W-4 are tested.
 *   score    u8 [B][H][W]: the largest t for which 9 contiguous circle pixels (wrapping) are all > p + t or all < p - t,
 *            0 where that is below 10
 *   corners  u8 [B][H][W]: 1 where score > 0 and strictly above the scores of all 8 neighbours
 *   prob     fp32 [B][H][W] or NULL: 1.0 at corners with 20 <= y <= H-20 and 20 <= x <= W-20 (the descriptor's patch lies
 *            inside the frame), 0 elsewhere */
int mp_lghd_detect(mp_handle* h, const unsigned char* u8, int B, int H, int W, unsigned char* score, unsigned char* corners,
                   float* prob, void* stream);

/* orientation u8 [B][4][H][W]: for scale sc the first o in [0, 6) that maximises |ifft2(fft2(u8) * bank[sc * 6 + o])|.
 * bank fp32 [24][H][W] (real, in FFT order).  The workspace holds the spectrum and the 24 half-transformed planes of as many
 * images as fit (at least one): mp_lghd_workspace_bytes sizes it for min(B, 4).
 * MP_EINVAL: H or W outside the FFT's lengths, B outside [1, 65535], a workspace smaller than one image needs. */
int mp_lghd_workspace_bytes(int B, int H, int W, long long* bytes);
int mp_lghd_orientation(mp_handle* h, const unsigned char* u8, const float* bank, int B, int H, int W,
                        unsigned char* orientation, void* workspace, long long workspace_bytes, void* stream);

/* The 384 patch-histogram counts of every keypoint: rows [y-20, y+20) x columns [x-20, x+20) of the four orientation planes in
 * 4 x 4 cells of 10 x 10 pixels, laid out [scale][cell row][cell col][orientation].  kp_yx int32 [B][K][2], kp_count int32 [B];
 * raw fp32 [B][K][384] exact counts, unit the same rows L2-normalised; either may be NULL.  Rows beyond kp_count, and keypoints
 * whose patch leaves the frame, are zero. */
int mp_lghd_describe(mp_handle* h, const unsigned char* orientation, int B, int H, int W, const int* kp_yx, const int* kp_count,
                     int K, float* raw, float* unit, void* stream);

/* ---- SIFT baseline (Lowe 2004 with the constants of opencv-contrib 4.2's sift.cpp; DESIGN.md 3.19, not verified against OpenCV) ----
 * u8 [B][H][W] is the quantised frame (mp_lghd_quantize).  Every intermediate buffer lies in ONE caller-provided workspace of
 * mp_sift_workspace_bytes(B, H, W, capacity) bytes; `capacity` is the number of slots per image of the candidate list and of the
 * oriented-keypoint list, and every call on one workspace passes the same (B, H, W, capacity).  Nothing is read back between
 * the stages, and results are bit-identical from run to run.
 * MP_EINVAL (all entries): H or W below 16 or above 4096, B outside [1, 65535], capacity outside [1, 2^24], a workspace that is
 * too small, NULL tensors.
 *
 * mp_sift_layout: where the tests find the stages' results in the workspace -- layout[0] octaves; layout[1..4] byte offsets of the
 * candidate list int32 [B][capacity][4] (octave, layer, row, column), its counts int32 [B], the oriented list fp32 [B][capacity][6]
 * (the record below in doubled-base coordinates) and its counts int32 [B] (both counts may exceed the capacity: overflow);
 * layout[5..7] per candidate slot: fp32 [B][capacity][5] x, y, size, response, octave * 8 + layer; int32 [B][capacity] emitted
 * orientations (0: rejected or no peak); int32 [B][capacity][4] final row, final column, peak bins 0..17 and 18..35 as bit masks;
 * layout[8 + 4 o ..]: height, width of octave o and the byte offsets of its Gaussian planes fp32 [B][6][h][w] and difference
 * planes fp32 [B][5][h][w].  layout holds 8 + 4 * 16 values.
 *
 * mp_sift_scale_space: the Gaussian and difference-of-Gaussian pyramids of u8 into the workspace.
 *
 * mp_sift_detect: scale space (skipped when u8 is NULL: the workspace's pyramids are used), candidates, refinement + orientation,
 * duplicate removal and the nfeatures largest responses in list order (octave, layer, row, column of the candidate, then
 * orientation bin; a tie at the cut goes to the earlier entry).  1 <= nfeatures <= N.
 *   keypoints  fp32 [B][N][6]: x, y, size (frame coordinates), angle (degrees), response, octave * 8 + layer; rows beyond count zero
 *   count      int32 [B]
 *   flags      int32 [B]: MP_SIFT_FLAG_CANDIDATES (1) / MP_SIFT_FLAG_KEYPOINTS (2) when a list outgrew the capacity; its entries
 *              beyond the capacity were dropped from the end
 *
 * mp_sift_select: the selection step alone on records fp32 [B][M][6] in doubled-base coordinates (rec_count [B], clipped to M):
 * an entry whose x, y, size and angle equal an earlier one's is dropped, then the nfeatures largest responses are kept in list
 * order and x, y, size are halved.  scratch: B * M bytes.
 *
 * mp_sift_describe: desc fp32 [B][N][128], the 4 x 4 x 8 histograms of the records in keypoints [B][N][6] (as mp_sift_detect writes
 * them), read from the Gaussian pyramid in the workspace: values 0 .. 255, laid out [row][column][orientation]; rows beyond
 * count [b] are zero.
 *
 * mp_sift_scatter: prob fp32 [B][1][H][W] = 1.0 at (round(y), round(x)) of every keypoint, 0 elsewhere; owner int32 [B][H][W] = the
 * largest list index that rounds to the pixel, -1 elsewhere (the last in list order owns the pixel's descriptor). */
#define MP_SIFT_FLAG_CANDIDATES 1
#define MP_SIFT_FLAG_KEYPOINTS 2
int mp_sift_workspace_bytes(int B, int H, int W, int capacity, long long* bytes);
int mp_sift_layout(int B, int H, int W, int capacity, long long* layout);
int mp_sift_scale_space(mp_handle* h, const unsigned char* u8, int B, int H, int W, int capacity, void* workspace,
                        long long workspace_bytes, void* stream);
int mp_sift_detect(mp_handle* h, const unsigned char* u8, int B, int H, int W, int capacity, int nfeatures, void* workspace,
                   long long workspace_bytes, float* keypoints, int* count, int* flags, int N, void* stream);
int mp_sift_select(mp_handle* h, const float* records, const int* rec_count, int B, int M, int nfeatures, float* keypoints, int* count,
                   int N, void* scratch, long long scratch_bytes, void* stream);
int mp_sift_describe(mp_handle* h, int B, int H, int W, int capacity, const void* workspace, long long workspace_bytes,
                     const float* keypoints, const int* count, int N, float* desc, void* stream);
int mp_sift_scatter(mp_handle* h, const float* keypoints, const int* count, int B, int N, int H, int W, float* prob, int* owner,
                    void* stream);

/* ---- Fourier-Mellin registration: a keypoint-free similarity between two frames ----
 * The stages around mp_fft2d.  Complex planes are interleaved fp32 (re, im); every table is the caller's, computed in double
 * and rounded once to fp32.  No entry uses float atomics: results are bit-identical from run to run.
 *
 * mp_register_prepare: frames fp32 [n][H][W] -> out complex [n][N][N], N >= max(H, W), imaginary part 0.  The H x W window sits at
 * row (N - H) / 2, column (N - W) / 2 (integer divisions) of a zeroed plane.  For a window pixel (x, y) the taps (x +- 1, y) and
 * (x, y +- 1) are mapped through the frame's similarity about its centre (cx, cy) = ((W - 1) / 2, (H - 1) / 2) --
 *   sx = fmaf(c, px - cx, fmaf(-s, py - cy, cx)),  sy = fmaf(s, px - cx, fmaf(c, py - cy, cy)),  (c, s) = cs[frame] or (1, 0)
 * for cs == NULL -- and sampled bilinearly; the pixel is sqrt(gx^2 + gy^2) wy[y] wx[x] with gx, gy half the tap differences, or
 * 0 when one of the 16 source samples lies outside the frame (floor(sx) outside [0, W - 2], floor(sy) outside [0, H - 2]).
 * wy [H], wx [W]: the window tables.
 *
 * mp_register_logpolar: spectrum complex [n][N][N] in FFT order -> out complex [n][A][R], imaginary part 0:
 * log1p|F| of the fftshifted spectrum (value i of it is bin (i - N / 2) mod N) sampled bilinearly, indices modulo N, at
 * x = fmaf(rho[r], ca[a], N / 2), y = fmaf(rho[r], sa[a], N / 2), times wr[r].  ca, sa [A]; rho, wr [R].
 *
 * mp_register_cross_power: a, b complex [P][hh][ww], group_offsets int32 [G + 1] non-decreasing (as mp_pool_matches writes
 * them; clamped to [0, P]) -> out complex [G][hh][ww]: per bin the sum, in pair order, of X / |X| with X = a conj(b) over the
 * group's pairs (0 where |X| == 0).  Bin (0, 0) is 0; an empty group gives zeros.  accumulate != 0: the sums start from the
 * values in `out`, so a batch fed in several calls gives the bits of one call.
 *
 * mp_register_peak: planes [G][hh][ww], 3 <= hh, ww <= 4096, values `stride` floats apart (1: real planes, 2: the real part of
 * complex planes).  out_i int32 [G][2]: row and column of the maximum, the first in row-major order on a tie.  out_f fp32
 * [G][6]: the row and column offsets 0.5 (l - r) / (l - 2 c + r) of a parabola through the maximum and its wrapped neighbours
 * (0 where the second difference is 0); row and column folded to signed form (an index above hh / 2 or ww / 2 has the size
 * subtracted) plus the offset; the maximum; the largest value outside the wrapped 3 x 3 block around it (-inf if there is
 * none).  Two-stage reduction over chunks of 16384 values with the same tie rule in both; the workspace holds the chunks'
 * results (mp_register_peak_workspace_bytes).
 * MP_EINVAL (all entries): NULL tensors, n, G outside [1, 65535], sizes outside the ranges above. */
int mp_register_prepare(mp_handle* h, const float* frames, const float* cs, const float* wy, const float* wx, int n, int H, int W,
                        int N, float* out, void* stream);
int mp_register_logpolar(mp_handle* h, const float* spectrum, int n, int N, const float* ca, const float* sa, const float* rho,
                         const float* wr, int A, int R, float* out, void* stream);
int mp_register_cross_power(mp_handle* h, const float* a, const float* b, const int* group_offsets, int P, int G, int hh, int ww,
                            int accumulate, float* out, void* stream);
int mp_register_peak_workspace_bytes(int G, int hh, int ww, long long* bytes);
int mp_register_peak(mp_handle* h, const float* planes, int G, int hh, int ww, int stride, int* out_i, float* out_f,
                     void* workspace, long long workspace_bytes, void* stream);

/* ---- ECC direct alignment: Gauss-Newton maximisation of the enhanced correlation coefficient ----
 * A transform is a 3x3 float64 matrix, row-major, that maps a template (thermal) pixel to an image (optical) pixel.
 *
 * mp_ecc_prepare: blurred fp32 [n][H][W] -> feat fp32 [n][H][W] and, if packed != NULL, packed fp32 [n][H][W][4] (16-byte
 * aligned).  feature MP_ECC_GRADIENT: feat = sqrtf(fmaf(gx, gx, gy * gy)) with gx = 0.5f * (f[x + 1] - f[x - 1]), gy likewise
 * along rows, BORDER_REFLECT_101 (both 0 on the border lines); MP_ECC_INTENSITY: feat = blurred.  packed holds (feat, gx, gy, 0)
 * per pixel, gx and gy taken from feat by the same rule: the image side of the sums pass, one 16-byte load per bilinear tap.
 *
 * mp_ecc_sums: the raw sums of n_problems (pair[q] host int32, transforms[q] device float64 [9]) -> sums device float64
 * [n_problems][S], S = 6 + K + K (K + 1) / 2 + 2 K for the K parameters of `model` (MP_MODEL_HOMOGRAPHY 8, _AFFINE 6, _SIMILARITY
 * 4: a, b, tx, ty of [[a, -b, tx], [b, a, ty]], _TRANSLATION 2).  The nine entries are rounded once to fp32; for template pixel
 * (x, y): X = fmaf(T00, x, fmaf(T01, y, T02)), Y and D likewise from rows 1 and 2, xs = X / D, ys = Y / D.  The pixel is valid iff
 * 0 <= floor(xs) <= Wo - 2 and 0 <= floor(ys) <= Ho - 2 (a NaN fails).  w, gx, gy: the bilinear sample of packed (per component
 * top = fmaf(fx, p01 - p00, p00), bot likewise, fmaf(fy, bot - top, top)); r the template value; G_k the fp32 Jacobian columns
 * of DESIGN.md 3.21.  Order of the sums: n, w, r, w w, r r, w r, G_k (K), G_k G_l for k <= l row by row, G_k w (K), G_k r (K);
 * every product is the exact float64 product of its fp32 factors, added in float64.  One workgroup adds MP_ECC_CHUNK = 4096
 * consecutive template pixels; the order depends on (problem, pixel index) alone, so a problem has the same bits in any batch.
 *
 * mp_ecc_begin / mp_ecc_step / mp_ecc_result: the batched refinement.  begin takes the start matrices (device float64
 * [n_problems][9], divided by their T22 here; a constrained model reads its parameters from them: similarity a = T00, b = T10).
 * step enqueues n_iters iterations -- one sums launch, one solve launch -- without synchronising and then writes the number of
 * problems still running to *live (device int32).  result: transforms [P][9], rho [P] float64; nit, status, converged int32 [P].
 * A problem stops with status MP_ECC_OK when |rho - rho_prev| < eps (converged = 1) or after maxiter updates (converged = 0);
 * with MP_ECC_FEW_VALID when fewer than min_valid H W pixels are valid, MP_ECC_NOT_POSITIVE when the Cholesky factorisation of
 * G^T G fails, MP_ECC_LAMBDA when lambda's denominator is <= 0, MP_ECC_NONFINITE on a non-finite value; it keeps its last iterate.
 * The workspace (mp_ecc_workspace_bytes) must stay untouched between begin and result.
 * MP_EINVAL: a NULL tensor, frames outside 8 x 8 .. 4096 x 4096, n, n_pairs outside [1, 65535], n_problems outside
 * [1, MP_ECC_MAX_PROBLEMS], a pair index outside [0, n_pairs), an unknown model or feature, eps < 0 or NaN, maxiter < 1, min_valid
 * outside [0, 1], n_iters outside [1, 100000], a small workspace.  MP_ESTATE: step / result on a workspace other than the one of
 * the handle's latest begin. */
#define MP_MODEL_TRANSLATION 3      /* mp_ecc_* only */
#define MP_ECC_GRADIENT 0
#define MP_ECC_INTENSITY 1
#define MP_ECC_MAX_PROBLEMS 4096
#define MP_ECC_OK 0
#define MP_ECC_FEW_VALID 1
#define MP_ECC_NOT_POSITIVE 2
#define MP_ECC_LAMBDA 3
#define MP_ECC_NONFINITE 4
int mp_ecc_workspace_bytes(int n_problems, int H, int W, long long* bytes);
int mp_ecc_prepare(mp_handle* h, const float* blurred, int n, int H, int W, int feature, float* feat, float* packed, void* stream);
int mp_ecc_sums(mp_handle* h, const float* packed, int Ho, int Wo, const float* thermal, int H, int W, int n_pairs, const int* pair,
                const double* transforms, int n_problems, int model, double* sums, void* workspace, long long workspace_bytes,
                void* stream);
int mp_ecc_begin(mp_handle* h, const float* packed, int Ho, int Wo, const float* thermal, int H, int W, int n_pairs,
                 const int* pair, const double* init_transforms, int n_problems, int model, double eps, int maxiter,
                 double min_valid, void* workspace, long long workspace_bytes, void* stream);
int mp_ecc_step(mp_handle* h, void* workspace, int n_iters, int* live, void* stream);
int mp_ecc_result(mp_handle* h, void* workspace, double* transforms, double* rho, int* iterations, int* status, int* converged,
                  void* stream);

/* ---- Pooled ECC: one transform per group of pairs, static masks, per-pair correlations ----
 * Features, motion models, per-pixel terms, the raw sums and their order are those of mp_ecc_*.  A pair is one optical and one
 * thermal frame with the same index; group[p] (host int32 [n_pairs]) names the group whose transform T_g it shares.  Every mask
 * is a uint8 plane, nonzero = use.
 *
 * mp_ecc_mask_grow: masks [n][H][W] -> out [n][H][W], 0 at every pixel within Chebyshev distance `radius` of a 0 of the input
 * (clipped at the frame, no reflection; radius 0 copies zero / nonzero as 0 / 1; a radius larger than the frame is allowed), else
 * 1.  tmp [n][H][W] holds the row pass.  The template's masks are grown by R_t = ksize / 2 + 1 for MP_ECC_GRADIENT, ksize / 2 for
 * MP_ECC_INTENSITY, the image's by R_t + 1 (the packed plane differentiates the feature frame once more).
 * mp_ecc_static_update: the running minimum lo and maximum hi (fp32 [H][W]) of every pixel over frames fp32 [n][H][W]; first != 0
 * starts them from frames[0], so the frames of a recording may arrive in any number of batches.  mp_ecc_static_finish: mask =
 * 0 where lo == hi, else 1: a pixel that never changed is excluded.
 * mp_ecc_flag_packed: writes 1.0f into the fourth component of packed [n][H][W][4] where the mask of the frame is 0: masks
 * [n_masks][H][W], mask_of_frame host int32 [n] (-1: the frame has none).  Run it after mp_ecc_prepare, with grown masks.
 *
 * mp_ecc_pooled_sums: the raw sums of every pair at the transform of its group (transforms device float64 [n_groups][9]) -> sums
 * device float64 [n_pairs][S] as mp_ecc_sums, over the valid pixels whose template pixel is kept by the group's thermal mask
 * (thermal_masks [n_masks][H][W] grown, mask_of_group host int32 [n_groups], -1 or a NULL list: none) and whose four bilinear taps
 * all have a zero fourth component.  Skipped pixels count in no sum.  With no mask the sums of a pair have the bits of mp_ecc_sums.
 *
 * mp_ecc_pooled_begin / _step / _result: the refinement.  At every evaluation, per pair (over its own pixels): wbar = Sw / n, rbar =
 * Sr / n, ww = Sww - n wbar^2, rr = Srr - n rbar^2, corr = Swr - n wbar rbar, A = S G_k G_l, ip_k = S G_k w - wbar S G_k, tp_k = S G_k r -
 * rbar S G_k.  A pair is included iff it is active (active host int32 [n_pairs], NULL: all), n >= min_valid M (M: the template
 * pixels its group's mask keeps, H W without one), all its sums are finite, ww > 0 and rr > 0; rho_i = corr / (sqrt ww sqrt rr),
 * NaN for a pair that is not included.  Per group the included pairs' quantities are added in ascending pair index, rho = C /
 * (sqrt WW sqrt RR), and the step, its order of decisions and the status codes are those of mp_ecc_step, with MP_ECC_FEW_VALID for a
 * group without an included pair.  step enqueues n_iters iterations -- a sums launch over (chunk, pair), a pair launch, a group
 * launch -- without synchronising, then writes the number of groups still running to *live (device int32).  result, per group:
 * transforms [G][9], rho [G] float64; iterations, status, converged, n_included int32 [G]; per pair at the group's latest
 * evaluation: rho_pair, n_pair float64 [n_pairs], included int32 [n_pairs].  A group's bits depend on its own ordered pair list
 * alone; an excluded pair adds nothing.
 * MP_EINVAL: the limits of mp_ecc_*, n_groups outside [1, MP_ECC_MAX_PROBLEMS], a group index outside [0, n_groups), a group
 * without a pair, a mask index outside [-1, n_masks), a negative radius, tmp aliasing, a small workspace
 * (mp_ecc_pooled_workspace_bytes).  MP_ESTATE: step / result on a workspace other than the one of the handle's latest
 * mp_ecc_pooled_begin. */
int mp_ecc_mask_grow(mp_handle* h, const unsigned char* masks, int n, int H, int W, int radius, unsigned char* tmp, unsigned char* out,
                     void* stream);
int mp_ecc_static_update(mp_handle* h, const float* frames, int n, int H, int W, int first, float* lo, float* hi, void* stream);
int mp_ecc_static_finish(mp_handle* h, const float* lo, const float* hi, int H, int W, unsigned char* mask, void* stream);
int mp_ecc_flag_packed(mp_handle* h, float* packed, int n, int H, int W, const unsigned char* masks, int n_masks,
                       const int* mask_of_frame, void* stream);
int mp_ecc_pooled_workspace_bytes(int n_pairs, int n_groups, int H, int W, long long* bytes);
int mp_ecc_pooled_sums(mp_handle* h, const float* packed, int Ho, int Wo, const float* thermal, int H, int W, int n_pairs,
                       const int* group, int n_groups, const double* transforms, const unsigned char* thermal_masks, int n_masks,
                       const int* mask_of_group, int model, double* sums, void* workspace, long long workspace_bytes, void* stream);
int mp_ecc_pooled_begin(mp_handle* h, const float* packed, int Ho, int Wo, const float* thermal, int H, int W, int n_pairs,
                        const int* group, const int* active, int n_groups, const double* init_transforms,
                        const unsigned char* thermal_masks, int n_masks, const int* mask_of_group, int model, double eps, int maxiter,
                        double min_valid, void* workspace, long long workspace_bytes, void* stream);
int mp_ecc_pooled_step(mp_handle* h, void* workspace, int n_iters, int* live, void* stream);
int mp_ecc_pooled_result(mp_handle* h, void* workspace, double* transforms, double* rho, int* iterations, int* status, int* converged,
                         int* n_included, double* rho_pair, double* n_pair, int* included, void* stream);

/* ---- Local residual field: windowed correlation of an aligned pair ----
 * optical_feat (the aligned optical frames) and thermal_feat: fp32 [B][H][W] outputs of mp_ecc_prepare; mask: uint8 [mask_frames][H][W]
 * on the optical side with mask_frames 1 (one plane for every frame) or B, nonzero = use, or NULL (all ones).
 * Windows of window x window pixels have their origins at y0 = radius + i stride for every i with y0 + window + radius <= H, and
 * likewise in x: mp_residual_grid gives their counts gy, gx.  The score of a displacement d = (dy, dx), |dy|, |dx| <= radius, is
 * taken over S_d = {p in the window: mask[p + d] != 0}, n = |S_d|: the zero-mean normalised cross-correlation of thermal_feat[p]
 * and optical_feat[p + d] from the sums St, So, Stt, Soo, Sto (fp32 products, float64 sums): mt = St / n, mo = So / n,
 * ctt = Stt - mt St, coo = Soo - mo So, cto = Sto - mt So, score = cto / (sqrt(ctt) sqrt(coo)).  It is undefined when
 * n < min_valid window^2 or when ctt or coo is <= var_floor n.  thermal_feat[p] ~ optical_feat[p + d]: d is the residual
 * misalignment of the optical frame at that window, in pixels.
 * Per window (row-major over (frame, window row, window column)): out_d float64 [..][5] = (dy, dx, rho, rho0, second), out_i int32
 * [..][2] = (n, status).  d* is the defined displacement with the largest score, ties to the first in row-major (dy, dx) order from
 * -radius; an axis on which |d*| < radius and both neighbours' scores a, c are defined is refined by 0.5 (a - c) / (a - 2 rho + c)
 * (0 when the denominator is not negative, clamped to +-0.5); rho is the score at d*, rho0 the one at d = 0 (NaN if undefined), second
 * the largest defined score outside the 3 x 3 block around d* (-inf when there is none), n the count at d*.
 * status: MP_RES_FEW_VALID when d = 0 has n < min_valid window^2; else MP_RES_FLAT when no displacement is defined; else
 * MP_RES_AT_EDGE when d* touches the search border on some axis, else MP_RES_OK.  The first two leave NaN in out_d and the count of
 * d = 0 in n.  A window's bits depend on its own pixels and the parameters alone.
 * MP_EINVAL: window outside {8, 16, 24, 32, 48, 64}, stride < 1, radius outside [1, 8], min_valid outside (0, 1], var_floor negative or
 * not finite, B outside [1, 65535], frames outside 8 x 8 .. 4096 x 4096, a frame that holds no window, mask_frames other than 1 or
 * B.  Nothing is launched then. */
#define MP_RES_OK 0
#define MP_RES_FEW_VALID 1
#define MP_RES_FLAT 2
#define MP_RES_AT_EDGE 3
int mp_residual_grid(int H, int W, int window, int stride, int radius, int* gy, int* gx);
int mp_residual_field(mp_handle* h, const float* optical_feat, const float* thermal_feat, const unsigned char* mask, int mask_frames,
                      int B, int H, int W, int window, int stride, int radius, double min_valid, double var_floor, double* out_d,
                      int* out_i, void* stream);

/* ---- Local alignment correction: fit and apply a smooth displacement field ----
 * mp_field_fit: d float64 [B][gy][gx][2] = (dy, dx), the displacements measured at the nodes of a gy x gx lattice (sides 1..256), and
 * weight float64 [B][gy][gx].  Per frame and axis the fit minimises sum_k w_k (u_k - d_k)^2 + lambda sum_(k,l) (u_k - u_l)^2 over the
 * edges of the 4-neighbour lattice: (W + lambda L) u = W d, L the lattice's graph Laplacian.  A node counts with weight 0, and its d
 * is never read (it may be NaN), unless its weight is positive and finite; a node with such a weight and a non-finite d counts with
 * weight 0 as well and is counted in out_info.  No node left: u = 0, status MP_FIELD_NO_DATA.
 * Solver: conjugate gradients preconditioned by the diagonal, float64, both axes at once as two right-hand sides, each with its own
 * step lengths; an axis stops at r^T r <= tol^2 b^T b (b = W d, r the recurrence's residual), the solve after max_iter iterations at
 * the latest (or when p^T A p of a running axis is not positive).  Status MP_FIELD_MAX_ITER says that the last solve ended without
 * MEETING that rule: at max_iter, at such a breakdown, or because r^T r or b^T b is not finite -- weights so large that w d or its
 * square overflows give no solution, and this status instead of a wrong MP_FIELD_OK.
 * Robust rounds (robust_px > 0 and rounds > 0): after solve t < rounds, e_k = |u_k - d_k| (Euclidean over both axes) and
 * w_k = w0_k (1 - (e_k / robust_px)^2)^2 for e_k < robust_px, else 0, from the INPUT weight w0; then the system is solved again,
 * started at the previous solution.  The first solve starts at u = 0.  If a round leaves no weight, the previous solution and
 * its weights stay, with status MP_FIELD_ALL_REJECTED.
 *   workspace   device memory of mp_field_fit_workspace's size (that entry touches no device), 16-byte aligned
 *   out_u       float64 [B][gy][gx][2]
 *   out_info    int32 [B][MP_FIELD_INFO_INTS]: status, iterations of the last solve, nodes with a non-zero weight in the system of
 *               the returned solution, nodes with a usable weight and a non-finite d
 *   out_res     float64 [B]: sqrt(r^T r / b^T b) at the end of the last solve, the larger of the two axes (0 for an axis with b = 0)
 *   out_w       float64 [B][gy][gx] or NULL: the weights of the system of the returned solution
 * One workgroup per frame, every sum in a fixed order: a frame's bits depend on its own lattice and the parameters alone.
 * out_u is the solver's working vector, written before d is read for the last time: no output and not the workspace may be the
 * buffer of d or weight, and out_u, out_w and the workspace are three different buffers.
 * MP_EINVAL, before any launch and with the outputs untouched: a NULL tensor, B outside [1, 65535], a lattice side outside [1, 256],
 * lambda not positive or not finite, robust_px or tol negative or not finite, rounds outside [0, 16], max_iter outside [1, 2^20], a
 * workspace that is too small or not 16-byte aligned, buffers that are one where the line above wants two.
 *
 * mp_field_warp: dst fp32 [B][H][W] (and valid uint8 [B][H][W], or NULL) sampled from src fp32 [n_src][Hs][Ws] (n_src 1: every frame
 * reads the same source, or B) through the field u float64 [B][gy][gx][2] (16-byte aligned: a node is read as one double2) whose
 * node (0, 0) has its centre at pixel (y0, x0) and whose nodes are `step` pixels apart.  Per output pixel (y, x), in float64 with no contraction:
 *   ty = (y - y0) / step, i = clamp(floor(ty), 0, max(gy - 2, 0)), fy = ty - i, clamped to [0, 1] with extrapolate = 0 (1: linear
 *   continuation of the border cells); gy = 1: row 0 and fy = 0; likewise j, fx in x.
 *   u(p) = (u[i][j] (1 - fx) + u[i][j+1] fx) (1 - fy) + (u[i+1][j] (1 - fx) + u[i+1][j+1] fx) fy per component
 *   q = (y + u_y, x + u_x); with hom (float64 [B][9], row-major on (x, y, 1), or NULL): (X, Y, Z) = hom (q_x, q_y, 1) with each
 *   row as (a q_x + b q_y) + c, and q = (Y / Z, X / Z)
 *   the pixel is invalid (dst 0, valid 0) when Z <= 0, when any of these values is not finite, or when |q_y| or |q_x| > 2^30
 *   else the bilinear sample of src at q: integer parts by floor, the fractions rounded to fp32, taps outside the source read 0,
 *   dst = (s00 (1 - fx) + s01 fx) (1 - fy) + (s10 (1 - fx) + s11 fx) fy in fp32, and valid = 1 iff every tap whose two weight
 *   factors are both non-zero lies inside the source
 * So u = 0 without hom on a source of dst's size returns the source (for a finite source without negative zeros: its bits) and
 * a mask of ones.
 * MP_EINVAL, before any launch: a NULL src, u or dst, src == dst, a u that is not 16-byte aligned, B outside [1, 65535], n_src other than 1 or B, a frame outside
 * 8 x 8 .. 4096 x 4096, a lattice side outside [1, 256], a non-finite origin, a step that is not positive and finite, extrapolate
 * other than 0 or 1. */
#define MP_FIELD_OK 0
#define MP_FIELD_NO_DATA 1
#define MP_FIELD_ALL_REJECTED 2
#define MP_FIELD_MAX_ITER 3
#define MP_FIELD_INFO_INTS 4
int mp_field_fit_workspace(int B, int gy, int gx, long long* bytes);
int mp_field_fit(mp_handle* h, const double* d, const double* weight, int B, int gy, int gx, double lambda, double robust_px, int rounds,
                 double tol, int max_iter, void* workspace, long long workspace_bytes, double* out_u, int* out_info, double* out_res,
                 double* out_w, void* stream);
int mp_field_warp(mp_handle* h, const float* src, int n_src, int Hs, int Ws, const double* u, int gy, int gx, double y0, double x0,
                  double step, int extrapolate, const double* hom, int B, int H, int W, float* dst, unsigned char* valid, void* stream);

/* per-launch timing of mp_forward with hipEvents on the caller's stream (bench.py roofline leg).
 * mp_profile_read synchronises; names[i] points to static strings. */
int mp_profile_enable(mp_handle* h, int enable);
int mp_profile_read(mp_handle* h, const char** names, float* ms, double* flop, int capacity, int* n);

/* ---- RIFT baseline (Li, Hu, Ai, IEEE TIP 2020; DESIGN.md 3.26: restated from the paper, not verified against the authors' code) ----
 * u8 [B][H][W] is the quantised frame (mp_lghd_quantize), bank fp32 [24][H][W] the log-Gabor bank of mp_lghd_orientation (4
 * scales x 6 orientations, scale-major), H and W lengths of the FFT.
 *
 * mp_phase_congruency.  R[s][o] = ifft2(fft2(u8) * bank[6 s + o]) / (H W), E = Re R, O = Im R, A = |R|, all in fp32; eps = 1e-4.
 * Per orientation o (theta = o pi / 6), sums over the four scales in ascending s:
 *   sumE, sumO, sumA, maxA;  X = sqrt(sumE^2 + sumO^2) + eps, mE = sumE / X, mO = sumO / X
 *   En = sum_s (E_s mE + O_s mO - |E_s mO - O_s mE|)
 *   En = max(En - T[b][o], 0), width = (sumA / (maxA + eps) - 1) / 3, weight = 1 / (1 + exp((cutoff - width) g))
 *   PC = weight En / (sumA + eps),  cx = PC cos theta, cy = PC sin theta
 * and over the orientations in ascending o: cx2 = sum cx^2 / 3, cy2 = sum cy^2 / 3, cxy = (sum cx cy) 4 / 6,
 *   d = sqrt(cxy^2 + (cx2 - cy2)^2) + eps,  M = (cy2 + cx2 + d) / 2,  m = (cy2 + cx2 - d) / 2
 *   mim = the first o with the largest sumA
 * T fp32 [B][6]: with the median of the H W values of A[0][o] (exact order statistics of the fp32 plane, the mean of the two
 * middle ones for an even count), in float64 with every operation rounded on its own and the result rounded once to fp32:
 *   tau = median / sqrt(ln 4), tot = tau (1 - q q q q) / (1 - q) with q = 1 / 1.6, T = tot sqrt(pi / 2) + (k tot) sqrt((4 - pi) / 2)
 * M, m fp32 [B][H][W], mim u8 [B][H][W]; amp fp32 [B][6][H][W] or NULL: the planes A[0][o] the medians were taken from.
 * Every sum runs in a fixed order without atomics: the maps of an image have the same bits in any batch and with any workspace.
 * The workspace holds the spectrum, the 24 half-transformed planes and the six amplitude planes of as many images as fit (at
 * least one; 224 H W bytes each): mp_rift_workspace_bytes sizes it for min(B, 4).
 * MP_EINVAL: H or W outside the FFT's lengths, B outside [1, 65535], k negative or not finite, g or cutoff not finite, a
 * workspace smaller than one image needs.
 *
 * mp_rift_detect.  range fp32 [B][2] = (min, max) of M[b]; u8m u8 [B][H][W] = (uint8) floor(255 ((M - min) / (max - min))), the
 * subtraction, the correctly rounded division and the multiplication each rounded to fp32, all 0 where max == min; then
 * mp_lghd_detect's FAST on u8m with `fast_threshold` in place of 10: score and corners as there, prob fp32 [B][H][W] or NULL
 * = score / 255 at corners with patch_size / 2 <= y <= H - patch_size / 2 and likewise in x, 0 elsewhere (everywhere on a frame
 * smaller than the patch).
 * MP_EINVAL: fast_threshold outside [1, 255], patch_size not a positive multiple of 12 or above MP_RIFT_MAX_PATCH.
 *
 * mp_rift_describe.  Rows [y - p/2, y + p/2) x columns [x - p/2, x + p/2) of mim, p = patch_size, in 6 x 6 cells of p / 6 pixels
 * with 6 bins, laid out [cell row][cell col][bin]: raw fp32 [B][K][256] holds the 216 exact counts, unit the same rows
 * L2-normalised (the sum of squares is an exact integer below 2^24 up to MP_RIFT_MAX_PATCH); columns 216..255 are 0; either may
 * be NULL.  kp_yx int32 [B][K][2], kp_count int32 [B].  Rows beyond kp_count, and keypoints whose patch leaves the frame, are zero.
 * MP_EINVAL: patch_size as above, or larger than H or W. */
#define MP_RIFT_MAX_PATCH 156
#define MP_RIFT_DESCRIPTOR_SIZE 256
int mp_rift_workspace_bytes(int B, int H, int W, long long* bytes);
int mp_phase_congruency(mp_handle* h, const unsigned char* u8, const float* bank, int B, int H, int W, float k, float g, float cutoff,
                        float* M, float* m, unsigned char* mim, float* T, float* amp, void* workspace, long long workspace_bytes,
                        void* stream);
int mp_rift_detect(mp_handle* h, const float* M, int B, int H, int W, int fast_threshold, int patch_size, unsigned char* u8m,
                   float* range, unsigned char* score, unsigned char* corners, float* prob, void* stream);
int mp_rift_describe(mp_handle* h, const unsigned char* mim, int B, int H, int W, int patch_size, const int* kp_yx,
                     const int* kp_count, int K, float* raw, float* unit, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MULTIPOINT_HIP_H */
