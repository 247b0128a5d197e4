/*
 * wm_hip.h -- C-ABI of the MI355X-native WildlifeMapper inference path.
 *
 * The reference (lgemc/WildlifeMapper) is pure Python/PyTorch and has no FFI
 * of its own: the boundary it exposes is a set of
 * nn.Module call signatures.  This header is the C-ABI inserted *below* those
 * signatures; every entry point names the reference call it replaces
 * (paths relative to /root/reference/wildlifemapper/).  INTEGRATION.md shows
 * the ctypes stub a reference maintainer would add.
 *
 * Conventions
 *   - every function returns 0 on success, <0 on error; wm_last_error() gives
 *     the message of the calling thread's last failure.  Nothing throws
 *     across the ABI.
 *   - device pointers are BORROWED (the caller, e.g. PyTorch-ROCm, owns them);
 *     contiguous fp32, NCHW where an image-like tensor is meant.  The handle
 *     owns packed weights and workspace, sized at create for `max_batch`.
 *   - launches are asynchronous on the caller's stream (`hipStream_t` passed
 *     as void*; NULL = default stream).  One handle per (device, stream);
 *     a handle is not thread-safe.
 *   - there is NO CPU fallback anywhere behind this ABI.
 */
#ifndef WM_HIP_H
#define WM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 13: wm_census_scratch_bytes, wm_census, WM_CENSUS_MAX_DETS, WM_CENSUS_SAME_CLASS, WM_CENSUS_UNSOLVED (survey census: the
 *    detections of overlapping frames grouped into individuals on the ground); nothing else changed.
 *    13, additive: wm_coverage_raster, wm_coverage_points, WM_COVERAGE_MAX_SIDE, WM_COVERAGE_MAX_CELLS,
 *    WM_COVERAGE_MAX_FRAMES, WM_COVERAGE_CLASSES, WM_COVERAGE_STATS (survey coverage: the ground a survey saw, its gaps and
 *    the individuals per cell); the number stays 13 because no v13 caller is affected, and a library without the two
 *    names is still refused by a binding that looks them up.
 *    13, additive: wm_mosaic_plan, wm_mosaic_fill_u8, WM_MOSAIC_NEAREST, WM_MOSAIC_BILINEAR, WM_MOSAIC_NORTH_UP and the
 *    status bits WM_MOSAIC_BAD_SLOT, WM_MOSAIC_BAD_SIZE, WM_MOSAIC_BAD_SOURCE (survey mosaic: the frames laid onto the
 *    coverage's ground grid); the number stays 13 for the same reason.
 *    13, additive: wm_register_render_u8, wm_register_search, wm_register_pair, WM_REGISTER_MAX_SIDE, WM_REGISTER_MAX_SEARCH,
 *    WM_REGISTER_MAX_PAIRS and the status bits WM_REGISTER_BAD_SLOT, WM_REGISTER_BAD_SIZE, WM_REGISTER_BAD_PAIR (survey
 *    registration: frame georeferences corrected by image matching); the number stays 13 for the same reason.
 *    13, additive: wm_register_search_zncc (survey registration, correlation search: a score that a gain and an offset
 *    between the two frames of a pair do not change); the number stays 13 for the same reason.
 *    13, additive: wm_register_refine, WM_REGISTER_REFINE_SUMS (survey registration, refinement: the integer normal
 *    equations of a sub-cell shift, yaw, scale, gain and offset per pair); the number stays 13 for the same reason.
 *    13, also additive: wm_mosaic_blend_plan, wm_mosaic_blend_accum_u8, wm_mosaic_blend_finish_u8 (survey mosaic, blended:
 *    every cell an integer-weighted mean of the exposure-corrected frames that see it); the number stays 13 for the same reason.
 *    13, also additive: wm_register_reduce_u8, WM_REGISTER_MAX_LEVEL (survey registration, pyramid: rendered planes reduced
 *    by 2 x 2 rounded means so the refinement converges from far off); the number stays 13 for the same reason.
 *    13, also additive: wm_undistort_u8 (survey lens: a frame resampled to the pinhole picture of its Brown-Conrady
 *    calibration, so the affine georeference holds for it); the number stays 13 for the same reason.
 *    13, also additive: wm_rectify_u8 (survey attitude: a tilted frame resampled to the picture of a level camera, by its
 *    roll and pitch and its calibration in one gather); the number stays 13 for the same reason.
 *    13, also additive: wm_ortho_u8 (survey terrain: a frame resampled onto a ground grid over a height grid, by its pose, the
 *    terrain's height and its calibration in one gather); the number stays 13 for the same reason.
 * 12: wm_box_outline_rect, wm_draw_boxes_u8, wm_plot_image_u8, WM_DRAW_MAX_WIDTH, WM_DRAW_MAX_PALETTE, WM_PLOT_SCRATCH_BYTES
 *    (survey overlays: detections outlined on frames and tiles, on the GPU); nothing else changed.
 * 11: wm_chip_window, wm_crop_chips_u8, WM_CHIP_MAX_SIDE (survey review chips: one PIL-exact crop per detection, cut on
 *    the GPU); nothing else changed.
 * 10: wm_criterion_scratch_bytes, wm_criterion (the validation losses of `evaluate`: Hungarian match + DETR losses);
 *    nothing else changed.
 * 9: wm_merge_frames_fuse (the survey merge's opt-in fuse policy: detections split by tile seams become one, with the
 *    union box); nothing else changed.
 * 8: the single-frame tile cut and merge entries removed: a single frame is a survey of one frame (wm_tile_frames_u8,
 *    wm_merge_frames_nms, same results); nothing else changed.
 * 7: WM_GEMM32_PRESPLIT for wm_op_gemm32; the split fp32 GEMM carries its lo parts scaled by 2^11 (no change in its
 *    contract beyond accuracy); nothing else changed.
 * 6: wm_resample_u8, wm_scaled_size (survey frames resampled to the model's training scale before tiling); nothing
 *    else changed.
 * 5: wm_frame_desc, wm_tile_frames_u8, wm_merge_frames_scratch_bytes, wm_merge_frames_nms (many frames of any size);
 *    nothing else changed.
 * 3 (round 3, second half): wm_op_encoder_attention_qkv added; nothing else changed.
 * 2 (round 3): wm_config.fp8_gemms; wm_debug_saturation_*; wm_op_layernorm rejects WM_PREC_FP8 with an fp32 output;
 * wm_profile_read no longer reports the fused-LayerNorm time-out (wm_forward / wm_encoder_forward do); precision value 2
 * (fp8), WM_FLAG_MERGED and a NULL handle in wm_postprocess_nms date from round 2.  The Python binding refuses a library
 * whose wm_abi_version() differs from the value it was written for. */
#define WM_ABI_VERSION 13

/* operand type of the transformer blocks' MFMA GEMMs / attention (accumulation, residual stream, LayerNorm
 * statistics, softmax and the whole decoder are fp32; the stem, the HFC adaptor and the neck -- 2.9 % of the
 * FLOPs -- always use fp16 operands, see DESIGN.md "Precision") */
#define WM_PREC_BF16 0   /* the type north_star names: bf16 MFMA; logits 0.7e-3 .. 2.0e-3 of the fp32 reference, weight-dependent */
#define WM_PREC_FP16 1   /* fp16 MFMA, same rate, 3 more mantissa bits: 1.7-2.4e-4; what the Python drop-in selects by default */
#define WM_PREC_FP8 2    /* BASELINE.json configs[4]: the blocks' qkv / proj / MLP GEMMs on the block-scaled fp8 MFMA
                            (OCP e4m3 weights with one fp32 scale per output channel, e4m3 activations at unit scale,
                            fp32 accumulation); attention stays bf16.  Tolerance re-stated in DESIGN.md section 3. */

#define WM_MAX_GLOBAL 8
#define WM_NUM_QUERIES 51   /* segment_anything/modeling/box_decoder.py:53 (50 + 1) */
#define WM_NUM_LOGITS 8     /* box_decoder.py:50,68 (6 + 1 classes, + background)   */

/* Encoder dims: what segment_anything/build_sam.py:19-52 passes to _build_sam.
 * Everything else (img 1024, patch 16, window 14, out 256, HFC dim 1024 / 8
 * heads, decoder 256 / 8 heads / depth 2 / 51 queries) is fixed by
 * build_sam.py:266-309 and image_encoder.py:65-87. */
typedef struct wm_config {
    int32_t embed_dim;                        /* 1280 (vit_h) | 1024 | 768 */
    int32_t depth;                            /* 32 | 24 | 12 */
    int32_t num_heads;                        /* 16 | 16 | 12 */
    int32_t num_global;                       /* 4 */
    int32_t global_attn_indexes[WM_MAX_GLOBAL];
    int32_t max_batch;                        /* tiles per call the workspace is sized for */
    int32_t precision;                        /* WM_PREC_* */
    int32_t flags;                            /* WM_CFG_* engine options, 0 = defaults */
    int32_t fp8_gemms;                        /* WM_PREC_FP8 only: WM_FP8_* mask of the blocks' GEMMs that run e4m3; 0 = default (all) */
    int32_t reserved[2];
} wm_config;

/* wm_config.fp8_gemms (also env WM_FP8_GEMMS when the field is 0): which GEMMs of a transformer block use the fp8 MFMA in
 * WM_PREC_FP8 mode; the others and attention run bf16.  lin1 and lin2 switch together (lin1's epilogue writes lin2's operand). */
#define WM_FP8_QKV 1
#define WM_FP8_PROJ 2
#define WM_FP8_MLP 4
#define WM_FP8_ALL 7

/* wm_config.flags.  Bit 0 (WM_CFG_FUSE_LN, rounds 1-2: LayerNorm fused into the residual GEMMs' epilogues with an in-kernel
 * exchange of row statistics between workgroups) is accepted and ignored: the folded LayerNorm below replaced it. */
#define WM_CFG_FUSE_LN 1
/* WM_CFG_FOLD_LN (round 3): the blocks' two LayerNorms run inside the GEMMs around them -- the residual GEMM's epilogue also
 * produces each row's statistics and a 16-bit copy of the row, the following qkv / lin1 GEMM multiplies that copy with
 * gamma (.) W and applies rstd (acc - mean c1) + c2 in its epilogue (csrc/gemm16_v5.h "Folded LayerNorm") -- so the residual
 * stream is not re-read by a LayerNorm kernel.  Results differ from the unfolded path within the operand rounding (the
 * rounding points move), they do not depend on the batch size.  The Python drop-in
 * sets it by default (WM_LN_FOLD=0 turns it off): +2.6 % tiles/s (ViT-H, B = 16), logits 2.3e-4 against 2.4e-4 unfolded.
 * gamma (.) W is computed from the fp32 weight (kept on the device) and rounded once (round 3 folded from the 16-bit weight).
 * It covers the blocks whose operands are fp16 (measured on five ViT-H tiles: logits 1.8-1.9e-4 folded, 2.3-2.4e-4 unfolded).
 * bf16-operand blocks keep their LayerNorm kernel unless WM_CFG_FOLD_LN_BF16 is set as well: with 8-bit mantissas the logits
 * error sits at ~1e-3 and every change of a rounding point is another draw from that distribution -- measured in round 4 with
 * gamma (.) W rounded once: ViT-H 1.29-1.36e-3 (LayerNorm kernel: 7.5-8.0e-4), ViT-L 8.2e-4 (9.3e-4); parity first, so the
 * mode that holds 1e-3 on both fixtures stays the default for bf16 and the faster folded form (+3.6 % tiles/s) is opt-in. */
#define WM_CFG_FOLD_LN 2
#define WM_CFG_FOLD_LN_BF16 4

typedef struct wm_handle wm_handle;

/* One detection slot; WM_NUM_QUERIES of them per tile, fixed size so that the
 * multi-GPU collation is a single fixed-size all-gather (replaces the pickle
 * gather of segment_anything/utils/misc.py:180-220). */
typedef struct wm_box_record {
    float   box[4];      /* x0,y0,x1,y1 scaled to target size (build_sam.py:250-254) */
    float   score;       /* max softmax prob over the 7 non-background columns (:232-233) */
    int32_t label;       /* argmax column */
    int32_t flags;       /* bit0: score > conf_thr (PostProcess keep, :239)
                            bit1: score > score_thr (visualize_prediction.py:150)
                            bit2: survives NMS (visualize_prediction.py:154) */
    int32_t nms_rank;    /* position in the NMS output list (descending score), -1 if not kept */
} wm_box_record;

#define WM_FLAG_CONF 1
#define WM_FLAG_SCORE 2
#define WM_FLAG_NMS 4
#define WM_FLAG_MERGED 8   /* wm_merge_frames_nms: survives the cross-tile NMS of its frame (_fuse: a keeper) */

const char* wm_last_error(void);
int wm_abi_version(void);

/* ---- lifetime / weights ---------------------------------------------------
 * Replaces model construction + load_state_dict:
 *   segment_anything/build_sam.py:260-322 (_build_sam), visualize_prediction.py:112-115.
 * wm_load_weight copies one state_dict tensor (fp32, host memory, names of
 * SURVEY.md §8b, e.g. "image_encoder.blocks.3.attn.qkv.weight"); unknown names
 * are an error, missing names are reported by wm_finalize_weights, which packs
 * everything into device buffers (16-bit GEMM operands, fp32 vectors). */
int wm_create(const wm_config* cfg, int device, wm_handle** out);
int wm_destroy(wm_handle* h);
int wm_load_weight(wm_handle* h, const char* name, const float* host_data,
                   const int64_t* shape, int ndim);
int wm_finalize_weights(wm_handle* h);

/* ---- the path ------------------------------------------------------------- */

/* Input pipeline in front of the path: uint8 HWC images [B,h,w,3] (h, w <= 1024) -> the model's
 * input tensor [B,3,1024,1024] fp32: ToTensor + Normalize(ImageNet) of dataloader_coco.py:286-292 and the zero
 * padding to 1024 x 1024 of segment_anything/utils/misc.py:46-67 (the resize to 768 is not part of it). */
int wm_preprocess_u8(const uint8_t* img_dev, float* out_dev, int batch, int height, int width, void* stream);

/* The same with the val transform's resize in front (dataloader_coco.py:286-292: T.RandomResize([size], max_size) ->
 * segment_anything/utils/augmentation.py:77-133 -> torchvision F.resize on a PIL image): frames [B,height,width,3] u8 of
 * any size are resampled to (oh, ow) = wm_resized_size(...) with Pillow's 8-bit bilinear resample arithmetic
 * (antialiased triangle filter, 22-bit fixed-point coefficients, horizontal then vertical pass; bit-exact with
 * PIL.Image.resize, tests/golden/resize_pil.npz), then ToTensor + Normalize + zero padding to 1024 x 1024.  Coefficient
 * tables are cached by the library per device and geometry, the intermediate image per (device, stream), so calls on
 * different streams may overlap.  (oh, ow) must fit the canvas. */
int wm_preprocess_u8_resized(const uint8_t* img_dev, float* out_dev, int batch, int height, int width, int size, int max_size,
                             void* stream);
/* augmentation.py:80-99 get_size_with_aspect_ratio: the (oh, ow) the resize above produces */
int wm_resized_size(int height, int width, int size, int max_size, int* out_h, int* out_w);
/* host-only (tests): the fixed-point coefficient tables of one axis, bounds [out_size][2], kk [out_size][*ksize_out] */
int wm_debug_resize_coeffs(int in_size, int out_size, int* bounds_out, int* kk_out, int kk_capacity, int* ksize_out);

/* MedSAM.fft, segment_anything/network.py:36-57.
 * x (B,3,1024,1024) fp32 -> hfc (B,1,1024,1024) fp32. */
int wm_hfc_fft(wm_handle* h, const float* x_dev, float* hfc_dev, int batch, void* stream);

/* ImageEncoderViT.forward(x, x_hfc), segment_anything/modeling/image_encoder.py:123-138.
 * x (B,3,1024,1024), x_hfc (B,1,1024,1024) -> out (B,256,64,64), all fp32. */
int wm_encoder_forward(wm_handle* h, const float* x_dev, const float* hfc_dev,
                       float* out_dev, int batch, void* stream);

/* MaskDecoder.forward with image_pe = PromptEncoder.get_dense_pe(),
 * segment_anything/modeling/box_decoder.py:71-107, pos_encoder.py:24-33.
 * emb (B,256,64,64) -> pred_logits (B,51,8), pred_boxes (B,51,4) (sigmoid applied). */
int wm_decoder_forward(wm_handle* h, const float* emb_dev, float* logits_dev,
                       float* boxes_dev, int batch, void* stream);

/* PostProcess.forward (segment_anything/build_sam.py:219-258) followed by the
 * score cut + torchvision.ops.nms step of visualize_prediction.py:150-157, per tile.
 * target_sizes (B,2) fp32 as build_sam.py:252-253 reads them.
 * records: B * WM_NUM_QUERIES slots in query order.  The kernel needs no weights and no workspace:
 * h may be NULL (the launch then goes to the calling thread's current device). */
int wm_postprocess_nms(wm_handle* h, const float* logits_dev, const float* boxes_dev,
                       const float* target_sizes_dev, float conf_thr, float score_thr,
                       float iou_thr, wm_box_record* records_dev, int batch, void* stream);

/* MedSAM.forward (network.py:59-87) + post-processing in one call; hfc and the
 * embedding stay in the handle's workspace.  logits/boxes/records may be NULL
 * if not wanted. */
int wm_forward(wm_handle* h, const float* x_dev, const float* target_sizes_dev,
               float* logits_dev, float* boxes_dev, wm_box_record* records_dev,
               int batch, void* stream);

/* ---- validation losses (inference.py:52, contract row A23) -----------------------------------------------------------
 * wm_criterion replaces criterion(outputs, targets) of the reference's evaluate: HungarianMatcher.forward
 * (segment_anything/modeling/matcher.py:33-81, which copies the cost matrix to the host and calls scipy's
 * linear_sum_assignment per image) followed by the forward losses of SetCriterion (segment_anything/build_sam.py:93-147;
 * utils/box_ops.py:9-61, utils/misc.py accuracy).  Forward only: no gradients.  Weightless like wm_postprocess_nms: h may
 * be NULL, nothing is allocated, the launches are asynchronous on the caller's stream.
 * Inputs: logits (B,51,8) and boxes (B,51,4) fp32, cxcywh in [0,1]; the images' targets packed, tgt_boxes_dev
 * (total,4) fp32 cxcywh normalised and tgt_labels_dev (total) int32 in 0..6 (both may be NULL when total = 0); image b owns
 * the targets [tgt_offsets[b], tgt_offsets[b+1]).  tgt_offsets is HOST memory (as wm_merge_frames_nms's), batch + 1
 * entries, starting at 0, not decreasing; at most WM_CRITERION_MAX_TARGETS targets per image, more is an error.
 * Cost (fp32, the reference's operation order): C[q][t] = w_bbox L1(box_q, box_t) - w_class softmax(logits_q)[label_t]
 * - w_giou GIoU(xyxy(box_q), xyxy(box_t)).  Assignment: shortest augmenting paths with row and column duals (the
 * algorithm of scipy's linear_sum_assignment) in double on the fp32 costs, one workgroup per image, ties to the lowest
 * index, every loop bounded by the matrix size.
 * Outputs: match_dev (B,51) int32 = the target (index within its image) matched to each query, or -1;
 * status_dev (B) int32, 0 or WM_CRITERION_* bits: an image whose cost matrix holds a non-finite value (scipy raises
 * there) or a label outside 0..6 is not solved -- all its matches are -1; sums_dev [WM_CRITERION_SUMS] double, the raw
 * sums over the call, added in a fixed order (bit-identical from run to run), all NaN if any status is set:
 *   [0] sum of w nll and [1] sum of w over the B * 51 slots (target class = the matched label or 7, w[7] = eos_coef:
 *       F.cross_entropy(..., empty_weight) = [0] / [1], build_sam.py:100-106),
 *   [2] sum of L1 and [3] sum of (1 - GIoU) over the matched pairs (:138-146; the caller divides by num_boxes, which
 *       needs an all-reduce), [4] the matched pairs, [5] those whose argmax over logits[:7] is the label (:111),
 *   [6] sum over images of |#{q: argmax over 8 != 7} - T_b| (:119-124), [7] reserved (0).
 * Debug outputs, each may be NULL: cost_dev [51 * total] fp32, image b's matrix [51][T_b] at 51 * tgt_offsets[b];
 * dual_u_dev (B,51) and dual_v_dev (total) double, the final duals of the queries and the targets (u_q + v_t <= C[q][t],
 * equal on matched pairs).  scratch_dev (16-byte aligned, device) holds at least wm_criterion_scratch_bytes(batch,
 * total) bytes. */
#define WM_CRITERION_MAX_TARGETS 2048   /* per image: the solver's column state lives in LDS */
#define WM_CRITERION_SUMS 8
#define WM_CRITERION_NONFINITE 1        /* status bit 0 */
#define WM_CRITERION_UNSOLVED 2         /* status bit 1: the solver's structural step bound was reached (finite costs cannot) */
int64_t wm_criterion_scratch_bytes(int batch, int total_targets);    /* <0 on error */
int wm_criterion(wm_handle* h, const float* logits_dev, const float* boxes_dev, const float* tgt_boxes_dev,
                 const int32_t* tgt_labels_dev, const int32_t* tgt_offsets, int batch, float w_class, float w_bbox, float w_giou,
                 float eos_coef, void* scratch_dev, int64_t scratch_bytes, int32_t* match_dev, double* sums_dev,
                 int32_t* status_dev, float* cost_dev, double* dual_u_dev, double* dual_v_dev, void* stream);

/* ---- large-frame front end (no reference behaviour: the reference down-scales whole frames) -------
 * One frame or a survey of many frames of any size per launch.
 * wm_tile_frames_u8: one model batch of 1024 x 1024 tiles cut from several frames.  frames_dev[n_frames] (device) gives
 * each frame's uint8 HWC base pointer and size; tiles_dev[n_tiles][3] = (frame index, y0, x0) (int32, device).  Output
 * [n_tiles,3,1024,1024] fp32: ToTensor + Normalize as in wm_preprocess_u8, zeros where a tile reaches past its frame;
 * each tile depends only on its own frame and origin.
 * wm_merge_frames_nms: records of the tiles of several frames (wm_forward / wm_postprocess_nms output, boxes in tile
 * pixels) and each tile's origin (y0, x0) in its frame (int32, device) -> merged records in frame coordinates.  In each
 * frame, with no limit on its tiles, the slots that survived their tile's NMS compete in one more greedy class-agnostic
 * NMS (IoU > iou_thr suppresses, descending score, stable).  Frame f is the tiles [frame_tile_offsets[f],
 * frame_tile_offsets[f+1]) of records_dev / origins_dev; frame_tile_offsets is HOST memory, n_frames + 1 entries,
 * starting at 0 and strictly increasing.  merged_dev[n_slots] (n_slots = total tiles * WM_NUM_QUERIES): every slot with
 * its box in frame coordinates and its other fields as given, except that survivors carry WM_FLAG_MERGED and nms_rank =
 * their position in the frame's merged list (the flag clear and -1 otherwise).  The compacted detection list: frame f's
 * survivors in merged order are det_dev / det_tile_dev [frame_tile_offsets[f] * WM_NUM_QUERIES + k], k <
 * det_count_dev[f] (det_tile = tile within the frame).  scratch_dev (16-byte aligned, device) holds at least
 * wm_merge_frames_scratch_bytes(total tiles) bytes; nothing is allocated.  Boxes must be finite; iou_thr in [0, 1).
 * Frame coordinates are fp32: below 0.01 px of fractional resolution up to 65536 px.
 * wm_merge_frames_fuse: the same inputs, candidates and priority order, greedy absorption instead of suppression.  Walking
 * the candidates in priority order, one not yet absorbed becomes a keeper and absorbs every later unabsorbed candidate
 * of ANOTHER tile whose box matches its own: inter / min(area_keeper, area_other) > fuse_thr (intersection over the
 * smaller box, fp32 as in the NMS; 0 / 0 never matches).  merged_dev as for the NMS, every slot with its own box:
 * keepers carry WM_FLAG_MERGED and nms_rank = their position in the frame's list, absorbed slots neither.  det_dev[k] is
 * keeper k's record with the union box of its members (elementwise min / max, exact), det_tile_dev[k] its tile,
 * det_members_dev[k] = 1 + the number of boxes it absorbed (same indexing as det_dev); slot_det_dev[n_slots] = the list
 * index of the detection a candidate slot belongs to (kept or absorbed), -1 for every other slot.  Same scratch;
 * fuse_thr in [0, 1). */
typedef struct wm_frame_desc {
    const uint8_t* data;      /* [height, width, 3] uint8, device */
    int32_t height, width;
} wm_frame_desc;
int wm_tile_frames_u8(const wm_frame_desc* frames_dev, int n_frames, const int32_t* tiles_dev, float* out_dev, int n_tiles,
                      void* stream);
int64_t wm_merge_frames_scratch_bytes(int n_tiles);    /* <0 on error */
int wm_merge_frames_nms(const wm_box_record* records_dev, const int32_t* origins_dev, const int32_t* frame_tile_offsets,
                        int n_frames, float iou_thr, void* scratch_dev, int64_t scratch_bytes, wm_box_record* merged_dev,
                        wm_box_record* det_dev, int32_t* det_tile_dev, int32_t* det_count_dev, void* stream);
int wm_merge_frames_fuse(const wm_box_record* records_dev, const int32_t* origins_dev, const int32_t* frame_tile_offsets,
                         int n_frames, float fuse_thr, void* scratch_dev, int64_t scratch_bytes, wm_box_record* merged_dev,
                         wm_box_record* det_dev, int32_t* det_tile_dev, int32_t* det_count_dev,
                         int32_t* det_members_dev, int32_t* slot_det_dev, void* stream);

/* Survey census (tiling.census): survey frames overlap (60-80 % along a flight line, and sideways between lines), so an
 * animal is detected in two to four frames; the census groups the detections of a whole survey into individuals.  No
 * reference behaviour exists; this rule is the contract, and tests/ground_oracle.py restates it sequentially.
 * Inputs: n detections, each a box (x0, y0, x1, y1) fp32 in the pixels of its frame, a score fp32, a label int32 and a
 * frame index f int32; georef_dev[n_frames][6] doubles (a0..a5) per frame, frame pixels -> ground metres, X east, Y north.
 * Ground point, in double, every operation correctly rounded on its own (no contraction):
 *     cx = ((double)x0 + (double)x1) * 0.5      cy = ((double)y0 + (double)y1) * 0.5
 *     X  = (a0 * cx + a1 * cy) + a2             Y  = (a3 * cx + a4 * cy) + a5
 * Invalid detections: a box coordinate or the score not finite, f outside [0, n_frames), or X or Y not finite.  An invalid
 * detection belongs to no individual: individual -1, point (NaN, NaN).
 * Priority: valid detections by score descending (-0 ties with +0), then by input index ascending.
 * Association: sequential, in priority order; r2 = radius * radius once, in double, on the host.  Individual q is
 * eligible for detection p when
 *   1. dx * dx + dy * dy <= r2 (double, inclusive) between p's point and the point of q's KEEPER (its founder; not a mean
 *      of the members);
 *   2. no member of q, keeper included, comes from p's frame;
 *   3. with WM_CENSUS_SAME_CLASS in flags: p's label equals the keeper's label.
 * If an individual is eligible, p joins the one at the smallest squared distance, ties to the individual founded
 * earlier; otherwise p founds a new individual and is its keeper.  Individuals are numbered in the order they are founded.
 * Condition 2 is what keeps a herd's count right: two animals a metre apart are both seen by the same frames, and the
 * second one's detections cannot all be absorbed by the first.
 * Outputs (device): points_dev[n][2] every detection's ground point; individual_dev[n] its individual or -1;
 * keeper_dev[k] the input index of individual k's keeper and members_dev[k] its member count, k < count_dev[0];
 * count_dev[1] = status bits: WM_CENSUS_UNSOLVED if the kernel's bounded round loop (at most n rounds; a round always
 * decides the highest-priority open detection, so it cannot happen) ended with detections undecided, which stay at -1.
 * Argument limits: radius finite and >= 0 with r2 finite; 0 <= n <= WM_CENSUS_MAX_DETS; n_frames >= 1; scratch_dev
 * 16-byte aligned with at least wm_census_scratch_bytes(n) bytes.  Bad arguments fail before any HIP call; n == 0
 * returns 0 before looking at any pointer (count 0: nothing is written).  One launch of one workgroup on `stream`,
 * asynchronous, nothing allocated.  After the call the first int32 of scratch_dev holds the rounds taken (diagnostic). */
#define WM_CENSUS_MAX_DETS 262144
#define WM_CENSUS_SAME_CLASS 1
#define WM_CENSUS_UNSOLVED 1            /* status bit 0 */
int64_t wm_census_scratch_bytes(int n);                       /* <0 on error */
int wm_census(const float* boxes_dev, const float* scores_dev, const int32_t* labels_dev, const int32_t* box_frame_dev, int n,
              const double* georef_dev /* [n_frames][6] */, int n_frames, double radius, int flags,
              void* scratch_dev, int64_t scratch_bytes,
              double* points_dev /* [n][2] */, int32_t* individual_dev /* [n] */, int32_t* keeper_dev /* [n]: input index of individual k's keeper, k < count */,
              int32_t* members_dev /* [n]: members of individual k */, int32_t* count_dev /* [2]: individuals, status */, void* stream);

/* Survey coverage (tiling.coverage): a count of individuals becomes a density only over the ground that was observed, and
 * frames overlap, so that ground is the union of the frame footprints, not their sum.  A ground grid is laid over the
 * survey; every cell gets the number of frames that saw its centre, and the census' individuals are counted into the same
 * grid per class, each with the number of frames that could have seen it.  No reference behaviour exists; this rule is the
 * contract, and tests/ground_oracle.py restates it sequentially (coverage_oracle).  All arithmetic is IEEE double, every
 * operation correctly rounded on its own (no contraction), in the order written.
 * Frames: g2p_dev[n_frames][6] doubles (b0..b5), the GROUND -> PIXEL affine of each frame (the inverse of the census'
 * georeference: tiling.ground_to_pixel); size_dev[n_frames][2] int32, (height, width) of the source frame in the pixels
 * the georeference speaks of.
 * Grid: (x0, y0) metres, the ground position of its south-west corner; cell metres, finite and > 0; gx cells east, gy
 * cells north.  Row j = 0 is the SOUTHERNMOST row (a north-up picture is the raster flipped along its first axis).
 * Predicate sees(f, X, Y):
 *     u = (b0 * X + b1 * Y) + b2               v = (b3 * X + b4 * Y) + b5
 *     true iff height >= 1, width >= 1, 0 <= u < width and 0 <= v < height.
 * A NaN or an infinity anywhere makes it false, so a frame whose georeference is not finite or is singular (its inverse
 * is NaN) sees nothing and needs no special case.  The footprint is half-open, as the pixel continuum [0, W) x [0, H) is.
 * Raster: the centre of cell (j, i) is Xc = x0 + ((double)i + 0.5) * cell, Yc = y0 + ((double)j + 0.5) * cell;
 * coverage_dev[gy][gx] uint16 = the number of frames f with sees(f, Xc, Yc) (n_frames <= 65535: nothing saturates);
 * stats_dev[16] int64: stats[m], m < 15, the number of cells with coverage == m, stats[15] those with coverage >= 15.
 * The observed area is (gx * gy - stats[0]) * cell * cell.
 * Points (optional, an entry of their own): points_dev[n_points][2] doubles (X, Y) on the ground, labels_dev[n_points].
 *     seen_by_dev[p] int32 = the number of frames with sees(f, X, Y), at the point itself, not at a cell centre; a point
 *         that is not finite gets 0;
 *     i = floor((X - x0) / cell), j = floor((Y - y0) / cell): a subtraction, a division, a floor, in double;
 *     the point is BINNED iff it is finite, 0 <= i < gx, 0 <= j < gy and 0 <= label < 7; a binned point adds 1 to
 *         counts_dev[label][j][i] (int32 [7][gy][gx]; NULL: nothing is binned into a raster, everything else is written);
 *     cell_dev[p] = (j, i) int32, (-1, -1) for a point that is not binned;
 *     pstats_dev[2] int64: [0] binned points, [1] points not binned.
 * Both entries zero what they accumulate into (stats, pstats, counts) on `stream` and write every element of their
 * outputs; asynchronous, nothing allocated.  The raster is gathered (a workgroup owns a block of cells and walks the
 * frames; frames that cannot touch the block are dropped by a conservative test that changes no count), so no atomics touch
 * it; stats and pstats take 64-bit integer atomics, counts int32 ones: integers, so the order is irrelevant.
 * Argument limits: 1 <= gx, gy <= WM_COVERAGE_MAX_SIDE, gx * gy <= WM_COVERAGE_MAX_CELLS; 0 <= n_frames <=
 * WM_COVERAGE_MAX_FRAMES (g2p_dev and size_dev may be NULL at 0, which gives an all-zero raster); 0 <= n_points <=
 * WM_CENSUS_MAX_DETS; x0, y0, cell finite, cell > 0; doubles and int64 8-byte, int32 4-byte, uint16 2-byte aligned.  Bad
 * arguments fail before any HIP call with a message that names the argument; n_points == 0 returns 0 before looking at
 * any pointer (nothing is written). */
#define WM_COVERAGE_MAX_SIDE 16384
#define WM_COVERAGE_MAX_CELLS 67108864          /* 2^26 */
#define WM_COVERAGE_MAX_FRAMES 65535
#define WM_COVERAGE_CLASSES 7
#define WM_COVERAGE_STATS 16
int wm_coverage_raster(const double* g2p_dev /* [n_frames][6] */, const int32_t* size_dev /* [n_frames][2] */, int n_frames,
                       double x0, double y0, double cell, int gx, int gy, uint16_t* coverage_dev /* [gy][gx] */,
                       int64_t* stats_dev /* [16] */, void* stream);
int wm_coverage_points(const double* g2p_dev, const int32_t* size_dev, int n_frames, const double* points_dev /* [n_points][2] */,
                       const int32_t* labels_dev, int n_points, double x0, double y0, double cell, int gx, int gy,
                       int32_t* seen_by_dev /* [n_points] */, int32_t* cell_dev /* [n_points][2] */,
                       int32_t* counts_dev /* [7][gy][gx], may be NULL */, int64_t* pstats_dev /* [2] */, void* stream);

/* Survey mosaic (tiling.mosaic, tiling.mosaic_plan): the map itself -- the frames laid onto the ground grid, one picture of
 * the whole survey.  For every ground cell ONE frame is chosen and its pixel fetched.  No reference behaviour exists (the
 * reference has no georeferencing); this rule is the contract, and tests/ground_oracle.py restates it sequentially
 * (mosaic_oracle).  The grid, the cell centres, the frames and sees are those of "Survey coverage", word for word:
 * g2p_dev[n_frames][6] doubles (b0..b5, ground -> pixel) and size_dev[n_frames][2] int32 (height, width); the centre of cell
 * (j, i) is Xc = x0 + ((double)i + 0.5) * cell, Yc = y0 + ((double)j + 0.5) * cell, row j = 0 the SOUTHERNMOST;
 *     u = (b0 * Xc + b1 * Yc) + b2             v = (b3 * Xc + b4 * Yc) + b5
 * all IEEE double, every operation correctly rounded on its own (no contraction), in the order written.
 * Seam rule: among the frames f with sees(f, Xc, Yc), the SOURCE of cell (j, i) is the one with the smallest
 *     e = du * du + dv * dv,      du = u - 0.5 * (double)width,      dv = v - 0.5 * (double)height
 * (two products and one sum); ties go to the lowest frame index; a cell that no frame sees has source -1.  e is the squared
 * pixel distance from the frame's centre -- for one camera the off-nadir angle, whatever the altitude -- so every piece of
 * ground is shown by the frame that looked at it most vertically, and the seams are the Voronoi lines between the frame
 * centres.  A frame that is NaN, infinite, singular or smaller than 1 x 1 sees nothing: it is never a source and needs no
 * special case.
 * Sampling, from the source frame (HWC uint8), per channel:
 *   WM_MOSAIC_NEAREST: the pixel ((int)floor(v), (int)floor(u)), which sees guarantees is in range.
 *   WM_MOSAIC_BILINEAR, pixel centres at integer + 0.5: fu = u - 0.5, xf = floor(fu), tx = fu - xf, and the same for v
 *     (fv, yf, ty); the columns (int)xf and (int)xf + 1 are each clamped to [0, width - 1], the rows (int)yf and (int)yf + 1
 *     to [0, height - 1] (edge replicate); with p00, p10 the pixels of row yf at the two columns and p01, p11 those of row
 *     yf + 1:  a = (1.0 - tx) * p00 + tx * p10,  b = (1.0 - tx) * p01 + tx * p11,  val = (1.0 - ty) * a + ty * b;
 *     the output is (uint8)min(floor(val + 0.5), 255.0).
 * A cell finer than the ground sampling distance magnifies; a coarser one point-samples and aliases: shrink the frames
 * first (wm_resample_u8) and rescale their georeferences (tiling.resampled_georef).  There is no area filter.
 * wm_mosaic_plan, geometry only: source_dev[gy][gx] int32; won_dev[n_frames] int32, the cells each frame is the source
 * of; stats_dev[2] int64: [0] the cells with a source, [1] the cells without.  Every element is written; won and stats are
 * zeroed on `stream` first.  A gather in the shape of wm_coverage_raster (no atomics touch source; won and stats take
 * integer atomics).  n_frames == 0 (g2p_dev, size_dev and won_dev may then be NULL) gives an all -1 raster.
 * wm_mosaic_fill_u8, the pixel gather: frames_dev[n_resident] describes the frames that are on the device in this call;
 * slot_dev[n_frames] int32 maps a survey frame to its index in frames_dev, negative when it is not resident; g2p_dev and
 * size_dev are the whole survey's, the grid and source_dev the plan's; mode is WM_MOSAIC_NEAREST or WM_MOSAIC_BILINEAR;
 * flags may hold WM_MOSAIC_NORTH_UP, which stores cell row j in picture row gy - 1 - j (only the picture is flipped, never
 * source).  mosaic_dev[gy][gx][3] uint8: a cell is written iff its source is resident, and every other byte is left as it
 * was, so the frames of a survey may be split over any number of calls in any order with the bytes of one call.  u, v are
 * recomputed with the expression above, which gives the plan's bits.  Nothing is read out of range: a cell is SKIPPED, and
 * a bit ORed into status_dev[0] (int32, which the caller zeroes before its first call and reads after its last; the entry
 * never clears it), when slot_dev[f] >= n_resident or the descriptor's data is NULL (WM_MOSAIC_BAD_SLOT), when the
 * descriptor's (height, width) differ from size_dev[f] (WM_MOSAIC_BAD_SIZE), or when source is not the plan's: f >=
 * n_frames, or f does not see the cell's centre (WM_MOSAIC_BAD_SOURCE).  n_frames == 0 or n_resident == 0 writes nothing.
 * Both entries: asynchronous on `stream`, nothing allocated, plain loads and stores.  Argument limits are the coverage's:
 * 1 <= gx, gy <= WM_COVERAGE_MAX_SIDE, gx * gy <= WM_COVERAGE_MAX_CELLS, 0 <= n_frames, n_resident <=
 * WM_COVERAGE_MAX_FRAMES, x0, y0, cell finite, cell > 0; doubles, int64 and descriptors 8-byte, int32 4-byte aligned.  Bad
 * arguments fail before any HIP call with a message that names the argument. */
#define WM_MOSAIC_NEAREST 0
#define WM_MOSAIC_BILINEAR 1
#define WM_MOSAIC_NORTH_UP 1            /* flags bit 0 */
#define WM_MOSAIC_BAD_SLOT 1            /* status bits */
#define WM_MOSAIC_BAD_SIZE 2
#define WM_MOSAIC_BAD_SOURCE 4
int wm_mosaic_plan(const double* g2p_dev /* [n_frames][6] */, const int32_t* size_dev /* [n_frames][2] */, int n_frames,
                   double x0, double y0, double cell, int gx, int gy, int32_t* source_dev /* [gy][gx] */,
                   int32_t* won_dev /* [n_frames] */, int64_t* stats_dev /* [2] */, void* stream);
int wm_mosaic_fill_u8(const wm_frame_desc* frames_dev, int n_resident, const int32_t* slot_dev /* [n_frames] */,
                      const double* g2p_dev, const int32_t* size_dev, int n_frames, double x0, double y0, double cell, int gx,
                      int gy, const int32_t* source_dev /* [gy][gx] */, int mode, int flags,
                      uint8_t* mosaic_dev /* [gy][gx][3] */, int32_t* status_dev /* [1] */, void* stream);

/* Survey mosaic, blended (tiling.mosaic(blend=), tiling.mosaic_blend_plan): the hard mosaic above gives every cell to one
 * frame, so residual misregistration tears and an exposure difference steps at the Voronoi lines.  Here every cell is an
 * integer-weighted mean of the exposure-corrected pixels of ALL the frames that see it, each frame's weight falling to
 * zero at its own border and away from the seam, over a band the caller chooses.  No reference behaviour exists; this rule
 * is the contract, and tests/ground_oracle.py restates it sequentially (blend_oracle).  The grid, the cell centres,
 * g2p, size, sees and the (u, v) expression are those of "Survey coverage", word for word; all double arithmetic is IEEE,
 * one rounding per operation, no contraction, in the order written; there is no sqrt, and one division, k, on the host.
 * For a cell with centre (Xc, Yc) and every frame f with sees(f, Xc, Yc):
 *     m_f    = min(min(u, (double)width - u), min(v, (double)height - v))      distance to the frame's nearest border, px
 *     m*     = the largest m_f over the frames that see the cell
 *     k      = 256.0 / band          band: double, finite, > 0, in source pixels; k computed once on the host, and finite
 *     edge_f = min(m_f * k, 256.0)
 *     seam_f = 256.0                                           if m_f >= m*
 *              min(max(((m_f - m*) + band) * k, 0.0), 255.0)   otherwise
 *     q_f    = (int)floor(min(seam_f, edge_f));   a frame with m_f >= m* gets max(q_f, 1)
 * Every frame fades to nothing at its own border; a frame contributes only where its border distance is within band
 * pixels of the best one's; the best frame, or frames at a tie, always contributes, so the weight sum is at least 1 wherever
 * a frame sees the cell.  Far inside one frame's territory (m* - m_f >= band for all others) the cell is that frame's pixel
 * alone.  Frames of different ground sampling distance compare in their OWN pixels: of two frames that reach equally far
 * over the ground, the finer one has the larger m and is favoured.
 * Pixel: p_c of frame f is the uint8 sample wm_mosaic_fill_u8 would fetch, WM_MOSAIC_NEAREST or WM_MOSAIC_BILINEAR as above.
 * Exposure: exposure_dev[n_frames][2] int32 (A, B), Q12 fixed point, NULL for none:
 *     p'_c = min(max(floor(((int64)A * p_c + B + 2048) / 4096), 0), 255)
 * in int64, so that no int32 table overflows; the same (A, B) for the three channels (the luma weights 77 + 150 + 29 = 256
 * make a gain and an offset on luma a gain and an offset per channel).  (4096, 0) is the identity, p' = p exactly: a NULL
 * table and an all-identity table give the same bytes.
 * Accumulators: acc[j][i] = (sum q_f * p'_r, sum q_f * p'_g, sum q_f * p'_b, sum q_f), four uint32.  With q <= 256, p' <= 255
 * and at most 65535 frames a channel sum is at most 4 278 124 800 < 2^32; integer sums do not depend on the order.
 * Picture: a cell with wsum > 0 gets (acc_c + (wsum >> 1)) / wsum per channel -- in uint32 at most 4 286 513 280, which still
 * fits; a cell with wsum == 0 is left as it was (the caller's fill colour).
 * wm_mosaic_blend_plan, geometry only, in the shape of wm_mosaic_plan: best_dev[gy][gx] double, m*, or -1.0 where no frame
 * sees the cell; cells_dev[n_frames] int32, the cells where frame f has q_f > 0 (exactly the frames a caller has to load);
 * stats_dev[3] int64: [0] cells seen, [1] cells not seen, [2] cells with two or more frames of q > 0.  Every element is
 * written; cells and stats are zeroed on `stream` first.  n_frames == 0 (g2p_dev, size_dev, cells_dev may be NULL) gives
 * all -1.0.
 * wm_mosaic_blend_accum_u8: frames_dev[n_resident] describes the frames on the device in this call and index_dev[n_resident]
 * int32 the survey index of each; only these are walked, never all n_frames.  The caller zeroes acc_dev[gy][gx][4] before
 * its first call; the entry never clears it.  A frame adds into the cells where its q_f > 0; m_f is recomputed with the
 * plan's expression, so m_f >= best compares the plan's bits.  A cell's accumulators are read and written only when a
 * resident frame contributes to it.  The frames of a survey may be split over any number of calls in any order, each
 * frame once (a frame given twice counts twice: the caller's contract).  A frame is SKIPPED, and a bit ORed into
 * status_dev[0] (int32, zeroed by the caller, never cleared here), when its index is outside [0, n_frames) or its data is
 * NULL (WM_MOSAIC_BAD_SLOT), or its descriptor's (height, width) differ from size_dev[f] (WM_MOSAIC_BAD_SIZE).
 * n_resident == 0 returns 0 after the checks.
 * wm_mosaic_blend_finish_u8 performs the division into mosaic_dev[gy][gx][3]; flags may hold WM_MOSAIC_NORTH_UP, which flips
 * the picture only: acc and best keep row 0 south.
 * All three: asynchronous on `stream`, nothing allocated; no atomics touch best, acc or the picture.  Argument limits are
 * the coverage's, plus band finite and > 0 (and 256 / band finite); doubles, int64 and descriptors 8-byte, int32 and uint32
 * 4-byte aligned.  Bad arguments fail before any HIP call with a message that names the argument. */
int wm_mosaic_blend_plan(const double* g2p_dev /* [n_frames][6] */, const int32_t* size_dev /* [n_frames][2] */, int n_frames,
                         double x0, double y0, double cell, int gx, int gy, double band, double* best_dev /* [gy][gx] */,
                         int32_t* cells_dev /* [n_frames] */, int64_t* stats_dev /* [3] */, void* stream);
int wm_mosaic_blend_accum_u8(const wm_frame_desc* frames_dev, const int32_t* index_dev /* [n_resident] */, int n_resident,
                             const double* g2p_dev, const int32_t* size_dev, int n_frames,
                             const int32_t* exposure_dev /* [n_frames][2], may be NULL */, double x0, double y0, double cell, int gx,
                             int gy, double band, const double* best_dev /* [gy][gx] */, int mode,
                             uint32_t* acc_dev /* [gy][gx][4] */, int32_t* status_dev /* [1] */, void* stream);
int wm_mosaic_blend_finish_u8(const uint32_t* acc_dev /* [gy][gx][4] */, int gx, int gy, int flags,
                              uint8_t* mosaic_dev /* [gy][gx][3] */, void* stream);

/* Survey registration (tiling.register): census, coverage and mosaic take each frame's georeference on trust, and one built
 * from GPS and heading is wrong by metres from frame to frame.  Frames overlap, so every pair of neighbours shows the same
 * ground twice: each pair is rendered onto a common ground patch and the shift at which the two agree is found by an
 * exhaustive integer search; one translation per frame is then solved on the host (tiling.adjust).  No reference behaviour
 * exists; this rule is the contract, and tests/register_cases.py restates it sequentially (register_oracle).  The frames
 * (g2p_dev[n_frames][6] doubles b0..b5, ground -> pixel; size_dev[n_frames][2] int32, (height, width)), the predicate sees
 * and the cell-centre expression are those of "Survey coverage", word for word; all double arithmetic is IEEE, every
 * operation correctly rounded on its own (no contraction), in the order written.  Everything after the render is integer.
 * Pairs: pairs_dev[n_pairs] of wm_register_pair, 32 bytes each, 8-byte aligned.  The patch of a pair is gx x gy cells of `cell`
 * metres with south-west corner (x0, y0); 1 <= gx, gy <= side <= WM_REGISTER_MAX_SIDE; 0 <= search <=
 * WM_REGISTER_MAX_SEARCH; 0 <= n_pairs <= WM_REGISTER_MAX_PAIRS.
 * Render (wm_register_render_u8): plane A of pair p is a_dev[p][side][side] uint8, of frame_a; plane B is b_dev[p][E][E],
 * E = side + 2 * search, of frame_b.  Cell (j, i) of A has centre Xc = x0 + ((double)i + 0.5) * cell, Yc = y0 + ((double)j +
 * 0.5) * cell; cell (j, i) of B has centre Xc = x0 + ((double)(i - search) + 0.5) * cell, Yc likewise (the subtraction in
 * int): B is the same grid grown by `search` cells on every side, and the centre of B cell (j + search, i + search) has the
 * bits of A cell (j, i).  A cell's value is 0 if its frame does not see the centre; else, with
 *     u = (b0 * Xc + b1 * Yc) + b2             v = (b3 * Xc + b4 * Yc) + b5
 * and (R, G, B) the NEAREST pixel ((int)floor(v), (int)floor(u)) of the frame (HWC uint8), it is
 *     max(1, (77 * R + 150 * G + 29 * B + 128) >> 8)
 * -- integer luma; 0 is reserved for "not seen".  Cells of A with i >= gx or j >= gy, and of B with i >= gx + 2 * search or
 * j >= gy + 2 * search, are written 0.  Residency is wm_mosaic_fill_u8's: frames_dev[n_resident] describes the frames on
 * the device in this call, slot_dev[n_frames] int32 maps a survey frame to its index there, negative when it is not
 * resident.  A plane is written, every byte of it, iff its frame is resident, and is otherwise left untouched, so the
 * frames of a survey may come in any number of calls in any order.  Nothing is read out of range: a plane is SKIPPED, and
 * a bit ORed into status_dev[0] (int32, which the caller zeroes before its first call and reads after its last), when the
 * frame's slot is >= n_resident or its descriptor's data is NULL (WM_REGISTER_BAD_SLOT), when the descriptor's (height,
 * width) differ from size_dev[f] (WM_REGISTER_BAD_SIZE), or -- both planes of the pair -- when frame_a or frame_b is outside
 * [0, n_frames) or gx or gy outside [1, side] (WM_REGISTER_BAD_PAIR).
 * Search (wm_register_search): for every pair and every offset (dy, dx) in [-search, search]^2,
 *     n(dy, dx)   = the number of cells (j, i), j < gy, i < gx, with A[j][i] != 0 and B[j + search + dy][i + search + dx] != 0;
 *     sad(dy, dx) = the sum of |A[j][i] - B[j + search + dy][i + search + dx]| over exactly those cells;
 * score_dev[p][2 * search + 1][2 * search + 1][2] int32 holds (sad, n) at [dy + search][dx + search] (at most 254 * 512^2 =
 * 66 584 576: nothing overflows).  Only gx and gy of a pair are read here; a pair with gx or gy outside [1, side] keeps an
 * all-zero score.  Offset p BEATS q iff sad_p * n_q < sad_q * n_p in int64 -- the means compared without a division -- and
 * at equality the smaller (dy * dy + dx * dx, dy, dx) wins, lexicographically.  best_dev[p][8] int32 = (dy, dx, sad, n,
 * dy2, dx2, sad2, n2): the first four are the offset that beats all others among those with n >= min_cells (min_cells >=
 * 1); the last four the same among the offsets with max(|dy - dy*|, |dx - dx*|) >= 2 of the first: the runner-up outside
 * the peak's 3 x 3, the confidence measure.  Where there is no eligible offset the four are (0, 0, -1, 0).
 * Meaning of the sign: a best (dx, dy) says B's content appears (dx, dy) * cell metres displaced relative to A's; with t_f
 * the translation added to (a2, a5) of frame f's georeference, the measurement is t_b - t_a = -(dx, dy) * cell.
 * Both entries: asynchronous on `stream`, nothing allocated; the search zeroes score_dev on `stream` and accumulates into
 * it with int32 atomics (integers: the order is irrelevant); plain vector loads and stores.  Limits beside those above:
 * 0 <= n_frames, n_resident <= WM_COVERAGE_MAX_FRAMES, cell finite and > 0; doubles, pairs and descriptors 8-byte, int32
 * 4-byte aligned.  Bad arguments fail before any HIP call with a message that names the argument; n_pairs == 0 returns 0
 * before looking at any pointer. */
#define WM_REGISTER_MAX_SIDE 512
#define WM_REGISTER_MAX_SEARCH 64
#define WM_REGISTER_MAX_PAIRS 65535
#define WM_REGISTER_BAD_SLOT 1          /* status bits */
#define WM_REGISTER_BAD_SIZE 2
#define WM_REGISTER_BAD_PAIR 4
typedef struct wm_register_pair {
    int32_t frame_a, frame_b, gx, gy;
    double x0, y0;
} wm_register_pair;
int wm_register_render_u8(const wm_frame_desc* frames_dev, int n_resident, const int32_t* slot_dev /* [n_frames] */,
                          const double* g2p_dev, const int32_t* size_dev, int n_frames, const wm_register_pair* pairs_dev,
                          int n_pairs, double cell, int search, int side, uint8_t* a_dev /* [n_pairs][side][side] */,
                          uint8_t* b_dev /* [n_pairs][E][E] */, int32_t* status_dev /* [1] */, void* stream);
int wm_register_search(const uint8_t* a_dev, const uint8_t* b_dev, const wm_register_pair* pairs_dev, int n_pairs, int search,
                       int side, int min_cells, int32_t* score_dev /* [n_pairs][2S+1][2S+1][2] */,
                       int32_t* best_dev /* [n_pairs][8] */, void* stream);

/* Survey registration, correlation search (tiling.register(metric="zncc")): the search above compares grey levels as they
 * are, so a pair whose frames differ in exposure -- b -> g * b + o, g > 0 -- moves its minimum or flattens it.  This search
 * scores an offset by the zero-mean normalised correlation of the two planes, which no such change alters.  Planes, pairs,
 * limits, the offset convention and the meaning of the sign are those of "Survey registration", word for word; the planes
 * are wm_register_render_u8's.
 * Search (wm_register_search_zncc): for every pair and every offset (dy, dx) in [-search, search]^2, over exactly the cells
 * that wm_register_search counts -- (j, i), j < gy, i < gx, with a = A[j][i] != 0 and b = B[j + search + dy][i + search + dx]
 * != 0 -- six integers:
 *     n = their number, Sa = sum a, Sb = sum b, Saa = sum a * a, Sbb = sum b * b, Sab = sum a * b      (a, b in 1..255)
 * moments_dev[p][2 * search + 1][2 * search + 1][6] int64 holds (n, Sa, Sb, Saa, Sbb, Sab) at [dy + search][dx + search]
 * (Sab is at most 255^2 * 512^2 = 1.7e10: int64 is required).  Only gx and gy of a pair are read here; a pair with gx or gy
 * outside [1, side] keeps all-zero moments.  From the moments, all exact in int64 and every product below 2^53,
 *     c = n * Sab - Sa * Sb          va = n * Saa - Sa * Sa          vb = n * Sbb - Sb * Sb
 * An offset is ELIGIBLE iff n >= min_cells (min_cells >= 1), va > 0 and vb > 0: a flat plane has no correlation.  Its score
 * is the signed squared correlation in IEEE double,
 *     q = ((double)c * fabs((double)c)) / ((double)va * (double)vb)
 * -- two multiplications and one division, each correctly rounded on its own, no contraction, no square root; the
 * conversions are exact.  Offset p BEATS q iff q_p > q_q as doubles, and at equality the smaller (dy * dy + dx * dx, dy,
 * dx) wins, lexicographically: the tie key above.  best_dev[p][8] int32 = (dy, dx, ok, n, dy2, dx2, ok2, n2): the first
 * four are the eligible offset that beats all others, with ok = 1; the last four the same among the eligible offsets with
 * max(|dy - dy*|, |dx - dx*|) >= 2 of the first, the runner-up outside the peak's 3 x 3.  Where there is no eligible offset
 * the four are (0, 0, 0, 0).  peak_dev[p][2] double = (q, q2) of the two, NaN where ok (ok2) is 0.
 * Asynchronous on `stream`, nothing allocated; moments_dev is zeroed on `stream` and accumulated into with 64-bit integer
 * vector atomics (integers: the order is irrelevant); plain vector loads and stores.  Arguments as for wm_register_search;
 * moments_dev and peak_dev 8-byte, best_dev 4-byte aligned.  Bad arguments fail before any HIP call with a message that names
 * the argument; n_pairs == 0 returns 0 before looking at any pointer. */
int wm_register_search_zncc(const uint8_t* a_dev, const uint8_t* b_dev, const wm_register_pair* pairs_dev, int n_pairs, int search,
                            int side, int min_cells, int64_t* moments_dev /* [n_pairs][2S+1][2S+1][6] */,
                            int32_t* best_dev /* [n_pairs][8] */, double* peak_dev /* [n_pairs][2] */, void* stream);

/* Survey registration, refinement (tiling.refine, tiling.register(refine=k)): the searches above resolve one cell and one
 * translation per frame.  Around the integer peak, one Gauss-Newton step of the brightness-constancy equation gives the
 * sub-cell shift, the rotation and the scale of a pair, and the gain and offset between its two exposures; it reads every
 * cell once.  This entry computes the integer normal equations of that step; the 4 x 4 or 6 x 6 solve is the host's
 * (tiling.refine_solve).  Planes, pairs and limits are those of "Survey registration", word for word, and the planes are
 * wm_register_render_u8's -- except 1 <= search <= WM_REGISTER_MAX_SEARCH: B must carry a ring of at least one cell.  Only
 * the centre offset is used.
 * Sums (wm_register_refine): for pair p and cell (j, i), j < gy, i < gx, let J = j + search, I = i + search and
 *     a = A[j][i]    b = B[J][I]    e = B[J][I + 1]    w = B[J][I - 1]    nn = B[J + 1][I]    ss = B[J - 1][I]
 * A cell COUNTS iff all six are non-zero.  For a counted cell, all in integers (rows grow north, columns east),
 *     r  = a - b                gxv = e - w               gyv = nn - ss
 *     x  = 2 * i + 1 - gx       y   = 2 * j + 1 - gy      (twice the cell centre's offset from the patch centre, in cells)
 *     c0 = gxv    c1 = gyv    c2 = x * gyv - y * gxv    c3 = x * gxv + y * gyv    c4 = b    c5 = 1
 * sums_dev[p][WM_REGISTER_REFINE_SUMS] int64 holds, over the counted cells: the 21 products sum c_k * c_l, k <= l, row-major
 * -- (0,0), (0,1), ... (0,5), (1,1), ... (5,5); entry 20 is the number of counted cells -- then the 6 values sum c_k * r,
 * then sum r * r.  Nothing overflows: |c2|, |c3| <= 2 * 511 * 254 = 259 588, a square is below 6.8e10, and 512^2 of them are
 * below 1.8e16 < 2^63.  Only gx and gy of a pair are read here; a pair with gx or gy outside [1, side] keeps all-zero sums.
 * Meaning of the sums, which fixes the signs: the model is A(X) ~ (1 + gamma) * B(X + d(X)) + o with the field, in cells,
 *     d = (tx - theta * y' + sigma * x', ty + theta * x' + sigma * y'),   (x', y') = (x, y) / 2
 * With N the symmetric 6 x 6 matrix of the products and R the six sums c_k * r, the solution q of N q = R gives
 *     tx = 2 q0    ty = 2 q1    theta = 4 q2 (radians, counter-clockwise)    sigma = 4 q3    gamma = q4    o = q5
 * (the central differences gxv, gyv are twice the gradient, and x, y twice the offset); without the exposure terms it is the
 * leading 4 x 4.  As in "Survey registration", B's content appears d displaced relative to A's, so the corrections u_f of
 * the two frames satisfy u_b(X) - u_a(X) = -d(X) * cell.
 * Asynchronous on `stream`, nothing allocated; sums_dev is zeroed on `stream` and accumulated into with 64-bit integer
 * vector atomics (integers: the order is irrelevant); plain vector loads and stores.  sums_dev and pairs_dev 8-byte aligned.
 * Bad arguments fail before any HIP call with a message that names the argument; n_pairs == 0 returns 0 before looking at
 * anything. */
#define WM_REGISTER_REFINE_SUMS 28
int wm_register_refine(const uint8_t* a_dev, const uint8_t* b_dev, const wm_register_pair* pairs_dev, int n_pairs, int search,
                       int side, int64_t* sums_dev /* [n_pairs][WM_REGISTER_REFINE_SUMS] */, void* stream);

/* Survey registration, pyramid (tiling.reduce_planes, tiling.refine(levels=L), tiling.register(refine=k, levels=L)): the
 * refinement above is one linearisation and converges from within about two cells at the patch corners.  A coarser `cell`
 * widens that basin, but wm_register_render_u8 samples the nearest pixel, so a coarse cell aliases the ground's fine
 * texture.  This entry reduces planes rendered at the FINE cell by 2 x 2 rounded means, so wm_register_refine can run on
 * area-averaged planes, coarse to fine, with a `cell` of 2^l times the fine one.
 * Rule (wm_register_reduce_u8), per plane, all in integers:
 *     R_0 = in
 *     R_{k+1}[j][i] = 0 if any of R_k[2j][2i], R_k[2j][2i+1], R_k[2j+1][2i], R_k[2j+1][2i+1] is 0,
 *                     else (their sum + 2) >> 2
 *     out = R_level
 * 0 keeps its meaning "not seen": a coarse cell is seen iff all 4^level fine cells under it are, and a seen cell stays in
 * 1..255 (four ones give (4 + 2) >> 2 = 1).  The rule is the recursion with its rounding at every level, not the rounded
 * mean of the 2^level x 2^level block: the 4 x 4 block of the 2 x 2 blocks [1,1,2,2], [1,1,2,2], [1,1,2,2], [1,1,1,2]
 * gives 2 where the rounded block mean is 1.
 * in_dev [n_planes][ext][ext] uint8 -> out_dev [n_planes][ext >> level][ext >> level] uint8.  Limits: 1 <= level <=
 * WM_REGISTER_MAX_LEVEL; 1 <= ext <= WM_REGISTER_MAX_SIDE + 2 * WM_REGISTER_MAX_SEARCH; ext % (1 << level) == 0; 0 <=
 * n_planes <= WM_REGISTER_MAX_PAIRS; in_dev and out_dev 4-byte aligned, their ranges disjoint.
 * Ring alignment: plane B of a render with search = 2^l has side + 2^(l+1) cells a side; with side % 2^l == 0 the reduced
 * B is the reduced A's grid grown by exactly one coarse cell on every side, which is what wm_register_refine needs
 * (search = 1, side >> l, pairs with gx >> l and gy >> l and the same x0, y0).
 * One pass: every input byte is read once and only R_level is written.  Asynchronous on `stream`, nothing allocated;
 * plain vector loads and stores, no atomics.  Bad arguments fail before any HIP call with a message that names the
 * argument; n_planes == 0 returns 0 before looking at any pointer. */
#define WM_REGISTER_MAX_LEVEL 6
int wm_register_reduce_u8(const uint8_t* in_dev /* [n_planes][ext][ext] */, int n_planes, int ext, int level,
                          uint8_t* out_dev /* [n_planes][ext >> level][ext >> level] */, void* stream);

/* Survey resampling (tiling.detect_frames(scale=..., resize=...)): a frame brought to the scale the checkpoint was trained
 * at (the val transform's long side of 768, dataloader_coco.py:288) before it is tiled.
 * wm_resample_u8: in_dev [height][width][3] uint8 -> out_dev [out_height][out_width][3] uint8, any size to any size (down
 * and up), with the 8-bit arithmetic of wm_preprocess_u8_resized = Pillow's ImagingResample bilinear filter: 22-bit
 * fixed-point coefficients, horizontal pass into an 8-bit intermediate, then the vertical pass, clip8((acc + 2^21) >> 22);
 * bit-exact with PIL.Image.resize(..., BILINEAR).  A pass whose size does not change is the identity (Pillow skips it).
 * Sides 1..65536; buffers must not overlap.  Coefficient tables are cached per (device, stream) for the last 8 geometries
 * and uploaded on the stream (a new geometry does not block the host); the intermediate image is scratch per (device,
 * stream), so calls on different streams may overlap.
 * wm_scaled_size: (out_h, out_w) = (max(1, floor(height * scale + 0.5)), the same for width), in double; scale positive
 * and finite, result sides <= 65536.  Host only. */
int wm_resample_u8(const uint8_t* in_dev, int height, int width, uint8_t* out_dev, int out_height, int out_width, void* stream);
int wm_scaled_size(int height, int width, double scale, int* out_h, int* out_w);

/* Survey lens (lens.lens_plan, preprocess.undistort_u8, tiling.undistorted): a frame resampled ONCE to the pinhole picture of
 * the same camera, so that the one affine per frame of the census, the coverage, the mosaic and the registration is true of
 * it.  No reference behaviour exists (the reference has no camera model); this rule is the contract, and tests/lens_cases.py
 * restates it sequentially (lens_oracle).  All arithmetic is IEEE double, every operation correctly rounded on its own (no
 * contraction), in the order and with the parentheses written.
 * Camera: camera[9] doubles fx, fy, cx, cy, k1, k2, p1, p2, k3 -- the Brown-Conrady model in OpenCV's order, as every
 * photogrammetry package exports it.  cx, cy follow OpenCV's convention, pixel CENTRES at integers; the pixel POSITION used
 * everywhere else in this header (centres at integer + 0.5) is that plus 0.5.
 * Output: a pinhole picture of out_height x out_width pixels (oh, ow below) with the one focal length f_out and its principal
 * point at its geometric centre, so tiling.nadir_affine(oh, ow, centre, gsd, yaw) holds for it with gsd = altitude / f_out.
 * For the output pixel of row j and column i:
 *     x   = (((double)i + 0.5) - 0.5 * (double)ow) / f_out          y = (((double)j + 0.5) - 0.5 * (double)oh) / f_out
 *     r2  = x * x + y * y
 *     rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
 *     xd  = x * rad + (((2.0 * p1) * x) * y + p2 * (r2 + 2.0 * (x * x)))
 *     yd  = y * rad + (p1 * (r2 + 2.0 * (y * y)) + ((2.0 * p2) * x) * y)
 *     u   = fx * xd + (cx + 0.5)                                    v = fy * yd + (cy + 0.5)
 * (u, v) is the position in the source frame.  The source pixel is INSIDE iff 0 <= u < width && 0 <= v < height (a NaN is
 * outside).  Inside, the three bytes are the sample "Survey mosaic" fetches at (u, v): WM_MOSAIC_NEAREST, the pixel
 * ((int)floor(v), (int)floor(u)), or WM_MOSAIC_BILINEAR, edge replicate, rounded as written there.  Outside, they are the
 * fill colour.  Every output byte is written by every call.  Shrinking aliases as the mosaic does (no area filter).
 * wm_undistort_u8: in_dev [height][width][3] uint8 -> out_dev [out_height][out_width][3] uint8; camera and fill_rgb (three
 * bytes) are read on the host during the call; mode is WM_MOSAIC_NEAREST or WM_MOSAIC_BILINEAR; stats_dev, unless NULL, is
 * one int64 that receives the number of output pixels that were filled (zeroed on `stream` first, then one 64-bit atomic
 * per workgroup that filled any).  One launch, a gather: plain loads and stores, no atomics on the picture, nothing
 * allocated, asynchronous on `stream`.  Limits: all four sides in 1..65536 (wm_resample_u8's); every camera entry finite;
 * fx, fy, f_out > 0 (f_out finite); stats_dev 8-byte aligned; the ranges of in_dev and out_dev disjoint.  Bad arguments fail
 * before any HIP call with a message that names the argument. */
int wm_undistort_u8(const uint8_t* in_dev, int height, int width, const double camera[9], uint8_t* out_dev, int out_height,
                    int out_width, double f_out, int mode, const uint8_t fill_rgb[3], int64_t* stats_dev /* [1], may be NULL */,
                    void* stream);

/* Survey attitude (attitude.attitude_rotation, attitude.rectify_plan, preprocess.rectify_u8, tiling.rectified): a frame taken
 * by a camera that was not level, resampled ONCE to the picture a level (nadir) pinhole camera at the same place would have
 * taken: the rotation and the lens model of "Survey lens" in one gather, so the frame is neither blurred nor paid for twice.
 * No reference behaviour exists; this rule is the contract, and tests/attitude_cases.py restates it sequentially
 * (attitude_oracle).  All arithmetic is IEEE double, every operation correctly rounded on its own (no contraction), in the
 * order and with the parentheses written.
 * Rotation: rot[9] doubles r0..r8, row-major, maps a ray of the level camera into the real camera: d_cam = rot * d_nadir.
 * Both frames have x to the picture's right, y down the picture and z along the optical axis.  Convention of
 * attitude.attitude_rotation(roll, pitch): the camera is fixed to the airframe, the optical axis points down, the picture's up
 * direction is the nose and its right the right wing; yaw stays in tiling.nadir_affine.  Pitch t > 0 is nose up (the axis
 * swings towards the picture's up direction), roll p > 0 is right wing down (the axis swings towards the picture's left).
 * With P = [[1,0,0],[0,cos t,-sin t],[0,sin t,cos t]] and Q = [[cos p,0,-sin p],[0,1,0],[sin p,0,cos p]], A = P Q maps
 * airframe to level and rot = A^T; the third column of A, the optical axis in level coordinates, is
 * (-sin p, -sin t cos p, cos t cos p).  The kernel does not require rot to be orthonormal: the rule is a homography.
 * Output: as in "Survey lens", out_height x out_width pixels (oh, ow), one focal length f_out, the principal point at the
 * geometric centre; tiling.nadir_affine(oh, ow, position, altitude / f_out, yaw) holds for it, position the ground point
 * straight below the camera.  For the output pixel of row j and column i:
 *     x  = (((double)i + 0.5) - 0.5 * (double)ow) / f_out          y = (((double)j + 0.5) - 0.5 * (double)oh) / f_out
 *     X  = (r0 * x + r1 * y) + r2
 *     Y  = (r3 * x + r4 * y) + r5
 *     Z  = (r6 * x + r7 * y) + r8
 * The pixel is OUTSIDE unless Z > 0 (a NaN is outside); otherwise
 *     xn = X / Z                                                   yn = Y / Z
 * and (xn, yn) goes through exactly the expressions of "Survey lens" in place of its (x, y): its r2 (the squared radius, not
 * the rotation's entry), rad, xd, yd, u, v.  The source pixel is INSIDE iff Z > 0 && 0 <= u < width && 0 <= v < height; inside,
 * the three bytes are "Survey mosaic"'s nearest or bilinear sample at (u, v); outside, the fill colour.  Every output byte is
 * written by every call.  With rot the identity X == x, Y == y and Z == 1 exactly, and the rule equals wm_undistort_u8's bit
 * for bit.
 * wm_rectify_u8: the arguments of wm_undistort_u8 and rot, read on the host during the call; stats_dev, unless NULL, is one
 * int64 that receives the number of output pixels that got the fill colour, those with Z <= 0 included (zeroed on `stream`
 * first, then one 64-bit atomic per workgroup that filled any).  One launch, a gather: plain loads and stores, no atomics on
 * the picture, nothing allocated, asynchronous on `stream`.  Limits and checks: wm_undistort_u8's, and every rot entry finite.
 * Bad arguments fail before any HIP call with a message that names the argument. */
int wm_rectify_u8(const uint8_t* in_dev, int height, int width, const double camera[9], const double rot[9], uint8_t* out_dev,
                  int out_height, int out_width, double f_out, int mode, const uint8_t fill_rgb[3],
                  int64_t* stats_dev /* [1], may be NULL */, void* stream);

/* Survey terrain (terrain.terrain_grid, terrain.camera_pose, terrain.ortho_plan, preprocess.ortho_u8, tiling.orthorectified): a
 * frame resampled ONCE onto a ground grid, each output pixel's height taken from a digital elevation model (DEM): the
 * orthophoto, whose affine georeference is exact whatever the relief.  "Survey attitude" takes the ground for the plane of
 * tiling.nadir_affine; a point z metres above that plane, d from the nadir point of a level camera H above it, is seen at
 * d * H / (H - z).  Lens, attitude, yaw, position and relief go into one gather, so the frame is neither blurred nor paid for
 * twice.  No reference behaviour exists; this rule is the contract, and tests/terrain_cases.py restates it sequentially
 * (terrain_oracle).  All arithmetic is IEEE double, every operation correctly rounded on its own (no contraction), in the
 * order and with the parentheses written.
 * DEM: dem_dev [dem_height][dem_width] float32 (dem_h, dem_w below), north-up: row 0 is the northernmost.  Heights are at cell
 * CENTRES (GeoTIFF's "pixel is area").  dem_geo[3] = (e0, n0, dcell): east and north of the grid's top-left CORNER, and the
 * post spacing in metres, so post [r][c] stands at (e0 + (c + 0.5) dcell, n0 - (r + 0.5) dcell).  Each float32 height is
 * converted to double exactly.
 * Pose: pose[12] = Ce, Cn, Cu, m0..m8.  (Ce, Cn, Cu) is the camera's position: east, north, and height in the DEM's own
 * vertical datum.  M = m0..m8, row-major, maps a world vector (east, north, up) into the camera frame of "Survey attitude": x
 * to the picture's right, y down the picture, z along the optical axis.  For a level camera whose picture-up heading is psi
 * clockwise from north, M = L(psi) = [[c, -s, 0], [-s, -c, 0], [0, 0, -1]] with c = cos psi, s = sin psi (the rows are
 * tiling.nadir_affine's (a0, a1) and (a3, a4) over the ground sampling distance; the determinant is +1).  With roll and pitch,
 * M = rot L(psi), rot being "Survey attitude"'s.  The kernel does not require M to be orthonormal.
 * Output: out_height x out_width pixels (oh, ow), and out_geo[6] = g0..g5, its pixel-to-ground affine exactly as wm_census
 * takes one.  For the output pixel of row j and column i, with px = (double)i + 0.5 and py = (double)j + 0.5:
 *     E  = (g0 * px + g1 * py) + g2                                N  = (g3 * px + g4 * py) + g5
 *     a  = (E - e0) / dcell - 0.5                                  b  = (n0 - N) / dcell - 0.5
 * The pixel HAS A HEIGHT iff 0 <= a && a <= dem_w - 1 && 0 <= b && b <= dem_h - 1 (a NaN has none).  Then
 *     ia = min((int)floor(a), dem_w - 2)                           ib = min((int)floor(b), dem_h - 2)
 *     ta = a - (double)ia                                          tb = b - (double)ib
 *     z  = (z00 * (1.0 - ta) + z01 * ta) * (1.0 - tb) + (z10 * (1.0 - ta) + z11 * ta) * tb
 *            with z00 = dem[ib][ia], z01 = dem[ib][ia + 1], z10 = dem[ib + 1][ia], z11 = dem[ib + 1][ia + 1]
 *     dE = E - Ce                   dN = N - Cn                    dU = z - Cu
 *     X  = (m0 * dE + m1 * dN) + m2 * dU
 *     Y  = (m3 * dE + m4 * dN) + m5 * dU
 *     Z  = (m6 * dE + m7 * dN) + m8 * dU
 * The pixel is OUTSIDE unless it has a height and Z > 0 (a NaN is outside: a post that is not finite -- nodata -- leaves no
 * finite (u, v) below); otherwise
 *     xn = X / Z                                                   yn = Y / Z
 * and (xn, yn) goes through exactly the expressions of "Survey lens" in place of its (x, y): its r2, rad, xd, yd, u, v.  The
 * source pixel is INSIDE iff it has a height && Z > 0 && 0 <= u < width && 0 <= v < height; inside, the three bytes are
 * "Survey mosaic"'s nearest or bilinear sample at (u, v); outside, the fill colour.  Every output byte is written by every
 * call.  Occlusion is NOT tested: a cell hidden behind a ridge shows the ridge's pixel (no true-ortho visibility).
 * wm_ortho_u8: in_dev [height][width][3] uint8 -> out_dev [out_height][out_width][3] uint8; camera, pose, dem_geo, out_geo
 * and fill_rgb are read on the host during the call, dem_dev on the device; mode is WM_MOSAIC_NEAREST or WM_MOSAIC_BILINEAR.
 * stats_dev, unless NULL, is two int64: [0] the number of output pixels that got the fill colour, [1] how many of those had
 * no height or a height that is not finite -- the diagnostic for a DEM that is too small (both zeroed on `stream` first, then
 * at most one 64-bit atomic each per workgroup).  One launch, a gather: plain loads and stores, no atomics on the picture,
 * nothing allocated, asynchronous on `stream`.  Limits and checks: wm_rectify_u8's on the frame, the camera, the picture's
 * sides, mode, fill, stats_dev's alignment and the disjoint ranges of in_dev and out_dev; every pose, dem_geo and out_geo entry
 * finite; dcell > 0; dem_height and dem_width in 2..32768; dem_dev 4-byte aligned, its range disjoint from out_dev's.  Bad
 * arguments fail before any HIP call with a message that names the argument. */
int wm_ortho_u8(const uint8_t* in_dev, int height, int width, const double camera[9], const double pose[12], const float* dem_dev,
                int dem_height, int dem_width, const double dem_geo[3], uint8_t* out_dev, int out_height, int out_width,
                const double out_geo[6], int mode, const uint8_t fill_rgb[3], int64_t* stats_dev /* [2], may be NULL */, void* stream);

/* Survey review chips (tiling.detect_frames(chips=...), tiling.crop_chips): one chip x chip uint8 crop per detection, each
 * with a window and a scale of its own, in one launch.
 * The chip rule, fp32 with every operation rounded on its own, for a box (x0, y0, x1, y1) in frame pixels:
 *   m = max(x1 - x0, y1 - y0);  s = ceilf(m * context) clamped to [min_side, max_side];  side = (int)s
 *   cx = (x0 + x1) * 0.5f;  cy = (y0 + y1) * 0.5f
 *   x0w = floorf(cx - 0.5f * side);  y0w = floorf(cy - 0.5f * side), each clamped to [-2^30, 2^30];  window = (y0w, x0w, side)
 * A box with a non-finite coordinate, or a frame index outside [0, n_frames), has the window (0, 0, 0) and an all-zero chip.
 * The chip is PIL.Image.fromarray(Wimg).resize((chip, chip), BILINEAR) bit for bit, Wimg the side x side x 3 image of the
 * window's pixels with zeros where the window reaches past the frame: wm_resample_u8's arithmetic, filter taps clipped at
 * the WINDOW's edge, zeros from outside the frame taking part as ordinary pixels, both passes the identity where side ==
 * chip.  A window that does not meet its frame gives an all-zero chip.
 * wm_chip_window: the rule on the host (no device call).
 * wm_crop_chips_u8: frames_dev [n_frames] as for wm_tile_frames_u8, boxes_dev [n][4] xyxy fp32 and box_frame_dev [n] (NULL:
 * every box in frame 0) on the device, n a host count -> chips_dev [n][chip][chip][3] uint8 and, unless NULL, windows_dev
 * [n][3] = (y0, x0, side).  Windows and coefficient tables are derived on the device: no handle, no scratch, no
 * allocation, no upload; asynchronous on `stream`.  chip a multiple of 4 in 16..256, chips_dev 4-byte aligned, context in
 * [1, 8], 1 <= min_side <= max_side <= WM_CHIP_MAX_SIDE, n >= 0 (n == 0 returns 0 before looking at any pointer); bad
 * arguments fail before any HIP call. */
#define WM_CHIP_MAX_SIDE 1024
int wm_chip_window(const float box[4], float context, int min_side, int max_side, int32_t out[3]);   /* host only */
int wm_crop_chips_u8(const wm_frame_desc* frames_dev, int n_frames, const float* boxes_dev /* [n][4] xyxy */,
                     const int32_t* box_frame_dev /* [n], NULL = all frame 0 */, int n, int chip, float context,
                     int min_side, int max_side, uint8_t* chips_dev /* [n][chip][chip][3] */,
                     int32_t* windows_dev /* [n][3] (y0, x0, side), may be NULL */, void* stream);

/* Survey overlays (tiling.detect_frames(overlay=...), tiling.draw_boxes, visualize.plot_points): box outlines drawn onto
 * uint8 frames in place, and the reference's tile preparation (visualize_prediction.py:118-133).
 * The outline rule, for a box (x0, y0, x1, y1) in the pixels of its frame:
 *   each coordinate is clamped to [-2^30, 2^30] and truncated toward zero, as the reference's int(box[k]) does: (l, t, r, b),
 *   with r and b INCLUSIVE.
 *   A box is skipped -- it draws nothing and is not an error -- if a coordinate is not finite, if r < l or b < t, if its
 *   frame index is outside [0, n_frames), or if its label is outside [0, palette_size).
 *   The outline is every pixel (x, y) with l <= x <= r and t <= y <= b that lies inside the frame and satisfies
 *     x - l < width  or  r - x < width  or  y - t < width  or  b - y < width.
 *   The border grows inward, clipped to the frame; nothing is drawn outside the box.  This is the pixel set of
 *   PIL.ImageDraw.rectangle([l, t, r, b], outline=c, width=width) whenever r - l + 1 and b - t + 1 both exceed width
 *   (Pillow 12.2.0; its line code paints outside the box when a side is smaller, which is not copied).  cv2.rectangle's
 *   thickness-2 raster, which the reference calls, is not matched: OpenCV straddles the edge, this rule stays inside it.
 *   An outline pixel gets the three bytes palette[label], no blending.
 *   Painter's order: the frames end as if the boxes had been drawn one after another in index order, later over earlier,
 *   bit for bit, with exactly one store per written pixel (deterministic, race-free).
 * wm_box_outline_rect: the first step on the host (no device call): out = (l, t, r, b) and 0, or out = zeros and 1 for a
 * box that is skipped for its coordinates; <0 on a NULL argument.
 * wm_draw_boxes_u8: frames_dev [n_frames] as for wm_crop_chips_u8 (the frames are WRITTEN), boxes_dev [n][4] xyxy fp32,
 * labels_dev [n] int32, box_frame_dev [n] (NULL: every box in frame 0), palette_dev [palette_size][3] uint8, all on the
 * device; n a host count.  One launch, no handle, no scratch, no allocation; asynchronous on `stream`.  width in
 * 1..WM_DRAW_MAX_WIDTH, palette_size in 1..WM_DRAW_MAX_PALETTE, n >= 0 (n == 0 returns 0 before looking at any pointer);
 * bad arguments fail before any HIP call.
 * wm_plot_image_u8: in_dev [batch][3][height][width] fp32 -> out_dev [batch][height][width][3] uint8, per image
 *   out[y][x][c] = (int)(((v - mn) / mx) * 255.0f),  v = in[2 - c][y][x]  (the reference's cvtColor swaps channels 0 and 2),
 *   mn the image's minimum over all three channels, mx the maximum of v - mn; every operation a correctly rounded fp32
 * operation of its own, so the bytes are those of numpy's
 *   a = x.transpose(1,2,0)[..., ::-1].copy(); a -= a.min(); a /= a.max(); np.int32(a * 255).
 * A constant image (mx == 0; the reference divides by zero there) gives all zeros; a non-finite input gives unspecified
 * bytes and no fault.  Two launches (a deterministic two-stage min / max, then the map); scratch_dev holds at least batch *
 * WM_PLOT_SCRATCH_BYTES bytes, 4-byte aligned, and is the caller's: no allocation, asynchronous on `stream`.  batch == 0
 * returns 0 before looking at any pointer; bad arguments fail before any HIP call. */
#define WM_DRAW_MAX_WIDTH 16
#define WM_DRAW_MAX_PALETTE 256
#define WM_PLOT_SCRATCH_BYTES 1024
int wm_box_outline_rect(const float box[4], int32_t out[4]);   /* host only; 0 drawn, 1 skipped */
int wm_draw_boxes_u8(const wm_frame_desc* frames_dev, int n_frames, const float* boxes_dev /* [n][4] xyxy */,
                     const int32_t* labels_dev /* [n] */, const int32_t* box_frame_dev /* [n], NULL = all frame 0 */, int n,
                     const uint8_t* palette_dev /* [palette_size][3] */, int palette_size, int width, void* stream);
int wm_plot_image_u8(const float* in_dev, int batch, int height, int width, uint8_t* out_dev, void* scratch_dev,
                     int64_t scratch_bytes, void* stream);

/* ---- intermediate taps (parity tests) -------------------------------------
 * Copies the fp32 token stream (B,64,64,embed_dim) as it stood after the patch embed + pos_embed
 * (which = -3, image_encoder.py:124-126), after the stem = that + the HFC adaptor's output (which = -1,
 * image_encoder.py:128-131: the input of blocks[0]) or after block `which` of the most recent
 * wm_encoder_forward with taps enabled.  wm_set_tap selects which single point is captured. */
int wm_set_tap(wm_handle* h, int which);      /* -2 = off */
int wm_read_tap(wm_handle* h, float* out_dev, int batch, void* stream);

/* ---- per-kernel timing (bench.py roofline) --------------------------------
 * When enabled, every launch of a kernel class is bracketed by HIP events on
 * the launch stream.  wm_profile_read synchronises and returns, per class,
 * launches, total milliseconds and total algorithmic FLOPs/bytes since the
 * last wm_profile_reset. */
#define WM_KCLASS_GEMM16 0       /* 16-bit MFMA GEMM (qkv/proj/MLP/1x1 convs/embeds) */
#define WM_KCLASS_ATTN_WIN 1
#define WM_KCLASS_ATTN_GLOBAL 2
#define WM_KCLASS_LAYERNORM 3
#define WM_KCLASS_OTHER 4
#define WM_KCLASS_COUNT 5
typedef struct wm_kclass_stat {
    int64_t launches;
    double  ms;
    double  flops;
    double  bytes;
} wm_kclass_stat;
int wm_profile_enable(wm_handle* h, int on);
int wm_profile_reset(wm_handle* h);
int wm_profile_read(wm_handle* h, wm_kclass_stat* out /* [WM_KCLASS_COUNT] */);

/* ---- which GEMM kernel instance ran (parity tests) -------------------------
 * Process-wide launch counts per 16-bit GEMM kernel instance since the last reset.  The dispatch between the
 * instances is a heuristic on (M, N, K); the tests assert on these counters so that a heuristic change can never
 * silently leave an instance (e.g. the 256x320 staggered kernel with the LDS-DMA residual epilogue that the ViT-H
 * bench runs) without a value check. */
#define WM_GEMM_V1_128 0        /* gemm16_kernel 128x128x64 (M % 256 != 0) */
#define WM_GEMM_V2_160 1        /* gemm16v2_kernel<160>: half-width, few tiles (1-2 image tiles per call) */
#define WM_GEMM_V2_128 2        /* gemm16v2_kernel<128> */
#define WM_GEMM_V3_LOCKSTEP 3   /* (round 1-2 A/B instance, no longer built; id kept) */
#define WM_GEMM_V3_CONV3X3 4    /* gemm16v3_kernel AMODE 1: implicit-GEMM 3x3 conv (neck) */
#define WM_GEMM_V5_320 5        /* gemm16v5_kernel<320>, no residual */
#define WM_GEMM_V5_320_RES 6    /* gemm16v5_kernel<320>, fp32 residual by LDS-DMA (proj / lin2 of ViT-H) */
#define WM_GEMM_V5_256 7        /* gemm16v5_kernel<256>, no residual */
#define WM_GEMM_V5_256_RES 8    /* gemm16v5_kernel<256>, fp32 residual */
#define WM_GEMM_V5_320_LNF 9    /* (rounds 1-2: fused-LayerNorm instance, no longer built; id kept) */
#define WM_GEMM_V5_256_LNF 10
#define WM_GEMM_FP8_320 11      /* gemm8_kernel<320>: MX-fp8 block-scaled MFMA (WM_PREC_FP8) */
#define WM_GEMM_FP8_256 12      /* gemm8_kernel<256> */
#define WM_GEMM_V5_320_FOLDP 13 /* gemm16v5_kernel<320> fp32 + residual + row statistics + 16-bit copy (folded LayerNorm, producer) */
#define WM_GEMM_V5_256_FOLDP 14
#define WM_GEMM_V5_320_SPLIT 15 /* gemm16v5_kernel<320> split-stream producer: residual planes (hi, lo) in and out, row statistics (round 4) */
#define WM_GEMM_V5_256_SPLIT 16
#define WM_GEMM_V3_PATCH 17     /* gemm16v3_kernel AMODE 2: implicit-GEMM 16x16 / stride-16 patch embed (round 4) */
#define WM_GEMM_FP8_256_PLANES 18 /* gemm8_kernel<256> with the stream as planes of rows (hi, lo) in and out (fp8 blocks' proj / lin2, round 4) */
#define WM_GEMM_V5_320_WALK 19  /* a gemm16v5_kernel<320> folded-LayerNorm consumer whose workgroups walk several column tiles; counted IN ADDITION to WM_GEMM_V5_320 */
#define WM_GEMM_V5_256_WALK 20
#define WM_GEMM_VARIANT_COUNT 21
int wm_debug_gemm_variant_counts(int64_t* out /* [WM_GEMM_VARIANT_COUNT] */, int n);
int wm_debug_reset_gemm_variant_counts(void);

/* ---- saturation census (opt-in; a trained checkpoint with activation outliers) ----------------------------------------
 * fp16 operands clamp at +-65504 (every fp32 -> fp16 conversion of the path saturates instead of producing inf) and e4m3
 * operands at +-448.  With the census enabled, every encoder forward counts, after the kernel that produced them, the
 * elements of the blocks' operand buffers that sit AT the clamp value (or are inf / NaN: bf16): LayerNorm outputs, the
 * packed qkv, the attention output, the GELU hidden, the 16-bit copy of the last block's output.  A non-zero count
 * means clamped operands: switch that checkpoint to WM_PREC_BF16 (no clamp, 8-bit mantissa).  Costs one streaming read of
 * each buffer; off by default and absent from timed runs. */
/* Always on (round 4): the producers of the residual stream's fp16 plane (residual GEMM epilogues, the standalone statistics
 * kernel) set a host-visible word when a stream value reaches the fp16 clamp (|x| >= 65504).  wm_stream_overflow returns WM_OVERFLOW_STREAM if
 * that happened since the last reset (kernels that have finished; no synchronisation), 0 otherwise.  The Python drop-in checks
 * it at every call and warns once: such a checkpoint should run with WM_PREC_BF16. */
/* The decoder's GEMMs (fp32 values split into fp16 pairs, gemm32.h) raise a second word when an operand leaves fp16's range
 * (|activation| >= 65504 or |weight| >= 1023; the affected products are inf / nan, not clamped values): WM_GEMM32_F32=1 keeps the fp32 MFMA.
 * Return value: a mask of the two. */
#define WM_OVERFLOW_STREAM 1
#define WM_OVERFLOW_DECODER 2
int wm_stream_overflow(wm_handle* h, int reset);

#define WM_SAT_LN 0
#define WM_SAT_QKV 1
#define WM_SAT_ATTN 2
#define WM_SAT_HID 3
#define WM_SAT_LAST 4
#define WM_SAT_COUNT 5
int wm_debug_saturation_enable(wm_handle* h, int on);
int wm_debug_saturation_read(wm_handle* h, int64_t* out /* [WM_SAT_COUNT] */, int n, int reset, void* stream);

/* ---- single-op entry points (kernel-level parity tests) --------------------
 * Thin launches of individual kernels on caller-provided device buffers.
 * 16-bit buffers hold bf16 or fp16 per `precision`. */

/* fp32 -> 16-bit and back */
int wm_op_cvt_f32_to_16(const float* in_dev, void* out_dev, int64_t n, int precision, void* stream);
int wm_op_cvt_16_to_f32(const void* in_dev, float* out_dev, int64_t n, int precision, void* stream);

/* C[M,N] = act(A[M,K] * W[N,K]^T + bias) (+ residual[(row % res_mod), N]).
 * A, W 16-bit; bias/residual fp32 or NULL; out_f32 and/or out_16 (either may be NULL).
 * act: 0 none, 1 GELU(erf), 2 ReLU.  res_mod <= 0 means M.
 *
 * Operand layout flags, OR-ed into `act` (round 3).  The 256-row-tile kernel stages operands by 1 KiB LDS-DMA pieces
 * (16 rows x 64 B of one 32-deep K-step); from a row-major operand a piece is 16 half lines, in "LDS-image order" it is 8
 * whole 128-byte lines, which is worth 8 % of the GEMM time.  LDS-image order of a [rows][K] 16-bit matrix (rows % 16 == 0,
 * K % 32 == 0): [rows / 16][K / 32][64 positions x 16 B], position l holding row l >> 2, 16-byte chunk (l & 3) ^ ((-(l >> 4)) & 3)
 * of the 16 x 32 block (wm_op_pack16 produces it).  The engine packs every encoder GEMM weight at wm_finalize_weights and its
 * LayerNorm / GELU epilogues write the activations that feed such a GEMM in this order; results are bit-identical to the
 * row-major path.  Only shapes for which wm_op_gemm16_takes_packed() returns 1 accept the flags. */
#define WM_GEMM_W_PACKED 0x1000     /* w_dev is in LDS-image order */
#define WM_GEMM_A_PACKED 0x2000     /* a_dev is in LDS-image order */
#define WM_GEMM_OUT_PACKED 0x4000   /* out_16_dev is written in LDS-image order (16-bit-only form: no fp32 output, no residual) */
#define WM_LAYOUT_PACKED 0x100      /* wm_op_layernorm: OR into `precision`, 16-bit-only form: out_16_dev in LDS-image order */
int wm_op_gemm16(const void* a_dev, const void* w_dev, const float* bias_dev,
                 const float* residual_dev, int res_mod, float* out_f32_dev, void* out_16_dev,
                 int M, int N, int K, int act, int precision, void* stream);
int wm_op_gemm16_takes_packed(int M, int N, int K);

/* Folded LayerNorm, the three pieces as single ops (kernel-level parity tests; the engine uses them under WM_CFG_FOLD_LN).
 * wm_op_ln_stats16: x [rows][C] fp32 -> stats [rows][C / BN][2] = per-row (mean, M2) over column tiles of BN = 320 (C % 320 == 0)
 *   or 256 columns, and x16 = the rows as 16-bit in LDS-image order (rows % 16 == 0, C / BN <= 4).
 * wm_op_fold_weight16: w16 [N][K] 16-bit row-major, gamma / beta [K], bias [N] (may be NULL) -> wf = round16(gamma (.) w16) in
 *   LDS-image order, c1[n] = sum_k wf[n][k], c2[n] = sum_k beta[k] w16[n][k] + bias[n].
 * wm_op_gemm16_folded: out16 = act(rstd (x16 wf^T - mean c1) + c2) with (mean, rstd) combined per row from `stats`
 *   = act(LayerNorm(x; gamma, beta, eps) w16^T + bias) up to operand rounding; act 0 | 1 (GELU), optional WM_GEMM_OUT_PACKED.
 * wm_op_gemm16_stats: out_f32 = residual + a w^T + bias (may alias), plus stats and x16 of out_f32 as wm_op_ln_stats16
 *   writes them (bit-identical: same arithmetic); `layout`: WM_GEMM_W_PACKED | WM_GEMM_A_PACKED. */
int wm_op_ln_stats16(const float* x_dev, float* stats_dev, void* x16_dev, int64_t rows, int C, int precision, void* stream);
int wm_op_fold_weight16(const void* w16_dev, const float* gamma_dev, const float* beta_dev, const float* bias_dev, void* wf_dev,
                        float* c1_dev, float* c2_dev, int N, int K, int precision, void* stream);
int wm_op_gemm16_folded(const void* x16_dev, const void* wf_dev, const float* c1_dev, const float* c2_dev, const float* stats_dev,
                        float eps, void* out_16_dev, int M, int N, int K, int act, int precision, void* stream);
/* wm_op_gemm16_folded with the column tiles per workgroup given (csrc/gemm16_v5.h "Column walk"): walk = 0 the launcher's choice (what
 * wm_op_gemm16_folded and the engine run), 1 one tile per workgroup, T > 1 that many whatever the grid size; a T that does not divide
 * (N / tile width) / 4 runs as 1.  With walk > 0 the 256-row-tile kernel runs every shape it can (M % 256 == 0, N % 320 or 256 == 0,
 * K % 32 == 0, K >= 64), also those the dispatch would give to a half-width kernel.  The output bits do not depend on walk. */
int wm_op_gemm16_folded_walk(const void* x16_dev, const void* wf_dev, const float* c1_dev, const float* c2_dev, const float* stats_dev,
                             float eps, void* out_16_dev, int M, int N, int K, int act, int walk, int precision, void* stream);
int wm_op_gemm16_stats(const void* a_dev, const void* w_dev, const float* bias_dev, const float* residual_dev, float* out_f32_dev,
                       void* x16_dev, float* stats_dev, int M, int N, int K, int layout, int precision, void* stream);
int wm_op_pack16(const void* in_dev, void* out_dev, int64_t rows, int K, void* stream);
int wm_op_unpack16(const void* in_dev, void* out_dev, int64_t rows, int K, void* stream);     /* the inverse: LDS-image order -> row-major */

/* Split residual stream (round 4; csrc/gemm16_v5.h "Split stream").  The blocks' residual stream x is kept as two 16-bit planes
 * in LDS-image order: hi = round16(x) in the block's operand type (it IS the folded LayerNorm's operand) and lo = fp16(x - hi);
 * x = hi + lo carries 22 (fp16) / 19 (bf16) significant bits, and a residual GEMM's epilogue moves 8 instead of 10 bytes per element.
 * wm_op_ln_stats16_split: as wm_op_ln_stats16, also writing lo and, with x_rw_dev (may alias x_dev), the fp32 rows rounded to
 *   float(hi) + float(lo): what a small call (fp32 stream) does so that its bits equal a large call's (split stream).
 * wm_op_gemm16_split: (hi, lo) += a w^T + bias, in place: v = (acc + bias) + (float(hi) + float(lo)), statistics of v as
 *   wm_op_gemm16_stats writes them, hi' = round16(v), lo' = fp16(v - hi').  `layout`: WM_GEMM_W_PACKED | WM_GEMM_A_PACKED.
 * wm_op_stream_merge: out[rows][C] fp32 = float(hi) + float(lo). */
int wm_op_ln_stats16_split(const float* x_dev, float* stats_dev, void* hi_dev, void* lo_dev, float* x_rw_dev, int64_t rows, int C,
                           int precision, void* stream);
int wm_op_gemm16_split(const void* a_dev, const void* w_dev, const float* bias_dev, void* hi_dev, void* lo_dev, float* stats_dev,
                       int M, int N, int K, int layout, int precision, void* stream);
int wm_op_stream_merge(const void* hi_dev, const void* lo_dev, float* out_dev, int64_t rows, int C, int precision, void* stream);

/* fp8 (OCP e4m3) GEMM of WM_PREC_FP8, gemm8.h: C = act((A W^T) * wscale[n] + bias[n]) (+ residual).
 * a [M,K] e4m3 (unit scale), w [N,K] e4m3, wscale [N] fp32; exactly one of: residual + out_f32 (+ out_16), out_8 (e4m3),
 * out_16 alone.  M % 256 == 0, N % 256 == 0, K % 128 == 0, K >= 256.  precision = type of out_16 (WM_PREC_BF16 | FP16). */
int wm_op_gemm8(const void* a_dev, const void* w_dev, const float* wscale_dev, const float* bias_dev,
                const float* residual_dev, float* out_f32_dev, void* out_16_dev, void* out_8_dev,
                int M, int N, int K, int act, int precision, void* stream);
/* The fp8 blocks' residual stream as two 16-bit planes of rows (round 4): hi = round16(x) of type `precision`, lo = fp16(x - hi).
 * Inside a row each 256-column block is held in the residual epilogue's pass order: column c sits at position
 * (c & ~255) + ((c >> 5) & 1) * 128 + ((c >> 6) & 3) * 32 + (c & 31).   C % 256 == 0.
 * wm_op_stream_rows: merge == 0: fp32 x[rows][C] (row-major) -> (hi, lo); merge != 0: (hi, lo) -> x = float(hi) + float(lo).
 * wm_op_gemm8_planes: (hi, lo) [M,N] += (a w^T) * wscale[n] + bias[n], in place: v = (acc * wscale + bias) + (float(hi) + float(lo)),
 *   hi' = round16(v), lo' = fp16(v - hi'); shapes as wm_op_gemm8.
 * wm_op_layernorm_fp8_plane: the blocks' LayerNorm on the hi plane, position-wise: out_8[row][p] = e4m3(LN(x)[column at position p]),
 *   i.e. e4m3 rows in the SAME column order; the consuming wm_op_gemm8 takes a weight whose K columns are permuted alike.  Mean and
 *   centred variance over the row (not the column-tiled sums of wm_op_layernorm).  512 <= C <= 1536. */
int wm_op_stream_rows(float* x_f32_dev, void* hi_dev, void* lo_dev, int64_t rows, int C, int precision, int merge, void* stream);
int wm_op_gemm8_planes(const void* a_dev, const void* w_dev, const float* wscale_dev, const float* bias_dev, void* hi_dev, void* lo_dev,
                       int M, int N, int K, int precision, void* stream);
int wm_op_layernorm_fp8_plane(const void* hi_dev, const float* gamma_dev, const float* beta_dev, float eps, void* out_8_dev, int64_t rows, int C,
                              int precision, void* stream);
/* fp32 -> e4m3 bytes, unit scale, round to nearest even, saturating at +-448 (n % 4 == 0) */
int wm_op_cvt_f32_to_fp8(const float* in_dev, void* out_dev, int64_t n, void* stream);

/* 3x3 / stride 1 / pad 1 convolution without bias over a 64x64 token grid as an implicit GEMM (no im2col
 * buffer): the second neck conv, image_encoder.py:113-119.  a [B,64,64,c_in] NHWC 16-bit,
 * w [c_out][ky*3+kx][c_in] 16-bit (packed tap-major), out [B*4096, c_out] fp32.  c_out % 256 == 0, c_in % 32 == 0. */
int wm_op_conv3x3_16(const void* a_dev, const void* w_dev, float* out_dev, int batch, int c_out, int c_in,
                     int precision, void* stream);

/* 16 x 16 / stride-16 patch embedding (PatchEmbed / HfcEmbed, image_encoder.py:386-450) as an implicit GEMM, no im2col buffer:
 * img16 [batch][c_in][1024][1024] 16-bit NCHW, w [n_out][c_in * 256] 16-bit row-major (Conv2d weight flattened), bias fp32 or
 * NULL; out [batch * 4096][n_out] token-major, fp32 and / or 16-bit.  n_out % 320 == 0 or % 256 == 0. */
int wm_op_patch_embed16(const void* img16_dev, const void* w_dev, const float* bias_dev, float* out_f32_dev, void* out_16_dev,
                        int batch, int n_out, int c_in, int precision, void* stream);

/* fp32 GEMM, fp32 in and out, same contract (act 3 = sigmoid): on the fp32-input MFMA, or with act | WM_GEMM32_SPLIT in the form the
 * decoder runs since round 4: every operand value split into two fp16 numbers (hi + 2^-11 lo = x to 2^-22 |x| + 2^-36), three 16-bit
 * MFMAs per product (the lo x lo term dropped), fp32 accumulate: rel-L2 3e-7 against float64 (the fp32 MFMA: 1e-7); the error of
 * each row of A and column of W stays below 2e-7 of that row / column of |A| |W|^T down to rows of size 1e-4, and below 2e-6 down
 * to 1e-5 (tests/test_gpu_ranges.py).  K % 32 == 0 for that form. */
#define WM_GEMM32_SPLIT 0x100
/* act | WM_GEMM32_PRESPLIT: the same split form as the decoder inside wm_forward runs it, W split once into fp16 planes
 * (split_w32_kernel, into a scratch buffer of the stream) and read pre-split by the GEMM.  Exclusive with WM_GEMM32_SPLIT. */
#define WM_GEMM32_PRESPLIT 0x200
int wm_op_gemm32(const float* a_dev, const float* w_dev, const float* bias_dev,
                 const float* residual_dev, float* out_dev, int M, int N, int K, int act, void* stream);

/* LayerNorm over the last dim of [rows, C] fp32 (biased variance); writes fp32 and/or 16-bit
 * (precision WM_PREC_FP8 with out_f32 NULL: e4m3 bytes into out_16, the blocks' form only). */
int wm_op_layernorm(const float* x_dev, const float* gamma_dev, const float* beta_dev, float eps,
                    float* out_f32_dev, void* out_16_dev, int64_t rows, int C, int precision, void* stream);

/* Attention of image_encoder.py:246-262 on a packed qkv buffer [B*4096, 3*D] (16-bit),
 * D = heads*head_dim.  window = 14 (25 padded windows per tile, padded keys/values = qkv bias,
 * image_encoder.py:190-194,278-285) or 0 (global 4096 keys).  rel_pos_h/w fp32
 * [(2*size-1), head_dim].  qkv_bias fp32 [3*D] (used for the padded tokens).  out 16-bit [B*4096, D]. */
int wm_op_encoder_attention(const void* qkv_dev, const float* qkv_bias_dev,
                            const float* rel_pos_h_dev, const float* rel_pos_w_dev, void* out_dev,
                            int batch, int heads, int head_dim, int window, int precision, void* stream);

/* The same with q, k and v as three [B*4096, >= D] tensors of one token stride (elements): any layout whose heads are
 * head_dim-wide column groups, e.g. a head-major copy passed as batch = B*heads images of one head
 * (tools/attn_headmajor_probe.py). */
int wm_op_encoder_attention_qkv(const void* q_dev, const void* k_dev, const void* v_dev, int token_stride,
                                const float* qkv_bias_dev, const float* rel_pos_h_dev, const float* rel_pos_w_dev,
                                void* out_dev, int batch, int heads, int head_dim, int window, int precision, void* stream);

/* Plain multi-head attention softmax(q k^T / sqrt(hd)) v, no bias terms (HFC adaptor,
 * image_encoder.py:500-503).  q [B,Nq,*] row stride q_stride, k/v [B,Nk,*] (16-bit). */
int wm_op_mha16(const void* q_dev, int q_stride, const void* k_dev, int k_stride,
                const void* v_dev, int v_stride, void* out_dev, int out_stride,
                int batch, int heads, int head_dim, int nq, int nk, int precision, void* stream);

/* fp32 attention of the decoder (transformer.py:217-240 core), q [B,Nq,heads*hd], k/v [B,Nk,heads*hd]. */
int wm_op_mha32(const float* q_dev, const float* k_dev, const float* v_dev, float* out_dev,
                int batch, int heads, int head_dim, int nq, int nk, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* WM_HIP_H */
