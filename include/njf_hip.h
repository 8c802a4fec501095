/*
 * njf_hip.h -- C ABI of the MI355X (gfx950) volumetric-rendering hot path of Neural Jacobian Fields.
 *
 * The reference (sizhe-li/neural-jacobian-field) has no FFI: its seam is the Python object API of
 * project/neural_jacobian_field/models/model.py (Model.forward :316, encode_image :458,
 * compute_density :416) and the operator registry in models/decoder/__init__.py:11-44.  This header
 * is the boundary placed *underneath* that API: every entry point names the
 * reference code it replaces.  INTEGRATION.md shows the ctypes binding a maintainer adds on the
 * reference side.
 *
 * Conventions
 *   - Every pointer is a DEVICE pointer to fp32 unless noted; tensors are dense row-major.
 *   - Caller owns all memory; the library never allocates, frees or keeps state between calls.
 *   - All work is enqueued on `stream` (a hipStream_t passed as void*); no host synchronisation.
 *   - Return value: 0 = ok; negative = invalid argument (nothing was launched, see
 *     njf_error_string); positive = a hipError_t from the launch.
 *   - Re-entrant and thread-safe.
 *
 * Packed-weight layout ("fragment-major")
 *   The fused kernels keep activations in MFMA C/D registers between layers
 *   (v_mfma_f32_32x32x2_f32; a wave owns 32 points, lane l owns point l&31 and half l>>5 of the
 *   features).  A layer y = W x + b with W [d_out, d_in] (torch.nn.Linear layout) is stored as
 *   P[kb][q][mb][lane][e] = W[fo(mb, lane&31)][16*KB*(lane>>5) + 16*kb + 4*q + e]
 *   with MB = ceil(d_out/32), KB = ceil(d_in/32), zero padding, and
 *   fo(mb, i) = 16*MB*((i>>2)&1) + 16*mb + (i&3) + 4*(i>>3).
 *   njf_pack_* produce these blobs from reference-layout tensors; callers never build them by hand.
 */
#ifndef NJF_HIP_H
#define NJF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NJF_ABI_VERSION 20
#define NJF_MAX_ACTION_DIM 10   /* 3*A <= 32 outputs of the Jacobian head */
#define NJF_HIDDEN 128          /* MlpCfg.d_hidden (model_components/resnet_fc.py:12-18) */
#define NJF_LATENT 512          /* encoder feature channels (models/encoder/encoder_resnet.py:88) */
#define NJF_PE_DIM 63           /* NeRFEncoding(3, 10 freqs, include_input) output width */
#define NJF_ZDIM 384            /* 3 lin_z layers x 128: channels of one net's hoisted feature map */

/* floats in one packed ResnetFC blob (weights) and its bias blob */
#define NJF_RESNET_CHUNKS 22
#define NJF_RESNET_CHUNKS_F16 12  /* NJF_PRECISION_F16 fills the first 12 chunk slots of the same NJF_RESNET_W_FLOATS blob */
#define NJF_CHUNK_FLOATS 8192
#define NJF_RESNET_W_FLOATS (NJF_RESNET_CHUNKS * NJF_CHUNK_FLOATS)
#define NJF_RESNET_B_FLOATS (10 * 128 + 32)
#define NJF_COLOR_W_FLOATS NJF_CHUNK_FLOATS
#define NJF_COLOR_B_FLOATS (64 + 32)
/* folded transformer Jacobian head: 14 half-chunks [query | (Mqk, Nov, W1, W2) x 3 | head]; 64 hoisted query channels */
#define NJF_TRANSFORMER_CHUNKS 7
#define NJF_TRANSFORMER_W_FLOATS (NJF_TRANSFORMER_CHUNKS * NJF_CHUNK_FLOATS)
#define NJF_TRANSFORMER_B_FLOATS (3 * 256 + 32)
#define NJF_QDIM 64

/* MFMA precision of the fused MLPs.  A packed blob and the forward call that consumes it must agree. */
#define NJF_PRECISION_F32 0    /* v_mfma_f32_32x32x2_f32: exact fp32 products */
#define NJF_PRECISION_F16X2 1  /* fp32 operands split hi+lo into two fp16; hi*hi + hi*lo + lo*hi accumulated in fp32
                                  by v_mfma_f32_32x32x16_f16: fp32-class accuracy (dropped term 2^-22) at 3/16 the cost */
#define NJF_PRECISION_F16F6 2  /* hi*hi as above; the two correction products hi*lo + lo*hi (2^-11 of the result) in
                                  block-scaled fp6 (e2m3, one power-of-two scale per lane and 32 K-values) by
                                  v_mfma_scale_f32_32x32x64_f8f6f4 at 4x the f16 rate: half the matrix time of F16X2,
                                  ~1.5e-5 relative error per ResnetFC (tools/sim_split_precision.py).  Applies to the
                                  128-wide layers; the narrow layers (lin_out, colour head, transformer head) and
                                  the feature projection keep the F16X2 form */

#define NJF_PRECISION_F16 3    /* PLAIN fp16 products (BASELINE config 5: "fp16 MFMA fused-MLP"): weights packed once as single
                                  fp16, layer inputs rounded to fp16 behind the ReLU, v_mfma_f32_32x32x16_f16 with fp32
                                  accumulation and fp32 biases / residuals -- no hi/lo split, no correction products (issue
                                  factor 1).  A REDUCED-precision mode with its own stated tolerance (every matrix operand is
                                  rounded to 11 significant bits: ~1e-3 norm-wise per network output),
                                  never the default.  Differences at the boundary: (a) the hoisted map such a network reads is
                                  a map of HALVES -- njf_project_features* / njf_project_pyramid with this precision write
                                  `out` as _Float16 [B, Hf*Wf, N] (the projection itself stays error-compensated, its fp32
                                  result is rounded once), NjfFeatureMap.data points to halves and NjfFeatureMap.stride / the
                                  gmap offsets count halves (multiples of 8); (b) a whole 128 x 128 layer is one weight chunk:
                                  the packed ResnetFC keeps its NJF_RESNET_W_FLOATS extent and fills the first
                                  NJF_RESNET_CHUNKS_F16 chunk slots; (c) inference only: the training forwards (activation
                                  dumps) return the "unknown mode" error; (d) never part of a MIXED code */

/* njf_render_forward / njf_points_forward: density + colour networks in precision `d`, Jacobian head in `j` (both one of
 * F32 / F16X2 / F16F6; mixed forms exist for the two split precisions).  A plain NJF_PRECISION_* value means d = j, and is the only code of
 * d = j: NJF_PRECISION_MIXED(d, d) returns the "unknown mode" error like every other code outside the six accepted ones. */
#define NJF_PRECISION_MIXED(d, j) ((d) | (((j) + 1) << 4))

#define NJF_JACOBIAN_NONE 0
#define NJF_JACOBIAN_MLP 1          /* ActionDecoderJacobianMLP (action_decoder_jacobian.py:261-337) */
#define NJF_JACOBIAN_TRANSFORMER 2  /* ActionDecoderJacobianTransformer (:340-446), host-folded, see decoder.py */

/* Reference-layout tensors of one ResnetFC (model_components/resnet_fc.py:82-128), all device fp32. */
typedef struct NjfResnetFcWeights {
  const float* lin_in_w;    /* [128, 63]  */
  const float* lin_in_b;    /* [128]      */
  const float* fc0_w[5];    /* blocks.i.fc_0.weight [128,128] */
  const float* fc0_b[5];    /* [128] */
  const float* fc1_w[5];    /* blocks.i.fc_1.weight [128,128] */
  const float* fc1_b[5];
  const float* lin_z_w[3];  /* lin_z.i.weight [128, 512] */
  const float* lin_z_b[3];  /* [128] */
  const float* lin_out_w;   /* [d_out, 128] */
  const float* lin_out_b;   /* [d_out] */
  int d_out;                /* 1 (proposal), 16 (density+15 features), 3*A (Jacobian) ; <= 32 */
} NjfResnetFcWeights;

/* color_head of ActionDecoderJacobian* (models/decoder/action_decoder_jacobian.py:315-322). */
typedef struct NjfColorHeadWeights {
  const float* w0; const float* b0;   /* [64, 31], [64]  (15 geometry features ++ 16 SH) */
  const float* w1; const float* b1;   /* [64, 64], [64] */
  const float* w2; const float* b2;   /* [3, 64],  [3]  */
} NjfColorHeadWeights;

/* Cameras + scene bounds shared by the fused kernels.  Inverses are taken by the caller
 * (torch.linalg.inv on device), mirroring transform_world2cam (rendering/geometry.py:59-65). */
typedef struct NjfCameras {
  const float* ctxt_w2c;     /* [B,4,4] inverse of the context cam2world */
  const float* ctxt_k;       /* [B,3,3] normalised context intrinsics */
  const float* trgt_w2c;     /* [B,4,4] inverse of the target cam2world (may be NULL when no flow is rendered) */
  const float* trgt_k;       /* [B,3,3] target intrinsics in pixels */
  const float* z_near;       /* [B] */
  const float* z_far;        /* [B] */
  const float* action;       /* [B,A] robot command (may be NULL -> flow outputs are skipped) */
  int batch;                 /* B */
  int action_dim;            /* A <= NJF_MAX_ACTION_DIM */
} NjfCameras;

/* Hoisted, channels-last feature map: G[b][y][x][c] = lin_z(F)[c] (see njf_project_features). */
typedef struct NjfFeatureMap {
  const float* data;   /* [B, Hf, Wf, stride] */
  int height, width;   /* Hf, Wf */
  int stride;          /* floats per texel (>= offset + NJF_ZDIM) */
} NjfFeatureMap;

/* ---- library info ------------------------------------------------------------------------ */
int njf_abi_version(void);
/* Rays one workgroup of the fused ray kernels renders (one per wave): NjfRenderOutputs.frame_partials has
 * ceil(B*R / njf_rays_per_workgroup()) rows. */
int njf_rays_per_workgroup(void);
const char* njf_error_string(int code);

/* ---- camera matrices -------------------------------------------------------------------------- */
/* out[i] = inverse(matrices[i]) for `count` row-major 4x4 fp32 matrices (Gauss-Jordan with partial pivoting evaluated
 * in float64 and rounded once, one thread per matrix).  Replaces torch.inverse on camera extrinsics (transform_world2cam, rendering/geometry.py:59-65;
 * project_world_coords_to_camera, :206-215), which PyTorch-ROCm runs as six rocSOLVER launches per call. */
int njf_invert_4x4(const float* matrices, int count, float* out, void* stream);

/* ---- weight packing (one-off per weight update) -------------------------------------------- */
/* Packs one ResnetFC into `w_out` [NJF_RESNET_W_FLOATS] / `b_out` [NJF_RESNET_B_FLOATS] and its
 * three lin_z layers into `wz_out` [512,384] (k-major) / `bz_out` [384] (inputs of
 * njf_project_features).  Replaces nothing in the reference: it is the layout change that lets
 * ResnetFC.forward (resnet_fc.py:130-154) run as one fused kernel.  NJF_PRECISION_F16: `wz_out` / `bz_out` are REQUIRED -- the
 * biases of blocks 0 and 1's fc_1 are folded into `bz_out` (the latent of the next block is added right behind them and a
 * bilinear footprint's weights sum to 1), so the weight blob and the lin_z pack of one network always come from the same call. */
int njf_pack_resnetfc(const NjfResnetFcWeights* src, float* w_out, float* b_out, float* wz_out, float* bz_out,
                      int precision, void* stream);
/* Same, writing lin_z into a wider [512, wz_ld] matrix (several nets side by side: pass wz_out + column offset). */
int njf_pack_resnetfc_ld(const NjfResnetFcWeights* src, float* w_out, float* b_out, float* wz_out, int wz_ld,
                         float* bz_out, int precision, void* stream);
int njf_pack_color_head(const NjfColorHeadWeights* src, float* w_out, float* b_out, int precision, void* stream);
/* One torch.nn.Linear [d_out, d_in] -> fragment-major block of ceil(d_in/32)*4*ceil(d_out/32)*256 floats
 * (+ zero-padded bias of 32*ceil(d_out/32) floats when b_out != NULL).  kind 0: plain.  kind 1: the input is
 * the 63-d positional encoding (slot order [sin 30 | x | y || cos 30 | z | 1], bias folded into slot 63). */
int njf_pack_linear(const float* w, const float* b, int d_out, int d_in, int kind, float* w_out, float* b_out,
                    int precision, void* stream);

/* ---- per-image feature projection ("lin_z hoist") ------------------------------------------ */
/* G[b,p,n] = sum_k F[b,k,p] * wz[k,n] + bz[n];  F is the encoder output [B,512,Hf,Wf] (NCHW),
 * wz [512,N] (k-major, as written by njf_pack_resnetfc*), bz [N], out [B, Hf*Wf, N].  Because bilinear interpolation is linear with weights
 * summing to 1, lin_z(grid_sample(F)) == grid_sample(G): this moves resnet_fc.py:138-141's
 * 3 x (512->128) GEMMs from per-point to per-texel.  `precision` selects the MFMA path as in the fused kernels
 * (operands stay fp32 in memory; NJF_PRECISION_F16X2 splits them on the fly). */
int njf_project_features(const float* feats, const float* wz, const float* bz, int batch, int hw, int n,
                         float* out, int precision, void* stream);
int njf_project_features_ld(const float* feats, const float* wz, int wz_ld, const float* bz, int batch, int hw, int n,
                            float* out, int precision, void* stream);

/* ---- feature-pyramid producer: encoder_resnet.py:78-86 fused with the lin_z hoist ----------- */
/* The encoder output is cat_l(bilinear_upsample(latent_l)) (align_corners=False) of its conv1 / layer1..3 latents.
 * Given the latents themselves (NCHW, level 0 at the output resolution, channel counts summing to 512 in
 * concatenation order) this computes the same hoisted map G = F . wz + bz without ever forming F: every level is
 * projected at its own resolution, the coarser ones are bilinearly up-sampled and added.  `workspace` (caller-owned)
 * holds the projected coarser levels: sum over l >= 1 of batch * height_l * width_l * n floats.  NJF_PRECISION_F16 with more
 * than one level: the sum is formed in fp32 and rounded once into `out` (halves); the workspace then holds the fp32 level-0
 * map IN FRONT of the coarser levels (batch * height_0 * width_0 * n more floats). */
typedef struct NjfPyramidLevel {
  const float* feats; /* [B, channels, height, width] */
  int channels;       /* multiple of 16 */
  int height, width;
} NjfPyramidLevel;
int njf_project_pyramid(const NjfPyramidLevel* levels, int num_levels, const float* wz, int wz_ld, const float* bz,
                        int batch, int n, float* out, float* workspace, int precision, void* stream);

/* The encoder output itself, channels-last: out [B*H_0*W_0, sum C_l] = cat_l(upsample_l(latent_l)) per texel
 * (models/encoder/encoder_resnet.py:78-86: F.interpolate(bilinear, align_corners=False) to the level-0 resolution +
 * torch.cat) in one pass from the NCHW latents -- the matrix the lin_z weight gradients contract against on the training
 * path (the forward pass never forms it, see njf_project_pyramid).  C_l % 4 == 0. */
int njf_upsample_concat(const NjfPyramidLevel* levels, int num_levels, int batch, float* out, void* stream);
/* Adjoint of njf_upsample_concat (the encoder tail's backward pass: what autograd runs as slice +
 * upsample_bilinear2d_backward for encoder_resnet.py:78-86).  grad [B*H_0*W_0, sum C_l] channels-last (the gradient
 * w.r.t. the matrix njf_upsample_concat writes) -> levels[l].feats receives the gradient of latent l, [B,C_l,H_l,W_l]
 * NCHW (the `feats` pointers of `levels` are the OUTPUTS here; geometry as for njf_upsample_concat).  Gather form, no
 * atomics: bit-reproducible.  One launch per level. */
int njf_upsample_concat_backward(const float* grad, const NjfPyramidLevel* levels, int num_levels, int batch, void* stream);

/* Channel order of the hoisted map.  Inside every block of `block_channels` channels (128 for a ResnetFC's lin_z layer,
 * 64 for the transformer head's query projection) logical feature f of the layer is stored at position
 * njf_hoisted_channel(f, block_channels, precision) -- the order in which the fused kernels' gather reads it, which
 * follows the MFMA precision (NJF_PRECISION_F32 / _F16X2 / _F16F6 / _F16, not a MIXED code) the network that owns the block
 * is packed for: F32 and F16X2 networks fetch per lane (the two lanes that own a point read adjacent 16-byte pieces), F16
 * networks likewise from a map of halves (8-channel pieces), F16F6 networks per quad of lanes (csrc/njf_device.h:
 * add_hoisted_latent).  The njf_pack_* entry points apply it
 * themselves.  Host function, no GPU work; for callers that write hoisted channels directly (flow_mlp's per-image action
 * bias, the transformer head's folded query weights).  Returns a negative error code for an invalid argument. */
int njf_hoisted_channel(int feature, int block_channels, int precision);

/* ---- ray generation: rendering/geometry.py:117-134 + :170-203 ------------------------------ */
/* coords [B,R,2] normalised pixel centres (NULL -> full H x W grid of get_pixel_coordinates),
 * k_inv [B,3,3] inverse normalised intrinsics, c2w [B,4,4];  outputs origins/directions [B,R,3], z [B,R]. */
int njf_generate_rays(const float* coords, int height, int width, const float* k_inv, const float* c2w,
                      int batch, int rays, float* origins, float* directions, float* z, void* stream);

/* ---- training forward: inputs of one ResnetFC's backward pass (resnet_fc.py:130-154) --------- */
/* Written per point p (P = points of the launch) when passed to a forward entry point; all four pointers must be
 * set.  The backward chain itself runs as library GEMMs on these matrices (host side: training.py). */
typedef struct NjfActivationDump {
  float* act;      /* [11, P, 128] ReLU'd input of fc_0 / fc_1 of block b at 2b / 2b+1, of lin_out at 10 */
  float* pe;       /* [P, 64] positional encoding in slot order [sin 30 | x | y | cos 30 | z | 1] */
  int* foot_idx;   /* [P, 4] texel indices (b*Hf*Wf + y*Wf + x) of the bilinear footprint */
  float* foot_w;   /* [P, 4] bilinear weights (nw, ne, sw, se) */
  unsigned* mask;  /* ABI v17, may be NULL: [11, P, 4] ReLU masks of `act` -- bit i of the 128 bits of (layer, point) says whether
                    * one of that layer input's 128 values is > 0, in an order only njf_resnetfc_backward needs to know (its
                    * `masks` argument): the backward chain reads these 16 bytes per point and layer instead of the 512 of `act` */
  int act_f16;     /* ABI v17: non-zero = `act` addresses [11, P, 128] HALVES (16-bit training storage: the weight-gradient GEMMs
                    * then read fp16 operands with fp32 accumulation; the reference trains on TF32 products) */
} NjfActivationDump;

/* ---- fused proposal pass: ray_samplers.py:497-552 (level loop body) ------------------------ */
/* For every ray: sample `s_in` bins (bins_in: [s_in+1] shared, or [B*R, s_in+1] when
 * bins_per_ray), evaluate DensityDecoderMlp.get_density (density_decoder.py:45-71), get_weights
 * (ray_samplers.py:77-101), weights**anneal (:529), PDFSampler (:351-451) with `u` ([s_out+1]
 * shared or per ray) -> bins_out [B*R, s_out+1].  Optional per-sample outputs (may be NULL):
 * weights_out, density_out [B*R, s_in]; `dump` (NULL for inference) receives the proposal net's activations
 * with P = B*R*s_in. */
int njf_proposal_forward(const float* origins, const float* directions, int rays_per_batch,
                         const NjfCameras* cams, const NjfFeatureMap* gmap, int gmap_offset,
                         const float* w_pack, const float* b_pack,
                         const float* bins_in, int bins_per_ray, int s_in,
                         const float* u, int u_per_ray, int s_out, float anneal,
                         float* bins_out, float* weights_out, float* density_out, const NjfActivationDump* dump,
                         int precision, void* stream);

/* ---- fused final pass: action_decoder_jacobian.py:147-215 + model.py:257-314 --------------- */
typedef struct NjfRenderOutputs {
  float* rgb;             /* [B*R,3]  render_rgb (model.py:257-270) */
  float* depth;           /* [B*R]    render_depth before the tensor-global clip (model.py:276) */
  float* step_minmax;     /* [B*R,2]  per-ray min/max of the sample mid-points (inputs of the clip, model.py:277) */
  float* flow;            /* [B*R,2]  render_optical_flow (model.py:288-314); NULL to skip */
  float* pos;             /* [B*R,3]  sum_s w x            (vis_output.ray_positions); NULL to skip */
  float* pos_warped;      /* [B*R,3]  sum_s w (x + flow)   (vis_output.ray_positions_warped); NULL to skip */
  float* action_features; /* [B*R,3A] sum_s w J            (render_action_features, model.py:281-286); NULL to skip */
  float* weights;         /* [B*R,S]  per-sample weights   (training_output / vis_output); NULL to skip */
  float* density;         /* [B*R,S]  per-sample density; NULL to skip */
  float* color;           /* [B*R,S,3]; NULL to skip */
  float* sample_flow;     /* [B*R,S,3] per-sample 3-D flow; NULL to skip */
  float* jacobian;        /* [B*R,S,3A] per-sample action features (encode_image, model.py:458-495); NULL to skip */
  /* training forward, all NULL for inference (P = B*R*S; layouts as in NjfActivationDump).  jac_pe / foot_idx /
   * foot_w select a training forward and are shared by both modes: with den_act + col_* it is the perception mode
   * (backward of the density net and the colour head), otherwise the action mode (backward of the Jacobian head:
   * jac_act is required for NJF_JACOBIAN_MLP; for NJF_JACOBIAN_TRANSFORMER it is optional and has another shape -- the head's
   * residual stream [4, P, 64] that njf_transformer_backward reads). */
  float* jac_act;         /* [11, P, 128] activations of the Jacobian ResnetFC; transformer head: [4, P, 64] residual stream */
  float* jac_pe;          /* [P, 64] positional encoding (the density and Jacobian nets see the same one) */
  int* foot_idx;          /* [P, 4] */
  float* foot_w;          /* [P, 4] */
  float* den_act;         /* [11, P, 128] activations of the density ResnetFC */
  float* col_in;          /* [P, 32] colour-head input [geo 15 | 1 | sh 16] (action_decoder_jacobian.py:315-322) */
  float* col_act;         /* [2, P, 64] ReLU'd outputs of the colour head's first and second layer */
  /* frame-level reductions folded into the kernel's epilogue (ABI v15; all may be NULL).  frame_partials
   * [ceil(B*R / njf_rays_per_workgroup()), 4]: per workgroup (min_t, max_t, sum (rgb - trgt_rgb)^2, sum (flow - trgt_flow)^2) --
   * the bounds of render_depth's tensor-global clip (model.py:277) and the numerators of the photometric / flow mse
   * (model_wrapper.py:117-163) of this launch's rays, reduced in a fixed order (bit-reproducible); the sums are 0 where
   * the target pointer is NULL.  njf_reduce_frame_partials folds the rows into one 4-vector. */
  float* frame_partials;
  const float* trgt_rgb;  /* [B*R,3] target colours of the rays, or NULL */
  const float* trgt_flow; /* [B*R,2] target optical flow of the rays, or NULL */
  /* ABI v17, training forwards, may be NULL: ReLU masks [11, P, 4] of jac_act / den_act (NjfActivationDump.mask) */
  unsigned* jac_mask;
  unsigned* den_mask;
  int dump_f16;           /* non-zero: jac_act / den_act address halves (NjfActivationDump.act_f16) */
} NjfRenderOutputs;

/* bins [B*R, S+1] are spacing-domain bin edges in [0,1] (output of njf_proposal_forward or a
 * sampler); the kernel maps them to Euclidean t = b*far + (1-b)*near (ray_samplers.py:240-243). */
int njf_render_forward(const float* origins, const float* directions, int rays_per_batch,
                       const NjfCameras* cams, const NjfFeatureMap* gmap, int gmap_offset_density,
                       int gmap_offset_jacobian, int jacobian_kind /* NJF_JACOBIAN_* */,
                       const float* w_density, const float* b_density,
                       const float* w_color, const float* b_color,
                       const float* w_jacobian, const float* b_jacobian,
                       const float* bins, int samples, const NjfRenderOutputs* out, int precision, void* stream);

/* ---- frame-level reductions of a (ray-sharded) render: model.py:277, model_wrapper.py:117-163 ------------------------------ */
/* partials [groups,4] (NjfRenderOutputs.frame_partials) -> out4 = (min, max, sum, sum) over the rows, one workgroup, fixed
 * summation order.  This is the 16-byte record a rank contributes to the one collective of a ray-sharded step. */
int njf_reduce_frame_partials(const float* partials, int groups, float* out4, void* stream);
/* Assemble the frame of a ray-sharded step from the all-gathered per-rank packets.  packets [world, packet_floats]; the
 * packet of rank k holds rgb [B,n_k,3] | depth [B,n_k] | flow [B,n_k,2] of its contiguous ray shard (n_k = R/world rays
 * per batch element, the first R % world ranks one more: parallel.shard_bounds) at float offsets 0, 3*B*cap, 4*B*cap with
 * cap = ceil(R / world), and its njf_reduce_frame_partials record in the last four floats.  Writes frame [B,R,6]
 * (rgb | depth | flow per ray) with depth clipped to the GLOBAL [min, max] (render_depth's clip, model.py:277, which the
 * sharded render defers to this point) and scalars6 = (global min, global max, S_rgb = global sum (rgb - trgt)^2, S_flow =
 * global sum (flow - trgt)^2, S_rgb * rgb_scale, S_flow * flow_scale), ranks folded in rank order: with rgb_scale =
 * 1 / (3 B R) and flow_scale = 0.01 / (2 B R) the last two are the frame's rgb loss and flow loss
 * (model_wrapper.py:119-121,148-160). */
int njf_assemble_frame(const float* packets, int world, int packet_floats, int batch, int rays_per_batch, float rgb_scale,
                       float flow_scale, float* frame, float* scalars6, void* stream);

/* ---- point-list evaluation (arbitrary xyz): density_decoder.py:45-71, model.py:416-456 ----- */
/* xyz [B,N,3] world-space points, dirs [B,N,3] or NULL.  mode 0: proposal net -> density [B*N].
 * mode 1: decoder -> density [B*N], color [B*N,3], flow [B*N,3], jacobian [B*N,3A], geo [B*N,15]
 * (any may be NULL); the Jacobian head is selected by jacobian_kind.  The decoder blobs must be
 * one allocation laid out [density | colour | jacobian] (also for njf_render_forward).
 * `features` (ABI v18, may be NULL; mode 1 with NJF_JACOBIAN_MLP, not NJF_PRECISION_F16): [5, B*N, 128] -- the head's residual
 * stream after each of its five blocks, i.e. ResnetFC.forward(compute_features=True).features (model_components/resnet_fc.py:
 * 141-151) block-major; the 640 hidden "action features" ActionDecoderFlowMlp.compute_flow returns (action_decoder_flow.py:
 * 168-176) are its transpose [B*N, 5, 128]. */
int njf_points_forward(const float* xyz, const float* dirs, int points_per_batch, const NjfCameras* cams,
                       const NjfFeatureMap* gmap, int gmap_offset_density, int gmap_offset_jacobian, int mode,
                       int jacobian_kind /* NJF_JACOBIAN_* */, const float* w_density, const float* b_density, const float* w_color, const float* b_color,
                       const float* w_jacobian, const float* b_jacobian,
                       float* density, float* color, float* flow, float* jacobian, float* geo, float* features, int precision,
                       void* stream);

/* ---- voxel-grid field extraction (additive within ABI v20): the 3-D Jacobian-field point cloud --------------------- */
/* The reference colours point clouds of per-point Jacobians (inference/jacobian_color_map.py:113-160) that it obtains by
 * hand: a dense grid through Model.compute_density (model.py:416-456), then threshold / nonzero / gather.  These entry
 * points generate the grid on the device, cull it in stages and evaluate the decoder on the survivors only.
 *
 * A grid is shared by the B context images of a call.  Node (ix, iy, iz) has the linear index n = (ix*ny + iy)*nz + iz,
 * the coordinate fmaf((float)i_c, step[c], origin[c]) per component c, and -- for batch element b -- the GLOBAL index
 * b*N + n with N = nx*ny*nz; B*N must stay below 2^31 (NJF_E_SHAPE otherwise, as for any dims[c] < 1).
 *
 * A LIST names nodes: `indices` (device int32 global indices; NULL = the identity 0, 1, 2, ...), `count` (device int32,
 * the number of entries; NULL = `capacity`) and `capacity` (host int >= 0: the extent the launch covers and the most
 * entries ever read; with indices == NULL it may not exceed B*N).  The entries used are the first min(*count, capacity);
 * the count is read ON THE DEVICE, so a caller that may not synchronise (graph capture) launches for a capacity and the
 * surplus workgroups leave at once.  Indices outside [0, B*N) are clamped into it.  Every per-entry array below is
 * COMPACT: row i belongs to list entry i. */
typedef struct NjfFieldGrid {
  float origin[3];  /* coordinate of node (0, 0, 0) */
  float step[3];    /* spacing per axis */
  int dims[3];      /* (nx, ny, nz), each >= 1 */
} NjfFieldGrid;

/* xyz [capacity, 3] <- the coordinates of the list's nodes (rows past the entry count are left untouched). */
int njf_field_points(const NjfFieldGrid* grid, int batch, const int* indices, const int* count, int capacity, float* xyz,
                     void* stream);

/* Ordered selection.  Entry i of the list is kept when
 *   (values == NULL || values[i] >= threshold)  and
 *   (cams == NULL   || its node projects inside the context image of its batch element with positive camera depth:
 *                      the camera-space point and the normalised image coordinates (u, v) of the fused kernels' feature
 *                      gather; kept iff z_cam > 0 and 0 <= u <= 1 and 0 <= v <= 1; only ctxt_w2c / ctxt_k are read and
 *                      cams->batch must equal `batch`).
 * At least one of `values` (device fp32 [capacity], compact) and `cams` must be given (NJF_E_NULL).  Writes the GLOBAL
 * indices of the kept entries to out_indices IN INPUT ORDER -- the first out_capacity of them -- and the TRUE number of
 * kept entries to *out_count (device int32; it may exceed out_capacity; out_indices may be NULL when out_capacity == 0).
 * out_indices must not alias indices.  `workspace`: device int32 [ceil(capacity / NJF_FIELD_SELECT_BLOCK)] (at least one
 * element), caller-owned.  Three launches -- per-workgroup counts by ballot + popcount, a one-workgroup exclusive scan, a
 * scatter -- in integer arithmetic without atomics: the output bytes are reproducible. */
#define NJF_FIELD_SELECT_BLOCK 1024
int njf_field_select(const NjfFieldGrid* grid, const NjfCameras* cams, int batch, const float* values, float threshold,
                     const int* indices, const int* count, int capacity, int* out_indices, int* out_count, int out_capacity,
                     int* workspace, void* stream);

/* njf_points_forward on the nodes of a list (the batch is cams->batch): same networks, same weight / bias / map / precision
 * arguments and the same per-point arithmetic -- a node's outputs equal what njf_points_forward returns for its coordinate.
 * mode 0: proposal net -> density [capacity] (required).  mode 1: decoder -> density [capacity], color [capacity, 3],
 * jacobian [capacity, 3A]; with jacobian_kind == NJF_JACOBIAN_NONE and color == NULL only the density network runs (and only
 * its blob is read: w_color / b_color may be NULL); otherwise density / color may be NULL, `jacobian` is required when a head
 * is selected.  view_dir: HOST pointer to the 3 floats of the colour head's constant view direction, used as given (NULL =
 * (0, 0, 1), what Model.compute_density feeds).  cams->action is not read.  Rows past the entry count are left untouched. */
int njf_field_forward(const NjfFieldGrid* grid, const int* indices, const int* count, int capacity, const float* view_dir,
                      const NjfCameras* cams, const NjfFeatureMap* gmap, int gmap_offset_density, int gmap_offset_jacobian,
                      int mode, int jacobian_kind /* NJF_JACOBIAN_* */, const float* w_density, const float* b_density,
                      const float* w_color, const float* b_color, const float* w_jacobian, const float* b_jacobian,
                      float* density, float* color, float* jacobian, int precision, void* stream);

/* ---- isosurface mesh of a scalar on the grid (additive within ABI v20): the 3-D Jacobian-field surface ---------------- */
/* Marching tetrahedra on the Kuhn cut of every cell; the semantics are fixed so the result is
 * checkable against a plain restatement:
 *   inside(g) = values[g] >= threshold (NaN: outside); valid(g) = (valid == NULL || valid[g] != 0) && (cams == NULL || node g
 *   projects inside the context image of its batch element: the predicate of njf_field_select).
 *   Cell (ix, iy, iz) -- (nx-1)(ny-1)(nz-1) = Nc per batch element, local index (ix*(ny-1) + iy)*(nz-1) + iz, global b*Nc +
 *   local -- is cut into six tetrahedra, one per axis order (a, b, c) in the order xyz, xzy, yxz, yzx, zxy, zyx, with the
 *   corners c0 = (0,0,0), c1 = c0 + e_a, c2 = c1 + e_b, c3 = (1,1,1).  Every tetrahedron edge is (lower node) + direction k:
 *   0..6 = (1,0,0) (0,1,0) (0,0,1) (1,1,0) (1,0,1) (0,1,1) (1,1,1); the lower node owns it.
 *   VERTICES: one per edge inside the grid whose ends are both valid and differ in `inside`, in ascending (owner global
 *   index, k).  With end 0 = owner: t = (threshold - v0) / (v1 - v0) (IEEE division), 0.5 if that is not finite, then clamped
 *   to [0, 1]; position fmaf(t, x1 - x0, x0) per component on the node coordinates.
 *   TRIANGLES: cells in ascending global index, tetrahedra in the order above; a tetrahedron with an invalid corner emits
 *   nothing.  With the local corner order c0 < c1 < c2 < c3: one inside corner i (others j < k < l) -> (ij, ik, il); three
 *   inside corners -> the same with i the outside corner; two (i < j inside, k < l outside) -> (ik, il, jl) and (ik, jl, jk).
 *   The geometric normal points from inside to outside: where the listed order would point the other way the LAST TWO
 *   entries of each triangle are swapped -- decided from the case and the parity of the axis order, never from coordinates
 *   (zero-area triangles of t = 0 or 1 do not flip).  Entries are vertex ranks: rank of edge k of node g =
 *   vertex_offset[g] + popcount(edge_mask[g] & ((1 << k) - 1)).
 * `phase`: NJF_FIELD_MESH_COUNT runs the counting launch and the scan (the true count lands in *vertex_count /
 * *triangle_count, device int32), NJF_FIELD_MESH_EMIT the emitting launch of a count made before on the same stream with the
 * same arguments; both bits: all three launches without a host read in between.  Rows of ranks >= the capacity are dropped
 * (the counts stay true; triangles keep true vertex ranks).  edge_mask: device bytes [B*N] (bits 0..6: edge k carries a
 * vertex, bit 7: the node is valid), vertex_offset: device int32 [B*N]; both are written by njf_field_mesh_vertices and read
 * by njf_field_mesh_triangles.  workspace: device int32 [ceil(B*N / NJF_FIELD_MESH_BLOCK)], caller-owned, per call.  Integer
 * arithmetic apart from t and the position, no atomics: the output bytes are reproducible.  NJF_E_VALUE: a dims[c] < 2, a
 * non-finite threshold, a negative capacity, an unknown phase. */
#define NJF_FIELD_MESH_BLOCK 1024
#define NJF_FIELD_MESH_COUNT 1
#define NJF_FIELD_MESH_EMIT 2
/* values fp32 [B*N]; vertex_node int32 / vertex_edge bytes / vertex_t fp32 [max_vertices], vertices fp32 [max_vertices, 3]
 * (may be NULL without NJF_FIELD_MESH_EMIT or with max_vertices == 0: the emitting launch then writes vertex_offset only). */
int njf_field_mesh_vertices(const NjfFieldGrid* grid, const NjfCameras* cams, int batch, const float* values,
                            const unsigned char* valid, float threshold, int phase, unsigned char* edge_mask,
                            int* vertex_offset, int* vertex_node, unsigned char* vertex_edge, float* vertex_t, float* vertices,
                            int max_vertices, int* vertex_count, int* workspace, void* stream);
/* triangles int32 [max_triangles, 3] vertex ranks, triangle_cell int32 [max_triangles] global cell indices. */
int njf_field_mesh_triangles(const NjfFieldGrid* grid, int batch, const float* values, float threshold, int phase,
                             const unsigned char* edge_mask, const int* vertex_offset, int* triangles, int* triangle_cell,
                             int max_triangles, int* triangle_count, int* workspace, void* stream);

/* The decoder (mode 1 of njf_points_forward) at stored positions of a RAGGED batch in one launch: row i is the point
 * xyz[i] of batch element node[i] / nodes_per_batch (node: device int32, clamped into [0, B*nodes_per_batch); for a mesh
 * the owning node of the vertex).  The entry count min(*count, capacity) is read on the device (count NULL = capacity).
 * density [capacity] (may be NULL), color [capacity, 3] (may be NULL with a Jacobian head), jacobian [capacity, 3A] (required
 * with a head).  Every other argument, the per-point arithmetic and the results are those of njf_field_forward /
 * njf_points_forward on that position.  Rows past the entry count are left untouched. */
int njf_field_forward_at(const float* xyz, const int* node, const int* count, int capacity, int nodes_per_batch,
                         const float* view_dir, const NjfCameras* cams, const NjfFeatureMap* gmap, int gmap_offset_density,
                         int gmap_offset_jacobian, int jacobian_kind /* NJF_JACOBIAN_* */, const float* w_density,
                         const float* b_density, const float* w_color, const float* b_color, const float* w_jacobian,
                         const float* b_jacobian, float* density, float* color, float* jacobian, int precision, void* stream);

/* ---- fusion of the fields of several context views (additive within ABI v20): one cloud / mesh per multi-camera scene ---- */
/* The B context images of a call are G = B / V SCENES of V consecutive VIEWS: calibrated cameras that look at one scene in
 * one world frame (the convention of views_per_command in the inverse-dynamics solve), batch element b = g*V + v, on one
 * shared grid.  The per-view global index of node n is (g*V + v)*N + n, the FUSED global index g*N + n; G*V*N must stay below
 * 2^31.  The semantics are fixed so the result is checkable against a plain restatement:
 *   s_v(x) = the frustum predicate of njf_field_select for batch element g*V + v at the point x (cams == NULL: 1).
 *   c = sum_v s_v; a node is VALID iff c >= min_views.
 *   fused density of a valid node from the per-view values d_v --
 *     NJF_FIELD_FUSE_MEAN: acc = 0; for v ascending: if (s_v) acc += d_v (fp32 adds); fused = acc / (float)c (IEEE division);
 *     NJF_FIELD_FUSE_MIN / _MAX: m = d of the first seen view; for every later seen view, ascending: m = (d_v < m) ? d_v : m
 *     (`>` for _MAX).  _MIN carves: a node is occupied only if every view that sees it says so.
 *   An invalid node has fused = 0. */
#define NJF_FIELD_MAX_VIEWS 8
#define NJF_FIELD_FUSE_MEAN 0
#define NJF_FIELD_FUSE_MIN 1
#define NJF_FIELD_FUSE_MAX 2
/* values: device fp32 [G*V*N] (what the density-only pass of njf_field_forward writes for the identity list).  fused: device
 * fp32 [G*N]; seen: device bytes [G*N], bit v = s_v (may be NULL); valid: device bytes [G*N], 0 / 1 (may be NULL; the `valid`
 * argument of njf_field_mesh_vertices on the fused values).  cams: only ctxt_w2c / ctxt_k are read and cams->batch must equal
 * scenes * views (NJF_E_SHAPE; as for an oversize G*V*N).  NJF_E_VALUE: views outside [1, NJF_FIELD_MAX_VIEWS], min_views
 * outside [1, views], an unknown mode.  One launch: a workgroup takes NJF_FIELD_SELECT_BLOCK consecutive nodes of one scene,
 * loads the scene's cameras once and reads every view's values coalesced.  No atomics: the output bytes are a function of the
 * inputs alone. */
int njf_field_fuse(const NjfFieldGrid* grid, const NjfCameras* cams, int scenes, int views, const float* values, int mode,
                   int min_views, float* fused, unsigned char* seen, unsigned char* valid, void* stream);

/* Colour and Jacobian at the positions of a list -- survivor nodes or mesh vertices -- from the decoder's per-view outputs.
 * Entry i is the point xyz[i] of scene node[i] / nodes_per_scene (node: device int32 FUSED global index, clamped into the
 * scenes; for a mesh the owning node of the vertex); the entry count min(*count, capacity) is read on the device (count
 * NULL = capacity).  Per-view rows are ENTRY-MAJOR, row i*views + v: density [capacity*views], color [capacity*views, 3],
 * jacobian [capacity*views, 3*action_dim] -- what njf_field_forward / njf_field_forward_at write for the expanded list.
 *   w_v = s_v(x) ? d_v(x) : 0;  W = sum_v w_v (fp32 adds, v ascending);  if (!(W > 0)): every w_v = 1 and W = (float)views
 *   (no view sees a vertex between two nodes seen by different views, or every density is zero);
 *   out = acc / W with acc = 0; for v ascending: acc = fmaf(w_v, x_v, acc), per output component.
 * out_color [capacity, 3] (required with color), out_jacobian [capacity, 3*action_dim] (required with jacobian), out_views:
 * device bytes [capacity], bit v = s_v(x) (may be NULL).  color and / or jacobian may be NULL; with both NULL density may be
 * NULL too and out_views alone is written.  cams == NULL: every s_v = 1; else only ctxt_w2c / ctxt_k are read and cams->batch
 * must be a multiple of views (NJF_E_SHAPE).  NJF_E_VALUE: views outside [1, NJF_FIELD_MAX_VIEWS], nodes_per_scene < 1;
 * NJF_E_ACTION_DIM: a jacobian with action_dim outside [1, NJF_MAX_ACTION_DIM].  Rows past the entry count are left
 * untouched.  One launch, no atomics: the output bytes are a function of the inputs alone. */
int njf_field_combine(const float* xyz, const int* node, const int* count, int capacity, int nodes_per_scene, int views,
                      const NjfCameras* cams, const float* density, const float* color, const float* jacobian, int action_dim,
                      float* out_color, float* out_jacobian, unsigned char* out_views, void* stream);

/* ---- connected components of the inside nodes (additive within ABI v20): drop floaters, split a body by key -------------- */
/* The semantics are fixed so the result is checkable against a plain restatement:
 *   DENSE form (values != NULL, indices == NULL): node g is INSIDE iff (valid == NULL || valid[g] != 0) && (cams == NULL ||
 *   it projects inside the context image of its batch element: the predicate of njf_field_select) && values[g] >= threshold
 *   (NaN: outside).  LIST form (indices != NULL, values == valid == cams == NULL): the inside nodes are the first
 *   min(*count, capacity) entries of `indices`, ASCENDING global indices (count NULL = capacity; rows past the count are
 *   never read; entries out of order or outside [0, B*N) are dropped).
 *   Two inside nodes of one batch element are ADJACENT iff they differ by one of the first connectivity/2 directions of the
 *   mesh table -- 6: (1,0,0) (0,1,0) (0,0,1); 14: those and (1,1,0) (1,0,1) (0,1,1) (1,1,1), the edges of the Kuhn tetrahedra
 *   -- in either sign, without wrap at the grid faces, and -- with keys -- iff their keys are equal as well.
 *   labels[g] = the smallest global index of g's component, -1 outside; sizes[g] = the node count of that component, 0
 *   outside; *component_count = the number of components (of nodes with labels[g] == g).
 * keys: device int32, [B*N] in the dense form, [capacity] (per entry) in the list form, or NULL.  labels, sizes: device int32
 * [B*N]; component_count, status: device int32 [1].  workspace: device int32 [2*B*N] (parents, per-root sizes), [3*B*N] in the
 * list form with keys (the per-entry keys are scattered to a dense array).  *status: 0, or NJF_FIELD_COMPONENTS_E_* bits when a
 * find / union loop of the lock-free union-find passed its iteration cap (a broken invariant -- the results are then
 * unspecified, nothing hangs).  Four launches over workgroups of NJF_FIELD_COMPONENTS_BLOCK nodes behind two 4-byte memsets:
 * a fixed sequence without a host read.  Integer arithmetic; the atomics are integer min / add / or, so the output bytes are a
 * function of the inputs alone.  `phase`: NJF_FIELD_COMPONENTS_ALL; the single bits run one launch each, so that a caller can
 * time them apart -- the results are defined once all four have run in order, on one stream, with the same arguments and
 * workspace.  NJF_E_VALUE: connectivity not 6 or 14, an unknown phase, both forms at once, valid / cams with a list;
 * NJF_E_NULL: neither form, a missing output; NJF_E_SHAPE: as for njf_field_select. */
#define NJF_FIELD_COMPONENTS_BLOCK 1024
#define NJF_FIELD_COMPONENTS_INIT 1   /* the memsets, inside flags, in-workgroup unions */
#define NJF_FIELD_COMPONENTS_MERGE 2  /* unions across workgroups */
#define NJF_FIELD_COMPONENTS_LABEL 4  /* labels, per-root sizes, the component count */
#define NJF_FIELD_COMPONENTS_SIZES 8  /* sizes */
#define NJF_FIELD_COMPONENTS_ALL 15
#define NJF_FIELD_COMPONENTS_E_LOCAL 1  /* an in-workgroup (LDS) loop */
#define NJF_FIELD_COMPONENTS_E_FIND 2   /* a find over the global parents */
#define NJF_FIELD_COMPONENTS_E_UNION 4  /* the retries of a global union */
int njf_field_components(const NjfFieldGrid* grid, const NjfCameras* cams, int batch, const float* values, float threshold,
                         const unsigned char* valid, const int* indices, const int* count, int capacity, const int* keys,
                         int connectivity, int phase, int* labels, int* sizes, int* component_count, int* status,
                         int* workspace, void* stream);

/* ---- coarse-to-fine band (additive within ABI v20): the fine density pass only near the surface ------------------------- */
/* The semantics are fixed so the result is checkable against a plain restatement.  `grid` is the FINE
 * grid; factor k in {2, 4, 8, 16}; every axis needs (n_c - 1) % k == 0 and n_c >= k + 1; m_c = (n_c - 1) / k.  The COARSE
 * grid has the origin of the fine one, the step k*step (exact: k is a power of two) and the dims (m_x+1, m_y+1, m_z+1), so
 * coarse node j IS fine node k*j; M = prod(m_c + 1) coarse nodes and Nb = prod(m_c) BLOCKS per batch element, block (jx, jy,
 * jz) with 0 <= j_c < m_c at the local index (jx*m_y + jy)*m_z + jz.
 *   hit(b, q) = (coarse_valid == NULL || coarse_valid[b*M + q] != 0) && coarse_values[b*M + q] >= coarse_threshold
 *   (NaN: no hit; a value equal to the threshold: a hit).
 *   block_active(b, j) iff some coarse node q with max(0, j_c - dilate) <= q_c <= min(m_c, j_c + 1 + dilate) on every axis is
 *   a hit (dilate 0: the block's own eight corners).
 *   Fine node (ix, iy, iz) of element b is in the BAND iff some active block j of b has j_c*k <= i_c <= (j_c + 1)*k on every
 *   axis (block faces are shared: a node belongs to up to eight blocks).  Nothing crosses batch elements.
 * coarse_values: device fp32 [batch*M]; coarse_valid: device bytes [batch*M] or NULL; block_active: device bytes [batch*Nb],
 * 0 / 1; band: device bytes [batch*N], 0 / 1; out_indices: the ASCENDING global indices of the band nodes -- the first
 * out_capacity of them (may be NULL when out_capacity == 0); *out_count (device int32): the TRUE number of band nodes.
 * workspace: device int32 [ceil(batch*N / NJF_FIELD_BAND_BLOCK)], caller-owned.  Four launches (blocks; band bytes + counts;
 * the scan of njf_field_select; the scatter) in integer arithmetic without atomics: the output bytes are reproducible.
 * NJF_E_VALUE: a factor not in the set, dims not 1 mod k or below k + 1, dilate outside [0, 2], a non-finite threshold;
 * NJF_E_NULL: a missing pointer; NJF_E_SHAPE: as for njf_field_select.  Every check precedes the first launch. */
#define NJF_FIELD_BAND_BLOCK 1024
int njf_field_band(const NjfFieldGrid* grid, int factor, int dilate, int batch, const float* coarse_values,
                   const unsigned char* coarse_valid, float coarse_threshold, unsigned char* block_active, unsigned char* band,
                   int* out_indices, int* out_count, int out_capacity, int* workspace, void* stream);

/* out[indices[i]] = values[i] for i < min(*count, capacity) (count: device int32, NULL = capacity; it is read on the device,
 * workgroups past it leave and rows past it are never read).  values: device fp32 [capacity], indices: device int32
 * [capacity], out: device fp32 [out_size]; an index outside [0, out_size) is skipped.  Indices that repeat give an
 * unspecified winner (the lists of this library do not repeat).  One launch. */
int njf_field_scatter(const float* values, const int* indices, const int* count, int capacity, float* out, int out_size,
                      void* stream);

/* *leaks (device int32) = the number of entries g of the list (`indices`: ascending global indices of INSIDE nodes, the
 * first min(*count, capacity); count NULL = capacity; entries outside [0, batch*N) are dropped) that have a neighbour g +- one
 * of the seven mesh directions, inside the grid and the same batch element (no wrap at the faces, as for
 * njf_field_components), whose band byte is 0.  0 proves that every connected component the band touches lies wholly in it
 * with all of its surface edges.  A 4-byte memset and one launch; one integer atomic add per
 * workgroup, so the result does not depend on scheduling. */
int njf_field_band_leaks(const NjfFieldGrid* grid, int batch, const unsigned char* band, const int* indices, const int* count,
                         int capacity, int* leaks, void* stream);

/* ---- rigid twists of the parts of an extracted field (ABI v20, additive) --------------------------------
 * For each part (the rows of one label) and command channel a, the least-squares rigid field J_a(x) = v_a + omega_a x (x - c)
 * of the rows' Jacobians: a screw axis per part and channel.
 * Inputs, all on the device: xyz [n,3] and jacobian [n,A,3] fp32, labels [n] int32 (a negative label belongs to no part),
 * weights [n] fp32 or NULL (w_i = weights[i] > 0 ? weights[i] : 0, so NaN and negatives count as 0; NULL: w_i = 1), count
 * (int32, NULL = n: rows from min(*count, n) on are never read), parts [K] int32 (ascending, distinct, non-negative) and
 * parts_count (int32, NULL = K: the true number of parts; it may exceed K, then the first K are fitted).  Row i belongs to
 * slot p iff i < *count, p < min(*parts_count, K) and labels[i] == parts[p].  A row with w_i == 0 counts in nodes[p] but its
 * xyz and jacobian enter no sum (a NaN there is harmless).
 * All arithmetic is in DOUBLE on the fp32 inputs converted exactly, in the order written, without contraction:
 *   pass A  nodes, W = sum w, S = sum w*x;  c = S / W
 *   pass B  r = x - c:  Q_ab = sum w*(r_a*r_b) stored (xx, xy, xz, yy, yz, zz);  per channel P = sum w*J,
 *           L = sum w*(r x J) with r x J = (ry*Jz - rz*Jy, rz*Jx - rx*Jz, rx*Jy - ry*Jx),  E = sum w*((Jx*Jx + Jy*Jy) + Jz*Jz)
 *   solve   M = tr(Q) I - Q, Cholesky in the order x, y, z; a pivot <= 1e-9 * tr(M) makes the part TRANSLATION-ONLY (omega = 0,
 *           status bit NJF_FIELD_TWISTS_TRANSLATION: one node, collinear nodes; a planar part is not degenerate -- beyond a
 *           condition number of about 1e9 fp32 Jacobians do not determine omega); else omega_a = M^-1 L_a.  v_a = P_a / W is
 *           the velocity at the centroid (with centred coordinates the two blocks of the 6x6 normal equations decouple).
 *           W == 0 or no rows: status bit NJF_FIELD_TWISTS_EMPTY and every floating-point output of the slot is 0.
 *   pass C  residual[p][a] = sum w*|J_a - (v_a + omega_a x r)|^2, summed directly (the closed form E - W|v|^2 - omega.L cancels
 *           to noise for a near-rigid part), and row_residual [n] fp32 = sum_a |J_a - model|^2, unweighted, rounded once from
 *           double; 0 for the rows of no fitted part (a memset, then every row is written by the one workgroup that owns it).
 * Outputs: out_labels [K] int32 (parts[p]; -1 for the slots >= min(*parts_count, K), whose other outputs are 0), out_count
 * (int32: *parts_count), nodes [K] and status [K] int32; double weight [K], centroid [K,3], omega, velocity [K,A,3], energy,
 * residual [K,A] and the raw sums q [K,6], p, l [K,A,3].
 * No floating-point atomics: NJF_FIELD_TWISTS_CHUNK consecutive rows per chunk, workgroup (chunk, part) compacts the matching
 * rows in order, thread t adds list entries t, t + 256, ... sequentially, then a fixed butterfly over the wave, the four wave
 * partials in wave order and, in a finishing launch, the chunks in ascending order: every sum has an order that depends on
 * (n, K, A) alone, two calls give equal bytes.  workspace: NJF_FIELD_TWISTS_STRIDE(A) * K * ceil(n / NJF_FIELD_TWISTS_CHUNK)
 * doubles of the caller's (workspace_doubles says how many it holds).  One memset and six launches on `stream`, no host read
 * (capture-safe); `phases` = NJF_FIELD_TWISTS_ALL, or a subset to time the launches apart (each reads what the earlier ones
 * left).  Returns, before the first launch: NJF_E_VALUE for A outside [1, NJF_MAX_ACTION_DIM], K outside
 * [1, NJF_FIELD_TWISTS_MAX_PARTS] or unknown phases; NJF_E_SHAPE for n < 0, a workspace that is too small, or K * chunks *
 * stride past 2^31 - 1; NJF_E_NULL for a missing pointer. */
#define NJF_FIELD_TWISTS_CHUNK 4096
#define NJF_FIELD_TWISTS_MAX_PARTS 256
#define NJF_FIELD_TWISTS_STRIDE(A) (6 + 7 * (A))
#define NJF_FIELD_TWISTS_EMPTY 1        /* status bits */
#define NJF_FIELD_TWISTS_TRANSLATION 2
#define NJF_FIELD_TWISTS_CLEAR 1        /* phases: the memset of row_residual, then one launch each */
#define NJF_FIELD_TWISTS_SUMS 2
#define NJF_FIELD_TWISTS_CENTROID 4
#define NJF_FIELD_TWISTS_MOMENTS 8
#define NJF_FIELD_TWISTS_SOLVE 16
#define NJF_FIELD_TWISTS_RESIDUAL 32
#define NJF_FIELD_TWISTS_RESIDUAL_SUM 64
#define NJF_FIELD_TWISTS_ALL 127
int njf_field_twists(const float* xyz, const float* jacobian, const int* labels, const float* weights, const int* count, int n,
                     int action_dim, const int* parts, const int* parts_count, int num_parts, int* out_labels, int* out_count,
                     int* nodes, int* status, double* weight, double* centroid, double* omega, double* velocity,
                     double* energy, double* residual, double* q, double* p, double* l, float* row_residual,
                     double* workspace, long long workspace_doubles, int phases, void* stream);

/* ---- joints between the parts of an extracted field (ABI v20, additive) ---------------------------------
 * Which parts touch on the grid, where, and how one moves relative to the other under each command channel: the relative twist
 * of two parts in contact is the joint, its screw axis the hinge.
 * Inputs, all on the device: grid and batch B (N = nx*ny*nz, B*N < 2^31); the list of a cloud -- indices [n] int32, ascending
 * global indices, and count (int32, NULL = n: rows from min(*count, n) on are never read; an index outside [0, B*N) is
 * dropped) --; labels [n] int32 per row (negative: no part); the part list and twists of njf_field_twists: parts [K] (ascending
 * in the used slots), parts_count (int32, NULL = K: the true number, it may exceed K), part_status [K], double centroid [K,3],
 * omega, velocity [K,A,3]; connectivity 6 or 14 (the direction table of njf_field_components); min_contacts >= 1; max_joints J.
 * SLOTS  row i has slot p iff i < *count, p < min(*parts_count, K) and labels[i] == parts[p] (the rule of njf_field_twists);
 *        every other row has none.
 * CONTACTS  for every row with slot p at node g = (b, ix, iy, iz) and every direction d among the FIRST connectivity/2 of the
 *        table -- the positive sense only, so each unordered node pair is seen once --, the neighbour g' = g + d must lie inside
 *        the grid (no wrap at the faces, nothing crosses batch elements) and be a list row with slot q != p.  Then, with lo =
 *        min(p, q), hi = max(p, q): contacts[lo][hi] += 1 and sum2[lo][hi][c] += i_c + i'_c for c = x, y, z, in 64-bit
 *        integers: sum2 is twice the contact midpoint in node units, exact, whatever the order of the adds.
 * LIST   the pairs with contacts >= min_contacts in ascending (lo, hi); the first J are stored and *out_count is their true
 *        number.  part_a, part_b [J] int32 = lo, hi; contacts [J] int64; status [J] int32 = part_status[lo] | part_status[hi].
 *        Unused rows hold -1 in part_a and part_b and 0 elsewhere.
 * TWISTS anchor [J,3] double, per component m = (double)sum2_c / (2.0 * (double)contacts), x_c = (double)origin_c +
 *        (double)step_c * m (a multiply, then an add).  Per joint and channel a, all in double in this order, s = lo, hi:
 *        r_s = x - c_s;  u_s = v_{s,a} + cross(omega_{s,a}, r_s) with cross(w, r) = (wy*rz - wz*ry, wz*rx - wx*rz, wx*ry - wy*rx);
 *        out_omega [J,A,3] = omega_hi - omega_lo;  out_velocity [J,A,3] = u_hi - u_lo.  No sum runs over rows.
 * workspace: NJF_FIELD_JOINTS_WORKSPACE(B*N, K) 64-bit words of the caller's (workspace_words says how many it holds): the table
 * [K][K][4] (contacts, sum2), then the dense int32 slot volume [B*N] (-1: no slot).  Two memsets and four launches on `stream`,
 * no host read (capture-safe); the only atomics are 64-bit integer adds.  `phases` = NJF_FIELD_JOINTS_ALL, or a subset to time
 * the launches apart (each reads what the earlier ones left); with NJF_FIELD_JOINTS_PER_LANE the contacts launch runs in its
 * per-lane form -- every lane adds for itself instead of the wave combining equal pairs first: the same table, kept to be
 * measured against.  Returns, before the first launch: NJF_E_VALUE for a connectivity not 6 or 14, K outside
 * [1, NJF_FIELD_TWISTS_MAX_PARTS], A outside [1, NJF_MAX_ACTION_DIM], J outside [1, NJF_FIELD_JOINTS_MAX], min_contacts < 1 or
 * unknown phases; NJF_E_SHAPE for n < 0, batch < 1, B*N >= 2^31 or a workspace that is too small; NJF_E_NULL for a missing
 * pointer (indices and labels may be NULL when n == 0). */
#define NJF_FIELD_JOINTS_MAX 4096
#define NJF_FIELD_JOINTS_TABLE_WORDS(K) (4LL * (K) * (K))
#define NJF_FIELD_JOINTS_WORKSPACE(total, K) (NJF_FIELD_JOINTS_TABLE_WORDS(K) + ((long long)(total) + 1) / 2)
#define NJF_FIELD_JOINTS_CLEAR 1        /* phases: the two memsets, then one launch each */
#define NJF_FIELD_JOINTS_SLOTS 2
#define NJF_FIELD_JOINTS_CONTACTS 4
#define NJF_FIELD_JOINTS_LIST 8
#define NJF_FIELD_JOINTS_TWISTS 16
#define NJF_FIELD_JOINTS_ALL 31
#define NJF_FIELD_JOINTS_PER_LANE 32    /* modifier of _CONTACTS, not part of _ALL */
int njf_field_joints(const NjfFieldGrid* grid, int batch, const int* indices, const int* labels, const int* count, int n,
                     const int* parts, const int* parts_count, int num_parts, const int* part_status, const double* centroid,
                     const double* omega, const double* velocity, int action_dim, int connectivity, int min_contacts,
                     int max_joints, int* part_a, int* part_b, long long* contacts, int* status, int* out_count, double* anchor,
                     double* out_omega, double* out_velocity, long long* workspace, long long workspace_words, int phases,
                     void* stream);

/* ---- posing the parts under a command: twist exponentials along the tree (ABI v20, additive) --------------
 * Where every part, and every labelled point, goes under each of M commands: the finite rigid motion of a part is the product
 * of the exponentials of the joint twists along its chain to the root, the space-frame product of exponentials.
 * Inputs, all on the device: the part list and twists of njf_field_twists -- parts [K], parts_count (int32, NULL = K), part_status
 * [K], double centroid [K,3], omega, velocity [K,A,3]; used slots are p < Ku = min(*parts_count, K) --; optionally the joints of
 * njf_field_joints -- part_a, part_b [J], joints_count (int32, NULL = J; stored joints are j < Ju = min(*joints_count, J)),
 * double anchor [J,3], joint_omega, joint_velocity [J,A,3] -- WITH a tree parent, joint_of [K] int32 (all of them or none;
 * joints_count alone may be NULL); commands [M,A] float, converted exactly to double.
 * LINK   G[m,p] = (R, t), x -> R x + t, in double.  With u = commands[m]: w = sum_a u_a omega_a, v = sum_a u_a v_a in ascending
 *        a from 0.0, of the slot's own twist about c = centroid[p] (no tree, or parent[p] < 0) or, with q = parent[p] >= 0 and
 *        j = joint_of[p], of joint j's relative twist about c = anchor[j], times +1 when part_a[j] == q and -1 when part_b[j]
 *        == q.  th2 = (wx*wx + wy*wy) + wz*wz.  th2 <= 1e-6: a = (1 - th2/6) + th4/120, b = (1/2 - th2/24) + th4/720, g = (1/6 -
 *        th2/120) + th4/5040; otherwise th = sqrt(th2), a = sin(th)/th, b = 2 sin(th/2)^2 / th2, g = (th - sin(th)) / (th2 th).
 *        R = I + a [w]x + b [w]x^2, V = I + b [w]x + g [w]x^2, [w]x^2 = w w^T - th2 I, t = (c - R c) + V v.
 * LINK BITS  1: p >= Ku or part_status[p] & 1.  2 (bad link): parent[p] >= 0 and (q >= Ku, or q == p, or j outside [0, Ju), or
 *        {part_a[j], part_b[j]} != {p, q}).  A slot with a bit set has G = identity.
 * POSE   T = G[m,p], q = parent[p]; while q != -1: T <- G[m,q] o T (R = R_q R_T, t = (R_q t_T) + t_q, sums of three products in
 *        ascending index), q = parent[q].  The identity, with status bit 2, when p or a slot on the walk is a bad link, when
 *        the walk would take more than K steps (a cycle) or meets a q outside [-1, K).  rotation [M,K,3,3], translation [M,K,3]
 *        double; status [K] int32 = the link bits | that bit; depth [K] int32 = the steps taken (neither depends on m).
 * POINTS (xyz != NULL and n > 0): xyz [n,3] float, labels [n] int32, count (int32, NULL = n), jacobian [n,A,3] float or NULL,
 *        posed [M,n,3] float.  Row i < min(*count, n) has slot p iff labels[i] >= 0, p < Ku and labels[i] == parts[p] (parts
 *        ascending in the used slots).  With a slot of status 0: x'_c = (float)(((R_c0 x + R_c1 y) + R_c2 z) + t_c) in double.
 *        Otherwise, with a jacobian: x'_c = (float)(x_c + u_0 J_0c + u_1 J_1c + ...), in double, one add per term in ascending a;
 *        without: x' = x.  Rows from min(*count, n) on are neither read nor written.  Offsets are 64-bit.
 * workspace: NJF_FIELD_POSE_WORKSPACE(M, K) doubles of the caller's: G [M][K][12], then the int32 link bits [K].  Three launches
 * on `stream`, no atomics, no host read (capture-safe).  `phases` = NJF_FIELD_POSE_ALL or a subset, to time the launches apart
 * (each reads what the earlier ones left); two modifiers select the other forms of the points launch, which give the same
 * bytes and are kept to be measured against: NJF_FIELD_POSE_STAGED copies one command's transforms of the used slots into LDS
 * instead of reading them per lane from L2, NJF_FIELD_POSE_WIDE lays a workgroup's output out in LDS and writes 16-byte
 * stores instead of three dwords per lane.  Returns, before the first launch: NJF_E_VALUE for K outside [1,
 * NJF_FIELD_TWISTS_MAX_PARTS], A outside [1, NJF_MAX_ACTION_DIM], M outside [1, NJF_FIELD_POSE_MAX_COMMANDS], with joints J
 * outside [1, NJF_FIELD_JOINTS_MAX], or unknown phases; NJF_E_SHAPE for n < 0 or a workspace that is too small; NJF_E_NULL for
 * a missing pointer, joints without a tree or a tree without joints, or points without xyz, labels or posed.  Only the links
 * launch reads part_status and the twists, only the links and chain launches the workspace: a call of the points launch alone
 * may pass NULL for them. */
#define NJF_FIELD_POSE_MAX_COMMANDS 65535
#define NJF_FIELD_POSE_WORKSPACE(M, K) (12LL * (M) * (K) + ((K) + 1) / 2)
#define NJF_FIELD_POSE_LINKS 1          /* phases: one launch each */
#define NJF_FIELD_POSE_CHAIN 2
#define NJF_FIELD_POSE_POINTS 4
#define NJF_FIELD_POSE_ALL 7
#define NJF_FIELD_POSE_STAGED 8         /* modifiers of _POINTS, not part of _ALL */
#define NJF_FIELD_POSE_WIDE 16
int njf_field_pose(const int* parts, const int* parts_count, int num_parts, const int* part_status, const double* centroid,
                   const double* omega, const double* velocity, int action_dim, const int* part_a, const int* part_b,
                   const int* joints_count, int max_joints, const double* anchor, const double* joint_omega,
                   const double* joint_velocity, const int* parent, const int* joint_of, const float* commands, int num_commands,
                   double* rotation, double* translation, int* status, int* depth, const float* xyz, const int* labels,
                   const int* count, int n, const float* jacobian, float* posed, double* workspace, long long workspace_doubles,
                   int phases, void* stream);

/* ---- inverse kinematics on the part tree: commands from 3-D point targets (ABI v20, additive) --------------
 * For each of M problems, the command u whose finite pose (njf_field_pose's, not its linearisation) brings labelled points to
 * their targets: L_m(u) = (1/W_m) sum_i w_i |R_p(u) x_i + t_p(u) - y_mi|^2 + (reg/A) |u|^2, in double.
 * Inputs, all on the device: the part list, twists, optional joints and tree exactly as njf_field_pose takes them; the points xyz
 * [n,3] float, labels [n] int32, count (int32, NULL = n); targets [M,n,3] float; weights float, NULL, [n] (weights_per_problem 0)
 * or [M,n] (1); init, lower, upper [M,A] float or NULL (zeros, -inf, +inf).
 * COUNTED ROWS of problem m: i < min(*count, n); the label has a slot p by njf_field_pose's rule; the slot's pose status is 0; the
 *        weight is finite and > 0 (1 without weights; a NaN or a negative weight counts as 0); the three target coordinates are
 *        finite (a NaN target leaves a row unconstrained).  Every other row is neither in the objective nor an error.
 * MOMENTS [M,K,23] double per (problem, slot), centred on c = centroid[p], x~ = x - c, y~ = y - c: s0 = sum w; s1 = sum w x~ [3];
 *        S2 = sum (w x~_r) x~_c [6: xx xy xz yy yz zz]; t1 = sum w y~ [3]; C[r][c] = sum (w y~_r) x~_c [9]; e = sum w ((y~0 y~0 +
 *        y~1 y~1) + y~2 y~2).  Workgroup (chunk of NJF_FIELD_TWISTS_CHUNK rows, slot, tile of problems) compacts the chunk's rows
 *        of the slot in order; a wave owns a problem, lane l adds the list entries l, l + 64, ..., a butterfly adds the lanes, and
 *        the finishing launch adds the chunks in ascending order: the order depends on (n, K, M) alone, there are no
 *        floating-point atomics, two calls give equal bytes.  A slot whose pose status is not 0 has zeros.
 * SOLVE  One workgroup per problem, thread p owns slot p.  At a point u: the link motions G and, per link and channel, the
 *        spatial derivative twist (W, U) -- W = V w', U = -W x (c + V v) + V v' + dV v, dV = 2 (w.w') (b2 [w]x + g2 [w]x^2) + b
 *        [w']x + g ([w']x [w]x + [w]x [w']x), b2 = db/dth2 and g2 = dg/dth2 by their series up to th2 <= 1e-2 and in closed form
 *        above --; up the parents S <- Ad_G(S) + S_q, then T <- G_q o T, a walk of at most K steps with every index checked; cost,
 *        half-gradient g and Gauss-Newton matrix H per part from the moments, added in a fixed order.  Then the rule of
 *        njf_solve_action_robust in double: u = (float)clamp(init), lam = damping; per iteration g~ = g + (reg/A) u, H~ = H +
 *        (reg/A) I, a coordinate on a bound whose g~ points out of the box is frozen, H~_ii += lam max(H~_ii, 1e-12), un-pivoted
 *        Gauss-Jordan, cand = (float)clamp(u - step), accepted iff L(cand) < L(u) (a NaN rejects), lam <- clamp(accepted ? lam /
 *        3 : 4 lam, 1e-9, 1e9).  `iterations` rounds follow the first evaluation; the iterate lives on the fp32 lattice.
 * Outputs: commands [M,A] float; cost, initial_cost, weight [M] double (the mean squared distance at commands and at the start,
 *        clamped at 0; W_m); steps [M] int32 (accepted); gradient [M,A] double (g~ at commands); status [M] int32, bit
 *        NJF_FIELD_COMMANDS_NO_ROWS: no counted row, NJF_FIELD_COMMANDS_NOT_FINITE: the starting objective is not finite (either
 *        way commands = the clamped init); part_status, depth [K] int32: njf_field_pose's status and depth.
 * workspace: NJF_FIELD_COMMANDS_WORKSPACE(M, K, A, n) doubles of the caller's: the chunks' partial moments [chunks,K,M,23], then
 * the twists of the links and of the chains [M,2,K,A,6].
 * `phases`: NJF_FIELD_COMMANDS_MOMENTS (two launches; writes moments, part_status, depth) | NJF_FIELD_COMMANDS_SOLVE (one launch;
 * READS moments, so it can be fed given ones, and writes every other output, and part_status and depth once more with the same
 * values: it walks the tree itself and does not trust what a caller may have left there).  One stream, no host read (capture-safe).
 * Returns, before the first launch: NJF_E_VALUE for K, A, M or J outside njf_field_pose's ranges, iterations outside [0, 1000],
 * damping not > 0, reg not >= 0, weights_per_problem not 0 or 1, or unknown phases; NJF_E_SHAPE for n < 0 or a workspace that is
 * too small; NJF_E_NULL for a missing pointer, or joints without a tree or a tree without joints. */
#define NJF_FIELD_COMMANDS_MOMENTS_PER_PART 23
#define NJF_FIELD_COMMANDS_MAX_ITERATIONS 1000
#define NJF_FIELD_COMMANDS_WORKSPACE(M, K, A, n) \
  ((23LL * (((n) + NJF_FIELD_TWISTS_CHUNK - 1LL) / NJF_FIELD_TWISTS_CHUNK) + 12LL * (A)) * (M) * (K))
#define NJF_FIELD_COMMANDS_MOMENTS 1    /* phases */
#define NJF_FIELD_COMMANDS_SOLVE 2
#define NJF_FIELD_COMMANDS_ALL 3
#define NJF_FIELD_COMMANDS_NO_ROWS 1    /* status bits */
#define NJF_FIELD_COMMANDS_NOT_FINITE 2
int njf_field_commands(const int* parts, const int* parts_count, int num_parts, const int* part_status, const double* centroid,
                       const double* omega, const double* velocity, int action_dim, const int* part_a, const int* part_b,
                       const int* joints_count, int max_joints, const double* anchor, const double* joint_omega,
                       const double* joint_velocity, const int* parent, const int* joint_of, const float* xyz, const int* labels,
                       const int* count, int n, const float* targets, int num_problems, const float* weights,
                       int weights_per_problem, const float* init, const float* lower, const float* upper, double reg,
                       int iterations, double damping, float* commands, double* cost, double* initial_cost, double* weight,
                       int* steps, double* gradient, int* status, int* out_part_status, int* depth, double* moments,
                       double* workspace, long long workspace_doubles, int phases, void* stream);

/* ---- inverse kinematics with a 3x3 information per target: pixel rays, planes, depth noise (ABI v20, additive; DESIGN.md
 * section 20) ----------------------------------------------------------------------------------------------------------------------
 * njf_field_commands with an anisotropic error per row: L_m(u) = (1/W_m) sum_i w_i z_mi^T Q_mi z_mi + (reg/A) |u|^2, z_mi =
 * R_p(u) x_i + t_p(u) - y_mi, W_m = sum w_i, in double.  Q = I - d d^T holds a point to the ray of a pixel, Q = n n^T to a plane
 * (point-to-plane registration), an inverse covariance weighs a depth camera's noise; Q = I is njf_field_commands' objective.
 * Inputs: everything njf_field_commands takes, and information float, [n,6] (information_per_problem 0) or [M,n,6] (1): the
 * symmetric Q of a row as [xx xy xz yy yz zz], widened to double.  Q is not tested for definiteness -- that is the caller's
 * contract -- and the cost is clamped at 0 as before.
 * COUNTED ROWS: njf_field_commands' rule, and all six information entries finite: a NaN in the information leaves the row out,
 *        like a NaN target.
 * MOMENTS [M,K,74] double per (problem, slot) about c = centroid[p]; x^ = (x~0, x~1, x~2, 1), x~ = x - c, y~ = y - c, b_a =
 *        (Q_a0 y~0 + Q_a1 y~1) + Q_a2 y~2:
 *        [0] s0 = sum w; [1 + 10 e + f] P[e][f] = sum (w Q_e) (x^_i x^_j), e over xx xy xz yy yz zz, f over the pairs i <= j in the
 *        order 00 01 02 03 11 12 13 22 23 33; [61 + 4 a + j] B[a][j] = sum (w b_a) x^_j; [73] e = sum w ((y~0 b0 + y~1 b1) + y~2
 *        b2).  Every term in double in exactly this parenthesisation, no contraction.  The launch has njf_field_commands' shape
 *        -- workgroup (chunk, slot, tile of problems), the chunk's rows compacted in order, a wave per problem, lane l adding the
 *        list entries l, l + 64, ... -- and the lanes are added by a REDUCE-SCATTER: with the partner at lane ^ 32 a lane exchanges
 *        one half of its 74 sums and keeps the pair's sums of the other (lower half [0, ceil(L/2)) to the lane whose bit is
 *        clear), then ^ 16 on the 37 it kept, and so on -- 37 + 19 + 10 + 5 + 3 + 2 = 76 cross-lane moves instead of 74 x 6 --
 *        until every lane holds at most two finished sums, which it stores.  Each finished sum is the butterfly's tree over the
 *        lanes (offsets 32, 16, ..., 1); the finishing launch adds the chunks in ascending order.  The order depends on (n, K, M)
 *        alone, there are no floating-point atomics, two calls give equal bytes.  A slot whose pose status is not 0 has zeros.
 *        NJF_FIELD_COMMANDS_METRIC_BUTTERFLY: the same sums by 74 butterflies, kept to be measured against.
 * SOLVE  njf_field_commands' solver with the block that turns moments into shares replaced.  Slot p at pose (R, t) with derivative
 *        twists (W_k, U_k): d = R c + t, G = (R | d - c) and D_k = ([W_k]x R | W_k x d + U_k), 3 x 4 each, <X, Y> = sum_{a,b,i,j}
 *        X_ai Y_bj P[ab][ij].  The slot's shares: cost <G, G> - 2 sum G_ai B_ai + e, half-gradient <D_k, G> - sum D_k,ai B_ai,
 *        Gauss-Newton matrix <D_k, D_l>.  The links, the chain walk with its index checks, the order in which the shares are
 *        added, the Levenberg-Marquardt rule on the fp32 lattice with bounds and reg, and the status bits are
 *        njf_field_commands', word for word.
 * Outputs: those of njf_field_commands, moments being [M,K,74].
 * workspace: NJF_FIELD_COMMANDS_METRIC_WORKSPACE(M, K, A, n) doubles: the chunks' partial moments [chunks,K,M,74], then the
 * twists of the links and of the chains [M,2,K,A,6].
 * `phases`: NJF_FIELD_COMMANDS_MOMENTS | NJF_FIELD_COMMANDS_SOLVE as in njf_field_commands (the solve phase READS moments) [|
 * NJF_FIELD_COMMANDS_METRIC_BUTTERFLY, a modifier of the moments phase].  One stream, no host read (capture-safe).
 * Returns, before the first launch: NJF_E_VALUE for everything njf_field_commands answers so, information_per_problem not 0 or
 * 1, or unknown phases (the modifier without the moments phase included); NJF_E_SHAPE for n < 0 or a workspace that is too
 * small; NJF_E_NULL for a missing pointer -- information, with the moments phase and n > 0, is one --, or joints without a tree
 * or a tree without joints. */
#define NJF_FIELD_COMMANDS_METRIC_MOMENTS_PER_PART 74
#define NJF_FIELD_COMMANDS_METRIC_WORKSPACE(M, K, A, n) \
  ((74LL * (((n) + NJF_FIELD_TWISTS_CHUNK - 1LL) / NJF_FIELD_TWISTS_CHUNK) + 12LL * (A)) * (M) * (K))
#define NJF_FIELD_COMMANDS_METRIC_BUTTERFLY 4    /* modifier of _MOMENTS, not part of _ALL */
int njf_field_commands_metric(const int* parts, const int* parts_count, int num_parts, const int* part_status,
                              const double* centroid, const double* omega, const double* velocity, int action_dim,
                              const int* part_a, const int* part_b, const int* joints_count, int max_joints, const double* anchor,
                              const double* joint_omega, const double* joint_velocity, const int* parent, const int* joint_of,
                              const float* xyz, const int* labels, const int* count, int n, const float* targets,
                              const float* information, int information_per_problem, int num_problems, const float* weights,
                              int weights_per_problem, const float* init, const float* lower, const float* upper, double reg,
                              int iterations, double damping, float* commands, double* cost, double* initial_cost, double* weight,
                              int* steps, double* gradient, int* status, int* out_part_status, int* depth, double* moments,
                              double* workspace, long long workspace_doubles, int phases, void* stream);

/* ---- closest points of an unlabelled cloud against a cell list (ABI v20, additive) -------------------------
 * For each of M problems and each row of a set of query points, the closest valid point of an observed cloud: the
 * correspondence step between the posed rows of a body and an observation of it (njf_field_commands takes `matched` as its
 * targets unchanged).  The result is the exact brute-force arg-min of the fp32 expression below; the cell list changes only
 * the cost.
 * Inputs, all on the device: observed [Mo,T,3] float; observed_count int32 [Mo] or NULL (= T); queries [Mq,n,3] float; count
 * int32 [1] or NULL (= n); labels int32 [n] or NULL.  Mo and Mq are each 1 or M: with Mo = 1 every problem searches the same
 * cloud, and its cell list is built once.  `cells`: the lattice -- origin = its lower corner, the three steps equal to one
 * cell > 0, dims = cells per axis.
 * VALID POINT j of problem m: j < min(observed_count[m], T) and three finite coordinates.
 * SEARCHED ROW i: i < min(*count, n), three finite coordinates, and labels[i] >= 0 when labels are given.
 * DISTANCE d2(q, p) = (dx*dx + dy*dy) + dz*dz in float, dx = q.x - p.x and so on, in exactly this order, no contraction.
 * RESULT of a searched row: the valid point of the smallest d2, ties to the LOWEST j; accepted iff d2 <= (float)max_distance *
 *        (float)max_distance, a float product.
 * Outputs: index [M,n] int32 (-1 = none); distance2 [M,n] float (+inf = none); matched [M,n,3] float: the observed point itself,
 *        bit for bit, or three NaNs (njf_field_commands' "this row is free"); found [M] int32: the accepted rows.  Every row i <
 *        n is written; a row that is not searched -- rows from the count on included -- is not READ and gets -1 / +inf / NaN.
 * CELLS  cell(p)_c = clamp(floor((p_c - origin_c) * (1 / cell)), 0, dims_c - 1) in float, for points and queries alike: what lies
 *        outside the box lands in a boundary cell and is still found.  Cell (cx, cy, cz) has the index (cx*dy + cy)*dz + cz.
 * BUILD  one memset and five launches: counts per (problem, cell) with integer atomics; an exclusive scan over the Mo * C
 *        counts (sums of blocks of 1024, one workgroup over those sums, the cells of every block); a fill that writes each
 *        valid point as one 16-byte record (x, y, z, j) at its cell's range.  The slot inside a range is taken with an integer
 *        atomic: the order inside a cell, and with it the workspace bytes, may differ from run to run; the outputs may not --
 *        the arg-min with its lowest-j tie-break does not depend on the visiting order.
 * QUERY  one memset (found) and one launch, one lane per (m, i): Chebyshev rings r = 0, 1, ... of cells around the query's
 *        cell (ring 0), clipped to the lattice; after ring r >= 1 the search stops when best_d2 < ((r - 1/128) * cell)^2 or (r -
 *        1/128) * cell > max_distance (float), after any ring when no cell is left beyond it, and at the latest after ring
 *        NJF_FIELD_NEAREST_MAX_RINGS -- which the second test reaches first for every max_distance the entry admits.  The
 *        clamp is 1-Lipschitz per axis, so a point in a ring beyond r is at least r cells away up to the rounding of the
 *        cell coordinate (< 2^-12 cells) and of d2 (~2^-22): the slack of cell / 128 covers both.  Every cell index is
 *        checked against [0, Mo * C) and every range against [0, Mo * T) before use.
 *        NJF_FIELD_NEAREST_WAVE: the same search with one wave per (m, i), the lanes sharing a range's records.
 * workspace: NJF_FIELD_NEAREST_WORKSPACE(Mo, C, T) 32-bit words of the caller's, C = dims[0]*dims[1]*dims[2]: Mo (C + 1) starts,
 * Mo C cursors, 4 Mo T record words and 3 words to bring the records to a 16-byte boundary.
 * `phases`: NJF_FIELD_NEAREST_BUILD (reads observed, writes the workspace) | NJF_FIELD_NEAREST_QUERY (reads the workspace and
 * the queries, writes the outputs) [| NJF_FIELD_NEAREST_WAVE]: build once, query many times.  One stream, no host read
 * (capture-safe).
 * Returns, before the first launch: NJF_E_VALUE for M outside [1, NJF_FIELD_POSE_MAX_COMMANDS], Mo or Mq not 1 or M, a dims[c]
 * outside [1, NJF_FIELD_NEAREST_MAX_DIM], unequal, non-positive or non-finite steps (or 1 / cell not finite), a non-finite
 * origin, max_distance not > 0 or not finite as a float, ceil(max_distance / cell) + 1 > NJF_FIELD_NEAREST_MAX_RINGS, Mo * C >=
 * 2^31, or unknown phases; NJF_E_SHAPE for n < 0, T < 1, Mo * T >= 2^31 or a workspace that is too small; NJF_E_NULL for a
 * missing pointer. */
#define NJF_FIELD_NEAREST_MAX_RINGS 64
#define NJF_FIELD_NEAREST_MAX_DIM 1024
#define NJF_FIELD_NEAREST_WORKSPACE(Mo, C, T) ((long long)(Mo) * (2LL * (C) + 1LL + 4LL * (T)) + 3LL)
#define NJF_FIELD_NEAREST_BUILD 1    /* phases */
#define NJF_FIELD_NEAREST_QUERY 2
#define NJF_FIELD_NEAREST_ALL 3
#define NJF_FIELD_NEAREST_WAVE 4     /* with QUERY: a wave per query */
int njf_field_nearest(const float* observed, const int* observed_count, int num_observed, int points, const float* queries,
                      const int* count, const int* labels, int num_queries, int n, int num_problems, const NjfFieldGrid* cells,
                      double max_distance, int* index, float* distance2, float* matched, int* found, int* workspace,
                      long long workspace_words, int phases, void* stream);

/* ---- surface normals of an observed cloud from exact moments on the cell list (ABI v20, additive) -----------
 * For each of M problems and each row of a set of query points: the normal, the neighbour count and the surface variation of the
 * observed points within `radius`, from their covariance -- what plane_information needs of a cloud that comes with points alone.
 * The neighbourhood sums are integers, so that the order in which the cell list is read cannot change a byte of any output.
 * Inputs, all on the device: observed [Mo,T,3] float; observed_count int32 [Mo] or NULL (= T); queries [Mq,n,3] float; count
 * int32 [1] or NULL (= n); viewpoint [Mv,3] float or NULL.  Mo, Mq and Mv are each 1 or M.  `cells`: njf_field_nearest's
 * lattice, under the same rules.  `radius` is used as (float)radius; `min_neighbours` >= 3.
 * VALID POINT j of problem m: j < min(observed_count[m], T) and three finite coordinates.
 * SEARCHED ROW i: i < min(*count, n) and three finite coordinates.
 * NEIGHBOUR of a searched row q: a valid point p with d2 = (ex*ex + ey*ey) + ez*ez <= (float)radius * (float)radius, e_c = p_c -
 *        q_c, all in float, in exactly this order, no contraction.  A query that is a point of the cloud is its own neighbour.
 * CELLS  visited: the Chebyshev rings 0 .. R around the query's cell (njf_field_nearest's CELLS), clipped to the lattice, R the
 *        smallest r >= 1 with ((float)r - 1/128) * cell > (float)radius in float: njf_field_nearest's second stop test, exact by
 *        its argument (the clamp is 1-Lipschitz, the slack of cell / 128 covers the rounding).  Every cell index is checked
 *        against [0, Mo * C) and every range against [0, Mo * T) before use.
 * MOMENTS scale = 262144.0 / (double)(float)radius (2^18 / radius, one double division); k_c = rint((double)e_c * scale), a double
 *        product rounded to the nearest integer, ties to even; d2 <= r2 gives |k_c| <= 2^18 + 1.  Ten int64 sums over the
 *        neighbours of a row: S0 = sum 1; S1[3] = sum k; S2[6] = sum k_a k_b as [xx xy xz yy yz zz]; moments [M,n,10] int64 holds
 *        (S0, S1, S2), zeros for a row that is not searched.  |S2| < (2^18 + 1)^2 T < 2^63 for T < 2^26.  Integer addition is
 *        associative: the sums are the same bytes in any visiting order, and in both kernel forms.
 *        NJF_FIELD_NORMALS_WAVE: one wave per (m, i) instead of one lane, the lanes sharing a range's records.
 * FINISH one lane per (m, i), in double, no contraction; reads the moments of the rows i < min(*count, n) and nothing else,
 *        except the query and the viewpoint of a row whose normal it orients.
 *        N = S0; with N < min_neighbours there is no normal.  mean_a = (double)S1_a / (double)N; C_ab = (double)S2_ab / (double)N
 *        - mean_a * mean_b.  Eigen-decomposition by cyclic Jacobi rotations on the pairs (p,q) = (0,1), (0,2), (1,2), exactly
 *        8 sweeps; a pair with C_pq == 0 is skipped and there is no other exit.  One rotation, o the third axis: theta = (C_qq -
 *        C_pp) / (2 C_pq); t = sgn(theta) / (|theta| + sqrt(theta * theta + 1)), sgn(0) = 1; c = 1 / sqrt(t * t + 1); s = t * c;
 *        C_pp -= t C_pq; C_qq += t C_pq; C_pq = 0; (C_op, C_oq) <- (c C_op - s C_oq, s C_op + c C_oq); every row k of V (the
 *        identity at first): (V_kp, V_kq) <- (c V_kp - s V_kq, s V_kp + c V_kq).  lambda = the diagonal, sorted ascending (ties
 *        in the order of the axes) and clamped at 0; with (lambda0 + lambda1) + lambda2 == 0 -- all neighbours coincide -- there
 *        is no normal.  Otherwise the normal is the column of V that belongs to lambda0, divided by its length.
 * SIGN   with a viewpoint v of three finite coordinates: flipped iff (n_x (v_x - q_x) + n_y (v_y - q_y)) + n_z (v_z - q_z) < 0, in
 *        double from the float inputs.  Otherwise (NULL, or not finite): flipped iff the component of largest magnitude, ties
 *        to the lowest axis, is negative.
 * Outputs, every row i < n written: normal [M,n,3] float (three NaNs where there is no normal); neighbours [M,n] int32 = S0 (0
 *        for a row that is not searched); variation [M,n] float = lambda0 / ((lambda0 + lambda1) + lambda2), 0 on a plane and 1/3
 *        for an isotropic neighbourhood (NaN where there is no normal); eigenvalues [M,n,3] double or NULL = lambda / (scale *
 *        scale), ascending, in the cloud's units (NaN where there is no normal).
 * workspace: njf_field_nearest's, NJF_FIELD_NORMALS_WORKSPACE(Mo, C, T) = NJF_FIELD_NEAREST_WORKSPACE(Mo, C, T) words in its
 * documented layout; one that njf_field_nearest's build phase wrote for the same observed and cells is taken as it is.
 * `phases`: NJF_FIELD_NORMALS_BUILD (njf_field_nearest's build: reads observed, writes the workspace) | NJF_FIELD_NORMALS_MOMENTS
 * (reads the workspace and the queries, writes moments) [| NJF_FIELD_NORMALS_WAVE] | NJF_FIELD_NORMALS_FINISH (reads moments, writes
 * the outputs).  One stream, no host read (capture-safe), no atomics beyond the build's integer ones.
 * Returns, before the first launch: NJF_E_VALUE for everything njf_field_nearest answers so (radius in max_distance's place), Mv
 * not 1 or M with a viewpoint, min_neighbours < 3, or unknown phases (the modifier without the moments phase included);
 * NJF_E_SHAPE for n < 0, T < 1, T >= 2^26, Mo * T >= 2^31 or, with the build or the moments phase, a workspace that is too small;
 * NJF_E_NULL for a missing pointer: cells; the workspace with the build or the moments phase; observed with the build; with n >
 * 0, queries and moments with the moments or the finish phase, normal, neighbours and variation with the finish phase. */
#define NJF_FIELD_NORMALS_WORKSPACE(Mo, C, T) NJF_FIELD_NEAREST_WORKSPACE(Mo, C, T)
#define NJF_FIELD_NORMALS_MOMENTS_PER_ROW 10
#define NJF_FIELD_NORMALS_SWEEPS 8
#define NJF_FIELD_NORMALS_BUILD 1    /* phases */
#define NJF_FIELD_NORMALS_MOMENTS 2
#define NJF_FIELD_NORMALS_FINISH 4
#define NJF_FIELD_NORMALS_ALL 7
#define NJF_FIELD_NORMALS_WAVE 8     /* with MOMENTS: a wave per row */
int njf_field_normals(const float* observed, const int* observed_count, int num_observed, int points, const float* queries,
                      const int* count, int num_queries, int n, int num_problems, const NjfFieldGrid* cells, double radius,
                      int min_neighbours, const float* viewpoint, int num_viewpoints, long long* moments, float* normal,
                      int* neighbours, float* variation, double* eigenvalues, int* workspace, long long workspace_words,
                      int phases, void* stream);

/* ---- a depth frame to world points (ABI v20, additive) -------------------------------------------------------
 * The back-projection of B depth images through the package's cameras: the observed cloud that njf_field_nearest, njf_field_normals
 * and njf_field_voxels take, with the invalid and the "flying" pixels of a real sensor taken out.
 * Inputs, all on the device: depth [B,H,W] float; k_inv [B,3,3] float, the INVERSE of the normalised intrinsics; c2w [B,4,4] float.
 * PIXEL  r = row * W + col has the centre x = ((float)col + 0.5f) / (float)W, y = ((float)row + 0.5f) / (float)H (row-major,
 *        get_pixel_coordinates' grid).
 * RAY    njf_generate_rays' of that centre, bit for bit -- the same fma chains, sqrtf and divisions: origin o = the translation of
 *        c2w, unit direction d, and cz, the camera-space z of the unit direction.
 * POINT  t = depth for NJF_FIELD_DEPTH_RAY (a distance along the unit ray: the package's own rendered depth), t = depth / cz, an
 *        IEEE division, for NJF_FIELD_DEPTH_Z (what depth cameras report).  p_c = o_c + d_c * t: one float multiply and one float
 *        add per component, no contraction.
 * VALID  a pixel of depth d is valid when d is finite and near < d <= far, compared in float: near = 0 drops the zeros that sensors
 *        write for "no return".  With max_jump > 0 a valid pixel is dropped as well when one of its 4-neighbours inside the image
 *        has a valid depth dn with fabsf(d - dn) > max_jump * fminf(d, dn) (a float product).  Invalid neighbours do not count; the
 *        rule is symmetric, so both sides of a depth edge go; it reads the input only.  max_jump = 0: no such test.
 * Outputs: points [B,H*W,3] float -- read as [B / V, V*H*W, 3], the V = views_per_scene consecutive views of a scene are one
 *        cloud; EVERY row is written, a pixel that gives no point gets three NaNs, which the cell-list build skips.  kept [B / V]
 *        int32: the pixels that gave a point, counted with integer atomics.
 * One memset (kept) and one launch, one lane per pixel; one stream, no host read (capture-safe).
 * Returns, before the launch: NJF_E_NULL for a missing pointer; NJF_E_SHAPE for B, H or W < 1, B*H*W >= 2^31, V < 1 or B % V != 0;
 * NJF_E_VALUE for an unknown kind, near not in [0, inf), far not > near (NaN included), max_jump negative or not finite. */
#define NJF_FIELD_DEPTH_RAY 0        /* kind */
#define NJF_FIELD_DEPTH_Z 1
int njf_field_depth_points(const float* depth, int batch, int height, int width, const float* k_inv, const float* c2w, int kind,
                           float near, float far, float max_jump, int views_per_scene, float* points, int* kept, void* stream);

/* ---- one centroid per occupied cell of a cloud (ABI v20, additive) ---------------------------------------------
 * For each of M clouds: the points that fall into one cell of a lattice are replaced by their centroid -- the standard thinning of
 * a cloud that is much denser than its cells, which also averages sensor noise.  The sums are integers, so that the order in
 * which the cell list is read cannot change a byte of any output.
 * Inputs, all on the device: points [M,T,3] float; points_count int32 [M] or NULL (= T).  `cells`: njf_field_nearest's lattice,
 * under the same rules: origin = its lower corner, three equal steps `cell` > 0, dims = cells per axis, inv_cell = 1.0f / cell.
 * VALID POINT j of problem m: j < min(points_count[m], T) and three finite coordinates.
 * INSIDE a valid point is inside when 0 <= floorf(t_c) < dims_c on all three axes, t_c = (p_c - origin_c) * inv_cell in float,
 *        njf_field_nearest's cell coordinate: its unclamped cell is the cell the build stores it in.  The other valid points,
 *        which the build puts into boundary cells, are not reduced; they are counted in outside [M].
 * SUMS   an inside point adds q_c = (long long)rintf((t_c - floorf(t_c)) * 1048576.0f), in [0, 2^20], to three int64 sums S_c of its
 *        cell, and 1 to the cell's count k.  Integer addition is associative: the same bytes in any order, and in both forms.
 * KEPT   a cell with k >= min_points, 1 <= min_points.  Its centroid is (float)(origin_c + (cell_index_c + S_c / (k * 2^20)) * cell)
 *        in double with exactly this association: (double)S_c / ((double)k * 1048576.0), plus (double)cell_index_c, times
 *        (double)cell, plus (double)origin_c, no contraction.
 * ORDER  the kept cells of a problem in ascending cell index (cx*dy + cy)*dz + cz.
 * Outputs: out_points [M,capacity,3] float; weight [M,capacity] int32 = k; cell_index [M,capacity] int32; sums [M,capacity,3] int64;
 *        count [M] int32 = the TRUE number of kept cells, which may exceed capacity (the rows beyond it are dropped); outside [M]
 *        int32.  Rows from min(count, capacity) on are written too: NaN, 0, -1, 0 -- out_points is a valid `observed` of
 *        njf_field_nearest with or without count as its observed_count.  capacity = min(T, C) cannot overflow.
 * BUILD  njf_field_nearest's build (a memset, five launches) on the same workspace.
 * REDUCE a memset (outside) and one launch, one lane per (problem, cell), which reads the cell's range of 16-byte records and writes
 *        the cell's sums, its count and its kept flag into the workspace; outside with integer atomics.  Every range is clamped
 *        to [0, M * T) and to T records before use: on a workspace that was never built it reads nothing outside it.
 *        NJF_FIELD_VOXELS_WAVE: one wave per (problem, cell), the lanes sharing the records.
 * COMPACT four launches: the exclusive scan of the kept flags over the M * C cells -- the build's three scan launches on a second
 *        starts array -- and the ordered scatter, which also writes the fill rows and count.  The scan clears the flags (they
 *        live in the build's cursors, which nothing reads after the build): every COMPACT needs a REDUCE of its own before it.
 *        A row index is checked against [0, capacity) before it is written.
 * workspace: NJF_FIELD_VOXELS_WORKSPACE(M, C, T) 32-bit words, C = dims[0]*dims[1]*dims[2]: njf_field_nearest's, in its layout, and
 * behind its records 3 M C int64 sums, M C counts and M C + 1 second starts.  The starts and the records stay as the build wrote
 * them: the same workspace still answers njf_field_nearest's query phase, and one that njf_field_nearest's build wrote (in a
 * buffer of this size) is taken as it is.
 * `phases`: NJF_FIELD_VOXELS_BUILD | NJF_FIELD_VOXELS_REDUCE [| NJF_FIELD_VOXELS_WAVE] | NJF_FIELD_VOXELS_COMPACT.  One stream, no
 * host read (capture-safe), integer atomics only.
 * Returns, before the first launch: NJF_E_VALUE for M outside [1, NJF_FIELD_POSE_MAX_COMMANDS], a lattice njf_field_nearest
 * refuses, M * C >= 2^31, min_points < 1 or unknown phases (the modifier without the reduce phase included); NJF_E_SHAPE for T <
 * 1, M * T >= 2^31, capacity < 1, M * capacity >= 2^31 or a workspace that is too small; NJF_E_NULL for a missing pointer: cells;
 * the workspace; points with the build; outside with the reduce; the other five outputs with the compact phase. */
#define NJF_FIELD_VOXELS_WORKSPACE(M, C, T) (NJF_FIELD_NEAREST_WORKSPACE(M, C, T) + 8LL * (M) * (C) + 1LL)
#define NJF_FIELD_VOXELS_QUANTUM 1048576   /* 2^20 steps per cell */
#define NJF_FIELD_VOXELS_BUILD 1     /* phases */
#define NJF_FIELD_VOXELS_REDUCE 2
#define NJF_FIELD_VOXELS_COMPACT 4
#define NJF_FIELD_VOXELS_ALL 7
#define NJF_FIELD_VOXELS_WAVE 8      /* with REDUCE: a wave per cell */
int njf_field_voxels(const float* points, const int* points_count, int num_problems, int num_points, const NjfFieldGrid* cells,
                     int min_points, int capacity, float* out_points, int* weight, int* cell_index, long long* sums, int* count,
                     int* outside, int* workspace, long long workspace_words, int phases, void* stream);

/* ---- which posed rows a depth camera sees: a z-buffer of points (ABI v20, additive) -----------------------------
 * For each of M problems and V cameras: the rows of a point set splatted into a depth image -- the inverse of
 * njf_field_depth_points with NJF_FIELD_DEPTH_Z --, and per row whether it is the nearest thing in its own pixel.  `culled` goes into
 * njf_field_nearest's QUERY phase as its queries: a hidden row is a row that is not searched.
 * Inputs, all on the device: points [Mq,n,3] float, Mq = 1 or M; count int32 [1] or NULL (= n); labels int32 [n] or NULL; k [V,3,3]
 * float, the normalised intrinsics (NOT their inverse; the third row is not read and taken as 0 0 1); w2c [V,4,4] float, world to
 * camera (its fourth row is not read).  The cameras are shared by the M problems.
 * READ ROW i: i < min(*count, n), three finite coordinates, and labels[i] >= 0 when labels are given (njf_field_nearest's SEARCHED
 *        ROW).  A row that is not read is not splatted, not visible, and gets the fill values below.
 * PROJECTION of a read row p in view v, in float, nothing contracted beyond the fmaf written here:
 *        xc = fmaf(w[2], p.z, fmaf(w[1], p.y, fmaf(w[0], p.x, w[3]))), yc and zc likewise from w[4..7] and w[8..11], w = w2c[v]
 *        row-major; PROJECTABLE when zc is finite and zc > near.  s = xc / zc, t = yc / zc (IEEE divisions);
 *        pu = fmaf(k[1], t, fmaf(k[0], s, k[2])), pv = fmaf(k[4], t, fmaf(k[3], s, k[5])); col = floorf(pu * (float)W), row =
 *        floorf(pv * (float)H) (get_pixel_coordinates' grid: pixel (row, col) covers [col, col + 1) / W x [row, row + 1) / H).
 *        INSIDE when projectable and 0 <= col < W and 0 <= row < H, compared as floats before any conversion to int.
 * SPLAT  a projectable row writes the key (bits(zc) << 32) | i, a 64-bit unsigned minimum, into the pixels (row + dr, col + dc),
 *        |dr|, |dc| <= footprint, that lie in the image -- also where its own pixel does not.  The key image starts as all ones.
 *        zc > 0 is finite, so its bits order as the float does: a pixel's winner is the smallest zc, ties to the LOWEST row i, in
 *        any order of the atomics.  By default a plain load of the key precedes the atomic, which is skipped where the pixel
 *        already holds a key that is not larger; the minimum is monotone, so this cannot change a byte.
 *        NJF_FIELD_VISIBLE_DIRECT: every atomic is issued.
 * RESOLVE a workgroup per 2,048 pixels of one image, eight per lane, and one count atomic per workgroup: depth [M,V,H,W] float =
 *        the winner's zc, 0 for an empty pixel (njf_field_depth_points drops it with near = 0); index [M,V,H,W] int32 = the
 *        winner's row, -1 for an empty pixel; covered [M,V] int32 = the pixels with a winner.
 * TEST   one lane per (m, i), one count atomic per workgroup.  A lane projects again (the same expressions: the same bits) and
 *        reads `depth`: row i is VISIBLE in view v iff it is inside and zc - zmin <= tolerance * zmin, zmin = depth at its own
 *        pixel: a float subtraction, a float product and a comparison, no contraction.  seen [M,n] int32: bit v set iff visible
 *        in view v; culled [M,n,3] float: the point itself, bit for bit, if seen != 0, else three NaNs; visible [M] int32: the
 *        rows with seen != 0; pixel [M,V,n] int32: row * W + col of the row's own pixel, -1 when not inside (or not read); z
 *        [M,V,n] float: zc, NaN when the row is not read.
 * Every element of every output of a phase is written by it.  Integer atomics only (the minimum and the three counts).
 * workspace: NJF_FIELD_VISIBLE_WORKSPACE(M, V, H, W) 32-bit words of the caller's: the M V H W keys of 8 bytes and one word that brings
 * them to an 8-byte boundary.
 * `phases`: NJF_FIELD_VISIBLE_SPLAT (a memset and one launch: reads points, writes the workspace) [| NJF_FIELD_VISIBLE_DIRECT] |
 * NJF_FIELD_VISIBLE_RESOLVE (a memset and one launch: reads the workspace, writes depth, index, covered) | NJF_FIELD_VISIBLE_TEST (a
 * memset and one launch: reads points and depth, writes the other five outputs).  One stream, no host read (capture-safe).
 * Returns, before the first launch: NJF_E_NULL for a missing pointer a requested phase needs (k and w2c: always); NJF_E_VALUE for
 * unknown phases (the modifier without the splat included), M outside [1, NJF_FIELD_POSE_MAX_COMMANDS], Mq not 1 or M, V outside
 * [1, NJF_FIELD_VISIBLE_MAX_VIEWS], a footprint outside [0, NJF_FIELD_VISIBLE_MAX_FOOTPRINT], near or tolerance negative or not
 * finite; NJF_E_SHAPE for n < 0, H or W < 1, M * V * H * W >= 2^31, M * V * n >= 2^31 or, with the splat or the resolve, a workspace
 * that is too small. */
#define NJF_FIELD_VISIBLE_MAX_VIEWS 32
#define NJF_FIELD_VISIBLE_MAX_FOOTPRINT 4
#define NJF_FIELD_VISIBLE_WORKSPACE(M, V, H, W) (2LL * (M) * (V) * (H) * (W) + 1LL)
#define NJF_FIELD_VISIBLE_SPLAT 1    /* phases */
#define NJF_FIELD_VISIBLE_RESOLVE 2
#define NJF_FIELD_VISIBLE_TEST 4
#define NJF_FIELD_VISIBLE_ALL 7
#define NJF_FIELD_VISIBLE_DIRECT 8   /* with SPLAT: no load before the atomic */
int njf_field_visible(const float* points, const int* count, const int* labels, int num_queries, int n, int num_problems,
                      const float* k, const float* w2c, int views, int height, int width, int footprint, float near,
                      float tolerance, float* depth, int* index, int* covered, int* seen, float* culled, int* visible, int* pixel,
                      float* z, int* workspace, long long workspace_words, int phases, void* stream);

/* ---- posed rows against a depth frame by projection: occlusion, free space, window match (ABI v20, additive) ----
 * For each of M problems: every row of a posed point set is projected into V depth cameras, classified against the ORGANISED cloud
 * those cameras observed -- njf_field_depth_points' output, pixel by pixel --, and matched to the closest observed point in a window
 * of pixels around its own.  The frame tells what njf_field_visible cannot know: what the SCENE hides (a row behind something else
 * is not matched to that thing) and where the camera saw through (a row in free space).  No cell list, no build, no workspace.
 * Inputs, all on the device: points [Mq,n,3] float, Mq = 1 or M; count int32 [1] or NULL (= n); labels int32 [n] or NULL; frame
 * [Mo,V*H*W,3] float, Mo = 1 or M: row v*H*W + row*W + col is the point of pixel (row, col) of view v, three NaNs (anything not
 * three finite numbers) where the pixel gave no point; k [V,3,3] and w2c [V,4,4] float, njf_field_visible's, shared by the problems.
 * READ ROW, PROJECTION, INSIDE and the own pixel: njf_field_visible's, word for word -- the kernels call the same device function,
 *        so the bits are the same.  pixel [M,V,n] int32 and z [M,V,n] float: njf_field_visible's, with its fills (-1; NaN when the row
 *        is not read).
 * STATE  of row i in view v, state [M,V,n] int32: NJF_FIELD_FRAME_OUTSIDE (0) when the row is not read or not inside; else, with
 *        (fx, fy, fz) the frame's point at the own pixel, NJF_FIELD_FRAME_NO_RETURN (1) when these are not three finite numbers;
 *        else with zo = fmaf(w[10], fz, fmaf(w[9], fy, fmaf(w[8], fx, w[11]))), the chain that gave zc from the row: IN_FRONT (2)
 *        when zo - zc > tolerance * zo; else BEHIND (4) when zc - zo > tolerance * zo; else ON (3).  A float subtraction, a float
 *        product and a comparison each, nothing contracted; a comparison with a NaN is false.
 * SEARCHED in view v: the state is not OUTSIDE and not BEHIND; with NJF_FIELD_FRAME_KEEP_HIDDEN: not OUTSIDE.
 * WINDOW the pixels (row + dr, col + dc), |dr|, |dc| <= reach, that lie in the image: clipped to [0, H) x [0, W) before any address
 *        is formed, so j = v*H*W + r*W + c lies in [0, V*H*W).
 * RESULT over the windows of all views in which the row is searched: the frame point of three finite coordinates with the smallest
 *        d2 = (dx*dx + dy*dy) + dz*dz in float, dx = q.x - p.x and so on (njf_field_nearest's DISTANCE, in its order, no contraction),
 *        ties to the LOWEST frame row j; accepted iff d2 <= (float)max_distance * (float)max_distance, a float product.
 * Outputs: index [M,n] int32, distance2 [M,n] float, matched [M,n,3] float, found [M] int32: njf_field_nearest's, with its fills
 *        (-1 / +inf / three NaNs) -- index is a row of the frame; states [M,5] int32: the (v, i) pairs of every state code, i < n
 *        (they add up to V n).  Every element of every output is written.
 * One lane per (m, i), which loops over the views and the window.  Integer atomics only: one per workgroup and counter (found and
 * the five states), after a workgroup sum.  Two memsets (found, states) and one launch; one stream, no host read (capture-safe).
 * `phases`: NJF_FIELD_FRAME_MATCH [| NJF_FIELD_FRAME_KEEP_HIDDEN].
 * Returns, before the launch: NJF_E_NULL for a missing pointer (count and labels may be NULL); NJF_E_VALUE for unknown phases (a
 * modifier without MATCH included), M outside [1, NJF_FIELD_POSE_MAX_COMMANDS], Mq or Mo not 1 or M, V outside [1,
 * NJF_FIELD_VISIBLE_MAX_VIEWS], reach outside [0, NJF_FIELD_FRAME_MAX_REACH], near, tolerance or (float)max_distance negative or
 * not finite; NJF_E_SHAPE for n < 0, H or W < 1, Mo * V * H * W >= 2^31 or M * V * n >= 2^31. */
#define NJF_FIELD_FRAME_MAX_REACH 8
#define NJF_FIELD_FRAME_OUTSIDE 0    /* state */
#define NJF_FIELD_FRAME_NO_RETURN 1
#define NJF_FIELD_FRAME_IN_FRONT 2
#define NJF_FIELD_FRAME_ON 3
#define NJF_FIELD_FRAME_BEHIND 4
#define NJF_FIELD_FRAME_STATES 5
#define NJF_FIELD_FRAME_MATCH 1      /* phases */
#define NJF_FIELD_FRAME_KEEP_HIDDEN 2  /* with MATCH: BEHIND rows are searched too */
int njf_field_frame(const float* points, const int* count, const int* labels, int num_queries, int n, int num_problems,
                    const float* frame, int num_frames, const float* k, const float* w2c, int views, int height, int width,
                    int reach, float near, float tolerance, double max_distance, int* pixel, float* z, int* state, int* index,
                    float* distance2, float* matched, int* found, int* states, int phases, void* stream);

/* ---- depth frames fused into a truncated signed distance on a grid; the distance and its gradient at rows (ABI v20, additive;
 * DESIGN.md section 27) ---------------------------------------------------------------------------------------------------------------
 * njf_field_tsdf: for each of M problems, V depth images are fused into one value and one weight per node of `grid`.  Inputs, all on
 * the device: depth [M,V,H,W] float, the camera-space z of every pixel (njf_field_depth_points' NJF_FIELD_DEPTH_Z); k [V,3,3] and w2c
 * [V,4,4] float, njf_field_visible's, shared by the problems; values_in and weight_in [M,N] float, the running state, both or
 * neither (NULL) -- they may BE values and weight: a lane reads and writes its own node only.
 * NODE g of problem m, g = (ix*ny + iy)*nz + iz, at p = fmaf((float)i_c, step[c], origin[c]) per component (njf_field_points' floats):
 *        sum = 0, c = 0; for v = 0 .. V-1 in this order: the node is projected by njf_field_visible's PROJECTION, word for word -- the
 *        kernels call the same device function, so zc, row and col are the bits njf_field_visible reports for the node as a row, with
 *        this `near`.  The view CONTRIBUTES iff the node is INSIDE, d = depth[m, v, row*W + col] is finite, near < d <= far
 *        (njf_field_depth_points' validity) and s = d - zc (one float subtraction) satisfies s >= -truncation (inclusive; a
 *        comparison with a NaN is false); then sum = sum + fminf(s, truncation) and c = c + 1.0f, float additions, nothing contracted.
 * UPDATE with W0 = weight_in[m,g] and D0 = values_in[m,g], W0 = 0 without a state:
 *        c == 0:          values = D0, weight = W0 (the state copied through); without a state values = NaN, weight = 0;
 *        c > 0, W0 > 0:   values = fmaf(W0, D0, sum) / (W0 + c), an IEEE division; weight = fminf(W0 + c, max_weight);
 *        c > 0 otherwise: values = sum / c, an IEEE division -- D0 is not read and may be NaN --; weight = fminf(c, max_weight).
 *        The value is positive in observed free space (in front of the surface) and negative behind it.
 * known [M] int32: the nodes of the problem with weight > 0 after the update.
 * Every element of every output is written.  One lane per (m, g), workgroups of 256 consecutive nodes of one problem; one integer
 * atomic per workgroup for `known`, after a workgroup sum.  One memset (known) and one launch; one stream, no host read (capture-safe).
 * Returns, before the launch: NJF_E_NULL for a missing pointer, or one of values_in / weight_in without the other; NJF_E_VALUE for M
 * outside [1, NJF_FIELD_POSE_MAX_COMMANDS], V outside [1, NJF_FIELD_VISIBLE_MAX_VIEWS], near negative or not finite, far not > near
 * (NaN included; +inf is allowed), truncation not in (0, inf), max_weight not > 0 (NaN included; +inf is allowed); NJF_E_SHAPE for H or
 * W < 1, a dims[c] < 1, nx*ny*nz, M * N or M * V * H * W >= 2^31.
 *
 * njf_field_tsdf_sample: the trilinear interpolant of such a field, and its exact derivative, at the rows of a point set.  Inputs, all
 * on the device: points [Mq,n,3] float, Mq = 1 or M; count int32 [1] or NULL (= n); labels int32 [n] or NULL; values and weight [Mf,N]
 * float, Mf = 1 or M.  A row is READ by njf_field_visible's READ ROW rule (the same device function).
 * CELL   per axis c: g_c = (x_c - origin[c]) / step[c], one float subtraction and one IEEE division.  The row is IN THE GRID iff g_c >=
 *        0 and g_c <= (float)(dims[c] - 1) on all three axes (a comparison with a NaN is false); then i_c = min((int)floorf(g_c),
 *        dims[c] - 2) and f_c = g_c - (float)i_c, a float subtraction: a row on the last node plane has f_c = 1 in the last cell.
 * STATE  state [M,n] int32: NJF_FIELD_TSDF_OUTSIDE (0) when the row is not read or not in the grid; else NJF_FIELD_TSDF_UNKNOWN (1)
 *        when weight == 0 at any of the eight corners (i_x + a, i_y + b, i_z + c), a, b, c in {0, 1}; else NJF_FIELD_TSDF_KNOWN (2).
 * KNOWN  rows, with C[a][b][c] the values at the corners and lerp(u, w, f) = fmaf(f, w - u, u), w - u a float subtraction:
 *        e[a][b] = lerp(C[a][b][0], C[a][b][1], f_z); h[a] = lerp(e[a][0], e[a][1], f_y); distance = lerp(h[0], h[1], f_x);
 *        gradient.x = (h[1] - h[0]) / step[0];
 *        gradient.y = lerp(q[0], q[1], f_x) / step[1], q[a] = e[a][1] - e[a][0];
 *        gradient.z = lerp(t[0], t[1], f_x) / step[2], t[a] = lerp(r[a][0], r[a][1], f_y), r[a][b] = C[a][b][1] - C[a][b][0];
 *        float subtractions and IEEE divisions, nothing contracted beyond the fmaf written here.
 * Outputs: state; distance [M,n] float and gradient [M,n,3] float, NaN unless the row is KNOWN; states [M,3] int32: the rows i < n of
 * every state code (they add up to n).  Every element of every output is written.  One lane per (m, i); one integer atomic per
 * workgroup and counter, after a workgroup sum.  One memset (states) and one launch; one stream, no host read (capture-safe).
 * Returns, before the launch: NJF_E_NULL for a missing pointer (count and labels may be NULL); NJF_E_VALUE for M outside [1,
 * NJF_FIELD_POSE_MAX_COMMANDS], Mq or Mf not 1 or M, a step[c] not in (0, inf), an origin[c] that is not finite, a dims[c] of 1;
 * NJF_E_SHAPE for a dims[c] < 1, n < 0, nx*ny*nz, M * n or Mf * N >= 2^31. */
#define NJF_FIELD_TSDF_OUTSIDE 0     /* state */
#define NJF_FIELD_TSDF_UNKNOWN 1
#define NJF_FIELD_TSDF_KNOWN 2
#define NJF_FIELD_TSDF_STATES 3
int njf_field_tsdf(const NjfFieldGrid* grid, const float* depth, int num_problems, int views, int height, int width, const float* k,
                   const float* w2c, float near, float far, float truncation, float max_weight, const float* values_in,
                   const float* weight_in, float* values, float* weight, int* known, void* stream);
int njf_field_tsdf_sample(const float* points, const int* count, const int* labels, int num_queries, int n, int num_problems,
                          const NjfFieldGrid* grid, const float* values, const float* weight, int num_fields, int* state,
                          float* distance, float* gradient, int* states, void* stream);

/* ---- stand-alone sampler / compositing ops (API parity with the un-fused reference calls) -- */
/* RaySamples.get_weights (ray_samplers.py:77-101): deltas, densities [N,S] -> weights [N,S]. */
int njf_alpha_weights(const float* deltas, const float* densities, int rays, int samples, float* weights, void* stream);
/* PDFSampler.generate_ray_samples (ray_samplers.py:351-451) on spacing bins. */
int njf_pdf_resample(const float* weights, const float* bins_in, int bins_per_ray, int s_in, const float* u,
                     int u_per_ray, int s_out, float anneal, int rays, float* bins_out, void* stream);

/* ---- training: backward of alpha compositing ------------------------------------------------------------------------------- */
/* What autograd runs for RaySamples.get_weights (ray_samplers.py:77-101), render_rgb and the UN-clipped render_depth
 * (model.py:257-279), as one launch: deltas, steps (sample mid-points), sigma [rays,S], color [rays,S,3] (or NULL) are the
 * forward pass's per-sample fields; g_weights [rays,S], g_rgb [rays,3], g_depth [rays] (each may be NULL) the gradients
 * w.r.t. the weights, the composited colour and the depth before render_depth's clip.  Writes g_sigma [rays,S] and (when not
 * NULL) g_color [rays,S,3].  One wave per ray, fixed summation order (bit-reproducible). */
int njf_composite_backward(const float* deltas, const float* steps, const float* sigma, const float* color,
                           const float* g_weights, const float* g_rgb, const float* g_depth, int rays, int samples,
                           float* g_sigma, float* g_color, void* stream);

/* ---- training: backward of the pixel-aligned bilinear sampling -------------------------------- */
/* Input gradient of F.grid_sample(bilinear, border, align_corners=True) as get_pixel_aligned_features uses it
 * (model_components/pixel_aligned_features.py:29-33), in hoisted order: grad [P,channels] is the gradient w.r.t. the
 * sampled (already lin_z-projected) latent of every point, foot_idx [P,4] (int32 texel index on the flattened
 * [B*Hf*Wf] grid) / foot_w [P,4] the bilinear footprint the training forward dumped (NjfActivationDump).
 * out [texels,channels] += sum over points and footprint corners (accumulates: zero it first for a fresh gradient).
 * run_length >= 1: points p*run_length .. (p+1)*run_length-1 are handled by one thread per channel, which merges
 * consecutive contributions to the same texel before touching memory -- pass the samples per ray (points are ordered
 * ray-major, neighbouring samples mostly share texels); 1 = no merging.  The result does not depend on it beyond
 * rounding.  fp32 hardware atomics: the summation order, hence the last bits, vary from run to run (as they do for
 * ATen's grid_sampler_2d_backward on a GPU).
 * `slices` >= 1 gradients of the same points are scattered in one launch: slice s is read at grad + s * slice_stride
 * ([P,channels] each; the three lin_z latents of a ResnetFC are deltas[0], [2], [4] of njf_resnetfc_backward, i.e.
 * slice_stride = 2*P*128) and lands in columns [s*channels, (s+1)*channels) of out [texels, slices*channels]
 * (slices > 1 needs channels % 64 == 0). */
int njf_scatter_footprint(const float* grad, int slices, long long slice_stride, const int* foot_idx, const float* foot_w,
                          int points, int channels, int texels, int run_length, float* out, void* stream);

/* The whole data-gradient chain of one ResnetFC's backward pass in one launch: what autograd runs as 11 x (GEMM with the
 * transposed weight + ReLU mask + residual add) for model_components/resnet_fc.py:69-79,130-154.  `w_backward`
 * [NJF_RESNET_BACKWARD_CHUNKS * NJF_CHUNK_FLOATS] comes from njf_pack_resnetfc_backward (transposed weights, re-packed
 * after every optimiser step); `activations` [11,P,128] are the ReLU'd layer inputs the training forward dumped
 * (NjfActivationDump.act / NjfRenderOutputs.jac_act / den_act); `d_out` [P,d_out_dim] is the gradient w.r.t. lin_out's
 * output.  Writes `deltas` [11,P,128]: deltas[l+1] is the gradient w.r.t. the OUTPUT of the layer whose input is
 * activations[l] (l = 0..9), so that layer's weight gradient is deltas[l+1]^T activations[l] and its bias gradient the
 * column sum of deltas[l+1]; deltas[0], deltas[2], deltas[4] are the gradients w.r.t. the three hoisted latents
 * (lin_z outputs) and deltas[0] also w.r.t. lin_in's output.  Exact-fp32 MFMA.
 * `colsum_partial` (may be NULL) [ceil(P / 32), 11, 128]: per 32-point tile, the column sums of every deltas slice (the
 * bias gradients are their sum over the tiles: 32x less data than re-reading deltas; fixed summation order inside a
 * tile).
 * `masks` (ABI v17, may be NULL) [11,P,4]: the ReLU masks the same training forward dumped next to the activations
 * (NjfActivationDump.mask / NjfRenderOutputs.jac_mask / den_mask).  The chain needs only the SIGN of activations[l]; with `masks`
 * it does not read `activations` at all (which may then be NULL): 16 instead of 512 bytes per point and layer.
 * `precision` (ABI v17, of BOTH entry points: the blob is packed for it): NJF_PRECISION_F32 -- exact fp32 products, the default of
 * the host side -- or NJF_PRECISION_F16X2: hi*hi + hi*lo + lo*hi of fp16 halves (fp32-class: 2^-22 per product) on gradients the
 * kernel scales by a power of two taken from `d_out_absmax` (device scalar max|d_out|, required then) and scales back on the way
 * out.  (The reference trains on TF32 products, train.py:64-65.)
 * `deltas16` (ABI v17, may be NULL; needs `masks` and `d_out_absmax`): 16-bit training storage -- [11,P,128] HALVES receive
 * deltas x 2^k, k = 6 - exponent(max|d_out|) (the caller divides the weight-gradient products by 2^k), and `deltas` is then a
 * compact [3,P,128] fp32 array that receives slices 0, 2, 4 only (the latent gradients njf_scatter_footprint reads). */
#define NJF_RESNET_BACKWARD_CHUNKS 21
int njf_pack_resnetfc_backward(const NjfResnetFcWeights* src, float* w_out, int precision, void* stream);
int njf_resnetfc_backward(const float* d_out, int d_out_dim, const float* activations, const float* w_backward, int points,
                          float* deltas, float* colsum_partial, const unsigned* masks, int precision,
                          const float* d_out_absmax, void* deltas16, void* stream);

/* The data-gradient chain of the folded Jacobian transformer head (ActionDecoderJacobianTransformer.compute_jacobian,
 * action_decoder_jacobian.py:418-446 with model_components/transformer.py:38-135, as njf_render_forward evaluates it: decoder.py
 * folds keys / values / LayerNorm affines into 64 x 64 matrices) in one launch, exact fp32 MFMA -- what autograd runs for the
 * reference's parameterisation of the head.  Per layer l: n = norm(x), a = softmax_8(Mqk n + bqk), xm = x + Nov a + bo,
 * n2 = norm(xm), u = W1' n2 + b1', h = gelu(u), x_next = xm + W2 h + b2.
 * x [4,P,64]: the residual stream in front of layers 0, 1, 2 and behind layer 2 -- NjfRenderOutputs.jac_act of an action-mode
 * training forward with NJF_JACOBIAN_TRANSFORMER (slice 3 is not read here: the caller contracts it with d_out for the output
 * Linear's gradient).  d_out [P,d_out_dim]: gradient w.r.t. the head's 3A outputs.  keys = A (valid key slots per head).
 * Outputs: wg_x, wg_dy [12,P,64] -- per layer l the pairs the weight gradients contract over the points, at 4l + (0, 1, 2, 3) for
 * (Mqk, Nov, W1', W2): X = (n, a, n2, h), dY = (d dots, d xm, d u, d x_next); dW = dY^T X (K = points: library GEMM on the host),
 * bias gradients = column sums of dY (colsum_partial, may be NULL: [ceil(P / 32), 12, 64] per-tile sums, to be added over the
 * tiles).  half_storage != 0 (16-bit training storage, as `deltas16` of njf_resnetfc_backward): wg_x / wg_dy address [12,P,64]
 * HALVES, the dY stored x 2^k with k = 6 - exponent(*d_out_absmax) (device scalar max|d_out|, required then).  dx0 [P,64]: gradient w.r.t. the head's input (the query MLP's output): its weight gradient
 * contracts with the positional encoding, its hoisted feature part goes through njf_scatter_footprint.
 * njf_pack_transformer_backward: mats [3,4,64,64] = (Mqk, Nov, W1', W2) per layer, row-major [out][in]; biases [3,3,64] = (bqk, bo,
 * b1'); head_w [d_out,64]; -> w_out (NJF_TRANSFORMER_BACKWARD_CHUNKS chunks), b_out [3,192].
 * precision (ABI v19, both entry points, the same value): NJF_PRECISION_F32 -- exact fp32 MFMA -- or NJF_PRECISION_F16X2: split fp16
 * products (hi*hi + hi*lo + lo*hi, fp32-class inside fp16's range) for the layer's re-evaluation and for the chain, which then runs on
 * d_out x 2^k (d_out_absmax required) and scales its fp32 results back; the opt-in TF32-class form of njf_resnetfc_backward, for
 * callers whose reference trains on TF32 products (train.py:64-65). */
#define NJF_TRANSFORMER_BACKWARD_CHUNKS 13
int njf_pack_transformer_backward(const float* mats, const float* biases, const float* head_w, int d_out, float* w_out,
                                  float* b_out, int precision, void* stream);
int njf_transformer_backward(const float* x, const float* d_out, int d_out_dim, int keys, int points, const float* w_backward,
                             const float* b_backward, float* wg_x, float* wg_dy, float* dx0, float* colsum_partial,
                             int half_storage, const float* d_out_absmax, int precision, void* stream);

/* One layer step of the ResnetFC backward chain (model_components/resnet_fc.py:69-79,130-154 differentiated; what
 * autograd runs as compare + multiply + add + sum kernels):  out [P,C] = residual + upstream * [act > 0], with act the
 * ReLU'd forward activation the training forward dumped (residual may be NULL), and the bias gradient of the layer below
 * as column sums of out: partial_colsum [ceil(P / rows_per_block), C] receives one deterministic partial row per
 * workgroup (the caller adds the rows; NULL = no sums).  C % 4 == 0 and C/4 must divide 256 (C = 64, 128, ...). */
int njf_relu_backward(const float* upstream, const float* act, const float* residual, int points, int channels,
                      int rows_per_block, float* out, float* partial_colsum, void* stream);

/* Epilogue of a convolution of the frozen encoder trunk in eval mode (models/encoder/encoder_resnet.py:24-89: the torchvision
 * BasicBlock's  relu(bn(conv(x)))  and  relu(bn(conv(y)) + skip)  with batch norm on its running statistics; ABI v20):
 * out = [relu]( (x - running_mean[c]) / sqrt(running_var[c] + eps) * gamma[c] + beta[c] [+ skip] ), x / skip / out [batch, channels,
 * hw] fp32 NCHW (out may alias x; skip may be NULL), one launch instead of the library's batch-norm + add + ReLU kernels. */
int njf_bn_act(const float* x, const float* gamma, const float* beta, const float* running_mean, const float* running_var,
               float eps, const float* skip, int relu, int batch, int channels, int hw, float* out, void* stream);

/* ---- inverse dynamics on the composited Jacobian field ---------------------------------------- */
/* The control loop of notebooks/real_world/2_inverse_dynamics.ipynb (cells 26-29: 100 Adam steps through
 * Model.infer_optical_flow, model.py:497-525) as a least-squares problem: optical_flow(a) = proj(x + M a) - proj(x),
 * x = mean_position [B,R,3] and M = jacobian [B,R,3,A] being the composited outputs of njf_render_forward (pos,
 * action_features re-ordered spatial-major), projection [B,3,4] = K . inv(E)[:3] of the target camera.  Runs
 * `iterations` Levenberg-Marquardt steps on sum_r mask_r |flow_r(a) - target_flow_r|^2 inside one launch (one
 * workgroup per batch element, deterministic reductions) and writes the command to action [B,A].
 * visible_mask [B,R] and init_action [B,A] may be NULL (all rays, start from zero).  A <= 16. */
int njf_solve_action(const float* mean_position, const float* jacobian, const float* projection, const float* target_flow,
                     const float* visible_mask, const float* init_action, int batch, int rays, int action_dim,
                     int iterations, float damping, float* action, void* stream);

/* The notebook's own objective (2_inverse_dynamics.ipynb: smooth_l1_loss(pred_flow, target_flow) + reg * a.pow(2).mean(),
 * Adam; inference/action.py::optimize_actions: the same with mse_loss), with joint limits and several cameras per
 * command.  B = G * views linearisations, each run of `views` consecutive batch elements sharing one command (G commands;
 * batch % views == 0).  mean_position, jacobian, projection, target_flow and visible_mask keep njf_solve_action's layout;
 * init_action, lower and upper are [G,A] (each may be NULL: zero start / unbounded).  Per command
 *   L(a) = (1/N) sum_i m_i rho(r_i(a)) + (reg/A) sum_k a_k^2,  N = 2 sum_r m_r  (mask weights m_r >= 0),
 * r_i the two flow components of every ray of every view of the command, rho = r^2 (loss NJF_LOSS_MSE) or torch's
 * smooth-L1 with `beta` (NJF_LOSS_SMOOTH_L1), minimised over lower <= a <= upper by `iterations` projected IRLS
 * Levenberg-Marquardt steps in ONE launch (one workgroup per command, deterministic reductions, capture-safe); a step
 * is kept only if L drops.  The start is clamped into the box; a command with no observed ray returns it.  A <= 16;
 * beta <= 0, reg < 0 or damping < 0 return NJF_E_VALUE (lower <= upper is the caller's to check: it lives on the
 * device).  Writes action [G,A]. */
#define NJF_LOSS_MSE 0
#define NJF_LOSS_SMOOTH_L1 1
int njf_solve_action_robust(const float* mean_position, const float* jacobian, const float* projection,
                            const float* target_flow, const float* visible_mask, const float* init_action,
                            const float* lower, const float* upper, int batch, int views, int rays, int action_dim,
                            int loss, float beta, float reg, int iterations, float damping, float* action, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NJF_HIP_H */
