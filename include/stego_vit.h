/*
 * stego_vit.h - C ABI of the frozen DINO ViT backbone forward (the step right before the
 * correspondence-loss hot path), exported by the same libstego_corr.so.
 *
 * Replaces, for inference on a frozen backbone:
 *   src/dino/vision_transformer.py:225-237  VisionTransformer.get_intermediate_feat(x, n=1)  (feat only)
 *   src/dino/vision_transformer.py:195-205  prepare_tokens  (patch embed conv :123-133, cls token, pos embed)
 *   src/dino/vision_transformer.py:69-130   Attention / Mlp / Block  (qkv bias, softmax(QK^T/sqrt(d))V, proj, GELU MLP)
 * as called by DinoFeaturizer.forward (src/modules.py:83-107) and precompute_knns.get_feats (:15-21).
 *
 * Arithmetic: residual stream, LayerNorm statistics, softmax statistics and every accumulation are fp32; GEMM and
 * attention operands go to the fp16 matrix cores - in precision STEGO_VIT_F16X3 as hi + lo pairs with three MFMAs per product
 * (x = hi + lo to 2^-22: the fp32 class the reference's fp32 torch model computes in, and what the loss kernels and the
 * segmentation head of this library use), in STEGO_VIT_F16 as plain fp16 operands (2 - 3 x faster, error at the level of
 * torch's fp16 autocast).  Measured deviations from the fp32 / fp64 torch model: DESIGN.md 4.9 / tests/test_vit_native.py.
 * The attention maps and the qkv tensor the reference materialises at every block (:232-236) are never built; the keys of the last
 * block, the reference's feature type "KK", come from stego_vit_forward_keys, and the one row of the last block's attention maps that
 * outlines the foreground - the class token's - from stego_vit_forward_attn; stego_attn_salience makes a mask of it.
 *
 * Conventions as in stego_corr.h: device pointers, nothing allocated / freed / synchronised, work enqueued on
 * `stream`, return STEGO_OK or an error code.
 */
#ifndef STEGO_VIT_H
#define STEGO_VIT_H

#include "stego_corr.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct StegoVitDesc {
    int32_t B;        /* images per call                                                     */
    int32_t H, W;     /* image size, multiples of `patch`                                    */
    int32_t patch;    /* 8 or 16                     (vision_transformer.py:123-133)         */
    int32_t D;        /* embed dim: any multiple of 64 up to 768 (192 / 384 / 768 are        */
                      /* vit_tiny/small/base; the others end in a partial column tile)       */
    int32_t depth;    /* blocks                                                              */
    int32_t heads;    /* D / heads must be 64                                                */
    int32_t hidden;   /* MLP hidden width: any multiple of 64 (4 * D in the DINO models)     */
    int32_t precision;/* STEGO_VIT_F16 | STEGO_VIT_F16X3 (ABI 6); weights packed for one precision   */
                      /* are read by forwards of the same precision only                            */
} StegoVitDesc;

enum { STEGO_VIT_F16 = 0, STEGO_VIT_F16X3 = 1 };

/* Number of fp32 parameter tensors stego_vit_pack_weights() takes: 4 + 12 * depth + 2, in this order
 *   patch_embed.proj.weight [D, 3*patch*patch]   patch_embed.proj.bias [D]   cls_token [D]
 *   pos_embed [1 + (H/patch)*(W/patch), D]   (already interpolated to this H, W: vision_transformer.py:171-193)
 *   per block: norm1.weight, norm1.bias, attn.qkv.weight [3D, D], attn.qkv.bias [3D], attn.proj.weight [D, D],
 *              attn.proj.bias, norm2.weight, norm2.bias, mlp.fc1.weight [hidden, D], mlp.fc1.bias,
 *              mlp.fc2.weight [D, hidden], mlp.fc2.bias
 *   norm.weight, norm.bias
 * all contiguous fp32 on the device (the layouts of the DINO checkpoints / nn.Linear). */
int32_t stego_vit_param_count(const StegoVitDesc* d);

/* Packs the weights once into the layout the kernels read (fp16 operand panels + fp32 vectors). */
size_t stego_vit_weights_bytes(const StegoVitDesc* d);
int stego_vit_pack_weights(const StegoVitDesc* d, const float* const* params, int32_t n_params, void* packed,
                           size_t packed_bytes, stego_stream_t stream);

/* tokens_out: OUT fp32 [B, 1 + hw, D] = norm(x) after the last block (the `feat[0]` of get_intermediate_feat(n=1));
 * row 0 of every image is the class token (DinoFeaturizer return_class_feat), rows 1.. are the patch tokens, i.e.
 * tokens_out[:, 1:, :] viewed as [B, h, w, D] is the channels-last feature map the loss kernels read directly.
 * img: fp32 [B, 3, H, W] contiguous. */
size_t stego_vit_workspace_bytes(const StegoVitDesc* d);
int stego_vit_forward(const StegoVitDesc* d, const void* packed, const float* img, float* tokens_out, void* workspace,
                      size_t workspace_bytes, stego_stream_t stream);

/* The attention keys of the LAST block instead of the normalised tokens: the reference's other feature type,
 *   src/modules.py:98-101                    DinoFeaturizer.forward, feat_type == "KK": qkv[1, :, :, 1:, :] -> [B, heads * 64, h, w]
 *   src/dino/vision_transformer.py:78-81     Attention.forward: qkv = self.qkv(x).reshape(B, N, 3, heads, C // heads).permute(2, 0, 3, 1, 4)
 *   src/dino/vision_transformer.py:232-236   get_intermediate_feat: the qkv tensor of the block (only its K third is computed here)
 * keys_out: OUT fp32 [B, 1 + hw, D], row t of image b = LN1(x) . W_qkv[D:2D]^T + b_qkv[D:2D] of token t in block depth-1, channel
 * head * 64 + d = qkv[1][b, head, t, d].  Row 0 is the class token's key; keys_out[:, 1:, :] viewed as [B, h, w, D] is the channels-last
 * key map - same shape and row order as tokens_out, so everything downstream of the tokens takes it unchanged.  (The reference
 * hard-codes 6 heads at modules.py:99; the channel order here is that of the model's own head count, the same thing for ViT-S.)
 * Same descriptor, same packed weights, same stego_vit_workspace_bytes, same argument checks in the same order as stego_vit_forward.
 * Runs prepare_tokens and blocks 0 .. depth-2 as stego_vit_forward does, then LN1 and the K columns of the QKV GEMM of block depth-1
 * and nothing else (no Q / V columns, attention, proj, MLP or final norm; depth == 1 is legal).  The keys leave the GEMM's fp32
 * accumulators directly: F16X3 keys are fp32 class, F16 keys carry the operand rounding only. */
int stego_vit_forward_keys(const StegoVitDesc* d, const void* packed, const float* img, float* keys_out, void* workspace,
                           size_t workspace_bytes, stego_stream_t stream);

/* tokens_out exactly as stego_vit_forward (same launches, same bits), and in addition
 * attn_out: OUT fp32 [B, heads, 1 + hw]: softmax_t(q_cls . k_t / 8) of block depth-1,
 * i.e. attn[:, :, 0, :] of vision_transformer.py:83-85 / get_last_selfattention (:239-246).
 * Column 0 is the class token's own weight; each row sums to 1 over the 1 + hw real tokens.
 * One more launch after those of stego_vit_forward: a read-only pass over the Q and K the last block's QKV GEMM left in the workspace
 * (one workgroup per image and head; F16X3: q = hi + lo and k = hi + lo in fp32 FMAs, F16: the fp16 operands; fp32 statistics).  The
 * entry point is combined on purpose: the workspace holds that Q and K only right after a stego_vit_forward of the same batch
 * (stego_vit_forward_keys stops before the last QKV GEMM).  Argument checks as stego_vit_forward, attn_out: non-NULL, 4-byte aligned. */
int stego_vit_forward_attn(const StegoVitDesc* d, const void* packed, const float* img, float* tokens_out, float* attn_out, void* workspace,
                           size_t workspace_bytes, stego_stream_t stream);

/* An attention salience mask per image: the smallest set of strongest patches that holds `keep` of the class token's attention mass.
 * attn: [B, heads, 1 + h*w] as above.  Per image, in fp64 from the fp32 inputs:
 *   m_i     = sum over heads (head order) of attn[b, hd, 1 + i]          i = 0 .. h*w-1 (class column left out)
 *   T       = sum_i m_i (index order)
 *   ahead_i = sum of m_j over the patches that come before i in the order (m descending, index ascending on ties)
 *   kept_i  = ahead_i < (double)keep * T        (the smallest set of strongest patches holding >= keep of the mass)
 * soft: OUT fp32 [B, h, w] = m_i / T, may be NULL.
 * mask: OUT uint8 [B, h*patch, w*patch], kept_i replicated over its patch (0 / 1), may be NULL; 16-byte aligned.
 * 0 < keep <= 1.
 * The kernel (a workgroup per image and slice of patch rows) needs no sort: ahead_i is accumulated in increasing j over the j with
 * m_j > m_i, or equal and j < i; T by a tree.  Both differ from the sums in the stated order by fp64 rounding only (1e-16 relative), so kept_i is the stated one
 * wherever |ahead_i - keep * T| / T is above that.
 * Errors, all before the first HIP call: STEGO_ERR_NULL (attn), STEGO_ERR_SHAPE (B, heads, h, w <= 0; keep outside (0, 1]),
 * STEGO_ERR_UNSUPPORTED (patch not 8 or 16; h*w > 4096 - 512 x 512 pixels at patch 8), STEGO_ERR_ALIGN.                                 */
int stego_attn_salience(const float* attn, int32_t B, int32_t heads, int32_t h, int32_t w, int32_t patch, float keep,
                        float* soft, uint8_t* mask, stego_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* STEGO_VIT_H */
