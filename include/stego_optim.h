/*
 * stego_optim.h - C ABI of the fused Adam step of STEGO's training loop, exported by the same libstego_corr.so.
 *
 * Replaces the parameter update of the reference's training_step (train_segmentation.py:117-119, the three torch.optim.Adam of
 * configure_optimizers; :228-230, their three step() calls; :373-383, the two fresh Adams of the probe reset) and the zero_grad()
 * calls that open the next step: one launch updates every trainable tensor of every optimizer, advances the step counters that live
 * on the device and, when asked to, leaves the gradient buffer zeroed for the next backward.
 *
 * Plain Adam (no weight decay, no amsgrad, no maximize), per element in fp32:
 *     m += (1 - beta1) * (g - m)
 *     v  = beta2 * v + (1 - beta2) * g * g
 *     p -= (lr / bc1) * (m / (sqrt(v) / sqrt(bc2) + eps))          bc1 = 1 - beta1^t, bc2 = 1 - beta2^t, t = steps[group] + 1
 * The two bias corrections, lr / bc1 and sqrt(bc2) are computed on the device in double precision from the counter the kernel reads,
 * then rounded to fp32 once.  This is what torch.optim.Adam computes; the results agree with it to rounding, not bit for bit.
 *
 * A SEGMENT is one parameter tensor: its contiguous fp32 data stays where nn.Module put it, its gradient and its two moments are
 * slices of three flat buffers.  A GROUP is one logical optimizer: lr, betas and eps by value in the descriptor and one int32 step
 * counter on the device.  The caller keeps the segment table twice: on the host, where every check of a call reads it, and in device
 * memory, where the kernel reads it; the two must hold the same records.
 *
 * The counters: the kernel reads steps[g] and uses t = steps[g] + 1.  Every workgroup draws a ticket after its last chunk; the one
 * that draws the last ticket writes t back for every active group and sets the ticket word to 0 again, so no workgroup of the launch
 * can see an incremented counter and a call is one launch.  `ticket` is one uint32 the caller zeroes once, before the first call; a
 * launch that did not run to its end leaves it dirty.  Two calls on the same counters must not run at the same time.
 *
 * Alignment: the four addresses of a segment (parameter, gradient, exp_avg, exp_avg_sq) need 4-byte alignment only.  A chunk whose
 * four addresses are all 16-byte aligned moves 16 bytes per lane and finishes its last count % 4 elements one by one; any other
 * chunk moves 4 bytes per lane.
 *
 * Conventions as in stego_probe.h: device pointers, nothing allocated / freed / synchronised, work enqueued on `stream`, STEGO_OK or
 * an error code; every check is on the host, before anything is enqueued.
 */
#ifndef STEGO_OPTIM_H
#define STEGO_OPTIM_H

#include "stego_corr.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
    STEGO_ERR_OPTIM_COUNT = 110,    /* n_segments outside [1, STEGO_ADAM_MAX_SEGMENTS], n_groups outside [1, STEGO_ADAM_MAX_GROUPS], or
                                       STEGO_ADAM_MAX_ELEMS elements or more in all                                                   */
    STEGO_ERR_OPTIM_SEGMENT = 111,  /* a segment with count < 1, a group index outside [0, n_groups), or a gradient / state slice
                                       outside [0, grad_elems) / [0, state_elems)                                                    */
    STEGO_ERR_OPTIM_PARAM = 112,    /* a group's beta1 or beta2 outside [0, 1), or its lr or eps negative or not finite              */
    STEGO_ERR_OPTIM_FLAGS = 113     /* zero_grads or a group's `active` neither 0 nor 1, or no active group                          */
};

#define STEGO_ADAM_MAX_SEGMENTS 256            /* parameter tensors per call (the kernel scans the table once per chunk) */
#define STEGO_ADAM_MAX_GROUPS 8                /* logical optimizers per call (the trainer has 3)                         */
#define STEGO_ADAM_MAX_ELEMS (1ll << 31)       /* the counts of all segments together stay below this                    */
#define STEGO_ADAM_CHUNK 1024                  /* elements one workgroup updates at a time                               */
#define STEGO_ADAM_MAX_GRID 2048               /* workgroups of a launch; beyond it a workgroup takes several chunks     */

/* One record of the segment table (40 bytes; the same layout on the host and in device memory). */
typedef struct StegoAdamSegment {
    void* param;                 /* device pointer: `count` contiguous float32, 4-byte aligned, updated in place       */
    int64_t count;               /* elements (>= 1)                                                                    */
    int64_t grad_offset;         /* element offset of the gradient in `grads`                                          */
    int64_t state_offset;        /* element offset of both moments in `exp_avg` and `exp_avg_sq`                       */
    int32_t group;               /* index into desc->groups and `steps`                                                */
    int32_t reserved;            /* 0                                                                                  */
} StegoAdamSegment;

typedef struct StegoAdamGroup {
    double lr, beta1, beta2, eps;    /* as torch.optim.Adam holds them (Python floats)                                 */
    int32_t active;                  /* 1: this call steps the group; 0: its segments and its counter are left alone   */
    int32_t reserved;                /* 0                                                                              */
} StegoAdamGroup;

typedef struct StegoAdamDesc {
    int32_t n_segments;          /* records of the table (1 .. STEGO_ADAM_MAX_SEGMENTS)                                */
    int32_t n_groups;            /* groups in use (1 .. STEGO_ADAM_MAX_GROUPS)                                         */
    int32_t zero_grads;          /* 1: every gradient element of an active group is overwritten with 0 after it is read */
    int32_t reserved;            /* 0                                                                                  */
    int64_t grad_elems;          /* floats in `grads`                                                                  */
    int64_t state_elems;         /* floats in `exp_avg` and in `exp_avg_sq`                                            */
    StegoAdamGroup groups[STEGO_ADAM_MAX_GROUPS];
} StegoAdamDesc;

/* One Adam step of every segment of every active group, in one kernel launch.
 *   segments_host : the table in host memory: n_segments records (read by the checks, never by the device)
 *   segments      : the same records in device memory, 8-byte aligned
 *   grads         : float32 [grad_elems]; read, and zeroed where desc->zero_grads says so
 *   exp_avg, exp_avg_sq : float32 [state_elems], updated in place
 *   steps         : int32 [n_groups]: steps taken so far; an active group's goes up by one (it stops at 2^31 - 1)
 *   ticket        : uint32 [1], 0 before the first call (see above)
 * Slices of different segments must not overlap (not checked).
 * Returns STEGO_ERR_NULL (desc, a table, a buffer, steps, ticket, a segment's param), STEGO_ERR_OPTIM_COUNT, STEGO_ERR_OPTIM_FLAGS,
 * STEGO_ERR_OPTIM_PARAM (active groups only), STEGO_ERR_OPTIM_SEGMENT, STEGO_ERR_ALIGN (a float pointer, steps or ticket not 4-byte
 * aligned, `segments` not 8-byte aligned), in this order. */
int stego_adam_step(const StegoAdamDesc* desc, const StegoAdamSegment* segments_host, const StegoAdamSegment* segments, float* grads,
                    float* exp_avg, float* exp_avg_sq, int32_t* steps, uint32_t* ticket, stego_stream_t stream);

/* Host only: the launch stego_adam_step would make for this table.  Chunk c (0 <= c < *n_chunks) is elements
 * [(c - first) * *chunk, min(count, (c - first + 1) * *chunk)) of the segment whose first chunk `first` is the number of chunks of the
 * segments before it, a segment having ceil(count / *chunk) chunks; workgroup b takes chunks b, b + *grid, ...  Reads the counts (and,
 * for the checks, the rest) of segments_host; touches no device.  Returns what stego_adam_step's descriptor and table checks return
 * (STEGO_ERR_NULL, _COUNT, _FLAGS, _PARAM, _SEGMENT) and writes nothing then. */
int stego_adam_plan(const StegoAdamDesc* desc, const StegoAdamSegment* segments_host, int32_t* grid, int32_t* chunk, int64_t* n_chunks);

#ifdef __cplusplus
}
#endif

#endif
