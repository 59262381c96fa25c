/*
 * stego_stats.h - C ABI of the device-side step statistics of STEGO's training loop, exported by the same libstego_corr.so.
 *
 * Replaces what the reference's training_step does for its TensorBoard log (train_segmentation.py:144-146, :165-168, :172-177): the three
 * cd.mean() launches of every step and, on histogram steps, three .cpu() copies with np.histogram over TensorBoard's default bins.  One
 * launch per step reads up to four float32 tensors once and writes a fixed-size RECORD into a RING in device memory: per tensor the
 * counts, the extremes, the fp64 sum and sum of squares and (when asked to) the 1548 bucket counts, and beside them up to 16 float32
 * scalars copied from device pointers.  The host drains the ring with one copy whenever it likes and never waits in between.
 *
 * Buckets: TensorBoard's default limits (torch/utils/tensorboard/writer.py: v = 1e-12; while v < 1e20: v *= 1.1; mirrored, 0 in the
 * middle): STEGO_STATS_LIMITS = 774 + 1 + 774 doubles.  Bucket i is [limit[i], limit[i + 1]), which is how np.histogram(x, bins=limits)
 * counts float32 data: no float32 equals the last limit, so numpy's closed last bucket changes nothing.  A float32 x satisfies
 * x >= limit[i] exactly when x >= threshold[i], the smallest float32 not below limit[i]; the kernel compares the ordered integer images of
 * x and of the thresholds, so nothing depends on the denormal mode and the counts equal numpy's exactly.  -0.0 and +0.0 are in bucket 774,
 * a negative denormal in bucket 773.
 *
 * Per tensor the record holds
 *     n_finite   values that are neither NaN nor +-inf
 *     n_nan      NaNs
 *     n_out      values no bucket holds: +-inf and finite values below limit[0] or not below limit[1548] (numpy drops them, and the NaNs)
 *     min, max   over the finite values, float32 (+inf / -inf when there is none; a zero extreme is reported as +0.0)
 *     sum, sum_sq  over the finite values in fp64; every square is formed in fp64 and is exact
 *     counts     uint32 [STEGO_STATS_BUCKETS], written only by a call with with_hist = 1 (otherwise the bytes keep what they held)
 * so that n_finite + n_nan + (number of infinities) is the tensor's count and the counts add up to count - n_nan - n_out.
 *
 * The step counter lives in `state` ({int64 step, uint32 ticket, uint32 0}; the caller zeroes it once): a call reads it, fills slot
 * step % ring_slots and the workgroup that draws the last ticket advances it, the scheme of stego_adam_step.  The launch arguments of
 * consecutive steps are identical, so a call can be captured into a graph and replayed.  Two calls on the same state must not run at
 * the same time; a launch that did not run to its end leaves ticket and workspace dirty.
 *
 * Determinism: integer counts are added with atomics (integer adds commute); sum and sum_sq go thread -> workgroup -> per-workgroup
 * partial in `workspace` -> one fold by the last workgroup, every stage in a fixed order, so two runs on the same inputs give the same
 * bytes.  The bucket counts of a launch are gathered in the workspace and moved into the slot by the last workgroup, which leaves the
 * workspace zeroed again: a slot needs no clearing and a call is ONE launch with no memset.  The caller zeroes `workspace` once.
 *
 * Conventions as in stego_optim.h: device pointers, nothing allocated / freed / synchronised, work enqueued on `stream`, STEGO_OK or
 * an error code; every check is on the host, before anything is enqueued.
 */
#ifndef STEGO_STATS_H
#define STEGO_STATS_H

#include "stego_corr.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
    STEGO_ERR_STATS_COUNT = 160,    /* n_tensors outside [1, STEGO_STATS_MAX_TENSORS], n_scalars outside [0, STEGO_STATS_MAX_SCALARS], or
                                       a tensor's count outside [0, STEGO_STATS_MAX_ELEMS)                                            */
    STEGO_ERR_STATS_RING = 161,     /* ring_slots outside [1, STEGO_STATS_MAX_SLOTS]                                                  */
    STEGO_ERR_STATS_FLAGS = 162     /* with_hist neither 0 nor 1                                                                      */
};

#define STEGO_STATS_MAX_TENSORS 4
#define STEGO_STATS_MAX_SCALARS 16
#define STEGO_STATS_MAX_ELEMS (1ll << 31)      /* a tensor's count stays below this: a bucket's uint32 holds a whole tensor */
#define STEGO_STATS_MAX_SLOTS 65536
#define STEGO_STATS_BUCKETS 1548
#define STEGO_STATS_LIMITS 1549
#define STEGO_STATS_CHUNK 4096                 /* elements one workgroup reads at a time                                    */
#define STEGO_STATS_MAX_GRID 1024              /* workgroups of a launch; beyond it a workgroup takes several chunks        */

typedef struct StegoStatsDesc {
    int32_t n_tensors;                              /* 1 .. STEGO_STATS_MAX_TENSORS                                       */
    int32_t n_scalars;                              /* 0 .. STEGO_STATS_MAX_SCALARS                                       */
    int32_t with_hist;                              /* 1: this call also counts the buckets                               */
    int32_t ring_slots;                             /* records the ring holds (>= 1)                                      */
    int64_t counts[STEGO_STATS_MAX_TENSORS];        /* elements of each tensor (0 is allowed); beyond n_tensors: ignored  */
} StegoStatsDesc;

/* What stego_step_stats_plan reports.  Offsets are in bytes: off_* from the start of a record, t_* from the start of a tensor's block
 * (tensor i's block begins at off_tensors + i * tensor_stride, its bucket counts at off_hist + i * hist_stride). */
typedef struct StegoStatsPlan {
    int64_t grid;                /* workgroups of the launch                                                               */
    int64_t chunk;               /* elements a workgroup takes at a time: workgroup b reads chunks b, b + grid, ... of every tensor */
    int64_t record_bytes;        /* size of a record (a multiple of 16); the ring is ring_slots records                    */
    int64_t off_step;            /* int64: the step number                                                                 */
    int64_t off_with_hist;       /* int32: the call's with_hist                                                            */
    int64_t off_n_tensors;       /* int32: the call's n_tensors                                                            */
    int64_t off_tensors, tensor_stride;
    int64_t t_n_finite, t_n_nan, t_n_out;          /* int64 each                                                           */
    int64_t t_sum, t_sum_sq;                       /* double each                                                          */
    int64_t t_min, t_max;                          /* float each                                                           */
    int64_t off_scalars;         /* float32 [n_scalars], bit copies                                                        */
    int64_t off_hist, hist_stride;                 /* uint32 [STEGO_STATS_BUCKETS] per tensor                              */
    int64_t ring_bytes;          /* ring_slots * record_bytes                                                              */
    int64_t state_bytes;         /* 16                                                                                     */
    int64_t workspace_bytes;     /* does not depend on the descriptor                                                      */
} StegoStatsPlan;

/* One record into slot step % ring_slots, in one kernel launch.
 *   tensors   : HOST array of n_tensors device pointers to contiguous float32, 4-byte aligned (a view at any element offset will do);
 *               an entry whose count is 0 may be NULL
 *   scalars   : HOST array of n_scalars device pointers to one float32 each (may be NULL when n_scalars is 0)
 *   ring      : ring_slots records in device memory, 8-byte aligned; needs no initialisation
 *   state     : 16 bytes, 8-byte aligned, zeroed once by the caller
 *   workspace : workspace_bytes, 8-byte aligned, zeroed once by the caller
 * Returns STEGO_ERR_NULL (desc, tensors, ring, state, workspace; scalars when n_scalars > 0), STEGO_ERR_STATS_COUNT,
 * STEGO_ERR_STATS_RING, STEGO_ERR_STATS_FLAGS, STEGO_ERR_NULL (a tensor pointer with count > 0, a scalar pointer), STEGO_ERR_ALIGN (ring,
 * state or workspace not 8-byte aligned, a tensor or scalar pointer not 4-byte aligned), in this order. */
int stego_step_stats(const StegoStatsDesc* desc, const float* const* tensors, const float* const* scalars, void* ring, void* state,
                     void* workspace, stego_stream_t stream);

/* Host only: the launch and the record layout of this descriptor.  Returns what stego_step_stats's descriptor checks return
 * (STEGO_ERR_NULL, _STATS_COUNT, _STATS_RING, _STATS_FLAGS) and writes nothing then. */
int stego_step_stats_plan(const StegoStatsDesc* desc, StegoStatsPlan* plan);

/* Host only: the STEGO_STATS_LIMITS bucket limits and the float32 thresholds the kernel compares with (either may be NULL). */
int stego_step_stats_edges(double* limits, float* thresholds);

#ifdef __cplusplus
}
#endif

#endif
