/*
 * dhd_amd_optim.h -- the tail of the training step as one operator of libdhd_amd.so: gradient unscaling, global-norm clipping,
 * AdamW, the weight EMA and the half weight copies in one sweep over the parameters.  Entry points of the same library, under the
 * conventions of dhd_amd.h (caller-owned [dev] memory, `stream` a hipStream_t as void*, 0 / positive hipError_t / negative DHD_E*
 * return codes, the DHD_F16 / DHD_BF16 dtype codes).
 *
 * Why a header, a prefix and a directory of its own: the reason dhd_amd_occ_train.h gives.  Every other surface of the library is
 * a closed list held by a table that lives in a test file, and so are the listings of the directories that hold the other
 * headers, so the family ships beside them as dhdw_*, with its own copies of the guarantees (tests/test_optim_capi.py,
 * tests/test_gpu_optim_step.py).  Compile with include/ on the include path.  Nothing here alters another header:
 * DHD_ABI_VERSION is unchanged by this header.
 */
#ifndef DHD_AMD_OPTIM_H
#define DHD_AMD_OPTIM_H

#include "dhd_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------ *
 * W1. The optimizer step.  Three launches over a table of chunks; a chunk is at most DHDW_OPTIM_CHUNK consecutive float32
 *     elements of ONE parameter tensor, dense in memory, with the same elements of its gradient and its two AdamW moments and,
 *     where present, of its EMA copy (float32) and its half copy (DHD_F16 or DHD_BF16), all in the same order.
 *
 *       dhdw_optim_grad_norm      partial[c] = sum over the chunk of (g * inv_scale)^2, inv_scale = 1 / *scale (1 without a scale)
 *       dhdw_optim_finalize       norm, found_inf, coef = min(1, max_norm / (norm + 1e-6)), mult = inv_scale * coef; per slot,
 *                                 unless found_inf: step += 1 and the scalars of that step; the dynamic loss-scale rule
 *       dhdw_optim_adamw_update   g' = g * mult;  p *= 1 - lr wd;  m += (g' - m)(1 - beta1);  v = v beta2 + (1 - beta2) g' g';
 *                                 p -= lr / (1 - beta1^step) * (m / (sqrt(v) / sqrt(1 - beta2^step) + eps));
 *                                 ema = ema * d + (1 - d) * p;  half = round(p)
 *
 *     float32 arithmetic, one rounding per operation (no contraction); the powers and the scalars derived from them in double,
 *     rounded once.  found_inf (any non-finite gradient): p, m, v and the step counts keep their bytes, the EMA advances with the
 *     unchanged p and half = round(p) is written again (the same bytes where the copy was current).  No atomics: the partials are added in index order, so two calls on the same bytes give
 *     the same bytes.  Every element of p, m, v, ema and half is read and written at most once, g is read once per launch.
 * ------------------------------------------------------------------------------------ */

#define DHDW_OPTIM_CHUNK 65536

/* One row of the chunk table [dev], 64 bytes.  Addresses are device addresses of the chunk's first element; ema, half: 0 =
 * absent.  The update takes 16-byte vectors where every address of the row is 16-byte aligned and single elements otherwise. */
typedef struct dhdw_optim_chunk {
  uint64_t p, g, exp_avg, exp_avg_sq, ema, half;
  int32_t len;        /* 1 .. DHDW_OPTIM_CHUNK */
  int32_t group;      /* row of the hyper-parameter table */
  int32_t half_dtype; /* DHD_F16 or DHD_BF16; ignored where half == 0 */
  int32_t slot;       /* the tensor the chunk belongs to: row of the step counts */
} dhdw_optim_chunk;

/* Per parameter group, written by the host: a row of the hyper-parameter table [dev], float64. */
typedef struct dhdw_optim_group {
  double lr, beta1, beta2, eps, weight_decay;
} dhdw_optim_group;

/* The caller's tables, all [dev] and all read on the device at run time, so that a captured launch follows them.
 *   chunks          n_chunks rows, 16-byte aligned
 *   groups          n_groups rows
 *   slot_group      int32 (n_slots): the group of each tensor; negative: the tensor takes no part in this step (no gradient)
 *   steps           float32 (n_slots): the step count of each tensor (torch.optim.AdamW's `step`), advanced by the finalize launch
 *   slot_scalars    float32 (n_slots, 4), written by the finalize launch, read by the update: 1 - lr wd, lr / (1 - beta1^step),
 *                   sqrt(1 - beta2^step), 0
 *   group_scalars   float32 (n_groups, 4), likewise: 1 - beta1, beta2, 1 - beta2, eps
 *   decay_pair      float32 (2) {d, 1 - d} of this update of the EMA; required where a chunk has an ema address
 *   scale           float32 (1) the loss scale, or NULL: no scale (inv_scale = 1, no scale rule)
 *   growth_tracker  int32 (1), given with scale
 *   workspace       dhdw_optim_workspace_bytes(n_partials) bytes, 16-byte aligned: the step record, then one float64 partial and
 *                   one int32 flag per chunk */
typedef struct dhdw_optim_tables {
  const dhdw_optim_chunk* chunks;
  const dhdw_optim_group* groups;
  const int32_t* slot_group;
  float* steps;
  float* slot_scalars;
  float* group_scalars;
  const float* decay_pair;
  float* scale;
  int32_t* growth_tracker;
  int32_t n_chunks, n_groups, n_slots;
  int32_t n_partials; /* >= n_chunks: partials and flags n_chunks .. n_partials - 1 are the caller's own (tensors it sweeps itself) */
} dhdw_optim_tables;

/* Byte offsets into the workspace: the step record float32 {norm, coef, found_inf, scale after the rule}, the gradient
 * multiplier float32, found_inf as int32; partials from DHDW_OPTIM_PARTIALS_AT, the flags behind the last partial. */
#define DHDW_OPTIM_RECORD_AT 0
#define DHDW_OPTIM_MULT_AT 16
#define DHDW_OPTIM_FOUND_AT 20
#define DHDW_OPTIM_PARTIALS_AT 64

/* Bytes of the workspace for n_partials partial sums (a multiple of 16); 0 for a negative count. */
size_t dhdw_optim_workspace_bytes(int n_chunks);

/* One workgroup per chunk: partial and flag of chunks 0 .. n_chunks - 1.  Reads g and *scale.
 * NULL tables, chunks or workspace, a negative count, n_partials < n_chunks, a misaligned chunk table or workspace ->
 * DHD_EINVAL; workspace_bytes too small -> DHD_ENOSPACE.  n_chunks == 0: nothing is launched.  One launch on `stream`; nothing
 * allocated, kept or synchronised. */
int dhdw_optim_grad_norm(const dhdw_optim_tables* t, void* workspace, size_t workspace_bytes, void* stream);

/* One workgroup: the record, the multiplier, the step counts and scalars of every slot, the scale rule.  max_norm < 0: no
 * clipping (coef = 1).  growth_factor, backoff_factor, growth_interval: torch._amp_update_scale_'s, looked at only with a scale.
 * Checked as above, and: NULL groups, slot_group, steps, slot_scalars or group_scalars with n_slots > 0, scale without
 * growth_tracker, NaN max_norm -> DHD_EINVAL. */
int dhdw_optim_finalize(const dhdw_optim_tables* t, float max_norm, float growth_factor, float backoff_factor, int growth_interval,
                        void* workspace, size_t workspace_bytes, void* stream);

/* One workgroup per chunk: the update above.  Checked as above, and: a chunk table with n_chunks > 0 without groups,
 * slot_scalars or group_scalars -> DHD_EINVAL.  The rows themselves live on the device and are not looked at by the host: the
 * caller answers for addresses, lengths and indices. */
int dhdw_optim_adamw_update(const dhdw_optim_tables* t, const void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DHD_AMD_OPTIM_H */
