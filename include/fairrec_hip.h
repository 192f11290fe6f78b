/*
 * fairrec_hip.h -- C ABI of libfairrec_hip.so: the MI355X (gfx950) kernels behind the
 * RecBole-FairRec training hot path (embedding gather -> score -> fairness-regularised loss ->
 * backward -> Adam).
 *
 * The reference has no native boundary at all: its "operators" on this
 * path are stock PyTorch calls made from Python.  Every entry point below therefore cites the
 * reference Python call sites (file:line under the reference checkout) whose work it replaces.
 *
 * Conventions
 *   - plain C: raw DEVICE pointers, sizes, scalars and a hipStream_t (passed as void*); no torch types.
 *   - every call is asynchronous on `stream`, never synchronises, never allocates or frees: the caller
 *     owns all buffers and passes a workspace (size from the matching *_workspace_bytes query).
 *   - return value: 0 = ok, <0 = FR_E* (invalid argument / HIP error); message via fr_last_error()
 *     (thread-local).  Data-dependent faults that can only be seen on the device (row id out of range,
 *     more than two sensitive groups in a batch) set bits in the caller-supplied `err_flag` word.
 *   - ids are int64 at the boundary (torch.LongTensor, dataset.py:1790-1791), values fp32, tables
 *     fp32 [n_rows, dim] row-major.
 */
#ifndef FAIRREC_HIP_H
#define FAIRREC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__) || defined(__clang__)
#define FR_API __attribute__((visibility("default")))
#else
#define FR_API
#endif

#define FR_OK 0
#define FR_EINVAL (-1)      /* bad argument (null pointer, unsupported dim, workspace too small ...) */
#define FR_EHIP (-2)        /* a HIP runtime call failed; see fr_last_error() */
#define FR_EUNSUPPORTED (-3)

/* bits of the device-side error word */
#define FR_DEV_ERR_INDEX_RANGE 1u   /* a row id was <0 or >= n_rows (reference: IndexError in F.embedding) */
#define FR_DEV_ERR_SST_GROUPS 2u    /* >2 distinct sensitive values in one batch (reference: IndexError at focf.py:86) */

#define FR_DEV_ERR_BUCKET_OVERFLOW 4u /* a per-owner exchange bucket exceeded its fixed capacity (raise shard_capacity) */
#define FR_DEV_ERR_PIPE_WAIT 8u     /* fr_focf_step_runs_pipe: a row of the previous batch was not published within the wait bound */
#define FR_DEV_ERR_SAMPLE_ROUNDS 16u /* fr_sample_negatives_pop*: a call still had positions open after its round cap (2^20) */

/* FOCF fairness objectives -- FOCF.get_loss_fun, focf.py:50-68 */
enum fr_focf_objective {
    FR_FOCF_NONE = 0, FR_FOCF_VALUE = 1, FR_FOCF_ABSOLUTE = 2, FR_FOCF_UNDER = 3, FR_FOCF_OVER = 4,
    FR_FOCF_NONPARITY = 5
};

/*
 * An embedding table with lazily-applied dense Adam (coupled L2).
 *
 * Replaces: nn.Embedding weight + the per-parameter state of torch.optim.Adam built at
 * trainer.py:139 (exp_avg, exp_avg_sq, step).  The reference sweeps the whole table every step
 * (dense gradient, dense Adam).  Here a row's state is (p,m,v) "as of step last[row]"; the steps a
 * row missed have gradient wd*p only and are replayed in registers, in the reference's op order,
 * when the row is next read (or by the bounded-staleness sweeper / fr_table_flush).  Results are
 * those of the dense update up to fp32 rounding.
 */
typedef struct fr_table {
    float* p;          /* [n_rows, dim] parameters (the nn.Embedding weight storage) */
    float* m;          /* [n_rows, dim] exp_avg */
    float* v;          /* [n_rows, dim] exp_avg_sq */
    int32_t* last;     /* [n_rows] optimizer step the row's (p,m,v) are current for */
    int32_t* stamp;    /* [n_rows] last step at which the row was gathered for training */
    int64_t n_rows;
    int32_t dim;       /* embedding_size; 1..256 */
    int32_t step;      /* optimizer step count of this tensor so far (torch: state['step']) */
    /* Optional device-resident step counter (NULL = none).  When set, the effective step of a call is
     * *step_dev + step, read on the device: a training step captured once in a hipGraph can then be replayed every
     * iteration (the host passes the constant offset, e.g. 1 for "the step being applied", and advances the counter
     * with a kernel inside the graph).  Honoured by fr_table_gather / _gather_train / _apply_grad / _flush. */
    const int32_t* step_dev;
} fr_table;

/*
 * Adam hyper-parameters (torch.optim.Adam defaults + lr/weight_decay from trainer.py:131-139) and the
 * per-step scalars torch computes in double on the host (torch/optim/adam.py, _single_tensor_adam):
 *   scalars[4*j]   = (float)(lr / (1 - beta1^j))                      step_size_j
 *   scalars[4*j+1] = (float)(1 / sqrt(1 - beta2^j))                   1/sqrt(bias_correction2_j)
 *   scalars[4*j+2] = (float)(sqrt(k2) * scalars[4j+1] / (step_size_j * k1))   with k1 = (1-beta1)*wd,
 *   scalars[4*j+3] = (float)(eps / (step_size_j * k1))                         k2 = (1-beta2)*wd^2 (0 when wd = 0)
 * for j = 1..cap ; entry 0 unused.  Entries 2,3 let a replayed step (gradient = wd*p only) run on scaled moments.
 * Steps beyond `cap` use entry `cap` (the host guarantees the scalars have saturated there).
 *
 * `learner` selects the optimizer (torch.optim.<Learner> with torch's defaults and coupled L2 weight decay; the reference's
 * trainer passes only lr and weight_decay).  The same struct carries every learner; per learner:
 *   FR_LEARNER_ADAM    as above.  State: fr_table.m = exp_avg, fr_table.v = exp_avg_sq.
 *   FR_LEARNER_SGD     momentum 0.  scalars[4j] = (float)lr_j, scalars[4j+1] = (float)(-lr_j * wd) (the coefficient of the
 *                      one fma of a replayed step, p <- p + k_j*p), 4j+2..3 = 0.  beta1, beta2, eps unused.
 *                      State: none -- fr_table.m and .v may be NULL and are never read or written.
 *   FR_LEARNER_ADAGRAD lr_decay 0, initial_accumulator_value 0.  scalars[4j] = (float)(lr / (1 + (j-1)*lr_decay)) (clr),
 *                      4j+1..3 = 0.  eps = 1e-10 by default.  beta1, beta2 unused.
 *                      State: fr_table.m = sum; fr_table.v may be NULL and is never read or written.
 *   FR_LEARNER_RMSPROP momentum 0, not centered.  scalars[4j] = (float)lr_j, 4j+1..3 = 0.  beta2 = alpha (0.99), eps = 1e-8.
 *                      beta1 unused.  State: fr_table.m = square_avg; fr_table.v may be NULL and is never touched.
 * A zero-data-gradient step is the identity for SGD and Adagrad with weight_decay = 0: their tables are never replayed or
 * swept (rows outside a batch do not change), and fr_table_flush launches nothing.  RMSprop with weight_decay = 0 only
 * decays square_avg.  The FOCF entry points (fr_focf_*) run Adam only and refuse any other learner with FR_EINVAL.
 */
#define FR_LEARNER_ADAM 0
#define FR_LEARNER_SGD 1
#define FR_LEARNER_ADAGRAD 2
#define FR_LEARNER_RMSPROP 3
typedef struct fr_adam {
    const float* scalars;  /* device, float[4*(cap+1)] */
    int32_t cap;
    int32_t learner;       /* FR_LEARNER_*; 0 = Adam */
    double weight_decay, beta1, beta2, eps; /* doubles: torch derives (1 - beta) in double before the fp32 cast */
} fr_adam;
typedef fr_adam fr_optim;   /* the same struct under a learner-neutral name */

FR_API int fr_version(void);
FR_API const char* fr_last_error(void);

/*
 * Sort the M row ids of a batch and cut them into segments of equal id.
 * Replaces the dedup the reference gets implicitly from dense embedding_dense_backward (autograd of
 * nn.Embedding, focf.py:138-139) and from torch.unique(return_inverse) at focf.py:77-78 / nfcf.py:79-80.
 *   perm[j]      : batch position of the j-th smallest (id, position) pair        [M]
 *   seg_start[k] : first j of segment k; seg_start[n_seg] = M                      [M+1]
 *   seg_row[k]   : the row id of segment k                                         [M]
 *   seg_of[b]    : segment index of batch position b  (= torch.unique inverse)     [M]
 *   n_seg        : number of distinct ids                                          [1]
 * M <= FR_SORT_MAX.
 */
#define FR_SORT_MAX 16384
FR_API int fr_sort_segments(const int64_t* idx, int64_t M, int64_t n_rows, int32_t* perm, int32_t* seg_start,
                     int32_t* seg_row, int32_t* seg_of, int32_t* n_seg, uint32_t* err_flag, void* stream);

/* ---- FOCF (focf.py) ---------------------------------------------------------------------------- */

FR_API size_t fr_focf_workspace_bytes(int64_t B, int32_t dim);

/*
 * Forward of one training batch: FOCF.calculate_loss, focf.py:152-169 (= forward :136-143, MSELoss
 * :158, get_item_ratings :75-91 and the unfairness terms :93-134).  Reads the tables (never writes
 * p/m/v/last), leaves the caught-up rows and dLoss/dpred in the workspace for fr_focf_backward_adam.
 *   loss_out[0] = loss, loss_out[1] = mse part, loss_out[2] = fairness part (unweighted)   (device)
 *   pred_out    = pred_scores [B] (device, may be NULL)
 */
#define FR_FOCF_PREPARED 1   /* flags: fr_focf_prepare(_many) already ran for this batch on this workspace */
/* FR_FOCF_DEFER_LOSS: loss_out is written by the fr_focf_backward_adam that follows on the same workspace and stream
 * (one extra workgroup of its launch) instead of by this call -- for step loops that read the loss after optimizer.step().
 * Takes the reduction's ticket round trip off the end of the fairness kernel, i.e. off the step's critical path.
 * The record of what is still to be reduced travels in the workspace (device memory): the library keeps no host state. */
#define FR_FOCF_DEFER_LOSS 2
/* FR_FOCF_ITEM_RUNS: a hint -- the interactions of an item sit next to each other in the batch (item-complete batches,
 * focf_dataloader.py:37-51).  The gather kernel then replays an item row once per workgroup instead of once per wave (the
 * item row carries the longest replay there: 25.6 -> 21.1 us at K = 82 items per batch).  Same results either way. */
#define FR_FOCF_ITEM_RUNS 4
FR_API int fr_focf_forward(const fr_table* U, const fr_table* I, const fr_adam* adam, const int64_t* user,
                    const int64_t* item, const float* rating, const float* sst, int64_t B, int32_t objective,
                    float fair_weight, int32_t flags, void* ws, size_t ws_bytes, float* loss_out, float* pred_out,
                    uint32_t* err_flag, void* stream);

/*
 * The index-only part of fr_focf_forward (sort + segmentation of the id columns, min/max of sst), callable one
 * batch AHEAD on another stream while the previous batch's kernels run: it depends on nothing but the ids, the
 * way a dataloader prefetches the next batch (trainer.py:181 iterates `train_data`).  Pass `sst` = NULL for
 * fair_objective none.  The caller orders it against the consumers of `ws` with events.
 */
FR_API int fr_focf_prepare(const int64_t* user, const int64_t* item, const float* sst, int64_t B, int64_t n_users,
                    int64_t n_items, int32_t dim, void* ws, size_t ws_bytes, uint32_t* err_flag, void* stream);

/*
 * The same for up to FR_FOCF_PREPARE_MAX COMING batches in one launch (one workgroup per id column: the sort is
 * latency-bound, so n batches cost the time of one, and the per-step critical path holds no sort and no stream join).
 */
#define FR_FOCF_PREPARE_MAX 8
typedef struct fr_focf_batch {
    const int64_t* user;
    const int64_t* item;
    const float* sst;      /* NULL for fair_objective none */
    int64_t B;
    void* ws;
    size_t ws_bytes;
    const float* rating;   /* fr_focf_prepare_step only (fr_focf_prepare_many ignores it) */
} fr_focf_batch;
FR_API int fr_focf_prepare_many(const fr_focf_batch* batches, int32_t n, int64_t n_users, int64_t n_items, int32_t dim,
                         uint32_t* err_flag, void* stream);

/*
 * torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm, norm_type=2) of the reference's step loop
 * (trainer.py:194-195, config `clip_grad_norm`), for the batch of the preceding fr_focf_forward on this workspace and
 * before its fr_focf_backward_adam.  The dense embedding gradients are never materialised: their squared 2-norm is
 * the sum over the distinct rows of the batch of |sum_b dLoss/dpred[b] * other_row[b]|^2 (one wave per row, fixed
 * order), `extra_sqnorm` (device float, may be NULL) adds other parameters' share, clip_coef = min(1, max_norm /
 * (norm + 1e-6)) scales dLoss/dpred in the workspace, i.e. every gradient row the backward launch forms.
 * `norm_out` (device float[2], may be NULL) receives (total_norm, clip_coef).
 */
FR_API int fr_focf_clip_grad_norm(const fr_table* U, const fr_table* I, int64_t B, float max_norm,
                           const float* extra_sqnorm, float* norm_out, void* ws, size_t ws_bytes, void* stream);

/*
 * loss.backward() + optimizer.step() for the batch of the preceding fr_focf_forward on the same
 * workspace: autograd of focf.py:152-169 (dense embedding gradient) followed by Adam.step()
 * (trainer.py:193-196).  Duplicate rows are summed in batch order before the update, rows not in the
 * batch are left to the lazy replay; `sweep_period` S>0 additionally brings rows
 * [s*ceil(n/S), (s+1)*ceil(n/S)), s = step mod S, up to date each call (bounds the replay length).
 * Increments U->step / I->step semantics are the CALLER's: pass tables whose .step is the step being
 * applied (old step + 1) in both calls of a batch.
 */
FR_API int fr_focf_backward_adam(const fr_table* U, const fr_table* I, const fr_adam* adam, int64_t B,
                          int32_t sweep_period, void* ws, size_t ws_bytes, void* stream);

/*
 * The whole training step of one batch as ONE launch: FOCF.calculate_loss (focf.py:152-169) + loss.backward()
 * (trainer.py:193) + optimizer.step() (trainer.py:196), for step loops that read the loss after the optimizer step
 * (what FR_FOCF_DEFER_LOSS serves on the three-launch path).  Same results as fr_focf_forward + fr_focf_backward_adam;
 * objectives none / value / absolute / under / over (nonparity and clip_grad_norm need batch-wide values between the
 * forward and the update: use the three-launch path).  A wave keeps both rows of its interaction in registers from
 * the gather to the Adam write-back; rows shared by several interactions of the batch are finished by the last of
 * their waves to arrive (csrc/focf_step.hip).
 *   fr_focf_prepare_step : fr_focf_prepare_many plus what the fused launch needs from the index side: per batch
 *                          position one packed record (user row, item row, rating, sst) -- ids range-checked here, so
 *                          the step itself reads no id column -- and the extent of its user / item segment, zeroed
 *                          arrival counters, and
 *                          stamp[row] = max(stamp[row], stamps[q]) on every row of batch q in both tables -- the
 *                          sweeper waves of fr_focf_step leave rows stamped >= its `stamp` argument alone.  Callable
 *                          ahead on another stream (depends on the id columns only; the stamp raise is an atomic max).
 *                          stamps[q]: any value >= every stamp handed out before (the engine uses the step at which
 *                          the batch is expected to be applied).  It also leaves a START ORDER of the interactions,
 *                          longest estimated replay first (from the rows' `last` as of now; replay_cap = the sweep
 *                          period that bounds a replay, 0 = unbounded): the step's launch ends one wave latency after
 *                          its last wave starts, so long replays must not start last.  Order only, never a result.
 *   fr_focf_step         : the step (U->step == I->step = the step being applied).  `stamp` = the value given to
 *                          fr_focf_prepare_step for this batch.  The loss needs every wave of the launch, so it is
 *                          reduced LATER: by the next fr_focf_step (prev_ws / prev_B / prev_loss_out name the earlier
 *                          batch; one extra workgroup) or by fr_focf_step_finish.  loss_acc (device float[8], may be
 *                          NULL): [0..2] += (loss, mse, fair) of every reduced batch, [3] += 1, [4] = 1-based index of the
 *                          first reduced batch whose loss was NaN (sticky; 0 = none): a running total for epoch loops.
 *                          loss_out is where THIS batch's loss will be written by that later reduction (recorded by the
 *                          caller; not written here).
 *   fr_focf_step_finish  : the reduction for a batch no later step will reduce (end of an epoch, before reading).
 */
FR_API int fr_focf_prepare_step(const fr_focf_batch* batches, const int32_t* stamps, int32_t n, const fr_table* U,
                                const fr_table* I, int32_t replay_cap, uint32_t* err_flag, void* stream);
FR_API int fr_focf_step(const fr_table* U, const fr_table* I, const fr_adam* adam, const int64_t* user,
                        const int64_t* item, const float* rating, const float* sst, int64_t B, int32_t objective,
                        float fair_weight, int32_t sweep_period, int32_t stamp, void* ws, size_t ws_bytes,
                        float* loss_out, void* prev_ws, int64_t prev_B, float* prev_loss_out, float* loss_acc,
                        uint32_t* err_flag, void* stream);
FR_API int fr_focf_step_finish(void* ws, size_t ws_bytes, int64_t B, int32_t dim, int32_t objective, float fair_weight,
                               float* loss_out, float* loss_acc, void* stream);
/*
 * fr_focf_step for ITEM-COMPLETE batches -- what the reference's own loader feeds FOCF with (focf_dataloader.py:37-51:
 * random items, all interactions of each, until >= train_batch_size rows: tens of distinct items of ~100 rows) -- same
 * contract (batch prepared by fr_focf_prepare_step with `stamp`, loss reduced by the next step or fr_focf_step_finish), same
 * results as fr_focf_forward(FR_FOCF_ITEM_RUNS) + fr_focf_backward_adam (every sum in the same order), bit-reproducible.
 * Two launches instead of three: the chain's gather, then ONE WORKGROUP PER ITEM RUN that forms the per-group sums by wave
 * shuffles (the fairness kernel's lane order), updates the members' user rows with all its waves, sums the item's gradient
 * from LDS in ascending batch position and updates the item row; the sweep slice rides in the second launch.  Only users that
 * recur under several items of the batch go through an arrival counter (csrc/focf_runs.hip).
 */
FR_API int fr_focf_step_runs(const fr_table* U, const fr_table* I, const fr_adam* adam, const int64_t* user,
                             const int64_t* item, const float* rating, const float* sst, int64_t B, int32_t objective,
                             float fair_weight, int32_t sweep_period, int32_t stamp, void* ws, size_t ws_bytes, void* prev_ws,
                             int64_t prev_B, float* prev_loss_out, float* loss_acc, uint32_t* err_flag, void* stream);
/* The same step with the two launches of CONSECUTIVE steps side by side (csrc/focf_runs.hip): one launch = the item runs of
 * the batch the previous call gathered (`fin_ws`, `fin_B`, applied at `fin_step`; NULL: none) + the gather of this call's batch
 * (`user` == NULL: none -- the call that drains the pipeline) + this step's sweep slice + the loss reduction of the batch
 * the previous call finished (`prev_ws`).  A row that both batches hold is taken by the gather only after the finisher has
 * published it.  `own_u` / `own_i`: int32 [2 * n_rows] each, zero-initialised (and zeroed again when the tables' steps are
 * rewound).  Same results as fr_focf_step_runs; U / I carry the step of the batch being gathered (fin_step if there is none). */
FR_API int fr_focf_step_runs_pipe(const fr_table* U, const fr_table* I, const fr_adam* adam, const int64_t* user,
                                  const int64_t* item, const float* rating, const float* sst, int64_t B, int32_t objective,
                                  float fair_weight, int32_t sweep_period, int32_t stamp, void* ws, size_t ws_bytes, void* fin_ws,
                                  int64_t fin_B, int32_t fin_step, void* prev_ws, int64_t prev_B, float* prev_loss_out,
                                  float* loss_acc, int32_t* own_u, int32_t* own_i, uint32_t* err_flag, void* stream);

/*
 * The same step with the index work of the COMING batches riding in the step launches themselves, instead of a look-ahead
 * sort on a second stream (fr_focf_prepare_step): no sort, no stream fork / join in the step loop.  Every table row has
 * one 64-bit word per generation (`row_words`: fr_focf_row_words() words, zeroed once by the caller; three generations =
 * the batch being applied and the two behind it), and a batch goes through two stages of a few workgroups each:
 *   claim (two launches before its step): one thread per interaction counts itself into its rows' words (stamp << 29 |
 *         members << 14 | base; a word left by an older batch is first raised to the new stamp by an atomic maximum, so
 *         nothing is ever reset), stamps the rows for the sweeper, takes a place in its start class by replay length; K and
 *         the sensitive values by atomics; the sweeper tasks of the stamped step are classed the same way;
 *   place (one launch before): counts are final -- (members of its user, of its item) per interaction, a slice of the
 *         member list per shared row, the records written in start order.
 * In the step, the members of a shared row enter their batch position in the row's list and leave the word one by one;
 * whoever brings the count to zero reads the list, orders it (ascending batch position, in registers) and finishes the
 * row exactly as the sorted path does: same sums in the same order, bit-identical parameters.  The reported fairness
 * value sums the items' terms in batch order of their first members instead of item-id order (last-bit differences in
 * the loss value only).
 *   fr_focf_stage        : stages on their own launch (the first batches of a loop; either batch may be NULL).  U->step /
 *                          I->step = the optimizer step the batch to place -- without one, the batch to claim -- will be
 *                          applied at (with both, the claimed batch is applied one step later): the start order of that
 *                          step's sweeper tasks is built for the step's slice of the tables, whatever the stamps are.
 *   fr_focf_step_staged  : fr_focf_step for a batch that went through both stages with stamp `stamp`, carrying the
 *                          claim of one coming batch and the place of another (either may be NULL).  Stamps must be
 *                          handed out in strictly increasing order.  `gen` (0..2) names the generation of row words a
 *                          batch uses from its claim to its step: the (up to) three batches in flight at any time --
 *                          claimed, placed, being applied -- must hold three different ones.
 *   fr_focf_step_finish_staged : fr_focf_step_finish for such a batch (also returns its workspace's counters to zero,
 *                          as the next fr_focf_step_staged would have).
 * A workspace must be zero-filled before its first claim.
 */
FR_API size_t fr_focf_row_words(int64_t n_users, int64_t n_items);
FR_API int fr_focf_stage(const fr_table* U, const fr_table* I, const fr_focf_batch* claim, int32_t claim_stamp,
                         int32_t claim_gen, const fr_focf_batch* place, int32_t place_stamp, int32_t place_gen,
                         int32_t sweep_period, uint64_t* row_words, uint32_t* err_flag, void* stream);
FR_API int fr_focf_step_staged(const fr_table* U, const fr_table* I, const fr_adam* adam, const float* sst, int64_t B,
                               int32_t objective, float fair_weight, int32_t sweep_period, int32_t stamp, int32_t gen,
                               void* ws, size_t ws_bytes, void* prev_ws, int64_t prev_B, float* prev_loss_out,
                               float* loss_acc, uint64_t* row_words, const fr_focf_batch* claim, int32_t claim_stamp,
                               int32_t claim_gen, const fr_focf_batch* place, int32_t place_stamp, int32_t place_gen,
                               uint32_t* err_flag, void* stream);
FR_API int fr_focf_step_finish_staged(void* ws, size_t ws_bytes, int64_t B, int32_t dim, int32_t objective,
                                      float fair_weight, float* loss_out, float* loss_acc, void* stream);
/*
 * The step loop itself (trainer.py:181-196: `for batch in train_data: zero_grad; calculate_loss; backward; step`) for a run
 * of `n` batches in ONE call: n launches of fr_focf_step_staged issued by the library, so the host pays one foreign call
 * per run instead of an interpreter round trip per step.  Batch k is applied at step U->step + k (U->step = the step of
 * the FIRST batch, as everywhere), with stamp first_stamp + k and generation (first_gen + k) % 3; its launch carries the
 * place stage of batch k + 1 and the claim stage of batch k + 2 and reduces the loss of batch k - 1 into
 * loss_ring[4 * ((first_slot + k - 1) % loss_slots)] and loss_acc (batch 0's launch reduces `prev_*`, an earlier staged
 * batch still unreduced, or nothing when prev_ws is NULL).  The first two batches' stages take two launches of their own.
 * Any four consecutive batches (and prev_ws with the first three) need four different workspaces, each zero-filled before
 * its first use.  Nothing may be in flight through the stages when the call starts; the LAST batch's loss stays unreduced
 * (hand it to the next call as prev_*, or to fr_focf_step_finish_staged).  Same launches, same bits as n calls of
 * fr_focf_step_staged.
 */
/*
 * The same loop for ITEM-COMPLETE batches (the only shape the reference's FOCFDataLoader yields, focf_dataloader.py:37-51):
 * n launches of fr_focf_step_runs_pipe issued by the library, the batches' sorted prepare (fr_focf_prepare_step,
 * FR_FOCF_PREPARE_MAX batches per launch) running one group ahead on the library's side stream and joined once per group.
 * Batch k is gathered at step U->step + k with stamp first_stamp + k; its item runs ride in the launch of batch k + 1, and the
 * launch of batch k + 2 reduces its loss into loss_ring[4 * ((first_slot + k) % loss_slots)] and loss_acc.  `fin_*`: a batch
 * the previous call gathered and nobody finished yet (fin_step = U->step - 1, fin_loss_out = its loss slot; NULL: none);
 * `prev_*`: a finished batch whose loss is still unreduced (NULL: none).  When the call returns, batch n - 1 is in the `fin`
 * position and batch n - 2 (or the incoming `fin`) in the `prev` position: hand them to the next call, or drain them with
 * fr_focf_step_runs_pipe(user = NULL) + fr_focf_step_finish.  Batches closer than 2 * FR_FOCF_PREPARE_MAX + 2 in the run need
 * different workspaces, none of them a pending one.  Same launches, same bits as n calls of fr_focf_step_runs_pipe.
 */
FR_API int fr_focf_runs_many(const fr_table* U, const fr_table* I, const fr_adam* adam, const fr_focf_batch* batches,
                             int32_t n, int32_t objective, float fair_weight, int32_t sweep_period, int32_t first_stamp,
                             void* fin_ws, int64_t fin_B, int32_t fin_step, float* fin_loss_out, void* prev_ws, int64_t prev_B,
                             float* prev_loss_out, float* loss_ring, int32_t loss_slots, int32_t first_slot, float* loss_acc,
                             int32_t* own_u, int32_t* own_i, uint32_t* err_flag, void* stream);
FR_API int fr_focf_steps_many(const fr_table* U, const fr_table* I, const fr_adam* adam, const fr_focf_batch* batches,
                              int32_t n, int32_t objective, float fair_weight, int32_t sweep_period, int32_t first_stamp,
                              int32_t first_gen, void* prev_ws, int64_t prev_B, float* prev_loss_out, float* loss_ring,
                              int32_t loss_slots, int32_t first_slot, float* loss_acc, uint64_t* row_words,
                              uint32_t* err_flag, void* stream);

/* FOCF.predict, focf.py:145-150: clamp(pred, 0, max_rating) / max_rating on up-to-date rows (read only). */
FR_API int fr_focf_predict(const fr_table* U, const fr_table* I, const fr_adam* adam, const int64_t* user,
                    const int64_t* item, int64_t B, float max_rating, float* out, uint32_t* err_flag, void* stream);

/* ---- lazy Adam table maintenance ---------------------------------------------------------------- */

/* Bring every row of the table up to step `t->step` (needed before anything reads the whole table:
 * state_dict / checkpoint trainer.py:221-240, full_sort_predict focf.py:171-178, evaluation). */
FR_API int fr_table_flush(const fr_table* t, const fr_adam* adam, void* stream);

/* Gather rows as of step t->step (read only; replay in registers): out[j,:] = p[idx[j],:]. */
FR_API int fr_table_gather(const fr_table* t, const fr_adam* adam, const int64_t* idx, int64_t M, float* out,
                    uint32_t* err_flag, void* stream);

/*
 * Generic training pair for models whose score is not a plain dot product (NFCF nfcf.py:69-74, PFCN
 * pfcn_biasedmf.py:144-166) and for the owner side of the row-sharded multi-GPU path:
 *   fr_table_gather_train : sort idx into segments + gather the rows as of step t->step-1 (lazy replay) into
 *                           rows_out[M,dim]; caught-up moments stay in the workspace.  Replaces nn.Embedding.forward.
 *   ... the caller runs its forward/backward on rows_out and produces grad_rows[M,dim] = dLoss/d rows_out ...
 *   fr_table_apply_grad   : per distinct row, sum grad_rows over duplicates in ascending position (what
 *                           embedding_dense_backward does), apply Adam step t->step, write the row back; plus the
 *                           sweeper slice.  Replaces loss.backward() on the embedding + optimizer.step().
 * `t->step` is the step being applied in both calls; M <= FR_SORT_MAX.
 *
 * Slot layout (chunk, stride) of idx / rows_out / rows / grad_rows: logical position j sits at
 * (j / chunk) * stride + j % chunk  rows (ids) from the pointer; chunk = 0 is the dense [M, ...] layout.  With
 * chunk = cap, stride = T*cap and pointers advanced by t*cap rows, table t of T works in place on a shared
 * [G, T, cap, ...] all-to-all buffer (multi-GPU path), so the exchange needs no packing copies.
 */
FR_API size_t fr_table_train_workspace_bytes(int64_t M, int32_t dim);
/* Orders `stream` behind the index work (the sort fr_table_gather_train launches on the library's side stream) still pending
 * on workspace `ws`.  fr_table_apply_grad, fr_focf_shard_fair and fr_nfcf_loss do this themselves; a caller that reads the
 * segments of a workspace on its own (copying them for fr_table_gather_train_prepared) calls this first. */
FR_API int fr_table_join(const void* ws, void* stream);

/*
 * The stream fr_table_gather_train runs its id sort on, beside the caller's stream (NULL when it sorts in line: profiler on,
 * FAIRREC_NO_OVERLAP=1).  The sort reads the id list and writes the workspace until the consumer of the segments
 * (fr_table_apply_grad, fr_table_join) has ordered the caller's stream behind it; a caller whose allocator recycles memory in
 * stream order must tell it that both buffers are in use on this stream as well (torch: Tensor.record_stream), or a buffer
 * freed after a forward pass that no backward pass followed can be handed out again while the sort still writes to it.
 */
FR_API void* fr_side_stream_handle(void);
/* fr_table_gather_train(t, idx) and fr_table_gather(ro, ro_idx) -- a frozen table next to a training one: NFCF's finetune
 * stage, nfcf.py:66-71 -- in ONE launch that also carries the sort of `idx` (same results as the two calls; falls back to
 * them when the two tables' rows have different fragment counts). */
FR_API int fr_table_lookup_pair(const fr_table* t, const fr_adam* adam, const int64_t* idx, int64_t M, float* rows_out,
                                void* ws, size_t ws_bytes, const fr_table* ro, const fr_adam* ro_adam, const int64_t* ro_idx,
                                int64_t ro_M, float* ro_out, uint32_t* err_flag, void* stream);
/* The first fr_table_segments_bytes(M) bytes of a workspace hold the sorted segments of the id list (independent of the
 * table's width).  fr_table_gather_train_prepared skips the sort: the caller has put the segments of `idx` there, e.g. by
 * copying them from the workspace of another table with the same number of rows looked up with the same ids in this step
 * (PFCN_BiasedMF's bias tables next to the embedding tables, pfcn_biasedmf.py:186-190). */
FR_API size_t fr_table_segments_bytes(int64_t M);
FR_API int fr_table_gather_train_prepared(const fr_table* t, const fr_adam* adam, const int64_t* idx, int64_t M,
                                          int32_t chunk, int32_t stride, float* rows_out, void* ws, size_t ws_bytes,
                                          uint32_t* err_flag, void* stream);
FR_API int fr_table_gather_train(const fr_table* t, const fr_adam* adam, const int64_t* idx, int64_t M, int32_t chunk,
                                 int32_t stride, float* rows_out, void* ws, size_t ws_bytes, uint32_t* err_flag,
                                 void* stream);
FR_API int fr_table_apply_grad(const fr_table* t, const fr_adam* adam, int64_t M, int32_t chunk, int32_t stride,
                               const float* rows, const float* grad_rows, int32_t sweep_period, void* ws,
                               size_t ws_bytes, void* stream);
/* The same for TWO tables of equal dim and M in one launch each (one sort workgroup / one grid slice per table):
 * the user and item table of a step.  ws_a != ws_b, each of fr_table_train_workspace_bytes(M, dim). */
#define FR_TABLE_PREPARED 1   /* flags: fr_table_sort2 already ran for these id lists on these workspaces */
FR_API int fr_table_gather_train2(const fr_table* ta, const fr_table* tb, const fr_adam* adam, const int64_t* idx_a,
                                  const int64_t* idx_b, int64_t M, int32_t chunk, int32_t stride, float* rows_a,
                                  float* rows_b, int32_t flags, void* ws_a, void* ws_b, size_t ws_bytes,
                                  uint32_t* err_flag, void* stream);
/* The index-only part of fr_table_gather_train2 (sort + segmentation of both id lists into the workspaces), callable
 * one batch AHEAD on another stream: it depends on nothing but the ids.  The caller orders it against the users of the
 * workspaces with events. */
FR_API int fr_table_sort2(const int64_t* idx_a, const int64_t* idx_b, int64_t n_rows_a, int64_t n_rows_b, int64_t M,
                          int32_t chunk, int32_t stride, int32_t dim, void* ws_a, void* ws_b, size_t ws_bytes,
                          uint32_t* err_flag, void* stream);
FR_API int fr_table_apply_grad2(const fr_table* ta, const fr_table* tb, const fr_adam* adam, int64_t M, int32_t chunk,
                                int32_t stride, const float* rows_a, const float* grad_a, const float* rows_b,
                                const float* grad_b, int32_t sweep_a, int32_t sweep_b, void* ws_a, void* ws_b,
                                size_t ws_bytes, void* stream);
/* fr_table_apply_grad on two tables of one width in ONE launch, each with its own id count (PFCN: the user rows of a batch and
 * the item rows of its positive + negative ids, pfcn_pmf.py:169-176; their two bias columns likewise): the shorter table's
 * update and sweep slice run beside the longer one's.  Same results as the two calls; both tables step under `adam`. */
FR_API int fr_table_apply_grad_two(const fr_table* ta, const fr_table* tb, const fr_adam* adam, int64_t Ma, int64_t Mb,
                                   const float* rows_a, const float* grad_a, const float* rows_b, const float* grad_b,
                                   int32_t sweep_a, int32_t sweep_b, void* ws_a, size_t ws_a_bytes, void* ws_b,
                                   size_t ws_b_bytes, void* stream);

/* ---- row-sharded tables (multi-GPU) -----------------------------------------------------
 * owner(row) = row mod G, local row = row div G.  All exchange buffers have the fixed shape [G, cap] slots so
 * that a step needs no host sync; -1 ids are padding (ignored by fr_sort_segments / fr_table_gather_train).
 * fr_bucket_by_owner: stable partition of idx by owner; slot (o, k) = o*stride + offset + k is where the k-th id owned
 * by rank o sits in send_ids and where its answer will sit in every reply buffer (slot_of[pos], -1 on overflow).
 * stride = cap, offset = 0: a [G, cap] buffer of its own; stride = T*cap, offset = t*cap: list t of a shared
 * [G, T, cap] buffer (one all-to-all for T id lists).
 * aux (may be NULL): (min, max) of that float column over the M positions is written, as two floats, into the int64
 * slot o*stride + aux_slot of every owner's chunk (a slot outside the id lists), so batch-wide extrema ride along
 * with the id exchange (FOCF: the two sensitive-attribute values present in the global batch, focf.py:77-79). */
FR_API int fr_bucket_by_owner(const int64_t* idx, int64_t M, int32_t G, int32_t cap, int32_t stride, int32_t offset,
                              int64_t* send_ids, int32_t* slot_of, int32_t* counts, const float* aux, int32_t aux_slot,
                              uint32_t* err_flag, void* stream);
/* Two id lists of the same length in ONE launch (one workgroup each): list a at offset_a, list b at offset_b of the
 * same [G, stride] buffer; counts = [2, G]; aux / aux_slot as above (computed by list b's workgroup). */
/* Item-owner-computes schedule of the row-sharded FOCF step (fairrec/sharded.py, ShardedFocfEngineV2): every interaction is
 * sent to the rank that owns its item row.  A record chunk is [4 * cap + 1] int64: item local rows (fr_bucket_by_owner with
 * stride 4 * cap + 1, offset 0; -1 = empty) | user ids | rating bits | sst bits | the sender's (min, max) of sst (the bucket
 * kernel's aux pair).  fr_shard_pack_records fills planes 1-3 at the slots the bucket kernel assigned; the receiver's
 * fr_shard_unpack_records turns its G chunks into per-slot arrays (item row, user id, own slot index or -1, rating or 0,
 * sst) and the G (min, max) pairs.  fr_shard_post_fair / fr_shard_loss_finish: see csrc/shard.hip. */
FR_API int fr_shard_pack_records(const int32_t* slot, const int64_t* user, const float* rating, const float* sst, int64_t B,
                                 int32_t cap, int64_t* send, void* stream);
FR_API int fr_shard_unpack_records(const int64_t* recv, int32_t G, int32_t cap, int64_t* iid, int64_t* uid, int32_t* islot,
                                   float* rating, float* sst, int64_t* mm, void* stream);
/* out[0] = number of distinct ids >= 0 of the list; bitmap = (n_rows + 31) / 32 words, all zero before and after; count = one
 * zero int32, zero again afterwards. */
FR_API int fr_shard_count_distinct(const int64_t* ids, int64_t n, int64_t n_rows, uint32_t* bitmap, int32_t* count, float* out,
                                   void* stream);
FR_API int fr_shard_post_fair(float* reply, const float* k_all, int32_t G, int32_t cap, float* sums, void* stream);
FR_API int fr_shard_loss_finish(const float* sums, const float* k_all, int32_t G, int64_t n_global, float fair_weight,
                                int32_t fair, float* loss, void* stream);
/* fr_bucket_by_owner for a list with EMPTY positions (id -1, the padding of a received exchange buffer): they are
 * given to no owner (slot -1) and raise no error. */
FR_API int fr_bucket_by_owner_sparse(const int64_t* idx, int64_t M, int32_t G, int32_t cap, int32_t stride, int32_t offset,
                                     int64_t* send_ids, int32_t* slot_of, int32_t* counts, uint32_t* err_flag, void* stream);
FR_API int fr_bucket_pair_by_owner(const int64_t* idx_a, const int64_t* idx_b, int64_t M, int32_t G, int32_t cap,
                                   int32_t stride, int32_t offset_a, int32_t offset_b, int64_t* send_ids,
                                   int32_t* slot_a, int32_t* slot_b, int32_t* counts, const float* aux,
                                   int32_t aux_slot, uint32_t* err_flag, void* stream);
/* out[j,:] = src[slot_of[j],:]  (reply buffer in slot order -> batch order) */
FR_API int fr_unbucket_rows(const float* src, const int32_t* slot_of, int64_t M, int32_t dim, float* out, void* stream);
/* dst[slot_of[j],:] = scale[j] * src[j,:]  (batch order -> slot order; scale may be NULL; dst pre-zeroed) */
FR_API int fr_bucket_rows(const float* src, const float* scale, const int32_t* slot_of, int64_t M, int32_t dim,
                          float* dst, void* stream);

/*
 * Row-sharded FOCF step (one rank's share of focf.py:152-169 on the GLOBAL batch = concatenation of all ranks'
 * batches).  Requester side works on the rows returned by the owners ([G*cap, dim] slot order):
 *   fr_focf_shard_score : pred, MSE part of dLoss/dpred (2(pred-r)/n_global), sum of squared errors (sq_err_sum; NULL:
 *                         only the (B+3)/4 per-workgroup partials in `scratch`, for fr_focf_shard_fair), and the
 *                         (pred, rating, sst) records for the item owners: rec = [G, 3, cap], record of item slot
 *                         s = o*slot_stride + slot_offset + k (as produced by fr_bucket_by_owner) at rec[o][0..2][k]
 *   fr_focf_shard_fair  : on the item OWNER, over the segments fr_table_gather_train left in the item table's
 *                         workspace: per-item group statistics of the received records ([G(src), 3, cap]) ->
 *                         fairness part of dLoss/dpred per slot, NOT yet divided by K, into the reply buffer
 *                         [G, cap + FR_SHARD_TAIL]; the tail of every chunk = (this owner's distinct items, its sum
 *                         of smooth-L1 terms, this rank's sum of squared errors = sum of sq_part[0..n_sq_part), the
 *                         partials fr_focf_shard_score left in its scratch), written by the last workgroup to
 *                         arrive, so the scalars of the loss ride along with the reply exchange (no all-reduce).
 *                         scratch: >= n_slots/64 + 32 floats, scratch[0] zero on first use (arrival ticket).
 *                         minmax: mm_count (min, max) pairs, mm_stride floats apart (one per source rank, as
 *                         delivered by fr_bucket_by_owner's aux slot), folded in the kernel
 *   fr_focf_shard_grads : gradient rows c*ie / c*ue written at the user / item slots for the owners.  coef_slots =
 *                         the RECEIVED reply buffer (NULL for fair_objective none): K, fairness sum and squared-error
 *                         sum are folded over its G tails in rank order (identical on every rank) and
 *                         loss_out[0..2] = loss, mse, fair is written (may be NULL)
 *   fr_focf_shard_nonparity_sums / _coef : fair_objective nonparity (focf.py:127-134) needs no item statistics, only
 *                         the two group means of pred over the GLOBAL batch: _sums leaves this rank's (sum err^2,
 *                         sum pred|g0, n0, sum pred|g1, n1) in out5 (one 5-float all-reduce makes them global); _coef
 *                         adds the fairness part of dLoss/dpred to coef[b] in place and writes loss_out[0..2]
 * rows_u / rows_i / grad_*_slots are addressed by slot, so both may point at one shared [G, 2, cap, dim] buffer.
 */
#define FR_SHARD_TAIL 3
FR_API int fr_focf_shard_score(const float* rows_u, const float* rows_i, const int32_t* slot_u, const int32_t* slot_i,
                               const float* rating, const float* sst, int64_t B, int32_t dim, int64_t n_global,
                               float* pred, float* coef, float* rec, int32_t cap, int32_t slot_stride,
                               int32_t slot_offset, float* sq_err_sum, float* scratch, void* stream);
FR_API int fr_focf_shard_fair(void* item_ws, size_t ws_bytes, int64_t n_slots, int32_t dim, const float* rec,
                              int32_t cap, const float* minmax, int32_t mm_count, int32_t mm_stride, int32_t objective,
                              float fair_weight, float* reply, const float* sq_part, int32_t n_sq_part, float* scratch,
                              uint32_t* err_flag, void* stream);
FR_API int fr_focf_shard_nonparity_sums(const float* pred, const float* sst, int64_t B, const float* minmax,
                                        int32_t mm_count, int32_t mm_stride, const float* sq_part, int32_t n_sq_part,
                                        float* out5, void* stream);
FR_API int fr_focf_shard_nonparity_coef(float* coef, const float* sst, int64_t B, const float* minmax, int32_t mm_count,
                                        int32_t mm_stride, const float* global5, int64_t n_global, float fair_weight,
                                        float* loss_out, uint32_t* err_flag, void* stream);
FR_API int fr_focf_shard_grads(const float* rows_u, const float* rows_i, const int32_t* slot_u, const int32_t* slot_i,
                               const float* coef, const float* coef_slots, int32_t G, int64_t n_global,
                               float fair_weight, float* loss_out, int32_t cap, int32_t slot_stride,
                               int32_t slot_offset, int64_t B, int32_t dim, float* grad_u_slots, float* grad_i_slots,
                               void* stream);

/* ---- dense layers (fp32 MFMA) ---------------------------------------------------------------------------
 * One layer of recbole/model/layers.py MLPLayers (:62-72): Dropout -> Linear -> activation, forward and backward.
 *   X = [x0 | x1] : [M, k0 + k1] (x1 may be NULL; the split serves cat(U[u], I[i]) of nfcf.py:72 without a copy)
 *   mask          : [M, k0 + k1] bytes, 0 = dropped (the Bernoulli draw stays with the host RNG),
 *                   NULL = no dropout; kept elements are multiplied by `scale` = 1/(1-p)
 *   W [N, K], bias [N] : nn.Linear layout;  act: 0 none, 1 relu, 2 leakyrelu(0.01), 3 sigmoid, 4 tanh
 *   Y [M, N]      : POST-activation output; the backward kernels rebuild act'(.) from it
 * fr_linear_bwd_weight reduces over the batch in a fixed order (per-split slabs summed in split order). */
FR_API int fr_linear_fwd(const float* x0, int32_t k0, const float* x1, int32_t k1, const uint8_t* mask, float scale,
                         const float* W, const float* bias, int64_t M, int32_t N, int32_t act, float* Y, void* stream);
FR_API int fr_linear_bwd_input(const float* dY, const float* Y, int32_t act, const float* W, const uint8_t* mask,
                               float scale, int64_t M, int32_t N, float* dx0, int32_t k0, float* dx1, int32_t k1,
                               void* stream);
FR_API size_t fr_linear_bwd_weight_workspace_bytes(int64_t M, int32_t N, int32_t K);
FR_API int fr_linear_bwd_weight(const float* dY, const float* Y, int32_t act, const float* x0, int32_t k0,
                                const float* x1, int32_t k1, const uint8_t* mask, float scale, int64_t M, int32_t N,
                                float* dW, float* db, void* ws, size_t ws_bytes, void* stream);
/* out[n] = dY o act'(Y), elementwise (n % 4 == 0, 16-byte aligned): the shared pre-pass of a layer's two backward
 * products (the autograd of the activation in layers.py:68-72), after which both are called with act = 0 and take
 * their fast form (LDS-DMA kernels: no dropout mask, act = 0, widths multiples of 32). */
/* Both backward products of a layer with ONE output (N == 1, one input block, no mask) in one pass over X: dW [K], db [1]
 * (may be NULL) and dX [M, K] (may be NULL) -- what fr_linear_bwd_weight + fr_linear_bwd_input give for that shape.
 * FR_EUNSUPPORTED unless K % 64 == 0, K <= 512 and X, W, dX are 16-byte aligned (take the two general calls then).
 * ws: fr_linear_bwd_weight_workspace_bytes(M, 1, K).
 * relu_scale > 0: X is the previous layer's ReLU output dropped in place (keep = 0 or relu_scale) and dX comes out as the
 * gradient at that layer's pre-activation (fr_act_bwd_dropped folded in); 0: plain dX. */
FR_API int fr_linear_n1_bwd(const float* dY, const float* Y, int32_t act, const float* X, int32_t K, const float* W, int64_t M,
                            float relu_scale, float* dX, float* dW, float* db, void* ws, size_t ws_bytes, void* stream);
/* dA = (dY W) o scale o [Xd > 0]: fr_linear_bwd_input followed by fr_act_bwd_dropped, in one launch, for a layer whose
 * input Xd [M, K] is the previous layer's ReLU output dropped in place.  Fast form only (FR_EUNSUPPORTED unless N % 32 == 0,
 * K % 32 == 0, 16-byte aligned operands). */
FR_API int fr_linear_bwd_input_relu(const float* dY, const float* W, int64_t M, int32_t N, int32_t K, const float* Xd,
                                    float scale, float* dA, void* stream);
/* dA = (dY W) o act'(Yin): fr_linear_bwd_input followed by the fr_act_bwd of the layer BELOW, in one launch: Yin [M, K] is this
 * layer's input = that layer's activation output (activation code `act`, 1..4), dA the gradient at its pre-activation --
 * the autograd of `activation(Linear(...))` between two Linear layers (recbole/model/layers.py:62-72) without a pass of its
 * own.  Same bits as the two calls.  Fast form only (FR_EUNSUPPORTED unless N % 32 == 0, K % 32 == 0, aligned operands). */
FR_API int fr_linear_bwd_input_act(const float* dY, const float* W, int64_t M, int32_t N, int32_t K, const float* Yin,
                                   int32_t act, float* dA, void* stream);
FR_API int fr_act_bwd(const float* dY, const float* Y, int32_t act, int64_t n, float* out, void* stream);
/* The same pre-pass through a ReLU whose OUTPUT went through dropout in place: Yd = relu(z) o keep (keep = 0 or scale),
 * dY = gradient with respect to Yd; out = dY o scale o [Yd > 0] = dY o keep o relu'(z).  Replaces the reference's
 * Dropout.backward + ReLU.backward pair between two Linear layers (recbole/model/layers.py:62-72). */
FR_API int fr_act_bwd_dropped(const float* dY, const float* Yd, float scale, int64_t n, float* out, void* stream);

/* ---- dropout without a stored mask (csrc/dropout.hip) ----------------------------------------------------------------
 * out[i] = x[i] * keep_i for i < n (in place allowed), keep_i = 0 with probability p, else 1/(1-p); keep_i is a pure
 * function (Philox4x32-10) of (seed, *counter, offset + i).  offset % 4 == 0; x, out 16-byte aligned.
 *   counter     device int64: the call counter to use.  A forward pass hands its state word; the backward pass the
 *               value that forward recorded, so that it regenerates the same pattern.
 *   used_out    optional device int64[1]: receives the counter value this launch used.
 *   tick_state  optional device int64[2] {counter, ticket}, ticket == 0 between launches: this launch advances the
 *               counter by one AFTER all of its workgroups have read it (pass it with the LAST launch of a forward pass,
 *               whose launches then all see the same value; `counter` must then be tick_state).
 * nn.Dropout of the reference's MLPLayers (recbole/model/layers.py:62-63); see DESIGN.md §8a. */
FR_API int fr_dropout_apply(const float* x, int64_t n, float p, uint64_t seed, uint64_t offset, const int64_t* counter,
                            int64_t* used_out, int64_t* tick_state, float* out, void* stream);
/* The same for two tensors in ONE launch (the two blocks [x0 | x1] of a first layer's input); x1 may be NULL. */
FR_API int fr_dropout_apply2(const float* x0, int64_t n0, uint64_t offset0, float* out0, const float* x1, int64_t n1,
                             uint64_t offset1, float* out1, float p, uint64_t seed, const int64_t* counter,
                             int64_t* used_out, int64_t* tick_state, void* stream);

/* The running loss total of a step loop that reads its losses once per epoch (trainer.py:184-193 reads `.item()` and checks
 * `isnan` every step: two host syncs per step).  acc = device float[8]: acc[0..n-1] += part[0..n-1] (n <= 3 loss values of this
 * step), acc[3] += 1 (steps so far), and the FIRST step whose loss was not a number is remembered in acc[4] (1-based, 0 =
 * none; sticky): the ValueError('Training loss is nan') raised at the epoch's end names the step the reference would have
 * stopped at.  The one-launch FOCF steps keep the same record in their `loss_acc` (csrc/focf_loss.hpp). */
FR_API int fr_loss_accumulate(const float* part, int32_t n, float* acc, void* stream);

/* n <= FR_COPY_MAX device-to-device copies of bytes[j] bytes in ONE launch (jobs must not overlap each other). */
#define FR_COPY_MAX 16
FR_API int fr_copy_many(const void* const* src, void* const* dst, const int64_t* bytes, int32_t n, void* stream);

/* BatchNorm1d on batch statistics between Linear and activation (MLPLayers(bn=True), layers.py:66-67; the PFCN filters
 * and discriminators, which the reference never puts in eval mode).  Z [M,N] -> Y = act(gamma * xhat + beta);
 * xhat [M,N] and invstd [N] are kept for fr_bn_bwd; running_mean/var (may be NULL) follow torch (momentum, unbiased).
 * ws (fr_bn_workspace_bytes) holds the per-row-chunk partial statistics of the two-launch reduction. */
FR_API size_t fr_bn_workspace_bytes(int64_t M, int32_t N);
FR_API int fr_bn_fwd(const float* Z, const float* gamma, const float* beta, float eps, float momentum,
                     float* running_mean, float* running_var, int64_t M, int32_t N, int32_t act, float* Y, float* xhat,
                     float* invstd, void* ws, size_t ws_bytes, void* stream);
/* fr_bn_fwd that also writes Yd = dropout(Y), the next layer's input, from its last launch: what
 * fr_dropout_apply(Y, M*N, p, seed, offset, counter, used_out, tick_state, Yd) would give (same pattern, same counter
 * protocol), without the extra pass.  N % 4 == 0; all tensors 16-byte aligned. */
FR_API int fr_bn_fwd_drop(const float* Z, const float* gamma, const float* beta, float eps, float momentum,
                          float* running_mean, float* running_var, int64_t M, int32_t N, int32_t act, float* Y, float* xhat,
                          float* invstd, void* ws, size_t ws_bytes, float* Yd, float p, uint64_t seed, uint64_t offset,
                          const int64_t* counter, int64_t* used_out, int64_t* tick_state, void* stream);
/* The product of a layer that has BatchNorm behind it with the BatchNorm's per-chunk statistics formed in the product's epilogue
 * (into `bn_ws`, fr_bn_workspace_bytes(M, N)), and fr_bn_fwd / fr_bn_fwd_drop as one entry that can skip its statistics launch
 * (`have_stats`): layers.py:64-67 in two BatchNorm launches instead of three.  fr_linear_fwd_bnstats: fast form only
 * (FR_EUNSUPPORTED otherwise: fr_linear_fwd + fr_bn_fwd then).  `num_batches_tracked` (may be NULL): the layer's int64 batch
 * counter, moved by `passes` in the same launch that updates the running statistics (nn.BatchNorm1d's bookkeeping). */
FR_API int fr_linear_fwd_bnstats(const float* x0, int32_t k0, const float* x1, int32_t k1, const float* W, const float* bias,
                                 int64_t M, int32_t N, float* Z, void* bn_ws, size_t bn_ws_bytes, void* stream);
FR_API int fr_bn_fwd_ex(const float* Z, const float* gamma, const float* beta, float eps, float momentum, float* running_mean,
                        float* running_var, int64_t M, int32_t N, int32_t act, float* Y, float* xhat, float* invstd, void* ws,
                        size_t ws_bytes, int32_t have_stats, float* Yd, float p, uint64_t seed, uint64_t offset,
                        const int64_t* counter, int64_t* used_out, int64_t* tick_state, int64_t* num_batches_tracked,
                        int32_t passes, void* stream);
FR_API int fr_bn_bwd(const float* dY, const float* Y, int32_t act, const float* xhat, const float* invstd,
                     const float* gamma, int64_t M, int32_t N, float* dZ, float* dgamma, float* dbeta, void* ws,
                     size_t ws_bytes, void* stream);
/* A BatchNorm layer's backward fed by the product above it (layers.py:62-70 in reverse: Linear_l's input gradient is the
 * gradient at the dropped output of BatchNorm layer l - 1): fr_linear_bwd_input_bnstats computes dX = (dY W) o keep -- the
 * dropout's pattern regenerated from (p, seed, element offset, the call counter value in `used`), p = 0: none -- stores it, and
 * leaves that layer's backward statistics per 32-row tile in bn_ws (fr_bn_workspace_bytes(M, K)); fr_bn_bwd_ex(have_stats = 1)
 * on dY = dX and the same bn_ws is then the apply launch alone: one launch where there were three (product, dropout,
 * statistics).  The tile sums are added in another order than fr_bn_bwd's statistics launch adds them (rounding-level
 * differences).  Fast form only: FR_EUNSUPPORTED unless N % 32 == 0, K % 32 == 0, 16-byte aligned operands, M <= 32768. */
FR_API int fr_linear_bwd_input_bnstats(const float* dY, const float* W, int64_t M, int32_t N, int32_t K, float* dX,
                                       const float* Yb, const float* xhat_b, int32_t act_b, void* bn_ws, size_t bn_ws_bytes,
                                       float p, uint64_t seed, uint64_t offset, const int64_t* used, void* stream);
FR_API int fr_bn_bwd_ex(const float* dY, const float* Y, int32_t act, const float* xhat, const float* invstd,
                        const float* gamma, int64_t M, int32_t N, float* dZ, float* dgamma, float* dbeta, void* ws,
                        size_t ws_bytes, int32_t have_stats, void* stream);

/* ---- PFCN scoring / losses (pfcn_pmf.py, pfcn_biasedmf.py, loss.py) -------------------------------------------------
 * fr_rowdot_*   : torch.mul(a, b).sum(-1) on gathered rows and its backward (da = g*b, db = g*a; either may be NULL)
 * fr_bpr        : BPRLoss, loss.py:45-47
 * fr_bpr_outer  : the same loss under PFCN_BiasedMF's [B] + [B,1] -> [B,B] broadcast (pfcn_biasedmf.py:192-195,
 *                 SURVEY.md App. B-1): mean over all (i,j) of -log(1e-10 + sigmoid(a_j + c_i)); nothing of size B^2 is stored
 * fr_softmax_ce : nn.CrossEntropyLoss (multi-class discriminators, pfcn_biasedmf.py:216) */
FR_API int fr_rowdot_fwd(const float* a, const float* b, int64_t B, int32_t dim, float* out, void* stream);
FR_API int fr_rowdot_bwd(const float* g, const float* a, const float* b, int64_t B, int32_t dim, float* da, float* db,
                         void* stream);
FR_API size_t fr_bpr_workspace_bytes(int64_t B, int32_t outer);
FR_API int fr_bpr(const float* pos, const float* neg, int64_t B, float* loss, float* dpos, float* dneg, void* ws,
                  size_t ws_bytes, void* stream);
FR_API int fr_bpr_outer(const float* a, const float* c, int64_t B, float* loss, float* da, float* dc, void* ws,
                        size_t ws_bytes, void* stream);
/* The same on the four columns themselves: a = pos - neg and c = pos_bias - neg_bias are formed in the kernel and the
 * gradients of all four come out (d_neg = -d_pos, d_neg_bias = -d_pos_bias): no elementwise launches around the loss. */
/* fr_bpr_outer_rect: the same term matrix for Nc rows (c) and Na columns (a) of possibly different batches, scaled by
 * `inv`: loss[0] = inv * sum_ij -log(1e-10 + sigmoid(a_j + c_i)); da [Na] / dc [Nc] (either may be NULL) = the column / row
 * sums of its derivative.  A row-sharded step evaluates its part of the GLOBAL batch's [G B, G B] matrix with it: own
 * columns against all rows (da), own rows against all columns (dc), inv = 1 / (G B)^2 (fairrec/functional.py). */
FR_API size_t fr_bpr_outer_rect_workspace_bytes(int64_t Na, int64_t Nc);
FR_API int fr_bpr_outer_rect(const float* a, int64_t Na, const float* c, int64_t Nc, float inv, float* loss, float* da,
                             float* dc, void* ws, size_t ws_bytes, void* stream);
FR_API int fr_bpr_outer2(const float* pos, const float* neg, const float* pos_bias, const float* neg_bias, int64_t B,
                         float* loss, float* d_pos, float* d_neg, float* d_pos_bias, float* d_neg_bias, void* ws,
                         size_t ws_bytes, void* stream);
/* Row dots with the rows of a [A, dim] reused by `reps` row blocks of b [reps*A, dim] (a user row against its positive and
 * its negative item row of one [2B, dim] lookup): out[r*A + i] = a[i] . b[r*A + i];
 * da[i] = sum_r g[r*A + i] b[r*A + i] (in r order), db[r*A + i] = g[r*A + i] a[i]; da or db may be NULL. */
FR_API int fr_rowdot_rep_fwd(const float* a, const float* b, int64_t A, int32_t reps, int32_t dim, float* out, void* stream);
FR_API int fr_rowdot_rep_bwd(const float* g, const float* a, const float* b, int64_t A, int32_t reps, int32_t dim, float* da,
                             float* db, void* stream);
/* fr_rowdot_rep_bwd with the gradient of `a` left unsummed: da_sep[r*A + i] = g[r*A + i] b[r*A + i] ([reps*A, dim]) -- what
 * `reps` fr_rowdot_bwd calls write, in one launch, for a caller whose autograd graph adds the parts up in its own order (the
 * reference's two torch.mul(u, i).sum(-1) nodes, pfcn_pmf.py:182-183). */
FR_API int fr_rowdot_rep_bwd_sep(const float* g, const float* a, const float* b, int64_t A, int32_t reps, int32_t dim,
                                 float* da_sep, float* db, void* stream);
FR_API int fr_softmax_ce(const float* logits, const int64_t* label, int64_t M, int32_t C, float* loss, float* dlogits,
                         void* ws, size_t ws_bytes, uint32_t* err_flag, void* stream);

/* ---- FairGo graph ops (fairgo_pmf.py / fairgo_gcn.py) -----------------------------------------------------------
 * fr_spmm_csr        : Y = L X for a CSR matrix (torch.sparse.mm at fairgo_pmf.py:198 with L = D^-1 A, :102-129); the
 *                      backward is the same call on the CSR of L^T
 * fr_row_gather      : out[j,:] = X[idx[j],:]           (`all_embeddings[user]`, fairgo_pmf.py:178-179, :194)
 * fr_row_scatter_sum : its backward as a dense [n_rows, dim] gradient, duplicates summed in ascending position
 * fr_mse             : nn.MSELoss (fairgo_pmf.py:182): loss[0], dpred = 2 (pred - target) / B */
FR_API int fr_spmm_csr(const int64_t* indptr, const int32_t* col, const float* val, const float* X, int64_t n_rows,
                       int32_t dim, float* Y, void* stream);
/* fr_spmm_csr_sel : the same product where the batch can see it (the frontier-restricted propagation of
 *                   fairgo_pmf.py:196-200, :204-216): Y[i,:] = sum_j val[j] * X[xrow(col[j]),:] over the nonzeros of row
 *                   rows[i] (rows == NULL: row i) in ascending j, xrow(c) = map ? map[c] : c, nonzeros with map[c] < 0
 *                   skipped.  `rows` (int32 [n_out]) makes Y compact; `map` (int32 [number of columns]) lets X be a compact
 *                   block of a whole-table operand or, on the CSR of L^T, names the columns that carry a gradient row.
 *                   `map_bits` (optional, uint32 [ceil(columns / 32)]): bit c set exactly where map[c] >= 0 -- the kernel
 *                   then reads the map only at set bits (the bitmap of 11 M columns is 1.4 MB and lives in every L2; the
 *                   map is 44 MB).  Kept terms are added in fr_spmm_csr's order: the rows equal the whole-table product's. */
FR_API int fr_spmm_csr_sel(const int64_t* indptr, const int32_t* col, const float* val, const float* X, const int32_t* rows,
                           int64_t n_out, const int32_t* map, const uint32_t* map_bits, int32_t dim, float* Y, void* stream);
FR_API int fr_row_gather(const float* X, const int64_t* idx, int64_t M, int64_t n_rows, int32_t dim, float* out,
                         uint32_t* err_flag, void* stream);
FR_API size_t fr_row_scatter_workspace_bytes(int64_t M);
FR_API int fr_row_scatter_sum(const float* g, const int64_t* idx, int64_t M, int64_t n_rows, int32_t dim, float* dX,
                              void* ws, size_t ws_bytes, uint32_t* err_flag, void* stream);
/* ... ADDED into a dX that already holds another contribution to the same gradient (no clear): the backward of a table that
 * is both row-gathered and propagated (fairgo_pmf.py:178-201) then costs one dense [n_rows, dim] pass instead of three. */
FR_API int fr_row_scatter_add(const float* g, const int64_t* idx, int64_t M, int64_t n_rows, int32_t dim, float* dX,
                              void* ws, size_t ws_bytes, uint32_t* err_flag, void* stream);
/* The same two calls when the table they differentiate is the OUTPUT of an activation (FairGo's filtered table,
 * fairgo_pmf.py:173-185 through layers.py:62-72) and what is wanted is the gradient at the activation's INPUT: every output
 * row goes on through act'(act_src[row]) (act = 1 relu, 2 leaky relu, 3 sigmoid, 4 tanh; the derivative through the output,
 * as fr_act_bwd takes it) inside the launches -- a row no term reaches is stored as zeros without reading act_src, a row whose
 * bit in `skip_bits` (uint32 [ceil(n_out / 32)], optional) is set is left unscaled for fr_row_scatter_add_act, which scales
 * the rows of `idx` after it has added to them.  Together: (L^T dY + scatter(g)) o act'(act_src), bit for bit what
 * fr_spmm_csr_sel, fr_row_scatter_add and fr_act_bwd give in three whole-table passes. */
FR_API int fr_spmm_csr_sel_act(const int64_t* indptr, const int32_t* col, const float* val, const float* X, const int32_t* rows,
                               int64_t n_out, const int32_t* map, const uint32_t* map_bits, int32_t dim, float* Y,
                               const float* act_src, int32_t act, const uint32_t* skip_bits, void* stream);
FR_API int fr_row_scatter_add_act(const float* g, const int64_t* idx, int64_t M, int64_t n_rows, int32_t dim, float* dX,
                                  void* ws, size_t ws_bytes, const float* act_src, int32_t act, uint32_t* err_flag, void* stream);
FR_API int fr_mse(const float* pred, const float* target, int64_t B, float* loss, float* dpred, void* ws, size_t ws_bytes,
                  void* stream);

/* ---- NFCF (nfcf.py) ---------------------------------------------------------------------------------------
 * Loss head of NFCF.calculate_loss, nfcf.py:99-110: y [B] is the scorer MLP's output AFTER its last ReLU
 * (layers.py:63-70); out = sigmoid(y) (:73); loss = BCELoss(out, label) (:105) [+ fair_weight * differential
 * fairness over the label==1 rows (:76-97) when `item_ws` != NULL, i.e. when fine-tuning].  `item_ws` is the
 * item table's workspace after fr_table_gather_train on the batch's item ids (its segments = torch.unique(item)).
 * Writes out [B], dy [B] = dLoss/dy (the scorer's backward starts from it), loss[3] = (loss, bce, df). */
FR_API size_t fr_nfcf_loss_workspace_bytes(int64_t B);
FR_API int fr_nfcf_loss(const float* y, const float* label, const float* sst, int64_t B, float fair_weight, void* item_ws,
                        size_t item_ws_bytes, int32_t dim, float* out, float* dy, float* loss, void* ws, size_t ws_bytes,
                        uint32_t* err_flag, void* stream);

/* The same loss head behind the fused scorer (fr_scorer_fwd below), which has already written out, the BCE share of dy and the
 * per-workgroup partials: bce_part [n_part] (sums of the rows' BCE terms) and, with `sst`, mm_part [n_part, 2] ((min, max)
 * of the attribute over each workgroup's positive rows).  Adds the differential-fairness share to dy (when item_ws != NULL)
 * and writes loss[3]; ws as for fr_nfcf_loss. */
FR_API int fr_nfcf_loss_tail(const float* label, const float* sst, int64_t B, float fair_weight, void* item_ws,
                             size_t item_ws_bytes, int32_t dim, const float* out, float* dy, float* loss,
                             const float* bce_part, const float* mm_part, int32_t n_part, void* ws, size_t ws_bytes,
                             uint32_t* err_flag, void* stream);

/* ---- the NFCF scorer in one forward and one backward launch (csrc/scorer.hip) ----------------------------------------
 * MLPLayers([k0 + k1, n1, n2, 1], dropout p) on cat(x0, x1) (nfcf.py:40, :68-73; layers.py:56-85: per layer Dropout ->
 * Linear -> ReLU, the last layer included).  Shapes: k0 == k1, multiples of 32, k0 + k1 <= 512; n1 in 32..128, n2 in 32..64,
 * multiples of 32 (fr_scorer_supported; the layer-by-layer entry points above cover everything else).  Dropout is
 * fr_dropout_apply's generator: `off_*` are the element offsets of the four dropped tensors inside the call's pattern
 * (the layered form's: x0 at 0, x1 behind it, then the two hidden activations), `counter` / `used_out` / `tick_state` as
 * there (the forward is the pattern's first and last launch).
 *   fr_scorer_fwd  x0d / x1d [B, k] = the dropped inputs (p > 0 only; what the weight gradient multiplies), h1 [B, n1],
 *                  h2 [B, n2] = the dropped hidden activations, y [B] = the output after its ReLU.  With `label`: out =
 *                  sigmoid(y), dy = d mean(BCE) / dy, bce_part / mm_part [fr_scorer_blocks(B)] (see fr_nfcf_loss_tail);
 *                  `loss` != NULL (no fairness term follows: the pre-training stage): loss[3] = (mean BCE, mean BCE, 0),
 *                  written by the launch's last workgroup -- no fr_nfcf_loss_tail call then.  `ticket` (needed with `loss`)
 *                  is that launch's arrival counter: one device word, 0 on entry, which the last workgroup returns to 0 --
 *                  launches that may run at the same time (other streams, other host threads) each need their own.
 *   fr_scorer_bwd  from dy (times gscale[0] when given): dz3 [B], dz2 [B, n2], dz1 [B, n1] = the gradients at the three
 *                  pre-activations, dx0 / dx1 = the input blocks' gradients (either may be NULL: a frozen table), w3part
 *                  [fr_scorer_blocks(B), n2 + 1] = per-workgroup shares of (dW3 | db3), summed by fr_parts_sum.
 *                  dW1 / db1 = fr_linear_bwd_weight(dz1, x0d | x1d), dW2 / db2 = fr_linear_bwd_weight(dz2, h1). */
typedef struct fr_scorer {
    int32_t k0, k1, n1, n2;
    const float *W1, *b1, *W2, *b2, *W3, *b3;
    float p;
    uint64_t seed;
    uint64_t off_x0, off_x1, off_h1, off_h2;
} fr_scorer;
FR_API int fr_scorer_supported(const fr_scorer* s);
FR_API int64_t fr_scorer_blocks(int64_t B);
FR_API int fr_scorer_fwd(const fr_scorer* s, const float* x0, const float* x1, int64_t B, const int64_t* counter,
                         int64_t* used_out, int64_t* tick_state, float* x0d, float* x1d, float* h1, float* h2, float* y,
                         const float* label, const float* sst, float* out, float* dy, float* bce_part, float* mm_part,
                         float* loss, uint32_t* ticket, void* stream);
FR_API int fr_scorer_bwd(const fr_scorer* s, const float* dy, const float* gscale, const float* y, const float* h1,
                         const float* h2, int64_t B, const int64_t* used, float* dz1, float* dz2, float* dz3, float* dx0,
                         float* dx1, float* w3part, void* stream);
/* The weight gradients of several layers in two launches (every product, then every slab sum): job = fr_linear_bwd_weight's
 * (dY at the pre-activation, x0 | x1, N) -> dW [N, k0 + k1], db [N] (may be NULL), fast form only (N, k0, k0 + k1 multiples
 * of 32, 16-byte aligned; FR_EUNSUPPORTED otherwise).  A job with dY == NULL sums `n_parts` partial results
 * parts[n_parts][N * (k0 + k1)] into dW (the scorer's last layer: fr_scorer_bwd's w3part).  At most FR_WGRAD_MAX jobs. */
#define FR_WGRAD_MAX 8
typedef struct fr_wgrad_job {
    const float* dY;
    const float* x0;
    int32_t k0;
    const float* x1;
    int32_t k1;
    int32_t N;
    float* dW;
    float* db;
    const float* parts;
    int32_t n_parts;
} fr_wgrad_job;
FR_API size_t fr_linear_bwd_weight_multi_workspace_bytes(const fr_wgrad_job* jobs, int32_t n, int64_t M);
FR_API int fr_linear_bwd_weight_multi(const fr_wgrad_job* jobs, int32_t n, int64_t M, void* ws, size_t ws_bytes, void* stream);
/* out[i] = sum over the parts p of part[p * n + i], in a fixed order (64 interleaved ascending chains, then a butterfly) */
FR_API int fr_parts_sum(const float* part, int32_t parts, int64_t n, float* out, void* stream);

/* The differential-fairness term (nfcf.py:76-97) of a ROW-SHARDED step on the GLOBAL batch (one process per GPU, item
 * table row r on rank r mod G): M[k, g], K and the mean of eps are statistics of the whole batch, so every positive row's
 * (score, attribute) travels to the owner of its item and the per-(item, group) sums come back -- two all-to-alls that
 * the caller issues between the three launches below.  Both buffers have one chunk of `cap` slots + 1 tail per peer:
 *   rec   [G, cap + 1, 2] floats  slot = (sigmoid score, or -1 where label != 1; attribute), tail = the sender's (min, max)
 *                                 of the attribute over its positive rows
 *   reply [G, cap + 1, 4] floats  slot = (S0 with the sign bit set on the ONE member that reports the item's eps, S1, n0, n1),
 *                                 tail = (K_owner = owned items with a positive row, smin, smax, 0)
 * A row's slot is the one its item id took in the lookup's id exchange: slot[b] = o * slot_stride + slot_off + k
 * (fr_bucket_by_owner), i.e. chunk o, position k.
 *   fr_nfcf_df_pack  (requester) writes the records of this rank's B rows and the tails.
 *   fr_nfcf_df_owner (owner) reduces over the segments of the ids it received (`item_ws` = the item table's workspace after
 *                    fr_table_gather_train on the G * cap received slots; members in rank order, then batch position = the
 *                    order of the concatenated batch) and writes the reply.
 *   fr_nfcf_df_apply (requester) K = sum of the tails' K_owner; M = (S + 1/K) / (n + 1); eps = |log M0 - log M1|;
 *                    dy[b] += scale * fair_weight * d(mean eps)/d score_b * out_b (1 - out_b); loss[0] += fair_weight *
 *                    scale * (sum of the eps this rank reports) / K, loss[2] = that DF share.  scale = G where the caller
 *                    averages the ranks' gradients and losses (the DF term is not a per-rank mean).
 * `ws` (fr_nfcf_df_workspace_bytes(B, G * cap), ZERO-initialised once, reusable) holds partial sums and arrival tickets. */
FR_API size_t fr_nfcf_df_workspace_bytes(int64_t B, int64_t n_slots);
FR_API int fr_nfcf_df_pack(const float* out, const float* label, const float* sst, const int32_t* slot, int32_t slot_stride,
                           int32_t slot_off, int32_t cap, int64_t B, int32_t G, float* rec, void* ws, size_t ws_bytes,
                           void* stream);
FR_API int fr_nfcf_df_owner(void* item_ws, size_t item_ws_bytes, int32_t dim, const float* rec, int32_t G, int32_t cap,
                            float* reply, void* ws, size_t ws_bytes, int64_t B, uint32_t* err_flag, void* stream);
FR_API int fr_nfcf_df_apply(const float* reply, const int32_t* slot, int32_t slot_stride, int32_t slot_off, int32_t cap,
                            int32_t G, const float* out, const float* label, const float* sst, int64_t B, float fair_weight,
                            float scale, float* dy, float* loss, void* ws, size_t ws_bytes, void* stream);

/* Dense fused Adam step for small dense parameters (MLP weights, biases): one step of
 * torch.optim.Adam on a flat fp32 tensor, `step` = the step being applied. */
FR_API int fr_adam_dense(float* p, const float* g, float* m, float* v, int64_t n, const fr_adam* adam, int32_t step,
                  void* stream);
/* The same for many tensors at once (all dense parameters of an optimizer group: one launch per FR_ADAM_DENSE_MAX tensors
 * instead of one per tensor); every tensor keeps its own step counter, as torch.optim.Adam's per-parameter state does. */
#define FR_ADAM_DENSE_MAX 48
typedef struct fr_dense_desc {
    float* p;
    const float* g;
    float* m;
    float* v;
    int64_t n;
    int32_t step;
    const int32_t* step_dev;   /* optional device counter, as fr_table.step_dev: effective step = *step_dev + step */
} fr_dense_desc;
FR_API int fr_adam_dense_multi(const fr_dense_desc* descs, int32_t n_tensors, const fr_adam* adam, void* stream);

/* ---- negative sampler (next-row f-1: the batch feed), bit-exact with the reference's host sampler ---------------
 * state: numpy's legacy RandomState layout in device memory, uint32 key[624] followed by uint32 pos (625 words), so the
 * stream can be exchanged with np.random.get_state() / set_state() at any point.
 *   fr_mt19937_seed     : np.random.seed(seed)                          (numpy mt19937_seed)
 *   fr_sample_negatives : Sampler.sample_by_user_ids, sampler.py:283-303 -> sample_by_key_ids :145-197 with
 *                         _uni_sampling = np.random.randint(low, high, .) :240-241:
 *                         out[j] for j in [0, n_keys*num) is drawn for key key_ids[j % n_keys]; draw all, then re-draw
 *                         -- from the continuing stream, in ascending position order -- exactly the positions whose
 *                         value is in the key's used-set, until none is left (rounds_out[0] = number of rounds).
 *                         used-set of key u = used_items[used_indptr[u] .. used_indptr[u+1]) sorted ascending.
 *                         used_indptr = NULL: plain np.random.randint(low, high, n_keys*num) (key_ids unused).
 *                         high - 1 - low < 2^32 - 1 (numpy then draws single 32-bit words, masked rejection).
 * One workgroup per call; the state after the call is exactly numpy's, so calls chain without host syncs.
 *   fr_sample_negatives_calls : a SEQUENCE of single-key calls on one stream in one launch: call c fills
 *                         out[call_offsets[c] .. call_offsets[c+1]) for key call_keys[c] and completes its re-draw rounds
 *                         before call c+1 draws -- the evaluation loader's user-by-user sampling
 *                         (general_dataloader.py:141-146).  max_call >= the longest call (sizes the workspace). */
FR_API int fr_mt19937_seed(uint32_t* state, uint32_t seed, void* stream);
FR_API size_t fr_sample_negatives_workspace_bytes(int64_t total);
/* ... for fr_sample_negatives_calls: with this much workspace (`total` = values of the whole sequence) a sequence of 16 or more
 * calls is resolved SPECULATIVELY -- the stream's accepted values generated once, every call laid out as if none before it
 * had collided with its used-set, the rare colliding call resolved round by round and the rest shifted (csrc/sampler.hip) --
 * instead of call by call: the same values and the same generator state, 30 ms -> ~1.5 ms for the ~2 800 calls of an
 * evaluation batch.  With fr_sample_negatives_workspace_bytes(max_call) bytes the calls run one after the other.  The host
 * can not read `total` (call_offsets[n_calls] is device memory), so it lays the workspace out for the largest total it holds:
 * a workspace of this size for a smaller total than the sequence's -- room for n_calls values or more but fewer than the
 * sequence draws -- is accepted, and the calls then run one after the other from the incoming state (the same values and
 * state, at the call-by-call speed).  ws_bytes must also be >= fr_sample_negatives_workspace_bytes(max_call). */
FR_API size_t fr_sample_negatives_calls_workspace_bytes(int64_t total, int64_t max_call);
FR_API int fr_sample_negatives(uint32_t* state, int64_t low, int64_t high, const int64_t* key_ids, int64_t n_keys,
                               int32_t num, const int64_t* used_indptr, const int32_t* used_items, int64_t n_users,
                               int64_t* out, int32_t* rounds_out, void* ws, size_t ws_bytes, uint32_t* err_flag,
                               void* stream);
FR_API int fr_sample_negatives_calls(uint32_t* state, int64_t low, int64_t high, const int64_t* call_keys,
                                     const int64_t* call_offsets, int64_t n_calls, int64_t max_call,
                                     const int64_t* used_indptr, const int32_t* used_items, int64_t n_users, int64_t* out,
                                     void* ws, size_t ws_bytes, uint32_t* err_flag, void* stream);
/* Popularity-biased negatives: Sampler._pop_sampling (the alias method, sampler.py:72-118) inside the same rejection loop.
 * The table is the reference's, built on the host in float64 (fairrec/sampler/sampler.py _build_alias_table): n keys in
 * insertion order, prob[i] and alias[i] of key keys[i] (alias -1 = none, copied into the output as numpy does).
 * A round over the m positions still open draws idx = np.random.randint(0, n, m) (no words when n == 1), then
 * coin = np.random.random(m) (2m raw words, fp64), value = keys[idx] if prob[idx] > coin else alias[idx]; the positions
 * whose value is in the key's used-set, ascending, form the next round.
 *   fr_sample_negatives_pop       : fr_sample_negatives' semantics with that draw (used_indptr = NULL: a plain
 *                                   _pop_sampling(n_keys * num), key_ids unused); workspace fr_sample_negatives_workspace_bytes(
 *                                   n_keys * num).
 *   fr_sample_negatives_pop_calls : fr_sample_negatives_calls' semantics with that draw, the calls one after the other in one
 *                                   launch; workspace fr_sample_negatives_workspace_bytes(max_call).  A call longer than
 *                                   max_call is skipped with FR_DEV_ERR_INDEX_RANGE.
 * A call that is still open after 2^20 rounds ends the launch with FR_DEV_ERR_SAMPLE_ROUNDS (a used-set covering every key
 * never terminates in the reference; the host refuses it before launching).  FR_EINVAL for a null table pointer, n < 1,
 * n - 1 >= 2^32 - 1, bad sizes or a workspace that is too small. */
typedef struct fr_alias_table {
    const int64_t* keys;
    const double* prob;
    const int64_t* alias;
    int64_t n;
} fr_alias_table;
FR_API int fr_sample_negatives_pop(uint32_t* state, const fr_alias_table* table, const int64_t* key_ids, int64_t n_keys,
                                   int32_t num, const int64_t* used_indptr, const int32_t* used_items, int64_t n_users,
                                   int64_t* out, int32_t* rounds_out, void* ws, size_t ws_bytes, uint32_t* err_flag,
                                   void* stream);
FR_API int fr_sample_negatives_pop_calls(uint32_t* state, const fr_alias_table* table, const int64_t* call_keys,
                                         const int64_t* call_offsets, int64_t n_calls, int64_t max_call,
                                         const int64_t* used_indptr, const int32_t* used_items, int64_t n_users, int64_t* out,
                                         void* ws, size_t ws_bytes, uint32_t* err_flag, void* stream);

/* ---- the row sets of a frontier-restricted propagation (csrc/frontier.hip) -----------------------------------------------------
 * Which rows of H_l = L H_(l-1) a batch can see (fairgo_pmf.py:196-216 aggregates every layer's rows of the batch's users): the
 * sets fr_spmm_csr_sel takes.  A set is a bitmap over the graph rows (bits: (n_rows + 31) / 32 words, zeroed by the caller):
 * fr_frontier_mark sets the bits of an id list (ids outside [0, n_rows) raise FR_DEV_ERR_INDEX_RANGE), fr_frontier_expand the
 * bits of the columns of the listed rows of a CSR matrix, fr_frontier_count writes popcount(bits[w]) per word, and -- given the
 * inclusive cumulative sum of those counts -- fr_frontier_scatter writes the set's row ids in ascending order (rows_out) and
 * pos[row] = rank of the row in the set, -1 outside it (pos: n_rows entries, every one written). */
FR_API int fr_frontier_mark(const int64_t* ids, int64_t n, int64_t n_rows, uint32_t* bits, uint32_t* err_flag, void* stream);
FR_API int fr_frontier_expand(const int64_t* indptr, const int32_t* col, const int32_t* rows, int64_t n_list, uint32_t* bits,
                              void* stream);
FR_API int fr_frontier_count(const uint32_t* bits, int64_t n_rows, int32_t* count, void* stream);
FR_API int fr_frontier_scatter(const uint32_t* bits, const int32_t* incl, int64_t n_rows, int32_t* rows_out, int32_t* pos,
                               void* stream);

/* ---- FOCF's item-complete batcher (next-row f-3): the picks of a whole epoch in one HOST call ---------------------------------
 * focf_dataloader.py:37-51 composes a batch by `np.random.choice(select_item[is_select], 1, False)` per picked item: numpy's
 * legacy choice permutes the whole candidate list per pick and reads one element.  fr_focf_compose_epoch makes the same draws
 * from the same stream (state: numpy's legacy layout key[624] + pos in HOST memory, advanced in place) and returns the same
 * picks without building the permutations (csrc/focf_compose.hip).  item_uniques [n_uniq] ascending, indptr [n_items + 1] the
 * CSR of the item-sorted interaction table, `pr` / `pr_end` / `step` the loader's counters; picks_out [cap] the picked items,
 * batch_end_out[b] the number of picks up to and including batch b.  No device work, no stream. */
FR_API int fr_focf_compose_epoch(uint32_t* state, const int64_t* item_uniques, int64_t n_uniq, const int64_t* indptr,
                                 int64_t step, int64_t pr, int64_t pr_end, int64_t* picks_out, int64_t cap,
                                 int64_t* batch_end_out, int64_t max_batches, int64_t* n_batches_out);

/* ---- epoch shuffle (next-row f-1: the batch feed): torch.randperm(n) on the device, bit-exact ---------------------------
 * Replaces the `torch.randperm(self.length)` behind Interaction.shuffle (interaction.py:293-297), the training loader's
 * per-epoch shuffle (abstract_dataloader.py:81-84).  Underneath: ATen's randperm_cpu for n < 2^32 / 20 -- r[i] = i, then for
 * i = 0 .. n-2: swap(r[i], r[i + mt19937() % (n - i)]) on single 32-bit outputs of torch's CPU generator (the standard
 * MT19937).  state: uint32 key[624] followed by uint32 pos (625 words; pos = index of the next unused word, 624 = regenerate
 * first), taken from torch.get_rng_state() by the caller and left where the n - 1 draws put it, so the host generator can be
 * set to exactly the state torch.randperm(n) would have left.  out: int64 [n].  The swap chain is resolved in parallel
 * (csrc/randperm.hip); only the generator is walked sequentially, by one workgroup. */
FR_API size_t fr_randperm_workspace_bytes(int64_t n);
FR_API int fr_randperm(uint32_t* state, int64_t n, int64_t* out, void* ws, size_t ws_bytes, void* stream);

/* ---- evaluation metrics (next-row f-2), recbole/evaluator/metrics.py ------------------------------------------------
 *   fr_topk_metrics           : rec_topk int32 [n_users, k+1] = hit flags of the ranked list | number of positives
 *                               (collector.py:146-154) -> out[6][k] doubles = Hit, MRR, NDCG, Recall, Precision, MAP
 *                               @ 1..k, means over users (metrics.py:40-232).  A hit flag is any non-zero value.  A row
 *                               with zero positives: NDCG 0 (divided by the ideal DCG of all k ranks, where the
 *                               reference's index wraps), MAP 0, Recall 0 / 0 = NaN as the reference -- and then every
 *                               Recall@j of the call is NaN
 *   fr_group_sums             : stats[s][g][0..2] = sum value, count, sum wtrue over the members
 *                               perm[seg_start[s] .. seg_start[s+1]) of segment s whose group index is g (perm = NULL:
 *                               identity; wtrue = NULL: the third sum is 0).  A group no member of the segment has:
 *                               0, 0, 0; an empty segment: all zeros.  A member whose group index is outside
 *                               [0, n_groups) is counted in no cell.  1 <= n_groups <= 8.  The (item, group) tables of
 *                               the fairness metrics (:948-970, :1322-1335)
 *   fr_fair_metrics_from_stats: out[0..4] = Value, Absolute, Under, Over unfairness (n_groups == 2; `+ 1e-5` counts as
 *                               the reference) and DifferentialFairness (float32 table, alpha = 1/n_segments) as means
 *                               over the segments (:972-979, :1068-1075, :1164-1171, :1260-1267, :1337-1342).  Any
 *                               other n_groups: out[0..3] = 0.  DifferentialFairness per segment = the largest
 *                               |logf(a) - logf(b)| over the pairs of table entries; a pair whose difference is NaN (the
 *                               logarithm of a non-positive entry, i.e. a negative score sum) does not enter the maximum
 *                               and the result stays finite (numpy's maximum in the reference's formula gives NaN there)
 *   fr_df_cells               : DifferentialFairness for ANY number of groups, out[0] (double) = what fr_group_sums +
 *                               fr_fair_metrics_from_stats give in out[4], without an [items, groups] table: memory is
 *                               O(members + items).  Positions j in [item_start[k], item_start[k+1]) are the members of
 *                               item k, member b = perm[j] (perm = NULL: identity); group[b] (int32) and value[b] (float)
 *                               are indexed by member.  Inside an item's range the members must be SORTED by group, or at
 *                               least the members of one group contiguous (a run): the caller's sort of the key
 *                               item * n_groups + group gives that; a group split into two runs counts as two cells.
 *                               A run whose group index is outside [0, n_groups) forms no cell.  Per run: s = sum of
 *                               value in double, c = its members; table entry a = (float)((s + 1.0 / n_items) / (c + 1.0)).
 *                               A group without a run in the item: the entry (float)(1.0 / n_items).  Per item: l =
 *                               logf(a) over its entries, the absent entry once if fewer than n_groups groups have a run,
 *                               NaN logarithms left out; d = lmax - lmin in float32, eps = d > 0 ? d : 0 -- the largest
 *                               |logf(a) - logf(b)| over the pairs, as float32 subtraction is monotone, with the rule
 *                               above for NaN pairs.  out[0] = mean over the n_items items of (double)eps.  n_groups == 1:
 *                               exactly +0.0.  An empty item range has the absent entry only: eps = 0.
 *                               1 <= n_items, 1 <= n_groups <= INT32_MAX; ws of fr_df_cells_workspace_bytes(n_items) bytes
 *                               (0 for n_items < 1)
 *   fr_topk_metrics_grouped   : fr_topk_metrics per GROUP of users, groups as segments: the members of group g are the rows
 *                               perm[group_start[g] .. group_start[g+1]) of rec_topk (perm int64 [n_users], NULL = identity;
 *                               group_start int64 [n_groups + 1] on the device, ascending, [0] = 0, [n_groups] = n_users).
 *                               out[g][6][k] = the mean over group g's members of the per-user terms fr_topk_metrics averages,
 *                               rows in its order.  A group with a zero-positive row: Recall NaN in that group only (NDCG and
 *                               MAP of the row 0, as above); an empty group: NaN everywhere.  Any n_groups >= 1.
 *                               SUMMATION ORDER (a contract): group g's range is cut into chunks of 64 consecutive positions,
 *                               lane = position within the chunk; a chunk is reduced by the xor butterfly (offsets 32, 16, ..,
 *                               1); the chunk sums are added in ascending chunk order from 0.0; the result is multiplied by
 *                               1.0 / (double)n_g.  With one group and the identity permutation (NULL or explicit) that is
 *                               fr_topk_metrics' order and the two entries return the same bits.
 *                               group_start and perm are clamped into [0, n_users]: a malformed table gives unspecified values
 *                               and no access outside rec_topk.  ws: fr_topk_metrics_grouped_workspace_bytes(n_users, k,
 *                               n_groups) bytes; the group sizes are never read on the host.
 *   fr_gauc_grouped           : GAUC's sums per group from the `rec.meanrank` triples { 2 * pos_rank_sum, user_len, pos_len }
 *                               (int64 [n_users][3]), groups as above.  A user without a positive (pos_len == 0) or without a
 *                               negative (user_len == pos_len) is dropped; for the others auc_u = pair / ((user_len - pos_len)
 *                               * pos_len), pair = (user_len + 1) * pos_len - pos_len * (pos_len + 1) / 2 - pos_rank_sum,
 *                               integers up to the one division.  out[g] = { sum of auc_u * pos_len, sum of pos_len } (the
 *                               caller divides; both 0 when every user of the group is dropped), kept[g] = { users kept,
 *                               dropped for no positive, dropped for no negative }.  The chunks and the order of
 *                               fr_topk_metrics_grouped, without the last multiplication.
 * Double-precision sums in a fixed order, no floating-point atomics: the same input gives the same bits on every call.
 * FR_EINVAL (null pointer -- other than a perm that may be NULL --, a size below 1, n_groups outside 1..8 -- fr_df_cells and
 * the *_grouped entries: below 1 --, workspace below *_workspace_bytes) is returned before anything is launched or written;
 * the *_workspace_bytes functions return 0 for arguments out of range. */
/* fr_eval_hits: the `rec.topk` matrix of a batch of users (collector.py:146-154): rec_topk int32 [n_rows, k+1], entry
 * [u][j] = 1 if topk_idx[u][j] (the j-th ranked item id of row u) is a positive of row u, [u][k] = its number of
 * positives.  pos_keys = the sorted keys row * n_items + item of the batch's positives (no dense 0/1 matrix; may be NULL
 * when n_pos == 0; distinct: a key listed twice counts twice in [u][k]).  List entries are item ids in [0, n_items); an entry outside that range is never a hit (its key would
 * lie in another row's range).  FR_EINVAL (null pointer, n_rows, k or n_items below 1, n_pos < 0) before any launch. */
FR_API int fr_eval_hits(const int64_t* topk_idx, int64_t n_rows, int32_t k, int64_t n_items, const int64_t* pos_keys,
                        int64_t n_pos, int32_t* rec_topk, void* stream);
/* fr_eval_topk_segments: the ranked lists of an evaluation batch under the uniN protocol (trainer.py:441-456 + collector.py:149).
 * User row u's candidates are rows [seg_start[u], seg_start[u+1]) of the batch (items int64, scores float); topk_idx int64
 * [n_users, k] = its k best DISTINCT items, best first, padded with 0; flags int32 [n_users]: bit 0 = two of its first k + 1
 * entries score equal (rank that row with fr_topk_like_torch_cpu), bit 1 = fewer than k + 1 distinct candidates.  1 <= k <= 62.
 * fr_eval_lookup_segments: out[q] = the score of item q_items[q] among user row q_rows[q]'s candidates, -inf if absent. */
FR_API int fr_eval_topk_segments(const int64_t* seg_start, int64_t n_users, const int64_t* items, const float* scores,
                                 int32_t k, int64_t* topk_idx, int32_t* flags, void* stream);
FR_API int fr_eval_lookup_segments(const int64_t* seg_start, int64_t n_users, const int64_t* items, const float* scores,
                                   const int64_t* q_rows, const int64_t* q_items, int64_t n_q, float* out, void* stream);
/* fr_topk_like_torch_cpu (HOST, no stream): torch.topk(rows, k, dim=-1) of the CPU backend with ITS order among equal values --
 * what the reference's evaluation ranks with (collector.py:149 on the dense -inf matrix of trainer.py:441-456).  rows: float
 * [n_rows, n] in host memory; idx_out int64 [n_rows, k] (val_out float [n_rows, k], optional).  For the user rows whose list
 * hangs on an exact score tie; every other row is ranked on the device (csrc/topk_host.hip says why the order can be had). */
FR_API int fr_topk_like_torch_cpu(const float* rows, int64_t n_rows, int64_t n, int32_t k, int64_t* idx_out, float* val_out);
/* ---- evaluation by value (`eval_args.mode: labeled`): recbole/evaluator/metrics.py MAE / RMSE / LogLoss / AUC, and GAUC -----------
 * fr_value_metrics: one streaming pass over score / label (float [n], what `predict` returned and LABEL_FIELD, all batches back
 *   to back) -> out[0..2] (double) = sum |score - label|, sum (score - label)^2, sum of -y log p - (1 - y) log(1 - p) with
 *   p = clip(score, 1e-15, 1 - 1e-15) in double; counts[0..1] (int64) = n, number of rows with label == 1.  Double sums in a fixed
 *   order (per-workgroup partials in ws, folded by a second launch): the same input gives the same bits on every call.
 * fr_auc_sorted: score_sorted = the score column sorted ascending, label_sorted = the labels in that order (NaN scores: undefined
 *   result, no fault) -> out[0..2] (int64) = 2U, P, Nn: P rows with label == 1, Nn = n - P, and 2U = sum over the positives of
 *   C[s_i] + C[e_i], [s_i, e_i) = the run of rows with the positive's score, C[j] = negatives among rows [0, j).  AUC with tied
 *   scores sharing one threshold (sklearn.metrics.roc_auc_score) = 2U / (2 P Nn), exact integers here; the caller divides.
 * Both: 1 <= n < 2^31; ws of at least the *_workspace_bytes(n) (0 for an n out of range).  FR_EINVAL (null pointer, n out of
 *   range, workspace too small) is returned before anything is launched or written.
 * fr_eval_meanrank_segments: `rec.meanrank` of an evaluation batch, a wave per user (the arguments of fr_eval_topk_segments and
 *   fr_eval_hits).  User row u's cells are the DISTINCT items among rows [seg_start[u], seg_start[u+1]) (a repeated item counts
 *   once and carries one score); items == NULL: row j of the segment is the cell of item j (a dense `full` row: seg_start[u] =
 *   u * n_items).  Its positives are the items of the keys u * n_items + item in pos_keys (SORTED, int64 [n_pos]; a key listed
 *   twice is one positive; a positive that is no cell of the user is none; a positive scores above -inf).  out int64
 *   [n_users, 3] = { 2 * pos_rank_sum, user_len, pos_len }: user_len = cells scoring above -inf, pos_len = distinct positives,
 *   pos_rank_sum = sum over the positives of #{cells greater} + (#{cells equal} + 1) / 2 (1-based descending rank, ties share the
 *   mean rank).  n_rows = seg_start[n_users]; ws: fr_eval_meanrank_workspace_bytes(n_rows) bytes when items != NULL (may be NULL
 *   otherwise).  FR_EINVAL before any launch as above. */
FR_API size_t fr_value_metrics_workspace_bytes(int64_t n);
FR_API int fr_value_metrics(const float* score, const float* label, int64_t n, double* out, int64_t* counts, void* ws,
                            size_t ws_bytes, void* stream);
FR_API size_t fr_auc_sorted_workspace_bytes(int64_t n);
FR_API int fr_auc_sorted(const float* score_sorted, const float* label_sorted, int64_t n, int64_t* out, void* ws, size_t ws_bytes,
                         void* stream);
FR_API size_t fr_eval_meanrank_workspace_bytes(int64_t n_rows);
FR_API int fr_eval_meanrank_segments(const int64_t* seg_start, int64_t n_users, const int64_t* items, const float* scores,
                                     const int64_t* pos_keys, int64_t n_pos, int64_t n_items, int64_t n_rows, int64_t* out,
                                     void* ws, size_t ws_bytes, void* stream);
FR_API size_t fr_topk_metrics_workspace_bytes(int64_t n_users, int32_t k);
FR_API int fr_topk_metrics(const int32_t* rec_topk, int64_t n_users, int32_t k, double* out, void* ws, size_t ws_bytes,
                           void* stream);
FR_API size_t fr_topk_metrics_grouped_workspace_bytes(int64_t n_users, int32_t k, int64_t n_groups);
FR_API int fr_topk_metrics_grouped(const int32_t* rec_topk, const int64_t* perm, const int64_t* group_start, int64_t n_users,
                                   int32_t k, int64_t n_groups, double* out, void* ws, size_t ws_bytes, void* stream);
FR_API size_t fr_gauc_grouped_workspace_bytes(int64_t n_users, int64_t n_groups);
FR_API int fr_gauc_grouped(const int64_t* meanrank, const int64_t* perm, const int64_t* group_start, int64_t n_users,
                           int64_t n_groups, double* out, int64_t* kept, void* ws, size_t ws_bytes, void* stream);
/* fr_exposure_grouped: the sums of the six exposure metrics (GiniIndex, ItemCoverage, ShannonEntropy, PopularityPercentage,
 * TailPercentage, AveragePopularity @ k, metrics.py:438-821) per GROUP of users, for n_k cut-offs, in one chain; memory is
 * O(entries), no [groups, items] table.
 *   keys_sorted int64 [n_entries], n_entries = n_users * k_cols: the entry at rank r (0-based) of a user of group g with item i is
 *   the key (g * n_items + i) * k_cols + r; the keys ascend.  Equal keys may occur; the sort need not be stable.  A CELL is the run
 *   of entries with equal key / k_cols, one (group, item) pair; its count at cut-off ks[j] is c_j = the entries with r < ks[j],
 *   found by a search for the key cell * k_cols + min(ks[j], k_cols), never by a walk of the cell.
 *   group_start int64 [n_groups + 1] on the device: the users per group, cumulative; n_g = group_start[g+1] - group_start[g],
 *   T_gj = n_g * ks[j] (ks[j] as given, also beyond k_cols).  ks: a HOST array, read by the entry, strictly ascending, >= 1,
 *   1 <= n_k <= 8.  popular, tail uint8 [n_items] (any non-zero value is a flag), count_items int64 [n_items]: each may be NULL,
 *   and its sum is then 0.
 *   out_i int64 [n_groups][n_k][5] = { m, S, pop, tl, cnt }: m = the cells with c_j > 0 (distinct recommended items); S = the Gini
 *   numerator, the sum over the n_items items of the catalogue sorted ascending by their count c_j in the group (the items without
 *   an entry first, ties in any order) of (2 idx - n_items - 1) * c_j, idx 1-based, an exact integer; pop, tl, cnt = the sums over
 *   the group's entries with r < ks[j] of popular[i] != 0, tail[i] != 0, count_items[i].  A count above n_g (a padded list repeats
 *   item 0) is counted as it is, never clamped.
 *   out_entropy double [n_groups][n_k] = sum over the cells of -p log(p), p = c_j / T_gj.  SUMMATION ORDER (a contract): with
 *   h[c] = the cells of count c, term(c) = (double)h[c] * (-(q * log(q))), q = (double)c / ((double)n_g * (double)ks[j]), and +0.0
 *   where h[c] = 0; the counts 1 .. n_g are cut into chunks of 256 consecutive counts, lane = count within the chunk; a chunk is
 *   reduced per wave of 64 lanes by the xor butterfly (offsets 32, 16, .., 1) and its four wave sums are added in ascending wave
 *   order; the chunk sums are added in ascending chunk order from 0.0; then the cells with c > n_g, sorted ascending by c, are
 *   added one by one, each as 1.0 * (-(q * log(q))).
 *   An empty group: five zeros and NaN.  Integer sums by integer atomics, the entropy without atomics: the same input gives the
 *   same bits on every call.  Malformed keys (unsorted, group part >= n_groups) and a malformed group_start are clamped: unspecified
 *   values, no access outside the arrays.
 *   FR_EINVAL before anything is launched or written: a null pointer other than popular / tail / count_items, a size below 1,
 *   n_entries no multiple of k_cols or >= 2^32, n_k outside 1..8, ks not strictly ascending or below 1, n_groups * n_items * k_cols
 *   >= 2^63 (the key), n_items * n_users * k_cols >= 2^62 (the bound on |S|), ws below fr_exposure_grouped_workspace_bytes(n_users,
 *   k_cols, n_groups, n_k), which is 0 for arguments out of range. */
FR_API size_t fr_exposure_grouped_workspace_bytes(int64_t n_users, int32_t k_cols, int64_t n_groups, int32_t n_k);
FR_API int fr_exposure_grouped(const int64_t* keys_sorted, int64_t n_entries, int64_t n_items, int32_t k_cols,
                               const int64_t* group_start, int64_t n_groups, const int32_t* ks, int32_t n_k,
                               const uint8_t* popular, const uint8_t* tail, const int64_t* count_items, int64_t* out_i,
                               double* out_entropy, void* ws, size_t ws_bytes, void* stream);
FR_API int fr_group_sums(const int64_t* perm, const int64_t* seg_start, int64_t n_segments, const int32_t* group,
                         const float* value, const float* wtrue, int32_t n_groups, double* stats, void* stream);
FR_API size_t fr_fair_metrics_workspace_bytes(int64_t n_segments);
FR_API int fr_fair_metrics_from_stats(const double* stats, int64_t n_segments, int32_t n_groups, double* out, void* ws,
                                      size_t ws_bytes, void* stream);
FR_API size_t fr_df_cells_workspace_bytes(int64_t n_items);
FR_API int fr_df_cells(const int64_t* perm, const int64_t* item_start, int64_t n_items, const int32_t* group,
                       const float* value, int32_t n_groups, double* out, void* ws, size_t ws_bytes, void* stream);

/* ---- bootstrap over rows: the sampling error of the per-group metrics and of their gaps ----------------------------------------
 * THE RESAMPLING WEIGHTS (a contract: a CPU reference reproduces them bit for bit).  A Poisson bootstrap: in replicate b row r
 * counts w(r, b) times, w ~ Poisson(1), independent over rows and replicates.  With
 *   (x, y, z, t) = philox4x32_10(counter = (r, 0, b >> 2, 0), key = (seed & 0xffffffff, seed >> 32))   (Salmon et al., SC'11)
 * and word = component b & 3 of it, w(r, b) = the number of j in 0..11 with word >= T[j], T[j] = floor(2^32 e^-1 sum_{i<=j} 1/i!):
 *   0x5e2d58d8, 0xbc5ab1b1, 0xeb715e1d, 0xfb239797, 0xff1025f5, 0xffd90f3b, 0xfffa8b71, 0xffff540c, 0xffffed1f, 0xfffffe21,
 *   0xffffffd4, 0xfffffffc;  so w lies in 0..12.  r is the row's index in `values`, not its position within its group: a row
 * carries the same weight under every grouping, and the sums of groups that refine a grouping add up to its sums.
 *
 * fr_bootstrap_group_sums: values double [n_rows][ld] (the first n_cols columns of every row are read); groups as segments, the
 *   arguments of fr_topk_metrics_grouped: the members of group g are the rows perm[group_start[g] .. group_start[g+1]) (perm int64
 *   [n_rows], NULL = identity; group_start int64 [n_groups + 1] on the device).
 *     out_sums   double [n_groups][n_rep][n_cols] = sum over the group's rows r of (double)w(r, b) * values[r][c]
 *     out_weight int64  [n_groups][n_rep]         = sum over the group's rows of w(r, b)
 *   Every row's product enters the sum, w = 0 included: a NaN (or infinite) value makes its (group, column) NaN in every replicate,
 *   as it makes the point estimate NaN.  An empty group: zeros.  No weight is ever stored: a workgroup takes one chunk of one
 *   group's positions, 1024 replicates and 8 columns; a lane owns four replicates, one Philox call per (row, lane) gives its four
 *   weights, and the lane adds w * value into its own accumulators row after row (fused multiply-add, ascending position; no
 *   cross-lane reduction).  The per-chunk partials are added per group in ascending chunk order from 0.0.  No floating-point
 *   atomics: the same input gives the same bytes on every call.  Any summand passes through at most n_g roundings.
 *   CHUNKS AND WORKSPACE: chunk length L = 64 * ceil(n_rows / (64 * 2048)) positions, so there are at most
 *   blocks = ceil(n_rows / L) + n_groups <= 2048 + n_groups chunks, and
 *     fr_bootstrap_group_sums_workspace_bytes = (blocks * n_rep * (n_cols + 1) + n_groups + 1) * 8
 *   (partial sums double [blocks][n_rep][n_cols], partial weights int64 [blocks][n_rep], chunk_start int64 [n_groups + 1]): bounded
 *   by the number of chunks times n_rep * n_cols, never by n_rows * n_rep.
 *   Limits: 1 <= n_rows < 2^31, 1 <= n_cols <= 64 (FR_BOOTSTRAP_MAX_COLS), n_cols <= ld, 1 <= n_rep <= 65536 (FR_BOOTSTRAP_MAX_REP),
 *   n_groups >= 1 (and n_groups * n_rep * n_cols within one launch of 2^31 - 1 blocks of 256).  perm and group_start are clamped as
 *   in the other grouped entries: a malformed table gives unspecified values and no access outside the arrays.
 *   FR_EINVAL before anything is launched or written: a null pointer other than perm, a size out of range, ld < n_cols, ws below the
 *   _workspace_bytes value, which is 0 for arguments out of range.
 * fr_topk_user_terms: out double [n_users][n_cols], out[u][j] = row u's term of top-k metric metric[j] (0..5 = hit, mrr, ndcg,
 *   recall, precision, map) at cut-off cut[j] (1 <= cut[j] <= k): the per-row terms fr_topk_metrics averages, from the same device
 *   function, the same bits (a mean over one row is that row's term).  metric, cut: HOST arrays, 1 <= n_cols <= 64
 *   (FR_USER_TERMS_MAX_COLS).  rec_topk int32 [n_users][k + 1] as fr_topk_metrics.  A zero-positive row: Recall NaN, NDCG and MAP 0.
 * fr_gauc_user_terms: out double [n_users][2] = (auc_u * pos_len, pos_len) of a kept user, (0, 0) of a dropped one, from the
 *   `rec.meanrank` triples of fr_gauc_grouped and the device function it uses.
 *   Both: 1 <= n_users < 2^31; FR_EINVAL (null pointer, size or column out of range) before anything is launched or written.
 *
 * fr_bootstrap_fair_metrics: the fairness metrics (fr_group_sums + fr_fair_metrics_from_stats, and NonParity's group means) in
 *   every replicate of the same bootstrap, resampling USERS: replicate b is the metric of the multiset in which member j occurs
 *   w(unit[j], b) times, w as above with r = unit[j].  The unit is the user's row in the evaluation, so a user weighs the same
 *   here, in fr_bootstrap_group_sums over the users, and under every attribute.  unit int64 per member, in [0, 2^31) (the Philox
 *   counter takes its low 32 bits).
 *   Members and items as in fr_group_sums: positions j in [item_start[k], item_start[k+1]) are the members of item k, member
 *   perm[j] (perm int64 [n_members], NULL = identity; item_start int64 [n_items + 1] on the device); group int32, value float,
 *   wtrue float (NULL: every wtrue is 0) and unit are indexed by member.  A member whose group index is outside [0, n_groups)
 *   is counted in no cell and no total.  perm is clamped into [0, n_members), item_start into [0, n_members]: a malformed table
 *   gives unspecified values and no access outside the arrays.
 *   Per replicate b, item k and group g the cell is S = sum w * value, C = sum w, T = sum w * wtrue.  Item k is PRESENT in b when
 *   its sum over g of C is > 0; K_b = the number of present items.  `want` selects what is computed beyond K_b and the totals:
 *     FR_FAIR_WANT_VALUE (n_groups must be 2): out_terms[0..3][b] = the sums over the present items of the Value, Absolute, Under
 *       and Over terms of fr_fair_metrics_from_stats (n = C + 1e-5, p = S / n, r = T / n);
 *     FR_FAIR_WANT_DF: out_terms[4][b] = the sum over the present items of the DifferentialFairness epsilon of that entry with
 *       the table entries (float)((S + 1.0 / K_b) / (C + 1.0)): alpha = 1 / K_b, the replicate's own number of items, not
 *       1 / n_items; float32 logf, a NaN pair left out.
 *   A term not selected is written as 0.
 *     out_terms        double [5][n_rep]         sums, NOT divided: the caller divides by K_b (K_b = 0: 0 / 0 = NaN)
 *     out_items        int64  [n_rep]            K_b
 *     out_group_sum    double [n_groups][n_rep]  sum over ALL members of group g of w * value   (NonParity: the group mean is
 *     out_group_weight int64  [n_groups][n_rep]  sum over them of w, exact                       their quotient)
 *   SUMMATION ORDER (a contract): the items are cut into `chunks` runs of consecutive whole items, item k in chunk
 *   floor(item_start[k] / L), L = ceil(n_members / chunks), chunks = min(1024, n_items, max(1, 2^20 / n_rep),
 *   ceil(n_members / 64)).  One wave takes one chunk and 256 replicates; a lane owns four replicates, one Philox call per (member,
 *   lane) gives its four weights, nothing is stored per member or per item.  The lane walks the chunk's members in ascending
 *   position, adds w * value (exact in double) into the member's cell and group total, closes an item after its last member
 *   and adds the item's terms to its running sums in ascending item order.  K_b comes from a first walk, which also gives the
 *   value-type sums and the totals; the DifferentialFairness sums come from a second walk that starts from 1 / K_b.  The
 *   per-chunk partials are added in ascending chunk order from 0.  An item is never split: the longest item bounds the chain.
 *   No floating-point atomics: the same input gives the same bytes on every call.
 *   Workspace: fr_bootstrap_fair_metrics_workspace_bytes = chunks * n_rep * (2 * n_groups + 6) * 8: bounded by the chunks, never
 *   by members * n_rep or items * n_rep.
 *   Limits: 1 <= n_members <= 2^28, 1 <= n_items < 2^31, 1 <= n_groups <= 8, 1 <= n_rep <= 65536 (FR_BOOTSTRAP_MAX_REP), want a
 *   combination of the two bits (0: K_b and the totals only).  FR_EINVAL before anything is launched or written: a null pointer
 *   other than perm / wtrue, a size out of range, FR_FAIR_WANT_VALUE with n_groups != 2, ws below the _workspace_bytes value,
 *   which is 0 for arguments out of range. */
#define FR_FAIR_WANT_VALUE 1
#define FR_FAIR_WANT_DF 2
#define FR_BOOTSTRAP_MAX_COLS 64
#define FR_BOOTSTRAP_MAX_REP 65536
#define FR_USER_TERMS_MAX_COLS 64
FR_API size_t fr_bootstrap_group_sums_workspace_bytes(int64_t n_rows, int32_t n_cols, int64_t n_groups, int32_t n_rep);
FR_API int fr_bootstrap_group_sums(const double* values, int64_t n_rows, int32_t n_cols, int64_t ld, const int64_t* perm,
                                   const int64_t* group_start, int64_t n_groups, int32_t n_rep, uint64_t seed, double* out_sums,
                                   int64_t* out_weight, void* ws, size_t ws_bytes, void* stream);
FR_API int fr_topk_user_terms(const int32_t* rec_topk, int64_t n_users, int32_t k, const int32_t* metric, const int32_t* cut,
                              int32_t n_cols, double* out, void* stream);
FR_API int fr_gauc_user_terms(const int64_t* meanrank, int64_t n_users, double* out, void* stream);
FR_API size_t fr_bootstrap_fair_metrics_workspace_bytes(int64_t n_members, int64_t n_items, int32_t n_groups, int32_t n_rep);
FR_API int fr_bootstrap_fair_metrics(const int64_t* perm, const int64_t* item_start, int64_t n_items, int64_t n_members,
                                     const int32_t* group, const float* value, const float* wtrue, const int64_t* unit,
                                     int32_t n_groups, int32_t n_rep, uint64_t seed, int32_t want, double* out_terms,
                                     int64_t* out_items, double* out_group_sum, int64_t* out_group_weight, void* ws,
                                     size_t ws_bytes, void* stream);

/* ---- built-in profiler -------------------------------------------------------------------------------
 * When enabled every kernel launch of this library is bracketed by a hipEvent pair recorded on the
 * launch stream; fr_prof_read synchronises the outstanding events and returns the accumulated device
 * time and launch count of one kernel kind (bench.py's `roofline.achieved` comes from here).
 * Process-global diagnostic state (one table of kernel kinds per process = per GPU), guarded by a mutex: any thread may
 * launch while it is on, the counts of all threads are summed; enable / reset / read from one thread at a time.  Apart
 * from this table, the library's helper stream and the last-error string (thread-local), the entry points keep no state
 * between calls: everything lives in the caller's tables and workspaces. */
FR_API int fr_prof_enable(int on);
FR_API int fr_prof_reset(void);
FR_API int fr_prof_kernel_count(void);
FR_API const char* fr_prof_kernel_name(int kind);
FR_API int fr_prof_read(int kind, double* total_ms, int64_t* count);
/* Algorithmic work the launches of `kind` stood for since the last reset: FLOP (2 M N K per product) for linear_fwd /
 * linear_bwd_input / linear_bwd_weight / mlp_infer, bytes (12 nnz + 8 n_rows dim) for spmm_csr, 0 for the kinds that do not account.
 * work / total_ms is the rate bench.py holds against the MFMA / HBM peak. */
FR_API int fr_prof_read_work(int kind, double* work);

/*
 * Dynamic negative sampling (`neg_sampling: {uniform: 1, dynamic: M}`): keep the highest-scoring of M candidates per slot.
 * scores / cand are [M, cols] row-major; out[c] = cand[r*cols + c] with r = the first index of the maximum of
 * scores[:, c] -- torch.max(dim=0) semantics: the lowest index among equal maxima, a NaN beats every number and the
 * first NaN wins.
 */
FR_API int fr_dyn_neg_select(const float* scores, const int64_t* cand, int64_t cols, int32_t M, int64_t* out, void* stream);

/* The same for a dot-product model (PFCN_PMF / PFCN_BiasedMF predict), scores computed in the kernel: candidate r of output
 * column c = j*n + i (j < num) is cand[(r*num + j)*n + i], its score
 *     sigmoid(((dot(user_rows[i,:], item row) + user_bias[i]) + item bias) + *global_bias)
 * with the item (and item bias) rows read as of the tables' step, as fr_table_gather reads them; each bias term is
 * skipped when its pointer is NULL.  An id outside the item table sets FR_DEV_ERR_INDEX_RANGE in *err_flag. */
FR_API int fr_dyn_neg_dot_select(const fr_table* item_t, const fr_adam* item_adam, const fr_table* item_bias_t,
                                 const fr_adam* item_bias_adam, const float* user_rows, const float* user_bias,
                                 const float* global_bias, const int64_t* cand, int64_t n, int32_t num, int32_t M,
                                 int64_t* out, uint32_t* err_flag, void* stream);
/* The [num*M*n] scores fr_dyn_neg_dot_select picks from, in cand's order (for checking them). */
FR_API int fr_dyn_neg_dot_scores(const fr_table* item_t, const fr_adam* item_adam, const fr_table* item_bias_t,
                                 const fr_adam* item_bias_adam, const float* user_rows, const float* user_bias,
                                 const float* global_bias, const int64_t* cand, int64_t n, int32_t num, int32_t M,
                                 float* scores, uint32_t* err_flag, void* stream);

/*
 * Recommendation: the k best cells of every row, ranked by ONE total order -- higher score first, NaN above +inf, and among
 * equal scores (-0 == +0, all NaNs equal) the lower column / item id first -- so a result does not depend on how the work
 * is split.  Masked cells have score -inf and take part like any other cell: a row with fewer than k unmasked cells is
 * completed by -inf entries in ascending id.  k must be in 1..min(FR_TOPK_MAX, n_cols); anything else, a null pointer or a
 * short workspace is FR_EINVAL before anything is launched or written.
 *
 * `slices`: into how many ranges the columns / items are cut (one workgroup each, merged by a second kernel); 0 = chosen
 * from the shape so that the chip is filled (or FAIRREC_REC_SLICES when that is set).  At most 64, and slices * k <= 8192.
 * The workspace holds the slices' lists: rows * slices * k * 8 bytes; it does not grow with rows * n_cols.
 *
 * fr_topk_rows: from a dense fp32 [n_rows, n_cols] matrix with leading dimension ld >= n_cols; val_out [n_rows, k] are the
 *   selected cells' own bits, idx_out [n_rows, k] their columns.
 */
#define FR_TOPK_MAX 256
FR_API size_t fr_topk_rows_workspace_bytes(int64_t n_rows, int64_t n_cols, int32_t k, int32_t slices);
FR_API int fr_topk_rows(const float* scores, int64_t n_rows, int64_t n_cols, int64_t ld, int32_t k, int32_t slices,
                        float* val_out, int64_t* idx_out, void* ws, size_t ws_bytes, void* stream);

/*
 * fr_recommend_topk: the same selection over scores computed in the kernel and never stored,
 *     score(u, i) = epilogue(((dot(X[u,:], W[i,:]) + user_bias[u]) + item_bias[i]) + bias0)
 * dot = one ascending-column fp32 fmaf chain from 0 (v_mfma_f32_32x32x2_f32); a bias term is skipped when its pointer is
 * NULL.  epilogue 0: none; 1: clamp(x, 0, scale) / scale (IEEE division; a NaN stays a NaN); 2: 1 / (1 + expf(-x)), the form
 * of fr_dyn_neg_dot_select.  A zero score is +0.  mask_pad: item 0 scores -inf.  hist_indptr [n_users + 1] / hist_items
 * [hist_len] (either both or hist_indptr NULL): items of user u, hist_items[hist_indptr[u] .. hist_indptr[u+1]), score -inf;
 * they must ascend within a user, which the caller states with hist_sorted = 1 (anything else is FR_EINVAL).
 * W is read as it lies in memory, row stride dim; 1 <= dim <= 256, no alignment asked of it.
 * scores_out (optional): also receives the dense masked [n_users, n_items] matrix of exactly the scores that were ranked.
 * val_out of a NaN score is the canonical quiet NaN.
 */
typedef struct fr_rec_args {
    const float* X;             /* [n_users, dim] the users' final embeddings */
    const float* W;             /* [n_items, dim] the item table */
    const float* user_bias;     /* [n_users] or NULL */
    const float* item_bias;     /* [n_items] or NULL */
    const int64_t* hist_indptr; /* [n_users + 1] or NULL */
    const int64_t* hist_items;  /* [hist_len] */
    float* scores_out;          /* [n_users, n_items] or NULL */
    int64_t n_users;
    int64_t n_items;
    int64_t hist_len;
    int32_t dim;
    int32_t k;
    int32_t epilogue;
    int32_t mask_pad;
    int32_t hist_sorted;
    int32_t slices;
    float bias0;
    float scale;                /* epilogue 1 */
} fr_rec_args;
FR_API size_t fr_recommend_topk_workspace_bytes(const fr_rec_args* a);
FR_API int fr_recommend_topk(const fr_rec_args* a, float* val_out, int64_t* idx_out, void* ws, size_t ws_bytes, void* stream);

/*
 * Full-sort evaluation without the matrix (`full_sort_eval: fused`).  Both entries read an fr_rec_args as fr_recommend_topk
 * does and ignore its k, slices and scores_out; they speak of the matrix scores_out WOULD hold for the same arguments.
 *
 * fr_recommend_cells: score_out[c] = the bits of scores_out[cell_user[c], cell_item[c]], c < n_cells -- -inf for the pad item
 *   (mask_pad) and for a cell of the user's history.  The dot is the one ascending-column fp32 fmaf chain from 0 of
 *   fr_recommend_topk, run on the same instruction (v_mfma_f32_32x32x2_f32 over the cells' 32 user rows and 32 item rows, of
 *   which the diagonal is kept), then the bias adds, the epilogue and the mask in that entry's order.  A cell_user outside
 *   [0, n_users) or a cell_item outside [0, n_items) sets FR_DEV_ERR_INDEX_RANGE in *err_flag; its score_out is a quiet NaN.
 *
 * fr_recommend_meanrank: out int64 [n_users, 3] = what fr_eval_meanrank_segments(items = NULL, seg_start[u] = u * n_items)
 *   returns on that matrix for the same pos_keys (SORTED keys user * n_items + item, int64 [n_pos]): { 2 * pos_rank_sum,
 *   user_len, pos_len }.  As there, a key listed twice is one positive, a key outside the matrix is none, a positive that is a
 *   masked cell scores -inf (every live cell ranks above it), and a user without positives gets { 0, user_len, 0 }.  A NaN cell
 *   is no live cell; a NaN positive counts in pos_len and adds 1 to the first column, as it does there.
 *   The tiling, staging and MFMA chain are fr_recommend_topk's, so a counted cell has the ranked cell's bits; the positives'
 *   own scores (fr_recommend_cells' kernel) are the thresholds the live cells are counted against.  Integer atomics only: the
 *   same output on every call.  Nothing of size n_users * n_items is stored: ws holds 4 bytes per key,
 *   fr_recommend_meanrank_workspace_bytes(a, n_pos) (0 for arguments that are refused).  The items are cut into slices by the
 *   shape (or FAIRREC_REC_SLICES); a tile of 32 users whose longest list has more than 128 positives goes over its slice once
 *   per 128 of them.  err_flag is not written (no key is an error).
 *
 * FR_EINVAL before anything is launched or written: a null pointer (the struct, X, W, an output, err_flag, the lists of a
 * positive count, a short or misaligned workspace), dim outside 1..256, n_users outside 0..2^31-1, n_items outside 1..2^31-1,
 * an unknown epilogue, epilogue 1 without a positive scale, a history with hist_sorted != 1, a negative count, cells with
 * n_users == 0.  n_cells == 0 and n_pos == 0 are FR_OK; with n_pos == 0, out still gets user_len.
 */
FR_API int fr_recommend_cells(const fr_rec_args* a, const int64_t* cell_user, const int64_t* cell_item, int64_t n_cells,
                              float* score_out, uint32_t* err_flag, void* stream);
FR_API size_t fr_recommend_meanrank_workspace_bytes(const fr_rec_args* a, int64_t n_pos);
FR_API int fr_recommend_meanrank(const fr_rec_args* a, const int64_t* pos_keys, int64_t n_pos, int64_t* out, void* ws,
                                 size_t ws_bytes, uint32_t* err_flag, void* stream);

/*
 * fr_rows_l2_normalize: Y[r, :] = X[r, :] / max(|X[r, :]|_2, eps) for the M rows of an fp32 matrix -- the unit vectors whose
 * dot product is the cosine similarity of the rows (eps as in nn.CosineSimilarity).  With both factors of fr_recommend_topk
 * normalised once, epilogue 2 ranks sigmoid(cos(x_u, w_i)): PFCN_DMF's `full_sort_scorer: towers`.
 *
 * X [M, D] with row stride ldx, Y [M, D] with row stride ldy (floats; ldx, ldy >= D; the columns D.. of a row of Y are not
 * written), norm_out optional [M].  1 <= D <= 256 (the fused ranking entries' own limit), M >= 0; M == 0 is FR_OK with
 * nothing launched.  Y == X (with ldy == ldx) is allowed: a wave reads the whole of a row before it writes it; any other
 * overlap of X and Y is not.  No workspace, no atomics, no LDS: one wave per row, column c in lane c % 64, slot e = c / 64.
 *
 * A row, in fp32 with every operation rounded to nearest:
 *   1. each lane l:  s_l = 0;  for e = 0, 1, ... while l + 64 e < D:  s_l = fmaf(x[l + 64 e], x[l + 64 e], s_l)
 *   2. s = the sum of the 64 s_l in the fixed butterfly order of the library's wave sum: six rounds
 *      s_l += s_(l xor o), o = 32, 16, 8, 4, 2, 1, after which every lane holds s
 *   3. n = sqrt(s), d = fmaxf(n, eps), y[c] = x[c] / d          (square root and quotient correctly rounded: __fsqrt_rn and
 *      __fdiv_rn in their IEEE meaning)
 *   4. norm_out[r] = n, the unclamped norm
 *   5. a NaN or an infinity comes out as IEEE arithmetic gives it: an infinite norm (an infinite entry, or a sum of squares
 *      that overflows) turns finite entries into 0 and infinite ones into NaN; a NaN entry makes n NaN, fmaxf then returns
 *      eps, so the row's NaN stays NaN and its other entries come out as x / eps.  An all-zero row stays all zero (eps > 0).
 * The bits of a row of Y and its norm depend on that row, D and eps alone -- not on M, the row's position, the wave that
 * takes it, its neighbours' contents or the strides.  Against exact arithmetic: E + 6 roundings in s (E = ceil(D / 64)), halved
 * by the root, one each for root and quotient: |y - y_exact| <= ((E + 6) / 2 + 2) 2^-24 |y_exact| to first order.
 *
 * FR_EINVAL before anything is launched or written, fr_last_error naming the entry: M < 0, D outside 1..256, ldx < D or
 * ldy < D, a negative or NaN eps, a null X or Y with M > 0.
 */
FR_API int fr_rows_l2_normalize(const float* X, int64_t M, int32_t D, int64_t ldx, float eps, float* Y, int64_t ldy,
                                float* norm_out, void* stream);

/*
 * fr_mlp_infer: a whole MLP in one launch, for inference.  Each layer is Linear, then (optionally) BatchNorm1d on its RUNNING
 * statistics, then the activation (the codes of fr_linear_fwd: 0 none, 1 relu, 2 leakyrelu 0.01, 3 sigmoid, 4 tanh);
 *     Y[M, n_out_last] = (net_0(X) + net_1(X) + ...  in list order, fp32 adds from the first) / out_div      (IEEE division,
 * also when out_div is 1).  Nothing is kept for a backward pass; there is no workspace and no atomic; no argument but Y is
 * written -- the running statistics are read and never advanced, and there is no num_batches_tracked.
 *
 * Shapes: every width (k_in and each n_out) in 1..FR_MLP_INFER_MAX_WIDTH with no multiple asked of it, pointers float-aligned,
 * 1..FR_MLP_INFER_MAX_LAYERS layers, 1..FR_MLP_INFER_MAX_NETS nets that share k_in and the last n_out.  M >= 0; M == 0 is
 * success with nothing launched.  Anything else, a null pointer, an act outside 0..4, a partly-null BatchNorm quadruple or
 * out_div == 0 is FR_EINVAL before anything is launched or written, and fr_last_error names the argument.
 *
 * Row independence: the bits of output row r depend on row r of X and on the parameters only -- not on M, on r's position, on
 * the tile r falls in or on any other row's content (a NaN or Inf elsewhere does not reach it).  Row r of one layer, for
 * output column j, in fp32 with every operation rounded to nearest:
 *     acc = 0;  for k = 0, 2, 4, ... < n_in:  acc = (acc + x[k] W[j,k]) + x[k+1] W[j,k+1]     one v_mfma_f32_32x32x2_f32 per k
 *               pair, ascending, the two products of a pair accumulated as the instruction does (x[n_in] = W[j,n_in] = 0
 *               closes an odd n_in)
 *     z   = acc + bias[j]
 *     y   = fmaf(z - bn_mean[j], sc, bn_bias[j]),   sc = bn_weight[j] * (1 / sqrtf(bn_var[j] + bn_eps))     (BatchNorm layers;
 *               sqrtf and the division correctly rounded)
 *     out = act(y):  relu  y < 0 ? 0 : y;  leakyrelu  y < 0 ? 0.01f * y : y  (both keep a NaN);  sigmoid  1 / (1 + expf(-y));
 *               tanh  tanhf(y)
 * The order is the same for every shape: the kernel always cuts rows into tiles of 32, input columns into chunks of 32 and
 * output columns into groups of 128, and a cell's chain does not see the cuts.
 */
#define FR_MLP_INFER_MAX_LAYERS 8
#define FR_MLP_INFER_MAX_WIDTH  512
#define FR_MLP_INFER_MAX_NETS   8
typedef struct fr_mlp_layer {
    const float *W, *bias;                 /* nn.Linear layout [n_out, n_in], [n_out] */
    const float *bn_weight, *bn_bias, *bn_mean, *bn_var;   /* all four, or all NULL = no BatchNorm in this layer */
    float bn_eps;
    int32_t n_out;
    int32_t act;                           /* the codes of fr_linear_fwd, 0..4 */
} fr_mlp_layer;
typedef struct fr_mlp_net {
    int32_t n_layers, k_in;
    fr_mlp_layer layer[FR_MLP_INFER_MAX_LAYERS];
} fr_mlp_net;
FR_API int fr_mlp_infer(const fr_mlp_net* nets, int32_t n_nets, float out_div, const float* X, int64_t M, float* Y, void* stream);

/*
 * fr_pair_mlp_scores: every (user, item) score of an MLP scorer over cat(user, item) whose first Linear the caller has split,
 *     z1(u, i) = (W1[:, :D] x_u + b1) + W1[:, D:] w_i = P[u] + Q[i]
 * (P [n_users, n1] carries b1, Q [n_items, n1] carries no bias: two fr_linear_fwd products).  With the remaining n_linears - 1
 * layers (W[l] [n_out[l], n_out[l-1]], bias[l]) in nn.Linear layout, the last with ONE output,
 *     score(u, i) = sigmoid(act(w_L . act(... act(W[0] act(P[u] + Q[i]) + bias[0]) ...) + bias_L))
 * the activation after every layer, the last included (MLPLayers.forward in eval mode), the sigmoid as 1 / (1 + expf(-x)) with
 * the IEEE quotient (epilogue 2 of fr_recommend_topk).  act: the codes of fr_linear_fwd; only relu (1) is served.
 * scores_out [n_users, ld], ld >= n_items: columns n_items .. ld-1 are not touched.  mask_pad: item 0 scores -inf; hist_indptr
 * [n_users + 1] / hist_items [hist_len] as in fr_rec_args (either both or hist_indptr NULL), -inf at every listed cell, ascending
 * within a user, which the caller states with hist_sorted = 1.  No workspace, no atomic; nothing but scores_out is written.
 *
 * Shapes: n1 and every n_out[l] in 1..FR_PAIR_MLP_MAX_WIDTH with no multiple asked of them, 2..FR_PAIR_MLP_MAX_LINEARS linears in
 * the whole MLP (the split first layer counts), n_users, n_items >= 0 (zero: success, nothing launched).  Anything else, a null
 * pointer, an act other than relu or hist_sorted != 1 with a history is FR_EINVAL before any device work, and fr_last_error
 * names the argument.  fr_pair_mlp_supported: 1 when widths, layer count and activation are served (a host query).
 *
 * A cell's bits depend on P[u], Q[i] and the parameters alone -- not on n_users, n_items, ld, the tile or slice the cell falls
 * in, or any other cell's content (a NaN elsewhere does not reach it).  Cell (u, i), in fp32, every operation rounded to nearest:
 *     h[c] = relu(P[u, c] + Q[i, c])                                                  one add per column
 *     each further layer, output column j:  acc = 0;  for k = 0, 2, 4, ... < n_in:  acc = (acc + h[k] W[j,k]) + h[k+1] W[j,k+1]
 *               one v_mfma_f32_32x32x2_f32 per k pair: an ascending-column fmaf chain from 0 (h[n_in] = W[j,n_in] = 0 closes
 *               an odd n_in);  z = acc + bias[j], the bias added last;  h'[j] = relu(z)
 *     score = 1 / (1 + expf(-relu(z_L)))
 * relu(x) is x < 0 ? 0 : x: it KEEPS a NaN, as every relu of fr_linear_fwd does (x <= 0 ? 0 : x, or v > 0 ? v : v * 0 in its
 * fast forms; fmaxf would return the other operand), so a NaN in P[u] or Q[i] reaches every unmasked score of that user or
 * item, as it does through predict.
 */
#define FR_PAIR_MLP_MAX_LINEARS 6
#define FR_PAIR_MLP_MAX_WIDTH   256
typedef struct fr_pair_mlp_args {
    const float* P;                                   /* [n_users, n1], b1 added */
    const float* Q;                                   /* [n_items, n1] */
    const float* W[FR_PAIR_MLP_MAX_LINEARS - 1];      /* linears 2 .. n_linears */
    const float* bias[FR_PAIR_MLP_MAX_LINEARS - 1];
    const int64_t* hist_indptr;                       /* [n_users + 1] or NULL */
    const int64_t* hist_items;                        /* [hist_len] */
    float* scores_out;                                /* [n_users, ld] */
    int64_t n_users;
    int64_t n_items;
    int64_t ld;
    int64_t hist_len;
    int32_t n_out[FR_PAIR_MLP_MAX_LINEARS - 1];       /* the last used entry is 1 */
    int32_t n1;
    int32_t n_linears;                                /* of the whole MLP: 2..FR_PAIR_MLP_MAX_LINEARS */
    int32_t act;
    int32_t mask_pad;
    int32_t hist_sorted;
} fr_pair_mlp_args;
FR_API int fr_pair_mlp_supported(int32_t n1, int32_t n_linears, const int32_t* n_out, int32_t act);
FR_API int fr_pair_mlp_scores(const fr_pair_mlp_args* a, void* stream);

/*
 * fr_dyn_neg_mlp_select: the pick of dynamic negative sampling (fr_dyn_neg_select) for an MLP scorer over cat(user, item),
 * scores computed in the kernel with the first Linear split as fr_pair_mlp_scores splits it,
 *     z1 = (W1[:, :D] x_u + b1) + W1[:, D:] w_c = P[i] + q(c)
 * P [n, n1] (leading dimension ldp >= n1) is the caller's one product over the n batch rows and carries b1; q(c) is formed in
 * the kernel from the candidate's item row, which is never materialised.  W1_item points INTO the [n1, 2 D] first weight
 * (W1 + D) and ldw1 is that weight's row stride (2 D): nothing is copied.  W[l], bias[l], n_out[l], n_linears, act: the
 * remaining linears, as in fr_pair_mlp_args.  Candidate r of output column c = j*n + i (j < num) is cand[(r*num + j)*n + i],
 * its user row is row i of P: the layout of fr_dyn_neg_dot_select.  out [num*n].
 * fr_dyn_neg_mlp_scores: the [M*num*n] scores the pick is taken from, in cand's order (for checking them); the same kernel,
 * so the same bits.
 *
 * Shapes: fr_pair_mlp_supported(n1, n_linears, n_out, act) and 1 <= D = item_t->dim <= 256; n >= 0, num >= 1, M >= 1.  Anything
 * else, a null pointer (err_flag included) or an unknown learner is FR_EINVAL before any device work, and fr_last_error names
 * the argument.  n == 0 is success with nothing launched.
 *
 * Candidate (r, c), in fp32, every operation rounded to nearest:
 *     w       = the item row cand[...] as of the table's step: the replay fr_table_gather and fr_dyn_neg_dot_select do
 *     q[j]    = acc,  acc = 0;  for k = 0, 2, 4, ... < D:  acc = (acc + w[k] W1[j, D+k]) + w[k+1] W1[j, D+k+1]
 *               one v_mfma_f32_32x32x2_f32 per k pair: an ascending-column fmaf chain from 0 (w[D] = W1[j, 2 D] = 0 closes an
 *               odd D)
 *     h[j]    = relu(P[i, j] + q[j])                                                  one add per column
 *     every further layer, the one-output layer, relu (x < 0 ? 0 : x: it KEEPS a NaN) and score = 1 / (1 + expf(-relu(z_L))):
 *               exactly as fr_pair_mlp_scores states them
 * The pick of a column follows torch.max(dim=0): the lowest r among equal maxima, a NaN beats every number, the first NaN
 * wins.  A candidate's score bits depend on its row as of the step, its P row and the parameters alone -- not on n, num, M,
 * its position or any other candidate (a NaN elsewhere does not reach it).  An id outside the item table sets
 * FR_DEV_ERR_INDEX_RANGE in *err_flag; its loads stay on a clamped index (row 0) and the id itself is what a pick of it
 * returns.  No workspace, no atomic but the flag's; nothing but out / scores and the flag is written, the table never.
 */
typedef struct fr_dyn_neg_mlp_args {
    const fr_table* item_t;
    const fr_optim* item_optim;
    const float* P;                                   /* [n, ldp], b1 added */
    const float* W1_item;                             /* W1 + D: row j at W1_item + j*ldw1, D columns */
    const float* W[FR_PAIR_MLP_MAX_LINEARS - 1];      /* linears 2 .. n_linears */
    const float* bias[FR_PAIR_MLP_MAX_LINEARS - 1];
    const int64_t* cand;                              /* [M*num*n] */
    int64_t ldp;
    int64_t ldw1;
    int64_t n;
    int32_t n_out[FR_PAIR_MLP_MAX_LINEARS - 1];       /* the last used entry is 1 */
    int32_t n1;
    int32_t n_linears;                                /* of the whole MLP: 2..FR_PAIR_MLP_MAX_LINEARS */
    int32_t act;
    int32_t num;
    int32_t M;
} fr_dyn_neg_mlp_args;
FR_API int fr_dyn_neg_mlp_select(const fr_dyn_neg_mlp_args* a, int64_t* out, uint32_t* err_flag, void* stream);
FR_API int fr_dyn_neg_mlp_scores(const fr_dyn_neg_mlp_args* a, float* scores, uint32_t* err_flag, void* stream);

/* ---- sensitive-attribute leakage probe (csrc/probe.hip; fairrec/evaluator/leakage.py) -------------------------------------
 * Up to FR_PROBE_MAX_HEADS attackers ("heads", one per sensitive attribute, no shared parameters) read the same rows of a
 * user-embedding matrix X [U, D] (row stride ldx).  Head a has C_a = classes[a] classes and, with the shared hidden width H,
 *     H > 0 :  z1 = W1 x + b1, h = relu(z1) (x < 0 ? 0 : x), z2 = W2 h + b2        W1 [H, D], W2 [C_a, H]
 *     H == 0:  z2 = W x + b                                                         W  [C_a, D]
 * its loss is the mean softmax cross-entropy over the batch by fr_softmax_ce's formulas (the maximum taken off first,
 * p = __expf(z - mx) / se, term = __logf(se) - (z[y] - mx), dz2 = (p - onehot) / (float)B), relu' = (z1 > 0).
 *
 * Flat layout, shared by params, m, v and grad_out: [head 0][head 1]..., a head = [W1 | b1 | W2 | b2] row-major (H == 0:
 * [W | b]); fr_probe_param_count floats in all.
 *
 * Rows: batch position b reads X row r = rows ? rows[b] : b and head a's label labels[a * ldl + r] (int64): a label table
 * [n_heads, ldl] indexed like X, so a permutation slice needs no gathered copy.  A row index outside 0..U-1 sets
 * FR_DEV_ERR_INDEX_RANGE in *err_flag and the row contributes nothing to any head; a label outside 0..C_a-1 sets it and the row
 * contributes nothing to head a.  The divisor stays B.  No read goes out of bounds.
 *
 * Limits: 1 <= D <= 256; H == 0 or 1 <= H <= 256; 2 <= C_a <= 64; 1 <= n_heads <= 8 (FR_EUNSUPPORTED otherwise, as
 * fr_probe_supported answers); 1 <= B <= 65536 (FR_EUNSUPPORTED); 1 <= U < 2^31, ldx >= D, ldl >= U (rows given) or >= B,
 * B <= U when rows is NULL, step >= 1, Adam as the learner with weight_decay 0, a workspace of
 * fr_probe_step_workspace_bytes, no null pointer but rows and grad_out (FR_EINVAL).  Every refusal comes before anything is
 * launched or written, and fr_last_error names the argument.
 *
 * fr_probe_step: ONE optimiser step of all heads on one batch, in two launches whatever n_heads is.
 *   launch 1  fr_probe_grid(B) workgroups: tiles = ceil(B / 32), tiles per workgroup tpw = ceil(tiles / 256), workgroups =
 *             ceil(tiles / tpw); workgroup w walks tiles w tpw .. -- a function of B alone.  A tile of X is read once and
 *             serves every head: forward, softmax, loss terms, dz2, dW2 = dz2^T h, db2, dh = dz2 W2, dz1 = dh (z1 > 0),
 *             dW1 = dz1^T X, db1.  Every product is a chain of v_mfma_f32_32x32x2_f32, ascending from 0, two inner indices per
 *             step (exact fp32 fma, the first index of a pair first): over the input columns in the forward, over the classes
 *             in dh, over the 32 rows of the tile in the weight gradients (bias gradients: the 32 rows added ascending from 0).
 *             Rows beyond B contribute exact zeros.  A tile's gradient is added to the workgroup's own slot of the workspace
 *             (first tile: stored), each cell by the one lane that owns it: no float atomic.
 *   launch 2  gradient = the slots added in workgroup order; grad_out (optional) receives it; Adam by fr_adam_dense's formulas
 *             with the scalars of `step` on params / m / v: bit for bit fr_adam_dense on grad_out.  loss [1 + n_heads]:
 *             loss[1 + a] = (head a's terms: per tile row slot over the workgroup's tiles, the 32 slots ascending, the
 *             workgroups ascending) * (1 / (float)B); loss[0] = the heads' losses added in head order.
 *   The bits of every output depend on the inputs alone, not on the device: two calls on equal inputs give equal bits.
 * fr_probe_forward: launch 1's forward alone, logits [B, sum C_a] (head a's columns from sum_{a' < a} C_a'), the same bits the
 *   step computes; nothing else is written.  The probe's own kernel, not fr_mlp_infer: one launch for all heads, one read of X.
 * fr_probe_eval: the metric reduction over n held-out rows.  logits [n, sum C_a] (position b), labels / rows / U as above.
 *   Per head: correct [n_heads] int64 = rows whose argmax (the lowest class among equal maxima) is the label; logloss
 *   [n_heads] double = sum of log(se) - (z[y] - mx) in double; class_count [sum C_a] int64 = rows per label; probs
 *   [n, sum C_a] float = the double softmax rounded once (a row with a bad index or label sets the flag and is counted
 *   nowhere; its probabilities are still written).  Partials per 256 rows, added in block order: deterministic.
 *   AUC: torch.sort of a class's probs column, then fr_auc_sorted. */
#define FR_PROBE_MAX_HEADS   8
#define FR_PROBE_MAX_WIDTH   256
#define FR_PROBE_MAX_CLASSES 64
#define FR_PROBE_MAX_BATCH   65536
typedef struct fr_probe_args {
    const float* X;
    const int64_t* rows;      /* [B] or NULL */
    const int64_t* labels;    /* [n_heads, ldl]; unused by fr_probe_forward */
    int64_t U;
    int64_t ldx;
    int64_t ldl;
    int64_t B;
    int32_t D;
    int32_t H;
    int32_t n_heads;
    int32_t classes[FR_PROBE_MAX_HEADS];
} fr_probe_args;
FR_API int fr_probe_supported(int32_t D, int32_t H, int32_t n_heads, const int32_t* classes);
FR_API int64_t fr_probe_param_count(int32_t D, int32_t H, int32_t n_heads, const int32_t* classes);   /* 0: unsupported */
FR_API int32_t fr_probe_grid(int64_t B);                                                            /* 0: unsupported */
FR_API size_t fr_probe_step_workspace_bytes(int32_t D, int32_t H, int32_t n_heads, const int32_t* classes, int64_t B);
FR_API int fr_probe_step(const fr_probe_args* a, float* params, float* m, float* v, const fr_adam* adam, int32_t step,
                         float* loss, float* grad_out, void* ws, size_t ws_bytes, uint32_t* err_flag, void* stream);
FR_API int fr_probe_forward(const fr_probe_args* a, const float* params, float* logits, uint32_t* err_flag, void* stream);
FR_API size_t fr_probe_eval_workspace_bytes(int64_t n, int32_t n_heads, const int32_t* classes);
FR_API int fr_probe_eval(const float* logits, const int64_t* labels, int64_t ldl, const int64_t* rows, int64_t U, int64_t n,
                         int32_t n_heads, const int32_t* classes, int64_t* correct, double* logloss, int64_t* class_count,
                         float* probs, void* ws, size_t ws_bytes, uint32_t* err_flag, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FAIRREC_HIP_H */
