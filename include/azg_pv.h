/*
 * azg_pv.h -- C-ABI of the MI355X (gfx950) policy/value engine.
 *
 * The reference has no FFI layer: its boundary is Python duck typing at
 * network.PyTorchModel (reference network.py:132-265).  This library sits BELOW
 * a Python class that reproduces that surface (alphazero-gomoku_amd/network.py);
 * each entry point below replaces the ATen work behind one reference call:
 *
 *   azg_pv_forward        <- PyTorchModel.predict            (network.py:168-183)
 *                            = AlphaZeroNet.forward in eval mode (network.py:85-117)
 *                              + F.softmax(dim=1) (network.py:180)
 *   azg_pv_forward_boards <- Gomoku.get_encoded_state (games/gomoku.py:130-150) on every
 *                            queued leaf + predict + p * valid (mcts/new_mcts_alpha.py:
 *                            158-166), from int8 boards
 *   azg_pv_train_backward <- train_batch: zero_grad, train-mode forward, log_softmax,
 *                            KLDiv(batchmean) + MSE, loss.backward()  (network.py:213-222)
 *   azg_pv_train_apply    <- clip_grad_norm_(params, 3.0) + Adam.step()
 *                                                            (network.py:223-224, 161)
 *   azg_pv_create/destroy <- AlphaZeroNet.__init__ shape config (network.py:41-73)
 *
 * Conventions
 *  - All pointers are DEVICE pointers (HIP, gfx950) unless stated; fp32 everywhere.
 *  - Python/torch owns every tensor: parameters, gradients and Adam moments are
 *    flat buffers in nn.Module.parameters() order with torch's own per-tensor
 *    layout (see azg_pv_param_layout); BN running stats are a flat buffer of
 *    [mean(c) | var(c)] per BatchNorm layer in module order.  The handle owns only
 *    its workspace (packed weights, activations, partial sums).
 *  - `stream` is a hipStream_t (torch.cuda.current_stream().cuda_stream); every
 *    entry point is asynchronous on it, does no host sync and no allocation
 *    unless the batch exceeds the workspace high-water mark.
 *  - Return value: 0 = ok, nonzero = error; azg_pv_last_error() gives the text
 *    (thread-local).  No C++ exception crosses the ABI.
 *  - One handle per process/GPU; not re-entrant (the reference host is
 *    single-threaded too).
 */
#ifndef AZG_PV_H
#define AZG_PV_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct azg_pv azg_pv;

typedef struct {
    int32_t blocks;    /* residual blocks (reference default 3; BASELINE 6; Pente 10) */
    int32_t channels;  /* 64, 128 or 256 */
    int32_t board;     /* 15 (only 15x15 is built) */
    int32_t in_ch;     /* 3 input planes */
} azg_pv_config;

/* Version of this ABI (bumped on incompatible change). */
int32_t azg_pv_abi_version(void);

const char* azg_pv_last_error(void);

int32_t azg_pv_create(const azg_pv_config* cfg, azg_pv** out);
int32_t azg_pv_destroy(azg_pv* h);

/* Number of trainable parameters (flat length) and of BN running-stat floats. */
int64_t azg_pv_param_count(const azg_pv* h);
int64_t azg_pv_bn_count(const azg_pv* h);
int32_t azg_pv_num_param_tensors(const azg_pv* h);
/* HOST arrays of length azg_pv_num_param_tensors: element offset and numel of each
 * parameter tensor inside the flat buffer, in nn.Module.parameters() order. */
int32_t azg_pv_param_layout(const azg_pv* h, int64_t* offsets, int64_t* numels);

/* Bind torch-owned flat buffers.  params: azg_pv_param_count floats; grads:
 * azg_pv_grad_count floats = the parameter gradients followed by ONE skip word
 * (ABI 3): azg_pv_train_backward writes 1.0 there when its split-fp16 forward (key 49)
 * met an activation beyond fp16's range, else 0.0; a data-parallel caller all-reduces
 * the whole buffer (any nonzero result skips the step on every rank) and
 * azg_pv_train_apply commits the step only where the word is 0.  bn_stats:
 * azg_pv_bn_count floats.  grads may be NULL for inference-only use. */
int32_t azg_pv_bind(azg_pv* h, float* params, float* grads, float* bn_stats);
int64_t azg_pv_grad_count(const azg_pv* h);

/* Optional: bind the int64 num_batches_tracked counters, one per BatchNorm layer
 * in module order (azg_pv_num_bn_layers of them, device).  Each
 * azg_pv_train_backward then advances all of them by one inside its own kernels
 * (the train-mode forward's update, network.py:213 via nn.BatchNorm2d). */
int32_t azg_pv_bind_counters(azg_pv* h, int64_t* num_batches_tracked);
int32_t azg_pv_num_bn_layers(const azg_pv* h);

/* Optional: a running average of the weights (EMA), kept by the Adam kernel.  The caller
 * owns two device buffers, ema_params of azg_pv_param_count floats and ema_bn of
 * azg_pv_bn_count floats, and initialises them (usually to the current parameters and BN
 * running stats).  While bound, every azg_pv_train_apply that COMMITS moves them inside its
 * own pass over the parameters (no extra launch):
 *   ema_params[i] = fmaf(w, p_new[i] - ema_params[i], ema_params[i])
 *   ema_bn[i]     = fmaf(w, bn[i]    - ema_bn[i],     ema_bn[i])
 * with w = (float)(1.0 - (double)decay), p_new the parameter the step just wrote and bn the
 * running stats the step's azg_pv_train_backward produced.  A step that does not commit
 * (the skip word, azg_pv_train_apply) does not touch them.  The average is never read by
 * the library's forwards: copy it into a second handle's buffers to evaluate it.
 * Both pointers NULL unbinds (decay is then ignored).  Returns nonzero (azg_pv_last_error
 * names azg_pv_bind_ema) and leaves the handle as it was on a null handle, exactly one NULL
 * pointer, or a decay outside [0, 1) or NaN.  Makes no device call; may be called before or
 * after azg_pv_bind.
 * azg_pv_get_ema: 1 if an average is bound, 0 if not, -1 on a null handle; the non-NULL
 * outputs (HOST pointers) receive the bound pointers and decay (NULL, NULL, 0 when off). */
int32_t azg_pv_bind_ema(azg_pv* h, float* ema_params, float* ema_bn, float decay);
int32_t azg_pv_get_ema(const azg_pv* h, float** ema_params, float** ema_bn, float* decay);

/* Parameters or BN stats changed outside the library (load_state_dict, copy_, a
 * write through the bound pointers, a collective that rewrites them): re-derive
 * packed weights / folded BN before the next forward AND the next train step.
 * azg_pv_train_apply refreshes the packs itself; between two train steps the
 * library trusts them unless this is called (the Python engine calls it whenever a
 * parameter tensor's version counter moved). */
int32_t azg_pv_mark_dirty(azg_pv* h);

/* Eval-mode forward (BN running stats).  x: [batch,3,15,15] NCHW fp32.
 * probs: [batch,225] softmax(logits); values: [batch,1] tanh; logits: optional
 * [batch,225] (NULL to skip). */
int32_t azg_pv_forward(azg_pv* h, const float* x, int32_t batch,
                       float* probs, float* values, float* logits, void* stream);

/* Eval-mode forward from int8 boards: boards [batch,225] (0 empty, 1, 2), players
 * [batch] (side to move, 1|2), both device.  The reference encoding (planes
 * board==player, board==3-player, ones) is built inside the stem kernel.  probs /
 * values as azg_pv_forward; priors (optional, NULL to skip): probs * (board == 0),
 * the reference's masked prior, bitwise equal to numpy's p * valid. */
int32_t azg_pv_forward_boards(azg_pv* h, const int8_t* boards, const int8_t* players, int32_t batch,
                              float* probs, float* values, float* priors, void* stream);

/* azg_pv_forward_boards under board symmetries.  Symmetry s in 0..7 is the one of
 * MCTS.symmetries (mcts/new_mcts_alpha.py:42-56) and of azg_pv_replay_gather: np.rot90 by
 * k = s >> 1 (counter-clockwise), then a column flip when s is odd.  The net sees the
 * image; the result for an image square is returned at the board square it came from, and
 * the value is untouched.  The transform costs no extra pass: the stem reads the board
 * through the square permutation and the heads' last kernel stores through its inverse.
 * mode 0: board b is evaluated as its image syms[b] (device int8 [batch], values 0..7;
 *         a value outside is taken & 7; syms == NULL means all 0 and is bitwise
 *         azg_pv_forward_boards).  probs / values / priors come back in the BOARD's
 *         own coordinates, bitwise what transforming on the host, azg_pv_forward_boards
 *         and transforming back give.
 * mode 1: every board is evaluated as all 8 images (8*batch images in one forward) and
 *         probs / values are their mean, summed in image order 0..7 and scaled by 1/8
 *         (bitwise the sequential float32 sum of the 8 mode-0 results); syms is
 *         ignored.  batch <= 2048.
 * priors (optional): probs * (board == 0) on the caller's untransformed board.
 * Checked first, before the bound check and any device call: null handle, mode not 0 or
 * 1, negative batch, batch > 2048 in mode 1, null boards / players / probs / values with
 * batch > 0.  batch 0 returns 0.
 * Like boards and players, the caller's syms buffer must stay intact until the forward
 * is settled: azg_pv_recover recomputes a posted launch from the same boards, players and
 * syms with the same symmetry handling into the same outputs. */
int32_t azg_pv_forward_boards_sym(azg_pv* h, const int8_t* boards, const int8_t* players,
                                  const int8_t* syms, int32_t mode, int32_t batch,
                                  float* probs, float* values, float* priors, void* stream);

/* Eval precision of ONE handle (not a tuning key: those are process-wide).
 * AZG_PV_EVAL_EXACT (the default): the eval forward runs the arithmetic key 19 selects, all
 * of which hold 1e-5 parity with the fp32 reference.
 * AZG_PV_EVAL_FP16: the residual convs run on fp16 operands with ONE product per MFMA step
 * (the 16x16x32 board tower without the split's two correction products): conv operands are
 * rounded once to fp16 (the weights times the layer's 2^e, the activations under the
 * activation-exponent fold), accumulated in fp32; the trunk, the BN epilogue, the stem and
 * the heads stay fp32.  Outputs deviate from the fp32 reference by about 1e-3 on values and
 * 1e-4 on probabilities: meant for self-play leaf evaluation, not for gating or anything
 * compared with the reference.  In this mode every azg_pv_forward* entry point, every batch
 * size and every launch form computes the same MFMA sequence per element, whatever keys 5, 6
 * and 19 say; an activation beyond fp16's range is still posted and azg_pv_recover recomputes
 * it in fp32.  azg_pv_recover reruns a posted launch in the precision it was launched with.
 * set: returns nonzero (azg_pv_last_error) on a null handle, an unknown value, or FP16 on a
 * net it has no kernel for -- it needs channels == 128 and 1..32 blocks (channels 256 and
 * 64 have no one-product form); checked before any device call.  get: -1 on a null handle. */
enum { AZG_PV_EVAL_EXACT = 0, AZG_PV_EVAL_FP16 = 1 };
int32_t azg_pv_set_eval_precision(azg_pv* h, int32_t precision);
int32_t azg_pv_get_eval_precision(const azg_pv* h);

/* Train-mode forward + loss + backward on the local batch (reference
 * network.py:213-222).  Writes d(loss)/d(param) into the bound grad buffer
 * (overwrites: zero_grad semantics), updates BN running stats (momentum 0.1,
 * unbiased var), and writes {policy_loss, value_loss, total_loss} as 3 floats
 * to losses (device).  pis: [batch,225]; zs: [batch,1]. */
int32_t azg_pv_train_backward(azg_pv* h, const float* x, const float* pis,
                              const float* zs, int32_t batch, float* losses,
                              void* stream);

/* azg_pv_train_backward with per-example loss weights: wp (policy) and wv (value), device
 * fp32 [batch], either may be NULL (= all ones).  The losses become
 *   policy_loss = (1/batch) sum_b wp[b] KL_b,  value_loss = (1/batch) sum_b wv[b] (v_b - z_b)^2
 * -- the divisor stays `batch`, not the sum of the weights -- and each board's gradient seeds
 * are the unweighted ones times its weight.  Weights of 1.0 give azg_pv_train_backward's
 * bits; with both pointers NULL exactly its kernels are launched.  A zero-weight board still
 * passes through the forward and the batch statistics of every BN.  The values are not
 * checked (they are on the device): callers pass finite weights >= 0.
 * azg_pv_train_fp32_once applies to this call as to the plain one. */
int32_t azg_pv_train_backward_weighted(azg_pv* h, const float* x, const float* pis,
                                       const float* zs, const float* wp, const float* wv,
                                       int32_t batch, float* losses, void* stream);

/* clip_grad_norm_(max_norm) over the bound grads (call after any DP all-reduce
 * of the grad buffer), then one Adam step (torch semantics: L2-coupled weight
 * decay, bias correction for `step`, which is the post-increment step count).
 * exp_avg / exp_avg_sq: flat buffers like params.  total_norm (device, 1 float,
 * may be NULL) receives the pre-clip global L2 norm.
 * If the grad buffer's skip word (azg_pv_bind) is nonzero the step does NOT commit:
 * params, grads and moments are left as they are, the BN running stats and counters
 * are restored to what the step started from, and the skipped-step count
 * (azg_pv_train_status) advances.  The caller then redoes the step, e.g. after
 * azg_pv_train_fp32_once, with the same `step`.  A committed step also moves the weight
 * average bound with azg_pv_bind_ema, if any; a skipped one leaves it as it is. */
int32_t azg_pv_train_apply(azg_pv* h, float* exp_avg, float* exp_avg_sq,
                           int64_t step, float lr, float beta1, float beta2,
                           float eps, float weight_decay, float max_norm,
                           float* total_norm, void* stream);

/* The next azg_pv_train_backward on this handle runs its forward convs with fp32
 * MFMA (tuning key 49 = 0 for that one step): the redo of a skipped step. */
int32_t azg_pv_train_fp32_once(azg_pv* h);

/* Training batch from a device-resident replay ring (handle-free; replaces
 * ReplayBuffer.sample's random.sample + np.stack + three host-to-device copies, reference
 * train.py:272-297, and the 8 stored images per position of MCTS.symmetries,
 * mcts/new_mcts_alpha.py:42-56).  The ring stores each position ONCE: stones
 * [cap_pos][225] int8 (0 empty, 1 side to move, 2 opponent), pis [cap_pos][225], zs
 * [cap_pos]; it holds `count` positions, the oldest at slot `head`.  nsym is 1 or 8.
 * ids [batch] (device, int64) are image numbers in [0, count*nsym): image i is symmetry
 * i % nsym of position (head + i / nsym) % cap_pos; symmetry s is np.rot90 by k = s / 2
 * (counter-clockwise) followed by a column flip when s is odd.  An id outside the range
 * is clamped into it (the kernel never reads outside the ring; callers range-check on
 * the host).  Outputs: x [batch,3,15,15] (planes stones == 1, stones == 2, ones:
 * games/gomoku.py:130-150), pi_out [batch,225], z_out [batch,1] -- copies and 0/1
 * constants only, so bitwise what numpy gives.  Arguments are checked before any device
 * call: a null pointer, nsym not 1 or 8, batch < 1, cap_pos < 1, count outside
 * [1, cap_pos] or head outside [0, cap_pos) return nonzero.  One launch, asynchronous
 * on `stream`, no allocation. */
int32_t azg_pv_replay_gather(const int8_t* stones, const float* pis, const float* zs,
                             int32_t cap_pos, int32_t head, int32_t count, int32_t nsym,
                             const int64_t* ids, int32_t batch,
                             float* x, float* pi_out, float* z_out, void* stream);

/* One fp32 value per position of the same ring (vals [cap_pos], by slot: the policy loss
 * weight), gathered for the same image ids: out[b] = vals[slot of image ids[b]], with
 * azg_pv_replay_gather's id -> slot map, clamping and argument checks.  One launch,
 * asynchronous on `stream`, no allocation. */
int32_t azg_pv_replay_gather_weight(const float* vals, int32_t cap_pos, int32_t head,
                                    int32_t count, int32_t nsym, const int64_t* ids,
                                    int32_t batch, float* out, void* stream);

/* Surprise-weighted sampling from the same ring (handle-free; three entry points beside
 * azg_pv_replay_gather, which they feed and do not change).  Every position carries a
 * weight in FIXED POINT: weights [cap_pos] uint32, one unit of weight = 65536 quanta, at
 * most 2^31 - 1 quanta.  Sums of integers are exact in any order and the draw is an integer
 * function of the random words, so a host restatement in integers gives the same ids.
 *
 * azg_pv_replay_surprise_weights: weights of freshly added positions from their "surprise"
 * (KataGo's policy surprise weighting: field AZG_PV_SCORE_KL of azg_pv_score_outputs'
 * records, below).  surprise (device fp32) holds n_sum records `stride` floats apart; record
 * i is sanitised to s_i = surprise[i*stride] if finite and > 0, else 0, and S = sum of ALL
 * n_sum s_i in fp64, in an order fixed by n_sum alone (one workgroup: thread i adds i,
 * i + 256, ... in increasing order, then a fixed tree; no atomics).  In fp64, in this
 * operation order,  w_i = (1 - mix) + mix * n_sum * s_i / S   (w_i = 1 when S == 0): a
 * uniform share plus a share in proportion to the surprise, mean 1 over the n_sum records.
 * Only the NEWEST n records (i in [n_sum - n, n_sum), n <= n_sum: the ones that survive in a
 * ring of cap_pos when more were added at once) are written, record n_sum - n + k to
 * weights[(at + k) % cap_pos], as  min(2^31 - 1, llrint(w_i * 65536))  quanta.  The sum
 * range is thus given by the one extra length n_sum, not by a second pointer.
 * Checked before any device call: null surprise or weights, mix outside [0, 1] (NaN
 * included), stride < 1, cap_pos < 1, n outside [1, cap_pos], n_sum < n, at outside
 * [0, cap_pos).  One launch of one workgroup.
 *
 * azg_pv_replay_prefix: prefix[j] = sum over i <= j of weights[(head + i) % cap_pos], uint64,
 * for j < count -- running sums in ring order (oldest position first).  A three-pass scan
 * (per-thread chunks, wavefront scan, LDS across waves; tile totals; carried offsets) that
 * uses `prefix` itself as its only workspace.  Call it when the weights or the ring have
 * changed, not per batch.  Checked: null weights or prefix, cap_pos < 1, count outside
 * [1, cap_pos], head outside [0, cap_pos).  One launch up to 1024 positions, else three.
 *
 * azg_pv_replay_draw: batch image ids, with replacement.  rnd [batch][2] (device uint64) are
 * uniform random words.  With total = prefix[count - 1], element k takes
 * t = floor(rnd[2k] * total / 2^64) (the high half of the 128-bit product), j = the smallest
 * index with prefix[j] > t (binary search), and ids[k] = j * nsym + (nsym == 8 ?
 * rnd[2k+1] & 7 : 0) -- azg_pv_replay_gather's image numbers.  A position is chosen with
 * probability weight / total up to 2^-64 * count; a position of weight 0 never.  With
 * total == 0 (no weight anywhere: the caller's error) every id is position count - 1: ids
 * never leave the ring.  Checked: null prefix, rnd or ids, count < 1, nsym not 1 or 8,
 * batch < 1.  One launch.
 * All three are asynchronous on `stream` and allocate nothing. */
int32_t azg_pv_replay_surprise_weights(const float* surprise, int32_t stride, int32_t n, int32_t n_sum,
                                       double mix, uint32_t* weights, int32_t cap_pos, int32_t at,
                                       void* stream);
int32_t azg_pv_replay_prefix(const uint32_t* weights, int32_t cap_pos, int32_t head, int32_t count,
                             uint64_t* prefix, void* stream);
int32_t azg_pv_replay_draw(const uint64_t* prefix, int32_t count, int32_t nsym, const uint64_t* rnd,
                           int32_t batch, int64_t* ids, void* stream);

/* Position averaging in the same ring (handle-free; two entry points beside
 * azg_pv_replay_gather, which reads their outputs through the pis / zs / vals pointers it
 * always took and is not changed).  Positions with the same board -- with nsym = 8: up to a
 * rotation or a flip -- get the mean of their targets.  Ring index i is slot
 * (head + i) % cap_pos.  Everything is an integer or an fp64 sum in ring order rounded once,
 * so a host restatement gives the same bits; no atomics.
 *
 * azg_pv_replay_canon_keys: keys_out[i] (64 bits in an int64) and syms_out[i] (int8) for ring
 * index i < count.  splitmix64(x): x += 0x9E3779B97F4A7C15; x = (x ^ x >> 30) *
 * 0xBF58476D1CE4E5B9; x = (x ^ x >> 27) * 0x94D049BB133111EB; return x ^ x >> 31 (mod 2^64).
 * Z(j, v) = splitmix64(2 j + v - 1) for square j and stone v in {1, 2}.  Image s of a position
 * is img_s[j] = stones[src(j, s)], src being azg_pv_replay_gather's map (image square j of
 * symmetry s reads board square src), and h_s = the XOR of Z(j, img_s[j]) over its non-empty
 * squares (0 for the empty board).  nsym = 8: key = min_s h_s compared as unsigned, sym = the
 * smallest s attaining it -- all 8 images of a board get one key, and img_sym is the same
 * CANONICAL BOARD for all of them.  nsym = 1: key = h_0, sym = 0 (exact repeats only).
 * Checked before any device call: null stones, keys_out or syms_out, nsym not 1 or 8,
 * cap_pos < 1, count outside [1, cap_pos], head outside [0, cap_pos).  One launch.
 *
 * azg_pv_replay_average: keys_sorted [count] are the keys in ascending order of a STABLE sort
 * and perm [count] (int64) the ring index at each sorted place (equal keys adjacent, in ring
 * order); syms [count] is indexed by ring index.  Place k starts a group when k == 0, its key
 * differs from place k - 1's, or its canonical board stones[src(j, sym)] differs from place
 * k - 1's in any square: unequal boards never merge, a key collision can only split a group.
 * For a group with members m = 1..n in ring order, c_m = member m's sym, in fp64 in member
 * order:  W = sum pw_m,  A[j] = sum pw_m * pis_m[src(j, c_m)]  for canonical square j,
 * Zs = sum zs_m.  pw (by slot) and pw_avg are both NULL (every pw_m = 1.0, nothing written)
 * or both set.  Written for every member -- pi_avg [cap_pos][225], z_avg and pw_avg
 * [cap_pos] by SLOT, as the gather reads them; group_first and group_size [count] int32 by
 * ring index:
 *   pi_avg_m[src(j, c_m)] = (float)(A[j] / W) if W > 0, else pis_m[src(j, c_m)]
 *   z_avg_m = (float)(Zs / n)     pw_avg_m = (float)(W / n)
 *   group_first = the ring index of the group's oldest member     group_size = n
 * A group of one comes out bit-identical to its raw targets.  A perm entry outside
 * [0, count) is clamped into it.  Checked before any device call: null stones, pis, zs,
 * keys_sorted, perm, syms, pi_avg, z_avg, group_first or group_size, exactly one of pw /
 * pw_avg null, cap_pos < 1, count outside [1, cap_pos], head outside [0, cap_pos).  Two
 * launches: the group starts (one wavefront per place), then one workgroup per group, which
 * walks its members 256 at a time -- a group may be the whole ring.
 * Both are asynchronous on `stream` and allocate nothing. */
int32_t azg_pv_replay_canon_keys(const int8_t* stones, int32_t cap_pos, int32_t head, int32_t count,
                                 int32_t nsym, int64_t* keys_out, int8_t* syms_out, void* stream);
int32_t azg_pv_replay_average(const int8_t* stones, const float* pis, const float* zs, const float* pw,
                              int32_t cap_pos, int32_t head, int32_t count, const int64_t* keys_sorted,
                              const int64_t* perm, const int8_t* syms, float* pi_avg, float* z_avg,
                              float* pw_avg, int32_t* group_first, int32_t* group_size, void* stream);

/* Score eval-forward outputs against targets without a train step (handle-free): the two
 * loss terms of the reference's train_batch -- KLDivLoss(batchmean) on log_softmax(logits)
 * and MSELoss on the value, network.py:162-163,216-219 -- per board and summed, plus policy
 * and value metrics.  Nothing is written but per_board and sums.
 * Inputs (device fp32): logits [batch][225], exactly what azg_pv_forward writes to its
 * `logits` output; values [batch]; pis [batch][225]; zs [batch].  Targets are just device
 * tensors: passing ANOTHER model's probs and values as pis and zs gives the policy drift
 * (KL) and value distance between two models.
 * per_board [batch][AZG_PV_SCORE_FIELDS]: one record per board, from that board's inputs
 * only (one wavefront per board), with lp_j = (l_j - max) - logf(sum_j expf(l_j - max)),
 * t = pis, v = values, z = zs:
 *   0 KL           sum over t_j > 0 of t_j * (logf(t_j) - lp_j)   (the train step's term)
 *   1 SQ           (v - z)^2
 *   2 ENTROPY      -sum_j expf(lp_j) * lp_j   (from lp: an underflowed probability adds 0)
 *   3 TOP1         1.0 if argmax_j l_j == argmax_j t_j, else 0.0 (both argmaxes take the
 *                  lowest index among equal maxima)
 *   4 P_BEST       expf(lp_j*), j* = argmax_j t_j
 *   5 V_AGREE      1.0 if v * z > 0, else 0.0
 *   6 DECIDED      1.0 if z != 0, else 0.0
 *   7 TARGET_MASS  sum_j t_j
 * sums [AZG_PV_SCORE_FIELDS] (device fp64, or NULL to skip): the records summed in fp64 in
 * an order that depends on batch alone (one workgroup, thread i adds records i, i + 256,
 * ... in increasing order, then a fixed tree; no atomics), so equal records give equal
 * sums bit for bit.  Means are the caller's: policy loss = sums[0] / batch, value loss =
 * sums[1] / batch, value sign agreement = sums[5] / sums[6].
 * Arguments are checked before any device call: a null logits, values, pis, zs or
 * per_board, or batch < 1, returns nonzero and azg_pv_last_error names the argument.  Two
 * launches, asynchronous on `stream`, no allocation. */
enum {
    AZG_PV_SCORE_KL = 0,
    AZG_PV_SCORE_SQ = 1,
    AZG_PV_SCORE_ENTROPY = 2,
    AZG_PV_SCORE_TOP1 = 3,
    AZG_PV_SCORE_P_BEST = 4,
    AZG_PV_SCORE_V_AGREE = 5,
    AZG_PV_SCORE_DECIDED = 6,
    AZG_PV_SCORE_TARGET_MASS = 7,
    AZG_PV_SCORE_FIELDS = 8
};
int32_t azg_pv_score_outputs(const float* logits, const float* values, const float* pis, const float* zs,
                             int32_t batch, float* per_board /* [batch][8] */, double* sums /* [8] or NULL */,
                             void* stream);

/* Kernel-class event timing (bench / roofline instrumentation).  When enabled,
 * every launch of a profiled class is bracketed by hipEvents on the stream it is
 * launched on; azg_pv_profile_read synchronises those events and returns the
 * summed device time (ms) and launch count per class since the last enable. */
enum {
    AZG_PROF_CONV3X3 = 0,   /* residual 3x3 conv, eval epilogue        */
    AZG_PROF_STEM = 1,
    AZG_PROF_HEADS = 2,
    AZG_PROF_TRAIN_CONV = 3, /* train-mode 3x3 conv fwd + dgrad        */
    AZG_PROF_TRAIN_WGRAD = 4,
    AZG_PROF_TRAIN_OTHER = 5,
    AZG_PROF_TOWER = 6,      /* persistent residual tower (all 2*NB convs, one launch),
                                64x64 / 128x64 tiles, 2-4 workgroups per CU          */
    AZG_PROF_TOWER_WIDE = 7, /* the same with 128x128 tiles: 16 waves, 1 workgroup per CU
                                (fp32), or h3_tile's 4 waves of 64x64 (split-fp16, shape 12) */
    AZG_PROF_BOARD = 8,      /* the board-resident tower (split-fp16, C = 128, shape 13): one
                                board's activations in LDS through all 2*NB convs */
    AZG_PROF_BOARD16 = 9,    /* the 16x16x32 board tower (key 19 = 2, C = 128) */
    AZG_PROF_NCLASS = 10
};
int32_t azg_pv_profile_enable(azg_pv* h, int32_t enable);
int32_t azg_pv_profile_read(azg_pv* h, double* ms, int64_t* launches);
/* Boards (eval) / samples (train) processed per class since the last enable, so a
 * caller can price launches of varying batch (self-play) in algorithmic FLOPs.
 * A residual-conv launch (CONV3X3) counts its batch once per conv; a TOWER / TOWER_WIDE /
 * BOARD launch counts its batch once for all 2*blocks convs. */
int32_t azg_pv_profile_boards(const azg_pv* h, int64_t* boards);

/* Keys of azg_pv_set_tuning: process-wide tuning knobs (benchmarks / A-B tests).  The
 * numbers are frozen: benchmarks and scripts pass them as integers.  A retired key
 * belonged to a finished timing study: it sets nothing, in any build, and returns the
 * constant given with it. */
enum azg_pv_tuning_key {
    /* force the 3x3-conv tile shape index (-1 = automatic) */
    AZG_PV_TUNE_CONV_SHAPE = 0,
    /* conv autotuning on/off (default on: the first launch for a (C, M) times every tile
     * shape on the real operands and caches the fastest; shapes give bitwise-identical
     * results, so this never changes numerics) */
    AZG_PV_TUNE_CONV_AUTOTUNE = 1,
    /* query the tuned shape for value = M*1024 + C (-1 if not tuned yet) */
    AZG_PV_TUNE_QUERY_CONV_SHAPE = 2,
    /* retired (ablation mask of the per-layer conv): returns 0 */
    AZG_PV_TUNE_CONV_ABLATION = 3,
    /* retired (per-chunk staging against the halo-staged kernel, the only one now):
     * returns 1 */
    AZG_PV_TUNE_CONV_STAGING = 4,
    /* eval residual tower: 0 one launch per conv, 1 one persistent launch (shape from
     * TOWER_SHAPE), 2 (default) chosen per (C, blocks, batch bucket) by timing every
     * variant on first use -- all bitwise identical */
    AZG_PV_TUNE_TOWER_MODE = 5,
    /* persistent-tower tile shape for TOWER_MODE = 1 (8: 128x64 / 8 waves, default;
     * 5: 64x64 / 4 waves; 10: 128x128 / 16 waves, one workgroup per CU, C = 128, fp32
     * only; 12: h3_tile 128x128 / 4 waves of 64x64, split-fp16 only; 13: the
     * board-resident tower (pv_board.hip: one board per 16-wave workgroup, its
     * activations in LDS through every conv), split-fp16 and C = 128 only -- a shape
     * the current arithmetic lacks runs as 8); with EVAL_ARITH = 2 at C = 128
     * TOWER_MODE / TOWER_SHAPE do not apply (one form: the 16x16x32 board tower) */
    AZG_PV_TUNE_TOWER_SHAPE = 6,
    /* retired (tile shape of the per-layer conv ablations): returns 5 */
    AZG_PV_TUNE_ABLATION_SHAPE = 7,
    /* timing-only ablation mask of the persistent tower (1 no dependency wait, 2 no
     * publish drain; results invalid while set); study build only */
    AZG_PV_TUNE_TOWER_ABLATION = 8,
    /* stem kernel (1 = fp32 MFMA, default; 0 = VALU reference, bitwise equal) */
    AZG_PV_TUNE_STEM_KERNEL = 9,
    /* retired (tile-body variants of the persistent tower; none beat the default):
     * returns 0 */
    AZG_PV_TUNE_TOWER_BODY = 10,
    /* retired (stem ablation mask): returns 0 */
    AZG_PV_TUNE_STEM_ABLATION = 11,
    /* persistent-tower dependency wait bound in microseconds of the waiting wave's
     * awake time (default 100000 = 100 ms; -1 restores it; 0 makes every dependency
     * wait time out at once, exercising the recovery path) */
    AZG_PV_TUNE_TOWER_WAIT_US = 14,
    /* query: 1 if the library was built with the A/B study variants (make study) */
    AZG_PV_TUNE_QUERY_STUDY_BUILD = 15,
    /* persistent-tower claim granularity (1 = one M tile with all its N tiles, run
     * back to back by the claiming workgroup, default: the second tile's halo rows hit
     * the XCD's L2, +2 % at B = 512 and 4096, measured; 0 = one 128x64 tile per
     * claim); bitwise identical results */
    AZG_PV_TUNE_TOWER_CLAIM = 17,
    /* seconds a handle keeps off cross-workgroup waits after azg_pv_recover recomputed
     * one of its timed-out launches (default 30; 0 disables the breaker): the tile towers
     * give way to per-layer convs, and the 16x16x32 board tower (key 19 = 2, the fp16
     * precision) runs one workgroup per board instead of its split form.  A timed-out
     * wait means parts of the dispatch were suspended while others ran (the GPU is
     * shared with another process) */
    AZG_PV_TUNE_BREAKER_SECONDS = 18,
    /* eval residual-conv arithmetic: 2 (default) and 1 split-fp16 -- every fp32 operand
     * x is split into hi = fp16(x), lo = fp16(x - hi) and a product is lo*hi + hi*lo +
     * hi*hi by fp16 MFMAs with fp32 accumulation (weights scaled by a per-layer power
     * of two, undone in the BN scale; error ~2^-22 per product, the fp32 MFMA chain's
     * order of magnitude); 1 sums 16 channels per
     * v_mfma_f32_32x32x16_f16 (per-layer launches, tile towers, the 32x32 board
     * tower), 2 at C = 128 sums 32 per v_mfma_f32_16x16x32_f16 in the 16x16x32 board
     * tower (pv_board16.hip), the one form of that arithmetic (C = 256: as 1); 0 fp32
     * MFMA.  Every eval path (tower, per-layer, recompute) uses the selected
     * arithmetic, so within it the forms are bitwise equal and the forward is
     * batch-independent.  An activation at or above fp16's range (65520 rounds to inf)
     * makes its products non-finite: the epilogue posts the launch and azg_pv_recover
     * recomputes it with fp32 MFMA */
    AZG_PV_TUNE_EVAL_ARITH = 19,
    /* the split-fp16 tower's tile body (1 = halo rows keyed on the board position,
     * conflict-free fragment reads, default; 0 = row-keyed); bitwise identical */
    AZG_PV_TUNE_H3_TOWER_BODY = 20,
    /* per-layer 128x64 conv: the last partial round of workgroups runs as a second
     * launch of 64x64 tiles (1, default) or not (0); bitwise identical */
    AZG_PV_TUNE_CONV_TAIL_SPLIT = 21,
    /* per-layer 128x64 conv tile body (1 = halo rows keyed on the board position,
     * conflict-free fragment reads, default; 0 = row-keyed; 4 / 5 = LDS-DMA staging);
     * bitwise identical */
    AZG_PV_TUNE_CONV_BODY = 22,
    /* train forward BN apply + ReLU (+ residual) folded into the next conv's halo
     * staging (1, default; C <= 128 only: at C = 256 the prologue spills and the
     * separate passes are faster) or separate bn_apply passes (0); bitwise identical */
    AZG_PV_TUNE_TRAIN_FUSE_APPLY = 23,
    /* train BN finalize run by the last workgroup of the conv producing the layer's
     * partials (1, default) or by separate finalize kernels (0); one shared fp64
     * reduction order, bitwise identical */
    AZG_PV_TUNE_TRAIN_FUSE_FINALIZE = 24,
    /* train conv weight-grad pixel splits (0 = automatic, default; 8..64, a multiple
     * of 8); bitwise identical only at a fixed value */
    AZG_PV_TUNE_WGRAD_SPLITS = 27,
    /* retired (the 64x64 / 128x64 towers with sc1 dependent loads and no acquire, at
     * two or more workgroups per CU: outside the microarch guide's measured envelope;
     * the acquire is used there and the sc1 form only for the one-workgroup-per-CU
     * 16-wave tile): returns 0 */
    AZG_PV_TUNE_TOWER_SC1_LOADS = 31,
    /* train BN apply / BN-backward apply passes: workgroup cap of their grid-stride
     * launch (0 = four float4 per thread, default); bitwise identical */
    AZG_PV_TUNE_TRAIN_APPLY_GRID = 44,
    /* train weight-grad tile (1 = padded-row table, buffer LDS-DMA, slabs in the MFMA
     * layout, default; 0 = round-4 form); bitwise identical */
    AZG_PV_TUNE_WGRAD_TILE = 48,
    /* train-step forward convs: 2 (default) split-fp16 with all four hi / lo products
     * (~2^-33 per product: the two-step goldens hold), 1 three products, 0 fp32 MFMA;
     * the weight grads stay fp32; a staged activation beyond fp16's range sets the
     * step's skip word (azg_pv_bind): the step does not commit and the caller redoes
     * it in fp32 (azg_pv_train_fp32_once) */
    AZG_PV_TUNE_TRAIN_ARITH = 49,
    /* train-step dgrad convs: 0 (default) fp32 MFMA, 1 split-fp16 with three products,
     * 2 with four (inputs scaled by a power of two from their maximum); measured
     * slower and below the two-step goldens */
    AZG_PV_TUNE_TRAIN_DGRAD_ARITH = 50,
    /* timing ablations of the board towers (1 no DMA wait, 2 no barrier, 4 no
     * epilogue; results invalid while set); study build only: the product library
     * does not know the key (-1) */
    AZG_PV_TUNE_BOARD_ABLATION = 51,
    /* EVAL_ARITH = 2 at C = 128: the largest batch whose boards each run over three
     * 8-wave workgroups (pixel thirds) that exchange their conv outputs' 16 boundary
     * rows through L2 (default 85: 3 x 85 workgroups fit 256 CUs; 0 never) -- bitwise
     * the one-workgroup tower, about 2/3 of its latency; a timed-out exchange wait
     * (TOWER_WAIT_US) posts the launch (azg_pv_recover reruns it one workgroup per
     * board) */
    AZG_PV_TUNE_BOARD16_SPLIT_MAX = 52
};

/* Sets the knob `key` (an azg_pv_tuning_key) and returns its previous value; a value the
 * key does not accept leaves it unchanged.  The two queries return their answer; an
 * unknown key returns -1. */
int32_t azg_pv_set_tuning(int32_t key, int32_t value);

/* Persistent-tower dependency waits (pv_tower.hip).  A tile of the one-launch eval
 * tower waits for the three tiles of the previous layer whose rows its halo reads.
 * The wait is bounded by the waiting wave's AWAKE time (s_memrealtime deltas, each
 * capped at 10 us, so a wave that was suspended together with its producer resumes
 * without timing out); past the bound (key 14) the tile computes on stale inputs, the
 * launch drains, and the launch's sequence number is posted to a ring in pinned,
 * mapped host memory.  Every forward that runs the tower gets a sequence number
 * (azg_pv_last_seq: the last one on this handle, 0 if the last forward ran per-layer
 * convs).  azg_pv_recover(seq) -- called after synchronising with that forward --
 * recomputes a posted launch with per-layer convs (bitwise equal to a tower that did
 * not time out) into the SAME output buffers on `stream`, provided the caller's input
 * and output buffers of that forward are still intact; *recovered = 1 then (0: the
 * launch did not time out).  The Python layer does this at every host-synchronising
 * forward (predict, predict_boards, BoardEvaluator.wait), so a timeout costs one
 * per-layer forward instead of an error. */
/* Error word of the last tower launch on this handle: 1 if one of its waits timed
 * out, 0 otherwise and before the handle has launched a tower (synchronises `stream`). */
int32_t azg_pv_tower_status(azg_pv* h, void* stream);
uint32_t azg_pv_last_seq(const azg_pv* h);
int32_t azg_pv_recover(azg_pv* h, uint32_t seq, int32_t* recovered, void* stream);

/* Number of posted eval launches not yet recovered -- timed-out tower launches and
 * split-fp16 launches whose activations left fp16's range (a plain host load of the
 * pinned rings: complete for every forward the caller has synchronised with).
 * azg_pv_posted(seq): bit 0 = launch `seq` timed out, bit 1 = it met a range overflow,
 * both not yet recovered (0: nothing to settle).  The Python layer raises on a posted
 * launch it cannot recover (its buffers are gone).  azg_pv_clear_status drops every
 * posted launch without recomputing it, zeroes the skipped-step count and closes the
 * breaker (key 18).  It leaves the overflow flag of a train step in flight alone: a step
 * still queued when it is called is skipped or committed as if it had not been called
 * (a train call that failed on the host after its forward had set the flag leaves it to
 * the next step, which is then skipped once). */
int32_t azg_pv_status(const azg_pv* h);
int32_t azg_pv_posted(const azg_pv* h, uint32_t seq);
int32_t azg_pv_clear_status(azg_pv* h);
/* Train steps azg_pv_train_apply skipped because their skip word was set (a split-fp16
 * train forward, key 49, met an activation beyond fp16's range on some rank) since the
 * last azg_pv_clear_status (a plain host load; complete for every step the caller has
 * synchronised with). */
int32_t azg_pv_train_status(const azg_pv* h);

/* Self-describing record of the tower's waits since the last azg_pv_tower_diag_clear
 * (device counters + the first timed-out wait; synchronises `stream`).  Times are
 * microseconds from s_memrealtime (100 MHz).  hwid = the HW_ID hardware register of the
 * wave (CU, SE, VMID, queue, ...), xcc = its XCD (HW_REG_XCC_ID). */
typedef struct {
    uint32_t timeouts;          /* waits that timed out */
    uint32_t waits_over_100us;  /* waits whose awake time exceeded 0.1 / 1 / 10 / 100 ms */
    uint32_t waits_over_1ms;
    uint32_t waits_over_10ms;
    uint32_t waits_over_100ms;
    uint32_t max_wait_us;       /* longest awake wait */
    uint32_t recovered;         /* launches recomputed by azg_pv_recover (host count) */
    /* the first timed-out wait */
    uint32_t seq;               /* its launch */
    uint32_t layer;             /* the waiting tile: conv layer (1 .. 2*blocks-1) and M tile */
    uint32_t mtile;
    uint32_t wait_mtile;        /* the layer-1 M tile it waited on */
    uint32_t observed;          /* that tile's completion counter when the wait gave up */
    uint32_t needed;            /* ... and the value it waited for (N tiles per M tile) */
    uint32_t waited_us;         /* awake time of the wait */
    uint32_t wall_us;           /* wall time from the wait's start to its timeout */
    uint32_t waiter_hwid, waiter_xcc;
    uint32_t claims;            /* tiles claimed in the launch when it timed out */
    uint32_t producer_claimed;  /* 1: the producer tile had been claimed */
    uint32_t producer_started;  /* 1: its workgroup had started it in this launch */
    uint32_t producer_hwid, producer_xcc;
    int32_t producer_start_us;  /* its start relative to the wait's start */
    uint32_t max_wall_us;       /* longest WALL time of a wait (awake + suspended) */
    uint32_t waits_suspended;   /* waits whose wall time exceeded their awake time by > 1 ms */
    uint32_t breaker_trips;     /* recoveries that opened the breaker (key 18) */
    uint32_t breaker_launches;  /* forwards the open breaker changed: per layer, or board16 unsplit */
    uint32_t h3_overflows;      /* split-fp16 forwards recomputed with fp32 MFMA (key 19: an activation
                                   beyond fp16's range, 65504) */
    uint32_t train_h3_overflows;   /* train steps skipped because a split-fp16 train forward (key 49) met an
                                      activation beyond fp16's range (= azg_pv_train_status; the Python layer
                                      redoes each in fp32; azg_pv_clear_status resets it) */
    uint32_t reserved[3];
} azg_pv_tower_diag;
int32_t azg_pv_tower_diag_read(azg_pv* h, azg_pv_tower_diag* out, void* stream);
int32_t azg_pv_tower_diag_clear(azg_pv* h, void* stream);

/* Debug/test access to train-workspace activations of the last train step:
 * copies the interior [batch][15][15][C] (NHWC) of buffer `which` (block `index`
 * where relevant) into dst (device, batch*225*C floats), stream-ordered.
 * which: 0 z0 (stem conv out), 1 a0 (stem act), 2 z1[i], 3 h[i], 4 z2[i],
 * 5 xo[i] (block out), 6 gX, 7 DZ, 8 DH, 9 GR, 10 gX snapshot i (env
 * AZG_DEBUG_SNAP), and raw head features (no unpadding): 11 policy features
 * [batch][450], 12 value features [batch][225], 13 value hidden [batch][64]. */
int32_t azg_pv_debug_copy(azg_pv* h, int32_t which, int32_t index, float* dst,
                          int32_t batch, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AZG_PV_H */
