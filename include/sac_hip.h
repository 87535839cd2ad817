/* sac_hip.h -- C ABI of libsac_hip.so: the MI355X-native SAC training inner loop.
 *
 * Drop-in boundary for the hot path of jeremy29tien/robosuite-benchmark:
 *   replay_buffer.random_batch(B)  ->  trainer.train(batch)
 * as driven by  /root/reference/util/rlkit_custom.py:233-240.  The reference has no FFI
 * (pure Python duck typing); each entry point below names the
 * reference interface it replaces.  Plain pointers and sizes only; no torch types.
 *
 * Conventions
 *   - every function returns 0 on success, <0 on error; sac_last_error() gives the text
 *     of the last error on the calling thread.  The library never aborts the process.
 *   - the library owns all device memory behind the opaque handles; the caller owns every
 *     host buffer passed in or out.  Host buffers are plain (pageable) memory; the library
 *     stages them through its own pinned buffers.
 *   - a handle is bound to one GPU and one HIP stream; handles are not thread-safe, distinct
 *     handles are independent.
 *   - all floating point is IEEE fp32; sampled indices are int64 (NumPy's default dtype).
 */
#ifndef SAC_HIP_H
#define SAC_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sac_buffer sac_buffer_t;
typedef struct sac_trainer sac_trainer_t;

const char *sac_last_error(void);
/* number of visible GPUs (0 when there is none: every create call then fails loudly) */
int sac_device_count(void);
const char *sac_version(void);

/* ------------------------------------------------------------------------------------------
 * Replay buffer in HBM, structure-of-arrays fp32.
 * Replaces rlkit EnvReplayBuffer / SimpleReplayBuffer as constructed at
 * /root/reference/util/rlkit_utils.py:139-142 and used at
 * /root/reference/util/rlkit_custom.py:207,230 (add_paths), :235-236 (random_batch),
 * :250-253 (get_diagnostics -> 'size').
 * ------------------------------------------------------------------------------------------ */
int sac_buffer_create(sac_buffer_t **out, int64_t capacity, int obs_dim, int act_dim, int device);
int sac_buffer_destroy(sac_buffer_t *buf);

/* add_paths / add_sample: append n transitions at the ring head (top = (top+1) % capacity,
 * size = min(size+1, capacity)).  Row-major host arrays: obs (n,O) act (n,A) rew (n) next_obs (n,O)
 * term (n) uint8 (the reference's terminal dtype).  fp32 here == the reference's float64 storage
 * followed by np_to_pytorch_batch's float32 cast.  The _f64 form takes the reference's native
 * float64 arrays and rounds to fp32 on the way in. */
int sac_buffer_add(sac_buffer_t *buf, int64_t n, const float *obs, const float *act, const float *rew,
                   const float *next_obs, const uint8_t *term);
int sac_buffer_add_f64(sac_buffer_t *buf, int64_t n, const double *obs, const double *act, const double *rew,
                       const double *next_obs, const uint8_t *term);
/* The inserts are ASYNCHRONOUS (ingest overlapping env stepping; the reference inserts 2 500
 * rows per epoch between rollouts and training, /root/reference/util/rlkit_custom.py:223-231): rows are packed into
 * one of two pinned staging buffers and handed to the copy engine on the buffer's stream; the call returns once the
 * copies are enqueued, the caller's arrays are free for reuse, and size/top already count the rows.  Sampling,
 * gathering and sac_buffer_read are ordered behind the inserts on that stream, so nobody has to wait explicitly;
 * sac_buffer_ingest_pending polls (1 = rows still in flight), sac_buffer_ingest_wait blocks until they have landed. */
int sac_buffer_ingest_pending(sac_buffer_t *buf);
int sac_buffer_ingest_wait(sac_buffer_t *buf);
int64_t sac_buffer_size(const sac_buffer_t *buf);      /* 'replay_buffer/size' */
int64_t sac_buffer_top(const sac_buffer_t *buf);
int64_t sac_buffer_capacity(const sac_buffer_t *buf);
/* Rows stored since the buffer was created: every row sac_buffer_add / sac_buffer_add_f64 hands to the ring (the
 * pinned async ingest), the head an oversized add skips included, so top == rows_written mod capacity as long as nobody
 * moves the cursor.  Never decreases; sac_buffer_set_cursor leaves it alone.  Incremental checkpoints compare it (and
 * top) with their values at the last save to find the rows written since. */
int64_t sac_buffer_rows_written(const sac_buffer_t *buf);

/* Checkpointing (SURVEY.md 8b "Snapshot contract": the reference saves no buffer -- rlkit's
 * get_snapshot() for it is {}, /root/reference/util/rlkit_custom.py:80 -- so a resumed run starts from an
 * empty one; here a run resumes exactly).  sac_buffer_read copies storage rows [start, start+n) to dense
 * host arrays in the sac_buffer_add layout; restore = sac_buffer_add of the saved rows in storage order,
 * then sac_buffer_set_cursor(top, size). */
int sac_buffer_read(sac_buffer_t *buf, int64_t start, int64_t n, float *obs, float *act, float *rew,
                    float *next_obs, uint8_t *term);
int sac_buffer_set_cursor(sac_buffer_t *buf, int64_t top, int64_t size);

/* The global NumPy legacy stream (np.random.seed at /root/reference/scripts/train.py:112) as the
 * replay buffer consumes it.  State layout = np.random.get_state(): key[624] + pos.  Round-tripping
 * the state keeps host NumPy consumers (env resets between training blocks) coherent. */
int sac_rng_seed(sac_buffer_t *buf, uint32_t seed);
int sac_rng_get_state(sac_buffer_t *buf, uint32_t key[624], int32_t *pos);
int sac_rng_set_state(sac_buffer_t *buf, const uint32_t key[624], int32_t pos);
/* Bind the generator to a HOST-resident MT19937 state: key[624] + *pos are the words of np.random's own state struct
 * (numpy.random.MT19937().ctypes.state_address: {uint32_t key[624]; int pos;}), so the buffer samples THE process-wide
 * stream the reference seeds at /root/reference/scripts/train.py:112 and rlkit's random_batch consumes -- by default,
 * with no per-call state transfer: every device draw is mirrored on those host words (a few ns per index), which are
 * therefore right when the call returns, and a change anybody else made to them (np.random.seed, np.random.set_state, a
 * host consumer such as an env reset) is noticed in front of the next draw and adopted.  The read-ahead of
 * sac_random_batch_device survives (the speculation is only dropped when the host words were changed from outside).
 * While bound, sac_rng_seed / sac_rng_set_state write through to the host words and sac_rng_get_state reads them.
 * key == NULL unbinds (the generator keeps its current state, privately).  The memory must outlive the binding. */
int sac_rng_bind_host(sac_buffer_t *buf, uint32_t *key, int32_t *pos);

/* np.random.randint(0, size, batch) drawn n_batches times on the device, bit-exact with NumPy
 * including rejected draws and the generator state afterwards.  idx_out (host, n_batches*batch
 * int64) may be NULL: indices then stay on the device for sac_gather_sampled / sac_train_loop. */
int sac_sample_indices(sac_buffer_t *buf, int batch, int64_t n_batches, int64_t *idx_out);

/* random_batch(batch): sample + gather + copy out.  Outputs are host arrays shaped like the
 * reference's dict entries after np_to_pytorch_batch: observations (B,O), actions (B,A),
 * rewards (B,1), terminals (B,1), next_observations (B,O), all fp32.  idx_out may be NULL. */
int sac_random_batch(sac_buffer_t *buf, int batch, float *obs, float *act, float *rew, float *term,
                     float *next_obs, int64_t *idx_out);
/* The stepwise interface without a PCIe round trip per step.  The reference's loop is
 *     train_data = replay_buffer.random_batch(bs); trainer.train(train_data)     (/root/reference/util/rlkit_custom.py:235-238)
 * where rlkit gathers on the host and copies the batch to the device inside train().  Here random_batch can leave
 * the batch where it is needed: sac_random_batch_device draws the next `batch` indices of the NumPy stream and
 * gathers them into a device slot, asynchronously, and returns a token (the batch number); sac_step_device
 * (below) runs trainer.train on it; sac_read_batch_device copies it to the host only if somebody looks at it.
 * A token stays valid until (at least) 16 more batches have been drawn (then the calls fail with "expired").
 * Read-ahead: called again and again with nothing in between that touches the generator or the buffer -- the loop above --
 * the call draws and gathers up to sixteen batches in its two launches and the following calls hand them out.  Every entry
 * point that reads or changes the generator's state, the buffer's rows or its size (add, seed / get / set state, the
 * other draws, sac_train_loop) first takes the speculation back: the generator's state saved in front of the chunk is
 * restored and advanced by the batches actually handed out.  The index stream is NumPy's, bit for bit, under any
 * interleaving (tests/test_gpu_device_batches.py).  SAC_READAHEAD=0 switches it off. */
int sac_random_batch_device(sac_buffer_t *buf, int batch, int64_t *token);
int sac_read_batch_device(sac_buffer_t *buf, int64_t token, float *obs, float *act, float *rew, float *term,
                          float *next_obs, int64_t *idx_out);

/* the gather half alone, for caller-supplied indices (parity tests, prioritised variants) */
int sac_gather(sac_buffer_t *buf, const int64_t *idx, int batch, float *obs, float *act, float *rew,
               float *term, float *next_obs);

/* Device-side batched form used for measurement: draws n_batches index vectors and gathers all
 * of them into contiguous minibatch slots in HBM in ONE gather launch; nothing is copied to the
 * host.  kernel_ms (may be NULL) receives {index kernel ms, gather kernel ms} from HIP events on
 * the handle's stream. */
int sac_sample_gather_device(sac_buffer_t *buf, int batch, int64_t n_batches, float kernel_ms[2]);
/* copy slot s of the last sac_sample_gather_device back to the host (tests) */
int sac_read_slot(sac_buffer_t *buf, int64_t slot, float *obs, float *act, float *rew, float *term,
                  float *next_obs, int64_t *idx_out);
/* The two row images of a minibatch slot (tests): per 16-row block the rows once more as the swizzled LDS row-block
 * [16][KLQ] the fused step starts from, KLQ = round_up(round_up(obs_dim, 16) + 16, 64); element (row, k) of a block at
 * row * KLQ + ((((k >> 2) ^ row) << 2) | (k & 3)).  img_sa holds [obs | 0 | act at round_up(obs_dim, 16) | 0], img_n
 * [next_obs | 0]; each receives round_up(batch, 16) * KLQ floats.  ring = 0: slot `which` of the last batched draw
 * (sac_read_slot's slots); ring = 1: the device batch with token `which` (sac_random_batch_device). */
int sac_read_slot_images(sac_buffer_t *buf, int ring, int64_t which, float *img_sa, float *img_n);

/* ------------------------------------------------------------------------------------------
 * SAC trainer.  Replaces rlkit SACTrainer (+ TorchTrainer.train, np_to_pytorch_batch,
 * ptu.soft_update_from_to) as constructed at /root/reference/util/rlkit_utils.py:98-106 with the
 * kwargs of /root/reference/scripts/train.py:29-37 and driven at
 * /root/reference/util/rlkit_custom.py:238 (train), :258 (get_diagnostics), :63/:70 (snapshot).
 * Networks: FlattenMlp x4 (rlkit_utils.py:64-83) and TanhGaussianPolicy (:92-96).
 * ------------------------------------------------------------------------------------------ */
typedef struct sac_config {
    int32_t obs_dim, act_dim;
    int32_t hidden;              /* both hidden layers; 256 in every shipped variant.json (see policy_hidden / qf_hidden) */
    int32_t batch;               /* algorithm_kwargs.batch_size: any positive size (slots are padded to whole 16-row
                                  * blocks; pad rows carry zero weight in every mean of the step) */
    float discount;              /* trainer_kwargs.discount */
    float reward_scale;          /* trainer_kwargs.reward_scale */
    float policy_lr, qf_lr;      /* trainer_kwargs.policy_lr / qf_lr (alpha uses policy_lr) */
    float soft_target_tau;       /* trainer_kwargs.soft_target_tau */
    int32_t target_update_period;
    int32_t use_automatic_entropy_tuning;
    float target_entropy;        /* NaN => -act_dim (rlkit default) */
    uint64_t noise_seed;         /* device counter-based N(0,1) stream for rsample */
    int32_t device;
    int32_t reserved;
    /* policy_kwargs / qf_kwargs hidden_sizes (/root/reference/util/arguments.py:98,104): two layers of at most 256 units
     * each, per network family; 0 = `hidden`.  Narrower layers run EXACTLY on the 256-wide kernels: the missing units are
     * zero rows / columns whose gradients, Adam updates and Polyak averages are identically zero. */
    int32_t policy_hidden[2];
    int32_t qf_hidden[2];
} sac_config_t;

enum { SAC_NET_POLICY = 0, SAC_NET_QF1 = 1, SAC_NET_QF2 = 2, SAC_NET_TARGET_QF1 = 3, SAC_NET_TARGET_QF2 = 4,
       SAC_NET_TARGET_POLICY = 5 /* TD3 handles only */ };

/* TD3.  Replaces rlkit TD3Trainer + TanhMlpPolicy x2 as assembled at
 * /root/reference/util/rlkit_utils.py:107-135 with the trainer kwargs of /root/reference/scripts/train.py:38-47
 * (defaults /root/reference/util/arguments.py:141-156).  The handle type, the replay buffer and every sac_*
 * accessor / step / loop entry point are shared with SAC: net id 5 is the target policy, both policies are
 * [fc0, fc1, last_fc] (tanh output), sac_step's eps2 is the N(0,1) draw of the target-policy smoothing noise
 * (eps1 unused), sac_set/get_scalars carry {policy Adam steps, 0, 0, critic Adam steps, n_train_steps_total, 0}.
 * Diagnostics vector: slots 0-15 as for SAC (QF1/QF2 Loss, Policy Loss = -mean Q1(s, pi(s)), Q1/Q2 Predictions,
 * Q Targets), 16-19 Bellman Errors 1, 20-23 Bellman Errors 2, 24-27 Policy Action (Mean Std Max Min).
 * Parity: unpinned (the reference ships no TD3 run); checked against oracle/td3_step_torch.py. */
typedef struct td3_config {
    int32_t obs_dim, act_dim;
    int32_t hidden;                          /* 256 */
    int32_t batch;
    float discount;                          /* train.py:41 fixes 0.99 */
    float reward_scale;
    float policy_learning_rate, qf_learning_rate;
    float tau;                               /* soft update of all three targets, on policy steps */
    float target_policy_noise;               /* sigma of the smoothing noise (default 0.2) */
    float target_policy_noise_clip;          /* rlkit default 0.5 */
    int32_t policy_and_target_update_period; /* default 2 */
    uint64_t noise_seed;
    int32_t device;
    int32_t reserved;
    int32_t policy_hidden[2];                /* as in sac_config_t */
    int32_t qf_hidden[2];
} td3_config_t;
int td3_trainer_create(sac_trainer_t **out, const td3_config_t *cfg);
/* as sac_trainer_create_mlp: hidden_sizes of any depth / width for TD3 (two layers of at most 256 units: the fused kernels) */
int td3_trainer_create_mlp(sac_trainer_t **out, const td3_config_t *cfg, const int32_t *policy_hidden, int32_t n_policy_hidden,
                           const int32_t *qf_hidden, int32_t n_qf_hidden);

/* diagnostics vector written per step; names = the 'trainer/...' columns of progress.csv
 * (/root/reference/runs/.../progress.csv:1) plus the optimised actor loss. */
enum {
    SAC_D_QF1_LOSS = 0, SAC_D_QF2_LOSS, SAC_D_POLICY_LOSS /* logged: mean(log_pi - q_new) */,
    SAC_D_ACTOR_LOSS /* optimised: mean(alpha*log_pi - q_new) */,
    SAC_D_Q1_MEAN, SAC_D_Q1_STD, SAC_D_Q1_MAX, SAC_D_Q1_MIN,
    SAC_D_Q2_MEAN, SAC_D_Q2_STD, SAC_D_Q2_MAX, SAC_D_Q2_MIN,
    SAC_D_QT_MEAN, SAC_D_QT_STD, SAC_D_QT_MAX, SAC_D_QT_MIN,
    SAC_D_LOGPI_MEAN, SAC_D_LOGPI_STD, SAC_D_LOGPI_MAX, SAC_D_LOGPI_MIN,
    SAC_D_MU_MEAN, SAC_D_MU_STD, SAC_D_MU_MAX, SAC_D_MU_MIN,
    SAC_D_LOGSTD_MEAN, SAC_D_LOGSTD_STD, SAC_D_LOGSTD_MAX, SAC_D_LOGSTD_MIN,
    SAC_D_ALPHA, SAC_D_ALPHA_LOSS,
    SAC_DIAG_N = 32
};

int sac_trainer_create(sac_trainer_t **out, const sac_config_t *cfg);
/* hidden_sizes of ANY depth (variant['policy_kwargs'|'qf_kwargs']['hidden_sizes'], /root/reference/util/arguments.py:98,104;
 * FlattenMlp / TanhGaussianPolicy take a list of any length: /root/reference/util/rlkit_utils.py:64-97): 1..7 hidden layers
 * of 1..4096 units per network family (cfg->hidden / policy_hidden / qf_hidden are ignored).  Two hidden layers of at most
 * 256 units -- every shipped variant.json -- run on the fused kernels exactly as with sac_trainer_create; every other shape
 * runs the GENERAL step: the same step in the same order as a sequence of 2 Lp + 2 Lq + 2 launches around one
 * matrix-product kernel (csrc/sac_general.h), results within fp32 round-off of the oracle like the fused kernels'
 * (tests/test_gpu_general_shapes.py); sac_trainer_step_kind reports 3.  Every sac_* entry point works on such a handle except
 * sac_profile_loop.  (TD3: td3_trainer_create_mlp.) */
int sac_trainer_create_mlp(sac_trainer_t **out, const sac_config_t *cfg, const int32_t *policy_hidden, int32_t n_policy_hidden,
                           const int32_t *qf_hidden, int32_t n_qf_hidden);
int sac_trainer_destroy(sac_trainer_t *t);

/* flat fp32 parameter vector of one net, nn.Linear layout (W (out,in) row-major, then b):
 *   Q nets : fc0.W fc0.b fc1.W fc1.b last_fc.W last_fc.b
 *   policy : fc0.W fc0.b fc1.W fc1.b last_fc.W last_fc.b last_fc_log_std.W last_fc_log_std.b */
/* The six getters and setters below return, or overwrite, the state AS OF THE LAST COMPLETED STEP -- the one the counters
 * in `scalars` name.  A trainer on the fused step may have up to 47 sac_step_device steps in flight that nobody has
 * verified; each of these entries first waits for them and, if a fused launch among them gave up, re-runs the lost
 * steps on the four-launch step (what sac_sync does), so a getter never returns parameters that lack steps the counters
 * count, and a setter's state is never stepped on by steps launched in front of it.  Those re-runs read the buffers'
 * slots: see sac_step_device for how long a buffer must live. */
int64_t sac_param_count(const sac_trainer_t *t, int net);
int sac_set_params(sac_trainer_t *t, int net, const float *flat, int64_t n);
int sac_get_params(sac_trainer_t *t, int net, float *flat, int64_t n);
/* Adam state of the three trained nets (same flat layout) + step count; the reference's snapshot
 * omits these (SURVEY.md section 5 "Checkpoint / resume"), true resume needs them. */
int sac_set_opt_state(sac_trainer_t *t, int net, const float *exp_avg, const float *exp_avg_sq, int64_t n);
int sac_get_opt_state(sac_trainer_t *t, int net, float *exp_avg, float *exp_avg_sq, int64_t n);
/* scalars[6] = {log_alpha, alpha_exp_avg, alpha_exp_avg_sq, adam_step_count, n_train_steps_total, alpha} */
int sac_set_scalars(sac_trainer_t *t, const double scalars[6]);
int sac_get_scalars(sac_trainer_t *t, double scalars[6]);

/* trainer.train(np_batch) == np_to_pytorch_batch + train_from_torch: ONE gradient step on a
 * caller-supplied batch (host fp32, shapes as sac_random_batch writes them).  eps1/eps2 (B,A) are
 * the N(0,1) draws of the two rsample() calls (policy on obs, then on next_obs); NULL => the
 * device counter-based stream.  diag (SAC_DIAG_N floats, may be NULL) receives this step's stats. */
int sac_step(sac_trainer_t *t, const float *obs, const float *act, const float *rew, const float *term,
             const float *next_obs, const float *eps1, const float *eps2, float *diag);

/* trainer.train(batch) on a device-resident batch (token of sac_random_batch_device on `buf`): four kernel
 * launches behind the gather, no host copy, no synchronisation -- unless diag != NULL, which copies the step's
 * diagnostics out (rlkit reads them on the first step of an epoch only).  Noise: the device stream.
 * Lifetime: with diag == NULL the trainer keeps (buf, token) on record until it has seen the step applied, and a later
 * call that settles it (sac_sync, a step with diag, sac_train_loop, sac_get_* / sac_set_*, sac_policy_mirror /
 * sac_policy_act, sac_trainer_set_xcd_mask) may re-run the step from buf's slot.  `buf` must therefore outlive a
 * sac_sync -- or a sac_trainer_destroy -- of every trainer that stepped on its device batches: sac_buffer_destroy does
 * not know of these records. */
int sac_step_device(sac_trainer_t *t, sac_buffer_t *buf, int64_t token, float diag[SAC_DIAG_N]);

/* The whole hot loop of rlkit_custom.py:234-238 on the device:
 *   for _ in range(n_steps): batch = buffer.random_batch(B); trainer.train(batch)
 * Indices for all n_steps are drawn first (same stream consumption as n_steps random_batch calls:
 * nothing else touches np.random or the buffer inside the loop), gathered into HBM slots, then the
 * steps run back to back with no host round trip.  diag_first / diag_last (may be NULL) receive the
 * diagnostics of the first and last step (the reference logs the first step of each epoch). */
/* Calls in a row: a call that directly follows another sac_train_loop on the same buffer (nothing in between that touches
 * the generator, the rows or the slots) leaves the NEXT call's first four batches drawn and gathered behind its own, under
 * its last steps, so that the next call's first step has no draw and no gather in front of it (~15 us of a call).  That
 * chunk is speculation: the generator's state as everybody sees it (sac_rng_get_state, np.random when bound) stays behind
 * the batches handed out, and any other entry point that comes first takes the speculation back.  Results and index
 * stream are those of calls that never speculate, bit for bit (tests/test_gpu_train_loop.py). */
int sac_train_loop(sac_trainer_t *t, sac_buffer_t *buf, int64_t n_steps, float *diag_first, float *diag_last);

/* 1 while the trainer runs the FUSED step: launches A + B + C of the step as one launch (k_abc) whose workgroups hand
 * their partial sums to each other inside the launch, then the weight-gradient / Adam launch -- two launches per step
 * instead of four.  It needs the chip to itself (every workgroup resident).  A hand-off that times out (50 ms) makes
 * the step apply NOTHING, the call that notices returns an error, and the trainer falls back to the four-launch step
 * for good; SAC_FUSED=0 in the environment selects the four-launch step from the start.  Both give identical results
 * (tests/test_gpu_fused_step.py). */
int sac_trainer_is_fused(const sac_trainer_t *t);
/* How a trainer's step is launched: 0 = four launches (k_fwd_a, k_fwd_b, k_bwd, k_dw_adam); 1 = the fused step above
 * (k_abc, k_dw_adam: batches up to 256 rows); 2 = three launches for batches whose 256-wide layers are not split over
 * workgroups (1024 rows and more): the two forward launches as ONE, k_chain8 -- a workgroup runs the policy, takes its own
 * head and goes on into the Q nets, no hand-off involved -- then k_bwd and k_dw_adam; 3 = the general step of
 * sac_trainer_create_mlp (network shapes beyond the fused kernels'); 4 = kind 2 with the backward blocks inside the chained
 * launch behind in-launch hand-offs (k_chain8<..., BWD>, then k_dw_adam: two launches; chosen when the launch's 4 x
 * row-blocks workgroups fill the CUs exactly -- batch 1024 on 256 CUs -- and the first layers are one k-chunk;
 * SAC_CHAIN_BWD=0/1 overrides).  Like kind 1 it can give up inside a launch; the trainer then re-runs that step as kind 2
 * and stays there (sac_trainer_step_kind reports 2 from then on), results unchanged.  (TD3: 0 or 1.) */
int sac_trainer_step_kind(const sac_trainer_t *t);

/* measurement helpers: HIP events on the trainer's stream around the last sac_train_loop (total_ms == steps_ms: first
 * launch to last step), and around the index draw (sample_ms) and the gather (gather_ms) of ONE of its chunks -- the
 * second chunk when the call has one (12 batches at the default plan), else the first. */
int sac_sync(sac_trainer_t *t);
int sac_last_loop_ms(sac_trainer_t *t, float *total_ms, float *sample_ms, float *gather_ms, float *steps_ms);

/* profiling pass: the same loop with HIP events (on the launching streams) around every kernel.
 * out_ms[9] = {index kernel, gather kernel, then the MEAN per-launch ms of k_fwd_a, k_fwd_b, k_bwd,
 * a reserved slot (0), k_dw_adam (fused step: k_abc in the k_fwd_a slot, 0 in the next two) (each minus the cost of an empty event pair), that empty-pair cost,
 * and the wall ms of all n_steps steps}.  n_steps <= 4096. */
int sac_profile_loop(sac_trainer_t *t, sac_buffer_t *buf, int64_t n_steps, float out_ms[9]);

/* Experiment hooks (bench.py --replicas-per-gpu R --xcd-replicas): confine a handle's launches to
 * the CUs of one XCD (0..7) through a CU-masked stream, so that eight independent runs -- the reference's real workload is
 * many independent jobs, /root/reference/launch_jobs.sh:15-24 -- can share one GPU without each launch spanning the chip.
 * A trainer confined this way takes the four-launch step (the fused step needs all its workgroups resident).
 * The _mask variants take a set of XCDs (bit k = XCD k): a trainer whose fused step fits the CUs it is given (batch 128
 * on four XCDs) KEEPS the fused step and is no longer serialised with the other trainers of the process -- the caller
 * promises that trainers confined this way own disjoint XCDs; mask 0xff undoes the confinement. */
int sac_buffer_set_xcd(sac_buffer_t *buf, int xcd);
int sac_trainer_set_xcd(sac_trainer_t *t, int xcd);
int sac_buffer_set_xcd_mask(sac_buffer_t *buf, unsigned xcd_mask);
/* (sac_trainer_set_xcd[_mask] settles the trainer first, like the state getters above: unverified fused steps are looked
 *  at, and re-run if lost, on the stream they were launched on, before that stream is replaced.) */
int sac_trainer_set_xcd_mask(sac_trainer_t *t, unsigned xcd_mask);

/* SURVEY.md 8d "Bounding roofline": the peaks the roofline fractions divide by, MEASURED on the box -- a float4
 * stream copy of 1 GiB (read + write GB/s) and a back-to-back v_mfma_f32_16x16x4_f32 loop on every SIMD (TFLOP/s).
 * out[4] = {copy GB/s, fp32 MFMA TFLOP/s, GB moved per copy pass, ms of the best MFMA pass}. */
int sac_measure_peaks(int device, float out[4]);

/* test access to intermediates of the last step: name in {"a_new","log_pi","mu","log_std","q1","q2",
 * "q_target","q1_new","q2_new","a_next","log_pi_next","g_policy","g_qf1","g_qf2","ext_img_sa","ext_img_n"} (g_* = flat
 * gradient in the sac_get_params layout; ext_img_*: the row images sac_step staged with its last batch, see
 * sac_read_slot_images).  And two read-only views of the trained state, which settle the trainer first like the state
 * getters: "pt_policy" / "pt_qf1" / "pt_qf2" -- sac_get_params' vector with the weights taken from the TRANSPOSED copy
 * the backward passes and Adam read (fused kernels' shapes only; equal to sac_get_params bit for bit by invariant) --
 * and "pad_nonzero" -- counts of elements x with !(x == 0) at the padding positions no flat index reaches: for each
 * trained net 0..2 the counts of P, PT, MT, VT (general step: P, M, V), then of P for each target net (all 0 by
 * invariant).  Returns the element count, <0 on error. */
int64_t sac_debug_fetch(sac_trainer_t *t, const char *name, float *out, int64_t cap);
/* Test hook: put a trainer that runs a fused step (kinds 1 and 4) at launch number `seq`.  A fused launch carries the
 * number of fused launches of its trainer so far (a 32-bit count that wraps), and the workgroups of a launch wait for
 * hand-off counters to reach fixed multiples of it modulo 2^32 ("The hand-off protocol").  The call settles
 * the trainer like the state getters and then leaves it exactly as `seq` completed launches would: the launch number,
 * every counter at its units x seq modulo 2^32, every tagged word tagged seq, the give-up word clear.  Parameters,
 * optimizer state and step counts are untouched -- results do not depend on the launch number, which is what
 * tests/test_gpu_launch_numbers.py checks around every power of two the multiples cross.  SAC_FUSED_TEST_STALL=n counts
 * from the number set here: it stalls launch seq + n.  A trainer on any other step is refused (-1, sac_last_error). */
int sac_debug_set_launch_number(sac_trainer_t *t, uint32_t seq);

/* policy.get_action(obs) on the HOST with weights mirrored from the device (acting path,
 * /root/reference/util/rlkit_custom.py:437; MakeDeterministic => tanh(mean)).
 * eps (A floats) may be NULL when deterministic.  The mirror is a state read: it holds the policy as of the last completed
 * step (see sac_get_params), and sac_policy_act takes a new one on its first call behind any step. */
int sac_policy_mirror(sac_trainer_t *t);
int sac_policy_act(sac_trainer_t *t, const float *obs, int deterministic, const float *eps, float *act);
/* policy.get_actions(obs) on the DEVICE from the live weights: n rows in one launch (k_act, csrc/sac_act.h).  The kernel
 * reads the policy where the step kernels keep it -- no mirror, no parameter copy -- and sees the weights as of the last
 * completed step of any step path (sac_step, sac_step_device, sac_train_loop, sac_group_train_loop) or sac_set_params:
 * the call first drains the trainer as sac_sync does, a fused step that gave up included.  n is 1..1024; SAC stochastic:
 * tanh(mean + exp(clamp(log_std, -20, 2)) * eps), deterministic: tanh(mean); TD3: tanh(last_fc) always (eps unused).  A
 * row's action depends on that row's observation, its eps and the weights only -- not on its place, on n or on the rest
 * of the launch -- so row r of any call is bit for bit the one-row call.  The call returns with the actions in `act`;
 * the host mirror of sac_policy_act is left alone, and nothing the step reads is written.
 * For trainers with the fused kernels' shapes (two hidden layers of at most 256 units: every shipped variant).
 * General-step trainers (sac_trainer_create_mlp with other shapes) are refused: they act through sac_policy_act. */
int sac_policy_act_device(sac_trainer_t *t, int64_t n, const float *obs /* (n,O) host */, int deterministic,
                          const float *eps /* (n,A) host; NULL when deterministic or TD3 */, float *act /* (n,A) host */);
/* the same for 1..SAC_GROUP_MAX (16) trainers of one device in ONE launch; n_rows[i] == 0: member i sits out (its
 * arrays are not touched).  It takes trainers, not a group, so it serves every group kind; SAC and TD3 members, dims,
 * row counts and deterministic flags may be mixed.  Each member's actions are bit for bit its own
 * sac_policy_act_device's.  Refused (<0, sac_last_error, nothing changed): null or duplicate trainers, n_rows outside
 * 0..1024 or all zero, a stochastic SAC member without eps, trainers on different devices, general-step trainers,
 * members confined by sac_trainer_set_xcd[_mask]. */
int sac_policy_act_many(sac_trainer_t *const *trainers, int n_trainers, const int32_t *n_rows,
                        const float *const *obs, const int32_t *deterministic, const float *const *eps,
                        float *const *act);
/* The same two entries for GENERAL-STEP trainers (sac_trainer_create_mlp / td3_trainer_create_mlp with hidden sizes
 * beyond two layers of at most 256 units: depth 1..7, widths 1..4096): k_act_layer (csrc/sac_act_general.h), one launch
 * per layer depth on the live weights of the general step -- no mirror, no repacking, no second copy of the weights --
 * and one wait at the end.  The contract is that of sac_policy_act_device / sac_policy_act_many: 1..16 trainers of one
 * device, SAC and TD3 mixed, 0..1024 rows each (0 = sits out, at least one with rows), eps only for stochastic SAC,
 * every member with rows drained as by sac_sync first, each member's actions bit for bit its own
 * sac_policy_act_general's and row r of any call bit for bit the one-row call.  The host mirror of sac_policy_act is
 * left alone; the kernel writes the trainers' own activation scratch and `act`, nothing the step reads.  Refused (<0,
 * sac_last_error, nothing changed): what sac_policy_act_many refuses, and trainers with the fused kernels' shapes
 * (sac_policy_act_device is their entry).  The three entries above keep refusing general-step trainers. */
int sac_policy_act_general(sac_trainer_t *t, int64_t n, const float *obs /* (n,O) host */, int deterministic,
                           const float *eps /* (n,A) host; NULL when deterministic or TD3 */, float *act /* (n,A) host */);
int sac_policy_act_general_many(sac_trainer_t *const *trainers, int n_trainers, const int32_t *n_rows,
                                const float *const *obs, const int32_t *deterministic, const float *const *eps,
                                float *const *act);

/* Q_net(obs, act) on the DEVICE from the live weights: n rows of any non-empty subset of the four Q networks in one
 * launch (k_qval, csrc/sac_qval.h).  `nets` is a mask of SAC_Q_* bits (bit 1 << (SAC_NET_* - 1)); q receives one row of n
 * values per selected net, the selected nets in ascending SAC_NET_* order.  The kernel reads the nets where the step
 * kernels keep them -- no mirror, no parameter copy -- and sees the weights as of the last completed step of any step
 * path or sac_set_params: the call first drains the trainer as sac_sync does, a fused step that gave up included.  n is
 * 1..1024.  A row's value depends on that row's observation and action and the net's weights only -- not on its place,
 * on n, on the other nets selected or on the rest of the launch -- so row r of any call is bit for bit the one-row call.
 * Nothing the step reads is written.  SAC and TD3 handles with the fused kernels' shapes (two hidden layers of at most
 * 256 units); general-step trainers are refused: their Q values come from sac_get_params and a forward on the host, or
 * from sac_q_values_general below. */
enum { SAC_Q_QF1 = 1, SAC_Q_QF2 = 2, SAC_Q_TARGET_QF1 = 4, SAC_Q_TARGET_QF2 = 8 };
int sac_q_values(sac_trainer_t *t, int64_t n, const float *obs /* (n,O) host */, const float *act /* (n,A) host */,
                 uint32_t nets, float *q /* (popcount(nets), n) host */);
/* the same for 1..SAC_GROUP_MAX (16) trainers of one device in ONE launch; n_rows[i] == 0: member i sits out (its
 * arrays and its mask are not looked at).  SAC and TD3 members, dims, row counts and masks may be mixed.  Each member's
 * values are bit for bit its own sac_q_values'.  Refused (<0, sac_last_error, nothing changed): null or duplicate
 * trainers, trainers on different devices, general-step trainers, members confined by sac_trainer_set_xcd[_mask],
 * n_rows outside 0..1024 or all zero, and for a member with rows a mask that is 0 or has bits above 8, or a null array. */
int sac_q_values_many(sac_trainer_t *const *trainers, int n_trainers, const int32_t *n_rows,
                      const float *const *obs, const float *const *act, const uint32_t *nets, float *const *q);
/* The same two entries for GENERAL-STEP trainers (a policy or critics beyond two hidden layers of at most 256 units:
 * depth 1..7, widths 1..4096; a trainer whose critics alone have the fused shape is served here too): k_qval_layer
 * (csrc/sac_qval_general.h), one launch per layer depth on the live critic weights of the general step -- no mirror, no
 * repacking, no parameter copy -- and one wait at the end.  The contract is that of sac_q_values / sac_q_values_many:
 * SAC_Q_* masks, the selected nets in ascending order, q (popcount(nets), n), n 1..1024 for the solo call, 1..16
 * trainers of one device, SAC and TD3 handles, dims, depths, widths, row counts and masks mixed, n_rows[i] == 0 = sits
 * out (at least one with rows), every member with rows drained as by sac_sync first, each member's values bit for bit
 * its own sac_q_values_general's and row r of any call bit for bit the one-row call.  The kernel writes the trainers' own
 * activation scratch (shared with sac_policy_act_general: the calls never overlap) and q, nothing the step reads.
 * Refused (<0, sac_last_error, nothing changed): what sac_q_values_many refuses, and trainers with the fused kernels'
 * shapes (sac_q_values is their entry).  sac_q_values / sac_q_values_many keep refusing general-step trainers. */
int sac_q_values_general(sac_trainer_t *t, int64_t n, const float *obs /* (n,O) host */, const float *act /* (n,A) host */,
                         uint32_t nets, float *q /* (popcount(nets), n) host */);
int sac_q_values_general_many(sac_trainer_t *const *trainers, int n_trainers, const int32_t *n_rows,
                              const float *const *obs, const float *const *act, const uint32_t *nets, float *const *q);

/* The SAC objectives on HELD-OUT transitions, on the DEVICE from the live weights: the forward half of the step as an
 * evaluation (k_eval, csrc/sac_eval.h) -- n transitions (s, a, r, d, s') with their N(0,1) draws in one launch, three
 * independent chains per 16-row block:
 *   rows[SAC_EVAL_Q1 / Q2]                  Q1 / Q2(s, a)
 *   rows[SAC_EVAL_Q1_NEW / Q2_NEW]          Q1 / Q2(s, a_new), a_new = tanh(mean(s) + exp(clamp(log_std(s), -20, 2)) eps)
 *   rows[SAC_EVAL_LOG_PI]                   log pi(a_new | s)   (mu, log_std: the head's mean and clamped log_std)
 *   rows[SAC_EVAL_TQ1 / TQ2]                target_qf1 / target_qf2(s', a_next), a_next from s' and eps_next
 *   rows[SAC_EVAL_LOG_PI_NEXT]              log pi(a_next | s')
 *   rows[SAC_EVAL_Y]                        reward_scale r + (1 - d) discount (min(tq1, tq2) - alpha log_pi_next), each
 *                                           operation rounded to float32 on its own, in this order
 * alpha is the trainer's CURRENT entropy coefficient -- sac_get_scalars' scalars[5], 1 with automatic tuning off, exp(log_alpha) for a trainer that
 * has neither stepped nor been given scalars, whose scalars[5] still reads 0 -- read behind the drain and returned in io->alpha: the objective at the current parameters.  (The training step logs Alpha,
 * Q Targets and its losses behind its own alpha update, one alpha step further on.)  The Q columns are bit for bit
 * sac_q_values' on the same rows and a_new / a_next bit for bit sac_policy_act_device's; row r of any call is bit for
 * bit the one-row call.  The call drains the trainer as sac_sync does, reads the nets where the step keeps them and
 * writes nothing the step reads: parameters, optimizer state, scalars, the step's noise counter and the buffer
 * generator stay untouched.  n is 1..1024.  SAC trainers with the fused kernels' shapes; general-step trainers are
 * refused (sac_get_params and a forward on the host is their path, or sac_evaluate_general below) and so are TD3
 * trainers (this is the SAC objective). */
enum { SAC_EVAL_Q1, SAC_EVAL_Q2, SAC_EVAL_Q1_NEW, SAC_EVAL_Q2_NEW, SAC_EVAL_TQ1, SAC_EVAL_TQ2,
       SAC_EVAL_LOG_PI, SAC_EVAL_LOG_PI_NEXT, SAC_EVAL_Y, SAC_EVAL_ROWS_N };
typedef struct {
    const float *obs, *act, *rew, *term, *next_obs;   /* (n,O) (n,A) (n) (n) (n,O), host */
    const float *eps, *eps_next;                      /* (n,A) N(0,1) draws, host */
    float *rows;                                      /* (SAC_EVAL_ROWS_N, n) */
    float *mu, *log_std, *a_new, *a_next;             /* (n,A) each; any may be NULL */
    float alpha;                                      /* out: the entropy coefficient used */
} sac_eval_io_t;
int sac_evaluate(sac_trainer_t *t, int64_t n, sac_eval_io_t *io);                 /* n in 1..1024 */
/* the same for 1..SAC_GROUP_MAX (16) trainers of one device in ONE launch, io[i] for trainer i; n_rows[i] == 0: member i
 * sits out (its io is not looked at).  Dims, hidden sizes and row counts may be mixed; each member's columns are bit for
 * bit its own sac_evaluate's.  Refused (<0, sac_last_error, nothing changed): null or duplicate trainers, trainers on
 * different devices, TD3 trainers, general-step trainers, members confined by sac_trainer_set_xcd[_mask], n_rows outside
 * 0..1024 or all zero, and for a member with rows a null input array or null rows. */
int sac_evaluate_many(sac_trainer_t *const *trainers, int n_trainers, const int32_t *n_rows, sac_eval_io_t *io);
/* The same two entries for GENERAL-STEP SAC trainers (a policy or critics beyond two hidden layers of at most 256 units:
 * depth 1..7, widths 1..4096): k_eval_layer (csrc/sac_eval_general.h), one launch per layer depth on the live weights of
 * the general step -- the policy's layers on s and s', then the critics' layers on [s | a], [s | a_new] and
 * [s' | a_next], then y -- on the first trainer's stream with one wait at the end; no mirror, no repacking, no parameter
 * copy.  The contract is that of sac_evaluate / sac_evaluate_many: the same sac_eval_io_t, the same nine rows, the same
 * optional arrays, io->alpha read the same way, n 1..1024 for the solo call, 1..16 trainers of one device with dims,
 * depths, widths and row counts mixed, n_rows[i] == 0 = sits out (at least one with rows), every member with rows
 * drained as by sac_sync first.  The six Q columns are bit for bit sac_q_values_general's on the same rows, a_new / a_next
 * bit for bit sac_policy_act_general's, y its float32 restatement; each member's columns are bit for bit its own
 * sac_evaluate_general's and row r of any call bit for bit the one-row call.  The kernels write the trainers' own
 * activation scratch (shared with sac_policy_act_general and sac_q_values_general: the calls never overlap) and the
 * outputs, nothing the step reads.  Refused (<0, sac_last_error, nothing changed, no output written): what
 * sac_evaluate_many refuses (general-step trainers apart), and trainers with the fused kernels' shapes (sac_evaluate is their entry).  sac_evaluate /
 * sac_evaluate_many keep refusing general-step trainers. */
int sac_evaluate_general(sac_trainer_t *t, int64_t n, sac_eval_io_t *io);         /* n in 1..1024 */
int sac_evaluate_general_many(sac_trainer_t *const *trainers, int n_trainers, const int32_t *n_rows, sac_eval_io_t *io);
/* The STATISTICS of such an evaluation reduced on the device as well (k_eval_moments, csrc/sac_eval_moments.h): one more
 * launch behind the evaluation's kernels and in front of the call's single wait reads the float32 columns where they
 * lie and leaves nine moment records per member, every element formed in float64:
 *   SAC_EVAL_M_Q1 / Q2 / Y / LOG_PI     the rows q1, q2, y, log_pi                                  (n elements)
 *   SAC_EVAL_M_MU / LOG_STD             the head's mean and clamped log_std                         (n A elements)
 *   SAC_EVAL_M_TD1 / TD2                (double)q1 - (double)y, (double)q2 - (double)y              (n)
 *   SAC_EVAL_M_POLICY                   (double)log_pi - min((double)q1_new, (double)q2_new)        (n)
 * A record: count; sum = sum of x; sumsq = sum of x^2; m2 = sum of (x - sum / count)^2 in a second pass over the same
 * elements (np.std's form: 0 for a constant column); max and min, which keep a NaN as np.max / np.min do.  The order of
 * every sum is a function of the record's own element count only -- never of the other members of the call, of a
 * member's place among them or of the optional arrays asked for: a member's records are byte for byte those of its
 * solo call.  alpha is io->alpha; log_alpha what sac_get_scalars' scalars[0] would return at this moment, from the same
 * read.  The contract is that of sac_evaluate_many / sac_evaluate_general_many (admission, refusals, the drain, 0..1024
 * rows, 1..16 trainers, each family refusing the other's trainers) with two differences: io[i].rows may be NULL -- then no
 * column is copied back -- and stats[i] is filled for every member with rows.  Null stats: refused.  The columns are
 * bit for bit those of the entries above. */
enum { SAC_EVAL_M_Q1, SAC_EVAL_M_Q2, SAC_EVAL_M_Y, SAC_EVAL_M_LOG_PI, SAC_EVAL_M_MU, SAC_EVAL_M_LOG_STD,
       SAC_EVAL_M_TD1, SAC_EVAL_M_TD2, SAC_EVAL_M_POLICY, SAC_EVAL_MOMENTS_N };
typedef struct { double count, sum, m2, sumsq, max, min; } sac_eval_moment_t;
typedef struct { sac_eval_moment_t m[SAC_EVAL_MOMENTS_N]; double alpha, log_alpha; } sac_eval_stats_t;
int sac_evaluate_stats_many(sac_trainer_t *const *trainers, int n_trainers, const int32_t *n_rows, sac_eval_io_t *io,
                            sac_eval_stats_t *stats);
int sac_evaluate_general_stats_many(sac_trainer_t *const *trainers, int n_trainers, const int32_t *n_rows, sac_eval_io_t *io,
                                    sac_eval_stats_t *stats);
/* The same evaluations on REPLAY rows IN PLACE: the five input arrays of member i are storage rows src[i].idx[0 .. n_rows[i])
 * of the replay buffer src[i].buf, copied on the device (k_eval_rows, csrc/sac_eval_rows.h: one launch in front of the
 * evaluation's kernels) from the replay storage into the staging the evaluation reads (mapped pinned host memory, as
 * for the entries above) -- no synchronised gather to the host, no host conversion and no memcpy into the staging.  io[i].obs / act / rew / term / next_obs are ignored and may be NULL; eps and eps_next still come from the
 * host.  stats NULL: the contract of sac_evaluate_many / sac_evaluate_general_many (io[i].rows needed); with stats that of
 * the *_stats_many entries (rows may be NULL).  The columns and the moment records are bit for bit those of the same
 * entry on the rows sac_gather returns for the same indices.  A storage row is an index into [0, sac_buffer_size): the
 * rows as they lie, not in insertion order.  Two members may name one buffer.  The rows are read behind every insert
 * pending on the buffer's stream (an event, no host wait), and the buffer is only read: its generator, bound host words,
 * read-ahead and loop speculation stay as they are.  Refused in addition (<0, sac_last_error, nothing launched, no
 * output written), each naming the member: a null buf or idx, a buffer on another device, buffer dims other than the
 * trainer's, an empty buffer, an index outside [0, sac_buffer_size). */
typedef struct { sac_buffer_t *buf; const int64_t *idx; } sac_eval_src_t;   /* idx: n_rows[i] storage rows, host */
int sac_evaluate_replay_many(sac_trainer_t *const *trainers, int n_trainers, const int32_t *n_rows,
                             const sac_eval_src_t *src, sac_eval_io_t *io, sac_eval_stats_t *stats /* may be NULL */);
int sac_evaluate_replay_general_many(sac_trainer_t *const *trainers, int n_trainers, const int32_t *n_rows,
                                     const sac_eval_src_t *src, sac_eval_io_t *io, sac_eval_stats_t *stats /* may be NULL */);

/* The TD3 objectives on HELD-OUT transitions, on the DEVICE from the live weights: the forward half of the TD3 step as an
 * evaluation (k_eval_td3, csrc/td3_eval.h) -- n transitions (s, a, r, d, s') with their N(0,1) smoothing draw in one
 * launch, three independent chains per 16-row block:
 *   rows[TD3_EVAL_Q1 / Q2]      Q1 / Q2(s, a)
 *   rows[TD3_EVAL_Q_PI]         Q1(s, a_pi), a_pi = tanh(last_fc(s)) of the policy (the policy loss is -mean of it)
 *   rows[TD3_EVAL_TQ1 / TQ2]    target_qf1 / target_qf2(s', a_smooth), a_target = tanh(last_fc(s')) of the TARGET policy,
 *                               a_smooth = a_target + clamp(eps * target_policy_noise, -noise_clip, +noise_clip): the
 *                               step's expression, the sum is not clipped again; a NaN draw stays a NaN
 *   rows[TD3_EVAL_Y]            reward_scale r + ((1 - d) discount) min(tq1, tq2), each operation rounded to float32 on
 *                               its own, in this order (fminf for the minimum)
 * target_policy_noise and noise_clip are the trainer's td3_config_t values.  The Q columns are bit for bit sac_q_values'
 * on the same rows and a_pi bit for bit sac_policy_act_device's; row r of any call is bit for bit the one-row call.  The
 * call drains the trainer as sac_sync does, reads the six nets where the step keeps them and writes nothing the step
 * reads: parameters, optimizer state, scalars, the step's noise counter and the buffer generator stay untouched.  n is
 * 1..1024.  TD3 trainers with the fused kernels' shapes; SAC trainers are refused (sac_evaluate is their entry) and so
 * are general-step TD3 trainers (sac_get_params and a forward on the host is their path). */
enum { TD3_EVAL_Q1, TD3_EVAL_Q2, TD3_EVAL_Q_PI, TD3_EVAL_TQ1, TD3_EVAL_TQ2, TD3_EVAL_Y, TD3_EVAL_ROWS_N };
typedef struct {
    const float *obs, *act, *rew, *term, *next_obs;   /* (n,O) (n,A) (n) (n) (n,O), host */
    const float *eps;                                 /* (n,A) N(0,1): the smoothing draw, host */
    float *rows;                                      /* (TD3_EVAL_ROWS_N, n) */
    float *a_pi, *a_target, *a_smooth;                /* (n,A) each; any may be NULL */
} td3_eval_io_t;
int td3_evaluate(sac_trainer_t *t, int64_t n, td3_eval_io_t *io);                 /* n in 1..1024 */
/* the same for 1..SAC_GROUP_MAX (16) TD3 trainers of one device in ONE launch, io[i] for trainer i; n_rows[i] == 0: member
 * i sits out (its io is not looked at).  Dims, hidden sizes and row counts may be mixed; each member's columns are bit
 * for bit its own td3_evaluate's.  Refused (<0, sac_last_error, nothing changed, no output written): null or duplicate
 * trainers, more than 16, trainers on different devices, SAC trainers, general-step trainers, members confined by
 * sac_trainer_set_xcd[_mask], n_rows outside 0..1024 or all zero, and for a member with rows a null input array or null
 * rows. */
int td3_evaluate_many(sac_trainer_t *const *trainers, int n_trainers, const int32_t *n_rows, td3_eval_io_t *io);
/* The same two entries for GENERAL-STEP TD3 trainers (a policy or critics beyond two hidden layers of at most 256 units:
 * depth 1..7, widths 1..4096): k_eval_layer_td3 (csrc/td3_eval_general.h) and k_eval_layer, one launch per layer depth on
 * the live weights of the general step -- the policy's layers on s and the TARGET policy's on s', then the critics'
 * layers on [s | a], [s | a_pi] and [s' | a_smooth], then y -- on the first trainer's stream with one wait at the end; no
 * mirror, no repacking, no parameter copy.  The contract is that of td3_evaluate / td3_evaluate_many: the same
 * td3_eval_io_t, the same six rows, the same optional arrays, n 1..1024 for the solo call, 1..16 trainers of one device
 * with dims, depths, widths and row counts mixed, n_rows[i] == 0 = sits out (at least one with rows), every member with
 * rows drained as by sac_sync first.  The five Q columns are bit for bit sac_q_values_general's on the same rows, a_pi bit
 * for bit sac_policy_act_general's, a_smooth and y their float32 restatements; each member's columns are bit for bit its
 * own td3_evaluate_general's and row r of any call bit for bit the one-row call.  The kernels write the trainers' own
 * activation scratch (shared with sac_policy_act_general and sac_q_values_general: the calls never overlap) and the
 * outputs, nothing the step reads.  Refused (<0, sac_last_error, nothing changed, no output written): what
 * td3_evaluate_many refuses (general-step trainers apart), and trainers with the fused kernels' shapes (td3_evaluate is
 * their entry).  td3_evaluate / td3_evaluate_many keep refusing general-step trainers. */
int td3_evaluate_general(sac_trainer_t *t, int64_t n, td3_eval_io_t *io);         /* n in 1..1024 */
int td3_evaluate_general_many(sac_trainer_t *const *trainers, int n_trainers, const int32_t *n_rows, td3_eval_io_t *io);
/* The STATISTICS of a TD3 evaluation reduced on the device as well (k_eval_moments_td3, csrc/td3_eval_moments.h): one more
 * launch behind k_eval_td3 (fused shapes) or k_eval_y_td3 (general step) and in front of the call's single wait reads the
 * float32 columns where they lie and leaves nine moment records (sac_eval_moment_t, above) per member, every element
 * formed in float64:
 *   TD3_EVAL_M_Q1 / Q2 / Y / Q_PI       the rows q1, q2, y, q_pi                                    (n elements)
 *   TD3_EVAL_M_A_PI                     the policy's action                                         (n A elements)
 *   TD3_EVAL_M_TD1 / TD2                (double)q1 - (double)y, (double)q2 - (double)y              (n)
 *   TD3_EVAL_M_BELLMAN1 / BELLMAN2      d * d with d as above, the product rounded on its own       (n)
 * The reduction is k_eval_moments': the order of every sum is a function of the record's own element count only, so a
 * member's records are byte for byte those of its solo call, whatever its neighbours, its place among them or the
 * optional arrays asked for.  The contract is that of td3_evaluate_many / td3_evaluate_general_many (admission,
 * refusals, the drain, 0..1024 rows, 1..16 trainers, SAC trainers refused, each family refusing the other's trainers)
 * with two differences: io[i].rows may be NULL -- then no column is copied back -- and stats[i] is filled for every
 * member with rows.  Null stats: refused.  The columns are bit for bit those of the entries above. */
enum { TD3_EVAL_M_Q1, TD3_EVAL_M_Q2, TD3_EVAL_M_Y, TD3_EVAL_M_Q_PI, TD3_EVAL_M_A_PI,
       TD3_EVAL_M_TD1, TD3_EVAL_M_TD2, TD3_EVAL_M_BELLMAN1, TD3_EVAL_M_BELLMAN2, TD3_EVAL_MOMENTS_N };
typedef struct { sac_eval_moment_t m[TD3_EVAL_MOMENTS_N]; } td3_eval_stats_t;
int td3_evaluate_stats_many(sac_trainer_t *const *trainers, int n_trainers, const int32_t *n_rows, td3_eval_io_t *io,
                            td3_eval_stats_t *stats);
int td3_evaluate_general_stats_many(sac_trainer_t *const *trainers, int n_trainers, const int32_t *n_rows, td3_eval_io_t *io,
                                    td3_eval_stats_t *stats);
/* The same TD3 evaluations on REPLAY rows IN PLACE, as sac_evaluate_replay_many / sac_evaluate_replay_general_many above:
 * the five input arrays of member i are storage rows src[i].idx[0 .. n_rows[i]) of the replay buffer src[i].buf, copied
 * on the device (k_eval_rows, unchanged, one launch in front of k_eval_td3 or the first k_eval_layer_td3) into the staging
 * the evaluation reads.  io[i].obs / act / rew / term / next_obs are ignored and may be NULL; eps still comes from the
 * host.  stats NULL: the contract of td3_evaluate_many / td3_evaluate_general_many (io[i].rows needed); with stats that of
 * the *_stats_many entries (rows may be NULL).  The columns and the moment records are bit for bit those of the same entry
 * on the rows sac_gather returns for the same indices.  Two members may name one buffer.  The rows are read behind every
 * insert pending on the buffer's stream (an event, no host wait), and the buffer is only read.  Refused in addition (<0,
 * sac_last_error, nothing launched, no output written), each naming the member: a null buf or idx, a buffer on another
 * device, buffer dims other than the trainer's, an empty buffer, an index outside [0, sac_buffer_size). */
int td3_evaluate_replay_many(sac_trainer_t *const *trainers, int n_trainers, const int32_t *n_rows,
                             const sac_eval_src_t *src, td3_eval_io_t *io, td3_eval_stats_t *stats /* may be NULL */);
int td3_evaluate_replay_general_many(sac_trainer_t *const *trainers, int n_trainers, const int32_t *n_rows,
                                     const sac_eval_src_t *src, td3_eval_io_t *io, td3_eval_stats_t *stats /* may be NULL */);

/* PER-UNIT statistics of the hidden layers, on the device from the live weights: how much of each network is alive
 * (dormant units, Sokar et al. 2023; dead units; the feature norm).  For n (obs, act) rows, each selected net and each of
 * its hidden layers l of N_l true units, the post-ReLU activations h[r][u] (float32, as the inference kernels produce
 * them) are reduced per unit into a record of SAC_UNIT_FIELDS_N arrays of N_l float64 (k_unit_moments,
 * csrc/sac_units.h):
 *   SAC_UNIT_SUM      sum over rows of (double)h
 *   SAC_UNIT_SUMSQ    sum over rows of (double)h (double)h
 *   SAC_UNIT_ACTIVE   the number of rows with h > 0 (a NaN is not active)
 *   SAC_UNIT_MAX      the largest h; a NaN stays
 * The order of every sum is a function of n alone (rows w, w + 4, ... for w = 0..3, then (p0 + p1) + (p2 + p3)), no
 * atomics: a member's records are byte for byte those of its solo call, whatever else is selected or asked for.
 * `nets`: bit k selects net SAC_NET_* == k (bit 5, the target policy: TD3 handles only).  The policy's layers see obs,
 * the Q nets' cat(obs, act); output layers and heads are not computed.  SAC and TD3 trainers are served.
 * sac_unit_moments[_many] serve the fused kernels' shapes (k_units, csrc/sac_units.h): ONE launch for up to 16 members,
 * 6 nets and 1024 rows each -- one workgroup per (member, selected net, 16-row block) runs the two hidden layers exactly
 * as k_act / k_qval do and stores rows < n and columns < the true widths (pad units of hidden sizes below 256 are not
 * units: a (64, 32) net has records of 64 and 32 entries) -- and one k_unit_moments launch behind it.
 * sac_unit_moments_general[_many] serve general-step trainers (csrc/sac_units_general.h): per layer depth one
 * k_qval_layer launch over every (member, selected net) that has a hidden layer there and one k_unit_moments launch on
 * its outputs; with `activations` the layers' outputs are written straight into the staging the caller's copy is made
 * from.  Either way everything runs on the first member's stream with one wait at the end.  Admission, the drain
 * (sac_sync semantics: the weights as of the last completed step), 0..1024 rows per member (0 = sits out) and 1..16
 * trainers are those of sac_q_values_many / sac_q_values_general_many.  The entries write staging, activation scratch
 * and the caller's outputs only: nothing the step reads, no generator.  Refused (<0, sac_last_error, nothing changed):
 * what those entries refuse (each family the other's trainers, naming the right entry), a mask that selects no net or an
 * unknown bit, bit 5 on a SAC handle, a Q net selected with act == NULL, null obs or moments. */
enum { SAC_UNIT_SUM, SAC_UNIT_SUMSQ, SAC_UNIT_ACTIVE, SAC_UNIT_MAX, SAC_UNIT_FIELDS_N };
typedef struct sac_units_io {
    const float *obs;        /* (n, O) host */
    const float *act;        /* (n, A) host; may be NULL when no Q net is selected */
    uint32_t nets, reserved;
    double *moments;         /* out: per selected net in ascending id, per hidden layer l: SAC_UNIT_FIELDS_N arrays of N_l */
    float *activations;      /* out, may be NULL: per selected net, per hidden layer l: (n, N_l) row-major */
} sac_units_io_t;
int sac_unit_moments(sac_trainer_t *t, int64_t n, sac_units_io_t *io);                             /* n in 1..1024 */
int sac_unit_moments_many(sac_trainer_t *const *trainers, int n_trainers, const int32_t *n_rows, sac_units_io_t *io);
int sac_unit_moments_general(sac_trainer_t *t, int64_t n, sac_units_io_t *io);                     /* n in 1..1024 */
int sac_unit_moments_general_many(sac_trainer_t *const *trainers, int n_trainers, const int32_t *n_rows, sac_units_io_t *io);

/* PER-TENSOR statistics of the state the step kernels write -- parameters, Adam moments, Polyak targets -- reduced on
 * the device where that state lives (k_param_moments / k_param_finish, csrc/sac_params.h): weight norms, the size of
 * Adam's moments, non-finite weights, how far a target lags its online net, without copying a parameter to the host.
 * A tensor is one tensor of the flat nn.Linear layout of sac_get_params: fc<i>.weight, fc<i>.bias, ..., last_fc.weight,
 * last_fc.bias and, on a SAC policy, last_fc_log_std.weight, last_fc_log_std.bias.  sac_param_tensors returns net's
 * tensor count (at most 18) and, where sizes is not NULL, their element counts E; <0 for a bad argument.
 * Per tensor a record of SAC_PARAM_FIELDS_N float64, formed in float64 from the float32 words with add, multiply,
 * compare and fabs only:
 *   SAC_PARAM_SUM, SAC_PARAM_SUMSQ          sum x, sum x x over the parameters
 *   SAC_PARAM_ABSMAX                        the largest |x|; a NaN stays
 *   SAC_PARAM_NONFINITE                     the number of elements that are not finite
 *   SAC_PARAM_M_SUMSQ, SAC_PARAM_M_ABSMAX   the same over Adam's first moment (the words sac_get_opt_state returns)
 *   SAC_PARAM_V_SUM, SAC_PARAM_V_MAX        the sum and the largest value of Adam's second moment
 *   SAC_PARAM_GAP_SUMSQ                     sum (x - x_target)^2, the difference in float64: qf1 against target_qf1, qf2
 *                                           against target_qf2, on TD3 handles the policy against the target policy
 * A field that does not apply is exactly 0.0: the Adam fields of target nets or without SAC_PARAMS_OPT, the gap of a SAC
 * policy and of target nets or without SAC_PARAMS_GAP.  The order of every sum is a function of the tensor's element
 * count E alone -- chunks of 16384 elements, lane l of 256 adds e = l, l + 256, ... ascending from 0.0, the lanes meet by
 * halving (128, 64, ..., 1), the chunks are joined in ascending order -- no atomics: a tensor's record is byte for byte
 * the same grouped or solo, under any mask and any flags, and infer.param_moments_reference restates it in NumPy.
 * Both families (the fused kernels' shapes and the general step) and both algorithms are served, mixed in one call: ONE
 * k_param_moments launch and one k_param_finish launch on the first member's stream, one wait.  Admission and the drain
 * are those of sac_q_values_many (1..16 trainers of one device, none confined by sac_trainer_set_xcd[_mask]; the state as
 * of the last completed step of any step path; unverified fused steps are settled first, as by the getters).  The call
 * writes staging and the caller's records: nothing the step reads, no generator.  Refused in addition (<0,
 * sac_last_error, nothing written): a mask that selects no net or an unknown bit, bit 5 (the target policy) on a SAC
 * handle, unknown flags, null moments. */
enum { SAC_PARAM_SUM, SAC_PARAM_SUMSQ, SAC_PARAM_ABSMAX, SAC_PARAM_NONFINITE, SAC_PARAM_M_SUMSQ, SAC_PARAM_M_ABSMAX,
       SAC_PARAM_V_SUM, SAC_PARAM_V_MAX, SAC_PARAM_GAP_SUMSQ, SAC_PARAM_FIELDS_N };
enum { SAC_PARAMS_OPT = 1, SAC_PARAMS_GAP = 2 };
typedef struct sac_params_io {
    uint32_t nets;      /* bit k selects SAC_NET_* == k */
    uint32_t flags;     /* SAC_PARAMS_OPT | SAC_PARAMS_GAP */
    double *moments;    /* out: for the selected nets ascending, their tensors in flat order, SAC_PARAM_FIELDS_N doubles each */
} sac_params_io_t;
int sac_param_tensors(const sac_trainer_t *t, int net, int64_t *sizes /* may be NULL */);
int sac_param_moments(sac_trainer_t *t, sac_params_io_t *io);
int sac_param_moments_many(sac_trainer_t *const *trainers, int n_trainers, sac_params_io_t *io);   /* up to SAC_GROUP_MAX */

/* RECYCLING hidden units on the device (ReDo, Sokar et al. 2023: the remedy that goes with the dormant / dead fractions of
 * sac_unit_moments): k_unit_recycle, csrc/sac_recycle.h.  For a listed unit u of hidden layer l (0-based) of a TRAINED net
 * (policy, qf1, qf2; on TD3 handles the online policy), in terms of the flat nn.Linear tensors of sac_get_params:
 *   incoming   fc<l>.weight[u, :] becomes the caller's fresh row and fc<l>.bias[u] the fresh bias
 *   outgoing   column u of the tensor(s) that read layer l becomes +0.0: fc<l+1>.weight[:, u]; for the last hidden layer
 *              last_fc.weight[:, u] and, on a SAC policy, last_fc_log_std.weight[:, u] too
 *   moments    with SAC_RECYCLE_OPT, Adam's m and v of every element written above become +0.0; step counts and bias
 *              corrections are untouched
 *   crossing   where an element is both incoming and outgoing -- (v, u) of fc<l+1>.weight with v listed in layer l + 1
 *              and u listed in layer l -- zero wins
 * Nothing else changes: target nets are left alone (the paper resets the online net; the Polyak average carries the
 * change over, and sac_param_moments' gap jumps for a while), pads stay +0.0, scalars, counters, generators and buffers
 * stay bit for bit.  Both weight copies of the fused kernels' shapes and the moments where they live are written through
 * the parameter map (csrc/sac_param_map.h, sac_recycle_map.h): what sac_get_params / sac_get_opt_state return afterwards
 * is infer.recycle_reference of what they returned before, byte for byte.
 * Both families and both algorithms are served, mixed in one call: two k_unit_recycle launches (incoming, then outgoing)
 * on the first member's stream, one wait before return.  Admission is sac_param_moments_many's (1..16 trainers of one
 * device, none confined by sac_trainer_set_xcd[_mask], none twice); every member is settled first (unverified fused steps,
 * as by the setters) and its acting mirror invalidated.  A call in which every list is empty returns 0 and launches
 * nothing.  Refused (<0, sac_last_error, nothing written): a mask that selects no net, bits 3..5 (target nets are not
 * recycled) or an unknown bit, unknown flags, null counts, null units or fresh with units listed, a unit outside the
 * layer's true width (the pads of a narrow fused layer are not units), a list that is not strictly ascending. */
enum { SAC_RECYCLE_OPT = 1 };
typedef struct sac_recycle_io {
    uint32_t nets;          /* bit k selects SAC_NET_* == k; only 0..2 */
    uint32_t flags;         /* SAC_RECYCLE_OPT */
    const int32_t *counts;  /* per selected net ascending, per hidden layer: units listed (0 allowed) */
    const int32_t *units;   /* the lists, concatenated in that order; strictly ascending, each in [0, true width N_l) */
    const float *fresh;     /* per listed unit in that order: K_l incoming weights (flat row order), then its bias */
} sac_recycle_io_t;
int sac_recycle_units(sac_trainer_t *t, const sac_recycle_io_t *io);
int sac_recycle_units_many(sac_trainer_t *const *trainers, int n_trainers, const sac_recycle_io_t *io);   /* up to SAC_GROUP_MAX */

/* RESET and SHRINK-AND-PERTURB of whole networks on the device (Nikishin et al. 2022, D'Oro et al. 2023; Ash & Adams 2020):
 * k_param_perturb, csrc/sac_perturb.h -- the whole-network remedies next to sac_recycle_units, the per-unit one.  For every
 * element x of every flat nn.Linear tensor (sac_get_params) of a selected TRAINED net (policy, qf1, qf2; on TD3 handles the
 * online policy):
 *   fresh      f(e) of element e of tensor j (its place in the net's flat tensor list) of net k:
 *                hidden weight fc<l>.weight   bound * s, bound = float32(1 / sqrt((double)N_l)) (networks._Mlp's rule)
 *                hidden bias   fc<l>.bias     the constant b_init[k]: no draw
 *                head weight and head bias    init_w[k] * s (last_fc and, on a SAC policy, last_fc_log_std)
 *              s = 2u - 1 (exact in float32), u = (float(word >> 8) + 0.5f) * 2^-24, word = output word e & 3 of
 *              Philox4x32-10 with counter (e >> 2, j | k << 8, draw lo, draw hi) and key (seed lo, seed hi); the product
 *              with the bound is rounded once
 *   new value  a = shrink * x, formed only if shrink != 0; b = perturb * f, formed only if perturb != 0; x' = a + b where
 *              both are present, else the one that is: every operation rounded once, no FMA.  With shrink == 0 the old
 *              value is not read into the result -- a reset clears a NaN or Inf weight; with shrink != 0 a NaN stays NaN
 *   moments    with SAC_PERTURB_OPT, Adam's m and v of every element written become +0.0; step counts and bias
 *              corrections are untouched (as with sac_recycle_units)
 *   targets    with SAC_PERTURB_TARGETS the target paired with a selected net (target_qf1, target_qf2; on TD3 the target
 *              policy; a SAC policy has none) receives the same new bits in every copy it has.  Without it targets are
 *              left alone, and sac_param_moments' gap jumps
 * Nothing else changes: pads stay +0.0, scalars, counters, generators and buffers stay bit for bit.  Both weight copies of
 * the fused kernels' shapes and the moments where they live are written through the parameter map (csrc/sac_param_map.h);
 * the fresh values are drawn on the device (csrc/sac_perturb_map.h): no parameter crosses the link.  What sac_get_params /
 * sac_get_opt_state return afterwards is infer.shrink_perturb_reference of what they returned before, byte for byte.
 * Both families and both algorithms are served, mixed in one call: ONE k_param_perturb launch on the first member's
 * stream, one wait before return; a member's result does not depend on its neighbours.  Admission is
 * sac_recycle_units_many's (1..16 trainers of one device, none confined by sac_trainer_set_xcd[_mask], none twice); every
 * member is settled first and its acting mirror invalidated.  Refused (<0, sac_last_error, nothing written): a mask that
 * selects no net, bits 3..5 or an unknown bit, unknown flags, shrink or perturb not finite, negative or both zero, a
 * non-finite or negative init_w or a non-finite b_init of a selected net. */
enum { SAC_PERTURB_OPT = 1, SAC_PERTURB_TARGETS = 2 };
typedef struct sac_perturb_io {
    uint32_t nets, flags;        /* nets: bit k selects SAC_NET_* == k, bits 0..2 only; flags: SAC_PERTURB_* */
    float shrink, perturb;
    uint64_t seed, draw;
    float init_w[3], b_init[3];  /* per net id 0..2; read for the selected nets */
} sac_perturb_io_t;
int sac_shrink_perturb(sac_trainer_t *t, const sac_perturb_io_t *io);
int sac_shrink_perturb_many(sac_trainer_t *const *trainers, int n_trainers, const sac_perturb_io_t *io);   /* up to SAC_GROUP_MAX */

/* ------------------------------------------------------------------------------------------
 * Trainer groups: several runs of one configuration (the reference's seed sweeps, /root/reference/launch_jobs.sh)
 * stepped together.  A group holds 1..SAC_GROUP_MAX existing SAC trainers that share obs_dim, act_dim, batch (at most
 * 256 rows), hidden sizes (two layers of at most 256 units) and device; their hyperparameters and noise seeds may differ.
 * sac_group_train_loop runs  for _ in range(n_steps): batch_r = buffers[r].random_batch(B); trainer_r.train(batch_r)
 * for every member r at once: one grouped index draw and one grouped gather per chunk, four grouped launches per step
 * (the four-launch step of every member, fused ones included).  Each member's result -- weights, Adam state, scalars,
 * diagnostics, the generator of its buffer -- is bit for bit that of sac_train_loop(members[r], buffers[r], n_steps),
 * and the members stay ordinary trainers: every sac_* entry point sees the trained state afterwards.  Members must
 * outlive the group; destroying the group leaves them as they are.  Refused (error, nothing changed): TD3 or
 * general-step members, batches above 256, members confined by sac_trainer_set_xcd[_mask], the same trainer or buffer
 * twice, buffers of other dims, empty buffers.
 * diag_first / diag_last (may be NULL): [n_members][SAC_DIAG_N], the first and last step of each member.
 * ------------------------------------------------------------------------------------------ */
enum { SAC_GROUP_MAX = 16 };
typedef struct sac_group sac_group_t;
int sac_group_create(sac_group_t **out, sac_trainer_t *const *members, int n_members);
/* The TD3 form: 1..SAC_GROUP_MAX trainers of td3_trainer_create, under the same conditions (SAC members, and so mixed
 * groups, are refused here as TD3 members are by sac_group_create).  Their policy_and_target_update_period, step counts
 * and every other hyperparameter may differ: each member keeps its own delayed-update plan -- critic step every step,
 * policy step and target update on every policy_and_target_update_period-th step number, the policy statistics on the
 * call's first step too -- and its result is bit for bit sac_train_loop's.
 * sac_group_train_loop and sac_group_destroy serve both kinds.  For a TD3 group, diag_first holds each member's first
 * step (its Policy Loss / Policy Action from the actor pass that step always runs) and diag_last the most recent value of
 * every entry at the end of the call (the policy entries: of the member's last actor pass), as sac_train_loop's do. */
int td3_group_create(sac_group_t **out, sac_trainer_t *const *members, int n_members);
/* Mixed groups: runs of DIFFERENT tasks (a sweep of tasks x seeds) on one device.  1..SAC_GROUP_MAX trainers of one
 * algorithm (sac_group_create_mixed: SAC, td3_group_create_mixed: TD3) whose obs_dim, act_dim (at most 16) and batch
 * (1..256 rows) may differ per member; hidden sizes and the device must still agree, and every other refusal of
 * sac_group_create holds.  Members of one kernel variant (head tiles from act_dim, first-layer width from obs_dim)
 * share one grouped launch per step kernel; the variants follow one another on the group's stream.  Buffer r must have
 * member r's dims, and member r draws n_steps batches of its own batch size from it; buffers bound to one host generator
 * continue it in member order with each member's batch.  Each member's result is bit for bit that of
 * sac_train_loop(members[r], buffers[r], n_steps).  sac_group_train_loop and sac_group_destroy serve mixed groups too. */
int sac_group_create_mixed(sac_group_t **out, sac_trainer_t *const *members, int n_members);
int td3_group_create_mixed(sac_group_t **out, sac_trainer_t *const *members, int n_members);
/* MLP groups: runs of the GENERAL step (sac_trainer_create_mlp / td3_trainer_create_mlp: hidden sizes other than two
 * layers of at most 256 units -- a network-width or network-depth sweep) on one device.  1..SAC_GROUP_MAX trainers of one
 * algorithm (sac_group_create_mlp: SAC, td3_group_create_mlp: TD3) that share the device and the hidden sizes (the
 * policy's list and the Q nets' list); obs_dim, act_dim and batch may differ per member, as may every hyperparameter and
 * noise seed, and TD3 members keep their own delayed-update plan as in td3_group_create.  Each stage of the general
 * step's launch list is one grouped launch (the elementwise stages: one per action bound, up to 8 / up to 16 actions);
 * every member keeps its own tiles, split reductions and summation orders, so its result -- weights, Adam state,
 * scalars, diagnostics, the generator of its buffer -- is bit for bit that of sac_train_loop(members[r], buffers[r],
 * n_steps), and the members stay ordinary trainers.  Refused (error, nothing changed): members with the shapes of the
 * fused kernels (their solo step is not the general step), members of the other algorithm, different hidden sizes or
 * devices, members confined by sac_trainer_set_xcd[_mask], the same trainer or buffer twice, buffers of other dims than
 * their member, empty buffers, more than SAC_GROUP_MAX members.  The other group kinds keep refusing general-step
 * members.  sac_group_train_loop and sac_group_destroy serve MLP groups too. */
int sac_group_create_mlp(sac_group_t **out, sac_trainer_t *const *members, int n_members);
int td3_group_create_mlp(sac_group_t **out, sac_trainer_t *const *members, int n_members);
/* Arch groups: general-step runs of DIFFERENT hidden sizes (a network-width or network-depth sweep) on one device.
 * 1..SAC_GROUP_MAX trainers of one algorithm (sac_group_create_arch: SAC, td3_group_create_arch: TD3); each member's
 * policy and Q hidden lists may be any the general step takes (1..7 layers of 1..4096 units), and may differ from each
 * other; dims, batch, hyperparameters, noise seeds and TD3 update periods may differ as in MLP groups.  The group walks
 * a merged schedule: every member's launch list has the same elementwise stages in the same order, and between two of
 * them runs of GEMM stages by mode (forward, backward, weight gradients); each such run becomes as many grouped GEMM
 * launches as the longest member's, member m taking part in the first count_m of them.  Every member runs its own
 * stages in its own order with its own tiles, split factors and job order, so its result is bit for bit that of
 * sac_train_loop(members[r], buffers[r], n_steps).  Refused (error, nothing changed) as by sac_group_create_mlp, except
 * that hidden sizes may differ.  sac_group_train_loop and sac_group_destroy serve arch groups too. */
int sac_group_create_arch(sac_group_t **out, sac_trainer_t *const *members, int n_members);
int td3_group_create_arch(sac_group_t **out, sac_trainer_t *const *members, int n_members);
/* The grouped stages of one full step of group g, any kind (MLP and arch groups: SAC the step's grouped stages, TD3 the
 * critic pass's plus the actor pass's; the fused kinds: 4 for SAC, 7 for TD3), or -2 for NULL (an argument error). */
int sac_group_stage_count(const sac_group_t *g);
int sac_group_destroy(sac_group_t *g);
int sac_group_train_loop(sac_group_t *g, sac_buffer_t *const *buffers, int64_t n_steps, float *diag_first,
                         float *diag_last);

/* ------------------------------------------------------------------------------------------
 * Acting sessions: sac_policy_act_many for a FIXED list of trainers without the per-call marshalling (csrc/sac_actor.h).
 * A session owns one mapped pinned slab that holds every member's observations, eps and actions at fixed addresses --
 * the caller writes and reads them in place, a call copies nothing -- and a member table in device memory that is
 * written once, at creation.  sac_actor_act rewrites a 256-byte control block (rows, first workgroup, stochastic flag
 * per member), launches k_act_session once and waits for one event.  Each member's actions are bit for bit those of
 * sac_policy_act_device on the observations cast to float32 with the same eps; every refusal returns <0, sets
 * sac_last_error and changes nothing.  Several sessions over the same trainers coexist (they share the weights only).
 * ------------------------------------------------------------------------------------------ */
typedef struct sac_actor sac_actor_t;
/* 1..SAC_GROUP_MAX trainers of one device with the fused kernels' shapes (SAC and TD3, dims mixed); max_rows[i] in
 * 1..1024.  Refused: null or duplicate trainers, more than SAC_GROUP_MAX, trainers on different devices, general-step
 * trainers, max_rows outside 1..1024. */
int sac_actor_create(sac_actor_t **out, sac_trainer_t *const *trainers, int n_trainers, const int32_t *max_rows);
int sac_actor_destroy(sac_actor_t *a);          /* members are left as they are; they must outlive the session */
/* member i's arrays inside the session's mapped pinned slab, fixed for the session's life and 256-byte aligned:
 * obs (max_rows, O) FLOAT64 row-major (rounded to fp32 by the kernel as numpy's astype(float32) does),
 * eps (max_rows, A) float32, act (max_rows, A) float32.  Any of the three out pointers may be NULL. */
int sac_actor_arrays(sac_actor_t *a, int member, double **obs, float **eps, float **act);
/* act on rows [0, n_rows[i]) of every member's obs (and eps, for a stochastic SAC member); 0 = sits out (its arrays are
 * not touched); rows of act at and beyond n_rows[i] are not written.  The members with rows are drained first as by
 * sac_sync, so the actions come from the weights as of the last completed step of any step path.  Refused: n_rows[i]
 * outside 0..max_rows[i], all n_rows zero, a member confined by sac_trainer_set_xcd[_mask]. */
int sac_actor_act(sac_actor_t *a, const int32_t *n_rows, const int32_t *deterministic);

/* ------------------------------------------------------------------------------------------
 * Acting sessions for GENERAL-STEP trainers: sac_policy_act_general_many for a FIXED list of trainers without the
 * per-call marshalling (csrc/sac_actor_general.h).  A session owns one mapped pinned slab laid out as sac_actor's (a
 * control block, then per member obs float64, eps and act float32 at fixed 256-byte-aligned addresses), a job table in
 * device memory -- member i's layer l: weights, input, output, shapes -- written once at creation, and two activation
 * buffers per member of its own (not the trainers': sessions over the same trainers and sac_policy_act_general share
 * the weights only).  sac_gactor_act rewrites the control block (rows and stochastic flag per member, first workgroup
 * per layer depth and member), launches k_act_layer_session once per layer depth and waits for one event; it copies
 * nothing, allocates nothing and rebuilds no table.  Each member's actions are bit for bit those of
 * sac_policy_act_general on the observations cast to float32 with the same eps; every refusal returns <0, sets
 * sac_last_error and changes nothing.
 * ------------------------------------------------------------------------------------------ */
typedef struct sac_gactor sac_gactor_t;
/* 1..SAC_GROUP_MAX general-step trainers of one device (SAC and TD3, dims, depths and widths mixed); max_rows[i] in
 * 1..1024.  Refused (*out is NULL): null or duplicate trainers, more than SAC_GROUP_MAX, trainers on different devices,
 * trainers with the fused kernels' shapes (sac_actor_create is their entry), max_rows outside 1..1024. */
int sac_gactor_create(sac_gactor_t **out, sac_trainer_t *const *trainers, int n_trainers, const int32_t *max_rows);
int sac_gactor_destroy(sac_gactor_t *a);        /* members are left as they are; they must outlive the session */
/* member i's arrays inside the slab, as sac_actor_arrays: obs (max_rows, O) FLOAT64 (rounded to fp32 by the kernel as
 * numpy's astype(float32) does), eps (max_rows, A) float32, act (max_rows, A) float32.  Out pointers may be NULL. */
int sac_gactor_arrays(sac_gactor_t *a, int member, double **obs, float **eps, float **act);
/* as sac_actor_act: rows [0, n_rows[i]) of every member, 0 = sits out, rows of act at and beyond n_rows[i] are not
 * written, members with rows are drained first as by sac_sync.  Refused: n_rows[i] outside 0..max_rows[i], all n_rows
 * zero, a member confined by sac_trainer_set_xcd[_mask]. */
int sac_gactor_act(sac_gactor_t *a, const int32_t *n_rows, const int32_t *deterministic);

#ifdef __cplusplus
}
#endif
#endif /* SAC_HIP_H */
