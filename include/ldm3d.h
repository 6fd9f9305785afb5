/* ldm3d.h - C ABI of libldm3d.so: the MI355X-native (gfx950) 3D latent-diffusion denoising path.
 *
 * This is the drop-in boundary for the hot path of sanazkaviani/3d-latent-diffusion-model.  The reference has
 * no native code: its plug point is the JSON "_target_" class instantiated by define_instance
 * (3d_ldm/utils.py:243-246) and then used through the nn.Module surface; each entry point below cites the
 * reference call it serves.  The host-side mirror (the .py files of 3d-latent-diffusion-model_amd/, loaded with ctypes)
 * exposes these as the same nn.Module / scheduler / inferer objects.  See INTEGRATION.md.
 *
 * Conventions
 *   - every function returns 0 on success or a negative ldm_status; ldm_last_error() gives the message
 *     (thread local).  Nothing aborts, nothing throws across the ABI.
 *   - all tensor arguments are DEVICE pointers owned by the caller; image/latent tensors are fp32 NCDHW
 *     (the reference's layout); the library converts to its internal NDHWC bf16 layout itself.
 *   - the caller owns the workspace (size from *_workspace_bytes); the library owns weights and plans.
 *     No allocation, no synchronisation on the forward/step path: every launch goes to `stream`
 *     (a hipStream_t passed as void*), so calls may be captured into a hipGraph.
 *   - handles are not thread safe; one process per GPU (torchrun model, 3d_ldm/train_diffusion.py:43-51).
 */
#ifndef LDM3D_H
#define LDM3D_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LDM_MAX_LEVELS 8
#define LDM_ABI_VERSION 1

typedef enum {
    LDM_OK = 0,
    LDM_ERR_BAD_ARG = -1,
    LDM_ERR_UNSUPPORTED = -2,     /* shape / config outside what the kernels implement */
    LDM_ERR_HIP = -3,
    LDM_ERR_NOT_LOADED = -4,      /* forward called before every parameter was uploaded */
    LDM_ERR_WORKSPACE = -5,       /* workspace too small */
    LDM_ERR_RCCL = -6
} ldm_status;

/* kwargs of "diffusion_def" (3d_ldm/config/config_train_16g.json:39-48); MONAI defaults norm_num_groups=32,
 * norm_eps=1e-6 are filled by the host mirror. */
typedef struct {
    int spatial_dims;                         /* only 3 */
    int in_channels, out_channels;
    int num_levels;
    int channels[LDM_MAX_LEVELS];
    int attention_levels[LDM_MAX_LEVELS];
    int num_head_channels[LDM_MAX_LEVELS];
    int num_res_blocks[LDM_MAX_LEVELS];
    int norm_num_groups;
    float norm_eps;
} ldm_unet_cfg;

/* kwargs of "autoencoder_def" (3d_ldm/config/config_train_16g.json:7-28). */
typedef struct {
    int spatial_dims;                         /* only 3 */
    int in_channels, out_channels, latent_channels;
    int num_levels;
    int channels[LDM_MAX_LEVELS];
    int num_res_blocks[LDM_MAX_LEVELS];
    int attention_levels[LDM_MAX_LEVELS];
    int norm_num_groups;
    float norm_eps;
    int with_encoder_nonlocal_attn, with_decoder_nonlocal_attn;
} ldm_vae_cfg;

typedef struct ldm_model ldm_model;           /* a UNet or an AutoencoderKL: weights + cached launch plans */

int ldm_version(void);
const char* ldm_last_error(void);

/* ---- construction (replaces define_instance(args, "diffusion_def" / "autoencoder_def"),
 *      3d_ldm/utils.py:243-246, 3d_ldm/inference.py:71,75, 3d_ldm/train_diffusion.py:90,127) ------------ */
int ldm_unet_create(const ldm_unet_cfg* cfg, ldm_model** out);
int ldm_vae_create(const ldm_vae_cfg* cfg, ldm_model** out);
void ldm_model_destroy(ldm_model* m);

/* ---- parameters: MONAI-shaped state_dict (replaces load_state_dict, 3d_ldm/inference.py:73,77,
 *      3d_ldm/train_diffusion.py:92-95,129-136).  Enumerate names/shapes, then upload fp32 HOST arrays. ----- */
int ldm_model_num_params(const ldm_model* m);
const char* ldm_model_param_name(const ldm_model* m, int i);
int ldm_model_param_ndim(const ldm_model* m, int i);
const int64_t* ldm_model_param_shape(const ldm_model* m, int i);
int ldm_model_load_param(ldm_model* m, const char* name, const float* host_data, size_t numel);
int64_t ldm_model_param_numel_total(const ldm_model* m);

/* ---- DiffusionModelUNet.forward(x, timesteps, context=None)
 *      (reached via inferer(...) 3d_ldm/train_diffusion.py:197-205,260-268 and inferer.sample(...)
 *      3d_ldm/train_diffusion.py:326-333, 3d_ldm/inference.py:94-99).
 *      x:[B,Cx,D,H,W], cond:[B,Cc,D,H,W] or NULL (mode="concat": Cx + Cc == in_channels), timesteps:[B] fp32,
 *      out:[B,out_channels,D,H,W]; all fp32 NCDHW device memory. ---------------------------------------------- */
size_t ldm_unet_workspace_bytes(ldm_model* m, int B, int D, int H, int W);
int ldm_unet_forward(ldm_model* m, const float* x, int x_channels, const float* cond, int cond_channels,
                     const float* timesteps, float* out, int B, int D, int H, int W,
                     void* workspace, size_t workspace_bytes, void* stream);

/* ---- one training step of the diffusion UNet (3d_ldm/train_diffusion.py:197-223: inferer(...) -> F.mse_loss ->
 *      loss.backward() -> clip_grad_norm_(1.0) -> Adam.step()).
 *      train_forward == forward, but keeps every activation / statistic in `workspace`; train_backward consumes that
 *      workspace and dLoss/d eps_hat (fp32 [B,out_channels,D,H,W]) and overwrites flat_grads (fp32, one element per
 *      parameter element: parameter i starts at ldm_model_param_offset(m, i) and has its MONAI tensor layout).
 *      load_params_device re-packs the fp32 master parameters (HOST array of n DEVICE pointers, library order) into
 *      the bf16 weight arena after an optimizer step.  The flat layout is what the data-parallel all-reduce
 *      (3d_ldm/train_diffusion.py:147-149 DDP) runs over: one ldm_comm_allreduce of the whole buffer. ----------------- */
int64_t ldm_model_param_offset(const ldm_model* m, int i);
int ldm_model_load_params_device(ldm_model* m, const float* const* device_ptrs, int n, void* stream);
int ldm_model_load_params_flat(ldm_model* m, const float* flat_device, void* stream);   /* all parameters in ONE buffer at their ldm_model_param_offset */
size_t ldm_unet_train_workspace_bytes(ldm_model* m, int B, int D, int H, int W);
int ldm_unet_train_forward(ldm_model* m, const float* x, int x_channels, const float* cond, int cond_channels,
                           const float* timesteps, float* out, int B, int D, int H, int W,
                           void* workspace, size_t workspace_bytes, void* stream);
int ldm_unet_train_backward(ldm_model* m, const float* grad_out, float* flat_grads, int B, int D, int H, int W,
                            void* workspace, size_t workspace_bytes, void* stream);
/* The same backward with gradients w.r.t. the network input (guidance by the gradient of a loss on the model's prediction:
 * DPS, reconstruction guidance): dx fp32 [B,x_channels,D,H,W] and dcond [B,cond_channels,D,H,W], the channel counts of the
 * ldm_unet_train_forward call that filled `workspace`, are overwritten with dLoss/dx and dLoss/dcond.  Either may be NULL.
 * flat_grads as above, or NULL: the data-only backward -- no bias column sums, no weight or time-embedding gradients, no
 * export into a gradient buffer and no all-reduce even with a communicator attached (ldm_model_grad_sync_pending stays 0).
 * dx == dcond == NULL is ldm_unet_train_backward: the same plan, launches and bytes.  All three NULL: LDM_ERR_BAD_ARG,
 * nothing launched.  conv_in's data gradient runs on the general data-gradient conv and an unpack into dx | dcond, or with
 * LDM_DGRAD_THIN=1 (read when a plan is built) on conv3_dgrad_thin_kernel (at most 32 input channels).  The three forms
 * are plans of their own over the forward's activations: ldm_unet_train_input_workspace_bytes is the workspace that serves
 * the forward and all of them; ldm_unet_train_workspace_bytes is unchanged. */
int ldm_unet_train_backward_input(ldm_model* m, const float* grad_out, float* flat_grads /* NULL: no parameter gradients */,
                                  float* dx /* NULL */, float* dcond /* NULL */,
                                  int B, int D, int H, int W, void* workspace, size_t workspace_bytes, void* stream);
size_t ldm_unet_train_input_workspace_bytes(ldm_model* m, int B, int D, int H, int W);
/* AutoencoderKL.forward(images) -> (reconstruction, z_mu, z_sigma) with its backward (stage-1 trainer,
 * 3d_ldm/train_autoencoder.py:366-451: recons + KL losses -> loss_g.backward()).  eps: [B,L,d,h,w] N(0,1) draws of the
 * sampling step; d_mu / d_sigma: gradients of the KL term w.r.t. z_mu / z_sigma (NULL = 0); flat_grads as above. */
size_t ldm_vae_train_workspace_bytes(ldm_model* m, int B, int D, int H, int W);
int ldm_vae_train_forward(ldm_model* m, const float* x, const float* eps, float* recon, float* z_mu, float* z_sigma,
                          int B, int D, int H, int W, void* workspace, size_t workspace_bytes, void* stream);
int ldm_vae_train_backward(ldm_model* m, const float* d_recon, const float* d_mu, const float* d_sigma, float* flat_grads,
                           int B, int D, int H, int W, void* workspace, size_t workspace_bytes, void* stream);
/* Optimizer tail on flat fp32 buffers (torch.nn.utils.clip_grad_norm_(params, max_norm) 3d_ldm/train_diffusion.py:216
 * and torch.optim.Adam(lr) :155, torch defaults betas (0.9, 0.999), eps 1e-8, no weight decay):
 *   grad_sq_norm: *out (device fp32 scalar) = sum g^2.
 *   adam_step: g' = g * min(1, max_norm / (sqrt(*sq_norm) + 1e-6)) when sq_norm != NULL and max_norm > 0; then
 *              m = b1 m + (1-b1) g'; v = b2 v + (1-b2) g'^2; p = p (1 - lr wd) - lr * (m / (1-b1^step)) / (sqrt(v / (1-b2^step)) + eps)
 *              (wd = 0: torch.optim.Adam of train_diffusion.py:155; wd > 0: the decoupled AdamW of train_autoencoder.py:274-279).
 *   sq_norm points at TWO device floats {sum g^2, skipped steps}: the NaN-skip of the reference's trainers (train_diffusion.py:210-212
 *   `continue`s in front of backward when the loss is NaN) without a host read: when sum g^2 is not finite (a NaN loss makes every
 *   gradient NaN; the data-parallel mean carries it to every rank) the step leaves params / exp_avg / exp_avg_sq untouched and adds 1
 *   to sq_norm[1]; the bias corrections use step - sq_norm[1].  The caller zeroes sq_norm[1] once; ldm_grad_sq_norm writes out[0] only.
 *   The skip depends on sq_norm alone: max_norm <= 0 switches the clip factor off, not the finite check (pass sq_norm = NULL for a
 *   plain Adam step with neither).
 *   ldm_grad_sq_norm and ldm_op_mse_loss reduce through ONE scratch buffer per process (allocated on the device that is current at
 *   the first call): call them from one stream of one device at a time. */
int ldm_grad_sq_norm(const float* flat_grads, int64_t n, float* out, void* stream);
/* F.mse_loss(noise_pred, noise) of 3d_ldm/train_diffusion.py:207 together with the gradient loss.backward() (:214) hands to the network:
 * loss_out[0] = mean((pred - target)^2), grad_out (optional) = 2 (pred - target) / n; fp32 device buffers of n elements. */
int ldm_op_mse_loss(const float* pred, const float* target, int64_t n, float* loss_out, float* grad_out, void* stream);
int ldm_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1,
                  float beta2, float eps, float weight_decay, int step, const float* sq_norm, float max_norm, void* stream);
/* Adam(W) over a model's flat fp32 parameter buffer (layout of ldm_model_param_offset) that re-packs the library's bf16 weight
 * arena from the updated values in the same pass (optimizer.step() + the implicit "weights changed", train_diffusion.py:219). */
int ldm_model_adam_step(ldm_model* m, float* params_flat, const float* grads_flat, float* exp_avg, float* exp_avg_sq, float lr,
                        float beta1, float beta2, float eps, float weight_decay, int step, const float* sq_norm, float max_norm,
                        void* stream);
/* The two optimizer steps above with an exponential moving average of the parameters kept in the same launch: `ema` is a fp32
 * buffer in the layout of `params` (the caller initialises it, usually as a copy of the parameters), and per updated element, after
 * the new parameter value p is formed,
 *   a = (step - sq_norm[1]) - 1 (updates applied before this one);  d = ema_warmup ? min(ema_decay, (1 + a) / (10 + a)) : ema_decay;
 *   ema = ema + (1 - d) (p - ema)
 * (warm-up series 0.1, 2/11, 3/12, ... capped at ema_decay).  It lives here because the NaN-skip is decided on the device: a skipped
 * step leaves `ema` untouched like params / exp_avg / exp_avg_sq and does not advance the warm-up; sq_norm == NULL counts no skips.
 * params / exp_avg / exp_avg_sq come out bit-identical to the entries without EMA.  ema == NULL or ema_decay outside [0, 1) (NaN
 * included): LDM_ERR_BAD_ARG before any launch.  ldm_model_adam_step_ema packs the arena from the LIVE weights and leaves the model
 * in the state ldm_model_adam_step leaves it in. */
int ldm_adam_step_ema(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* ema, int64_t n, float lr,
                      float beta1, float beta2, float eps, float weight_decay, int step, float ema_decay, int ema_warmup,
                      const float* sq_norm, float max_norm, void* stream);
int ldm_model_adam_step_ema(ldm_model* m, float* params_flat, const float* grads_flat, float* exp_avg, float* exp_avg_sq,
                            float* ema_flat, float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                            float ema_decay, int ema_warmup, const float* sq_norm, float max_norm, void* stream);

/* HIP-graph replay of the UNet forward plan (the sampling loop of 3d_ldm/inference.py:88-99 calls the UNet 1000 times per
 * volume with the same shapes): with on != 0, ldm_unet_forward records its launches into a hipGraph the second time it sees
 * a (x, cond, timesteps, out, workspace, stream) pointer set and replays it afterwards.  Results are identical. */
int ldm_model_set_graph_mode(ldm_model* m, int on);

/* ---- precision of the inference AND training plans of both networks.  The reference computes in fp32 (autocast off: 3d_ldm/train_diffusion.py:177,237;
 *      3d_ldm/inference.py:91-99 has no autocast): LDM_PREC_FP32 runs the same plans on fp32 activations / weights with the
 *      fp32 matrix instruction (v_mfma_f32_32x32x2_f32; the convolutions of the inference plans as three bf16 MFMAs per product on
 *      hi / lo splits of the fp32 operands, fp32-class accuracy) and stays within ~5e-5 rel-L2 of the CPU path; LDM_PREC_BF16 (default)
 *      is the bf16-MFMA headline path (~3e-2 at the benchmark depth, its own rounding floor).  After switching to fp32 upload the
 *      parameters again (the unrounded copies are made at upload time). ------------------------------------------------- */
#define LDM_PREC_BF16 0
#define LDM_PREC_FP32 1
int ldm_model_set_precision(ldm_model* m, int precision);
int ldm_model_get_precision(const ldm_model* m);

/* ---- debug taps: every block output of an inference plan as fp32 NCDHW, optionally followed by overwriting it with the
 *      caller's tensor (teacher forcing), for stage-wise parity tests against the oracle.  kind = "unet" | "enc" | "dec". ---- */
int ldm_model_tap_count(ldm_model* m, const char* kind, int B, int D, int H, int W);
int64_t ldm_model_tap_elems(ldm_model* m, const char* kind, int B, int D, int H, int W);
int ldm_model_tap_info(ldm_model* m, const char* kind, int B, int D, int H, int W, int i, char* name, int name_cap, int dims[5],
                       int64_t* offset);
size_t ldm_model_taps_workspace_bytes(ldm_model* m, const char* kind, int B, int D, int H, int W, int force);
int ldm_unet_forward_taps(ldm_model* m, const float* x, int x_channels, const float* cond, int cond_channels,
                          const float* timesteps, float* out, int B, int D, int H, int W, float* taps_out, const float* taps_in,
                          void* workspace, size_t workspace_bytes, void* stream);
int ldm_vae_encode_taps(ldm_model* m, const float* x, const float* eps, float* z_mu, float* z_sigma, float* z,
                        int B, int D, int H, int W, float* taps_out, const float* taps_in,
                        void* workspace, size_t workspace_bytes, void* stream);
int ldm_vae_decode_taps(ldm_model* m, const float* z, float* out, int B, int d, int h, int w, float* taps_out, const float* taps_in,
                        void* workspace, size_t workspace_bytes, void* stream);

/* ---- AutoencoderKL.encode / sampling / decode (3d_ldm/train_diffusion.py:104,180,195,249,258,310,324;
 *      3d_ldm/train_autoencoder.py:366,579).  encode: x:[B,Cin,D,H,W] -> z_mu, z_sigma, z = mu + sigma*eps
 *      (each [B,L,D/f,H/f,W/f], any of the three outputs may be NULL; eps NULL means eps = 0).
 *      decode: z:[B,L,d,h,w] -> out:[B,Cout,d*f,h*f,w*f]. ------------------------------------------------------ */
size_t ldm_vae_encode_workspace_bytes(ldm_model* m, int B, int D, int H, int W);
size_t ldm_vae_decode_workspace_bytes(ldm_model* m, int B, int d, int h, int w);
int ldm_vae_encode(ldm_model* m, const float* x, const float* eps, float* z_mu, float* z_sigma, float* z,
                   int B, int D, int H, int W, void* workspace, size_t workspace_bytes, void* stream);
int ldm_vae_decode(ldm_model* m, const float* z, float* out, int B, int d, int h, int w,
                   void* workspace, size_t workspace_bytes, void* stream);

/* ---- scheduler arithmetic (monai DDPMScheduler / DDIMScheduler as built at 3d_ldm/inference.py:79-84,
 *      3d_ldm/train_diffusion.py:140-145).  The host mirror keeps the fp32 beta / alpha-bar tables and passes
 *      the per-step scalars; these launches are the element-wise part, n = number of elements. ------------------ */
/* add_noise: out = sqrt_a[b]*x0 + sqrt_b[b]*eps; sqrt_a, sqrt_b: [B] device fp32 (3d_ldm/train_diffusion.py:197-205) */
int ldm_add_noise(const float* x0, const float* eps, const float* sqrt_a, const float* sqrt_b, float* out,
                  int B, int64_t per_sample, void* stream);
int ldm_scale(const float* x, float* y, int64_t n, float s, void* stream);
/* the host-driven scheduler step.  prediction types (monai prediction_type): 0 "epsilon", 1 "sample" (x0), 2 "v_prediction".
 * a = abar_t, b = 1 - abar_t, m = model output:
 *      epsilon  x0 = (x - sqrt(b) m) / sqrt(a)   eps = m
 *      sample   x0 = m                          eps = (x - sqrt(a) m) / sqrt(b)   (before the clip)
 *      v        x0 = sqrt(a) x - sqrt(b) m      eps = sqrt(a) m + sqrt(b) x
 *      then clip x0; ddpm: prev = c0*x0 + c1*x, ddim: prev = c0*x0 + c1*eps (c1 = dir); + sigma*noise.  kind 0 = DDPM, 1 = DDIM.
 *      row: the 8 host floats of one sampler row (ldm_sampler_create), read before the call returns.  The same per-element arithmetic
 *      as the device sampler (bit for bit); x0_out may be NULL, and a NULL noise means sigma = 0. */
int ldm_scheduler_step(const float* model_out, const float* x, const float* noise, float* prev, float* x0_out, int64_t n, int kind, int pred,
                       const float* row, int clip, void* stream);
/* noisy = sqrt_a[b]*x0 + sqrt_b[b]*eps (skipped if noisy is NULL) and the training target of type `pred` in one pass: eps | x0 |
 * sqrt_a[b]*eps - sqrt_b[b]*x0 (monai get_velocity). */
int ldm_add_noise_target(const float* x0, const float* eps, const float* sqrt_a, const float* sqrt_b, float* noisy, float* target,
                         int B, int64_t per_sample, int pred, void* stream);
/* Stage-2 training from cached latents: the input side of one step in one launch.  The cache is four device tensors [N][per_sample]
 * fp32 (mu and sigma of the frozen autoencoder for the label and for the image of every sample); idx is a HOST array of B dataset
 * indices, read before the call returns.  For batch slot b and row r = idx[b]:
 *      z      = (mu_label[r] + sigma_label[r] * e_label[b]) * scale          (the multiply is skipped when scale == 1)
 *      cond   =  mu_image[r] + sigma_image[r] * e_image[b]                   (unscaled)
 *      noisy  = sqrt_a[b] * z + sqrt_b[b] * noise[b]
 *      target = noise[b] | z | sqrt_a[b] * noise[b] - sqrt_b[b] * z          (pred 0 | 1 | 2, as ldm_add_noise_target)
 * sqrt_a, sqrt_b: [B] device; noisy, cond, target: [B][per_sample] device.  Rounded exactly as the chain ldm_vae_encode (z = mu + sigma *
 * eps) -> fp32 multiply by scale -> ldm_add_noise (pred 0) | ldm_add_noise_target (pred 1, 2) rounds, so the outputs equal that chain's
 * bit for bit (for pred 0: as ldm_add_noise rounds launches of at most 2^20 elements).
 * Explicit draws: e_label, e_image, noise, each [B][per_sample] device, draws_out NULL.
 * Device draws: all three NULL; N(0, 1) by Philox4x32-10 + Box-Muller with
 *      counter = (element / 4 within the sample, dataset index idx[b], step, 0x1a7e0000 + stream), key = (seed low word, seed high word),
 *      stream 0 = e_label, 1 = e_image, 2 = noise; output lane e of a block is element 4 * (element / 4) + e.
 *   A draw depends on (seed, step, dataset index, stream, element) alone, never on the batch slot or the batch size; counter word 3 keeps
 *   the stream apart from the device sampler's (constant 0x5eed there).  draws_out (optional, [3][B][per_sample]: e_label, e_image, noise)
 *   receives the draws, so that the call can be replayed with explicit draws.
 * LDM_ERR_BAD_ARG, with nothing launched: a NULL tensor, B outside 1 .. 64, an idx[b] outside 0 .. N - 1, per_sample outside 1 .. 2^33,
 * an unknown pred, some but not all of the three draws NULL, draws_out together with explicit draws. */
int ldm_latent_batch(const float* mu_label, const float* sigma_label, const float* mu_image, const float* sigma_image, int N, int64_t per_sample,
                     const int* idx, int B, const float* sqrt_a, const float* sqrt_b, float scale, int pred,
                     const float* e_label, const float* e_image, const float* noise, uint64_t seed, uint32_t step,
                     float* noisy, float* cond, float* target, float* draws_out, void* stream);

/* ---- rectified flow (MONAI >= 1.4 monai.networks.schedulers.RFlowScheduler, restated; not on the reference's path).  T =
 *      num_train_timesteps, tau = t / T: tau = 1 is pure noise, tau = 0 is data, and the model predicts the velocity x0 - noise.
 *      These are new entries: the pred / kind arguments of the entries above keep their domains. ------------------------------------ */
/* RFlowScheduler.step: prev = x + dt m, x0_out (optional) = x + tau m, each one fused multiply-add, with one sampler row
 * {dt, tau, 0, 0, 0, t, 0, 0} (8 host floats, as ldm_sampler_create_rflow takes them, read before the call returns).  The same
 * per-element arithmetic as the device sampler, bit for bit.  prev may alias x; x0_out may alias nothing. */
int ldm_rflow_step(const float* m, const float* x, float* prev, float* x0_out, int64_t n, const float* row, void* stream);
/* RFlowScheduler.add_noise and the training target in one pass: noisy = a[b]*x0 + b[b]*noise (skipped if noisy is NULL; a = 1 - tau,
 * b = tau: [B] device) and target = x0 - noise.  noisy rounds as ldm_add_noise rounds launches of at most 2^20 elements. */
int ldm_rflow_noise_target(const float* x0, const float* noise, const float* a, const float* b, float* noisy, float* target,
                           int B, int64_t per_sample, void* stream);
/* ldm_latent_batch for a rectified-flow model: its parameters without pred, one_minus_tau / tau [B] where sqrt_a / sqrt_b stand
 * there; noisy = one_minus_tau[b] * z + tau[b] * noise[b] (rounded the same way) and target = z - noise[b].  Draws, keys, the unscaled
 * condition and the refusals are ldm_latent_batch's; the outputs equal the chain ldm_vae_encode -> scale -> ldm_rflow_noise_target bit
 * for bit. */
int ldm_latent_batch_rflow(const float* mu_label, const float* sigma_label, const float* mu_image, const float* sigma_image, int N, int64_t per_sample,
                           const int* idx, int B, const float* one_minus_tau, const float* tau, float scale,
                           const float* e_label, const float* e_image, const float* noise, uint64_t seed, uint32_t step,
                           float* noisy, float* cond, float* target, float* draws_out, void* stream);
/* RFlowScheduler.sample_timesteps and the two coefficients of its add_noise for the B samples of a training step, in one launch (in place
 * of torch.rand / randn, the multiply, the floor, the transform and two more element-wise launches).  method 0 "uniform": t = u T, u in
 * [0, 1); 1 "logit-normal": t = sigmoid(loc + scale n) T, n ~ N(0, 1); discrete != 0 floors t; transform_ratio r != 0 then maps t to
 * T r s / (1 + (r - 1) s), s = t / T (r = (input_img_size_numel / base_img_size_numel)^(1 / spatial_dim) * transform_scale; 0 = off).
 * draw: [B] device (u or n), or NULL for Philox4x32-10 with counter = (0, idx[b], step, 0x1a7e0000 + 3), key = seed: the key layout of
 * ldm_latent_batch on a fourth stream, so a draw depends on (seed, step, dataset index) alone.  idx: HOST array of B dataset indices
 * (NULL: 0 .. B-1), read before the call returns.  Outputs, [B] device fp32: t (the UNet's timestep input), one_minus_tau = 1 - t / T
 * and tau = t / T (what ldm_rflow_noise_target / ldm_latent_batch_rflow take).
 * LDM_ERR_BAD_ARG, with nothing launched: B outside 1 .. 64, an unknown method, T < 1, scale <= 0 for logit-normal, a negative ratio,
 * a NULL output. */
int ldm_rflow_timesteps(const int* idx, int B, int T, int method, float loc, float scale, int discrete, float transform_ratio,
                        const float* draw, uint64_t seed, uint32_t step, float* t, float* one_minus_tau, float* tau, void* stream);

/* ---- stage-2 objective: per-timestep loss weights, a per-bin tracker of the loss, a loss-aware timestep draw (csrc/loss_weight.h).
 * Weighted loss: l_b = mean_i (pred - target)^2 over sample b of [B][per_sample] device fp32, w_b = w_table[timesteps[b]] * sample_w[b]
 * (w_table [T] and sample_w [B] device fp32; a NULL factor is 1; timesteps [B] device int64, required with w_table or tracker),
 *   loss_out[0] = (1/B) sum w_b l_b (the value differentiated)     loss_out[1] = (1/B) sum l_b (what ldm_op_mse_loss reports)
 *   per_sample_out[b] = l_b (optional)                             grad_out = 2 w_b (pred - target) / (B per_sample) (optional).
 * Two launches, a deterministic two-stage reduction (no atomics; a repeat is bit-identical); with B = 1 and no weights both outputs are
 * ldm_op_mse_loss's bit for bit.  16-byte accesses where per_sample % 4 == 0 and pred / target / grad_out are 16-byte aligned, scalar
 * ones otherwise; nothing behind B * per_sample is touched.  A timestep outside [0, T) does not index the table: that sample's weight
 * is NaN (loss_out[0] and its gradient NaN: the optimizer's device NaN-skip counts the step).
 * tracker (optional, device fp32 [2][K]: second moments, then counts; zero-filled = empty) is updated by one thread in batch order:
 * bin k = (t_b K) / T; a sample with a non-finite l_b or a timestep outside the table is skipped; count_k == 0: m2_k = l_b^2, else
 * m2_k = beta m2_k + (1 - beta) l_b^2; count_k += 1 (fp32, stops at 2^24).  It sees the unweighted l_b.
 * One scratch buffer per device: one stream at a time, as for ldm_op_mse_loss.
 * LDM_ERR_UNSUPPORTED: B > 64.  LDM_ERR_BAD_ARG: NULL pred / target / loss_out, B, per_sample or T < 1, K outside 1 .. min(64, T)
 * (K is checked with or without a tracker), beta outside [0, 1) with a tracker.  Nothing is launched on a refusal. */
int ldm_op_weighted_mse_loss(const float* pred, const float* target, int B, int64_t per_sample, const int64_t* timesteps,
                             const float* w_table, int T, const float* sample_w, float* tracker, int K, float tracker_beta,
                             float* loss_out, float* per_sample_out, float* grad_out, void* stream);
/* Loss-aware draw of B training timesteps from a tracker.  Bin k holds the n_k timesteps t with (t K) / T == k.  While any count_k <
 * warmup, or when sum q is zero or not finite: P_k = n_k / T and iw = 1.  Otherwise q_k = n_k sqrt(m2_k) and
 * P_k = (1 - uniform_prob) q_k / sum q + uniform_prob n_k / T.  The bin is the first k whose cumulative P exceeds u0 (fp64),
 * t_out[b] = lo_k + min(n_k - 1, floor(u1 n_k)) (device int64), iw_out[b] = n_k / (T P_k) (device fp32): E[iw f(t)] is the uniform mean.
 * (u0, u1) = draw[b][0..1] (device fp32 [B][2]) or, with draw NULL, Philox4x32-10(counter = (0, idx[b], step, 0x1a7e0000 + 5), key =
 * seed), words 0 and 1 as (r >> 8) 2^-24: a sixth stream in ldm_latent_batch's key layout, a function of (seed, step, dataset index)
 * alone.  idx: HOST [B] (NULL: 0 .. B-1), read before the call returns.  Refusals as above, plus uniform_prob outside [0, 1]. */
int ldm_timestep_resample(const float* tracker, int K, int T, int warmup, float uniform_prob, const int* idx, int B, uint64_t seed,
                          uint32_t step, const float* draw, int64_t* t_out, float* iw_out, void* stream);

/* ---- device-resident sampler: the scheduler step with its noise drawn inside the kernel (Philox4x32-10 keyed by a seed) and its
 *      coefficients / current timestep read from device memory, so that the loop body of 3d_ldm/inference.py:94-99 (UNet forward +
 *      scheduler.step) is one fixed launch sequence: ldm_unet_denoise_step replays it as ONE HIP graph in graph mode.
 *      coef_host: [n_steps][8] = {1/sqrt(abar_t), sqrt(1 - abar_t), c0, c1 | dir, sigma, t, sqrt(abar_t), 1/sqrt(1 - abar_t)} per
 *      step in sampling order; pred: the prediction type (0 epsilon, 1 sample, 2 v_prediction; ldm_scheduler_step). ---------------- */
typedef struct ldm_sampler ldm_sampler;
int ldm_sampler_create(const float* coef_host, int n_steps, int kind /* 0 DDPM, 1 DDIM */, int pred, int clip, uint64_t seed, ldm_sampler** out);
/* PNDM (MONAI's PNDMScheduler: Runge-Kutta warm-up + 4th-order linear multistep), row-programmed: coef_host = [n_steps][LDM_PNDM_ROW],
 * one row per UNet call in sampling order,
 *   {cx, ce, sqrt(abar_t), sqrt(1 - abar_t), flags, t, wm, w1, w2, w3, wacc, am, head, 0, 0, 0}
 *   e = wm m + w1 h1 + w2 h2 + w3 h3 + wacc acc (h_j: the j-th latest pushed model output; a zero weight is not read);
 *   acc := am m (LDM_PNDM_ACC_SET) | acc + am m (LDM_PNDM_ACC_ADD); xs = the saved sample (LDM_PNDM_USE_SAVED) or x;
 *   v_prediction (pred 2): e := sqrt(abar_t) e + sqrt(1 - abar_t) xs;  x := cx xs + ce e; then m is pushed (LDM_PNDM_PUSH) and the
 *   incoming x saved (LDM_PNDM_SAVE).  t: the UNet's timestep of the call; head: the pushes made by the rows before this one.
 * A row that reads state no earlier row wrote is refused.  pred: 0 epsilon or 2 v_prediction.  The multistep state (4 history slots,
 * the saved sample, the accumulator: n floats each) lives in a caller-owned device buffer of ldm_sampler_state_bytes(sp, n) bytes handed
 * over with ldm_sampler_bind_state; nothing is allocated on the step path, the buffer needs no zeroing, and ldm_sampler_reset rewinds
 * it with the step counter.  ldm_sampler_step / ldm_unet_denoise_step / ldm_unet_denoise_step_windows take such a sampler; without a
 * bound buffer of the step's size, or with a non-NULL x0_out (PNDM has no x0_hat), they return LDM_ERR_BAD_ARG and launch nothing. */
#define LDM_PNDM_ROW 16
#define LDM_PNDM_PUSH 1
#define LDM_PNDM_SAVE 2
#define LDM_PNDM_USE_SAVED 4
#define LDM_PNDM_ACC_SET 8
#define LDM_PNDM_ACC_ADD 16
int ldm_sampler_create_pndm(const float* coef_host, int n_steps, int pred, ldm_sampler** out);
/* Rectified flow (RFlowScheduler.step over its timesteps): coef_host = [n_steps][8] rows {dt, tau, 0, 0, 0, t, 0, 0} in sampling order,
 * dt = (t - t_next) / T, tau = t / T; a step is x := x + dt m with x0_hat = x + tau m (x0_out is allowed).  It draws nothing and keeps
 * no state: ldm_sampler_noise and ldm_sampler_bind_state return LDM_ERR_BAD_ARG for it; ldm_sampler_reset / step / destroy,
 * ldm_unet_denoise_step and ldm_unet_denoise_step_windows take it as they take the others. */
int ldm_sampler_create_rflow(const float* coef_host, int n_steps, ldm_sampler** out);
/* DPM-Solver++ (the 2M multistep solver in its data-prediction form; ODE and SDE variant), row-programmed: coef_host =
 * [n_steps][LDM_DPM_ROW], one row per UNet call in sampling order,
 *   {cx, c0, sqrt(abar_s), sqrt(1 - abar_s), flags, t, c1, cz, 1/sqrt(abar_s), clip_min, clip_max, 0, 0, 0, 0, 0}
 *   x0 = m (pred 1) | (x - sqrt(1 - abar_s) m) * (1/sqrt(abar_s)) (pred 0) | sqrt(abar_s) x - sqrt(1 - abar_s) m (pred 2), clamped to
 *   [clip_min, clip_max] with LDM_DPM_CLIP;  x := cx x + c0 x0 + c1 x0_prev (LDM_DPM_HAS_PREV) + cz z (LDM_DPM_DRAWS);  then x0 becomes
 *   the state.  t: the UNet's timestep of the call.  z: the sampler's Philox stream, counter = (element quad, row index), key = seed, so
 *   ldm_sampler_noise(sp, k) returns the z of row k; rows without LDM_DPM_DRAWS draw nothing.
 * Refused (LDM_ERR_BAD_ARG): a first row with LDM_DPM_HAS_PREV, a non-finite row, cz < 0, LDM_DPM_DRAWS set with cz == 0 (or cz != 0
 * without it), c1 != 0 without LDM_DPM_HAS_PREV, unknown flag bits.  The multistep state (the previous x0_hat, n floats) lives in a
 * caller-owned device buffer of ldm_sampler_state_bytes(sp, n) bytes handed over with ldm_sampler_bind_state; nothing is allocated on the
 * step path, the buffer needs no zeroing, and ldm_sampler_reset rewinds it with the step counter.  ldm_sampler_step (x0_out is allowed) /
 * ldm_unet_denoise_step / _guided / _windows / _windows_guided take such a sampler; without a bound buffer of the step's size they
 * return LDM_ERR_BAD_ARG and launch nothing.  ldm_sampler_seek with k0 > 0, ldm_sampler_start and ldm_sampler_create_repaint refuse
 * it: the row program assumes the history from row 0.  The windowed step blends the model outputs, then converts and clamps once per
 * element: the state holds the x0_hat of the blended full latent. */
#define LDM_DPM_ROW 16
#define LDM_DPM_HAS_PREV 1
#define LDM_DPM_DRAWS 2
#define LDM_DPM_CLIP 4
int ldm_sampler_create_dpm(const float* coef_host, int n_steps, int pred, uint64_t seed, ldm_sampler** out);
/* the host-driven DPM-Solver++ step: one row by value, the previous x0_hat and the draw as explicit pointers (NULL where the row does
 * not use them); x_out := the step, prev_x0_out and x0_out (each optional) := x0_hat (prev_x0_out may alias prev_x0_in).  Same
 * per-element arithmetic as the device sampler, bit for bit. */
int ldm_dpm_step(const float* m, const float* x, const float* prev_x0_in, const float* z, float* prev_x0_out, float* x_out, float* x0_out,
                 int64_t n, int pred, const float* row, void* stream);
size_t ldm_sampler_state_bytes(const ldm_sampler* sp, int64_t n);
int ldm_sampler_bind_state(ldm_sampler* sp, void* state, size_t bytes, int64_t n);
/* the host-driven PNDM step: one row by value, the state as explicit pointers (NULL where the row does not use it); prev := the step,
 * acc_out := the updated accumulator (may alias acc_in).  Same per-element arithmetic as the device sampler, bit for bit. */
int ldm_pndm_step(const float* m, const float* x, const float* h1, const float* h2, const float* h3, const float* saved,
                  const float* acc_in, float* acc_out, float* prev, int64_t n, int pred, const float* row, void* stream);
void ldm_sampler_destroy(ldm_sampler* sp);
int ldm_sampler_reset(ldm_sampler* sp, float* tbuf, int B, void* stream);
int ldm_sampler_step(ldm_sampler* sp, const float* eps, float* x, float* x0_out, int64_t n, float* tbuf, int B, void* stream);
int ldm_sampler_noise(const ldm_sampler* sp, int step, float* out, int64_t n, void* stream);
/* Warm starts (csrc/warm_start.h): a chain that begins at row k0 of the sampler's table from a given latent z0, not at row 0 from noise.
 * seek: ldm_sampler_reset at row k0: step counter := k0, tbuf[0..B) := t of row k0; 0 <= k0 < n_steps, and k0 = 0 only for a PNDM or DPM-Solver++
 *   sampler (its warm-up and history are defined from the first row).  The Philox step index of a stochastic step is the ROW index, so step k of
 *   a warm chain draws the same z as step k of the full chain (ldm_sampler_noise(sp, k)).  Ascending DDIM rows (DDIM inversion) need no
 *   entry of their own: ldm_sampler_create(kind 1) takes them and every step entry steps them.
 * start: x[b] = a z0[b or 0] + s e[b] for b < B, one pass, rounded as one multiply and one fused multiply-add (fma(a, z0, s e)).  DDPM /
 *   DDIM sampler: a = row[6] = sqrt(abar_t), s = row[1] = sqrt(1 - abar_t) of row k0; rectified flow: s = row[1] = tau, a = 1 - tau in
 *   fp32; PNDM and DPM-Solver++ are refused.  z0 is [z0_batch][per_sample] with z0_batch 1 (broadcast to the B members, no copy) or B; x [B][per_sample]
 *   may alias z0 only when z0_batch == B.  e = noise [B][per_sample], or with noise NULL Philox4x32-10 + Box-Muller with
 *      counter = (element / 4 within the sample: low word, high word, first_member + b, 0x57a27000), key = (seed low word, seed high word),
 *   lane e of a block being element 4 * (element / 4) + e: a draw depends on (seed, first_member + b, element) alone, so member k of an
 *   ensemble starts from the same draw however the members are chunked.  Counter word 3 keeps the stream apart from the sampler's
 *   (0x5eed) and from ldm_latent_batch's (0x1a7e0000 + 0 .. 4).
 * start_noise: the draws of global member `member`, [per_sample].
 * LDM_ERR_BAD_ARG with nothing launched: a NULL sampler / tensor (noise excepted), k0 outside 0 .. n_steps - 1, B outside 1 .. 65535,
 *   per_sample outside 1 .. 2^33, z0_batch other than 1 or B, x aliasing z0 with z0_batch == 1, x aliasing noise, a PNDM or
 *   DPM-Solver++ sampler (seek: k0 > 0). */
int ldm_sampler_seek(ldm_sampler* sp, int k0, float* tbuf, int B, void* stream);
int ldm_sampler_start(const ldm_sampler* sp, int k0, const float* z0, int z0_batch, const float* noise, float* x, int B, int64_t per_sample,
                      uint64_t seed, uint32_t first_member, void* stream);
int ldm_sampler_start_noise(uint64_t seed, uint32_t member, float* out, int64_t per_sample, void* stream);
/* Inpainting (csrc/repaint.h; RePaint, Lugmayr et al. 2022): a chain that keeps the trusted part of a latent and regenerates the rest.
 * create_repaint: coef_host = [n_rows][LDM_REPAINT_ROW] rows, one per UNet call in sampling order; the timesteps (slot 5) need not fall:
 *     [0..7]  the base scheduler's row, kind 0 DDPM / 1 DDIM as ldm_sampler_create takes it, kind 2 rectified flow as
 *             ldm_sampler_create_rflow does (pred / clip / seed of the base; a flow sampler ignores pred and clip)
 *     [8] ka [9] ks    the known region at the level the step arrives at is ka known + ks z_known (last level: 1, 0)
 *     [10] ja [11] js  the jump back from that level is ja x + js z_jump, applied only with the jump flag (no jump: 1, 0)
 *     [12] flags (1 = jump), [13..15] 0
 *   A step computes, per element i: xn = the base step (x0_out = its x0_hat); where keep[i % dhw] != 0, xn = fma(ka, known, ks z_known)
 *   (ks == 0: ka known, nothing drawn); with the jump flag, xn = fma(ja, xn, js z_jump) (js == 0: ja xn).  The step noise is the
 *   sampler's stream with the ROW index as its step (ldm_sampler_noise(sp, row)); z_known and z_jump are Philox4x32-10 + Box-Muller with
 *      counter = (element / 4: low word, high word, row, 0x4e9a1701 known | 0x4e9a1702 jump), key = (seed low word, seed high word).
 *   Refused: a non-finite row, a flags word other than 0 or 1, js != 0 without the jump flag, a negative ks or js (LDM_ERR_BAD_ARG);
 *   more than LDM_REPAINT_MAX_ROWS rows (LDM_ERR_UNSUPPORTED: the time-embedding table of ldm_unet_denoise_step has one row per call).
 * bind_known: known [known_batch][per_sample] (known_batch 1: one latent for every sample, no copy; else the step's sample count) and
 *   keep [dhw] fp32, nonzero = keep, shared by the per_sample / dhw channels and by the samples.  Caller-owned; both must outlive every step
 *   and every recorded graph replay that uses them.  Rebinding gives the sampler a new identity in the graph cache: no graph recorded on
 *   the old pointers is replayed.
 * repaint_noise: the draws of row `row` for n elements on the known stream (which 0) or the jump stream (which 1).
 * ldm_repaint_merge: the merge and the jump alone, host-driven on explicit draws: x, out [B][per_sample] (out may alias x), coef4_host =
 *   {ka, ks, ja, js} on the HOST, jump 0 | 1; z_known may be NULL when ks == 0, z_jump when there is no jump or js == 0.  The device
 *   step's arithmetic, bit for bit.
 * ldm_sampler_reset / seek / step / destroy, ldm_unet_denoise_step, _guided, _step_windows and _windows_guided take a repaint sampler;
 * ldm_sampler_start and ldm_sampler_bind_state refuse it.  A step on an unbound sampler, with n != samples * per_sample or with known_batch
 * neither 1 nor the sample count returns LDM_ERR_BAD_ARG and launches nothing (a windowed step has one sample: per_sample = C * voxels). */
#define LDM_REPAINT_ROW 16
#define LDM_REPAINT_MAX_ROWS 16384
int ldm_sampler_create_repaint(const float* coef_host, int n_rows, int kind, int pred, int clip, uint64_t seed, ldm_sampler** out);
int ldm_sampler_bind_known(ldm_sampler* sp, const float* known, int known_batch, const float* keep, int64_t per_sample, int64_t dhw);
int ldm_sampler_repaint_noise(const ldm_sampler* sp, int which, int row, float* out, int64_t n, void* stream);
int ldm_repaint_merge(const float* x, const float* known, int known_batch, const float* keep, const float* z_known, const float* z_jump,
                      float* out, int B, int64_t per_sample, int64_t dhw, const float* coef4_host, int jump, void* stream);
int ldm_unet_denoise_step(ldm_model* m, ldm_sampler* sp, float* x, int x_channels, const float* cond, int cond_channels,
                          float* tbuf, float* eps_scratch, int B, int D, int H, int W,
                          void* workspace, size_t workspace_bytes, void* stream);

/* ---- measurement-guided sampling (diffusion posterior sampling, Chung et al. 2023; csrc/guidance.h): every step is steered by the
 *      gradient of a loss on the model's own UNCLIPPED prediction of the clean latent, x0_hat = (x - s m) / a (epsilon) | m (sample) |
 *      a x - s m (v_prediction), a = sqrt(abar_t), s = sqrt(1 - abar_t).  The built-in measurement is a weighted pooled quadratic in
 *      latent space: r = weight .* (P x0_hat - target), P = the mean over non-overlapping pool^3 cubes per channel, L_b = 1/2 |r_b|^2,
 *      g = dL/dx0_hat = pool^-3 upsample_nearest(weight .* r), grad_x L = c_x g + J^T(c_m g) with (c_x, c_m) = (1/a, -s/a) | (0, 1) |
 *      (a, -s) and J^T the UNet's input VJP (ldm_unet_train_backward_input, data-only), and
 *      x_{t-1} = scheduler step(m, t, x_t) - zeta_b grad_x L_b,  zeta_b = scale / max(|r_b|, 1e-12) (normalize) or scale.
 *      target: fp32 [target_batch = 1 | B][C][D/pool][H/pool][W/pool]; weight: the same shape per sample, [weight_batch = 1 | B], >= 0,
 *      or NULL (= 1).  grad_out, gx, dx: caller-owned fp32 scratch [B][C][D][H][W]; norm2: [B], |r_b|^2 of the last step; norm_table:
 *      optional [n_steps][B], row k := |r_b| of the sampler's step k.  All of it stays on the device; the host reads nothing in a chain. */
typedef struct ldm_measurement {
    const float* target; int target_batch;
    const float* weight; int weight_batch;
    int pool; float scale; int normalize;
    float* grad_out; float* gx; float* dx; float* norm2; float* norm_table;
} ldm_measurement;
/* One guided step on a DDPM or DDIM sampler (anything else, a repaint sampler included: LDM_ERR_UNSUPPORTED), launch order: training
 * forward -> residual kernel -> data-only input backward -> ldm_sampler_step -> update kernel.  Everything is checked before anything
 * is launched; a sampler whose timesteps ascend (DDIM inversion) is refused too.  workspace: ldm_unet_train_input_workspace_bytes.
 * The step is not graph-replayed (the training plans never are). */
int ldm_unet_denoise_step_measured(ldm_model* m, ldm_sampler* sp, const ldm_measurement* g, float* x, int x_channels, const float* cond,
                                   int cond_channels, float* tbuf, float* eps_scratch, int B, int D, int H, int W,
                                   void* workspace, size_t workspace_bytes, void* stream);
/* The two kernels on their own (tests): the residual kernel with a and s by value -- grad_out := c_m g, gx := c_x g, norm2[b] := |r_b|^2,
 * a fixed-order reduction (no atomics: the same inputs give the same bits) -- and the update x -= zeta_b (gx + dx) in place. */
int ldm_op_guidance_residual(const float* x, const float* m, const float* target, int target_batch, const float* weight, int weight_batch,
                             float sqrt_abar, float sqrt_one_minus_abar, int pred, int pool, float* grad_out, float* gx, float* norm2,
                             int B, int C, int D, int H, int W, void* stream);
int ldm_op_guidance_update(float* x, const float* gx, const float* dx, const float* norm2, float scale, int normalize, int B, int64_t per_sample,
                           void* stream);

/* ---- AutoencoderKL.decode with gradients w.r.t. the latent (plan "dec_x"): the decoder half of the training plan (pack z ->
 *      post_quant_conv -> decoder), in that plan's arithmetic in both precision modes, with a DATA-ONLY backward: no column sums, weight
 *      gradients, exports or buckets, no parameter gradient written, nothing exchanged with other ranks.
 *      _forward: z [B][L][d][h][w] -> out [B][Cout][d f][h f][w f], f = 2^(levels - 1), keeping the tape in `workspace`, which must reach
 *      _backward untouched.  _backward: d_out (the shape of out) -> dz (the shape of z), every element overwritten.
 *      Checked before anything is launched: the handle's type, NULL tensors, B and dims >= 1, the workspace
 *      (ldm_vae_decode_grad_workspace_bytes).  _backward before any _forward at that shape: LDM_ERR_BAD_ARG.
 *      ldm_vae_train_*, ldm_vae_decode and ldm_vae_decode_workspace_bytes are unaffected. ------------------------------------------- */
size_t ldm_vae_decode_grad_workspace_bytes(ldm_model* m, int B, int d, int h, int w);
int ldm_vae_decode_grad_forward(ldm_model* m, const float* z, float* out, int B, int d, int h, int w,
                                void* workspace, size_t workspace_bytes, void* stream);
int ldm_vae_decode_grad_backward(ldm_model* m, const float* d_out, float* dz, int B, int d, int h, int w,
                                 void* workspace, size_t workspace_bytes, void* stream);

/* ---- image-space measurement guidance (csrc/guidance_image.h): the measurement above on the DECODED prediction.  With sf the
 *      inferer's scale_factor and Dec the AutoencoderKL decoder:
 *        z0 = x0_hat / sf;  y_hat = Dec(z0);  r = weight .* (P y_hat - target), P = the mean over non-overlapping pool^3 cubes of the
 *        image per image channel;  L_b = 1/2 |r_b|^2;  g_img = pool^-3 upsample_nearest(weight .* r);  dz = Dec'^T g_img;
 *        grad_x L = c_x (dz / sf) + J^T(c_m (dz / sf));  the step and zeta_b as above.
 *      target: fp32 [target_batch = 1 | B][Cimg][Di/pool][Hi/pool][Wi/pool] on the image dims (Di, Hi, Wi) = (D, H, W) * 2^(levels - 1);
 *      weight: the same shape per sample or NULL.  Caller-owned fp32 scratch: z0, dz, grad_out, gx, dx [B][C][D][H][W] (latent); recon
 *      [B][Cimg][Di][Hi][Wi] (the decoded prediction, overwritten in place by g_img); norm2 [B]; norm_table optional [n_steps][B];
 *      partials: ldm_image_residual_scratch_bytes(B, Cimg, Di, Hi, Wi, pool) bytes, 8-byte aligned; vae_workspace:
 *      ldm_vae_decode_grad_workspace_bytes.  inv_scale_factor = 1 / sf. */
typedef struct ldm_image_measurement {
    const float* target; int target_batch;
    const float* weight; int weight_batch;
    int pool; float scale; int normalize; float inv_scale_factor;
    float* z0; float* recon; float* dz; float* grad_out; float* gx; float* dx; float* norm2; float* norm_table; void* partials;
    void* vae_workspace; size_t vae_workspace_bytes;
} ldm_image_measurement;
/* One image-guided step, launch order: UNet training forward -> x0 kernel -> decoder grad-forward -> image residual and fold -> decoder
 * data-only backward -> chain kernel -> UNet data-only input backward -> ldm_sampler_step -> update kernel.  The refusals of
 * ldm_unet_denoise_step_measured; in addition `vae` must be an AutoencoderKL whose latent_channels equal x_channels, and the target and
 * weight shapes are checked against the image dims.  All plans of both models and both workspaces are readied before the first launch;
 * the host reads nothing.  workspace: ldm_unet_train_input_workspace_bytes.  Not graph-replayed. */
int ldm_unet_denoise_step_measured_image(ldm_model* unet, ldm_model* vae, ldm_sampler* sp, const ldm_image_measurement* g, float* x, int x_channels,
                                         const float* cond, int cond_channels, float* tbuf, float* eps_scratch, int B, int D, int H, int W,
                                         void* workspace, size_t workspace_bytes, void* stream);
/* The kernels on their own (tests), sqrt(abar_t) and sqrt(1 - abar_t) by value.  guidance_x0: z0 := x0_hat(x, m) * inv_scale_factor over n
 * elements.  image_residual: g_img := pool^-3 upsample_nearest(weight .* r) (g_img may alias y_hat), norm2[b] := |r_b|^2 on an image
 * [B][C][D][H][W]; many workgroups per sample, the chunk count a function of the shape alone, per-chunk partial sums in double folded in
 * index order by a second launch: no atomics, the same inputs give the same bits on any device, slot b does not depend on B.
 * guidance_chain: grad_out := c_m dz * inv_scale_factor, gx := c_x dz * inv_scale_factor.  LDM_ERR_BAD_ARG with nothing launched: a NULL
 * tensor, an unknown pred, sqrt_abar <= 0, a pool outside [1, 1024] or not dividing the dims, a batch count that is neither 1 nor B;
 * LDM_ERR_WORKSPACE: partials smaller than ldm_image_residual_scratch_bytes (which is 0 for a refused shape) or not 8-byte aligned. */
size_t ldm_image_residual_scratch_bytes(int B, int C, int D, int H, int W, int pool);
int ldm_op_guidance_x0(const float* x, const float* m, float sqrt_abar, float sqrt_one_minus_abar, int pred, float inv_scale_factor, float* z0,
                       int64_t n, void* stream);
int ldm_op_image_residual(const float* y_hat, const float* target, int target_batch, const float* weight, int weight_batch, int pool,
                          float* g_img, float* norm2, void* partials, size_t partials_bytes, int B, int C, int D, int H, int W, void* stream);
int ldm_op_guidance_chain(const float* dz, float sqrt_abar, float sqrt_one_minus_abar, int pred, float inv_scale_factor, float* grad_out, float* gx,
                          int64_t n, void* stream);

/* ---- likelihood of a GIVEN latent x0 under a DDPM (MONAI >= 1.4 DiffusionInferer.get_likelihood, restated; csrc/likelihood.h): per
 *      timestep the KL between q(x_{t-1} | x_t, x0) and the model's p(x_{t-1} | x_t), at t = 0 the discretised decoder term, averaged per
 *      sample and summed into total[b] (nats per dimension).  One noise tensor z serves every timestep.  Fixed variance only.
 *      coef_host: [n_steps][LDM_LIK_ROW] fp32 rows in scheduler.timesteps order,
 *        {sqrt(abar_t), sqrt(1 - abar_t), 1/sqrt(abar_t), c0, 1/var, t, 1/sqrt(var), c1, 0 ...}
 *      (c0, c1: the posterior-mean coefficients of x0 and x_t; var: the step's variance); the row with t == 0 scores the decoder term
 *      with bin_width = (scaled range) / (original range).  pred: 0 epsilon, 1 sample, 2 v_prediction; clip: clamp x0_hat to [-1, 1].
 *      Tensors are fp32 device [B][per_sample]; per_sample = C D H W.  Deterministic: per-workgroup partial sums in double, laid out
 *      per sample and folded in a fixed order by a second launch; slot b's results do not depend on B.  scratch: at least
 *      ldm_likelihood_scratch_bytes(B, per_sample) bytes, 8-byte aligned.  LDM_ERR_BAD_ARG with nothing launched: a NULL tensor, B < 1,
 *      an unknown pred, bin_width <= 0, a step past the last row. ---------------------------------------------------------------- */
#define LDM_LIK_ROW 16
typedef struct ldm_likelihood ldm_likelihood;
int ldm_likelihood_create(const float* coef_host, int n_steps, int pred, int clip, uint64_t seed, float bin_width, ldm_likelihood** out);
void ldm_likelihood_destroy(ldm_likelihood* lk);
size_t ldm_likelihood_scratch_bytes(int B, int64_t per_sample);
/* counter := 0, total[0..B) := 0, x_t := row 0's noising of x0 with z = noise (NULL: Philox4x32-10 keyed by the seed, counter =
 * (sample b's quad, step 0) of the sampler's stream: a function of (seed, per_sample, b, element), not of B), tbuf[0..B) := t of row 0.
 * The handle keeps `noise` for the steps that follow. */
int ldm_likelihood_reset(ldm_likelihood* lk, const float* x0, const float* noise, float* x_t, float* tbuf, int B, int64_t per_sample,
                         float* total, void* stream);
/* the Philox z as a tensor */
int ldm_likelihood_noise(const ldm_likelihood* lk, float* out, int B, int64_t per_sample, void* stream);
/* The two host-driven halves, one row by value, the device loop's arithmetic bit for bit: x_t = row[0] x0 + row[1] noise (both
 * products rounded, then the sum); and the terms of (x0, x_t, m): kl_map (optional) per element, term_out[b] (optional) = the sample's
 * mean, total[b] += that mean. */
int ldm_likelihood_noisy(const float* x0, const float* noise, const float* row, float* x_t, int B, int64_t per_sample, void* stream);
int ldm_likelihood_term(const float* x0, const float* x_t, const float* m, const float* row, int pred, int clip, float bin_width,
                        float* kl_map, float* term_out, float* total, int B, int64_t per_sample, void* scratch, size_t scratch_bytes,
                        void* stream);
/* One whole step on the row the device counter points at: m = UNet(x_t | cond, tbuf) into m_scratch, the term kernel (kl_map optional;
 * x_t := the NEXT row's noising, in place), the finalize kernel (total[b] += mean; terms [n_steps][B] optional; counter and tbuf
 * advance).  Graph mode: ONE graph launch per step, keyed by the handle's never-reused id and every pointer. */
int ldm_unet_likelihood_step(ldm_model* m, ldm_likelihood* lk, const float* x0, float* x_t, int x_channels, const float* cond, int cond_channels,
                             float* tbuf, float* m_scratch, float* kl_map, float* terms, float* total, int B, int D, int H, int W,
                             void* scratch, size_t scratch_bytes, void* workspace, size_t workspace_bytes, void* stream);
/* y [N][C][D][H][W] = nearest-neighbour resize of x [N][C][d][h][w] (fp32 device), any sizes, PyTorch's rule
 * (F.interpolate(mode="nearest")): src = min(floor(dst * (float)in / out), in - 1) per axis, the scale in fp32. */
int ldm_op_resize_nearest(const float* x, float* y, int N, int C, int d, int h, int w, int D, int H, int W, void* stream);

/* ---- ensemble statistics: the per-voxel mean and spread of K member volumes (K draws of one scan's posterior) without holding the K
 *      volumes (csrc/ensemble.h).  The state is two fp32 device arrays of n elements, mean and m2 (the sum of squared deviations from
 *      the running mean), plus a member count that the caller keeps.  Welford's recurrence per element, members in order:
 *        c += 1;  d = x - mean;  mean += d / c;  m2 += d * (x - mean)
 *      every operation rounded on its own, so the state's bits do not depend on how the members are split over calls.  Non-finite
 *      members make that voxel's mean / m2 / std, and then the scalars, non-finite: nothing is masked. ------------------------------- */
/* Folds members[b][0 .. n), b = 0 .. B-1 (member b at members + b * member_stride, member_stride >= n) into (mean, m2) holding `count`
 * members.  count == 0: the state's contents are ignored (it needs no zeroing) and the first member sets mean = x, m2 = 0.  16-byte
 * accesses where all three pointers are 16-byte aligned and member_stride % 4 == 0.  LDM_ERR_BAD_ARG with nothing launched: a NULL
 * pointer, B < 1, n < 1, count < 0, count + B past INT_MAX, member_stride < n, the members range overlapping mean or m2. */
int ldm_ensemble_update(const float* members, int B, int64_t member_stride, int64_t n, float* mean, float* m2, int count, void* stream);
/* bytes of ldm_ensemble_finalize's scratch for n elements (0 with the error set for n < 1) */
size_t ldm_ensemble_stats_scratch_bytes(int64_t n);
/* var = max(m2, 0) / (count - ddof); std_out (optional, n floats) = sqrt(var); stats (device, LDM_ENS_STATS floats) =
 * {mean of std, max of std, mean of var, bias_sq = mean((mean - target)^2) or 0 where target is NULL, 0, 0, 0, 0}.  Per-workgroup
 * partial sums in double in `scratch` (8-byte aligned), folded in a fixed order by a second launch: bit-identical run to run.
 * LDM_ERR_BAD_ARG with nothing launched: a NULL mean / m2 / stats / scratch, n < 1, ddof outside {0, 1}, count - ddof < 1, scratch
 * smaller than ldm_ensemble_stats_scratch_bytes(n), std_out overlapping an input. */
#define LDM_ENS_STATS 8
int ldm_ensemble_finalize(const float* mean, const float* m2, int count, int ddof, const float* target, float* std_out, float* stats,
                          void* scratch, size_t scratch_bytes, int64_t n, void* stream);

/* ---- sliding-window sampling of a latent larger than the trained window (one volume, fp32 [C][D][H][W]): the grid of overlapping
 *      windows (MONAI dense_patch_slices starts, separable importance map normalised per axis: the host builds the tables, sliding.py),
 *      window gather / blend, and one whole windowed denoising step: the UNet on the windows in chunks of `chunk`, then blend + scheduler
 *      step + write-back of the new x into the windows in one kernel; in graph mode the whole step is one graph launch.
 *      dims, roi, n: [3]; starts: n[0] + n[1] + n[2] ints; weights: n[a] * roi[a] floats per axis; cover: {first, count} per position. */
typedef struct ldm_window_grid ldm_window_grid;
int ldm_window_grid_create(const int* dims, const int* roi, const int* n, const int* starts, const float* weights, const int* cover,
                           ldm_window_grid** out);
void ldm_window_grid_destroy(ldm_window_grid* grid);
int ldm_window_gather(const ldm_window_grid* grid, const float* src, float* dst, int C, void* stream);
int ldm_window_blend(const ldm_window_grid* grid, const float* src, float* dst, int C, void* stream);
int ldm_unet_denoise_step_windows(ldm_model* m, ldm_sampler* sp, const ldm_window_grid* grid, float* x, int x_channels,
                                  const float* cond_w, int cond_channels, float* xw, float* eps_w, float* tbuf, int chunk,
                                  void* workspace, size_t workspace_bytes, void* stream);

/* ---- classifier-free guidance for concat conditioning (MONAI >= 1.5: cfg / cfg_fill_value of DiffusionInferer.sample and
 *      LatentDiffusionInferer.sample, restated): the UNet runs once on a doubled batch, the unconditional half FIRST (its condition
 *      channels hold `fill`, MONAI's default -1), the conditional half second, and the scheduler receives u + w (c - u).  New entries:
 *      the unguided ones above, their plans and their recorded graphs are untouched. ------------------------------------------------ */
/* out[i] = u[i] + w (c[i] - u[i]) over n fp32 device elements: the difference rounded once, then one fused multiply-add (w = 0 gives
 * u, w = 1 gives c up to that rounding).  out may alias u, not c. */
int ldm_guidance_combine(const float* u, const float* c, float w, float* out, int64_t n, void* stream);
/* Workspace of the two guided entries below for B samples (or chunks of B windows) of D x H x W: the guided plan at batch 2 B plus
 * room for one doubled output [2 B][out][DHW], which the windowed entry uses.  0 with the error set on a bad argument. */
size_t ldm_unet_guided_workspace_bytes(ldm_model* m, int B, int D, int H, int W);
/* ldm_unet_denoise_step under guidance, from the caller's B-sample x and cond (no doubled fp32 tensor is built): the guided plan at
 * batch 2 B (samples 0 .. B-1 see (x | fill), samples B .. 2B-1 see (x | cond); fill is rounded as a condition tensor holding it would
 * be) into eps_scratch [2 B][out][DHW], the combine in place on its first half, then ldm_sampler_step on that half with n = B out DHW.
 * Every sampler kind is taken; a PNDM sampler's state is bound for the B samples and its history holds guided outputs.  tbuf has 2 B
 * entries (ldm_sampler_reset(sp, tbuf, 2 B)); the sampler publishes the next t to all of them.  cond NULL or cond_channels 0:
 * LDM_ERR_BAD_ARG with nothing launched.  Graph mode: the whole step is ONE graph launch; w and fill are part of the replay key. */
int ldm_unet_denoise_step_guided(ldm_model* m, ldm_sampler* sp, float* x, int x_channels, const float* cond, int cond_channels,
                                 float w, float fill, float* tbuf, float* eps_scratch, int B, int D, int H, int W,
                                 void* workspace, size_t workspace_bytes, void* stream);
/* ldm_unet_denoise_step_windows under guidance: each chunk of nb windows runs the guided plan at 2 nb from xw / cond_w, the combine
 * writes eps_w window by window, and the blend-step kernels run unchanged.  tbuf: at least 2 chunk entries; workspace: at least
 * ldm_unet_guided_workspace_bytes(m, chunk, roi).  Graph mode: ONE graph launch per step. */
int ldm_unet_denoise_step_windows_guided(ldm_model* m, ldm_sampler* sp, const ldm_window_grid* grid, float* x, int x_channels,
                                         const float* cond_w, int cond_channels, float w, float fill, float* xw, float* eps_w, float* tbuf,
                                         int chunk, void* workspace, size_t workspace_bytes, void* stream);
/* Condition dropout, the training side of guidance: slot b of cond [B][per_sample] (device fp32) is overwritten with `fill` where the
 * decision says so.  mask_in (HOST [B], non-zero = drop) wins if given; otherwise slot b drops iff u < p,
 *   Philox4x32-10(counter = (0, idx[b], step, 0x1a7e0000 + 4), key = seed),  u = (word 0 >> 8) 2^-24:
 * a fifth stream in ldm_latent_batch's key layout, so a decision depends on (seed, step, dataset index) alone, never on the batch slot
 * or B.  idx: HOST [B] (NULL: 0 .. B-1).  The decisions are taken on the host and passed to the kernel by value; mask_out_host
 * (optional, HOST [B]) receives them.  p = 0 drops nothing and launches nothing, p = 1 drops all.  LDM_ERR_BAD_ARG with nothing
 * launched: B outside 1 .. 64, p outside [0, 1], NULL cond, per_sample < 1, a negative index. */
int ldm_cond_dropout(float* cond, int B, int64_t per_sample, const int* idx, float p, float fill, const unsigned char* mask_in,
                     uint64_t seed, uint32_t step, unsigned char* mask_out_host, void* stream);

/* ---- operator level: the kernels the plans are made of, on the library's internal layout (NDHWC bf16 device
 *      tensors, C % 32 == 0).  They replace torch.nn.functional.conv3d / group_norm+silu / softmax-attention as
 *      MONAI's blocks call them and exist for per-kernel parity tests and micro-benchmarks.
 *      conv3d: out[m][co] = sum_tap sum_ci w[tap][co][ci] * cat(xa,xb)[voxel(m,tap)][ci]  (+ optional fused 1x1
 *      conv over cat(x1a,x1b) with w1) + bias + bias2 + temb[n][co] + residual[m][co].  w: [k^3][cout_pad][ca+cb]
 *      bf16, cout_pad % 64 == 0.  stride 2 with pad 0 means F.pad(x,(0,1)*3) then stride-2 conv (AEKLDownsample).
 *      ups = 1 folds a nearest x2 upsample of the input into the loader.  Exactly one of out_bf16 ([M][rup32(cout)])
 *      / out_f32 (NCDHW [N][cout][DHW]) is written.  wgn in {0 auto,1,2,4} picks the tile (BN = 64*wgn), splitk 0 =
 *      auto; scratch holds the fp32 split-K slabs (splitk * M * cout_pad * 4 bytes). ------------------------------ */
int ldm_op_conv3d(const void* xa, int ca, const void* xb, int cb, const void* w, const float* bias,
                  const void* x1a, int c1a, const void* x1b, int c1b, const void* w1, const float* bias2,
                  const float* temb, int temb_stride, const void* residual, void* out_bf16, float* out_f32,
                  int N, int Din, int Hin, int Win, int ksize, int stride, int pad, int ups,
                  int cout, int cout_pad, int wgn, int splitk, void* scratch, size_t scratch_bytes, void* stream);
/* ---- training building blocks (backward of train_diffusion.py:207-219) ----------------
 *      data gradient of a conv = ldm_op_conv3d on dY with flipped + transposed weights (ldm_op_weight_flip_transpose),
 *      pad' = k-1-pad; for a stride-2 forward conv pass ups = 2 (zero-insertion upsample: odd tap positions read 0). */
/*      the same 3^3 stride-1 pad-1 convolution for 64 OUTPUT channels over a large grid (the AutoencoderKL's full-resolution ResBlocks:
 *      3d_ldm/train_autoencoder.py:139-148 construction; Encoder / Decoder blocks at num_channels[0] = 64), conv3_block_kernel: one
 *      (4, th, 16) block of output voxels per workgroup, its input halo copied into LDS once per 32 input channels.  x [N][D][H][W][cin],
 *      w packed [27][64][cin], out [N*D*H*W][64]; stats (optional) [N * rows][64][2], rows = ldm_op_conv3d_block_stats_rows; th = 8 | 4. */
int ldm_op_conv3d_block_stats_rows(int D, int H, int W, int th);
/*      the same for 128 OUTPUT channels (conv3_block128_kernel: eight waves per workgroup, double-buffered halo chunks; the AutoencoderKL's
 *      half-resolution ResBlocks at num_channels[1] = 128): w packed [27][128][cin], out / residual [N*D*H*W][128],
 *      stats [N * ldm_op_conv3d_block_stats_rows(D, H, W, 8)][128][2]. */
int ldm_op_conv3d_block128(const void* x, int cin, const void* w, const float* bias, const float* temb, int temb_stride, const void* residual,
                           void* out, float* stats, int N, int D, int H, int W, void* stream);
/* tests only, experiments builds (make EXTRA=-DLDM_EXPERIMENTS): number of workgroups of conv3_block_kernel's tile loop (0 = default: two per
 * CU; a multiple of 8); returns the previous value.  The product library has no tile-loop form: returns -1. */
int ldm_debug_conv_block_slots(int slots);
int ldm_op_conv3d_block(const void* x, int cin, const void* w, const float* bias, const float* temb, int temb_stride, const void* residual,
                        void* out, float* stats, int N, int D, int H, int W, int th, void* stream);
int ldm_op_weight_flip_transpose(const void* w, void* wt, int ksize, int cout, int cout_pad, int cin, void* stream);
/*      weight gradient: dw[tap][co][ci] (fp32) = sum_m dy[m][co] * x[src(m, tap)][ci]; deterministic (no atomics).
 *      ksplit > 1 splits the voxel range over workgroups: dw = ksplit partial matrices [ksplit][k^3][cout][cin] to sum. */
int ldm_op_conv3d_wgrad(const void* dy, int cdy, const void* x, int cx, float* dw, int cout, int cin,
                        int N, int Din, int Hin, int Win, int ksize, int stride, int pad, int ups, int ksplit, void* stream);
/*      thin data gradient of a 3^3 stride-1 pad-1 conv with cin_real = cx + cc <= 32 input channels (the UNet's conv_in):
 *      dy [N*D*H*W][cdy] bf16 (fp32_mode: fp32, computed as the 3 x bf16 product), w the conv's own fp32 [cout][cin_real][3][3][3];
 *      rows [0, cx) -> dx fp32 [N][cx][DHW], rows [cx, cx + cc) -> dcond fp32 [N][cc][DHW]; either destination may be NULL.
 *      Packs the weights as the backward plans do, launches conv3_dgrad_thin_kernel and synchronises (it owns a temporary buffer). */
int ldm_op_conv3d_dgrad_thin(const void* dy, int cdy, const float* w, int cout, int cin_real, int cx, int cc, float* dx, float* dcond,
                             int N, int D, int H, int W, int fp32_mode, void* stream);
/*      its two halves on caller-owned memory, nothing allocated or synchronised (timing): the re-pack into wp (27 * 32 * K bf16,
 *      K = cdy, fp32_mode: 3 cdy) and the kernel alone on packed weights (fp32_mode: dy is the (hi | lo) bf16 split [M][2 cdy]). */
int ldm_op_conv3d_dgrad_thin_pack(const float* w, int cdy, int cout, int cin_real, int fp32_mode, void* wp, void* stream);
int ldm_op_conv3d_dgrad_thin_packed(const void* dy, int cdy, const void* wp, int cx, int cc, float* dx, float* dcond,
                                    int N, int D, int H, int W, int fp32_mode, void* stream);
/*      backward of y = act(GroupNorm(cat(xa, xb))): dxa, dxb (bf16 NDHWC, plus acc_a / acc_b when given), dgamma, dbeta (fp32). */
size_t ldm_op_group_norm_bwd_scratch_bytes(int N, int C, int DHW, int groups);
int ldm_op_group_norm_bwd(const void* dy, const void* xa, int ca, const void* xb, int cb, const float* gamma, const float* beta,
                          int groups, float eps, int silu, const void* acc_a, const void* acc_b, void* dxa, void* dxb,
                          float* dgamma, float* dbeta, int N, int DHW, void* scratch, size_t scratch_bytes, void* stream);
/* GroupNorm(groups, eps, affine) over cat(xa, xb), optional fused SiLU -> out [N*DHW][ca+cb] bf16. */
/* ---- data path (3d_ldm/utils.py:94-107): ScaleIntensityRangePercentiles per volume on the device (exact order statistics by radix
 *      select, numpy "linear" interpolation); x / out: B volumes of n fp32 values ------------------------------------------------ */
size_t ldm_op_scale_intensity_percentiles_scratch_bytes(int B);
int ldm_op_scale_intensity_percentiles(const float* x, float* out, int B, int64_t n, float lower, float upper, float b_min, float b_max,
                                       void* scratch, size_t scratch_bytes, void* stream);
/* ---- image-quality metrics of a prediction x against a target y (extension; MONAI `SSIMMetric` / `PSNRMetric` / `MAEMetric` semantics,
 *      [MONAI-ext]: the reference reports none, a low-count -> high-count PET paper reports these).  One pass over two fp32 volumes
 *      [B, C, D, H, W]; x_strides / y_strides: HOST arrays of the five element strides (B, C, D, H, W; W must be 1, so a cropped view of
 *      a padded buffer is scored in place).  weights: HOST array of the `win` normalised 1-D window weights (win odd, 3..11; the window
 *      is separable and the map is valid-mode, (D-win+1) x (H-win+1) x (W-win+1)); c1 = (k1 data_range)^2, c2 = (k2 data_range)^2.
 *      out [B][8] fp32 on the device: ssim (mean over C and the map), psnr = 20 log10(data_range) - 10 log10(mse), mse, mae (means over
 *      C D H W), nrmse = sqrt(sum (x-y)^2 / sum y^2), min(y), max(y), 0.  ssim_map (optional): [B][C][D-win+1][H-win+1][W-win+1].
 *      Deterministic (no atomics: per-workgroup partials in scratch, folded in a fixed order), no allocation, no synchronisation. */
size_t ldm_op_image_metrics_scratch_bytes(int B, int C, int D, int H, int W, int win);
int ldm_op_image_metrics(const float* x, const int64_t* x_strides, const float* y, const int64_t* y_strides, int B, int C, int D, int H, int W,
                         const float* weights, int win, float data_range, float k1, float k2, float* out, float* ssim_map,
                         void* scratch, size_t scratch_bytes, void* stream);
/* ---- PatchDiscriminator building blocks (stage-1 GAN tail, 3d_ldm/train_autoencoder.py:150-158,407-424,454-494): 4^3 strided convs as
 *      im2col + the 1x1 GEMM kernels (forward, data gradient through col2im, weight gradient through ldm_op_conv3d_wgrad with ksize 1);
 *      InstanceNorm + LeakyReLU(0.2) = ldm_op_group_norm(_bwd) with groups = C and activation code 2 (0 none, 1 SiLU, 2 LeakyReLU 0.2). */
int ldm_op_im2col(const void* x, void* col, int N, int D, int H, int W, int Cs, int C, int k, int stride, int pad, int Kp, void* stream);
int ldm_op_col2im(const void* dcol, void* dx, int N, int D, int H, int W, int Cs, int C, int k, int stride, int pad, int Kp, void* stream);
int ldm_op_leaky_relu(const void* x, void* y, int64_t n, float slope, void* stream);
int ldm_op_leaky_relu_bwd(const void* x, const void* dy, void* dx, int64_t n, float slope, void* stream);
int ldm_op_pack_ncdhw(const float* x, void* out_bf16_ndhwc, int N, int C, int Cs, int64_t DHW, void* stream);
int ldm_op_unpack_ndhwc(const void* act_bf16_ndhwc, float* out, int N, int C, int Cs, int64_t DHW, void* stream);
/* The same PatchDiscriminator building blocks on fp32 NDHWC tensors: the reference trains the discriminator in fp32 when AMP is off
 * (3d_ldm/train_autoencoder.py:150-158 construction, :454-494 discriminator step); `--precision fp32` selects them
 * (ldm3d/discriminator.py).  Exact fp32 MFMA (csrc/f32_path.h, f32_train.h).  K / stored channels are multiples of 16, weight
 * matrices have cout_pad % 64 == 0 rows (rows >= cout zero), bias cout_pad entries.
 *   gemm_f32:        out[M][couts] = x[M][K] w[cout_pad][K]^T + bias          (couts % 4 == 0, cout <= couts <= cout_pad)
 *   gemm_wgrad_f32:  dw[ksplit][cout][K] = partial sums over row ranges of dy[M][cdy]^T x[M][K]
 *   group_norm_f32 / _bwd_f32: y = act(GroupNorm(x)) with act 0 none, 1 SiLU, 2 LeakyReLU(0.2) (InstanceNorm: groups = C), and its
 *                    backward (dx, dgamma, dbeta summed over the batch); scratch from ldm_op_group_norm_f32_scratch_bytes. */
int ldm_op_pack_ncdhw_f32(const float* x, float* out_f32_ndhwc, int N, int C, int Cs, int64_t DHW, void* stream);
int ldm_op_unpack_ndhwc_f32(const float* act_f32_ndhwc, float* out, int N, int C, int Cs, int64_t DHW, void* stream);
int ldm_op_im2col_f32(const float* x, float* col, int N, int D, int H, int W, int Cs, int C, int k, int stride, int pad, int Kp, void* stream);
int ldm_op_col2im_f32(const float* dcol, float* dx, int N, int D, int H, int W, int Cs, int C, int k, int stride, int pad, int Kp, void* stream);
int ldm_op_leaky_relu_f32(const float* x, float* y, int64_t n, float slope, void* stream);
int ldm_op_leaky_relu_bwd_f32(const float* x, const float* dy, float* dx, int64_t n, float slope, void* stream);
int ldm_op_gemm_f32(const float* x, int K, const float* w, const float* bias, float* out, int64_t M, int cout, int cout_pad, int couts, void* stream);
int ldm_op_gemm_wgrad_f32(const float* dy, int cdy, const float* x, int K, float* dw, int cout, int64_t M, int ksplit, void* stream);
/* The 1x1x1 convolutions of the fp32 inference plans (SABlock's q|k|v and output projections, the ResBlock's nin_shortcut; SURVEY.md
 * section 8a row a2.3) as one launch on fp32 operands: out[M][couts] = (xa | xb)[M][ca + cb] w[cout_pad][ca + cb]^T + bias (+ residual),
 * every product as three bf16 MFMAs on hi / lo splits made in registers (csrc/gemm_light_x3.h; ~1e-5 relative).  ca, cb % 32 == 0
 * (cb = 0: one source), cout_pad, couts % 32 == 0.  stats (optional): [ceil(M / rows)][couts][2] per-tile (sum, sum of squares), rows = 64
 * when big else 32; big = -1: the planner's choice. */
int ldm_op_linear_f32x3(const float* xa, int ca, const float* xb, int cb, const float* w, const float* bias, const float* residual, float* out,
                        float* stats, int64_t M, int cout_pad, int couts, int big, void* stream);
/* The 1x1x1 convolutions of the bf16 plans (SABlock's q|k|v and output projections, the im2col first conv) as one launch:
 * out[M][couts] = (xa | xb)[M][ca + cb] w[cout_pad][ca + cb]^T + bias (+ residual) on bf16 operands, fp32 accumulation, bf16 store.  ca, cb % 32
 * == 0 (cb = 0: one source), cout_pad, couts % 32 == 0.  stats (optional): [ceil(M / rows)][couts][2] per-tile (sum, sum of squares) of the
 * stored values, rows = 64 when big else 32; big = -1: the planner's choice.  kernel: 0 = gemm_light_kernel (csrc/gemm_light.h), 1 =
 * gemm_wg_kernel (csrc/gemm_wg.h: operand tiles shared in LDS; one source, K = 128 .. 512 in steps of 128), -1 = the planner's choice
 * (knob LDM_GEMM_WG).  The two kernels give the same bits.
 * gn_slabs (optional): the attention blocks' GroupNorm (gamma, beta, groups, eps; no activation) of xa in front of the GEMM, from the
 * [samples * gn_nrb][K][2] partial (sum, sum of squares) rows xa's producer left; gn_dhw = rows per sample.  fold 0: the one-launch
 * GroupNorm into scratch ([M][K] bf16), then the GEMM; fold 1: inside gemm_wg_kernel (K >= 256, gn_nrb <= 16), nothing written but out.
 * Same bits either way. */
int ldm_op_linear_bf16(const void* xa, int ca, const void* xb, int cb, const void* w, const float* bias, const void* residual, void* out,
                       float* stats, int64_t M, int cout_pad, int couts, int big, int kernel,
                       const float* gn_slabs, int gn_nrb, int gn_dhw, const float* gamma, const float* beta, int groups, float eps, int fold,
                       void* scratch, void* stream);
size_t ldm_op_group_norm_f32_scratch_bytes(int N, int C, int DHW, int groups);
int ldm_op_group_norm_f32(const float* x, int C, const float* gamma, const float* beta, int groups, float eps, int act, float* out,
                          int N, int DHW, void* scratch, size_t scratch_bytes, void* stream);
int ldm_op_group_norm_bwd_f32(const float* dy, const float* x, int C, const float* gamma, const float* beta, int groups, float eps, int act,
                              float* dx, float* dgamma, float* dbeta, int N, int DHW, void* scratch, size_t scratch_bytes, void* stream);
/* The convolution, weight-gradient, attention, GroupNorm-backward and upsample-backward kernels of the fp32 plans (csrc/f32_path.h,
 * f32_train.h), launched by the same helpers the plan executor uses; fp32 NDHWC tensors throughout.
 *   conv3d_f32:  out[m][co] = sum_tap sum_ci w[tap][co][ci] cat(xa, xb)[voxel(m, tap)][ci] + bias + temb[n] + residual[m]: the addressing
 *                of ldm_op_conv3d (ksize 1|3, stride 1|2, ups 0|1|2 with 2 = zero insertion).  w [k^3][cout_pad][ca + cb]; bias, temb
 *                rows: cout_pad entries; form 0 = exact fp32 MFMA (ca, cb % 16 == 0), 1 = 3 x bf16 (ca, cb % 32 == 0).  Exactly one of out
 *                ([M][couts], cout <= couts <= cout_pad, couts % 4 == 0) / out_ncdhw ([N][cout][DHW], no residual).  bn 0|64|128 and splitk
 *                0..64 (0 = the planner's rule; normalised so that no split is empty); scratch: splitk * M * cout_pad floats.  stats
 *                (splitk >= 2): [N * nrb][couts][2] (sum, sum of squares) of the stored values over the row blocks of
 *                ldm_op_conv3d_f32_stats_blocks (returns nrb; *rows = rows per block).
 *   weight_flip_transpose_f32: wt[tap'][ci][co] = w[taps-1-tap'][co][ci_off + ci], wt [k^3][round64(ci_cnt)][round32(cout)].
 *   conv3d_wgrad_f32: ksplit slabs [k^3][cout][dw_ld] of dW, this source's columns at dw_ci_off.
 *   attention_f32 / _bwd_f32: head_dim 32|64|128|256, lse [B][C/head_dim][N], x3 = 3 x bf16 products (split kernel at head_dim 64).
 *   group_norm_bwd2_f32: two sources, acc_a / acc_b added to dxa / dxb, dgamma / dbeta summed over the batch.
 *   upsample_bwd_f32: adjoint of the nearest x2 upsample; D, H, W = source size. */
int ldm_op_conv3d_f32_stats_blocks(int N, int dhwo, int couts, int* rows);
int ldm_op_conv3d_f32(const float* xa, int ca, const float* xb, int cb, const float* w, const float* bias, const float* temb, int temb_stride,
                      const float* residual, float* out, int couts, float* out_ncdhw, float* stats, int N, int Din, int Hin, int Win,
                      int ksize, int stride, int pad, int ups, int cout, int cout_pad, int form, int bn, int splitk,
                      void* scratch, size_t scratch_bytes, void* stream);
size_t ldm_op_weight_flip_transpose_f32_ws_bytes(int ksize, int cout, int ci_cnt);
int ldm_op_weight_flip_transpose_f32(const float* w, float* wt, int ksize, int cout, int cout_pad, int cin, int ci_off, int ci_cnt,
                                     void* desc_ws, size_t desc_ws_bytes, void* stream);
int ldm_op_conv3d_wgrad_f32(const float* dy, int cdy, const float* x, int cx, float* dw, int cout, int cin, int dw_ld, int dw_ci_off,
                            int N, int Din, int Hin, int Win, int ksize, int stride, int pad, int ups, int ksplit, void* stream);
int ldm_op_attention_f32(const float* qkv, float* out, float* lse, int B, int N, int C, int head_dim, int x3, void* stream);
int ldm_op_attention_bwd_f32(const float* qkv, const float* o, const float* d_o, const float* lse, float* delta_scratch, float* dqkv,
                             int B, int N, int C, int head_dim, void* stream);
int ldm_op_group_norm_bwd2_f32(const float* dy, const float* xa, int ca, const float* xb, int cb, const float* gamma, const float* beta,
                               int groups, float eps, int act, const float* acc_a, const float* acc_b, float* dxa, float* dxb,
                               float* dgamma, float* dbeta, int N, int DHW, void* scratch, size_t scratch_bytes, void* stream);
int ldm_op_upsample_bwd_f32(const float* dy, float* dx, int N, int D, int H, int W, int C, void* stream);
/* The kernels of the bf16 training plans (OP_GNB, OP_COLSUM(_BATCH), OP_EXPORT(_BATCH), OP_WT_BATCH, OP_LIN_DX / _DW, OP_SUMPOOL, OP_ADD,
 * OP_VAE_HEADS(_BWD)), launched by the same helpers and with the same geometry as the plan executor; bf16 NDHWC activations.
 *   group_norm_bwd_saved: backward of act(GroupNorm(cat(xa, xb))) from the forward's saved ab [N][C][2] and mr [N][G][2]; dxa / dxb
 *                (+= acc_a / acc_b), dgamma / dbeta summed over the batch.  ca, cb % 8 == 0; form 0 = stats + finalize + apply, 1 = stats +
 *                fold-apply (LDM_ERR_UNSUPPORTED where the planner would not pick it: see _fold_chunks, which returns `chunks`); cs (form 1,
 *                optional) = column sums of the stored dx per row chunk, [N][chunks][ca][2] then [N][chunks][cb][2] (pairs (sum, 0)).
 *   colsum_finalize: desc = k rows of {partial_off, out_off, N, nslab, C, accumulate_over_n, count, out_stride} (offsets in floats);
 *                batched 0 (k = 1) | 1 (one launch; table in desc_ws, ldm_op_colsum_finalize_ws_bytes).
 *   grad_export: desc = k rows of {src_off, dst_off, slab_stride, taps, rows_total, ld, row_off, col_off, cout, cin, nsplit} (floats);
 *                dst[(co * cin + ci) * taps + t] = sum_k src[k * slab_stride + (t * rows_total + row_off + co) * ld + col_off + ci].
 *   weight_flip_transpose_batched: desc = k rows of {w_off, wt_off (bf16 elements), ksize, cout, cout_pad, cin, ci_off, ci_cnt}.
 *   linear_bwd: dx (row stride x_stride; part: ldm_op_linear_bwd_nz(O) * B * I floats), dW [O][I], db [O] of y = W act(x) + b.
 *   upsample_bwd / add_bf16: sumpool2 (adjoint of the nearest x2 upsample) and out = a + b on bf16.
 *   vae_heads / _bwd: AutoencoderKL sampling head and its backward; fp32 = 1 for fp32 dz / dy storage. */
size_t ldm_op_group_norm_bwd_saved_scratch_bytes(int N, int C, int DHW, int groups);
int ldm_op_group_norm_bwd_fold_chunks(int N, int C, int groups, int DHW);
int ldm_op_group_norm_bwd_saved(const void* dy, const void* xa, int ca, const void* xb, int cb, const float* ab, const float* mr,
                                const float* gamma, int groups, int act, const void* acc_a, const void* acc_b, void* dxa, void* dxb,
                                float* dgamma, float* dbeta, float* cs, int N, int DHW, int form, void* scratch, size_t scratch_bytes,
                                void* stream);
size_t ldm_op_colsum_finalize_ws_bytes(const int64_t* desc, int k);
int ldm_op_colsum_finalize(const float* partial, float* out, const int64_t* desc, int k, int batched, void* desc_ws, size_t desc_ws_bytes,
                           void* stream);
size_t ldm_op_grad_export_ws_bytes(const int64_t* desc, int k);
int ldm_op_grad_export(const float* src, float* dst, const int64_t* desc, int k, int batched, void* desc_ws, size_t desc_ws_bytes, void* stream);
size_t ldm_op_weight_flip_transpose_batched_ws_bytes(const int64_t* desc, int k);
int ldm_op_weight_flip_transpose_batched(const void* w, void* wt, const int64_t* desc, int k, void* desc_ws, size_t desc_ws_bytes, void* stream);
int ldm_op_linear_bwd_nz(int O);
int ldm_op_linear_bwd(const void* W, const float* dy, const float* x_pre, float* dx, float* dW, float* db, int B, int I, int O, int dy_stride,
                      int x_stride, int silu_in, float* part, size_t part_bytes, void* stream);
int ldm_op_upsample_bwd(const void* dy, void* dx, int N, int D, int H, int W, int C, void* stream);
int ldm_op_add_bf16(const void* a, const void* b, void* out, int64_t n, void* stream);
int ldm_op_vae_heads(const float* ml, const float* eps, float* mu, float* sigma, float* z, int N, int L, int DHW, void* stream);
int ldm_op_vae_heads_bwd(const void* dz, int Ls, const float* ml, const float* z, const float* g_mu, const float* g_sigma, void* dy,
                         int N, int L, int Cs, int DHW, int fp32, void* stream);
/* The split-K conv -> GroupNorm pair as the inference plans launch it at the low-resolution levels (conv + ONE finalize-and-GroupNorm
 * launch, csrc/fin_gn.h; MONAI ResBlock conv1 -> norm2 -> SiLU behind 3d_ldm/train_diffusion.py:197-205): gn_out = GroupNorm(+SiLU) of
 * bf16(conv + bias + temb[n] + residual), conv_out (optional) = that bf16 tensor itself.  splitk >= 2.  Every workgroup of the second launch
 * owns one (sample, group) over all rows (the conv writes its fp32 slabs one plane per group), so no statistics cross workgroups.
 * LDM_ERR_UNSUPPORTED for shapes the plans keep on two launches (channels per group not a power of two in 4 ... 64, > 4096 items per group). */
size_t ldm_op_conv3d_fin_gn_scratch_bytes(int N, int D, int H, int W, int cout_pad, int splitk);
int ldm_op_conv3d_fin_gn(const void* x, int cin, const void* w, const float* bias, const float* temb, int temb_stride, const void* residual,
                         const float* gamma, const float* beta, int groups, float eps, int silu, void* conv_out, void* gn_out,
                         int N, int D, int H, int W, int cout, int cout_pad, int wgn, int splitk, void* scratch, size_t scratch_bytes,
                         void* stream);
/* producer -> GroupNorm pair as the inference plans launch it (conv epilogue / write-through split-K finalize leave the statistics
 * slabs, one-launch GroupNorm(+SiLU) with write-through stores folds them): the per-kernel gate of exactly those kernel variants */
size_t ldm_op_conv3d_gn_scratch_bytes(int N, int D, int H, int W, int cout_pad, int splitk);
int ldm_op_conv3d_gn(const void* x, int cin, const void* w, const float* bias, const float* gamma, const float* beta, int groups, float eps,
                     int silu, void* conv_out, void* gn_out, int N, int D, int H, int W, int cout, int cout_pad, int wgn, int splitk,
                     void* scratch, size_t scratch_bytes, void* stream);
size_t ldm_op_group_norm_scratch_bytes(int N, int C, int DHW);
int ldm_op_group_norm(const void* xa, int ca, const void* xb, int cb, const float* gamma, const float* beta,
                      int groups, float eps, int silu, void* out, int N, int DHW, void* scratch, size_t scratch_bytes,
                      void* stream);
/* softmax(q k^T / 8) v with head_dim 64: qkv [B*N][3C] bf16 (q|k|v, channel = head*64 + d) -> out [B*N][C] bf16. */
int ldm_op_attention(const void* qkv, void* out, int B, int N, int C, void* stream);
/* the same for head_dim = 32 | 64 | 128 | 256 (num_head_channels 32: 3d_ldm/config/config_train_stable.json:45-46; the AutoencoderKL
 * attention blocks are single-head, head_dim = C: config_train_32g.json:21-25); lse (optional) receives the log-sum-exp rows */
int ldm_op_attention_hd(const void* qkv, void* out, float* lse, int B, int N, int C, int head_dim, void* stream);
int ldm_op_attention_bwd_hd(const void* qkv, const void* o, const void* d_o, const float* lse, float* delta_scratch, void* dqkv,
                            int B, int N, int C, int head_dim, void* stream);
/*      training form (also writes lse [B][C/64][N] fp32) and backward: dqkv [B*N][3C] bf16 from d_o [B*N][C] bf16;
 *      delta_scratch: B * (C/64) * N floats. */
int ldm_op_attention_train(const void* qkv, void* out, float* lse, int B, int N, int C, void* stream);
int ldm_op_attention_bwd(const void* qkv, const void* o, const void* d_o, const float* lse, float* delta_scratch, void* dqkv,
                         int B, int N, int C, void* stream);

/* ---- measurement support (bench.py): HIP events around every launch of ONE conv tile configuration
 *      (wgm x wgn waves, K depth bk), recorded on the launch stream.  stop() fills
 *      out = {instrumented launches, their total ms, their algorithmic FLOPs, all conv launches, all conv FLOPs}.
 *      plan_conv_cfgs lists the {wgm, wgn, bk | halo << 8, splitk} the planner chose per conv of a plan ("unet"|"enc"|"dec");
 *      halo: 0 = conv_igemm_kernel, 1 / 2 = conv3_halo_kernel (126 x 128 / 254 x 64 tiles), 3 = conv3_block_kernel, 4 = conv3_block128_kernel. -- */
int ldm_profile_start(int wgm, int wgn, int bk, int max_launches);
/*      wgm = LDM_PROFILE_GRAD_ACCUM (wgn, bk ignored) instruments the gradient-accumulation launches instead of a conv configuration
 *      (ldm_model_set_grad_accum, ldm_op_grad_accumulate): detail()'s flops[k] then holds the BYTES launch k moves (8 per element in
 *      assign mode, 12 in add mode) and stop()'s out[2] their sum. */
#define LDM_PROFILE_GRAD_ACCUM (-1)
int ldm_profile_detail(double* flops, double* ms, int max);   /* per instrumented launch; call before ldm_profile_stop; returns their number */
int ldm_profile_stop(double out[5]);
/* Per-op timeline (HIP events around every op of every launch plan that runs while it is on) appended as CSV rows to `path`; NULL or
 * "" = off.  Replaces the torch.profiler window of 3d_ldm/train_autoencoder.py:312-329 (--profile).  Initially: $LDM_PLAN_TRACE. */
int ldm_set_plan_trace(const char* path);
/* diagnostic builds (-DLDM_KSTAMPS) only: in-kernel 100 MHz stamps of the instrumented kernels, [entries][8] in launch order; the
 * product library returns 0 entries */
int ldm_debug_kstamps(unsigned long long* out, int max_entries, int reset);
int ldm_model_plan_conv_cfgs(ldm_model* m, const char* kind, int B, int D, int H, int W, int* cfgs, int max_convs);
/* launches of a cached inference plan ("unet"|"enc"|"dec"; builds it if needed) */
int ldm_model_plan_launches(ldm_model* m, const char* kind, int B, int D, int H, int W);

/* ---- data-parallel collectives (replaces init_process_group("nccl") + DDP all-reduce,
 *      3d_ldm/utils.py:55-63, 3d_ldm/train_diffusion.py:121-123,147-149,281-283): RCCL over xGMI.
 *      unique_id is the 128-byte ncclUniqueId produced by ldm_comm_unique_id on rank 0 and distributed
 *      by the launcher's store.  dtype: 0 = fp32, 1 = bf16; op: 0 = sum, 1 = avg. ------------------------------ */
typedef struct ldm_comm ldm_comm;
int ldm_comm_unique_id(char id[128]);
int ldm_comm_init(int rank, int world, const char id[128], ldm_comm** out);
/* Same communicator object over a caller-supplied transport instead of RCCL: fn must leave the reduction (op) over the `world`
 * ranks in buf, ordered on `stream`; non-zero return = failure.  What the library does around the transport (bucket ranges, issue
 * points, streams, op = avg, the join in front of the optimizer) is identical, which is what lets tests/test_gpu_comm.py play the
 * second rank of a 2-rank job on one GPU.  No reference counterpart (test seam). */
typedef int (*ldm_allreduce_fn)(void* user, void* buf, int64_t count, int dtype, int op, void* stream);
int ldm_comm_init_custom(int rank, int world, ldm_allreduce_fn fn, void* user, ldm_comm** out);
int ldm_comm_allreduce(ldm_comm* c, void* buf, int64_t count, int dtype, int op, void* stream);
int ldm_comm_broadcast(ldm_comm* c, void* buf, int64_t count, int dtype, int root, void* stream);
int ldm_comm_barrier(ldm_comm* c, void* stream);
void ldm_comm_destroy(ldm_comm* c);
int ldm_comm_rank(const ldm_comm* c);
int ldm_comm_world(const ldm_comm* c);
/* Bucketed gradient all-reduce overlapped with backward (replaces DistributedDataParallel's bucket hooks,
 * 3d_ldm/train_diffusion.py:147-149): while a communicator is attached, ldm_unet_train_backward / ldm_vae_train_backward average the
 * flat gradient buffer over the ranks, bucket by bucket (LDM_GRAD_BUCKET_MB, default 48), each collective queued on the
 * communicator's stream as soon as backward has finished that tail range of the buffer; `stream` waits for the last one.
 * ldm_model_grad_sync_trace returns the bucket timeline of the last backward call (n buckets; entry n = end of the call). */
int ldm_model_set_grad_sync(ldm_model* m, ldm_comm* comm);
int ldm_model_grad_sync_trace(ldm_model* m, double* issue_ms, double* done_ms, int64_t* elems, int max);
/* Wire dtype of the bucketed exchange: 0 = fp32 (default, what DDP reduces: 3d_ldm/train_diffusion.py:147-149), 1 = bf16 (each
 * bucket cast into a staging slice on the communicator's stream, all-reduced (avg) as bf16, cast back: half the bytes on xGMI;
 * SURVEY.md section 8a row a7 "382 MB if bf16 grads").  ldm_model_grad_sync_pending: buckets issued that no join has covered yet
 * (0 = nothing of this communicator is in flight ahead of the launch stream; host bookkeeping, no synchronisation). */
int ldm_model_set_grad_wire(ldm_model* m, int dtype);
int ldm_model_grad_sync_pending(const ldm_model* m);
/* Gradient accumulation over micro-batches inside the backward's buckets (no reference counterpart: its multi-GPU notes recommend
 * "gradient accumulation steps", its trainers never implemented them).  acc_flat: a caller-owned device buffer in the layout of
 * flat_grads (ldm_model_param_numel_total floats), or NULL = off (the default: the plans then run exactly the launches they ran
 * before).  While armed, every training backward that receives a non-NULL flat_grads (ldm_unet_train_backward,
 * ldm_unet_train_backward_input, ldm_vae_train_backward; bf16 and fp32 precision) is micro-batch `micro_index` of a window of
 * `micro_count`: flat_grads still ends up holding that micro-batch's own gradient, bit for bit, and at every bucket point of the plan,
 * behind the exports of that range and on the launch stream, one streaming launch folds the finished tail range into acc_flat with
 * scale = (float)(1.0 / micro_count): acc = g * scale if micro_index == 0 (acc is not read: no zeroing, nothing stale survives),
 * acc += g * scale otherwise (the product rounded before the sum).  With a communicator attached, micro-batches in front of the
 * last exchange nothing (no bucket, no join; ldm_model_grad_sync_pending stays 0, ldm_model_grad_sync_trace reports 0 buckets); on
 * the last one every bucket's all-reduce runs on the acc_flat range, behind that range's accumulate launch and still overlapped with
 * the rest of backward, in either wire format, and the join is where it was.  The data-only backward (flat_grads == NULL) ignores
 * accumulation as it ignores the exchange.  The caller calls this before each backward of the window; every micro-batch of a window
 * must have the same batch size.  micro_count < 1 or micro_index outside [0, micro_count): LDM_ERR_BAD_ARG, the previous setting
 * stays in force. */
int ldm_model_set_grad_accum(ldm_model* m, float* acc_flat /* NULL: off */, int micro_index, int micro_count);
/* The accumulate kernel on its own over n fp32 elements: acc[i] = g[i] * scale (assign != 0) or acc[i] = acc[i] + g[i] * scale, one
 * launch, 16 bytes per lane between the first and the last 16-byte boundary of the range when acc and g share their misalignment
 * (scalar throughout otherwise).  NaN and +-inf propagate by ordinary arithmetic.  n == 0: returns 0 without a launch; NULL acc or g
 * with n > 0, or n < 0: LDM_ERR_BAD_ARG before any launch. */
int ldm_op_grad_accumulate(float* acc, const float* g, int64_t n, float scale, int assign, void* stream);
/* Evidence for bench records / tests: {all-reduce calls, all-reduce bytes in the wire dtype, broadcast calls, broadcast bytes} as
 * handed to the transport; whether that transport is RCCL; ncclGetVersion() of the loaded librccl (e.g. 22606; negative = status). */
int ldm_comm_stats(const ldm_comm* c, int64_t out[4]);
int ldm_comm_is_rccl(const ldm_comm* c);
int ldm_comm_rccl_version(void);
/* The exchange schedule of the training plan for this shape, built on the host (no GPU needed): events in launch order with
 * kind 0 = an op leaves final values in flat_grads[lo, lo + n), 1 = bucket [lo, lo + n) handed to the communicator, 2 = join,
 * 3 = unclassified write; op = index of the launch-plan op.  Returns the event count (only `max` are written). */
int ldm_model_grad_schedule(ldm_model* m, int B, int D, int H, int W, int* kind, int64_t* lo, int64_t* n, int* op, int max);

/* ---- Plan-only operators: the kernels that only the launch plans, the derived-weight rebuild after an upload and the time-embedding
 * table build run, behind the launch helpers those use, for per-kernel tests against fp64.  All pointers are device pointers, all
 * tensors 16-byte aligned.  Bad arguments return LDM_ERR_BAD_ARG / LDM_ERR_UNSUPPORTED / LDM_ERR_WORKSPACE before anything is launched. */
/* 3x3x3 stride-1 "same" convolution with 1 .. 4 output channels (conv3_thin_kernel, the networks' last layer):
 * x bf16 [N][D][H][W][cin], w bf16 packed [27][cout_pad][cin] (rows 0 .. cout_real-1 are read), bias [>= cout_real] or NULL,
 * out fp32 [N][cout_real][D][H][W].  cin % 32 == 0, cin <= 128 (above: LDM_ERR_UNSUPPORTED). */
int ldm_op_conv3d_thin(const void* x_bf16_ndhwc, int cin, const void* w_packed, const float* bias, float* out_f32_ncdhw, int N, int D, int H, int W,
                       int cout_real, int cout_pad, void* stream);
/* The same layer as the fp32 precision mode runs it: x fp32 [N][D][H][W][cin] is split into (hi | lo) bf16 halves, w fp32
 * [27][cout_pad][cin] into [hi | lo | hi], and the kernel adds the three bf16 products hi hi + lo hi + hi lo in fp32.
 * ws: ldm_op_conv3d_thin_f32_ws_bytes(cin, N, D, H, W, cout_pad) bytes. */
size_t ldm_op_conv3d_thin_f32_ws_bytes(int cin, int N, int D, int H, int W, int cout_pad);
int ldm_op_conv3d_thin_f32(const float* x_f32_ndhwc, int cin, const float* w_packed, const float* bias, float* out_f32_ncdhw, int N, int D, int H,
                           int W, int cout_real, int cout_pad, void* ws, size_t ws_bytes, void* stream);
/* out[b][0 .. dim) = cos(t[b] f_j) | sin(t[b] f_j), f_j = exp(-ln(10000) j / (dim / 2)), j = 0 .. dim / 2 - 1 (cos first); B dim <= 2^20 */
int ldm_op_timestep_embedding(const float* t, float* out, int B, int dim, void* stream);
/* y[b][o] = sum_i w[o][i] act(x[b][i]) + bias[o] (bias may be NULL), act = SiLU when silu_in.  w [O][I] bf16, or fp32 when fp32_weights;
 * x rows x_stride floats apart, y rows y_stride (y[b][O .. y_stride) is not written).  bf16 weights: I % 8 == 0; fp32 weights: I % 4 == 0
 * and x_stride % 4 == 0.  B <= 65535. */
int ldm_op_gemv(const void* w, int fp32_weights, const float* bias, const float* x, float* y, int B, int I, int O, int x_stride, int y_stride,
                int silu_in, void* stream);
/* (x [N'][cx][DHW] | cond [N'][cc][DHW]) fp32 -> out [N][DHW][Cs], bf16 or (fp32_out) fp32, channels >= cx + cc zero; cond may be NULL.
 * guided_B = 0: N' = N.  guided_B = B > 0 (classifier-free guidance): N = 2 B, N' = B; samples 0 .. B-1 hold (x | fill), samples
 * B .. 2B-1 hold (x | cond). */
int ldm_op_pack2(const float* x, int cx, const float* cond, int cc, void* out, int N, int Cs, int64_t DHW, int fp32_out, int guided_B, float fill,
                 void* stream);
/* The first conv's patch matrix: out bf16 [N D H W][Kp], column tap (cx + cc) + c = channel c of (x | cond) at the voxel that tap
 * (kd, kh, kw) of a 3x3x3 pad-1 conv reads; out-of-volume taps and columns >= 27 (cx + cc) are zero.  Kp % 8 == 0, Kp >= 27 (cx + cc). */
int ldm_op_pack_im2col(const float* x, int cx, const float* cond, int cc, void* out, int N, int D, int H, int W, int Kp, int guided_B, float fill,
                       void* stream);
/* Weights derived from a packed 3x3x3 matrix after an upload.
 * phase: w3 bf16 [27][cout_pad][cin_s] -> wp bf16 [parity 8][tap 8][cout_pad][cin_s], the taps of (nearest x2 upsample -> conv) that read
 *   the same source voxel summed in fp32 (cin_s % 8 == 0);
 * im2col: w3 -> w2 bf16 [cout_pad][Kp], w2[co][tap cin + c] = w3[tap][co][c], other columns zero;
 * x3: w fp32 [rows][cin] -> bf16 [rows][hi | lo | hi], hi = bf16(w), lo = bf16(w - hi) (cin % 4 == 0);
 * x3_phase: w3 fp32 [27][cout_pad][cin] -> bf16 [parity 8][tap 8][cout_pad][hi | hi | lo] of the fp32 phase sums (cin % 4 == 0). */
int ldm_op_phase_weights(const void* w3, void* wp, int cout_pad, int cin_s, void* stream);
int ldm_op_im2col_weights(const void* w3, void* w2, int cout_pad, int cin_s, int cin, int Kp, void* stream);
int ldm_op_x3_weights(const float* w, void* out, int64_t rows, int cin, void* stream);
int ldm_op_x3_phase_weights(const float* w3, void* wp, int cout_pad, int cin, void* stream);
/* x fp32 [N][D][H][W][C] -> out bf16 [N][D << up][H << up][W << up][hi(C) | lo(C)] (up 0 | 1: nearest x2 upsample), C % 4 == 0 */
int ldm_op_split_f32(const float* x, void* out, int N, int C, int D, int H, int W, int up, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LDM3D_H */
