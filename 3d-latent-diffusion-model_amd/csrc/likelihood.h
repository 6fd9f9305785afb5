// Likelihood of a GIVEN latent under a DDPM (MONAI >= 1.4 DiffusionInferer.get_likelihood, monai/inferers/inferer.py, restated): for every
// timestep of the schedule the KL between the true posterior q(x_{t-1} | x_t, x_0) and the model's p(x_{t-1} | x_t), at t = 0 the
// discretised decoder log-likelihood instead, averaged per sample and summed over the timesteps (nats per dimension).  One noise
// tensor z serves every timestep: x_t = sqrt(abar_t) x0 + sqrt(1 - abar_t) z.
//
// One row per timestep, LIK_ROW floats, t in slot 5 like every sampler row (sampler_reset_kernel, the time-embedding table and
// temb_row_kernel serve it unchanged):
//   {sqrt(abar_t), sqrt(1 - abar_t), 1/sqrt(abar_t), c0, 1/var, t, 1/sqrt(var), c1, 0 ...}
// c0 / c1: DDPMScheduler's posterior-mean coefficients of x0 and x_t; var: the fixed variance of the step (fixed_small clamps it at
// 1e-20, fixed_large is beta_t).  With a fixed variance both log-variances are equal and the KL of t > 0 is
//   (mean_q - mean_p)^2 / (2 var),    mean_q - mean_p = c0 (x0 - x0_hat)   exactly,
// evaluated in that form: MONAI subtracts the two O(1) means, which cancels (2e-4 relative in fp32 at t = 999).
// t = 0: -log of the probability mass the Gaussian N(mean_p, var) puts on the bin of width `bin` around x0, with the tanh
// approximation of the normal CDF MONAI uses; the outermost bins (x0 < -0.999, x0 > 0.999) are open-ended; the mass is floored at 1e-12.
// With fixed_small, var(0) = 1e-20: the term is a step function, 0 where mean_p falls into x0's bin and -log(1e-12) = 27.631 elsewhere.
//
// lik_term<PRED> (t > 0, fp32) and lik_decoder_term<PRED> (t = 0, double rounded once) are the only copies of that arithmetic, inside the
// one lik_term_kernel behind both the host-driven ldm_likelihood_term and the device-resident ldm_unet_likelihood_step, which therefore
// agree bit for bit; contraction is off and every fused multiply-add is spelled out, as in sampler_update.
//
// Reduction: grid (blocks, B), blocks a function of per_sample alone.  A thread owns whole quads of ONE sample, adds its terms in
// double in element order, the workgroup folds over a fixed LDS tree and writes one double; lik_finalize_kernel (one workgroup per
// sample, a second launch) folds the sample's partials over the same tree, rounds sum / per_sample to fp32 once and adds it to
// total[b].  No atomics, no cross-workgroup hand-off: the same inputs give the same bits, and sample b's bits do not depend on B.
#pragma once

#define LIK_ROW 16
#define LIK_THREADS 256
#define LIK_MAX_BLOCKS 256                   // per sample: the finalize kernel reads one partial per thread

struct LikCoef { float sqrt_a, sqrt_b, inv_sqrt_a, c0, inv_var, inv_std, c1; int last; };   // last: t == 0, the decoder term
__host__ __device__ __forceinline__ LikCoef lik_coef(const float* r) {
    return LikCoef{r[0], r[1], r[2], r[3], r[4], r[6], r[7], r[5] == 0.f ? 1 : 0};
}

// v = sqrt(2 / pi) (u + 0.044715 u^3): MONAI's normal CDF is 0.5 (1 + tanh v)
__device__ __forceinline__ double lik_cdf_arg(double u) {
#pragma clang fp contract(off)
    return 0.79788456080286535588 * (u + 0.044715 * ((u * u) * u));
}

// The decoder term (the row with t == 0), from the fp32 inputs and the fp32 row in DOUBLE, rounded to fp32 once: log(P - M) of two
// nearly equal CDF values, and 1 - M in a tail, are what fp32 loses first, and this row is one launch of a whole loop.
//   P = 0.5 (1 + tanh vp), M = 0.5 (1 + tanh vm), v = lik_cdf_arg(inv_std (cx +- bin / 2)), cx = x0 - (c0 x0_hat + c1 x_t).
// The open-ended bins use the same functions in their logistic form, P = 1 / (1 + exp(-2 vp)) and 1 - M = 1 / (1 + exp(2 vm)), which
// keeps the relative accuracy of a small tail.  fixed_small: inv_std = 1e10, v is huge, tanh = +-1 and exp = 0 or inf: no NaN.
template <int PRED>
__device__ __forceinline__ float lik_decoder_term(const LikCoef& c, int clip, float half_bin, float x0, float xt, float m) {
#pragma clang fp contract(off)
    const double xd = (double)xt, md = (double)m, x0d = (double)x0, hb = (double)half_bin, inv = (double)c.inv_std;
    double xh;
    if constexpr (PRED == PRED_EPSILON) xh = (xd - (double)c.sqrt_b * md) / (double)c.sqrt_a;
    else if constexpr (PRED == PRED_SAMPLE) xh = md;
    else xh = (double)c.sqrt_a * xd - (double)c.sqrt_b * md;
    if (clip) xh = fmin(fmax(xh, -1.0), 1.0);
    const double cx = x0d - ((double)c.c0 * xh + (double)c.c1 * xd);
    double p;
    if (x0 < -0.999f) p = 1.0 / (1.0 + exp(-2.0 * lik_cdf_arg(inv * (cx + hb))));
    else if (x0 > 0.999f) p = 1.0 / (1.0 + exp(2.0 * lik_cdf_arg(inv * (cx - hb))));
    else p = 0.5 * (tanh(lik_cdf_arg(inv * (cx + hb))) - tanh(lik_cdf_arg(inv * (cx - hb))));
    return (float)(-log(fmax(p, 1e-12)));
}

// One element's KL term (a row with t > 0) for model output m at x_t, x0 the scored latent.
template <int PRED>
__device__ __forceinline__ float lik_term(const LikCoef& c, int clip, float x0, float xt, float m) {
#pragma clang fp contract(off)
    float xh;
    if constexpr (PRED == PRED_EPSILON) xh = __fmaf_rn(-c.sqrt_b, m, xt) * c.inv_sqrt_a;
    else if constexpr (PRED == PRED_SAMPLE) xh = m;
    else { static_assert(PRED == PRED_V, "prediction type"); xh = __fmaf_rn(c.sqrt_a, xt, -(c.sqrt_b * m)); }
    if (clip) xh = fminf(fmaxf(xh, -1.f), 1.f);
    const float d = c.c0 * (x0 - xh);
    return 0.5f * ((d * d) * c.inv_var);
}

// The per-sample launch geometry of the three kernels below: a function of per_sample alone
static inline int lik_blocks(long per_sample) {
    const long nq = (per_sample + 3) / 4;
    long nb = (nq + 4 * LIK_THREADS - 1) / (4 * LIK_THREADS);
    return (int)(nb < 1 ? 1 : nb > LIK_MAX_BLOCKS ? LIK_MAX_BLOCKS : nb);
}

// z of the likelihood's one noise tensor: Philox block (sample b's quad q, step 0) of the sampler's stream, lane e = element 4 q + e of
// the sample.  A function of (seed, per_sample, b, element): not of B.
__device__ __forceinline__ float4 lik_normal4(int b, long nqs, long q, unsigned seed_lo, unsigned seed_hi) {
    return sampler_normal4((unsigned long long)b * (unsigned long long)nqs + (unsigned long long)q, 0u, seed_lo, seed_hi);
}

// out = a x0 + s z, rounded as latent_add_noise rounds it (both products, then the sum) at every size; z from `noise` or, where that is
// null, from lik_normal4.  x0 null: out = z (the draw as a tensor).  grid (lik_blocks, B).
__global__ __launch_bounds__(LIK_THREADS) void lik_noisy_kernel(const float* __restrict__ x0, const float* __restrict__ noise,
                                                                float* __restrict__ out, long per_sample, int vec, float a, float s,
                                                                unsigned seed_lo, unsigned seed_hi) {
    const int b = blockIdx.y;
    const long nqs = (per_sample + 3) / 4, base = (long)b * per_sample;
    for (long q = (long)blockIdx.x * LIK_THREADS + threadIdx.x; q < nqs; q += (long)gridDim.x * LIK_THREADS) {
        const long j = 4 * q;
        const int cnt = (int)(per_sample - j < 4 ? per_sample - j : 4);
        float zz[4], xv[4] = {0.f, 0.f, 0.f, 0.f}, o[4];
        if (noise) latent_load4(noise + base + j, cnt, vec, zz);
        else { const float4 z = lik_normal4(b, nqs, q, seed_lo, seed_hi); zz[0] = z.x; zz[1] = z.y; zz[2] = z.z; zz[3] = z.w; }
        if (x0) latent_load4(x0 + base + j, cnt, vec, xv);
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = x0 ? latent_add_noise(a, xv[e], s, zz[e]) : zz[e];
        latent_store4(out + base + j, cnt, vec, o);
    }
}

struct LikParams {
    const float* x0; float* xt; const float* m; const float* noise;   // xt: read; with a table, rewritten in place for the NEXT row
    float* map;                                                      // optional per-element terms
    double* partial; int* kk;                                        // [B][gridDim.x] partial sums; kk[b]: the row this launch scored (table form)
    const float* coef; const SamplerState* st; int n_steps;          // the device table and counter, or null: the row arrives by value
    LikCoef c;
    long per_sample; int vec; int clip; float half_bin;
    unsigned seed_lo, seed_hi;
};

template <int PRED>
__global__ __launch_bounds__(LIK_THREADS) void lik_term_kernel(const LikParams p) {
    __shared__ double red[LIK_THREADS];
    int k = 0; bool live = true, renoise = false;
    LikCoef c = p.c; float na = 0.f, ns = 0.f;
    if (p.coef) {
        k = p.st->k; live = k >= 0 && k < p.n_steps;
        c = lik_coef(p.coef + (size_t)(live ? k : p.n_steps - 1) * LIK_ROW);
        if (live && k + 1 < p.n_steps) { renoise = true; na = p.coef[(size_t)(k + 1) * LIK_ROW]; ns = p.coef[(size_t)(k + 1) * LIK_ROW + 1]; }
    }
    const int b = blockIdx.y;
    const long nqs = (p.per_sample + 3) / 4, base = (long)b * p.per_sample;
    double acc = 0.0;
    if (live)
    for (long q = (long)blockIdx.x * LIK_THREADS + threadIdx.x; q < nqs; q += (long)gridDim.x * LIK_THREADS) {
        const long j = 4 * q;
        const int cnt = (int)(p.per_sample - j < 4 ? p.per_sample - j : 4);
        if (c.last) {
            // the decoder row: one element at a time through ONE copy of the double-precision code (four unrolled copies do not fit
            // the scalar registers); the same element order as below
            float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
            if (renoise && !p.noise) z = lik_normal4(b, nqs, q, p.seed_lo, p.seed_hi);
#pragma unroll 1
            for (int e = 0; e < cnt; ++e) {
                const long i = base + j + e;
                const float x0e = p.x0[i];
                const float kle = lik_decoder_term<PRED>(c, p.clip, p.half_bin, x0e, p.xt[i], p.m[i]);
                acc += (double)kle;
                if (p.map) p.map[i] = kle;
                if (renoise) p.xt[i] = latent_add_noise(na, x0e, ns, p.noise ? p.noise[i] : e == 0 ? z.x : e == 1 ? z.y : e == 2 ? z.z : z.w);
            }
            continue;
        }
        float xv[4], tv[4], mv[4], kl[4];
        latent_load4(p.x0 + base + j, cnt, p.vec, xv);
        latent_load4(p.xt + base + j, cnt, p.vec, tv);
        latent_load4(p.m + base + j, cnt, p.vec, mv);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            kl[e] = lik_term<PRED>(c, p.clip, xv[e], tv[e], mv[e]);
            if (e < cnt) acc += (double)kl[e];
        }
        if (p.map) latent_store4(p.map + base + j, cnt, p.vec, kl);
        if (renoise) {
            float zz[4], o[4];
            if (p.noise) latent_load4(p.noise + base + j, cnt, p.vec, zz);
            else { const float4 z = lik_normal4(b, nqs, q, p.seed_lo, p.seed_hi); zz[0] = z.x; zz[1] = z.y; zz[2] = z.z; zz[3] = z.w; }
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = latent_add_noise(na, xv[e], ns, zz[e]);
            latent_store4(p.xt + base + j, cnt, p.vec, o);
        }
    }
    const double f = metrics_block_fold(acc, red, 0);
    if (threadIdx.x == 0) {
        p.partial[(long)b * gridDim.x + blockIdx.x] = f;
        if (p.kk && blockIdx.x == 0) p.kk[b] = k;
    }
}

// Workgroup b: mean_b = fp32(sum of sample b's nb partials / per_sample); total[b] += mean_b; terms[k][b] = mean_b (optional).
// Table form (st non-null): k is the row the term kernel scored (kk[b]: no workgroup reads the counter here, so workgroup 0 may advance
// it), tbuf[b] := t of the next row, counter := k + 1; a k outside the table changes nothing.  Row-by-value form: k = k_host.
__global__ __launch_bounds__(LIK_THREADS) void lik_finalize_kernel(const double* __restrict__ partial, int nb, const int* __restrict__ kk, int k_host,
                                                                   double per_sample, float* __restrict__ total, float* __restrict__ terms, int B,
                                                                   SamplerState* st, const float* __restrict__ coef, int n_steps, float* __restrict__ tbuf) {
    __shared__ double red[LIK_THREADS];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int k = st ? kk[b] : k_host;
    const double s = metrics_block_fold(tid < nb ? partial[(long)b * nb + tid] : 0.0, red, 0);
    if (tid == 0 && k >= 0 && k < n_steps) {
        const float mean = (float)(s / per_sample);
        total[b] += mean;
        if (terms) terms[(long)k * B + b] = mean;
        if (st) {
            const int kn = k + 1;
            tbuf[b] = coef[(size_t)(kn < n_steps ? kn : n_steps - 1) * LIK_ROW + 5];
            if (b == 0) st->k = kn;
        }
    }
}

// Nearest-neighbour resize of fp32 [NC][d][h][w] -> [NC][D][H][W] with PyTorch's index rule (F.interpolate(mode="nearest")):
// src = min(floor(dst * scale), in - 1), scale = float(in) / out in fp32, per axis.
__global__ __launch_bounds__(256) void resize_nearest_kernel(const float* __restrict__ x, float* __restrict__ y, long NC, int d, int h, int w,
                                                             int D, int H, int W, float sd, float sh, float sw) {
#pragma clang fp contract(off)
    const long total = NC * D * H * W;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int ow = (int)(i % W); long r = i / W;
        const int oh = (int)(r % H); r /= H;
        const int od = (int)(r % D); const long nc = r / D;
        const int iw = min((int)floorf(ow * sw), w - 1), ih = min((int)floorf(oh * sh), h - 1), id = min((int)floorf(od * sd), d - 1);
        y[i] = x[((nc * d + id) * h + ih) * w + iw];
    }
}
