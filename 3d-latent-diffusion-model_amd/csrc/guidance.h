// Measurement-guided sampling (DPS, Chung et al. 2023; reconstruction guidance): the two element-wise kernels around the UNet's input VJP
// for the built-in measurement, a weighted pooled quadratic in latent space:
//   x0_hat = (x - s m) / a (epsilon) | m (sample) | a x - s m (v_prediction), UNCLIPPED, a = sqrt(abar_t), s = sqrt(1 - abar_t)
//   r = w .* (P x0_hat - y), P = mean over non-overlapping pool^3 cubes per channel;  L_b = 1/2 |r_b|^2
//   g = dL/dx0_hat = pool^-3 upsample_nearest(w .* r);  grad_x L = c_x g + J^T(c_m g), (c_x, c_m) = (1/a, -s/a) | (0, 1) | (a, -s)
// guidance_residual_kernel reads x_t and m and writes c_m g (the grad_out of the data-only backward), c_x g and |r_b|^2;
// guidance_update_kernel applies x -= zeta_b (c_x g + J^T(c_m g)) after the scheduler step, zeta_b = scale / max(|r_b|, 1e-12) (DPS's step
// size) or scale, with the norm read from device memory.  One workgroup per sample and a fixed-order tree over its 256 partial sums: no
// floating-point atomics, the same inputs give the same bits.
#pragma once
#include "common.h"
#include "norm_elem.h"

struct GuideResParams {
    const float* x; const float* m;                  // x_t and the model output, fp32 [B][C][D][H][W]
    const float* target; int target_batch;           // y [1 or B][C][D/p][H/p][W/p]
    const float* weight; int weight_batch;           // w, the target's shape per sample, [1 or B]; null: 1
    float* grad_out; float* gx;                      // c_m g and c_x g, [B][C][D][H][W]
    float* norm2;                                    // [B]: |r_b|^2 of this step
    float* norm_tab;                                 // optional [n_steps][B]: row k (the sampler's step counter) := |r_b|
    const float* coef; const SamplerState* st; int n_steps;   // the sampler's 8-float rows and device step counter, or (st null) ...
    float a, s;                                      // ... sqrt(abar_t), sqrt(1 - abar_t) by value
    int pred, pool, B, C, D, H, W;
};

__global__ __launch_bounds__(256) void guidance_residual_kernel(const GuideResParams p) {
#pragma clang fp contract(off)
    __shared__ float red[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    int k = 0;
    float a = p.a, s = p.s, inv_a = 1.0f / p.a;
    if (p.st) {
        k = p.st->k;
        const float* c = p.coef + (size_t)(k < p.n_steps ? k : p.n_steps - 1) * 8;
        inv_a = c[0]; s = c[1]; a = c[6];
    }
    float cx, cm;
    if (p.pred == PRED_EPSILON) { cx = inv_a; cm = -s * inv_a; }
    else if (p.pred == PRED_SAMPLE) { cx = 0.f; cm = 1.f; }
    else { cx = a; cm = -s; }
    const int pl = p.pool, pd = p.D / pl, ph = p.H / pl, pw = p.W / pl;
    const long cells = (long)p.C * pd * ph * pw, dhw = (long)p.D * p.H * p.W;
    const float inv_p3 = 1.0f / (float)(pl * pl * pl);
    const float* xb = p.x + (size_t)b * p.C * dhw; const float* mb = p.m + (size_t)b * p.C * dhw;
    float* gob = p.grad_out + (size_t)b * p.C * dhw; float* gxb = p.gx + (size_t)b * p.C * dhw;
    const float* yb = p.target + (p.target_batch > 1 ? (size_t)b * cells : 0);
    const float* wb = p.weight ? p.weight + (p.weight_batch > 1 ? (size_t)b * cells : 0) : nullptr;
    float part = 0.f;
    for (long q = tid; q < cells; q += 256) {
        const int qw = (int)(q % pw); long r = q / pw; const int qh = (int)(r % ph); r /= ph; const int qd = (int)(r % pd); const int c = (int)(r / pd);
        const long base = (long)c * dhw + ((long)qd * pl * p.H + (long)qh * pl) * p.W + (long)qw * pl;
        float sum = 0.f;
        for (int dz = 0; dz < pl; ++dz)
            for (int dy = 0; dy < pl; ++dy)
                for (int dx = 0; dx < pl; ++dx) {
                    const long i = base + ((long)dz * p.H + dy) * p.W + dx;
                    const float xv = xb[i], mv = mb[i];
                    sum += p.pred == PRED_EPSILON ? (xv - s * mv) * inv_a : p.pred == PRED_SAMPLE ? mv : a * xv - s * mv;
                }
        const float w = wb ? wb[q] : 1.f;
        const float res = w * (sum * inv_p3 - yb[q]);
        part += res * res;
        const float g = inv_p3 * (w * res);
        const float go = cm * g, gxv = cx * g;
        for (int dz = 0; dz < pl; ++dz)
            for (int dy = 0; dy < pl; ++dy)
                for (int dx = 0; dx < pl; ++dx) {
                    const long i = base + ((long)dz * p.H + dy) * p.W + dx;
                    gob[i] = go; gxb[i] = gxv;
                }
    }
    red[tid] = part;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {                  // fixed order: the same inputs give the same bits
        if (tid < h) red[tid] += red[tid + h];
        __syncthreads();
    }
    if (tid == 0) {
        p.norm2[b] = red[0];
        if (p.norm_tab && k < p.n_steps) p.norm_tab[(size_t)k * p.B + b] = sqrtf(red[0]);
    }
}

// x -= zeta_b (gx + dx): gx = c_x g, dx = J^T(c_m g) from the data-only backward; norm2 [B] = |r_b|^2 from the residual kernel
__global__ __launch_bounds__(256) void guidance_update_kernel(float* __restrict__ x, const float* __restrict__ gx, const float* __restrict__ dx,
                                                              const float* __restrict__ norm2, float scale, int normalize, long per_sample, int B) {
#pragma clang fp contract(off)
    const long n = per_sample * B;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int b = (int)(i / per_sample);
        const float zeta = normalize ? scale / fmaxf(sqrtf(norm2[b]), 1e-12f) : scale;
        x[i] = x[i] - zeta * (gx[i] + dx[i]);
    }
}
