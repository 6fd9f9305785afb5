// Stage-2 training objective beyond the plain mean: per-timestep loss weights, a per-bin tracker of the loss and a loss-aware draw
// of the training timesteps.  ldm_op_weighted_mse_loss (lw_part_kernel + lw_fold_kernel) / ldm_timestep_resample (lw_resample_kernel).
//
// (a) Weighted loss.  l_b = mean_i (pred - target)^2 over sample b, w_b = w_table[t_b] * sample_w[b] (either factor 1 when its pointer
//     is null), loss_out[0] = (1/B) sum w_b l_b (the value that is differentiated), loss_out[1] = (1/B) sum l_b (comparable with
//     ldm_op_mse_loss), grad = 2 w_b (pred - target) / (B per_sample).  A t_b outside [0, T) never indexes the table: that sample's
//     weight is NaN, so loss_out[0] and the sample's gradient are NaN and the optimizer's device NaN-skip counts the step.
//     The [T] table itself is built on the host (Min-SNR-gamma, Hang et al. 2023, or a user table): there is no kernel for it.
//
//     Reduction: two stages, no float atomics, bit-identical on a repeat.  The arithmetic is mse_part_kernel's, laid out per sample:
//     a sample is covered by G = min(ceil(per_sample / 1024), cap(B)) "virtual blocks" of 256 "virtual threads"; virtual thread v
//     sums elements v, v + 256 G, v + 512 G, ... of ITS sample with one fma each, a virtual block folds its 256 sums as
//     mse_part_kernel folds its threads' (wave_sum over 64, then the four wave sums left to right), and lw_fold_kernel adds a sample's G
//     partials in double as mse_fold_kernel does (thread j takes partials j, j + 256, ..., then a pairwise tree).  With B = 1 and unit
//     weights that is ldm_op_mse_loss's sum term for term, so both its outputs come out bit for bit; a power-of-two weight scales them
//     exactly.  A real thread carries FOUR consecutive virtual threads (4 r .. 4 r + 3), so that it touches 16 contiguous bytes per
//     pass: one 16-byte load / store where per_sample % 4 == 0 and every pointer is 16-byte aligned (VEC), four guarded scalar ones
//     otherwise; a real block is four virtual blocks and belongs to one sample.  cap(B) = max(4, 2^floor(log2(1024 / B))) keeps
//     B G <= 1024 partials (the scratch) and at most 1024 fold slots (lw_fold_slots).
//     Bit equality with ldm_op_mse_loss at B = 1 is a contract CHOSEN here, not a necessity: it makes "the options cost nothing in
//     accuracy" checkable to the bit (a table of ones, or of 0.25, against the default trainer).  The virtual layout and the LDS
//     transpose in lw_part_kernel exist only for it; a plain per-sample two-stage reduction (each thread summing its own four
//     lanes) would be simpler and about as fast, and gives up exactly that equality (it then agrees to rounding, ~1e-7).
//
//     Tracker (optional, fp32 [2][K]: row 0 the second moments m2_k, row 1 the counts): thread 0 of the fold block walks b = 0 .. B-1
//     in batch order.  It works on an LDS copy of the tracker and on per-sample values that the block's threads prepared in parallel.
//     Bin k = (t_b K) / T in integers; a non-finite l_b (or a t_b outside the table) is skipped; count_k == 0: m2_k = l_b^2, else
//     m2_k = beta m2_k + (1 - beta) l_b^2 (formed in double from the fp32 state, stored fp32); count_k += 1 up to 2^24.  The tracker
//     sees the UNWEIGHTED l_b.
//
// (b) Loss-aware draw.  Bin k holds the n_k timesteps with (t K) / T == k, lo_k = ceil(k T / K).  While any count_k < warmup, or when
//     sum q is zero or not finite: P_k = n_k / T and iw = 1 exactly.  Otherwise q_k = n_k sqrt(m2_k),
//     P_k = (1 - uniform_prob) q_k / sum q + uniform_prob n_k / T.  The CDF is walked in fp64 by every thread (K <= 64): the bin is the
//     first k with u0 < C_k (the last otherwise), t = lo_k + min(n_k - 1, floor(u1 n_k)), iw = n_k / (T P_k), so that E[iw f(t)] is
//     the uniform mean of f.  (u0, u1) = draw[b][0..1] or, with draw null, Philox4x32-10 with the latent batch's key layout on a
//     stream of its own: counter = (0, idx[b], step, LATENT_STREAM_TAG + 5), key = seed, words 0 and 1 as (r >> 8) 2^-24: a function
//     of (seed, step, dataset index) alone, never of the batch slot.  One block; thread b serves sample b (rflow_timesteps_kernel).
//
//     This is the loss-second-moment resampler of Improved DDPM (Nichol & Dhariwal 2021) with three changes that are this project's
//     choices and not a restatement of it: an exponential moving average in place of its history of the last 10 losses per timestep,
//     bins of timesteps in place of single timesteps, and no collective (every rank keeps a tracker of its own).
#pragma once

#define LW_TIMESTEP_STREAM 5u                       // beside the latent batch's 0 .. 2, the rectified-flow draw (3) and condition dropout (4)
static_assert(repaint_tag_free(LATENT_STREAM_TAG + LW_TIMESTEP_STREAM) && LATENT_STREAM_TAG + LW_TIMESTEP_STREAM != REPAINT_KNOWN_STREAM_TAG &&
              LATENT_STREAM_TAG + LW_TIMESTEP_STREAM != REPAINT_JUMP_STREAM_TAG, "the timestep draw needs a Philox stream of its own");
enum { LW_BINS_MAX = 64, LW_PARTS_MAX = 1024, LW_VBLOCK = 256, LW_VPER_THREAD = 4 };

// virtual blocks per sample at most: max(4, 2^floor(log2(1024 / B))); 1024 at B = 1 (ldm_op_mse_loss's own cap), 16 at B = 64
__host__ __device__ __forceinline__ int lw_cap(int B) {
    int c = 4;
    while (c * 2 * B <= LW_PARTS_MAX) c *= 2;
    return c;
}
__host__ __device__ __forceinline__ int lw_vblocks(long per_sample, int B) {
    const long g = (per_sample + 1023) / 1024;
    const int cap = lw_cap(B);
    return g > cap ? cap : (g < 1 ? 1 : (int)g);
}
// fold slots per sample: the power of two at or above min(G, 256).  mse_fold_kernel's tree is 256 wide; slots at or above G hold zeros
// there, and a pairwise tree over the first 2^k >= G slots adds the same pairs in the same order, so the narrower tree has its bits.
__host__ __device__ __forceinline__ int lw_fold_slots(int G) {
    int w = 1;
    while (w < G && w < 256) w *= 2;
    return w;
}
// w_b; NaN for a timestep outside the table
__device__ __forceinline__ float lw_weight(const int64_t* __restrict__ ts, const float* __restrict__ wt, int T, const float* __restrict__ sw, int b) {
#pragma clang fp contract(off)
    float w = 1.f;
    if (wt) {
        const int64_t t = ts[b];
        w = (t >= 0 && t < (int64_t)T) ? wt[t] : __builtin_nanf("");
    }
    if (sw) w = wt ? w * sw[b] : sw[b];
    return w;
}
struct LossWeightParams {
    const float* pred; const float* target; float* grad; float* parts;                // parts [B][G]
    const int64_t* timesteps; const float* w_table; const float* sample_w;
    long per_sample; int B, T, G, rblocks;                                            // rblocks = ceil(G / 4) real blocks per sample
};
template <int VEC>
__global__ __launch_bounds__(256) void lw_part_kernel(const LossWeightParams p) {
#pragma clang fp contract(off)
    __shared__ float vacc[4 * LW_VBLOCK];
    __shared__ float red[16];
    const int b = blockIdx.x / p.rblocks, rb = blockIdx.x - b * p.rblocks;
    const float* __restrict__ pr = p.pred + (long)b * p.per_sample;
    const float* __restrict__ tg = p.target + (long)b * p.per_sample;
    float* __restrict__ gr = p.grad ? p.grad + (long)b * p.per_sample : nullptr;
    const float gs = lw_weight(p.timesteps, p.w_table, p.T, p.sample_w, b) * (2.0f / (float)((long)p.B * p.per_sample));
    const long pass = (long)p.G * LW_VBLOCK;                                          // elements of the sample per pass
    const long v0 = ((long)rb * 256 + threadIdx.x) * LW_VPER_THREAD;                  // this thread's first virtual thread
    float a[4] = {0.f, 0.f, 0.f, 0.f};
    if (v0 < pass)
    for (long i = v0; i < p.per_sample; i += pass) {
        if constexpr (VEC) {                                                          // per_sample % 4 == 0: i + 3 < per_sample
            const float4 x = *reinterpret_cast<const float4*>(pr + i), y = *reinterpret_cast<const float4*>(tg + i);
            const float d0 = x.x - y.x, d1 = x.y - y.y, d2 = x.z - y.z, d3 = x.w - y.w;
            a[0] = __fmaf_rn(d0, d0, a[0]); a[1] = __fmaf_rn(d1, d1, a[1]); a[2] = __fmaf_rn(d2, d2, a[2]); a[3] = __fmaf_rn(d3, d3, a[3]);
            if (gr) *reinterpret_cast<float4*>(gr + i) = make_float4(gs * d0, gs * d1, gs * d2, gs * d3);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (i + e < p.per_sample) {
                    const float d = pr[i + e] - tg[i + e];
                    a[e] = __fmaf_rn(d, d, a[e]);
                    if (gr) gr[i + e] = gs * d;
                }
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) vacc[4 * threadIdx.x + e] = a[e];
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int s = 0; s < 4; ++s) {                                                     // virtual wave 4 wave + s: 64 virtual threads
        const float r = wave_sum(vacc[64 * (4 * wave + s) + lane]);
        if (lane == 0) red[4 * wave + s] = r;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        const int vb = 4 * rb + threadIdx.x;
        const float* r4 = red + 4 * threadIdx.x;
        if (vb < p.G) p.parts[(long)b * p.G + vb] = r4[0] + r4[1] + r4[2] + r4[3];
    }
}
struct LossFoldParams {
    const float* parts; const int64_t* timesteps; const float* w_table; const float* sample_w;
    float* tracker; float* loss_out; float* per_sample_out;
    long per_sample; int B, T, K, G, w, wlog;                                         // w = 2^wlog fold slots per sample: lw_fold_slots(G)
    float beta;
};
// One block of 128 .. 1024 threads (one per fold slot where they suffice).  The per-sample work (fold, weight, bin) runs in
// parallel; only the two sums and the tracker update are serial, in batch order and on LDS copies, so no global load sits inside
// the serial loop.
template <int = 0>
__global__ __launch_bounds__(1024) void lw_fold_kernel(const LossFoldParams p) {
#pragma clang fp contract(off)
    __shared__ double red[LW_PARTS_MAX];
    __shared__ double sw[LATENT_BATCH_MAX], su[LATENT_BATCH_MAX];                     // w_b l_b and l_b
    __shared__ int bin[LATENT_BATCH_MAX];                                             // the sample's tracker bin, -1: skipped
    __shared__ float trk[2 * LW_BINS_MAX];
    const int slots = p.B * p.w, mask = p.w - 1;                                      // B w <= B lw_cap(B) <= 1024, w a power of two
    for (int s = threadIdx.x; s < slots; s += blockDim.x) {
        const int b = s >> p.wlog, j = s & mask;
        double acc = 0.0;
        for (int i = j; i < p.G; i += p.w) acc += (double)p.parts[(long)b * p.G + i];
        red[s] = acc;
    }
    if (p.tracker && threadIdx.x < 2 * p.K) trk[threadIdx.x] = p.tracker[threadIdx.x];
    __syncthreads();
    for (int o = p.w >> 1; o > 0; o >>= 1) {
        for (int s = threadIdx.x; s < slots; s += blockDim.x)
            if ((s & mask) < o) red[s] += red[s + o];
        __syncthreads();
    }
    if (threadIdx.x < p.B) {
        const int b = threadIdx.x;
        const double l = red[b << p.wlog] / (double)p.per_sample;
        sw[b] = (double)lw_weight(p.timesteps, p.w_table, p.T, p.sample_w, b) * l;
        su[b] = l;
        if (p.per_sample_out) p.per_sample_out[b] = (float)l;
        int k = -1;
        if (p.tracker) {
            const int64_t t = p.timesteps[b];
            if (t >= 0 && t < (int64_t)p.T && __builtin_isfinite(l)) k = (int)((t * (int64_t)p.K) / (int64_t)p.T);
        }
        bin[b] = k;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double sum_w = 0.0, sum_u = 0.0;
        const double beta = (double)p.beta;
        for (int b = 0; b < p.B; ++b) {                                               // batch order: part of the tracker's contract
            sum_w += sw[b];
            sum_u += su[b];
            const int k = bin[b];
            if (k >= 0) {
                const float c = trk[p.K + k];
                const double l2 = su[b] * su[b];
                trk[k] = c == 0.f ? (float)l2 : (float)(beta * (double)trk[k] + (1.0 - beta) * l2);
                if (c < 16777216.f) trk[p.K + k] = c + 1.f;
            }
        }
        p.loss_out[0] = (float)(sum_w / (double)p.B);
        p.loss_out[1] = (float)(sum_u / (double)p.B);
    }
    __syncthreads();
    if (p.tracker && threadIdx.x < 2 * p.K) p.tracker[threadIdx.x] = trk[threadIdx.x];
}
struct ResampleParams {
    const float* tracker; const float* draw; int64_t* t_out; float* iw_out;
    int K, T, warmup, B; float uniform_prob;
    unsigned seed_lo, seed_hi, step;
    int idx[LATENT_BATCH_MAX];
};
__host__ __device__ __forceinline__ int lw_bin_lo(int k, int K, int T) { return (int)(((long)k * T + K - 1) / K); }   // ceil(k T / K)
// Thread k < K prepares bin k (edge, size, q_k = n_k sqrt(m2_k), whether it is still in warm-up); then thread b < B walks the bins.
template <int = 0>
__global__ __launch_bounds__(LATENT_BATCH_MAX) void lw_resample_kernel(const ResampleParams p) {
#pragma clang fp contract(off)
    static_assert(LW_BINS_MAX <= LATENT_BATCH_MAX, "one thread per bin");
    __shared__ double q[LW_BINS_MAX];
    __shared__ int lo_s[LW_BINS_MAX + 1];
    __shared__ int cold[LW_BINS_MAX];
    const int b = threadIdx.x;
    if (b < p.K) {
        const int lo = lw_bin_lo(b, p.K, p.T);
        lo_s[b] = lo;
        q[b] = (double)(lw_bin_lo(b + 1, p.K, p.T) - lo) * sqrt((double)p.tracker[b]);
        cold[b] = (double)p.tracker[p.K + b] < (double)p.warmup;
    }
    if (b == 0) lo_s[p.K] = p.T;
    __syncthreads();
    if (b >= p.B) return;
    float f0, f1;
    if (p.draw) { f0 = p.draw[2 * b]; f1 = p.draw[2 * b + 1]; }
    else {
        unsigned r[4];
        philox4x32_10(0u, (unsigned)p.idx[b], p.step, LATENT_STREAM_TAG + LW_TIMESTEP_STREAM, p.seed_lo, p.seed_hi, r);
        f0 = (float)(r[0] >> 8) * (1.0f / 16777216.0f); f1 = (float)(r[1] >> 8) * (1.0f / 16777216.0f);
    }
    const double u0 = (double)f0, u1 = (double)f1, T = (double)p.T;
    bool uniform = false;
    double sq = 0.0;
    for (int k = 0; k < p.K; ++k) {
        if (cold[k]) uniform = true;
        sq += q[k];
    }
    if (!(sq > 0.0) || !__builtin_isfinite(sq)) uniform = true;
    const double up = (double)p.uniform_prob;
    double C = 0.0, P = 0.0;
    int lo = 0, n = 1;
    for (int k = 0; k < p.K; ++k) {
        lo = lo_s[k]; n = lo_s[k + 1] - lo;
        P = uniform ? (double)n / T : (1.0 - up) * q[k] / sq + up * ((double)n / T);
        C += P;
        if (u0 < C) break;
    }
    int off = (int)floor(u1 * (double)n);
    if (off > n - 1) off = n - 1;
    if (off < 0) off = 0;
    p.t_out[b] = (int64_t)(lo + off);
    p.iw_out[b] = uniform ? 1.0f : (float)((double)n / (T * P));
}
