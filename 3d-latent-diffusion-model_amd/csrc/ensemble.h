// Per-voxel statistics of an ensemble of K member volumes (K draws of the same scan's posterior): a running (mean, m2) state in fp32
// that members are folded into B at a time, and the maps / scalars read off it.  No stack of K volumes exists anywhere.
//
// Recurrence (Welford), per element, members in order b = 0 .. B-1, c = members folded so far:
//   c += 1;  d = x - mean;  mean += d / c;  m2 += d * (x - mean)
// m2 is the sum of squared deviations from the running mean: no sum of squares is formed, so a volume whose values sit at 100 with a
// spread of 0.01 keeps its variance (sum x^2 - (sum x)^2 / K in fp32 loses all of it).  ens_fold is the ONLY copy of that arithmetic:
// contraction is off and the division is IEEE, so every member goes through the same four roundings whatever call it arrives in, on the
// vector path or the scalar one: folding 5 members as 5, 2 + 3 or 1 + 1 + 1 + 1 + 1 gives the same bits.
// count == 0 on entry: the state is not read; the first member sets mean = x, m2 = x - x (0, or NaN for a non-finite x).
//
// ensemble_update_kernel: a thread owns quads of elements (grid-stride); per quad it issues the loads of up to ENS_GROUP members, then
// runs their dependent chains.  A quad is one 16-byte access where everything is 16-byte aligned (vec) and the quad is whole; the last
// n % 4 elements, and every element of a misaligned call, go one float at a time.  HBM-bound: 4 n (B + 4) bytes, 4 n (B + 2) at count 0.
//
// ensemble_finalize_kernel: var = max(m2, 0) / (count - ddof), std = sqrt(var) into std_out (optional); per workgroup one
// EnsPartial {sum std, max std, sum var, sum (mean - target)^2} in double over a fixed LDS tree.  ensemble_stats_kernel (one workgroup,
// a second launch) folds the partials in index order over the same tree.  No atomics: the same inputs give the same bits.  A NaN
// anywhere reaches every scalar: the sums carry it, and the max here propagates it (fmax would drop it).
//
// The three kernels are templates (<>) launched from the end of ldm3d.hip: hipcc emits template kernels behind the plain ones in the order
// of their first instantiation, so they land behind every kernel that was there before and move none of them in the code object.
#pragma once

#define ENS_THREADS 256
#define ENS_GROUP 8                          // members whose loads are in flight before the first dependent chain starts
#define ENS_MAX_BLOCKS 1024                  // of the finalize kernel: ensemble_stats_kernel reads four partials per thread
#define ENS_STATS 8

struct EnsPartial { double sum_std, max_std, sum_var, sum_bias; };

// one member's value x folded into (mean, m2); c = the number of members folded INCLUDING this one
__device__ __forceinline__ void ens_fold(float x, float c, float& mean, float& m2) {
#pragma clang fp contract(off)
    if (c == 1.f) { mean = x; m2 = x - x; return; }
    const float d = x - mean;
    mean = mean + d / c;
    m2 = m2 + d * (x - mean);
}

template <int = 0>
__global__ __launch_bounds__(ENS_THREADS) void ensemble_update_kernel(const float* __restrict__ members, int B, long stride, long n,
                                                                      float* __restrict__ mean, float* __restrict__ m2, int count, int vec) {
    const long nq = (n + 3) / 4;
    for (long q = (long)blockIdx.x * ENS_THREADS + threadIdx.x; q < nq; q += (long)gridDim.x * ENS_THREADS) {
        const long j = 4 * q;
        const int cnt = (int)(n - j < 4 ? n - j : 4);
        const bool v4 = vec && cnt == 4;
        float mu[4] = {0.f, 0.f, 0.f, 0.f}, s[4] = {0.f, 0.f, 0.f, 0.f};
        if (count > 0) {
            if (v4) {
                const float4 a = *reinterpret_cast<const float4*>(mean + j), b = *reinterpret_cast<const float4*>(m2 + j);
                mu[0] = a.x; mu[1] = a.y; mu[2] = a.z; mu[3] = a.w; s[0] = b.x; s[1] = b.y; s[2] = b.z; s[3] = b.w;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) if (e < cnt) { mu[e] = mean[j + e]; s[e] = m2[j + e]; }
            }
        }
        for (int b0 = 0; b0 < B; b0 += ENS_GROUP) {
            const int nb = B - b0 < ENS_GROUP ? B - b0 : ENS_GROUP;
            const float* src = members + (long)b0 * stride + j;
            float x[ENS_GROUP][4];
#pragma unroll
            for (int g = 0; g < ENS_GROUP; ++g) {
                if (g < nb) {
                    const float* p = src + (long)g * stride;
                    if (v4) { const float4 t = *reinterpret_cast<const float4*>(p); x[g][0] = t.x; x[g][1] = t.y; x[g][2] = t.z; x[g][3] = t.w; }
                    else {
#pragma unroll
                        for (int e = 0; e < 4; ++e) x[g][e] = e < cnt ? p[e] : 0.f;
                    }
                }
            }
#pragma unroll
            for (int g = 0; g < ENS_GROUP; ++g) {
                if (g < nb) {
                    const float c = (float)(count + b0 + g + 1);
#pragma unroll
                    for (int e = 0; e < 4; ++e) ens_fold(x[g][e], c, mu[e], s[e]);
                }
            }
        }
        if (v4) {
            *reinterpret_cast<float4*>(mean + j) = make_float4(mu[0], mu[1], mu[2], mu[3]);
            *reinterpret_cast<float4*>(m2 + j) = make_float4(s[0], s[1], s[2], s[3]);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) if (e < cnt) { mean[j + e] = mu[e]; m2[j + e] = s[e]; }
        }
    }
}

// fixed-order fold of one double per thread: sum (op 0) or a maximum that keeps a NaN (op 1); result valid in thread 0
__device__ __forceinline__ double ens_max(double a, double b) { return (b > a || b != b) ? b : a; }
__device__ __forceinline__ double ens_block_fold(double v, double* red, int op) {
    const int tid = threadIdx.x;
    __syncthreads();
    red[tid] = v;
    __syncthreads();
    for (int s = ENS_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) {
            const double a = red[tid], b = red[tid + s];
            red[tid] = op == 0 ? a + b : ens_max(a, b);
        }
        __syncthreads();
    }
    return red[0];
}

// the finalize kernel's workgroups: a function of n alone
static inline int ens_blocks(long n) {
    const long nq = (n + 3) / 4;
    long nb = (nq + 4 * ENS_THREADS - 1) / (4 * ENS_THREADS);
    return (int)(nb < 1 ? 1 : nb > ENS_MAX_BLOCKS ? ENS_MAX_BLOCKS : nb);
}

__device__ __forceinline__ void ens_var_std(float m2, float denom, float& var, float& sd) {
#pragma clang fp contract(off)
    var = (m2 < 0.f ? 0.f : m2) / denom;              // not fmaxf: a NaN stays
    sd = sqrtf(var);
}

template <int = 0>
__global__ __launch_bounds__(ENS_THREADS) void ensemble_finalize_kernel(const float* __restrict__ mean, const float* __restrict__ m2,
                                                                        const float* __restrict__ target, float* __restrict__ std_out,
                                                                        EnsPartial* __restrict__ partial, long n, float denom, int vec) {
    __shared__ double red[ENS_THREADS];
    const long nq = (n + 3) / 4;
    double ssd = 0.0, svar = 0.0, sbias = 0.0, mx = 0.0;              // std >= 0: 0 is the maximum's identity
    for (long q = (long)blockIdx.x * ENS_THREADS + threadIdx.x; q < nq; q += (long)gridDim.x * ENS_THREADS) {
        const long j = 4 * q;
        const int cnt = (int)(n - j < 4 ? n - j : 4);
        const bool v4 = vec && cnt == 4;
        float s[4] = {0.f, 0.f, 0.f, 0.f}, mu[4] = {0.f, 0.f, 0.f, 0.f}, tg[4] = {0.f, 0.f, 0.f, 0.f}, sd[4];
        if (v4) {
            const float4 a = *reinterpret_cast<const float4*>(m2 + j);
            s[0] = a.x; s[1] = a.y; s[2] = a.z; s[3] = a.w;
            if (target) {
                const float4 b = *reinterpret_cast<const float4*>(mean + j), c = *reinterpret_cast<const float4*>(target + j);
                mu[0] = b.x; mu[1] = b.y; mu[2] = b.z; mu[3] = b.w; tg[0] = c.x; tg[1] = c.y; tg[2] = c.z; tg[3] = c.w;
            }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) if (e < cnt) { s[e] = m2[j + e]; if (target) { mu[e] = mean[j + e]; tg[e] = target[j + e]; } }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float var;
            ens_var_std(s[e], denom, var, sd[e]);
            if (e < cnt) {
                ssd += (double)sd[e]; svar += (double)var; mx = ens_max(mx, (double)sd[e]);
                const double df = (double)mu[e] - (double)tg[e];
                sbias = fma(df, df, sbias);
            }
        }
        if (std_out) {
            if (v4) *reinterpret_cast<float4*>(std_out + j) = make_float4(sd[0], sd[1], sd[2], sd[3]);
            else {
#pragma unroll
                for (int e = 0; e < 4; ++e) if (e < cnt) std_out[j + e] = sd[e];
            }
        }
    }
    const double f0 = ens_block_fold(ssd, red, 0), f1 = ens_block_fold(mx, red, 1), f2 = ens_block_fold(svar, red, 0),
                 f3 = ens_block_fold(sbias, red, 0);
    if (threadIdx.x == 0) { EnsPartial r; r.sum_std = f0; r.max_std = f1; r.sum_var = f2; r.sum_bias = f3; partial[blockIdx.x] = r; }
}

// stats[0..8) = {mean std, max std, mean var, mean (mean - target)^2 (0 without a target), 0, 0, 0, 0}; partials folded in index order
template <int = 0>
__global__ __launch_bounds__(ENS_THREADS) void ensemble_stats_kernel(const EnsPartial* __restrict__ partial, int nb, double n, int has_target,
                                                                     float* __restrict__ stats) {
    __shared__ double red[ENS_THREADS];
    const int tid = threadIdx.x;
    double ssd = 0.0, svar = 0.0, sbias = 0.0, mx = 0.0;
    for (int i = tid; i < nb; i += ENS_THREADS) {
        const EnsPartial r = partial[i];
        ssd += r.sum_std; svar += r.sum_var; sbias += r.sum_bias; mx = ens_max(mx, r.max_std);
    }
    ssd = ens_block_fold(ssd, red, 0); mx = ens_block_fold(mx, red, 1); svar = ens_block_fold(svar, red, 0); sbias = ens_block_fold(sbias, red, 0);
    if (tid == 0) {
        stats[0] = (float)(ssd / n); stats[1] = (float)mx; stats[2] = (float)(svar / n); stats[3] = has_target ? (float)(sbias / n) : 0.f;
        stats[4] = 0.f; stats[5] = 0.f; stats[6] = 0.f; stats[7] = 0.f;
    }
}
