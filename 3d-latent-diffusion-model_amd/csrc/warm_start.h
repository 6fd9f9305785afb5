// Warm-start sampling (ldm_sampler_seek / ldm_sampler_start / ldm_sampler_start_noise): a chain that begins at row k0 of its sampler's
// table from a given latent z0 instead of at row 0 from pure noise (SDEdit; with DDIM inversion the start is computed by the step
// kernels themselves on an ascending row table and only the seek below is needed).
//
//   seek   counter := k0, done := 0, tbuf[0..B) := t of row k0: sampler_reset_kernel at another row.  The Philox step index of a
//          stochastic step is the ROW index (sampler_step_loop passes the counter), so step k of a warm chain draws the z that step k
//          of the full chain draws.
//   start  x[b] = a z0[b or 0] + s e[b], one pass, four elements per thread:
//            DDPM / DDIM rows  a = row[6] = sqrt(abar_t), s = row[1] = sqrt(1 - abar_t)
//            flow rows         s = row[1] = tau, a = 1 - tau, the subtraction in fp32 here
//          rounded as one multiply and one fused multiply-add, fma(a, z0, s * e); contraction is off.  z0_batch == 1 broadcasts the one
//          start latent to the B members without a copy.  x may alias z0 only when z0_batch == B: every thread reads its quad of z0 before
//          it writes that quad of x and no other thread touches it.
//   noise  e explicit ([B][per_sample]) or, DRAW, Philox4x32-10 + philox_normal4 with
//            counter = (quad within the sample: low word, high word, first_member + b, WARM_START_STREAM_TAG), key = (seed_lo, seed_hi);
//          lane e of a block is element 4 * quad + e of the sample.  A draw is a function of (seed, global member index, element) alone:
//          not of the chunk the member runs in.  Counter word 3 differs from the sampler's 0x5eed and from LATENT_STREAM_TAG + 0 .. 4, so
//          the streams of one seed do not meet.
// The kernels are templates so that they are emitted behind the ones that were here before them (see rflow_noise_target_kernel).
#pragma once

#define WARM_START_STREAM_TAG 0x57a27000u
static_assert(WARM_START_STREAM_TAG != 0x5eedu && (WARM_START_STREAM_TAG < LATENT_STREAM_TAG || WARM_START_STREAM_TAG > LATENT_STREAM_TAG + 4u),
              "the start draws need a Philox stream of their own");

// stride: floats per coefficient row (8, or PNDM_ROW where k0 is 0); t sits in slot 5 of either
template <int = 0>
__global__ void sampler_seek_kernel(SamplerState* st, const float* coef, int stride, int k0, float* tbuf, int B) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        st->k = k0; st->done = 0;
        const float t = coef[(size_t)k0 * stride + 5];
        for (int b = 0; b < B; ++b) tbuf[b] = t;
    }
}

struct WarmStartParams {
    const float* z0; const float* noise; float* x;          // z0 [z0_batch][per_sample], noise [B][per_sample] (unused with DRAW), x [B][per_sample]
    const float* row;                                        // row k0 of the sampler's device table (8 floats)
    long per_sample; int B; int z0_batch; int vec; int flow; // vec: per_sample % 4 == 0 and every pointer 16-byte aligned
    unsigned seed_lo, seed_hi, first_member;
};
__device__ __forceinline__ float4 warm_start_normal4(long quad, unsigned member, unsigned seed_lo, unsigned seed_hi) {
    return philox_normal4((unsigned)quad, (unsigned)((unsigned long long)quad >> 32), member, WARM_START_STREAM_TAG, seed_lo, seed_hi);
}
template <bool DRAW>
__global__ __launch_bounds__(256) void warm_start_kernel(const WarmStartParams p) {
#pragma clang fp contract(off)
    float a, s;
    if (p.flow) { s = p.row[1]; a = 1.0f - s; }
    else { a = p.row[6]; s = p.row[1]; }
    const long nqs = (p.per_sample + 3) / 4, nq = nqs * p.B;
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (long)gridDim.x * blockDim.x) {
        const int b = (int)(q / nqs);
        const long qs = q - (long)b * nqs, e0 = 4 * qs, left = p.per_sample - e0;
        const int cnt = left < 4 ? (int)left : 4;
        const long src = (p.z0_batch == 1 ? 0 : (long)b * p.per_sample) + e0, dst = (long)b * p.per_sample + e0;
        float zv[4], nv[4], out[4];
        latent_load4(p.z0 + src, cnt, p.vec, zv);
        if constexpr (DRAW) {
            const float4 d = warm_start_normal4(qs, p.first_member + (unsigned)b, p.seed_lo, p.seed_hi);
            nv[0] = d.x; nv[1] = d.y; nv[2] = d.z; nv[3] = d.w;
        } else latent_load4(p.noise + dst, cnt, p.vec, nv);
#pragma unroll
        for (int e = 0; e < 4; ++e) out[e] = __fmaf_rn(a, zv[e], s * nv[e]);
        latent_store4(p.x + dst, cnt, p.vec, out);
    }
}
// the draws of one member, as warm_start_kernel<true> makes them
template <int = 0>
__global__ __launch_bounds__(256) void warm_start_noise_kernel(float* out, long per_sample, unsigned member, unsigned seed_lo, unsigned seed_hi) {
    const long nqs = (per_sample + 3) / 4;
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < nqs; q += (long)gridDim.x * blockDim.x) {
        const float4 d = warm_start_normal4(q, member, seed_lo, seed_hi);
        const float dd[4] = {d.x, d.y, d.z, d.w};
        for (int e = 0; e < 4; ++e) if (4 * q + e < per_sample) out[4 * q + e] = dd[e];
    }
}
