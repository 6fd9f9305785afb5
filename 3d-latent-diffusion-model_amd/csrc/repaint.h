// Inpainting on the device sampler (RePaint, Lugmayr et al. 2022, Alg. 1): a chain that keeps the trusted part of a latent and
// regenerates the rest.  ldm_sampler_create_repaint / ldm_sampler_bind_known / ldm_sampler_repaint_noise / ldm_repaint_merge.
//
// A repaint chain is a row table like any other, one REPAINT_ROW-float row per UNet call, whose timesteps need not fall: after the
// chain has arrived at some levels it jumps back towards noise and denoises again (resampling), which is what lets the regenerated
// region agree with the kept one.  sampler_advance reads the next t from slot 5 of the next row whatever its order.  Row:
//   [0..7]   the base scheduler's own sampler row (DDPM / DDIM: sampler_coef, rectified flow: flow_coef); slot 5 is t
//   [8] ka  [9] ks    the known region at the level the step arrives at: ka known + ks z_known   (last level: 1, 0)
//   [10] ja [11] js   the jump back from that level: ja x + js z_jump, only with the jump flag    (no jump: 1, 0)
//   [12]     flags, 1 = jump;  [13..15] 0
// Per element i of row k, with xn the base family's update (sampler_update<PRED> / flow_update, the same device functions as the plain
// step kernels) and x0_out its x0_hat, taken before the merge:
//   keep[i % DHW] != 0:  xn = fma(ka, known[known_batch == 1 ? i % per_sample : i], ks * z_known)      ks == 0: xn = ka * known, no draw
//   jump:                xn = fma(ja, xn, js * z_jump)                                                    js == 0: xn = ja * xn, no draw
// repaint_merge_jump is the only copy of that arithmetic: shared by the fused step kernels and the host-driven repaint_merge_kernel,
// which must agree bit for bit; contraction is off and every rounding is spelled out, as in warm_start_kernel.
// Noise: the step noise stays the sampler's stream (counter word 3 = 0x5eed) with the ROW index k as its step, so a resampled pass over
// the same timestep draws afresh; z_known and z_jump are two more Philox4x32-10 streams,
//   counter = (quad: low word, high word, k, REPAINT_KNOWN_STREAM_TAG | REPAINT_JUMP_STREAM_TAG), key = (seed_lo, seed_hi),
// drawn per quad of the flat index like the step noise: at most three Philox blocks are live per quad.
// keep is fp32 [DHW], shared by channels and samples; known is fp32 [known_batch][per_sample], one latent broadcast when known_batch == 1.
// The existing step kernels keep their argument record (StepParams) and their loop: this family has a loop of its own built from the
// same pieces (the rule's update functions, the Source functors, sampler_advance).  The kernels are templates and are launched from
// the end of the translation unit so that they are emitted behind the ones that were here before them.
#pragma once

#define REPAINT_KNOWN_STREAM_TAG 0x4e9a1701u
#define REPAINT_JUMP_STREAM_TAG 0x4e9a1702u
constexpr bool repaint_tag_free(unsigned tag) {
    return tag != 0x5eedu && tag != WARM_START_STREAM_TAG && (tag < LATENT_STREAM_TAG || tag > LATENT_STREAM_TAG + 4u);
}
static_assert(REPAINT_KNOWN_STREAM_TAG != REPAINT_JUMP_STREAM_TAG && repaint_tag_free(REPAINT_KNOWN_STREAM_TAG) &&
              repaint_tag_free(REPAINT_JUMP_STREAM_TAG), "the known-region and jump draws need Philox streams of their own");

enum { REPAINT_ROW = 16 };
struct RepaintCoef { float ka, ks, ja, js; int jump; };
// slots 8 .. 12 of a row
__host__ __device__ __forceinline__ RepaintCoef repaint_coef(const float* row) {
    return RepaintCoef{row[8], row[9], row[10], row[11], row[12] != 0.f ? 1 : 0};
}
// The one argument record of a repaint step: the plain step's record and the bound known latent and keep mask.
struct RepaintParams {
    StepParams s;
    const float* known; const float* keep;                   // known [known_batch][per_sample], keep [dhw]
    long per_sample, dhw; int known_batch;                    // s.n = samples * per_sample, per_sample = C * dhw
};
__device__ __forceinline__ float4 repaint_normal4(long quad, unsigned row, unsigned tag, unsigned seed_lo, unsigned seed_hi) {
    return philox_normal4((unsigned)quad, (unsigned)((unsigned long long)quad >> 32), row, tag, seed_lo, seed_hi);
}
// Merge and jump of one element: xn is the base rule's new value, kn the known latent's element (read only where kept).
__device__ __forceinline__ float repaint_merge_jump(const RepaintCoef& c, float xn, bool kept, float kn, float zk, float zj) {
#pragma clang fp contract(off)
    if (kept) xn = c.ks != 0.f ? __fmaf_rn(c.ka, kn, c.ks * zk) : c.ka * kn;
    if (c.jump) xn = c.js != 0.f ? __fmaf_rn(c.ja, xn, c.js * zj) : c.ja * xn;
    return xn;
}
// The repaint step loop: sampler_step_loop with up to three draws per quad and the merge behind the base rule's update.  FAMILY is
// STEP_DDPM (DDPM and DDIM) or STEP_FLOW; `src` is the Source of the plain loop (StepDirect, StepWindows).  Beyond the end of the
// chain no element is touched and the counter stays.
template <int PRED, int FAMILY, class Source>
__device__ __forceinline__ void repaint_step_loop(const RepaintParams& rp, const Source& src) {
    static_assert(FAMILY == STEP_DDPM || FAMILY == STEP_FLOW, "repaint: DDPM / DDIM or rectified flow");
    const StepParams& p = rp.s;
    const int k = p.st->k;                                  // every block reads the counter before it can bump `done`
    const bool live = k < p.n_steps;
    const float* row = p.coef + (size_t)(live ? k : p.n_steps - 1) * REPAINT_ROW;
    const SamplerCoef sc = sampler_coef<PRED>(row, 0, 1);
    const FlowCoef fc = flow_coef(row, 0, 1);
    const RepaintCoef rc = repaint_coef(row);
    const bool draw_step = FAMILY == STEP_DDPM && sc.sigma != 0.f, draw_known = rc.ks != 0.f, draw_jump = rc.jump && rc.js != 0.f;
    const long nq = (p.n + 3) / 4;
    const unsigned bdim = __builtin_amdgcn_workgroup_size_x();
    if (live)
    for (long q = (long)blockIdx.x * bdim + threadIdx.x; q < nq; q += (long)gridDim.x * bdim) {
        float4 z = make_float4(0.f, 0.f, 0.f, 0.f), zk = z, zj = z;
        if (draw_step) z = sampler_normal4((unsigned long long)q, (unsigned)k, p.seed_lo, p.seed_hi);
        if (draw_known) zk = repaint_normal4(q, (unsigned)k, REPAINT_KNOWN_STREAM_TAG, p.seed_lo, p.seed_hi);
        if (draw_jump) zj = repaint_normal4(q, (unsigned)k, REPAINT_JUMP_STREAM_TAG, p.seed_lo, p.seed_hi);
        const float zz[4] = {z.x, z.y, z.z, z.w}, zzk[4] = {zk.x, zk.y, zk.z, zk.w}, zzj[4] = {zj.x, zj.y, zj.z, zj.w};
        long iv = (4 * q) % rp.dhw;                         // voxel of the quad's first element; the elements after it wrap
        long is = rp.known_batch == 1 ? (4 * q) % rp.per_sample : 4 * q;   // its element of the known latent
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const long i = 4 * q + e;
            if (i >= p.n) break;
            src(p, i, [&](float m) {
                float x0, xn;
                if constexpr (FAMILY == STEP_FLOW) xn = flow_update(fc, p.x[i], m, &x0);
                else xn = sampler_update<PRED>(sc, p.kind, p.clip, p.x[i], m, zz[e], &x0);
                if (p.x0_out) p.x0_out[i] = x0;
                const bool kept = rp.keep[iv] != 0.f;
                xn = repaint_merge_jump(rc, xn, kept, kept ? rp.known[is] : 0.f, zzk[e], zzj[e]);
                p.x[i] = xn;
                return xn;
            });
            if (++iv == rp.dhw) iv = 0;
            if (++is == rp.per_sample && rp.known_batch == 1) is = 0;
        }
    }
    sampler_advance(p.st, p.coef, p.n_steps, k, p.tbuf, p.B, REPAINT_ROW);
}
template <int PRED, int FAMILY>
__global__ __launch_bounds__(256) void repaint_step_kernel(const RepaintParams rp) {
    repaint_step_loop<PRED, FAMILY>(rp, StepDirect{});
}
template <int PRED, int FAMILY>
__global__ __launch_bounds__(256) void repaint_window_step_kernel(const WinGeom g, const RepaintParams rp) {   // rp.s.n = C * dim[0] * dim[1] * dim[2]
    repaint_step_loop<PRED, FAMILY>(rp, StepWindows{g});
}
// The host-driven merge and jump on explicit draws (ldm_repaint_merge): the coefficients by value; zk / zj null where their
// coefficient is 0.  out may alias x: a thread reads element i before it writes it and no other thread touches it.
struct RepaintMergeParams {
    const float* x; const float* known; const float* keep; const float* zk; const float* zj; float* out;
    long n, per_sample, dhw; int known_batch; RepaintCoef c;
};
template <int = 0>
__global__ __launch_bounds__(256) void repaint_merge_kernel(const RepaintMergeParams p) {
    const long nq = (p.n + 3) / 4;
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (long)gridDim.x * blockDim.x) {
        long iv = (4 * q) % p.dhw;
        long is = p.known_batch == 1 ? (4 * q) % p.per_sample : 4 * q;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const long i = 4 * q + e;
            if (i >= p.n) break;
            const bool kept = p.keep[iv] != 0.f;
            p.out[i] = repaint_merge_jump(p.c, p.x[i], kept, kept ? p.known[is] : 0.f, p.zk ? p.zk[i] : 0.f, p.zj ? p.zj[i] : 0.f);
            if (++iv == p.dhw) iv = 0;
            if (++is == p.per_sample && p.known_batch == 1) is = 0;
        }
    }
}
// the draws of one row on one of the two streams, as repaint_step_loop makes them
template <int = 0>
__global__ __launch_bounds__(256) void repaint_noise_kernel(float* out, long n, unsigned row, unsigned tag, unsigned seed_lo, unsigned seed_hi) {
    const long nq = (n + 3) / 4;
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (long)gridDim.x * blockDim.x) {
        const float4 d = repaint_normal4(q, row, tag, seed_lo, seed_hi);
        const float dd[4] = {d.x, d.y, d.z, d.w};
        for (int e = 0; e < 4; ++e) if (4 * q + e < n) out[4 * q + e] = dd[e];
    }
}
