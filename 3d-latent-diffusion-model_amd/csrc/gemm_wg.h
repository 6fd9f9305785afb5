// The light GEMM (gemm_light.h) on operand tiles that a workgroup SHARES in LDS: out[m][co] = sum_k x[m][k] * w[co][k] + bias (+ residual),
// one source, K = 128 .. 512 in steps of 128 (the attention projections and the im2col first conv).
//
// gemm_light_kernel's waves each pull both operands of their tile through the vector L1 into registers, in dependent chunk round trips.
// Here a workgroup of 2 or 4 waves copies its (16 MT) rows of x and its 64 or 128 weight rows over the WHOLE K range into LDS by LDS-DMA
// in one burst (weights first: the bytes that come from HBM), waits once (vmcnt(0) per wave, one raw barrier) and runs every K step out
// of LDS.  Each wave owns all rows of the tile and 32 couts, so a row of x is fetched once per 64 / 128 couts instead of once per 32 / 64.
//
// Results equal gemm_light_kernel's bit for bit: one accumulator per 16 x 16 output tile, the 32-deep K steps in ascending order, lane
// group fg holding k = 8 fg .. + 7 of a step, and the same epilogue (light_epilogue: a lane sums its rows in tile order, then the DPP row
// rotation), so a GroupNorm partial row is the same sum in the same order whichever kernel wrote it.
//
// LDS image, per operand: [128-channel block kb][row][16 chunks of 16 B]; chunk c of row r sits in slot c ^ (r & 15).  One ds_read_b128
// lane group (MI355X: {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32) holds all 16 fragment rows fr, with fg = b for the rows
// of some 4-aligned blocks and b + 1 for the others; two lanes meet in a slot only if fr1 ^ fr2 == fg1 ^ fg2, i.e. 1, and fr ^ 1 lies in
// fr's own block where fg is equal: conflict-free.  The swizzle is applied on the source side: lane i of a copy writes LDS slot i of its
// 1 KiB piece (4 rows x 256 B) and picks which global 16-byte chunk to fetch.  Weight rows are stored in fragment order (LDS row
// 32 wave + 16 nt + f <-> cout 32 wave + 8 (f >> 2) + 4 nt + (f & 3), the MFMA row order of light_epilogue's lane <-> cout map), so the
// rows of a fragment read are 16 consecutive LDS rows for both operands.  Rows past M and couts past CoutPad lie beyond the buffer
// descriptors' ranges: the copy writes zeros, and the epilogue drops them.
//
// GN = true: GroupNorm (no activation) of x folded into the prologue, for a q|k|v projection whose input's producer left `nrb` <= 16 partial
// (sum, sum of squares) rows per sample (WgGnParams).  x is then the UN-normalised tensor: every workgroup folds the slabs of all K channels
// of the (at most two) samples its rows belong to -- loads requested before the operand burst, summed in gn_fold_cover's order (fp32 per slab
// lane b % 8, rows ascending; fp64 over the 8 lanes; fp64 over a group's channels, statistics as gn_fused_fold) -- forms a = gamma rstd,
// b = beta - mean a, and rewrites its x tile in LDS in place between the barrier and the first fragment read with gn_fused_apply_kernel's
// expression and rounding.  The normalised tensor never exists in memory, and equals that kernel's output bit for bit.
#pragma once
#include "conv_cube.h"                 // cube_barrier()
#include "gemm_light.h"

struct WgGnParams {
    const float* slabs;                   // [N * nrb][K][2] partial rows of x
    const float* gamma; const float* beta;
    int nrb, groups, DHW; float eps;      // K % groups == 0, K / groups even and <= 64, groups <= 128, DHW >= rows of the tile
};

__device__ __forceinline__ void wg_copies_landed_barrier() {   // this wave's copies, then everybody's: nothing else orders a ds_read behind another wave's LDS-DMA
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// workgroup tile = (16 MT) rows x (32 NWV) couts, NWV waves; grid mtiles * ceil(CoutPad / (32 NWV)), mtile fastest.  Dynamic LDS (16 MT + 32 NWV) * 2 K bytes.
template <int MT, int NWV, bool GN>
__global__ __launch_bounds__(64 * NWV) void gemm_wg_kernel(const LightParams p, const int cout_pad, const WgGnParams g) {
#if defined(__HIP_DEVICE_COMPILE__)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    typedef __attribute__((address_space(3))) void* lds_ptr_t;
    constexpr int NT = 2, R = 16 * MT, NW = 32 * NWV;
    const int tid = threadIdx.x, lane = tid & 63, fr = lane & 15, fg = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int mtile = blockIdx.x % p.mtiles, ntile = blockIdx.x / p.mtiles;       // mtile fastest: neighbours share the weight rows
    const int m0 = mtile * R, n0 = ntile * NW;
    const int nkb = p.K >> 7;                                                     // 128-channel blocks
    const unsigned row2 = (unsigned)p.K * 2u;
    const int xbase = nkb * NW * 256;                                             // weights at 0, x behind them

    // ---- GN: slab rows of this thread's first channel pair and its gamma / beta, requested ahead of the burst (loads return in order)
    constexpr int T = 64 * NWV;
    const int C = p.K;
    int ns0 = 0, ns1 = 0;                                                         // samples of the tile's rows
    float4 t[16]; float gm[4], bt[4];
    float* const ab = reinterpret_cast<float*>(smem + nkb * (NW + R) * 256);      // [2][C][2] scale / shift
    double* const csum = reinterpret_cast<double*>(ab + 4 * C);                   // [C][2] channel totals
    float* const gstat = reinterpret_cast<float*>(csum + 2 * C);                  // [groups][2] mean, rstd
    auto slab_loads = [&](const int smp, const int pp) {
        const float* base = g.slabs + ((size_t)smp * g.nrb * C + 2 * pp) * 2;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            int bb = k; const bool ok = bb < g.nrb; if (!ok) bb = g.nrb - 1;      // clamped: unconditional loads stay in flight together
            t[k] = *reinterpret_cast<const float4*>(base + (size_t)bb * C * 2);
            if (!ok) t[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    if constexpr (GN) {
        ns0 = m0 / g.DHW;
        int ml = m0 + R - 1; if (ml > p.M - 1) ml = p.M - 1;
        ns1 = ml / g.DHW;
        if (tid < (C >> 1)) slab_loads(ns0, tid);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = tid + j * T;
            gm[j] = c < C ? g.gamma[c] : 0.f; bt[j] = c < C ? g.beta[c] : 0.f;
        }
    }

    // ---- copies: piece u = block u / (rows / 4), rows 4 (u % (rows / 4)) .. + 3; lane = (row lane >> 4, slot lane & 15)
    {
        __amdgpu_buffer_rsrc_t rs_w = __builtin_amdgcn_make_buffer_rsrc((void*)p.w, 0, (int)((unsigned)cout_pad * row2), 0x00020000);
        for (int u = wave; u < nkb * (NW / 4); u += NWV) {
            const int kb = u / (NW / 4), lr = 4 * (u % (NW / 4)) + (lane >> 4), f = lr & 15;
            const int co = n0 + (lr & ~31) + 8 * (f >> 2) + 4 * ((lr >> 4) & 1) + (f & 3);
            const unsigned vo = (unsigned)co * row2 + (unsigned)kb * 256u + (unsigned)((lane & 15) ^ f) * 16u;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_w, (lds_ptr_t)(smem + u * 1024), 16, vo, 0, 0, 0);
        }
        __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc((void*)p.x, 0, (int)((unsigned)p.M * row2), 0x00020000);
        for (int u = wave; u < nkb * (R / 4); u += NWV) {
            const int kb = u / (R / 4), lr = 4 * (u % (R / 4)) + (lane >> 4);
            const unsigned vo = (unsigned)(m0 + lr) * row2 + (unsigned)kb * 256u + (unsigned)((lane & 15) ^ (lr & 15)) * 16u;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_x, (lds_ptr_t)(smem + xbase + u * 1024), 16, vo, 0, 0, 0);
        }
    }
    // fragment addressing under the copies' round trip: row 16 t + fr of a block, slot (4 j + fg) ^ fr in K step 4 kb + j
    const int n0w = n0 + 32 * wave;
    const int wrow = (32 * wave + fr) * 256, xrow = xbase + fr * 256;
    f32x4 acc[NT][MT];
#pragma unroll
    for (int a = 0; a < NT; ++a)
#pragma unroll
        for (int b = 0; b < MT; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if constexpr (GN) {
        const int cpg = C / g.groups;
        for (int smp = ns0; smp <= ns1; ++smp) {
            for (int pp = tid; pp < (C >> 1); pp += T) {
                if (smp != ns0 || pp != tid) slab_loads(smp, pp);
                double s0 = 0.0, q0 = 0.0, s1 = 0.0, q1 = 0.0;
#pragma unroll
                for (int k = 0; k < 8; ++k) {                                     // slab lane k: rows k, k + 8 in fp32, then the lanes in fp64
                    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
                    a.x += t[k].x; a.y += t[k].y; a.z += t[k].z; a.w += t[k].w;
                    a.x += t[k + 8].x; a.y += t[k + 8].y; a.z += t[k + 8].z; a.w += t[k + 8].w;
                    s0 += (double)a.x; q0 += (double)a.y; s1 += (double)a.z; q1 += (double)a.w;
                }
                csum[4 * pp] = s0; csum[4 * pp + 1] = q0; csum[4 * pp + 2] = s1; csum[4 * pp + 3] = q1;
            }
            cube_barrier();
            if (tid < g.groups) {
                double s = 0.0, q = 0.0;
                for (int k = 0; k < cpg; ++k) { s += csum[(tid * cpg + k) * 2]; q += csum[(tid * cpg + k) * 2 + 1]; }
                const double cnt = (double)cpg * (double)g.DHW;
                const double mean = s / cnt;
                double var = q / cnt - mean * mean; if (var < 0.0) var = 0.0;
                const float rstd = (float)(1.0 / sqrt(var + (double)g.eps));
                gstat[2 * tid] = (float)mean; gstat[2 * tid + 1] = rstd;
            }
            cube_barrier();
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = tid + j * T;
                if (c < C) {
                    const int gi = c / cpg;
                    const float a = gm[j] * gstat[2 * gi + 1];
                    const float b = bt[j] - gstat[2 * gi] * a;
                    ab[((smp - ns0) * C + c) * 2] = a; ab[((smp - ns0) * C + c) * 2 + 1] = b;
                }
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
    wg_copies_landed_barrier();
    if constexpr (GN) {
        // ---- normalise the x tile in place: 16-byte slot q of the image = (block, row, slot), channels 128 kb + 8 (slot ^ (row & 15)) .. + 7
        const int split = (ns0 + 1) * g.DHW;                                      // first row of the tile's second sample
        for (int q = tid; q < nkb * R * 16; q += T) {
            const int slot = q & 15, lr = (q >> 4) & (R - 1), kb = q / (16 * R);
            const int m = m0 + lr;
            if (m >= p.M) continue;                                               // zero rows stay zero: dropped by the epilogue
            const int ch = kb * 128 + ((slot ^ (lr & 15)) << 3);
            const float4* abp = reinterpret_cast<const float4*>(ab + ((m >= split ? C : 0) + ch) * 2);
            u32x4* xp = reinterpret_cast<u32x4*>(smem + xbase + q * 16);
            const u32x4 v = *xp;
            u32x4 o;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float4 e = abp[j];
                const float lo = __uint_as_float(v[j] << 16) * e.x + e.y;
                const float hi = __uint_as_float(v[j] & 0xffff0000u) * e.z + e.w;
                o[j] = pack2bf(lo, hi);
            }
            *xp = o;
        }
        cube_barrier();
    }
    if (n0w >= cout_pad) return;                                                  // a wave past the last weight row (CoutPad % (32 NWV) != 0)

    bf16x8 wa[NT], xa[MT], wb[NT], xb[MT];                                        // two K steps of fragments
    const int nsteps = p.K >> 5;
#define GW_LOAD(WF, XF, S) do {                                                                       \
        int s_ = (S); if (s_ >= nsteps) s_ = nsteps - 1;              /* unconditional (clamped) */   \
        const int kb_ = s_ >> 2, so_ = ((4 * (s_ & 3) + fg) ^ fr) * 16;                               \
        const char* wp_ = smem + wrow + kb_ * (NW * 256) + so_;                                       \
        const char* xp_ = smem + xrow + kb_ * (R * 256) + so_;                                        \
        _Pragma("unroll") for (int nt = 0; nt < NT; ++nt) WF[nt] = *reinterpret_cast<const bf16x8*>(wp_ + nt * 4096); \
        _Pragma("unroll") for (int mt = 0; mt < MT; ++mt) XF[mt] = *reinterpret_cast<const bf16x8*>(xp_ + mt * 4096); \
    } while (0)
#define GW_MFMA(WF, XF) do {                                                                          \
        _Pragma("unroll") for (int nt = 0; nt < NT; ++nt)                                             \
            _Pragma("unroll") for (int mt = 0; mt < MT; ++mt)                                         \
                acc[nt][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(WF[nt], XF[mt], acc[nt][mt], 0, 0, 0); \
    } while (0)
    GW_LOAD(wa, xa, 0);
    for (int s = 0; s < nsteps; s += 2) {                                         // nsteps % 4 == 0
        GW_LOAD(wb, xb, s + 1);
        GW_MFMA(wa, xa);
        GW_LOAD(wa, xa, s + 2);
        GW_MFMA(wb, xb);
    }
#undef GW_LOAD
#undef GW_MFMA
    light_epilogue<MT, NT>(p, acc, mtile, m0, n0w, fr, fg);
#endif
}

// one source, K = 128 .. 512 in steps of 128 (whole 128-channel blocks; 64 rows + 128 couts of K = 384 or 64 + 64 of K = 512 fill 144 / 128 KiB of LDS).
// LDM_GEMM_WG=0: every light GEMM on gemm_light_kernel.  Read per plan / operator call.
static inline bool gemm_wg_ok(bool single_source, int K, long M) {
    return ldm_knob("LDM_GEMM_WG", 1) != 0 && single_source && K % 128 == 0 && K >= 128 && K <= 512 && M * (long)K * 2 < (1L << 31);
}
// LDS beside the operand tiles with the GroupNorm prologue: scale / shift of two samples, fp64 channel totals, group statistics
static inline int gemm_wg_gn_lds(int K, int groups) { return 32 * K + 8 * groups; }
static inline int gemm_wg_rows(int big) { return big ? 64 : 32; }
static inline int gemm_wg_couts(int big, int K) { return big && K <= 384 ? 128 : 64; }
// the GroupNorm prologue: a shape gemm_wg_ok() admits with K >= 256, few slab rows, whole even groups, tiles within two samples, LDS.
// LDM_GEMM_WG_GN=0: the plans keep gn_fused_apply_kernel in front of the q|k|v GEMM.  Read per plan.
static inline bool gemm_wg_gn_shape_ok(int K, long DHW, int groups, int nrb, int big) {
    return K >= 256 && groups >= 1 && groups <= 128 && K % groups == 0 && (K / groups) % 2 == 0 && K / groups <= 64 && nrb >= 1 && nrb <= 16 &&
           DHW >= gemm_wg_rows(big) && (gemm_wg_rows(big) + gemm_wg_couts(big, K)) * 2 * K + gemm_wg_gn_lds(K, groups) <= 160 * 1024;
}
static inline bool gemm_wg_gn_ok(int K, long DHW, int groups, int nrb, int big) {
    return ldm_knob("LDM_GEMM_WG_GN", 0) != 0 && gemm_wg_gn_shape_ok(K, DHW, groups, nrb, big);
}
template <int MT, int NWV, bool GN>
static inline hipError_t launch_gemm_wg_t(const LightParams& p, int cout_pad, const WgGnParams& g, hipStream_t s) {
    constexpr int kmax = (16 * MT + 32 * NWV) * 2 * 512 <= 160 * 1024 ? 512 : 384;
    const int lds = (16 * MT + 32 * NWV) * 2 * p.K + (GN ? gemm_wg_gn_lds(p.K, g.groups) : 0);
    if (p.K > kmax || lds > 160 * 1024) return hipErrorInvalidValue;
    static bool attr_tab[32] = {}; bool& attr_set = attr_flag(attr_tab);   // per device
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_wg_kernel<MT, NWV, GN>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           GN ? 160 * 1024 : (16 * MT + 32 * NWV) * 2 * kmax);
        if (e != hipSuccess) return e;
        attr_set = true;
    }
    hipLaunchKernelGGL((gemm_wg_kernel<MT, NWV, GN>), dim3(p.mtiles * ((cout_pad + 32 * NWV - 1) / (32 * NWV))), dim3(64 * NWV), lds, s, p, cout_pad, g);
    return hipGetLastError();
}
// gn: the GroupNorm prologue (p.x = the un-normalised tensor; a shape gemm_wg_gn_shape_ok() admits), or null
static inline hipError_t launch_gemm_wg(const LightParams& p0, int cout_pad, int big, hipStream_t s, const WgGnParams* gn = nullptr) {
    LightParams p = p0;
    const WgGnParams g = gn ? *gn : WgGnParams{};
    if (big) {
        p.mtiles = (p.M + 63) / 64;
        if (p.K <= 384) return gn ? launch_gemm_wg_t<4, 4, true>(p, cout_pad, g, s) : launch_gemm_wg_t<4, 4, false>(p, cout_pad, g, s);
        return gn ? launch_gemm_wg_t<4, 2, true>(p, cout_pad, g, s) : launch_gemm_wg_t<4, 2, false>(p, cout_pad, g, s);
    }
    p.mtiles = (p.M + 31) / 32;
    return gn ? launch_gemm_wg_t<2, 2, true>(p, cout_pad, g, s) : launch_gemm_wg_t<2, 2, false>(p, cout_pad, g, s);
}
// the light GEMM of a plan op or an operator call: wg = gemm_wg_kernel (a shape gemm_wg_ok() admits), else gemm_light_kernel
static inline hipError_t launch_gemm_1x1(const LightParams& p, int cout_pad, int big, int wg, hipStream_t s) {
    return wg ? launch_gemm_wg(p, cout_pad, big, s) : launch_gemm_light(p, cout_pad, big, s);
}
