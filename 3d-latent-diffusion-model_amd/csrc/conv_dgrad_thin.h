// Data gradient of a 3x3x3 stride-1 pad-1 convolution with a THIN input (1 .. 32 real channels): the UNet's conv_in, whose input is the
// packed (x | cond) tensor.  dx[ci](v) = sum_tap sum_co dy[co](v + 1 - tap) w[tap][co][ci]: the same convolution over dy with mirrored taps
// and transposed weights, so the kernel is conv3_thin_kernel's (conv_thin.h) with the roles turned: a workgroup owns a 4 x 4 x 16 block of
// dx voxels, copies the 6 x 6 x 18 halo of dy into LDS once per 32-channel chunk (41 KB, three workgroups per CU) and reads every voxel row
// 27 times from there.  MFMA 16x16x32 with the dx channels on the A side: one 16-row tile for up to 16 real channels, two for up to 32 (twice
// the accumulators, the same LDS).  The A fragments (one 16-byte load per lane, tap and row tile) come straight from the packed weights in
// global memory, [27 mirrored taps][32 rows][K] bf16: 27 x 32 x K x 2 bytes stay in L2, and the load of tap + 1 is issued before the MFMAs
// of tap, so no weight copy takes LDS that the second row tile would double.
// Output: fp32 NCDHW, split over two destinations: rows [0, cx) -> dx [N][cx][DHW], rows [cx, cx + cc) -> dcond [N][cc][DHW] (the inverse of
// the input packing's concat); a null destination's rows are not stored, rows past cx + cc never are.  No bias.
// bf16 operands, fp32 accumulation; or the fp32 precision mode as the 3 x bf16 product: dy = the (hi | lo) split [..][2 C] bf16 against
// weights [hi | lo | hi] (K = 3 C), chunk c of the weights meeting chunk c (hi), c - C (hi again) or c - C (lo) of a voxel row (conv_thin.h's
// x3_c mapping).  C % 32 == 0, any D / H / W (ragged blocks are bounds-checked on the loads and on the stores).
#pragma once
#include "common.h"
#include "conv_thin.h"

struct DgradThinParams {
    const bf16_t* dy; const bf16_t* w;     // dy [N][D][H][W][C] (x3: [..][2 C]); w packed [27][32][K], K = C (x3: 3 C), rows >= the real count zero
    float* dx; float* dcond;               // fp32 [N][cx][DHW], [N][cc][DHW]; either may be null
    int N, D, H, W, K, cx, cc;
    int td, th, tw;                        // blocks per dimension
    int x3_c;                              // 0, or the channel count C of the fp32 mode
};

// What the kernel reads: wp[tap'][row][k] = w(co = k, ci = row, tap = 26 - tap') for row < cin_real and k < cout, else 0.  The source is
// addressed by strides (elements): the conv's own [Cout][Cin][27] tensor (27 Cin, 27, 1) or the packed arenas' [27][cout_pad][cin_s]
// (cin_s, 1, cout_pad cin_s).  x3: k runs over [hi(C) | lo(C) | hi(C)] of the fp32 source (C = K / 3).
template <typename T>
__global__ __launch_bounds__(256) void dgrad_thin_pack_kernel(const T* __restrict__ w, bf16_t* __restrict__ wp, int cout, int cin_real, int K, int x3,
                                                              long s_co, long s_ci, long s_tap) {
    const int C = x3 ? K / 3 : K;
    const long total = 27L * 32 * K;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const int k = (int)(e % K); const int row = (int)((e / K) & 31); const int tap = (int)(e / (32L * K));
        const int part = k / C, co = k - part * C;
        float v = 0.f;
        if (row < cin_real && co < cout) {
            const T* src = w + co * s_co + row * s_ci + (26 - tap) * s_tap;
            if constexpr (sizeof(T) == 2) v = bf2f(*src); else v = *src;
        }
        bf16_t o = f2bf(v);
        if (x3 && part == 1) o = f2bf(v - bf2f(o));
        wp[e] = o;
    }
}

template <int RT>
__global__ __launch_bounds__(256) void conv3_dgrad_thin_kernel(const DgradThinParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* sx = smem;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fg = lane >> 4;
    int b = blockIdx.x;
    const int bw = b % p.tw; b /= p.tw; const int bh = b % p.th; b /= p.th; const int bd = b % p.td; const int n = b / p.td;
    const int d0 = bd * THIN_TD, h0 = bh * THIN_TH, w0 = bw * THIN_TW;
    const size_t xn = (size_t)n * p.D * p.H * p.W;
    const int xstride = p.x3_c ? 2 * p.x3_c : p.K;     // channels per voxel row of dy
    // MFMA column fr <-> voxel w0 + wm: conv_thin.h's conflict-free column order under the (hv >> 2) & 3 slot swizzle
    const int wm = fr < 4 ? 2 * fr : fr < 12 ? 2 * (fr - 4) + 1 : 2 * (fr - 8);
    f32x4 acc[RT][4];
#pragma unroll
    for (int r = 0; r < RT; ++r)
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[r][t] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const u32x4 zero = {0u, 0u, 0u, 0u};
    // this lane's A fragment of (tap, row tile r): 8 consecutive k of row 16 r + fr
    const bf16_t* wl = p.w + (size_t)fr * p.K + fg * 8;
    const size_t wtile = (size_t)16 * p.K, wtap = (size_t)32 * p.K;
    for (int c0 = 0; c0 < p.K; c0 += THIN_CK) {
        __syncthreads();                                  // the previous chunk's reads are done
        const int xc0 = (p.x3_c && c0 >= p.x3_c) ? c0 - p.x3_c : c0;       // channel offset of this chunk inside a voxel row
        constexpr int NIT = (THIN_HV * THIN_NC + 255) / 256;
        u32x4 hv_v[NIT];
#pragma unroll
        for (int k = 0; k < NIT; ++k) {
            const int e = tid + k * 256;
            const int hv = e / THIN_NC, c16 = e % THIN_NC;
            const int wx = hv % THIN_HW, r = hv / THIN_HW, hy = r % THIN_HH, dz = r / THIN_HH;
            const int gd = d0 - 1 + dz, gh = h0 - 1 + hy, gw = w0 - 1 + wx;
            hv_v[k] = zero;
            if (e < THIN_HV * THIN_NC && (unsigned)gd < (unsigned)p.D && (unsigned)gh < (unsigned)p.H && (unsigned)gw < (unsigned)p.W)
                hv_v[k] = *reinterpret_cast<const u32x4*>(p.dy + (xn + ((size_t)gd * p.H + gh) * p.W + gw) * xstride + xc0 + c16 * 8);
        }
        u32x4 wv[RT];                                     // tap 0's fragments travel under the halo copy
#pragma unroll
        for (int r = 0; r < RT; ++r) wv[r] = *reinterpret_cast<const u32x4*>(wl + r * wtile + c0);
#pragma unroll
        for (int k = 0; k < NIT; ++k) {
            const int e = tid + k * 256;
            const int hv = e / THIN_NC, c16 = e % THIN_NC;
            if (e < THIN_HV * THIN_NC) *reinterpret_cast<u32x4*>(sx + hv * THIN_RB + ((c16 ^ ((hv >> 2) & (THIN_NC - 1))) << 4)) = hv_v[k];
        }
        __syncthreads();
#pragma unroll 1
        for (int tap = 0; tap < 27; ++tap) {
            const int kd = tap / 9, kh = (tap / 3) % 3, kw = tap % 3;
            bf16x8 wf[RT];
#pragma unroll
            for (int r = 0; r < RT; ++r) wf[r] = *reinterpret_cast<const bf16x8*>(&wv[r]);
            const int nt = tap < 26 ? tap + 1 : 26;       // the next tap's fragments (the last tap re-reads its own: no branch, in bounds)
#pragma unroll
            for (int r = 0; r < RT; ++r) wv[r] = *reinterpret_cast<const u32x4*>(wl + nt * wtap + r * wtile + c0);
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int hv = ((wave + kd) * THIN_HH + (t + kh)) * THIN_HW + wm + kw;
                const bf16x8 xf = *reinterpret_cast<const bf16x8*>(sx + hv * THIN_RB + ((fg ^ ((hv >> 2) & (THIN_NC - 1))) << 4));
#pragma unroll
                for (int r = 0; r < RT; ++r) acc[r][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[r], xf, acc[r][t], 0, 0, 0);
            }
        }
    }
    // accumulator row 4 fg + i of tile r = channel 16 r + 4 fg + i, column fr = voxel
    const int gd = d0 + wave, gw = w0 + wm;
    if (gd >= p.D || gw >= p.W) return;
    const size_t dhw = (size_t)p.D * p.H * p.W;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int gh = h0 + t;
        if (gh >= p.H) continue;
        const size_t sp = ((size_t)gd * p.H + gh) * p.W + gw;
#pragma unroll
        for (int r = 0; r < RT; ++r)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int ch = 16 * r + 4 * fg + i;
                if (ch < p.cx) { if (p.dx) p.dx[((size_t)n * p.cx + ch) * dhw + sp] = acc[r][t][i]; }
                else if (ch < p.cx + p.cc) { if (p.dcond) p.dcond[((size_t)n * p.cc + (ch - p.cx)) * dhw + sp] = acc[r][t][i]; }
            }
    }
#endif
}
