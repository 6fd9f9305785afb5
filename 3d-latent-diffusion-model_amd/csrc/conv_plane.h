// 3x3x3 stride-1 "same" convolution of a volume of at most 12^3, UNSPLIT: one output z-plane per workgroup (gfx950, bf16 MFMA 16x16x32): the
// UNet's 12^3 level.
//
// At 12^3 (1728 voxels, 256 output channels) conv3_halo_kernel splits K 8 - 9 ways to fill the chip: every workgroup stores a 126 x 128
// fp32 tile (15.9 MB of slabs for 0.9 MB of output), splitk_finalize_kernel reads them back.  Here one workgroup owns (sample, output
// plane d, 16-cout slice) over the WHOLE K range: no slabs, no finalize, the epilogue (bias, time-embedding row, residual, bf16 store,
// GroupNorm partials) in the kernel.  grid (CoutPad / 16, D, N) = 192 workgroups for the benchmark's convs, 8 waves, 126 KiB of LDS.
//
// K walk: Cin in 32-channel stages (one MFMA K step per tap), double buffered: the LDS-DMA copies of stage s + 1 are in flight while the
// 27 taps of stage s run out of LDS; one barrier per stage.  A stage is the image of planes d - 1 .. d + 1 (576 rows x 64 B = 36,864 B)
// and the 27 x 16 x 32 weights ([tap][16 couts][64 B] = 27,648 B).
// Image: ROW-major [row][chunk 4][16 B], voxel (plane pl, h, w) at row pl * PP + (h + 1) * RP + (w + 1) with RP = W + 1 and PP =
// (H + 1) * RP (the pitches of conv_cube.h): one zero column / line shared by neighbouring borders, a tap is the constant row offset
// kd * PP + kh * RP + kw, no border masks; zero rows (and planes outside the volume) come from out-of-range buffer offsets (LDS-DMA writes
// zeros).  Row-major because of the copies: four neighbouring lanes fetch the 64 contiguous bytes of one voxel row.  The chunk-major image
// of conv_cube.h (a lane per row: 64 cache lines per 1 KiB copy) was built first and took in 36 GB/s per CU, 1.8 us per stage, whoever
// issued the copies.  The price: a B-fragment read (16 rows x 2 chunks per lane group) is a 2-way bank conflict at every tap shift; the
// XOR swizzle that removes it (chunk ^ 2 * bit 2 of the row: conflict-free at every shift, checked by enumeration) makes the address
// non-linear in the tap offset and is not built; the weights, whose rows never shift, carry it.
// M domain: H x (W + 1) image rows (156 at 12^3 = ten 16-row MFMA tiles; the pad column is computed and never stored); the largest row
// read is 159 + 2 * 169 + 2 * 13 + 2 = 525 < 576.
// Waves: 8 = two per SIMD.  Waves 4 .. 7 only issue copies (a 1 KiB piece costs its issuing wave 100+ cycles), waves
// 0 .. 3 only multiply: wave w takes tiles 5 (w & 1) .. + 4 and the taps 0 .. 13 (w >> 1 == 0) or 14 .. 26; the two tap halves are added
// through LDS at the end in a fixed order.  (A 32-channel stage is ONE K step, so K cannot be halved by channels.)  MFMA roles as
// conv_cube.h: A = weights (rows = cout), B = voxels: a lane holds 4 consecutive couts of one voxel -> one 8-byte bf16 store.
// Fused 1x1 skip (ConvParams::steps1 = 64-channel chunks of (x1a | x1b)): extra stages behind the taps, two 64-channel chunks per stage
// (the skip reads the centre plane only: [chunk 8][192 domain rows][16 B] per 64 channels, so 128 channels fit a stage buffer and the
// per-stage barrier + copy round trip is paid 6 times for 768 channels, not 24); wave w takes K step (w >> 1) of each chunk.
// Epilogue: the rounding points of conv3_halo_kernel's unsplit epilogue: fp32 sum + (bias + bias2) + time-embedding row + residual ->
// bf16 -> NDHWC; GroupNorm partials (sum, sum of squares of the ROUNDED values) as one slab row per plane (stats_nrb = D).
// Deterministic: no atomics; order = stages 0 .., taps ascending within a half, half 0 + half 1, tiles 0 .. 4, lanes by DPP, wave 0 + wave 1.
#pragma once
#include <type_traits>
#include "conv_cube.h"

constexpr int PLANE_EDGE = 12;                              // largest D / H / W
constexpr int PLANE_ROWS = 576;                             // image rows (36 copies of 16 rows x 64 B)
constexpr int PLANE_TILES = 10;                             // 16-row tiles over the (h, w' < W + 1) domain of a 12 x 12 plane
constexpr int PLANE_IMG = PLANE_ROWS * 64;                  // a stage's image; its weights [tap][16 couts][chunk 4, swizzled][16 B] follow
constexpr int PLANE_STAGE = PLANE_IMG + 27 * 1024;          // 64,512 B
constexpr int PLANE_SROWS = 192;                            // skip stage: [unit 2][chunk 8][192 domain rows][16 B] ...
constexpr int PLANE_SUNIT = 8 * PLANE_SROWS * 16;
constexpr int PLANE_SWOFF = 2 * PLANE_SUNIT;                // ... then its weights [unit 2][chunk 8][16 couts][16 B]
constexpr int PLANE_RED = 16384;                            // end of kernel: tap-half exchange at 0 (10 KiB), statistics fold here
constexpr int PLANE_LDS = 2 * PLANE_STAGE;                  // 129,024 B
static_assert(PLANE_LDS <= 160 * 1024, "LDS budget");
static_assert(PLANE_ROWS % 64 == 0 && PLANE_SROWS % 64 == 0, "whole LDS-DMA copies; chunk strides a multiple of 16 rows");
static_assert(PLANE_TILES * 16 >= PLANE_EDGE * (PLANE_EDGE + 1), "tiles cover the domain");
static_assert(PLANE_TILES * 16 - 1 + 2 * (PLANE_EDGE + 1) * (PLANE_EDGE + 1) + 2 * (PLANE_EDGE + 1) + 2 < PLANE_ROWS, "largest row read");
static_assert(PLANE_TILES * 16 <= PLANE_SROWS && PLANE_SWOFF + 2 * 2048 <= PLANE_STAGE, "skip stage fits a stage buffer");
static_assert(PLANE_TILES * 1024 <= PLANE_RED && PLANE_RED + 256 <= PLANE_LDS, "end-of-kernel areas");

// grid (CoutPad / 16, D, N), 512 threads.  Host side checks (launch_conv_plane): D, H, W <= 12, c0a % 64 == 0, c1a / c1b % 64 == 0, bf16
// NDHWC output, x0b / x3 unused, splitk 1.
__global__ __launch_bounds__(512, 1) __attribute__((amdgpu_waves_per_eu(2, 2))) void conv3_plane_kernel(const ConvParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    typedef __attribute__((address_space(3))) void* lds_ptr_t;
    constexpr unsigned OOB = 0x80000000u;                   // beyond every descriptor's range: the copy writes zeros
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave8 = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool loader = wave8 >= 4;                          // waves 4 .. 7 issue every copy, waves 0 .. 3 run the MFMAs
    const int wave = wave8 & 3;                              // copy share of a loader wave / tile and tap share of an MFMA wave
    const int n0 = blockIdx.x * 16, d = blockIdx.y, smp = blockIdx.z;
    if (n0 >= p.CoutS) return;                              // a slice of padding couts only (CoutS % 32 == 0): nothing to store
    const int D = p.Dout, H = p.Hout, W = p.Wout, DHW = D * H * W, RP = W + 1, PP = (H + 1) * RP, dom = H * RP;
    const unsigned cin2 = (unsigned)p.c0a * 2u;
    const int nst0 = p.c0a >> 5, units = p.steps1, nst = nst0 + ((units + 1) >> 1);

    // ---- copy addressing.  Image: loader wave w copies the 16-row pieces w, w + 4, .. of every stage: four neighbouring lanes fetch the four
    //      16-byte chunks of ONE voxel row (64 contiguous bytes; a lane per row and chunk-major pieces gathered 64 cache lines per copy and
    //      ran at 36 GB/s per CU); weights: taps w, w + 4, .., four lanes per cout row, chunks XOR-swizzled by bit 2 of the row so that the
    //      A-fragment reads stay conflict-free
    const bf16_t* xs = p.x0a + (size_t)smp * DHW * p.c0a;
    __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc((void*)xs, 0, (int)((unsigned)DHW * cin2), 0x00020000);
    __amdgpu_buffer_rsrc_t rs_w = __builtin_amdgcn_make_buffer_rsrc((void*)p.w0, 0, (int)(27u * (unsigned)p.CoutPad * cin2), 0x00020000);
    unsigned vo[PLANE_ROWS / 64];
#pragma unroll
    for (int i = 0; i < PLANE_ROWS / 64; ++i) {
        const int r = (wave + 4 * i) * 16 + (lane >> 2);
        const int pl = r / PP, rem = r - pl * PP, hp = rem / RP, wp = rem - hp * RP, dd = d - 1 + pl;
        const bool real = pl <= 2 && dd >= 0 && dd < D && hp >= 1 && wp >= 1;
        vo[i] = real ? (unsigned)((dd * H + hp - 1) * W + wp - 1) * cin2 + (unsigned)(lane & 3) * 16u : OOB;
    }
    const unsigned wv = (unsigned)(wave * p.CoutPad + n0 + (lane >> 2)) * cin2 + (unsigned)((lane & 3) ^ ((lane >> 3) & 2)) * 16u;
    const unsigned wstep = 4u * (unsigned)p.CoutPad * cin2;
    auto issue_main = [&](const int s, const int b) {
        char* buf = smem + b * PLANE_STAGE;
        const unsigned so = (unsigned)s * 64u;
#pragma unroll
        for (int i = 0; i < 7; ++i) {
            const int tap = wave + 4 * i;
            if (tap < 27) __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_w, (lds_ptr_t)(buf + PLANE_IMG + tap * 1024), 16, wv + (unsigned)i * wstep + so, 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < PLANE_ROWS / 64; ++i)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_x, (lds_ptr_t)(buf + (wave + 4 * i) * 1024), 16, vo[i] + so, 0, 0, 0);
    };
    // fused 1x1 skip: a lane's row in copy g is domain row 64 g + lane of the centre plane
    unsigned s_vox[PLANE_SROWS / 64];
#pragma unroll
    for (int g = 0; g < PLANE_SROWS / 64; ++g) {
        const int q = g * 64 + lane;
        s_vox[g] = OOB;
        if (q < dom) {
            const int h = q / RP, w = q - h * RP;
            if (w < W) s_vox[g] = (unsigned)((d * H + h) * W + w);
        }
    }
    const int nca = p.c1a / 64;
    const unsigned w1row2 = (unsigned)(p.c1a + p.c1b) * 2u;
    auto issue_skip = [&](const int j, const int b) {         // skip stage j: 64-channel chunks 2 j and 2 j + 1 of (x1a | x1b)
        char* buf = smem + b * PLANE_STAGE;
#pragma unroll
        for (int ul = 0; ul < 2; ++ul) {
            const int u = 2 * j + ul;
            if (u >= units) break;
            const bool a = u < nca;
            const bf16_t* src = (a ? p.x1a : p.x1b) + (size_t)smp * DHW * (a ? p.c1a : p.c1b);
            const unsigned row2 = (unsigned)(a ? p.c1a : p.c1b) * 2u, jc = (unsigned)(a ? u : u - nca) * 128u;
            __amdgpu_buffer_rsrc_t rs_s = __builtin_amdgcn_make_buffer_rsrc((void*)src, 0, (int)((unsigned)DHW * row2), 0x00020000);
#pragma unroll
            for (int i = 0; i < 2 * (PLANE_SROWS / 64); ++i) {
                const int ch = wave + 4 * (i & 1), g = i >> 1;
                const unsigned v = s_vox[g] != OOB ? s_vox[g] * row2 + jc + (unsigned)ch * 16u : OOB;
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_s, (lds_ptr_t)(buf + ul * PLANE_SUNIT + ch * (PLANE_SROWS * 16) + g * 1024), 16, v, 0, 0, 0);
            }
            if ((wave >> 1) == ul) {                         // weights: 16 couts x chunks 4 (wave & 1) .. + 3
                const int hf = wave & 1;
                __amdgpu_buffer_rsrc_t rs_1w = __builtin_amdgcn_make_buffer_rsrc((void*)p.w1, 0, (int)((unsigned)p.CoutPad * w1row2), 0x00020000);
                const unsigned v = (unsigned)(n0 + (lane & 15)) * w1row2 + (unsigned)u * 128u + (unsigned)(hf * 4 + (lane >> 4)) * 16u;
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_1w, (lds_ptr_t)(buf + PLANE_SWOFF + ul * 2048 + hf * 1024), 16, v, 0, 0, 0);
            }
        }
    };
    auto issue = [&](const int s) { if (s < nst0) issue_main(s, s & 1); else issue_skip(s - nst0, s & 1); };
    if (loader) issue(0);

    // ---- fragment addressing (under the first copies' round trip)
    const int mh = wave & 1, kh = wave >> 1;
    const int fr = lane & 15, kq = lane >> 4;                // voxel column / cout row of the fragment, 16-byte chunk of the K step
    // byte offset of the (kd, kh, 0) tap's row for each of the wave's tiles: with kw and the buffer as immediates of the ds_read, the
    // tap loop has no address arithmetic (with it the scheduler sank every fragment read to just in front of its MFMA)
    int abase[9][5];
#pragma unroll
    for (int t = 0; t < 5; ++t) {
        const int q = (mh * 5 + t) * 16 + fr;
        const int a0 = kq * 16 + (q < dom ? q : 0) * 64;                 // domain rows past the plane: never stored
#pragma unroll
        for (int j = 0; j < 9; ++j) abase[j][t] = a0 + ((j / 3) * PP + (j % 3) * RP) * 64;
    }
    const int wbase = PLANE_IMG + fr * 64 + (kq ^ ((fr >> 1) & 2)) * 16;
    f32x4 acc[5];
#pragma unroll
    for (int t = 0; t < 5; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // taps [T0, T1) of the stage in the buffer at byte offset bo: fragments of tap k + 1 are read while tap k's MFMAs run
    auto taps = [&](auto boc, auto t0c, auto t1c) {
        constexpr int BO = decltype(boc)::value, T0 = decltype(t0c)::value, T1 = decltype(t1c)::value;
        bf16x8 wf[2], af[2][5];
        wf[0] = *reinterpret_cast<const bf16x8*>(smem + wbase + (BO + T0 * 1024));
#pragma unroll
        for (int t = 0; t < 5; ++t) af[0][t] = *reinterpret_cast<const bf16x8*>(smem + abase[T0 / 3][t] + (BO + (T0 % 3) * 64));
#pragma unroll
        for (int k = T0; k < T1; ++k) {
            const int cur = (k - T0) & 1, nxt = cur ^ 1;
            if (k + 1 < T1) {
                const int k1 = k + 1;
                wf[nxt] = *reinterpret_cast<const bf16x8*>(smem + wbase + (BO + k1 * 1024));
#pragma unroll
                for (int t = 0; t < 5; ++t) af[nxt][t] = *reinterpret_cast<const bf16x8*>(smem + abase[k1 / 3][t] + (BO + (k1 % 3) * 64));
            }
#pragma unroll
            for (int t = 0; t < 5; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[cur], af[cur][t], acc[t], 0, 0, 0);
            // one fragment read of tap k + 1 in the shadow of each MFMA of tap k (as conv3_cube_kernel)
#pragma unroll
            for (int t = 0; t < 5; ++t) { __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); __builtin_amdgcn_sched_group_barrier(0x100, 1, 0); }
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
            // ... and nothing crosses a tap: left free, the scheduler ran the taps of ONE tile back to back (a dependent MFMA chain, every
            // fragment read waited for in front of its MFMA)
            __builtin_amdgcn_sched_barrier(0);
        }
    };

    for (int s = 0; s < nst; ++s) {
        if (loader) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // this wave's copies of stage s have landed
        cube_barrier();                                      // ... every loader's, and every MFMA wave is past its reads of stage s - 1
        if (loader) {
            if (s + 1 < nst) issue(s + 1);                   // into the buffer stage s - 1 used
            continue;
        }
        const int bo = (s & 1) * PLANE_STAGE;
        if (s < nst0) {
            typedef std::integral_constant<int, 0> B0; typedef std::integral_constant<int, PLANE_STAGE> B1;
            typedef std::integral_constant<int, 14> T14; typedef std::integral_constant<int, 27> T27;
            if (kh == 0) { if (s & 1) taps(B1{}, B0{}, T14{}); else taps(B0{}, B0{}, T14{}); }
            else { if (s & 1) taps(B1{}, T14{}, T27{}); else taps(B0{}, T14{}, T27{}); }
        } else {                                             // skip stage: K step kh of each 64-channel chunk, the domain row itself
            const int nu = units - 2 * (s - nst0) < 2 ? units - 2 * (s - nst0) : 2;
            for (int ul = 0; ul < nu; ++ul) {
                const int ch = kh * 4 + kq;
                const bf16x8 sw = *reinterpret_cast<const bf16x8*>(smem + bo + PLANE_SWOFF + ul * 2048 + ch * 256 + fr * 16);
#pragma unroll
                for (int t = 0; t < 5; ++t) {
                    const bf16x8 sa = *reinterpret_cast<const bf16x8*>(smem + bo + ul * PLANE_SUNIT + ch * (PLANE_SROWS * 16) + ((mh * 5 + t) * 16 + fr) * 16);
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(sw, sa, acc[t], 0, 0, 0);
                }
            }
        }
    }

    // ---- tap half 1 -> LDS (the buffers are free once every wave is past its last fragment read), tap half 0 adds it and runs the epilogue
    const int c = n0 + 4 * kq;                               // this lane's 4 couts
    float4 eb = make_float4(0.f, 0.f, 0.f, 0.f), et = eb;
    if (kh == 0 && !loader) {                                // epilogue operands, requested ahead of the exchange
        if (p.bias) eb = *reinterpret_cast<const float4*>(p.bias + c);
        if (p.bias2) { const float4 b2 = *reinterpret_cast<const float4*>(p.bias2 + c); eb.x += b2.x; eb.y += b2.y; eb.z += b2.z; eb.w += b2.w; }
        if (p.temb) et = *reinterpret_cast<const float4*>(p.temb + (size_t)smp * p.temb_stride + c);
    }
    cube_barrier();
    float4* xch = reinterpret_cast<float4*>(smem);
    if (kh == 1 && !loader) {
#pragma unroll
        for (int t = 0; t < 5; ++t) xch[(mh * 5 + t) * 64 + lane] = make_float4(acc[t][0], acc[t][1], acc[t][2], acc[t][3]);
    }
    cube_barrier();
    float ssum[4] = {0.f, 0.f, 0.f, 0.f}, ssq[4] = {0.f, 0.f, 0.f, 0.f};
    if (kh == 0 && !loader) {
#pragma unroll
        for (int t = 0; t < 5; ++t) {
            const int q = (mh * 5 + t) * 16 + fr;
            if (q >= dom) continue;
            const int h = q / RP, w = q - h * RP;
            if (w >= W) continue;
            const float4 o = xch[(mh * 5 + t) * 64 + lane];
            float v[4] = {acc[t][0] + o.x, acc[t][1] + o.y, acc[t][2] + o.z, acc[t][3] + o.w};
            if (p.bias || p.bias2) { v[0] += eb.x; v[1] += eb.y; v[2] += eb.z; v[3] += eb.w; }
            if (p.temb) { v[0] += et.x; v[1] += et.y; v[2] += et.z; v[3] += et.w; }
            const size_t m = (size_t)smp * DHW + (size_t)((d * H + h) * W + w);
            if (p.residual) {
                const u32x2 rv = *reinterpret_cast<const u32x2*>(p.residual + m * p.CoutS + c);
                v[0] += __uint_as_float(rv[0] << 16); v[1] += __uint_as_float(rv[0] & 0xffff0000u);
                v[2] += __uint_as_float(rv[1] << 16); v[3] += __uint_as_float(rv[1] & 0xffff0000u);
            }
            u32x2 ov;
            ov[0] = pack2bf(v[0], v[1]); ov[1] = pack2bf(v[2], v[3]);
#pragma unroll
            for (int i = 0; i < 2; ++i) {                    // statistics of the values as stored
                const float lo = __uint_as_float(ov[i] << 16), hi = __uint_as_float(ov[i] & 0xffff0000u);
                ssum[2 * i] += lo; ssq[2 * i] += lo * lo; ssum[2 * i + 1] += hi; ssq[2 * i + 1] += hi * hi;
            }
            *reinterpret_cast<u32x2*>(p.out + m * p.CoutS + c) = ov;
        }
    }
    if (p.stats) {                                           // one slab row per (sample, plane): [N * D][CoutS][2]
        float* red = reinterpret_cast<float*>(smem + PLANE_RED);         // [mh 2][16 couts][2]
        if (kh == 0 && !loader) {
#define PLANE_ROW_ADD(X, CTRL) X += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(X), CTRL, 0xf, 0xf, true))
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                PLANE_ROW_ADD(ssum[r], 0x128); PLANE_ROW_ADD(ssum[r], 0x124); PLANE_ROW_ADD(ssum[r], 0x122); PLANE_ROW_ADD(ssum[r], 0x121);
                PLANE_ROW_ADD(ssq[r], 0x128); PLANE_ROW_ADD(ssq[r], 0x124); PLANE_ROW_ADD(ssq[r], 0x122); PLANE_ROW_ADD(ssq[r], 0x121);
            }
#undef PLANE_ROW_ADD
            if (fr == 0) {
#pragma unroll
                for (int r = 0; r < 4; ++r) { red[(mh * 16 + 4 * kq + r) * 2] = ssum[r]; red[(mh * 16 + 4 * kq + r) * 2 + 1] = ssq[r]; }
            }
        }
        cube_barrier();
        if (tid < 16)
            *reinterpret_cast<float2*>(p.stats + (((size_t)smp * D + d) * p.CoutS + n0 + tid) * 2) =
                make_float2(red[tid * 2] + red[(16 + tid) * 2], red[tid * 2 + 1] + red[(16 + tid) * 2 + 1]);
    }
#endif  // __HIP_DEVICE_COMPILE__
}
