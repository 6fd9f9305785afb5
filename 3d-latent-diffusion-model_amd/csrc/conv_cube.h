// 3x3x3 stride-1 "same" convolution over a WHOLE small volume per workgroup (gfx950, bf16 MFMA 16x16x32): the UNet's 6^3 level.
//
// At 6^3 (216 voxels, 512 channels) conv3_halo_kernel needs 24 - 32 K splits to fill the chip: each workgroup runs 9 K steps behind the
// full halo prologue and stores a 126 x 128 fp32 tile, and fin_gn_kernel then streams 24 slabs back.  Here one workgroup owns
// (sample, 16-cout slice, 64-channel Cin chunk): it copies its 27 x 64 x 16 weights (54 KiB, the bytes that come from HBM, requested first)
// and the chunk's whole volume (a zero-padded image, 27 KiB of voxels) into LDS ONCE, then runs all 27 taps out of LDS behind one barrier.
// splits = Cin / 64 (8 instead of 24 at 512 channels), so the planar slabs fin_gn reads are 3x smaller.
//
// Image: [chunk 8][448 rows][16 B]: chunk-major, so the 16 rows one ds_read_b128 lane group touches are 16 DIFFERENT banks whenever the
// rows differ mod 16 -- true of any 16 consecutive image rows, whatever the tap shift.  Voxel (d, h, w) sits at row
// (d + 1) * 49 + (h + 1) * 7 + (w + 1) (plane pitch 49, row pitch 7: one zero column shared by the w = -1 and w = W borders of
// neighbouring lines, one zero line shared by h = -1 / h = H), so a tap is a constant row offset (kd * 49 + kh * 7 + kw from the
// (0, 0, 0) tap): an immediate in the ds_read, no border masks.  Zero rows come from out-of-range buffer offsets (LDS-DMA writes zeros).
// M order: the 16-row MFMA tiles walk the (d, h, w' < 7) domain -- consecutive image rows, including the pad column (computed, never
// stored): 16 tiles for 6^3 instead of 14, against 2 - 2.6x bank conflicts for a voxel-only order (offline count over the 27 taps).
// Waves: 4 (one per SIMD); wave w takes tiles 8 (w & 1) .. + 7 and the 32-channel K half (w >> 1) of every tap; the two K halves are
// added through LDS at the end (fixed order).  MFMA roles as conv_igemm.h: A = weights (rows = cout), B = voxels, so a lane holds 4
// consecutive couts of one voxel -> one 16-byte store into the planar slab (ConvParams::slab_lg) per tile.
// Fused 1x1 skip (ConvParams::steps1): its 64-channel chunks are dealt to the splits as conv3_halo_kernel does (per = ceil(steps1 / splits));
// a split's first skip chunk is copied with the main operands into an area of its own, further ones after the main loop.
// Deterministic: no atomics; per split the order is taps 0 .. 26 (K half 0 + K half 1), then the skip chunks.
// Measured on the 12^3 sibling (conv_plane.h, which began with this image): a chunk-major copy gathers 16 B from each of 64 cache lines
// and took in 36 GB/s per CU; row-major pieces (four neighbouring lanes per voxel row) 46 GB/s, at the price of 2-way conflicts on the
// fragment reads unless the chunks are XOR-swizzled by bit 2 of the row.  The same change is open here.
#pragma once
#include "conv_igemm.h"

constexpr int CUBE_EDGE = 6;                               // largest D / H / W
constexpr int CUBE_RP = 7, CUBE_PP = 49;                    // image pitches (rows) along h and d
constexpr int CUBE_ROWS = 448;                             // image rows per chunk (7 copies of 64); the last read row is 400
constexpr int CUBE_TILES = 16;                             // 16-row tiles over the (d, h, w' < 7) domain of a 6^3 volume
constexpr int CUBE_WOFF = 8 * CUBE_ROWS * 16;              // weights [tap][chunk][16 couts][16 B]
constexpr int CUBE_SOFF = CUBE_WOFF + 27 * 2048;           // skip voxels [chunk][256 domain rows][16 B]
constexpr int CUBE_SWOFF = CUBE_SOFF + 8 * 256 * 16;       // skip weights [chunk][16 couts][16 B]
constexpr int CUBE_LDS = CUBE_SWOFF + 2048;                // 147,456 B
static_assert(CUBE_LDS <= 160 * 1024, "LDS budget");
static_assert(CUBE_ROWS % 64 == 0 && CUBE_ROWS % 16 == 0, "whole LDS-DMA copies; chunk stride a multiple of 16 rows");

// s_waitcnt vmcnt(n) for a wave-uniform n known only at run time (0 .. 9 here)
__device__ __forceinline__ void cube_vm_wait(int n) {
    switch (n) {
    case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    case 8: asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); break;
    case 9: asm volatile("s_waitcnt vmcnt(9)" ::: "memory"); break;
    default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    }
}
__device__ __forceinline__ void cube_barrier() {             // LDS-only wait + raw barrier: copies in flight stay in flight
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// grid (splits = Cin / 64, CoutPad / 16, N), 256 threads.  Host side checks: D, H, W <= 6, c0a % 64 == 0, c1a / c1b % 64 == 0, x0b / x3 unused.
__global__ __launch_bounds__(256, 1) __attribute__((amdgpu_waves_per_eu(1, 1))) void conv3_cube_kernel(const ConvParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    typedef __attribute__((address_space(3))) void* lds_ptr_t;
    constexpr unsigned OOB = 0x80000000u;                   // beyond every descriptor's range: the copy writes zeros
    KSTAMP_BEGIN(12);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int split = blockIdx.x, n0 = blockIdx.y * 16, smp = blockIdx.z;
    const int D = p.Dout, H = p.Hout, W = p.Wout, DHW = D * H * W, dom = D * H * CUBE_RP;
    const unsigned cin2 = (unsigned)p.c0a * 2u, ci2 = (unsigned)split * 128u;

    // ---- copies: weights first (HBM), then the image of this Cin chunk, then the split's first skip chunk
    {
        __amdgpu_buffer_rsrc_t rs_w = __builtin_amdgcn_make_buffer_rsrc((void*)p.w0, 0, (int)(27u * (unsigned)p.CoutPad * cin2), 0x00020000);
        const int co = lane & 15, cq = lane >> 4;
        for (int u = wave; u < 54; u += 4) {               // copy u: tap u / 2, chunks 4 (u & 1) .. + 3, 16 couts
            const int tap = u >> 1, ch = (u & 1) * 4 + cq;
            const unsigned vo = (unsigned)(tap * p.CoutPad + n0 + co) * cin2 + ci2 + (unsigned)ch * 16u;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_w, (lds_ptr_t)(smem + CUBE_WOFF + u * 1024), 16, vo, 0, 0, 0);
        }
    }
    {
        const bf16_t* xs = p.x0a + (size_t)smp * DHW * p.c0a;
        __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc((void*)xs, 0, (int)((unsigned)DHW * cin2), 0x00020000);
        for (int v = wave; v < 8 * (CUBE_ROWS / 64); v += 4) {   // copy v: chunk v / 7, image rows 64 (v % 7) + lane
            const int ch = v / (CUBE_ROWS / 64), r = (v - ch * (CUBE_ROWS / 64)) * 64 + lane;
            const int dp = r / CUBE_PP, rem = r - dp * CUBE_PP, hp = rem / CUBE_RP, wp = rem - hp * CUBE_RP;
            const bool real = dp >= 1 && dp <= D && hp >= 1 && hp <= H && wp >= 1 && wp <= W;
            const unsigned vo = real ? (unsigned)(((dp - 1) * H + hp - 1) * W + wp - 1) * cin2 + ci2 + (unsigned)ch * 16u : OOB;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_x, (lds_ptr_t)(smem + ch * (CUBE_ROWS * 16) + (v - ch * (CUBE_ROWS / 64)) * 1024), 16, vo, 0, 0, 0);
        }
    }
    // skip chunks of this split: [j0, j1)
    int j0 = 0, j1 = 0;
    if (p.steps1 > 0) {
        const int per = (p.steps1 + p.splitk - 1) / p.splitk;
        j0 = split * per; j1 = j0 + per; if (j1 > p.steps1) j1 = p.steps1; if (j0 > j1) j0 = j1;
    }
    // a lane's skip row is domain row 64 * wave + lane in every chunk (copy v = 4 i + wave: chunk i, rows 64 wave .. + 63)
    unsigned s_vox = OOB;
    {
        const int q = wave * 64 + lane;
        if (q < dom) {
            const int d = q / (H * CUBE_RP), rem = q - d * H * CUBE_RP, h = rem / CUBE_RP, w = rem - h * CUBE_RP;
            if (w < W) s_vox = (unsigned)((d * H + h) * W + w);
        }
    }
    const int nca = p.c1a / 64;
    const unsigned w1row2 = (unsigned)(p.c1a + p.c1b) * 2u;
    auto issue_skip = [&](const int j) {
        const bool a = j < nca;
        const bf16_t* src = (a ? p.x1a : p.x1b) + (size_t)smp * DHW * (a ? p.c1a : p.c1b);
        const unsigned row2 = (unsigned)(a ? p.c1a : p.c1b) * 2u, jc = (unsigned)(a ? j : j - nca) * 128u;
        __amdgpu_buffer_rsrc_t rs_s = __builtin_amdgcn_make_buffer_rsrc((void*)src, 0, (int)((unsigned)DHW * row2), 0x00020000);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const unsigned vo = s_vox != OOB ? s_vox * row2 + jc + (unsigned)i * 16u : OOB;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_s, (lds_ptr_t)(smem + CUBE_SOFF + i * 4096 + wave * 1024), 16, vo, 0, 0, 0);
        }
        if (wave < 2) {                                      // weights: 16 couts x chunks 4 wave .. + 3
            __amdgpu_buffer_rsrc_t rs_1w = __builtin_amdgcn_make_buffer_rsrc((void*)p.w1, 0, (int)((unsigned)p.CoutPad * w1row2), 0x00020000);
            const unsigned vo = (unsigned)(n0 + (lane & 15)) * w1row2 + (unsigned)j * 128u + (unsigned)(wave * 4 + (lane >> 4)) * 16u;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_1w, (lds_ptr_t)(smem + CUBE_SWOFF + wave * 1024), 16, vo, 0, 0, 0);
        }
    };
    const bool has_skip = j1 > j0;
    if (has_skip) issue_skip(j0);
    const int skip_copies = 8 + (wave < 2 ? 1 : 0);

    // ---- fragment addressing (prologue work under the copies' round trip)
    const int mh = wave & 1, kh = wave >> 1;
    const int fr = lane & 15, ch = kh * 4 + (lane >> 4);     // this lane's 16-byte chunk of the 64-channel K step
    int abase[8];                                            // byte address of the (0, 0, 0) tap's row for each of the wave's tiles
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const int q = (mh * 8 + t) * 16 + fr;
        int row = 0;                                         // domain rows past the volume: zero rows, never stored
        if (q < dom) {
            const int d = q / (H * CUBE_RP), rem = q - d * H * CUBE_RP, h = rem / CUBE_RP, w = rem - h * CUBE_RP;
            row = d * CUBE_PP + h * CUBE_RP + w;
        }
        abase[t] = ch * (CUBE_ROWS * 16) + row * 16;
    }
    const int wbase = CUBE_WOFF + ch * 256 + fr * 16;
    f32x4 acc[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};

    cube_vm_wait(has_skip ? skip_copies : 0);                // this wave's weight and image copies have landed
    cube_barrier();                                          // ... and every other wave's
    KSTAMP(1);
    // ---- 27 taps out of LDS: fragments of tap k + 1 are read while tap k's MFMAs run
    bf16x8 wf[2], af[2][8];
    wf[0] = *reinterpret_cast<const bf16x8*>(smem + wbase);
#pragma unroll
    for (int t = 0; t < 8; ++t) af[0][t] = *reinterpret_cast<const bf16x8*>(smem + abase[t]);
#pragma unroll
    for (int tap = 0; tap < 27; ++tap) {
        const int cur = tap & 1, nxt = cur ^ 1;
        if (tap + 1 < 27) {
            const int k = tap + 1, off = ((k / 9) * CUBE_PP + ((k / 3) % 3) * CUBE_RP + k % 3) * 16;
            wf[nxt] = *reinterpret_cast<const bf16x8*>(smem + wbase + k * 2048);
#pragma unroll
            for (int t = 0; t < 8; ++t) af[nxt][t] = *reinterpret_cast<const bf16x8*>(smem + abase[t] + off);
        }
#pragma unroll
        for (int t = 0; t < 8; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[cur], af[cur][t], acc[t], 0, 0, 0);
        // one fragment read of tap k + 1 in the shadow of each MFMA of tap k (left alone, the scheduler serialised read -> wait -> MFMA)
#pragma unroll
        for (int t = 0; t < 8; ++t) { __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); __builtin_amdgcn_sched_group_barrier(0x100, 1, 0); }
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
    }
    // ---- the split's share of the fused 1x1 skip (centre tap = domain row itself)
    for (int j = j0; j < j1; ++j) {
        if (j > j0) { cube_barrier(); issue_skip(j); }       // every wave is done with the previous chunk's fragments
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        cube_barrier();
        const bf16x8 sw = *reinterpret_cast<const bf16x8*>(smem + CUBE_SWOFF + ch * 256 + fr * 16);
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const bf16x8 sa = *reinterpret_cast<const bf16x8*>(smem + CUBE_SOFF + ch * 4096 + ((mh * 8 + t) * 16 + fr) * 16);
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(sw, sa, acc[t], 0, 0, 0);
        }
    }
    KSTAMP(2);
    // ---- K half 1 -> LDS (the image area is free once every wave is past its last fragment read), K half 0 adds it and stores
    cube_barrier();
    float4* xch = reinterpret_cast<float4*>(smem);
    if (kh == 1) {
#pragma unroll
        for (int t = 0; t < 8; ++t) xch[(mh * 8 + t) * 64 + lane] = make_float4(acc[t][0], acc[t][1], acc[t][2], acc[t][3]);
    }
    cube_barrier();
    if (kh == 0) {
        const int c = n0 + 4 * (lane >> 4);
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const int q = (mh * 8 + t) * 16 + fr;
            if (q >= dom) continue;
            const int d = q / (H * CUBE_RP), rem = q - d * H * CUBE_RP, h = rem / CUBE_RP, w = rem - h * CUBE_RP;
            if (w >= W) continue;
            const float4 o = xch[(mh * 8 + t) * 64 + lane];
            const int m = smp * DHW + (d * H + h) * W + w;
            *reinterpret_cast<float4*>(slab_ptr(p.partial, split, p.M, p.CoutPad, p.slab_lg, m, c)) =
                make_float4(acc[t][0] + o.x, acc[t][1] + o.y, acc[t][2] + o.z, acc[t][3] + o.w);
        }
    }
    KSTAMP_DRAIN(3);
#endif  // __HIP_DEVICE_COMPILE__
}
